"""The tracker's constant-velocity motion model on the host: pipeline.track_heads_host(motion=...), the numpy twin of mcg_track_heads_motion
(include/mcgaze_hip.h, "head identities with a constant-velocity motion model"), and the surface around it.  Every comparison is exact --
floats as their int32 patterns; there is no tolerance anywhere.

1. the scenario the model exists for, worked by hand (tests/track_motion_cases.py): a walking person missed for three frames
2. gain = 0 is the plain tracker, on every case of tests/track_cases.py
3. T frames in one call = T calls of one frame, tables, state boxes and state
4. the edge rules: a rebirth at rest, overflowing predictions and updates, bad rows and counts, a -0.0 at rest
5. the state passes between the two forms; the plain one leaves the velocity words alone
6. exports, header, binding; argument errors of the entry (refused before any launch: no device is needed) and of the Python layers
"""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from mcgaze_amd import harness, live
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from mcgaze_amd.head_detect import TRACK_HEADER_WORDS, TRACK_SLOT_WORDS
from tests import track_cases as TC
from tests import track_motion_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('slot_boxes', 'image_of', 'track_id', 'age', 'det_of', 'flags', 'state', 'state_boxes')
F = np.float32


def same(got, want, what='', n=8):
    assert len(got) >= n and len(want) >= n
    for g, w, name in zip(got[:n], want[:n], NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(np.ascontiguousarray(g).view(np.int32), np.ascontiguousarray(w).view(np.int32)), (what, name)


def velocity(state, s=0, q=0):
    """(vx, vy) of slot s as the state holds it."""
    at = TRACK_HEADER_WORDS + TRACK_SLOT_WORDS * s + 6
    return np.ascontiguousarray(state[q, at:at + 2]).view(F).tolist()


def slot_box(state, s=0, q=0):
    at = TRACK_HEADER_WORDS + TRACK_SLOT_WORDS * s
    return np.ascontiguousarray(state[q, at:at + 4]).view(F)


@pytest.fixture(scope='module')
def results():
    return {name: P.track_heads_host(boxes, counts, **opts) for name, (boxes, counts, opts) in MC.ALL.items()}


def velocities_per_frame(boxes, counts, opts):
    """Slot 0's velocity after every frame, from T calls of one frame."""
    state, out = None, []
    for t in range(len(counts)):
        state = P.track_heads_host(boxes[t:t + 1], counts[t:t + 1], state=state, **opts)[6]
        out.append(velocity(state))
    return out


# ---------------------------------------------------------------- 1. the hand scenario
def test_the_plain_tracker_loses_the_walker():
    boxes, counts = MC.HAND
    r = P.track_heads_host(boxes, counts, **MC.HAND_OPTIONS)
    assert len(r) == 7
    assert r[2][:, 0].tolist() == [1] * 9 + [0] and r[2][:, 1].tolist() == [0] * 7 + [2] * 3      # frame 7 is born as id 2 in slot 1; id 1 dies of age
    assert r[4][:, 0].tolist() == [0, 0, 0, 0] + [-1] * 6 and r[4][:, 1].tolist() == [-1] * 7 + [0] * 3
    assert set(r[2][r[4] >= 0].tolist()) == {1, 2}


@pytest.mark.parametrize('gain, v, coast, predicted', [(1.0, [12.0, 12.0, 12.0], [48.0, 60.0, 72.0], 84.0), (0.5, [6.0, 9.0, 10.5], [46.5, 57.0, 67.5], 78.0)])
def test_the_motion_model_keeps_the_walker(results, gain, v, coast, predicted):
    boxes, counts, opts = MC.ALL[f'hand_gain_{gain}']
    assert opts['motion'] == dict(gain=gain, decay=1.0)
    slot_boxes, image_of, track_id, age, det_of, flags, state, state_boxes = results[f'hand_gain_{gain}']
    seen = [t for t in range(10) if t not in MC.HAND_MISSED]
    assert track_id[:, 0].tolist() == [1] * 10 and not track_id[:, 1:].any() and int(state[0, 0]) == 1      # ONE id, ever
    assert det_of[:, 0].tolist() == [0 if t in seen else -1 for t in range(10)] and image_of[:, 0].tolist() == [t if t in seen else -1 for t in range(10)]
    assert age[:, 0].tolist() == [0, 0, 0, 0, 1, 2, 3, 0, 0, 0] and flags.tolist() == [0] * 10
    vel = velocities_per_frame(boxes, counts, opts)
    assert [vel[t] for t in (1, 2, 3)] == [[x, 0.0] for x in v]
    assert vel[0] == [0.0, 0.0] and vel[4] == vel[5] == vel[6] == [v[2], 0.0]                                # decay 1: the coasting velocity stays
    assert [state_boxes[t, 0].tolist() for t in MC.HAND_MISSED] == [[x, 0.0, x + 24.0, 24.0] for x in coast]  # the coasting box moves
    assert all(state_boxes[t, 0].tolist() == slot_boxes[t, 0].tolist() == [12.0 * t, 0.0, 12.0 * t + 24.0, 24.0] for t in seen)
    assert not slot_boxes[list(MC.HAND_MISSED)].any() and not state_boxes[:, 1:].any()
    # frame 7: the detection at 84 against the predicted box -- and against the plain tracker's stale one
    assert coast[2] + v[2] == predicted
    inter = (predicted + 24.0 - 84.0) * 24.0
    assert inter / (2 * 576.0 - inter) == {84.0: 1.0, 78.0: 0.6}[predicted]


# ---------------------------------------------------------------- 2. gain = 0
@pytest.mark.parametrize('name', list(TC.ALL))
@pytest.mark.parametrize('decay', [1.0, 0.5])
def test_gain_0_is_the_plain_tracker(name, decay):
    boxes, counts, opts = TC.ALL[name]
    plain = P.track_heads_host(boxes, counts, **opts)
    got = P.track_heads_host(boxes, counts, motion=dict(gain=0.0, decay=decay), **opts)
    assert len(plain) == 7 and len(got) == 8
    same(got, plain, name, n=7)
    same(P.track_heads_host(boxes, counts, state=plain[6], motion=dict(gain=0, decay=decay), **opts), P.track_heads_host(boxes, counts, state=plain[6], **opts),
         name + ', second pass', n=7)


# ---------------------------------------------------------------- 3. purity
def in_single_frames(boxes, counts, opts):
    given_q = boxes.ndim == 4
    b4, c2 = (boxes, counts) if given_q else (boxes[None], counts[None])
    Q, T = c2.shape
    parts, state = [], None
    for t in range(T):
        r = P.track_heads_host(b4[:, t:t + 1], c2[:, t:t + 1], state=state, **opts)
        state = r[6]
        image_of = np.where(r[1] >= 0, (np.arange(Q) * T)[:, None, None] + t, -1).astype(np.int32)              # q * T + t of the whole call
        parts.append((r[0], image_of) + r[2:6] + (r[7],))
    out = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(7))
    out = out if given_q else tuple(o[0] for o in out)
    return out[:6] + (state, out[6])


@pytest.mark.parametrize('name', MC.PURITY)
def test_frames_in_one_call_or_one_by_one(results, name):
    boxes, counts, opts = MC.ALL[name]
    same(in_single_frames(boxes, counts, opts), results[name], name)
    moved = np.abs(np.ascontiguousarray(results[name][6][:, TRACK_HEADER_WORDS:]).reshape(-1, TRACK_SLOT_WORDS)[:, 6:8].view(F)).max()
    assert moved > 0.5                                                                         # velocities are at work in the case
    coasting = (results[name][2] > 0) & (results[name][4] < 0)
    assert coasting.any()                                                                      # and slots coast in it


# ---------------------------------------------------------------- 4. the edge rules
def test_a_slot_freed_and_reborn_in_one_frame_starts_at_rest(results):
    boxes, counts, opts = MC.ALL['freed_and_reborn_in_one_frame']
    r = results['freed_and_reborn_in_one_frame']
    assert r[2][:, 0].tolist() == [1, 1, 2, 2] and r[4][:, 0].tolist() == [0, 0, 0, 0]
    assert velocities_per_frame(boxes, counts, opts) == [[0.0, 0.0], [10.0, 0.0], [0.0, 0.0], [1.0, 0.0]]


def test_an_overflowing_prediction_keeps_the_box_and_stops_the_slot(results):
    boxes, counts, opts = MC.ALL['prediction_overflows']
    r = results['prediction_overflows']
    vel = velocities_per_frame(boxes, counts, opts)
    assert vel[1] == [float((boxes[1, 0, 0] + boxes[1, 0, 2]) * F(0.5)), 0.0] and vel[1][0] > 1.4e38 and vel[2] == [0.0, 0.0] and vel[3] == [0.0, 0.0]
    with np.errstate(over='ignore'):
        assert np.isinf(boxes[1, 0, 2] + F(vel[1][0]))                                          # x2 + vx is past f32
    assert r[2][:, 0].tolist() == [1] * 4 and r[3][:, 0].tolist() == [0, 0, 1, 0]
    same([r[7][2, 0]], [boxes[1, 0]], 'the coasting box is the last match', n=1)


def test_a_velocity_update_that_is_not_finite_zeroes_the_velocity(results):
    boxes, counts, opts = MC.ALL['velocity_update_overflows']
    with np.errstate(over='ignore'):
        assert np.isinf(boxes[1, 0, 0] + boxes[1, 0, 2])
    assert results['velocity_update_overflows'][2][:, 0].tolist() == [1, 1, 1]
    assert velocities_per_frame(boxes, counts, opts) == [[0.0, 0.0]] * 3
    # a velocity handed in through the state that is not finite: the prediction fails, the slot stops
    state = results['velocity_update_overflows'][6].copy()
    state[0, TRACK_HEADER_WORDS + 6:TRACK_HEADER_WORDS + 8] = np.asarray([np.nan, 1.0], F).view(np.int32)
    after = P.track_heads_host(boxes[2:], counts[2:], state=state, **opts)
    assert velocity(after[6]) == [0.0, 0.0] and after[2][0, 0] == 1


@pytest.mark.parametrize('name', ['nan_and_inf_rows', 'counts_out_of_range'])
def test_bad_rows_and_counts_are_flagged_as_the_plain_tracker_flags_them(results, name):
    boxes, counts, opts = TC.ALL[name]
    plain = P.track_heads_host(boxes, counts, **opts)
    got = results[name]
    assert got[5].tolist() == plain[5].tolist() and set(got[5].tolist()) == {0, 2 if name == 'nan_and_inf_rows' else 4}
    assert got[2].tolist() == plain[2].tolist() and got[4].tolist() == plain[4].tolist()         # nobody was born from a bad row
    assert np.isfinite(got[7]).all() and np.isfinite(np.ascontiguousarray(got[6][:, TRACK_HEADER_WORDS:]).view(F).reshape(-1, 8)[:, [0, 1, 2, 3, 6, 7]]).all()


def test_a_negative_zero_survives_a_frame_at_rest(results):
    r = results['negative_zero_at_rest']
    minus0 = np.asarray([-0.0, -0.0, 20, 20], F).view(np.int32).tolist()
    assert minus0[0] == minus0[1] == -2 ** 31
    assert r[3][:, 0].tolist() == [0, 1, 0, 1]
    for t in range(4):
        assert r[7][t, 0].view(np.int32).tolist() == minus0, t
    assert slot_box(r[6]).view(np.int32).tolist() == minus0 and velocity(r[6]) == [0.0, 0.0]


# ---------------------------------------------------------------- 5. one state, two forms
def test_the_plain_form_leaves_the_velocity_words_alone():
    boxes, counts = MC.HAND
    motion = dict(gain=1.0, decay=1.0)
    a = P.track_heads_host(boxes[:4], counts[:4], motion=motion, **MC.HAND_OPTIONS)
    assert velocity(a[6]) == [12.0, 0.0]
    b = P.track_heads_host(boxes[4:6], counts[4:6], state=a[6], **MC.HAND_OPTIONS)                # the plain form: coasts where it stands
    assert velocity(b[6]) == [12.0, 0.0] and slot_box(b[6]).tolist() == [36.0, 0.0, 60.0, 24.0] and b[3][:, 0].tolist() == [1, 2]
    c = P.track_heads_host(boxes[6:], counts[6:], state=b[6], motion=motion, **MC.HAND_OPTIONS)   # and on, moving: 48 at frame 6, 60 at frame 7
    assert c[7][0, 0].tolist() == [48.0, 0.0, 72.0, 24.0] and c[7][1, 0].tolist() == [60.0, 0.0, 84.0, 24.0]
    assert c[2][:, 0].tolist() == [1, 1, 1, 0] and c[2][:, 1].tolist() == [0, 2, 2, 2]            # two frames late: 60 against 84 no longer overlaps
    # slots that are free and stay free keep whatever their words hold
    state = np.zeros((1, P.track_state_words(4)), np.int32)
    state[0, TRACK_HEADER_WORDS + 3 * TRACK_SLOT_WORDS + 6] = 1234
    assert P.track_heads_host(boxes, counts, state=state, motion=motion, **MC.HAND_OPTIONS)[6][0, TRACK_HEADER_WORDS + 3 * TRACK_SLOT_WORDS + 6] == 1234


# ---------------------------------------------------------------- 6. surface
def test_header_binding_and_library_agree_on_the_motion_entry():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    assert re.search(r'\bint mcg_track_heads_motion\(mcg_stream s, const float\* boxes_dev, long long frame_stride, const int32_t\* counts_dev,', hdr)
    assert re.search(r'int max_age, double velocity_gain, double coast_decay,\s+void\* state_dev,', hdr) and 'float* state_boxes_dev' in hdr
    assert 'mcg_track_heads_motion' in L.EXPORTS and hasattr(lib, 'mcg_track_heads_motion') and len(lib.mcg_track_heads_motion.argtypes) == 20
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20
    assert 'The reserved words are neither read nor\n * written.' in hdr                         # the plain entry's contract stands


def test_the_entry_refuses_bad_arguments_before_any_launch():
    """Every call here is refused by the argument checks (or has no sequences): nothing is launched and no pointer is followed."""
    lib = L.load()
    vp = C.c_void_p
    fake = 4096                                                                                # never dereferenced

    def call(q=1, t=1, d=4, stride=16, slots=4, iou=0.3, max_age=5, gain=0.5, decay=1.0, state=fake, boxes=fake, state_boxes=fake):
        return lib.mcg_track_heads_motion(vp(0), vp(boxes), stride, vp(fake), q, t, d, slots, iou, max_age, gain, decay, vp(state), *[vp(fake)] * 6, vp(state_boxes))

    for bad, word in [(dict(gain=v), b'velocity_gain') for v in (float('nan'), float('inf'), -0.1, 1.5)] + \
                     [(dict(decay=v), b'coast_decay') for v in (float('nan'), float('inf'), -0.1, 1.5, -float('inf'))] + \
                     [(dict(slots=0), b'slots'), (dict(slots=65), b'slots'), (dict(d=0), b'max_det'), (dict(d=1025, stride=4100), b'max_det'), (dict(t=0), b'num_frames'),
                      (dict(max_age=-1), b'max_age'), (dict(iou=float('nan')), b'finite'), (dict(stride=15), b'frame_stride'), (dict(q=-1), b'sequences'),
                      (dict(q=65536), b'sequences'), (dict(boxes=0), b'null pointer'), (dict(state=0), b'null pointer'), (dict(state=fake + 4), b'aligned'),
                      (dict(q=65535, t=1024, slots=64), b'2^31')]:
        assert call(**bad) == 1, bad                                                           # MCG_ERR_ARG
        msg = lib.mcg_last_error()
        assert word in msg and b'mcg_track_heads_motion' in msg, (bad, msg)
    assert call(q=0) == L.MCG_OK and call(q=0, gain=0.0, decay=0.0, state=0, boxes=0, state_boxes=0) == L.MCG_OK
    assert call(q=0, gain=1.5) == 1                                                            # the parameters are checked whatever the sizes
    # and the plain entry's messages still carry its own name
    assert lib.mcg_track_heads(vp(0), vp(fake), 16, vp(fake), 1, 1, 4, 0, 0.3, 5, vp(fake), *[vp(fake)] * 6) == 1
    assert lib.mcg_last_error().startswith(b'mcg_track_heads: slots')


ENGINE = types.SimpleNamespace(device='cuda:0')                 # run_head_video reads the device before it checks track=
BAD_MOTION = (False, 0.5, 'on', dict(gain=0.5, decya=1.0), dict(gain=float('nan')), dict(gain=-0.1), dict(gain=1.5), dict(decay=float('inf')),
              dict(decay=-0.1), dict(decay=1.5), dict(gain=True), dict(gain='0.5'))


def test_argument_errors_of_the_python_layers():
    boxes, counts = MC.HAND
    for bad in BAD_MOTION:
        with pytest.raises(ValueError, match='motion'):
            P.track_heads_host(boxes, counts, motion=bad)
        with pytest.raises(ValueError, match='motion'):
            harness.run_head_video(ENGINE, None, [], [], track=dict(motion=bad))
        with pytest.raises(ValueError, match='motion'):
            live.LiveGaze(None, None, cameras=1, slots=4, motion=bad)
    with pytest.raises(ValueError, match='slots, match_iou, max_age and motion'):
        harness.run_head_video(ENGINE, None, [], [], track=dict(gain=0.5))
    for ok in (True, dict(), dict(gain=0), dict(decay=1), dict(gain=np.float32(0.25), decay=0.75)):
        assert len(P.track_heads_host(boxes, counts, motion=ok)) == 8
    r = P.track_heads_host(boxes, counts, motion=True, **MC.HAND_OPTIONS)                        # the defaults are gain 0.5, decay 1
    same(r, P.track_heads_host(boxes, counts, motion=dict(gain=0.5, decay=1.0), **MC.HAND_OPTIONS))
    q = P.track_heads_host(boxes[None], counts[None], motion=True, **MC.HAND_OPTIONS)
    assert q[7].shape == (1, 10, 4, 4) and r[7].shape == (10, 4, 4)
    same(tuple(x[0] for x in q[:6]) + (q[6], q[7][0]), r)
