"""Head identities across frames on the host: pipeline.track_heads_host (the numpy twin of mcg_track_heads) and harness.tracks_from_slots.
Every comparison is exact -- floats as their int32 patterns; there is no tolerance anywhere.

1. the twin against a deliberately naive restatement of the header's section (plain loops, np.float32 scalars, one max() per round)
2. hand-worked stories with the expected tables written out
3. T frames in one call = T calls of one frame = two calls of T / 2, tables and state
4. on videos of separated walkers the tracker's persons are segment_tracks' persons
5. where segment_tracks' rule breaks -- a crossing, someone entering and leaving -- and the tracker does not
6. ValueError / TypeError for every bad shape and option; exports, header and binding agree
"""
import os
import re

import numpy as np
import pytest

from mcgaze_amd import harness
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from mcgaze_amd.head_detect import TRACK_HEADER_WORDS, TRACK_SLOT_WORDS
from tests import track_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('slot_boxes', 'image_of', 'track_id', 'age', 'det_of', 'flags', 'state')
F = np.float32
EVERY = {**TC.ALL, **{'hand_' + k: v + (TC.HAND_OPTIONS,) for k, v in TC.HAND.items()}}


def same(got, want, what=''):
    assert len(got) == len(want) == 7
    for g, w, name in zip(got, want, NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(np.ascontiguousarray(g).view(np.int32), np.ascontiguousarray(w).view(np.int32)), (what, name)


# ---------------------------------------------------------------- 1. the naive restatement
def naive_iou(a, b):
    """Step 2 of the header on two boxes of np.float32 scalars."""
    area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    w, h = max(F(0), min(a[2], b[2]) - max(a[0], b[0])), max(F(0), min(a[3], b[3]) - max(a[1], b[1]))
    inter = w * h
    return inter / (area_a + area_b - inter) + F(0)


def naive_track(boxes, counts, state, slots, match_iou, max_age):
    """The section "head identities across frames" of include/mcgaze_hip.h, one sentence at a time."""
    boxes, counts = np.asarray(boxes, F), np.asarray(counts)
    given_q = boxes.ndim == 4
    if not given_q:
        boxes, counts = boxes[None], counts[None]
    Q, T, D, S = boxes.shape[0], boxes.shape[1], boxes.shape[2], slots
    words = TRACK_HEADER_WORDS + TRACK_SLOT_WORDS * S
    state = np.zeros((Q, words), np.int32) if state is None else state.copy()
    thr = F(match_iou)
    out_box, out_img, out_id = np.zeros((Q, T, S, 4), F), np.zeros((Q, T, S), np.int32), np.zeros((Q, T, S), np.int32)
    out_age, out_det, out_flags = np.zeros((Q, T, S), np.int32), np.zeros((Q, T, S), np.int32), np.zeros((Q, T), np.int32)
    with np.errstate(all='ignore'):
        for q in range(Q):
            next_id, frames_seen = int(state[q, 0]), int(state[q, 1])
            slot = []
            for s in range(S):
                rec = state[q, TRACK_HEADER_WORDS + TRACK_SLOT_WORDS * s:][:TRACK_SLOT_WORDS]
                slot.append(dict(box=[F(v) for v in rec[:4].view(F)], id=int(rec[4]), age=int(rec[5])))
            for t in range(T):
                c = int(counts[q, t])
                n = min(max(c, 0), D)
                det = [[F(v) for v in boxes[q, t, d]] for d in range(n)]
                usable = [all(np.isfinite(v) for v in b) for b in det]
                flag = (4 if c != n else 0) | (0 if all(usable) else 2)
                got = {}                                         # slot -> the detection it was matched with or born from
                taken = set()
                while True:
                    pairs = []
                    for s in range(S):
                        for d in range(n):
                            if slot[s]['id'] > 0 and usable[d] and s not in got and d not in taken:
                                iou = naive_iou(slot[s]['box'], det[d])
                                if iou > thr:
                                    pairs.append((iou, -s, -d))
                    if not pairs:
                        break
                    _, s, d = max(pairs)
                    got[-s] = -d
                    taken.add(-d)
                for s in range(S):
                    if s in got:
                        slot[s]['box'], slot[s]['age'] = det[got[s]], 0
                    elif slot[s]['id'] > 0:
                        slot[s]['age'] += 1
                        if slot[s]['age'] > max_age:
                            slot[s] = dict(box=[F(0)] * 4, id=0, age=0)
                for d in range(n):
                    if usable[d] and d not in taken:
                        free = [s for s in range(S) if slot[s]['id'] == 0]
                        if not free:
                            flag |= 1
                            continue
                        next_id += 1
                        slot[free[0]] = dict(box=det[d], id=next_id, age=0)
                        got[free[0]] = d
                        taken.add(d)
                for s in range(S):
                    hit = s in got
                    out_box[q, t, s] = det[got[s]] if hit else [0, 0, 0, 0]
                    out_img[q, t, s], out_det[q, t, s] = (q * T + t, got[s]) if hit else (-1, -1)
                    out_id[q, t, s], out_age[q, t, s] = slot[s]['id'], slot[s]['age'] if slot[s]['id'] != 0 else -1
                out_flags[q, t] = flag
            state[q, 0], state[q, 1] = next_id, frames_seen + T
            for s in range(S):
                rec = state[q, TRACK_HEADER_WORDS + TRACK_SLOT_WORDS * s:][:TRACK_SLOT_WORDS]
                rec[:4], rec[4], rec[5] = np.asarray(slot[s]['box'], F).view(np.int32), slot[s]['id'], slot[s]['age']
    out = (out_box, out_img, out_id, out_age, out_det, out_flags)
    return (out if given_q else tuple(o[0] for o in out)) + (state,)


@pytest.fixture(scope='module')
def host_results():
    return {name: P.track_heads_host(boxes, counts, **opts) for name, (boxes, counts, opts) in EVERY.items()}


@pytest.mark.parametrize('name', list(EVERY))
def test_the_twin_equals_the_naive_restatement(host_results, name):
    boxes, counts, opts = EVERY[name]
    want = naive_track(boxes, counts, None, **opts)
    same(host_results[name], want, name)
    # and from a state that is not empty: the state the case leaves, fed the case again
    same(P.track_heads_host(boxes, counts, state=want[6], **opts), naive_track(boxes, counts, want[6], **opts), name + ', second pass')


def test_the_cases_reach_what_they_are_there_for(host_results):
    flags = {name: np.asarray(r[5]).reshape(-1) for name, r in host_results.items()}
    crowd = host_results['s64_d300_crowd']
    assert flags['s64_d300_crowd'].tolist() == [1, 1, 1, 0] and (crowd[2][0] > 0).all() and crowd[4][0].tolist() == list(range(64))   # the best 64 of 70
    assert crowd[2][3].tolist() == crowd[2][0].tolist() and sorted(crowd[3][3].tolist()) == [0] * 40 + [1] * 24
    assert TC.ALL['s64_d300_crowd'][0].shape[1] == 300 and 64 * 70 > 256
    assert flags['more_heads_than_slots'].tolist() == [1, 1, 0, 1]
    assert flags['nan_and_inf_rows'].tolist() == [0, 2, 2, 0] and flags['counts_out_of_range'].tolist() == [0, 4, 4, 0]
    assert host_results['nan_and_inf_rows'][2][-1].tolist() == [1, 2, 0, 0]                 # nothing was born from the bad rows
    assert host_results['d300_rows_behind_counts'][2].tolist() == [[1, 2, 0, 0]] * 4        # box(1) behind the counts would have been id 3
    assert host_results['identical_boxes'][4].tolist() == [[0, 1, -1], [0, 1, 2], [0, 1, 2], [0, 1, -1]]   # ties: the lower slot takes the lower detection
    r = host_results['coast_exactly_max_age']
    assert r[3][:, 0].tolist() == [0, 1, 2, 3, 0] and r[2][:, 0].tolist() == [1] * 5
    r = host_results['coast_one_more_than_max_age']
    assert r[3][:, 0].tolist() == [0, 1, 2, 3, -1, 0] and r[2][:, 0].tolist() == [1, 1, 1, 1, 0, 3]
    assert host_results['max_age_0'][2].tolist() == [[1, 2, 0, 0], [0, 2, 0, 0], [3, 2, 0, 0], [3, 0, 0, 0]]
    assert host_results['freed_and_refilled_in_one_frame'][2].tolist() == [[1], [2], [2], [2]]
    assert flags['freed_and_refilled_in_one_frame'].tolist() == [0, 0, 0, 1]
    assert host_results['touching_boxes_match_iou_0'][2].tolist() == [[1, 0, 0, 0], [1, 2, 0, 0], [1, 2, 3, 0]]   # one pixel of overlap matches, touching does not
    assert host_results['negative_match_iou'][4].tolist() == [[0, 1, -1], [0, 1, 2], [0, -1, -1]]
    empty = host_results['count0_and_an_empty_sequence']
    assert (empty[2][1] == 0).all() and (empty[1][1] == -1).all() and empty[6][1, :2].tolist() == [0, 8] and not empty[6][1, 2:].any()
    assert (empty[1][0, 4] == -1).all() and (empty[2][0, 4] > 0).sum() == 3
    assert TC.ALL['q3_different_histories'][0].shape[0] == 3 and len({r.tobytes() for r in host_results['q3_different_histories'][2]}) == 3
    assert TC.ALL['s1_d1_one_person'][0].shape[1:] == (1, 4) and host_results['s1_d1_one_person'][2].reshape(-1).tolist() == [1, 1, 1, 1, 1, 1]


# ---------------------------------------------------------------- 2. hand-worked stories
def check_story(name, ids, dets, ages, people):
    """people[s][t]: the box slot s holds in frame t when it was matched there."""
    boxes, counts = TC.HAND[name]
    slot_boxes, image_of, track_id, age, det_of, flags, state = P.track_heads_host(boxes, counts, **TC.HAND_OPTIONS)
    T = len(ids)
    assert track_id.tolist() == ids and det_of.tolist() == dets and age.tolist() == ages and flags.tolist() == [0] * T
    assert image_of.tolist() == [[t if d >= 0 else -1 for d in row] for t, row in enumerate(dets)]
    assert slot_boxes.tolist() == [[[float(v) for v in people[s][t]] if dets[t][s] >= 0 else [0.0] * 4 for s in range(3)] for t in range(T)]
    assert state[0, :2].tolist() == [max(max(r) for r in ids), T]


def test_two_people_crossing():
    a, b = [TC.A(x) for x in (0, 8, 16, 24, 32)], [TC.B(x) for x in (36, 28, 20, 12, 4)]
    check_story('crossing', ids=[[1, 2, 0]] * 5, dets=[[0, 1, -1]] * 3 + [[1, 0, -1]] * 2, ages=[[0, 0, -1]] * 5, people=[a, b, None])


def test_a_third_person_present_for_three_frames():
    a, b = [TC.A(2 * t) for t in range(7)], [TC.B(100 - 2 * t) for t in range(7)]
    c = [None, None, TC.C3(50), TC.C3(52), TC.C3(54), None, None]
    check_story('enter_leave', ids=[[1, 2, 0]] * 2 + [[1, 2, 3]] * 5, dets=[[0, 1, -1]] * 2 + [[1, 2, 0]] * 3 + [[0, 1, -1]] * 2,
                ages=[[0, 0, -1]] * 2 + [[0, 0, 0]] * 3 + [[0, 0, 1], [0, 0, 2]], people=[a, b, c])


def test_one_missed_detection():
    a, b = [TC.A(2 * t) for t in range(5)], [TC.B(100 - 2 * t) for t in range(5)]
    check_story('missed', ids=[[1, 2, 0]] * 5, dets=[[0, 1, -1]] * 2 + [[0, -1, -1]] + [[0, 1, -1]] * 2,
                ages=[[0, 0, -1]] * 2 + [[0, 1, -1]] + [[0, 0, -1]] * 2, people=[a, b, None])


# ---------------------------------------------------------------- 3. carrying the state
def in_parts(boxes, counts, opts, bounds):
    """The case run as consecutive calls over frames bounds[i] .. bounds[i + 1], the state carried -> the seven results of one call."""
    given_q = boxes.ndim == 4
    b4, c2 = (boxes, counts) if given_q else (boxes[None], counts[None])
    Q, T = c2.shape
    parts, state = [], None
    for a, z in zip(bounds[:-1], bounds[1:]):
        r = P.track_heads_host(b4[:, a:z], c2[:, a:z], state=state, **opts)
        state = r[6]
        image_of = np.where(r[1] >= 0, r[1] - (np.arange(Q) * (z - a))[:, None, None] - np.arange(z - a)[None, :, None]
                            + (np.arange(Q) * T)[:, None, None] + np.arange(a, z)[None, :, None], -1).astype(np.int32)   # q * T + t of the whole call
        parts.append((r[0], image_of) + r[2:6])
    out = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(6))
    return (out if given_q else tuple(o[0] for o in out)) + (state,)


@pytest.mark.parametrize('name', list(TC.ALL))
def test_frames_in_one_call_or_in_many(host_results, name):
    boxes, counts, opts = TC.ALL[name]
    T = counts.shape[-1]
    same(in_parts(boxes, counts, opts, list(range(T + 1))), host_results[name], name + ', one frame per call')
    same(in_parts(boxes, counts, opts, [0, T // 2, T]), host_results[name], name + ', two halves')


# ---------------------------------------------------------------- 4. the tie to the reference's rule
MATCH_IOU = 0.3


def iou64(a, b):
    w, h = max(0.0, min(a[2], b[2]) - max(a[0], b[0])), max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    return w * h / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - w * h)


def separated_walkers(seed, T=10, people=4):
    """A video in which segment_tracks' rule holds: a constant head count, no crossings in x1, every person's consecutive boxes overlapping
    with IoU > MATCH_IOU and different people's boxes never overlapping at all -- asserted, every one, for every video.  The detector's order
    is random per frame.  -> (boxes_per_frame, per person its boxes)."""
    rs = np.random.RandomState(seed)
    x = 150.0 * np.arange(people) + rs.uniform(0, 20, people)
    y = rs.uniform(0, 300, people)
    person = [[] for _ in range(people)]
    for t in range(T):
        x, y = x + rs.uniform(-4, 4, people), y + rs.uniform(-4, 4, people)
        for p in range(people):
            s = 30 + rs.uniform(-1, 1)
            person[p].append(np.asarray([x[p], y[p], x[p] + s, y[p] + s], F).tolist())           # python floats that are exact f32 values
    frames = [[person[p][t] for p in rs.permutation(people)] for t in range(T)]
    assert all(len(f) == people for f in frames)                                                  # a constant head count
    for t in range(T):
        assert [b[0] for b in sorted(frames[t], key=lambda b: b[0])] == [person[p][t][0] for p in range(people)]   # no crossings: x1 order = person order
    for p in range(people):
        for t in range(1, T):
            assert iou64(person[p][t - 1], person[p][t]) > MATCH_IOU + 0.05                       # the same person overlaps from frame to frame
        for o in range(people):
            if o != p:
                assert all(iou64(a, b) == 0.0 for a in person[p] for b in person[o])              # different people never do
    return frames, person


@pytest.mark.parametrize('seed', range(6))
def test_separated_walkers_give_the_persons_of_segment_tracks(seed):
    people = 2 + seed % 4
    frames, person = separated_walkers(100 + seed, people=people)
    boxes, counts = TC.table(frames, people + 1)
    r = P.track_heads_host(boxes, counts, slots=8, match_iou=MATCH_IOU, max_age=5)
    tracks = harness.tracks_from_slots(r[0], r[2], r[1])
    segments = harness.segment_tracks(frames)
    assert len(segments) == 1 and len(segments[0]['boxes']) == people
    ref = {(tuple(segments[0]['frame_id']), tuple(map(tuple, b))) for b in segments[0]['boxes']}
    got = {(tuple(tr['frame_id']), tuple(map(tuple, tr['boxes'][0]))) for tr in tracks}
    assert got == ref and len(got) == people
    assert [tr['id'] for tr in tracks] == list(range(1, people + 1))                              # numbered in detection order of frame 0, not by x1
    assert [tr['boxes'][0][0] for tr in tracks] == frames[0]


# ---------------------------------------------------------------- 5. where the reference's rule breaks, as designed
def hand_tracks(name):
    r = P.track_heads_host(*TC.HAND[name], **TC.HAND_OPTIONS)
    return harness.tracks_from_slots(r[0], r[2], r[1])


def test_a_crossing_swaps_segment_tracks_persons_and_not_the_trackers():
    a, b = [TC.A(x) for x in (0, 8, 16, 24, 32)], [TC.B(x) for x in (36, 28, 20, 12, 4)]
    seg = harness.segment_tracks(TC.CROSSING)
    assert len(seg) == 1 and seg[0]['boxes'] == [a[:3] + b[3:], b[:3] + a[3:]]                    # from frame 3 on each holds the other person
    tracks = hand_tracks('crossing')
    as_float = lambda boxes: [[float(v) for v in bx] for bx in boxes]
    assert [tr['id'] for tr in tracks] == [1, 2] and all(tr['frame_id'] == [0, 1, 2, 3, 4] for tr in tracks)
    assert tracks[0]['boxes'] == [as_float(a)] and tracks[1]['boxes'] == [as_float(b)]


def test_entering_and_leaving_cuts_segment_tracks_and_not_the_trackers():
    seg = harness.segment_tracks(TC.ENTER_LEAVE)
    assert len(seg) == 3 and sum(len(s['boxes']) for s in seg) == 7
    tracks = hand_tracks('enter_leave')
    assert [(tr['id'], tr['frame_id']) for tr in tracks] == [(1, list(range(7))), (2, list(range(7))), (3, [2, 3, 4])]
    missed = hand_tracks('missed')
    assert [(tr['id'], tr['frame_id']) for tr in missed] == [(1, [0, 1, 2, 3, 4]), (2, [0, 1, 3, 4])]      # the coasted frame is left out
    assert len(harness.segment_tracks(TC.MISSED)) == 3                                           # one miss cuts everyone's track in two


# ---------------------------------------------------------------- 6. arguments, exports
def test_argument_errors():
    boxes, counts = TC.HAND['crossing']
    for bad in (dict(slots=0), dict(slots=65), dict(slots=2.5), dict(match_iou=float('nan')), dict(match_iou=float('inf')), dict(max_age=-1), dict(max_age=1.5)):
        with pytest.raises(ValueError):
            P.track_heads_host(boxes, counts, **bad)
    for b, c in ((boxes[0], counts), (boxes[..., :3], counts), (boxes, counts[:-1]), (boxes, counts[None]), (boxes[None], counts), (boxes[:0], counts[:0]),
                 (boxes[:, :0], counts), (np.zeros((2, 1025, 4), F), np.zeros(2, np.int32)), (np.zeros((1, 1, 2, 3, 4), F), np.zeros((1, 1, 2), np.int32))):
        with pytest.raises(ValueError):
            P.track_heads_host(b, c)
    state = P.track_heads_host(boxes, counts, slots=4)[6]
    assert state.shape == (1, P.track_state_words(4)) and state.dtype == np.int32
    with pytest.raises(ValueError):
        P.track_heads_host(boxes, counts, state=state, slots=5)                                   # a state of another number of slots
    with pytest.raises(ValueError):
        P.track_heads_host(np.stack([boxes, boxes]), np.stack([counts, counts]), state=state, slots=4)
    with pytest.raises(TypeError):
        P.track_heads_host(boxes.astype(np.float64), counts)
    with pytest.raises(TypeError):
        P.track_heads_host(boxes, counts.astype(np.float32))
    with pytest.raises(TypeError):
        P.track_heads_host(boxes, counts, state=state.astype(np.int64), slots=4)
    before = state.copy()
    P.track_heads_host(boxes, counts, state=state, slots=4)
    assert np.array_equal(state, before)                                                          # the host twin hands back a new state
    with pytest.raises(ValueError):
        harness.tracks_from_slots(np.zeros((2, 3, 4), F), np.zeros((2, 2), np.int32), np.zeros((2, 3), np.int32))


def test_header_binding_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    assert re.search(r'\bint mcg_track_heads\(mcg_stream s, const float\* boxes_dev, long long frame_stride, const int32_t\* counts_dev,', hdr)
    assert re.search(r'\bsize_t mcg_track_state_bytes\(int num_sequences, int slots\);', hdr)
    for name, nargs in (('mcg_track_heads', 17), ('mcg_track_state_bytes', 2)):
        assert name in L.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20
    for slots in (1, 16, 64):                                     # the published layout: a 16-byte header, 32 bytes per slot
        assert lib.mcg_track_state_bytes(3, slots) == 3 * 4 * P.track_state_words(slots) == 3 * (16 + 32 * slots)
    assert lib.mcg_track_state_bytes(1, 0) == 0 and lib.mcg_track_state_bytes(1, 65) == 0 and lib.mcg_track_state_bytes(-1, 4) == 0
    assert P.track_heads_host is not None and 'track.hip' in open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'Makefile')).read()
