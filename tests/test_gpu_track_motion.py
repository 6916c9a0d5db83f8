"""-m gpu: the tracker with its constant-velocity motion model on the device -- DevicePipeline.track_heads(motion=...) and
mcg_track_heads_motion through ctypes -- against pipeline.track_heads_host(motion=...) (held to hand-worked numbers in
tests/test_track_motion_cpu.py).  Every comparison is bit for bit, in all six tables, the state and state_boxes: no tolerance anywhere.
The NaN and infinite rows, the boxes near the end of f32 and the counts out of range are inputs the entry documents; nothing here provokes a
fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from mcgaze_amd.head_detect import TRACK_HEADER_WORDS, TRACK_SLOT_WORDS
from tests import track_cases as TC
from tests import track_motion_cases as MC
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES = ('slot_boxes', 'image_of', 'track_id', 'age', 'det_of', 'flags', 'state', 'state_boxes')
PLAIN = {**TC.ALL, **{'hand_' + k: v + (TC.HAND_OPTIONS,) for k, v in TC.HAND.items()}}


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(64))


@pytest.fixture(scope='module')
def host_results():
    return {name: P.track_heads_host(boxes, counts, **opts) for name, (boxes, counts, opts) in MC.ALL.items()}


def same(got, want, what='', n=8):
    """Device tensors against host arrays, bit for bit (floats as their int32 patterns)."""
    torch.cuda.synchronize()
    assert len(got) >= n and len(want) >= n, (what, len(got), len(want))
    for g, w, name in zip(got[:n], want[:n], NAMES):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(np.ascontiguousarray(g).view(np.int32), np.ascontiguousarray(w).view(np.int32)), (what, name)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- 1. the device computes what the host computes
@pytest.mark.parametrize('name', list(MC.ALL))
def test_track_heads_with_motion_equals_the_host_twin(pipe, host_results, name):
    boxes, counts, opts = MC.ALL[name]
    got = pipe.track_heads(dev(boxes), dev(counts), **opts)
    assert len(got) == 8
    same(got, host_results[name], name)
    # and from the state the case leaves, updated in place: velocities come in through the state words
    state = dev(host_results[name][6])
    again = pipe.track_heads(dev(boxes), dev(counts), state=state, **opts)
    assert again[6] is state
    same(again, P.track_heads_host(boxes, counts, state=host_results[name][6], **opts), name + ', second pass')


def test_the_hand_scenario_on_the_device(pipe):
    boxes, counts = MC.HAND
    plain = pipe.track_heads(dev(boxes), dev(counts), **MC.HAND_OPTIONS)
    moving = pipe.track_heads(dev(boxes), dev(counts), motion=dict(gain=1.0, decay=1.0), **MC.HAND_OPTIONS)
    torch.cuda.synchronize()
    assert len(plain) == 7 and sorted(set(plain[2].cpu()[plain[4].cpu() >= 0].tolist())) == [1, 2]
    assert set(moving[2].cpu()[moving[4].cpu() >= 0].tolist()) == {1}
    assert moving[7][4:7, 0].cpu().tolist() == [[x, 0.0, x + 24.0, 24.0] for x in (48.0, 60.0, 72.0)]


# ---------------------------------------------------------------- 2. gain = 0 is the plain entry
@pytest.mark.parametrize('name', list(PLAIN))
def test_gain_0_equals_the_plain_entry(pipe, name):
    boxes, counts, opts = PLAIN[name]
    plain = pipe.track_heads(dev(boxes), dev(counts), **opts)
    got = pipe.track_heads(dev(boxes), dev(counts), motion=dict(gain=0.0, decay=0.5), **opts)
    torch.cuda.synchronize()
    same(got, [t.cpu().numpy() for t in plain], name, n=7)


# ---------------------------------------------------------------- 3. the state carried across calls; a frame stride; a graph
def test_one_frame_per_call_equals_one_call():
    pipe = P.DevicePipeline(chain(64))
    for name in ('q3_gain_0.5', 'q3_decay_0.5'):
        boxes, counts, opts = MC.ALL[name]
        assert counts.shape == (3, 12)
        whole = pipe.track_heads(dev(boxes), dev(counts), **opts)
        state_d, state_h = None, None
        for t in range(12):
            got = pipe.track_heads(dev(boxes[:, t:t + 1]), dev(counts[:, t:t + 1]), state=state_d, **opts)
            want = P.track_heads_host(boxes[:, t:t + 1], counts[:, t:t + 1], state=state_h, **opts)
            same(got, want, f'{name}, tick {t}')
            assert torch.equal(got[7][:, 0], whole[7][:, t]) and torch.equal(got[2][:, 0], whole[2][:, t]), (name, t)
            state_d, state_h = got[6], want[6]
        assert torch.equal(state_d, whole[6])


def test_frames_further_apart_than_their_rows(pipe, host_results):
    name = 'q3_gain_0.5'
    boxes, counts, opts = MC.ALL[name]
    Q, T, Dn, _ = boxes.shape
    buf = torch.full((Q, T, Dn + 3, 4), 7.0, dtype=torch.float32, device=DEV)      # what lies between the frames would be born if it were read
    buf[..., 2:] = 30.0
    view = buf[:, :, :Dn]
    view.copy_(dev(boxes))
    assert view.stride() == (T * (Dn + 3) * 4, (Dn + 3) * 4, 4, 1) and not view.is_contiguous()
    same(pipe.track_heads(view, dev(counts), **opts), host_results[name], 'frame stride')


def test_track_heads_with_motion_captures_in_a_graph(pipe):
    boxes, counts, opts = MC.ALL['q3_gain_0.5']
    Q, S = 3, opts['slots']
    box_buf, count_buf = dev(boxes[:, :1]), dev(counts[:, :1])
    state = torch.zeros(Q, P.track_state_words(S), dtype=torch.int32, device=DEV)
    pipe.track_heads(box_buf, count_buf, state=state, **opts)                        # eager once: nothing is left to be set up
    torch.cuda.synchronize()
    before = pipe._ring.i
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                 # one stream, one kernel
        out = pipe.track_heads(box_buf, count_buf, state=state, **opts)
    assert pipe._ring.i == before and out[6] is state
    state.zero_()
    eager_state = torch.zeros_like(state)
    for t in range(4):
        box_buf.copy_(dev(boxes[:, t:t + 1]))
        count_buf.copy_(dev(counts[:, t:t + 1]))
        graph.replay()
        want = pipe.track_heads(dev(boxes[:, t:t + 1]), dev(counts[:, t:t + 1]), state=eager_state, **opts)
        torch.cuda.synchronize()
        for g, w, n in zip(out, want, NAMES):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w), (n, t)
    assert int(state[:, 1].min()) == 4


# ---------------------------------------------------------------- 4. one state, two entries
def test_a_state_handed_from_the_plain_entry_to_the_motion_entry_and_back(pipe):
    boxes, counts, opts = MC.ALL['q3_gain_0.5']
    plain = {k: v for k, v in opts.items() if k != 'motion'}
    words = lambda st: st.cpu().numpy()[:, TRACK_HEADER_WORDS:].reshape(3, -1, TRACK_SLOT_WORDS)[..., 6:8].copy()
    state_h = None
    state = torch.zeros(3, P.track_state_words(opts['slots']), dtype=torch.int32, device=DEV)
    for a, z, o in ((0, 3, plain), (3, 7, opts), (7, 9, plain), (9, 12, opts)):
        before = words(state)
        got = pipe.track_heads(dev(boxes[:, a:z]), dev(counts[:, a:z]), state=state, **o)
        want = P.track_heads_host(boxes[:, a:z], counts[:, a:z], state=state_h, **o)
        same(got, want, f'frames {a} .. {z}', n=len(want))
        state_h = want[6]
        if o is plain:
            assert np.array_equal(words(state), before)                           # the plain entry leaves the velocity words as they were
        else:
            assert np.abs(words(state).view(np.float32)).max() > 0.5


# ---------------------------------------------------------------- 5. the entry through ctypes
def test_the_entry_with_and_without_state_boxes(host_results):
    lib = L.load()
    name = 'q3_gain_0.5'
    boxes, counts, opts = MC.ALL[name]
    Q, T, Dn, _ = boxes.shape
    S, (gain, decay) = opts['slots'], (opts['motion']['gain'], opts['motion']['decay'])
    b, c = dev(boxes), dev(counts)
    new = lambda *shape, dtype=torch.int32: torch.full(shape, -7, dtype=dtype, device=DEV)
    vp = C.c_void_p
    s = vp(torch.cuda.current_stream().cuda_stream)
    for with_boxes in (False, True):
        state = torch.zeros(Q, P.track_state_words(S), dtype=torch.int32, device=DEV)
        out = [new(Q, T, S, 4, dtype=torch.float32), new(Q, T, S), new(Q, T, S), new(Q, T, S), new(Q, T, S), new(Q, T)]
        state_boxes = new(Q, T, S, 4, dtype=torch.float32)

        def call(gain_=gain, state_=state.data_ptr()):
            return lib.mcg_track_heads_motion(s, vp(b.data_ptr()), 4 * Dn, vp(c.data_ptr()), Q, T, Dn, S, opts['match_iou'], opts['max_age'], gain_, decay,
                                              vp(state_), *(vp(t.data_ptr()) for t in out), vp(state_boxes.data_ptr() if with_boxes else None))

        assert call(gain_=1.5) == 1 and b'velocity_gain' in lib.mcg_last_error()
        assert call(state_=state.data_ptr() + 4) == 1 and b'aligned' in lib.mcg_last_error()
        torch.cuda.synchronize()
        assert all((t_ == -7).all() for t_ in out + [state_boxes]) and not state.any()           # refused before any launch: nothing was written
        L.check(call(), 'mcg_track_heads_motion')
        same(out + [state], host_results[name], 'state_boxes given' if with_boxes else 'state_boxes NULL', n=7)
        if with_boxes:
            same([state_boxes], [host_results[name][7]], 'state_boxes', n=1)
        else:
            assert (state_boxes == -7).all()


def test_host_arguments_are_checked_before_anything_is_launched(pipe):
    boxes, counts = MC.HAND
    for bad in (False, 0.5, dict(gain=1.5), dict(decay=-0.1), dict(gain=float('nan')), dict(speed=1.0)):
        with pytest.raises(ValueError, match='motion'):
            pipe.track_heads(dev(boxes), dev(counts), motion=bad)
    got = pipe.track_heads(torch.zeros(0, 2, 3, 4, device=DEV), torch.zeros(0, 2, dtype=torch.int32, device=DEV), slots=5, motion=True)
    assert [tuple(t.shape) for t in got] == [(0, 2, 5, 4), (0, 2, 5), (0, 2, 5), (0, 2, 5), (0, 2, 5), (0, 2), (0, P.track_state_words(5)), (0, 2, 5, 4)]
    one = pipe.track_heads(boxes, counts, device=DEV, motion=True, **MC.HAND_OPTIONS)               # numpy inputs, one sequence
    same(one, P.track_heads_host(boxes, counts, motion=True, **MC.HAND_OPTIONS), 'host inputs')
