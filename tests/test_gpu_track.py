"""-m gpu: head identities across frames on the device -- DevicePipeline.track_heads (mcg_track_heads), the entry through ctypes, the chain
detect_heads -> track_heads -> head_crops inside one graph, and harness.run_head_video(track=...).

Every comparison is bit for bit against pipeline.track_heads_host (itself checked against a naive restatement of the header and against
hand-worked tables in tests/test_track_cpu.py), in all seven results: no tolerance anywhere.  The NaN and infinite rows and the counts out of
range are inputs the entry documents (flag bits 2 and 4); nothing here provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import detect_cases as D
from tests import track_cases as TC
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES = ('slot_boxes', 'image_of', 'track_id', 'age', 'det_of', 'flags', 'state')
EVERY = {**TC.ALL, **{'hand_' + k: v + (TC.HAND_OPTIONS,) for k, v in TC.HAND.items()}}


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(64))


@pytest.fixture(scope='module')
def host_results():
    return {name: P.track_heads_host(boxes, counts, **opts) for name, (boxes, counts, opts) in EVERY.items()}


def same(got, want, what=''):
    """Seven device tensors against seven host arrays, bit for bit (floats as their int32 patterns)."""
    torch.cuda.synchronize()
    assert len(got) == len(want) == 7
    for g, w, name in zip(got, want, NAMES):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(np.ascontiguousarray(g).view(np.int32), np.ascontiguousarray(w).view(np.int32)), (what, name)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- 1. the device computes what the host computes
@pytest.mark.parametrize('name', list(EVERY))
def test_track_heads_equals_track_heads_host(pipe, host_results, name):
    boxes, counts, opts = EVERY[name]
    same(pipe.track_heads(dev(boxes), dev(counts), **opts), host_results[name], name)
    before = pipe._ring.i
    same(pipe.track_heads(boxes, counts, device=DEV, **opts), host_results[name], name + ', host inputs')
    assert pipe._ring.i == (before + 1) % pipe.STAGES                       # numpy inputs went up through one stage
    # and from a state that is not empty, updated in place
    state = dev(host_results[name][6])
    got = pipe.track_heads(dev(boxes), dev(counts.astype(np.int64)), state=state, **opts)
    assert got[6] is state and pipe._ring.i == (before + 1) % pipe.STAGES   # device inputs take no stage
    same(got, P.track_heads_host(boxes, counts, state=host_results[name][6], **opts), name + ', second pass')


# ---------------------------------------------------------------- 2. the state carried across calls, one frame a tick
def test_the_state_carried_across_device_calls_is_the_hosts():
    pipe = P.DevicePipeline(chain(64))
    boxes, counts, opts = TC.ALL['q3_different_histories']
    assert counts.shape == (3, 12)
    state_d, state_h = None, None
    for t in range(12):
        got = pipe.track_heads(dev(boxes[:, t:t + 1]), dev(counts[:, t:t + 1]), state=state_d, **opts)
        want = P.track_heads_host(boxes[:, t:t + 1], counts[:, t:t + 1], state=state_h, **opts)
        same(got, want, f'tick {t}')
        state_d, state_h = got[6], want[6]
    assert state_h[:, 1].tolist() == [12, 12, 12] and state_h[:, 0].min() >= 2


# ---------------------------------------------------------------- 3. strided views of a larger buffer
def test_inputs_that_are_strided_views(pipe, host_results):
    name = 'q3_different_histories'
    boxes, counts, opts = TC.ALL[name]
    Q, T, Dn, _ = boxes.shape
    # frames a gap of 3 rows apart; what lies between would be born as a head if it were read
    buf = torch.full((Q, T, Dn + 3, 4), 7.0, dtype=torch.float32, device=DEV)
    buf[..., 2:] = 30.0
    view = buf[:, :, :Dn]
    view.copy_(dev(boxes))
    assert view.stride() == (T * (Dn + 3) * 4, (Dn + 3) * 4, 4, 1) and not view.is_contiguous()
    wide = torch.zeros(Q, 2 * T, dtype=torch.int32, device=DEV)
    wide[:, ::2] = dev(counts)
    same(pipe.track_heads(view, wide[:, ::2], **opts), host_results[name], 'frame stride')
    # layouts the entry does not read are made contiguous first: boxes 8 floats apart, sequences not T frames apart
    loose = torch.zeros(Q, T, Dn, 8, device=DEV)
    loose[..., :4] = dev(boxes)
    same(pipe.track_heads(loose[..., :4], dev(counts), **opts), host_results[name], 'box stride')
    apart = torch.zeros(Q, T + 2, Dn, 4, device=DEV)
    apart[:, :T] = dev(boxes)
    same(pipe.track_heads(apart[:, :T], dev(counts), **opts), host_results[name], 'sequence stride')
    one, one_n, one_opts = TC.ALL['walkers_s16']                              # [T, D, 4]: one sequence
    pad = torch.full((one.shape[0], one.shape[1] + 1, 4), 5.0, device=DEV)
    pad[:, :one.shape[1]] = dev(one)
    same(pipe.track_heads(pad[:, :one.shape[1]], dev(one_n), **one_opts), host_results['walkers_s16'], 'one sequence, frame stride')


# ---------------------------------------------------------------- 4. the entry through ctypes
def test_the_entry_checks_its_arguments_before_any_launch(host_results):
    lib = L.load()
    name = 'q3_different_histories'
    boxes, counts, opts = TC.ALL[name]
    Q, T, Dn, _ = boxes.shape
    S = opts['slots']
    b, c = dev(boxes), dev(counts)
    state = torch.zeros(Q, P.track_state_words(S), dtype=torch.int32, device=DEV)
    assert lib.mcg_track_state_bytes(Q, S) == state.numel() * 4
    new = lambda *shape, dtype=torch.int32: torch.full(shape, -7, dtype=dtype, device=DEV)
    out = [new(Q, T, S, 4, dtype=torch.float32), new(Q, T, S), new(Q, T, S), new(Q, T, S), new(Q, T, S), new(Q, T)]
    vp = C.c_void_p
    s = vp(torch.cuda.current_stream().cuda_stream)

    def call(boxes_=b.data_ptr(), stride=4 * Dn, counts_=c.data_ptr(), q=Q, t=T, d=Dn, slots=S, iou=opts['match_iou'], max_age=opts['max_age'],
             state_=state.data_ptr(), null=None):
        ptrs = [None if k == null else t_.data_ptr() for k, t_ in enumerate(out)]
        return lib.mcg_track_heads(s, vp(boxes_), stride, vp(counts_), q, t, d, slots, iou, max_age, vp(state_), *(vp(p) for p in ptrs))

    err = lambda: lib.mcg_last_error()
    for bad, word in ((dict(slots=0), b'slots'), (dict(slots=65), b'slots'), (dict(d=0), b'max_det'), (dict(d=1025, stride=4 * 1025), b'max_det'),
                      (dict(t=0), b'num_frames'), (dict(max_age=-1), b'max_age'), (dict(iou=float('nan')), b'finite'), (dict(iou=float('inf')), b'finite'),
                      (dict(stride=4 * Dn - 1), b'frame_stride'), (dict(q=-1), b'sequences'), (dict(q=65536), b'sequences'), (dict(boxes_=None), b'null pointer'),
                      (dict(counts_=None), b'null pointer'), (dict(state_=None), b'null pointer'), (dict(state_=state.data_ptr() + 4), b'aligned'),
                      *((dict(null=k), b'null pointer') for k in range(6))):
        assert call(**bad) == 1 and word in err(), bad                       # MCG_ERR_ARG
    assert call(q=0) == L.MCG_OK                                              # no sequences: no launch
    torch.cuda.synchronize()
    assert all((t_ == -7).all() for t_ in out) and not state.any()            # refused before any launch: nothing was written
    L.check(call(), 'mcg_track_heads')                                        # and the call itself writes every output in full
    same(out + [state], host_results[name], 'poisoned outputs')


def test_host_arguments_are_checked_before_anything_is_launched(pipe):
    boxes, counts = TC.HAND['crossing']
    b, c = dev(boxes), dev(counts)
    for bad in (dict(slots=0), dict(slots=65), dict(match_iou=float('nan')), dict(max_age=-1)):
        with pytest.raises(ValueError):
            pipe.track_heads(b, c, **bad)
    with pytest.raises(ValueError):
        pipe.track_heads(b[0], c)
    with pytest.raises(ValueError):
        pipe.track_heads(b, c[:-1])
    with pytest.raises(ValueError):
        pipe.track_heads(b, c, state=torch.zeros(1, P.track_state_words(4), dtype=torch.int32, device=DEV), slots=5)
    with pytest.raises(TypeError):
        pipe.track_heads(b.double(), c)
    with pytest.raises(TypeError):
        pipe.track_heads(b, c.float())
    with pytest.raises(TypeError):
        pipe.track_heads(b, c, state=torch.zeros(1, P.track_state_words(4), dtype=torch.int32), slots=4)      # a host state cannot be updated in place
    got = pipe.track_heads(torch.zeros(0, 2, 3, 4, device=DEV), torch.zeros(0, 2, dtype=torch.int32, device=DEV), slots=5)
    assert [tuple(t.shape) for t in got] == [(0, 2, 5, 4), (0, 2, 5), (0, 2, 5), (0, 2, 5), (0, 2, 5), (0, 2), (0, P.track_state_words(5))]


# ---------------------------------------------------------------- 5. detect_heads -> track_heads -> head_crops in one graph
SIDE = 64                                                        # frames and the detector's input: gain 1, no pads -- the boxes are the rows'
TICKS = [[(4, 4, 24, 26), (36, 30, 58, 52)],                     # two heads
         [(38, 32, 60, 54), (6, 5, 26, 27)],                     # both moved, listed the other way round
         [(8, 6, 28, 28), (30, 2, 44, 16), (40, 34, 62, 56)],    # a third in between
         [(42, 36, 62, 58)]]                                     # only the second is seen: the others coast


def tick_inputs(k):
    pred = D.rows([h + (0.9 - 0.1 * j, 0, 1) for j, h in enumerate(TICKS[k])] + [(h[0] + 1, h[1], h[2] + 1, h[3], 0.4, 0, 1) for h in TICKS[k]], n=32)
    return pred, np.random.RandomState(90 + k).randint(0, 256, (SIDE, SIDE, 3)).astype(np.uint8)


def test_detect_track_crop_captures_in_a_graph(pipe):
    S, opts = 4, dict(slots=4, match_iou=0.3, max_age=2)
    pred_buf, frame_buf = dev(tick_inputs(0)[0]), dev(tick_inputs(0)[1])
    state = torch.zeros(1, P.track_state_words(S), dtype=torch.int32, device=DEV)

    def step():
        d = pipe.detect_heads(pred_buf, (SIDE, SIDE), (SIDE, SIDE), max_det=6)
        tr = pipe.track_heads(d[0], d[4], state=state, **opts)
        return tr, pipe.head_crops([frame_buf], tr[0].view(-1, 4), tr[1].view(-1), device=DEV)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # the eager call: workspace, frame sizes and the frame table, once
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cached = (len(pipe._detect_workspaces), len(pipe._frame_hw_tables), len(pipe._image_tables), pipe._ring.i)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr, crops = step()
    assert cached == (len(pipe._detect_workspaces), len(pipe._frame_hw_tables), len(pipe._image_tables), pipe._ring.i)
    state.zero_()                                                 # the eager call and the capture's warm-up saw tick 0
    state_h, ids = None, []
    for k in range(len(TICKS)):
        pred, frame = tick_inputs(k)
        pred_buf.copy_(dev(pred))
        frame_buf.copy_(dev(frame))
        graph.replay()
        torch.cuda.synchronize()
        det = P.detect_heads_host(pred, (SIDE, SIDE), (SIDE, SIDE), max_det=6)
        assert det[4].tolist() == [len(TICKS[k])]
        want = P.track_heads_host(det[0], det[4], state=state_h, **opts)
        state_h = want[6]
        same(tr[:6] + (state,), want, f'tick {k}')
        valid = want[1].reshape(-1) >= 0
        ref = pipe.head_crops([frame], want[0].reshape(-1, 4)[valid], np.zeros(int(valid.sum()), np.int32), device=DEV)
        torch.cuda.synchronize()
        for g, w in zip(crops, ref):
            assert torch.equal(g.cpu()[torch.from_numpy(valid)], w.cpu()), f'tick {k}'
        assert crops[4].cpu()[torch.from_numpy(~valid)].tolist() == [2] * int((~valid).sum())       # slots that saw no head: flagged, skipped
        ids.append(want[2][0].tolist())
    assert ids == [[1, 2, 0, 0], [1, 2, 0, 0], [1, 2, 3, 0], [1, 2, 3, 0]]


# ---------------------------------------------------------------- 6. run_head_video with tracking
def crossing_video():
    """Eight 48 x 64 frames, two heads that cross: the left one is listed first in every frame, so the order flips where they pass."""
    frames = [np.random.RandomState(60 + t).randint(0, 256, (48, 64, 3)).astype(np.uint8) for t in range(8)]
    a = [[4.0 + 4 * t, 2.0, 24.0 + 4 * t, 22.0] for t in range(8)]
    b = [[40.0 - 4 * t, 18.0, 60.0 - 4 * t, 38.0] for t in range(8)]
    per_frame = [sorted([a[t], b[t]], key=lambda bx: bx[0]) for t in range(8)]
    assert per_frame[0][0] == a[0] and per_frame[7][0] == b[7]
    return frames, per_frame, a, b


def same_records(got, want, skip=()):
    assert len(got) == len(want)
    for g, r in zip(got, want):
        assert sorted(g) == sorted(r)
        for k in r:
            if k not in skip:
                assert np.array_equal(g[k], r[k]) if isinstance(r[k], np.ndarray) else g[k] == r[k], k


def test_run_head_video_with_tracking():
    from mcgaze_amd.engine import HipEngine
    e = HipEngine(synth.make_state_dict(0), precision='f16x3')
    pipe = P.DevicePipeline(chain(64))
    frames, per_frame, a, b = crossing_video()
    records = harness.run_head_video(e, pipe, frames, per_frame, max_len=4, track=True, smooth=0.5)
    assert [r['id'] for r in records] == [1, 2] and all(r['frame_id'] == list(range(8)) for r in records)
    assert records[0]['head_box'].tolist() == a and records[1]['head_box'].tolist() == b          # each person keeps ONE track through the crossing
    # the records are those of the existing path fed the tracker's tracks one person at a time
    for rec, person in zip(records, (a, b)):
        alone = harness.run_head_video(e, pipe, frames, [[bx] for bx in person], max_len=4, smooth=0.5)
        assert len(alone) == 1 and alone[0]['id'] == (0, 0)
        same_records([rec], alone, skip=('id',))
    # the detector's raw output instead of lists: detect_heads' device outputs go to the tracker where they are
    pred = np.concatenate([D.rows([tuple(bx) + (0.9 - 0.2 * j, 0, 1) for j, bx in enumerate(heads)], n=8) for heads in per_frame])
    for p in (pred, torch.from_numpy(pred).to(DEV)):
        same_records(harness.run_head_video(e, pipe, frames, detections=dict(pred=p, in_shape=(48, 64), max_det=4), max_len=4, track=dict(slots=4), smooth=0.5), records)
    # track=None is the path without the option: segment_tracks' (segment, person) records, which swap the people at the crossing
    default = harness.run_head_video(e, pipe, frames, per_frame, max_len=4, smooth=0.5)
    same_records(harness.run_head_video(e, pipe, frames, per_frame, max_len=4, smooth=0.5, track=None), default)
    assert [r['id'] for r in default] == [(0, 0), (0, 1)] and default[0]['head_box'].tolist() != a
    # drawn in ascending id
    _, annotated = harness.run_head_video(e, pipe, frames, per_frame, max_len=4, track=True, draw=True)
    assert len(annotated) == 8
    with pytest.raises(ValueError, match=r'frame 0 .*slots=1'):
        harness.run_head_video(e, pipe, frames, per_frame, max_len=4, track=dict(slots=1))
    with pytest.raises(ValueError):
        harness.run_head_video(e, pipe, frames, per_frame, track=dict(slot=4))
