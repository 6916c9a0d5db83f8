"""-m gpu: head boxes from a detector's raw output on the device -- DevicePipeline.detect_heads (mcg_detect_heads), the entry through ctypes,
and head_crops / harness.run_head_video(detections=...) on top.

Every comparison is bit for bit against pipeline.detect_heads_host (itself checked against the reference restated in torch and against
hand-worked answers in tests/test_detect_cpu.py), in all six outputs including the zeroed rows behind each image's count: no tolerance
anywhere.  The NaN and infinite boxes of the hand cases are inputs the entry documents (the rows are dropped); nothing here provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import detect_cases as D
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES = ('boxes', 'scores', 'classes', 'image_of', 'counts', 'flags')


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(64))


@pytest.fixture(scope='module')
def host_results():
    return {name: P.detect_heads_host(pred, in_shape, hw, **opts) for name, (pred, in_shape, hw, opts) in D.ALL.items()}


def same(got, want, what=''):
    """Six device tensors against six host arrays, bit for bit (floats as their int32 patterns)."""
    torch.cuda.synchronize()
    assert len(got) == len(want) == 6
    for g, w, name in zip(got, want, NAMES):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(np.ascontiguousarray(g).view(np.int32), np.ascontiguousarray(w).view(np.int32)), (what, name)


# ---------------------------------------------------------------- 1. the device computes what the host computes
@pytest.mark.parametrize('name', list(D.ALL))
def test_detect_heads_equals_detect_heads_host(pipe, host_results, name):
    pred, in_shape, hw, opts = D.ALL[name]
    same(pipe.detect_heads(torch.from_numpy(pred).to(DEV), in_shape, hw, **opts), host_results[name], name)


def test_host_predictions_go_through_the_staging_ring_and_frame_hw_may_be_on_the_device(pipe, host_results):
    for name in ('n1025_b3_mixed_frames', 'n64_agnostic'):
        pred, in_shape, hw, opts = D.ALL[name]
        before = pipe._ring.i
        same(pipe.detect_heads(pred, in_shape, hw, device=DEV, **opts), host_results[name], name)
        assert pipe._ring.i == (before + 1) % pipe.STAGES
        hw_dev = torch.from_numpy(np.broadcast_to(np.asarray(hw, dtype=np.int64), (len(pred), 2)).copy()).to(DEV)
        same(pipe.detect_heads(torch.from_numpy(pred).to(DEV), in_shape, hw_dev, **opts), host_results[name], name + ', device frame_hw')
        assert pipe._ring.i == (before + 1) % pipe.STAGES                 # a device prediction takes no stage


@pytest.mark.parametrize('name', list(D.HAND))
def test_hand_cases(pipe, name):
    pred, opts, want_boxes, want_classes = D.HAND[name]
    got = pipe.detect_heads(torch.from_numpy(pred).to(DEV), D.SQUARE, D.SQUARE, **opts)
    same(got, P.detect_heads_host(pred, D.SQUARE, D.SQUARE, **opts), name)
    n = int(got[4][0])
    assert got[0][0, :n].tolist() == want_boxes and got[2][0, :n].tolist() == want_classes and got[5].tolist() == [0]


def test_strides_come_from_the_tensor_and_fp16_is_widened(pipe, host_results):
    name = 'n1025_b3_mixed_frames'
    pred, in_shape, hw, opts = D.ALL[name]
    B, N, F = pred.shape
    # rows 9 floats apart, images a gap of 5 rows apart; what lies between would pass every filter if it were read
    buf = torch.full((B, N + 5, 9), 0.999, dtype=torch.float32, device=DEV)
    view = buf[:, :N, :F]
    view.copy_(torch.from_numpy(pred).to(DEV))
    assert view.stride() == ((N + 5) * 9, 9, 1)
    same(pipe.detect_heads(view, in_shape, hw, **opts), host_results[name], 'strided')
    # a layout the entry does not read (class scores 2 floats apart): made contiguous first
    wide = torch.zeros(B, N, 2 * F, device=DEV)
    wide[:, :, ::2] = torch.from_numpy(pred).to(DEV)
    same(pipe.detect_heads(wide[:, :, ::2], in_shape, hw, **opts), host_results[name], 'inner stride 2')
    half = torch.from_numpy(pred).to(DEV).half()
    want = P.detect_heads_host(half.cpu().numpy(), in_shape, hw, **opts)
    assert want[4].max() >= 2
    same(pipe.detect_heads(half, in_shape, hw, **opts), want, 'fp16')


def test_max_nms_uses_the_prefix_of_the_full_result(pipe):
    pred, in_shape, hw, opts = D.ALL['n2048_all_max_nms']
    dev = torch.from_numpy(pred).to(DEV)
    cut = [t.cpu().numpy() for t in pipe.detect_heads(dev, in_shape, hw, **opts)]
    full = [t.cpu().numpy() for t in pipe.detect_heads(dev, in_shape, hw, **{**opts, 'max_nms': 2048, 'max_det': 300})]
    assert cut[5].tolist() == [1] and full[5].tolist() == [0]
    conf = np.sort((pred[0, :, 5:] * pred[0, :, 4:5]).max(axis=1))[::-1]             # every row is a head candidate here
    floor = conf[opts['max_nms'] - 1]
    assert conf[opts['max_nms']] < floor
    # the full run's detections whose score is among the best max_nms, in order: the truncated run's
    inside = full[1][0, :full[4][0]] >= floor
    n = int(cut[4][0])
    assert n == min(int(inside.sum()), 300) and n >= 2
    assert np.array_equal(cut[0][0, :n], full[0][0, :full[4][0]][inside][:n]) and np.array_equal(cut[1][0, :n], full[1][0, :full[4][0]][inside][:n])


# ---------------------------------------------------------------- 2. the entry through ctypes
def test_the_entry_writes_every_output_in_full_and_checks_its_arguments(host_results):
    lib = L.load()
    name = 'no_frame'                                                  # B = 3, flags 0, 2, 2
    pred, in_shape, hw, _ = D.ALL[name]
    B, N, F = pred.shape
    p = torch.from_numpy(pred).to(DEV)
    hw_dev = torch.tensor(hw, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.mcg_detect_heads_workspace_bytes(B, N), dtype=torch.uint8, device=DEV)
    new = lambda *shape, dtype=torch.int32: torch.full(shape, -7, dtype=dtype, device=DEV)
    out = [new(B, 300, 4, dtype=torch.float32), new(B, 300, dtype=torch.float32), new(B, 300), new(B, 300), new(B), new(B)]
    vp = C.c_void_p
    s = vp(torch.cuda.current_stream().cuda_stream)

    def call(pred_=p.data_ptr(), b=B, n=N, nc=F - 5, row=F, in_h=in_shape[0], conf=0.25, iou=0.45, max_nms=N, max_det=300, flags=out[5].data_ptr(),
             ws_bytes=ws.numel()):
        return lib.mcg_detect_heads(s, vp(pred_), b, n, nc, N * F, row, in_h, in_shape[1], vp(hw_dev.data_ptr()), conf, iou, 1, 0, max_nms, max_det,
                                    *(vp(t.data_ptr()) for t in out[:5]), vp(flags), vp(ws.data_ptr()), ws_bytes)

    L.check(call(), 'mcg_detect_heads')
    same(out, host_results[name], 'poisoned outputs')
    for t in out:
        t.fill_(-7)
    L.check(call(flags=None), 'mcg_detect_heads')                      # flags_dev = NULL: everything else as before, flags untouched
    same(out[:5] + [torch.zeros_like(out[5])], host_results[name][:5] + (np.zeros(B, np.int32),), 'no flags')
    assert out[5].tolist() == [-7] * B
    for t in out:
        t.fill_(-7)
    assert call(b=0) == L.MCG_OK                                        # B = 0: no launch, nothing written
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in out)
    err = lambda: lib.mcg_last_error()
    assert call(nc=0) != L.MCG_OK and b'num_classes' in err()
    assert call(max_det=0) != L.MCG_OK and b'max_det' in err()
    assert call(max_det=301) != L.MCG_OK and b'max_det' in err()
    assert call(max_nms=0) != L.MCG_OK and b'max_nms' in err()
    assert call(max_nms=N + 1) != L.MCG_OK and b'max_nms' in err()
    assert call(ws_bytes=ws.numel() - 1) != L.MCG_OK and b'workspace too small' in err()
    assert call(conf=float('nan')) != L.MCG_OK and b'finite' in err()
    assert call(iou=float('inf')) != L.MCG_OK and b'finite' in err()
    assert call(row=F - 1) != L.MCG_OK and b'strides' in err()
    assert call(in_h=0) != L.MCG_OK and b'input' in err()
    assert call(n=0) != L.MCG_OK and b'anchors' in err()
    assert call(pred_=None) != L.MCG_OK and b'null pointer' in err()
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in out)                            # refused before any launch


def test_host_arguments_are_checked_before_anything_is_launched(pipe):
    pred, in_shape, hw, _ = D.RANDOM['n63_tight_iou']
    dev = torch.from_numpy(pred).to(DEV)
    for bad in (dict(max_det=0), dict(max_det=301), dict(max_nms=0), dict(conf_thres=float('nan')), dict(iou_thres=float('inf'))):
        with pytest.raises(ValueError):
            pipe.detect_heads(dev, in_shape, hw, **bad)
    with pytest.raises(ValueError):
        pipe.detect_heads(dev[0], in_shape, hw)
    with pytest.raises(ValueError):
        pipe.detect_heads(dev, in_shape, torch.zeros(2, 2, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError):
        pipe.detect_heads(dev.double(), in_shape, hw)
    with pytest.raises(TypeError):
        pipe.detect_heads(dev, in_shape, (160.0, 160.0))
    got = pipe.detect_heads(dev[:0], in_shape, np.zeros((0, 2), np.int32), max_det=5)
    assert [tuple(t.shape) for t in got] == [(0, 5, 4), (0, 5), (0, 5), (0, 5), (0,), (0,)]


# ---------------------------------------------------------------- 3. nothing is read on the host
def test_detect_heads_captures_in_a_graph(pipe, host_results):
    name = 'n1025_b3_mixed_frames'
    pred, in_shape, hw, opts = D.ALL[name]
    dev = torch.from_numpy(pred).to(DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # the eager call: allocates the workspace and uploads the frame sizes, once
        eager = pipe.detect_heads(dev, in_shape, hw, **opts)
    torch.cuda.current_stream().wait_stream(side)
    same(eager, host_results[name], 'eager')
    cached = (len(pipe._detect_workspaces), len(pipe._frame_hw_tables), pipe._ring.i)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pipe.detect_heads(dev, in_shape, hw, **opts)
    assert cached == (len(pipe._detect_workspaces), len(pipe._frame_hw_tables), pipe._ring.i)
    for _ in range(2):
        for t in got:
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(g, e) for g, e in zip(got, eager))
    same(got, host_results[name], 'replayed')


# ---------------------------------------------------------------- 4. on top: head_crops and run_head_video
def two_frames():
    """Two 48 x 64 frames seen by a 96 x 128 detector (gain 2, no pads), two heads each, a second anchor firing on every head."""
    heads = [[(20, 16, 60, 60), (70, 30, 110, 80)], [(8, 10, 40, 50), (60, 40, 120, 90)]]
    pred = np.concatenate([D.rows([h + (0.9, 0, 1) for h in hs] + [(h[0] + 2, h[1], h[2] + 2, h[3], 0.6, 0, 1) for h in hs], n=16) for hs in heads])
    frames = [np.random.RandomState(70 + k).randint(0, 256, (48, 64, 3)).astype(np.uint8) for k in range(2)]
    return pred, (96, 128), frames


def test_detections_feed_head_crops_without_a_read_back(pipe):
    pred, in_shape, frames = two_frames()
    dev_frames = [torch.from_numpy(f).to(DEV) for f in frames]
    boxes, _, _, image_of, counts, flags = pipe.detect_heads(torch.from_numpy(pred).to(DEV), in_shape, (48, 64), max_det=6)
    got = pipe.head_crops(dev_frames, boxes.view(-1, 4), image_of.view(-1), device=DEV)
    torch.cuda.synchronize()
    assert counts.tolist() == [2, 2] and flags.tolist() == [0, 0]
    assert boxes[0, :2].tolist() == [[10, 8, 30, 30], [35, 15, 55, 40]]
    valid = (image_of.view(-1) >= 0).cpu()
    assert valid.tolist() == ([True] * 2 + [False] * 4) * 2
    per_frame = harness.head_boxes_per_frame(boxes, counts)
    want = pipe.head_crops(frames, np.asarray([b for f in per_frame for b in f], np.float32), np.asarray([0, 0, 1, 1], np.int32), device=DEV)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g.cpu()[valid], w.cpu())
    assert got[4].cpu()[~valid].tolist() == [2] * 8 and got[4].cpu()[valid].tolist() == [0] * 4     # the rows behind the counts come back flagged


def test_run_head_video_from_raw_predictions():
    from mcgaze_amd.engine import HipEngine
    e = HipEngine(synth.make_state_dict(0), precision='f16x3')
    pipe = P.DevicePipeline(chain(64))
    h, w = 48, 64
    frames = [np.random.RandomState(80 + t).randint(0, 256, (h, w, 3)).astype(np.uint8) for t in range(3)]
    # in_shape == the frame: the boxes are the rows'.  Two heads per frame, a weaker second anchor on each; the last frame shows one head
    heads = [[(8 + t, 6, 30 + t, 30), (36 + t, 20, 60 + t, 44)] for t in range(3)]
    heads[2] = heads[2][:1]
    pred = np.concatenate([D.rows([b + (0.9, 0, 1) for b in hs] + [(b[0] + 1, b[1], b[2] + 1, b[3], 0.5, 0, 1) for b in hs], n=8) for hs in heads])
    detections = dict(pred=pred, in_shape=(h, w), max_det=4)
    got = pipe.detect_heads(torch.from_numpy(pred).to(DEV), (h, w), (h, w), max_det=4)
    per_frame = harness.head_boxes_per_frame(got[0], got[4])
    assert per_frame == [[[float(v) for v in b] for b in hs] for hs in heads]
    want = harness.run_head_video(e, pipe, frames, per_frame, max_len=4)
    for records in (harness.run_head_video(e, pipe, frames, detections=detections, max_len=4),
                    harness.run_head_video(e, pipe, frames, detections=dict(detections, pred=torch.from_numpy(pred).to(DEV)), max_len=4)):
        assert len(records) == len(want) == 3                       # a segment of two people over two frames, one of one person
        for g, r in zip(records, want):
            assert sorted(g) == sorted(r)
            for k in r:
                assert np.array_equal(g[k], r[k]) if isinstance(r[k], np.ndarray) else g[k] == r[k], k
    with pytest.raises(ValueError):
        harness.run_head_video(e, pipe, frames, per_frame, detections=detections)
    with pytest.raises(ValueError):
        harness.run_head_video(e, pipe, frames)
