"""-m gpu: the detector's input on the device -- DevicePipeline.letterbox (mcg_letterbox_frames / mcg_letterbox_frames_nv12), the entries
through ctypes, and the chain letterbox -> detector -> detect_heads -> head_crops / harness.run_head_video(detections=dict(detector=...)).

Every comparison is torch.equal against head_detect.letterbox_host (itself checked against the oracle's resize, np.pad and torch's own
conversion in tests/test_letterbox_cpu.py): no tolerance anywhere, halves and floats compared as values that are never NaN.  Frames and
options come from tests/letterbox_cases.py.  The descriptors the direct calls pass are ones the entry documents (an empty or clipped
rectangle is all border); nothing here provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import head_detect as H
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import detect_cases as D
from tests import letterbox_cases as LC
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TORCH = dict(uint8=torch.uint8, float16=torch.float16, float32=torch.float32)
_HOST = {}


def host(name, dtype, geometry=False):
    """letterbox_host of a case (geometry: its per-frame geometries), computed once per (case, dtype) and left alone."""
    if (name, dtype) not in _HOST:
        frames, opts = LC.CASES[name]
        img, geoms = H.letterbox_host(frames, dtype=TORCH[dtype], **opts)
        _HOST[name, dtype] = torch.from_numpy(img), geoms
    return _HOST[name, dtype][int(geometry)]


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(64))


def to_device(frame):
    return tuple(torch.from_numpy(p).to(DEV) for p in frame) if isinstance(frame, tuple) else torch.from_numpy(frame).to(DEV)


def same(got, want, what=''):
    torch.cuda.synchronize()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want), what


# ---------------------------------------------------------------- 1. the device computes what the host computes
@pytest.mark.parametrize('dtype', LC.DTYPES)
@pytest.mark.parametrize('name', list(LC.CASES))
def test_letterbox_equals_letterbox_host(pipe, name, dtype):
    frames, opts = LC.CASES[name]
    before = pipe._ring.i
    img, geoms = pipe.letterbox(frames, dtype=TORCH[dtype], device=DEV, **opts)                  # numpy frames: through the staging ring
    same(img, host(name, dtype), 'host frames')
    assert pipe._ring.i == (before + 1) % pipe.STAGES
    assert geoms == host(name, dtype, geometry=True)
    img, _ = pipe.letterbox([to_device(f) for f in frames], dtype=TORCH[dtype], device=DEV, **opts)   # device frames: read in place
    same(img, host(name, dtype), 'device frames')
    assert pipe._ring.i == (before + 1) % pipe.STAGES            # no stage: the descriptor table is all that goes up, once, and is kept
    again, _ = pipe.letterbox(frames, dtype=TORCH[dtype], rgb=not opts.get('rgb', False), device=DEV,
                              **{k: v for k, v in opts.items() if k != 'rgb'})
    if opts.get('pixel_format', 'bgr') == 'bgr':                 # the other channel order is the same planes reversed
        same(again, host(name, dtype).flip(1), 'channel order')


@pytest.mark.parametrize('dtype', LC.DTYPES)
def test_device_frames_with_a_row_pitch_and_mixed_with_host_frames(pipe, dtype):
    frames, opts = LC.CASES['five_sizes']
    views = []
    for junk, f in zip((255, 0, 255, 0, 255), frames):           # views into wider buffers; the padding would change the result if it were read
        h, w, _ = f.shape
        buf = torch.full((h, 3 * w + 13), junk, dtype=torch.uint8, device=DEV)
        view = buf[:, :3 * w].view(h, w, 3)
        view.copy_(torch.from_numpy(f).to(DEV))
        assert view.stride() == (3 * w + 13, 3, 1)
        views.append(view)
    same(pipe.letterbox(views, dtype=TORCH[dtype], device=DEV, **opts)[0], host('five_sizes', dtype), 'pitched views')
    mixed = [views[0], frames[1], views[2], frames[3], to_device(frames[4])]
    same(pipe.letterbox(mixed, dtype=TORCH[dtype], device=DEV, **opts)[0], host('five_sizes', dtype), 'mixed')
    # NV12 planes with their own pitches, and one [3H/2, W] surface
    frames, opts = LC.CASES['nv12_three_sizes_bt709']
    planes = []
    for y, uv in frames:
        h, w = y.shape
        ybuf, uvbuf = torch.full((h, w + 14), 255, dtype=torch.uint8, device=DEV), torch.full((h // 2, w + 6), 255, dtype=torch.uint8, device=DEV)
        ybuf[:, :w], uvbuf[:, :w] = torch.from_numpy(y).to(DEV), torch.from_numpy(uv.reshape(h // 2, w)).to(DEV)
        planes.append((ybuf[:, :w], uvbuf[:, :w]))
    same(pipe.letterbox(planes, dtype=TORCH[dtype], device=DEV, **opts)[0], host('nv12_three_sizes_bt709', dtype), 'pitched planes')
    surfaces = [np.concatenate([y, uv.reshape(y.shape[0] // 2, y.shape[1])]) for y, uv in frames]
    same(pipe.letterbox([surfaces[0], to_device(surfaces[1]), planes[2]], dtype=TORCH[dtype], device=DEV, **opts)[0], host('nv12_three_sizes_bt709', dtype), 'surfaces')


# ---------------------------------------------------------------- 2. the entries through ctypes
def descriptors(frames, geoms, top=None, left=None):
    desc = np.zeros(len(frames), dtype=P._LETTERBOX)
    fd = desc['frame']
    fd['src'] = [f.data_ptr() for f in frames]
    fd['src_h'], fd['src_w'], fd['src_pitch'] = [f.shape[0] for f in frames], [f.shape[1] for f in frames], [f.stride(0) for f in frames]
    fd['out_h'], fd['out_w'] = [g.unpad_h for g in geoms], [g.unpad_w for g in geoms]
    desc['top'], desc['left'] = [g.top for g in geoms] if top is None else top, [g.left for g in geoms] if left is None else left
    return torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(DEV)


@pytest.mark.parametrize('dtype', LC.DTYPES)
@pytest.mark.parametrize('name', ['five_sizes', 'odd_width_out'])
def test_the_entry_writes_all_of_dst_and_nothing_else(name, dtype):
    lib = L.load()
    frames, opts = LC.CASES[name]
    dev_frames = [to_device(f) for f in frames]
    want = host(name, dtype)
    geoms = host(name, dtype, geometry=True)
    table = descriptors(dev_frames, geoms)
    n, guard = want.numel(), 64
    vp = C.c_void_p
    s = vp(torch.cuda.current_stream().cuda_stream)
    # dst aligned to 4 bytes (the wide stores where the width allows them) and, for the 8- and 16-bit outputs, only to its element
    for shift in (0, 1) if dtype != 'float32' else (0,):
        buf = torch.full((guard + shift + n + guard,), 77, dtype=TORCH[dtype], device=DEV)      # 77: not a value byte / 255 takes
        dst = buf[guard + shift:guard + shift + n]
        assert dst.data_ptr() % 4 == (shift * buf.element_size()) % 4
        L.check(lib.mcg_letterbox_frames(s, vp(table.data_ptr()), len(frames), vp(dst.data_ptr()), want.shape[2], want.shape[3], P._LETTERBOX_TYPES[TORCH[dtype]], 1),
                'mcg_letterbox_frames')
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu().view(want.shape), want), shift
        assert (buf[:guard + shift] == 77).all() and (buf[guard + shift + n:] == 77).all()
        assert not (dst == 77).any() or dtype == 'uint8'
    if dtype == 'uint8':                                         # 77 is a byte a frame may hold: an element left alone cannot equal `want` under a second poison too
        buf = torch.full((guard + n + guard,), 141, dtype=torch.uint8, device=DEV)
        L.check(lib.mcg_letterbox_frames(s, vp(table.data_ptr()), len(frames), vp(buf[guard:].data_ptr()), want.shape[2], want.shape[3], L.LETTERBOX_U8, 1), 'mcg_letterbox_frames')
        torch.cuda.synchronize()
        assert torch.equal(buf[guard:guard + n].cpu().view(want.shape), want) and (buf[:guard] == 141).all() and (buf[guard + n:] == 141).all()


def test_a_rectangle_that_does_not_fit_is_clipped_and_an_unreadable_frame_is_all_border():
    lib = L.load()
    frames, opts = LC.CASES['five_sizes']
    dev_frames = [to_device(f) for f in frames]
    geoms, want = host('five_sizes', 'uint8', geometry=True), host('five_sizes', 'uint8')
    # frame 0: its rectangle moved 40 rows down and 30 columns left; frame 1: no rows; frame 2: no columns in the frame; the rest as they are
    table = descriptors(dev_frames, geoms, top=[geoms[0].top + 40] + [g.top for g in geoms[1:]], left=[geoms[0].left - 30] + [g.left for g in geoms[1:]])
    desc = table.cpu().numpy().view(P._LETTERBOX).copy()
    desc['frame']['out_h'][1] = 0
    desc['frame']['src_w'][2] = 0
    table = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(DEV)
    guard, n = 64, want.numel()
    buf = torch.full((guard + n + guard,), 141, dtype=torch.uint8, device=DEV)
    vp = C.c_void_p
    L.check(lib.mcg_letterbox_frames(vp(torch.cuda.current_stream().cuda_stream), vp(table.data_ptr()), 5, vp(buf[guard:].data_ptr()), 64, 64, L.LETTERBOX_U8, 1),
            'mcg_letterbox_frames')
    torch.cuda.synchronize()
    got = buf[guard:guard + n].cpu().view(want.shape)
    assert (buf[:guard] == 141).all() and (buf[guard + n:] == 141).all()
    g = geoms[0]
    moved = torch.full_like(want[0], 114)
    moved[:, g.top + 40:, :g.unpad_w - 30] = want[0][:, g.top:g.top + 64 - (g.top + 40), g.left + 30:g.left + g.unpad_w]
    assert torch.equal(got[0], moved)
    assert (got[1] == 114).all() and (got[2] == 114).all() and torch.equal(got[3:], want[3:])


def test_bad_arguments_are_refused_before_any_launch():
    lib = L.load()
    frames, opts = LC.CASES['wide_37x50']
    dev_frames = [to_device(f) for f in frames]
    table = descriptors(dev_frames, host('wide_37x50', 'float32', geometry=True))
    out = torch.full((3 * 64 * 64 + 1,), -7, dtype=torch.float32, device=DEV)
    vp = C.c_void_p
    s = vp(torch.cuda.current_stream().cuda_stream)
    coef = L.YuvCoef(**P.YUV_COEF['bt601'])

    def call(table_=table.data_ptr(), n=1, dst=out.data_ptr(), out_h=64, out_w=64, out_type=L.LETTERBOX_F32, nv12=False, coef_=coef):
        if nv12:
            return lib.mcg_letterbox_frames_nv12(s, vp(table_), n, vp(dst), out_h, out_w, out_type, 1, None if coef_ is None else C.byref(coef_))
        return lib.mcg_letterbox_frames(s, vp(table_), n, vp(dst), out_h, out_w, out_type, 1)

    err = lambda: lib.mcg_last_error()
    assert call(n=0) == L.MCG_OK                                 # no frames: no launch
    for nv12 in (False, True):
        assert call(table_=None, nv12=nv12) != L.MCG_OK and b'null pointer' in err()
        assert call(dst=None, nv12=nv12) != L.MCG_OK and b'null pointer' in err()
        assert call(n=-1, nv12=nv12) != L.MCG_OK and b'bad sizes' in err()
        assert call(out_h=0, nv12=nv12) != L.MCG_OK and b'bad sizes' in err()
        assert call(out_w=-64, nv12=nv12) != L.MCG_OK and b'bad sizes' in err()
        assert call(out_h=1 << 16, out_w=1 << 15, nv12=nv12) != L.MCG_OK and b'bad sizes' in err()
        assert call(n=65536, nv12=nv12) != L.MCG_OK and b'65535' in err()
        assert call(out_type=3, nv12=nv12) != L.MCG_OK and b'out_type' in err()
        assert call(dst=out.data_ptr() + 2, nv12=nv12) != L.MCG_OK and b'aligned' in err()
        assert call(dst=out.data_ptr() + 1, out_type=L.LETTERBOX_F16, nv12=nv12) != L.MCG_OK and b'aligned' in err()
    assert call(nv12=True, coef_=None) != L.MCG_OK and b'null coef' in err()
    assert call(nv12=True, coef_=L.YuvCoef(**dict(P.YUV_COEF['bt601'], cy=1 << 22))) != L.MCG_OK and b'outside' in err()
    torch.cuda.synchronize()
    assert (out == -7).all()                                     # nothing was launched
    L.check(call(), 'mcg_letterbox_frames')
    torch.cuda.synchronize()
    assert torch.equal(out[:-1].cpu().view(1, 3, 64, 64), host('wide_37x50', 'float32')) and out[-1] == -7


def test_host_arguments_are_checked_before_anything_is_launched(pipe):
    frames, opts = LC.CASES['wide_37x50']
    dev = to_device(frames[0])
    i = pipe._ring.i
    with pytest.raises(ValueError, match='one output shape'):
        pipe.letterbox([dev, to_device(LC.frame(3, 21, 64))], 64, device=DEV)
    with pytest.raises(ValueError):
        pipe.letterbox([], 64, device=DEV)
    with pytest.raises(ValueError):
        pipe.letterbox([dev], 0, device=DEV)
    with pytest.raises(ValueError):
        pipe.letterbox([dev], 64, stride=0, device=DEV)
    y, uv = LC.surface(1, 36, 50)
    with pytest.raises(ValueError):
        pipe.letterbox([(to_device(y[:35]), to_device(uv))], 64, pixel_format='nv12', device=DEV)
    with pytest.raises(ValueError):
        pipe.letterbox([np.zeros((27, 21), np.uint8)], 64, pixel_format='nv12', device=DEV)
    with pytest.raises(TypeError):
        pipe.letterbox([torch.from_numpy(frames[0])], 64, device=DEV)                # a CPU tensor
    with pytest.raises(TypeError):
        pipe.letterbox([(torch.from_numpy(y), torch.from_numpy(uv))], 64, pixel_format='nv12', device=DEV)
    with pytest.raises(TypeError):
        pipe.letterbox([dev.float()], 64, device=DEV)
    with pytest.raises(TypeError):
        pipe.letterbox([frames[0].astype(np.int16)], 64, device=DEV)
    with pytest.raises(TypeError):
        pipe.letterbox([dev], 64, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        pipe.letterbox([dev], 64, pixel_format='rgb', device=DEV)
    with pytest.raises(L.McgError):
        pipe.letterbox([frames[0]], 64, device='cpu')
    assert pipe._ring.i == i                                     # no stage was taken: nothing went up


# ---------------------------------------------------------------- 3. nothing is read on the host
@pytest.mark.parametrize('name', ['five_sizes', 'nv12_three_sizes_bt709'])
def test_letterbox_captures_in_a_graph_and_follows_the_frames(pipe, name):
    frames, opts = LC.CASES[name]
    dev_frames = [to_device(f) for f in frames]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # the eager call uploads the descriptor table, once
        eager, _ = pipe.letterbox(dev_frames, device=DEV, **opts)
    torch.cuda.current_stream().wait_stream(side)
    same(eager, host(name, 'float16'), 'eager')
    cached = (len(pipe._image_tables), pipe._ring.i)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got, _ = pipe.letterbox(dev_frames, device=DEV, **opts)
    assert cached == (len(pipe._image_tables), pipe._ring.i)
    got.fill_(-3)
    graph.replay()
    same(got, host(name, 'float16'), 'replayed')
    # new contents in the same memory: a decoder's buffer ring
    flip = lambda a: np.ascontiguousarray(255 - a)
    new = [tuple(flip(p) for p in f) if isinstance(f, tuple) else flip(f) for f in frames]
    for d, f in zip(dev_frames, new):
        for dp, fp in zip(d, f) if isinstance(f, tuple) else ((d, f),):
            dp.copy_(torch.from_numpy(fp).to(DEV))
    graph.replay()
    same(got, torch.from_numpy(H.letterbox_host(new, **opts)[0]), 'new contents')


# ---------------------------------------------------------------- 4. the live chain, and run_head_video on top
def two_frames():
    """Two 48 x 64 frames in a 128 detector: r = 2, unpad 96 x 128, no pads (tests/test_gpu_detect.py::two_frames' boxes, doubled)."""
    heads = [[(20, 16, 60, 60), (70, 30, 110, 80)], [(8, 10, 40, 50), (60, 40, 120, 90)]]
    pred = np.concatenate([D.rows([h + (0.9, 0, 1) for h in hs] + [(h[0] + 2, h[1], h[2] + 2, h[3], 0.6, 0, 1) for h in hs], n=16) for hs in heads])
    return pred, [LC.frame(70 + k, 48, 64) for k in range(2)]


def test_letterbox_detector_detect_heads_head_crops_without_a_read_back(pipe):
    pred, frames = two_frames()
    dev_frames = [to_device(f) for f in frames]
    prepared = torch.from_numpy(pred).to(DEV)
    seen = []

    def detector(img):                                            # a stand-in network on the device: checks its input, returns a prepared prediction
        assert img.is_cuda and img.dtype == torch.float16 and tuple(img.shape) == (2, 3, 96, 128)
        seen.append(img)
        return prepared, None

    img, geoms = pipe.letterbox(dev_frames, 128, device=DEV)
    raw = detector(img)[0]
    boxes, _, _, image_of, counts, flags = pipe.detect_heads(raw, img.shape[2:], (48, 64), max_det=6)
    got = pipe.head_crops(dev_frames, boxes.view(-1, 4), image_of.view(-1), device=DEV)
    torch.cuda.synchronize()                                      # the first read of anything
    assert [(g.unpad_h, g.unpad_w, g.top, g.left, g.out_h, g.out_w) for g in geoms] == [(96, 128, 0, 0, 96, 128)] * 2
    same(seen[0], torch.from_numpy(H.letterbox_host(frames, 128)[0]), 'what the detector saw')
    assert counts.tolist() == [2, 2] and flags.tolist() == [0, 0]
    assert boxes[0, :2].tolist() == [[10, 8, 30, 30], [35, 15, 55, 40]]
    valid = (image_of.view(-1) >= 0).cpu()
    per_frame = harness.head_boxes_per_frame(boxes, counts)
    want = pipe.head_crops(frames, np.asarray([b for f in per_frame for b in f], np.float32), np.asarray([0, 0, 1, 1], np.int32), device=DEV)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g.cpu()[valid], w.cpu())


def test_run_head_video_runs_the_detector():
    from mcgaze_amd.engine import HipEngine
    e = HipEngine(synth.make_state_dict(0), precision='f16x3')
    pipe = P.DevicePipeline(chain(64))
    h, w = 48, 64
    # frames 0 - 2 are 48 x 64 (letterboxed 96 x 128), frame 3 is 64 x 48 (128 x 96): the group ends early there
    frames = [LC.frame(80 + t, h, w) for t in range(3)] + [LC.frame(83, w, h)]
    heads = [[(8 + t, 6, 30 + t, 30), (36 + t, 20, 60 + t, 44)] for t in range(3)] + [[(6, 8, 30, 30), (20, 36, 44, 60)]]
    heads[2] = heads[2][:1]
    # the rows are in pixels of the letterboxed input: r = 2, no pads
    raw = [D.rows([tuple(2 * v for v in b) + (0.9, 0, 1) for b in hs] + [(2 * b[0] + 2, 2 * b[1], 2 * b[2] + 2, 2 * b[3], 0.5, 0, 1) for b in hs], n=8) for hs in heads]
    groups = [torch.from_numpy(np.concatenate(raw[:3])).to(DEV), torch.from_numpy(raw[3]).to(DEV)]
    seen = []

    def detector(img):
        assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == ((3, 3, 96, 128), (1, 3, 128, 96))[len(seen)]
        seen.append(img.clone())
        return groups[len(seen) - 1]

    records = harness.run_head_video(e, pipe, frames, detections=dict(detector=detector, new_shape=128, dtype=torch.float32, max_det=4), max_len=4)
    assert len(seen) == 2
    same(seen[0], torch.from_numpy(H.letterbox_host(frames[:3], 128, dtype=torch.float32)[0]), 'group 0')
    same(seen[1], torch.from_numpy(H.letterbox_host(frames[3:], 128, dtype=torch.float32)[0]), 'group 1')
    # the same predictions handed over as pred=: one call per in_shape, since pred= takes one in_shape
    want = harness.run_head_video(e, pipe, frames[:3], detections=dict(pred=groups[0], in_shape=(96, 128), max_det=4), max_len=4)
    want_last = harness.run_head_video(e, pipe, frames[3:], detections=dict(pred=groups[1], in_shape=(128, 96), max_det=4), max_len=4)
    per_frame = [[[float(v) for v in b] for b in hs] for hs in heads]
    whole = harness.run_head_video(e, pipe, frames, per_frame, max_len=4)
    assert len(records) == len(whole) == len(want) + len(want_last)
    for g, r in zip(records, whole):
        assert sorted(g) == sorted(r)
        for k in r:
            assert np.array_equal(g[k], r[k]) if isinstance(r[k], np.ndarray) else g[k] == r[k], k
    for g, r in zip(records[:len(want)], want):                    # segments 0 and 1 lie inside the first group
        for k in r:
            assert np.array_equal(g[k], r[k]) if isinstance(r[k], np.ndarray) else g[k] == r[k], k
    with pytest.raises(ValueError, match='detector'):
        harness.run_head_video(e, pipe, frames, detections=dict(detector=detector, pred=groups[0], in_shape=(96, 128)))
    with pytest.raises(ValueError, match='detector'):
        harness.run_head_video(e, pipe, frames, detections=dict(detector=detector, in_shape=(96, 128)))
    assert len(seen) == 2                                         # refused before the detector ran
