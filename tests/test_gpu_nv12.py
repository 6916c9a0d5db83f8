"""-m gpu: NV12 surfaces through the pixel kernels -- DevicePipeline.head_crops(pixel_format='nv12') (mcg_preprocess_head_crops_nv12),
mcg_preprocess_frames_nv12 through ctypes, and harness.run_head_video on top.

The kernel converts each tap it samples and then runs the unchanged resize, so its output must equal the BGR entry's on the frame
pipeline.nv12_to_bgr makes of the same planes (itself checked against a per-pixel restatement and hand-worked answers in
tests/test_nv12_cpu.py): every comparison is torch.equal, no tolerance anywhere.  Frames, boxes and the hand-worked windows come from
tests/nv12_cases.py.  The flag rows are inputs the entry documents (a box of no extent, an image index one past the table); nothing here
provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import nv12_cases as N
from tests.test_preprocess import NORM

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MATRICES = ['bt601', 'bt709']
NAMES = ('img', 'img_hw', 'scale_factor', 'crop', 'flags')


def chain(scale, to_rgb=True):
    return [dict(type='LoadImageFromFile'), dict(type='Resize', img_scale=(scale, scale), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.0),
            dict(type='Normalize', **dict(NORM, to_rgb=to_rgb)), dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
            dict(type='Collect', keys=['img'])]


def same(a, b, what=''):
    for x, y, name in zip(a, b, NAMES):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu()), (what, name)


def device_planes(k, junk=255):
    """Frame k of the cases in device memory with ITS pitches (tests/nv12_cases.py::PITCHES): views into wider buffers whose padding holds
    `junk`, which no tap may read."""
    (y, uv), (h, w), (py, puv) = N.FRAMES[k], N.SHAPES[k], N.PITCHES[k]
    ybuf = torch.full((h, py), junk, dtype=torch.uint8, device=DEV)
    uvbuf = torch.full((h // 2, puv), junk, dtype=torch.uint8, device=DEV)
    ybuf[:, :w] = torch.from_numpy(y).to(DEV)
    uvbuf[:, :w] = torch.from_numpy(uv.reshape(h // 2, w)).to(DEV)
    return ybuf[:, :w], uvbuf[:, :w]


@pytest.fixture(scope='module')
def bgr_frames():
    """nv12_to_bgr of every frame, per matrix (computed once; read-only)."""
    return {m: [P.nv12_to_bgr(y, uv, m) for y, uv in N.FRAMES] for m in MATRICES}


# ---------------------------------------------------------------- 1. head crops: NV12 equals BGR of the converted frame
@pytest.mark.parametrize('to_rgb', [True, False], ids=['to_rgb', 'bgr_out'])
@pytest.mark.parametrize('matrix', MATRICES)
def test_nv12_head_crops_equal_bgr_head_crops_on_the_converted_frames(bgr_frames, matrix, to_rgb):
    pipe = P.DevicePipeline(chain(32, to_rgb))
    want = pipe.head_crops(bgr_frames[matrix], N.BOXES, N.IMAGE_OF, device=DEV)
    got = pipe.head_crops(N.FRAMES, N.BOXES, N.IMAGE_OF, device=DEV, pixel_format='nv12', matrix=matrix)
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (len(N.CASES), 3, 32, 32) and got[3].cpu().tolist() == N.WINDOWS.tolist()   # the hand-worked windows
    assert got[1].cpu().tolist() == [[32, 32]] * 4 + [[26, 32]] + [[32, 32]] * 3 and got[4].cpu().tolist() == [0] * len(N.CASES)
    same(got, want, 'host planes')
    # rgb= is ignored for NV12: the output order is the config's
    same(pipe.head_crops(N.FRAMES, N.BOXES, N.IMAGE_OF, device=DEV, pixel_format='nv12', matrix=matrix, rgb=True), want, 'rgb=True')
    # device-resident planes with their own pitches (image 1: 32 and 24), read in place; junk in the padding is never sampled
    boxes, image_of = torch.from_numpy(N.BOXES).to(DEV), torch.from_numpy(N.IMAGE_OF).to(DEV)
    for junk in (255, 0):
        planes = [device_planes(k, junk) for k in range(len(N.FRAMES))]
        assert (planes[1][0].stride(0), planes[1][1].stride(0)) == (32, 24)
        same(pipe.head_crops(planes, boxes, image_of, device=DEV, pixel_format='nv12', matrix=matrix), want, f'device planes, padding {junk}')
    same(pipe.head_crops(planes, N.BOXES, N.IMAGE_OF, device=DEV, pixel_format='nv12', matrix=matrix), want, 'device planes, host tables')
    same(pipe.head_crops([planes[0], N.FRAMES[1], planes[2]], boxes, image_of, device=DEV, pixel_format='nv12', matrix=matrix), want, 'mixed')
    # the UV plane as [H/2, W/2, 2] on the device, and every frame as ONE [3H/2, W] surface, on the host and on the device
    pairs = [(torch.from_numpy(y).to(DEV), torch.from_numpy(uv).to(DEV)) for y, uv in N.FRAMES]
    same(pipe.head_crops(pairs, boxes, image_of, device=DEV, pixel_format='nv12', matrix=matrix), want, 'uv [H/2,W/2,2] on the device')
    surfaces = [np.concatenate([y, uv.reshape(y.shape[0] // 2, y.shape[1])]) for y, uv in N.FRAMES]
    assert [s.shape for s in surfaces] == [(18, 16), (27, 22), (3, 2)]
    same(pipe.head_crops(surfaces, N.BOXES, N.IMAGE_OF, device=DEV, pixel_format='nv12', matrix=matrix), want, 'host surfaces')
    same(pipe.head_crops([torch.from_numpy(s).to(DEV) for s in surfaces], boxes, image_of, device=DEV, pixel_format='nv12', matrix=matrix), want,
         'device surfaces')
    torch.cuda.synchronize()


def test_nv12_down_scale_of_the_whole_frame(bgr_frames):
    """img_scale (8, 8): the whole 18 x 22 frame comes out 7 x 8 (f = 8 / 22, int(18 f + 0.5) = 7), a down-scale by 2.75; the 6 x 6 window 3 x 3 -> 8 x 8."""
    pipe = P.DevicePipeline(chain(8))
    rows = [4, 3]
    want = pipe.head_crops(bgr_frames['bt709'], N.BOXES[rows], N.IMAGE_OF[rows], device=DEV)
    got = pipe.head_crops([device_planes(k) for k in range(3)], N.BOXES[rows], N.IMAGE_OF[rows], device=DEV, pixel_format='nv12', matrix='bt709')
    torch.cuda.synchronize()
    assert got[1].cpu().tolist() == [[7, 8], [8, 8]] and got[3].cpu().tolist() == N.WINDOWS[rows].tolist()
    same(got, want)


def test_nv12_flags_from_device_tables(bgr_frames):
    pipe = P.DevicePipeline(chain(32))
    boxes, image_of = torch.from_numpy(N.FLAG_BOXES).to(DEV), torch.from_numpy(N.FLAG_IMAGE_OF).to(DEV)
    want = pipe.head_crops(bgr_frames['bt601'], boxes, image_of, device=DEV)
    got = pipe.head_crops([device_planes(k) for k in range(3)], boxes, image_of, device=DEV, pixel_format='nv12')
    torch.cuda.synchronize()
    assert got[4].cpu().tolist() == N.FLAGS and got[3].cpu().tolist() == N.FLAG_WINDOWS.tolist()
    same(got, want)
    # host tables: the same rows are refused before anything is launched, as for BGR
    for bad in (2, 6):
        with pytest.raises(ValueError):
            pipe.head_crops(N.FRAMES, N.FLAG_BOXES[[0, bad]], N.FLAG_IMAGE_OF[[0, bad]], device=DEV, pixel_format='nv12')
    with pytest.raises(TypeError, match='packed rows'):          # every other byte of a row is no Y plane
        y, uv = device_planes(1)
        pipe.head_crops([(y[:, ::2][:, :10], uv[::1, :10])], boxes[:1], image_of[:1] * 0, device=DEV, pixel_format='nv12')


def test_an_odd_sized_row_of_a_device_image_table_is_flagged_and_not_read():
    """mcg_preprocess_head_crops_nv12 through ctypes (head_crops refuses odd sizes before it builds a table): image rows 1 and 2 of a DEVICE table
    claim 18 x 21 and 17 x 22.  Their crops come back with flag 2 as pixel (0, 0) of image 0, like the crops of an image index past the table,
    and the usable row beside them is untouched."""
    lib = L.load()
    pipe = P.DevicePipeline(chain(32))
    planes = [device_planes(k) for k in range(2)]
    boxes = torch.from_numpy(N.BOXES[[0, 6, 4]]).to(DEV)          # image 0's 5 x 5 window, then two boxes that are fine in an 18 x 22 frame
    want = pipe.head_crops(planes, boxes, torch.tensor([0, 2, 2], dtype=torch.int32, device=DEV), device=DEV, pixel_format='nv12')
    assert want[4].tolist() == [0, 2, 2]
    table = np.zeros(3, dtype=P._NV12_IMAGE)
    (y0, uv0), (y1, uv1) = planes
    table[0] = (y0.data_ptr(), uv0.data_ptr(), 12, 16, y0.stride(0), uv0.stride(0))
    table[1] = (y1.data_ptr(), uv1.data_ptr(), 18, 21, y1.stride(0), uv1.stride(0))
    table[2] = (y1.data_ptr(), uv1.data_ptr(), 17, 22, y1.stride(0), uv1.stride(0))
    table_dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    image_of = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
    n = 3
    img = torch.full((n, 3, 32, 32), float('nan'), device=DEV)
    desc = torch.zeros(n, P._NV12_DESC_WORDS, dtype=torch.int32, device=DEV)
    img_hw, scale = torch.zeros(n, 2, dtype=torch.int32, device=DEV), torch.zeros(n, 4, device=DEV)
    flags = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    mean = (C.c_float * 3)(*NORM['mean'])
    stdinv = (C.c_float * 3)(*[float(np.float32(1.0 / np.float64(np.float32(v)))) for v in NORM['std']])
    vp = C.c_void_p
    L.check(lib.mcg_preprocess_head_crops_nv12(vp(torch.cuda.current_stream().cuda_stream), vp(table_dev.data_ptr()), 3, vp(boxes.data_ptr()), vp(image_of.data_ptr()), n,
                                               0.8, 32, 32, vp(desc.data_ptr()), vp(img_hw.data_ptr()), vp(scale.data_ptr()), vp(flags.data_ptr()), vp(img.data_ptr()),
                                               32, 32, mean, stdinv, 1, C.byref(L.YuvCoef(**P.YUV_COEF['bt601']))), 'mcg_preprocess_head_crops_nv12')
    torch.cuda.synchronize()
    assert flags.tolist() == [0, 2, 2] and desc[:, P._CROP_WORD:P._CROP_WORD + 4].tolist() == [[7, 11, 5, 5], [0, 0, 1, 1], [0, 0, 1, 1]]
    same((img, img_hw, scale, desc[:, P._CROP_WORD:P._CROP_WORD + 4], flags), want)
    # a coefficient no |c| < 2^22 holds is refused, the most negative int included
    for bad in (1 << 22, -(1 << 22), -2 ** 31):
        rc = lib.mcg_preprocess_head_crops_nv12(vp(0), vp(table_dev.data_ptr()), 3, vp(boxes.data_ptr()), vp(image_of.data_ptr()), n, 0.8, 32, 32, vp(desc.data_ptr()),
                                                vp(img_hw.data_ptr()), vp(scale.data_ptr()), vp(flags.data_ptr()), vp(img.data_ptr()), 32, 32, mean, stdinv, 1,
                                                C.byref(L.YuvCoef(16, 1220542, bad, 0, 0, 0)))
        assert rc != L.MCG_OK and b'2^22' in lib.mcg_last_error(), bad


@pytest.mark.parametrize('frames_on', ['host', 'device'])
@pytest.mark.parametrize('fmt', ['bgr', 'nv12'])
@pytest.mark.parametrize('host_table', ['boxes', 'image_of'])
def test_head_crops_with_one_table_on_the_host_and_the_other_on_the_device(bgr_frames, host_table, fmt, frames_on):
    """One host operand beside a device one: every operand must be read where it really is -- the host table at its staged address, the
    device table at its own.  The result is the all-host call's bit for bit, and the call takes exactly one stage."""
    pipe = P.DevicePipeline(chain(32))
    kw = dict(device=DEV, pixel_format=fmt, matrix='bt709')
    host = bgr_frames['bt709'] if fmt == 'bgr' else N.FRAMES
    want = pipe.head_crops(host, N.BOXES, N.IMAGE_OF, **kw)
    if frames_on == 'host':
        frames = host
    else:
        frames = [torch.from_numpy(f).to(DEV) for f in host] if fmt == 'bgr' else [device_planes(k) for k in range(len(N.FRAMES))]
    boxes = N.BOXES if host_table == 'boxes' else torch.from_numpy(N.BOXES).to(DEV)
    image_of = N.IMAGE_OF if host_table == 'image_of' else torch.from_numpy(N.IMAGE_OF).to(DEV)
    before = pipe._ring.i
    got = pipe.head_crops(frames, boxes, image_of, **kw)
    assert pipe._ring.i == (before + 1) % pipe.STAGES
    torch.cuda.synchronize()
    assert got[4].tolist() == [0] * len(N.CASES) and got[3].cpu().tolist() == N.WINDOWS.tolist()
    same(got, want, f'{host_table} on the host, frames on the {frames_on}')


# ---------------------------------------------------------------- 2. nothing is read on the host
def test_nv12_head_crops_capture_in_a_graph_and_reuse_the_frame_table(bgr_frames):
    """Device surfaces and device tables: the first call uploads the frame table (32 bytes per surface), the second finds it -- no pixel, no
    table goes from the host to the device -- and the call is captured in a graph and follows the box tensor, like the BGR one."""
    pipe = P.DevicePipeline(chain(32))
    planes = [device_planes(k) for k in range(3)]
    boxes, image_of = torch.from_numpy(N.BOXES).to(DEV), torch.from_numpy(N.IMAGE_OF).to(DEV)
    want = pipe.head_crops(bgr_frames['bt709'], N.BOXES, N.IMAGE_OF, device=DEV)
    stage_i = pipe._ring.i
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # eager warm-up: uploads the frame table of these surfaces, once
        pipe.head_crops(planes, boxes, image_of, device=DEV, pixel_format='nv12', matrix='bt709')
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(pipe._image_tables) == 1 and pipe._ring.i == stage_i      # one cached table; no staging buffer was taken
    table = next(iter(pipe._image_tables.values()))
    again = pipe.head_crops(planes, boxes, image_of, device=DEV, pixel_format='nv12', matrix='bt709')
    assert len(pipe._image_tables) == 1 and next(iter(pipe._image_tables.values())) is table and pipe._ring.i == stage_i
    same(again, want, 'second call')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pipe.head_crops(planes, boxes, image_of, device=DEV, pixel_format='nv12', matrix='bt709')
    graph.replay()
    torch.cuda.synchronize()
    same(out, want, 'replay')
    order = [1, 0, 3, 2, 6, 5, 4, 7]                           # the same boxes, each still with its frame's partner: rows move
    boxes.copy_(torch.from_numpy(N.BOXES[order]).to(DEV))
    image_of.copy_(torch.from_numpy(N.IMAGE_OF[order]).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    same(out, [t[order] for t in want], 'replay on new boxes')


# ---------------------------------------------------------------- 3. mcg_preprocess_frames_nv12 through ctypes
@pytest.mark.parametrize('matrix', MATRICES)
def test_preprocess_frames_nv12_equals_preprocess_frames_on_the_converted_frame(bgr_frames, matrix):
    lib = L.load()
    k = 1                                                        # the 18 x 22 frame, pitches 32 and 24
    h, w = N.SHAPES[k]
    y, uv = device_planes(k)
    bgr = torch.from_numpy(bgr_frames[matrix][k]).to(DEV)
    # crop y, x, h, w -> out h, w: an odd origin, the whole frame (Resize's 26 x 32), the last pixel, an even origin down-scaled
    rows = [((5, 7, 8, 8), (32, 32)), ((0, 0, 18, 22), (26, 32)), ((17, 21, 1, 1), (32, 32)), ((2, 4, 16, 18), (5, 6))]
    nv, pk = np.zeros(len(rows), dtype=P._NV12_DESC), np.zeros(len(rows), dtype=P._DESC)
    for d in (nv, pk):
        d['src_h'], d['src_w'] = h, w
        for j, f in enumerate(('crop_y', 'crop_x', 'crop_h', 'crop_w')):
            d[f] = [r[0][j] for r in rows]
        d['out_h'], d['out_w'] = [r[1][0] for r in rows], [r[1][1] for r in rows]
    nv['src'], nv['src_pitch'], nv['uv'], nv['uv_pitch'] = y.data_ptr(), y.stride(0), uv.data_ptr(), uv.stride(0)
    pk['src'], pk['src_pitch'] = bgr.data_ptr(), 3 * w
    nv_dev, pk_dev = (torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).to(DEV) for d in (nv, pk))
    mean = (C.c_float * 3)(*NORM['mean'])
    stdinv = (C.c_float * 3)(*[float(np.float32(1.0 / np.float64(np.float32(v)))) for v in NORM['std']])
    coef = L.YuvCoef(**P.YUV_COEF[matrix])
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for to_rgb in (1, 0):
        got = torch.full((len(rows), 3, 32, 32), float('nan'), device=DEV)
        want = torch.full((len(rows), 3, 32, 32), float('nan'), device=DEV)
        L.check(lib.mcg_preprocess_frames_nv12(s, C.c_void_p(nv_dev.data_ptr()), len(rows), C.c_void_p(got.data_ptr()), 32, 32, mean, stdinv, to_rgb, C.byref(coef)),
                'mcg_preprocess_frames_nv12')
        L.check(lib.mcg_preprocess_frames(s, C.c_void_p(pk_dev.data_ptr()), len(rows), C.c_void_p(want.data_ptr()), 32, 32, mean, stdinv, to_rgb), 'mcg_preprocess_frames')
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want).all()) and torch.equal(got, want), to_rgb
        assert float(want[3, :, 5:].abs().max()) == 0.0 and float(want[3, :, :, 6:].abs().max()) == 0.0        # padding below / right of the 5 x 6 output
    # argument checks follow mcg_preprocess_frames: null pointers, sizes, the 65535 limit -- and the coefficient bound
    call = lambda frames, n, c, pad=32: lib.mcg_preprocess_frames_nv12(s, frames, n, C.c_void_p(got.data_ptr()), pad, 32, mean, stdinv, 1, c)
    assert call(None, 1, C.byref(coef)) != L.MCG_OK and b'null pointer' in lib.mcg_last_error()
    assert call(C.c_void_p(nv_dev.data_ptr()), 1, None) != L.MCG_OK and b'null coef' in lib.mcg_last_error()
    assert call(C.c_void_p(nv_dev.data_ptr()), 65536, C.byref(coef)) != L.MCG_OK and b'65535' in lib.mcg_last_error()
    assert call(C.c_void_p(nv_dev.data_ptr()), 1, C.byref(coef), pad=0) != L.MCG_OK and b'bad sizes' in lib.mcg_last_error()
    assert call(C.c_void_p(nv_dev.data_ptr()), 1, C.byref(L.YuvCoef(16, 1 << 22, 0, 0, 0, 0))) != L.MCG_OK and b'2^22' in lib.mcg_last_error()
    assert call(C.c_void_p(nv_dev.data_ptr()), 0, C.byref(coef)) == L.MCG_OK


# ---------------------------------------------------------------- 4. end to end
def test_run_head_video_on_nv12_frames_equals_the_run_on_converted_frames():
    from mcgaze_amd.engine import HipEngine
    e = HipEngine(synth.make_state_dict(0), precision='f16x3')
    h, w = 48, 64
    frames = [N.planes(60 + t, h, w) for t in range(3)]
    per_frame = [[[8 + t, 6, 30 + t, 29.5], [40 + t, 20, 66 + t, 44]] for t in range(3)]      # the second head's window leaves the frame right and below
    pipe = P.DevicePipeline(chain(64))
    want = harness.run_head_video(e, pipe, [P.nv12_to_bgr(y, uv, 'bt709') for y, uv in frames], per_frame, max_len=4)
    surfaces = [torch.from_numpy(np.concatenate([y, uv.reshape(h // 2, w)])).to(DEV) for y, uv in frames]
    for what, src in (('host pairs', frames), ('device surfaces', surfaces)):
        got = harness.run_head_video(e, pipe, src, per_frame, max_len=4, pixel_format='nv12', matrix='bt709')
        assert len(got) == len(want) == 2
        for g, r in zip(got, want):
            assert sorted(g) == sorted(r) and len(g['frame_id']) == 3
            for key in r:
                if isinstance(r[key], np.ndarray):
                    assert g[key].dtype == r[key].dtype and g[key].shape == r[key].shape and np.array_equal(g[key], r[key]), (what, key)
                else:
                    assert g[key] == r[key], (what, key)
    assert any(r['crop'][:, 0].max() + r['crop'][:, 2].max() >= h for r in want)                 # a window clipped by the frame is in the set
