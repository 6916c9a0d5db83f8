"""-m gpu: gaze arrows drawn on the device -- DevicePipeline.draw_arrows (mcg_draw_gaze_arrows, mcg_draw_gaze_arrows_nv12), the entries through
ctypes, and harness.run_head_video(draw=...) on top.

Every comparison is torch.equal / array_equal against pipeline.draw_arrows_host (itself checked against rationals, hand-worked answers and a
cube search in tests/test_draw_cpu.py): no tolerance anywhere.  Frames, rows and flag rows come from tests/draw_cases.py.  The flag rows are
inputs the entries document (a NaN gaze, an infinite box, an image index one past the table, an end point beyond the bound); nothing here
provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import draw_cases as D
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FORMATS = [('bgr', 'bt601'), ('nv12', 'bt601'), ('nv12', 'bt709')]
IDS = ['bgr', 'nv12-bt601', 'nv12-bt709']


def host_frames(fmt):
    return D.BGR_FRAMES if fmt == 'bgr' else D.NV12_FRAMES


def as_arrays(fmt, images):
    """draw_arrows' images -> numpy, in draw_arrows_host's form."""
    if fmt == 'bgr':
        return [im.cpu().numpy() for im in images]
    return [tuple(p.cpu().numpy().reshape(p.shape[0], -1) for p in im) for im in images]


def same_frames(fmt, got, want, what=''):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(as_arrays(fmt, got), want)):
        if fmt == 'bgr':
            assert g.shape == w.shape and np.array_equal(g, w), (what, k)
        else:
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1].reshape(g[1].shape)), (what, k)


def device_frames(fmt, junk):
    """The frames in device memory with THEIR pitches: views into wider buffers whose padding holds `junk`.  -> (views, buffers)."""
    views, bufs = [], []
    for k, (h, w) in enumerate(D.SHAPES):
        if fmt == 'bgr':
            pitch = D.BGR_PITCHES[k]
            buf = torch.full((h, pitch), junk, dtype=torch.uint8, device=DEV)
            buf[:, :3 * w] = torch.from_numpy(D.BGR_FRAMES[k].reshape(h, 3 * w)).to(DEV)
            views.append(buf.as_strided((h, w, 3), (pitch, 3, 1)))
            bufs.append((buf,))
        else:
            (y, uv), (py, puv) = D.NV12_FRAMES[k], D.NV12_PITCHES[k]
            ybuf = torch.full((h, py), junk, dtype=torch.uint8, device=DEV)
            uvbuf = torch.full((h // 2, puv), junk, dtype=torch.uint8, device=DEV)
            ybuf[:, :w] = torch.from_numpy(y).to(DEV)
            uvbuf[:, :w] = torch.from_numpy(uv.reshape(h // 2, w)).to(DEV)
            views.append((ybuf[:, :w], uvbuf[:, :w]))
            bufs.append((ybuf, uvbuf))
    return views, bufs


def expected_buffers(fmt, want, junk):
    """What the buffers of device_frames must hold after the call: the host result inside, `junk` untouched in the padding."""
    out = []
    for k, (h, w) in enumerate(D.SHAPES):
        if fmt == 'bgr':
            b = np.full((h, D.BGR_PITCHES[k]), junk, np.uint8)
            b[:, :3 * w] = want[k].reshape(h, 3 * w)
            out.append((b,))
        else:
            yb, uvb = np.full((h, D.NV12_PITCHES[k][0]), junk, np.uint8), np.full((h // 2, D.NV12_PITCHES[k][1]), junk, np.uint8)
            yb[:, :w], uvb[:, :w] = want[k][0], want[k][1].reshape(h // 2, w)
            out.append((yb, uvb))
    return out


# ---------------------------------------------------------------- 1. the device draws what the host draws
@pytest.mark.parametrize('thickness', [1, 5, 9])
@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_draw_arrows_equals_draw_arrows_host(fmt, matrix, thickness):
    pipe = P.DevicePipeline(chain(32))
    kw = dict(pixel_format=fmt, matrix=matrix, min_thickness=thickness)
    frames = host_frames(fmt)
    want, want_flags = P.draw_arrows_host(frames, D.BOXES, D.GAZE, D.IMAGE_OF, **kw)
    assert want_flags.tolist() == [0] * len(D.ROWS)
    changed = [not np.array_equal(w if fmt == 'bgr' else w[0], f if fmt == 'bgr' else f[0]) for w, f in zip(want, frames)]
    assert all(changed)                                          # every frame of the cases gets an arrow (the 2 x 2 one included)
    # host frames, host tables: staged, drawn into fresh device tensors; the arrays given are untouched
    before = [np.array(f) if fmt == 'bgr' else tuple(np.array(p) for p in f) for f in frames]
    got, flags = pipe.draw_arrows(frames, D.BOXES, D.GAZE, D.IMAGE_OF, device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.dtype == torch.int32 and flags.tolist() == [0] * len(D.ROWS)
    same_frames(fmt, got, want, 'host frames')
    for f, b in zip(frames, before):
        assert np.array_equal(f, b) if fmt == 'bgr' else all(np.array_equal(p, q) for p, q in zip(f, b))
    # device frames with their own pitches, drawn IN PLACE; the padding (255, then 0) is compared byte for byte
    boxes, gaze, image_of = (torch.from_numpy(t).to(DEV) for t in (D.BOXES, D.GAZE, D.IMAGE_OF))
    for junk, tables in ((255, (boxes, gaze, image_of)), (0, (D.BOXES, D.GAZE, D.IMAGE_OF))):      # device tables, then host tables
        views, bufs = device_frames(fmt, junk)
        got, flags = pipe.draw_arrows(views, *tables, device=DEV, **kw)
        torch.cuda.synchronize()
        assert flags.tolist() == [0] * len(D.ROWS) and all(g is v for g, v in zip(got, views))
        for k, (bs, es) in enumerate(zip(bufs, expected_buffers(fmt, want, junk))):
            for b, e in zip(bs, es):
                assert np.array_equal(b.cpu().numpy(), e), (junk, k)
    # copy=True leaves the source untouched
    views, bufs = device_frames(fmt, 7)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    got, _ = pipe.draw_arrows(views, boxes, gaze, image_of, device=DEV, copy=True, **kw)
    torch.cuda.synchronize()
    same_frames(fmt, got, want, 'copy=True')
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    # mixed: some frames on the host, some on the device; per-row colours; rows in another order (the highest row wins: order matters)
    order = np.arange(len(D.ROWS))[::-1].copy()
    want2, _ = P.draw_arrows_host(frames, D.BOXES[order], D.GAZE[order], D.IMAGE_OF[order], color=D.COLORS, **kw)
    views, _ = device_frames(fmt, 9)
    got, _ = pipe.draw_arrows([views[0], frames[1], views[2], frames[3]], D.BOXES[order], gaze[torch.from_numpy(order).to(DEV)], D.IMAGE_OF[order],
                              color=D.COLORS, device=DEV, **kw)
    torch.cuda.synchronize()
    same_frames(fmt, got, want2, 'mixed, per-row colours')
    assert not all(np.array_equal(a if fmt == 'bgr' else a[0], b if fmt == 'bgr' else b[0]) for a, b in zip(want2, want))


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_overlaps_outside_arrows_no_rows_and_the_2x2_frame(fmt, matrix):
    pipe = P.DevicePipeline(chain(32))
    kw = dict(pixel_format=fmt, matrix=matrix)
    frames = host_frames(fmt)
    # two and three overlapping arrows with per-row colours, in both orders
    for rows in ([0, 10], [10, 0], [0, 10, 11], [11, 10, 0]):
        want, _ = P.draw_arrows_host(frames[3:], D.BOXES[rows], D.GAZE[rows], color=D.COLORS[:len(rows)], min_thickness=3, **kw)
        got, flags = pipe.draw_arrows(frames[3:], D.BOXES[rows], D.GAZE[rows], np.zeros(len(rows), np.int32), color=D.COLORS[:len(rows)], min_thickness=3,
                                      device=DEV, **kw)
        torch.cuda.synchronize()
        same_frames(fmt, got, want, rows)
    # one arrow wholly outside: flag 0, nothing changes; a zero-length arrow: a disc
    for row, changes in ((5, False), (6, True)):
        views, bufs = device_frames(fmt, 255)
        keep = [b.clone() for b in bufs[3]]
        want, _ = P.draw_arrows_host(frames[3], D.BOXES[row:row + 1], D.GAZE[row:row + 1], **kw)
        got, flags = pipe.draw_arrows(views[3:], D.BOXES[row:row + 1], D.GAZE[row:row + 1], [0], device=DEV, **kw)
        torch.cuda.synchronize()
        assert flags.tolist() == [0]
        same_frames(fmt, got, [want], row)
        assert all(torch.equal(b, c) for b, c in zip(bufs[3], keep)) != changes
    # no rows: the frames come back as they are (host frames: uploaded)
    got, flags = pipe.draw_arrows(frames, np.zeros((0, 4), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.int32), device=DEV, **kw)
    torch.cuda.synchronize()
    assert tuple(flags.shape) == (0,)
    same_frames(fmt, got, P.draw_arrows_host(frames, np.zeros((0, 4)), np.zeros((0, 2)), **kw)[0], 'no rows')
    # the 2 x 2 frame alone, every thickness up to 9
    for t in (1, 2, 9):
        want, _ = P.draw_arrows_host(frames[2], D.BOXES[9:10], D.GAZE[9:10], min_thickness=t, **kw)
        got, _ = pipe.draw_arrows(frames[2:3], D.BOXES[9:10], D.GAZE[9:10], [0], min_thickness=t, device=DEV, **kw)
        torch.cuda.synchronize()
        same_frames(fmt, got, [want], ('2x2', t))


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_flag_rows_from_device_tables_write_nothing(fmt, matrix):
    pipe = P.DevicePipeline(chain(32))
    kw = dict(pixel_format=fmt, matrix=matrix)
    want, want_flags = P.draw_arrows_host(host_frames(fmt), D.FLAG_BOXES, D.FLAG_GAZE, D.FLAG_IMAGE_OF, **kw)
    assert want_flags.tolist() == D.FLAGS
    boxes, gaze, image_of = (torch.from_numpy(t).to(DEV) for t in (D.FLAG_BOXES, D.FLAG_GAZE, D.FLAG_IMAGE_OF))
    views, bufs = device_frames(fmt, 255)
    got, flags = pipe.draw_arrows(views, boxes, gaze, image_of, device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.tolist() == D.FLAGS
    for k, (bs, es) in enumerate(zip(bufs, expected_buffers(fmt, want, 255))):
        for b, e in zip(bs, es):
            assert np.array_equal(b.cpu().numpy(), e), k
    # only flagged rows: the frames stay byte-identical
    bad = [k for k, f in enumerate(D.FLAGS) if f]
    views, bufs = device_frames(fmt, 0)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    idx = torch.tensor(bad, device=DEV)
    _, flags = pipe.draw_arrows(views, boxes[idx], gaze[idx], image_of[idx], device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.tolist() == [2] * len(bad) and all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    # host tables: the same rows are refused before anything is launched
    for k in bad:
        with pytest.raises(ValueError):
            pipe.draw_arrows(views, D.FLAG_BOXES[[0, k]], D.FLAG_GAZE[[0, k]], D.FLAG_IMAGE_OF[[0, k]], device=DEV, **kw)
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    with pytest.raises(ValueError):
        pipe.draw_arrows(views, D.BOXES[:1], D.GAZE[:1], [0], min_thickness=0, device=DEV, **kw)
    with pytest.raises(TypeError):
        pipe.draw_arrows([np.zeros((4, 4), np.float32)], D.BOXES[:1], D.GAZE[:1], [0], device=DEV)
    with pytest.raises(ValueError):
        pipe.draw_arrows([], D.BOXES[:1], D.GAZE[:1], [0], device=DEV)


@pytest.mark.parametrize('host_table,per_row', [('boxes', False), ('gaze', True), ('image_of', False), (None, True)],
                         ids=['boxes', 'gaze+colours', 'image_of', 'colours'])
@pytest.mark.parametrize('fmt', ['bgr', 'nv12'])
def test_draw_arrows_with_one_table_on_the_host_and_the_rest_on_the_device(fmt, host_table, per_row):
    """One host operand beside device ones (per-row colours are a host operand too): every operand must be read where it really is -- a host
    table at its staged address, a device table at its own.  Device frames drawn in place come out as the all-host call's frames bit for bit,
    and the call takes exactly one stage."""
    pipe = P.DevicePipeline(chain(32))
    kw = dict(device=DEV, pixel_format=fmt, matrix='bt709', color=D.COLORS if per_row else None)
    want, want_flags = pipe.draw_arrows(host_frames(fmt), D.BOXES, D.GAZE, D.IMAGE_OF, **kw)
    tables = dict(boxes=D.BOXES, gaze=D.GAZE, image_of=D.IMAGE_OF)
    tables = {name: t if name == host_table else torch.from_numpy(t).to(DEV) for name, t in tables.items()}
    views, _ = device_frames(fmt, 255)
    before = pipe._ring.i
    got, flags = pipe.draw_arrows(views, tables['boxes'], tables['gaze'], tables['image_of'], **kw)
    assert pipe._ring.i == (before + 1) % pipe.STAGES
    torch.cuda.synchronize()
    assert torch.equal(flags.cpu(), want_flags.cpu()) and flags.tolist() == [0] * len(D.ROWS)
    assert len(got) == len(want) and all(g is v for g, v in zip(got, views))
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b in zip((g,) if fmt == 'bgr' else g, (w,) if fmt == 'bgr' else w):
            assert a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), (host_table, k)


# ---------------------------------------------------------------- 2. the entries through ctypes
def test_plan_descriptors_and_argument_checks():
    lib = L.load()
    views, _ = device_frames('bgr', 255)
    table = np.zeros(len(views), dtype=P._IMAGE)
    for k, v in enumerate(views):
        table[k] = (v.data_ptr(), v.shape[0], v.shape[1], v.stride(0))
    table_dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    b, g, io = (np.concatenate([x, y]) for x, y in ((D.BOXES, D.FLAG_BOXES), (D.GAZE, D.FLAG_GAZE), (D.IMAGE_OF, D.FLAG_IMAGE_OF)))
    n = len(b)
    boxes, gaze, image_of = (torch.from_numpy(t).to(DEV) for t in (b, g, io))
    plan = torch.full((n, P._ARROW_WORDS), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    vp, color = C.c_void_p, (C.c_ubyte * 3)(*P.ARROW_COLOR)
    s = vp(torch.cuda.current_stream().cuda_stream)

    def call(images=table_dev.data_ptr(), num_images=len(views), max_h=40, max_w=48, boxes_=boxes.data_ptr(), stride=3, n_=n, length=1.0, min_t=5, ratio=0.01,
             tip=0.1, color_=color, plan_=plan.data_ptr()):
        return lib.mcg_draw_gaze_arrows(s, vp(images), num_images, max_h, max_w, vp(boxes_), vp(gaze.data_ptr()), stride, vp(image_of.data_ptr()), n_, length,
                                        min_t, ratio, tip, color_, None, vp(plan_), vp(flags.data_ptr()))

    L.check(call(), 'mcg_draw_gaze_arrows')
    torch.cuda.synchronize()
    d = plan.cpu().numpy().view(P._ARROW).reshape(n)
    seg, t, want_flags = P.arrow_segments(b, g)
    want_flags = np.where((io < 0) | (io >= len(views)), 2, want_flags)
    assert flags.tolist() == want_flags.tolist() == [0] * len(D.ROWS) + D.FLAGS
    ok = want_flags == 0
    assert np.array_equal(d['seg'][ok], seg[ok]) and np.array_equal(d['thickness'][ok], t[ok]) and np.array_equal(d['image'][ok], io[ok])
    assert np.array_equal(d['flag'], want_flags) and (d['image'][~ok] == -1).all() and not d['seg'][~ok].any() and not d['thickness'][~ok].any()
    # the clipped box: end points -+ (t + 1) // 2, inside the frame, half open
    for k in np.flatnonzero(ok):
        h, w = D.SHAPES[io[k]]
        r = (int(t[k]) + 1) // 2
        box = (max(seg[k, :, :, 0].min() - r, 0), max(seg[k, :, :, 1].min() - r, 0), min(seg[k, :, :, 0].max() + r + 1, w), min(seg[k, :, :, 1].max() + r + 1, h))
        assert (d['x0'][k], d['y0'][k], d['x1'][k], d['y1'][k]) == box, k
    # argument checks follow mcg_preprocess_head_crops: null pointers, sizes, the row limit, parameter ranges -- each with its text
    err = lambda: lib.mcg_last_error()
    assert call(images=None) != L.MCG_OK and b'null pointer' in err()
    assert call(plan_=None) != L.MCG_OK and b'null pointer' in err()
    assert call(color_=None) != L.MCG_OK and b'null pointer' in err()
    assert call(num_images=0) != L.MCG_OK and b'bad sizes' in err()
    assert call(stride=1) != L.MCG_OK and b'bad sizes' in err()
    assert call(n_=-1) != L.MCG_OK and b'bad sizes' in err()
    assert call(n_=65536) != L.MCG_OK and b'65535' in err()
    assert call(max_h=0) != L.MCG_OK and b'8192' in err()
    assert call(max_w=8193) != L.MCG_OK and b'8192' in err()
    assert call(min_t=0) != L.MCG_OK and b'min_thickness' in err()
    assert call(min_t=256) != L.MCG_OK and b'min_thickness' in err()
    assert call(length=float('inf')) != L.MCG_OK and b'finite' in err()
    assert call(tip=float('nan')) != L.MCG_OK and b'finite' in err()
    assert call(n_=0) == L.MCG_OK
    assert lib.mcg_draw_gaze_arrows_nv12(s, None, 1, 2, 2, vp(boxes.data_ptr()), vp(gaze.data_ptr()), 3, vp(image_of.data_ptr()), 1, 1.0, 5, 0.01, 0.1, color,
                                         None, vp(plan.data_ptr()), None) != L.MCG_OK and b'mcg_draw_gaze_arrows_nv12: null pointer' in err()
    # an image larger than (max_h, max_w) is flagged, not drawn: with max 18 x 22 the 40 x 48 frame's rows come back 2
    keep = views[3].clone()
    L.check(call(max_h=18, max_w=22), 'mcg_draw_gaze_arrows')
    torch.cuda.synchronize()
    assert flags[:len(D.ROWS)].tolist() == [2 if k == 3 else 0 for k in D.IMAGE_OF] and torch.equal(views[3], keep)


def test_an_odd_sized_row_of_a_device_nv12_table_is_flagged_and_not_written():
    lib = L.load()
    views, bufs = device_frames('nv12', 255)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    table = np.zeros(2, dtype=P._NV12_IMAGE)
    (y, uv) = views[1]
    table[0] = (y.data_ptr(), uv.data_ptr(), 18, 21, y.stride(0), uv.stride(0))
    table[1] = (y.data_ptr(), uv.data_ptr(), 17, 22, y.stride(0), uv.stride(0))
    table_dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    boxes, gaze = torch.from_numpy(D.BOXES[[8, 8]]).to(DEV), torch.from_numpy(D.GAZE[[8, 8]]).to(DEV)
    image_of = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    plan, flags = torch.zeros(2, P._ARROW_WORDS, dtype=torch.int32, device=DEV), torch.full((2,), -1, dtype=torch.int32, device=DEV)
    vp = C.c_void_p
    L.check(lib.mcg_draw_gaze_arrows_nv12(vp(torch.cuda.current_stream().cuda_stream), vp(table_dev.data_ptr()), 2, 18, 22, vp(boxes.data_ptr()), vp(gaze.data_ptr()), 3,
                                          vp(image_of.data_ptr()), 2, 1.0, 5, 0.01, 0.1, (C.c_ubyte * 3)(100, 110, 120), None, vp(plan.data_ptr()), vp(flags.data_ptr())),
            'mcg_draw_gaze_arrows_nv12')
    torch.cuda.synchronize()
    assert flags.tolist() == [2, 2] and all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))


# ---------------------------------------------------------------- 3. nothing is read on the host
@pytest.mark.parametrize('fmt,matrix', [FORMATS[0], FORMATS[2]], ids=[IDS[0], IDS[2]])
def test_draw_arrows_captures_in_a_graph_and_follows_the_gaze_tensor(fmt, matrix):
    pipe = P.DevicePipeline(chain(32))
    kw = dict(pixel_format=fmt, matrix=matrix, device=DEV)
    frames = host_frames(fmt)
    views, bufs = device_frames(fmt, 255)
    pristine = [tuple(b.clone() for b in bs) for bs in bufs]
    boxes, image_of = torch.from_numpy(D.BOXES).to(DEV), torch.from_numpy(D.IMAGE_OF).to(DEV)
    store = torch.zeros(len(D.ROWS), 5, device=DEV)                # the gaze as columns 1..3 of a wider table: a row stride of 5 floats
    gaze = store[:, 1:4]
    gaze.copy_(torch.from_numpy(D.GAZE).to(DEV))
    restore = lambda: [b.copy_(c) for bs, cs in zip(bufs, pristine) for b, c in zip(bs, cs)]
    stage_i = pipe._ring.i
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # eager warm-up: uploads the frame table of these frames, once
        pipe.draw_arrows(views, boxes, gaze, image_of, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(pipe._image_tables) == 1 and pipe._ring.i == stage_i
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        restore()
        _, flags = pipe.draw_arrows(views, boxes, gaze, image_of, **kw)
    assert len(pipe._image_tables) == 1 and pipe._ring.i == stage_i      # one cached table; no staging buffer was taken
    for g in (D.GAZE, -D.GAZE[::-1].copy()):
        gaze.copy_(torch.from_numpy(g).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want, want_flags = P.draw_arrows_host(frames, D.BOXES, g, D.IMAGE_OF, pixel_format=fmt, matrix=matrix)
        assert flags.tolist() == want_flags.tolist()
        for k, (bs, es) in enumerate(zip(bufs, expected_buffers(fmt, want, 255))):
            for b, e in zip(bs, es):
                assert np.array_equal(b.cpu().numpy(), e), k


# ---------------------------------------------------------------- 4. end to end
def test_run_head_video_draws_its_own_arrows():
    from mcgaze_amd.engine import HipEngine
    from tests import nv12_cases as N
    e = HipEngine(synth.make_state_dict(0), precision='f16x3')
    h, w = 48, 64
    nv12 = [N.planes(60 + t, h, w) for t in range(3)]
    per_frame = [[[8 + t, 6, 30 + t, 29.5], [40 + t, 20, 66 + t, 44]] for t in range(3)]      # the second head's window leaves the frame right and below
    pipe = P.DevicePipeline(chain(64))
    for fmt, matrix, frames in (('bgr', 'bt601', [P.nv12_to_bgr(y, uv, 'bt709') for y, uv in nv12]), ('nv12', 'bt709', nv12)):
        kw = dict(max_len=4, pixel_format=fmt, matrix=matrix)
        plain = harness.run_head_video(e, pipe, frames, per_frame, **kw)
        for smooth, key in ((None, 'fused'), (0.6, 'fused_smooth')):
            ref = plain if smooth is None else harness.run_head_video(e, pipe, frames, per_frame, smooth=smooth, **kw)
            records, annotated = harness.run_head_video(e, pipe, frames, per_frame, smooth=smooth, draw=dict(min_thickness=2), **kw)
            torch.cuda.synchronize()
            assert len(records) == len(ref) == 2 and len(annotated) == 3
            for g, r in zip(records, ref):                        # the records are those of the run without drawing, key for key
                assert sorted(g) == sorted(r)
                for k in r:
                    assert np.array_equal(g[k], r[k]) if isinstance(r[k], np.ndarray) else g[k] == r[k], (fmt, smooth, k)
            for t in range(3):
                boxes = np.stack([r['head_box'][t] for r in records])
                gaze = np.stack([r[key][t] for r in records])
                want, flags = P.draw_arrows_host(frames[t], boxes, gaze, pixel_format=fmt, matrix=matrix, min_thickness=2)
                assert not flags.any()
                same_frames(fmt, annotated[t:t + 1], [want], (fmt, smooth, t))
                # the drawn shaft ends are the records' arrows
                assert np.array_equal(P.arrow_segments(boxes, gaze)[0][:, 0], np.stack([r['arrow'][t] for r in records]))
        assert not any(np.array_equal(a if fmt == 'bgr' else a[0], f if fmt == 'bgr' else f[0]) for a, f in zip(as_arrays(fmt, annotated), frames))
    # draw=True: the demo's parameters (thickness 5), here on the NV12 frames; the host arrays given are left alone
    records, annotated = harness.run_head_video(e, pipe, nv12, per_frame, draw=True, **kw)
    torch.cuda.synchronize()
    for t in range(3):
        want, _ = P.draw_arrows_host(nv12[t], np.stack([r['head_box'][t] for r in records]), np.stack([r['fused'][t] for r in records]),
                                     pixel_format='nv12', matrix='bt709')
        same_frames('nv12', annotated[t:t + 1], [want], ('draw=True', t))
    # device frames: drawn into clones by default, IN PLACE with copy=False in the dict -- then annotated[t] is the tensor that was given
    bgr = [P.nv12_to_bgr(y, uv, 'bt709') for y, uv in nv12]
    for copy in (True, False):
        dev_frames = [torch.from_numpy(f).to(DEV) for f in bgr]
        draw = dict(color=(1, 2, 3)) if copy else dict(color=(1, 2, 3), copy=False)
        records, annotated = harness.run_head_video(e, pipe, dev_frames, per_frame, max_len=4, draw=draw)
        torch.cuda.synchronize()
        for t in range(3):
            want, _ = P.draw_arrows_host(bgr[t], np.stack([r['head_box'][t] for r in records]), np.stack([r['fused'][t] for r in records]), color=(1, 2, 3))
            assert np.array_equal(annotated[t].cpu().numpy(), want) and not np.array_equal(want, bgr[t]), (copy, t)
            assert (annotated[t] is dev_frames[t]) == (not copy)
            assert np.array_equal(dev_frames[t].cpu().numpy(), bgr[t] if copy else want), (copy, t)
