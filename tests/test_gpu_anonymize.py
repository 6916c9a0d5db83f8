"""DevicePipeline.anonymize_heads / mcg_anonymize_heads(_nv12) on the device against arrows.anonymize_heads_host (include/mcgaze_hip.h,
"anonymised heads"), byte for byte, padding included: the small pitched frames of tests/draw_cases.py and the 70 x 134 frames of
tests/anonymize_cases.py (more than one tile both ways, cut edge tiles, three kinds of pitch).  Every comparison is array_equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import anonymize_cases as AC
from tests import draw_cases as D
from tests.test_gpu_draw import DEV, FORMATS, IDS, device_frames, expected_buffers, host_frames
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu
JUNK = 171


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(32))


def big_host(fmt):
    return AC.BGR if fmt == 'bgr' else AC.NV12


def big_device(fmt):
    """The 70 x 134 frames in device memory, frame k with pitch kind k, the padding full of JUNK -> (views, buffers)."""
    views, bufs = [], []
    for k in range(3):
        if fmt == 'bgr':
            buf = torch.full((AC.H, AC.BGR_PITCHES[k]), JUNK, dtype=torch.uint8, device=DEV)
            buf[:, :3 * AC.W] = torch.from_numpy(AC.BGR[k].reshape(AC.H, 3 * AC.W)).to(DEV)
            views.append(buf.as_strided((AC.H, AC.W, 3), (AC.BGR_PITCHES[k], 3, 1)))
            bufs.append((buf,))
        else:
            ybuf = torch.full((AC.H, AC.NV12_PITCHES[k][0]), JUNK, dtype=torch.uint8, device=DEV)
            uvbuf = torch.full((AC.H // 2, AC.NV12_PITCHES[k][1]), JUNK, dtype=torch.uint8, device=DEV)
            ybuf[:, :AC.W], uvbuf[:, :AC.W] = torch.from_numpy(AC.NV12[k][0]).to(DEV), torch.from_numpy(AC.NV12[k][1]).to(DEV)
            views.append((ybuf[:, :AC.W], uvbuf[:, :AC.W]))
            bufs.append((ybuf, uvbuf))
    return views, bufs


def big_expected(fmt, want):
    out = []
    for k in range(3):
        if fmt == 'bgr':
            b = np.full((AC.H, AC.BGR_PITCHES[k]), JUNK, np.uint8)
            b[:, :3 * AC.W] = want[k].reshape(AC.H, 3 * AC.W)
            out.append((b,))
        else:
            yb, uvb = np.full((AC.H, AC.NV12_PITCHES[k][0]), JUNK, np.uint8), np.full((AC.H // 2, AC.NV12_PITCHES[k][1]), JUNK, np.uint8)
            yb[:, :AC.W], uvb[:, :AC.W] = want[k][0], want[k][1].reshape(AC.H // 2, AC.W)
            out.append((yb, uvb))
    return out


def same_buffers(bufs, expected, what):
    for k, (bs, es) in enumerate(zip(bufs, expected)):
        for b, e in zip(bs, es):
            assert np.array_equal(b.cpu().numpy(), e), (what, k)


def check_big(pipe, fmt, matrix, boxes, image_of, on_device=(True, True), **kw):
    """In place into the pitched 70 x 134 frames == the twin, padding untouched."""
    views, bufs = big_device(fmt)
    want, want_flags = P.anonymize_heads_host(big_host(fmt), boxes, image_of, pixel_format=fmt, matrix=matrix, **kw)
    b, io = (torch.from_numpy(np.asarray(t)).to(DEV) if there else t for t, there in zip((boxes, image_of), on_device))
    out, flags = pipe.anonymize_heads(views, b, io, pixel_format=fmt, matrix=matrix, device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.tolist() == want_flags.tolist() and all(o is v for o, v in zip(out, views))
    same_buffers(bufs, big_expected(fmt, want), (fmt, kw))
    return want


# ---------------------------------------------------------------- 1. the device writes what the host writes
@pytest.mark.parametrize('cell', [None, 2, 4, 8, 16, 32, 64])
@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_fixed_shifts_on_the_70x134_frames(pipe, fmt, matrix, cell):
    for shape in ('ellipse', 'box'):
        want = check_big(pipe, fmt, matrix, AC.BOXES[AC.SMALL], AC.IMAGE_OF[AC.SMALL], shape=shape, cell=cell)
        assert not all(np.array_equal(w if fmt == 'bgr' else w[0], f if fmt == 'bgr' else f[0]) for w, f in zip(want, big_host(fmt)))


@pytest.mark.parametrize('blocks', [1, 8, 64])
@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_automatic_shifts_modes_expand_and_the_row_over_everything(pipe, fmt, matrix, blocks):
    for mode, expand, rows in (('mosaic', 0.125, slice(None)), ('fill', 0.0, AC.SMALL), ('mosaic', 0.0, AC.SMALL), ('fill', 1.0, slice(None))):
        check_big(pipe, fmt, matrix, AC.BOXES[rows], AC.IMAGE_OF[rows], blocks=blocks, mode=mode, expand=expand, color=(12, 230, 97))


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_300_random_rows_are_more_than_one_descriptor_chunk(pipe, fmt, matrix):
    boxes, image_of = AC.random_rows(300, 3)
    check_big(pipe, fmt, matrix, boxes, image_of)
    check_big(pipe, fmt, matrix, boxes, image_of, shape='box', mode='fill', color=(3, 2, 1))
    check_big(pipe, fmt, matrix, boxes[:257], image_of[:257], cell=8)


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_the_small_pitched_frames_and_the_2x2_frame(pipe, fmt, matrix):
    boxes = np.array([(2.5, 1.0, 11.0, 9.5), (4.0, 3.0, 19.0, 16.0), (0.0, 0.0, 2.0, 2.0), (-3.0, 10.0, 30.0, 45.0), (40.0, 30.0, 47.5, 39.0), (0.2, 0.2, 0.9, 0.9)],
                     dtype=np.float32)
    image_of = np.array([0, 1, 2, 3, 3, 2], dtype=np.int32)
    for kw in (dict(), dict(shape='box', cell=4), dict(mode='fill', color=(200, 100, 50), expand=0.5)):
        views, bufs = device_frames(fmt, JUNK)
        want, want_flags = P.anonymize_heads_host(host_frames(fmt), boxes, image_of, pixel_format=fmt, matrix=matrix, **kw)
        _, flags = pipe.anonymize_heads(views, torch.from_numpy(boxes).to(DEV), torch.from_numpy(image_of).to(DEV), pixel_format=fmt, matrix=matrix, device=DEV, **kw)
        torch.cuda.synchronize()
        assert flags.tolist() == want_flags.tolist() == [0] * 6
        same_buffers(bufs, expected_buffers(fmt, want, JUNK), (fmt, kw))


# ---------------------------------------------------------------- 2. where the tables live, copies, nothing to do
@pytest.mark.parametrize('on_device', [(False, False), (True, False), (False, True)], ids=['host', 'boxes-on-device', 'image_of-on-device'])
@pytest.mark.parametrize('fmt', ['bgr', 'nv12'])
def test_host_and_mixed_tables(pipe, fmt, on_device):
    check_big(pipe, fmt, 'bt601', AC.BOXES, AC.IMAGE_OF, on_device=on_device)


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_copy_leaves_the_source_alone_and_host_frames_go_up(pipe, fmt, matrix):
    views, bufs = big_device(fmt)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    want, _ = P.anonymize_heads_host(big_host(fmt), AC.BOXES, AC.IMAGE_OF, pixel_format=fmt, matrix=matrix)
    as_np = lambda images: [im.cpu().numpy() if fmt == 'bgr' else tuple(p.cpu().numpy() for p in im) for im in images]
    same = lambda got: all(np.array_equal(g, w) if fmt == 'bgr' else (np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])) for g, w in zip(as_np(got), want))
    out, _ = pipe.anonymize_heads(views, AC.BOXES, AC.IMAGE_OF, pixel_format=fmt, matrix=matrix, copy=True, device=DEV)
    torch.cuda.synchronize()
    assert same(out) and all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    out, _ = pipe.anonymize_heads(big_host(fmt), AC.BOXES, AC.IMAGE_OF, pixel_format=fmt, matrix=matrix, device=DEV)      # numpy frames: fresh device tensors
    torch.cuda.synchronize()
    assert same(out)
    # no rows: the frames come back as they are; no frames: an error like the neighbours'
    out, flags = pipe.anonymize_heads(views, np.zeros((0, 4), np.float32), np.zeros(0, np.int32), pixel_format=fmt, matrix=matrix, device=DEV)
    torch.cuda.synchronize()
    assert flags.numel() == 0 and all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    with pytest.raises(ValueError):
        pipe.anonymize_heads([], AC.BOXES, AC.IMAGE_OF, pixel_format=fmt, matrix=matrix, device=DEV)
    for bad in (dict(cell=3), dict(blocks=0), dict(expand=5), dict(shape='x'), dict(mode='blur'), dict(color=(1, 2))):
        with pytest.raises(ValueError):
            pipe.anonymize_heads(views, AC.BOXES, AC.IMAGE_OF, pixel_format=fmt, matrix=matrix, device=DEV, **bad)
    with pytest.raises(ValueError):                               # host rows are checked before anything is launched
        pipe.anonymize_heads(views, np.array([(5, 5, 5, 9)], np.float32), np.zeros(1, np.int32), pixel_format=fmt, matrix=matrix, device=DEV)
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))


# ---------------------------------------------------------------- 3. rows that cannot be used, the plan, the argument checks
@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_flag_rows_from_device_tables_write_nothing(pipe, fmt, matrix):
    boxes, image_of, want_flags = AC.flag_rows(3)
    views, bufs = big_device(fmt)
    ok = np.asarray(want_flags) == 0
    want, _ = P.anonymize_heads_host(big_host(fmt), boxes[ok], image_of[ok], pixel_format=fmt, matrix=matrix)
    _, flags = pipe.anonymize_heads(views, torch.from_numpy(boxes).to(DEV), torch.from_numpy(image_of).to(DEV), pixel_format=fmt, matrix=matrix, device=DEV)
    torch.cuda.synchronize()
    assert flags.tolist() == want_flags
    same_buffers(bufs, big_expected(fmt, want), fmt)
    # nothing but unusable rows: every byte stays
    views, bufs = big_device(fmt)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    _, flags = pipe.anonymize_heads(views, torch.from_numpy(boxes[~ok]).to(DEV), torch.from_numpy(image_of[~ok]).to(DEV), pixel_format=fmt, matrix=matrix, device=DEV)
    torch.cuda.synchronize()
    assert flags.tolist() == [2] * int((~ok).sum()) and all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))


def raw_table(views):
    table = np.zeros(len(views), dtype=P._IMAGE)
    for k, v in enumerate(views):
        table[k] = (v.data_ptr(), v.shape[0], v.shape[1], v.stride(0))
    return torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)


def test_plan_descriptors_and_argument_checks():
    lib = L.load()
    views, bufs = big_device('bgr')
    table_dev = raw_table(views)
    fb, fio, fflags = AC.flag_rows(3)
    b, io = np.concatenate([AC.BOXES, fb]), np.concatenate([AC.IMAGE_OF, fio])
    n = len(b)
    boxes, image_of = torch.from_numpy(b).to(DEV), torch.from_numpy(io).to(DEV)
    plan = torch.full((n, P._ANON_WORDS), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    vp, color = C.c_void_p, (C.c_ubyte * 3)(1, 2, 3)
    s = vp(torch.cuda.current_stream().cuda_stream)

    def call(images=table_dev.data_ptr(), num_images=3, max_h=AC.H, max_w=AC.W, boxes_=boxes.data_ptr(), image_of_=image_of.data_ptr(), n_=n, expand=0.125,
             shape=1, cell_shift=0, blocks=8, mode=0, color_=color, plan_=plan.data_ptr()):
        return lib.mcg_anonymize_heads(s, vp(images), num_images, max_h, max_w, vp(boxes_), vp(image_of_), n_, expand, shape, cell_shift, blocks, mode, color_,
                                       vp(plan_), vp(flags.data_ptr()))

    fields = [f for f, _ in L.AnonDesc._fields_]
    for kw, host_kw in ((dict(), dict()), (dict(shape=0, cell_shift=3, expand=0.0), dict(shape='box', cell=8, expand=0.0)), (dict(blocks=64), dict(blocks=64))):
        L.check(call(**kw), 'mcg_anonymize_heads')
        torch.cuda.synchronize()
        d = plan.cpu().numpy()
        want = P.anonymize_plan_host(b, io, [(AC.H, AC.W)] * 3, **host_kw)
        assert flags.tolist() == want['flag'].tolist() and (kw.get('expand') == 0.0 or flags.tolist() == [0] * len(AC.ROWS) + fflags)   # (without expand 8000 stays inside the bound)
        for j, f in enumerate(fields):
            assert np.array_equal(d[:, j], want[f]), (kw, f)
    err = lambda: lib.mcg_last_error()
    keep = [bs[0].clone() for bs in bufs]
    for bad, text in ((dict(images=None), b'null pointer'), (dict(boxes_=None), b'null pointer'), (dict(image_of_=None), b'null pointer'),
                      (dict(plan_=None), b'null pointer'), (dict(mode=1, color_=None), b'null pointer'), (dict(num_images=0), b'65535 images'),
                      (dict(n_=-1), b'65536'), (dict(n_=65537), b'65536'), (dict(max_h=0), b'8192'), (dict(max_w=8193), b'8192'), (dict(expand=-0.5), b'expand'),
                      (dict(expand=4.5), b'expand'), (dict(expand=float('nan')), b'expand'), (dict(shape=2), b'shape'), (dict(mode=2), b'mode'),
                      (dict(mode=-1), b'mode'), (dict(cell_shift=7), b'cell_shift'), (dict(cell_shift=-1), b'cell_shift'), (dict(blocks=0), b'blocks'),
                      (dict(blocks=65), b'blocks')):
        assert call(**bad) == 1 and text in err(), bad            # MCG_ERR_ARG, before any launch
    assert call(n_=0, boxes_=None, image_of_=None, plan_=None) == L.MCG_OK and call(cell_shift=3, blocks=0) == L.MCG_OK      # blocks is read only where cell_shift == 0
    torch.cuda.synchronize()
    L.check(call(), 'mcg_anonymize_heads')
    # an image larger than (max_h, max_w) is flagged and left alone: with max 64 x 134 every row comes back 2
    for bs, k in zip(bufs, keep):
        bs[0].copy_(k)
    L.check(call(max_h=64), 'mcg_anonymize_heads')
    torch.cuda.synchronize()
    assert flags.tolist() == [2] * n and all(torch.equal(bs[0], k) for bs, k in zip(bufs, keep))
    assert lib.mcg_anonymize_heads_nv12(s, None, 1, 2, 2, vp(boxes.data_ptr()), vp(image_of.data_ptr()), 1, 0.0, 0, 0, 8, 0, None, vp(plan.data_ptr()),
                                        None) == 1 and b'mcg_anonymize_heads_nv12: null pointer' in err()


def test_an_odd_sized_row_of_a_device_nv12_table_is_flagged_and_not_written():
    lib = L.load()
    views, bufs = device_frames('nv12', 255)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    table = np.zeros(2, dtype=P._NV12_IMAGE)
    (y, uv) = views[1]
    table[0] = (y.data_ptr(), uv.data_ptr(), 18, 21, y.stride(0), uv.stride(0))
    table[1] = (y.data_ptr(), uv.data_ptr(), 17, 22, y.stride(0), uv.stride(0))
    table_dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    boxes = torch.tensor([[2, 2, 12, 12], [2, 2, 12, 12]], dtype=torch.float32, device=DEV)
    image_of = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    plan, flags = torch.zeros(2, P._ANON_WORDS, dtype=torch.int32, device=DEV), torch.full((2,), -1, dtype=torch.int32, device=DEV)
    vp = C.c_void_p
    L.check(lib.mcg_anonymize_heads_nv12(vp(torch.cuda.current_stream().cuda_stream), vp(table_dev.data_ptr()), 2, 18, 22, vp(boxes.data_ptr()),
                                         vp(image_of.data_ptr()), 2, 0.125, 1, 0, 8, 0, None, vp(plan.data_ptr()), vp(flags.data_ptr())), 'mcg_anonymize_heads_nv12')
    torch.cuda.synchronize()
    assert flags.tolist() == [2, 2] and all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))


# ---------------------------------------------------------------- 4. nothing is read on the host
@pytest.mark.parametrize('fmt,matrix', [FORMATS[0], FORMATS[2]], ids=[IDS[0], IDS[2]])
def test_anonymize_heads_captures_in_a_graph_and_follows_the_box_tensor(fmt, matrix):
    pipe = P.DevicePipeline(chain(32))
    kw = dict(pixel_format=fmt, matrix=matrix, device=DEV)
    views, bufs = big_device(fmt)
    pristine = [tuple(b.clone() for b in bs) for bs in bufs]
    boxes, image_of = torch.from_numpy(AC.BOXES[AC.SMALL]).to(DEV), torch.from_numpy(AC.IMAGE_OF[AC.SMALL]).to(DEV)
    restore = lambda: [b.copy_(c) for bs, cs in zip(bufs, pristine) for b, c in zip(bs, cs)]
    stage_i = pipe._ring.i
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # eager warm-up: uploads the frame table of these frames, once
        pipe.anonymize_heads(views, boxes, image_of, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert len(pipe._image_tables) == 1 and pipe._ring.i == stage_i
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        restore()
        _, flags = pipe.anonymize_heads(views, boxes, image_of, **kw)
    assert len(pipe._image_tables) == 1 and pipe._ring.i == stage_i      # one cached table; no staging buffer was taken
    moved = AC.BOXES[AC.SMALL] + np.array([7.5, -3.25, 9.0, 2.0], np.float32)
    for b in (AC.BOXES[AC.SMALL], moved):
        boxes.copy_(torch.from_numpy(b).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want, want_flags = P.anonymize_heads_host(big_host(fmt), b, AC.IMAGE_OF[AC.SMALL], pixel_format=fmt, matrix=matrix)
        assert flags.tolist() == want_flags.tolist()
        same_buffers(bufs, big_expected(fmt, want), fmt)


# ---------------------------------------------------------------- 5. end to end
def test_run_head_video_anonymizes_first_and_leaves_frames_and_records_alone():
    """20 device frames -- more than one drawing batch -- through run_head_video(anonymize=, draw=): every annotated frame is
    anonymize_heads_host and then draw_arrows_host over the records' rows, the caller's frames are byte-identical afterwards and the records
    are those of the run without it; with heat and labels the documented order: faces, heat map, arrows, labels."""
    from mcgaze_amd import arrows as AR
    from mcgaze_amd import harness, synth
    from mcgaze_amd.engine import HipEngine
    e = HipEngine(synth.make_state_dict(0), precision='f16x3')
    pipe = P.DevicePipeline(chain(64))
    T, h, w = 20, 70, 134
    assert T > harness.DRAW_FRAMES
    raw = np.random.default_rng(9).integers(0, 256, (T, h, w, 3), dtype=np.uint8)
    frames = [torch.from_numpy(f).to(DEV) for f in raw]
    per_frame = [[[10 + t, 20, 40 + t, 56], [80, 24, 112, 60]] for t in range(12)] + [[[50, 20, 82, 66]] for _ in range(T - 12)]
    with pytest.raises(ValueError):
        harness.run_head_video(e, pipe, frames, per_frame, max_len=4, anonymize=True)
    with pytest.raises(ValueError):
        harness.run_head_video(e, pipe, frames, per_frame, max_len=4, anonymize=dict(cell=5), draw=True)
    plain, drawn = harness.run_head_video(e, pipe, frames, per_frame, max_len=4, draw=dict(min_thickness=2))
    options = dict(blocks=4, expand=0.25)
    records, annotated = harness.run_head_video(e, pipe, frames, per_frame, max_len=4, anonymize=options, draw=dict(min_thickness=2))
    torch.cuda.synchronize()
    assert all(np.array_equal(f.cpu().numpy(), r) for f, r in zip(frames, raw))      # on the copies, in every batch
    assert len(records) == len(plain)
    for g, r in zip(records, plain):
        assert sorted(g) == sorted(r)
        for k in r:
            assert np.array_equal(g[k], r[k]) if isinstance(r[k], np.ndarray) else g[k] == r[k], k

    def rows_of(t):
        here = [(r, r['frame_id'].index(t)) for r in records if t in r['frame_id']]
        return np.stack([r['head_box'][j] for r, j in here]), np.stack([r['fused'][j] for r, j in here])

    changed = 0
    for t in range(T):
        boxes, gaze = rows_of(t)
        under, flags = AR.anonymize_heads_host(raw[t], boxes, **options)
        want, _ = AR.draw_arrows_host(under, boxes, gaze, min_thickness=2)
        assert not flags.any() and np.array_equal(annotated[t].cpu().numpy(), want), t
        changed += not np.array_equal(want, drawn[t].cpu().numpy())
    assert changed == T
    # with heat and labels: faces first, then the heat map, the arrows and the labels
    attention = dict(regions=[[100, 0, w, 40]], expand=0.5)
    heat = dict(cell=4, radius=2, min_level=2, draw=True)
    records, annotated, grid = harness.run_head_video(e, pipe, frames, per_frame, max_len=4, attention=attention, heat=heat, anonymize=True,
                                                      draw=dict(min_thickness=2, labels=True))
    torch.cuda.synchronize()
    assert all(np.array_equal(f.cpu().numpy(), r) for f, r in zip(frames, raw)) and grid.sum() > 0
    for t in range(T):
        boxes, gaze = rows_of(t)
        want, _ = AR.anonymize_heads_host(raw[t], boxes)
        want = AR.draw_heat_host(want, grid, int(grid.max()), 2, period=1, min_level=2)
        want, _ = AR.draw_arrows_host(want, boxes, gaze, min_thickness=2)
        ids = [n + 1 for n, r in enumerate(records) if t in r['frame_id']]
        want, _ = AR.draw_labels_host(want, boxes, None, AR.format_labels_host(np.asarray(ids, np.int32)))
        assert np.array_equal(annotated[t].cpu().numpy(), want), t
