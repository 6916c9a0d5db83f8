"""-m gpu: text labels on the device -- DevicePipeline.draw_labels (mcg_draw_labels, mcg_draw_labels_nv12), DevicePipeline.format_labels
(mcg_format_labels) and the entries through ctypes.

Every comparison is array_equal against arrows.draw_labels_host / format_labels_host (themselves checked against hand-worked pixels, a scalar
restatement and str() in tests/test_labels_cpu.py): no tolerance anywhere.  Scenes come from tests/labels_cases.py over the frames of
tests/draw_cases.py.  The flag rows are table contents the entries document (a box that is not finite or beyond +-8191, an image index outside
the table, an odd-sized NV12 image); nothing here provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import arrows as R
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from mcgaze_amd.nv12 import bgr_to_yuv
from tests import draw_cases as D
from tests import labels_cases as LC
from tests.test_gpu_draw import FORMATS, IDS, as_arrays, device_frames, expected_buffers, host_frames
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(32))


def buffers_equal(fmt, bufs, want, junk, what=''):
    for k, (bs, es) in enumerate(zip(bufs, expected_buffers(fmt, want, junk))):
        for b, e in zip(bs, es):
            assert np.array_equal(b.cpu().numpy(), e), (what, k)


def device_colors(fmt, matrix, colors):
    """Per-row colours as a DEVICE table: read as they are, so (Y, U, V) for NV12."""
    return dev(colors if fmt == 'bgr' else np.stack([bgr_to_yuv(c, matrix) for c in colors]).astype(np.uint8))


# ---------------------------------------------------------------- 1. the device draws what the host draws
@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_draw_labels_equals_draw_labels_host(pipe, fmt, matrix):
    kw = dict(pixel_format=fmt, matrix=matrix, scale=1, place=LC.PLACE)
    frames = host_frames(fmt)
    want, want_flags = R.draw_labels_host(frames, LC.BOXES, LC.IMAGE_OF, LC.TEXT, colors=LC.COLORS, **kw)
    assert want_flags.tolist() == LC.FLAGS
    assert all(not np.array_equal(w if fmt == 'bgr' else w[0], f if fmt == 'bgr' else f[0]) for w, f in zip(want, frames))     # every frame gets a label
    # host frames, host tables: staged, drawn into fresh device tensors; the arrays given are untouched
    before = [np.array(f) if fmt == 'bgr' else tuple(np.array(p) for p in f) for f in frames]
    got, flags = pipe.draw_labels(frames, LC.BOXES, LC.IMAGE_OF, LC.TEXT, colors=LC.COLORS, device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.dtype == torch.int32 and flags.tolist() == LC.FLAGS
    LC.same(fmt, as_arrays(fmt, got), want, 'host frames')
    for f, b in zip(frames, before):
        assert np.array_equal(f, b) if fmt == 'bgr' else all(np.array_equal(p, q) for p, q in zip(f, b))
    # device frames with their own pitches, drawn IN PLACE; the padding (255, then 0) is compared byte for byte
    tables = (dev(LC.BOXES), dev(LC.IMAGE_OF), dev(LC.TEXT))
    for junk, t, colors, place in ((255, tables, device_colors(fmt, matrix, LC.COLORS), dev(LC.PLACE)), (0, (LC.BOXES, LC.IMAGE_OF, LC.TEXT), LC.COLORS, LC.PLACE)):
        views, bufs = device_frames(fmt, junk)
        got, flags = pipe.draw_labels(views, *t, colors=colors, device=DEV, **dict(kw, place=place))
        torch.cuda.synchronize()
        assert flags.tolist() == LC.FLAGS and all(g is v for g, v in zip(got, views))
        buffers_equal(fmt, bufs, want, junk)
    # copy=True leaves the source untouched; one colour for every row, no plates, the default scale
    views, bufs = device_frames(fmt, 7)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    want1, _ = R.draw_labels_host(frames, LC.BOXES, LC.IMAGE_OF, LC.TEXT, color=(3, 200, 100), background=None, pixel_format=fmt, matrix=matrix)
    got, _ = pipe.draw_labels(views, *tables, color=(3, 200, 100), background=None, pixel_format=fmt, matrix=matrix, copy=True, device=DEV)
    torch.cuda.synchronize()
    LC.same(fmt, as_arrays(fmt, got), want1, 'copy=True')
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    # rows in another order (the highest row wins: order matters), some frames on the host
    order = np.arange(len(LC.ROWS))[::-1].copy()
    want2, _ = R.draw_labels_host(frames, LC.BOXES[order], LC.IMAGE_OF[order], LC.TEXT[order], colors=LC.COLORS, **dict(kw, place=LC.PLACE[order]))
    views, _ = device_frames(fmt, 9)
    got, _ = pipe.draw_labels([views[0], frames[1], views[2], frames[3]], LC.BOXES[order], LC.IMAGE_OF[order], dev(LC.TEXT[order]), colors=LC.COLORS, device=DEV,
                              **dict(kw, place=LC.PLACE[order]))
    torch.cuda.synchronize()
    LC.same(fmt, as_arrays(fmt, got), want2, 'reversed, mixed')
    assert not np.array_equal(want2[3] if fmt == 'bgr' else want2[3][0], want[3] if fmt == 'bgr' else want[3][0])
    # no rows: the frames come back as they are
    got, flags = pipe.draw_labels(frames, np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros((0, 24), np.uint8), device=DEV, pixel_format=fmt, matrix=matrix)
    torch.cuda.synchronize()
    assert tuple(flags.shape) == (0,)
    LC.same(fmt, as_arrays(fmt, got), [f if fmt == 'bgr' else tuple(f) for f in frames], 'no rows')


@pytest.mark.parametrize('scale,advance,pad,background', [(1, 6, 1, True), (2, 6, 1, True), (3, 1, 0, False), (16, 8, 1, True), (1, 8, 0, False),
                                                           (2, 6, 0, True), (16, 1, 1, False)])
@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_scales_advances_pads_and_plates(pipe, fmt, matrix, scale, advance, pad, background):
    kw = dict(colors=LC.COLORS, background=(9, 8, 7) if background else None, scale=scale, advance=advance, pad=pad, place=LC.PLACE, pixel_format=fmt,
              matrix=matrix)
    frames = host_frames(fmt)
    want, want_flags = R.draw_labels_host(frames, LC.BOXES, LC.IMAGE_OF, LC.TEXT, **kw)
    views, bufs = device_frames(fmt, 255)
    _, flags = pipe.draw_labels(views, LC.BOXES, LC.IMAGE_OF, LC.TEXT, device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.tolist() == want_flags.tolist() == LC.FLAGS
    buffers_equal(fmt, bufs, want, 255, (scale, advance, pad))


@pytest.mark.parametrize('n', [63, 64, 65])
@pytest.mark.parametrize('fmt,matrix', [FORMATS[0], FORMATS[2]], ids=[IDS[0], IDS[2]])
def test_63_64_65_rows_with_every_flag_from_device_tables(pipe, fmt, matrix, n):
    """The gather kernel ballots 64 plan records at a time: one short of a slice, a slice, one past it.  Random rows that overlap, with boxes
    wholly outside the frames and rows of every flag."""
    boxes, image_of, text, place = LC.random_tables(100 + n, n, D.SHAPES)
    colors = np.random.RandomState(n).randint(0, 256, (n, 3)).astype(np.uint8)
    kw = dict(background=(20, 30, 40), scale=1, pixel_format=fmt, matrix=matrix)
    want, want_flags = R.draw_labels_host(host_frames(fmt), boxes, image_of, text, colors=colors, place=place, **kw)
    assert {0, 1, 2} <= set(want_flags.tolist())
    views, bufs = device_frames(fmt, 255)
    _, flags = pipe.draw_labels(views, dev(boxes), dev(image_of), dev(text), colors=device_colors(fmt, matrix, colors), place=dev(place), device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.tolist() == want_flags.tolist()
    buffers_equal(fmt, bufs, want, 255, n)


@pytest.mark.parametrize('fmt,matrix,h,w', [('bgr', 'bt601', 9, 33), ('nv12', 'bt709', 18, 66)], ids=['bgr-33x9', 'nv12-66x18'])
def test_frames_one_cell_past_a_tile(pipe, fmt, matrix, h, w):
    rs = np.random.RandomState(h)
    frame = rs.randint(0, 256, (h, w, 3)).astype(np.uint8) if fmt == 'bgr' else (rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w)).astype(np.uint8))
    text = R.encode_labels(['#12 3.4s', 'Wg', '|'])
    boxes = np.array([(0, 0, 5, 5), (w - 3, h - 1, w, h), (w - 1, 0, w, 1)], np.float32)      # the last column and row of the frame are written
    for scale, pad in ((1, 0), (1, 1), (2, 1)):
        kw = dict(scale=scale, pad=pad, advance=6, color=(250, 5, 90), background=(1, 2, 3), pixel_format=fmt, matrix=matrix)
        want, want_flags = R.draw_labels_host([frame], boxes, np.zeros(3, np.int32), text, **kw)
        got, flags = pipe.draw_labels([frame], boxes, np.zeros(3, np.int32), text, device=DEV, **kw)
        torch.cuda.synchronize()
        assert flags.tolist() == want_flags.tolist() == [0, 0, 0]
        LC.same(fmt, as_arrays(fmt, got), want, (scale, pad))
        last = want[0] if fmt == 'bgr' else want[0][0]
        assert not np.array_equal(last[:, w - 1], (frame if fmt == 'bgr' else frame[0])[:, w - 1])


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_text_codes_and_lengths(pipe, fmt, matrix):
    """Codes 0, 31, 32, 126, 127 and 255; lengths 0, 1, 23 and 24 with no terminator -- on a frame wide enough for 24 characters."""
    n = len(LC.CODE_TEXT)
    h, w = 6 * 12, 160
    rs = np.random.RandomState(2)
    frame = rs.randint(0, 256, (h, w, 3)).astype(np.uint8) if fmt == 'bgr' else (rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w)).astype(np.uint8))
    boxes = np.array([(3, 12 * k, 10, 12 * k + 2) for k in range(n)], np.float32)
    kw = dict(scale=1, place=np.ones(n, np.int32), color=(255, 255, 255), pixel_format=fmt, matrix=matrix)
    want, want_flags = R.draw_labels_host([frame], boxes, np.zeros(n, np.int32), LC.CODE_TEXT, **kw)
    got, flags = pipe.draw_labels([frame], dev(boxes), dev(np.zeros(n, np.int32)), dev(LC.CODE_TEXT), device=DEV, **dict(kw, place=dev(kw['place'])))
    torch.cuda.synchronize()
    assert flags.tolist() == want_flags.tolist() == [0, 0, 1, 0, 0, 0]
    LC.same(fmt, as_arrays(fmt, got), want)


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_flag_rows_from_device_tables_write_nothing(pipe, fmt, matrix):
    kw = dict(pixel_format=fmt, matrix=matrix, scale=1)
    want, want_flags = R.draw_labels_host(host_frames(fmt), LC.FLAG_BOXES, LC.FLAG_IMAGE_OF, LC.FLAG_TEXT, **kw)
    assert want_flags.tolist() == LC.FLAG_FLAGS
    boxes, image_of, text = dev(LC.FLAG_BOXES), dev(LC.FLAG_IMAGE_OF), dev(LC.FLAG_TEXT)
    views, bufs = device_frames(fmt, 255)
    _, flags = pipe.draw_labels(views, boxes, image_of, text, device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.tolist() == LC.FLAG_FLAGS
    buffers_equal(fmt, bufs, want, 255)
    # only flagged rows, and empty labels: the frames stay byte-identical
    bad = [k for k, f in enumerate(LC.FLAG_FLAGS) if f]
    views, bufs = device_frames(fmt, 0)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    idx = torch.tensor(bad, device=DEV)
    _, flags = pipe.draw_labels(views, boxes[idx], image_of[idx], text[idx], device=DEV, **kw)
    _, empty = pipe.draw_labels(views, boxes[:1], image_of[:1], torch.zeros(1, 24, dtype=torch.uint8, device=DEV), device=DEV, **kw)
    torch.cuda.synchronize()
    assert flags.tolist() == [2] * len(bad) and empty.tolist() == [1]
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    # host tables: the same rows are refused before anything is launched, and so are bad parameters
    for k in bad:
        with pytest.raises(ValueError):
            pipe.draw_labels(views, LC.FLAG_BOXES[[0, k]], LC.FLAG_IMAGE_OF[[0, k]], LC.FLAG_TEXT[[0, k]], device=DEV, **kw)
    for more in (dict(scale=0), dict(advance=9), dict(pad=9), dict(color=LC.COLORS[:2]), dict(colors=(1, 2, 3)), dict(background=(1, 2)), dict(place=[1])):
        with pytest.raises(ValueError):
            pipe.draw_labels(views, LC.FLAG_BOXES[:2], LC.FLAG_IMAGE_OF[[0, 0]], LC.FLAG_TEXT[:2], device=DEV, **dict(kw, **more))
    with pytest.raises(ValueError):
        pipe.draw_labels(views, LC.FLAG_BOXES[:2], LC.FLAG_IMAGE_OF[[0, 0]], np.zeros((2, 23), np.uint8), device=DEV, **kw)
    with pytest.raises(ValueError):
        pipe.draw_labels(views, boxes[:2], image_of[:2], text[:1], device=DEV, **kw)
    with pytest.raises(TypeError):
        pipe.draw_labels(views, LC.FLAG_BOXES[:1], [0.5], LC.FLAG_TEXT[:1], device=DEV, **kw)
    with pytest.raises(ValueError):
        pipe.draw_labels([], LC.FLAG_BOXES[:1], [0], LC.FLAG_TEXT[:1], device=DEV)
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))


@pytest.mark.parametrize('host_table', ['boxes', 'image_of', 'text', 'place', 'colors'])
@pytest.mark.parametrize('fmt', ['bgr', 'nv12'])
def test_one_table_on_the_host_and_the_rest_on_the_device(pipe, fmt, host_table):
    """Every operand must be read where it really is -- a host table at its staged address, a device table at its own -- and the call takes
    exactly one stage."""
    matrix = 'bt709'
    kw = dict(pixel_format=fmt, matrix=matrix, scale=1)
    want, want_flags = R.draw_labels_host(host_frames(fmt), LC.BOXES, LC.IMAGE_OF, LC.TEXT, colors=LC.COLORS, place=LC.PLACE, **kw)
    host = dict(boxes=LC.BOXES, image_of=LC.IMAGE_OF, text=LC.TEXT, place=LC.PLACE, colors=LC.COLORS)
    t = {k: v if k == host_table else device_colors(fmt, matrix, v) if k == 'colors' else dev(v) for k, v in host.items()}
    views, bufs = device_frames(fmt, 255)
    before = pipe._ring.i
    got, flags = pipe.draw_labels(views, t['boxes'], t['image_of'], t['text'], colors=t['colors'], place=t['place'], device=DEV, **kw)
    assert pipe._ring.i == (before + 1) % pipe.STAGES
    torch.cuda.synchronize()
    assert flags.tolist() == want_flags.tolist()
    buffers_equal(fmt, bufs, want, 255, host_table)


# ---------------------------------------------------------------- 2. the format entry
@pytest.mark.parametrize('n', [255, 256, 257])
def test_format_labels_equals_format_labels_host(pipe, n):
    rs = np.random.RandomState(n)
    ids = rs.randint(-3, 2000, n).astype(np.int32)
    values = rs.randint(-2, 100000, n).astype(np.int32)
    ids[:6], values[:6] = (0, -1, 1, 9, 10, 2147483647), (5, 5, 0, 1, 299, 2147483647)
    for rate in ((30, 1), (30000, 1001), (1, 1), (1 << 20, 1)):
        want = R.format_labels_host(ids, values, rate)
        assert np.array_equal(pipe.format_labels(ids, values, rate=rate, device=DEV).cpu().numpy(), want), rate
        assert np.array_equal(pipe.format_labels(dev(ids), dev(values), rate=rate, device=DEV).cpu().numpy(), want), rate
    assert np.array_equal(pipe.format_labels(dev(ids), device=DEV).cpu().numpy(), R.format_labels_host(ids))
    # out=: the tail of a larger text table; nothing else of it is written
    table = torch.full((n + 9, 24), 77, dtype=torch.uint8, device=DEV)
    out = pipe.format_labels(ids, dev(values), rate=(25, 1), out=table[7:7 + n], device=DEV)
    torch.cuda.synchronize()
    assert out.data_ptr() == table[7].data_ptr() and np.array_equal(table[7:7 + n].cpu().numpy(), R.format_labels_host(ids, values, (25, 1)))
    assert (table[:7] == 77).all() and (table[7 + n:] == 77).all()
    for bad in (dict(rate=(1, 2)), dict(rate=(0, 0)), dict(out=table[:n, :23]), dict(out=torch.zeros(n, 24, dtype=torch.uint8)), dict(values=values[:5])):
        with pytest.raises(ValueError):
            pipe.format_labels(ids, **dict(dict(values=values, device=DEV), **bad))
    with pytest.raises(TypeError):
        pipe.format_labels(ids.astype(np.float32), device=DEV)
    assert tuple(pipe.format_labels(np.zeros(0, np.int32), device=DEV).shape) == (0, 24)


def test_formatted_labels_are_drawn_as_their_strings(pipe):
    ids, values = np.array([12, 0, 7], np.int32), np.array([102, 50, 0], np.int32)
    text = pipe.format_labels(dev(ids), dev(values), rate=(30, 1), device=DEV)
    boxes = np.array([(2, 14, 9, 20), (2, 30, 9, 35), (30, 30, 40, 39)], np.float32)
    frame = D.BGR_FRAMES[3]
    got, flags = pipe.draw_labels([frame], boxes, np.zeros(3, np.int32), text, scale=1, device=DEV)
    want, _ = R.draw_labels_host(frame, boxes, None, R.encode_labels(['#12 3.4s', '', '#7']), scale=1)
    torch.cuda.synchronize()
    assert flags.tolist() == [0, 1, 0] and np.array_equal(got[0].cpu().numpy(), want)


# ---------------------------------------------------------------- 3. nothing is read on the host
def test_device_tables_with_no_host_touch_captured_and_replayed_twice(monkeypatch):
    pipe = P.DevicePipeline(chain(32))
    fmt, matrix, n = 'nv12', 'bt709', 20
    cases = [LC.random_tables(s, n, D.SHAPES) for s in (31, 32, 33)]
    colors = [np.random.RandomState(s).randint(0, 256, (n, 3)).astype(np.uint8) for s in (31, 32, 33)]
    views, bufs = device_frames(fmt, 255)
    pristine = [tuple(b.clone() for b in bs) for bs in bufs]
    t = [dev(a) for a in cases[0]] + [device_colors(fmt, matrix, colors[0])]
    kw = dict(background=(5, 6, 7), scale=1, pixel_format=fmt, matrix=matrix)
    call = lambda: pipe.draw_labels(views, t[0], t[1], t[2], place=t[3], colors=t[4], device=DEV, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                    # warm-up outside the capture: uploads the frame table and the font, once
    torch.cuda.synchronize()
    stage_i = pipe._ring.i

    def refuse(*a, **k):
        raise AssertionError('the call touched the host')

    for owner, name in ((torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'), (torch.cuda, 'synchronize'),
                        (torch.cuda.Stream, 'synchronize')):
        monkeypatch.setattr(owner, name, refuse)
    with torch.cuda.stream(side):
        call()
        pipe.format_labels(t[1], t[1], out=t[2], device=DEV)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert pipe._ring.i == stage_i and len(pipe._image_tables) == 1 and len(pipe._label_fonts) == 1      # no staging buffer was taken
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for bs, cs in zip(bufs, pristine):
            for b, c in zip(bs, cs):
                b.copy_(c)
        _, flags = call()
    for case, col in zip(cases[1:], colors[1:]):
        for dst, src in zip(t, [dev(a) for a in case] + [device_colors(fmt, matrix, col)]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        want, want_flags = R.draw_labels_host(host_frames(fmt), case[0], case[1], case[2], place=case[3], colors=col, **kw)
        assert flags.tolist() == want_flags.tolist()
        buffers_equal(fmt, bufs, want, 255)


# ---------------------------------------------------------------- 4. the entries through ctypes
def test_the_entries_through_ctypes_between_guard_words():
    lib = L.load()
    views, bufs = device_frames('bgr', 255)
    table = np.zeros(len(views), dtype=P._IMAGE)
    for k, v in enumerate(views):
        table[k] = (v.data_ptr(), v.shape[0], v.shape[1], v.stride(0))
    table_dev = dev(table.view(np.uint8).reshape(-1).copy())
    b, io, tx = (np.concatenate([x, y]) for x, y in ((LC.BOXES, LC.FLAG_BOXES), (LC.IMAGE_OF, LC.FLAG_IMAGE_OF), (LC.TEXT, LC.FLAG_TEXT)))
    place = np.concatenate([LC.PLACE, np.zeros(len(LC.FLAG_BOXES), np.int32)])
    n = len(b)
    boxes, image_of, text, place_dev, font = dev(b), dev(io), dev(tx), dev(place), dev(R.LABEL_FONT.copy())
    guard = lambda size: torch.full((size + 16,), -7, dtype=torch.int32, device=DEV)
    plan, flags = guard(n * P._LABEL_WORDS), guard(n)
    vp, s = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.mcg_draw_labels(s, vp(table_dev.data_ptr()), len(views), 40, 48, vp(boxes.data_ptr()), vp(image_of.data_ptr()), vp(text.data_ptr()),
                                vp(place_dev.data_ptr()), n, vp(font.data_ptr()), 1, 6, 1, (C.c_ubyte * 3)(11, 22, 33), None, (C.c_ubyte * 3)(1, 2, 3),
                                vp(plan[8:].data_ptr()), vp(flags[8:].data_ptr())), 'mcg_draw_labels')
    torch.cuda.synchronize()
    want, want_flags = R.draw_labels_host(D.BGR_FRAMES, b, io, tx, color=(11, 22, 33), background=(1, 2, 3), scale=1, place=place)
    buffers_equal('bgr', bufs, want, 255)
    for got, size in ((plan, n * P._LABEL_WORDS), (flags, n)):
        got = got.cpu().numpy()
        assert (got[:8] == -7).all() and (got[8 + size:] == -7).all()                 # the guard words stand
    assert flags[8:8 + n].tolist() == want_flags.tolist() == LC.FLAGS + LC.FLAG_FLAGS
    d = plan[8:8 + n * P._LABEL_WORDS].cpu().numpy().view(P._LABEL).reshape(n)
    p = R.label_plan(b, io, tx, D.SHAPES, place, scale=1, advance=6, pad=1)
    for f in ('x', 'y', 'x0', 'y0', 'x1', 'y1', 'image', 'flag', 'len'):
        assert np.array_equal(d[f], p[f]), f
    ok = p['flag'] == 0
    assert (d['color'][ok] == 11 | 22 << 8 | 33 << 16).all() and not d['color'][~ok].any() and not d['text'][~ok].any()
    assert np.array_equal(d['text'][ok], tx[ok])
    # an image larger than (max_h, max_w) is flagged, not drawn
    keep = views[3].clone()
    L.check(lib.mcg_draw_labels(s, vp(table_dev.data_ptr()), len(views), 18, 22, vp(boxes.data_ptr()), vp(image_of.data_ptr()), vp(text.data_ptr()), None, n,
                                vp(font.data_ptr()), 1, 6, 1, (C.c_ubyte * 3)(0, 0, 0), None, None, vp(plan[8:].data_ptr()), vp(flags[8:].data_ptr())), 'mcg_draw_labels')
    torch.cuda.synchronize()
    assert all(f == 2 for f, k in zip(flags[8:8 + n].tolist(), io) if k == 3) and torch.equal(views[3], keep)
    # mcg_format_labels between guard bytes
    ids, values = dev(np.array([2147483647, 5, 0], np.int32)), dev(np.array([2147483647, 30, 9], np.int32))
    out = torch.full((16 + 3 * 24 + 16,), 200, dtype=torch.uint8, device=DEV)
    L.check(lib.mcg_format_labels(s, vp(ids.data_ptr()), vp(values.data_ptr()), 3, 1, 1, vp(out[16:].data_ptr())), 'mcg_format_labels')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:16] == 200).all() and (got[16 + 72:] == 200).all()                  # the 25-character text is cut at its row's end
    assert np.array_equal(got[16:16 + 72].reshape(3, 24), R.format_labels_host([2147483647, 5, 0], [2147483647, 30, 9], (1, 1)))
    assert bytes(got[16:40]) == b'#2147483647 2147483647.0'                           # 2147483647 frames at 1 / 1: q % 10 == 0, and the 's' is the byte cut


def test_an_odd_sized_row_of_a_device_nv12_table_is_flagged_and_not_written():
    lib = L.load()
    views, bufs = device_frames('nv12', 255)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    table = np.zeros(2, dtype=P._NV12_IMAGE)
    (y, uv) = views[1]
    table[0] = (y.data_ptr(), uv.data_ptr(), 18, 21, y.stride(0), uv.stride(0))
    table[1] = (y.data_ptr(), uv.data_ptr(), 17, 22, y.stride(0), uv.stride(0))
    table_dev = dev(table.view(np.uint8).reshape(-1).copy())
    boxes, text, font = dev(np.array([(2, 12, 9, 15)] * 2, np.float32)), dev(R.encode_labels(['ab', 'cd'])), dev(R.LABEL_FONT.copy())
    image_of = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    plan, flags = torch.zeros(2, P._LABEL_WORDS, dtype=torch.int32, device=DEV), torch.full((2,), -1, dtype=torch.int32, device=DEV)
    vp = C.c_void_p
    L.check(lib.mcg_draw_labels_nv12(vp(torch.cuda.current_stream().cuda_stream), vp(table_dev.data_ptr()), 2, 18, 22, vp(boxes.data_ptr()), vp(image_of.data_ptr()),
                                     vp(text.data_ptr()), None, 2, vp(font.data_ptr()), 1, 6, 1, (C.c_ubyte * 3)(100, 110, 120), None, (C.c_ubyte * 3)(16, 128, 128),
                                     vp(plan.data_ptr()), vp(flags.data_ptr())), 'mcg_draw_labels_nv12')
    torch.cuda.synchronize()
    assert flags.tolist() == [2, 2] and all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
