"""-m gpu: the attention overlay drawn on the device -- DevicePipeline.draw_attention (mcg_draw_attention, mcg_draw_attention_nv12) and the entries
through ctypes -- against arrows.draw_attention_host (itself checked in tests/test_overlay_cpu.py), bit for bit: frames with their own
pitches and junk in the padding, the ballot slice edge (63 / 64 / 65 rows and regions), frames one cell past a tile, polygons of 3, 4, 31 and
32 vertices, a vertex table that ends at and one short of the last polygon, one region on pictures of different size, strokes outside their
frame, strided gaze, every layer switched off, the anchor against draw_arrows, the unusable regions and flag rows, device tables with no host
touch, graph capture.  The odd inputs are table contents the entries document; nothing here provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import arrows as AR
from mcgaze_amd import attention as AT
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import draw_cases as D
from tests import overlay_cases as O
from tests.test_gpu_draw import as_arrays, device_frames, expected_buffers
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FORMATS = [('bgr', 'bt601'), ('nv12', 'bt601'), ('nv12', 'bt709')]
IDS = ['bgr', 'nv12-bt601', 'nv12-bt709']
TABLES = ('boxes', 'gaze', 'image_of', 'kind', 'target', 'hit', 'mutual', 'region_image')


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def on_device(a):
    """The arguments of draw_attention_host with every table a device tensor (regions as PolyRegions of device tensors)."""
    a = dict(a)
    regions = a.get('regions')
    if regions is not None:
        xy, start = regions if isinstance(regions, AT.PolyRegions) else AT.region_polygons(regions)
        a['regions'] = AT.PolyRegions(dev(xy), dev(start))
    return {k: dev(np.asarray(v)) if k in TABLES and v is not None else v for k, v in a.items()}


def check(pipe, fmt, matrix, frames, args, what, device_tables=True):
    """The call on host frames (device or host tables) against the twin: frames and the three tables."""
    want = AR.draw_attention_host(frames, pixel_format=fmt, matrix=matrix, **args)
    got = pipe.draw_attention(frames, pixel_format=fmt, matrix=matrix, device=DEV, **(on_device(args) if device_tables else args))
    torch.cuda.synchronize()
    O.same(fmt, as_arrays(fmt, got[0]), want[0], what)
    for g, w, name in zip(got[1:], want[1:], ('flags', 'region_flags', 'region_active')):
        assert g.dtype == torch.int32 and tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), (what, name)
    return want


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_the_scene_on_frames_with_their_own_pitches_and_junk_in_the_padding(pipe, fmt, matrix):
    for kw in (dict(), dict(min_thickness=1, line_thickness=1, region_thickness=1), dict(min_thickness=3, line_thickness=4, region_thickness=5, region_period=2)):
        args = O.scene(**kw)
        want = check(pipe, fmt, matrix, O.frames(fmt), args, ('host frames', kw), device_tables=False)
        for junk, tables in ((255, on_device(args)), (0, args)):
            views, bufs = device_frames(fmt, junk)
            got = pipe.draw_attention(views, pixel_format=fmt, matrix=matrix, device=DEV, **tables)
            torch.cuda.synchronize()
            assert all(g is v for g, v in zip(got[0], views)) and got[1].tolist() == want[1].tolist()
            for k, (bs, es) in enumerate(zip(bufs, expected_buffers(fmt, want[0], junk))):
                for b, e in zip(bs, es):
                    assert np.array_equal(b.cpu().numpy(), e), (kw, junk, k)
    views, bufs = device_frames(fmt, 7)                           # copy=True leaves the source untouched
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    got = pipe.draw_attention(views, pixel_format=fmt, matrix=matrix, device=DEV, copy=True, **on_device(O.scene()))
    torch.cuda.synchronize()
    O.same(fmt, as_arrays(fmt, got[0]), AR.draw_attention_host(O.frames(fmt), pixel_format=fmt, matrix=matrix, **O.scene())[0], 'copy')
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))


@pytest.mark.parametrize('host_table,stages', [('gaze', 1), ('hit', 0), ('start', 0), ('region_image', 0)])
@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_one_table_of_each_group_on_the_host_and_the_rest_on_the_device(fmt, matrix, host_table, stages):
    """Every operand must be read where it really is.  A host row table beside device ones goes up through the staging ring (one stage); a
    host table among gaze_targets' results or among the region tables, which are each decided as a group, is moved with torch (no stage:
    the frame table of device frames drawn in place does not go through the ring)."""
    pipe = P.DevicePipeline(chain(32))
    args = O.scene()
    want = AR.draw_attention_host(O.frames(fmt), pixel_format=fmt, matrix=matrix, **args)
    tables = on_device(args)
    if host_table == 'start':
        xy, start = AT.region_polygons(args['regions'])
        tables['regions'] = AT.PolyRegions(tables['regions'].xy, start)
    else:
        tables[host_table] = np.asarray(args[host_table])
    views, bufs = device_frames(fmt, 255)
    before = pipe._ring.i
    got = pipe.draw_attention(views, pixel_format=fmt, matrix=matrix, device=DEV, **tables)
    assert pipe._ring.i == (before + stages) % pipe.STAGES
    torch.cuda.synchronize()
    assert all(g is v for g, v in zip(got[0], views))
    for g, w, name in zip(got[1:], want[1:], ('flags', 'region_flags', 'region_active')):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w), (host_table, name)
    for k, (bs, es) in enumerate(zip(bufs, expected_buffers(fmt, want[0], 255))):
        for b, e in zip(bs, es):
            assert np.array_equal(b.cpu().numpy(), e), (host_table, k)


@pytest.mark.parametrize('n,m', [(63, 65), (64, 64), (65, 63), (0, 64), (64, 0), (1, 1)])
@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_the_ballot_slice_edge(pipe, fmt, matrix, n, m):
    """m + 2 n records in slices of 64: layers that begin and end one short of, at and one past a slice edge, on one 40 x 48 frame."""
    case = O.random_case(100 + n + 3 * m, n, m)
    check(pipe, fmt, matrix, O.blank(fmt, [(40, 48)]), case, (n, m))


@pytest.mark.parametrize('fmt,matrix,shape', [('bgr', 'bt601', (9, 33)), ('nv12', 'bt601', (18, 66)), ('nv12', 'bt709', (18, 66)), ('bgr', 'bt601', (8, 32))],
                         ids=['bgr-9x33', 'nv12-bt601-18x66', 'nv12-bt709-18x66', 'bgr-8x32'])
def test_frames_one_cell_past_a_tile(pipe, fmt, matrix, shape):
    case = O.random_case(17, 20, 6, [shape], counts=(2, 3, 4))
    check(pipe, fmt, matrix, O.blank(fmt, [shape]), case, shape)


def test_polygons_of_3_4_31_and_32_vertices_and_the_end_of_the_vertex_table(pipe):
    case = O.random_case(77, 30, 12, counts=(3, 4, 31, 32))
    xy, start = case['regions']
    assert sorted(set(np.diff(start).tolist())) == [3, 4, 31, 32] and start[-1] == len(xy) and np.diff(start)[-1] == 32
    frames = O.blank('bgr', [(40, 48)])
    want = check(pipe, 'bgr', 'bt601', frames, case, 'V at the last polygon\'s end')
    assert want[2].tolist() == [0] * 12
    short = dict(case, regions=AT.PolyRegions(xy[:-1], start))    # the last polygon one vertex beyond the table: not usable
    want = check(pipe, 'bgr', 'bt601', frames, short, 'V one short')
    assert want[2].tolist() == [0] * 11 + [2]
    words = dict(case, regions=AT.PolyRegions(xy, O.garbage_offsets(xy, 12)))
    check(pipe, 'nv12', 'bt709', O.blank('nv12', [(40, 48)]), words, 'garbage offsets')


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_one_region_on_pictures_of_different_size_and_strokes_outside_their_frame(pipe, fmt, matrix):
    shapes = D.SHAPES
    args = dict(boxes=[[100, 100, 120, 120], [30, 4, 50, 24]], gaze=[[0.5, 0.5, 0], [0, 0, 0]], image_of=[3, 0], kind=[2, 1], target=[1, 0],
                hit=[[130, 140], [60, 14]], mutual=[0, 0], regions=[[1, 1, 30, 30], [200, 200, 260, 240], [[-40, -40], [-20, -45], [-30, -10]]],
                region_image=[-1, -1, 3], palette=O.PALETTE)
    args = {k: np.asarray(v, np.float32 if k in ('boxes', 'gaze', 'hit') else np.int32) if k in TABLES else v for k, v in args.items()}
    want = check(pipe, fmt, matrix, O.frames(fmt), args, 'regions past the small frames, rows outside')
    assert want[1].tolist() == [0, 0] and want[2].tolist() == [0, 0, 0] and want[3][3].tolist() == [0, 1, 0]
    assert not np.array_equal(O.luma(fmt, want[0][2]), O.luma(fmt, O.frames(fmt)[2]))     # the 2 x 2 frame gets its corner of region 0


def test_strided_gaze(pipe):
    case = O.random_case(11, 40, 5)
    frames = O.blank('bgr', [(40, 48)])
    want = AR.draw_attention_host(frames, **case)
    wide = np.full((40, 5), 7.0, np.float32)
    wide[:, :3] = case['gaze']
    tail = np.full((40, 8), 7.0, np.float32)
    tail[:, 5:] = case['gaze']
    a = on_device(case)
    for what, g in (('[n, 5] rows', dev(wide)), ('a [:, :3] view of [n, 5]', dev(wide)[:, :3]), ('a [:, 5:] view of [n, 8]', dev(tail)[:, 5:])):
        got = pipe.draw_attention(frames, device=DEV, **dict(a, gaze=g))
        O.same('bgr', as_arrays('bgr', got[0]), want[0], what)


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_thickness_zero_switches_each_layer_off(pipe, fmt, matrix):
    for off in ('min_thickness', 'line_thickness', 'region_thickness'):
        want = check(pipe, fmt, matrix, O.frames(fmt), O.scene(**{off: 0}), off)
        assert want[1].tolist() == [0] * len(D.ROWS) and want[2].tolist() == [0] * 5 and want[3].sum() == 4
    check(pipe, fmt, matrix, O.frames(fmt), O.scene(min_thickness=0, line_thickness=0, region_thickness=0), 'all off')


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_the_anchor_against_draw_arrows_on_the_device(pipe, fmt, matrix):
    n = len(D.ROWS) + len(D.FLAGS)
    b, g, io = (dev(np.concatenate([x, y])) for x, y in ((D.BOXES, D.FLAG_BOXES), (D.GAZE, D.FLAG_GAZE), (D.IMAGE_OF, D.FLAG_IMAGE_OF)))
    zero = torch.zeros(n, dtype=torch.int32, device=DEV)
    pal = np.array(AR.OVERLAY_PALETTE)
    pal[0] = (9, 200, 77)
    for t in (1, 5):
        a_views, a_bufs = device_frames(fmt, 255)
        b_views, b_bufs = device_frames(fmt, 255)
        _, want_flags = pipe.draw_arrows(a_views, b, g, io, color=(9, 200, 77), pixel_format=fmt, matrix=matrix, min_thickness=t, device=DEV)
        _, flags, region_flags, active = pipe.draw_attention(b_views, b, g, io, zero, zero - 1, torch.zeros(n, 2, device=DEV), zero, palette=pal, pixel_format=fmt,
                                                             matrix=matrix, min_thickness=t, device=DEV)
        torch.cuda.synchronize()
        assert torch.equal(flags, want_flags) and flags.tolist() == [0] * len(D.ROWS) + D.FLAGS and tuple(active.shape) == (4, 0)
        assert all(torch.equal(x, y) for xs, ys in zip(a_bufs, b_bufs) for x, y in zip(xs, ys))


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_unusable_regions_and_flag_rows_from_device_tables_write_nothing(pipe, fmt, matrix):
    regions, region_image, names = O.unusable_regions()
    none = dict(boxes=np.zeros((0, 4), np.float32), gaze=np.zeros((0, 3), np.float32), image_of=np.zeros(0, np.int32), kind=np.zeros(0, np.int32),
                target=np.zeros(0, np.int32), hit=np.zeros((0, 2), np.float32), mutual=np.zeros(0, np.int32))
    want = check(pipe, fmt, matrix, O.frames(fmt)[3:], dict(none, regions=regions, region_image=region_image), 'unusable regions')
    assert want[2].tolist() == O.UNUSABLE_FLAGS
    xy, start = regions
    bad = [j for j, f in enumerate(O.UNUSABLE_FLAGS) if f]
    only_bad = AT.PolyRegions(xy, np.concatenate([start[bad], start[[bad[-1] + 1]]]))      # (regions 1 .. 8 are consecutive)
    views, bufs = device_frames(fmt, 255)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    got = pipe.draw_attention(views, device=DEV, pixel_format=fmt, matrix=matrix, **on_device(dict(none, regions=only_bad)))
    torch.cuda.synchronize()
    assert got[2].tolist() == [2] * len(bad) and all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    # the flag rows: a NaN / beyond-the-bound / infinite hit drops the line and keeps the arrow; flagged rows write nothing
    want = check(pipe, fmt, matrix, O.frames(fmt), O.flag_scene(), 'flag rows')
    assert want[1].tolist() == D.FLAGS
    with pytest.raises(ValueError):                               # host tables: refused before anything is launched
        pipe.draw_attention(O.frames(fmt), device=DEV, pixel_format=fmt, matrix=matrix, **O.flag_scene())


def test_device_tables_with_no_host_touch_captured_and_replayed_twice(pipe, monkeypatch):
    fmt, matrix = 'nv12', 'bt709'
    first, second, third = (O.random_case(s, 30, 8, D.SHAPES, period=2) for s in (21, 22, 23))
    V = max(len(c['regions'].xy) for c in (first, second, third))

    def padded(c):                                                # one shape for the three: vertices nobody owns behind the last polygon
        xy, start = c['regions']
        return dict({k: c[k] for k in TABLES}, xy=np.concatenate([xy, np.zeros((V - len(xy), 2), np.float32)]), start=start)

    views, bufs = device_frames(fmt, 255)
    pristine = [tuple(b.clone() for b in bs) for bs in bufs]
    t = {k: dev(v) for k, v in padded(first).items()}
    call = lambda: pipe.draw_attention(views, *(t[k] for k in TABLES[:7]), regions=AT.PolyRegions(t['xy'], t['start']), region_image=t['region_image'],
                                       region_period=2, palette=O.PALETTE, pixel_format=fmt, matrix=matrix, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                    # warm-up outside the capture: uploads the frame table once
    torch.cuda.synchronize()
    stage_i = pipe._ring.i

    def refuse(*a, **k):
        raise AssertionError('the call touched the host')

    for owner, name in ((torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'), (torch.cuda, 'synchronize'),
                        (torch.cuda.Stream, 'synchronize')):
        monkeypatch.setattr(owner, name, refuse)
    with torch.cuda.stream(side):
        call()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert pipe._ring.i == stage_i                                # no staging buffer was taken
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for bs, cs in zip(bufs, pristine):
            for b, c in zip(bs, cs):
                b.copy_(c)
        out = call()
    for case in (second, third):
        for k, v in padded(case).items():
            t[k].copy_(dev(v))
        graph.replay()
        torch.cuda.synchronize()
        want = AR.draw_attention_host(O.frames(fmt), pixel_format=fmt, matrix=matrix, **case)
        for g, w in zip(out[1:], want[1:]):
            assert np.array_equal(g.cpu().numpy(), w)
        for k, (bs, es) in enumerate(zip(bufs, expected_buffers(fmt, want[0], 255))):
            for b, e in zip(bs, es):
                assert np.array_equal(b.cpu().numpy(), e), k


def test_the_entries_through_ctypes_guard_words_and_argument_checks():
    lib = L.load()
    views, bufs = device_frames('bgr', 255)
    table = np.zeros(len(views), dtype=P._IMAGE)
    for k, v in enumerate(views):
        table[k] = (v.data_ptr(), v.shape[0], v.shape[1], v.stride(0))
    table_dev = dev(table.view(np.uint8).reshape(-1).copy())
    a = O.scene()
    xy, start = AT.region_polygons(a['regions'])
    n, m, V, images = len(D.ROWS), len(start) - 1, len(xy), len(views)
    t = {k: dev(np.asarray(a[k])) for k in TABLES}
    xy_d, start_d = dev(xy), dev(start)
    words = 24 * (m + 2 * n) + 64 * m
    guard = lambda size: torch.full((size + 16,), -7, dtype=torch.int32, device=DEV)
    work, flags, region_flags, active = guard(words), guard(n), guard(m), guard(images * m)
    vp = C.c_void_p
    s = vp(torch.cuda.current_stream().cuda_stream)
    pal = (C.c_ubyte * 21)(*[int(v) for v in O.PALETTE.reshape(-1)])

    def call(entry=lib.mcg_draw_attention, images_=table_dev.data_ptr(), num_images=images, max_h=40, max_w=48, stride=3, n_=n, m_=m, V_=V, period=0, palette=pal,
             length=1.0, min_t=5, line_t=2, region_t=2, work_=work.data_ptr() + 32, bytes_=4 * words, flags_=flags.data_ptr() + 32, xy_=xy_d.data_ptr()):
        return entry(s, vp(images_), num_images, max_h, max_w, vp(t['boxes'].data_ptr()), vp(t['gaze'].data_ptr()), stride, vp(t['image_of'].data_ptr()), n_,
                     vp(t['kind'].data_ptr()), vp(t['target'].data_ptr()), vp(t['hit'].data_ptr()), vp(t['mutual'].data_ptr()), vp(xy_), V_, vp(start_d.data_ptr()),
                     vp(t['region_image'].data_ptr()), m_, period, palette, length, min_t, 0.01, 0.1, line_t, region_t, vp(work_), bytes_, vp(flags_),
                     vp(region_flags.data_ptr() + 32), vp(active.data_ptr() + 32))

    L.check(call(), 'mcg_draw_attention')
    torch.cuda.synchronize()
    want = AR.draw_attention_host(O.frames('bgr'), **a)
    for k, (bs, es) in enumerate(zip(bufs, expected_buffers('bgr', want[0], 255))):
        assert np.array_equal(bs[0].cpu().numpy(), es[0]), k
    for buf, w in ((flags, want[1]), (region_flags, want[2]), (active, want[3].reshape(-1))):
        got = buf.cpu().numpy()
        assert np.array_equal(got[8:8 + w.size], w) and (got[:8] == -7).all() and (got[8 + w.size:] == -7).all()      # the guard words stand
    got = work.cpu().numpy()
    assert (got[:8] == -7).all() and (got[8 + words:] == -7).all()
    plan = got[8:8 + 24 * (m + 2 * n)].reshape(-1, 24)
    seg, thick, _ = AR.arrow_segments(D.BOXES, D.GAZE)
    assert np.array_equal(plan[m + n:, :12].reshape(n, 3, 2, 2), seg) and np.array_equal(plan[m + n:, 12], thick)       # the arrows' records are draw_arrows' plan
    assert plan[:m, 19].tolist() == [0] * m and plan[m:m + n, 19].tolist() == [1] * n and plan[m + n:, 19].tolist() == [2] * n and plan[:m, 20].tolist() == [4, 4, 6, 3, 4]
    err = lambda: lib.mcg_last_error()
    assert call(n_=65536) != L.MCG_OK and b'65535' in err()
    assert call(m_=4097) != L.MCG_OK and b'4096' in err()
    assert call(V_=65537) != L.MCG_OK and b'65536' in err()
    assert call(num_images=65535, m_=17) != L.MCG_OK and b'num_images * m' in err()
    assert call(max_h=8193) != L.MCG_OK and b'8192' in err()
    assert call(num_images=0) != L.MCG_OK and b'bad sizes' in err()
    assert call(stride=1) != L.MCG_OK and b'bad sizes' in err()
    assert call(period=-1) != L.MCG_OK and b'bad sizes' in err()
    for kw in (dict(min_t=256), dict(line_t=-1), dict(region_t=256)):
        assert call(**kw) != L.MCG_OK and b'0 .. 255' in err()
    assert call(length=float('nan')) != L.MCG_OK and b'finite' in err()
    assert call(images_=None) != L.MCG_OK and b'null pointer' in err()
    assert call(palette=None) != L.MCG_OK and b'null pointer' in err()
    assert call(flags_=None) != L.MCG_OK and b'null row table' in err()
    assert call(xy_=None) != L.MCG_OK and b'null vertex table' in err()
    assert call(work_=None) != L.MCG_OK and b'workspace' in err()
    assert call(bytes_=4 * words - 4) != L.MCG_OK and b'workspace' in err()
    assert call(n_=0, m_=0, V_=0) == L.MCG_OK
    assert call(entry=lib.mcg_draw_attention_nv12, images_=None) != L.MCG_OK and b'mcg_draw_attention_nv12: null pointer' in err()
