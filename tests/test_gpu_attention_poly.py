"""mcg_gaze_targets_poly on the device against attention.gaze_targets_host, all six tables bit for bit (include/mcgaze_hip.h, "gaze targets,
polygonal regions"): every case of tests/attention_poly_cases.py, the tile edges of the kernel (256 regions and 256 rows a tile), polygons
of 3, 4, 31 and 32 vertices, a vertex table that ends with the last polygon, offsets of garbage, rectangles only against mcg_gaze_targets
itself, strided gaze tables, graph capture, the guard words around the outputs and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import attention as AT
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import attention_cases as AC
from tests import attention_poly_cases as PC
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = PC.all_cases()
RECT = PC.rectangle_cases()
ROWS = ('boxes', 'gaze', 'image_of', 'region_image')


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(64))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def on_device(pipe, a, tables=True):
    """gaze_targets over the arguments of gaze_targets_host: every table a device tensor, or as they are (through the staging ring)."""
    a = dict(a)
    if tables:
        a = {k: dev(v) if k in ROWS else v for k, v in a.items()}
        a['regions'] = AT.PolyRegions(dev(a['regions'].xy), dev(a['regions'].start))
    got = pipe.gaze_targets(a.pop('boxes'), a.pop('gaze'), a.pop('image_of'), device=DEV, **a)
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_every_cpu_case(pipe, case):
    want = AT.gaze_targets_host(**PC.args(case))
    AC.same_tables(on_device(pipe, PC.tables(case)), want, case['name'] + ' (device tables)')
    AC.same_tables(on_device(pipe, PC.args(case), tables=False), want, case['name'] + ' (host tables, as the case gives them)')


@pytest.mark.parametrize('n,pictures,m,shuffle,garbage', [(255, 2, 255, True, 0), (256, 2, 256, True, 0), (257, 2, 257, True, 0), (600, 7, 16, True, 0),
                                                         (600, 7, 16, False, 0), (300, 40, 257, False, 6), (300, 3, 0, True, 0), (300, 3, 1, False, 0)])
def test_tile_edges_and_the_skip_branch(pipe, n, pictures, m, shuffle, garbage):
    """256 regions and 256 rows a tile: one short of a tile, a full tile, one over; 600 rows in 7 pictures shuffled (no tile is skipped) and in
    ascending order (a workgroup skips the tiles of the other pictures); two region tiles keyed by camera with garbage among the offsets; 0
    and 1 regions.  The vertex table ends exactly with the last polygon (region_polygons makes it so)."""
    case = PC.random_case(200 + n + m, n, pictures, m, period=4 if garbage else 0, shuffle=shuffle, garbage=garbage)
    a = PC.tables(case)
    assert garbage or int(a['regions'].start[-1]) == len(a['regions'].xy)
    want = AT.gaze_targets_host(**a)
    assert len(set(want[0].tolist())) >= 3
    AC.same_tables(on_device(pipe, a), want, case['name'])


def test_polygons_of_3_4_31_and_32_vertices_and_offsets_of_garbage(pipe):
    case = PC.random_case(77, 300, 2, 24, counts=(3, 4, 31, 32), bad=0.0)
    a = PC.tables(case)
    xy, start = a['regions']
    assert sorted(set(np.diff(start).tolist())) == [3, 4, 31, 32] and start[-1] == len(xy)
    want = AT.gaze_targets_host(**a)
    assert {3, 4, 31, 32} <= set(np.diff(start)[want[1][want[0] == AT.KIND_REGION]].tolist())
    AC.same_tables(on_device(pipe, a), want, 'V exactly at the last polygon\'s end')
    rng = np.random.default_rng(5)
    words = rng.integers(-2 ** 31, 2 ** 31, len(start)).astype(np.int32)         # every offset a garbage word: nothing is usable, nothing outside xy is read
    words[::4] = rng.integers(-40, len(xy) + 40, len(words[::4]))
    b = dict(a, regions=AT.PolyRegions(xy, words))
    AC.same_tables(on_device(pipe, b), AT.gaze_targets_host(**b), 'garbage offsets')
    short = dict(a, regions=AT.PolyRegions(xy[:-1], start))       # the last polygon one vertex beyond the table: not usable
    want = AT.gaze_targets_host(**short)
    assert not (want[1][want[0] == AT.KIND_REGION] == len(start) - 2).any()
    AC.same_tables(on_device(pipe, short), want, 'V one short of the last polygon\'s end')


@pytest.mark.parametrize('name,old,new', RECT, ids=[r[0] for r in RECT])
def test_rectangles_only_give_the_bits_of_mcg_gaze_targets(pipe, name, old, new):
    AC.same_tables(on_device(pipe, new), on_device(pipe, old, tables=False), name)


def test_rows_and_regions_are_each_decided_as_a_group(pipe):
    """Rows on the device beside vertex tables on the host, and the reverse: the host group goes up through one stage; one table of a group
    on the device (here ``start`` alone) moves the rest of that group with torch."""
    a = PC.tables(next(c for c in PC.hand_cases() if c['name'] == 'regions of every picture, of one picture, of a camera'))
    want = AT.gaze_targets_host(**a)
    xy, start = a['regions']
    rows = {k: dev(a[k]) for k in ('boxes', 'gaze', 'image_of')}
    for what, b, stages in (('rows on the device', dict(a, **rows), 1),
                            ('regions on the device', dict(a, regions=AT.PolyRegions(dev(xy), dev(start)), region_image=dev(a['region_image'])), 1),
                            ('boxes and start on the device', dict(a, boxes=rows['boxes'], regions=AT.PolyRegions(xy, dev(start))), 0)):
        before = pipe._ring.i
        got = pipe.gaze_targets(b.pop('boxes'), b.pop('gaze'), b.pop('image_of'), device=DEV, **b)
        assert pipe._ring.i == (before + stages) % pipe.STAGES
        torch.cuda.synchronize()
        AC.same_tables(tuple(g.cpu().numpy() for g in got), want, what)


def test_strided_gaze_tables(pipe):
    case = PC.random_case(11, 70, 2, 9)
    a = PC.tables(case)
    want = AT.gaze_targets_host(**a)
    wide = np.full((70, 5), 7.0, np.float32)                      # the fused [n, 3] inside a wider tensor
    wide[:, :3] = a['gaze']
    tail = np.full((70, 8), 7.0, np.float32)
    tail[:, 5:] = a['gaze']
    regions = AT.PolyRegions(dev(a['regions'].xy), dev(a['regions'].start))
    for what, g in (('[n, 5] rows', dev(wide)), ('a [:, :3] view of [n, 5]', dev(wide)[:, :3]), ('a [:, 5:] view of [n, 8]', dev(tail)[:, 5:])):
        got = pipe.gaze_targets(dev(a['boxes']), g, dev(a['image_of']), regions=regions, region_image=dev(a['region_image']), device=DEV)
        AC.same_tables(tuple(x.cpu().numpy() for x in got), want, what)


def test_device_tables_with_no_host_touch_captured_and_replayed(pipe, monkeypatch):
    first, second, third = (PC.tables(PC.random_case(s, 300, 3, 20, period=2)) for s in (21, 22, 23))
    V, M = (max(len(c['regions'][k]) for c in (first, second, third)) for k in (0, 1))

    def padded(c):                                                # one shape for the three: vertices nobody owns, regions without vertices
        xy, start = c['regions']
        return dict(boxes=c['boxes'], gaze=c['gaze'], image_of=c['image_of'], xy=np.concatenate([xy, np.zeros((V - len(xy), 2), np.float32)]),
                    start=np.concatenate([start, np.full(M - len(start), start[-1], np.int32)]),
                    region_image=np.concatenate([c['region_image'], np.full(M - len(start), -1, np.int32)]))

    bufs = {k: dev(v) for k, v in padded(first).items()}
    call = lambda: pipe.gaze_targets(bufs['boxes'], bufs['gaze'], bufs['image_of'], regions=AT.PolyRegions(bufs['xy'], bufs['start']),
                                     region_image=bufs['region_image'], region_period=2, device=DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()                                                    # warm-up outside the capture
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('the call touched the host')

    for owner, name in ((torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'), (torch.cuda, 'synchronize'),
                        (torch.cuda.Stream, 'synchronize')):
        monkeypatch.setattr(owner, name, refuse)
    with torch.cuda.stream(side):
        call()
    monkeypatch.undo()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for case in (second, third):
        p = padded(case)
        for k in bufs:
            bufs[k].copy_(dev(p[k]))
        graph.replay()
        torch.cuda.synchronize()
        want = AT.gaze_targets_host(**dict(case, regions=AT.PolyRegions(p['xy'], p['start']), region_image=p['region_image']))
        AC.same_tables(tuple(x.cpu().numpy() for x in out), want, 'replay')
        AC.same_tables(want, AT.gaze_targets_host(**case), 'the padding adds nothing')


def test_guard_words_and_rows_beyond_n_stay_untouched():
    """The entry itself, on outputs that lie inside larger guarded arrays: n of the 300 rows are written, nothing before, behind or beyond."""
    lib = L.load()
    a = PC.tables(PC.random_case(31, 300, 3, 20))
    xy, start = a['regions']
    n, rows, guard, mark = 270, 300, 64, 0x5a5a5a5a
    want = AT.gaze_targets_host(a['boxes'][:n], a['gaze'][:n], a['image_of'][:n], regions=a['regions'], region_image=a['region_image'])
    words = (1, 1, 1, 2, 1, 1)                                    # 32-bit words per row: kind, target, t, hit, mutual, flags
    outs = [torch.full((guard + rows * w + guard,), mark, dtype=torch.int32, device=DEV) for w in words]
    b, g, io, v, s, ri = (dev(t) for t in (a['boxes'], a['gaze'], a['image_of'], xy, start, a['region_image']))
    vp = C.c_void_p
    L.check(lib.mcg_gaze_targets_poly(vp(torch.cuda.current_stream().cuda_stream), vp(b.data_ptr()), vp(g.data_ptr()), 3, vp(io.data_ptr()), n,
                                      vp(v.data_ptr()), len(xy), vp(s.data_ptr()), vp(ri.data_ptr()), len(start) - 1, 0, 0.25, AT._target_params()[1],
                                      *(vp(o.data_ptr() + 4 * guard) for o in outs)), 'mcg_gaze_targets_poly')
    torch.cuda.synchronize()
    got = []
    for o, w, ref in zip(outs, words, want):
        o = o.cpu().numpy()
        assert (o[:guard] == mark).all() and (o[guard + n * w:] == mark).all()
        got.append(o[guard:guard + n * w].view(ref.dtype).reshape(ref.shape))
    AC.same_tables(tuple(got), want, 'the first n rows')


def test_argument_errors_raise_before_any_launch(pipe):
    a = PC.tables(PC.hand_cases()[0])
    b, g, io = dev(a['boxes']), dev(a['gaze']), dev(a['image_of'])
    xy, start = dev(a['regions'].xy), dev(a['regions'].start)
    for bad in (dict(regions=AT.PolyRegions(xy[:, :1], start)), dict(regions=AT.PolyRegions(xy, start[:0])), dict(regions=AT.PolyRegions(xy, start.view(1, -1))),
                dict(regions=AT.PolyRegions(xy, start), region_image=dev(np.zeros(3, np.int32))), dict(regions=AT.PolyRegions(xy, start), expand=-1),
                dict(regions=AT.PolyRegions(dev(np.zeros((AT.MAX_VERTICES + 1, 2), np.float32)), start)),
                dict(regions=AT.PolyRegions(xy, dev(np.zeros(AT.MAX_REGIONS + 2, np.int32)))), dict(regions=[PC.TRI[:2]]), dict(regions=[PC.TRI, [1, 2, 3]])):
        with pytest.raises(ValueError):
            pipe.gaze_targets(b, g, io, device=DEV, **bad)
    with pytest.raises(TypeError):
        pipe.gaze_targets(b, g, io, device=DEV, regions=[PC.TRI, 5])
    lib, vp, p = L.load(), C.c_void_p, C.c_void_p(256)
    for V, m in ((AT.MAX_VERTICES + 1, 1), (4, AT.MAX_REGIONS + 1), (-1, 1)):
        assert lib.mcg_gaze_targets_poly(None, p, p, 3, p, 1, p, V, p, p, m, 0, 0.25, 0.5, p, p, p, p, p, p) != L.MCG_OK
    empty = pipe.gaze_targets(b[:0], g[:0], io[:0], regions=AT.PolyRegions(xy, start), device=DEV)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0,), (0, 2), (0,), (0,)]
