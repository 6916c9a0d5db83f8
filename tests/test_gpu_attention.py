"""mcg_gaze_targets on the device against attention.gaze_targets_host, all six tables bit for bit (include/mcgaze_hip.h, "gaze targets"):
every case of tests/attention_cases.py, the tile edges of the kernel (256 candidates a tile, the tile skipped when its pictures are not
asked about), strided gaze tables, graph capture and the guard words around the outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import attention as AT
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import attention_cases as AC
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = AC.all_cases()
TABLES = ('boxes', 'gaze', 'image_of', 'regions', 'region_image')


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(64))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def on_device(pipe, a, tables=True):
    """gaze_targets over the arguments of gaze_targets_host: as device tensors, or as they are (numpy, through the staging ring)."""
    a = {k: dev(v) if tables and k in TABLES else v for k, v in a.items()}
    got = pipe.gaze_targets(a.pop('boxes'), a.pop('gaze'), a.pop('image_of'), device=DEV, **a)
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_every_cpu_case(pipe, case):
    want = AT.gaze_targets_host(**AC.args(case))
    AC.same_tables(on_device(pipe, AC.args(case)), want, case['name'] + ' (device tables)')
    AC.same_tables(on_device(pipe, AC.args(case), tables=False), want, case['name'] + ' (host tables)')


@pytest.mark.parametrize('n,pictures,m,shuffle', [(255, 2, 3, True), (256, 2, 3, True), (257, 2, 3, True), (600, 7, 16, True), (600, 7, 16, False),
                                                 (300, 3, 0, True), (300, 3, 1, False), (300, 40, 257, False)])
def test_tile_edges_and_the_skip_branch(pipe, n, pictures, m, shuffle):
    """256 rows a tile: one row short of a tile, a full tile, one row over; 600 rows in 7 pictures shuffled (every tile holds every picture:
    no tile is skipped) and in ascending order (a workgroup asks about 3 - 4 pictures and skips the tiles of the others); 0, 1 and 257
    regions (two region tiles, with region_period some keyed by camera)."""
    case = AC.random_case(100 + n + m, n, pictures, m, period=4 if m == 257 else 0, shuffle=shuffle)
    want = AT.gaze_targets_host(**AC.args(case))
    assert len(set(want[0].tolist())) >= 3                        # heads, regions or the camera, and nothing: the table is not trivial
    AC.same_tables(on_device(pipe, AC.args(case)), want, case['name'])


def test_rows_and_regions_are_each_decided_as_a_group(pipe):
    """Rows on the device beside regions on the host, and the reverse: the host group goes up through one stage, the device group is read
    where it is.  One table of a group on the device moves the rest of that group with torch, and no stage is taken."""
    a = AC.args(next(c for c in AC.hand_cases() if c['name'] == 'a region of every picture, of one picture, of a camera'))
    want = AT.gaze_targets_host(**a)
    rows, regions = ('boxes', 'gaze', 'image_of'), ('regions', 'region_image')
    for there, stages in ((rows, 1), (regions, 1), (('gaze', 'regions'), 0)):
        b = {k: dev(v) if k in there else v for k, v in a.items()}
        before = pipe._ring.i
        got = pipe.gaze_targets(b.pop('boxes'), b.pop('gaze'), b.pop('image_of'), device=DEV, **b)
        assert pipe._ring.i == (before + stages) % pipe.STAGES
        torch.cuda.synchronize()
        AC.same_tables(tuple(g.cpu().numpy() for g in got), want, f'{there} on the device')


def test_strided_gaze_tables(pipe):
    case = AC.random_case(11, 70, 2, 4)
    a = AC.args(case)
    want = AT.gaze_targets_host(**a)
    wide = np.full((70, 5), 7.0, np.float32)                      # det-like rows: the gaze in the first three of five columns
    wide[:, :3] = a['gaze']
    tail = np.full((70, 8), 7.0, np.float32)                      # ... or in the last three of eight: a view that starts inside a row
    tail[:, 5:] = a['gaze']
    for what, g in (('[n, 5] rows', dev(wide)), ('a [:, :3] view of [n, 5]', dev(wide)[:, :3]), ('a [:, 5:] view of [n, 8]', dev(tail)[:, 5:]),
                    ('a transposed table', dev(a['gaze'].T.copy()).T), ('float64', dev(a['gaze'].astype(np.float64)))):
        got = pipe.gaze_targets(dev(a['boxes']), g, dev(a['image_of']), regions=dev(a['regions']), region_image=dev(a['region_image']), device=DEV)
        AC.same_tables(tuple(x.cpu().numpy() for x in got), want, what)
    # image_of None: one picture; int64 tables are converted
    one = AT.gaze_targets_host(a['boxes'], a['gaze'])
    AC.same_tables(tuple(x.cpu().numpy() for x in pipe.gaze_targets(dev(a['boxes']), dev(a['gaze']), None, device=DEV)), one, 'image_of None')


def test_option_and_shape_checks_raise_before_any_launch(pipe):
    a = AC.args(AC.hand_cases()[0])
    b, g, io = dev(a['boxes']), dev(a['gaze']), dev(a['image_of'])
    for bad in (dict(expand=-1), dict(camera_angle=100), dict(region_period=-2), dict(regions=dev(np.zeros((2, 3), np.float32))),
                dict(regions=dev(np.zeros((2, 4), np.float32)), region_image=dev(np.zeros(3, np.int32))), dict(region_image=dev(np.zeros(1, np.int32)))):
        with pytest.raises(ValueError):
            pipe.gaze_targets(b, g, io, device=DEV, **bad)
    for rows in ((b, g[:, :2], io), (b[:, :3], g, io), (b, g, io[:1]), (b, g[:1], io)):
        with pytest.raises(ValueError):
            pipe.gaze_targets(*rows, device=DEV)
    with pytest.raises(L.McgError):
        pipe.gaze_targets(a['boxes'], a['gaze'], a['image_of'], device='cpu')
    empty = pipe.gaze_targets(b[:0], g[:0], io[:0], device=DEV)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0,), (0, 2), (0,), (0,)]


def test_the_call_is_capturable(pipe):
    """Device tables, captured once, replayed with new contents in the same buffers."""
    first, second, third = (AC.random_case(s, 300, 3, 9, period=2) for s in (21, 22, 23))
    bufs = {k: dev(first[k]) for k in TABLES}
    call = lambda: pipe.gaze_targets(bufs['boxes'], bufs['gaze'], bufs['image_of'], regions=bufs['regions'], region_image=bufs['region_image'],
                                     region_period=2, device=DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()                                                    # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for case in (second, third):
        for k in TABLES:
            bufs[k].copy_(dev(case[k]))
        graph.replay()
        torch.cuda.synchronize()
        AC.same_tables(tuple(x.cpu().numpy() for x in out), AT.gaze_targets_host(**AC.args(case)), case['name'] + ' (replay)')


def test_guard_words_and_rows_beyond_n_stay_untouched():
    """The entry itself, on outputs that lie inside larger guarded arrays: n of the 300 rows are written, nothing before, behind or beyond."""
    lib = L.load()
    case = AC.random_case(31, 300, 3, 5)
    a = AC.args(case)
    n, rows, guard, mark = 270, 300, 64, 0x5a5a5a5a
    want = AT.gaze_targets_host(a['boxes'][:n], a['gaze'][:n], a['image_of'][:n], regions=a['regions'], region_image=a['region_image'])
    words = (1, 1, 1, 2, 1, 1)                                    # 32-bit words per row: kind, target, t, hit, mutual, flags
    outs = [torch.full((guard + rows * w + guard,), mark, dtype=torch.int32, device=DEV) for w in words]
    b, g, io, r, ri = (dev(a[k]) for k in TABLES)
    vp = C.c_void_p
    L.check(lib.mcg_gaze_targets(vp(torch.cuda.current_stream().cuda_stream), vp(b.data_ptr()), vp(g.data_ptr()), 3, vp(io.data_ptr()), n, vp(r.data_ptr()),
                                 vp(ri.data_ptr()), len(a['regions']), 0, 0.25, AT._target_params()[1], *(vp(o.data_ptr() + 4 * guard) for o in outs)),
            'mcg_gaze_targets')
    torch.cuda.synchronize()
    got = []
    for o, w, ref in zip(outs, words, want):
        o = o.cpu().numpy()
        assert (o[:guard] == mark).all() and (o[guard + n * w:] == mark).all()
        got.append(o[guard:guard + n * w].view(ref.dtype).reshape(ref.shape))
    AC.same_tables(tuple(got), want, 'the first n rows')
