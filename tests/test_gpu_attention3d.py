"""mcg_gaze_targets_3d on the device against attention.gaze_targets_3d_host, all seven tables bit for bit (include/mcgaze_hip.h, "gaze
targets, 3-D"): every case of tests/attention3d_cases.py, the tile edges of the kernel (256 rows and 256 regions a tile), pictures shuffled
and in order, polygons of 3, 4, 31 and 32 vertices with the vertex table ending at and one short of the last polygon, depth given and not,
both frames, strided gaze tables, host, device and mixed tables, n == 0, guard words, the argument errors, no host touch and graph
capture."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import attention as AT
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import attention3d_cases as TC
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = TC.all_cases()
ROWS = ('boxes', 'gaze', 'image_of', 'cam', 'depth', 'region_image')
MCG_ERR_ARG = 1                                                  # include/mcgaze_hip.h


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(64))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def on_device(pipe, a, tables=True):
    """gaze_targets_3d over the arguments of gaze_targets_3d_host: every table a device tensor, or as they are (through the staging ring)."""
    a = dict(a)
    if tables:
        a = {k: dev(v) if k in ROWS and v is not None else v for k, v in a.items()}
        if a.get('regions') is not None:
            a['regions'] = AT.PolyRegions3D(dev(a['regions'].xyz), dev(a['regions'].start))
    got = pipe.gaze_targets_3d(a.pop('boxes'), a.pop('gaze'), a.pop('image_of'), a.pop('cam'), device=DEV, **a)
    torch.cuda.synchronize()
    return tuple(g.cpu().numpy() for g in got)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_every_cpu_case(pipe, case):
    want = AT.gaze_targets_3d_host(**TC.args(case))
    TC.check_expect(want, case)
    TC.same_tables(on_device(pipe, TC.args(case)), want, case['name'] + ' (device tables)')
    TC.same_tables(on_device(pipe, TC.args(case), tables=False), want, case['name'] + ' (host tables, as the case gives them)')


@pytest.mark.parametrize('n,pictures,m,shuffle,garbage,depth,frame', [
    (255, 2, 255, True, 0, True, 'eye'), (256, 2, 256, True, 0, False, 'camera'), (257, 2, 257, True, 0, True, 'camera'), (600, 7, 16, True, 0, True, 'eye'),
    (600, 7, 16, False, 0, False, 'eye'), (300, 40, 257, False, 6, True, 'camera'), (300, 3, 0, True, 0, True, 'eye'), (300, 3, 1, False, 0, False, 'camera')])
def test_tile_edges_and_the_skip_branch(pipe, n, pictures, m, shuffle, garbage, depth, frame):
    """256 rows and 256 regions a tile: one short of a tile, a full tile, one over; 600 rows in 7 pictures shuffled (no tile is skipped) and in
    ascending order (a workgroup skips the tiles of the other pictures); two region tiles keyed by camera with garbage among the offsets; 0
    and 1 regions; depth given and NULL; both frames."""
    case = TC.random_case(300 + n + m, n, pictures, m, cameras=4 if garbage else 2, period=4 if garbage else 0, shuffle=shuffle, garbage=garbage,
                          depth=depth, frame=frame)
    a = TC.args(case)
    want = AT.gaze_targets_3d_host(**a)
    assert len(set(want[0].tolist())) >= 3
    TC.same_tables(on_device(pipe, a), want, case['name'])


def test_polygons_of_3_4_31_and_32_vertices_and_offsets_of_garbage(pipe):
    case = TC.random_case(77, 300, 2, 24, counts=(3, 4, 31, 32), bad=0.0)
    a = TC.args(case)
    xyz, start = a['regions']
    assert sorted(set(np.diff(start).tolist())) == [3, 4, 31, 32] and start[-1] == len(xyz)
    want = AT.gaze_targets_3d_host(**a)
    assert {3, 4, 31, 32} <= set(np.diff(start)[want[1][want[0] == AT.KIND_REGION]].tolist())
    TC.same_tables(on_device(pipe, a), want, 'V exactly at the last polygon\'s end')
    rng = np.random.default_rng(5)
    words = rng.integers(-2 ** 31, 2 ** 31, len(start)).astype(np.int32)         # every offset a garbage word: nothing outside xyz is read
    words[::4] = rng.integers(-40, len(xyz) + 40, len(words[::4]))
    b = dict(a, regions=AT.PolyRegions3D(xyz, words))
    TC.same_tables(on_device(pipe, b), AT.gaze_targets_3d_host(**b), 'garbage offsets')
    short = dict(a, regions=AT.PolyRegions3D(xyz[:-1], start))   # the last polygon one vertex beyond the table: not usable
    want = AT.gaze_targets_3d_host(**short)
    assert not (want[1][want[0] == AT.KIND_REGION] == len(start) - 2).any()
    TC.same_tables(on_device(pipe, short), want, 'V one short of the last polygon\'s end')


def test_rows_cameras_and_regions_are_each_decided_as_a_group(pipe):
    """Host, device and mixed tables: a group that is all on the host goes up through the one stage of the call; one table of a group on
    the device moves the rest of that group with torch."""
    a = TC.args(TC.random_case(9, 90, 3, 10, cameras=3, period=3))
    want = AT.gaze_targets_3d_host(**a)
    xyz, start = a['regions']
    rows = {k: dev(a[k]) for k in ('boxes', 'gaze', 'image_of', 'depth')}
    everything = dict(a, **rows, cam=dev(a['cam']), regions=AT.PolyRegions3D(dev(xyz), dev(start)), region_image=dev(a['region_image']))
    for what, b, stages in (('all on the host', dict(a), 1), ('rows on the device', dict(a, **rows), 1), ('the cameras on the device', dict(a, cam=dev(a['cam'])), 1),
                            ('regions on the device', dict(a, regions=everything['regions'], region_image=everything['region_image']), 1),
                            ('depth and start alone on the device', dict(a, depth=rows['depth'], regions=AT.PolyRegions3D(xyz, dev(start))), 1),
                            ('everything on the device', everything, 0)):
        before = pipe._ring.i
        got = pipe.gaze_targets_3d(b.pop('boxes'), b.pop('gaze'), b.pop('image_of'), b.pop('cam'), device=DEV, **b)
        assert pipe._ring.i == (before + stages) % pipe.STAGES, what
        torch.cuda.synchronize()
        TC.same_tables(tuple(g.cpu().numpy() for g in got), want, what)


def test_strided_gaze_tables(pipe):
    a = TC.args(TC.random_case(11, 70, 2, 9))
    want = AT.gaze_targets_3d_host(**a)
    wide = np.full((70, 5), 7.0, np.float32)                      # the fused [n, 3] inside a wider tensor
    wide[:, :3] = a['gaze']
    tail = np.full((70, 8), 7.0, np.float32)
    tail[:, 5:] = a['gaze']
    b = {k: dev(a[k]) for k in ('boxes', 'image_of', 'cam', 'depth', 'region_image')}
    regions = AT.PolyRegions3D(dev(a['regions'].xyz), dev(a['regions'].start))
    for what, g in (('[n, 5] rows', dev(wide)), ('a [:, :3] view of [n, 5]', dev(wide)[:, :3]), ('a [:, 5:] view of [n, 8]', dev(tail)[:, 5:])):
        got = pipe.gaze_targets_3d(b['boxes'], g, b['image_of'], b['cam'], depth=b['depth'], regions=regions, region_image=b['region_image'],
                                   cam_period=a['cam_period'], head_size=a['head_size'], frame=a['frame'], device=DEV)
        TC.same_tables(tuple(x.cpu().numpy() for x in got), want, what)


def test_device_tables_with_no_host_touch_captured_and_replayed(pipe, monkeypatch):
    first, second, third = (TC.args(TC.random_case(s, 300, 3, 20, cameras=2, period=2)) for s in (21, 22, 23))
    V, M = (max(len(c['regions'][k]) for c in (first, second, third)) for k in (0, 1))

    def padded(c):                                                # one shape for the three: vertices nobody owns, regions without vertices
        xyz, start = c['regions']
        return dict(boxes=c['boxes'], gaze=c['gaze'], image_of=c['image_of'], cam=c['cam'], depth=c['depth'],
                    xyz=np.concatenate([xyz, np.zeros((V - len(xyz), 3), np.float32)]), start=np.concatenate([start, np.full(M - len(start), start[-1], np.int32)]),
                    region_image=np.concatenate([c['region_image'], np.full(M - len(start), -1, np.int32)]))

    bufs = {k: dev(v) for k, v in padded(first).items()}
    call = lambda: pipe.gaze_targets_3d(bufs['boxes'], bufs['gaze'], bufs['image_of'], bufs['cam'], depth=bufs['depth'],
                                        regions=AT.PolyRegions3D(bufs['xyz'], bufs['start']), region_image=bufs['region_image'], region_period=2,
                                        cam_period=2, head_size=0.25, device=DEV)
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
        want = AT.gaze_targets_3d_host(**dict(case, regions=AT.PolyRegions3D(p['xyz'], p['start']), region_image=p['region_image']))
        TC.same_tables(tuple(x.cpu().numpy() for x in out), want, 'replay')
        TC.same_tables(want, AT.gaze_targets_3d_host(**case), 'the padding adds nothing')


def entry_args(a, n, outs, guard=0, depth=True):
    """The arguments of the entry itself for the tables of a case, device tensors kept alive by the caller's list."""
    xyz, start = a['regions']
    keep = [dev(t) for t in (a['boxes'], a['gaze'], a['image_of'], a['cam'], a['depth'], xyz, start, a['region_image'])]
    b, g, io, cam, d, v, s, ri = keep
    vp = C.c_void_p
    return keep, [vp(torch.cuda.current_stream().cuda_stream), vp(b.data_ptr()), vp(g.data_ptr()), 3, vp(io.data_ptr()), n, vp(cam.data_ptr()), len(a['cam']),
                  a['cam_period'], vp(d.data_ptr()) if depth else None, a['head_size'], AT.GAZE_FRAMES.index(a['frame']), vp(v.data_ptr()), len(xyz),
                  vp(s.data_ptr()), vp(ri.data_ptr()), len(start) - 1, a['region_period'], 0.25, AT._target_params()[1],
                  *(vp(o.data_ptr() + 4 * guard) for o in outs)]


def test_guard_words_and_rows_beyond_n_stay_untouched():
    """The entry itself, on outputs that lie inside larger guarded arrays: n of the 300 rows are written, nothing before, behind or beyond."""
    lib = L.load()
    a = TC.args(TC.random_case(31, 300, 3, 20, cameras=2))
    n, rows, guard, mark = 270, 300, 64, 0x5a5a5a5a
    want = AT.gaze_targets_3d_host(**dict(a, boxes=a['boxes'][:n], gaze=a['gaze'][:n], image_of=a['image_of'][:n], depth=a['depth'][:n]))
    words = (1, 1, 1, 2, 1, 1, 3)                                 # 32-bit words per row: kind, target, t, hit, mutual, flags, hit3d
    outs = [torch.full((guard + rows * w + guard,), mark, dtype=torch.int32, device=DEV) for w in words]
    keep, args = entry_args(a, n, outs, guard)
    L.check(lib.mcg_gaze_targets_3d(*args), 'mcg_gaze_targets_3d')
    torch.cuda.synchronize()
    got = []
    for o, w, ref in zip(outs, words, want):
        o = o.cpu().numpy()
        assert (o[:guard] == mark).all() and (o[guard + n * w:] == mark).all()
        got.append(o[guard:guard + n * w].view(ref.dtype).reshape(ref.shape))
    TC.same_tables(tuple(got), want, 'the first n rows')


def test_every_documented_argument_error_writes_nothing(pipe):
    lib = L.load()
    a = TC.args(TC.random_case(32, 40, 2, 5, cameras=2))
    mark, words = 0x5a5a5a5a, (1, 1, 1, 2, 1, 1, 3)
    outs = [torch.full((40 * w,), mark, dtype=torch.int32, device=DEV) for w in words]
    keep, good = entry_args(a, 40, outs)
    # positions in the argument list: 3 gaze_stride, 5 n, 6 cam, 7 num_cameras, 8 cam_period, 10 head_size, 11 frame, 12 xyz, 13 V, 14 start,
    # 15 region_image, 16 m, 17 region_period, 18 expand, 19 camera_cos2, 20 .. 26 the outputs
    for at, value in ((5, -1), (5, AT.MAX_ROWS + 1), (16, -1), (16, AT.MAX_REGIONS + 1), (13, -1), (13, AT.MAX_VERTICES + 1), (7, 0), (7, AT.MAX_CAMERAS + 1),
                      (3, 2), (17, -1), (8, -1), (18, -1.0), (18, float('inf')), (18, float('nan')), (19, float('nan')), (10, 0.0), (10, float('inf')),
                      (10, float('nan')), (11, 2), (1, None), (2, None), (4, None), (6, None), (12, None), (14, None), (15, None), (20, None), (23, None),
                      (24, None), (26, None)):
        bad = list(good)
        bad[at] = value
        assert lib.mcg_gaze_targets_3d(*bad) == MCG_ERR_ARG, (at, value)
        assert b'mcg_gaze_targets_3d' in lib.mcg_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == mark).all()) for o in outs), 'an argument error wrote to an output'
    L.check(lib.mcg_gaze_targets_3d(*good), 'mcg_gaze_targets_3d')  # the same arguments, unspoilt, are a valid call
    torch.cuda.synchronize()
    got = tuple(o.cpu().numpy().view(r.dtype).reshape(r.shape) for o, r in zip(outs, AT.gaze_targets_3d_host(**a)))
    TC.same_tables(got, AT.gaze_targets_3d_host(**a), 'the valid call')
    b, g, io, cam = (dev(a[k]) for k in ('boxes', 'gaze', 'image_of', 'cam'))
    xyz, start = dev(a['regions'].xyz), dev(a['regions'].start)
    for bad in (dict(regions=AT.PolyRegions3D(xyz[:, :2], start)), dict(regions=AT.PolyRegions3D(xyz, start[:0])), dict(regions=AT.PolyRegions3D(xyz, start.view(1, -1))),
                dict(regions=AT.PolyRegions3D(xyz, start), region_image=dev(np.zeros(3, np.int32))), dict(expand=-1), dict(head_size=0), dict(frame='world'),
                dict(cam_period=-1), dict(depth=dev(np.zeros(3, np.float32))), dict(region_image=dev(np.zeros(3, np.int32))),
                dict(regions=AT.PolyRegions3D(dev(np.zeros((AT.MAX_VERTICES + 1, 3), np.float32)), start)),
                dict(regions=AT.PolyRegions3D(xyz, dev(np.zeros(AT.MAX_REGIONS + 2, np.int32)))), dict(regions=[TC.SCREEN[:2]])):
        with pytest.raises(ValueError):
            pipe.gaze_targets_3d(b, g, io, cam, device=DEV, **bad)
    for bad_cam in (cam[:, :3], cam[:0], dev(np.zeros((AT.MAX_CAMERAS + 1, 4), np.float32))):
        with pytest.raises(ValueError):
            pipe.gaze_targets_3d(b, g, io, bad_cam, device=DEV)
    with pytest.raises(TypeError):
        pipe.gaze_targets_3d(b, g, io, cam, device=DEV, regions=[TC.SCREEN, 5])


def test_no_rows(pipe):
    a = TC.args(TC.random_case(33, 10, 2, 3))
    for tables in (True, False):
        b = dict(a, boxes=a['boxes'][:0], gaze=a['gaze'][:0], image_of=a['image_of'][:0], depth=a['depth'][:0])
        empty = on_device(pipe, b, tables=tables)
        assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0,), (0, 2), (0,), (0,), (0, 3)]
        TC.same_tables(empty, AT.gaze_targets_3d_host(**b), 'n == 0')
