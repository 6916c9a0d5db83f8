"""-m gpu: the surface heat map on the device -- DevicePipeline.surface_heat (mcg_surface_heat_add), DevicePipeline.draw_surface_heat
(mcg_draw_surface_heat, mcg_draw_surface_heat_nv12) and the entries through ctypes.

Every comparison is array_equal against attention.surface_heat_host / arrows.draw_surface_heat_host (themselves checked against hand-worked
charts, grids and levels and scalar restatements in tests/test_surface_heat_cpu.py): no tolerance anywhere.  Scenes come from
tests/surface_heat_cases.py, frames from tests/heat_cases.py (one pitch per access path, a picture that crosses a tile) and
tests.test_gpu_draw's helpers.  The odd rows and regions (NaN and infinite points, kinds and targets outside their ranges, flagged and masked
rows, offsets out of order or beyond the vertex table, regions behind the lens) are table contents the entries document; nothing here
provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import arrows as R
from mcgaze_amd import attention as A
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import heat_cases as HC
from tests import surface_heat_cases as SC
from tests.test_gpu_draw import FORMATS, IDS, as_arrays, device_frames, expected_buffers, host_frames
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MCG_ERR_ARG = 1
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
on_device = lambda t: A.PolyRegions3D(dev(t.xyz), dev(t.start))


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(32))


def state_of(heat):
    return A.SurfaceHeatState(dev(heat), torch.full((heat.shape[0],), -3, dtype=torch.int32, device=DEV))


def state_equals(state, want, what=''):
    assert np.array_equal(state.heat.cpu().numpy(), want[0]) and np.array_equal(state.peak.cpu().numpy(), want[1]), what


def buffers_equal(bufs, want, what=''):
    for k, (bs, es) in enumerate(zip(bufs, want)):
        for b, e in zip(bs, es):
            assert np.array_equal(b.cpu().numpy(), e), (what, k)


@pytest.fixture(scope='module')
def heated():
    """One set of grids per grid shape with something in them, made on the host once and shared (never changed): grid -> (heat, peak)."""
    out = {}
    for grid in SC.GRIDS:
        before = (SC.preloaded(grid).astype(np.int64).clip(0) % 1000).astype(np.int32)
        heat, peak = A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, before, flags=SC.FLAGS, mask=SC.MASK, radius=2)
        heat[0, 0, 0] = -9                                        # a negative cell is drawn as 0
        out[grid] = (heat, peak)
    return out


# ---------------------------------------------------------------- 1. accumulate
@pytest.mark.parametrize('radius', [0, 1, 3])
@pytest.mark.parametrize('grid', SC.GRIDS)
def test_surface_heat_equals_surface_heat_host(pipe, grid, radius):
    before = SC.preloaded(grid)
    tables = (SC.HIT3D, SC.KIND, SC.TARGET)
    for decay, regions in ((0, SC.TABLES), (2, SC.BAD_TABLES)):
        kw = dict(radius=radius, decay=decay)
        want1 = A.surface_heat_host(*tables, regions, before, flags=SC.FLAGS, mask=SC.MASK, **kw)
        want2 = A.surface_heat_host(*tables, regions, want1[0], **kw)                                 # the state carries; no flags, no mask
        want3 = A.surface_heat_host(np.zeros((0, 3), np.float32), [], [], regions, want2[0], **kw)    # no rows: it still decays
        for where, order in (('host', slice(None)), ('device', slice(None)), ('device', slice(None, None, -1)), ('mixed', slice(None))):
            put = dev if where == 'device' else (lambda a: a)
            t = [put(a[order]) for a in tables]
            reg = on_device(regions) if where == 'device' else regions
            if where == 'mixed':
                t[0], reg = dev(t[0]), A.PolyRegions3D(dev(regions.xyz), regions.start)      # one table of a group on the device: the others are moved with torch
            state = state_of(before)
            got = pipe.surface_heat(*t, reg, state, flags=put(SC.FLAGS[order]), mask=put(SC.MASK[order]), device=DEV, **kw)
            assert got is state
            state_equals(state, want1, (where, decay))
            pipe.surface_heat(*t, reg, state, device=DEV, **kw)
            state_equals(state, want2, (where, decay, 'second'))
            pipe.surface_heat(t[0][:0], t[1][:0], t[2][:0], reg, state, device=DEV, **kw)
            state_equals(state, want3, (where, decay, 'n == 0'))
        if decay:
            assert not np.array_equal(want3[0], want2[0])


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_row_counts_around_a_block(pipe, n):
    tables, _, hit, kind, target, flags, mask = SC.random_tables(20 + n, m=6, n=n)
    want = A.surface_heat_host(hit, kind, target, tables, np.zeros((6, 5, 3), np.int32), flags=flags, mask=mask, radius=0)
    state = pipe.surface_heat_state(6, grid=(3, 5), device=DEV)
    pipe.surface_heat(dev(hit), dev(kind), dev(target), on_device(tables), state, flags=dev(flags), mask=dev(mask), radius=0, device=DEV)
    state_equals(state, want, n)


def test_more_rows_than_a_block_one_region_many_regions_and_the_state(pipe):
    """700 rows at radius 8 -- 11900 scatter threads, 47 blocks; M = 1; 40 regions whose 33 x 17 grids span three update blocks each."""
    state = pipe.surface_heat_state(3, device=DEV)
    assert tuple(state.heat.shape) == (3, 32, 32) and tuple(state.peak.shape) == (3,) and state.heat.dtype == state.peak.dtype == torch.int32
    assert not state.heat.any() and tuple(pipe.surface_heat_state(2, grid=(33, 17), device=DEV).heat.shape) == (2, 17, 33)
    for bad in ((0, 4), (4, 1025), (4,), 8, (4.0, 4)):
        with pytest.raises(ValueError):
            pipe.surface_heat_state(2, grid=bad, device=DEV)
    with pytest.raises(ValueError):
        pipe.surface_heat_state(4097, grid=(1, 1), device=DEV)
    tables, _, hit, kind, target, _, _ = SC.random_tables(31, m=40, n=700)
    want = A.surface_heat_host(hit, kind, target, tables, np.zeros((40, 17, 33), np.int32), radius=8)
    state = pipe.surface_heat_state(40, grid=(33, 17), device=DEV)
    pipe.surface_heat(dev(hit), dev(kind), dev(target), on_device(tables), state, radius=8, device=DEV)
    state_equals(state, want)
    assert (want[1] > 0).sum() > 30
    one = A.regions_3d([SC.REGIONS[0][1]])
    want = A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, one, np.zeros((1, 1, 1), np.int32), radius=1)
    state = pipe.surface_heat_state(1, grid=(1, 1), device=DEV)
    pipe.surface_heat(SC.HIT3D, SC.KIND, SC.TARGET, one, state, radius=1, device=DEV)
    state_equals(state, want, 'M = 1')
    assert want[1].tolist() == [5 * 4 + 2 + 1 + 1]                # rows 0, 1, 4, 22, 23 in the one cell; row 2 beside it; rows 3 and 5 at its corners
    with pytest.raises(ValueError):
        pipe.surface_heat(SC.HIT3D, SC.KIND[:5], SC.TARGET, one, state, device=DEV)
    with pytest.raises(ValueError):
        pipe.surface_heat(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, state, device=DEV)       # 14 regions, one grid
    with pytest.raises(TypeError):
        pipe.surface_heat(SC.HIT3D, SC.KIND, SC.TARGET, one, (state.heat, state.peak), device=DEV)
    with pytest.raises(ValueError):
        pipe.surface_heat(SC.HIT3D, SC.KIND, SC.TARGET, one, state, radius=9, device=DEV)


# ---------------------------------------------------------------- 2. render
RENDER = dict(cam_period=SC.CAM_PERIOD)


@pytest.mark.parametrize('grid', [(4, 4), (33, 17)])
@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_draw_surface_heat_equals_draw_surface_heat_host(pipe, heated, fmt, matrix, grid):
    heat, peak = heated[grid]
    frames = HC.host_frames(fmt)
    kw = dict(pixel_format=fmt, matrix=matrix)
    state = A.SurfaceHeatState(dev(heat), dev(peak))
    host = lambda fr=frames, tables=SC.TABLES, full=peak, **more: R.draw_surface_heat_host(fr, heat, full, SC.CAM, tables, SC.REGION_IMAGE, **more, **kw)
    want = host(**RENDER)
    assert all(not np.array_equal(w if fmt == 'bgr' else w[0], f if fmt == 'bgr' else f[0]) for w, f in zip(want, frames))
    # device frames with their own pitches -- one per access path of the kernel --, drawn IN PLACE; the padding is compared byte for byte
    for junk, there in ((255, False), (0, True)):
        views, bufs = HC.device_frames(fmt, junk, DEV)
        tables, cam, ri = (on_device(SC.TABLES), dev(SC.CAM), dev(SC.REGION_IMAGE)) if there else (SC.TABLES, SC.CAM, SC.REGION_IMAGE)
        got = pipe.draw_surface_heat(views, state, cam, tables, ri, device=DEV, **RENDER, **kw)
        torch.cuda.synchronize()
        assert all(g is v for g, v in zip(got, views))
        buffers_equal(bufs, HC.expected_buffers(fmt, want, junk), (junk, 'in place'))
    # pictures 2 and 3 without a camera (cam_period 0, C = 2) come back untouched; a camera row that is not finite; a region period; the
    # offsets that are contents; a fixed scale; thresholds
    broken = SC.CAM.copy()
    broken[1, 2] = np.nan
    for more in (dict(cam_period=0), dict(cam=broken, **RENDER), dict(region_period=2, **RENDER), dict(tables=SC.BAD_TABLES, **RENDER),
                 dict(full_scale=300, **RENDER), dict(min_level=255, **RENDER), dict(min_level=40, full_scale=2 ** 31 - 1, **RENDER)):
        opts = dict(more)
        cam, tables, full = opts.pop('cam', SC.CAM), opts.pop('tables', SC.TABLES), opts.pop('full_scale', None)
        want_m = R.draw_surface_heat_host(frames, heat, peak if full is None else full, cam, tables, SC.REGION_IMAGE, **opts, **kw)
        views, bufs = HC.device_frames(fmt, 255, DEV)
        pipe.draw_surface_heat(views, state, cam, tables, SC.REGION_IMAGE, device=DEV, **opts, **({} if full is None else dict(full_scale=full)), **kw)
        torch.cuda.synchronize()
        buffers_equal(bufs, HC.expected_buffers(fmt, want_m, 255), sorted(more))
        if 'cam_period' in more and more['cam_period'] == 0 or 'cam' in more:
            HC.same(fmt, want_m[3:], frames[3:], 'no camera')
    # copy=True leaves the source untouched; host frames come back as fresh device tensors; mixed host and device frames
    views, bufs = HC.device_frames(fmt, 7, DEV)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    got = pipe.draw_surface_heat(views, state, SC.CAM, SC.TABLES, SC.REGION_IMAGE, copy=True, device=DEV, **RENDER, **kw)
    torch.cuda.synchronize()
    HC.same(fmt, as_arrays(fmt, got), want, 'copy=True')
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    got = pipe.draw_surface_heat(frames, state, SC.CAM, SC.TABLES, SC.REGION_IMAGE, device=DEV, **RENDER, **kw)
    HC.same(fmt, as_arrays(fmt, got), want, 'host frames')
    got = pipe.draw_surface_heat([views[0], frames[1], views[2], frames[3]], state, SC.CAM, SC.TABLES, SC.REGION_IMAGE, device=DEV, **RENDER, **kw)
    HC.same(fmt, as_arrays(fmt, got), want, 'mixed')
    # a ramp of the caller's: a host table is converted like the default, a device table is read as it is
    lut = np.random.RandomState(9).randint(0, 256, (256, 4)).astype(np.uint8)
    want_l = host(lut=lut, **RENDER)
    for table in (lut, dev(R.heat_lut(lut, fmt == 'nv12', matrix))):
        got = pipe.draw_surface_heat(frames, state, SC.CAM, SC.TABLES, SC.REGION_IMAGE, lut=table, device=DEV, **RENDER, **kw)
        HC.same(fmt, as_arrays(fmt, got), want_l, 'lut')


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_the_frames_of_the_drawing_tests_random_regions_and_nothing_to_draw(pipe, heated, fmt, matrix):
    """The 12 x 16, 18 x 22 (odd pitch), 2 x 2 and 40 x 48 (a pitch of 160) frames through tests.test_gpu_draw's helpers, under the scene
    and under random polygons, some of them around and behind the lens; regions that cover nothing leave every byte alone."""
    kw = dict(pixel_format=fmt, matrix=matrix)
    cam = (SC.CAM * np.float32(0.75)).astype(np.float32)
    for grid in ((5, 3), (1, 1)):
        heat, peak = heated[grid]
        want = R.draw_surface_heat_host(host_frames(fmt), heat, peak, cam, SC.TABLES, SC.REGION_IMAGE, **RENDER, **kw)
        views, bufs = device_frames(fmt, 255)
        pipe.draw_surface_heat(views, A.SurfaceHeatState(dev(heat), dev(peak)), cam, SC.TABLES, SC.REGION_IMAGE, device=DEV, **RENDER, **kw)
        torch.cuda.synchronize()
        buffers_equal(bufs, expected_buffers(fmt, want, 255), grid)
    for seed in (41, 42):
        tables, ri, hit, kind, target, _, _ = SC.random_tables(seed, m=12, n=300)
        heat, peak = A.surface_heat_host(hit, kind, target, tables, np.zeros((12, 6, 7), np.int32), radius=2)
        want = R.draw_surface_heat_host(HC.host_frames(fmt), heat, peak, SC.CAM, tables, ri, **RENDER, **kw)
        views, bufs = HC.device_frames(fmt, 255, DEV)
        pipe.draw_surface_heat(views, A.SurfaceHeatState(dev(heat), dev(peak)), SC.CAM, tables, ri, device=DEV, **RENDER, **kw)
        torch.cuda.synchronize()
        buffers_equal(bufs, HC.expected_buffers(fmt, want, 255), seed)
    nothing = A.regions_3d([SC.REGIONS[k][1] for k in (10, 12, 13)])
    views, bufs = device_frames(fmt, 0)
    pipe.draw_surface_heat(views, A.SurfaceHeatState(dev(np.full((3, 4, 4), 9, np.int32)), dev(np.full(3, 9, np.int32))), cam, nothing, device=DEV, **RENDER, **kw)
    torch.cuda.synchronize()
    buffers_equal(bufs, expected_buffers(fmt, host_frames(fmt), 0), 'nothing to draw')


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_a_wide_picture_regions_that_are_not_flat_and_regions_on_tile_borders(pipe, fmt, matrix):
    """72 x 648: three tiles across, five (NV12: three) tile rows.  The oblique quadrilateral and the pentagon are NOT coplanar: what the
    exact test covers reaches beyond the box of their projected vertices, into tiles that box does not touch -- the tile lists must
    still hold them.  Small squares sit on the tile borders at x = 256 and 512 and y = 16, 32, 48."""
    h, w = SC.WIDE_HW
    m = len(SC.WIDE_REGIONS)
    heat = np.random.RandomState(8).randint(1, 1000, (m, 6, 9)).astype(np.int32)
    peak = heat.reshape(m, -1).max(axis=1).astype(np.int32)
    # the scene is what it is meant to be: thousands of pixels of region 0 lie in tiles that the box of its projected vertices does not touch
    region, _ = R.surface_cover(h, w, SC.WIDE_CAM[0].astype(np.float64), A.surface_charts_host(SC.WIDE_TABLES), SC.WIDE_TABLES.xyz.astype(np.float64),
                                SC.WIDE_TABLES.start, range(m))
    assert SC.beyond_the_vertex_box(region, 0, 32 if fmt == 'nv12' else 16) > 1000 and {int(j) for j in np.unique(region)} == set(range(-1, m))
    rs = np.random.RandomState(21)
    if fmt == 'bgr':
        frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2)]
        views = [dev(f) for f in frames]
    else:
        frames = [(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w)).astype(np.uint8)) for _ in range(2)]
        views = [(dev(y), dev(uv)) for y, uv in frames]
    kw = dict(cam_period=1, pixel_format=fmt, matrix=matrix)
    want = R.draw_surface_heat_host(frames, heat, peak, SC.WIDE_CAM, SC.WIDE_TABLES, **kw)
    got = pipe.draw_surface_heat(views, A.SurfaceHeatState(dev(heat), dev(peak)), dev(SC.WIDE_CAM), on_device(SC.WIDE_TABLES), device=DEV, **kw)
    torch.cuda.synchronize()
    HC.same(fmt, as_arrays(fmt, got), want, 'wide')


# ---------------------------------------------------------------- 3. the entries
def test_the_entries_refuse_bad_arguments_and_write_nothing():
    lib = L.load()
    vp = C.c_void_p
    n, M, V = len(SC.ROWS), SC.M, len(SC.XYZ)
    hit, kind, target, xyz, start, ri, cam = (dev(a) for a in (SC.HIT3D, SC.KIND, SC.TARGET, SC.XYZ, SC.START, SC.REGION_IMAGE, SC.CAM))
    need = 160 * M + 4 * M * 15
    heat, peak = dev(SC.preloaded((5, 3))), torch.full((M,), -3, dtype=torch.int32, device=DEV)
    work = torch.full((need // 4 + 2,), -5, dtype=torch.int32, device=DEV)
    keep = heat.clone()
    stream = vp(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: vp(t.data_ptr() if t is not None else 0)

    def add(hit=hit, kind=kind, target=target, n=n, xyz=xyz, V=V, start=start, M=M, heat=heat, peak=peak, GH=3, GW=5, radius=1, decay=0, work=work.data_ptr(),
            work_bytes=need):
        return lib.mcg_surface_heat_add(stream, ptr(hit), ptr(kind), ptr(target), vp(0), vp(0), n, ptr(xyz), V, ptr(start), M, ptr(heat), ptr(peak), GH, GW,
                                        radius, decay, vp(work), work_bytes)

    for kw in (dict(hit=None), dict(kind=None), dict(target=None), dict(heat=None), dict(peak=None), dict(work=0), dict(work=work.data_ptr() + 4), dict(xyz=None),
               dict(start=None), dict(n=-1), dict(n=65537), dict(V=-1), dict(V=65537), dict(M=0), dict(M=4097), dict(GH=0), dict(GW=1025), dict(radius=-1),
               dict(radius=9), dict(decay=-1), dict(decay=31), dict(work_bytes=need - 1)):
        assert add(**kw) == MCG_ERR_ARG, kw
    torch.cuda.synchronize()
    assert torch.equal(heat, keep) and (peak == -3).all() and (work == -5).all()
    assert add() == 0                                             # ... and as documented it runs
    want = A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, keep.cpu().numpy(), radius=1)
    state_equals(A.SurfaceHeatState(heat, peak), want)
    charts = work[:40 * M].view(torch.float64).cpu().numpy().reshape(M, 20)                       # the plan launch's table, bit for bit
    assert np.array_equal(charts.view(np.uint64), A.surface_charts_host(SC.TABLES).view(np.uint64))
    assert (work[need // 4:] == -5).all()

    views, bufs = HC.device_frames('bgr', 255, DEV)
    table = np.zeros(4, dtype=P._IMAGE)
    for k, v in enumerate(views):
        table[k] = (v.data_ptr(), v.shape[0], v.shape[1], v.stride(0))
    images, lut = dev(table.view(np.uint8)), dev(R.HEAT_LUT.copy())      # (the default ramp is read-only)
    before = [b[0].clone() for b in bufs]
    work.fill_(-5)

    def draw(images=images, num=4, max_h=37, max_w=300, cam=cam, Cn=2, cam_period=2, xyz=xyz, V=V, start=start, ri=ri, M=M, region_period=0, heat=heat,
             full=peak, GH=3, GW=5, lut=lut.data_ptr(), min_level=1, work=work.data_ptr(), work_bytes=160 * M):
        return lib.mcg_draw_surface_heat(stream, ptr(images), num, max_h, max_w, ptr(cam), Cn, cam_period, ptr(xyz), V, ptr(start), ptr(ri), M, region_period,
                                         ptr(heat), ptr(full), GH, GW, vp(lut), min_level, vp(work), work_bytes)

    for kw in (dict(images=None), dict(cam=None), dict(xyz=None), dict(start=None), dict(ri=None), dict(heat=None), dict(full=None), dict(lut=0),
               dict(lut=lut.data_ptr() + 1), dict(work=0), dict(work=work.data_ptr() + 4), dict(num=0), dict(num=65536), dict(max_h=0), dict(max_w=8193),
               dict(Cn=0), dict(Cn=4097), dict(cam_period=-1), dict(region_period=-1), dict(V=65537), dict(M=0), dict(M=4097), dict(GH=1025), dict(GW=0),
               dict(min_level=0), dict(min_level=256), dict(work_bytes=160 * M - 1)):
        assert draw(**kw) == MCG_ERR_ARG, kw
    torch.cuda.synchronize()
    assert all(torch.equal(b[0], k) for b, k in zip(bufs, before)) and (work == -5).all()
    # a picture larger than (max_h, max_w) is left untouched: max_w = 53 leaves out the 20 x 300 picture
    assert draw(max_w=53) == 0
    torch.cuda.synchronize()
    want = R.draw_surface_heat_host(HC.BGR_FRAMES, heat.cpu().numpy(), peak.cpu().numpy(), SC.CAM, SC.TABLES, SC.REGION_IMAGE, cam_period=2)
    buffers_equal(bufs, HC.expected_buffers('bgr', want[:3] + [HC.BGR_FRAMES[3]], 255), 'max_w')


def test_both_calls_are_capturable(pipe):
    """Device tables and device frames, captured once, replayed with new rows in the same buffers: the grids go on accumulating and the
    frames are drawn over again."""
    grid = (6, 5)
    cases = [SC.random_tables(50, m=6, n=60, rows_seed=60 + k) for k in range(3)]
    tables, ri = on_device(cases[0][0]), dev(cases[0][1])
    bufs = [dev(t) for t in cases[0][2:5]]
    cam = dev(SC.CAM)
    state = pipe.surface_heat_state(6, grid=grid, device=DEV)
    views, fbufs = HC.device_frames('bgr', 255, DEV)

    def call():
        pipe.surface_heat(*bufs, tables, state, radius=2, decay=2, device=DEV)
        pipe.draw_surface_heat(views, state, cam, tables, ri, cam_period=2, device=DEV)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()                                                    # warm-up outside the capture: the workspaces, the ramp and the frame table are kept
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for case in cases:
        for b, t in zip(bufs, case[2:5]):
            b.copy_(dev(t))
        state.heat.zero_()
        for (buf,), f in zip(fbufs, HC.BGR_FRAMES):
            buf[:, :3 * f.shape[1]] = dev(f.reshape(f.shape[0], -1))
        graph.replay()
        torch.cuda.synchronize()
        heat, peak = A.surface_heat_host(*case[2:5], case[0], np.zeros((6, 5, 6), np.int32), radius=2, decay=2)
        state_equals(state, (heat, peak), 'replay')
        assert peak.max() > 0
        buffers_equal(fbufs, HC.expected_buffers('bgr', R.draw_surface_heat_host(HC.BGR_FRAMES, heat, peak, SC.CAM, case[0], case[1], cam_period=2), 255),
                      'replay')
