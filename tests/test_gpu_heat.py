"""-m gpu: the gaze heat map on the device -- DevicePipeline.gaze_heat (mcg_gaze_heat_add), DevicePipeline.draw_heat (mcg_draw_heat,
mcg_draw_heat_nv12) and the entries through ctypes.

Every comparison is array_equal against attention.gaze_heat_host / arrows.draw_heat_host (themselves checked against hand-worked grids and
pixels and scalar restatements in tests/test_heat_cpu.py): no tolerance anywhere.  Scenes come from tests/heat_cases.py; the frames of
tests/draw_cases.py go through tests.test_gpu_draw's helpers as well.  The odd rows (a NaN, an infinite and a far hit, kind words outside the
mask, flagged and masked rows, image_of -1 or beyond the cameras) are table contents the entries document; nothing here provokes a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import arrows as R
from mcgaze_amd import attention as A
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import heat_cases as HC
from tests.test_gpu_draw import FORMATS, IDS, as_arrays, device_frames, expected_buffers, host_frames
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
MCG_ERR_ARG = 1
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(32))


def state_of(heat, cell_shift):
    return A.HeatState(dev(heat), torch.full((heat.shape[0],), -3, dtype=torch.int32, device=DEV), cell_shift)


def buffers_equal(bufs, want, what=''):
    for k, (bs, es) in enumerate(zip(bufs, want)):
        for b, e in zip(bs, es):
            assert np.array_equal(b.cpu().numpy(), e), (what, k)


@pytest.fixture(scope='module')
def heated():
    """One grid per cell size with something in it, made on the host once and shared (never changed): cell_shift -> (heat, peak)."""
    out = {}
    for cell_shift, grid in HC.GRIDS:
        heat, peak = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, np.maximum(HC.preloaded(cell_shift, grid), 0) % 1000, flags=HC.FLAGS, mask=HC.MASK,
                                      cell_shift=cell_shift, radius=3, period=HC.PERIOD)
        heat[0, 0, 0] = -9                                        # a negative cell is drawn as 0
        out[cell_shift, grid] = (heat, peak)
    return out


# ---------------------------------------------------------------- 1. accumulate
@pytest.mark.parametrize('radius', HC.RADII)
@pytest.mark.parametrize('cell_shift,grid', HC.GRIDS)
def test_gaze_heat_equals_gaze_heat_host(pipe, cell_shift, grid, radius):
    before = HC.preloaded(cell_shift, grid)
    tables = (HC.HIT, HC.KIND, HC.IMAGE_OF)
    for decay, kinds, period in ((0, ('head', 'region'), HC.PERIOD), (1, 0b1111, HC.PERIOD), (30, 0b0110, 0)):
        kw = dict(radius=radius, kinds=kinds, period=period, decay=decay)
        want1 = A.gaze_heat_host(*tables, before, flags=HC.FLAGS, mask=HC.MASK, cell_shift=cell_shift, **kw)
        want2 = A.gaze_heat_host(*tables, want1[0], cell_shift=cell_shift, **kw)                      # the state carries; no flags, no mask
        want3 = A.gaze_heat_host(np.zeros((0, 2), np.float32), [], [], want2[0], cell_shift=cell_shift, **kw)   # no rows: it still decays
        for where, order in (('host', slice(None)), ('device', slice(None)), ('device', slice(None, None, -1)), ('mixed', slice(None))):
            put = dev if where == 'device' else (lambda a: a)
            t = [put(a[order]) for a in tables]
            if where == 'mixed':
                t[0] = dev(t[0])                                  # one table on the device: the others are moved with torch
            state = state_of(before, cell_shift)
            got = pipe.gaze_heat(*t, state, flags=put(HC.FLAGS[order]), mask=put(HC.MASK[order]), device=DEV, **kw)
            assert got is state
            assert np.array_equal(state.heat.cpu().numpy(), want1[0]) and np.array_equal(state.peak.cpu().numpy(), want1[1]), (where, decay)
            pipe.gaze_heat(*t, state, device=DEV, **kw)
            assert np.array_equal(state.heat.cpu().numpy(), want2[0]) and np.array_equal(state.peak.cpu().numpy(), want2[1]), (where, decay, 'second')
            pipe.gaze_heat(t[0][:0], t[1][:0], t[2][:0], state, device=DEV, **kw)
            assert np.array_equal(state.heat.cpu().numpy(), want3[0]) and np.array_equal(state.peak.cpu().numpy(), want3[1]), (where, decay, 'n == 0')
        if decay == 1:
            assert not np.array_equal(want3[0], want2[0])


def test_more_rows_than_a_block_and_the_heat_state(pipe):
    """700 rows at radius 8 -- 11900 scatter threads, 47 blocks -- over 3 cameras whose grids span several update blocks; heat_state's shapes."""
    state = pipe.heat_state(3, HC.FRAME_HW, cell=1, device=DEV)
    assert tuple(state.heat.shape) == (3, 37, 53) and tuple(state.peak.shape) == (3,) and state.cell_shift == 0
    assert state.heat.dtype == state.peak.dtype == torch.int32 and not state.heat.any()
    assert tuple(pipe.heat_state(2, HC.FRAME_HW, device=DEV).heat.shape) == (2, 5, 7) and pipe.heat_state(2, HC.FRAME_HW, cell=64, device=DEV).cell_shift == 6
    for bad in (0, 3, 12, 128, 8.0):
        with pytest.raises(ValueError):
            pipe.heat_state(2, HC.FRAME_HW, cell=bad, device=DEV)
    rs = np.random.RandomState(11)
    hit = rs.uniform(-12, 70, (700, 2)).astype(np.float32)
    kind, image_of = rs.randint(0, 4, 700).astype(np.int32), rs.randint(-1, 5, 700).astype(np.int32)
    want = A.gaze_heat_host(hit, kind, image_of, np.zeros((3, 37, 53), np.int32), cell_shift=0, radius=8)
    pipe.gaze_heat(dev(hit), dev(kind), dev(image_of), state, radius=8, device=DEV)
    assert np.array_equal(state.heat.cpu().numpy(), want[0]) and np.array_equal(state.peak.cpu().numpy(), want[1]) and want[1].min() > 0
    with pytest.raises(ValueError):
        pipe.gaze_heat(hit, kind[:5], image_of, state, device=DEV)
    with pytest.raises(TypeError):
        pipe.gaze_heat(hit, kind, image_of, (state.heat, state.peak, 0), device=DEV)
    with pytest.raises(ValueError):
        pipe.gaze_heat(hit, kind, image_of, state, radius=9, device=DEV)


# ---------------------------------------------------------------- 2. render
@pytest.mark.parametrize('cell_shift,grid', HC.GRIDS)
@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_draw_heat_equals_draw_heat_host(pipe, heated, fmt, matrix, cell_shift, grid):
    heat, peak = heated[cell_shift, grid]
    frames = HC.host_frames(fmt)
    kw = dict(pixel_format=fmt, matrix=matrix)
    state = A.HeatState(dev(heat), dev(peak), cell_shift)
    want = R.draw_heat_host(frames, heat, peak, cell_shift, period=HC.PERIOD, **kw)
    assert all(not np.array_equal(w if fmt == 'bgr' else w[0], f if fmt == 'bgr' else f[0]) for w, f in zip(want, frames))
    # device frames with their own pitches -- one per access path of the kernel --, drawn IN PLACE; the padding is compared byte for byte
    for junk in (255, 0):
        views, bufs = HC.device_frames(fmt, junk, DEV)
        got = pipe.draw_heat(views, state, period=HC.PERIOD, device=DEV, **kw)
        torch.cuda.synchronize()
        assert all(g is v for g, v in zip(got, views))
        buffers_equal(bufs, HC.expected_buffers(fmt, want, junk), (junk, 'period 2'))
    # period 0: pictures 2 and 3 show cameras that have no grid and come back untouched; a fixed scale; a threshold
    for more in (dict(period=0), dict(period=HC.PERIOD, full_scale=300), dict(period=HC.PERIOD, min_level=255), dict(period=HC.PERIOD, min_level=40, full_scale=2 ** 31 - 1)):
        host = dict(more)
        full = host.pop('full_scale', None)
        want_m = R.draw_heat_host(frames, heat, peak if full is None else full, cell_shift, **host, **kw)
        views, bufs = HC.device_frames(fmt, 255, DEV)
        pipe.draw_heat(views, state, device=DEV, **more, **kw)
        torch.cuda.synchronize()
        buffers_equal(bufs, HC.expected_buffers(fmt, want_m, 255), more)
    # copy=True leaves the source untouched; host frames come back as fresh device tensors; mixed host and device frames
    views, bufs = HC.device_frames(fmt, 7, DEV)
    keep = [tuple(b.clone() for b in bs) for bs in bufs]
    got = pipe.draw_heat(views, state, period=HC.PERIOD, copy=True, device=DEV, **kw)
    torch.cuda.synchronize()
    HC.same(fmt, as_arrays(fmt, got), want, 'copy=True')
    assert all(torch.equal(b, c) for bs, cs in zip(bufs, keep) for b, c in zip(bs, cs))
    got = pipe.draw_heat(frames, state, period=HC.PERIOD, device=DEV, **kw)
    HC.same(fmt, as_arrays(fmt, got), want, 'host frames')
    got = pipe.draw_heat([views[0], frames[1], views[2], frames[3]], state, period=HC.PERIOD, device=DEV, **kw)
    HC.same(fmt, as_arrays(fmt, got), want, 'mixed')
    # a ramp of the caller's: a host table is converted like the default, a device table is read as it is
    lut = np.random.RandomState(9).randint(0, 256, (256, 4)).astype(np.uint8)
    want_l = R.draw_heat_host(frames, heat, peak, cell_shift, period=HC.PERIOD, lut=lut, **kw)
    for table in (lut, dev(R.heat_lut(lut, fmt == 'nv12', matrix))):
        got = pipe.draw_heat(frames, state, period=HC.PERIOD, lut=table, device=DEV, **kw)
        HC.same(fmt, as_arrays(fmt, got), want_l, 'lut')


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_the_frames_of_the_drawing_tests_and_an_empty_grid(pipe, heated, fmt, matrix):
    """The 12 x 16, 18 x 22 (odd pitch), 2 x 2 and 40 x 48 (a pitch of 160) frames through tests.test_gpu_draw's helpers; the grid is the
    one made for a 37 x 53 frame, so the 40 x 48 picture reads repeated edge cells."""
    kw = dict(pixel_format=fmt, matrix=matrix)
    for (cell_shift, grid), (heat, peak) in heated.items():
        want = R.draw_heat_host(host_frames(fmt), heat, peak, cell_shift, period=HC.PERIOD, **kw)
        views, bufs = device_frames(fmt, 255)
        pipe.draw_heat(views, A.HeatState(dev(heat), dev(peak), cell_shift), period=HC.PERIOD, device=DEV, **kw)
        torch.cuda.synchronize()
        buffers_equal(bufs, expected_buffers(fmt, want, 255), (cell_shift, grid))
    views, bufs = device_frames(fmt, 0)
    pipe.draw_heat(views, pipe.heat_state(HC.C, (40, 48), device=DEV), period=HC.PERIOD, device=DEV, **kw)
    torch.cuda.synchronize()
    buffers_equal(bufs, expected_buffers(fmt, host_frames(fmt), 0), 'an empty grid')


# ---------------------------------------------------------------- 3. the entries
def test_the_entries_refuse_bad_arguments_and_write_nothing():
    lib = L.load()
    vp = C.c_void_p
    n = len(HC.ROWS)
    hit, kind, image_of = dev(HC.HIT), dev(HC.KIND), dev(HC.IMAGE_OF)
    heat, peak, work = dev(HC.preloaded(3, (5, 7))), torch.full((2,), -3, dtype=torch.int32, device=DEV), torch.full((70,), -5, dtype=torch.int32, device=DEV)
    keep = heat.clone()
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def add(hit=hit, kind=kind, image_of=image_of, n=n, heat=heat, peak=peak, Cn=2, GH=5, GW=7, shift=3, radius=2, kinds=6, period=0, decay=0, work=work,
            work_bytes=280):
        ptr = lambda t: vp(t.data_ptr() if t is not None else 0)
        return lib.mcg_gaze_heat_add(stream, ptr(hit), ptr(kind), ptr(image_of), vp(0), vp(0), n, ptr(heat), ptr(peak), Cn, GH, GW, shift, radius, kinds,
                                     period, decay, ptr(work), work_bytes)

    for kw in (dict(hit=None), dict(kind=None), dict(image_of=None), dict(heat=None), dict(peak=None), dict(work=None), dict(n=-1), dict(n=65537), dict(Cn=0),
               dict(Cn=4097), dict(GH=0), dict(GW=8193), dict(Cn=4096, GH=4097, GW=1), dict(shift=-1), dict(shift=7), dict(radius=-1), dict(radius=9),
               dict(period=-1), dict(decay=-1), dict(decay=31), dict(work_bytes=279)):
        assert add(**kw) == MCG_ERR_ARG, kw
    torch.cuda.synchronize()
    assert torch.equal(heat, keep) and peak.tolist() == [-3, -3] and (work == -5).all()
    assert add() == 0                                             # ... and as documented it runs
    want = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, keep.cpu().numpy(), cell_shift=3, radius=2, kinds=6)
    assert np.array_equal(heat.cpu().numpy(), want[0]) and np.array_equal(peak.cpu().numpy(), want[1])

    views, bufs = HC.device_frames('bgr', 255, DEV)
    table = np.zeros(4, dtype=P._IMAGE)
    for k, v in enumerate(views):
        table[k] = (v.data_ptr(), v.shape[0], v.shape[1], v.stride(0))
    images, lut = dev(table.view(np.uint8)), dev(R.HEAT_LUT.copy())      # (the default ramp is read-only)
    before = [b[0].clone() for b in bufs]

    def draw(images=images, num=4, max_h=37, max_w=300, heat=heat, full=peak, Cn=2, GH=5, GW=7, shift=3, period=2, lut=lut.data_ptr(), min_level=1):
        ptr = lambda t: vp(t.data_ptr() if t is not None else 0)
        return lib.mcg_draw_heat(stream, ptr(images), num, max_h, max_w, ptr(heat), ptr(full), Cn, GH, GW, shift, period, vp(lut), min_level)

    for kw in (dict(images=None), dict(heat=None), dict(full=None), dict(lut=0), dict(lut=lut.data_ptr() + 1), dict(num=0), dict(num=65536), dict(max_h=0),
               dict(max_w=8193), dict(Cn=0), dict(Cn=4097), dict(GH=8193), dict(GW=0), dict(shift=7), dict(period=-1), dict(min_level=0), dict(min_level=256)):
        assert draw(**kw) == MCG_ERR_ARG, kw
    torch.cuda.synchronize()
    assert all(torch.equal(b[0], k) for b, k in zip(bufs, before))
    # a picture larger than (max_h, max_w) is left untouched: max_w = 53 leaves out the 20 x 300 picture
    assert draw(max_w=53) == 0
    torch.cuda.synchronize()
    want = R.draw_heat_host(HC.BGR_FRAMES, heat.cpu().numpy(), peak.cpu().numpy(), 3, period=2)
    buffers_equal(bufs, HC.expected_buffers('bgr', want[:3] + [HC.BGR_FRAMES[3]], 255), 'max_w')


def test_both_calls_are_capturable(pipe):
    """Device tables and device frames, captured once, replayed with new rows in the same buffers: the grid goes on accumulating and the
    frames are drawn over again."""
    cell_shift, grid = 2, (10, 14)
    rs = np.random.RandomState(4)
    rows = [(rs.uniform(-4, 56, (40, 2)).astype(np.float32), rs.randint(0, 4, 40).astype(np.int32), rs.randint(0, 4, 40).astype(np.int32)) for _ in range(3)]
    bufs = [dev(t) for t in rows[0]]
    state = pipe.heat_state(HC.C, (40, 56), cell=4, device=DEV)
    views, fbufs = HC.device_frames('bgr', 255, DEV)

    def call():
        pipe.gaze_heat(*bufs, state, radius=3, period=HC.PERIOD, decay=2, device=DEV)
        pipe.draw_heat(views, state, period=HC.PERIOD, device=DEV)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()                                                    # warm-up outside the capture: the workspace, the ramp and the frame table are kept
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    heat = np.zeros((HC.C,) + grid, np.int32)
    for case in rows:
        for b, t in zip(bufs, case):
            b.copy_(dev(t))
        state.heat.zero_()
        for (buf,), f in zip(fbufs, HC.BGR_FRAMES):
            buf[:, :3 * f.shape[1]] = dev(f.reshape(f.shape[0], -1))
        graph.replay()
        torch.cuda.synchronize()
        heat, peak = A.gaze_heat_host(*case, np.zeros_like(heat), cell_shift=cell_shift, radius=3, period=HC.PERIOD, decay=2)
        assert np.array_equal(state.heat.cpu().numpy(), heat) and np.array_equal(state.peak.cpu().numpy(), peak) and peak.min() > 0
        buffers_equal(fbufs, HC.expected_buffers('bgr', R.draw_heat_host(HC.BGR_FRAMES, heat, peak, cell_shift, period=HC.PERIOD), 255), 'replay')
        # the eager calls give the same
        eager = pipe.heat_state(HC.C, (40, 56), cell=4, device=DEV)
        pipe.gaze_heat(*map(dev, case), eager, radius=3, period=HC.PERIOD, decay=2, device=DEV)
        assert torch.equal(eager.heat, state.heat) and torch.equal(eager.peak, state.peak)
