"""No GPU: the host side of the surface heat map (include/mcgaze_hip.h, "surface heat map") -- attention.surface_charts_host,
attention.surface_heat_host and arrows.draw_surface_heat_host against charts, grids and levels worked by hand and against the scalar
restatements of tests/surface_heat_cases.py, what the map means for one look at a screen, the options of LiveGaze / run_head_video, and the
entries' argument checks (which return before any launch).  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mcgaze_amd import arrows as R
from mcgaze_amd import attention as A
from mcgaze_amd import lib as L
from tests import surface_heat_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCG_ERR_ARG = 1                                                   # enum of include/mcgaze_hip.h
zeros = lambda *shape: np.zeros(shape, dtype=np.int32)
SQUARE = [[(-1, -1, 2), (1, -1, 2), (1, 1, 2), (-1, 1, 2)]]      # 2 m a side at z = 2, clockwise from its top-left corner as the camera sees it
col = A.CHART_INDEX


# ---------------------------------------------------------------- the chart and the accumulation, by hand
def test_a_chart_by_hand():
    c = A.surface_charts_host(SQUARE)
    assert c.shape == (1, 20) and c.dtype == np.float64
    assert c[0, 0:3].tolist() == [-1, -1, 2] and c[0, 3:6].tolist() == [2, 0, 0] and c[0, 6:9].tolist() == [0, 8, 0] and c[0, 9:12].tolist() == [0, 0, 4]
    assert c[0, col['aa']] == 4 and c[0, col['bb']] == 64 and c[0, col['usable']] == 1 and c[0, col['axis']] == 2
    assert (c[0, col['smin']], c[0, col['ws']], c[0, col['rmin']], c[0, col['hr']]) == (0, 1, 0, 0.25)      # s, r of v2 are (1, 0.25)
    fu, fv = A.surface_coords(c, np.array([0]), np.array([[1.0, 1.0, 2.0]]), 1, 1)
    assert (fu[0], fv[0]) == (1.0, 1.0)
    heat, peak = A.surface_heat_host([[0.5, -0.5, 2]], [2], [0], SQUARE, zeros(1, 4, 4), radius=0)
    assert heat.dtype == np.int32 and peak.dtype == np.int32 and peak.tolist() == [1]
    assert np.argwhere(heat[0]).tolist() == [[1, 3]]             # cell (ix, iy) = (3, 1)
    assert np.array_equal(A.surface_extent(SQUARE), [[2.0, 2.0]])
    assert np.array_equal(A.surface_extent([[(0, 0, 1), (3, 0, 1), (3, 0, 5), (0, 0, 5)]]), [[3.0, 4.0]])


def test_a_radius_1_splat_at_a_corner_decay_and_saturation_by_hand():
    heat, peak = A.surface_heat_host([[-1, -1, 2]], [2], [0], SQUARE, zeros(1, 3, 4), radius=1)      # the first vertex: cell (0, 0)
    assert heat.tolist() == [[[4, 2, 0, 0], [2, 1, 0, 0], [0, 0, 0, 0]]] and peak.tolist() == [4]
    heat, _ = A.surface_heat_host([[1, 1, 2]], [2], [0], SQUARE, zeros(1, 3, 4), radius=1)           # the far corner: cell (4, 3), off the grid
    assert heat.tolist() == [[[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]]
    before = np.array([[[100, 7, -7, 2 ** 31 - 5]]], dtype=np.int32)
    heat, peak = A.surface_heat_host([[-0.9, 0, 2]], [2], [0], SQUARE, before, radius=0, decay=2)
    assert heat.tolist() == [[[76, 6, 0, 2 ** 31 - 5 - ((2 ** 31 - 5) >> 2)]]]
    heat, peak = A.surface_heat_host([[0.9, 0, 2]] * 9, [2] * 9, [0] * 9, SQUARE, before, radius=0)
    assert heat.tolist() == [[[100, 7, 0, 2 ** 31 - 1]]] and peak.tolist() == [2 ** 31 - 1]
    assert before.tolist() == [[[100, 7, -7, 2 ** 31 - 5]]]       # the grid given is not changed
    heat, peak = A.surface_heat_host(np.zeros((0, 3)), [], [], SQUARE, before, decay=1)             # no rows: it still decays
    assert heat.tolist() == [[[50, 4, 0, 2 ** 31 - 5 - ((2 ** 31 - 5) >> 1)]]] and peak.tolist() == [heat.max()]


def test_which_rows_count_and_the_flipped_winding():
    kw = dict(flags=SC.FLAGS, mask=SC.MASK, radius=0)
    heat, peak = A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, zeros(SC.M, 4, 4), **kw)
    # rows 2 .. 6 of the square have their cell off the grid at radius 0: rows 0, 1 and 4 remain
    assert heat[0].sum() == 3 and heat[0, 1, 2] == 2 and heat[0, 0, 0] == 1
    assert heat[[1, 2, 3, 4, 5, 10, 11]].reshape(7, -1).sum(axis=1).tolist() == [1] * 7 and not heat[[6, 7, 8, 9, 12, 13]].any()
    assert peak.tolist() == heat.reshape(SC.M, -1).max(axis=1).tolist()
    # the same look at the same screen listed the other way round lands in the vertically mirrored cell ... of the transposed chart:
    # clockwise a = +x and b = +y; counter-clockwise a = +y and b = N x a = +x with N reversed -> fu runs DOWN the screen's left edge
    cw, _ = A.surface_heat_host([[-0.6, -0.6, 2]], [2], [0], SC.TABLES, zeros(SC.M, 4, 4), radius=0)
    assert np.argwhere(cw[0]).tolist() == [[0, 2]] and np.argwhere(heat[1]).tolist() == [[2, 0]]
    # a quadrilateral listed from the same corner along the same first edge, but wound the other way, flips the map vertically
    up = [[(-1, 1, 2), (1, 1, 2), (1, -1, 2), (-1, -1, 2)]]      # starts bottom-left, first edge to the right: counter-clockwise
    flipped, _ = A.surface_heat_host([[0.5, -0.3, 2]], [2], [0], up, zeros(1, 4, 4), radius=0)
    upright, _ = A.surface_heat_host([[0.5, -0.3, 2]], [2], [0], SQUARE, zeros(1, 4, 4), radius=0)
    assert np.argwhere(upright[0]).tolist() == [[1, 3]] and np.argwhere(flipped[0]).tolist() == [[2, 3]]      # fv = 1.4 and 4 - 1.4
    # without flags and mask rows 22 and 23 count too
    more, _ = A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, zeros(SC.M, 4, 4), radius=0)
    assert more[0].sum() == 5 and more[0, 1, 2] == 4
    # at radius 1 the hits on and just outside the far edge light the edge cells
    edge, _ = A.surface_heat_host(SC.HIT3D[[2, 5]], [2, 2], [0, 0], SC.TABLES, zeros(SC.M, 4, 4), radius=1)
    assert edge[0, :, 3].tolist() == [1, 2, 1, 0] and edge[0, 0, 0] == 1 and edge.sum() == 5
    # offsets that are contents: regions 2, 4, 5, 7, 8 are not usable, nothing outside the tables is looked at
    bad = A.surface_charts_host(SC.BAD_TABLES)
    assert bad[:, col['usable']].tolist() == [1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 1, 1, 0, 0]


# ---------------------------------------------------------------- against the scalar restatement
def chart_rows(tables):
    rows = []
    for j in range(len(tables.start) - 1):
        c = SC.chart_scalar(tables.xyz, tables.start, j)
        rows.append([0.0] * 20 if c is None else [*c['v0'], *c['a'], *c['b'], *c['N'], c['aa'], c['bb'], c['smin'], c['ws'], c['rmin'], c['hr'], 1.0,
                                                  float(c['axis'])])
    return np.array(rows)


@pytest.mark.parametrize('tables', [SC.TABLES, SC.BAD_TABLES, SC.random_tables(1)[0], SC.random_tables(2, m=9)[0]], ids=['scene', 'offsets', 'random1', 'random2'])
def test_surface_charts_host_equals_the_scalar_restatement(tables):
    got = A.surface_charts_host(tables)
    assert np.array_equal(got.view(np.uint64), chart_rows(tables).view(np.uint64))


@pytest.mark.parametrize('radius', [0, 1, 3])
@pytest.mark.parametrize('grid', SC.GRIDS)
def test_surface_heat_host_equals_the_scalar_restatement_in_any_row_order(grid, radius):
    for tables in (SC.TABLES, SC.BAD_TABLES):
        before = SC.preloaded(grid)
        for decay, flags, mask in ((0, SC.FLAGS, SC.MASK), (3, None, None)):
            want = SC.surface_add_scalar(SC.HIT3D, SC.KIND, SC.TARGET, tables, before, flags, mask, radius, decay)
            for order in (slice(None), slice(None, None, -1)):
                got = A.surface_heat_host(SC.HIT3D[order], SC.KIND[order], SC.TARGET[order], tables, before, flags=None if flags is None else flags[order],
                                          mask=None if mask is None else mask[order], radius=radius, decay=decay)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    tables, _, hit, kind, target, flags, mask = SC.random_tables(5)
    before = SC.preloaded(grid, 6)
    want = SC.surface_add_scalar(hit, kind, target, tables, before, flags, mask, radius, 1)
    got = A.surface_heat_host(hit, kind, target, tables, before, flags=flags, mask=mask, radius=radius, decay=1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].sum() > before.clip(0).sum() // 2


def filled(tables, grid, m):
    heat = (SC.preloaded(grid, m).astype(np.int64) % 1000).astype(np.int32)
    heat[0, 0, 0] = -9                                            # a negative cell is drawn as 0
    return heat


@pytest.mark.parametrize('grid', [(4, 4), (5, 3)])
def test_the_levels_equal_the_scalar_restatement(grid):
    h, w = 24, 36
    for tables, ri, period in ((SC.TABLES, SC.REGION_IMAGE, 0), (SC.BAD_TABLES, SC.REGION_IMAGE, 2), (SC.random_tables(7)[0], SC.random_tables(7)[1], 0)):
        m = len(tables.start) - 1
        heat = filled(tables, grid, m)
        full = np.maximum(heat.reshape(m, -1).max(axis=1), 0)
        charts, xyz = A.surface_charts_host(tables), tables.xyz.astype(np.float64)
        for p in range(4):
            cam = (SC.CAM[p % 2] * [0.6, 0.6, 0.65, 0.65]).astype(np.float32).astype(np.float64)       # the scene in 24 x 36 pixels
            key = p % period if period else p
            with np.errstate(all='ignore'):
                region, t = R.surface_cover(h, w, cam, charts, xyz, tables.start, np.flatnonzero((ri < 0) | (ri == key)))
                level = R.surface_levels(h, w, cam, charts, region, t, heat, full)
            want_region, want_level = SC.surface_levels_scalar(h, w, p, cam, tables, ri, period, heat, full)
            assert np.array_equal(region, want_region) and np.array_equal(level, want_level), (p, period)
            if tables is SC.TABLES:
                assert (region >= 0).sum() > 50 and level.max() > 100


# ---------------------------------------------------------------- render, by hand
HAND = [[(0, 0, 1), (4, 0, 1), (4, 4, 1), (0, 4, 1)]]           # with fx = fy = 16 and cx = cy = 0: fu = px / 16 on a 4 x 4 grid
HAND_CAM = np.array([16.0, 16.0, 0.0, 0.0])


def hand_levels(heat, full, h=70, w=70):
    tables = A.regions_3d(HAND)
    charts = A.surface_charts_host(tables)
    region, t = R.surface_cover(h, w, HAND_CAM, charts, tables.xyz.astype(np.float64), tables.start, [0])
    return region, R.surface_levels(h, w, HAND_CAM, charts, region, t, np.asarray(heat, np.int32), np.asarray(full))


def test_levels_by_hand():
    heat = zeros(1, 4, 4)
    heat[0, 0] = [100, 200, 0, 0]
    region, level = hand_levels(heat, [200])
    assert (region[8, 1:64] == 0).all() and (region[8, 65:] == -1).all() and (region[1:64, 8] == 0).all()
    row = level[8]                                                # py = 8: V = 0, the centre of grid row 0
    assert row[8] == 255 * 100 // 200 == 127 and row[24] == 255  # cell centres: U = 0 and U = 256
    assert row[16] == 255 * 150 // 200 == 191                    # halfway: fx = 128
    assert row[15] == (144 * 100 + 112 * 200) * 255 // (256 * 200) == 183 and row[17] == (112 * 100 + 144 * 200) * 255 // (256 * 200) == 199
    assert row[2] == row[7] == 127                               # left of the first centre: i0 = -1, both cells clamp to cell 0
    assert level[2, 8] == 127 and level[16, 8] == 63             # ... and above it; halfway to the empty row below: 50 / 200
    assert row[40] == 255 * 100 // 200 - 127 == 0 and row[32] == 127      # cell 2 is empty: its centre is 0, halfway to it is 100 / 200
    assert hand_levels(heat, [0])[1][8, 8] == 255                # a scale below 1 is 1
    heat[0, 3, 3] = 2 ** 31 - 1
    assert hand_levels(heat, [2 ** 31 - 1])[1][60, 60] == 255    # the bottom-right border: clamped, no overflow


def test_the_nearest_region_wins_and_the_lower_index_wins_a_tie():
    charts, xyz = A.surface_charts_host(SC.TABLES), SC.XYZ.astype(np.float64)
    cam = SC.CAM[0].astype(np.float64)
    every = np.arange(SC.M)
    on = lambda picture: every[(SC.REGION_IMAGE < 0) | (SC.REGION_IMAGE == picture)]
    region, t = R.surface_cover(37, 53, cam, charts, xyz, SC.START, on(2))
    assert region[18, 26] == 6 and 1.0 < t[18, 26] < 1.2         # the principal point: region 6 at about 1.1 m hides region 7 at 3 m
    assert region[24, 26] == 7 and t[24, 26] == 3.0              # below it only the far one
    region, t = R.surface_cover(37, 53, cam, charts, xyz, SC.START, on(3))
    assert region[20, 30] == 8 and region[10, 38] == 9 and t[20, 30] == t[10, 38] == 2.0       # coplanar: the lower index where both cover
    assert (region == 10).sum() == 0                             # the region behind the lens covers nothing, anywhere


def test_frames_that_come_back_byte_identical():
    frames = [np.random.RandomState(k).randint(0, 256, (37, 53, 3)).astype(np.uint8) for k in range(2)]
    nv12 = [(np.random.RandomState(k).randint(0, 256, (38, 54)).astype(np.uint8), np.random.RandomState(9 + k).randint(0, 256, (19, 54)).astype(np.uint8))
            for k in range(2)]
    heat = np.full((SC.M, 4, 4), 50, np.int32)
    same = lambda got, want: all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))
    nothing = A.regions_3d([SC.REGIONS[k][1] for k in (10, 12, 13)])      # behind the lens (it has a chart, and covers nothing); collinear; a NaN
    for fmt, fr in (('bgr', frames), ('nv12', nv12)):
        out = R.draw_surface_heat_host(fr, heat[:3], 50, SC.CAM, nothing, cam_period=2, pixel_format=fmt)
        assert all(same(o, f) if fmt == 'nv12' else np.array_equal(o, f) for o, f in zip(out, fr))
        # a low grid under a scale of 1000: no level reaches 255
        out = R.draw_surface_heat_host(fr, heat, 1000, SC.CAM, SC.TABLES, cam_period=2, min_level=255, pixel_format=fmt)
        assert all(same(o, f) if fmt == 'nv12' else np.array_equal(o, f) for o, f in zip(out, fr))
        # ... and drawn it is another picture; a camera that is not finite, or beyond the table, leaves its picture alone
        cams = np.array([[40, 40, 26, 18], [np.inf, 40, 26, 18]], np.float32)
        out = R.draw_surface_heat_host(fr + fr[:1], heat, 50, cams, SC.TABLES, pixel_format=fmt)
        first = out[0] if fmt == 'bgr' else out[0][0]
        assert not np.array_equal(first, fr[0] if fmt == 'bgr' else fr[0][0])
        assert all(same(o, f) if fmt == 'nv12' else np.array_equal(o, f) for o, f in zip(out[1:], (fr + fr[:1])[1:]))


def test_what_the_map_means_for_one_look_at_a_screen():
    """One person in front of the lens looks at a screen beside it: gaze_targets_3d_host finds the point, the cell lit at radius 0 is the
    one that holds it, and the pixel at rint(hit) is drawn."""
    cam = [400.0, 400.0, 160.0, 120.0]
    screen = [[(0.2, -0.3, 1.0), (0.5, -0.3, 1.5), (0.5, 0.0, 1.5), (0.2, 0.0, 1.0)]]
    boxes, gaze = [[130.0, 90.0, 190.0, 150.0]], [[-0.33, 0.17, -0.35]]      # the head is at (0, 0, 1.6); D = (-gx, -gy, gz): right, a little up, nearer
    kind, target, t, hit, mutual, flags, hit3d = A.gaze_targets_3d_host(boxes, gaze, [0], cam, regions=screen, frame='camera')
    assert kind.tolist() == [2] and target.tolist() == [0] and flags.tolist() == [0]
    heat, peak = A.surface_heat_host(hit3d, kind, target, screen, zeros(1, 8, 8), flags=flags, radius=0)
    (iy, ix), = np.argwhere(heat[0]).tolist()
    x, y, z = (float(v) for v in hit3d[0])
    along = ((x - 0.2) ** 2 + (z - 1.0) ** 2) ** 0.5 / (0.3 ** 2 + 0.5 ** 2) ** 0.5      # the way along the top edge, in metres over metres
    assert ix == int(along * 8) and iy == int((y + 0.3) / 0.3 * 8) and 0 < ix < 7 and 0 < iy < 7
    frame = np.full((240, 320, 3), 90, np.uint8)
    out = R.draw_surface_heat_host(frame, heat, peak, cam, screen)
    px, py = (int(v) for v in np.rint(hit[0]))
    assert (out[py, px] != 90).any()
    changed = np.argwhere((out != frame).any(axis=2))
    assert len(changed) and abs(changed[:, 0].mean() - py) < 12 and abs(changed[:, 1].mean() - px) < 12     # a radius-0 cell around the look
    region, _ = R.surface_cover(240, 320, np.array(cam), A.surface_charts_host(screen), np.array(screen[0], dtype=np.float64), np.array([0, 4]), [0])
    assert region[py, px] == 0 and set(map(tuple, changed)) <= set(map(tuple, np.argwhere(region == 0)))


# ---------------------------------------------------------------- options
def test_options_are_refused_with_value_errors():
    for bad in (dict(radius=9), dict(radius=-1), dict(decay=31), dict(radius=1.0)):
        with pytest.raises(ValueError):
            A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, zeros(SC.M, 2, 2), **bad)
    with pytest.raises(ValueError):
        A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, zeros(SC.M + 1, 2, 2))
    with pytest.raises(ValueError):
        A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, zeros(SC.M, 1025, 1))
    with pytest.raises(ValueError):
        A.surface_heat_host(SC.HIT3D, SC.KIND[:3], SC.TARGET, SC.TABLES, zeros(SC.M, 2, 2))
    with pytest.raises(ValueError):
        A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, None, zeros(SC.M, 2, 2))
    with pytest.raises(TypeError):
        A.surface_heat_host(SC.HIT3D, SC.KIND.astype(np.float32), SC.TARGET, SC.TABLES, zeros(SC.M, 2, 2))
    with pytest.raises(TypeError):
        A.surface_heat_host(SC.HIT3D, SC.KIND, SC.TARGET, SC.TABLES, np.zeros((SC.M, 2, 2), np.int64))
    frame = np.zeros((4, 4, 3), np.uint8)
    for bad in (dict(min_level=0), dict(min_level=256), dict(cam_period=-1), dict(region_period=-1), dict(region_image=[0]), dict(lut=np.zeros((5, 4), np.uint8))):
        with pytest.raises(ValueError):
            R.draw_surface_heat_host(frame, zeros(SC.M, 2, 2), 1, SC.CAM, SC.TABLES, **bad)
    with pytest.raises(ValueError):
        R.draw_surface_heat_host(frame, zeros(SC.M, 2, 2), [1, 2], SC.CAM, SC.TABLES)


def test_live_gaze_and_run_head_video_check_surface_heat_before_anything_else():
    from mcgaze_amd import harness, live
    three_d = dict(camera=[400.0, 400.0, 160.0, 120.0], regions3d=[SQUARE])      # one list of polygons per camera
    with pytest.raises(ValueError, match='regions3d'):
        live.LiveGaze(None, None, cameras=1, surface_heat=True)
    with pytest.raises(ValueError, match='regions3d'):
        live.LiveGaze(None, None, cameras=1, attention=True, surface_heat=True)
    with pytest.raises(ValueError, match='regions3d'):
        live.LiveGaze(None, None, cameras=1, attention=dict(camera=three_d['camera']), surface_heat=True)
    with pytest.raises(ValueError, match='needs draw'):
        live.LiveGaze(None, None, cameras=1, attention=three_d, surface_heat=dict(draw=True))
    with pytest.raises(ValueError, match='grid'):
        live.LiveGaze(None, None, cameras=1, attention=three_d, surface_heat=dict(grid=(0, 4), draw=False))
    with pytest.raises(ValueError, match='radius'):
        live.LiveGaze(None, None, cameras=1, attention=three_d, surface_heat=dict(radius=9, draw=False))
    with pytest.raises(ValueError, match='regions3d'):
        harness.run_head_video(None, None, [np.zeros((4, 4, 3), np.uint8)], [np.zeros((0, 4), np.float32)], surface_heat=True)
    with pytest.raises(ValueError, match='needs draw'):
        harness.run_head_video(None, None, [np.zeros((4, 4, 3), np.uint8)], [np.zeros((0, 4), np.float32)], surface_heat=dict(draw=True),
                               attention=dict(camera=three_d['camera'], regions3d=SQUARE))


# ---------------------------------------------------------------- the library
def test_abi_line_exports_and_header():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    assert int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) == L.ABI_VERSION == 20
    lib = L.load()
    for name in ('mcg_surface_heat_add', 'mcg_draw_surface_heat', 'mcg_draw_surface_heat_nv12'):
        assert name in L.EXPORTS and re.search(r'\bint %s\(' % name, hdr) and hasattr(lib, name)
    assert 'surface heat map (additions to ABI 20; nothing above changes)' in hdr
    assert int(re.search(r'#define MCG_SURFACE_CHART_BYTES (\d+)', hdr).group(1)) == L.SURFACE_CHART_BYTES == 8 * len(A.CHART_FIELDS)


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """Every call here fails the host-side checks and returns MCG_ERR_ARG: nothing is launched, so no GPU is needed and no pointer is read."""
    lib = L.load()
    vp, p = C.c_void_p, 0x1000                                    # a non-null, aligned address that is never read

    def add(hit=p, kind=p, target=p, n=4, xyz=p, V=8, start=p, M=2, heat=p, peak=p, GH=5, GW=7, radius=1, decay=0, work=p, work_bytes=160 * 2 + 4 * 70):
        return lib.mcg_surface_heat_add(vp(0), vp(hit), vp(kind), vp(target), vp(0), vp(0), n, vp(xyz), V, vp(start), M, vp(heat), vp(peak), GH, GW, radius,
                                        decay, vp(work), work_bytes)

    for kw in (dict(hit=0), dict(kind=0), dict(target=0), dict(heat=0), dict(peak=0), dict(work=0), dict(work=p + 4), dict(xyz=0), dict(start=0), dict(n=-1),
               dict(n=65537), dict(V=-1), dict(V=65537), dict(M=0), dict(M=4097), dict(GH=0), dict(GW=1025), dict(GH=1025),
               dict(M=4096, GH=65, GW=64, work_bytes=1 << 40), dict(radius=-1), dict(radius=9), dict(decay=-1), dict(decay=31), dict(work_bytes=160 * 2 + 4 * 70 - 1)):
        assert add(**kw) == MCG_ERR_ARG, kw
        assert lib.mcg_last_error()

    def draw(entry, images=p, num=4, max_h=37, max_w=53, cam=p, Cn=2, cam_period=2, xyz=p, V=8, start=p, ri=p, M=2, region_period=0, heat=p, full=p, GH=5, GW=7,
             lut=p, min_level=1, work=p, work_bytes=320):
        return entry(vp(0), vp(images), num, max_h, max_w, vp(cam), Cn, cam_period, vp(xyz), V, vp(start), vp(ri), M, region_period, vp(heat), vp(full), GH, GW,
                     vp(lut), min_level, vp(work), work_bytes)

    for entry in (lib.mcg_draw_surface_heat, lib.mcg_draw_surface_heat_nv12):
        for kw in (dict(images=0), dict(cam=0), dict(xyz=0), dict(start=0), dict(ri=0), dict(heat=0), dict(full=0), dict(lut=0), dict(lut=p + 1), dict(work=0),
                   dict(work=p + 4), dict(num=0), dict(num=65536), dict(max_h=0), dict(max_w=8193), dict(Cn=0), dict(Cn=4097), dict(cam_period=-1),
                   dict(region_period=-1), dict(V=65537), dict(M=0), dict(M=4097), dict(GH=1025), dict(GW=0), dict(M=4096, GH=65, GW=64, work_bytes=1 << 40),
                   dict(min_level=0), dict(min_level=256), dict(work_bytes=319)):
            assert draw(entry, **kw) == MCG_ERR_ARG, kw
