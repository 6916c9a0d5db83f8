"""Shared by tests/test_surface_heat_cpu.py and tests/test_gpu_surface_heat.py (a helper, not a test): the scenes of include/mcgaze_hip.h,
"surface heat map", and scalar restatements of its chart, accumulation and render in plain Python floats and ints, written from the
header's text.  Frames are those of tests/heat_cases.py (37 x 53 BGR / 38 x 54 NV12 pictures, one pitch per access path, and a 20 x 300
picture that crosses a tile): four pictures, whose cameras are CAM[p % 2]."""
import math

import numpy as np

from mcgaze_amd.attention import PolyRegions3D

NAN, INF = float('nan'), float('inf')
CAM = np.array([[40.0, 40.0, 26.0, 18.0], [35.5, 38.25, 24.5, 17.75]], dtype=np.float32)       # fx fy cx cy; the second one in halves and quarters
CAM_PERIOD = 2


def _ngon(n, cx, cy, z, r):
    return [(cx + r * math.cos(2 * math.pi * k / n), cy + r * math.sin(2 * math.pi * k / n), z + 0.1 * math.cos(2 * math.pi * k / n)) for k in range(n)]


# (what, vertices, region_image)
REGIONS = [
    ('a square screen facing the lens, clockwise from its top-left corner', [(-1.0, -0.75, 2), (-0.25, -0.75, 2), (-0.25, 0.0, 2), (-1.0, 0.0, 2)], -1),
    ('the same screen listed counter-clockwise', [(-1.0, -0.75, 2), (-1.0, 0.0, 2), (-0.25, 0.0, 2), (-0.25, -0.75, 2)], 1),
    ('an oblique quadrilateral', [(0.1, -0.8, 1.5), (1.2, -0.7, 3.0), (1.1, 0.1, 3.2), (0.15, -0.1, 1.6)], -1),
    ('a triangle', [(-1.2, 0.2, 2.5), (-0.2, 0.3, 2.0), (-0.7, 0.9, 2.2)], 0),
    ('a concave L', [(0.0, 0.2, 2), (0.9, 0.2, 2), (0.9, 0.45, 2), (0.3, 0.45, 2), (0.3, 0.8, 2), (0.0, 0.8, 2)], 0),
    ('a 32-gon, tilted', _ngon(32, 0.6, 0.5, 2.4, 0.35), 1),
    ('the nearer of two overlapping regions', [(-0.3, -0.3, 1.0), (0.2, -0.3, 1.0), (0.2, 0.1, 1.2), (-0.3, 0.1, 1.2)], 2),
    ('the farther of the two', [(-1.0, -0.9, 3.0), (0.9, -0.9, 3.0), (0.9, 0.6, 3.0), (-1.0, 0.6, 3.0)], 2),
    ('two coplanar overlapping regions: the tie, lower index', [(-0.6, -0.2, 2), (0.4, -0.2, 2), (0.4, 0.5, 2), (-0.6, 0.5, 2)], 3),
    ('... and the higher index', [(0.0, -0.5, 2), (0.9, -0.5, 2), (0.9, 0.3, 2), (0.0, 0.3, 2)], 3),
    ('a region behind the lens', [(-0.5, -0.5, -2), (0.5, -0.5, -2), (0.5, 0.5, -2), (-0.5, 0.5, -2)], -1),
    ('a region straddling z = 0: a floor under the lens', [(-0.6, 0.4, -0.5), (0.6, 0.4, -0.5), (0.6, 0.45, 4.0), (-0.6, 0.45, 4.0)], 3),
    ('unusable: collinear', [(0, 0, 2), (1, 0, 2), (2, 0, 2), (3, 1, 2)], -1),
    ('unusable: a NaN vertex', [(-1, -1, 2), (1, -1, NAN), (1, 1, 2), (-1, 1, 2)], -1),
]
XYZ = np.array([v for _, vs, _ in REGIONS for v in vs], dtype=np.float32)
START = np.cumsum([0] + [len(vs) for _, vs, _ in REGIONS]).astype(np.int32)
REGION_IMAGE = np.array([ri for _, _, ri in REGIONS], dtype=np.int32)
TABLES = PolyRegions3D(XYZ, START)
M = len(REGIONS)
UNUSABLE = [12, 13]
# the same vertices under offsets that are contents, not errors: out of order, beyond V, negative, a region of two vertices
BAD_START = START.copy()
BAD_START[2], BAD_START[5], BAD_START[8] = BAD_START[3] + 1, len(XYZ) + 7, -3       # regions 1, 2 / 4, 5 / 7, 8 lose their offsets
BAD_TABLES = PolyRegions3D(XYZ, BAD_START)
# A picture several tiles wide and several tile rows high (tiles are 256 x 16, NV12 256 x 32), for the render's tile lists: regions whose
# vertices are NOT coplanar -- the exact test takes the polygon along the dropped axis on the plane through v0, so what is drawn reaches
# beyond the projected vertices --, squares that sit on the tile borders at x = 256 and 512 and y = 16, 32, 48, and one far to the right.
WIDE_HW = (72, 648)
WIDE_CAM = np.array([[1000.0, 1000.0, 448.0, 348.0]], dtype=np.float32)


def _square(u, v, half, z, cam=(1000.0, 1000.0, 448.0, 348.0)):
    """A square around the point that pixel (u, v) shows at depth z, `half` pixels to each side."""
    x0, x1, y0, y1 = ((u - half - cam[2]) * z / cam[0], (u + half - cam[2]) * z / cam[0], (v - half - cam[3]) * z / cam[1], (v + half - cam[3]) * z / cam[1])
    return [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]


WIDE_REGIONS = [
    REGIONS[2][1],                                              # the oblique quadrilateral: its v3 is about 0.15 m off the plane of v0 v1 v2
    [(-0.40, -0.33, 1.0), (0.1, -0.34, 1.4), (0.12, -0.29, 0.9), (-0.38, -0.28, 1.3), (-0.45, -0.31, 1.6)],      # a pentagon that is nowhere flat
    _square(256, 16, 6, 0.8), _square(512, 32, 6, 0.8), _square(255.5, 48, 3, 0.7), _square(600, 60, 9, 0.9), _square(130, 31.5, 2, 0.6),
]
WIDE_TABLES = PolyRegions3D(np.array([v for r in WIDE_REGIONS for v in r], dtype=np.float32),
                            np.cumsum([0] + [len(r) for r in WIDE_REGIONS]).astype(np.int32))


def beyond_the_vertex_box(region, j, tile_h, cam=WIDE_CAM[0], tables=WIDE_TABLES):
    """How many pixels that show region j (``region``: arrows.surface_cover's map) lie in tiles of 256 x tile_h pixels that the box of j's
    PROJECTED VERTICES, grown by a pixel, does not touch: what a tile list made from the vertices as they are would leave undrawn."""
    v = tables.xyz[tables.start[j]:tables.start[j + 1]].astype(np.float64)
    fx, fy, cx, cy = (float(c) for c in cam)
    pu, pv = fx * (v[:, 0] / v[:, 2]) + cx, fy * (v[:, 1] / v[:, 2]) + cy
    ys, xs = np.nonzero(region == j)
    tx, ty = (xs // 256) * 256, (ys // tile_h) * tile_h
    return int(((pu.max() + 1 < tx) | (pu.min() - 1 > tx + 255) | (pv.max() + 1 < ty) | (pv.min() - 1 > ty + tile_h - 1)).sum())


GRIDS = [(1, 1), (4, 4), (5, 3), (33, 17)]                      # (GW, GH)

# (what, hit3d, kind, target, flag, mask)
ROWS = [
    ('inside the square', (-0.6, -0.4, 2.0), 2, 0, 0, 1),
    ('inside the square again: the same cell on a 4 x 4 grid', (-0.62, -0.41, 2.0), 2, 0, 0, 1),
    ('the far edge of the square: fu == GW', (-0.25, -0.5, 2.0), 2, 0, 0, 1),
    ('the far corner: fu == GW and fv == GH', (-0.25, 0.0, 2.0), 2, 0, 0, 1),
    ('the first vertex: cell (0, 0)', (-1.0, -0.75, 2.0), 2, 0, 0, 1),
    ('outside the chart, within a radius of the edge', (-1.05, -0.8, 2.0), 2, 0, 0, 1),
    ('far outside the chart: |fu| > 16384 on every grid', (1.0e6, 0.0, 2.0), 2, 0, 0, 1),
    ('the counter-clockwise screen: the map is flipped', (-0.6, -0.6, 2.0), 2, 1, 0, 1),
    ('on the oblique quadrilateral', (0.6, -0.4, 2.2), 2, 2, 0, 1),
    ('the triangle', (-0.7, 0.5, 2.25), 2, 3, 0, 1),
    ('the L', (0.15, 0.6, 2.0), 2, 4, 0, 1),
    ('the 32-gon', (0.6, 0.5, 2.4), 2, 5, 0, 1),
    ('the region behind the lens has a chart too', (0.1, 0.1, -2.0), 2, 10, 0, 1),
    ('the floor', (0.0, 0.43, 2.0), 2, 11, 0, 1),
    ('a NaN hit3d', (NAN, 0.0, 2.0), 2, 0, 0, 1),
    ('an infinite hit3d', (0.0, INF, 2.0), 2, 0, 0, 1),
    ('kind 0', (-0.6, -0.4, 2.0), 0, 0, 0, 1),
    ('kind 1: a head, whose target is a row', (-0.6, -0.4, 2.0), 1, 0, 0, 1),
    ('kind 3', (-0.6, -0.4, 2.0), 3, 0, 0, 1),
    ('a target of -1', (-0.6, -0.4, 2.0), 2, -1, 0, 1),
    ('a target of M', (-0.6, -0.4, 2.0), 2, M, 0, 1),
    ('a target of 2^30', (-0.6, -0.4, 2.0), 2, 2 ** 30, 0, 1),
    ('a flagged row', (-0.6, -0.4, 2.0), 2, 0, 2, 1),
    ('a masked row', (-0.6, -0.4, 2.0), 2, 0, 0, 0),
    ('a collinear region', (1.0, 0.0, 2.0), 2, 12, 0, 1),
    ('a region with a NaN vertex', (0.0, 0.0, 2.0), 2, 13, 0, 1),
]
HIT3D = np.array([r[1] for r in ROWS], dtype=np.float32)
KIND = np.array([r[2] for r in ROWS], dtype=np.int32)
TARGET = np.array([r[3] for r in ROWS], dtype=np.int32)
FLAGS = np.array([r[4] for r in ROWS], dtype=np.int32)
MASK = np.array([r[5] for r in ROWS], dtype=np.int32)
COUNTED = list(range(14))                                        # rows 5 and 6 count only where a tap (or the test of |fu|) lets them


def preloaded(grid, m=M):
    """Grids [m, GH, GW] that already hold something: a few hundred, one cell near 2^31 (the next call saturates it), one negative (read as 0)."""
    GW, GH = grid
    heat = np.random.RandomState(3 + GW).randint(0, 400, (m, GH, GW)).astype(np.int32)
    heat[0, GH // 2, GW // 2] = 2 ** 31 - 5
    heat[min(2, m - 1), 0, 0] = -7
    return heat


def random_tables(seed, m=6, n=200, rows_seed=None):
    """Random planar polygons in front of and around the lens and random rows, most of them hits on the regions' planes (rows_seed: other
    rows over the same regions)."""
    rs = np.random.RandomState(seed)
    regions = []
    for _ in range(m):
        c = rs.randint(3, 9)
        centre, ang = rs.uniform([-1, -1, 0.5], [1, 1, 4]), np.sort(rs.uniform(0, 2 * np.pi, c))
        e1, e2 = rs.normal(size=3), rs.normal(size=3)
        regions.append(centre + 0.6 * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2))
    xyz = np.concatenate(regions).astype(np.float32)
    start = np.cumsum([0] + [len(r) for r in regions]).astype(np.int32)
    region_image = rs.randint(-1, 4, m).astype(np.int32)
    rs = rs if rows_seed is None else np.random.RandomState(rows_seed)
    target = rs.randint(-1, m + 1, n).astype(np.int32)
    hit = np.stack([regions[t % m][0] + rs.uniform(-0.2, 1.2) * (regions[t % m][1] - regions[t % m][0]) +
                    rs.uniform(-0.2, 1.2) * (regions[t % m][2] - regions[t % m][0]) for t in target]).astype(np.float32)
    kind = np.where(rs.uniform(size=n) < 0.8, 2, rs.randint(0, 4, n)).astype(np.int32)
    return PolyRegions3D(xyz, start), region_image, hit, kind, target, (rs.uniform(size=n) < 0.1).astype(np.int32) * 2, \
        (rs.uniform(size=n) < 0.9).astype(np.int32)


# ---------------------------------------------------------------- scalar restatements, written from the header's text
def div(a, b):
    """a / b as IEEE does it (Python raises where the divisor is zero)."""
    if b != 0.0 or b != b:
        return a / b
    if a == 0.0 or a != a:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


fin = math.isfinite


def chart_scalar(xyz, start, j):
    """The chart of region j -> None (not usable) or a dict of Python floats and the vertex list."""
    V = len(xyz)
    s, e = int(start[j]), int(start[j + 1])
    if not (0 <= s <= e <= V) or not 3 <= e - s <= 32:
        return None
    v = [[float(x) for x in xyz[k]] for k in range(s, e)]
    if not all(fin(x) for p in v for x in p):
        return None
    v0 = v[0]
    e1, e2 = [v[1][i] - v0[i] for i in range(3)], [v[2][i] - v0[i] for i in range(3)]
    N = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    if N[0] == 0.0 and N[1] == 0.0 and N[2] == 0.0:
        return None
    a = e1
    b = [N[1] * a[2] - N[2] * a[1], N[2] * a[0] - N[0] * a[2], N[0] * a[1] - N[1] * a[0]]
    aa, bb = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    c = dict(v=v, v0=v0, a=a, b=b, N=N, aa=aa, bb=bb)
    lo_s = hi_s = lo_r = hi_r = None
    for k, p in enumerate(v):
        s_, r_ = sr_scalar(c, p)
        if k == 0:
            lo_s = hi_s = s_
            lo_r = hi_r = r_
        else:
            lo_s = s_ if s_ < lo_s else lo_s
            hi_s = s_ if s_ > hi_s else hi_s
            lo_r = r_ if r_ < lo_r else lo_r
            hi_r = r_ if r_ > hi_r else hi_r
    c.update(smin=lo_s, ws=hi_s - lo_s, rmin=lo_r, hr=hi_r - lo_r)
    if not all(fin(c[k]) and c[k] > 0.0 for k in ('aa', 'bb', 'ws', 'hr')):
        return None
    ax, ay, az = abs(N[0]), abs(N[1]), abs(N[2])
    c['axis'] = 0 if ax >= ay and ax >= az else 1 if ay >= az else 2
    return c


def sr_scalar(c, Q):
    w = [Q[i] - c['v0'][i] for i in range(3)]
    return div((w[0] * c['a'][0] + w[1] * c['a'][1]) + w[2] * c['a'][2], c['aa']), div((w[0] * c['b'][0] + w[1] * c['b'][1]) + w[2] * c['b'][2], c['bb'])


def coords_scalar(c, Q, GW, GH):
    s, r = sr_scalar(c, Q)
    return div(s - c['smin'], c['ws']) * float(GW), div(r - c['rmin'], c['hr']) * float(GH)


def surface_add_scalar(hit3d, kind, target, tables, heat, flags, mask, radius, decay):
    m, GH, GW = heat.shape
    charts = [chart_scalar(tables.xyz, tables.start, j) for j in range(m)]
    taps = [[[0] * GW for _ in range(GH)] for _ in range(m)]
    for k in range(len(hit3d)):
        if flags is not None and int(flags[k]) != 0:
            continue
        if mask is not None and int(mask[k]) == 0:
            continue
        j = int(target[k])
        if int(kind[k]) != 2 or not 0 <= j < m or charts[j] is None:
            continue
        Q = [float(x) for x in hit3d[k]]
        if not all(fin(x) for x in Q):
            continue
        fu, fv = coords_scalar(charts[j], Q, GW, GH)
        if not (fin(fu) and fin(fv) and abs(fu) <= 16384 and abs(fv) <= 16384):
            continue
        ix, iy = math.floor(fu), math.floor(fv)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if 0 <= ix + dx < GW and 0 <= iy + dy < GH:
                    taps[j][iy + dy][ix + dx] += (radius + 1 - abs(dx)) * (radius + 1 - abs(dy))
    out = np.zeros_like(heat)
    for j in range(m):
        for y in range(GH):
            for x in range(GW):
                h = max(int(heat[j, y, x]), 0)
                if decay > 0:
                    h -= h >> decay
                out[j, y, x] = min(h + taps[j][y][x], 2 ** 31 - 1)
    return out, out.reshape(m, -1).max(axis=1).astype(np.int32)


def inside_scalar(c, P):
    iu, iv = (1 if c['axis'] == 0 else 0), (1 if c['axis'] == 2 else 2)
    pu, pv = P[iu], P[iv]
    v, inside = c['v'], False
    for e in range(len(v)):
        (au, av), (bu, bv) = (v[e][iu], v[e][iv]), (v[(e + 1) % len(v)][iu], v[(e + 1) % len(v)][iv])
        if (av > pv) != (bv > pv) and pu < au + div((pv - av) * (bu - au), bv - av):
            inside = not inside
    return inside


def surface_level_scalar(px, py, cam, charts, applies, heat, full):
    """-> (the winner or -1, the level) of one pixel."""
    fx, fy, cx, cy = (float(v) for v in cam)
    _, GH, GW = heat.shape
    d = ((px - cx) / fx, (py - cy) / fy, 1.0)
    best, win = INF, -1
    for j in applies:
        c = charts[j]
        if c is None:
            continue
        N, v0 = c['N'], c['v0']
        den = (N[0] * d[0] + N[1] * d[1]) + N[2] * d[2]
        t = div((N[0] * v0[0] + N[1] * v0[1]) + N[2] * v0[2], den)
        if not (den != 0.0 and fin(t) and t > 0.0) or not t < best:
            continue
        if inside_scalar(c, (t * d[0], t * d[1], t)):
            best, win = t, j
    if win < 0:
        return -1, 0
    fu, fv = coords_scalar(charts[win], (best * d[0], best * d[1], best), GW, GH)
    if not (fin(fu) and fin(fv)):
        return win, 0

    def axis(f, cells):
        U = int(min(max(math.floor(f * 256.0), -2 ** 30), 2 ** 30)) - 128
        i0 = U >> 8
        return min(max(i0, 0), cells - 1), min(max(i0 + 1, 0), cells - 1), U - i0 * 256

    x0, x1, wx = axis(fu, GW)
    y0, y1, wy = axis(fv, GH)
    h = lambda y, x: max(int(heat[win, y, x]), 0)
    val = (256 - wx) * (256 - wy) * h(y0, x0) + wx * (256 - wy) * h(y0, x1) + (256 - wx) * wy * h(y1, x0) + wx * wy * h(y1, x1)
    return win, min(255, (val * 255) // (65536 * max(int(full[win]), 1)))


def surface_levels_scalar(h, w, p, cam, tables, region_image, region_period, heat, full):
    """The winner and the level of every pixel of picture p -> (int [h, w], int [h, w])."""
    m = heat.shape[0]
    charts = [chart_scalar(tables.xyz, tables.start, j) for j in range(m)]
    key = p % region_period if region_period else p
    applies = [j for j in range(m) if region_image[j] < 0 or region_image[j] == key]
    out = [[surface_level_scalar(px, py, cam, charts, applies, heat, full) for px in range(w)] for py in range(h)]
    return np.array([[o[0] for o in row] for row in out]), np.array([[o[1] for o in row] for row in out])
