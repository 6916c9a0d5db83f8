"""Cases for the polygonal regions of the gaze targets (include/mcgaze_hip.h, "gaze targets, polygonal regions"), shared by
tests/test_attention_poly_cpu.py and tests/test_gpu_attention_poly.py: scenes worked by hand with every output table written out, regions
that must not be usable, random tables in which equal-t ties occur, and ``targets_poly_scalar``, a second statement of the rules in plain
Python floats and loops (no numpy arithmetic) that the numpy twin is compared with bit for bit.

A case is dict(name=, boxes=, gaze=, image_of=, regions=, and optionally region_image=, region_period=, expand=, camera_angle=, expect=);
``regions`` is the mixed list of attention.region_polygons or an attention.PolyRegions (tables written by hand, garbage included).
``args(case)`` gives the keyword arguments of gaze_targets_host, ``tables(case)`` those of targets_poly_scalar.  Gaze convention: the ray's
direction is (-gx, -gy); -z is the lens.  The coordinates of the hand-worked scenes make every product, difference and quotient exact."""
import math

import numpy as np

from mcgaze_amd import attention as AT
from tests import attention_cases as AC

OPTION_NAMES = ('region_image', 'region_period', 'expand', 'camera_angle')
NAN, INF = AC.NAN, AC.INF
RIGHT, LEFT, DOWN, UP, AWAY = AC.RIGHT, AC.LEFT, AC.DOWN, AC.UP, AC.AWAY
A, B = AC.A, AC.B                                                 # centres (5, 5) and (105, 5); B grown by 0.25 * 10: [97.5, 112.5] x [-2.5, 12.5]


def at(x, y):
    """A head box whose centre is (x, y)."""
    return (x - 1, y - 1, x + 1, y + 1)


QUAD = [(20, 0), (40, 0), (30, 20), (10, 20)]                     # a slanted screen; its bounding rectangle is [10, 40] x [0, 20]
ELL = [(100, 0), (130, 0), (130, 10), (110, 10), (110, 30), (100, 30)]      # an L: arms [100, 130] x [0, 10] and [100, 110] x [0, 30]; the notch is
#                                                                   [110, 130] x [10, 30], inside the bounding rectangle [100, 130] x [0, 30]
TRI = [(10, 0), (20, -10), (20, 10)]                              # its apex (10, 0) is shared by two slanted edges
SQUARE = [(10, 0), (20, 0), (20, 10), (10, 10)]
NEAR = [(30, 0), (40, 0), (40, 10), (30, 10)]                     # from A looking right: t = 25
FAR = [(50, 0), (60, 0), (60, 10), (50, 10)]                      # ... t = 45


def case(name, boxes, gaze, regions, image_of=None, expect=None, **options):
    n = len(boxes)
    assert not set(options) - set(OPTION_NAMES)
    c = dict(name=name, boxes=np.asarray(boxes, dtype=np.float32).reshape(n, 4), gaze=np.asarray(gaze, dtype=np.float32).reshape((n, -1) if n else (0, 3)),
             image_of=np.zeros(n, np.int32) if image_of is None else np.asarray(image_of, dtype=np.int32), regions=regions, expect=expect)
    if 'region_image' in options:
        options['region_image'] = np.asarray(options['region_image'], dtype=np.int32)
    return dict(c, **options)


def args(c):
    return dict(boxes=c['boxes'], gaze=c['gaze'], image_of=c['image_of'], regions=c['regions'], **{k: c[k] for k in OPTION_NAMES if k in c})


def tables(c):
    """The case with its regions as the vertex tables: what the entry takes."""
    r = c['regions'] if isinstance(c['regions'], AT.PolyRegions) else AT.region_polygons(c['regions'])
    return dict(args(c), regions=AT.PolyRegions(np.asarray(r.xy, dtype=np.float32).reshape(-1, 2), np.asarray(r.start, dtype=np.int32)))


def rotations(polygon):
    """The same polygon in both windings and with every vertex as the first."""
    out = []
    for p in (list(polygon), list(polygon)[::-1]):
        out += [p[k:] + p[:k] for k in range(len(p))]
    return out


def e(kind, target, t, hit, mutual, flags=None):
    return dict(kind=kind, target=target, t=t, hit=hit, mutual=mutual, flags=[0] * len(kind) if flags is None else flags)


def hand_cases():
    """Scenes worked by hand: ``expect`` holds the tables the header's rules give."""
    none = e([0], [-1], [0], [[0, 0]], [0])
    table = lambda xy, start: AT.PolyRegions(np.asarray(xy, dtype=np.float32).reshape(-1, 2), np.asarray(start, dtype=np.int32))
    # 33 vertices up the line x = 30 across the ray y = 5: one too many.  32 of them are a polygon without area whose edges (30, 4) -> (30, 5),
    # (30, 5) -> (30, 6) and the closing (30, 15) -> (30, -16) are all crossed at 25 (den = 1, 1, -31; tn = 25, 25, -775)
    zigzag = [(30, -16 + k) for k in range(33)]
    return [
        # o = (0, 15), d = (1, 0).  Edge (10, 20) -> (20, 0): den = -20, tn = -250, sn = -5: crossed at 12.5; edge (40, 0) -> (30, 20): den = 20,
        # tn = 650, sn = 15: crossed at 32.5; the two horizontal edges are parallel.  The bounding rectangle is entered at 10.
        case('a slanted quadrilateral is entered later than its bounding rectangle', [at(0, 15)], [RIGHT], [QUAD],
             expect=e([2], [0], [12.5], [[12.5, 15]], [0])),
        case('... which alone is entered at 10', [at(0, 15)], [RIGHT], [(10, 0, 40, 20)], expect=e([2], [0], [10], [[10, 15]], [0])),
        # o = (16, -2), d = (-1, 1): through (14, 0) .. (10, 4), the corner of the bounding rectangle that the quadrilateral leaves out
        case('a ray through the bounding rectangle that misses the quadrilateral', [at(16, -2)], [(1, -1, 0)], [QUAD], expect=none),
        case('... and does hit the bounding rectangle', [at(16, -2)], [(1, -1, 0)], [(10, 0, 40, 20)], expect=e([2], [0], [2], [[14, 0]], [0])),
        # o = (140, 20), d = (-1, 0): the notch x in (110, 130) is passed, edge (110, 10) -> (110, 30) is crossed at 30, edge (100, 30) -> (100, 0) at 40
        case('an L: a ray through the notch enters the far arm', [at(140, 20)], [LEFT], [ELL], expect=e([2], [0], [30], [[110, 20]], [0])),
        case('an origin inside a polygon: t = 0 and hit = o', [at(105, 20)], [LEFT], [ELL], expect=e([2], [0], [0], [[105, 20]], [0])),
        # o = (120, 20), d = (0, -1): inside the bounding rectangle, outside the L; edge (130, 10) -> (110, 10) is crossed at 10, edge (100, 0) -> (130, 0) at 20
        case('an origin inside the notch is outside', [at(120, 20)], [UP], [ELL], expect=e([2], [0], [10], [[120, 10]], [0])),
        case('... and looking away from both arms sees nothing', [at(120, 20)], [(-1, -1, 0)], [ELL], expect=none),
        # o = (0, 0), d = (1, 0): both edges at the apex are crossed at 10 (sn = 0 on one, sn = den on the other), the far edge at 20
        case('a ray through a shared vertex', [at(0, 0)], [RIGHT], [TRI], expect=e([2], [0], [10], [[10, 0]], [0])),
        # o = (0, 0), d = (1, 0) along the edge (10, 0) -> (20, 0): den = 0, nothing by itself; its neighbours are crossed at their end points, 10 and 20
        case('a ray collinear with an edge', [at(0, 0)], [RIGHT], [SQUARE], expect=e([2], [0], [10], [[10, 0]], [0])),
        case('a polygon behind the origin', [at(0, 0)], [LEFT], [TRI, SQUARE], expect=none),
        # the head B grown by 2.5 is entered at 92.5, and so is the polygon: edge (97.5, 10) -> (97.5, 0) has den = -10, tn = -925
        case('a head and a polygon at equal t: the head', [A, B], [RIGHT, AWAY], [[(97.5, 0), (120, 0), (120, 10), (97.5, 10)]],
             expect=e([1, 0], [1, -1], [92.5, 0], [[97.5, 5], [0, 0]], [0, 0])),
        case('the same polygon alone is hit', [A], [RIGHT], [[(97.5, 0), (120, 0), (120, 10), (97.5, 10)]], expect=e([2], [0], [92.5], [[97.5, 5]], [0])),
        case('a rectangle and a polygon at equal t: the lower index', [A], [RIGHT], [(50, 0, 60, 10), [(50, -5), (70, -5), (70, 20), (50, 20)]],
             expect=e([2], [0], [45], [[50, 5]], [0])),
        case('a polygon and a rectangle at equal t: the lower index', [A], [RIGHT], [[(50, -5), (70, -5), (70, 20), (50, 20)], (50, 0, 60, 10)],
             expect=e([2], [0], [45], [[50, 5]], [0])),
        case('a nearer polygon behind a farther rectangle in the list', [A], [RIGHT], [(50, 0, 60, 10), NEAR], expect=e([2], [1], [25], [[30, 5]], [0])),
        # a point is hit as a rectangle; as a polygon every edge of it is parallel to everything (den = 0): whatever the rules give, and they give nothing
        case('a rectangle without area is hit', [A], [RIGHT], [(50, 5, 50, 5)], expect=e([2], [0], [45], [[50, 5]], [0])),
        case('a polygon without extent is not', [A], [RIGHT], [[(50, 5), (50, 5), (50, 5)]], expect=none),
        case('regions of every picture, of one picture, of a camera', [A, A, A, A], [RIGHT] * 4, [FAR, (40, 0, 45, 10), NEAR], image_of=[0, 1, 2, 3],
             region_image=[-1, 2, 1], region_period=2, expect=e([2] * 4, [0, 2, 0, 2], [45, 25, 45, 25], [[50, 5], [30, 5], [50, 5], [30, 5]], [0] * 4)),
        # ---- regions that must not be usable: each would be hit before FAR (t = 45) if it were
        case('a vertex that is NaN', [A], [RIGHT], [[(30, 0), (40, 0), (40, NAN), (30, 10)], FAR], expect=e([2], [1], [45], [[50, 5]], [0])),
        case('a vertex that is infinite', [A], [RIGHT], [[(30, 0), (INF, 0), (40, 10), (30, 10)], [(30, 0), (40, 0), (40, 10), (30, -INF)], FAR],
             expect=e([2], [2], [45], [[50, 5]], [0])),
        case('two vertices that are an inverted rectangle, or not finite', [A], [RIGHT], [(40, 0, 30, 10), (30, 10, 40, 0), (30, 0, NAN, 10), FAR],
             expect=e([2], [3], [45], [[50, 5]], [0])),
        case('c = 0', [A], [RIGHT], table(FAR, [0, 0, 4]), expect=e([2], [1], [45], [[50, 5]], [0])),
        case('c = 1', [A], [RIGHT], table([(30, 5)] + FAR, [0, 1, 5]), expect=e([2], [1], [45], [[50, 5]], [0])),
        case('c = 33', [A], [RIGHT], table(zigzag + FAR, [0, 33, 37]), expect=e([2], [1], [45], [[50, 5]], [0])),
        case('c = 32 of the same vertices is a polygon', [A], [RIGHT], table(zigzag + FAR, [0, 32, 37]), expect=e([2], [0], [25], [[30, 5]], [0])),
        case('region_start negative', [A], [RIGHT], table(NEAR + FAR, [-1, 4, 8]), expect=e([2], [1], [45], [[50, 5]], [0])),
        case('region_start beyond V', [A], [RIGHT], table(FAR + NEAR, [0, 4, 9]), expect=e([2], [0], [45], [[50, 5]], [0])),
        case('region_start descending', [A], [RIGHT], table(NEAR + FAR, [8, 4, 8]), expect=e([2], [1], [45], [[50, 5]], [0])),
        case('region_start of garbage words: nothing is usable', [A], [RIGHT], table(NEAR + FAR, [7, -3, 100000, 2, -2 ** 31, 2 ** 31 - 1, 0]), expect=none),
        case('V = 0 with regions', [A], [RIGHT], table([], [0, 0, 3]), expect=none),
        case('m = 0', [A, B], [RIGHT, LEFT], table(NEAR, [0]), expect=e([1, 1], [1, 0], [92.5, 92.5], [[97.5, 5], [12.5, 5]], [1, 1])),
        case('n = 0', np.zeros((0, 4)), np.zeros((0, 3)), [NEAR], expect=e([], [], [], np.zeros((0, 2)), [], [])),
    ]


def random_case(seed, n, pictures, m, period=0, bad=0.1, shuffle=True, garbage=0, counts=None):
    """The rows of attention_cases.random_case (integer-pixel boxes, a gaze on a grid of multiples of 1 / 64, a fifth of the rays axis-aligned)
    with m regions of integer vertices: a third rectangles of 2 vertices, a third the same kind of rectangle as 4 vertices in either winding
    (so that equal-t ties between the two forms and with box edges occur), a third polygons of 3 .. 32 vertices around a centre (or of
    ``counts``, cycled).  A share ``bad`` of the regions has a vertex that is not finite; ``garbage`` words of region_start are overwritten."""
    rows = AC.random_case(seed, n, pictures, 0, period=period, bad=bad, shuffle=shuffle)
    rng = np.random.default_rng(1000 + seed)
    regions = []
    for j in range(m):
        x, y, w, h = int(rng.integers(0, 200)), int(rng.integers(0, 200)), int(rng.integers(0, 57)), int(rng.integers(0, 57))
        how = j % 3 if counts is None else 2
        if how == 0:
            r = [x, y, x + w, y + h]
        elif how == 1:
            r = [[x, y], [x + w, y], [x + w, y + h], [x, y + h]][::1 if rng.integers(0, 2) else -1]
        else:
            c = int(rng.integers(3, AT.POLY_VERTS + 1)) if counts is None else counts[j % len(counts)]
            angle = np.sort(rng.random(c)) * 2 * math.pi
            radius = rng.integers(4, 40, c)
            r = np.stack([np.rint(x + radius * np.cos(angle)), np.rint(y + radius * np.sin(angle))], axis=1).tolist()
        if rng.random() < bad:
            r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
            r[rng.integers(0, len(r)), rng.integers(0, 2)] = (NAN, INF, -INF)[rng.integers(0, 3)]
            r = r.reshape(-1).tolist() if how == 0 else r.tolist()
        regions.append(r)
    xy, start = AT.region_polygons(regions)
    for _ in range(garbage):
        start[rng.integers(0, len(start))] = rng.integers(-5, len(xy) + 40)
    region_image = rng.integers(-1, max(period, pictures), m).astype(np.int32)
    return case(f'random seed {seed}: {n} rows in {pictures} pictures, {m} regions, period {period}, {garbage} garbage offsets', rows['boxes'], rows['gaze'],
                AT.PolyRegions(xy, start), image_of=rows['image_of'], region_image=region_image, region_period=period)


def all_cases():
    return hand_cases() + [random_case(1, 300, 3, 12), random_case(2, 260, 4, 30, period=2), random_case(3, 200, 5, 24, shuffle=False, garbage=4),
                           random_case(4, 200, 2, 16, counts=(3, 4, 31, 32))]


def rectangle_cases():
    """Every case of tests/attention_cases.py -> (its arguments in today's form, the same with every region as 2 vertices)."""
    out = []
    for c in AC.all_cases():
        a = AC.args(c)
        r = np.asarray(a.get('regions', np.zeros((0, 4), np.float32)), dtype=np.float32).reshape(-1, 4)
        out.append((c['name'], a, dict(a, regions=AT.PolyRegions(r.reshape(-1, 2), 2 * np.arange(len(r) + 1, dtype=np.int32)))))
    return out


# ---------------------------------------------------------------- the rules a second time: plain Python floats, loops, no numpy arithmetic
def polygon(o, d, v):
    """INSIDE, then CROSSINGS -> the entry t, or None for a miss."""
    inside, best = False, None
    for k in range(len(v)):
        (ax, ay), (bx, by) = v[k], v[(k + 1) % len(v)]
        if (ay > o[1]) != (by > o[1]) and o[0] < ax + ((o[1] - ay) * (bx - ax)) / (by - ay):
            inside = not inside
        ex, ey, wx, wy = bx - ax, by - ay, ax - o[0], ay - o[1]
        den, tn, sn = d[0] * ey - d[1] * ex, wx * ey - wy * ex, wx * d[1] - wy * d[0]
        if (den > 0.0 and tn >= 0.0 and 0.0 <= sn <= den) or (den < 0.0 and tn <= 0.0 and den <= sn <= 0.0):
            q = tn / den                                          # (den is not zero here; an infinite operand gives inf or nan, never an exception)
            t = q if q > 0.0 else 0.0
            if math.isfinite(t) and (best is None or t < best):
                best = t
    return 0.0 if inside else best


def usable_region(xy, start, j):
    """-> the region's vertices, or None."""
    s, e_ = start[j], start[j + 1]
    if not 0 <= s <= e_ <= len(xy):
        return None
    v = xy[s:e_]
    if not (len(v) == 2 or 3 <= len(v) <= 32) or not all(math.isfinite(x) and math.isfinite(y) for x, y in v):
        return None
    if len(v) == 2 and (v[1][0] < v[0][0] or v[1][1] < v[0][1]):
        return None
    return v


def targets_poly_scalar(boxes, gaze, image_of=None, regions=None, region_image=None, region_period=0, expand=0.25, camera_angle=10.0):
    """The header's rules row by row over the vertex tables ``regions`` = PolyRegions(xy, start) -> dict of lists (t and hit already rounded to
    f32).  Rows, the camera, the ray, the heads and the choice are those of attention_cases.targets_scalar."""
    boxes = [[float(v) for v in row] for row in np.asarray(boxes, dtype=np.float32).reshape(-1, 4).tolist()]
    n = len(boxes)
    gaze = [[float(v) for v in row[:3]] for row in np.asarray(gaze, dtype=np.float32).reshape((n, -1) if n else (0, 3)).tolist()]
    image_of = [0] * n if image_of is None else [int(v) for v in image_of]
    xy = [(float(x), float(y)) for x, y in np.asarray(regions.xy, dtype=np.float32).reshape(-1, 2).tolist()]
    start = [int(v) for v in regions.start]
    m = len(start) - 1
    polys = [usable_region(xy, start, j) for j in range(m)]
    region_image = [-1] * m if region_image is None else [int(v) for v in region_image]
    cos2 = 2.0 if camera_angle is None else math.cos(math.radians(camera_angle)) ** 2
    good = lambda b: all(math.isfinite(v) for v in b) and not b[2] < b[0] and not b[3] < b[1]
    usable = [good(boxes[i]) and all(math.isfinite(v) for v in gaze[i]) and image_of[i] >= 0 for i in range(n)]
    out = dict(kind=[0] * n, target=[-1] * n, t=[0.0] * n, hit=[[0.0, 0.0] for _ in range(n)], mutual=[0] * n, flags=[0 if u else 2 for u in usable])
    for i in range(n):
        if not usable[i]:
            continue
        (x1, y1, x2, y2), (gx, gy, gz) = boxes[i], gaze[i]
        if gz < 0.0 and gz * gz >= cos2 * ((gx * gx + gy * gy) + gz * gz):
            out['kind'][i] = 3
            continue
        o, d = ((x1 + x2) * 0.5, (y1 + y2) * 0.5), (-gx, -gy)
        if d[0] == 0.0 and d[1] == 0.0:
            continue
        best = None                                               # (t, kind, index)
        for j in range(n):
            if j == i or not usable[j] or image_of[j] != image_of[i]:
                continue
            a1, b1, a2, b2 = boxes[j]
            w, h = a2 - a1, b2 - b1
            g = expand * (w if w > h else h)
            t = AC.slab(o, d, (a1 - g, b1 - g), (a2 + g, b2 + g))
            if t is not None and (best is None or t < best[0]):
                best = (t, 1, j)
        for j, v in enumerate(polys):
            ri = region_image[j]
            applies = ri < 0 or (ri == image_of[i] % region_period if region_period > 0 else ri == image_of[i])
            if not applies or v is None:
                continue
            t = AC.slab(o, d, v[0], v[1]) if len(v) == 2 else polygon(o, d, v)
            if t is not None and (best is None or t < best[0]):
                best = (t, 2, j)
        if best is not None:
            t, out['kind'][i], out['target'][i] = best
            out['t'][i], out['hit'][i] = AC.f32(t), [AC.f32(o[0] + t * d[0]), AC.f32(o[1] + t * d[1])]
    for i in range(n):
        r = out['target'][i]
        out['mutual'][i] = int(out['kind'][i] == 1 and out['kind'][r] == 1 and out['target'][r] == i)
    return out
