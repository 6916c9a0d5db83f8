"""Cases for the gaze targets (include/mcgaze_hip.h, "gaze targets"), shared by tests/test_attention_cpu.py and tests/test_gpu_attention.py:
hand-worked scenes with their expected tables written out, edge cases, random tables in which equal-t ties occur, and ``targets_scalar``, a
second statement of the arithmetic in plain Python floats and loops (no numpy arithmetic) that the numpy twin is compared with bit for bit.

A case is dict(name=, boxes=, gaze=, image_of=, and optionally regions=, region_image=, region_period=, expand=, camera_angle=, expect=);
``args(case)`` gives the keyword arguments of gaze_targets_host.  Gaze convention: the ray's direction is (-gx, -gy); -z is the lens."""
import math
import struct

import numpy as np

OPTION_NAMES = ('regions', 'region_image', 'region_period', 'expand', 'camera_angle')
FIELDS = ('kind', 'target', 't', 'hit', 'mutual', 'flags')
NAN, INF = float('nan'), float('inf')

A = (0, 0, 10, 10)               # centre (5, 5)
B = (100, 0, 110, 10)            # centre (105, 5); grown by 0.25 * 10: [97.5, 112.5] x [-2.5, 12.5]
C = (100, 100, 110, 110)         # centre (105, 105)
RIGHT, LEFT, DOWN, UP, AWAY, LENS = (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1)


def case(name, boxes, gaze, image_of=None, expect=None, **options):
    n = len(boxes)
    c = dict(name=name, boxes=np.asarray(boxes, dtype=np.float32).reshape(n, 4), gaze=np.asarray(gaze, dtype=np.float32).reshape((n, -1) if n else (0, 3)),
             image_of=np.zeros(n, np.int32) if image_of is None else np.asarray(image_of, dtype=np.int32), expect=expect)
    assert not set(options) - set(OPTION_NAMES)
    if 'regions' in options:
        options['regions'] = np.asarray(options['regions'], dtype=np.float32).reshape(-1, 4)
    if 'region_image' in options:
        options['region_image'] = np.asarray(options['region_image'], dtype=np.int32)
    return dict(c, **options)


def args(c):
    return dict(boxes=c['boxes'], gaze=c['gaze'], image_of=c['image_of'], **{k: c[k] for k in OPTION_NAMES if k in c})


def hand_cases():
    """Scenes worked by hand: ``expect`` holds the tables the header's rules give."""
    e = lambda kind, target, t, hit, mutual, flags=None: dict(kind=kind, target=target, t=t, hit=hit, mutual=mutual,
                                                              flags=[0] * len(kind) if flags is None else flags)
    return [
        case('two people facing each other', [A, B], [RIGHT, LEFT],
             expect=e([1, 1], [1, 0], [92.5, 92.5], [[97.5, 5], [12.5, 5]], [1, 1])),
        case('a 3-cycle: nobody mutual', [A, B, C], [RIGHT, DOWN, (1, 1, 0)],
             expect=e([1, 1, 1], [1, 2, 0], [92.5, 92.5, 92.5], [[97.5, 5], [105, 97.5], [12.5, 12.5]], [0, 0, 0])),
        case('A looks at B, B at the camera', [A, B], [RIGHT, LENS],
             expect=e([1, 3], [1, -1], [92.5, 0], [[97.5, 5], [0, 0]], [0, 0])),
        case('the nearer of two heads on one ray', [A, B, (50, 0, 60, 10)], [RIGHT, AWAY, AWAY],
             expect=e([1, 0, 0], [2, -1, -1], [42.5, 0, 0], [[47.5, 5], [0, 0], [0, 0]], [0, 0, 0])),
        case('a target behind the origin', [A, B], [LEFT, AWAY],
             expect=e([0, 0], [-1, -1], [0, 0], [[0, 0], [0, 0]], [0, 0])),
        case('an origin inside a grown box', [A, (4, 0, 14, 10)], [RIGHT, AWAY],
             expect=e([1, 0], [1, -1], [0, 0], [[5, 5], [0, 0]], [0, 0])),
        case('expand 0.25 reaches a box one row lower', [A, (100, 6, 110, 16)], [RIGHT, AWAY],
             expect=e([1, 0], [1, -1], [92.5, 0], [[97.5, 5], [0, 0]], [0, 0])),
        case('expand 0 misses it', [A, (100, 6, 110, 16)], [RIGHT, AWAY], expand=0.0,
             expect=e([0, 0], [-1, -1], [0, 0], [[0, 0], [0, 0]], [0, 0])),
        case('a head and a region at equal t: the head', [A, B], [RIGHT, AWAY], regions=[(97.5, 0, 120, 10)],
             expect=e([1, 0], [1, -1], [92.5, 0], [[97.5, 5], [0, 0]], [0, 0])),
        case('the same region alone is hit', [A], [RIGHT], regions=[(97.5, 0, 120, 10)],
             expect=e([2], [0], [92.5], [[97.5, 5]], [0])),
        case('two regions at equal t: the lower index', [A], [RIGHT], regions=[(50, -5, 70, 20), (50, 0, 60, 10)],
             expect=e([2], [0], [45], [[50, 5]], [0])),
        case('d_x == 0 with o_x inside the slab', [A, (0, 100, 10, 110)], [DOWN, AWAY],
             expect=e([1, 0], [1, -1], [92.5, 0], [[5, 97.5], [0, 0]], [0, 0])),
        case('d_x == 0 with o_x outside the slab', [A, (20, 100, 30, 110)], [DOWN, AWAY],
             expect=e([0, 0], [-1, -1], [0, 0], [[0, 0], [0, 0]], [0, 0])),
        case('gx = -0.0 is gx = +0.0', [A, (0, 100, 10, 110)], [(-0.0, -1, 0), AWAY],
             expect=e([1, 0], [1, -1], [92.5, 0], [[5, 97.5], [0, 0]], [0, 0])),
        case('no in-plane gaze: away is nothing, towards the lens the camera', [A, B], [AWAY, LENS],
             expect=e([0, 3], [-1, -1], [0, 0], [[0, 0], [0, 0]], [0, 0])),
        case('camera_angle None: the lens is nothing', [A, B], [LENS, (0.125, 0, -1)], camera_angle=None,
             expect=e([0, 1], [-1, 0], [0, 740], [[0, 0], [12.5, 5]], [0, 0])),
        case('the same gaze with the default cone', [A, B], [LENS, (0.125, 0, -1)],
             expect=e([3, 3], [-1, -1], [0, 0], [[0, 0], [0, 0]], [0, 0])),
        case('a region of every picture, of one picture, of a camera', [A, A, A, A], [RIGHT] * 4, image_of=[0, 1, 2, 3],
             regions=[(80, 0, 90, 10), (60, 0, 70, 10), (40, 0, 50, 10)], region_image=[-1, 2, 1], region_period=2,
             expect=e([2] * 4, [0, 2, 0, 2], [75, 35, 75, 35], [[80, 5], [40, 5], [80, 5], [40, 5]], [0] * 4)),
        case('region_period 0: region_image is the picture', [A, A, A, A], [RIGHT] * 4, image_of=[0, 1, 2, 3],
             regions=[(80, 0, 90, 10), (60, 0, 70, 10), (40, 0, 50, 10)], region_image=[-1, 2, 1],
             expect=e([2] * 4, [0, 2, 1, 0], [75, 35, 55, 75], [[80, 5], [40, 5], [60, 5], [80, 5]], [0] * 4)),
        case('unusable regions are never hit', [A], [RIGHT], regions=[(NAN, 0, 30, 10), (40, 0, 30, 10), (50, 0, INF, 10), (60, 10, 70, 0), (80, 0, 90, 10)],
             expect=e([2], [4], [75], [[80, 5]], [0])),
        case('unusable rows look at nothing and are not looked at',
             [A, (NAN, 0, 40, 10), B, (30, 0, 20, 10), (50, 0, 60, 10), (50, 0, 60, 10), A, (70, 0, 80, 10), B],
             [RIGHT, RIGHT, LEFT, RIGHT, (INF, 0, 0), RIGHT, RIGHT, RIGHT, LEFT], image_of=[0, 0, 0, 0, 0, -1, 1, 0, 1],
             expect=e([1, 0, 1, 0, 0, 0, 1, 1, 1], [7, -1, 7, -1, -1, -1, 8, 2, 6], [62.5, 0, 22.5, 0, 0, 0, 92.5, 22.5, 92.5],
                      [[67.5, 5], [0, 0], [82.5, 5], [0, 0], [0, 0], [0, 0], [97.5, 5], [97.5, 5], [12.5, 5]], [0, 0, 1, 0, 0, 0, 1, 1, 1],
                      [0, 2, 0, 2, 2, 2, 0, 0, 0])),
        case('n = 1: nobody else', [A], [RIGHT], expect=e([0], [-1], [0], [[0, 0]], [0])),
        case('n = 0', np.zeros((0, 4)), np.zeros((0, 3)), regions=[(0, 0, 1, 1)], expect=e([], [], [], np.zeros((0, 2)), [], [])),
        case('m = 0 given as an empty table', [A, B], [RIGHT, LEFT], regions=np.zeros((0, 4)), region_image=np.zeros(0, np.int32),
             expect=e([1, 1], [1, 0], [92.5, 92.5], [[97.5, 5], [12.5, 5]], [1, 1])),
    ]


def edge_cases():
    """No expected tables: the numpy twin, the scalar restatement and the kernel have to agree."""
    tiny = np.float32(1e-42)                                      # a denormal f32
    return [
        case('a gaze of denormal magnitude', [A, B, C], [(-tiny, 0, 0), (tiny, tiny, 0), (0, 0, -tiny)]),
        case('boxes without area and boxes that coincide', [(5, 5, 5, 5), (5, 5, 5, 5), (20, 5, 20, 5), (0, 0, 40, 40)],
             [RIGHT, LEFT, LEFT, (1, 1, 0.5)], expand=0.0),
        case('a wide row table: gaze [n, 5]', [A, B, C], [(-1, 0, 0, 9, 9), (1, 0, 0, 9, 9), (1, 1, 0, 9, 9)]),
        case('large coordinates and a large expand', [(-3e38, 0, 3e38, 10), B, A], [RIGHT, LEFT, (-1, -1e-3, 0)], expand=1e300),
    ]


def random_case(seed, n, pictures, m, period=0, bad=0.1, stride=3, shuffle=True):
    """Integer-pixel boxes in 256 x 256 pictures and a gaze on a grid of multiples of 1/64, so that equal-t ties occur; a share ``bad`` of
    rows and regions is unusable in one of the ways the header names.  image_of ascending by row, or shuffled so that tiles mix pictures."""
    rng = np.random.default_rng(seed)
    xy, wh = rng.integers(0, 224, (n, 2)), rng.integers(0, 33, (n, 2))
    boxes = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    gaze = (rng.integers(-64, 65, (n, stride)) / 64.0).astype(np.float32)
    lens = rng.random(n) < 0.1                                    # towards the lens: inside the default cone
    gaze[:, 2] = np.where(lens, -1.0, gaze[:, 2] * 0.25)
    gaze[lens, :2] *= np.float32(0.125)
    gaze[rng.random(n) < 0.2, 1] = 0.0                            # axis-aligned rays: exact ties on box edges
    image_of = np.sort(rng.integers(0, pictures, n)).astype(np.int32)
    if shuffle:
        rng.shuffle(image_of)
    for i in np.flatnonzero(rng.random(n) < bad):
        how = rng.integers(0, 5)
        if how == 0:
            boxes[i, rng.integers(0, 4)] = (NAN, INF, -INF)[rng.integers(0, 3)]
        elif how == 1:
            gaze[i, rng.integers(0, 3)] = (NAN, INF)[rng.integers(0, 2)]
        elif how == 2:
            boxes[i, 2] = boxes[i, 0] - 1
        elif how == 3:
            boxes[i, 3] = boxes[i, 1] - 1
        else:
            image_of[i] = -1 - rng.integers(0, 3)
    rxy, rwh = rng.integers(0, 200, (m, 2)), rng.integers(0, 57, (m, 2))
    regions = np.concatenate([rxy, rxy + rwh], axis=1).astype(np.float32)
    region_image = rng.integers(-1, max(period, pictures), m).astype(np.int32)
    for j in np.flatnonzero(rng.random(m) < bad):
        regions[j, rng.integers(0, 4)] = (NAN, INF, -1000.0)[rng.integers(0, 3)] if rng.integers(0, 2) else regions[j, rng.integers(0, 4)]
        if rng.integers(0, 2):
            regions[j, 2] = regions[j, 0] - 1
    return case(f'random seed {seed}: {n} rows in {pictures} pictures, {m} regions, period {period}', boxes, gaze, image_of, regions=regions,
                region_image=region_image, region_period=period)


def all_cases():
    return hand_cases() + edge_cases() + [random_case(1, 40, 3, 6), random_case(2, 60, 4, 9, period=2), random_case(3, 33, 1, 0),
                                          random_case(4, 48, 5, 5, stride=5, shuffle=False)]


# ---------------------------------------------------------------- the arithmetic a second time: plain Python floats, loops, no numpy arithmetic
def f32(x):
    """A Python float rounded once to f32 (round to nearest even; beyond the range: infinity), as a Python float."""
    try:
        return struct.unpack('f', struct.pack('f', x))[0]
    except OverflowError:
        return math.copysign(INF, x)


def slab(o, d, lo, hi):
    """-> the entry t, or None for a miss."""
    near, far = -INF, INF
    for a in (0, 1):
        if d[a] == 0.0:
            if not lo[a] <= o[a] <= hi[a]:
                return None
            continue
        t1, t2 = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
        near, far = max(near, min(t1, t2)), min(far, max(t1, t2))
    if not (near <= far and far >= 0.0):
        return None
    t = near if near > 0.0 else 0.0
    return t if math.isfinite(t) else None


def targets_scalar(boxes, gaze, image_of=None, regions=None, region_image=None, region_period=0, expand=0.25, camera_angle=10.0):
    """The header's rules row by row -> dict of lists (t and hit already rounded to f32)."""
    boxes = [[float(v) for v in row] for row in np.asarray(boxes, dtype=np.float32).reshape(-1, 4).tolist()]
    n = len(boxes)
    gaze = [[float(v) for v in row[:3]] for row in np.asarray(gaze, dtype=np.float32).reshape((n, -1) if n else (0, 3)).tolist()]
    image_of = [0] * n if image_of is None else [int(v) for v in image_of]
    regions = [] if regions is None else [[float(v) for v in row] for row in np.asarray(regions, dtype=np.float32).reshape(-1, 4).tolist()]
    region_image = [-1] * len(regions) if region_image is None else [int(v) for v in region_image]
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
            e = expand * (w if w > h else h)
            t = slab(o, d, (a1 - e, b1 - e), (a2 + e, b2 + e))
            if t is not None and (best is None or t < best[0]):
                best = (t, 1, j)
        for j, r in enumerate(regions):
            ri = region_image[j]
            applies = ri < 0 or (ri == image_of[i] % region_period if region_period > 0 else ri == image_of[i])
            if not applies or not good(r):
                continue
            t = slab(o, d, (r[0], r[1]), (r[2], r[3]))
            if t is not None and (best is None or t < best[0]):
                best = (t, 2, j)
        if best is not None:
            t, out['kind'][i], out['target'][i] = best
            out['t'][i], out['hit'][i] = f32(t), [f32(o[0] + t * d[0]), f32(o[1] + t * d[1])]
    for i in range(n):
        r = out['target'][i]
        out['mutual'][i] = int(out['kind'][i] == 1 and out['kind'][r] == 1 and out['target'][r] == i)
    return out


DTYPES = dict(kind=np.int32, target=np.int32, t=np.float32, hit=np.float32, mutual=np.int32, flags=np.int32)


def as_tables(d):
    """A dict of lists (targets_scalar, an ``expect``) -> the six arrays in the dtypes the kernel writes."""
    n = len(d['kind'])
    return tuple(np.asarray(d[k], dtype=DTYPES[k]).reshape((n, 2) if k == 'hit' else (n,)) for k in FIELDS)


def same_tables(got, want, what):
    """Bit for bit, all six."""
    for name, a, b in zip(FIELDS, got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        same = a.view(np.int32) == b.view(np.int32)
        assert same.all(), (what, name, np.argwhere(~same)[:5].tolist(), a[~same][:5].tolist(), b[~same][:5].tolist())
