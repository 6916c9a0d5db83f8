"""Shared by tests/test_overlay_cpu.py, tests/test_gpu_overlay.py and tests/test_gpu_live_overlay.py (a helper, not a test): frames, rows and
regions for the attention overlay of include/mcgaze_hip.h, "attention overlay", a scalar restatement of it in plain Python ints, and the
unusable-region and flag-row cases.

Frames: those of tests/draw_cases.py (12 x 16, 18 x 22, 2 x 2, 40 x 48) with their device pitches.  The rows are draw_cases' rows with
kind / target / hit / mutual words set by hand: the overlay takes them as table contents, whatever gaze_targets would have found."""
import math

import numpy as np

from mcgaze_amd import arrows as AR
from mcgaze_amd import attention as AT
from tests import draw_cases as D

PALETTE = np.array([(11 + 30 * k, 240 - 25 * k, (70 + 53 * k) % 256) for k in range(7)], dtype=np.uint8)      # seven different B, G, R

# ---------------------------------------------------------------- the main scene: draw_cases' 12 rows over its 4 frames
# regions: a rectangle and a slanted quadrilateral on the 40 x 48 frame, an L for EVERY picture (it reaches past the small ones), a triangle on
# the 12 x 16 frame, a rectangle with fractional corners on the 18 x 22 frame (5.5 and 12.5 round half to even: 6 and 12)
REGIONS = [[4, 4, 40, 30], [[30, 2], [46, 6], [44, 20], [28, 16]], [[2, 22], [20, 22], [20, 30], [10, 30], [10, 38], [2, 38]],
           [[3, 2], [12, 4], [6, 10]], [5.5, 3.5, 15.4, 12.5]]
REGION_IMAGE = np.array([3, 3, -1, 0, 1], dtype=np.int32)
#                 row  0   1   2   3   4   5   6   7   8   9  10  11
KIND = np.array([2, 1, 0, 3, 2, 0, 1, 2, 2, 0, 1, 7], dtype=np.int32)        # 7: a word outside 0 .. 3 is "none"
TARGET = np.array([0, 10, -1, -1, 2, -1, 0, 3, 4, -1, 1, 5], dtype=np.int32)
MUTUAL = np.array([0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0], dtype=np.int32)
HIT = np.array([(10.5, 26.5), (30, 18), (0, 0), (0, 0), (12.4, 33.6), (0, 0), (44, 30), (7, 5), (15.4, 6.5), (0, 0), (20, 10), (3, 3)], dtype=np.float32)


def scene(rows=None, **more):
    """The arguments of draw_attention_host after ``frames`` for the main scene (rows: a subset, in that order)."""
    rows = np.arange(len(D.ROWS)) if rows is None else np.asarray(rows)
    a = dict(boxes=D.BOXES[rows], gaze=D.GAZE[rows], image_of=D.IMAGE_OF[rows], kind=KIND[rows], target=TARGET[rows], hit=HIT[rows], mutual=MUTUAL[rows],
             regions=REGIONS, region_image=REGION_IMAGE, palette=PALETTE)
    a.update(more)
    return a


def frames(fmt):
    return D.BGR_FRAMES if fmt == 'bgr' else D.NV12_FRAMES


def luma(fmt, f):
    return f if fmt == 'bgr' else f[0]


def polygon(rng, c, cx, cy, radius):
    """c vertices around (cx, cy), angles ascending (simple, possibly concave), coordinates with halves among them."""
    ang = np.sort(rng.uniform(0, 2 * math.pi, c))
    rad = rng.uniform(0.4, 1.0, c) * radius
    return (np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1) * 2) / 2).tolist()


def random_case(seed, n, m, shapes=((40, 48),), counts=(2, 3, 4, 8), period=0):
    """n rows and m regions spread over pictures of ``shapes``: boxes inside the picture, random kinds 0 .. 3, targets within m, hits around the
    picture (some outside), one row in eight mutual -> the arguments of draw_attention_host after ``frames``."""
    rng = np.random.default_rng(seed)
    P = len(shapes)
    image_of = rng.integers(0, P, n).astype(np.int32)
    hw = np.asarray(shapes)[image_of] if n else np.zeros((0, 2), int)
    side = rng.uniform(3, 12, n)
    x1, y1 = rng.uniform(-2, hw[:, 1] - 2), rng.uniform(-2, hw[:, 0] - 2)
    boxes = np.stack([x1, y1, x1 + side, y1 + side * rng.uniform(0.6, 1.4, n)], axis=1).astype(np.float32)
    gaze = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    kind = rng.integers(0, 4, n).astype(np.int32)
    target = np.where(kind == 2, rng.integers(0, max(m, 1), n), np.where(kind == 1, rng.integers(0, max(n, 1), n), -1)).astype(np.int32)
    hit = np.stack([rng.uniform(-6, hw[:, 1] + 6), rng.uniform(-6, hw[:, 0] + 6)], axis=1).astype(np.float32)
    mutual = ((rng.integers(0, 8, n) == 0) & (kind == 1)).astype(np.int32)
    regions = []
    for j in range(m):
        c = counts[j % len(counts)]
        h, w = shapes[int(rng.integers(0, P))]
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2, 0.45 * min(h, w) + 2)
        regions.append([round(cx - r * 0.7, 1), round(cy - r * 0.5, 1), round(cx + r * 0.7, 1), round(cy + r * 0.5, 1)] if c == 2 else polygon(rng, c, cx, cy, r))
    keys = max(period, P) if period else P
    region_image = rng.integers(-1, keys, m).astype(np.int32)
    xy, start = AT.region_polygons(regions)
    return dict(boxes=boxes, gaze=gaze, image_of=image_of, kind=kind, target=target, hit=hit, mutual=mutual, regions=AT.PolyRegions(xy, start),
                region_image=region_image, region_period=period, palette=PALETTE)


def blank(fmt, shapes, seed=3):
    """Random frames of ``shapes`` in draw_attention_host's form."""
    rng = np.random.RandomState(seed)
    if fmt == 'bgr':
        return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    return [(rng.randint(0, 256, (h, w)).astype(np.uint8), rng.randint(0, 256, (h // 2, w)).astype(np.uint8)) for h, w in shapes]


# ---------------------------------------------------------------- regions that cannot be used: region_flags 2, no byte changes
def unusable_regions():
    """-> (PolyRegions, region_image, names): region 0 is good; every other one is a documented way of being unusable."""
    good = [[6, 6, 30, 20]]
    xy = [good[0][:2], good[0][2:]]
    start, names = [0, 2], ['good']

    def add(name, verts):
        xy.extend(verts)
        start.append(len(xy))
        names.append(name)

    add('no vertices', [])
    add('one vertex', [(5, 5)])
    add('33 vertices', [(10 + 8 * math.cos(k), 10 + 8 * math.sin(k)) for k in range(33)])
    add('a NaN vertex', [(4, 4), (20, float('nan')), (12, 30)])
    add('an infinite vertex', [(4, 4), (float('inf'), 8), (12, 30)])
    add('a vertex that rounds to 8192', [(4, 4), (8191.5, 8), (12, 30)])
    add('a vertex that rounds to -8192', [(4, 4), (20, -8191.5), (12, 30)])
    add('an inverted rectangle', [(30, 6), (6, 20)])
    add('8191.4 rounds to 8191: usable', [(4, 30), (8191.4, 30), (4, 36)])
    xy, start = np.asarray(xy, dtype=np.float32), np.asarray(start, dtype=np.int32)
    return AT.PolyRegions(xy, start), np.full(len(names), -1, np.int32), names


UNUSABLE_FLAGS = [0, 2, 2, 2, 2, 2, 2, 2, 2, 0]


def garbage_offsets(xy, m, seed=5):
    """Offsets of garbage words: nothing outside xy may be read, whatever they hold."""
    rng = np.random.default_rng(seed)
    words = rng.integers(-2 ** 31, 2 ** 31, m + 1).astype(np.int32)
    words[::3] = rng.integers(-40, len(xy) + 40, len(words[::3]))
    return words


# ---------------------------------------------------------------- flag rows: draw_cases' (a NaN gaze, an infinite box, an index past the table, a
# centre beyond the bound) and hits that drop the sight line only
FLAG_KIND = np.array([2, 1, 2, 1, 2, 1, 2], dtype=np.int32)
FLAG_TARGET = np.array([0, 0, 0, 0, 0, 0, 4], dtype=np.int32)
FLAG_HIT = np.array([(np.nan, 4), (3, 3), (3, 3), (9000, 3), (3, 3), (3, 3), (np.inf, 2)], dtype=np.float32)     # rows 0, 3, 6 are drawable: arrow, no line


def flag_scene(**more):
    a = dict(boxes=D.FLAG_BOXES, gaze=D.FLAG_GAZE, image_of=D.FLAG_IMAGE_OF, kind=FLAG_KIND, target=FLAG_TARGET, hit=FLAG_HIT,
             mutual=np.zeros(len(D.FLAGS), np.int32), regions=REGIONS, region_image=REGION_IMAGE, palette=PALETTE)
    a.update(more)
    return a


# ---------------------------------------------------------------- the overlay once more, pixel by pixel, in plain Python ints
def covers(px, py, a, b, t):
    """The COVERAGE rule of the header for one pixel, in Python ints."""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    dx, dy, qx, qy = bx - ax, by - ay, px - ax, py - ay
    L, u = dx * dx + dy * dy, qx * dx + qy * dy
    if u <= 0:
        return 4 * (qx * qx + qy * qy) <= t * t
    if u >= L:
        return 4 * ((px - bx) ** 2 + (py - by) ** 2) <= t * t
    return 4 * ((qx * qx + qy * qy) * L - u * u) <= t * t * L


def scalar_overlay(fmt, frames_, boxes, gaze, image_of, kind, target, hit, mutual, regions, region_image, region_period=0, palette=PALETTE,
                   line_thickness=2, region_thickness=2, matrix='bt601', **params):
    """draw_attention_host restated: the strokes listed with Python's own round() and comparisons, then every pixel of every picture asked which
    is the highest stroke that covers it.  The arrow plan alone comes from arrows.arrow_segments (tests/test_draw_cpu.py checks it by hand).
    regions: a PolyRegions.  -> (frames, flags, region_flags, region_active) in the twin's form."""
    xy, start = regions
    n, m, P = len(boxes), len(start) - 1, len(frames_)
    pal = np.asarray(palette, dtype=np.uint8)
    if fmt != 'bgr':
        pal = np.stack([AR.bgr_to_yuv(c, matrix) for c in pal]).astype(np.uint8)
    sizes = [luma(fmt, f).shape[:2] for f in frames_]
    seg, t, flags = AR.arrow_segments(boxes, gaze, lowest=0, **params)
    flags = [2 if not 0 <= int(io) < P else int(f) for f, io in zip(flags, image_of)]
    strokes = []                                                  # (segments, thickness, applies(p), colour(p)) in stroke order
    region_flags = []
    active = [[0] * m for _ in range(P)]
    for k in range(n):
        if int(kind[k]) == 2 and 0 <= int(target[k]) < m and 0 <= int(image_of[k]) < P:
            active[int(image_of[k])][int(target[k])] = 1
    for j in range(m):
        s, e = int(start[j]), int(start[j + 1])
        ok = 0 <= s <= e <= len(xy) and (e - s == 2 or 3 <= e - s <= 32)
        v = [(float(x), float(y)) for x, y in xy[s:e]] if ok else []
        ok = ok and all(math.isfinite(c) and abs(round(c)) <= 8191 for q in v for c in q)
        if ok and len(v) == 2:
            ok = not (v[1][0] < v[0][0] or v[1][1] < v[0][1])
        region_flags.append(0 if ok else 2)
        segs = []
        if ok:
            c = [(round(x), round(y)) for x, y in v]              # Python rounds half to even
            if len(c) == 2:
                c = [c[0], (c[1][0], c[0][1]), c[1], (c[0][0], c[1][1])]
            segs = [(c[i], c[(i + 1) % len(c)]) for i in range(len(c))]
        key = int(region_image[j])
        strokes.append((segs if region_thickness else [], region_thickness,
                        (lambda p, key=key: key < 0 or key == p or (region_period > 0 and key == p % region_period)),
                        (lambda p, j=j: pal[6 if active[p][j] else 5])))
    colour = [4 if int(mutual[k]) != 0 else int(kind[k]) if 1 <= int(kind[k]) <= 3 else 0 for k in range(n)]
    for k in range(n):
        hx, hy = float(hit[k][0]), float(hit[k][1])
        ok = flags[k] == 0 and int(kind[k]) in (1, 2) and math.isfinite(hx) and math.isfinite(hy) and abs(round(hx)) <= 8191 and abs(round(hy)) <= 8191
        segs = [((int(seg[k, 0, 0, 0]), int(seg[k, 0, 0, 1])), (round(hx), round(hy)))] if ok and line_thickness else []
        strokes.append((segs, line_thickness, (lambda p, k=k: int(image_of[k]) == p), (lambda p, k=k: pal[colour[k]])))
    for k in range(n):
        segs = [(tuple(int(v) for v in s[0]), tuple(int(v) for v in s[1])) for s in seg[k]] if flags[k] == 0 and params.get('min_thickness', 5) else []
        strokes.append((segs, int(t[k]), (lambda p, k=k: int(image_of[k]) == p), (lambda p, k=k: pal[colour[k]])))
    out = []
    for p, f in enumerate(frames_):
        h, w = sizes[p]
        here = [(i, s) for i, s in enumerate(strokes) if s[0] and s[2](p)]
        win = [[-1] * w for _ in range(h)]
        for py in range(h):
            for px in range(w):
                for i, (segs, th, _, _) in here:
                    if any(covers(px, py, a, b, th) for a, b in segs):
                        win[py][px] = i
        if fmt == 'bgr':
            g = np.array(f)
            for py in range(h):
                for px in range(w):
                    if win[py][px] >= 0:
                        g[py, px] = strokes[win[py][px]][3](p)
            out.append(g)
        else:
            y, uv = np.array(f[0]), np.array(f[1]).reshape(h // 2, w)
            for py in range(h):
                for px in range(w):
                    if win[py][px] >= 0:
                        y[py, px] = strokes[win[py][px]][3](p)[0]
            for cy in range(h // 2):
                for cx in range(w // 2):
                    top = max(win[2 * cy][2 * cx], win[2 * cy][2 * cx + 1], win[2 * cy + 1][2 * cx], win[2 * cy + 1][2 * cx + 1])
                    if top >= 0:
                        uv[cy, 2 * cx:2 * cx + 2] = strokes[top][3](p)[1:]
            out.append((y, uv))
    return out, np.asarray(flags, np.int32), np.asarray(region_flags, np.int32), np.asarray(active, np.int32).reshape(P, m)


def same(fmt, got, want, what=''):
    """Frames in the twin's form, bit for bit."""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if fmt == 'bgr':
            assert g.shape == w.shape and np.array_equal(g, w), (what, k)
        else:
            assert np.array_equal(g[0], w[0]) and np.array_equal(np.asarray(g[1]).reshape(w[1].shape), w[1]), (what, k)
