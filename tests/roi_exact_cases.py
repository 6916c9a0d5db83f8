"""Shared by tests/test_roi_exact_cases_cpu.py and tests/test_gpu_roi_exact.py: integer feature pyramids, boxes with dyadic geometry, a
float64 statement of RoIAlign written from the published definition (as tests/roi_align_pins.py: mmcv roi_align_cuda_kernel.cuh v1.4.8 and
single_level_roi_extractor.py:36-55; explicit loops over bin, sample and tap; neither the oracle nor the engine is called), and the
condition under which roi_align_kernel (csrc/roi_align.hip, csrc/roi_sample.hpp) must return that statement BIT FOR BIT.

THE EXACTNESS CONDITION (``check_exactness`` proves it per case by integer arithmetic; a case that fails is rejected, never skipped).
  Features: integers in [-255, 255] -- f32, bf16 and fp16 values.
  Boxes: every corner is stride_l * d with d a multiple of 1/8 level pixel (most are multiples of 1/4; a sample lands exactly on -1 or
  on L at bin 0.5 only from a corner on the 1/8 grid, as in roi_align_pins.EDGE_BOXES); every extent in level pixels is 7 * 2^j,
  j in -2..3, or zero, or the negative of such a value.  Then start = a * ss - 0.5 is exact, bin = (end - start) / 7 = 2^j exactly,
  and the sample coordinate c = start + (2 i + 1) bin / 4 and the weights l, 1 - l are binary fractions with at most 4 fractional
  bits (bin 0.25 puts samples on odd sixteenths), however the compiler contracts the expression: every intermediate is such a fraction
  below 2^12.  w1..w4 have at most 8 fractional bits, every product w * v and the 16-term sum of a bin are multiples of 2^-8 below
  4 * 255, i.e. integers below 2^18 in that unit -- f32 values in any order -- and * 0.25f is exact: outputs are multiples of 2^-10
  (FRAC_BITS), at most 255 in magnitude.
  Level: (x2 - x1) * (y2 - y1) is exact in f32 and, in quarter pixels, either >= (4 B)^2 or <= (4 B - 1)^2 for B = 112, 224, 448:
  sqrt(w h) is exactly on a boundary, above it, or at least a quarter pixel below -- far outside what the rounding of sqrtf, the
  + 1e-6f and log2f can move.  (With extents of 7 * 2^j level pixels sqrt(w h) is 28 * 2^(k/2) px, so "one step below 112" is
  79.2 px: 56 x 112.)
  Result: f32 -- the number itself; bf16 / fp16 -- ONE round-to-nearest-even of it (include/mcgaze_hip.h), ``expected``.

All arrays are built once per process and shared (functools.lru_cache): do not write to them.
"""
import functools
import math

import numpy as np
import torch

from tests import exact_cases as X

FRAC_BITS = 10
STRIDES = (4, 8, 16, 32)
N_FRAMES = 3
STORE_ROWS = 5
FEAT_MAX = 255
PYRAMIDS = {
    'frame': [(16, 24), (8, 12), (4, 6), (2, 3)],     # a real 64 x 96 frame
    'odd': [(16, 24), (9, 13), (5, 7), (3, 2)],       # NOT consistent with any frame: the entry takes h, w, stride per level
}
LEVEL_BOUNDS = (112, 224, 448)
P, S = 7, 2
NS = P * S


# ------------------------------------------------------------------------------------------------ features
@functools.lru_cache(maxsize=None)
def features(pyr, C, rows=N_FRAMES):
    """4 levels of int64 [rows, H, W, C] in [-255, 255]; every frame and level holds different integers."""
    g = np.random.RandomState(7100 + 13 * list(PYRAMIDS).index(pyr) + C + 1000 * rows)
    out = [g.randint(-FEAT_MAX, FEAT_MAX + 1, size=(rows, h, w, C)).astype(np.int64) for h, w in PYRAMIDS[pyr]]
    for f in out:
        f.setflags(write=False)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ boxes (integer geometry -> floats)
def _box(level, y, x):
    """y, x: (corner, extent) in sixteenths of a level pixel -> (x1, y1, x2, y2) in image pixels (exact floats)."""
    s = STRIDES[level]
    return (x[0] * s / 16.0, y[0] * s / 16.0, (x[0] + x[1]) * s / 16.0, (y[0] + y[1]) * s / 16.0)


def _ext(j):
    return 7 * (1 << (j + 4))     # 7 * 2^j level pixels in sixteenths


def _axis_edges(L, j):
    """Corners (sixteenths of a level pixel, even: the 1/8 grid) that put sample 0 / sample 13 of a 7 * 2^j extent on each edge of the
    definition.  c16_i = corner - 8 + q (2 i + 1) with q = bin16 / 4."""
    q = (1 << (j + 4)) // 4
    odd = q & 1                    # bin 0.25: samples sit on odd sixteenths and cannot hit -1 or L; their nearest neighbours then
    out = [('interior', 24)]
    if not odd:
        out += [('at -1', -8 - q), ('at L', 16 * L + 8 - 27 * q)]
    out += [('below -1', -8 - q - (1 if odd else 2)), ('in (-1, 0)', -8 - q + (1 if odd else 2)),
            ('above L', 16 * L + 8 - 27 * q + (1 if odd else 2)), ('in [L-1, L]', 16 * L + 8 - 27 * q - (7 if odd else 8))]
    return out


def _routes_to(level, j, k):
    """Extents 7 * 2^j x 7 * 2^k level pixels: sqrt(w h) / stride = 7 * 2^((j + k) / 2), which is below 28 at level 0, in [14, 28) at
    levels 1 and 2 and at least 14 at level 3."""
    return j + k <= 3 if level == 0 else j + k >= 2 if level == 3 else j + k in (2, 3)


def _partner(level, j):
    """An extent exponent for the other axis that routes the box to ``level``, or None (bin 0.25 exists at level 0 only)."""
    for k in (0, 2 - j, 3 - j, 3):
        if -2 <= k <= 3 and _routes_to(level, j, k):
            return k
    return None


EDGE_BINS = (-2, -1, 1, 3)      # the edges are built at bins 0.25 (level 0 only), 0.5, 2 and 8


@functools.lru_cache(maxsize=None)
def all_boxes(pyr):
    """-> [(tag, level, box)] for the four levels of a pyramid, in a seeded order that spreads every level over every frame."""
    out = []
    for level, (H, W) in enumerate(PYRAMIDS[pyr]):
        for j in range(-2, 4):
            k = _partner(level, j)
            if k is None:
                continue
            # interior boxes at every bin size, mixed extents included (j != k)
            out.append((f'interior bin {2.0 ** j} x {2.0 ** k}', level, _box(level, (24, _ext(j)), (20, _ext(k)))))
            out.append((f'interior bin {2.0 ** k} x {2.0 ** j}', level, _box(level, (28, _ext(k)), (24, _ext(j)))))
            out.append((f'inverted bin -{2.0 ** j} x -{2.0 ** k}', level, _box(level, (24 + _ext(j), -_ext(j)), (20 + _ext(k), -_ext(k)))))
            out.append((f'outside bin {2.0 ** j}', level, _box(level, (-16 * 300, _ext(j)), (-16 * 300, _ext(k)))))
            if j not in EDGE_BINS:
                continue
            for tag, a in _axis_edges(H, j)[1:]:
                out.append((f'y {tag} bin {2.0 ** j}', level, _box(level, (a, _ext(j)), (24, _ext(k)))))
            for tag, a in _axis_edges(W, j)[1:]:
                out.append((f'x {tag} bin {2.0 ** j}', level, _box(level, (24, _ext(k)), (a, _ext(j)))))
        # both axes on an edge at once
        j = 1 if level else 0
        k = _partner(level, j)
        ey, ex = dict(_axis_edges(H, j)), dict(_axis_edges(W, k))
        if 'at -1' in ey and 'at L' in ex:
            out.append(('y at -1, x at L', level, _box(level, (ey['at -1'], _ext(j)), (ex['at L'], _ext(k)))))
            out.append(('y at L, x at -1', level, _box(level, (ey['at L'], _ext(j)), (ex['at -1'], _ext(k)))))
    # zero area routes to level 0 whatever the other extent
    out.append(('zero area: one point', 0, _box(0, (88, 0), (92, 0))))
    out.append(('zero width', 0, _box(0, (24, _ext(1)), (92, 0))))
    out.append(('zero height, wide', 0, _box(0, (88, 0), (24, _ext(3)))))
    # level routing exactly at 112 / 224 / 448 px and one lattice step below (half the area)
    for level in (1, 2, 3):
        for j, k in ((1, 1), (0, 2), (2, 0), (-1, 3)):
            out.append((f'sqrt(w h) = {LEVEL_BOUNDS[level - 1]} px', level, _box(level, (8, _ext(j)), (12, _ext(k)))))
        for j, k in ((1, 2), (2, 1), (0, 3), (3, 0)):
            out.append((f'sqrt(w h) one step below {LEVEL_BOUNDS[level - 1]} px', level - 1, _box(level - 1, (8, _ext(j)), (12, _ext(k)))))
    order = np.random.RandomState(7300 + list(PYRAMIDS).index(pyr)).permutation(len(out))
    return tuple(out[i] for i in order)


def pick(pyr, n, seed):
    """n boxes of ``all_boxes(pyr)``, levels in rotation, seeded."""
    boxes = all_boxes(pyr)
    by_level = [[b for b in boxes if b[1] == l] for l in range(4)]
    rs = np.random.RandomState(seed)
    return tuple(by_level[i % 4][rs.randint(len(by_level[i % 4]))] for i in range(n))


def _frames(boxes, bpf):
    """[(tag, level, box)] -> (float box list [N_FRAMES][bpf][4], tags, levels); padded with an interior box."""
    boxes = list(boxes)
    while len(boxes) < N_FRAMES * bpf:
        boxes.append(('pad', 0, _box(0, (24, _ext(0)), (24, _ext(0)))))
    assert len(boxes) == N_FRAMES * bpf
    grid = [[boxes[n * bpf + p][2] for p in range(bpf)] for n in range(N_FRAMES)]
    return grid, [b[0] for b in boxes], [b[1] for b in boxes]


# ------------------------------------------------------------------------------------------------ the cases
# name: (pyramid, C, boxes_per_frame or None = all boxes, box seed).  C = 8: one 16-bit channel group, 256 bin slots for 49 bins; 1024:
# 256 f32 groups, one bin per pass.
PLAIN_CASES = {
    'frame-all-c8': ('frame', 8, None, 0), 'frame-all-c16': ('frame', 16, None, 0),
    'odd-all-c8': ('odd', 8, None, 0), 'odd-all-c16': ('odd', 16, None, 0),
    'odd-bpf1-c256': ('odd', 256, 1, 11), 'frame-bpf3-c256': ('frame', 256, 3, 12), 'odd-bpf5-c256': ('odd', 256, 5, 13),
    'frame-bpf1-c1024': ('frame', 1024, 1, 14), 'odd-bpf3-c1024': ('odd', 1024, 3, 15), 'frame-bpf5-c1024': ('frame', 1024, 5, 16),
}
INDEXED_TABLES = {'permuted': (4, 0, 2), 'repeated': (1, 1, 1), 'revisit': (0, 4, 0)}
GUARD_TABLE = (1, -1, 5)
INDEXED_CASE = ('odd', 16, 7, 21)        # pyramid, C, boxes_per_frame, seed: a store of STORE_ROWS rows read by N_FRAMES window frames


class Case:
    """One launch: feats (4 int64 arrays), boxes [N][bpf][4] floats, frame_of or None, and the statement's result (``ref`` float64
    [R, 49, C], ``q`` = ref * 2^FRAC_BITS as int64 tensor, ``levels``)."""

    def __init__(self, name, feats, boxes, bpf, tags, frame_of=None, want_levels=None):
        self.name, self.feats, self.boxes, self.bpf, self.tags, self.frame_of = name, feats, boxes, bpf, tags, frame_of
        self.hw = [f.shape[1:3] for f in feats]
        self.C = feats[0].shape[-1]
        self.ref, self.levels = roi_align_ref(feats, boxes, frame_of=frame_of)
        assert want_levels is None or self.levels == want_levels, (name, 'a box does not route to the level it was built for')
        self.q = quantize(self.ref)

    def flat_boxes(self):
        return [b for fr in self.boxes for b in fr]


@functools.lru_cache(maxsize=None)
def plain_case(name):
    pyr, C, bpf, seed = PLAIN_CASES[name]
    boxes = all_boxes(pyr) if bpf is None else pick(pyr, N_FRAMES * bpf, seed)
    bpf = bpf or -(-len(boxes) // N_FRAMES)
    grid, tags, levels = _frames(boxes, bpf)
    return Case(name, features(pyr, C), grid, bpf, tags, want_levels=levels)


@functools.lru_cache(maxsize=None)
def indexed_case(table):
    pyr, C, bpf, seed = INDEXED_CASE
    grid, tags, levels = _frames(pick(pyr, N_FRAMES * bpf, seed), bpf)
    return Case(f'indexed-{table}', features(pyr, C, STORE_ROWS), grid, bpf, tags, frame_of=INDEXED_TABLES[table], want_levels=levels)


NAN, INF = float('nan'), float('inf')
# The kernel's interface for non-finite corners (csrc/roi_sample.hpp): a box whose area is NaN reads level 0, and a sample whose
# coordinate is NaN contributes 0.  A non-finite corner makes start, end or bin non-finite and every sample coordinate of that axis NaN
# (0 * inf, inf - inf), with or without fused multiply-add; a sample counts only if both axes are valid: such a box is 49 x C zeros.
# The oracle has no such guard and is not the reference for these rows.  Two finite boxes stand among them.
NONFINITE_BOXES = [
    ('all NaN', (NAN, NAN, NAN, NAN)), ('x1 NaN', (NAN, 6.0, 34.0, 34.0)), ('y2 NaN', (6.0, 6.0, 34.0, NAN)),
    ('finite control', _box(0, (24, _ext(0)), (20, _ext(0)))),
    ('x2 +inf, zero height: area inf * 0 = NaN', (6.0, 6.0, INF, 6.0)), ('x1 = x2 = +inf: width inf - inf = NaN', (INF, 6.0, INF, 34.0)),
    ('x -inf .. +inf, zero height', (-INF, 10.0, INF, 10.0)), ('y1 -inf, inverted x: area -inf, sqrt NaN', (34.0, -INF, 6.0, 34.0)),
    ('finite control, level 1', _box(1, (8, _ext(1)), (12, _ext(1)))),
]


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    grid = [[b for _, b in NONFINITE_BOXES[3 * n:3 * n + 3]] for n in range(N_FRAMES)]
    return Case('nonfinite', features('odd', 16), grid, 3, [t for t, _ in NONFINITE_BOXES])


# ------------------------------------------------------------------------------------------------ the statement
def level_of(box, mut=None):
    """map_roi_levels: floor(log2(sqrt(w h) / 56 + 1e-6)) clamped to [0, 3]; a NaN scale (NaN or negative area) reads level 0."""
    x1, y1, x2, y2 = box
    area = (x2 - x1) * (y2 - y1)
    if not area >= 0.0:
        return 0
    sc = math.sqrt(area)
    if mut == 'level boundary <= at 112' and sc == 112.0:
        return 0
    v = sc / 56.0 + 1e-6
    t = math.log2(v)
    return 3 if t >= 3 else 0 if t < 0 else int(math.floor(t))


def axis_sample(a1, a2, ss, L, i, mut=None):
    """Sample i (bin i // 2, sample i % 2) of one axis -> (lo, hi, l, valid)."""
    start, end = a1 * ss - 0.5, a2 * ss - 0.5
    bin_ = (end - start) / P
    c = start + (i // S) * bin_ + ((i % S) + 0.5) * bin_ / S
    if c != c:
        return 0, 0, 0.0, False
    if mut == 'c >= L dropped':
        outside = c < -1.0 or c >= L
    elif mut == 'c <= -1 dropped':
        outside = c <= -1.0 or c > L
    else:
        outside = c < -1.0 or c > L
    if outside:
        return 0, 0, 0.0, False
    if mut != 'no clamp at 0':
        c = max(c, 0.0)
    lo = int(c)
    if mut == 'no far-edge collapse':
        hi = lo + 1
    elif mut == 'hi = lo + 1 clamped':
        hi = min(lo + 1, L - 1)
    elif lo >= L - 1:
        lo = hi = L - 1
        c = float(lo)
    else:
        hi = lo + 1
    return lo, hi, c - lo, True


def _tap(F, frame, y, x, C):
    """One tap: C channels; (mutants only) a tap outside the map reads zeros."""
    _, H, W, _ = F.shape
    if not (0 <= y < H and 0 <= x < W):
        return np.zeros(C)
    return F[frame, y, x]


def _tap_stride0(F, frame, y, x, C, hw0):
    """MUTANT: frame stride taken from level 0's size -- the level's buffer addressed flat (wrapped where it leaves the buffer)."""
    rows, H, W, _ = F.shape
    return F.reshape(-1, C)[(frame * hw0 + y * W + x) % (rows * H * W)]


def roi_align_ref(feats, boxes, strides=STRIDES, frame_of=None, mut=None, sample_round=None):
    """The statement.  feats: 4 int64 arrays [rows, H, W, C]; boxes [N][bpf][4]; frame_of: window frame -> row.  -> (float64
    [N bpf, 49, C], levels).  ``mut`` names one mutation (tests/test_roi_exact_cases_cpu.py); sample_round(v) rounds one sample."""
    bpf = len(boxes[0])
    flat = [b for fr in boxes for b in fr]
    C = feats[0].shape[-1]
    out = np.zeros((len(flat), P * P, C))
    as_f64 = [f.astype(np.float64) for f in feats]       # integers up to 255: exact
    levels = []
    for r, box in enumerate(flat):
        level = level_of(box, mut)
        levels.append(level)
        F = as_f64[level]
        rows, H, W, _ = F.shape
        ss = 1.0 / strides[level]
        n = r // (3 if mut == 'boxes_per_frame taken as 3' else bpf)
        frame = n if frame_of is None or mut == 'frame_of ignored' else frame_of[n]
        if mut is None:
            assert 0 <= frame < rows
        frame %= rows
        x1, y1, x2, y2 = box
        ys = [axis_sample(y1, y2, ss, H, i, mut) for i in range(NS)]
        xs = [axis_sample(x1, x2, ss, W, i, mut) for i in range(NS)]
        if mut == 'frame stride of level 0':
            tap = functools.partial(_tap_stride0, F, frame, C=C, hw0=feats[0].shape[1] * feats[0].shape[2])
        else:
            tap = functools.partial(_tap, F, frame, C=C)
        for ph in range(P):
            for pw in range(P):
                acc = np.zeros(C)
                for iy in range(S):
                    yl, yh, ly, yv = ys[ph * S + iy]
                    for ix in range(S):
                        xl, xh, lx, xv = xs[pw * S + ix]
                        if not (yv and xv):
                            continue
                        hy, hx = 1.0 - ly, 1.0 - lx
                        if mut == 'l and 1 - l swapped on x':
                            lx, hx = hx, lx
                        v =hy * hx * tap(yl, xl) + hy * lx * tap(yl, xh) + ly * hx * tap(yh, xl) + ly * lx * tap(yh, xh)
                        acc += sample_round(v) if sample_round else v
                out[r, ph * P + pw] = acc / (S * S)
    return out, levels


def quantize(ref):
    """float64 reference -> int64 tensor in units of 2^-FRAC_BITS; asserts that nothing is lost."""
    q = ref * float(1 << FRAC_BITS)
    assert np.array_equal(q, np.round(q)) and float(np.abs(q).max(initial=0)) < X.LIMIT, 'the reference is not a multiple of 2^-10'
    return torch.from_numpy(q.astype(np.int64))


def expected(q, dtype):
    """The value the kernel must store: the number itself (f32) or ONE round-to-nearest-even of it (exact_cases.expected)."""
    return X.expected(q, dtype, FRAC_BITS)


# ------------------------------------------------------------------------------------------------ the exactness condition
def _exact_int(v, what):
    assert v == v and abs(v) != INF and v == int(v), f'{what}: {v!r} is not an integer'
    return int(v)


def check_exactness(case):
    """Integer-arithmetic proof of the module docstring's condition for every box and level of a case (finite boxes only).  Returns
    (largest number of fractional bits of a sample coordinate, levels)."""
    for f in case.feats:
        assert f.dtype == np.int64 and int(np.abs(f).max()) <= FEAT_MAX, f'{case.name}: features leave [-255, 255]'
    worst, levels = 0, []
    for tag, box in zip(case.tags, case.flat_boxes()):
        what = f'{case.name} / {tag} {box}'
        qx1, qy1, qx2, qy2 = (_exact_int(v * 4.0, what) for v in box)          # quarter pixels
        wq, hq = qx2 - qx1, qy2 - qy1
        area = wq * hq
        assert area >= 0, f'{what}: one inverted axis makes sqrt(w h) NaN'
        assert max(abs(wq), abs(hq)) < 1 << 24 and (area == 0 or (area // (area & -area)) < 1 << 24), f'{what}: w * h is not an f32 value'
        for B in LEVEL_BOUNDS:
            assert area >= (4 * B) ** 2 or area <= (4 * B - 1) ** 2, f'{what}: sqrt(w h) within a quarter pixel below {B}'
        level = sum(area >= (4 * B) ** 2 for B in LEVEL_BOUNDS)
        levels.append(level)
        s = STRIDES[level]
        for (q1, q2), L in (((qy1, qy2), case.hw[level][0]), ((qx1, qx2), case.hw[level][1])):
            assert (4 * q1) % s == 0 and (4 * q2) % s == 0, f'{what}: a corner is not on the 1/16 grid of level {level}'
            a16, e16 = 4 * q1 // s, 4 * (q2 - q1) // s
            assert a16 % 2 == 0, f'{what}: a corner is not a multiple of 1/8 level pixel'
            assert e16 == 0 or abs(e16) in [7 * (1 << (j + 4)) for j in range(-2, 4)], f'{what}: extent {e16 / 16} px is not 7 * 2^j'
            q = e16 // 7                                                         # the bin in sixteenths (floor division is exact here)
            assert q * 7 == e16 and q % 4 == 0
            c16 = [a16 - 8 + (q // 4) * (2 * i + 1) for i in range(NS)]          # every sample coordinate, in sixteenths
            assert max(abs(c) for c in c16) < 1 << 16, f'{what}: a coordinate needs more than 12 + 4 bits'
            worst = max(worst, max(4 - min((c & -c).bit_length() - 1, 4) if c else 0 for c in c16))
    # weights: worst + worst fractional bits; 16 terms of |w v| with sum of w = 4: below 4 * 255 * 2^8 in units of 2^-8
    assert 2 * worst <= 8 and 4 * FEAT_MAX << 8 < X.LIMIT and 2 * worst + 2 <= FRAC_BITS
    return worst, levels


def edge_census(case):
    """Which edges of the definition the case's boxes hit, per level and axis: {(level, axis, kind)}."""
    seen = set()
    for box in case.flat_boxes():
        level = level_of(box)
        s = STRIDES[level]
        for axis, (a1, a2), L in ((0, (box[1], box[3]), case.hw[level][0]), (1, (box[0], box[2]), case.hw[level][1])):
            start = a1 / s - 0.5
            bin_ = (a2 - a1) / s / P
            cs = [start + (2 * i + 1) * bin_ / 4 for i in range(NS)]
            kinds = [('at -1', lambda c: c == -1.0), ('at L', lambda c: c == L), ('below -1', lambda c: -1.5 <= c < -1.0),
                     ('above L', lambda c: L < c <= L + 0.5), ('in (-1, 0)', lambda c: -1.0 < c < 0.0), ('in [L-1, L]', lambda c: L - 1 <= c <= L)]
            seen |= {(level, axis, k) for k, f in kinds if any(f(c) for c in cs)}
            if bin_ == 0:
                seen.add((level, axis, 'zero'))
            if bin_ < 0:
                seen.add((level, axis, 'inverted'))
            if all(c < -1.0 or c > L for c in cs):
                seen.add((level, axis, 'outside'))
    return seen
