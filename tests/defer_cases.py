"""Shared by tests/test_defer_cases_cpu.py and tests/test_gpu_defer_blocks.py: the three kernels of the deferred FPN P2 path, each through
its stand-alone entry -- roi_mark_kernel (mcg_roi_mark_blocks), inner_mark_kernel (mcg_inner_mark_blocks) and wino_x3w_blocks_kernel
(mcg_conv3x3_wino_x3_blocks) -- against host statements written here with explicit loops.  Neither the oracle nor the engine is called.

THE FOOTPRINT STATEMENT (``footprint``).  A box on a level of H x W pixels and stride s, in frame f: if roi_exact_cases.level_of(box) is
not the deferred level, nothing; else rows = {lo >> 3, hi >> 3} over the VALID y samples of roi_exact_cases.axis_sample, columns likewise
over x, and the footprint is rows x columns, block id = f * by_n * bx_n + row * bx_n + column.  ``read_pixels`` is the same product in
pixels, {lo, hi} of the valid samples: what RoIAlign addresses (a tap of weight zero included).  The CPU file proves that the block
footprint is exactly the 8 x 8 cover of the read set.

THE BOXES.  Map 'frame' (16 x 24, 2 x 3 blocks, 3 frames): roi_exact_cases.all_boxes('frame') in full -- every validity edge, inverted,
outside, zero-area and level-boundary box of all four levels -- and its NONFINITE_BOXES.  Map 'edge56' (56 x 56, 7 x 7 blocks, 4 frames):
boxes of the same dyadic geometry (corners on the 1/8 grid of a level pixel, extents 7 * 2^j level pixels, so that the kernel's f32 sample
coordinates are the statement's float64 ones, roi_exact_cases.check_exactness) placed at block borders, EDGE56 below; per axis, the other
axis inside one block.  A level-0 box has w * h < 28^2 level pixels, so no box of positive area covers the 56 x 56 map; the box that does
('whole map') has ONE inverted axis: its area is negative, sqrt(w h) NaN, and such a box reads level 0 (roi_sample.hpp's guard).

THE BLOCK CONV.  Integer inputs under exact_cases' condition (check_exactness_wino, F(2,3)); y starts as SENTINEL everywhere; expected =
the int64 statement (exact_cases.conv3x3_ref) on the pixels of the listed blocks, the sentinel everywhere else -- blocks that only the
entries BEYOND the count name included.  ``conv_lists`` builds the lists of a shape; ``unit_order`` restates the kernel's walk.

All arrays are built once per process and shared (functools.lru_cache): do not write to them.
"""
import functools

import numpy as np
import torch

from tests import exact_cases as X
from tests import roi_exact_cases as R

DEFER_LEVEL, DEFER_STRIDE = 0, 4          # the engine defers P2: level 0, stride 4
NS = R.NS


# ------------------------------------------------------------------------------------------------ the footprint statement
def blocks_of(hw):
    return (hw[0] + 7) // 8, (hw[1] + 7) // 8


def axis_samples(a1, a2, L, stride=DEFER_STRIDE, mut=None):
    """The 14 samples of one axis -> [(lo, hi, l, valid)] (roi_exact_cases.axis_sample; ``mut`` is one of ITS validity mutants)."""
    return [R.axis_sample(a1, a2, 1.0 / stride, L, i, mut) for i in range(NS)]


def read_pixels(box, hw, stride=DEFER_STRIDE, level=DEFER_LEVEL):
    """-> (rows, columns): the pixel rows and columns RoIAlign addresses for the box on this level; the read set is their product.  Empty
    when the box is routed to another level or an axis has no valid sample."""
    if R.level_of(box) != level:
        return set(), set()
    x1, y1, x2, y2 = box
    rows, cols = set(), set()
    for lo, hi, _, valid in axis_samples(y1, y2, hw[0], stride):
        if valid:
            rows |= {lo, hi}
    for lo, hi, _, valid in axis_samples(x1, x2, hw[1], stride):
        if valid:
            cols |= {lo, hi}
    if not rows or not cols:
        return set(), set()
    return rows, cols


MUTANTS = ('no hi tap', 'valid: c > -1', 'valid: c < L', 'from the corners', 'dilated by one block', 'frame offset dropped', 'routing dropped')


def _axis_blocks(a1, a2, L, stride, mut):
    if mut == 'from the corners':                     # the pixels the box's own extent covers, clipped to the map
        p1, p2 = sorted((a1 / stride, a2 / stride))
        if not (p2 >= 0 and p1 <= L - 1):             # NaN corners: nothing
            return set()
        return set(range(int(max(p1, 0.0)) >> 3, (int(min(p2, L - 1.0)) >> 3) + 1))
    vmut = {'valid: c > -1': 'c <= -1 dropped', 'valid: c < L': 'c >= L dropped'}.get(mut)
    out = set()
    for lo, hi, _, valid in axis_samples(a1, a2, L, stride, vmut):
        if valid:
            out.add(lo >> 3)
            if mut != 'no hi tap':
                out.add(hi >> 3)
    return out


def footprint(box, frame, hw, stride=DEFER_STRIDE, level=DEFER_LEVEL, mut=None):
    """The statement: the set of block ids roi_mark_kernel must flag for one box.  ``mut`` names one of MUTANTS."""
    assert mut is None or mut in MUTANTS
    if mut != 'routing dropped' and R.level_of(box) != level:
        return set()
    by_n, bx_n = blocks_of(hw)
    x1, y1, x2, y2 = box
    rows, cols = _axis_blocks(y1, y2, hw[0], stride, mut), _axis_blocks(x1, x2, hw[1], stride, mut)
    if mut == 'dilated by one block' and rows and cols:
        rows = {r + d for r in rows for d in (-1, 0, 1) if 0 <= r + d < by_n}
        cols = {c + d for c in cols for d in (-1, 0, 1) if 0 <= c + d < bx_n}
    base = 0 if mut == 'frame offset dropped' else frame * by_n * bx_n
    out = set()
    for r in sorted(rows):
        for c in sorted(cols):
            out.add(base + r * bx_n + c)
    return out


# ------------------------------------------------------------------------------------------------ the boxes
OUTSIDE = R._box(0, (-16 * 300, R._ext(0)), (-16 * 300, R._ext(0)))


def inside(k):
    """(corner, extent) in sixteenths of a level pixel: samples 8 k + 0.25 .. 8 k + 6.75, taps 8 k .. 8 k + 7 -- block k alone."""
    return (128 * k + 8, R._ext(0))


# name: the spec of the axis under test; the other axis lies inside ONE block, another one for every box of a frame, so that no box
# hides what another lists (the GPU test compares the union of a call).  c_i = corner / 16 - 0.5 + (2 i + 1) * 2^j / 4
EDGE56_AXIS = {
    'sample at 7.0':     (12, R._ext(0)),    # samples 0.5 .. 7.0: the last has lo = 7, hi = 8, l = 0 -- block 1 by a tap of weight zero alone
    'sample at 8.0':     (104, R._ext(3)),   # corner 6.5 (block 0), samples 8, 12 .. 56, 60: lo = 8 first -- block 0 is not read; 60 > L is not valid
    'sample in (7, 8)':  (20, R._ext(0)),    # samples 1.0 .. 7.5: lo = 7, hi = 8, l = 0.5
    'one block':         inside(2),
    'three blocks':      (96, R._ext(1)),    # samples 6 .. 19, taps 6 .. 20: blocks 0, 1, 2
    'every block':       (8, R._ext(3)),     # samples 2, 6 .. 54: every block of the axis
    'last pixel':        (788, R._ext(0)),   # samples 49.0 .. 55.5: the last has lo >= L - 1 -> lo = hi = 55
    'lone sample at -1': (-116, R._ext(0)),  # samples -7.5 .. -1.0: only the last is valid; it reads taps 0 (weight 1) and 1 (weight 0)
    'lone sample at L':  (900, R._ext(0)),   # samples 56.0 .. 62.5: only the first is valid, lo = hi = 55
    'just below -1':     (-118, R._ext(0)),  # samples .. -1.125: none valid
    'just above L':      (902, R._ext(0)),   # samples 56.125 ..: none valid
}
EDGE56_FRAMES, EDGE56_BPF = 5, 7


def _e56(y, x):
    return R._box(0, y, x)


def _ya(name, k):
    return (f'y {name}', 0, _e56(EDGE56_AXIS[name], inside(k)))


def _xa(name, k):
    return (f'x {name}', 0, _e56(inside(k), EDGE56_AXIS[name]))


LEVEL1_BOX = ('routed to level 1', 1, R._box(1, (8, R._ext(1)), (12, R._ext(1))))       # 112 x 112 px: in level-0 geometry it would cover blocks 0 .. 3
WHOLE_MAP = ('whole map: y 56 px, x inverted 56 px (negative area reads level 0)', 0, _e56((8, R._ext(3)), (904, -R._ext(3))))   # x samples 54, 50 .. 2
LAST_BLOCK = ('last block of the last frame', 0, _e56(EDGE56_AXIS['last pixel'], EDGE56_AXIS['last pixel']))
_Y7 = ('sample at 7.0', 'sample in (7, 8)', 'sample at 8.0', 'one block', 'three blocks', 'every block', 'last pixel')
EDGE56 = (
    # frame 0: the y situations, box k in block column k
    [_ya(n, k) for k, n in enumerate(_Y7)],
    # frame 1: the x situations, box k in block row k; a level-1 box between two level-0 boxes
    [_xa(n, k) if n != 'one block' else LEVEL1_BOX for k, n in enumerate(('sample at 7.0', 'one block') + _Y7[1:3] + _Y7[4:])],
    # frame 2: a lone valid sample exactly on each validity edge; just beyond the edge: nothing
    [_ya('lone sample at -1', 0), _ya('lone sample at L', 1), _xa('lone sample at -1', 2), _xa('lone sample at L', 3), _ya('just below -1', 4),
     _xa('just below -1', 5), _ya('just above L', 6)],
    # frame 3: every block of a frame by one box; boxes without a footprint
    [WHOLE_MAP, _xa('just above L', 1), ('all NaN', 0, (R.NAN,) * 4), ('outside', 0, OUTSIDE), ('outside', 0, OUTSIDE), ('outside', 0, OUTSIDE),
     ('outside', 0, OUTSIDE)],
    # frame 4: frame 0's 'one block' box again and a point inside its block; two boxes that share blocks (0, 0) and (1, 0); the largest id last
    [_ya('one block', 3), ('zero area: one point', 0, _e56((264, 0), (396, 0))), _ya('sample at 7.0', 0), _ya('sample in (7, 8)', 0),
     ('outside', 0, OUTSIDE), ('all NaN', 0, (R.NAN,) * 4), LAST_BLOCK],
)
# the chain test's boxes: three per frame of a 2-frame map (frame 1's last box reaches the largest id of THAT map)
CHAIN_BOXES = ([_ya('sample at 7.0', 1), _ya('sample at 8.0', 3), _xa('three blocks', 5)], [_xa('sample in (7, 8)', 2), _ya('last pixel', 0), LAST_BLOCK])


class MarkCase:
    """One map and its boxes: hw, frames, bpf, boxes [frames][bpf][4] floats, tags and levels per box row, the pyramid's level sizes."""

    def __init__(self, name, pyramid, grid, tags, levels):
        self.name, self.pyramid, self.boxes, self.tags, self.levels = name, pyramid, grid, tags, levels
        self.hw, self.frames, self.bpf = pyramid[0], len(grid), len(grid[0])
        self.nblk = self.frames * blocks_of(self.hw)[0] * blocks_of(self.hw)[1]
        for tag, level, box in zip(tags, levels, self.flat()):
            assert R.level_of(box) == level, (name, tag, 'a box does not route to the level it was built for')

    def flat(self):
        return [b for fr in self.boxes for b in fr]

    def rows(self):
        """-> [(tag, frame, box)] per box row"""
        return [(self.tags[i], i // self.bpf, b) for i, b in enumerate(self.flat())]

    def footprint(self, mut=None, keep=None):
        """The union over the case's box rows (``keep``: a predicate on the row index)."""
        out = set()
        for i, (_, frame, box) in enumerate(self.rows()):
            if keep is None or keep(i):
                out |= footprint(box, frame, self.hw, mut=mut)
        return out


@functools.lru_cache(maxsize=None)
def mark_case(name):
    if name == 'frame':
        boxes = list(R.all_boxes('frame')) + [(tag, R.level_of(box), box) for tag, box in R.NONFINITE_BOXES]
        grid, tags, levels = R._frames(boxes, -(-len(boxes) // R.N_FRAMES))
        return MarkCase(name, R.PYRAMIDS['frame'], grid, tags, levels)
    assert name == 'edge56' and len(EDGE56) == EDGE56_FRAMES and all(len(fr) == EDGE56_BPF for fr in EDGE56)
    flat = [b for fr in EDGE56 for b in fr]
    return MarkCase(name, [(56, 56), (28, 28), (14, 14), (7, 7)], [[b[2] for b in fr] for fr in EDGE56], [b[0] for b in flat], [b[1] for b in flat])


MARK_CASES = ('frame', 'edge56')


@functools.lru_cache(maxsize=None)
def chain_case():
    flat = [b for fr in CHAIN_BOXES for b in fr]
    return MarkCase('chain', [(56, 56), (28, 28), (14, 14), (7, 7)], [[b[2] for b in fr] for fr in CHAIN_BOXES], [b[0] for b in flat], [b[1] for b in flat])


class _ExactShim:
    """What roi_exact_cases.check_exactness reads of a case."""

    def __init__(self, case, rows):
        self.name, self.hw = case.name, case.pyramid
        self.feats = [np.zeros((1, h, w, 1), dtype=np.int64) for h, w in case.pyramid]
        self.tags, self._boxes = [case.tags[i] for i in rows], [case.flat()[i] for i in rows]

    def flat_boxes(self):
        return self._boxes


def check_box_exactness(case):
    """roi_exact_cases' integer proof that the kernel's f32 sample coordinates are the statement's, for every finite box of positive or
    zero area.  The others are routed before any rounding -- a NaN or infinite corner leaves no valid sample, a negative area is level 0 by
    the NaN guard -- and the latter's coordinates get the same dyadic condition stated directly: corners on the 1/8 grid of a level-0
    pixel, extents +-7 * 2^j.  -> how many boxes went through either."""
    plain, flipped = [], []
    for i, box in enumerate(case.flat()):
        if not all(np.isfinite(box)):
            continue
        x1, y1, x2, y2 = box
        (plain if (x2 - x1) * (y2 - y1) >= 0 else flipped).append(i)
    R.check_exactness(_ExactShim(case, plain))
    for i in flipped:
        q = [v * 4.0 for v in case.flat()[i]]                       # sixteenths of a level-0 pixel
        assert all(v == int(v) and int(v) % 2 == 0 for v in q), (case.tags[i], 'a corner is not on the 1/8 grid')
        for a, b in ((q[1], q[3]), (q[0], q[2])):
            assert abs(int(b - a)) in [7 * (1 << (j + 4)) for j in range(-2, 4)], (case.tags[i], 'extent is not 7 * 2^j')
    return len(plain) + len(flipped)


# ------------------------------------------------------------------------------------------------ the census of edge56
def axis_situations(a1, a2, L):
    """Which of the block-border situations the samples of one axis show -> set of names."""
    s = axis_samples(a1, a2, L)
    valid = [(lo, hi, l) for lo, hi, l, v in s if v]
    out = set()
    if not valid:
        return {'no valid sample'}
    blocks = {lo >> 3 for lo, _, _ in valid} | {hi >> 3 for _, hi, _ in valid}
    without_zero_taps = {lo >> 3 for lo, _, _ in valid} | {hi >> 3 for _, hi, l in valid if l > 0}
    if any(lo % 8 == 7 and hi == lo + 1 and l == 0.0 for lo, hi, l in valid) and blocks != without_zero_taps:
        out.add('sample at 7.0')                # a block listed by a tap of weight zero alone
    first = min(valid)
    if first[0] % 8 == 0 and first[0] > 0 and first[2] == 0.0 and int(min(a1, a2) / DEFER_STRIDE) >> 3 == (first[0] >> 3) - 1:
        out.add('sample at 8.0')                # the lowest sample sits on a block's first pixel; the box's corner lies in the block before
    if any(lo % 8 == 7 and hi == lo + 1 and 0.0 < l < 1.0 for lo, hi, l in valid):
        out.add('sample in (7, 8)')
    if len(blocks) == 1:
        out.add('one block')
    if len(blocks) == 3:
        out.add('three blocks')
    if len(blocks) == (L + 7) // 8:
        out.add('every block')
    if any(lo == hi == L - 1 for lo, hi, _ in valid):
        out.add('last pixel')
    # (that the lone sample is exactly at -1 / at L is what the validity mutants show: (lo, hi, l) is the same for c in [-1, 0] / [L - 1, L])
    if len(valid) == 1 and s[NS - 1][3] and valid[0] == (0, 1, 0.0):
        out.add('lone sample at -1')
    if len(valid) == 1 and s[0][3] and valid[0][:2] == (L - 1, L - 1):
        out.add('lone sample at L')
    return out


# ------------------------------------------------------------------------------------------------ the inner-block rule
def dilate(ids, frames, hw):
    """The blocks whose inner pixels the 3 x 3 convs of the listed output blocks read: a 3 x 3 dilation inside each frame, explicit loops."""
    by_n, bx_n = blocks_of(hw)
    out = set()
    for b in ids:
        f, rem = divmod(b, by_n * bx_n)
        assert 0 <= f < frames
        r, c = divmod(rem, bx_n)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if 0 <= r + dr < by_n and 0 <= c + dc < bx_n:
                    out.add(f * by_n * bx_n + (r + dr) * bx_n + c + dc)
    return out


# (frames, H, W): a one-block frame, a one-row frame, 2 x 3 blocks, 7 x 7 blocks
INNER_MAPS = ((3, 8, 8), (2, 8, 40), (3, 16, 24), (2, 56, 56))


def inner_lists(frames, hw):
    """-> {name: ids} the given output lists of a map: frame corners, the last block of one frame with the first of the next, a seeded set."""
    by_n, bx_n = blocks_of(hw)
    bpf = by_n * bx_n
    corners = sorted({f * bpf + r * bx_n + c for f in range(frames) for r in (0, by_n - 1) for c in (0, bx_n - 1)})
    rs = np.random.RandomState(7700 + 31 * frames + hw[0] + hw[1])
    seeded = sorted(int(v) for v in rs.permutation(frames * bpf)[:max(1, frames * bpf // 5)])
    return {'corners': corners, 'frame seam': [bpf - 1, bpf], 'seeded': seeded, 'first': [0], 'last': [frames * bpf - 1]}


# ------------------------------------------------------------------------------------------------ the block conv
SENTINEL = -7.5            # no possible result: every result is an integer
CONV_DENSITY = 0.5
# (frames, H, W, Cin, Cout)
CONV_SHAPES = (
    (1, 8, 8, 32, 128),        # one block is the whole frame: every halo row and column is padding
    (3, 16, 24, 64, 256),      # two channel tiles
    (2, 48, 48, 32, 256),      # 72 blocks: the unit counts below
    (1, 8, 72, 32, 128),       # wider than the raster tiles' 62 pixels
)
UNIT_COUNTS = (2, 14, 16, 18, 34)                       # units = 2 * ceil(count / 4) at Cout = 256
UNIT_LIST_COUNTS = {2: 3, 14: 27, 16: 32, 18: 33, 34: 66}
GRID_CAPS = (0, 16, 3)


def conv_nblk(shape):
    return shape[0] * (shape[1] // 8) * (shape[2] // 8)


def units_of(count, cout):
    """wino_x3w_blocks_kernel: groups of four blocks x 128-channel tiles."""
    return ((count + 3) >> 2) * (cout // 128)


def unit_order(count, cout):
    """The kernel's walk restated: u in [0, padded) -> the logical unit it runs, or None where logical >= units (a padding slot).
    -> (units, padded, [logical or None per u])."""
    n_tiles = cout // 128
    units = units_of(count, cout)
    padded = (units + 15) & ~15 if n_tiles == 2 else units
    order = []
    for u in range(padded):
        logical = u
        if n_tiles == 2:
            x, j = u & 7, u >> 3
            logical = (j & 1) + 2 * (x + 8 * (j >> 1))
        order.append(logical)
    return units, padded, order


class ConvList:
    """A device list as the entry takes it: ``ids`` (count entries, distinct, in range) and ``buffer`` = ids + the entries beyond the
    count (in-range block ids that the kernel must not compute), so capacity = len(buffer) > count."""

    def __init__(self, name, ids, tail, caps=(0,)):
        self.name, self.ids, self.buffer, self.caps = name, [int(v) for v in ids], [int(v) for v in ids] + [int(v) for v in tail], caps
        assert len(set(self.ids)) == len(self.ids) and len(self.buffer) > len(self.ids)


@functools.lru_cache(maxsize=None)
def conv_lists(shape):
    """The lists of a shape.  Every tail names in-range blocks; where the list leaves blocks out the tail names some of THOSE."""
    frames, H, W, _, cout = shape
    by_n, bx_n = H // 8, W // 8
    bpf, nblk = by_n * bx_n, conv_nblk(shape)
    rs = np.random.RandomState(7800 + 7 * frames + H + 3 * W + cout)

    def tail(ids, n=3):
        rest = [b for b in range(nblk) if b not in set(ids)]
        return (rest + [0] * n)[:n] if rest else [0] * n

    out = [ConvList('count 0', [], tail([], 4))]
    for c in (1, 2, 3, 5):
        if c <= nblk:
            ids = [int(v) for v in rs.permutation(nblk)[:c]]
            out.append(ConvList(f'count {c}', ids, tail(ids)))
    out.append(ConvList('all, raster', range(nblk), tail(range(nblk))))
    out.append(ConvList('all, permuted', rs.permutation(nblk), tail(range(nblk), 5)))
    corners = sorted({f * bpf + r * bx_n + c for f in range(frames) for r in (0, by_n - 1) for c in (0, bx_n - 1)})
    out.append(ConvList('frame corners', corners, tail(corners)))
    if frames >= 2:
        # ONE group of four: the last block of frame 0 and the first of frame 1 side by side, then the same across the next seam or two more blocks
        ids = [bpf - 1, bpf] + ([2 * bpf - 1, 2 * bpf] if frames >= 3 else [0, 2 * bpf - 1])
        out.append(ConvList('frame seam in one group', ids, tail(ids)))
    if cout == 256 and nblk >= max(UNIT_LIST_COUNTS.values()) + 1:
        for units in UNIT_COUNTS:
            ids = [int(v) for v in rs.permutation(nblk)[:UNIT_LIST_COUNTS[units]]]
            out.append(ConvList(f'{units} units', ids, tail(ids), GRID_CAPS))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """-> (x NCHW, w OIHW, b, {full: dense reference NHWC int64}) -- full = with bias and ReLU, else without both."""
    frames, H, W, cin, cout = shape
    g = X.gen(9300 + CONV_SHAPES.index(shape))
    x = X.acts(g, (frames, cin, H, W))
    w = X.ternary(g, (cout, cin, 3, 3), CONV_DENSITY)
    b = X.small(g, (cout,))
    return x, w, b, {True: X.conv3x3_ref(x, w, b, True)[0], False: X.conv3x3_ref(x, w, None, False)[0]}


def listed_pixels(shape, ids):
    """bool [frames][H][W]: the pixels of the listed blocks."""
    frames, H, W = shape[:3]
    by_n, bx_n = H // 8, W // 8
    m = torch.zeros(frames, H, W, dtype=torch.bool)
    for b in ids:
        assert 0 <= b < frames * by_n * bx_n
        f, rem = divmod(b, by_n * bx_n)
        r, c = divmod(rem, bx_n)
        m[f, 8 * r:8 * r + 8, 8 * c:8 * c + 8] = True
    return m


def conv_expected(shape, ids, dense):
    """What y must hold after a run over a SENTINEL-filled buffer: ``dense`` (f32 NHWC) on the listed pixels, the sentinel elsewhere."""
    return torch.where(listed_pixels(shape, ids)[..., None], dense, torch.full_like(dense, SENTINEL))


def conv_ref_frames_stacked(x, w, b, relu):
    """MUTANT of the statement: the frames stacked into one tall image, so that a block's halo row at a frame's first / last row is the
    neighbouring frame's row instead of zero."""
    n, c, h, wd = x.shape
    tall = x.permute(1, 0, 2, 3).reshape(1, c, n * h, wd)
    return X.conv3x3_ref(tall, w, b, relu)[0].reshape(n, h, wd, -1)


# raster comparison (randn inputs, no CPU convolution): (frames, H, W, Cin, Cout)
RASTER_SHAPES = ((2, 16, 24, 64, 256), (1, 56, 56, 256, 256))


def sparse_list(shape, seed=7900):
    nblk = conv_nblk(shape)
    rs = np.random.RandomState(seed + nblk)
    return sorted(int(v) for v in rs.permutation(nblk)[:max(2, nblk // 3)])
