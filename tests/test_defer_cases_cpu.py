"""No GPU: tests/defer_cases.py's statements of the deferred P2 kernels are what tests/test_gpu_defer_blocks.py needs them to be.

  * the block footprint of every box is exactly the 8 x 8 cover of the pixels RoIAlign addresses -- no block short, none too many;
  * the census: every block-border situation of the 56 x 56 map occurs on both axes, boxes without a footprint occur for both reasons;
  * the mutants: each subtly wrong footprint rule gives another block set on a named case, so set equality on the GPU rejects it;
  * the geometry is exact in f32 (roi_exact_cases' integer proof), the block-conv inputs obey exact_cases' condition;
  * the inner-block rule (mcg_inner_block_neighbours, the kernel's own inline function) is the 3 x 3 in-frame dilation;
  * the block-conv lists are what the issue of the kernel's walk asks for: group paddings, unit counts 2, 14, 16, 18, 34, and the unit
    permutation restated in Python is a bijection.
Nothing here skips.
"""
import ctypes as C
import os
import re

import pytest
import torch

from mcgaze_amd import lib as L
from tests import defer_cases as D
from tests import exact_cases as X
from tests import roi_exact_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ footprint = cover of the read set
@pytest.mark.parametrize('name', D.MARK_CASES + ('chain',))
def test_footprint_is_the_block_cover_of_the_read_set(name):
    case = D.chain_case() if name == 'chain' else D.mark_case(name)
    by_n, bx_n = D.blocks_of(case.hw)
    nonempty = 0
    for tag, frame, box in case.rows():
        rows, cols = D.read_pixels(box, case.hw)
        assert all(0 <= r < case.hw[0] for r in rows) and all(0 <= c < case.hw[1] for c in cols), (tag, 'a tap outside the map')
        cover = {frame * by_n * bx_n + (r >> 3) * bx_n + (c >> 3) for r in rows for c in cols}
        fp = D.footprint(box, frame, case.hw)
        assert fp == cover, (name, tag)
        assert all(frame * by_n * bx_n <= b < (frame + 1) * by_n * bx_n for b in fp), (tag, 'a block of another frame')
        nonempty += bool(fp)
    assert nonempty >= 6


def test_boxes_are_exact_in_f32():
    """Every finite box goes through roi_exact_cases' proof (or, with a negative area, its grid condition): the kernel's sample
    coordinates are the statement's."""
    frame = D.mark_case('frame')
    pads = frame.frames * frame.bpf - len(R.all_boxes('frame')) - len(R.NONFINITE_BOXES)
    assert D.check_box_exactness(frame) == len(R.all_boxes('frame')) + sum(all(abs(v) < R.INF for v in b) for _, b in R.NONFINITE_BOXES) + pads
    finite56 = sum(all(v == v and abs(v) < R.INF for v in b) for b in D.mark_case('edge56').flat())
    assert D.check_box_exactness(D.mark_case('edge56')) == finite56 == 33
    assert D.check_box_exactness(D.chain_case()) == 6


def test_frame_case_holds_every_box():
    case = D.mark_case('frame')
    want = [b for _, _, b in R.all_boxes('frame')] + [b for _, b in R.NONFINITE_BOXES]
    got = case.flat()[:len(want)]
    assert len(got) == len(want) and all(str(a) == str(b) for a, b in zip(got, want))       # str: NaN corners compare
    assert case.hw == (16, 24) and case.frames == 3 and {0, 1, 2, 3} <= set(case.levels)


# ------------------------------------------------------------------------------------------------ census
SITUATIONS = ('sample at 7.0', 'sample at 8.0', 'sample in (7, 8)', 'one block', 'three blocks', 'every block', 'last pixel',
              'lone sample at -1', 'lone sample at L', 'no valid sample')


def test_census_of_the_56_map():
    case = D.mark_case('edge56')
    H, W = case.hw
    seen = {0: set(), 1: set()}
    per_box = []
    for tag, frame, box in case.rows():
        x1, y1, x2, y2 = box
        sy, sx = D.axis_situations(y1, y2, H), D.axis_situations(x1, x2, W)
        per_box.append((tag, frame, box, sy, sx))
        if R.level_of(box) == 0:
            seen[0] |= sy
            seen[1] |= sx
    for axis in (0, 1):
        assert set(SITUATIONS) <= seen[axis], (axis, set(SITUATIONS) - seen[axis])
    fps = [D.footprint(box, frame, case.hw) for _, frame, box in case.rows()]
    # three block rows x ONE block column, and the mirror
    assert any('three blocks' in sy and 'one block' in sx and len(fp) == 3 for (_, _, _, sy, sx), fp in zip(per_box, fps))
    assert any('one block' in sy and 'three blocks' in sx and len(fp) == 3 for (_, _, _, sy, sx), fp in zip(per_box, fps))
    # the zero-weight tap: the box at 7.0 lists both blocks of the axis, 'no hi tap' only the first
    for tag in ('y sample at 7.0', 'x sample at 7.0'):
        i = case.tags.index(tag)
        _, frame, box = case.rows()[i]
        assert len(fps[i]) == 2 and len(D.footprint(box, frame, case.hw, mut='no hi tap')) == 1
    # a box covering the whole map
    assert any(len(fp) == 49 for fp in fps)
    # two boxes of one frame that share blocks, neither inside the other's tag
    rows = case.rows()
    assert any(rows[i][1] == rows[j][1] and fps[i] & fps[j] for i in range(len(rows)) for j in range(i + 1, len(rows)) if case.flat()[i] != case.flat()[j])
    # the same box in two frames, with a footprint
    assert any(case.flat()[i] == case.flat()[j] and rows[i][1] != rows[j][1] and fps[i] for i in range(len(rows)) for j in range(i + 1, len(rows)))
    # the largest id, from a box of the last frame
    assert case.nblk - 1 in fps[-1] and rows[-1][1] == case.frames - 1 and fps[-1] == {case.nblk - 1}
    # a box routed to level 1 between two level-0 boxes (with footprints) of one frame
    assert any(case.levels[i] == 1 and rows[i - 1][1] == rows[i][1] == rows[i + 1][1] and fps[i - 1] and fps[i + 1] and not fps[i]
               and case.levels[i - 1] == case.levels[i + 1] == 0 for i in range(1, len(rows) - 1))
    # empty footprints: no valid sample; routing
    assert any(not fp and R.level_of(box) == 0 for (_, _, box), fp in zip(rows, fps))
    assert any(not fp and R.level_of(box) != 0 and D.footprint(box, frame, case.hw, mut='routing dropped') for (_, frame, box), fp in zip(rows, fps))
    union = case.footprint()
    assert union and len(union) < case.nblk and len(union) == 100


def test_census_of_the_frame_map():
    """The 16 x 24 map's boxes hit every validity edge on level 0 (roi_exact_cases.edge_census), and hold both kinds of empty footprint."""
    case = D.mark_case('frame')
    shim = D._ExactShim(case, [i for i, b in enumerate(case.flat()) if all(v == v and abs(v) < R.INF for v in b)])
    seen = R.edge_census(shim)
    for axis in (0, 1):
        for kind in ('at -1', 'at L', 'below -1', 'above L', 'in (-1, 0)', 'in [L-1, L]', 'zero', 'inverted', 'outside'):
            assert (0, axis, kind) in seen, (axis, kind)
    rows = case.rows()
    fps = [D.footprint(box, frame, case.hw) for _, frame, box in rows]
    assert any(not fp and R.level_of(box) == 0 for (_, _, box), fp in zip(rows, fps))
    assert any(not fp and R.level_of(box) != 0 for (_, _, box), fp in zip(rows, fps))
    assert sum(bool(fp) for fp in fps) >= 50


# ------------------------------------------------------------------------------------------------ mutants
# mutant -> (case, tag of a box on which it must give another block set)
MUTANT_WITNESS = {
    'no hi tap': ('edge56', 'y sample at 7.0'),
    'valid: c > -1': ('edge56', 'x lone sample at -1'),
    'valid: c < L': ('edge56', 'y lone sample at L'),
    'from the corners': ('edge56', 'y sample at 8.0'),
    'dilated by one block': ('edge56', 'y one block'),
    'frame offset dropped': ('edge56', 'last block of the last frame'),
    'routing dropped': ('edge56', 'routed to level 1'),
}


@pytest.mark.parametrize('mut', D.MUTANTS)
def test_mutant_gives_another_block_set(mut):
    name, tag = MUTANT_WITNESS[mut]
    case = D.mark_case(name)
    _, frame, box = case.rows()[case.tags.index(tag)]
    assert D.footprint(box, frame, case.hw, mut=mut) != D.footprint(box, frame, case.hw), (mut, tag)
    # and the union over the call, which is what the GPU test compares
    assert case.footprint(mut=mut) != case.footprint(), (mut, name)


def test_mutants_are_all_witnessed():
    assert set(MUTANT_WITNESS) == set(D.MUTANTS)
    # 'no hi tap' and the corners rule differ on the 16 x 24 map as well; the two validity mutants only where a sample is the LONE valid one
    frame = D.mark_case('frame')
    assert any(D.footprint(b, f, frame.hw, mut='no hi tap') != D.footprint(b, f, frame.hw) for _, f, b in frame.rows())
    for mut in ('valid: c > -1', 'valid: c < L'):
        assert all(D.footprint(b, f, frame.hw, mut=mut) == D.footprint(b, f, frame.hw) for _, f, b in frame.rows())


# ------------------------------------------------------------------------------------------------ the inner-block rule
def _twin(bid, H, W):
    buf = (C.c_int * 9)()
    k = L.load().mcg_inner_block_neighbours(int(bid), H, W, buf)
    ids = list(buf[:k])
    assert 1 <= k <= 9 and len(set(ids)) == k
    return set(ids)


@pytest.mark.parametrize('frames,H,W', D.INNER_MAPS)
def test_inner_rule_is_the_in_frame_dilation(frames, H, W):
    by_n, bx_n = D.blocks_of((H, W))
    bpf = by_n * bx_n
    for bid in range(frames * bpf):
        assert _twin(bid, H, W) == D.dilate([bid], frames, (H, W)), (bid, H, W)
        assert all(b // bpf == bid // bpf for b in _twin(bid, H, W))
    for name, ids in D.inner_lists(frames, (H, W)).items():
        assert set().union(*[_twin(b, H, W) for b in ids]) == D.dilate(ids, frames, (H, W)), name
    assert len(_twin(0, H, W)) == min(2, by_n) * min(2, bx_n)                                # a frame corner; a one-block frame: itself
    if frames > 1:
        seam = D.dilate([bpf - 1, bpf], frames, (H, W))
        assert seam == _twin(bpf - 1, H, W) | _twin(bpf, H, W)
        assert not (_twin(bpf - 1, H, W) & _twin(bpf, H, W))                                  # last of frame 0, first of frame 1: nothing shared
    assert D.INNER_MAPS[0][1:] == (8, 8) and D.INNER_MAPS[1][1] == 8


# ------------------------------------------------------------------------------------------------ the block conv
@pytest.mark.parametrize('shape', D.CONV_SHAPES)
def test_conv_cases_are_exact_and_lists_are_sound(shape):
    x, w, b, refs = D.conv_case(shape)
    bound = X.check_exactness_wino(x, w, b, 2, f'block conv {shape}')
    assert bound < X.LIMIT
    X.check_exactness(X.conv3x3_ref, f'block conv {shape}', x3=True, activations=('x',), x=x, w=w, b=b, relu=True)
    frames, H, W, cin, cout = shape
    assert H % 8 == 0 and W % 8 == 0 and cin % 32 == 0 and cout % 128 == 0
    nblk = D.conv_nblk(shape)
    lists = D.conv_lists(shape)
    names = [l.name for l in lists]
    assert 'count 0' in names and 'all, raster' in names and 'all, permuted' in names and 'frame corners' in names
    for c in (1, 2, 3, 5):
        assert (f'count {c}' in names) == (c <= nblk)
    for l in lists:
        assert len(set(l.ids)) == len(l.ids) and all(0 <= v < nblk for v in l.buffer) and len(l.buffer) > len(l.ids), l.name
        if len(l.ids) < nblk:                        # the entries beyond the count name blocks the list leaves out
            assert not set(l.buffer[len(l.ids):]) & set(l.ids), l.name
        want = D.conv_expected(shape, l.ids, X.expected(refs[True], torch.float32))
        assert int((want == D.SENTINEL).all(dim=-1).sum()) == (nblk - len(l.ids)) * 64, l.name
    assert not bool((refs[True] == D.SENTINEL).any()) and not bool((refs[False] == D.SENTINEL).any())
    by_name = {l.name: l for l in lists}
    assert sorted(by_name['all, permuted'].ids) == by_name['all, raster'].ids == list(range(nblk)) and (nblk == 1 or by_name['all, permuted'].ids != list(range(nblk)))
    if frames >= 2:
        bpf = nblk // frames
        seam = by_name['frame seam in one group'].ids
        assert len(seam) == 4 and {bpf - 1, bpf} <= set(seam)                                # ONE group of four holds both sides of a frame seam
        # ... and there the statement differs from a conv over the stacked frames (a halo row taken from the neighbouring frame)
        stacked = D.conv_ref_frames_stacked(x, w, b, True)
        m = D.listed_pixels(shape, [bpf - 1, bpf])
        assert bool((stacked[m] != refs[True][m]).any())
    assert (W > 62) == (shape == (1, 8, 72, 32, 128))


def test_unit_counts_and_permutation():
    shape = (2, 48, 48, 32, 256)
    lists = {l.name: l for l in D.conv_lists(shape)}
    for units in D.UNIT_COUNTS:
        l = lists[f'{units} units']
        assert D.units_of(len(l.ids), 256) == units == 2 * -(-len(l.ids) // 4) and l.caps == (0, 16, 3)
    assert D.UNIT_COUNTS == (2, 14, 16, 18, 34)
    for shape in D.CONV_SHAPES:
        for l in D.conv_lists(shape):
            units, padded, order = D.unit_order(len(l.ids), shape[4])
            assert sorted(order) == list(range(padded)) and padded >= units, (shape, l.name)   # a bijection of [0, padded)
            assert padded == (units if shape[4] == 128 else -(-units // 16) * 16)
            assert sorted(v for v in order if v < units) == list(range(units))                  # every unit runs exactly once
            if shape[4] == 256:                      # the two channel tiles of one group of blocks are eight slots apart: one XCD
                pos = {v: u for u, v in enumerate(order)}
                assert all(pos[2 * m + 1] - pos[2 * m] == 8 for m in range(padded // 2))
    # the counts straddle the padding to 16 and one persistent trip of a 16- and a 3-workgroup grid
    assert [D.unit_order(c, 256)[1] for c in (3, 27, 32, 33, 66)] == [16, 16, 16, 32, 48]


def test_symbols_are_declared():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    for name, nargs in (('mcg_roi_mark_blocks', 11), ('mcg_inner_mark_blocks', 9), ('mcg_conv3x3_wino_x3_blocks', 16)):
        assert name in L.EXPORTS and re.search(r'\bint %s\s*\(' % name, hdr) and hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
        decl = re.search(r'\bint %s\s*\(([^;]*)\);' % name, hdr).group(1)
        assert len(decl.split(',')) == nargs, name
    assert lib.mcg_abi_version() == L.ABI_VERSION == int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) >= 20
    for phrase in ('MUST BE DISTINCT AND INSIDE [0, frames * (H / 8) * (W / 8))', 'is added to, not reset', 'routes to another level does nothing'):
        assert phrase in hdr, phrase
