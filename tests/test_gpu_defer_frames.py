"""-m gpu: the two kernels of the FPN levels deferred by whole frames (engine option fpn_levels_deferred), without the engine around them --
the frame marking of roi_mark_kernel (mcg_roi_mark_frames) and wino_x3w_frames_kernel (mcg_conv3x3_wino_x3_frames).  Every assertion is a
set equality or a bit equality: there is no tolerance.

  frame conv   small-integer activations and ternary weights (tests/exact_cases.py): listed frames hold the int64 statement AND the bits of
               the raster tile (mcg_conv3x3_wino_x3) on the same input, unlisted frames keep the sentinel -- for the empty list, one frame,
               all frames reversed, and all frames under grid_cap = 2 (one workgroup walks several units); on the maps of 64 x 64 and
               96 x 64 frames (16 / 8 / 4 / 2 pixels square, 24 x 16 / 12 x 8 / 6 x 4 / 3 x 2)
  marking      boxes whose scale sits below, at and above 112, 224 and 448 pixels: per level, the listed frames and the flags equal a NumPy
               statement of the level rule (roi_sample.hpp: roi_level); a second stage that shares the flags lists the new frames only
"""
import functools

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from tests import exact_cases as X

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -7.5            # no possible result: every result is an integer
FRAMES, CIN, COUT = 5, 256, 256
MAPS = ((16, 16), (8, 8), (4, 4), (2, 2), (24, 16), (12, 8), (6, 4), (3, 2))
LISTS = {'empty': ([], 0), 'one frame': ([3], 0), 'all, reversed': ([4, 3, 2, 1, 0], 0), 'all, grid_cap 2': ([1, 4, 0, 2, 3], 2)}


@pytest.fixture(scope='module')
def eng():
    from mcgaze_amd import engine
    return engine


def _i32(values, n=None):
    t = torch.zeros(len(values) if n is None else n, dtype=torch.int32, device=DEV)
    if len(values):
        t[:len(values)] = torch.tensor(list(values), dtype=torch.int32)
    return t


@functools.lru_cache(maxsize=None)
def _case(hw):
    """-> (x NHWC f32 device, w OHWI f32, packed u, bias device, dense int64 statement as f32 NHWC)"""
    from mcgaze_amd.packing import wino_pack
    H, W = hw
    g = X.gen(9500 + 31 * H + W)
    x = X.acts(g, (FRAMES, CIN, H, W))
    w = X.ternary(g, (COUT, CIN, 3, 3), 0.5)
    b = X.small(g, (COUT,))
    want = X.expected(X.conv3x3_ref(x, w, b, False)[0], torch.float32)
    wf = X.nhwc(w).float()
    return X.nhwc(x).float().to(DEV), wf, wino_pack(wf, g=2).to(DEV), b.float().to(DEV), want


@pytest.mark.parametrize('hw', MAPS, ids=lambda s: 'x'.join(map(str, s)))
def test_frame_conv_is_exact_and_has_the_raster_tiles_bits(eng, hw):
    H, W = hw
    x, wf, u, b, want = _case(hw)
    lib = L.load()
    dense = torch.empty(FRAMES, H, W, COUT, dtype=torch.float32, device=DEV)
    L.check(lib.mcg_conv3x3_wino_x3(None, x.data_ptr(), u.data_ptr(), b.data_ptr(), dense.data_ptr(), FRAMES, H, W, CIN, COUT, 0, 0, 1.0, 2), 'dense')
    outs = []
    for name, (ids, cap) in LISTS.items():
        y = torch.full((FRAMES, H, W, COUT), SENTINEL, dtype=torch.float32, device=DEV)
        # entries beyond the count name frames the list leaves out: the kernel must not compute them
        rest = [f for f in range(FRAMES) if f not in ids]
        buf = _i32(ids + rest, FRAMES)
        eng.conv3x3_wino_frames(x, u, (buf, _i32([len(ids)])), y, bias=b, grid_cap=cap)
        outs.append((name, ids, y))
    torch.cuda.synchronize()
    X.assert_exact(dense, want, f'raster tile {hw}')
    dense = dense.cpu()
    for name, ids, y in outs:
        keep = torch.zeros(FRAMES, dtype=torch.bool)
        keep[torch.tensor(ids, dtype=torch.long)] = True
        exp = torch.where(keep[:, None, None, None], want, torch.full_like(want, SENTINEL))
        X.assert_exact(y, exp, f'frame conv {hw} list "{name}"')
        assert torch.equal(y.cpu()[keep].view(torch.int32), dense[keep].view(torch.int32)), f'{hw} "{name}": not the raster tile\'s bits'


def test_frame_conv_bits_on_random_inputs(eng):
    """randn inputs and weights on the 14 x 14 and 28 x 28 maps of a 224-pixel frame (NB = 1 and 2, one and four tiles per frame): the listed
    frames carry the raster tile's bits, the others the sentinel."""
    from mcgaze_amd.packing import wino_pack
    for H in (14, 28):
        g = torch.Generator().manual_seed(9600 + H)
        x = torch.randn(FRAMES, H, H, CIN, generator=g).to(DEV)
        w = torch.randn(COUT, 3, 3, CIN, generator=g) * (9 * CIN) ** -0.5
        b = torch.randn(COUT, generator=g).to(DEV)
        u = wino_pack(w, g=2).to(DEV)
        dense = torch.empty(FRAMES, H, H, COUT, dtype=torch.float32, device=DEV)
        L.check(L.load().mcg_conv3x3_wino_x3(None, x.data_ptr(), u.data_ptr(), b.data_ptr(), dense.data_ptr(), FRAMES, H, H, CIN, COUT, 0, 0, 1.0, 2), 'dense')
        ids = [4, 0, 2]
        y = eng.conv3x3_wino_frames(x, u, ids, torch.full_like(dense, SENTINEL), bias=b)
        torch.cuda.synchronize()
        keep = torch.zeros(FRAMES, dtype=torch.bool)
        keep[torch.tensor(ids, dtype=torch.long)] = True
        assert not bool(torch.isnan(dense).any())
        assert torch.equal(y.cpu()[keep].view(torch.int32), dense.cpu()[keep].view(torch.int32)), H
        assert bool((y.cpu()[~keep] == SENTINEL).all()), H


def test_frame_conv_refuses_what_it_does_not_support():
    """Host side: a map wider than two window pieces, channel counts the tile does not divide -> MCG_ERR_UNSUPPORTED (3), nothing launched."""
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    lib = L.load()
    for n, h, w, cin, cout in ((1, 8, 32, 32, 128), (1, 56, 56, 32, 128), (1, 8, 8, 48, 128), (1, 8, 8, 32, 192), (1, 8, 1, 32, 128)):
        u = torch.zeros(max(int(lib.mcg_conv3x3_wino_x3_weight_bytes(cin - cin % 32 or 32, cout - cout % 128 or 128, 2)) // 2, 1), dtype=torch.float16, device=DEV)
        rc = lib.mcg_conv3x3_wino_x3_frames(None, z(n, h, w, cin).data_ptr(), u.data_ptr(), None, z(n, h, w, cout).data_ptr(), n, h, w, cin, cout,
                                            _i32([0]).data_ptr(), _i32([0]).data_ptr(), 0)
        assert rc == 3, (h, w, cin, cout, rc)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ marking
def roi_level(boxes, finest_scale=56.0):
    """roi_sample.hpp: roi_level, restated in float32: floor(log2(sqrt(w h) / 56 + 1e-6)) clamped to 0 .. 3, a NaN scale reads level 0."""
    b = np.asarray(boxes, dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        sc = np.sqrt((b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]), dtype=np.float32)
        lv = np.floor(np.log2(sc / np.float32(finest_scale) + np.float32(1e-6), dtype=np.float32))
    lv = np.fmin(np.fmax(lv, np.float32(0)), np.float32(3))
    return np.where(np.isnan(sc), 0, lv).astype(np.int64)


def _sq(side, cx=100.0, cy=90.0, aspect=1.0):
    """A box of scale `side` (sqrt of its area), width / height = aspect^2."""
    w, h = side * aspect, side / aspect
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


# one row per frame (3 boxes): scales around the three thresholds, square and elongated, a degenerate and an inverted box
STAGE_A = [
    [_sq(111.5), _sq(40.0), _sq(8.0)],                       # P2 only
    [_sq(112.5), _sq(111.5), _sq(60.0)],                     # P3
    [_sq(112.0), _sq(30.0), _sq(30.0)],                      # exactly 112: the rule's 1e-6 puts it on P3
    [_sq(223.5, aspect=2.0), _sq(20.0), _sq(20.0)],          # P3, elongated
    [_sq(224.5), _sq(223.5), _sq(10.0)],                     # P4 and P3
    [_sq(447.5), _sq(50.0), _sq(50.0)],                      # P4
    [_sq(448.5), _sq(447.5, aspect=0.5), _sq(112.5)],        # P5, P4, P3
    [_sq(2000.0), [5.0, 5.0, 5.0, 90.0], [90.0, 10.0, 10.0, 90.0]],   # P5; zero area and negative area (NaN scale) read P2
]
# the next stage: frames 0, 2 and 5 move to new levels, the others repeat a level they already read
STAGE_B = [
    [_sq(300.0), _sq(113.0), _sq(8.0)],
    [_sq(150.0), _sq(111.5), _sq(60.0)],
    [_sq(500.0), _sq(30.0), _sq(30.0)],
    [_sq(200.0), _sq(20.0), _sq(20.0)],
    [_sq(224.5), _sq(10.0), _sq(10.0)],
    [_sq(120.0), _sq(460.0), _sq(50.0)],
    [_sq(448.5), _sq(10.0), _sq(10.0)],
    [_sq(2000.0), _sq(10.0), _sq(10.0)],
]


def _listed(flist, count, first=0):
    n = int(count.cpu()[0])
    assert first <= n <= flist.numel(), (first, n, flist.numel())
    return flist.cpu()[first:n].tolist()


def test_frame_marking_is_the_level_rule(eng):
    a, b = np.array(STAGE_A, dtype=np.float32), np.array(STAGE_B, dtype=np.float32)
    la, lb = roi_level(a), roi_level(b)
    # the table is what it is meant to be
    assert la[:, 0].tolist() == [0, 1, 1, 1, 2, 2, 3, 3] and la[7].tolist() == [3, 0, 0] and la[6].tolist() == [3, 2, 1]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    runs = []
    for level in range(4):
        s, l1, c1 = eng.roi_mark_frames(ta, level)
        s_after_a = s.clone()
        _, l2, c2 = eng.roi_mark_frames(tb, level, state=s)
        runs.append((level, s_after_a, l1, c1, s, l2, c2))
    torch.cuda.synchronize()
    moved = False
    for level, sa, l1, c1, sb, l2, c2 in runs:
        want_a = set(np.flatnonzero((la == level).any(axis=1)).tolist())
        want_b = set(np.flatnonzero((lb == level).any(axis=1)).tolist())
        got_a, got_b = _listed(l1, c1), _listed(l2, c2)
        assert len(got_a) == len(set(got_a)) and set(got_a) == want_a, (level, got_a, want_a)       # three boxes of a frame list it once
        assert len(got_b) == len(set(got_b)) and set(got_b) == want_b - want_a, (level, got_b, want_b - want_a)
        assert sa.cpu().tolist() == [int(f in want_a) for f in range(len(a))]
        assert sb.cpu().tolist() == [int(f in want_a | want_b) for f in range(len(a))]
        moved = moved or (bool(want_b - want_a) and bool(want_b & want_a))
    assert moved, 'no level sees both a new frame and an already listed one at the second stage'


def test_frame_marking_appends_to_a_nonzero_count(eng):
    a = torch.tensor(STAGE_A, dtype=torch.float32, device=DEV)
    pre = [-11, -12]
    flist, count = _i32(pre, len(STAGE_A) + len(pre)), _i32([len(pre)])
    eng.roi_mark_frames(a, 2, flist=flist, count=count)
    torch.cuda.synchronize()
    assert flist.cpu()[:2].tolist() == pre and sorted(_listed(flist, count, first=2)) == [4, 5, 6]
