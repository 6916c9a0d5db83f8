"""The inner-block rule of the deferred FPN P2 lateral (inner_mark_kernel, roi_align.hip; engine option fpn_lateral_deferred): the 3 x 3
output conv of a listed 8 x 8 block reads that block and its neighbours INSIDE THE SAME FRAME, and nothing beyond the image border.  The
kernel's rule has a host twin (mcg_inner_block_neighbours, the same inline function); here it is checked against a numpy dilation."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from mcgaze_amd import lib as L


def dilate(listed):
    """listed [N, by, bx] bool -> the blocks whose inner pixels the listed blocks' 3 x 3 convs read: a 3 x 3 dilation per frame."""
    n, by, bx = listed.shape
    pad = np.zeros((n, by + 2, bx + 2), dtype=bool)
    pad[:, 1:-1, 1:-1] = listed
    out = np.zeros_like(listed)
    for dy in range(3):
        for dx in range(3):
            out |= pad[:, dy:dy + by, dx:dx + bx]
    return out


def twin(listed, H, W):
    lib = L.load()
    out = np.zeros(listed.size, dtype=bool)
    buf = (C.c_int * 9)()
    for bid in np.flatnonzero(listed.reshape(-1)):
        k = lib.mcg_inner_block_neighbours(int(bid), H, W, buf)
        assert 1 <= k <= 9
        ids = list(buf[:k])
        assert len(set(ids)) == k and int(bid) in ids
        out[ids] = True
    return out.reshape(listed.shape)


@pytest.mark.parametrize('frames,H,W', [(3, 16, 16), (4, 16, 24), (2, 56, 56), (3, 8, 8), (2, 8, 40), (2, 64, 48)])
def test_inner_rule_single_blocks(frames, H, W):
    """Every block on its own: corners have 4 blocks, edges 6, the interior 9 -- and never one of another frame."""
    by, bx = H // 8, W // 8
    for bid in range(frames * by * bx):
        listed = np.zeros((frames, by, bx), dtype=bool)
        listed.reshape(-1)[bid] = True
        got = twin(listed, H, W)
        assert np.array_equal(got, dilate(listed)), (bid, H, W)
        f = bid // (by * bx)
        assert not got[np.arange(frames) != f].any()


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_inner_rule_random_sets(seed):
    rs = np.random.RandomState(seed)
    for frames, H, W in [(3, 32, 32), (5, 56, 56), (4, 16, 24)]:
        listed = rs.rand(frames, H // 8, W // 8) < 0.2
        listed[0, -1, :] = True            # the whole last block row of frame 0: frame 1's first row must stay out unless frame 1 asks
        listed[1] = False
        got = twin(listed, H, W)
        assert np.array_equal(got, dilate(listed))
        assert not got[1].any()


def test_symbols_are_declared():
    hdr = open(os.path.join(os.path.dirname(L.__file__), '..', 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    for name in ('mcg_deferred_pyramid_state', 'mcg_inner_block_neighbours'):
        assert name in L.EXPORTS and re.search(r'\bint %s\s*\(' % name, hdr) and hasattr(lib, name)
    assert 'fpn_lateral_deferred' in hdr
