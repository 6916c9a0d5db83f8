"""No GPU: the host side of the gaze heat map (include/mcgaze_hip.h, "gaze heat map") -- attention.gaze_heat_host and arrows.draw_heat_host
against grids and pixels worked by hand and against the scalar restatements of tests/heat_cases.py, the default ramp, the options of
LiveGaze / run_head_video, and the entries' argument checks (which return before any launch).  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mcgaze_amd import arrows as R
from mcgaze_amd import attention as A
from mcgaze_amd import lib as L
from tests import heat_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCG_ERR_ARG = 1                                                   # enum of include/mcgaze_hip.h
zeros = lambda *shape: np.zeros(shape, dtype=np.int32)


# ---------------------------------------------------------------- accumulate
def test_a_radius_1_splat_at_a_corner_by_hand():
    """hit (0, 0) at cell_shift 0: the 3 x 3 pyramid 1 2 1 / 2 4 2 / 1 2 1 around cell (0, 0); five of its taps fall off the grid."""
    heat, peak = A.gaze_heat_host([[0.0, 0.0]], [1], [0], zeros(1, 3, 4), cell_shift=0, radius=1)
    assert heat.dtype == np.int32 and heat.tolist() == [[[4, 2, 0, 0], [2, 1, 0, 0], [0, 0, 0, 0]]]
    assert peak.dtype == np.int32 and peak.tolist() == [4]
    # the far corner of a second camera, picked by the period: image_of 3 % 2 = 1
    heat, peak = A.gaze_heat_host([[3.0, 2.0]], [2], [3], zeros(2, 3, 4), cell_shift=0, radius=1, period=2)
    assert heat.tolist() == [[[0] * 4] * 3, [[0, 0, 0, 0], [0, 0, 1, 2], [0, 0, 2, 4]]] and peak.tolist() == [0, 4]


def test_cells_floors_rounding_decay_and_saturation_by_hand():
    # cell_shift 2: (5, 6) and (7.4, 4.5 -> 4, half to even) both land in cell (1, 1); (-1, 2) floors to cell (-1, 0): dropped at radius 0
    heat, peak = A.gaze_heat_host([[5, 6], [7.4, 4.5], [-1, 2]], [1, 2, 1], [0, 0, 0], zeros(1, 2, 3), cell_shift=2, radius=0)
    assert heat.tolist() == [[[0, 0, 0], [0, 2, 0]]] and peak.tolist() == [2]
    # ... and at radius 1 the hit outside lights the edge: weights 2 (dx = 1, dy = 0) and 1 (dx = 1, dy = 1) in column 0
    heat, _ = A.gaze_heat_host([[-1, 2]], [1], [0], zeros(1, 2, 3), cell_shift=2, radius=1)
    assert heat.tolist() == [[[2, 0, 0], [1, 0, 0]]]
    # decay once per call, before the taps: 100 - (100 >> 2) = 75, + 1;  7 - (7 >> 2) = 6;  a negative cell counts as 0;  2^31 - 5 + 9 saturates
    before = np.array([[[100, 7, -7, 2 ** 31 - 5]]], dtype=np.int32)
    heat, peak = A.gaze_heat_host([[0, 0]], [1], [0], before, cell_shift=0, radius=0, decay=2)
    assert heat.tolist() == [[[76, 6, 0, 2 ** 31 - 5 - ((2 ** 31 - 5) >> 2)]]]
    heat, peak = A.gaze_heat_host([[3, 0]] * 9, [1] * 9, [0] * 9, before, cell_shift=0, radius=0)
    assert heat.tolist() == [[[100, 7, 0, 2 ** 31 - 1]]] and peak.tolist() == [2 ** 31 - 1]
    assert before.tolist() == [[[100, 7, -7, 2 ** 31 - 5]]]       # the grid given is not changed
    # no rows: the call still decays and writes the peak
    heat, peak = A.gaze_heat_host(np.zeros((0, 2)), [], [], before, cell_shift=0, decay=1)
    assert heat.tolist() == [[[50, 4, 0, 2 ** 31 - 5 - ((2 ** 31 - 5) >> 1)]]] and peak.tolist() == [heat.max()]


def test_which_rows_count():
    kw = dict(flags=HC.FLAGS, mask=HC.MASK, cell_shift=0, radius=0, period=HC.PERIOD)
    heat, _ = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, zeros(HC.C, 37, 53), **kw)
    assert int(heat.sum()) == len(HC.COUNTED) - 1                # the hit at (-5, 5) is outside: its one tap is dropped
    assert heat[1, 4, 2] == 1 and heat[0, 12, 20] == 1 and heat[0, 12, 21] == 1 and heat[0, 36, 10] == 1
    more, _ = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, zeros(HC.C, 37, 53), **dict(kw, kinds=15))
    assert int(more.sum()) == int(heat.sum()) + 2 and more[0, 25, 25] == 1 and more[1, 30, 40] == 1      # kinds 0 and 3; a kind word of 7 never counts
    names, _ = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, zeros(HC.C, 37, 53), **dict(kw, kinds=('none', 'head', 'region', 'camera')))
    assert np.array_equal(names, more)
    # period 0: image_of 2 and 3 have no camera
    p0, _ = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, zeros(HC.C, 37, 53), **dict(kw, period=0))
    assert int(p0.sum()) == int(heat.sum()) - 2
    # without flags and mask the flagged and the masked row count
    bare, _ = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, zeros(HC.C, 37, 53), cell_shift=0, radius=0, period=HC.PERIOD)
    assert int(bare.sum()) == int(heat.sum()) + 2


@pytest.mark.parametrize('radius', HC.RADII)
@pytest.mark.parametrize('cell_shift,grid', HC.GRIDS)
def test_gaze_heat_host_equals_the_scalar_restatement_in_any_row_order(cell_shift, grid, radius):
    before = HC.preloaded(cell_shift, grid)
    for decay, kinds in ((0, 0b0110), (1, 0b1111), (30, 0b0110)):
        args = dict(cell_shift=cell_shift, radius=radius, kinds=kinds, period=HC.PERIOD, decay=decay)
        got = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, before, flags=HC.FLAGS, mask=HC.MASK, **args)
        want = HC.heat_add_scalar(HC.HIT, HC.KIND, HC.IMAGE_OF, before, HC.FLAGS, HC.MASK, **args)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        if decay == 0 and radius == 3:                            # row 0 adds 16 to its own cell, which stood at 2^31 - 5
            assert got[0].max() == 2 ** 31 - 1 == got[1][0]
        assert got[0].min() >= 0                                  # the negative cell was read as 0
        for order in (np.arange(len(HC.ROWS))[::-1], np.random.RandomState(3).permutation(len(HC.ROWS))):
            again = A.gaze_heat_host(HC.HIT[order], HC.KIND[order], HC.IMAGE_OF[order], before, flags=HC.FLAGS[order], mask=HC.MASK[order], **args)
            assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


# ---------------------------------------------------------------- render
def test_levels_by_hand():
    # cell_shift 0: the cell's own value, 255 h / full floored
    assert R.heat_levels([[0, 10], [5, 20]], 20, 2, 2, 0).tolist() == [[0, 127], [63, 255]]
    assert R.heat_levels([[0, 10], [5, 20]], 0, 2, 2, 0).tolist() == [[0, 255], [255, 255]]             # a scale below 1 is 1
    assert R.heat_levels([[-3, 10]], 40, 1, 2, 0).tolist() == [[0, 63]]                                  # a negative cell is 0
    # cell_shift 2 (S = 4), one row of cells 0 | 80, full 80.  Cell centres lie at x = 1.5 and 5.5 -- between pixels, as for every S >= 2 --
    # so the pixels next to them are worked: u = 2 px - 3, fx = u mod 8, v = 8 ((8 - fx) 0 + fx 80), L = 255 v / (64 * 80) floored.
    #   px 0, 1: left of the first centre, both indices clamp to cell 0 -> 0      px 2: fx 1 -> 640 -> 31      px 3: fx 3 -> 1920 -> 95
    #   px 4: fx 5 -> 3200 -> 159 (3 and 4 lie either side of halfway, 3.5: 95 + 159 = 2 * 127)     px 5: fx 7 -> 4480 -> 223
    #   px 6 ..: right of the last centre, both indices clamp to cell 1 -> 255, also beyond the grid's 8 pixels
    assert R.heat_levels([[0, 80]], 80, 1, 11, 2).tolist() == [[0, 0, 31, 95, 159, 223, 255, 255, 255, 255, 255]]
    # the same in y, and both at once: pixel (3, 3) has fx = fy = 3: v = 5 * 5 * 0 + 3 * 5 * 0 + 5 * 3 * 0 + 3 * 3 * 80 = 720 -> 35
    assert R.heat_levels([[0], [80]], 80, 11, 1, 2)[:, 0].tolist() == [0, 0, 31, 95, 159, 223, 255, 255, 255, 255, 255]
    assert R.heat_levels([[0, 0], [0, 80]], 80, 8, 8, 2)[3, 3] == 720 * 255 // (64 * 80) == 35


def test_the_blend_rounds_as_stated_at_alpha_0_1_254_255():
    lut = np.zeros((256, 4), dtype=np.uint8)
    lut[1], lut[2], lut[3], lut[4] = (10, 20, 30, 0), (10, 20, 30, 1), (10, 20, 30, 254), (10, 20, 30, 255)
    frame = np.full((1, 6, 3), 200, dtype=np.uint8)
    frame[0, 5] = (0, 1, 255)
    out = R.draw_heat_host(frame, np.array([[[1, 2, 3, 4, 0, 4]]], dtype=np.int32), 255, 0, lut=lut)
    # (200 * 254 + 10 + 127) // 255 = 199, (... + 20 ...) = 199, (... + 30 ...) = 199;  (200 + 2540 + 127) // 255 = 11, 21, 31
    assert out[0].tolist() == [[200, 200, 200], [199, 199, 199], [11, 21, 31], [10, 20, 30], [200, 200, 200], [10, 20, 30]]
    assert frame[0, 1].tolist() == [200, 200, 200]               # a copy: the frame given is untouched
    # min_level: levels 1 and 2 keep their bytes
    out = R.draw_heat_host(frame, np.array([[[1, 2, 3, 4, 0, 4]]], dtype=np.int32), 255, 0, lut=lut, min_level=3)
    assert out[0, :3].tolist() == [[200, 200, 200], [200, 200, 200], [11, 21, 31]]


def test_the_nv12_chroma_pair_takes_the_highest_of_its_four_levels():
    lut = np.zeros((256, 4), dtype=np.uint8)
    lut[:, 3] = 255
    lut[:, 0], lut[:, 1], lut[:, 2] = np.arange(256), 255 - np.arange(256), np.arange(256) // 2
    y, uv = np.full((2, 4), 7, np.uint8), np.full((1, 4), 9, np.uint8)
    # levels: 0 0 | 0 100 over 0 40 | 0 0 (full 255, cell_shift 0): the left pair's level is 40, the right pair's 100
    heat = np.array([[[0, 0, 0, 100], [0, 40, 0, 0]]], dtype=np.int32)
    got_y, got_uv = R.draw_heat_host((y, uv), heat, 255, 0, lut=lut, pixel_format='nv12')
    t = R.heat_lut(lut, True, 'bt601')                           # a host table is (B, G, R, alpha): each entry converted once; alpha 255 -> the colour itself
    assert t[40, :3].tolist() == R.bgr_to_yuv(lut[40, :3]).tolist() and t[40, 3] == 255
    assert got_y.tolist() == [[7, 7, 7, t[100, 0]], [7, t[40, 0], 7, 7]] and got_uv.tolist() == [[t[40, 1], t[40, 2], t[100, 1], t[100, 2]]]
    # below min_level nothing of the left pair is written
    got_y, got_uv = R.draw_heat_host((y, uv), heat, 255, 0, lut=lut, pixel_format='nv12', min_level=41)
    assert got_y.tolist() == [[7, 7, 7, t[100, 0]], [7, 7, 7, 7]] and got_uv.tolist() == [[9, 9, t[100, 1], t[100, 2]]]


@pytest.mark.parametrize('fmt', ['bgr', 'nv12'])
@pytest.mark.parametrize('cell_shift,grid', HC.GRIDS)
def test_draw_heat_host_equals_the_scalar_restatement(fmt, cell_shift, grid):
    heat, peak = A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, np.maximum(HC.preloaded(cell_shift, grid), 0) % 1000, flags=HC.FLAGS, mask=HC.MASK,
                                  cell_shift=cell_shift, radius=3, period=HC.PERIOD)
    heat[0, 0, 0] = -9
    frames = HC.host_frames(fmt)[:3]
    lut = R.heat_lut(None, fmt == 'nv12', 'bt601')
    for period, full, min_level in ((2, peak, 1), (0, 300, 60)):
        got = R.draw_heat_host(frames, heat, full, cell_shift, period=period, min_level=min_level, pixel_format=fmt)
        for p, frame in enumerate(frames):
            c = p % period if period else p
            full_c = int(np.broadcast_to(full, (HC.C,))[c]) if c < HC.C else 0
            want = HC.draw_heat_scalar(fmt, frame, heat[c], full_c, cell_shift, lut, min_level) if c < HC.C else frame
            HC.same(fmt, [got[p]], [want], (period, p))
        changed = [not np.array_equal(g if fmt == 'bgr' else g[0], f if fmt == 'bgr' else f[0]) for g, f in zip(got, frames)]
        assert changed == [True, True, period == 2]


def test_an_empty_grid_leaves_every_frame_byte_identical():
    for fmt in ('bgr', 'nv12'):
        frames = HC.host_frames(fmt)
        got = R.draw_heat_host(frames, zeros(HC.C, 5, 7), zeros(HC.C), 3, period=2, pixel_format=fmt)
        HC.same(fmt, got, frames)
        one = R.draw_heat_host(frames[0], zeros(HC.C, 5, 7), 1, 3, pixel_format=fmt)         # one frame in, one frame out
        HC.same(fmt, [one], frames[:1])


def test_the_default_ramp():
    lut = R.HEAT_LUT
    assert lut.shape == (256, 4) and lut.dtype == np.uint8
    assert lut[0, 3] == 0 and lut[255, 3] == 160 and (np.diff(lut[:, 3].astype(int)) >= 0).all()
    assert lut[0, :3].tolist() == [255, 0, 0] and lut[63, :3].tolist() == [255, 255, 0] and lut[127, :3].tolist() == [0, 255, 0]      # blue, cyan, green
    assert lut[191, :3].tolist() == [0, 255, 255] and lut[255, :3].tolist() == [0, 0, 255]                                            # yellow, red
    assert np.array_equal(R.heat_lut(), lut)
    for table in (lut, R.heat_lut(), R.heat_lut(None, True, 'bt601')):       # the defaults are everybody's: nobody edits them in place
        with pytest.raises(ValueError):
            table[0, 0] = 1
    yuv = R.heat_lut(None, True, 'bt709')
    assert np.array_equal(yuv[:, 3], lut[:, 3]) and yuv[200, :3].tolist() == R.bgr_to_yuv(lut[200, :3], 'bt709').tolist()
    with pytest.raises(ValueError):
        R.heat_lut(np.zeros((255, 4), np.uint8))


# ---------------------------------------------------------------- options
def test_options_are_refused_with_value_errors():
    att = object()                                               # "attention was given": only its presence is looked at
    assert A._heat_options('LiveGaze', None, None, False) is None
    assert A._heat_options('LiveGaze', True, att, True) == dict(cell=8, radius=2, decay=0, kinds=A.HEAT_KINDS, draw=True, full_scale=None, min_level=1)
    assert A._heat_options('LiveGaze', dict(cell=16, draw=False), att, False)['cell'] == 16
    with pytest.raises(ValueError, match='attention'):
        A._heat_options('LiveGaze', True, None, True)            # heat without attention
    with pytest.raises(ValueError, match='needs draw'):
        A._heat_options('LiveGaze', dict(draw=True), att, False)  # heat drawn, but no frames are drawn
    for bad in (dict(cell=12), dict(cell=128), dict(cell=0), dict(radius=9), dict(decay=31), dict(kinds=('shelf',)), dict(min_level=0), dict(full_scale=0),
                dict(colour=1), 'yes'):
        with pytest.raises(ValueError):
            A._heat_options('LiveGaze', bad, att, True)
    assert A.heat_grid_shape((1080, 1920), 8) == (135, 240) and A.heat_grid_shape((37, 53), 8) == (5, 7)
    with pytest.raises(ValueError):
        A.heat_grid_shape((37, 53), 6)
    for kw in (dict(cell_shift=7), dict(radius=-1), dict(period=-1), dict(decay=31), dict(kinds=16)):
        with pytest.raises(ValueError):
            A.gaze_heat_host(HC.HIT, HC.KIND, HC.IMAGE_OF, zeros(1, 2, 2), **kw)
    with pytest.raises(ValueError):
        A.gaze_heat_host(HC.HIT, HC.KIND[:3], HC.IMAGE_OF, zeros(1, 2, 2))
    with pytest.raises(TypeError):
        A.gaze_heat_host(HC.HIT, HC.KIND.astype(np.float32), HC.IMAGE_OF, zeros(1, 2, 2))


def test_live_gaze_and_run_head_video_check_heat_before_anything_else():
    from mcgaze_amd import harness, live
    with pytest.raises(ValueError, match='attention'):
        live.LiveGaze(None, None, cameras=1, heat=True)
    with pytest.raises(ValueError, match='needs draw'):
        live.LiveGaze(None, None, cameras=1, attention=True, heat=dict(draw=True))
    with pytest.raises(ValueError, match='power of two'):
        live.LiveGaze(None, None, cameras=1, attention=True, heat=dict(cell=24, draw=False))
    with pytest.raises(ValueError, match='attention'):
        harness.run_head_video(None, None, [np.zeros((4, 4, 3), np.uint8)], [np.zeros((0, 4), np.float32)], heat=True)


# ---------------------------------------------------------------- the library
def test_abi_line_exports_and_header():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    assert int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) == L.ABI_VERSION == 20
    lib = L.load()
    for name in ('mcg_gaze_heat_add', 'mcg_draw_heat', 'mcg_draw_heat_nv12'):
        assert name in L.EXPORTS and re.search(r'\bint %s\(' % name, hdr) and hasattr(lib, name)
    assert 'gaze heat map (additions to ABI 19; nothing above changes)' in hdr


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """Every call here fails the host-side checks and returns MCG_ERR_ARG: nothing is launched, so no GPU is needed and no pointer is read."""
    lib = L.load()
    vp, p = C.c_void_p, 0x1000                                    # a non-null address that is never read

    def add(hit=p, kind=p, image_of=p, n=4, heat=p, peak=p, Cn=2, GH=5, GW=7, shift=3, radius=2, kinds=6, period=0, decay=0, work=p, work_bytes=4 * 70):
        return lib.mcg_gaze_heat_add(vp(0), vp(hit), vp(kind), vp(image_of), vp(0), vp(0), n, vp(heat), vp(peak), Cn, GH, GW, shift, radius, kinds, period,
                                     decay, vp(work), work_bytes)

    for kw in (dict(hit=0), dict(kind=0), dict(image_of=0), dict(heat=0), dict(peak=0), dict(work=0), dict(n=-1), dict(n=65537), dict(Cn=0), dict(Cn=4097),
               dict(GH=0), dict(GW=8193), dict(Cn=4096, GH=4097, GW=1), dict(shift=-1), dict(shift=7), dict(radius=-1), dict(radius=9), dict(period=-1),
               dict(decay=-1), dict(decay=31), dict(work_bytes=4 * 70 - 1)):
        assert add(**kw) == MCG_ERR_ARG, kw
        assert lib.mcg_last_error()

    def draw(entry, images=p, num=4, max_h=37, max_w=53, heat=p, full=p, Cn=2, GH=5, GW=7, shift=3, period=2, lut=p, min_level=1):
        return entry(vp(0), vp(images), num, max_h, max_w, vp(heat), vp(full), Cn, GH, GW, shift, period, vp(lut), min_level)

    for entry in (lib.mcg_draw_heat, lib.mcg_draw_heat_nv12):
        for kw in (dict(images=0), dict(heat=0), dict(full=0), dict(lut=0), dict(lut=p + 1), dict(num=0), dict(num=65536), dict(max_h=0), dict(max_w=8193),
                   dict(Cn=0), dict(Cn=4097), dict(GH=8193), dict(GW=0), dict(Cn=4096, GH=4097, GW=1), dict(shift=7), dict(shift=-1), dict(period=-1),
                   dict(min_level=0), dict(min_level=256)):
            assert draw(entry, **kw) == MCG_ERR_ARG, kw
