"""Gaze arrows on the host (not gpu): the arithmetic of include/mcgaze_hip.h, "annotated frames out", as mcgaze_amd/pipeline.py restates it
-- the plan (arrow_segments), the capsule coverage (segment_coverage), the drawing (draw_arrows_host) and the colour an NV12 surface is drawn
with (bgr_to_yuv) -- against restatements in rationals, answers worked by hand and a search of the whole (Y, U, V) cube.  The device kernels
are compared with draw_arrows_host, bit for bit, in tests/test_gpu_draw.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from mcgaze_amd import harness
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import draw_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- coverage
def test_coverage_equals_the_distance_test_in_rationals():
    rs = np.random.RandomState(7)
    for _ in range(300):
        a, b = rs.randint(-4, 14, 2), rs.randint(-4, 14, 2)
        if rs.rand() < 0.1:
            b = a.copy()                                         # a segment of no length
        t = int(rs.randint(1, 10))
        got = P.segment_coverage(10, 11, a, b, t)
        want = np.array([[D.covered_exactly(x, y, a, b, t) for x in range(11)] for y in range(10)])
        assert np.array_equal(got, want), (a, b, t)
        # a window of the same plane: the origin arguments only move it
        assert np.array_equal(P.segment_coverage(4, 5, a, b, t, y0=3, x0=2), want[3:7, 2:7])


def test_coverage_counts_worked_by_hand():
    m = P.segment_coverage(8, 9, (2, 3), (6, 3), 1)                  # radius 1/2: only the pixels the segment passes through
    assert m.sum() == 5 and m[3, 2:7].all()
    m = P.segment_coverage(8, 9, (0, 0), (3, 3), 1)                  # (1, 0) is sqrt(1/2) away: the 4 diagonal pixels
    assert m.sum() == 4 and all(m[k, k] for k in range(4))
    m = P.segment_coverage(9, 9, (4, 4), (4, 4), 5)                  # 4 (dx^2 + dy^2) <= 25: the 21 pixels with dx^2 + dy^2 <= 6
    yy, xx = np.mgrid[-4:5, -4:5]
    assert m.sum() == 21 and np.array_equal(m, xx * xx + yy * yy <= 6)


def test_coverage_is_exact_at_the_bound():
    """End points at +-8191, a pixel at the far corner of an 8192 frame, t = 255: the products stay below 2^60 (python ints agree)."""
    a, b, t = (-8191, -8191), (8191, 8190), 255
    for px, py in ((8191, 8191), (0, 0), (8191, 0), (4000, 4000), (4000, 4127), (4000, 4181)):
        got = bool(P.segment_coverage(1, 1, a, b, t, y0=py, x0=px)[0, 0])
        assert got == D.covered_exactly(px, py, a, b, t), (px, py)


# ---------------------------------------------------------------- plan
def test_head_strokes_and_thickness_worked_by_hand():
    # pt1 = (0, 0), pt2 = (100, 0): centre 0, l = 100, gaze (-1, 0).  k = 0.1 sqrt(1/2) = 0.0707..: strokes start at 100 - 7.07 = 92.9 -> 93, -+ 7.07 -> -+ 7
    seg, t, flags = P.arrow_segments([[-50, -50, 50, 50]], [[-1, 0]])
    assert seg[0].tolist() == [[[0, 0], [100, 0]], [[93, -7], [100, 0]], [[93, 7], [100, 0]]] and t.tolist() == [5] and flags.tolist() == [0]
    # t = max(5, int(l * 0.01)): int(4.99) = 4 -> 5, int(5.0) = 5, int(6.0) = 6
    boxes = [[0, 0, l, 10] for l in (499, 500, 600)]
    assert P.arrow_segments(boxes, np.zeros((3, 2)))[1].tolist() == [5, 5, 6]
    _, t, flags = P.arrow_segments(boxes, np.zeros((3, 2)), min_thickness=1, thickness_ratio=0.5)
    assert t.tolist() == [249, 250, 0] and flags.tolist() == [0, 0, 2]                            # 300 > 255: flagged, a zero row
    # tip_length 0: k = 0 and the strokes have no length -- they start at the tip
    seg, _, _ = P.arrow_segments([[-1, -1, 1, 1], [-3, -3, 3, 3]], [[-0.5, 0], [-0.5, 0]], tip_length=0.0)
    assert seg[:, 1].tolist() == seg[:, 2].tolist() == [[[1, 0], [1, 0]], [[3, 0], [3, 0]]]
    # half to even: tip_length 0.7071067811865475 makes k = tip_length * 0.7071067811865476 exactly 0.5.  pt1 = (0, 0), pt2 = (5, 0): dx = -5, the
    # stroke starts are (5 - 2.5, -+ 2.5) -> (2, -+ 2); pt2 = (int(7.5), 0): (7 - 3.5, -+ 3.5) -> (4, -+ 4).  (Half away from zero would give 3 and 3.)
    assert 0.7071067811865475 * 0.7071067811865476 == 0.5
    seg, _, _ = P.arrow_segments([[-5, -5, 5, 5]] * 2, [[-0.5, 0], [-0.75, 0]], tip_length=0.7071067811865475)
    assert seg[:, 0, 1].tolist() == [[5, 0], [7, 0]]
    assert seg[:, 1, 0].tolist() == [[2, -2], [4, -4]] and seg[:, 2, 0].tolist() == [[2, 2], [4, 4]]


def test_shaft_equals_head_arrows():
    assert np.array_equal(P.arrow_segments(D.BOXES, D.GAZE)[0][:, 0], D.SHAFTS)               # worked by hand in tests/draw_cases.py
    rs = np.random.RandomState(11)
    boxes = np.concatenate([D.BOXES, rs.uniform(-300, 900, (40, 4)).astype(np.float32)])
    gaze = np.concatenate([D.GAZE, rs.uniform(-1, 1, (40, 3)).astype(np.float32)])
    seg, _, flags = P.arrow_segments(boxes, gaze)
    assert not flags.any()
    assert np.array_equal(seg[:, 0], harness.head_arrows(boxes, gaze))
    assert torch.equal(torch.from_numpy(seg[:, 0]), harness.head_arrows(boxes, torch.from_numpy(gaze)))
    assert np.array_equal(seg[:, 1:, 1], seg[:, :1, 1].repeat(2, axis=1))                      # both strokes run into the tip


# ---------------------------------------------------------------- drawing
def frame(h=40, w=48, seed=1):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def test_the_highest_row_wins_an_overlap():
    f = frame()
    boxes, gaze = D.BOXES[[0, 10]], D.GAZE[[0, 10]]                  # both start at (24, 20)
    red, blue = (0, 0, 255), (255, 0, 0)
    a, fa = P.draw_arrows_host(f, boxes, gaze, color=np.array([red, blue]))
    b, fb = P.draw_arrows_host(f, boxes[::-1], gaze[::-1], color=np.array([blue, red]))      # the same two arrows, each with its colour, swapped
    assert fa.tolist() == fb.tolist() == [0, 0]
    only0 = (P.draw_arrows_host(f, boxes[:1], gaze[:1])[0] != f).any(axis=2)
    only1 = (P.draw_arrows_host(f, boxes[1:], gaze[1:])[0] != f).any(axis=2)
    both = only0 & only1
    assert both.sum() > 10 and (only0 & ~both).any() and (only1 & ~both).any()
    assert (a[both] == blue).all() and (b[both] == red).all()       # the second row of each call
    for img in (a, b):
        assert (img[only0 & ~both] == red).all() and (img[only1 & ~both] == blue).all()
        assert np.array_equal(img[~(only0 | only1)], f[~(only0 | only1)])
    # swapping the rows swaps the colour in the overlap, and only there
    assert np.array_equal((a != b).any(axis=2), both)


def test_unusable_rows_are_flagged_or_refused_and_change_no_byte():
    frames = [frame(12, 16, 2), frame(40, 48, 3)]
    ok_box, ok_gaze = [14, 10, 34, 30], [0.5, -0.25]
    kinds = {
        'nan gaze': (ok_box, [np.nan, 0.0], 1),
        'inf box': ([0, 0, np.inf, 4], ok_gaze, 1),
        'image_of past the table': (ok_box, ok_gaze, 2),
        'negative image_of': (ok_box, ok_gaze, -1),
        'centre beyond 8191': ([0, 0, 20000, 20000], ok_gaze, 1),
        'tip beyond -8191': ([0, 0, 4000, 4000], [3.0, 0.0], 1),      # 2000 - 4000 * 3 = -10000
        'stroke start beyond 8191': ([8000, 0, 8300, 300], [-0.1, -1.0], 1),   # tip (8180, 450); stroke: 8180 + 7.07 (-30 + 300) / 100 -> 8199
    }
    for what, (box, gaze, io) in kinds.items():
        out, flags = P.draw_arrows_host(frames, [ok_box, box], [ok_gaze, gaze], image_of=[1, io], min_thickness=3)
        assert flags.tolist() == [0, 2], what
        want, _ = P.draw_arrows_host(frames, [ok_box], [ok_gaze], image_of=[1], min_thickness=3)
        assert all(np.array_equal(o, w) for o, w in zip(out, want)) and np.array_equal(out[0], frames[0]) and (out[1] != frames[1]).any(), what
        with pytest.raises(ValueError):
            P.draw_arrows_host(frames, [ok_box, box], [ok_gaze, gaze], image_of=[1, io], strict=True)
    _, flags = P.draw_arrows_host(frames, [[0, 0, 30000, 10]], [[0, 0]], thickness_ratio=0.01)       # t = 300
    assert flags.tolist() == [2]
    assert P.draw_arrows_host(frames, [[100, 100, 120, 120]], [[0.5, 0.5]], image_of=[1], strict=True)[1].tolist() == [0]   # wholly outside: drawn, no pixel
    for bad in (dict(min_thickness=0), dict(min_thickness=256), dict(length=np.inf), dict(tip_length=np.nan)):
        with pytest.raises(ValueError):
            P.draw_arrows_host(frames, [ok_box], [ok_gaze], **bad)
    with pytest.raises(ValueError):                                  # an NV12 surface with an odd size
        P.draw_arrows_host((np.zeros((6, 5), np.uint8), np.zeros((3, 5), np.uint8)), [ok_box], [ok_gaze], pixel_format='nv12')
    with pytest.raises(TypeError):
        P.draw_arrows_host(np.zeros((4, 4), np.uint8), [ok_box], [ok_gaze])
    with pytest.raises(ValueError):
        P.draw_arrows_host(frames, [ok_box], [ok_gaze], color=[1, 2])


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
def test_nv12_chroma_rule_and_read_back(matrix):
    y, uv = D.NV12_FRAMES[3]
    yuv = P.bgr_to_yuv(P.ARROW_COLOR, matrix)
    shown = P._yuv_to_bgr(yuv, P.YUV_COEF[matrix]).astype(np.uint8)
    # ONE covered luma pixel -- (5, 7), the odd / odd corner of its block: a disc of thickness 1 -- sets its chroma pair
    (y1, uv1), flags = P.draw_arrows_host((y, uv), [[5, 7, 5, 7]], [[0, 0]], pixel_format='nv12', matrix=matrix, min_thickness=1)
    assert flags.tolist() == [0] and (y1 != y).sum() <= 1 and y1[7, 5] == yuv[0]
    assert uv1.reshape(20, 24, 2)[3, 2].tolist() == yuv[1:].tolist()
    rest = np.ones((20, 24), bool)
    rest[3, 2] = False
    assert np.array_equal(uv1.reshape(20, 24, 2)[rest], uv.reshape(20, 24, 2)[rest])
    # the cases: every covered pixel shows the converted colour, Y is untouched elsewhere, chroma is touched exactly under covered blocks
    rows = D.IMAGE_OF == 3
    (y2, uv2), flags = P.draw_arrows_host((y, uv), D.BOXES[rows], D.GAZE[rows], pixel_format='nv12', matrix=matrix)
    covered = (P.draw_arrows_host(np.zeros((40, 48, 3), np.uint8), D.BOXES[rows], D.GAZE[rows], color=(1, 1, 1))[0] != 0).any(axis=2)
    assert not flags.any() and 300 < covered.sum() < 40 * 48
    bgr = P.nv12_to_bgr(y2, uv2, matrix)
    assert (bgr[covered] == shown).all() and np.array_equal(y2[~covered], y[~covered]) and (y2[covered] == yuv[0]).all()
    blocks = covered.reshape(20, 2, 24, 2).any(axis=(1, 3))
    assert (uv2.reshape(20, 24, 2)[blocks] == yuv[1:]).all() and np.array_equal(uv2.reshape(20, 24, 2)[~blocks], uv.reshape(20, 24, 2)[~blocks])


# ---------------------------------------------------------------- the colour of an NV12 arrow
# The demo's colour and two more whose channels keep clear of 0 and 255.  (At the clamp the cube holds many far-away triples that convert to the
# same BGR -- every Y below 16 shows black -- and its lexicographically first one is not the neighbour of the inverse that bgr_to_yuv keeps.)
CUBE_COLORS = [P.ARROW_COLOR, (17, 130, 200), (128, 128, 128)]


@pytest.fixture(scope='module')
def cube():
    g = np.arange(256, dtype=np.int32)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
def test_bgr_to_yuv_equals_a_search_of_the_whole_cube(cube, matrix):
    k = P.YUV_COEF[matrix]
    shown = P._yuv_to_bgr(cube, k)
    # a channel is cy y + cu u + cv v: half a step of Y, half a step of each chroma component that enters it, and the final rounding
    step = lambda *cs: sum(abs(k[c]) for c in cs) / 2.0 / (1 << 20) + 0.5
    bound = np.array([step('cy', 'cub'), step('cy', 'cug', 'cvg'), step('cy', 'cvr')])
    for color in CUBE_COLORS:
        err = np.abs(shown - np.array(color)).max(axis=1)
        best = cube[int(np.argmin(err))]                             # the first of the smallest: lexicographic order
        got = P.bgr_to_yuv(color, matrix)
        assert got.dtype == np.uint8 and got.tolist() == best.tolist(), (color, matrix)
        back = P._yuv_to_bgr(got, k)
        assert (np.abs(back - np.array(color)) <= bound).all(), (color, back.tolist(), bound.tolist())
        # the conversion used is nv12_to_bgr's
        y = np.full((2, 2), got[0], np.uint8)
        assert P.nv12_to_bgr(y, np.array([[got[1], got[2]]], np.uint8), matrix)[0, 0].tolist() == back.tolist()


# ---------------------------------------------------------------- the boundary
def test_header_binding_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    for name in ('mcg_draw_gaze_arrows', 'mcg_draw_gaze_arrows_nv12'):
        assert re.search(r'\bint ' + name + r'\(', hdr) and name in L.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 18
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20 and '#define MCG_ABI_VERSION 20' in hdr
    assert P._ARROW.itemsize == 80 and 'draw.hip' in open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'Makefile')).read()
    assert P.DevicePipeline.draw_arrows is not None


def test_run_head_video_draw_defaults_to_none():
    sig = inspect.signature(harness.run_head_video)
    assert sig.parameters['draw'].default is None and list(sig.parameters)[-1] == 'draw'
