"""The attention overlay on the host (not gpu): arrows.draw_attention_host, the twin of mcg_draw_attention / mcg_draw_attention_nv12
(include/mcgaze_hip.h, "attention overlay"), against answers worked by hand, draw_arrows_host (the anchor), compositions of its own layers,
plain double loops and a scalar restatement in Python ints.  Every comparison is exact.  The device kernels are compared with the twin, bit
for bit, in tests/test_gpu_overlay.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mcgaze_amd import arrows as AR
from mcgaze_amd import attention as AT
from mcgaze_amd import lib as L
from tests import draw_cases as D
from tests import overlay_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [('bgr', 'bt601'), ('nv12', 'bt601'), ('nv12', 'bt709')]
IDS = ['bgr', 'nv12-bt601', 'nv12-bt709']
draw = AR.draw_attention_host


def test_a_scene_worked_by_hand_on_the_12x16_frame():
    """Thickness 1 covers exactly the pixels ON a segment (4 d^2 <= 1 and d^2 an integer or a half: d = 0).  A degenerate triangle
    (2,2) (9,2) (9,2) is one horizontal edge; the rectangle (3,5)-(8,9) is its four sides; the head box (8,8)-(12,12) has its centre at
    (10, 10) and looks at the rectangle, hit (13.5, 6.5): both round half to even, to (14, 6), and the 45-degree line passes through pixel
    centres only at its five lattice points.  No arrows (min_thickness 0)."""
    frame = np.zeros((12, 16, 3), np.uint8)
    regions = [[[2, 2], [9, 2], [9, 2]], [3, 5, 8, 9]]
    got, flags, region_flags, active = draw(frame, [[8, 8, 12, 12]], [[0.5, 0.5, 0]], [0], [2], [1], [[13.5, 6.5]], [0], regions=regions, palette=O.PALETTE,
                                            line_thickness=1, region_thickness=1, min_thickness=0)
    assert flags.tolist() == [0] and region_flags.tolist() == [0, 0] and active.tolist() == [[0, 1]]
    edge = {(x, 2) for x in range(2, 10)}
    rect = {(x, y) for x in range(3, 9) for y in (5, 9)} | {(x, y) for x in (3, 8) for y in range(5, 10)}
    line = {(10, 10), (11, 9), (12, 8), (13, 7), (14, 6)}
    want = np.zeros_like(frame)
    for pixels, colour in ((edge, O.PALETTE[5]), (rect, O.PALETTE[6]), (line, O.PALETTE[2])):      # outline, outline looked at, kind "region"
        for x, y in pixels:
            want[y, x] = colour
    assert np.array_equal(got, want) and len(edge) == 8 and len(rect) == 18


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_the_anchor_no_regions_and_kind_zero_is_draw_arrows_host(fmt, matrix):
    n = len(D.ROWS)
    zero = np.zeros(n, np.int32)
    for color, t in ((None, 5), ((9, 200, 77), 1), ((250, 3, 128), 9)):
        pal = np.array(AR.OVERLAY_PALETTE)
        pal[0] = AR.ARROW_COLOR if color is None else color
        want, want_flags = AR.draw_arrows_host(O.frames(fmt), D.BOXES, D.GAZE, D.IMAGE_OF, color=color, pixel_format=fmt, matrix=matrix, min_thickness=t)
        got, flags, region_flags, active = draw(O.frames(fmt), D.BOXES, D.GAZE, D.IMAGE_OF, zero, zero - 1, np.zeros((n, 2), np.float32), zero, palette=pal,
                                                pixel_format=fmt, matrix=matrix, min_thickness=t)
        O.same(fmt, got, want, t)
        assert np.array_equal(flags, want_flags) and region_flags.shape == (0,) and active.shape == (4, 0)
    assert AR.OVERLAY_PALETTE[0] == AR.ARROW_COLOR and len(set(AR.OVERLAY_PALETTE)) == 7
    want, want_flags = AR.draw_arrows_host(O.frames(fmt), D.FLAG_BOXES, D.FLAG_GAZE, D.FLAG_IMAGE_OF, pixel_format=fmt, matrix=matrix)
    k = len(D.FLAGS)
    got, flags, _, _ = draw(O.frames(fmt), D.FLAG_BOXES, D.FLAG_GAZE, D.FLAG_IMAGE_OF, [0] * k, [-1] * k, np.zeros((k, 2)), [0] * k, pixel_format=fmt, matrix=matrix)
    O.same(fmt, got, want, 'flag rows')
    assert flags.tolist() == want_flags.tolist() == D.FLAGS


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_a_rectangle_as_two_vertices_and_as_its_polygon_in_both_windings(fmt, matrix):
    frames = O.frames(fmt)[3:]
    none = dict(boxes=np.zeros((0, 4)), gaze=np.zeros((0, 3)), image_of=[], kind=[], target=[], hit=np.zeros((0, 2)), mutual=[], pixel_format=fmt, matrix=matrix)
    for t in (1, 2, 5):
        a, _, fa, _ = draw(frames, regions=[[6, 8, 40, 30]], region_thickness=t, **none)
        b, _, fb, _ = draw(frames, regions=[[[6, 8], [40, 8], [40, 30], [6, 30]]], region_thickness=t, **none)
        c, _, fc, _ = draw(frames, regions=[[[6, 30], [40, 30], [40, 8], [6, 8]]], region_thickness=t, **none)
        d, _, _, _ = draw(frames, regions=np.array([[6, 8, 40, 30]], np.float32), region_thickness=t, **none)      # the [m, 4] form
        O.same(fmt, a, b, t), O.same(fmt, a, c, t), O.same(fmt, a, d, t)
        assert fa.tolist() == fb.tolist() == fc.tolist() == [0] and not np.array_equal(O.luma(fmt, a[0]), O.luma(fmt, frames[0]))


def masks(fmt, before, after):
    return [O.luma(fmt, a) != O.luma(fmt, b) if fmt != 'bgr' else (a != b).any(axis=2) for a, b in zip(after, before)]


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_layers_drawn_alone_and_composed_by_masks_equal_the_one_call(fmt, matrix):
    """Frames of a constant the palette never gives, so that a changed pixel is a covered pixel."""
    kw = dict(pixel_format=fmt, matrix=matrix, min_thickness=3, line_thickness=3, region_thickness=3)
    shapes = D.SHAPES
    base = [np.full((h, w, 3), 1, np.uint8) for h, w in shapes] if fmt == 'bgr' else [(np.full((h, w), 1, np.uint8), np.full((h // 2, w), 1, np.uint8)) for h, w in shapes]
    whole, flags, region_flags, active = draw(base, **O.scene(**kw))
    alone = {name: draw(base, **O.scene(**dict(kw, **off)))[0] for name, off in
             (('regions', dict(min_thickness=0, line_thickness=0)), ('lines', dict(min_thickness=0, region_thickness=0)),
              ('arrows', dict(line_thickness=0, region_thickness=0)))}
    composed = [np.array(f) if fmt == 'bgr' else tuple(np.array(p) for p in f) for f in base]
    triple = 0
    for name in ('regions', 'lines', 'arrows'):                    # low to high
        for k, m in enumerate(masks(fmt, base, alone[name])):
            if fmt == 'bgr':
                composed[k][m] = alone[name][k][m]
            else:
                composed[k][0][m] = alone[name][k][0][m]
    if fmt == 'bgr':
        O.same(fmt, whole, composed, 'composed')
    else:                                                         # chroma belongs to the highest stroke of the four: composed luma, and the scalar test does the pairs
        assert all(np.array_equal(w[0], c[0]) for w, c in zip(whole, composed))
    ms = {name: masks(fmt, base, alone[name]) for name in alone}
    triple = sum(int((ms['regions'][k] & ms['lines'][k] & ms['arrows'][k]).sum()) for k in range(len(base)))
    assert triple > 0                                             # arrow over line over outline on one pixel
    k = 3
    both = ms['regions'][k] & ms['lines'][k] & ms['arrows'][k]
    assert np.array_equal(O.luma(fmt, whole[k])[both], O.luma(fmt, alone['arrows'][k])[both])
    assert flags.tolist() == [0] * len(D.ROWS) and region_flags.tolist() == [0] * 5


def test_within_a_layer_the_higher_index_wins():
    frame = np.zeros((40, 48, 3), np.uint8)
    # two crossing outlines: where they cross, the pixel is the second's (both idle: the same colour -- so one is looked at)
    rows = dict(boxes=[[14, 10, 34, 30]] * 2, gaze=[[0.5, -0.25, 0], [-0.5, -0.25, 0]], image_of=[0, 0], mutual=[0, 0], palette=O.PALETTE)
    for order in ([[4, 4, 30, 30], [10, 10, 40, 36]], [[10, 10, 40, 36], [4, 4, 30, 30]]):
        got, _, _, active = draw(frame, kind=[2, 0], target=[1, -1], hit=[[0, 0]] * 2, regions=order, min_thickness=0, line_thickness=0, region_thickness=3, **rows)
        first = draw(frame, kind=[0, 0], target=[-1, -1], hit=[[0, 0]] * 2, regions=order[:1], min_thickness=0, line_thickness=0, region_thickness=3, **rows)[0]
        second = draw(frame, kind=[2, 0], target=[0, -1], hit=[[0, 0]] * 2, regions=order[1:], min_thickness=0, line_thickness=0, region_thickness=3, **rows)[0]
        cross = first.any(axis=2) & second.any(axis=2)
        assert cross.sum() > 0 and (got[cross] == O.PALETTE[6]).all() and (got[first.any(axis=2) & ~cross] == O.PALETTE[5]).all()
        assert active.tolist() == [[0, 1]]
    # two crossing arrows of different colours (kind 1 and 3), two crossing sight lines
    for kinds in ([1, 3], [3, 1]):
        got = draw(frame, kind=kinds, target=[1, -1], hit=[[0, 0]] * 2, line_thickness=0, min_thickness=3, **rows)[0]
        a = draw(frame, kind=kinds[:1], target=[-1], hit=[[0, 0]], line_thickness=0, min_thickness=3, **{k: v[:1] if k != 'palette' else v for k, v in rows.items()})[0]
        b = draw(frame, kind=kinds[1:], target=[-1], hit=[[0, 0]], line_thickness=0, min_thickness=3, **{k: v[1:] if k != 'palette' else v for k, v in rows.items()})[0]
        cross = a.any(axis=2) & b.any(axis=2)
        assert cross.sum() > 0 and (got[cross] == O.PALETTE[kinds[1]]).all()
    got = draw(frame, kind=[1, 2], target=[1, 0], hit=[[40, 4], [4, 6]], line_thickness=3, min_thickness=0, regions=[[0, 0, 2, 2]], region_thickness=0,
               **dict(rows, boxes=[[0, 0, 16, 16], [30, 0, 46, 16]]))[0]       # (8, 8) -> (40, 4) and (38, 8) -> (4, 6) cross
    one = draw(frame, kind=[1], target=[0], hit=[[40, 4]], line_thickness=3, min_thickness=0, boxes=[[0, 0, 16, 16]], gaze=[[0, 0, 0]], image_of=[0], mutual=[0], palette=O.PALETTE)[0]
    two = draw(frame, kind=[2], target=[0], hit=[[4, 6]], line_thickness=3, min_thickness=0, boxes=[[30, 0, 46, 16]], gaze=[[0, 0, 0]], image_of=[0], mutual=[0], palette=O.PALETTE)[0]
    cross = one.any(axis=2) & two.any(axis=2)
    assert cross.sum() > 0 and (got[cross] == O.PALETTE[2]).all() and (got[one.any(axis=2) & ~cross] == O.PALETTE[1]).all()


def test_every_palette_index_is_reached():
    frame = np.zeros((40, 48, 3), np.uint8)
    seen = set()
    for kind, mutual, index in ((0, 0, 0), (1, 0, 1), (2, 0, 2), (3, 0, 3), (1, 1, 4), (3, 5, 4), (0, -1, 4), (7, 0, 0), (-1, 0, 0), (4, 0, 0), (2 ** 31 - 1, 0, 0)):
        got = draw(frame, [[14, 10, 34, 30]], [[0.5, -0.25, 0]], [0], [kind], [0], [[2, 2]], [mutual], palette=O.PALETTE, line_thickness=0)[0]
        colours = {tuple(c) for c in got[got.any(axis=2)]}
        assert colours == {tuple(O.PALETTE[index])}, (kind, mutual)
        seen.add(index)
    for looked, index in ((False, 5), (True, 6)):
        got = draw(frame, [[14, 10, 34, 30]], [[0.5, -0.25, 0]], [0], [2 if looked else 1], [0], [[2, 2]], [0], regions=[[4, 4, 30, 30]], palette=O.PALETTE,
                   line_thickness=0, min_thickness=0)[0]
        assert {tuple(c) for c in got[got.any(axis=2)]} == {tuple(O.PALETTE[index])}
        seen.add(index)
    assert seen == set(range(7))
    yuv = draw(O.frames('nv12')[3], [[14, 10, 34, 30]], [[0.5, -0.25, 0]], [0], [3], [0], [[2, 2]], [0], palette=O.PALETTE, pixel_format='nv12', matrix='bt709')[0]
    changed = yuv[0] != O.frames('nv12')[3][0]
    assert set(yuv[0][changed].tolist()) <= {int(AR.bgr_to_yuv(O.PALETTE[3], 'bt709')[0])}


@pytest.mark.parametrize('period', [0, 2])
def test_region_active_against_a_plain_double_loop(period):
    shapes = [(40, 48), (18, 22), (12, 16), (40, 48)]
    case = O.random_case(31 + period, 90, 12, shapes, period=period)
    case['image_of'][:5] = [-1, 4, 7, -3, 100]                     # rows outside the table light nothing
    case['target'][5:9] = [-1, 12, 99, -7]
    _, flags, _, active = draw(O.blank('bgr', shapes), **case)
    want = np.zeros((4, 12), np.int32)
    for p in range(4):
        for j in range(12):
            want[p, j] = int(any(case['image_of'][k] == p and case['kind'][k] == 2 and case['target'][k] == j for k in range(90)))
    assert np.array_equal(active, want) and active.dtype == np.int32 and want.sum() > 4 and flags[:5].tolist() == [2] * 5


def test_region_image_of_every_picture_one_picture_and_a_period():
    shapes = [(18, 22), (18, 22), (18, 22), (18, 22)]
    frames = [np.zeros((18, 22, 3), np.uint8) for _ in shapes]
    none = dict(boxes=np.zeros((0, 4)), gaze=np.zeros((0, 3)), image_of=[], kind=[], target=[], hit=np.zeros((0, 2)), mutual=[], regions=[[3, 3, 15, 12]])
    drawn = lambda **kw: [bool(f.any()) for f in draw(frames, **none, **kw)[0]]
    assert drawn(region_image=[-1]) == [True] * 4 and drawn(region_image=[-5]) == [True] * 4 and drawn() == [True] * 4
    assert drawn(region_image=[2]) == [False, False, True, False]
    assert drawn(region_image=[1], region_period=2) == [False, True, False, True]
    assert drawn(region_image=[0], region_period=3) == [True, False, False, True]
    assert drawn(region_image=[3], region_period=2) == [False, False, False, True]      # equal to the picture itself
    assert drawn(region_image=[9]) == [False] * 4
    # one region on pictures of different size: bounded by each picture's own h, w
    mixed = [np.zeros((h, w, 3), np.uint8) for h, w in D.SHAPES]
    got = draw(mixed, **dict(none, regions=[[1, 1, 30, 30]]), region_thickness=1)[0]
    assert [int(g.any(axis=2).sum()) for g in got] == [11 + 15 - 1, 17 + 21 - 1, 2 - 1, 4 * 29]


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_unusable_regions_leave_the_bytes_and_flag_2(fmt, matrix):
    regions, region_image, names = O.unusable_regions()
    frames = O.frames(fmt)[3:]
    none = dict(boxes=np.zeros((0, 4)), gaze=np.zeros((0, 3)), image_of=[], kind=[], target=[], hit=np.zeros((0, 2)), mutual=[], pixel_format=fmt, matrix=matrix)
    got, _, region_flags, _ = draw(frames, regions=regions, region_image=region_image, **none)
    assert region_flags.tolist() == O.UNUSABLE_FLAGS, names
    usable = [j for j, f in enumerate(O.UNUSABLE_FLAGS) if f == 0]
    xy, start = regions
    only = AT.region_polygons([xy[start[j]:start[j + 1]].reshape(-1).tolist() if start[j + 1] - start[j] == 2 else xy[start[j]:start[j + 1]].tolist() for j in usable])
    O.same(fmt, got, draw(frames, regions=only, **none)[0], 'only the usable ones draw')
    for j in range(1, len(names) - 1):                            # each unusable one alone: nothing changes
        alone = AT.PolyRegions(xy, np.array([start[j], start[j + 1]], np.int32))
        got, _, f, _ = draw(frames, regions=alone, **none)
        O.same(fmt, got, [tuple(frames[0]) if fmt != 'bgr' else frames[0]], names[j])
        assert f.tolist() == [2], names[j]
    words = O.garbage_offsets(xy, 40)
    got, _, f, _ = draw(frames, regions=AT.PolyRegions(xy, words), **none)
    s, e = words[:-1].astype(np.int64), words[1:].astype(np.int64)
    assert (f[~((0 <= s) & (s <= e) & (e <= len(xy)))] == 2).all() and (f == 2).sum() >= 30


@pytest.mark.parametrize('fmt,matrix', FORMATS[:2], ids=IDS[:2])
def test_a_bad_hit_drops_the_line_and_keeps_the_arrow(fmt, matrix):
    kw = dict(pixel_format=fmt, matrix=matrix)
    got, flags, _, _ = draw(O.frames(fmt), **O.flag_scene(**kw))
    assert flags.tolist() == D.FLAGS
    # rows 0, 3, 6 are drawable and their hits are NaN, beyond 8191, infinite: exactly their arrows, coloured by kind, and the outlines
    keep = [0, 3, 6]
    want, _, _, _ = draw(O.frames(fmt), **O.flag_scene(line_thickness=0, **kw))
    O.same(fmt, got, want, 'no line')
    arrows = draw(O.frames(fmt), **dict(O.flag_scene(region_thickness=0, **kw), **{k: O.flag_scene()[k][keep] for k in ('boxes', 'gaze', 'image_of', 'kind', 'target', 'hit', 'mutual')}))[0]
    O.same(fmt, arrows, draw(O.frames(fmt), **O.flag_scene(region_thickness=0, **kw))[0], 'flagged rows write nothing')
    good = O.flag_scene(**kw)
    good['hit'] = np.where(np.isfinite(good['hit']) & (np.abs(good['hit']) < 8000), good['hit'], 5).astype(np.float32)
    assert not all(np.array_equal(O.luma(fmt, a), O.luma(fmt, b)) for a, b in zip(draw(O.frames(fmt), **good)[0], got))     # with a hit there IS a line
    with pytest.raises(ValueError):
        draw(O.frames(fmt), strict=True, **O.flag_scene(**kw))


@pytest.mark.parametrize('fmt,matrix', FORMATS, ids=IDS)
def test_the_scalar_restatement_agrees_bit_for_bit(fmt, matrix):
    xy, start = AT.region_polygons(O.REGIONS)
    for kw in (dict(), dict(min_thickness=1, line_thickness=1, region_thickness=1), dict(min_thickness=3, line_thickness=4, region_thickness=5, region_period=2)):
        a = O.scene(matrix=matrix, **kw)
        got = draw(O.frames(fmt), pixel_format=fmt, **a)
        a['regions'] = AT.PolyRegions(xy, start)
        want = O.scalar_overlay(fmt, O.frames(fmt), **a)
        O.same(fmt, got[0], want[0], kw)
        assert all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:])), kw
    shapes = [(18, 22), (12, 16), (18, 22)]
    case = O.random_case(7, 40, 9, shapes, counts=(2, 3, 5, 32), period=2)
    f = O.blank(fmt, shapes)
    got, want = draw(f, pixel_format=fmt, matrix=matrix, **case), O.scalar_overlay(fmt, f, matrix=matrix, **case)
    O.same(fmt, got[0], want[0], 'random')
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
    flagged = O.flag_scene(matrix=matrix, regions=AT.PolyRegions(xy, start))
    got, want = draw(O.frames(fmt), pixel_format=fmt, **flagged), O.scalar_overlay(fmt, O.frames(fmt), **flagged)
    O.same(fmt, got[0], want[0], 'flag rows')
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))


def test_argument_checks_and_limits():
    f = np.zeros((8, 8, 3), np.uint8)
    row = dict(boxes=[[1, 1, 5, 5]], gaze=[[0.5, 0, 0]], image_of=[0], kind=[0], target=[-1], hit=[[0, 0]], mutual=[0])
    draw(f, **row)
    for bad in (dict(line_thickness=-1), dict(region_thickness=256), dict(line_thickness=1.5), dict(min_thickness=256), dict(min_thickness=-1),
                dict(length=float('inf')), dict(palette=[(1, 2, 3)] * 6), dict(palette=[(1, 2, 300)] * 7), dict(region_period=-1),
                dict(kind=[0, 0]), dict(hit=[[0, 0, 0]]), dict(mutual=[]), dict(regions=[[1, 2, 3]]), dict(regions=[[1, 2, 3, 4]], region_image=[0, 1]),
                dict(image_of=[0, 0]), dict(pixel_format='yuv')):
        with pytest.raises(ValueError):
            draw(f, **dict(row, **bad))
    for bad in (dict(kind=[0.5]), dict(target=[1.0]), dict(image_of=[0.0]), dict(region_image=[0.5], regions=[[1, 2, 3, 4]])):
        with pytest.raises(TypeError):
            draw(f, **dict(row, **bad))
    many = lambda n: dict(boxes=np.zeros((n, 4)), gaze=np.zeros((n, 3)), image_of=np.zeros(n, int), kind=np.zeros(n, int), target=np.zeros(n, int),
                          hit=np.zeros((n, 2)), mutual=np.zeros(n, int))
    with pytest.raises(ValueError, match='65535'):
        draw(f, min_thickness=0, **many(65536))
    with pytest.raises(ValueError, match='4096'):
        draw(f, regions=np.zeros((4097, 4)), **row)
    with pytest.raises(ValueError, match='65536'):
        draw(f, regions=AT.PolyRegions(np.zeros((65537, 2), np.float32), np.array([0, 3], np.int32)), **row)
    with pytest.raises(ValueError, match='frames x regions'):
        draw([f] * 257, regions=np.zeros((4096, 4)), **row)
    assert draw(f, strict=False, **dict(row, image_of=[3]))[1].tolist() == [2]
    with pytest.raises(ValueError):
        draw(f, strict=True, **dict(row, image_of=[3]))


def test_header_binding_makefile_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    for name in ('mcg_draw_attention', 'mcg_draw_attention_nv12'):
        assert re.search(r'\bint ' + name + r'\(', hdr) and name in L.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == 32
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20 and '#define MCG_ABI_VERSION 20' in hdr
    for phrase in ('attention overlay (additions to ABI 19; nothing above changes)', 'workspace_bytes >= 96 * (m + 2 n) + 256 * m', 'ANCHOR', 'region_active[p][j]'):
        assert phrase in hdr, phrase
    assert C.sizeof(L.StrokeDesc) == 96 and 'overlay.hip' in open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'Makefile')).read()
    assert os.path.exists(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'overlay.hip'))
    from mcgaze_amd import pipeline as P
    assert P.DevicePipeline.draw_attention is not None and P.draw_attention_host is AR.draw_attention_host
