"""Polygonal gaze regions without a GPU (include/mcgaze_hip.h, "gaze targets, polygonal regions"): attention.gaze_targets_host over the vertex
tables against scenes worked by hand and against a second, scalar statement of the rules (tests/attention_poly_cases.py); rectangles given
as 2 vertices against today's form; the exactness property that pins the edge formulas to the slab test; the surface (region_polygons,
PolyRegions, the attention option) and the boundary (exports, header, ABI, the entry's argument checks)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from mcgaze_amd import lib as L
from tests import attention_cases as AC
from tests import attention_poly_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = PC.all_cases()
HAND = PC.hand_cases()
RECT = PC.rectangle_cases()


@pytest.mark.parametrize('case', HAND, ids=[c['name'] for c in HAND])
def test_hand_worked_scenes(case):
    AC.same_tables(AT.gaze_targets_host(**PC.args(case)), AC.as_tables(case['expect']), case['name'])


@pytest.mark.parametrize('polygon', [PC.QUAD, PC.ELL, PC.TRI, PC.SQUARE], ids=['quadrilateral', 'L', 'triangle', 'square'])
def test_winding_and_the_first_vertex_do_not_matter(polygon):
    """The same polygon clockwise and counter-clockwise, and rotated in its vertex list: rays from outside, from inside, through the notch,
    through vertices and along edges give equal tables."""
    boxes = [PC.at(0, 15), PC.at(16, -2), PC.at(140, 20), PC.at(105, 20), PC.at(120, 20), PC.at(0, 0), PC.at(25, 5), PC.at(15, 5)]
    gaze = [PC.RIGHT, (1, -1, 0), PC.LEFT, PC.LEFT, PC.UP, PC.RIGHT, (1, 1, 0), (-0.5, 0.25, 0)]
    image_of = np.arange(len(boxes))                              # one picture each: no head sees another
    want = AT.gaze_targets_host(boxes, gaze, image_of, regions=[polygon])
    assert (want[0] == AT.KIND_REGION).sum() >= 3
    for p in PC.rotations(polygon):
        AC.same_tables(AT.gaze_targets_host(boxes, gaze, image_of, regions=[p]), want, repr(p))


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_numpy_twin_equals_the_scalar_restatement(case):
    got = AT.gaze_targets_host(**PC.args(case))
    assert [a.dtype for a in got] == [np.int32, np.int32, np.float32, np.float32, np.int32, np.int32]
    AC.same_tables(got, AC.as_tables(PC.targets_poly_scalar(**PC.tables(case))), case['name'])


def test_the_random_cases_hold_what_they_are_for():
    """Every kind, rectangles and polygons of 3 .. 32 vertices among the winners, unusable regions, garbage offsets and ties at equal t between
    two regions occur in the random tables, or they would check nothing."""
    seen, ties, sizes, unusable = np.zeros(4, int), 0, set(), 0
    for case in CASES[len(HAND):]:
        a = PC.tables(case)
        kind, target, t, hit, mutual, flags = AT.gaze_targets_host(**a)
        seen += np.bincount(kind, minlength=4)
        xy, start = a['regions']
        ok, first, count = AT._usable_regions(xy.astype(np.float64), start)
        assert ok.any()
        unusable += int((~ok).sum())
        won = np.unique(target[kind == AT.KIND_REGION])
        assert ok[won].all()
        sizes |= set(count[won].tolist())
        for i in np.flatnonzero(kind == AT.KIND_REGION)[:60]:    # the winner made unusable: another candidate enters at the very same t
            s2 = start.copy()
            cut = xy.copy()
            cut[first[target[i]]] = np.nan
            k2, g2, t2, _, _, _ = AT.gaze_targets_host(**dict(a, regions=AT.PolyRegions(cut, s2)))
            ties += int(k2[i] == AT.KIND_REGION and g2[i] != target[i] and t2[i] == t[i])
    assert (seen > 0).all() and ties > 0 and unusable > 4 and {2, 3, 4, 31, 32} <= sizes and len(sizes) > 8, (seen.tolist(), ties, unusable, sorted(sizes))


@pytest.mark.parametrize('name,old,new', RECT, ids=[r[0] for r in RECT])
def test_rectangles_as_two_vertices_give_the_bits_of_todays_form(name, old, new):
    AC.same_tables(AT.gaze_targets_host(**new), AT.gaze_targets_host(**old), name)
    AC.same_tables(AC.as_tables(PC.targets_poly_scalar(**new)), AC.as_tables(AC.targets_scalar(**old)), name + ' (scalar)')


@pytest.mark.parametrize('seed', range(6))
def test_exactness_a_rectangle_as_two_vertices_and_as_four(seed):
    """Boxes with integer corners and odd width and height (origins at .5), region rectangles with integer corners below 2^12, gaze
    components 0 or +- a power of two: every product, difference and quotient of the slab test and of the edge formulas is exact, so the
    rectangle as c == 2 and as 4 vertices in both windings gives bit-equal tables.  Rectangles of width or height 0 (segments) are among
    them.  A rectangle that is one POINT is not: as a polygon all its edges have den == 0 and by the rules it is never hit ("zero-area
    polygons are whatever these rules give" -- hand case 'a polygon without extent is not'), so both sides cannot be zero at once."""
    rng = np.random.default_rng(seed)
    n, m, pictures = 160, 40, 3
    xy1 = rng.integers(0, 4000, (n, 2))
    boxes = np.concatenate([xy1, xy1 + 1 + 2 * rng.integers(0, 30, (n, 2))], axis=1).astype(np.float32)
    power = lambda size: np.where(rng.random(size) < 0.3, 0.0, rng.choice([-1.0, 1.0], size) * 2.0 ** rng.integers(-6, 4, size))
    gaze = np.stack([power(n), power(n), np.where(rng.random(n) < 0.1, -64.0, power(n))], axis=1).astype(np.float32)
    image_of = rng.integers(0, pictures, n).astype(np.int32)
    r1 = rng.integers(0, 4000, (m, 2))
    wh = rng.integers(0, 96, (m, 2))
    wh[(wh == 0).all(axis=1), 0] = 1
    wh[::5] *= 20                                                 # some large ones that hold origins: t = 0
    x1, y1, x2, y2 = r1[:, 0], r1[:, 1], np.minimum(r1[:, 0] + wh[:, 0], 4095), np.minimum(r1[:, 1] + wh[:, 1], 4095)
    region_image = rng.integers(-1, pictures, m).astype(np.int32)
    two = [[a, b, c, d] for a, b, c, d in zip(x1.tolist(), y1.tolist(), x2.tolist(), y2.tolist())]
    four = [[[a, b], [c, b], [c, d], [a, d]] for a, b, c, d in two]
    want = AT.gaze_targets_host(boxes, gaze, image_of, regions=two, region_image=region_image, expand=0.0)
    assert (want[0] == AT.KIND_REGION).sum() > 20 and ((want[0] == AT.KIND_REGION) & (want[2] == 0)).any() and (want[2] > 0).any()
    for what, regions in (('as 2 vertices', AT.region_polygons(two)), ('4 vertices', four), ('4 vertices, the other winding', [p[::-1] for p in four])):
        AC.same_tables(AT.gaze_targets_host(boxes, gaze, image_of, regions=regions, region_image=region_image, expand=0.0), want, what)
    mixed = [four[j][::-1] if j % 3 == 0 else four[j] if j % 3 == 1 else two[j] for j in range(m)]
    AC.same_tables(AT.gaze_targets_host(boxes, gaze, image_of, regions=mixed, region_image=region_image, expand=0.0), want, 'mixed')
    AC.same_tables(AC.as_tables(PC.targets_poly_scalar(boxes, gaze, image_of, regions=AT.region_polygons(mixed), region_image=region_image, expand=0.0)),
                   want, 'mixed (scalar)')


def test_region_polygons():
    xy, start = r = AT.region_polygons([[1, 2, 3, 4], PC.TRI, (5, 6, 7, 8), np.asarray(PC.ELL), np.asarray([9, 9, 9, 9])])
    assert isinstance(r, AT.PolyRegions) and r.xy is xy and r.start is start
    assert xy.dtype == np.float32 and xy.shape == (15, 2) and start.dtype == np.int32 and start.tolist() == [0, 2, 5, 7, 13, 15]
    assert xy[:2].tolist() == [[1, 2], [3, 4]] and xy[2:5].tolist() == [list(map(float, v)) for v in PC.TRI]
    xy, start = AT.region_polygons([])
    assert xy.shape == (0, 2) and start.tolist() == [0]
    xy, start = AT.region_polygons(np.zeros((3, 4)))              # an [m, 4] array: rectangles
    assert xy.shape == (6, 2) and start.tolist() == [0, 2, 4, 6]
    assert AT.region_polygons([[(k, k * k) for k in range(32)]])[1].tolist() == [0, 32]
    assert np.isnan(AT.region_polygons([[0, 0, float('nan'), 1]]).xy[1, 0]) and AT.region_polygons([[4, 4, 1, 1]]).xy.tolist() == [[4, 4], [1, 1]]      # contents
    for bad in (None, 5, 'regions', dict(), [5], [[1, 2, 3, 4], 'abcd'], [['a', 'b', 'c', 'd']], [[True, False, True, False]]):
        with pytest.raises(TypeError):
            AT.region_polygons(bad)
    for bad in ([[1, 2, 3]], [[1, 2, 3, 4, 5]], [[[0, 0], [1, 1]]], [[[0, 0, 0], [1, 1, 1], [2, 2, 2]]], [[(k, k) for k in range(33)]], [[]],
                [[[0, 0], [1, 1], [2]]], [[[[0, 0], [1, 1], [2, 2]]]], [[0, 0, 1, 1]] * (AT.MAX_REGIONS + 1), [PC.ELL * 5] * 2200):
        with pytest.raises(ValueError):
            AT.region_polygons(bad)


def test_the_twin_takes_the_three_forms_and_keeps_its_signature():
    a = PC.args(HAND[0])
    want = AT.gaze_targets_host(**a)
    r = AT.region_polygons(a['regions'])
    AC.same_tables(AT.gaze_targets_host(**dict(a, regions=r)), want, 'PolyRegions')
    AC.same_tables(AT.gaze_targets_host(**dict(a, regions=AT.PolyRegions(r.xy.astype(np.float64).tolist(), r.start.astype(np.int64)))), want, 'other dtypes')
    import torch
    AC.same_tables(AT.gaze_targets_host(**dict(a, regions=AT.PolyRegions(torch.from_numpy(r.xy), torch.from_numpy(r.start)))), want, 'torch')
    sig = inspect.signature(AT.gaze_targets_host)
    assert [p.name for p in sig.parameters.values()] == ['boxes', 'gaze', 'image_of', 'regions', 'region_image', 'region_period', 'expand', 'camera_angle']
    for bad in (AT.PolyRegions(np.zeros((4, 3)), [0, 4]), AT.PolyRegions(np.zeros((4, 2)), [[0, 4]]), AT.PolyRegions(np.zeros((4, 2)), []),
                AT.PolyRegions(np.zeros((AT.MAX_VERTICES + 1, 2)), [0, 3]), AT.PolyRegions(np.zeros((4, 2)), np.zeros(AT.MAX_REGIONS + 2, np.int32))):
        with pytest.raises(ValueError):
            AT.gaze_targets_host(**dict(a, regions=bad))
    with pytest.raises(ValueError):
        AT.gaze_targets_host(**dict(a, regions=r, region_image=[0, 0]))
    with pytest.raises(TypeError):
        AT.gaze_targets_host(**dict(a, regions=AT.PolyRegions(r.xy, r.start.astype(np.float32))))
    assert (AT.MAX_VERTICES, AT.POLY_VERTS) == (65536, 32)


def test_the_attention_option_takes_the_mixed_list():
    rect, opts = [[1, 2, 3, 4], [5, 6, 7, 8]], dict(expand=0.5)
    regions, image, got = AT._attention_options('run_head_video', dict(regions=rect + [PC.TRI], **opts))
    assert isinstance(regions, AT.PolyRegions) and regions.start.tolist() == [0, 2, 4, 7] and regions.xy.shape == (7, 2) and image.tolist() == [-1] * 3
    assert got == opts and regions.xy.dtype == np.float32 and regions.start.dtype == image.dtype == np.int32
    # per camera: the indices count through the cameras' tables in order, rectangles-only tables included
    regions, image, got = AT._attention_options('LiveGaze', dict(regions=[np.asarray(rect), None, [PC.ELL, [9, 9, 10, 10]], [[1, 1, 2, 2]]]), 4)
    assert isinstance(regions, AT.PolyRegions) and regions.start.tolist() == [0, 2, 4, 10, 12, 14] and image.tolist() == [0, 0, 2, 2, 3] and got == {}
    assert regions.xy[4:10].tolist() == [list(map(float, v)) for v in PC.ELL] and regions.xy[12:].tolist() == [[1, 1], [2, 2]]
    # rectangles only: exactly today's tables
    regions, image, got = AT._attention_options('LiveGaze', dict(regions=[rect, None]), 2)
    assert isinstance(regions, np.ndarray) and regions.shape == (2, 4) and image.tolist() == [0, 0]
    for bad in (dict(regions=[PC.TRI[:2]]), dict(regions=[[(0, 0), (1, 1), 'x']]), dict(regions=[[(k, k) for k in range(33)]]), dict(regions=[PC.TRI, 5])):
        with pytest.raises(ValueError):
            AT._attention_options('run_head_video', bad)
        with pytest.raises(ValueError):
            live.LiveGaze(None, None, cameras=1, slots=4, attention=dict(regions=[bad['regions']]))
        with pytest.raises(ValueError):
            harness.run_head_video(None, None, [], boxes_per_frame=[], attention=bad)


def test_header_binding_and_library_agree_on_the_new_entry():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    assert 'mcg_gaze_targets_poly' in L.EXPORTS and re.search(r'\bint mcg_gaze_targets_poly\(', hdr) and hasattr(lib, 'mcg_gaze_targets_poly')
    assert len(lib.mcg_gaze_targets_poly.argtypes) == 20
    declared = re.search(r'\bint mcg_gaze_targets_poly\(([^;]*)\);', hdr).group(1)
    assert len(declared.split(',')) == 20
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20 and '#define MCG_ABI_VERSION 20' in hdr
    assert '#define MCG_ATTEND_POLY_VERTS 32' in hdr
    for phrase in ('gaze targets, polygonal regions', 'USABLE REGION', 'INSIDE (even-odd rule)', 'CROSSINGS', 'Winding does not matter'):
        assert phrase in hdr, phrase
    assert 'polygonal regions, arrows' not in hdr and 'dwell per polygonal region' not in hdr      # no longer out of scope
    rules = open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'check_resources.py')).read()
    assert "'gaze_targets_poly_kernel': dict(scratch=0, vgpr_spill=0, unit='attend')" in rules


def test_the_entry_checks_its_host_arguments_before_any_launch():
    """Counts, strides, parameters and null tables are argument errors; no device is needed to be told so."""
    lib = L.load()
    p = C.c_void_p(256)                                           # never dereferenced: every call below fails its checks first
    ok = dict(n=1, m=1, V=4, stride=3, period=0, expand=0.25, cos2=0.5, boxes=p, xy=p, start=p, image=p)
    call = lambda **kw: (lambda a: lib.mcg_gaze_targets_poly(None, a['boxes'], p, a['stride'], p, a['n'], a['xy'], a['V'], a['start'], a['image'], a['m'],
                                                             a['period'], a['expand'], a['cos2'], p, p, p, p, p, p))(dict(ok, **kw))
    for kw in (dict(n=-1), dict(n=65537), dict(m=-1), dict(m=4097), dict(V=-1), dict(V=65537), dict(stride=2), dict(period=-1), dict(expand=-1.0),
               dict(expand=float('inf')), dict(cos2=float('nan')), dict(boxes=None), dict(xy=None), dict(start=None), dict(image=None)):
        assert call(**kw) != L.MCG_OK, kw
        assert b'mcg_gaze_targets_poly' in lib.mcg_last_error()
    assert call(n=0, boxes=None) == L.MCG_OK                      # n == 0 launches nothing and reads nothing
    assert call(n=0, m=0, V=0, xy=None, start=None, image=None) == L.MCG_OK      # the tables may be null where their count is 0


def test_the_demo_tool_documents_the_mixed_list():
    import importlib.util
    spec = importlib.util.spec_from_file_location('demo_video', os.path.join(ROOT, 'tools', 'demo_video.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert 'polygon [[x, y], [x, y], ...]' in tool.__doc__
