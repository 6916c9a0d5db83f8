"""arrows.anonymize_plan_host / anonymize_heads_host, the numpy twin of mcg_anonymize_heads (include/mcgaze_hip.h, "anonymised heads"), on the
CPU: against a scalar restatement pixel by pixel, against frames worked by hand, and the properties the header states.  Every comparison is
array_equal."""
import numpy as np
import pytest

from mcgaze_amd import arrows as AR
from tests import anonymize_cases as AC


def test_a_4x6_bgr_frame_worked_by_hand():
    idx = np.arange(24).reshape(4, 6)
    frame = np.stack([idx, 100 + 2 * idx, 255 - 3 * idx], axis=2).astype(np.uint8)
    # box (1, 1, 3, 3) as it is: the integer rectangle [1, 3) x [1, 3), cells of 2 x 2 (shift 1) -- each covered pixel lies in another cell
    out, flags = AR.anonymize_heads_host(frame, [[1, 1, 3, 3]], expand=0, shape='box', cell=2)
    want = frame.copy()
    want[1, 1] = (4, 107, 245)      # cell (0, 0), idx 0 1 6 7:     (14 + 2) // 4, (428 + 2) // 4, (978 + 2) // 4
    want[1, 2] = (6, 111, 239)      # cell (1, 0), idx 2 3 8 9:     (22 + 2) // 4, (444 + 2) // 4, (954 + 2) // 4
    want[2, 1] = (16, 131, 209)     # cell (0, 1), idx 12 13 18 19: (62 + 2) // 4, (524 + 2) // 4, (834 + 2) // 4
    want[2, 2] = (18, 135, 203)     # cell (1, 1), idx 14 15 20 21: (70 + 2) // 4, (540 + 2) // 4, (810 + 2) // 4
    assert flags.tolist() == [0] and np.array_equal(out, want)
    plan = AR.anonymize_plan_host([[1, 1, 3, 3]], [0], [(4, 6)], expand=0, shape='box', cell=2)
    assert {k: int(v[0]) for k, v in plan.items()} == dict(image=0, flag=0, x0=1, y0=1, x1=3, y1=3, cx2=4, cy2=4, W=2, H=2, shift=1, shape=0)
    # cells of 4: the cell right of x = 4 is cut to 2 x 4 pixels, idx 4 5 10 11 16 17 22 23 -- (108 + 4) // 8, (1016 + 4) // 8, (1716 + 4) // 8
    out, _ = AR.anonymize_heads_host(frame, [[4, 0, 6, 4]], expand=0, shape='box', cell=4)
    want = frame.copy()
    want[:, 4:] = (14, 127, 215)
    assert np.array_equal(out, want)
    # fill: the colour, whatever the frame held
    out, _ = AR.anonymize_heads_host(frame, [[1, 1, 3, 3]], expand=0, shape='box', mode='fill', color=(9, 8, 7))
    want = frame.copy()
    want[1:3, 1:3] = (9, 8, 7)
    assert np.array_equal(out, want)


def test_a_4x4_nv12_surface_worked_by_hand():
    y = np.array([[1, 4, 7, 10], [17, 20, 23, 26], [33, 36, 39, 42], [49, 52, 55, 58]], dtype=np.uint8)
    uv = np.array([[10, 200, 30, 180], [50, 160, 71, 140]], dtype=np.uint8)
    kw = dict(expand=0, shape='box', pixel_format='nv12')
    # shift 1: four luma cells; every pair has a covered luma pixel and is its own chroma cell (one pair): written with its own value
    (oy, ouv), flags = AR.anonymize_heads_host((y, uv), [[1, 1, 3, 3]], cell=2, **kw)
    want = y.copy()
    want[1, 1], want[1, 2], want[2, 1], want[2, 2] = (42 + 2) // 4, (66 + 2) // 4, (170 + 2) // 4, (194 + 2) // 4      # 11 17 43 49
    assert flags.tolist() == [0] and np.array_equal(oy, want) and np.array_equal(ouv, uv)
    # shift 2: one luma cell, (472 + 8) // 16 = 30; one chroma cell of 2 x 2 pairs, U (161 + 2) // 4 = 40, V (680 + 2) // 4 = 170, for all
    # four pairs, each of which has one covered luma pixel
    (oy, ouv), _ = AR.anonymize_heads_host((y, uv), [[1, 1, 3, 3]], cell=4, **kw)
    want = y.copy()
    want[1:3, 1:3] = 30
    assert np.array_equal(oy, want) and np.array_equal(ouv, np.array([[40, 170, 40, 170]] * 2, dtype=np.uint8))
    # a box over one pair only: the other three keep their bytes
    (oy, ouv), _ = AR.anonymize_heads_host((y, uv), [[2, 0, 4, 2]], cell=4, **kw)
    assert np.array_equal(ouv, np.array([[10, 200, 40, 170], [50, 160, 71, 140]], dtype=np.uint8)) and (oy[:2, 2:] == 30).all()
    # fill with a BGR colour goes through bgr_to_yuv once
    from mcgaze_amd.nv12 import bgr_to_yuv
    yuv = bgr_to_yuv(np.array([10, 200, 90], np.uint8), 'bt709')
    (oy, ouv), _ = AR.anonymize_heads_host((y, uv), [[2, 0, 4, 2]], mode='fill', color=(10, 200, 90), matrix='bt709', **kw)
    assert (oy[:2, 2:] == yuv[0]).all() and ouv[0, 2:].tolist() == [int(yuv[1]), int(yuv[2])] and np.array_equal(ouv[1], uv[1])


@pytest.mark.parametrize('shape', ['box', 'ellipse'])
@pytest.mark.parametrize('mode', ['mosaic', 'fill'])
@pytest.mark.parametrize('cell,blocks', [(None, 8), (None, 1), (4, 8), (64, 8)])
def test_the_twin_equals_the_scalar_restatement(shape, mode, cell, blocks):
    rng = np.random.RandomState(3)
    boxes = [(2.5, 1.25, 13.75, 12.0), (9.0, 6.0, 26.0, 21.5), (-4.0, 14.0, 5.5, 25.0), (20.0, 0.0, 20.5, 3.0), (40.0, 40.0, 50.0, 50.0)]
    kw = dict(expand=0.125, shape=shape, cell=cell, blocks=blocks, mode=mode)
    frame = rng.randint(0, 256, (23, 27, 3)).astype(np.uint8)
    out, flags = AR.anonymize_heads_host(frame, boxes, color=(1, 2, 3), **kw)
    assert not flags.any() and np.array_equal(out, AC.scalar_anonymize(frame, boxes, color=(1, 2, 3), **kw))
    assert not np.array_equal(out, frame)
    y, uv = rng.randint(0, 256, (22, 26)).astype(np.uint8), rng.randint(0, 256, (11, 26)).astype(np.uint8)
    from mcgaze_amd.nv12 import bgr_to_yuv
    (oy, ouv), flags = AR.anonymize_heads_host((y, uv), boxes, color=(1, 2, 3), pixel_format='nv12', **kw)
    wy, wuv = AC.scalar_anonymize((y, uv), boxes, color=tuple(int(v) for v in bgr_to_yuv(np.array([1, 2, 3], np.uint8), 'bt601')), **kw)
    assert not flags.any() and np.array_equal(oy, wy) and np.array_equal(ouv, wuv)


def test_rounding_never_uncovers_a_face():
    """shape='box': every pixel whose unit square meets the float box (grown or not) is covered."""
    rng = np.random.RandomState(11)
    frame = np.full((40, 50, 3), 200, dtype=np.uint8)
    for expand in (0.0, 0.125, 1.0):
        for _ in range(40):
            x1, y1 = rng.uniform(-5, 45), rng.uniform(-5, 35)
            box = np.array([x1, y1, x1 + rng.uniform(0.01, 20), y1 + rng.uniform(0.01, 20)], dtype=np.float32)
            out, flags = AR.anonymize_heads_host(frame, [box], expand=expand, shape='box', mode='fill', color=(0, 0, 0))
            bx1, by1, bx2, by2 = (float(v) for v in box)
            py, px = np.mgrid[0:40, 0:50]
            meets = (px + 1 > bx1) & (px < bx2) & (py + 1 > by1) & (py < by2)
            assert flags.tolist() == [0] and (out[meets] == 0).all(), (box, expand)


def test_where_rows_overlap_the_larger_shift_wins():
    """A head 16 pixels wide gets cells of 2 (8 blocks), one 64 wide cells of 8: where they overlap the cells of 8 show, in either order."""
    frame = np.random.RandomState(5).randint(0, 256, (32, 32, 3)).astype(np.uint8)
    small, large = [4, 4, 20, 20], [12, 12, 76, 76]
    kw = dict(expand=0, shape='box', blocks=8)
    assert AR.anonymize_plan_host([small, large], [0, 0], [(32, 32)], **kw)['shift'].tolist() == [1, 3]
    both, _ = AR.anonymize_heads_host(frame, [small, large], **kw)
    fine, _ = AR.anonymize_heads_host(frame, [small], cell=2, expand=0, shape='box')
    coarse, _ = AR.anonymize_heads_host(frame, [large], cell=8, expand=0, shape='box')
    assert np.array_equal(both[12:, 12:], coarse[12:, 12:])       # under the large box its cells of 8, the overlap included
    assert not np.array_equal(coarse[12:20, 12:20], fine[12:20, 12:20])
    assert np.array_equal(both[4:12, 4:20], fine[4:12, 4:20]) and np.array_equal(both[4:20, 4:12], fine[4:20, 4:12])      # the rest of the small one: cells of 2
    assert np.array_equal(both[:4], frame[:4]) and np.array_equal(both[:, :4], frame[:, :4])
    swapped, _ = AR.anonymize_heads_host(frame, [large, small], **kw)
    assert np.array_equal(swapped, both)                          # the order of the rows does not matter


def test_the_plan_flags_each_unusable_kind():
    sizes = [(70, 134), (0, 10), (9000, 10), (7, 10)]
    rows = [((1, 1, 9, 9), 0, 0), ((np.nan, 1, 9, 9), 0, 2), ((1, 1, np.inf, 9), 0, 2), ((1, -np.inf, 9, 9), 0, 2), ((9, 1, 9, 9), 0, 2), ((9, 1, 1, 9), 0, 2),
            ((1, 9, 9, 9), 0, 2), ((1, 1, 9, 9), -1, 2), ((1, 1, 9, 9), 4, 2), ((1, 1, 9, 9), 1, 2), ((1, 1, 9, 9), 2, 2), ((6000, 1, 8000, 9), 0, 2),
            ((-8191, 1, 9, 8191), 0, 2), ((-6000, 1, 6000, 6000), 0, 0), ((1, 1, 9, 9), 3, 0)]
    boxes, image_of, want = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    plan = AR.anonymize_plan_host(boxes, image_of, sizes)
    assert plan['flag'].tolist() == want
    bad = plan['flag'] == 2
    assert (plan['image'][bad] == -1).all() and all(not plan[k][bad].any() for k in plan if k not in ('image', 'flag'))
    # an NV12 surface of odd size is not writable
    want[-1] = 2
    assert AR.anonymize_plan_host(boxes, image_of, sizes, nv12=True)['flag'].tolist() == want
    # expand = 0 keeps (-8191 .. 8191) inside the bound; a far head gets the largest cells, a near one the smallest
    plan = AR.anonymize_plan_host([(-8191, 1, 9, 8191), (3, 3, 4, 4), (0, 0, 100, 33)], [0, 0, 0], sizes, expand=0)
    assert plan['flag'].tolist() == [0, 0, 0] and plan['shift'].tolist() == [6, 1, 4] and plan['W'].tolist() == [8200, 1, 100]
    assert AR.anonymize_plan_host([(0, 0, 100, 33)], [0], sizes, expand=0, blocks=64)['shift'].tolist() == [1]
    assert AR.anonymize_plan_host([(0, 0, 100, 33)], [0], sizes, expand=0, cell=32)['shift'].tolist() == [5]
    for bad in (dict(expand=-0.1), dict(expand=4.5), dict(expand=float('nan')), dict(shape='disc'), dict(cell=3), dict(cell=128), dict(cell=1), dict(blocks=0),
                dict(blocks=65)):
        with pytest.raises(ValueError):
            AR.anonymize_plan_host([(1, 1, 9, 9)], [0], sizes, **bad)
    with pytest.raises(ValueError):
        AR.anonymize_heads_host(np.zeros((4, 4, 3), np.uint8), [(1, 1, 3, 3)], mode='blur')
