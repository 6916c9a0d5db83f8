"""Cases for the gaze targets in 3-D (include/mcgaze_hip.h, "gaze targets, 3-D"), shared by tests/test_attention3d_cpu.py and
tests/test_gpu_attention3d.py: scenes worked by hand with the tables they must give written out, edge cases, random tables, and
``targets_scalar``, a second statement of the arithmetic in plain Python floats and loops (no numpy arithmetic) that the numpy twin is
compared with bit for bit.

A case is dict(name=, boxes=, gaze=, image_of=, cam=, and optionally depth=, regions=, region_image=, region_period=, cam_period=,
head_size=, frame=, expand=, camera_angle=, expect=); ``args(case)`` gives the keyword arguments of gaze_targets_3d_host.  ``expect`` names
only the tables (and values) that the scene fixes exactly.

The camera of the hand scenes: fx = fy = 512, (cx, cy) = (320, 240) -- a 640 x 480 picture.  A point (X, Y, Z) is at pixel
(320 + 512 X / Z, 240 + 512 Y / Z).  Gaze convention: frame 'camera' gives D = (-gx, -gy, gz); gz < 0 is towards the lens."""
import math

import numpy as np

from mcgaze_amd import attention as AT
from tests.attention_cases import INF, NAN, f32

OPTION_NAMES = ('depth', 'regions', 'region_image', 'region_period', 'cam_period', 'head_size', 'frame', 'expand', 'camera_angle')
FIELDS = ('kind', 'target', 't', 'hit', 'mutual', 'flags', 'hit3d')
CAM = (512.0, 512.0, 320.0, 240.0)


def box_at(X, Y, Z, side, cam=CAM):
    """The square head box of ``side`` pixels whose centre is the image of (X, Y, Z)."""
    u, v = cam[2] + cam[0] * X / Z, cam[3] + cam[1] * Y / Z
    return (u - side / 2, v - side / 2, u + side / 2, v + side / 2)


def quad(x0, x1, y0, y1, z):
    """A rectangle in the plane z = const, as a region of four vertices."""
    return [[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]]


def case(name, boxes, gaze, image_of=None, cam=CAM, expect=None, **options):
    n = len(boxes)
    c = dict(name=name, boxes=np.asarray(boxes, dtype=np.float32).reshape(n, 4), gaze=np.asarray(gaze, dtype=np.float32).reshape((n, -1) if n else (0, 3)),
             image_of=np.zeros(n, np.int32) if image_of is None else np.asarray(image_of, dtype=np.int32),
             cam=np.asarray(cam, dtype=np.float32).reshape(-1, 4), expect=expect)
    assert not set(options) - set(OPTION_NAMES)
    if options.get('depth') is not None:
        options['depth'] = np.asarray(options['depth'], dtype=np.float32)
    if 'regions' in options and not isinstance(options['regions'], AT.PolyRegions3D):
        options['regions'] = AT.regions_3d(options['regions'])
    if 'region_image' in options:
        options['region_image'] = np.asarray(options['region_image'], dtype=np.int32)
    return dict(c, **options)


def args(c):
    return dict(boxes=c['boxes'], gaze=c['gaze'], image_of=c['image_of'], cam=c['cam'], **{k: c[k] for k in OPTION_NAMES if k in c})


# ---- the scenes of the depth ordering: a viewer V at (-2, 0, 4), a near head N at (0, 0, 2) and a far head F at (0, 0, 6), N and F on ONE
# image ray (the optical axis: both boxes are centred on (320, 240), N's 64 pixels around F's 20).  V's box is centred on (64, 240).
V_BOX, N_BOX, F_BOX = (48, 224, 80, 256), (288, 208, 352, 272), (310, 230, 330, 250)
DEPTH_VNF = (4.0, 2.0, 6.0)
LENS = (0, 0, -1)
SCREEN = quad(0.5, 1.5, -0.5, 0.5, 3.0)                          # a screen at 3 m, right of the axis; its image: [405.33, 576] x [154.67, 325.33]
SCREEN_PX = [[320 + 512 * x / 3, 240 + 512 * y / 3] for x, y, _ in SCREEN]
AXIS_BOX = (304, 224, 336, 256)                                  # 32 pixels around the principal point


def hand_cases():
    """Scenes worked by hand."""
    return [
        # D = (1, 0, 1): (-2 + t, 0, 4 + t) enters F's box [-0.17578125, 0.17578125]^2 x [5.82421875, 6.17578125] at t = 1.82421875
        # (hw = ((10 + 0.25 * 20) * 6) / 512); it never comes near z = 2
        case('depth ordering: gz away from the lens picks the FAR head', [V_BOX, N_BOX, F_BOX], [(-1, 0, 1), LENS, LENS], depth=DEPTH_VNF, frame='camera',
             expect=dict(kind=[1, 3, 3], target=[2, -1, -1], t=[1.82421875, 0, 0], hit3d=[[-0.17578125, 0, 5.82421875], [0, 0, 0], [0, 0, 0]],
                         mutual=[0, 0, 0], flags=[0, 0, 0])),
        # D = (1, 0, -1): (-2 + t, 0, 4 - t) enters N's box [-0.1875, 0.1875]^2 x [1.8125, 2.1875] at t = 1.8125 (hw = ((32 + 16) * 2) / 512)
        case('depth ordering: gz flipped picks the NEAR head', [V_BOX, N_BOX, F_BOX], [(-1, 0, -1), LENS, LENS], depth=DEPTH_VNF, frame='camera',
             expect=dict(kind=[1, 3, 3], target=[1, -1, -1], t=[1.8125, 0, 0], hit3d=[[-0.1875, 0, 2.1875], [0, 0, 0], [0, 0, 0]], mutual=[0, 0, 0],
                         flags=[0, 0, 0])),
        # the same two looks stated relative to the line from the lens to V (frame 'eye'): g = (-D.right, -D.down, D.forward)
        case('depth ordering in the eye frame: the far head', [V_BOX, N_BOX, F_BOX], [(-3, 0, 1), LENS, LENS], depth=DEPTH_VNF,
             expect=dict(kind=[1, 3, 3], target=[2, -1, -1])),
        case('depth ordering in the eye frame: the near head', [V_BOX, N_BOX, F_BOX], [(-1, 0, -3), LENS, LENS], depth=DEPTH_VNF,
             expect=dict(kind=[1, 3, 3], target=[1, -1, -1])),
        # a viewer on the axis at 2 m looks along (1, 0, 1): the plane z = 3 at t = 1, P = (1, 0, 3), inside the screen
        case('a look at a screen lands INSIDE it', [AXIS_BOX], [(-1, 0, 1)], depth=[2.0], regions=[SCREEN], frame='camera',
             expect=dict(kind=[2], target=[0], t=[1.0], hit3d=[[1, 0, 3]], mutual=[0], flags=[0])),
        # (t, 0, 2 + t / 8) meets z = 3 at t = 8: x = 8, far right of the screen -- while its image crosses the screen's image
        case('a look passing in front of the screen misses it', [AXIS_BOX], [(-1, 0, 0.125)], depth=[2.0], regions=[SCREEN], frame='camera',
             expect=dict(kind=[0], target=[-1], t=[0], hit=[[0, 0]], hit3d=[[0, 0, 0]], mutual=[0], flags=[0])),
        case('a look parallel to the screen never meets its plane', [AXIS_BOX], [(-1, 0, 0)], depth=[2.0], regions=[SCREEN], frame='camera',
             expect=dict(kind=[0], target=[-1])),
        case('a look away from the screen: q < 0', [AXIS_BOX], [(1, 0, 1)], depth=[2.0], regions=[quad(-1.5, -0.5, -0.5, 0.5, 1.0)], frame='camera',
             expect=dict(kind=[0], target=[-1])),
        # boxes centred 256 pixels right of the principal point: X = Z / 2.  D = (0, 0, 1) meets the wall z = 10 at t = 10 - Z, x = Z / 2.
        # head_size 0.25: a 64-pixel head is at (512 * 0.25) / 64 = 2 m, a 32-pixel head at 4 m
        case('depth overrides the head size; zero, NaN and negative depth fall back; no size and no depth is flagged',
             [(544, 208, 608, 272)] * 3 + [(560, 224, 592, 256), (576, 240, 576, 240), (576, 240, 576, 240)], [(0, 0, 1)] * 6, image_of=[0, 1, 2, 3, 4, 5],
             cam_period=1, depth=[3.0, 0.0, NAN, -1.0, 5.0, 0.0], head_size=0.25, regions=[quad(-20, 20, -20, 20, 10.0)], frame='camera',
             expect=dict(kind=[2, 2, 2, 2, 2, 0], target=[0, 0, 0, 0, 0, -1], t=[7, 8, 8, 6, 5, 0],
                         hit3d=[[1.5, 0, 10], [1, 0, 10], [1, 0, 10], [2, 0, 10], [2.5, 0, 10], [0, 0, 0]], flags=[0, 0, 0, 0, 0, 2])),
        case('depth None: every row from its head size', [(544, 208, 608, 272), (560, 224, 592, 256), (576, 240, 576, 240)], [(0, 0, 1)] * 3,
             image_of=[0, 1, 2], cam_period=1, head_size=0.25, regions=[quad(-20, 20, -20, 20, 10.0)], frame='camera',
             expect=dict(kind=[2, 2, 0], target=[0, 0, -1], t=[8, 6, 0], flags=[0, 0, 2])),
        # the viewer on the axis at 2 m looks along +z at a head at 6 m: its box starts at z = 6 - ((16 + 8) * 6) / 512 = 5.71875, t = 3.71875;
        # a region IN that plane has the same t: the head wins.  Then two regions in one plane: the lower index.
        case('a head and a region at equal t: the head', [AXIS_BOX, AXIS_BOX], [(0, 0, 1), LENS], depth=[2.0, 6.0], frame='camera',
             regions=[quad(-1, 1, -1, 1, 5.71875)],
             expect=dict(kind=[1, 3], target=[1, -1], t=[3.71875, 0], hit3d=[[0, 0, 5.71875], [0, 0, 0]], hit=[[320, 240], [0, 0]])),
        case('the same region alone is hit', [AXIS_BOX], [(0, 0, 1)], depth=[2.0], frame='camera', regions=[quad(-1, 1, -1, 1, 5.71875)],
             expect=dict(kind=[2], target=[0], t=[3.71875], hit3d=[[0, 0, 5.71875]], hit=[[320, 240]])),
        case('two regions at equal t: the lower index', [AXIS_BOX], [(0, 0, 1)], depth=[2.0], frame='camera',
             regions=[quad(-2, 2, -2, 2, 5.0), quad(-1, 1, -1, 1, 5.0), quad(-1, 1, -1, 1, 4.0)], region_image=[0, 0, 7],
             expect=dict(kind=[2], target=[0], t=[3.0])),
        # (1.5 t', ...) a look back past the lens: D = (0.5, 0, -1) is 26.6 degrees off the line to the lens, so it is not 'the camera'
        case('a hit behind the lens: Pz <= 0 gives a NaN hit', [AXIS_BOX], [(-0.5, 0, -1)], depth=[2.0], frame='camera', regions=[quad(-4, 4, -4, 4, -1.0)],
             expect=dict(kind=[2], target=[0], t=[3.0], hit=[[NAN, NAN]], hit3d=[[1.5, 0, -1]])),
        case('a hit IN the plane of the lens: Pz == 0 gives a NaN hit', [AXIS_BOX], [(-0.5, 0, -1)], depth=[2.0], frame='camera',
             regions=[quad(-4, 4, -4, 4, 0.0)], expect=dict(kind=[2], target=[0], t=[2.0], hit=[[NAN, NAN]], hit3d=[[1, 0, 0]])),
        case('unusable rows: a camera beyond the table, a bad camera', [AXIS_BOX] * 4, [(0, 0, 1)] * 4, image_of=[0, 1, 2, 3],
             cam=[CAM, (NAN, 512, 320, 240), (512, 0, 320, 240)], depth=[2.0] * 4, regions=[quad(-1, 1, -1, 1, 5.0)], frame='camera',
             expect=dict(kind=[2, 0, 0, 0], target=[0, -1, -1, -1], flags=[0, 2, 2, 2])),
        case('cam_period folds the pictures onto the cameras', [AXIS_BOX] * 4, [(0, 0, 1)] * 4, image_of=[0, 1, 2, 3],
             cam=[CAM, (NAN, 512, 320, 240)], cam_period=2, depth=[2.0] * 4, regions=[quad(-1, 1, -1, 1, 5.0)], frame='camera',
             expect=dict(kind=[2, 0, 2, 0], flags=[0, 2, 0, 2])),
        case('n = 0', np.zeros((0, 4)), np.zeros((0, 3)), regions=[SCREEN],
             expect=dict(kind=[], target=[], t=[], hit=np.zeros((0, 2)), mutual=[], flags=[], hit3d=np.zeros((0, 3)))),
        case('two people facing each other across the axis: mutual', [box_at(-1, 0, 4, 32), box_at(1, 0, 4, 32)], [(-1, 0, 0), (1, 0, 0)],
             depth=[4.0, 4.0], frame='camera', expect=dict(kind=[1, 1], target=[1, 0], mutual=[1, 1], t=[1.8125, 1.8125])),
    ]


def unusable_regions_case():
    """Regions that are never hit, written as tables by hand -- three first vertices on one line, 2 vertices, 33 vertices, a NaN vertex,
    offsets of garbage --, and behind them all one good wall that the look reaches."""
    wall = lambda z: quad(-1, 1, -1, 1, z)
    parts = [[[-1, -1, 3.0], [0, 0, 3.0], [1, 1, 3.0], [-1, 1, 3.0]],                    # 0: v0, v1, v2 on one line
             wall(3.25)[:2],                                                             # 1: 2 vertices
             [[math.cos(k), math.sin(k), 3.5] for k in range(33)],                       # 2: 33 vertices
             [[-1, -1, 3.75], [1, -1, 3.75], [1, 1, NAN], [-1, 1, 3.75]],                 # 3: a NaN vertex (not among the first three)
             wall(4.0), wall(4.25), wall(4.5),                                           # 4, 5, 6: their offsets are garbage below
             wall(5.0)]                                                                  # 7: usable
    xyz = np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])
    start = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=start[1:])
    start = start.astype(np.int32)
    V = len(xyz)
    # region 4 ends where region 5 is made to begin: before its own start; region 5 begins below zero; region 6 begins beyond the table
    words = start.copy()
    words[5], words[6] = -3, V + 100
    return case('unusable regions are never hit', [AXIS_BOX], [(0, 0, 1)], depth=[2.0], frame='camera', regions=AT.PolyRegions3D(xyz, words),
                expect=dict(kind=[2], target=[7], t=[3.0], hit3d=[[0, 0, 5.0]]))


def frame_pair():
    """One scene in both frames: the viewer (row 0) is ON the optical axis with Z a power of two, where 'eye' is 'camera' with D scaled by
    Z * Z exactly -- kind, target, hit and hit3d of row 0 are the same bits, t is Z * Z times smaller."""
    boxes = [AXIS_BOX, box_at(1.25, 0.5, 5, 30), box_at(-1, 0.25, 3, 40)]
    gaze = [(-0.25, -0.09375, 1), (0.5, 0, 0.25), (1, 0, -0.125)]
    common = dict(depth=[2.0, 5.0, 3.0], regions=[quad(-3, 3, -2, 2, 9.0)])
    return (case('the viewer on the axis, frame eye', boxes, gaze, frame='eye', **common),
            case('the viewer on the axis, frame camera', boxes, gaze, frame='camera', **common))


def cone_cases():
    """The camera rule in both frames, one degree either side of the 10 degree cone.  frame 'eye': the angle between g and (0, 0, -1).  frame
    'camera': the angle between D and the line from the head at (1, 0.5, 3) back to the lens."""
    out = []
    O = np.array([1.0, 0.5, 3.0])
    back = -O / np.linalg.norm(O)
    side = np.cross(back, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    for degrees, kind in ((9.0, 3), (11.0, 0)):
        a = math.radians(degrees)
        out.append(case(f'eye frame, {degrees} degrees off the lens', [box_at(1, 0.5, 3, 40)], [(math.sin(a), 0, -math.cos(a))], depth=[3.0],
                        expect=dict(kind=[kind])))
        D = math.cos(a) * back + math.sin(a) * side
        out.append(case(f'camera frame, {degrees} degrees off the line to the lens', [box_at(1, 0.5, 3, 40)], [(-D[0], -D[1], D[2])], depth=[3.0],
                        frame='camera', expect=dict(kind=[kind])))
    return out


def edge_cases():
    """No expected tables: the numpy twin, the scalar restatement and the kernel have to agree."""
    tiny = np.float32(1e-42)                                      # a denormal f32
    return [
        case('a gaze of denormal magnitude', [V_BOX, N_BOX, F_BOX], [(-tiny, 0, tiny), (tiny, tiny, 0), (0, 0, -tiny)], depth=DEPTH_VNF),
        case('no gaze at all, in both frames', [V_BOX, N_BOX], [(0, 0, 0), (-0.0, 0, 0)], depth=[4.0, 2.0], frame='camera'),
        case('large coordinates, a huge head size and a large expand', [(-3e38, 0, 3e38, 10), N_BOX, V_BOX], [(-1, 0, 1), (1, 0, 0), (-1, -1e-3, 0)],
             head_size=1e300, expand=1e300),
        case('a wide row table: gaze [n, 5]', [V_BOX, N_BOX, F_BOX], [(-1, 0, 1, 9, 9), (0, 0, -1, 9, 9), (1, 1, 0, 9, 9)], depth=DEPTH_VNF),
        case('boxes without area at a given depth', [(5, 5, 5, 5), (5, 5, 5, 5), (20, 5, 20, 5)], [(-1, 0, 0), (1, 0, 0), (1, 0, 0)], depth=[2.0, 2.0, 2.0],
             expand=0.0, frame='camera'),
    ]


def random_case(seed, n, pictures, m, cameras=1, period=0, bad=0.1, stride=3, shuffle=True, counts=(3, 4, 5, 8), depth=True, frame='eye', garbage=0):
    """Integer-pixel boxes in 640 x 480 pictures, depths on a grid of quarter metres (half of them left to the head size), a gaze on a grid
    of multiples of 1/64; planar polygons of ``counts`` vertices scattered through the room.  A share ``bad`` of rows, cameras and regions is
    unusable in one of the ways the header names; ``garbage`` offsets of region_start are random words.  image_of ascending by row, or
    shuffled so that tiles mix pictures; the camera of a row is image_of % cameras."""
    rng = np.random.default_rng(seed)
    side = rng.integers(12, 97, n)
    xy = np.stack([rng.integers(0, 640 - 96, n), rng.integers(0, 480 - 96, n)], axis=1)
    boxes = np.concatenate([xy, xy + np.stack([side, side - rng.integers(0, 9, n)], axis=1)], axis=1).astype(np.float32)
    gaze = (rng.integers(-64, 65, (n, stride)) / 64.0).astype(np.float32)
    lens = rng.random(n) < 0.1
    gaze[:, 2] = np.where(lens, -1.0, gaze[:, 2])
    gaze[lens, :2] *= np.float32(0.125)
    gaze[rng.random(n) < 0.2, 1] = 0.0
    image_of = np.sort(rng.integers(0, pictures, n)).astype(np.int32)
    if shuffle:
        rng.shuffle(image_of)
    d = (rng.integers(4, 33, n) / 4.0).astype(np.float32)
    d[rng.random(n) < 0.5] = 0.0
    for i in np.flatnonzero(rng.random(n) < bad):
        how = rng.integers(0, 6)
        if how == 0:
            boxes[i, rng.integers(0, 4)] = (NAN, INF, -INF)[rng.integers(0, 3)]
        elif how == 1:
            gaze[i, rng.integers(0, 3)] = (NAN, INF)[rng.integers(0, 2)]
        elif how == 2:
            boxes[i, 2] = boxes[i, 0] - 1
        elif how == 3:
            boxes[i, 2:] = boxes[i, :2]
            d[i] = 0.0
        elif how == 4:
            d[i] = (NAN, INF, -2.0)[rng.integers(0, 3)]
        else:
            image_of[i] = -1 - rng.integers(0, 3)
    cam = np.stack([rng.integers(300, 700, cameras), rng.integers(300, 700, cameras), rng.integers(280, 360, cameras), rng.integers(200, 280, cameras)],
                   axis=1).astype(np.float32)
    if cameras > 2:
        cam[rng.integers(0, cameras), rng.integers(0, 4)] = (NAN, INF, -1.0)[rng.integers(0, 3)]
    parts = []
    for j in range(m):
        c = counts[j % len(counts)]
        centre = np.array([rng.integers(-12, 13) / 4.0, rng.integers(-8, 9) / 4.0, rng.integers(4, 33) / 4.0])
        normal = np.array([(0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 0, 1), (1, 1, 2)][rng.integers(0, 5)], dtype=np.float64)
        u = np.cross(normal, (0, 1, 0) if normal[1] == 0 else (1, 0, 0))
        v = np.cross(normal, u)
        u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
        radius = rng.integers(2, 9) / 4.0
        theta = 2 * math.pi * (np.arange(c) + 0.25) / c
        p = centre + radius * (np.cos(theta)[:, None] * u + np.sin(theta)[:, None] * v)
        if rng.integers(0, 2):
            p = p[::-1]                                           # either winding
        p = p.astype(np.float32)
        if rng.random() < bad:
            if rng.integers(0, 2):
                p[rng.integers(0, c), rng.integers(0, 3)] = (NAN, INF)[rng.integers(0, 2)]
            else:
                p[1] = p[0]                                       # e1 = 0: N is all zero
        parts.append(p)
    start = np.zeros(m + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=start[1:])
    start = start.astype(np.int32)
    xyz = np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)
    for j in rng.integers(0, m + 1, garbage):
        start[j] = rng.integers(-2 ** 31, 2 ** 31) if rng.integers(0, 2) else rng.integers(-40, len(xyz) + 40)
    region_image = rng.integers(-1, max(period, pictures), m).astype(np.int32)
    return case(f'random seed {seed}: {n} rows in {pictures} pictures of {cameras} cameras, {m} regions, period {period}, frame {frame}', boxes, gaze,
                image_of, cam=cam, depth=d if depth else None, regions=AT.PolyRegions3D(xyz, start), region_image=region_image, region_period=period,
                cam_period=cameras, head_size=0.25, frame=frame)


def all_cases():
    return hand_cases() + [unusable_regions_case()] + list(frame_pair()) + cone_cases() + edge_cases() + [
        random_case(1, 40, 3, 6), random_case(2, 60, 4, 9, cameras=2, period=2, frame='camera'), random_case(3, 33, 1, 0),
        random_case(4, 48, 5, 5, cameras=3, stride=5, shuffle=False, depth=False), random_case(5, 50, 2, 12, garbage=4, frame='camera')]


# ---------------------------------------------------------------- the arithmetic a second time: plain Python floats, loops, no numpy arithmetic
def sqrtf(x):
    """(double)sqrtf((float)x): the double square root of an f32 rounded to f32 is the correctly rounded f32 square root."""
    x = f32(x)
    return f32(math.sqrt(x)) if x >= 0.0 else NAN


def div(a, b):
    """IEEE division, where Python raises."""
    if b == 0.0:
        return NAN if a == 0.0 or a != a else math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def targets_scalar(boxes, gaze, image_of, cam, depth=None, regions=None, region_image=None, region_period=0, cam_period=0, head_size=0.24,
                   frame='eye', expand=0.25, camera_angle=10.0):
    """The header's rules row by row -> dict of lists (t, hit and hit3d already rounded to f32)."""
    boxes = [[float(v) for v in row] for row in np.asarray(boxes, dtype=np.float32).reshape(-1, 4).tolist()]
    n = len(boxes)
    gaze = [[float(v) for v in row[:3]] for row in np.asarray(gaze, dtype=np.float32).reshape((n, -1) if n else (0, 3)).tolist()]
    image_of = [int(v) for v in image_of]
    cam = [[float(v) for v in row] for row in np.asarray(cam, dtype=np.float32).reshape(-1, 4).tolist()]
    depth = None if depth is None else [float(v) for v in np.asarray(depth, dtype=np.float32).tolist()]
    if regions is None:
        xyz, start = [], [0]
    else:
        xyz = [[float(v) for v in row] for row in np.asarray(regions.xyz, dtype=np.float32).tolist()]
        start = [int(v) for v in regions.start]
    m = len(start) - 1
    region_image = [-1] * m if region_image is None else [int(v) for v in region_image]
    cos2 = 2.0 if camera_angle is None else math.cos(math.radians(camera_angle)) ** 2
    fin = math.isfinite
    rows = []                                                     # per row: None, or (fx, fy, cx, cy, X, Y, Z)
    for i in range(n):
        (x1, y1, x2, y2), g = boxes[i], gaze[i]
        rows.append(None)
        if not (all(fin(v) for v in boxes[i]) and all(fin(v) for v in g) and not x2 < x1 and not y2 < y1 and image_of[i] >= 0):
            continue
        c = image_of[i] % cam_period if cam_period > 0 else image_of[i]
        if c >= len(cam):
            continue
        fx, fy, cx, cy = cam[c]
        if not (fin(fx) and fin(fy) and fin(cx) and fin(cy) and fx > 0.0 and fy > 0.0):
            continue
        if depth is not None and fin(depth[i]) and depth[i] > 0.0:
            Z = depth[i]
        else:
            w, h = x2 - x1, y2 - y1
            Z = div(fx * head_size, w if w > h else h)
        if not (fin(Z) and Z > 0.0):
            continue
        X, Y = ((((x1 + x2) * 0.5) - cx) * Z) / fx, ((((y1 + y2) * 0.5) - cy) * Z) / fy
        if fin(X) and fin(Y):
            rows[i] = (fx, fy, cx, cy, X, Y, Z)
    good = []                                                     # per region: None, or (N, axis, vertices)
    for j in range(m):
        s, e = start[j], start[j + 1]
        good.append(None)
        if not (0 <= s <= e <= len(xyz) and 3 <= e - s <= 32):
            continue
        v = xyz[s:e]
        if not all(fin(x) for p in v for x in p):
            continue
        e1, e2 = [v[1][a] - v[0][a] for a in range(3)], [v[2][a] - v[0][a] for a in range(3)]
        N = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        if N[0] == 0.0 and N[1] == 0.0 and N[2] == 0.0:
            continue
        ax, ay, az = abs(N[0]), abs(N[1]), abs(N[2])
        good[j] = (N, 0 if ax >= ay and ax >= az else 1 if ay >= az else 2, v)
    out = dict(kind=[0] * n, target=[-1] * n, t=[0.0] * n, hit=[[0.0, 0.0] for _ in range(n)], mutual=[0] * n,
               flags=[0 if r is not None else 2 for r in rows], hit3d=[[0.0, 0.0, 0.0] for _ in range(n)])
    for i in range(n):
        if rows[i] is None:
            continue
        fx, fy, cx, cy, X, Y, Z = rows[i]
        gx, gy, gz = gaze[i]
        if frame == 'camera':
            D = (-gx, -gy, gz)
            s = -((D[0] * X + D[1] * Y) + D[2] * Z)
            lens = s > 0.0 and s * s >= cos2 * (((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]) * ((X * X + Y * Y) + Z * Z))
        else:
            a2 = X * X + Z * Z
            a, r = sqrtf(a2), sqrtf(a2 + Y * Y)
            p, q = gx * r, gz * a
            D = (((q * X) - (p * Z)) + (gy * (X * Y)), (q * Y) - (gy * a2), ((q * Z) + (p * X)) + (gy * (Y * Z)))
            lens = gz < 0.0 and gz * gz >= cos2 * ((gx * gx + gy * gy) + gz * gz)
        if lens:
            out['kind'][i] = 3
            continue
        if not all(fin(v) for v in D) or (D[0] == 0.0 and D[1] == 0.0 and D[2] == 0.0):
            continue
        O = (X, Y, Z)
        best = None                                               # (t, kind, index)
        for j in range(n):
            if j == i or rows[j] is None or image_of[j] != image_of[i]:
                continue
            jfx, jfy, _, _, jX, jY, jZ = rows[j]
            a1, b1, a2_, b2 = boxes[j]
            w, h = a2_ - a1, b2 - b1
            e = expand * (w if w > h else h)
            hw, hh = (((w * 0.5) + e) * jZ) / jfx, (((h * 0.5) + e) * jZ) / jfy
            half = (hw, hh, hw if hw > hh else hh)
            near, far, ok = -INF, INF, True
            for a, oj in enumerate((jX, jY, jZ)):
                lo, hi = oj - half[a], oj + half[a]
                if D[a] == 0.0:
                    ok = ok and lo <= O[a] <= hi
                    continue
                t1, t2 = (lo - O[a]) / D[a], (hi - O[a]) / D[a]
                l, u = (t1, t2) if t1 < t2 else (t2, t1)
                near, far = (l if l > near else near), (u if u < far else far)
            t = near if near > 0.0 else 0.0
            if ok and near <= far and far >= 0.0 and fin(t) and (best is None or t < best[0]):
                best = (t, 1, j)
        for j in range(m):
            ri = region_image[j]
            applies = ri < 0 or (ri == image_of[i] % region_period if region_period > 0 else ri == image_of[i])
            if not applies or good[j] is None:
                continue
            N, axis, v = good[j]
            den = (N[0] * D[0] + N[1] * D[1]) + N[2] * D[2]
            tn = (N[0] * (v[0][0] - X) + N[1] * (v[0][1] - Y)) + N[2] * (v[0][2] - Z)
            if not den != 0.0:
                continue
            q = div(tn, den)
            if not (fin(q) and q >= 0.0):
                continue
            t = q if q > 0.0 else 0.0
            P = (X + t * D[0], Y + t * D[1], Z + t * D[2])
            iu, iv = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
            pu, pv = P[iu], P[iv]
            inside = False
            for k in range(len(v)):
                (au, av), (bu, bv) = (v[k][iu], v[k][iv]), (v[(k + 1) % len(v)][iu], v[(k + 1) % len(v)][iv])
                if (av > pv) != (bv > pv) and pu < au + div((pv - av) * (bu - au), bv - av):
                    inside = not inside
            if inside and (best is None or t < best[0]):
                best = (t, 2, j)
        if best is not None:
            t, out['kind'][i], out['target'][i] = best
            P = (X + t * D[0], Y + t * D[1], Z + t * D[2])
            out['t'][i], out['hit3d'][i] = f32(t), [f32(v) for v in P]
            u, v = fx * div(P[0], P[2]) + cx, fy * div(P[1], P[2]) + cy
            out['hit'][i] = [f32(w) if P[2] > 0.0 and w == w else NAN for w in (u, v)]
    for i in range(n):
        r = out['target'][i]
        out['mutual'][i] = int(out['kind'][i] == 1 and out['kind'][r] == 1 and out['target'][r] == i)
    return out


DTYPES = dict(kind=np.int32, target=np.int32, t=np.float32, hit=np.float32, mutual=np.int32, flags=np.int32, hit3d=np.float32)
WIDTH = dict(hit=2, hit3d=3)


def as_table(name, values):
    n = len(values)
    a = np.asarray(values, dtype=DTYPES[name]).reshape((n, WIDTH[name]) if name in WIDTH else (n,))
    if a.dtype == np.float32:
        a = np.where(a != a, AT.NAN32, a)                         # the one NaN the entry writes
    return a


def as_tables(d):
    """A dict of lists (targets_scalar) -> the seven arrays in the dtypes the kernel writes."""
    return tuple(as_table(k, d[k]) for k in FIELDS)


def same_tables(got, want, what):
    """Bit for bit, all seven."""
    assert len(got) == len(want) == len(FIELDS), (what, len(got), len(want))
    for name, a, b in zip(FIELDS, got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, a.shape, b.dtype, b.shape)
        same = a.view(np.int32) == b.view(np.int32)
        assert same.all(), (what, name, np.argwhere(~same)[:5].tolist(), a[~same][:5].tolist(), b[~same][:5].tolist())


def check_expect(got, case):
    """The tables a hand case fixes, bit for bit."""
    for name, values in (case.get('expect') or {}).items():
        a, b = np.ascontiguousarray(got[FIELDS.index(name)]), as_table(name, values)
        assert a.dtype == b.dtype and a.shape == b.shape, (case['name'], name, a.shape, b.shape)
        assert (a.view(np.int32) == b.view(np.int32)).all(), (case['name'], name, a.tolist(), b.tolist())
