"""Shared by tests/test_draw_cpu.py and tests/test_gpu_draw.py (a helper, not a test): the small frames, the head boxes and gazes, and
answers worked by hand for the arrows of include/mcgaze_hip.h, "annotated frames out".

Frames: the surfaces of tests/nv12_cases.py (12 x 16, 18 x 22 with device pitches 32 / 24, 2 x 2) plus one 40 x 48 frame, as NV12 planes and
as random BGR frames of the same sizes."""
import fractions

import numpy as np

from tests import nv12_cases as N

SHAPES = N.SHAPES + [(40, 48)]
NV12_PITCHES = N.PITCHES + [(64, 48)]                  # (pitch_y, pitch_uv) on the device
BGR_PITCHES = [3 * 16, 3 * 22 + 7, 3 * 2 + 1, 3 * 48 + 16]
NV12_FRAMES = N.FRAMES + [N.planes(23, 40, 48)]
BGR_FRAMES = [np.random.RandomState(40 + k).randint(0, 256, (h, w, 3)).astype(np.uint8) for k, (h, w) in enumerate(SHAPES)]

# (what, image, box x1 y1 x2 y2, gaze g0 g1, shaft (cx, cy) -> (tx, ty)), length 1: cx = int(x1 + x2) // 2, l = int(max side), tip = int(c - l g)
ROWS = [
    # cx = 48 // 2 = 24, cy = 40 // 2 = 20, l = 20: tip (24 - 10, 20 + 5)
    ('interior of the 40x48 frame', 3, (14, 10, 34, 30), (0.5, -0.25), ((24, 20), (14, 25))),
    ('leaves the frame on the left', 3, (14, 10, 34, 30), (1.5, 0.0), ((24, 20), (-6, 20))),
    ('leaves it on the right', 3, (14, 10, 34, 30), (-1.5, 0.25), ((24, 20), (54, 15))),
    ('leaves it at the top', 3, (14, 10, 34, 30), (0.25, 1.5), ((24, 20), (19, -10))),
    ('leaves it at the bottom', 3, (14, 10, 34, 30), (0.0, -1.5), ((24, 20), (24, 50))),
    # centre (110, 110), l = 20: nothing of it is inside a 40 x 48 frame -- flag 0, no pixel
    ('wholly outside', 3, (100, 100, 120, 120), (0.5, 0.5), ((110, 110), (100, 100))),
    # a gaze of zero: the tip is the centre, all three segments have no length -- a disc
    ('no length', 3, (30, 4, 50, 24), (0.0, 0.0), ((40, 14), (40, 14))),
    # cx = 16 // 2 = 8, cy = 12 // 2 = 6, l = 8: tip (8 - 6, 6 - 4); ends on odd and even pixels of the 12 x 16 frame
    ('12x16 frame', 0, (4, 2, 12, 10), (0.75, 0.5), ((8, 6), (2, 2))),
    # cx = int(21.5) // 2 = 10, cy = int(17.0) // 2 = 8, l = int(9.0) = 9: tip (int(10 + 7.2), int(8 - 4.5)) = (17, 3)
    ('pitched 18x22 frame', 1, (6.25, 4.0, 15.25, 13.0), (-0.8, 0.5), ((10, 8), (17, 3))),
    # cx = cy = 1, l = 2: tip (1 - 1, 1 - 1): covers the 2 x 2 frame and more
    ('2x2 frame', 2, (0, 0, 2, 2), (0.5, 0.5), ((1, 1), (0, 0))),
    # two more over row 0's pixels: three arrows overlap around (24, 20)
    ('crosses row 0', 3, (14, 10, 34, 30), (-0.5, -0.25), ((24, 20), (34, 25))),
    ('crosses rows 0 and 10', 3, (12, 12, 32, 32), (0.25, 0.5), ((22, 22), (17, 12))),
]
BOXES = np.array([r[2] for r in ROWS], dtype=np.float32)
GAZE = np.array([r[3] + (0.5,) for r in ROWS], dtype=np.float32)            # [n,3], like a stream's fused gaze: the third component is not read
IMAGE_OF = np.array([r[1] for r in ROWS], dtype=np.int32)
SHAFTS = np.array([r[4] for r in ROWS], dtype=np.int64)
COLORS = np.array([(10 + 20 * k, 250 - 17 * k, (90 + 37 * k) % 256) for k in range(len(ROWS))], dtype=np.uint8)   # one B, G, R per row, all different

# device tables only -- documented inputs that come back with flag 2 and write nothing: a NaN gaze, an infinite box, an image index one past
# the table, a box whose centre (10000, 10000) lies beyond +-8191; usable rows between them
FLAG_BOXES = np.concatenate([BOXES[:1], BOXES[:1], [(0, 0, np.inf, 4)], BOXES[7:8], BOXES[:1], [(0, 0, 20000, 20000)], BOXES[8:9]]).astype(np.float32)
FLAG_GAZE = np.concatenate([GAZE[:1], [(np.nan, 0, 0)], GAZE[:1], GAZE[7:8], GAZE[:1], GAZE[:1], GAZE[8:9]]).astype(np.float32)
FLAG_IMAGE_OF = np.array([3, 3, 3, 0, len(SHAPES), 3, 1], dtype=np.int32)
FLAGS = [0, 2, 2, 0, 2, 2, 0]


def covered_exactly(px, py, a, b, t):
    """Whether pixel (px, py) lies within t / 2 of the segment a -> b, in rationals: the distance to the nearest point a + s (b - a), s the
    projection clamped to [0, 1] -- written from the definition, not from the three-case integer test."""
    F = fractions.Fraction
    ax, ay, bx, by = (F(int(v)) for v in (*a, *b))
    dx, dy = bx - ax, by - ay
    L = dx * dx + dy * dy
    s = F(0) if L == 0 else min(max(((px - ax) * dx + (py - ay) * dy) / L, F(0)), F(1))
    nx, ny = ax + s * dx, ay + s * dy
    return (px - nx) ** 2 + (py - ny) ** 2 <= F(int(t) * int(t), 4)
