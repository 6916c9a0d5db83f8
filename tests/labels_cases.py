"""Shared by tests/test_labels_cpu.py and tests/test_gpu_labels.py (a helper, not a test): scenes of text labels over the frames of
tests/draw_cases.py, a second, scalar statement of include/mcgaze_hip.h's "text labels" in plain Python integers, and ``same``."""
import math

import numpy as np

from mcgaze_amd import arrows as R
from tests import draw_cases as D

# (text, image, box x1 y1 x2 y2, place): the frames are 12 x 16, 18 x 22 (pitched), 2 x 2 and 40 x 48 (h x w)
ROWS = [
    ('#7', 3, (5.5, 14.2, 20, 30), 0),            # above the box: Y = 14 - PH
    ('#12 3.4s', 3, (2, 3, 30, 20), 0),           # no room above: below the box, Y = 21, then clamped from the bottom edge
    ('AB', 3, (40, 30, 47, 39), 0),               # clamped at the right edge
    ('SHELF A', 3, (10.9, 22, 44, 38), 1),        # place 1: inside the top-left corner
    ('~', 0, (3, 9, 9, 11), 0),                   # the 12 x 16 frame
    ('a wide plate, wider', 1, (4, 12, 9, 15), 7),  # wider than the 18 x 22 frame: starts at 0, clipped; any place word but 1 is "above"
    ('i', 2, (0, 0, 2, 2), 0),                    # the 2 x 2 frame: a corner of the plate
    ('', 3, (5, 5, 9, 9), 0),                     # an empty label: flag 1
    ('xy', 3, (6, 15, 20, 30), 0),                # overlaps row 0: its plate hides row 0's text
    ('Qg', 3, (100, 100, 120, 120), 0),           # a box wholly outside: the label is moved inside, bottom right
    ('-', 3, (-50.5, -60, -40, -45), 2),          # wholly outside, top left
]
TEXT = R.encode_labels([r[0] for r in ROWS])
IMAGE_OF = np.array([r[1] for r in ROWS], dtype=np.int32)
BOXES = np.array([r[2] for r in ROWS], dtype=np.float32)
PLACE = np.array([r[3] for r in ROWS], dtype=np.int32)
COLORS = np.array([(15 + 21 * k, 240 - 19 * k, (70 + 41 * k) % 256) for k in range(len(ROWS))], dtype=np.uint8)
FLAGS = [1 if not r[0] else 0 for r in ROWS]

# text codes: 0 ends a text; 31, 127 and 255 are drawn as '?'; 32 and 126 are the ends of the font.  Lengths 0, 1, 23 and 24 (no terminator).
CODE_TEXT = np.zeros((6, 24), dtype=np.uint8)
CODE_TEXT[0, :6] = (65, 31, 32, 126, 127, 255)
CODE_TEXT[1, :4] = (66, 67, 0, 68)                # cut at the zero: 'BC'
CODE_TEXT[3, 0] = 33                              # row 2 has length 0
CODE_TEXT[4, :23] = np.arange(40, 63)
CODE_TEXT[5] = np.arange(97, 121)
CODE_LENGTHS = [6, 2, 0, 1, 23, 24]

# device tables only -- rows that come back with flag 2 and write nothing, usable rows between them: an infinite and a NaN box, a box beyond
# +-8191, an image index one past the table and a negative one
FLAG_BOXES = np.array([(5, 14, 20, 30), (0, 0, np.inf, 4), (np.nan, 1, 2, 3), (2, 3, 30, 20), (0, 0, 8192.5, 4), (0, -8192, 5, 4), (0, 0, 8191.9, 4),
                       (5, 5, 9, 9), (5, 5, 9, 9)], dtype=np.float32)
FLAG_IMAGE_OF = np.array([3, 3, 3, 0, 3, 3, 3, len(D.SHAPES), -1], dtype=np.int32)
FLAG_TEXT = R.encode_labels(['ok', 'inf', 'nan', 'fine', 'far', 'far', 'edge', 'past', 'neg'])
FLAG_FLAGS = [0, 2, 2, 0, 2, 2, 0, 2, 2]


def random_tables(seed, n, sizes, flags=True):
    """Random label rows over frames of ``sizes``, boxes around and beyond the frames; with ``flags`` some rows of every flag."""
    rs = np.random.RandomState(seed)
    boxes = rs.uniform(-30, 70, (n, 4)).astype(np.float32)
    boxes[:, 2:] = boxes[:, :2] + rs.uniform(0, 30, (n, 2)).astype(np.float32)
    image_of = rs.randint(0, len(sizes), n).astype(np.int32)
    text = rs.randint(1, 256, (n, 24)).astype(np.uint8)
    for k in range(n):
        text[k, rs.randint(0, 25):] = 0
    place = rs.randint(0, 3, n).astype(np.int32)
    if flags:
        boxes[rs.randint(0, n)] = (1, 2, np.nan, 4)
        boxes[rs.randint(0, n)] = (1, 2, 9000, 4)
        image_of[rs.randint(0, n)] = len(sizes)
        text[rs.randint(0, n)] = 0
    return boxes, image_of, text, place


def scalar_labels(sizes, boxes, image_of, text, place, scale, advance, pad, font, nv12=False, background=True):
    """"text labels" once more, a pixel and a row at a time in Python integers -> (winner: one int array [h, w] per frame holding the highest
    stroke over each pixel, -1 for none; flags).  Written from the header, not from arrows.py: no numpy arithmetic on the way."""
    winner = [np.full((h, w), -1, dtype=np.int64) for h, w in sizes]
    flags = []
    for k in range(len(boxes)):
        b = [float(np.float32(v)) for v in boxes[k]]
        io = int(image_of[k])
        usable = 0 <= io < len(sizes) and all(math.isfinite(v) for v in b)
        if usable:
            h, w = (int(v) for v in sizes[io])
            usable = h > 0 and w > 0 and h <= 8192 and w <= 8192 and not (nv12 and (h % 2 or w % 2))
        if usable:
            bx1, by1, bx2, by2 = (int(v) for v in b)                 # int() truncates
            usable = all(-8191 <= v <= 8191 for v in (bx1, by1, bx2, by2))
        if not usable:
            flags.append(2)
            continue
        codes = [int(c) for c in text[k]]
        length = codes.index(0) if 0 in codes else 24
        if length == 0:
            flags.append(1)
            continue
        flags.append(0)
        P = pad * scale
        TW, TH = length * advance * scale, 8 * scale
        PW, PH = TW + 2 * P, TH + 2 * P
        X, Y = bx1, by1
        if int(place[k]) != 1:
            Y = by1 - PH
            if Y < 0:
                Y = by2 + 1
        X, Y = max(0, min(X, w - PW)), max(0, min(Y, h - PH))
        for py in range(Y, min(Y + PH, h)):
            for px in range(X, min(X + PW, w)):
                if background:
                    winner[io][py, px] = 2 * k
                fx, fy = px - (X + P), py - (Y + P)
                if 0 <= fx < TW and 0 <= fy < TH:
                    c = codes[fx // (advance * scale)]
                    g = c - 32 if 32 <= c <= 126 else 31
                    if (int(font[g][fy // scale]) >> ((fx % (advance * scale)) // scale)) & 1:
                        winner[io][py, px] = 2 * k + 1
    return winner, flags


def paint(frames, winner, fg, bg, nv12=False):
    """The frames with the strokes of ``winner`` painted: an odd stroke 2 k + 1 in fg[k], an even one in bg (triples in the planes' own
    format) -- pixel by pixel, the NV12 chroma pair from the highest stroke among its four luma pixels."""
    out = []
    for f, win in zip(frames, winner):
        colour = lambda s: fg[s >> 1] if s & 1 else bg
        if not nv12:
            a = np.array(f)
            for py, px in zip(*np.nonzero(win >= 0)):
                a[py, px] = colour(int(win[py, px]))
            out.append(a)
            continue
        y, uv = np.array(f[0]), np.array(f[1]).reshape(f[0].shape[0] // 2, -1)
        for py, px in zip(*np.nonzero(win >= 0)):
            y[py, px] = colour(int(win[py, px]))[0]
        for cy in range(y.shape[0] // 2):
            for cx in range(y.shape[1] // 2):
                top = int(win[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2].max())
                if top >= 0:
                    uv[cy, 2 * cx:2 * cx + 2] = colour(top)[1:]
        out.append((y, uv))
    return out


def same(fmt, got, want, what=''):
    """Frames as numpy (BGR arrays, NV12 (y, uv) pairs), bit for bit."""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        if fmt == 'bgr':
            assert g.shape == w.shape and np.array_equal(g, w), (what, k)
        else:
            assert np.array_equal(g[0], w[0]) and np.array_equal(np.asarray(g[1]).reshape(w[0].shape[0] // 2, -1), np.asarray(w[1]).reshape(w[0].shape[0] // 2, -1)), (what, k)
