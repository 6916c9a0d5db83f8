"""Shared by tests/test_anonymize_cpu.py, tests/test_gpu_anonymize.py and tests/test_gpu_live_anonymize.py (a helper, not a test): frames, head
boxes and a scalar restatement of include/mcgaze_hip.h, "anonymised heads".

Frames: 70 x 134 pixels -- the smallest with more than one 64 x 64 tile in both directions, cut edge tiles, and edge cells whose count is not
a power of two (70 = 64 + 6, 134 = 128 + 6) -- as random BGR frames and NV12 planes, with device pitches that are 16-byte aligned, 4-byte
aligned and odd."""
import numpy as np

H, W = 70, 134
BGR = [np.random.RandomState(70 + k).randint(0, 256, (H, W, 3)).astype(np.uint8) for k in range(3)]
NV12 = [(np.random.RandomState(80 + k).randint(0, 256, (H, W)).astype(np.uint8), np.random.RandomState(90 + k).randint(0, 256, (H // 2, W)).astype(np.uint8))
        for k in range(3)]
BGR_PITCHES = [416, 404, 403]                          # 3 * 134 = 402 bytes a row: 16-byte aligned, 4-byte aligned, odd
NV12_PITCHES = [(144, 144), (136, 140), (135, 137)]    # (pitch_y, pitch_uv): the same three kinds

# (what, image, box x1 y1 x2 y2)
ROWS = [
    ('over the tile corner at (64, 64)', 0, (58.5, 60.0, 71.0, 68.25)),
    ('inside one cell of 8', 0, (33.2, 17.1, 34.5, 18.9)),
    ('two that overlap, the first small', 1, (10.0, 10.0, 30.0, 40.0)),
    ('and the second large: another shift', 1, (20.0, 30.0, 100.0, 60.0)),
    ('half outside, negative coordinates', 1, (-20.5, -10.0, 15.0, 12.0)),
    ('wholly outside', 2, (200.0, 100.0, 230.0, 130.0)),
    ('one pixel wide without expand', 2, (50.0, 40.0, 50.5, 44.0)),
    ('over the right and bottom edges', 2, (120.0, 55.0, 140.0, 75.0)),
    ('the whole frame and more', 0, (-5.0, -5.0, 140.0, 75.0)),
]
BOXES = np.array([r[2] for r in ROWS], dtype=np.float32)
IMAGE_OF = np.array([r[1] for r in ROWS], dtype=np.int32)
SMALL = slice(0, 8)                                    # without the row that covers all of frame 0

# device tables only -- documented contents that come back with flag 2 and write nothing, usable rows between them: NaN, infinite, x2 <= x1,
# y2 <= y1, image_of -1 and one past the table, a rectangle beyond 8191 once grown (8000 + 0.125 * 2000 > 8191)
def flag_rows(images):
    boxes = np.array([BOXES[0], (np.nan, 0, 9, 9), (0, 0, np.inf, 9), BOXES[2], (30, 5, 30, 20), (5, 20, 30, 20), BOXES[0], BOXES[0], (6000, 10, 8000, 20),
                      BOXES[6]], dtype=np.float32)
    image_of = np.array([0, 0, 0, 1, 0, 0, -1, images, 0, 2], dtype=np.int32)
    return boxes, image_of, [0, 2, 2, 0, 2, 2, 2, 2, 2, 0]


def random_rows(n, images, seed=5):
    """n head boxes of mixed sizes over ``images`` frames of 70 x 134, some partly or wholly outside."""
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)
    hw, hh = rng.uniform(0.3, 30, n), rng.uniform(0.3, 30, n)
    return (np.stack([cx - hw, cy - hh, cx + hw, cy + hh], axis=1).astype(np.float32), rng.randint(0, images, n).astype(np.int32))


def scalar_plan(box, h, w, expand, cell, blocks):
    """One usable row's plan in python numbers, from the header's text: (X0, Y0, X1, Y1, shift)."""
    import math
    x1, y1, x2, y2 = (float(np.float32(v)) for v in box)
    ex, ey = expand * (x2 - x1), expand * (y2 - y1)
    X0, X1, Y0, Y1 = math.floor(x1 - ex), math.ceil(x2 + ex), math.floor(y1 - ey), math.ceil(y2 + ey)
    if cell is not None:
        s = cell.bit_length() - 1
    else:
        s = next((c for c in range(1, 7) if (blocks << c) >= max(X1 - X0, Y1 - Y0)), 6)
    return X0, Y0, X1, Y1, s


def scalar_anonymize(frame, boxes, expand=0.125, shape='ellipse', cell=None, blocks=8, mode='mosaic', color=(0, 0, 0)):
    """"anonymised heads" pixel by pixel over ONE frame and usable rows: a BGR array [h, w, 3], or a (y [h, w], uv [h / 2, w]) pair with color
    as (Y, U, V).  Python integers and loops only -- none of the twin's array code."""
    nv12 = isinstance(frame, tuple)
    y = frame[0] if nv12 else frame
    h, w = y.shape[:2]
    plans = [scalar_plan(b, h, w, expand, cell, blocks) for b in boxes]

    def shift_of(px, py):
        top = 0
        for X0, Y0, X1, Y1, s in plans:
            if not (max(X0, 0) <= px < min(X1, w) and max(Y0, 0) <= py < min(Y1, h)):
                continue
            Wd, Hd = X1 - X0, Y1 - Y0
            if shape == 'box' or (2 * px + 1 - X0 - X1) ** 2 * Hd ** 2 + (2 * py + 1 - Y0 - Y1) ** 2 * Wd ** 2 <= Wd ** 2 * Hd ** 2:
                top = max(top, s)
        return top

    def cell_mean(plane, px, py, s, c):
        S = 1 << s
        xs, ys = range(px // S * S, min(px // S * S + S, plane.shape[1])), range(py // S * S, min(py // S * S + S, plane.shape[0]))
        total, count = sum(int(plane[j, i, c]) for j in ys for i in xs), len(xs) * len(ys)
        return (total + (count >> 1)) // count

    top = [[shift_of(px, py) for px in range(w)] for py in range(h)]
    if not nv12:
        out = frame.copy()
        for py in range(h):
            for px in range(w):
                if top[py][px]:
                    out[py, px] = color if mode == 'fill' else [cell_mean(frame, px, py, top[py][px], c) for c in range(3)]
        return out
    luma, pairs = frame[0].reshape(h, w, 1), frame[1].reshape(h // 2, w // 2, 2)
    out_y, out_uv = luma.copy(), pairs.copy()
    for py in range(h):
        for px in range(w):
            if top[py][px]:
                out_y[py, px, 0] = color[0] if mode == 'fill' else cell_mean(luma, px, py, top[py][px], 0)
    for qy in range(h // 2):
        for qx in range(w // 2):
            s = max(top[2 * qy][2 * qx], top[2 * qy][2 * qx + 1], top[2 * qy + 1][2 * qx], top[2 * qy + 1][2 * qx + 1])
            if s:
                out_uv[qy, qx] = color[1:] if mode == 'fill' else [cell_mean(pairs, qx, qy, s - 1, c) for c in range(2)]
    return out_y.reshape(h, w), out_uv.reshape(h // 2, w)
