"""Shared by tests/test_heat_cpu.py and tests/test_gpu_heat.py (a helper, not a test): the scenes of include/mcgaze_hip.h, "gaze heat map".

Frames.  tests.test_gpu_draw's host_frames / device_frames serve the fixed frames of tests/draw_cases.py (12 x 16, 18 x 22, 2 x 2, 40 x 48) and
cannot be given other sizes, so the GPU test runs over those through the imported helpers AND over the frames made here, built the same way:
BGR pictures of 37 x 53 with pitches of 163 (odd), 164 (a multiple of 4) and 160 (a multiple of 16) bytes -- one picture per access path of
the render kernel -- and one of 20 x 300 that crosses a tile in x; NV12 surfaces of 38 x 54 and 20 x 300 likewise.  Four pictures: with
period 2 they show cameras 0, 1, 0, 1; with period 0 pictures 2 and 3 have no grid (C = 2) and must come back untouched."""
import numpy as np

C = 2
PERIOD = 2
FRAME_HW = (37, 53)
SHAPES = {'bgr': [(37, 53), (37, 53), (37, 53), (20, 300)], 'nv12': [(38, 54), (38, 54), (38, 54), (20, 300)]}
BGR_PITCHES = [163, 164, 160, 912]
NV12_PITCHES = [(54, 54), (60, 56), (64, 64), (304, 304)]       # packed (2 mod 4), multiples of 4, multiples of 16
BGR_FRAMES = [np.random.RandomState(70 + k).randint(0, 256, (h, w, 3)).astype(np.uint8) for k, (h, w) in enumerate(SHAPES['bgr'])]
NV12_FRAMES = [(np.random.RandomState(80 + k).randint(0, 256, (h, w)).astype(np.uint8),
                np.random.RandomState(90 + k).randint(0, 256, (h // 2, w)).astype(np.uint8)) for k, (h, w) in enumerate(SHAPES['nv12'])]

# (what, hit x y, kind, image_of, flag, mask)
ROWS = [
    ('interior', (20.4, 11.6), 1, 0, 0, 1),
    ('the same cell at cell_shift 2 and 3', (21.2, 12.4), 2, 2, 0, 1),
    ('left border: taps fall off the grid', (0.0, 18.0), 2, 1, 0, 1),
    ('top border', (30.0, 0.0), 2, 0, 0, 1),
    ('right border', (52.0, 20.0), 1, 1, 0, 1),
    ('bottom border', (10.0, 36.0), 1, 2, 0, 1),
    ('outside the frame, within the radius', (-5.0, 5.0), 2, 3, 0, 1),
    ('halves round to even: (2, 4)', (2.5, 3.5), 1, 1, 0, 1),
    ('a NaN hit', (np.nan, 4.0), 1, 0, 0, 1),
    ('an infinite hit', (4.0, np.inf), 2, 0, 0, 1),
    ('a hit at 9000', (9000.0, 4.0), 2, 1, 0, 1),
    ('kind 0: nothing was looked at', (25.0, 25.0), 0, 0, 0, 1),
    ('kind 3: the camera', (40.0, 30.0), 3, 1, 0, 1),
    ('a kind word of 7', (26.0, 26.0), 7, 0, 0, 1),
    ('a flagged row', (27.0, 27.0), 1, 0, 2, 1),
    ('a masked row', (28.0, 28.0), 1, 1, 0, 0),
    ('an image_of of -1', (29.0, 29.0), 2, -1, 0, 1),
]
HIT = np.array([r[1] for r in ROWS], dtype=np.float32)
KIND = np.array([r[2] for r in ROWS], dtype=np.int32)
IMAGE_OF = np.array([r[3] for r in ROWS], dtype=np.int32)
FLAGS = np.array([r[4] for r in ROWS], dtype=np.int32)
MASK = np.array([r[5] for r in ROWS], dtype=np.int32)
COUNTED = [0, 1, 2, 3, 4, 5, 6, 7]                               # with the default kinds and period 2; kinds 15 adds rows 11 and 12

# (cell_shift, (GH, GW)): grids that do not divide the 37 x 53 frame, and one deliberately smaller than the frame (the edge clamp)
GRIDS = [(0, (37, 53)), (2, (10, 14)), (3, (5, 7)), (2, (6, 9))]
RADII = [0, 3]


def preloaded(cell_shift, grid):
    """A grid [C, GH, GW] that already holds something: row 0's cell of camera 0 stands at 2^31 - 5 (the next call saturates it), the cell of
    the top-border row is negative (read as 0), the rest a few hundred."""
    GH, GW = grid
    heat = np.random.RandomState(5 + cell_shift).randint(0, 400, (C, GH, GW)).astype(np.int32)
    heat[0, min(12 >> cell_shift, GH - 1), min(20 >> cell_shift, GW - 1)] = 2 ** 31 - 5
    heat[0, 0, min(30 >> cell_shift, GW - 1)] = -7
    return heat


def host_frames(fmt):
    return BGR_FRAMES if fmt == 'bgr' else NV12_FRAMES


def device_frames(fmt, junk, dev):
    """tests.test_gpu_draw.device_frames over the frames of this module: views into wider buffers whose padding holds `junk` -> (views, buffers)."""
    import torch
    views, bufs = [], []
    for k, (h, w) in enumerate(SHAPES[fmt]):
        if fmt == 'bgr':
            pitch = BGR_PITCHES[k]
            buf = torch.full((h, pitch), junk, dtype=torch.uint8, device=dev)
            buf[:, :3 * w] = torch.from_numpy(BGR_FRAMES[k].reshape(h, 3 * w)).to(dev)
            views.append(buf.as_strided((h, w, 3), (pitch, 3, 1)))
            bufs.append((buf,))
        else:
            (y, uv), (py, puv) = NV12_FRAMES[k], NV12_PITCHES[k]
            ybuf = torch.full((h, py), junk, dtype=torch.uint8, device=dev)
            uvbuf = torch.full((h // 2, puv), junk, dtype=torch.uint8, device=dev)
            ybuf[:, :w] = torch.from_numpy(y).to(dev)
            uvbuf[:, :w] = torch.from_numpy(uv).to(dev)
            views.append((ybuf[:, :w], uvbuf[:, :w]))
            bufs.append((ybuf, uvbuf))
    return views, bufs


def expected_buffers(fmt, want, junk):
    """What the buffers of device_frames must hold after the call: the host result inside, `junk` untouched in the padding."""
    out = []
    for k, (h, w) in enumerate(SHAPES[fmt]):
        if fmt == 'bgr':
            b = np.full((h, BGR_PITCHES[k]), junk, np.uint8)
            b[:, :3 * w] = want[k].reshape(h, 3 * w)
            out.append((b,))
        else:
            yb, uvb = np.full((h, NV12_PITCHES[k][0]), junk, np.uint8), np.full((h // 2, NV12_PITCHES[k][1]), junk, np.uint8)
            yb[:, :w], uvb[:, :w] = want[k][0], want[k][1].reshape(h // 2, w)
            out.append((yb, uvb))
    return out


def same(fmt, got, want, what=''):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if fmt == 'bgr':
            assert g.shape == w.shape and np.array_equal(g, w), (what, k)
        else:
            assert np.array_equal(g[0], w[0]) and np.array_equal(np.asarray(g[1]).reshape(w[0].shape[0] // 2, -1), np.asarray(w[1]).reshape(w[0].shape[0] // 2, -1)), (what, k)


# ---------------------------------------------------------------- scalar restatements, written from the header's text
def heat_add_scalar(hit, kind, image_of, heat, flags, mask, cell_shift, radius, kinds, period, decay):
    Cn, GH, GW = heat.shape
    taps = [[[0] * GW for _ in range(GH)] for _ in range(Cn)]
    for k in range(len(hit)):
        if flags is not None and int(flags[k]) != 0:
            continue
        if mask is not None and int(mask[k]) == 0:
            continue
        kd = int(kind[k])
        if not 0 <= kd <= 3 or not (kinds >> kd) & 1:
            continue
        io = int(image_of[k])
        if io < 0:
            continue
        c = io if period == 0 else io % period
        if c >= Cn:
            continue
        x, y = float(np.float32(hit[k][0])), float(np.float32(hit[k][1]))
        if not (np.isfinite(x) and np.isfinite(y)):
            continue
        hx, hy = round(x), round(y)                              # python's round: half to even
        if abs(hx) > 8191 or abs(hy) > 8191:
            continue
        ix, iy = hx >> cell_shift, hy >> cell_shift
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if 0 <= ix + dx < GW and 0 <= iy + dy < GH:
                    taps[c][iy + dy][ix + dx] += (radius + 1 - abs(dx)) * (radius + 1 - abs(dy))
    out = np.zeros_like(heat)
    for c in range(Cn):
        for y in range(GH):
            for x in range(GW):
                h = max(int(heat[c, y, x]), 0)
                if decay > 0:
                    h -= h >> decay
                out[c, y, x] = min(h + taps[c][y][x], 2 ** 31 - 1)
    return out, np.array([max(0, int(out[c].max())) for c in range(Cn)], dtype=np.int32)


def level_scalar(grid, full, px, py, cell_shift):
    GH, GW = grid.shape
    S = 1 << cell_shift

    def axis(p, cells):
        u = 2 * p + 1 - S
        i0 = u >> (cell_shift + 1)
        return min(max(i0, 0), cells - 1), min(max(i0 + 1, 0), cells - 1), u - i0 * 2 * S

    x0, x1, fx = axis(px, GW)
    y0, y1, fy = axis(py, GH)
    h = lambda y, x: max(int(grid[y, x]), 0)
    v = (2 * S - fx) * (2 * S - fy) * h(y0, x0) + fx * (2 * S - fy) * h(y0, x1) + (2 * S - fx) * fy * h(y1, x0) + fx * fy * h(y1, x1)
    return min(255, (v * 255) // (4 * S * S * max(int(full), 1)))


def draw_heat_scalar(fmt, frame, grid, full, cell_shift, lut, min_level):
    """One picture over one camera's grid, pixel by pixel -> the annotated copy."""
    blend = lambda s, c, a: (int(s) * (255 - a) + int(c) * a + 127) // 255
    if fmt == 'bgr':
        out = np.array(frame)
        for py in range(out.shape[0]):
            for px in range(out.shape[1]):
                L = level_scalar(grid, full, px, py, cell_shift)
                if L >= min_level:
                    out[py, px] = [blend(out[py, px, ch], lut[L][ch], int(lut[L][3])) for ch in range(3)]
        return out
    y, uv = np.array(frame[0]), np.array(frame[1]).reshape(frame[0].shape[0] // 2, -1)
    h, w = y.shape
    level = [[level_scalar(grid, full, px, py, cell_shift) for px in range(w)] for py in range(h)]
    for py in range(h):
        for px in range(w):
            L = level[py][px]
            if L >= min_level:
                y[py, px] = blend(y[py, px], lut[L][0], int(lut[L][3]))
    for cy in range(h // 2):
        for cx in range(w // 2):
            L = max(level[2 * cy][2 * cx], level[2 * cy][2 * cx + 1], level[2 * cy + 1][2 * cx], level[2 * cy + 1][2 * cx + 1])
            if L >= min_level:
                uv[cy, 2 * cx] = blend(uv[cy, 2 * cx], lut[L][1], int(lut[L][3]))
                uv[cy, 2 * cx + 1] = blend(uv[cy, 2 * cx + 1], lut[L][2], int(lut[L][3]))
    return y, uv
