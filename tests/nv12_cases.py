"""Shared by tests/test_nv12_cpu.py and tests/test_gpu_nv12.py (a helper, not a test): an independent restatement of the NV12 -> BGR
conversion, known answers worked by hand, and the small frames and head boxes the device tests run.

The restatement is written from the formula alone (include/mcgaze_hip.h, "NV12 surfaces in"), one pixel at a time in python's unbounded
ints, and imports nothing from mcgaze_amd.pipeline:

    u = U - 128, v = V - 128, yy = max(0, Y - y_off) * cy
    R = sat8((yy + cvr * v + 2^19) >> 20), G = sat8((yy + cvg * v + cug * u + 2^19) >> 20), B = sat8((yy + cub * u + 2^19) >> 20)

with U, V the nearest chroma sample, UV[y >> 1][x >> 1]."""
import numpy as np

# y_off, cy, cub, cug, cvg, cvr at 20 fractional bits
COEF = {'bt601': (16, 1220542, 2116026, -409993, -852492, 1673527),
        'bt709': (16, 1220945, 2215014, -223607, -558796, 1879825)}


def convert_pixel(Y, U, V, matrix):
    """-> (R, G, B) of one pixel, python ints (>> on a negative int floors: an arithmetic shift)."""
    y_off, cy, cub, cug, cvg, cvr = COEF[matrix]
    Y, u, v = int(Y), int(U) - 128, int(V) - 128
    yy = max(0, Y - y_off) * cy
    sat8 = lambda t: min(max(t, 0), 255)
    return sat8((yy + cvr * v + (1 << 19)) >> 20), sat8((yy + cvg * v + cug * u + (1 << 19)) >> 20), sat8((yy + cub * u + (1 << 19)) >> 20)


def convert_frame(y, uv, matrix):
    """y [H,W], uv [H/2,W/2,2] -> HxWx3 uint8 in cv2's BGR order, pixel by pixel."""
    h, w = y.shape
    out = np.zeros((h, w, 3), np.uint8)
    for r in range(h):
        for c in range(w):
            out[r, c] = convert_pixel(y[r, c], uv[r >> 1, c >> 1, 0], uv[r >> 1, c >> 1, 1], matrix)[::-1]
    return out


# (Y, U, V) -> (R, G, B), every sum worked by hand; 2^19 = 524288, 2^20 = 1048576
KNOWN = {
    'bt601': [
        ((16, 128, 128), (0, 0, 0)),            # yy = 0, u = v = 0: 524288 >> 20 = 0
        ((235, 128, 128), (255, 255, 255)),     # yy = 219 * 1220542 = 267298698; + 524288 = 267822986 = 255 * 1048576 + 436106
        ((5, 128, 128), (0, 0, 0)),             # Y < 16: max(0, -11) = 0, as black
        # yy = 184 * 1220542 = 224579728, v = 127.  R: + 1673527 * 127 = 212537929 -> 437641945 >> 20 = 417 -> 255 (saturates high);
        # G: - 852492 * 127 = 108266484 -> 116837532 >> 20 = 111;  B: 225104016 >> 20 = 214
        ((200, 128, 255), (255, 111, 214)),
        # u = 127.  B: + 2116026 * 127 = 268735302 -> 493839318 >> 20 = 470 -> 255 (saturates high);  G: - 409993 * 127 = 52069111 ->
        # 173034905 >> 20 = 165;  R: 214
        ((200, 255, 128), (214, 165, 255)),
        # yy = 14 * 1220542 = 17087588, u = v = 127.  G: 17087588 - 108266484 - 52069111 + 524288 = -142723719 >> 20 = -137 -> 0 (saturates
        # low);  R: 17087588 + 212537929 + 524288 = 230149805 >> 20 = 219;  B: 17087588 + 268735302 + 524288 = 286347178 >> 20 = 273 -> 255
        ((30, 255, 255), (219, 0, 255)),
        # yy = 0, u = -128.  B: 2116026 * -128 + 524288 = -270327040: an ARITHMETIC shift gives -258 -> 0 (a logical one 3838 -> 255);
        # G: -409993 * -128 + 524288 = 53003392 >> 20 = 50;  R: 0
        ((16, 0, 128), (0, 50, 0)),
        # nothing clamps: yy = 112 * 1220542 = 136700704, u = -28, v = 32.  R: + 53552864 + 524288 = 190777856 >> 20 = 181;
        # G: - 27279744 + 11479804 + 524288 = 121425052 >> 20 = 115;  B: - 59248728 + 524288 = 77976264 >> 20 = 74
        ((128, 100, 160), (181, 115, 74)),
    ],
    'bt709': [
        ((16, 128, 128), (0, 0, 0)),
        ((235, 128, 128), (255, 255, 255)),     # yy = 219 * 1220945 = 267386955; + 524288 = 267911243 = 255 * 1048576 + 524363
        ((5, 128, 128), (0, 0, 0)),
        # yy = 184 * 1220945 = 224653880, v = 127.  R: + 1879825 * 127 = 238737775 -> 463915943 >> 20 = 442 -> 255;
        # G: - 558796 * 127 = 70967092 -> 154211076 >> 20 = 147;  B: 225178168 >> 20 = 214
        ((200, 128, 255), (255, 147, 214)),
        # u = 127.  B: + 2215014 * 127 = 281306778 -> 506484946 >> 20 = 483 -> 255;  G: - 223607 * 127 = 28398089 -> 196780079 >> 20 = 187;  R: 214
        ((200, 255, 128), (214, 187, 255)),
        # yy = 14 * 1220945 = 17093230.  G: 17093230 - 70967092 - 28398089 + 524288 = -81747663 >> 20 = -78 -> 0;
        # R: 17093230 + 238737775 + 524288 = 256355293 >> 20 = 244;  B: 17093230 + 281306778 + 524288 = 298924296 >> 20 = 285 -> 255
        ((30, 255, 255), (244, 0, 255)),
        # B: 2215014 * -128 + 524288 = -282997504 >> 20 = -270 -> 0;  G: -223607 * -128 + 524288 = 29145984 >> 20 = 27;  R: 0
        ((16, 0, 128), (0, 27, 0)),
        # yy = 112 * 1220945 = 136745840, u = -28, v = 32.  R: + 60154400 + 524288 = 197424528 >> 20 = 188;
        # G: - 17881472 + 6260996 + 524288 = 125649652 >> 20 = 119;  B: - 62020392 + 524288 = 75249736 >> 20 = 71
        ((128, 100, 160), (188, 119, 71)),
    ],
}


def planes(seed, h, w):
    """Random FULL-range planes: y [h,w], uv [h/2,w/2,2].  Bytes outside the nominal 16..235 / 16..240 hit every clamp constantly."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w // 2, 2)).astype(np.uint8)


# image 0: 12 x 16, pitches equal to the width; image 1: 18 x 22, pitch_y 32 and pitch_uv 24 on the device (different, both padded);
# image 2: one 2 x 2 frame -- the smallest shapes that still reach every index path
SHAPES = [(12, 16), (18, 22), (2, 2)]
PITCHES = [(16, 16), (32, 24), (2, 2)]
FRAMES = [planes(20 + k, h, w) for k, (h, w) in enumerate(SHAPES)]

# (what, image, box x1 y1 x2 y2, window y0 x0 h w), worked by hand from the demo's expressions (tests/test_head_crops_cpu.py):
#   cy, cx = int(y1 + y2) // 2, int(x1 + x2) // 2;  l = int(max(y2 - y1, x2 - x1) * 0.8);  rows [max(0, cy - l), min(cy + l, h)), columns alike
CASES = [
    # cy = 20 // 2 = 10, cx = 28 // 2 = 14, l = int(3.2) = 3: rows [7, min(13, 12)), columns [11, min(17, 16)): 5 x 5 -> 32 x 32, an up-scale;
    # crop_y and crop_x ODD; touches the bottom and right borders
    ('5x5 bottom-right, odd origin', 0, (12, 8, 16, 12), (7, 11, 5, 5)),
    # cy = cx = 4 // 2 = 2, l = 3: rows [max(0, -1), 5), columns alike: touches the top and left borders; shares image 0
    ('5x5 top-left, even origin', 0, (0, 0, 4, 4), (0, 0, 5, 5)),
    # cy = int(12.0) // 2 = 6, cx = int(14.0) // 2 = 7, l = int(2.4) = 2: rows [4, 8), columns [5, 9): crop_y even, crop_x odd
    ('interior, even y odd x', 0, (5.5, 4.5, 8.5, 7.5), (4, 5, 4, 4)),
    # cy = 12 // 2 = 6, cx = 18 // 2 = 9, l = 3: rows [3, 9), columns [6, 12): crop_y odd, crop_x even
    ('interior, odd y even x', 0, (7, 4, 11, 8), (3, 6, 6, 6)),
    # cy = 18 // 2 = 9, cx = 22 // 2 = 11, l = int(42 * 0.8) = 33: the whole 18 x 22 frame, all four borders.  At img_scale 32 it is resized to
    # 26 x 32 (f = 32 / 22); test_gpu_nv12.py runs it at img_scale 8 as well, where it is a down-scale to 7 x 8
    ('whole 18x22 frame', 1, (-10, -10, 32, 28), (0, 0, 18, 22)),
    # cy = 36 // 2 = 18, cx = 44 // 2 = 22, l = int(1.6) = 1: rows [17, min(19, 18)), columns [21, min(23, 22)): ONE pixel, the last of both planes
    ('1x1 at the last pixel', 1, (21, 17, 23, 19), (17, 21, 1, 1)),
    # cy = int(18.0) // 2 = 9, cx = int(22.0) // 2 = 11, l = int(4.0) = 4: rows [5, 13), columns [7, 15): odd, odd in the pitched frame
    ('interior of the pitched frame', 1, (8.5, 6.5, 13.5, 11.5), (5, 7, 8, 8)),
    # cy = cx = 1, l = int(1.6) = 1: rows [0, 2), columns [0, 2): the whole 2 x 2 frame
    ('whole 2x2 frame', 2, (0, 0, 2, 2), (0, 0, 2, 2)),
]
BOXES = np.array([c[2] for c in CASES], dtype=np.float32)
IMAGE_OF = np.array([c[1] for c in CASES], dtype=np.int32)
WINDOWS = np.array([c[3] for c in CASES], dtype=np.int32)
# device tables only: a box of no extent (l = int(0.8) = 0: rows [5, 5) -- flag 1, one pixel at (5, 5)) and an image index one past the table
# (flag 2, pixel (0, 0) of image 0) between usable rows
FLAG_BOXES = np.concatenate([BOXES[:2], np.array([(5, 5, 6, 6)], np.float32), BOXES[2:5], BOXES[:1], BOXES[5:]])
FLAG_IMAGE_OF = np.concatenate([IMAGE_OF[:2], [0], IMAGE_OF[2:5], [len(SHAPES)], IMAGE_OF[5:]]).astype(np.int32)
FLAGS = [0, 0, 1, 0, 0, 0, 2, 0, 0, 0]
FLAG_WINDOWS = np.concatenate([WINDOWS[:2], [(5, 5, 1, 1)], WINDOWS[2:5], [(0, 0, 1, 1)], WINDOWS[5:]]).astype(np.int32)
