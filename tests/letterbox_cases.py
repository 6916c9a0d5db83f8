"""Shared by tests/test_letterbox_cpu.py and tests/test_gpu_letterbox.py (a helper, not a test): the known answers of the reference's
letterbox geometry, a literal restatement of its lines, and the small frames the host and device tests run.  Every frame is at most 128
pixels a side except the one 360 x 640 identity, built once; nothing here is modified by a test.

GEOMETRY  (h, w), new_shape, options -> (unpad_h, unpad_w), (top, bottom, left, right), (out_h, out_w): worked from
          MCGaze_demo/yolo_head/utils/datasets.py:810-840 by hand
CASES     name -> (frames, options of letterbox / letterbox_host): what the pixel tests run, in all three dtypes
"""
import numpy as np

GEOMETRY = [
    # r = 1/3: 360 x 640, dh = 280 % 32 = 24 -> 12 | 12
    ((1080, 1920), 640, {}, (360, 640), (12, 12, 0, 0), (384, 640)),
    ((720, 1280), 640, {}, (360, 640), (12, 12, 0, 0), (384, 640)),
    ((480, 640), 640, {}, (480, 640), (0, 0, 0, 0), (480, 640)),
    # r = 1.28: round(47.36) = 47, dh = 17 -> 8.5: round(8.4) = 8, round(8.6) = 9
    ((37, 50), 64, {}, (47, 64), (8, 9, 0, 0), (64, 64)),
    ((50, 37), 64, {}, (64, 47), (0, 0, 8, 9), (64, 64)),
    # r = 1: dh = 43 % 32 = 11 -> 5.5: 5 | 6;  without auto 43 -> 21.5: 21 | 22
    ((21, 64), 64, {}, (21, 64), (5, 6, 0, 0), (32, 64)),
    ((21, 64), 64, dict(auto=False), (21, 64), (21, 22, 0, 0), (64, 64)),
    # r = 0.64: round(25.6) = 26, dw = 38 % 32 = 6 -> 3 | 3;  without auto 38 -> 19 | 19
    ((100, 40), 64, {}, (64, 26), (0, 0, 3, 3), (64, 32)),
    ((100, 40), 64, dict(auto=False), (64, 26), (0, 0, 19, 19), (64, 64)),
    # r = 64 / 45: round(42.67) = 43, dh = 21 -> 10.5: 10 | 11
    ((30, 45), 64, {}, (43, 64), (10, 11, 0, 0), (64, 64)),
    # the whole-number geometries of the detect_heads round trip
    ((48, 64), 32, {}, (24, 32), (4, 4, 0, 0), (32, 32)),
    # an up-scale by 16 / 3, an exact halving, the workload's identity, and a frame that scaleup=False leaves alone in a 32 x 32 output
    ((9, 12), 64, {}, (48, 64), (8, 8, 0, 0), (64, 64)),
    ((128, 96), 64, {}, (64, 48), (0, 0, 8, 8), (64, 64)),
    ((360, 640), 640, {}, (360, 640), (12, 12, 0, 0), (384, 640)),
    ((9, 12), 64, dict(scaleup=False), (9, 12), (11, 12, 10, 10), (32, 32)),
    # a rectangular new_shape with an odd width: r = min(50 / 30, 37 / 45) = 37 / 45, round(24.67) = 25, dh = 25 -> 12.5: 12 | 13
    ((30, 45), (50, 37), dict(auto=False), (25, 37), (12, 13, 0, 0), (50, 37)),
]


def reference_lines(shape, new_shape=(640, 640), auto=True, scaleup=True, stride=32):
    """datasets.py:810-840 without the pixel calls, kept literal (np.mod and all) -> (new_unpad (w, h), ratio, (dw, dh), (top, bottom, left, right))."""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    ratio = r, r
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = np.mod(dw, stride), np.mod(dh, stride)
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return new_unpad, ratio, (dw, dh), (top, bottom, left, right)


def frame(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def surface(seed, h, w):
    """Full-range NV12 planes: y [h, w], uv [h/2, w/2, 2]."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w // 2, 2)).astype(np.uint8)


ALL_BYTES = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16), np.arange(256, dtype=np.uint8)[::-1].reshape(16, 16),
                      np.arange(256, dtype=np.uint8).reshape(16, 16).T], axis=-1).copy()          # every byte value in every channel
FIVE = [(37, 50), (50, 37), (21, 64), (100, 40), (9, 12)]        # all 64 x 64 without auto

# name: (frames, options).  Output widths 64 / 32 / 640 / 16 take the 4-byte stores (u8: four pixels a thread, f16: two), 37 the narrow ones;
# the rectangles begin and end inside such a group (left = 3, 8, 19; widths 47, 26), above and below it (top 5 .. 21) or fill the output.
CASES = {
    'wide_37x50': ([frame(1, 37, 50)], dict(new_shape=64)),
    'tall_50x37': ([frame(2, 50, 37)], dict(new_shape=64)),
    'auto_21x64': ([frame(3, 21, 64)], dict(new_shape=64)),
    'no_auto_21x64': ([frame(3, 21, 64)], dict(new_shape=64, auto=False)),
    'auto_100x40': ([frame(4, 100, 40)], dict(new_shape=64)),
    'no_auto_100x40': ([frame(4, 100, 40)], dict(new_shape=64, auto=False)),
    'odd_pads_30x45': ([frame(5, 30, 45)], dict(new_shape=64)),
    'upscale_9x12': ([frame(6, 9, 12)], dict(new_shape=64)),
    'halving_128x96': ([frame(7, 128, 96)], dict(new_shape=64)),
    'no_scaleup_9x12': ([frame(6, 9, 12)], dict(new_shape=64, scaleup=False)),
    'odd_width_out': ([frame(8, 30, 45), frame(9, 30, 45)], dict(new_shape=(50, 37), auto=False)),
    'rgb_frames': ([frame(10, 37, 50)], dict(new_shape=64, rgb=True)),
    'stride_8': ([frame(11, 48, 64)], dict(new_shape=32, stride=8)),
    'all_bytes_16x16': ([ALL_BYTES], dict(new_shape=16, stride=16)),
    'five_sizes': ([frame(20 + k, h, w) for k, (h, w) in enumerate(FIVE)], dict(new_shape=64, auto=False)),
    'identity_360x640': ([frame(30, 360, 640)], dict(new_shape=640)),
    'nv12_36x50_bt601': ([surface(40, 36, 50)], dict(new_shape=64, pixel_format='nv12', matrix='bt601')),
    'nv12_three_sizes_bt709': ([surface(41, 36, 50), surface(42, 50, 36), surface(43, 20, 64)],
                               dict(new_shape=64, auto=False, pixel_format='nv12', matrix='bt709')),
    'nv12_odd_width_out': ([surface(44, 30, 44)], dict(new_shape=(50, 37), auto=False, pixel_format='nv12', matrix='bt601')),
    'nv12_upscale_2x2': ([surface(45, 2, 2)], dict(new_shape=32, pixel_format='nv12', matrix='bt709')),
}
BGR_CASES = [k for k, (_, o) in CASES.items() if o.get('pixel_format', 'bgr') == 'bgr']
NV12_CASES = [k for k in CASES if k not in BGR_CASES]
DTYPES = ['uint8', 'float16', 'float32']
