"""Cases shared by tests/test_detect_cpu.py and tests/test_gpu_detect.py: raw predictions of a YOLO-style head detector, [B, N, 5 + nc]
rows of x, y, w, h, objectness, class scores in pixels of the detector's letterboxed input.  Every case is small (N <= 2048, B <= 3) and
built once; nothing here is modified by a test.

RANDOM  seeded predictions with clustered heads (several anchors fire per head, so NMS has something to suppress)
SIZES   predictions with an exact number of candidates, at the sizes where indexing goes wrong (a wave is 64 lanes, a block step 1024 anchors)
HAND    rows with integer coordinates and in_shape == frame_hw (gain 1, pads 0), so every expected box is exact and written by hand
"""
import numpy as np

NC = 2                                                           # person, head: the demo's detector
HEAD = 1


def clustered(seed, B, N, in_shape, heads, fire=(3, 9), empty=(), nc=NC):
    """B predictions of N anchors: background rows of low objectness and, per image, ``heads`` clusters of fire[0] .. fire[1] anchors around one
    box each, objectness 0.3 .. 0.98, the head class winning most of the time.  Images in ``empty`` keep the background only."""
    rs = np.random.RandomState(seed)
    h, w = in_shape
    p = np.zeros((B, N, 5 + nc), np.float32)
    p[..., 0] = rs.uniform(0, w, (B, N))
    p[..., 1] = rs.uniform(0, h, (B, N))
    p[..., 2:4] = rs.uniform(4, 80, (B, N, 2))
    p[..., 4] = rs.uniform(0, 0.2, (B, N))
    p[..., 5:] = rs.uniform(0, 1, (B, N, nc))
    for b in range(B):
        if b in empty:
            continue
        free = rs.permutation(N)
        at = 0
        for _ in range(heads):
            k = min(int(rs.randint(fire[0], fire[1] + 1)), N - at)
            if k <= 0:
                break
            rows = free[at:at + k]
            at += k
            cx, cy, size = rs.uniform(0.1 * w, 0.9 * w), rs.uniform(0.15 * h, 0.85 * h), rs.uniform(12, 60)
            p[b, rows, 0] = cx + rs.uniform(-0.08, 0.08, k) * size
            p[b, rows, 1] = cy + rs.uniform(-0.08, 0.08, k) * size
            p[b, rows, 2] = size * rs.uniform(0.9, 1.1, k)
            p[b, rows, 3] = size * rs.uniform(0.9, 1.2, k)
            p[b, rows, 4] = rs.uniform(0.3, 0.98, k)
            p[b, rows, 5:] = rs.uniform(0, 0.3, (k, nc))
            p[b, rows, 5 + HEAD] = rs.uniform(0.6, 1.0, k)
            if rs.rand() < 0.3:                                  # a person box on the same spot: class-aware NMS keeps it apart
                p[b, rows[0], 5:] = 0.1
                p[b, rows[0], 5] = 0.95
    return p.astype(np.float32)


def exact_candidates(seed, N, k, in_shape=(96, 160)):
    """One prediction of N anchors of which exactly k pass conf_thres = 0.25 as heads (k = N: every row), boxes spread over the input."""
    rs = np.random.RandomState(seed)
    h, w = in_shape
    p = np.zeros((1, N, 5 + NC), np.float32)
    p[0, :, 0], p[0, :, 1] = rs.uniform(0, w, N), rs.uniform(0, h, N)
    p[0, :, 2:4] = rs.uniform(3, 30, (N, 2))
    p[0, :, 4] = rs.uniform(0.01, 0.2, N)
    p[0, :, 5], p[0, :, 6] = rs.uniform(0.0, 0.3, N), rs.uniform(0.7, 1.0, N)
    rows = rs.permutation(N)[:k]
    p[0, rows, 4] = rs.uniform(0.5, 0.99, k)
    return p


LETTERBOX = (384, 640)                                           # a 1080p frame in the demo's 640 detector: gain 1/3, pads (0, 12)
RANDOM = {
    # name: (pred, in_shape, frame_hw, options)
    'n2048_1080p': (clustered(1, 2, 2048, LETTERBOX, 7), LETTERBOX, (1080, 1920), {}),
    'n1025_b3_mixed_frames': (clustered(2, 3, 1025, (640, 640), 5, empty=(1,)), (640, 640), [[1080, 1920], [720, 1280], [1920, 1080]], {}),
    'n65_every_class': (clustered(3, 1, 65, (160, 160), 3, fire=(4, 6)), (160, 160), (480, 480), dict(only_class=-1)),
    'n64_agnostic': (clustered(4, 2, 64, (160, 160), 3, fire=(4, 6)), (160, 160), (100, 300), dict(only_class=-1, agnostic=True)),
    'n63_tight_iou': (clustered(5, 1, 63, (160, 160), 3, fire=(4, 6)), (160, 160), (160, 160), dict(iou_thres=0.2, conf_thres=0.4)),
    'n700_max_det': (clustered(6, 1, 700, LETTERBOX, 40, fire=(2, 4)), LETTERBOX, (1080, 1920), dict(max_det=7)),
    'n700_max_nms': (clustered(6, 2, 700, LETTERBOX, 40, fire=(2, 4)), LETTERBOX, (1080, 1920), dict(max_nms=50)),
}
SIZES = {
    **{f'n{n}_k{k}': (exact_candidates(10 + i, n, k), (96, 160), (270, 480), {})
       for i, (n, k) in enumerate([(1, 0), (1, 1), (63, 63), (64, 64), (65, 65), (1025, 0), (1025, 1), (1025, 64), (1025, 65), (2048, 64), (2048, 65)])},
    # every anchor a candidate: conf_thres = 0 (objectness and scores are positive), more than max_det survive
    'n1025_all': (exact_candidates(30, 1025, 1025), (96, 160), (270, 480), dict(conf_thres=0.0)),
    'n2048_all': (exact_candidates(31, 2048, 2048), (96, 160), (270, 480), dict(conf_thres=0.0, max_det=300)),
    'n2048_all_max_nms': (exact_candidates(31, 2048, 2048), (96, 160), (270, 480), dict(conf_thres=0.0, max_nms=1500)),
}
SCALE_BACK = {
    'portrait': (clustered(40, 1, 256, (640, 384), 4), (640, 384), (1920, 1080), {}),
    'no_frame': (clustered(41, 3, 128, (160, 160), 3), (160, 160), [[120, 160], [0, 160], [120, -1]], {}),     # flag 2 for images 1 and 2
}
ALL = {**RANDOM, **SIZES, **SCALE_BACK}


def rows(specs, n=None):
    """[(x1, y1, x2, y2, objectness, person score, head score), ...] -> a [1, n, 7] prediction (rows behind the specs: objectness 0)."""
    p = np.zeros((1, max(len(specs), n or 0), 5 + NC), np.float32)
    for k, (x1, y1, x2, y2, obj, c0, c1) in enumerate(specs):
        p[0, k] = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, obj, c0, c1)
    return p


SQUARE = (64, 64)                                                # in_shape == frame_hw: gain 1, pads 0
A, B_, C_ = (0, 0, 10, 10), (0, 4, 10, 14), (0, 8, 10, 18)       # IoU(A, B) = IoU(B, C) = 60 / 140, IoU(A, C) = 20 / 180
nan, inf = float('nan'), float('inf')
# name: (pred, options, expected boxes, expected classes) -- in_shape = frame_hw = SQUARE; scores are the objectness (the winning class scores 1)
HAND = {
    # [0,0,2,3] and [0,1,2,4]: inter 4, union 8, IoU exactly 0.5 -- not ABOVE 0.5
    'iou_half_at_0.5': (rows([(0, 0, 2, 3, 0.9, 0, 1), (0, 1, 2, 4, 0.8, 0, 1)]), dict(iou_thres=0.5), [[0, 0, 2, 3], [0, 1, 2, 4]], [1, 1]),
    'iou_half_at_0.49': (rows([(0, 0, 2, 3, 0.9, 0, 1), (0, 1, 2, 4, 0.8, 0, 1)]), dict(iou_thres=0.49), [[0, 0, 2, 3]], [1]),
    # A suppresses B; B, which is gone, would have suppressed C: C survives
    'chain': (rows([C_ + (0.7, 0, 1), A + (0.9, 0, 1), B_ + (0.8, 0, 1)]), dict(iou_thres=0.4), [list(A), list(C_)], [1, 1]),
    'two_classes_apart': (rows([A + (0.9, 1, 0), A + (0.8, 0, 1)]), dict(only_class=-1), [list(A), list(A)], [0, 1]),
    'two_classes_agnostic': (rows([A + (0.9, 1, 0), A + (0.8, 0, 1)]), dict(only_class=-1, agnostic=True), [list(A)], [0]),
    # objectness 0.5 passes, 0.5 * 0.5 does not
    'product_below_threshold': (rows([A + (0.5, 0, 0.5), (20, 20, 30, 30, 0.5, 0, 1)]), {}, [[20, 20, 30, 30]], [1]),
    'equal_scores_lower_anchor_first': (rows([(40, 40, 50, 50, 0.5, 0, 1), (20, 20, 30, 30, 0.75, 0, 1), A + (0.75, 0, 1)]), {},
                                        [[20, 20, 30, 30], list(A), [40, 40, 50, 50]], [1, 1, 1]),
    'nan_and_inf_boxes': (rows([(nan, 0, 10, 10, 0.9, 0, 1), (0, 0, inf, 10, 0.9, 0, 1), (20, 20, 30, 30, 0.5, 0, 1)]), {}, [[20, 20, 30, 30]], [1]),
    'class_never_wins': (rows([A + (0.9, 1, 0.5), (20, 20, 30, 30, 0.8, 0.75, 0.5)]), dict(only_class=1), [], []),
    # a box that reaches past the frame is clamped: [-6, 50, 70, 80] -> [0, 50, 64, 64]
    'clamped': (rows([(-6, 50, 70, 80, 0.9, 0, 1)]), {}, [[0, 50, 64, 64]], [1]),
}
