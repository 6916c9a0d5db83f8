"""Cases shared by tests/test_track_motion_cpu.py and tests/test_gpu_track_motion.py: the tracker with its constant-velocity motion model
(mcg_track_heads_motion; track_heads_host(motion=...)).  Built once; nothing here is modified by a test.
ALL: name -> (boxes, counts, dict(slots=, match_iou=, max_age=, motion=)).

The hand scenario is the one the model exists for: ONE person, a 24 x 24 box at x = 12 t, y = 0 for t = 0 .. 9, not detected at t = 4, 5, 6.
Every number below is exact in f32 (small integers and halves).
  plain tracker   consecutive boxes overlap with IoU 12 * 24 / (2 * 576 - 288) = 288 / 864 = 1 / 3 > 0.3: frames 0 - 3 are id 1.  The slot then
                  coasts at x = 36; the detection of frame 7 at x = 84 has IoU 0 with it and is born as id 2.
  gain 1, decay 1 frame 1: predicted x = 0 (at rest), centre residual 12 -> v = 12; frames 2, 3 are predicted exactly (residual 0).  Coasting:
                  x1 = 48, 60, 72.  Frame 7 is predicted at 84: IoU 1.
  gain 0.5        v = 6 after frame 1; frame 2 is predicted at 18, residual 6 -> v = 9; frame 3 at 33, residual 3 -> v = 10.5.  Coasting:
                  x1 = 46.5, 57, 67.5.  Frame 7 is predicted at 78 against 84: IoU 18 * 24 / (1152 - 432) = 0.6.
"""
import numpy as np

from tests import track_cases as TC

F = np.float32
BIG = 1e38                                                       # f32 ends at 3.4e38

HAND_OPTIONS = dict(slots=4, match_iou=0.3, max_age=5)
HAND_MISSED = (4, 5, 6)
HAND = TC.table([[] if t in HAND_MISSED else [TC.box(12 * t, 0, 24)] for t in range(10)], 1)


def flat(x1, x2):
    """A box 1e-3 high whose area is finite for x of the order of 1e38."""
    return [x1, 0.0, x2, 1e-3]


def _cases():
    c = {}
    for gain in (1.0, 0.5):
        c[f'hand_gain_{gain}'] = HAND + (dict(HAND_OPTIONS, motion=dict(gain=gain, decay=1.0)),)
    # S = 1, max_age = 0: the person moves (v = 10), then is seen somewhere else: the slot is freed and refilled in one frame, at rest
    c['freed_and_reborn_in_one_frame'] = TC.table([[TC.box(0)], [TC.box(10)], [TC.box(200)], [TC.box(201)]], 1) + \
        (dict(slots=1, match_iou=0.3, max_age=0, motion=dict(gain=1.0, decay=1.0)),)
    # the prediction overflows: centres 0 and 1.5e38 are finite, v = 1.5e38, and 2.5e38 + 1.5e38 is not: the box stays, the velocity is zeroed
    c['prediction_overflows'] = TC.table([[flat(-BIG, BIG)], [flat(0.5 * BIG, 2.5 * BIG)], [], [flat(0.5 * BIG, 2.5 * BIG)]], 1) + \
        (dict(slots=2, match_iou=0.1, max_age=3, motion=dict(gain=1.0, decay=1.0)),)
    # the velocity update overflows: x1 + x2 of the detection is 4.4e38 -> an infinite residual -> the velocity is zeroed
    c['velocity_update_overflows'] = TC.table([[flat(0.0, 2 * BIG)], [flat(1.2 * BIG, 3.2 * BIG)], [flat(1.2 * BIG, 3.2 * BIG)]], 1) + \
        (dict(slots=2, match_iou=0.1, max_age=3, motion=dict(gain=1.0, decay=1.0)),)
    # a -0.0 coordinate in a slot at rest: coasting must not add a + 0.0f to it
    c['negative_zero_at_rest'] = TC.table([[[-0.0, -0.0, 20, 20]], [], [[-0.0, -0.0, 20, 20]], []], 1) + \
        (dict(slots=2, match_iou=0.3, max_age=3, motion=dict(gain=0.5, decay=1.0)),)
    # the plain tracker's documented bad inputs, moving
    for name in ('nan_and_inf_rows', 'counts_out_of_range'):
        boxes, counts, opts = TC.ALL[name]
        c[name] = (boxes, counts, dict(opts, motion=dict(gain=0.5, decay=1.0)))
    # S = 1, D = 1
    boxes, counts, opts = TC.ALL['s1_d1_one_person']
    c['s1_d1'] = (boxes, counts, dict(opts, motion=dict(gain=0.5, decay=0.5)))
    # S = 64, D = 1024: 64 walkers with misses, every slot and most of the detection rows' range in use
    c['s64_d1024_walkers'] = TC.walkers(31, 6, 64, 1024, miss=0.15, step=6.0) + (dict(slots=64, match_iou=0.3, max_age=2, motion=dict(gain=0.5, decay=1.0)),)
    # D = 5 .. 9 heads: the detections spread over the four waves' d = w + 4 j
    for D in range(5, 10):
        c[f'd{D}_walkers'] = TC.walkers(40 + D, 8, D, D, miss=0.2, step=6.0) + (dict(slots=12, match_iou=0.3, max_age=3, motion=dict(gain=0.5, decay=0.5)),)
    # Q = 3 sequences with different histories
    boxes, counts, opts = TC.ALL['q3_different_histories']
    c['q3_gain_0.5'] = (boxes, counts, dict(opts, motion=dict(gain=0.5, decay=1.0)))
    c['q3_decay_0.5'] = (boxes, counts, dict(opts, motion=dict(gain=1.0, decay=0.5)))
    # the defaults
    boxes, counts, opts = TC.ALL['walkers_s16']
    c['walkers_s16_defaults'] = (boxes, counts, dict(opts, motion=True))
    return c


ALL = _cases()
PURITY = ('q3_gain_0.5', 'q3_decay_0.5', 'walkers_s16_defaults', 'd7_walkers')      # walkers with misses, at gain 0.5 and at decay 0.5
