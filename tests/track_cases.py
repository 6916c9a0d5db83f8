"""Cases shared by tests/test_track_cpu.py and tests/test_gpu_track.py: head boxes per frame as detect_heads emits them -- boxes [T, D, 4] or
[Q, T, D, 4] f32 with counts [T] or [Q, T] -- and the tracker's options.  Every case is small and built once; nothing here is modified by a
test.  ALL: name -> (boxes, counts, dict(slots=, match_iou=, max_age=)).  The NaN and infinite rows are inputs the entry documents (bit 2 of
the frame's flag, the row is never matched or born).

HAND   three stories with expected tables written out by hand (tests/test_track_cpu.py): two people crossing, a third person present for
       three frames, one missed detection
"""
import numpy as np

F = np.float32
FAR = [500, 500, 520, 520]                                       # a head far from everything else: rows behind counts hold boxes that WOULD match


def table(frames, D, fill=None):
    """frames: per frame a list of boxes -> (boxes [T, D, 4], counts [T]); the rows behind each count are ``fill`` (default zeros)."""
    boxes = np.zeros((len(frames), D, 4), F)
    if fill is not None:
        boxes[:] = np.asarray(fill, F)
    for t, f in enumerate(frames):
        boxes[t, :len(f)] = np.asarray(f, F).reshape(-1, 4)
    return boxes, np.asarray([len(f) for f in frames], np.int32)


def box(x, y=0, size=20):
    return [x, y, x + size, y + size]


def walkers(seed, T, people, D, miss=0.0, enter=None, size=24, step=3.0):
    """``people`` heads that drift ``step`` pixels a frame with sub-pixel jitter, listed in a random order per frame; each is missed with
    probability ``miss``; enter[p] = (first, last) frame of person p (default: always there)."""
    rs = np.random.RandomState(seed)
    pos = rs.uniform(0, 600, (people, 2))
    vel = rs.uniform(-step, step, (people, 2))
    frames = []
    for t in range(T):
        pos = pos + vel + rs.uniform(-0.5, 0.5, (people, 2))
        heads = []
        for p in rs.permutation(people):
            a, b = (0, T - 1) if enter is None or p not in enter else enter[p]
            if a <= t <= b and rs.rand() >= miss:
                s = size + rs.uniform(-1, 1)
                heads.append([pos[p, 0], pos[p, 1], pos[p, 0] + s, pos[p, 1] + s])
        frames.append(heads)
    return table(frames, D)


def grid(count, t, size=20, pitch=30, per_row=10):
    """``count`` heads on a grid, none overlapping another, each moved by t pixels."""
    return [box((k % per_row) * pitch + t, (k // per_row) * pitch, size) for k in range(count)]


def _cases():
    c = {}
    # S = 1, D = 1: one person, a frame without a head in the middle (counts = 0), found again
    c['s1_d1_one_person'] = table([[box(0)], [box(2)], [], [box(5)], [box(7)], [box(60)]], 1) + (dict(slots=1, match_iou=0.3, max_age=2),)
    # S = 64, D = 300: 70 heads in every frame -- more pairs than threads, more heads than slots (bit 1; the best 64 keep their slots) -- then 40
    c['s64_d300_crowd'] = table([grid(70, 0), grid(70, 1), grid(70, 2), grid(40, 3)], 300, fill=box(1)) + (dict(slots=64, match_iou=0.3, max_age=1),)
    # rows behind counts hold a box that would match slot 0 if it were read
    c['d300_rows_behind_counts'] = table([[box(0), box(100)], [box(101)], [box(3), box(102)], []], 300, fill=box(1)) + (dict(slots=4, match_iou=0.3, max_age=5),)
    # Q = 2: a frame with counts = 0 in a busy sequence, and a sequence that is empty throughout
    busy, busy_n = walkers(3, 8, 3, 6)
    busy_n = busy_n.copy()
    busy_n[4] = 0
    c['count0_and_an_empty_sequence'] = (np.stack([busy, np.full_like(busy, 7)]), np.stack([busy_n, np.zeros_like(busy_n)]), dict(slots=4, match_iou=0.3, max_age=5))
    # identical boxes: every pair ties at IoU 1 -- the lower slot, then the lower detection
    same = box(10)
    c['identical_boxes'] = table([[same, same], [same, same, same], [same, same, same, same], [box(11), box(11)]], 4) + (dict(slots=3, match_iou=0.5, max_age=1),)
    # coasting for exactly max_age frames and matched again; one frame more: freed, then born with a new id
    c['coast_exactly_max_age'] = table([[box(0), box(100)], [box(100)], [box(100)], [box(100)], [box(1), box(100)]], 2) + (dict(slots=4, match_iou=0.3, max_age=3),)
    c['coast_one_more_than_max_age'] = table([[box(0), box(100)], [box(100)], [box(100)], [box(100)], [box(100)], [box(1), box(100)]], 2) + (dict(slots=4, match_iou=0.3, max_age=3),)
    c['max_age_0'] = table([[box(0), box(100)], [box(101)], [box(1), box(102)], [box(2)]], 2) + (dict(slots=4, match_iou=0.3, max_age=0),)
    # S = 1, max_age = 0: the slot is freed and refilled in the same frame
    c['freed_and_refilled_in_one_frame'] = table([[box(0)], [box(200)], [box(201)], [box(0), box(202)]], 2) + (dict(slots=1, match_iou=0.3, max_age=0),)
    # more heads than slots: the best S keep slots, the rest is dropped (bit 1), and a freed slot lets the next one in
    c['more_heads_than_slots'] = table([[box(0), box(50), box(100), box(150)], [box(1), box(51), box(101), box(151)], [box(101), box(151)],
                                        [box(102), box(152), box(300)]], 4) + (dict(slots=2, match_iou=0.3, max_age=0),)
    # a NaN or an infinite coordinate in a valid row: bit 2, never matched or born
    bad, bad_n = table([[box(0), box(50)], [box(1), [np.nan, 0, 70, 20], box(51)], [[2, 0, np.inf, 20], box(52), [-np.inf, 0, 5, 5]], [box(3), box(53)]], 3)
    c['nan_and_inf_rows'] = (bad, bad_n, dict(slots=4, match_iou=0.3, max_age=5))
    # counts outside 0 .. D: bit 4; -1 reads nothing, D + 5 reads D rows
    out, out_n = table([[box(0), box(50)], [box(1), box(51)], [box(2), box(52)], [box(3), box(53)]], 2)
    c['counts_out_of_range'] = (out, np.asarray([2, -1, 7, 2], np.int32), dict(slots=4, match_iou=0.3, max_age=5))
    # match_iou = 0 and boxes that touch but do not overlap: IoU 0 is not > 0
    c['touching_boxes_match_iou_0'] = table([[box(0)], [box(20)], [box(40), box(39)]], 2) + (dict(slots=4, match_iou=0.0, max_age=5),)
    # match_iou < 0: every finite pair is a candidate, IoU 0 included (-0 and +0 are one value: an inverted box gives -0); ties by slot, detection
    c['negative_match_iou'] = table([[box(0), box(100)], [box(300), [90, 0, 60, 20], box(200)], [box(1)]], 3) + (dict(slots=3, match_iou=-1.0, max_age=5),)
    # Q = 3 sequences with different histories in one call: people enter and leave, detections are missed
    seqs = [walkers(11, 12, 5, 8, miss=0.15), walkers(12, 12, 7, 8, enter={0: (3, 8), 2: (0, 4), 5: (6, 11)}), walkers(13, 12, 2, 8, miss=0.4)]
    c['q3_different_histories'] = (np.stack([s[0] for s in seqs]), np.stack([s[1] for s in seqs]), dict(slots=6, match_iou=0.3, max_age=2))
    # a crowd that moves: 20 people, 16 slots, misses -- the default options
    c['walkers_s16'] = walkers(21, 10, 20, 24, miss=0.1, step=6.0) + (dict(slots=16, match_iou=0.3, max_age=5),)
    return c


ALL = _cases()

# ---------------------------------------------------------------- hand-worked stories (slots = 3, match_iou = 0.3, max_age = 2, D = 3)
HAND_OPTIONS = dict(slots=3, match_iou=0.3, max_age=2)
A = lambda x: box(x, 0)                                          # person A walks right along y = 0
B = lambda x: box(x, 10)                                         # person B walks left along y = 10
# two people crossing, 8 pixels a frame each (IoU with one's own last box 12 * 20 / (800 - 240) = 0.43; with the other's at the closest,
# frame 3 against frame 2: x offset 4 -> 16 * 10 / (800 - 160) = 0.25).  The detector lists the LEFT one first in every frame.
CROSSING_PEOPLE = [[A(0), B(36)], [A(8), B(28)], [A(16), B(20)], [A(24), B(12)], [A(32), B(4)]]
CROSSING = [sorted(f, key=lambda b: b[0]) for f in CROSSING_PEOPLE]
# a third person present for three frames (2 .. 4), listed first while there
C3 = lambda x: box(x, 200)
ENTER_LEAVE = [[A(0), B(100)], [A(2), B(98)], [C3(50), A(4), B(96)], [C3(52), A(6), B(94)], [C3(54), A(8), B(92)], [A(10), B(90)], [A(12), B(88)]]
# one missed detection: B is not seen in frame 2
MISSED = [[A(0), B(100)], [A(2), B(98)], [A(4)], [A(6), B(94)], [A(8), B(92)]]
HAND = {name: table(frames, 3) for name, frames in (('crossing', CROSSING), ('enter_leave', ENTER_LEAVE), ('missed', MISSED))}
