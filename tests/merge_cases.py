"""Shared by tests/test_device_merge_cpu.py and tests/test_gpu_device_merge.py: random decoder outputs for the windows of a plan, the ways
a plan is split over decoder calls, and a numpy statement of mcg_merge_windows (csrc/merge.hip) that applies a plan table row by row."""
import numpy as np
import torch

from mcgaze_amd import harness

THR = np.float32(0.5)
BELOW = np.nextafter(np.float32(0.5), np.float32(0))           # the largest f32 below the threshold
SCORES = np.array([0.2, 0.5, 0.7, BELOW], dtype=np.float32)     # 0.5 itself is NOT low: the compare is <
CONFIGS = [(7, 4), (5, 1), (7, 7), (3, 2)]


def window_outputs(rs, T):
    """Engine-layout outputs of one window of T frames: gaze [4,T,3], boxes [T,3,4], scores [T,3], f32; one box coordinate is -0.0."""
    gaze = rs.standard_normal((4, T, 3)).astype(np.float32)
    boxes = rs.uniform(-20, 200, (T, 3, 4)).astype(np.float32)
    boxes[rs.randint(T), rs.randint(3), rs.randint(4)] = np.float32(-0.0)
    scores = SCORES[rs.randint(0, 4, (T, 3))]
    return gaze, boxes, scores


def splits(num_windows):
    """The three ways the windows of a plan are dealt to decoder calls: all in one, one per call, two halves (lists of window indices)."""
    idx = list(range(num_windows))
    h = (num_windows + 1) // 2
    return {'one call': [idx], 'one per call': [[i] for i in idx], 'two halves': [c for c in (idx[:h], idx[h:]) if c]}


def call_of(outs, part):
    """The outputs of the windows ``part`` as ONE decoder call: (gaze [4,n,3], boxes [n,3,4], scores [n,3], first row of each window)."""
    first = np.concatenate([[0], np.cumsum([outs[i][1].shape[0] for i in part])]).tolist()[:-1]
    return (np.concatenate([outs[i][0] for i in part], axis=1), np.concatenate([outs[i][1] for i in part]),
            np.concatenate([outs[i][2] for i in part]), first)


def reference(plan, outs, scale=None, thr=THR):
    """harness.merge_video over the plan, as [L, 27] rows.  scale: None, [4], or one [T,4] array per window."""
    clips = []
    for i, (g, b, s) in enumerate(outs):
        sc = None
        if scale is not None:
            sc = torch.from_numpy(np.asarray(scale if np.ndim(scale) == 1 else scale[i], dtype=np.float32).reshape(-1, 1, 4))
        clips.append(harness.clip_outputs(dict(gaze=torch.from_numpy(g), boxes=torch.from_numpy(b), scores=torch.from_numpy(s)), sc))
    det, fused, others = harness.merge_video(plan, clips, thr)
    L = det.shape[0]
    return np.concatenate([det.reshape(L, 15), fused.reshape(L, 3), others.reshape(L, 9)], axis=1)


def emulate(table, max_src, gaze, boxes, scores, scale, store, thr=THR):
    """mcg_merge_windows in numpy, one (plan row, clue) after the other; store [rows, 27] is updated in place."""
    n = scores.shape[0]
    assert table.dtype == np.int32 and table.shape[1] == 2 + max_src
    for row in table:
        dst, cont = int(row[0]), int(row[1])
        if not 0 <= dst < store.shape[0]:
            continue
        for c in range(3):
            have = bool(cont)
            box, score, fused, oth = store[dst, 5 * c:5 * c + 4].copy(), store[dst, 5 * c + 4], store[dst, 15 + c], store[dst, 18 + 3 * c:21 + 3 * c].copy()
            changed = False
            for s in row[2:].tolist():
                if not 0 <= s < n:
                    continue
                sc = scores[s, c]
                low = sc < thr
                b = boxes[s, c]
                if scale is not None:
                    b = b / (scale if scale.ndim == 1 else scale[s])
                b = np.where(low, np.float32(0), b).astype(np.float32)
                f, o = gaze[0, s, c], gaze[1 + c, s]
                if not have:
                    box, score, fused, oth, have = b, sc, f, o, True
                else:
                    bad = (score < thr) | low
                    box = np.where(bad, np.float32(0), (box + b) / np.float32(2)).astype(np.float32)
                    score, fused, oth = (score + sc) / np.float32(2), (fused + f) / np.float32(2), (oth + o) / np.float32(2)
                changed = True
            if changed:
                store[dst, 5 * c:5 * c + 4], store[dst, 5 * c + 4], store[dst, 15 + c], store[dst, 18 + 3 * c:21 + 3 * c] = box, score, fused, oth


def run_plan(plan, outs, parts, apply, scale=None, perm=None):
    """Deal the windows ``parts`` (lists of window indices, one list per decoder call) through harness.merge_plan and ``apply(table,
    max_src, gaze, boxes, scores, scale of the call)``.  Frame f of the video has store row perm[f] (default f).  -> the longest source
    list met.  scale: None, [4], or one [T,4] array per window (concatenated per call)."""
    L = plan[-1][1]
    written, longest = set(), 0
    for part in parts:
        g, b, s, first = call_of(outs, part)
        table, max_src = harness.merge_plan([(0, plan[i], r) for i, r in zip(part, first)], lambda k, f: f if perm is None else perm[f], written,
                                            s.shape[0], L if perm is None else max(perm) + 1)
        sc = scale if scale is None or np.ndim(scale) == 1 else np.concatenate([scale[i] for i in part])
        apply(table, max_src, g, b, s, None if sc is None else np.asarray(sc, dtype=np.float32))
        for i in part:
            written.update((0, f) for f in range(plan[i][0], plan[i][1]))
        longest = max(longest, max_src)
    return longest
