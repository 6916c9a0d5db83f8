"""One scripted scene for the live chain (mcgaze_amd/live.py), shared by tests/test_live_cpu.py and tests/test_gpu_live.py: Q = 2 cameras,
S = 4 slots, D = 8 detection rows, 28 ticks, max_age = 2, clip 7 / stride 4.

Camera 0:  A at every tick, with no detection at ticks 17 and 18 (it coasts);  B at ticks 0 .. 9 (it coasts 10 and 11 and its slot is free
           from tick 12);  C enters at tick 14 and lands in B's freed slot.
Camera 1:  empty until tick 6, then D, detected up to tick 24 (it coasts 25 and 26 and its slot is free at tick 27, the last);  at tick 20
           the camera shows six heads -- D and five others, two more than there are free slots: flag bit 1.
The variant scene ('other'): C enters at the same tick and position, B never existed, and camera 1 shows one other head from tick 2 on.

``run_host`` is the whole chain on the host with the schedule LiveGaze has: track_heads_host, live_slots_host, the spans of a WindowPlanner,
live_gate_host -- one frame per tick, a frame handed out once it is final (one frame later with smoothing), the rest at the end; with
``lanes``, the same schedule over live_lanes_host and live_gate_lanes_host (tests/live_lanes_cases.py holds the scene made for it)."""
import numpy as np

from mcgaze_amd import live
from mcgaze_amd.head_detect import track_heads_host, track_state_words
from mcgaze_amd.stream import WindowPlanner

Q, S, D, TICKS, MAX_AGE, CLIP, STRIDE = 2, 4, 8, 28, 2, 7, 4
FRAME_HW = (96, 128)
OPTIONS = dict(slots=S, match_iou=0.3, max_age=MAX_AGE)
SLOT_A, SLOT_BC, SLOT_D = (0, 0), (0, 1), (1, 0)               # (camera, slot) of the people, by the lowest-free-slot rule


def box_a(t):
    return (2 + t // 2, 10, 32 + t // 2, 44)                   # its window is clipped by the left border: the crop is not square


def box_b(t):
    return (70, 20 + t % 2, 98, 50 + t % 2)


def box_c(t):
    return (72, 22, 100 + t % 3, 54)


def box_d(t):
    return (40 + t % 2, 30, 76 + t % 2, 70)


CROWD = [(4, 4, 20, 22), (24, 4, 40, 22), (90, 4, 110, 24), (4, 70, 22, 92), (100, 70, 124, 94)]


def scene(variant='main'):
    """-> (boxes float32 [TICKS, Q, D, 4], counts int32 [TICKS, Q])."""
    boxes, counts = np.zeros((TICKS, Q, D, 4), np.float32), np.zeros((TICKS, Q), np.int32)
    for t in range(TICKS):
        cam0 = [box_a(t)] if t not in (17, 18) else []
        if variant == 'main' and t <= 9:
            cam0.append(box_b(t))
        if t >= 14:
            cam0.append(box_c(t))
        if variant == 'main':
            cam1 = ([box_d(t)] if 6 <= t <= 24 else []) + (CROWD if t == 20 else [])
        else:
            cam1 = [(50, 40, 80, 76)] if t >= 2 else []
        for q, heads in enumerate((cam0, cam1)):
            boxes[t, q, :len(heads)], counts[t, q] = np.asarray(heads, np.float32).reshape(-1, 4), len(heads)
    return boxes, counts


def fake_gaze(k, first, lanes=None):
    """Stand-ins for a pool's gaze rows of frames first .. first + k - 1, each value naming its (frame, camera, slot, component) -- with
    lanes, its (frame, lane, component) --, and their 'smoothed' twins (negated): the gate copies rows, it computes nothing on them."""
    if lanes is None:
        f, q, s = np.meshgrid(np.arange(first, first + k), np.arange(Q), np.arange(S), indexing='ij')
        base = (f * 1000 + q * 100 + s * 10).astype(np.float32)
    else:
        f, p = np.meshgrid(np.arange(first, first + k), np.arange(lanes), indexing='ij')
        base = (f * 10000 + p * 10).astype(np.float32)
    fused = base[..., None] + np.arange(3, dtype=np.float32)
    others = base[..., None, None] + np.arange(3, 12, dtype=np.float32).reshape(3, 3)
    return fused, others, -fused, -others


def run_host(boxes, counts, smooth=False, gaze=fake_gaze, lanes=None):
    """The fixed schedule, or with ``lanes`` the lanes of LiveGaze(lanes=lanes).
    -> dict(ticks=[per tick: crop_boxes, image_of, ring_id row, ring_box row, matched, flags, track_id; with lanes also lane_state, lane_of,
    overflow and the ring_col row], emitted=[(tick it was returned at, first, k)], windows, tables=[(table, first_out)], and the gate's
    outputs concatenated over the frames: track_id, valid, image_of, head_box[, camera, slot][, smooth_valid, fused_smooth,
    others_smooth]).  gaze(k, first, lanes) -> (fused, others, fused_smooth, others_smooth) of the returned frames."""
    R = live.ring_depth(CLIP)
    lead = (Q, S) if lanes is None else (lanes,)
    ring_id, ring_box = np.zeros((R,) + lead, np.int32), np.zeros((R,) + lead + (4,), np.float32)
    ring_col, lane_state = np.zeros((R,) + lead, np.int32), np.zeros(lead + (2,), np.int32)      # with lanes only
    state = np.zeros((Q, track_state_words(S)), np.int32)
    planner, windows, emitted = WindowPlanner(CLIP, STRIDE), [], 0
    out = dict(ticks=[], emitted=[], tables=[], windows=[])
    parts = []

    def assign(t):
        if lanes is None:
            crop_boxes, image_of, matched = live.live_slots_host(state, t, ring_id, ring_box)
            return dict(crop_boxes=crop_boxes, image_of=image_of, matched=matched)
        crop_boxes, image_of, lane_of, matched, overflow = live.live_lanes_host(state, t, lane_state, ring_id, ring_box, ring_col)
        return dict(crop_boxes=crop_boxes, image_of=image_of, matched=matched, lane_state=lane_state.copy(), lane_of=lane_of, overflow=overflow,
                    ring_col=ring_col[t % R].copy())

    def emit(tick, ended):
        nonlocal emitted
        k = max(0, planner.final_upto - emitted - int(smooth and not ended))
        if k:
            table, first_out = live.live_gate_table(windows, emitted, k, smooth, tick if ended else None)
            table = live.check_gate_table(table, tick, R)
            g = gaze(k, emitted, lanes) if smooth else (None,) * 4
            if lanes is None:
                parts.append(live.live_gate_host(ring_id, ring_box, tick, table, first_out, k, *g))
            else:
                parts.append(live.live_gate_lanes_host(ring_id, ring_box, ring_col, Q, S, tick, table, first_out, k, *g))
            out['tables'].append((table, first_out))
        out['emitted'].append((tick, emitted, k))
        emitted += k

    for t in range(len(boxes)):
        res = track_heads_host(boxes[t][:, None], counts[t][:, None], state=state, **OPTIONS)
        state = res[6]
        out['ticks'].append(dict(assign(t), ring_id=ring_id[t % R].copy(), ring_box=ring_box[t % R].copy(), flags=res[5].reshape(Q),
                                 track_id=res[2].reshape(Q, S)))
        windows += planner.feed(1)
        emit(t, False)
    windows += planner.finish()
    emit(len(boxes) - 1, True)
    out['windows'] = windows
    for name in parts[0]:
        out[name] = np.concatenate([p[name] for p in parts])
    return out


def ring_at(run, tick):
    """The identity ring of a fixed-schedule run_host as it stood after ``tick``, from the rows its ticks recorded."""
    R = live.ring_depth(CLIP)
    ring_id, ring_box = np.zeros((R, Q, S), np.int32), np.zeros((R, Q, S, 4), np.float32)
    for t in range(max(0, tick - R + 1), tick + 1):
        ring_id[t % R], ring_box[t % R] = run['ticks'][t]['ring_id'], run['ticks'][t]['ring_box']
    return ring_id, ring_box


def as_lane_ring(ring_id, ring_box):
    """A slot ring as the lane ring it is: P = Q * S lanes, lane p naming column p wherever a person is.  -> (ring_id, ring_box, ring_col)."""
    ids = ring_id.reshape(len(ring_id), Q * S)
    return ids, ring_box.reshape(len(ring_id), Q * S, 4), np.where(ids != 0, np.arange(Q * S, dtype=np.int32), -1).astype(np.int32)
