"""The live chain with lanes (mcgaze_amd/live.py, ``LiveGaze(lanes=P)``), shared by tests/test_live_lanes_cpu.py and
tests/test_gpu_live_lanes.py: the scenes of tests/live_cases.py and a second scripted scene, 'queue', in which a person waits for a lane.

'queue': Q = 2 cameras, S = 4 slots, D = 8 detection rows, 28 ticks, max_age = 2, clip 7 / stride 4, and P = 2 lanes for three people.
Camera 0:  A (box_a) detected at ticks 0 .. 9; it coasts at 10 and 11 and its slot is free from tick 12.  C (box_c) detected from tick 4 to
           the end: slot (0, 1), id 2.
Camera 1:  D (box_d) detected at every tick: slot (1, 0), id 1 -- the same id as A, in another camera.
So A holds lane 0 and D lane 1 from tick 0, C waits from tick 4 (overflow 1) and takes lane 0 at tick 12, in the call that releases it.

``run_host_lanes`` is the whole chain on the host with the schedule LiveGaze has, in the shape of live_cases.run_host: track_heads_host,
live_lanes_host, the spans of a WindowPlanner, live_gate_lanes_host."""
import numpy as np

from mcgaze_amd import live
from mcgaze_amd.head_detect import track_heads_host, track_state_words
from mcgaze_amd.stream import WindowPlanner
from tests import live_cases as LC

Q, S, D, TICKS, CLIP, STRIDE = LC.Q, LC.S, LC.D, LC.TICKS, LC.CLIP, LC.STRIDE
QUEUE_LANES = 2
COL_A, COL_C, COL_D = 0, 1, 4                                    # column = camera * S + slot


def scene(variant):
    """-> (boxes float32 [TICKS, Q, D, 4], counts int32 [TICKS, Q]); 'queue', or a scene of live_cases."""
    if variant != 'queue':
        return LC.scene(variant)
    boxes, counts = np.zeros((TICKS, Q, D, 4), np.float32), np.zeros((TICKS, Q), np.int32)
    for t in range(TICKS):
        cam0 = ([LC.box_a(t)] if t <= 9 else []) + ([LC.box_c(t)] if t >= 4 else [])
        for q, heads in enumerate((cam0, [LC.box_d(t)])):
            boxes[t, q, :len(heads)], counts[t, q] = np.asarray(heads, np.float32).reshape(-1, 4), len(heads)
    return boxes, counts


def fake_gaze(k, first, lanes):
    """live_cases.fake_gaze over lanes: each value names its (frame, lane, component); the 'smoothed' twins are the negated values."""
    f, p = np.meshgrid(np.arange(first, first + k), np.arange(lanes), indexing='ij')
    base = (f * 10000 + p * 10).astype(np.float32)
    fused = base[..., None] + np.arange(3, dtype=np.float32)
    others = base[..., None, None] + np.arange(3, 12, dtype=np.float32).reshape(3, 3)
    return fused, others, -fused, -others


def run_host_lanes(boxes, counts, lanes, smooth=False, gaze=fake_gaze):
    """-> dict(ticks=[per tick: lane_state, crop_boxes, image_of, lane_of, overflow, matched, ring_id / ring_box / ring_col row, flags,
    track_id], emitted=[(tick it was returned at, first, k)], windows, tables=[(table, first_out)], and the gate's outputs concatenated over
    the frames: track_id, valid, camera, slot, image_of, head_box[, smooth_valid, fused_smooth, others_smooth]).  gaze(k, first, lanes) ->
    (fused, others, fused_smooth, others_smooth) of the returned frames."""
    R = live.ring_depth(CLIP)
    ring_id, ring_col, ring_box = np.zeros((R, lanes), np.int32), np.zeros((R, lanes), np.int32), np.zeros((R, lanes, 4), np.float32)
    lane_state = np.zeros((lanes, 2), np.int32)
    state = np.zeros((Q, track_state_words(S)), np.int32)
    planner, windows, emitted = WindowPlanner(CLIP, STRIDE), [], 0
    out = dict(ticks=[], emitted=[], tables=[], windows=[])
    parts = []

    def emit(tick, ended):
        nonlocal emitted
        k = max(0, planner.final_upto - emitted - int(smooth and not ended))
        if k:
            table, first_out = live.live_gate_table(windows, emitted, k, smooth, tick if ended else None)
            table = live.check_gate_table(table, tick, R)
            g = gaze(k, emitted, lanes) if smooth else (None,) * 4
            parts.append(live.live_gate_lanes_host(ring_id, ring_box, ring_col, Q, S, tick, table, first_out, k, *g))
            out['tables'].append((table, first_out))
        out['emitted'].append((tick, emitted, k))
        emitted += k

    for t in range(len(boxes)):
        res = track_heads_host(boxes[t][:, None], counts[t][:, None], state=state, **LC.OPTIONS)
        state = res[6]
        crop_boxes, image_of, lane_of, matched, overflow = live.live_lanes_host(state, t, lane_state, ring_id, ring_box, ring_col)
        out['ticks'].append(dict(lane_state=lane_state.copy(), crop_boxes=crop_boxes, image_of=image_of, lane_of=lane_of, overflow=overflow,
                                 matched=matched, ring_id=ring_id[t % R].copy(), ring_box=ring_box[t % R].copy(), ring_col=ring_col[t % R].copy(),
                                 flags=res[5].reshape(Q), track_id=res[2].reshape(Q, S)))
        windows += planner.feed(1)
        emit(t, False)
    windows += planner.finish()
    emit(len(boxes) - 1, True)
    out['windows'] = windows
    for name in parts[0]:
        out[name] = np.concatenate([p[name] for p in parts])
    return out
