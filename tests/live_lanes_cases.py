"""The live chain with lanes (mcgaze_amd/live.py, ``LiveGaze(lanes=P)``), shared by tests/test_live_lanes_cpu.py and
tests/test_gpu_live_lanes.py: the scenes of tests/live_cases.py and a second scripted scene, 'queue', in which a person waits for a lane.

'queue': Q = 2 cameras, S = 4 slots, D = 8 detection rows, 28 ticks, max_age = 2, clip 7 / stride 4, and P = 2 lanes for three people.
Camera 0:  A (box_a) detected at ticks 0 .. 9; it coasts at 10 and 11 and its slot is free from tick 12.  C (box_c) detected from tick 4 to
           the end: slot (0, 1), id 2.
Camera 1:  D (box_d) detected at every tick: slot (1, 0), id 1 -- the same id as A, in another camera.
So A holds lane 0 and D lane 1 from tick 0, C waits from tick 4 (overflow 1) and takes lane 0 at tick 12, in the call that releases it.

The whole chain on the host, with the schedule LiveGaze has, is live_cases.run_host(..., lanes=P): track_heads_host, live_lanes_host, the spans
of a WindowPlanner, live_gate_lanes_host."""
import numpy as np

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
