"""Live multi-person gaze with no host step: the tracker's slots as streams of a pool.

``letterbox -> detector -> detect_heads -> track_heads -> head_crops`` leaves one crop per head in device memory, and ``GazeStreamPool``
(merge='device', results='device', smooth=) turns streams of crops into gaze -- but who is in which slot is decided on the device
(mcg_track_heads), while the pool's planning is a host function of how many frames each stream was given.  ``LiveGaze`` joins the two with
a FIXED SCHEDULE: every slot of every camera is a stream that is always open and gets one crop per tick, whether or not a person is in the
slot, and which result rows belong to a person is decided on the device, afterwards:

  * mcg_live_slots (``live_slots_host``): the tracker state -> the crop table of the tick (a live slot's box, matched or coasting; a free
    slot's unusable row), one row of an identity ring ``ring_id[tick % R]`` / ``ring_box[tick % R]``, and ``matched``;
  * mcg_live_gate (``live_gate_host``): per returned frame and slot, ``track_id``, ``valid`` -- every frame of every window merged into the
    row was a crop of that person --, the head box, the arrow table's ``image_of`` and, with smoothing, ``smooth_valid`` and the fall-back of
    the smoothed gaze to the raw one next to an invalid neighbour.

Nothing in a tick waits for the device or copies to the host.  The arithmetic of both kernels is stated in include/mcgaze_hip.h ("live:
tracker slots as streams"); the host twins here are the same bit for bit.  ``live_gate_table`` is the host side of the gate: the spans of
the windows a planner handed out, per returned frame.

``LiveGaze(lanes=P)`` compacts the occupied slots into P streams instead ("live: occupied slots compacted into lanes" in the header):
mcg_live_lanes (``live_lanes_host``) keeps a lane table (id, column) on the device, releases the lanes whose slot lost its person and hands
the free lanes to the waiting slots in a fixed order; mcg_live_gate_lanes (``live_gate_lanes_host``) is the gate over the lanes' ring, with
the same host-built table.  Trunk and decoder work per tick is then P frames, not Q * S.

The gate is stated ONCE, in ``_gate``, over a ring of columns: the slot ring is the lane ring with one column per (camera, slot) whose
identity is its own index, so ``live_gate_host`` and ``live_gate_lanes_host`` share the "usable" rule of an entry, the neighbour rule of
smoothing and the argument checks (live.hip does the same with one kernel)."""
import ctypes as C

import numpy as np
import torch

from . import lib as L
from .arrows import LABEL_CHARS, _anon_params, _label_background, _label_options, _overlay_options, _overlay_palette, heat_lut
from .attention import KIND_HEAD, PolyRegions, PolyRegions3D, _attention_options, _dwell_options, _heat_options, _surface_options, region_label_rows
from .engine import _upload_table
from .harness import _host, check_smooth
from .head_detect import TRACK_HEADER_WORDS, TRACK_MAX_SLOTS, TRACK_SLOT_WORDS, _track_motion, _track_params, track_state_words
from .stream import GazeStreamPool, WindowPlanner

MAX_CAMERAS, MAX_RING, MAX_ENTRIES = 65535, 65536, 65536         # the bounds of mcg_live_slots / mcg_live_gate
MAX_LANES, MAX_COLUMNS = 1024, 4096                              # the bounds of mcg_live_lanes: lanes, cameras x slots
ENTRY = 5                                                        # tick, lo, hi, prev, next


def ring_depth(clip_len):
    """Rows of the identity ring a lockstep LiveGaze needs: 2 * clip_len + 2.  A frame f is handed out at tick f + clip_len (one later with
    smoothing: f + clip_len + 1); the windows that cover it start above f - clip_len, and the gate also reads the span of its predecessor
    f - 1, which starts at f - clip_len at the lowest.  So the ticks f - clip_len .. f + clip_len + 1 are live at once."""
    return 2 * int(clip_len) + 2


def _check_sizes(who, cameras, slots, depth=1, tick=0):
    for name, v, lo, hi in (('cameras', cameras, 0, MAX_CAMERAS), ('slots', slots, 1, TRACK_MAX_SLOTS), ('ring depth', depth, 1, MAX_RING),
                            ('tick', tick, 0, 0x7fffffff)):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} in {lo} .. {hi}, got {v!r}')


def _check_ring(who, ring_id, ring_box, ring_col=None):
    """-> ring_id.shape: (R, Q, S) of the slot ring, or (R, P) of the lane ring (the one with a ring_col)."""
    cols = ring_col is not None
    if ring_id.ndim != (2 if cols else 3) or ring_id.dtype != np.int32 or ring_box.dtype != np.float32 or ring_box.shape != ring_id.shape + (4,) or \
            (cols and (ring_col.dtype != np.int32 or ring_col.shape != ring_id.shape)):
        lead = '[R, P]' if cols else '[R, Q, S]'
        raise ValueError(f'{who}: the ring is ring_id{", ring_col" * cols} int32 {lead} and ring_box float32 {lead[:-1]}, 4], got ' +
                         ', '.join(f'{x.dtype} {x.shape}' for x in (ring_id, ring_col, ring_box) if x is not None))
    return ring_id.shape


def live_slots_host(state, tick, ring_id, ring_box):
    """``mcg_live_slots`` in numpy, bit for bit.  state: int32 [Q, track_state_words(S)] as track_heads_host returns it, after the tick's
    frame; ring_id int32 [R, Q, S] and ring_box float32 [R, Q, S, 4]: row tick % R is WRITTEN.
    -> (crop_boxes float32 [Q * S, 4], image_of int32 [Q * S], matched int32 [Q, S]): head_crops' tables over the tick's Q frames -- a live
    slot's box (a coasting slot keeps its last) with image_of = q, a free slot's zero box with image_of = -1 -- and which slots saw a
    detection in this tick."""
    state = np.asarray(_host(state))
    R, Q, S = _check_ring('live_slots', ring_id, ring_box)
    _check_sizes('live_slots', Q, S, R, tick)
    if state.dtype != np.int32 or state.shape != (Q, track_state_words(S)):
        raise ValueError(f'live_slots: the state of {Q} cameras of {S} slots is an int32 [{Q}, {track_state_words(S)}] array, got {state.dtype} {state.shape}')
    table = np.ascontiguousarray(state[:, TRACK_HEADER_WORDS:]).reshape(Q, S, TRACK_SLOT_WORDS)
    ids, age = table[..., 4], table[..., 5]
    live = ids > 0
    boxes = np.where(live[..., None], np.ascontiguousarray(table[..., :4]).view(np.float32), np.float32(0))
    ring_id[tick % R], ring_box[tick % R] = np.where(live, ids, 0), boxes
    image_of = np.where(live, np.arange(Q, dtype=np.int32)[:, None], -1).astype(np.int32)
    return boxes.reshape(Q * S, 4).copy(), image_of.reshape(Q * S), (live & (age == 0)).astype(np.int32)


def _span(windows, f):
    """The union [lo, hi) of the windows (start, stop, ...) that cover frame f."""
    over = [(w[0], w[1]) for w in windows if w[0] <= f < w[1]]
    if not over:
        raise L.McgError(f'live_gate_table: no window handed out covers frame {f}')
    return min(a for a, _ in over), max(b for _, b in over)


def live_gate_table(windows, first, k, smoothing=False, last=None):
    """The table mcg_live_gate takes for the frames [first, first + k) a lockstep pool handed out -> (int32 [n, 5] = tick, lo, hi, prev, next
    per entry; first_out: the entry of frame ``first``).  One frame per tick: a frame's index is its tick.  windows: the (start, stop,
    overlap) tuples the planner handed out so far (WindowPlanner.feed / finish), the flush-to-end window of finish() included -- [lo, hi) is
    the union of those that cover the frame.  smoothing: prev / next are the frames the filter read -- f - 1 unless f is 0, f + 1 unless f is
    ``last`` (the stream's last frame, known once it has ended) -- and those frames get entries of their own, as neighbours."""
    first, k = int(first), int(k)
    if first < 0 or k < 0:
        raise ValueError(f'live_gate_table: first and k must not be negative (got {first}, {k})')
    if k == 0:
        return np.zeros((0, ENTRY), np.int32), 0
    lo_f = first - 1 if smoothing and first > 0 else first
    hi_f = first + k + (1 if smoothing and first + k - 1 != last else 0)
    table = np.full((hi_f - lo_f, ENTRY), -1, np.int32)
    for i, f in enumerate(range(lo_f, hi_f)):
        table[i, 0] = f
        table[i, 1:3] = _span(windows, f)
        if smoothing and first <= f < first + k:
            table[i, 3], table[i, 4] = (f - 1 if f > 0 else -1), (-1 if f == last else f + 1)
    return table, first - lo_f


def check_gate_table(table, tick, depth):
    """ValueError unless every tick the table names is still in a ring of ``depth`` rows whose newest is ``tick`` -- a span deeper than the ring
    would read rows a later tick has overwritten.  -> the table as a contiguous int32 [n, 5] array."""
    table = np.ascontiguousarray(table, dtype=np.int32)
    if table.ndim != 2 or table.shape[1] != ENTRY or table.shape[0] > MAX_ENTRIES:
        raise ValueError(f'live_gate: the table is int32 [n <= {MAX_ENTRIES}, {ENTRY}] = tick, lo, hi, prev, next; got {table.shape}')
    if len(table):
        t, lo, hi = table[:, 0].astype(np.int64), table[:, 1].astype(np.int64), table[:, 2].astype(np.int64)
        if (t < 0).any() or (lo < 0).any() or (hi < lo).any() or (table[:, 3:] < -1).any() or (t > tick).any() or (hi > tick + 1).any():
            raise ValueError(f'live_gate: an entry names a tick outside 0 .. {tick} or an empty span: {table.tolist()}')
        oldest = min(int(t.min()), int(lo[hi > lo].min()) if (hi > lo).any() else int(t.min()))
        if oldest <= tick - depth:
            raise ValueError(f'live_gate: tick {oldest} has left the identity ring ({depth} rows, newest tick {tick}): a span deeper than the ring')
    return table


def _gate(who, ring_id, ring_col, ring_box, Q, S, tick, table, first_out, num_out, fused, others, fused_smooth, others_smooth):
    """The gate of both entries, stated once, over a ring of C columns: ring_id [R, C], ring_box [R, C, 4] and ring_col [R, C], or None for
    the slot ring, where C = Q * S and a column's identity is its own index.  -> the dict of live_gate_lanes_host, over [k, C]."""
    R, C = ring_id.shape
    _check_sizes(who, Q, S, R, tick)
    table = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, ENTRY)
    n, k = len(table), int(num_out)
    if n > MAX_ENTRIES or first_out < 0 or k < 0 or first_out + k > n or k * C >= 1 << 31:
        raise ValueError(f'{who}: the frames handed out must be entries of the table (first_out {first_out}, num_out {k}, {n} entries)')
    smoothing = [x is not None for x in (fused, others, fused_smooth, others_smooth)]
    if any(smoothing) != all(smoothing):
        raise ValueError(f'{who}: smoothing takes fused, others and both smoothed tables, or none')
    own = np.arange(C, dtype=np.int32)
    column = lambda t: own if ring_col is None else ring_col[t % R]

    def state(j):
        t, lo, hi, prev, nxt = (int(v) for v in table[j])
        old = tick - R
        usable = old < t <= tick and 0 <= lo <= hi <= tick + 1 and (hi == lo or lo > old) and prev >= -1 and nxt >= -1
        if not usable:
            return np.zeros(C, np.int32), np.full(C, -1, np.int32), np.zeros(C, bool)
        ids, col = ring_id[t % R], column(t)
        valid = ids != 0
        for u in range(lo, hi):
            valid = valid & (ring_id[u % R] == ids) & (column(u) == col)
        return ids, col, valid

    def neighbour(tk, ids, col):
        for j in range(n):
            if int(table[j, 0]) == tk:
                idn, cn, vn = state(j)
                return vn & (idn == ids) & (cn == col)
        return np.zeros(C, bool)

    new = lambda fill=0: np.full((k, C), fill, np.int32)
    out = dict(track_id=new(), valid=new(), camera=new(-1), slot=new(-1), image_of=new(-1), head_box=np.zeros((k, C, 4), np.float32))
    if all(smoothing):
        out.update(smooth_valid=new(), fused_smooth=np.array(fused_smooth, dtype=np.float32).reshape(k, C, 3),
                   others_smooth=np.array(others_smooth, dtype=np.float32).reshape(k, C, 3, 3))
        fused, others = np.asarray(fused, dtype=np.float32).reshape(k, C, 3), np.asarray(others, dtype=np.float32).reshape(k, C, 3, 3)
    for i in range(k):
        e = first_out + i
        ids, col, valid = state(e)
        named = valid & (col >= 0) & (col < Q * S)                # every valid row of a slot ring
        out['track_id'][i], out['valid'][i] = ids, valid
        out['camera'][i], out['slot'][i] = np.where(named, col // S, -1), np.where(named, col % S, -1)
        out['image_of'][i] = np.where(named, i * Q + col // S, -1)
        if valid.any():
            out['head_box'][i] = np.where(valid[:, None], ring_box[int(table[e, 0]) % R], np.float32(0))
        if all(smoothing):
            ok = valid.copy()
            for tk in (int(table[e, 3]), int(table[e, 4])):
                if tk != -1:
                    ok &= neighbour(tk, ids, col)
            out['smooth_valid'][i] = ok
            raw = valid & ~ok
            out['fused_smooth'][i][raw], out['others_smooth'][i][raw] = fused[i][raw], others[i][raw]
    return out


def live_gate_host(ring_id, ring_box, tick, table, first_out, num_out, fused=None, others=None, fused_smooth=None, others_smooth=None):
    """``mcg_live_gate`` in numpy, bit for bit.  ring_id / ring_box: the identity ring (live_slots_host), whose newest row is ``tick``; table
    int32 [n, 5] (live_gate_table), entries first_out .. first_out + num_out - 1 the frames handed out.  fused [k, Q, S, 3], others
    [k, Q, S, 3, 3], fused_smooth, others_smooth: all four (smoothing) or none.
    -> dict(track_id, valid, image_of int32 [k, Q, S], head_box float32 [k, Q, S, 4][, smooth_valid, fused_smooth, others_smooth -- copies,
    the raw gaze where a row is valid next to a neighbour that is not]).  An entry that is not usable (a tick outside the ring) gives id 0,
    invalid rows: defined, like the kernel."""
    R, Q, S = _check_ring('live_gate', ring_id, ring_box)
    out = _gate('live_gate', ring_id.reshape(R, Q * S), None, ring_box.reshape(R, Q * S, 4), Q, S, tick, table, first_out, num_out, fused, others,
                fused_smooth, others_smooth)
    return {name: v.reshape((len(v), Q, S) + v.shape[2:]) for name, v in out.items() if name not in ('camera', 'slot')}


def _check_lanes(who, lanes, cameras, slots):
    if isinstance(lanes, bool) or not isinstance(lanes, (int, np.integer)) or not 1 <= lanes <= MAX_LANES:
        raise ValueError(f'{who}: lanes is an int in 1 .. {MAX_LANES}, got {lanes!r}')
    if cameras * slots > MAX_COLUMNS:
        raise ValueError(f'{who}: with lanes, cameras x slots must not exceed {MAX_COLUMNS} (got {cameras} x {slots})')
    return int(lanes)


def live_lanes_host(state, tick, lane_state, ring_id, ring_box, ring_col):
    """``mcg_live_lanes`` in numpy, bit for bit.  state: int32 [Q, track_state_words(S)] after the tick's frame; lane_state int32 [P, 2] =
    (id, column) per lane, UPDATED in place (all zero: every lane free); ring_id, ring_col int32 [R, P] and ring_box float32 [R, P, 4]: row
    tick % R is WRITTEN.  Release: a lane stays held iff id > 0, its column lies in 0 .. Q * S - 1, the slot there still has that id and no
    lower lane holds the same column.  Assign: the live slots no held lane names, in ascending column order, take the free lanes in
    ascending lane order; the rest wait.
    -> (crop_boxes float32 [P, 4], image_of int32 [P] -- head_crops' tables over the tick's Q frames: a held lane's slot box and camera, a
    free lane's zero box and -1 --, lane_of int32 [Q, S] (-1: the slot is free, or live and left out), matched int32 [P], overflow int32 [1]:
    the live slots left without a lane)."""
    state = np.asarray(_host(state))
    R, P = _check_ring('live_lanes', ring_id, ring_box, ring_col)
    if state.ndim != 2 or state.dtype != np.int32 or state.shape[1] < TRACK_HEADER_WORDS + TRACK_SLOT_WORDS or \
            (state.shape[1] - TRACK_HEADER_WORDS) % TRACK_SLOT_WORDS:
        raise ValueError(f'live_lanes: the state of Q cameras of S slots is an int32 [Q, {TRACK_HEADER_WORDS} + {TRACK_SLOT_WORDS} * S] array, got '
                         f'{state.dtype} {state.shape}')
    Q, S = state.shape[0], (state.shape[1] - TRACK_HEADER_WORDS) // TRACK_SLOT_WORDS
    _check_sizes('live_lanes', Q, S, R, tick)
    _check_lanes('live_lanes', P, Q, S)
    if lane_state.dtype != np.int32 or lane_state.shape != (P, 2):
        raise ValueError(f'live_lanes: the lane state of {P} lanes is an int32 [{P}, 2] array, got {lane_state.dtype} {lane_state.shape}')
    table = np.ascontiguousarray(state[:, TRACK_HEADER_WORDS:]).reshape(Q * S, TRACK_SLOT_WORDS)
    ids, age, box = table[:, 4], table[:, 5], np.ascontiguousarray(table[:, :4]).view(np.float32)
    lane_of = np.full(Q * S, -1, np.int32)
    for p in range(P):                                           # 1. release
        i, c = int(lane_state[p, 0]), int(lane_state[p, 1])
        if i > 0 and 0 <= c < Q * S and ids[c] == i and lane_of[c] == -1:
            lane_of[c] = p
        else:
            lane_state[p] = 0
    free = [p for p in range(P) if lane_state[p, 0] == 0]
    waiting = [c for c in range(Q * S) if ids[c] > 0 and lane_of[c] == -1]
    for p, c in zip(free, waiting):                              # 2. assign
        lane_state[p], lane_of[c] = (ids[c], c), p
    held = lane_state[:, 0] != 0                                 # 3. outputs
    col = lane_state[:, 1]
    crop_boxes = np.where(held[:, None], box[col], np.float32(0))
    row = tick % R
    ring_id[row], ring_box[row], ring_col[row] = lane_state[:, 0], crop_boxes, np.where(held, col, -1)
    image_of = np.where(held, col // S, -1).astype(np.int32)
    matched = (held & (age[col] == 0)).astype(np.int32)
    return crop_boxes, image_of, lane_of.reshape(Q, S), matched, np.array([max(0, len(waiting) - len(free))], np.int32)


def live_gate_lanes_host(ring_id, ring_box, ring_col, cameras, slots, tick, table, first_out, num_out, fused=None, others=None, fused_smooth=None,
                         others_smooth=None):
    """``mcg_live_gate_lanes`` in numpy, bit for bit: live_gate_host over the P columns of the lane ring (live_lanes_host), a lane's identity
    being the pair (ring_id, ring_col) -- ids are per camera.  table, first_out, num_out as for live_gate_host; fused [k, P, 3], others
    [k, P, 3, 3], fused_smooth, others_smooth: all four (smoothing) or none.
    -> dict(track_id, valid, camera, slot, image_of int32 [k, P], head_box float32 [k, P, 4][, smooth_valid, fused_smooth, others_smooth]).
    camera / slot name the slot the lane held at the frame's tick and image_of is i * Q + camera, all three -1 on invalid rows."""
    _, P = _check_ring('live_gate_lanes', ring_id, ring_box, ring_col)
    _check_lanes('live_gate_lanes', P, int(cameras), int(slots))
    return _gate('live_gate_lanes', ring_id, ring_col, ring_box, int(cameras), int(slots), tick, table, first_out, num_out, fused, others, fused_smooth,
                 others_smooth)


def _clone_frame(f):
    if isinstance(f, (tuple, list)):
        return tuple(_clone_frame(p) for p in f)
    return f.clone(memory_format=torch.contiguous_format) if isinstance(f, torch.Tensor) else np.array(f)


class LiveGaze:
    """Frames in, gaze for every tracked head a few ticks later, with no host step in between.

        live = LiveGaze(engine_or_model, pipeline, cameras=Q, slots=S, smooth=0.6)
        r = live.tick(frames, boxes, counts)     # frames: Q device frames; boxes [Q, D, 4], counts [Q] as detect_heads emits them
        ...
        r = live.finish()

    ``tick`` runs, on the current stream of the engine's device: track_heads (the state is kept here), mcg_live_slots, head_crops, one push
    per (camera, slot) stream of an internal GazeStreamPool(merge='device', results='device', smooth=smooth) whose Q * S streams were opened
    at construction, pool.step(), mcg_live_gate and, with draw=True, pipeline.draw_arrows on copies of the frames of the returned ticks
    (the gated boxes, ``fused_smooth`` if smoothing, else ``fused``).  It returns device tensors stacked over the k frames that became final
    (k may be 0): first (a host int: the tick of row 0), track_id, valid [k, Q, S] int32, head_box [k, Q, S, 4], det [k, Q, S, 3, 5] (boxes
    in the crop's resized pixels), fused [k, Q, S, 3], others [k, Q, S, 3, 3], image_of [k, Q, S] (draw_arrows' table over the k * Q returned
    frames; -1 on invalid rows), with smoothing fused_smooth, others_smooth, smooth_valid, the tick's own ``flags`` [Q] (the tracker's) and
    ``matched`` [Q, S], and with draw ``frames``: k lists of Q annotated frames.  ``finish`` returns the rest (no flags / matched).
    Neither waits for the device or copies to the host.

    What the rows mean: windows are aligned to the tick count, so a row is ``valid`` -- every frame of every window merged into it was a
    crop of the person ``track_id`` -- from the first multiple of ``stride`` at or after the person's birth tick, plus clip_len - stride, and
    symmetrically before the slot is freed; a slot that coasts (up to max_age missed detections) keeps its last box and stays valid; a
    slot handed to another person yields invalid rows around the hand-over.  det / fused / others are never altered: of an invalid row
    they are what the network made of a mixture or of an empty slot's crop (pixel (0, 0) of frame 0).  Where a row is valid but a
    neighbour the filter read is not, fused_smooth / others_smooth are the raw gaze (smooth_valid 0).  All S slots of every camera go
    through the network every tick.  The fp16 engine (precision 'f16') needs max_decode_windows <= 12 at clip_len 7, as for any pool.

    LANES.  ``lanes=None`` is everything above.  ``lanes=P`` (an int in 1 .. 1024, with cameras * slots <= 4096) gives the pool P streams
    instead of Q * S: mcg_live_lanes decides on the device, every tick, which live slot holds which lane -- a person keeps the lane for as
    long as they keep the slot; the live slots that hold none take the free lanes in ascending (camera, slot) / ascending lane order --, and
    head_crops, the trunk and the decoder run over P rows a tick.  P should be the most people expected at once over ALL cameras; a slot
    table is sized for the worst case per camera, P for the scene.  A tick then runs track_heads, mcg_live_lanes, head_crops over P rows,
    P pushes, pool.step(), mcg_live_gate_lanes and the drawing, still with no wait for the device and no copy to the host, and with host
    work that does not depend on who is in the picture.  The results are per LANE: track_id, valid, camera, slot, image_of [k, P] int32
    (camera / slot: the slot the lane held at the frame's tick, -1 on invalid rows; image_of = i * Q + camera), head_box [k, P, 4], det
    [k, P, 3, 5], fused [k, P, 3], others [k, P, 3, 3] and the smoothed tables likewise; every tick also returns flags [Q], matched [P],
    lane_of [Q, S] (the lane of each slot, -1 if the slot is free or was left out) and overflow [1] (the live slots left without a lane in
    this tick).  A row means what it means above with the LANE GRANT tick in place of the birth tick: a person is valid from the first
    multiple of ``stride`` at or after the tick they got a lane, plus clip_len - stride, and symmetrically before the slot is freed; a lane
    handed from one person to another (it can happen within one tick) yields invalid rows around the hand-over; a person left out by
    overflow has no rows until a lane frees, and is a candidate again every tick.  ``ring_depth`` is unchanged.

    MOTION.  ``motion=None`` is everything above.  ``motion=True`` or ``dict(gain=0.5, decay=1.0)`` (pipeline.track_heads' option: conventional
    alpha-beta values, not tuned on data) runs the tracker with its constant-velocity model (mcg_track_heads_motion): a head that is missed
    for a few ticks is looked for where its velocity takes it, so it keeps its id, slot and lane where the plain tracker would have given
    birth to a new person, and the box a coasting slot's crop is cut at is the PREDICTED one -- mcg_live_slots / mcg_live_lanes read it from
    the state as before.

    ATTENTION.  ``attention=None`` is everything above.  ``attention=True`` or ``dict(regions=, expand=0.25, camera_angle=10.0)`` adds what
    every returned row looks at (pipeline.gaze_targets, mcg_gaze_targets: one call per tick that returns frames, over the gated head_box, the
    gaze that ``draw`` uses and the gate's image_of, so an invalid row looks at nothing and nothing looks at it): target_kind (0 none, 1 head,
    2 region, 3 camera), target (the slot of the person looked at -- with lanes their lane --, or the region's index, else -1), target_id (that
    person's track_id, else 0), target_t, target_hit [.., 2] (where the ray from the head's centre enters the target, in frame pixels) and
    mutual (the two look at each other), shaped like track_id.  regions: a list of Q tables [m_q, 4] of rectangles x1 y1 x2 y2 in frame
    pixels, one per camera (None: none there), uploaded once; a region's index counts through the cameras' tables in order.  A camera's
    table may also be the mixed list of attention.region_polygons -- rectangles and polygons [[x, y], ...] of 3 .. 32 vertices, a screen seen
    off-axis, an L-shaped shelf --: then the call is mcg_gaze_targets_poly, and a polygon is a region index like any other.  Targets are
    decided in the image plane, and expand / camera_angle are conventions, not tuned on data.  Still no wait for the device, no copy to the
    host.
    With ``camera=[fx, fy, cx, cy]`` (or one such row per camera) in the dict the tick's call is pipeline.gaze_targets_3d instead
    (mcg_gaze_targets_3d: targets decided in camera space, depth from the size of the head): ``regions3d=`` a list of Q lists of planar
    polygons [[x, y, z], ...] in that camera's coordinates (None: none there), ``head_size=0.24`` metres and ``frame='eye'`` (conventions,
    not tuned on data).  Every table above keeps its name -- target_hit is the 3-D point projected to frame pixels, NaN where it is not in
    front of the lens, and a region's index counts through regions3d --, target_hit3d [.., 3] is added, and dwell, heat, overlay and labels
    run on top unchanged; ``regions=`` are then only what the overlay draws and the labels name.

    OVERLAY.  ``overlay=True`` or ``dict(palette=, line_thickness=, region_thickness=)`` (it needs ``draw`` and ``attention``; ValueError
    without) draws the frames with pipeline.draw_attention instead of draw_arrows, from the gated tables and the per-camera regions: region
    outlines (lit where somebody looks at them), sight lines to the hit points, arrows coloured by their target.  Every table comes back as
    without it, and the tick still never waits for the device.
    LABELS.  ``labels=True`` or ``dict(scale=2, advance=6, pad=1, background=(0, 0, 0), fps=(30, 1), region_names=None)`` (it needs ``draw``;
    ValueError without) writes words into the returned frames after the arrows or the overlay: per returned frame one pipeline.format_labels
    call makes '#<track_id>' for every valid row -- with ``dwell`` followed by the seconds of dwell_frames at fps = (num, den) -- into the tail
    of one preallocated text table, and one pipeline.draw_labels call draws it above the head boxes, in the arrow's colour (with ``overlay``
    in palette[4 if mutual else kind], gathered on the device).  region_names: one list of names per camera, a name (or None) per region of
    that camera's ``attention`` regions (ValueError without them); they are drawn inside the regions' top-left corners in palette[5], in front
    of the row labels in the tables, so head labels win.  Every other table comes back as without it; still no wait for the device.
    DWELL.  ``dwell=None`` is everything above.  ``dwell=True`` or ``dict(enter=3, exit=2)`` (it needs ``attention``; ValueError without) adds how
    LONG every row has looked at its target (pipeline.gaze_dwell, mcg_gaze_dwell: one call per tick that returns frames, over the k frames
    handed out, frame0 = first).  A column is a slot or a lane; its owner is person = track_id where valid, else 0, with lanes tagged by the
    ring column camera * S + slot (ids are per camera); the target's identity is target_id for a head and the region's index for a region.
    An observation becomes the current target after ``enter`` consecutive frames and its episode ends after ``exit`` consecutive frames
    without it (conventions, not tuned on data).  The result gains dwell_kind, dwell_id, dwell_start, dwell_frames, shaped like track_id
    (the current target after each frame: its kind, its identity, the frame it began in, its frames so far), ``episodes`` [k * columns, 10]
    int32 (attention.EVENT_FIELDS: the episodes that ENDED in these frames, in ascending (frame, column); rows behind the count are zero) and
    ``num_episodes`` int32 [1].  ``LiveGaze.region_frames`` holds the person-frames every region has collected so far, int32 [m] on the
    device, and ``LiveGaze.dwell_state`` the state [columns, 16] (attention.STATE_WORDS): episodes still open -- after finish() too, which
    adds nothing beyond its frames -- are read there.  Still no wait for the device, no copy to the host.
    HEAT.  ``heat=None`` is everything above.  ``heat=True`` or ``dict(cell=8, radius=2, decay=0, kinds=('head', 'region'), draw=True,
    full_scale=None, min_level=1)`` (it needs ``attention``; ValueError without) accumulates WHERE in the picture looks land
    (pipeline.gaze_heat, mcg_gaze_heat_add; include/mcgaze_hip.h, "gaze heat map"): per returned frame one call over that frame's rows --
    target_hit, target_kind, image_of, mask = valid, period = Q, so every camera has its own grid of ``cell``-pixel cells, made at the first
    tick from the size of its frames (one size for all cameras) -- whose grid decays by h >> decay before the frame's looks are added.  Every
    tick gains ``heat`` int32 [Q, GH, GW] and ``heat_peak`` int32 [Q]: the LIVE device tensors (``LiveGaze.heat_state``), which later ticks
    go on updating; None before the first tick.  With draw=True (it needs ``draw``; ValueError without; heat=True draws where draw does) the
    grid as it stands after a frame's looks is blended into that frame's pictures FIRST (pipeline.draw_heat with full_scale and min_level),
    under the arrows, the overlay and the labels.  Still no wait for the device, no copy to the host.
    SURFACE HEAT.  ``surface_heat=None`` is everything above.  ``surface_heat=True`` or ``dict(grid=(32, 32), radius=1, decay=0, draw=True,
    full_scale=None, min_level=1)`` (it needs attention=dict(camera=..., regions3d=...); ValueError without) accumulates WHERE ON each
    planar region looks land, in the region's own coordinates (pipeline.surface_heat, mcg_surface_heat_add; include/mcgaze_hip.h, "surface
    heat map"): per returned frame one call over that frame's rows -- target_hit3d, target_kind, target, mask = valid -- into one grid of
    GW x GH cells per region of regions3d, counted through the cameras as ``target`` counts them; the grid and the radius are
    conventions, not tuned on data.  Every tick gains ``surface_heat`` int32 [M, GH, GW] and ``surface_heat_peak`` int32 [M]: the LIVE
    device tensors (``LiveGaze.surface_heat_state``, made with the object; the caller may set them).  With draw=True (it needs ``draw``;
    ValueError without; surface_heat=True draws where draw does) the grids as they stand after a frame's looks are drawn back onto their
    regions in that frame's pictures with the right perspective (pipeline.draw_surface_heat), AFTER the image-plane heat map and before
    the arrows, the overlay and the labels.  Still no wait for the device, no copy to the host.
    ANONYMIZE.  ``anonymize=None`` is everything above.  ``anonymize=True`` or a dict of pipeline.anonymize_heads' options (expand, shape,
    cell, blocks, mode, color; it needs ``draw``; ValueError without) removes the faces from the returned frames (include/mcgaze_hip.h,
    "anonymised heads"): one call per tick that returns frames, over the kept copies, from head_box and image_of of the gated rows -- a row
    that is not valid has image_of -1 and hides nothing -- BEFORE the heat map is blended and anything is drawn.  The network has read the
    frames by then: every table comes back as without it.  It hides the heads the tracker holds: a head the detector missed stays visible.
    Still no wait for the device, no copy to the host."""

    def __init__(self, engine_or_model, pipeline, cameras, slots=16, clip_len=7, stride=4, expand=0.8, match_iou=0.3, max_age=5, smooth=None,
                 pixel_format='bgr', draw=False, matrix='bt601', rgb=False, person_threshold=0.5, max_decode_windows=None, lanes=None, motion=None,
                 attention=None, dwell=None, overlay=None, labels=None, heat=None, anonymize=None, surface_heat=None):
        self.S, self.match_iou, self.max_age = _track_params(slots, match_iou, max_age)
        _track_motion(motion, 'LiveGaze')
        self.motion = motion
        _check_sizes('LiveGaze', cameras, self.S)
        if cameras < 1:
            raise ValueError(f'LiveGaze: at least one camera (got {cameras})')
        self.P = None if lanes is None else _check_lanes('LiveGaze', lanes, int(cameras), self.S)
        self.Q, self.T, self.s = int(cameras), int(clip_len), int(stride)
        self.smooth = check_smooth('LiveGaze', smooth)
        attention = _attention_options('LiveGaze', attention, self.Q)
        self.dwell = _dwell_options('LiveGaze', dwell, attention)
        self.overlay = _overlay_options('LiveGaze', overlay, draw, attention)
        self.labels = _label_options('LiveGaze', labels, draw)
        self.heat, self.heat_state = _heat_options('LiveGaze', heat, attention, draw), None
        self.surface_heat, self.surface_heat_state = _surface_options('LiveGaze', surface_heat, attention, draw), None
        if anonymize is not None and not draw:
            raise ValueError('LiveGaze: anonymize changes the returned frames; it needs draw')
        self.anonymize = None if anonymize is None else {} if anonymize is True else dict(anonymize)
        if self.anonymize is not None:
            if set(self.anonymize) - {'expand', 'shape', 'cell', 'blocks', 'mode', 'color'}:
                raise ValueError(f'LiveGaze: anonymize is True or a dict of expand, shape, cell, blocks, mode, color; got {sorted(self.anonymize)}')
            _anon_params('LiveGaze(anonymize=...)', **{k: v for k, v in self.anonymize.items() if k != 'color'})
        self.pipe, self.expand, self.draw = pipeline, float(expand), bool(draw)
        self.frame_options = dict(pixel_format=pixel_format, matrix=matrix)
        self.rgb = bool(rgb)
        _, _, pad_h, pad_w, _ = pipeline.head_crop_geometry()
        # the pool's streams, and what the gate says of a row besides: every slot, or the lanes and the slot each held
        self.lead, self.extra = ((self.Q, self.S), ()) if self.P is None else ((self.P,), ('camera', 'slot'))
        n = int(np.prod(self.lead))
        self.pool = GazeStreamPool(engine_or_model, pad_h, pad_w, clip_len, stride, rows=n * (clip_len + stride + 1), person_threshold=person_threshold,
                                   max_decode_windows=max_decode_windows, max_trunk_frames=max(448, n), merge='device', results='device', smooth=self.smooth)
        self.sids = [self.pool.open() for _ in range(n)]
        self.dev = torch.device(self.pool.e.device)
        self.lib = L.load()
        self.R = ring_depth(clip_len)
        new = lambda *shape, dtype=torch.int32: torch.zeros(*shape, dtype=dtype, device=self.dev)
        self.ring_id, self.ring_box = new(self.R, *self.lead), new(self.R, *self.lead, 4, dtype=torch.float32)
        if self.P is not None:
            self.ring_col, self.lane_state = new(self.R, self.P), new(self.P, 2)
        self.crop_boxes, self.image_of = new(n, 4, dtype=torch.float32), new(n)
        self.state = new(self.Q, track_state_words(self.S))
        self.planner = WindowPlanner(clip_len, stride)           # fed like every stream of the pool: the windows they were handed
        self.windows, self.kept = [], {}
        self.ticks = self.emitted = 0
        self.finished = False
        self.attention = self.attention3d = None
        if attention is not None:                                # the regions go up once: region_image = camera, matched through region_period = Q
            regions, region_image, options = attention
            up = lambda t: torch.from_numpy(t).to(self.dev)
            three_d = options.pop('three_d', None)               # camera=: mcg_gaze_targets_3d decides, its tables go up once as well
            if three_d is not None:
                self.attention3d = dict(options, cam=up(three_d['cam']), regions=PolyRegions3D(*map(up, three_d['regions'])),
                                        region_image=up(three_d['region_image']), head_size=three_d['head_size'], frame=three_d['frame'])
            regions = PolyRegions(*map(up, regions)) if isinstance(regions, PolyRegions) else up(regions)      # (a polygon somewhere: the vertex form)
            self.attention = dict(options, regions=regions, region_image=up(region_image))
        if self.surface_heat is not None:                        # one grid per region of regions3d, in the region's own coordinates
            self.surface_heat_state = pipeline.surface_heat_state(len(three_d['region_image']), grid=self.surface_heat['grid'], device=self.dev)
        if self.dwell is not None:
            counted = attention[1] if self.attention3d is None else self.attention3d['region_image']
            self.dwell_state, self.region_frames = pipeline.dwell_state(n, device=self.dev), new(len(counted))
        if self.labels is not None:
            self._label_tables(attention, n, matrix)

    def _label_tables(self, attention, n, matrix):
        """labels=: the tables of the one draw_labels call per returned frame, allocated once -- the rows of the named regions of the Q
        pictures of a frame in front (built here, on the host, once), the n row labels behind them, so that head labels win an overlap."""
        names = self.labels.pop('region_names')
        boxes, image_of, text = np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros((0, LABEL_CHARS), np.uint8)
        if names is not None:
            if attention is None:
                raise ValueError('LiveGaze: region_names names the regions of attention: it needs attention with regions')
            if len(names) != self.Q or any(not isinstance(c, (list, tuple, type(None))) for c in names):
                raise ValueError(f'LiveGaze: region_names is one list of names per camera ({self.Q}), a name per region of that camera; got {names!r}')
            boxes, image_of, text, _ = region_label_rows(attention[0], attention[1], [s for c in names for s in (c or ())], self.Q, region_period=self.Q)
        r = self.label_regions = len(boxes)
        nv12 = self.frame_options['pixel_format'] == 'nv12'
        up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(self.dev)
        palette = _overlay_palette('LiveGaze', None if self.overlay is None else self.overlay.get('palette'), nv12, matrix)
        self.label_palette = up(palette)                          # in the frames' own format: a device colour table is read as it is
        self.label_boxes = up(np.concatenate([boxes, np.zeros((n, 4), np.float32)]))
        self.label_image_of = up(np.concatenate([image_of, np.full(n, -1, np.int32)]))
        self.label_text = up(np.concatenate([text, np.zeros((n, LABEL_CHARS), np.uint8)]))
        # region names in the outline's colour, row labels in the arrow's (with overlay: gathered per row, every frame)
        self.label_colors = up(np.concatenate([np.tile(palette[5], (r, 1)), np.tile(palette[0], (n, 1))]).astype(np.uint8))
        # a HOST table: with it the frame table of the fresh frames travels pinned through the staging ring, not as a pageable upload
        self.label_place = np.concatenate([np.ones(r, np.int32), np.zeros(n, np.int32)])
        _label_background(self.labels['background'], nv12, matrix)

    def _draw_labels(self, out, images, i):
        """labels=: the words of returned frame i into its Q drawn frames -- one format_labels call into the tail of the text buffer, one
        draw_labels call."""
        r, Q = self.label_regions, self.Q
        fps, options = self.labels['fps'], {k: v for k, v in self.labels.items() if k != 'fps'}
        ids = torch.where(out['valid'][i] != 0, out['track_id'][i], torch.zeros_like(out['track_id'][i])).reshape(-1)
        values = out['dwell_frames'][i].reshape(-1) if self.dwell is not None else None
        self.pipe.format_labels(ids, values, rate=fps, out=self.label_text[r:], device=self.dev)
        self.label_boxes[r:].copy_(out['head_box'][i].reshape(-1, 4))
        image_of = out['image_of'][i].reshape(-1)
        self.label_image_of[r:].copy_(torch.where(image_of >= 0, image_of - i * Q, image_of))
        if self.overlay is not None:
            kind, mutual = out['target_kind'][i].reshape(-1), out['mutual'][i].reshape(-1)
            index = torch.where(mutual != 0, torch.full_like(kind, 4), torch.where((kind >= 1) & (kind <= 3), kind, torch.zeros_like(kind)))
            self.label_colors[r:].copy_(self.label_palette[index.long()])
        self.pipe.draw_labels(images[i * Q:(i + 1) * Q], self.label_boxes, self.label_image_of, self.label_text, colors=self.label_colors,
                              place=self.label_place, device=self.dev, **self.frame_options, **options)

    def _call(self, name, *args):
        """One entry of the library on the current stream: a tensor goes as its address, None as a null pointer, an int as it is."""
        ptr = lambda a: C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else C.c_void_p(0) if a is None else a
        L.check(getattr(self.lib, name)(C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream), *map(ptr, args)), name)

    def _assign(self):
        """The tick's crop table (crop_boxes, image_of) and ring row from the tracker state -> what the tick returns of it."""
        new = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=self.dev)
        matched = new(*self.lead)
        if self.P is None:
            self._call('mcg_live_slots', self.state, self.Q, self.S, self.ticks, self.R, self.crop_boxes, self.image_of, self.ring_id, self.ring_box,
                       matched)
            return dict(matched=matched)
        lane_of, overflow = new(self.Q, self.S), new(1)
        self._call('mcg_live_lanes', self.state, self.Q, self.S, self.P, self.ticks, self.R, self.lane_state, self.crop_boxes, self.image_of,
                   self.ring_id, self.ring_box, self.ring_col, lane_of, matched, overflow)
        return dict(matched=matched, lane_of=lane_of, overflow=overflow)

    def _gate(self, plan, num_entries, first_out, k, out):
        """The gate over the k frames handed out, into the tables of ``out``."""
        smooth = [out[name] if self.smooth is not None else None for name in ('fused', 'others', 'fused_smooth', 'others_smooth')]
        table = [self.ticks - 1, plan, num_entries, first_out, k, *smooth, out['track_id'], out['valid']]
        tail = [out['head_box'], out['image_of'], out.get('smooth_valid')]
        if self.P is None:
            self._call('mcg_live_gate', self.ring_id, self.ring_box, self.R, self.Q, self.S, *table, *tail)
        else:
            self._call('mcg_live_gate_lanes', self.ring_id, self.ring_box, self.ring_col, self.R, self.Q, self.S, self.P, *table, out['camera'],
                       out['slot'], *tail)

    def _targets(self, out, k):
        """attention=: what every gated row looks at, over the k * Q pictures handed out -> the tables _emit adds."""
        lead = self.lead
        if k:
            gaze = out['fused_smooth' if self.smooth is not None else 'fused']
            if self.attention3d is not None:                     # (pictures are numbered i * Q + camera: both periods are Q)
                kind, target, t, hit, mutual, _, hit3d = self.pipe.gaze_targets_3d(out['head_box'].view(-1, 4), gaze.view(-1, 3), out['image_of'].view(-1),
                                                                                   region_period=self.Q, cam_period=self.Q, device=self.dev,
                                                                                   **self.attention3d)
            else:
                kind, target, t, hit, mutual, _ = self.pipe.gaze_targets(out['head_box'].view(-1, 4), gaze.view(-1, 3), out['image_of'].view(-1),
                                                                         region_period=self.Q, device=self.dev, **self.attention)
            head = kind == KIND_HEAD
            # a head's target is a flat row of [k, Q, S] / [k, P]: its id is gathered there, and what is handed back is the index within
            # the picture's rows -- the slot (the same camera, since the same picture) or the lane
            target_id = torch.where(head, out['track_id'].view(-1)[target.clamp(min=0).long()], torch.zeros_like(kind))
            target = torch.where(head, target % lead[-1], target)
        else:
            new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=self.dev)
            kind, target, target_id, mutual, t, hit = new(0), new(0), new(0), new(0), new(0, dtype=torch.float32), new(0, 2, dtype=torch.float32)
            hit3d = new(0, 3, dtype=torch.float32)
        tables = dict(target_kind=kind.view(k, *lead), target=target.view(k, *lead), target_id=target_id.view(k, *lead), target_t=t.view(k, *lead),
                      target_hit=hit.view(k, *lead, 2), mutual=mutual.view(k, *lead))
        if self.attention3d is not None:
            tables['target_hit3d'] = hit3d.view(k, *lead, 3)
        return tables

    def _dwell(self, out, k):
        """dwell=: the targets of the k frames handed out, accumulated into dwell_state and region_frames -> the tables _emit adds."""
        lead = self.lead
        rows = lambda t: t.reshape(k, len(self.sids))             # (k may be 0)
        person = torch.where(out['valid'] != 0, out['track_id'], torch.zeros_like(out['track_id']))
        tag = None if self.P is None else rows(out['camera'] * self.S + out['slot'])
        ident = torch.where(out['target_kind'] == KIND_HEAD, out['target_id'], out['target'])
        dwell, _, events, num, _, _ = self.pipe.gaze_dwell(rows(person), rows(out['target_kind']), rows(ident), rows(out['mutual']), tag=tag,
                                                           state=self.dwell_state, frame0=self.emitted, region_frames=self.region_frames,
                                                           device=self.dev, **self.dwell)
        dwell = dwell.view(k, *lead, 4)
        return dict(dwell_kind=dwell[..., 0], dwell_id=dwell[..., 1], dwell_start=dwell[..., 2], dwell_frames=dwell[..., 3], episodes=events,
                    num_episodes=num)

    def _heat(self, out, k, images):
        """heat=: the hit points of each of the k frames handed out into the grids, and with draw the grids as they then stand into that
        frame's Q pictures (``images``: the kept copies, drawn in place) -> the tables _emit adds."""
        state, o, Q = self.heat_state, self.heat, self.Q
        for i in range(k):
            self.pipe.gaze_heat(out['target_hit'][i].reshape(-1, 2), out['target_kind'][i].reshape(-1), out['image_of'][i].reshape(-1), state,
                                mask=out['valid'][i].reshape(-1), radius=o['radius'], kinds=o['kinds'], period=Q, decay=o['decay'], device=self.dev)
            if o['draw']:
                # the ramp as a HOST table: with it the frame table of the fresh frames travels pinned through the staging ring
                self.pipe.draw_heat(images[i * Q:(i + 1) * Q], state, lut=heat_lut(None, self.frame_options['pixel_format'] == 'nv12', self.frame_options['matrix']),
                                    full_scale=o['full_scale'], min_level=o['min_level'], device=self.dev, **self.frame_options)
        return dict(heat=None if state is None else state.heat, heat_peak=None if state is None else state.peak)

    def _surface_heat(self, out, k, images):
        """surface_heat=: the 3-D hit points of each of the k frames handed out into the grids of their regions, and with draw the grids as
        they then stand drawn back onto the regions in that frame's Q pictures (``images``: the kept copies, drawn in place) -> the tables
        _emit adds."""
        state, o, Q, a = self.surface_heat_state, self.surface_heat, self.Q, self.attention3d
        for i in range(k):
            self.pipe.surface_heat(out['target_hit3d'][i].reshape(-1, 3), out['target_kind'][i].reshape(-1), out['target'][i].reshape(-1), a['regions'],
                                   state, mask=out['valid'][i].reshape(-1), radius=o['radius'], decay=o['decay'], device=self.dev)
            if o['draw']:                                         # (picture p of a frame is camera p: no periods; the ramp as a HOST table, as _heat has it)
                self.pipe.draw_surface_heat(images[i * Q:(i + 1) * Q], state, a['cam'], a['regions'], a['region_image'],
                                            lut=heat_lut(None, self.frame_options['pixel_format'] == 'nv12', self.frame_options['matrix']),
                                            full_scale=o['full_scale'], min_level=o['min_level'], device=self.dev, **self.frame_options)
        return dict(surface_heat=state.heat, surface_heat_peak=state.peak)

    def tick(self, frames, boxes, counts):
        """One frame per camera and its detections -> the frames that became final (see the class)."""
        if self.finished:
            raise L.McgError('LiveGaze: tick() after finish()')
        frames = list(frames)
        if len(frames) != self.Q or boxes.ndim != 3 or (boxes.shape[0], boxes.shape[2]) != (self.Q, 4) or tuple(counts.shape) != (self.Q,):
            raise ValueError(f'LiveGaze.tick: {self.Q} frames, boxes [{self.Q}, D, 4] and counts [{self.Q}] (got {len(frames)} frames, '
                             f'{tuple(boxes.shape)}, {tuple(counts.shape)})')
        with torch.cuda.device(self.dev):
            if self.heat is not None and self.heat_state is None:  # the grids, from the size of the first frames
                f = frames[0][0] if isinstance(frames[0], (tuple, list)) else frames[0]
                hw = (f.shape[0] * 2 // 3, f.shape[1]) if self.frame_options['pixel_format'] == 'nv12' and not isinstance(frames[0], (tuple, list)) else f.shape[:2]
                self.heat_state = self.pipe.heat_state(self.Q, hw, cell=self.heat['cell'], device=self.dev)
            out = self.pipe.track_heads(boxes[:, None], counts[:, None], state=self.state, slots=self.S, match_iou=self.match_iou, max_age=self.max_age,
                                        device=self.dev, motion=self.motion)
            more = dict(flags=out[5].reshape(self.Q), **self._assign())
            img, img_hw, _, _, _ = self.pipe.head_crops(frames, self.crop_boxes, self.image_of, expand=self.expand, device=self.dev, rgb=self.rgb,
                                                        **self.frame_options)
            for j, sid in enumerate(self.sids):
                self.pool.push(sid, img[j:j + 1], img_hw[j:j + 1])
            res = self.pool.step()
            if self.draw:                                         # the caller's buffers may be a decoder's, rewritten before the tick is returned
                self.kept[self.ticks] = [_clone_frame(f) for f in frames]
            self.ticks += 1
            self.windows += self.planner.feed(1)
            return self._emit(res, **more)

    def finish(self):
        """The cameras ended: the windows that depend on the length, and every frame not returned yet."""
        if self.finished:
            raise L.McgError('LiveGaze: finish() called twice')
        with torch.cuda.device(self.dev):
            for sid in self.sids:
                self.pool.close(sid)
            res = self.pool.step()
            self.finished = True
            self.windows += self.planner.finish()
            return self._emit(res)

    def _emit(self, res, **more):
        Q, lead, smoothing = self.Q, self.lead, self.smooth is not None
        upto = self.planner.final_upto
        k = max(0, upto - self.emitted - int(smoothing and not self.finished))
        got = [res.get(sid) for sid in self.sids]
        shapes = {(r['first'], int(r['det'].shape[0])) for r in got if r is not None}
        if (shapes - {(self.emitted, k)}) or (k and any(r is None for r in got)):
            raise L.McgError(f'LiveGaze: the streams left lockstep -- frames [{self.emitted}, {self.emitted + k}) were due from each of {len(self.sids)} '
                             f'streams, {sum(r is not None for r in got)} returned (first, k) = {sorted(shapes)}')
        names = ('det', 'fused', 'others') + (('fused_smooth', 'others_smooth') if smoothing else ())
        tail = dict(det=(3, 5), fused=(3,), others=(3, 3), fused_smooth=(3,), others_smooth=(3, 3))
        if k:
            parts = {name: torch.stack([r[name] for r in got], dim=1).reshape((k,) + lead + tail[name]) for name in names}
        else:
            parts = {name: torch.empty((0,) + lead + tail[name], dtype=torch.float32, device=self.dev) for name in names}
        new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=self.dev)
        gate = dict(track_id=new(k, *lead), valid=new(k, *lead), head_box=new(k, *lead, 4, dtype=torch.float32), image_of=new(k, *lead))
        gate.update({name: new(k, *lead) for name in self.extra + (('smooth_valid',) if smoothing else ())})
        out = dict(first=self.emitted, **gate, **parts, **more)
        if k:
            table, first_out = live_gate_table(self.windows, self.emitted, k, smoothing, self.ticks - 1 if self.finished else None)
            table = check_gate_table(table, self.ticks - 1, self.R)
            self._gate(_upload_table(table, self.dev), len(table), first_out, k, out)
            self.windows = [w for w in self.windows if w[1] > self.emitted + k - 1]     # the next call's first neighbour is the last frame of this
        if self.attention is not None:
            out.update(self._targets(out, k))
        if self.dwell is not None:
            out.update(self._dwell(out, k))
        images = [f for t in range(self.emitted, self.emitted + k) for f in self.kept.pop(t)] if self.draw else None
        if self.anonymize is not None and k:                     # first: into the kept copies, in place, before anything is blended or drawn over the faces
            self.pipe.anonymize_heads(images, out['head_box'].view(-1, 4), out['image_of'].view(-1), device=self.dev, **self.frame_options, **self.anonymize)
        if self.heat is not None:
            out.update(self._heat(out, k, images))
        if self.surface_heat is not None:                        # after the image-plane heat map, before arrows, overlay and labels
            out.update(self._surface_heat(out, k, images))
        if self.draw:
            if k:
                gaze = out['fused_smooth' if smoothing else 'fused']
                # copy=True: the frame table of fresh tensors then travels pinned through the staging ring, not as a pageable upload
                rows = (out['head_box'].view(-1, 4), gaze.view(-1, 3), out['image_of'].view(-1))
                if self.overlay is None:
                    drawn, _ = self.pipe.draw_arrows(images, *rows, copy=True, device=self.dev, **self.frame_options)
                else:                                             # (a head's target is a slot or lane by now: the overlay reads target only where kind is "region")
                    drawn = self.pipe.draw_attention(images, *rows, out['target_kind'].view(-1), out['target'].view(-1), out['target_hit'].view(-1, 2),
                                                     out['mutual'].view(-1), regions=self.attention['regions'], region_image=self.attention['region_image'],
                                                     region_period=self.Q, copy=True, device=self.dev, **self.frame_options, **self.overlay)[0]
                images = list(drawn)
                for i in range(k if self.labels is not None else 0):
                    self._draw_labels(out, images, i)             # in place, into the copies just drawn
            out['frames'] = [images[i * Q:(i + 1) * Q] for i in range(k)]
        self.emitted += k
        return out
