"""Video as a stream of frames: each frame goes through the trunk (backbone + FPN) ONCE, however many windows hold it.

The reference's harness cuts a video into windows of ``clip_len`` frames at ``stride`` (tools/test_gaze360_gaze.py:72-86,
harness.plan_windows) and runs the whole model on every window, so at (7, 4) three of every seven frames go through ResNet-50 + FPN
twice.  The trunk of a frame does not depend on its window -- only the decoder mixes frames, through temporal attention inside a
window -- so here a window frame is a ROW of a pyramid store: the trunk writes each new frame into one row of a ring
(``PyramidRing``), and the decoder reads its windows' frames through a device index table (``HipEngine.decode`` ->
mcg_decoder_forward_indexed, the gather happens inside the RoIAlign read).

  * ``WindowPlanner``: pure host bookkeeping.  Fed a growing frame count, it says which windows of the FINAL ``plan_windows(L)`` are
    already certain and below which frame no later window can reach.
  * ``StreamMerger``: the overlap merge of ``harness.merge_video`` applied window by window, handing out frames once they are final.
  * ``DeviceMerger``: the same merge on the device, for any number of streams -- one store of result rows in device memory, one plan
    upload and one mcg_merge_windows launch per decoder call (``merge='device'`` of GazeStream / GazeStreamPool).
  * ``StreamSmoother`` / ``DeviceMerger(smooth=alpha)``: the temporal filter the reference's metric runs over every video
    (tools/calculate_mae_gaze360.py:16-29) as a stream goes -- a frame is handed out one frame late, once its successor is final -- on the
    host, and on the device as one mcg_smooth_gaze launch per pop over all streams (``smooth=`` of GazeStream / GazeStreamPool).
  * ``GazeStream``: push frames as they arrive, get back the per-frame results that became final; ``finish()`` returns the rest.
    It owns a ``PyramidRing`` (the trunk writes in place, no scatter launch) and one ``_StreamState``.
  * ``PyramidStore`` / ``GazeStreamPool``: MANY streams at once (S cameras, or the reference demo's one clip per tracked person,
    MCGaze_demo/demo.ipynb cell 4, each the sliding-window loop of tools/test_gaze360_gaze.py:72-111): one store shared by all streams,
    rows handed out from a free list; per tick ONE trunk call over every stream's new frames, scattered into whichever rows are free
    (``HipEngine.backbone_fpn_rows`` -> mcg_pyramid_scatter_rows), and ONE indexed, ragged decoder call over every stream's newly certain
    windows.  Per stream the same bits as a lone ``GazeStream``, by the same code: everything above the two stores is stated once --
    ``_StreamState`` (a stream's planner, host merger and filter, frames handed out; a pool stream adds its queue and rows),
    ``_decode_windows`` (windows -> decoder calls -> merge; a lone stream is the one-stream case) and ``_stream_setup`` (the arguments both
    take) -- and the result-row layout is harness.pack_rows / split_rows.
"""
import numpy as np
import torch

from . import lib as L
from .harness import (ROW, SMOOTH_ROW, _host, bucket_key, check_smooth, clip_outputs, merge_plan, merge_window, plan_windows, smooth_host, smooth_plan,
                      split_rows)


def _on_device(t):
    """Whether t is a tensor in device memory (an img_hw table that must not be read back)."""
    return isinstance(t, torch.Tensor) and t.is_cuda


class WindowPlanner:
    """Which windows of ``plan_windows(L, clip_len, stride)`` are known while L is still growing.

    A regular window i = (i * stride, i * stride + clip_len) belongs to the final plan iff i * stride + clip_len < L, so it is
    certain once MORE than i * stride + clip_len frames have arrived.  The flush-to-end last window (L - clip_len, L) and the single
    short window of an L <= clip_len video depend on L itself: they are only known at ``finish()``.  No later window starts below
    min(next regular start, frames - clip_len): frames under ``final_upto`` are never touched again."""

    def __init__(self, clip_len=7, stride=4):
        if not (clip_len >= 1 and 1 <= stride <= clip_len):
            # windows that skip frames leave rows merge_video never writes (and its overlap arithmetic assumes stride <= clip_len)
            raise ValueError(f'WindowPlanner needs 1 <= stride <= clip_len (got clip_len={clip_len}, stride={stride})')
        self.T, self.s = clip_len, stride
        self.frames = 0          # frames arrived so far
        self.next = 0            # index of the first regular window not yet handed out
        self.finished = False

    def feed(self, n):
        """n more frames arrived -> the windows (start, stop, overlap) that became certain, in plan order."""
        if self.finished:
            raise L.McgError('WindowPlanner: feed() after finish()')
        self.frames += int(n)
        out = []
        while self.next * self.s + self.T < self.frames:
            a = self.next * self.s
            out.append((a, a + self.T, self.T - self.s))
            self.next += 1
        return out

    def finish(self):
        """The stream ended at L = frames -> the windows of plan_windows(L) not handed out yet (at least one unless L == 0)."""
        if self.finished:
            raise L.McgError('WindowPlanner: finish() called twice')
        self.finished = True
        if self.frames == 0:
            return []
        return plan_windows(self.frames, self.T, self.s)[self.next:]   # the handed-out regular windows are the plan's first `next`

    @property
    def keep_from(self):
        """The lowest frame a window not handed out yet may read (the rows below it may be overwritten)."""
        if self.finished:
            return self.frames
        return max(0, min(self.next * self.s, self.frames - self.T))

    @property
    def final_upto(self):
        """Frames below this index are final: every window that covers them has been handed out."""
        return self.keep_from


class StreamMerger:
    """``harness.merge_video`` one window at a time: windows must be added in plan order; ``pop(upto)`` returns the merged frames
    [emitted, upto) -- which no later window may touch -- and forgets them.  Each step is harness.merge_window, the one merge_video
    runs, so the concatenated output of a stream equals merge_video over the whole plan bit for bit."""

    def __init__(self, person_threshold=0.5):
        self.thr = np.float32(person_threshold)
        self.base = 0            # frame index of row 0 of the buffers (= frames handed out so far)
        self.end = 0             # frames written so far
        self.first = True
        self.det = np.empty((0, 3, 5), np.float32)
        self.fused = np.empty((0, 3), np.float32)
        self.others = np.empty((0, 3, 3), np.float32)

    def _grow(self, stop):
        n = stop - self.base
        if n > self.det.shape[0]:
            cap = max(n, 2 * self.det.shape[0], 16)
            for name, shape in (('det', (3, 5)), ('fused', (3,)), ('others', (3, 3))):
                old = getattr(self, name)
                new = np.empty((cap,) + shape, np.float32)
                new[:old.shape[0]] = old
                setattr(self, name, new)

    def add(self, window, d, f, o):
        """window = (start, stop, overlap) from the plan; d [T,3,5], f [T,3], o [T,3,3] (f32)."""
        start, stop, _ = window
        if start < self.base:
            raise L.McgError(f'StreamMerger: window {window} reaches below frame {self.base}, which was already handed out')
        self._grow(stop)
        merge_window(self.det, self.fused, self.others, self.base, self.first, window, d, f, o, self.thr)
        self.first = False
        self.end = max(self.end, stop)

    def pop(self, upto):
        """-> (det [k,3,5], fused [k,3], others [k,3,3]) for frames [base, upto), copies; upto is clamped to the frames written."""
        k = max(0, min(upto, self.end) - self.base)
        out = (self.det[:k].copy(), self.fused[:k].copy(), self.others[:k].copy())
        if k:
            self.det, self.fused, self.others = self.det[k:], self.fused[k:], self.others[k:]
            self.base += k
        return out


class StreamSmoother:
    """The temporal filter of the reference's metric (tools/calculate_mae_gaze360.py:16-29, smooth_filter) on a stream that is still
    growing, for merge='host': ``push(det, fused, others)`` takes the frames that became final, in order, and returns
    (det, fused, others, fused_smooth [k,3], others_smooth [k,3,3]) of the frames whose successor is known -- so it runs ONE frame behind
    what it is fed; ``finish()`` returns the last frame.  det / fused / others pass through with their bits.  The arithmetic is
    harness.smooth_host's -- mcg_smooth_gaze's -- and over a whole stream the concatenated output equals the filter over the whole
    sequence bit for bit however the frames were chunked.  It keeps two frames: the last one handed out and the one held back."""

    def __init__(self, alpha=0.6):
        self.alpha = check_smooth('StreamSmoother', alpha)
        self.prev = None         # gaze [4,3] (fused | others) of the last frame handed out
        self.held = None         # (det [1,3,5], fused [1,3], others [1,3,3]) of the newest frame: its successor is not known yet
        self.finished = False

    def push(self, det, fused, others, ended=False):
        if self.finished:
            raise L.McgError('StreamSmoother: push() after finish()')
        self.finished = bool(ended)
        parts = [np.asarray(x, dtype=np.float32) for x in (det, fused, others)]
        if self.held is not None:
            parts = [np.concatenate([h, x]) for h, x in zip(self.held, parts)]
        det, fused, others = parts
        n = det.shape[0]
        k = n if ended else max(0, n - 1)                  # the newest frame waits for its successor
        g = np.concatenate([fused[:, None], others], axis=1)                       # [n,4,3]
        lead = self.prev is not None
        sm = smooth_host(np.concatenate([self.prev[None], g]) if lead else g, self.alpha, lead=lead, trail=k < n)
        if k:
            self.prev = g[k - 1]
        self.held = None if k == n else tuple(x[k:].copy() for x in parts)
        return det[:k].copy(), fused[:k].copy(), others[:k].copy(), np.ascontiguousarray(sm[:, 0]), np.ascontiguousarray(sm[:, 1:])

    def finish(self):
        """The stream ended -> the frame held back (no frame of an empty stream)."""
        z = np.empty
        return self.push(z((0, 3, 5), np.float32), z((0, 3), np.float32), z((0, 3, 3), np.float32), ended=True)


class _Written:
    """The frames of DeviceMerger's streams that held state before the current call: per stream the range [base, end)."""

    def __init__(self, spans):
        self.spans = spans

    def __contains__(self, key_frame):
        a, b = self.spans.get(key_frame[0], (0, 0))
        return a <= key_frame[1] < b


class DeviceMerger:
    """The device counterpart of StreamMerger, for any number of streams: the merged frames live in ONE store tensor [rows, 27] on the
    engine's device (a row = det 3x5 | fused 3 | others 3x3) and never visit the host.

    ``add_call(windows, out, scale)`` folds the outputs of one decoder call -- however many windows of however many streams -- into the
    store: one plan table (harness.merge_plan, uploaded pinned and non-blocking) and one mcg_merge_windows launch on the current stream.
    ``pop([(key, upto)])`` hands out, per stream, the frames [handed out so far, upto) -- which no later window may touch -- with one
    index_select over all of them, and gives their rows back for reuse.  Nothing here waits for the device unless ``host=True`` asks for
    the popped frames as numpy arrays (one copy for all streams).  Per stream the windows must come in plan order; the concatenated
    output of a stream equals harness.merge_video over its plan bit for bit (tests/test_gpu_device_merge.py).
    Rows come from a free list; a store that runs out of rows is replaced by one twice as large (a device copy, no sync).

    smooth=alpha: ``pop`` also returns the frames' gaze after the temporal filter of the reference's metric
    (tools/calculate_mae_gaze360.py:16-29): (det, fused, others, fused_smooth [k,3], others_smooth [k,3,3]) per item, from ONE
    mcg_smooth_gaze launch over all items (a host-built table, harness.smooth_plan) beside the index_select.  A frame needs its
    successor, so it is handed out once the successor is final or the stream has ended (``ended``: the keys of such streams): ``pop``
    then runs one frame behind what it returns without smoothing.  The row of the last frame handed out stays allocated, as the next
    frame's predecessor, until that frame has been handed out, the stream has ended, or ``forget``.  det / fused / others keep their bits."""

    ROW, SMOOTH_ROW = ROW, SMOOTH_ROW

    class _Stream:
        def __init__(self):
            self.base, self.end, self.rows = 0, 0, {}      # frames handed out / written so far; frame -> store row of the live frames

    def __init__(self, device, person_threshold=0.5, rows=256, smooth=None):
        self.smooth = check_smooth('DeviceMerger', smooth)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise L.McgError(f'DeviceMerger: merging on the device needs a HIP device (got {self.device}); there is no CPU fallback path')
        from .engine import _ptr, _stream, _upload_table
        self._ptr, self._cur, self._upload = _ptr, _stream, _upload_table
        self.lib = L.load()
        self.thr = float(np.float32(person_threshold))
        self.store = torch.empty(max(int(rows), 1), self.ROW, dtype=torch.float32, device=self.device)
        self._free = list(range(self.store.shape[0] - 1, -1, -1))
        self.streams = {}

    def _alloc(self):
        if not self._free:
            old = self.store
            self.store = torch.empty(2 * old.shape[0], self.ROW, dtype=torch.float32, device=self.device)
            self.store[:old.shape[0]].copy_(old)
            self._free = list(range(self.store.shape[0] - 1, old.shape[0] - 1, -1))
        return self._free.pop()

    def add_call(self, windows, out, scale=None):
        """windows: [(key, (start, stop, overlap), first output row)] of ONE decoder call whose outputs are ``out`` (the engine's dict:
        gaze [4,n,3], boxes [n,3,4], scores [n,3], f32 on the device); scale: None, 4 values for every frame alike, or [n,4] / [n,1,4] per
        frame (a device tensor): rescale=True's division, done in the kernel."""
        if not windows:
            return
        n = out['scores'].shape[0]
        spans = {}
        for key, (start, stop, _), _ in windows:
            st = self.streams.setdefault(key, self._Stream())
            if key not in spans:
                spans[key] = (st.base, st.end)
            if start < st.base:
                raise L.McgError(f'DeviceMerger: window ({start}, {stop}) reaches below frame {st.base}, which was already handed out')
        taken = []
        try:
            for key, (start, stop, _), _ in windows:
                st = self.streams[key]
                for f in range(start, stop):
                    if f not in st.rows:
                        st.rows[f] = self._alloc()
                        taken.append((st, f))
            table, max_src = merge_plan(windows, lambda key, f: self.streams[key].rows[f], _Written(spans), n, self.store.shape[0])
        except ValueError:
            for st, f in taken:                             # a rejected call leaves the merger as it was
                self._free.append(st.rows.pop(f))
            raise
        per_frame = 0
        if scale is not None:
            scale = scale.to(self.device, torch.float32).contiguous()
            if scale.numel() not in (4, 4 * n):
                raise ValueError(f'DeviceMerger: scale must hold 4 or {n} x 4 values (got {tuple(scale.shape)})')
            per_frame = int(scale.numel() != 4)
        g, b, s = (out[k].to(torch.float32).contiguous() for k in ('gaze', 'boxes', 'scores'))
        plan = self._upload(table, self.device)
        L.check(self.lib.mcg_merge_windows(self._cur(self.device), self._ptr(g), self._ptr(b), self._ptr(s), n, self._ptr(scale), per_frame,
                                           self._ptr(plan), table.shape[0], max_src, self._ptr(self.store), self.store.shape[0], self.thr),
                'mcg_merge_windows')
        for key, (_, stop, _), _ in windows:
            st = self.streams[key]
            st.end = max(st.end, stop)

    def pop_rows(self, items, ended=()):
        """items: [(key, upto)] -> (rows [K,27], smoothed [K,12] = fused 3 | others 3x3 or None without smooth=, [k per item]): the frames
        [handed out, min(upto, written)) of every item's stream -- but the last one, if the merger smooths and the stream is not in ``ended`` --
        item after item, gathered into ONE fresh device tensor by one index_select and filtered by one mcg_smooth_gaze launch.  Their store
        rows are free for reuse, except (smoothing) each stream's last, which stays allocated unless the stream has ended."""
        smoothing = self.smooth is not None
        rows, counts, plans, freed = [], [], [], []
        for key, upto in items:
            st = self.streams.get(key)
            over = key in ended
            k = 0 if st is None else max(0, min(int(upto), st.end) - st.base - int(smoothing and not over))
            if k:
                frames = range(st.base, st.base + k)
                if smoothing:
                    plans.append(smooth_plan(frames, st.rows.__getitem__, 0, st.end - 1 if over else None, self.store.shape[0]))
                rows += [st.rows[f] for f in frames] if smoothing else [st.rows.pop(f) for f in frames]   # plain: released as handed out
                st.base += k
            if smoothing and st is not None:               # the rows below the last frame handed out are no one's neighbour any more
                keep = st.base - (0 if over and st.base == st.end else 1)
                freed += [st.rows.pop(f) for f in sorted(f for f in st.rows if f < keep)]
            counts.append(k)
        new = lambda n, w: torch.empty(n, w, dtype=torch.float32, device=self.device)
        packed = self.store.index_select(0, self._upload(np.asarray(rows, dtype=np.int64), self.device)) if rows else new(0, ROW)
        smoothed = new(len(rows), SMOOTH_ROW) if smoothing else None
        if rows and smoothing:
            plan = self._upload(np.concatenate(plans), self.device)
            L.check(self.lib.mcg_smooth_gaze(self._cur(self.device), self._ptr(self.store), self.store.shape[0], self._ptr(plan), len(rows),
                                             self.smooth, self._ptr(smoothed)), 'mcg_smooth_gaze')
        self._free.extend(reversed(freed if smoothing else rows))   # later launches on this stream run after the gather and the filter
        return packed, smoothed, counts

    def pop(self, items, host=False, ended=()):
        """pop_rows as one (det [k,3,5], fused [k,3], others [k,3,3]) per item: views of the gathered tensor on the device, or (host=True)
        numpy arrays after ONE copy to the host for all items together.  A smoothing merger (``ended``: the keys whose stream is over)
        adds fused_smooth [k,3] and others_smooth [k,3,3] to every item."""
        packed, smoothed, counts = self.pop_rows(items, ended)
        if host:
            packed, smoothed = (packed if smoothed is None else torch.cat([packed, smoothed], dim=1)).cpu().numpy(), None
        parts = split_rows(packed)                         # split once, then cut per item: views either way
        if smoothed is not None:
            parts += (smoothed[:, :3], smoothed[:, 3:].reshape(smoothed.shape[0], 3, 3))
        res, at = [], 0
        for k in counts:
            res.append(tuple(p[at:at + k] for p in parts))
            at += k
        if host:
            res = [tuple(np.ascontiguousarray(x) for x in r) for r in res]
        return res

    def forget(self, key):
        """The stream ended: its remaining rows (none after a pop up to its end) go back to the free list."""
        st = self.streams.pop(key, None)
        if st is not None:
            self._free.extend(st.rows.values())


def _stream_setup(who, engine_or_model, clip_len, stride, scale_factor, person_threshold, merge, results, smooth, merger_rows):
    """The arguments GazeStream and GazeStreamPool share, checked -> (engine, smooth, scale [1,1,4] on its device or None, the DeviceMerger
    of ``merger_rows`` rows or None with merge='host')."""
    e = engine_or_model
    if not hasattr(e, 'decode') and hasattr(e, 'engine'):
        e = e.engine()
    if merge not in ('host', 'device') or results not in ('host', 'device'):
        raise ValueError(f"{who}: merge and results are 'host' or 'device' (got merge={merge!r}, results={results!r})")
    if results == 'device' and merge != 'device':
        raise ValueError(f"{who}: results='device' needs merge='device' (the host merge has its results on the host)")
    if merge == 'device' and torch.device(e.device).type != 'cuda':
        raise L.McgError(f"{who}: merge='device' needs an engine on a HIP device (got {e.device}); there is no CPU fallback path")
    smooth = check_smooth(who, smooth)
    WindowPlanner(clip_len, stride)                         # rejects a bad (clip_len, stride) here, not at the first frame
    scale = None if scale_factor is None else torch.as_tensor(scale_factor, dtype=torch.float32, device=e.device).reshape(1, 1, 4)
    dmerger = DeviceMerger(e.device, person_threshold, rows=merger_rows, smooth=smooth) if merge == 'device' else None
    return e, smooth, scale, dmerger


class _StreamState:
    """One stream above its pyramid rows, for a lone GazeStream and a stream of a GazeStreamPool alike: its plan, its host merge and host
    filter (idle with merge='device': the DeviceMerger holds the stream's frames under this object as key) and the frames handed out."""

    def __init__(self, clip_len, stride, person_threshold, smooth=None):
        self.planner = WindowPlanner(clip_len, stride)
        self.merger = StreamMerger(person_threshold)
        self.smoother = None if smooth is None else StreamSmoother(smooth)     # merge='host' only: the device merger filters its own rows
        self.emitted = 0

    def upto(self):
        """Frames below this index can be handed out: the final ones, which is all of them once the stream has ended."""
        return self.planner.final_upto

    def add_host(self, window, det, fused, others):
        self.merger.add(window, det, fused, others)

    def emit(self, popped=None):
        """popped: this stream's tuple of DeviceMerger.pop, or None: the host merger's frames below upto(), through the host filter
        -> dict(first, det, fused, others[, fused_smooth, others_smooth])."""
        if popped is None:
            popped = self.merger.pop(self.upto())
            if self.smoother is not None:
                popped = self.smoother.push(*popped, ended=self.planner.finished)
        res = dict(first=self.emitted, **dict(zip(('det', 'fused', 'others', 'fused_smooth', 'others_smooth'), popped)))
        self.emitted += popped[0].shape[0]
        return res


def _decode_windows(engine, levels, hw, H, W, items, row_of, scale, max_windows, dmerger):
    """items: [(state, window)], frame f of a state in row row_of(state, f) of ``levels`` -> one decoder call per longest-clip class
    (harness.bucket_key) and per max_windows windows, merged per stream: ONE dmerger.add_call keyed by the state, or (dmerger None) one
    blocking copy and add_host per window.  Windows of one length: clip_length is that length; of different lengths: the ragged call.
    A lone GazeStream brings what ONE feed() or finish() of its planner handed out -- regular windows and the flush-to-end last one,
    all clip_len long, or the single short window of a stream of at most clip_len frames -- so: one class, the scalar clip_length."""
    classes = {}
    for it in items:
        classes.setdefault(bucket_key(H, W, it[1][1] - it[1][0], True), []).append(it)
    for key in sorted(classes):
        group = classes[key]
        for i in range(0, len(group), max_windows or len(group)):
            part = group[i:i + (max_windows or len(group))]
            lengths = [w[1] - w[0] for _, w in part]
            starts = np.concatenate([[0], np.cumsum(lengths)]).tolist()
            table = [row_of(st, f) for st, w in part for f in range(w[0], w[1])]
            out = engine.decode(levels, table, lengths[0] if len(set(lengths)) == 1 else lengths, img_hw=hw)
            if dmerger is not None:
                dmerger.add_call([(st, w, at) for (st, w), at in zip(part, starts)], out, scale)
                continue
            det, fused, others = (t.cpu().numpy() for t in clip_outputs(out, scale))
            for (st, w), a, b in zip(part, starts, starts[1:]):    # a stream's windows are in plan order within its class
                st.add_host(w, det[a:b], fused[a:b], others[a:b])


class PyramidRing:
    """The per-level pyramid store of a stream, used as a ring of ``capacity`` rows: frame i lives in row i % capacity.

    ``append`` runs the trunk on the new frames only (two trunk calls where the rows wrap) and returns their rows.  Rows of frames at
    or above ``keep_from`` (set by the owner through ``release``) are still needed by a pending window: an append that would overwrite
    one raises instead.  ``hw`` holds img_shape per row once any frame came with one (the decoder reads it by row)."""

    def __init__(self, engine, capacity, H, W):
        if capacity < 1:
            raise L.McgError(f'PyramidRing: capacity must be positive (got {capacity})')
        self.e, self.capacity, self.H, self.W = engine, int(capacity), H, W
        self.levels = [torch.empty(self.capacity, (H // 4) >> i, (W // 4) >> i, 256, dtype=engine.dtype, device=engine.device) for i in range(4)]
        self.hw = None
        self.count = 0           # frames appended so far
        self.keep_from = 0

    def free(self):
        """Frames that can be appended now without overwriting a row still needed."""
        return self.capacity - (self.count - self.keep_from)

    def release(self, keep_from):
        """Rows of frames below keep_from may be overwritten from now on."""
        self.keep_from = max(self.keep_from, min(int(keep_from), self.count))

    def row(self, frame):
        return frame % self.capacity

    def append(self, frames, img_hw=None):
        """frames [n,3,H,W] f32 on the engine's device -> list of the n rows they were written to."""
        n = frames.shape[0]
        if n > self.free():
            raise L.McgError(f'PyramidRing: appending {n} frames would overwrite rows still needed (capacity {self.capacity}, '
                             f'frames {self.keep_from}..{self.count - 1} pending)')
        if tuple(frames.shape[1:]) != (3, self.H, self.W):
            raise L.McgError(f'PyramidRing: frames must be [n,3,{self.H},{self.W}] (got {tuple(frames.shape)})')
        frames = frames.to(self.e.device, torch.float32).contiguous()
        if img_hw is not None and self.hw is None:
            self.hw = torch.empty(self.capacity, 2, dtype=torch.int32, device=self.e.device)
            self.hw[:, 0], self.hw[:, 1] = self.H, self.W       # = what the decoder assumes without a table
        r0 = self.count % self.capacity
        first = min(n, self.capacity - r0)
        for a, b, row in ((0, first, r0), (first, n, 0)):
            if b > a:
                self.e.backbone_fpn(frames[a:b], out=self.levels, row=row)
                if self.hw is not None:
                    hw = (torch.tensor([[self.H, self.W]] * (b - a), dtype=torch.int32) if img_hw is None
                          else torch.as_tensor(np.asarray(_host(img_hw), dtype=np.int32).reshape(n, 2)[a:b]))
                    self.hw[row:row + b - a].copy_(hw)
        rows = [(self.count + i) % self.capacity for i in range(n)]
        self.count += n
        return rows


class GazeStream:
    """Gaze on a live feed: ``push`` frames as they arrive, get back the per-frame results that became final.

    Every frame runs through the trunk once, into a ``PyramidRing``; then ONE indexed decoder call (``HipEngine.decode``) runs every
    window that became certain (``WindowPlanner``), and the windows are merged in plan order (``StreamMerger``).

    Contract: over a whole stream of L frames the concatenated outputs of ``push`` and ``finish`` equal, bit for bit,
    ``harness.merge_video(plan_windows(L), [one engine.forward per window])`` -- the contract ``harness.run_videos`` has.  It rests on
    the trunk giving a frame the same bits in any batch (tests/test_gpu_window_reuse.py) and on the decoder giving a window the same
    bits whichever windows share its call.  The fp16 engine (precision 'f16') keeps the latter only below 256 tokens per call
    (ADVICE.md): give it ``max_decode_windows`` <= 12 at clip_len 7.

    engine_or_model: a ``HipEngine`` or a model from ``init_detector`` (its ``engine()``).  capacity: pyramid rows of the ring
    (default clip_len + 64); a push larger than the free rows is run in steps.  scale_factor: 4 floats the boxes are divided by
    (rescale=True, multiclue_gaze_roi_head.py:360-363).
    Results: dicts of numpy arrays det [k,3,5] (boxes xyxy + score), fused [k,3], others [k,3,3] -- merge_video's layout -- plus
    ``first``: the index of the first frame in the dict.
    merge='device': the windows are merged on the device (``DeviceMerger``: one mcg_merge_windows launch per decoder call) instead of on
    the host after a blocking copy per decoder call -- the same bits.  results='host' then makes ONE copy to the host per push;
    results='device' (needs merge='device') returns the same dicts with f32 tensors on the engine's device: their values are valid on
    the engine's current stream, and push / finish never wait for the device.
    smooth: None, or the alpha in (0, 1] of the temporal filter the reference's published accuracy is measured with
    (tools/calculate_mae_gaze360.py:16-29; 0.6 there).  The dicts gain ``fused_smooth`` [k,3] and ``others_smooth`` [k,3,3]: every gaze
    vector mixed with the same vector of the frames before and after it and re-normalised (include/mcgaze_hip.h, mcg_smooth_gaze, states
    the arithmetic; ``StreamSmoother`` on the host, one mcg_smooth_gaze launch per push with merge='device' -- the same bits).  A frame
    needs its successor, so every frame is returned ONE frame later than without the option and ``finish`` returns the last; ``first``
    and the lengths describe the frames a dict holds.  det / fused / others are the bits they are without it; a one-frame stream's
    smoothed gaze is its gaze, not normalised (the reference's rule).  results='device' keeps its guarantee."""

    def __init__(self, engine_or_model, H, W, clip_len=7, stride=4, capacity=None, scale_factor=None, person_threshold=0.5,
                 max_decode_windows=None, merge='host', results='host', smooth=None):
        self.e, smooth, self.scale, self.dmerger = _stream_setup('GazeStream', engine_or_model, clip_len, stride, scale_factor, person_threshold,
                                                                 merge, results, smooth, 4 * clip_len)
        self.results = results
        self.T, self.s = clip_len, stride
        self.state = _StreamState(clip_len, stride, person_threshold, smooth if merge == 'host' else None)
        capacity = clip_len + 64 if capacity is None else int(capacity)
        if capacity <= clip_len:
            raise L.McgError(f'GazeStream: capacity must exceed clip_len ({capacity} <= {clip_len})')
        self.ring = PyramidRing(self.e, capacity, H, W)
        self.max_windows = max_decode_windows

    def _decode(self, windows):
        _decode_windows(self.e, self.ring.levels, self.ring.hw, self.ring.H, self.ring.W, [(self.state, w) for w in windows],
                        lambda st, f: self.ring.row(f), self.scale, self.max_windows, self.dmerger)

    def _emit(self):
        st = self.state
        if self.dmerger is None:
            return st.emit()
        return st.emit(self.dmerger.pop([(st, st.upto())], host=self.results == 'host', ended=(st,) if st.planner.finished else ())[0])

    def push(self, frames, img_hw=None):
        """frames [n,3,H,W] f32 (preprocessed like engine.forward's input); img_hw: [n,2] img_shape per frame or None.
        -> the frames that became final (possibly none)."""
        n, i, planner = frames.shape[0], 0, self.state.planner
        while i < n:
            m = min(n - i, self.ring.free())
            if m <= 0:
                raise L.McgError('GazeStream: the pyramid ring has no free row (capacity too small)')
            self.ring.append(frames[i:i + m], None if img_hw is None else np.asarray(_host(img_hw)).reshape(n, 2)[i:i + m])
            self._decode(planner.feed(m))
            self.ring.release(planner.keep_from)
            i += m
        return self._emit()

    def finish(self):
        """End of the stream: the windows that depend on its length, and every frame not returned yet."""
        self._decode(self.state.planner.finish())
        return self._emit()


class PyramidStore:
    """A pyramid store SHARED by many streams: ``rows`` frames per level, handed out from a free list in no particular order (streams of
    different pace free their rows out of order, so a ring of one head would be pinned by its slowest stream).

    ``alloc(n)`` -> n free rows (McgError when fewer are free: a live row is never handed out again before ``free`` returned it);
    ``write(frames, rows)`` runs the trunk on the frames and writes frame i to rows[i] (``HipEngine.backbone_fpn_rows``).  ``hw`` holds
    img_shape per row once any frame came with one (the decoder reads it by row), like ``PyramidRing.hw``."""

    def __init__(self, engine, rows, H, W):
        if rows < 1:
            raise L.McgError(f'PyramidStore: rows must be positive (got {rows})')
        self.e, self.rows, self.H, self.W = engine, int(rows), H, W
        self.levels = [torch.empty(self.rows, (H // 4) >> i, (W // 4) >> i, 256, dtype=engine.dtype, device=engine.device) for i in range(4)]
        self.hw = None
        self._free = list(range(self.rows - 1, -1, -1))     # a stack: the lowest rows go out first
        self._live = set()

    def free_rows(self):
        return len(self._free)

    def alloc(self, n):
        if n > len(self._free):
            raise L.McgError(f'PyramidStore: {n} rows asked for, {len(self._free)} of {self.rows} are free')
        rows = [self._free.pop() for _ in range(n)]
        self._live.update(rows)
        return rows

    def free(self, rows):
        for r in rows:
            if r not in self._live:
                raise L.McgError(f'PyramidStore: row {r} is freed but was not handed out')
            self._live.remove(r)
            self._free.append(r)

    def write(self, frames, rows, img_hw=None):
        """frames [n,3,H,W] f32 -> rows[i] of every level holds frame i's pyramid; img_hw [n,2] (host, or a device tensor, which stays on the
        device) or None (every frame fills H x W)."""
        n = frames.shape[0]
        if tuple(frames.shape[1:]) != (3, self.H, self.W):
            raise L.McgError(f'PyramidStore: frames must be [n,3,{self.H},{self.W}] (got {tuple(frames.shape)})')
        rows = [int(r) for r in rows]
        if len(rows) != n or any(r not in self._live for r in rows):
            raise L.McgError(f'PyramidStore: write() takes one row from alloc() per frame (got {len(rows)} rows for {n} frames)')
        self.e.backbone_fpn_rows(frames.to(self.e.device, torch.float32).contiguous(), self.levels, rows)
        if img_hw is not None and self.hw is None:
            self.hw = torch.empty(self.rows, 2, dtype=torch.int32, device=self.e.device)
            self.hw[:, 0], self.hw[:, 1] = self.H, self.W       # = what the decoder assumes without a table
        if self.hw is not None and n and _on_device(img_hw):
            # a table that is on the device stays there: one indexed copy, the row indices uploaded pinned -- nothing waits (live.LiveGaze)
            from .engine import _upload_table
            self.hw.index_copy_(0, _upload_table(np.asarray(rows, dtype=np.int64), self.e.device), img_hw.to(self.e.device, torch.int32).reshape(n, 2))
        elif self.hw is not None and n:
            hw = (np.array([[self.H, self.W]] * n, dtype=np.int32) if img_hw is None else np.asarray(_host(img_hw), dtype=np.int32).reshape(n, 2))
            self.hw[torch.as_tensor(rows, dtype=torch.int64).to(self.e.device)] = torch.from_numpy(hw).to(self.e.device)
        return rows


class _PoolStream(_StreamState):
    """One stream of a GazeStreamPool: a _StreamState plus where its live frames lie in the store and the frames pushed but not run yet."""

    def __init__(self, clip_len, stride, person_threshold, smooth=None):
        super().__init__(clip_len, stride, person_threshold, smooth)
        self.row_of = {}         # frame index -> store row, for the frames a later window may still read
        self.queue = []          # (frames [n,3,H,W], img_hw [n,2] numpy or None) in push order
        self.queued = 0
        self.closed = False
        self.admitted = False    # holds a reservation of clip_len + stride rows
        self.released = 0        # frames below this index gave their rows back

    def take(self, m):
        """The first m queued frames -> ([frames...], [img_hw or None per part])."""
        parts, hws = [], []
        while m:
            x, hw = self.queue[0]
            k = min(m, x.shape[0])
            parts.append(x[:k])
            hws.append(None if hw is None else hw[:k])
            if k == x.shape[0]:
                self.queue.pop(0)
            else:
                self.queue[0] = (x[k:], None if hw is None else hw[k:])
            m -= k
            self.queued -= k
        return parts, hws


class GazeStreamPool:
    """Gaze on MANY live feeds at once -- S cameras, or S tracked people (one clip per person, like the reference demo): ``push`` queues a
    stream's new frames, ``step`` runs every stream's queued frames through ONE trunk call into a shared ``PyramidStore`` and every
    stream's newly certain windows through ONE indexed, ragged decoder call (per longest-clip class, ``harness.bucket_key``), where S
    ``GazeStream`` objects make S calls of each.

        pool = GazeStreamPool(engine, H, W)
        sid = pool.open()
        pool.push(sid, frames)            # queues only: no GPU work
        for sid, r in pool.step().items():  # r = dict(first, det, fused, others): the frames of stream sid that became final
            ...
        pool.close(sid)                   # its last windows run in the next step(); then the stream is gone and its rows are free

    Contract: for every stream the concatenation of what ``step`` returned for it equals, bit for bit, a lone ``GazeStream`` fed the same
    frames in the same order -- so also ``harness.merge_video(plan_windows(L), [one engine.forward per window])`` -- however the other
    streams' pushes, lengths and closes interleave with it.  It rests on the trunk giving a frame the same bits in any batch and on the
    decoder giving a window the same bits whichever windows share its call.  The fp16 engine (precision 'f16') keeps the latter only below
    256 tokens per call: give it ``max_decode_windows`` <= 12 at clip_len 7.

    rows: rows of the shared store (default 64 * (clip_len + stride) + max_trunk_frames).  A stream that runs holds a reservation of
    clip_len + stride rows, so it can always reach its next window; a ``step`` that finds fewer rows free than the queued frames need runs
    what fits -- a part of a stream's queue, or none of a stream that cannot get its reservation yet -- and leaves the rest queued for the
    next ``step`` (``pending()`` says whether anything is left).  It raises McgError only where the store cannot hold one stream's
    reservation.  max_trunk_frames: the trunk call is split only above this many frames; max_decode_windows: windows per decoder call.
    Driven from one thread.  Results: ``GazeStream.push``'s dicts, keyed by stream id; a closed stream gets an entry in the step that ends
    it even when no frame was left.
    merge / results: as for ``GazeStream`` -- merge='device' folds every decoder call into ONE ``DeviceMerger`` shared by all streams (one
    plan upload and one mcg_merge_windows launch per decoder call, where the host merge makes a blocking copy per call and one numpy
    merge per window); results='host' then costs one copy per ``step`` for all streams together, results='device' none: ``step``
    returns device tensors that are valid on the engine's current stream and never waits for the device.
    smooth: as for ``GazeStream`` -- every dict gains ``fused_smooth`` and ``others_smooth``, every stream's frames come one frame late and
    the step that ends a stream returns its last; with merge='device' ONE mcg_smooth_gaze launch per ``step`` covers all streams."""

    def __init__(self, engine_or_model, H, W, clip_len=7, stride=4, rows=None, scale_factor=None, person_threshold=0.5, max_decode_windows=None,
                 max_trunk_frames=448, merge='host', results='host', smooth=None):
        self.e, self.smooth, self.scale, self.dmerger = _stream_setup('GazeStreamPool', engine_or_model, clip_len, stride, scale_factor,
                                                                      person_threshold, merge, results, smooth, 16 * (clip_len + stride))
        self.results = results
        self.H, self.W = H, W
        self.T, self.s, self.thr = clip_len, stride, person_threshold
        if max_trunk_frames < 1 or (max_decode_windows is not None and max_decode_windows < 1):
            raise L.McgError(f'GazeStreamPool: max_trunk_frames and max_decode_windows must be positive (got {max_trunk_frames}, {max_decode_windows})')
        self.max_trunk, self.max_windows = int(max_trunk_frames), max_decode_windows
        self.store = PyramidStore(self.e, 64 * (clip_len + stride) + self.max_trunk if rows is None else int(rows), H, W)
        self.streams = {}        # sid -> _PoolStream, in open order
        self.next_sid = 0

    def open(self):
        sid = self.next_sid
        self.next_sid += 1
        self.streams[sid] = _PoolStream(self.T, self.s, self.thr, None if self.dmerger is not None else self.smooth)
        return sid

    def _stream(self, sid, what):
        st = self.streams.get(sid)
        if st is None:
            raise L.McgError(f'GazeStreamPool.{what}: no open stream {sid!r}')
        if st.closed:
            raise L.McgError(f'GazeStreamPool.{what}: stream {sid!r} is closed')
        return st

    def push(self, sid, frames, img_hw=None):
        """Queue frames [n,3,H,W] f32 (host or device, preprocessed like engine.forward's input) of stream sid; img_hw: [n,2] or None.  An
        img_hw that is a device tensor (head_crops' as it comes) is not read back: it reaches the store's table by an indexed copy."""
        st = self._stream(sid, 'push')
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (3, self.H, self.W):
            raise L.McgError(f'GazeStreamPool.push: frames must be [n,3,{self.H},{self.W}] (got {tuple(frames.shape)})')
        n = frames.shape[0]
        if n:
            if _on_device(img_hw):                         # kept where it is, and not read back: step() copies it into the store's table
                hw = img_hw.to(torch.int32).reshape(n, 2)
            else:
                hw = None if img_hw is None else np.array(_host(img_hw), dtype=np.int32).reshape(n, 2)
            st.queue.append((frames, hw))
            st.queued += n

    def close(self, sid):
        self._stream(sid, 'close').closed = True

    def pending(self):
        """Whether a step() has work left: queued frames, or a closed stream whose last windows have not run."""
        return any(st.queued or st.closed for st in self.streams.values())

    def _plan_step(self):
        """-> {sid: frames of its queue that run now}.  Every admitted stream keeps clip_len + stride rows reserved (held + still free), so it
        can always run up to its next window, whose decode releases rows again; rows beyond the reservations go to whoever asks first."""
        R = self.T + self.s
        spare = self.store.free_rows() - sum(max(0, R - len(st.row_of)) for st in self.streams.values() if st.admitted)
        take = {}
        for sid, st in self.streams.items():
            if not st.queued:
                continue
            if not st.admitted:
                if spare < R:
                    continue
                st.admitted, spare = True, spare - R
            own = max(0, R - len(st.row_of))
            m = min(st.queued, own + max(0, spare))
            spare -= max(0, m - own)
            if m:
                take[sid] = m
        if not take and not any(st.admitted for st in self.streams.values()) and any(st.queued for st in self.streams.values()):
            raise L.McgError(f'GazeStreamPool: a store of {self.store.rows} rows cannot hold one stream (clip_len + stride = {R} live frames)')
        return take

    def step(self):
        """Run what is queued -> {sid: dict(first, det, fused, others)} for every stream that had frames become final."""
        take = self._plan_step()
        # 1. one trunk call over every stream's frames, into whichever rows are free
        parts, hws, rows = [], [], []
        for sid, m in take.items():
            st = self.streams[sid]
            p, h = st.take(m)
            r = self.store.alloc(m)
            for k, row in enumerate(r):
                st.row_of[st.planner.frames + k] = row
            parts, hws, rows = parts + p, hws + h, rows + r
        if rows:
            x = [p.to(self.e.device, torch.float32) for p in parts]
            x = x[0] if len(x) == 1 else torch.cat(x)
            hw = None
            if self.store.hw is not None or any(h is not None for h in hws):
                full = lambda p: np.array([[self.H, self.W]] * p.shape[0], dtype=np.int32)
                if any(_on_device(h) for h in hws):           # device tables stay on the device; host ones join them (pinned, non-blocking)
                    from .engine import _upload_table
                    hw = [h.to(self.e.device) if _on_device(h) else _upload_table(full(p) if h is None else h, self.e.device) for p, h in zip(parts, hws)]
                    hw = hw[0] if len(hw) == 1 else torch.cat(hw)
                else:
                    hw = np.concatenate([full(p) if h is None else h for p, h in zip(parts, hws)])
            for i in range(0, len(rows), self.max_trunk):
                self.store.write(x[i:i + self.max_trunk], rows[i:i + self.max_trunk], None if hw is None else hw[i:i + self.max_trunk])
        # 2. one decoder call over every window that became certain
        items, touched = [], []
        for sid, st in self.streams.items():
            wins = st.planner.feed(take[sid]) if sid in take else []
            if st.closed and not st.queued:
                wins = wins + st.planner.finish()
            items += [(st, w) for w in wins]
            if sid in take or st.planner.finished:
                touched.append((sid, st))
        _decode_windows(self.e, self.store.levels, self.store.hw, self.H, self.W, items, lambda st, f: st.row_of[f], self.scale,
                        self.max_windows, self.dmerger)
        # 3. + 4. per stream: hand out the frames that are final, give back the rows no later window reads
        results = {}
        popped = [None] * len(touched)
        if self.dmerger is not None:                       # one gather (and, results='host', one copy) for all streams together
            popped = self.dmerger.pop([(st, st.upto()) for _, st in touched], host=self.results == 'host',
                                      ended=[st for _, st in touched if st.planner.finished])
        for (sid, st), out in zip(touched, popped):
            res = st.emit(out)
            if res['det'].shape[0] or st.planner.finished:
                results[sid] = res
            keep = st.planner.keep_from
            self.store.free([st.row_of.pop(f) for f in range(st.released, keep)])
            st.released = max(st.released, keep)
            if st.planner.finished:                        # the stream is gone; its frames left the device merger in the pop above
                if self.dmerger is not None:
                    self.dmerger.forget(st)
                del self.streams[sid]
        return results
