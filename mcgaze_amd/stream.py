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
  * ``GazeStream``: push frames as they arrive, get back the per-frame results that became final; ``finish()`` returns the rest.
"""
import numpy as np
import torch

from . import lib as L
from .harness import _host, clip_outputs, merge_window, plan_windows


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
    ``first``: the index of the first frame in the dict."""

    def __init__(self, engine_or_model, H, W, clip_len=7, stride=4, capacity=None, scale_factor=None, person_threshold=0.5,
                 max_decode_windows=None):
        e = engine_or_model
        if not hasattr(e, 'decode') and hasattr(e, 'engine'):
            e = e.engine()
        self.e = e
        self.T, self.s = clip_len, stride
        self.planner = WindowPlanner(clip_len, stride)
        self.merger = StreamMerger(person_threshold)
        capacity = clip_len + 64 if capacity is None else int(capacity)
        if capacity <= clip_len:
            raise L.McgError(f'GazeStream: capacity must exceed clip_len ({capacity} <= {clip_len})')
        self.ring = PyramidRing(e, capacity, H, W)
        self.scale = None if scale_factor is None else torch.as_tensor(scale_factor, dtype=torch.float32, device=e.device).reshape(1, 1, 4)
        self.max_windows = max_decode_windows
        self.emitted = 0

    def _decode(self, windows):
        for i in range(0, len(windows), self.max_windows or max(1, len(windows))):
            part = windows[i:i + (self.max_windows or len(windows))]
            T = part[0][1] - part[0][0]
            table = [self.ring.row(f) for a, b, _ in part for f in range(a, b)]
            out = self.e.decode(self.ring.levels, table, T, img_hw=self.ring.hw)
            det, fused, others = (t.cpu().numpy() for t in clip_outputs(out, self.scale))
            for k, w in enumerate(part):
                self.merger.add(w, det[k * T:(k + 1) * T], fused[k * T:(k + 1) * T], others[k * T:(k + 1) * T])

    def _emit(self, upto):
        det, fused, others = self.merger.pop(upto)
        res = dict(first=self.emitted, det=det, fused=fused, others=others)
        self.emitted += det.shape[0]
        return res

    def push(self, frames, img_hw=None):
        """frames [n,3,H,W] f32 (preprocessed like engine.forward's input); img_hw: [n,2] img_shape per frame or None.
        -> the frames that became final (possibly none)."""
        n, i = frames.shape[0], 0
        while i < n:
            m = min(n - i, self.ring.free())
            if m <= 0:
                raise L.McgError('GazeStream: the pyramid ring has no free row (capacity too small)')
            self.ring.append(frames[i:i + m], None if img_hw is None else np.asarray(_host(img_hw)).reshape(n, 2)[i:i + m])
            wins = self.planner.feed(m)
            if wins:
                self._decode(wins)
            self.ring.release(self.planner.keep_from)
            i += m
        return self._emit(self.planner.final_upto)

    def finish(self):
        """End of the stream: the windows that depend on its length, and every frame not returned yet."""
        wins = self.planner.finish()
        if wins:
            self._decode(wins)
        return self._emit(self.planner.frames)
