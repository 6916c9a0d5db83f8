"""Caller of the hot path: the reference's inference harness logic --
sliding 7-frame windows with stride 4 over every video, one forward per window, overlap merging, result
records -- restated from tools/test_gaze360_gaze.py:60-269 so that whole videos can be pushed through the
engine in large batches (the reference runs one clip per forward).

Semantics kept exactly (pinned by tests/golden/harness_merge.json, produced by running the reference's own
``main`` on a seeded fake model):
  * windows (:72-86): ``clip_num = ceil((L-7)/4)+1``; the last window is the LAST 7 frames; a video with
    L <= 7 frames is one short clip of T = L frames (so T is variable);
  * merge (:129-206): the first window is taken verbatim; later windows append their new frames and average the
    overlapping ones ``(old+new)/2`` -- gaze vectors are NOT re-normalised; box coordinates are zeroed where the
    score is < 0.5 in either prediction (the stored score may itself be an average);
  * record schema (:210-260): per frame fused gaze, per-clue boxes as [x, y, w, h] or None when zeroed, gazes, scores.
"""
import collections
import json
import math
import os

import numpy as np
import torch

from .attention import END_VIDEO_ENDED, KIND_HEAD, KIND_REGION, MAX_COLUMNS, MAX_ROWS, _attention_options, _dwell_options, _heat_options, _surface_options, open_episodes
from .engine import _upload_table
from .arrows import OVERLAY_PALETTE, _anon_params, _label_options, _overlay_options, format_labels_host
from .pipeline import ARROW_COLOR, _track_motion, _track_params, letterbox_geometry

CLUES = ('face', 'eyes', 'head')
last_run_stats = {}       # run_annotation's frame-cache counters of the last call (tools/dataset_throughput.py prints them); trunk_frames of run_videos


def plan_windows(video_length, clip_len=7, stride=4):
    """-> list of (start, stop, overlap_with_previous).  tools/test_gaze360_gaze.py:72-86."""
    L = video_length
    if L <= clip_len:
        return [(0, L, 0)]
    clip_num = math.ceil((L - clip_len) / stride) + 1
    out = []
    for i in range(clip_num):
        if i != clip_num - 1:
            out.append((i * stride, i * stride + clip_len, clip_len - stride))
        else:
            rem = (L - clip_len) % stride
            out.append((L - clip_len, L, clip_len - rem if rem else clip_len - stride))
    return out


def _host(t):
    """torch tensor (any device) or array -> numpy array on the host (a view where possible)."""
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def merge_window(det, fused, others, base, first, window, d, f, o, thr):
    """One step of the overlap merge (tools/test_gaze360_gaze.py:129-206): window = (start, stop, overlap) of the plan with outputs
    d [T,3,5], f [T,3], o [T,3,3] (torch tensors or numpy arrays, f32) into the per-frame buffers det / fused / others, whose row 0 is frame
    ``base``; windows come in plan order, ``first`` marks the plan's first.  Host arithmetic in f32 -- sums and halvings, exactly rounded,
    the same bits the reference's torch expressions give."""
    start, stop, overlap = window
    d, f, o = _host(d), _host(f), _host(o)
    half = np.float32(2)
    low = d[..., 4:] < thr
    d = np.concatenate([np.where(low, np.float32(0), d[..., :4]), d[..., 4:]], axis=-1)      # boxes of low-score detections are zeroed (:140-150)
    if first:
        det[start - base:stop - base], fused[start - base:stop - base], others[start - base:stop - base] = d, f, o
        return
    # overlapping frames: the last `overlap` stored frames against the first `overlap` frames of this window
    ov = slice(start - base, start + overlap - base)
    old_d, cur_d = det[ov], d[:overlap]
    bad = (old_d[..., 4:] < thr) | low[:overlap]
    det[ov, :, :4] = np.where(bad, np.float32(0), (old_d[..., :4] + cur_d[..., :4]) / half)
    det[ov, :, 4:] = (old_d[..., 4:] + cur_d[..., 4:]) / half
    fused[ov] = (fused[ov] + f[:overlap]) / half
    others[ov] = (others[ov] + o[:overlap]) / half
    new = slice(start + overlap - base, stop - base)
    det[new], fused[new], others[new] = d[overlap:], f[overlap:], o[overlap:]


def merge_video(windows, clip_outputs, person_threshold=0.5):
    """windows from plan_windows; clip_outputs[i] = (det_bboxes [T,3,5], fused [T,3], others [T,3,3]) of window i (torch tensors or
    numpy arrays, f32).  Returns per-frame numpy arrays (det_bboxes [L,3,5], fused [L,3], others [L,3,3]): merge_window over the plan;
    the windows of a video tile it from frame 0 with the last one flush to the end, so frame t of window (start, stop) lands at row
    start + t."""
    L = windows[-1][1]
    det, fused, others = np.empty((L, 3, 5), np.float32), np.empty((L, 3), np.float32), np.empty((L, 3, 3), np.float32)
    for i, (window, (d, f, o)) in enumerate(zip(windows, clip_outputs)):
        merge_window(det, fused, others, 0, i == 0, window, d, f, o, np.float32(person_threshold))
    return det, fused, others


def merge_plan(windows, row_of, written, num_frames=None, store_rows=None):
    """The table mcg_merge_windows takes for ONE decoder call: merge_window turned inside out.  merge_window applies windows one after the
    other and its result is not associative (at clip_len 7, stride 4, L = 12 frames 5 and 6 become ((a + b) / 2 + c) / 2), so windows
    cannot run in parallel -- but frames can: every destination frame gets the decoder-output frames that land on it, in plan order.

    windows: [(stream key, (start, stop, overlap), first output row)] in call order -- frame start + t of the stream is row first + t of the
    call's outputs; per stream the windows are in plan order.  row_of(key, frame) -> the store row of that frame.  written: the frames
    that hold state from an EARLIER call, anything that answers ``(key, frame) in written``.
    -> (int32 [num_dst, 2 + max_src]: dst_row, cont, src[max_src] padded with -1; max_src).  cont = 1 exactly when an earlier call wrote
    that frame: the fold starts from the stored row.  max_src: the longest source list of the call (at least 1).
    ValueError: windows of one stream out of plan order (starts and stops must rise, and the frames of a window that already hold state
    must be its first ``overlap`` ones -- what merge_window averages), an output row outside [0, num_frames), a store row outside
    [0, store_rows) or named by two frames (the last three only when the bound is given)."""
    order, sources, last = [], {}, {}
    for key, (start, stop, overlap), first in windows:
        start, stop, first = int(start), int(stop), int(first)
        if stop <= start:
            raise ValueError(f'merge_plan: empty window ({start}, {stop}) of stream {key!r}')
        if first < 0 or (num_frames is not None and first + stop - start > num_frames):
            raise ValueError(f'merge_plan: window ({start}, {stop}) of stream {key!r} reads output rows {first}..{first + stop - start - 1}, '
                             f'outside the call\'s {num_frames} frames')
        prev = last.get(key)
        if prev is not None and not (start > prev[0] and stop > prev[1]):
            raise ValueError(f'merge_plan: window ({start}, {stop}) of stream {key!r} follows {prev}: windows must come in plan order')
        held = [((key, f) in sources) or ((key, f) in written) for f in range(start, stop)]
        k = sum(held)
        if any(held[k:]) or (k != overlap and (k or prev is not None)):
            raise ValueError(f'merge_plan: window ({start}, {stop}, {overlap}) of stream {key!r} is out of plan order: {k} of its frames hold '
                             'state, and they must be its first `overlap` ones')
        last[key] = (start, stop)
        for t in range(stop - start):
            kf = (key, start + t)
            if kf not in sources:
                sources[kf] = []
                order.append(kf)
            sources[kf].append(first + t)
    max_src = max([len(s) for s in sources.values()] + [1])
    table = np.full((len(order), 2 + max_src), -1, dtype=np.int32)
    for i, kf in enumerate(order):
        r = int(row_of(*kf))
        if r < 0 or (store_rows is not None and r >= store_rows):
            raise ValueError(f'merge_plan: frame {kf[1]} of stream {kf[0]!r} has store row {r}, outside the store of {store_rows} rows')
        table[i, 0], table[i, 1] = r, int(kf in written)
        table[i, 2:2 + len(sources[kf])] = sources[kf]
    if len(set(table[:, 0].tolist())) != len(order):
        raise ValueError('merge_plan: two frames share a store row')
    return table, max_src


def check_smooth(who, smooth):
    """The ``smooth=`` option: None, or smooth_filter's alpha as a number in (0, 1] -> None or the float."""
    if smooth is None:
        return None
    if isinstance(smooth, bool) or not isinstance(smooth, (int, float, np.integer, np.floating)) or not 0 < float(smooth) <= 1:
        raise ValueError(f'{who}: smooth is None or the filter\'s alpha, a number in (0, 1] (got {smooth!r})')
    return float(smooth)


def smooth_host(g, alpha, lead=False, trail=False):
    """The temporal filter of tools/calculate_mae_gaze360.py:16-29 (smooth_filter) on the host, in the arithmetic mcg_smooth_gaze has
    (include/mcgaze_hip.h states it): g [m, ..., 3] f32, consecutive frames of one stream -> the smoothed frames, same trailing shape.
    lead / trail: g[0] / g[-1] is there only as a neighbour (the frame handed out before, the frame not handed out yet) and gets no output
    row; without them g[0] is the stream's first frame and g[-1] its last.  A one-frame stream comes back as it is, not normalised.
    Everything is f32 numpy, which contracts nothing; each of the norm's two fma is taken in float64 and rounded once."""
    g = np.asarray(g, dtype=np.float32)
    m, lo = g.shape[0], int(bool(lead))
    hi = m - int(bool(trail))
    if hi <= lo:
        return g[:0].copy()
    if m == 1:
        return g.copy()
    a, b = np.float32(alpha), np.float32(1.0 - float(alpha))
    x, at = g[lo:hi], np.arange(lo, hi)
    p, q = g[np.maximum(at - 1, 0)], g[np.minimum(at + 1, m - 1)]
    shape = (-1,) + (1,) * (g.ndim - 1)
    has_p, has_q = (at > 0).reshape(shape), (at < m - 1).reshape(shape)
    with np.errstate(all='ignore'):
        o = a * x
        o = np.where(has_p & has_q, o + (b * (p + q)) / np.float32(2), o + b * np.where(has_p, p, q))
        d = o.astype(np.float64)
        n = (d[..., 1] * d[..., 1] + (o[..., 0] * o[..., 0]).astype(np.float64)).astype(np.float32)
        n = np.sqrt((d[..., 2] * d[..., 2] + n.astype(np.float64)).astype(np.float32))
        return o / n[..., None]


def smooth_plan(frames, row_of, first=0, last=None, store_rows=None):
    """The table mcg_smooth_gaze takes for the frames of ONE stream that are about to be handed out: int32 [k, 3] = (row of the frame
    before, row of the frame, row of the frame after), in the order of ``frames``.  row_of(frame) -> its store row.  -1 stands for the
    previous row of frame ``first`` (the stream's first frame) and for the next row of frame ``last`` (its last one, known only once the
    stream has ended: None before).  ValueError: a row that is negative or (store_rows given) at or past store_rows."""
    frames = [int(f) for f in frames]
    table = np.full((len(frames), 3), -1, dtype=np.int32)
    for i, f in enumerate(frames):
        for j, g in enumerate((f - 1, f, f + 1)):
            if (j == 0 and f == first) or (j == 2 and last is not None and f == last):
                continue
            r = int(row_of(g))
            if r < 0 or (store_rows is not None and r >= store_rows):
                raise ValueError(f'smooth_plan: frame {g} has store row {r}, outside the store of {store_rows} rows')
            table[i, j] = r
    return table


def video_record(video_id, det, fused, others, smoothed=None):
    """Result record of one video (tools/test_gaze360_gaze.py:210-260): python floats of the f32 values; a box is [x, y, w, h] with
    the differences taken in double (the reference subtracts python floats), or None where the four coordinates sum to zero.
    smoothed = (fused [L,3], others [L,3,3]) after the temporal filter adds ``fusion_gazes_smooth`` and ``<clue>_gazes_smooth``."""
    det, fused, others = _host(det), _host(fused), _host(others)
    rec = dict(video_id=video_id, category_id=1, fusion_gazes=fused.tolist())
    if smoothed is not None:
        rec['fusion_gazes_smooth'] = _host(smoothed[0]).tolist()
        for ci, c in enumerate(CLUES):
            rec[f'{c}_gazes_smooth'] = _host(smoothed[1])[:, ci].tolist()
    m = det[..., :4].astype(np.float64)
    empty = (((m[..., 0] + m[..., 1]) + m[..., 2]) + m[..., 3] == 0).tolist()
    xywh = np.stack([m[..., 0], m[..., 1], m[..., 2] - m[..., 0], m[..., 3] - m[..., 1]], axis=-1).tolist()
    gazes, score = others.tolist(), det[..., 4].tolist()
    for ci, c in enumerate(CLUES):
        rec[f'{c}_bboxes'] = [None if e[ci] else b[ci] for e, b in zip(empty, xywh)]
        rec[f'{c}_gazes'] = [g[ci] for g in gazes]
        rec[f'{c}_score'] = [sc[ci] for sc in score]
    return rec


def result_file_name(config_path, json_path):
    """``results_<config stem>_<annotation file name>`` (tools/test_gaze360_gaze.py:268; note rstrip('.py') semantics)."""
    return f'results_{config_path.rstrip(".py").split("/")[-1]}_{json_path.split("/")[-1]}'


FUSED_ATTN_MAX_T = 10     # longest clip the fused attention block takes (3 T <= 32 token rows: one MFMA tile, csrc/attn_block.hpp)
ROW, SMOOTH_ROW = 27, 12  # columns of a result row (pack_rows): det 3x5 | fused 3 | others 3x3, and of what smooth= adds: fused_smooth 3 | others_smooth 3x3


def bucket_key(H, W, T, mixed):
    """The batch a clip of T frames of H x W joins.  mixed (clips of different lengths in one ragged call): (H, W, longest-clip class), the
    classes T <= 10 and T > 10, so that one long clip does not push a batch of short ones off the fused attention block; else (T, H, W)."""
    return (H, W, int(T > FUSED_ATTN_MAX_T)) if mixed else (T, H, W)


def clip_outputs(out, scale=None):
    """Engine output dict(gaze [4,n,3], boxes [n,3,4], scores [n,3]) -> (det [n,3,5] = box | score, fused [n,3], others [n,3,3]) on its
    device: merge_video's layout.  scale (broadcastable to the boxes): rescale=True, every frame's boxes divided by its scale_factor
    (multiclue_gaze_roi_head.py:360-363)."""
    boxes = out['boxes'] if scale is None else out['boxes'] / scale
    return torch.cat([boxes, out['scores'][..., None]], dim=-1), out['gaze'][0], out['gaze'][1:].permute(1, 0, 2)


def pack_rows(det, fused, others, fused_smooth=None, others_smooth=None):
    """clip_outputs' / merge_video's (det [k,3,5], fused [k,3], others [k,3,3])[, the smoothed fused and others] -> ONE [k,27] or [k,39] array
    of result rows: numpy arrays or torch tensors alike, one concatenation."""
    parts = [det, fused, others] + ([] if fused_smooth is None else [fused_smooth, others_smooth])
    parts = [p.reshape(det.shape[0], w) for p, w in zip(parts, (15, 3, 9, 3, 9))]
    return torch.cat(parts, dim=1) if isinstance(det, torch.Tensor) else np.concatenate(parts, axis=1)


def split_rows(r):
    """pack_rows' inverse: [k,27] -> (det, fused, others), [k,39] -> the five parts, all views of r.  ValueError on any other width."""
    if r.ndim != 2 or r.shape[1] not in (ROW, ROW + SMOOTH_ROW):
        raise ValueError(f'split_rows: result rows have {ROW} or {ROW + SMOOTH_ROW} columns (got shape {tuple(r.shape)})')
    k = r.shape[0]
    out = (r[:, :15].reshape(k, 3, 5), r[:, 15:18], r[:, 18:27].reshape(k, 3, 3))
    return out if r.shape[1] == ROW else out + (r[:, 27:30], r[:, 30:39].reshape(k, 3, 3))


def _run_windows(engine, ids, plans, get_window, batch_clips, person_threshold, reuse_frames=False, mixed_lengths=False, merge='host',
                 smooth=None):
    """Core of run_videos / run_annotation, STREAMING: windows are visited in (video, window) order -- the reference's order, so the
    crop RNG draws inside ``get_window`` fall where upstream's do -- and dropped into per-(T, H, W) buckets; a bucket runs through
    the engine (batched semantics: N = B*T frames, clip_length = T) as soon as it holds ``batch_clips`` clips and its inputs are
    released; a video is merged and turned into its record as soon as its last window has come back.  Device memory is bounded by
    ``batch_clips`` clips per distinct window shape, not by the size of the dataset.
    get_window(vi, wi) -> (frames [T,3,H,W] f32, img_hw [T,2] int or None, scale [T,4] f32 or None).
    reuse_frames: frame t of window (a, b) of video vi IS frame a + t of the video: each distinct (video, frame) of a flush goes through the
    trunk once, into one row of a pyramid store, and one indexed decoder call (engine.decode) reads the windows' frames from it -- the
    same batch of windows as forward would run, so the same bits.  ``trunk`` counts the frames run through the trunk.
    mixed_lengths: windows of DIFFERENT lengths share a bucket -- keyed (H, W, longest-clip class) with the classes T <= 10 and T > 10, so
    that one long clip does not push a bucket of short windows off the fused attention block -- and a flush is one ragged forward / decode
    (clip_length = the list of the windows' lengths): a video shorter than clip_len no longer runs alone.  A window's results do not
    depend on its batch, so the records are those of the default bucketing.
    merge='device': every flush is folded into a stream.DeviceMerger (one mcg_merge_windows launch per engine call; a video's windows share
    one bucket, so they arrive in plan order) and a video's merged frames come to the host in ONE copy once its last window has run.
    smooth: None, or the alpha of the temporal filter (smooth_host; merge='device': mcg_smooth_gaze, one launch per video, its rows go
    to the host in the same copy) -- every record then also holds the smoothed gazes (video_record)."""
    if merge not in ('host', 'device'):
        raise ValueError(f"merge is 'host' or 'device' (got {merge!r})")
    smooth = check_smooth('run_videos', smooth)
    dev = engine.device
    merger = None
    if merge == 'device':
        from .stream import DeviceMerger               # McgError on an engine without a HIP device: no CPU fallback
        merger = DeviceMerger(dev, person_threshold, rows=2 * batch_clips * max([p[0][1] - p[0][0] for p in plans if p] + [1]), smooth=smooth)
    merged = []                                        # merge='device': (vi, pinned [L, 27], event) of the videos on their way to the host
    trunk = [0]
    buckets = {}                                       # (T, H, W) -> list of (vi, wi, frames, hw, scale)
    outputs = [[None] * len(p) for p in plans]
    pending = [len(p) for p in plans]
    records = [None] * len(plans)

    inflight = collections.deque()                     # batches whose results are on their way to the host: (items (vi, wi, T), pinned buffer, event)
    spare = []                                         # pinned result buffers free for reuse

    def upload(t):                                     # small per-batch tables (img_shape, scale_factor)
        return _upload_table(t, dev)

    def collect(leave):
        # results of finished batches -> per-window host arrays -> (once a video's last window is back) merge + record, all on the host:
        # the consumer never waits for a forward it has just queued (round 3 / 4 did, in video_record's .cpu(): host and device took turns)
        while len(inflight) > leave or (inflight and (inflight[0][2] is None or inflight[0][2].query())):
            items, buf, ev = inflight.popleft()
            if ev is not None:
                ev.synchronize()
            res = buf[:sum(T for _, _, T in items)].numpy().copy()  # [frames, 27] result rows; copied: the pinned buffer is reused
            if ev is not None:
                spare.append(buf)
            parts, row = split_rows(res), 0
            for vi, wi, T in items:
                outputs[vi][wi] = tuple(p[row:row + T] for p in parts)
                row += T
                pending[vi] -= 1
                if pending[vi] == 0:                   # all windows of the video are back: merge, record, release
                    whole = merge_video(plans[vi], outputs[vi], person_threshold)
                    records[vi] = video_record(ids[vi], *whole, None if smooth is None else (smooth_host(whole[1], smooth), smooth_host(whole[2], smooth)))
                    outputs[vi] = None

    def length_of(it):
        a, b, _ = plans[it[0]][it[1]]
        return b - a

    def decode_distinct(items, Ts):
        # rows of the pyramid store: the distinct (video, frame) of the batch, in order of first appearance; runs of consecutive frames
        # of one window are taken as slices
        row_of, parts, hws, table = {}, [], [], []
        for (vi, wi, x, hw, _), T in zip(items, Ts):
            a = plans[vi][wi][0]
            for t in range(T):
                k = (vi, a + t)
                if k not in row_of:
                    row_of[k] = len(row_of)
                    if parts and parts[-1][0] is x and parts[-1][2] == t:
                        parts[-1][2] = t + 1
                    else:
                        parts.append([x, t, t + 1])
                    if hw is not None:
                        hws.append(np.asarray(hw, dtype=np.int32).reshape(-1, 2)[t])
                table.append(row_of[k])
        x = torch.cat([p[0][p[1]:p[2]] for p in parts]).to(dev, torch.float32).contiguous()
        hw = None if items[0][3] is None else upload(torch.from_numpy(np.stack(hws)))
        pyr = engine.backbone_fpn(x)
        trunk[0] += x.shape[0]
        return engine.decode(pyr, table, Ts if mixed_lengths else Ts[0], img_hw=hw)

    def flush(key):
        items = buckets.pop(key, [])
        if not items:
            return
        Ts = [length_of(it) for it in items]         # default bucketing: all equal (the key's T)
        collect(2)
        if reuse_frames:
            out = decode_distinct(items, Ts)
        else:
            x = torch.cat([it[2] for it in items]).to(dev, torch.float32).contiguous()
            hw = None if items[0][3] is None else upload(torch.cat([torch.as_tensor(it[3], dtype=torch.int32).reshape(-1, 2) for it in items]))
            out = engine.forward(x, Ts if mixed_lengths else Ts[0], img_hw=hw)
            trunk[0] += x.shape[0]
        scale = None      # rescale=True: every frame's boxes by its own scale_factor
        if items[0][4] is not None:
            scale = upload(torch.cat([torch.as_tensor(it[4], dtype=torch.float32) for it in items]))[:, None, :]
        n = sum(Ts)
        if merger is not None:
            rows = np.concatenate([[0], np.cumsum(Ts)]).tolist()
            merger.add_call([(it[0], plans[it[0]][it[1]], r) for it, r in zip(items, rows)], out, scale)
            for it in items:
                vi = it[0]
                pending[vi] -= 1
                if pending[vi] == 0:                   # the video's last window is queued: its frames leave the store in one copy
                    packed, smoothed, _ = merger.pop_rows([(vi, plans[vi][-1][1])], ended=(vi,))   # ended: the whole video at once, no frame waits for its successor
                    if smoothed is not None:
                        packed = torch.cat([packed, smoothed], dim=1)
                    merger.forget(vi)
                    buf = torch.empty(packed.shape[0], packed.shape[1], dtype=torch.float32).pin_memory()
                    buf.copy_(packed, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(dev))
                    merged.append((vi, buf, ev))
            return
        packed = pack_rows(*clip_outputs(out, scale)).to(torch.float32)   # ONE copy to the host
        who = [(it[0], it[1], T) for it, T in zip(items, Ts)]
        if dev.type != 'cuda':
            inflight.append((who, packed, None))
            return
        buf = next((b for b in spare if b.shape[0] >= n), None)
        if buf is not None:
            spare.remove(buf)
        else:
            buf = torch.empty(max(n, batch_clips * max(Ts)), ROW, dtype=torch.float32).pin_memory()
        buf[:n].copy_(packed, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        inflight.append((who, buf, ev))

    for vi, plan in enumerate(plans):
        for wi in range(len(plan)):
            x, hw, sc = get_window(vi, wi)
            T = plan[wi][1] - plan[wi][0]
            key = bucket_key(x.shape[-2], x.shape[-1], T, mixed_lengths)
            buckets.setdefault(key, []).append((vi, wi, x, hw, sc))
            if len(buckets[key]) >= batch_clips:
                flush(key)
    for key in sorted(buckets):
        flush(key)
    collect(0)
    for vi, buf, ev in merged:
        ev.synchronize()
        r = split_rows(buf.numpy())
        records[vi] = video_record(ids[vi], *r[:3], r[3:] or None)
    last_run_stats['trunk_frames'] = trunk[0]
    return records


def run_videos(engine, videos, clip_len=7, stride=4, batch_clips=64, scale_factor=None, person_threshold=0.5, reuse_frames=False,
               mixed_lengths=False, merge='host', smooth=None):
    """Push whole videos through the HIP engine.

    videos: list of dict(id=…, frames=Tensor[L,3,H,W] f32 already preprocessed (normalised, padded to /32)[, img_hw=[L,2] int: the
    per-frame img_shape inside the padded frame -- all videos or none]).
    scale_factor (4 floats) divides the boxes like rescale=True does (multiclue_gaze_roi_head.py:360-363).
    reuse_frames: overlapping windows share their frames' trunk.  Each batch runs every distinct (video, frame) of its windows through
    backbone + FPN once, into a pyramid store, then one indexed decoder call over the batch's windows (engine.decode): about 4 / 7 of the
    trunk work at (7, 4) on long videos, records == those of the default path (which runs engine.forward on every window's frames).
    Frames shared by windows that land in different batches are computed in each: at most clip_len - stride per video per batch
    boundary.  last_run_stats['trunk_frames'] holds the frames the trunk ran on, for both settings.
    mixed_lengths: windows of different lengths (videos shorter than clip_len) share batches -- one ragged engine call per flush
    (_run_windows); the records are those of the default.
    merge='device': the overlap merge runs on the device (mcg_merge_windows, one launch per engine call) and every video comes to the
    host in one copy -- the same records; McgError on an engine without a HIP device.
    smooth: None, or the alpha in (0, 1] of the temporal filter the reference's metric runs over every video before the angular error
    (tools/calculate_mae_gaze360.py:16-29, alpha 0.6 there): every record gains ``fusion_gazes_smooth`` and ``<clue>_gazes_smooth``, the
    filtered gazes (mcg_smooth_gaze's arithmetic; on the device with merge='device'); everything else in it is unchanged."""
    plans = [plan_windows(v['frames'].shape[0], clip_len, stride) for v in videos]

    def get_window(vi, wi):
        a, b, _ = plans[vi][wi]
        sc = None if scale_factor is None else torch.as_tensor(scale_factor, dtype=torch.float32).expand(b - a, 4)
        hw = videos[vi].get('img_hw')
        return videos[vi]['frames'][a:b], (None if hw is None else hw[a:b]), sc

    return _run_windows(engine, [v['id'] for v in videos], plans, get_window, batch_clips, person_threshold, reuse_frames=reuse_frames,
                        mixed_lengths=mixed_lengths, merge=merge, smooth=smooth)


def expected_frame_bytes(path):
    """What a decode-ring slot will really hold for a run that starts with the image file ``path``: twice its decoded size (frames of a dataset
    vary), from the file's header alone (no decode) -- the /dev/shm check of the decode ring (frame_cache.FrameCache) prices a slot at that instead
    of the 3 MiB worst case (a 360 x 360 frame is 390 KB).  None where the header cannot be read."""
    try:
        from PIL import Image
        with Image.open(path) as im:
            return 2 * im.size[0] * im.size[1] * 3
    except (OSError, ValueError):
        return None


def run_annotation(engine, anno, root, pipeline, clip_len=7, stride=4, batch_clips=64, person_threshold=0.5, rng=None, workers=0, lookahead=None,
                   processes=False, video_rng=None, mixed_lengths=False):
    """tools/test_gaze360_gaze.py:57-269 from the annotation file down: for every ``anno['videos']`` entry (``id``,
    ``file_names``) each window's frames are loaded and preprocessed ANEW through ``pipeline`` (a
    mcgaze_amd.pipeline.DevicePipeline built from cfg.data.test.pipeline) -- like the reference, which re-runs its test
    pipeline, random crop included, for every window (:88-100) -- then all windows go through the engine in large batches
    and are merged per video.  Frames of a window are drawn in file-name order (the reference sorts its threads' results by
    file name, :96); ``rng`` seeds the crop draws (default: the global numpy RNG, as upstream).
    Each file is decoded once while it stays cached (windows overlap by three frames); windows are preprocessed in groups (one
    pinned copy and one launch per padded size).  ``workers`` > 0 adds host threads that decode ``lookahead`` windows ahead of the
    consumer (the reference uses 7 loader threads per window, :88-95) -- measured slower than in-line decoding for small frames
    (frame_cache.FrameCache), hence 0 by default; ``processes=True`` makes them helper PROCESSES that decode into a shared-memory ring (no
    interpreter lock in common with this loop).  The records do not depend on any of it.
    ``video_rng``: video id -> numpy RandomState.  With it every video draws its crops from its OWN generator (created when its first
    window is planned) instead of the shared ``rng``: the records then do not depend on which videos a process was given or in what
    order -- what a run sharded over several consumer processes needs to reproduce a single-process run record for record (the
    reference's single global generator makes its results depend on the shard layout).
    ``mixed_lengths``: as in run_videos -- windows of different lengths in one ragged engine call per flush; same records."""
    from .pipeline import FrameCache
    rng = np.random if rng is None else rng
    videos = anno['videos']
    plans = [plan_windows(len(v['file_names']), clip_len, stride) for v in videos]
    order = [(vi, wi) for vi, plan in enumerate(plans) for wi in range(len(plan))]     # the order _run_windows visits windows in
    pos = {vw: i for i, vw in enumerate(order)}
    lookahead = 2 * batch_clips if lookahead is None else lookahead
    group = max(1, min(batch_clips, 32))                                    # windows staged per preprocessing call
    frame_bytes = None
    if workers > 0 and processes and videos and videos[0]['file_names']:
        name = videos[0]['file_names'][0]
        frame_bytes = expected_frame_bytes(os.path.join(root, name) if root is not None else name)
    cache = FrameCache(workers, capacity=((lookahead if workers > 0 else 0) + group + 2) * clip_len, processes=processes, frame_bytes=frame_bytes)   # in-line decoding never runs ahead: only the staged group (and the 3-frame overlap) is worth keeping
    state = dict(ahead=0)

    def names_of(vi, wi):
        a, b, _ = plans[vi][wi]
        return sorted(videos[vi]['file_names'][a:b])

    staged = {}
    per_video = {}

    def rng_of(vi):
        if video_rng is None:
            return rng
        if vi not in per_video:
            per_video[vi] = video_rng(videos[vi]['id'])
        return per_video[vi]

    def get_window(vi, wi):
        i = pos[(vi, wi)]
        if i not in staged:
            # stage the next `group` windows in one go (one pinned copy, one launch per padded size); planned in visiting order, so
            # the crop draws fall exactly where they do one window at a time
            todo = order[i:i + group]
            if workers > 0:
                while state['ahead'] < min(i + len(todo) + lookahead, len(order)):   # decoders stay `lookahead` windows ahead
                    v2, w2 = order[state['ahead']]
                    cache.prefetch(os.path.join(root, n) if root is not None else n for n in names_of(v2, w2))
                    state['ahead'] += 1
            res = pipeline.run_many([names_of(v2, w2) for v2, w2 in todo], device=engine.device, rng=[rng_of(v2) for v2, _ in todo], img_prefix=root, loader=cache)
            staged.update({i + k: r for k, r in enumerate(res)})
        img, metas = staged.pop(i)
        hw = [m['img_shape'][:2] for m in metas]
        return img, hw, np.stack([m['scale_factor'] for m in metas])

    try:
        return _run_windows(engine, [v['id'] for v in videos], plans, get_window, batch_clips, person_threshold, mixed_lengths=mixed_lengths)
    finally:
        last_run_stats.update(decodes=cache.decodes, decode_waits=cache.waits, decode_wait_s=round(cache.wait_s, 3), decode_first_wait_s=round(cache.first_wait_s, 3))
        cache.close()


def plan_track_chunks(track_length, max_len=100):
    """-> list of (start, stop): how the reference's demo cuts one person's track into clips (MCGaze_demo/demo.ipynb, cell 4): frames are
    gathered one by one and run as ONE clip as soon as more than max_len are held (``len(datas) > max_len``) or the track ends -- so
    consecutive chunks of max_len + 1 frames, the last one shorter; an empty track gives no chunk."""
    step = max_len + 1
    return [(a, min(a + step, track_length)) for a in range(0, track_length, step)]


def run_tracks(engine, tracks, max_len=100, batch_frames=448, scale_factor=None):
    """The inference loop of the reference's demo (MCGaze_demo/demo.ipynb, cell 4) on preprocessed frames: one clip per (person, segment),
    as long as the person stays in view, cut every max_len + 1 frames -- where the demo runs one forward per chunk, the chunks of ALL
    tracks are batched here as clips of different lengths (engine.forward(x, [lengths])).

    tracks: list of dict(id=..., frames=Tensor[L,3,H,W] f32 preprocessed head crops (normalised, padded to /32)[, img_hw=[L,2] int -- a host
    array or a device tensor, sliced per chunk where it is][, scale_factor=[L,4] f32 per FRAME, host or device]), one per (person, segment).
    Chunks (plan_track_chunks) are visited in (track, chunk) order and batched per (H, W, longest-clip class) -- chunks
    of at most 10 frames and longer ones in separate calls, so that short clips keep the fused attention block -- up to batch_frames
    frames per call (a single chunk may exceed it and then runs alone).  No overlap merge: the demo has none; a track's outputs are its
    chunks' outputs concatenated.  scale_factor divides the boxes like rescale=True (the demo's setting), on the device: the argument (4
    floats) for every frame alike, a track's own table frame by frame (img_hw and scale_factor: all tracks or none).
    Returns one dict(id, det [L,3,5], fused [L,3], others [L,3,3]) per track, numpy f32 in merge_video's layout (det = box | score).
    Head detection stays with the caller; run_head_video cuts the crops from full frames and a detector's boxes."""
    dev = engine.device
    plans = [plan_track_chunks(int(t['frames'].shape[0]), max_len) for t in tracks]
    parts = [[None] * len(p) for p in plans]
    buckets = {}                                       # (H, W, class) -> list of (ti, ci)

    def flush(key):
        items = buckets.pop(key, [])
        if not items:
            return
        spans = [plans[ti][ci] for ti, ci in items]
        Ts = [b - a for a, b in spans]
        x = torch.cat([tracks[ti]['frames'][a:b] for (ti, _), (a, b) in zip(items, spans)]).to(dev, torch.float32).contiguous()
        first = tracks[items[0][0]]
        hw = None
        if isinstance(first.get('img_hw'), torch.Tensor):
            hw = torch.cat([tracks[ti]['img_hw'].reshape(-1, 2)[a:b] for (ti, _), (a, b) in zip(items, spans)])
        elif first.get('img_hw') is not None:
            hw = np.concatenate([np.asarray(tracks[ti]['img_hw'], dtype=np.int32).reshape(-1, 2)[a:b] for (ti, _), (a, b) in zip(items, spans)])
        out = engine.forward(x, Ts, img_hw=hw)
        bdev = out['boxes'].device
        scale = None if scale_factor is None else torch.as_tensor(scale_factor, dtype=torch.float32, device=bdev)
        if first.get('scale_factor') is not None:      # per frame: [n,1,4] against boxes [n,3,4]
            scale = torch.cat([torch.as_tensor(tracks[ti]['scale_factor'], dtype=torch.float32).reshape(-1, 4)[a:b].to(bdev)
                               for (ti, _), (a, b) in zip(items, spans)])[:, None, :]
        det, fused, others = (_host(t) for t in clip_outputs(out, scale))
        row = 0
        for (ti, ci), T in zip(items, Ts):
            parts[ti][ci] = (det[row:row + T], fused[row:row + T], others[row:row + T])
            row += T

    for ti, plan in enumerate(plans):
        fr = tracks[ti]['frames']
        for ci, (a, b) in enumerate(plan):
            key = bucket_key(fr.shape[-2], fr.shape[-1], b - a, True)
            held = sum(plans[t][c][1] - plans[t][c][0] for t, c in buckets.get(key, []))
            if held and held + (b - a) > batch_frames:
                flush(key)
            buckets.setdefault(key, []).append((ti, ci))
    for key in sorted(buckets):
        flush(key)
    out = []
    for t, p in zip(tracks, parts):
        cat = lambda k, shape: np.concatenate([c[k] for c in p]) if p else np.zeros(shape, np.float32)
        out.append(dict(id=t['id'], det=cat(0, (0, 3, 5)), fused=cat(1, (0, 3)), others=cat(2, (0, 3, 3))))
    return out


def read_head_labels(path, head_class=1):
    """One label file of the demo's ``result/labels`` (the YOLO head detector's ``--save-txt`` output; MCGaze_demo/demo.ipynb, cell 1) ->
    list of [x1, y1, x2, y2], one per line whose class is ``head_class``, in file order.  Lines are ``class x1 y1 x2 y2`` separated by
    blanks; a field is an int where it reads as one and a float otherwise -- what the notebook's ``eval`` gives, without evaluating
    anything.  Blank lines are skipped."""
    def number(tok):
        try:
            return int(tok)
        except ValueError:
            return float(tok)

    boxes = []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if len(tok) < 5:
                raise ValueError(f'{path}: expected "class x1 y1 x2 y2", got {line.strip()!r}')
            v = [number(t) for t in tok[:5]]
            if v[0] == head_class:
                boxes.append(v[1:5])
    return boxes


def segment_tracks(boxes_per_frame):
    """Cell 1 of the demo (MCGaze_demo/demo.ipynb): boxes_per_frame[t] = the head boxes [x1, y1, x2, y2] of frame t, any order ->
    list of dict(frame_id=[t, ...], boxes=[P][L][4]).  A new segment starts wherever the NUMBER of heads changes; inside a frame people
    are ordered by x1 (a stable sort, like the notebook's), and person i of a segment is the i-th box of each of its frames -- the demo
    has no other notion of identity.  Frames without a head belong to no segment and end the one before them (the notebook opens a
    segment of zero people there, and fails on a video that starts with such a frame)."""
    segments, cur, count = [], None, 0
    for t, boxes in enumerate(boxes_per_frame):
        boxes = sorted([list(b) for b in boxes], key=lambda b: b[0])
        if len(boxes) != count:
            cur = None
            if boxes:
                cur = dict(frame_id=[], boxes=[[] for _ in boxes])
                segments.append(cur)
            count = len(boxes)
        if cur is not None:
            cur['frame_id'].append(t)
            for person, b in zip(cur['boxes'], boxes):
                person.append(b)
    return segments


def head_arrows(head_boxes, gaze):
    """Cell 5 of the demo: the arrow it draws per head, as end points.  head_boxes [L,4] x1 y1 x2 y2, gaze [L,>=2] (the fused gaze) ->
    int64 [L,2,2]: (cx, cy) = (int(x1 + x2) // 2, int(y1 + y2) // 2) and (int(cx - l * g0), int(cy - l * g1)) with
    l = int(max(y2 - y1, x2 - x1) * 1); the products are taken in double and int() truncates toward zero.
    gaze as a torch tensor (the ``fused`` of a results='device' stream): the same steps in torch, in double, on gaze's device -> an
    int64 tensor there, nothing is copied to the host."""
    if isinstance(gaze, torch.Tensor):
        b = torch.as_tensor(np.asarray(head_boxes, dtype=np.float64) if not isinstance(head_boxes, torch.Tensor) else head_boxes)
        b = b.to(gaze.device, torch.float64).reshape(-1, 4)
        g = gaze.to(torch.float64).reshape(b.shape[0], -1)
        cx, cy = torch.floor(torch.trunc(b[:, 0] + b[:, 2]) / 2), torch.floor(torch.trunc(b[:, 1] + b[:, 3]) / 2)
        l = torch.trunc(torch.maximum(b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]) * 1)
        tip = torch.stack([torch.trunc(cx - l * g[:, 0]), torch.trunc(cy - l * g[:, 1])], dim=1)
        return torch.stack([torch.stack([cx, cy], dim=1), tip], dim=1).to(torch.int64)
    b = np.asarray(head_boxes, dtype=np.float64).reshape(-1, 4)
    g = np.asarray(gaze, dtype=np.float64).reshape(len(b), -1)
    cx, cy = np.floor(np.trunc(b[:, 0] + b[:, 2]) / 2), np.floor(np.trunc(b[:, 1] + b[:, 3]) / 2)
    l = np.trunc(np.maximum(b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]) * 1)
    tip = np.stack([np.trunc(cx - l * g[:, 0]), np.trunc(cy - l * g[:, 1])], axis=1)
    return np.stack([np.stack([cx, cy], axis=1), tip], axis=1).astype(np.int64)


DRAW_FRAMES = 16                                       # frames per drawing call of run_head_video(draw=...)
DETECT_FRAMES = 64                                     # frames per pipeline.detect_heads call of run_head_video(detections=...)
ATTENTION_FRAMES = 64                                  # frames per pipeline.gaze_targets call of run_head_video(attention=...)


def head_boxes_per_frame(boxes, counts):
    """The padded output of pipeline.detect_heads / detect_heads_host -> the ``boxes_per_frame`` lists segment_tracks and run_head_video take:
    boxes [B, max_det, 4] and counts [B], numpy arrays or device tensors -> B lists of [x1, y1, x2, y2], best detection first.  This is the ONE
    read-back of the offline route; a live route feeds ``boxes.view(-1, 4)`` and ``image_of.view(-1)`` to head_crops instead."""
    boxes, counts = np.asarray(_host(boxes), dtype=np.float32), np.asarray(_host(counts)).reshape(-1)
    if boxes.ndim != 3 or boxes.shape[2] != 4 or len(counts) != len(boxes) or (len(counts) and (counts.min() < 0 or counts.max() > boxes.shape[1])):
        raise ValueError(f'head_boxes_per_frame: boxes [B, max_det, 4] and counts [B] in 0 .. max_det, got {boxes.shape} and {counts.shape}')
    return [boxes[b, :int(n)].tolist() for b, n in enumerate(counts)]


def tracks_from_slots(slot_boxes, track_id, image_of):
    """The slot tables of a whole video as pipeline.track_heads / track_heads_host give them -- slot_boxes [T, S, 4], track_id [T, S] and
    image_of [T, S], numpy arrays or device tensors (chunks of frames concatenated; device tensors come back in ONE copy) -> the tracks in
    segment_tracks' format, one person each: dict(id=track id, frame_id=[t, ...], boxes=[[[x1, y1, x2, y2], ...]]) in ascending id order.
    frame_id holds the frames the track was matched (or born) in, image_of >= 0; a frame it coasted through is left out."""
    if isinstance(slot_boxes, torch.Tensor) and slot_boxes.is_cuda and slot_boxes.ndim == 3 and slot_boxes.dtype == torch.float32:
        dev = slot_boxes.device
        words = torch.cat([slot_boxes.contiguous().view(torch.int32), track_id.to(dev, torch.int32)[..., None], image_of.to(dev, torch.int32)[..., None]],
                          dim=2).cpu().numpy()
        slot_boxes, track_id, image_of = np.ascontiguousarray(words[..., :4]).view(np.float32), words[..., 4], words[..., 5]
    slot_boxes, track_id, image_of = np.asarray(_host(slot_boxes), dtype=np.float32), np.asarray(_host(track_id)), np.asarray(_host(image_of))
    if slot_boxes.ndim != 3 or slot_boxes.shape[2] != 4 or track_id.shape != slot_boxes.shape[:2] or image_of.shape != slot_boxes.shape[:2]:
        raise ValueError(f'tracks_from_slots: slot_boxes [T, S, 4], track_id [T, S] and image_of [T, S], got {slot_boxes.shape}, {track_id.shape} '
                         f'and {image_of.shape}')
    tracks = {}
    for t, s in zip(*np.nonzero(image_of >= 0)):                  # row-major: frames in order
        k = int(track_id[t, s])
        tr = tracks.setdefault(k, dict(id=k, frame_id=[], boxes=[[]]))
        tr['frame_id'].append(int(t))
        tr['boxes'][0].append(slot_boxes[t, s].tolist())
    return [tracks[k] for k in sorted(tracks)]


class _HeadTracker:
    """run_head_video(track=...): pipeline.track_heads over a video, DETECT_FRAMES frames at most per call, the state carried from call to call
    and every table left on the device until ``tracks``."""

    def __init__(self, pipeline, track, device):
        self.options = {} if track is True else dict(track)
        if track is False or set(self.options) - {'slots', 'match_iou', 'max_age', 'motion'}:
            raise ValueError(f'run_head_video: track is None, True or a dict of slots, match_iou, max_age and motion, got {track!r}')
        self.slots = _track_params(**{k: v for k, v in self.options.items() if k != 'motion'})[0]
        _track_motion(self.options.get('motion'), 'run_head_video(track=...)')
        self.pipeline, self.device, self.state, self.parts, self.frames = pipeline, device, None, [], 0

    def feed(self, boxes, counts):
        """The next frames: boxes [T, D, 4] and counts [T], on the host or the device."""
        got = self.pipeline.track_heads(boxes, counts, state=self.state, device=self.device, **self.options)
        self.state = got[6]
        self.parts.append((got[0], got[2], got[1], got[5]))
        self.frames += int(counts.shape[0])

    def feed_lists(self, boxes_per_frame):
        width = max([1] + [len(b) for b in boxes_per_frame])
        table, counts = np.zeros((len(boxes_per_frame), width, 4), np.float32), np.asarray([len(b) for b in boxes_per_frame], dtype=np.int32)
        for t, b in enumerate(boxes_per_frame):
            table[t, :len(b)] = np.asarray(b, dtype=np.float32).reshape(-1, 4)
        for t0 in range(0, len(table), DETECT_FRAMES):
            self.feed(table[t0:t0 + DETECT_FRAMES], counts[t0:t0 + DETECT_FRAMES])

    def tracks(self):
        if not self.parts:
            return []
        slot_boxes, track_id, image_of, flags = (torch.cat([p[k] for p in self.parts]) for k in range(4))
        full = np.flatnonzero(_host(flags) & 1)
        if len(full):
            raise ValueError(f'run_head_video(track=...): frame {int(full[0])} shows more heads than the tracker has free slots (slots={self.slots}); '
                             'give track=dict(slots=...) more')
        return tracks_from_slots(slot_boxes, track_id, image_of)


LETTERBOX_OPTIONS = ('new_shape', 'stride', 'auto', 'scaleup', 'dtype')      # of run_head_video(detections=dict(detector=...)): pipeline.letterbox's


def _detector_groups(pipeline, frames, detector, letterbox, source):
    """The head detector run over a video: yields (raw prediction, in_shape, [(h, w) per frame]) per group of up to DETECT_FRAMES consecutive frames
    that share one letterboxed shape -- pipeline.letterbox (options ``letterbox``; ``source``: rgb, pixel_format, matrix, device), then
    ``detector(img)``, which returns the [B, N, 5 + nc] prediction or a tuple / list that starts with it."""
    geometry = {k: v for k, v in letterbox.items() if k != 'dtype'}

    def run(group, hw):
        img, _ = pipeline.letterbox(group, **letterbox, **source)
        pred = detector(img)
        return pred[0] if isinstance(pred, (tuple, list)) else pred, tuple(img.shape[2:]), hw

    group, hw, shape = [], [], None
    for t in range(len(frames)):
        f = frames[t]                                             # fetched (decoded) once for the detector
        size = _frame_hw(f, source['pixel_format'])
        g = letterbox_geometry(*size, **geometry)
        if group and ((g.out_h, g.out_w) != shape or len(group) == DETECT_FRAMES):
            yield run(group, hw)
            group, hw = [], []
        group.append(f)
        hw.append(size)
        shape = (g.out_h, g.out_w)
    if group:
        yield run(group, hw)


def _frame_hw(frame, pixel_format):
    """(h, w) of one frame as run_head_video takes it."""
    if pixel_format == 'nv12':
        y = frame[0] if isinstance(frame, (tuple, list)) else frame
        return (int(y.shape[0]), int(y.shape[1])) if isinstance(frame, (tuple, list)) else (int(y.shape[0]) // 3 * 2, int(y.shape[1]))
    return int(frame.shape[0]), int(frame.shape[1])


def _add_targets(records, pipeline, device, num_frames, gaze_key, regions, region_image, options):
    """run_head_video(attention=...): the gaze targets of every record and frame, ATTENTION_FRAMES frames per pipeline.gaze_targets call (host
    tables up through the staging ring, the result tables read back), written into the records."""
    rows = [[] for _ in range(num_frames)]                        # frame -> (record, index in it) of its heads, in record order
    options = dict(options)
    three_d = options.pop('three_d', None)
    for r, rec in enumerate(records):
        L_ = len(rec['frame_id'])
        rec.update(target_kind=np.zeros(L_, np.int32), target_id=[None] * L_, target_region=np.full(L_, -1, np.int32),
                   target_hit=np.zeros((L_, 2), np.float32), mutual=np.zeros(L_, np.int32))
        if three_d is not None:
            rec['target_hit3d'] = np.zeros((L_, 3), np.float32)
        for j, t in enumerate(rec['frame_id']):
            rows[t].append((r, j))
    for t0 in range(0, num_frames, ATTENTION_FRAMES):
        part = [(k, r, j) for k, heads in enumerate(rows[t0:t0 + ATTENTION_FRAMES]) for r, j in heads]
        if not part:
            continue
        boxes = np.asarray([records[r]['head_box'][j] for _, r, j in part], dtype=np.float32).reshape(-1, 4)
        gaze = np.asarray([records[r][gaze_key][j, :3] for _, r, j in part], dtype=np.float32).reshape(-1, 3)
        image_of = np.asarray([k for k, _, _ in part], dtype=np.int32)
        if three_d is None:
            got = pipeline.gaze_targets(boxes, gaze, image_of, regions=regions, region_image=region_image, device=device, **options)
        else:                                                     # camera=: one camera for every frame (cam_period 1), decided in camera space
            got = pipeline.gaze_targets_3d(boxes, gaze, image_of, three_d['cam'], regions=three_d['regions'], region_image=three_d['region_image'],
                                           cam_period=1, head_size=three_d['head_size'], frame=three_d['frame'], device=device, **options)
        kind, target, _, hit, mutual, _ = (np.asarray(_host(g)) for g in got[:6])
        for i, (_, r, j) in enumerate(part):
            rec, k = records[r], int(kind[i])
            rec['target_kind'][j], rec['mutual'][j], rec['target_hit'][j] = k, mutual[i], hit[i]
            if three_d is not None:
                rec['target_hit3d'][j] = np.asarray(_host(got[6]))[i]
            if k == 1:
                rec['target_id'][j] = records[part[int(target[i])][1]]['id']
            elif k == 2:
                rec['target_region'][j] = target[i]


def _dwell_episodes(events, state, columns, id_of):
    """The episodes of every column, in the order they began: the rows of an event table [n, 10] (attention.EVENT_FIELDS, ascending frames),
    then the one still open in the column's state [columns, 16], with reason END_VIDEO_ENDED.  id_of(ident): the ``id`` of the record a
    head's ident names.  -> ``columns`` lists of dict(kind, target_id | target_region, start, frames, mutual_frames, reason)."""
    out = [[] for _ in range(columns)]

    def episode(kind, ident, start, frames, mutual, reason):
        target = dict(target_id=id_of(int(ident))) if kind == KIND_HEAD else dict(target_region=int(ident)) if kind == KIND_REGION else {}
        return dict(kind=int(kind), **target, start=int(start), frames=int(frames), mutual_frames=int(mutual), reason=int(reason))

    for row in np.asarray(events).reshape(-1, 10):
        out[int(row[1])].append(episode(*row[4:10]))
    cols, rows = open_episodes(state)
    for c, row in zip(cols, rows):
        out[int(c)].append(episode(*row[2:7], END_VIDEO_ENDED))
    return out


def _dwell_tables(records, num_frames):
    """run_head_video(dwell=...): the [T, R] tables of pipeline.gaze_dwell from records that hold their targets -- a column per record, whose
    person is its index + 1 in the frames it has; a head's ident is the looked-at record's index + 1, a region's its index."""
    R = len(records)
    person, kind, ident, mutual = (np.zeros((num_frames, R), np.int32) for _ in range(4))
    index = {rec['id']: r for r, rec in enumerate(records)}
    for r, rec in enumerate(records):
        t = np.asarray(rec['frame_id'], dtype=np.int64)
        person[t, r], kind[t, r], mutual[t, r] = r + 1, rec['target_kind'], rec['mutual']
        ident[t, r] = [index[tid] + 1 if k == KIND_HEAD else reg for k, tid, reg in zip(rec['target_kind'], rec['target_id'], rec['target_region'])]
    return person, kind, ident, mutual


def _add_dwell(records, pipeline, device, num_frames, options):
    """run_head_video(dwell=...): how long every record looks at what, MAX_ROWS // R frames at most per pipeline.gaze_dwell call with the
    state carried from call to call (host tables up through the staging ring, dwell and the ended episodes read back), written into the
    records; the episodes still open at the last frame are taken from the state, with reason END_VIDEO_ENDED."""
    R = len(records)
    if R > MAX_COLUMNS:
        raise ValueError(f'run_head_video(dwell=...): at most {MAX_COLUMNS} records (got {R})')
    for rec in records:
        rec.update(dwell_kind=np.zeros(len(rec['frame_id']), np.int32), dwell_frames=np.zeros(len(rec['frame_id']), np.int32), episodes=[])
    if R == 0 or num_frames == 0:
        return
    tables = _dwell_tables(records, num_frames)
    state, events, dwell = None, [], []
    for t0 in range(0, num_frames, MAX_ROWS // R):
        got = pipeline.gaze_dwell(*(t[t0:t0 + MAX_ROWS // R] for t in tables), state=state, frame0=t0, device=device, **options)
        state = got[4]
        dwell.append(_host(got[0]))
        events.append(_host(got[2])[:int(_host(got[3])[0])])
    dwell = np.concatenate(dwell)
    episodes = _dwell_episodes(np.concatenate(events), _host(state), R, lambda ident: records[ident - 1]['id'])
    for r, rec in enumerate(records):
        t = np.asarray(rec['frame_id'], dtype=np.int64)
        rec['dwell_kind'], rec['dwell_frames'], rec['episodes'] = dwell[t, r, 0], dwell[t, r, 3], episodes[r]


def _add_heat(records, pipeline, device, num_frames, frame_hw, options):
    """run_head_video(heat=...): the hit points of records that hold their targets into one camera's grid, a pipeline.gaze_heat call per frame
    (the grid decays once per frame) -> the HeatState on the device."""
    state = pipeline.heat_state(1, frame_hw, cell=options['cell'], device=device)
    rows = [[] for _ in range(num_frames)]
    for r in records:
        for j, t in enumerate(r['frame_id']):
            rows[t].append((r['target_hit'][j], r['target_kind'][j]))
    for heads in rows:
        pipeline.gaze_heat(np.asarray([h[0] for h in heads], np.float32).reshape(-1, 2), np.asarray([h[1] for h in heads], np.int32),
                           np.zeros(len(heads), np.int32), state, radius=options['radius'], kinds=options['kinds'], decay=options['decay'], device=device)
    return state


def _add_surface_heat(records, pipeline, device, num_frames, three_d, options):
    """run_head_video(surface_heat=...): the 3-D hit points of records that hold their targets into the grids of regions3d, a
    pipeline.surface_heat call per frame (the grids decay once per frame) -> the SurfaceHeatState on the device."""
    state = pipeline.surface_heat_state(len(three_d['region_image']), grid=options['grid'], device=device)
    regions = type(three_d['regions'])(*(torch.from_numpy(t).to(device) for t in three_d['regions']))      # up once, read where they are by every call
    rows = [[] for _ in range(num_frames)]
    for r in records:
        for j, t in enumerate(r['frame_id']):
            rows[t].append((r['target_hit3d'][j], r['target_kind'][j], r['target_region'][j]))
    for heads in rows:
        pipeline.surface_heat(np.asarray([h[0] for h in heads], np.float32).reshape(-1, 3), np.asarray([h[1] for h in heads], np.int32),
                              np.asarray([h[2] for h in heads], np.int32), regions, state, radius=options['radius'], decay=options['decay'],
                              device=device)
    return state


def run_head_video(engine, pipeline, frames, boxes_per_frame=None, max_len=100, batch_frames=448, expand=0.8, rgb=False, smooth=None, pixel_format='bgr',
                   matrix='bt601', detections=None, track=None, attention=None, dwell=None, heat=None, anonymize=None, surface_heat=None, draw=None):
    """Steps 3-4 of the demo from what its users hold -- the video's frames and one head box per person per frame -- to per-person gaze:
    segment_tracks (cell 1), the head windows cut, resized and normalised on the device (pipeline.head_crops: cell 4's crop arithmetic and
    ``cfg.data.test.pipeline[1:]``), run_tracks (cell 4's loop, batched), head_arrows (cell 5's end points).

    frames: sequence of HxWx3 uint8 frames, numpy arrays (cv2's BGR; rgb=True: RGB) or tensors on the engine's device, indexed by frame
    number; boxes_per_frame[t]: the head boxes of frame t.  pipeline: a DevicePipeline of the L2CS config's test pipeline.
    pixel_format='nv12': frames[t] is a decoder's NV12 surface instead -- a (y, uv) pair or one [3H/2, W] array, on the host or the device -- read
    as it is, with the YUV -> RGB coefficients ``matrix`` names (pipeline.head_crops; rgb is ignored).
    The work goes in groups of about batch_frames crops -- whole chunks (plan_track_chunks), the people of a segment side by side, so that
    a frame showing P heads is uploaded once per group and a long video never has all its crops resident: a chunk is one clip whichever
    group it lands in, so the records do not depend on the grouping.  rescale=True as in the demo: every frame's boxes are divided by ITS
    scale_factor, on the device; they are in pixels of the head window (``crop`` places it in the frame).
    -> one dict per (segment, person), in that order: run_tracks' record (id = (segment, person), det, fused, others) plus frame_id [L],
    head_box [L,4] f32 (as the device read it), crop [L,4] = y0, x0, h, w of the window, arrow int [L,2,2].
    smooth: None, or the alpha in (0, 1] of the temporal filter (tools/calculate_mae_gaze360.py:16-29): every record gains ``fused_smooth``
    [L,3], the fused gaze filtered over the person's whole track (smooth_host: the track is on the host by then), and ``arrow`` is drawn
    from it instead of from ``fused``.
    draw: None (the return value above, untouched), True, or a dict of pipeline.draw_arrows' options (color, length, min_thickness,
    thickness_ratio, tip_length, copy): cell 5's arrows are drawn on the device once the records exist, DRAW_FRAMES frames per call, from the
    gaze ``arrow`` comes from (``fused``, or ``fused_smooth`` with smooth=) -- the drawn shaft ends are ``arrow`` -- and the return value is
    (records, annotated): annotated[t] is frame t on the device in draw_arrows' form, for every t of boxes_per_frame, a frame without a head
    unchanged.  Device frames are drawn into clones (copy=False in the dict: in place).  ``color`` is B, G, R whatever rgb= says.  In a
    frame the people of a segment are drawn left to right: where two arrows overlap, the person further right wins.
    ``overlay=True`` or ``dict(palette=, line_thickness=, region_thickness=)`` in the dict (it needs attention=; ValueError without, and with
    color): the frames are drawn with pipeline.draw_attention from the records' target tables -- region outlines, sight lines, arrows
    coloured by their target -- instead of draw_arrows.
    ``labels=True`` or ``dict(scale=, advance=, pad=, background=, fps=(num, den))`` in the dict: every head gets '#<id>' above its box --
    the record's id (its number where no tracker gave one), with dwell= followed by the seconds of its per-frame dwell_frames at fps --
    through pipeline.draw_labels, after the arrows, in their colour.
    detections: in place of boxes_per_frame (exactly one of the two is given) a dict(pred=..., in_shape=..., **options): the head detector's
    raw prediction [T, N, 5 + nc] for the T frames, on the host or the device, the (h, w) of its letterboxed input, and options of
    pipeline.detect_heads (conf_thres, iou_thres, only_class, agnostic, max_nms, max_det).  The boxes come from DETECT_FRAMES frames per
    call of pipeline.detect_heads and one read-back (head_boxes_per_frame); the records are those of the same boxes given as lists.
    A second form runs the detector too: dict(detector=callable, new_shape=640, stride=32, dtype=torch.float16, auto=True, scaleup=True,
    **options).  Per group of DETECT_FRAMES frames -- a group ends early where the letterboxed shape changes -- pipeline.letterbox makes the
    detector's input from the frames (rgb, pixel_format and matrix as above), ``callable(img)`` returns the raw [B, N, 5 + nc] prediction
    on the device (or a tuple / list whose first item it is), and pipeline.detect_heads reads it with in_shape = img.shape[2:].  pred or
    in_shape together with detector is a ValueError.
    track: None (everything above), True, or a dict of pipeline.track_heads' options (slots, match_iou, max_age, motion): identities come from the
    tracker on the device (mcg_track_heads) instead of segment_tracks -- a person keeps ONE track while others enter, leave or cross, and
    through up to max_age missed detections (motion=True or dict(gain=, decay=): looked for where their velocity takes them, the
    constant-velocity model of mcg_track_heads_motion).  The tracker runs per DETECT_FRAMES frames with its state carried along: with detections= it
    reads detect_heads' outputs where they are, and what is read back are the slot tables (tracks_from_slots) and the flags; boxes_per_frame
    is padded to the largest count and uploaded.  -> one record per track in ascending id order, id = the track's id, frame_id = the frames
    it was matched in (a frame it coasted through is left out); everything downstream is as above, and in a frame the tracks are drawn in
    ascending id.  ValueError, naming the frame and ``slots``, where a frame shows more heads than there are free slots.
    attention: None (everything above), True, or dict(regions=[[x1, y1, x2, y2], ...], expand=0.25, camera_angle=10.0): what every person looks
    at in every frame (pipeline.gaze_targets, mcg_gaze_targets), worked out once the records exist, ATTENTION_FRAMES frames per call, from
    the boxes and the gaze ``arrow`` comes from.  Every record gains, per frame: target_kind int32 [L] (attention.KIND_NONE / KIND_HEAD /
    KIND_REGION / KIND_CAMERA), target_id (a list: the ``id`` of the record of the person looked at, else None), target_region int32 [L] (the
    index into regions, else -1), target_hit f32 [L,2] (where the ray from the head's centre enters the target, in frame pixels) and mutual
    int32 [L] (the two look at each other).  The regions apply to every frame.  regions may be the mixed list of attention.region_polygons:
    an item is a rectangle [x1, y1, x2, y2] or a polygon [[x, y], ...] of 3 .. 32 vertices (mcg_gaze_targets_poly); target_region indexes
    that list.  Decided in the image plane; expand and camera_angle are conventions, not tuned on data.
    dwell: None (everything above), True, or dict(enter=3, exit=2); it needs ``attention`` (ValueError without): how LONG every person looks at
    what (pipeline.gaze_dwell, mcg_gaze_dwell; include/mcgaze_hip.h, "gaze dwell").  The columns are the records; the frames go in chunks of
    at most 65536 // records with the state carried between them.  Every record gains, per frame, dwell_kind and dwell_frames int32 [L] (the
    current target after that frame and its frames so far: a look becomes current after ``enter`` consecutive frames and ends after
    ``exit`` consecutive frames without it -- conventions, not tuned on data) and ``episodes``: a list of dict(kind, target_id (a head: the
    ``id`` of that person's record) or target_region, start, frames, mutual_frames, reason (attention.END_LOOKED_AWAY / END_OWNER_LEFT /
    END_REPLACED; END_VIDEO_ENDED for the episode still open at the last frame, which is appended from the state on the host)), in the order
    they began.
    heat: None (everything above), True, or dict(cell=8, radius=2, decay=0, kinds=('head', 'region'), draw=True, full_scale=None, min_level=1);
    it needs ``attention`` (ValueError without), and with draw=True it needs ``draw``: WHERE in the picture the looks landed
    (pipeline.gaze_heat, mcg_gaze_heat_add; include/mcgaze_hip.h, "gaze heat map"), one call per frame over the records' target_hit, so the
    grid decays once per frame; one camera, cells of ``cell`` pixels over the size of frame 0.  The return value gains, as its LAST item, the
    final grid as a numpy array int32 [1, GH, GW] -- (records, heat), or (records, annotated, heat) with draw --, and with draw=True in the
    dict that final grid is blended into every annotated frame first (pipeline.draw_heat), under the arrows, the overlay and the labels.
    anonymize: None (everything above), True, or a dict of pipeline.anonymize_heads' options (expand, shape, cell, blocks, mode, color); it
    needs ``draw`` (ValueError without): the faces under the records' head boxes are removed from the annotated frames
    (include/mcgaze_hip.h, "anonymised heads"), FIRST in every drawing batch -- before the heat map, the arrows, the overlay and the labels
    -- and on the copies: the crops were cut from the untouched frames, so ``frames`` and the records are exactly those of a run without
    it.  It hides the heads the records hold: a head the detector missed stays visible.
    surface_heat: None (everything above), True, or dict(grid=(32, 32), radius=1, decay=0, draw=True, full_scale=None, min_level=1); it
    needs attention=dict(camera=..., regions3d=...) (ValueError without), and with draw=True it needs ``draw``: WHERE ON each planar region
    the looks landed, as a grid of GW x GH cells in the region's own coordinates (pipeline.surface_heat, mcg_surface_heat_add;
    include/mcgaze_hip.h, "surface heat map"), one call per frame over the records' target_hit3d.  The final grids, a numpy array int32
    [M, GH, GW], are appended after everything returned above, and with draw=True in the dict they are drawn back onto their regions in
    every annotated frame with the right perspective (pipeline.draw_surface_heat), after the image-plane heat map and under the arrows,
    the overlay and the labels.  The grid and the radius are conventions, not tuned on data."""
    smooth = check_smooth('run_head_video', smooth)
    attention = _attention_options('run_head_video', attention)
    dwell = _dwell_options('run_head_video', dwell, attention)
    heat = _heat_options('run_head_video', heat, attention, draw is not None)
    surface = _surface_options('run_head_video', surface_heat, attention, draw is not None)
    if anonymize is not None and draw is None:
        raise ValueError('run_head_video: anonymize changes the annotated frames; it needs draw')
    if anonymize is not None:
        anonymize = {} if anonymize is True else dict(anonymize)
        if set(anonymize) - {'expand', 'shape', 'cell', 'blocks', 'mode', 'color'}:
            raise ValueError(f"run_head_video(anonymize=...): True or a dict of expand, shape, cell, blocks, mode, color; got {sorted(anonymize)}")
        _anon_params('run_head_video(anonymize=...)', **{k: v for k, v in anonymize.items() if k != 'color'})
        if rgb and pixel_format == 'bgr' and anonymize.get('color') is not None:      # the frames hold R, G, B: the colour goes in in their order
            anonymize['color'] = np.asarray(anonymize['color'])[..., ::-1]
    if (boxes_per_frame is None) == (detections is None):
        raise ValueError('run_head_video: give exactly one of boxes_per_frame and detections')
    tracker = None if track is None else _HeadTracker(pipeline, track, engine.device)
    if detections is not None:
        opts = dict(detections)
        if 'detector' in opts:
            if 'pred' in opts or 'in_shape' in opts:
                raise ValueError('run_head_video(detections=...): either pred and in_shape, or a detector that makes them')
            groups = _detector_groups(pipeline, frames, opts.pop('detector'), {k: opts.pop(k) for k in LETTERBOX_OPTIONS if k in opts},
                                      dict(rgb=rgb, pixel_format=pixel_format, matrix=matrix, device=engine.device))
        else:
            if 'pred' not in opts or 'in_shape' not in opts:
                raise ValueError('run_head_video(detections=...): a dict with pred and in_shape, or with detector')
            pred, in_shape = opts.pop('pred'), opts.pop('in_shape')
            groups = ((pred[t0:t0 + DETECT_FRAMES], in_shape, [_frame_hw(frames[t], pixel_format) for t in range(t0, min(t0 + DETECT_FRAMES, len(pred)))])
                      for t0 in range(0, len(pred), DETECT_FRAMES))
        boxes_per_frame = []
        for part, in_shape, hw in groups:
            got = pipeline.detect_heads(part, in_shape, np.asarray(hw, dtype=np.int32).reshape(-1, 2), device=engine.device, **opts)
            if tracker is None:
                boxes_per_frame += head_boxes_per_frame(got[0], got[4])
            else:
                tracker.feed(got[0], got[4])
    if tracker is None:
        segments = segment_tracks(boxes_per_frame)
    else:
        if detections is None:
            tracker.feed_lists(boxes_per_frame)
        segments, boxes_per_frame = tracker.tracks(), range(tracker.frames)
    chunks = [(si, a, b, pi) for si, seg in enumerate(segments) for a, b in plan_track_chunks(len(seg['frame_id']), max_len)
              for pi in range(len(seg['boxes']))]
    pieces = {}                                        # (segment, person) -> list of (record, crop) in chunk order

    def flush(group):
        slot, images, boxes, image_of = {}, [], [], []
        for si, a, b, pi in group:
            for j in range(a, b):
                t = segments[si]['frame_id'][j]
                if t not in slot:
                    slot[t] = len(images)
                    images.append(frames[t])
                image_of.append(slot[t])
                boxes.append(segments[si]['boxes'][pi][j])
        img, img_hw, scale, crop, _ = pipeline.head_crops(images, np.asarray(boxes, dtype=np.float32).reshape(-1, 4), np.asarray(image_of, dtype=np.int32),
                                                          expand=expand, device=engine.device, rgb=rgb, pixel_format=pixel_format, matrix=matrix)
        rows = np.concatenate([[0], np.cumsum([b - a for _, a, b, _ in group])])
        tracks = [dict(id=k, frames=img[r0:r1], img_hw=img_hw[r0:r1], scale_factor=scale[r0:r1]) for k, (r0, r1) in enumerate(zip(rows[:-1], rows[1:]))]
        records = run_tracks(engine, tracks, max_len=max_len, batch_frames=batch_frames)
        crop = _host(crop)
        for (si, a, b, pi), rec, r0, r1 in zip(group, records, rows[:-1], rows[1:]):
            pieces.setdefault((si, pi), []).append((rec, crop[r0:r1]))

    group, held = [], 0
    for c in chunks:
        if held and held + (c[2] - c[1]) > batch_frames:
            flush(group)
            group, held = [], 0
        group.append(c)
        held += c[2] - c[1]
    if group:
        flush(group)
    out = []
    for si, seg in enumerate(segments):
        for pi, person in enumerate(seg['boxes']):
            got = pieces[(si, pi)]
            rec = {k: np.concatenate([r[k] for r, _ in got]) for k in ('det', 'fused', 'others')}
            head_box = np.asarray(person, dtype=np.float32).reshape(-1, 4)
            if smooth is not None:
                rec['fused_smooth'] = smooth_host(rec['fused'], smooth)
            out.append(dict(id=(si, pi) if tracker is None else seg['id'], **rec, frame_id=list(seg['frame_id']), head_box=head_box, crop=np.concatenate([c for _, c in got]),
                            arrow=head_arrows(person, rec['fused' if smooth is None else 'fused_smooth'])))
    if attention is not None:
        _add_targets(out, pipeline, engine.device, len(boxes_per_frame), 'fused' if smooth is None else 'fused_smooth', *attention)
    if dwell is not None:
        _add_dwell(out, pipeline, engine.device, len(boxes_per_frame), dwell)
    heat_state = None if heat is None else _add_heat(out, pipeline, engine.device, len(boxes_per_frame), _frame_hw(frames[0], pixel_format), heat)
    three_d = None if surface is None else attention[2]['three_d']
    surface_state = None if surface is None else _add_surface_heat(out, pipeline, engine.device, len(boxes_per_frame), three_d, surface)
    last = () if surface is None else (_host(surface_state.heat),)      # appended after everything returned without the option
    if draw is None:
        got = out if heat is None else (out, _host(heat_state.heat))
        return got if surface is None else ((got,) if heat is None else got) + last
    opts = {'copy': True, **({} if draw is True else dict(draw))}
    overlay = _overlay_options('run_head_video(draw=...)', opts.pop('overlay', None), True, attention)
    labels = _label_options('run_head_video(draw=...)', opts.pop('labels', None), True)
    if labels is not None and labels.pop('region_names') is not None:
        raise ValueError('run_head_video(draw=...): labels takes no region_names here; draw them with attention.region_label_rows and draw_labels')
    if overlay is not None and opts.get('color') is not None:
        raise ValueError('run_head_video(draw=...): with overlay the colours are the palette\'s, not color')
    if overlay is not None and rgb and pixel_format == 'bgr':
        overlay['palette'] = np.asarray(OVERLAY_PALETTE if overlay.get('palette') is None else overlay['palette'])[..., ::-1]
    elif rgb and pixel_format == 'bgr':                # the frames hold R, G, B: the colour goes in in their order
        opts['color'] = np.asarray(ARROW_COLOR if opts.get('color') is None else opts['color'])[..., ::-1]
    rows = [[] for _ in boxes_per_frame]               # frame -> (box, gaze) of its heads, in record order
    named = [[] for _ in boxes_per_frame]              # frame -> (id, dwell_frames) of its heads, for labels
    for number, r in enumerate(out):
        g = r['fused' if smooth is None else 'fused_smooth']
        ident = r['id'] if isinstance(r['id'], (int, np.integer)) else number + 1      # (without a tracker a record's id is a pair: its number)
        for j, t in enumerate(r['frame_id']):
            rows[t].append((r['head_box'][j], g[j, :2]) + (() if overlay is None else (r['target_kind'][j], r['target_region'][j], r['target_hit'][j], r['mutual'][j])))
            named[t].append((int(ident), int(r['dwell_frames'][j]) if dwell is not None else 0))
    if opts.get('color') is not None and np.ndim(opts['color']) == 2:
        raise ValueError('run_head_video(draw=...): color is one (B, G, R) triple')
    annotated, drawing = [], opts                     # drawing: the caller's options, copy among them, the same for every batch
    for t0 in range(0, len(rows), DRAW_FRAMES):
        part = rows[t0:t0 + DRAW_FRAMES]
        image_of = np.asarray([k for k, heads in enumerate(part) for _ in heads], dtype=np.int32)
        boxes = np.asarray([h[0] for heads in part for h in heads], dtype=np.float32).reshape(-1, 4)
        gaze = np.asarray([h[1] for heads in part for h in heads], dtype=np.float32).reshape(-1, 2)
        images = [frames[t] for t in range(t0, t0 + len(part))]
        opts, copy = drawing, drawing['copy']
        if anonymize is not None:                      # first of all: the faces go before anything is drawn over them; what follows draws into THESE frames, in place
            images, _ = pipeline.anonymize_heads(images, boxes, image_of, pixel_format=pixel_format, matrix=matrix, copy=copy, device=engine.device,
                                                 **anonymize)
            opts, copy = dict(drawing, copy=False), False
        if heat is not None and heat['draw']:          # first, under everything else (period 1: every picture shows the one camera); what follows draws into THESE frames, in place
            images = pipeline.draw_heat(images, heat_state, period=1, full_scale=heat['full_scale'], min_level=heat['min_level'], pixel_format=pixel_format,
                                        matrix=matrix, copy=copy, device=engine.device)
            opts = dict(drawing, copy=False)
        if surface is not None and surface['draw']:   # after the image-plane map, under everything else (one camera: cam_period 1, the regions on every picture)
            images = pipeline.draw_surface_heat(images, surface_state, three_d['cam'], three_d['regions'], three_d['region_image'], cam_period=1,
                                                full_scale=surface['full_scale'], min_level=surface['min_level'], pixel_format=pixel_format, matrix=matrix,
                                                copy=copy if opts is drawing else False, device=engine.device)
            opts = dict(drawing, copy=False)
        if overlay is None:
            imgs, _ = pipeline.draw_arrows(images, boxes, gaze, image_of, pixel_format=pixel_format, matrix=matrix, device=engine.device, **opts)
        else:                                          # the records' own tables: a head's target is not read by the overlay, a region's is target_region
            kind, target, hit, mutual = ([h[i] for heads in part for h in heads] for i in (2, 3, 4, 5))
            imgs = pipeline.draw_attention(images, boxes, gaze, image_of, np.asarray(kind, np.int32), np.asarray(target, np.int32),
                                           np.asarray(hit, np.float32).reshape(-1, 2), np.asarray(mutual, np.int32), regions=attention[0],
                                           region_image=attention[1], pixel_format=pixel_format, matrix=matrix, device=engine.device, **opts, **overlay)[0]
        if labels is not None and len(boxes):           # into the frames just drawn, in place: the id, with dwell the seconds of dwell_frames
            ids, values = (np.asarray([h[i] for heads in named[t0:t0 + len(part)] for h in heads], dtype=np.int32) for i in (0, 1))
            text = format_labels_host(ids, values if dwell is not None else None, labels['fps'])
            if overlay is None:
                colors = dict(color=opts.get('color'))
            else:
                pal = np.asarray(OVERLAY_PALETTE if overlay.get('palette') is None else overlay['palette'])
                colors = dict(colors=pal[[4 if m else k if 1 <= k <= 3 else 0 for k, m in zip(kind, mutual)]].astype(np.uint8))
            imgs, _ = pipeline.draw_labels(imgs, boxes, image_of, text, pixel_format=pixel_format, matrix=matrix, device=engine.device, **colors,
                                           **{k: v for k, v in labels.items() if k != 'fps'})
        annotated += imgs
    return ((out, annotated) if heat is None else (out, annotated, _host(heat_state.heat))) + last


def dump_results(records, config_path, json_path, out_dir='results'):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, result_file_name(config_path, json_path))
    with open(path, 'w') as f:
        json.dump(records, f)
    return path
