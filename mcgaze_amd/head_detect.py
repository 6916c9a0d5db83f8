"""Around the demo's head detector.  Its input: ``DevicePipeline.letterbox`` (``mcg_letterbox_frames``; csrc/preprocess.hip) turns frames into
the letterboxed tensor the detector reads, ``letterbox_geometry`` is the reference's size rule and ``letterbox_host`` the same pixels in numpy.
Its output: ``DevicePipeline.detect_heads`` (``mcg_detect_heads``: confidence filter, NMS and scale-back; csrc/detect.hip) never leaves the
device; ``detect_heads_host`` is the same in numpy, and the option and shape checks they share.  Behind it: ``DevicePipeline.track_heads``
(``mcg_track_heads``; csrc/track.hip) gives the heads of consecutive frames one identity per person; ``track_heads_host`` is the same in numpy."""
import collections

import numpy as np
import torch

from .nv12 import _nv12_planes, _pixel_format, nv12_to_bgr
from .staging import _bgr_frame, _host_array

DETECT_MAX_DET = 300                                             # the reference's max_det, and the bound of the entry


def _detect_params(conf_thres=0.25, iou_thres=0.45, only_class=1, agnostic=False, max_nms=30000, max_det=300):
    """The options of detect_heads_host / DevicePipeline.detect_heads, checked -> (conf_thres, iou_thres, only_class, agnostic, max_nms, max_det)."""
    conf_thres, iou_thres = float(conf_thres), float(iou_thres)
    if not (np.isfinite(conf_thres) and np.isfinite(iou_thres)):
        raise ValueError(f'detect_heads: conf_thres and iou_thres must be finite, got {conf_thres}, {iou_thres}')
    only_class = -1 if only_class is None else int(only_class)
    if only_class < -1:
        raise ValueError(f'detect_heads: only_class is a class index, or -1 / None for every class, got {only_class}')
    if int(max_det) != max_det or not 1 <= max_det <= DETECT_MAX_DET:
        raise ValueError(f'detect_heads: max_det in 1 .. {DETECT_MAX_DET}, got {max_det}')
    if int(max_nms) != max_nms or max_nms < 1:
        raise ValueError(f'detect_heads: max_nms must be at least 1, got {max_nms}')
    return conf_thres, iou_thres, only_class, bool(agnostic), int(max_nms), int(max_det)


def _detect_shapes(shape, in_shape, frame_hw):
    """-> (B, N, nc, in_h, in_w, frame_hw [B,2] int32 or None for a device tensor, which is checked for its shape only)."""
    if len(shape) != 3 or shape[2] < 6 or shape[1] < 1:
        raise ValueError(f'detect_heads: pred must be [B, N, 5 + nc] with N >= 1 and nc >= 1, got {tuple(shape)}')
    B, N, nc = int(shape[0]), int(shape[1]), int(shape[2]) - 5
    in_h, in_w = (int(v) for v in in_shape)
    if in_h < 1 or in_w < 1:
        raise ValueError(f'detect_heads: in_shape is the detector\'s (h, w) input, got {tuple(in_shape)}')
    if isinstance(frame_hw, torch.Tensor) and frame_hw.is_cuda:
        if tuple(frame_hw.shape) != (B, 2) or frame_hw.dtype not in (torch.int32, torch.int64):
            raise ValueError(f'detect_heads: a device frame_hw is an integer [{B}, 2] tensor, got {frame_hw.dtype} {tuple(frame_hw.shape)}')
        return B, N, nc, in_h, in_w, None
    hw = _host_array(frame_hw)
    if hw.dtype.kind not in 'iu':
        raise TypeError(f'detect_heads: frame_hw must hold integers, got {hw.dtype}')
    if hw.shape == (2,):
        hw = np.broadcast_to(hw, (B, 2))
    if hw.shape != (B, 2):
        raise ValueError(f'detect_heads: frame_hw is one (h, w) or [{B}, 2], got {hw.shape}')
    return B, N, nc, in_h, in_w, np.ascontiguousarray(hw, dtype=np.int32)


def detect_heads_host(pred, in_shape, frame_hw, conf_thres=0.25, iou_thres=0.45, only_class=1, agnostic=False, max_nms=30000, max_det=300):
    """``mcg_detect_heads`` in numpy, bit for bit (the arithmetic: include/mcgaze_hip.h, "head boxes from raw detector output"): the demo's
    head detector's post-processing -- non_max_suppression on a float32 prediction with classes=[only_class] and multi_label=False, then
    scale_coords(...).round() (MCGaze_demo/yolo_head/utils/general.py:291-312, 393-481) -- for checks and for users without a GPU.

    pred [B, N, 5 + nc] (x, y, w, h, objectness, classes; f32, or fp16 which is widened exactly); in_shape: the (h, w) of the detector's
    letterboxed input; frame_hw: one (h, w) or [B, 2], the frames the boxes are scaled back into.  only_class: the head class of the
    demo's detector is 1; -1 or None keeps every class.
    -> (boxes [B, max_det, 4] f32, scores [B, max_det] f32, classes [B, max_det] int32, image_of [B, max_det] int32, counts [B] int32,
    flags [B] int32): row k < counts[b] is a detection of image b (image_of = b), best first; the rows behind are zero with image_of = -1.
    flags: 1 where more than max_nms candidates stood (the best max_nms took part), 2 for a frame without pixels (count 0)."""
    conf_thres, iou_thres, only_class, agnostic, max_nms, max_det = _detect_params(conf_thres, iou_thres, only_class, agnostic, max_nms, max_det)
    pred = _host_array(pred)
    B, N, nc, in_h, in_w, hw = _detect_shapes(pred.shape, in_shape, _host_array(frame_hw))
    if pred.dtype not in (np.float32, np.float16):
        raise TypeError(f'detect_heads: pred must be float32 or float16, got {pred.dtype}')
    pred = pred.astype(np.float32)
    f32 = np.float32
    with np.errstate(all='ignore'):
        thr, it = f32(conf_thres), f32(iou_thres)
    boxes, scores = np.zeros((B, max_det, 4), f32), np.zeros((B, max_det), f32)
    classes, image_of = np.zeros((B, max_det), np.int32), np.full((B, max_det), -1, np.int32)
    counts, flags = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        h0, w0 = int(hw[b, 0]), int(hw[b, 1])
        if h0 <= 0 or w0 <= 0:
            flags[b] = 2
            continue
        p = pred[b]
        with np.errstate(all='ignore'):
            sc = p[:, 5:] * p[:, 4:5]
            conf = sc.max(axis=1)                                # a NaN score makes conf NaN: the row is dropped below
            cls = sc.argmax(axis=1)                              # the lowest class that reaches the maximum
            half_w, half_h = p[:, 2] / f32(2), p[:, 3] / f32(2)
            box = np.stack([p[:, 0] - half_w, p[:, 1] - half_h, p[:, 0] + half_w, p[:, 1] + half_h], axis=1)
            keep = (p[:, 4] > thr) & (conf > thr) & np.isfinite(box).all(axis=1) & np.isfinite(conf)
            if only_class >= 0:
                keep &= cls == only_class
            idx = np.flatnonzero(keep)
            idx = idx[np.argsort(-(conf[idx] + f32(0)), kind='stable')]          # conf descending, ties by the lower anchor
            if len(idx) > max_nms:
                flags[b] = 1
                idx = idx[:max_nms]
            off = box[idx] + (f32(0) if agnostic else cls[idx].astype(f32) * f32(4096))[..., None]
            x1, y1, x2, y2 = off.T
            area = (x2 - x1) * (y2 - y1)
            gone, kept = np.zeros(len(idx), bool), []
            for i in range(len(idx)):
                if gone[i]:
                    continue
                kept.append(i)
                if len(kept) == max_det:
                    break
                r = slice(i + 1, None)
                w = np.maximum(f32(0), np.minimum(x2[i], x2[r]) - np.maximum(x1[i], x1[r]))
                h = np.maximum(f32(0), np.minimum(y2[i], y2[r]) - np.maximum(y1[i], y1[r]))
                inter = w * h
                gone[r] |= inter / (area[i] + area[r] - inter) > it                # NaN suppresses nothing
            rows = idx[kept]
            gain = min(in_h / h0, in_w / w0)
            pad_x, pad_y = (in_w - w0 * gain) / 2, (in_h - h0 * gain) / 2
            g, pad, hi = f32(gain), np.array([pad_x, pad_y, pad_x, pad_y], f32), np.array([w0, h0, w0, h0], f32)
            v = (box[rows] - pad) / g
            v = np.where(v < 0, f32(0), v)
            v = np.where(v > hi, hi, v)
            n = len(rows)
            boxes[b, :n], scores[b, :n], classes[b, :n], image_of[b, :n], counts[b] = np.rint(v), conf[rows], cls[rows], b, n
    return boxes, scores, classes, image_of, counts, flags


# ---------------------------------------------------------------- identities across frames
TRACK_MAX_SLOTS, TRACK_MAX_DET = 64, 1024                        # the bounds of mcg_track_heads
TRACK_HEADER_WORDS, TRACK_SLOT_WORDS = 4, 8                      # mcg_track_header / mcg_track_slot in int32 words: next_id frames_seen - - | box[4] id age vx vy
TRACK_MOTION_DEFAULTS = dict(gain=0.5, decay=1.0)                # conventional alpha-beta values; not tuned on data


def track_state_words(slots):
    """int32 words of one sequence's tracker state (mcg_track_state_bytes(1, slots) / 4): a state is an int32 [Q, words] array, zeros when empty."""
    return TRACK_HEADER_WORDS + TRACK_SLOT_WORDS * int(slots)


def _track_params(slots=16, match_iou=0.3, max_age=5):
    """The options of track_heads_host / DevicePipeline.track_heads, checked -> (slots, match_iou, max_age)."""
    if isinstance(slots, bool) or int(slots) != slots or not 1 <= slots <= TRACK_MAX_SLOTS:
        raise ValueError(f'track_heads: slots in 1 .. {TRACK_MAX_SLOTS}, got {slots!r}')
    match_iou = float(match_iou)
    if not np.isfinite(match_iou):
        raise ValueError(f'track_heads: match_iou must be finite, got {match_iou}')
    if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 0 or max_age > 0x7fffffff:
        raise ValueError(f'track_heads: max_age is a number of frames, 0 or more, got {max_age!r}')
    return int(slots), match_iou, int(max_age)


def _track_motion(motion, who='track_heads'):
    """motion= of track_heads_host / DevicePipeline.track_heads, checked -> None (the plain tracker) or (gain, decay) of mcg_track_heads_motion.
    None, True (gain 0.5, decay 1.0: conventional alpha-beta values, not tuned on data) or a dict of gain and decay, each in [0, 1]."""
    if motion is None:
        return None
    if motion is True:
        motion = {}
    if not isinstance(motion, dict) or set(motion) - set(TRACK_MOTION_DEFAULTS):
        raise ValueError(f'{who}: motion is None, True or a dict of gain and decay, got {motion!r}')
    values = {**TRACK_MOTION_DEFAULTS, **motion}
    for name, v in values.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:   # not for a NaN
            raise ValueError(f'{who}: motion {name} must lie in 0 .. 1, got {v!r}')
    return float(values['gain']), float(values['decay'])


def _track_shapes(boxes_shape, counts_shape, state_shape, slots):
    """boxes [T, D, 4] (one sequence) or [Q, T, D, 4], counts [T] or [Q, T], state None or [Q, words] -> (Q, T, D, whether Q was given)."""
    shape = tuple(int(v) for v in boxes_shape)
    if len(shape) not in (3, 4) or shape[-1] != 4 or shape[-2] < 1 or shape[-2] > TRACK_MAX_DET or shape[-3] < 1:
        raise ValueError(f'track_heads: boxes must be [T, D, 4] or [Q, T, D, 4] with T >= 1 and D in 1 .. {TRACK_MAX_DET}, got {shape}')
    if tuple(int(v) for v in counts_shape) != shape[:-2]:
        raise ValueError(f'track_heads: counts must be {list(shape[:-2])} for boxes {shape}, got {tuple(counts_shape)}')
    Q = shape[0] if len(shape) == 4 else 1
    if Q > 65535:
        raise ValueError(f'track_heads: at most 65535 sequences per call, got {Q}')
    if state_shape is not None and tuple(int(v) for v in state_shape) != (Q, track_state_words(slots)):
        raise ValueError(f'track_heads: the state of {Q} sequences of {slots} slots is an int32 [{Q}, {track_state_words(slots)}] array, got {tuple(state_shape)}')
    return Q, shape[-3], shape[-2], len(shape) == 4


def track_heads_host(boxes, counts, state=None, slots=16, match_iou=0.3, max_age=5, motion=None):
    """``mcg_track_heads`` in numpy, bit for bit (the arithmetic: include/mcgaze_hip.h, "head identities across frames"), for checks and for
    users without a GPU: which head box of frame t is the person of which box of frame t - 1, by greedy IoU matching against the ``slots``
    tracks of a sequence (one camera).

    boxes [T, D, 4] f32 (one sequence) or [Q, T, D, 4], counts [T] or [Q, T] integers: the first counts rows of a frame are its heads, best
    first -- ``detect_heads_host``'s boxes and counts as they come.  state: None for the empty state, or what an earlier call returned (int32
    [Q, track_state_words(slots)]; it is not written to).  A slot matched to a detection with IoU > match_iou keeps its id; an unmatched slot
    coasts for max_age frames with its last box and is then freed; an unmatched detection opens the lowest free slot with the next id (1, 2, ...
    per sequence).  ValueError for bad shapes and options, TypeError for boxes that are not float32 or counts that are not integers.
    -> (slot_boxes [.., T, S, 4] f32, image_of [.., T, S] int32, track_id [.., T, S] int32, age [.., T, S] int32, det_of [.., T, S] int32,
    flags [.., T] int32, state): row s of frame (q, t) is slot s -- for a slot matched or born in the frame the detection's box, image_of =
    q * T + t and det_of = the detection; for every other slot zeros, -1, -1; track_id is the slot's id after the frame (0: free), age the frames
    since its last match (-1: free).  flags: 1 a head was dropped for want of a slot, 2 a row was not finite (never matched or born), 4 a count
    outside 0 .. D.  ``slot_boxes.reshape(-1, 4)`` and ``image_of.reshape(-1)`` are head_crops' tables when its images are the call's frames.

    motion: None is everything above.  True or dict(gain=0.5, decay=1.0) is ``mcg_track_heads_motion`` instead, bit for bit (the header's
    "head identities with a constant-velocity motion model"): a slot carries the velocity of its box's centre in the last two words of its
    record, its box is moved by it before every match, a match corrects the velocity by ``gain`` times the distance between the detection's
    centre and the predicted one, and a coasting slot keeps the PREDICTED box with its velocity times ``decay``.  Both lie in [0, 1]; the
    defaults are conventional alpha-beta values, not tuned on data.  An eighth result follows the state: state_boxes [.., T, S, 4] f32, each
    slot's box after the frame (a coasting slot's predicted box; zeros for a free slot).  gain=0 on a state without velocities gives the
    plain tracker's seven results."""
    slots, match_iou, max_age = _track_params(slots, match_iou, max_age)
    motion = _track_motion(motion)
    boxes, counts = _host_array(boxes), _host_array(counts)
    state = None if state is None else _host_array(state)
    Q, T, D, given_q = _track_shapes(boxes.shape, counts.shape, None if state is None else state.shape, slots)
    if boxes.dtype != np.float32:
        raise TypeError(f'track_heads: boxes must be float32, got {boxes.dtype}')
    if counts.dtype.kind not in 'iu':
        raise TypeError(f'track_heads: counts must hold integers, got {counts.dtype}')
    if state is not None and state.dtype != np.int32:
        raise TypeError(f'track_heads: the state is an int32 array, got {state.dtype}')
    S, f32, zero = slots, np.float32, np.float32(0)
    boxes, counts = boxes.reshape(Q, T, D, 4), counts.reshape(Q, T)
    state = np.zeros((Q, track_state_words(S)), np.int32) if state is None else np.array(state, dtype=np.int32, order='C')
    thr = f32(match_iou)
    gain, decay = (None, None) if motion is None else (f32(motion[0]), f32(motion[1]))
    slot_boxes, state_boxes = np.zeros((Q, T, S, 4), f32), np.zeros((Q, T, S, 4), f32)
    image_of, det_of = np.full((Q, T, S), -1, np.int32), np.full((Q, T, S), -1, np.int32)
    track_id, age_out, flags = np.zeros((Q, T, S), np.int32), np.zeros((Q, T, S), np.int32), np.zeros((Q, T), np.int32)
    for q in range(Q):
        table = state[q, TRACK_HEADER_WORDS:].reshape(S, TRACK_SLOT_WORDS)
        box, ids, age, next_id = table[:, :4].copy().view(f32), table[:, 4].copy(), table[:, 5].copy(), int(state[q, 0])
        vel = table[:, 6:8].copy().view(f32)
        for t in range(T):
            c = int(counts[q, t])
            n = min(max(c, 0), D)
            det = boxes[q, t, :n]
            usable = np.isfinite(det).all(axis=1)
            flag = (0 if usable.all() else 2) | (4 if c != n else 0)
            slot_det, det_open = np.full(S, -1), usable.copy()
            live = ids > 0
            if motion is not None:                                                       # step 0: a slot at rest is not touched
                with np.errstate(all='ignore'):
                    for s in np.flatnonzero(live & ~((vel[:, 0] == 0) & (vel[:, 1] == 0))):
                        p = box[s] + vel[s][[0, 1, 0, 1]]
                        if np.isfinite(p).all():
                            box[s] = p
                        else:
                            vel[s] = 0
            if n and live.any():
                with np.errstate(all='ignore'):
                    a, b = box[:, None, :], det[None, :, :]
                    area_a, area_b = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]), (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
                    dw = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
                    dh = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
                    inter = np.where(dw < 0, zero, dw) * np.where(dh < 0, zero, dh)
                    iou = inter / (area_a + area_b - inter) + zero
                    cand = (iou > thr) & live[:, None] & usable[None, :]                 # a NaN is no candidate; a candidate's iou is >= 0
                while cand.any():
                    held = np.where(cand, iou, f32(-1))
                    s, d = np.argwhere(held == held.max())[0]                            # row-major: the lower slot, then the lower detection
                    slot_det[s], det_open[d] = d, False
                    cand[s, :] = False
                    cand[:, d] = False
            for s in range(S):
                if slot_det[s] >= 0:
                    if motion is not None:
                        with np.errstate(all='ignore'):
                            d = det[slot_det[s]]
                            r = ((d[:2] + d[2:]) - (box[s, :2] + box[s, 2:])) * f32(0.5)
                            v = vel[s] + gain * r                                        # the product is rounded, then the sum
                        vel[s] = v if np.isfinite(v).all() else 0
                    box[s], age[s] = det[slot_det[s]], 0
                elif ids[s] > 0:
                    age[s] += 1
                    if age[s] > max_age:
                        box[s], ids[s], age[s] = 0, 0, 0
                        if motion is not None:
                            vel[s] = 0
                    elif motion is not None:                                             # it keeps the predicted box
                        vel[s] = vel[s] * decay
            free = [s for s in range(S) if ids[s] == 0]
            for d in np.flatnonzero(det_open):
                if not free:
                    flag |= 1
                    break
                s = free.pop(0)
                next_id += 1
                box[s], ids[s], age[s], slot_det[s] = det[d], next_id, 0, d
                if motion is not None:
                    vel[s] = 0
            hit = slot_det >= 0
            slot_boxes[q, t, hit] = det[slot_det[hit]]
            image_of[q, t, hit], det_of[q, t] = q * T + t, slot_det
            track_id[q, t], age_out[q, t], flags[q, t] = ids, np.where(ids != 0, age, -1), flag
            state_boxes[q, t] = np.where((ids > 0)[:, None], box, zero)
        table[:, :4], table[:, 4], table[:, 5] = box.view(np.int32), ids, age
        if motion is not None:
            table[:, 6:8] = vel.view(np.int32)
        state[q, 0], state[q, 1] = next_id, state[q, 1] + T
    out = (slot_boxes, image_of, track_id, age_out, det_of, flags)
    if motion is None:
        return (out if given_q else tuple(o[0] for o in out)) + (state,)
    return (out if given_q else tuple(o[0] for o in out)) + (state, state_boxes if given_q else state_boxes[0])


# ---------------------------------------------------------------- the detector's input
LETTERBOX_PAD = 114                                             # letterbox(color=(114, 114, 114))
LETTERBOX_DTYPES = {torch.uint8: np.uint8, torch.float16: np.float16, torch.float32: np.float32}

LetterboxGeometry = collections.namedtuple('LetterboxGeometry', 'unpad_h unpad_w top bottom left right out_h out_w ratio pad')


def _letterbox_options(new_shape, stride):
    """new_shape (an integer is a square) and stride, checked -> (new_h, new_w, stride)."""
    shape = (new_shape, new_shape) if np.ndim(new_shape) == 0 else tuple(new_shape)
    if len(shape) != 2 or any(int(v) != v or v < 1 for v in shape):
        raise ValueError(f'letterbox: new_shape is a positive integer or (h, w), got {new_shape!r}')
    if int(stride) != stride or stride < 1:
        raise ValueError(f'letterbox: stride must be a positive integer, got {stride!r}')
    return int(shape[0]), int(shape[1]), int(stride)


def letterbox_geometry(h, w, new_shape=640, stride=32, auto=True, scaleup=True):
    """The sizes of letterbox(img, new_shape, color=(114, 114, 114), auto, scaleFill=False, scaleup, stride)
    (MCGaze_demo/yolo_head/utils/datasets.py:810-840) for an h x w frame, line for line in python floats:

        r = min(new_h / h, new_w / w);  scaleup false: r = min(r, 1.0)
        unpad_w, unpad_h = int(round(w * r)), int(round(h * r))
        dw, dh = new_w - unpad_w, new_h - unpad_h;  auto: dw, dh = dw % stride, dh % stride;  dw /= 2;  dh /= 2
        top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1));  left, right = int(round(dw - 0.1)), int(round(dw + 0.1))

    -> LetterboxGeometry(unpad_h, unpad_w, top, bottom, left, right, out_h, out_w, ratio, pad): the resized frame, the border on each side, the
    output (top + unpad_h + bottom, left + unpad_w + right) and the reference's other two return values, ratio = (r, r) and pad = (dw, dh)
    (halved, before rounding).  scaleFill is not offered.  ValueError for sizes that are not positive and for a frame so thin that a
    resized side rounds to zero, which cv2.resize refuses."""
    new_h, new_w, stride = _letterbox_options(new_shape, stride)
    if int(h) != h or int(w) != w or h < 1 or w < 1:
        raise ValueError(f'letterbox: a frame has a positive (h, w), got ({h!r}, {w!r})')
    h, w = int(h), int(w)
    r = min(new_h / h, new_w / w)
    if not scaleup:
        r = min(r, 1.0)
    unpad_w, unpad_h = int(round(w * r)), int(round(h * r))
    if unpad_w < 1 or unpad_h < 1:
        raise ValueError(f'letterbox: a {h} x {w} frame in {new_h} x {new_w} would be resized to {unpad_h} x {unpad_w}')
    dw, dh = new_w - unpad_w, new_h - unpad_h
    if auto:
        dw, dh = dw % stride, dh % stride
    dw, dh = dw / 2, dh / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return LetterboxGeometry(unpad_h, unpad_w, top, bottom, left, right, top + unpad_h + bottom, left + unpad_w + right, (r, r), (dw, dh))


def _letterbox_plan(sizes, new_shape, stride, auto, scaleup):
    """letterbox_geometry of every (h, w) of ``sizes`` -> (geometries, out_h, out_w); ValueError, naming the shapes, unless they share one output."""
    geoms = [letterbox_geometry(h, w, new_shape, stride, auto, scaleup) for h, w in sizes]
    if not geoms:
        raise ValueError('letterbox: no frames')
    outs = [(g.out_h, g.out_w) for g in geoms]
    if len(set(outs)) != 1:
        raise ValueError(f'letterbox: the frames of one call must share one output shape, got {sorted(set(outs))} for frames {[tuple(s) for s in sizes]}')
    return geoms, outs[0][0], outs[0][1]


def _letterbox_dtype(dtype):
    """torch.uint8 / float16 / float32, or the numpy type of the same name -> the torch dtype (TypeError for anything else)."""
    for t, n in LETTERBOX_DTYPES.items():
        if dtype is t or (not isinstance(dtype, torch.dtype) and np.dtype(dtype) == n):
            return t
    raise TypeError(f'letterbox: dtype is uint8, float16 or float32, got {dtype!r}')


def _linear_coef(dst, src):
    """Per destination index of a dst <- src resize: the two source indices and their 11-bit coefficients -- lin_coef of csrc/preprocess.hip
    (OpenCV's published 8-bit INTER_LINEAR rule, restated): (d + 0.5) * (src / dst) - 0.5 in double, cast to float, floor + fraction, clamped
    to the image with a zero fraction at the borders, coefficients rounded half to even."""
    scale = 1.0 / (float(dst) / float(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    edge = (s < 0) | (s >= src - 1)
    f[edge] = 0
    s = np.clip(s, 0, src - 1)
    return s, np.minimum(s + 1, src - 1), np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64), np.rint(f * np.float32(2048)).astype(np.int64)


def _resize_linear(img, new_h, new_w):
    """HxWx3 uint8 -> new_h x new_w x 3 uint8 by the two integer passes of the pixel kernels."""
    x0, x1, ax0, ax1 = _linear_coef(new_w, img.shape[1])
    y0, y1, ay0, ay1 = _linear_coef(new_h, img.shape[0])
    src = img.astype(np.int64)
    hor = src[:, x0] * ax0[None, :, None] + src[:, x1] * ax1[None, :, None]
    out = (((ay0[:, None, None] * (hor[y0] >> 4)) >> 16) + ((ay1[:, None, None] * (hor[y1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def letterbox_host(frames, new_shape=640, stride=32, auto=True, scaleup=True, dtype=torch.float16, rgb=False, pixel_format='bgr', matrix='bt601'):
    """``DevicePipeline.letterbox`` in numpy, bit for bit (the arithmetic: include/mcgaze_hip.h, "the detector's input"), for checks and for
    users without a GPU: the demo's LoadImages (letterbox, then img[:, :, ::-1].transpose(2, 0, 1); utils/datasets.py:185-189) and the
    conversion of detect.py:64-65, with cv2.resize and cv2.copyMakeBorder restated, not linked.

    frames: HxWx3 uint8 arrays in cv2's BGR order (rgb=True: RGB, no swap), or with pixel_format='nv12' surfaces as head_crops takes them
    ((y, uv) pairs or [3H/2, W] arrays, even sizes), converted by ``nv12_to_bgr(..., matrix)``; device tensors are read back.  The frames may
    differ in size but must share one output shape (ValueError).  dtype: uint8 (the bytes), float32 (byte / 255) or float16 (that float
    rounded to half: what ``img.half() / 255.0`` gives) -- a torch or numpy type.
    -> (img [B, 3, out_h, out_w] numpy array, [LetterboxGeometry per frame])."""
    nv12, _ = _pixel_format(pixel_format, matrix)
    np_dtype = LETTERBOX_DTYPES[_letterbox_dtype(dtype)]
    _letterbox_options(new_shape, stride)
    images = []
    for k, im in enumerate(frames):
        if nv12:
            host = lambda t: _host_array(t) if isinstance(t, torch.Tensor) else t
            y, uv, _ = _nv12_planes(k, tuple(host(t) for t in im) if isinstance(im, (tuple, list)) else host(im))
            images.append(nv12_to_bgr(y, uv, matrix))
        else:
            images.append(_bgr_frame(k, np.ascontiguousarray(_host_array(im))))
    geoms, out_h, out_w = _letterbox_plan([im.shape[:2] for im in images], new_shape, stride, auto, scaleup)
    out = np.full((len(images), out_h, out_w, 3), LETTERBOX_PAD, np.uint8)
    for k, (im, g) in enumerate(zip(images, geoms)):
        out[k, g.top:g.top + g.unpad_h, g.left:g.left + g.unpad_w] = _resize_linear(im, g.unpad_h, g.unpad_w)
    if not (rgb and not nv12):
        out = out[..., ::-1]
    out = np.ascontiguousarray(out.transpose(0, 3, 1, 2))
    if np_dtype is np.uint8:
        return out, geoms
    table = np.arange(256, dtype=np.float32) / np.float32(255)        # one IEEE f32 division per byte value, then one rounding to half
    return table.astype(np_dtype)[out], geoms
