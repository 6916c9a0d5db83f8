"""Head boxes from the raw output of the demo's head detector: ``DevicePipeline.detect_heads`` (``mcg_detect_heads``: confidence filter, NMS and
scale-back; csrc/detect.hip) never leaves the device; ``detect_heads_host`` is the same in numpy, and the option and shape checks they share."""
import numpy as np
import torch

from .staging import _host_array

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
