"""Head boxes from a detector's raw output, on the host (not gpu): pipeline.detect_heads_host -- the arithmetic of include/mcgaze_hip.h, "head
boxes from raw detector output" -- against a restatement of the reference's non_max_suppression + scale_coords(...).round() in torch CPU f32
tensor operations, in the reference's order, and against answers worked by hand.  The device kernel is compared with detect_heads_host, bit
for bit, in tests/test_gpu_detect.py.  The reference tree is not read: torchvision's nms, which it calls, is restated as a plain loop."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from mcgaze_amd import harness
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import detect_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(conf_thres=0.25, iou_thres=0.45, only_class=1, agnostic=False, max_nms=30000, max_det=300)


def restated(pred, in_shape, frame_hw, conf_thres, iou_thres, only_class, agnostic, max_nms, max_det):
    """utils/general.py:393-481 and 291-312 on pred.float(), line for line in torch, with the three things the header states on top: rows that are
    not finite are dropped (the commented-out constraint), the sort is stable (ties: the lower anchor), and the sort happens whatever the count.
    -> per image (det [n, 6] = xyxy rounded, conf, cls; candidates that took part; whether max_nms cut them), None for a frame without pixels."""
    prediction = torch.from_numpy(np.asarray(pred).astype(np.float32)).clone()
    frame_hw = np.broadcast_to(np.asarray(frame_hw), (len(prediction), 2))
    xc = prediction[..., 4] > conf_thres
    out = []
    for xi, x in enumerate(prediction):
        h0, w0 = int(frame_hw[xi][0]), int(frame_hw[xi][1])
        if h0 <= 0 or w0 <= 0:
            out.append(None)
            continue
        x = x[xc[xi]]
        x[:, 5:] *= x[:, 4:5]
        box = x[:, :4].clone()                                   # xywh2xyxy
        box[:, 0] = x[:, 0] - x[:, 2] / 2
        box[:, 1] = x[:, 1] - x[:, 3] / 2
        box[:, 2] = x[:, 0] + x[:, 2] / 2
        box[:, 3] = x[:, 1] + x[:, 3] / 2
        conf, j = x[:, 5:].max(1, keepdim=True)
        x = torch.cat((box, conf, j.float()), 1)[conf.view(-1) > conf_thres]
        if only_class >= 0:
            x = x[(x[:, 5:6] == torch.tensor([only_class])).any(1)]
        x = x[torch.isfinite(x).all(1)]
        order = torch.sort(x[:, 4], descending=True, stable=True)[1]
        cut = x.shape[0] > max_nms
        x = x[order[:max_nms]]
        c = x[:, 5:6] * (0 if agnostic else 4096)
        boxes = x[:, :4] + c
        # torchvision's published nms rule, as a plain loop over the sorted rows
        areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        gone, keep = torch.zeros(len(boxes), dtype=torch.bool), []
        for i in range(len(boxes)):
            if gone[i]:
                continue
            keep.append(i)
            w = (torch.minimum(boxes[i, 2], boxes[i + 1:, 2]) - torch.maximum(boxes[i, 0], boxes[i + 1:, 0])).clamp(min=0)
            h = (torch.minimum(boxes[i, 3], boxes[i + 1:, 3]) - torch.maximum(boxes[i, 1], boxes[i + 1:, 1])).clamp(min=0)
            inter = w * h
            gone[i + 1:] |= inter / (areas[i] + areas[i + 1:] - inter) > iou_thres
        det = x[keep[:max_det]].clone()
        gain = min(in_shape[0] / h0, in_shape[1] / w0)           # scale_coords
        pad = (in_shape[1] - w0 * gain) / 2, (in_shape[0] - h0 * gain) / 2
        det[:, [0, 2]] -= pad[0]
        det[:, [1, 3]] -= pad[1]
        det[:, :4] /= gain
        det[:, 0].clamp_(0, w0)
        det[:, 1].clamp_(0, h0)
        det[:, 2].clamp_(0, w0)
        det[:, 3].clamp_(0, h0)
        det[:, :4] = det[:, :4].round()
        out.append((det, len(boxes), cut))
    return out


@pytest.fixture(scope='module')
def host_results():
    return {name: P.detect_heads_host(pred, in_shape, hw, **opts) for name, (pred, in_shape, hw, opts) in D.ALL.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize('name', list(D.ALL))
def test_host_equals_the_reference_restated_in_torch(host_results, name):
    pred, in_shape, hw, opts = D.ALL[name]
    boxes, scores, classes, image_of, counts, flags = host_results[name]
    o = {**DEFAULTS, **opts}
    assert boxes.dtype == scores.dtype == np.float32 and classes.dtype == image_of.dtype == counts.dtype == flags.dtype == np.int32
    assert boxes.shape == (len(pred), o['max_det'], 4) and scores.shape == classes.shape == image_of.shape == (len(pred), o['max_det'])
    for b, ref in enumerate(restated(pred, in_shape, hw, **o)):
        n = int(counts[b])
        if ref is None:
            assert flags[b] == 2 and n == 0
        else:
            det, _, cut = ref
            assert n == len(det) and flags[b] == int(cut), (name, b)
            assert np.array_equal(bits(boxes[b, :n]), bits(det[:, :4].numpy())), (name, b)          # bit for bit
            assert np.array_equal(bits(scores[b, :n]), bits(det[:, 4].numpy())), (name, b)
            assert np.array_equal(classes[b, :n], det[:, 5].numpy().astype(np.int32)) and (image_of[b, :n] == b).all()
        assert not boxes[b, n:].any() and not scores[b, n:].any() and not classes[b, n:].any() and (image_of[b, n:] == -1).all()


def test_fp16_predictions_are_widened_exactly():
    pred, in_shape, hw, opts = D.RANDOM['n65_every_class']
    half = pred.astype(np.float16)
    got, want = P.detect_heads_host(half, in_shape, hw, **opts), P.detect_heads_host(half.astype(np.float32), in_shape, hw, **opts)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[4][0] >= 2


@pytest.mark.parametrize('name', list(D.HAND))
def test_hand_cases(name):
    pred, opts, want_boxes, want_classes = D.HAND[name]
    boxes, scores, classes, image_of, counts, flags = P.detect_heads_host(pred, D.SQUARE, D.SQUARE, **opts)
    n = int(counts[0])
    assert n == len(want_boxes) and flags.tolist() == [0]
    assert boxes[0, :n].tolist() == want_boxes and classes[0, :n].tolist() == want_classes
    assert (np.diff(scores[0, :n]) <= 0).all() and image_of[0].tolist() == [0] * n + [-1] * (300 - n)


def test_the_cases_prove_themselves(host_results):
    for name, (pred, in_shape, hw, opts) in D.RANDOM.items():
        # an image with two or more detections and a suppressed candidate: fewer rows kept than took part, with max_det out of the way
        full = restated(pred, in_shape, hw, **{**DEFAULTS, **opts, 'max_det': 300})
        assert any(2 <= len(det) < min(took_part, 300) for det, took_part, _ in full), name
        assert host_results[name][4].max() >= 2, name
    assert host_results['n1025_b3_mixed_frames'][4][1] == 0 and host_results['n1_k0'][4][0] == 0        # images without a candidate
    assert host_results['n700_max_det'][4][0] == 7 and host_results['n2048_all'][4][0] == 300              # count == max_det
    assert host_results['n700_max_nms'][5].tolist() == [1, 1] and host_results['n2048_all_max_nms'][5].tolist() == [1]
    assert host_results['no_frame'][5].tolist() == [0, 2, 2] and host_results['no_frame'][4][0] > 0
    for name, (pred, _, _, _) in D.SIZES.items():                  # the stated candidate counts
        n, k = re.match(r'n(\d+)_(?:k(\d+)|all)', name).groups()
        passing = int(((pred[0, :, 4] > (0.0 if k is None else 0.25)) & (pred[0, :, 6] * pred[0, :, 4] > (0.0 if k is None else 0.25))).sum())
        assert pred.shape[1] == int(n) and passing == (int(n) if k is None else int(k)), name


def test_max_nms_keeps_the_prefix_of_the_full_result():
    """Greedy NMS decides a row from the rows before it only: the truncated run's detections are the full run's, restricted to the best max_nms."""
    for name, full_name in (('n700_max_nms', None), ('n2048_all_max_nms', 'n2048_all')):
        pred, in_shape, hw, opts = D.ALL[name]
        cut = P.detect_heads_host(pred, in_shape, hw, **opts)
        full = P.detect_heads_host(pred, in_shape, hw, **{**opts, 'max_nms': 30000})
        for b in range(len(pred)):
            thr, sc = np.float32(opts.get('conf_thres', 0.25)), pred[b, :, 5:] * pred[b, :, 4:5]
            conf = np.sort(sc.max(axis=1)[(pred[b, :, 4] > thr) & (sc.max(axis=1) > thr) & (sc.argmax(axis=1) == 1)])[::-1]      # the head candidates
            assert cut[5][b] == 1 and full[5][b] == 0
            floor = conf[opts['max_nms'] - 1]                       # the score of the last row that took part (no ties at the cut in these cases)
            assert conf[opts['max_nms']] < floor
            inside = full[1][b, :full[4][b]] >= floor
            n = int(cut[4][b])
            assert n == min(int(inside.sum()), 300) and np.array_equal(cut[0][b, :n], full[0][b, :full[4][b]][inside][:n])


def test_argument_checks():
    pred, in_shape, hw, _ = D.RANDOM['n63_tight_iou']
    for bad in (dict(max_det=0), dict(max_det=301), dict(max_nms=0), dict(conf_thres=float('nan')), dict(iou_thres=float('inf')), dict(only_class=-2)):
        with pytest.raises(ValueError):
            P.detect_heads_host(pred, in_shape, hw, **bad)
    with pytest.raises(ValueError):
        P.detect_heads_host(pred[0], in_shape, hw)                       # not [B, N, 5 + nc]
    with pytest.raises(ValueError):
        P.detect_heads_host(pred[:, :, :5], in_shape, hw)                # no class
    with pytest.raises(ValueError):
        P.detect_heads_host(pred, in_shape, [[1, 2], [3, 4]])            # frame_hw for another batch
    with pytest.raises(ValueError):
        P.detect_heads_host(pred, (0, 160), hw)
    with pytest.raises(TypeError):
        P.detect_heads_host(pred, in_shape, (160.5, 160.0))
    with pytest.raises(TypeError):
        P.detect_heads_host(pred.astype(np.float64), in_shape, hw)
    assert P.detect_heads_host(pred[:0], in_shape, np.zeros((0, 2), np.int32))[0].shape == (0, 300, 4)
    assert P.detect_heads_host(pred, in_shape, hw, only_class=None)[4][0] >= P.detect_heads_host(pred, in_shape, hw)[4][0]


def test_head_boxes_per_frame_and_the_run_head_video_signature():
    boxes, _, _, _, counts, _ = P.detect_heads_host(*D.RANDOM['n1025_b3_mixed_frames'][:3])
    per_frame = harness.head_boxes_per_frame(boxes, counts)
    assert [len(f) for f in per_frame] == counts.tolist() and per_frame[1] == [] and per_frame[0][0] == boxes[0, 0].tolist()
    assert harness.head_boxes_per_frame(torch.from_numpy(boxes), torch.from_numpy(counts)) == per_frame
    with pytest.raises(ValueError):
        harness.head_boxes_per_frame(boxes, counts[:2])
    sig = inspect.signature(harness.run_head_video)
    assert sig.parameters['detections'].default is None and sig.parameters['boxes_per_frame'].default is None
    for both in (dict(), dict(boxes_per_frame=[], detections=dict(pred=np.zeros((0, 4, 7), np.float32), in_shape=(8, 8)))):
        with pytest.raises(ValueError):
            harness.run_head_video(None, None, [], **both)


def test_header_binding_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    assert re.search(r'\bsize_t mcg_detect_heads_workspace_bytes\(int num_images, int num_anchors\);', hdr)
    assert re.search(r'\bint mcg_detect_heads\(mcg_stream s, const float\* pred_dev,', hdr)
    for name, nargs in (('mcg_detect_heads_workspace_bytes', 2), ('mcg_detect_heads', 24)):
        assert name in L.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20 and '#define MCG_ABI_VERSION 20' in hdr
    assert 'detect.hip' in open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'Makefile')).read()
    # 32 bytes per anchor (rounded up to 64 anchors) per image; sizes the entry refuses give 0
    assert lib.mcg_detect_heads_workspace_bytes(3, 1025) == 3 * 1088 * 32 and lib.mcg_detect_heads_workspace_bytes(0, 5) == 0
    assert lib.mcg_detect_heads_workspace_bytes(1, 0) == 0 and lib.mcg_detect_heads_workspace_bytes(-1, 5) == 0
    assert P.DevicePipeline.detect_heads is not None
