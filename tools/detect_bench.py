#!/usr/bin/env python3
"""Head boxes from a detector's raw output on the device, measured against the same steps in torch on the device.  Prints ONE JSON line.

usage: detect_bench.py [--images 1,8,64] [--anchors 25200] [--heads 3,40] [--steps 20] [--warmup 3] [--rounds 3]

Workload: for each batch size of `--images`, a synthetic raw prediction [B, N, 7] (nc = 2: person, head) of a 640-pixel detector in device
memory: background anchors below the threshold and per image between `--heads` lo and hi clustered heads, 4 - 12 anchors firing on each;
frames are 1080p in a 384 x 640 letterbox.  Two ways, alternated --rounds times, each round = --warmup untimed calls, then --steps calls
bracketed by synchronize:
  device:  DevicePipeline.detect_heads (mcg_detect_heads: one launch, one workgroup per image, nothing read back);
  torch:   what a caller did before -- non_max_suppression + scale_coords(...).round() with torch operations on the device, image by image,
           with a pure-torch greedy NMS in place of torchvision's (which is not importable next to this project).  SYNC-BOUND: boolean
           indexing and the greedy loop wait for the device once or more per image and per kept box, so its time is launch and sync
           latency, not arithmetic; a round of it is --steps / 5 calls after one untimed call.
Reported per batch size and way: ms per call of every round and the median; the two ways' boxes and counts are compared once."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mcgaze_amd import lib  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402

CHAIN = [dict(type='LoadImageFromFile'), dict(type='Resize', img_scale=(448, 448), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.0),
         dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True), dict(type='Pad', size_divisor=32),
         dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img'])]
IN_SHAPE, FRAME = (384, 640), (1080, 1920)


def prediction(rs, B, N, heads):
    h, w = IN_SHAPE
    p = np.zeros((B, N, 7), np.float32)
    p[..., 0], p[..., 1] = rs.uniform(0, w, (B, N)), rs.uniform(0, h, (B, N))
    p[..., 2:4] = rs.uniform(4, 80, (B, N, 2))
    p[..., 4] = rs.uniform(0, 0.2, (B, N))
    p[..., 5:] = rs.uniform(0, 1, (B, N, 2))
    total = 0
    for b in range(B):
        rows = rs.permutation(N)
        at = 0
        for _ in range(int(rs.randint(heads[0], heads[1] + 1))):
            k = int(rs.randint(4, 13))
            r = rows[at:at + k]
            at += k
            cx, cy, size = rs.uniform(0.05 * w, 0.95 * w), rs.uniform(0.1 * h, 0.9 * h), rs.uniform(10, 60)
            p[b, r, 0], p[b, r, 1] = cx + rs.uniform(-0.08, 0.08, k) * size, cy + rs.uniform(-0.08, 0.08, k) * size
            p[b, r, 2], p[b, r, 3] = size * rs.uniform(0.9, 1.1, k), size * rs.uniform(0.9, 1.2, k)
            p[b, r, 4], p[b, r, 5], p[b, r, 6] = rs.uniform(0.3, 0.98, k), rs.uniform(0, 0.3, k), rs.uniform(0.6, 1.0, k)
        total += at
    return p, total


def torch_route(pred, conf_thres=0.25, iou_thres=0.45, head=1, max_det=300):
    """utils/general.py:393-481 and 291-312 with torch operations on pred's device -> (boxes [B, max_det, 4], counts [B])."""
    B = pred.shape[0]
    boxes, counts = torch.zeros(B, max_det, 4, device=pred.device), torch.zeros(B, dtype=torch.int32, device=pred.device)
    gain = min(IN_SHAPE[0] / FRAME[0], IN_SHAPE[1] / FRAME[1])
    pad = (IN_SHAPE[1] - FRAME[1] * gain) / 2, (IN_SHAPE[0] - FRAME[0] * gain) / 2
    for b in range(B):
        x = pred[b][pred[b, :, 4] > conf_thres]
        sc = x[:, 5:] * x[:, 4:5]
        half = x[:, 2:4] / 2
        box = torch.cat((x[:, :2] - half, x[:, :2] + half), 1)
        conf, j = sc.max(1)
        ok = (conf > conf_thres) & (j == head)
        box, conf = box[ok], conf[ok]
        order = torch.sort(conf, descending=True, stable=True)[1]
        off = box[order] + head * 4096
        area = (off[:, 2] - off[:, 0]) * (off[:, 3] - off[:, 1])
        alive, keep = torch.arange(len(order), device=pred.device), []
        while alive.numel() and len(keep) < max_det:             # one wait for the device per kept box
            i, rest = alive[0], alive[1:]
            keep.append(i)
            w = (torch.minimum(off[i, 2], off[rest, 2]) - torch.maximum(off[i, 0], off[rest, 0])).clamp(min=0)
            h = (torch.minimum(off[i, 3], off[rest, 3]) - torch.maximum(off[i, 1], off[rest, 1])).clamp(min=0)
            inter = w * h
            alive = rest[~(inter / (area[i] + area[rest] - inter) > iou_thres)]
        if keep:
            det = box[order[torch.stack(keep)]].clone()
            det[:, [0, 2]] -= pad[0]
            det[:, [1, 3]] -= pad[1]
            det /= gain
            det[:, [0, 2]] = det[:, [0, 2]].clamp(0, FRAME[1])
            det[:, [1, 3]] = det[:, [1, 3]].clamp(0, FRAME[0])
            boxes[b, :len(keep)] = det.round()
            counts[b] = len(keep)
    return boxes, counts


def timed(fn, steps, warmup):
    for _ in range(max(warmup, 1)):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', default='1,8,64')
    ap.add_argument('--anchors', type=int, default=25200)
    ap.add_argument('--heads', default='3,40')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    dev = 'cuda:0'
    rs = np.random.RandomState(5)
    heads = tuple(int(v) for v in a.heads.split(','))
    pipe = P.DevicePipeline(CHAIN)
    cases = []
    for B in [int(v) for v in a.images.split(',')]:
        host_pred, fired = prediction(rs, B, a.anchors, heads)
        pred = torch.from_numpy(host_pred).to(dev)
        hw = torch.tensor([FRAME] * B, dtype=torch.int32, device=dev)

        def device():
            return pipe.detect_heads(pred, IN_SHAPE, hw)

        def torch_way():
            return torch_route(pred)

        got, old = device(), torch_way()
        torch.cuda.synchronize()
        equal = bool(torch.equal(got[0], old[0])) and bool(torch.equal(got[4], old[1]))
        detections = int(got[4].sum())
        ways = dict(device=device, torch=torch_way)
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                ms[k].append(timed(fn, a.steps if k == 'device' else max(a.steps // 5, 1), a.warmup if k == 'device' else 1))
        cases.append(dict(images=B, candidates=fired, detections=detections, boxes_equal=equal,
                          ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3)) for k in ways}))
    print(json.dumps(dict(tool='detect_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                          anchors=a.anchors, classes=2, in_shape=IN_SHAPE, frame_hw=FRAME, heads=heads, steps=a.steps, torch_steps=max(a.steps // 5, 1),
                          warmup=a.warmup, rounds=a.rounds, cases=cases)))


if __name__ == '__main__':
    main()
