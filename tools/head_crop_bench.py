#!/usr/bin/env python3
"""The head-crop stage alone, measured.  Prints ONE JSON line.

usage: head_crop_bench.py [--frames 64] [--heads 4] [--height 1080] [--width 1920] [--scale 448] [--steps 20] [--warmup 3] [--rounds 3]

Workload: `--frames` synthetic frames with `--heads` head boxes each (sides 120 - 400 px, some clipped by the frame border) -> frames x heads
crops through the L2CS chain at img_scale (`--scale`, `--scale`).  Three ways, alternated --rounds times, each round = --warmup untimed
calls, then --steps calls bracketed by synchronize:
  (a) host_frames:    DevicePipeline.head_crops on numpy frames and host tables (every frame staged and uploaded once per call);
  (b) device_frames:  head_crops on frames, boxes and image_of already in device memory (nothing uploaded);
  (c) numpy_slices:   what a caller could do before: slice every head out on the host and hand the slices to DevicePipeline.__call__
                      (every crop staged and uploaded on its own).
Reported per way: ms per call of every round, the median, and the bytes a call uploads.  (c) pads to the largest crop of the call like
mmcv's collate, (a) and (b) to img_scale: the tensors are checked equal on the region (c) holds."""
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

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


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
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--heads', type=int, default=4)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--scale', type=int, default=448)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    dev = 'cuda:0'
    rs = np.random.RandomState(3)
    H, W = a.height, a.width
    frames = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(a.frames)]
    side = rs.randint(120, 401, (a.frames, a.heads))
    x1 = rs.randint(-40, W - 80, (a.frames, a.heads))
    y1 = rs.randint(-40, H - 80, (a.frames, a.heads))
    boxes = np.stack([x1, y1, x1 + side, y1 + side], axis=-1).reshape(-1, 4).astype(np.float32)
    image_of = np.repeat(np.arange(a.frames), a.heads).astype(np.int32)
    pipe = P.DevicePipeline([dict(type='LoadImageFromFile'), dict(type='Resize', img_scale=(a.scale, a.scale), keep_ratio=True),
                             dict(type='RandomFlip', flip_ratio=0.0), dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32),
                             dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img'])])
    windows, empty = P.head_crop_windows(boxes, H, W)
    assert not empty.any()
    dev_frames = [torch.from_numpy(f).to(dev) for f in frames]
    dev_boxes, dev_image_of = torch.from_numpy(boxes).to(dev), torch.from_numpy(image_of).to(dev)

    def slices():
        return [frames[k][y:y + h, x:x + w] for k, (y, x, h, w) in zip(image_of, windows)]

    ways = dict(host_frames=lambda: pipe.head_crops(frames, boxes, image_of, device=dev),
                device_frames=lambda: pipe.head_crops(dev_frames, dev_boxes, dev_image_of, device=dev),
                numpy_slices=lambda: pipe(slices(), device=dev))
    ref = ways['host_frames']()[0]
    old = ways['numpy_slices']()[0]
    torch.cuda.synchronize()
    equal = bool(torch.equal(ref[:, :, :old.shape[2], :old.shape[3]], old) and torch.equal(ways['device_frames']()[0], ref))
    del ref, old
    ms = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            ms[k].append(timed(fn, a.steps, a.warmup))
    uploaded = dict(host_frames=sum(f.nbytes for f in frames) + boxes.nbytes + image_of.nbytes + a.frames * P._IMAGE.itemsize,
                    device_frames=0,
                    numpy_slices=int((windows[:, 2] * windows[:, 3] * 3).sum()) + len(boxes) * P._DESC.itemsize)
    print(json.dumps(dict(tool='head_crop_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName, frames=a.frames, heads=a.heads, frame_hw=[H, W], crops=len(boxes), img_scale=a.scale,
                          steps=a.steps, warmup=a.warmup, rounds=a.rounds, tensors_equal=equal,
                          ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3), uploaded_bytes=int(uploaded[k])) for k in ways})))


if __name__ == '__main__':
    main()
