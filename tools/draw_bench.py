#!/usr/bin/env python3
"""Gaze arrows drawn on the device, measured against the route a caller had before.  Prints ONE JSON line.

usage: draw_bench.py [--frames 8] [--heads 1,4,16] [--height 1080] [--width 1920] [--matrix bt709] [--steps 20] [--warmup 3] [--rounds 3]

Workload: `--frames` synthetic frames (random bytes) in device memory, packed BGR and NV12 surfaces, and for each head count of `--heads`
frames x heads arrows from head boxes of sides 120 - 400 px with unit gazes; boxes, gazes and image_of are device tensors.  Two ways,
alternated --rounds times, each round = --warmup untimed calls, then --steps calls bracketed by synchronize:
  device:  DevicePipeline.draw_arrows on the frames where they are, in place (mcg_draw_gaze_arrows / mcg_draw_gaze_arrows_nv12);
  host:    what a caller did before -- every frame and the tables copied to the host, pipeline.draw_arrows_host (numpy), every frame copied
           back.  HOST-BOUND: its time is the two PCIe copies plus numpy on one core, not a GPU figure; it is slow enough that a round of
           it is --steps / 10 calls after one untimed call.
Reported per pixel format, head count and way: ms per call of every round and the median.  The two ways' frames are checked equal once, on
fresh copies of the frames (arrows drawn over arrows would be equal too, but say less)."""
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
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--heads', default='1,4,16')
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--matrix', default='bt709', choices=sorted(P.YUV_COEF))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    dev = 'cuda:0'
    rs = np.random.RandomState(3)
    H, W = a.height, a.width
    pipe = P.DevicePipeline(CHAIN)
    sources = dict(bgr=[torch.from_numpy(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)).to(dev) for _ in range(a.frames)],
                   nv12=[torch.from_numpy(rs.randint(0, 256, (H * 3 // 2, W)).astype(np.uint8)).to(dev) for _ in range(a.frames)])
    cases = []
    for heads in [int(v) for v in a.heads.split(',')]:
        side = rs.randint(120, 401, (a.frames, heads))
        x1 = rs.randint(-40, W - 80, (a.frames, heads))
        y1 = rs.randint(-40, H - 80, (a.frames, heads))
        boxes = np.stack([x1, y1, x1 + side, y1 + side], axis=-1).reshape(-1, 4).astype(np.float32)
        g = rs.normal(size=(len(boxes), 3))
        gaze = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
        image_of = np.repeat(np.arange(a.frames), heads).astype(np.int32)
        tables = [torch.from_numpy(t).to(dev) for t in (boxes, gaze, image_of)]
        for fmt, frames in sources.items():
            kw = dict(pixel_format=fmt, matrix=a.matrix)

            def device(frames=frames):
                return pipe.draw_arrows(frames, *tables, device=dev, **kw)[0]

            def host(frames=frames):
                arrays = [f.cpu().numpy() for f in frames]
                out, _ = P.draw_arrows_host(arrays, *[t.cpu().numpy() for t in tables], **kw)
                if fmt == 'nv12':
                    out = [np.concatenate([y, uv]) for y, uv in out]
                return [torch.from_numpy(o).to(dev) for o in out]

            fresh = [f.clone() for f in frames]
            got, old = device(fresh), host(frames)
            torch.cuda.synchronize()
            equal = all(bool(torch.equal(x, y)) for x, y in zip(got, old))
            changed = sum(int((x != y).sum()) for x, y in zip(got, frames))       # bytes the arrows changed
            del got, old, fresh
            ways = dict(device=device, host=host)
            ms = {k: [] for k in ways}
            for _ in range(a.rounds):
                for k, fn in ways.items():
                    ms[k].append(timed(fn, a.steps if k == 'device' else max(a.steps // 10, 1), a.warmup if k == 'device' else 1))
            cases.append(dict(pixel_format=fmt, heads=heads, arrows=len(boxes), frames_equal=equal, changed_bytes=changed,
                              ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3)) for k in ways}))
    print(json.dumps(dict(tool='draw_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                          frames=a.frames, frame_hw=[H, W], matrix=a.matrix, steps=a.steps, host_steps=max(a.steps // 10, 1), warmup=a.warmup, rounds=a.rounds,
                          cases=cases)))


if __name__ == '__main__':
    main()
