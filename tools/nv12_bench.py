#!/usr/bin/env python3
"""NV12 surfaces into the head-crop stage, measured against the route a caller had before.  Prints ONE JSON line.

usage: nv12_bench.py [--frames 8] [--heads 1,4,16] [--height 1080] [--width 1920] [--scale 448] [--matrix bt709] [--steps 20] [--warmup 3] [--rounds 3]

Workload: `--frames` synthetic NV12 surfaces (full-range random bytes) in device memory with head boxes of sides 120 - 400 px, some clipped by
the frame border, and for each head count of `--heads` frames x heads crops through the L2CS chain at img_scale (`--scale`, `--scale`).
Boxes and image_of are device tensors: neither way touches the host.  Two ways, alternated --rounds times, each round = --warmup untimed
calls, then --steps calls bracketed by synchronize:
  nv12:       DevicePipeline.head_crops(pixel_format='nv12') on the surfaces as they are (mcg_preprocess_head_crops_nv12);
  torch_bgr:  every surface converted WHOLE to packed BGR with torch on the device (the same integer arithmetic, chroma repeated 2 x 2),
              then head_crops on the packed frames -- what a caller with NV12 surfaces had to do before.
Reported per head count and way: ms per call of every round, the median, and the bytes the way must move at the least (`min_bytes`: each
byte counted once however often a cache serves it again; torch's own intermediates -- int32 planes of the whole frame -- come on top for
torch_bgr and are NOT counted).  The two ways' tensors are checked equal."""
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


def torch_nv12_to_bgr(y, uv, k):
    """pipeline.nv12_to_bgr in torch on the device: y [H,W], uv [H/2,W] uint8 -> [H,W,3] uint8."""
    h, w = y.shape
    c = uv.reshape(h // 2, w // 2, 2).to(torch.int32) - 128
    u, v = (c[..., j].repeat_interleave(2, 0).repeat_interleave(2, 1) for j in (0, 1))
    yy = (y.to(torch.int32) - k['y_off']).clamp_(min=0) * k['cy'] + (1 << 19)
    sat8 = lambda t: (t >> 20).clamp_(0, 255)
    return torch.stack([sat8(yy + k['cub'] * u), sat8(yy + k['cvg'] * v + k['cug'] * u), sat8(yy + k['cvr'] * v)], dim=-1).to(torch.uint8)


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
    ap.add_argument('--scale', type=int, default=448)
    ap.add_argument('--matrix', default='bt709', choices=sorted(P.YUV_COEF))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    dev = 'cuda:0'
    rs = np.random.RandomState(3)
    H, W = a.height, a.width
    coef = P.YUV_COEF[a.matrix]
    surfaces = [torch.from_numpy(rs.randint(0, 256, (H * 3 // 2, W)).astype(np.uint8)).to(dev) for _ in range(a.frames)]
    pipe = P.DevicePipeline([dict(type='LoadImageFromFile'), dict(type='Resize', img_scale=(a.scale, a.scale), keep_ratio=True),
                             dict(type='RandomFlip', flip_ratio=0.0), dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32),
                             dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img'])])
    pad = pipe.head_crop_geometry()[2:4]
    cases = []
    for heads in [int(v) for v in a.heads.split(',')]:
        side = rs.randint(120, 401, (a.frames, heads))
        x1 = rs.randint(-40, W - 80, (a.frames, heads))
        y1 = rs.randint(-40, H - 80, (a.frames, heads))
        boxes = np.stack([x1, y1, x1 + side, y1 + side], axis=-1).reshape(-1, 4).astype(np.float32)
        image_of = np.repeat(np.arange(a.frames), heads).astype(np.int32)
        windows, empty = P.head_crop_windows(boxes, H, W)
        assert not empty.any()
        dev_boxes, dev_image_of = torch.from_numpy(boxes).to(dev), torch.from_numpy(image_of).to(dev)

        def nv12():
            return pipe.head_crops(surfaces, dev_boxes, dev_image_of, device=dev, pixel_format='nv12', matrix=a.matrix)

        def torch_bgr():
            return pipe.head_crops([torch_nv12_to_bgr(s[:H], s[H:], coef) for s in surfaces], dev_boxes, dev_image_of, device=dev)

        ways = dict(nv12=nv12, torch_bgr=torch_bgr)
        got, old = nv12(), torch_bgr()
        torch.cuda.synchronize()
        equal = all(bool(torch.equal(x, y)) for x, y in zip(got, old))
        del got, old
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                ms[k].append(timed(fn, a.steps, a.warmup))
        win_px = int((windows[:, 2] * windows[:, 3]).sum())
        out_bytes = len(boxes) * 3 * pad[0] * pad[1] * 4
        # nv12: the windows' Y bytes and half as many chroma bytes in, img out.  torch_bgr: every surface in (1.5 H W), its packed frame out
        # (3 H W) and the windows' 3 bytes per pixel back in, img out
        moved = dict(nv12=win_px * 3 // 2 + out_bytes, torch_bgr=a.frames * H * W * 9 // 2 + win_px * 3 + out_bytes)
        cases.append(dict(heads=heads, crops=len(boxes), tensors_equal=equal, img_bytes=out_bytes,
                          ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3), min_bytes=int(moved[k])) for k in ways}))
    print(json.dumps(dict(tool='nv12_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                          frames=a.frames, frame_hw=[H, W], img_scale=a.scale, matrix=a.matrix, steps=a.steps, warmup=a.warmup, rounds=a.rounds, cases=cases)))


if __name__ == '__main__':
    main()
