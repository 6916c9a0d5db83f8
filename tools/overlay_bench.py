#!/usr/bin/env python3
"""The attention overlay drawn on the device, measured against plain arrows and against the route a caller had before.  Prints ONE JSON line.

usage: overlay_bench.py [--frames 8] [--heads 1,4,16] [--regions 16] [--height 1080] [--width 1920] [--matrix bt709] [--steps 20] [--warmup 3]
                        [--rounds 3]

Workload: `--frames` synthetic frames (random bytes) in device memory, packed BGR and NV12 surfaces; for each head count of `--heads`
frames x heads rows from head boxes of sides 120 - 400 px with unit gazes; `--regions` regions of sides 200 - 600 px, a quarter of them on
every frame and the rest on one frame each, as rectangles, as quadrilaterals (every rectangle sheared) and as 8-gons (the octagon in every
rectangle).  kind / target / hit / mutual are what DevicePipeline.gaze_targets finds for these rows and regions; every table is a device
tensor.  Three ways, the two device ways alternated --rounds times, each round = --warmup untimed calls, then --steps calls bracketed by
synchronize:
  overlay: DevicePipeline.draw_attention on the frames where they are, in place (mcg_draw_attention / mcg_draw_attention_nv12);
  arrows:  DevicePipeline.draw_arrows on the same rows and frames, in the same process (mcg_draw_gaze_arrows / _nv12);
  host:    what a caller did before -- every frame and the tables copied to the host, arrows.draw_attention_host (numpy), every frame
           copied back.  HOST-BOUND: its time is the two PCIe copies plus numpy on one core, not a GPU figure; it is timed ONCE per case,
           and that one call is also the check that both routes draw the same bytes (on fresh copies of the frames).
Reported per pixel format, region form, head count and way: ms per call of every round and the median.  No ratio is claimed in advance:
the overlay's cost over the arrows is whatever this prints."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from mcgaze_amd import arrows as AR  # noqa: E402
from mcgaze_amd import attention as AT  # noqa: E402
from mcgaze_amd import lib  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from draw_bench import CHAIN, timed  # noqa: E402  (tools/ is the script's directory)


def region_forms(rs, count, frames, H, W):
    """-> ({form: mixed list}, region_image): the same rectangles as they are, sheared into quadrilaterals, and cut into octagons."""
    side_w, side_h = rs.randint(200, 601, count), rs.randint(200, 601, count)
    x1, y1 = rs.randint(0, W - 200, count), rs.randint(0, H - 200, count)
    rects = np.stack([x1, y1, x1 + side_w, y1 + side_h], axis=1).astype(np.float32)
    quads = [[[x, y], [X, y + 0.1 * (Y - y)], [X - 0.1 * (X - x), Y], [x + 0.05 * (X - x), Y - 0.05 * (Y - y)]] for x, y, X, Y in rects.tolist()]
    octs = [[[(x + X) / 2 + (X - x) / 2 * math.cos(math.pi * k / 4 + 0.3), (y + Y) / 2 + (Y - y) / 2 * math.sin(math.pi * k / 4 + 0.3)] for k in range(8)]
            for x, y, X, Y in rects.tolist()]
    region_image = np.where(np.arange(count) % 4 == 0, -1, rs.randint(0, frames, count)).astype(np.int32)
    return dict(rectangles=rects.tolist(), quadrilaterals=quads, octagons=octs), region_image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--heads', default='1,4,16')
    ap.add_argument('--regions', type=int, default=16)
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
    forms, region_image = region_forms(rs, a.regions, a.frames, H, W)
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    cases = []
    for heads in [int(v) for v in a.heads.split(',')]:
        side = rs.randint(120, 401, (a.frames, heads))
        x1 = rs.randint(-40, W - 80, (a.frames, heads))
        y1 = rs.randint(-40, H - 80, (a.frames, heads))
        boxes = np.stack([x1, y1, x1 + side, y1 + side], axis=-1).reshape(-1, 4).astype(np.float32)
        g = rs.normal(size=(len(boxes), 3))
        gaze = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
        image_of = np.repeat(np.arange(a.frames), heads).astype(np.int32)
        rows = [up(t) for t in (boxes, gaze, image_of)]
        for form, mixed in forms.items():
            xy, start = AT.region_polygons(mixed)
            regions = dict(regions=AT.PolyRegions(up(xy), up(start)), region_image=up(region_image))
            kind, target, _, hit, mutual, _ = pipe.gaze_targets(*rows, device=dev, **regions)
            tables = rows + [kind, target, hit, mutual]
            kinds = np.bincount(kind.cpu().numpy(), minlength=4).tolist()
            for fmt, frames in sources.items():
                kw = dict(pixel_format=fmt, matrix=a.matrix)

                def overlay(frames=frames):
                    return pipe.draw_attention(frames, *tables, device=dev, **regions, **kw)[0]

                def arrows(frames=frames):
                    return pipe.draw_arrows(frames, *rows, device=dev, **kw)[0]

                def host(frames=frames):
                    arrays = [f.cpu().numpy() for f in frames]
                    out = AR.draw_attention_host(arrays, *[t.cpu().numpy() for t in tables], regions=AT.PolyRegions(xy, start), region_image=region_image, **kw)[0]
                    if fmt == 'nv12':
                        out = [np.concatenate([y, uv]) for y, uv in out]
                    return [torch.from_numpy(o).to(dev) for o in out]

                fresh = [f.clone() for f in frames]
                got = overlay(fresh)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                old = host(frames)
                torch.cuda.synchronize()
                host_ms = (time.perf_counter() - t0) * 1e3
                equal = all(bool(torch.equal(x, y)) for x, y in zip(got, old))
                changed = sum(int((x != y).sum()) for x, y in zip(got, frames))   # bytes the overlay changed
                del got, old, fresh
                ways = dict(overlay=overlay, arrows=arrows)
                ms = {k: [] for k in ways}
                for _ in range(a.rounds):
                    for k, fn in ways.items():
                        ms[k].append(timed(fn, a.steps, a.warmup))
                cases.append(dict(pixel_format=fmt, regions=form, heads=heads, rows=len(boxes), kinds=kinds, frames_equal=equal, changed_bytes=changed,
                                  host_ms_one_call=round(host_ms, 1),
                                  ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3)) for k in ways}))
    print(json.dumps(dict(tool='overlay_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                          frames=a.frames, frame_hw=[H, W], regions=a.regions, matrix=a.matrix, steps=a.steps, warmup=a.warmup, rounds=a.rounds, cases=cases)))


if __name__ == '__main__':
    main()
