#!/usr/bin/env python3
"""Text labels drawn on the device, measured against the arrows on the same rows, against the route a caller had before, and inside a live
tick.  Prints ONE JSON line.

usage: labels_bench.py [--frames 8] [--rows 8,32,128] [--scales 2,4] [--height 1080] [--width 1920] [--matrix bt709] [--steps 20] [--warmup 3]
                       [--rounds 3] [--live 1x8x3,4x16x6] [--live-steps 20] [--live-warmup 16]

Workload: `--frames` synthetic frames (random bytes) in device memory, packed BGR and NV12 surfaces; for each row count of `--rows` that many
head boxes of sides 120 - 400 px spread over the frames, ids 1 .. rows and dwell counts of up to 60 s (texts '#12 3.4s' of 5 to 10
characters, made by DevicePipeline.format_labels), unit gazes for the arrows; every table is a device tensor.  Three ways, the two device
ways alternated --rounds times, each round = --warmup untimed calls, then --steps calls bracketed by synchronize:
  labels: DevicePipeline.draw_labels on the frames where they are, in place (mcg_draw_labels / mcg_draw_labels_nv12), at each of --scales;
  arrows: DevicePipeline.draw_arrows on the same rows and frames, in the same process;
  host:   what a caller did before -- every frame and the tables copied to the host, arrows.draw_labels_host (numpy), every frame copied
          back.  HOST-BOUND: the two PCIe copies plus numpy on one core, not a GPU figure; timed ONCE per case, and that one call is also the
          check that both routes draw the same bytes (on fresh copies of the frames).
format: DevicePipeline.format_labels alone on the same rows.
live: LiveGaze.tick at tools/live_bench.py's shapes (cameras x slots x people, 1080p frames, walkers that are always matched), draw=True with
and without labels=True, alternated --rounds times.
No target is fixed in advance: the cost of the labels is whatever this prints."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from mcgaze_amd import arrows as AR  # noqa: E402
from mcgaze_amd import lib, synth  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from draw_bench import CHAIN, timed  # noqa: E402  (tools/ is the script's directory)


def live_cases(a, dev):
    from live_bench import CLIP, FRAME_H, FRAME_W, STRIDE, walkers
    from live_bench import timed as timed_ticks
    from mcgaze_amd.engine import HipEngine
    from mcgaze_amd.live import LiveGaze
    rs = np.random.RandomState(11)
    engine = HipEngine(synth.make_state_dict(0), precision='f16x3')
    out = []
    for case in [c for c in a.live.split(',') if c]:
        Q, S, people = (int(v) for v in case.split('x'))
        ticks = a.rounds * (a.live_warmup + a.live_steps)
        host_boxes, host_counts = walkers(rs, Q, ticks, people)
        boxes, counts = torch.from_numpy(host_boxes).to(dev), torch.from_numpy(host_counts).to(dev)
        frames = [torch.randint(0, 256, (FRAME_H, FRAME_W, 3), dtype=torch.uint8, device=dev) for _ in range(Q)]
        pipe = P.DevicePipeline(CHAIN)
        options = dict(cameras=Q, slots=S, clip_len=CLIP, stride=STRIDE, smooth=0.6, draw=True)
        routes = dict(draw=LiveGaze(engine, pipe, **options), draw_labels=LiveGaze(engine, pipe, labels=True, **options))
        at = {k: 0 for k in routes}

        def step(name):
            routes[name].tick(frames, boxes[at[name]], counts[at[name]])
            at[name] += 1

        ms = {k: [] for k in routes}
        for _ in range(a.rounds):
            for name in routes:
                for _ in range(a.live_warmup):
                    step(name)
                ms[name].append(timed_ticks(lambda: step(name), a.live_steps))
        out.append(dict(cameras=Q, slots=S, people=people, frame=[FRAME_H, FRAME_W], precision='f16x3',
                        ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3)) for k in ms}))
        del routes
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--rows', default='8,32,128')
    ap.add_argument('--scales', default='2,4')
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--matrix', default='bt709', choices=sorted(P.YUV_COEF))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--live', default='1x8x3,4x16x6')
    ap.add_argument('--live-steps', type=int, default=20)
    ap.add_argument('--live-warmup', type=int, default=16)
    a = ap.parse_args()
    dev = 'cuda:0'
    rs = np.random.RandomState(3)
    H, W = a.height, a.width
    pipe = P.DevicePipeline(CHAIN)
    sources = dict(bgr=[torch.from_numpy(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)).to(dev) for _ in range(a.frames)],
                   nv12=[torch.from_numpy(rs.randint(0, 256, (H * 3 // 2, W)).astype(np.uint8)).to(dev) for _ in range(a.frames)])
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    cases = []
    for n in [int(v) for v in a.rows.split(',')]:
        side = rs.randint(120, 401, n)
        x1, y1 = rs.randint(-40, W - 80, n), rs.randint(-40, H - 80, n)
        boxes = np.stack([x1, y1, x1 + side, y1 + side], axis=-1).astype(np.float32)
        g = rs.normal(size=(n, 3))
        gaze = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
        image_of = (np.arange(n) % a.frames).astype(np.int32)
        ids, values = np.arange(1, n + 1, dtype=np.int32), rs.randint(1, 1800, n).astype(np.int32)
        d_boxes, d_gaze, d_image_of, d_ids, d_values = (up(t) for t in (boxes, gaze, image_of, ids, values))
        text = pipe.format_labels(d_ids, d_values, rate=(30, 1), device=dev)
        text_host = text.cpu().numpy()
        assert np.array_equal(text_host, AR.format_labels_host(ids, values, (30, 1)))
        format_ms = [round(timed(lambda: pipe.format_labels(d_ids, d_values, rate=(30, 1), out=text, device=dev), a.steps, a.warmup), 4) for _ in range(a.rounds)]
        for fmt, frames in sources.items():
            kw = dict(pixel_format=fmt, matrix=a.matrix)
            for scale in [int(v) for v in a.scales.split(',')]:

                def labels(frames=frames):
                    return pipe.draw_labels(frames, d_boxes, d_image_of, text, scale=scale, device=dev, **kw)[0]

                def arrows(frames=frames):
                    return pipe.draw_arrows(frames, d_boxes, d_gaze, d_image_of, device=dev, **kw)[0]

                def host(frames=frames):
                    arrays = [f.cpu().numpy() for f in frames]
                    out = AR.draw_labels_host(arrays, d_boxes.cpu().numpy(), d_image_of.cpu().numpy(), text.cpu().numpy(), scale=scale, **kw)[0]
                    if fmt == 'nv12':
                        out = [np.concatenate([y, uv]) for y, uv in out]
                    return [torch.from_numpy(o).to(dev) for o in out]

                fresh = [f.clone() for f in frames]
                got = labels(fresh)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                old = host(frames)
                torch.cuda.synchronize()
                host_ms = (time.perf_counter() - t0) * 1e3
                equal = all(bool(torch.equal(x, y)) for x, y in zip(got, old))
                changed = sum(int((x != y).sum()) for x, y in zip(got, frames))   # bytes the labels changed
                del got, old, fresh
                ways = dict(labels=labels, arrows=arrows)
                ms = {k: [] for k in ways}
                for _ in range(a.rounds):
                    for k, fn in ways.items():
                        ms[k].append(timed(fn, a.steps, a.warmup))
                cases.append(dict(pixel_format=fmt, rows=n, scale=scale, frames_equal=equal, changed_bytes=changed, host_ms_one_call=round(host_ms, 1),
                                  format_ms=format_ms,
                                  ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3)) for k in ways}))
    live = live_cases(a, dev)
    print(json.dumps(dict(tool='labels_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                          frames=a.frames, frame_hw=[H, W], matrix=a.matrix, steps=a.steps, warmup=a.warmup, rounds=a.rounds, cases=cases, live=live)))


if __name__ == '__main__':
    main()
