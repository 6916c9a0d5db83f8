#!/usr/bin/env python3
"""Gaze targets: the device call against the only route there was before it, and what LiveGaze(attention=True) adds to a tick.  Prints ONE
JSON line; --out also appends the note profiles/attention_<build id>.md holds.

usage: attention_bench.py [--shapes 8x1,64x8,1024x64] [--regions 16] [--calls 20] [--rounds 3] [--runs 2] [--live 1x8x3,4x16x6] [--steps 20]
                          [--warmup 16] [--out FILE]

1. The call.  Per shape n x pictures: n rows spread evenly over the pictures (ascending image_of, as LiveGaze's tables are), integer-pixel
   boxes in 1280 x 720 pictures, random unit gaze, --regions rectangles that apply to every picture; every table in device memory.
     device:    DevicePipeline.gaze_targets on the device tables (mcg_gaze_targets: two launches, nothing read back).
     readback:  the route before: boxes, gaze and image_of copied to the host, attention.gaze_targets_host, the six tables uploaded.
     quads, octagons:  the same rows and the same number of regions as polygons (mcg_gaze_targets_poly): every rectangle sheared into a
                quadrilateral, and with its corners cut into an 8-gon; vertex tables in device memory.
   --runs times: --rounds rounds alternated, each --calls calls bracketed by synchronize; the median round of each run, us per call.
2. The tick.  tools/live_bench.py's shapes and walkers (Q x S x people, 720 x 1280 frames, 448 x 448 crops, clip 7 / stride 4, synthetic
   weights, f16x3, smooth 0.6): LiveGaze.tick without and with attention=True in ONE process, two passes of each alternated, each --warmup
   untimed ticks then --steps timed; ms per tick per pass, the difference of the means, and the no-attention route's own spread between
   its two passes to set it against.
The ratios are those of this comparison only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from live_bench import CHAIN, CLIP, DEV, FRAME_H, FRAME_W, STRIDE, timed, walkers  # noqa: E402
from mcgaze_amd import lib, synth  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from mcgaze_amd.attention import PolyRegions, gaze_targets_host, region_polygons  # noqa: E402
from mcgaze_amd.engine import HipEngine  # noqa: E402
from mcgaze_amd.live import LiveGaze  # noqa: E402


def tables(rs, n, pictures, m):
    xy, wh = rs.randint(0, FRAME_W - 120, (n, 2)), rs.randint(40, 120, (n, 2))
    xy[:, 1] %= FRAME_H - 120
    boxes = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    gaze = rs.standard_normal((n, 3)).astype(np.float32)
    gaze /= np.linalg.norm(gaze, axis=1, keepdims=True)
    image_of = (np.arange(n) * pictures // n).astype(np.int32)
    rxy = rs.randint(0, FRAME_W - 300, (m, 2))
    rxy[:, 1] %= FRAME_H - 300
    regions = np.concatenate([rxy, rxy + rs.randint(50, 300, (m, 2))], axis=1).astype(np.float32)
    return boxes, gaze, image_of, regions


def polygons(regions, corners):
    """The rectangles as quadrilaterals (sheared by a fifth of the width) or as 8-gons (a quarter of each side cut off every corner)."""
    out = []
    for x1, y1, x2, y2 in regions.tolist():
        w, h = x2 - x1, y2 - y1
        if corners == 4:
            out.append([[x1 + w // 5, y1], [x2, y1], [x2 - w // 5, y2], [x1, y2]])
        else:
            a, b = w // 4, h // 4
            out.append([[x1 + a, y1], [x2 - a, y1], [x2, y1 + b], [x2, y2 - b], [x2 - a, y2], [x1 + a, y2], [x1, y2 - b], [x1, y1 + b]])
    return region_polygons(out)


def bench_call(pipe, shape, m, calls, rounds, runs, rs):
    n, pictures = shape
    host = tables(rs, n, pictures, m)
    boxes, gaze, image_of, regions = (torch.from_numpy(t).to(DEV) for t in host)
    region_image = torch.full((m,), -1, dtype=torch.int32, device=DEV)
    poly = {name: PolyRegions(*(torch.from_numpy(t).to(DEV) for t in polygons(host[3], c))) for name, c in (('quads', 4), ('octagons', 8))}

    def device():
        return pipe.gaze_targets(boxes, gaze, image_of, regions=regions, region_image=region_image, device=DEV)

    def readback():
        host = gaze_targets_host(boxes.cpu().numpy(), gaze.cpu().numpy(), image_of.cpu().numpy(), regions=regions.cpu().numpy(),
                                 region_image=region_image.cpu().numpy())
        return tuple(torch.from_numpy(t).to(DEV) for t in host)

    def polygon_route(name):
        return lambda: pipe.gaze_targets(boxes, gaze, image_of, regions=poly[name], region_image=region_image, device=DEV)

    same = all(torch.equal(a, b) for a, b in zip(device(), readback()))
    for name in poly:                                             # the polygon legs against the twin over the same vertex tables
        twin = gaze_targets_host(host[0], host[1], host[2], regions=PolyRegions(*(t.cpu().numpy() for t in poly[name])))
        same = same and all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(polygon_route(name)(), twin))
    routes = (('device', device), ('readback', readback), ('quads', polygon_route('quads')), ('octagons', polygon_route('octagons')))
    out = dict(rows=n, pictures=pictures, regions=m, equal=bool(same), us={name: [] for name, _ in routes})
    for _ in range(runs):
        us = {name: [] for name, _ in routes}
        for _ in range(rounds):
            for name, fn in routes:
                us[name].append(timed(fn, calls) * 1e3)
        for name in us:
            out['us'][name].append(round(float(np.median(us[name])), 2))
    out['readback_over_device'] = [round(r / d, 2) for d, r in zip(out['us']['device'], out['us']['readback'])]
    return out


def bench_live(engine, case, steps, warmup, rs):
    Q, S, people = case
    passes = 2
    ticks = passes * (warmup + steps)
    host_boxes, host_counts = walkers(rs, Q, ticks, people)
    boxes, counts = torch.from_numpy(host_boxes).to(DEV), torch.from_numpy(host_counts).to(DEV)
    frames = [torch.randint(0, 256, (FRAME_H, FRAME_W, 3), dtype=torch.uint8, device=DEV) for _ in range(Q)]
    pipe = P.DevicePipeline(CHAIN)
    options = dict(cameras=Q, slots=S, clip_len=CLIP, stride=STRIDE, smooth=0.6)
    routes = dict(plain=LiveGaze(engine, pipe, **options), attention=LiveGaze(engine, pipe, attention=True, **options))
    at = {k: 0 for k in routes}

    def step(name):
        routes[name].tick(frames, boxes[at[name]], counts[at[name]])
        at[name] += 1

    ms = {k: [] for k in routes}
    for _ in range(passes):
        for name in routes:
            for _ in range(warmup):
                step(name)
            ms[name].append(round(timed(lambda: step(name), steps), 4))
    mean = {k: float(np.mean(v)) for k, v in ms.items()}
    return dict(cameras=Q, slots=S, people=people, rows_per_call=Q * S, ms=ms, added_ms=round(mean['attention'] - mean['plain'], 4),
                plain_spread_ms=round(abs(ms['plain'][0] - ms['plain'][1]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x1,64x8,1024x64')
    ap.add_argument('--regions', type=int, default=16)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--live', default='1x8x3,4x16x6')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=16)
    ap.add_argument('--out')
    a = ap.parse_args()
    rs = np.random.RandomState(5)
    pipe = P.DevicePipeline(CHAIN)
    calls = [bench_call(pipe, tuple(int(v) for v in s.split('x')), a.regions, a.calls, a.rounds, a.runs, rs) for s in a.shapes.split(',') if s]
    ticks = []
    if a.live:
        engine = HipEngine(synth.make_state_dict(0), precision='f16x3')
        ticks = [bench_live(engine, tuple(int(v) for v in c.split('x')), a.steps, a.warmup, rs) for c in a.live.split(',')]
    line = dict(tool='attention_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                calls_per_round=a.calls, rounds=a.rounds, runs=a.runs, steps=a.steps, warmup=a.warmup, call=calls, tick=ticks)
    print(json.dumps(line))
    if a.out:
        rows = ['| rows x pictures, regions | device us / call (runs) | read-back us / call (runs) | read-back / device | quadrilaterals us / call (runs) | '
                '8-gons us / call (runs) | equal |', '|---|---|---|---|---|---|---|']
        for c in calls:
            rows.append(f"| {c['rows']} x {c['pictures']}, {c['regions']} | {c['us']['device']} | {c['us']['readback']} | {c['readback_over_device']} | "
                        f"{c['us']['quads']} | {c['us']['octagons']} | {c['equal']} |")
        more = ['| Q x S, people | rows a call | plain ms / tick (passes) | attention=True ms / tick (passes) | added ms | plain: spread between its passes |',
                '|---|---|---|---|---|---|']
        for t in ticks:
            more.append(f"| {t['cameras']} x {t['slots']}, {t['people']} | {t['rows_per_call']} | {t['ms']['plain']} | {t['ms']['attention']} | {t['added_ms']} | "
                        f"{t['plain_spread_ms']} |")
        with open(a.out, 'a') as f:
            f.write(f"\n## Run on {line['device']} ({line['arch']}), build {line['build_id']}\n\nThe call: {a.calls} calls a round, {a.rounds} rounds alternated, "
                    f"the median round of each of {a.runs} runs.\n\n" + '\n'.join(rows) + f"\n\nThe tick (f16x3, smooth 0.6): {a.steps} ticks a pass after "
                    f"{a.warmup} untimed, two passes of each route alternated.\n\n" + '\n'.join(more) + '\n')


if __name__ == '__main__':
    main()
