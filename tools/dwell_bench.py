#!/usr/bin/env python3
"""Gaze dwell: the device call against the only route there was before it, and what LiveGaze(dwell=True) adds to a tick.  Prints ONE JSON
line; --out also appends the note profiles/dwell_<build id>.md holds.

usage: dwell_bench.py [--shapes 1x8,1x64,1x1024,64x1024] [--regions 16] [--calls 20] [--rounds 3] [--runs 2] [--live 1x8x3,4x16x6] [--steps 20]
                      [--warmup 16] [--out FILE]

1. The call.  Per shape F x R: F frames of R columns; persons that change rarely, targets from a small alphabet that flicker (so episodes
   form, end and are replaced), --regions regions; every table, the state and the totals in device memory, the state carried from call to
   call.
     device:    DevicePipeline.gaze_dwell on the device tables (mcg_gaze_dwell: two launches, nothing read back), Python layer included.
     readback:  the route before: the five tables, the state and the totals copied to the host, attention.gaze_dwell_host, the six results
                uploaded.
   --runs times: --rounds rounds alternated, each --calls calls bracketed by synchronize; the median round of each run, us per call.
2. The tick.  tools/live_bench.py's shapes and walkers: LiveGaze.tick with attention=True, without and with dwell=True in ONE process, two
   passes of each alternated, each --warmup untimed ticks then --steps timed; ms per tick per pass, the difference of the means, and the
   no-dwell route's own spread between its two passes to set it against.
The ratios are those of this comparison only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from live_bench import CHAIN, CLIP, DEV, FRAME_H, FRAME_W, STRIDE, timed, walkers  # noqa: E402
from mcgaze_amd import lib, synth  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from mcgaze_amd.attention import gaze_dwell_host  # noqa: E402
from mcgaze_amd.engine import HipEngine  # noqa: E402
from mcgaze_amd.live import LiveGaze  # noqa: E402


def tables(rs, F, R, m):
    """person, kind, ident, mutual, tag [F, R] int32: sticky over the frames, so that looks last and flicker."""
    def sticky(values, keep):
        cur = rs.randint(0, values, R)
        out = np.empty((F, R), np.int32)
        for f in range(F):
            cur = np.where(rs.random_sample(R) < keep, cur, rs.randint(0, values, R))
            out[f] = cur
        return out

    person = sticky(4, 0.98) + np.arange(R, dtype=np.int32)[None] * 4
    target = sticky(8, 0.8)
    kind = np.asarray([0, 1, 1, 2, 2, 2, 3, 0], np.int32)[target]
    ident = np.where(kind == 2, target % max(m, 1), target).astype(np.int32)
    return person, kind, ident, rs.randint(0, 2, (F, R)).astype(np.int32), sticky(2, 0.99)


def bench_call(pipe, shape, m, calls, rounds, runs, rs):
    F, R = shape
    dev = [torch.from_numpy(t).to(DEV) for t in tables(rs, F, R, m)]
    state = {k: pipe.dwell_state(R, device=DEV) for k in ('device', 'readback', 'check')}
    totals = {k: torch.zeros(m, dtype=torch.int32, device=DEV) for k in state}

    def device(key='device'):
        return pipe.gaze_dwell(*dev[:4], tag=dev[4], state=state[key], region_frames=totals[key], device=DEV)

    def readback(key='readback'):
        host = gaze_dwell_host(*(t.cpu().numpy() for t in dev[:4]), tag=dev[4].cpu().numpy(), state=state[key].cpu().numpy(),
                               region_frames=totals[key].cpu().numpy())
        out = tuple(torch.from_numpy(t).to(DEV) for t in host)
        state[key].copy_(out[4])
        totals[key].copy_(out[5])
        return out

    same = all(torch.equal(a, b) for a, b in zip(device('check'), readback('readback')))
    state['readback'].zero_()
    totals['readback'].zero_()
    out = dict(frames=F, columns=R, regions=m, equal=bool(same), us=dict(device=[], readback=[]))
    for _ in range(runs):
        us = dict(device=[], readback=[])
        for _ in range(rounds):
            for name, fn in (('device', device), ('readback', readback)):
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
    options = dict(cameras=Q, slots=S, clip_len=CLIP, stride=STRIDE, smooth=0.6, attention=True)
    routes = dict(plain=LiveGaze(engine, pipe, **options), dwell=LiveGaze(engine, pipe, dwell=True, **options))
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
    return dict(cameras=Q, slots=S, people=people, columns=Q * S, ms=ms, added_ms=round(mean['dwell'] - mean['plain'], 4),
                plain_spread_ms=round(abs(ms['plain'][0] - ms['plain'][1]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1x8,1x64,1x1024,64x1024')
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
    line = dict(tool='dwell_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                calls_per_round=a.calls, rounds=a.rounds, runs=a.runs, steps=a.steps, warmup=a.warmup, call=calls, tick=ticks)
    print(json.dumps(line))
    if a.out:
        rows = ['| frames x columns, regions | device us / call (runs) | read-back us / call (runs) | read-back / device | equal |', '|---|---|---|---|---|']
        for c in calls:
            rows.append(f"| {c['frames']} x {c['columns']}, {c['regions']} | {c['us']['device']} | {c['us']['readback']} | {c['readback_over_device']} | {c['equal']} |")
        more = ['| Q x S, people | columns | attention ms / tick (passes) | attention + dwell ms / tick (passes) | added ms | no-dwell: spread between its passes |',
                '|---|---|---|---|---|---|']
        for t in ticks:
            more.append(f"| {t['cameras']} x {t['slots']}, {t['people']} | {t['columns']} | {t['ms']['plain']} | {t['ms']['dwell']} | {t['added_ms']} | "
                        f"{t['plain_spread_ms']} |")
        with open(a.out, 'a') as f:
            f.write(f"\n## Run on {line['device']} ({line['arch']}), build {line['build_id']}\n\nThe call: {a.calls} calls a round, {a.rounds} rounds alternated, "
                    f"the median round of each of {a.runs} runs.\n\n" + '\n'.join(rows) + f"\n\nThe tick (f16x3, smooth 0.6, attention=True): {a.steps} ticks a pass "
                    f"after {a.warmup} untimed, two passes of each route alternated.\n\n" + '\n'.join(more) + '\n')


if __name__ == '__main__':
    main()
