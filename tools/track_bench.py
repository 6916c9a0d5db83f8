#!/usr/bin/env python3
"""Head identities across frames on the device, measured against the only route there was before it.  Prints ONE JSON line.

usage: track_bench.py [--cases 1x1x4,8x1x16,1x64x16] [--max-det 300] [--slots 16] [--steps 20] [--warmup 3] [--rounds 3] [--motion]

Workload: per case Q x T x heads, Q sequences of T frames with `heads` people each, drifting a few pixels a frame and listed in a random order,
as detect_heads leaves them in device memory: boxes [Q, T, max_det, 4] and counts [Q, T].  The state carries over from call to call, so after
the first call every head is matched -- the steady state of a live stream.  Two ways, alternated --rounds times, each round = --warmup untimed
calls, then --steps calls bracketed by synchronize:
  device:  DevicePipeline.track_heads (mcg_track_heads: one launch, one workgroup per sequence, nothing read back);
  host:    what a caller could do before -- read boxes and counts back, run track_heads_host, upload the tables.  HOST-BOUND: a read-back that
           waits for the device, python loops and an upload, so its time is not the arithmetic's and the ratio is that of this comparison only.
--motion adds a third way, alternated with the others in the same run:
  motion:  DevicePipeline.track_heads(motion=True) (mcg_track_heads_motion: the same launch with the constant-velocity model), on a state of its
           own, its tables compared once with track_heads_host(motion=True).  The plain entry is its yardstick.
Reported per case and way: ms per call of every round and the median; the ways' tables are compared once."""
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


def walkers(rs, Q, T, heads, D):
    """Heads on a grid 120 pixels apart, 60 pixels a side, each wandering at most 2 pixels a frame around its place: a call that follows another
    finds every head where its slot left it."""
    boxes = np.zeros((Q, T, D, 4), np.float32)
    home = np.stack([(np.arange(heads) % 8) * 120.0, (np.arange(heads) // 8) * 120.0], axis=1)
    for q in range(Q):
        for t in range(T):
            at = home[rs.permutation(heads)] + rs.uniform(-2, 2, (heads, 2))
            boxes[q, t, :heads] = np.concatenate([at, at + 60.0], axis=1)
    return boxes, np.full((Q, T), heads, np.int32)


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
    ap.add_argument('--cases', default='1x1x4,8x1x16,1x64x16')
    ap.add_argument('--max-det', type=int, default=300)
    ap.add_argument('--slots', type=int, default=16)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--motion', action='store_true', help='also time mcg_track_heads_motion (gain 0.5, decay 1) beside the plain entry')
    a = ap.parse_args()
    dev = 'cuda:0'
    rs = np.random.RandomState(7)
    pipe = P.DevicePipeline(CHAIN)
    opts = dict(slots=a.slots, match_iou=0.3, max_age=5)
    cases = []
    for case in a.cases.split(','):
        Q, T, heads = (int(v) for v in case.split('x'))
        host_boxes, host_counts = walkers(rs, Q, T, heads, a.max_det)
        boxes, counts = torch.from_numpy(host_boxes).to(dev), torch.from_numpy(host_counts).to(dev)
        states = dict(device=torch.zeros(Q, P.track_state_words(a.slots), dtype=torch.int32, device=dev), host=None)
        states['motion'] = torch.zeros_like(states['device'])

        def device():
            return pipe.track_heads(boxes, counts, state=states['device'], **opts)

        def host():
            out = P.track_heads_host(boxes.cpu().numpy(), counts.cpu().numpy(), state=states['host'], **opts)
            states['host'] = out[6]
            return tuple(torch.from_numpy(t).to(dev) for t in out)

        def motion():
            return pipe.track_heads(boxes, counts, state=states['motion'], motion=True, **opts)

        got, old = device(), host()
        torch.cuda.synchronize()
        equal = all(bool(torch.equal(g, o)) for g, o in zip(got, old))
        matched = int((got[1] >= 0).sum())
        ways = dict(device=device, host=host)
        if a.motion:
            moved = motion()
            torch.cuda.synchronize()
            twin = P.track_heads_host(host_boxes, host_counts, motion=True, **opts)
            equal = equal and all(np.array_equal(g.cpu().numpy().view(np.int32), np.ascontiguousarray(o).view(np.int32)) for g, o in zip(moved, twin))
            ways['motion'] = motion
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                ms[k].append(timed(fn, a.steps, a.warmup))
        cases.append(dict(sequences=Q, frames=T, heads=heads, matched_rows=matched, tables_equal=equal,
                          ways={k: dict(ms=[round(v, 4) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 4)) for k in ways}))
    print(json.dumps(dict(tool='track_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                          max_det=a.max_det, steps=a.steps, warmup=a.warmup, rounds=a.rounds, host_route='host-bound: read-back, python, upload', **opts, cases=cases)))


if __name__ == '__main__':
    main()
