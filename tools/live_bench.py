#!/usr/bin/env python3
"""Live multi-person gaze: the fixed-schedule route (live.LiveGaze), the lanes route (live.LiveGaze(lanes=P)) and the read-back route, ms
per tick at steady state.  Prints ONE JSON line; --out also writes the note profiles/live_lanes_<build id>.md holds.

usage: live_bench.py [--cases 1x8x3,4x16x6,8x8x3] [--precisions f16x3,f16] [--steps 20] [--warmup 16] [--rounds 3] [--smooth 0.6] [--out FILE]

Workload: per case Q x S x people, Q cameras of 720 x 1280 BGR frames in device memory with `people` heads each, wandering a few pixels a tick
and listed as detect_heads leaves them (boxes [Q, max_det, 4], counts [Q] on the device); crops are 448 x 448 (the L2CS chain), clip 7 /
stride 4, synthetic weights.  Three routes, alternated --rounds times, each round = --warmup untimed ticks (windows are being decoded and
frames returned by then), then --steps ticks bracketed by synchronize:
  fixed:     LiveGaze.tick -- every one of the Q x S slots is a pool stream and gets a crop every tick; nothing is read back.
             Trunk frames per tick: Q x S.
  lanes:     LiveGaze(lanes=P).tick -- the occupied slots compacted on the device into P pool streams, P = the people present over all
             cameras rounded up to a multiple of 8 (--lane-multiple); nothing is read back.  Trunk frames per tick: P.
  readback:  written here only: track_heads, then track_id, det_of and the slot boxes are copied to the host (ONE wait for the device per
             tick, in front of the trunk), head_crops cuts the matched heads only, and pool streams are opened, pushed and closed per track.
             Trunk frames per tick: Q x people.
All pools run merge='device', results='device' and the same smoothing.  The ratios are those of this comparison only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mcgaze_amd import lib, synth  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from mcgaze_amd.engine import HipEngine  # noqa: E402
from mcgaze_amd.live import LiveGaze  # noqa: E402
from mcgaze_amd.stream import GazeStreamPool  # noqa: E402

CHAIN = [dict(type='LoadImageFromFile'), dict(type='Resize', img_scale=(448, 448), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.0),
         dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True), dict(type='Pad', size_divisor=32),
         dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img'])]
FRAME_H, FRAME_W, MAX_DET, CLIP, STRIDE = 720, 1280, 32, 7, 4
DEV = 'cuda:0'


def walkers(rs, Q, ticks, people):
    """people heads per camera on a grid 150 pixels apart, 90 pixels a side, each wandering at most 2 pixels a tick: always matched."""
    boxes = np.zeros((ticks, Q, MAX_DET, 4), np.float32)
    home = np.stack([40 + (np.arange(people) % 8) * 150.0, 40 + (np.arange(people) // 8) * 150.0], axis=1)
    for t in range(ticks):
        for q in range(Q):
            at = home + rs.uniform(-2, 2, (people, 2))
            boxes[t, q, :people] = np.concatenate([at, at + 90.0], axis=1)
    return boxes, np.full((ticks, Q), people, np.int32)


class ReadBack:
    """The read-back route: who is where is read back every tick, and the pool's streams follow the tracks."""

    def __init__(self, engine, pipe, Q, S, smooth, max_windows):
        self.pipe, self.Q, self.S = pipe, Q, S
        self.pool = GazeStreamPool(engine, 448, 448, CLIP, STRIDE, rows=Q * S * (CLIP + STRIDE + 1), max_decode_windows=max_windows,
                                   max_trunk_frames=max(448, Q * S), merge='device', results='device', smooth=smooth)
        self.state = torch.zeros(Q, P.track_state_words(S), dtype=torch.int32, device=DEV)
        self.sid = {}                                            # (camera, track id) -> stream
        self.trunk_frames = 0

    def tick(self, frames, boxes, counts):
        out = self.pipe.track_heads(boxes[:, None], counts[:, None], state=self.state, slots=self.S, match_iou=0.3, max_age=5, device=DEV)
        words = torch.cat([out[0].view(torch.int32).reshape(self.Q, self.S, 4), out[2].reshape(self.Q, self.S, 1), out[4].reshape(self.Q, self.S, 1)],
                          dim=2).cpu().numpy()                   # the wait for the device
        hit = np.argwhere(words[..., 5] >= 0)
        keys = [(int(q), int(words[q, s, 4])) for q, s in hit]
        for key in [k for k in self.sid if k not in keys]:       # a track that was not matched in this tick ends
            self.pool.close(self.sid.pop(key))
        if len(hit):
            crop_boxes = np.ascontiguousarray(words[hit[:, 0], hit[:, 1], :4]).view(np.float32)
            img, img_hw, _, _, _ = self.pipe.head_crops(frames, crop_boxes, hit[:, 0].astype(np.int32), device=DEV)
            for j, key in enumerate(keys):
                if key not in self.sid:
                    self.sid[key] = self.pool.open()
                self.pool.push(self.sid[key], img[j:j + 1], img_hw[j:j + 1])
            self.trunk_frames += len(keys)
        return self.pool.step()


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='1x8x3,4x16x6,8x8x3')
    ap.add_argument('--precisions', default='f16x3,f16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--smooth', type=float, default=0.6)
    ap.add_argument('--lane-multiple', type=int, default=8)
    ap.add_argument('--out')
    a = ap.parse_args()
    rs = np.random.RandomState(11)
    sd = synth.make_state_dict(0)
    results = []
    for precision in a.precisions.split(','):
        engine = HipEngine(sd, precision=precision)
        max_windows = 12 if precision == 'f16' else None         # the fp16 decoder keeps its bits below 256 tokens per call
        for case in a.cases.split(','):
            Q, S, people = (int(v) for v in case.split('x'))
            ticks = a.rounds * (a.warmup + a.steps)
            host_boxes, host_counts = walkers(rs, Q, ticks, people)
            boxes, counts = torch.from_numpy(host_boxes).to(DEV), torch.from_numpy(host_counts).to(DEV)
            frames = [torch.randint(0, 256, (FRAME_H, FRAME_W, 3), dtype=torch.uint8, device=DEV) for _ in range(Q)]
            pipe = P.DevicePipeline(CHAIN)
            lanes = -(-Q * people // a.lane_multiple) * a.lane_multiple
            options = dict(cameras=Q, slots=S, clip_len=CLIP, stride=STRIDE, smooth=a.smooth, max_decode_windows=max_windows)
            routes = dict(fixed=LiveGaze(engine, pipe, **options), lanes=LiveGaze(engine, pipe, lanes=lanes, **options),
                          readback=ReadBack(engine, pipe, Q, S, a.smooth, max_windows))
            at = {k: 0 for k in routes}

            def step(name):
                t = at[name]
                routes[name].tick(frames, boxes[t], counts[t])
                at[name] = t + 1

            ms = {k: [] for k in routes}
            for _ in range(a.rounds):
                for name in routes:
                    for _ in range(a.warmup):
                        step(name)
                    ms[name].append(timed(lambda: step(name), a.steps))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            results.append(dict(precision=precision, cameras=Q, slots=S, people=people, lanes=lanes,
                                trunk_frames_per_tick=dict(fixed=Q * S, lanes=lanes, readback=routes['readback'].trunk_frames / at['readback']),
                                ms={k: [round(v, 3) for v in ms[k]] for k in ms}, median_ms={k: round(v, 3) for k, v in med.items()},
                                fixed_over_readback=round(med['fixed'] / med['readback'], 3), lanes_over_fixed=round(med['lanes'] / med['fixed'], 3),
                                lanes_over_readback=round(med['lanes'] / med['readback'], 3), fastest=min(med, key=med.get)))
            del routes
            torch.cuda.empty_cache()
    line = dict(tool='live_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                frame=[FRAME_H, FRAME_W], crop=448, clip_len=CLIP, stride=STRIDE, smooth=a.smooth, steps=a.steps, warmup=a.warmup, rounds=a.rounds,
                cases=results)
    print(json.dumps(line))
    if a.out:
        rows = ['| precision | Q x S, people | trunk frames / tick: fixed, lanes, read-back | fixed ms / tick (rounds) | lanes ms / tick (rounds) | '
                'read-back ms / tick (rounds) | lanes / fixed | lanes / read-back | fixed / read-back | fastest |', '|---|---|---|---|---|---|---|---|---|---|']
        cell = lambda r, k: f"{r['median_ms'][k]} ({', '.join(str(v) for v in r['ms'][k])})"
        for r in results:
            rows.append(f"| {r['precision']} | {r['cameras']} x {r['slots']}, {r['people']} | {r['trunk_frames_per_tick']['fixed']}, "
                        f"{r['trunk_frames_per_tick']['lanes']}, {r['trunk_frames_per_tick']['readback']:.1f} | {cell(r, 'fixed')} | {cell(r, 'lanes')} | "
                        f"{cell(r, 'readback')} | {r['lanes_over_fixed']} | {r['lanes_over_readback']} | {r['fixed_over_readback']} | {r['fastest']} |")
        with open(a.out, 'a') as f:
            f.write(f"\n## Run on {line['device']} ({line['arch']}), build {line['build_id']}\n\n{a.steps} ticks a round after {a.warmup} untimed, "
                    f"{a.rounds} rounds alternated, medians; smooth = {a.smooth}.\n\n" + '\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
