#!/usr/bin/env python3
"""Frame reuse across overlapping windows, measured: harness.run_videos with reuse_frames off and on over synthetic videos, and the
per-push latency of stream.GazeStream.  Prints ONE JSON line.

usage: window_reuse_bench.py [--videos 48] [--frames 100] [--side 224] [--precision f16x3] [--batch-clips 64] [--rounds 3]
                             [--stream-frames 100]

  * videos: synth.make_clips(seed, 1, L), kept on the device (the timed work is the engine's, not the host's frame copies);
  * run_videos off / on alternated --rounds times each after one warm-up of both, each timed by a host clock around work that ends in
    torch.cuda.synchronize(); frames/s = distinct video frames per second, median over the rounds;
  * trunk_frames of both settings (harness.last_run_stats) and whether the records are equal (they must be: == on the record dicts);
  * GazeStream, one frame per push, at stride 4 and at stride 1: per-push latency (host clock around push + synchronize), median / p99;
  * the library build id."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mcgaze_amd import harness, lib, synth  # noqa: E402
from mcgaze_amd.engine import HipEngine  # noqa: E402
from mcgaze_amd.stream import GazeStream  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--videos', type=int, default=48)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--side', type=int, default=224)
    ap.add_argument('--precision', default='f16x3')
    ap.add_argument('--batch-clips', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--stream-frames', type=int, default=100)
    a = ap.parse_args()
    dev = 'cuda:0'
    e = HipEngine(synth.make_state_dict(0), precision=a.precision, device=dev)
    videos = [dict(id=i, frames=torch.from_numpy(synth.make_clips(1000 + i, 1, a.frames, a.side, a.side)).to(dev)) for i in range(a.videos)]
    total = a.videos * a.frames

    def run(reuse):
        return harness.run_videos(e, videos, batch_clips=a.batch_clips, reuse_frames=reuse)

    rec = {}
    trunk = {}
    for reuse in (False, True):                      # warm-up (workspaces, pinned buffers, first-call probes)
        rec[reuse] = run(reuse)
        trunk[reuse] = harness.last_run_stats['trunk_frames']
    times = {False: [], True: []}
    for _ in range(a.rounds):
        for reuse in (False, True):
            dt, _ = timed(lambda: run(reuse))
            times[reuse].append(dt)
    fps = {k: total / float(np.median(v)) for k, v in times.items()}

    lat = {}
    v = videos[0]['frames'][:a.stream_frames]
    for stride in (4, 1):
        for rep in range(2):                         # rep 0: warm-up
            s = GazeStream(e, a.side, a.side, stride=stride)
            ms = []
            for f in range(v.shape[0]):
                dt, _ = timed(lambda: s.push(v[f:f + 1]))
                ms.append(dt * 1e3)
            s.finish()
        lat[stride] = dict(median_ms=round(float(np.median(ms)), 3), p99_ms=round(float(np.percentile(ms, 99)), 3), pushes=len(ms))

    print(json.dumps(dict(
        tool='window_reuse_bench', build_id=lib.build_id(), precision=a.precision, videos=a.videos, frames=a.frames, side=a.side,
        batch_clips=a.batch_clips, rounds=a.rounds,
        run_videos=dict(default_fps=round(fps[False], 1), reuse_fps=round(fps[True], 1), speedup=round(fps[True] / fps[False], 3),
                        default_s=[round(t, 4) for t in times[False]], reuse_s=[round(t, 4) for t in times[True]],
                        trunk_frames_default=trunk[False], trunk_frames_reuse=trunk[True],
                        trunk_ratio=round(trunk[False] / trunk[True], 3), records_equal=rec[False] == rec[True]),
        stream_push_latency={f'stride{k}': d for k, d in lat.items()})))


if __name__ == '__main__':
    main()
