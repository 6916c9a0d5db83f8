#!/usr/bin/env python3
"""What ragged batches cost and what they buy, measured.  Prints ONE JSON line.

usage: ragged_bench.py [--clips 64] [--clip-length 7] [--side 224] [--precision f16x3] [--steps 100] [--warmup 10] [--rounds 5]
                       [--tracks 64] [--max-track 10] [--seed 7]

  * uniform: `--clips` clips of `--clip-length` frames through the two-deep batch pipeline (engine.PipelinedRunner: the schedule bench.py
    times) with clip_length = T (mcg_*_forward) and with clip_length = [T] * clips (mcg_*_ragged), ALTERNATED --rounds times each on one
    engine; a round = --warmup untimed steps, then --steps steps bracketed by synchronize, as bench.py times its headline.  Reported:
    ms per step of every round, median, and the spread (max - min) of each entry's own rounds -- the ragged entry is "not taxed" when its
    median lies inside the fixed entry's spread.  The same for serial engine.forward calls;
  * crowd: `--tracks` tracks with lengths drawn uniformly from 1 .. `--max-track` (fixed --seed), once as ONE ragged forward and once as
    one forward per distinct length (what a caller could do before: equal lengths only), alternated --rounds times; ms per pass;
  * the library build id."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mcgaze_amd import lib, synth  # noqa: E402
from mcgaze_amd.engine import HipEngine, PipelinedRunner  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(max(warmup, 1)):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def stats(ms):
    return dict(ms=[round(v, 4) for v in ms], median_ms=round(float(np.median(ms)), 4), spread_ms=round(max(ms) - min(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--clip-length', type=int, default=7)
    ap.add_argument('--side', type=int, default=224)
    ap.add_argument('--precision', default='f16x3')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--tracks', type=int, default=64)
    ap.add_argument('--max-track', type=int, default=10)
    ap.add_argument('--seed', type=int, default=7)
    a = ap.parse_args()
    dev = 'cuda:0'
    e = HipEngine(synth.make_state_dict(0), precision=a.precision, device=dev)
    B, T = a.clips, a.clip_length
    N = B * T
    x = torch.from_numpy(synth.make_clips(1234, B, T, a.side, a.side)).to(dev)
    out = dict(gaze=torch.empty(4, N, 3, device=dev), boxes=torch.empty(N, 3, 4, device=dev), scores=torch.empty(N, 3, device=dev))

    # ---- uniform lengths through both entries
    entries = {'fixed': T, 'ragged': [T] * B}
    runners = {k: PipelinedRunner(e, N, a.side, a.side, v) for k, v in entries.items()}
    ref = {k: {n: t.clone() for n, t in e.forward(x, v).items()} for k, v in entries.items()}
    same = all(torch.equal(ref['fixed'][n], ref['ragged'][n]) for n in ref['fixed'])
    pipe, serial = {k: [] for k in entries}, {k: [] for k in entries}
    for _ in range(a.rounds):
        for k in entries:
            r = runners[k]
            with torch.cuda.stream(r.sa):              # the loop submits from the pipeline's trunk stream, like bench.py's
                pipe[k].append(timed(lambda: r.submit(x, out), a.steps, a.warmup))
                r.flush()
        for k, v in entries.items():
            serial[k].append(timed(lambda: e.forward(x, v, out=out), max(a.steps // 4, 1), 2))
    uniform = dict(clips=B, clip_length=T, frames=N, bits_equal=same, pipelined={k: stats(v) for k, v in pipe.items()},
                   serial={k: stats(v) for k, v in serial.items()})
    for sched in ('pipelined', 'serial'):
        f, r = uniform[sched]['fixed'], uniform[sched]['ragged']
        uniform[sched]['ragged_minus_fixed_ms'] = round(r['median_ms'] - f['median_ms'], 4)
        uniform[sched]['ragged_inside_fixed_spread'] = bool(min(f['ms']) <= r['median_ms'] <= max(f['ms']))

    # ---- a crowd: tracks of 1 .. max_track frames
    rs = np.random.RandomState(a.seed)
    lengths = rs.randint(1, a.max_track + 1, a.tracks).tolist()
    M = sum(lengths)
    y = torch.from_numpy(synth.make_clips(4321, 1, M, a.side, a.side)).to(dev)
    start = np.concatenate([[0], np.cumsum(lengths)])
    by_len = {}
    for i, n in enumerate(lengths):
        by_len.setdefault(n, []).append(i)
    groups = {n: torch.cat([y[start[i]:start[i + 1]] for i in idx]).contiguous() for n, idx in sorted(by_len.items())}

    def one_call():
        e.forward(y, lengths)

    def per_length():
        for n, g in groups.items():
            e.forward(g, n)
    crowd_ms = {'one_ragged_call': [], 'one_call_per_length': []}
    for _ in range(a.rounds):
        crowd_ms['one_ragged_call'].append(timed(one_call, max(a.steps // 4, 1), 2))
        crowd_ms['one_call_per_length'].append(timed(per_length, max(a.steps // 4, 1), 2))
    crowd = dict(tracks=a.tracks, frames=M, lengths=lengths, distinct_lengths=len(groups), **{k: stats(v) for k, v in crowd_ms.items()})
    crowd['speedup'] = round(crowd['one_call_per_length']['median_ms'] / crowd['one_ragged_call']['median_ms'], 3)

    print(json.dumps(dict(tool='ragged_bench', build_id=lib.build_id(), precision=a.precision, side=a.side, steps=a.steps, warmup=a.warmup,
                          rounds=a.rounds, uniform=uniform, crowd=crowd)))


if __name__ == '__main__':
    main()
