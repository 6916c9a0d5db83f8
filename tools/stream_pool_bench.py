"""GPU tool (a measurement, not a test): S live streams, one new 224 x 224 frame per stream per tick -- S lone GazeStream objects (S trunk calls
and up to S decoder calls per tick: the only live API before GazeStreamPool, so this leg is the baseline) against ONE GazeStreamPool (one
trunk call + one scatter, one decoder call).  Reports ms per tick of both legs (warmed up, legs alternated, --runs runs each, host clock
around ticks that end with the results on the host), checks that the two legs' outputs are bit-equal, and times the row scatter against
the trunk call it follows (HIP events; engine.profile records contraction launches only, and the scatter is none).

Usage: python tools/stream_pool_bench.py --streams 1,8,64 --ticks 16 --precision f16x3,f16 [--out profiles/stream_pool_<build id>.md]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mcgaze_amd import lib as L, synth
from mcgaze_amd.engine import HipEngine
from mcgaze_amd.stream import GazeStream, GazeStreamPool

H = W = 224
CLIP, STRIDE = 7, 4
WARM = 12          # ticks before the timed window: past every stream's first window and one full stride of steady state


def frame(base, stream, tick):
    return base[(3 * tick + stream) % base.shape[0]][None]


def cat(parts):
    return [np.concatenate([p[k] for p in parts]) for k in ('det', 'fused', 'others')]


def run_lone(e, base, S, ticks, limit):
    streams = [GazeStream(e, H, W, CLIP, STRIDE, capacity=CLIP + STRIDE + 1, max_decode_windows=limit) for _ in range(S)]
    parts = [[] for _ in range(S)]
    t0 = None
    for t in range(WARM + ticks):
        if t == WARM:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for i, s in enumerate(streams):
            parts[i].append(s.push(frame(base, i, t)))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / ticks
    for i, s in enumerate(streams):
        parts[i].append(s.finish())
    return ms, [cat(p) for p in parts]


def run_pool(e, base, S, ticks, limit):
    pool = GazeStreamPool(e, H, W, CLIP, STRIDE, rows=S * (CLIP + STRIDE + 1), max_decode_windows=limit)
    sids = [pool.open() for _ in range(S)]
    parts = {s: [] for s in sids}
    t0 = None

    def step():
        for s, r in pool.step().items():
            parts[s].append(r)
    for t in range(WARM + ticks):
        if t == WARM:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for i, s in enumerate(sids):
            pool.push(s, frame(base, i, t))
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / ticks
    for s in sids:
        pool.close(s)
    while pool.pending():
        step()
    return ms, [cat(parts[s]) for s in sids]


def scatter_share(e, base, S, reps=20):
    """-> (ms of the trunk call over S frames into the scratch pyramid, ms of the scatter of those S frames), medians over reps."""
    x = base[torch.arange(S) % base.shape[0]].contiguous()
    store = [torch.empty(S + 3, (H // 4) >> i, (W // 4) >> i, 256, dtype=e.dtype, device=e.device) for i in range(4)]
    rows = [int(r) for r in np.random.RandomState(0).permutation(S + 3)[:S]]
    src = e.backbone_fpn(x)
    table = torch.tensor(rows, dtype=torch.int32, device=e.device)
    sp = (C.c_void_p * 4)(*[t.data_ptr() for t in src])
    dp = (C.c_void_p * 4)(*[t.data_ptr() for t in store])
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    trunk, copy = [], []
    for r in range(reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        e.backbone_fpn(x, out=src)
        ev[1].record()
        L.check(e.lib.mcg_pyramid_scatter_rows(stream(), e.code, sp, dp, S, S + 3, H, W, C.c_void_p(table.data_ptr())), 'mcg_pyramid_scatter_rows')
        ev[2].record()
        torch.cuda.synchronize()
        if r >= 3:
            trunk.append(ev[0].elapsed_time(ev[1]))
            copy.append(ev[1].elapsed_time(ev[2]))
    return float(np.median(trunk)), float(np.median(copy))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', default='1,8,64')
    ap.add_argument('--ticks', type=int, default=16)
    ap.add_argument('--precision', default='f16x3,f16')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stream_pool_bench needs a HIP device: a time taken anywhere else says nothing')
    base = torch.from_numpy(synth.make_clips(7, 1, 32, H, W)).to('cuda:0')
    sd = synth.make_state_dict(0)
    differ = False
    lines = [f'# Many live streams: S lone GazeStream objects against one GazeStreamPool (build {L.build_id()})', '',
             f'{torch.cuda.get_device_name(0)}; one {H} x {W} frame per stream per tick, clip_len {CLIP}, stride {STRIDE}; {a.ticks} timed ticks after {WARM} '
             f'warm-up ticks; legs alternated, {a.runs} runs each, every run listed (their range is the run-to-run spread); ms per tick, host clock, results '
             'on the host at the end of every tick.  scatter / trunk: HIP-event medians of mcg_pyramid_scatter_rows and of the trunk call over the same S frames.', '',
             '| precision | S | lone ms/tick (runs) | pool ms/tick (runs) | lone / pool (medians) | bit-equal | trunk ms | scatter ms | scatter share |',
             '|---|---|---|---|---|---|---|---|---|']
    for prec in a.precision.split(','):
        e = HipEngine(sd, precision=prec)
        limit = 12 if prec in ('f16', 'fp16') else None     # the fp16 decoder keeps its bits below 256 tokens per call
        for S in (int(s) for s in a.streams.split(',')):
            lone, pool, same = [], [], True
            for r in range(a.runs):
                ms_l, out_l = run_lone(e, base, S, a.ticks, limit)
                ms_p, out_p = run_pool(e, base, S, a.ticks, limit)
                lone.append(ms_l)
                pool.append(ms_p)
                same = same and all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
                                    for sl, sp in zip(out_l, out_p) for x, y in zip(sl, sp))
            tr, sc = scatter_share(e, base, S)
            fmt = lambda v: ' '.join(f'{x:.3f}' for x in v)
            lines.append(f'| {prec} | {S} | {fmt(lone)} | {fmt(pool)} | {np.median(lone) / np.median(pool):.2f} | {"yes" if same else "NO"} | {tr:.3f} | {sc:.4f} | '
                         f'{100 * sc / (tr + sc):.2f} % |')
            print(lines[-1], flush=True)
            if not same:
                differ = True
                print(f'{prec} S={S}: the two legs DIFFER', flush=True)
        del e
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main())
