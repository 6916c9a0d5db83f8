"""GPU tool (a measurement, not a test): what the temporal filter (``smooth=``) adds to a tick of a GazeStreamPool whose results stay on
the device.  S live streams, one new 224 x 224 frame per stream per tick (the protocol of tools/device_merge_bench.py), every leg with
merge='device', results='device' -- a tick never waits for the device:

  plain   smooth=None: the yardstick, the tick as it was
  kernel  smooth=0.6: one mcg_smooth_gaze launch per tick over all streams, every frame one frame late
  torch   smooth=None, and the same filter done by the consumer with torch ops on the device tensors the pool returned: per stream it
          keeps the last row handed out and the newest row, and filters what lies between (about nine small launches per stream per tick)

Reports ms per tick of the three legs (warmed up, legs alternated, --runs runs each, every run listed; host clock, the device drained at
the end of the timed window), the time the two filtering legs add to the plain tick, whether kernel and torch legs agree (the torch leg's
norm is torch's own, so it may differ from the kernel's by its rounding of the sum of squares: the largest difference in ulp is listed),
and times mcg_smooth_gaze alone on one tick's table (S interior frames; HIP events, median).

Usage: python tools/smooth_bench.py --streams 1,8,64 --ticks 16 --precision f16x3 [--out profiles/smooth_<build id>.md]"""
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
from mcgaze_amd.stream import GazeStreamPool

H = W = 224
CLIP, STRIDE = 7, 4
ALPHA = 0.6
WARM = 12          # ticks before the timed window: past every stream's first window and one full stride of steady state
LEGS = ('plain', 'kernel', 'torch')


def frame(base, stream, tick):
    return base[(3 * tick + stream) % base.shape[0]][None]


class TorchSmoother:
    """smooth_filter (tools/calculate_mae_gaze360.py:16-29) on a growing stream with torch ops on the device: what a consumer of
    results='device' has to write without the option.  One frame late, like the kernel leg."""

    def __init__(self):
        self.rows = None         # [prev handed out (if any)] + the frames not handed out yet, [m,4,3]
        self.lead = False

    def push(self, fused, others, ended=False):
        g = torch.cat([fused[:, None], others], dim=1)
        g = g if self.rows is None else torch.cat([self.rows, g])
        m = g.shape[0]
        lo, hi = int(self.lead), m if ended else m - 1
        if hi <= lo:
            self.rows = g
            return g[:0]
        if m == 1:
            return g
        out = ALPHA * g[lo:hi]
        at = 0
        if lo == 0:
            out[0] += (1 - ALPHA) * g[1]
            at = 1
        end = hi
        if hi == m:
            out[-1] += (1 - ALPHA) * g[-2]
            end = m - 1
        if end > lo + at:
            out[at:end - lo] += (1 - ALPHA) * (g[lo + at - 1:end - 1] + g[lo + at + 1:end + 1]) / 2
        self.rows, self.lead = g[hi - 1:], True
        return out / torch.norm(out, dim=2).unsqueeze(2)


def run_pool(e, base, S, ticks, limit, leg):
    pool = GazeStreamPool(e, H, W, CLIP, STRIDE, rows=S * (CLIP + STRIDE + 1), max_decode_windows=limit, merge='device', results='device',
                          smooth=ALPHA if leg == 'kernel' else None)
    sids = [pool.open() for _ in range(S)]
    parts = {s: [] for s in sids}
    filt = {s: TorchSmoother() for s in sids} if leg == 'torch' else None
    closing = set()
    t0 = None

    def step():
        for s, r in pool.step().items():
            if leg == 'kernel':
                parts[s].append(torch.cat([r['fused_smooth'][:, None], r['others_smooth']], dim=1))
            elif leg == 'torch':
                parts[s].append(filt[s].push(r['fused'], r['others'], ended=s in closing))
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
        closing.add(s)
    while pool.pending():
        step()
    return ms, [torch.cat(parts[s]).cpu().numpy() if parts[s] else None for s in sids]


def ulp_apart(a, b):
    o = lambda x: (lambda i: np.where(i < 0, -(i & 0x7fffffff), i))(np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64))
    return int(np.abs(o(a) - o(b)).max()) if a.size else 0


def kernel_ms(S, reps=50):
    """mcg_smooth_gaze on one tick's table at steady state: S streams, one interior frame each.  -> median ms over reps (HIP events
    around the launch alone; the table is already on the device)."""
    dev = 'cuda:0'
    store = torch.randn(3 * S, 27, device=dev)
    plan = torch.arange(3 * S, dtype=torch.int32, device=dev).reshape(S, 3).contiguous()
    out = torch.empty(S, 12, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    lib, ms = L.load(), []
    for r in range(reps + 5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        L.check(lib.mcg_smooth_gaze(C.c_void_p(torch.cuda.current_stream().cuda_stream), p(store), store.shape[0], p(plan), S, ALPHA, p(out)), 'mcg_smooth_gaze')
        ev[1].record()
        torch.cuda.synchronize()
        if r >= 5:
            ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', default='1,8,64')
    ap.add_argument('--ticks', type=int, default=16)
    ap.add_argument('--precision', default='f16x3')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('smooth_bench needs a HIP device: a time taken anywhere else says nothing')
    base = torch.from_numpy(synth.make_clips(7, 1, 32, H, W)).to('cuda:0')
    sd = synth.make_state_dict(0)
    lines = [f'# The temporal filter of a GazeStreamPool: none, mcg_smooth_gaze, torch ops on the returned tensors (build {L.build_id()})', '',
             f"{torch.cuda.get_device_name(0)}; one {H} x {W} frame per stream per tick, clip_len {CLIP}, stride {STRIDE}, merge='device', results='device'; "
             f'{a.ticks} timed ticks after {WARM} warm-up ticks; legs alternated, {a.runs} runs each, every run listed (their range is the run-to-run '
             'spread); ms per tick, host clock, the device drained at the end of the timed window.  plain = smooth=None (the yardstick, measured in '
             f'this run); kernel = smooth={ALPHA}; torch = smooth=None and the filter done with torch ops on the returned device tensors.  added: median '
             'minus the plain median of the same run.  max ulp: the largest difference between the kernel leg and the torch leg (torch.norm rounds '
             "the sum of squares its own way).  kernel alone: HIP-event median of mcg_smooth_gaze over one tick's table (S frames).", '',
             '| precision | S | plain ms/tick (runs) | kernel ms/tick (runs) | torch ms/tick (runs) | kernel added ms | torch added ms | max ulp | kernel alone ms |',
             '|---|---|---|---|---|---|---|---|---|']
    for prec in a.precision.split(','):
        e = HipEngine(sd, precision=prec)
        limit = 12 if prec in ('f16', 'fp16') else None     # the fp16 decoder keeps its bits below 256 tokens per call
        for S in (int(s) for s in a.streams.split(',')):
            ms = {name: [] for name in LEGS}
            apart = 0
            for r in range(a.runs):
                outs = {}
                for name in LEGS:
                    t, outs[name] = run_pool(e, base, S, a.ticks, limit, name)
                    ms[name].append(t)
                apart = max([apart] + [ulp_apart(x, y) if x.shape == y.shape else 1 << 31 for x, y in zip(outs['kernel'], outs['torch'])])
            fmt = lambda v: ' '.join(f'{x:.3f}' for x in v)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            lines.append(f"| {prec} | {S} | {fmt(ms['plain'])} | {fmt(ms['kernel'])} | {fmt(ms['torch'])} | {med['kernel'] - med['plain']:+.3f} | "
                         f"{med['torch'] - med['plain']:+.3f} | {apart} | {kernel_ms(S):.4f} |")
            print(lines[-1], flush=True)
        del e
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
