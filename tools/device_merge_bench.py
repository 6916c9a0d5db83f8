"""GPU tool (a measurement, not a test): what the host round trip of the overlap merge costs a GazeStreamPool.  S live streams, one new
224 x 224 frame per stream per tick (the protocol of tools/stream_pool_bench.py), three legs:

  host            merge='host' (the default, the baseline): per decoder call a blocking copy to the host, one numpy merge per window
  device -> host  merge='device', results='host': one mcg_merge_windows launch per decoder call, ONE copy per tick for all streams
  device          merge='device', results='device': the results stay on the device, a tick never waits for it

Reports ms per tick of the three legs (warmed up, legs alternated, --runs runs each, every run listed; host clock, the device drained at
the end of the timed window -- the first two legs also wait for it in every tick, the third does not), checks that the three legs'
outputs are bit-equal, and times mcg_merge_windows alone on the merge of one tick's decoder call (S windows of 7 frames, 3 frames of
each continuing from the store; HIP events, median).

Usage: python tools/device_merge_bench.py --streams 1,8,64 --ticks 16 --precision f16x3,f16 [--out profiles/device_merge_<build id>.md]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from mcgaze_amd import harness, lib as L, synth
from mcgaze_amd.engine import HipEngine
from mcgaze_amd.stream import GazeStreamPool

H = W = 224
CLIP, STRIDE = 7, 4
WARM = 12          # ticks before the timed window: past every stream's first window and one full stride of steady state
LEGS = (('host', {}), ('device -> host', dict(merge='device')), ('device', dict(merge='device', results='device')))


def frame(base, stream, tick):
    return base[(3 * tick + stream) % base.shape[0]][None]


def run_pool(e, base, S, ticks, limit, kw):
    pool = GazeStreamPool(e, H, W, CLIP, STRIDE, rows=S * (CLIP + STRIDE + 1), max_decode_windows=limit, **kw)
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
    return ms, [[np.concatenate([harness._host(p[k]) for p in parts[s]]) for k in ('det', 'fused', 'others')] for s in sids]


def kernel_ms(S, reps=50):
    """mcg_merge_windows on one tick's decoder call at steady state: S streams, one window of CLIP frames each, whose first CLIP - STRIDE
    frames continue from the store.  -> median ms over reps (HIP events around the launch alone; the plan is already on the device)."""
    dev = 'cuda:0'
    n = S * CLIP
    g = torch.randn(4, n, 3, device=dev)
    b = torch.rand(n, 3, 4, device=dev) * 200
    s = torch.rand(n, 3, device=dev)
    scale = torch.tensor([224 / 177, 224 / 199, 224 / 177, 224 / 199], device=dev)
    windows = [(i, (STRIDE, STRIDE + CLIP, CLIP - STRIDE), i * CLIP) for i in range(S)]
    written = {(i, f) for i in range(S) for f in range(STRIDE, CLIP)}
    table, max_src = harness.merge_plan(windows, lambda k, f: k * (CLIP + STRIDE) + f, written, n, S * (CLIP + STRIDE))
    plan = torch.from_numpy(table).to(dev)
    store = torch.zeros(S * (CLIP + STRIDE), 27, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    lib, ms = L.load(), []
    for r in range(reps + 5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        L.check(lib.mcg_merge_windows(C.c_void_p(torch.cuda.current_stream().cuda_stream), p(g), p(b), p(s), n, p(scale), 0, p(plan), table.shape[0], max_src,
                                      p(store), store.shape[0], 0.5), 'mcg_merge_windows')
        ev[1].record()
        torch.cuda.synchronize()
        if r >= 5:
            ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', default='1,8,64')
    ap.add_argument('--ticks', type=int, default=16)
    ap.add_argument('--precision', default='f16x3,f16')
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('device_merge_bench needs a HIP device: a time taken anywhere else says nothing')
    base = torch.from_numpy(synth.make_clips(7, 1, 32, H, W)).to('cuda:0')
    sd = synth.make_state_dict(0)
    differ = False
    lines = [f'# The overlap merge of a GazeStreamPool: on the host, on the device, results left on the device (build {L.build_id()})', '',
             f'{torch.cuda.get_device_name(0)}; one {H} x {W} frame per stream per tick, clip_len {CLIP}, stride {STRIDE}; {a.ticks} timed ticks after {WARM} '
             f'warm-up ticks; legs alternated, {a.runs} runs each, every run listed (their range is the run-to-run spread); ms per tick, host clock, the '
             "device drained at the end of the timed window.  host = merge='host' (the baseline, measured in this run); device -> host = merge='device', "
             "results='host'; device = merge='device', results='device'.  kernel: HIP-event median of mcg_merge_windows alone over one tick's decoder call "
             f'(S windows of {CLIP} frames).', '',
             '| precision | S | host ms/tick (runs) | device -> host ms/tick (runs) | device ms/tick (runs) | host / device -> host | host / device | bit-equal | kernel ms |',
             '|---|---|---|---|---|---|---|---|---|']
    for prec in a.precision.split(','):
        e = HipEngine(sd, precision=prec)
        limit = 12 if prec in ('f16', 'fp16') else None     # the fp16 decoder keeps its bits below 256 tokens per call
        for S in (int(s) for s in a.streams.split(',')):
            ms = {name: [] for name, _ in LEGS}
            same = True
            for r in range(a.runs):
                outs = {}
                for name, kw in LEGS:
                    t, outs[name] = run_pool(e, base, S, a.ticks, limit, kw)
                    ms[name].append(t)
                same = same and all(x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
                                    for name in ('device -> host', 'device') for sa, sb in zip(outs['host'], outs[name]) for x, y in zip(sa, sb))
            fmt = lambda v: ' '.join(f'{x:.3f}' for x in v)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            lines.append(f"| {prec} | {S} | {fmt(ms['host'])} | {fmt(ms['device -> host'])} | {fmt(ms['device'])} | {med['host'] / med['device -> host']:.2f} | "
                         f"{med['host'] / med['device']:.2f} | {'yes' if same else 'NO'} | {kernel_ms(S):.4f} |")
            print(lines[-1], flush=True)
            if not same:
                differ = True
                print(f'{prec} S={S}: the legs DIFFER', flush=True)
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
