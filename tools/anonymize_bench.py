#!/usr/bin/env python3
"""Anonymised heads on the device, measured against a plain device copy of the same frames, against the heat map's dense whole-frame pass
and against the route a caller had before.  Prints ONE JSON line.

usage: anonymize_bench.py [--frames 8] [--heads 8,32,128] [--height 1080] [--width 1920] [--matrix bt709] [--steps 20] [--warmup 3] [--rounds 3]

Workload: `--frames` synthetic frames (random bytes) in device memory, packed BGR and NV12 surfaces; for each count of --heads that many head
boxes of mixed sizes (24 .. 400 pixels a side) spread over the frames.  Every table is a device tensor.  Each way is timed --rounds times,
the ways alternated, each round = --warmup untimed calls, then --steps calls bracketed by synchronize:
  anonymize:  DevicePipeline.anonymize_heads in place, the defaults (ellipse, 8 blocks, mosaic), per head count; fill for the largest count;
  copy:       dst.copy_(src) of the same frames, one launch per frame;  copy_one: ONE copy_ of as many bytes;
  draw_dense: DevicePipeline.draw_heat over a grid with every cell above zero: every pixel of every frame read, blended and written;
  host:       what a caller did before -- every frame read back, arrows.anonymize_heads_host (numpy), every frame copied up again.
              HOST-BOUND, not a GPU figure; timed ONCE per head count, and that call is also the check that both routes give the same bytes.
No target is fixed in advance: the cost is whatever this prints."""
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
from mcgaze_amd import attention as AT  # noqa: E402
from mcgaze_amd import lib  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from draw_bench import CHAIN, timed  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--heads', default='8,32,128')
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--matrix', default='bt709', choices=sorted(P.YUV_COEF))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    dev = 'cuda:0'
    rs = np.random.RandomState(3)
    H, W, F = a.height, a.width, a.frames
    pipe = P.DevicePipeline(CHAIN)
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    summary = lambda ms: dict(ms=[round(v, 4) for v in ms], median_ms=round(float(np.median(ms)), 4))
    counts = [int(v) for v in a.heads.split(',')]
    flat = lambda x: torch.cat([p.reshape(-1) for p in x]) if isinstance(x, (tuple, list)) else x.reshape(-1)     # a frame, a surface or a (y, uv) pair
    rows = {}
    for n in counts:
        side = rs.randint(24, 401, n)
        x1, y1 = rs.randint(0, W - 400, n), rs.randint(0, H - 400, n)
        rows[n] = (np.stack([x1, y1, x1 + side, y1 + side * 1.25], axis=-1).astype(np.float32), (np.arange(n) % F).astype(np.int32))
    state = pipe.heat_state(F, (H, W), cell=8, device=dev)
    dense = AT.HeatState(up(rs.randint(1, 1000, tuple(state.heat.shape)).astype(np.int32)), up(np.full(F, 999, np.int32)), state.cell_shift)
    sources = dict(bgr=[up(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)) for _ in range(F)],
                   nv12=[up(rs.randint(0, 256, (H * 3 // 2, W)).astype(np.uint8)) for _ in range(F)])
    out = []
    for fmt, frames in sources.items():
        kw = dict(pixel_format=fmt, matrix=a.matrix)
        copies = [torch.empty_like(f) for f in frames]
        big_src = torch.cat([f.reshape(-1) for f in frames])
        big_dst = torch.empty_like(big_src)
        tables = {n: (up(b), up(io)) for n, (b, io) in rows.items()}
        ways = {f'anonymize_{n}': (lambda n=n: pipe.anonymize_heads(frames, *tables[n], device=dev, **kw)) for n in counts}
        ways[f'anonymize_fill_{counts[-1]}'] = lambda: pipe.anonymize_heads(frames, *tables[counts[-1]], mode='fill', device=dev, **kw)
        ways.update(copy=lambda: [c.copy_(f) for c, f in zip(copies, frames)], copy_one=lambda: big_dst.copy_(big_src),
                    draw_dense=lambda: pipe.draw_heat(frames, dense, device=dev, **kw))
        checks = {}
        for n in counts:                                          # before anything is timed in place: the frames are still the sources
            got, flags = pipe.anonymize_heads(frames, *tables[n], copy=True, device=dev, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            old, _ = AR.anonymize_heads_host([f.cpu().numpy() for f in frames], *rows[n], **kw)
            old = [up(np.concatenate([o[0], o[1]]) if fmt == 'nv12' else o) for o in old]
            torch.cuda.synchronize()
            same = all(bool(torch.equal(flat(x), flat(y))) for x, y in zip(got, old))
            changed = sum(int((flat(x) != flat(f)).sum()) for x, f in zip(got, frames))
            checks[n] = dict(host_ms_one_call=round((time.perf_counter() - t0) * 1e3, 1), frames_equal=same, flags_all_zero=not bool(flags.any()),
                             changed_bytes=changed)
            del got, old
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                ms[k].append(timed(fn, a.steps, a.warmup))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out.append(dict(pixel_format=fmt, frame_bytes=sum(f.numel() for f in frames), checks=checks, ways={k: summary(v) for k, v in ms.items()},
                        over_draw_dense={k: round(med[k] / med['draw_dense'], 3) for k in med if k.startswith('anonymize')},
                        over_copy_one={k: round(med[k] / med['copy_one'], 3) for k in med if k.startswith('anonymize')}))
        del big_src, big_dst
    print(json.dumps(dict(tool='anonymize_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0),
                          arch=torch.cuda.get_device_properties(0).gcnArchName, frames=F, frame_hw=[H, W], heads=counts, matrix=a.matrix, steps=a.steps,
                          warmup=a.warmup, rounds=a.rounds, formats=out)))


if __name__ == '__main__':
    main()
