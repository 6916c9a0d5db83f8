#!/usr/bin/env python3
"""The gaze heat map on the device, measured against the route a caller had before, against the attention overlay and a plain device copy
of the same frames, and inside a live tick.  Prints ONE JSON line.

usage: heat_bench.py [--frames 8] [--rows 8,64,1024] [--cell 8] [--radius 2] [--height 1080] [--width 1920] [--matrix bt709] [--steps 20]
                     [--warmup 3] [--rounds 3] [--live 1x8x3] [--live-steps 20] [--live-warmup 16]

Workload: `--frames` synthetic frames (random bytes) in device memory, packed BGR and NV12 surfaces, one camera per frame; grids of
`--cell`-pixel cells over them.  Every table is a device tensor.  Each way is timed --rounds times, the ways alternated, each round =
--warmup untimed calls, then --steps calls bracketed by synchronize:
  add:     DevicePipeline.gaze_heat for each row count of --rows (hit points spread over the frames, kinds 1 and 2);
  draw:    DevicePipeline.draw_heat in place over a SPARSE grid (what 1024 rows leave: most tiles hold only zeros and read no pixel) and over
           a DENSE grid (every cell above zero: every pixel of every frame is read, blended and written);
  copy:    dst.copy_(src) of the same frames, one launch per frame -- every byte read once and written once;
  copy_one: ONE copy_ of one tensor that holds as many bytes as all the frames -- the same bytes in a single launch, as draw_heat is: the
           floor of a whole-frame pass without the launches of `copy`;
  overlay: DevicePipeline.draw_attention with 64 rows and 16 regions on the same frames, for scale;
  host:    what a caller did before -- hit read back, attention.gaze_heat_host; every frame read back, arrows.draw_heat_host (numpy), every
           frame copied up again.  HOST-BOUND, not a GPU figure; timed ONCE, and that call is also the check that both routes give the same.
live: LiveGaze.tick at tools/live_bench.py's shapes (cameras x slots x people, 1080p frames), draw=True and attention=True with and without
heat=dict(draw=True), alternated --rounds times.
No target is fixed in advance: the cost of the heat map is whatever this prints."""
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
from mcgaze_amd import lib, synth  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from draw_bench import CHAIN, timed  # noqa: E402  (tools/ is the script's directory)


def live_cases(a, dev):
    from live_bench import CLIP, FRAME_H, FRAME_W, STRIDE, walkers
    from live_bench import timed as timed_ticks
    from mcgaze_amd.engine import HipEngine
    from mcgaze_amd.live import LiveGaze
    rs = np.random.RandomState(11)
    engine = HipEngine(synth.make_state_dict(0), precision='f16x3')
    out = []
    for case in [c for c in a.live.split(',') if c]:
        Q, S, people = (int(v) for v in case.split('x'))
        ticks = a.rounds * (a.live_warmup + a.live_steps)
        host_boxes, host_counts = walkers(rs, Q, ticks, people)
        boxes, counts = torch.from_numpy(host_boxes).to(dev), torch.from_numpy(host_counts).to(dev)
        frames = [torch.randint(0, 256, (FRAME_H, FRAME_W, 3), dtype=torch.uint8, device=dev) for _ in range(Q)]
        pipe = P.DevicePipeline(CHAIN)
        options = dict(cameras=Q, slots=S, clip_len=CLIP, stride=STRIDE, smooth=0.6, draw=True, attention=True)
        routes = dict(draw=LiveGaze(engine, pipe, **options), draw_heat=LiveGaze(engine, pipe, heat=dict(cell=a.cell, radius=a.radius, draw=True), **options))
        at = {k: 0 for k in routes}

        def step(name):
            routes[name].tick(frames, boxes[at[name]], counts[at[name]])
            at[name] += 1

        ms = {k: [] for k in routes}
        for _ in range(a.rounds):
            for name in routes:
                for _ in range(a.live_warmup):
                    step(name)
                ms[name].append(timed_ticks(lambda: step(name), a.live_steps))
        out.append(dict(cameras=Q, slots=S, people=people, frame=[FRAME_H, FRAME_W], precision='f16x3',
                        ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3)) for k in ms}))
        del routes
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--rows', default='8,64,1024')
    ap.add_argument('--cell', type=int, default=8)
    ap.add_argument('--radius', type=int, default=2)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--matrix', default='bt709', choices=sorted(P.YUV_COEF))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--live', default='1x8x3')
    ap.add_argument('--live-steps', type=int, default=20)
    ap.add_argument('--live-warmup', type=int, default=16)
    a = ap.parse_args()
    dev = 'cuda:0'
    rs = np.random.RandomState(3)
    H, W, F = a.height, a.width, a.frames
    pipe = P.DevicePipeline(CHAIN)
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    summary = lambda ms: dict(ms=[round(v, 4) for v in ms], median_ms=round(float(np.median(ms)), 4))

    # ---- accumulate
    add = []
    for n in [int(v) for v in a.rows.split(',')]:
        hit = np.stack([rs.uniform(-20, W + 20, n), rs.uniform(-20, H + 20, n)], axis=-1).astype(np.float32)
        kind, image_of = rs.randint(1, 3, n).astype(np.int32), (np.arange(n) % F).astype(np.int32)
        d = [up(t) for t in (hit, kind, image_of)]
        state = pipe.heat_state(F, (H, W), cell=a.cell, device=dev)
        pipe.gaze_heat(*d, state, radius=a.radius, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = AT.gaze_heat_host(d[0].cpu().numpy(), d[1].cpu().numpy(), d[2].cpu().numpy(), np.zeros(tuple(state.heat.shape), np.int32),
                                 cell_shift=state.cell_shift, radius=a.radius)
        back = up(want[0])
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3
        equal = bool(torch.equal(back, state.heat)) and np.array_equal(want[1], state.peak.cpu().numpy())
        ms = [timed(lambda: pipe.gaze_heat(*d, state, radius=a.radius, decay=4, device=dev), a.steps, a.warmup) for _ in range(a.rounds)]
        add.append(dict(rows=n, grid=list(state.heat.shape), equal=equal, host_ms_one_call=round(host_ms, 2), **summary(ms)))

    # ---- draw
    sparse = pipe.heat_state(F, (H, W), cell=a.cell, device=dev)
    n = 1024
    pipe.gaze_heat(up(np.stack([rs.normal(W / 2, W / 8, n), rs.normal(H / 2, H / 8, n)], axis=-1).astype(np.float32)), up(np.ones(n, np.int32)),
                   up((np.arange(n) % F).astype(np.int32)), sparse, radius=a.radius, device=dev)
    dense = AT.HeatState(up(rs.randint(1, 1000, tuple(sparse.heat.shape)).astype(np.int32)), up(np.full(F, 999, np.int32)), sparse.cell_shift)
    sources = dict(bgr=[up(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)) for _ in range(F)],
                   nv12=[up(rs.randint(0, 256, (H * 3 // 2, W)).astype(np.uint8)) for _ in range(F)])
    # the overlay's rows, for scale: 64 heads, 16 regions
    m = 64
    side = rs.randint(120, 401, m)
    x1, y1 = rs.randint(0, W - 400, m), rs.randint(0, H - 400, m)
    boxes = up(np.stack([x1, y1, x1 + side, y1 + side], axis=-1).astype(np.float32))
    g = rs.normal(size=(m, 3))
    gaze, image_of = up((g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)), up((np.arange(m) % F).astype(np.int32))
    rx, ry = rs.randint(0, W - 300, 16), rs.randint(0, H - 300, 16)
    regions = up(np.stack([rx, ry, rx + 280, ry + 200], axis=-1).astype(np.float32))
    targets = pipe.gaze_targets(boxes, gaze, image_of, regions=regions, device=dev)
    draw = []
    for fmt, frames in sources.items():
        kw = dict(pixel_format=fmt, matrix=a.matrix)
        copies = [torch.empty_like(f) for f in frames]
        big_src = torch.cat([f.reshape(-1) for f in frames])
        big_dst = torch.empty_like(big_src)
        ways = dict(draw_sparse=lambda: pipe.draw_heat(frames, sparse, device=dev, **kw), draw_dense=lambda: pipe.draw_heat(frames, dense, device=dev, **kw),
                    copy=lambda: [c.copy_(f) for c, f in zip(copies, frames)], copy_one=lambda: big_dst.copy_(big_src),
                    overlay=lambda: pipe.draw_attention(frames, boxes, gaze, image_of, targets[0], targets[1], targets[3], targets[4], regions=regions,
                                                        device=dev, **kw))
        checks = {}
        for name, state in (('sparse', sparse), ('dense', dense)):
            fresh = [f.clone() for f in frames]
            got = pipe.draw_heat(fresh, state, device=dev, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            old = AR.draw_heat_host([f.cpu().numpy() for f in frames], state.heat.cpu().numpy(), state.peak.cpu().numpy(), state.cell_shift, **kw)
            old = [up(np.concatenate([o[0], o[1]]) if fmt == 'nv12' else o) for o in old]
            torch.cuda.synchronize()
            checks[name] = dict(host_ms_one_call=round((time.perf_counter() - t0) * 1e3, 1), frames_equal=all(bool(torch.equal(x, y)) for x, y in zip(got, old)),
                                changed_bytes=sum(int((x != y).sum()) for x, y in zip(got, frames)))
            del got, old, fresh
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                ms[k].append(timed(fn, a.steps, a.warmup))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        draw.append(dict(pixel_format=fmt, bytes_per_pass=2 * sum(f.numel() for f in frames), checks=checks, ways={k: summary(v) for k, v in ms.items()},
                         dense_over_copy=round(med['draw_dense'] / med['copy'], 2), sparse_over_copy=round(med['draw_sparse'] / med['copy'], 2),
                         dense_over_copy_one=round(med['draw_dense'] / med['copy_one'], 2), sparse_over_copy_one=round(med['draw_sparse'] / med['copy_one'], 2)))
        del big_src, big_dst
    live = live_cases(a, dev)
    print(json.dumps(dict(tool='heat_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                          frames=F, frame_hw=[H, W], cell=a.cell, radius=a.radius, matrix=a.matrix, steps=a.steps, warmup=a.warmup, rounds=a.rounds, add=add,
                          draw=draw, live=live)))


if __name__ == '__main__':
    main()
