#!/usr/bin/env python3
"""The surface heat map on the device, measured against the image-plane heat map of the same process, against the route a caller had before
(read back, host twin, upload) and inside a live tick.  Prints ONE JSON line.

usage: surface_heat_bench.py [--frames 8] [--regions 16] [--rows 8,64,1024] [--grids 32,128] [--radius 1] [--height 1080] [--width 1920]
                             [--matrix bt709] [--steps 20] [--warmup 3] [--rounds 3] [--live 1x8x3] [--live-steps 20] [--live-warmup 16]

Workload: `--frames` synthetic frames (random bytes) in device memory, packed BGR and NV12 surfaces, one camera (fx = fy = the width) for
all; `--regions` planar quadrilaterals -- tilted screens of 0.5 .. 1 m, 2 .. 5 m from the lens, spread over the field of view -- with a
grid of G x G cells each for every G of --grids.  Every table is a device tensor.  Each way is timed --rounds times, the ways alternated,
each round = --warmup untimed calls, then --steps calls bracketed by synchronize:
  add:   DevicePipeline.surface_heat for each row count of --rows (3-D points on the regions' planes), next to DevicePipeline.gaze_heat over as
         many rows (cells of 8 pixels, one grid per frame);
  draw:  DevicePipeline.draw_surface_heat in place, grids dense (every cell above zero), next to DevicePipeline.draw_heat over a dense grid;
  host:  what a caller did before -- hit3d read back, attention.surface_heat_host, the grids copied up; every frame read back,
         arrows.draw_surface_heat_host (numpy), every frame copied up again.  HOST-BOUND, not a GPU figure; timed ONCE, and that call is also
         the check that both routes give the same.
live: LiveGaze.tick at tools/live_bench.py's shapes (cameras x slots x people, 1080p frames), draw=True and attention in 3-D over the same
kind of regions, with and without surface_heat=dict(draw=True), alternated --rounds times.
No target is fixed in advance: the cost of the surface heat map is whatever this prints."""
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


def screens(rs, m, H, W, f):
    """m tilted quadrilaterals whose centres project inside an H x W picture of focal length f -> a list of [4, 3] vertex lists."""
    out = []
    for _ in range(m):
        z = rs.uniform(2.0, 5.0)
        c = np.array([(rs.uniform(0.1, 0.9) * W - W / 2) * z / f, (rs.uniform(0.1, 0.9) * H - H / 2) * z / f, z])
        yaw = rs.uniform(-0.8, 0.8)
        right, down = np.array([np.cos(yaw), 0.0, np.sin(yaw)]), np.array([0.0, 1.0, 0.0])
        w, h = rs.uniform(0.5, 1.0), rs.uniform(0.5, 1.0)
        out.append([(c + sx * w / 2 * right + sy * h / 2 * down).tolist() for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1))])   # clockwise from the top-left
    return out


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
        attention = dict(camera=[float(FRAME_W), float(FRAME_W), FRAME_W / 2, FRAME_H / 2],
                         regions3d=[screens(rs, a.regions, FRAME_H, FRAME_W, FRAME_W) for _ in range(Q)])
        options = dict(cameras=Q, slots=S, clip_len=CLIP, stride=STRIDE, smooth=0.6, draw=True, attention=attention)
        routes = dict(draw=LiveGaze(engine, pipe, **options), draw_surface_heat=LiveGaze(engine, pipe, surface_heat=dict(radius=a.radius, draw=True), **options))
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
        out.append(dict(cameras=Q, slots=S, people=people, regions=a.regions, frame=[FRAME_H, FRAME_W], precision='f16x3',
                        ways={k: dict(ms=[round(v, 3) for v in ms[k]], median_ms=round(float(np.median(ms[k])), 3)) for k in ms}))
        del routes
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--regions', type=int, default=16)
    ap.add_argument('--rows', default='8,64,1024')
    ap.add_argument('--grids', default='32,128')
    ap.add_argument('--radius', type=int, default=1)
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
    H, W, F, M = a.height, a.width, a.frames, a.regions
    pipe = P.DevicePipeline(CHAIN)
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    summary = lambda ms: dict(ms=[round(v, 4) for v in ms], median_ms=round(float(np.median(ms)), 4))
    host_tables = AT.regions_3d(screens(rs, M, H, W, float(W)))
    tables = AT.PolyRegions3D(up(host_tables.xyz), up(host_tables.start))
    cam_host = np.array([[W, W, W / 2, H / 2]], np.float32)
    cam, region_image = up(cam_host), up(np.full(M, -1, np.int32))
    quads = host_tables.xyz.reshape(M, 4, 3).astype(np.float64)
    sources = dict(bgr=[up(rs.randint(0, 256, (H, W, 3)).astype(np.uint8)) for _ in range(F)],
                   nv12=[up(rs.randint(0, 256, (H * 3 // 2, W)).astype(np.uint8)) for _ in range(F)])
    plane = pipe.heat_state(F, (H, W), cell=8, device=dev)
    dense_plane = AT.HeatState(up(rs.randint(1, 1000, tuple(plane.heat.shape)).astype(np.int32)), up(np.full(F, 999, np.int32)), plane.cell_shift)

    add, draw = [], []
    for G in [int(v) for v in a.grids.split(',')]:
        # ---- accumulate
        for n in [int(v) for v in a.rows.split(',')]:
            target = rs.randint(0, M, n).astype(np.int32)
            s, r = rs.uniform(-0.05, 1.05, (2, n, 1))
            hit3d = (quads[target, 0] + s * (quads[target, 1] - quads[target, 0]) + r * (quads[target, 3] - quads[target, 0])).astype(np.float32)
            d = [up(hit3d), up(np.full(n, 2, np.int32)), up(target)]
            state = pipe.surface_heat_state(M, grid=(G, G), device=dev)
            pipe.surface_heat(*d, tables, state, radius=a.radius, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = AT.surface_heat_host(d[0].cpu().numpy(), d[1].cpu().numpy(), d[2].cpu().numpy(), host_tables, np.zeros((M, G, G), np.int32), radius=a.radius)
            back = up(want[0])
            torch.cuda.synchronize()
            host_ms = (time.perf_counter() - t0) * 1e3
            equal = bool(torch.equal(back, state.heat)) and np.array_equal(want[1], state.peak.cpu().numpy())
            hit = up(np.stack([rs.uniform(0, W, n), rs.uniform(0, H, n)], axis=-1).astype(np.float32))
            image_of = up((np.arange(n) % F).astype(np.int32))
            ways = dict(surface_heat=lambda: pipe.surface_heat(*d, tables, state, radius=a.radius, decay=4, device=dev),
                        gaze_heat=lambda: pipe.gaze_heat(hit, d[1], image_of, plane, radius=2, decay=4, device=dev))
            ms = {k: [] for k in ways}
            for _ in range(a.rounds):
                for k, fn in ways.items():
                    ms[k].append(timed(fn, a.steps, a.warmup))
            add.append(dict(rows=n, grid=[M, G, G], equal=equal, counted=int(want[0].sum() > 0), host_ms_one_call=round(host_ms, 2),
                            ways={k: summary(v) for k, v in ms.items()}))
        # ---- draw
        dense = AT.SurfaceHeatState(up(rs.randint(1, 1000, (M, G, G)).astype(np.int32)), up(np.full(M, 999, np.int32)))
        for fmt, frames in sources.items():
            kw = dict(pixel_format=fmt, matrix=a.matrix)
            fresh = [f.clone() for f in frames]
            got = pipe.draw_surface_heat(fresh, dense, cam, tables, region_image, cam_period=1, device=dev, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            old = AR.draw_surface_heat_host([f.cpu().numpy() for f in frames], dense.heat.cpu().numpy(), dense.peak.cpu().numpy(), cam_host, host_tables,
                                            cam_period=1, **kw)
            old = [up(np.concatenate([o[0], o[1]]) if fmt == 'nv12' else o) for o in old]
            torch.cuda.synchronize()
            check = dict(host_ms_one_call=round((time.perf_counter() - t0) * 1e3, 1), frames_equal=all(bool(torch.equal(x, y)) for x, y in zip(got, old)),
                         changed_bytes=sum(int((x != y).sum()) for x, y in zip(got, frames)))
            del got, old, fresh
            ways = dict(draw_surface_heat=lambda: pipe.draw_surface_heat(frames, dense, cam, tables, region_image, cam_period=1, device=dev, **kw),
                        draw_heat=lambda: pipe.draw_heat(frames, dense_plane, device=dev, **kw))
            ms = {k: [] for k in ways}
            for _ in range(a.rounds):
                for k, fn in ways.items():
                    ms[k].append(timed(fn, a.steps, a.warmup))
            draw.append(dict(pixel_format=fmt, grid=[M, G, G], check=check, ways={k: summary(v) for k, v in ms.items()}))
    live = live_cases(a, dev)
    print(json.dumps(dict(tool='surface_heat_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0),
                          arch=torch.cuda.get_device_properties(0).gcnArchName, frames=F, frame_hw=[H, W], regions=M, radius=a.radius, matrix=a.matrix,
                          steps=a.steps, warmup=a.warmup, rounds=a.rounds, add=add, draw=draw, live=live)))


if __name__ == '__main__':
    main()
