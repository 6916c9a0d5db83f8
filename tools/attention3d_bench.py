#!/usr/bin/env python3
"""Gaze targets in 3-D against the 2-D polygon call, in one process, at tools/attention_bench.py's shapes.  Prints ONE JSON line; --out also
appends the note profiles/attention3d_<build id>.md holds.

usage: attention3d_bench.py [--shapes 8x1,64x8,1024x64] [--regions 16] [--calls 20] [--rounds 3] [--runs 2] [--out FILE]

Per shape n x pictures: attention_bench's rows (n rows spread evenly over the pictures, ascending image_of, integer-pixel boxes in 1280 x
720 pictures, random unit gaze), every table in device memory.
  poly:    DevicePipeline.gaze_targets with --regions quadrilaterals (attention_bench's sheared rectangles; mcg_gaze_targets_poly).
  eye, camera:  DevicePipeline.gaze_targets_3d in either frame (mcg_gaze_targets_3d), one camera (fx = fy = 1000, the principal point in
           the picture's middle), depth from the head size, --regions planar quadrilaterals of 4 vertices: the same rectangles lifted to
           walls 2 .. 6 m away.
  depth:   the 'eye' call with a depth table given.
--runs times: --rounds rounds alternated, each --calls calls bracketed by synchronize; the median round of each run, us per call.  Every
3-D leg is first compared with attention.gaze_targets_3d_host, bit for bit.  The ratios are those of this comparison only."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from attention_bench import polygons, tables  # noqa: E402
from live_bench import CHAIN, DEV, FRAME_H, FRAME_W, timed  # noqa: E402
from mcgaze_amd import lib  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from mcgaze_amd.attention import PolyRegions, PolyRegions3D, gaze_targets_3d_host, regions_3d, unproject  # noqa: E402

CAM = np.asarray([[1000.0, 1000.0, FRAME_W / 2, FRAME_H / 2]], np.float32)


def walls(regions, rs):
    """Every rectangle of the picture as a wall facing the lens, 2 .. 6 m away: its corners lifted to that depth."""
    out = []
    for (x1, y1, x2, y2), z in zip(regions.tolist(), rs.randint(8, 25, len(regions)) / 4.0):
        out.append(unproject([[x1, y1], [x2, y1], [x2, y2], [x1, y2]], z, CAM[0]).tolist())
    return regions_3d(out)


def bench_call(pipe, shape, m, calls, rounds, runs, rs):
    n, pictures = shape
    host = tables(rs, n, pictures, m)
    boxes, gaze, image_of, _ = (torch.from_numpy(t).to(DEV) for t in host)
    region_image = torch.full((m,), -1, dtype=torch.int32, device=DEV)
    quads = PolyRegions(*(torch.from_numpy(t).to(DEV) for t in polygons(host[3], 4)))
    host_walls = walls(host[3], rs)
    walls_dev = PolyRegions3D(*(torch.from_numpy(t).to(DEV) for t in host_walls))
    host_depth = (rs.randint(4, 33, n) / 4.0).astype(np.float32)
    depth, cam = torch.from_numpy(host_depth).to(DEV), torch.from_numpy(CAM).to(DEV)

    def three_d(frame, d=None):
        return lambda: pipe.gaze_targets_3d(boxes, gaze, image_of, cam, depth=d, regions=walls_dev, region_image=region_image, cam_period=1, frame=frame,
                                            device=DEV)

    routes = (('poly', lambda: pipe.gaze_targets(boxes, gaze, image_of, regions=quads, region_image=region_image, device=DEV)), ('eye', three_d('eye')),
              ('camera', three_d('camera')), ('depth', three_d('eye', depth)))
    same = True
    for name, frame, d in (('eye', 'eye', None), ('camera', 'camera', None), ('depth', 'eye', host_depth)):
        twin = gaze_targets_3d_host(host[0], host[1], host[2], CAM, depth=d, regions=host_walls, cam_period=1, frame=frame)
        same = same and all(torch.equal(a.cpu().view(torch.int32), torch.from_numpy(b).view(torch.int32)) for a, b in zip(dict(routes)[name](), twin))
    out = dict(rows=n, pictures=pictures, regions=m, equal=bool(same), us={name: [] for name, _ in routes})
    for _ in range(runs):
        us = {name: [] for name, _ in routes}
        for _ in range(rounds):
            for name, fn in routes:
                us[name].append(timed(fn, calls) * 1e3)
        for name in us:
            out['us'][name].append(round(float(np.median(us[name])), 2))
    out['eye_over_poly'] = [round(e / p, 2) for p, e in zip(out['us']['poly'], out['us']['eye'])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='8x1,64x8,1024x64')
    ap.add_argument('--regions', type=int, default=16)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--out')
    a = ap.parse_args()
    rs = np.random.RandomState(5)
    pipe = P.DevicePipeline(CHAIN)
    calls = [bench_call(pipe, tuple(int(v) for v in s.split('x')), a.regions, a.calls, a.rounds, a.runs, rs) for s in a.shapes.split(',') if s]
    line = dict(tool='attention3d_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0), arch=torch.cuda.get_device_properties(0).gcnArchName,
                calls_per_round=a.calls, rounds=a.rounds, runs=a.runs, call=calls)
    print(json.dumps(line))
    if a.out:
        rows = ['| rows x pictures, regions | 2-D quadrilaterals us / call (runs) | 3-D eye us / call (runs) | 3-D camera us / call (runs) | '
                '3-D eye with depth us / call (runs) | eye / quadrilaterals | equal to the twin |', '|---|---|---|---|---|---|---|']
        for c in calls:
            rows.append(f"| {c['rows']} x {c['pictures']}, {c['regions']} | {c['us']['poly']} | {c['us']['eye']} | {c['us']['camera']} | {c['us']['depth']} | "
                        f"{c['eye_over_poly']} | {c['equal']} |")
        with open(a.out, 'a') as f:
            f.write(f"\n## Run on {line['device']} ({line['arch']}), build {line['build_id']}\n\n{a.calls} calls a round, {a.rounds} rounds alternated, "
                    f"the median round of each of {a.runs} runs.\n\n" + '\n'.join(rows) + '\n')


if __name__ == '__main__':
    main()
