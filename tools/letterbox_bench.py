#!/usr/bin/env python3
"""The detector's input on the device, measured against the only route there was before: frames to the host, letterbox there, upload.  Prints
ONE JSON line.

usage: letterbox_bench.py [--images 1,8,64] [--host-images 1,8] [--frame 1080x1920] [--new-shape 640] [--dtype float16] [--steps 20] [--warmup 3]
                          [--rounds 3]

Workload: for each batch size of `--images`, that many DISTINCT random frames of `--frame` (h x w) in device memory, as packed BGR and as NV12
surfaces, letterboxed to the demo's 640 detector (1080p -> 384 x 640) in `--dtype`.  Ways, alternated --rounds times, each round = --warmup
untimed calls, then --steps calls bracketed by synchronize:
  bgr, nv12:  DevicePipeline.letterbox on the device frames (mcg_letterbox_frames / _nv12: one launch, nothing read back);
  host:       what a caller did before -- every BGR frame copied to the host, head_detect.letterbox_host, the result uploaded.  HOST-BOUND:
              numpy on one core, about a third of a second per 1080p frame, so its time says nothing about the device and its ratio to
              `bgr` is that of this comparison only; run for the batch sizes of `--host-images`, one untimed call and one timed call a round.
Reported per batch size and way: ms per call of every round and the median; for the device ways also the bytes the call must move by
construction -- every source byte some tap reads, counted once (worked out from the coefficient tables), plus the output -- and the
bytes per second that makes at the median.  The device result is compared with letterbox_host once, on the first frame of each batch."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mcgaze_amd import head_detect as H  # noqa: E402
from mcgaze_amd import lib  # noqa: E402
from mcgaze_amd import pipeline as P  # noqa: E402
from tools.detect_bench import CHAIN, timed  # noqa: E402


def source_bytes(g, h, w, nv12):
    """The distinct source bytes the four taps of every output pixel of the rectangle read."""
    y0, y1, _, _ = H._linear_coef(g.unpad_h, h)
    x0, x1, _, _ = H._linear_coef(g.unpad_w, w)
    rows, cols = np.union1d(y0, y1), np.union1d(x0, x1)
    if not nv12:
        return 3 * len(rows) * len(cols)
    return len(rows) * len(cols) + 2 * len(np.unique(rows >> 1)) * len(np.unique(cols >> 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', default='1,8,64')
    ap.add_argument('--host-images', default='1,8')
    ap.add_argument('--frame', default='1080x1920')
    ap.add_argument('--new-shape', type=int, default=640)
    ap.add_argument('--dtype', default='float16', choices=['uint8', 'float16', 'float32'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    dev = 'cuda:0'
    h, w = (int(v) for v in a.frame.lower().split('x'))
    dtype = getattr(torch, a.dtype)
    host_sizes = [int(v) for v in a.host_images.split(',') if v]
    rs = np.random.RandomState(7)
    pipe = P.DevicePipeline(CHAIN)
    g = H.letterbox_geometry(h, w, a.new_shape)
    out_bytes = 3 * g.out_h * g.out_w * torch.empty(0, dtype=dtype).element_size()
    cases = []
    for B in [int(v) for v in a.images.split(',')]:
        bgr = [torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(dev) for _ in range(B)]
        nv12 = [torch.from_numpy(rs.randint(0, 256, (h * 3 // 2, w)).astype(np.uint8)).to(dev) for _ in range(B)]

        def device_bgr():
            return pipe.letterbox(bgr, a.new_shape, dtype=dtype, device=dev)[0]

        def device_nv12():
            return pipe.letterbox(nv12, a.new_shape, dtype=dtype, pixel_format='nv12', matrix='bt709', device=dev)[0]

        def host():
            img, _ = H.letterbox_host([f.cpu().numpy() for f in bgr], a.new_shape, dtype=dtype)
            return torch.from_numpy(img).to(dev)

        got = device_bgr()[:1], device_nv12()[:1]
        torch.cuda.synchronize()
        want = (H.letterbox_host(bgr[:1], a.new_shape, dtype=dtype)[0], H.letterbox_host(nv12[:1], a.new_shape, dtype=dtype, pixel_format='nv12', matrix='bt709')[0])
        equal = all(bool(torch.equal(x.cpu(), torch.from_numpy(y))) for x, y in zip(got, want))
        ways = dict(bgr=device_bgr, nv12=device_nv12, **(dict(host=host) if B in host_sizes else {}))
        ms = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, fn in ways.items():
                ms[k].append(timed(fn, 1, 1) if k == 'host' else timed(fn, a.steps, a.warmup))
        report = {}
        for k in ways:
            med = float(np.median(ms[k]))
            report[k] = dict(ms=[round(v, 4) for v in ms[k]], median_ms=round(med, 4))
            if k != 'host':
                must = B * (source_bytes(g, h, w, k == 'nv12') + out_bytes)
                report[k].update(must_move_bytes=must, gb_per_s=round(must / (med * 1e-3) / 1e9, 1))
        cases.append(dict(images=B, equals_host=equal, ways=report))
    print(json.dumps(dict(tool='letterbox_bench', build_id=lib.build_id(), device=torch.cuda.get_device_name(0),
                          arch=torch.cuda.get_device_properties(0).gcnArchName, frame_hw=(h, w), new_shape=a.new_shape, out_shape=(g.out_h, g.out_w),
                          dtype=a.dtype, steps=a.steps, host_steps=1, warmup=a.warmup, rounds=a.rounds, cases=cases)))


if __name__ == '__main__':
    main()
