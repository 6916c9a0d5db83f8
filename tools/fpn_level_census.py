"""CPU tool: which FPN levels do the decoder's boxes read, frame by frame?  Runs the CPU oracle on bench.py's seeded batch
(synth.make_clips(3, clips, 7, 224, 224), make_state_dict(0)) and on the 'trained' weight family of the parity fuzz, takes the boxes
every stage's RoIAlign sees, applies the level rule as roi_align.hip states it (roi_sample.hpp: roi_level, float32, finest scale 56)
and counts, per level, the share of frames in which at least one box of any stage reads it -- the share of (frame, level) pairs a
per-frame deferred FPN output conv would still compute.  Prints a Markdown table.
usage: python tools/fpn_level_census.py [clips=16] [size=224] [clip_length=7]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mcgaze_amd import synth
from oracle import mcgaze_oracle as orc

# dense launch time of the level's output conv per 448-frame step (ms): DESIGN.md 3.1i, profiles/r06_h_bench.json rows 43 / 44
DENSE_MS = {1: 0.81, 2: 0.232, 3: 0.083}


def roi_level(boxes, finest_scale=56.0):
    """roi_sample.hpp: roi_level, in float32 like the device; boxes [..., 4] xyxy -> int level 0 .. 3 (a NaN box reads level 0)."""
    b = np.asarray(boxes, dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        sc = np.sqrt((b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]), dtype=np.float32)
        lv = np.floor(np.log2(sc / np.float32(finest_scale) + np.float32(1e-6), dtype=np.float32))
    lv = np.fmin(np.fmax(lv, np.float32(0)), np.float32(3))   # fmaxf / fminf: NaN loses
    lv = np.where(np.isnan(sc), np.float32(0), lv)
    return lv.astype(np.int64)


def stage_boxes(sd, img, metas, T, batch=14):
    """[stages][N, 3, 4]: the boxes each stage's RoIAlign reads (stage 0: the initial proposals), clip batches of `batch` frames."""
    per_stage = None
    for f0 in range(0, img.shape[0], batch):
        m = metas[f0:f0 + batch]
        collect = []
        orc.forward(sd, img[f0:f0 + batch], m, T, collect=collect)
        init, _ = orc.init_proposals(orc.as_torch(sd), m)
        got = [init.numpy()] + [c['boxes'].numpy() for c in collect[:-1]]
        per_stage = [[g] for g in got] if per_stage is None else [p + [g] for p, g in zip(per_stage, got)]
    return [np.concatenate(p) for p in per_stage]


def census(family, clips, size, T):
    sd = synth.make_state_dict(0, family=family)
    img = synth.make_clips(3, clips, T, size, size)
    metas = synth.make_img_metas(clips * T, (size, size, 3))
    boxes = stage_boxes(sd, img, metas, T, batch=2 * T)
    lv = np.stack([roi_level(b) for b in boxes])                        # [stages, N, 3]
    read = np.stack([(lv == l).any(axis=(0, 2)) for l in range(4)])     # [level, N]: some box of some stage reads it
    per_stage = np.stack([[(lv[s] == l).any(axis=1).mean() for l in range(4)] for s in range(lv.shape[0])])
    return read.mean(axis=1), per_stage


def main():
    clips = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 224
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    print(f'Frames of {size} x {size}, {clips} clips x {T} frames of synth.make_clips(3, ...), make_state_dict(0, family).  '
          'Share of frames in which at least one of the 3 boxes of at least one of the 4 stages maps to the level '
          '(roi_level, finest scale 56).\n')
    print('| weights | P2 read | P3 read | P4 read | P5 read | per stage (P2 / P3 / P4 / P5) |')
    print('|---|---|---|---|---|---|')
    shares = {}
    for family in ('uniform', 'trained'):
        share, per_stage = census(family, clips, size, T)
        shares[family] = share
        stages = '; '.join(f'{s}: ' + ' / '.join(f'{v:.2f}' for v in row) for s, row in enumerate(per_stage))
        print(f'| {family} | ' + ' | '.join(f'{v:.3f}' for v in share) + f' | {stages} |', flush=True)
    print('\n| level | dense ms per step | unread share (uniform) | removable ms | unread share (trained) | defer (unread >= 25 %) |')
    print('|---|---|---|---|---|---|')
    total = 0.0
    for l in (1, 2, 3):
        u, t = 1 - shares['uniform'][l], 1 - shares['trained'][l]
        total += u * DENSE_MS[l]
        print(f'| P{l + 2} | {DENSE_MS[l]} | {u:.3f} | {u * DENSE_MS[l]:.3f} | {t:.3f} | {"yes" if u >= 0.25 else "no"} |')
    print(f'\nExpected removable time on the benchmark batch: {total:.3f} ms per step, before the list launches\' own cost.')


if __name__ == '__main__':
    main()
