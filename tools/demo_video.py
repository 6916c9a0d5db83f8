#!/usr/bin/env python3
"""Steps 3 - 5 of the reference's demo (MCGaze_demo/README.md; demo.ipynb, cells 1 - 5): a directory of video frames and the head detector's
label files in, per-person per-frame gaze out -- and, with --draw, the frames with cell 5's arrows drawn on the device.

usage: demo_video.py FRAMES_DIR LABELS_DIR CONFIG CHECKPOINT --out gaze.json [--precision f16x3] [--device cuda:0] [--max-len 100]
                     [--batch-frames 448] [--head-class 1] [--ext jpg] [--smooth ALPHA] [--nv12 WxH FILE] [--matrix bt601] [--draw OUT] [--overlay] [--labels [SCALE]] [--fps NUM[/DEN]]
                     [--track [--slots 16] [--match-iou 0.3] [--max-age 5]] [--track-motion [GAIN[,DECAY]]]
                     [--color B,G,R] [--predictions DIR --in-shape HxW [--conf-thres 0.25] [--iou-thres 0.45]]
                     [--detector MODULE:FACTORY [--img-size 640] [--half]] [--attention [--regions FILE.json] [--camera FX,FY,CX,CY [--regions3d FILE.json] [--head-size M] [--gaze-frame eye|camera]] [--dwell [ENTER,EXIT]] [--heat [CELL,RADIUS]] [--heat-out FILE.npy] [--surface-heat [GW,GH,RADIUS]] [--surface-heat-out FILE.npy]]

FRAMES_DIR holds 0.<ext>, 1.<ext>, ... (the demo's `frames/`), LABELS_DIR holds 0.txt, 1.txt, ... with lines `class x1 y1 x2 y2` in pixels
(the demo's `result/labels/`); a frame without a label file shows no head.  CONFIG is the L2CS config, whose test pipeline the demo runs
on every head crop.  The result file holds one entry per (segment, person) in the notebook's order -- a segment is a run of frames with
the same number of heads, people are numbered left to right: `frame_id`, `head_box`, `crop` (y0, x0, h, w of the window cut from the
frame), `gaze` (the fused gaze the notebook draws), `arrow` ((cx, cy) and the tip of the arrow of cell 5), and the per-clue boxes (in
pixels of the head window, rescale=True), scores and gazes of harness.run_tracks (`det`, `others`).  --smooth ALPHA (the reference's metric
uses 0.6, tools/calculate_mae_gaze360.py:16-29) adds `gaze_smooth`, the fused gaze filtered over each track, and draws `arrow` from it.
--nv12 WxH FILE: the frames come from a raw NV12 video instead (`ffmpeg -i in.mp4 -pix_fmt nv12 -f rawvideo FILE`: per frame H rows of Y, then
H/2 rows of interleaved U, V, W bytes each), read frame by frame with numpy and handed to the device as they are; FRAMES_DIR is then `-`.
--matrix names the YUV -> RGB coefficients, bt601 or bt709 (limited range; HD video is usually bt709).  The records are the same.
--draw OUT: the arrows of cell 5 are drawn into every frame on the device (harness.run_head_video(draw=...), from the gaze `arrow` comes
from) and the annotated frames written into the directory OUT with numpy alone: 0.ppm, 1.ppm, ... (binary PPM, RGB), or with --nv12 ONE raw
NV12 file OUT/annotated.nv12 (`ffmpeg -f rawvideo -pix_fmt nv12 -s WxH -i OUT/annotated.nv12 out.mp4` encodes it).  --color B,G,R sets
the arrows' colour (default: the demo's 230,253,11).
--predictions DIR: instead of label files (LABELS_DIR is then `-`) DIR holds the head detector's RAW output, one `<t>.npy` per frame:
the [N, 5 + nc] (or [1, N, 5 + nc]) prediction of frame t, as the YOLOv5 model returns it before non_max_suppression.  --in-shape HxW is
the size of the letterboxed image the detector saw (e.g. 384x640 for 1080p frames).  The confidence filter, NMS and the scale-back into the
frame run on the device (harness.run_head_video(detections=...), pipeline.detect_heads); --head-class, --conf-thres and --iou-thres are
the detector's options.
--detector MODULE:FACTORY: the detector itself runs (LABELS_DIR is then `-`, and --predictions is not given): MODULE is imported,
`FACTORY()` returns a callable that takes the letterboxed batch [B, 3, h, w] on the device -- RGB planes in [0, 1], half with --half, else
float -- and returns the raw [B, N, 5 + nc] prediction (or a tuple / list that starts with it).  The letterbox (--img-size, the demo's 640,
stride 32), the filter, NMS and the scale-back run on the device (harness.run_head_video(detections=dict(detector=...)),
pipeline.letterbox and pipeline.detect_heads); the network is the caller's.
--attention: what every person looks at in every frame (harness.run_head_video(attention=...), pipeline.gaze_targets on the device): each
entry gains per frame `target_kind` (0 none, 1 another person, 2 a region, 3 the camera), `target_id` (the [segment, person] looked at, or
null), `target_region`, `target_hit` (where the gaze ray enters the target, in frame pixels) and `mutual`.  --regions FILE.json: a JSON list
of regions in frame pixels -- a screen, a shelf, a door --, each a rectangle [x1, y1, x2, y2] or a polygon [[x, y], [x, y], ...] of 3 .. 32
vertices in either winding (a screen seen off-axis is a quadrilateral, a shelf beside a pillar an L: even-odd rule, so a notch is outside);
`target_region` is the index into that list.  Decided in the image plane, with conventional,
untuned defaults (a looked-at head box grown by 0.25 of its longer side, a 10 degree cone for the camera).
--camera FX,FY,CX,CY, with --attention: the targets are decided in camera space (pipeline.gaze_targets_3d): depth from --head-size M (0.24) over the
head's size in pixels, the gaze relative to the line from the lens to the head (--gaze-frame eye, the default) or to the optical axis (camera),
--regions3d FILE.json a JSON list of planar polygons [[x, y, z], ...] in camera coordinates (metres).  `target_hit` is then the 3-D point projected
to pixels and `target_hit3d` the point; --regions are only what --overlay draws.
--dwell [ENTER,EXIT], with --attention: how LONG they look (harness.run_head_video(dwell=...), pipeline.gaze_dwell on the device): each entry
gains per frame `dwell_kind` and `dwell_frames` (the current target and its frames so far) and `episodes`, a list of {kind, target_id or
target_region, start, frames, mutual_frames, reason (1 looked away, 2 the person left, 3 replaced by another target, 4 the video ended)}.  A
look becomes current after ENTER consecutive frames and ends after EXIT consecutive frames without it (default 3,2: conventions, not tuned
on data).
--heat [CELL,RADIUS], with --attention: WHERE in the picture the looks land (harness.run_head_video(heat=...), pipeline.gaze_heat on the
device): the hit points of every frame splatted into a grid of CELL-pixel cells (a power of two, default 8) with a radius of RADIUS cells
(default 2).  With --draw the final grid is blended into every annotated frame, under the arrows (pipeline.draw_heat); --heat-out FILE.npy
writes the grid, int32 [1, GH, GW].
--surface-heat [GW,GH,RADIUS], with --camera and --regions3d: WHERE ON each planar region the looks land
(harness.run_head_video(surface_heat=...), pipeline.surface_heat on the device): the 3-D hit points of every frame taken into the region's
own coordinates and splatted into a grid of GW x GH cells per region (default 32,32; radius 1 -- conventions, not tuned on data).  With
--draw the final grids are drawn back onto the regions in every annotated frame with the right perspective
(pipeline.draw_surface_heat); --surface-heat-out FILE.npy writes the grids, int32 [M, GH, GW] (attention.surface_extent gives each
region's width and height in metres, for showing a grid at the right aspect).
--anonymize [BLOCKS], with --draw: the faces under the head boxes are removed from the written frames on the device
(harness.run_head_video(anonymize=...), pipeline.anonymize_heads), before anything is drawn over them -- a mosaic of about BLOCKS cells
across every head (default 8) under the ellipse inscribed in the grown box; --anonymize-shape box covers the whole box.  It hides the heads
that were detected: a head the detector missed stays visible."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mcgaze_amd import harness, init_detector  # noqa: E402
from mcgaze_amd.pipeline import DevicePipeline, LoadImageFromFile  # noqa: E402


class Frames:
    """The demo's frames/ directory, decoded when a group of crops asks for them (RGB, as the decoder delivers them)."""

    def __init__(self, root, n, ext):
        self.root, self.n, self.ext = root, n, ext

    def __len__(self):
        return self.n

    def __getitem__(self, t):
        return LoadImageFromFile.load(os.path.join(self.root, f'{t}.{self.ext}'), rgb=True)


class Nv12File:
    """A raw NV12 video (`-pix_fmt nv12 -f rawvideo`): frame t is the (y [H,W], uv [H/2,W]) pair of views of its 3 H W / 2 bytes, read when a
    group of crops asks for it.  Bytes behind the last whole frame are ignored."""

    def __init__(self, path, w, h):
        if w <= 0 or h <= 0 or w % 2 or h % 2:
            raise ValueError(f'NV12 frames have even, positive sizes, got {w}x{h}')
        self.path, self.w, self.h = path, w, h
        self.frame_bytes = w * h * 3 // 2
        self.n = os.path.getsize(path) // self.frame_bytes

    def __len__(self):
        return self.n

    def __getitem__(self, t):
        if not 0 <= t < self.n:
            raise IndexError(t)
        s = np.fromfile(self.path, dtype=np.uint8, count=self.frame_bytes, offset=t * self.frame_bytes).reshape(self.h * 3 // 2, self.w)
        return s[:self.h], s[self.h:]


def parse_size(text):
    """'1920x1080' -> (1920, 1080)"""
    w, _, h = text.lower().partition('x')
    if not (w.isdigit() and h.isdigit()):
        raise ValueError(f'expected WxH, got {text!r}')
    return int(w), int(h)


def parse_color(text):
    """'230,253,11' -> (230, 253, 11)"""
    v = text.split(',')
    if len(v) != 3 or not all(t.strip().isdigit() and int(t) <= 255 for t in v):
        raise ValueError(f'expected B,G,R with each in 0..255, got {text!r}')
    return tuple(int(t) for t in v)


def write_annotated(out_dir, annotated, nv12):
    """The annotated frames of run_head_video(draw=...) -> files, with numpy alone.  Packed frames (RGB: the frames were loaded in the decoder's
    order) become binary PPM files 0.ppm, 1.ppm, ...; NV12 surfaces are appended to ONE raw file, annotated.nv12 (H rows of Y, then H/2 rows
    of U, V per frame -- what `ffmpeg -f rawvideo -pix_fmt nv12` reads)."""
    os.makedirs(out_dir, exist_ok=True)
    if nv12:
        with open(os.path.join(out_dir, 'annotated.nv12'), 'wb') as f:
            for y, uv in annotated:
                f.write(np.ascontiguousarray(y.cpu().numpy()).tobytes())
                f.write(np.ascontiguousarray(uv.cpu().numpy()).tobytes())
        return
    for t, im in enumerate(annotated):
        rgb = np.ascontiguousarray(im.cpu().numpy())
        with open(os.path.join(out_dir, f'{t}.ppm'), 'wb') as f:
            f.write(b'P6\n%d %d\n255\n' % (rgb.shape[1], rgb.shape[0]))
            f.write(rgb.tobytes())


def load_detector(spec):
    """'package.module:factory' -> factory()"""
    module, _, factory = spec.partition(':')
    if not module or not factory:
        raise ValueError(f'expected MODULE:FACTORY, got {spec!r}')
    return getattr(importlib.import_module(module), factory)()


def dwell_option(text):
    """--dwell's value -> harness.run_head_video's dwell: '' is True (the defaults), 'ENTER,EXIT' a dict."""
    if not text:
        return True
    try:
        enter, exit = (int(v) for v in text.split(','))
    except ValueError:
        raise SystemExit(f'--dwell takes ENTER,EXIT (two integers), got {text!r}') from None
    return dict(enter=enter, exit=exit)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('frames_dir')
    ap.add_argument('labels_dir')
    ap.add_argument('config')
    ap.add_argument('checkpoint')
    ap.add_argument('--out', required=True)
    ap.add_argument('--precision', default='f16x3', choices=['f16x3', 'fp32', 'f16', 'bf16'])
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--max-len', type=int, default=100)
    ap.add_argument('--batch-frames', type=int, default=448)
    ap.add_argument('--head-class', type=int, default=1)
    ap.add_argument('--ext', default='jpg')
    ap.add_argument('--smooth', type=float, default=None, metavar='ALPHA', help='temporal filter of the reference\'s metric, alpha in (0, 1]')
    ap.add_argument('--nv12', nargs=2, default=None, metavar=('WxH', 'FILE'), help='read the frames from a raw NV12 video (FRAMES_DIR is then -)')
    ap.add_argument('--matrix', default='bt601', choices=['bt601', 'bt709'], help='YUV -> RGB coefficients of --nv12')
    ap.add_argument('--draw', default=None, metavar='OUT', help='write the frames with the gaze arrows drawn into this directory')
    ap.add_argument('--color', default=None, metavar='B,G,R', help='colour of the arrows of --draw')
    ap.add_argument('--overlay', action='store_true', help='--draw with --attention: region outlines, sight lines and arrows coloured by their target '
                                                             '(pipeline.draw_attention) instead of the plain arrows')
    ap.add_argument('--labels', nargs='?', const=2, type=int, default=None, metavar='SCALE',
                    help='--draw: write every person\'s id -- with --dwell the seconds they have looked at their target -- next to the head, SCALE pixels per font bit')
    ap.add_argument('--fps', default=None, metavar='NUM[/DEN]', help='frames per second of the video, for the seconds of --labels (30)')
    ap.add_argument('--predictions', default=None, metavar='DIR', help='raw detector output, <t>.npy per frame, instead of LABELS_DIR (then -)')
    ap.add_argument('--in-shape', default=None, metavar='HxW', help='the letterboxed input of the detector behind --predictions')
    ap.add_argument('--conf-thres', type=float, default=0.25)
    ap.add_argument('--iou-thres', type=float, default=0.45)
    ap.add_argument('--detector', default=None, metavar='MODULE:FACTORY', help='run the head detector FACTORY() returns, instead of LABELS_DIR (then -)')
    ap.add_argument('--img-size', type=int, default=640, help='the letterbox size of --detector')
    ap.add_argument('--half', action='store_true', help='--detector reads half instead of float')
    ap.add_argument('--track', action='store_true', help='identities from the tracker on the device instead of the head count and x1 order')
    ap.add_argument('--slots', type=int, default=16, help='tracks held at once, of --track')
    ap.add_argument('--match-iou', type=float, default=0.3, help='IoU above which a head continues a track, of --track')
    ap.add_argument('--max-age', type=int, default=5, help='frames a track outlives its last detection, of --track')
    ap.add_argument('--track-motion', nargs='?', const='', default=None, metavar='GAIN[,DECAY]',
                    help='--track with the constant-velocity motion model: a head missed for a few frames is looked for where it was going '
                         '(default 0.5,1.0: conventional alpha-beta values, not tuned on data)')
    ap.add_argument('--attention', action='store_true', help='add what every person looks at: another person, a region of --regions, the camera')
    ap.add_argument('--camera', default=None, metavar='FX,FY,CX,CY', help='--attention decided in 3-D (pipeline.gaze_targets_3d): the intrinsics of the camera, in pixels')
    ap.add_argument('--regions3d', default=None, metavar='FILE.json', help='regions of --camera: a JSON list of planar polygons [[x, y, z], ...] of 3 .. 32 vertices in camera coordinates (metres)')
    ap.add_argument('--head-size', type=float, default=0.24, metavar='M', help='with --camera: the size of a head in metres, from which its depth follows (a convention, not tuned on data)')
    ap.add_argument('--gaze-frame', choices=('eye', 'camera'), default='eye', help='with --camera: the gaze is relative to the line from the lens to the head (eye) or to the optical axis (camera)')
    ap.add_argument('--regions', default=None, metavar='FILE.json', help='regions of --attention in frame pixels: a JSON list of rectangles [x1, y1, x2, y2] and polygons [[x, y], ...] of 3 .. 32 vertices')
    ap.add_argument('--dwell', nargs='?', const='', default=None, metavar='ENTER,EXIT',
                    help='--attention with how long every look lasts: episodes with a start, a length and an end (default 3,2: conventions, not '
                         'tuned on data)')
    ap.add_argument('--heat', nargs='?', const='', default=None, metavar='CELL,RADIUS',
                    help='--attention with where the looks land: a heat map of CELL-pixel cells (8) and a splat of RADIUS cells (2), drawn under --draw')
    ap.add_argument('--heat-out', default=None, metavar='FILE.npy', help='write the final grid of --heat, int32 [1, GH, GW]')
    ap.add_argument('--surface-heat', nargs='?', const='', default=None, metavar='GW,GH,RADIUS',
                    help='--camera and --regions3d with where ON each region the looks land: a grid of GW x GH cells (32,32) over every region and a '
                         'splat of RADIUS cells (1) -- conventions, not tuned on data --, drawn back onto the regions under --draw')
    ap.add_argument('--surface-heat-out', default=None, metavar='FILE.npy', help='write the final grids of --surface-heat, int32 [M, GH, GW]')
    ap.add_argument('--anonymize', nargs='?', const=8, type=int, default=None, metavar='BLOCKS',
                    help='--draw with the faces removed first: a mosaic of about BLOCKS cells across every head (8)')
    ap.add_argument('--anonymize-shape', default='ellipse', choices=['ellipse', 'box'], help='what of the grown head box --anonymize covers')
    a = ap.parse_args(argv)
    if a.anonymize is not None and a.draw is None:
        raise SystemExit('--anonymize changes the frames --draw writes: it needs --draw')
    if a.anonymize is not None and not 1 <= a.anonymize <= 64:
        raise SystemExit(f'--anonymize takes BLOCKS in 1 .. 64, got {a.anonymize}')
    anonymize = None if a.anonymize is None else dict(blocks=a.anonymize, shape=a.anonymize_shape)
    if (a.heat is not None or a.heat_out is not None) and not a.attention:
        raise SystemExit('--heat and --heat-out belong to --attention')
    if a.heat_out is not None and a.heat is None:
        a.heat = ''
    heat = None
    if a.heat is not None:
        try:
            values = [int(v) for v in a.heat.split(',')] if a.heat else []
        except ValueError:
            values = None
        if values is None or len(values) > 2:
            raise SystemExit(f'--heat takes CELL or CELL,RADIUS, got {a.heat!r}')
        heat = dict(zip(('cell', 'radius'), values), draw=a.draw is not None)
    if (a.surface_heat is not None or a.surface_heat_out is not None) and (a.camera is None or a.regions3d is None):
        raise SystemExit('--surface-heat and --surface-heat-out belong to --attention --camera --regions3d')
    if a.surface_heat_out is not None and a.surface_heat is None:
        a.surface_heat = ''
    surface = None
    if a.surface_heat is not None:
        try:
            values = [int(v) for v in a.surface_heat.split(',')] if a.surface_heat else []
        except ValueError:
            values = None
        if values is None or len(values) not in (0, 2, 3):
            raise SystemExit(f'--surface-heat takes GW,GH or GW,GH,RADIUS, got {a.surface_heat!r}')
        surface = dict(draw=a.draw is not None, **(dict(grid=tuple(values[:2])) if values else {}), **(dict(radius=values[2]) if len(values) == 3 else {}))
    if a.regions is not None and not a.attention:
        raise SystemExit('--regions belongs to --attention')
    if a.dwell is not None and not a.attention:
        raise SystemExit('--dwell belongs to --attention')
    if a.camera is not None and not a.attention:
        raise SystemExit('--camera belongs to --attention')
    if a.camera is None and (a.regions3d is not None or a.head_size != 0.24 or a.gaze_frame != 'eye'):
        raise SystemExit('--regions3d, --head-size and --gaze-frame belong to --camera')
    dwell = None if a.dwell is None else dwell_option(a.dwell)
    attention = None
    if a.attention:
        attention = {}
        if a.regions is not None:
            with open(a.regions) as f:
                attention['regions'] = json.load(f)
        if a.camera is not None:                              # targets in 3-D: camera space instead of the image plane
            try:
                attention['camera'] = [float(v) for v in a.camera.split(',')]
            except ValueError:
                attention['camera'] = []
            if len(attention['camera']) != 4:
                raise SystemExit(f'--camera takes FX,FY,CX,CY, got {a.camera!r}')
            attention.update(head_size=a.head_size, frame=a.gaze_frame)
            if a.regions3d is not None:
                with open(a.regions3d) as f:
                    attention['regions3d'] = json.load(f)
    track = dict(slots=a.slots, match_iou=a.match_iou, max_age=a.max_age) if a.track or a.track_motion is not None else None
    if a.track_motion is not None:
        try:
            values = [float(v) for v in a.track_motion.split(',')] if a.track_motion else []
        except ValueError:
            values = None
        if values is None or len(values) > 2:
            raise SystemExit(f'--track-motion takes GAIN or GAIN,DECAY, got {a.track_motion!r}')
        track['motion'] = dict(zip(('gain', 'decay'), values))
    if (a.predictions is None) != (a.in_shape is None):
        raise SystemExit('--predictions and --in-shape go together')
    if a.detector is not None and a.predictions is not None:
        raise SystemExit('--detector takes the place of --predictions')
    draw = None
    if a.draw is not None:
        draw = {} if a.color is None else dict(color=parse_color(a.color))
    if a.overlay:
        if a.draw is None or not a.attention or a.color is not None:
            raise SystemExit('--overlay belongs to --draw and --attention, and its colours are the palette\'s (no --color)')
        draw['overlay'] = True
    if a.labels is not None or a.fps is not None:
        if a.draw is None:
            raise SystemExit('--labels and --fps belong to --draw')
        labels = {} if a.labels is None else dict(scale=a.labels)
        if a.fps is not None:
            try:
                num, _, den = a.fps.partition('/')
                labels['fps'] = (int(num), int(den or 1))
            except ValueError:
                raise SystemExit(f'--fps takes NUM or NUM/DEN, got {a.fps!r}')
        draw['labels'] = labels or True
    if a.nv12 is not None:
        frames = Nv12File(a.nv12[1], *parse_size(a.nv12[0]))
        n = len(frames)
    else:
        n = len([f for f in os.listdir(a.frames_dir) if f.endswith('.' + a.ext)])      # the notebook: vid_len = len(os.listdir(frames))
        missing = [t for t in range(n) if not os.path.exists(os.path.join(a.frames_dir, f'{t}.{a.ext}'))]
        if missing:
            raise SystemExit(f'{a.frames_dir}: {n} .{a.ext} files but no {missing[0]}.{a.ext} -- frames are numbered from 0 without gaps')
        frames = Frames(a.frames_dir, n, a.ext)
    per_frame = detections = None
    if a.detector is not None:
        detections = dict(detector=load_detector(a.detector), new_shape=a.img_size, dtype=torch.float16 if a.half else torch.float32,
                          only_class=a.head_class, conf_thres=a.conf_thres, iou_thres=a.iou_thres)
    elif a.predictions is not None:
        in_h, _, in_w = a.in_shape.lower().partition('x')
        raw = [np.load(os.path.join(a.predictions, f'{t}.npy')) for t in range(n)]
        pred = np.stack([r.reshape(r.shape[-2], r.shape[-1]) for r in raw]) if n else np.zeros((0, 1, 6), np.float32)
        detections = dict(pred=pred, in_shape=(int(in_h), int(in_w)), only_class=a.head_class, conf_thres=a.conf_thres, iou_thres=a.iou_thres)
    else:
        labels = [os.path.join(a.labels_dir, f'{t}.txt') for t in range(n)]
        per_frame = [harness.read_head_labels(p, a.head_class) if os.path.exists(p) else [] for p in labels]
    model = init_detector(a.config, a.checkpoint, device=a.device, precision=a.precision)
    pipe = DevicePipeline(model.cfg.data.test.pipeline)
    res = harness.run_head_video(model.engine(), pipe, frames, per_frame, max_len=a.max_len, batch_frames=a.batch_frames, rgb=True,
                                 smooth=a.smooth, pixel_format='bgr' if a.nv12 is None else 'nv12', matrix=a.matrix, detections=detections, draw=draw,
                                 track=track, attention=attention, dwell=dwell, heat=heat, anonymize=anonymize, surface_heat=surface)
    as_json = lambda v: list(v) if isinstance(v, tuple) else v
    if surface is not None:                               # the grids come last, after everything a run without the option returns
        res, grids = res[:-1], res[-1]
        res = res[0] if len(res) == 1 else res
        if a.surface_heat_out is not None:
            np.save(a.surface_heat_out, grids)
    if heat is not None:
        res, grid = res[:-1], res[-1]
        res = res[0] if draw is None else res
        if a.heat_out is not None:
            np.save(a.heat_out, grid)
    if draw is not None:
        res, annotated = res
        write_annotated(a.draw, annotated, a.nv12 is not None)
    out = [dict(segment=r['id'][0], person=r['id'][1], frame_id=r['frame_id'], head_box=r['head_box'].tolist(), crop=r['crop'].tolist(),
                gaze=r['fused'].tolist(), arrow=r['arrow'].tolist(), det=r['det'].tolist(), others=r['others'].tolist(),
                **({} if a.smooth is None else dict(gaze_smooth=r['fused_smooth'].tolist())),
                **({} if attention is None else dict(target_kind=r['target_kind'].tolist(), target_id=[None if v is None else list(v) for v in r['target_id']],
                                                     target_region=r['target_region'].tolist(), target_hit=r['target_hit'].tolist(),
                                                     mutual=r['mutual'].tolist())),
                **({} if attention is None or 'camera' not in attention else dict(target_hit3d=r['target_hit3d'].tolist())),
                **({} if dwell is None else dict(dwell_kind=r['dwell_kind'].tolist(), dwell_frames=r['dwell_frames'].tolist(),
                                                 episodes=[{k: as_json(v) for k, v in e.items()} for e in r['episodes']]))) for r in res]
    with open(a.out, 'w') as f:
        json.dump(dict(frames=n, tracks=out), f)
    print(f'{n} frames, {len(out)} (segment, person) tracks, {sum(len(r["frame_id"]) for r in out)} head crops -> {a.out}')


if __name__ == '__main__':
    main()
