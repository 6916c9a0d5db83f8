"""What tests/test_gpu_live.py and tests/test_gpu_live_lanes.py share: the set-up (96 x 128 frames, synthetic weights, 64 x 64 crops), the
bit-for-bit compare and ``run_live``, a scene of tests/live_cases.py or tests/live_lanes_cases.py through live.LiveGaze.  A plain module:
each test file makes its own module-scoped fixtures from make_engine and make_pipe."""
import ctypes as C

import numpy as np
import torch

from mcgaze_amd import lib as L
from mcgaze_amd import live, synth
from mcgaze_amd import pipeline as P
from tests import live_cases as LC
from tests import live_lanes_cases as LL
from tests.test_gpu_nv12 import chain

DEV = 'cuda:0'
ALPHA = 0.6
H, W = LC.FRAME_HW
GAZE = ('det', 'fused', 'others')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_frames(seed):
    """[TICKS, 96, 128, 3] uint8: one frame per tick of one camera."""
    return np.random.default_rng(seed).integers(0, 256, (LC.TICKS, H, W, 3), dtype=np.uint8)


CAMS = (make_frames(1), make_frames(2))


def make_engine():
    from mcgaze_amd.engine import HipEngine
    return HipEngine(synth.make_state_dict(0), precision='f16x3')


def make_pipe():
    return P.DevicePipeline(chain(64))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, a.shape, b.dtype, b.shape)
    assert np.array_equal(bits(a), bits(b)), what


def call(name, *args):
    """One entry of the library on the current stream: a tensor goes as its address, None as a null pointer, an int as it is."""
    ptr = lambda a: C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else C.c_void_p(0) if a is None else a
    L.check(getattr(L.load(), name)(C.c_void_p(torch.cuda.current_stream().cuda_stream), *map(ptr, args)), name)


def run_live(engine, pipe, variant, cams=CAMS, lanes=None, smooth=ALPHA, draw=False):
    """A scene through LiveGaze(lanes=lanes) (None: the fixed schedule) -> dict of host arrays: the results concatenated over all returned
    frames, ``ticks`` (what each tick left in the object's tables and returned), ``calls`` ((first, k) of every call) and, with draw,
    ``frames`` [(frame index, [Q annotated frames])]."""
    boxes, counts = LL.scene(variant)
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=smooth, draw=draw, lanes=lanes, **LC.OPTIONS)
    bufs = [torch.empty(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(LC.Q)]      # a camera's buffer, rewritten every tick
    ticks, results = [], []
    for t in range(LC.TICKS):
        for q in range(LC.Q):
            bufs[q].copy_(dev(cams[q][t]))
        r = lg.tick(bufs, dev(boxes[t]), dev(counts[t]))
        row = t % lg.R
        ticks.append(dict(crop_boxes=lg.crop_boxes.clone(), image_of=lg.image_of.clone(), ring_id=lg.ring_id[row].clone(),
                          ring_box=lg.ring_box[row].clone(), matched=r['matched'], flags=r['flags']))
        if lanes is not None:
            ticks[-1].update(lane_state=lg.lane_state.clone(), ring_col=lg.ring_col[row].clone(), lane_of=r['lane_of'], overflow=r['overflow'])
        results.append(r)
    results.append(lg.finish())
    torch.cuda.synchronize()
    out = dict(calls=[(r['first'], int(r['valid'].shape[0])) for r in results],
               ticks=[{k: v.cpu().numpy() for k, v in rec.items()} for rec in ticks])
    names = ('track_id', 'valid', 'head_box', 'image_of') + GAZE + (('smooth_valid', 'fused_smooth', 'others_smooth') if smooth else ()) + \
        (('camera', 'slot') if lanes is not None else ())
    for name in names:
        out[name] = torch.cat([r[name] for r in results]).cpu().numpy()
    if draw:
        out['frames'] = [(r['first'] + i, [f.cpu().numpy() for f in fr]) for r in results for i, fr in enumerate(r['frames'])]
    return out
