"""-m gpu: frame reuse across overlapping windows -- the trunk writes each distinct frame into one row of a pyramid store, the decoder
reads its windows' frames through a device index table (mcg_roi_align_indexed, mcg_decoder_forward_indexed, HipEngine.decode,
harness.run_videos(reuse_frames=True), stream.GazeStream).  Everything here is asserted BIT FOR BIT against the per-window path.
No test hands the kernels an out-of-range table: the guard is there for callers, not to be provoked."""
import os

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd.stream import GazeStream, PyramidRing

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PRECISIONS = ('fp32', 'f16x3', 'bf16', 'f16')


@pytest.fixture(scope='module')
def engines():
    from mcgaze_amd.engine import HipEngine
    sd = synth.make_state_dict(0)
    return {p: HipEngine(sd, precision=p) for p in PRECISIONS}


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def video(seed, L, H=224, W=224):
    return torch.from_numpy(synth.make_clips(seed, 1, L, H, W))


def img_hw_of(L, seed, H=224, W=224):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(H // 2, H + 1, L), rs.randint(W // 2, W + 1, L)], axis=1).astype(np.int32)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_trunk_rows_do_not_depend_on_the_batch(engines, precision):
    """A 33-frame video as one trunk call and as calls of 1, 4 and 7 frames into a 16-row ring (wrapping): every row bit-identical.
    33 x 56 x 56 rows cross the M thresholds of the streaming 1x1 kernels (pw_single*.hpp: M >= 64 Ki), the small calls do not."""
    e = engines[precision]
    x = video(11, 33).to(DEV)
    whole = [p.clone() for p in e.backbone_fpn(x)]
    ring = PyramidRing(e, 16, 224, 224)
    sizes, f = [1, 4, 7], 0
    for k in range(100):
        n = min(sizes[k % 3], 33 - f)
        if n == 0:
            break
        ring.release(ring.count)
        rows = ring.append(x[f:f + n])
        torch.cuda.synchronize()
        for j, r in enumerate(rows):
            for lvl in range(4):
                assert torch.equal(bits(ring.levels[lvl][r]), bits(whole[lvl][f + j])), (precision, f + j, lvl, n)
        f += n
    assert f == 33 and ring.count == 33


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_roi_align_indexed_equals_plain(engines, precision):
    from mcgaze_amd.engine import roi_align, roi_align_indexed
    e = engines[precision]
    x = video(12, 6).to(DEV)
    pyr = e.backbone_fpn(x)
    rs = np.random.RandomState(3)
    xy = rs.uniform(0, 150, (6, 3, 2)).astype(np.float32)
    wh = rs.uniform(8, 200, (6, 3, 2)).astype(np.float32)
    boxes = torch.from_numpy(np.concatenate([xy, xy + wh], -1)).to(DEV)
    ref, ref_lv = roi_align(pyr, boxes)
    out, lv = roi_align_indexed(pyr, boxes, list(range(6)))
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(ref)) and torch.equal(lv, ref_lv)
    perm = [4, 0, 5, 2, 1, 3]                               # store row r holds frame perm[r]
    inv = [perm.index(n) for n in range(6)]
    store = [p[perm].contiguous() for p in pyr]
    out, lv = roi_align_indexed(store, boxes, inv)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(ref)) and torch.equal(lv, ref_lv)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_decode_equals_forward(engines, precision):
    e = engines[precision]
    # identity table over the trunk of the same frames
    x = video(13, 14).to(DEV)
    ref = {k: v.clone() for k, v in e.forward(x, 7).items()}
    out = e.decode(e.backbone_fpn(x), list(range(14)), 7)
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(out[k], ref[k]), (precision, k)
    # windows that share frames, a row-shuffled store, non-square img_shape per frame
    L = 12
    v = video(14, L).to(DEV)
    hw = img_hw_of(L, 5)
    wins = [(0, 7), (4, 11), (5, 12)]
    stacked = torch.cat([v[a:b] for a, b in wins]).contiguous()
    ref = {k: t.clone() for k, t in e.forward(stacked, 7, img_hw=np.concatenate([hw[a:b] for a, b in wins])).items()}
    order = np.random.RandomState(1).permutation(L)       # store row r holds frame order[r]
    row_of = np.argsort(order)
    store = e.backbone_fpn(v[torch.from_numpy(order).to(DEV)].contiguous())
    table = [int(row_of[f]) for a, b in wins for f in range(a, b)]
    for tab in (table, torch.tensor(table, dtype=torch.int32, device=DEV)):
        out = e.decode(store, tab, 7, img_hw=hw[order])
        torch.cuda.synchronize()
        for k in ref:
            assert torch.equal(out[k], ref[k]), (precision, k, type(tab))


LENGTHS = [3, 7, 8, 9, 16, 33, 100]


@pytest.mark.parametrize('precision', ['fp32', 'f16x3', 'bf16'])
def test_run_videos_reuse_frames_equals_the_default_path(engines, precision):
    e = engines[precision]
    videos = [dict(id=i + 1, frames=video(60 + i, L), img_hw=img_hw_of(L, 70 + i)) for i, L in enumerate(LENGTHS)]
    sf = (1.4, 1.25, 1.4, 1.25)
    base = harness.run_videos(e, videos, scale_factor=sf)
    base_trunk = harness.last_run_stats['trunk_frames']
    reuse = harness.run_videos(e, videos, scale_factor=sf, reuse_frames=True)
    assert reuse == base
    windows7 = sum(len(harness.plan_windows(L)) for L in LENGTHS if L > 7)
    assert base_trunk == 7 * (windows7 + 1) + 3                 # L = 7 is one window of 7, L = 3 one of 3
    assert harness.last_run_stats['trunk_frames'] == sum(LENGTHS)   # one flush per window length: every frame once
    # batches that cut videos: shared frames of windows in different batches are recomputed, results unchanged
    base = harness.run_videos(e, videos, scale_factor=sf, batch_clips=5)
    reuse = harness.run_videos(e, videos, scale_factor=sf, batch_clips=5, reuse_frames=True)
    assert reuse == base
    assert sum(LENGTHS) <= harness.last_run_stats['trunk_frames'] < 7 * (windows7 + 1) + 3


def stream_record(s, vid, frames, sizes, img_hw=None):
    parts, f = [], 0
    for n in sizes:
        r = s.push(frames[f:f + n], None if img_hw is None else img_hw[f:f + n])
        assert r['first'] == sum(p['det'].shape[0] for p in parts)
        parts.append(r)
        f += n
    parts.append(s.finish())
    cat = [np.concatenate([p[k] for p in parts]) for k in ('det', 'fused', 'others')]
    return harness.video_record(vid, *cat)


@pytest.mark.parametrize('precision', ['f16x3', 'f16'])
def test_gaze_stream_equals_run_videos(engines, precision):
    e = engines[precision]
    limit = 12 if precision == 'f16' else None              # the fp16 decoder keeps its bits below 256 tokens per call
    rs = np.random.RandomState(8)
    sf = (1.4, 1.4, 1.4, 1.4)
    for L, stride in ((33, 4), (33, 1), (5, 4), (12, 4)):
        v = video(80 + L, L).to(DEV)
        hw = img_hw_of(L, 90 + L)
        want = harness.run_videos(e, [dict(id=7, frames=v, img_hw=hw)], stride=stride, scale_factor=sf, batch_clips=limit or 64)[0]
        rnd = []
        while sum(rnd) < L:
            rnd.append(min(L - sum(rnd), int(rs.randint(1, 10))))
        for sizes in ([1] * L, [3] * (L // 3) + ([L % 3] if L % 3 else []), rnd):
            for cap in (12, None):                          # 12 rows: the ring wraps several times
                s = GazeStream(e, 224, 224, stride=stride, capacity=cap, scale_factor=sf, max_decode_windows=limit)
                got = stream_record(s, 7, v, sizes, hw)
                assert got == want, (precision, L, stride, sizes, cap)


def test_gaze_stream_from_the_registry_model():
    from mcgaze_amd import init_detector
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = init_detector(os.path.join(root, 'configs', 'mcgaze', 'r50_clip7_gaze360.py'), None, device=DEV, precision='f16x3')
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(0).items()}, strict=True)
    v = video(99, 19).to(DEV)
    a = stream_record(GazeStream(model, 224, 224), 1, v, [2] * 9 + [1])
    b = stream_record(GazeStream(model.engine(), 224, 224), 1, v, [5, 5, 9])
    c = harness.run_videos(model.engine(), [dict(id=1, frames=v)])[0]
    assert a == b == c
