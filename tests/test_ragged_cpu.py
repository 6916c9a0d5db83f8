"""Ragged batches on the host (-m "not gpu"): the clip-length check, the demo's chunking rule, the mixed-length bucketing of the
harness with a fake engine, and the C-ABI surface of the four mcg_*_ragged entry points (no compute calls here)."""
import os
import re

import numpy as np
import pytest
import torch

from mcgaze_amd import harness
from mcgaze_amd import lib as L
from mcgaze_amd.engine import check_clip_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ['mcg_stage_forward_ragged', 'mcg_decoder_forward_ragged', 'mcg_decoder_forward_deferred_ragged', 'mcg_clip_forward_ragged']


def test_check_clip_lengths_accepts():
    for lengths, want in (([7, 3, 12], [0, 7, 10, 22]), ((1,), [0, 1]), (np.array([2, 2], dtype=np.int64), [0, 2, 4]),
                          (torch.tensor([5, 1, 1]), [0, 5, 6, 7]), ([101, 7, 7], [0, 101, 108, 115])):
        start = check_clip_lengths(lengths, want[-1])
        assert start.dtype == np.int32 and start.tolist() == want


@pytest.mark.parametrize('lengths,n', [([], 0),                   # empty
                                       ([7, 0, 3], 10),           # a clip without frames
                                       ([7, -1, 4], 10),          # negative
                                       ([7, 3], 11),              # sum != num_frames
                                       ([7, 3], 9),
                                       ([7.0, 3.0], 10),          # not integers
                                       ([[7, 3]], 10),            # not flat
                                       ([[7], [3, 1]], 11)])      # ragged nesting
def test_check_clip_lengths_rejects(lengths, n):
    with pytest.raises(L.McgError):
        check_clip_lengths(lengths, n)


def test_plan_track_chunks_is_the_demo_flush_rule():
    """MCGaze_demo/demo.ipynb, cell 4, max_len = 100: frames are appended one by one; a clip is run when ``len(datas) > max_len`` (the
    101st frame has just been appended) or at the track's last frame.  By hand:
      0   frames: the loop body never runs                              -> no clip
      1   frame : j = 0 is the last frame                               -> [0, 1)
      100 frames: never more than 100 held; flushed at j = 99 (last)    -> [0, 100)
      101 frames: at j = 100 both conditions hold, ONE flush of 101     -> [0, 101)
      102 frames: 101 held at j = 100 -> flush; j = 101 is the last     -> [0, 101), [101, 102)
      230 frames: flushes at j = 100, j = 201 and j = 229 (last)        -> [0, 101), [101, 202), [202, 230)"""
    want = {0: [], 1: [(0, 1)], 100: [(0, 100)], 101: [(0, 101)], 102: [(0, 101), (101, 102)], 230: [(0, 101), (101, 202), (202, 230)]}
    for n, chunks in want.items():
        assert harness.plan_track_chunks(n, 100) == chunks, n

    def demo(n, max_len):                      # the notebook's loop itself, on frame indices
        out, datas = [], []
        for j in range(n):
            datas.append(j)
            if len(datas) > max_len or j == n - 1:
                out.append((datas[0], datas[-1] + 1))
                datas = []
        return out
    for n in (0, 1, 2, 3, 4, 7, 100, 101, 102, 230, 303):
        for max_len in (1, 2, 100):
            assert harness.plan_track_chunks(n, max_len) == demo(n, max_len), (n, max_len)


class FakeEngine:
    """Stands in for HipEngine on the host: records how it is called and returns values that depend on the frame's CONTENT only (like the
    real engine's, whose results do not depend on the batch), so that any bucketing must give the same records."""
    device = torch.device('cpu')

    def __init__(self):
        self.calls = []

    def _out(self, x):
        n = x.shape[0]
        v = x.reshape(n, -1)[:, :3].double()                                  # three pixels identify the frame
        s = (v.sum(1, keepdim=True) * 0.37).sin().float()
        gaze = torch.stack([(v * (k + 1)).cos().float() for k in range(4)])  # [4, n, 3]
        boxes = (s[:, :, None] * 10 + torch.arange(12, dtype=torch.float32).reshape(1, 3, 4)).float()
        scores = (0.5 + 0.5 * (v * 1.7).sin()).float()                        # both sides of the person threshold
        return dict(gaze=gaze, boxes=boxes, scores=scores)

    def forward(self, x, clip_length, img_hw=None):
        self.calls.append(('forward', tuple(x.shape), clip_length))
        return self._out(x)

    def backbone_fpn(self, x):
        return x

    def decode(self, pyramid, frame_of, clip_length, img_hw=None):
        self.calls.append(('decode', tuple(pyramid.shape), clip_length))
        return self._out(pyramid[torch.as_tensor(frame_of, dtype=torch.long)])


def _videos():
    g = torch.Generator().manual_seed(3)
    spec = [(3, 32, 32), (7, 32, 32), (8, 32, 32), (12, 32, 32), (30, 32, 32), (2, 32, 64), (5, 32, 64), (1, 32, 32)]
    return [dict(id=i, frames=torch.randn(n, 3, h, w, generator=g)) for i, (n, h, w) in enumerate(spec)]


@pytest.mark.parametrize('reuse_frames', [False, True])
def test_run_windows_mixed_lengths_buckets_by_shape_and_class(reuse_frames):
    """clip_len = 12, stride 5: windows of 3, 7, 8, 12 (x 1), 12 (x 5: the 30-frame video) and 1 frames at 32 x 32, of 2 and 5 frames at
    32 x 64.  Mixed bucketing: (32, 32, T <= 10) holds [3, 7, 8, 1], (32, 32, T > 10) the six 12-frame windows, (32, 64, T <= 10) holds
    [2, 5] -- three calls, each with its list of lengths; the default bucketing makes one call per distinct (T, H, W) = seven."""
    videos = _videos()
    base = FakeEngine()
    want = harness.run_videos(base, videos, clip_len=12, stride=5, batch_clips=64, reuse_frames=reuse_frames)
    assert len(base.calls) == 7 and all(isinstance(c[2], int) for c in base.calls)
    fake = FakeEngine()
    got = harness.run_videos(fake, videos, clip_len=12, stride=5, batch_clips=64, reuse_frames=reuse_frames, mixed_lengths=True)
    assert got == want
    kind = 'decode' if reuse_frames else 'forward'
    assert [c[0] for c in fake.calls] == [kind] * 3
    by_key = {(c[1][2], c[1][3], max(c[2]) > 10): list(c[2]) for c in fake.calls}
    assert by_key == {(32, 32, False): [3, 7, 8, 1], (32, 32, True): [12] * 6, (32, 64, False): [2, 5]}
    frames = {c[1][2:] + (max(c[2]) > 10,): c[1][0] for c in fake.calls}
    if reuse_frames:     # the 30-frame video's windows (0-12, 5-17, ..., 18-30) share frames: 30 distinct rows, not 72
        assert frames == {(32, 32, False): 19, (32, 32, True): 12 + 30, (32, 64, False): 7}
    else:
        assert frames == {(32, 32, False): 19, (32, 32, True): 72, (32, 64, False): 7}


def test_run_windows_mixed_lengths_flushes_full_buckets():
    """batch_clips = 2: a bucket runs as soon as it holds two windows, whatever their lengths."""
    videos = _videos()[:4]                                             # 3, 7, 8, 12 frames -> windows 3, 7, (7, 7), (7, 7, 7)
    want = harness.run_videos(FakeEngine(), videos, batch_clips=2)
    fake = FakeEngine()
    assert harness.run_videos(fake, videos, batch_clips=2, mixed_lengths=True) == want
    assert [list(c[2]) for c in fake.calls] == [[3, 7], [7, 7], [7, 7], [7]]


def test_run_tracks_batches_chunks_of_all_tracks():
    """Tracks of 5, 24, 3 and 11 frames, max_len = 10 (chunks of 11): chunks 5 | 11, 11, 2 | 3 | 11.  Chunks of at most 10 frames
    ([5, 2, 3]) share one call, the 11-frame ones run in calls of at most batch_frames = 22 frames; every track's rows are its chunks'
    outputs in order."""
    g = torch.Generator().manual_seed(9)
    tracks = [dict(id=f'p{i}', frames=torch.randn(n, 3, 32, 32, generator=g)) for i, n in enumerate((5, 24, 3, 11, 0))]
    fake = FakeEngine()
    out = harness.run_tracks(fake, tracks, max_len=10, batch_frames=22)
    assert sorted(list(c[2]) for c in fake.calls) == [[5, 2, 3], [11], [11, 11]]
    assert [o['id'] for o in out] == ['p0', 'p1', 'p2', 'p3', 'p4']
    for t, o in zip(tracks, out):
        n = t['frames'].shape[0]
        assert o['det'].shape == (n, 3, 5) and o['fused'].shape == (n, 3) and o['others'].shape == (n, 3, 3)
        if n == 0:
            continue
        ref = fake._out(t['frames'])
        assert np.array_equal(o['det'][..., :4], ref['boxes'].numpy()) and np.array_equal(o['det'][..., 4], ref['scores'].numpy())
        assert np.array_equal(o['fused'], ref['gaze'][0].numpy())
        assert np.array_equal(o['others'], ref['gaze'][1:].permute(1, 0, 2).numpy())


def test_header_declares_and_binding_exports_the_ragged_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    for name in RAGGED:
        m = re.search(r'\bint ' + name + r'\s*\(([^;]*)\);', hdr)
        assert m, name
        args = m.group(1)
        assert re.search(r'const int\* clip_start,\s*int num_clips,\s*int max_clip_length', args), name
        assert 'clip_length,' not in args.replace('max_clip_length,', ''), name
        assert name in L.EXPORTS
    assert 'frame_of' in re.search(r'mcg_decoder_forward_ragged\s*\(([^;]*)\);', hdr).group(1)
    assert int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) == L.ABI_VERSION >= 16
    lib = L.load()
    for name in RAGGED:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
