"""CPU: the host side of frame reuse across overlapping windows (mcgaze_amd/stream.py) -- which windows of the final plan are certain
while a stream grows, which frames are final, the window-by-window merge against harness.merge_video, and the host check of a
window-frame -> pyramid-row table.  No device."""
import numpy as np
import pytest
import torch

from mcgaze_amd import harness
from mcgaze_amd.lib import McgError
from mcgaze_amd.stream import StreamMerger, WindowPlanner


def fake_window(a, b, L):
    """A deterministic per-window output (det [T,3,5], fused [T,3], others [T,3,3]) that depends on the frame ids AND the window, so
    that overlapping frames really get averaged; some scores below the 0.5 threshold."""
    f = np.arange(a, b, dtype=np.float64)[:, None, None]
    q = np.arange(3, dtype=np.float64)[None, :, None]
    w = (a * 7 + b * 13 + L) % 17
    det = np.concatenate([np.sin(f * 1.3 + q * 0.7 + np.arange(4)[None, None, :] + w) * 100,
                          (np.cos(f * 0.9 + q + w * 0.31) + 1) / 2], axis=-1).astype(np.float32)
    fused = np.sin(f[:, :, 0] * 0.37 + np.arange(3)[None] + w).astype(np.float32)
    others = np.cos(f * 0.21 + q * 1.1 + np.arange(3)[None, None, :] * 0.5 + w).astype(np.float32)
    return det, fused, others


def pushes(L, pattern, rs):
    if pattern == 'all':
        return [L] if L else []
    if pattern == 'one':
        return [1] * L
    out, left = [], L
    while left:
        k = min(left, int(rs.randint(1, 10)))
        out.append(k)
        left -= k
    return out


def run_stream(L, clip_len, stride, sizes):
    """Drive planner + merger like GazeStream.push / finish do, with the fake engine; check finality on the way."""
    pl, mg = WindowPlanner(clip_len, stride), StreamMerger()
    got, windows, emitted = [], [], 0
    for k in sizes:
        before = pl.frames
        wins = pl.feed(k)
        assert pl.frames == before + k
        for w in wins:
            assert w[1] <= pl.frames                         # a certain window only reads frames that arrived
            mg.add(w, *fake_window(w[0], w[1], 0))
        windows += wins
        upto = pl.final_upto
        assert upto >= emitted
        # no window handed out later may touch a frame emitted now: every later window starts at or after frames - clip_len, and
        # every regular one at or after the next regular start
        assert upto <= max(0, pl.frames - clip_len) and upto <= pl.next * stride
        part = mg.pop(upto)
        emitted += part[0].shape[0]
        got.append(part)
    wins = pl.finish()
    for w in wins:
        mg.add(w, *fake_window(w[0], w[1], 0))
    windows += wins
    got.append(mg.pop(pl.frames))
    return windows, got


@pytest.mark.parametrize('clip_len', [3, 7])
@pytest.mark.parametrize('stride', range(1, 8))
def test_planner_and_merger_reproduce_plan_and_merge(clip_len, stride):
    if stride > clip_len:
        with pytest.raises(ValueError):
            WindowPlanner(clip_len, stride)
        return
    rs = np.random.RandomState(clip_len * 10 + stride)
    for L in range(1, 41):
        plan = harness.plan_windows(L, clip_len, stride)
        want = harness.merge_video(plan, [fake_window(a, b, 0) for a, b, _ in plan])
        for pattern in ('all', 'one', 'random', 'random'):
            windows, got = run_stream(L, clip_len, stride, pushes(L, pattern, rs))
            assert windows == plan, (L, pattern)
            for i in range(3):
                cat = np.concatenate([g[i] for g in got])
                assert cat.shape == want[i].shape, (L, pattern, i)
                assert np.array_equal(cat.view(np.uint32), want[i].view(np.uint32)), (L, pattern, i)


def test_no_frame_is_emitted_before_it_is_final():
    """A frame handed out must not change afterwards: emit, then compare with the finished merge of the same stream."""
    for L in (8, 9, 16, 33):
        pl, mg = WindowPlanner(7, 4), StreamMerger()
        early = {}
        for _ in range(L):
            for w in pl.feed(1):
                mg.add(w, *fake_window(w[0], w[1], 0))
            base = mg.base
            d, f, o = mg.pop(pl.final_upto)
            for j in range(d.shape[0]):
                early[base + j] = (d[j].copy(), f[j].copy(), o[j].copy())
        plan = harness.plan_windows(L)
        want = harness.merge_video(plan, [fake_window(a, b, 0) for a, b, _ in plan])
        assert early, L
        for j, (d, f, o) in early.items():
            assert np.array_equal(d, want[0][j]) and np.array_equal(f, want[1][j]) and np.array_equal(o, want[2][j]), (L, j)
        # frames inside the last clip_len are never final before finish(): the flush-to-end window may still cover them
        assert max(early) < L - 7 + 1


def test_planner_keep_from_and_short_streams():
    pl = WindowPlanner(7, 4)
    assert pl.feed(7) == [] and pl.keep_from == 0      # 7 frames: could still be the single short window of an L = 7 video
    assert pl.feed(1) == [(0, 7, 3)] and pl.keep_from == 1
    assert pl.finish() == [(1, 8, 6)]
    pl = WindowPlanner(7, 4)
    pl.feed(5)
    assert pl.finish() == [(0, 5, 0)]
    with pytest.raises(McgError):
        pl.feed(1)
    assert WindowPlanner(7, 4).finish() == []


def test_frame_table_is_checked_on_the_host():
    from mcgaze_amd.engine import check_frame_table
    assert check_frame_table([0, 1, 2, 2, 1, 0, 3], 4, 7).dtype == np.int32
    assert check_frame_table(torch.arange(14, dtype=torch.int64) % 5, 5, 7).tolist() == [i % 5 for i in range(14)]
    for bad, K, T in (([0, 1, 2, 3, 4, 5, 7], 7, 7),      # row 7 of a 7-row store
                      ([0, 1, 2, 3, 4, 5, -1], 7, 7),     # negative
                      ([0, 1, 2, 3, 4, 5], 7, 7),         # not a multiple of clip_length
                      ([], 7, 7),                         # empty
                      ([[0, 1, 2, 3, 4, 5, 6]], 7, 7),    # not flat
                      ([0.0] * 7, 7, 7),                  # not integers
                      ([0] * 7, 0, 7)):                   # empty store
        with pytest.raises(McgError):
            check_frame_table(bad, K, T)


def test_decode_rejects_a_bad_host_table_before_touching_the_device():
    """HipEngine.decode range-checks a host table first: a table that reaches past the store raises McgError, with no device."""
    from mcgaze_amd.engine import HipEngine
    e = object.__new__(HipEngine)          # no weights, no device: the check comes before either is needed
    pyr = [torch.empty(4, 56 >> i, 56 >> i, 256) for i in range(4)]
    with pytest.raises(McgError, match=r'\[0, 4\)'):
        e.decode(pyr, [0, 1, 2, 3, 4, 0, 1], 7)
    with pytest.raises(McgError, match='multiple of clip_length'):
        e.decode(pyr, [0, 1, 2, 3, 0, 1], 7)
