"""CPU: the host side of many live streams on one pyramid store (mcgaze_amd/stream.py: PyramidStore, GazeStreamPool) -- rows from a free
list, one trunk write and one decoder call per step over every stream, per-stream merge and release -- against harness.merge_video over
plan_windows(L), with a fake engine whose outputs are a pure function of the frames a window holds.  No device."""
import numpy as np
import pytest
import torch

from mcgaze_amd import harness
from mcgaze_amd.engine import HipEngine, check_row_table
from mcgaze_amd.lib import McgError
from mcgaze_amd.stream import GazeStreamPool, PyramidStore

H = W = 32


def window_out(tags):
    """Engine-layout outputs (gaze [4,T,3], boxes [T,3,4], scores [T,3]) of ONE window, a function of the frame tags it holds: every frame's
    values depend on the whole window, so the overlap merge really averages; some scores fall below the 0.5 threshold."""
    t = np.asarray(tags, dtype=np.float64)
    w = float((t * np.arange(1, t.size + 1)).sum() % 17)
    f, q = t[:, None, None], np.arange(3, dtype=np.float64)[None, :, None]
    boxes = np.sin(f * 1.3 + q * 0.7 + np.arange(4)[None, None, :] + w) * 100
    scores = (np.cos(f * 0.9 + q + w * 0.31) + 1)[..., 0] / 2
    gaze = np.cos(f[None] * 0.21 + q[None] * 1.1 + np.arange(4)[:, None, None, None] * 0.5 + w)[..., 0]
    return gaze.astype(np.float32), boxes.astype(np.float32), scores.astype(np.float32)


class FakeEngine:
    """backbone_fpn_rows records (frame tag -> row), decode returns window_out of the tags its table reads.  A frame's tag is its pixel
    value.  Also the bookkeeping checks: no row is written while live, no row is read that no frame was written to."""
    dtype, device = torch.float32, torch.device('cpu')

    def __init__(self):
        self.tag_of_row, self.live = {}, set()
        self.writes, self.decodes = [], []

    def backbone_fpn_rows(self, img, store_levels, rows, chunk_frames=0):
        rows = check_row_table(rows, store_levels[0].shape[0], img.shape[0])
        self.writes.append(len(rows))
        for x, r in zip(img, rows.tolist()):
            assert r not in self.live, f'row {r} handed out while a pending window still reads it'
            self.live.add(r)
            self.tag_of_row[r] = int(x[0, 0, 0])
        return store_levels

    def decode(self, pyramid, frame_of, clip_length, img_hw=None, out=None):
        if isinstance(clip_length, int):                     # windows of one length
            clip_length = [clip_length] * (len(frame_of) // clip_length)
        assert sum(clip_length) == len(frame_of)
        self.decodes.append(list(clip_length))
        outs, at = [], 0
        for T in clip_length:
            rows = frame_of[at:at + T]
            assert all(r in self.live for r in rows), 'a window reads a row that was given back'
            outs.append(window_out([self.tag_of_row[r] for r in rows]))
            at += T
        return dict(gaze=torch.from_numpy(np.concatenate([o[0] for o in outs], axis=1)), boxes=torch.from_numpy(np.concatenate([o[1] for o in outs])),
                    scores=torch.from_numpy(np.concatenate([o[2] for o in outs])))


def make_pool(eng, **kw):
    pool = GazeStreamPool(eng, H, W, **kw)
    free = pool.store.free

    def spy(rows):                     # the fake learns which rows came back
        rows = list(rows)
        free(rows)
        eng.live.difference_update(rows)
    pool.store.free = spy
    return pool


def frames_of(base, a, b):
    """Frames [a, b) of the stream whose tags start at base: [n,3,H,W] with every pixel = the tag."""
    return torch.arange(base + a, base + b, dtype=torch.float32)[:, None, None, None].expand(b - a, 3, H, W)


def expected(base, L, clip_len, stride):
    plan = harness.plan_windows(L, clip_len, stride)
    outs = []
    for a, b, _ in plan:
        g, bx, sc = (torch.from_numpy(x) for x in window_out(range(base + a, base + b)))
        outs.append(harness.clip_outputs(dict(gaze=g, boxes=bx, scores=sc)))
    return harness.merge_video(plan, outs)


def check_stream(parts, base, L, clip_len, stride):
    first = 0
    for p in parts:
        assert p['first'] == first                           # contiguous, nothing twice
        first += p['det'].shape[0]
    assert first == L
    if L == 0:
        return
    want = expected(base, L, clip_len, stride)
    for k, w in zip(('det', 'fused', 'others'), want):
        got = np.concatenate([p[k] for p in parts])
        assert got.shape == w.shape and np.array_equal(got.view(np.uint32), w.view(np.uint32)), (base, L, k)


def drive(pool, lengths, rs, max_push=9):
    """Random interleaving of push / step / close over streams of the given lengths -> {sid: parts}; checks finality on the way."""
    sids = [pool.open() for _ in lengths]
    T = pool.T
    sent, closed, parts = {s: 0 for s in sids}, set(), {s: [] for s in sids}

    def step():
        res = pool.step()
        for s, r in res.items():
            parts[s].append(r)
            n = sum(p['det'].shape[0] for p in parts[s])
            # no frame before it is final: an open stream never gets one of its last clip_len frames
            assert s in closed or n <= max(0, sent[s] - T), (s, n, sent[s])
    while len(closed) < len(sids):
        s = sids[rs.randint(len(sids))]
        op = rs.randint(4)
        if op == 0:
            step()
        elif s not in closed:
            L = lengths[sids.index(s)]
            if sent[s] == L and op == 1:
                pool.close(s)
                closed.add(s)
            elif sent[s] < L:
                n = min(L - sent[s], int(rs.randint(1, max_push + 1)))
                pool.push(s, frames_of(1000 * s, sent[s], sent[s] + n))
                sent[s] += n
    for _ in range(200):
        if not pool.pending():
            break
        step()
    assert not pool.pending() and not pool.streams
    return sids, parts


@pytest.mark.parametrize('clip_len,stride', [(7, 4), (5, 5), (3, 1)])
def test_pool_equals_merge_video_per_stream(clip_len, stride):
    lengths = [0, 5, 7, 18]
    for seed in range(6):
        eng = FakeEngine()
        pool = make_pool(eng, clip_len=clip_len, stride=stride)
        sids, parts = drive(pool, lengths, np.random.RandomState(100 * clip_len + seed))
        for s, L in zip(sids, lengths):
            check_stream(parts[s], 1000 * s, L, clip_len, stride)
        assert pool.store.free_rows() == pool.store.rows and not eng.live      # every row is back on the free list
        assert sorted(pool.store._free) == list(range(pool.store.rows))


def test_one_write_and_one_decode_per_step():
    """Three streams, one new frame each per tick: a step is ONE trunk write of three frames, and ONE decoder call holds all three windows
    once they become certain together."""
    eng = FakeEngine()
    pool = make_pool(eng)
    sids = [pool.open() for _ in range(3)]
    for t in range(8):
        for s in sids:
            pool.push(s, frames_of(1000 * s, t, t + 1))
        res = pool.step()
        assert eng.writes[-1] == 3 and len(eng.writes) == t + 1
        assert (len(res) == 3 and all(r['det'].shape[0] == 1 for r in res.values())) if t == 7 else not res
    assert eng.decodes == [[7, 7, 7]]
    # windows of both longest-clip classes (T <= 10, T > 10) do not share a call; max_decode_windows splits a class
    eng = FakeEngine()
    pool = make_pool(eng, max_decode_windows=2)
    sids = [pool.open() for _ in range(5)]
    for s in sids:
        pool.push(s, frames_of(1000 * s, 0, 8))
    pool.step()
    assert eng.writes == [40] and eng.decodes == [[7, 7], [7, 7], [7]]
    eng = FakeEngine()
    pool = make_pool(eng, clip_len=12, stride=4)
    a, b = pool.open(), pool.open()
    pool.push(a, frames_of(0, 0, 13))
    pool.push(b, frames_of(1000, 0, 5))
    pool.close(b)
    res = pool.step()
    assert eng.decodes == [[5], [12]] and res[b]['det'].shape[0] == 5 and res[a]['det'].shape[0] == 1
    # a closed short stream's window shares the call of the full windows (one class): a list of lengths
    eng = FakeEngine()
    eng.decode, lengths = (lambda *a, _d=eng.decode, **k: (lengths.append(a[2]), _d(*a, **k))[1]), []
    pool = make_pool(eng)
    a, b, c = pool.open(), pool.open(), pool.open()
    pool.push(a, frames_of(0, 0, 8))
    pool.push(b, frames_of(1000, 0, 5))
    pool.push(c, frames_of(2000, 0, 8))
    pool.close(b)
    pool.step()
    assert lengths == [[7, 5, 7]]


def test_max_trunk_frames_splits_the_write():
    eng = FakeEngine()
    pool = make_pool(eng, max_trunk_frames=16, rows=64)
    s = pool.open()
    pool.push(s, frames_of(0, 0, 37))
    pool.close(s)
    res = pool.step()
    assert eng.writes == [16, 16, 5]
    check_stream([res[s]], 0, 37, 7, 4)


@pytest.mark.parametrize('rows', [11, 16, 25])
def test_a_small_store_runs_in_several_steps(rows):
    """Fewer rows than queued frames (11 = one stream's clip_len + stride: the streams take turns): several steps, same results."""
    lengths = [18, 30, 5, 9]
    eng = FakeEngine()
    pool = make_pool(eng, rows=rows)
    sids = [pool.open() for _ in lengths]
    for s, L in zip(sids, lengths):
        pool.push(s, frames_of(1000 * s, 0, L))
        pool.close(s)
    parts, steps = {s: [] for s in sids}, 0
    while pool.pending():
        for s, r in pool.step().items():
            parts[s].append(r)
        steps += 1
        assert steps < 100
    assert steps > 1 and max(eng.writes) <= rows
    for s, L in zip(sids, lengths):
        check_stream(parts[s], 1000 * s, L, 7, 4)
    assert pool.store.free_rows() == rows and not eng.live
    # the same under random interleaving, open streams holding their rows while others wait
    eng = FakeEngine()
    pool = make_pool(eng, rows=rows)
    sids, parts = drive(pool, lengths, np.random.RandomState(rows))
    for s, L in zip(sids, lengths):
        check_stream(parts[s], 1000 * s, L, 7, 4)
    assert pool.store.free_rows() == rows and not eng.live


def test_a_store_too_small_for_one_stream_raises():
    eng = FakeEngine()
    pool = make_pool(eng, rows=10)                          # clip_len + stride = 11
    s = pool.open()
    pool.push(s, frames_of(0, 0, 3))
    with pytest.raises(McgError, match='cannot hold one stream'):
        pool.step()
    assert eng.writes == []


def test_store_alloc_and_free():
    store = PyramidStore(FakeEngine(), 6, H, W)
    a = store.alloc(4)
    assert len(set(a)) == 4 and store.free_rows() == 2
    with pytest.raises(McgError, match='2 of 6 are free'):
        store.alloc(3)                                      # never a live row
    b = store.alloc(2)
    assert not set(a) & set(b)
    store.free(a[1:3])
    assert sorted(store.alloc(2)) == sorted(a[1:3])
    with pytest.raises(McgError, match='was not handed out'):
        store.free([a[1], a[1]])
    with pytest.raises(McgError):
        store.write(frames_of(0, 0, 2), [a[0]])             # one row per frame
    with pytest.raises(McgError):
        PyramidStore(FakeEngine(), 0, H, W)


def test_row_table_is_checked_on_the_host():
    assert check_row_table([4, 0, 2], 5, 3).dtype == np.int32
    assert check_row_table(torch.tensor([3, 1]), 4, 2).tolist() == [3, 1]
    assert check_row_table([], 5, 0).size == 0
    for bad, K, n in (([0, 1, 1], 5, 3),                    # a row named twice
                      ([0, 1, 5], 5, 3),                    # row 5 of a 5-row store
                      ([0, -1, 2], 5, 3),                   # negative
                      ([0, 1], 5, 3),                       # one row per frame
                      ([[0, 1, 2]], 5, 3),                  # not flat
                      ([0.0, 1.0, 2.0], 5, 3),              # not integers
                      ([0], 0, 1)):                         # empty store
        with pytest.raises(McgError):
            check_row_table(bad, K, n)


def test_backbone_fpn_rows_rejects_a_bad_table_before_touching_the_device():
    e = object.__new__(HipEngine)          # no weights, no device: the check comes before either is needed
    store = [torch.empty(5, 8 >> i, 8 >> i, 256) for i in range(4)]
    img = torch.zeros(3, 3, H, W)
    with pytest.raises(McgError, match='names row 2'):
        e.backbone_fpn_rows(img, store, [2, 0, 2])
    with pytest.raises(McgError, match=r'\[0, 5\)'):
        e.backbone_fpn_rows(img, store, [0, 1, 5])
    with pytest.raises(McgError, match='3 frames'):
        e.backbone_fpn_rows(img, store, [0, 1])


def test_push_and_close_are_checked():
    pool = make_pool(FakeEngine())
    s = pool.open()
    pool.push(s, frames_of(0, 0, 2))
    with pytest.raises(McgError, match='no open stream'):
        pool.push(s + 1, frames_of(0, 0, 1))
    with pytest.raises(McgError, match='frames must be'):
        pool.push(s, torch.zeros(1, 3, H, W + 32))
    pool.close(s)
    with pytest.raises(McgError, match='is closed'):
        pool.push(s, frames_of(0, 2, 3))
    with pytest.raises(McgError, match='is closed'):
        pool.close(s)
    res = pool.step()
    assert res[s]['first'] == 0 and res[s]['det'].shape == (2, 3, 5)
    with pytest.raises(McgError, match='no open stream'):   # ended: the stream is gone
        pool.push(s, frames_of(0, 2, 3))
    assert pool.step() == {}
