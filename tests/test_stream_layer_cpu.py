"""CPU: what GazeStream and GazeStreamPool share (mcgaze_amd/stream.py: _StreamState, _decode_windows) -- a lone stream makes the decoder
calls and returns the bits of a pool of one stream -- and the result-row layout (harness.pack_rows / split_rows).  Fake engines, no device."""
import numpy as np
import pytest
import torch

from mcgaze_amd import harness
from mcgaze_amd.stream import GazeStream
from tests import smooth_cases as SC
from tests.test_stream_pool_cpu import H, W, frames_of, make_pool

KEYS = ('det', 'fused', 'others', 'fused_smooth', 'others_smooth')


def recording_engine():
    """A fake engine that lists its decode calls as (clip_length as given, rows in the table)."""
    eng = SC.RingFakeEngine()
    eng.calls = []
    decode = eng.decode
    eng.decode = lambda pyramid, frame_of, clip_length, **kw: (eng.calls.append((clip_length, len(frame_of))), decode(pyramid, frame_of, clip_length, **kw))[1]
    return eng


def whole(parts):
    first = 0
    for p in parts:
        assert p['first'] == first
        first += p['det'].shape[0]
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS if k in parts[0]}


@pytest.mark.parametrize('clip_len,stride', [(7, 4), (3, 1), (3, 3)])
def test_a_lone_stream_is_a_pool_of_one(clip_len, stride):
    for length in (0, 1, clip_len, clip_len + 1, 2 * clip_len + stride + 1):
        for sizes in ((1,), (2, 5, 1), (length or 1,)):
            for max_windows in (None, 1, 2):
                for smooth in (None, 0.6):
                    what = (length, sizes, max_windows, smooth)
                    kw = dict(clip_len=clip_len, stride=stride, max_decode_windows=max_windows, smooth=smooth)
                    lone_eng, pool_eng = recording_engine(), recording_engine()
                    lone, pool = GazeStream(lone_eng, H, W, **kw), make_pool(pool_eng, **kw)
                    sid = pool.open()
                    a_parts, b_parts = [], []
                    for a, b in SC.chunks(length, sizes):
                        a_parts.append(lone.push(frames_of(0, a, b)))
                        pool.push(sid, frames_of(0, a, b))
                        b_parts += [r for r in [pool.step().get(sid)] if r is not None]
                    a_parts.append(lone.finish())
                    pool.close(sid)
                    b_parts.append(pool.step()[sid])
                    assert not pool.pending() and not pool.streams, what
                    # the same decoder calls: a lone stream's windows are of one length, so clip_length is that int and never a list
                    assert lone_eng.calls == pool_eng.calls and all(type(T) is int for T, _ in lone_eng.calls), (what, lone_eng.calls, pool_eng.calls)
                    assert all(n % T == 0 and (max_windows is None or n // T <= max_windows) for T, n in lone_eng.calls), what
                    assert bool(lone_eng.calls) == (length > 0), what
                    got, want = whole(b_parts), whole(a_parts)
                    assert list(got) == list(want) == list(KEYS[:3 if smooth is None else 5]), what
                    for k in want:
                        assert want[k].shape[0] == length and np.array_equal(SC.bits(got[k]), SC.bits(want[k])), (what, k)


def parts_of(k, seed, as_torch):
    rs = np.random.RandomState(seed)
    parts = [rs.standard_normal((k,) + s).astype(np.float32) for s in ((3, 5), (3,), (3, 3), (3,), (3, 3))]
    return [torch.from_numpy(p) for p in parts] if as_torch else parts


@pytest.mark.parametrize('as_torch', [False, True])
def test_pack_rows_and_split_rows(as_torch):
    for k in (0, 1, 6):
        for n in (3, 5):
            parts = parts_of(k, 10 * k + n, as_torch)[:n]
            packed = harness.pack_rows(*parts)
            assert type(packed) is type(parts[0]) and tuple(packed.shape) == (k, harness.ROW + (harness.SMOOTH_ROW if n == 5 else 0))
            back = harness.split_rows(packed)
            assert len(back) == n
            for p, q in zip(parts, back):
                assert p.shape == q.shape and np.array_equal(SC.bits(p), SC.bits(q))
            # the layout: det 3x5 | fused 3 | others 3x3 | fused_smooth 3 | others_smooth 3x3, row-major
            widths = (15, 3, 9, 3, 9)[:n]
            flat = np.concatenate([harness._host(p).reshape(k, w) for p, w in zip(parts, widths)], axis=1)
            assert np.array_equal(SC.bits(packed), SC.bits(flat))
            if k:                                              # views: a write through a part lands in the packed rows
                for i, q in enumerate(back):
                    q[...] = float(100 + i)
                want = np.concatenate([np.full((k, w), 100 + i, np.float32) for i, w in enumerate(widths)], axis=1)
                assert np.array_equal(harness._host(packed), want)
    z = (lambda *s: torch.zeros(*s)) if as_torch else (lambda *s: np.zeros(s, np.float32))
    for bad in (z(4, 26), z(4, 28), z(4, 12), z(4, 40), z(0, 15), z(27), z(2, 3, 9)):
        with pytest.raises(ValueError, match='27 or 39 columns'):
            harness.split_rows(bad)
