"""CPU: the temporal filter of the reference's metric as a stream option (``smooth=``) -- the arithmetic mcg_smooth_gaze states
(tests/smooth_cases.py::smooth_vector restates it) against metric.smooth_filter, the incremental host filter (stream.StreamSmoother)
against that arithmetic over the whole sequence, the table the kernel takes (harness.smooth_plan), and GazeStream / GazeStreamPool with
merge='host' on the fake engine of tests/test_stream_pool_cpu.py.  No device."""
import os
import re

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, metric
from mcgaze_amd import lib as L
from mcgaze_amd.stream import GazeStream, GazeStreamPool, StreamSmoother
from tests import smooth_cases as SC
from tests.test_stream_pool_cpu import H, W, frames_of, make_pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKINGS = ((1,), (3, 5, 4), (1 << 20,))                    # frame by frame; 3, 5, 4, 3, ...; everything at once


@pytest.mark.parametrize('length', [1, 2, 3, 4, 12, 101])
def test_specification_against_the_reference_filter(length):
    """metric.smooth_filter is the reference's torch expression.  The only freedom it leaves is how torch.norm rounds the sum of squares
    (it depends on the CPU's vector path): that moves the norm by at most 1 ulp and so the quotient by at most 2."""
    x = SC.gaze_sequence(length, length)
    want = metric.smooth_filter(torch.from_numpy(x.copy()), SC.ALPHA).numpy()
    got = SC.spec(x)
    print(f'L={length}: {int((SC.bits(got) != SC.bits(want)).sum())} of {got.size} elements differ from torch in their bits')
    assert np.abs(SC.ordered(got) - SC.ordered(want)).max() <= 2
    if length == 1:
        assert np.array_equal(SC.bits(got), SC.bits(x))    # the input itself: not normalised
        assert abs(float(np.linalg.norm(got[0])) - 1) > 1e-4
    # harness.smooth_host is the vectorised form every host path uses
    assert np.array_equal(SC.bits(harness.smooth_host(x, SC.ALPHA)), SC.bits(got))


@pytest.mark.parametrize('length', [1, 2, 3, 12])
def test_stream_smoother_equals_the_specification_in_any_chunking(length):
    rs = np.random.RandomState(length)
    det = rs.uniform(0, 100, (length, 3, 5)).astype(np.float32)
    fused, others = SC.gaze_sequence(10 + length, length), SC.gaze_sequence(20 + length, length, (3,))
    want_f, want_o = SC.spec(fused), SC.spec(others)
    for sizes in CHUNKINGS:
        s = StreamSmoother(SC.ALPHA)
        parts, fed = [], 0
        for a, b in SC.chunks(length, sizes):
            parts.append(s.push(det[a:b], fused[a:b], others[a:b]))
            fed = b
            assert sum(p[0].shape[0] for p in parts) == fed - 1      # the newest frame waits for its successor
        parts.append(s.finish())
        assert parts[-1][0].shape[0] == 1                  # ... and comes with the stream's end
        got = [np.concatenate([p[i] for p in parts]) for i in range(5)]
        for g, w, name in zip(got, (det, fused, others, want_f, want_o), ('det', 'fused', 'others', 'fused_smooth', 'others_smooth')):
            assert g.shape == w.shape and np.array_equal(SC.bits(g), SC.bits(w)), (length, sizes, name)
        assert all(p[3].shape == (p[0].shape[0], 3) and p[4].shape == (p[0].shape[0], 3, 3) for p in parts)
        with pytest.raises(L.McgError):
            s.push(det[:1], fused[:1], others[:1])
    # an empty stream ends with nothing
    assert StreamSmoother(SC.ALPHA).finish()[3].shape == (0, 3)


def test_smooth_plan():
    rows = {f: r for f, r in enumerate((5, 2, 9, 0, 7, 3, 8))}
    # the first chunk of a stream: frame 0 has no predecessor; frame 2's successor is final but not handed out
    assert harness.smooth_plan(range(0, 3), rows.__getitem__, 0, None).tolist() == [[-1, 5, 2], [5, 2, 9], [2, 9, 0]]
    # a middle chunk: the predecessor of its first frame is the row held back from the chunk before
    assert harness.smooth_plan(range(3, 5), rows.__getitem__, 0, None).tolist() == [[9, 0, 7], [0, 7, 3]]
    # the final chunk: the stream ended at frame 6
    t = harness.smooth_plan(range(5, 7), rows.__getitem__, 0, 6, store_rows=10)
    assert t.dtype == np.int32 and t.tolist() == [[7, 3, 8], [3, 8, -1]]
    # a one-frame stream, and no frame at all
    assert harness.smooth_plan([0], {0: 4}.__getitem__, 0, 0).tolist() == [[-1, 4, -1]]
    assert harness.smooth_plan([], rows.__getitem__, 0, None).shape == (0, 3)
    # a stream whose first frame is not frame 0
    assert harness.smooth_plan([3, 4], rows.__getitem__, 3, 4).tolist() == [[-1, 0, 7], [0, 7, -1]]
    for kw in (dict(store_rows=9), dict(store_rows=3)):      # row 9 (frame 2, a neighbour here) and rows past a 3-row store
        with pytest.raises(ValueError, match='outside the store'):
            harness.smooth_plan(range(0, 2), rows.__getitem__, 0, None, **kw)
    with pytest.raises(ValueError, match='outside the store'):
        harness.smooth_plan([0], {0: -3, 1: 1}.__getitem__, 0, None)


def run_stream(length, sizes, **kw):
    s = GazeStream(SC.RingFakeEngine(), H, W, **kw)
    return [s.push(frames_of(0, a, b)) for a, b in SC.chunks(length, sizes)] + [s.finish()]


def check_against_plain(parts, plain, length, what):
    cat = lambda ps, k: np.concatenate([p[k] for p in ps])
    for k in ('det', 'fused', 'others'):
        assert np.array_equal(SC.bits(cat(parts, k)), SC.bits(cat(plain, k))), (what, k)
    assert np.array_equal(SC.bits(cat(parts, 'fused_smooth')), SC.bits(SC.spec(cat(plain, 'fused')))), what
    assert np.array_equal(SC.bits(cat(parts, 'others_smooth')), SC.bits(SC.spec(cat(plain, 'others')))), what
    first = 0
    for p in parts:
        k = p['det'].shape[0]
        assert p['first'] == first and p['fused'].shape == p['fused_smooth'].shape == (k, 3), what
        assert p['others'].shape == p['others_smooth'].shape == (k, 3, 3), what
        first += k
    assert first == length, what


@pytest.mark.parametrize('length', [1, 2, 9, 13])
def test_gaze_stream_host_smooth(length):
    for sizes in CHUNKINGS:
        plain = run_stream(length, sizes)
        assert all('fused_smooth' not in p and list(p) == ['first', 'det', 'fused', 'others'] for p in plain)
        parts = run_stream(length, sizes, smooth=SC.ALPHA)
        check_against_plain(parts, plain, length, (length, sizes))
        # one frame behind the plain stream at every push, level with it after finish()
        for i in range(len(parts) - 1):
            done = sum(p['det'].shape[0] for p in plain[:i + 1])
            assert sum(p['det'].shape[0] for p in parts[:i + 1]) == max(0, done - 1), (length, sizes, i)


def test_pool_host_smooth():
    lengths, pace = (1, 2, 13, 0), (1, 1, 3, 1)

    def run(**kw):
        pool = make_pool(SC.RingFakeEngine(), **kw)
        sids = [pool.open() for _ in lengths]
        got, sent = {s: [] for s in sids}, [0] * len(lengths)
        while pool.pending() or any(a < n for a, n in zip(sent, lengths)) or pool.streams:
            for i, s in enumerate(sids):
                if s in pool.streams and not pool.streams[s].closed:
                    if sent[i] < lengths[i]:
                        b = min(lengths[i], sent[i] + pace[i])
                        pool.push(s, frames_of(1000 * s, sent[i], b))
                        sent[i] = b
                    else:
                        pool.close(s)
            for s, r in pool.step().items():
                got[s].append(r)
        assert pool.store.free_rows() == pool.store.rows
        return [got[s] for s in sids]

    plain, parts = run(), run(smooth=SC.ALPHA)
    for i, n in enumerate(lengths):
        if n:
            check_against_plain(parts[i], plain[i], n, i)
        else:                                              # an empty stream still gets its closing entry, with the new keys
            assert len(parts[i]) == 1 and parts[i][0]['fused_smooth'].shape == (0, 3) and parts[i][0]['others_smooth'].shape == (0, 3, 3)


@pytest.mark.parametrize('bad', [0, 1.5, 'x', -0.6, True, float('nan')])
def test_smooth_is_validated(bad):
    with pytest.raises(ValueError, match='smooth'):
        GazeStream(SC.RingFakeEngine(), H, W, smooth=bad)
    with pytest.raises(ValueError, match='smooth'):
        GazeStreamPool(SC.RingFakeEngine(), H, W, smooth=bad)
    with pytest.raises(ValueError, match='smooth'):
        StreamSmoother(bad)
    with pytest.raises(ValueError, match='smooth'):
        harness.run_videos(SC.RingFakeEngine(), [], smooth=bad)
    with pytest.raises(ValueError, match='smooth'):
        harness.run_head_video(SC.RingFakeEngine(), None, [], [], smooth=bad)


def test_smooth_one_is_a_plain_normalisation():
    """alpha = 1 is allowed: b = 0, the neighbours drop out (finite inputs) and the filter only normalises."""
    x = SC.gaze_sequence(3, 5)
    got = harness.smooth_host(x, 1)
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.array_equal(SC.bits(got), SC.bits(SC.spec(x, 1.0)))


def test_boundary():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    assert re.search(r'\bint mcg_smooth_gaze\(mcg_stream s, const float\* store, int store_rows, const int32_t\* plan, int num_out,\s*'
                     r'double alpha, float\* out\);', hdr)
    assert 'tools/calculate_mae_gaze360.py:16-29' in hdr      # the reference citation
    assert 'mcg_smooth_gaze' in L.EXPORTS
    assert L.ABI_VERSION == 20 and int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) == 20
    assert 'smooth.hip' in open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'Makefile')).read()
    lib = L.load()
    assert hasattr(lib, 'mcg_smooth_gaze') and len(lib.mcg_smooth_gaze.argtypes) == 7
