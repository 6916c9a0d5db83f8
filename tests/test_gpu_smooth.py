"""-m gpu: the temporal filter on the device -- mcg_smooth_gaze alone against its specification (tests/smooth_cases.py, bit for bit: f32
multiplies and adds, two fma, a correctly rounded square root and division), its defined behaviour on bad tables; then ``smooth=`` of
GazeStream, GazeStreamPool, harness.run_videos and harness.run_head_video.  Frames are 64 x 64 with random weights, as in the other
stream tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from mcgaze_amd.stream import GazeStream, GazeStreamPool
from tests import smooth_cases as SC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
POISON = 12345.0
KEYS = ('det', 'fused', 'others')


def launch(store, plan, out, num_out=None, alpha=SC.ALPHA, rows=None):
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    return L.load().mcg_smooth_gaze(C.c_void_p(torch.cuda.current_stream().cuda_stream), p(store), store.shape[0] if rows is None else rows, p(plan),
                                    plan.shape[0] if num_out is None else num_out, alpha, p(out))


def same_with_nan(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(SC.bits(got)[ok], SC.bits(want)[ok]), what


def kernel_case():
    """A 64-row store and a plan of 40 outputs over scattered rows: interior frames, first frames, last frames, one-frame streams; rows
    0..2 hold zero vectors, row 3 an infinite component; outputs 38 and 39 carry an index outside the store."""
    rs = np.random.RandomState(11)
    store = rs.standard_normal((64, 27)).astype(np.float32)
    store[0:3, 15:] = 0
    store[3, 16] = np.inf
    perm = rs.permutation(np.arange(4, 64))
    plan = []
    for i in range(30):
        a, b, c = perm[i], perm[(i + 7) % 60], perm[(i + 19) % 60]
        plan.append([(a, b, c), (-1, b, c), (a, b, -1), (-1, b, -1)][i % 4])
    plan += [(0, 1, 2), (-1, 1, 2), (0, 1, -1), (-1, 1, -1),       # 0 / 0: NaN; a one-frame stream of zeros: zeros
             (10, 0, 11), (3, 12, 13), (12, 3, 13), (-1, 3, -1),   # a zero frame between two others; inf as a neighbour and as the frame
             (20, 21, 64), (-2, 22, 23)]                           # one past the store; a negative index that is not -1
    assert len(plan) == 40
    return store, np.asarray(plan, dtype=np.int32)


def test_kernel_equals_the_specification():
    store, plan = kernel_case()
    want = SC.emulate(store, plan)
    assert np.isnan(want[38:]).all() and np.isnan(want[30:33]).all() and (want[33] == 0).all() and np.isfinite(want[:30]).all()
    assert np.isnan(want[36]).any() and not np.isnan(want[36]).all()
    out = torch.full((48, 12), POISON, dtype=torch.float32, device=DEV)
    dstore, dplan = torch.from_numpy(store).to(DEV), torch.from_numpy(plan).to(DEV)
    L.check(launch(dstore, dplan, out), 'mcg_smooth_gaze')
    got = out.cpu().numpy()
    same_with_nan(got[:40], want, 'kernel')
    assert np.isnan(got[38:40]).all()                      # the two rows with an index outside the store
    assert (got[40:] == POISON).all()                      # nothing past num_out
    assert np.array_equal(SC.bits(dstore.cpu().numpy()), SC.bits(store))
    # another alpha, and alpha = 1 (b = 0)
    for alpha in (0.25, 1.0):
        L.check(launch(dstore, dplan[:30], out, alpha=alpha), 'mcg_smooth_gaze')
        same_with_nan(out.cpu().numpy()[:30], SC.emulate(store, plan[:30], alpha), alpha)
    # more than one block (64 outputs each), the last one partly filled
    rs = np.random.RandomState(12)
    big = np.stack([rs.randint(-1, 64, 150), rs.randint(0, 64, 150), rs.randint(-1, 64, 150)], axis=1).astype(np.int32)
    out = torch.full((151, 12), POISON, dtype=torch.float32, device=DEV)
    L.check(launch(dstore, torch.from_numpy(big).to(DEV), out), 'mcg_smooth_gaze')
    got = out.cpu().numpy()
    same_with_nan(got[:150], SC.emulate(store, big), 'three blocks')
    assert (got[150] == POISON).all()


def test_kernel_arguments():
    store, plan = kernel_case()
    dstore, dplan = torch.from_numpy(store).to(DEV), torch.from_numpy(plan).to(DEV)
    out = torch.full((40, 12), POISON, dtype=torch.float32, device=DEV)
    assert launch(dstore, dplan, out, num_out=0) == L.MCG_OK
    assert launch(dstore, None, None, num_out=0) == L.MCG_OK
    assert launch(dstore, dplan, out, rows=0) != L.MCG_OK
    assert launch(dstore, dplan, out, num_out=-1) != L.MCG_OK
    assert launch(dstore, None, out, num_out=40) != L.MCG_OK
    assert launch(dstore, dplan, out, alpha=float('nan')) != L.MCG_OK
    assert bool((out == POISON).all())
    # a store that is declared smaller than it is: rows 32 and above become "outside"
    L.check(launch(dstore, dplan, out, rows=32), 'mcg_smooth_gaze')
    same_with_nan(out.cpu().numpy(), SC.emulate(store[:32], plan), 'rows=32')


def test_kernel_in_a_graph():
    store, plan = kernel_case()
    dstore, dplan = torch.from_numpy(store).to(DEV), torch.from_numpy(plan).to(DEV)
    out = torch.full((40, 12), POISON, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.check(launch(dstore, dplan, out), 'mcg_smooth_gaze')
    for seed in (1, 2):                                    # the replay reads the store as it is then
        fresh = np.random.RandomState(seed).standard_normal((64, 27)).astype(np.float32)
        dstore.copy_(torch.from_numpy(fresh))
        out.fill_(POISON)
        graph.replay()
        same_with_nan(out.cpu().numpy(), SC.emulate(fresh, plan), seed)


# ------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def engines():
    from mcgaze_amd.engine import HipEngine
    sd = synth.make_state_dict(0)
    return {p: HipEngine(sd, precision=p) for p in ('f16x3', 'f16')}


LIMIT = {'f16x3': None, 'f16': 12}                         # the fp16 decoder keeps its bits below 256 tokens per call


def cat(parts, key):
    return np.concatenate([harness._host(p[key]) for p in parts])


def run_stream(e, v, piece, limit, **kw):
    s = GazeStream(e, 64, 64, max_decode_windows=limit, **kw)
    return [s.push(v[a:b]) for a, b in SC.chunks(v.shape[0], (piece,))] + [s.finish()]


def check_smoothed(parts, plain, length, what):
    for k in KEYS:
        assert np.array_equal(SC.bits(cat(parts, k)), SC.bits(cat(plain, k))), (what, k)
    assert np.array_equal(SC.bits(cat(parts, 'fused_smooth')), SC.bits(SC.spec(cat(plain, 'fused')))), what
    assert np.array_equal(SC.bits(cat(parts, 'others_smooth')), SC.bits(SC.spec(cat(plain, 'others')))), what
    first = 0
    for p in parts:
        k = p['det'].shape[0]
        assert p['first'] == first and tuple(p['fused_smooth'].shape) == (k, 3) and tuple(p['others_smooth'].shape) == (k, 3, 3), what
        first += k
    assert first == length, what


@pytest.mark.parametrize('precision', ['f16x3', 'f16'])
def test_gaze_stream_smooth(engines, precision):
    e, limit = engines[precision], LIMIT[precision]
    for length in (1, 2, 7, 12, 13):
        v = torch.from_numpy(synth.make_clips(40 + length, 1, length, 64, 64)).to(DEV)
        plain = run_stream(e, v, 3, limit, merge='device', results='device')
        assert all('fused_smooth' not in p for p in plain)
        for piece in (1, 3, 5):
            dev = run_stream(e, v, piece, limit, merge='device', results='device', smooth=SC.ALPHA)
            assert all(isinstance(p[k], torch.Tensor) and p[k].is_cuda and p[k].dtype == torch.float32
                       for p in dev for k in KEYS + ('fused_smooth', 'others_smooth'))
            check_smoothed(dev, plain, length, (precision, length, piece, 'device'))
            host = run_stream(e, v, piece, limit, smooth=SC.ALPHA)
            assert all(isinstance(p[k], np.ndarray) for p in host for k in KEYS + ('fused_smooth', 'others_smooth'))
            assert [p['first'] for p in host] == [p['first'] for p in dev]
            for k in KEYS + ('fused_smooth', 'others_smooth'):
                assert np.array_equal(SC.bits(cat(host, k)), SC.bits(cat(dev, k))), (precision, length, piece, k)
        if length not in (1, 12):
            continue
        # merge='device' with its results copied to the host: the same dicts as numpy arrays
        mid = run_stream(e, v, 3, limit, merge='device', smooth=SC.ALPHA)
        assert all(isinstance(p[k], np.ndarray) for p in mid for k in KEYS + ('fused_smooth', 'others_smooth'))
        check_smoothed(mid, plain, length, (precision, length, 'device -> host'))
        if length == 1:                                    # a one-frame stream: its gaze as it is
            assert np.array_equal(SC.bits(cat(mid, 'fused_smooth')), SC.bits(cat(plain, 'fused')))


def test_pool_smooth(engines):
    """Three streams of 1, 2 and 13 frames at different pace, closed at different steps: each is a lone smoothed GazeStream, and every
    row of the result store -- the held predecessors too -- is back on the free list at the end."""
    e = engines['f16x3']
    lengths, pace = (1, 2, 13), (1, 1, 3)
    vids = [torch.from_numpy(synth.make_clips(60 + i, 1, n, 64, 64)).to(DEV) for i, n in enumerate(lengths)]
    pool = GazeStreamPool(e, 64, 64, rows=40, merge='device', results='device', smooth=SC.ALPHA)
    sids = [pool.open() for _ in lengths]
    got, sent = {s: [] for s in sids}, [0] * 3
    while pool.streams:
        for i, s in enumerate(sids):
            if s in pool.streams and not pool.streams[s].closed:
                if sent[i] < lengths[i]:
                    pool.push(s, vids[i][sent[i]:sent[i] + pace[i]])
                    sent[i] = min(lengths[i], sent[i] + pace[i])
                else:                                      # closed one step after its last frame
                    pool.close(s)
        for s, r in pool.step().items():
            got[s].append(r)
    assert pool.store.free_rows() == 40
    assert not pool.dmerger.streams and sorted(pool.dmerger._free) == list(range(pool.dmerger.store.shape[0]))
    for i, s in enumerate(sids):
        lone = run_stream(e, vids[i], 2, None, merge='device', results='device', smooth=SC.ALPHA)
        assert all(p[k].is_cuda for p in got[s] for k in KEYS + ('fused_smooth', 'others_smooth'))
        for k in KEYS + ('fused_smooth', 'others_smooth'):
            a, b = cat(got[s], k), cat(lone, k)
            assert a.shape == b.shape and a.shape[0] == lengths[i] and np.array_equal(SC.bits(a), SC.bits(b)), (i, k)
        first = 0
        for p in got[s]:
            assert p['first'] == first
            first += p['det'].shape[0]


def test_run_videos_smooth(engines):
    e = engines['f16x3']
    videos = [dict(id=i + 1, frames=torch.from_numpy(synth.make_clips(30 + i, 1, n, 64, 64))) for i, n in enumerate((1, 5, 12))]
    plain = harness.run_videos(e, videos, batch_clips=2)
    for kw in (dict(), dict(merge='device'), dict(merge='device', reuse_frames=True)):
        got = harness.run_videos(e, videos, batch_clips=2, smooth=SC.ALPHA, **kw)
        for g, w in zip(got, plain):
            assert {k: v for k, v in g.items() if not k.endswith('_smooth')} == w, kw
            assert sorted(set(g) - set(w)) == ['eyes_gazes_smooth', 'face_gazes_smooth', 'fusion_gazes_smooth', 'head_gazes_smooth'], kw
            for k in ('fusion', 'face', 'eyes', 'head'):
                want = SC.spec(np.asarray(w[f'{k}_gazes'], dtype=np.float32))
                assert np.array_equal(SC.bits(np.asarray(g[f'{k}_gazes_smooth'], dtype=np.float32)), SC.bits(want)), (kw, k)


def test_run_head_video_smooth(engines):
    """Two people for nine frames (one track each): fused_smooth is the specification over the track, the arrow is drawn from it, and
    without the option the records are what they were."""
    from tests.test_gpu_head_crops import chain
    e = engines['f16x3']
    rs = np.random.RandomState(7)
    frames = [rs.randint(0, 256, (96, 128, 3)).astype(np.uint8) for _ in range(9)]
    per_frame = [[[10 + t, 20, 40 + t, 55.5], [100 - t, 60, 135 - t, 100]] for t in range(9)]
    pipe = P.DevicePipeline(chain(64))
    plain = harness.run_head_video(e, pipe, frames, per_frame, max_len=4)
    got = harness.run_head_video(e, pipe, frames, per_frame, max_len=4, smooth=SC.ALPHA)
    assert len(plain) == len(got) == 2
    for w, g in zip(plain, got):
        assert list(w) == ['id', 'det', 'fused', 'others', 'frame_id', 'head_box', 'crop', 'arrow']
        assert sorted(set(g) - set(w)) == ['fused_smooth'] and g['id'] == w['id'] and g['frame_id'] == w['frame_id']
        for k in KEYS + ('head_box', 'crop'):
            assert np.array_equal(g[k], w[k]) and g[k].dtype == w[k].dtype, k
        assert g['fused'].shape == (9, 3) and np.array_equal(SC.bits(g['fused_smooth']), SC.bits(SC.spec(w['fused'])))
        assert np.array_equal(w['arrow'], harness.head_arrows(w['head_box'], w['fused']))
        assert np.array_equal(g['arrow'], harness.head_arrows(g['head_box'], g['fused_smooth']))
