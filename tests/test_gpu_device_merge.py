"""-m gpu: the overlap merge on the device -- mcg_merge_windows alone against harness.merge_video (bit for bit: the arithmetic is f32
adds, exact halvings, compares and one IEEE division), its defined behaviour on bad tables, graph capture; then GazeStream, GazeStreamPool
and harness.run_videos with merge='device' against their host merge, and results='device'.  The plans, random outputs and call splits are
those of tests/test_device_merge_cpu.py (tests/merge_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import lib as L
from mcgaze_amd.stream import GazeStream, GazeStreamPool
from tests import merge_cases as MC

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 12345.0
LENGTHS = (1, 7, 8, 12, 13, 30)      # one short clip; exactly clip_len; one frame more; the last window over two others; 30


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def launch(table, max_src, gaze, boxes, scores, scale, store, thr=0.5, num_dst=None):
    """Device tensors in, one mcg_merge_windows launch on the current stream."""
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    L.check(L.load().mcg_merge_windows(C.c_void_p(torch.cuda.current_stream().cuda_stream), p(gaze), p(boxes), p(scores), scores.shape[0], p(scale),
                                       int(scale is not None and scale.numel() != 4), p(table), table.shape[0] if num_dst is None else num_dst,
                                       max_src, p(store), store.shape[0], thr), 'mcg_merge_windows')


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def scale_of(form, plan, rs):
    """None; [4] for every frame; one [T,4] per window.  No value is a power of two or has an exact reciprocal: x * (1 / s) != x / s."""
    if form == 'none':
        return None
    if form == 'one':
        return np.array([224 / 177, 224 / 199, 224 / 177, 224 / 199], dtype=np.float32)
    return [rs.uniform(0.4, 2.5, (b - a, 4)).astype(np.float32) for a, b, _ in plan]


@pytest.mark.parametrize('form', ['none', 'one', 'per_frame'])
def test_kernel_equals_merge_video(form):
    """Every (clip_len, stride) of the CPU test at L in LENGTHS, the windows dealt to calls three ways; the frames' store rows are a random
    selection of a store with three rows to spare, which must keep their sentinel."""
    for clip_len, stride in MC.CONFIGS:
        for L_ in LENGTHS:
            plan = harness.plan_windows(L_, clip_len, stride)
            rs = np.random.RandomState(1000 * clip_len + 100 * stride + L_)
            outs = [MC.window_outputs(rs, b - a) for a, b, _ in plan]
            scale = scale_of(form, plan, rs)
            want = MC.reference(plan, outs, scale)
            perm = rs.permutation(L_ + 3).tolist()
            for name, parts in MC.splits(len(plan)).items():
                store = torch.full((L_ + 3, 27), SENTINEL, dtype=torch.float32, device=DEV)
                MC.run_plan(plan, outs, parts, lambda t, m, g, b, s, sc: launch(dev(t), m, dev(g), dev(b), dev(s), dev(sc), store), scale, perm)
                got = store.cpu().numpy()
                assert np.array_equal(bits(got[perm[:L_]]), bits(want)), (form, clip_len, stride, L_, name)
                assert (got[perm[L_:]] == SENTINEL).all(), (form, clip_len, stride, L_, name)


def test_threshold_edges_and_negative_zero():
    """Scores exactly at the threshold (not low), one ulp below (low), and a -0.0 coordinate: on its own, averaged with +0.0, with -0.0
    and zeroed by a low score -- the sign bits are the host's."""
    plan = harness.plan_windows(8)                          # (0, 7), (1, 8): frames 1..6 are averaged
    outs = [MC.window_outputs(np.random.RandomState(i), 7) for i in range(2)]
    for g, b, s in outs:
        s[:] = 0.7
    (_, b0, s0), (_, b1, s1) = outs
    s0[2, 0], s1[1, 0] = 0.5, 0.5                           # frame 2, clue 0: both exactly at the threshold -> averaged
    s0[3, 1], s1[2, 1] = MC.BELOW, 0.5                      # frame 3, clue 1: the stored score is low -> zeroed
    s0[4, 2], s1[3, 2] = 0.5, MC.BELOW                      # frame 4, clue 2: the new score is low -> zeroed
    b0[0, 0, 0] = -0.0                                      # frame 0: -0.0 alone
    b0[5, 0, 1], b1[4, 0, 1] = -0.0, 0.0                    # frame 5: (-0 + +0) / 2 = +0
    b0[6, 1, 2], b1[5, 1, 2] = -0.0, -0.0                   # frame 6: (-0 + -0) / 2 = -0
    b1[6, 2, 3], s1[6, 2] = -0.0, 0.2                       # frame 7: low score, the box is +0 whatever it held
    want = MC.reference(plan, outs)
    assert np.signbit(want[0, 0]) and not np.signbit(want[5, 1]) and np.signbit(want[6, 5 + 2]) and not np.signbit(want[7, 10 + 3])
    assert want[2, 0] != 0 and (want[3, 5:9] == 0).all() and (want[4, 10:14] == 0).all()
    for parts in MC.splits(2).values():
        store = torch.full((8, 27), SENTINEL, dtype=torch.float32, device=DEV)
        MC.run_plan(plan, outs, parts, lambda t, m, g, b, s, sc: launch(dev(t), m, dev(g), dev(b), dev(s), None, store))
        assert np.array_equal(bits(store.cpu().numpy()), bits(want))


def test_nan_scores_keep_their_place():
    """A NaN score is not < threshold: its box is kept and averaged, and the NaN stays where the host merge has it."""
    plan = harness.plan_windows(12)
    rs = np.random.RandomState(77)
    outs = [MC.window_outputs(rs, 7) for _ in plan]
    outs[0][2][5, 1] = outs[1][2][2, 0] = outs[2][2][6, 2] = np.nan
    want = MC.reference(plan, outs)
    assert np.isnan(want).any()
    store = torch.full((12, 27), SENTINEL, dtype=torch.float32, device=DEV)
    MC.run_plan(plan, outs, [[0, 1, 2]], lambda t, m, g, b, s, sc: launch(dev(t), m, dev(g), dev(b), dev(s), None, store))
    got = store.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])


def test_rows_and_sources_out_of_range_are_skipped():
    """What merge_plan would reject, handed to the kernel directly: a dst_row outside the store writes nothing, a source outside [0, n)
    is left out of its row's fold; max_src wider than any list and num_dst = 0 are fine too."""
    rs = np.random.RandomState(9)
    g, b, s = (dev(x) for x in MC.window_outputs(rs, 6))
    store = torch.full((5, 27), SENTINEL, dtype=torch.float32, device=DEV)
    bad = np.array([[-1, 0, 0, 1, -1, -1], [5, 0, 2, -1, -1, -1], [1 << 20, 1, 3, -1, -1, -1], [-(1 << 31), 0, 4, -1, -1, -1]], dtype=np.int32)
    launch(dev(bad), 4, g, b, s, None, store)
    launch(dev(bad), 4, g, b, s, None, store, num_dst=0)
    assert bool((store == SENTINEL).all())
    mixed = np.array([[3, 0, 2, 99, 3, -7], [1, 0, 6, 0, 1 << 30, -1], [0, 0, -1, 6, 7, -(1 << 31)], [9, 0, 1, 2, 3, 4]], dtype=np.int32)
    clean = np.array([[3, 0, 2, 3, -1, -1], [1, 0, 0, -1, -1, -1]], dtype=np.int32)
    other = torch.full((5, 27), SENTINEL, dtype=torch.float32, device=DEV)
    launch(dev(mixed), 4, g, b, s, None, store)
    launch(dev(clean), 4, g, b, s, None, other)
    got = store.cpu().numpy()
    assert np.array_equal(bits(got), bits(other.cpu().numpy()))
    assert (got[[0, 2, 4]] == SENTINEL).all() and not (got[[1, 3]] == SENTINEL).any()    # row 0: every source out of range, nothing written
    # a cont = 1 row whose sources are all out of range keeps the stored row
    launch(dev(np.array([[3, 1, 6, -1, 1 << 24, -1]], dtype=np.int32)), 4, g, b, s, None, store)
    assert np.array_equal(bits(store.cpu().numpy()), bits(got))
    # argument checks come back as errors, nothing is launched
    for kw in (dict(max_src=0), dict(rows=0)):
        rc = L.load().mcg_merge_windows(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(g.data_ptr()), C.c_void_p(b.data_ptr()),
                                        C.c_void_p(s.data_ptr()), 6, C.c_void_p(0), 0, C.c_void_p(dev(clean).data_ptr()), 2, kw.get('max_src', 4),
                                        C.c_void_p(store.data_ptr()), kw.get('rows', 5), 0.5)
        assert rc != L.MCG_OK, kw


def test_two_calls_in_a_graph():
    """(7, 4), L = 12, one window per call: the first call runs eagerly, calls two and three -- whose rows continue from the store
    (cont = 1) -- are captured into ONE graph and replayed twice; each replay gives the eager result."""
    plan = harness.plan_windows(12)
    rs = np.random.RandomState(5)
    outs = [MC.window_outputs(rs, 7) for _ in plan]
    scale = dev(np.array([224 / 177, 224 / 199, 224 / 177, 224 / 199], dtype=np.float32))
    calls = []
    MC.run_plan(plan, outs, [[0], [1], [2]], lambda t, m, g, b, s, sc: calls.append((dev(t), m, dev(g), dev(b), dev(s), scale)))
    assert all(bool(c[0][:, 1].any()) for c in calls[1:])
    store = torch.full((12, 27), SENTINEL, dtype=torch.float32, device=DEV)
    launch(*calls[0], store)
    after_first = store.clone()
    for c in calls[1:]:
        launch(*c, store)
    eager = store.cpu().numpy()
    want = MC.reference(plan, outs, np.array([224 / 177, 224 / 199, 224 / 177, 224 / 199], dtype=np.float32))
    assert np.array_equal(bits(eager), bits(want))
    store.copy_(after_first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for c in calls[1:]:
            launch(*c, store)
    for _ in range(2):
        store.copy_(after_first)
        graph.replay()
        assert np.array_equal(bits(store.cpu().numpy()), bits(eager))


# ------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def engines():
    from mcgaze_amd.engine import HipEngine
    sd = synth.make_state_dict(0)
    return {p: HipEngine(sd, precision=p) for p in ('f16x3', 'fp32')}


def cat(parts, key):
    return np.concatenate([harness._host(p[key]) for p in parts])


def same(parts, want, what):
    for k in ('det', 'fused', 'others'):
        a, b = cat(parts, k), cat(want, k)
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, k)
    assert [p['first'] for p in parts] == [p['first'] for p in want], what


SF = (224 / 177, 1.25, 224 / 177, 1.25)


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_gaze_stream_device_merge(engines, precision):
    e = engines[precision]
    for L_ in (5, 12, 30):
        v = torch.from_numpy(synth.make_clips(70 + L_, 1, L_, 64, 64)).to(DEV)
        for step in (1, 3, 8):
            runs = {}
            for name, kw in (('host', {}), ('device', dict(merge='device')), ('results', dict(merge='device', results='device'))):
                s = GazeStream(e, 64, 64, scale_factor=SF, **kw)
                runs[name] = [s.push(v[a:a + step]) for a in range(0, L_, step)] + [s.finish()]
            assert all(isinstance(p[k], np.ndarray) for p in runs['device'] for k in ('det', 'fused', 'others'))
            assert all(isinstance(p[k], torch.Tensor) and p[k].is_cuda and p[k].dtype == torch.float32
                       for p in runs['results'] for k in ('det', 'fused', 'others'))
            assert all(tuple(p['det'].shape[1:]) == (3, 5) and tuple(p['others'].shape[1:]) == (3, 3) for p in runs['results'])
            same(runs['device'], runs['host'], (precision, L_, step, 'device'))
            same(runs['results'], runs['host'], (precision, L_, step, 'results'))
            assert cat(runs['host'], 'det').shape[0] == L_


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_pool_device_merge(engines, precision):
    """Three streams of 5, 12 and 23 frames at different pace; the short one is closed mid-run, while the others go on."""
    e = engines[precision]
    lengths = (5, 12, 23)
    vids = [torch.from_numpy(synth.make_clips(90 + i, 1, n, 64, 64)).to(DEV) for i, n in enumerate(lengths)]
    pace = (1, 2, 3)

    def run(**kw):
        pool = GazeStreamPool(e, 64, 64, rows=40, scale_factor=SF, **kw)
        sids = [pool.open() for _ in lengths]
        got, sent = {s: [] for s in sids}, [0] * 3
        while pool.pending() or any(a < n for a, n in zip(sent, lengths)):
            for i, s in enumerate(sids):
                if sent[i] < lengths[i]:
                    pool.push(s, vids[i][sent[i]:sent[i] + pace[i]])
                    sent[i] = min(lengths[i], sent[i] + pace[i])
                    if sent[i] == lengths[i]:
                        pool.close(s)
            for s, r in pool.step().items():
                got[s].append(r)
        assert pool.store.free_rows() == 40
        if pool.dmerger is not None:                          # every row of the result store came back
            assert not pool.dmerger.streams and len(pool.dmerger._free) == pool.dmerger.store.shape[0]
        return [got[s] for s in sids]

    want = run()
    for kw in (dict(merge='device'), dict(merge='device', results='device')):
        got = run(**kw)
        for i in range(3):
            same(got[i], want[i], (precision, kw, i))
            assert cat(got[i], 'det').shape[0] == lengths[i]
        if kw.get('results') == 'device':
            assert all(p[k].is_cuda for g in got for p in g for k in ('det', 'fused', 'others'))


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_run_videos_device_merge(engines, precision):
    e = engines[precision]
    videos = [dict(id=i + 1, frames=torch.from_numpy(synth.make_clips(30 + i, 1, n, 64, 64))) for i, n in enumerate((5, 12, 23))]
    for kw in (dict(batch_clips=2, scale_factor=SF), dict(batch_clips=3, reuse_frames=True), dict(batch_clips=4, mixed_lengths=True, scale_factor=SF)):
        want = harness.run_videos(e, videos, **kw)
        got = harness.run_videos(e, videos, merge='device', **kw)
        assert got == want, (precision, kw)
        assert [len(r['fusion_gazes']) for r in got] == [5, 12, 23]


def test_head_arrows_on_device_results(engines):
    e = engines['f16x3']
    v = torch.from_numpy(synth.make_clips(3, 1, 9, 64, 64)).to(DEV)
    s = GazeStream(e, 64, 64, merge='device', results='device')
    parts = [s.push(v), s.finish()]
    fused = torch.cat([p['fused'] for p in parts])
    rs = np.random.RandomState(1)
    boxes = rs.uniform(0, 400, (9, 4)).astype(np.float32)
    boxes[:, 2:] += boxes[:, :2]
    got = harness.head_arrows(torch.from_numpy(boxes).to(DEV), fused)
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (9, 2, 2)
    assert np.array_equal(got.cpu().numpy(), harness.head_arrows(boxes, fused.cpu().numpy()))
    assert np.array_equal(harness.head_arrows(boxes, fused).cpu().numpy(), got.cpu().numpy())
