"""-m gpu: ragged batches -- clips of different lengths in one forward / decode / stage (mcg_*_ragged, HipEngine.forward / decode and
engine.stage_forward with a sequence of lengths, harness.run_videos(mixed_lengths=True), harness.run_tracks, model(clip_length=[...])).

Everything is asserted BIT FOR BIT against the per-clip path (one call per clip with clip_length = its length), which the goldens and the
oracle pin; no new tolerance.  The one exception is the f16 engine in a call whose longest clip exceeds 10 frames: such a call runs the
unfused attention sequence for ALL its clips, a short clip run alone takes the fused block, and for fp16 the two differ by one ulp
(tests/test_gpu_kernels.py::test_mlp_chain_matches_unfused_bitwise[float16], whose constants F16_NDIFF / F16_DMAX are taken here).  So
for f16 the long clips of a mixed call are asserted bit for bit and the short ones to that bound; fp32 / f16x3 / bf16 are bit for bit
throughout.  No test hands the kernels an invalid clip table: the guard is there for callers, not to be provoked."""
import os

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import lib as L
from oracle import mcgaze_oracle as orc
from tests.test_gpu_forward import F32_TOL, KEYS     # the golden tests' bounds (test 5 takes them as they are)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EXACT = ('fp32', 'f16x3', 'bf16')           # fused and unfused attention agree bit for bit
PRECISIONS = EXACT + ('f16',)
SHORT = [7, 1, 10, 3, 7, 2]                 # every clip <= 10 frames: the fused attention block
MIXED = [7, 11, 4, 23]                      # a clip > 10 frames: the whole call takes the unfused sequence
F16_NDIFF, F16_DMAX = 0.06, 2.5e-3          # test_mlp_chain_matches_unfused_bitwise[float16]: differing share, max |d| / max(scale, 1)
OUT = ('gaze', 'boxes', 'scores')


@pytest.fixture(scope='module')
def engines():
    from mcgaze_amd.engine import HipEngine
    sd = synth.make_state_dict(0)
    return {p: HipEngine(sd, precision=p) for p in PRECISIONS}


def bits(t):
    return t.contiguous().view(torch.int32)


def frames(seed, n, H=224, W=224):
    return torch.from_numpy(synth.make_clips(seed, 1, n, H, W)).to(DEV)


def spans(lengths):
    s = np.concatenate([[0], np.cumsum(lengths)])
    return [(int(a), int(b)) for a, b in zip(s[:-1], s[1:])]


def rows(out, a, b):
    """Frames [a, b) of a forward's outputs (gaze is [4, N, 3])."""
    return dict(gaze=out['gaze'][:, a:b], boxes=out['boxes'][a:b], scores=out['scores'][a:b])


def clone(out):
    return {k: v.clone() for k, v in out.items()}


def check_clip(got, ref, where, exact=True):
    for k in OUT:
        a, b = got[k], ref[k]
        same = torch.equal(bits(a), bits(b))
        ndiff, dmax, scale = int((a != b).sum()), float((a - b).abs().max()), float(b.abs().max())
        if not same:
            print(f'{where} {k}: {ndiff} of {a.numel()} elements differ, max |d| = {dmax:.3e} (scale {scale:.2f})')
        if exact:
            assert same, (where, k, ndiff, dmax)
        else:
            assert same or (ndiff <= F16_NDIFF * a.numel() and dmax <= F16_DMAX * max(scale, 1.0)), (where, k, ndiff, dmax)


def check_against_per_clip(e, precision, lengths, got, per_clip, what):
    """got: the ragged call's outputs; per_clip(a, b) -> the outputs of the call that holds clip [a, b) alone."""
    call_is_unfused = max(lengths) > 10
    for ci, (a, b) in enumerate(spans(lengths)):
        ref = per_clip(a, b)
        torch.cuda.synchronize()
        exact = precision != 'f16' or not call_is_unfused or b - a > 10
        check_clip(rows(got, a, b), ref, f'{what} {precision} clip {ci} ({b - a} frames)', exact)


# ---------------------------------------------------------------- 1. ragged equals per clip
@pytest.mark.parametrize('lengths', [SHORT, MIXED], ids=['short', 'mixed'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_ragged_forward_equals_per_clip(engines, precision, lengths):
    e = engines[precision]
    x = frames(21 + len(lengths), sum(lengths))
    got = clone(e.forward(x, lengths))
    check_against_per_clip(e, precision, lengths, got, lambda a, b: e.forward(x[a:b].contiguous(), b - a), 'forward')


@pytest.mark.parametrize('with_hw', [False, True], ids=['full', 'img_hw'])
@pytest.mark.parametrize('lengths', [SHORT, MIXED], ids=['short', 'mixed'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_ragged_decode_equals_per_clip(engines, precision, lengths, with_hw):
    """decode over a pyramid store of 19 rows with a frame_of table that permutes and repeats them: one ragged call against forward on each
    clip's gathered frames (what test_gpu_window_reuse.py pins the per-window decode to)."""
    e = engines[precision]
    K, N = 19, sum(lengths)
    x = frames(33, K)
    rs = np.random.RandomState(5 + N)
    table = np.concatenate([rs.permutation(K), rs.randint(0, K, N)])[:N].astype(np.int64)
    hw = np.stack([rs.randint(112, 225, K), rs.randint(112, 225, K)], axis=1).astype(np.int32) if with_hw else None
    pyr = e.backbone_fpn(x)
    got = clone(e.decode(pyr, table.tolist(), lengths, img_hw=hw))
    idx = torch.from_numpy(table).to(DEV)

    def per_clip(a, b):
        return e.forward(x[idx[a:b]].contiguous(), b - a, img_hw=None if hw is None else hw[table[a:b]])
    check_against_per_clip(e, precision, lengths, got, per_clip, 'decode')


# ---------------------------------------------------------------- 2. uniform lengths, both entries
@pytest.mark.parametrize('precision', PRECISIONS)
def test_uniform_lengths_through_both_entries(engines, precision):
    e = engines[precision]
    x = frames(41, 35)
    ref = clone(e.forward(x, 7))
    got = e.forward(x, [7] * 5)
    torch.cuda.synchronize()
    check_clip(got, ref, f'uniform {precision}')


# ---------------------------------------------------------------- 3. order of clips
@pytest.mark.parametrize('precision', PRECISIONS)
def test_clip_order_does_not_matter(engines, precision):
    e = engines[precision]
    sp = spans(SHORT)
    x = frames(43, sum(SHORT))
    ref = clone(e.forward(x, SHORT))
    order = [4, 0, 5, 2, 1, 3]
    xp = torch.cat([x[sp[c][0]:sp[c][1]] for c in order]).contiguous()
    lp = [SHORT[c] for c in order]
    got = e.forward(xp, lp)
    torch.cuda.synchronize()
    for (a, b), c in zip(spans(lp), order):
        check_clip(rows(got, a, b), rows(ref, *sp[c]), f'permuted {precision} clip {c}')


# ---------------------------------------------------------------- 4. stage level
def _stage_inputs(N, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    roi = (torch.randn(N * 3, 49, 256, generator=g) * 3).to(dtype).to(DEV)
    obj = torch.randn(N, 3, 256, generator=g).to(dtype).to(DEV)
    boxes = (torch.tensor([[20., 30., 200., 210.], [60., 50., 160., 150.], [90., 60., 130., 100.]])[None].repeat(N, 1, 1)
             + torch.randn(N, 3, 4, generator=g)).to(DEV)
    return roi, obj, boxes


def _same(a, b):
    return torch.equal(a.view(torch.int16) if a.element_size() == 2 else a.view(torch.int32), b.view(torch.int16) if b.element_size() == 2 else b.view(torch.int32))


@pytest.mark.parametrize('kind', ['f16x3', 'bf16'])
def test_ragged_stage_block_matches_unfused_bitwise(kind):
    """The ragged counterpart of test_attn_block_x3_matches_unfused_bitwise / test_mlp_chain_matches_unfused_bitwise[bfloat16]: one stage
    over clips of [7, 1, 10, 3] frames -- the fused attention block reading the clip table against the launch sequences
    (MCG_FLAG_NO_ATTN_BLOCK: attn_core_kernel reading the table; MCG_FLAG_NO_SPECIALISED: no chains at all), and against one
    equal-length stage call per clip."""
    from mcgaze_amd import engine as eng
    from mcgaze_amd.packing import PackedWeights
    lengths = [7, 1, 10, 3]
    N = sum(lengths)
    split = kind == 'f16x3'
    dtype = torch.float32 if split else torch.bfloat16
    pw = PackedWeights(synth.make_state_dict(0), dtype=dtype, split=split)
    roi, obj, boxes = _stage_inputs(N, dtype, 900)
    modes = [('block', 0), ('generic', L.FLAG_NO_SPECIALISED)] + ([('chains', L.FLAG_NO_ATTN_BLOCK)] if split else [])
    outs = {m: [t.clone() for t in eng.stage_forward(pw.stages[2], roi, obj, boxes, lengths, split=split, flags=f)] for m, f in modes}
    torch.cuda.synchronize()
    for m, _ in modes[1:]:
        for name, a, b in zip(('obj', 'boxes', 'cls'), outs['block'], outs[m]):
            assert _same(a, b), (f'block vs {m}', name, float((a.float() - b.float()).abs().max()))
    for a, b in spans(lengths):
        ref = eng.stage_forward(pw.stages[2], roi[3 * a:3 * b].contiguous(), obj[a:b].contiguous(), boxes[a:b].contiguous(), b - a, split=split)
        torch.cuda.synchronize()
        for name, r, g in zip(('obj', 'boxes', 'cls'), ref, outs['block']):
            assert _same(r, g[a:b].contiguous()), ('per clip', (a, b), name)


# ---------------------------------------------------------------- 5. oracle
@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_ragged_forward_matches_the_oracle_per_clip(engines, precision):
    """One ragged call against oracle.mcgaze_oracle.forward run clip by clip on the CPU, held to the bounds
    tests/test_gpu_forward.py::test_fp32_engine_matches_reference_golden uses for the goldens: (yaw, pitch) within F32_TOL = 1e-3 on all
    four gaze outputs, boxes within 5e-3 px, scores within 1e-3."""
    lengths = [7, 3, 5]
    N = sum(lengths)
    sd = synth.make_state_dict(0)
    img = synth.make_clips(77, 1, N)
    out = engines[precision].forward(torch.from_numpy(img).to(DEV), lengths)
    torch.cuda.synchronize()
    gaze, boxes, scores = out['gaze'].cpu(), out['boxes'].cpu().numpy(), out['scores'].cpu().numpy()
    for a, b in spans(lengths):
        det, want = orc.forward(sd, img[a:b], synth.make_img_metas(b - a), b - a)
        for i, k in enumerate(KEYS):
            d = orc.yaw_pitch_diff(gaze[i, a:b], want[k]).max().item()
            print(f'{precision} clip [{a}, {b}) {k}: max |d(yaw,pitch)| = {d:.2e}')
            assert d < F32_TOL, (k, d)
        det = det.numpy()
        print(f'{precision} clip [{a}, {b}) boxes: max |d| = {float(np.abs(boxes[a:b] - det[..., :4]).max()):.2e} px')
        np.testing.assert_allclose(boxes[a:b], det[..., :4], atol=5e-3, rtol=0)
        np.testing.assert_allclose(scores[a:b], det[..., 4], atol=1e-3)


# ---------------------------------------------------------------- 6. a long clip
@pytest.mark.parametrize('precision', EXACT)
def test_demo_sized_clip_beside_short_ones(engines, precision):
    """101 frames (what the demo feeds at most: max_len = 100) beside two 7-frame clips, 64 x 64 padded frames."""
    e = engines[precision]
    lengths = [7, 101, 7]
    x = frames(51, sum(lengths), 64, 64)
    got = clone(e.forward(x, lengths))
    check_against_per_clip(e, precision, lengths, got, lambda a, b: e.forward(x[a:b].contiguous(), b - a), 'long')


# ---------------------------------------------------------------- 7. harness
@pytest.mark.parametrize('reuse_frames', [False, True])
def test_run_videos_mixed_lengths_gives_the_same_records(engines, reuse_frames):
    e = engines['f16x3']
    g = torch.Generator().manual_seed(61)
    videos = [dict(id=i, frames=torch.randn(n, 3, 96, 96, generator=g)) for i, n in enumerate((3, 7, 8, 12, 30))]
    want = harness.run_videos(e, videos, reuse_frames=reuse_frames)
    got = harness.run_videos(e, videos, reuse_frames=reuse_frames, mixed_lengths=True)
    assert got == want


@pytest.mark.parametrize('precision', EXACT)
def test_run_tracks_equals_one_forward_per_chunk(engines, precision):
    e = engines[precision]
    g = torch.Generator().manual_seed(62)
    tracks = [dict(id=f'person{i}', frames=torch.randn(n, 3, 64, 64, generator=g)) for i, n in enumerate((5, 101, 102, 230))]
    out = harness.run_tracks(e, tracks)
    assert [o['id'] for o in out] == [t['id'] for t in tracks]
    for t, o in zip(tracks, out):
        n = t['frames'].shape[0]
        assert o['det'].shape == (n, 3, 5) and o['fused'].shape == (n, 3) and o['others'].shape == (n, 3, 3)
        for a, b in harness.plan_track_chunks(n, 100):
            ref = e.forward(t['frames'][a:b].to(DEV).contiguous(), b - a)
            torch.cuda.synchronize()
            where = (precision, t['id'], a, b)
            assert np.array_equal(o['det'][a:b, :, :4], ref['boxes'].cpu().numpy()), where
            assert np.array_equal(o['det'][a:b, :, 4], ref['scores'].cpu().numpy()), where
            assert np.array_equal(o['fused'][a:b], ref['gaze'][0].cpu().numpy()), where
            assert np.array_equal(o['others'][a:b], ref['gaze'][1:].permute(1, 0, 2).cpu().numpy()), where


# ---------------------------------------------------------------- 8. registry surface
def test_registry_surface_takes_a_list_of_lengths():
    from mcgaze_amd import init_detector
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    model = init_detector(os.path.join(root, 'configs', 'mcgaze', 'r50_clip7_gaze360.py'), None, device=DEV, precision='fp32')
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state_dict(0).items()}, strict=True)
    img = torch.from_numpy(synth.make_clips(71, 1, 12))
    metas = synth.make_img_metas(12)

    def run(x, m, **kw):
        with torch.no_grad():
            (det, labels), gaze = model(img=[x], img_metas=[m], return_loss=False, format=False, **kw)
        torch.cuda.synchronize()
        return torch.stack(det).clone(), {k: v.clone() for k, v in gaze.items()}
    det, gaze = run(img, metas, clip_length=[7, 5])
    assert tuple(det.shape) == (12, 3, 5) and set(gaze) == set(KEYS)
    for a, b in ((0, 7), (7, 12)):
        d, g = run(img[a:b], metas[a:b])
        assert torch.equal(bits(det[a:b]), bits(d))
        for k in KEYS:
            assert torch.equal(bits(gaze[k][a:b]), bits(g[k])), k


# ---------------------------------------------------------------- 9. graph capture
@pytest.mark.parametrize('precision', ['f16x3', 'bf16'])
def test_ragged_forward_is_graph_capturable(engines, precision):
    """The ragged call reads nothing back (num_clips and max_clip_length are host integers), so it captures into a HIP graph like the
    equal-length one: eager warm-up on the capture stream first (GraphedForward, INTEGRATION.md "Streams"), the clip table uploaded once
    before the capture; the replay gives the eager bits, also on new frames."""
    from mcgaze_amd.engine import GraphedForward
    e = engines[precision]
    lengths = [7, 3, 10, 1]
    x = frames(81, sum(lengths))
    ref = clone(e.forward(x, lengths))
    gf = GraphedForward(e, sum(lengths), 224, 224, lengths)
    got = gf(x)
    torch.cuda.synchronize()
    check_clip(got, ref, f'graph {precision}')
    y = frames(82, sum(lengths))
    ref = clone(e.forward(y, lengths))
    got = gf(y)
    torch.cuda.synchronize()
    check_clip(got, ref, f'graph {precision}, second input')


@pytest.mark.parametrize('precision', ['f16x3', 'bf16'])
def test_pipelined_runner_takes_a_list_of_lengths(engines, precision):
    """The two-deep batch pipeline with ragged batches (mcg_decoder_forward_deferred_ragged): three batches equal forward's bits."""
    from mcgaze_amd.engine import PipelinedRunner
    e = engines[precision]
    N = sum(SHORT)
    runner = PipelinedRunner(e, N, 224, 224, SHORT)
    xs = [frames(90 + k, N) for k in range(3)]
    outs = [dict(gaze=torch.empty(4, N, 3, device=DEV), boxes=torch.empty(N, 3, 4, device=DEV), scores=torch.empty(N, 3, device=DEV)) for _ in xs]
    for x, o in zip(xs, outs):
        runner.submit(x, o)
    runner.flush()
    torch.cuda.synchronize()
    for k, (x, o) in enumerate(zip(xs, outs)):
        ref = e.forward(x, SHORT)
        torch.cuda.synchronize()
        check_clip(o, ref, f'pipeline {precision} batch {k}')
