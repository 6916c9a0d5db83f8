"""-m gpu: mcg_stage_forward -- attn_block* / attn_core_kernel, chain* / pw_single* / dynconv_kernel / dynconv_x3_kernel, ln_kernel and
heads_kernel -- against the FLOAT64 oracle, in every engine kind, at the clip lengths where the launch sequence changes, across operand
magnitudes and through the delta2bbox clamp.  tests/decoder_cases.py holds the cases, the references and the bounds (all computed on the
CPU from STAGE_TOL, the f32 oracle's own error and a model of the f16x3 number format -- none from a GPU result);
tests/test_decoder_cases_cpu.py proves the cases and that each bound rejects the mutants listed there.

BASE        (B, T) = (1, 7), (2, 3), (3, 1): the shapes of test_decoder_stage, now against float64.
T_EDGE      T = 10 (30 of the attention block's 32 tile rows), T = 11 (the first T on the launch sequence), T = 33 (attn_core_kernel's
            second trip), and ragged batches [10, 1, 3] (block kernel with a clip table) and [11, 2] (launch sequence with one).
MAGNITUDE   21 tokens, fp32 and f16x3: theta, RoI features, fc_layer, the towers and the FFN's hidden tensor scaled down by 2^-k.  The
            decoder's matrices are packed without a power-of-two pre-scale and DynamicConv's two products have data on both sides, so
            small operands reach the fp16 halves' subnormal range.  f16x3 must stay within MARGIN x the format model; fp32, whose MFMA
            has no such dependence, keeps the BASE bound -- the control.
CLAMP       dw / dh rows of fc_reg scaled so that tokens are clamped above, below and not at all; boxes per token; a second case with
            std 2 on dw / dh, where the order of clamp and multiplication matters.

Where a specialised path exists at the shape -- B1T7, B1T10, theta_k10 -- the generic launch sequence (MCG_FLAG_NO_SPECIALISED) and, f16x3,
the chain sequence (MCG_FLAG_NO_ATTN_BLOCK) are run too, each against float64, not against each other.  Measured figures: DESIGN.md 3.2.
"""
import pytest
import torch

from mcgaze_amd import lib as L
from tests import decoder_cases as D

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
VARIANT_CASES = ('B1T7', 'B1T10', 'theta_k10')
# f16x3 MAGNITUDE cases that exceed the bound of the stated sites.  Cause (read, then reproduced by the format model on the CPU,
# test_decoder_cases_cpu.py::test_unscaled_packing_explains_the_cases_over_their_bound): the family scales a weight matrix that packing.py
# split-packs WITHOUT a power-of-two pre-scale -- dynamic_layer.weight, ffn.layers.0.0.weight -- so the packed low halves lose k bits before a
# kernel runs; the kernels stay within the format as packed (test_magnitude_as_packed).  The fix is a pre-scale with a descale factor for
# igemm / pw_single_x3 linear calls of the decoder: a new ABI field.  Figures: worst GPU error / bound over both stages.
OVER_THE_STATED_BOUND = {
    ('theta_k6', 'f16x3'): 'obj 1.9e-5 / 1.1e-5, cls 2.8e-5 / 1.7e-5, boxes 7.8e-6 / 2.3e-6: dynamic_layer.weight x 2^-6 is packed unscaled',
    ('theta_k10', 'f16x3'): 'obj 2.5e-4 / 9.1e-5, cls 2.2e-4 / 7.9e-5, boxes 7.5e-5 / 2.1e-5: dynamic_layer.weight x 2^-10 is packed unscaled',
    ('ffn_hidden_k6', 'f16x3'): 'obj 9.6e-6 / 8.5e-6, cls 1.1e-5 / 9.2e-6, boxes 2.6e-6 / 2.2e-6: ffn.layers.0.0.weight x 2^-6 is packed unscaled',
}
_PACKED = {}


@pytest.fixture(scope='module')
def eng():
    from mcgaze_amd import engine
    return engine


def _packed(case, kind):
    """Packed weights, once per (state dict, kind)."""
    from mcgaze_amd.packing import PackedWeights
    sd = D.case_sd(case)
    key = (id(sd), kind)
    if key not in _PACKED:
        _PACKED[key] = PackedWeights(sd, dtype=D.KIND_DTYPE[kind], split=kind == 'f16x3', device=DEV)
    return _PACKED[key]


def _variants(case, kind):
    v = [('default', 0)]
    if case.name in VARIANT_CASES:
        v.append(('generic', L.FLAG_NO_SPECIALISED))
        if kind == 'f16x3':
            v.append(('chains', L.FLAG_NO_ATTN_BLOCK))
    return v


def _check(eng, name, kind, packed=False):
    case = D.CASES[name]
    dtype, split = D.KIND_DTYPE[kind], kind == 'f16x3'
    pw = _packed(case, kind)
    roi, obj, boxes = D.inputs(case)
    roi_dev = roi.permute(0, 2, 3, 1).reshape(-1, 49, 256).contiguous().to(dtype).to(DEV)
    obj_dev, boxes_dev = obj.to(dtype).to(DEV), boxes.to(DEV)
    outs = [(s, what, eng.stage_forward(pw.stages[s], roi_dev, obj_dev, boxes_dev, D.engine_clips(case), stds=case.stds, split=split, flags=flags))
            for s in D.STAGES for what, flags in _variants(case, kind)]
    torch.cuda.synchronize()
    failed = []
    for s, what, (o, b, c) in outs:
        ref, fl, bd = D.reference(name, s, dtype), D.floor(name, s, dtype), D.bound(name, s, kind, packed)
        m = D.model(name, s, packed) if case.group == 'MAGNITUDE' else {}
        out = dict(obj=o.cpu(), boxes=b.cpu(), cls=c.cpu())
        assert all(bool(torch.isfinite(t).all()) for t in out.values()), (name, kind, s, what)
        e = D.errors(out, ref)
        print(f'{name} stage {s} {kind} {what}: ' + ', '.join(
            f'{k} {e[k]:.2e} (floor {fl[k]:.1e}' + (f', model {m[k]:.1e}' if m else '') + f', bound {bd[k]:.2e})' for k in bd) +
            ('' if 'boxes' in bd else f', boxes (max-norm, not asserted) {e["boxes"]:.2e}'))
        failed += [(s, what, k, e[k], bd[k]) for k in bd if not e[k] < bd[k]]
    assert not failed, (name, kind, failed)


def _params(cases):
    xf = lambda c, kind: [pytest.mark.xfail(strict=True, reason=OVER_THE_STATED_BOUND[c.name, kind])] if (c.name, kind) in OVER_THE_STATED_BOUND else []
    return [pytest.param(c.name, kind, id=f'{c.name}-{kind}', marks=xf(c, kind)) for c in cases for kind in D.kinds_of(c)]


@pytest.mark.parametrize('name,kind', _params(D.BASE))
def test_base(eng, name, kind):
    _check(eng, name, kind)


@pytest.mark.parametrize('name,kind', _params(D.T_EDGE))
def test_t_edge(eng, name, kind):
    _check(eng, name, kind)


@pytest.mark.parametrize('name,kind', _params(D.MAGNITUDE))
def test_magnitude(eng, name, kind):
    _check(eng, name, kind)


@pytest.mark.parametrize('name,kind', sorted(OVER_THE_STATED_BOUND))
def test_magnitude_as_packed(eng, name, kind):
    """The cases over their stated bound, held to the format as the weights are packed today: the model with the scaled matrix's own
    site added (decoder_cases.PACK_SITES).  What the strict xfails above leave open is the packing, not these kernels."""
    _check(eng, name, kind, packed=True)


@pytest.mark.parametrize('name,kind', _params(D.CLAMP))
def test_clamp(eng, name, kind):
    _check(eng, name, kind)
