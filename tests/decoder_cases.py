"""Shared by tests/test_decoder_cases_cpu.py and tests/test_gpu_decoder.py: the decoder stage (mcg_stage_forward) against a FLOAT64
run of the oracle, across clip lengths, operand magnitudes and the delta2bbox clamp.  CPU only, seeded, cached.

THE REFERENCE is oracle.mcgaze_oracle.stqi_stage + delta2bbox on a float64 copy of the state dict and of the inputs (the inputs first
rounded to the storage type of the engine kind, as the kernel receives them).  Ragged batches are run clip by clip and concatenated.

THE FORMAT MODEL.  An f16x3 contraction splits each operand into two fp16 halves, hi = RTZ_f16(x), lo = RTZ_f16(x - hi) (subnormal
halves kept, each half saturating at +-65504), and sums lo.hi + hi.lo + hi.hi.  ``split_rtz16`` / ``x3_product`` state that in float64
with the three terms summed exactly; ``x3_hooks(sites)`` substitutes it at named contraction sites of the oracle.  With the low halves
zeroed it is the 11-BIT MUTANT: a kernel that lost its low-half terms.

THE BOUNDS are computed here, on the CPU, from three things only: STAGE_TOL (the bounds tests/test_gpu_kernels.py::test_decoder_stage
holds today against the f32 oracle), ``floor`` (the f32 oracle's own distance to the float64 one on the case) and ``model`` (the format
model's distance to float64 with the case's stressed sites substituted).  ``bound`` says how they combine per group.  Nothing here is
taken from a GPU result.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

from mcgaze_amd import synth
from oracle import mcgaze_oracle as orc

# the kinds, their storage types and the bounds test_decoder_stage holds today against the f32 oracle
from tests.test_gpu_kernels import KINDS, KIND_DTYPE, STAGE_TOL  # noqa: E402

STAGES = (0, 3)
STDS = (0.5, 0.5, 1.0, 1.0)
MAX_RATIO = abs(math.log(16 / 1000))
OUTS = ('obj', 'cls', 'boxes')
# The one margin on a modelled or measured CPU figure (f16x3 MAGNITUDE: on ``model``; CLAMP: on ``floor_tok``).  The model sums its three
# terms exactly and keeps every subnormal; the kernel accumulates them in f32 inside the MFMA in an order the ISA does not state, K = 64 to
# 12544 terms deep.  4 covers that and is small against the 11-bit mutant, which sits orders of magnitude above the 22-bit model.
MARGIN = 4

# family -> the oracle's contraction sites it stresses
FAMILY_SITES = {'theta': ('dyn_in', 'dyn_out'), 'roi': ('dyn_in',), 'fc': ('fc_layer',), 'towers': ('cls_fc', 'reg_fc'), 'ffn_hidden': ('ffn2',)}

# family -> the site whose WEIGHT MATRIX the family scales without the table above naming it.  The decoder's matrices are split-packed
# without a power-of-two pre-scale (packing.py), so 2^-k on dynamic_layer.weight (|w| ~ 0.06) or ffn.layers.0.0.weight costs the packed
# low halves k bits before any kernel runs: ``model(..., packed=True)`` adds these sites, and ``bound(..., packed=True)`` is the bound a
# kernel that is as good as the format AS PACKED must keep.
PACK_SITES = {'theta': ('dynamic_layer',), 'ffn_hidden': ('ffn1',)}

Case = collections.namedtuple('Case', 'name group clips family k stds')
#   clips: (B, T) for equal-length clips, or a list of per-clip lengths (the engine's clip-list form, the oracle clip by clip)


def _case(name, group, clips, family=None, k=0, stds=STDS):
    return Case(name, group, clips, family, k, stds)


BASE = [_case(f'B{b}T{t}', 'BASE', (b, t)) for b, t in ((1, 7), (2, 3), (3, 1))]
T_EDGE = [_case(f'B{b}T{t}', 'T_EDGE', (b, t)) for b, t in ((1, 10), (2, 10), (1, 11), (1, 33))] + \
         [_case('ragged_' + '_'.join(map(str, c)), 'T_EDGE', list(c)) for c in ((10, 1, 3), (11, 2))]
# fc k = 3 stands beside fc k = 6: fc_layer's weights (K = 12544, |w| ~ 0.009) have subnormal low halves already unscaled, and at k = 6
# the high halves are subnormal too -- the format itself is down to 11-12 bits there (model 1.5e-4) and MARGIN x model lies above the
# 11-bit mutant (2e-4).  k = 6 still holds the kernel to its format; k = 3 is the largest k at which the bound also rejects the mutant
# on every output of both stages (test_decoder_cases_cpu.py prints both).
MAGNITUDE = [_case(f'{fam}_k{k}', 'MAGNITUDE', (1, 7), fam, k)
             for fam, k in (('theta', 6), ('theta', 10), ('roi', 6), ('roi', 10), ('fc', 3), ('fc', 6), ('towers', 6), ('ffn_hidden', 6))]
MUTANT_BLIND = {('fc_k6', 'f16x3')}     # (case, kind) whose bound cannot tell the 11-bit mutant from the format: see above
# CLAMP: ``k`` is the factor on the dw / dh rows of fc_reg.  The product factor x std is 48 in both cases: 8 clamps 1 of 21 tokens with
# these weights and inputs, and of 8, 16, 24, 32, 48 the last is the first at which dw and dh are each clamped above, clamped below and
# left alone for at least CLAMP_MIN_TOKENS tokens in both stages.  The second case moves the std off 1: only there does "clamp, then
# multiply" differ from "multiply, then clamp".
CLAMP_MIN_TOKENS = 2
CLAMP = [_case('clamp', 'CLAMP', (1, 7), 'clamp', 48), _case('clamp_std2', 'CLAMP', (1, 7), 'clamp', 24, stds=(0.5, 0.5, 2.0, 2.0))]
CASES = {c.name: c for c in BASE + T_EDGE + MAGNITUDE + CLAMP}
assert len(CASES) == len(BASE + T_EDGE + MAGNITUDE + CLAMP)


def clip_lengths(case):
    return list(case.clips) if isinstance(case.clips, list) else [case.clips[1]] * case.clips[0]


def engine_clips(case):
    """What mcgaze_amd.engine.stage_forward takes as ``clip_length``."""
    return list(case.clips) if isinstance(case.clips, list) else case.clips[1]


def num_frames(case):
    return sum(clip_lengths(case))


def scale_err(a, b):
    """max |a - b| over max |b|: the metric of STAGE_TOL."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def token_err(a, b):
    """Boxes, per token: max |d| over the token's four coordinates over the token's largest coordinate; the worst token.  (A clamped box
    is 62.5 x its input size and would hide every other token in a max-norm.)"""
    a, b = a.detach().double().cpu().reshape(-1, 4), b.detach().double().cpu().reshape(-1, 4)
    return float(((a - b).abs().amax(dim=1) / b.abs().amax(dim=1).clamp_min(1e-12)).max())


# ------------------------------------------------------------------------------------------------ the format model
def _rtz16(x):
    """float64 -> the fp16 value toward zero, as float64: 11 significant bits above 2^-14, multiples of 2^-24 below (subnormals kept),
    +-65504 beyond the range."""
    _, e = torch.frexp(x)                                        # |x| in [2^(e-1), 2^e)
    q = torch.ldexp(torch.ones_like(x), (e - 1).clamp(min=-14) - 10)
    return (torch.trunc(x / q) * q).clamp(-65504.0, 65504.0)


def split_rtz16(x):
    """x -> (hi, lo), float64: hi = RTZ_f16(x), lo = RTZ_f16(x - hi) (igemm_dma.hpp: split_pair)."""
    x = x.double()
    hi = _rtz16(x)
    return hi, _rtz16(x - hi)


def x3_product(a, b, low=True):
    """a @ b as the f16x3 contraction forms it: lo.hi + hi.lo + hi.hi, every product and the sum in float64.  ``low=False`` zeroes both
    low halves (the 11-bit mutant)."""
    ah, al = split_rtz16(a)
    bh, bl = split_rtz16(b)
    if not low:
        return ah @ bh
    return al @ bh + ah @ bl + ah @ bh


def x3_hooks(sites, low=True):
    """``linear`` / ``bmm`` hooks of the oracle with the model at ``sites``, plain float64 elsewhere."""
    def linear(x, w, b=None, site=None):
        if site not in sites:
            return F.linear(x, w, b)
        y = x3_product(x, w.t(), low)
        return y if b is None else y + b

    def bmm(a, b, site=None):
        return x3_product(a, b, low) if site in sites else torch.bmm(a, b)
    return dict(linear=linear, bmm=bmm)


# ------------------------------------------------------------------------------------------------ state dicts and inputs
@functools.lru_cache(maxsize=None)
def base_sd():
    return orc.as_torch(synth.make_state_dict(0))


def _scaled(sd, factors):
    out = dict(sd)
    for key, f in factors.items():
        out[key] = sd[key] * f                                  # powers of two: exact
    return out


def rescaled(sd, stage, family, k):
    """A copy of ``sd`` with the family's tensors of decoder stage ``stage`` multiplied by 2^-k (``ffn_hidden``: the first FFN layer by
    2^-k and the second's matrix by 2^k -- the same function in real arithmetic, with a small hidden tensor)."""
    p = f'roi_head.bbox_head.{stage}'
    q = p + '.instance_interactive_conv'
    dn, up = 2.0 ** -k, 2.0 ** k
    keys = {'theta': {q + '.dynamic_layer.weight': dn, q + '.dynamic_layer.bias': dn},
            'fc': {q + '.fc_layer.weight': dn, q + '.fc_layer.bias': dn},
            'towers': {p + '.cls_fcs.0.weight': dn, **{p + f'.reg_fcs.{j}.weight': dn for j in (0, 3, 6)}},
            'ffn_hidden': {p + '.ffn.layers.0.0.weight': dn, p + '.ffn.layers.0.0.bias': dn, p + '.ffn.layers.1.weight': up}}[family]
    return _scaled(sd, keys)


def clamp_sd(sd, stage, factor):
    """Rows 2 and 3 (dw, dh) of every clue's fc_reg weight and bias times ``factor``."""
    out = dict(sd)
    for clue in orc.CLUES:
        for t in ('weight', 'bias'):
            key = f'roi_head.bbox_head.{stage}.{clue}_fc_reg.{t}'
            v = sd[key].clone()
            v[2:4] *= factor
            out[key] = v
    return out


@functools.lru_cache(maxsize=None)
def _case_sd(family, k):
    sd = base_sd()
    for s in STAGES:
        if family == 'clamp':
            sd = clamp_sd(sd, s, k)
        elif family in ('theta', 'fc', 'towers', 'ffn_hidden'):
            sd = rescaled(sd, s, family, k)
    return sd


def case_sd(case):
    """The f32 state dict of a case (both tested stages changed alike; ``roi`` is an input scale, not a state-dict change).  One object
    per (family, k): the GPU file keys its packed weights on it."""
    return _case_sd(case.family if case.family != 'roi' else None, case.k if case.family != 'roi' else 0)


@functools.lru_cache(maxsize=None)
def _sd64(family, k):
    return {key: (v.double() if v.is_floating_point() else v) for key, v in _case_sd(family, k).items()}


def case_sd64(case):
    return _sd64(case.family if case.family != 'roi' else None, case.k if case.family != 'roi' else 0)


@functools.lru_cache(maxsize=None)
def _inputs(N, roi_k):
    """The inputs of test_decoder_stage: roi ~ 3 randn, obj ~ randn, three nested boxes jittered by randn; seed 100 + N."""
    g = torch.Generator().manual_seed(100 + N)
    roi = torch.randn(N * 3, 256, 7, 7, generator=g) * 3
    obj = torch.randn(N, 3, 256, generator=g)
    boxes = torch.tensor([[20., 30., 200., 210.], [60., 50., 160., 150.], [90., 60., 130., 100.]])[None].repeat(N, 1, 1)
    boxes = boxes + torch.randn(N, 3, 4, generator=g)
    return roi * 2.0 ** -roi_k, obj, boxes


def inputs(case):
    """(roi [N*3,256,7,7], obj [N,3,256], boxes [N,3,4]), f32."""
    return _inputs(num_frames(case), case.k if case.family == 'roi' else 0)


# ------------------------------------------------------------------------------------------------ oracle runs
def decode(boxes, delta, stds, clamp='after', max_ratio=MAX_RATIO):
    """delta2bbox (delta_xywh_bbox_coder.py:224-260) with the clamp as a parameter: 'after' the multiplication by the std (the
    reference; equal to oracle.delta2bbox, asserted on the CPU), 'before' it, or None -- the last two are mutants."""
    boxes, d = boxes.reshape(-1, 4), delta.reshape(-1, 4)
    stds = d.new_tensor(stds)
    dwh = d[:, 2:]
    if clamp == 'before':
        dwh = dwh.clamp(-max_ratio, max_ratio)
    dwh = dwh * stds[2:]
    if clamp == 'after':
        dwh = dwh.clamp(-max_ratio, max_ratio)
    pxy, pwh = (boxes[:, :2] + boxes[:, 2:]) * 0.5, boxes[:, 2:] - boxes[:, :2]
    gxy, gwh = pxy + pwh * d[:, :2] * stds[:2], pwh * dwh.exp()
    return torch.cat([gxy - gwh * 0.5, gxy + gwh * 0.5], dim=-1).reshape(-1, 3, 4)


def run_oracle(case, stage, dtype=torch.float64, store=torch.float32, stage_fn=None, hooks=None, decode_kw=None, lengths=None):
    """One stage of the oracle on the case -> dict(obj [N,3,256], cls [N,3], boxes [N,3,4], delta [N,3,4]) in ``dtype``.  ``store``: the
    storage type the inputs are rounded to first (the engine kind's).  Clip by clip, concatenated.  The mutants pass ``stage_fn`` (a
    replacement for oracle.stqi_stage), ``hooks`` (contraction hooks), ``decode_kw`` or other clip ``lengths``."""
    sd = case_sd64(case) if dtype == torch.float64 else case_sd(case)
    roi, obj, boxes = inputs(case)
    roi, obj = roi.to(store).to(dtype), obj.to(store).to(dtype)
    fn = stage_fn or orc.stqi_stage
    outs, f0 = [], 0
    with torch.no_grad():
        for T in (lengths or clip_lengths(case)):
            cls, delta, x = fn(sd, stage, roi[3 * f0:3 * (f0 + T)], obj[f0:f0 + T], T, **(hooks or {}))
            outs.append((x, cls.squeeze(-1), delta))
            f0 += T
    assert f0 == obj.shape[0]
    x, cls, delta = (torch.cat(t) for t in zip(*outs))
    if decode_kw is None:
        bx = orc.delta2bbox(boxes.to(dtype).reshape(-1, 4), delta.reshape(-1, 4), stds=case.stds, clip_border=False).reshape(-1, 3, 4)
    else:
        bx = decode(boxes.to(dtype), delta, case.stds, **decode_kw)
    return dict(obj=x, cls=cls, boxes=bx, delta=delta)


@functools.lru_cache(maxsize=None)
def reference(name, stage, store=torch.float32):
    """The float64 oracle on the case's inputs as the engine kind stores them."""
    return run_oracle(CASES[name], stage, store=store)


def errors(out, ref):
    """scale_err per output, and the per-token box metric."""
    e = {k: scale_err(out[k], ref[k]) for k in OUTS}
    e['boxes_tok'] = token_err(out['boxes'], ref['boxes'])
    return e


@functools.lru_cache(maxsize=None)
def floor(name, stage, store=torch.float32):
    """The f32 CPU oracle against the float64 one, per output (and ``boxes_tok``: the per-token box metric)."""
    return errors(run_oracle(CASES[name], stage, dtype=torch.float32, store=store), reference(name, stage, store))


@functools.lru_cache(maxsize=None)
def model(name, stage, packed=False):
    """The float64 oracle with the format model at the case's stressed sites (``packed``: and at PACK_SITES) against the plain float64
    oracle, per output."""
    case = CASES[name]
    sites = FAMILY_SITES[case.family] + (PACK_SITES.get(case.family, ()) if packed else ())
    return errors(run_oracle(case, stage, hooks=x3_hooks(sites)), reference(name, stage))


def bound(name, stage, kind, packed=False):
    """-> {output: bound} for one engine kind; the keys are the metrics the GPU test asserts ('boxes_tok' replaces 'boxes' in CLAMP).

    BASE, T_EDGE, MAGNITUDE fp32:  STAGE_TOL[kind] + floor.  On the BASE shapes this follows from the test that passes today by the
                                   triangle inequality; T changes the softmax length only, and f32 MFMA has no magnitude dependence.
    MAGNITUDE f16x3:               STAGE_TOL['f16x3'] + floor + MARGIN x model (``packed``: the model with PACK_SITES added).
    CLAMP:                         obj, cls as BASE; boxes per token: MARGIN x floor_tok x STAGE_TOL[kind]['boxes'] / STAGE_TOL['fp32']['boxes']."""
    case = CASES[name]
    fl = floor(name, stage, KIND_DTYPE[kind])
    b = {k: STAGE_TOL[kind][k] + fl[k] for k in OUTS}
    if case.group == 'MAGNITUDE' and kind == 'f16x3':
        m = model(name, stage, packed)
        b = {k: b[k] + MARGIN * m[k] for k in OUTS}
    if case.group == 'CLAMP':
        del b['boxes']
        b['boxes_tok'] = MARGIN * fl['boxes_tok'] * STAGE_TOL[kind]['boxes'] / STAGE_TOL['fp32']['boxes']
    return b


def kinds_of(case):
    """MAGNITUDE is the f16x3 question with fp32 as its control; the 16-bit kinds' storage rounding dominates there."""
    return ('fp32', 'f16x3') if case.group == 'MAGNITUDE' else KINDS


def clamp_counts(case, stage):
    """(above, below, inside) token counts for dw and for dh on the float64 reference."""
    d = reference(case.name, stage)['delta'].reshape(-1, 4)[:, 2:] * torch.tensor(case.stds[2:], dtype=torch.float64)
    return [(int((d[:, j] > MAX_RATIO).sum()), int((d[:, j] < -MAX_RATIO).sum()), int((d[:, j].abs() < MAX_RATIO).sum())) for j in (0, 1)]
