"""CPU: the instrument of tests/test_gpu_decoder.py proved without a GPU (tests/decoder_cases.py).  The oracle's contraction hooks change
no bit by default; the format model holds its hand values; every case satisfies the conditions it claims (clamp counts, subnormal low
halves); the floor / model / bound table is printed; and every bound rejects the subtly wrong decoder stages listed in
test_mutants_are_rejected, each applied to the float64 oracle."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import mcgaze_oracle as orc
from tests import decoder_cases as D


# ------------------------------------------------------------------------------------------------ the hooks
def _stqi_stage_before_hooks(sd, s, roi_feat, obj, clip_length):
    """oracle.stqi_stage / mha_self / dynamic_conv as they stood before they took hooks, in one piece: the statement the hooked functions
    must reproduce bit for bit."""
    _ln = orc._ln

    def mha_self(p, x, num_heads=8):
        L, Bt, d = x.shape
        hd = d // num_heads
        qkv = F.linear(x, sd[p + '.attn.in_proj_weight'], sd[p + '.attn.in_proj_bias'])
        q, k, v = qkv.split(d, dim=-1)
        heads = lambda t: t.reshape(L, Bt * num_heads, hd).transpose(0, 1)
        q, k, v = heads(q) * (1.0 / math.sqrt(hd)), heads(k), heads(v)
        a = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
        o = torch.bmm(a, v).transpose(0, 1).reshape(L, Bt, d)
        return x + F.linear(o, sd[p + '.attn.out_proj.weight'], sd[p + '.attn.out_proj.bias'])

    def dynamic_conv(p, x, roi, feat=64):
        R, d = x.shape
        f = roi.flatten(2).permute(0, 2, 1)
        theta = F.linear(x, sd[p + '.dynamic_layer.weight'], sd[p + '.dynamic_layer.bias'])
        f = F.relu(_ln(sd, p + '.norm_in', torch.bmm(f, theta[:, :d * feat].view(R, d, feat))))
        f = F.relu(_ln(sd, p + '.norm_out', torch.bmm(f, theta[:, -d * feat:].view(R, feat, d))))
        f = F.linear(f.flatten(1), sd[p + '.fc_layer.weight'], sd[p + '.fc_layer.bias'])
        return F.relu(_ln(sd, p + '.fc_norm', f))

    p = f'roi_head.bbox_head.{s}'
    N, P, d = obj.shape
    T = clip_length
    x = obj.permute(1, 0, 2)
    x = _ln(sd, p + '.attention_norm', mha_self(p + '.attention', x)).permute(1, 0, 2)
    x = x.reshape(N // T, T, P, d).permute(1, 0, 2, 3).reshape(T, N * P // T, d)
    x = _ln(sd, p + '.attention_norm', mha_self(p + '.attention', x))
    x = x.reshape(T, N // T, P, d).permute(1, 0, 2, 3).reshape(N, P, d)
    x = x.reshape(-1, d)
    x = _ln(sd, p + '.instance_interactive_conv_norm', x + dynamic_conv(p + '.instance_interactive_conv', x, roi_feat))
    h = F.linear(F.relu(F.linear(x, sd[p + '.ffn.layers.0.0.weight'], sd[p + '.ffn.layers.0.0.bias'])),
                 sd[p + '.ffn.layers.1.weight'], sd[p + '.ffn.layers.1.bias'])
    x = _ln(sd, p + '.ffn_norm', x + h).view(N, P, d)
    cls_f = F.relu(_ln(sd, p + '.cls_fcs.1', F.linear(x, sd[p + '.cls_fcs.0.weight'])))
    reg_f = x
    for j in range(3):
        reg_f = F.relu(_ln(sd, p + f'.reg_fcs.{3 * j + 1}', F.linear(reg_f, sd[p + f'.reg_fcs.{3 * j}.weight'])))
    cls = torch.stack([F.linear(cls_f[:, c], sd[p + f'.{n}_fc_cls.weight'], sd[p + f'.{n}_fc_cls.bias']) for c, n in enumerate(orc.CLUES)], dim=1)
    delta = torch.stack([F.linear(reg_f[:, c], sd[p + f'.{n}_fc_reg.weight'], sd[p + f'.{n}_fc_reg.bias']) for c, n in enumerate(orc.CLUES)], dim=1)
    return cls, delta, x


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_hook_defaults_change_no_bit(dtype):
    case = D.CASES['B2T3']
    sd = D.case_sd(case) if dtype == torch.float32 else D.case_sd64(case)
    roi, obj, _ = D.inputs(case)
    roi, obj = roi.to(dtype), obj.to(dtype)
    with torch.no_grad():
        want = _stqi_stage_before_hooks(sd, 3, roi, obj, 3)
        got = orc.stqi_stage(sd, 3, roi, obj, 3)
        assert got[0].dtype == dtype
        for a, b, name in zip(got, want, ('cls', 'delta', 'obj')):
            assert torch.equal(a, b), name
        # every contraction site is named, in the order the stage runs them
        seen = []
        lin = lambda x, w, b=None, site=None: (seen.append(site), F.linear(x, w, b))[1]
        bmm = lambda a, b, site=None: (seen.append(site), torch.bmm(a, b))[1]
        again = orc.stqi_stage(sd, 3, roi, obj, 3, linear=lin, bmm=bmm)
    assert seen == ['in_proj', 'out_proj'] * 2 + ['dynamic_layer', 'dyn_in', 'dyn_out', 'fc_layer', 'ffn1', 'ffn2', 'cls_fc'] + ['reg_fc'] * 3
    assert set(seen) == set(orc.SITES) - {'gaze_fc0', 'gaze_fc1'}               # the two sites of oracle.gaze_head: tests/test_gaze_cases_cpu.py
    assert all(torch.equal(a, b) for a, b in zip(again, want))


def test_decode_is_the_oracles_delta2bbox():
    g = torch.Generator().manual_seed(5)
    boxes = torch.tensor([[20., 30., 200., 210.]]).repeat(12, 1).double() + torch.randn(12, 4, generator=g).double()
    delta = torch.randn(12, 4, generator=g).double() * 6
    for stds in (D.STDS, (0.5, 0.5, 2.0, 2.0)):
        want = orc.delta2bbox(boxes, delta, stds=stds, clip_border=False)
        assert torch.equal(D.decode(boxes, delta, stds).reshape(-1, 4), want)
    assert abs(D.MAX_RATIO - math.log(1000 / 16)) < 1e-15


# ------------------------------------------------------------------------------------------------ the format model
def test_split_model_hand_values():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    hi, lo = D.split_rtz16(t(2049.0, -2049.0))
    assert hi.tolist() == [2048.0, -2048.0] and lo.tolist() == [1.0, -1.0]
    x = 2.0 ** -3 * (1 + 2.0 ** -12)                            # the low half 2^-15 lies below fp16's smallest normal 2^-14: a subnormal, kept
    hi, lo = D.split_rtz16(t(x))
    assert hi.item() == 2.0 ** -3 and lo.item() == 2.0 ** -15 and lo.item() < 2.0 ** -14
    hi, lo = D.split_rtz16(t(2.0 ** -3 * (1 + 2.0 ** -12 + 2.0 ** -22)))   # ... on the subnormal grid of 2^-24: the 2^-25 is cut
    assert hi.item() == 2.0 ** -3 and lo.item() == 2.0 ** -15
    hi, lo = D.split_rtz16(t(1e5, -1e5, 2e5))
    assert hi.tolist() == [65504.0, -65504.0, 65504.0] and lo.tolist() == [34496.0, -34496.0, 65504.0]
    hi, lo = D.split_rtz16(t(0.0, 2.0 ** -24, 2.0 ** -25, 1 + 2.0 ** -10 + 2.0 ** -11))
    assert hi.tolist() == [0.0, 2.0 ** -24, 0.0, 1 + 2.0 ** -10] and lo.tolist() == [0.0, 0.0, 0.0, 2.0 ** -11]
    # round toward zero, not to nearest: 1 + 2^-11 + 2^-12 stays at 1 in the high half
    hi, lo = D.split_rtz16(t(1 + 2.0 ** -11 + 2.0 ** -12))
    assert hi.item() == 1.0 and lo.item() == 2.0 ** -11 + 2.0 ** -12
    # agrees with torch's fp16 wherever the value is an fp16 number already
    v = torch.randn(4096, generator=torch.Generator().manual_seed(1)).half().double() * 2.0 ** -9
    v = v.half().double()
    hi, lo = D.split_rtz16(v)
    assert torch.equal(hi, v) and not lo.any()


def test_x3_product_keeps_22_bits_and_the_mutant_11():
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(8, 64, generator=g).double(), torch.randn(64, 8, generator=g).double()
    full, mutant, ref = D.x3_product(a, b), D.x3_product(a, b, low=False), a @ b
    assert D.scale_err(full, ref) < 2.0 ** -19 and 2.0 ** -14 < D.scale_err(mutant, ref) < 2.0 ** -8
    a[0, 0], b[0, 0] = 2049.0, 3.0                              # lo.hi + hi.lo + hi.hi: the lo.lo term is the one left out
    ah, al = D.split_rtz16(a)
    bh, bl = D.split_rtz16(b)
    assert torch.equal(D.x3_product(a, b), al @ bh + ah @ bl + ah @ bh)


# ------------------------------------------------------------------------------------------------ the cases
def test_rescaled_touches_what_it_names():
    sd = D.base_sd()
    for fam, n in (('theta', 2), ('fc', 2), ('towers', 4), ('ffn_hidden', 3)):
        out = D.rescaled(sd, 3, fam, 6)
        changed = [k for k in sd if out[k] is not sd[k]]
        assert len(changed) == n and all('bbox_head.3.' in k for k in changed), (fam, changed)
        for k in changed:
            up = fam == 'ffn_hidden' and k.endswith('layers.1.weight')
            assert torch.equal(out[k], sd[k] * (64.0 if up else 1 / 64.0))
    out = D.clamp_sd(sd, 0, 48)
    for clue in orc.CLUES:
        for t in ('weight', 'bias'):
            k = f'roi_head.bbox_head.0.{clue}_fc_reg.{t}'
            assert torch.equal(out[k][:2], sd[k][:2]) and torch.equal(out[k][2:], sd[k][2:] * 48)


def test_groups_are_the_stated_cases():
    assert [c.clips for c in D.BASE] == [(1, 7), (2, 3), (3, 1)]
    assert [c.clips for c in D.T_EDGE] == [(1, 10), (2, 10), (1, 11), (1, 33), [10, 1, 3], [11, 2]]
    assert {(c.family, c.k) for c in D.MAGNITUDE} >= {('theta', 6), ('theta', 10), ('roi', 6), ('roi', 10), ('fc', 6), ('towers', 6), ('ffn_hidden', 6)}
    assert all(c.clips == (1, 7) and 3 * D.num_frames(c) == 21 for c in D.MAGNITUDE + D.CLAMP)
    assert max(3 * D.num_frames(c) for c in D.CASES.values()) <= 99
    assert all(D.kinds_of(c) == ('fp32', 'f16x3') for c in D.MAGNITUDE) and all(tuple(D.kinds_of(c)) == tuple(D.KINDS) for c in D.BASE + D.T_EDGE + D.CLAMP)


def test_clamp_cases_clamp_both_ways_and_not_at_all():
    for case in D.CLAMP:
        for s in D.STAGES:
            counts = D.clamp_counts(case, s)
            print(f'{case.name} stage {s}: (above, below, inside) dw {counts[0]}, dh {counts[1]} of 21 tokens')
            assert all(n >= D.CLAMP_MIN_TOKENS for c in counts for n in c), (case.name, s, counts)
    # the unscaled weights never reach the clamp: what test_decoder_stage cannot see
    assert float(D.reference('B1T7', 0)['delta'][..., 2:].abs().max()) < D.MAX_RATIO / 2


def test_magnitude_cases_reach_the_subnormal_low_halves():
    case = D.CASES['theta_k10']
    sd, (roi, obj, _) = D.case_sd64(case), D.inputs(case)
    for s in D.STAGES:
        seen = {}
        bmm = lambda a, b, site=None: (seen.__setitem__(site, (a, b)), torch.bmm(a, b))[1]
        with torch.no_grad():
            orc.stqi_stage(sd, s, roi.double(), obj.double(), 7, bmm=bmm)
        theta = torch.cat([seen['dyn_in'][1].flatten(), seen['dyn_out'][1].flatten()])
        share = float((theta.abs() < 2.0 ** -3).double().mean())
        _, lo = D.split_rtz16(theta)
        sub = float(((lo != 0) & (lo.abs() < 2.0 ** -14)).double().mean())
        print(f'theta k=10 stage {s}: share of |theta| < 2^-3 = {share:.4f}; low halves that are non-zero subnormals: {sub:.4f}')
        assert share > 0.9
    roi = D.inputs(D.CASES['roi_k10'])[0]
    assert float(roi.abs().max()) < 2.0 ** -3
    assert torch.equal(roi * 1024, D.inputs(D.CASES['B1T7'])[0])      # the power of two changed nothing else


def test_floor_model_bound_table():
    print(f'\n{"case":16s} st kind   ' + ' '.join(f'{"floor " + k:>15s} {"model " + k:>15s} {"bound " + k:>15s}' for k in D.OUTS + ('boxes_tok',)))
    for case in D.CASES.values():
        for s in D.STAGES:
            for kind in D.kinds_of(case):
                fl, b = D.floor(case.name, s, D.KIND_DTYPE[kind]), D.bound(case.name, s, kind)
                m = D.model(case.name, s) if case.group == 'MAGNITUDE' else {}
                f = lambda d, k: f'{d[k]:15.2e}' if k in d else f'{"-":>15s}'
                print(f'{case.name:16s} {s}  {kind:6s} ' + ' '.join(f'{f(fl, k)} {f(m, k)} {f(b, k)}' for k in D.OUTS + ('boxes_tok',)))
                assert all(math.isfinite(v) and v > 0 for v in b.values())
                # a bound is never below what the reference itself can resolve, and never loose by more than MARGIN x the modelled format
                assert all(b[k] >= D.STAGE_TOL[kind][k] for k in b if k in D.STAGE_TOL[kind])
                assert set(b) == ({'obj', 'cls', 'boxes_tok'} if case.group == 'CLAMP' else set(D.OUTS))
    # the f32 reference's own error is a sizeable part of the bounds it was used for: the reason the reference here is float64
    worst = max(D.floor(c.name, s)[k] for c in D.BASE for s in D.STAGES for k in D.OUTS)
    assert 2e-7 < worst < 2e-6


# ------------------------------------------------------------------------------------------------ the mutants
def _swapped_passes(sd, s, roi_feat, obj, T, linear=orc._linear, bmm=orc._bmm):
    p = f'roi_head.bbox_head.{s}'
    x = orc.spatial_attention(sd, p, orc.temporal_attention(sd, p, obj, T, linear, bmm), linear, bmm)
    return orc.stqi_after_attention(sd, p, roi_feat, x, linear, bmm)[:3]


def _eps_1e6_at_norm_in():
    """LayerNorm(c y; eps) = LayerNorm(y; eps / c^2): scaling the dyn_in product by sqrt(10) IS norm_in with eps = 1e-6."""
    return dict(bmm=lambda a, b, site=None: torch.bmm(a, b) * (math.sqrt(10.0) if site == 'dyn_in' else 1.0))


def _mutants():
    m = [(f'11-bit contraction at {"+".join(D.FAMILY_SITES[c.family])}', c.name, ('fp32', 'f16x3'), dict(hooks=D.x3_hooks(D.FAMILY_SITES[c.family], low=False)))
         for c in D.MAGNITUDE]
    m.append(('11-bit contraction at dyn_in', 'B1T7', ('fp32', 'f16x3'), dict(hooks=D.x3_hooks(('dyn_in',), low=False))))
    for c in D.CLAMP:
        m.append(('clamp removed', c.name, D.KINDS, dict(decode_kw=dict(clamp=None))))
        m.append(('max_ratio log(1000/32)', c.name, D.KINDS, dict(decode_kw=dict(max_ratio=math.log(1000 / 32)))))
    m.append(('clamp before the std multiplication', 'clamp_std2', D.KINDS, dict(decode_kw=dict(clamp='before'))))
    m.append(('temporal attention over T = 5 (as 4 clips)', 'B2T10', D.KINDS, dict(lengths=[5, 5, 5, 5])))
    m += [('temporal pass before spatial pass', n, D.KINDS, dict(stage_fn=_swapped_passes)) for n in ('B1T7', 'ragged_10_1_3')]
    m.append(('norm_in eps 1e-6', 'roi_k10', ('fp32', 'f16x3'), dict(hooks=_eps_1e6_at_norm_in())))
    return m


@pytest.mark.parametrize('what,name,kinds,kw', _mutants(), ids=[f'{m[1]}-{m[0].replace(" ", "_")}' for m in _mutants()])
def test_mutants_are_rejected(what, name, kinds, kw):
    """Each mutation is applied to the float64 oracle; its error must exceed the case's bound on at least one asserted output, in both
    stages and for every kind listed.  (The 11-bit mutant is an f16-grade contraction: it is put to the kinds that claim more.)"""
    case = D.CASES[name]
    for s in D.STAGES:
        for kind in kinds:
            store = D.KIND_DTYPE[kind]
            e = D.errors(D.run_oracle(case, s, store=store, **kw), D.reference(name, s, store))
            b = D.bound(name, s, kind)
            over = {k: e[k] / b[k] for k in b}
            print(f'{what:45s} {name:14s} stage {s} {kind:6s} ' + ' '.join(f'{k} {e[k]:.2e} / {b[k]:.2e}' for k in b) +
                  ('   (the format itself is at 11-12 bits here: not told apart)' if (name, kind) in D.MUTANT_BLIND else ''))
            if (name, kind) in D.MUTANT_BLIND:
                assert what.startswith('11-bit') and D.bound(name, s, 'fp32')['obj'] < e['obj']    # the fp32 control's bound still rejects it
                continue
            assert max(over.values()) > 1.0, (what, name, s, kind, e, b)


def test_unscaled_packing_explains_the_cases_over_their_bound():
    """theta and ffn_hidden scale a weight matrix whose own contraction the stated sites leave out, and the decoder's matrices are packed
    without a pre-scale: with that site in the model, the FORMAT is over the stated f16x3 bound on some output in both stages (the GPU
    file's strict xfails), and the other families' scaled matrices are stated sites already."""
    assert {f for f in D.FAMILY_SITES if f not in D.PACK_SITES} == {'roi', 'fc', 'towers'}
    for name in ('theta_k6', 'theta_k10', 'ffn_hidden_k6'):
        for s in D.STAGES:
            m, mp, b, bp = D.model(name, s), D.model(name, s, packed=True), D.bound(name, s, 'f16x3'), D.bound(name, s, 'f16x3', packed=True)
            print(f'{name} stage {s}: ' + ', '.join(f'{k} model {m[k]:.2e} -> as packed {mp[k]:.2e} (stated bound {b[k]:.2e}, as packed {bp[k]:.2e})' for k in D.OUTS))
            assert any(mp[k] > b[k] for k in D.OUTS), (name, s)
            assert all(mp[k] < bp[k] for k in D.OUTS)
            # the 11-bit mutant at the data-on-both-sides products is still rejected by the as-packed bound wherever the packing leaves room
            # (theta k = 10 packs dynamic_layer.weight at 10 - 11 bits: there the format and the mutant coincide)
            if name != 'theta_k10':
                e = D.errors(D.run_oracle(D.CASES[name], s, hooks=D.x3_hooks(D.FAMILY_SITES[D.CASES[name].family], low=False)), D.reference(name, s))
                assert any(e[k] > bp[k] for k in D.OUTS), (name, s, e, bp)


def test_identity_passes_every_bound():
    """The instrument does not reject the reference itself, nor the format model where a model is part of the bound."""
    for case in D.CASES.values():
        for s in D.STAGES:
            for kind in D.kinds_of(case):
                b = D.bound(case.name, s, kind)
                fl = D.floor(case.name, s, D.KIND_DTYPE[kind])
                assert all(fl[k] < b[k] for k in b), (case.name, s, kind)
                if case.group == 'MAGNITUDE' and kind == 'f16x3':
                    m = D.model(case.name, s)
                    assert all(m[k] < b[k] for k in b if k in m), (case.name, s)
