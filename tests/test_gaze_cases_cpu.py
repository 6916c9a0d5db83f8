"""CPU: the instrument of tests/test_gpu_gaze_head.py proved without a GPU (tests/gaze_cases.py).  The oracle's gaze head changes no bit
by default and runs in float64; the float64 reference and the f32 oracle agree to ``floor``; the N_EDGE rows are BASE rows; the cases
satisfy what they claim (variance below the LayerNorm epsilon at k = 10); the floor / model / bound table and the worst-conditioned frame
of every case are printed; and every bound rejects the subtly wrong gaze heads of test_order_one_mutants_are_rejected and
test_format_and_epsilon_mutants_are_rejected, each a float64 variant of the oracle."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import mcgaze_oracle as orc
from tests import gaze_cases as G


# ------------------------------------------------------------------------------------------------ the oracle
def _gaze_head_before_hooks(sd, s, obj):
    """oracle.gaze_head as it stood before it took ``linear`` and ``return_raw``: what the default must reproduce bit for bit."""
    g = f'roi_head.gaze_head.{s}'

    def mlp(branch, x):
        for j in range(2):
            x = F.relu(orc._ln(sd, g + f'.{branch}.{3 * j + 1}', F.linear(x, sd[g + f'.{branch}.{3 * j}.weight'])))
        return x

    gz, conf = [], []
    for c, n in enumerate(orc.CLUES):
        f = obj[:, c, :]
        gz.append(F.linear(mlp(f'gaze_{n}_fcs', f), sd[g + f'.fc_{n}.weight'], sd[g + f'.fc_{n}.bias']))
        conf.append(F.linear(mlp(f'gaze_{n}_confidence', f), sd[g + f'.fc_{n}_confidence.weight'], sd[g + f'.fc_{n}_confidence.bias']))
    fused = F.linear(torch.cat([c * z for c, z in zip(conf, gz)], dim=1), sd[g + '.fc_gaze.weight'], sd[g + '.fc_gaze.bias'])
    unit = lambda t: t / torch.norm(t, dim=-1, keepdim=True)
    return dict(gaze_score=unit(fused), face_gaze_score=unit(gz[0]), eyes_gaze_score=unit(gz[1]), head_gaze_score=unit(gz[2]))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_hook_defaults_change_no_bit(dtype):
    case = G.CASES['N9']
    sd = G.case_sd(case) if dtype == torch.float32 else G.case_sd64(case)
    obj = G.inputs(case).to(dtype)
    with torch.no_grad():
        want = _gaze_head_before_hooks(sd, G.STAGE, obj)
        got = orc.gaze_head(sd, G.STAGE, obj)
        assert set(got) == set(G.OUTS) and all(got[k].dtype == dtype and torch.equal(got[k], want[k]) for k in G.OUTS)
        seen = []
        lin = lambda x, w, b=None, site=None: (seen.append(site), F.linear(x, w, b))[1]
        again, r = orc.gaze_head(sd, G.STAGE, obj, linear=lin, return_raw=True)
    # both MLP layers of all six branches are named; nothing else is
    assert seen == ['gaze_fc0', 'gaze_fc1'] * 6 and set(seen) == set(G.SITES) and set(G.SITES) <= set(orc.SITES)
    assert all(torch.equal(again[k], want[k]) for k in G.OUTS)
    # the raw vectors are the ones the unit vectors come from, and the confidences the ones the fusion used
    assert r['fused'].dtype == dtype and len(r['gaze']) == 3 and len(r['conf']) == 3
    for k, v in zip(G.OUTS, [r['fused']] + r['gaze']):
        assert torch.equal(v / torch.norm(v, dim=-1, keepdim=True), want[k])
    cat = torch.cat([c * z for c, z in zip(r['conf'], r['gaze'])], dim=1)
    g = f'roi_head.gaze_head.{G.STAGE}'
    assert torch.equal(F.linear(cat, sd[g + '.fc_gaze.weight'], sd[g + '.fc_gaze.bias']), r['fused'])


def test_reference_is_float64_and_the_f32_oracle_within_floor():
    for case in G.CASES.values():
        ref = G.reference(case.name)
        assert ref.dtype == torch.float64 and tuple(ref.shape) == (4, case.N, 3)
        assert float((ref.norm(dim=-1) - 1).abs().max()) < 1e-15
        if case.group == 'N_EDGE':
            continue
        f32 = orc.gaze_head(G.case_sd(case), G.STAGE, G.inputs(case))
        fl = G.floor(case.name)
        assert all(f32[k].dtype == torch.float32 for k in G.OUTS)
        assert G.errors(G.stack(f32), ref) == fl                                 # ``floor`` is this distance
        # f32-sized (2^-24 over raw norms down to 0.03; the figure moves with the host BLAS's summation order), and not zero: the reference is
        # not the f32 run in disguise
        assert all(1e-8 < v < 5e-6 for v in fl.values()), (case.name, fl)
    fl = G.floor('N9')
    print('floor, BASE: ' + ', '.join(f'{k} {v:.2e}' for k, v in fl.items()))
    assert max(fl.values()) > 0.05 * G.GAZE_TOL['fp32']                          # a sizeable part of the bound it was the reference for


def test_n_edge_rows_are_base_rows():
    assert G.EDGE_NS == (1, 127, 128, 129, 255, 256, 257) and [c.N for c in G.N_EDGE] == list(G.EDGE_NS)
    assert all(math.gcd(G.BASE_N, h) == 1 for h in (128, 256))
    # one below, at and above the tile height and twice the tile height
    assert {G.TILE_ROWS + d for d in (-1, 0, 1)} | {2 * G.TILE_ROWS + d for d in (-1, 0, 1)} | {1} == set(G.EDGE_NS)
    base_in, base_ref = G.inputs(G.CASES['N9']), G.reference('N9')
    for case in G.N_EDGE:
        obj, rows = G.inputs(case), G.rows_of(case)
        assert tuple(obj.shape) == (case.N, 3, 256) and torch.equal(obj, base_in[rows])
        assert torch.equal(G.reference(case.name), base_ref[:, rows])
        direct = G.run_oracle(case)                                              # the oracle on all N rows: frames are independent
        assert float((direct - G.reference(case.name)).abs().max()) < 1e-13
        assert G.bound(case.name, 'f16x3') == G.bound('N9', 'f16x3')
        # a shift by one tile does not map the expected rows onto themselves
        if case.N > G.TILE_ROWS:
            assert not torch.equal(rows[G.TILE_ROWS:], rows[:case.N - G.TILE_ROWS])


def test_cases_touch_what_they_name():
    sd = G.base_sd()
    assert len(G.family_keys('mlp')) == 12 and len(G.family_keys('fuse')) == 2 and len(G.family_keys('clue')) == 6
    for case in G.MAGNITUDE + G.SCALE:
        out = G.case_sd(case)
        changed = sorted(k for k in sd if out[k] is not sd[k])
        assert changed == sorted(G.family_keys(case.family)), case.name
        assert all(torch.equal(out[k] * 2.0 ** case.k, sd[k]) for k in changed)  # the power of two changed nothing else, nothing underflowed
    for k in (6, 10):
        assert torch.equal(G.inputs(G.CASES[f'obj_k{k}']) * 2.0 ** k, G.base_obj())
    assert G.case_sd(G.CASES['obj_k6']) is sd and G.case_sd(G.CASES['N257']) is sd
    assert [(c.family, c.k) for c in G.MAGNITUDE] == [('mlp', 6), ('mlp', 10), ('obj', 6), ('obj', 10)]
    assert all(G.kinds_of(c) == ('fp32', 'f16x3') for c in G.MAGNITUDE) and all(G.kinds_of(c) == tuple(G.KINDS) for c in G.BASE + G.N_EDGE + G.SCALE)
    assert max(c.N for c in G.CASES.values()) == 257


def test_k10_puts_the_variance_below_the_layernorm_epsilon():
    """... in both layers of the mlp family and in the first of the obj family, and k = 6 does not: the epsilon's placement shows at k = 10."""
    def variances(case):
        seen = []
        lin = lambda x, w, b=None, site=None: (seen.append((site, F.linear(x, w, b))), seen[-1][1])[1]
        with torch.no_grad():
            orc.gaze_head(G.case_sd64(case), G.STAGE, G.inputs(case).double(), linear=lin)
        return {s: max(float(y.var(dim=-1, unbiased=False).max()) for t, y in seen if t == s) for s in G.SITES}
    for name in ('N9', 'mlp_k6', 'mlp_k10', 'obj_k6', 'obj_k10'):
        v = variances(G.CASES[name])
        print(f'{name}: largest pre-LayerNorm variance, layer 0 {v["gaze_fc0"]:.2e}, layer 1 {v["gaze_fc1"]:.2e}')
    v = variances(G.CASES['mlp_k10'])
    assert v['gaze_fc0'] < 1e-5 and v['gaze_fc1'] < 1e-5
    assert variances(G.CASES['obj_k10'])['gaze_fc0'] < 1e-5
    assert min(variances(G.CASES['mlp_k6']).values()) > 1e-5 * 10


def test_floor_model_bound_table():
    print(f'\n{"case":10s} kind   ' + ' '.join(f'{"floor " + k[:4]:>11s} {"model " + k[:4]:>11s} {"bound " + k[:4]:>11s}' for k in G.OUTS))
    for case in G.CASES.values():
        for kind in G.kinds_of(case):
            fl, b = G.floor(case.name, G.KIND_DTYPE[kind]), G.bound(case.name, kind)
            m = G.model(case.name) if case.group == 'MAGNITUDE' else {}
            f = lambda d, k: f'{d[k]:11.2e}' if k in d else f'{"-":>11s}'
            print(f'{case.name:10s} {kind:6s} ' + ' '.join(f'{f(fl, k)} {f(m, k)} {f(b, k)}' for k in G.OUTS))
            assert set(b) == set(G.OUTS) and all(math.isfinite(v) and v >= G.GAZE_TOL[kind] for v in b.values())
            # the identity passes: neither the f32 oracle nor, where it is part of the bound, the format model is rejected
            assert all(fl[k] < b[k] for k in G.OUTS)
            if case.group == 'MAGNITUDE':
                assert all(m[k] < G.bound(case.name, 'f16x3')[k] for k in G.OUTS)
                if kind == 'fp32':                                               # the control carries no model term
                    assert all(b[k] == G.GAZE_TOL['fp32'] + fl[k] for k in G.OUTS)


def test_worst_conditioned_frames():
    """Per case: the smallest raw norm (the tail divides by it without an epsilon) and the angle the floor's worst row corresponds to."""
    for case in G.BASE + G.MAGNITUDE + G.SCALE:
        v, _ = G.raw(case.name)
        nrm = v.norm(dim=-1)                                                     # [4, N]
        slot, row = divmod(int(nrm.argmin()), case.N)
        f32, ref = G.run_oracle(case, dtype=torch.float32).double(), G.reference(case.name)
        chord = (f32 - ref).norm(dim=-1)                                         # both are unit vectors
        ws, wr = divmod(int(chord.argmax()), case.N)
        print(f'{case.name:10s} smallest raw norm {float(nrm.min()):.3e} ({G.OUTS[slot]}, frame {row}), largest {float(nrm.max()):.3e}; '
              f'floor {max(G.floor(case.name).values()):.2e} = {2 * math.asin(float(chord.max()) / 2):.2e} rad at {G.OUTS[ws]}, frame {wr} (raw norm {float(nrm[ws, wr]):.3e})')
        assert float(nrm.min()) > 0 and math.isfinite(float(nrm.max()))
    nrm = G.raw('N9')[0][1:].norm(dim=-1)
    assert 0.1 < float(nrm.min()) < 0.3 and 2 < float(nrm.max()) < 4             # the per-clue norms span more than a decade on nine frames
    # a power of two on the output layers moves the raw norms and nothing else
    assert torch.allclose(G.raw('fuse_k40')[0][0] * 2.0 ** 40, G.raw('N9')[0][0], rtol=1e-14, atol=0)
    assert torch.allclose(G.raw('clue_k20')[0][1:] * 2.0 ** 20, G.raw('N9')[0][1:], rtol=1e-14, atol=0)


def test_scale_changes_no_bit_of_the_f32_oracle():
    """What the GPU file asserts of the kernel holds for the f32 CPU oracle: fc_gaze x 2^-k leaves the fused unit vectors, and
    fc_{clue} x 2^-k the per-clue ones, bit for bit."""
    base = G.run_oracle(G.CASES['N9'], dtype=torch.float32)
    for name in ('fuse_k20', 'fuse_k40'):
        assert torch.equal(G.run_oracle(G.CASES[name], dtype=torch.float32), base), name
    clue = G.run_oracle(G.CASES['clue_k20'], dtype=torch.float32)
    assert torch.equal(clue[1:], base[1:]) and not torch.equal(clue[0], base[0])  # the fused vector of clue_k20 is another function: bias + 2^-20 x ...


# ------------------------------------------------------------------------------------------------ the mutants
def _ln_eps(eps_inside=1e-5, eps_outside=0.0):
    def ln(x, g, b):
        d = x - x.mean(dim=-1, keepdim=True)
        return d / ((d * d).mean(dim=-1, keepdim=True) + eps_inside).sqrt().add(eps_outside) * g + b
    return ln


def _variant(clue_shift=0, swap_sets=False, ln_last_row_next=False, no_conf=False, k_major=False, ln=None):
    """A float64 restatement of the gaze head in the kernel's own terms -- six branches (branch = 3 k + clue, k = 0 gaze, 1 confidence),
    two layers of matrix, LayerNorm and ReLU per branch, the per-clue heads, the fusion, the normalisation -- with one thing wrong:
      clue_shift        branch (k, clue) reads token (clue + shift) % 3                            (a wrong x_g_period)
      swap_sets         the gaze branches contract with the confidence branches' matrices and back  (a wrong weight group)
      ln_last_row_next  the last row of each branch is normalised with the next branch's parameters (rows_per_group off by one)
      no_conf           cat = gaze, not confidence x gaze
      k_major           cat[3 k + clue] where fc_gaze expects cat[3 clue + k]
      ln                another LayerNorm(x, gamma, beta)"""
    ln = ln or _ln_eps()

    def fn(sd, s, obj, linear=orc._linear):
        g = f'roi_head.gaze_head.{s}'
        names = [f'gaze_{n}_fcs' for n in orc.CLUES] + [f'gaze_{n}_confidence' for n in orc.CLUES]
        heads = [f'fc_{n}' for n in orc.CLUES] + [f'fc_{n}_confidence' for n in orc.CLUES]
        o = []
        for br in range(6):
            x = obj[:, (br % 3 + clue_shift) % 3, :]
            for j in range(2):
                w = sd[g + f'.{names[(br + 3) % 6 if swap_sets else br]}.{3 * j}.weight']
                y = linear(x, w, None, f'gaze_fc{j}')
                p = g + f'.{names[br]}.{3 * j + 1}'
                x = ln(y, sd[p + '.weight'], sd[p + '.bias'])
                if ln_last_row_next:
                    p = g + f'.{names[(br + 1) % 6]}.{3 * j + 1}'
                    x = torch.cat([x[:-1], ln(y[-1:], sd[p + '.weight'], sd[p + '.bias'])])
                x = F.relu(x)
            o.append(F.linear(x, sd[g + f'.{heads[br]}.weight'], sd[g + f'.{heads[br]}.bias']))
        cat = torch.stack([o[c] if no_conf else o[3 + c] * o[c] for c in range(3)], dim=1)          # [N, clue, k]
        cat = (cat.transpose(1, 2) if k_major else cat).reshape(-1, 9)
        fused = F.linear(cat, sd[g + '.fc_gaze.weight'], sd[g + '.fc_gaze.bias'])
        unit = lambda t: t / torch.norm(t, dim=-1, keepdim=True)
        return dict(zip(G.OUTS, (unit(fused), unit(o[0]), unit(o[1]), unit(o[2]))))
    return fn


def test_the_variant_without_a_mutation_is_the_oracle():
    for name in ('N9', 'mlp_k10', 'clue_k20'):
        case = G.CASES[name]
        assert float((G.run_oracle(case, fn=_variant()) - G.reference(name)).abs().max()) < 1e-14
    # ... and its LayerNorm with the epsilon elsewhere is another function only where the variance is small
    for ln in (_ln_eps(0.0), _ln_eps(0.0, 1e-5)):
        assert float((G.run_oracle(G.CASES['N9'], fn=_variant(ln=ln)) - G.reference('N9')).abs().max()) < 1e-4


ORDER_ONE = [('branch g reads clue (g + 1) % 3', dict(clue_shift=1)),
             ('gaze and confidence matrices swapped', dict(swap_sets=True)),
             ('last row of each group under the next branch\'s LN parameters', dict(ln_last_row_next=True)),
             ('fusion without the confidence product', dict(no_conf=True)),
             ('fusion with cat in k-major order', dict(k_major=True))]
EDGE_OVER_ONE_TILE = [c for c in G.N_EDGE if c.N > G.TILE_ROWS]


@pytest.mark.parametrize('what,kw', ORDER_ONE, ids=[m[0].replace(' ', '_') for m in ORDER_ONE])
def test_order_one_mutants_are_rejected(what, kw):
    """Mutants 1 - 5, applied to the float64 oracle on all N rows: over the bound in every kind on every N_EDGE case above one tile (and on
    BASE).  The rows_per_group mutant touches ONE row in N -- the metric is a per-row maximum, not a mean."""
    assert len(EDGE_OVER_ONE_TILE) >= 4
    for case in G.BASE + EDGE_OVER_ONE_TILE:
        for kind in G.KINDS:
            store = G.KIND_DTYPE[kind]
            ref = G.reference(case.name, store)
            out = G.run_oracle(case, store=store, fn=_variant(**kw))
            e, b = G.errors(out, ref), G.bound(case.name, kind)
            rows = int((G.row_err(out, ref) > torch.tensor([b[k] for k in G.OUTS])[:, None]).any(dim=0).sum())
            print(f'{what:62s} {case.name:5s} {kind:6s} ' + ' '.join(f'{k[:4]} {e[k]:.2e} / {b[k]:.2e}' for k in G.OUTS) + f'   rows over: {rows} of {case.N}')
            assert max(e[k] / b[k] for k in G.OUTS) > 1.0, (what, case.name, kind, e, b)
            if 'ln_last_row_next' in kw:
                assert rows == 1


def _format_mutants():
    m = [('11-bit contraction at gaze_fc0+gaze_fc1', c.name, dict(linear=G.x3_hooks(G.SITES, low=False)['linear'])) for c in G.MAGNITUDE]
    m.append(('LayerNorm without its epsilon', 'mlp_k10', dict(fn=_variant(ln=_ln_eps(0.0)))))
    m.append(('LayerNorm with the epsilon outside the square root', 'mlp_k10', dict(fn=_variant(ln=_ln_eps(0.0, 1e-5)))))
    return m


@pytest.mark.parametrize('what,name,kw', _format_mutants(), ids=[f'{m[1]}-{m[0].replace(" ", "_")}' for m in _format_mutants()])
def test_format_and_epsilon_mutants_are_rejected(what, name, kw):
    """Mutants 6 - 8 against fp32 and f16x3 (the 11-bit mutant is an f16-grade contraction: it is put to the kinds that claim more)."""
    case = G.CASES[name]
    for kind in ('fp32', 'f16x3'):
        e, b = G.errors(G.run_oracle(case, **kw), G.reference(name)), G.bound(name, kind)
        blind = (name, kind) in G.MUTANT_BLIND and what.startswith('11-bit')
        print(f'{what:52s} {name:8s} {kind:6s} ' + ' '.join(f'{k[:4]} {e[k]:.2e} / {b[k]:.2e}' for k in G.OUTS) +
              ('   (the format itself is at 12 - 13 bits here: not told apart)' if blind else ''))
        if blind:
            assert max(e[k] / G.bound(name, 'fp32')[k] for k in G.OUTS) > 1.0   # the fp32 control's bound still rejects it
            continue
        assert max(e[k] / b[k] for k in G.OUTS) > 1.0, (what, name, kind, e, b)


def test_mutant_blind_stays_within_its_cap():
    fam = [G.CASES[n].family for n, _ in G.MUTANT_BLIND]
    assert len(fam) == len(set(fam))                                             # at most one entry per family
    for n, kind in G.MUTANT_BLIND:
        c = G.CASES[n]
        assert c.group == 'MAGNITUDE' and kind == 'f16x3' and c.k > min(o.k for o in G.MAGNITUDE if o.family == c.family)   # never the smaller k
        # and the entry is needed: the bound does sit above the mutant
        e = G.model(n, low=False)
        assert all(e[k] <= G.bound(n, kind)[k] for k in G.OUTS), n
