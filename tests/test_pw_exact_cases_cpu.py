"""CPU: the instrument of tests/test_gpu_pw_exact.py proved without a GPU (tests/pw_exact_cases.py).  The case tables name exactly what the
launchers dispatch; every case satisfies the exactness condition; the weight packing is exact on the cases' weights; the upsample reference
is torch's rule on every size pair used; the scaled cases hold rounding ties (16-bit) and non-zero fp16 low halves (f16x3); and the bit
comparison rejects each subtly wrong kernel listed in MUTANTS, every mutation applied to the reference."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_cases as X
from tests import pw_exact_cases as P

KINDS = ('bf16', 'fp16', 'f16x3')


def test_case_tables_are_the_launch_tables():
    """Parses nothing: the literal lists below are read against launch_pw_single_f, launch_pw_single_x3, launch_pw_single_x3_blocks,
    launch_pw_pair_f, launch_pw_dyn and launch_pw_dyn_x3; the tables of the cases module must say the same."""
    assert sorted(P.STREAM16_FORMS.items()) == sorted({
        (512, 128, 0): (32, 1, 0, 1), (512, 256, 0): (32, 1, 0, 2), (512, 256, 2): (32, 1, 2, 2),
        (256, 256, 0): (16, 2, 0, 1), (256, 256, 1): (16, 2, 1, 1), (256, 256, 2): (16, 2, 2, 1),
        (256, 1024, 0): (16, 2, 0, 4), (256, 1024, 1): (16, 2, 1, 4), (256, 1024, 2): (16, 2, 2, 4),
        (128, 512, 0): (8, 4, 0, 1), (128, 512, 1): (8, 4, 1, 1), (128, 512, 2): (8, 4, 2, 1)}.items())
    assert sorted(P.STREAM_X3_FORMS.items()) == sorted({(256, 256, r): (16, r, 2) for r in range(3)}.items()) + sorted({(256, 1024, r): (16, r, 8) for r in range(3)}.items())
    assert P.LIST_FORM == {(256, 256, 2): (16, 2)}
    assert P.PAIR_FORMS == {(0, 64): (1, 1), (0, 128): (1, 2), (64, 64): (2, 1), (64, 128): (2, 2)}
    assert P.DYN_FORMS == {'bf16': (16, 2, 0, 128), 'fp16': (16, 2, 0, 128), 'f16x3': (16, 0, 256)} and (P.DYN_K, P.DYN_N) == (256, 32768)
    # 2 formats x (12 + 1 dynamic_layer) pw_single_kernel + 6 + 1 pw_single_x3_kernel + 1 list form = 34; 2 x 4 pw_pair_kernel = 8
    n_single = 2 * (len(P.STREAM16_FORMS) + 1) + len(P.STREAM_X3_FORMS) + 1 + len(P.LIST_FORM)
    assert (n_single, 2 * len(P.PAIR_FORMS)) == (34, 8)
    # the template arguments are consistent with the shapes: K = 16 KS, N = 128 TPW NSPLIT (f16x3: 128 NSPLIT), RES = res_mode
    for (K, N, r), (ks, tpw, res, nsplit) in P.STREAM16_FORMS.items():
        assert (16 * ks, 128 * tpw * nsplit, res) == (K, N, r)
    for (K, N, r), (ks, res, nsplit) in P.STREAM_X3_FORMS.items():
        assert (16 * ks, 128 * nsplit, res) == (K, N, r)
    assert 128 * 2 * 128 == P.DYN_N == 128 * 256


def test_row_counts_reach_what_they_claim():
    """The tile arithmetic behind DENSE_M, UP_SHAPES, PAIR_M and the list: tiles, the last tile's rows, trips per walker under a cap of one
    group (8 walkers per slice)."""
    trips = lambda tiles, walkers: [len(range(w, tiles, walkers)) for w in range(walkers)]
    assert P.DENSE_M == (1, 31, 32, 33, 753) and P.M_MAX == 753
    assert (753 + 31) // 32 == 24 and 753 - 23 * 32 == 17 and trips(24, 8) == [3] * 8
    assert trips((33 + 31) // 32, 8) == [1, 1] + [0] * 6
    (f, ho, wo), (hr, wr) = P.UP_SHAPES[0]
    assert f * ho * wo == 690 and (690 + 31) // 32 == 22 and max(trips(22, 8)) == 3 and (f, hr, wr) == (3, 2, 14)
    assert [m for m, _ in P.PAIR_M] == [1, 63, 64, 65, 177, 369, 369]
    assert trips((177 + 63) // 64, 1) == [3] and trips((369 + 63) // 64, 2) == [3, 3] and 369 - 5 * 64 == 49
    (f, ho, wo), (hr, wr) = P.LIST_MAP
    assert f * (ho // 8) * (wo // 8) == P.LIST_NBLK == 18 and (ho, wo) == (2 * hr, 2 * wr)
    part = P.LISTS['partial']
    assert len(part) == 13 and len(set(part)) == 13 and sum(0 <= b < 18 for b in part) == 11 and -1 in part and max(part) >= P.LIST_NBLK
    assert sorted(P.LISTS['full']) == list(range(18)) and list(P.LISTS['full']) != list(range(18)) and P.LISTS['empty'] == ()
    assert max(trips(2 * 18, 8)) == 5 and max(trips(2 * 13, 8)) == 4
    assert int(P.listed_pixels(part).sum()) == 11 * 64 and int(P.listed_pixels(P.LISTS['full']).sum()) == 18 * 64
    assert [m for m, _ in P.DYN_M] == [17, 17, 273, 273] and (273 + 31) // 32 == 9
    assert P.SENTINEL != round(P.SENTINEL) and torch.tensor(P.SENTINEL).to(torch.bfloat16).item() == P.SENTINEL


def test_upsample_reference_is_torchs_rule():
    """nearest_index against F.interpolate(mode='nearest') on f32 for every (out, in) pair a case gathers with; where the integer rule
    differs: 46 from 14 at index 23 (torch reads 6), and nowhere on the 'up' case's 9 x 11 from 4 x 5."""
    assert {(46, 14), (5, 2), (9, 4), (11, 5), (16, 8), (24, 12)} <= set(P.SIZE_PAIRS)
    for out, inn in P.SIZE_PAIRS:
        src = torch.arange(inn, dtype=torch.float32)
        assert torch.equal(X.nearest_index(out, inn), F.interpolate(src[None, None, None, :], size=(1, out), mode='nearest')[0, 0, 0].long()), (out, inn)
        assert torch.equal(X.nearest_index(out, inn), F.interpolate(src[None, None, :, None], size=(out, 1), mode='nearest')[0, 0, :, 0].long()), (out, inn)
    differ = {(o, i): (X.nearest_index(o, i) != X.nearest_index_integer(o, i)).nonzero().flatten().tolist() for o, i in P.SIZE_PAIRS}
    assert differ == {pair: ([23] if pair == (46, 14) else []) for pair in P.SIZE_PAIRS}
    assert int(X.nearest_index(46, 14)[23]) == 6 and int(X.nearest_index_integer(46, 14)[23]) == 7
    kw, ref = X.conv_case('up')                           # the existing case: 9 x 11 from 4 x 5 agrees under both rules, and with F.interpolate
    r = kw['res']
    assert tuple(r.shape[2:]) == (4, 5) and tuple(ref.shape[1:3]) == (9, 11)
    assert torch.equal(X.upsample_nearest(r, (9, 11)), X.upsample_nearest(r, (9, 11), index=X.nearest_index_integer))
    assert torch.equal(X.upsample_nearest(r, (9, 11)), F.interpolate(r.float(), size=(9, 11), mode='nearest').long())
    for i, ((f, ho, wo), _) in enumerate(P.UP_SHAPES):
        r = P.stream_inputs(256, 256)['up'][i]
        assert torch.equal(X.upsample_nearest(r, (ho, wo)), F.interpolate(r.float(), size=(ho, wo), mode='nearest').long())


def _scaled_runs(kind):
    return [(K, N, r, P.M_MAX, None, True, P.SCALE[kind]) for K, N, r in P.SCALED_STREAM[kind]]


def _all_stream_cases(kind):
    for K, N, r in P.stream_forms(kind):
        for M, up, _ in P.stream_runs(r):
            for relu in (False, True):
                yield (K, N, r, M, up, relu, 1)
    yield from _scaled_runs(kind)


def test_every_case_satisfies_the_exactness_condition():
    worst = {}
    for kind in KINDS:
        for case in set(_all_stream_cases(kind)):
            K, N, r, M, up, relu, scale = case
            kw = P.stream_kwargs(K, N, r, M, up, relu, scale)
            worst[('stream', kind) + case] = X.check_exactness(X.conv2d_ref, f'stream {case}', x3=kind == 'f16x3', **kw)
            if kind == 'fp16':
                assert int(P.stream_ref(*case).abs().max()) <= 65504
        for scale in (1, P.SCALE[kind]):
            ref, bound = P.dyn_ref(scale)
            assert bound < X.LIMIT and int(P.dyn_inputs(scale)['a'].abs().max()) < X.X3_LIMIT
            assert kind != 'fp16' or int(ref.abs().max()) <= 65504
            worst[('dyn', kind, scale)] = bound
    worst['list'] = X.check_exactness(X.conv2d_ref, 'list form', x3=True, **P.list_inputs())
    for kind in P.KINDS16:
        for (K2, C2) in P.PAIR_FORMS:
            for scale in (1, P.PAIR_SCALE[kind][K2]):
                for with_res in ((True, False) if K2 == 0 else (False,)):
                    kw = P.pair_args(K2, C2, P.PAIR_M_MAX, scale, with_res)
                    worst[('pair', kind, K2, C2, scale, with_res)] = P.check_pair_exactness(kw, f'pair {K2} {C2} x{scale}')
                    y, ys, z = P.pair_ref(**kw, dtype=X.TORCH_DT[kind])
                    X.expected(ys, X.TORCH_DT[kind]), X.expected(z, X.TORCH_DT[kind])      # asserts the fp16 range
    top = max(worst, key=worst.get)
    print(f'largest sum of absolute values over {len(worst)} cases: {worst[top]} ({top}); the limit is 2^24 = {X.LIMIT}')
    assert worst[top] < X.LIMIT


def test_packing_is_exact_on_the_case_weights():
    """engine.pointwise_weights: frag_major holds every ternary weight at the documented place in both 16-bit formats; frag_major_split after
    pow2_prescale holds w * 2^14 in the high halves, empty low halves, and the descale factor 2^-14."""
    from mcgaze_amd.engine import pointwise_weights
    mats = [P.stream_inputs(K, N)['w'] for K, N in {(k, n) for k, n, _ in P.STREAM16_FORMS}] + [P.pair_inputs(64, 128)['w3'], P.pair_inputs(0, 64)['w1']]
    lane, e = torch.arange(64), torch.arange(8)
    for w in mats + [P.dyn_inputs()['w'][:512].long()]:
        n, k = w.shape
        rows = (32 * torch.arange(n // 32)[:, None, None, None] + (lane & 31)[None, None, :, None]).expand(n // 32, k // 16, 64, 8)
        cols = (16 * torch.arange(k // 16)[None, :, None, None] + 8 * (lane >> 5)[None, None, :, None] + e[None, None, None, :]).expand(n // 32, k // 16, 64, 8)
        want = w[rows, cols].double()
        for dt in (torch.bfloat16, torch.float16):
            wf, wscale = pointwise_weights(w.float(), dt, device='cpu')
            assert wf.dtype == dt and wscale == 0.0 and torch.equal(wf.reshape(n // 32, k // 16, 64, 8).double(), want)
        if k == 256:
            wf, wscale = pointwise_weights(w.float(), torch.float32, split=True, device='cpu')
            v = wf.reshape(n // 32, k // 16, 2, 64, 8).double()
            assert wf.dtype == torch.float16 and wscale == 2.0 ** -14
            assert torch.equal(v[:, :, 0], want * 2 ** 14) and float(v[:, :, 1].abs().max()) == 0.0


def test_scaled_cases_hold_ties_and_low_halves():
    """>= 100 reference outputs exactly halfway between two representable values per 16-bit format in every scaled case (stream, pair y and
    z, dynamic_layer); for f16x3 the x 683 activations have a non-zero fp16 low half.  The counts are the GPU module's docstring."""
    for kind in P.KINDS16:
        dt = X.TORCH_DT[kind]
        for case in _scaled_runs(kind):
            ties = X.count_ties(P.stream_ref(*case), dt)
            print(f'{kind} stream {case[0]} -> {case[1]} res {case[2]} x{case[6]}: {ties} ties')
            assert ties >= 100, (kind, case, ties)
        for (K2, C2) in P.PAIR_FORMS:
            y, ys, z = P.pair_ref(**P.pair_args(K2, C2, P.PAIR_M_MAX, P.PAIR_SCALE[kind][K2]), dtype=dt)
            ty, tz, moved = X.count_ties(y, dt), X.count_ties(z, dt), int((y != ys).sum())
            print(f'{kind} pair K2 {K2} C2 {C2} x{P.PAIR_SCALE[kind][K2]}: y {ty} ties, {moved} of {y.numel()} y values move when rounded; z {tz} ties')
            assert ty >= 100 and tz >= 100 and moved >= 100, (kind, K2, C2, ty, tz, moved)
        ties = X.count_ties(P.dyn_ref(P.SCALE[kind])[0][:P.DYN_SCALED_M], dt)
        print(f'{kind} dynamic_layer x{P.SCALE[kind]}, 17 rows: {ties} ties')
        assert ties >= 100
    for K, N in {(k, n) for k, n, _ in P.SCALED_STREAM['f16x3']}:
        low = X.count_inexact(P.stream_inputs(K, N, P.SCALE['f16x3'])['a'])
        print(f'f16x3 stream {K} -> {N} x683: {low} of {P.M_MAX * K} activations with a non-zero low half')
        assert low >= 100 and X.count_inexact(P.stream_inputs(K, N)['a']) == 0
    low = X.count_inexact(P.dyn_inputs(P.SCALE['f16x3'])['a'][:P.DYN_SCALED_M])
    print(f'f16x3 dynamic_layer x683, 17 rows: {low} activations with a non-zero low half')
    assert low >= 100


# ------------------------------------------------------------------------------------------------ mutants
def _stream_parts(case):
    """-> (acc [M][N], b, gathered residual rows [M][N] or None, relu, inputs, (ho, wo))"""
    K, N, r, M, up, relu, scale = case
    d = P.stream_inputs(K, N, scale)
    res = None
    if r == 1:
        res = d['res'][:M]
    elif r == 2:
        (f, ho, wo), _ = P.UP_SHAPES[up]
        res = X.nhwc(X.upsample_nearest(d['up'][up], (ho, wo))).reshape(M, N)
    return P._mm(d['a'][:M], d['w']), d['b'], res, relu, d


def _finish(acc, b, res, relu):
    y = acc + b + (res if res is not None else 0)
    return y.clamp_min(0) if relu else y


def _m_stale_residual(case, dt):
    acc, b, res, relu, _ = _stream_parts(case)
    stale = res.clone()
    stale[256:] = res[:-256]                       # tile t reads what tile t - 8 left in the buffer
    return X.expected(_finish(acc, b, stale, relu), dt)


def _m_residual_after_rounding(case, dt):
    if dt not in X.SIG_BITS:
        return None
    acc, b, res, relu, _ = _stream_parts(case)
    v = (acc + b).float().to(dt).float() + res.float()
    return (v.clamp_min(0) if relu else v).to(dt)


def _m_truncates(case, dt):
    return X.truncated(P.stream_ref(*case), dt) if dt in X.SIG_BITS else None


def _m_slices_swapped(case, dt):
    y = X.expected(P.stream_ref(*case), dt).clone()
    c = 128 if dt == torch.float32 else P.channels_per_workgroup('bf16', case[0], case[1])
    y[:, :c], y[:, c:2 * c] = y[:, c:2 * c].clone(), y[:, :c].clone()
    return y


def _m_k_tail_dropped(case, dt):
    acc, b, res, relu, d = _stream_parts(case)
    w = d['w'].clone()
    w[:, -16:] = 0
    return X.expected(_finish(P._mm(d['a'][:case[3]], w), b, res, relu), dt)


def _m_bias_of_another_channel(case, dt):
    acc, b, res, relu, _ = _stream_parts(case)
    return X.expected(_finish(acc, b.roll(-128), res, relu), dt)


def _m_integer_upsample(case, dt):
    K, N, r, M, up, relu, scale = case
    acc, b, _, _, d = _stream_parts(case)
    (f, ho, wo), _ = P.UP_SHAPES[up]
    res = X.nhwc(X.upsample_nearest(d['up'][up], (ho, wo), index=X.nearest_index_integer)).reshape(M, N)
    return X.expected(_finish(acc, b, res, relu), dt)


BIG, UP0 = (P.M_MAX, None), (690, 0)
STREAM_MUTANTS = [
    # (name, function, {kind: [case]})
    ('residual rows of tile t taken from tile t - 8', _m_stale_residual,
     {k: [(256, 256, 1) + BIG + (True, 1), (256, 1024, 2) + UP0 + (False, 1)] + ([(128, 512, 1) + BIG + (True, 1), (512, 256, 2) + UP0 + (False, 1)] if k != 'f16x3' else []) for k in KINDS}),
    ('residual added after the 16-bit rounding', _m_residual_after_rounding, {k: [c for c in _scaled_runs(k) if c[2] == 1] for k in P.KINDS16}),
    ('truncation instead of RNE', _m_truncates, {k: _scaled_runs(k) for k in P.KINDS16}),
    ('the channel slices of two nsp swapped', _m_slices_swapped, {k: [(256, 1024, 0) + BIG + (False, 1), (256, 1024, 1) + BIG + (True, 1)] for k in KINDS}),
    ('the last 16 K elements dropped', _m_k_tail_dropped,
     {k: [(K, N, r) + BIG + (False, 1) for K, N, r in P.stream_forms(k) if r == 0] for k in KINDS}),
    ('bias of channel c + 128', _m_bias_of_another_channel,   # (512, 256): TPW = 1, the bias in registers; the others: in LDS; f16x3: registers
     {k: [(K, N, 0) + BIG + (False, 1) for K, N in (((512, 256), (256, 256), (128, 512), (256, 1024)) if k != 'f16x3' else ((256, 256), (256, 1024)))] for k in KINDS}),
    ('the integer upsample rule instead of torch\'s', _m_integer_upsample,
     {k: [(K, N, r) + UP0 + (False, 1) for K, N, r in P.stream_forms(k) if r == 2] for k in KINDS}),
]


def _rejected(got, want, what):
    with pytest.raises(AssertionError, match='elements differ'):
        X.assert_exact(got, want, what)


def test_stream_mutants_are_rejected():
    """Each mutation of the reference is what a subtly wrong kernel would store; the bit comparison rejects it on every listed case, in
    every precision it applies to."""
    for name, fn, cases in STREAM_MUTANTS:
        for kind, lst in cases.items():
            assert lst, (name, kind)
            for case in lst:
                dt = X.TORCH_DT[kind]
                got = fn(case, dt)
                assert got is not None, (name, kind)
                _rejected(got, X.expected(P.stream_ref(*case), dt), f'{name} {kind} {case}')
    # the integer rule is NOT visible on the map where both rules agree -- which is why 46 from 14 is a case
    case = (256, 256, 2, 198, 1, False, 1)
    assert torch.equal(_m_integer_upsample(case, torch.float32), X.expected(P.stream_ref(*case), torch.float32))


def test_unwritten_last_row_and_touched_guard_rows_are_rejected():
    for kind in KINDS:
        dt = X.TORCH_DT[kind]
        K, N, r = P.stream_forms(kind)[0]
        for M in P.DENSE_M:
            want = P.with_guard(X.expected(P.stream_ref(K, N, r, M), dt))
            assert want.shape[0] == M + P.GUARD
            got = want.clone()
            got[M - 1] = P.SENTINEL                # row M - 1 not written
            _rejected(got, want, f'row M - 1 not written, M = {M}')
            got = want.clone()
            got[M, :8] = 0                         # a row past M stored
            _rejected(got, want, f'row M written, M = {M}')
    ref, _ = P.dyn_ref()
    want = P.with_guard(X.expected(ref[:P.DYN_SCALED_M], torch.float32))
    got = want.clone()
    got[16] = P.SENTINEL
    _rejected(got, want, 'dynamic_layer: row M - 1 not written')


def test_dyn_mutants_are_rejected():
    """dynamic_layer has 128 / 256 channel slices: two swapped, the K tail, the bias of another channel, truncation."""
    d = P.dyn_inputs()
    ref = P.dyn_ref()[0][:P.DYN_SCALED_M]
    a, w, b = d['a'][:P.DYN_SCALED_M], d['w'].long(), d['b']
    for kind in KINDS:
        dt = X.TORCH_DT[kind]
        want = X.expected(ref, dt)
        c = 128 if kind == 'f16x3' else 256
        sw = want.clone()
        sw[:, :c], sw[:, c:2 * c] = want[:, c:2 * c], want[:, :c]
        _rejected(sw, want, 'dyn slices swapped')
        wt = w.clone()
        wt[:, -16:] = 0
        _rejected(X.expected(P._mm(a, wt) + b, dt), want, 'dyn K tail')
        _rejected(X.expected(P._mm(a, w) + b.roll(-128), dt), want, 'dyn bias')
        if kind in P.KINDS16:
            sref = P.dyn_ref(P.SCALE[kind])[0][:P.DYN_SCALED_M]
            _rejected(X.truncated(sref, dt), X.expected(sref, dt), 'dyn truncation')


def test_pair_mutants_are_rejected():
    for kind in P.KINDS16:
        dt = X.TORCH_DT[kind]
        for (K2, C2) in P.PAIR_FORMS:
            kw = P.pair_args(K2, C2, P.PAIR_M_MAX, P.PAIR_SCALE[kind][K2])
            y, ys, z = P.pair_ref(**kw, dtype=dt)
            assert torch.equal(X.expected(y, dt), X.expected(ys, dt))         # rounding twice is rounding once: ys is y as stored
            # z from the unrounded y
            _, _, z_unrounded = P.pair_ref(**kw, dtype=None)
            _rejected(X.expected(z_unrounded, dt), X.expected(z, dt), f'pair {kind} {K2} {C2}: z from the unrounded y')
            _rejected(X.truncated(y, dt), X.expected(y, dt), 'pair: y truncated')
            _rejected(X.truncated(z, dt), X.expected(z, dt), 'pair: z truncated')
            for scale in (1, P.PAIR_SCALE[kind][K2]):
                kw = P.pair_args(K2, C2, P.PAIR_M_MAX, scale)
                y, ys, z = P.pair_ref(**kw, dtype=dt)
                if K2:                                                          # the second source ignored
                    ym, _, zm = P.pair_ref(**dict(kw, a2=None), dtype=dt)
                    _rejected(X.expected(ym, dt), X.expected(y, dt), 'pair: second source ignored (y)')
                    _rejected(X.expected(zm, dt), X.expected(z, dt), 'pair: second source ignored (z)')
                else:                                                           # the stale residual buffer: tile t reads tile t - 2's rows (two workgroups)
                    stale = kw['res'].clone()
                    stale[128:] = kw['res'][:-128]
                    ym, _, zm = P.pair_ref(**dict(kw, res=stale), dtype=dt)
                    _rejected(X.expected(ym, dt), X.expected(y, dt), 'pair: stale residual (y)')
                    _rejected(X.expected(zm, dt), X.expected(z, dt), 'pair: stale residual (z)')
                wt = kw['w1'].clone()
                wt[:, -16:] = 0
                _, _, zm = P.pair_ref(**dict(kw, w1=wt), dtype=dt)
                _rejected(X.expected(zm, dt), X.expected(z, dt), 'pair: conv1 K tail')


def test_list_mutants_are_rejected():
    dense = X.expected(P.list_ref(), torch.float32)
    for name in ('partial', 'full'):
        ids = P.LISTS[name]
        want = P.list_expected(ids)
        listed = P.listed_pixels(ids)
        assert bool((want[listed] == dense[listed]).all()) and bool((want[~listed] == P.SENTINEL).all())
        # the second half-tile of a block (its rows 4..7) shifted by one map row
        shifted = dense.clone()
        rows = torch.arange(dense.shape[1])
        second = (rows % 8) >= 4
        shifted[:, second] = dense[:, (rows[second] + 1).clamp_max(dense.shape[1] - 1)]
        _rejected(P.list_expected(ids, shifted), want, f'list {name}: second half-tile shifted')
        if name == 'partial':
            _rejected(torch.where(listed[..., None], dense, dense * 0), want, f'list {name}: unlisted pixels written')
    assert bool((P.list_expected(P.LISTS['empty']) == P.SENTINEL).all())
    _rejected(P.list_expected(P.LISTS['full']), P.list_expected(P.LISTS['partial']), 'an unlisted block computed')
    want = P.list_expected(P.LISTS['partial'])
    assert torch.equal(want, P.list_expected([b for b in P.LISTS['partial'] if 0 <= b < P.LIST_NBLK]))   # ids outside the map: nothing written
