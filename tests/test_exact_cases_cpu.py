"""CPU: the instrument of tests/test_gpu_exact.py proved without a GPU (tests/exact_cases.py).  Every case the GPU file runs satisfies
the exactness condition; the packers are exact on its weights; the 16-bit cases contain rounding ties; the comparison rejects every
subtly wrong kernel listed below (each mutation applied to the reference), and the table printed by test_mutants_are_rejected says which
of them the scale_err bounds of tests/test_gpu_kernels.py accept on the same inputs; and packing.pack_stem returns the bytes
PackedWeights always packed."""
import hashlib

import pytest
import torch
import torch.nn.functional as F

from mcgaze_amd import packing
from tests import exact_cases as X

# the bounds of tests/test_gpu_kernels.py (TOL, X3_TOL): maximum absolute error over the reference's largest element
TODAY_TOL = {'f32': 1e-4, 'bf16': 2e-2, 'fp16': 2.5e-3, 'f16x3': 1.5e-6}


def scale_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def test_every_gpu_case_satisfies_the_exactness_condition():
    worst = {}
    for name in X.CONV_CASES:
        kw, ref = X.conv_case(name)
        worst['conv ' + name] = X.check_exactness(X.conv2d_ref, 'conv ' + name, x3=True, **kw)
        assert name in X.CONV_ONLY or int(ref.abs().max()) <= 65504     # the fp16 runs stay finite
    for g, shapes in X.WINO_CASES.items():
        for shape in shapes:
            x, w, b, _ = X.wino_case(g, shape)
            X.check_exactness(X.conv3x3_ref, f'wino g={g} {shape}', x3=True, x=x, w=w, b=b)
            worst[f'wino g={g} {shape} (transformed domain)'] = X.check_exactness_wino(x, w, b, g, f'wino g={g} {shape}')
    for shape in X.STEM_SHAPES:
        kw, ref = X.stem_case(shape)
        worst[f'stem {shape}'] = X.check_exactness(X.stem_ref, f'stem {shape}', x3=True, **kw)
        assert worst[f'stem {shape}'] <= 3 * 3 * 147 + 3
    for shape, combo, scale in X.BNECK_CASES:
        kw, _ = X.bneck_case(shape, combo, scale)
        worst[f'bneck {shape} {combo} x{scale}'] = X.check_exactness(X.bneck_ref, f'bneck {shape} {combo} x{scale}', x3=True, **kw)
    top = max(worst, key=worst.get)
    print(f'largest sum of absolute values over {len(worst)} cases: {worst[top]} ({top}); the limit is 2^24 = {X.LIMIT}')
    assert worst[top] < X.LIMIT


def test_the_condition_rejects_instead_of_skipping():
    g = X.gen(1)
    x = X.acts(g, (1, 32, 4, 4), scale=1 << 20)
    w = X.ternary(g, (8, 32, 1, 1), 1.0)
    with pytest.raises(AssertionError, match='2\\^24'):
        X.check_exactness(X.conv2d_ref, 'too large', x=x, w=w)
    x = X.acts(g, (1, 32, 4, 4), scale=1 << 21)
    w = X.ternary(g, (8, 32, 1, 1), 0.0)
    with pytest.raises(AssertionError, match='2\\^22'):
        X.check_exactness(X.conv2d_ref, 'activation too large', x3=True, x=x + (1 << 22), w=w)


def test_references_agree_with_torch():
    """upsample_nearest is F.interpolate(size=, nearest); conv2d_ref is F.conv2d with the epilogue spelled out; expected() rounds ties to even."""
    r = torch.arange(2 * 3 * 4 * 5).reshape(2, 3, 4, 5)
    for size in ((9, 11), (8, 10), (4, 5), (7, 6)):
        assert torch.equal(X.upsample_nearest(r, size), F.interpolate(r.double(), size=size, mode='nearest').long())
    kw, ref = X.conv_case('up')
    y = F.conv2d(kw['x'].double(), kw['w'].double(), kw['b'].double()) + F.interpolate(kw['res'].double(), size=(9, 11), mode='nearest')
    assert torch.equal(ref, X.nhwc(y).long())
    kw, ref = X.conv_case('cat_s2')
    y = F.relu(F.conv2d(kw['x'].double(), kw['w'][:, :128].double()) + F.conv2d(kw['x2'].double(), kw['w'][:, 128:].double(), stride=2) + kw['b'].double()[None, :, None, None])
    assert torch.equal(ref, X.nhwc(y).long())
    v = torch.tensor([255, 257, 259, 261, -257, 2049, 2051, -2051, 4098, 4102])
    assert X.expected(v, torch.bfloat16).tolist() == [255, 256, 260, 260, -256, 2048, 2048, -2048, 4096, 4096]
    assert X.expected(v, torch.float16).tolist() == [255, 257, 259, 261, -257, 2048, 2052, -2052, 4096, 4104]
    assert X.truncated(v, torch.float16).tolist() == [255, 257, 259, 261, -257, 2048, 2050, -2050, 4096, 4100]
    assert X.count_ties(v, torch.bfloat16) == 4 and X.count_ties(v, torch.float16) == 5    # bf16: 257 .. -257; fp16: 2049 .. 4102
    assert X.count_inexact(v, torch.float16) == 5


def test_assert_exact_semantics():
    a = torch.tensor([[[[0.0, 1.0], [2.0, 3.0]]]])
    X.assert_exact(a.clone(), a, 'same')
    X.assert_exact(-a * 0, a * 0, 'minus zero equals zero')
    b = a.clone()
    b[0, 0, 1, 0] = 2.5
    b[0, 0, 1, 1] = 7.0
    with pytest.raises(AssertionError) as e:
        X.assert_exact(b, a, 'two wrong')
    msg = str(e.value)
    assert '2 of 4 elements differ' in msg and '(0, 0, 1, 0)' in msg and 'got 2.5' in msg and 'want 2.0' in msg and 'max |d| = 4' in msg
    n = a.clone()
    n[0, 0, 0, 1] = float('nan')
    with pytest.raises(AssertionError, match='1 of 4'):
        X.assert_exact(n, n.clone(), 'NaN equals nothing')
    with pytest.raises(AssertionError):
        X.assert_exact(a.to(torch.bfloat16), a, 'dtype')


def _halves(packed_pairs):
    """[..., K / 8, 2, 8] chunks of split_pack -> hi + lo as float64 [..., K]."""
    v = packed_pairs.double()
    return (v[..., 0, :] + v[..., 1, :]).reshape(*v.shape[:-3], -1)


def test_packers_are_exact_on_the_test_weights():
    """After pow2_prescale, hi + lo == w * 2^e exactly: split_pack, frag_major_split, bneck_stream's slabs and wino_pack(g=2) on ternary
    weights, wino_pack(g=4) on 24 x ternary (G w stays integral)."""
    g = X.gen(3)
    w = X.ternary(g, (128, 3, 3, 64), 0.5)                                     # OHWI
    ws, d = packing.pow2_prescale(w.reshape(128, -1))
    assert d == 2.0 ** -14 and torch.equal(ws, w.reshape(128, -1).double() * 2 ** 14)
    sp = packing.split_pack(ws)
    assert sp.dtype == torch.float16 and torch.equal(_halves(sp.reshape(128, -1, 2, 8)), ws)
    m = X.ternary(g, (64, 256), 0.25)
    ms, _ = packing.pow2_prescale(m)
    f = packing.frag_major_split(ms).reshape(64 // 32, 256 // 16, 2, 64, 8).double()      # [t][ks][hl][lane][e]
    assert torch.equal(f[:, :, 0] + f[:, :, 1], packing.frag_major(ms).reshape(2, 16, 64, 8))
    assert float(f[:, :, 1].abs().max()) == 0.0                                # ternary x 2^14: the low halves are empty, the high ones the weight
    # bneck_stream: every slab holds its 64 x 64 block of w * 2^14 (same multiset of values per slab; the layout is test_packing_cpu's subject)
    cm, cn = 64, 128
    w2, w3, w1 = X.ternary(g, (cm, 3, 3, cm), 0.25), X.ternary(g, (4 * cm, cm + 64), 0.25), X.ternary(g, (cn, 4 * cm), 0.125)
    b2, b3, b1 = X.small(g, (cm,)), X.small(g, (4 * cm,)), X.small(g, (cn,))
    stream, bias = packing.bneck_stream(w2.float(), b2.float(), w3.float(), b3.float(), w1.float(), b1.float())
    slabs = stream.reshape(-1, 2, 4, 2, 64, 8).double()
    assert torch.equal(bias[:cm + 4 * cm + cn], torch.cat([b2, b3, b1]).float()) and bias[-4:].tolist() == [2.0 ** -14] * 3 + [0.0]
    assert float(slabs[:, :, :, 1].abs().max()) == 0.0
    blocks = [w2[:, kh, kw, :] for kh in range(3) for kw in range(3)]
    blocks += [t for oc in range(4) for t in ([w3[oc * 64:(oc + 1) * 64, p * 64:(p + 1) * 64] for p in range(2)] + [w1[p * 64:(p + 1) * 64, oc * 64:(oc + 1) * 64] for p in range(2)])]
    assert len(blocks) == slabs.shape[0]
    for sl, blk in zip(slabs[:, :, :, 0], blocks):
        for ct in range(2):                                                    # lane l of channel tile ct holds row 32 ct + (l & 31)
            rows = sl[ct].permute(1, 0, 2).reshape(2, 32, 32)                  # [lane >> 5][lane & 31][s, e]
            got = torch.cat([rows[0], rows[1]], dim=1).sort(dim=1).values
            assert torch.equal(got, (blk[32 * ct:32 * ct + 32].double() * 2 ** 14).sort(dim=1).values)
    # Winograd: hi + lo == G (w 2^e), G w stated in integer arithmetic (exact_cases.wino_transformed_weights)
    def halves_and_u(tern, gg):
        wsc, d = packing.pow2_prescale(tern)                                   # OHWI
        e = round(1 / d)
        assert torch.equal(wsc, tern.double() * e)
        nv = len(packing.WINO_G[gg])
        v = packing.wino_pack(wsc, g=gg).reshape(1, 2, 3, nv, 4, 2, 2, 32, 8).double()          # nt, cs, ky, nu, ct, hl, half, n, e
        u = X.wino_transformed_weights(tern.permute(0, 3, 1, 2), gg).double() * e / X.WINO_UNIT[gg]   # [nu][co][ky][ci], exact: e is a power of two
        u = u.reshape(nv, 1, 4, 32, 3, 2, 2, 8).permute(1, 5, 4, 0, 2, 6, 3, 7)                  # nt, cs, ky, nu, ct, half, n, e
        return v[:, :, :, :, :, 0] + v[:, :, :, :, :, 1], u
    for gg in (2, 4):
        got, u = halves_and_u(X.ternary(g, (128, 3, 3, 32), 0.5) * X.WINO_WSCALE[gg], gg)
        assert torch.equal(got, u) and float(u.abs().max()) > 0
    # ... and F(4,3) on PLAIN ternary weights is not even integral in any power-of-two unit (thirds): the reason for the factor 24
    with pytest.raises(AssertionError, match='not a multiple'):
        X.wino_transformed_weights(X.ternary(g, (128, 32, 3, 3), 0.5), 4)


def test_sixteen_bit_cases_contain_ties_and_the_x3_cases_low_halves():
    """Per 16-bit dtype, how many reference integers of each conv case lie exactly halfway between two representable values: at least one
    case per dtype must have some (else round-to-nearest-even would go untested), and the x 16 case must for both.  For f16x3: the
    activations whose split has a non-zero low half -- the x 683 input, and the chained t and y of the fused tail's x 16 run."""
    for dt in (torch.bfloat16, torch.float16):
        counts = {name: X.count_ties(X.conv_case(name)[1], dt) for name in X.CONV_CASES if name not in X.CONV_ONLY}
        print(f'{dt}: reference integers on a rounding tie, per conv case: {counts}')
        assert any(counts.values()) and counts['deep_x16'] > 0, (dt, counts)
        inexact = X.count_inexact(X.conv_case('deep_x16')[1], dt)
        assert inexact > counts['deep_x16']                                    # values that round, ties and others
    low = X.count_inexact(X.conv_case('tails_wide')[0]['x'])
    print(f'f16x3: activations with a non-zero low half: conv tails_wide input {low}')
    assert low > 0
    for shape, combo, scale in X.BNECK_SCALED:
        t, y, z = X.bneck_case(shape, combo, scale)[1]
        lt, ly = X.count_inexact(t), X.count_inexact(y)
        print(f'f16x3: fused tail x{scale}: t {lt} of {t.numel()} (max {int(t.max())}), y {ly} of {y.numel()} (max {int(y.max())}) with a non-zero low half')
        assert ly > 0 and (lt > 0 or scale == 16)
    for dt in (torch.bfloat16, torch.float16):
        x = X.layout_case(X.LAYOUT_SHAPES[-1])
        assert X.count_ties(x, dt) > 0


# ------------------------------------------------------------------------------------------------ mutants
def _acc(kw, w=None, stride2=None):
    """The bare contraction of a conv case, NCHW int64."""
    w = kw['w'] if w is None else w
    cin = kw['x'].shape[1]
    y = X._conv(kw['x'], w[:, :cin], kw['stride'], kw['pad'])
    if kw.get('x2') is not None:
        y = y + X._conv(kw['x2'], w[:, cin:], stride2 or kw['stride2'])[:, :, :y.shape[2], :y.shape[3]]
    return y


def _finish(acc, kw, up=None):
    y = acc + kw['b'][None, :, None, None]
    if kw.get('res_mode') == 1:
        y = y + kw['res']
    elif kw.get('res_mode') == 2:
        y = y + (X.upsample_nearest(kw['res'], y.shape[2:]) if up is None else up)
    return X.nhwc(y.clamp_min(0) if kw['relu'] else y)


def _k_tail_dropped(kw, dt):
    w = kw['w'].clone()
    w[:, -8:, -1, -1] = 0                       # K = (kh, kw, cin): its last 8 elements are the last tap's last 8 channels
    return X.expected(_finish(_acc(kw, w), kw), dt)


def _border_tap_wraps(kw, dt):
    acc = _acc(kw).clone()                      # output column 0, tap (ky 1, kx 0) lies in the pad: read the row's LAST pixel instead of zero
    acc[:, :, :, 0] += torch.einsum('oc,nch->noh', kw['w'][:, :, 1, 0], kw['x'][:, :, :, -1])
    return X.expected(_finish(acc, kw), dt)


def _stride2_ignored(kw, dt):
    return X.expected(_finish(_acc(kw, stride2=1), kw), dt)


def _upsample_halves_the_index(kw, dt):
    r, (ho, wo) = kw['res'], _acc(kw).shape[2:]
    ih, iw = (torch.arange(ho) // 2).clamp_max(r.shape[2] - 1), (torch.arange(wo) // 2).clamp_max(r.shape[3] - 1)
    return X.expected(_finish(_acc(kw), kw, up=r[:, :, ih][:, :, :, iw]), dt)


def _truncates(kw, dt):
    return X.truncated(_finish(_acc(kw), kw), dt) if dt in X.SIG_BITS else None


def _rounds_before_the_residual(kw, dt):
    if dt not in X.SIG_BITS:
        return None
    r = (_acc(kw) + kw['b'][None, :, None, None]).float().to(dt).float() + kw['res'].float()
    return X.nhwc(r.clamp_min(0)).to(dt)


def _frame_shifted(kw, dt):
    y = _finish(_acc(kw), kw).clone()
    y[1] = y[1].roll(1, dims=0)                 # frame 1's rows land one row down
    return X.expected(y, dt)


MUTANTS = [('last 8 K elements dropped', 'c64', _k_tail_dropped),
           ('last 8 K elements dropped, K = 4608', 'deep', _k_tail_dropped),
           ('border tap from the wrong side of the pad', 'c64', _border_tap_wraps),
           ('stride2 ignored', 'cat_s2', _stride2_ignored),
           ('upsample index y // 2 on an odd map', 'up', _upsample_halves_the_index),
           ('truncation instead of RNE', 'deep_x16', _truncates),
           ('rounded before the residual add', 'deep_x16', _rounds_before_the_residual),
           ("one frame's rows shifted by one", 'c64', _frame_shifted)]

# What was observed: per mutant, the kinds whose scale_err bound of tests/test_gpu_kernels.py ACCEPTS it on these inputs (every kind's
# bit comparison rejects every mutant).  The two rounding mutants do not exist for f32 / f16x3.
ACCEPTED_TODAY = {
    'last 8 K elements dropped': (),
    'last 8 K elements dropped, K = 4608': (),
    'border tap from the wrong side of the pad': (),
    'stride2 ignored': (),
    'upsample index y // 2 on an odd map': (),
    'truncation instead of RNE': ('bf16', 'fp16'),
    'rounded before the residual add': ('bf16', 'fp16'),
    "one frame's rows shifted by one": (),
}


def test_mutants_are_rejected():
    """Each mutation of the reference is what a subtly wrong kernel would store.  assert_exact must reject every one in every precision;
    the table says which of them today's scale_err bounds accept on the same inputs."""
    print(f'\n{"mutant (case)":<56}' + ''.join(f'{k:>22}' for k in X.DTYPES))
    for name, case, fn in MUTANTS:
        kw, ref = X.conv_case(case)
        assert torch.equal(_finish(_acc(kw), kw), ref)
        cells, accepted = [], []
        for kind in X.DTYPES:
            dt = X.TORCH_DT[kind]
            got = fn(kw, dt)
            if got is None:
                cells.append('-')
                continue
            want = X.expected(ref, dt)
            with pytest.raises(AssertionError, match='elements differ'):
                X.assert_exact(got, want, name)
            err = scale_err(got, ref)
            if err < TODAY_TOL[kind]:
                accepted.append(kind)
            cells.append(f'{err:.1e} {"ACCEPTED" if err < TODAY_TOL[kind] else "rejected"}')
        print(f'{name + " (" + case + ")":<56}' + ''.join(f'{c:>22}' for c in cells))
        assert tuple(accepted) == ACCEPTED_TODAY[name], (name, accepted)


# ------------------------------------------------------------------------------------------------ pack_stem
STEM_SHA256 = {   # sha256 over weight bytes + bias bytes of PackedWeights(synth.make_state_dict(0)).stem before pack_stem existed
    ('f32', False): '0401b886ecafcc30b0038a488d17864fc802a74a6b8db3b6c1496f037ced9fda',
    ('bf16', False): 'd7933982fab61040c89134aa99e8ab963db802c0e1910c4a4bcd9ac750ad6021',
    ('fp16', False): 'b0c1336673473f33404853d89452224ba2d859accd0c266068c44b1ea6dcf302',
    ('f32', True): 'b60ca3a931d26b28316e91fa3f102e0add9879fc831350b2695246eecbaac105',
}


def test_pack_stem_changes_no_bytes():
    from mcgaze_amd import synth
    sd = packing.normalize_state_dict(synth.make_state_dict(0))
    w, b = packing.fold_bn(sd, 'backbone.conv1.weight', 'backbone.bn1')
    raw = lambda t: t.contiguous().view(torch.uint8).numpy().tobytes()
    for (kind, split), digest in STEM_SHA256.items():
        dt = X.TORCH_DT[kind]
        ws, bs = packing.pack_stem(w, b, dt, split)
        assert hashlib.sha256(raw(ws) + raw(bs)).hexdigest() == digest, (kind, split)
        stem = torch.zeros(64, 7, 8, 4)                                        # the four lines it replaces, restated
        stem[:, :, :7, :3] = w.permute(0, 2, 3, 1)
        old = packing.split_pack(stem.reshape(64, -1)) if split else stem.to(dt)
        assert ws.dtype == old.dtype and ws.shape == old.shape and raw(ws) == raw(old) and raw(bs) == raw(b.float())
    pw = packing.PackedWeights(sd, dtype=torch.bfloat16, device='cpu')        # ... and PackedWeights hands out exactly that
    ws, bs = packing.pack_stem(w, b, torch.bfloat16)
    assert raw(pw.stem['w']) == raw(ws) and raw(pw.stem['bias']) == raw(bs)
