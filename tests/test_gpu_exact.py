"""-m gpu: the contraction kernels of libmcgaze_hip.so -- mcg_conv2d in every precision, tile and variant, mcg_conv3x3_wino_x3,
mcg_stem_forward, mcg_bottleneck_x3 (and the layout helpers' 16-bit conversion) -- against an int64 statement of the same operator,
BIT FOR BIT.  tests/exact_cases.py holds the inputs, the references and the condition; tests/test_exact_cases_cpu.py proves them on the CPU.

THE EXACTNESS CONDITION.  Activations are integers in {-3..3} ({0..3} where the real input is post-ReLU; a few cases scale them), weights
ternary (24 x ternary for F(4,3), whose G divides by 24), biases and residuals integers in {-3..3}.  For every layer of every case the same
operator over absolute values, sum |x| |w| + |b| + |res|, stays below 2^24 (largest: 10 545 312), so every product and every partial sum
is an integer that f32 holds, whatever the summation order, tile, K split or power-of-two pre-scale; every activation fed to an f16x3
contraction stays below 2^22, so its split into two fp16 halves is exact.  exact_cases.check_exactness asserts this on the inputs of
every case (CPU test); it is never a skip.  No tolerance is left: a wrong tap, pad, stride, channel slice, K tail, masked row, frame
boundary, residual index, upsample index or rounding point changes some integer.

THE ROUNDING CONVENTION.  f32 / f16x3: the integer itself.  bf16 / fp16: ONE round-to-nearest-even of the integer, after bias, residual
and ReLU (include/mcgaze_hip.h: f32 accumulate, bias / residual / ReLU in f32, one store).  The x 16 case has 2138 (bf16) and 848 (fp16)
outputs exactly halfway between two representable values; the fused tail's scaled runs feed 4420 (x 16: y) and 6268 / 118 199
(x 64: t / y) activations with a non-zero fp16 low half into the chained contractions.

WHAT THE TOLERANCES LET THROUGH.  Each mutation below was applied to the reference on the CPU (test_exact_cases_cpu.py::
test_mutants_are_rejected); the bit comparison rejects every one in every precision.  Beside it, scale_err (max |d| over the
reference's largest element) of the mutant on the same inputs, and whether the bounds of tests/test_gpu_kernels.py -- 1e-4 f32, 2e-2 bf16,
2.5e-3 fp16, 1.5e-6 f16x3 -- accept it:

    mutant (case)                                          f32               bf16               fp16               f16x3
    last 8 K elements dropped (c64, K = 576)               1.1e-01 rejected  1.1e-01 rejected   1.1e-01 rejected   1.1e-01 rejected
    last 8 K elements dropped (deep, K = 4608)             4.4e-02 rejected  4.4e-02 rejected   4.4e-02 rejected   4.4e-02 rejected
    border tap from the wrong side of the pad (c64)        2.4e-01 rejected  2.4e-01 rejected   2.4e-01 rejected   2.4e-01 rejected
    stride2 ignored (cat_s2)                               6.5e-01 rejected  6.5e-01 rejected   6.5e-01 rejected   6.5e-01 rejected
    upsample index y // 2 on an odd map (up)               4.3e-02 rejected  4.3e-02 rejected   4.3e-02 rejected   4.3e-02 rejected
    truncation instead of RNE (deep_x16)                   -                 5.0e-03 ACCEPTED   4.8e-04 ACCEPTED   -
    rounded before the residual add (deep_x16)             -                 2.7e-03 ACCEPTED   6.5e-04 ACCEPTED   -
    one frame's rows shifted by one (c64)                  1.0e+00 rejected  1.0e+00 rejected   1.0e+00 rejected   1.0e+00 rejected

Both rounding mutants pass today's 16-bit bounds with a margin of 4 to 7.  The K-tail mutant does not on THESE inputs (dense small
integers make 8 dropped terms 4 - 11 % of the largest output, twice the bf16 bound); a tolerance test sees it only while the dropped
terms are large against the bound, the bit comparison always.
"""
import functools

import pytest
import torch

from mcgaze_amd import lib as L
from tests import exact_cases as X

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def eng():
    from mcgaze_amd import engine
    return engine


def _dev(t_nchw, dtype):
    """int64 NCHW -> NHWC ``dtype`` on the device; the conversion itself must be exact."""
    v = X.nhwc(t_nchw).to(dtype)
    assert torch.equal(v.to(torch.int64), X.nhwc(t_nchw)), 'an input is not representable in its storage type'
    return v.to(DEV)


# ------------------------------------------------------------------------------------------------ mcg_conv2d
def _conv_params():
    out = []
    for name in X.CONV_CASES:
        for kind in X.CONV_ONLY.get(name, X.DTYPES):
            marks = () if X.conv_supported(name, kind) else pytest.mark.skip(
                reason=f'mcg_conv2d ({kind}): channel counts are multiples of {X.CIN_GRANULE[kind]} (Cin) and {X.COUT_GRANULE[kind]} (Cout)')
            out.append(pytest.param(name, kind, marks=marks, id=f'{name}-{kind}'))
    return out


@functools.lru_cache(maxsize=None)
def _conv_inputs(name, kind):
    kw, _ = X.conv_case(name)
    dt = X.TORCH_DT[kind]
    d = dict(x=_dev(kw['x'], dt), w=_dev(kw['w'], dt), bias=kw['b'].float().to(DEV), stride=kw['stride'], pad=kw['pad'], relu=kw['relu'],
             split=kind == 'f16x3')
    if kw.get('res') is not None:
        d.update(residual=_dev(kw['res'], dt), residual_mode=kw['res_mode'])
    if kw.get('x2') is not None:
        d.update(x2=_dev(kw['x2'], dt), stride2=kw['stride2'])
    return d


def _conv_variants(name, kind):
    """Beyond the default launch: every tile the launcher accepts for the problem (igemm.hip: tile_ok; forced tiles apply to Cout > 64),
    the register-staged kernel (16-bit), the unscaled packing (f16x3), and the generic path where a specialised kernel exists."""
    N, H, W, cin, cout, k, stride, pad, relu, resk, cat, scale = X.CONV_CASES[name]
    v = []
    if name == 'c64':
        v.append(dict(flags=L.FLAG_NO_SPECIALISED))
    if cout > 64 and kind in ('bf16', 'fp16'):
        v += [dict(tile=t) for t in (9, 11, 12, 15)]
        if cin % 64 == 0 and not cat:          # 128-byte K slices, no second source
            v.append(dict(tile=14))
        v.append(dict(flags=L.FLAG_STAGED_GEMM))
    if cout > 64 and kind == 'f16x3':
        v += [dict(tile=t) for t in (50, 51, 53)] + [dict(prescale=False)]
    return v


@pytest.mark.parametrize('name,kind', _conv_params())
def test_conv2d_is_exact(eng, name, kind):
    """mcg_conv2d, the launcher's own choice of kernel and tile."""
    want = X.expected(X.conv_case(name)[1], X.TORCH_DT[kind])
    y = eng.conv2d(**_conv_inputs(name, kind))
    torch.cuda.synchronize()
    X.assert_exact(y, want, f'conv2d {name} {kind}')


@pytest.mark.parametrize('name,kind', [p for p in _conv_params() if _conv_variants(*p.values)])
def test_conv2d_variants_are_exact(eng, name, kind):
    """Every forced tile, MCG_FLAG_STAGED_GEMM, MCG_FLAG_NO_SPECIALISED and prescale=False: each against the integers, not against each other."""
    want = X.expected(X.conv_case(name)[1], X.TORCH_DT[kind])
    outs = [(v, eng.conv2d(**_conv_inputs(name, kind), **v)) for v in _conv_variants(name, kind)]
    torch.cuda.synchronize()
    for v, y in outs:
        X.assert_exact(y, want, f'conv2d {name} {kind} {v}')


# ------------------------------------------------------------------------------------------------ mcg_conv3x3_wino_x3
@pytest.mark.parametrize('full', [True, False], ids=['bias_relu', 'plain'])
@pytest.mark.parametrize('g,shape', [(g, s) for g, shapes in X.WINO_CASES.items() for s in shapes])
def test_conv3x3_wino_x3_is_exact(eng, g, shape, full):
    """F(2,3) on tiles 0..4 and F(4,3) (weights 24 x ternary) on tiles 0..2, with bias and ReLU and without both."""
    x, w, b, refs = X.wino_case(g, shape)
    want = X.expected(refs[full], torch.float32)
    xd, wd, bd = _dev(x, torch.float32), _dev(w, torch.float32), b.float().to(DEV) if full else None
    outs = [(t, eng.conv3x3_wino(xd, wd, bd, relu=full, tile=t, g=g)) for t in X.WINO_TILES[g]]
    torch.cuda.synchronize()
    for t, y in outs:
        X.assert_exact(y, want, f'wino g={g} {shape} tile {t} {"bias + relu" if full else "plain"}')


# ------------------------------------------------------------------------------------------------ mcg_stem_forward
@pytest.mark.parametrize('kind', X.DTYPES)
@pytest.mark.parametrize('shape', X.STEM_SHAPES)
def test_stem_is_exact(eng, shape, kind):
    """The fused stem and the three-kernel path (MCG_FLAG_NO_SPECIALISED) on an integer image, integer 7x7 weights and bias."""
    from mcgaze_amd.packing import pack_stem
    kw, ref = X.stem_case(shape)
    dt, split = X.TORCH_DT[kind], kind == 'f16x3'
    ws, bs = pack_stem(kw['w'].float(), kw['b'].float(), dt, split)
    img = kw['img'].float().to(DEV)
    outs = [(f, eng.stem(img, ws.to(DEV), bs.to(DEV), dt, flags=f, split=split)) for f in (0, L.FLAG_NO_SPECIALISED)]
    torch.cuda.synchronize()
    for f, y in outs:
        X.assert_exact(y, X.expected(ref, dt), f'stem {shape} {kind} flags={f}')


# ------------------------------------------------------------------------------------------------ mcg_bottleneck_x3
@pytest.mark.parametrize('shape,combo,scale', X.BNECK_CASES, ids=[f'{s[0]}x{s[1]}x{s[2]}-cm{c[0]}-nsrc{c[1]}-cn{c[2]}-x{k}' for s, c, k in X.BNECK_CASES])
def test_fused_bottleneck_tail_is_exact(eng, shape, combo, scale):
    """conv2 -> conv3 (+ downsample source | + residual) -> next conv1, chained in registers: y AND z are the integers."""
    from mcgaze_amd.packing import bneck_stream
    cm, nsrc, cn = combo
    kw, ref = X.bneck_case(shape, combo, scale)
    f = lambda t: t.float() if t is not None else None
    ws, bs = bneck_stream(X.nhwc(kw['w2']).float(), f(kw['b2']), f(kw['w3']), f(kw['b3']), f(kw.get('w1n')), f(kw.get('b1n')))
    gy, gz = eng.bottleneck_x3(_dev(kw['x'], torch.float32), _dev(kw['src2'], torch.float32), ws.to(DEV), bs.to(DEV), cn, nsrc)
    torch.cuda.synchronize()
    X.assert_exact(gy, X.expected(ref[1], torch.float32), f'fused tail {shape} {combo} x{scale}: y')
    assert (gz is None) == (cn == 0)
    if cn:
        X.assert_exact(gz, X.expected(ref[2], torch.float32), f'fused tail {shape} {combo} x{scale}: z')


# ------------------------------------------------------------------------------------------------ layout helpers
@pytest.mark.parametrize('kind', ['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape', X.LAYOUT_SHAPES)
def test_layout_conversion_rounds_ties_to_even(eng, shape, kind):
    """mcg_nchw_to_nhwc is a 16-bit store of its own: integers up to 5000 hold bf16 and fp16 ties (test_layout_roundtrip's randn holds none)."""
    dt = X.TORCH_DT[kind]
    x = X.layout_case(shape)
    y = eng.to_nhwc(x.float().to(DEV), dt)
    back = eng.to_nchw(y)
    torch.cuda.synchronize()
    X.assert_exact(y, X.expected(X.nhwc(x), dt), f'to_nhwc {shape} {kind}')
    assert torch.equal(back.cpu(), X.expected(x, dt).float())
