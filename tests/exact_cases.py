"""Shared by tests/test_exact_cases_cpu.py and tests/test_gpu_exact.py: small-integer inputs for the contraction kernels, an int64 statement
of each operator, and the condition under which a kernel that accumulates in f32 must return that statement bit for bit.

THE EXACTNESS CONDITION.  Activations are integers in {-3..3} ({0..3} where the real input is post-ReLU), weights are ternary, biases and
residuals integers in {-3..3}.  If sum |x| |w| + |b| + |res| stays below 2^24 at every output, every product and every partial sum of the
contraction is an integer below 2^24 in magnitude, hence an f32 value, whatever the summation order, the tile or the split into fp16
halves (a pre-scale by a power of two moves exponents only).  For the f16x3 kernels an activation is split into two fp16 halves of 11
bits each, which is exact for integers below 2^22: inputs and chained intermediates must stay below that.  ``check_exactness`` asserts
both on the inputs of a case (the same operator over absolute values); it never skips.

THE ROUNDING CONVENTION.  f32 and f16x3 results are the integers themselves.  bf16 / fp16 results are ONE round-to-nearest-even of the
integer after bias, residual and ReLU (``expected``).
"""
import functools

import torch
import torch.nn.functional as F

LIMIT = 1 << 24        # integers below this magnitude are f32 values
X3_LIMIT = 1 << 22     # ... and split exactly into two fp16 halves
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}


# ------------------------------------------------------------------------------------------------ generators (int64, seeded)
def gen(seed):
    return torch.Generator().manual_seed(seed)


def acts(g, shape, post_relu=False, scale=1):
    """Activations: integers in {-3..3}, or {0..3} where the real input is post-ReLU, times ``scale``."""
    return torch.randint(0 if post_relu else -3, 4, shape, generator=g) * scale


def ternary(g, shape, density):
    """Weights in {-1, 0, +1}: non-zero with probability ``density``, either sign equally often."""
    nz = torch.rand(shape, generator=g) < density
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return sign * nz


def small(g, shape):
    """Biases and residuals: integers in {-3..3}."""
    return torch.randint(-3, 4, shape, generator=g)


# ------------------------------------------------------------------------------------------------ references (NCHW in, NHWC int64 out)
def _integral(t, what='reference'):
    assert bool((t == t.round()).all()) and float(t.abs().max()) < 2.0 ** 52, f'{what}: not an integer tensor'
    return t.round().to(torch.int64)


def _conv(x, w, stride=1, pad=0):
    """Integer convolution (NCHW x OIHW) through float64, whose products and sums of such integers are exact."""
    return _integral(F.conv2d(x.double(), w.double(), stride=stride, padding=pad), 'conv')


def nearest_index(out, inn):
    """The source index F.interpolate(mode='nearest') reads for each of ``out`` destinations of an axis of ``inn`` sources, by torch's own
    rule on f32 tensors: min(floor(dst * scale), in - 1) with scale = in / out divided in f32 and the product rounded to f32
    (include/mcgaze_hip.h; common.hpp: nearest_src_row).  It is NOT floor(dst * in / out) in integers: for out <= 64 the two part at (out,
    in, dst) = (44, 26, 22), (46, 14, 23), (46, 28, 23), (58, 30, 29), where the rounded scale falls below in / out."""
    scale = torch.tensor(float(inn), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
    return torch.floor(torch.arange(out, dtype=torch.float32) * scale).to(torch.int64).clamp_max(inn - 1)


def nearest_index_integer(out, inn):
    """MUTANT of ``nearest_index``: floor(dst * in / out) in integer arithmetic."""
    return (torch.arange(out) * inn) // out


def upsample_nearest(r, size, index=nearest_index):
    """F.interpolate(r, size=size, mode='nearest') on integers: the gather by torch's index rule (``nearest_index``)."""
    ih, iw = index(size[0], r.shape[2]), index(size[1], r.shape[3])
    return r[:, :, ih][:, :, :, iw]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv2d_ref(x, w, b=None, stride=1, pad=0, relu=False, res=None, res_mode=0, x2=None, stride2=1):
    """mcg_conv2d.  x [N,Cin,H,W], w [Cout,Cin(+Cin2),k,k], b [Cout], res [N,Cout,Ho,Wo] (res_mode 1) or [N,Cout,Hr,Wr] (2: nearest
    upsample to the output's size, then add), x2 [N,Cin2,H2,W2]: a second source K-concatenated behind x and sampled at stride2
    (1x1 convs only).  -> (y,), NHWC int64."""
    cin = x.shape[1]
    y = _conv(x, w[:, :cin], stride, pad)
    if x2 is not None:
        assert w.shape[2:] == (1, 1) and stride == 1 and pad == 0
        y = y + _conv(x2, w[:, cin:], stride2)[:, :, :y.shape[2], :y.shape[3]]
    if b is not None:
        y = y + b[None, :, None, None]
    if res_mode == 1:
        y = y + res
    elif res_mode == 2:
        y = y + upsample_nearest(res, y.shape[2:])
    if relu:
        y = y.clamp_min(0)
    return (nhwc(y),)


def conv3x3_ref(x, w, b=None, relu=False):
    """mcg_conv3x3_wino_x3: 3x3 / stride 1 / pad 1."""
    return conv2d_ref(x, w, b, 1, 1, relu)


def stem_ref(img, w, b):
    """mcg_stem_forward: conv 7x7 / stride 2 / pad 3 + bias + ReLU, then max pool 3x3 / stride 2 / pad 1 (which pads with -inf)."""
    c = (_conv(img, w, 2, 3) + b[None, :, None, None]).clamp_min(0)
    return (nhwc(_integral(F.max_pool2d(c.double(), 3, 2, 1), 'pool')),)


def bneck_ref(x, w2, b2, w3, b3, src2, nsrc, w1n=None, b1n=None):
    """mcg_bottleneck_x3, the three layers of test_fused_bottleneck_tail_f16x3: t = relu(conv2 3x3 (x) + b2);
    y = relu(conv3 1x1 ([t | src2] if nsrc == 2 else t) + b3 (+ src2 if nsrc == 1)); z = relu(conv1 1x1 (y) + b1n) when there is a next
    conv1.  w2 OIHW, w3 [4 cm][cm (+ 64)], w1n [cn][4 cm].  -> (t, y[, z]), NHWC int64."""
    t = (_conv(x, w2, 1, 1) + b2[None, :, None, None]).clamp_min(0)
    a = torch.cat([t, src2], dim=1) if nsrc == 2 else t
    y = _conv(a, w3[:, :, None, None]) + b3[None, :, None, None]
    if nsrc == 1:
        y = y + src2
    y = y.clamp_min(0)
    out = (nhwc(t), nhwc(y))
    if w1n is not None:
        out += (nhwc((_conv(y, w1n[:, :, None, None]) + b1n[None, :, None, None]).clamp_min(0)),)
    return out


# ------------------------------------------------------------------------------------------------ the exactness condition
def check_exactness(fn, what, x3=False, activations=('x', 'x2', 'img'), **kw):
    """Asserts that ``fn(**kw)`` is a case a kernel must reproduce bit for bit: the same operator over absolute values -- whose
    outputs bound every partial sum of every layer, in any order -- stays below 2^24, and for an f16x3 kernel (x3=True) the activation
    inputs and every intermediate layer stay below 2^22.  Returns the largest bound.  A case that fails is rejected, never skipped."""
    layers = fn(**{k: (v.abs() if torch.is_tensor(v) else v) for k, v in kw.items()})
    worst = max(int(t.max()) for t in layers)
    assert worst < LIMIT, f'{what}: sum |x| |w| + |b| + |res| reaches {worst} >= 2^24'
    if x3:
        fed = [kw[k].abs() for k in activations if kw.get(k) is not None] + list(layers[:-1])
        if kw.get('nsrc') is not None:
            fed.append(kw['src2'].abs())
        top = max(int(t.max()) for t in fed)
        assert top < X3_LIMIT, f'{what}: an activation fed to an f16x3 contraction reaches {top} >= 2^22'
    return worst


WINO_AT = {2: [[1, 1, 1, 0], [0, 1, -1, -1]],
           4: [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]}
WINO_BT = {2: [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
           4: [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]}
WINO_UNIT = {2: 2, 4: 1}    # G w is a multiple of 1 / unit: halves for F(2,3) on ternary weights, integers for F(4,3) on 24 x ternary


def wino_transformed_weights(w, g, absolute=False):
    """U = G w along kx in units of 1 / WINO_UNIT[g], in integer arithmetic (24 G is an integer matrix for both forms):
    w [Cout][Cin][3][3] int64 -> [position][Cout][ky][Cin] int64.  Asserts that U is integral in that unit."""
    from mcgaze_amd.packing import WINO_G
    g24 = (torch.tensor(WINO_G[g], dtype=torch.float64) * 24).round().to(torch.int64)
    if absolute:
        g24, w = g24.abs(), w.abs()
    u = torch.einsum('pk,ocyk->poyc', g24, w) * WINO_UNIT[g]
    assert bool((u % 24 == 0).all()), f'G w is not a multiple of 1/{WINO_UNIT[g]} for g = {g}'
    return u // 24


def check_exactness_wino(x, w, b, g, what):
    """The Winograd kernels sum in the transformed domain, where the bound is another one: with U = G w the transformed weights,
    every partial sum is at most rowsum |A^T| * rowsum |B^T| * max |x| * max over (position, output channel) of the sum over
    (ky, channel) of |G| |w| (the textbook matrices for the points 0, +-1, (+-2,) infinity; include/mcgaze_hip.h names the same
    constants).  In the unit that makes U integral that, plus |b|, must stay below 2^24 and the transformed inputs below 2^22; that U
    is exact in fp16 after the power-of-two pre-scale is test_exact_cases_cpu.py's packer test.  Returns the bound."""
    u = wino_transformed_weights(w, g, absolute=True)
    ra = max(sum(abs(v) for v in row) for row in WINO_AT[g])
    rb = max(sum(abs(v) for v in row) for row in WINO_BT[g])
    xmax = int(x.abs().max())
    bound = ra * rb * xmax * int(u.sum(dim=(2, 3)).max()) + (int(b.abs().max()) * WINO_UNIT[g] if b is not None else 0)
    assert bound < LIMIT, f'{what}: the transformed-domain bound reaches {bound} >= 2^24'
    assert rb * xmax < X3_LIMIT, what
    return bound


# ------------------------------------------------------------------------------------------------ expected values, ties, comparison
def expected(ref_int, dtype, frac_bits=0):
    """The value a kernel must store for the int64 reference: the integer itself (f32, f16x3), or ONE round-to-nearest-even of it
    (bf16, fp16) -- applied after bias, residual and ReLU.  frac_bits: the reference is the dyadic fraction ref_int / 2^frac_bits
    (tests/roi_exact_cases.py); a power-of-two scale moves exponents only, and a non-zero value of at least 2^-frac_bits is a normal
    number of every storage type as long as frac_bits <= 14."""
    assert int(ref_int.abs().max()) < LIMIT and 0 <= frac_bits <= 14
    want = ref_int.float() * 2.0 ** -frac_bits
    if dtype in SIG_BITS:
        assert dtype != torch.float16 or int(ref_int.abs().max()) <= 65504 << frac_bits, 'fp16 overflow'
        want = want.to(dtype)
    return want


def _ulp(a, bits):
    """Spacing of the ``bits``-significand format at the positive integers ``a`` (int64; 1 where the format holds every integer)."""
    e = torch.frexp(a.clamp_min(1).double())[1].to(torch.int64) - 1             # floor(log2 a), exact
    return torch.ones_like(a) << (e - (bits - 1)).clamp_min(0)


def count_ties(ref_int, dtype):
    """How many reference integers lie exactly halfway between two ``dtype`` values (bf16: any odd integer in (256, 512), ...)."""
    a = ref_int.abs()
    u = _ulp(a, SIG_BITS[dtype])
    return int(((u > 1) & (a % u == u // 2)).sum())


def count_inexact(ref_int, dtype=torch.float16):
    """How many integers ``dtype`` cannot hold: for fp16, the activations whose f16x3 split has a non-zero low half."""
    a = ref_int.abs()
    return int((a % _ulp(a, SIG_BITS[dtype]) != 0).sum())


def truncated(ref_int, dtype, frac_bits=0):
    """MUTANT of ``expected``: round toward zero instead of to nearest even."""
    a = ref_int.abs()
    return ((ref_int.sign() * (a - a % _ulp(a, SIG_BITS[dtype]))).float() * 2.0 ** -frac_bits).to(dtype)


def assert_exact(got, want, what):
    """Bit equality of the VALUES (torch.equal: -0.0 equals +0.0, NaN equals nothing).  On failure: how many elements differ, the first
    of them as (n, y, x, c), both values there, and the largest absolute difference."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    if torch.equal(got, want):
        return
    g, w = got.double(), want.double()
    bad = ~(g == w)
    first = tuple(bad.nonzero()[0].tolist())
    raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at (n, y, x, c) = {first}: got {float(g[first])!r}, '
                         f'want {float(w[first])!r}; max |d| = {float((g - w).abs().nan_to_num(nan=float("inf")).max()):.6g}')


# ------------------------------------------------------------------------------------------------ the cases
DTYPES = ['f32', 'bf16', 'fp16', 'f16x3']
TORCH_DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16, 'f16x3': torch.float32}
CIN_GRANULE = {'f32': 16, 'bf16': 32, 'fp16': 32, 'f16x3': 32}   # mcg_conv2d: 64-byte K slices (igemm.hip); f16x3: its 32-channel K tile
COUT_GRANULE = {'f32': 4, 'bf16': 8, 'fp16': 8, 'f16x3': 4}      # one 16-byte chunk of outputs
CONV_DENSITY = 0.5

CONV_CASES = {
    # name: (N, H, W, Cin, Cout, k, stride, pad, relu, residual, (Cin2, stride2), activation scale)
    'm1':        (1, 1, 1, 32, 8, 1, 1, 0, False, None, None, 1),        # M = 1, one K step, the smallest Cout
    'c64':       (2, 9, 11, 64, 64, 3, 1, 1, True, None, None, 1),       # conv3x3_c64 (16-bit) and the 256 x 64 tile
    'ragged_s2': (3, 13, 10, 96, 72, 3, 2, 1, False, None, None, 1),     # M = 105 < 128; Cout tail of 72; odd map under stride 2
    'tails':     (1, 17, 16, 320, 136, 1, 1, 0, False, None, None, 1),   # M = 272 = 256 + 16; Cout = 128 + 8
    'taps25':    (1, 7, 5, 32, 40, 5, 1, 2, False, None, None, 1),       # 25 taps; the pad is wider than half the map
    'down':      (2, 8, 8, 256, 512, 1, 2, 0, False, None, None, 1),     # the downsample conv
    'add':       (2, 9, 11, 64, 256, 1, 1, 0, True, 'add', None, 1),     # residual add
    'up':        (2, 9, 11, 512, 256, 1, 1, 0, False, 'up', None, 1),    # residual 4 x 5: nearest upsample onto an odd map
    'cat_s1':    (3, 9, 7, 128, 512, 1, 1, 0, True, None, (256, 1), 1),  # conv3 + downsample as one K-concatenated conv
    'cat_s2':    (3, 9, 7, 128, 512, 1, 1, 0, True, None, (256, 2), 1),
    'deep':      (1, 7, 7, 512, 512, 3, 1, 1, True, None, None, 1),      # K = 4608: the deep-K tiles
    # activations x 16: sums of hundreds to thousands, odd through the bias and the residual -- the 16-bit store rounds, with ties, and
    # a kernel that rounds before it adds the residual (or the bias) shows
    'deep_x16':  (1, 7, 7, 512, 512, 3, 1, 1, True, 'add', None, 16),
    # f16x3 only: activations a * 683, |a| = 3 -> 2049 = 2048 + 1: the activation split has a non-zero LOW half (x 16 alone does not
    # reach fp16's 11 bits at a kernel's INPUT; it does at the chained contractions of the fused tail)
    'tails_wide': (1, 17, 16, 320, 136, 1, 1, 0, False, None, None, 683),
}
CONV_ONLY = {'tails_wide': ('f16x3',)}


def conv_supported(name, kind):
    """False where mcg_conv2d documents the shape as unsupported for this precision (the channel granularity)."""
    c = CONV_CASES[name]
    cins = [c[3]] + ([c[10][0]] if c[10] else [])
    return all(ci % CIN_GRANULE[kind] == 0 for ci in cins) and c[4] % COUT_GRANULE[kind] == 0


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """-> (kwargs of conv2d_ref, its result): int64 tensors, built once per process and shared -- do not write to them."""
    N, H, W, cin, cout, k, stride, pad, relu, resk, cat, scale = CONV_CASES[name]
    g = gen(9000 + list(CONV_CASES).index(name))
    kw = dict(x=acts(g, (N, cin, H, W), scale=scale), stride=stride, pad=pad, relu=relu)
    kw['w'] = ternary(g, (cout, cin + (cat[0] if cat else 0), k, k), CONV_DENSITY)
    kw['b'] = small(g, (cout,))
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if resk == 'add':
        kw.update(res=small(g, (N, cout, ho, wo)), res_mode=1)
    elif resk == 'up':
        kw.update(res=small(g, (N, cout, ho // 2, wo // 2)), res_mode=2)
    if cat:
        kw.update(x2=acts(g, (N, cat[0], H * cat[1], W * cat[1]), post_relu=True), stride2=cat[1])
    return kw, conv2d_ref(**kw)[0]


WINO_DENSITY = 0.5
WINO_CASES = {
    # g: [(N, H, W, Cin, Cout)]
    2: [(1, 4, 8, 32, 128),      # one partly filled tile
        (1, 7, 9, 256, 256),     # odd width: a phantom pixel
        (9, 5, 12, 64, 256),     # many frames in one tile
        (5, 7, 7, 512, 128),     # a tile spans frames
        (2, 13, 30, 32, 256)],
    4: [(7, 9, 16, 32, 128), (3, 16, 20, 96, 256), (2, 28, 28, 64, 128)],
}
WINO_TILES = {2: (0, 1, 2, 3, 4), 4: (0, 1, 2)}     # include/mcgaze_hip.h: tile 4 is valid for g = 2 only
WINO_WSCALE = {2: 1, 4: 24}                         # F(4,3)'s G divides by 4, 6, 12 and 24: weights of 24 x ternary keep G w integral


@functools.lru_cache(maxsize=None)
def wino_case(g, shape):
    """-> (x, w, b, {(bias, relu): reference}) for the two variants every Winograd case runs in: with bias and ReLU, and without both."""
    N, H, W, cin, cout = shape
    rg = gen(9200 + 31 * g + WINO_CASES[g].index(shape))
    x = acts(rg, (N, cin, H, W))
    w = ternary(rg, (cout, cin, 3, 3), WINO_DENSITY) * WINO_WSCALE[g]
    b = small(rg, (cout,))
    return x, w, b, {True: conv3x3_ref(x, w, b, True)[0], False: conv3x3_ref(x, w, None, False)[0]}


STEM_SHAPES = [(1, 32, 32), (2, 64, 96), (1, 36, 52)]    # 36 x 52 -> 9 x 13: not a multiple of the pool's tiles


@functools.lru_cache(maxsize=None)
def stem_case(shape):
    """Integer image, 7x7 weights and bias, all in {-3..3}: |sums| <= 3 * 3 * 147 + 3."""
    N, H, W = shape
    g = gen(9400 + STEM_SHAPES.index(shape))
    kw = dict(img=small(g, (N, 3, H, W)), w=small(g, (64, 3, 7, 7)), b=small(g, (64,)))
    return kw, stem_ref(**kw)[0]


BNECK_COMBOS = [(64, 1, 64), (64, 1, 128), (64, 2, 64), (64, 1, 0), (64, 2, 128), (64, 2, 0), (128, 1, 128), (128, 1, 0)]   # cm, nsrc, cn
BNECK_SHAPES = [(1, 9, 5), (2, 30, 37), (2, 28, 84), (3, 56, 56)]
BNECK_DENSITY = (1 / 4, 1 / 4, 1 / 8)     # conv2, conv3 (+ downsample), the next conv1
BNECK_CASES = [(s, c, 1) for s in BNECK_SHAPES for c in BNECK_COMBOS if s != (3, 56, 56) or c[0] == 64]   # 56 x 56: cm = 64 only
# x scaled by 16: y passes 2048 (t reaches about 1500), so the chained next conv1 splits activations with non-zero low halves; by 64: t
# passes 2048 as well, so conv3 does too
BNECK_SCALED = [((2, 30, 37), (64, 2, 128), 16), ((2, 30, 37), (64, 2, 128), 64)]
BNECK_CASES += BNECK_SCALED


@functools.lru_cache(maxsize=None)
def bneck_case(shape, combo, scale):
    N, H, W = shape
    cm, nsrc, cn = combo
    g = gen(9600 + 97 * BNECK_SHAPES.index(shape) + 7 * BNECK_COMBOS.index(combo) + scale)
    c = 4 * cm
    kw = dict(x=acts(g, (N, cm, H, W), post_relu=True, scale=scale), nsrc=nsrc,
              w2=ternary(g, (cm, cm, 3, 3), BNECK_DENSITY[0]), b2=small(g, (cm,)),
              w3=ternary(g, (c, cm + 64 * (nsrc - 1)), BNECK_DENSITY[1]), b3=small(g, (c,)),
              src2=acts(g, (N, 64 if nsrc == 2 else c, H, W), post_relu=True))
    if cn:
        kw.update(w1n=ternary(g, (cn, c), BNECK_DENSITY[2]), b1n=small(g, (cn,)))
    return kw, bneck_ref(**kw)


LAYOUT_SHAPES = [(1, 1, 1, 1), (2, 3, 1, 7), (3, 37, 5, 9)]


def layout_case(shape):
    """Integers up to 5000 in magnitude: odd ones in (256, 512) are bf16 ties, odd ones in (2048, 4096) fp16 ties."""
    return torch.randint(-5000, 5001, shape, generator=gen(9800 + len(shape) + shape[1]))
