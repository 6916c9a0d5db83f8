"""-m gpu: every C-ABI operator of libmcgaze_hip.so against the oracle (oracle/mcgaze_oracle.py,
plain torch fp32 on the CPU) on the same seeded inputs.

Tolerances (see STAGE_TOL / GAZE_TOL / PYRAMID_TOL below: measured x 1.5): MCG_F32 mode uses f32 MFMA (exact f32 fma chains) -> only summation order differs
from the CPU reference, 1e-4 relative to the tensor's scale.  MCG_BF16 mode rounds operands and
stored activations to bf16 (8 mantissa bits): 2e-2 relative to the tensor's scale per operator.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mcgaze_amd import synth
from oracle import mcgaze_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 2.5e-3}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def scale_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@pytest.fixture(scope='module')
def eng():
    from mcgaze_amd import engine
    return engine


@pytest.fixture(scope='module')
def sd():
    return orc.as_torch(synth.make_state_dict(0))


def test_library_loads_on_gpu(eng):
    import ctypes as C
    from mcgaze_amd import lib as L
    lib = L.load()
    cu, hbm, arch = C.c_int(), C.c_size_t(), C.create_string_buffer(64)
    L.check(lib.mcg_device_info(C.byref(cu), C.byref(hbm), arch, 64), 'mcg_device_info')
    assert arch.value.decode().startswith('gfx950'), arch.value
    assert cu.value == 256 and hbm.value > 200 << 30


CONV_CASES = [
    # N, H, W, Cin, Cout, k, stride, pad, relu, residual
    (2, 14, 14, 64, 64, 1, 1, 0, True, None),
    (2, 14, 14, 64, 64, 3, 1, 1, True, None),
    (3, 10, 12, 256, 128, 1, 1, 0, False, None),
    (2, 12, 12, 128, 128, 3, 2, 1, True, None),
    (2, 8, 8, 256, 512, 1, 2, 0, False, None),
    (5, 7, 7, 512, 2048, 1, 1, 0, True, 'add'),
    (2, 9, 11, 64, 256, 1, 1, 0, True, 'add'),
    (2, 8, 12, 512, 256, 1, 1, 0, False, 'up'),
    (1, 7, 9, 256, 256, 3, 1, 1, False, None),
    (1, 3, 3, 2048, 512, 1, 1, 0, True, None),
]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', CONV_CASES)
def test_conv2d(eng, dtype, case):
    N, H, W, Cin, Cout, k, stride, pad, relu, resk = case
    g = torch.Generator().manual_seed(1000 + CONV_CASES.index(case))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    q = (lambda t: t.to(dtype).float())  # the values the kernel actually sees
    ref = F.conv2d(q(x), q(w), b, stride=stride, padding=pad)
    res = None
    mode = 0
    if resk == 'add':
        res = torch.randn(ref.shape, generator=g)
        ref = ref + q(res)
        mode = 1
    elif resk == 'up':
        res = torch.randn(N, Cout, ref.shape[2] // 2, ref.shape[3] // 2, generator=g)
        ref = ref + F.interpolate(q(res), size=ref.shape[2:], mode='nearest')
        mode = 2
    if relu:
        ref = F.relu(ref)
    dev = 'cuda:0'
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
    y = eng.conv2d(nhwc(x), w.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev), b.to(dev), stride=stride, pad=pad, relu=relu,
                   residual=nhwc(res) if res is not None else None, residual_mode=mode)
    torch.cuda.synchronize()
    assert scale_err(y.permute(0, 3, 1, 2), ref) < TOL[dtype]


X3_TOL = 1.5e-6   # of the tensor's scale (measured <= 8.4e-7): operands carry 22 significant bits (fp16 hi + lo), products lo.hi + hi.lo + hi.hi, f32 accumulate


@pytest.mark.parametrize('case', CONV_CASES)
def test_conv2d_f16x3(eng, case):
    """The MCG_F16X3 contraction (f32 activations, split-packed weights, three fp16 MFMAs per product) against the UNQUANTISED
    f32 convolution: it must sit two orders of magnitude inside the plain bf16 kernel's error."""
    N, H, W, Cin, Cout, k, stride, pad, relu, resk = case
    g = torch.Generator().manual_seed(1000 + CONV_CASES.index(case))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
    res, mode = None, 0
    if resk == 'add':
        res = torch.randn(ref.shape, generator=g)
        ref = ref + res.double()
        mode = 1
    elif resk == 'up':
        res = torch.randn(N, Cout, ref.shape[2] // 2, ref.shape[3] // 2, generator=g)
        ref = ref + F.interpolate(res.double(), size=ref.shape[2:], mode='nearest')
        mode = 2
    if relu:
        ref = F.relu(ref)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to('cuda:0')
    y = eng.conv2d(nhwc(x), nhwc(w), b.to('cuda:0'), stride=stride, pad=pad, relu=relu,
                   residual=nhwc(res) if res is not None else None, residual_mode=mode, split=True)
    torch.cuda.synchronize()
    err = scale_err(y.permute(0, 3, 1, 2), ref.float())
    print(f'f16x3 conv {case}: {err:.2e} of scale')
    assert err < X3_TOL, err


WINO_CASES = [
    # N, H, W, Cin, Cout, relu, bias   (3x3 / stride 1 / pad 1)
    (2, 14, 14, 256, 256, True, True),      # layer3's conv2 / FPN P4
    (1, 7, 9, 256, 256, False, True),       # odd width: the last pair of a row has a phantom pixel
    (3, 28, 28, 64, 128, False, True),      # two blocks per window row, one channel tile column
    (2, 56, 56, 32, 128, True, False),      # four blocks per window row (P2's geometry), no bias
    (5, 7, 7, 512, 512, True, True),        # layer4's conv2: a tile spans several frames (zero rows between them)
    (3, 10, 12, 96, 384, False, True),      # ragged everything
    (1, 4, 8, 32, 128, False, True),        # a single small frame: one partly filled tile
    (9, 5, 12, 64, 256, True, True),        # many small frames in one tile
]


@pytest.mark.parametrize('case', WINO_CASES)
def test_conv3x3_wino_x3(eng, case):
    """wino_x3.hpp (1-D Winograd F(2,3) along x in the f16x3 arithmetic) against the f64 convolution: the same bound as the direct f16x3
    kernel, and within a small factor of that kernel's own error on the same input ("a -m gpu test of the new kernel
    against oracle conv on ragged shapes")."""
    N, H, W, Cin, Cout, relu, has_b = case
    g = torch.Generator().manual_seed(4100 + WINO_CASES.index(case))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) if has_b else None
    ref = F.conv2d(x.double(), w.double(), b.double() if has_b else None, padding=1)
    if relu:
        ref = F.relu(ref)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to('cuda:0')
    y = eng.conv3x3_wino(nhwc(x), nhwc(w), b.to('cuda:0') if has_b else None, relu=relu)
    yd = eng.conv2d(nhwc(x), nhwc(w), b.to('cuda:0') if has_b else None, pad=1, relu=relu, split=True)
    torch.cuda.synchronize()
    err = scale_err(y.permute(0, 3, 1, 2), ref.float())
    err_d = scale_err(yd.permute(0, 3, 1, 2), ref.float())
    print(f'wino f16x3 conv {case}: {err:.2e} of scale (direct f16x3 kernel: {err_d:.2e})')
    assert err < X3_TOL, err
    assert err < 4 * err_d + 2e-7, (err, err_d)


WINO4_CASES = [
    # N, H, W, Cin, Cout, relu, bias   F(4,3): width a multiple of 4, at least 16
    (2, 28, 28, 64, 128, False, True),      # P3's geometry: tiles run over frame boundaries
    (3, 56, 56, 32, 128, True, True),       # P2's geometry: tiles are cut at frame boundaries (a 32 KiB window holds no zero row)
    (3, 16, 20, 96, 256, False, True),      # ragged
    (1, 28, 28, 256, 256, True, False),     # the FPN's channel counts
    (7, 9, 16, 32, 128, False, True),       # many small frames in one tile
]
X3_WINO4_TOL = 3e-6   # of scale; measured <= ~1.5e-6: the F(4,3) constants (x4, x5 in, x8 out) cost about 1.5 bits against the direct kernel


@pytest.mark.parametrize('case', WINO4_CASES)
def test_conv3x3_wino_x3_f43(eng, case):
    """The F(4,3) form of wino_x3.hpp against the f64 convolution, with the direct kernel's and the F(2,3) kernel's errors beside it."""
    N, H, W, Cin, Cout, relu, has_b = case
    g = torch.Generator().manual_seed(4400 + WINO4_CASES.index(case))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(Cin * 9)
    b = torch.randn(Cout, generator=g) if has_b else None
    ref = F.conv2d(x.double(), w.double(), b.double() if has_b else None, padding=1)
    if relu:
        ref = F.relu(ref)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to('cuda:0')
    bd = b.to('cuda:0') if has_b else None
    y4 = eng.conv3x3_wino(nhwc(x), nhwc(w), bd, relu=relu, g=4)
    y2 = eng.conv3x3_wino(nhwc(x), nhwc(w), bd, relu=relu, g=2)
    yd = eng.conv2d(nhwc(x), nhwc(w), bd, pad=1, relu=relu, split=True)
    torch.cuda.synchronize()
    e4, e2, ed = (scale_err(t.permute(0, 3, 1, 2), ref.float()) for t in (y4, y2, yd))
    print(f'F(4,3) {case}: {e4:.2e} of scale (F(2,3) {e2:.2e}, direct {ed:.2e})')
    assert e4 < X3_WINO4_TOL, e4
    for t in (1, 2):   # both tile shapes: the same bits
        assert torch.equal(y4, eng.conv3x3_wino(nhwc(x), nhwc(w), bd, relu=relu, g=4, tile=t))


def test_conv3x3_wino_x3_f43_is_batch_invariant(eng):
    g = torch.Generator().manual_seed(4500)
    x = torch.randn(5, 56, 56, 64, generator=g).to('cuda:0')
    w = (torch.randn(128, 3, 3, 64, generator=g) / 24).to('cuda:0')
    b = torch.randn(128, generator=g).to('cuda:0')
    y5 = eng.conv3x3_wino(x, w, b, relu=True, g=4)
    y2 = eng.conv3x3_wino(x[1:3].contiguous(), w, b, relu=True, g=4)
    torch.cuda.synchronize()
    assert torch.equal(y5[1:3], y2)


def test_conv3x3_wino_x3_is_batch_invariant(eng):
    """A frame's result must not depend on the batch it came in (tile boundaries move with the batch): frames 0..2 of a 5-frame call equal
    a 3-frame call bit for bit."""
    g = torch.Generator().manual_seed(4200)
    x = torch.randn(5, 14, 14, 256, generator=g).to('cuda:0')
    w = (torch.randn(256, 3, 3, 256, generator=g) / 48).to('cuda:0')
    b = torch.randn(256, generator=g).to('cuda:0')
    y5 = eng.conv3x3_wino(x, w, b, relu=True)
    y3 = eng.conv3x3_wino(x[:3].contiguous(), w, b, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(y5[:3], y3)


@pytest.mark.parametrize('shape', [(7, 14, 14, 256, 256), (3, 9, 11, 64, 128), (2, 28, 28, 32, 256), (3, 56, 56, 64, 128), (5, 7, 7, 512, 128), (2, 13, 30, 32, 256)])
def test_conv3x3_wino_x3_tiles_are_bit_identical(eng, shape):
    """The workgroup tiles of wino_x3.hpp (128 x 128 on eight waves, 64 x 64, 32 x 64, and round 5's 128 x 128 with one wave per SIMD and
    the weight fragments straight from global memory) walk K in the same order and apply the same output transform: same bits, so the tile
    the launcher picks from the grid size (i.e. from the batch) never shows in a result."""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(4300 + N)
    x = torch.randn(N, H, W, Cin, generator=g).to('cuda:0')
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5).to('cuda:0')
    b = torch.randn(Cout, generator=g).to('cuda:0')
    ys = [eng.conv3x3_wino(x, w, b, relu=True, tile=t) for t in (1, 2, 3, 4, 0)]
    torch.cuda.synchronize()
    for y in ys[1:]:
        assert torch.equal(ys[0], y)


def test_conv3x3_wino_x3_rejects_what_it_cannot_tile(eng):
    from mcgaze_amd import lib as L
    x = torch.zeros(1, 8, 112, 32, device='cuda:0')
    w = torch.zeros(128, 3, 3, 32, device='cuda:0')
    with pytest.raises(L.McgError, match='unsupported shape'):
        eng.conv3x3_wino(x, w)


@pytest.mark.parametrize('wscale', [1e2, 1.0, 1e-2, 1e-3, 1e-4])
def test_f16x3_small_weights(eng, wscale):
    """VERDICT r3 item 5a.  A weight below 0.125 has its fp16 LOW half in the subnormal range (absolute error 2^-25): unscaled, a matrix of
    ~1e-3 weights (a BN fold with a small gamma / sigma ratio) keeps ~15 bits.  The packers therefore pre-scale every trunk matrix by a
    power of two (packing.pow2_prescale: max |w| into (2^13, 2^14]) and the kernels multiply the f32 sums back (mcg_conv_desc.wscale,
    exact): the error against the f64 product must be the 22-bit one -- the same few 1e-7 of scale -- for weight scales 1e-4 .. 1e2.
    The unscaled path (prescale=False) is measured beside it and must show the loss it is there to remove."""
    g = torch.Generator().manual_seed(99)
    N, H, W, Cin, Cout = 2, 12, 12, 256, 256
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) * wscale
    ref = F.conv2d(x.double(), w.double())
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to('cuda:0')
    y = eng.conv2d(nhwc(x), nhwc(w), None, split=True)
    y_raw = eng.conv2d(nhwc(x), nhwc(w), None, split=True, prescale=False)
    torch.cuda.synchronize()
    err = scale_err(y.permute(0, 3, 1, 2), ref.float())
    err_raw = scale_err(y_raw.permute(0, 3, 1, 2), ref.float())
    print(f'f16x3 1x1 conv, weights ~{wscale:g}: {err:.2e} of scale pre-scaled, {err_raw:.2e} unscaled')
    assert err < 6e-7, (wscale, err)                        # the 22-bit operand error over K = 256 (measured 3.4 - 4.9e-7), whatever the weights' magnitude
    if wscale <= 1e-3:
        assert err_raw > 2 * err, (wscale, err, err_raw)    # measured in round 3: 1e-3 -> 4e-6


@pytest.mark.parametrize('xscale', [1e2, 1.0, 1e-1])
def test_f16x3_activation_magnitudes(eng, xscale):
    """The ACTIVATION side of the same question (tools/lab/act_scale_probe.py).  An activation below 0.125 has its fp16 low half in the subnormal
    range -- an ABSOLUTE error of 2^-25, harmless while the tensor as a whole is O(0.1) or larger (every trunk tensor of both synthetic
    weight families: per-layer median |x| 0.17 .. 8.5), not harmless for a tensor that is small as a whole: measured 3.3e-6 of
    scale at |x| ~ 1e-2, 4e-5 at 1e-3 (the f32 kernel: 5e-7 throughout).  Activations are not pre-scaled (a per-tensor scale would make a
    clip's bits depend on the batch it came in); the 22-bit product is asserted for tensors of magnitude 0.1 .. 100."""
    g = torch.Generator().manual_seed(98)
    N, H, W, Cin, Cout = 2, 12, 12, 256, 256
    x = torch.randn(N, Cin, H, W, generator=g).relu() * xscale
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / 16
    ref = F.conv2d(x.double(), w.double())
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to('cuda:0')
    y = eng.conv2d(nhwc(x), nhwc(w), None, split=True)
    torch.cuda.synchronize()
    err = scale_err(y.permute(0, 3, 1, 2), ref.float())
    print(f'f16x3 1x1 conv, activations ~{xscale:g}: {err:.2e} of scale')
    assert err < 8e-7, (xscale, err)


def test_conv2d_f16x3_randomized_shapes(eng):
    """The randomized sweep of test_conv2d_randomized_shapes for the f16x3 kernel (channel counts are multiples of 32: its K tile)."""
    rs = np.random.RandomState(4048)
    for trial in range(30):
        k = int(rs.choice([1, 1, 3, 3, 5]))
        stride = int(rs.choice([1, 1, 2]))
        pad = int(rs.choice([0, k // 2])) if k > 1 else 0
        cin = int(rs.choice([32, 64, 96, 128, 256, 320]))
        cout = int(rs.choice([32, 64, 72, 128, 256, 640]))
        N = int(rs.randint(1, 5))
        H, W = int(rs.randint(max(k, 1), 23)), int(rs.randint(max(k, 1), 23))
        relu = bool(rs.randint(2))
        g = torch.Generator().manual_seed(7000 + trial)
        x = torch.randn(N, cin, H, W, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
        b = torch.randn(cout, generator=g)
        ref = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
        mode, res = int(rs.randint(3)), None
        if mode == 1:
            res = torch.randn(ref.shape, generator=g)
            ref = ref + res.double()
        elif mode == 2:
            hr, wr = max(ref.shape[2] // 2, 1), max(ref.shape[3] // 2, 1)
            res = torch.randn(N, cout, hr, wr, generator=g)
            ref = ref + F.interpolate(res.double(), size=ref.shape[2:], mode='nearest')
        if relu:
            ref = F.relu(ref)
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to('cuda:0')
        y = eng.conv2d(nhwc(x), nhwc(w), b.to('cuda:0'), stride=stride, pad=pad, relu=relu,
                       residual=nhwc(res) if res is not None else None, residual_mode=mode, split=True)
        torch.cuda.synchronize()
        err = scale_err(y.permute(0, 3, 1, 2), ref.float())
        assert err < X3_TOL, (trial, (N, H, W, cin, cout, k, stride, pad, relu, mode), err)


@pytest.mark.parametrize('stride2', [1, 2])
def test_conv3_plus_downsample_f16x3(eng, stride2):
    g = torch.Generator().manual_seed(177 + stride2)
    N, Ho, Wo, planes, inpl, cout = 3, 9, 7, 128, 256, 512
    o2 = torch.randn(N, planes, Ho, Wo, generator=g)
    x = torch.randn(N, inpl, Ho * stride2, Wo * stride2, generator=g)
    w3 = torch.randn(cout, planes, 1, 1, generator=g) / planes ** 0.5
    wd = torch.randn(cout, inpl, 1, 1, generator=g) / inpl ** 0.5
    b = torch.randn(cout, generator=g)
    ref = F.relu(F.conv2d(o2.double(), w3.double()) + F.conv2d(x.double(), wd.double(), stride=stride2) + b.double()[None, :, None, None])
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to('cuda:0')
    wcat = torch.cat([w3, wd], dim=1).permute(0, 2, 3, 1).contiguous().to('cuda:0')
    y = eng.conv2d(nhwc(o2), wcat, b.to('cuda:0'), relu=True, x2=nhwc(x), stride2=stride2, split=True)
    torch.cuda.synchronize()
    assert scale_err(y.permute(0, 3, 1, 2), ref.float()) < X3_TOL


@pytest.mark.parametrize('dtype', DTYPES)
def test_conv2d_randomized_shapes(eng, dtype):
    """Seeded sweep over the contraction kernel's paths: ragged row / channel tiles, 1x1 / 3x3 / 5x5 taps, stride 1-2, padding 0-2,
    channel counts from 32 to 640, every residual mode, single-pixel maps and row counts below one tile."""
    rs = np.random.RandomState(2024)
    dev = 'cuda:0'
    for trial in range(36):
        k = int(rs.choice([1, 1, 3, 3, 5]))
        stride = int(rs.choice([1, 1, 2]))
        pad = int(rs.choice([0, k // 2])) if k > 1 else 0
        cin = int(rs.choice([32, 64, 96, 128, 256, 320]))
        cout = int(rs.choice([32, 64, 72, 128, 256, 640]))
        N = int(rs.randint(1, 5))
        H, W = int(rs.randint(max(k, 1), 23)), int(rs.randint(max(k, 1), 23))
        relu = bool(rs.randint(2))
        g = torch.Generator().manual_seed(5000 + trial)
        x = torch.randn(N, cin, H, W, generator=g)
        w = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
        b = torch.randn(cout, generator=g)
        q = (lambda t: t.to(dtype).float())
        ref = F.conv2d(q(x), q(w), b, stride=stride, padding=pad)
        mode, res = int(rs.randint(3)), None
        if mode == 1:
            res = torch.randn(ref.shape, generator=g)
            ref = ref + q(res)
        elif mode == 2:
            hr, wr = max(ref.shape[2] // 2, 1), max(ref.shape[3] // 2, 1)
            res = torch.randn(N, cout, hr, wr, generator=g)
            ref = ref + F.interpolate(q(res), size=ref.shape[2:], mode='nearest')
        if relu:
            ref = F.relu(ref)
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)
        y = eng.conv2d(nhwc(x), w.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev), b.to(dev), stride=stride, pad=pad, relu=relu,
                       residual=nhwc(res) if res is not None else None, residual_mode=mode)
        torch.cuda.synchronize()
        err = scale_err(y.permute(0, 3, 1, 2), ref)
        assert err < TOL[dtype], (trial, (N, H, W, cin, cout, k, stride, pad, relu, mode), err)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stride2', [1, 2])
def test_conv3_plus_downsample_as_one_k_concatenated_conv(eng, dtype, stride2):
    """relu(conv3(o2) + downsample(x)) (resnet.py:289-298, res_layer.py:51-61) == one 1x1 conv over [o2 | x@stride]."""
    g = torch.Generator().manual_seed(77 + stride2)
    N, Ho, Wo, planes, inpl, cout = 3, 9, 7, 128, 256, 512
    o2 = torch.randn(N, planes, Ho, Wo, generator=g)
    x = torch.randn(N, inpl, Ho * stride2, Wo * stride2, generator=g)
    w3 = torch.randn(cout, planes, 1, 1, generator=g) / planes ** 0.5
    wd = torch.randn(cout, inpl, 1, 1, generator=g) / inpl ** 0.5
    b = torch.randn(cout, generator=g)
    q = lambda t: t.to(dtype).float()
    ref = F.relu(F.conv2d(q(o2), q(w3)) + F.conv2d(q(x), q(wd), stride=stride2) + b[None, :, None, None])
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dtype).to('cuda:0')
    wcat = torch.cat([w3, wd], dim=1).permute(0, 2, 3, 1).contiguous().to(dtype).to('cuda:0')
    y = eng.conv2d(nhwc(o2), wcat, b.to('cuda:0'), relu=True, x2=nhwc(x), stride2=stride2)
    torch.cuda.synchronize()
    assert scale_err(y.permute(0, 3, 1, 2), ref) < TOL[dtype]


@pytest.mark.parametrize('dtype', DTYPES)
def test_layout_roundtrip(eng, dtype):
    x = torch.randn(3, 37, 5, 9).to('cuda:0')
    y = eng.to_nhwc(x, dtype)
    assert torch.equal(y.float().cpu(), x.permute(0, 2, 3, 1).to(dtype).float().cpu())
    assert torch.equal(eng.to_nchw(y).cpu(), x.to(dtype).float().cpu())


@pytest.mark.parametrize('dtype', DTYPES)
def test_stem(eng, sd, dtype):
    from mcgaze_amd.packing import PackedWeights
    pw = PackedWeights(sd, dtype=dtype)
    img = torch.from_numpy(synth.make_clips(3, 1, 2, 64, 96))
    ref = F.relu(orc._bn(sd, 'backbone.bn1', F.conv2d(img, sd['backbone.conv1.weight'], stride=2, padding=3)))
    ref = F.max_pool2d(ref, 3, 2, 1)
    y = eng.stem(img.to('cuda:0'), pw.stem['w'], pw.stem['bias'], dtype)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (2, 16, 24, 64)
    assert scale_err(y.permute(0, 3, 1, 2), ref) < TOL[dtype]


@pytest.mark.parametrize('shape', [(21, 14, 14, 256, 256, 3, 1, 1), (3, 28, 28, 128, 512, 1, 1, 0), (2, 30, 22, 64, 256, 3, 2, 1)])
def test_every_dma_tile_is_bit_identical(eng, shape):
    """All tile shapes of igemm_dma_kernel walk K in the same order, so their outputs must agree bit for bit -- which also
    catches tiling bugs a tolerance hides (a ragged last epilogue pass once wrote stale rows into the next tile)."""
    n, h, w, cin, cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(17)
    x = torch.randn(n, h, w, cin, generator=g).to(torch.bfloat16).to('cuda:0')
    wt = (torch.randn(cout, k, k, cin, generator=g) / (cin * k * k) ** 0.5).to(torch.bfloat16).to('cuda:0')
    b = torch.randn(cout, generator=g).to('cuda:0')
    ho = (h + 2 * pad - k) // stride + 1
    r = torch.randn(n, ho, (w + 2 * pad - k) // stride + 1, cout, generator=g).to(torch.bfloat16).to('cuda:0')
    outs = {}
    for tile in (9, 11, 12, 14, 15):   # every tile the heuristic can choose (igemm.hip), forced through mcg_conv_desc.tile
        outs[tile] = eng.conv2d(x, wt, b, stride=stride, pad=pad, relu=True, residual=r, residual_mode=1, tile=tile).clone()
    from mcgaze_amd import lib as L
    outs['staged'] = eng.conv2d(x, wt, b, stride=stride, pad=pad, relu=True, residual=r, residual_mode=1, flags=L.FLAG_STAGED_GEMM).clone()
    torch.cuda.synchronize()
    for tile, y in outs.items():
        assert torch.equal(y.view(torch.int16), outs[9].view(torch.int16)), tile


@pytest.mark.parametrize('shape', [(7, 14, 14, 256, 256, 3, 1, 1), (3, 28, 28, 128, 512, 1, 1, 0), (2, 30, 22, 64, 256, 3, 2, 1), (7, 7, 7, 512, 512, 3, 1, 1)])
def test_every_x3_tile_is_bit_identical(eng, shape):
    """The f16x3 tiles (50: 256 x 256; 51: 128 x 128, two stages; 53: 128 x 128 with the four-stage ring chosen for grids of at most one
    workgroup per CU -- a single clip's layer3 / layer4) walk K in the same order: bit-identical outputs, so the tile choice (which depends
    on the batch) can never show in a result."""
    n, h, w, cin, cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(19)
    x = torch.randn(n, h, w, cin, generator=g).to('cuda:0')
    wt = (torch.randn(cout, k, k, cin, generator=g) / (cin * k * k) ** 0.5).to('cuda:0')
    b = torch.randn(cout, generator=g).to('cuda:0')
    ho = (h + 2 * pad - k) // stride + 1
    r = torch.randn(n, ho, (w + 2 * pad - k) // stride + 1, cout, generator=g).to('cuda:0')
    outs = {}
    for tile in (0, 50, 51, 53):       # 0: the heuristic's choice
        outs[tile] = eng.conv2d(x, wt, b, stride=stride, pad=pad, relu=True, residual=r, residual_mode=1, tile=tile, split=True).clone()
    torch.cuda.synchronize()
    for tile, y in outs.items():
        assert torch.equal(y.view(torch.int32), outs[50].view(torch.int32)), tile


def test_fused_bottleneck_tail_is_deterministic_under_contention(eng):
    """bneck_x3.hpp's ring protocol under a busy device (profiles/r03_x_lds_war.md): while a second thread runs another engine's forwards on
    its own stream, 1500 launches of the layer1 identity-block tail must reproduce the quiet launch bit for bit.  (Before the fix --
    LDS reads left in flight across the barrier behind which the loader refills their ring slot -- about one launch in 200 did not.)"""
    import threading
    from mcgaze_amd import engine as E, synth
    from mcgaze_amd.packing import bneck_stream
    g = torch.Generator().manual_seed(1)
    cm, cn, N, H, W = 64, 64, 70, 56, 56
    w2 = torch.randn(cm, 3, 3, cm, generator=g) / (9 * cm / 2) ** 0.5
    w3 = torch.randn(4 * cm, cm, generator=g) / 8
    w1 = torch.randn(cn, 4 * cm, generator=g) / 11
    ws, bs = bneck_stream(w2, torch.randn(cm, generator=g) * 0.1, w3, torch.randn(4 * cm, generator=g) * 0.1, w1, torch.randn(cn, generator=g) * 0.1)
    ws, bs = ws.cuda(), bs.cuda()
    x = torch.randn(N, H, W, cm, generator=g).relu_().cuda()
    res = torch.randn(N, H, W, 4 * cm, generator=g).relu_().cuda()
    ref = [t.clone() for t in E.bottleneck_x3(x, res, ws, bs, cn, 1)]
    torch.cuda.synchronize()
    stop, started = [False], threading.Event()

    def noise():
        other = E.HipEngine(synth.make_state_dict(0), precision='f16x3')
        img = torch.from_numpy(synth.make_clips(7, 10, 7)).cuda()
        s2 = torch.cuda.Stream()
        with torch.cuda.stream(s2):
            while not stop[0]:
                other.forward(img, 7)
                s2.synchronize()
                started.set()
    th = threading.Thread(target=noise)
    th.start()
    try:
        assert started.wait(120)
        s = torch.cuda.Stream()
        bad = 0
        with torch.cuda.stream(s):
            for _ in range(1500):
                out = E.bottleneck_x3(x, res, ws, bs, cn, 1)
                s.synchronize()
                bad += int(not (torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])))
    finally:
        stop[0] = True
        th.join()
    assert bad == 0, f'{bad} of 1500 launches differ from the quiet launch'


BNECK_TOL = 4e-6   # of the tensor's scale: three chained f16x3 contractions (X3_TOL each) -- measured <= 1.2e-6


@pytest.mark.parametrize('cm,nsrc,cn', [(64, 1, 64), (64, 1, 128), (64, 2, 64), (64, 1, 0), (64, 2, 128), (64, 2, 0), (128, 1, 128), (128, 1, 0)])
@pytest.mark.parametrize('shape', [(3, 56, 56), (2, 28, 84), (1, 9, 5), (2, 30, 37), (5, 28, 28)])
def test_fused_bottleneck_tail_f16x3(eng, shape, cm, nsrc, cn):
    """bneck_x3.hpp (conv2 3x3 -> conv3 1x1 (+ downsample source | + residual) -> next conv1 1x1 in one kernel, the three contractions
    chained in registers) against the f64 statement of the same three layers (resnet.py:263-302), on tile-aligned maps (56x56 = 7 x 2
    tiles), ragged ones (9x5, 30x37: masked pixels, partial windows) and several frames per launch (persistent grid)."""
    from mcgaze_amd.packing import bneck_stream
    N, H, W = shape
    g = torch.Generator().manual_seed(300 + 7 * nsrc + cn + H + cm)
    c = 4 * cm                                                             # block output channels (256 / 512)
    x = torch.randn(N, cm, H, W, generator=g).relu()                      # conv1's output is post-ReLU
    w2 = torch.randn(cm, cm, 3, 3, generator=g) / np.sqrt(9 * cm / 2)
    b2 = torch.randn(cm, generator=g) * 0.1
    k3 = cm + 64 * (nsrc - 1)                                              # conv3's K: t (+ the downsample conv's 64-channel input)
    w3 = torch.randn(c, k3, generator=g) / np.sqrt(k3)
    b3 = torch.randn(c, generator=g) * 0.1
    src2 = torch.randn(N, 64 if nsrc == 2 else c, H, W, generator=g).relu()
    w1n = torch.randn(cn, c, generator=g) / np.sqrt(c / 2) if cn else None
    b1n = torch.randn(cn, generator=g) * 0.1 if cn else None
    t = F.relu(F.conv2d(x.double(), w2.double(), b2.double(), padding=1))
    a = torch.cat([t, src2.double()], dim=1) if nsrc == 2 else t
    y = F.conv2d(a, w3.double()[:, :, None, None], b3.double())
    if nsrc == 1:
        y = y + src2.double()
    y = F.relu(y)
    z = F.relu(F.conv2d(y, w1n.double()[:, :, None, None], b1n.double())) if cn else None
    ws, bs = bneck_stream(w2.permute(0, 2, 3, 1).contiguous(), b2, w3, b3, w1n, b1n)
    nhwc = lambda v: v.permute(0, 2, 3, 1).contiguous().to('cuda:0')
    gy, gz = eng.bottleneck_x3(nhwc(x), nhwc(src2), ws.to('cuda:0'), bs.to('cuda:0'), cn, nsrc)
    torch.cuda.synchronize()
    ey = scale_err(gy.permute(0, 3, 1, 2), y.float())
    ez = scale_err(gz.permute(0, 3, 1, 2), z.float()) if cn else 0.0
    assert gy.shape[-1] == c and x.shape[1] == cm
    print(f'fused bottleneck tail {shape} cm={cm} nsrc={nsrc} cn={cn}: y {ey:.2e}, z {ez:.2e} of scale')
    assert ey < BNECK_TOL and ez < BNECK_TOL, (ey, ez)


@pytest.mark.parametrize('shape', [(3, 56, 56), (2, 28, 84), (1, 9, 5), (2, 80, 112)])
@pytest.mark.parametrize('relu', [True, False])
def test_conv3x3_c64_is_bit_identical_to_the_generic_kernel(eng, shape, relu):
    """conv3x3_c64.hpp (layer1's conv2: input window staged once, taps by address) keeps the generic kernel's K order: same bits,
    incl. maps that are not a multiple of its 8 x 28 tile and maps smaller than one tile."""
    n, h, w = shape
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, h, w, 64, generator=g).to(torch.bfloat16).to('cuda:0')
    wt = (torch.randn(64, 3, 3, 64, generator=g) / 24.0).to(torch.bfloat16).to('cuda:0')
    b = torch.randn(64, generator=g).to('cuda:0')
    from mcgaze_amd import lib as L
    a = eng.conv2d(x, wt, b, stride=1, pad=1, relu=relu, flags=L.FLAG_NO_SPECIALISED).clone()
    c = eng.conv2d(x, wt, b, stride=1, pad=1, relu=relu)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))


@pytest.mark.parametrize('shape', [(2, 64, 96), (3, 224, 224), (1, 320, 448), (2, 36, 52)])
def test_fused_stem_is_bit_identical_to_the_three_kernel_path(eng, sd, shape):
    """stem_fused.hpp keeps the unfused path's packing and K order, so not even rounding may differ -- incl. sizes whose
    pooled map is not a multiple of the 8x8 tile (36x52 -> 9x13)."""
    from mcgaze_amd.packing import PackedWeights
    pw = PackedWeights(sd, dtype=torch.bfloat16)
    n, h, w = shape
    img = torch.from_numpy(synth.make_clips(7, 1, n, h, w)).to('cuda:0')
    from mcgaze_amd import lib as L
    a = eng.stem(img, pw.stem['w'], pw.stem['bias'], torch.bfloat16, flags=L.FLAG_NO_SPECIALISED).clone()
    b = eng.stem(img, pw.stem['w'], pw.stem['bias'], torch.bfloat16)
    torch.cuda.synchronize()
    assert a.shape == b.shape == (n, h // 4, w // 4, 64)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    # the f16x3 form (f32 activations, split-packed weights, 8 x 4 pooled tiles: 36x52 -> 9x13 is ragged in both directions)
    px = PackedWeights(sd, dtype=torch.float32, split=True)
    a = eng.stem(img, px.stem['w'], px.stem['bias'], torch.float32, flags=L.FLAG_NO_SPECIALISED, split=True).clone()
    b = eng.stem(img, px.stem['w'], px.stem['bias'], torch.float32, split=True)
    torch.cuda.synchronize()
    assert a.shape == b.shape == (n, h // 4, w // 4, 64) and torch.equal(a, b)


@pytest.mark.parametrize('dtype', DTYPES)
def test_roi_align_all_levels(eng, dtype):
    """Random features and generic boxes on all four levels, within 1e-5 (f32) / 1e-2 (16-bit) of the tensor's scale; the test of the
    16-bit rounding (and of every edge, bit for bit) is tests/test_gpu_roi_exact.py."""
    g = torch.Generator().manual_seed(5)
    N = 3
    feats = [torch.randn(N, 256, 64 >> i, 96 >> i, generator=g) for i in range(4)]  # a 256x384 frame
    boxes = torch.tensor([[[10., 12., 60., 70.], [30., 20., 180., 150.], [0., 0., 384., 256.]],
                          [[-20., -15., 500., 400.], [100., 100., 101., 101.], [300., 200., 420., 300.]],
                          [[5.5, 7.25, 250.75, 201.5], [150., 40., 380., 250.], [-300., -300., -200., -200.]]])
    q = lambda t: t.to(dtype).float()
    ref = orc.roi_extract([q(f) for f in feats], boxes)  # [R,256,7,7]
    ref_lv = orc.map_roi_levels(boxes.reshape(-1, 4))
    assert set(ref_lv.tolist()) == {0, 1, 2, 3}
    out, lv = eng.roi_align([f.permute(0, 2, 3, 1).contiguous().to(dtype).to('cuda:0') for f in feats], boxes.to('cuda:0'))
    torch.cuda.synchronize()
    assert lv.cpu().tolist() == ref_lv.tolist()
    got = out.float().cpu().reshape(-1, 7, 7, 256).permute(0, 3, 1, 2)
    assert scale_err(got, ref) < (1e-5 if dtype == torch.float32 else 1e-2)
    assert float(got[-1].abs().max()) == 0.0  # a box entirely outside the map samples zeros


def _affine_pyramid(H0, W0, channels=256):
    """P2..P5 of a (4 H0) x (4 W0) frame, level l = base 10000 l + affine map (tests/roi_align_pins.py), NHWC f32 on the device."""
    from tests import roi_align_pins as P
    lv = []
    for l in range(4):
        m = P.affine_map(H0 >> l, W0 >> l, base=10000.0 * l, channels=1)[0, 0]           # [H, W]
        lv.append(torch.from_numpy(m)[None, :, :, None].repeat(1, 1, 1, channels).contiguous().to('cuda:0'))
    return lv


def test_roi_align_hip_against_independent_pins(eng):
    """The HIP RoIAlign kernel itself (f32) against the pins derived from the published mmcv kernel (tests/roi_align_pins.py):
    every enumerated edge case on an affine map in closed form, the hand-worked non-affine numbers, and the level routing at
    exactly 112 / 224 / 448 px (the level is visible in the sampled values: each pyramid level carries its own offset)."""
    from tests import roi_align_pins as P
    H0 = W0 = 16
    pyr = _affine_pyramid(H0, W0, channels=8)
    boxes = torch.tensor([b for _, b in P.EDGE_BOXES])[None]                      # one frame, 12 boxes, all < 112 px -> level 0
    out, lv = eng.roi_align(pyr, boxes.to('cuda:0'))
    torch.cuda.synchronize()
    assert lv.cpu().tolist() == [0] * len(P.EDGE_BOXES)
    got = out.cpu().reshape(len(P.EDGE_BOXES), 7, 7, 8)
    for i, (name, box) in enumerate(P.EDGE_BOXES):
        want = P.expected_affine(box, 4, H0, W0)[0]
        np.testing.assert_allclose(got[i, :, :, 0].numpy(), want, rtol=0, atol=2e-4, err_msg=name)
        assert torch.allclose(got[i, :, :, 0], got[i, :, :, 7], rtol=1e-6, atol=1e-6)   # every channel carries the same map
    # level routing at the exact boundaries; a 2048 x 2048 frame so that every box lies inside its level's map
    pyr = _affine_pyramid(512, 512, channels=8)
    boxes = torch.tensor([b for b, _ in P.LEVEL_EDGE_BOXES])[None]
    out, lv = eng.roi_align(pyr, boxes.to('cuda:0'))
    torch.cuda.synchronize()
    assert lv.cpu().tolist() == [l for _, l in P.LEVEL_EDGE_BOXES]
    got = out.cpu().reshape(len(P.LEVEL_EDGE_BOXES), 7, 7, 8)
    for i, (box, l) in enumerate(P.LEVEL_EDGE_BOXES):
        want = P.expected_affine(box, 4 << l, 512 >> l, 512 >> l, base=10000.0 * l)[0]
        np.testing.assert_allclose(got[i, :, :, 0].numpy(), want, rtol=0, atol=5e-3, err_msg=str(box))   # 3e4-sized values in f32
    # hand-worked non-affine numbers
    sq = torch.from_numpy(P.SQUARE_MAP[0, 0])[None, :, :, None].repeat(1, 1, 1, 8).contiguous().to('cuda:0')
    pyr = [sq] + [torch.zeros(1, 4 >> i or 1, 4 >> i or 1, 8, device='cuda:0') for i in (1, 2, 3)]
    out, _ = eng.roi_align(pyr, torch.tensor([[P.SQUARE_BOX]]).to('cuda:0'))
    got = out.cpu().reshape(7, 7, 8)
    for (ph, pw), v in P.SQUARE_HAND.items():
        assert abs(float(got[ph, pw, 0]) - v) < 1e-5, ((ph, pw), float(got[ph, pw, 0]), v)


def test_roi_align_hip_equals_scalar_statement(eng):
    """The HIP kernel DIRECTLY against the scalar loop form of the published definition (oracle.roi_align_scalar, f32 arithmetic in
    the kernel's order), on random features: random boxes that leave the map, the enumerated edge boxes scaled to every level,
    zero-area and inverted boxes.  f32 on both sides; what separates them is fused multiply-add contraction in the sample
    coordinates (hipcc contracts `start + ph * bin + ...`, as nvcc does for the original): a coordinate near 50 moves by an ulp
    (4e-6) and a unit-variance map has gradients of ~2 per pixel -> agreement to ~1e-5; measured 8.9e-6."""
    from tests import roi_align_pins as P
    rs = np.random.RandomState(11)
    N, C = 2, 16
    H0, W0 = 40, 56                                  # a 160 x 224 frame
    feats = [rs.standard_normal((N, C, H0 >> i, W0 >> i)).astype(np.float32) for i in range(4)]
    boxes = []
    for scale in (1.0, 2.5, 5.0, 9.0):               # the edge boxes blown up so that they land on every level
        for _, b in P.EDGE_BOXES:
            boxes.append([v * scale for v in b])
    xy = rs.uniform(-60, 230, size=(40, 2)); wh = rs.uniform(0, 500, size=(40, 2)) * rs.choice([1, 1, 1, -0.2], size=(40, 1))
    boxes += np.concatenate([xy, xy + wh], axis=1).tolist()
    while len(boxes) % N:
        boxes.append([0., 0., 10., 10.])
    bt = torch.tensor(boxes, dtype=torch.float32).reshape(N, -1, 4)
    out, lv = eng.roi_align([torch.from_numpy(f).permute(0, 2, 3, 1).contiguous().to('cuda:0') for f in feats], bt.to('cuda:0'))
    torch.cuda.synchronize()
    ref_lv = orc.map_roi_levels(bt.reshape(-1, 4))
    assert lv.cpu().tolist() == ref_lv.tolist() and set(ref_lv.tolist()) == {0, 1, 2, 3}
    P_ = bt.shape[1]
    got = out.cpu().reshape(-1, 7, 7, C).permute(0, 3, 1, 2).numpy()
    worst = 0.0
    for r in range(bt.shape[0] * P_):
        l = int(ref_lv[r])
        roi = np.array([[r // P_, *bt.reshape(-1, 4)[r].tolist()]], dtype=np.float32)
        want = orc.roi_align_scalar(feats[l], roi, 1.0 / (4 << l))[0]
        worst = max(worst, float(np.abs(got[r] - want).max()))
    print(f'HIP RoIAlign vs scalar statement: max |d| = {worst:.2e} on unit-variance features')
    assert worst < 2e-5


KINDS = ['fp32', 'f16x3', 'bf16', 'f16']   # engine kinds of the whole-operator tests below ('f16': MCG_F16, round 6)
KIND_DTYPE = {'fp32': torch.float32, 'f16x3': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
# Per-operator bounds as a fraction of the tensor's scale: measured worst case over the parametrised cases x 1.5 (printed by the tests).
# fp32: only the summation order differs from the CPU reference.  f16x3: operands carry 22 bits (bf16 halves, the first version: 16-17 bits,
# bounds 2.5e-5 / 4.5e-5 / 3e-5).  bf16: 8 bits on operands and
# stored activations.
STAGE_TOL = {'fp32': dict(obj=2e-6, cls=2e-6, boxes=1e-6),          # measured <= 1.0e-6 / 1.3e-6 / 5.7e-7
             'f16x3': dict(obj=3.5e-6, cls=4.5e-6, boxes=9e-7),    # measured <= 2.1e-6 / 3.0e-6 / 5.7e-7
             'bf16': dict(obj=1.5e-2, cls=2e-2, boxes=6e-3),        # measured <= 9.6e-3 / 1.3e-2 / 4.0e-3 (round 1 allowed 6e-2)
             'f16': dict(obj=2.5e-3, cls=3e-3, boxes=1e-3)}         # fp16 storage: bf16's bounds / 6 (three more bits would be / 8)
GAZE_TOL = {'fp32': 2e-6, 'f16x3': 3.5e-6, 'bf16': 4e-2, 'f16': 7e-3}           # measured 1.1e-6 / 2.2e-6 / 2.7e-2 (absolute, unit vectors)
PYRAMID_TOL = {'fp32': 4e-6, 'f16x3': 5e-6, 'bf16': 1.7e-2, 'f16': 3e-3}        # measured <= 2.6e-6 / 3.2e-6 / 1.13e-2 (round 1 allowed 5e-2)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('B,T', [(1, 7), (2, 3), (3, 1)])
def test_decoder_stage(eng, sd, kind, B, T):
    from mcgaze_amd.packing import PackedWeights
    dtype, split = KIND_DTYPE[kind], kind == 'f16x3'
    pw = PackedWeights(sd, dtype=dtype, split=split)
    N = B * T
    g = torch.Generator().manual_seed(100 + N)
    q = lambda t: t.to(dtype).float()
    roi = torch.randn(N * 3, 256, 7, 7, generator=g) * 3
    obj = torch.randn(N, 3, 256, generator=g)
    boxes = torch.tensor([[20., 30., 200., 210.], [60., 50., 160., 150.], [90., 60., 130., 100.]])[None].repeat(N, 1, 1)
    boxes = boxes + torch.randn(N, 3, 4, generator=g)
    for s in (0, 3):
        cls_r, delta_r, obj_r, inter = orc.stqi_stage(sd, s, q(roi), q(obj), T, return_intermediates=True)
        boxes_r = orc.delta2bbox(boxes.reshape(-1, 4), delta_r.reshape(-1, 4), stds=(0.5, 0.5, 1., 1.), clip_border=False).reshape(N, 3, 4)
        roi_dev = roi.permute(0, 2, 3, 1).reshape(N * 3, 49, 256).contiguous().to(dtype).to('cuda:0')
        obj_o, boxes_o, cls_o = eng.stage_forward(pw.stages[s], roi_dev, obj.to(dtype).to('cuda:0'), boxes.to('cuda:0'), T, split=split)
        torch.cuda.synchronize()
        errs = dict(obj=scale_err(obj_o, obj_r), cls=scale_err(cls_o, cls_r.squeeze(-1)), boxes=scale_err(boxes_o, boxes_r))
        print(f'decoder stage {s} {kind} B={B} T={T}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        for k, v in errs.items():
            assert v < STAGE_TOL[kind][k], (k, v)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('B,T', [(1, 7), (5, 3), (11, 1), (2, 10), (1, 11), (13, 7), (64, 7)])
def test_mlp_chain_matches_unfused_bitwise(eng, sd, B, T, dtype):
    """(bf16 and, round 6, the fp16 instantiations of the same templates.)  attn_block.hpp (both attention passes of a stage as one launch, one clip per workgroup, for 3 T <= 32; T = 11 takes the
    per-pass chain) and chain.hpp (towers and attention out-projection + LayerNorm as single launches) keep the K order, the bf16 rounding points
    and the LayerNorm reduction order of the launch sequence it replaces -- incl. row counts that are not a multiple of its 32-row
    block.  From 256 tokens on, `dynamic_layer` runs through pw_single.hpp (128 column slices with register-resident weights, tokens streamed in
    32-row tiles): 13 x 7 frames give 273 tokens = eight full tiles and one of 17 rows."""
    from mcgaze_amd.packing import PackedWeights
    pw = PackedWeights(sd, dtype=dtype)
    N = B * T
    g = torch.Generator().manual_seed(300 + N)
    roi = (torch.randn(N * 3, 49, 256, generator=g) * 3).to(dtype).to('cuda:0')
    obj = torch.randn(N, 3, 256, generator=g).to(dtype).to('cuda:0')
    boxes = (torch.tensor([[20., 30., 200., 210.], [60., 50., 160., 150.], [90., 60., 130., 100.]])[None].repeat(N, 1, 1) + torch.randn(N, 3, 4, generator=g)).to('cuda:0')
    outs = {}
    from mcgaze_amd import lib as L
    for mode, flags in (('0', L.FLAG_NO_SPECIALISED), ('1', 0)):
        outs[mode] = [t.clone() for t in eng.stage_forward(pw.stages[1], roi, obj, boxes, T, flags=flags)]
    torch.cuda.synchronize()
    for a, b, name in zip(outs['0'], outs['1'], ('obj', 'boxes', 'cls')):
        same = torch.equal(a.view(torch.int16) if a.element_size() == 2 else a, b.view(torch.int16) if b.element_size() == 2 else b)
        ndiff, dmax = int((a.float() != b.float()).sum()), float((a.float() - b.float()).abs().max())
        if dtype == torch.bfloat16:
            assert same, (name, f'{ndiff} of {a.numel()} elements differ, max |d| = {dmax:.3e}')
        else:
            # fp16: NOT bit-identical from a few hundred tokens on.  Measured (profiles/r06_f16_engine.md): the fused and the unfused decoder sequences agree
            # bit for bit up to 60 tokens and differ by ONE fp16 ulp in 0.2 - 4 % of the query features at 273 - 1344 tokens (13 x 7: 145 of 69 888) --
            # f32-level differences between the two instruction sequences that an 11-bit rounding exposes eight times as often as bf16's 8-bit one
            # (bf16: 0 differences on every case).  What the product needs holds bit for bit: a clip's result does not depend on its batch
            # (test_batched_equals_per_clip_bitwise, test_full_batch_properties[f16]); this is an A / B option of a throughput engine.
            scale = float(a.float().abs().max())
            print(f'f16 B={B} T={T} {name}: {ndiff} of {a.numel()} elements differ, max |d| = {dmax:.3e} (scale {scale:.2f})')
            assert same or (ndiff <= 0.06 * a.numel() and dmax <= 2.5e-3 * max(scale, 1.0)), (name, ndiff, dmax)


@pytest.mark.parametrize('B,T', [(1, 7), (5, 3), (11, 1), (2, 10), (1, 11), (13, 7), (64, 7)])
def test_attn_block_x3_matches_unfused_bitwise(eng, sd, B, T):
    """f16x3 (round 6): attn_block_x3.hpp -- both attention passes of a stage (in_proj, attention core, out_proj + residual + LayerNorm, twice) as
    ONE launch, one clip per workgroup, for 3 T <= 32 (T = 11 keeps the launch sequence) -- against the sequence it replaces
    (MCG_FLAG_NO_ATTN_BLOCK: igemm_dma in_proj, attn_core_kernel, mlp_chain_kernel<OpsX3> per pass) and against the generic launch sequence
    (MCG_FLAG_NO_SPECIALISED: no chains at all): same K order, same order of the three split terms, the same f32 rounding points, the
    same attention device function, ln_kernel's reduction order -- every output of the stage must be bit-identical in all three."""
    from mcgaze_amd.packing import PackedWeights
    from mcgaze_amd import lib as L
    pw = PackedWeights(sd, dtype=torch.float32, split=True)
    N = B * T
    g = torch.Generator().manual_seed(400 + N)
    roi = (torch.randn(N * 3, 49, 256, generator=g) * 3).to('cuda:0')
    obj = torch.randn(N, 3, 256, generator=g).to('cuda:0')
    boxes = (torch.tensor([[20., 30., 200., 210.], [60., 50., 160., 150.], [90., 60., 130., 100.]])[None].repeat(N, 1, 1) + torch.randn(N, 3, 4, generator=g)).to('cuda:0')
    outs = {}
    for mode, flags in (('generic', L.FLAG_NO_SPECIALISED), ('chains', L.FLAG_NO_ATTN_BLOCK), ('block', 0)):
        outs[mode] = [t.clone() for t in eng.stage_forward(pw.stages[2], roi, obj, boxes, T, split=True, flags=flags)]
    torch.cuda.synchronize()
    for name, a, b, c in zip(('obj', 'boxes', 'cls'), outs['generic'], outs['chains'], outs['block']):
        assert torch.equal(b, c), ('block vs chains', name, float((b - c).abs().max()))
        assert torch.equal(a, b), ('chains vs generic', name, float((a - b).abs().max()))


@pytest.mark.parametrize('kind', KINDS)
def test_gaze_head(eng, sd, kind):
    from mcgaze_amd.packing import PackedWeights
    dtype, split = KIND_DTYPE[kind], kind == 'f16x3'
    pw = PackedWeights(sd, dtype=dtype, split=split)
    obj = torch.randn(9, 3, 256, generator=torch.Generator().manual_seed(8))
    ref = orc.gaze_head(sd, 3, obj.to(dtype).float())
    out = eng.gaze_head(pw.gaze, obj.to(dtype).to('cuda:0'), split=split).cpu()
    torch.cuda.synchronize()
    worst = max(float((out[i] - ref[k]).abs().max()) for i, k in enumerate(('gaze_score', 'face_gaze_score', 'eyes_gaze_score', 'head_gaze_score')))
    print(f'gaze head {kind}: max |d| = {worst:.2e}')
    assert worst < GAZE_TOL[kind]
    assert torch.allclose(out.norm(dim=-1), torch.ones(4, 9), atol=1e-5)


@pytest.mark.parametrize('kind', KINDS)
def test_backbone_fpn(eng, sd, kind):
    e = eng.HipEngine(sd, precision=kind)
    img = torch.from_numpy(synth.make_clips(21, 1, 3, 64, 96))
    with torch.no_grad():
        ref = orc.fpn(sd, orc.resnet(sd, img))
    for chunk in (0, 2):
        pyr = e.backbone_fpn(img.to('cuda:0'), chunk_frames=chunk)
        torch.cuda.synchronize()
        for lvl, (p, r) in enumerate(zip(pyr, ref)):
            assert tuple(p.shape) == (r.shape[0], r.shape[2], r.shape[3], r.shape[1])
            err = scale_err(p.permute(0, 3, 1, 2), r)
            print(f'pyramid P{lvl + 2} {kind} chunk={chunk}: {err:.2e} of scale')
            assert err < PYRAMID_TOL[kind], f'P{lvl + 2} chunk={chunk}'
