"""-m gpu: the streaming 1x1 kernels -- pw_single_kernel, pw_single_x3_kernel, pw_single_x3_blocks_kernel, pw_pair_kernel, in every
instantiation the launchers dispatch, dynamic_layer's two forms included -- at SMALL M, through mcg_pointwise_stream / mcg_pointwise_dyn /
mcg_pointwise_pair, against an int64 statement of the operator, BIT FOR BIT.  tests/pw_exact_cases.py holds the forms, the row counts and the
references, tests/exact_cases.py the exactness condition and the rounding convention; tests/test_pw_exact_cases_cpu.py proves them on the CPU
and lists the subtly wrong kernels the comparison rejects.

WHY SMALL M.  The engine takes these kernels from 64 Ki rows on, at product grid size (2 x CUs walkers) a walker needs more than 16 Ki rows
for a second trip, and the engine-level tests compare with the generic kernel, which shares the upsample gather.  Here grid_cap = 1 leaves
8 walkers per channel slice: M = 753 is 24 tiles, the last of 17 rows, three trips per walker (both buffer parities, the reuse of the
first, the single-A-tile refill), M = 33 a second walker with one row, and every dense run stores into a buffer with 32 sentinel rows
behind row M, which must survive.  The list form runs over a sentinel-filled map: listed pixels equal the dense reference, every other
pixel is still the sentinel.

ROUNDING.  One scaled run per 16-bit form family puts ties under the store; counted on the reference alone (CPU test), outputs exactly
halfway between two representable values:

    activations x 16 (bf16) / x 64 (fp16), M = 753, ReLU        bf16      fp16
    stream 512 -> 128                                          11 984     8 230
    stream 256 -> 256  + residual                              18 726     7 254
    stream 128 -> 512  + residual                              27 980     4 261
    stream 256 -> 1024 + residual                              75 467    29 298
    dynamic_layer, 17 rows                                    125 785    48 323
    pair (K2, C2), M = 369: ties in y / y values that move when rounded / ties in z; fp16 with one source x 128 (x 64: too few sums pass 2048)
      (0, 64)                                     3312 / 3366 / 2065     3312 / 3366 / 2076
      (0, 128)                                    2361 / 2388 / 4420     2361 / 2388 / 4421
      (64, 64)                                    7793 / 9170 / 2230     1377 / 1377 / 2982
      (64, 128)                                   7197 / 8327 / 3580     1130 / 1130 / 4771

f16x3: the x 683 runs feed 55 048 (256 -> 256) and 55 157 (256 -> 1024) of 192 768 activations with a non-zero fp16 low half, dynamic_layer
1225 of 4352.
"""
import functools

import pytest
import torch

from mcgaze_amd import lib as L
from tests import exact_cases as X
from tests import pw_exact_cases as P

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
KINDS = ('bf16', 'fp16', 'f16x3')


@pytest.fixture(scope='module')
def eng():
    from mcgaze_amd import engine
    return engine


def _dev(t, dtype):
    """int64 -> ``dtype`` on the device; the conversion itself must be exact."""
    v = t.to(dtype)
    assert torch.equal(v.to(torch.int64), t), 'an input is not representable in its storage type'
    return v.contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def _weights(fn, args, kind):
    """(w, b) = fn(*args) -> (wf, wscale, bias) on the device, packed once per weight matrix and precision."""
    from mcgaze_amd.engine import pointwise_weights
    w, b = fn(*args)
    wf, wscale = pointwise_weights(w.float(), X.TORCH_DT[kind], split=kind == 'f16x3', device=DEV)
    return wf, wscale, b.float().to(DEV)


def _stream_wb(K, N):
    d = P.stream_inputs(K, N)
    return d['w'], d['b']


def _buffer(M, N, dt):
    return torch.full((M + P.GUARD, N), P.SENTINEL, dtype=dt, device=DEV)


def _run_stream(eng, kind, K, N, r, M, up, relu, scale, cap):
    dt = X.TORCH_DT[kind]
    d = P.stream_inputs(K, N, scale)
    wf, wscale, bias = _weights(_stream_wb, (K, N), kind)
    assert torch.equal(d['w'], P.stream_inputs(K, N)['w']) and torch.equal(d['b'], P.stream_inputs(K, N)['b'])   # a scaled case scales the activations only
    kw = {}
    if r == 1:
        kw = dict(residual=_dev(d['res'][:M], dt), residual_mode=L.RES_ADD)
    elif r == 2:
        (f, ho, wo), _ = P.UP_SHAPES[up]
        kw = dict(residual=_dev(X.nhwc(d['up'][up]), dt), residual_mode=L.RES_UPSAMPLE_ADD, out_hw=(ho, wo))
    return eng.pointwise_stream(_dev(d['a'][:M], dt), wf, bias, N, relu=relu, split=kind == 'f16x3', wscale=wscale, grid_cap=cap,
                                out=_buffer(M, N, dt), **kw)


def _form_params():
    return [pytest.param(kind, K, N, r, id=f'{kind}-{K}-{N}-res{r}') for kind in KINDS for K, N, r in P.stream_forms(kind)]


@pytest.mark.parametrize('kind,K,N,r', _form_params())
def test_stream_is_exact(eng, kind, K, N, r):
    """Every dispatched (K, N, res_mode) form at every row count, one group of walkers and the product grid, with and without ReLU;
    the sentinel rows behind row M untouched."""
    dt = X.TORCH_DT[kind]
    outs = [((M, up, cap, relu), _run_stream(eng, kind, K, N, r, M, up, relu, 1, cap)) for M, up, cap in P.stream_runs(r) for relu in (False, True)]
    torch.cuda.synchronize()
    for (M, up, cap, relu), y in outs:
        X.assert_exact(y, P.with_guard(X.expected(P.stream_ref(K, N, r, M, up, relu), dt)), f'stream {kind} {K} -> {N} res {r} M={M} cap={cap} relu={relu}')


@pytest.mark.parametrize('kind,K,N,r', [pytest.param(kind, K, N, r, id=f'{kind}-{K}-{N}-res{r}') for kind in KINDS for K, N, r in P.SCALED_STREAM[kind]])
def test_stream_scaled_is_exact(eng, kind, K, N, r):
    """Activations x 16 / x 64: rounding ties under the 16-bit store; x 683 for f16x3: non-zero fp16 low halves in the split."""
    dt = X.TORCH_DT[kind]
    y = _run_stream(eng, kind, K, N, r, P.M_MAX, None, True, P.SCALE[kind], 1)
    torch.cuda.synchronize()
    X.assert_exact(y, P.with_guard(X.expected(P.stream_ref(K, N, r, P.M_MAX, None, True, P.SCALE[kind]), dt)), f'stream {kind} {K} -> {N} res {r} x{P.SCALE[kind]}')


def _dyn_wb():
    d = P.dyn_inputs()
    return d['w'], d['b']


@pytest.mark.parametrize('kind', KINDS)
def test_dynamic_layer_is_exact(eng, kind):
    """pw_single_kernel<16, 2, 0, 128> (bf16, fp16) and pw_single_x3_kernel<16, 0, 256>: 17 and 273 rows, one walker per slice and the
    product rule; and the scaled 17 rows."""
    dt = X.TORCH_DT[kind]
    runs = [(1, M, cap) for M, cap in P.DYN_M] + [(P.SCALE[kind], P.DYN_SCALED_M, 1)]
    wf, wscale, bias = _weights(_dyn_wb, (), kind)
    for scale, M, cap in runs:
        assert torch.equal(P.dyn_inputs(scale)['w'], P.dyn_inputs()['w'])
        a = _dev(P.dyn_inputs(scale)['a'][:M], dt)
        y = eng.pointwise_stream(a, wf, bias, P.DYN_N, split=kind == 'f16x3', wscale=wscale, many_slices=True, grid_cap=cap, out=_buffer(M, P.DYN_N, dt))
        torch.cuda.synchronize()
        X.assert_exact(y, P.with_guard(X.expected(P.dyn_ref(scale)[0][:M], dt)), f'dynamic_layer {kind} M={M} cap={cap} x{scale}')


def _list_wb():
    d = P.list_inputs()
    return d['w'][:, :, 0, 0], d['b']


@pytest.mark.parametrize('cap', [1, 0], ids=['cap1', 'product'])
@pytest.mark.parametrize('name', list(P.LISTS))
def test_list_form_is_exact(eng, name, cap):
    """pw_single_x3_blocks_kernel<16, 2>: listed pixels equal the dense reference, every other pixel is still the sentinel; ids outside
    the map and an empty list write nothing."""
    d = P.list_inputs()
    (f, ho, wo), _ = P.LIST_MAP
    wf, wscale, bias = _weights(_list_wb, (), 'f16x3')
    y = torch.full((f * ho * wo, 256), P.SENTINEL, dtype=torch.float32, device=DEV)
    eng.pointwise_stream(_dev(X.nhwc(d['x']).reshape(-1, 256), torch.float32), wf, bias, 256, residual=_dev(X.nhwc(d['res']), torch.float32),
                         residual_mode=L.RES_UPSAMPLE_ADD, out_hw=(ho, wo), split=True, wscale=wscale, blocks=P.LISTS[name], grid_cap=cap, out=y)
    torch.cuda.synchronize()
    X.assert_exact(y.reshape(f, ho, wo, 256), P.list_expected(P.LISTS[name]), f'list {name} cap={cap}')


def _pair_w3(K2, C2):
    d = P.pair_inputs(K2, C2)
    return d['w3'], d['b3']


def _pair_w1(K2, C2):
    d = P.pair_inputs(K2, C2)
    return d['w1'], d['b1']


def _run_pair(eng, kind, K2, C2, M, cap, scale, with_res=None):
    dt = X.TORCH_DT[kind]
    kw = P.pair_args(K2, C2, M, scale, with_res)
    assert torch.equal(kw['w3'], P.pair_inputs(K2, C2)['w3']) and torch.equal(kw['w1'], P.pair_inputs(K2, C2)['w1'])
    w3f, _, b3 = _weights(_pair_w3, (K2, C2), kind)
    w1f, _, b1 = _weights(_pair_w1, (K2, C2), kind)
    dev = lambda t: _dev(t, dt) if t is not None else None
    y, z = eng.pointwise_pair(dev(kw['a1']), w3f, b3, w1f, b1, C2, a2=dev(kw['a2']), residual=dev(kw['res']), grid_cap=cap,
                              out=(_buffer(M, 256, dt), _buffer(M, C2, dt)))
    ry, _, rz = P.pair_ref(**kw, dtype=dt)
    return y, z, P.with_guard(X.expected(ry, dt)), P.with_guard(X.expected(rz, dt))


@pytest.mark.parametrize('K2,C2', list(P.PAIR_FORMS))
@pytest.mark.parametrize('kind', P.KINDS16)
def test_pair_is_exact(eng, kind, K2, C2):
    """pw_pair_kernel<F, NSRC, C2T>, all four forms: y and z at every row count, the scaled run (z from the ROUNDED y), and the
    one-source form without a residual."""
    runs = [(M, cap, 1, None) for M, cap in P.PAIR_M] + [(P.PAIR_M_MAX, 2, P.PAIR_SCALE[kind][K2], None)] + ([(177, 1, 1, False)] if K2 == 0 else [])
    outs = [(run, _run_pair(eng, kind, K2, C2, *run)) for run in runs]
    torch.cuda.synchronize()
    for (M, cap, scale, with_res), (y, z, wy, wz) in outs:
        what = f'pair {kind} K2={K2} C2={C2} M={M} cap={cap} x{scale}' + (' no residual' if with_res is False else '')
        X.assert_exact(y, wy, what + ': y')
        X.assert_exact(z, wz, what + ': z')


def test_unsupported_answers(eng):
    """Host side: outside the launch tables the entries answer MCG_ERR_UNSUPPORTED (3) and launch nothing; they never fall back."""
    def refused(fn, *a, **kw):
        with pytest.raises(L.McgError, match=r'\(code 3\)'):
            fn(*a, **kw)
    z16 = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=DEV)
    z32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    refused(eng.pointwise_stream, z16(33, 256), z16(512, 256), z32(512), 512)                                           # (256, 512) is no form
    refused(eng.pointwise_stream, z16(33, 512), z16(256, 512), z32(256), 256, residual=z16(33, 256), residual_mode=L.RES_ADD)   # (512, 256) + residual
    refused(eng.pointwise_stream, z16(33, 512), z16(128, 512), z32(128), 128, residual=z16(33, 128), residual_mode=L.RES_ADD)   # (512, 128) + residual
    refused(eng.pointwise_stream, z32(33, 128), z16(512, 256), z32(512), 512, split=True)                               # f16x3: (128, 512) is no form
    refused(eng.pointwise_stream, z32(33, 256), z32(256, 256), z32(256), 256)                                           # plain f32 has no streaming kernel
    up = dict(residual_mode=L.RES_UPSAMPLE_ADD, split=True)
    refused(eng.pointwise_stream, z32(2 * 12 * 16, 256), z16(256, 512), z32(256), 256, residual=z32(2, 6, 8, 256), out_hw=(12, 16), blocks=[0], **up)   # 12 rows: no whole blocks
    refused(eng.pointwise_stream, z16(128, 256), z16(256, 256), z32(256), 256, residual=z16(1, 4, 8, 256), residual_mode=L.RES_UPSAMPLE_ADD,
            out_hw=(8, 16), blocks=[0])                                                                                 # the list form is f16x3's
    refused(eng.pointwise_stream, z32(128, 256), z16(256, 512), z32(256), 256, residual=z32(128, 256), residual_mode=L.RES_ADD, split=True, blocks=[0])
    refused(eng.pointwise_pair, z16(65, 64), z16(256, 64), z32(256), z16(96, 256), z32(96), 96)                          # C2 = 96
    refused(eng.pointwise_pair, z16(65, 64), z16(256, 128), z32(256), z16(64, 256), z32(64), 64, a2=z16(65, 64), residual=z16(65, 256))   # two sources + residual
    refused(eng.pointwise_pair, z32(65, 64), z32(256, 64), z32(256), z32(64, 256), z32(64), 64)                          # f32
    with pytest.raises(L.McgError, match=r'\(code 1\)'):
        eng.pointwise_stream(z16(33, 256), z16(256, 256), z32(256), 256, grid_cap=-1)
    torch.cuda.synchronize()
