"""-m gpu: mcg_gaze_head -- the grouped igemm launch of its six MLP branches, ln_kernel with per-row-group parameters and gaze_tail_kernel --
against the FLOAT64 oracle, in every engine kind.  tests/gaze_cases.py holds the cases, the references and the bounds (all computed on
the CPU from GAZE_TOL, the f32 oracle's own error and the f16x3 format model of tests/decoder_cases.py -- none from a GPU result);
tests/test_gaze_cases_cpu.py proves the cases and that each bound rejects the mutants listed there.

BASE        N = 9: the input of test_gpu_kernels.py::test_gaze_head, now against float64 and per output.
N_EDGE      N = 1, 127, 128, 129, 255, 256, 257 rows, row n = BASE row n % 9: every kind's 128-row tile one below, at and above one and two
            tiles.  Held to the BASE bound, and BIT FOR BIT to a separate N = 9 call: a row's result depends neither on its position in
            a tile nor on the neighbouring group's rows.
MAGNITUDE   fp32 and f16x3: the twelve MLP matrices, or the input, x 2^-6 and 2^-10.  f16x3 must stay within MARGIN x the format model;
            fp32 keeps the BASE bound -- the control.  At k = 10 the LayerNorm epsilon dominates the variance.
SCALE       fc_gaze, or the three per-clue output layers, x 2^-20 (2^-40): the float64 bound, and the normalised rows BIT FOR BIT equal
            to the unscaled call's (fma, sqrtf and the division all commute with a power of two; the library is built without fast-math
            flags, so hipcc's sqrtf and division are the correctly rounded ones).

Every output is finite and of unit norm to 1e-5.  The argument checks of mcg_gaze_head are exercised through ctypes on poisoned buffers.
Measured figures: DESIGN.md 3.2a.
"""
import ctypes as C

import pytest
import torch

from mcgaze_amd import lib as L
from tests import gaze_cases as G

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
_PACKED = {}


@pytest.fixture(scope='module')
def eng():
    from mcgaze_amd import engine
    return engine


def _packed(case, kind):
    """Packed weights, once per (state dict, kind)."""
    from mcgaze_amd.packing import PackedWeights
    sd = G.case_sd(case)
    key = (id(sd), kind)
    if key not in _PACKED:
        _PACKED[key] = PackedWeights(sd, dtype=G.KIND_DTYPE[kind], split=kind == 'f16x3', device=DEV)
    return _PACKED[key]


def _run(eng, case, kind):
    """mcg_gaze_head on the case -> [4, N, 3] f32 on the host."""
    obj = G.inputs(case).to(G.KIND_DTYPE[kind]).to(DEV)
    out = eng.gaze_head(_packed(case, kind).gaze, obj, split=kind == 'f16x3').cpu()
    assert tuple(out.shape) == (4, case.N, 3) and out.dtype == torch.float32
    return out


def _check(eng, name, kind):
    case = G.CASES[name]
    out = _run(eng, case, kind)
    dtype = G.KIND_DTYPE[kind]
    ref, fl, bd = G.reference(name, dtype), G.floor(name, dtype), G.bound(name, kind)
    m = G.model(name) if case.group == 'MAGNITUDE' else {}
    assert bool(torch.isfinite(out).all()), (name, kind)
    e, rows = G.errors(out, ref), G.row_err(out, ref).argmax(dim=1).tolist()
    print(f'{name} {kind}: ' + ', '.join(
        f'{k} {e[k]:.2e} at row {r} (floor {fl[k]:.1e}' + (f', model {m[k]:.1e}' if m else '') + f', bound {bd[k]:.2e})' for k, r in zip(G.OUTS, rows)))
    failed = [(k, e[k], bd[k]) for k in G.OUTS if not e[k] < bd[k]]
    assert not failed, (name, kind, failed)
    off = float((out.double().norm(dim=-1) - 1).abs().max())
    assert off < 1e-5, (name, kind, off)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, what):
    n = int((_bits(a) != _bits(b)).sum())
    assert n == 0, (what, f'{n} of {a.numel()} elements differ, max |d| = {float((a - b).abs().max()):.3e}')


def _params(cases):
    return [pytest.param(c.name, kind, id=f'{c.name}-{kind}') for c in cases for kind in G.kinds_of(c)]


@pytest.mark.parametrize('name,kind', _params(G.BASE))
def test_base(eng, name, kind):
    _check(eng, name, kind)


@pytest.mark.parametrize('name,kind', _params(G.N_EDGE))
def test_n_edge(eng, name, kind):
    """The bound, and row independence bit for bit: row n of the N-row call is row n % 9 of a separate 9-row call, whatever tile row, tile
    and neighbouring group it falls in (every N here runs the same 128-row tile configuration in a kind: gaze_cases.py)."""
    out = _check(eng, name, kind)
    out9 = _run(eng, G.CASES['N9'], kind)
    _same_bits(out, out9[:, G.rows_of(G.CASES[name])], (name, kind, 'rows of the N = 9 call'))


@pytest.mark.parametrize('name,kind', _params(G.MAGNITUDE))
def test_magnitude(eng, name, kind):
    _check(eng, name, kind)


@pytest.mark.parametrize('name,kind', _params(G.SCALE))
def test_scale(eng, name, kind):
    """The float64 bound on all four outputs, and bit for bit: the rows behind the scaled layer equal the unscaled call's (the fused row
    of fuse_k*, the three per-clue rows of clue_k20), and so do the rows the scale does not reach (the per-clue rows of fuse_k*)."""
    case = G.CASES[name]
    out = _check(eng, name, kind)
    out0 = _run(eng, G.CASES['N9'], kind)
    if case.family == 'fuse':
        _same_bits(out[0], out0[0], (name, kind, 'fused row under fc_gaze x 2^-k'))
    _same_bits(out[1:], out0[1:], (name, kind, 'per-clue rows'))


# ------------------------------------------------------------------------------------------------ argument checks
def _raw_call(eng, kind, N, n_call=None, null_entry=None, ws_short=0):
    """mcg_gaze_head through ctypes on a NaN-poisoned output and a 0xA5-poisoned workspace -> (rc, message, output untouched, workspace
    untouched)."""
    lib = L.load()
    pw = _packed(G.CASES['N9'], kind)
    dt = L.MCG_F16X3 if kind == 'f16x3' else {torch.float32: L.MCG_F32, torch.bfloat16: L.MCG_BF16, torch.float16: L.MCG_F16}[G.KIND_DTYPE[kind]]
    obj = G.inputs(G.CASES['N9'])[:N].to(G.KIND_DTYPE[kind]).to(DEV).contiguous()
    need = lib.mcg_gaze_head_workspace_bytes(dt, N)
    out = torch.full((4, N, 3), float('nan'), dtype=torch.float32, device=DEV)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    out0, ws0 = _bits(out).clone(), ws.clone()
    ptrs = [pw.gaze[k].data_ptr() for k in L.GAZE_KEYS]
    if null_entry is not None:
        ptrs[null_entry] = None
    table = (C.c_void_p * len(ptrs))(*ptrs)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.mcg_gaze_head(stream, dt, table, C.c_void_p(obj.data_ptr()), N if n_call is None else n_call, C.c_void_p(out.data_ptr()),
                           C.c_void_p(ws.data_ptr()), need - ws_short)
    torch.cuda.synchronize()
    return rc, lib.mcg_last_error().decode(errors='replace'), torch.equal(_bits(out), out0), torch.equal(ws, ws0), out


@pytest.mark.parametrize('kind', G.KINDS)
def test_argument_checks_write_nothing(eng, kind):
    rc, msg, out_same, ws_same, _ = _raw_call(eng, kind, 9, n_call=0)
    assert rc == 1 and 'bad argument' in msg and out_same and ws_same, (rc, msg)                    # MCG_ERR_ARG
    for i in range(L.GW_COUNT):
        rc, msg, out_same, ws_same, _ = _raw_call(eng, kind, 9, null_entry=i)
        assert rc == 1 and f'weight table entry {i} is null' in msg and out_same and ws_same, (i, rc, msg)
    rc, msg, out_same, ws_same, _ = _raw_call(eng, kind, 9, ws_short=1)
    assert rc == 4 and 'workspace too small' in msg and out_same and ws_same, (rc, msg)             # MCG_ERR_WORKSPACE
    # the same call with nothing wrong succeeds, overwrites every poisoned element and is the engine wrapper's result
    rc, msg, out_same, ws_same, out = _raw_call(eng, kind, 9)
    assert rc == 0 and not out_same and not ws_same and bool(torch.isfinite(out).all()), (rc, msg)
    _same_bits(out.cpu(), _run(eng, G.CASES['N9'], kind), (kind, 'ctypes call against engine.gaze_head'))
