"""-m gpu: roi_align_kernel (csrc/roi_align.hip, csrc/roi_sample.hpp) through mcg_roi_align and mcg_roi_align_indexed, in f32, bf16 and
fp16, against a float64 statement of the published definition, BIT FOR BIT.  tests/roi_exact_cases.py holds the inputs, the statement and
the condition; tests/test_roi_exact_cases_cpu.py proves them on the CPU (the statement equals the f32 oracle to the bit there).

THE EXACTNESS CONDITION.  Features are integers in [-255, 255]; every box corner is a multiple of 1/8 level pixel and every extent is
7 * 2^j level pixels (j in -2..3), zero, or the negative of one.  Then bin = 2^j, every sample coordinate and weight is a binary fraction
of at most 4 fractional bits however the expression is contracted, every product w * v and every 16-term sum is an f32 value (below 2^18
in units of 2^-8), * 0.25f is exact, and sqrt(w h) is exactly on a level boundary or at least a factor sqrt(2) from it.  Outputs are
multiples of 2^-10.  roi_exact_cases.check_exactness asserts this on every case (CPU test); it is never a skip.  No tolerance is left: a
wrong tap, weight, validity edge, clamp, collapse, level, frame stride, frame index or channel chunk changes some number.

THE ROUNDING CONVENTION.  f32: the number itself.  bf16 / fp16: ONE round-to-nearest-even of it (include/mcgaze_hip.h).  Over the cases
408 294 (bf16) and 54 973 (fp16) expected outputs are not representable in the storage type, and 147 897 (bf16) and 42 363 (fp16) lie
exactly halfway between two representable values; every case holds at least 498 ties per type (the CPU test asserts >= 64).

WHAT THE TOLERANCES LET THROUGH.  Each mutation below was applied to the statement on the CPU (test_roi_exact_cases_cpu.py::
test_mutants_are_rejected); the bit comparison rejects every one in every storage type it applies to.  Beside it, scale_err (max |d| over
the reference's largest element) of the mutant on the same inputs, and whether the bounds of test_roi_align_all_levels (tests/
test_gpu_kernels.py: 1e-5 f32, 1e-2 bf16 / fp16) accept it:

    mutant                                  f32                bf16               fp16
    truncation instead of RNE               -                  3.9e-03 ACCEPTED   4.3e-04 ACCEPTED
    each sample rounded before the mean     -                  3.4e-03 ACCEPTED   4.3e-04 ACCEPTED
    l and 1 - l swapped on x                1.8e+00 rejected   1.8e+00 rejected   1.8e+00 rejected
    c >= L dropped (c > L is the test)      7.3e-01 rejected   7.3e-01 rejected   7.3e-01 rejected
    c <= -1 dropped (c < -1 is the test)    6.5e-01 rejected   6.5e-01 rejected   6.5e-01 rejected
    no clamp at 0                           1.4e+00 rejected   1.4e+00 rejected   1.4e+00 rejected
    no far-edge collapse                    8.5e-01 rejected   8.5e-01 rejected   8.5e-01 rejected
    hi = lo + 1 clamped, not collapsed      7.3e-01 rejected   7.3e-01 rejected   7.3e-01 rejected
    level boundary <= at 112                1.2e+00 rejected   1.2e+00 rejected   1.2e+00 rejected
    frame stride of level 0                 1.8e+00 rejected   1.8e+00 rejected   1.8e+00 rejected
    frame_of ignored                        1.8e+00 rejected   1.8e+00 rejected   1.8e+00 rejected
    boxes_per_frame taken as 3              1.9e+00 rejected   1.9e+00 rejected   1.9e+00 rejected
    channel group off by one chunk          2.0e+00 rejected   2.0e+00 rejected   2.0e+00 rejected

The two rounding mutants pass the 16-bit bound with a margin of 2.5 to 23: no test before this one told a 16-bit RoIAlign that truncates
from one that rounds.  The geometry mutants are large on THESE inputs (independent integers per pixel, boxes built on the edges); on the
smooth maps and generic boxes of the tolerance tests most of them move a few outputs by a fraction of a pixel's gradient.  "Rounded
before the * 0.25" is no mutant: 0.25 is a power of two, so it is the same function (proved in the CPU file).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from tests import exact_cases as X
from tests import roi_exact_cases as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
KINDS = {'f32': (torch.float32, L.MCG_F32), 'bf16': (torch.bfloat16, L.MCG_BF16), 'fp16': (torch.float16, L.MCG_F16)}
POISON = -768.0        # a value of all three storage types that no output can take (|outputs| <= 255)
kinds = pytest.mark.parametrize('kind', list(KINDS))


@pytest.fixture(scope='module')
def eng():
    from mcgaze_amd import engine
    return engine


def _dev(f, dtype):
    """int64 NHWC array -> ``dtype`` on the device; the conversion itself must be exact."""
    t = torch.from_numpy(np.array(f))
    v = t.to(dtype)
    assert torch.equal(v.to(torch.int64), t), 'a feature is not representable in its storage type'
    return v.to(DEV)


def _boxes(case):
    b = torch.tensor(case.boxes, dtype=torch.float32)
    assert b.shape == (R.N_FRAMES, case.bpf, 4)
    return b.to(DEV)


# ------------------------------------------------------------------------------------------------ mcg_roi_align
@kinds
@pytest.mark.parametrize('name', list(R.PLAIN_CASES))
def test_roi_align_is_exact(eng, name, kind):
    """Both pyramids, every level, every edge of the definition, C = 8 .. 1024 and boxes_per_frame = 1, 3, 5 and 91."""
    dt = KINDS[kind][0]
    case = R.plain_case(name)
    out, lv = eng.roi_align([_dev(f, dt) for f in case.feats], _boxes(case))
    torch.cuda.synchronize()
    assert lv.cpu().tolist() == case.levels
    X.assert_exact(out, R.expected(case.q, dt), f'roi_align {name} {kind}')


@kinds
def test_roi_align_nonfinite_boxes(eng, kind):
    """The interface of csrc/roi_sample.hpp: a NaN box reads level 0, a NaN sample coordinate contributes 0 -- finite zeros, with the
    finite boxes among them untouched."""
    dt = KINDS[kind][0]
    case = R.nonfinite_case()
    out, lv = eng.roi_align([_dev(f, dt) for f in case.feats], _boxes(case))
    torch.cuda.synchronize()
    assert lv.cpu().tolist() == case.levels
    assert bool(torch.isfinite(out.float()).all())
    X.assert_exact(out, R.expected(case.q, dt), f'roi_align nonfinite {kind}')


# ------------------------------------------------------------------------------------------------ mcg_roi_align_indexed
@kinds
@pytest.mark.parametrize('table', list(R.INDEXED_TABLES))
def test_roi_align_indexed_is_exact(eng, table, kind):
    """A store of 5 rows read by 3 window frames: exact against the statement on the gathered rows, and bit-equal to the plain call on a
    physically gathered copy."""
    dt = KINDS[kind][0]
    case = R.indexed_case(table)
    store = [_dev(f, dt) for f in case.feats]
    assert store[0].shape[0] == R.STORE_ROWS
    out, lv = eng.roi_align_indexed(store, _boxes(case), list(case.frame_of))
    rows = torch.tensor(case.frame_of, device=DEV)
    plain, plain_lv = eng.roi_align([f[rows].contiguous() for f in store], _boxes(case))
    torch.cuda.synchronize()
    assert lv.cpu().tolist() == case.levels == plain_lv.cpu().tolist()
    X.assert_exact(out, R.expected(case.q, dt), f'roi_align_indexed {table} {kind}')
    assert torch.equal(out, plain)


def _raw(entry, code, feats, hw, Cc, boxes, num_boxes, bpf, out, lv, table=None, rows=None, null_level=None):
    """The C entry itself, past the host-side checks of engine.roi_align_indexed.  -> return code."""
    lib = L.load()
    fp = (C.c_void_p * 4)(*[None if i == null_level else f.data_ptr() for i, f in enumerate(feats)])
    fh = (C.c_int * 4)(*[h for h, _ in hw])
    fw = (C.c_int * 4)(*[w for _, w in hw])
    st = (C.c_int * 4)(*R.STRIDES)
    gather = () if table is None else (C.c_void_p(table.data_ptr()), rows)
    return getattr(lib, entry)(C.c_void_p(torch.cuda.current_stream().cuda_stream), code, fp, fh, fw, st, Cc, C.c_void_p(boxes.data_ptr()),
                               num_boxes, bpf, *gather, C.c_void_p(out.data_ptr()), C.c_void_p(lv.data_ptr()))


@kinds
def test_roi_align_indexed_guard(kind):
    """The device-side guard, which engine.roi_align_indexed's host check never lets a caller reach: a frame_of entry outside
    [0, pyramid_frames) gives NaN rows, reads nothing, leaves the neighbours and everything past the output untouched, and levels_out is
    still written for every box."""
    dt, code = KINDS[kind]
    case = R.indexed_case('repeated')                    # table (1, 1, 1): its first frame is what GUARD_TABLE's good entry reads
    assert R.GUARD_TABLE[0] == case.frame_of[0] and all(not 0 <= t < R.STORE_ROWS for t in R.GUARD_TABLE[1:])
    store = [_dev(f, dt) for f in case.feats]
    boxes = _boxes(case)
    nb, per = R.N_FRAMES * case.bpf, 49 * case.C
    out = torch.full((nb + 2, per), POISON, dtype=dt, device=DEV)
    lv = torch.full((nb + 2,), -1, dtype=torch.int32, device=DEV)
    table = torch.tensor(R.GUARD_TABLE, dtype=torch.int32, device=DEV)
    rc = _raw('mcg_roi_align_indexed', code, store, case.hw, case.C, boxes, nb, case.bpf, out, lv, table, R.STORE_ROWS)
    torch.cuda.synchronize()
    assert rc == L.MCG_OK
    out, lv = out.cpu(), lv.cpu()
    assert lv[:nb].tolist() == case.levels and lv[nb:].tolist() == [-1, -1]
    X.assert_exact(out[:case.bpf].reshape(case.bpf, 49, case.C), R.expected(case.q[:case.bpf], dt), f'guard {kind}: the good frame')
    assert bool(torch.isnan(out[case.bpf:nb]).all())
    assert bool((out[nb:] == POISON).all())


@kinds
@pytest.mark.parametrize('what', ['null level', 'num_boxes = 0', 'pyramid_frames = 0', 'C = 12'])
def test_roi_align_argument_checks_write_nothing(what, kind):
    dt, code = KINDS[kind]
    case = R.indexed_case('permuted')
    store = [_dev(f, dt) for f in case.feats]
    boxes = _boxes(case)
    nb = R.N_FRAMES * case.bpf
    out = torch.full((nb, 49 * case.C), POISON, dtype=dt, device=DEV)
    lv = torch.full((nb,), -1, dtype=torch.int32, device=DEV)
    table = torch.tensor(case.frame_of, dtype=torch.int32, device=DEV)
    args = dict(feats=store, hw=case.hw, Cc=case.C, boxes=boxes, num_boxes=nb, bpf=case.bpf, out=out, lv=lv)
    if what == 'null level':
        rcs = [_raw('mcg_roi_align', code, **args, null_level=2), _raw('mcg_roi_align_indexed', code, **args, table=table, rows=R.STORE_ROWS, null_level=2)]
    elif what == 'num_boxes = 0':
        args['num_boxes'] = 0
        rcs = [_raw('mcg_roi_align', code, **args), _raw('mcg_roi_align_indexed', code, **args, table=table, rows=R.STORE_ROWS)]
    elif what == 'pyramid_frames = 0':
        rcs = [_raw('mcg_roi_align_indexed', code, **args, table=table, rows=0)]
    else:
        args['Cc'] = 12
        rcs = [_raw('mcg_roi_align', code, **args), _raw('mcg_roi_align_indexed', code, **args, table=table, rows=R.STORE_ROWS)]
    torch.cuda.synchronize()
    assert all(rc != L.MCG_OK for rc in rcs), rcs
    assert bool((out == POISON).all()) and bool((lv == -1).all())
