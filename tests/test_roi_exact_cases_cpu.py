"""CPU: the instrument of tests/test_gpu_roi_exact.py proved without a GPU (tests/roi_exact_cases.py).  Every case satisfies the
exactness condition; the statement equals the f32 oracle (both forms) bit for bit and the hand-worked pins; the 16-bit expectations
contain rounding ties; and the bit comparison rejects every subtly wrong kernel listed in MUTANTS (each applied to the statement).  The
table printed by test_mutants_are_rejected says which of them the scale_err bounds of test_roi_align_all_levels accept on the same inputs."""
import numpy as np
import pytest
import torch

from oracle import mcgaze_oracle as orc
from tests import exact_cases as X
from tests import roi_align_pins as PINS
from tests import roi_exact_cases as R

DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
ALL_LEVELS_TOL = {'f32': 1e-5, 'bf16': 1e-2, 'fp16': 1e-2}     # test_roi_align_all_levels (tests/test_gpu_kernels.py)
MIN_TIES = 64


def _finite_cases():
    return [R.plain_case(n) for n in R.PLAIN_CASES] + [R.indexed_case(t) for t in R.INDEXED_TABLES]


def scale_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _nchw(f, rows=None):
    t = torch.from_numpy(np.array(f if rows is None else f[list(rows)])).float()
    return t.permute(0, 3, 1, 2).contiguous()


def test_every_case_satisfies_the_exactness_condition():
    worst = 0
    for case in _finite_cases():
        bits, levels = R.check_exactness(case)
        assert levels == case.levels, case.name          # the integer routing and the statement's log2 agree
        worst = max(worst, bits)
    print(f'largest number of fractional bits of a sample coordinate: {worst}; outputs are multiples of 2^-{R.FRAC_BITS}')
    assert worst == 4
    assert {len(c.boxes[0]) for c in _finite_cases()} >= {1, 3, 5} and {c.C for c in _finite_cases()} == {8, 16, 256, 1024}


def test_the_condition_rejects_instead_of_skipping():
    good = R.plain_case('odd-bpf1-c256')
    for box, match in (((0.0, 0.0, 111.75, 111.75), 'not 7 \\* 2\\^j'), ((0.0, 0.0, 30.0, 28.0), 'not 7 \\* 2\\^j'),
                       ((1.0 / 3, 0.0, 28.0, 28.0), 'not an integer'), ((0.25, 0.0, 28.25, 28.0), '1/8 level pixel'),
                       ((28.0, 0.0, 0.0, 28.0), 'one inverted axis')):
        bad = R.Case.__new__(R.Case)
        bad.__dict__.update(good.__dict__)
        bad.boxes, bad.tags = [[box]], ['bad']
        with pytest.raises(AssertionError, match=match):
            R.check_exactness(bad)
    bad.boxes, bad.feats = good.boxes, tuple(f * 2 for f in good.feats)
    bad.tags = good.tags
    with pytest.raises(AssertionError, match='255'):
        R.check_exactness(bad)


def test_every_edge_of_the_definition_is_hit_at_every_level():
    """Per pyramid, level and axis: a sample exactly at -1, exactly at L, one step outside each, in (-1, 0), in [L-1, L], an inverted
    box and a box entirely outside; zero extents at level 0 (a zero-area box routes there)."""
    kinds = ['at -1', 'at L', 'below -1', 'above L', 'in (-1, 0)', 'in [L-1, L]', 'inverted', 'outside']
    for name in ('frame-all-c8', 'odd-all-c8'):
        case = R.plain_case(name)
        seen = R.edge_census(case)
        missing = [(l, a, k) for l in range(4) for a in range(2) for k in kinds + ['zero'] * (l == 0) if (l, a, k) not in seen]
        assert not missing, (name, missing)
        tags = ' '.join(case.tags)
        assert all(f'sqrt(w h) = {b} px' in tags and f'one step below {b} px' in tags for b in R.LEVEL_BOUNDS)
        flat = case.flat_boxes()
        for level in range(4):       # every level is read from every frame: a wrong frame stride at any level changes some integer
            assert {r // case.bpf for r in range(len(flat)) if case.levels[r] == level and np.abs(case.ref[r]).max() > 0} == {0, 1, 2}


def test_statement_equals_the_f32_oracle_bit_for_bit():
    """The inputs are exact, so f32 arithmetic in any order gives the statement's numbers: oracle.roi_extract (vectorised, f32) and
    oracle.map_roi_levels on every finite case, oracle.roi_align_scalar (loop form, f32) on the full box sets."""
    for case in _finite_cases():
        boxes = torch.tensor(case.boxes, dtype=torch.float32)
        assert torch.equal(boxes.double(), torch.tensor(case.boxes, dtype=torch.float64))
        feats = [_nchw(f, case.frame_of) for f in case.feats]
        got = orc.roi_extract(feats, boxes, R.STRIDES)                                # [R, C, 7, 7] f32
        want = R.expected(case.q, torch.float32).reshape(-1, 7, 7, case.C).permute(0, 3, 1, 2)
        X.assert_exact(got, want, f'{case.name}: oracle.roi_extract')
        assert orc.map_roi_levels(boxes.reshape(-1, 4)).tolist() == case.levels
    for name in ('frame-all-c8', 'odd-all-c8'):
        case = R.plain_case(name)
        want = R.expected(case.q, torch.float32).reshape(-1, 7, 7, case.C).permute(0, 3, 1, 2).numpy()
        for r, box in enumerate(case.flat_boxes()):
            l = case.levels[r]
            roi = np.array([[r // case.bpf, *box]], dtype=np.float32)
            got = orc.roi_align_scalar(_nchw(case.feats[l]).numpy(), roi, 1.0 / R.STRIDES[l])[0]
            assert np.array_equal(got, want[r]), (name, case.tags[r])


def test_statement_equals_the_hand_worked_pins():
    sq = PINS.SQUARE_MAP[0, 0].astype(np.int64)[None, :, :, None]
    feats = [sq] + [np.zeros((1, 1, 1, 1), dtype=np.int64)] * 3
    ref, levels = R.roi_align_ref(feats, [[PINS.SQUARE_BOX]])
    assert levels == [0]
    for (ph, pw), v in PINS.SQUARE_HAND.items():
        assert ref[0, ph * 7 + pw, 0] == v, ((ph, pw), ref[0, ph * 7 + pw, 0], v)
    # and the affine closed form on the pins' own edge boxes (a 16 x 16 map at stride 4)
    amap = PINS.affine_map(16, 16)[0, 0].astype(np.int64)[None, :, :, None]
    ref, levels = R.roi_align_ref([amap] + feats[1:], [[b for _, b in PINS.EDGE_BOXES]])
    assert levels == [0] * len(PINS.EDGE_BOXES)
    for i, (name, box) in enumerate(PINS.EDGE_BOXES):
        np.testing.assert_allclose(ref[i, :, 0].reshape(7, 7), PINS.expected_affine(box, 4, 16, 16)[0], rtol=0, atol=1e-9, err_msg=name)


def test_nonfinite_boxes_state_the_kernel_interface():
    """csrc/roi_sample.hpp: a NaN box reads level 0 and a NaN sample coordinate contributes 0 -- zeros, finite, for every such row."""
    case = R.nonfinite_case()
    for r, (tag, box) in enumerate(R.NONFINITE_BOXES):
        if 'finite control' in tag:
            assert np.abs(case.ref[r]).max() > 0
        else:
            assert case.levels[r] == 0 and not case.ref[r].any(), tag
    assert case.levels[-1] == 1


def test_sixteen_bit_expectations_contain_ties():
    """The inputs exercise the rounding: outputs that the storage type cannot hold, and outputs exactly halfway between two of its
    values, per case and in total (printed; the GPU file's docstring quotes the totals)."""
    total = {k: [0, 0] for k in ('bf16', 'fp16')}
    for case in _finite_cases():
        for kind in total:
            inexact, ties = X.count_inexact(case.q, DTYPES[kind]), X.count_ties(case.q, DTYPES[kind])
            print(f'{case.name:22s} {kind}: {inexact:6d} of {case.q.numel():7d} outputs not representable, {ties:6d} ties')
            total[kind][0] += inexact
            total[kind][1] += ties
            assert ties >= MIN_TIES, (case.name, kind, ties)
    print('total', total)
    assert all(t[1] >= MIN_TIES for t in total.values())
    # exact_cases.expected with fractional bits rounds ties to even: 257 / 1024 and friends
    v = torch.tensor([257, 259, 2049, 2051, -257, 1 << 18])
    assert (X.expected(v, torch.bfloat16, 10).double() * 1024).tolist() == [256, 260, 2048, 2048, -256, 1 << 18]
    assert (X.expected(v, torch.float16, 10).double() * 1024).tolist() == [257, 259, 2048, 2052, -257, 1 << 18]
    assert (X.truncated(v, torch.float16, 10).double() * 1024).tolist() == [257, 259, 2048, 2050, -257, 1 << 18]


# ------------------------------------------------------------------------------------------------ mutants
def _mut_statement(name):
    done = {}      # one evaluation per case, shared by the storage types

    def run(case, kind):
        if case.name not in done:
            done[case.name] = R.quantize(R.roi_align_ref(case.feats, case.boxes, frame_of=case.frame_of, mut=name)[0])
        return R.expected(done[case.name], DTYPES[kind])
    return run


def _mut_truncate(case, kind):
    return X.truncated(case.q, DTYPES[kind], R.FRAC_BITS)


def _mut_sample_rounded(case, kind):
    """Each of the 4 samples of a bin rounded to the storage type before the mean."""
    rnd = lambda v: X.expected(torch.from_numpy(np.round(v * 256.0).astype(np.int64)), DTYPES[kind], 8).double().numpy()
    ref, _ = R.roi_align_ref(case.feats, case.boxes, frame_of=case.frame_of, sample_round=rnd)
    return torch.from_numpy(ref).float().to(DTYPES[kind])


def _mut_chunk_off_by_one(case, kind):
    """Channel group cg reads the features of group cg + 1 (wrapping): 4 channels per group in f32, 8 in the 16-bit types."""
    epc = 4 if kind == 'f32' else 8
    return R.expected(torch.roll(case.q, -epc, dims=-1), DTYPES[kind])


SIXTEEN = ('bf16', 'fp16')
EVERY = ('f32',) + SIXTEEN
# name: (function(case, kind) -> the mutant's output in the storage type, kinds it applies to, cases it is applied to)
MUTANTS = {
    'truncation instead of RNE': (_mut_truncate, SIXTEEN, ('plain:odd-all-c16',)),
    'each sample rounded before the mean': (_mut_sample_rounded, SIXTEEN, ('plain:odd-all-c16',)),
    'l and 1 - l swapped on x': (_mut_statement('l and 1 - l swapped on x'), EVERY, ('plain:odd-all-c16',)),
    'c >= L dropped (c > L is the test)': (_mut_statement('c >= L dropped'), EVERY, ('plain:odd-all-c16',)),
    'c <= -1 dropped (c < -1 is the test)': (_mut_statement('c <= -1 dropped'), EVERY, ('plain:odd-all-c16',)),
    'no clamp at 0': (_mut_statement('no clamp at 0'), EVERY, ('plain:odd-all-c16',)),
    'no far-edge collapse': (_mut_statement('no far-edge collapse'), EVERY, ('plain:odd-all-c16',)),
    'hi = lo + 1 clamped, not collapsed': (_mut_statement('hi = lo + 1 clamped'), EVERY, ('plain:odd-all-c16',)),
    'level boundary <= at 112': (_mut_statement('level boundary <= at 112'), EVERY, ('plain:odd-all-c16',)),
    'frame stride of level 0': (_mut_statement('frame stride of level 0'), EVERY, ('plain:odd-all-c16',)),
    'frame_of ignored': (_mut_statement('frame_of ignored'), EVERY, ('indexed:permuted', 'indexed:repeated', 'indexed:revisit')),
    'boxes_per_frame taken as 3': (_mut_statement('boxes_per_frame taken as 3'), EVERY, ('plain:odd-bpf1-c256', 'plain:odd-bpf5-c256')),
    'channel group off by one chunk': (_mut_chunk_off_by_one, EVERY, ('plain:odd-all-c16', 'plain:frame-bpf5-c1024')),
}


def _case(key):
    kind, name = key.split(':')
    return R.plain_case(name) if kind == 'plain' else R.indexed_case(name)


def test_rounding_before_the_quarter_is_not_a_mutant():
    """'Rounded before the * 0.25' cannot be told from 'rounded after': 0.25 is a power of two and nothing here is subnormal or
    overflows, so RNE(s) * 0.25 == RNE(s * 0.25) for every sum s.  Proved on the cases instead of listed as a mutant."""
    for case in (R.plain_case('odd-all-c16'), R.plain_case('frame-bpf5-c1024')):
        s = case.q * 4                                  # the 4-sample sums, in units of 2^-10
        for dt in (torch.bfloat16, torch.float16):
            before = (X.expected(s, dt, R.FRAC_BITS).float() * 0.25).to(dt)
            assert torch.equal(before.float(), X.expected(s, dt, R.FRAC_BITS).float() * 0.25)     # the product is representable
            assert torch.equal(before, R.expected(case.q, dt))


def test_mutants_are_rejected():
    """Every mutant differs from the expectation in at least one element, in every storage type it applies to and on EVERY case it is
    applied to.  The printed table says which of them the scale_err bounds of test_roi_align_all_levels accept on the same inputs."""
    lines = []
    for name, (fn, kinds, keys) in MUTANTS.items():
        row = {}
        for kind in kinds:
            worst = 0.0
            for key in keys:
                case = _case(key)
                want, got = R.expected(case.q, DTYPES[kind]), fn(case, kind)
                assert got.dtype == want.dtype and got.shape == want.shape
                with pytest.raises(AssertionError):
                    X.assert_exact(got, want, f'{name} / {key} / {kind}')
                worst = max(worst, scale_err(got, torch.from_numpy(case.ref)))
            row[kind] = f'{worst:.1e} ' + ('ACCEPTED' if worst < ALL_LEVELS_TOL[kind] else 'rejected')
        lines.append(f'    {name:40s}' + ''.join(f'{row.get(k, "-"):19s}' for k in EVERY).rstrip())
    print('\n    ' + f'{"mutant":40s}' + ''.join(f'{k:19s}' for k in EVERY).rstrip())
    print('\n'.join(lines))
