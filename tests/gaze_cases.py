"""Shared by tests/test_gaze_cases_cpu.py and tests/test_gpu_gaze_head.py: the gaze head (mcg_gaze_head) against a FLOAT64 run of the oracle,
across the row-tile edges of its grouped contraction, operand magnitudes and power-of-two scales of its output layers.  CPU only, seeded,
cached.  The format model, its hooks and MARGIN are tests/decoder_cases.py's; nothing of them is restated here.

THE REFERENCE is oracle.mcgaze_oracle.gaze_head on a float64 copy of the state dict and of the input, the input first rounded to the
storage type of the engine kind, as the kernel receives it.

BASE        N = 9 frames, seed 8: the input of tests/test_gpu_kernels.py::test_gaze_head.
N_EDGE      N frames whose row n is row n % 9 of the BASE input.  Frames are independent in this operator, so every row's expected value
            is a BASE row's and BASE's bound applies by construction; 9 is coprime to the tile heights, so a permutation of rows by a
            whole tile does not map the expected values onto themselves.  The grouped contraction (launch_igemm, 6 groups, M = N rows
            per group, Cout = 256, K = 256) stores group g's rows directly in front of group g + 1's, and ln_kernel changes its
            parameters every N rows of 6 N.  Row-tile height per kind, read from launch_typed / launch_x3 in csrc/igemm.hip:
              fp32        ES = 4: never the DMA kernel; Cin x 4 bytes is a multiple of 128 and Cout > 64 -> launch_cfg<128,128,128,2,2>:
                          128 rows, at every N.
              bf16, f16   DMA kernel, Cout > 64, K = 256 < 384, blocks9 = ceil(N / 256) x 2 < kT9Min = 300 and N <= 4096 -> tile 11
                          (128 x 128): 128 rows, at every N here.  Tile 9 (256 rows) needs blocks9 >= 300: N > 38 144.
              f16x3       t256 = ceil(N / 256) < 200 -> tile 51 (128 x 128, 4 waves); tile 53 needs K >= 512: 128 rows, at every N here.
                          Tile 50 (256 rows) needs t256 >= 200: N > 50 944.
            So 128 is the one height taken up to the sizes a quick test can hold: N = 1 (one row of a tile), 127 / 128 / 129 (one below,
            at, above), 255 / 256 / 257 (two tiles; and one below, at, above the 256 the code holds for larger problems).
MAGNITUDE   fp32 (control) and f16x3.  ``mlp_k{6,10}``: the twelve MLP matrices x 2^-k (packed without a pre-scale, packing.py);
            ``obj_k{6,10}``: the input x 2^-k (split in registers by the kernel).  At k = 10 the pre-LayerNorm variance is below the 1e-5
            epsilon: the one place where ln_kernel's epsilon placement shows.
SCALE       ``fuse_k{20,40}``: fc_gaze.weight and .bias x 2^-k; ``clue_k20``: fc_{face,eyes,head}.weight and .bias x 2^-k.  A power of
            two on a vector that is then L2-normalised changes no bit of the f32 result short of underflow.

THE BOUNDS, all from the CPU (``bound``): GAZE_TOL[kind] + floor, where ``floor`` is the f32 CPU oracle's distance to float64 on the case
(the triangle inequality on the test that passes today); MAGNITUDE f16x3 adds MARGIN x model, the float64 oracle with the f16x3 format
model at 'gaze_fc0' and 'gaze_fc1' against plain float64.  THE METRIC is GAZE_TOL's: max |d| over a row's three components, the worst
row, per output (``row_err`` keeps the per-row figures).
"""
import collections
import functools

import torch

from oracle import mcgaze_oracle as orc
from tests.decoder_cases import MARGIN, base_sd, split_rtz16, x3_hooks, x3_product  # noqa: F401  (split_rtz16, x3_product: re-exported)
from tests.test_gpu_kernels import GAZE_TOL, KIND_DTYPE, KINDS  # noqa: E402

STAGE = 3                                                    # only the last stage's gaze head runs at inference
OUTS = ('gaze_score', 'face_gaze_score', 'eyes_gaze_score', 'head_gaze_score')   # the slot order of mcg_gaze_head's [4][N][3]
SITES = ('gaze_fc0', 'gaze_fc1')
BASE_N, BASE_SEED = 9, 8
TILE_ROWS = 128
EDGE_NS = (1, 127, 128, 129, 255, 256, 257)

Case = collections.namedtuple('Case', 'name group N family k')

BASE = [Case('N9', 'BASE', BASE_N, None, 0)]
N_EDGE = [Case(f'N{n}', 'N_EDGE', n, None, 0) for n in EDGE_NS]
MAGNITUDE = [Case(f'{fam}_k{k}', 'MAGNITUDE', BASE_N, fam, k) for fam in ('mlp', 'obj') for k in (6, 10)]
SCALE = [Case('fuse_k20', 'SCALE', BASE_N, 'fuse', 20), Case('fuse_k40', 'SCALE', BASE_N, 'fuse', 40), Case('clue_k20', 'SCALE', BASE_N, 'clue', 20)]
CASES = {c.name: c for c in BASE + N_EDGE + MAGNITUDE + SCALE}
assert len(CASES) == len(BASE + N_EDGE + MAGNITUDE + SCALE)
# (case, kind) whose bound cannot tell the 11-bit mutant from the format (at most one per family, never a family's smaller k).  Empty:
# the closest is mlp_k10 / f16x3 -- 2^-10 on matrices of |w| ~ 0.09 that are split-packed unscaled leaves their low halves 0 - 2 bits
# above fp16's subnormal step of 2^-24, the format is down to 12 - 13 bits and MARGIN x model reaches the mutant on three outputs of four;
# face_gaze_score still rejects it (6.6e-4 against 5.9e-4; test_gaze_cases_cpu.py prints all of them).
MUTANT_BLIND = set()


def kinds_of(case):
    """MAGNITUDE is the f16x3 question with fp32 as its control."""
    return ('fp32', 'f16x3') if case.group == 'MAGNITUDE' else tuple(KINDS)


# ------------------------------------------------------------------------------------------------ state dicts and inputs
def family_keys(family):
    """The state-dict keys a family scales."""
    g = f'roi_head.gaze_head.{STAGE}'
    if family == 'mlp':
        return [g + f'.gaze_{c}_{b}.{j}.weight' for c in orc.CLUES for b in ('fcs', 'confidence') for j in (0, 3)]
    if family == 'fuse':
        return [g + '.fc_gaze.weight', g + '.fc_gaze.bias']
    if family == 'clue':
        return [g + f'.fc_{c}.{t}' for c in orc.CLUES for t in ('weight', 'bias')]
    return []                                                   # None, 'obj': the state dict is BASE's


@functools.lru_cache(maxsize=None)
def _case_sd(family, k):
    sd = base_sd()
    keys = family_keys(family)
    if not keys:
        return sd
    out = dict(sd)
    for key in keys:
        out[key] = sd[key] * 2.0 ** -k                          # a power of two: exact
    return out


def case_sd(case):
    """The f32 state dict of a case; one object per (family, k) -- the GPU file keys its packed weights on it."""
    return _case_sd(case.family, case.k) if family_keys(case.family) else base_sd()


@functools.lru_cache(maxsize=None)
def _sd64(family, k):
    g = f'roi_head.gaze_head.{STAGE}.'
    return {key: v.double() for key, v in _case_sd(family, k).items() if key.startswith(g)}


def case_sd64(case):
    return _sd64(case.family, case.k) if family_keys(case.family) else _sd64(None, 0)


@functools.lru_cache(maxsize=None)
def base_obj():
    """test_gaze_head's input: [9, 3, 256] ~ randn, seed 8."""
    return torch.randn(BASE_N, 3, 256, generator=torch.Generator().manual_seed(BASE_SEED))


def rows_of(case):
    """Row n of the case's input is row rows_of(case)[n] of the BASE input."""
    return torch.arange(case.N) % BASE_N


def inputs(case):
    """obj [N, 3, 256], f32."""
    obj = base_obj()[rows_of(case)]
    return obj * 2.0 ** -case.k if case.family == 'obj' else obj


# ------------------------------------------------------------------------------------------------ oracle runs
def stack(d):
    """The oracle's dict -> [4, N, 3] in the slot order of mcg_gaze_head."""
    return torch.stack([d[k] for k in OUTS])


def run_oracle(case, dtype=torch.float64, store=torch.float32, fn=None, **kw):
    """The oracle's gaze head on the case -> [4, N, 3] in ``dtype``.  ``store``: the storage type the input is rounded to first (the
    engine kind's).  ``fn`` replaces oracle.gaze_head (the mutants); ``kw`` goes to it (``linear=``)."""
    sd = case_sd64(case) if dtype == torch.float64 else case_sd(case)
    obj = inputs(case).to(store).to(dtype)
    with torch.no_grad():
        return stack((fn or orc.gaze_head)(sd, STAGE, obj, **kw))


def _unrolled(case):
    """N_EDGE -> the 9-row case that holds its expected values."""
    return CASES['N9'] if case.group == 'N_EDGE' else case


@functools.lru_cache(maxsize=None)
def reference(name, store=torch.float32):
    """The float64 oracle on the case's input as the engine kind stores it.  N_EDGE: the BASE reference's rows, by construction
    (test_gaze_cases_cpu.py checks the oracle run on all N rows against it)."""
    case = CASES[name]
    if case.group == 'N_EDGE':
        return reference('N9', store)[:, rows_of(case)]
    return run_oracle(case, store=store)


@functools.lru_cache(maxsize=None)
def raw(name, store=torch.float32):
    """The float64 oracle's un-normalised vectors [4, N, 3] (fused, face, eyes, head) and confidences [3, N, 3]."""
    case = CASES[name]
    if case.group == 'N_EDGE':
        v, c = raw('N9', store)
        return v[:, rows_of(case)], c[:, rows_of(case)]
    with torch.no_grad():
        _, r = orc.gaze_head(case_sd64(case), STAGE, inputs(case).to(store).double(), return_raw=True)
    return torch.stack([r['fused']] + r['gaze']), torch.stack(r['conf'])


def row_err(out, ref):
    """[4, N]: max |d| over a row's three components, per output."""
    return (out.detach().double().cpu() - ref.double()).abs().amax(dim=-1)


def errors(out, ref):
    """{output: the worst row's max |d|} -- GAZE_TOL's metric, per output."""
    e = row_err(out, ref).amax(dim=1)
    return {k: float(e[i]) for i, k in enumerate(OUTS)}


@functools.lru_cache(maxsize=None)
def floor(name, store=torch.float32):
    """The f32 CPU oracle against the float64 one, per output.  N_EDGE: BASE's."""
    case = _unrolled(CASES[name])
    return errors(run_oracle(case, dtype=torch.float32, store=store), reference(case.name, store))


@functools.lru_cache(maxsize=None)
def model(name, low=True):
    """The float64 oracle with the f16x3 format model at both MLP layers against plain float64, per output (``low=False``: the 11-bit
    mutant)."""
    case = _unrolled(CASES[name])
    return errors(run_oracle(case, linear=x3_hooks(SITES, low)['linear']), reference(case.name))


def bound(name, kind):
    """{output: bound} for one engine kind.
    BASE, N_EDGE, SCALE, MAGNITUDE fp32:  GAZE_TOL[kind] + floor
    MAGNITUDE f16x3:                      GAZE_TOL['f16x3'] + floor + MARGIN x model"""
    case = CASES[name]
    fl = floor(name, KIND_DTYPE[kind])
    b = {k: GAZE_TOL[kind] + fl[k] for k in OUTS}
    if case.group == 'MAGNITUDE' and kind == 'f16x3':
        m = model(name)
        b = {k: b[k] + MARGIN * m[k] for k in OUTS}
    return b
