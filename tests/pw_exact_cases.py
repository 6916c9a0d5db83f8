"""Shared by tests/test_pw_exact_cases_cpu.py and tests/test_gpu_pw_exact.py: the streaming 1x1 kernels (pw_single.hpp, pw_single_x3.hpp,
pw_pair.hpp) at SMALL M, through mcg_pointwise_stream / mcg_pointwise_dyn / mcg_pointwise_pair, against int64 statements of the operators.
tests/exact_cases.py holds the generators, the exactness condition, ``expected`` and the comparison; this module adds the forms, the row
counts and the references.

THE FORMS.  Every instantiation the launchers dispatch is named in a table below (STREAM16_FORMS, STREAM_X3_FORMS, LIST_FORM, PAIR_FORMS,
DYN_FORMS) with the template arguments it runs as; tests/test_pw_exact_cases_cpu.py compares the tables with a literal list, both are
reviewed against launch_pw_single_f, launch_pw_single_x3, launch_pw_single_x3_blocks, launch_pw_pair_f, launch_pw_dyn and launch_pw_dyn_x3.

THE ROW COUNTS.  A stream tile is 32 rows and a capped grid (grid_cap = 1) has 8 walkers per channel slice: M = 1, 31, 32, 33 are the
single row, the tile edge and a second walker with one row; M = 753 is 24 tiles, the last of 17 rows, three trips per walker -- both y / A
buffer parities and the reuse of the first.  The pair's tile is 64 rows and grid_cap counts workgroups.  Every dense run stores into a
buffer with GUARD sentinel rows behind row M.

THE REFERENCES.  Stream: exact_cases.conv2d_ref with k = 1.  Pair: y = ONE round-to-nearest-even of relu(a1 . W3a + a2 . W3b + b3 + res),
z = ONE round-to-nearest-even of relu(ROUNDED y . W1 + b1) (``pair_ref``).
"""
import functools

import torch

from tests import exact_cases as X

KINDS16 = ('bf16', 'fp16')
GUARD = 32                 # sentinel rows behind row M of every dense output
SENTINEL = -7.5            # no possible result: every result is an integer
DENSITY = 0.5
# activations x this put rounding ties under the 16-bit store (bf16: odd sums in (256, 512), ...; fp16: sums past 2048) and, for f16x3,
# a non-zero fp16 low half into the split (3 * 683 = 2049)
SCALE = {'bf16': 16, 'fp16': 64, 'f16x3': 683}
# the pair's y has K = 64 (+ 64): its sums pass fp16's 2048 often enough only from x 128 on with one source (x 64: fewer than 100 ties)
PAIR_SCALE = {'bf16': {0: 16, 64: 16}, 'fp16': {0: 128, 64: 64}}

# ------------------------------------------------------------------------------------------------ the dispatched forms
# (K, N, res_mode) -> pw_single_kernel<F, KS, TPW, RES, NSPLIT>: launch_pw_single_f
STREAM16_FORMS = {
    (512, 128, 0): (32, 1, 0, 1),
    (512, 256, 0): (32, 1, 0, 2), (512, 256, 2): (32, 1, 2, 2),
    (256, 256, 0): (16, 2, 0, 1), (256, 256, 1): (16, 2, 1, 1), (256, 256, 2): (16, 2, 2, 1),
    (256, 1024, 0): (16, 2, 0, 4), (256, 1024, 1): (16, 2, 1, 4), (256, 1024, 2): (16, 2, 2, 4),
    (128, 512, 0): (8, 4, 0, 1), (128, 512, 1): (8, 4, 1, 1), (128, 512, 2): (8, 4, 2, 1),
}
# (K, N, res_mode) -> pw_single_x3_kernel<KS, RES, NSPLIT>: launch_pw_single_x3
STREAM_X3_FORMS = {
    (256, 256, 0): (16, 0, 2), (256, 256, 1): (16, 1, 2), (256, 256, 2): (16, 2, 2),
    (256, 1024, 0): (16, 0, 8), (256, 1024, 1): (16, 1, 8), (256, 1024, 2): (16, 2, 8),
}
LIST_FORM = {(256, 256, 2): (16, 2)}                       # pw_single_x3_blocks_kernel<KS, NSPLIT>: launch_pw_single_x3_blocks
PAIR_FORMS = {(0, 64): (1, 1), (0, 128): (1, 2), (64, 64): (2, 1), (64, 128): (2, 2)}     # (K2, C2) -> pw_pair_kernel<F, NSRC, C2T>
DYN_FORMS = {'bf16': (16, 2, 0, 128), 'fp16': (16, 2, 0, 128), 'f16x3': (16, 0, 256)}    # launch_pw_dyn / launch_pw_dyn_x3, K = 256, N = 32768
DYN_K, DYN_N = 256, 32768


def channels_per_workgroup(kind, K, N):
    """The slice of the N output channels one workgroup owns (128 TPW; f16x3: 128)."""
    return 128 if kind == 'f16x3' else 128 * STREAM16_FORMS[(K, N, 0)][1]


def stream_forms(kind):
    return list(STREAM_X3_FORMS if kind == 'f16x3' else STREAM16_FORMS)


# ------------------------------------------------------------------------------------------------ row counts
DENSE_M = (1, 31, 32, 33, 753)
M_MAX = 753
# upsample residual: (frames, Ho, Wo) from (Hr, Wr).  46 from 14 holds the index where torch's rule and the integer rule part (wo = 23 reads
# column 6, not 7); 9 x 11 from 4 x 5 is exact_cases' 'up' map, on which the two rules agree
UP_SHAPES = (((3, 5, 46), (2, 14)), ((2, 9, 11), (4, 5)))
SIZE_PAIRS = sorted({(o, i) for (_, ho, wo), (hr, wr) in UP_SHAPES for o, i in ((ho, hr), (wo, wr))} | {(16, 8), (24, 12)})   # (out, in) of every gather
PAIR_M = ((1, 1), (63, 1), (64, 1), (65, 1), (3 * 64 - 15, 1), (3 * 64 * 2 - 15, 2), (3 * 64 * 2 - 15, 0))   # (M, grid_cap): 177 = 3 trips of one workgroup
PAIR_M_MAX = 3 * 64 * 2 - 15
DYN_M = ((17, 1), (17, 0), (273, 1), (273, 0))             # (M, walkers per slice capped at; 0 = the product rule)
DYN_M_MAX = 273
DYN_SCALED_M = 17
LIST_MAP = ((3, 16, 24), (8, 12))                          # 3 frames of 16 x 24 from 8 x 12: 18 blocks of 8 x 8
LIST_NBLK = 18


def stream_runs(res_mode):
    """-> [(M, index into UP_SHAPES or None, grid_cap)] of a form: every M with one group of walkers, the largest with the product grid too."""
    if res_mode == 2:
        return [(f * ho * wo, i, cap) for i, ((f, ho, wo), _) in enumerate(UP_SHAPES) for cap in (1, 0)]
    return [(m, None, 1) for m in DENSE_M] + [(M_MAX, None, 0)]


def _seed(*key):
    return 9900 + sum((i + 1) * 131 * int(v) for i, v in enumerate(key)) % 100000


# ------------------------------------------------------------------------------------------------ stream: inputs and reference
@functools.lru_cache(maxsize=None)
def stream_inputs(K, N, scale=1):
    """int64, built once and shared -- do not write to them: a [M_MAX][K] (rows of a smaller M are its first M), w [N][K], b [N],
    res [M_MAX][N], up[i] = the residual [frames][N][Hr][Wr] of UP_SHAPES[i]."""
    g = X.gen(_seed(K, N))                         # the seed leaves the scale out: the scaled case is the same draw, activations x scale
    d = dict(a=X.acts(g, (M_MAX, K), scale=scale), w=X.ternary(g, (N, K), DENSITY), b=X.small(g, (N,)), res=X.small(g, (M_MAX, N)))
    d['up'] = [X.small(g, (f, N, hr, wr)) for (f, _, _), (hr, wr) in UP_SHAPES]
    return d


def stream_kwargs(K, N, res_mode, M, up=None, relu=False, scale=1):
    """The case as exact_cases.conv2d_ref's arguments (k = 1): the M rows as a [frames][K][Ho][Wo] map (1 x 1 x M without an upsample)."""
    d = stream_inputs(K, N, scale)
    f, ho, wo = UP_SHAPES[up][0] if up is not None else (1, 1, M)
    assert f * ho * wo == M and M <= M_MAX
    kw = dict(x=d['a'][:M].reshape(f, ho, wo, K).permute(0, 3, 1, 2), w=d['w'][:, :, None, None], b=d['b'], relu=relu, res_mode=res_mode)
    if res_mode == 1:
        kw['res'] = d['res'][:M].reshape(1, 1, M, N).permute(0, 3, 1, 2)
    elif res_mode == 2:
        kw['res'] = d['up'][up]
    return kw


@functools.lru_cache(maxsize=None)
def stream_ref(K, N, res_mode, M, up=None, relu=False, scale=1):
    """-> int64 [M][N]"""
    return X.conv2d_ref(**stream_kwargs(K, N, res_mode, M, up, relu, scale))[0].reshape(M, N)


# one scaled run per form with a residual add (and 512 -> 128, which has none): M_MAX rows, one group of walkers, ReLU
SCALED_STREAM = {'bf16': [(512, 128, 0), (256, 256, 1), (128, 512, 1), (256, 1024, 1)],
                 'fp16': [(512, 128, 0), (256, 256, 1), (128, 512, 1), (256, 1024, 1)],
                 'f16x3': [(256, 256, 1), (256, 1024, 1)]}


# ------------------------------------------------------------------------------------------------ dynamic_layer
@functools.lru_cache(maxsize=None)
def dyn_inputs(scale=1):
    """a [DYN_M_MAX][256] int64; w [32768][256] int8 (8 M elements); b [32768] int64."""
    g = X.gen(_seed(DYN_K, DYN_N))
    return dict(a=X.acts(g, (DYN_M_MAX, DYN_K), scale=scale), w=X.ternary(g, (DYN_N, DYN_K), DENSITY).to(torch.int8), b=X.small(g, (DYN_N,)))


@functools.lru_cache(maxsize=None)
def dyn_ref(scale=1):
    """-> int64 [rows][32768], rows = DYN_M_MAX (rows of a smaller M are its first M; the scaled runs have DYN_SCALED_M), through float64 like
    exact_cases._conv; and the same over absolute values, the exactness bound."""
    d = dyn_inputs(scale)
    a, w = d['a'][:DYN_M_MAX if scale == 1 else DYN_SCALED_M], d['w'].double()
    ref = X._integral(a.double() @ w.t(), 'dynamic_layer') + d['b']
    bound = int((X._integral(a.abs().double() @ w.abs().t(), 'dynamic_layer') + d['b'].abs()).max())
    return ref, bound


# ------------------------------------------------------------------------------------------------ the list form
LISTS = {
    # 11 of the 18 valid ids, shuffled, plus two ids outside the map, which the kernel documents as "nothing read, nothing written"
    'partial': (7, 16, -1, 2, 11, 0, 13, 5, LIST_NBLK, 9, 17, 4, 10),
    'full': (12, 3, 17, 0, 8, 5, 14, 1, 10, 16, 7, 2, 13, 9, 4, 15, 6, 11),
    'empty': (),
}


@functools.lru_cache(maxsize=None)
def list_inputs():
    (f, ho, wo), (hr, wr) = LIST_MAP
    g = X.gen(_seed(f, ho, wo))
    return dict(x=X.acts(g, (f, 256, ho, wo)), w=X.ternary(g, (256, 256, 1, 1), DENSITY), b=X.small(g, (256,)), res=X.small(g, (f, 256, hr, wr)), res_mode=2)


@functools.lru_cache(maxsize=None)
def list_ref():
    """The DENSE reference of the list form's map, int64 [frames][Ho][Wo][256]."""
    return X.conv2d_ref(**list_inputs())[0]


def listed_pixels(ids):
    """bool [frames][Ho][Wo]: the pixels of the valid listed blocks."""
    (f, ho, wo), _ = LIST_MAP
    m = torch.zeros(f, ho, wo, dtype=torch.bool)
    for b in ids:
        if 0 <= b < LIST_NBLK:
            fr, rem = divmod(b, (ho // 8) * (wo // 8))
            by, bx = divmod(rem, wo // 8)
            m[fr, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = True
    return m


def list_expected(ids, dense=None):
    """What y must hold after a list run over a SENTINEL-filled buffer: the dense reference on the listed pixels, the sentinel elsewhere."""
    dense = X.expected(list_ref(), torch.float32) if dense is None else dense
    return torch.where(listed_pixels(ids)[..., None], dense, torch.full_like(dense, SENTINEL))


# ------------------------------------------------------------------------------------------------ the pair
@functools.lru_cache(maxsize=None)
def pair_inputs(K2, C2, scale=1):
    """int64: a1 [PAIR_M_MAX][64] (conv2's output: post-ReLU), a2 [..][64] (the block input, post-ReLU) when K2, w3 [256][64 + K2], b3,
    res [..][256], w1 [C2][256], b1."""
    g = X.gen(_seed(K2, C2, 1, 7))
    return dict(a1=X.acts(g, (PAIR_M_MAX, 64), post_relu=True, scale=scale), a2=X.acts(g, (PAIR_M_MAX, 64), post_relu=True, scale=scale) if K2 else None,
                w3=X.ternary(g, (256, 64 + K2), DENSITY), b3=X.small(g, (256,)), res=X.small(g, (PAIR_M_MAX, 256)),
                w1=X.ternary(g, (C2, 256), DENSITY), b1=X.small(g, (C2,)))


def _mm(a, w):
    return X._integral(a.double() @ w.double().t(), 'pair')


def pair_ref(a1, a2, w3, b3, res, w1, b1, dtype=None):
    """-> (y, y as stored, z), int64: y = relu([a1 | a2] . W3^T + b3 (+ res)); y as stored = ONE RNE of it to ``dtype`` (None: unrounded, for
    the bound over absolute values); z = relu(y as stored . W1^T + b1), itself rounded ONCE by ``expected``."""
    y = _mm(a1, w3[:, :64]) + b3
    if a2 is not None:
        y = y + _mm(a2, w3[:, 64:])
    if res is not None:
        y = y + res
    y = y.clamp_min(0)
    ys = X._integral(X.expected(y, dtype).double(), 'rounded y') if dtype is not None else y
    return y, ys, (_mm(ys, w1) + b1).clamp_min(0)


def pair_args(K2, C2, M, scale=1, with_res=None):
    """The first M rows of the case; a residual where the form has one source (the engine's identity block), unless with_res says otherwise."""
    d = pair_inputs(K2, C2, scale)
    with_res = (K2 == 0) if with_res is None else with_res
    return dict(a1=d['a1'][:M], a2=d['a2'][:M] if K2 else None, w3=d['w3'], b3=d['b3'], res=d['res'][:M] if with_res else None, w1=d['w1'], b1=d['b1'])


def check_pair_exactness(kw, what):
    """The chain over absolute values, unrounded, bounds every partial sum; one rounding of y grows it by at most 2^-8."""
    absd = {k: (v.abs() if torch.is_tensor(v) else v) for k, v in kw.items()}
    worst = max(int(t.max()) for t in pair_ref(**absd))
    assert worst * 257 // 256 < X.LIMIT, f'{what}: sum |x| |w| + |b| + |res| reaches {worst} (x 257 / 256 for the rounded y) >= 2^24'
    return worst


# ------------------------------------------------------------------------------------------------ guard rows
def with_guard(want):
    """[M][N] expected values -> [M + GUARD][N] as the output buffer must read after the run."""
    return torch.cat([want, torch.full((GUARD, want.shape[1]), SENTINEL, dtype=want.dtype)])
