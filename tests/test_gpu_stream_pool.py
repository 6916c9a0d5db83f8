"""-m gpu: many live streams on one pyramid store -- mcg_pyramid_scatter_rows (a batch's pyramid into arbitrary rows),
HipEngine.backbone_fpn_rows, stream.GazeStreamPool.  Everything here is asserted BIT FOR BIT: a scattered row against the frame it
came from, a pool's stream against a lone GazeStream fed the same frames.  No test hands the decoder an out-of-range table; the scatter's
skip of a frame without a row is part of its interface and is checked as such."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from mcgaze_amd import synth
from mcgaze_amd.stream import GazeStream, GazeStreamPool

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PRECISIONS = ('fp32', 'f16x3', 'bf16', 'f16')


@pytest.fixture(scope='module')
def engines():
    from mcgaze_amd.engine import HipEngine
    sd = synth.make_state_dict(0)
    return {p: HipEngine(sd, precision=p) for p in PRECISIONS}


def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def scatter(code, src, dst, row_of, H, W):
    lib = L.load()
    table = torch.tensor(row_of, dtype=torch.int32, device=DEV)
    sp = (C.c_void_p * 4)(*[t.data_ptr() for t in src])
    dp = (C.c_void_p * 4)(*[t.data_ptr() for t in dst])
    L.check(lib.mcg_pyramid_scatter_rows(C.c_void_p(torch.cuda.current_stream().cuda_stream), code, sp, dp, src[0].shape[0], dst[0].shape[0], H, W,
                                         C.c_void_p(table.data_ptr())), 'mcg_pyramid_scatter_rows')
    torch.cuda.synchronize()


@pytest.mark.parametrize('H,W', [(32, 32), (64, 96)])
@pytest.mark.parametrize('dtype,code', [(torch.float32, L.MCG_F32), (torch.bfloat16, L.MCG_BF16)])
def test_scatter_rows(H, W, dtype, code):
    """3 frames into a NaN-poisoned 5-row store.  32 x 32: levels 8^2 .. 1^2, the 16-bit 1 x 1 row is 512 bytes, the smallest slice; the
    8^2 f32 level is 4 slices of 16 KiB; 64 x 96: levels that are no whole number of slices."""
    g = torch.Generator().manual_seed(H + W)
    it = torch.int16 if dtype == torch.bfloat16 else torch.int32
    shapes = [((H // 4) >> i, (W // 4) >> i, 256) for i in range(4)]
    src = [torch.randint(-30000, 30000, (3,) + s, generator=g, dtype=it).to(DEV).view(dtype) for s in shapes]    # any bit pattern
    dst = [torch.full((5,) + s, float('nan'), dtype=dtype, device=DEV) for s in shapes]
    scatter(code, src, dst, [4, 0, 2], H, W)
    for lvl in range(4):
        for n, r in enumerate([4, 0, 2]):
            assert torch.equal(bits(dst[lvl][r]), bits(src[lvl][n])), (lvl, n, r)
        assert bool(torch.isnan(dst[lvl][[1, 3]]).all()), lvl
    before = [d.clone() for d in dst]
    scatter(code, src, dst, [1, -1, 7], H, W)               # frames 1 and 2 have no row: skipped
    for lvl in range(4):
        assert torch.equal(bits(dst[lvl][1]), bits(src[lvl][0])), lvl
        assert torch.equal(bits(dst[lvl][[0, 2, 3, 4]]), bits(before[lvl][[0, 2, 3, 4]])), lvl


@pytest.mark.parametrize('precision', ['f16x3', 'f16'])
def test_backbone_fpn_rows_equals_the_contiguous_call(engines, precision):
    e = engines[precision]
    x = torch.from_numpy(synth.make_clips(21, 1, 4, 64, 64)).to(DEV)
    ref = [p.clone() for p in e.backbone_fpn(x)]
    rows = [3, 0, 2, 5]
    store = [torch.full((6, 16 >> i, 16 >> i, 256), float('nan'), dtype=e.dtype, device=DEV) for i in range(4)]
    assert e.backbone_fpn_rows(x, store, rows) is store
    torch.cuda.synchronize()
    for lvl in range(4):
        for n, r in enumerate(rows):
            assert torch.equal(bits(store[lvl][r]), bits(ref[lvl][n])), (precision, lvl, n)
        assert bool(torch.isnan(store[lvl][[1, 4]].float()).all()), (precision, lvl)
    # a second call into other rows reuses the engine's scratch and leaves the rows of the first alone
    e.backbone_fpn_rows(x[:2], store, [4, 1])
    torch.cuda.synchronize()
    for lvl in range(4):
        for n, r in ((0, 4), (1, 1), (0, 3), (1, 0), (2, 2), (3, 5)):
            assert torch.equal(bits(store[lvl][r]), bits(ref[lvl][n])), (precision, lvl, n, r)
    # rows that are one ascending run are written in place by the trunk, without the copy: the same bits, the other rows untouched
    e.backbone_fpn_rows(x[2:], store, [0, 1])
    torch.cuda.synchronize()
    for lvl in range(4):
        for n, r in ((2, 0), (3, 1), (2, 2), (0, 3), (0, 4), (3, 5)):
            assert torch.equal(bits(store[lvl][r]), bits(ref[lvl][n])), (precision, lvl, n, r)


LENGTHS = [5, 7, 18, 30]


def schedule(seed):
    """A fixed interleaving: ('push', stream, a, b) / ('close', stream) / ('step',).  A stream is closed as soon as its last frame is
    pushed, so the short ones end while the others run on."""
    rs = np.random.RandomState(seed)
    sent, ops = [0] * len(LENGTHS), []
    while any(s < n for s, n in zip(sent, LENGTHS)):
        i = int(rs.choice([k for k, n in enumerate(LENGTHS) if sent[k] < n]))
        n = min(LENGTHS[i] - sent[i], int(rs.randint(1, 7)))
        ops.append(('push', i, sent[i], sent[i] + n))
        sent[i] += n
        if sent[i] == LENGTHS[i]:
            ops.append(('close', i))
        if rs.randint(3):
            ops.append(('step',))
    return ops


@pytest.fixture(scope='module')
def videos():
    return [torch.from_numpy(synth.make_clips(40 + i, 1, n, 64, 64)).to(DEV) for i, n in enumerate(LENGTHS)]


def img_hw_of(n, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(32, 65, n), rs.randint(32, 65, n)], axis=1).astype(np.int32)


@pytest.mark.parametrize('precision,with_hw', [('fp32', False), ('f16x3', False), ('f16x3', True), ('bf16', False), ('f16', False)])
def test_pool_equals_lone_streams(engines, videos, precision, with_hw):
    e = engines[precision]
    limit = 12 if precision == 'f16' else None              # the fp16 decoder keeps its bits below 256 tokens per call
    sf = (1.4, 1.25, 1.4, 1.25)
    hws = [img_hw_of(n, 50 + i) if with_hw else None for i, n in enumerate(LENGTHS)]
    ops = schedule(5)
    # each stream alone: the same pushes, in the same order
    want = []
    for i, v in enumerate(videos):
        s = GazeStream(e, 64, 64, scale_factor=sf, max_decode_windows=limit)
        parts = [s.push(v[a:b], None if hws[i] is None else hws[i][a:b]) for op, j, a, b in (o for o in ops if o[0] == 'push') if j == i]
        want.append(parts + [s.finish()])
    pool = GazeStreamPool(e, 64, 64, rows=40, scale_factor=sf, max_decode_windows=limit)    # 40 rows < 4 x 11 reserved + pushes: recycled
    sids = [pool.open() for _ in LENGTHS]
    got = {s: [] for s in sids}

    def step():
        for s, r in pool.step().items():
            assert r['first'] == sum(p['det'].shape[0] for p in got[s])
            got[s].append(r)
    for op in ops:
        if op[0] == 'push':
            _, i, a, b = op
            pool.push(sids[i], videos[i][a:b], None if hws[i] is None else hws[i][a:b])
        elif op[0] == 'close':
            pool.close(sids[op[1]])
        else:
            step()
    for _ in range(50):
        if not pool.pending():
            break
        step()
    assert not pool.pending() and pool.store.free_rows() == 40
    for i, s in enumerate(sids):
        for k in ('det', 'fused', 'others'):
            a = np.concatenate([p[k] for p in got[s]])
            b = np.concatenate([p[k] for p in want[i]])
            assert a.shape == b.shape and a.shape[0] == LENGTHS[i], (precision, i, k)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (precision, i, k)


def test_one_decoder_call_per_step(engines):
    """Three streams whose first window becomes certain in the same step: ONE decoder call, so one RoIAlign launch per stage over all
    3 x 7 x 3 boxes.  The engine's profile records contraction launches; every stage follows its RoIAlign with exactly one [boxes, 32768,
    256] contraction (the DynamicConv parameters), so those records count the RoIAlign launches and carry their box count."""
    e = engines['f16x3']
    pool = GazeStreamPool(e, 64, 64)
    sids = [pool.open() for _ in range(3)]
    vids = [torch.from_numpy(synth.make_clips(60 + i, 1, 8, 64, 64)).to(DEV) for i in range(3)]
    for s, v in zip(sids, vids):
        pool.push(s, v[:7])
    assert pool.step() == {}
    for s, v in zip(sids, vids):
        pool.push(s, v[7:])
    e.profile_start()
    try:
        res = pool.step()
    finally:
        rec = e.profile_stop()
    assert sorted(res) == sids and all(r['det'].shape[0] == 1 for r in res.values())
    dyn = [r[3] for r in rec if r[3][1:] == (32768, 256)]
    assert dyn == [(63, 32768, 256)] * 4, dyn
