"""-m gpu: the three kernels of the deferred FPN P2 path on their own -- roi_mark_kernel (mcg_roi_mark_blocks), inner_mark_kernel
(mcg_inner_mark_blocks), wino_x3w_blocks_kernel (mcg_conv3x3_wino_x3_blocks) -- without the engine around them.  tests/defer_cases.py holds
the statements and the cases, tests/test_defer_cases_cpu.py proves them on the CPU and names the wrong rules they reject.  Every assertion
here is a set equality or a bit equality: there is no tolerance.

  marking            set(list[:count]) == the footprint statement (neither short of a block nor a superset), no duplicates, state == its
                     indicator; a second call that shares state lists the new blocks only; a full state lists nothing; a non-zero count is
                     appended to
  marking / reader   mcg_roi_align over a map that is NaN outside the listed blocks returns the bits it returns over the whole map: a tap
                     outside the listed set, of weight zero included, would show as NaN
  inner marking      the listed set == the in-frame 3 x 3 dilation of the given list minus what state held; out_count > nblk is clamped;
                     negative ids are skipped
  block conv         an int64 statement on the listed blocks and the sentinel elsewhere, for every group padding, frame seam, unit count and
                     grid size; and the bits of the raster tile (mcg_conv3x3_wino_x3) on the same pixels, on randn inputs
  chain              mark -> inner mark -> listed lateral -> listed conv -> RoIAlign on NaN-initialised maps == the dense chain's RoIAlign

The tests never pass a block id outside the map or a count above a list's capacity.
"""
import functools

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from tests import defer_cases as D
from tests import exact_cases as X

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def eng():
    from mcgaze_amd import engine
    return engine


def _i32(values, n=None):
    t = torch.zeros(len(values) if n is None else n, dtype=torch.int32, device=DEV)
    if len(values):
        t[:len(values)] = torch.tensor(list(values), dtype=torch.int32)
    return t


def _boxes(grid):
    return torch.tensor(grid, dtype=torch.float32, device=DEV)


def _listed(blist, count, first=0):
    """The host's view of a device list: entries [first, count) -> list of ids; the count stays within the buffer."""
    n = int(count.cpu()[0])
    assert first <= n <= blist.numel(), (first, n, blist.numel())
    return blist.cpu()[first:n].tolist()


def _indicator(ids, n):
    t = torch.zeros(n, dtype=torch.int32)
    t[sorted(ids)] = 1
    return t


# ------------------------------------------------------------------------------------------------ marking
@pytest.mark.parametrize('name', D.MARK_CASES)
def test_marking_is_the_footprint(eng, name):
    """One call per map: the listed set is the statement's, nothing is listed twice, state is the indicator of the set."""
    case = D.mark_case(name)
    state, blist, count = eng.roi_mark_blocks(_boxes(case.boxes), case.hw)
    torch.cuda.synchronize()
    got = _listed(blist, count)
    want = case.footprint()
    assert len(got) == len(set(got)), f'{name}: a block is listed twice'
    assert set(got) == want, (name, 'missing', sorted(want - set(got)), 'not in the footprint', sorted(set(got) - want))
    assert torch.equal(state.cpu(), _indicator(want, case.nblk))


@pytest.mark.parametrize('name', D.MARK_CASES)
def test_marking_second_call_lists_the_new_blocks_only(eng, name):
    """As the decoder's stages do: the state is shared, list and count are fresh.  Call 1 has every other box of every other frame, the
    rest replaced by a box without a footprint; call 2 has all boxes and lists what call 1 did not."""
    case = D.mark_case(name)
    early = lambda i: i % 2 == 0 and (i // case.bpf) % 2 == 0
    flat = [b if early(i) else D.OUTSIDE for i, b in enumerate(case.flat())]
    first = [flat[f * case.bpf:(f + 1) * case.bpf] for f in range(case.frames)]
    state, l1, c1 = eng.roi_mark_blocks(_boxes(first), case.hw)
    _, l2, c2 = eng.roi_mark_blocks(_boxes(case.boxes), case.hw, state=state)
    torch.cuda.synchronize()
    want1, want = case.footprint(keep=early), case.footprint()
    got1, got2 = _listed(l1, c1), _listed(l2, c2)
    assert want1 and want - want1, 'the split leaves one call without blocks'
    assert len(got1) == len(set(got1)) and set(got1) == want1
    assert len(got2) == len(set(got2)) and set(got2) == want - want1
    assert torch.equal(state.cpu(), _indicator(want, case.nblk))


def test_marking_full_state_and_nonzero_count(eng):
    case = D.mark_case('edge56')
    boxes = _boxes(case.boxes)
    full = torch.ones(case.nblk, dtype=torch.int32, device=DEV)
    _, blist, count = eng.roi_mark_blocks(boxes, case.hw, state=full)
    # a count of 5 and a list that already holds five entries: the call appends behind them
    pre = [-11, -12, -13, -14, -15]
    blist2, count2 = _i32(pre, case.nblk + len(pre)), _i32([len(pre)])
    state2, _, _ = eng.roi_mark_blocks(boxes, case.hw, blist=blist2, count=count2)
    torch.cuda.synchronize()
    assert _listed(blist, count) == [] and bool((full == 1).all())
    want = case.footprint()
    assert int(count2.cpu()[0]) == len(pre) + len(want)
    assert blist2.cpu()[:len(pre)].tolist() == pre
    got = _listed(blist2, count2, first=len(pre))
    assert len(got) == len(set(got)) and set(got) == want and torch.equal(state2.cpu(), _indicator(want, case.nblk))


# ------------------------------------------------------------------------------------------------ marking against the reader
@pytest.mark.parametrize('name', D.MARK_CASES)
def test_roi_align_reads_listed_blocks_only(eng, name):
    """RoIAlign over a level-0 map that is NaN outside the blocks mcg_roi_mark_blocks listed agrees in every bit with RoIAlign over the
    whole map, for every edge box: 0 * NaN = NaN, so a tap outside the listed set shows whatever its weight."""
    case = D.mark_case(name)
    g = torch.Generator().manual_seed(8100 + len(name))
    C = 8
    feats = [torch.randn(case.frames, h, w, C, generator=g).to(DEV) for h, w in case.pyramid]
    boxes = _boxes(case.boxes)
    _, blist, count = eng.roi_mark_blocks(boxes, case.hw)
    torch.cuda.synchronize()
    ids = _listed(blist, count)
    H, W = case.hw
    keep = D.listed_pixels((case.frames, H, W), ids).to(DEV)
    assert 0 < int(keep.sum()) < keep.numel() or name == 'frame'
    poisoned = torch.where(keep[..., None], feats[0], torch.full_like(feats[0], float('nan')))
    full, lv = eng.roi_align(feats, boxes)
    part, lv2 = eng.roi_align([poisoned] + feats[1:], boxes)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(full).any())
    assert torch.equal(lv.cpu(), lv2.cpu()) and lv.cpu().tolist() == case.levels
    assert torch.equal(full.view(torch.int32).cpu(), part.view(torch.int32).cpu()), f'{name}: RoIAlign reads outside the listed blocks'


# ------------------------------------------------------------------------------------------------ inner marking
@pytest.mark.parametrize('frames,H,W', D.INNER_MAPS)
def test_inner_marking_is_the_dilation(eng, frames, H, W):
    nblk = frames * D.blocks_of((H, W))[0] * D.blocks_of((H, W))[1]
    runs = []
    for name, ids in D.inner_lists(frames, (H, W)).items():
        held = set(ids[::2])                                  # what an earlier stage computed: every other listed block
        state = _indicator(held, nblk).to(DEV)
        runs.append((name, ids, held, eng.inner_mark_blocks(_i32(ids, nblk), _i32([len(ids)]), (H, W), frames, state=state)))
        runs.append((name, ids, set(), eng.inner_mark_blocks(_i32(ids, nblk), _i32([len(ids)]), (H, W), frames)))
    torch.cuda.synchronize()
    for name, ids, held, (state, blist, count) in runs:
        got = _listed(blist, count)
        want = D.dilate(ids, frames, (H, W))
        assert len(got) == len(set(got)) and set(got) == want - held, (name, sorted(set(got) ^ (want - held)))
        assert torch.equal(state.cpu(), _indicator(want | held, nblk)), name


def test_inner_marking_clamps_the_count_and_skips_negative_ids(eng):
    frames, H, W = 3, 16, 24
    nblk = 18
    # out_count larger than nblk: the first nblk entries are read (the buffer is nblk long), no more
    every = list(np.random.RandomState(8200).permutation(nblk))
    s1, l1, c1 = eng.inner_mark_blocks(_i32(every), _i32([nblk + 5]), (H, W), frames)
    ids = [3, -1, 7, -5]
    s2, l2, c2 = eng.inner_mark_blocks(_i32(ids, nblk), _i32([len(ids)]), (H, W), frames)
    torch.cuda.synchronize()
    got1, got2 = _listed(l1, c1), _listed(l2, c2)
    assert sorted(got1) == list(range(nblk)) and bool((s1 == 1).all())
    want = D.dilate([3, 7], frames, (H, W))
    assert len(got2) == len(set(got2)) and set(got2) == want and torch.equal(s2.cpu(), _indicator(want, nblk))


# ------------------------------------------------------------------------------------------------ block conv, exact
def _nhwc(t, dtype=torch.float32):
    v = X.nhwc(t).to(dtype)
    assert torch.equal(v.to(torch.int64), X.nhwc(t))
    return v.to(DEV)


@functools.lru_cache(maxsize=None)
def _conv_operands(shape):
    from mcgaze_amd.engine import wino_weights
    x, w, b, _ = D.conv_case(shape)
    return _nhwc(x), wino_weights(X.nhwc(w).float(), 2, DEV), b.float().to(DEV)


@pytest.mark.parametrize('full', [True, False], ids=['bias_relu', 'plain'])
@pytest.mark.parametrize('shape', D.CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_block_conv_is_exact(eng, shape, full):
    """Every list of the shape (and every grid cap of the unit-count lists) over a sentinel-filled y: the int64 statement on the listed
    blocks, the sentinel on every other pixel -- the blocks that only the entries beyond the count name included."""
    frames, H, W, cin, cout = shape
    xd, packed, bd = _conv_operands(shape)
    dense = X.expected(D.conv_case(shape)[3][full], torch.float32)
    outs = []
    for l in D.conv_lists(shape):
        for cap in l.caps:
            y = torch.full((frames, H, W, cout), D.SENTINEL, dtype=torch.float32, device=DEV)
            eng.conv3x3_wino_blocks(xd, packed, (_i32(l.buffer), _i32([len(l.ids)])), y, bias=bd if full else None, relu=full, grid_cap=cap)
            outs.append((l, cap, y))
    torch.cuda.synchronize()
    for l, cap, y in outs:
        X.assert_exact(y, D.conv_expected(shape, l.ids, dense), f'block conv {shape} list "{l.name}" cap={cap} {"bias + relu" if full else "plain"}')


def test_block_conv_refuses_what_it_does_not_support(eng):
    """Host side: H or W that is no multiple of 8, channel counts the tile does not divide -> MCG_ERR_UNSUPPORTED (3), nothing launched."""
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    lib = L.load()
    for n, h, w, cin, cout in ((1, 12, 16, 32, 128), (1, 16, 20, 32, 128), (1, 16, 16, 48, 128), (1, 16, 16, 32, 192)):
        u = torch.zeros(max(int(lib.mcg_conv3x3_wino_x3_weight_bytes(cin - cin % 32 or 32, cout - cout % 128 or 128, 2)) // 2, 1), dtype=torch.float16, device=DEV)
        rc = lib.mcg_conv3x3_wino_x3_blocks(None, z(n, h, w, cin).data_ptr(), u.data_ptr(), None, z(n, h, w, cout).data_ptr(), n, h, w, cin, cout, 0, 0.0,
                                            _i32([0]).data_ptr(), _i32([0]).data_ptr(), 1, 0)
        assert rc == 3, (h, w, cin, cout, rc)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ block conv against the raster tiles
@pytest.mark.parametrize('shape', D.RASTER_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_block_conv_has_the_raster_tiles_bits(eng, shape):
    """wino_x3.hpp: "a block's bits are those of the same pixels in wino_x3w_kernel" -- on randn inputs and weights, all blocks (permuted)
    and a sparse list, against mcg_conv3x3_wino_x3 with the tile chosen by grid size."""
    frames, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(8300 + H)
    x = torch.randn(frames, H, W, cin, generator=g).to(DEV)
    w = torch.randn(cout, 3, 3, cin, generator=g) * (9 * cin) ** -0.5
    b = torch.randn(cout, generator=g).to(DEV)
    packed = eng.wino_weights(w, 2, DEV)
    nblk = D.conv_nblk(shape)
    every = [int(v) for v in np.random.RandomState(8300 + nblk).permutation(nblk)]
    sparse = D.sparse_list(shape)
    dense = eng.conv3x3_wino(x, w.to(DEV), b, relu=True, tile=0)
    nan = float('nan')
    y_all = eng.conv3x3_wino_blocks(x, packed, (_i32(every, nblk + 1), _i32([nblk])), torch.full_like(dense, nan), bias=b, relu=True)
    y_sp = eng.conv3x3_wino_blocks(x, packed, (_i32(sparse, nblk), _i32([len(sparse)])), torch.full_like(dense, D.SENTINEL), bias=b, relu=True)
    torch.cuda.synchronize()
    dense = dense.cpu()
    assert not bool(torch.isnan(dense).any()) and 0 < len(sparse) < nblk
    assert torch.equal(y_all.cpu().view(torch.int32), dense.view(torch.int32)), 'all blocks'
    want = D.conv_expected(shape, sparse, dense)
    assert torch.equal(y_sp.cpu().view(torch.int32), want.view(torch.int32)), 'sparse list'


# ------------------------------------------------------------------------------------------------ the chain
def test_deferred_chain_equals_the_dense_chain(eng):
    """(2, 56, 56) level 0, C = 256: mark -> inner mark -> the streaming lateral's list form -> the block conv -> RoIAlign, on inner and P2
    maps that start as NaN, against dense lateral + dense conv + RoIAlign: the RoIAlign outputs agree in every bit (and hold no NaN: every
    pixel a box reads was computed, from inner pixels that were computed)."""
    case = D.chain_case()
    frames, (H, W), C = case.frames, case.hw, 256
    g = torch.Generator().manual_seed(8400)
    c2 = torch.randn(frames * H * W, C, generator=g).to(DEV)
    p3_inner = torch.randn(frames, H // 2, W // 2, C, generator=g).to(DEV)
    lat_w, lat_b = torch.randn(C, C, generator=g) * C ** -0.5, torch.randn(C, generator=g).to(DEV)
    out_w, out_b = torch.randn(C, 3, 3, C, generator=g) * (9 * C) ** -0.5, torch.randn(C, generator=g).to(DEV)
    upper = [torch.randn(frames, h, w, C, generator=g).to(DEV) for h, w in case.pyramid[1:]]
    wf, wscale = eng.pointwise_weights(lat_w, torch.float32, split=True, device=DEV)
    packed = eng.wino_weights(out_w, 2, DEV)
    boxes = _boxes(case.boxes)
    lateral = dict(residual=p3_inner, residual_mode=L.RES_UPSAMPLE_ADD, out_hw=(H, W), split=True, wscale=wscale)

    inner = eng.pointwise_stream(c2, wf, lat_b, C, **lateral).view(frames, H, W, C)
    p2 = eng.conv3x3_wino(inner, out_w.to(DEV), out_b, tile=0)
    want, _ = eng.roi_align([p2] + upper, boxes)

    nan = float('nan')
    _, blist, count = eng.roi_mark_blocks(boxes, (H, W))
    _, ilist, icount = eng.inner_mark_blocks(blist, count, (H, W), frames)
    inner_d = torch.full((frames * H * W, C), nan, dtype=torch.float32, device=DEV)
    eng.pointwise_stream(c2, wf, lat_b, C, blocks=(ilist, icount), out=inner_d, **lateral)
    p2_d = eng.conv3x3_wino_blocks(inner_d.view(frames, H, W, C), packed, (blist, count), torch.full_like(p2, nan), bias=out_b)
    got, _ = eng.roi_align([p2_d] + upper, boxes)
    torch.cuda.synchronize()

    ids, inner_ids = _listed(blist, count), _listed(ilist, icount)
    assert set(ids) == case.footprint() and set(inner_ids) == D.dilate(ids, frames, (H, W)) and len(set(inner_ids)) == len(inner_ids)
    assert 0 < len(ids) < len(inner_ids) < case.nblk                      # the NaN really is there: part of both maps is never computed
    assert bool(torch.isnan(p2_d).any()) and bool(torch.isnan(inner_d).any())
    assert not bool(torch.isnan(want).any())
    assert torch.equal(got.cpu().view(torch.int32), want.cpu().view(torch.int32))
    # the computed part of both maps carries the dense maps' bits; the rest is untouched
    keep = D.listed_pixels((frames, H, W), ids)
    assert torch.equal(p2_d.cpu()[keep].view(torch.int32), p2.cpu()[keep].view(torch.int32)) and bool(torch.isnan(p2_d.cpu()[~keep]).all())
    ikeep = D.listed_pixels((frames, H, W), inner_ids)
    assert torch.equal(inner_d.view(frames, H, W, C).cpu()[ikeep].view(torch.int32), inner.cpu()[ikeep].view(torch.int32))
    assert bool(torch.isnan(inner_d.view(frames, H, W, C).cpu()[~ikeep]).all())
