"""-m gpu: the deferred FPN P2 LATERAL (engine option fpn_lateral_deferred, on top of fpn_deferred).  The decoder computes the P2 inner map
(lateral(C2) + bias + nearest-upsampled P3 inner map) only for the 8 x 8 blocks the deferred output conv reads -- the listed output blocks and
their in-frame neighbours -- with the streaming lateral's per-pixel code over a device list (pw_single_x3_blocks_kernel).  Everything is
asserted BIT FOR BIT against the dense lateral; a slot whose inner map holds NaN before the decoder shows which pixels were written."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from mcgaze_amd import synth
from mcgaze_amd.engine import HipEngine, PipelinedRunner, _ptr, _ws

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
KEYS = ('gaze', 'boxes', 'scores')

# init proposals (cx, cy, w, h, normalised).  'partial': a small box in the top-left image corner, a small box on the bottom edge (its
# blocks' lower neighbours would be the next frame's first block row), a box larger than the image (another level).  'whole': P2 boxes that
# cover the image.  'coarse': boxes routed to P3 - P5 only
BOXES = {
    'partial': [[0.05, 0.05, 0.1, 0.1], [0.45, 0.93, 0.1, 0.1], [0.5, 0.5, 1.8, 1.6]],
    'whole': [[0.5, 0.5, 1.0, 1.0]] * 3,
    'coarse': [[0.5, 0.5, 2.0, 2.5], [0.4, 0.6, 2.2, 2.2], [0.5, 0.5, 3.0, 2.0]],
}


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in KEYS)


def dilate(listed):
    """listed [N, by, bx] bool -> the inner blocks the listed output blocks read: a 3 x 3 dilation per frame (never across frames)."""
    n, by, bx = listed.shape
    pad = np.zeros((n, by + 2, bx + 2), dtype=bool)
    pad[:, 1:-1, 1:-1] = listed
    out = np.zeros_like(listed)
    for dy in range(3):
        for dx in range(3):
            out |= pad[:, dy:dy + by, dx:dx + bx]
    return out


_ENGINES = {}


def engine(boxes=None):
    if boxes not in _ENGINES:
        sd = synth.make_state_dict(0, family='trained' if boxes else 'uniform')
        if boxes:
            sd['rpn_head.init_proposal_bboxes.weight'] = np.array(BOXES[boxes], dtype=np.float32)
        _ENGINES[boxes] = HipEngine(sd, precision='f16x3')
    return _ENGINES[boxes]


def options(eng, deferred, lateral):
    eng.set_option('fpn_deferred', deferred)
    eng.set_option('fpn_lateral_deferred', lateral)


def forward(eng, img, T, deferred, lateral):
    options(eng, deferred, lateral)
    out = eng.forward(img, T)
    torch.cuda.synchronize()
    options(eng, 1, 1)
    return {k: v.clone() for k, v in out.items()}


class Slot:
    """One deferred pyramid slot under the engine's CURRENT options, and views of what it holds."""

    def __init__(self, eng, N, H, W):
        lib, h = eng.lib, eng._handle
        self.eng, self.N, self.H, self.W = eng, N, H, W
        self.mem = _ws(lib.mcg_deferred_pyramid_bytes(h, N, H, W), DEV)
        self.mem.zero_()
        lv, flag = (C.c_void_p * 4)(), C.c_int(-1)
        L.check(lib.mcg_deferred_pyramid_levels(h, _ptr(self.mem), N, H, W, lv, C.byref(flag)), 'levels')
        assert flag.value == 1, 'P2 is not deferred at this shape'
        inner, flags, counts, lists = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nblk, lat = C.c_int(), C.c_int()
        L.check(lib.mcg_deferred_pyramid_state(h, _ptr(self.mem), N, H, W, C.byref(inner), C.byref(flags), C.byref(counts), C.byref(lists),
                                               C.byref(nblk), C.byref(lat)), 'state')
        self.lateral, self.nblk, self.stages = lat.value, nblk.value, 4
        base = self.mem.data_ptr()
        px = N * (H // 4) * (W // 4) * 256 * 4
        self.p2 = self.view(lv[0] - base, px, torch.float32).view(N, H // 4, W // 4, 256)
        self.inner = self.view(inner.value - base, px, torch.float32).view(N, H // 4, W // 4, 256)
        assert self.nblk == N * (H // 32) * (W // 32)
        if self.lateral:
            self.flags = self.view(flags.value - base, 4 * self.nblk, torch.int32)
            self.counts = self.view(counts.value - base, 4 * self.stages, torch.int32)
            self.lists = self.view(lists.value - base, 4 * self.nblk * self.stages, torch.int32).view(self.stages, self.nblk)

    def view(self, off, nbytes, dtype):
        assert 0 <= off and off + nbytes <= self.mem.numel()
        return self.mem[off:off + nbytes].view(dtype)

    def trunk(self, img):
        eng, lib = self.eng, self.eng.lib
        tws = _ws(lib.mcg_trunk_workspace_bytes(eng._handle, self.N, self.H, self.W, 0), DEV)
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        L.check(lib.mcg_backbone_fpn_forward_deferred(eng._handle, stream, _ptr(img), self.N, self.H, self.W, 0, _ptr(self.mem), self.mem.numel(),
                                                      _ptr(tws), tws.numel()), 'trunk')
        torch.cuda.synchronize()

    def decoder(self, T):
        eng, lib = self.eng, self.eng.lib
        dws = _ws(lib.mcg_decoder_workspace_bytes(eng._handle, self.N), DEV)
        N = self.N
        out = dict(gaze=torch.empty(4, N, 3, device=DEV), boxes=torch.empty(N, 3, 4, device=DEV), scores=torch.empty(N, 3, device=DEV))
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        L.check(lib.mcg_decoder_forward_deferred(eng._handle, stream, _ptr(self.mem), self.mem.numel(), N, T, self.H, self.W, None, _ptr(out['gaze']),
                                                 _ptr(out['boxes']), _ptr(out['scores']), _ptr(dws), dws.numel()), 'decoder')
        torch.cuda.synchronize()
        return out

    def blocks(self, t):
        """[N, h, w, 256] -> [N, by, bx, 8 * 8 * 256]"""
        N, h, w, c = t.shape
        return t.view(N, h // 8, 8, w // 8, 8, c).permute(0, 1, 3, 2, 4, 5).reshape(N, h // 8, w // 8, -1)


_RUNS = {}


def poisoned_run(boxes, N, T, H, W, seed=21):
    """One forward with the lateral deferred through a slot whose inner map and P2 are NaN before the decoder; the dense inner map of the
    same input; the fully dense outputs.  Computed once per case and shared (read-only) by the tests below."""
    key = (boxes, N, T, H, W, seed)
    if key in _RUNS:
        return _RUNS[key]
    eng = engine(boxes)
    img = torch.from_numpy(synth.make_clips(seed, N // T, T, H, W)).to(DEV)
    ref = forward(eng, img, T, 0, 0)
    options(eng, 1, 0)
    dense = Slot(eng, N, H, W)
    assert dense.lateral == 0
    dense.trunk(img)                       # the dense lateral: the whole inner map
    options(eng, 1, 1)
    slot = Slot(eng, N, H, W)
    assert slot.lateral == 1, 'the P2 lateral is not deferred at this shape'
    slot.trunk(img)
    slot.inner.fill_(float('nan'))
    slot.p2.fill_(float('nan'))
    out = slot.decoder(T)
    r = dict(
        out=out, ref=ref,
        inner=slot.blocks(slot.inner).cpu(), dense=slot.blocks(dense.inner).cpu(),
        listed=torch.isfinite(slot.blocks(slot.p2)).all(dim=-1).cpu().numpy(),          # output blocks some stage computed
        flags=slot.flags.cpu().numpy().copy(), counts=slot.counts.cpu().numpy().copy(), lists=slot.lists.cpu().numpy().copy(),
        shape=(N, H // 32, W // 32))
    _RUNS[key] = r
    return r


# (init boxes, frames, clip length, H, W): 4 x 4 blocks per frame on the generic contraction kernel's side of the dense lateral; 7 x 7 blocks
# with 21 frames = 65 856 pixels, where the dense lateral IS pw_single_x3_kernel<16, 2, 2> (>= 64 Ki pixels)
PARTIAL = [('partial', 3, 3, 128, 128), ('partial', 21, 7, 224, 224)]


@pytest.mark.parametrize('case', PARTIAL, ids=lambda c: f'{c[1]}x{c[3]}x{c[4]}')
def test_inner_map_bitwise(case):
    r = poisoned_run(*case)
    N, by, bx = r['shape']
    listed = r['listed']
    want = dilate(listed)
    # the case is what it is meant to be: a corner block, a block on the bottom edge whose lower neighbour would be the next frame's first
    # row -- which stays unwritten there --, and neither nothing nor everything
    assert listed[:, 0, 0].all() and listed[:-1, by - 1, :].any(axis=1).all()
    assert 0 < want.sum() < want.size and listed.sum() < want.sum()
    f, col = 0, int(np.flatnonzero(listed[0, by - 1])[-1])
    cross = [c for c in (col - 1, col, col + 1) if 0 <= c < bx and not want[f + 1, 0, c]]
    assert cross, 'no block of the next frame distinguishes a frame-crossing neighbour'
    nan = torch.isnan(r['inner'])
    eq = (bits(r['inner']) == bits(r['dense'])).all(dim=-1).numpy()
    assert np.array_equal(eq, want), 'inner blocks of the dilated set differ from the dense lateral (or others were written)'
    assert bool(nan[torch.from_numpy(~want)].all()), 'an inner pixel outside the dilated set was written'
    assert not bool(nan[torch.from_numpy(want)].any())
    assert same(r['out'], r['ref'])


@pytest.mark.parametrize('case', PARTIAL, ids=lambda c: f'{c[1]}x{c[3]}x{c[4]}')
def test_no_duplicate_work(case):
    r = poisoned_run(*case)
    counts, flags, lists = r['counts'], r['flags'], r['lists']
    assert counts.min() >= 0 and counts.sum() == (flags != 0).sum() > 0
    ids = np.concatenate([lists[st, :counts[st]] for st in range(len(counts))])
    assert len(np.unique(ids)) == len(ids), 'a block is on two lists'
    assert np.array_equal(np.sort(ids), np.flatnonzero(flags)), 'the lists are not the flagged blocks'
    assert np.array_equal(flags.reshape(r['shape']) != 0, dilate(r['listed']))


def test_whole_image():
    """Boxes covering the image: every inner block is computed and the inner map is the dense one everywhere."""
    r = poisoned_run('whole', 4, 2, 64, 96)
    assert r['listed'].all() and (r['flags'] != 0).all()
    assert torch.equal(bits(r['inner']), bits(r['dense']))
    assert same(r['out'], r['ref'])


def test_no_p2_box():
    """Boxes that map to P3 - P5 only: the lateral launches write nothing, and the outputs are the dense path's."""
    r = poisoned_run('coarse', 4, 2, 64, 96)
    assert not r['listed'].any() and r['counts'].sum() == 0 and not r['flags'].any()
    assert bool(torch.isnan(r['inner']).all())
    assert same(r['out'], r['ref'])


@pytest.mark.parametrize('seed,size', [(0, 128), (1, 224)])
@pytest.mark.parametrize('lengths', [7, [3, 7, 4]], ids=['uniform', 'ragged'])
def test_forward_bitwise(seed, size, lengths):
    eng = engine()
    img = torch.from_numpy(synth.make_clips(seed, 2, 7, size, size)).to(DEV)
    options(eng, 1, 1)
    assert Slot(eng, 14, size, size).lateral == 1
    a, b, c = (forward(eng, img, lengths, *o) for o in ((1, 1), (1, 0), (0, 0)))
    assert same(a, b) and same(a, c)


def test_pipelined_runner_slot_lifetime():
    """Four submits alternating two inputs through the two slots: nothing the decoder reads lives in the trunk workspace, which the next
    batch's trunk overwrites while this batch's decoder runs."""
    eng = engine()
    N, T = 14, 7
    imgs = [torch.from_numpy(synth.make_clips(s, 2, T)).to(DEV) for s in (31, 32)]
    ref = [forward(eng, x, T, 0, 0) for x in imgs]
    options(eng, 1, 1)
    runner = PipelinedRunner(eng, N, 224, 224, T)
    order = [0, 1, 0, 1]
    outs = [dict(gaze=torch.empty(4, N, 3, device=DEV), boxes=torch.empty(N, 3, 4, device=DEV), scores=torch.empty(N, 3, device=DEV))
            for _ in order]
    for i, o in zip(order, outs):
        runner.submit(imgs[i], o)
    runner.flush()
    torch.cuda.synchronize()
    for i, o in zip(order, outs):
        assert same(o, ref[i])
