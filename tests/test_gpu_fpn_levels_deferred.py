"""-m gpu: FPN levels deferred by whole frames (engine option fpn_levels_deferred, on top of fpn_deferred): the output convs of P3 .. P5 run in
the decoder, per stage, over the frames one of the stage's boxes reads on that level (roi_mark_kernel's frame marking, then
wino_x3w_frames_kernel).  Everything is asserted BIT FOR BIT against the option off, at 64 x 64 frames (16 / 8 / 4 / 2-pixel maps) with two
clips of 3 frames and a ragged batch; a slot whose P3 .. P5 hold NaN before the decoder shows which frames were written."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from mcgaze_amd import synth
from mcgaze_amd.engine import GraphedForward, HipEngine, _ptr, _ws

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
KEYS = ('gaze', 'boxes', 'scores')
SIZE, N, T = 64, 6, 3
ALL = 14                   # the option's mask of P3 | P4 | P5
# init proposals (cx, cy, w, h, normalised) on a 64-pixel frame.  'mixed': one box each on P3 (128 px), P4 (256 px) and P2; 'huge': P5 (512 px),
# P4 and P3; None: the synthetic model's own (P2 only at this size)
BOXES = {
    'mixed': [[0.5, 0.5, 2.0, 2.0], [0.5, 0.5, 4.0, 4.0], [0.3, 0.3, 0.5, 0.5]],
    'huge': [[0.5, 0.5, 8.0, 8.0], [0.4, 0.6, 4.0, 4.0], [0.5, 0.5, 2.0, 2.0]],
}
CASES = (None, 'mixed', 'huge')


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in KEYS)


_ENGINES = {}


def engine(boxes=None):
    if boxes not in _ENGINES:
        sd = synth.make_state_dict(0, family='trained' if boxes else 'uniform')
        if boxes:
            sd['rpn_head.init_proposal_bboxes.weight'] = np.array(BOXES[boxes], dtype=np.float32)
        _ENGINES[boxes] = HipEngine(sd, precision='f16x3')
    return _ENGINES[boxes]


def image(seed=41):
    return torch.from_numpy(synth.make_clips(seed, N // T, T, SIZE, SIZE)).to(DEV)


def forward(eng, img, lengths, levels):
    eng.set_option('fpn_levels_deferred', levels)
    out = eng.forward(img, lengths)
    torch.cuda.synchronize()
    eng.set_option('fpn_levels_deferred', 1)
    return {k: v.clone() for k, v in out.items()}


def frame_state(eng, mem, level):
    flags, counts, lists, on = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(-1)
    L.check(eng.lib.mcg_deferred_pyramid_frame_state(eng._handle, _ptr(mem), N, SIZE, SIZE, level, C.byref(flags), C.byref(counts), C.byref(lists),
                                                     C.byref(on)), 'frame state')
    return flags.value, counts.value, lists.value, on.value


def test_option_values():
    eng = engine()
    for bad in (3, 16, -1):
        with pytest.raises(L.McgError):
            eng.set_option('fpn_levels_deferred', bad)
    mem = _ws(eng.lib.mcg_deferred_pyramid_bytes(eng._handle, N, SIZE, SIZE), DEV)
    for value, want in ((0, [0, 0, 0]), (1, [0, 0, 1]), (ALL, [1, 1, 1]), (6, [1, 1, 0])):
        eng.set_option('fpn_levels_deferred', value)
        mem = _ws(eng.lib.mcg_deferred_pyramid_bytes(eng._handle, N, SIZE, SIZE), DEV)
        assert [frame_state(eng, mem, lv)[3] for lv in (1, 2, 3)] == want, value
    eng.set_option('fpn_levels_deferred', 1)


@pytest.mark.parametrize('lengths', [T, [2, 4]], ids=['uniform', 'ragged'])
@pytest.mark.parametrize('boxes', CASES, ids=str)
def test_forward_bitwise(boxes, lengths):
    eng = engine(boxes)
    img = image()
    off, default, every = (forward(eng, img, lengths, v) for v in (0, 1, ALL))
    assert same(default, off) and same(every, off)


@pytest.mark.parametrize('boxes', CASES[1:], ids=str)
def test_only_listed_frames_are_written(boxes):
    """Trunk and decoder through one slot whose P3 .. P5 are NaN in between: the frames the decoder wrote are the listed ones, every frame is
    listed at most once over the stages, the lists are the flagged frames, and the outputs are those of the dense path."""
    eng = engine(boxes)
    img = image()
    ref = forward(eng, img, T, 0)
    lib, h = eng.lib, eng._handle
    eng.set_option('fpn_levels_deferred', ALL)
    try:
        mem = _ws(lib.mcg_deferred_pyramid_bytes(h, N, SIZE, SIZE), DEV)
        mem.zero_()
        lv = (C.c_void_p * 4)()
        L.check(lib.mcg_deferred_pyramid_levels(h, _ptr(mem), N, SIZE, SIZE, lv, None), 'levels')
        tws = _ws(lib.mcg_trunk_workspace_bytes(h, N, SIZE, SIZE, 0), DEV)
        dws = _ws(lib.mcg_decoder_workspace_bytes(h, N), DEV)
        stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        L.check(lib.mcg_backbone_fpn_forward_deferred(h, stream, _ptr(img), N, SIZE, SIZE, 0, _ptr(mem), mem.numel(), _ptr(tws), tws.numel()), 'trunk')
        torch.cuda.synchronize()
        base = mem.data_ptr()
        maps = {}
        for level in (1, 2, 3):
            side = (SIZE // 4) >> level
            nbytes = N * side * side * 256 * 4
            maps[level] = mem[lv[level] - base:lv[level] - base + nbytes].view(torch.float32).view(N, -1)
            maps[level].fill_(float('nan'))
        out = dict(gaze=torch.empty(4, N, 3, device=DEV), boxes=torch.empty(N, 3, 4, device=DEV), scores=torch.empty(N, 3, device=DEV))
        L.check(lib.mcg_decoder_forward_deferred(h, stream, _ptr(mem), mem.numel(), N, T, SIZE, SIZE, None, _ptr(out['gaze']), _ptr(out['boxes']),
                                                 _ptr(out['scores']), _ptr(dws), dws.numel()), 'decoder')
        torch.cuda.synchronize()
        assert same(out, ref)
        read_any = False
        for level in (1, 2, 3):
            fl, cn, ls, on = frame_state(eng, mem, level)
            assert on == 1
            flags = mem[fl - base:fl - base + 4 * N].view(torch.int32).cpu().numpy()
            counts = mem[cn - base:cn - base + 4 * 4].view(torch.int32).cpu().numpy()
            lists = mem[ls - base:ls - base + 4 * 4 * N].view(torch.int32).view(4, N).cpu().numpy()
            ids = np.concatenate([lists[st, :counts[st]] for st in range(4)])
            assert counts.min() >= 0 and len(np.unique(ids)) == len(ids), 'a frame is on two lists'
            assert np.array_equal(np.sort(ids), np.flatnonzero(flags)), 'the lists are not the flagged frames'
            written = torch.isfinite(maps[level]).all(dim=1).cpu().numpy()
            untouched = torch.isnan(maps[level]).all(dim=1).cpu().numpy()
            assert np.array_equal(written, flags != 0) and np.array_equal(untouched, flags == 0), level
            read_any = read_any or bool(flags.any())
        assert read_any, 'no box of the case reads P3 .. P5'
    finally:
        eng.set_option('fpn_levels_deferred', 1)


def test_decode_with_a_permuted_frame_table():
    """decode over a dense pyramid store with a permuted frame_of: the option changes nothing on that path."""
    eng = engine('mixed')
    img = image()
    table = [4, 2, 5, 0, 3, 1]
    outs = []
    for value in (0, ALL):
        eng.set_option('fpn_levels_deferred', value)
        pyr = eng.backbone_fpn(img)
        o = eng.decode(pyr, table, T)
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in o.items()})
    eng.set_option('fpn_levels_deferred', 1)
    assert same(outs[0], outs[1])


@pytest.mark.parametrize('levels', [1, ALL])
def test_graphed_forward_bitwise(levels):
    """The whole forward captured into a graph with the levels deferred (no host read-back: the capture would fail) replays the eager bits."""
    eng = engine('huge')
    img = image(43)
    ref = forward(eng, img, T, 0)
    eng.set_option('fpn_levels_deferred', levels)
    try:
        g = GraphedForward(eng, N, SIZE, SIZE, T)
        out = g(img)
        torch.cuda.synchronize()
        assert same(out, ref)
        out = g(image(44))
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out.items()}
    finally:
        eng.set_option('fpn_levels_deferred', 1)
    assert same(got, forward(eng, image(44), T, 0))
