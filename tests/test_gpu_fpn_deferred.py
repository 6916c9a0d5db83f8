"""-m gpu: the deferred FPN P2 output conv (engine option fpn_deferred, mcg_backbone_fpn_forward_deferred / mcg_decoder_forward_deferred).
The decoder computes only the 8 x 8-pixel P2 blocks RoIAlign reads; every result here is asserted BIT FOR BIT against the dense path
(fpn_deferred = 0), and a slot whose P2 holds NaN before the decoder shows that RoIAlign never reads a pixel the decoder did not compute."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from mcgaze_amd import synth
from mcgaze_amd.engine import HipEngine, PipelinedRunner, _ptr, _ws

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(a[k]), bits(b[k])) for k in ('gaze', 'boxes', 'scores'))


def forward(eng, img, T, deferred, img_hw=None):
    eng.set_option('fpn_deferred', deferred)
    out = eng.forward(img, T, img_hw=img_hw)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


# init proposals (cx, cy, w, h, normalised): a small box in the middle (P2), a box hugging / leaving the top-left corner, a box larger
# than the image (P4 / P5), a degenerate and a NaN box
BOX_SETS = {
    'synthetic': None,
    'border': [[0.5, 0.5, 0.08, 0.06], [0.02, 0.03, 0.25, 0.2], [0.97, 0.5, 0.3, 0.9]],
    'levels': [[0.3, 0.6, 0.12, 0.1], [0.5, 0.5, 0.6, 0.7], [0.5, 0.5, 1.8, 1.6]],
    'degenerate': [[0.5, 0.5, 0.0, 0.1], [0.2, 0.8, 0.15, 0.15], [1.2, -0.1, 0.3, 0.3]],
    'nan': [[float('nan'), 0.5, 0.1, 0.1], [0.4, 0.4, 0.1, 0.1], [0.5, 0.5, 0.4, 0.4]],
}


def state_dict(family='uniform', boxes=None):
    sd = synth.make_state_dict(0, family=family)
    if boxes is not None:
        sd['rpn_head.init_proposal_bboxes.weight'] = np.array(boxes, dtype=np.float32)
    return sd


@pytest.fixture(scope='module')
def engine():
    return HipEngine(state_dict(), precision='f16x3')


def test_deferred_is_on_for_f16x3_only(engine):
    lib, h = engine.lib, engine._handle
    slot = _ws(lib.mcg_deferred_pyramid_bytes(h, 7, 224, 224), DEV)
    lv, flag = (C.c_void_p * 4)(), C.c_int(-1)
    engine.set_option('fpn_deferred', 1)
    L.check(lib.mcg_deferred_pyramid_levels(h, _ptr(slot), 7, 224, 224, lv, C.byref(flag)), 'levels')
    assert flag.value == 1
    engine.set_option('fpn_deferred', 0)
    L.check(lib.mcg_deferred_pyramid_levels(h, _ptr(slot), 7, 224, 224, lv, C.byref(flag)), 'levels')
    assert flag.value == 0
    engine.set_option('fpn_deferred', 1)
    fp32 = HipEngine(state_dict(), precision='fp32')
    L.check(lib.mcg_deferred_pyramid_levels(fp32._handle, _ptr(slot), 7, 224, 224, lv, C.byref(flag)), 'levels')
    assert flag.value == 0


@pytest.mark.parametrize('clips', [1, 64])
def test_deferred_equals_dense(engine, clips):
    img = torch.from_numpy(synth.make_clips(0, clips, 7)).to(DEV)
    assert same(forward(engine, img, 7, 1), forward(engine, img, 7, 0))


@pytest.mark.parametrize('family', ['uniform', 'trained'])
@pytest.mark.parametrize('box_set', sorted(BOX_SETS))
def test_deferred_equals_dense_boxes(family, box_set):
    eng = HipEngine(state_dict(family, BOX_SETS[box_set]), precision='f16x3')
    img = torch.from_numpy(synth.make_clips(3, 2, 7)).to(DEV)
    assert same(forward(eng, img, 7, 1), forward(eng, img, 7, 0)), (family, box_set)


def test_deferred_equals_dense_non_square(engine):
    img = torch.from_numpy(synth.make_clips(5, 2, 7, 256, 192)).to(DEV)
    rs = np.random.RandomState(5)
    hw = np.stack([rs.randint(128, 257, 14), rs.randint(96, 193, 14)], axis=1).astype(np.int32)
    assert same(forward(engine, img, 7, 1, hw), forward(engine, img, 7, 0, hw))


def test_pipelined_runner_equals_forward(engine):
    N, T = 14, 7
    imgs = [torch.from_numpy(synth.make_clips(s, 2, T)).to(DEV) for s in (11, 12, 13)]
    ref = [forward(engine, x, T, 0) for x in imgs]
    engine.set_option('fpn_deferred', 1)
    runner = PipelinedRunner(engine, N, 224, 224, T)
    outs = [dict(gaze=torch.empty(4, N, 3, device=DEV), boxes=torch.empty(N, 3, 4, device=DEV), scores=torch.empty(N, 3, device=DEV))
            for _ in imgs]
    for x, o in zip(imgs, outs):
        runner.submit(x, o)
    runner.flush()
    torch.cuda.synchronize()
    for o, r in zip(outs, ref):
        assert same(o, r)


def test_poisoned_slot(engine):
    """P2 of the slot is NaN before the deferred decoder: what RoIAlign reads is exactly what the decoder computed."""
    N, T, H, W = 14, 7, 224, 224
    img = torch.from_numpy(synth.make_clips(21, 2, T)).to(DEV)
    ref = forward(engine, img, T, 0)
    engine.set_option('fpn_deferred', 1)
    lib, h = engine.lib, engine._handle
    slot = _ws(lib.mcg_deferred_pyramid_bytes(h, N, H, W), DEV)
    tws = _ws(lib.mcg_trunk_workspace_bytes(h, N, H, W, 0), DEV)
    dws = _ws(lib.mcg_decoder_workspace_bytes(h, N), DEV)
    lv, flag = (C.c_void_p * 4)(), C.c_int(-1)
    L.check(lib.mcg_deferred_pyramid_levels(h, _ptr(slot), N, H, W, lv, C.byref(flag)), 'levels')
    assert flag.value == 1
    p2_off = lv[0] - slot.data_ptr()
    p2_bytes = lv[1] - lv[0]
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    L.check(lib.mcg_backbone_fpn_forward_deferred(h, stream, _ptr(img), N, H, W, 0, _ptr(slot), slot.numel(), _ptr(tws), tws.numel()), 'trunk')
    slot[p2_off:p2_off + p2_bytes].view(torch.float32).fill_(float('nan'))
    out = dict(gaze=torch.empty(4, N, 3, device=DEV), boxes=torch.empty(N, 3, 4, device=DEV), scores=torch.empty(N, 3, device=DEV))
    L.check(lib.mcg_decoder_forward_deferred(h, stream, _ptr(slot), slot.numel(), N, T, H, W, None, _ptr(out['gaze']), _ptr(out['boxes']),
                                             _ptr(out['scores']), _ptr(dws), dws.numel()), 'decoder')
    torch.cuda.synchronize()
    assert same(out, ref)
    p2 = slot[p2_off:p2_off + N * 56 * 56 * 256 * 4].view(torch.float32).view(N, 56, 56, 256)
    written = torch.isfinite(p2).all(dim=-1).float().mean().item()
    assert 0.0 < written < 1.0, written   # some blocks were computed, not all of them
