"""LiveGaze(draw=True, anonymize=...) on the device: the frames handed out equal the host composition over the tables the run itself returns
-- arrows.anonymize_heads_host into the raw frame, then the existing host drawer --, and every other table is bit-equal to a run without it.
The scene, the frames and the engine are those of tests/test_gpu_live_heat.py, the smallest live shape tests/live_gpu_common.py offers."""
import numpy as np
import pytest
import torch

from mcgaze_amd import arrows as AR
from mcgaze_amd import live
from tests import heat_cases as HC
from tests import live_cases as LC
from tests.live_gpu_common import ALPHA, CAMS, DEV, H, W, dev, make_engine, make_pipe, same
from tests.test_gpu_live_attention_poly import TICKS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


def run(engine, pipe, **kw):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, draw=True, **kw, **LC.OPTIONS)
    bufs = [torch.empty(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(LC.Q)]
    host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v
    results = []
    for t in range(TICKS + 1):
        if t < TICKS:
            for q in range(LC.Q):
                bufs[q].copy_(dev(CAMS[q][t]))
            r = lg.tick(bufs, dev(boxes[t]), dev(counts[t]))
        else:
            r = lg.finish()
        results.append({k: [[host(f) for f in fr] for fr in v] if k == 'frames' else host(v) for k, v in r.items()})
    return results


@pytest.mark.parametrize('options', [True, dict(shape='box', cell=8, expand=0.5), dict(mode='fill', color=(7, 8, 9))], ids=['defaults', 'box-cell8', 'fill'])
def test_the_frames_equal_the_host_composition_and_the_tables_do_not_change(engine, pipe, options):
    got, plain = run(engine, pipe, anonymize=options), run(engine, pipe)
    kw = {} if options is True else options
    frames_out = changed = 0
    for r, p in zip(got, plain):
        assert set(r) == set(p) and r['first'] == p['first']
        for name in p:
            if name not in ('first', 'frames'):
                same(r[name], p[name], name)                      # every table is bit-equal to the run without it
        k = r['valid'].shape[0]
        assert len(r['frames']) == k
        for i in range(k):
            t = r['first'] + i
            image_of = r['image_of'][i].reshape(-1)
            rows = image_of >= 0                                  # a row that is not valid has image_of -1: it hides nothing, and draws nothing
            local = image_of[rows] - i * LC.Q
            under, flags = AR.anonymize_heads_host([CAMS[q][t] for q in range(LC.Q)], r['head_box'][i].reshape(-1, 4)[rows], local, **kw)
            want, _ = AR.draw_arrows_host(under, r['head_box'][i].reshape(-1, 4)[rows], r['fused_smooth'][i].reshape(-1, 3)[rows], local)
            assert not flags.any()
            HC.same('bgr', r['frames'][i], want, t)
            changed += sum(not np.array_equal(a, b) for a, b in zip(r['frames'][i], p['frames'][i]))
            frames_out += 1
    assert frames_out == TICKS and changed > 0


def test_anonymize_needs_draw_and_known_options(engine, pipe):
    kw = dict(cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, **LC.OPTIONS)
    for bad in (dict(anonymize=True), dict(anonymize=dict(cell=12), draw=True), dict(anonymize=dict(colour=1), draw=True), dict(anonymize=dict(mode='blur'), draw=True)):
        with pytest.raises(ValueError):
            live.LiveGaze(engine, pipe, **kw, **bad)
