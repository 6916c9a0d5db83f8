"""LiveGaze(draw=True, attention=..., overlay=...) and run_head_video(attention=..., draw=dict(overlay=True)) on the device: the frames handed
out are arrows.draw_attention_host over the tables the same call returns, every other table is bit-equal to a run with plain draw=True, and
overlay without draw or without attention is refused.  The scene, the frames and the engine are those of
tests/test_gpu_live_attention_poly.py."""
import numpy as np
import pytest
import torch

from mcgaze_amd import arrows as AR
from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from tests import live_cases as LC
from tests import overlay_cases as O
from tests.live_gpu_common import ALPHA, CAMS, DEV, H, W, dev, make_engine, make_pipe, same
from tests.test_gpu_live_attention_poly import MIXED, OPTIONS, TICKS, TRAPEZOID

pytestmark = pytest.mark.gpu

OVERLAY = dict(palette=O.PALETTE, line_thickness=3, region_thickness=1)


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


def run(engine, pipe, lanes, overlay):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, lanes=lanes, attention=dict(OPTIONS, regions=MIXED),
                       draw=True, overlay=overlay, **LC.OPTIONS)
    bufs = [torch.empty(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(LC.Q)]
    results = []
    for t in range(TICKS):
        for q in range(LC.Q):
            bufs[q].copy_(dev(CAMS[q][t]))
        results.append(lg.tick(bufs, dev(boxes[t]), dev(counts[t])))
    results.append(lg.finish())
    torch.cuda.synchronize()
    host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v
    return [{k: [[host(f) for f in fr] for fr in v] if k == 'frames' else host(v) for k, v in r.items()} for r in results]


@pytest.mark.parametrize('lanes', [None, 3], ids=['slots', 'lanes'])
def test_live_frames_are_the_twin_over_the_returned_tables_and_the_tables_do_not_change(engine, pipe, lanes):
    got, plain = run(engine, pipe, lanes, OVERLAY), run(engine, pipe, lanes, None)
    regions, region_image, _ = AT._attention_options('LiveGaze', dict(regions=MIXED), LC.Q)
    lines = changed = 0
    for r, p in zip(got, plain):
        assert set(r) == set(p) and r['first'] == p['first']
        for name in p:
            if name not in ('first', 'frames'):
                same(r[name], p[name], name)
        k = r['valid'].shape[0]
        assert len(r['frames']) == k
        if not k:
            continue
        frames = [CAMS[q][t] for t in range(r['first'], r['first'] + k) for q in range(LC.Q)]
        want = AR.draw_attention_host(frames, r['head_box'].reshape(-1, 4), r['fused_smooth'].reshape(-1, 3), r['image_of'].reshape(-1),
                                      r['target_kind'].reshape(-1), r['target'].reshape(-1), r['target_hit'].reshape(-1, 2), r['mutual'].reshape(-1),
                                      regions=regions, region_image=region_image, region_period=LC.Q, **OVERLAY)[0]
        O.same('bgr', [f for fr in r['frames'] for f in fr], want, r['first'])
        lines += int(np.isin(r['target_kind'], (1, 2)).sum())
        changed += sum(not np.array_equal(a, b) for fa, fb in zip(r['frames'], p['frames']) for a, b in zip(fa, fb))
    assert lines > 0 and changed > 0


def test_overlay_needs_draw_and_attention(engine, pipe):
    kw = dict(cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, **LC.OPTIONS)
    for bad in (dict(overlay=True), dict(overlay=True, draw=True), dict(overlay=True, attention=True), dict(overlay=dict(colour=1), draw=True, attention=True),
                dict(overlay=dict(line_thickness=256), draw=True, attention=True), dict(overlay=3, draw=True, attention=True)):
        with pytest.raises(ValueError):
            live.LiveGaze(engine, pipe, **kw, **bad)
    frames = [CAMS[0][t] for t in range(3)]
    with pytest.raises(ValueError):
        harness.run_head_video(engine, pipe, frames, [[[10, 20, 40, 56]]] * 3, max_len=4, draw=dict(overlay=True))


def test_run_head_video_draws_the_overlay_of_its_own_records(engine, pipe):
    frames = [CAMS[0][t] for t in range(9)]
    per_frame = [[[10 + t, 20, 40 + t, 56], [80, 24, 112, 60]] for t in range(6)] + [[[30, 20, 62, 58]] for _ in range(3)]
    regions = [[100, 0, W, 40], TRAPEZOID]
    attention = dict(regions=regions, expand=0.5)
    plain = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=ALPHA, attention=attention)
    records, annotated = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=ALPHA, attention=attention,
                                                draw=dict(overlay=dict(palette=O.PALETTE), min_thickness=2))
    torch.cuda.synchronize()
    assert len(annotated) == 9 and len(records) == len(plain)
    for g, r in zip(records, plain):                              # the records are those of the run without drawing
        assert sorted(g) == sorted(r)
        for k in r:
            assert np.array_equal(g[k], r[k]) if isinstance(r[k], np.ndarray) else g[k] == r[k], k
    for t in range(9):
        here = [(r, r['frame_id'].index(t)) for r in records if t in r['frame_id']]
        col = lambda name: np.stack([r[name][j] for r, j in here])
        want = AR.draw_attention_host(frames[t], col('head_box'), col('fused_smooth'), None, col('target_kind'), col('target_region'), col('target_hit'),
                                      col('mutual'), regions=regions, palette=O.PALETTE, min_thickness=2)[0]
        assert np.array_equal(annotated[t].cpu().numpy(), want) and not np.array_equal(want, frames[t]), t
