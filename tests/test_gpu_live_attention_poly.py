"""LiveGaze(attention=dict(regions=[mixed lists]), dwell=True) and run_head_video(attention=dict(regions=[mixed list])) on the device: the
target tables are attention.gaze_targets_host over the tables the call returns and the polygons, region_frames of a polygon counts the rows
the twin gives it, and a run whose usable regions are all rectangles returns what today's form returns.  The scene, the frames and the
engine are those of tests/test_gpu_live_attention.py."""
import numpy as np
import pytest
import torch

from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from tests import live_cases as LC
from tests.live_gpu_common import ALPHA, CAMS, DEV, H, W, dev, make_engine, make_pipe, same

pytestmark = pytest.mark.gpu

TICKS = 16
TRAPEZOID = [[0, 0], [W, 0], [W - 20, H], [20, H]]                # camera 0: most of the frame (most origins are inside: t = 0), seen off-axis
ELL = [[0, 0], [W // 2, 0], [W // 2, H // 2], [W // 4, H // 2], [W // 4, H], [0, H]]      # camera 1: the left half without its lower right quarter
MIXED = [[TRAPEZOID, [W - 30, 0, W, H]], [ELL]]
RECTANGLES = [np.array([[0, 0, W, H], [W - 30, 0, W, H]], np.float32), np.array([[0, 0, W // 2, H]], np.float32)]      # test_gpu_live_attention's
OPTIONS = dict(expand=0.5, camera_angle=20.0)
TARGETS = ('target_kind', 'target', 'target_id', 'target_t', 'target_hit', 'mutual')


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


def run(engine, pipe, lanes, regions, dwell=None):
    """-> (the results of every call as dicts of host arrays, region_frames on the host or None)."""
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, lanes=lanes, attention=dict(OPTIONS, regions=regions),
                       dwell=dwell, **LC.OPTIONS)
    bufs = [torch.empty(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(LC.Q)]
    results = []
    for t in range(TICKS):
        for q in range(LC.Q):
            bufs[q].copy_(dev(CAMS[q][t]))
        results.append(lg.tick(bufs, dev(boxes[t]), dev(counts[t])))
    results.append(lg.finish())
    torch.cuda.synchronize()
    totals = None if dwell is None else lg.region_frames.cpu().numpy()
    return [{k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in r.items()} for r in results], totals


@pytest.mark.parametrize('lanes', [None, 3], ids=['slots', 'lanes'])
def test_live_targets_equal_the_twin_and_a_polygon_collects_its_frames(engine, pipe, lanes):
    got, totals = run(engine, pipe, lanes, MIXED, dwell=True)
    lead = (LC.Q, LC.S) if lanes is None else (lanes,)
    regions, region_image, _ = AT._attention_options('LiveGaze', dict(regions=MIXED), LC.Q)
    assert isinstance(regions, AT.PolyRegions) and regions.start.tolist() == [0, 4, 6, 12] and region_image.tolist() == [0, 0, 1]
    frames, kinds = np.zeros(3, np.int32), np.zeros(4, int)
    for r in got:
        k = r['valid'].shape[0]
        want = AT.gaze_targets_host(r['head_box'].reshape(-1, 4), r['fused_smooth'].reshape(-1, 3), r['image_of'].reshape(-1), regions=regions,
                                    region_image=region_image, region_period=LC.Q, **OPTIONS)
        kind, target, t, hit, mutual, flags = want
        head = kind == AT.KIND_HEAD
        ids = np.where(head, r['track_id'].reshape(-1)[np.maximum(target, 0)], 0).astype(np.int32)
        within = np.where(head, target % lead[-1], target).astype(np.int32)
        for name, w, tail in (('target_kind', kind, ()), ('target', within, ()), ('target_id', ids, ()), ('target_t', t, ()), ('target_hit', hit, (2,)),
                              ('mutual', mutual, ())):
            same(r[name], w.reshape((k,) + lead + tail), name)
        person = np.where(r['valid'] != 0, r['track_id'], 0).reshape(-1)
        frames += np.bincount(target[(kind == AT.KIND_REGION) & (person > 0)], minlength=3).astype(np.int32)
        kinds += np.bincount(kind, minlength=4)
    same(totals, frames, 'region_frames')                         # exactly the rows the twin assigns to each region, polygons included
    assert frames[0] > 0 and frames[2] > 0 and kinds[2] > 0, (frames.tolist(), kinds.tolist())


def test_rectangles_through_the_polygon_entry_return_what_todays_form_returns(engine, pipe):
    """Camera 1 also gets a polygon with a vertex that is not finite: never hit, but it sends every region through mcg_gaze_targets_poly, the
    rectangles as 2 vertices.  Every returned table equals the run through mcg_gaze_targets, and so do the person-frames of the rectangles."""
    old, old_totals = run(engine, pipe, None, RECTANGLES, dwell=True)
    unusable = [[0, 0], [W, 0], [W, float('nan')]]
    regions = [RECTANGLES[0].tolist(), RECTANGLES[1].tolist() + [unusable]]
    assert isinstance(AT._attention_options('LiveGaze', dict(regions=regions), LC.Q)[0], AT.PolyRegions)
    new, new_totals = run(engine, pipe, None, regions, dwell=True)
    for r, p in zip(new, old):
        assert set(r) == set(p) and r['first'] == p['first']
        for name in p:
            if name != 'first':
                same(r[name], p[name], name)
    same(new_totals[:3], old_totals, 'region_frames')
    assert new_totals[3] == 0 and old_totals.sum() > 0


def test_run_head_video_records_carry_the_polygon(engine, pipe):
    frames = [CAMS[0][t] for t in range(9)]
    per_frame = [[[10 + t, 20, 40 + t, 56], [80, 24, 112, 60]] for t in range(6)] + [[[30, 20, 62, 58]] for _ in range(3)]
    regions = [[100, 0, W, 40], TRAPEZOID]
    got = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=ALPHA, attention=dict(regions=regions, expand=0.5))
    seen = np.zeros(4, int)
    polygon = 0
    for t in range(9):
        here = [(r, r['frame_id'].index(t)) for r in got if t in r['frame_id']]
        kind, target, _, hit, mutual, _ = AT.gaze_targets_host(np.stack([r['head_box'][j] for r, j in here]), np.stack([r['fused_smooth'][j] for r, j in here]),
                                                               regions=regions, expand=0.5)
        for i, (r, j) in enumerate(here):
            assert r['target_kind'][j] == kind[i] and r['mutual'][j] == mutual[i]
            same(r['target_hit'][j], hit[i], 'target_hit')
            assert r['target_id'][j] == (here[target[i]][0]['id'] if kind[i] == 1 else None)
            assert r['target_region'][j] == (target[i] if kind[i] == 2 else -1)
            polygon += int(r['target_region'][j] == 1)
        seen += np.bincount(kind, minlength=4)
    assert polygon > 0 and seen[2] > 0, (polygon, seen.tolist())
