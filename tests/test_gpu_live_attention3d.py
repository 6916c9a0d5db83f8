"""LiveGaze(attention=dict(camera=, regions3d=, ...), dwell=True, heat=...) and run_head_video(attention=dict(camera=, regions3d=)) on
the device: the target tables, target_hit3d among them, are attention.gaze_targets_3d_host over the tables the call returns; region_frames
counts the rows the twin gives each 3-D region; the heat grids are gaze_heat_host over the projected hits (a hit behind the lens is NaN and
counts nowhere); and a run without ``camera`` returns today's tables, bit for bit.  The scene, the frames and the engine are those of
tests/test_gpu_live_attention.py."""
import numpy as np
import pytest
import torch

from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from tests import live_cases as LC
from tests.attention3d_cases import quad
from tests.live_gpu_common import ALPHA, CAMS, DEV, H, W, dev, make_engine, make_pipe, same

pytestmark = pytest.mark.gpu

TICKS = 16
CAMERA = [128.0, 128.0, W / 2, H / 2]                             # a 96 x 128 picture seen through a 53 degree lens; a 30-pixel head is 1 m away
# camera 0: a wall in front of everybody and one behind the lens (its hits have Pz < 0: a NaN ``target_hit``); camera 1: the left half of a wall
REGIONS3D = [[quad(-6, 6, -5, 5, 3.0), quad(-6, 6, -5, 5, -2.0)], [quad(-6, 0, -5, 5, 3.0)]]
OPTIONS = dict(expand=0.5, camera_angle=20.0, head_size=0.24, frame='eye')
TARGETS = ('target_kind', 'target', 'target_id', 'target_t', 'target_hit', 'mutual')


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


def run(engine, pipe, lanes, attention, dwell=None, heat=None):
    """-> (the results of every call as dicts of host arrays, region_frames and the heat grids on the host or None)."""
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, lanes=lanes, attention=attention, dwell=dwell,
                       heat=heat, **LC.OPTIONS)
    bufs = [torch.empty(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(LC.Q)]
    results = []
    for t in range(TICKS):
        for q in range(LC.Q):
            bufs[q].copy_(dev(CAMS[q][t]))
        results.append(lg.tick(bufs, dev(boxes[t]), dev(counts[t])))
    results.append(lg.finish())
    torch.cuda.synchronize()
    totals = None if dwell is None else lg.region_frames.cpu().numpy()
    grids = None if heat is None else lg.heat_state.heat.cpu().numpy()
    return [{k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in r.items()} for r in results], totals, grids


@pytest.mark.parametrize('lanes', [None, 3], ids=['slots', 'lanes'])
def test_live_targets_in_3d_equal_the_twin_with_dwell_and_heat_on_top(engine, pipe, lanes):
    got, totals, grids = run(engine, pipe, lanes, dict(OPTIONS, camera=CAMERA, regions3d=REGIONS3D), dwell=True, heat=dict(draw=False))
    lead = (LC.Q, LC.S) if lanes is None else (lanes,)
    three_d = AT._attention_options('LiveGaze', dict(camera=CAMERA, regions3d=REGIONS3D), LC.Q)[2]['three_d']
    assert three_d['cam'].shape == (LC.Q, 4) and three_d['regions'].start.tolist() == [0, 4, 8, 12] and three_d['region_image'].tolist() == [0, 0, 1]
    frames, kinds, nans = np.zeros(3, np.int32), np.zeros(4, int), 0
    heat = np.zeros_like(grids)
    for r in got:
        k = r['valid'].shape[0]
        want = AT.gaze_targets_3d_host(r['head_box'].reshape(-1, 4), r['fused_smooth'].reshape(-1, 3), r['image_of'].reshape(-1), three_d['cam'],
                                       regions=three_d['regions'], region_image=three_d['region_image'], region_period=LC.Q, cam_period=LC.Q, **OPTIONS)
        kind, target, t, hit, mutual, flags, hit3d = want
        head = kind == AT.KIND_HEAD
        ids = np.where(head, r['track_id'].reshape(-1)[np.maximum(target, 0)], 0).astype(np.int32)
        within = np.where(head, target % lead[-1], target).astype(np.int32)
        for name, w, tail in (('target_kind', kind, ()), ('target', within, ()), ('target_id', ids, ()), ('target_t', t, ()), ('target_hit', hit, (2,)),
                              ('mutual', mutual, ()), ('target_hit3d', hit3d, (3,))):
            same(r[name], w.reshape((k,) + lead + tail), name)
        person = np.where(r['valid'] != 0, r['track_id'], 0).reshape(-1)
        frames += np.bincount(target[(kind == AT.KIND_REGION) & (person > 0)], minlength=3).astype(np.int32)
        kinds += np.bincount(kind, minlength=4)
        nans += int(np.isnan(hit).any(axis=1).sum())
        for i in range(k):                                        # the heat map on top, unchanged: one accumulation per returned frame
            heat, _ = AT.gaze_heat_host(r['target_hit'][i].reshape(-1, 2), r['target_kind'][i].reshape(-1), r['image_of'][i].reshape(-1), heat,
                                        mask=r['valid'][i].reshape(-1), cell_shift=3, radius=2, period=LC.Q)
    same(totals, frames, 'region_frames')                         # exactly the rows the twin assigns to each 3-D region
    same(grids, heat, 'heat')
    assert kinds[2] > 0 and frames.sum() > 0 and heat.sum() > 0, (frames.tolist(), kinds.tolist())
    assert nans == 0 or frames[1] > 0                             # a NaN hit is a look at the wall behind the lens


def test_without_a_camera_every_table_is_todays(engine, pipe):
    """The same run with and without the new keys' defaults spelt out nowhere: no ``camera``, no 3-D -- and no target_hit3d."""
    rectangles = [np.array([[0, 0, W, H], [W - 30, 0, W, H]], np.float32), np.array([[0, 0, W // 2, H]], np.float32)]
    flat = dict(expand=0.5, camera_angle=20.0, regions=rectangles)
    got, totals, _ = run(engine, pipe, None, flat, dwell=True)
    regions, region_image, _ = AT._attention_options('LiveGaze', flat, LC.Q)
    for r in got:
        assert 'target_hit3d' not in r
        k = r['valid'].shape[0]
        want = AT.gaze_targets_host(r['head_box'].reshape(-1, 4), r['fused_smooth'].reshape(-1, 3), r['image_of'].reshape(-1), regions=regions,
                                    region_image=region_image, region_period=LC.Q, expand=0.5, camera_angle=20.0)
        for name, w, tail in (('target_kind', want[0], ()), ('target_t', want[2], ()), ('target_hit', want[3], (2,)), ('mutual', want[4], ())):
            same(r[name], w.reshape((k, LC.Q, LC.S) + tail), name)
    assert totals.sum() > 0


def test_run_head_video_records_carry_the_3d_hit(engine, pipe):
    frames = [CAMS[0][t] for t in range(12)]
    per_frame = [[[10 + t, 20, 40 + t, 56], [80, 24, 112, 60]] for t in range(8)] + [[[30, 20, 62, 58]] for _ in range(4)]
    regions3d = REGIONS3D[0]
    got = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=ALPHA, attention=dict(camera=CAMERA, regions3d=regions3d, expand=0.5))
    seen = np.zeros(4, int)
    for t in range(12):
        here = [(r, r['frame_id'].index(t)) for r in got if t in r['frame_id']]
        kind, target, _, hit, mutual, _, hit3d = AT.gaze_targets_3d_host(np.stack([r['head_box'][j] for r, j in here]),
                                                                         np.stack([r['fused_smooth'][j] for r, j in here]), None, CAMERA,
                                                                         regions=regions3d, expand=0.5)
        for i, (r, j) in enumerate(here):
            assert r['target_kind'][j] == kind[i] and r['mutual'][j] == mutual[i]
            same(r['target_hit'][j], hit[i], 'target_hit')
            same(r['target_hit3d'][j], hit3d[i], 'target_hit3d')
            assert r['target_id'][j] == (here[target[i]][0]['id'] if kind[i] == 1 else None)
            assert r['target_region'][j] == (target[i] if kind[i] == 2 else -1)
        seen += np.bincount(kind, minlength=4)
    assert seen[2] > 0, seen.tolist()
    plain = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=ALPHA, attention=dict(expand=0.5))
    assert all('target_hit3d' not in r for r in plain)
