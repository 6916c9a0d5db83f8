"""LiveGaze(attention=dict(camera=, regions3d=), surface_heat=..., draw=True) and run_head_video(..., surface_heat=, draw=) on the device:
the grids and the frames handed out equal the host route over the tables the run itself returns -- attention.surface_heat_host per returned
frame, arrows.draw_surface_heat_host into the raw frame, then the existing host drawer --, every other table is bit-equal to a run without
surface_heat, and the tick still never waits for the device.  The scene, the frames, the camera and the engine are those of
tests/test_gpu_live_attention3d.py (2 cameras of 96 x 128)."""
import numpy as np
import pytest
import torch

from mcgaze_amd import arrows as AR
from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from tests import heat_cases as HC
from tests import live_cases as LC
from tests.attention3d_cases import quad
from tests.live_gpu_common import ALPHA, CAMS, DEV, H, W, dev, make_engine, make_pipe, same
from tests.test_gpu_live_attention3d import CAMERA, OPTIONS

pytestmark = pytest.mark.gpu

TICKS = 16
# camera 0: a wall in front of everybody, a pane between the lens and the heads (they are about 0.9 m away: a look towards the lens side
# crosses it where the camera sees it, and it hides a part of the wall) and a wall behind the lens; camera 1: the left half of a wall, tilted
REGIONS3D = [[quad(-6, 6, -5, 5, 3.0), quad(-0.4, 0.4, -0.3, 0.3, 0.6), quad(-6, 6, -5, 5, -2.0)],
             [[[-6, -5, 2.5], [0, -5, 3.5], [0, 5, 3.5], [-6, 5, 2.5]]]]
ATTENTION = dict(OPTIONS, camera=CAMERA, regions3d=REGIONS3D)
SURFACE = dict(grid=(24, 16), radius=2, decay=3, draw=True, full_scale=None, min_level=2)
# what the grids hold before the first tick (the state is the caller's to set): whatever the looks do, there is something to draw
PREFILL = np.random.RandomState(12).randint(0, 60, (4, 16, 24)).astype(np.int32)


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


def run(engine, pipe, **kw):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, draw=True, attention=ATTENTION, **kw, **LC.OPTIONS)
    if 'surface_heat' in kw:
        lg.surface_heat_state.heat.copy_(dev(PREFILL))
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
        # surface_heat and surface_heat_peak are the LIVE tensors, which the next tick goes on updating: read here, after this tick
        results.append({k: [[host(f) for f in fr] for fr in v] if k == 'frames' else host(v) for k, v in r.items()})
    return results


def test_grids_and_frames_equal_the_host_route_and_the_other_tables_do_not_change(engine, pipe):
    got, plain = run(engine, pipe, surface_heat=SURFACE), run(engine, pipe)
    three_d = AT._attention_options('LiveGaze', dict(camera=CAMERA, regions3d=REGIONS3D), LC.Q)[2]['three_d']
    regions, region_image, cam = three_d['regions'], three_d['region_image'], three_d['cam']
    assert region_image.tolist() == [0, 0, 0, 1]
    heat, peak = PREFILL, np.zeros(4, np.int32)
    frames_out = changed = counted = 0
    for r, p in zip(got, plain):
        assert set(r) == set(p) | {'surface_heat', 'surface_heat_peak'} and r['first'] == p['first']
        for name in p:
            if name not in ('first', 'frames'):
                same(r[name], p[name], name)                      # every other table is bit-equal to the run without surface_heat
        k = r['valid'].shape[0]
        assert len(r['frames']) == k
        for i in range(k):
            t = r['first'] + i
            counted += int(((r['target_kind'][i] == 2) & (r['valid'][i] != 0)).sum())
            heat, peak = AT.surface_heat_host(r['target_hit3d'][i].reshape(-1, 3), r['target_kind'][i].reshape(-1), r['target'][i].reshape(-1), regions, heat,
                                              mask=r['valid'][i].reshape(-1), radius=2, decay=3)
            under = AR.draw_surface_heat_host([CAMS[q][t] for q in range(LC.Q)], heat, peak, cam, regions, region_image, min_level=2)
            image_of = r['image_of'][i].reshape(-1)
            want, _ = AR.draw_arrows_host(under, r['head_box'][i].reshape(-1, 4), r['fused_smooth'][i].reshape(-1, 3),
                                          np.where(image_of >= 0, image_of - i * LC.Q, image_of))
            HC.same('bgr', r['frames'][i], want, t)
            changed += sum(not np.array_equal(a, b) for a, b in zip(r['frames'][i], p['frames'][i]))
            frames_out += 1
        assert np.array_equal(r['surface_heat'], heat) and np.array_equal(r['surface_heat_peak'], peak), r['first']
    assert frames_out == TICKS and changed > 0 and counted > 0 and peak.max() > 0


def test_a_tick_with_surface_heat_never_waits_for_the_device(engine, pipe, monkeypatch):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, draw=True, attention=ATTENTION, surface_heat=SURFACE,
                       **LC.OPTIONS)
    assert tuple(lg.surface_heat_state.heat.shape) == (4, 16, 24)
    bufs = [dev(CAMS[0][0]), dev(CAMS[1][0])]
    tables = [(dev(boxes[t]), dev(counts[t])) for t in range(12)]
    for t in range(11):
        lg.tick(bufs, *tables[t])
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('the tick touched the host')

    def only_if_complete(event):
        # a stage of the staging ring that is taken again asks for the event of the copy it made four uploads earlier: no wait iff that
        # copy is over (tests/test_gpu_live_labels.py)
        assert event.query(), 'the tick waited for the device'

    for owner, name in ((torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'), (torch.cuda, 'synchronize'),
                        (torch.cuda.Stream, 'synchronize')):
        monkeypatch.setattr(owner, name, refuse)
    monkeypatch.setattr(torch.cuda.Event, 'synchronize', only_if_complete)
    r = lg.tick(bufs, *tables[11])
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert r['first'] == 3 and len(r['frames']) == 1 and r['surface_heat'] is lg.surface_heat_state.heat and r['surface_heat_peak'] is lg.surface_heat_state.peak


def test_surface_heat_needs_the_3d_attention_and_drawn_it_needs_draw(engine, pipe):
    kw = dict(cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, **LC.OPTIONS)
    for bad in (dict(surface_heat=True), dict(surface_heat=True, attention=True), dict(surface_heat=True, attention=dict(camera=CAMERA)),
                dict(surface_heat=dict(draw=True), attention=ATTENTION), dict(surface_heat=dict(grid=(0, 1)), attention=ATTENTION, draw=True),
                dict(surface_heat=dict(colour=1), attention=ATTENTION, draw=True)):
        with pytest.raises(ValueError):
            live.LiveGaze(engine, pipe, **kw, **bad)
    lg = live.LiveGaze(engine, pipe, attention=ATTENTION, surface_heat=dict(draw=False), **kw)      # accumulated, not drawn: no draw needed
    assert lg.surface_heat['draw'] is False and tuple(lg.surface_heat_state.heat.shape) == (4, 32, 32)


def test_run_head_video_accumulates_and_draws_its_surface_heat_and_leaves_the_source_frames_alone(engine, pipe):
    """20 device frames -- more than one drawing batch of harness.DRAW_FRAMES -- through run_head_video(attention=dict(camera=, regions3d=),
    surface_heat=, draw=): the grids are surface_heat_host over the records frame by frame (one decay per frame), every annotated frame is
    draw_surface_heat_host with the FINAL grids into the raw frame and then draw_arrows_host over the records' rows, and the caller's device
    frames are byte-identical afterwards."""
    T = 20
    assert T > harness.DRAW_FRAMES
    raw = np.random.default_rng(9).integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    frames = [dev(f) for f in raw]
    per_frame = [[[10 + t, 20, 40 + t, 56], [80, 24, 112, 60]] for t in range(12)] + [[[30, 20, 62, 58]] for _ in range(T - 12)]
    attention = dict(camera=CAMERA, regions3d=REGIONS3D[0], expand=0.5)
    options = dict(grid=(12, 9), radius=1, decay=4, min_level=2)
    records, annotated, grid = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, attention=attention, surface_heat=options,
                                                      draw=dict(min_thickness=2))
    torch.cuda.synchronize()
    assert all(np.array_equal(f.cpu().numpy(), r) for f, r in zip(frames, raw))      # drawn into clones, in every batch
    plain = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, attention=attention)
    assert len(records) == len(plain) and all(np.array_equal(g['target_hit3d'], p['target_hit3d']) for g, p in zip(records, plain))
    regions = AT.regions_3d(REGIONS3D[0])
    heat, peak = np.zeros((3, 9, 12), np.int32), None
    for t in range(T):
        here = [(r, r['frame_id'].index(t)) for r in records if t in r['frame_id']]
        heat, peak = AT.surface_heat_host(np.asarray([r['target_hit3d'][j] for r, j in here], np.float32).reshape(-1, 3),
                                          [int(r['target_kind'][j]) for r, j in here], [int(r['target_region'][j]) for r, j in here], regions, heat,
                                          radius=1, decay=4)
    assert grid.dtype == np.int32 and np.array_equal(grid, heat) and heat.sum() > 0
    assert len(annotated) == T
    for t in range(T):
        here = [(r, r['frame_id'].index(t)) for r in records if t in r['frame_id']]
        under = AR.draw_surface_heat_host(raw[t], heat, peak, CAMERA, regions, min_level=2)
        want, flags = AR.draw_arrows_host(under, np.stack([r['head_box'][j] for r, j in here]), np.stack([r['fused'][j] for r, j in here]), None, min_thickness=2)
        assert flags.tolist() == [0] * len(here)
        assert np.array_equal(annotated[t].cpu().numpy(), want), t
    assert any(not np.array_equal(AR.draw_surface_heat_host(raw[t], heat, peak, CAMERA, regions, min_level=2), raw[t]) for t in (0, T - 1))
    # without draw the grids are the last item as well; with the image-plane heat map they come after its grid; drawn in place on request
    records2, grid2 = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, attention=attention, surface_heat=dict(options, draw=False))
    assert np.array_equal(grid2, heat) and len(records2) == len(records)
    _, plane, grid3 = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, attention=attention, heat=dict(draw=False),
                                             surface_heat=dict(options, draw=False))
    assert plane.shape[0] == 1 and np.array_equal(grid3, heat)
    _, inplace, _ = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, attention=attention, surface_heat=options,
                                           draw=dict(min_thickness=2, copy=False))
    torch.cuda.synchronize()
    assert all(a is f for a, f in zip(inplace, frames)) and all(torch.equal(a, b) for a, b in zip(inplace, annotated))
