"""LiveGaze(attention=...) and run_head_video(attention=...) on the device: the added tables are attention.gaze_targets_host of the tables the
call returns, everything else is what a run without attention returns, and a tick still never waits for the device.  The scene, the frames
and the engine are those of tests/test_gpu_live.py, cut to 16 ticks (A and B share camera 0 up to tick 9, D is in camera 1 from tick 6)."""
import numpy as np
import pytest
import torch

from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from tests import live_cases as LC
from tests.live_gpu_common import ALPHA, CAMS, DEV, H, W, dev, make_engine, make_pipe, same

pytestmark = pytest.mark.gpu

TICKS = 16
# camera 0: the whole frame (every ray starts inside it: t = 0 unless a head is met at 0 too) and a strip at the right; camera 1: the left half
REGIONS = [np.array([[0, 0, W, H], [W - 30, 0, W, H]], np.float32), np.array([[0, 0, W // 2, H]], np.float32)]
OPTIONS = dict(regions=REGIONS, expand=0.5, camera_angle=20.0)
ADDED = ('target_kind', 'target', 'target_id', 'target_t', 'target_hit', 'mutual')


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


def run(engine, pipe, lanes, attention, smooth=ALPHA):
    """-> the results of every call, as dicts of host arrays."""
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=smooth, lanes=lanes, attention=attention, **LC.OPTIONS)
    bufs = [torch.empty(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(LC.Q)]
    results = []
    for t in range(TICKS):
        for q in range(LC.Q):
            bufs[q].copy_(dev(CAMS[q][t]))
        results.append(lg.tick(bufs, dev(boxes[t]), dev(counts[t])))
    results.append(lg.finish())
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in r.items()} for r in results]


@pytest.mark.parametrize('lanes,smooth', [(None, ALPHA), (3, ALPHA), (None, None)], ids=['slots', 'lanes', 'slots-unsmoothed'])
def test_live_targets_equal_the_host_twin(engine, pipe, lanes, smooth):
    plain = run(engine, pipe, lanes, None, smooth)
    got = run(engine, pipe, lanes, OPTIONS, smooth)
    lead = (LC.Q, LC.S) if lanes is None else (lanes,)
    regions, region_image = np.concatenate(REGIONS), np.array([0, 0, 1], np.int32)
    kinds = np.zeros(4, int)
    for r, p in zip(got, plain):
        k = r['valid'].shape[0]
        assert set(r) == set(p) | set(ADDED) and r['first'] == p['first']
        for name in p:                                            # every table of a run without attention, bit for bit
            if name != 'first':
                same(r[name], p[name], name)
        gaze = r['fused' if smooth is None else 'fused_smooth']
        want = AT.gaze_targets_host(r['head_box'].reshape(-1, 4), gaze.reshape(-1, 3), r['image_of'].reshape(-1), regions=regions,
                                    region_image=region_image, region_period=LC.Q, expand=0.5, camera_angle=20.0)
        kind, target, t, hit, mutual, flags = want
        head = kind == AT.KIND_HEAD
        ids = np.where(head, r['track_id'].reshape(-1)[np.maximum(target, 0)], 0).astype(np.int32)     # gathered on the host
        within = np.where(head, target % lead[-1], target).astype(np.int32)
        for name, w, tail in (('target_kind', kind, ()), ('target', within, ()), ('target_id', ids, ()), ('target_t', t, ()), ('target_hit', hit, (2,)),
                              ('mutual', mutual, ())):
            same(r[name], w.reshape((k,) + lead + tail), name)
        assert ((flags == 2) == (r['image_of'].reshape(-1) < 0)).all()      # the gate's invalid rows, and only they
        assert (kind[flags == 2] == 0).all()
        kinds += np.bincount(kind, minlength=4)
        if head.any():                                            # a looked-at person is a valid row of the same picture
            assert (ids[head] > 0).all() and (r['image_of'].reshape(-1)[target[head]] == r['image_of'].reshape(-1)[head]).all()
    assert kinds[1:].sum() > 0, kinds.tolist()                    # somebody looks at something: camera 0's first region holds every origin


def test_a_tick_with_attention_never_waits_for_the_device(engine, pipe, monkeypatch):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, attention=OPTIONS, **LC.OPTIONS)
    bufs = [dev(CAMS[0][0]), dev(CAMS[1][0])]
    tables = [(dev(boxes[t]), dev(counts[t])) for t in range(12)]
    for t in range(11):
        lg.tick(bufs, *tables[t])
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('the tick touched the host')

    for owner, name in ((torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'), (torch.cuda, 'synchronize'),
                        (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
        monkeypatch.setattr(owner, name, refuse)
    r = lg.tick(bufs, *tables[11])                                # tick 11 returns frame 3: the gate, then gaze_targets over its rows
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert r['first'] == 3 and tuple(r['target_kind'].shape) == (1, LC.Q, LC.S) and tuple(r['target_hit'].shape) == (1, LC.Q, LC.S, 2)
    assert r['valid'][0, 0, 0].item() == 1 and r['target_kind'][0, 0, 0].item() != 0      # A is inside camera 0's whole-frame region


def test_run_head_video_attention(engine, pipe):
    """Two people for 6 frames and one for 3 more; the records of a run without attention, plus the targets of the host twin applied to each
    frame's boxes and the gaze ``arrow`` comes from."""
    frames = [CAMS[0][t] for t in range(9)]
    per_frame = [[[10 + t, 20, 40 + t, 56], [80, 24, 112, 60]] for t in range(6)] + [[[30, 20, 62, 58]] for _ in range(3)]
    regions = [[0, 0, W, H], [100, 0, W, 40]]
    for smooth in (None, ALPHA):
        plain = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=smooth)
        got = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=smooth, attention=dict(regions=regions, expand=0.5))
        assert [r['id'] for r in got] == [r['id'] for r in plain] == [(0, 0), (0, 1), (1, 0)]
        for r, p in zip(got, plain):
            assert set(r) == set(p) | {'target_kind', 'target_id', 'target_region', 'target_hit', 'mutual'}
            for name in p:
                assert np.array_equal(np.asarray(r[name]), np.asarray(p[name])), name
        key = 'fused' if smooth is None else 'fused_smooth'
        seen = np.zeros(4, int)
        for t in range(9):
            here = [(r, r['frame_id'].index(t)) for r in got if t in r['frame_id']]          # record order: the rows of the call
            kind, target, _, hit, mutual, _ = AT.gaze_targets_host(np.stack([r['head_box'][j] for r, j in here]), np.stack([r[key][j] for r, j in here]),
                                                                   regions=regions, expand=0.5)
            for i, (r, j) in enumerate(here):
                assert r['target_kind'][j] == kind[i] and r['mutual'][j] == mutual[i]
                same(r['target_hit'][j], hit[i], 'target_hit')
                assert r['target_id'][j] == (here[target[i]][0]['id'] if kind[i] == 1 else None)
                assert r['target_region'][j] == (target[i] if kind[i] == 2 else -1)
            seen += np.bincount(kind, minlength=4)
        assert seen[1:].sum() > 0, seen.tolist()
