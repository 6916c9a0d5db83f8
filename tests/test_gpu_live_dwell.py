"""LiveGaze(dwell=...) and run_head_video(dwell=...) on the device: the added tables and the episodes are attention.gaze_dwell_host run over the
gate and target tables the calls return, with the state carried from call to call; everything else is what a run without dwell returns;
and a tick still never waits for the device.  The scene, the frames and the engine are those of tests/test_gpu_live_attention.py."""
import numpy as np
import pytest
import torch

from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from tests import live_cases as LC
from tests.live_gpu_common import ALPHA, CAMS, DEV, H, W, dev, make_engine, make_pipe, same

pytestmark = pytest.mark.gpu

TICKS = 16
REGIONS = [np.array([[0, 0, W, H], [W - 30, 0, W, H]], np.float32), np.array([[0, 0, W // 2, H]], np.float32)]
OPTIONS = dict(regions=REGIONS, expand=0.5, camera_angle=20.0)
DWELL = dict(enter=2, exit=1)
ADDED = ('dwell_kind', 'dwell_id', 'dwell_start', 'dwell_frames', 'episodes', 'num_episodes')


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


def run(engine, pipe, lanes, dwell):
    """-> (the results of every call as dicts of host arrays, the object's dwell state and region totals on the host, or None)."""
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, lanes=lanes, attention=OPTIONS, dwell=dwell,
                       **LC.OPTIONS)
    bufs = [torch.empty(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(LC.Q)]
    results = []
    for t in range(TICKS):
        for q in range(LC.Q):
            bufs[q].copy_(dev(CAMS[q][t]))
        results.append(lg.tick(bufs, dev(boxes[t]), dev(counts[t])))
    results.append(lg.finish())
    torch.cuda.synchronize()
    left = None if dwell is None else (lg.dwell_state.cpu().numpy(), lg.region_frames.cpu().numpy())
    return [{k: v.cpu().numpy() if isinstance(v, torch.Tensor) else v for k, v in r.items()} for r in results], left


@pytest.mark.parametrize('lanes', [None, 3], ids=['slots', 'lanes'])
def test_live_dwell_equals_the_host_twin(engine, pipe, lanes):
    plain, _ = run(engine, pipe, lanes, None)
    got, (left_state, left_regions) = run(engine, pipe, lanes, DWELL)
    lead = (LC.Q, LC.S) if lanes is None else (lanes,)
    columns = int(np.prod(lead))
    state, totals = np.zeros((columns, 16), np.int32), np.zeros(3, np.int32)
    current = episodes = 0
    for r, p in zip(got, plain):
        k = r['valid'].shape[0]
        assert set(r) == set(p) | set(ADDED) and r['first'] == p['first']
        for name in p:                                            # every table of a run without dwell, bit for bit
            if name != 'first':
                same(r[name], p[name], name)
        person = np.where(r['valid'] != 0, r['track_id'], 0).reshape(k, columns)
        tag = None if lanes is None else (r['camera'] * LC.S + r['slot']).reshape(k, columns)
        ident = np.where(r['target_kind'] == AT.KIND_HEAD, r['target_id'], r['target']).reshape(k, columns)
        want = AT.gaze_dwell_host(person, r['target_kind'].reshape(k, columns), ident, r['mutual'].reshape(k, columns), tag=tag, state=state,
                                  frame0=r['first'], region_frames=totals, **DWELL)
        dwell, _, events, num, state, totals = want
        for j, name in enumerate(ADDED[:4]):
            same(r[name], dwell[..., j].reshape((k,) + lead), name)
        same(r['episodes'], events, 'episodes')
        same(r['num_episodes'], num, 'num_episodes')
        current += int((dwell[..., 0] != 0).sum())
        episodes += int(num[0])
    same(left_state, state, 'dwell_state')
    same(left_regions, totals, 'region_frames')
    # somebody dwells on something and an episode ends: camera 0's first region holds every origin, and A and B leave it at tick 9
    assert current > 0 and episodes > 0 and totals.sum() > 0, (current, episodes, totals.tolist())


def test_a_tick_with_dwell_never_waits_for_the_device(engine, pipe, monkeypatch):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, attention=OPTIONS, dwell=True, **LC.OPTIONS)
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
    r = lg.tick(bufs, *tables[11])                                # tick 11 returns frame 3: the gate, gaze_targets, then gaze_dwell over its rows
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert r['first'] == 3 and tuple(r['dwell_kind'].shape) == (1, LC.Q, LC.S) and tuple(r['episodes'].shape) == (LC.Q * LC.S, 10)
    assert tuple(r['num_episodes'].shape) == (1,) and tuple(lg.dwell_state.shape) == (LC.Q * LC.S, 16) and tuple(lg.region_frames.shape) == (3,)
    assert lg.dwell_state[0, 0].item() == r['track_id'][0, 0, 0].item() > 0      # A owns column 0


def test_run_head_video_dwell(engine, pipe):
    """Two people for 6 frames and one for 3 more: the records of a run without dwell, plus the twin's dwell over the records' own target
    tables -- a column per record --, its ended episodes and, with reason 4, those its state leaves open."""
    frames = [CAMS[0][t] for t in range(9)]
    per_frame = [[[10 + t, 20, 40 + t, 56], [80, 24, 112, 60]] for t in range(6)] + [[[30, 20, 62, 58]] for _ in range(3)]
    attention = dict(regions=[[0, 0, W, H], [100, 0, W, 40]], expand=0.5)
    plain = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, attention=attention)
    got = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, attention=attention, dwell=dict(enter=1, exit=1))
    assert [r['id'] for r in got] == [(0, 0), (0, 1), (1, 0)]
    for r, p in zip(got, plain):
        assert set(r) == set(p) | {'dwell_kind', 'dwell_frames', 'episodes'}
        for name in p:
            assert r[name] == p[name] if name == 'target_id' else np.array_equal(np.asarray(r[name]), np.asarray(p[name])), name
    R, index = len(got), {r['id']: n for n, r in enumerate(got)}
    person, kind, ident, mutual = (np.zeros((9, R), np.int32) for _ in range(4))
    for n, r in enumerate(got):
        for j, t in enumerate(r['frame_id']):
            person[t, n], kind[t, n], mutual[t, n] = n + 1, r['target_kind'][j], r['mutual'][j]
            ident[t, n] = index[r['target_id'][j]] + 1 if kind[t, n] == 1 else r['target_region'][j]
    dwell, ended, events, num, state, _ = AT.gaze_dwell_host(person, kind, ident, mutual, enter=1, exit=1)
    reasons = []
    for n, r in enumerate(got):
        t = np.asarray(r['frame_id'])
        same(np.asarray(r['dwell_kind']), dwell[t, n, 0], 'dwell_kind')
        same(np.asarray(r['dwell_frames']), dwell[t, n, 3], 'dwell_frames')
        want = [row[4:] for row in events[:int(num[0])].tolist() if row[1] == n]
        if state[n, 2]:
            want.append(state[n, 2:7].tolist() + [AT.END_VIDEO_ENDED])
        assert len(r['episodes']) == len(want)
        for e, (k, i, start, length, mutual_frames, reason) in zip(r['episodes'], want):
            target = dict(target_id=got[i - 1]['id']) if k == 1 else dict(target_region=i) if k == 2 else {}
            assert e == dict(kind=k, **target, start=start, frames=length, mutual_frames=mutual_frames, reason=reason)
            reasons.append(reason)
    # the first two records end at frame 5 with their owners (reason 2); the third is still looking when the video ends (reason 4)
    assert AT.END_OWNER_LEFT in reasons or AT.END_LOOKED_AWAY in reasons, reasons
    assert AT.END_VIDEO_ENDED in reasons, reasons
