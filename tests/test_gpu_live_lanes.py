"""-m gpu: live multi-person gaze with lanes -- mcg_live_lanes, mcg_live_gate_lanes and live.LiveGaze(lanes=P) over the scenes of
tests/live_lanes_cases.py (2 cameras x 4 slots, 28 ticks) on 96 x 128 frames, synthetic weights and 64 x 64 crops, the set-up of
tests/test_gpu_live.py.

Every comparison is bit for bit: the kernels against their host twins (themselves held to hand-written facts in
tests/test_live_lanes_cpu.py), a person's rows through lanes against the same person's rows in the fixed schedule, a lane's rows against a
lone GazeStream fed that lane's crops, the drawn frames against arrows.draw_arrows_host.  No tolerance anywhere.  Free lanes are rows the
head-crop entry documents (flag 2); nothing here provokes a fault."""
import numpy as np
import pytest
import torch

from mcgaze_amd import live
from mcgaze_amd.arrows import draw_arrows_host
from mcgaze_amd.stream import GazeStream
from tests import live_cases as LC
from tests import live_lanes_cases as LL
from tests.live_gpu_common import ALPHA, CAMS, DEV, GAZE, dev, make_engine, make_pipe, run_live, same

pytestmark = pytest.mark.gpu

TICK_TABLES = ('lane_state', 'crop_boxes', 'image_of', 'lane_of', 'overflow', 'matched', 'ring_id', 'ring_box', 'ring_col', 'flags')


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


@pytest.fixture(scope='module')
def runs(engine, pipe):
    """The smoothed runs, each made once: runs(variant, lanes)."""
    made = {}

    def get(variant, lanes):
        if (variant, lanes) not in made:
            made[variant, lanes] = run_live(engine, pipe, variant, lanes=lanes)
        return made[variant, lanes]
    return get


@pytest.fixture(scope='module')
def twins():
    made = {}

    def get(variant, lanes, smooth=True):
        if (variant, lanes, smooth) not in made:
            made[variant, lanes, smooth] = LC.run_host(*LL.scene(variant), smooth=smooth, lanes=lanes)
        return made[variant, lanes, smooth]
    return get


# ---------------------------------------------------------------- 1. the kernels against their twins
@pytest.mark.parametrize('variant, lanes', [('main', 6), ('main', 4), ('queue', LL.QUEUE_LANES)], ids=['main-6', 'main-4', 'queue-2'])
def test_kernels_equal_the_host_twins(runs, twins, variant, lanes):
    run, twin = runs(variant, lanes), twins(variant, lanes)
    for t in range(LC.TICKS):
        got, want = run['ticks'][t], twin['ticks'][t]
        for name in TICK_TABLES:
            same(got[name], want[name], f'{name}, tick {t}')
    assert run['calls'] == [(first, k) for _, first, k in twin['emitted']]
    for name in ('track_id', 'valid', 'camera', 'slot', 'smooth_valid', 'head_box', 'image_of'):
        same(run[name], twin[name], name)
    assert run['valid'].shape == (LC.TICKS, lanes) and run['valid'].sum() > 40
    # the fall-back: a valid row next to an invalid neighbour carries its raw gaze in the smoothed tables
    raw = (run['valid'] == 1) & (run['smooth_valid'] == 0)
    assert raw.sum() == (2 if variant == 'queue' else 4)
    same(run['fused_smooth'][raw], run['fused'][raw], 'fused_smooth where only valid')
    same(run['others_smooth'][raw], run['others'][raw], 'others_smooth where only valid')


def test_more_lanes_and_columns_than_threads():
    """The kernel ranks 256 lanes or columns per step: 9 cameras x 64 slots = 576 columns and 300 lanes take three and two steps.  Six ticks
    of a random tracker state -- more people than lanes at first (overflow), then people leave and others come --, starting from a lane
    table with a column out of range, a negative one and two lanes naming one slot: inputs the entry documents (they free the lane)."""
    import ctypes as C

    from mcgaze_amd import lib as L
    from mcgaze_amd.head_detect import track_state_words
    Q, S, lanes, R = 9, 64, 300, 16
    rs = np.random.RandomState(5)
    lib = L.load()
    state = np.zeros((Q, track_state_words(S)), np.int32)
    table = state[:, 4:].reshape(Q, S, 8)
    table[..., :4] = rs.uniform(0, 500, (Q, S, 4)).astype(np.float32).view(np.int32)
    table[..., 4] = np.where(rs.rand(Q, S) < 0.6, np.arange(1, S + 1), 0)
    lane_state = np.zeros((lanes, 2), np.int32)
    first = int(table[0, :, 4].nonzero()[0][0])
    lane_state[[7, 260, 299, 3, 280]] = [[table[0, first, 4], first]] * 2 + [[5, Q * S], [5, -1], [9, 0x7fffffff]]
    ring_id, ring_box, ring_col = np.zeros((R, lanes), np.int32), np.zeros((R, lanes, 4), np.float32), np.zeros((R, lanes), np.int32)
    d_lane, d_id, d_box, d_col = dev(lane_state), dev(ring_id), dev(ring_box), dev(ring_col)
    new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=DEV)
    overflows = []
    for tick in range(6):
        if tick:
            leave = rs.rand(Q, S) < (0.5 if tick == 2 else 0.1)
            come = (table[..., 4] == 0) & (rs.rand(Q, S) < 0.3)
            table[..., 4] = np.where(leave, 0, np.where(come, 100 * tick + np.arange(S), table[..., 4]))
            table[..., 5] = rs.randint(0, 2, (Q, S))
        want = live.live_lanes_host(state, tick, lane_state, ring_id, ring_box, ring_col)
        got = [new(lanes, 4, dtype=torch.float32), new(lanes), new(Q, S), new(lanes), new(1)]
        p = lambda t: C.c_void_p(t.data_ptr())
        L.check(lib.mcg_live_lanes(C.c_void_p(torch.cuda.current_stream().cuda_stream), p(dev(state)), Q, S, lanes, tick, R, p(d_lane), p(got[0]), p(got[1]),
                                   p(d_id), p(d_box), p(d_col), p(got[2]), p(got[3]), p(got[4])), 'mcg_live_lanes')
        torch.cuda.synchronize()
        for name, g, w in zip(('crop_boxes', 'image_of', 'lane_of', 'matched', 'overflow'), got, want):
            same(g.cpu().numpy(), w, f'{name}, tick {tick}')
        for name, g, w in (('lane_state', d_lane, lane_state), ('ring_id', d_id, ring_id), ('ring_box', d_box, ring_box), ('ring_col', d_col, ring_col)):
            same(g.cpu().numpy(), w, f'{name}, tick {tick}')
        people = int((table[..., 4] > 0).sum())
        assert int(want[4][0]) == max(0, people - lanes) and int((lane_state[:, 0] != 0).sum()) == min(people, lanes), tick      # nobody waits beside a free lane
        overflows.append(int(want[4][0]))
    assert overflows[0] > 0 and overflows[2] == 0 and overflows[5] > 0       # 358, 375, 234, 304, 356, 378 people for 300 lanes
    assert (lane_state[:, 1] < Q * S).all() and (lane_state[:, 1] >= 0).all()


# ---------------------------------------------------------------- 2. lanes give what the fixed schedule gives
def test_lanes_equal_the_fixed_schedule(runs):
    """Rests on the pool's contract that a stream's bits do not depend on its neighbours, which holds for f16x3 (not for 'f16')."""
    lanes, fixed = runs('main', 6), runs('main', None)
    assert lanes['calls'] == fixed['calls']
    fv = np.argwhere(fixed['valid'] == 1)                                      # (frame, q, s)
    lv = np.argwhere(lanes['valid'] == 1)                                      # (frame, lane)
    assert len(fv) == len(lv) > 50
    where = {(int(f), int(lanes['camera'][f, p]), int(lanes['slot'][f, p])): int(p) for f, p in lv}
    assert len(where) == len(lv)                                               # one lane row per (frame, camera, slot)
    assert sorted(where) == sorted((int(f), int(q), int(s)) for f, q, s in fv)  # and the same set: each way round
    lane_rows = (fv[:, 0], np.array([where[int(f), int(q), int(s)] for f, q, s in fv]))
    slot_rows = (fv[:, 0], fv[:, 1], fv[:, 2])
    for name in ('track_id', 'smooth_valid', 'head_box') + GAZE:
        same(lanes[name][lane_rows], fixed[name][slot_rows], name)
    sv = fixed['smooth_valid'][slot_rows] == 1
    assert sv.sum() > 40
    for name in ('fused_smooth', 'others_smooth'):
        same(lanes[name][lane_rows][sv], fixed[name][slot_rows][sv], name)


# ---------------------------------------------------------------- 3. a lane is a lone stream of its crops
def test_a_lane_is_a_lone_stream_of_its_crops(engine, pipe, runs, twins):
    run, twin = runs('queue', LL.QUEUE_LANES), twins('queue', LL.QUEUE_LANES)
    assert run['track_id'][:, 0].tolist() == [1] * 12 + [2] * 16               # lane 0 carries A and then C
    imgs, hws = [], []
    for t in range(LC.TICKS):                                                  # device tables: a free lane's row would be flag 2, not an error
        rec = twin['ticks'][t]
        img, img_hw, _, _, _ = pipe.head_crops([dev(CAMS[q][t]) for q in range(LC.Q)], dev(rec['crop_boxes']), dev(rec['image_of']), device=DEV)
        imgs.append(img[0]), hws.append(img_hw[0])
    imgs, hws = torch.stack(imgs), torch.stack(hws)
    lone = GazeStream(engine, 64, 64, LC.CLIP, LC.STRIDE, merge='device', results='device', smooth=ALPHA)
    parts = [lone.push(imgs[t:t + 1], hws[t:t + 1]) for t in range(LC.TICKS)] + [lone.finish()]
    torch.cuda.synchronize()
    for name in GAZE:                                                          # all 28 frames, valid or not
        same(run[name][:, 0], torch.cat([p[name] for p in parts]).cpu().numpy(), f'{name} of lane 0')


# ---------------------------------------------------------------- 4. waiting for a lane changes only when rows begin
def test_waiting_for_a_lane_changes_only_when_rows_begin(runs):
    lanes, fixed = runs('queue', LL.QUEUE_LANES), runs('queue', None)
    q, s = 0, 1                                                                # C's slot; with lanes C is in lane 0 from tick 12
    assert fixed['valid'][:, q, s].tolist() == [0] * 7 + [1] * 21              # born at tick 4: valid from 4 + 3
    assert lanes['valid'][:, 0].tolist() == [1] * 8 + [0] * 7 + [1] * 13       # A up to 7; C from 12 + 3 (tests/test_live_lanes_cpu.py)
    both = (lanes['valid'][:, 0] == 1) & (fixed['valid'][:, q, s] == 1) & (lanes['track_id'][:, 0] == 2)
    assert both.tolist() == [False] * 15 + [True] * 13
    assert (lanes['camera'][:, 0][both] == q).all() and (lanes['slot'][:, 0][both] == s).all()
    for name in GAZE + ('head_box', 'track_id'):
        same(lanes[name][:, 0][both], fixed[name][:, q, s][both], name)


# ---------------------------------------------------------------- 5. no host step
def test_a_tick_never_waits_for_the_device(engine, pipe, monkeypatch):
    boxes, counts = LL.scene('main')
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, lanes=6, **LC.OPTIONS)
    bufs = [dev(CAMS[0][0]), dev(CAMS[1][0])]
    tables = [(dev(boxes[t]), dev(counts[t])) for t in range(12)]
    for t in range(11):                                                       # warm-up: the frame table is uploaded, windows have been decoded
        lg.tick(bufs, *tables[t])
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('the tick touched the host')

    for owner, name in ((torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'), (torch.cuda, 'synchronize'),
                        (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
        monkeypatch.setattr(owner, name, refuse)
    r = lg.tick(bufs, *tables[11])                                            # tick 11: a trunk call, a decoder call (window (4, 11)), a pop, the gate
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert r['first'] == 3 and tuple(r['valid'].shape) == (1, 6) and r['valid'][0, 0].item() == 1
    assert tuple(r['lane_of'].shape) == (LC.Q, LC.S) and tuple(r['overflow'].shape) == (1,) and tuple(r['matched'].shape) == (6,)


# ---------------------------------------------------------------- 6. drawing
def test_drawn_frames_equal_the_host_drawing(engine, pipe, twins):
    run = run_live(engine, pipe, 'main', lanes=6, smooth=None, draw=True)
    host = twins('main', 6, smooth=False)
    same(run['valid'], host['valid'], 'valid')
    same(run['image_of'], host['image_of'], 'image_of')
    assert [f for f, _ in run['frames']] == list(range(LC.TICKS))
    changed = 0
    at = 0
    for first, k in run['calls']:
        if not k:
            continue
        sl = slice(at, at + k)
        clean = [cam[f] for f in range(first, first + k) for cam in CAMS]
        want, flags = draw_arrows_host(clean, host['head_box'][sl].reshape(-1, 4), run['fused'][sl].reshape(-1, 3), host['image_of'][sl].reshape(-1))
        assert (flags[host['valid'][sl].reshape(-1) == 0] == 2).all() and not flags[host['valid'][sl].reshape(-1) == 1].any()
        for i in range(k):
            for q in range(LC.Q):
                got = run['frames'][at + i][1][q]
                assert np.array_equal(got, want[i * LC.Q + q]), (first + i, q)
                n = int((got != clean[i * LC.Q + q]).any(axis=2).sum())
                changed += n
                if not (host['camera'][at + i] == q).any():
                    assert n == 0, (first + i, q)                             # invalid rows draw nothing
        at += k
    assert changed > 1000
