"""-m gpu: live multi-person gaze with no host step -- mcg_live_slots, mcg_live_gate and live.LiveGaze over the scripted scene of
tests/live_cases.py (2 cameras x 4 slots, 28 ticks) on 96 x 128 frames, synthetic weights and 64 x 64 crops.

Every comparison is bit for bit: the kernels against their host twins (themselves held to hand-written facts in tests/test_live_cpu.py), a
slot's rows against a lone GazeStream fed that slot's crops, a person's valid rows against the same person in another scene, the drawn frames
against arrows.draw_arrows_host.  No tolerance anywhere.  Free slots are rows the head-crop entry documents (flag 2); nothing here provokes a
fault."""
import numpy as np
import pytest
import torch

from mcgaze_amd import live
from mcgaze_amd.arrows import draw_arrows_host
from mcgaze_amd.stream import GazeStream, GazeStreamPool
from tests import live_cases as LC
from tests.live_gpu_common import ALPHA, CAMS, DEV, GAZE, call, dev, make_engine, make_frames, make_pipe, run_live, same

pytestmark = pytest.mark.gpu

CAM0, CAM1 = CAMS
CAMS_OTHER = (CAM0, make_frames(3))


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


@pytest.fixture(scope='module')
def main_run(engine, pipe):
    return run_live(engine, pipe, 'main')


@pytest.fixture(scope='module')
def twin():
    return LC.run_host(*LC.scene(), smooth=True)


def slot_crops(pipe, twin, where):
    """The 28 crops of one slot, cut by head_crops from the TWIN's crop table (device tables: a free slot's row is flag 2, not an error)."""
    q, s = where
    boxes, _ = LC.scene()
    imgs, hws = [], []
    cam = (CAM0, CAM1)
    for t in range(LC.TICKS):
        rec = twin['ticks'][t]
        img, img_hw, _, _, _ = pipe.head_crops([dev(cam[c][t]) for c in range(LC.Q)], dev(rec['crop_boxes']), dev(rec['image_of']), device=DEV)
        imgs.append(img[q * LC.S + s]), hws.append(img_hw[q * LC.S + s])
    return torch.stack(imgs), torch.stack(hws)


# ---------------------------------------------------------------- 1. the kernels against their twins
def test_kernels_equal_the_host_twins(main_run, twin):
    for t in range(LC.TICKS):
        got, want = main_run['ticks'][t], twin['ticks'][t]
        same(got['crop_boxes'], want['crop_boxes'], f'crop_boxes, tick {t}')
        for name in ('image_of', 'ring_id', 'ring_box', 'matched', 'flags'):
            same(got[name].reshape(want[name].shape), want[name], f'{name}, tick {t}')
    assert main_run['calls'] == [(first, k) for _, first, k in twin['emitted']]
    for name in ('track_id', 'valid', 'smooth_valid', 'head_box', 'image_of'):
        same(main_run[name], twin[name], name)
    assert main_run['valid'][:, 0, 0].all() and main_run['valid'].sum() == twin['valid'].sum() > 50
    # the fall-back: a valid row next to an invalid neighbour carries its raw gaze in the smoothed tables
    raw = (main_run['valid'] == 1) & (main_run['smooth_valid'] == 0)
    assert raw.sum() == 4
    same(main_run['fused_smooth'][raw], main_run['fused'][raw], 'fused_smooth where only valid')
    same(main_run['others_smooth'][raw], main_run['others'][raw], 'others_smooth where only valid')


def test_a_slot_ring_is_a_lane_ring_whose_column_is_its_own_index(twin):
    """mcg_live_gate and mcg_live_gate_lanes, called directly, over the twin's ring as it stood at its last tick() that returned a frame
    and at finish(): the slot ring handed to the lanes entry as P = Q * S lanes, lane p naming column p.  Every output both entries have
    is the same bit for bit (and the twin's); camera / slot are p // S and p % S on the valid rows and -1 elsewhere."""
    cols = LC.Q * LC.S
    calls = [c for c in twin['emitted'] if c[2]]
    assert calls[-2:] == [(27, 19, 1), (27, 20, 8)]
    new = lambda *shape, dtype=torch.int32: torch.full(shape, 77, dtype=dtype, device=DEV)
    for (tick, first, k), (table, first_out) in zip(calls[-2:], twin['tables'][-2:]):
        ring_id, ring_box = LC.ring_at(twin, tick)
        lane_id, lane_box, lane_col = LC.as_lane_ring(ring_id, ring_box)
        fused, others, fused_s, others_s = LC.fake_gaze(k, first)
        got = {}
        for name, ring, lead in (('mcg_live_gate', (dev(ring_id), dev(ring_box), live.ring_depth(LC.CLIP), LC.Q, LC.S), (k, LC.Q, LC.S)),
                                 ('mcg_live_gate_lanes', (dev(lane_id), dev(lane_box), dev(lane_col), live.ring_depth(LC.CLIP), LC.Q, LC.S, cols),
                                  (k, cols))):
            o = dict(fused_smooth=dev(fused_s), others_smooth=dev(others_s), head_box=new(*lead, 4, dtype=torch.float32))
            o.update({n: new(*lead) for n in ('track_id', 'valid', 'camera', 'slot', 'image_of', 'smooth_valid')})
            extra = (o['camera'], o['slot']) if name == 'mcg_live_gate_lanes' else ()
            call(name, *ring, tick, dev(table), len(table), first_out, k, dev(fused), dev(others), o['fused_smooth'], o['others_smooth'], o['track_id'],
                 o['valid'], *extra, o['head_box'], o['image_of'], o['smooth_valid'])
            torch.cuda.synchronize()
            got[name] = {n: v.cpu().numpy() for n, v in o.items()}
        slots, lanes = got['mcg_live_gate'], got['mcg_live_gate_lanes']
        for name in ('track_id', 'valid', 'image_of', 'head_box', 'smooth_valid', 'fused_smooth', 'others_smooth'):
            same(slots[name], twin[name][first:first + k], name)
            same(lanes[name], slots[name].reshape(lanes[name].shape), name + ' over lanes')
        valid, p = lanes['valid'] == 1, np.arange(cols, dtype=np.int32)[None]
        assert valid.sum() >= 2 and not valid.all()
        same(lanes['camera'], np.where(valid, p // LC.S, -1).astype(np.int32), 'camera')
        same(lanes['slot'], np.where(valid, p % LC.S, -1).astype(np.int32), 'slot')


# ---------------------------------------------------------------- 2. the pool's contract, through LiveGaze
@pytest.mark.parametrize('where', [LC.SLOT_A, LC.SLOT_BC], ids=['A', 'B_then_C'])
def test_a_slot_is_a_lone_stream_of_its_crops(engine, pipe, main_run, twin, where):
    q, s = where
    imgs, hws = slot_crops(pipe, twin, where)
    assert bool((hws != 64).any()) or where != LC.SLOT_A                      # A's window is clipped by the frame border
    lone = GazeStream(engine, 64, 64, LC.CLIP, LC.STRIDE, merge='device', results='device', smooth=ALPHA)
    parts = [lone.push(imgs[t:t + 1], hws[t:t + 1]) for t in range(LC.TICKS)] + [lone.finish()]
    torch.cuda.synchronize()
    want = {name: torch.cat([p[name] for p in parts]).cpu().numpy() for name in GAZE + ('fused_smooth', 'others_smooth')}
    for name in GAZE:                                                         # all 28 frames, valid or not
        same(main_run[name][:, q, s], want[name], f'{name} of slot {where}')
    keep = ~((main_run['valid'][:, q, s] == 1) & (main_run['smooth_valid'][:, q, s] == 0))
    for name in ('fused_smooth', 'others_smooth'):                            # every row the gate did not replace is the pool's
        same(main_run[name][:, q, s][keep], want[name][keep], f'{name} of slot {where}')


# ---------------------------------------------------------------- 3. independence: the point of the gate
def test_a_persons_valid_rows_do_not_depend_on_the_others(engine, pipe, main_run):
    other = run_live(engine, pipe, 'other', CAMS_OTHER)
    q, s = LC.SLOT_BC
    assert other['track_id'][14:, q, s].tolist() == [2] * 14 and main_run['track_id'][14:, q, s].tolist() == [3] * 14     # C, under another id
    both = (main_run['valid'][:, q, s] == 1) & (other['valid'][:, q, s] == 1)
    assert both.tolist() == [False] * 19 + [True] * 9
    assert main_run['valid'][:8, q, s].all() and not other['valid'][:19, q, s].any()      # B's rows exist in one run only
    for name in GAZE + ('head_box',):
        same(main_run[name][:, q, s][both], other[name][:, q, s][both], name)
    smooth_both = (main_run['smooth_valid'][:, q, s] == 1) & (other['smooth_valid'][:, q, s] == 1)
    assert smooth_both.tolist() == [False] * 20 + [True] * 8
    same(main_run['fused_smooth'][:, q, s][smooth_both], other['fused_smooth'][:, q, s][smooth_both], 'fused_smooth')
    # and A, who is in both scenes from the first tick to the last
    for name in GAZE + ('head_box', 'fused_smooth', 'others_smooth'):
        same(main_run[name][:, 0, 0], other[name][:, 0, 0], name + ' of A')


# ---------------------------------------------------------------- 4. no host step
def test_a_tick_never_waits_for_the_device(engine, pipe, monkeypatch):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, **LC.OPTIONS)
    bufs = [dev(CAM0[0]), dev(CAM1[0])]
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
    assert r['first'] == 3 and tuple(r['valid'].shape) == (1, LC.Q, LC.S) and r['valid'][0, 0, 0].item() == 1


# ---------------------------------------------------------------- 5. img_hw pushed from the device
def test_a_device_img_hw_gives_the_pools_outputs(engine, pipe, twin):
    imgs, hws = slot_crops(pipe, twin, LC.SLOT_A)
    imgs, hws = imgs[:16], hws[:16]
    host_hw = hws.cpu().numpy()
    assert (host_hw != 64).any() and (host_hw.max(axis=1) == 64).all()        # clipped by the border: img_hw is not the padded size
    got = []
    for table in (hws, host_hw):
        pool = GazeStreamPool(engine, 64, 64, LC.CLIP, LC.STRIDE, rows=48, merge='device', results='device')
        a, b = pool.open(), pool.open()
        parts = {a: [], b: []}
        for t in range(16):
            pool.push(a, imgs[t:t + 1], table[t:t + 1])
            if t % 2:
                pool.push(b, imgs[t - 1:t + 1].flip(0), table[t - 1:t + 1][::-1].copy() if isinstance(table, np.ndarray) else table[t - 1:t + 1].flip(0))
            if t == 15:
                pool.close(a), pool.close(b)
            for sid, r in pool.step().items():
                parts[sid].append(r)
        torch.cuda.synchronize()
        got.append({sid: {name: torch.cat([r[name] for r in rs]).cpu().numpy() for name in GAZE} for sid, rs in parts.items()})
        assert pool.store.hw is not None
    for sid in got[0]:
        for name in GAZE:
            assert got[0][sid][name].shape[0] == 16
            same(got[0][sid][name], got[1][sid][name], f'{name} of stream {sid}')


# ---------------------------------------------------------------- 6. drawing
def test_drawn_frames_equal_the_host_drawing(engine, pipe):
    run = run_live(engine, pipe, 'main', smooth=None, draw=True)
    host = LC.run_host(*LC.scene())
    same(run['valid'], host['valid'], 'valid')
    same(run['image_of'], host['image_of'], 'image_of')
    assert [f for f, _ in run['frames']] == list(range(LC.TICKS))
    changed = 0
    at = 0
    for first, k in run['calls']:
        if not k:
            continue
        sl = slice(at, at + k)
        clean = [cam[f] for f in range(first, first + k) for cam in (CAM0, CAM1)]
        want, flags = draw_arrows_host(clean, host['head_box'][sl].reshape(-1, 4), run['fused'][sl].reshape(-1, 3), host['image_of'][sl].reshape(-1))
        assert (flags[host['valid'][sl].reshape(-1) == 0] == 2).all() and not flags[host['valid'][sl].reshape(-1) == 1].any()
        for i in range(k):
            for q in range(LC.Q):
                got = run['frames'][at + i][1][q]
                assert np.array_equal(got, want[i * LC.Q + q]), (first + i, q)
                n = int((got != clean[i * LC.Q + q]).any(axis=2).sum())
                changed += n
                if not host['valid'][at + i, q].any():
                    assert n == 0, (first + i, q)                             # invalid rows draw nothing
        at += k
    assert changed > 1000
