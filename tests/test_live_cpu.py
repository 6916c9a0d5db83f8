"""The live chain on the host (mcgaze_amd/live.py): live_slots_host, live_gate_table and live_gate_host over the scripted scene of
tests/live_cases.py, against facts written out by hand; the arguments the two entry points refuse (they return MCG_ERR_ARG before any launch,
so this runs without a GPU); and GazeStreamPool.push keeping a host img_hw as it always did.  tests/test_gpu_live.py holds the kernels to
these twins bit for bit."""
import ctypes as C

import numpy as np
import pytest

from mcgaze_amd import lib as L
from mcgaze_amd import live
from mcgaze_amd.harness import plan_windows
from tests import live_cases as LC

CLIP, STRIDE = LC.CLIP, LC.STRIDE


@pytest.fixture(scope='module')
def plain():
    return LC.run_host(*LC.scene())


@pytest.fixture(scope='module')
def smoothed():
    return LC.run_host(*LC.scene(), smooth=True)


def slot(run, name, where):
    q, s = where
    return run[name][:, q, s]


def test_the_scene_is_the_one_described(plain):
    ids = np.stack([t['track_id'] for t in plain['ticks']])                   # [28, Q, S]
    assert ids[:, 0, 0].tolist() == [1] * 28                                  # A, its two coasting ticks included
    assert ids[:, 0, 1].tolist() == [2] * 12 + [0, 0] + [3] * 14              # B dies at tick 12, C is born at 14 in B's slot
    assert ids[:, 1, 0].tolist() == [0] * 6 + [1] * 21 + [0]                  # D: born at 6, last seen at 24, freed at 27
    assert [int(t['flags'][1]) for t in plain['ticks']] == [0] * 20 + [1] + [0] * 7      # six heads at tick 20: two found no slot
    assert [int(t['flags'][0]) for t in plain['ticks']] == [0] * 28
    matched_a = [int(t['matched'][0, 0]) for t in plain['ticks']]
    assert matched_a == [1] * 17 + [0, 0] + [1] * 9


def test_crop_table_and_ring_row(plain):
    R = live.ring_depth(CLIP)
    assert R == 16
    for t, rec in enumerate(plain['ticks']):
        ids = rec['track_id'].reshape(-1)
        assert rec['image_of'].tolist() == [(-1 if i == 0 else k // LC.S) for k, i in enumerate(ids)], t
        assert np.array_equal(rec['ring_id'].reshape(-1), ids) and np.array_equal(rec['ring_box'].reshape(-1, 4), rec['crop_boxes'])
        assert not rec['crop_boxes'][ids == 0].any(), t
    # a coasting slot keeps its last box: A's crop at ticks 17 and 18 is its box of tick 16
    for t in (16, 17, 18):
        assert plain['ticks'][t]['crop_boxes'][0].tolist() == list(LC.box_a(16)), t
    assert plain['ticks'][19]['crop_boxes'][0].tolist() == list(LC.box_a(19))


def test_frames_are_handed_out_on_the_pools_schedule(plain, smoothed):
    # frame f is final at tick f + clip_len; one tick later with smoothing; finish() returns the rest
    assert plain['emitted'][:8] == [(t, 0, 0) for t in range(7)] + [(7, 0, 1)]
    assert plain['emitted'][8:28] == [(t, t - 7, 1) for t in range(8, 28)] and plain['emitted'][28] == (27, 21, 7)
    assert smoothed['emitted'][8] == (8, 0, 1) and smoothed['emitted'][27] == (27, 19, 1) and smoothed['emitted'][28] == (27, 20, 8)
    assert plain['windows'] == plan_windows(28, CLIP, STRIDE)
    for run in (plain, smoothed):
        assert run['valid'].shape == (28, LC.Q, LC.S) and run['head_box'].shape == (28, LC.Q, LC.S, 4)


@pytest.mark.parametrize('which', ['plain', 'smoothed'])
def test_who_is_valid_where(which, plain, smoothed):
    run = plain if which == 'plain' else smoothed
    # A: every returned frame, the two it coasted through included
    assert slot(run, 'valid', LC.SLOT_A).tolist() == [1] * 28 and slot(run, 'track_id', LC.SLOT_A).tolist() == [1] * 28
    # B dies at tick d = 12: the last window wholly before it starts at ((d - clip) // stride) * stride = 4 and the next one takes over at 8,
    # so B's last valid frame is 7.  C is born at b = 14: the first multiple of stride at or after it is 16, plus clip - stride: 19.
    d, b = 12, 14
    last_b, first_c = ((d - CLIP) // STRIDE) * STRIDE + STRIDE - 1, -(-b // STRIDE) * STRIDE + CLIP - STRIDE
    assert (last_b, first_c) == (7, 19)
    assert slot(run, 'valid', LC.SLOT_BC).tolist() == [1] * 8 + [0] * 11 + [1] * 9
    assert slot(run, 'track_id', LC.SLOT_BC).tolist() == [2] * 12 + [0, 0] + [3] * 14      # the id of the frame's own tick, valid or not
    # camera 1: D is born at tick 6 -> no valid row before frame 8 + 3 = 11; its slot is free at tick 27, which only the flush-to-end
    # window (21, 28) of finish() reaches: frame 20 (windows (16, 23) and (20, 27)) is valid, frame 21 is not
    assert slot(run, 'valid', LC.SLOT_D).tolist() == [0] * 11 + [1] * 10 + [0] * 7
    assert not run['valid'][:, 1, 1:].any()                                   # the crowd of tick 20 lives three ticks: never a clean window
    assert not run['valid'][:, 0, 2:].any()
    # the box is the slot's at the frame's own tick, zero where invalid; image_of names frame (i, q) of the call that returned it
    for f in range(28):
        assert run['head_box'][f, 0, 0].tolist() == list(LC.box_a(16 if f in (17, 18) else f)), f
    assert not run['head_box'][run['valid'] == 0].any()
    assert (run['image_of'][run['valid'] == 0] == -1).all()
    assert slot(run, 'image_of', LC.SLOT_A)[:21 if which == 'plain' else 20].tolist() == [0] * (21 if which == 'plain' else 20)
    assert slot(run, 'image_of', LC.SLOT_A)[21 if which == 'plain' else 20:].tolist() == [2 * i for i in range(7 if which == 'plain' else 8)]


def test_the_flush_window_widens_the_span(plain):
    table, first_out = plain['tables'][-1]                                    # finish(): frames 21 .. 27
    assert first_out == 0 and table[:, 0].tolist() == list(range(21, 28))
    assert table[0].tolist() == [21, 16, 28, -1, -1]                          # (16, 23), (20, 27) and the flush-to-end (21, 28)
    assert table[2].tolist() == [23, 20, 28, -1, -1]
    assert plain['tables'][-2][0].tolist() == [[20, 16, 27, -1, -1]]          # frame 20: returned at tick 27, before the flush window existed


def test_smoothing_falls_back_next_to_an_invalid_neighbour(smoothed):
    sv, v = smoothed['smooth_valid'], smoothed['valid']
    assert not (sv & ~v.astype(bool)).any()
    assert slot(smoothed, 'smooth_valid', LC.SLOT_A).tolist() == [1] * 28
    # B: frame 7 is valid but its successor 8 is not; C: frame 19 is valid but its predecessor 18 is not
    assert slot(smoothed, 'smooth_valid', LC.SLOT_BC).tolist() == [1] * 7 + [0] * 13 + [1] * 8
    assert slot(smoothed, 'smooth_valid', LC.SLOT_D).tolist() == [0] * 12 + [1] * 8 + [0] * 8
    fused, others, fused_s, others_s = LC.fake_gaze(28, 0)
    raw = (v == 1) & (sv == 0)
    assert raw.sum() == 4                                                     # B's 7, C's 19, D's 11 and 20
    assert np.array_equal(smoothed['fused_smooth'][raw], fused[raw]) and np.array_equal(smoothed['others_smooth'][raw], others[raw])
    assert np.array_equal(smoothed['fused_smooth'][~raw], fused_s[~raw]) and np.array_equal(smoothed['others_smooth'][~raw], others_s[~raw])
    table, first_out = smoothed['tables'][5]                                  # frame 5, returned at tick 13 with neighbours 4 and 6
    assert first_out == 1 and table.tolist() == [[4, 0, 11, -1, -1], [5, 0, 11, 4, 6], [6, 0, 11, -1, -1]]
    table, first_out = smoothed['tables'][-1]                                 # finish(): the last frame has no successor
    assert first_out == 1 and table[1].tolist() == [20, 16, 27, 19, 21] and table[-1].tolist() == [27, 21, 28, 26, -1]


def test_a_slot_ring_is_a_lane_ring_whose_column_is_its_own_index(smoothed):
    """What the one gate rests on.  At every call that returned frames, the slot ring handed to live_gate_lanes_host as P = Q * S lanes,
    lane p naming column p where a person is and -1 elsewhere, gives the outputs of live_gate_host bit for bit, and camera / slot are
    p // S and p % S on the valid rows, -1 elsewhere."""
    cols = LC.Q * LC.S
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    calls = [c for c in smoothed['emitted'] if c[2]]
    assert len(calls) == len(smoothed['tables']) == 21 and sum(k for _, _, k in calls) == 28
    for (tick, first, k), (table, first_out) in zip(calls, smoothed['tables']):
        ring_id, ring_box, ring_col = LC.as_lane_ring(*LC.ring_at(smoothed, tick))
        gaze = [g.reshape((k, cols) + g.shape[3:]) for g in LC.fake_gaze(k, first)]
        got = live.live_gate_lanes_host(ring_id, ring_box, ring_col, LC.Q, LC.S, tick, table, first_out, k, *gaze)
        for name in ('track_id', 'valid', 'image_of', 'head_box', 'smooth_valid', 'fused_smooth', 'others_smooth'):
            want = smoothed[name][first:first + k]
            want = want.reshape((k, cols) + want.shape[3:])
            assert got[name].dtype == want.dtype and got[name].shape == want.shape and np.array_equal(bits(got[name]), bits(want)), (name, first)
        valid, p = got['valid'] == 1, np.arange(cols)[None]
        assert np.array_equal(got['camera'], np.where(valid, p // LC.S, -1)) and np.array_equal(got['slot'], np.where(valid, p % LC.S, -1)), first
        assert got['camera'].dtype == got['slot'].dtype == np.int32


def test_a_span_deeper_than_the_ring_raises():
    R = live.ring_depth(CLIP)
    ok = np.array([[20, 20 - R + 8, 28, -1, -1]], np.int32)
    assert live.check_gate_table(ok, 27, R) is not None
    with pytest.raises(ValueError, match='deeper than the ring'):
        live.check_gate_table(np.array([[20, 27 - R, 28, -1, -1]], np.int32), 27, R)
    with pytest.raises(ValueError, match='deeper than the ring'):
        live.check_gate_table(np.array([[27 - R, 20, 28, -1, -1]], np.int32), 27, R)
    with pytest.raises(ValueError):
        live.check_gate_table(np.array([[28, 20, 28, -1, -1]], np.int32), 27, R)     # a tick that has not been written
    with pytest.raises(ValueError):
        live.check_gate_table(np.zeros((2, 4), np.int32), 27, R)
    # the twin treats such an entry as the kernel does: no id, no valid row -- never a stale ring row
    ring_id, ring_box = np.ones((R, 1, 2), np.int32), np.ones((R, 1, 2, 4), np.float32)
    got = live.live_gate_host(ring_id, ring_box, 27, np.array([[20, 27 - R, 28, -1, -1]], np.int32), 0, 1)
    assert not got['track_id'].any() and not got['valid'].any() and not got['head_box'].any() and (got['image_of'] == -1).all()
    with pytest.raises(L.McgError):
        live.live_gate_table([(0, 7, 0)], 7, 1)                               # no window handed out covers frame 7


def test_host_twins_refuse_bad_arguments():
    R = 16
    ring_id, ring_box = np.zeros((R, 2, 4), np.int32), np.zeros((R, 2, 4, 4), np.float32)
    state = np.zeros((2, 4 + 8 * 4), np.int32)
    live.live_slots_host(state, 0, ring_id, ring_box)
    with pytest.raises(ValueError):
        live.live_slots_host(state, -1, ring_id, ring_box)
    with pytest.raises(ValueError):
        live.live_slots_host(state[:, :-1], 0, ring_id, ring_box)
    with pytest.raises(ValueError):
        live.live_slots_host(np.zeros((2, 4 + 8 * 65), np.int32), 0, np.zeros((R, 2, 65), np.int32), np.zeros((R, 2, 65, 4), np.float32))
    with pytest.raises(ValueError):
        live.live_gate_host(ring_id, ring_box, 3, np.zeros((1, 5), np.int32), 0, 2)
    with pytest.raises(ValueError):
        live.live_gate_host(ring_id, ring_box, 3, np.zeros((1, 5), np.int32), 0, 1, fused=np.zeros((1, 2, 4, 3), np.float32))


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every call here fails the host-side checks and returns MCG_ERR_ARG: nothing is launched, so no GPU is needed and no pointer is read."""
    lib = L.load()
    buf = (C.c_int32 * 64)()
    p, null = C.c_void_p(C.addressof(buf)), C.c_void_p(0)
    slots = lambda **kw: lib.mcg_live_slots(null, kw.get('state', p), kw.get('Q', 2), kw.get('S', 4), kw.get('tick', 0), kw.get('R', 16),
                                            kw.get('boxes', p), p, p, p, kw.get('matched', p))
    for bad in (dict(S=0), dict(S=65), dict(tick=-1), dict(R=0), dict(Q=-1), dict(Q=65536), dict(state=null), dict(boxes=null), dict(matched=null),
                dict(state=C.c_void_p(C.addressof(buf) + 4))):
        assert slots(**bad) != L.MCG_OK, bad
        assert b'mcg_live_slots' in lib.mcg_last_error()

    def gate(**kw):
        sm = kw.get('smooth', (null, null, null, null, null))
        return lib.mcg_live_gate(null, kw.get('ring', p), p, kw.get('R', 16), kw.get('Q', 2), kw.get('S', 4), kw.get('tick', 8), kw.get('table', p),
                                 kw.get('n', 3), kw.get('first', 1), kw.get('k', 1), sm[0], sm[1], sm[2], sm[3], kw.get('ids', p), p, p, p, sm[4])

    for bad in (dict(S=0), dict(S=65), dict(tick=-1), dict(R=0), dict(R=65537), dict(Q=-1), dict(n=-1), dict(n=65537), dict(first=-1), dict(k=-1),
                dict(first=3), dict(k=3), dict(ring=null), dict(table=null), dict(ids=null), dict(smooth=(p, p, p, null, p)),
                dict(smooth=(p, p, p, p, null)), dict(Q=65535, S=64, n=65536, first=0, k=65536)):
        assert gate(**bad) != L.MCG_OK, bad
        assert b'mcg_live_gate' in lib.mcg_last_error()
    assert gate(k=0) == L.MCG_OK and gate(Q=0) == L.MCG_OK and slots(Q=0) == L.MCG_OK      # nothing to do: no launch either


def test_pool_push_keeps_a_host_img_hw_as_it_was():
    """The device img_hw path is an addition: what push() queues for a host table is the int32 numpy array it always was."""
    import torch
    from mcgaze_amd.stream import GazeStreamPool, _on_device

    class Engine:
        device, dtype = 'cpu', torch.float32

        def decode(self):
            pass

    pool = GazeStreamPool(Engine(), 32, 32, rows=16)
    sid = pool.open()
    for hw in ([[20, 30], [32, 31]], np.array([[20, 30], [32, 31]], np.int64), torch.tensor([[20, 30], [32, 31]])):
        pool.push(sid, torch.zeros(2, 3, 32, 32), hw)
        queued = pool.streams[sid].queue[-1][1]
        assert isinstance(queued, np.ndarray) and queued.dtype == np.int32 and queued.tolist() == [[20, 30], [32, 31]]
        assert not _on_device(hw)
