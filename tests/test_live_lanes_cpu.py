"""The live chain with lanes on the host (mcgaze_amd/live.py): live_lanes_host and live_gate_lanes_host over the scenes of
tests/live_lanes_cases.py, against facts written out by hand; the arguments mcg_live_lanes and mcg_live_gate_lanes refuse (they return
MCG_ERR_ARG before any launch, so this runs without a GPU); and LiveGaze's validation of ``lanes``.  tests/test_gpu_live_lanes.py holds the
kernels to these twins bit for bit."""
import ctypes as C

import numpy as np
import pytest

from mcgaze_amd import lib as L
from mcgaze_amd import live
from mcgaze_amd.head_detect import track_state_words
from tests import live_cases as LC
from tests import live_lanes_cases as LL

CLIP, STRIDE = LL.CLIP, LL.STRIDE


@pytest.fixture(scope='module')
def main6():
    return LC.run_host(*LL.scene('main'), lanes=6)


@pytest.fixture(scope='module')
def main4():
    return LC.run_host(*LL.scene('main'), lanes=4)


@pytest.fixture(scope='module')
def queue():
    return LC.run_host(*LL.scene('queue'), lanes=LL.QUEUE_LANES)


@pytest.fixture(scope='module')
def queue_smoothed():
    return LC.run_host(*LL.scene('queue'), smooth=True, lanes=LL.QUEUE_LANES)


def lanes_at(run, t):
    """The lane table after tick t as [(id, column) or None]."""
    return [tuple(r) if r[0] else None for r in run['ticks'][t]['lane_state'].tolist()]


def make_state(ids, boxes=None, ages=None, Q=LC.Q, S=LC.S):
    """A tracker state with the given slot ids [Q][S]."""
    state = np.zeros((Q, track_state_words(S)), np.int32)
    table = state[:, 4:].reshape(Q, S, 8)
    table[..., 4] = np.asarray(ids, np.int32).reshape(Q, S)
    if ages is not None:
        table[..., 5] = np.asarray(ages, np.int32).reshape(Q, S)
    if boxes is not None:
        table[..., :4] = np.asarray(boxes, np.float32).reshape(Q, S, 4).view(np.int32)
    return state


def rings(P, R=16):
    return np.zeros((R, P), np.int32), np.zeros((R, P, 4), np.float32), np.zeros((R, P), np.int32)


# ---------------------------------------------------------------- 'main' with a lane for everybody
def test_main_with_six_lanes(main6):
    A, B, C_, D = (1, 0), (2, 1), (3, 1), (1, 4)                  # (id, column); C is born in B's slot; D is id 1 of camera 1
    for t in range(28):
        want = [A, B if t < 12 else (C_ if t >= 14 else None), D if 6 <= t < 27 else None] + [None] * 3
        if 20 <= t <= 22:
            want[3:] = [(2, 5), (3, 6), (4, 7)]                    # the three crowd heads that got slots, in ascending column order
        assert lanes_at(main6, t) == want, t
        assert main6['ticks'][t]['overflow'].tolist() == [0], t
    # lane 1 is free at ticks 12 and 13, and C takes it at 14: the lowest free lane, not a fresh one
    assert main6['ticks'][12]['lane_of'].tolist() == [[0, -1, -1, -1], [2, -1, -1, -1]]
    assert main6['ticks'][14]['lane_of'].tolist() == [[0, 1, -1, -1], [2, -1, -1, -1]]
    assert main6['ticks'][20]['lane_of'].tolist() == [[0, 1, -1, -1], [2, 3, 4, 5]]
    assert main6['ticks'][5]['lane_of'].tolist() == [[0, 1, -1, -1], [-1] * 4]


def test_the_tables_of_a_tick(main6):
    R = live.ring_depth(CLIP)
    assert R == 16
    for t, rec in enumerate(main6['ticks']):
        ids, col = rec['lane_state'][:, 0], rec['lane_state'][:, 1]
        held = ids != 0
        assert rec['image_of'].tolist() == [(int(c) // LC.S if h else -1) for c, h in zip(col, held)], t
        assert np.array_equal(rec['ring_id'], ids) and np.array_equal(rec['ring_col'], np.where(held, col, -1)), t
        assert np.array_equal(rec['ring_box'], rec['crop_boxes']) and not rec['crop_boxes'][~held].any(), t
        assert not rec['matched'][~held].any() and not col[~held].any(), t
        for p in np.flatnonzero(held):                             # lane_of is the inverse of the lane table
            assert rec['lane_of'].reshape(-1)[col[p]] == p, t
        assert (rec['lane_of'] >= 0).sum() == held.sum(), t
    # a coasting slot keeps its last box and its lane: A at ticks 17 and 18; matched says which
    for t in (16, 17, 18):
        assert main6['ticks'][t]['crop_boxes'][0].tolist() == list(LC.box_a(16)), t
    assert [int(rec['matched'][0]) for rec in main6['ticks']] == [1] * 17 + [0, 0] + [1] * 9
    assert main6['ticks'][8]['crop_boxes'][2].tolist() == list(LC.box_d(8)) and main6['ticks'][8]['image_of'][2] == 1
    assert main6['ticks'][20]['crop_boxes'][3].tolist() == list(LC.CROWD[0])


def test_lane_rows_equal_the_fixed_schedules_slot_rows(main6):
    """With a lane for everybody nobody waits: a person's rows are those of their slot in the fixed schedule."""
    fixed = LC.run_host(*LC.scene())
    assert main6['emitted'] == fixed['emitted']
    for p, (q, s) in enumerate((LC.SLOT_A, LC.SLOT_BC, LC.SLOT_D)):
        for name in ('track_id', 'valid', 'head_box', 'image_of'):
            assert np.array_equal(main6[name][:, p], fixed[name][:, q, s]), (name, p)
        v = main6['valid'][:, p] == 1
        assert (main6['camera'][:, p][v] == q).all() and (main6['slot'][:, p][v] == s).all()
        assert (main6['camera'][:, p][~v] == -1).all() and (main6['slot'][:, p][~v] == -1).all()
    assert not main6['valid'][:, 3:].any() and main6['valid'].sum() == fixed['valid'].sum() == 28 + 17 + 10


# ---------------------------------------------------------------- 'main' with four lanes: overflow
def test_main_with_four_lanes_overflows(main4):
    for t in range(28):
        crowd = 20 <= t <= 22
        assert main4['ticks'][t]['overflow'].tolist() == [2 if crowd else 0], t
        assert lanes_at(main4, t)[3] == ((2, 5) if crowd else None), t
        live_slots = main4['ticks'][t]['track_id'] > 0
        left_out = live_slots & (main4['ticks'][t]['lane_of'] == -1)
        assert np.argwhere(left_out).tolist() == ([[1, 2], [1, 3]] if crowd else []), t
    assert lanes_at(main4, 19)[:3] == lanes_at(main4, 20)[:3] == [(1, 0), (3, 1), (1, 4)]      # nobody loses a lane to the crowd


# ---------------------------------------------------------------- 'queue': a person waits for a lane
def test_queue_scene_lanes(queue):
    ids = np.stack([t['track_id'] for t in queue['ticks']])
    assert ids[:, 0, 0].tolist() == [1] * 12 + [0] * 16           # A: detected up to 9, coasts 10 and 11, freed at 12
    assert ids[:, 0, 1].tolist() == [0] * 4 + [2] * 24            # C
    assert ids[:, 1, 0].tolist() == [1] * 28                      # D
    for t in range(28):
        rec = queue['ticks'][t]
        assert lanes_at(queue, t) == [(1, LL.COL_A) if t < 12 else (2, LL.COL_C), (1, LL.COL_D)], t
        assert rec['overflow'].tolist() == [1 if 4 <= t <= 11 else 0], t
        assert rec['lane_of'][0, 1] == (-1 if t < 12 else 0) and rec['lane_of'][0, 0] == (0 if t < 12 else -1) and rec['lane_of'][1, 0] == 1, t
    # tick 12: lane 0 is released (A's slot is free) and taken by C in the same call; its crop is C's from that tick on
    assert queue['ticks'][11]['crop_boxes'][0].tolist() == list(LC.box_a(9)) and queue['ticks'][11]['matched'].tolist() == [0, 1]
    assert queue['ticks'][12]['crop_boxes'][0].tolist() == list(LC.box_c(12)) and queue['ticks'][12]['matched'].tolist() == [1, 1]
    assert queue['ticks'][12]['image_of'].tolist() == [0, 1]


@pytest.mark.parametrize('which', ['plain', 'smoothed'])
def test_queue_scene_rows(which, queue, queue_smoothed):
    run = queue if which == 'plain' else queue_smoothed
    # A's slot is freed at tick d = 12: the last window wholly before it starts at ((d - clip) // stride) * stride = 4 and the next takes over
    # at 8, so A's last valid frame is 7.  C got its lane at tick g = 12 (it was born at 4 and waited): the first multiple of stride at or
    # after g is 12, plus clip - stride: 15.  In the fixed schedule C would be valid from 4 + 3 = 7.
    d, g = 12, 12
    last_a, first_c = ((d - CLIP) // STRIDE) * STRIDE + STRIDE - 1, -(-g // STRIDE) * STRIDE + CLIP - STRIDE
    assert (last_a, first_c) == (7, 15)
    assert run['valid'][:, 0].tolist() == [1] * 8 + [0] * 7 + [1] * 13
    assert run['track_id'][:, 0].tolist() == [1] * 12 + [2] * 16  # the id of the frame's own tick, valid or not
    assert run['valid'][:, 1].tolist() == [1] * 28 and run['track_id'][:, 1].tolist() == [1] * 28      # D throughout
    # camera / slot name the slot on every valid row, -1 on the others
    assert run['camera'][:, 0].tolist() == [0] * 8 + [-1] * 7 + [0] * 13
    assert run['slot'][:, 0].tolist() == [0] * 8 + [-1] * 7 + [1] * 13
    assert run['camera'][:, 1].tolist() == [1] * 28 and run['slot'][:, 1].tolist() == [0] * 28
    for f in range(28):
        want = LC.box_a(f) if f < 8 else (LC.box_c(f) if f >= 15 else (0, 0, 0, 0))
        assert run['head_box'][f, 0].tolist() == list(want), f
        assert run['head_box'][f, 1].tolist() == list(LC.box_d(f)), f
    # image_of = i * Q + camera within the call that returned the frame: one frame per call until finish()
    n = 21 if which == 'plain' else 20
    assert run['image_of'][:n, 1].tolist() == [1] * n and run['image_of'][n:, 1].tolist() == [2 * i + 1 for i in range(28 - n)]
    assert run['image_of'][n:, 0].tolist() == [2 * i for i in range(28 - n)]
    assert (run['image_of'][:, 0][run['valid'][:, 0] == 0] == -1).all()


def test_smoothing_falls_back_next_to_an_invalid_neighbour(queue_smoothed):
    sv, v = queue_smoothed['smooth_valid'], queue_smoothed['valid']
    # A's frame 7 is valid but its successor 8 is not; C's frame 15 is valid but its predecessor 14 is not
    assert sv[:, 0].tolist() == [1] * 7 + [0] * 9 + [1] * 12 and sv[:, 1].tolist() == [1] * 28
    fused, others, fused_s, others_s = LC.fake_gaze(28, 0, LL.QUEUE_LANES)
    raw = (v == 1) & (sv == 0)
    assert np.argwhere(raw).tolist() == [[7, 0], [15, 0]]
    assert np.array_equal(queue_smoothed['fused_smooth'][raw], fused[raw]) and np.array_equal(queue_smoothed['others_smooth'][raw], others[raw])
    assert np.array_equal(queue_smoothed['fused_smooth'][~raw], fused_s[~raw]) and np.array_equal(queue_smoothed['others_smooth'][~raw], others_s[~raw])


# ---------------------------------------------------------------- the rules, one at a time
def test_a_zero_state_is_all_free_and_more_lanes_than_slots_work():
    P = LC.Q * LC.S + 3
    ring_id, ring_box, ring_col = rings(P)
    lane_state = np.zeros((P, 2), np.int32)
    state = make_state([[5, 0, 7, 0], [0, 0, 0, 9]], ages=[[0, 0, 1, 0], [0, 0, 0, 0]])
    crop_boxes, image_of, lane_of, matched, overflow = live.live_lanes_host(state, 3, lane_state, ring_id, ring_box, ring_col)
    assert lane_state[:3].tolist() == [[5, 0], [7, 2], [9, 7]] and not lane_state[3:].any()
    assert lane_of.tolist() == [[0, -1, 1, -1], [-1, -1, -1, 2]] and overflow.tolist() == [0]
    assert image_of.tolist() == [0, 0, 1] + [-1] * (P - 3) and matched.tolist() == [1, 0, 1] + [0] * (P - 3)
    assert ring_id[3].tolist() == [5, 7, 9] + [0] * (P - 3) and ring_col[3].tolist() == [0, 2, 7] + [-1] * (P - 3)
    assert not ring_id[:3].any() and not ring_id[4:].any()        # one ring row per tick


def test_release_rules():
    ring_id, ring_box, ring_col = rings(6)
    state = make_state([[5, 6, 0, 0], [5, 0, 0, 8]])
    # lane 0: its slot holds its id -- kept.  lane 1: column out of range -- freed, not followed.  lane 2: a negative column -- freed.
    # lane 3: the slot was handed to another person (id 6, not 4) -- freed.  lane 4: the slot is free -- freed.  lane 5: a second lane
    # naming column 0 -- the lowest lane keeps the slot.
    lane_state = np.array([[5, 0], [5, 8], [5, -4], [4, 1], [3, 2], [5, 0]], np.int32)
    _, _, lane_of, _, overflow = live.live_lanes_host(state, 0, lane_state, ring_id, ring_box, ring_col)
    # the waiting slots, ascending: column 1 (id 6), 4 (id 5 of camera 1), 7 (id 8) take the free lanes 1, 2, 3
    assert lane_state.tolist() == [[5, 0], [6, 1], [5, 4], [8, 7], [0, 0], [0, 0]]
    assert lane_of.tolist() == [[0, 1, -1, -1], [2, -1, -1, 3]] and overflow.tolist() == [0]
    huge = np.array([[5, 0x7fffffff], [5, -0x80000000]], np.int32)
    r2 = rings(2)
    _, _, lane_of, _, overflow = live.live_lanes_host(state, 0, huge, *r2)
    assert huge.tolist() == [[5, 0], [6, 1]] and overflow.tolist() == [2]


def test_the_same_id_in_another_camera_is_another_person():
    """Ids are per camera.  A lane handed within one tick from id 1 of camera 0 to id 1 of camera 1 keeps ring_id 1 throughout: the ring
    of columns is what makes the rows around the hand-over invalid."""
    P, R = 1, 16
    ring_id, ring_box, ring_col = rings(P, R)
    lane_state = np.zeros((P, 2), np.int32)
    for t in range(12):
        ids = [[1, 0, 0, 0], [0] * 4] if t < 6 else [[0] * 4, [1, 0, 0, 0]]
        live.live_lanes_host(make_state(ids), t, lane_state, ring_id, ring_box, ring_col)
    assert ring_id[:12, 0].tolist() == [1] * 12 and ring_col[:12, 0].tolist() == [0] * 6 + [4] * 6
    table = np.array([[2, 0, 6, -1, -1], [3, 0, 7, -1, -1], [8, 6, 12, -1, -1], [8, 5, 12, -1, -1]], np.int32)
    got = live.live_gate_lanes_host(ring_id, ring_box, ring_col, 2, 4, 11, table, 0, 4)
    assert got['valid'][:, 0].tolist() == [1, 0, 1, 0] and got['camera'][:, 0].tolist() == [0, -1, 1, -1]
    assert got['image_of'][:, 0].tolist() == [0, -1, 2 * 2 + 1, -1] and got['track_id'][:, 0].tolist() == [1] * 4
    # with smoothing, a neighbour on the other side of the hand-over is not the same person
    table = np.array([[5, 2, 6, 4, 6], [4, 2, 6, -1, -1], [6, 6, 10, -1, -1]], np.int32)
    z3, z9 = np.zeros((1, 1, 3), np.float32), np.zeros((1, 1, 3, 3), np.float32)
    got = live.live_gate_lanes_host(ring_id, ring_box, ring_col, 2, 4, 11, table, 0, 1, z3 + 1, z9 + 2, z3 + 3, z9 + 4)
    assert got['valid'].tolist() == [[1]] and got['smooth_valid'].tolist() == [[0]]
    assert (got['fused_smooth'] == 1).all() and (got['others_smooth'] == 2).all()          # the raw gaze


def test_an_entry_outside_the_ring_gives_no_row():
    ring_id, ring_box, ring_col = np.ones((16, 2), np.int32), np.ones((16, 2, 4), np.float32), np.ones((16, 2), np.int32)
    got = live.live_gate_lanes_host(ring_id, ring_box, ring_col, 2, 4, 27, np.array([[20, 27 - 16, 28, -1, -1]], np.int32), 0, 1)
    assert not got['track_id'].any() and not got['valid'].any() and not got['head_box'].any()
    assert (got['image_of'] == -1).all() and (got['camera'] == -1).all() and (got['slot'] == -1).all()
    # a valid row whose ring column is not a slot of this table names no camera: a value, never an index
    ring_col[:] = 99
    got = live.live_gate_lanes_host(ring_id, ring_box, ring_col, 2, 4, 27, np.array([[20, 20, 27, -1, -1]], np.int32), 0, 1)
    assert got['valid'].all() and (got['camera'] == -1).all() and (got['image_of'] == -1).all()


def test_host_twins_refuse_bad_arguments():
    state = make_state([[0] * 4] * 2)
    ok = lambda P=2: (np.zeros((P, 2), np.int32),) + rings(P)
    live.live_lanes_host(state, 0, *ok())
    with pytest.raises(ValueError):
        live.live_lanes_host(state, -1, *ok())
    with pytest.raises(ValueError):
        live.live_lanes_host(state[:, :-1], 0, *ok())
    with pytest.raises(ValueError):
        live.live_lanes_host(state, 0, *ok(1025))
    with pytest.raises(ValueError):
        live.live_lanes_host(state, 0, np.zeros((3, 2), np.int32), *rings(2))
    with pytest.raises(ValueError):
        live.live_lanes_host(np.zeros((65, track_state_words(64)), np.int32), 0, *ok())    # 4160 columns
    with pytest.raises(ValueError):
        live.live_gate_lanes_host(*rings(2), 2, 4, 3, np.zeros((1, 5), np.int32), 0, 2)
    with pytest.raises(ValueError):
        live.live_gate_lanes_host(*rings(2), 2, 4, 3, np.zeros((1, 5), np.int32), 0, 1, fused=np.zeros((1, 2, 3), np.float32))
    with pytest.raises(ValueError):
        live.live_gate_lanes_host(*rings(2), 65, 64, 3, np.zeros((1, 5), np.int32), 0, 1)


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every call here fails the host-side checks and returns MCG_ERR_ARG: nothing is launched, so no GPU is needed and no pointer is read."""
    lib = L.load()
    buf = (C.c_int32 * 64)()
    p, null = C.c_void_p(C.addressof(buf)), C.c_void_p(0)

    def lanes(**kw):
        return lib.mcg_live_lanes(null, kw.get('state', p), kw.get('Q', 2), kw.get('S', 4), kw.get('P', 2), kw.get('tick', 0), kw.get('R', 16),
                                  kw.get('lane_state', p), kw.get('boxes', p), p, p, p, kw.get('ring_col', p), kw.get('lane_of', p), p,
                                  kw.get('overflow', p))

    for bad in (dict(P=0), dict(P=1025), dict(P=-1), dict(Q=65, S=64), dict(Q=4097, S=1), dict(S=0), dict(S=65), dict(tick=-1), dict(R=0),
                dict(R=65537), dict(Q=-1), dict(Q=65536), dict(state=null), dict(lane_state=null), dict(boxes=null), dict(ring_col=null),
                dict(lane_of=null), dict(overflow=null), dict(state=C.c_void_p(C.addressof(buf) + 4))):
        assert lanes(**bad) != L.MCG_OK, bad
        assert b'mcg_live_lanes' in lib.mcg_last_error(), bad

    def gate(**kw):
        sm = kw.get('smooth', (null, null, null, null, null))
        return lib.mcg_live_gate_lanes(null, kw.get('ring', p), p, kw.get('ring_col', p), kw.get('R', 16), kw.get('Q', 2), kw.get('S', 4),
                                       kw.get('P', 2), kw.get('tick', 8), kw.get('table', p), kw.get('n', 3), kw.get('first', 1), kw.get('k', 1),
                                       sm[0], sm[1], sm[2], sm[3], kw.get('ids', p), p, kw.get('camera', p), kw.get('slot', p), p, p, sm[4])

    for bad in (dict(P=0), dict(P=1025), dict(Q=65, S=64), dict(S=0), dict(S=65), dict(tick=-1), dict(R=0), dict(R=65537), dict(Q=-1), dict(n=-1),
                dict(n=65537), dict(first=-1), dict(k=-1), dict(first=3), dict(k=3), dict(ring=null), dict(ring_col=null), dict(table=null),
                dict(ids=null), dict(camera=null), dict(slot=null), dict(smooth=(p, p, p, null, p)), dict(smooth=(p, null, null, null, null)),
                dict(smooth=(p, p, p, p, null))):
        assert gate(**bad) != L.MCG_OK, bad
        assert b'mcg_live_gate_lanes' in lib.mcg_last_error(), bad
    assert gate(k=0) == L.MCG_OK and gate(Q=0) == L.MCG_OK and lanes(Q=0) == L.MCG_OK      # nothing to do: no launch either


def test_livegaze_validates_lanes_before_it_builds_anything():
    """No engine, no pipeline, no GPU: the check of ``lanes`` precedes the pool."""
    for bad in (0, True, 1025, -3, 2.0, '4'):
        with pytest.raises(ValueError, match='lanes'):
            live.LiveGaze(None, None, cameras=2, slots=4, lanes=bad)
    with pytest.raises(ValueError, match='4096'):
        live.LiveGaze(None, None, cameras=65, slots=64, lanes=8)


def test_the_abi_is_unchanged_and_the_entries_are_exported():
    assert L.ABI_VERSION == 20 and L.load().mcg_abi_version() == 20
    assert 'mcg_live_lanes' in L.EXPORTS and 'mcg_live_gate_lanes' in L.EXPORTS
    assert hasattr(L.load(), 'mcg_live_lanes') and hasattr(L.load(), 'mcg_live_gate_lanes')
