"""mcg_gaze_dwell on the device against attention.gaze_dwell_host, every output and the state bit for bit (include/mcgaze_hip.h, "gaze
dwell"): every case of tests/dwell_cases.py, the 256-column workgroup edge, the 1024-row tile edge of the compaction, 600 owners changing
in one frame, the event table cut short, the state carried over calls, graph capture, and guard words around every output and the state."""
import ctypes as C

import numpy as np
import pytest
import torch

from mcgaze_amd import attention as AT
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import dwell_cases as DC
from tests.test_gpu_nv12 import chain

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CASES = DC.all_cases()
SIZED = DC.sized_cases()
TABLES = ('person', 'kind', 'ident', 'mutual', 'tag')
GUARD, MARK = 64, 0x5a5a5a5a                                      # 64 words: the payload stays 16-byte aligned


@pytest.fixture(scope='module')
def pipe():
    return P.DevicePipeline(chain(64))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def on_device(pipe, a, tables=True):
    """gaze_dwell over the arguments of gaze_dwell_host: tables as device tensors, or as they are (numpy, through the staging ring); the state
    and region_frames go up as tensors (they are updated in place) -> the six results on the host."""
    a = dict(a)
    for k in TABLES + ('state', 'region_frames'):
        if a[k] is not None and (tables or k in ('state', 'region_frames')):
            a[k] = dev(a[k])
    given = a['state'], a['region_frames']
    got = pipe.gaze_dwell(a.pop('person'), a.pop('kind'), a.pop('ident'), a.pop('mutual'), device=DEV, **a)
    torch.cuda.synchronize()
    assert given[0] is None or got[4] is given[0]                 # in place
    assert given[1] is None or got[5] is given[1]
    return tuple(g.cpu().numpy() for g in got)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_every_cpu_case(pipe, case):
    want = AT.gaze_dwell_host(**DC.args(case))
    DC.same(on_device(pipe, DC.args(case)), want, case['name'] + ' (device tables)')
    DC.same(on_device(pipe, DC.args(case), tables=False), want, case['name'] + ' (host tables)')


def guarded(words):
    return torch.full((GUARD + words + GUARD,), MARK, dtype=torch.int32, device=DEV)


def entry_between_guards(a, E, events=True):
    """The entry itself, every output and the state inside guarded arrays -> (dwell, ended, events, num_events, state, region_frames) on the
    host; the guard words are checked here."""
    lib = L.load()
    F, R = a['kind'].shape
    M = 0 if a['region_frames'] is None else len(a['region_frames'])
    state = np.zeros((R, 16), np.int32) if a['state'] is None else a['state']
    sizes = dict(dwell=F * R * 4, ended=F * R * 8, events=E * 10, num=1, state=R * 16, rf=M)
    bufs = {k: guarded(n) for k, n in sizes.items()}
    bufs['state'][GUARD:GUARD + R * 16] = dev(state.reshape(-1))
    if M:
        bufs['rf'][GUARD:GUARD + M] = dev(a['region_frames'])
    tables = [None if a[k] is None else dev(a[k]) for k in TABLES]
    vp = C.c_void_p
    at = lambda k: vp(bufs[k].data_ptr() + 4 * GUARD)
    ptr = lambda t: vp(None) if t is None else vp(t.data_ptr())
    person, kind, ident, mutual, tag = tables
    L.check(lib.mcg_gaze_dwell(vp(torch.cuda.current_stream().cuda_stream), ptr(person), ptr(tag), ptr(kind), ptr(ident), ptr(mutual), F, R, a['frame0'],
                               a['enter'], a['exit'], at('state'), at('rf') if M else vp(None), M, at('dwell'), at('ended'),
                               at('events') if events else vp(None), E if events else 0, at('num') if events else vp(None)), 'mcg_gaze_dwell')
    torch.cuda.synchronize()
    out = {}
    for k, n in sizes.items():
        o = bufs[k].cpu().numpy()
        assert (o[:GUARD] == MARK).all() and (o[GUARD + n:] == MARK).all(), k
        out[k] = o[GUARD:GUARD + n]
    return (out['dwell'].reshape(F, R, 4), out['ended'].reshape(F, R, 8), out['events'].reshape(E, 10), out['num'], out['state'].reshape(R, 16), out['rf'])


def same_with_marked_events(got, want, what):
    """The entry leaves the rows of ``events`` behind the count as they were: the mark here, zero in the twin."""
    E, total = len(want[2]), int(want[3][0])
    assert (got[2][min(E, total):] == MARK).all(), what
    got[2][min(E, total):] = 0
    DC.same(got, want, what)


@pytest.mark.parametrize('case', SIZED, ids=[c['name'] for c in SIZED])
def test_workgroup_and_tile_edges_between_guard_words(pipe, case):
    """R = 1, 255, 256, 257, 600 (256 columns a workgroup), F = 1, 2, 37, F * R = 1023, 1024, 1025 (1024 rows a compaction tile), and 600
    owners that change in one frame: 600 events of one frame, in column order."""
    a = DC.args(case)
    F, R = a['kind'].shape
    want = AT.gaze_dwell_host(**a)
    total = int(want[3][0])
    assert total > 0, case['name']
    if 'owners' in case['name']:
        assert total == R and (want[2][:R, 0] == a['frame0'] + 2).all() and (want[2][:R, 1] == np.arange(R)).all() and (want[2][:R, 9] == 2).all()
    same_with_marked_events(entry_between_guards(a, F * R), want, case['name'])
    DC.same(on_device(pipe, a), want, case['name'] + ' (pipeline)')


def test_the_event_table_cut_short_absent_and_full():
    case = SIZED[4]                                               # F 5, R 600
    a = DC.args(case)
    F, R = a['kind'].shape
    want = AT.gaze_dwell_host(**a)
    total = int(want[3][0])
    assert total > 40
    for E in (0, 7, total - 1, total, F * R):
        same_with_marked_events(entry_between_guards(a, E), AT.gaze_dwell_host(**dict(a, max_events=E)), f'E = {E}')
    got = entry_between_guards(a, 5, events=False)                # events NULL: no second launch, no count
    assert (got[2] == MARK).all() and (got[3] == MARK).all()
    for k in (0, 1, 4, 5):
        assert np.array_equal(got[k], want[k]), k


def test_max_events_through_the_pipeline(pipe):
    a = DC.args(DC.random_cases()[2])
    total = int(AT.gaze_dwell_host(**a)[3][0])
    for E in (0, 3, total):
        DC.same(on_device(pipe, dict(a, max_events=E)), AT.gaze_dwell_host(**dict(a, max_events=E)), f'max_events = {E}')


def test_the_state_carried_over_three_calls_and_tag_none(pipe):
    case = DC.random_cases()[1]
    a = DC.args(case)
    whole = AT.gaze_dwell_host(**a)
    F = a['kind'].shape[0]
    state, rf = pipe.dwell_state(a['kind'].shape[1], device=DEV), dev(a['region_frames'])
    assert tuple(state.shape) == (a['kind'].shape[1], 16) and state.dtype == torch.int32 and not state.any().item()
    parts = []
    for lo, hi in ((0, 1), (1, 20), (20, F)):
        got = pipe.gaze_dwell(*(dev(a[k][lo:hi]) for k in ('person', 'kind', 'ident', 'mutual')), tag=dev(a['tag'][lo:hi]), state=state, frame0=a['frame0'] + lo,
                              enter=a['enter'], exit=a['exit'], region_frames=rf, device=DEV)
        assert got[4] is state and got[5] is rf
        parts.append([g.cpu().numpy() for g in got[:4]])
    assert np.array_equal(np.concatenate([p[0] for p in parts]), whole[0]) and np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
    assert np.array_equal(np.concatenate([p[2][:int(p[3][0])] for p in parts]), whole[2][:int(whole[3][0])])
    assert np.array_equal(state.cpu().numpy(), whole[4]) and np.array_equal(rf.cpu().numpy(), whole[5])
    # tag NULL is a table of zeros
    zero = dict(a, tag=np.zeros_like(a['kind']))
    DC.same(on_device(pipe, dict(a, tag=None)), AT.gaze_dwell_host(**zero), 'tag None against zeros')
    DC.same(on_device(pipe, zero), AT.gaze_dwell_host(**dict(a, tag=None)), 'zeros against tag None')


def test_a_host_table_next_to_device_tables_is_moved_with_torch(pipe):
    """The five tables are decided as a group: with one of them on the device none goes through the staging ring."""
    a = DC.args(next(c for c in DC.hand_cases() if c['name'] == 'an owner change, a tag change and person <= 0'))
    assert a['tag'].any()                                         # the tag decides two of the three events
    want = AT.gaze_dwell_host(**a)
    for host in (('tag',), ('person', 'kind', 'ident', 'mutual')):
        b = {k: v if k in host or k not in TABLES + ('region_frames',) else dev(v) for k, v in a.items()}
        assert all(isinstance(b[k], np.ndarray) for k in host) and sum(isinstance(b[k], torch.Tensor) for k in TABLES) == 5 - len(host)
        before = pipe._ring.i
        got = pipe.gaze_dwell(b.pop('person'), b.pop('kind'), b.pop('ident'), b.pop('mutual'), device=DEV, **b)
        assert pipe._ring.i == before
        torch.cuda.synchronize()
        DC.same(tuple(g.cpu().numpy() for g in got), want, f'{host} on the host')


def test_option_and_shape_checks_raise_before_any_launch(pipe):
    a = DC.args(DC.hand_cases()[0])
    t = [dev(a[k]) for k in ('person', 'kind', 'ident', 'mutual')]
    for bad in (dict(enter=0), dict(exit=-1), dict(frame0=-1), dict(max_events=-1), dict(tag=dev(np.zeros((3, 3), np.int32)))):
        with pytest.raises(ValueError):
            pipe.gaze_dwell(*t, device=DEV, **bad)
    with pytest.raises(ValueError):
        pipe.gaze_dwell(t[0], t[1][:3], t[2], t[3], device=DEV)
    with pytest.raises(ValueError):
        pipe.gaze_dwell(*t, state=torch.zeros(2, 16, dtype=torch.int32, device=DEV), device=DEV)
    for bad in (dict(state=np.zeros((1, 16), np.int32)), dict(state=torch.zeros(1, 16, dtype=torch.int64, device=DEV)),
                dict(region_frames=torch.zeros(2, 2, dtype=torch.int32, device=DEV)), dict(kind=t[1].float())):
        with pytest.raises(TypeError):
            pipe.gaze_dwell(*(bad.get(k, v) for k, v in zip(('person', 'kind', 'ident', 'mutual'), t)), device=DEV,
                            **{k: v for k, v in bad.items() if k in ('state', 'region_frames')})
    empty = pipe.gaze_dwell(*(x[:0] for x in t), device=DEV)
    assert [tuple(x.shape) for x in empty] == [(0, 1, 4), (0, 1, 8), (0, 10), (1,), (1, 16), (0,)] and empty[3].item() == 0


def test_the_call_is_capturable(pipe):
    """Device tables, state and totals, captured once, replayed with new contents in the same buffers: equal to eager, state carried."""
    first, second, third = (DC.random_tables(s, 12, 300) for s in (31, 32, 33))
    bufs = {k: dev(first[k]) for k in TABLES}
    state, rf = pipe.dwell_state(300, device=DEV), dev(first['region_frames'])
    call = lambda: pipe.gaze_dwell(bufs['person'], bufs['kind'], bufs['ident'], bufs['mutual'], tag=bufs['tag'], state=state, frame0=40, enter=2, exit=3,
                                   region_frames=rf, device=DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()                                                    # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    host_state, host_rf = state.cpu().numpy(), rf.cpu().numpy()   # after the warm-up: what the replays continue from
    for n, case in enumerate((second, third)):
        for k in TABLES:
            bufs[k].copy_(dev(case[k]))
        graph.replay()
        torch.cuda.synchronize()
        want = AT.gaze_dwell_host(case['person'], case['kind'], case['ident'], case['mutual'], case['tag'], state=host_state, frame0=40, enter=2, exit=3,
                                  region_frames=host_rf)
        host_state, host_rf = want[4], want[5]
        assert int(want[3][0]) > 0
        DC.same(tuple(x.cpu().numpy() for x in out), want, f'replay {n}')
