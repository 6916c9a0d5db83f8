"""Gaze dwell without a GPU (include/mcgaze_hip.h, "gaze dwell"): attention.gaze_dwell_host against scenes worked by hand, against
itertools.groupby (enter 1, exit 0: an episode is a run), against a second, scalar statement of rules A to E (tests/dwell_cases.py), split
into chunks with the state carried, and the event table; then the boundary (export, header, ABI, the entry's argument checks, which return
before any launch) and the option checks of the layers above."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from mcgaze_amd import lib as L
from tests import dwell_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCG_ERR_ARG = 1                                                   # enum of include/mcgaze_hip.h
HAND = DC.hand_cases()
RANDOM = DC.random_cases()
SIZED = DC.sized_cases()


@pytest.mark.parametrize('case', HAND, ids=[c['name'] for c in HAND])
def test_hand_worked_scenes(case):
    DC.same(AT.gaze_dwell_host(**DC.args(case)), DC.as_results(case['expect'], case), case['name'])


@pytest.mark.parametrize('case', HAND + RANDOM + SIZED, ids=[c['name'] for c in HAND + RANDOM + SIZED])
def test_the_numpy_twin_equals_the_scalar_restatement(case):
    a = DC.args(case)
    before = None if a['state'] is None else a['state'].copy()
    DC.same(AT.gaze_dwell_host(**a), DC.dwell_scalar(**a), case['name'])
    assert before is None or (a['state'] == before).all()         # the twin hands back an updated COPY


def test_the_random_cases_hold_what_they_are_for():
    """Every reason occurs, flickers are bridged, candidates are dropped, regions are counted: or the comparisons would check nothing."""
    reasons, bridged = np.zeros(4, int), 0
    for case in RANDOM:
        a = DC.args(case)
        dwell, ended, events, num, state, rf = AT.gaze_dwell_host(**a)
        reasons += np.bincount(ended[..., 7].ravel(), minlength=4)[:4]
        frames = dwell[..., 3].astype(np.int64)
        bridged += int(((frames[1:] - frames[:-1] > 1) & (dwell[1:, :, 2] == dwell[:-1, :, 2]) & (dwell[1:, :, 0] != 0)).sum())
        assert int(num[0]) == int((ended[..., 7] != 0).sum()) > 0, case['name']
        if a['region_frames'] is not None and case.get('state') is None:
            assert (rf.astype(np.int64) - a['region_frames']).sum() > 0
    assert (reasons[1:] > 0).all() and bridged > 0, (reasons.tolist(), bridged)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_with_enter_1_and_exit_0_the_episodes_are_the_runs(seed):
    """An independent statement: ended episodes plus the open ones in the state are exactly the runs of itertools.groupby over each column's
    (person, tag, k, i), those of nobody and of "nothing" left out."""
    t = DC.random_tables(seed, 60, 6)
    frame0 = 1000
    dwell, ended, events, num, state, _ = AT.gaze_dwell_host(t['person'], t['kind'], t['ident'], t['mutual'], t['tag'], frame0=frame0, enter=1, exit=0)
    F, R = t['kind'].shape
    for c in range(R):
        keys = []
        for f in range(F):
            p = int(t['person'][f, c]) if t['person'][f, c] > 0 else 0
            k = int(t['kind'][f, c]) if 1 <= t['kind'][f, c] <= 3 else 0
            i = int(t['ident'][f, c]) if k in (1, 2) else 0
            keys.append((p, int(t['tag'][f, c]) if p else 0, k, i))
        runs, f = [], 0
        for key, grp in itertools.groupby(range(F), key=lambda f: keys[f]):
            grp = list(grp)
            if key[0] and key[2]:
                mutual = sum(int(key[2] == 1 and t['mutual'][f, c] != 0) for f in grp)
                runs.append((*key, frame0 + grp[0], len(grp), mutual, grp[-1] + 1))
        got = [tuple(int(v) for v in ended[f, c, :7]) + (f,) for f in range(F) if ended[f, c, 7]]
        if state[c, 0] and state[c, 2]:
            got.append(tuple(int(v) for v in state[c, :7]) + (F,))
        assert got == runs, c
        assert all(ended[f, c, 7] in (0, 1, 2) for f in range(F))


CHUNKED = [c for c in RANDOM if c['frame0'] < 2 ** 30]            # (a frame0 past 2^31 cannot be passed: the wrapping case is one call)


@pytest.mark.parametrize('case', CHUNKED, ids=[c['name'] for c in CHUNKED])
def test_chunks_with_the_state_carried_equal_one_call(case):
    a = DC.args(case)
    whole = AT.gaze_dwell_host(**a)
    F = a['kind'].shape[0]
    for cuts in ([0, 1, F], list(range(F + 1))):
        state, rf, parts = a['state'], a['region_frames'], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = {k: (None if a[k] is None else a[k][lo:hi]) for k in ('person', 'kind', 'ident', 'mutual', 'tag')}
            got = AT.gaze_dwell_host(**part, state=state, frame0=a['frame0'] + lo, enter=a['enter'], exit=a['exit'], region_frames=rf)
            state, rf = got[4], (got[5] if rf is not None else None)
            parts.append(got)
        assert (np.concatenate([g[0] for g in parts]) == whole[0]).all() and (np.concatenate([g[1] for g in parts]) == whole[1]).all()
        events = np.concatenate([g[2][:int(g[3][0])] for g in parts])
        assert (events == whole[2][:int(whole[3][0])]).all() and sum(int(g[3][0]) for g in parts) == int(whole[3][0])
        assert (parts[-1][4] == whole[4]).all() and (parts[-1][5] == whole[5]).all()


def test_events_are_ordered_counted_and_cut():
    case = RANDOM[2]
    a = DC.args(case)
    dwell, ended, events, num, state, rf = AT.gaze_dwell_host(**a)
    total = int(num[0])
    F, R = a['kind'].shape
    assert total > 8 and events.shape == (F * R, 10) and not events[total:].any()
    order = (events[:total, 0].astype(np.int64) - a['frame0']) * R + events[:total, 1]
    assert (np.diff(order) > 0).all()                             # ascending (frame, column), no row twice
    f, c = events[:total, 0] - a['frame0'], events[:total, 1]
    assert (events[:total, 2:] == ended[f, c]).all()
    for E in (0, 1, total - 1, total, total + 3):
        cut = AT.gaze_dwell_host(**dict(a, max_events=E))
        assert cut[2].shape == (E, 10) and int(cut[3][0]) == total
        assert (cut[2][:min(E, total)] == events[:min(E, total)]).all() and not cut[2][total:].any()
        assert all((x == y).all() for x, y in zip((cut[0], cut[1], cut[4], cut[5]), (dwell, ended, state, rf)))


def test_constants_and_signatures():
    assert (AT.DWELL_ENTER, AT.DWELL_EXIT) == (3, 2)
    assert (AT.END_LOOKED_AWAY, AT.END_OWNER_LEFT, AT.END_REPLACED, AT.END_VIDEO_ENDED) == (1, 2, 3, 4)
    assert AT.STATE_WORDS[:14] == ('person', 'tag', 'cur_kind', 'cur_ident', 'cur_start', 'cur_frames', 'cur_mutual', 'gap', 'cand_kind', 'cand_ident',
                                   'cand_start', 'cand_frames', 'cand_mutual', 'seen') and len(AT.STATE_WORDS) == 16
    assert AT.STATE_INDEX['cand_frames'] == 11 and AT.ENDED_FIELDS[-1] == 'reason' and AT.EVENT_FIELDS[:2] == ('frame', 'column')
    want = [('tag', None), ('state', None), ('frame0', 0), ('enter', 3), ('exit', 2), ('region_frames', None), ('max_events', None)]
    sig = inspect.signature(AT.gaze_dwell_host)
    assert list(sig.parameters)[:4] == ['person', 'kind', 'ident', 'mutual'] and [(p.name, p.default) for p in list(sig.parameters.values())[4:]] == want
    from mcgaze_amd import pipeline as P
    sig = inspect.signature(P.DevicePipeline.gaze_dwell)
    assert list(sig.parameters)[1:5] == ['person', 'kind', 'ident', 'mutual']
    assert [(p.name, p.default) for p in list(sig.parameters.values())[5:12]] == want and list(sig.parameters)[12:] == ['device', 'stream']
    assert hasattr(P.DevicePipeline, 'dwell_state')


@pytest.mark.parametrize('bad', [dict(enter=0), dict(enter=65537), dict(enter=1.5), dict(enter=True), dict(exit=-1), dict(exit=65537), dict(frame0=-1),
                                 dict(max_events=-1), dict(max_events=65537), dict(kind=np.zeros((3, 2), np.int32)), dict(tag=np.zeros((2, 3), np.int32)),
                                 dict(person=np.zeros(6, np.int32)), dict(state=np.zeros((2, 16), np.int32)), dict(state=np.zeros((1, 8), np.int32)),
                                 dict(region_frames=np.zeros(AT.MAX_REGIONS + 1, np.int32))], ids=repr)
def test_host_argument_checks(bad):
    a = DC.args(HAND[0])
    with pytest.raises(ValueError):
        AT.gaze_dwell_host(**dict(a, **bad))


def test_host_tables_must_hold_integers_and_fit():
    a = DC.args(HAND[0])
    with pytest.raises(TypeError):
        AT.gaze_dwell_host(**dict(a, kind=a['kind'].astype(np.float32)))
    z = np.zeros((17, 4096), np.int32)
    with pytest.raises(ValueError):
        AT.gaze_dwell_host(z, z, z, z)                            # 17 * 4096 rows > 65536
    z = np.zeros((1, 4097), np.int32)
    with pytest.raises(ValueError):
        AT.gaze_dwell_host(z, z, z, z)
    empty = AT.gaze_dwell_host(*[np.zeros((0, 3), np.int32)] * 4)
    assert [x.shape for x in empty] == [(0, 3, 4), (0, 3, 8), (0, 10), (1,), (3, 16), (0,)] and int(empty[3][0]) == 0


def test_header_binding_and_library_agree_on_the_new_entry():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    assert 'mcg_gaze_dwell' in L.EXPORTS and re.search(r'\bint mcg_gaze_dwell\(', hdr) and hasattr(lib, 'mcg_gaze_dwell')
    declared = re.search(r'\bint mcg_gaze_dwell\(([^;]*)\);', hdr).group(1)
    assert len(lib.mcg_gaze_dwell.argtypes) == len(declared.split(',')) == 19
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20 and '#define MCG_ABI_VERSION 20' in hdr
    assert 'dwell.hip' in open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'Makefile')).read()
    assert hdr.index('gaze dwell (additions') > hdr.index('gaze targets (additions')
    for phrase in ('AT MOST ONE END', 'not tuned on data', 'modulo 2^32', 'ascending (frame, column)'):
        assert phrase in hdr[hdr.index('gaze dwell (additions'):], phrase
    assert 'dwell-time accumulation' not in hdr                   # struck from the out-of-scope list of the gaze targets


def test_the_entry_checks_its_host_arguments_before_any_launch():
    """Counts, parameters, null pointers and alignment are argument errors; no device is needed to be told so."""
    lib = L.load()
    p = C.c_void_p(256)                                           # never dereferenced: every call below fails its checks first
    ok = dict(person=p, tag=p, kind=p, ident=p, mutual=p, F=1, R=1, frame0=0, enter=3, exit=2, state=p, rf=None, M=0, dwell=p, ended=p, events=p, E=1,
              num=p)
    order = ('person', 'tag', 'kind', 'ident', 'mutual', 'F', 'R', 'frame0', 'enter', 'exit', 'state', 'rf', 'M', 'dwell', 'ended', 'events', 'E', 'num')
    call = lambda **kw: lib.mcg_gaze_dwell(None, *(dict(ok, **kw)[k] for k in order))
    odd = C.c_void_p(264)
    for kw in (dict(R=0), dict(R=4097), dict(F=-1), dict(F=17, R=4096), dict(F=65537), dict(M=-1), dict(M=4097, rf=p), dict(E=-1), dict(E=65537),
               dict(frame0=-1), dict(enter=0), dict(enter=65537), dict(exit=-1), dict(exit=65537), dict(person=None), dict(kind=None), dict(ident=None),
               dict(mutual=None), dict(state=None), dict(dwell=None), dict(ended=None), dict(M=1), dict(rf=p), dict(events=None), dict(num=None),
               dict(state=odd), dict(dwell=odd), dict(ended=odd), dict(events=C.c_void_p(260))):
        assert call(**kw) == MCG_ERR_ARG, kw
        assert b'mcg_gaze_dwell' in lib.mcg_last_error(), kw
    assert call(F=0, person=None, kind=None, ident=None, mutual=None, dwell=None, ended=None) == L.MCG_OK     # F == 0 launches nothing


@pytest.mark.parametrize('dwell', [5, 'yes', False, dict(enter=0), dict(exit=-1), dict(enter=2.5), dict(frames=3)], ids=repr)
def test_live_gaze_and_run_head_video_check_the_dwell_option_before_anything_else(dwell):
    with pytest.raises(ValueError):
        live.LiveGaze(None, None, cameras=1, slots=4, attention=True, dwell=dwell)
    with pytest.raises(ValueError):
        harness.run_head_video(None, None, [], boxes_per_frame=[], attention=True, dwell=dwell)


def test_dwell_needs_attention():
    with pytest.raises(ValueError, match='attention'):
        live.LiveGaze(None, None, cameras=1, slots=4, dwell=True)
    with pytest.raises(ValueError, match='attention'):
        harness.run_head_video(None, None, [], boxes_per_frame=[], dwell=dict(enter=2, exit=1))
    assert inspect.signature(live.LiveGaze).parameters['dwell'].default is None
    assert inspect.signature(harness.run_head_video).parameters['dwell'].default is None
    assert AT._dwell_options('x', True, True) == dict(enter=3, exit=2) and AT._dwell_options('x', dict(exit=0), True) == dict(enter=3, exit=0)
    assert AT._dwell_options('x', None, None) is None


def test_open_episodes_become_video_ended_records():
    """harness: the episodes of run_head_video's records from the event table and the last state, reason 4 for those still open."""
    case = HAND[1]
    dwell, ended, events, num, state, _ = AT.gaze_dwell_host(**DC.args(case))
    ids = {3: 'a', 11: 'b', 12: 'c'}
    got = harness._dwell_episodes(events[:int(num[0])], state, 1, lambda person: ids[person])
    assert got == [[dict(kind=1, target_id='b', start=0, frames=4, mutual_frames=3, reason=3),
                    dict(kind=1, target_id='c', start=4, frames=3, mutual_frames=2, reason=4)]]


def test_the_demo_tool_takes_dwell(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location('demo_video', os.path.join(ROOT, 'tools', 'demo_video.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(SystemExit, match='--dwell belongs to --attention'):
        tool.main(['-', '-', 'cfg', 'ckpt', '--out', str(tmp_path / 'o.json'), '--dwell'])
    assert tool.dwell_option('') == True and tool.dwell_option('4,1') == dict(enter=4, exit=1)      # noqa: E712
    with pytest.raises(SystemExit):
        tool.dwell_option('4')
