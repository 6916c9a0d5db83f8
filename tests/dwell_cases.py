"""Cases for the gaze dwell (include/mcgaze_hip.h, "gaze dwell"), shared by tests/test_dwell_cpu.py and tests/test_gpu_dwell.py: scenes worked
by hand with every output written out, seeded random tables drawn from a small alphabet of persons and targets (so that episodes form),
tables at the sizes where the kernels change path, and ``dwell_scalar``: rules A to E once more, one column and one frame at a time in
plain Python ints -- written from the header, not from attention.gaze_dwell_host.

A case is a dict: name, person / kind / ident / mutual [F][R], tag ([F][R] or None), frame0, enter, exit, state ([R][16] or None),
region_frames ([M] or None); hand cases add expect = dict(dwell, ended, state, region_frames, events).  ``args(case)`` gives the keyword
arguments of gaze_dwell_host."""
import numpy as np

OUT = ('dwell', 'ended', 'events', 'num_events', 'state', 'region_frames')     # the order of the six results


def args(case):
    a = {k: np.asarray(case[k], dtype=np.int32) for k in ('person', 'kind', 'ident', 'mutual')}
    a['tag'] = None if case.get('tag') is None else np.asarray(case['tag'], dtype=np.int32)
    a['state'] = None if case.get('state') is None else np.asarray(case['state'], dtype=np.int32)
    a['region_frames'] = None if case.get('region_frames') is None else np.asarray(case['region_frames'], dtype=np.int32)
    a.update(frame0=case.get('frame0', 0), enter=case.get('enter', 3), exit=case.get('exit', 2))
    if 'max_events' in case:
        a['max_events'] = case['max_events']
    return a


def same(got, want, what):
    """The six results, bit for bit; of ``events`` the rows both hold (behind the count they are zero in both)."""
    assert len(got) == len(want) == 6
    for name, g, w in zip(OUT, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == np.int32 and w.dtype == np.int32, (what, name, g.dtype, w.dtype)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def u32(v):
    return v & 0xffffffff


def i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >= (1 << 31) else v


def dwell_scalar(person, kind, ident, mutual, tag=None, state=None, frame0=0, enter=3, exit=2, region_frames=None, max_events=None):
    """Rules A to E of the header in plain Python ints, a column at a time -> the six results as int32 arrays."""
    F, R = np.asarray(person).shape
    person, kind, ident, mutual = (np.asarray(t).tolist() for t in (person, kind, ident, mutual))
    tag = [[0] * R for _ in range(F)] if tag is None else np.asarray(tag).tolist()
    st = [[0] * 16 for _ in range(R)] if state is None else [[int(v) for v in row] for row in np.asarray(state).tolist()]
    rf = [] if region_frames is None else [int(v) for v in np.asarray(region_frames).tolist()]
    M = len(rf)
    dwell = [[[0] * 4 for _ in range(R)] for _ in range(F)]
    ended = [[[0] * 8 for _ in range(R)] for _ in range(F)]
    for c in range(R):
        s = st[c]
        for f in range(F):
            n = i32(frame0 + f)
            p = person[f][c] if person[f][c] > 0 else 0
            g = tag[f][c] if p else 0
            k = kind[f][c] if 1 <= kind[f][c] <= 3 else 0
            i = ident[f][c] if k in (1, 2) else 0
            m = 1 if k == 1 and mutual[f][c] != 0 else 0
            ends = []
            # A
            if s[0] != 0 and (s[0], s[1]) != (p, g):
                if s[2] != 0:
                    ends.append(s[:7] + [2])
                s[:] = [0] * 16
            if p == 0:
                assert len(ends) <= 1
                if ends:
                    ended[f][c] = ends[0]
                continue
            s[0], s[1] = p, g
            # B
            s[13] = i32(s[13] + 1)
            if k == 2 and 0 <= i < M:
                rf[i] = i32(rf[i] + 1)
            # C
            is_current = False
            if s[2] != 0:
                if (k, i) == (s[2], s[3]):
                    s[5] = i32(u32(s[5]) + 1 + u32(s[7]))
                    s[7] = 0
                    s[6] = i32(s[6] + m)
                    s[8:13] = [0] * 5
                    is_current = True
                else:
                    s[7] = i32(s[7] + 1)
                    if s[7] > exit:
                        ends.append(s[:7] + [1])
                        s[2:8] = [0] * 6
            # D
            if not is_current:
                if k == 0:
                    s[8:13] = [0] * 5
                elif (k, i) == (s[8], s[9]):
                    s[11] = i32(s[11] + 1)
                    s[12] = i32(s[12] + m)
                else:
                    s[8:13] = [k, i, n, 1, m]
                if s[11] >= enter:
                    if s[2] != 0:
                        ends.append(s[:7] + [3])
                    s[2:7] = s[8:13]
                    s[7] = 0
                    s[8:13] = [0] * 5
            # E
            assert len(ends) <= 1, 'at most one END per row and frame'
            dwell[f][c] = s[2:6]
            if ends:
                ended[f][c] = ends[0]
    E = F * R if max_events is None else max_events
    rows = [[i32(frame0 + f), c] + ended[f][c] for f in range(F) for c in range(R) if any(ended[f][c])]
    events = np.zeros((E, 10), np.int32)
    if rows[:E]:
        events[:len(rows[:E])] = np.asarray(rows[:E], dtype=np.int32)
    a = lambda v, *shape: np.asarray(v, dtype=np.int32).reshape(*shape)
    return a(dwell, F, R, 4), a(ended, F, R, 8), events, a([len(rows)], 1), a(st, R, 16), a(rf, M)


def as_results(expect, case):
    """A hand case's expect dict -> the six results (events: the listed rows, zero rows up to F * R)."""
    F, R = np.asarray(case['kind']).shape
    events = np.zeros((F * R, 10), np.int32)
    listed = np.asarray(expect['events'], dtype=np.int32).reshape(-1, 10)
    events[:len(listed)] = listed
    a = lambda v, *shape: np.asarray(v, dtype=np.int32).reshape(*shape)
    return (a(expect['dwell'], F, R, 4), a(expect['ended'], F, R, 8), events, a([len(listed)], 1), a(expect['state'], R, 16),
            a(expect['region_frames'], -1))


def _col(values):
    """One column's values -> [F][1]."""
    return [[v] for v in values]


Z4, Z8 = [0, 0, 0, 0], [0] * 8


def hand_cases():
    cases = []
    # ---- enter 3, exit 2: region 5 is looked at for 4 frames, lost for 2 (bridged: they count), seen 2 more, then lost for 3 -> ends
    kind = [2, 2, 2, 2, 0, 0, 2, 2, 0, 0, 0, 0]
    look = [2, 5, 100]
    cases.append(dict(
        name='a look survives a two-frame flicker and ends on a three-frame one', person=_col([7] * 12), kind=_col(kind), ident=_col([5] * 12),
        mutual=_col([1] * 12), tag=None, frame0=100, enter=3, exit=2, region_frames=[0] * 8,
        expect=dict(dwell=[[Z4], [Z4], [look + [3]], [look + [4]], [look + [4]], [look + [4]], [look + [7]], [look + [8]], [look + [8]], [look + [8]],
                           [Z4], [Z4]],
                    ended=[[Z8]] * 10 + [[[7, 0, 2, 5, 100, 8, 0, 1]], [Z8]],
                    state=[[7, 0] + [0] * 11 + [12, 0, 0]], region_frames=[0, 0, 0, 0, 0, 6, 0, 0], events=[[110, 0, 7, 0, 2, 5, 100, 8, 0, 1]])))
    # ---- a replacement needs enter <= exit (the candidate's frames are the current target's gap): enter 2, exit 3
    cases.append(dict(
        name='a replacement, with mutual frames and a tag', person=_col([3] * 7), tag=_col([9] * 7), kind=_col([1] * 7),
        ident=_col([11, 11, 11, 11, 12, 12, 12]), mutual=_col([0, 1, 1, 5, -1, 0, 1]), frame0=0, enter=2, exit=3, region_frames=None,
        expect=dict(dwell=[[Z4], [[1, 11, 0, 2]], [[1, 11, 0, 3]], [[1, 11, 0, 4]], [[1, 11, 0, 4]], [[1, 12, 4, 2]], [[1, 12, 4, 3]]],
                    ended=[[Z8]] * 5 + [[[3, 9, 1, 11, 0, 4, 3, 3]], [Z8]],
                    state=[[3, 9, 1, 12, 4, 3, 2, 0, 0, 0, 0, 0, 0, 7, 0, 0]], region_frames=[], events=[[5, 0, 3, 9, 1, 11, 0, 4, 3, 3]])))
    # ---- column 0: the owner changes; column 1: the tag changes, then the person is gone (person <= 0).  Kind 3 ignores its ident.
    cases.append(dict(
        name='an owner change, a tag change and person <= 0', person=[[5, 4], [5, 4], [6, 4], [6, -1]], tag=[[0, 1], [0, 2], [0, 2], [0, 2]],
        kind=[[3, 2]] * 4, ident=[[99, 1]] * 4, mutual=[[1, 1]] * 4, frame0=0, enter=1, exit=2, region_frames=[0, 0],
        expect=dict(dwell=[[[3, 0, 0, 1], [2, 1, 0, 1]], [[3, 0, 0, 2], [2, 1, 1, 1]], [[3, 0, 2, 1], [2, 1, 1, 2]], [[3, 0, 2, 2], Z4]],
                    ended=[[Z8, Z8], [Z8, [4, 1, 2, 1, 0, 1, 0, 2]], [[5, 0, 3, 0, 0, 2, 0, 2], Z8], [Z8, [4, 2, 2, 1, 1, 2, 0, 2]]],
                    state=[[6, 0, 3, 0, 2, 2, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0], [0] * 16], region_frames=[0, 3],
                    events=[[1, 1, 4, 1, 2, 1, 0, 1, 0, 2], [2, 0, 5, 0, 3, 0, 0, 2, 0, 2], [3, 1, 4, 2, 2, 1, 1, 2, 0, 2]])))
    # ---- kinds outside 0 .. 3 are "nothing"; a region ident outside [0, M) is a target like any other but counts nowhere
    odd = dict(person=_col([1] * 6), tag=None, kind=_col([7, -1, 2, 2, 2, 4]), ident=_col([3, 3, -1, 5, 1, 0]), mutual=_col([1] * 6), frame0=0, enter=1,
               exit=0)
    expect = dict(dwell=[[Z4], [Z4], [[2, -1, 2, 1]], [[2, 5, 3, 1]], [[2, 1, 4, 1]], [Z4]],
                  ended=[[Z8], [Z8], [Z8], [[1, 0, 2, -1, 2, 1, 0, 1]], [[1, 0, 2, 5, 3, 1, 0, 1]], [[1, 0, 2, 1, 4, 1, 0, 1]]],
                  state=[[1, 0] + [0] * 11 + [6, 0, 0]],
                  events=[[3, 0, 1, 0, 2, -1, 2, 1, 0, 1], [4, 0, 1, 0, 2, 5, 3, 1, 0, 1], [5, 0, 1, 0, 2, 1, 4, 1, 0, 1]])
    cases.append(dict(odd, name='kinds outside 0 .. 3 and a region ident outside [0, M)', region_frames=[10, 20], expect=dict(expect, region_frames=[10, 21])))
    cases.append(dict(odd, name='M = 0', region_frames=None, expect=dict(expect, region_frames=[])))
    return cases


PARAMS = ((3, 2), (2, 3), (1, 0), (2, 0), (1, 5), (3, 6))       # (enter, exit): reason 3 needs enter <= exit


def random_tables(seed, F, R, M=5, stay=0.9):
    """[F][R] tables from a small alphabet, sticky over frames: persons change rarely, targets flicker."""
    rng = np.random.default_rng(seed)
    persons, tags = np.asarray([0, -3, 1, 2, 3, 4]), np.asarray([0, 1])
    targets = np.asarray([(0, 0), (1, 2), (1, 3), (2, 0), (2, 1), (2, M + 1), (2, -1), (3, 0), (3, 7), (5, 1), (-1, 0)])

    def sticky(n_values, keep):
        first = rng.integers(0, n_values, R)
        draw = rng.integers(0, n_values, (F, R))
        change = rng.random((F, R)) >= keep
        out = np.empty((F, R), np.int64)
        cur = first
        for f in range(F):
            cur = np.where(change[f], draw[f], cur)
            out[f] = cur
        return out

    who = persons[sticky(len(persons), 0.93 if stay > 0.5 else stay)]
    t = targets[sticky(len(targets), stay * 0.85)]
    return dict(person=who.astype(np.int32), tag=tags[sticky(2, 0.97)].astype(np.int32), kind=t[..., 0].astype(np.int32), ident=t[..., 1].astype(np.int32),
                mutual=rng.integers(-1, 2, (F, R)).astype(np.int32), region_frames=rng.integers(0, 50, M).astype(np.int32))


def random_cases():
    cases = []
    for n, (enter, exit) in enumerate(PARAMS):
        cases.append(dict(random_tables(100 + n, 48, 7), name=f'random enter {enter} exit {exit}', frame0=17 * n, enter=enter, exit=exit))
    # whatever the state and the tables hold: a state of arbitrary words, counters next to 2^31 and 2^32, frame numbers that wrap
    rng = np.random.default_rng(7)
    t = random_tables(200, 40, 9)
    state = rng.integers(-2 ** 31, 2 ** 31, (9, 16)).astype(np.int32)
    state[:4, 0], state[:4, 1] = t['person'][0, :4], t['tag'][0, :4]              # some owners stay, so their words are walked on
    state[:4, 2], state[:4, 3] = t['kind'][0, :4], t['ident'][0, :4]
    state[0, 5:8] = 2 ** 31 - 1, 2 ** 31 - 1, -1
    state[1, 5:8] = -1, -1, 2 ** 31 - 1
    state[2, 8:14] = t['kind'][0, 2], t['ident'][0, 2], 5, 2 ** 31 - 1, -1, -1
    cases.append(dict(t, name='arbitrary state, wrapping counters', state=state, frame0=2 ** 31 - 3, enter=2, exit=3,
                      region_frames=np.asarray([2 ** 31 - 1, -1, 0, 5, -2 ** 31], np.int32)))
    cases.append(dict(random_tables(201, 30, 5), name='tag None', tag=None, frame0=0, enter=2, exit=2))
    return cases


def owner_change_case(R=600):
    """Every column changes owner in frame 2, each in the middle of an episode: R events in one frame."""
    F = 4
    person = np.tile(np.arange(1, R + 1, dtype=np.int32), (F, 1))
    person[2:] += R
    return dict(name=f'{R} owners change at once', person=person, tag=None, kind=np.full((F, R), 3, np.int32), ident=np.zeros((F, R), np.int32),
                mutual=np.zeros((F, R), np.int32), frame0=5, enter=1, exit=0, region_frames=None)


def sized_cases():
    """The sizes where the kernels change path: the 256-column workgroup edge, F = 1, 2, 37, the 1024-row compaction tile edge."""
    cases = []
    for n, (F, R) in enumerate([(3, 1), (37, 255), (2, 256), (1, 257), (5, 600), (31, 33), (32, 32), (25, 41)]):
        enter, exit = PARAMS[n % len(PARAMS)]
        cases.append(dict(random_tables(300 + n, F, R, stay=0.6 if F > 4 else 0.3), name=f'F {F} R {R} (rows {F * R})', frame0=n, enter=enter, exit=exit))
    # F = 1 and 2 end nothing from an empty state: give them one that holds episodes
    for c in cases:
        F, R = c['kind'].shape
        if F <= 3:
            warm = random_tables(400 + R, 6, R, stay=0.9)
            c['state'] = dwell_scalar(warm['person'], warm['kind'], warm['ident'], warm['mutual'], warm['tag'], enter=1, exit=0)[4]
    cases.append(owner_change_case())
    return cases


def all_cases():
    return hand_cases() + random_cases()
