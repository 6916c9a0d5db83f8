"""CPU: the host half of the device merge -- harness.merge_plan turns the windows of one decoder call into the per-destination-frame table
mcg_merge_windows (csrc/merge.hip) takes.  A numpy statement of the kernel (tests/merge_cases.py::emulate) applies such tables row by
row; plan + emulator must equal harness.merge_video BIT FOR BIT however the windows are dealt to calls, and reproduce the golden captured
from the reference's own main() (tests/golden/harness_merge.json).  Plus the table's rejections and the new surface.  No device."""
import json
import os
import re

import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import lib as L
from tests import merge_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize('clip_len,stride', MC.CONFIGS)
def test_plan_and_emulator_equal_merge_video(clip_len, stride):
    """L = 1..19 and 30, three ways of dealing the windows to calls: 60 cases per (clip_len, stride).  Scores sit at, just below and on
    both sides of the threshold.  (7, 4) at L = 12 is the plan whose last window overlaps TWO earlier ones."""
    longest = 0
    for L_ in list(range(1, 20)) + [30]:
        plan = harness.plan_windows(L_, clip_len, stride)
        rs = np.random.RandomState(1000 * clip_len + 100 * stride + L_)
        outs = [MC.window_outputs(rs, b - a) for a, b, _ in plan]
        want = MC.reference(plan, outs)
        for name, parts in MC.splits(len(plan)).items():
            store = np.full((L_, 27), np.nan, dtype=np.float32)
            longest = max(longest, MC.run_plan(plan, outs, parts, lambda t, m, g, b, s, sc: MC.emulate(t, m, g, b, s, sc, store)))
            assert np.array_equal(bits(store), bits(want)), (clip_len, stride, L_, name)
    assert longest == {(7, 4): 3, (5, 1): 5, (7, 7): 2, (3, 2): 2}[(clip_len, stride)]


def test_three_windows_on_one_frame_and_cont():
    """(7, 4), L = 12: the plan is (0,7), (4,11), (5,12); frames 5 and 6 gather three sources in ONE call, and in a later call they continue
    from the store (cont = 1) with the sources of that call only."""
    plan = harness.plan_windows(12)
    assert plan == [(0, 7, 3), (4, 11, 3), (5, 12, 6)]
    table, max_src = harness.merge_plan([(0, w, 7 * i) for i, w in enumerate(plan)], lambda k, f: f, set(), 21, 12)
    assert max_src == 3 and table.dtype == np.int32 and table.shape == (12, 5)
    assert table[:, 0].tolist() == list(range(12)) and not table[:, 1].any()
    assert table[5].tolist() == [5, 0, 5, 8, 14] and table[4].tolist() == [4, 0, 4, 7, -1] and table[11].tolist() == [11, 0, 20, -1, -1]
    written = {(0, f) for f in range(11)}
    table, max_src = harness.merge_plan([(0, plan[2], 0)], lambda k, f: 20 - f, written, 7, 21)
    assert max_src == 1 and table.tolist() == [[20 - f, int(f < 11), f - 5] for f in range(5, 12)]
    # two streams in one call: keys keep their frames apart
    table, _ = harness.merge_plan([('a', (0, 3, 0), 0), ('b', (0, 3, 0), 3)], lambda k, f: f + (3 if k == 'b' else 0), set(), 6, 6)
    assert table.tolist() == [[i, 0, i] for i in range(6)]


def test_golden_calls_through_the_plan(golden_dir):
    """The reference's own run (harness_merge.json): its calls, one decoder call each, through merge_plan + the emulator -> its records."""
    golden = json.load(open(os.path.join(golden_dir, 'harness_merge.json')))
    idx = 0
    for vid, L_ in enumerate(golden['video_lengths'], start=1):
        plan = harness.plan_windows(L_)
        outs, clips = [], []
        for a, b, _ in plan:
            det, fused, others = (t.numpy() for t in synth.fake_clip_outputs(vid, list(range(a, b)), call_index=idx))
            clips.append((det, fused, others))
            outs.append((np.ascontiguousarray(np.concatenate([fused[None], others.transpose(1, 0, 2)])), np.ascontiguousarray(det[..., :4]),
                         np.ascontiguousarray(det[..., 4])))
            idx += 1
        store = np.full((L_, 27), np.nan, dtype=np.float32)
        MC.run_plan(plan, outs, [[i] for i in range(len(plan))], lambda t, m, g, b, s, sc: MC.emulate(t, m, g, b, s, sc, store))
        host = harness.merge_video(plan, clips)
        assert np.array_equal(bits(store[:, :15]), bits(host[0].reshape(L_, 15))) and np.array_equal(bits(store[:, 15:18]), bits(host[1]))
        assert np.array_equal(bits(store[:, 18:]), bits(host[2].reshape(L_, 9)))
        rec = harness.video_record(vid, store[:, :15].reshape(L_, 3, 5), store[:, 15:18], store[:, 18:].reshape(L_, 3, 3))
        want = golden['results'][vid - 1]
        assert rec['video_id'] == want['video_id'] and set(rec) == set(want)
        for k, v in want.items():
            if k.endswith('_bboxes'):
                assert [x is None for x in rec[k]] == [x is None for x in v], (vid, k)
                np.testing.assert_allclose([x for x in rec[k] if x is not None], [x for x in v if x is not None], atol=1e-5)
            elif isinstance(v, list):
                np.testing.assert_allclose(np.array(rec[k], dtype=np.float64), np.array(v, dtype=np.float64), atol=1e-6, err_msg=f'{vid} {k}')
    assert idx == len(golden['calls'])


def test_bad_tables_are_rejected():
    row = lambda k, f: f
    with pytest.raises(ValueError, match='output rows'):          # a source row outside the call's n output frames
        harness.merge_plan([(0, (0, 7, 3), 0), (0, (4, 11, 3), 7)], row, set(), 13, 11)
    with pytest.raises(ValueError, match='output rows'):
        harness.merge_plan([(0, (0, 7, 3), -1)], row, set(), 7, 7)
    with pytest.raises(ValueError, match='plan order'):           # windows of one stream out of plan order, in one call
        harness.merge_plan([(0, (4, 11, 3), 0), (0, (0, 7, 3), 7)], row, set(), 14, 11)
    with pytest.raises(ValueError, match='plan order'):           # ... and across calls: (0, 7) after (4, 11) was written
        harness.merge_plan([(0, (0, 7, 3), 0)], row, {(0, f) for f in range(4, 11)}, 7, 11)
    with pytest.raises(ValueError, match='plan order'):           # a window skipped: (8, 15) straight after (0, 7)
        harness.merge_plan([(0, (0, 7, 3), 0), (0, (8, 15, 3), 7)], row, set(), 14, 15)
    with pytest.raises(ValueError, match='store row'):            # a dst_row outside the store
        harness.merge_plan([(0, (0, 7, 3), 0)], row, set(), 7, 6)
    with pytest.raises(ValueError, match='store row'):
        harness.merge_plan([(0, (0, 7, 3), 0)], lambda k, f: f - 1, set(), 7, 7)
    with pytest.raises(ValueError, match='share a store row'):
        harness.merge_plan([(0, (0, 7, 3), 0)], lambda k, f: f // 2, set(), 7, 7)
    # the other stream of the call is no excuse: every stream is checked on its own
    with pytest.raises(ValueError, match='plan order'):
        harness.merge_plan([('a', (0, 7, 3), 0), ('b', (4, 11, 3), 7), ('b', (0, 7, 3), 14)], lambda k, f: f + 20 * (k == 'b'), set(), 21, 40)


def test_surface():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    assert re.search(r'\bint mcg_merge_windows\(mcg_stream s, const float\* gaze, const float\* boxes, const float\* scores, int num_frames', hdr)
    assert 'tools/test_gaze360_gaze.py:129-206' in hdr and 'multiclue_gaze_roi_head.py:360-363' in hdr
    assert 'mcg_merge_windows' in L.EXPORTS and L.ABI_VERSION == 20
    assert int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) == 20
    lib = L.load()
    assert hasattr(lib, 'mcg_merge_windows') and len(lib.mcg_merge_windows.argtypes) == 13
    assert 'merge.hip' in open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'Makefile')).read()


class CpuEngine:
    dtype, device = torch.float32, torch.device('cpu')

    def decode(self, *a, **k):
        raise AssertionError('nothing may run')

    forward = backbone_fpn = decode


def test_device_merge_needs_a_device():
    """merge='device' on an engine without a HIP device is an error, not a quiet host merge."""
    from mcgaze_amd.stream import DeviceMerger, GazeStream, GazeStreamPool
    for make in (lambda: GazeStream(CpuEngine(), 32, 32, merge='device'), lambda: GazeStreamPool(CpuEngine(), 32, 32, merge='device'),
                 lambda: GazeStreamPool(CpuEngine(), 32, 32, merge='device', results='device'), lambda: DeviceMerger('cpu'),
                 lambda: harness.run_videos(CpuEngine(), [dict(id=1, frames=torch.zeros(9, 3, 32, 32))], merge='device')):
        with pytest.raises(L.McgError, match='HIP device'):
            make()
    for kw in (dict(merge='gpu'), dict(results='device'), dict(merge='device', results='numpy')):
        with pytest.raises(ValueError):
            GazeStreamPool(CpuEngine(), 32, 32, **kw)
        with pytest.raises(ValueError):
            GazeStream(CpuEngine(), 32, 32, **kw)
    with pytest.raises(ValueError):
        harness.run_videos(CpuEngine(), [], merge='gpu')
    GazeStreamPool(CpuEngine(), 32, 32)                       # the defaults are what they were


def test_head_arrows_takes_tensors():
    rs = np.random.RandomState(3)
    boxes = rs.uniform(0, 300, (40, 4))
    boxes[:, 2:] += boxes[:, :2]
    gaze = rs.standard_normal((40, 3)).astype(np.float32)
    want = harness.head_arrows(boxes, gaze)
    got = harness.head_arrows(boxes, torch.from_numpy(gaze))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    got = harness.head_arrows(torch.from_numpy(boxes.astype(np.float32)), torch.from_numpy(gaze))
    assert np.array_equal(got.numpy(), harness.head_arrows(boxes.astype(np.float32), gaze))
