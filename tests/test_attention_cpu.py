"""Gaze targets without a GPU (include/mcgaze_hip.h, "gaze targets"): attention.gaze_targets_host against scenes worked by hand and against a
second, scalar statement of the arithmetic (tests/attention_cases.py), the boundary (exports, header, ABI) and the argument checks of the
layers above.  run_head_video(attention=...) itself needs an engine, and the engine has no host form: it is covered in
tests/test_gpu_attention.py only."""
import inspect
import os
import re

import numpy as np
import pytest

from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from mcgaze_amd import lib as L
from tests import attention_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = AC.all_cases()
HAND = AC.hand_cases()


@pytest.mark.parametrize('case', HAND, ids=[c['name'] for c in HAND])
def test_hand_worked_scenes(case):
    AC.same_tables(AT.gaze_targets_host(**AC.args(case)), AC.as_tables(case['expect']), case['name'])


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_numpy_twin_equals_the_scalar_restatement(case):
    got = AT.gaze_targets_host(**AC.args(case))
    assert [a.dtype for a in got] == [np.int32, np.int32, np.float32, np.float32, np.int32, np.int32]
    AC.same_tables(got, AC.as_tables(AC.targets_scalar(**AC.args(case))), case['name'])


def test_the_random_cases_hold_what_they_are_for():
    """Ties at equal t, every kind, mutual pairs and unusable rows occur in the random tables, or they would check nothing."""
    seen, ties = np.zeros(4, int), 0
    for case in CASES[len(HAND):]:
        kind, target, t, hit, mutual, flags = AT.gaze_targets_host(**AC.args(case))
        seen += np.bincount(kind, minlength=4)
        if not case['name'].startswith('random'):
            continue
        assert (flags == 2).any() and (flags == 0).any()
        a = AC.args(case)
        # a tie: the row's winner taken out of the tables, another candidate enters at the very same t
        for i in np.flatnonzero(kind == AT.KIND_HEAD)[:40]:
            boxes = a['boxes'].copy()
            boxes[target[i]] = np.nan
            k2, _, t2, _, _, _ = AT.gaze_targets_host(**dict(a, boxes=boxes))
            ties += int(k2[i] in (1, 2) and t2[i] == t[i])
    assert (seen > 0).all() and ties > 0, (seen.tolist(), ties)


def test_signed_zero_and_the_kind_codes():
    a, b = (c for c in HAND if c['name'] in ('d_x == 0 with o_x inside the slab', 'gx = -0.0 is gx = +0.0'))
    assert np.signbit(b['gaze'][0, 0]) and not np.signbit(a['gaze'][0, 0])
    AC.same_tables(AT.gaze_targets_host(**AC.args(a)), AT.gaze_targets_host(**AC.args(b)), 'signed zero')
    assert (AT.KIND_NONE, AT.KIND_HEAD, AT.KIND_REGION, AT.KIND_CAMERA) == (0, 1, 2, 3) and AT.FIELDS == AC.FIELDS
    assert (AT.EXPAND, AT.CAMERA_ANGLE) == (0.25, 10.0)
    sig = inspect.signature(AT.gaze_targets_host)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[2:]] == [
        ('image_of', None), ('regions', None), ('region_image', None), ('region_period', 0), ('expand', 0.25), ('camera_angle', 10.0)]


def test_image_of_none_is_one_picture_and_torch_tables_are_read():
    import torch
    c = HAND[0]
    a = AC.args(c)
    want = AT.gaze_targets_host(**a)
    AC.same_tables(AT.gaze_targets_host(a['boxes'], a['gaze']), want, 'image_of None')
    AC.same_tables(AT.gaze_targets_host(torch.from_numpy(a['boxes']), torch.from_numpy(a['gaze']), torch.from_numpy(a['image_of'])), want, 'torch')
    AC.same_tables(AT.gaze_targets_host(a['boxes'].astype(np.float64), a['gaze'].tolist(), a['image_of'].astype(np.int64)), want, 'other dtypes')


@pytest.mark.parametrize('bad', [dict(expand=-0.1), dict(expand=float('nan')), dict(expand=float('inf')), dict(expand='1'), dict(camera_angle=-1),
                                 dict(camera_angle=91), dict(camera_angle=float('nan')), dict(region_period=-1), dict(region_period=1.5),
                                 dict(regions=np.zeros((2, 3))), dict(regions=np.zeros((2, 4)), region_image=[0]), dict(region_image=[0]),
                                 dict(image_of=[0]), dict(gaze=np.zeros((2, 2))), dict(boxes=np.zeros((2, 5))), dict(boxes=np.zeros((3, 4))),
                                 dict(regions=np.zeros((AT.MAX_REGIONS + 1, 4)))], ids=repr)
def test_host_argument_checks(bad):
    a = AC.args(HAND[0])
    with pytest.raises(ValueError):
        AT.gaze_targets_host(**dict(a, **bad))


def test_integer_tables_must_hold_integers():
    a = AC.args(HAND[0])
    with pytest.raises(TypeError):
        AT.gaze_targets_host(**dict(a, image_of=np.zeros(2, np.float32)))
    with pytest.raises(TypeError):
        AT.gaze_targets_host(**dict(a, regions=np.zeros((1, 4)), region_image=np.zeros(1, np.float32)))
    with pytest.raises(ValueError):
        AT.gaze_targets_host(np.zeros((AT.MAX_ROWS + 1, 4)), np.zeros((AT.MAX_ROWS + 1, 3)))


def test_header_binding_and_library_agree_on_the_new_entry():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    assert 'mcg_gaze_targets' in L.EXPORTS and re.search(r'\bint mcg_gaze_targets\(', hdr) and hasattr(lib, 'mcg_gaze_targets')
    assert len(lib.mcg_gaze_targets.argtypes) == 18
    declared = re.search(r'\bint mcg_gaze_targets\(([^;]*)\);', hdr).group(1)
    assert len(declared.split(',')) == 18
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20 and '#define MCG_ABI_VERSION 20' in hdr
    assert 'attend.hip' in open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'Makefile')).read()
    for phrase in ('gaze targets', 'not tuned on data', 'Out of scope', 'REAL centre'):
        assert phrase in hdr, phrase
    from mcgaze_amd import pipeline as P
    sig = inspect.signature(P.DevicePipeline.gaze_targets)
    assert list(sig.parameters)[1:] == ['boxes', 'gaze', 'image_of', 'regions', 'region_image', 'region_period', 'expand', 'camera_angle', 'device', 'stream']


def test_the_entry_checks_its_host_arguments_before_any_launch():
    """Counts, strides, parameters and null pointers are argument errors; no device is needed to be told so."""
    import ctypes as C
    lib = L.load()
    p = C.c_void_p(256)                                           # never dereferenced: every call below fails its checks first
    ok = dict(n=1, m=0, stride=3, period=0, expand=0.25, cos2=0.5)
    call = lambda boxes=p, regions=None, **kw: (lambda a: lib.mcg_gaze_targets(None, boxes, p, a['stride'], p, a['n'], regions, regions, a['m'], a['period'],
                                                                                a['expand'], a['cos2'], p, p, p, p, p, p))(dict(ok, **kw))
    for kw in (dict(n=-1), dict(n=65537), dict(m=-1), dict(m=4097), dict(stride=2), dict(period=-1), dict(expand=-1.0), dict(expand=float('inf')),
               dict(expand=float('nan')), dict(cos2=float('nan')), dict(boxes=None), dict(m=1)):
        assert call(**kw) != L.MCG_OK, kw
        assert b'mcg_gaze_targets' in lib.mcg_last_error()
    assert call(n=0, boxes=None) == L.MCG_OK                      # n == 0 launches nothing and reads nothing


@pytest.mark.parametrize('attention', [5, 'yes', False, dict(region=[]), dict(expand=-1), dict(camera_angle=120), dict(regions=[[0, 0, 1]]),
                                       dict(regions=np.zeros((1, 4)))], ids=repr)
def test_live_gaze_checks_the_attention_option_before_anything_else(attention):
    with pytest.raises(ValueError):
        live.LiveGaze(None, None, cameras=1, slots=4, attention=attention)      # regions: a LIST of one table per camera


def test_live_gaze_regions_are_per_camera():
    with pytest.raises(ValueError):
        AT._attention_options('LiveGaze', dict(regions=[np.zeros((1, 4))]), 2)
    regions, image, opts = AT._attention_options('LiveGaze', dict(regions=[np.zeros((2, 4)), None, [[1, 2, 3, 4]]], expand=0.5), 3)
    assert regions.shape == (3, 4) and regions.dtype == np.float32 and image.tolist() == [0, 0, 2] and image.dtype == np.int32 and opts == dict(expand=0.5)
    regions, image, opts = AT._attention_options('run_head_video', True)
    assert regions.shape == (0, 4) and image.shape == (0,) and opts == {}
    assert AT._attention_options('run_head_video', None) is None


@pytest.mark.parametrize('attention', [5, False, dict(regions=[[0, 0, 1]]), dict(expand=-1), dict(slots=3), dict(regions=[[[0, 0, 1, 1]]])], ids=repr)
def test_run_head_video_checks_the_attention_option_before_anything_else(attention):
    with pytest.raises(ValueError):
        harness.run_head_video(None, None, [], boxes_per_frame=[], attention=attention)
    sig = inspect.signature(harness.run_head_video)
    assert sig.parameters['attention'].default is None and inspect.signature(live.LiveGaze).parameters['attention'].default is None


def test_the_demo_tool_takes_attention_and_regions(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location('demo_video', os.path.join(ROOT, 'tools', 'demo_video.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(SystemExit, match='--regions belongs to --attention'):
        tool.main(['-', '-', 'cfg', 'ckpt', '--out', str(tmp_path / 'o.json'), '--regions', str(tmp_path / 'r.json')])
