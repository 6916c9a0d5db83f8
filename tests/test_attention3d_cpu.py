"""Gaze targets in 3-D without a GPU (include/mcgaze_hip.h, "gaze targets, 3-D"): attention.gaze_targets_3d_host against scenes whose
tables are written out by hand and against a second, scalar statement of the arithmetic (tests/attention3d_cases.py); the two scenes that
show the behaviour is NEW -- depth orders two heads on one image ray where gaze_targets_host takes the nearer in pixels, a look at a screen
lands inside it where gaze_targets_host stops at its rim --; the helpers, the boundary (export, header, ABI) and the argument checks of
the layers above."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from mcgaze_amd import lib as L
from tests import attention3d_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = TC.all_cases()
HAND = TC.hand_cases() + [TC.unusable_regions_case()] + TC.cone_cases()
by_name = lambda name: next(c for c in CASES if c['name'] == name)


@pytest.mark.parametrize('case', HAND, ids=[c['name'] for c in HAND])
def test_hand_worked_scenes(case):
    got = AT.gaze_targets_3d_host(**TC.args(case))
    assert [a.dtype for a in got] == [np.int32, np.int32, np.float32, np.float32, np.int32, np.int32, np.float32]
    n = len(case['boxes'])
    assert [a.shape for a in got] == [(n,), (n,), (n,), (n, 2), (n,), (n,), (n, 3)]
    TC.check_expect(got, case)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_numpy_twin_equals_the_scalar_restatement(case):
    TC.same_tables(AT.gaze_targets_3d_host(**TC.args(case)), TC.as_tables(TC.targets_scalar(**TC.args(case))), case['name'])


@pytest.mark.parametrize('frame', ['eye', 'camera'])
def test_200_seeded_random_rows_bit_for_bit(frame):
    case = TC.random_case(100 + len(frame), 200, 6, 14, cameras=3, period=3, frame=frame, garbage=2)
    a = TC.args(case)
    got = AT.gaze_targets_3d_host(**a)
    TC.same_tables(got, TC.as_tables(TC.targets_scalar(**a)), case['name'])
    seen = np.bincount(got[0], minlength=4)                       # every kind and unusable rows occur, or the tables would check nothing
    assert (seen > 0).all() and (got[5] == 2).any() and (got[5] == 0).any(), seen.tolist()


def test_depth_orders_two_heads_on_one_image_ray_where_the_image_plane_cannot():
    """N (2 m) and F (6 m) are centred on one pixel.  The viewer's 2-D ray meets N's larger box first whatever gz says; in 3-D gz decides."""
    far, near = by_name('depth ordering: gz away from the lens picks the FAR head'), by_name('depth ordering: gz flipped picks the NEAR head')
    for c in (far, near):
        flat = AT.gaze_targets_host(c['boxes'], c['gaze'], c['image_of'])
        assert (flat[0][0], flat[1][0]) == (AT.KIND_HEAD, 1), 'the image plane: always the head that is nearer in pixels'
    assert AT.gaze_targets_3d_host(**TC.args(far))[1][0] == 2 and AT.gaze_targets_3d_host(**TC.args(near))[1][0] == 1
    assert far['gaze'][0, 2] == -near['gaze'][0, 2] and (far['gaze'][0, :2] == near['gaze'][0, :2]).all()


def test_a_look_at_a_screen_lands_inside_it_and_heats_an_interior_cell():
    c = by_name('a look at a screen lands INSIDE it')
    kind, target, t, hit, mutual, flags, hit3d = AT.gaze_targets_3d_host(**TC.args(c))
    px = np.asarray(TC.SCREEN_PX)
    assert kind[0] == AT.KIND_REGION and px[:, 0].min() < hit[0, 0] < px[:, 0].max() and px[:, 1].min() < hit[0, 1] < px[:, 1].max()
    assert hit[0].tolist() == [np.float32(512 * (1 / 3) + 320), 240.0]
    flat = AT.gaze_targets_host(c['boxes'], c['gaze'], c['image_of'], regions=[TC.SCREEN_PX])
    assert flat[0][0] == AT.KIND_REGION and abs(flat[3][0, 0] - px[:, 0].min()) < 1e-3, 'the image plane: the rim of the polygon'
    heat, peak = AT.gaze_heat_host(hit, kind, c['image_of'], np.zeros((1, 60, 80), np.int32), flags=flags, cell_shift=3, radius=0)
    cell = (int(round(float(hit[0, 1]))) >> 3, int(round(float(hit[0, 0]))) >> 3)
    assert heat[0][cell] == 1 == peak[0] and heat.sum() == 1
    rim = np.ceil(px.min(axis=0) / 8), np.floor(px.max(axis=0) / 8) - 1
    assert rim[0][0] < cell[1] < rim[1][0] and rim[0][1] < cell[0] < rim[1][1], 'a cell strictly inside the screen'
    miss = by_name('a look passing in front of the screen misses it')
    flat = AT.gaze_targets_host(miss['boxes'], miss['gaze'], miss['image_of'], regions=[TC.SCREEN_PX])
    assert flat[0][0] == AT.KIND_REGION and AT.gaze_targets_3d_host(**TC.args(miss))[0][0] == AT.KIND_NONE


def test_eye_and_camera_frames_agree_on_the_optical_axis():
    eye, cam = (AT.gaze_targets_3d_host(**TC.args(c)) for c in TC.frame_pair())
    assert eye[0][0] in (AT.KIND_HEAD, AT.KIND_REGION)
    for name in ('kind', 'target', 'hit', 'hit3d'):
        k = TC.FIELDS.index(name)
        assert (eye[k][0].view(np.int32) == cam[k][0].view(np.int32)).all(), name
    assert eye[2][0] * 4 == cam[2][0]                             # D is Z * Z = 4 times as long


def test_a_nan_hit_is_skipped_by_the_heat_map():
    c = by_name('a hit behind the lens: Pz <= 0 gives a NaN hit')
    kind, _, _, hit, _, flags, _ = AT.gaze_targets_3d_host(**TC.args(c))
    assert hit.view(np.uint32).tolist() == [[0x7fc00000, 0x7fc00000]]
    heat, _ = AT.gaze_heat_host(hit, kind, c['image_of'], np.zeros((1, 60, 80), np.int32), flags=flags)
    assert heat.sum() == 0


def test_helpers_regions_3d_and_unproject():
    r = AT.regions_3d([TC.SCREEN, [[0, 0, 1], [1, 0, 1], [0, 1, 1]]])
    assert isinstance(r, AT.PolyRegions3D) and r.xyz.shape == (7, 3) and r.xyz.dtype == np.float32 and r.start.tolist() == [0, 4, 7] and r.start.dtype == np.int32
    empty = AT.regions_3d([])
    assert empty.xyz.shape == (0, 3) and empty.start.tolist() == [0]
    for bad in ([[[0, 0, 1], [1, 0, 1]]], [[[0, 0], [1, 0], [0, 1]]], [[[0, 0, 1]] * 33], [[[0, 0, 1], [1, 0, 1], [0, 1]]]):
        with pytest.raises(ValueError):
            AT.regions_3d(bad)
    for bad in (5, [5], [[['a', 0, 1]] * 3]):
        with pytest.raises(TypeError):
            AT.regions_3d(bad)
    # the corners of the screen as marked in the picture, lifted back with their distance
    back = AT.unproject(TC.SCREEN_PX, 3.0, TC.CAM)
    assert back.shape == (4, 3) and np.abs(back - np.asarray(TC.SCREEN)).max() < 1e-12
    assert AT.unproject([320.0, 240.0], 2.0, TC.CAM).tolist() == [0.0, 0.0, 2.0]
    assert AT.unproject([[576.0, 240.0]], [4.0], TC.CAM).tolist() == [[2.0, 0.0, 4.0]]
    with pytest.raises(ValueError):
        AT.unproject([1.0, 2.0, 3.0], 1.0, TC.CAM)
    # the origin rule itself: a marked point at the head's depth is where the head's row is lifted to
    c = by_name('depth None: every row from its head size')
    got = AT.gaze_targets_3d_host(**TC.args(c))
    assert got[6][0].tolist() == [1.0, 0.0, 10.0] and AT.unproject([576.0, 240.0], 2.0, TC.CAM).tolist() == [1.0, 0.0, 2.0]


def test_defaults_are_the_documented_conventions():
    assert (AT.HEAD_SIZE, AT.GAZE_FRAMES, AT.MAX_CAMERAS) == (0.24, ('camera', 'eye'), 4096) and AT.FIELDS_3D == TC.FIELDS
    sig = inspect.signature(AT.gaze_targets_3d_host)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[4:]] == [
        ('depth', None), ('regions', None), ('region_image', None), ('region_period', 0), ('cam_period', 0), ('head_size', 0.24), ('frame', 'eye'),
        ('expand', 0.25), ('camera_angle', 10.0)]
    from mcgaze_amd import pipeline as P
    sig = inspect.signature(P.DevicePipeline.gaze_targets_3d)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ('boxes', inspect.Parameter.empty), ('gaze', inspect.Parameter.empty), ('image_of', inspect.Parameter.empty), ('cam', inspect.Parameter.empty),
        ('depth', None), ('regions', None), ('region_image', None), ('region_period', 0), ('cam_period', 0), ('head_size', 0.24), ('frame', 'eye'),
        ('expand', 0.25), ('camera_angle', 10.0), ('device', 'cuda:0'), ('stream', None)]


def test_torch_tables_and_other_dtypes_are_read():
    import torch
    a = TC.args(CASES[0])
    want = AT.gaze_targets_3d_host(**a)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    TC.same_tables(AT.gaze_targets_3d_host(t(a['boxes']), t(a['gaze']), t(a['image_of']), t(a['cam']), depth=t(a['depth']), frame='camera'), want, 'torch')
    TC.same_tables(AT.gaze_targets_3d_host(a['boxes'].astype(np.float64), a['gaze'].tolist(), a['image_of'].astype(np.int64), list(TC.CAM),
                                           depth=a['depth'].tolist(), frame='camera'), want, 'other dtypes, one camera as four numbers')


@pytest.mark.parametrize('bad', [dict(head_size=0), dict(head_size=-1.0), dict(head_size=float('nan')), dict(head_size=float('inf')), dict(head_size='1'),
                                 dict(frame='world'), dict(frame=1), dict(cam_period=-1), dict(cam_period=1.5), dict(cam=[1, 2, 3]), dict(cam=np.zeros((0, 4))),
                                 dict(cam=np.zeros((2, 5))), dict(cam=np.zeros((AT.MAX_CAMERAS + 1, 4))), dict(depth=[1.0]), dict(expand=-0.1),
                                 dict(camera_angle=91), dict(region_period=-1), dict(region_image=[0]), dict(regions=[TC.SCREEN], region_image=[0, 1]),
                                 dict(regions=AT.PolyRegions3D(np.zeros((4, 2)), np.zeros(2, np.int32))),
                                 dict(regions=AT.PolyRegions3D(np.zeros((4, 3)), np.zeros(0, np.int32))), dict(regions=[TC.SCREEN[:2]]),
                                 dict(regions=AT.PolyRegions3D(np.zeros((AT.MAX_VERTICES + 1, 3)), np.zeros(2, np.int32))),
                                 dict(regions=AT.PolyRegions3D(np.zeros((4, 3)), np.zeros(AT.MAX_REGIONS + 2, np.int32))), dict(image_of=[0]),
                                 dict(gaze=np.zeros((3, 2))), dict(boxes=np.zeros((3, 5)))], ids=repr)
def test_host_argument_checks(bad):
    a = TC.args(CASES[0])
    with pytest.raises(ValueError):
        AT.gaze_targets_3d_host(**dict(a, **bad))


def test_tables_must_hold_numbers():
    a = TC.args(CASES[0])
    for bad in (dict(image_of=np.zeros(3, np.float32)), dict(cam=np.array(['a', 'b', 'c', 'd'])), dict(depth=np.array(['a', 'b', 'c'])),
                dict(regions=[TC.SCREEN], region_image=np.zeros(1, np.float32)), dict(regions=AT.PolyRegions3D(np.zeros((4, 3)), np.zeros(2, np.float32)))):
        with pytest.raises(TypeError):
            AT.gaze_targets_3d_host(**dict(a, **bad))


def test_header_binding_and_library_agree_on_the_new_entry():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    assert 'mcg_gaze_targets_3d' in L.EXPORTS and hasattr(lib, 'mcg_gaze_targets_3d')
    declared = re.search(r'\bint mcg_gaze_targets_3d\(([^;]*)\);', hdr).group(1)
    assert len(declared.split(',')) == len(lib.mcg_gaze_targets_3d.argtypes) == 27
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20 and '#define MCG_ABI_VERSION 20' in hdr
    section = hdr[hdr.index('gaze targets, 3-D (additions to ABI 20; nothing above changes)'):hdr.index('measurement aids (bench.py)')]
    for phrase in ('not tuned on data', 'Out of scope', 'lens distortion', 'one-sided', 'sqrtf', 'uncontracted', '0x7fc00000', 'hit3d'):
        assert phrase in section, phrase
    assert 'sqrt(' not in section.replace('sqrtf(', '')           # no double square root
    rules = open(os.path.join(ROOT, 'mcgaze_amd', 'csrc', 'check_resources.py')).read()
    assert re.search(r"'gaze_targets_3d_kernel': dict\(scratch=0, vgpr_spill=0, unit='attend'\)", rules)


def test_the_entry_checks_its_host_arguments_before_any_launch():
    """Counts, strides, parameters and null pointers are argument errors; no device is needed to be told so."""
    lib = L.load()
    p = C.c_void_p(256)                                           # never dereferenced: every call below fails its checks first
    ok = dict(n=1, m=0, V=0, cams=1, stride=3, period=0, cam_period=0, expand=0.25, cos2=0.5, head=0.24, frame=1, boxes=p, cam=p, xyz=None, start=None,
              hit3d=p, depth=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mcg_gaze_targets_3d(None, a['boxes'], p, a['stride'], p, a['n'], a['cam'], a['cams'], a['cam_period'], a['depth'], a['head'], a['frame'],
                                       a['xyz'], a['V'], a['start'], a['start'], a['m'], a['period'], a['expand'], a['cos2'], p, p, p, p, p, p, a['hit3d'])

    for kw in (dict(n=-1), dict(n=65537), dict(m=-1), dict(m=4097), dict(V=-1), dict(V=65537), dict(cams=0), dict(cams=4097), dict(stride=2),
               dict(period=-1), dict(cam_period=-1), dict(expand=-1.0), dict(expand=float('inf')), dict(expand=float('nan')), dict(cos2=float('nan')),
               dict(head=0.0), dict(head=-1.0), dict(head=float('inf')), dict(head=float('nan')), dict(frame=2), dict(frame=-1), dict(boxes=None),
               dict(cam=None), dict(hit3d=None), dict(m=1), dict(V=3), dict(m=1, V=3, xyz=p)):
        assert call(**kw) != L.MCG_OK, kw
        assert b'mcg_gaze_targets_3d' in lib.mcg_last_error()
    assert call(n=0, boxes=None, hit3d=None) == L.MCG_OK          # n == 0 launches nothing and reads nothing


TRIANGLE = [[0, 0, 1], [1, 0, 1], [0, 1, 1]]


def test_the_attention_option_carries_the_3d_tables():
    regions, image, opts = AT._attention_options('LiveGaze', dict(camera=[500, 500, 64, 48], regions3d=[[TRIANGLE, TC.SCREEN], None], head_size=0.2,
                                                                  frame='camera', expand=0.5, regions=[np.zeros((1, 4)), None]), 2)
    three_d = opts.pop('three_d')
    assert regions.shape == (1, 4) and image.tolist() == [0] and opts == dict(expand=0.5)          # the 2-D part is what it was
    assert three_d['cam'].tolist() == [[500, 500, 64, 48]] * 2 and three_d['cam'].dtype == np.float32
    assert isinstance(three_d['regions'], AT.PolyRegions3D) and three_d['regions'].start.tolist() == [0, 3, 7] and three_d['region_image'].tolist() == [0, 0]
    assert (three_d['head_size'], three_d['frame']) == (0.2, 'camera')
    _, image, opts = AT._attention_options('run_head_video', dict(camera=[500, 500, 64, 48], regions3d=[TRIANGLE]))
    assert opts['three_d']['cam'].shape == (1, 4) and opts['three_d']['region_image'].tolist() == [-1] and image.shape == (0,)
    assert (opts['three_d']['head_size'], opts['three_d']['frame']) == (0.24, 'eye')
    per_camera = AT._attention_options('LiveGaze', dict(camera=[[500, 500, 64, 48], [400, 400, 60, 40]]), 2)[2]['three_d']
    assert per_camera['cam'][1].tolist() == [400, 400, 60, 40] and len(per_camera['region_image']) == 0
    # without camera: byte for byte today's
    assert AT._attention_options('LiveGaze', dict(expand=0.5), 2)[2] == dict(expand=0.5)
    assert AT._attention_options('run_head_video', True)[2] == {}


@pytest.mark.parametrize('attention', [dict(regions3d=[[TRIANGLE], None]), dict(head_size=0.3), dict(frame='eye'), dict(camera=[1, 2, 3]),
                                       dict(camera=[500, 500, 64, 48], frame='world'), dict(camera=[500, 500, 64, 48], head_size=0),
                                       dict(camera=np.zeros((3, 4))), dict(camera=[500, 500, 64, 48], regions3d=[[TRIANGLE]]),
                                       dict(camera=[500, 500, 64, 48], regions3d=[[TRIANGLE[:2]], None]), dict(camera=[500, 500, 64, 48], regions3d=[5, None]),
                                       dict(camera='wide')], ids=repr)
def test_live_gaze_checks_the_3d_keys_before_anything_else(attention):
    with pytest.raises(ValueError):
        live.LiveGaze(None, None, cameras=2, slots=4, attention=attention)


@pytest.mark.parametrize('attention', [dict(regions3d=[TRIANGLE]), dict(camera=[1, 2, 3]), dict(camera=[[1, 2, 3, 4]] * 2),
                                       dict(camera=[500, 500, 64, 48], regions3d=[[[0, 0], [1, 0], [0, 1]]]), dict(camera=[500, 500, 64, 48], frame=0)], ids=repr)
def test_run_head_video_checks_the_3d_keys_before_anything_else(attention):
    with pytest.raises(ValueError):
        harness.run_head_video(None, None, [], boxes_per_frame=[], attention=attention)


def test_the_demo_tool_takes_the_camera(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location('demo_video', os.path.join(ROOT, 'tools', 'demo_video.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ['-', '-', 'cfg', 'ckpt', '--out', str(tmp_path / 'o.json')]
    with pytest.raises(SystemExit, match='--camera belongs to --attention'):
        tool.main(base + ['--camera', '500,500,64,48'])
    with pytest.raises(SystemExit, match='belong to --camera'):
        tool.main(base + ['--attention', '--regions3d', str(tmp_path / 'r.json')])
    with pytest.raises(SystemExit, match='belong to --camera'):
        tool.main(base + ['--attention', '--gaze-frame', 'camera'])
    with pytest.raises(SystemExit, match='--camera takes FX,FY,CX,CY'):
        tool.main(base + ['--attention', '--camera', '500,500,64'])


def test_the_documents_describe_the_feature_and_its_limits():
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    section = doc[doc.index('### Targets in 3-D'):]
    section = section[:section.index('\n### ', 10)]
    for phrase in ('gaze_targets_3d', 'head_size', "frame='eye'", 'not tuned on data', 'lens distortion', 'four image corners', 'one-sided', 'hit3d', 'unproject'):
        assert phrase in section, phrase
    assert 'camera intrinsics or depth' not in doc
    assert 'gaze_targets_3d' in open(os.path.join(ROOT, 'README.md')).read()
    assert os.path.exists(os.path.join(ROOT, 'tools', 'attention3d_bench.py'))
