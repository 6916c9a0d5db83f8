"""NV12 input, host side: pipeline.nv12_to_bgr against the independent per-pixel restatement and the hand-worked known answers of
tests/nv12_cases.py, the pinned coefficient tables, the ABI registration of the two NV12 entries and their three structs, the argument
checks of head_crops(pixel_format='nv12') (which run before any device work) and the raw-file reader of tools/demo_video.py.
tests/test_gpu_nv12.py runs the device kernels against nv12_to_bgr."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from tests import nv12_cases as N
from tests.test_preprocess import NORM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRICES = ['bt601', 'bt709']
CHAIN = [dict(type='LoadImageFromFile'), dict(type='Resize', img_scale=(32, 32), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.0),
         dict(type='Normalize', **NORM), dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img'])]


@pytest.mark.parametrize('matrix', MATRICES)
def test_known_answers_worked_by_hand(matrix):
    for (Y, U, V), rgb in N.KNOWN[matrix]:
        assert N.convert_pixel(Y, U, V, matrix) == rgb, (Y, U, V)
        y, uv = np.full((2, 2), Y, np.uint8), np.array([[[U, V]]], np.uint8)
        got = P.nv12_to_bgr(y, uv, matrix)
        assert got.dtype == np.uint8 and got.shape == (2, 2, 3) and (got == np.array(rgb[::-1], np.uint8)).all(), (Y, U, V, got[0, 0].tolist())
    # the list holds what it says: black, white, Y below 16, each channel saturating where named, and a negative sum
    y_off, cy, cub, cug, cvg, cvr = N.COEF[matrix]
    raw = lambda Y, U, V: ((max(0, Y - y_off) * cy + cvr * (V - 128) + (1 << 19)) >> 20, (max(0, Y - y_off) * cy + cvg * (V - 128) + cug * (U - 128) + (1 << 19)) >> 20,
                           (max(0, Y - y_off) * cy + cub * (U - 128) + (1 << 19)) >> 20)
    assert raw(200, 128, 255)[0] > 255 and raw(200, 255, 128)[2] > 255 and raw(30, 255, 255)[1] < 0 and raw(16, 0, 128)[2] < 0
    assert all(0 < v < 255 for v in raw(128, 100, 160))


@pytest.mark.parametrize('matrix', MATRICES)
def test_nv12_to_bgr_equals_the_restatement_on_full_range_planes(matrix):
    for (y, uv), (h, w) in zip(N.FRAMES + [N.planes(5, 10, 14)], N.SHAPES + [(10, 14)]):
        want = N.convert_frame(y, uv, matrix)
        got = P.nv12_to_bgr(y, uv, matrix)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
        assert np.array_equal(P.nv12_to_bgr(y, uv.reshape(h // 2, w), matrix), want)            # the UV plane as [H/2, W] rows
    # random full-range bytes hit the clamps: every channel saturates both ways somewhere in the two larger frames, before the clamp
    y_off, cy, cub, cug, cvg, cvr = N.COEF[matrix]
    for y, uv in N.FRAMES[:2]:
        yy = np.maximum(0, y.astype(np.int64) - y_off) * cy + (1 << 19)
        u, v = (np.repeat(np.repeat(uv[..., j].astype(np.int64) - 128, 2, 0), 2, 1) for j in (0, 1))
        for name, s in (('R', yy + cvr * v), ('G', yy + cvg * v + cug * u), ('B', yy + cub * u)):
            assert ((s >> 20) > 255).any() and ((s >> 20) < 0).any(), name
    with pytest.raises(ValueError, match='matrix'):
        P.nv12_to_bgr(*N.FRAMES[0], matrix='bt2020')
    with pytest.raises(ValueError, match='even'):
        P.nv12_to_bgr(np.zeros((3, 4), np.uint8), np.zeros((1, 2, 2), np.uint8))


def test_coefficient_tables_are_pinned():
    names = ('y_off', 'cy', 'cub', 'cug', 'cvg', 'cvr')
    assert set(P.YUV_COEF) == set(MATRICES)
    for m in MATRICES:
        assert tuple(P.YUV_COEF[m][n] for n in names) == N.COEF[m] and list(P.YUV_COEF[m]) == list(names)
    assert N.COEF['bt601'] == (16, 1220542, 2116026, -409993, -852492, 1673527)                 # OpenCV's published ITUR_BT_601 set, restated
    assert N.COEF['bt709'] == (16, 1220945, 2215014, -223607, -558796, 1879825)
    # ... and the BT.709 five are round(c * 2**20) of the limited-range matrix, recomputed here in double
    kr, kb = 0.2126, 0.0722
    kg = 1.0 - kr - kb
    luma, chroma = 255.0 / 219.0, 255.0 / 224.0
    c = (luma, 2 * (1 - kb) * chroma, -(kb / kg) * 2 * (1 - kb) * chroma, -(kr / kg) * 2 * (1 - kr) * chroma, 2 * (1 - kr) * chroma)
    assert tuple(round(v * 2 ** 20) for v in c) == N.COEF['bt709'][1:]
    # the largest and smallest intermediate of either set stay inside an int
    for y_off, cy, cub, cug, cvg, cvr in N.COEF.values():
        hi = (255 - y_off) * cy + 127 * max(cub, cvr, 0) + (1 << 19)
        lo = -128 * max(cub, cvr) + min(0, 127 * (cug + cvg))
        assert hi < 2 ** 31 and lo >= -2 ** 31


def test_abi_18_registers_the_nv12_entries_and_structs():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    assert int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) == L.ABI_VERSION == 20
    lib = L.load()
    assert lib.mcg_abi_version() == 20
    for name in ('mcg_preprocess_frames_nv12', 'mcg_preprocess_head_crops_nv12'):
        assert name in L.EXPORTS and re.search(r'\bint %s\s*\(' % name, hdr) and hasattr(lib, name)
    # the ctypes structs are the header's: same fields in the same order, and the sizes a C compiler gives them (LP64: 8-byte pointers, 4-byte ints)
    for cname, ctype, size in (('mcg_yuv_coef', L.YuvCoef, 24), ('mcg_nv12_image_desc', L.Nv12ImageDesc, 32), ('mcg_nv12_frame_desc', L.Nv12FrameDesc, 64),
                               ('mcg_frame_desc', L.FrameDesc, 48), ('mcg_image_desc', L.ImageDesc, 24)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), hdr, re.S).group(1)
        fields = re.findall(r'\b(\w+)\b(?=[,;])', body)
        assert fields == [n for n, _ in ctype._fields_], cname
        assert C.sizeof(ctype) == size, cname
    # mcg_nv12_frame_desc starts with mcg_frame_desc's fields at mcg_frame_desc's offsets
    for n, _ in L.FrameDesc._fields_:
        assert getattr(L.Nv12FrameDesc, n).offset == getattr(L.FrameDesc, n).offset
    assert P._NV12_IMAGE.itemsize == 32 and P._NV12_DESC.itemsize == 64 and P._NV12_DESC_WORDS == 16
    assert P._NV12_DESC.names[P._CROP_WORD - 1:P._CROP_WORD + 3] == ('crop_y', 'crop_x', 'crop_h', 'crop_w')
    # mcg_frame_desc and mcg_image_desc keep their layout
    assert [n for n, _ in L.FrameDesc._fields_] == ['src', 'src_h', 'src_w', 'src_pitch', 'crop_y', 'crop_x', 'crop_h', 'crop_w', 'out_h', 'out_w']
    assert [n for n, _ in L.ImageDesc._fields_] == ['src', 'h', 'w', 'pitch']


def test_head_crops_nv12_checks_its_frames_before_any_device_work():
    pipe = P.DevicePipeline(CHAIN)
    box, io = np.array([[0, 0, 4, 4]], np.float32), np.zeros(1, np.int32)
    y, uv = N.FRAMES[0]
    call = lambda images, **kw: pipe.head_crops(images, box, io, device='cpu', **dict(dict(pixel_format='nv12'), **kw))
    # good frames, in each accepted form, get as far as the device check
    for images in ([(y, uv)], [(y, uv.reshape(6, 16))], [np.concatenate([y, uv.reshape(6, 16)])], [[y, uv]]):
        with pytest.raises(L.McgError, match='no CPU path'):
            call(images)
    with pytest.raises(ValueError, match='even'):                 # odd height, odd width
        call([(y[:11], uv)])
    with pytest.raises(ValueError, match='even'):
        call([(y[:, :15], uv)])
    with pytest.raises(ValueError, match=r'not \[3H/2, W\]'):       # 17 rows are no Y plane plus half as many UV rows
        call([np.zeros((17, 16), np.uint8)])
    with pytest.raises(TypeError, match='uint8'):                 # wrong dtype, either plane
        call([(y.astype(np.int32), uv)])
    with pytest.raises(TypeError, match='uint8'):
        call([(y, uv.astype(np.float32))])
    with pytest.raises(TypeError, match='rank'):                  # a packed HxWx3 frame is not an NV12 surface
        call([np.zeros((12, 16, 3), np.uint8)])
    for bad_uv in (uv[:5], uv[:, :7], uv.reshape(6, 8, 2)[:, :, :1], np.zeros((6, 16, 1), np.uint8), np.zeros((12, 16), np.uint8)):
        with pytest.raises(ValueError, match='UV plane'):         # wrong UV shape
            call([(y, bad_uv)])
    with pytest.raises(TypeError, match='both'):                  # one plane on the host, one a tensor
        call([(y, torch.from_numpy(uv))])
    with pytest.raises(TypeError, match='device planes'):         # tensors must live on the device the call names
        call([(torch.from_numpy(y), torch.from_numpy(uv))])
    with pytest.raises(TypeError, match='pair'):
        call([(y, uv, uv)])
    with pytest.raises(ValueError, match='pixel_format'):
        call([(y, uv)], pixel_format='i420')
    with pytest.raises(ValueError, match='matrix'):
        call([(y, uv)], matrix='bt2020')
    # a bad frame is reported whichever place it has
    with pytest.raises(ValueError, match='frame 1'):
        call([(y, uv), (y[:11], uv)])
    # the BGR call is as it was: its frames are HxWx3
    with pytest.raises(L.McgError, match='no CPU path'):
        pipe.head_crops([np.zeros((8, 8, 3), np.uint8)], box, io, device='cpu')


def load_demo_video():
    spec = importlib.util.spec_from_file_location('demo_video', os.path.join(ROOT, 'tools', 'demo_video.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_demo_video_reads_frame_k_of_a_raw_nv12_file(tmp_path):
    demo = load_demo_video()
    w, h = 16, 12
    frames = [N.planes(40 + t, h, w) for t in range(3)]
    path = tmp_path / 'video.nv12'
    with open(path, 'wb') as f:
        for y, uv in frames:
            f.write(y.tobytes())
            f.write(uv.tobytes())
        f.write(b'\x00' * 7)                                      # a truncated tail is no frame
    video = demo.Nv12File(str(path), w, h)
    assert len(video) == 3
    for k in (2, 0, 1):
        y, uv = video[k]
        assert y.dtype == np.uint8 and y.shape == (h, w) and uv.shape == (h // 2, w)
        assert np.array_equal(y, frames[k][0]) and np.array_equal(uv.reshape(h // 2, w // 2, 2), frames[k][1])
        assert np.array_equal(P.nv12_to_bgr(y, uv), N.convert_frame(*frames[k], 'bt601'))      # what head_crops would read from it
    with pytest.raises(IndexError):
        video[3]
    assert demo.parse_size('1920x1080') == (1920, 1080) and demo.parse_size('16X12') == (16, 12)
    with pytest.raises(ValueError):
        demo.parse_size('1920')
    with pytest.raises(ValueError, match='even'):
        demo.Nv12File(str(path), 15, 12)
