"""The detector's input, on the host (not gpu): head_detect.letterbox_geometry against answers worked by hand and against the reference's
lines restated literally (tests/letterbox_cases.py), and head_detect.letterbox_host -- the arithmetic of include/mcgaze_hip.h, "the
detector's input" -- against the composition it claims to be: oracle/preprocess_oracle.resize_linear_u8 (cv2's 8-bit INTER_LINEAR restated),
np.pad with 114, the channel reversal and torch's own uint8 -> half / float conversion on the CPU.  Every comparison is exact.  The device
kernel is compared with letterbox_host, bit for bit, in tests/test_gpu_letterbox.py.  The reference tree is not read."""
import os
import re

import numpy as np
import pytest
import torch

from mcgaze_amd import head_detect as H
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P
from oracle.preprocess_oracle import resize_linear_u8
from tests import letterbox_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def composition(frame, new_shape=640, stride=32, auto=True, scaleup=True, rgb=False):
    """One HxWx3 frame -> [3, out_h, out_w] uint8 from the oracle's resize, np.pad and the reversal; the geometry from the literal lines."""
    (unpad_w, unpad_h), _, _, (top, bottom, left, right) = LC.reference_lines(frame.shape[:2], new_shape, auto, scaleup, stride)
    img = frame if frame.shape[:2] == (unpad_h, unpad_w) else resize_linear_u8(frame, unpad_w, unpad_h)     # "if shape[::-1] != new_unpad"
    img = np.pad(img, ((top, bottom), (left, right), (0, 0)), constant_values=114)
    return np.ascontiguousarray((img if rgb else img[:, :, ::-1]).transpose(2, 0, 1))


# ---------------------------------------------------------------- 1. geometry
@pytest.mark.parametrize('hw, new_shape, opts, unpad, pads, out', LC.GEOMETRY, ids=[f'{g[0][0]}x{g[0][1]}@{g[1]}{"".join(sorted(g[2]))}' for g in LC.GEOMETRY])
def test_geometry_known_answers(hw, new_shape, opts, unpad, pads, out):
    g = H.letterbox_geometry(*hw, new_shape, **opts)
    assert (g.unpad_h, g.unpad_w) == unpad and (g.top, g.bottom, g.left, g.right) == pads and (g.out_h, g.out_w) == out
    assert P.letterbox_geometry is H.letterbox_geometry and isinstance(g, P.LetterboxGeometry)


def test_geometry_follows_the_reference_lines_over_a_sweep():
    rs = np.random.RandomState(0)
    sizes = [(int(h), int(w)) for h, w in rs.randint(1, 2200, (300, 2))] + [(1080, 1920), (1920, 1080), (640, 640), (641, 640), (1, 1), (33, 47)]
    n = 0
    for new_shape, stride in ((640, 32), (64, 32), ((384, 640), 64), (97, 5)):
        for auto in (True, False):
            for scaleup in (True, False):
                for h, w in sizes:
                    (unpad_w, unpad_h), ratio, pad, pads = LC.reference_lines((h, w), new_shape, auto, scaleup, stride)
                    if unpad_w < 1 or unpad_h < 1:              # cv2.resize refuses an empty size; so does the geometry
                        with pytest.raises(ValueError):
                            H.letterbox_geometry(h, w, new_shape, stride, auto, scaleup)
                        continue
                    g = H.letterbox_geometry(h, w, new_shape, stride, auto, scaleup)
                    assert (g.unpad_h, g.unpad_w, g.top, g.bottom, g.left, g.right) == (unpad_h, unpad_w) + pads, (h, w, new_shape, auto, scaleup)
                    assert g.ratio == ratio and g.pad == (float(pad[0]), float(pad[1]))
                    assert (g.out_h, g.out_w) == (pads[0] + unpad_h + pads[1], pads[2] + unpad_w + pads[3])
                    n += 1
    assert n > 4000
    # scaleup=False on a frame smaller than new_shape: left alone (r = 1), only padded
    g = H.letterbox_geometry(100, 200, 640, scaleup=False)
    assert g.ratio == (1.0, 1.0) and (g.unpad_h, g.unpad_w) == (100, 200) and (g.out_h, g.out_w) == (128, 224)


# ---------------------------------------------------------------- 2. pixels
@pytest.mark.parametrize('name', LC.BGR_CASES)
def test_host_bytes_equal_the_composition(name):
    frames, opts = LC.CASES[name]
    got, geoms = H.letterbox_host(frames, dtype=torch.uint8, **opts)
    want = np.stack([composition(f, **opts) for f in frames])
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert len(geoms) == len(frames) and all((g.out_h, g.out_w) == got.shape[2:] for g in geoms)


def test_the_two_facts_next_to_the_pixel_rule():
    # a frame of the unpadded size comes through the resize unchanged ...
    frames, opts = LC.CASES['no_scaleup_9x12']
    got, (g,) = H.letterbox_host(frames, dtype=np.uint8, **opts)
    assert np.array_equal(got[0, ::-1, g.top:g.top + 9, g.left:g.left + 12].transpose(1, 2, 0), frames[0])
    assert (got[0, :, :g.top] == 114).all() and (got[0, :, :, :g.left] == 114).all() and (got[0, :, g.top + 9:] == 114).all()
    # ... and an exact halving is cv2's area path, (a + b + c + d + 2) >> 2
    frames, opts = LC.CASES['halving_128x96']
    got, (g,) = H.letterbox_host(frames, dtype=np.uint8, **opts)
    f = frames[0].astype(np.int32)
    area = (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2] + 2) >> 2
    assert np.array_equal(got[0, ::-1, :, g.left:g.left + 48].transpose(1, 2, 0), area)


@pytest.mark.parametrize('name', ['all_bytes_16x16', 'wide_37x50', 'five_sizes'])
def test_float_outputs_are_torchs_conversion_of_the_bytes(name):
    frames, opts = LC.CASES[name]
    u8 = torch.from_numpy(H.letterbox_host(frames, dtype=torch.uint8, **opts)[0])
    f32, f16 = (H.letterbox_host(frames, dtype=t, **opts)[0] for t in (torch.float32, torch.float16))
    assert f32.dtype == np.float32 and f16.dtype == np.float16
    assert torch.equal(torch.from_numpy(f32), u8.float() / 255.0)
    assert torch.equal(torch.from_numpy(f16).view(torch.int16), (u8.half() / 255.0).view(torch.int16))
    assert np.array_equal(H.letterbox_host(frames, dtype=np.float16, **opts)[0].view(np.int16), f16.view(np.int16))     # numpy names work too
    if name == 'all_bytes_16x16':                                 # an identity: every byte value goes through the conversion, in every plane
        assert all(len(np.unique(u8[0, c].numpy())) == 256 for c in range(3))
        assert np.array_equal(u8[0].numpy(), LC.ALL_BYTES[:, :, ::-1].transpose(2, 0, 1))


@pytest.mark.parametrize('name', LC.NV12_CASES)
def test_nv12_equals_bgr_of_the_converted_frame(name):
    frames, opts = LC.CASES[name]
    bgr = dict(opts, pixel_format='bgr')
    for dtype in (torch.uint8, torch.float16):
        got, geoms = H.letterbox_host(frames, dtype=dtype, **opts)
        want, want_geoms = H.letterbox_host([P.nv12_to_bgr(y, uv, opts['matrix']) for y, uv in frames], dtype=dtype, **bgr)
        assert np.array_equal(got, want) and geoms == want_geoms
        # rgb= is ignored for NV12, and one [3H/2, W] surface is the same frame
        assert np.array_equal(H.letterbox_host(frames, dtype=dtype, **dict(opts, rgb=True))[0], want)
        surfaces = [np.concatenate([y, uv.reshape(y.shape[0] // 2, y.shape[1])]) for y, uv in frames]
        assert np.array_equal(H.letterbox_host(surfaces, dtype=dtype, **opts)[0], want)
    other = 'bt709' if opts['matrix'] == 'bt601' else 'bt601'
    assert not np.array_equal(H.letterbox_host(frames, dtype=torch.uint8, **dict(opts, matrix=other))[0], H.letterbox_host(frames, dtype=torch.uint8, **opts)[0])


def test_nv12_odd_sizes_are_refused():
    y, uv = LC.surface(1, 36, 50)
    for bad in ((y[:35], uv), (y[:, :49], uv), np.zeros((27, 21), np.uint8)):
        with pytest.raises(ValueError):
            H.letterbox_host([bad], 64, pixel_format='nv12')


# ---------------------------------------------------------------- 3. letterbox and detect_heads belong together
@pytest.mark.parametrize('hw, new_shape, want', [((1080, 1920), 640, ((360, 640), (12, 12, 0, 0), (384, 640))), ((48, 64), 32, ((24, 32), (4, 4, 0, 0), (32, 32)))])
def test_boxes_mapped_into_the_letterbox_come_back_from_detect_heads(hw, new_shape, want):
    """h r and w r whole, pads even: scale_coords' own (in - frame * gain) / 2 is then the true pad and the round trip is exact."""
    from tests.detect_cases import rows
    h, w = hw
    g = H.letterbox_geometry(h, w, new_shape)
    assert ((g.unpad_h, g.unpad_w), (g.top, g.bottom, g.left, g.right), (g.out_h, g.out_w)) == want
    r = g.ratio[0]
    assert h * r == g.unpad_h and w * r == g.unpad_w
    rs = np.random.RandomState(3)
    # well separated heads: one per cell of a 3 x 4 grid of the frame, integer corners
    heads = []
    for gy in range(3):
        for gx in range(4):
            x1, y1 = gx * w // 4 + int(rs.randint(0, w // 16)), gy * h // 3 + int(rs.randint(0, h // 12))
            heads.append((x1, y1, x1 + int(rs.randint(w // 16, w // 8)), y1 + int(rs.randint(h // 12, h // 6))))
    conf = np.linspace(0.95, 0.6, len(heads))                    # distinct: the order is theirs
    pred = rows([(x1 * r + g.left, y1 * r + g.top, x2 * r + g.left, y2 * r + g.top, float(c), 0, 1) for (x1, y1, x2, y2), c in zip(heads, conf)])
    boxes, _, _, _, counts, flags = H.detect_heads_host(pred, (g.out_h, g.out_w), (h, w))
    assert counts.tolist() == [len(heads)] and flags.tolist() == [0]
    assert boxes[0, :len(heads)].tolist() == [[float(v) for v in b] for b in heads]


# ---------------------------------------------------------------- 4. exports, header, arguments
def test_header_binding_and_library_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    lib = L.load()
    assert re.search(r'\bint mcg_letterbox_frames\(mcg_stream stream, const mcg_letterbox_desc\* frames_dev,', hdr)
    assert re.search(r'\bint mcg_letterbox_frames_nv12\(mcg_stream stream, const mcg_nv12_letterbox_desc\* frames_dev,', hdr)
    for name, nargs in (('mcg_letterbox_frames', 8), ('mcg_letterbox_frames_nv12', 9)):
        assert name in L.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
    assert lib.mcg_abi_version() == L.ABI_VERSION == 20 and '#define MCG_ABI_VERSION 20' in hdr
    assert re.search(r'enum \{ MCG_LETTERBOX_U8 = 0, MCG_LETTERBOX_F16 = 1, MCG_LETTERBOX_F32 = 2 \};', hdr)
    assert (L.LETTERBOX_U8, L.LETTERBOX_F16, L.LETTERBOX_F32) == (0, 1, 2)
    # the records the pipeline writes are the header's structs: a frame descriptor, then top and left
    assert P._LETTERBOX.itemsize == 56 and P._LETTERBOX.fields['top'][1] == 48 and P._NV12_LETTERBOX.itemsize == 72 and P._NV12_LETTERBOX.fields['top'][1] == 64


def test_argument_errors():
    f = LC.frame(0, 20, 30)
    for bad in (dict(new_shape=0), dict(new_shape=-64), dict(new_shape=(64, 0)), dict(new_shape=(64, 64, 3)), dict(new_shape=64.5), dict(stride=0), dict(stride=-32)):
        with pytest.raises(ValueError):
            H.letterbox_geometry(20, 30, **bad)
        with pytest.raises(ValueError):
            H.letterbox_host([f], **bad)
    for h, w in ((0, 30), (20, -1), (20.5, 30)):
        with pytest.raises(ValueError):
            H.letterbox_geometry(h, w)
    with pytest.raises(ValueError, match='would be resized to'):
        H.letterbox_geometry(1, 1000, 64)
    with pytest.raises(ValueError, match=r'one output shape.*\(32, 64\).*\(64, 64\)'):     # 21 x 64 -> 32 x 64 with auto, 37 x 50 -> 64 x 64
        H.letterbox_host([LC.frame(1, 21, 64), LC.frame(2, 37, 50)], 64)
    with pytest.raises(ValueError, match='no frames'):
        H.letterbox_host([], 64)
    for bad in (f.astype(np.float32), f[:, :, 0], f[:, :, :2], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(TypeError):
            H.letterbox_host([bad], 64)
    for bad in (torch.float64, np.int8, torch.bfloat16):
        with pytest.raises(TypeError):
            H.letterbox_host([f], 64, dtype=bad)
    with pytest.raises(ValueError):
        H.letterbox_host([f], 64, pixel_format='yuv420')
    with pytest.raises(ValueError):
        H.letterbox_host([LC.surface(0, 20, 30)], 64, pixel_format='nv12', matrix='bt2020')
