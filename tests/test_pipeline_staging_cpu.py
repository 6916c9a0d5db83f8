"""The host-side pieces of DevicePipeline's upload path that its entry points share: the byte layout of a staging buffer
(mcgaze_amd/staging.py), the normalisation constants the pixel kernels take and the row tables of head_crops and draw_arrows
(mcgaze_amd/pipeline.py).  Equalities, no GPU.  tests/test_gpu_head_crops.py drives run_many and head_crops through one staging ring on the
device."""
import os

import numpy as np
import pytest
import torch

from mcgaze_amd import Config
from mcgaze_amd import pipeline as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ['r50_clip7_gaze360.py', 'r50_clip7_l2cs.py']


def test_layout_puts_every_part_on_a_multiple_of_256_and_none_on_another():
    sizes = [0, 1, 255, 256, 257]
    offs, total = P._layout(sizes)
    rounded = [0, 256, 256, 256, 512]                             # each size up to the next multiple of 256, by hand
    assert len(offs) == len(sizes) and all(isinstance(o, int) and o % 256 == 0 for o in offs)
    for k in range(len(sizes)):
        for j in range(k + 1, len(sizes)):                        # parts are in order and no two share a byte
            assert offs[k] + sizes[k] <= offs[j]
    assert offs == [0, 0, 256, 512, 768] and total == offs[-1] + rounded[-1] == 1280
    assert P._layout([]) == ([], 0) and P._layout([300]) == ([0], 512)
    assert P._layout(sizes[::-1]) == ([0, 512, 768, 1024, 1280], 1280)


@pytest.mark.parametrize('name', CONFIGS)
def test_kernel_norm_is_the_literal_arithmetic_on_the_configs_norm(name):
    pipe = P.DevicePipeline(Config.fromfile(os.path.join(ROOT, 'configs', 'mcgaze', name)).data.test.pipeline)
    norm = pipe.plan((8, 8, 3), np.random.RandomState(0)).img_norm_cfg
    assert norm['mean'].dtype == norm['std'].dtype == np.float32 and len(norm['mean']) == len(norm['std']) == 3
    mean, stdinv, swap = P._kernel_norm(norm, False)
    for k in range(3):
        assert np.float32(mean[k]).view(np.int32) == np.float32(norm['mean'][k]).view(np.int32)
        assert np.float32(stdinv[k]).view(np.int32) == np.float32(1 / np.float64(norm['std'][k])).view(np.int32)
    assert len(mean) == len(stdinv) == 3 and swap == int(bool(norm['to_rgb']))


@pytest.mark.parametrize('to_rgb', [True, False])
def test_kernel_norm_swaps_when_the_wanted_order_differs_from_the_sources(to_rgb):
    norm = dict(mean=np.zeros(3, np.float32), std=np.ones(3, np.float32), to_rgb=to_rgb)
    swap = lambda *a, **kw: P._kernel_norm(norm, *a, **kw)[2]
    assert swap(False) == int(to_rgb)                             # BGR frames: swapped for an RGB model
    assert swap(True) == int(not to_rgb)                          # RGB frames: swapped for a BGR model
    assert swap(False, nv12=True) == swap(True, nv12=True) == int(to_rgb)     # converted NV12 taps are BGR whatever rgb= says
    assert all(type(swap(r, nv12=n)) is int for r in (False, True) for n in (False, True))


# ---------------------------------------------------------------- the row tables of head_crops and draw_arrows: three frames, n <= 4 rows
CALLERS = [('head_crops', 'crops'), ('draw_arrows', 'arrows')]
FRAMES = 3
ROW_BOXES = [[1, 2, 3, 4], [0.5, 0, 8, 9.25], [2, 2, 2, 2]]
ROW_IMAGE_OF = [0, 2, 1]
ROW_GAZE = [[0.5, -0.25, 9.0], [0.0, 1.0, 9.0], [-1.5, 0.125, 9.0]]


@pytest.mark.parametrize('caller,rows', CALLERS)
def test_row_tables_come_back_in_the_types_the_device_reads(caller, rows):
    for image_of in (ROW_IMAGE_OF, np.array(ROW_IMAGE_OF, np.int64), np.array(ROW_IMAGE_OF, np.uint8), torch.tensor(ROW_IMAGE_OF)):
        boxes, index, gaze, n = P._row_tables(caller, rows, FRAMES, np.array(ROW_BOXES, np.float64), image_of)
        assert n == 3 and gaze is None
        assert boxes.dtype == np.float32 and boxes.shape == (3, 4) and boxes.flags.c_contiguous and boxes.tolist() == ROW_BOXES
        assert index.dtype == np.int32 and index.shape == (3,) and index.tolist() == ROW_IMAGE_OF
    # a [n,3] gaze (a stream's fused gaze) is cut to the two columns that are read; a flat list of 4 n numbers is n boxes
    boxes, index, gaze, n = P._row_tables(caller, rows, FRAMES, sum(ROW_BOXES, []), ROW_IMAGE_OF, torch.tensor(ROW_GAZE, dtype=torch.float64))
    assert n == 3 and boxes.shape == (3, 4) and boxes.tolist() == ROW_BOXES
    assert gaze.dtype == np.float32 and gaze.shape == (3, 2) and gaze.flags.c_contiguous and gaze.tolist() == [g[:2] for g in ROW_GAZE]
    # no rows: an empty gaze of any shape is accepted with n == 0
    for empty in ([], np.zeros((0, 3)), np.zeros(0, np.float32)):
        boxes, index, gaze, n = P._row_tables(caller, rows, FRAMES, np.zeros((0, 4)), np.zeros(0, np.int64), empty)
        assert n == 0 and boxes.shape == (0, 4) and index.shape == (0,) and index.dtype == np.int32 and gaze.shape == (0, 2) and gaze.dtype == np.float32


@pytest.mark.parametrize('caller,rows', CALLERS)
def test_row_tables_refuse_what_the_device_must_not_read(caller, rows):
    with pytest.raises(TypeError, match='image_of must hold integers'):
        P._row_tables(caller, rows, FRAMES, ROW_BOXES, [0.0, 2.0, 1.0])
    for bad, got in ((-1, r'\[-1, 2\]'), (FRAMES, r'\[0, 3\]')):
        with pytest.raises(ValueError, match=r'image_of must lie in \[0, 3\), got ' + got):
            P._row_tables(caller, rows, FRAMES, ROW_BOXES, [0, 2, bad])
    with pytest.raises(ValueError, match=caller + r': boxes \(3, 4\) and image_of \(2,\) must be \[n,4\] and \[n\]'):
        P._row_tables(caller, rows, FRAMES, ROW_BOXES, ROW_IMAGE_OF[:2])
    for gaze, shape in ((ROW_GAZE[:2], r'\(2, 2\)'), ([[0.5], [0.5], [0.5]], r'\(3, 1\)'), ([0.5, 0.5, 0.5], r'\(3,\)')):
        with pytest.raises(ValueError, match=caller + r': boxes \(3, 4\), gaze ' + shape + r' and image_of \(3,\) must be \[n,4\], \[n,>=2\] and \[n\]'):
            P._row_tables(caller, rows, FRAMES, ROW_BOXES, ROW_IMAGE_OF, gaze)


@pytest.mark.parametrize('caller,rows', CALLERS)
def test_row_tables_hold_at_most_65535_rows(caller, rows):
    boxes, image_of, gaze = np.zeros((65536, 4), np.float32), np.zeros(65536, np.int32), np.zeros((65536, 2), np.float32)
    with pytest.raises(ValueError, match=f'{caller}: at most 65535 {rows} per call \\(got 65536\\)'):
        P._row_tables(caller, rows, FRAMES, boxes, image_of, gaze)
    assert P._row_tables(caller, rows, FRAMES, boxes[:65535], image_of[:65535], gaze[:65535])[3] == 65535
    assert P._row_tables(caller, rows, FRAMES, boxes[:65535], image_of[:65535])[3] == 65535
