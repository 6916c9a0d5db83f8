"""The host-side pieces of DevicePipeline's upload path that run_many and head_crops share (mcgaze_amd/pipeline.py): the byte layout of
a staging buffer and the normalisation constants the pixel kernels take.  Equalities, no GPU.  tests/test_gpu_head_crops.py drives both entry
points through one staging ring on the device."""
import os

import numpy as np
import pytest

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
