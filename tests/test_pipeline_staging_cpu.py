"""The host-side pieces of DevicePipeline's upload path that its entry points share: the byte layout of a staging buffer and the scope of one
device call (mcgaze_amd/staging.py), the normalisation constants the pixel kernels take, the row tables of head_crops and draw_arrows, the gaze
operand and the region tables of gaze_targets and draw_attention (mcgaze_amd/pipeline.py).  Equalities on hand-written values, no GPU: the
pieces that are pure torch given a device run on CPU tensors.  tests/test_gpu_head_crops.py drives run_many and head_crops through one staging
ring on the device."""
import contextlib
import os

import numpy as np
import pytest
import torch

from mcgaze_amd import Config
from mcgaze_amd import pipeline as P
from mcgaze_amd import staging as S

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


# ---------------------------------------------------------------- the gaze operand of draw_arrows / draw_attention (2 columns) and gaze_targets (3)
CPU = torch.device('cpu')


@pytest.mark.parametrize('columns', [2, 3])
@pytest.mark.parametrize('n', [0, 1, 2])
def test_gaze_operand_reads_packed_rows_where_they_are_and_converts_the_rest(n, columns):
    values = ROW_GAZE[:n]
    packed = torch.tensor(values, dtype=torch.float32).reshape(n, 3)
    got, stride = P._gaze_operand(packed, n, columns, CPU)
    assert got is packed and stride == 3                          # the same storage; [n,3] rows are 3 floats apart (up to one row: the width)
    wide = torch.zeros(n, 8, dtype=torch.float32)
    wide[:, :3] = packed
    view = wide[:, :3]
    got, stride = P._gaze_operand(view, n, columns, CPU)
    assert got is view and stride == (8 if n > 1 else 3)          # the wider table's stride; up to one row there is none to take: the width
    every_other = wide[:, ::2]                                    # [n,4] with a column stride of 2: not what the kernels read
    got, stride = P._gaze_operand(every_other, n, columns, CPU)
    assert got.is_contiguous() and stride == 4 and got.dtype == torch.float32 and (n == 0 or not every_other.is_contiguous())
    assert got.tolist() == [[g[0], g[2], 0.0, 0.0] for g in values]
    got, stride = P._gaze_operand(packed.double(), n, columns, CPU)
    assert got.dtype == torch.float32 and got.is_contiguous() and stride == 3 and got.tolist() == values
    host = np.array(values, np.float32).reshape(n, 3)[:, :columns].copy()
    got, stride = P._gaze_operand(host, n, columns, CPU)
    assert got is host and stride == columns                      # a host array comes back as it is


def test_gaze_operand_makes_rows_narrower_than_the_columns_contiguous():
    wide = torch.arange(12, dtype=torch.float32).reshape(2, 6)
    overlapping = wide.as_strided((2, 3), (2, 1))                 # rows 2 floats apart hold 3 columns: gaze_targets must not read them in place
    got, stride = P._gaze_operand(overlapping, 2, 3, CPU)
    assert got is not overlapping and stride == 3 and got.tolist() == [[0.0, 1.0, 2.0], [2.0, 3.0, 4.0]]
    got, stride = P._gaze_operand(overlapping, 2, 2, CPU)
    assert got is overlapping and stride == 2                     # the drawing calls read 2 columns: these rows are packed for them


# ---------------------------------------------------------------- the region tables of gaze_targets (rectangles stay [m,4]) and draw_attention
REGION_CALLERS = [('gaze_targets', False), ('draw_attention', True)]
RECTS = [[1.0, 2.0, 5.0, 6.0], [0.0, 0.0, 3.0, 4.0]]
RECT_VERTICES = [[1.0, 2.0], [5.0, 6.0], [0.0, 0.0], [3.0, 4.0]]
TRIANGLE = [[0.0, 0.0], [4.0, 0.0], [0.0, 4.0]]
REGION_IMAGE = [1, 0]


@pytest.mark.parametrize('who,as_vertices', REGION_CALLERS)
@pytest.mark.parametrize('m', [0, 1, 2])
def test_region_operands_of_host_rectangles(who, as_vertices, m):
    for region_image, want in ((None, [-1] * m), (REGION_IMAGE[:m], REGION_IMAGE[:m]), (torch.tensor(REGION_IMAGE[:m]), REGION_IMAGE[:m])):
        for regions in (np.array(RECTS[:m], np.float64).reshape(m, 4), RECTS[:m] if m else None, torch.tensor(RECTS[:m]).reshape(m, 4)):
            poly, table, start, ri, got_m, V = P._region_operands(who, regions, region_image, CPU, as_vertices)
            assert got_m == m and isinstance(table, np.ndarray) and table.dtype == np.float32 and table.flags.c_contiguous
            assert isinstance(ri, np.ndarray) and ri.dtype == np.int32 and ri.tolist() == want
            if as_vertices:                                       # the overlay: a rectangle is a 2-vertex region
                assert poly is True and V == 2 * m and table.tolist() == RECT_VERTICES[:2 * m]
                assert start.dtype == np.int32 and start.tolist() == [0, 2, 4][:m + 1]
            else:                                                 # mcg_gaze_targets reads [m,4]
                assert poly is False and V == 0 and start is None and table.shape == (m, 4) and table.tolist() == RECTS[:m]


@pytest.mark.parametrize('who,as_vertices', REGION_CALLERS)
@pytest.mark.parametrize('m', [1, 2])
def test_region_operands_of_a_host_list_with_a_triangle(who, as_vertices, m):
    mixed = [RECTS[0], TRIANGLE][2 - m:]                          # m = 1: the triangle alone; m = 2: a rectangle, then the triangle
    xy = (RECT_VERTICES[:2] + TRIANGLE)[5 - (2 * m + 1):]
    for regions in (mixed, P.region_polygons(mixed), P.PolyRegions(torch.tensor(xy), torch.tensor([0, 3] if m == 1 else [0, 2, 5]))):
        for region_image, want in ((None, [-1] * m), (REGION_IMAGE[:m], REGION_IMAGE[:m])):
            poly, table, start, ri, got_m, V = P._region_operands(who, regions, region_image, CPU, as_vertices)
            assert poly is True and got_m == m and V == len(xy)   # the vertex form for either caller: mcg_gaze_targets_poly
            assert all(isinstance(t, np.ndarray) and t.flags.c_contiguous for t in (table, start, ri))
            assert table.dtype == np.float32 and table.tolist() == xy
            assert start.dtype == np.int32 and start.tolist() == ([0, 3] if m == 1 else [0, 2, 5])
            assert ri.dtype == np.int32 and ri.tolist() == want


@pytest.mark.parametrize('who,as_vertices', REGION_CALLERS)
@pytest.mark.parametrize('m', [0, 1, 2])
def test_device_regions_is_the_same_decision_in_torch(who, as_vertices, m):
    """The branch taken when one of the tables is a device tensor, on CPU tensors."""
    for region_image, want in ((None, [-1] * m), (torch.tensor(REGION_IMAGE[:m], dtype=torch.int64), REGION_IMAGE[:m]),
                               (np.array(REGION_IMAGE[:m], np.int16), REGION_IMAGE[:m])):
        # rectangles: [m,4] for mcg_gaze_targets, the 2-vertex form with start == [0, 2, 4] for the overlay
        poly, table, start, ri = P._device_regions(who, torch.tensor(RECTS[:m], dtype=torch.float64).reshape(m, 4), region_image, CPU, as_vertices)
        assert all(isinstance(t, torch.Tensor) and t.is_contiguous() for t in (table, ri)) and table.dtype == torch.float32
        assert ri.dtype == torch.int32 and ri.tolist() == want
        if as_vertices:
            assert poly is True and table.tolist() == RECT_VERTICES[:2 * m] and start.dtype == torch.int32 and start.tolist() == [0, 2, 4][:m + 1]
        else:
            assert poly is False and start is None and tuple(table.shape) == (m, 4) and table.tolist() == RECTS[:m]
        # a PolyRegions: m regions of which the last is the triangle; a host table next to a tensor is moved with torch
        xy = (RECT_VERTICES[:2] + TRIANGLE)[5 - (2 * m + 1):] if m else []
        starts = [[0], [0, 3], [0, 2, 5]][m]
        regions = P.PolyRegions(torch.tensor(xy, dtype=torch.float64).reshape(-1, 2), np.array(starts, np.int64))
        poly, table, start, ri = P._device_regions(who, regions, region_image, CPU, as_vertices)
        assert poly is True and all(isinstance(t, torch.Tensor) and t.is_contiguous() for t in (table, start, ri))
        assert table.dtype == torch.float32 and table.tolist() == xy and start.dtype == torch.int32 and start.tolist() == starts
        assert ri.dtype == torch.int32 and ri.tolist() == want


@pytest.mark.parametrize('who,as_vertices', REGION_CALLERS)
def test_device_regions_refuse_tables_of_the_wrong_shape(who, as_vertices):
    cases = [(r'regions must be \[m, 4\] x1 y1 x2 y2, got \(2, 3\)', torch.zeros(2, 3), None),
             (r'regions must be \[m, 4\] x1 y1 x2 y2, got \(8,\)', torch.zeros(8), None),
             (r'PolyRegions is xy \[V, 2\] and start \[m \+ 1\], got \(3, 3\) and \(2,\)', P.PolyRegions(torch.zeros(3, 3), torch.tensor([0, 3])), None),
             (r'PolyRegions is xy \[V, 2\] and start \[m \+ 1\], got \(3, 2\) and \(0,\)', P.PolyRegions(torch.zeros(3, 2), torch.zeros(0, dtype=torch.int32)), None),
             (r'PolyRegions is xy \[V, 2\] and start \[m \+ 1\], got \(3, 2\) and \(1, 2\)', P.PolyRegions(torch.zeros(3, 2), torch.tensor([[0, 3]])), None),
             (r'region_image must be \[2\], one per region; got \(1,\)', torch.tensor(RECTS), torch.tensor([0])),
             (r'region_image must be \[1\], one per region; got \(2,\)', P.PolyRegions(torch.tensor(TRIANGLE), torch.tensor([0, 3])), torch.tensor([0, 1])),
             (r'region_image must be \[0\], one per region; got \(1,\)', P.PolyRegions(torch.zeros(0, 2), torch.tensor([0])), torch.tensor([0])),
             (r'region_image without regions', None, torch.tensor([0]))]
    for message, regions, region_image in cases:
        with pytest.raises(ValueError, match=who + ': ' + message):
            P._device_regions(who, regions, region_image, CPU, as_vertices)


# ---------------------------------------------------------------- the scope of one device call, on a ring, a stage and streams that only keep count
class _CountingStage:
    """A stage as far as the scope sees it: 4 KiB of host and "device" memory (both on the host here), the twin at address 0x10000."""

    def __init__(self):
        self.host, self.dev, self.base, self.sent, self.readers = np.zeros(4096, np.uint8), torch.zeros(4096, dtype=torch.uint8), 0x10000, [], []

    def send(self, nbytes):
        self.sent.append(nbytes)
        self.dev[:nbytes] = torch.from_numpy(self.host[:nbytes].copy())

    def read_by(self, main):
        self.readers.append(main)


class _CountingRing:
    def __init__(self):
        self.stage, self.taken = _CountingStage(), []

    def take(self, nbytes, dev, main):
        self.taken.append((nbytes, dev, main))
        return self.stage


@pytest.fixture
def entered(monkeypatch):
    """torch's device and stream contexts and the caller's stream replaced by ones that record: no GPU is asked for."""
    log = []

    @contextlib.contextmanager
    def context(kind, what):
        log.append((kind, what))
        try:
            yield
        finally:
            log.append(('left ' + kind, what))

    monkeypatch.setattr(torch.cuda, 'device', lambda dev: context('device', dev))
    monkeypatch.setattr(torch.cuda, 'stream', lambda stream: context('stream', stream))
    monkeypatch.setattr(torch.cuda, 'ExternalStream', lambda stream, device: ('stream of', stream, device))
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev: ('current stream of', dev))
    return log


def test_call_scope_marks_the_stage_once_after_a_body_that_uploaded(entered):
    ring, main = _CountingRing(), ('stream of', 'handle', 'gpu')
    pixels, table, there, named = np.arange(1, 4, dtype=np.uint8), np.array([7, 8], np.int32), torch.zeros(3), []
    with S._call_scope(ring, 'gpu', 'handle') as call:
        assert entered == [('device', 'gpu'), ('stream', main)] and call.dev == 'gpu' and call.main == main
        staged, at = call.upload([pixels], (table, None, there), named.append)
        # 3 bytes of pixels at 0, the 8 bytes of the table on the next multiple of 256; a device operand at its own address
        assert ring.taken == [(512, 'gpu', main)] and ring.stage.sent == [512] and named == [[0x10000]]
        assert at == [0x10100, None, there.data_ptr()] and len(staged) == 1 and staged[0].tolist() == [1, 2, 3]
        assert ring.stage.dev[256:264].tolist() == [7, 0, 0, 0, 8, 0, 0, 0]
        assert ring.stage.readers == []                           # not before the body's launches
        with pytest.raises(AssertionError, match='one upload per call'):
            call.upload([], (table,))
    assert ring.stage.readers == [main]
    assert entered[2:] == [('left stream', main), ('left device', 'gpu')]


def test_call_scope_marks_nothing_after_a_body_that_took_no_stage(entered):
    ring, there = _CountingRing(), torch.zeros(3)

    def early(n):
        with S._call_scope(ring, 'gpu') as call:
            if n == 0:
                return 'empty'                                    # before any upload
            return call.upload([], (there, None))                 # device operands only: no stage is taken

    assert early(0) == 'empty' and early(1) == ([], [there.data_ptr(), None])
    assert ring.taken == [] and ring.stage.readers == []
    assert entered == [('device', 'gpu'), ('left device', 'gpu')] * 2          # no handle: the device's current stream is the caller's, nothing to switch


def test_call_scope_marks_nothing_after_a_body_that_raised(entered):
    ring = _CountingRing()
    with pytest.raises(KeyError, match='launch failed'):
        with S._call_scope(ring, 'gpu') as call:
            call.upload([], (np.zeros(4, np.uint8),))
            raise KeyError('launch failed')
    assert ring.taken == [(256, 'gpu', ('current stream of', 'gpu'))] and ring.stage.sent == [256] and ring.stage.readers == []
    assert entered == [('device', 'gpu'), ('left device', 'gpu')]
