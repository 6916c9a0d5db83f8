"""Head crops, host side: the demo's window arithmetic (MCGaze_demo/demo.ipynb, cell 4) as pipeline.head_crop_window restates it, the
segmentation of cell 1 (harness.read_head_labels / segment_tracks), the arrow end points of cell 5 (harness.head_arrows) and the ABI
registration of mcg_preprocess_head_crops.  Every expected value below is worked by hand from the notebook's expressions

    cy, cx = int(y1 + y2) // 2, int(x1 + x2) // 2;   l = int(max(y2 - y1, x2 - x1) * 0.8)
    rows [max(0, cy - l), min(cy + l, h)),  columns [max(0, cx - l), min(cx + l, w))

tests/test_gpu_head_crops.py runs the same cases through the device kernel."""
import os
import re

import numpy as np
import pytest

from mcgaze_amd import Config, harness
from mcgaze_amd import lib as L
from mcgaze_amd import pipeline as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(97, 131), (120, 90)]        # (h, w) of the two frames the cases live in
# (what, frame, box x1 y1 x2 y2, window y0 x0 h w)
CASES = [
    # cy = 80 // 2 = 40, cx = 100 // 2 = 50, l = int(20 * 0.8) = 16: rows [24, 56), columns [34, 66)
    ('interior', 0, (40, 30, 60, 50), (24, 34, 32, 32)),
    # cy = 26 // 2 = 13, cx = 24 // 2 = 12, l = int(24 * 0.8) = int(19.2) = 19: rows [max(0, -6), 32), columns [max(0, -7), 31)
    ('clipped top-left', 0, (2, 1, 22, 25), (0, 0, 32, 31)),
    # cy = 176 // 2 = 88, cx = 240 // 2 = 120, l = int(20 * 0.8) = 16: rows [72, min(104, 97)), columns [104, min(136, 131))
    ('clipped bottom-right', 0, (110, 80, 130, 96), (72, 104, 25, 27)),
    # cy = 120 // 2 = 60, cx = 90 // 2 = 45, l = int(140 * 0.8) = 112: the whole 120 x 90 frame, not square
    ('larger than the frame', 1, (-20, -10, 110, 130), (0, 0, 120, 90)),
    # y1 + y2 = 17.5 -> int 17 -> // 2 = 8; x1 + x2 = 30.5 -> 30 -> 15; l = int(11.5 * 0.8) = int(9.2) = 9: rows [max(0, -1), 17), columns [6, 24)
    ('half pixels', 0, (10.5, 3, 20, 14.5), (0, 6, 17, 18)),
    # x1 + x2 = -5.5 -> int() truncates to -5 -> // 2 FLOORS to -3 (division toward zero would give -2 and 7 columns); y: 5.5 -> 5 -> 2;
    # l = int(11.5 * 0.8) = 9: rows [max(0, -7), 11), columns [max(0, -12), 6)
    ('negative centre', 0, (-7.5, -3, 2, 8.5), (0, 0, 11, 6)),
    # cy = 83 // 2 = 41, cx = 103 // 2 = 51, l = int(3 * 0.8) = int(2.4) = 2: rows [39, 43), columns [49, 53)
    ('3 x 3 box', 0, (50, 40, 53, 43), (39, 49, 4, 4)),
]
# l = int(1 * 0.8) = 0: rows [40, 40);  cx = 210, l = 16: columns [194, min(226, 131)) -- both slices are empty
EMPTY = [('no extent', 0, (50, 40, 51, 41)), ('outside the frame', 0, (200, 10, 220, 30))]


@pytest.mark.parametrize('what,frame,box,window', CASES, ids=[c[0] for c in CASES])
def test_head_crop_window_cases_worked_by_hand(what, frame, box, window):
    h, w = SHAPES[frame]
    assert P.head_crop_window(box, h, w) == window
    # ... and it is the slice the notebook takes
    cy, cx = int(box[1] + box[3]) // 2, int(box[0] + box[2]) // 2
    l = int(max(box[3] - box[1], box[2] - box[0]) * 0.8)
    crop = np.zeros((h, w))[max(0, cy - l):min(cy + l, h), max(0, cx - l):min(cx + l, w)]
    assert crop.shape == window[2:]


@pytest.mark.parametrize('what,frame,box', EMPTY, ids=[c[0] for c in EMPTY])
def test_head_crop_window_refuses_an_empty_window(what, frame, box):
    h, w = SHAPES[frame]
    with pytest.raises(ValueError, match='empty window'):
        P.head_crop_window(box, h, w)
    win, empty = P.head_crop_windows([box], h, w)           # what the device writes for it: one pixel inside the frame, marked
    assert empty.tolist() == [True] and win[0, 2:].tolist() == [1, 1] and 0 <= win[0, 0] < h and 0 <= win[0, 1] < w


def test_head_crop_windows_takes_many_boxes_and_frame_sizes():
    boxes = [c[2] for c in CASES]
    hs, ws = [SHAPES[c[1]][0] for c in CASES], [SHAPES[c[1]][1] for c in CASES]
    win, empty = P.head_crop_windows(boxes, hs, ws)
    assert win.tolist() == [list(c[3]) for c in CASES] and not empty.any()
    assert P.head_crop_window((40, 30, 60, 50), 97, 131, expand=1.0) == (20, 30, 40, 40)       # l = 20
    with pytest.raises(ValueError, match='finite'):
        P.head_crop_windows([(0, 0, float('nan'), 4)], 10, 10)


def test_head_crop_geometry_is_the_l2cs_chain():
    l2 = Config.fromfile(os.path.join(ROOT, 'configs', 'mcgaze', 'r50_clip7_l2cs.py'))
    pipe = P.DevicePipeline(l2.data.test.pipeline)
    scale_w, scale_h, pad_h, pad_w, norm = pipe.head_crop_geometry()
    assert (scale_w, scale_h, pad_h, pad_w) == (448, 448, 448, 448) and norm['to_rgb'] is True
    chain = [dict(t) for t in l2.data.test.pipeline]
    chain[1] = dict(type='Resize', img_scale=(60, 60), keep_ratio=True)
    assert P.DevicePipeline(chain).head_crop_geometry()[:4] == (60, 60, 64, 64)             # Pad(size_divisor=32)
    own = Config.fromfile(os.path.join(ROOT, 'configs', 'mcgaze', 'r50_clip7_gaze360.py'))
    with pytest.raises(NotImplementedError, match='CenterCrop'):
        P.DevicePipeline(own.data.test.pipeline).head_crops([np.zeros((8, 8, 3), np.uint8)], np.zeros((1, 4), np.float32), np.zeros(1, np.int32))
    chain[1] = dict(type='Resize', img_scale=(64, 48), keep_ratio=True)
    with pytest.raises(NotImplementedError, match='keep_ratio'):
        P.DevicePipeline(chain).head_crop_geometry()
    with pytest.raises(L.McgError, match='no CPU path'):
        pipe.head_crops([np.zeros((8, 8, 3), np.uint8)], np.zeros((1, 4), np.float32), np.zeros(1, np.int32), device='cpu')


def box(x1, n=0):
    return [x1, 10 + n, x1 + 20, 40 + n]


def test_segment_tracks_cuts_where_the_head_count_changes():
    per_frame = [[box(50), box(10)],            # label order differs from x order
                 [box(12, 1), box(52, 1)],
                 [box(30, 2)],
                 [box(31, 3)],
                 [],
                 [box(33, 5)]]
    segs = harness.segment_tracks(per_frame)
    assert [s['frame_id'] for s in segs] == [[0, 1], [2, 3], [5]]
    assert segs[0]['boxes'] == [[box(10), box(12, 1)], [box(50), box(52, 1)]]               # person 0 is the leftmost head of each frame
    assert segs[1]['boxes'] == [[box(30, 2), box(31, 3)]] and segs[2]['boxes'] == [[box(33, 5)]]
    # frames without a head: skipped at the start, in the middle and at the end, and they cut a segment even when the count is the same after
    segs = harness.segment_tracks([[], [box(5)], [], [], [box(6)], []])
    assert [s['frame_id'] for s in segs] == [[1], [4]]
    assert harness.segment_tracks([]) == [] and harness.segment_tracks([[], []]) == []
    # equal x1: the label order stays (sorted() is stable)
    a, b = [7, 1, 9, 3], [7, 0, 8, 2]
    assert harness.segment_tracks([[a, b]])[0]['boxes'] == [[a], [b]]


def test_read_head_labels(tmp_path):
    path = tmp_path / '3.txt'
    path.write_text('0 100 50 160 120\n1 412 80.5 470 151\n\n1 12.25 9 60 70.75\n0 1 2 3 4\n')
    boxes = harness.read_head_labels(str(path))
    assert boxes == [[412, 80.5, 470, 151], [12.25, 9, 60, 70.75]]
    assert [type(v) for v in boxes[0]] == [int, float, int, int]                             # what the notebook's eval gives
    assert harness.read_head_labels(str(path), head_class=0) == [[100, 50, 160, 120], [1, 2, 3, 4]]
    (tmp_path / 'bad.txt').write_text('1 2 3\n')
    with pytest.raises(ValueError, match='class x1 y1 x2 y2'):
        harness.read_head_labels(str(tmp_path / 'bad.txt'))
    (tmp_path / 'code.txt').write_text('1 __import__("os").getcwd() 2 3 4\n')                # nothing is evaluated
    with pytest.raises(ValueError):
        harness.read_head_labels(str(tmp_path / 'code.txt'))


def test_arrow_end_points_worked_by_hand():
    # cx = 100 // 2 = 50, cy = 80 // 2 = 40, l = int(max(20, 20) * 1) = 20: tip (int(50 - 10), int(40 + 5))
    # cx = 24 // 2 = 12, cy = 26 // 2 = 13, l = 24: 12 - 24 * 0.6 = -2.4 -> int() gives -2 (floor: -3); 13 - 24 * 0.7 = -3.8 -> -3
    arrows = harness.head_arrows([(40, 30, 60, 50), (2, 1, 22, 25)], np.array([[0.5, -0.25, 0.1], [0.6, 0.7, 0.2]], dtype=np.float32))
    assert arrows.dtype == np.int64 and arrows.tolist() == [[[50, 40], [40, 45]], [[12, 13], [-2, -3]]]


def test_abi_18_registers_the_head_crop_entry():
    hdr = open(os.path.join(ROOT, 'include', 'mcgaze_hip.h')).read()
    assert int(re.search(r'#define MCG_ABI_VERSION (\d+)', hdr).group(1)) == L.ABI_VERSION == 20
    assert 'mcg_preprocess_head_crops' in L.EXPORTS and re.search(r'\bint mcg_preprocess_head_crops\s*\(', hdr)
    lib = L.load()
    assert lib.mcg_abi_version() == 20 and hasattr(lib, 'mcg_preprocess_head_crops')
    # the ctypes and numpy records are the header's struct: pointer, three ints
    fields = re.search(r'typedef struct mcg_image_desc \{(.*?)\} mcg_image_desc;', hdr, re.S).group(1)
    assert re.findall(r'\b(src|h|w|pitch)\b(?=[,;])', fields) == [n for n, _ in L.ImageDesc._fields_]
    assert P._IMAGE.itemsize == 24 and P._DESC.itemsize % 4 == 0 and P._DESC.names[P._CROP_WORD - 1:P._CROP_WORD + 3] == ('crop_y', 'crop_x', 'crop_h', 'crop_w')
