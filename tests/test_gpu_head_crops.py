"""-m gpu: head crops on the device -- DevicePipeline.head_crops (mcg_preprocess_head_crops: head_crop_plan_kernel + the pixel kernel) and
harness.run_head_video on top of it.

Everything is asserted BIT FOR BIT: the window is integer arithmetic worked by hand (tests/test_head_crops_cpu.py::CASES) or taken with
the notebook's own python expressions (demo_window below), the pixels are oracle.preprocess_oracle.test_pipeline on the numpy slice the
demo takes (MCGaze_demo/demo.ipynb, cell 4), zero-padded to the call's padded size, and the end-to-end records are harness.run_tracks on
those oracle-made crops.  No tolerance anywhere.  The flag test makes valid calls with defined results (an empty window, a NaN box and an
image index one past the table are inputs the entry documents); nothing here provokes a fault."""
import numpy as np
import pytest
import torch

from mcgaze_amd import harness, synth
from mcgaze_amd import pipeline as P
from oracle import preprocess_oracle as po
from tests.test_head_crops_cpu import CASES, SHAPES
from tests.test_preprocess import NORM, pattern

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FRAMES = [pattern(s + (3,)) for s in SHAPES]                 # 97 x 131 and 120 x 90
BOXES = np.array([c[2] for c in CASES], dtype=np.float32)
IMAGE_OF = np.array([c[1] for c in CASES], dtype=np.int32)
# other valid boxes for the same frames (graph replay): interior, clipped, larger than the frame, half pixels, negative centre, small
BOXES2 = np.array([(30, 20, 70, 66), (5, 5, 40, 30), (60, 50, 125, 90), (10, 10, 80, 100), (20.5, 13, 44, 30.5), (-3.5, -3, 12, 18.5),
                   (80, 60, 90, 70)], dtype=np.float32)


def chain(scale, to_rgb=True):
    return [dict(type='LoadImageFromFile'), dict(type='Resize', img_scale=(scale, scale), keep_ratio=True), dict(type='RandomFlip', flip_ratio=0.0),
            dict(type='Normalize', **dict(NORM, to_rgb=to_rgb)), dict(type='Pad', size_divisor=32), dict(type='DefaultFormatBundle'),
            dict(type='Collect', keys=['img'])]


def demo_window(box, h, w, expand=0.8):
    """Cell 4 of the notebook in its own python expressions (its `w` is the row count) -> y0, y1, x0, x1."""
    x1, y1, x2, y2 = (float(v) for v in box)
    cy, cx = int(y1 + y2) // 2, int(x1 + x2) // 2
    l = int(max(y2 - y1, x2 - x1) * expand)
    return max(0, cy - l), min(cy + l, h), max(0, cx - l), min(cx + l, w)


def oracle_crop(frame, window, scale, pad, to_rgb=True):
    """window y0, x0, h, w -> (img [3, pad, pad], img_hw, scale_factor): the demo's slice through the oracle's L2CS chain."""
    y0, x0, h, w = window
    chw, meta = po.test_pipeline(frame[y0:y0 + h, x0:x0 + w], crop=None, img_scale=(scale, scale), to_rgb=to_rgb)
    out = np.zeros((3, pad, pad), np.float32)
    out[:, :chw.shape[1], :chw.shape[2]] = chw
    return out, meta['img_shape'][:2], meta['scale_factor']


def oracle_crops(frames, boxes, image_of, scale, pad, to_rgb=True):
    wins = []
    for b, k in zip(boxes, image_of):
        y0, y1, x0, x1 = demo_window(b, *frames[k].shape[:2])
        assert y1 > y0 and x1 > x0
        wins.append((y0, x0, y1 - y0, x1 - x0))
    got = [oracle_crop(frames[k], win, scale, pad, to_rgb) for win, k in zip(wins, image_of)]
    return (np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int32), np.stack([g[2] for g in got]).astype(np.float32),
            np.array(wins, dtype=np.int32))


@pytest.fixture(scope='module')
def want64():
    """The oracle's answer for the hand-worked cases at img_scale 64 (computed once; read-only)."""
    want = oracle_crops(FRAMES, BOXES, IMAGE_OF, 64, 64)
    assert want[3].tolist() == [list(c[3]) for c in CASES]      # demo_window and the hand-worked windows agree
    return want


def check(got, want, what=''):
    img, img_hw, scale_factor, crop, flags = (t.cpu() for t in got)
    assert img.dtype == torch.float32 and img_hw.dtype == torch.int32 and scale_factor.dtype == torch.float32 and crop.dtype == torch.int32
    assert torch.equal(crop, torch.from_numpy(want[3])), (what, crop.tolist())
    assert torch.equal(img_hw, torch.from_numpy(want[1])), (what, img_hw.tolist())
    assert torch.equal(scale_factor, torch.from_numpy(want[2])), what
    assert torch.equal(img, torch.from_numpy(want[0])), (what, int((img != torch.from_numpy(want[0])).sum()))
    assert flags.tolist() == [0] * len(flags), what


def same(a, b):
    for x, y, name in zip(a, b, ('img', 'img_hw', 'scale_factor', 'crop', 'flags')):
        assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()), name


# ---------------------------------------------------------------- 1. bit-exact against the oracle
@pytest.mark.parametrize('to_rgb', [True, False], ids=['to_rgb', 'bgr'])
def test_head_crops_bit_exact_against_the_oracle(want64, to_rgb):
    want = want64 if to_rgb else oracle_crops(FRAMES, BOXES, IMAGE_OF, 64, 64, to_rgb=False)
    got = P.DevicePipeline(chain(64, to_rgb)).head_crops(FRAMES, BOXES, IMAGE_OF, device=DEV)
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (len(CASES), 3, 64, 64)
    check(got, want, f'to_rgb={to_rgb}')
    # rgb=True: the same frames handed over in the decoder's RGB order give the same tensor
    got = P.DevicePipeline(chain(64, to_rgb)).head_crops([np.ascontiguousarray(f[..., ::-1]) for f in FRAMES], BOXES, IMAGE_OF, device=DEV, rgb=True)
    torch.cuda.synchronize()
    check(got, want, f'to_rgb={to_rgb}, rgb source')


def test_one_crop_at_the_demo_scale():
    """img_scale (448, 448) as in the L2CS config: an up-scale by 14 of the interior case and a clipped, non-square one."""
    boxes, image_of = BOXES[[0, 2]], IMAGE_OF[[0, 2]]
    want = oracle_crops(FRAMES, boxes, image_of, 448, 448)
    assert want[1].tolist() == [[448, 448], [415, 448]]          # 25 x 27 window: f = 448 / 27, int(25 f + 0.5) = 415
    got = P.DevicePipeline(chain(448)).head_crops(FRAMES, boxes, image_of, device=DEV)
    torch.cuda.synchronize()
    check(got, want, '448')


# ---------------------------------------------------------------- 2. device tables and frames
def test_device_tables_and_frames_equal_host_ones(want64):
    pipe = P.DevicePipeline(chain(64))
    ref = pipe.head_crops(FRAMES, BOXES, IMAGE_OF, device=DEV)
    dev_frames = [torch.from_numpy(f).to(DEV) for f in FRAMES]
    boxes, image_of = torch.from_numpy(BOXES).to(DEV), torch.from_numpy(IMAGE_OF).to(DEV)
    same(pipe.head_crops(FRAMES, boxes, image_of, device=DEV), ref)                  # device tables, host frames
    same(pipe.head_crops(dev_frames, BOXES, IMAGE_OF, device=DEV), ref)              # host tables, device frames
    same(pipe.head_crops(dev_frames, boxes, image_of, device=DEV), ref)              # nothing from the host
    same(pipe.head_crops(dev_frames, boxes, image_of.to(torch.int64), device=DEV), ref)
    same(pipe.head_crops([dev_frames[0], FRAMES[1]], boxes, image_of, device=DEV), ref)   # mixed
    # rows further apart than 3 w bytes: a view into a wider buffer
    wide = []
    for f in FRAMES:
        buf = torch.full((f.shape[0], f.shape[1] + 5, 3), 255, dtype=torch.uint8, device=DEV)
        buf[:, :f.shape[1]] = torch.from_numpy(f).to(DEV)
        wide.append(buf[:, :f.shape[1]])
        assert wide[-1].stride(0) == 3 * (f.shape[1] + 5)
    got = pipe.head_crops(wide, boxes, image_of, device=DEV)
    torch.cuda.synchronize()
    same(got, ref)
    check(got, want64, 'pitched frames')
    with pytest.raises(TypeError, match='packed pixels'):
        pipe.head_crops([dev_frames[0][:, ::2], dev_frames[1]], boxes, image_of, device=DEV)


# ---------------------------------------------------------------- 3. nothing is read on the host
def test_head_crops_capture_in_a_graph_and_follow_the_box_tensor(want64):
    pipe = P.DevicePipeline(chain(64))
    dev_frames = [torch.from_numpy(f).to(DEV) for f in FRAMES]
    boxes, image_of = torch.from_numpy(BOXES).to(DEV), torch.from_numpy(IMAGE_OF).to(DEV)
    new_boxes = torch.from_numpy(BOXES2).to(DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # eager warm-up: uploads the frame table of these frames, once
        pipe.head_crops(dev_frames, boxes, image_of, device=DEV)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pipe.head_crops(dev_frames, boxes, image_of, device=DEV)
    graph.replay()
    torch.cuda.synchronize()
    check(out, want64, 'replay')
    boxes.copy_(new_boxes)
    graph.replay()
    torch.cuda.synchronize()
    check(out, oracle_crops(FRAMES, BOXES2, IMAGE_OF, 64, 64), 'replay on new boxes')


def test_run_many_and_head_crops_take_turns_on_one_staging_ring():
    """One DevicePipeline, 2 * STAGES + 1 calls on a side stream handed over as stream=, nothing synchronised between them: run_many and head_crops
    (BGR frames, NV12 planes; all from the host) alternate, so run_many refills every stage and each head_crops call lands between two of its
    uploads; the middle call stages a 640 x 600 frame, past the 1 MiB a stage starts with, so a stage is reallocated while earlier work is
    queued.  After ONE synchronise every call's output equals the same call on a fresh pipeline of its own, bit for bit."""
    rs = np.random.RandomState(11)
    frame = lambda h, w: rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    box = np.array([[2, 2, 7, 7], [1, 3, 6.5, 8]], dtype=np.float32)         # l = 4: rows [0, 8) and [1, 8) of any frame here
    calls, n = [], 2 * P.DevicePipeline.STAGES + 1
    for k in range(n):
        h, w = 8 + 2 * rs.randint(0, 5), 8 + 2 * rs.randint(0, 5)              # 8 .. 16, even: NV12 sizes
        if k % 2 == 0:
            big = [frame(600, 640)] if k == n // 2 else []
            windows = [[frame(h, w), frame(w, h)] + big, [frame(8, 16)]]        # padded to 64 x 64 and to 32 x 64: two launches
            calls.append(lambda pipe, windows=windows, k=k, **kw: pipe.run_many(windows, device=DEV, rng=np.random.RandomState(k), **kw))
        elif k % 4 == 1:
            frames = [frame(h, w), frame(12, 8)]
            calls.append(lambda pipe, frames=frames, **kw: pipe.head_crops(frames, box, [0, 1], device=DEV, **kw))
        else:
            planes = [(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h // 2, w // 2, 2)).astype(np.uint8)) for _ in range(2)]
            calls.append(lambda pipe, planes=planes, **kw: pipe.head_crops(planes, box, [1, 0], device=DEV, pixel_format='nv12', matrix='bt709', **kw))
    assert sum(k % 2 == 0 for k in range(n)) == P.DevicePipeline.STAGES + 1 and n // 2 % 2 == 0     # run_many comes round to every stage; it makes the big call
    assert 600 * 640 * 3 > 1 << 20                               # ... whose bytes no stage holds yet
    pipe, side = P.DevicePipeline(chain(64)), torch.cuda.Stream(DEV)
    got = [call(pipe, stream=side.cuda_stream) for call in calls]
    torch.cuda.synchronize()
    for k, (call, g) in enumerate(zip(calls, got)):
        want = call(P.DevicePipeline(chain(64)))
        torch.cuda.synchronize()
        if k % 2:
            same(g, want)
            continue
        assert len(g) == len(want) == 2
        for (img, metas), (wimg, wmetas) in zip(g, want):
            assert img.shape == wimg.shape and torch.equal(img.cpu(), wimg.cpu()), k
            assert [sorted(m) for m in metas] == [sorted(m) for m in wmetas]
            assert all(np.array_equal(m[key], wm[key]) for m, wm in zip(metas, wmetas) for key in ('ori_shape', 'img_shape', 'pad_shape', 'scale_factor')), k


# ---------------------------------------------------------------- 4. flags
def test_flags_mark_rows_without_a_window_and_leave_their_neighbours_alone(want64):
    pipe = P.DevicePipeline(chain(64))
    nan = float('nan')
    # rows 1, 3, 5 are the odd ones: no extent (l = 0), a NaN, an image index one past the table; rows 0, 2, 4, 6 are cases 0, 1, 3, 6
    keep = [0, 1, 3, 6]
    boxes = np.array([BOXES[0], (50, 40, 51, 41), BOXES[1], (10, nan, 30, 40), BOXES[3], BOXES[2], BOXES[6]], dtype=np.float32)
    image_of = np.array([0, 0, 0, 1, 1, len(FRAMES), 0], dtype=np.int32)
    got = pipe.head_crops(FRAMES, torch.from_numpy(boxes).to(DEV), torch.from_numpy(image_of).to(DEV), device=DEV)
    torch.cuda.synchronize()
    img, img_hw, scale_factor, crop, flags = (t.cpu() for t in got)
    assert flags.tolist() == [0, 1, 0, 2, 0, 2, 0]
    for t in (img, scale_factor):
        assert bool(torch.isfinite(t).all())
    rows = [0, 2, 4, 6]
    for t, w in zip((img, img_hw, scale_factor, crop), want64):
        assert torch.equal(t[rows], torch.from_numpy(w[keep]))
    # flag 1: one pixel inside the frame, where the empty slice started; flag 2: pixel (0, 0) of frame 0
    assert crop[1].tolist() == [40, 50, 1, 1] and crop[3].tolist() == [0, 0, 1, 1] and crop[5].tolist() == [0, 0, 1, 1]
    for row, (y, x) in ((1, (40, 50)), (3, (0, 0)), (5, (0, 0))):
        want = oracle_crop(FRAMES[0], (y, x, 1, 1), 64, 64)
        assert torch.equal(img[row], torch.from_numpy(want[0])) and img_hw[row].tolist() == [64, 64] and scale_factor[row].tolist() == [64.0] * 4
    # host tables: the same rows are refused before anything is launched
    for bad in (1, 3, 5):
        with pytest.raises(ValueError):
            pipe.head_crops(FRAMES, boxes[[0, bad]], image_of[[0, bad]], device=DEV)
    # a box wholly outside the frame on one axis (rows [4, 36), columns [194, 131)): still one pixel, inside; and one whose coordinates no int
    # holds (cx = 0, cy = 1.5e38, l = 2.4e38): the whole frame, as python's unbounded ints give
    got = pipe.head_crops(FRAMES, torch.tensor([[200., 10., 220., 30.], [-1e30, 0., 1e30, 3e38]], device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), device=DEV)
    torch.cuda.synchronize()
    assert got[4].tolist() == [1, 0] and got[3][0].tolist() == [4, 130, 1, 1] and got[3][1].tolist() == [0, 0, 97, 131]


# ---------------------------------------------------------------- 5. end to end
H, W = 96, 128


def video():
    rs = np.random.RandomState(7)
    frames = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(12)]
    per_frame = []
    for t in range(12):
        if t < 8:
            a, b = [10 + t, 20, 40 + t, 55.5], [100 + t, 60, 135 + t, 100]     # b's window leaves the frame right and below
            per_frame.append([b, a] if t % 2 else [a, b])                      # label order is not x order
        else:
            per_frame.append([[50, 30 + t, 80.5, 62 + t]])
    return frames, per_frame


@pytest.fixture(scope='module')
def engines():
    from mcgaze_amd.engine import HipEngine
    sd = synth.make_state_dict(0)
    return {p: HipEngine(sd, precision=p) for p in ('f16x3', 'fp32')}


def oracle_tracks(frames, segments):
    tracks = []
    for si, seg in enumerate(segments):
        for pi, person in enumerate(seg['boxes']):
            img, hw, sf, win = oracle_crops(frames, np.asarray(person, dtype=np.float32), seg['frame_id'], 64, 64)
            tracks.append(dict(id=(si, pi), frames=torch.from_numpy(img), img_hw=hw, scale_factor=sf, crop=win))
    return tracks


def check_records(got, want, tracks, segments):
    assert [g['id'] for g in got] == [t['id'] for t in tracks] == [w['id'] for w in want]
    for g, w, t in zip(got, want, tracks):
        si, pi = g['id']
        for k in ('det', 'fused', 'others'):
            assert g[k].dtype == np.float32 and np.array_equal(g[k].view(np.int32), w[k].view(np.int32)), (g['id'], k)
        assert g['frame_id'] == segments[si]['frame_id'] and np.array_equal(g['crop'], t['crop'])
        assert np.array_equal(g['head_box'], np.asarray(segments[si]['boxes'][pi], dtype=np.float32))
        for (x1, y1, x2, y2), f, arrow in zip(segments[si]['boxes'][pi], g['fused'], g['arrow']):     # cell 5, in python
            cx, cy, l = int(x1 + x2) // 2, int(y1 + y2) // 2, int(max(y2 - y1, x2 - x1) * 1)
            assert arrow.tolist() == [[cx, cy], [int(cx - l * float(f[0])), int(cy - l * float(f[1]))]]


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_run_head_video_equals_run_tracks_on_oracle_crops(engines, precision, monkeypatch):
    e = engines[precision]
    frames, per_frame = video()
    segments = harness.segment_tracks(per_frame)
    assert [len(s['frame_id']) for s in segments] == [8, 4] and [len(s['boxes']) for s in segments] == [2, 1]
    tracks = oracle_tracks(frames, segments)
    assert any(t['crop'][:, 2:].min() < t['crop'][:, 2:].max() for t in tracks)          # a clipped, non-square window is in the set
    want = harness.run_tracks(e, tracks, max_len=4)
    lengths = []
    forward = e.forward
    monkeypatch.setattr(e, 'forward', lambda x, T, **kw: (lengths.extend(T), forward(x, T, **kw))[1])
    pipe = P.DevicePipeline(chain(64))
    got = harness.run_head_video(e, pipe, frames, per_frame, max_len=4)
    assert sorted(lengths) == [3, 3, 4, 5, 5]                   # chunks of 5 + 3 for each of two people, of 4 for the third
    check_records(got, want, tracks, segments)
    # groups of at most 6 crops (every chunk its own upload and engine call) and device-resident frames: the same records
    got = harness.run_head_video(e, pipe, [torch.from_numpy(f).to(DEV) for f in frames], per_frame, max_len=4, batch_frames=6)
    check_records(got, want, tracks, segments)


@pytest.mark.parametrize('precision', ['f16x3', 'fp32'])
def test_run_head_video_on_a_clip_longer_than_ten_frames(engines, precision):
    """One person for 12 frames and the demo's max_len = 100: ONE clip of 12 frames, past the fused attention block's 10."""
    e = engines[precision]
    frames, _ = video()
    per_frame = [[[30 + 2 * t, 18, 75 + 2 * t, 70.5]] for t in range(12)]
    segments = harness.segment_tracks(per_frame)
    assert [len(s['frame_id']) for s in segments] == [12]
    tracks = oracle_tracks(frames, segments)
    want = harness.run_tracks(e, tracks, max_len=100)
    got = harness.run_head_video(e, P.DevicePipeline(chain(64)), frames, per_frame, max_len=100)
    check_records(got, want, tracks, segments)
