"""Test-time data pipeline behind the reference's config surface.

``cfg.data.test.pipeline`` of the reference (configs/_base_/datasets/gaze360.py:27-36 and the L2CS variant
configs/multiclue_gaze/multiclue_gaze_r50_l2cs.py:31-39) is a list of transform dicts that mmdet's ``Compose``
(mmdet/datasets/pipelines/compose.py) runs one frame at a time on the CPU.  Here the same dicts build the same-named classes
from a ``PIPELINES`` registry, but the classes only carry the validated options and the GEOMETRY of their transform (crop
window, resized size, padded size, meta keys, and the RNG draws the reference makes, in the reference's order).  The pixel
work of the whole chain runs as ONE HIP launch per clip batch (``mcg_preprocess_frames``): decoded uint8 BGR frames go to the
device as they are, and the kernel writes the model's ``img`` tensor.  There is no CPU pixel path: without the library
``DevicePipeline.__call__`` raises.

    pipe = DevicePipeline(cfg.data.test.pipeline)
    img, img_metas = pipe(frames, device='cuda:0')            # frames: list of HxWx3 uint8 BGR arrays or file names
    model(img=[img], img_metas=[img_metas], return_loss=False, rescale=True, clip_length=7)

Head crops (``DevicePipeline.head_crops``): the demo of the reference (MCGaze_demo/demo.ipynb, cell 4) cuts one window per person out of
every video frame before this chain; there the WINDOW is chosen on the device as well (``mcg_preprocess_head_crops``), from frames and head
boxes that may both live in device memory already.  ``head_crop_window`` is the same arithmetic on the host, for checks and for drawing.
``DevicePipeline.letterbox`` makes the head detector's input from the same frames, ``detect_heads`` head boxes from its raw output and
``track_heads`` one identity per person from the boxes of consecutive frames.
Re-exported from beside this module: decoded frames (frame_cache.py), NV12 (nv12.py), arrows (arrows.py), gaze targets (attention.py), the detector's two sides (head_detect.py), upload (staging.py).

What the device calls of ``DevicePipeline`` share is stated once, and a further call is written from these pieces: every call runs in a
``_call_scope`` (staging.py: the device, the caller's stream, the one upload, the mark on the stage it took); ``_row_tables`` checks the rows
of head_crops and the two drawing calls; ``_on_device`` / ``_there`` decide where a table lives and move a host table that stands next to a
device one; ``_gaze_operand`` is the gaze table with its row stride; ``_region_operands`` decides the region tables of gaze_targets and
draw_attention as a group; ``_drawing_checked``, ``_drawing_placed`` and ``_drawing_upload`` are, in the order of a call, what draw_arrows,
draw_attention, draw_labels and anonymize_heads do to frames and rows; and ``_device_table`` keeps the record tables of device frames on the device.

Randomness: the reference's ``CenterCrop(crop_type='relative_range')`` draws the crop size from the global numpy RNG at TEST
time too (transforms.py:1126-1130), and ``RandomFlip(flip_ratio=0.0)`` consumes one more uniform
(np.random.choice, transforms.py:463-497).  ``rng`` (default: the global ``np.random``) is drawn from in that order per frame,
so a seeded single-threaded run reproduces the reference's windows; ``crop_u=<float>`` pins the draw instead.
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import lib as L
from .arrows import (OVERLAY_PALETTE, _overlay_counts, _overlay_palette, _overlay_regions, _overlay_targets, _overlay_thickness,  # noqa: F401
                     draw_attention_host)
from .arrows import (ARROW_COLOR, ARROW_COORD, ARROW_SIDE, _arrow_colors, _arrow_params, _arrow_rows,  # noqa: F401
                     arrow_segments, draw_arrows_host, segment_coverage)
from .arrows import LABEL_CHARS, LABEL_FONT, _label_background, _label_ints, _label_params, _label_rate, _label_text, label_plan
from .arrows import draw_labels_host, encode_labels, format_labels_host  # noqa: F401  (re-exported beside draw_arrows_host, for users of pipeline.*)
from .arrows import HEAT_LUT, draw_heat_host, draw_surface_heat_host, heat_lut  # noqa: F401
from .arrows import _anon_color, _anon_params, anonymize_heads_host, anonymize_plan_host  # noqa: F401
from .attention import (HEAT_KINDS, HeatState, _heat_cell, _heat_grid, _heat_params, _heat_scale, gaze_heat_host,  # noqa: F401
                        heat_grid_shape)
from .attention import PolyRegions, _check_counts, _holds_polygon, _poly_tables, _region_tables, _target_params, gaze_targets_host, region_polygons  # noqa: F401
from .attention import _row_tables as _target_rows
from .attention import MAX_CAMERAS, PolyRegions3D, _camera_table, _depth_table, _poly3d_tables, _target3d_params, gaze_targets_3d_host, regions_3d  # noqa: F401
from .attention import (SURFACE_GRID, SURFACE_RADIUS, SurfaceHeatState, _surface_grid, _surface_grid_option, _surface_params,  # noqa: F401
                        _surface_regions, surface_charts_host, surface_extent, surface_heat_host)
from .attention import DWELL_ENTER, DWELL_EXIT, _dwell_counts, _dwell_params, _dwell_tables, gaze_dwell_host  # noqa: F401
from .frame_cache import FrameCache, _DecodeProcs, decode_image  # noqa: F401
from .head_detect import (DETECT_MAX_DET, LETTERBOX_PAD, LetterboxGeometry, _detect_params, _detect_shapes, _letterbox_dtype,  # noqa: F401
                          _letterbox_plan, _track_motion, _track_params, _track_shapes, detect_heads_host, letterbox_geometry, letterbox_host, track_heads_host,
                          track_state_words)
from .nv12 import YUV_COEF, _nv12_planes, _pixel_format, _yuv_coef, _yuv_to_bgr, bgr_to_yuv, nv12_to_bgr  # noqa: F401
from .registry import Registry
from .staging import _Stage, _StagingRing, _bgr_frame, _call_scope, _host_array, _layout  # noqa: F401

PIPELINES = Registry('pipeline')


class FramePlan:
    """Geometry of one frame on its way through the chain (what the reference keeps in the ``results`` dict)."""

    def __init__(self, shape, filename=None, ori_filename=None):
        self.ori_shape = tuple(shape)
        self.filename, self.ori_filename = filename, ori_filename
        self.crop = (0, 0, shape[0], shape[1])      # y, x, h, w inside the decoded frame
        self.img_shape = tuple(shape)                # current (h, w, c)
        self.pad_shape = None
        self.scale_factor = None
        self.flip, self.flip_direction = False, None
        self.img_norm_cfg = None
        self.resized = False


@PIPELINES.register_module()
class LoadImageFromFile:
    """loading.py:36-82.  Decode happens on the host (PIL); the array stays uint8 BGR like cv2.imread's."""

    def __init__(self, to_float32=False, color_type='color', channel_order='bgr', file_client_args=dict(backend='disk')):
        if to_float32 or color_type != 'color' or channel_order != 'bgr' or file_client_args.get('backend', 'disk') != 'disk':
            raise NotImplementedError('LoadImageFromFile: only uint8 colour BGR frames from disk feed the device pipeline')

    load = staticmethod(decode_image)

    def plan(self, p, rng):
        pass


@PIPELINES.register_module()
class CenterCrop:
    """transforms.py:953-1160: a CENTRED window whose size follows ``crop_type`` (the random offsets are commented out
    upstream, :1040-1043); 'relative_range' draws ONE uniform for both sides (:1126-1130)."""

    def __init__(self, crop_size, crop_type='absolute', allow_negative_crop=False, recompute_bbox=False, bbox_clip_border=True, crop_u=None):
        if crop_type not in ['relative_range', 'relative', 'absolute', 'absolute_range']:
            raise ValueError(f'Invalid crop_type {crop_type}.')
        if crop_type in ['absolute', 'absolute_range']:
            assert crop_size[0] > 0 and crop_size[1] > 0
            assert isinstance(crop_size[0], int) and isinstance(crop_size[1], int)
        else:
            assert 0 < crop_size[0] <= 1 and 0 < crop_size[1] <= 1
        self.crop_size, self.crop_type, self.crop_u = crop_size, crop_type, crop_u
        if crop_type == 'relative_range':
            # upstream: cs = float32 array, u = float64 array -> cs + u * (1 - cs) with (1 - cs) rounded in f32 and the rest in f64.
            # The same values as python floats (one rounding per operation, like the array expression), without three array temporaries per frame.
            cs = np.asarray(crop_size, dtype=np.float32)
            self._cs = [float(v) for v in cs]
            self._rest = [float(v) for v in (1 - cs)]

    def _get_crop_size(self, h, w, rng):
        if self.crop_type == 'absolute':
            return min(self.crop_size[0], h), min(self.crop_size[1], w)
        if self.crop_type == 'absolute_range':
            assert self.crop_size[0] <= self.crop_size[1]
            crop_h = rng.randint(min(h, self.crop_size[0]), min(h, self.crop_size[1]) + 1)
            crop_w = rng.randint(min(w, self.crop_size[0]), min(w, self.crop_size[1]) + 1)
            return crop_h, crop_w
        if self.crop_type == 'relative':
            return int(h * self.crop_size[0] + 0.5), int(w * self.crop_size[1] + 0.5)
        u = rng.random_sample() if self.crop_u is None else float(self.crop_u)        # ONE uniform for both sides (:1126-1130; rand(1) draws the same double)
        crop_h, crop_w = self._cs[0] + u * self._rest[0], self._cs[1] + u * self._rest[1]
        return int(h * crop_h + 0.5), int(w * crop_w + 0.5)

    def plan(self, p, rng):
        if p.resized:
            raise NotImplementedError('CenterCrop after Resize is not a chain the device kernel fuses')
        y, x, h, w = p.crop
        ch, cw = self._get_crop_size(h, w, rng)
        assert ch > 0 and cw > 0
        oy, ox = int(max(h - ch, 0) / 2 + 0.5), int(max(w - cw, 0) / 2 + 0.5)
        ch, cw = min(ch, h - oy), min(cw, w - ox)
        p.crop = (y + oy, x + ox, ch, cw)
        p.img_shape = (ch, cw) + p.img_shape[2:]


@PIPELINES.register_module()
class Resize:
    """transforms.py:31-330 for the single-scale test-time use: keep_ratio -> mmcv.imrescale's size rule, else exact size;
    bilinear (cv2.INTER_LINEAR), which is what the kernel implements."""

    def __init__(self, img_scale=None, multiscale_mode='range', ratio_range=None, keep_ratio=True, bbox_clip_border=True, backend='cv2',
                 override=False, interpolation='bilinear'):
        if isinstance(img_scale, list):
            if len(img_scale) != 1:
                raise NotImplementedError('Resize: multi-scale sampling is a training option')
            img_scale = img_scale[0]
        if img_scale is None or ratio_range is not None or backend != 'cv2' or interpolation != 'bilinear':
            raise NotImplementedError('Resize: only img_scale=(w, h) with the cv2 bilinear backend is supported')
        assert isinstance(img_scale, tuple) and len(img_scale) == 2
        self.img_scale, self.keep_ratio = img_scale, keep_ratio

    def plan(self, p, rng):
        if p.resized:
            raise NotImplementedError('two Resize transforms in one pipeline')
        h, w = p.img_shape[:2]
        if self.keep_ratio:
            f = min(max(self.img_scale) / max(h, w), min(self.img_scale) / min(h, w))
            new_w, new_h = int(w * float(f) + 0.5), int(h * float(f) + 0.5)
        else:
            new_w, new_h = self.img_scale
        p.scale_factor = np.array([new_w / w, new_h / h, new_w / w, new_h / h], dtype=np.float32)
        p.img_shape = (new_h, new_w) + p.img_shape[2:]
        p.pad_shape = p.img_shape
        p.resized = True


@PIPELINES.register_module()
class RandomFlip:
    """transforms.py:333-530.  Only the never-flipping test-time setting is supported; it still consumes the uniform
    np.random.choice draws in the reference (:485)."""

    def __init__(self, flip_ratio=None, direction='horizontal'):
        if isinstance(flip_ratio, list) or direction != 'horizontal':
            raise NotImplementedError('RandomFlip: list ratios / non-horizontal directions are training options')
        if isinstance(flip_ratio, float):
            assert 0 <= flip_ratio <= 1
        elif flip_ratio is not None:
            raise ValueError('flip_ratios must be None, float, or list of float')
        if flip_ratio:
            raise NotImplementedError('RandomFlip: flip_ratio > 0 is a training option; the test pipeline uses 0.0')
        self.flip_ratio = flip_ratio

    def plan(self, p, rng):
        if self.flip_ratio is not None:
            rng.random_sample()
        p.flip, p.flip_direction = False, None


@PIPELINES.register_module()
class Normalize:
    """transforms.py:722-760."""

    def __init__(self, mean, std, to_rgb=True):
        self.mean, self.std, self.to_rgb = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32), to_rgb
        self._cfg = dict(mean=self.mean, std=self.std, to_rgb=self.to_rgb)       # one object for every frame's meta (read-only by convention)

    def plan(self, p, rng):
        p.img_norm_cfg = self._cfg


@PIPELINES.register_module()
class Pad:
    """transforms.py:623-720: zeros below / right, up to a multiple of size_divisor or a fixed size."""

    def __init__(self, size=None, size_divisor=None, pad_to_square=False, pad_val=dict(img=0, masks=0, seg=255)):
        if pad_to_square:
            raise NotImplementedError('Pad: pad_to_square')
        assert size is not None or size_divisor is not None, 'only one of size and size_divisor should be valid'
        assert size is None or size_divisor is None
        v = pad_val.get('img', 0) if isinstance(pad_val, dict) else pad_val
        if v != 0:
            raise NotImplementedError('Pad: the device kernel pads with zeros')
        self.size, self.size_divisor = size, size_divisor

    def plan(self, p, rng):
        h, w = p.img_shape[:2]
        if self.size is not None:
            ph, pw = max(self.size[0], h), max(self.size[1], w)
        else:
            d = self.size_divisor
            ph, pw = -(-h // d) * d, -(-w // d) * d                      # int(np.ceil(h / d)) * d
        p.pad_shape = (ph, pw) + p.img_shape[2:]


@PIPELINES.register_module()
class DefaultFormatBundle:
    """formatting.py:175-260: HWC -> CHW tensor; the kernel writes that layout."""

    def __init__(self, img_to_float=True, pad_val=dict(img=0, masks=0, seg=255)):
        pass

    def plan(self, p, rng):
        pass


@PIPELINES.register_module()
class ImageToTensor:
    def __init__(self, keys):
        self.keys = keys

    def plan(self, p, rng):
        pass


@PIPELINES.register_module()
class Collect:
    """formatting.py:279-352."""

    def __init__(self, keys, meta_keys=('filename', 'ori_filename', 'ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip',
                                        'flip_direction', 'img_norm_cfg')):
        if list(keys) != ['img']:
            raise NotImplementedError(f'Collect: the test pipeline collects only img (got {keys})')
        self.keys, self.meta_keys = keys, meta_keys

    def plan(self, p, rng):
        pass

    def meta(self, p):
        return {k: getattr(p, k) for k in self.meta_keys}


_DESC = np.dtype([('src', np.uint64)] + [(f, np.int32) for f in ('src_h', 'src_w', 'src_pitch', 'crop_y', 'crop_x', 'crop_h', 'crop_w', 'out_h', 'out_w')],
                 align=True)                       # lib.FrameDesc / mcg_frame_desc, as a numpy record
assert _DESC.itemsize == C.sizeof(L.FrameDesc) and all(_DESC.fields[n][1] == getattr(L.FrameDesc, n).offset for n in _DESC.names)


_IMAGE = np.dtype([('src', np.uint64), ('h', np.int32), ('w', np.int32), ('pitch', np.int32)], align=True)   # lib.ImageDesc / mcg_image_desc
assert _IMAGE.itemsize == C.sizeof(L.ImageDesc) and all(_IMAGE.fields[n][1] == getattr(L.ImageDesc, n).offset for n in _IMAGE.names)
_DESC_WORDS = _DESC.itemsize // 4
# the NV12 records: lib.Nv12ImageDesc / mcg_nv12_image_desc, and mcg_nv12_frame_desc = the fields of _DESC, then the UV plane and its pitch
_NV12_IMAGE = np.dtype([('y', np.uint64), ('uv', np.uint64), ('h', np.int32), ('w', np.int32), ('pitch_y', np.int32), ('pitch_uv', np.int32)], align=True)
assert _NV12_IMAGE.itemsize == C.sizeof(L.Nv12ImageDesc) and all(_NV12_IMAGE.fields[n][1] == getattr(L.Nv12ImageDesc, n).offset for n in _NV12_IMAGE.names)
_NV12_DESC = np.dtype([(n, _DESC.fields[n][0]) for n in _DESC.names] + [('uv', np.uint64), ('uv_pitch', np.int32)], align=True)
assert _NV12_DESC.itemsize == C.sizeof(L.Nv12FrameDesc) and all(_NV12_DESC.fields[n][1] == getattr(L.Nv12FrameDesc, n).offset for n in _NV12_DESC.names)
_NV12_DESC_WORDS = _NV12_DESC.itemsize // 4
# the letterbox records: lib.LetterboxDesc / mcg_letterbox_desc and its NV12 twin = a frame descriptor, then the rectangle's corner
_LETTERBOX, _NV12_LETTERBOX = (np.dtype([('frame', d), ('top', np.int32), ('left', np.int32)], align=True) for d in (_DESC, _NV12_DESC))
for _d, _c in ((_LETTERBOX, L.LetterboxDesc), (_NV12_LETTERBOX, L.Nv12LetterboxDesc)):
    assert _d.itemsize == C.sizeof(_c) and all(_d.fields[n][1] == getattr(_c, n).offset for n in _d.names)
_LETTERBOX_TYPES = {torch.uint8: L.LETTERBOX_U8, torch.float16: L.LETTERBOX_F16, torch.float32: L.LETTERBOX_F32}
_CROP_WORD = _DESC.fields['crop_y'][1] // 4         # crop_y, crop_x, crop_h, crop_w are consecutive int32 words of a descriptor
_ARROW = np.dtype([('seg', np.int32, (3, 2, 2)), ('thickness', np.int32)] + [(f, np.int32) for f in ('x0', 'y0', 'x1', 'y1', 'image', 'flag', 'reserved')])
assert _ARROW.itemsize == C.sizeof(L.ArrowDesc) and all(_ARROW.fields[n][1] == getattr(L.ArrowDesc, n).offset for n in _ARROW.names)
_ARROW_WORDS = _ARROW.itemsize // 4
_LABEL = np.dtype([(f, np.int32) for f in ('x', 'y', 'x0', 'y0', 'x1', 'y1', 'image', 'flag', 'len')] + [('color', np.uint32), ('text', np.uint8, (LABEL_CHARS,))])
assert _LABEL.itemsize == C.sizeof(L.LabelDesc) == 64 and all(_LABEL.fields[n][1] == getattr(L.LabelDesc, n).offset for n in _LABEL.names)
_LABEL_WORDS = _LABEL.itemsize // 4
_ANON_WORDS = C.sizeof(L.AnonDesc) // 4


class _NoDraw:
    """The generator behind head_crop_geometry's planning pass: RandomFlip(0.0)'s uniform decides nothing and is not drawn from the caller's."""

    @staticmethod
    def random_sample():
        return 0.0


_NO_DRAW = _NoDraw()


def head_crop_windows(boxes, h, w, expand=0.8):
    """The demo's head windows (MCGaze_demo/demo.ipynb, cell 4) for n boxes at once, in the doubles python computes them in:

        head_center = [int(y1 + y2) // 2, int(x1 + x2) // 2];   l = int(max(y2 - y1, x2 - x1) * 0.8)
        head_crop = img[max(0, cy - l):min(cy + l, rows), max(0, cx - l):min(cx + l, cols)]

    boxes [n,4] x1 y1 x2 y2 (finite), h / w: frame size per box (scalars or [n]).  -> (windows int64 [n,4] = y0, x0, h, w; empty bool [n]):
    a window the slice would leave empty (a box of no extent, or wholly outside the frame) is reported as ONE pixel moved inside the frame
    and marked in ``empty`` -- what head_crop_plan_kernel (csrc/preprocess.hip) writes with flag 1; this is that kernel, line for line."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    if not np.isfinite(b).all():
        raise ValueError('head boxes must be finite')
    l = np.trunc(np.maximum(b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]) * float(expand))

    def span(a, c, size):
        size = np.broadcast_to(np.asarray(size, dtype=np.float64), a.shape)
        ctr = np.floor(np.trunc(a + c) / 2.0)        # int(a + c) // 2: truncate, then floor-divide (they differ below zero)
        lo, hi = np.maximum(0.0, ctr - l), np.minimum(ctr + l, size)
        return np.minimum(lo, size - 1), hi, ~(hi > lo)

    y0, y1, ey = span(b[:, 1], b[:, 3], h)
    x0, x1, ex = span(b[:, 0], b[:, 2], w)
    empty = ey | ex
    win = np.stack([y0, x0, np.where(empty, 1.0, y1 - y0), np.where(empty, 1.0, x1 - x0)], axis=1).astype(np.int64)
    return win, empty


def head_crop_window(box, h, w, expand=0.8):
    """(y0, x0, crop_h, crop_w) of ONE head box [x1, y1, x2, y2] in an h x w frame: the window ``DevicePipeline.head_crops`` cuts (and
    returns as ``crop``).  ValueError where the demo's slice is empty -- its cv2.resize would raise there."""
    win, empty = head_crop_windows([box], h, w, expand)
    if empty[0]:
        raise ValueError(f'head box {[float(v) for v in box]} leaves an empty window in a {h} x {w} frame')
    return tuple(int(v) for v in win[0])


def _device(device, entry=None):
    """torch.device(device); a bare 'cuda' is the current device BY INDEX -- staging buffers and device frames are compared with it.  With
    ``entry``, the library call about to be made, anything but a GPU is refused."""
    dev = torch.device(device)
    if entry is not None and dev.type != 'cuda':
        raise L.McgError(f'DevicePipeline runs its pixel work on the GPU ({entry}); there is no CPU path')
    return torch.device('cuda', torch.cuda.current_device()) if dev.type == 'cuda' and dev.index is None else dev


def _on_device(t):
    return isinstance(t, torch.Tensor) and t.is_cuda


def _tensor(t):
    return t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))


def _there(t, dev, dtype):
    """A table of any kind as a contiguous ``dtype`` tensor on ``dev``: how a host table next to a device one is moved (with torch, not
    through the staging ring), and how a device table of another type or layout becomes what the kernels read."""
    return (t if isinstance(t, torch.Tensor) else _tensor(t)).to(dev, dtype).contiguous()


def _gaze_operand(gaze, n, columns, dev):
    """The gaze table [n, >= columns] as the kernels take it -> (gaze, its row stride in floats).  A host array comes back as it is, its rows
    ``columns`` apart.  A tensor that is f32 on ``dev`` with packed rows -- the [n,3] ``fused`` of a results='device' stream, or the first
    columns of a wider table -- is read where it is; any other is converted and made contiguous.  Up to one row there is no row stride to
    take from the tensor: it is the row's width."""
    if not isinstance(gaze, torch.Tensor):
        return gaze, columns
    stride = gaze.stride(0) if n > 1 else gaze.shape[1]
    if not (gaze.device == dev and gaze.dtype == torch.float32 and gaze.stride(1) == 1 and stride >= columns):
        gaze, stride = gaze.to(dev, torch.float32).contiguous(), gaze.shape[1]
    return gaze, int(stride)


def _device_regions(who, regions, region_image, dev, as_vertices):
    """The region tables of ``who`` where one of them is a device tensor -> (poly, table, start, region_image) on ``dev``, the others moved
    with torch; nothing is read back, so only the shapes are checked (ValueError).  regions: a PolyRegions (table: xy [V,2]) or [m,4]
    rectangles, which stay [m,4] with no ``start`` unless ``as_vertices`` asks for them as 2-vertex regions."""
    poly = isinstance(regions, PolyRegions)
    if poly:
        table, start = _there(regions.xy, dev, torch.float32), _there(regions.start, dev, torch.int32)
        if table.ndim != 2 or table.shape[1] != 2 or start.ndim != 1 or start.shape[0] < 1:
            raise ValueError(f'{who}: PolyRegions is xy [V, 2] and start [m + 1], got {tuple(table.shape)} and {tuple(start.shape)}')
        m = int(start.shape[0]) - 1
    else:
        if regions is None:
            raise ValueError(f'{who}: region_image without regions')
        table, start = _there(regions, dev, torch.float32), None
        if table.ndim != 2 or table.shape[1] != 4:
            raise ValueError(f'{who}: regions must be [m, 4] x1 y1 x2 y2, got {tuple(table.shape)}')
        m = int(table.shape[0])
        if as_vertices:                                           # a rectangle is a 2-vertex region
            poly, table, start = True, table.view(-1, 2), torch.arange(0, 2 * m + 1, 2, dtype=torch.int32, device=dev)
    region_image = torch.full((m,), -1, dtype=torch.int32, device=dev) if region_image is None else _there(region_image, dev, torch.int32)
    if tuple(region_image.shape) != (m,):
        raise ValueError(f'{who}: region_image must be [{m}], one per region; got {tuple(region_image.shape)}')
    return poly, table, start, region_image


def _region_operands(who, regions, region_image, dev, as_vertices=False):
    """``regions`` / ``region_image`` as the user of ``who`` gave them -- [m,4] rectangles, the mixed list of ``region_polygons`` or a
    PolyRegions; region_image None: -1, every picture -- -> (poly, table, start, region_image, m, V).  Decided as a group: tables that are
    all on the host come back checked as numpy arrays, which go up through the staging ring; with one of them on the device all are tensors
    on ``dev`` (``_device_regions``).  poly: table is xy [V,2] with start [m+1]; else table is the rectangles [m,4], start None and V 0 --
    what mcg_gaze_targets takes.  as_vertices (the overlay): always the vertex form.
    Where to call it: inside the call's scope (the device branch allocates and copies on the caller's stream) and FIRST there, before
    anything is cloned or moved -- the host branch is a host check, and host checks come before the first clone, upload or launch.  The
    device branch's shape errors therefore come before the shape errors of the other device tables."""
    if _holds_polygon(regions):
        regions = region_polygons(regions)
    poly = isinstance(regions, PolyRegions)
    if any(_on_device(t) for t in ((*regions, region_image) if poly else (regions, region_image))):
        poly, table, start, region_image = _device_regions(who, regions, region_image, dev, as_vertices)
    elif as_vertices:
        poly, (table, start, region_image) = True, _overlay_regions(who, regions, region_image)
    elif poly:
        table, start, region_image = _poly_tables(who, regions, region_image)
    else:
        (table, region_image), start = _region_tables(who, regions, region_image), None
    return poly, table, start, region_image, int(region_image.shape[0]), int(table.shape[0]) if poly else 0


def _kernel_norm(norm, rgb, nv12=False):
    """-> (mean, stdinv, swap) as the pixel kernels take them.  swap: the wanted order differs from the source's; converted NV12 taps are BGR."""
    mean = (C.c_float * 3)(*[float(v) for v in norm['mean']])
    stdinv = (C.c_float * 3)(*[float(np.float32(1.0 / np.float64(v))) for v in norm['std']])
    return mean, stdinv, int(bool(norm['to_rgb']) != (bool(rgb) and not nv12))


def _image_table(images, dev, planes):
    """-> (table, parts).  table: one _IMAGE record per frame (_NV12_IMAGE with ``planes``, the frames as _nv12_planes returns them); parts: (frame,
    field of its record, bytes) of every HOST frame -- it gets its address once it is staged.  head_crops reads the frames it names, draw_arrows
    writes them."""
    table, parts = np.zeros(len(images), dtype=_IMAGE if planes is None else _NV12_IMAGE), []
    for k, im in enumerate(images):
        if planes is not None:
            y, uv, there = planes[k]
            h, w = y.shape
            if not there:
                parts += [(k, 'y', y.reshape(-1)), (k, 'uv', uv.reshape(-1))]
            table[k] = (y.data_ptr(), uv.data_ptr(), h, w, y.stride(0), uv.stride(0) if h > 2 else w) if there else (0, 0, h, w, w, w)
        elif isinstance(im, torch.Tensor):
            if not (im.is_cuda and im.device == dev and im.dtype == torch.uint8 and im.ndim == 3 and im.shape[2] == 3 and im.numel() > 0
                    and im.stride(2) == 1 and im.stride(1) == 3 and (im.shape[0] == 1 or im.stride(0) >= 3 * im.shape[1])):
                raise TypeError(f'frame {k}: device frames must be HxWx3 uint8 tensors on {dev} with packed pixels (stride (pitch, 3, 1)), '
                                f'got {im.dtype} {tuple(im.shape)} strides {tuple(im.stride())} on {im.device}')
            table[k] = (im.data_ptr(), im.shape[0], im.shape[1], im.stride(0) if im.shape[0] > 1 else 3 * im.shape[1])
        else:
            a = _bgr_frame(k, np.ascontiguousarray(im))
            parts.append((k, 'src', a.reshape(-1)))
            table[k] = (0, a.shape[0], a.shape[1], 3 * a.shape[1])
    return table, parts


def _arrow_targets(images, planes, copy, dev):
    """Where draw_arrows draws each frame -> (tensors, pixels, in_place): a device frame itself (copy: its packed clone), a fresh device tensor
    for a host frame (NV12: one [3H/2, W] surface as its (y, uv) views).  pixels: (the tensor they belong in, bytes) of the host frames, in image
    order; in_place: every frame is its own target."""
    out, pixels, in_place = [], [], not copy
    for k, im in enumerate(images):
        if planes is not None and not planes[k][2]:
            y, uv, in_place = planes[k][0], planes[k][1], False
            s = torch.empty(y.shape[0] * 3 // 2, y.shape[1], dtype=torch.uint8, device=dev)
            out.append((s[:y.shape[0]], s[y.shape[0]:]))
            pixels += [(out[-1][0], y.reshape(-1)), (out[-1][1], uv.reshape(-1))]
        elif planes is None and not isinstance(im, torch.Tensor):
            out.append(torch.empty(np.shape(im), dtype=torch.uint8, device=dev))
            in_place = False
            pixels.append((out[-1], np.ascontiguousarray(im).reshape(-1)))
        elif copy:
            clone = lambda t: t.clone(memory_format=torch.contiguous_format)
            out.append(tuple(clone(t) for t in im) if isinstance(im, (tuple, list)) else clone(im))
        else:
            out.append(im)
    return out, pixels, in_place


def _row_tables(caller, rows, frames, boxes, image_of, gaze=None):
    """The row tables of ``caller`` ('head_crops' cuts ``rows`` = 'crops', 'draw_arrows' draws 'arrows') over ``frames`` frames, as the device
    reads them -> (boxes, image_of, gaze, n).  Each of boxes [n,4], image_of [n] and the optional gaze [n,>=2] is a CUDA tensor, which comes
    back as it is and is not read back, or lives on the host and comes back CHECKED as a contiguous array: boxes f32 [n,4]; image_of int32
    [n] (TypeError unless it holds integers, ValueError outside [0, frames)); gaze f32, cut to its first two columns.  ValueError where the shapes
    do not belong together or n exceeds 65535."""
    if not _on_device(boxes):
        boxes = np.ascontiguousarray(_host_array(boxes), dtype=np.float32).reshape(-1, 4)     # f32 is what the device reads: the checks see the same boxes
    n = int(boxes.shape[0])
    if gaze is not None and not _on_device(gaze):
        gaze = np.ascontiguousarray(_host_array(gaze), dtype=np.float32)
        gaze = np.zeros((0, 2), np.float32) if n == 0 and gaze.size == 0 else np.ascontiguousarray(gaze[:, :2]) if gaze.ndim == 2 else gaze
    if not _on_device(image_of):
        image_of = np.ascontiguousarray(_host_array(image_of)).reshape(-1)
        if image_of.dtype.kind not in 'iu':
            raise TypeError(f'image_of must hold integers, got {image_of.dtype}')
        if len(image_of) and (image_of.min() < 0 or image_of.max() >= frames):
            raise ValueError(f'image_of must lie in [0, {frames}), got [{image_of.min()}, {image_of.max()}]')
        image_of = image_of.astype(np.int32)
    bad_gaze = gaze is not None and (gaze.ndim != 2 or gaze.shape[0] != n or gaze.shape[1] < 2)
    if tuple(boxes.shape) != (n, 4) or bad_gaze or tuple(image_of.shape) != (n,):
        got, want = ('', '') if gaze is None else (f', gaze {tuple(gaze.shape)}', ', [n,>=2]')
        raise ValueError(f'{caller}: boxes {tuple(boxes.shape)}{got} and image_of {tuple(image_of.shape)} must be [n,4]{want} and [n]')
    if n > 65535:
        raise ValueError(f'{caller}: at most 65535 {rows} per call (got {n})')
    return boxes, image_of, gaze, n


def _drawing_checked(who, rows, entry, images, boxes, gaze, image_of, nv12, device):
    """The first of the three steps draw_arrows and draw_attention (``who``; they draw ``rows`` = 'arrows' / 'rows') share: the frames and the
    row tables checked on the host, before anything is cloned, uploaded or launched -> (dev, images, planes, table, boxes, image_of, gaze, n),
    which ``_drawing_placed`` takes inside the call's scope; ``DevicePipeline._drawing_upload`` is the third."""
    dev = _device(device)                                         # the surfaces are checked whatever the device: a bad one is the caller's first error
    images = list(images)
    planes = [_nv12_planes(k, im, dev) for k, im in enumerate(images)] if nv12 else None
    dev = _device(dev, entry.__name__)
    if not len(images):
        raise ValueError(f'{who}: no frames')
    table, _ = _image_table(images, dev, planes)                  # every frame is checked before the first clone or upload
    boxes, image_of, gaze, n = _row_tables(who, rows, len(images), boxes, image_of, gaze)
    for name, t in (('box', boxes), ('gaze', gaze)):
        if isinstance(t, np.ndarray) and not np.isfinite(t).all():
            raise ValueError(f'{who}: {name} {int(np.flatnonzero(~np.isfinite(t).all(axis=1))[0])} is not finite')
    return dev, images, planes, table, boxes, image_of, gaze, n


def _drawing_placed(who, checked, nv12, copy, arrow, lowest):
    """Inside the scope: the tensors that are drawn into and the rows as the kernels read them -> (out, pixels, in_place, table, h_max, w_max,
    boxes, gaze, gaze_stride, image_of).  arrow: ``_arrow_params``' four, with ``lowest`` the least min_thickness they were checked against;
    host rows that cannot be drawn are a ValueError here."""
    dev, images, planes, table, boxes, image_of, gaze, n = checked
    out, pixels, in_place = _arrow_targets(images, planes, copy, dev)
    if not in_place:                                              # the table of the tensors that are drawn into
        table, _ = _image_table(out, dev, [_nv12_planes(k, o, dev) for k, o in enumerate(out)] if nv12 else None)
    h_max, w_max = int(table['h'].max()), int(table['w'].max())
    if h_max > ARROW_SIDE or w_max > ARROW_SIDE:
        raise ValueError(f'{who}: frames of at most {ARROW_SIDE} pixels a side, got {h_max} x {w_max}')
    if isinstance(boxes, np.ndarray) and isinstance(gaze, np.ndarray) and n:
        length, min_thickness, ratio, tip_length = arrow
        _arrow_rows(boxes, gaze, image_of if isinstance(image_of, np.ndarray) else np.zeros(n, np.int32),
                    [(int(r['h']), int(r['w'])) for r in table], True, length=length, min_thickness=min_thickness,
                    thickness_ratio=ratio, tip_length=tip_length, lowest=lowest)
    boxes = boxes if isinstance(boxes, np.ndarray) else boxes.to(dev, torch.float32).contiguous()
    image_of = image_of if isinstance(image_of, np.ndarray) else image_of.to(dev, torch.int32).contiguous()
    gaze, gaze_stride = _gaze_operand(gaze, n, 2, dev)
    return out, pixels, in_place, table, h_max, w_max, boxes, gaze, gaze_stride, image_of


class DevicePipeline:
    """``Compose(cfg.data.test.pipeline)`` (mmdet/datasets/pipelines/compose.py:11-51) whose pixel work is one HIP launch."""

    STAGES = 4
    IMAGE_TABLES = 16                                             # device-resident frame tables kept by head_crops (a decoder's buffer ring recurs)

    def __init__(self, transforms):
        self.transforms = [PIPELINES.build(dict(t)) if isinstance(t, dict) else t for t in transforms]
        kinds = [type(t).__name__ for t in self.transforms]
        if not kinds or kinds[0] != 'LoadImageFromFile':
            raise ValueError('the pipeline must start with LoadImageFromFile')
        if 'Normalize' not in kinds or not any(k in kinds for k in ('DefaultFormatBundle', 'ImageToTensor')) or kinds[-1] != 'Collect':
            raise ValueError(f'unsupported test pipeline {kinds}: need ... Normalize ... DefaultFormatBundle, Collect')
        self.collect = self.transforms[-1]
        self._planners = [t.plan for t in self.transforms if type(t) not in (LoadImageFromFile, DefaultFormatBundle, ImageToTensor, Collect)]   # the rest plan nothing
        self._ring = _StagingRing(self.STAGES)                    # run_many and head_crops upload through the same stages
        self._image_tables = collections.OrderedDict()            # head_crops, draw_arrows, letterbox: (device, table bytes) -> that table on the device
        self._frame_hw_tables = collections.OrderedDict()         # detect_heads: (device, host frame_hw bytes) -> that table on the device
        self._detect_workspaces = collections.OrderedDict()       # detect_heads: (device, B, N) -> scratch of mcg_detect_heads
        self._label_fonts = {}                                    # draw_labels: device -> LABEL_FONT on it
        self._heat_workspaces = collections.OrderedDict()         # gaze_heat: (device, cells) -> scratch of mcg_gaze_heat_add
        self._heat_tables = collections.OrderedDict()             # draw_heat: the ramp per (device, format, matrix), a fixed scale per (device, C, value)
        self._surface_workspaces = collections.OrderedDict()      # surface_heat, draw_surface_heat: (device, bytes) -> the charts and the scratch

    def _kept(self, cache, key, make):
        """cache[key], made the first time it is asked for; the least recently used of IMAGE_TABLES entries goes."""
        t = cache.get(key)
        if t is None:
            t = cache[key] = make()
            while len(cache) > self.IMAGE_TABLES:
                cache.popitem(last=False)
        else:
            cache.move_to_end(key)
        return t

    def _device_table(self, table, dev, *kind):
        """The record table ``table`` on the device: uploaded the first time this content (of this ``kind``) is seen, then found again."""
        return self._kept(self._image_tables, (dev.index, table.tobytes(), *kind), lambda: torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev))

    def _device_image_table(self, table, dev, nv12):
        """The frame table ``table`` on the device -- what lets head_crops and draw_arrows on device frames and tables touch the host nowhere."""
        return self._device_table(table, dev, *(('nv12',) if nv12 else ()))

    def _drawing_upload(self, call, nv12, table, pixels, in_place, tables, empty_is_null=False):
        """The third step of the drawing calls: everything that comes from the host in ONE pinned staging buffer and one copy -- pixels, frame
        table, host tables -- -> the addresses of the frame table and of ``tables`` (None for None; with ``empty_is_null`` for an empty
        table too: the overlay's entry runs without rows or without regions).  The pixels of host frames are copied out of the stage, which
        the next calls reuse, into the tensors handed back."""
        frame_table = table
        if in_place and np.ndarray not in map(type, tables):
            # device frames drawn in place and device tables: only the frame table, and only the first time the frames are seen
            frame_table = self._device_image_table(table, call.dev, nv12)
        if empty_is_null:
            tables = [t if (t.size if isinstance(t, np.ndarray) else t.numel()) else None for t in tables]
        staged, ptrs = call.upload([a for _, a in pixels], (frame_table, *tables))
        for (dst, _), src in zip(pixels, staged):
            dst.copy_(src.view(dst.shape))
        return ptrs

    def plan(self, shape, rng=np.random, filename=None, ori_filename=None):
        p = FramePlan(shape, filename, ori_filename)
        for plan in self._planners:
            plan(p, rng)
        if p.pad_shape is None:
            p.pad_shape = p.img_shape
        if p.scale_factor is None:
            p.scale_factor = 1.0
        return p

    def __call__(self, frames, device='cuda:0', rng=np.random, img_prefix=None, stream=None, loader=None):
        """frames: list of HxWx3 uint8 BGR arrays (cv2 order) or file names.  Returns (img [N,3,Hp,Wp] f32 on `device`,
        img_metas list of N dicts) -- one clip batch, padded to the largest padded frame like mmcv's collate.
        loader: path -> HxWx3 uint8 array (default LoadImageFromFile.load; a FrameCache decodes ahead on host threads)."""
        return self.run_many([frames], device, rng, img_prefix, stream, loader)[0]

    def _load_and_plan(self, windows, rngs, img_prefix, loader, load, rgb_source):
        """-> (arrays, src, plans, bounds).  arrays: the DISTINCT decoded frames of this call (a file named by several windows -- they overlap
        by three frames -- is staged and uploaded once); src[k]: the array the k-th (window, frame) reads; plans stay per (window, frame): every
        use draws its own crop; window wi is rows bounds[wi]:bounds[wi + 1]."""
        arrays, src, plans, bounds, seen = [], [], [], [0], {}
        for frames, rng in zip(windows, rngs):
            for f in frames:
                if isinstance(f, str):
                    path = os.path.join(img_prefix, f) if img_prefix is not None else f
                    k = seen.get(path)
                    if k is None:
                        arr = load(path)
                        if not rgb_source and getattr(loader, 'rgb', False):
                            arr = np.ascontiguousarray(arr[..., ::-1])       # mixed with caller-supplied BGR arrays: one order per call
                        k = seen[path] = len(arrays)
                        arrays.append(arr)
                    arr, names = arrays[k], (path, f)
                else:
                    arr, names = np.ascontiguousarray(f), (None, None)
                    k = len(arrays)
                    arrays.append(arr)
                if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
                    raise TypeError(f'frames must be HxWx3 uint8 arrays, got {arr.dtype} {arr.shape}')
                src.append(k)
                plans.append(self.plan(arr.shape, rng, *names))
            bounds.append(len(src))
        return arrays, src, plans, bounds

    def run_many(self, windows, device='cuda:0', rng=np.random, img_prefix=None, stream=None, loader=None):
        """Several clip batches (windows) through ONE staging copy and one launch per distinct padded size: windows = list of lists
        of frames (arrays or file names) -> list of (img, img_metas), each exactly what ``__call__`` returns for that window -- frames
        are planned window by window, frame by frame, so the RNG draws fall where they do one window at a time; padding is per
        window (mmcv's collate pads a clip to ITS largest frame)."""
        lib, release = L.load(), getattr(loader, 'release', lambda: None)
        dev = _device(device, 'mcg_preprocess_frames')
        rgb_source = all(isinstance(f, str) for w in windows for f in w)      # our own decode: keep PIL's RGB order, the kernel swaps
        if loader is not None:
            load = loader
            rgb_source = rgb_source and bool(getattr(loader, 'rgb', False))
        else:
            load = (lambda path: LoadImageFromFile.load(path, rgb=True)) if rgb_source else LoadImageFromFile.load
        rngs = rng if isinstance(rng, (list, tuple)) else [rng] * len(windows)   # one generator per window (harness: one per VIDEO), or one for all
        if len(rngs) != len(windows):
            raise ValueError(f'run_many: {len(rngs)} generators for {len(windows)} windows')
        try:
            arrays, src, plans, bounds = self._load_and_plan(windows, rngs, img_prefix, loader, load, rgb_source)
            out = [None if bounds[wi + 1] > bounds[wi] else (torch.empty(0, 3, 0, 0, dtype=torch.float32, device=dev), []) for wi in range(len(windows))]
            if not src:
                return out
            groups = {}                                           # padded size -> windows
            for wi in range(len(windows)):
                a, b = bounds[wi], bounds[wi + 1]
                if b > a:
                    pad = (max(p.pad_shape[0] for p in plans[a:b]), max(p.pad_shape[1] for p in plans[a:b]))
                    groups.setdefault(pad, []).append(wi)
            rows = {pad: np.concatenate([np.arange(bounds[wi], bounds[wi + 1]) for wi in wis]) for pad, wis in groups.items()}
            # the frame descriptors (mcg_frame_desc, one structured array per padded size) travel in the same pinned staging buffer, behind the
            # pixels: one non-blocking copy for everything (a pageable .to() per descriptor table blocked the host until the stream had
            # drained -- the engine's previous batch)
            descs = {pad: np.zeros(len(idx), dtype=_DESC) for pad, idx in rows.items()}

            def describe(at):
                release()                                         # ring views of a FrameCache: copied, their slots may go
                addr = np.asarray(at, dtype=np.int64)[src]
                shp = np.asarray([a.shape[:2] for a in arrays], dtype=np.int32)[src]
                geo = np.asarray([p.crop + p.img_shape[:2] for p in plans], dtype=np.int32)          # crop y, x, h, w, out h, w
                for pad, idx in rows.items():
                    desc = descs[pad]
                    desc['src'], desc['src_h'], desc['src_w'], desc['src_pitch'] = addr[idx], shp[idx, 0], shp[idx, 1], shp[idx, 1] * 3
                    for j, f in enumerate(('crop_y', 'crop_x', 'crop_h', 'crop_w', 'out_h', 'out_w')):
                        desc[f] = geo[idx, j]

            with _call_scope(self._ring, dev, stream) as call:
                _, desc_at = call.upload([a.reshape(-1) for a in arrays], list(descs.values()), describe)
                desc_at = dict(zip(descs, desc_at))
                mean, stdinv, swap = _kernel_norm(plans[0].img_norm_cfg, rgb_source)
                for (pad_h, pad_w), wis in groups.items():
                    n = len(rows[pad_h, pad_w])
                    img = torch.empty(n, 3, pad_h, pad_w, dtype=torch.float32, device=dev)
                    L.check(lib.mcg_preprocess_frames(C.c_void_p(call.main.cuda_stream), C.c_void_p(desc_at[pad_h, pad_w]), n, C.c_void_p(img.data_ptr()),
                                                      pad_h, pad_w, mean, stdinv, swap), 'mcg_preprocess_frames')
                    for wi, part in zip(wis, img.split([bounds[wi + 1] - bounds[wi] for wi in wis])):
                        out[wi] = (part, [self.collect.meta(p) for p in plans[bounds[wi]:bounds[wi + 1]]])
            return out
        except BaseException:
            # a TypeError for a non-uint8 frame, a decode error, a staging failure: the ring views handed out so far are not read any more --
            # without this they stayed pinned and a caller that carried on met 'all cached frames are handed out' later
            release()
            raise

    def head_crop_geometry(self):
        """-> (scale_w, scale_h, pad_h, pad_w, img_norm_cfg) of the chain a head crop goes through, which must be the demo's
        ``cfg.data.test.pipeline[1:]``: Resize(keep_ratio=True), no flip, Normalize, Pad -- NotImplementedError for anything else."""
        kinds = [type(t).__name__ for t in self.transforms]
        if 'CenterCrop' in kinds:
            raise NotImplementedError('head_crops: the window comes from the head box; a pipeline with a CenterCrop is not the demo\'s chain')
        resize = next((t for t in self.transforms if isinstance(t, Resize)), None)
        if resize is None or not resize.keep_ratio or resize.img_scale[0] != resize.img_scale[1]:
            raise NotImplementedError('head_crops needs Resize(img_scale=(s, s), keep_ratio=True): a window clipped by the frame border may be '
                                      'upright or lying, and keep_ratio puts the long edge of img_scale on its long side')
        scale_w, scale_h = resize.img_scale
        p = self.plan((scale_h, scale_w, 3), _NO_DRAW)            # the LARGEST resized crop through the planners: its pad_shape holds every crop
        return int(scale_w), int(scale_h), int(p.pad_shape[0]), int(p.pad_shape[1]), p.img_norm_cfg

    def head_crops(self, images, boxes, image_of, expand=0.8, device='cuda:0', stream=None, rgb=False, pixel_format='bgr', matrix='bt601'):
        """Video frames and head boxes -> the model's input, one head crop per box (MCGaze_demo/demo.ipynb, cell 4, then this chain): ONE
        plan launch chooses every window on the device, the pixel kernel reads it (mcg_preprocess_head_crops).

        images: list of HxWx3 uint8 frames in cv2's BGR order (rgb=True: RGB, the kernel swaps either way).  A numpy array is staged and
        uploaded ONCE however many heads it shows; a CUDA uint8 tensor is read where it is (rows stride(0) bytes apart, pixels packed).
        boxes [n,4] f32 x1 y1 x2 y2 in pixels of their frame; image_of [n] int: the frame of each box -- numpy arrays or device tensors.
        Host tables are checked here (ValueError for an image_of out of range, a non-finite box or a window the demo's
        slice leaves empty); device tables are not read back -- such rows come back flagged instead (1: empty window, cut as one pixel
        inside the frame; 2: unusable box / index, pixel (0, 0) of frame 0), and a call on device frames and tables touches the host
        nowhere: it can be captured in a graph once a first call has uploaded the frame table (kept per distinct set of frames).

        -> (img [n,3,Hp,Wp] f32, img_hw [n,2] int32, scale_factor [n,4] f32, crop [n,4] int32 = y0, x0, h, w, flags [n] int32), all on
        the device.  (Hp, Wp) is img_scale rounded up by Pad -- for every call, where mmcv's collate pads a chunk to ITS largest crop (the
        same unless the frame border clips every crop of the chunk on one axis); img_hw is each crop's true resized size, the reference's
        img_shape, and the decoder clips by it.

        pixel_format='nv12': the frames are a video decoder's NV12 surfaces and are read as they are (mcg_preprocess_head_crops_nv12 converts
        each tap it samples; no BGR frame is ever written).  Each image is a (y [H,W], uv [H/2,W/2,2] or [H/2,W]) pair or ONE [3H/2, W] surface
        (the Y rows, then the UV rows), uint8, H and W even: numpy arrays are staged in the same single copy, CUDA tensors are read in place
        (row strides are the pitches, at least W; bytes inside a row are packed).  matrix: 'bt601' (cv2's COLOR_YUV2BGR_NV12 constants) or
        'bt709' (what HD decoders emit), both limited range -- ``YUV_COEF``.  rgb= is ignored: the output order is the config's to_rgb.  TypeError
        / ValueError for a wrong dtype, rank, device or plane shape and for odd sizes, before anything is launched.  The result equals
        head_crops on ``nv12_to_bgr`` of the same planes bit for bit; tables, flags and the no-host-touch property are as for BGR."""
        lib = L.load()
        nv12, coef = _pixel_format(pixel_format, matrix)
        dev = _device(device)                                     # the surfaces are checked whatever the device: a bad one is the caller's first error
        planes = [_nv12_planes(k, im, dev) for k, im in enumerate(images)] if nv12 else None
        dev = _device(dev, 'mcg_preprocess_head_crops')
        scale_w, scale_h, pad_h, pad_w, norm = self.head_crop_geometry()
        if not len(images):
            raise ValueError('head_crops: no frames')
        table, parts = _image_table(images, dev, planes)
        boxes, image_of, _, n = _row_tables('head_crops', 'crops', len(images), boxes, image_of)
        if isinstance(boxes, np.ndarray) and isinstance(image_of, np.ndarray) and n:
            _, empty = head_crop_windows(boxes, table['h'][image_of], table['w'][image_of], expand)
            if empty.any():
                k = int(np.flatnonzero(empty)[0])
                raise ValueError(f'head box {k} {boxes[k].tolist()} leaves an empty window in frame {int(image_of[k])} '
                                 f'({int(table["h"][image_of[k]])} x {int(table["w"][image_of[k]])})')
        with _call_scope(self._ring, dev, stream) as call:
            boxes = boxes if isinstance(boxes, np.ndarray) else boxes.to(dev, torch.float32).contiguous()
            image_of = image_of if isinstance(image_of, np.ndarray) else image_of.to(dev, torch.int32).contiguous()
            new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
            if n == 0:
                return new(0, 3, pad_h, pad_w, dtype=torch.float32), new(0, 2), new(0, 4, dtype=torch.float32), new(0, 4), new(0)
            frame_table = table
            if not parts and isinstance(boxes, torch.Tensor) and isinstance(image_of, torch.Tensor):
                # nothing comes from the host but the frame table, and that only the first time these frames are seen: no stage is taken
                frame_table = self._device_image_table(table, dev, nv12)

            def name_frames(at):                                  # a host frame's address: where its bytes land in the device twin
                for (k, f, _), a in zip(parts, at):
                    table[f][k] = a

            # everything that comes from the host travels in ONE pinned staging buffer and one copy: pixels, frame table, host tables
            _, (images_ptr, boxes_ptr, image_of_ptr) = call.upload([a for _, _, a in parts], (frame_table, boxes, image_of), name_frames)
            img, scale_factor = new(n, 3, pad_h, pad_w, dtype=torch.float32), new(n, 4, dtype=torch.float32)
            desc, img_hw, flags = new(n, _NV12_DESC_WORDS if nv12 else _DESC_WORDS), new(n, 2), new(n)
            vp = C.c_void_p
            entry, more = (lib.mcg_preprocess_head_crops_nv12, (C.byref(L.YuvCoef(**coef)),)) if nv12 else (lib.mcg_preprocess_head_crops, ())
            L.check(entry(vp(call.main.cuda_stream), vp(images_ptr), len(images), vp(boxes_ptr), vp(image_of_ptr), n, float(expand),
                          scale_w, scale_h, vp(desc.data_ptr()), vp(img_hw.data_ptr()), vp(scale_factor.data_ptr()),
                          vp(flags.data_ptr()), vp(img.data_ptr()), pad_h, pad_w, *_kernel_norm(norm, rgb, nv12), *more), entry.__name__)
        return img, img_hw, scale_factor, desc[:, _CROP_WORD:_CROP_WORD + 4], flags

    def draw_arrows(self, images, boxes, gaze, image_of, color=None, pixel_format='bgr', matrix='bt601', copy=False, device='cuda:0', stream=None,
                    **params):
        """The demo's last step (MCGaze_demo/demo.ipynb, cell 5) on the device: one arrow per head, from the head's centre along its gaze, drawn
        into the frames (mcg_draw_gaze_arrows / mcg_draw_gaze_arrows_nv12: a plan launch and a raster launch) -- ``draw_arrows_host`` bit for bit.

        images: as for head_crops -- HxWx3 uint8 frames, or with pixel_format='nv12' (y, uv) pairs / [3H/2, W] surfaces; numpy arrays or CUDA
        tensors.  A CUDA frame is drawn IN PLACE (copy=True: into a packed clone) and handed back as it was given; a numpy frame goes up through the
        staging ring into a fresh device tensor (NV12: one [3H/2, W] surface, handed back as its (y [H,W], uv [H/2,W]) views), which is drawn into.
        boxes [n,4] x1 y1 x2 y2, gaze [n,>=2] (only g0, g1 are read), image_of [n]: numpy arrays or device tensors; an f32 device gaze with packed
        rows -- the [n,3] ``fused`` of a results='device' stream -- is read where it is, its row stride taken from the tensor.
        color: one (B, G, R) triple (None: the demo's (230, 253, 11)) or one per row, [n,3], on the host; for NV12 each is converted once by
        ``bgr_to_yuv(color, matrix)``.  params: length, min_thickness, thickness_ratio, tip_length (the demo's 1.0, 5, 0.01, 0.1).
        Where arrows overlap the highest row wins.  Host tables are checked before anything is launched (ValueError: an image_of out of range, a
        box or gaze that is not finite, an end point beyond +-8191 or a thickness beyond 255; a frame larger than 8192 a side); device tables are
        not read back -- such rows come back with flag 2 and write nothing.  TypeError / ValueError for frames as in head_crops.  With device
        frames drawn in place, device tables and one colour the call touches the host nowhere once a first call has uploaded the frame table (the
        cache head_crops keeps): it can be captured in a graph.
        -> (images on the device, in order; flags [n] int32 on the device: 0 drawn -- possibly no pixel --, 2 unusable)."""
        lib = L.load()
        nv12, _ = _pixel_format(pixel_format, matrix)
        arrow = _arrow_params(**params)
        entry = lib.mcg_draw_gaze_arrows_nv12 if nv12 else lib.mcg_draw_gaze_arrows
        checked = _drawing_checked('draw_arrows', 'arrows', entry, images, boxes, gaze, image_of, nv12, device)
        dev, n = checked[0], checked[-1]
        one, per_row = _arrow_colors(color, n, nv12, matrix)
        with _call_scope(self._ring, dev, stream) as call:
            out, pixels, in_place, table, h_max, w_max, boxes, gaze, gaze_stride, image_of = _drawing_placed('draw_arrows', checked, nv12, copy, arrow, 1)
            images_ptr, boxes_ptr, gaze_ptr, image_of_ptr, colors_ptr = self._drawing_upload(call, nv12, table, pixels, in_place,
                                                                                              (boxes, gaze, image_of, per_row))
            flags = torch.empty(n, dtype=torch.int32, device=dev)
            if n:
                plan = torch.empty(n, _ARROW_WORDS, dtype=torch.int32, device=dev)
                vp = C.c_void_p
                L.check(entry(vp(call.main.cuda_stream), vp(images_ptr), len(out), h_max, w_max, vp(boxes_ptr), vp(gaze_ptr),
                              gaze_stride, vp(image_of_ptr), n, *arrow,
                              None if one is None else (C.c_ubyte * 3)(*[int(v) for v in one]), vp(colors_ptr), vp(plan.data_ptr()),
                              vp(flags.data_ptr())), entry.__name__)
        return out, flags

    def draw_attention(self, images, boxes, gaze, image_of, kind, target, hit, mutual, regions=None, region_image=None, region_period=0,
                       palette=None, line_thickness=2, region_thickness=2, pixel_format='bgr', matrix='bt601', copy=False, device='cuda:0',
                       stream=None, **params):
        """What ``gaze_targets`` found, drawn into the frames on the device (mcg_draw_attention / mcg_draw_attention_nv12: region_active
        cleared, a plan launch, a gather launch) -- ``arrows.draw_attention_host`` bit for bit: the outlines of the regions (palette[6] in a
        picture where a row looks at the region, else palette[5]), a sight line from every head that looks at a head or a region to its hit
        point, and ``draw_arrows``' arrows in palette[4 if mutual else kind].  Higher layers and, inside a layer, higher indices win.

        images, boxes, gaze, image_of, pixel_format, matrix, copy and params (length, min_thickness, thickness_ratio, tip_length) are
        ``draw_arrows``': a CUDA frame is drawn IN PLACE (copy=True: into a packed clone), a numpy frame goes up through the staging ring.
        kind, target, mutual [n] and hit [n,2] are gaze_targets' results; regions, region_image and region_period are what gaze_targets took
        -- [m,4] rectangles, the mixed list of ``attention.region_polygons`` or a ``PolyRegions(xy, start)`` -- on the host or the device.
        palette: [7,3] B, G, R on the host (None: ``arrows.OVERLAY_PALETTE``, a convention), converted once per entry for NV12.  A thickness
        of 0 (line_thickness, region_thickness, min_thickness) switches its layer off.  Host tables are checked before anything is launched
        (TypeError / ValueError as in draw_arrows); device tables are never read back: a row or region that cannot be drawn comes back with
        flag 2 and writes nothing.  With device frames drawn in place, device tables and the frame table cached by a first call, the call
        touches the host nowhere and can be captured in a graph.
        -> (images on the device, in order; flags [n], region_flags [m], region_active [len(images), m]: int32 on the device)."""
        lib = L.load()
        who = 'draw_attention'
        nv12, _ = _pixel_format(pixel_format, matrix)
        arrow = _arrow_params(lowest=0, **params)
        line_thickness, region_thickness = _overlay_thickness(who, line_thickness=line_thickness, region_thickness=region_thickness)
        _, _, period = _target_params(region_period=region_period, who=who)
        pal = _overlay_palette(who, palette, nv12, matrix)
        entry = lib.mcg_draw_attention_nv12 if nv12 else lib.mcg_draw_attention
        checked = _drawing_checked(who, 'rows', entry, images, boxes, gaze, image_of, nv12, device)
        dev, n = checked[0], checked[-1]
        found = (kind, target, hit, mutual)
        if not any(_on_device(t) for t in found):
            found = _overlay_targets(who, n, *found)
        with _call_scope(self._ring, dev, stream) as call:
            _, xy, start, region_image, m, V = _region_operands(who, regions, region_image, dev, as_vertices=True)
            out, pixels, in_place, table, h_max, w_max, boxes, gaze, gaze_stride, image_of = _drawing_placed(who, checked, nv12, copy, arrow, 0)
            if not isinstance(found[0], np.ndarray):              # one of them is on the device: the others are moved with torch
                found = tuple(_there(t, dev, torch.float32 if k == 2 else torch.int32) for k, t in enumerate(found))
                for name, t, shape in zip(('kind', 'target', 'hit', 'mutual'), found, ((n,), (n,), (n, 2), (n,))):
                    if tuple(t.shape) != shape:
                        raise ValueError(f'{who}: {name} must be {list(shape)}, got {tuple(t.shape)}')
            _overlay_counts(who, n, m, V, len(out))
            ptrs = self._drawing_upload(call, nv12, table, pixels, in_place, (boxes, gaze, image_of, *found, xy, start, region_image), empty_is_null=True)
            new = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
            flags, region_flags, region_active = new(n), new(m), new(len(out), m)
            if n or m:
                work = new(24 * (m + 2 * n) + 64 * m)             # the header's formula: (m + 2 n) stroke records, then [m][32][2] vertices
                vp = C.c_void_p
                images_ptr, boxes_ptr, gaze_ptr, image_of_ptr, kind_ptr, target_ptr, hit_ptr, mutual_ptr, xy_ptr, start_ptr, ri_ptr = ptrs
                L.check(entry(vp(call.main.cuda_stream), vp(images_ptr), len(out), h_max, w_max, vp(boxes_ptr), vp(gaze_ptr), gaze_stride,
                              vp(image_of_ptr), n, vp(kind_ptr), vp(target_ptr), vp(hit_ptr), vp(mutual_ptr), vp(xy_ptr), V, vp(start_ptr),
                              vp(ri_ptr), m, period, (C.c_ubyte * 21)(*[int(v) for v in pal.reshape(-1)]), *arrow,
                              line_thickness, region_thickness, vp(work.data_ptr()), 4 * work.numel(), vp(flags.data_ptr()),
                              vp(region_flags.data_ptr()), vp(region_active.data_ptr())), entry.__name__)
        return out, flags, region_flags, region_active

    def format_labels(self, ids, values=None, rate=(30, 1), out=None, device='cuda:0', stream=None):
        """The text of one label per row, made on the device (mcg_format_labels, one launch) -- ``format_labels_host`` bit for bit: '#' and the
        id, and with ``values`` (frames, e.g. gaze_dwell's dwell_frames) the seconds they last at rate = (num, den) frames per second, in
        tenths: '#12 3.4s'.  A row whose id is <= 0 is empty, and draw_labels draws nothing for it.
        ids, values [n] integers: numpy arrays (checked: TypeError / ValueError) or device tensors, which are never read back.  out: a device
        uint8 [n, 24] tensor to write into (a slice of a larger text table), else a new one.  -> the text table uint8 [n, 24] on the device."""
        lib = L.load()
        num, den = _label_rate(rate)
        dev = _device(device, 'mcg_format_labels')
        tables = [None if t is None else t if _on_device(t) else _label_ints(name, t) for name, t in (('ids', ids), ('values', values))]
        n = int(tables[0].shape[0])
        if tables[0].ndim != 1 or (tables[1] is not None and tuple(tables[1].shape) != (n,)) or n > 65535:
            raise ValueError(f'format_labels: ids and values must be [n], n <= 65535; got {tuple(tables[0].shape)} and {None if tables[1] is None else tuple(tables[1].shape)}')
        if out is not None and not (_on_device(out) and out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (n, LABEL_CHARS) and out.is_contiguous()):
            raise ValueError(f'format_labels: out must be a contiguous uint8 [{n}, {LABEL_CHARS}] tensor on {dev}')
        with _call_scope(self._ring, dev, stream) as call:
            tables = [t if t is None or isinstance(t, np.ndarray) else t.to(dev, torch.int32).contiguous() for t in tables]
            _, (ids_ptr, values_ptr) = call.upload([], tables)
            text = torch.empty(n, LABEL_CHARS, dtype=torch.uint8, device=dev) if out is None else out
            if n:
                vp = C.c_void_p
                L.check(lib.mcg_format_labels(vp(call.main.cuda_stream), vp(ids_ptr), vp(values_ptr), n, num, den, vp(text.data_ptr())), 'mcg_format_labels')
        return text

    def draw_labels(self, images, boxes, image_of, text, colors=None, color=None, background=(0, 0, 0), scale=2, advance=6, pad=1, place=None,
                    pixel_format='bgr', matrix='bt601', copy=False, device='cuda:0', stream=None):
        """Words in the frames, on the device (mcg_draw_labels / mcg_draw_labels_nv12: a plan launch and a gather launch) --
        ``arrows.draw_labels_host`` bit for bit: the text of row k (``encode_labels``, ``format_labels``) on a plate of ``background`` above
        the row's box -- below it where there is no room above, inside its top-left corner with place[k] == 1 -- moved inside the frame.

        images, pixel_format, matrix, copy: ``draw_arrows``' -- a CUDA frame is drawn IN PLACE (copy=True: into a packed clone), a numpy frame
        goes up through the staging ring.  boxes [n,4], image_of [n], text uint8 [n,24], place [n] or None, colors [n,3] or None: numpy arrays
        or device tensors.  color: one (B, G, R) triple on the host (None: the arrows' (230, 253, 11)), used where ``colors`` is None; host
        colours are converted once by ``bgr_to_yuv`` for NV12, DEVICE colours are read as they are: (Y, U, V) for NV12.  background: one
        triple, or None for no plates.  scale 1 .. 16 pixels per font bit, advance 1 .. 8 font columns per character, pad 0 .. 8 font bits
        around the text.  The font is ``arrows.LABEL_FONT``, uploaded once per device and kept.  Later rows cover earlier ones.
        Host tables are checked before anything is launched (TypeError / ValueError: an image_of out of range, a box that is not finite or
        beyond +-8191); device tables are never read back -- such rows come back with flag 2 and write nothing.  With device frames drawn in
        place, device tables and the frame table cached by a first call, the call touches the host nowhere and can be captured in a graph.
        -> (images on the device, in order; flags [n] int32 on the device: 0 drawn, 1 an empty label, 2 unusable)."""
        lib = L.load()
        who = 'draw_labels'
        nv12, _ = _pixel_format(pixel_format, matrix)
        scale, advance, pad = _label_params(scale, advance, pad)
        bg = _label_background(background, nv12, matrix)
        entry = lib.mcg_draw_labels_nv12 if nv12 else lib.mcg_draw_labels
        checked = _drawing_checked(who, 'labels', entry, images, boxes, None, image_of, nv12, device)
        dev, n = checked[0], checked[-1]
        one = _arrow_colors(color, 0, nv12, matrix)[0]
        if one is None:
            raise ValueError(f'{who}: color must be one (B, G, R) triple; one per row goes in colors')
        if not _on_device(text):
            text = _label_text(text, n)
        if place is not None and not _on_device(place):
            place = _label_ints('place', place, n)
        if colors is not None and not _on_device(colors):
            colors = _arrow_colors(colors, n, nv12, matrix)[1]
            if colors is None:
                raise ValueError(f'{who}: colors must be one (B, G, R) triple per row, [{n}, 3]')
        with _call_scope(self._ring, dev, stream) as call:
            out, pixels, in_place, table, h_max, w_max, boxes, _, _, image_of = _drawing_placed(who, checked, nv12, copy, None, 0)
            if isinstance(boxes, np.ndarray) and n:
                if isinstance(image_of, np.ndarray):              # the whole plan, against each row's own frame
                    bad = label_plan(boxes, image_of, np.ones((n, LABEL_CHARS), np.uint8), [(int(r['h']), int(r['w'])) for r in table], None, scale,
                                     advance, pad, nv12)['flag'] == 2
                else:                                             # image_of is on the device and is not read back: what does not depend on the frame
                    bad = (np.abs(np.trunc(boxes.astype(np.float64))) > ARROW_COORD).any(axis=1)
                if bad.any():
                    k = int(np.flatnonzero(bad)[0])
                    raise ValueError(f'{who}: label {k} cannot be drawn: box {boxes[k].tolist()} -- a coordinate beyond +-{ARROW_COORD}, or a frame without pixels')
            moved = []
            for name, t, dtype, shape in (('text', text, torch.uint8, (n, LABEL_CHARS)), ('place', place, torch.int32, (n,)), ('colors', colors, torch.uint8, (n, 3))):
                if isinstance(t, torch.Tensor):
                    t = t.to(dev, dtype).contiguous()
                    if tuple(t.shape) != shape:
                        raise ValueError(f'{who}: {name} must be {list(shape)}, got {tuple(t.shape)}')
                moved.append(t)
            images_ptr, boxes_ptr, image_of_ptr, text_ptr, place_ptr, colors_ptr = self._drawing_upload(call, nv12, table, pixels, in_place,
                                                                                                         (boxes, image_of, *moved))
            font = self._label_fonts.get(dev.index)
            if font is None:                                      # the font is data the pipeline brings: uploaded once per device and kept
                font = self._label_fonts[dev.index] = torch.from_numpy(LABEL_FONT.reshape(-1).copy()).to(dev)
            flags = torch.empty(n, dtype=torch.int32, device=dev)
            if n:
                plan = torch.empty(n, _LABEL_WORDS, dtype=torch.int32, device=dev)
                vp, u8 = C.c_void_p, lambda c: None if c is None else (C.c_ubyte * 3)(*[int(v) for v in c])
                L.check(entry(vp(call.main.cuda_stream), vp(images_ptr), len(out), h_max, w_max, vp(boxes_ptr), vp(image_of_ptr), vp(text_ptr),
                              vp(place_ptr), n, vp(font.data_ptr()), scale, advance, pad, u8(one), vp(colors_ptr), u8(bg), vp(plan.data_ptr()),
                              vp(flags.data_ptr())), entry.__name__)
        return out, flags

    def gaze_targets(self, boxes, gaze, image_of, regions=None, region_image=None, region_period=0, expand=0.25, camera_angle=10.0, device='cuda:0',
                     stream=None):
        """What every head looks at, on the device (mcg_gaze_targets: one launch over the rows, one for ``mutual``) -- ``gaze_targets_host`` bit
        for bit, whose arguments and six results these are: the arrow's ray from the head's centre followed to the nearest other head of the
        same picture (its box grown by ``expand`` of its longer side), the nearest marked rectangle, or the lens (a gaze within
        ``camera_angle`` degrees of -z).  Decided in the image plane; the defaults are conventions, not tuned on data.

        boxes [n,4], gaze [n,>=3], image_of [n] (None: one picture): CUDA tensors are read where they are -- an f32 gaze with packed rows, the
        [n,3] ``fused`` of a results='device' stream or a wider table, has its row stride taken from the tensor; other views are made contiguous
        -- and numpy tables go up through the staging ring (a host table next to a device one is moved with torch).  regions [m,4] and
        region_image [m] (None: -1, every picture) likewise; region_period as in the header.  regions may also be the mixed list of
        ``attention.region_polygons`` (rectangles and polygons of 3 .. 32 vertices) or an ``attention.PolyRegions(xy [V,2], start [m+1])`` of
        host or device tables: then the call is mcg_gaze_targets_poly ("gaze targets, polygonal regions"), and what ``start`` holds is
        contents, never an error.  An [m,4] table or a list of 4-number items means rectangles, as ever.  Options and shapes are checked on the host
        before anything is launched (TypeError / ValueError); device tables are not read back: a row that cannot be used comes back with
        flag 2.  With device tables the call touches the host nowhere and can be captured in a graph.
        -> (kind, target [n] int32, t [n] f32, hit [n,2] f32, mutual, flags [n] int32) on the device."""
        lib = L.load()
        who = 'gaze_targets'
        expand, cos2, period = _target_params(expand, camera_angle, region_period, who)
        dev = _device(device, 'mcg_gaze_targets')
        rows_there = any(_on_device(t) for t in (boxes, gaze, image_of))
        if not rows_there:
            boxes, gaze, image_of = _target_rows(who, boxes, gaze, image_of)
        with _call_scope(self._ring, dev, stream) as call:
            # the vertex form is mcg_gaze_targets_poly; anything else is the rectangles [m,4] of mcg_gaze_targets
            poly, table, start, region_image, m, V = _region_operands(who, regions, region_image, dev)
            if rows_there:
                boxes, gaze = _there(boxes, dev, torch.float32), _tensor(gaze)
                n = int(boxes.shape[0])
                if boxes.ndim != 2 or boxes.shape[1] != 4 or gaze.ndim != 2 or gaze.shape[0] != n or gaze.shape[1] < 3:
                    raise ValueError(f'{who}: boxes {tuple(boxes.shape)} and gaze {tuple(gaze.shape)} must be [n,4] and [n,>=3]')
                image_of = torch.zeros(n, dtype=torch.int32, device=dev) if image_of is None else _there(image_of, dev, torch.int32)
                if tuple(image_of.shape) != (n,):
                    raise ValueError(f'{who}: image_of must be [{n}], one per row; got {tuple(image_of.shape)}')
            n = int(boxes.shape[0])
            gaze, gaze_stride = _gaze_operand(gaze, n, 3, dev)
            _check_counts(who, n, m, V)
            new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
            out = (new(n), new(n), new(n, dtype=torch.float32), new(n, 2, dtype=torch.float32), new(n), new(n))
            if n == 0:
                return out
            _, (boxes_ptr, gaze_ptr, image_of_ptr, table_ptr, start_ptr, region_image_ptr) = call.upload(
                [], (boxes, gaze, image_of, table if (V if poly else m) else None, start if m else None, region_image if m else None))
            vp = C.c_void_p
            entry, regions_at = (lib.mcg_gaze_targets_poly, (vp(table_ptr), V, vp(start_ptr), vp(region_image_ptr))) if poly else \
                (lib.mcg_gaze_targets, (vp(table_ptr), vp(region_image_ptr)))
            L.check(entry(vp(call.main.cuda_stream), vp(boxes_ptr), vp(gaze_ptr), gaze_stride, vp(image_of_ptr), n, *regions_at, m, period, expand, cos2,
                          *(vp(t.data_ptr()) for t in out)), entry.__name__)
        return out

    def gaze_targets_3d(self, boxes, gaze, image_of, cam, depth=None, regions=None, region_image=None, region_period=0, cam_period=0, head_size=0.24,
                        frame='eye', expand=0.25, camera_angle=10.0, device='cuda:0', stream=None):
        """What every head looks at, decided in CAMERA SPACE on the device (mcg_gaze_targets_3d: one launch over the rows, one for
        ``mutual``) -- ``gaze_targets_3d_host`` bit for bit, whose arguments and seven results these are: every row is lifted to a point
        with the intrinsics ``cam`` ([fx, fy, cx, cy], or [C,4] with row image_of or image_of % cam_period) and a depth (``depth`` [n] in
        metres where it is finite and positive, else (fx * head_size) / the box's longer side), its gaze becomes a direction there
        (``frame`` 'eye': relative to the line from the lens to the head; 'camera': (-gx, -gy, gz)), heads are boxes around those points
        and regions planar polygons in camera coordinates (``attention.regions_3d`` or a ``PolyRegions3D(xyz [V,3], start [m+1])``).
        head_size 0.24 m, frame, expand and camera_angle are conventions, not tuned on data.

        Host or device tables, as ``gaze_targets`` takes them: CUDA tensors are read where they are, numpy tables go up through the staging
        ring, a host table next to a device one of its group (rows and depth; cam; the region tables) is moved with torch.  Options and
        shapes are checked on the host before anything is launched (TypeError / ValueError); device tables are not read back.  With device
        tables the call touches the host nowhere and can be captured in a graph.
        -> (kind, target [n] int32, t [n] f32, hit [n,2] f32 -- the 3-D point projected to pixels, NaN where it is not in front of the lens
        --, mutual, flags [n] int32, hit3d [n,3] f32) on the device."""
        lib = L.load()
        who = 'gaze_targets_3d'
        expand, cos2, period = _target_params(expand, camera_angle, region_period, who)
        head_size, frame, cam_period = _target3d_params(head_size, frame, cam_period, who)
        dev = _device(device, 'mcg_gaze_targets_3d')
        rows_there = any(_on_device(t) for t in (boxes, gaze, image_of, depth))
        if not rows_there:
            boxes, gaze, image_of = _target_rows(who, boxes, gaze, image_of)
            depth = _depth_table(who, depth, len(boxes))
        if not _on_device(cam):
            cam = _camera_table(who, cam)
        regions_there = any(_on_device(t) for t in ((*regions, region_image) if isinstance(regions, PolyRegions3D) else (region_image,)))
        if not regions_there:
            xyz, start, region_image = _poly3d_tables(who, regions, region_image)
        elif regions is None:
            raise ValueError(f'{who}: region_image without regions')
        elif not isinstance(regions, PolyRegions3D):
            regions = regions_3d(regions)
        with _call_scope(self._ring, dev, stream) as call:
            if _on_device(cam):
                cam = _there(cam, dev, torch.float32)
                cam = cam.view(1, 4) if tuple(cam.shape) == (4,) else cam
                if cam.ndim != 2 or cam.shape[1] != 4 or not 1 <= cam.shape[0] <= MAX_CAMERAS:
                    raise ValueError(f'{who}: the camera table is [fx, fy, cx, cy] or [C, 4] with C in 1 .. {MAX_CAMERAS}, got {tuple(cam.shape)}')
            if regions_there:
                xyz, start = _there(regions.xyz, dev, torch.float32), _there(regions.start, dev, torch.int32)
                if xyz.ndim != 2 or xyz.shape[1] != 3 or start.ndim != 1 or start.shape[0] < 1:
                    raise ValueError(f'{who}: PolyRegions3D is xyz [V, 3] and start [m + 1], got {tuple(xyz.shape)} and {tuple(start.shape)}')
                m = int(start.shape[0]) - 1
                region_image = torch.full((m,), -1, dtype=torch.int32, device=dev) if region_image is None else _there(region_image, dev, torch.int32)
                if tuple(region_image.shape) != (m,):
                    raise ValueError(f'{who}: region_image must be [{m}], one per region; got {tuple(region_image.shape)}')
            m, V = int(region_image.shape[0]), int(xyz.shape[0])
            if rows_there:
                boxes, gaze = _there(boxes, dev, torch.float32), _tensor(gaze)
                n = int(boxes.shape[0])
                if boxes.ndim != 2 or boxes.shape[1] != 4 or gaze.ndim != 2 or gaze.shape[0] != n or gaze.shape[1] < 3:
                    raise ValueError(f'{who}: boxes {tuple(boxes.shape)} and gaze {tuple(gaze.shape)} must be [n,4] and [n,>=3]')
                image_of = torch.zeros(n, dtype=torch.int32, device=dev) if image_of is None else _there(image_of, dev, torch.int32)
                if tuple(image_of.shape) != (n,):
                    raise ValueError(f'{who}: image_of must be [{n}], one per row; got {tuple(image_of.shape)}')
                if depth is not None:
                    depth = _there(depth, dev, torch.float32)
                    if tuple(depth.shape) != (n,):
                        raise ValueError(f'{who}: depth must be [{n}], one per row; got {tuple(depth.shape)}')
            n = int(boxes.shape[0])
            gaze, gaze_stride = _gaze_operand(gaze, n, 3, dev)
            _check_counts(who, n, m, V)
            new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
            out = (new(n), new(n), new(n, dtype=torch.float32), new(n, 2, dtype=torch.float32), new(n), new(n), new(n, 3, dtype=torch.float32))
            if n == 0:
                return out
            _, (boxes_ptr, gaze_ptr, image_of_ptr, depth_ptr, cam_ptr, xyz_ptr, start_ptr, region_image_ptr) = call.upload(
                [], (boxes, gaze, image_of, depth, cam, xyz if V else None, start if m else None, region_image if m else None))
            vp = C.c_void_p
            L.check(lib.mcg_gaze_targets_3d(vp(call.main.cuda_stream), vp(boxes_ptr), vp(gaze_ptr), gaze_stride, vp(image_of_ptr), n, vp(cam_ptr),
                                            int(cam.shape[0]), cam_period, vp(depth_ptr), head_size, frame, vp(xyz_ptr), V, vp(start_ptr),
                                            vp(region_image_ptr), m, period, expand, cos2, *(vp(t.data_ptr()) for t in out)), 'mcg_gaze_targets_3d')
        return out

    def dwell_state(self, columns, device='cuda:0'):
        """The empty state of ``gaze_dwell`` for that many columns: int32 [columns, 16] zeros on the device (attention.STATE_WORDS)."""
        _dwell_counts('dwell_state', 0, int(columns), 0, 0)
        return torch.zeros(int(columns), 16, dtype=torch.int32, device=_device(device, 'mcg_gaze_dwell'))

    def gaze_dwell(self, person, kind, ident, mutual, tag=None, state=None, frame0=0, enter=DWELL_ENTER, exit=DWELL_EXIT, region_frames=None,
                   max_events=None, device='cuda:0', stream=None):
        """How long each person looks at what, on the device (mcg_gaze_dwell: one launch that walks the frames, one thread per column, and one
        that compacts the ended episodes) -- ``gaze_dwell_host`` bit for bit, whose arguments and six results these are: the per-frame targets
        of F frames of R columns become debounced episodes (``enter`` frames to become the current target, ``exit`` frames of grace; the
        defaults are conventions, not tuned on data), and every region collects its raw person-frames.

        person, kind, ident, mutual, tag [F, R] integers: CUDA tensors are read where they are (anything but contiguous int32 is converted on the
        device); numpy tables go up through the staging ring (a host table next to a device one is moved with torch).  state: an int32
        [R, 16] tensor on the device, which the call UPDATES IN PLACE and hands back; None allocates the empty one (``dwell_state``).
        region_frames: an int32 [M] tensor on the device, ACCUMULATED IN PLACE and handed back; None: no regions.  max_events: the rows of
        the event table (None: F * R, which always suffices).  Options and shapes are checked on the host before anything is launched
        (TypeError / ValueError); the tables are never read back.  With device tables, a given state and given region_frames the call touches
        the host nowhere and can be captured in a graph.
        -> (dwell [F, R, 4], ended [F, R, 8], events [max_events, 10] (rows behind the count zero), num_events [1], state [R, 16],
        region_frames [M]), int32 on the device."""
        lib = L.load()
        who = 'gaze_dwell'
        enter, exit, frame0 = _dwell_params(enter, exit, frame0, who)
        dev = _device(device, 'mcg_gaze_dwell')
        tables = (person, kind, ident, mutual, tag)
        there = any(isinstance(t, torch.Tensor) and t.is_cuda for t in tables)
        if not there:
            tables = _dwell_tables(who, *tables)
            F, R = tables[0].shape
            if tag is None:
                tables[4] = None                                  # a null pointer: all zero
        for name, t, shape in (('state', state, (None, 16)), ('region_frames', region_frames, (None,))):
            if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int32 and t.is_contiguous() and
                                      t.ndim == len(shape) and tuple(t.shape[1:]) == shape[1:]):
                raise TypeError(f'{who}: {name} is a contiguous int32 {list(shape)} tensor on {dev} (it is updated in place)')
        with _call_scope(self._ring, dev, stream) as call:
            if there:
                moved = []
                for name, t in zip(('person', 'kind', 'ident', 'mutual', 'tag'), tables):
                    if t is not None:
                        t = t if isinstance(t, torch.Tensor) else _tensor(t)
                        if t.dtype.is_floating_point or t.dtype.is_complex:
                            raise TypeError(f'{who}: {name} must hold integers, got {t.dtype}')
                        t = t.to(dev, torch.int32).contiguous()
                        if t.ndim != 2 or (moved and tuple(t.shape) != tuple(moved[0].shape)):
                            raise ValueError(f'{who}: person, kind, ident, mutual and tag are [F, R] tables of one shape; {name} is {tuple(t.shape)}')
                    moved.append(t)
                tables = moved
                F, R = (int(v) for v in tables[0].shape)
            M = 0 if region_frames is None else int(region_frames.shape[0])
            E = _dwell_counts(who, F, R, M, max_events)
            if state is not None and int(state.shape[0]) != R:
                raise ValueError(f'{who}: the state of {R} columns is [{R}, 16], got {tuple(state.shape)}')
            if state is None:
                state = torch.zeros(R, 16, dtype=torch.int32, device=dev)
            if region_frames is None:
                region_frames = torch.zeros(0, dtype=torch.int32, device=dev)
            new = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
            dwell, ended, events, num = new(F, R, 4), new(F, R, 8), torch.zeros(E, 10, dtype=torch.int32, device=dev), \
                torch.zeros(1, dtype=torch.int32, device=dev)
            if F == 0:
                return dwell, ended, events, num, state, region_frames
            _, ptrs = call.upload([], tuple(tables))
            ptrs = [ptrs[k] for k in (0, 4, 1, 2, 3)]             # the entry takes the tag behind the person
            vp = C.c_void_p
            # max_events = 0 still counts: the launch needs a table address and writes no row of it
            L.check(lib.mcg_gaze_dwell(vp(call.main.cuda_stream), *(vp(p) for p in ptrs), F, R, frame0, enter, exit, vp(state.data_ptr()),
                                       vp(region_frames.data_ptr() if M else None), M, vp(dwell.data_ptr()), vp(ended.data_ptr()),
                                       vp(events.data_ptr() if E else num.data_ptr()), E, vp(num.data_ptr())), 'mcg_gaze_dwell')
        return dwell, ended, events, num, state, region_frames

    def heat_state(self, cameras, frame_hw, cell=8, device='cuda:0'):
        """The empty state of ``gaze_heat`` for ``cameras`` cameras of h x w frames: HeatState(heat int32 [cameras, ceil(h / cell),
        ceil(w / cell)] zeros, peak int32 [cameras] zeros, cell_shift) on the device.  cell: the side of a cell in pixels, a power of two in
        1 .. 64 (ValueError)."""
        shift = _heat_cell('heat_state', cell)
        cams, GH, GW = _heat_grid('heat_state', (int(cameras), *heat_grid_shape(frame_hw, cell)))
        dev = _device(device, 'mcg_gaze_heat_add')
        return HeatState(torch.zeros(cams, GH, GW, dtype=torch.int32, device=dev), torch.zeros(cams, dtype=torch.int32, device=dev), shift)

    def _heat_state(self, who, state, dev):
        """``state`` as gaze_heat and draw_heat take it, checked (TypeError / ValueError) -> (cams, GH, GW)."""
        if not (isinstance(state, HeatState) and all(isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int32 and t.is_contiguous()
                                                     for t in state[:2])):
            raise TypeError(f'{who}: state is a HeatState of contiguous int32 tensors on {dev} (heat_state makes it; it is updated in place)')
        cams, GH, GW = _heat_grid(who, tuple(state.heat.shape))
        if tuple(state.peak.shape) != (cams,):
            raise ValueError(f'{who}: the peak of {cams} cameras is [{cams}], got {tuple(state.peak.shape)}')
        _heat_params(who, state.cell_shift, 0, 0, 0, 0)
        return cams, GH, GW

    def gaze_heat(self, hit, kind, image_of, state, flags=None, mask=None, radius=2, kinds=HEAT_KINDS, period=0, decay=0, device='cuda:0', stream=None):
        """Where looks land, accumulated on the device (mcg_gaze_heat_add: the workspace cleared, a scatter with integer atomics, a per-cell
        pass) -- ``attention.gaze_heat_host`` bit for bit: every row that counts adds a pyramid of (radius + 1 - |dx|) (radius + 1 - |dy|)
        around the cell of its hit point to the grid of its camera (image_of, or image_of % period).

        hit [n,2], kind, image_of [n] -- gaze_targets' results and its image_of --, flags / mask [n] or None (a row counts where its flag is
        0 and its mask is not): CUDA tensors are read where they are, numpy tables go up through the staging ring (a host table next to a
        device one is moved with torch).  state: ``heat_state``'s, UPDATED IN PLACE: heat decays by h >> decay once per call (0: off), gains
        the taps and saturates at 2^31 - 1; peak becomes each camera's maximum.  kinds: the kinds of target that count, names out of
        ('none', 'head', 'region', 'camera') or the bit mask.  Options and shapes are checked on the host before anything is launched
        (TypeError / ValueError); what the tables hold is never an error and is never read back.  With device tables the call touches the
        host nowhere once a first call has allocated the workspace, and can be captured in a graph.
        -> state."""
        lib = L.load()
        who = 'gaze_heat'
        dev = _device(device, 'mcg_gaze_heat_add')
        cams, GH, GW = self._heat_state(who, state, dev)
        shift, radius, kinds, period, decay = _heat_params(who, state.cell_shift, radius, kinds, period, decay)
        tables = [('hit', hit, torch.float32), ('kind', kind, torch.int32), ('image_of', image_of, torch.int32), ('flags', flags, torch.int32),
                  ('mask', mask, torch.int32)]
        there = any(_on_device(t) for _, t, _ in tables)
        if not there:                                             # all on the host: checked here, staged below
            host = []
            for name, t, dtype in tables:
                if t is None:
                    host.append(None)
                    continue
                a = np.asarray(_host_array(t))
                if name != 'hit' and a.size and a.dtype.kind not in 'iub':
                    raise TypeError(f'{who}: {name} must hold integers, got {a.dtype}')
                host.append(np.ascontiguousarray(a.reshape(-1, 2) if name == 'hit' else a.reshape(-1), dtype=np.float32 if name == 'hit' else np.int32))
        with _call_scope(self._ring, dev, stream) as call:
            moved = [None if t is None else _there(t, dev, dtype) for _, t, dtype in tables] if there else host
            if moved[0] is None or moved[1] is None or moved[2] is None:
                raise ValueError(f'{who}: hit, kind and image_of are required')
            n = int(moved[0].shape[0])
            for (name, _, _), t in zip(tables, moved):
                if t is not None and tuple(t.shape) != ((n, 2) if name == 'hit' else (n,)):
                    raise ValueError(f'{who}: {name} must be {[n, 2] if name == "hit" else [n]}, got {tuple(t.shape)}')
            if n > 65536:
                raise ValueError(f'{who}: at most 65536 rows per call (got {n})')
            work = self._kept(self._heat_workspaces, (dev.index, cams * GH * GW), lambda: torch.empty(cams * GH * GW, dtype=torch.int32, device=dev))
            _, ptrs = call.upload([], [t if t is None or (t.size if isinstance(t, np.ndarray) else t.numel()) else None for t in moved])
            vp = C.c_void_p
            L.check(lib.mcg_gaze_heat_add(vp(call.main.cuda_stream), *(vp(p) for p in ptrs), n, vp(state.heat.data_ptr()), vp(state.peak.data_ptr()), cams, GH,
                                          GW, shift, radius, kinds, period, decay, vp(work.data_ptr()), 4 * work.numel()), 'mcg_gaze_heat_add')
        return state

    def draw_heat(self, images, state, period=0, lut=None, full_scale=None, min_level=1, pixel_format='bgr', matrix='bt601', copy=False, device='cuda:0',
                  stream=None):
        """The heat map blended into the frames on the device (mcg_draw_heat / mcg_draw_heat_nv12: one launch over every pixel) --
        ``arrows.draw_heat_host`` bit for bit: picture p shows the grid of camera p (with a period: p % period), every pixel's level
        interpolated between cell centres and scaled so that ``full_scale`` is level 255, coloured by ``lut`` and blended with its alpha.

        images, pixel_format, matrix, copy: ``draw_arrows``' -- a CUDA frame is drawn IN PLACE (copy=True: into a packed clone), a numpy frame
        goes up through the staging ring.  state: gaze_heat's.  full_scale: None -- ``state.peak``, each camera's own maximum, read on the
        device -- or an int, the same fixed scale for every camera (a device table filled with it is kept).  lut: [256, 4] (B, G, R, alpha)
        per level on the host (None: ``arrows.HEAT_LUT``, kept on the device), converted once by ``bgr_to_yuv`` for NV12; a uint8 [256, 4]
        DEVICE tensor is read as it is, (Y, U, V, alpha) for NV12.  A pixel below min_level (1 .. 255) keeps its bytes.  A picture whose
        camera has no grid is handed back untouched.  With device frames drawn in place and the frame table cached by a first call, the
        call touches the host nowhere and can be captured in a graph.
        -> the images on the device, in order."""
        lib = L.load()
        who = 'draw_heat'
        nv12, _ = _pixel_format(pixel_format, matrix)
        full_scale, min_level = _heat_scale(who, full_scale, min_level)
        _heat_params(who, 0, 0, 0, period, 0)
        entry = lib.mcg_draw_heat_nv12 if nv12 else lib.mcg_draw_heat
        dev = _device(device)                                     # the surfaces are checked whatever the device: a bad one is the caller's first error
        images = list(images)
        planes = [_nv12_planes(k, im, dev) for k, im in enumerate(images)] if nv12 else None
        dev = _device(dev, entry.__name__)
        if not len(images):
            raise ValueError(f'{who}: no frames')
        table, _ = _image_table(images, dev, planes)              # every frame is checked before the first clone or upload
        cams, GH, GW = self._heat_state(who, state, dev)
        if _on_device(lut):
            if not (lut.device == dev and lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 4) and lut.is_contiguous()):
                raise TypeError(f'{who}: a device lut is a contiguous uint8 [256, 4] tensor on {dev}')
        elif lut is not None:
            lut = heat_lut(lut, nv12, matrix)                     # a host table: checked, converted, staged with the call
        with _call_scope(self._ring, dev, stream) as call:
            out, pixels, in_place = _arrow_targets(images, planes, copy, dev)
            if not in_place:                                      # the table of the tensors that are drawn into
                table, _ = _image_table(out, dev, [_nv12_planes(k, o, dev) for k, o in enumerate(out)] if nv12 else None)
            h_max, w_max = int(table['h'].max()), int(table['w'].max())
            if h_max > ARROW_SIDE or w_max > ARROW_SIDE:
                raise ValueError(f'{who}: frames of at most {ARROW_SIDE} pixels a side, got {h_max} x {w_max}')
            if lut is None:                                       # the ramp is data the pipeline brings: uploaded once per device and format, and kept
                lut = self._kept(self._heat_tables, (dev.index, 'lut', nv12, matrix), lambda: torch.from_numpy(heat_lut(None, nv12, matrix).copy()).to(dev))
            full = state.peak if full_scale is None else self._kept(self._heat_tables, (dev.index, 'full', cams, full_scale),
                                                                     lambda: torch.full((cams,), full_scale, dtype=torch.int32, device=dev))
            images_ptr, lut_ptr = self._drawing_upload(call, nv12, table, pixels, in_place, (lut,))
            vp = C.c_void_p
            L.check(entry(vp(call.main.cuda_stream), vp(images_ptr), len(out), h_max, w_max, vp(state.heat.data_ptr()), vp(full.data_ptr()), cams, GH, GW,
                          state.cell_shift, int(period), vp(lut_ptr), min_level), entry.__name__)
        return out

    def surface_heat_state(self, num_regions, grid=SURFACE_GRID, device='cuda:0'):
        """The empty state of ``surface_heat`` for ``num_regions`` planar regions: SurfaceHeatState(heat int32 [num_regions, GH, GW] zeros,
        peak int32 [num_regions] zeros) on the device.  grid: (GW, GH) cells over each region's chart, 1 .. 1024 a side (ValueError); the
        default of 32 x 32 is a convention, not tuned on data."""
        GW, GH = _surface_grid_option('surface_heat_state', grid)
        M, GH, GW = _surface_grid('surface_heat_state', (int(num_regions), GH, GW))
        dev = _device(device, 'mcg_surface_heat_add')
        return SurfaceHeatState(torch.zeros(M, GH, GW, dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.int32, device=dev))

    def _surface_state(self, who, state, dev):
        """``state`` as surface_heat and draw_surface_heat take it, checked (TypeError / ValueError) -> (M, GH, GW)."""
        if not (isinstance(state, SurfaceHeatState) and all(isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int32 and t.is_contiguous()
                                                            for t in state)):
            raise TypeError(f'{who}: state is a SurfaceHeatState of contiguous int32 tensors on {dev} (surface_heat_state makes it; it is updated in place)')
        M, GH, GW = _surface_grid(who, tuple(state.heat.shape))
        if tuple(state.peak.shape) != (M,):
            raise ValueError(f'{who}: the peak of {M} regions is [{M}], got {tuple(state.peak.shape)}')
        return M, GH, GW

    @staticmethod
    def _surface_region_tables(who, regions, region_image, M, dev, with_image):
        """The region tables of the surface entries -> (xyz, start, region_image or None, V): all on the host (checked numpy arrays, which
        go up through the staging ring) or, with one of them on the device, tensors on ``dev`` (only their shapes are checked).  The call
        is made inside the call's scope and first there."""
        if regions is None:
            raise ValueError(f'{who}: regions are required: the list of regions_3d or a PolyRegions3D')
        there = any(_on_device(t) for t in ((*regions, region_image) if isinstance(regions, PolyRegions3D) else (region_image,)))
        if not there:
            xyz, start, region_image = _poly3d_tables(who, regions, region_image)
        else:
            if not isinstance(regions, PolyRegions3D):
                regions = regions_3d(regions)
            xyz, start = _there(regions.xyz, dev, torch.float32), _there(regions.start, dev, torch.int32)
            if xyz.ndim != 2 or xyz.shape[1] != 3 or start.ndim != 1 or start.shape[0] < 1:
                raise ValueError(f'{who}: PolyRegions3D is xyz [V, 3] and start [m + 1], got {tuple(xyz.shape)} and {tuple(start.shape)}')
            m = int(start.shape[0]) - 1
            if with_image:
                region_image = torch.full((m,), -1, dtype=torch.int32, device=dev) if region_image is None else _there(region_image, dev, torch.int32)
                if tuple(region_image.shape) != (m,):
                    raise ValueError(f'{who}: region_image must be [{m}], one per region; got {tuple(region_image.shape)}')
        if int(start.shape[0]) - 1 != M:
            raise ValueError(f'{who}: the state holds {M} grids for {int(start.shape[0]) - 1} regions')
        _check_counts(who, 0, M, int(xyz.shape[0]))
        return xyz, start, (region_image if with_image else None), int(xyz.shape[0])

    def _surface_workspace(self, dev, nbytes):
        """The workspace of the surface entries: the charts and, for surface_heat, the scratch grid -- kept per device and size."""
        return self._kept(self._surface_workspaces, (dev.index, nbytes), lambda: torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev))

    def surface_heat(self, hit3d, kind, target, regions, state, flags=None, mask=None, radius=SURFACE_RADIUS, decay=0, device='cuda:0', stream=None):
        """Where ON a planar region looks land, accumulated on the device (mcg_surface_heat_add: the charts planned, the workspace cleared,
        a scatter with integer atomics, a per-cell pass) -- ``attention.surface_heat_host`` bit for bit: every row that looks at a region
        (kind 2) has its 3-D hit point taken into that region's chart -- the bounding rectangle of the polygon in the frame of its first
        edge and the normal, stretched over the grid -- and adds a pyramid of (radius + 1 - |dx|) (radius + 1 - |dy|) around its cell to
        the region's grid.  The grid is in the surface's own coordinates: it does not move when the camera does.

        hit3d [n,3], kind, target [n] -- gaze_targets_3d's results --, flags / mask [n] or None (a row counts where its flag is 0 and its
        mask is not): CUDA tensors are read where they are, numpy tables go up through the staging ring (a host table next to a device one
        is moved with torch).  regions: the list of ``regions_3d`` or a PolyRegions3D, host or device, in camera coordinates -- the
        regions gaze_targets_3d searched.  state: ``surface_heat_state``'s, UPDATED IN PLACE: heat decays by h >> decay once per call (0:
        off), gains the taps and saturates at 2^31 - 1; peak becomes each region's maximum.  radius 1 is a convention, not tuned on data.
        Options and shapes are checked on the host before anything is launched (TypeError / ValueError); what the tables hold is never an
        error and is never read back.  With device tables the call touches the host nowhere once a first call has allocated the workspace,
        and can be captured in a graph.
        -> state."""
        lib = L.load()
        who = 'surface_heat'
        dev = _device(device, 'mcg_surface_heat_add')
        M, GH, GW = self._surface_state(who, state, dev)
        radius, decay = _surface_params(who, radius, decay)
        tables = [('hit3d', hit3d, torch.float32), ('kind', kind, torch.int32), ('target', target, torch.int32), ('flags', flags, torch.int32),
                  ('mask', mask, torch.int32)]
        there = any(_on_device(t) for _, t, _ in tables)
        if not there:                                             # all on the host: checked here, staged below
            host = []
            for name, t, dtype in tables:
                if t is None:
                    host.append(None)
                    continue
                a = np.asarray(_host_array(t))
                if name != 'hit3d' and a.size and a.dtype.kind not in 'iub':
                    raise TypeError(f'{who}: {name} must hold integers, got {a.dtype}')
                host.append(np.ascontiguousarray(a.reshape(-1, 3) if name == 'hit3d' else a.reshape(-1), dtype=np.float32 if name == 'hit3d' else np.int32))
        with _call_scope(self._ring, dev, stream) as call:
            xyz, start, _, V = self._surface_region_tables(who, regions, None, M, dev, False)
            moved = [None if t is None else _there(t, dev, dtype) for _, t, dtype in tables] if there else host
            if moved[0] is None or moved[1] is None or moved[2] is None:
                raise ValueError(f'{who}: hit3d, kind and target are required')
            n = int(moved[0].shape[0])
            for (name, _, _), t in zip(tables, moved):
                if t is not None and tuple(t.shape) != ((n, 3) if name == 'hit3d' else (n,)):
                    raise ValueError(f'{who}: {name} must be {[n, 3] if name == "hit3d" else [n]}, got {tuple(t.shape)}')
            if n > 65536:
                raise ValueError(f'{who}: at most 65536 rows per call (got {n})')
            work = self._surface_workspace(dev, L.SURFACE_CHART_BYTES * M + 4 * M * GH * GW)
            empty = lambda t: t is None or not (t.size if isinstance(t, np.ndarray) else t.numel())
            _, ptrs = call.upload([], [None if empty(t) else t for t in moved] + [None if empty(xyz) else xyz, start])
            vp = C.c_void_p
            L.check(lib.mcg_surface_heat_add(vp(call.main.cuda_stream), *(vp(p) for p in ptrs[:5]), n, vp(ptrs[5]), V, vp(ptrs[6]), M,
                                             vp(state.heat.data_ptr()), vp(state.peak.data_ptr()), GH, GW, radius, decay, vp(work.data_ptr()),
                                             8 * work.numel()), 'mcg_surface_heat_add')
        return state

    def draw_surface_heat(self, images, state, cam, regions, region_image=None, region_period=0, cam_period=0, lut=None, full_scale=None, min_level=1,
                          pixel_format='bgr', matrix='bt601', copy=False, device='cuda:0', stream=None):
        """The surface heat maps drawn back onto their regions on the device, with the right perspective (mcg_draw_surface_heat /
        mcg_draw_surface_heat_nv12: the charts planned, then one launch over every pixel) -- ``arrows.draw_surface_heat_host`` bit for
        bit: every pixel's ray through the lens (``cam`` [fx, fy, cx, cy], or [C,4] with row p or p % cam_period for picture p) meets the
        nearest region that covers it, the pixel's level is interpolated between the cell centres of that region's grid and scaled so that
        ``full_scale`` is level 255, coloured by ``lut`` and blended with its alpha.

        images, pixel_format, matrix, copy, lut, full_scale, min_level: ``draw_heat``'s, staging and in-place rule included; full_scale
        None is ``state.peak``, each region's own maximum, read on the device.  state: surface_heat's.  regions: the list of
        ``regions_3d`` or a PolyRegions3D in camera coordinates; region_image [M] (None: every picture) and region_period as gaze_targets
        takes them, with the picture's index in image_of's place.  cam, regions and region_image may be host or device tables; device
        tables are read where they are.  A picture whose camera is missing or not finite is handed back untouched.  With device frames drawn
        in place, device tables and the frame table cached by a first call, the call touches the host nowhere and can be captured in a graph.
        -> the images on the device, in order."""
        lib = L.load()
        who = 'draw_surface_heat'
        nv12, _ = _pixel_format(pixel_format, matrix)
        full_scale, min_level = _heat_scale(who, full_scale, min_level)
        _, _, region_period = _target_params(0.0, None, region_period, who)
        _, _, cam_period = _target3d_params(0.24, 'eye', cam_period, who)
        entry = lib.mcg_draw_surface_heat_nv12 if nv12 else lib.mcg_draw_surface_heat
        dev = _device(device)                                     # the surfaces are checked whatever the device: a bad one is the caller's first error
        images = list(images)
        planes = [_nv12_planes(k, im, dev) for k, im in enumerate(images)] if nv12 else None
        dev = _device(dev, entry.__name__)
        if not len(images):
            raise ValueError(f'{who}: no frames')
        table, _ = _image_table(images, dev, planes)              # every frame is checked before the first clone or upload
        M, GH, GW = self._surface_state(who, state, dev)
        if not _on_device(cam):
            cam = _camera_table(who, cam)
        if _on_device(lut):
            if not (lut.device == dev and lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 4) and lut.is_contiguous()):
                raise TypeError(f'{who}: a device lut is a contiguous uint8 [256, 4] tensor on {dev}')
        elif lut is not None:
            lut = heat_lut(lut, nv12, matrix)                     # a host table: checked, converted, staged with the call
        with _call_scope(self._ring, dev, stream) as call:
            xyz, start, region_image, V = self._surface_region_tables(who, regions, region_image, M, dev, True)
            if _on_device(cam):
                cam = _there(cam, dev, torch.float32)
                cam = cam.view(1, 4) if tuple(cam.shape) == (4,) else cam
                if cam.ndim != 2 or cam.shape[1] != 4 or not 1 <= cam.shape[0] <= MAX_CAMERAS:
                    raise ValueError(f'{who}: the camera table is [fx, fy, cx, cy] or [C, 4] with C in 1 .. {MAX_CAMERAS}, got {tuple(cam.shape)}')
            out, pixels, in_place = _arrow_targets(images, planes, copy, dev)
            if not in_place:                                      # the table of the tensors that are drawn into
                table, _ = _image_table(out, dev, [_nv12_planes(k, o, dev) for k, o in enumerate(out)] if nv12 else None)
            h_max, w_max = int(table['h'].max()), int(table['w'].max())
            if h_max > ARROW_SIDE or w_max > ARROW_SIDE:
                raise ValueError(f'{who}: frames of at most {ARROW_SIDE} pixels a side, got {h_max} x {w_max}')
            if lut is None:                                       # the ramp is data the pipeline brings: uploaded once per device and format, and kept
                lut = self._kept(self._heat_tables, (dev.index, 'lut', nv12, matrix), lambda: torch.from_numpy(heat_lut(None, nv12, matrix).copy()).to(dev))
            full = state.peak if full_scale is None else self._kept(self._heat_tables, (dev.index, 'full', M, full_scale),
                                                                     lambda: torch.full((M,), full_scale, dtype=torch.int32, device=dev))
            work = self._surface_workspace(dev, L.SURFACE_CHART_BYTES * M)
            empty = lambda t: not (t.size if isinstance(t, np.ndarray) else t.numel())
            images_ptr, lut_ptr, cam_ptr, xyz_ptr, start_ptr, ri_ptr = self._drawing_upload(
                call, nv12, table, pixels, in_place, (lut, cam, None if empty(xyz) else xyz, start, region_image))
            vp = C.c_void_p
            L.check(entry(vp(call.main.cuda_stream), vp(images_ptr), len(out), h_max, w_max, vp(cam_ptr), int(cam.shape[0]), cam_period, vp(xyz_ptr), V,
                          vp(start_ptr), vp(ri_ptr), M, region_period, vp(state.heat.data_ptr()), vp(full.data_ptr()), GH, GW, vp(lut_ptr), min_level,
                          vp(work.data_ptr()), 8 * work.numel()), entry.__name__)
        return out

    def anonymize_heads(self, images, boxes, image_of, expand=0.125, shape='ellipse', cell=None, blocks=8, mode='mosaic', color=(0, 0, 0),
                        pixel_format='bgr', matrix='bt601', copy=False, device='cuda:0', stream=None):
        """The faces under the head boxes removed from the frames on the device (mcg_anonymize_heads / mcg_anonymize_heads_nv12: a plan launch
        and a render launch over the tiles under heads) -- ``arrows.anonymize_heads_host`` bit for bit: every pixel of the ellipse inscribed in
        the grown box (shape='box': of the box) becomes the mean of a coarse cell of the frame, or ``color`` with mode='fill'.  Call it after
        ``head_crops`` has read the frames and before anything is drawn on top.  It hides the heads it is GIVEN: a head the detector missed
        stays visible.

        images, pixel_format, matrix, copy: ``draw_arrows``' -- a CUDA frame is changed IN PLACE (copy=True: a packed clone is), a numpy frame
        goes up through the staging ring.  boxes [n,4] x1 y1 x2 y2, image_of [n]: numpy arrays or device tensors, read where they are.
        expand: the box grows by this share of its size on every side (0 .. 4).  cell: None -- every head gets about ``blocks`` (1 .. 64) cells
        across, a power of two of 2 .. 64 pixels each, so a far head is as unreadable as a near one -- or one power of two in 2 .. 64 for all.
        color: one (B, G, R) triple on the host, converted once by ``bgr_to_yuv`` for NV12; read only with mode='fill'.  The defaults are
        CONVENTIONS, not tuned on data.  Where boxes overlap the coarser cell wins.  Calling twice is not idempotent: the second call
        averages what the first one wrote.
        Host tables are checked before anything is launched (ValueError: an image_of out of range, a box that is not finite, empty, or
        beyond +-8191 once grown); device tables are never read back -- such rows come back with flag 2 and change no byte.  With device
        frames in place, device tables and the frame table cached by a first call, the call touches the host nowhere and can be captured
        in a graph.
        -> (images on the device, in order; flags [n] int32 on the device: 0 usable -- possibly no pixel --, 2 unusable)."""
        lib = L.load()
        who = 'anonymize_heads'
        nv12, _ = _pixel_format(pixel_format, matrix)
        expand, shape_id, cell_shift, blocks, mode_id = _anon_params(who, expand, shape, cell, blocks, mode)
        one = _anon_color(who, color, nv12, matrix)
        entry = lib.mcg_anonymize_heads_nv12 if nv12 else lib.mcg_anonymize_heads
        checked = _drawing_checked(who, 'heads', entry, images, boxes, None, image_of, nv12, device)
        dev, n = checked[0], checked[-1]
        with _call_scope(self._ring, dev, stream) as call:
            out, pixels, in_place, table, h_max, w_max, boxes, _, _, image_of = _drawing_placed(who, checked, nv12, copy, None, 0)
            if isinstance(boxes, np.ndarray) and n:                # image_of on the device is not read back: every frame's size then passes
                sizes = [(int(r['h']), int(r['w'])) for r in table] if isinstance(image_of, np.ndarray) else [(2, 2)]
                bad = anonymize_plan_host(boxes, image_of if isinstance(image_of, np.ndarray) else np.zeros(n, np.int32), sizes, expand, shape, cell,
                                          blocks, nv12)['flag'] == 2
                if bad.any():
                    k = int(np.flatnonzero(bad)[0])
                    raise ValueError(f'{who}: head {k} cannot be hidden: box {boxes[k].tolist()} -- x2 <= x1 or y2 <= y1, beyond +-{ARROW_COORD} once grown, '
                                     f'or a frame without pixels')
            images_ptr, boxes_ptr, image_of_ptr = self._drawing_upload(call, nv12, table, pixels, in_place, (boxes, image_of))
            flags = torch.empty(n, dtype=torch.int32, device=dev)
            if n:
                plan = torch.empty(n, _ANON_WORDS, dtype=torch.int32, device=dev)
                vp = C.c_void_p
                L.check(entry(vp(call.main.cuda_stream), vp(images_ptr), len(out), h_max, w_max, vp(boxes_ptr), vp(image_of_ptr), n, expand, shape_id,
                              cell_shift, blocks, mode_id, (C.c_ubyte * 3)(*[int(v) for v in one]), vp(plan.data_ptr()), vp(flags.data_ptr())),
                        entry.__name__)
        return out, flags

    def letterbox(self, frames, new_shape=640, stride=32, auto=True, scaleup=True, dtype=torch.float16, rgb=False, pixel_format='bgr', matrix='bt601',
                  device='cuda:0', stream=None):
        """Frames -> the input of the demo's head detector, on the device (mcg_letterbox_frames / mcg_letterbox_frames_nv12: one launch) --
        ``letterbox_host`` bit for bit: LoadImages' letterbox with a border of 114, RGB planes, and the ``img.half() / 255.0`` of detect.py:64-65
        (MCGaze_demo/yolo_head/utils/datasets.py:185-189, 810-840).

        frames: what head_crops takes as ``images`` -- HxWx3 uint8 frames in cv2's BGR order (rgb=True: RGB), or with pixel_format='nv12' a
        decoder's surfaces ((y, uv) pairs or [3H/2, W], even sizes; ``matrix`` names the coefficients, rgb is ignored).  A numpy frame goes up
        through the staging ring, a CUDA tensor is read where it is, its row pitch taken from the tensor.  new_shape, stride, auto, scaleup:
        ``letterbox_geometry``'s, worked out on the host from the shapes alone.  The frames of one call may differ in size but must share ONE
        output shape (ValueError naming the shapes); that, the frames (TypeError / ValueError as in head_crops) and the options are checked
        before anything is launched.  dtype: torch.uint8 (the bytes), float32 (byte / 255) or float16 (that float rounded to half).
        -> (img [B, 3, out_h, out_w] on the device, [LetterboxGeometry per frame] on the host).  ``img.shape[2:]`` is detect_heads' in_shape.
        The descriptor table of device frames is kept per content, so a call on device frames touches the host nowhere after the first and can
        be captured in a graph."""
        lib = L.load()
        nv12, coef = _pixel_format(pixel_format, matrix)
        out_dtype = _letterbox_dtype(dtype)
        entry, more = (lib.mcg_letterbox_frames_nv12, (C.byref(L.YuvCoef(**coef)),)) if nv12 else (lib.mcg_letterbox_frames, ())
        dev = _device(device)
        frames = list(frames)
        planes = [_nv12_planes(k, im, dev) for k, im in enumerate(frames)] if nv12 else None
        dev = _device(dev, entry.__name__)
        table, parts = _image_table(frames, dev, planes)
        geoms, out_h, out_w = _letterbox_plan([(int(r['h']), int(r['w'])) for r in table], new_shape, stride, auto, scaleup)
        desc = np.zeros(len(frames), dtype=_NV12_LETTERBOX if nv12 else _LETTERBOX)
        fd = desc['frame']
        fd['src'], fd['src_pitch'] = (table['y'], table['pitch_y']) if nv12 else (table['src'], table['pitch'])
        if nv12:
            fd['uv'], fd['uv_pitch'] = table['uv'], table['pitch_uv']
        fd['src_h'] = fd['crop_h'] = table['h']
        fd['src_w'] = fd['crop_w'] = table['w']
        fd['out_h'], fd['out_w'] = [g.unpad_h for g in geoms], [g.unpad_w for g in geoms]
        desc['top'], desc['left'] = [g.top for g in geoms], [g.left for g in geoms]
        with _call_scope(self._ring, dev, stream) as call:
            # device frames: only the descriptor table comes from the host, and only the first time these frames and sizes are seen
            frame_table = desc if parts else self._device_table(desc, dev, 'letterbox', nv12)

            def name_frames(at):                                  # a host frame's address: where its bytes land in the device twin
                for (k, f, _), a in zip(parts, at):
                    fd['uv' if f == 'uv' else 'src'][k] = a

            _, (desc_ptr,) = call.upload([a for _, _, a in parts], (frame_table,), name_frames)
            img = torch.empty(len(frames), 3, out_h, out_w, dtype=out_dtype, device=dev)
            vp = C.c_void_p
            L.check(entry(vp(call.main.cuda_stream), vp(desc_ptr), len(frames), vp(img.data_ptr()), out_h, out_w, _LETTERBOX_TYPES[out_dtype],
                          int(not (rgb and not nv12)), *more), entry.__name__)
        return img, geoms

    def detect_heads(self, pred, in_shape, frame_hw, conf_thres=0.25, iou_thres=0.45, only_class=1, agnostic=False, max_nms=30000, max_det=300,
                     device='cuda:0', stream=None):
        """Head boxes from the raw output of the demo's head detector, on the device (mcg_detect_heads: one launch, one workgroup per image) --
        ``detect_heads_host`` bit for bit: the confidence filter, class-aware greedy NMS and the scale-back into the frame of
        non_max_suppression + scale_coords(...).round() (MCGaze_demo/yolo_head/detect.py:74,95).

        pred [B, N, 5 + nc]: a CUDA tensor is read where it is, its image and row strides taken from the tensor (fp16 is widened with
        ``.float()``, which is exact; anything but unit-stride rows is made contiguous first); a numpy array goes up through the staging ring.
        in_shape: the (h, w) of the detector's letterboxed input.  frame_hw: one (h, w), an [B, 2] array, or an integer [B, 2] device tensor
        (h0, w0 per image), which is not read back.  The other arguments are detect_heads_host's; they and the shapes are checked before
        anything is launched (TypeError / ValueError).
        -> (boxes [B, max_det, 4] f32, scores [B, max_det] f32, classes, image_of [B, max_det] int32, counts [B] int32, flags [B] int32) on the
        device.  Rows behind counts[b] are zero with image_of = -1, which head_crops and draw_arrows flag as unusable rows: ``boxes.view(-1, 4)``
        and ``image_of.view(-1)`` feed them with no read-back.  The workspace is kept per (B, N) and the table of a host frame_hw per
        content, so a call on a device prediction touches the host nowhere after the first and can be captured in a graph; calls that share a
        (B, N) share the workspace and belong on one stream."""
        lib = L.load()
        params = _detect_params(conf_thres, iou_thres, only_class, agnostic, max_nms, max_det)
        conf_thres, iou_thres, only_class, agnostic, max_nms, max_det = params
        pred_there = isinstance(pred, torch.Tensor) and pred.is_cuda
        if not pred_there:
            pred = _host_array(pred)
        if pred.dtype not in ((torch.float32, torch.float16) if pred_there else (np.float32, np.float16)):
            raise TypeError(f'detect_heads: pred must be float32 or float16, got {pred.dtype}')
        B, N, nc, in_h, in_w, hw = _detect_shapes(tuple(pred.shape), in_shape, frame_hw)
        dev = _device(pred.device if pred_there else device, 'mcg_detect_heads')
        with _call_scope(self._ring, dev, stream) as call:
            new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
            out = (new(B, max_det, 4, dtype=torch.float32), new(B, max_det, dtype=torch.float32), new(B, max_det), new(B, max_det), new(B), new(B))
            if B == 0:
                return out
            if pred_there:
                pred = pred.float()
                if pred.stride(2) != 1 or pred.stride(1) < 5 + nc or pred.stride(0) < 0:
                    pred = pred.contiguous()
                image_stride, row_stride = int(pred.stride(0)), int(pred.stride(1))
            else:
                pred, image_stride, row_stride = np.ascontiguousarray(pred, dtype=np.float32), N * (5 + nc), 5 + nc
            _, (pred_ptr,) = call.upload([], (pred,))
            if hw is None:
                frame_hw = frame_hw.to(torch.int32).contiguous()
            else:
                frame_hw = self._kept(self._frame_hw_tables, (dev.index, hw.tobytes()), lambda: torch.from_numpy(hw.copy()).to(dev))
            ws = self._kept(self._detect_workspaces, (dev.index, B, N),
                            lambda: torch.empty(int(lib.mcg_detect_heads_workspace_bytes(B, N)), dtype=torch.uint8, device=dev))
            vp = C.c_void_p
            L.check(lib.mcg_detect_heads(vp(call.main.cuda_stream), vp(pred_ptr), B, N, nc, image_stride, row_stride, in_h, in_w, vp(frame_hw.data_ptr()),
                                         conf_thres, iou_thres, only_class, int(agnostic), min(max_nms, N), max_det, *(vp(t.data_ptr()) for t in out),
                                         vp(ws.data_ptr()), ws.numel()), 'mcg_detect_heads')
        return out

    def track_heads(self, boxes, counts, state=None, slots=16, match_iou=0.3, max_age=5, device='cuda:0', stream=None, motion=None):
        """Which head of frame t is the person of which head of frame t - 1, on the device (mcg_track_heads: one launch, one workgroup per
        sequence, the frames walked inside the kernel) -- ``track_heads_host`` bit for bit, whose arguments and seven results these are.

        boxes [T, D, 4] f32 (one sequence, one camera) or [Q, T, D, 4] and counts [T] or [Q, T]: CUDA tensors are read where they are --
        ``detect_heads``' boxes and counts as they come; the frame stride is taken from the tensor, any other view is made contiguous first --
        and numpy arrays go up through the staging ring.  state: an int32 [Q, track_state_words(slots)] tensor on the device, which the call
        UPDATES IN PLACE and hands back; None allocates a zeroed one (the empty state).  Shapes and options are checked before anything is
        launched (TypeError / ValueError).
        -> (slot_boxes [.., T, S, 4] f32, image_of, track_id, age, det_of [.., T, S] int32, flags [.., T] int32, state) on the device.
        ``slot_boxes.view(-1, 4)`` and ``image_of.view(-1)`` feed head_crops and draw_arrows directly when their images are the frames of this
        call: the rows of slots that saw no head in a frame have image_of = -1, which they flag as unusable rows (2) and skip.  With device
        inputs and a given state the call touches the host nowhere and can be captured in a graph.
        motion: None, True or dict(gain=0.5, decay=1.0) as for ``track_heads_host``: the constant-velocity motion model
        (mcg_track_heads_motion, the same launch), with state_boxes [.., T, S, 4] f32 -- every slot's box after the frame, a coasting slot's
        predicted one -- as an eighth result behind the state."""
        lib = L.load()
        slots, match_iou, max_age = _track_params(slots, match_iou, max_age)
        motion = _track_motion(motion)
        boxes_there = isinstance(boxes, torch.Tensor) and boxes.is_cuda
        if not boxes_there:
            boxes = _host_array(boxes)
        if boxes.dtype != (torch.float32 if boxes_there else np.float32):
            raise TypeError(f'track_heads: boxes must be float32, got {boxes.dtype}')
        counts_there = isinstance(counts, torch.Tensor) and counts.is_cuda
        if not counts_there:
            counts = _host_array(counts)
            if counts.dtype.kind not in 'iu':
                raise TypeError(f'track_heads: counts must hold integers, got {counts.dtype}')
        elif counts.dtype not in (torch.int32, torch.int64):
            raise TypeError(f'track_heads: counts must hold integers, got {counts.dtype}')
        Q, T, D, given_q = _track_shapes(tuple(boxes.shape), tuple(counts.shape), None if state is None else tuple(state.shape), slots)
        dev = _device(boxes.device if boxes_there else device, 'mcg_track_heads')
        if state is not None and not (isinstance(state, torch.Tensor) and state.device == dev and state.dtype == torch.int32 and state.is_contiguous()):
            raise TypeError(f'track_heads: the state is a contiguous int32 tensor on {dev} (it is updated in place)')
        with _call_scope(self._ring, dev, stream) as call:
            new = lambda *shape, dtype=torch.int32: torch.empty(*shape, dtype=dtype, device=dev)
            lead = (Q, T) if given_q else (T,)
            out = (new(*lead, slots, 4, dtype=torch.float32), new(*lead, slots), new(*lead, slots), new(*lead, slots), new(*lead, slots), new(*lead))
            more = () if motion is None else (new(*lead, slots, 4, dtype=torch.float32),)         # state_boxes
            if state is None:
                state = torch.zeros(Q, track_state_words(slots), dtype=torch.int32, device=dev)
            if Q == 0:
                return out + (state,) + more
            frame_stride = 4 * D
            if boxes_there:
                b = boxes if given_q else boxes[None]
                stride = b.stride(1) if T > 1 else b.stride(0) if Q > 1 else 4 * D
                if not (b.stride(3) == 1 and b.stride(2) == 4 and stride >= 4 * D and (Q == 1 or T == 1 or b.stride(0) == T * stride)):
                    b, stride = b.contiguous(), 4 * D
                boxes, frame_stride = b, int(stride)
            else:
                boxes = np.ascontiguousarray(boxes, dtype=np.float32)
            counts = counts.to(dev, torch.int32).contiguous() if counts_there else np.ascontiguousarray(counts, dtype=np.int32)
            _, (boxes_ptr, counts_ptr) = call.upload([], (boxes, counts))
            vp = C.c_void_p
            head = (vp(call.main.cuda_stream), vp(boxes_ptr), frame_stride, vp(counts_ptr), Q, T, D, slots, match_iou, max_age)
            tail = (vp(state.data_ptr()), *(vp(t.data_ptr()) for t in out + more))
            if motion is None:
                L.check(lib.mcg_track_heads(*head, *tail), 'mcg_track_heads')
            else:
                L.check(lib.mcg_track_heads_motion(*head, *motion, *tail), 'mcg_track_heads_motion')
        return out + (state,) + more


def build_pipeline(transforms):
    return DevicePipeline(transforms)
