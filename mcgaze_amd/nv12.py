"""Frames as BGR arrays or as a video decoder's NV12 surfaces (``pixel_format='nv12'``), which the pixel kernels convert tap by tap
(``mcg_preprocess_head_crops_nv12``): ``nv12_to_bgr`` is that conversion on the host, ``bgr_to_yuv`` the colour an NV12 surface is drawn with."""
import numpy as np
import torch

# YUV -> RGB coefficients at 20 fractional bits (include/mcgaze_hip.h, mcg_yuv_coef).  bt601: OpenCV's published limited-range constants
# (its ITUR_BT_601_* set, 1.164 / 2.018 / -0.391 / -0.813 / 1.596 scaled by 2^20), restated, not linked: parity with cv2's COLOR_YUV2BGR_NV12
# is not pinned on any machine this was built on.  bt709: limited range, round(c * 2**20) of the matrix with Kr = 0.2126, Kb = 0.0722,
# luma scale 255/219 and chroma scale 255/224, worked out once in double: cy = 255/219, cub = 2 (1 - Kb) 255/224,
# cug = -(Kb / Kg) 2 (1 - Kb) 255/224, cvg = -(Kr / Kg) 2 (1 - Kr) 255/224, cvr = 2 (1 - Kr) 255/224 with Kg = 1 - Kr - Kb.
YUV_COEF = {
    'bt601': dict(y_off=16, cy=1220542, cub=2116026, cug=-409993, cvg=-852492, cvr=1673527),
    'bt709': dict(y_off=16, cy=1220945, cub=2215014, cug=-223607, cvg=-558796, cvr=1879825),
}


def _yuv_coef(matrix):
    if matrix not in YUV_COEF:
        raise ValueError(f'matrix must be one of {sorted(YUV_COEF)}, got {matrix!r}')
    return YUV_COEF[matrix]


def _pixel_format(pixel_format, matrix):
    """The ``pixel_format`` / ``matrix`` options, checked (ValueError) -> (nv12, the matrix's YUV_COEF entry)."""
    if pixel_format not in ('bgr', 'nv12'):
        raise ValueError(f"pixel_format must be 'bgr' or 'nv12', got {pixel_format!r}")
    return pixel_format == 'nv12', _yuv_coef(matrix)


def _nv12_planes(k, im, dev=None):
    """One NV12 surface as head_crops takes it -> (y [H,W], uv [H/2,W] as a 2-d view, on_device): a (y, uv) pair with uv [H/2,W/2,2] or
    [H/2,W], or a single [3H/2, W] surface (Y rows, then the UV rows).  TypeError for a wrong dtype, rank or device, ValueError for odd sizes
    or a UV plane that does not belong to the Y plane."""
    if isinstance(im, (tuple, list)):
        if len(im) != 2:
            raise TypeError(f'frame {k}: an NV12 frame is a (y, uv) pair or one [3H/2, W] surface, got a sequence of {len(im)}')
        y, uv = im
    else:
        y, uv = im, None
    on_device = isinstance(y, torch.Tensor)
    if uv is not None and isinstance(uv, torch.Tensor) != on_device:
        raise TypeError(f'frame {k}: the Y and UV planes must both be numpy arrays or both be device tensors')
    if not on_device:
        y = np.asarray(y)
        uv = None if uv is None else np.asarray(uv)
    u8 = torch.uint8 if on_device else np.uint8
    for name, t in (('Y', y), ('UV', uv)):
        if t is None:
            continue
        if t.dtype != u8 or t.ndim not in ((2,) if name == 'Y' else (2, 3)) or (t.numel() if on_device else t.size) == 0:
            raise TypeError(f'frame {k}: the {name} plane must be a non-empty uint8 array of rank {"2" if name == "Y" else "2 or 3"}, got {t.dtype} {tuple(t.shape)}')
        if on_device and not (t.is_cuda and t.device == dev):
            raise TypeError(f'frame {k}: device planes must be uint8 tensors on {dev}, got one on {t.device}')
    if uv is None:                                                # one surface: 3H/2 rows
        rows, w = y.shape
        if rows % 3 or w % 2:
            raise ValueError(f'frame {k}: a {rows} x {w} surface is not [3H/2, W] with H and W even')
        h = rows // 3 * 2
        y, uv = y[:h], y[h:]
    h, w = y.shape
    if h % 2 or w % 2:
        raise ValueError(f'frame {k}: NV12 frames have even sizes, got {h} x {w}')
    if tuple(uv.shape) not in ((h // 2, w // 2, 2), (h // 2, w)):
        raise ValueError(f'frame {k}: the UV plane of a {h} x {w} frame is [{h // 2}, {w // 2}, 2] or [{h // 2}, {w}], got {tuple(uv.shape)}')
    if on_device:
        # rows may lie further apart than w bytes (a decoder's pitch); inside a row the bytes are packed
        packed = y.stride(1) == 1 and (uv.stride(1) == 1 if uv.ndim == 2 else (uv.stride(2) == 1 and (uv.shape[1] == 1 or uv.stride(1) == 2)))
        if not (packed and y.stride(0) >= w and (uv.shape[0] == 1 or uv.stride(0) >= w)):
            raise TypeError(f'frame {k}: device planes must have packed rows at least {w} bytes apart, got strides {tuple(y.stride())} and {tuple(uv.stride())}')
        if uv.ndim == 3:
            uv = uv.as_strided((h // 2, w), (uv.stride(0), 1))
    else:
        y, uv = np.ascontiguousarray(y), np.ascontiguousarray(uv).reshape(h // 2, w)
    return y, uv, on_device


def nv12_to_bgr(y, uv, matrix='bt601'):
    """An NV12 frame -> HxWx3 uint8 BGR on the host, in the arithmetic the pixel kernel applies per tap (csrc/preprocess.hip, Nv12Source):
    y [H,W] uint8, uv [H/2,W/2,2] or [H/2,W] uint8 interleaved (U, V), H and W even; matrix: a key of YUV_COEF.  Chroma is the nearest
    sample, uv[y >> 1][x >> 1], and with u = U - 128, v = V - 128 in 32-bit integers (>> is an arithmetic shift):

        yy = max(0, Y - y_off) * cy
        R = sat8((yy + cvr * v + (1 << 19)) >> 20);  G = sat8((yy + cvg * v + cug * u + (1 << 19)) >> 20);  B = sat8((yy + cub * u + (1 << 19)) >> 20)

    head_crops(pixel_format='nv12') on the planes equals head_crops on this frame bit for bit."""
    k = _yuv_coef(matrix)
    y, uv, _ = _nv12_planes(0, (np.asarray(y), np.asarray(uv)))
    h, w = y.shape
    u, v = (np.repeat(np.repeat(uv.reshape(h // 2, w // 2, 2)[..., j], 2, axis=0), 2, axis=1) for j in (0, 1))
    return _yuv_to_bgr(np.stack([y, u, v], axis=-1), k).astype(np.uint8)


def _yuv_to_bgr(yuv, k):
    """(Y, U, V) integer arrays [..., 3] -> BGR [..., 3] int32 by nv12_to_bgr's arithmetic."""
    yuv = np.asarray(yuv, dtype=np.int32)
    u, v = yuv[..., 1] - 128, yuv[..., 2] - 128
    yy = np.maximum(0, yuv[..., 0] - k['y_off']) * np.int32(k['cy']) + np.int32(1 << 19)
    sat8 = lambda t: np.clip(t >> 20, 0, 255)
    return np.stack([sat8(yy + k['cub'] * u), sat8(yy + k['cvg'] * v + k['cug'] * u), sat8(yy + k['cvr'] * v)], axis=-1)


def bgr_to_yuv(color, matrix='bt601'):
    """The (Y, U, V) an NV12 surface is drawn with so that it SHOWS the BGR colour ``color`` -> uint8 [3].  No new constants: the matrix of
    ``YUV_COEF[matrix]`` (B = cy y + cub u, G = cy y + cug u + cvg v, R = cy y + cvr v with y = Y - y_off, u = U - 128, v = V - 128, each
    coefficient / 2^20) is inverted numerically and the result rounded; among the triples within 2 of it in every component (and inside
    [0, 255]) the one whose conversion by nv12_to_bgr's integer arithmetic has the smallest maximum channel error against ``color`` is taken,
    ties going to the smallest (Y, U, V) in lexicographic order.  Runs once per colour, on the host."""
    k = _yuv_coef(matrix)
    c = np.asarray(color)
    if c.shape != (3,) or c.dtype.kind not in 'iu' or c.min() < 0 or c.max() > 255:
        raise ValueError(f'a colour is three integers in [0, 255] (B, G, R), got {color!r}')
    c = c.astype(np.int64)
    m = np.array([[k['cy'], k['cub'], 0], [k['cy'], k['cug'], k['cvg']], [k['cy'], 0, k['cvr']]], dtype=np.float64) / float(1 << 20)
    centre = np.rint(np.linalg.solve(m, c.astype(np.float64)) + np.array([k['y_off'], 128.0, 128.0])).astype(np.int64)
    grid = np.stack(np.meshgrid(*[np.arange(v - 2, v + 3) for v in centre], indexing='ij'), axis=-1).reshape(-1, 3)     # lexicographic order
    grid = grid[((grid >= 0) & (grid <= 255)).all(axis=1)]
    if not len(grid):                                            # (cannot happen for a colour in [0, 255]^3: its YUV is inside the nominal range)
        raise ValueError(f'no (Y, U, V) near {centre.tolist()} for colour {color!r}')
    err = np.abs(_yuv_to_bgr(grid, k) - c).max(axis=1)
    return grid[int(np.argmin(err))].astype(np.uint8)            # argmin: the FIRST of the smallest, i.e. the lexicographically smallest
