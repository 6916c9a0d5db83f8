"""Gaze targets on the host (include/mcgaze_hip.h, "gaze targets"): what every head looks at -- another head of its picture, a marked
rectangle, the lens or nothing.  ``gaze_targets_host`` is in numpy what ``DevicePipeline.gaze_targets`` (mcg_gaze_targets) writes on the
device, bit for bit; it serves checks and users without a GPU.  The ray is the demo's arrow (MCGaze_demo/demo.ipynb, cell 5) followed until
it meets something, in the image plane: no camera intrinsics, no depth.  The defaults (expand 0.25, a 10 degree cone for "the camera") are
conventions, not tuned on data."""
import math

import numpy as np

from .staging import _host_array

KIND_NONE, KIND_HEAD, KIND_REGION, KIND_CAMERA = 0, 1, 2, 3
KIND_NAMES = ('none', 'head', 'region', 'camera')
MAX_ROWS, MAX_REGIONS = 65536, 4096                              # the bounds of mcg_gaze_targets
EXPAND, CAMERA_ANGLE = 0.25, 10.0                                # conventions, not tuned on data
FIELDS = ('kind', 'target', 't', 'hit', 'mutual', 'flags')       # the order of the six tables


def _target_params(expand=EXPAND, camera_angle=CAMERA_ANGLE, region_period=0, who='gaze_targets'):
    """The options, validated (ValueError) -> (expand, camera_cos2, region_period) as the entry takes them.  camera_angle: the half angle of
    the cone around the lens axis, in degrees, 0 .. 90; None switches the camera test off (camera_cos2 = 2.0 never holds)."""
    if isinstance(expand, bool) or not isinstance(expand, (int, float, np.integer, np.floating)) or not (math.isfinite(expand) and expand >= 0):
        raise ValueError(f'{who}: expand must be a finite number >= 0, got {expand!r}')
    if camera_angle is not None and (isinstance(camera_angle, bool) or not isinstance(camera_angle, (int, float, np.integer, np.floating)) or
                                     not 0 <= camera_angle <= 90):
        raise ValueError(f'{who}: camera_angle is None or a half angle in degrees, 0 .. 90; got {camera_angle!r}')
    if isinstance(region_period, bool) or not isinstance(region_period, (int, np.integer)) or region_period < 0:
        raise ValueError(f'{who}: region_period must be an int >= 0, got {region_period!r}')
    cos2 = 2.0 if camera_angle is None else math.cos(math.radians(float(camera_angle))) ** 2
    return float(expand), cos2, int(region_period)


def _check_counts(who, n, m):
    if n > MAX_ROWS:
        raise ValueError(f'{who}: at most {MAX_ROWS} rows per call (got {n})')
    if m > MAX_REGIONS:
        raise ValueError(f'{who}: at most {MAX_REGIONS} regions per call (got {m})')


def _region_tables(who, regions, region_image):
    """Host regions -> (f32 [m,4], int32 [m]), checked (TypeError / ValueError).  None: no regions; region_image None: every picture (-1)."""
    if regions is None:
        if region_image is not None and np.size(_host_array(region_image)):
            raise ValueError(f'{who}: region_image without regions')
        return np.zeros((0, 4), np.float32), np.zeros(0, np.int32)
    r = np.asarray(_host_array(regions))
    if r.size == 0:
        r = r.reshape(0, 4)
    if r.ndim != 2 or r.shape[1] != 4 or r.dtype.kind not in 'fiu':
        raise ValueError(f'{who}: regions must be [m, 4] numbers x1 y1 x2 y2, got {r.dtype} {r.shape}')
    r = np.ascontiguousarray(r, dtype=np.float32)
    if region_image is None:
        ri = np.full(len(r), -1, np.int32)
    else:
        ri = np.asarray(_host_array(region_image)).reshape(-1)
        if ri.size and ri.dtype.kind not in 'iu':
            raise TypeError(f'{who}: region_image must hold integers, got {ri.dtype}')
        if ri.shape != (len(r),):
            raise ValueError(f'{who}: region_image must be [{len(r)}], one per region; got {ri.shape}')
        ri = np.ascontiguousarray(ri, dtype=np.int32)
    return r, ri


def _attention_options(who, attention, cameras=None):
    """The ``attention=`` option of LiveGaze and run_head_video, validated (ValueError) -> None (off), or (regions f32 [m,4], region_image
    int32 [m], dict(expand=, camera_angle=)).  attention: None, True or dict(regions=, expand=, camera_angle=).  regions: [[x1, y1, x2, y2],
    ...], which apply to every picture (region_image -1); with ``cameras`` a list of that many such tables (or None), one per camera, whose
    region_image is the camera."""
    if attention is None:
        return None
    if attention is not True and not isinstance(attention, dict):
        raise ValueError(f'{who}: attention is None, True or a dict of regions, expand and camera_angle; got {attention!r}')
    opts = {} if attention is True else dict(attention)
    if set(opts) - {'regions', 'expand', 'camera_angle'}:
        raise ValueError(f'{who}: attention takes regions, expand and camera_angle; got {sorted(opts)}')
    regions = opts.pop('regions', None)
    _target_params(opts.get('expand', EXPAND), opts.get('camera_angle', CAMERA_ANGLE), 0, f'{who}(attention=...)')
    try:
        if cameras is None:
            tables = [_region_tables(who, regions, None)[0]]
        else:
            if regions is not None and (isinstance(regions, np.ndarray) or len(regions) != cameras):
                raise ValueError(f'{who}: attention regions are a list of {cameras} tables, one per camera (None: no regions there)')
            tables = [_region_tables(who, r, None)[0] for r in (regions if regions is not None else [None] * cameras)]
    except TypeError as e:
        raise ValueError(f'{who}: attention regions: {e}') from None
    table = np.concatenate(tables) if tables else np.zeros((0, 4), np.float32)
    _check_counts(who, 0, len(table))
    image = np.full(len(table), -1, np.int32) if cameras is None else np.repeat(np.arange(len(tables), dtype=np.int32), [len(t) for t in tables])
    return table, image.astype(np.int32), opts


def _row_tables(who, boxes, gaze, image_of):
    """Host rows -> (f32 [n,4], f32 [n,3], int32 [n]), checked.  image_of None: every row is in picture 0."""
    b = np.asarray(_host_array(boxes))
    b = np.ascontiguousarray(b.reshape(0, 4) if b.size == 0 else b, dtype=np.float32)
    g = np.asarray(_host_array(gaze))
    g = g.reshape(0, 3) if g.size == 0 and len(b) == 0 else g
    if b.ndim != 2 or b.shape[1] != 4 or g.ndim != 2 or g.shape[0] != len(b) or g.shape[1] < 3:
        raise ValueError(f'{who}: boxes {b.shape} and gaze {g.shape} must be [n,4] and [n,>=3]')
    g = np.ascontiguousarray(g[:, :3], dtype=np.float32)
    if image_of is None:
        io = np.zeros(len(b), np.int32)
    else:
        io = np.asarray(_host_array(image_of)).reshape(-1)
        if io.size and io.dtype.kind not in 'iu':
            raise TypeError(f'{who}: image_of must hold integers, got {io.dtype}')
        if io.shape != (len(b),):
            raise ValueError(f'{who}: image_of must be [{len(b)}], one per row; got {io.shape}')
        io = np.ascontiguousarray(io, dtype=np.int32)
    return b, g, io


def _entries(o, d, lo, hi):
    """The slab test of the header for rays (o, d: [s, 2]) against rectangles (lo, hi: [c, 2]) -> t [s, c], +inf for a miss."""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        near, far = np.full((len(o), len(lo)), -np.inf), np.full((len(o), len(lo)), np.inf)
        ok = np.ones((len(o), len(lo)), bool)
        for a in (0, 1):
            oa, da, la, ha = o[:, a, None], d[:, a, None], lo[None, :, a], hi[None, :, a]
            zero = np.broadcast_to(da == 0.0, ok.shape)
            t1, t2 = (la - oa) / da, (ha - oa) / da
            ok &= np.where(zero, (la <= oa) & (oa <= ha), True)
            near = np.where(zero, near, np.maximum(near, np.minimum(t1, t2)))
            far = np.where(zero, far, np.minimum(far, np.maximum(t1, t2)))
        t = np.where(near > 0.0, near, 0.0)
        return np.where(ok & (near <= far) & (far >= 0.0) & np.isfinite(t), t, np.inf)


def gaze_targets_host(boxes, gaze, image_of=None, regions=None, region_image=None, region_period=0, expand=EXPAND, camera_angle=CAMERA_ANGLE):
    """``mcg_gaze_targets`` in numpy float64, bit for bit (include/mcgaze_hip.h, "gaze targets").

    boxes [n,4] x1 y1 x2 y2 and gaze [n,>=3] (gx, gy, gz; -z towards the lens), read as f32 and widened; image_of [n] integers, rows with equal
    image_of being in one picture (None: all in picture 0; negative: an unusable row).  regions [m,4] rectangles with region_image [m] (None:
    -1): a region applies to a row iff region_image < 0, or equals image_of (region_period 0), or equals image_of % region_period.  expand: a
    looked-at head's box is grown by expand * its longer side on each side.  camera_angle: half angle in degrees of the cone around the lens
    axis inside which a gaze is "at the camera" (None: never).  Both defaults are conventions, not tuned on data.
    -> (kind int32 [n]: KIND_NONE / KIND_HEAD / KIND_REGION / KIND_CAMERA; target int32 [n]: the row or region index, else -1; t float32 [n];
    hit float32 [n,2]; mutual int32 [n]; flags int32 [n]: 2 for an unusable row) -- the dtypes the kernel writes."""
    who = 'gaze_targets_host'
    expand, cos2, period = _target_params(expand, camera_angle, region_period, who)
    b32, g32, io = _row_tables(who, boxes, gaze, image_of)
    r32, ri = _region_tables(who, regions, region_image)
    n, m = len(b32), len(r32)
    _check_counts(who, n, m)
    b, g, r = b32.astype(np.float64), g32.astype(np.float64), r32.astype(np.float64)
    kind, target = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    t_out, hit = np.zeros(n, np.float64), np.zeros((n, 2), np.float64)
    usable = np.isfinite(b).all(axis=1) & np.isfinite(g).all(axis=1) & ~(b[:, 2] < b[:, 0]) & ~(b[:, 3] < b[:, 1]) & (io >= 0)
    flags = np.where(usable, 0, 2).astype(np.int32)
    b, g = np.where(usable[:, None], b, 0.0), np.where(usable[:, None], g, 0.0)
    gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
    # numpy rounds every elementwise product and sum on its own: nothing is contracted, as in the kernel
    camera = usable & (gz < 0.0) & (gz * gz >= cos2 * ((gx * gx + gy * gy) + gz * gz))
    kind[camera] = KIND_CAMERA
    o = np.stack([(b[:, 0] + b[:, 2]) * 0.5, (b[:, 1] + b[:, 3]) * 0.5], axis=1)
    d = np.stack([-gx, -gy], axis=1)
    searching = usable & ~camera & ~((d[:, 0] == 0.0) & (d[:, 1] == 0.0))
    side = np.maximum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])
    with np.errstate(over='ignore'):
        e = expand * side
    lo, hi = np.stack([b[:, 0] - e, b[:, 1] - e], axis=1), np.stack([b[:, 2] + e, b[:, 3] + e], axis=1)
    r_ok = np.isfinite(r).all(axis=1) & ~(r[:, 2] < r[:, 0]) & ~(r[:, 3] < r[:, 1])
    for picture in np.unique(io[searching]):
        rows = np.flatnonzero(usable & (io == picture))           # the candidates, ascending; the sources are among them
        src = rows[searching[rows]]
        heads = _entries(o[src], d[src], lo[rows], hi[rows])
        heads[src[:, None] == rows[None, :]] = np.inf              # every OTHER row
        applies = r_ok & ((ri < 0) | (ri == (int(picture) % period if period > 0 else int(picture))))
        regs = np.flatnonzero(applies)
        t = np.concatenate([heads, _entries(o[src], d[src], r[regs, :2], r[regs, 2:])], axis=1)
        if t.shape[1] == 0:
            continue
        best = np.argmin(t, axis=1)                               # the FIRST smallest: heads before regions, then the lower index
        tb = t[np.arange(len(src)), best]
        found = np.isfinite(tb)
        s, best, tb = src[found], best[found], tb[found]
        is_head = best < len(rows)
        kind[s] = np.where(is_head, KIND_HEAD, KIND_REGION)
        target[s] = np.where(is_head, rows[np.minimum(best, len(rows) - 1)], regs[np.maximum(best - len(rows), 0)] if len(regs) else -1)
        t_out[s] = tb
        hit[s] = o[s] + tb[:, None] * d[s]
    mutual = np.zeros(n, np.int32)
    heads = np.flatnonzero(kind == KIND_HEAD)
    back = target[heads]
    mutual[heads] = (kind[back] == KIND_HEAD) & (target[back] == heads)
    with np.errstate(over='ignore'):
        return kind, target, t_out.astype(np.float32), hit.astype(np.float32), mutual, flags
