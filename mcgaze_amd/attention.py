"""Gaze targets on the host (include/mcgaze_hip.h, "gaze targets"): what every head looks at -- another head of its picture, a marked
rectangle, the lens or nothing.  ``gaze_targets_host`` is in numpy what ``DevicePipeline.gaze_targets`` (mcg_gaze_targets) writes on the
device, bit for bit; it serves checks and users without a GPU.  The ray is the demo's arrow (MCGaze_demo/demo.ipynb, cell 5) followed until
it meets something, in the image plane: no camera intrinsics, no depth.  The defaults (expand 0.25, a 10 degree cone for "the camera") are
conventions, not tuned on data.  A region may also be a polygon of 3 .. 32 vertices ("gaze targets, polygonal regions", mcg_gaze_targets_poly):
``region_polygons`` turns the mixed list of rectangles and polygons into the vertex tables ``PolyRegions`` that both sides take.

Gaze dwell (include/mcgaze_hip.h, "gaze dwell"): how LONG each person looks at what.  ``gaze_dwell_host`` is in numpy what
``DevicePipeline.gaze_dwell`` (mcg_gaze_dwell) writes on the device, bit for bit: the per-frame targets of the columns (tracker slots or
lanes) become debounced episodes with a start, a length, an end and a reason, and every region collects its person-frames.  The defaults
(enter 3, exit 2) are conventions, not tuned on data."""
import collections
import math

import numpy as np

from .staging import _host_array

KIND_NONE, KIND_HEAD, KIND_REGION, KIND_CAMERA = 0, 1, 2, 3
KIND_NAMES = ('none', 'head', 'region', 'camera')
MAX_ROWS, MAX_REGIONS = 65536, 4096                              # the bounds of mcg_gaze_targets
MAX_VERTICES, POLY_VERTS = 65536, 32                             # ... and of mcg_gaze_targets_poly: vertices a call, vertices a polygon
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


def _check_counts(who, n, m, vertices=0):
    if n > MAX_ROWS:
        raise ValueError(f'{who}: at most {MAX_ROWS} rows per call (got {n})')
    if m > MAX_REGIONS:
        raise ValueError(f'{who}: at most {MAX_REGIONS} regions per call (got {m})')
    if vertices > MAX_VERTICES:
        raise ValueError(f'{who}: at most {MAX_VERTICES} vertices per call (got {vertices})')


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


def _holds_polygon(regions):
    """A nested list with an item that is itself a list of lists: the mixed form of ``region_polygons`` ([m, 4] arrays and lists of 4-number
    items keep meaning rectangles)."""
    return isinstance(regions, (list, tuple)) and not isinstance(regions, PolyRegions) and any(isinstance(r, (list, tuple, np.ndarray)) and len(r) and np.ndim(r[0]) > 0 for r in regions)


class PolyRegions(collections.namedtuple('PolyRegions', 'xy start')):
    """The region tables of mcg_gaze_targets_poly, (xy f32 [V, 2], start int32 [m + 1]): region j owns the vertices start[j] ..
    start[j + 1] - 1 -- 2 of them are the corners (x1, y1), (x2, y2) of a rectangle, 3 .. 32 a polygon.  ``regions=PolyRegions(xy, start)``
    is how gaze_targets_host and DevicePipeline.gaze_targets take the vertex form (the tables may be device tensors there); what ``start``
    HOLDS is contents, never an error."""
    __slots__ = ()


def _as_vertices(rectangles):
    """Rectangles f32 [m, 4] in the vertex form: two vertices each."""
    return PolyRegions(rectangles.reshape(-1, 2), 2 * np.arange(len(rectangles) + 1, dtype=np.int32))


def region_polygons(regions):
    """The mixed list of regions -> PolyRegions(xy f32 [V, 2], start int32 [m + 1]), the tables of mcg_gaze_targets_poly.  An item is 4
    numbers x1 y1 x2 y2 (a rectangle: the 2 vertices (x1, y1), (x2, y2)) or 3 .. 32 pairs [x, y] (a polygon, either winding, closed by
    itself).  TypeError for what is no list of such items or holds no numbers, ValueError for an item of another shape; the VALUES are
    contents (a vertex that is not finite makes its region unusable, as on the device)."""
    who = 'region_polygons'
    if not isinstance(regions, (list, tuple, np.ndarray)):
        raise TypeError(f'{who}: regions is a list of rectangles [x1, y1, x2, y2] and polygons [[x, y], ...]; got {type(regions).__name__}')
    parts = []
    for j, item in enumerate(regions):
        if not isinstance(item, (list, tuple, np.ndarray)):
            raise TypeError(f'{who}: region {j} is 4 numbers or a list of [x, y] pairs, got {type(item).__name__}')
        try:
            a = np.asarray(item)
        except ValueError:
            raise ValueError(f'{who}: region {j} is 4 numbers or 3 .. {POLY_VERTS} pairs [x, y], got a ragged list') from None
        if a.dtype.kind not in 'fiu':
            raise TypeError(f'{who}: region {j} must hold numbers, got {a.dtype}')
        if a.shape == (4,):
            a = a.reshape(2, 2)
        elif not (a.ndim == 2 and a.shape[1] == 2 and 3 <= a.shape[0] <= POLY_VERTS):
            raise ValueError(f'{who}: region {j} is 4 numbers or 3 .. {POLY_VERTS} pairs [x, y], got shape {a.shape}')
        parts.append(a.astype(np.float32))
    start = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=start[1:])
    _check_counts(who, 0, len(parts), int(start[-1]))
    return PolyRegions(np.concatenate(parts) if parts else np.zeros((0, 2), np.float32), start.astype(np.int32))


def _poly_tables(who, regions, region_image):
    """Host PolyRegions -> (f32 [V,2], int32 [m+1], int32 [m]), checked (TypeError / ValueError): the shapes, dtypes and counts only -- what
    start HOLDS is contents, as on the device.  region_image None: every picture (-1)."""
    v = np.asarray(_host_array(regions.xy))
    if v.size == 0:
        v = v.reshape(0, 2)
    if v.ndim != 2 or v.shape[1] != 2 or v.dtype.kind not in 'fiu':
        raise ValueError(f'{who}: PolyRegions.xy is the [V, 2] vertex table x y; got {v.dtype} {v.shape}')
    s = np.asarray(_host_array(regions.start))
    if s.size and s.dtype.kind not in 'iu':
        raise TypeError(f'{who}: PolyRegions.start must hold integers, got {s.dtype}')
    if s.ndim != 1 or len(s) < 1:
        raise ValueError(f'{who}: PolyRegions.start must be [m + 1], got {s.shape}')
    m = len(s) - 1
    if region_image is None:
        ri = np.full(m, -1, np.int32)
    else:
        ri = np.asarray(_host_array(region_image)).reshape(-1)
        if ri.size and ri.dtype.kind not in 'iu':
            raise TypeError(f'{who}: region_image must hold integers, got {ri.dtype}')
        if ri.shape != (m,):
            raise ValueError(f'{who}: region_image must be [{m}], one per region; got {ri.shape}')
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(s.astype(np.int32)), np.ascontiguousarray(ri, dtype=np.int32)


def _attention_options(who, attention, cameras=None):
    """The ``attention=`` option of LiveGaze and run_head_video, validated (ValueError) -> None (off), or (regions f32 [m,4], region_image
    int32 [m], dict(expand=, camera_angle=)).  attention: None, True or dict(regions=, expand=, camera_angle=).  regions: [[x1, y1, x2, y2],
    ...], which apply to every picture (region_image -1); with ``cameras`` a list of that many such tables (or None), one per camera, whose
    region_image is the camera.  A table may also be the mixed list of ``region_polygons``; where one holds a polygon, regions is the
    PolyRegions of all tables -- ``regions=`` of gaze_targets either way.  With camera= (and regions3d=, head_size=, frame=) the dict carries
    'three_d': the tables of ``_attention_3d_options``, by which gaze_targets_3d decides; ``regions`` are then only drawn and named."""
    if attention is None:
        return None
    if attention is not True and not isinstance(attention, dict):
        raise ValueError(f'{who}: attention is None, True or a dict of regions, expand and camera_angle; got {attention!r}')
    opts = {} if attention is True else dict(attention)
    if set(opts) - {'regions', 'expand', 'camera_angle'} - set(ATTENTION_3D_OPTIONS):
        raise ValueError(f'{who}: attention takes regions, expand and camera_angle, and for targets in 3-D camera, regions3d, head_size and frame; '
                         f'got {sorted(opts)}')
    regions = opts.pop('regions', None)
    _target_params(opts.get('expand', EXPAND), opts.get('camera_angle', CAMERA_ANGLE), 0, f'{who}(attention=...)')
    if set(opts) & set(ATTENTION_3D_OPTIONS):                     # camera=: the 3-D entry decides; ``regions`` are then only what is drawn
        opts['three_d'] = _attention_3d_options(who, {k: opts.pop(k) for k in ATTENTION_3D_OPTIONS if k in opts}, cameras)
    one = lambda r: region_polygons(r) if _holds_polygon(r) else _region_tables(who, r, None)[0]      # (xy, start), or [m, 4]
    try:
        if cameras is None:
            tables = [one(regions)]
        else:
            if regions is not None and (isinstance(regions, np.ndarray) or len(regions) != cameras):
                raise ValueError(f'{who}: attention regions are a list of {cameras} tables, one per camera (None: no regions there)')
            tables = [one(r) for r in (regions if regions is not None else [None] * cameras)]
    except TypeError as e:
        raise ValueError(f'{who}: attention regions: {e}') from None
    if any(isinstance(t, PolyRegions) for t in tables):          # a polygon somewhere: every table as vertices, the offsets counted through
        tables = [t if isinstance(t, PolyRegions) else _as_vertices(t) for t in tables]
        counts = [len(t.start) - 1 for t in tables]
        first = np.cumsum([0] + [len(t.xy) for t in tables])
        table = PolyRegions(np.concatenate([t.xy for t in tables]),
                            np.concatenate([t.start[:-1] + f for t, f in zip(tables, first)] + [first[-1:]]).astype(np.int32))
        _check_counts(who, 0, sum(counts), len(table.xy))
    else:
        counts = [len(t) for t in tables]
        table = np.concatenate(tables) if tables else np.zeros((0, 4), np.float32)
        _check_counts(who, 0, len(table))
    image = np.full(sum(counts), -1, np.int32) if cameras is None else np.repeat(np.arange(len(tables), dtype=np.int32), counts)
    return table, image.astype(np.int32), opts


ATTENTION_3D_OPTIONS = ('camera', 'regions3d', 'head_size', 'frame')


def _attention_3d_options(who, given, cameras=None):
    """The 3-D part of the ``attention=`` option, validated (ValueError) -> dict(cam f32 [C,4], regions PolyRegions3D, region_image int32
    [m], head_size, frame) as gaze_targets_3d takes them.  camera: [fx, fy, cx, cy] -- of every camera -- or with ``cameras`` one such row
    per camera.  regions3d: a list of planar polygons [[x, y, z], ...] in camera coordinates, which apply to every picture; with ``cameras``
    a list of that many such lists (or None), one per camera, in that camera's coordinates."""
    if given.get('camera') is None:
        raise ValueError(f'{who}: attention regions3d, head_size and frame belong to camera=[fx, fy, cx, cy]: targets in 3-D need the intrinsics')
    try:
        cam = _camera_table(who, given['camera'])
        if cam.shape[0] != (cameras or 1):
            if cam.shape[0] != 1:
                raise ValueError(f'{who}: attention camera is [fx, fy, cx, cy] or one such row per camera ({cameras or 1}), got {cam.shape}')
            cam = np.ascontiguousarray(np.repeat(cam, cameras, axis=0))
        regions = given.get('regions3d')
        if cameras is None:
            tables = [regions_3d(regions if regions is not None else [])]
        else:
            if regions is not None and (isinstance(regions, np.ndarray) or len(regions) != cameras):
                raise ValueError(f'{who}: attention regions3d are a list of {cameras} lists of polygons, one per camera (None: no regions there)')
            tables = [regions_3d(r if r is not None else []) for r in (regions if regions is not None else [None] * cameras)]
    except TypeError as e:
        raise ValueError(f'{who}: attention camera / regions3d: {e}') from None
    head_size, _, _ = _target3d_params(given.get('head_size', HEAD_SIZE), given.get('frame', 'eye'), 0, f'{who}(attention=...)')
    counts = [len(t.start) - 1 for t in tables]
    first = np.cumsum([0] + [len(t.xyz) for t in tables])
    table = PolyRegions3D(np.concatenate([t.xyz for t in tables]),
                          np.concatenate([t.start[:-1] + f for t, f in zip(tables, first)] + [first[-1:]]).astype(np.int32))
    _check_counts(who, 0, sum(counts), len(table.xyz))
    image = np.full(sum(counts), -1, np.int32) if cameras is None else np.repeat(np.arange(len(tables), dtype=np.int32), counts)
    return dict(cam=cam, regions=table, region_image=image.astype(np.int32), head_size=head_size, frame=given.get('frame', 'eye'))


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


def _usable_regions(xy, start):
    """The header's USABLE REGION for every region of the vertex tables (xy float64 [V,2]) -> (ok bool [m], first int64 [m], count int64 [m])."""
    s, e = start[:-1].astype(np.int64), start[1:].astype(np.int64)
    c = e - s
    ok = (0 <= s) & (s <= e) & (e <= len(xy)) & (c >= 2) & (c <= POLY_VERTS)
    for j in np.flatnonzero(ok):                                  # nothing outside xy is looked at: the offsets were checked first
        v = xy[s[j]:e[j]]
        ok[j] = np.isfinite(v).all() and not (c[j] == 2 and (v[1, 0] < v[0, 0] or v[1, 1] < v[0, 1]))
    return ok, s, c


def _polygon_entries(o, d, v):
    """INSIDE and CROSSINGS of the header for rays (o, d: [s, 2]) against ONE polygon (v: [c, 2], c >= 3) -> t [s], +inf for a miss."""
    ox, oy, dx, dy = o[:, 0], o[:, 1], d[:, 0], d[:, 1]
    inside, best = np.zeros(len(o), bool), np.full(len(o), np.inf)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for k in range(len(v)):
            (ax, ay), (bx, by) = v[k], v[(k + 1) % len(v)]
            ex, ey, wx, wy = bx - ax, by - ay, ax - ox, ay - oy
            inside ^= ((ay > oy) != (by > oy)) & (ox < ax + ((oy - ay) * ex) / ey)
            den, tn, sn = dx * ey - dy * ex, wx * ey - wy * ex, wx * dy - wy * dx
            crossed = ((den > 0.0) & (tn >= 0.0) & (sn >= 0.0) & (sn <= den)) | ((den < 0.0) & (tn <= 0.0) & (sn <= 0.0) & (sn >= den))
            q = tn / den
            t = np.where(q > 0.0, q, 0.0)
            best = np.where(crossed & np.isfinite(t) & (t < best), t, best)
    return np.where(inside, 0.0, best)


def _region_entries(o, d, xy, first, count, regs):
    """Rays (o, d: [s, 2]) against the usable regions ``regs`` of the vertex tables -> t [s, len(regs)], +inf for a miss: the slab test for
    2 vertices, the polygon rules for more."""
    t = np.full((len(o), len(regs)), np.inf)
    rect = count[regs] == 2
    f = first[regs[rect]]
    t[:, rect] = _entries(o, d, xy[f], xy[f + 1])
    for col in np.flatnonzero(~rect):
        j = regs[col]
        t[:, col] = _polygon_entries(o, d, xy[first[j]:first[j] + count[j]])
    return t


def gaze_targets_host(boxes, gaze, image_of=None, regions=None, region_image=None, region_period=0, expand=EXPAND, camera_angle=CAMERA_ANGLE):
    """``mcg_gaze_targets`` and ``mcg_gaze_targets_poly`` in numpy float64, bit for bit (include/mcgaze_hip.h, "gaze targets" and "gaze
    targets, polygonal regions").

    boxes [n,4] x1 y1 x2 y2 and gaze [n,>=3] (gx, gy, gz; -z towards the lens), read as f32 and widened; image_of [n] integers, rows with equal
    image_of being in one picture (None: all in picture 0; negative: an unusable row).  regions [m,4] rectangles -- or the mixed list of
    ``region_polygons``, or a ``PolyRegions`` (the vertex tables as the device takes them) -- with region_image [m] (None: -1): a region applies to a row iff region_image < 0, or equals image_of (region_period 0), or equals image_of % region_period.  expand: a
    looked-at head's box is grown by expand * its longer side on each side.  camera_angle: half angle in degrees of the cone around the lens
    axis inside which a gaze is "at the camera" (None: never).  Both defaults are conventions, not tuned on data.
    -> (kind int32 [n]: KIND_NONE / KIND_HEAD / KIND_REGION / KIND_CAMERA; target int32 [n]: the row or region index, else -1; t float32 [n];
    hit float32 [n,2]; mutual int32 [n]; flags int32 [n]: 2 for an unusable row) -- the dtypes the kernel writes."""
    who = 'gaze_targets_host'
    expand, cos2, period = _target_params(expand, camera_angle, region_period, who)
    b32, g32, io = _row_tables(who, boxes, gaze, image_of)
    if _holds_polygon(regions):
        regions = region_polygons(regions)
    if isinstance(regions, PolyRegions):
        xy32, start, ri = _poly_tables(who, regions, region_image)
    else:                                                         # rectangles: two vertices each, one statement of the rest
        r32, ri = _region_tables(who, regions, region_image)
        xy32, start = _as_vertices(r32)
    n, m = len(b32), len(ri)
    _check_counts(who, n, m, len(xy32))
    b, g, xy = b32.astype(np.float64), g32.astype(np.float64), xy32.astype(np.float64)
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
    r_ok, r_first, r_count = _usable_regions(xy, start)
    for picture in np.unique(io[searching]):
        rows = np.flatnonzero(usable & (io == picture))           # the candidates, ascending; the sources are among them
        src = rows[searching[rows]]
        heads = _entries(o[src], d[src], lo[rows], hi[rows])
        heads[src[:, None] == rows[None, :]] = np.inf              # every OTHER row
        applies = r_ok & ((ri < 0) | (ri == (int(picture) % period if period > 0 else int(picture))))
        regs = np.flatnonzero(applies)
        t = np.concatenate([heads, _region_entries(o[src], d[src], xy, r_first, r_count, regs)], axis=1)
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


# ---------------------------------------------------------------- gaze targets, 3-D (include/mcgaze_hip.h, "gaze targets, 3-D")
HEAD_SIZE, GAZE_FRAMES, MAX_CAMERAS = 0.24, ('camera', 'eye'), 4096       # head_size in metres and frame 'eye': conventions, not tuned on data
FIELDS_3D = FIELDS + ('hit3d',)                                  # the order of the seven tables
NAN32 = np.array([0x7fc00000], np.uint32).view(np.float32)[0]    # the one NaN ``hit`` holds


class PolyRegions3D(collections.namedtuple('PolyRegions3D', 'xyz start')):
    """The region tables of mcg_gaze_targets_3d, (xyz f32 [V, 3], start int32 [m + 1]): region j is the planar polygon of the 3 .. 32
    vertices start[j] .. start[j + 1] - 1, in camera coordinates (x right, y down, z away from the lens, metres).  The tables may be
    device tensors for DevicePipeline.gaze_targets_3d; what ``start`` HOLDS is contents, never an error."""
    __slots__ = ()


def regions_3d(regions):
    """A list of planar polygons [[x, y, z], ...] of 3 .. 32 vertices each, in camera coordinates -> PolyRegions3D(xyz f32 [V, 3], start
    int32 [m + 1]).  TypeError for what is no list of such items or holds no numbers, ValueError for an item of another shape; the VALUES
    are contents (a vertex that is not finite, or three first vertices on one line, make the region unusable, as on the device)."""
    who = 'regions_3d'
    if not isinstance(regions, (list, tuple, np.ndarray)):
        raise TypeError(f'{who}: regions is a list of polygons [[x, y, z], ...]; got {type(regions).__name__}')
    parts = []
    for j, item in enumerate(regions):
        if not isinstance(item, (list, tuple, np.ndarray)):
            raise TypeError(f'{who}: region {j} is a list of [x, y, z] vertices, got {type(item).__name__}')
        try:
            a = np.asarray(item)
        except ValueError:
            raise ValueError(f'{who}: region {j} is 3 .. {POLY_VERTS} vertices [x, y, z], got a ragged list') from None
        if a.dtype.kind not in 'fiu':
            raise TypeError(f'{who}: region {j} must hold numbers, got {a.dtype}')
        if not (a.ndim == 2 and a.shape[1] == 3 and 3 <= a.shape[0] <= POLY_VERTS):
            raise ValueError(f'{who}: region {j} is 3 .. {POLY_VERTS} vertices [x, y, z], got shape {a.shape}')
        parts.append(a.astype(np.float32))
    start = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=start[1:])
    _check_counts(who, 0, len(parts), int(start[-1]))
    return PolyRegions3D(np.concatenate(parts) if parts else np.zeros((0, 3), np.float32), start.astype(np.int32))


def _camera_table(who, cam):
    """``cam``: [fx, fy, cx, cy] or one such row per camera -> f32 [C, 4], 1 <= C <= MAX_CAMERAS (TypeError / ValueError).  The VALUES are
    contents: a camera that is not finite or has fx, fy <= 0 flags its rows."""
    c = np.asarray(_host_array(cam))
    if c.dtype.kind not in 'fiu':
        raise TypeError(f'{who}: the camera table must hold numbers fx fy cx cy, got {c.dtype}')
    c = c.reshape(1, 4) if c.shape == (4,) else c
    if c.ndim != 2 or c.shape[1] != 4 or not 1 <= c.shape[0] <= MAX_CAMERAS:
        raise ValueError(f'{who}: the camera table is [fx, fy, cx, cy] or [C, 4] with C in 1 .. {MAX_CAMERAS}, got {c.shape}')
    return np.ascontiguousarray(c, dtype=np.float32)


def _target3d_params(head_size=HEAD_SIZE, frame='eye', cam_period=0, who='gaze_targets_3d'):
    """The options of the 3-D entry, validated (ValueError) -> (head_size, frame as the entry's int, cam_period)."""
    if isinstance(head_size, bool) or not isinstance(head_size, (int, float, np.integer, np.floating)) or not (math.isfinite(head_size) and head_size > 0):
        raise ValueError(f'{who}: head_size must be a finite number of metres > 0, got {head_size!r}')
    if not isinstance(frame, str) or frame not in GAZE_FRAMES:
        raise ValueError(f"{who}: frame is 'eye' or 'camera', got {frame!r}")
    if isinstance(cam_period, bool) or not isinstance(cam_period, (int, np.integer)) or cam_period < 0:
        raise ValueError(f'{who}: cam_period must be an int >= 0, got {cam_period!r}')
    return float(head_size), GAZE_FRAMES.index(frame), int(cam_period)


def _depth_table(who, depth, n):
    """``depth``: None or [n] numbers -> None or f32 [n] (TypeError / ValueError)."""
    if depth is None:
        return None
    d = np.asarray(_host_array(depth)).reshape(-1)
    if d.size and d.dtype.kind not in 'fiu':
        raise TypeError(f'{who}: depth must hold numbers, got {d.dtype}')
    if d.shape != (n,):
        raise ValueError(f'{who}: depth must be [{n}], one per row; got {d.shape}')
    return np.ascontiguousarray(d, dtype=np.float32)


def _poly3d_tables(who, regions, region_image):
    """Host regions of the 3-D entry -- None, the list of ``regions_3d`` or a PolyRegions3D -> (f32 [V,3], int32 [m+1], int32 [m]), checked
    (TypeError / ValueError): shapes, dtypes and counts only.  region_image None: every picture (-1)."""
    if regions is None:
        if region_image is not None and np.size(_host_array(region_image)):
            raise ValueError(f'{who}: region_image without regions')
        return np.zeros((0, 3), np.float32), np.zeros(1, np.int32), np.zeros(0, np.int32)
    if not isinstance(regions, PolyRegions3D):
        regions = regions_3d(regions)
    v = np.asarray(_host_array(regions.xyz))
    if v.size == 0:
        v = v.reshape(0, 3)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype.kind not in 'fiu':
        raise ValueError(f'{who}: PolyRegions3D.xyz is the [V, 3] vertex table x y z; got {v.dtype} {v.shape}')
    s = np.asarray(_host_array(regions.start))
    if s.size and s.dtype.kind not in 'iu':
        raise TypeError(f'{who}: PolyRegions3D.start must hold integers, got {s.dtype}')
    if s.ndim != 1 or len(s) < 1:
        raise ValueError(f'{who}: PolyRegions3D.start must be [m + 1], got {s.shape}')
    m = len(s) - 1
    if region_image is None:
        ri = np.full(m, -1, np.int32)
    else:
        ri = np.asarray(_host_array(region_image)).reshape(-1)
        if ri.size and ri.dtype.kind not in 'iu':
            raise TypeError(f'{who}: region_image must hold integers, got {ri.dtype}')
        if ri.shape != (m,):
            raise ValueError(f'{who}: region_image must be [{m}], one per region; got {ri.shape}')
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(s.astype(np.int32)), np.ascontiguousarray(ri, dtype=np.int32)


def unproject(points_px, depth, cam):
    """Image points at a depth -> camera space, the header's ORIGIN rule: points_px [..., 2] pixels (u, v), depth a number or [...] metres
    along z, cam [fx, fy, cx, cy] -> float64 [..., 3] = (((u - cx) * Z) / fx, ((v - cy) * Z) / fy, Z).  How the corners of a screen marked
    in a picture, with their measured distances, become a region of ``regions_3d``."""
    p = np.asarray(points_px, dtype=np.float64)
    c = np.asarray(cam, dtype=np.float64)
    if p.ndim < 1 or p.shape[-1] != 2 or c.shape != (4,):
        raise ValueError(f'unproject: points_px is [..., 2] and cam [fx, fy, cx, cy]; got {p.shape} and {c.shape}')
    z = np.broadcast_to(np.asarray(depth, dtype=np.float64), p.shape[:-1])
    return np.stack([((p[..., 0] - c[2]) * z) / c[0], ((p[..., 1] - c[3]) * z) / c[1], z], axis=-1)


def _sqrtf(x):
    """(double)sqrtf((float)x)."""
    return np.sqrt(x.astype(np.float32)).astype(np.float64)


def _usable_regions_3d(xyz, start):
    """The header's USABLE region of the 3-D entry (xyz float64 [V,3]) -> (ok bool [m], first int64 [m], count int64 [m], N float64 [m,3],
    axis int64 [m]: the dropped one)."""
    s, e = start[:-1].astype(np.int64), start[1:].astype(np.int64)
    c = e - s
    ok = (0 <= s) & (s <= e) & (e <= len(xyz)) & (c >= 3) & (c <= POLY_VERTS)
    N, axis = np.zeros((len(s), 3)), np.zeros(len(s), np.int64)
    for j in np.flatnonzero(ok):                                  # nothing outside xyz is looked at: the offsets were checked first
        v = xyz[s[j]:e[j]]
        if not np.isfinite(v).all():
            ok[j] = False
            continue
        e1, e2 = v[1] - v[0], v[2] - v[0]
        N[j] = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        ax, ay, az = np.abs(N[j])
        axis[j] = 0 if ax >= ay and ax >= az else 1 if ay >= az else 2
        ok[j] = not (N[j, 0] == 0.0 and N[j, 1] == 0.0 and N[j, 2] == 0.0)
    return ok, s, c, N, axis


def gaze_targets_3d_host(boxes, gaze, image_of, cam, depth=None, regions=None, region_image=None, region_period=0, cam_period=0,
                         head_size=HEAD_SIZE, frame='eye', expand=EXPAND, camera_angle=CAMERA_ANGLE):
    """``mcg_gaze_targets_3d`` in numpy float64, bit for bit (include/mcgaze_hip.h, "gaze targets, 3-D"): gaze_targets_host decided in
    camera space, so that depth orders the heads along a ray and a look at a region lands inside it.

    boxes, gaze, image_of, region_image, region_period, expand, camera_angle: as gaze_targets_host takes them.  cam: [fx, fy, cx, cy] or
    [C, 4], one row per camera; row k's camera is image_of[k] (cam_period 0) or image_of[k] % cam_period.  depth: None or [n] metres along
    z; where it is not finite and positive the depth comes from the head's size: (fx * head_size) / the box's longer side.  regions: None,
    the list of ``regions_3d`` (planar polygons [[x, y, z], ...] in camera coordinates) or a PolyRegions3D.  frame: 'eye' -- the gaze is
    relative to the line from the lens to the head, as Gaze360 states it -- or 'camera': D = (-gx, -gy, gz).  head_size 0.24 m, frame,
    expand and camera_angle are conventions, not tuned on data.
    -> (kind, target, t, hit, mutual, flags as gaze_targets_host returns them -- hit is the 3-D point projected to pixels, NaN where it is
    not in front of the lens --, hit3d float32 [n,3]: the point in camera coordinates)."""
    who = 'gaze_targets_3d_host'
    expand, cos2, period = _target_params(expand, camera_angle, region_period, who)
    head_size, frame, cam_period = _target3d_params(head_size, frame, cam_period, who)
    b32, g32, io = _row_tables(who, boxes, gaze, image_of)
    cam32 = _camera_table(who, cam)
    n = len(b32)
    d32 = _depth_table(who, depth, n)
    xyz32, start, ri = _poly3d_tables(who, regions, region_image)
    _check_counts(who, n, len(ri), len(xyz32))
    b, g, xyz = b32.astype(np.float64), g32.astype(np.float64), xyz32.astype(np.float64)
    kind, target = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    t_out, hit, hit3d = np.zeros(n, np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32)
    with np.errstate(all='ignore'):
        # ---- every row in camera space.  numpy rounds every elementwise product and sum on its own: nothing is contracted, as in the kernel
        usable = np.isfinite(b).all(axis=1) & np.isfinite(g).all(axis=1) & ~(b[:, 2] < b[:, 0]) & ~(b[:, 3] < b[:, 1]) & (io >= 0)
        c = np.where(usable, io % cam_period if cam_period > 0 else io, 0)
        usable &= c < len(cam32)
        k = cam32[np.where(usable, c, 0)].astype(np.float64)
        fx, fy, cx, cy = k[:, 0], k[:, 1], k[:, 2], k[:, 3]
        usable &= np.isfinite(k).all(axis=1) & (fx > 0.0) & (fy > 0.0)
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        side = np.where(w > h, w, h)
        Z = (fx * head_size) / side
        if d32 is not None:
            dz = d32.astype(np.float64)
            Z = np.where(np.isfinite(dz) & (dz > 0.0), dz, Z)
        usable &= np.isfinite(Z) & (Z > 0.0)
        X = ((((b[:, 0] + b[:, 2]) * 0.5) - cx) * Z) / fx
        Y = ((((b[:, 1] + b[:, 3]) * 0.5) - cy) * Z) / fy
        usable &= np.isfinite(X) & np.isfinite(Y)
        flags = np.where(usable, 0, 2).astype(np.int32)
        gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
        if frame == 0:
            Dx, Dy, Dz = -gx, -gy, gz
            s = -((Dx * X + Dy * Y) + Dz * Z)
            camera = (s > 0.0) & (s * s >= cos2 * (((Dx * Dx + Dy * Dy) + Dz * Dz) * ((X * X + Y * Y) + Z * Z)))
        else:
            a2 = X * X + Z * Z
            a, r = _sqrtf(a2), _sqrtf(a2 + Y * Y)
            p, q = gx * r, gz * a
            Dx = ((q * X) - (p * Z)) + (gy * (X * Y))
            Dy = (q * Y) - (gy * a2)
            Dz = ((q * Z) + (p * X)) + (gy * (Y * Z))
            camera = (gz < 0.0) & (gz * gz >= cos2 * ((gx * gx + gy * gy) + gz * gz))
        camera &= usable
        kind[camera] = KIND_CAMERA
        searching = usable & ~camera & np.isfinite(Dx) & np.isfinite(Dy) & np.isfinite(Dz) & ~((Dx == 0.0) & (Dy == 0.0) & (Dz == 0.0))
        O, D = np.stack([X, Y, Z], axis=1), np.stack([Dx, Dy, Dz], axis=1)
        e = expand * side
        hw, hh = (((w * 0.5) + e) * Z) / fx, (((h * 0.5) + e) * Z) / fy
        half = np.stack([hw, hh, np.where(hw > hh, hw, hh)], axis=1)
        lo, hi = O - half, O + half
        r_ok, r_first, r_count, r_N, r_axis = _usable_regions_3d(xyz, start)
        best_t = np.full(n, np.inf)
        for picture in np.unique(io[searching]):
            rows = np.flatnonzero(usable & (io == picture))       # the candidates, ascending; the sources are among them
            src = rows[searching[rows]]
            o, d = O[src], D[src]
            # heads: the slab test, axes x y z
            near, far = np.full((len(src), len(rows)), -np.inf), np.full((len(src), len(rows)), np.inf)
            ok = np.ones((len(src), len(rows)), bool)
            for ax in (0, 1, 2):
                oa, da, la, ha = o[:, ax, None], d[:, ax, None], lo[None, rows, ax], hi[None, rows, ax]
                zero = np.broadcast_to(da == 0.0, ok.shape)
                t1, t2 = (la - oa) / da, (ha - oa) / da
                l, u = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
                ok &= np.where(zero, (la <= oa) & (oa <= ha), True)
                near = np.where(zero, near, np.where(l > near, l, near))
                far = np.where(zero, far, np.where(u < far, u, far))
            t = np.where(near > 0.0, near, 0.0)
            heads = np.where(ok & (near <= far) & (far >= 0.0) & np.isfinite(t), t, np.inf)
            heads[src[:, None] == rows[None, :]] = np.inf          # every OTHER row
            # regions: the plane, then the even-odd rule in the two kept coordinates
            applies = r_ok & ((ri < 0) | (ri == (int(picture) % period if period > 0 else int(picture))))
            regs = np.flatnonzero(applies)
            planes = np.full((len(src), len(regs)), np.inf)
            for col, j in enumerate(regs):
                N, v = r_N[j], xyz[r_first[j]:r_first[j] + r_count[j]]
                den = (N[0] * d[:, 0] + N[1] * d[:, 1]) + N[2] * d[:, 2]
                tn = (N[0] * (v[0, 0] - o[:, 0]) + N[1] * (v[0, 1] - o[:, 1])) + N[2] * (v[0, 2] - o[:, 2])
                q = tn / den
                met = (den != 0.0) & np.isfinite(q) & (q >= 0.0)
                t = np.where(q > 0.0, q, 0.0)
                P = o + t[:, None] * d
                iu, iv = (1 if r_axis[j] == 0 else 0), (1 if r_axis[j] == 2 else 2)
                pu, pv = P[:, iu], P[:, iv]
                inside = np.zeros(len(src), bool)
                for e_ in range(len(v)):
                    (au, av), (bu, bv) = v[e_, [iu, iv]], v[(e_ + 1) % len(v), [iu, iv]]
                    inside ^= ((av > pv) != (bv > pv)) & (pu < au + ((pv - av) * (bu - au)) / (bv - av))
                planes[:, col] = np.where(met & inside, t, np.inf)
            t = np.concatenate([heads, planes], axis=1)
            if t.shape[1] == 0:
                continue
            best = np.argmin(t, axis=1)                           # the FIRST smallest: heads before regions, then the lower index
            tb = t[np.arange(len(src)), best]
            found = tb < np.inf
            s_, best, tb = src[found], best[found], tb[found]
            is_head = best < len(rows)
            kind[s_] = np.where(is_head, KIND_HEAD, KIND_REGION)
            target[s_] = np.where(is_head, rows[np.minimum(best, len(rows) - 1)], regs[np.maximum(best - len(rows), 0)] if len(regs) else -1)
            best_t[s_] = tb
        found = np.flatnonzero((kind == KIND_HEAD) | (kind == KIND_REGION))
        tb = best_t[found]
        P = O[found] + tb[:, None] * D[found]
        t_out[found] = tb.astype(np.float32)
        hit3d[found] = P.astype(np.float32)
        u, v = fx[found] * (P[:, 0] / P[:, 2]) + cx[found], fy[found] * (P[:, 1] / P[:, 2]) + cy[found]
        front = P[:, 2] > 0.0
        hit[found, 0] = np.where(front & (u == u), u.astype(np.float32), NAN32)
        hit[found, 1] = np.where(front & (v == v), v.astype(np.float32), NAN32)
    mutual = np.zeros(n, np.int32)
    heads = np.flatnonzero(kind == KIND_HEAD)
    back = target[heads]
    mutual[heads] = (kind[back] == KIND_HEAD) & (target[back] == heads)
    return kind, target, t_out, hit, mutual, flags, hit3d


# ---------------------------------------------------------------- gaze dwell (include/mcgaze_hip.h, "gaze dwell")
DWELL_ENTER, DWELL_EXIT = 3, 2                                   # conventions, not tuned on data
END_LOOKED_AWAY, END_OWNER_LEFT, END_REPLACED, END_VIDEO_ENDED = 1, 2, 3, 4      # 4 is given on the host only (run_head_video), never by the kernel
END_NAMES = ('', 'looked_away', 'owner_left', 'replaced', 'video_ended')
STATE_WORDS = ('person', 'tag', 'cur_kind', 'cur_ident', 'cur_start', 'cur_frames', 'cur_mutual', 'gap', 'cand_kind', 'cand_ident', 'cand_start',
               'cand_frames', 'cand_mutual', 'seen', 'reserved0', 'reserved1')      # the 16 words of a column's state record, in order
STATE_INDEX = {name: k for k, name in enumerate(STATE_WORDS)}
DWELL_FIELDS = ('kind', 'ident', 'start', 'frames')              # the 4 words of a row of ``dwell``
ENDED_FIELDS = ('person', 'tag', 'kind', 'ident', 'start', 'frames', 'mutual_frames', 'reason')      # the 8 words of a row of ``ended``
EVENT_FIELDS = ('frame', 'column') + ENDED_FIELDS                # the 10 words of a row of ``events``
MAX_COLUMNS, MAX_EVENTS, MAX_DWELL_FRAMES = 4096, 65536, 65536  # the bounds of mcg_gaze_dwell (rows and regions: MAX_ROWS, MAX_REGIONS)


def _dwell_params(enter=DWELL_ENTER, exit=DWELL_EXIT, frame0=0, who='gaze_dwell'):
    """The options, validated (ValueError) -> (enter, exit, frame0) as the entry takes them."""
    for name, v, lo, hi in (('enter', enter, 1, MAX_DWELL_FRAMES), ('exit', exit, 0, MAX_DWELL_FRAMES), ('frame0', frame0, 0, 2 ** 31 - 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} must be an int in {lo} .. {hi}, got {v!r}')
    return int(enter), int(exit), int(frame0)


def _dwell_options(who, dwell, attention):
    """The ``dwell=`` option of LiveGaze and run_head_video, validated (ValueError) -> None (off) or dict(enter=, exit=).  dwell: None, True
    or dict(enter=, exit=); it needs ``attention`` (the targets it accumulates)."""
    if dwell is None:
        return None
    if dwell is not True and not isinstance(dwell, dict):
        raise ValueError(f'{who}: dwell is None, True or a dict of enter and exit; got {dwell!r}')
    if attention is None:
        raise ValueError(f'{who}: dwell accumulates the targets of attention=...; give attention as well')
    opts = {} if dwell is True else dict(dwell)
    if set(opts) - {'enter', 'exit'}:
        raise ValueError(f'{who}: dwell takes enter and exit; got {sorted(opts)}')
    enter, exit, _ = _dwell_params(opts.get('enter', DWELL_ENTER), opts.get('exit', DWELL_EXIT), 0, f'{who}(dwell=...)')
    return dict(enter=enter, exit=exit)


def _dwell_counts(who, F, R, m, max_events):
    """The counts of one call, checked (ValueError) -> max_events (None: F * R, every row can end an episode)."""
    if not 1 <= R <= MAX_COLUMNS:
        raise ValueError(f'{who}: 1 .. {MAX_COLUMNS} columns per call (got {R})')
    if F * R > MAX_ROWS:
        raise ValueError(f'{who}: frames x columns must not exceed {MAX_ROWS} per call (got {F} x {R})')
    if m > MAX_REGIONS:
        raise ValueError(f'{who}: at most {MAX_REGIONS} regions per call (got {m})')
    if max_events is None:
        return F * R
    if isinstance(max_events, bool) or not isinstance(max_events, (int, np.integer)) or not 0 <= max_events <= MAX_EVENTS:
        raise ValueError(f'{who}: max_events is None or an int in 0 .. {MAX_EVENTS}, got {max_events!r}')
    return int(max_events)


def _dwell_tables(who, person, kind, ident, mutual, tag):
    """Host tables -> five int32 [F, R] arrays (tag None: zeros), checked (TypeError / ValueError)."""
    out, shape = [], None
    for name, t in (('person', person), ('kind', kind), ('ident', ident), ('mutual', mutual), ('tag', tag)):
        if t is None and name == 'tag':
            out.append(np.zeros(shape, np.int32))
            continue
        a = np.asarray(_host_array(t))
        if a.dtype.kind not in 'iub':
            raise TypeError(f'{who}: {name} must hold integers, got {a.dtype}')
        if a.ndim != 2 or (shape is not None and a.shape != shape):
            raise ValueError(f'{who}: person, kind, ident, mutual and tag are [F, R] tables of one shape; {name} is {a.shape}' +
                             (f', person {shape}' if shape is not None else ''))
        shape = a.shape
        out.append(np.ascontiguousarray(a.astype(np.int32)))
    return out


def _dwell_events(ended, frame0, E):
    """The rows of ended [F, R, 8] that are not all zero, in ascending (frame, column) -> (events [E, 10], num_events [1])."""
    F, R = ended.shape[:2]
    f, c = np.nonzero(ended.any(axis=2))                          # row-major: ascending (frame, column)
    events = np.zeros((E, 10), np.int32)
    keep = min(E, len(f))
    events[:keep, 0] = ((frame0 + f[:keep].astype(np.int64)) & 0xffffffff).astype(np.uint32).view(np.int32)
    events[:keep, 1] = c[:keep]
    events[:keep, 2:] = ended[f[:keep], c[:keep]]
    return events, np.asarray([len(f)], np.int32)


def gaze_dwell_host(person, kind, ident, mutual, tag=None, state=None, frame0=0, enter=DWELL_ENTER, exit=DWELL_EXIT, region_frames=None,
                    max_events=None):
    """``mcg_gaze_dwell`` in numpy, bit for bit (include/mcgaze_hip.h, "gaze dwell"): the per-frame targets of F frames of R columns (a column
    is a tracker slot or a lane) become debounced episodes, walked in frame order.

    person [F, R]: > 0 the id of the person with a usable result there, <= 0 nobody; tag [F, R]: the second half of the identity (None:
    zeros); kind, ident, mutual [F, R]: what the person looks at -- kind in gaze_targets' values, ident the looked-at person's track id for a
    head and the region's index for a region.  state: int32 [R, 16] (STATE_WORDS), None: the empty state, all zero; it is NOT changed, the
    updated copy is returned.  frame0: the number of frame 0.  enter: the consecutive frames an observation must repeat to become the
    current target; exit: the consecutive frames the current target may go unobserved before its episode ends (the defaults, 3 and 2, are
    conventions, not tuned on data).  region_frames: int32 [M] totals to add to (None: no regions).  max_events: the rows of the event table
    (None: F * R).
    -> (dwell int32 [F, R, 4] = DWELL_FIELDS after every frame, ended int32 [F, R, 8] = ENDED_FIELDS of the episode that ended there, else
    zero, events int32 [max_events, 10] = EVENT_FIELDS in ascending (frame, column), rows behind the count zero, num_events int32 [1]: the
    episodes that ended in this call, those beyond max_events included, state int32 [R, 16], region_frames int32 [M])."""
    who = 'gaze_dwell_host'
    enter, exit, frame0 = _dwell_params(enter, exit, frame0, who)
    P, K, I, MU, T = _dwell_tables(who, person, kind, ident, mutual, tag)
    F, R = P.shape
    rf = np.zeros(0, np.int32) if region_frames is None else np.array(_host_array(region_frames), dtype=np.int32).reshape(-1)
    E = _dwell_counts(who, F, R, len(rf), max_events)
    M = len(rf)
    if state is None:
        s = np.zeros((R, 16), np.int32)
    else:
        s = np.asarray(_host_array(state))
        if s.shape != (R, 16) or s.dtype.kind not in 'iu':
            raise ValueError(f'{who}: the state is an integer [{R}, 16] table, got {s.dtype} {s.shape}')
        s = np.array(s, dtype=np.int32)
    u, rfu = s.view(np.uint32), rf.view(np.uint32)               # every sum is unsigned, modulo 2^32; every comparison reads the int32
    dwell, ended = np.zeros((F, R, 4), np.int32), np.zeros((F, R, 8), np.int32)
    one = np.uint32(1)
    for f in range(F):
        n = np.asarray([(frame0 + f) & 0xffffffff], np.uint32).view(np.int32)[0]
        p = np.where(P[f] > 0, P[f], 0)
        g = np.where(p != 0, T[f], 0)
        k = np.where((K[f] >= 1) & (K[f] <= 3), K[f], 0)
        i = np.where((k == 1) | (k == 2), I[f], 0)
        m = ((k == 1) & (MU[f] != 0)).astype(np.uint32)
        e = ended[f]

        def end(rows, reason):
            e[rows, :7] = s[rows, :7]                             # person, tag, cur_kind, cur_ident, cur_start, cur_frames, cur_mutual
            e[rows, 7] = reason

        # A. owner
        left = (s[:, 0] != 0) & ((s[:, 0] != p) | (s[:, 1] != g))
        end(left & (s[:, 2] != 0), END_OWNER_LEFT)
        s[left] = 0
        live = p != 0
        s[live, 0], s[live, 1] = p[live], g[live]
        # B. raw person-frames
        u[live, 13] += one
        hit = live & (k == 2) & (i >= 0) & (i < M)
        np.add.at(rfu, i[hit], one)
        # C. the current target
        has = live & (s[:, 2] != 0)
        same = has & (k == s[:, 2]) & (i == s[:, 3])
        u[same, 5] += one + u[same, 7]
        s[same, 7] = 0
        u[same, 6] += m[same]
        s[same, 8:13] = 0
        other = has & ~same
        u[other, 7] += one
        away = other & (s[:, 7] > exit)
        end(away, END_LOOKED_AWAY)
        s[away, 2:8] = 0
        # D. the candidate
        d = live & ~same
        s[d & (k == 0), 8:13] = 0
        cont = d & (k != 0) & (k == s[:, 8]) & (i == s[:, 9])
        fresh = d & (k != 0) & ~cont
        u[cont, 11] += one
        u[cont, 12] += m[cont]
        s[fresh, 8], s[fresh, 9], s[fresh, 10], s[fresh, 11], u[fresh, 12] = k[fresh], i[fresh], n, 1, m[fresh]
        prom = d & (s[:, 11] >= enter)
        end(prom & (s[:, 2] != 0), END_REPLACED)
        s[prom, 2:7] = s[prom, 8:13]
        s[prom, 7] = 0
        s[prom, 8:13] = 0
        # E. outputs
        dwell[f] = np.where(live[:, None], s[:, 2:6], 0)
    events, num = _dwell_events(ended, frame0, E)
    return dwell, ended, events, num, s, rf


def open_episodes(state):
    """The episodes still open in a state [R, 16] -> (columns, rows [len, 7] = the first seven ENDED_FIELDS), in ascending column."""
    s = np.asarray(_host_array(state)).reshape(-1, 16)
    cols = np.flatnonzero((s[:, 0] != 0) & (s[:, 2] != 0))
    return cols, s[cols, :7]


def region_label_rows(regions, region_image, names, num_images, region_period=0):
    """The rows that name the regions in the pictures, for ``DevicePipeline.draw_labels`` / ``arrows.draw_labels_host``: one row per (picture,
    named region) that draw_attention would draw the region's outline into -- the region usable, and region_image < 0, == p, or with a
    region_period == p % region_period.  regions, region_image, region_period: as gaze_targets_host takes them, on the HOST (TypeError for a
    device table: nothing is read back); names: one string per region, None or '' for a region without a name; num_images pictures.
    -> (boxes f32 [r,4]: the bounding box of the region's vertices; image_of int32 [r]; text uint8 [r,24] (``encode_labels``); place int32 [r],
    all 1: inside the box's top-left corner), pictures ascending and regions ascending inside a picture."""
    from . import arrows as R                                     # (arrows imports this module)
    who = 'region_label_rows'
    parts = (*regions, region_image) if isinstance(regions, PolyRegions) else (regions, region_image)
    if any(type(t).__module__.startswith('torch') and getattr(t, 'is_cuda', False) for t in parts):
        raise TypeError(f'{who}: regions on the host only; device tables are not read back')
    _, _, period = _target_params(region_period=region_period, who=who)
    xy, start, ri = R._overlay_regions(who, regions, region_image)
    if names is None or len(names) != len(ri):
        raise ValueError(f'{who}: names must hold one entry per region ({len(ri)}), got {None if names is None else len(names)}')
    text = R.encode_labels(['' if s is None else s for s in names])
    corners, _ = R.region_outlines(xy, start)
    rows = [(p, j) for p in range(int(num_images)) for j in range(len(ri))
            if text[j, 0] and corners[j] is not None and (ri[j] < 0 or ri[j] == p or (period > 0 and ri[j] == p % period))]
    boxes = np.zeros((len(rows), 4), dtype=np.float32)
    for k, (_, j) in enumerate(rows):
        v = xy[start[j]:start[j + 1]]
        boxes[k] = (v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max())
    regs = np.array([j for _, j in rows], dtype=np.int64)
    return boxes, np.array([p for p, _ in rows], dtype=np.int32), text[regs].reshape(-1, R.LABEL_CHARS), np.ones(len(rows), dtype=np.int32)


# ---------------------------------------------------------------- gaze heat map (include/mcgaze_hip.h, "gaze heat map")
HeatState = collections.namedtuple('HeatState', 'heat peak cell_shift')   # heat int32 [C, GH, GW], peak int32 [C]; a cell is 2^cell_shift pixels square
HEAT_KINDS = ('head', 'region')                                  # the rows that count by default: a look that lands on something in the picture
HEAT_MAX_CAMERAS, HEAT_MAX_SIDE, HEAT_MAX_CELLS, HEAT_COORD = 4096, 8192, 1 << 24, 8191
HEAT_MAX = 2 ** 31 - 1


def _heat_cell(who, cell):
    """``cell``, the side of a cell in pixels: a power of two in 1 .. 64 (ValueError) -> cell_shift."""
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or not 1 <= cell <= 64 or cell & (cell - 1):
        raise ValueError(f'{who}: cell must be a power of two in 1 .. 64 (pixels a side), got {cell!r}')
    return int(cell).bit_length() - 1


def _heat_kinds(who, kinds):
    """``kinds``: the bit mask the entry takes, or names out of KIND_NAMES (ValueError) -> the bit mask."""
    if isinstance(kinds, (int, np.integer)) and not isinstance(kinds, bool):
        if not 0 <= kinds <= 15:
            raise ValueError(f'{who}: kinds as a bit mask is 0 .. 15, got {kinds!r}')
        return int(kinds)
    names = [kinds] if isinstance(kinds, str) else list(kinds)
    if any(k not in KIND_NAMES for k in names):
        raise ValueError(f'{who}: kinds holds names out of {KIND_NAMES}, got {kinds!r}')
    return sum({1 << KIND_NAMES.index(k) for k in names})


def _heat_params(who, cell_shift, radius, kinds, period, decay):
    """The options of one accumulation, validated (ValueError) -> (cell_shift, radius, kinds as a bit mask, period, decay_shift)."""
    for name, v, lo, hi in (('cell_shift', cell_shift, 0, 6), ('radius', radius, 0, 8), ('period', period, 0, 2 ** 31 - 1), ('decay', decay, 0, 30)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} must be an int in {lo} .. {hi}, got {v!r}')
    return int(cell_shift), int(radius), _heat_kinds(who, kinds), int(period), int(decay)


def _heat_grid(who, shape):
    """The shape of a heat grid, checked against the entry's limits (ValueError) -> (C, GH, GW)."""
    if len(shape) != 3 or not (1 <= shape[0] <= HEAT_MAX_CAMERAS and 1 <= shape[1] <= HEAT_MAX_SIDE and 1 <= shape[2] <= HEAT_MAX_SIDE) or \
            shape[0] * shape[1] * shape[2] > HEAT_MAX_CELLS:
        raise ValueError(f'{who}: heat is [C, GH, GW] with C in 1 .. {HEAT_MAX_CAMERAS}, GH and GW in 1 .. {HEAT_MAX_SIDE} and at most 2^24 cells; '
                         f'got {tuple(shape)}')
    return tuple(int(v) for v in shape)


def _heat_options(who, heat, attention, draw):
    """The ``heat=`` option of LiveGaze and run_head_video, validated (ValueError) -> None (off) or dict(cell, radius, decay, kinds, draw,
    full_scale, min_level).  heat: None / False, True or a dict of those; it needs ``attention`` (whose hit points it accumulates), and with
    draw=True it needs ``draw`` (the frames it is blended into)."""
    if heat is None or heat is False:
        return None
    if heat is not True and not isinstance(heat, dict):
        raise ValueError(f'{who}: heat is None, True or a dict of cell, radius, decay, kinds, draw, full_scale and min_level; got {heat!r}')
    opts = dict(cell=8, radius=2, decay=0, kinds=HEAT_KINDS, draw=True, full_scale=None, min_level=1)
    given = {} if heat is True else dict(heat)
    if set(given) - set(opts):
        raise ValueError(f'{who}: heat takes {sorted(opts)}; got {sorted(given)}')
    if attention is None:
        raise ValueError(f'{who}: heat accumulates the hit points of attention=...; give attention as well')
    if heat is True:
        opts['draw'] = bool(draw)                                 # heat=True: drawn where frames are drawn at all
    opts.update(given)
    if not isinstance(opts['draw'], (bool, np.bool_)):
        raise ValueError(f"{who}: heat's draw is True or False, got {opts['draw']!r}")
    if opts['draw'] and not draw:
        raise ValueError(f'{who}: heat with draw=True is blended into the frames draw hands out: it needs draw')
    _heat_cell(f'{who}(heat=...)', opts['cell'])
    _heat_params(f'{who}(heat=...)', 0, opts['radius'], opts['kinds'], 0, opts['decay'])
    _heat_scale(f'{who}(heat=...)', opts['full_scale'], opts['min_level'])
    return opts


def _heat_scale(who, full_scale, min_level):
    """full_scale (None: the peak; else an int in 1 .. 2^31 - 1) and min_level (1 .. 255), validated (ValueError)."""
    if full_scale is not None and (isinstance(full_scale, bool) or not isinstance(full_scale, (int, np.integer)) or not 1 <= full_scale <= HEAT_MAX):
        raise ValueError(f'{who}: full_scale is None (the peak) or an int in 1 .. 2^31 - 1, got {full_scale!r}')
    if isinstance(min_level, bool) or not isinstance(min_level, (int, np.integer)) or not 1 <= min_level <= 255:
        raise ValueError(f'{who}: min_level must be an int in 1 .. 255, got {min_level!r}')
    return None if full_scale is None else int(full_scale), int(min_level)


def heat_grid_shape(frame_hw, cell=8):
    """(GH, GW) of the grid that covers an h x w frame with cells of ``cell`` pixels a side: ceil(h / cell), ceil(w / cell)."""
    _heat_cell('heat_grid_shape', cell)
    h, w = (int(v) for v in frame_hw)
    if h < 1 or w < 1:
        raise ValueError(f'heat_grid_shape: a frame of at least one pixel, got {h} x {w}')
    return -(-h // cell), -(-w // cell)


def gaze_heat_host(hit, kind, image_of, heat, flags=None, mask=None, cell_shift=3, radius=2, kinds=HEAT_KINDS, period=0, decay=0):
    """``mcg_gaze_heat_add`` in numpy, bit for bit (include/mcgaze_hip.h, "gaze heat map"): the hit points of the rows that count, splatted
    into the grid of their camera.  hit [n,2] (read as f32), kind, image_of [n] integers, flags / mask [n] integers or None; heat: int32
    [C, GH, GW], the grid as it stood (not changed); cell_shift 0 .. 6, radius 0 .. 8 cells, kinds: names out of KIND_NAMES or the bit
    mask, period as in the header, decay: the decay shift, 0 .. 30, 0 off.
    A row counts iff flags is None or 0, mask is None or not 0, kind in 0 .. 3 with its bit in ``kinds``, image_of >= 0, its camera
    (image_of, or image_of % period) below C, and both rounded hit coordinates finite and within +-8191.  It adds
    (radius + 1 - |dx|) (radius + 1 - |dy|) to every cell within ``radius`` of its own; taps off the grid are dropped.  Each cell: a negative
    value counts as 0, then h -= h >> decay (once per call), then the taps, saturated at 2^31 - 1.
    -> (heat int32 [C, GH, GW], peak int32 [C]: each camera's maximum)."""
    who = 'gaze_heat_host'
    cell_shift, radius, kinds, period, decay = _heat_params(who, cell_shift, radius, kinds, period, decay)
    heat = np.asarray(_host_array(heat))
    if heat.dtype != np.int32:
        raise TypeError(f'{who}: heat must be int32, got {heat.dtype}')
    C, GH, GW = _heat_grid(who, heat.shape)
    hit = np.asarray(_host_array(hit), dtype=np.float32)
    hit = hit.reshape(0, 2) if hit.size == 0 else hit
    n = len(hit)
    if hit.ndim != 2 or hit.shape[1] != 2 or n > MAX_ROWS:
        raise ValueError(f'{who}: hit must be [n, 2] with n <= {MAX_ROWS}, got {hit.shape}')
    ints = {}
    for name, t in (('kind', kind), ('image_of', image_of), ('flags', flags), ('mask', mask)):
        if t is None:
            if name in ('kind', 'image_of'):
                raise ValueError(f'{who}: {name} is required')
            continue
        a = np.asarray(_host_array(t)).reshape(-1)
        if a.size and a.dtype.kind not in 'iub':
            raise TypeError(f'{who}: {name} must hold integers, got {a.dtype}')
        if a.shape != (n,):
            raise ValueError(f'{who}: {name} must be [{n}], one per row; got {a.shape}')
        ints[name] = a.astype(np.int64)
    kd, io = ints['kind'], ints['image_of']
    ok = np.ones(n, dtype=bool)
    if 'flags' in ints:
        ok &= ints['flags'] == 0
    if 'mask' in ints:
        ok &= ints['mask'] != 0
    ok &= (kd >= 0) & (kd <= 3) & (((kinds >> np.clip(kd, 0, 3)) & 1) != 0)
    ok &= io >= 0
    cam = np.where(io >= 0, io % period if period else io, 0)
    ok &= cam < C
    with np.errstate(invalid='ignore'):
        h64 = np.rint(hit.astype(np.float64))                     # half to even
        ok &= (np.abs(h64) <= HEAT_COORD).all(axis=1)             # (a NaN fails the comparison)
    rows = np.flatnonzero(ok)
    taps = np.zeros((C, GH, GW), dtype=np.int64)
    if len(rows):
        cell = h64[rows].astype(np.int64) >> cell_shift           # arithmetic: floors
        d = np.arange(-radius, radius + 1, dtype=np.int64)
        wgt = radius + 1 - np.abs(d)
        x, y = cell[:, 0, None, None] + d[None, None, :], cell[:, 1, None, None] + d[None, :, None]      # [rows, dy, dx]
        x, y = np.broadcast_arrays(x, y)
        w = np.broadcast_to(wgt[None, :, None] * wgt[None, None, :], x.shape)
        c = np.broadcast_to(cam[rows][:, None, None], x.shape)
        inside = (x >= 0) & (x < GW) & (y >= 0) & (y < GH)
        np.add.at(taps, (c[inside], y[inside], x[inside]), w[inside])
    h = np.maximum(heat.astype(np.int64), 0)
    if decay:
        h -= h >> decay
    out = np.minimum(h + taps, HEAT_MAX).astype(np.int32)
    return out, out.reshape(C, -1).max(axis=1).astype(np.int32)


# ---------------------------------------------------------------- surface heat map (include/mcgaze_hip.h, "surface heat map")
SurfaceHeatState = collections.namedtuple('SurfaceHeatState', 'heat peak')     # heat int32 [M, GH, GW], peak int32 [M]: one grid per region
SURFACE_GRID, SURFACE_RADIUS = (32, 32), 1                       # (GW, GH) and the splat's radius in cells: conventions, not tuned on data
SURFACE_MAX_SIDE, SURFACE_COORD = 1024, 16384
CHART_FIELDS = ('v0x', 'v0y', 'v0z', 'ax', 'ay', 'az', 'bx', 'by', 'bz', 'Nx', 'Ny', 'Nz', 'aa', 'bb', 'smin', 'ws', 'rmin', 'hr', 'usable', 'axis')
CHART_INDEX = {name: k for k, name in enumerate(CHART_FIELDS)}   # the 20 doubles of a chart, MCG_SURFACE_CHART_BYTES = 160


def _surface_regions(who, regions):
    """``regions`` of the surface entries -- the list of ``regions_3d`` or a PolyRegions3D, at least one region -> (xyz f32 [V,3], start
    int32 [M+1]), checked (TypeError / ValueError): shapes, dtypes and counts only."""
    if regions is None:
        raise ValueError(f'{who}: regions are required: the list of regions_3d or a PolyRegions3D')
    xyz, start, _ = _poly3d_tables(who, regions, None)
    if len(start) < 2:
        raise ValueError(f'{who}: at least one region')
    _check_counts(who, 0, len(start) - 1, len(xyz))
    return xyz, start


def _surface_grid(who, shape):
    """The shape of the grids, checked against the entries' limits (ValueError) -> (M, GH, GW)."""
    if len(shape) != 3 or not (1 <= shape[0] <= MAX_REGIONS and 1 <= shape[1] <= SURFACE_MAX_SIDE and 1 <= shape[2] <= SURFACE_MAX_SIDE) or \
            shape[0] * shape[1] * shape[2] > HEAT_MAX_CELLS:
        raise ValueError(f'{who}: heat is [M, GH, GW] with M in 1 .. {MAX_REGIONS}, GH and GW in 1 .. {SURFACE_MAX_SIDE} and at most 2^24 cells; '
                         f'got {tuple(shape)}')
    return tuple(int(v) for v in shape)


def _surface_params(who, radius, decay):
    """radius 0 .. 8 and decay 0 .. 30, validated (ValueError)."""
    for name, v, lo, hi in (('radius', radius, 0, 8), ('decay', decay, 0, 30)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f'{who}: {name} must be an int in {lo} .. {hi}, got {v!r}')
    return int(radius), int(decay)


def _surface_grid_option(who, grid):
    """``grid`` = (GW, GH), two ints in 1 .. 1024 (ValueError) -> (GW, GH)."""
    ok = isinstance(grid, (tuple, list)) and len(grid) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and
                                                                   1 <= v <= SURFACE_MAX_SIDE for v in grid)
    if not ok:
        raise ValueError(f'{who}: grid is (GW, GH), two ints in 1 .. {SURFACE_MAX_SIDE}; got {grid!r}')
    return int(grid[0]), int(grid[1])


def _surface_options(who, surface_heat, attention, draw):
    """The ``surface_heat=`` option of LiveGaze and run_head_video, validated (ValueError) -> None (off) or dict(grid, radius, decay, draw,
    full_scale, min_level).  surface_heat: None / False, True or a dict of those.  It accumulates hit3d of attention=dict(camera=...,
    regions3d=...) on those regions and needs both; with draw=True it needs ``draw`` (the frames it is blended into).  surface_heat=True
    draws where frames are drawn at all.  grid (32, 32) and radius 1 are conventions, not tuned on data."""
    if surface_heat is None or surface_heat is False:
        return None
    if surface_heat is not True and not isinstance(surface_heat, dict):
        raise ValueError(f'{who}: surface_heat is None, True or a dict of grid, radius, decay, draw, full_scale and min_level; got {surface_heat!r}')
    opts = dict(grid=SURFACE_GRID, radius=SURFACE_RADIUS, decay=0, draw=True, full_scale=None, min_level=1)
    given = {} if surface_heat is True else dict(surface_heat)
    if set(given) - set(opts):
        raise ValueError(f'{who}: surface_heat takes {sorted(opts)}; got {sorted(given)}')
    three_d = None if attention is None else attention[2].get('three_d')
    if three_d is None or len(three_d['regions'].start) < 2:
        raise ValueError(f'{who}: surface_heat accumulates hit3d on planar regions: give attention=dict(camera=..., regions3d=...) as well')
    if surface_heat is True:
        opts['draw'] = bool(draw)
    opts.update(given)
    if not isinstance(opts['draw'], (bool, np.bool_)):
        raise ValueError(f"{who}: surface_heat's draw is True or False, got {opts['draw']!r}")
    if opts['draw'] and not draw:
        raise ValueError(f'{who}: surface_heat with draw=True is blended into the frames draw hands out: it needs draw')
    opts['grid'] = _surface_grid_option(f'{who}(surface_heat=...)', opts['grid'])
    _surface_grid(f'{who}(surface_heat=...)', (len(three_d['regions'].start) - 1, opts['grid'][1], opts['grid'][0]))
    _surface_params(f'{who}(surface_heat=...)', opts['radius'], opts['decay'])
    _heat_scale(f'{who}(surface_heat=...)', opts['full_scale'], opts['min_level'])
    return opts


def surface_charts_host(regions):
    """The CHART of every region ("surface heat map"), what the plan launch of mcg_surface_heat_add and mcg_draw_surface_heat writes, bit
    for bit -> float64 [M, 20], the columns CHART_FIELDS: v0, a = v1 - v0, b = N x a, N, aa, bb, smin, ws, rmin, hr, usable (1 / 0) and the
    dropped axis.  A region that is not usable, or whose aa, bb, ws or hr is not finite and positive, has a row of zeros.  regions: the
    list of ``regions_3d`` or a PolyRegions3D."""
    xyz32, start = _surface_regions('surface_charts_host', regions)
    xyz = xyz32.astype(np.float64)
    ok, first, count, N, axis = _usable_regions_3d(xyz, start)
    out = np.zeros((len(first), len(CHART_FIELDS)))
    with np.errstate(all='ignore'):
        for j in np.flatnonzero(ok):
            v = xyz[first[j]:first[j] + count[j]]
            v0, a, n = v[0], v[1] - v[0], N[j]
            b = np.array([n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0]])
            aa, bb = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
            w = v - v0
            s = ((w[:, 0] * a[0] + w[:, 1] * a[1]) + w[:, 2] * a[2]) / aa
            r = ((w[:, 0] * b[0] + w[:, 1] * b[1]) + w[:, 2] * b[2]) / bb
            smin = smax = s[0]
            rmin = rmax = r[0]
            for k in range(1, len(v)):                           # each written as the comparison it stands for: a NaN replaces nothing
                smin, smax = (s[k] if s[k] < smin else smin), (s[k] if s[k] > smax else smax)
                rmin, rmax = (r[k] if r[k] < rmin else rmin), (r[k] if r[k] > rmax else rmax)
            ws, hr = smax - smin, rmax - rmin
            if all(np.isfinite(x) and x > 0.0 for x in (aa, bb, ws, hr)):
                out[j] = (*v0, *a, *b, *n, aa, bb, smin, ws, rmin, hr, 1.0, float(axis[j]))
    return out


def surface_extent(regions):
    """The sides of every chart's rectangle in METRES -> float64 [M, 2] = (ws * |a|, hr * |b|), width along a = v1 - v0 and height along
    N x a; zeros for a chart that is not usable.  Host only (the one square root of this section): for showing an exported grid at the
    right aspect."""
    c = surface_charts_host(regions)
    return np.stack([c[:, CHART_INDEX['ws']] * np.sqrt(c[:, CHART_INDEX['aa']]), c[:, CHART_INDEX['hr']] * np.sqrt(c[:, CHART_INDEX['bb']])], axis=1)


def surface_coords(charts, j, Q, GW, GH):
    """fu, fv of the points Q float64 [..., 3] in the charts of the regions j [...] (usable ones) -> (fu, fv) float64 [...], as the header
    writes them; the caller silences the floating-point warnings."""
    c = charts[j]
    wx, wy, wz = Q[..., 0] - c[..., 0], Q[..., 1] - c[..., 1], Q[..., 2] - c[..., 2]
    s = ((wx * c[..., 3] + wy * c[..., 4]) + wz * c[..., 5]) / c[..., 12]
    r = ((wx * c[..., 6] + wy * c[..., 7]) + wz * c[..., 8]) / c[..., 13]
    return ((s - c[..., 14]) / c[..., 15]) * float(GW), ((r - c[..., 16]) / c[..., 17]) * float(GH)


def surface_heat_host(hit3d, kind, target, regions, heat, flags=None, mask=None, radius=SURFACE_RADIUS, decay=0):
    """``mcg_surface_heat_add`` in numpy, bit for bit (include/mcgaze_hip.h, "surface heat map"): the 3-D hit points of the rows that look
    at a region, taken into that region's chart and splatted into its grid.  hit3d [n,3] (read as f32), kind, target [n] integers --
    gaze_targets_3d's results --, flags / mask [n] integers or None; regions: the list of ``regions_3d`` or a PolyRegions3D; heat: int32
    [M, GH, GW], the grids as they stood (not changed); radius 0 .. 8 cells, decay: the decay shift, 0 .. 30, 0 off.
    A row counts iff flags is None or 0, mask is None or not 0, kind == 2, 0 <= target < M, that region's chart is usable, hit3d is finite
    and both grid coordinates are finite and within +-16384.  The splat, the update and the peak are gaze_heat_host's.
    -> (heat int32 [M, GH, GW], peak int32 [M]: each region's maximum)."""
    who = 'surface_heat_host'
    radius, decay = _surface_params(who, radius, decay)
    xyz32, start = _surface_regions(who, regions)
    heat = np.asarray(_host_array(heat))
    if heat.dtype != np.int32:
        raise TypeError(f'{who}: heat must be int32, got {heat.dtype}')
    M, GH, GW = _surface_grid(who, heat.shape)
    if M != len(start) - 1:
        raise ValueError(f'{who}: heat holds {M} grids for {len(start) - 1} regions')
    hit = np.asarray(_host_array(hit3d), dtype=np.float32)
    hit = hit.reshape(0, 3) if hit.size == 0 else hit
    n = len(hit)
    if hit.ndim != 2 or hit.shape[1] != 3 or n > MAX_ROWS:
        raise ValueError(f'{who}: hit3d must be [n, 3] with n <= {MAX_ROWS}, got {hit.shape}')
    ints = {}
    for name, t in (('kind', kind), ('target', target), ('flags', flags), ('mask', mask)):
        if t is None:
            if name in ('kind', 'target'):
                raise ValueError(f'{who}: {name} is required')
            continue
        a = np.asarray(_host_array(t)).reshape(-1)
        if a.size and a.dtype.kind not in 'iub':
            raise TypeError(f'{who}: {name} must hold integers, got {a.dtype}')
        if a.shape != (n,):
            raise ValueError(f'{who}: {name} must be [{n}], one per row; got {a.shape}')
        ints[name] = a.astype(np.int64)
    charts = surface_charts_host(PolyRegions3D(xyz32, start))
    ok = np.ones(n, dtype=bool)
    if 'flags' in ints:
        ok &= ints['flags'] == 0
    if 'mask' in ints:
        ok &= ints['mask'] != 0
    tg = ints['target']
    ok &= (ints['kind'] == KIND_REGION) & (tg >= 0) & (tg < M)
    j = np.where(ok, tg, 0)
    ok &= charts[j, CHART_INDEX['usable']] != 0.0
    Q = hit.astype(np.float64)
    ok &= np.isfinite(Q).all(axis=1)
    with np.errstate(all='ignore'):
        fu, fv = surface_coords(charts, j, Q, GW, GH)
        ok &= (np.abs(fu) <= SURFACE_COORD) & (np.abs(fv) <= SURFACE_COORD)      # (a NaN fails the comparison)
    rows = np.flatnonzero(ok)
    taps = np.zeros((M, GH, GW), dtype=np.int64)
    if len(rows):
        cell = np.stack([np.floor(fu[rows]), np.floor(fv[rows])], axis=1).astype(np.int64)
        d = np.arange(-radius, radius + 1, dtype=np.int64)
        wgt = radius + 1 - np.abs(d)
        x, y = cell[:, 0, None, None] + d[None, None, :], cell[:, 1, None, None] + d[None, :, None]      # [rows, dy, dx]
        x, y = np.broadcast_arrays(x, y)
        w = np.broadcast_to(wgt[None, :, None] * wgt[None, None, :], x.shape)
        c = np.broadcast_to(j[rows][:, None, None], x.shape)
        inside = (x >= 0) & (x < GW) & (y >= 0) & (y < GH)
        np.add.at(taps, (c[inside], y[inside], x[inside]), w[inside])
    h = np.maximum(heat.astype(np.int64), 0)
    if decay:
        h -= h >> decay
    out = np.minimum(h + taps, HEAT_MAX).astype(np.int32)
    return out, out.reshape(M, -1).max(axis=1).astype(np.int32)
