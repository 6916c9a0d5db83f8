"""Gaze arrows on the host (include/mcgaze_hip.h, "annotated frames out"): the plan (``arrow_segments``), the capsule coverage
(``segment_coverage``) and ``draw_arrows_host``, which draws in numpy what ``DevicePipeline.draw_arrows`` writes on the device, bit for bit.
``draw_attention_host`` is the same for the attention overlay ("attention overlay": region outlines, sight lines, arrows coloured by their
target), what ``DevicePipeline.draw_attention`` writes."""
import numpy as np

from . import attention as A
from .nv12 import _nv12_planes, _pixel_format, bgr_to_yuv
from .staging import _bgr_frame, _host_array

ARROW_COLOR = (230, 253, 11)                                     # the demo's, BGR (MCGaze_demo/demo.ipynb, cell 5)
ARROW_COORD, ARROW_SIDE = 8191, 8192                             # the bound under which the coverage test is exact in 64-bit integers
# The overlay's default colours, B, G, R: none (the demo's arrow), head, region, camera, mutual, a region's outline, the outline of a region
# that is looked at.  A convention, not tuned: seven colours that differ.
OVERLAY_PALETTE = (ARROW_COLOR, (0, 165, 255), (0, 255, 0), (255, 0, 255), (0, 0, 255), (160, 160, 160), (0, 255, 255))
OVERLAY_ACTIVE = 1 << 20                                         # num_images * m of mcg_draw_attention


def _arrow_params(length=1.0, min_thickness=5, thickness_ratio=0.01, tip_length=0.1, lowest=1):
    """The arrow parameters, validated (ValueError) -> (length, min_thickness, thickness_ratio, tip_length); the defaults are the demo's.
    lowest: the least min_thickness (the overlay takes 0, "no arrows")."""
    length, thickness_ratio, tip_length = float(length), float(thickness_ratio), float(tip_length)
    if not all(np.isfinite(v) for v in (length, thickness_ratio, tip_length)):
        raise ValueError('length, thickness_ratio and tip_length must be finite')
    if int(min_thickness) != min_thickness or not lowest <= int(min_thickness) <= 255:
        raise ValueError(f'min_thickness must be an integer in {lowest} .. 255, got {min_thickness!r}')
    return length, int(min_thickness), thickness_ratio, tip_length


def arrow_segments(boxes, gaze, **params):
    """The arrow plan on the host (include/mcgaze_hip.h, "annotated frames out"; arrow_plan_kernel line for line): boxes [n,4] x1 y1 x2 y2, gaze
    [n,>=2], both read as f32 and widened to double; params: length, min_thickness, thickness_ratio, tip_length (the demo's by default).
    -> (seg int64 [n,3,2,2]: shaft, stroke, stroke x (from, to) x (x, y); thickness int64 [n]; flags int32 [n]).  seg[:, 0] is
    harness.head_arrows of the same input.  Flag 2 (and a zero row): a box or gaze that is not finite, an end point outside [-8191, 8191] or a
    thickness above 255."""
    length, min_thickness, ratio, tip_length = _arrow_params(**params)
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    g = np.asarray(gaze, dtype=np.float32).astype(np.float64)
    g = g.reshape(len(b), -1)[:, :2] if g.size else np.zeros((len(b), 2 if not len(b) else 0))
    if g.shape[1] != 2:
        raise ValueError(f'gaze must be [n, >= 2], got {np.shape(gaze)}')
    ok = np.isfinite(b).all(axis=1) & np.isfinite(g).all(axis=1)
    b, g = np.where(ok[:, None], b, 0.0), np.where(ok[:, None], g, 0.0)
    inside = lambda *vs: np.logical_and.reduce([np.abs(v) <= ARROW_COORD for v in vs])
    # numpy rounds every elementwise product and sum on its own: nothing is contracted, as in the kernel
    cx, cy = np.floor(np.trunc(b[:, 0] + b[:, 2]) / 2.0), np.floor(np.trunc(b[:, 1] + b[:, 3]) / 2.0)
    l = np.trunc(np.maximum(b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]) * length)
    tx, ty = np.trunc(cx - l * g[:, 0]), np.trunc(cy - l * g[:, 1])
    t = np.maximum(float(min_thickness), np.trunc(l * ratio))
    ok &= inside(cx, cy, tx, ty) & (t <= 255.0)
    cx, cy, tx, ty, t = (np.where(ok, v, 0.0) for v in (cx, cy, tx, ty, t))
    dx, dy = cx - tx, cy - ty
    k = tip_length * 0.7071067811865476
    ax, ay = np.rint(tx + k * (dx - dy)), np.rint(ty + k * (dx + dy))          # np.rint rounds half to even
    bx, by = np.rint(tx + k * (dx + dy)), np.rint(ty + k * (dy - dx))
    ok &= inside(ax, ay, bx, by)
    tip = np.stack([tx, ty], axis=1)
    seg = np.stack([np.stack([np.stack([px, py], axis=1), tip], axis=1) for px, py in ((cx, cy), (ax, ay), (bx, by))], axis=1)
    seg, t = np.where(ok[:, None, None, None], seg, 0.0), np.where(ok, t, 0.0)
    return seg.astype(np.int64), t.astype(np.int64), np.where(ok, 0, 2).astype(np.int32)


def segment_coverage(h, w, a, b, t, y0=0, x0=0):
    """bool [h,w]: which pixels (integer centres (x0 + column, y0 + row)) belong to the segment a -> b (x, y each) of thickness t, i.e. lie
    within t / 2 of it -- a capsule, a disc for a segment of no length -- exactly, in 64-bit integers (the kernel's test, include/mcgaze_hip.h)."""
    py, px = np.mgrid[y0:y0 + h, x0:x0 + w].astype(np.int64)
    ax, ay, bx, by, tt = int(a[0]), int(a[1]), int(b[0]), int(b[1]), int(t) * int(t)
    dx, dy, qx, qy = bx - ax, by - ay, px - ax, py - ay
    L, u = dx * dx + dy * dy, qx * dx + qy * dy
    qq, rr = qx * qx + qy * qy, (px - bx) ** 2 + (py - by) ** 2
    return np.where(u <= 0, 4 * qq <= tt, np.where(u >= L, 4 * rr <= tt, 4 * (qq * L - u * u) <= tt * L))


def _arrow_colors(color, n, nv12, matrix):
    """-> (one uint8 [3] or None, per-row uint8 [n,3] or None), as the entries take them: B, G, R, or with nv12 the (Y, U, V) of bgr_to_yuv."""
    c = np.asarray(ARROW_COLOR if color is None else _host_array(color))
    if c.dtype.kind not in 'iu' or c.shape not in ((3,), (n, 3)) or (c.size and (c.min() < 0 or c.max() > 255)):
        raise ValueError(f'color must be one (B, G, R) triple or one per row, [{n}, 3], integers in [0, 255]; got {c.dtype} {c.shape}')
    c = c.astype(np.uint8)
    if nv12:
        if c.ndim == 1:
            c = bgr_to_yuv(c, matrix)
        else:
            uniq, inverse = np.unique(c, axis=0, return_inverse=True)
            c = np.stack([bgr_to_yuv(v, matrix) for v in uniq]).reshape(-1, 3)[inverse.reshape(-1)] if n else c
    return (c, None) if c.ndim == 1 else (None, np.ascontiguousarray(c))


def _arrow_rows(boxes, gaze, image_of, sizes, strict, **params):
    """Plan and flags of n rows on the host -> (seg, thickness, flags): arrow_segments plus what depends on the frames -- an image_of outside
    ``sizes`` ([(h, w), ...]) and an image larger than 8192 a side are flag 2.  strict: ValueError instead, naming the first such row."""
    seg, t, flags = arrow_segments(boxes, gaze, **params)
    image_of = np.asarray(image_of).reshape(-1)
    if image_of.dtype.kind not in 'iu':
        raise TypeError(f'image_of must hold integers, got {image_of.dtype}')
    if len(image_of) != len(flags):
        raise ValueError(f'boxes {np.shape(boxes)}, gaze {np.shape(gaze)} and image_of {image_of.shape} must be [n,4], [n,>=2] and [n]')
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    known = (image_of >= 0) & (image_of < len(hw))
    bad = ~known
    bad[known] = (hw[image_of[known]] > ARROW_SIDE).any(axis=1) | (hw[image_of[known]] <= 0).any(axis=1)
    flags = np.where(bad, 2, flags).astype(np.int32)
    if strict and flags.any():
        k = int(np.flatnonzero(flags)[0])
        raise ValueError(f'arrow {k} cannot be drawn: box {np.asarray(boxes).reshape(-1, 4)[k].tolist()}, gaze {np.asarray(gaze).reshape(len(flags), -1)[k, :2].tolist()}, '
                         f'image_of {int(image_of[k])} of {len(hw)} -- not finite, outside the image table, or an end point beyond +-{ARROW_COORD} '
                         f'/ a thickness beyond 255')
    seg[flags != 0], t[flags != 0] = 0, 0
    return seg, t, flags


def draw_arrows_host(frames, boxes, gaze, image_of=None, color=None, pixel_format='bgr', matrix='bt601', strict=False, **params):
    """The demo's arrows (MCGaze_demo/demo.ipynb, cell 5) drawn with numpy: what DevicePipeline.draw_arrows writes on the device, bit for bit
    (include/mcgaze_hip.h, "annotated frames out": the plan, the capsule coverage in 64-bit integers, the highest row winning an overlap, the
    NV12 chroma rule).  For checks and for users without a GPU.

    frames: one HxWx3 uint8 frame or a list of them; pixel_format='nv12': one surface -- a (y, uv) tuple or a [3H/2, W] array -- or a list of
    those.  boxes [n,4], gaze [n,>=2], image_of [n] (None: every row draws into frame 0), color: one (B, G, R) triple (None: the demo's
    (230, 253, 11)) or one per row; params: length, min_thickness, thickness_ratio, tip_length.
    -> (annotated COPIES in the form given -- NV12 frames as (y [H,W], uv [H/2,W]) pairs --, flags int32 [n]).  A row flagged 2 changes no
    byte; strict=True raises ValueError for it instead (what draw_arrows does for host tables)."""
    nv12, _ = _pixel_format(pixel_format, matrix)
    single = not isinstance(frames, list)
    frames = [frames] if single else frames
    if nv12:
        out = [tuple(np.array(p) for p in _nv12_planes(k, f)[:2]) for k, f in enumerate(frames)]
        sizes = [y.shape for y, _ in out]
    else:
        out = [_bgr_frame(k, np.array(f)) for k, f in enumerate(frames)]
        sizes = [a.shape[:2] for a in out]
    n = len(np.asarray(_host_array(boxes)).reshape(-1, 4))
    image_of = np.zeros(n, dtype=np.int32) if image_of is None else _host_array(image_of)
    seg, t, flags = _arrow_rows(_host_array(boxes), _host_array(gaze), image_of, sizes, strict, **params)
    one, per_row = _arrow_colors(color, n, nv12, matrix)
    for k in np.flatnonzero(flags == 0):                         # ascending: a later row overwrites an earlier one
        h, w = sizes[int(image_of[k])]
        r = (int(t[k]) + 1) // 2
        x0, y0 = max(int(seg[k, :, :, 0].min()) - r, 0), max(int(seg[k, :, :, 1].min()) - r, 0)
        x1, y1 = min(int(seg[k, :, :, 0].max()) + r + 1, w), min(int(seg[k, :, :, 1].max()) + r + 1, h)
        if x1 <= x0 or y1 <= y0:
            continue
        mask = np.zeros((h, w), dtype=bool)
        mask[y0:y1, x0:x1] = np.logical_or.reduce([segment_coverage(y1 - y0, x1 - x0, s[0], s[1], t[k], y0, x0) for s in seg[k]])
        c = one if per_row is None else per_row[k]
        if nv12:
            y, uv = out[int(image_of[k])]
            y[mask] = c[0]
            uv.reshape(h // 2, w // 2, 2)[mask.reshape(h // 2, 2, w // 2, 2).any(axis=(1, 3))] = c[1:]
        else:
            out[int(image_of[k])][mask] = c
    return (out[0] if single else out), flags


# ---------------------------------------------------------------- attention overlay (include/mcgaze_hip.h, "attention overlay")
def _overlay_thickness(who, **values):
    """line_thickness / region_thickness, validated (ValueError) -> ints in 0 .. 255; 0 switches the layer off."""
    for name, v in values.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 255:
            raise ValueError(f'{who}: {name} must be an integer in 0 .. 255 (0: the layer is off), got {v!r}')
    return [int(v) for v in values.values()]


def _overlay_palette(who, palette, nv12, matrix):
    """-> uint8 [7,3] as the entries take it: B, G, R, or with nv12 each entry converted once by bgr_to_yuv.  None: OVERLAY_PALETTE."""
    c = np.asarray(OVERLAY_PALETTE if palette is None else _host_array(palette))
    if c.dtype.kind not in 'iu' or c.shape != (7, 3) or c.min() < 0 or c.max() > 255:
        raise ValueError(f'{who}: palette must be [7, 3] (B, G, R) integers in [0, 255] -- none, head, region, camera, mutual, outline, outline '
                         f'looked at; got {c.dtype} {c.shape}')
    c = c.astype(np.uint8)
    return np.ascontiguousarray(np.stack([bgr_to_yuv(v, matrix) for v in c]).reshape(7, 3).astype(np.uint8) if nv12 else c)


def _overlay_options(who, overlay, draw, attention):
    """The ``overlay=`` option of LiveGaze and of run_head_video's draw dict, validated (ValueError) -> None (off) or the dict of
    draw_attention's palette, line_thickness and region_thickness that were given.  It needs both ``draw`` and ``attention``."""
    if overlay is None or overlay is False:
        return None
    if overlay is not True and not isinstance(overlay, dict):
        raise ValueError(f'{who}: overlay is None, True or a dict of palette, line_thickness and region_thickness; got {overlay!r}')
    opts = {} if overlay is True else dict(overlay)
    if set(opts) - {'palette', 'line_thickness', 'region_thickness'}:
        raise ValueError(f'{who}: overlay takes palette, line_thickness and region_thickness; got {sorted(opts)}')
    if not draw or attention is None:
        raise ValueError(f'{who}: overlay draws what attention found into the frames draw hands out: it needs both draw and attention')
    _overlay_thickness(who, **{k: v for k, v in opts.items() if k != 'palette'})
    _overlay_palette(who, opts.get('palette'), False, 'bt601')
    return opts


def _overlay_regions(who, regions, region_image):
    """The three forms gaze_targets_host takes -- [m,4] rectangles, the mixed list of region_polygons, a PolyRegions -- as HOST vertex tables
    -> (xy f32 [V,2], start int32 [m+1], region_image int32 [m]), checked as there."""
    if A._holds_polygon(regions):
        regions = A.region_polygons(regions)
    if isinstance(regions, A.PolyRegions):
        return A._poly_tables(who, regions, region_image)
    r32, ri = A._region_tables(who, regions, region_image)
    xy, start = A._as_vertices(r32)
    return np.ascontiguousarray(xy), start, ri


def _overlay_counts(who, n, m, vertices, images):
    if n > 65535:
        raise ValueError(f'{who}: at most 65535 rows per call (got {n})')
    A._check_counts(who, 0, m, vertices)
    if images * m > OVERLAY_ACTIVE:
        raise ValueError(f'{who}: frames x regions must not exceed {OVERLAY_ACTIVE} (got {images} x {m})')


def _overlay_targets(who, n, kind, target, hit, mutual):
    """Host kind / target / mutual [n] integers and hit [n,2] -> (int32, int32, f32 [n,2], int32), checked (TypeError / ValueError)."""
    out = []
    for name, t in (('kind', kind), ('target', target), ('mutual', mutual)):
        a = np.asarray(_host_array(t)).reshape(-1)
        if a.size and a.dtype.kind not in 'iub':
            raise TypeError(f'{who}: {name} must hold integers, got {a.dtype}')
        if a.shape != (n,):
            raise ValueError(f'{who}: {name} must be [{n}], one per row; got {a.shape}')
        out.append(np.ascontiguousarray(a, dtype=np.int32))
    h = np.asarray(_host_array(hit))
    h = h.reshape(0, 2) if h.size == 0 else h
    if h.shape != (n, 2) or h.dtype.kind not in 'fiu':
        raise ValueError(f'{who}: hit must be [{n}, 2] numbers, got {h.dtype} {h.shape}')
    return out[0], out[1], np.ascontiguousarray(h, dtype=np.float32), out[2]


def region_outlines(xy, start):
    """The outlines of the vertex tables (xy f32 [V,2], start [m+1]) as "attention overlay" draws them -> (corners: a list of m int64 [c,2]
    arrays, None for an unusable region; region_flags int32 [m]).  Usable: the rule of gaze_targets' regions, and every coordinate rounded
    (half to even, in double) within +-8191.  A rectangle's corners are (x1, y1) (x2, y1) (x2, y2) (x1, y2)."""
    xy64 = np.asarray(xy, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    ok, first, count = A._usable_regions(xy64, np.asarray(start))
    corners = []
    for j in range(len(ok)):
        v = np.rint(xy64[first[j]:first[j] + count[j]]) if ok[j] else None
        if v is not None and (np.abs(v) <= ARROW_COORD).all():
            v = v.astype(np.int64)
            corners.append(np.array([v[0], (v[1, 0], v[0, 1]), v[1], (v[0, 0], v[1, 1])]) if len(v) == 2 else v)
        else:
            corners.append(None)
    return corners, np.array([0 if c is not None else 2 for c in corners], dtype=np.int32)


def draw_attention_host(frames, boxes, gaze, image_of, kind, target, hit, mutual, regions=None, region_image=None, region_period=0, palette=None,
                        line_thickness=2, region_thickness=2, pixel_format='bgr', matrix='bt601', strict=False, **params):
    """The attention overlay drawn with numpy: what DevicePipeline.draw_attention (mcg_draw_attention / mcg_draw_attention_nv12) writes on the
    device, bit for bit (include/mcgaze_hip.h, "attention overlay").  Three layers, low to high, the higher index winning inside a layer: the
    outlines of the regions (palette[6] in a picture where a row looks at the region, else palette[5]), a sight line from every head that
    looks at a head or a region to its hit point, and draw_arrows_host's arrows in palette[4 if mutual else kind] (a kind outside 1 .. 3: 0).

    frames, boxes, gaze, image_of, pixel_format, matrix, strict and params (length, min_thickness, thickness_ratio, tip_length): as for
    draw_arrows_host; kind, target, mutual [n] integers and hit [n,2] as gaze_targets_host returns them; regions, region_image,
    region_period as gaze_targets_host takes them ([m,4] rectangles, the mixed list of region_polygons, or a PolyRegions).  palette: [7,3]
    B, G, R (None: OVERLAY_PALETTE, a convention); for NV12 each entry is converted once by bgr_to_yuv.  A thickness of 0 (line_thickness,
    region_thickness, min_thickness) switches its layer off.
    -> (annotated COPIES in the form given, flags int32 [n], region_flags int32 [m], region_active int32 [frames, m]).  A region that cannot be
    used (region_flags 2) and a row flagged 2 change no byte; a hit that is not finite or beyond +-8191 drops the sight line only."""
    who = 'draw_attention_host'
    nv12, _ = _pixel_format(pixel_format, matrix)
    line_thickness, region_thickness = _overlay_thickness(who, line_thickness=line_thickness, region_thickness=region_thickness)
    _, _, period = A._target_params(region_period=region_period, who=who)
    pal = _overlay_palette(who, palette, nv12, matrix)
    single = not isinstance(frames, list)
    frames = [frames] if single else frames
    if nv12:
        out = [tuple(np.array(p) for p in _nv12_planes(k, f)[:2]) for k, f in enumerate(frames)]
        sizes = [y.shape for y, _ in out]
    else:
        out = [_bgr_frame(k, np.array(f)) for k, f in enumerate(frames)]
        sizes = [a.shape[:2] for a in out]
    n = len(np.asarray(_host_array(boxes)).reshape(-1, 4))
    image_of = np.zeros(n, dtype=np.int32) if image_of is None or not np.size(_host_array(image_of)) else np.asarray(_host_array(image_of)).reshape(-1)
    kind, target, hit, mutual = _overlay_targets(who, n, kind, target, hit, mutual)
    xy, start, ri = _overlay_regions(who, regions, region_image)
    m = len(ri)
    _overlay_counts(who, n, m, len(xy), len(frames))
    seg, t, flags = _arrow_rows(_host_array(boxes), _host_array(gaze), image_of, sizes, strict, lowest=0, **params)
    min_thickness = _arrow_params(lowest=0, **params)[1]
    corners, region_flags = region_outlines(xy, start)
    region_active = np.zeros((len(frames), m), dtype=np.int32)
    looks = (kind == 2) & (target >= 0) & (target < m) & (image_of >= 0) & (image_of < len(frames))
    region_active[image_of[looks], target[looks]] = 1
    row_color = np.where(mutual != 0, 4, np.where((kind >= 1) & (kind <= 3), kind, 0))
    with np.errstate(invalid='ignore'):
        h64 = np.rint(hit.astype(np.float64))
        line_ok = (flags == 0) & ((kind == 1) | (kind == 2)) & (np.abs(h64) <= ARROW_COORD).all(axis=1)     # (a NaN fails the comparison)
    for p, (h, w) in enumerate(sizes):
        if h > ARROW_SIDE or w > ARROW_SIDE or h <= 0 or w <= 0:
            continue
        winner = np.full((h, w), -1, dtype=np.int64)              # the highest stroke that covers each pixel
        color = np.zeros((m + 2 * n, 3), dtype=np.uint8)

        def stroke(index, segments, thickness, c):
            pts = np.asarray([q for s in segments for q in s])
            r = (thickness + 1) // 2
            x0, y0 = max(int(pts[:, 0].min()) - r, 0), max(int(pts[:, 1].min()) - r, 0)
            x1, y1 = min(int(pts[:, 0].max()) + r + 1, w), min(int(pts[:, 1].max()) + r + 1, h)
            color[index] = c
            if x1 <= x0 or y1 <= y0:
                return
            cover = np.logical_or.reduce([segment_coverage(y1 - y0, x1 - x0, a, b, thickness, y0, x0) for a, b in segments])
            winner[y0:y1, x0:x1][cover] = index                   # ascending: a later stroke overwrites an earlier one

        for j in range(m if region_thickness else 0):
            if corners[j] is not None and (ri[j] < 0 or ri[j] == p or (period > 0 and ri[j] == p % period)):
                v = corners[j]
                stroke(j, [(v[k], v[(k + 1) % len(v)]) for k in range(len(v))], region_thickness, pal[6 if region_active[p, j] else 5])
        rows = np.flatnonzero((flags == 0) & (image_of == p))
        for k in rows[line_ok[rows]] if line_thickness else ():
            stroke(m + k, [(seg[k, 0, 0], h64[k].astype(np.int64))], line_thickness, pal[row_color[k]])
        for k in rows if min_thickness else ():
            stroke(m + n + k, list(seg[k]), int(t[k]), pal[row_color[k]])
        if nv12:
            y, uv = out[p]
            y[winner >= 0] = color[winner[winner >= 0], 0]
            top = winner.reshape(h // 2, 2, w // 2, 2).max(axis=(1, 3))   # the highest stroke among the four luma pixels of a chroma pair
            uv.reshape(h // 2, w // 2, 2)[top >= 0] = color[top[top >= 0], 1:]
        else:
            out[p][winner >= 0] = color[winner[winner >= 0]]
    return (out[0] if single else out), flags, region_flags, region_active


# ---------------------------------------------------------------- text labels (include/mcgaze_hip.h, "text labels")
LABEL_CHARS = 24                                                 # MCG_LABEL_CHARS
# The glyphs of LABEL_FONT, drawn by hand for this project: codes 32 .. 126 in order, seven rows of five columns each, '#' set.  The eighth
# row and the columns 5 .. 7 of the 8 x 8 cell stay empty (the gap between lines and characters).
_GLYPHS = (
    '...../...../...../...../...../...../.....',   # space
    '..#../..#../..#../..#../..#../...../..#..',   # !
    '.#.#./.#.#./.#.#./...../...../...../.....',   # "
    '.#.#./.#.#./#####/.#.#./#####/.#.#./.#.#.',   # #
    '..#../.####/#.#../.###./..#.#/####./..#..',   # $
    '##..#/##..#/...#./..#../.#.../#..##/#..##',   # %
    '.##../#..#./#.#../.#.../#.#.#/#..#./.##.#',   # &
    '..#../..#../..#../...../...../...../.....',   # '
    '...#./..#../.#.../.#.../.#.../..#../...#.',   # (
    '.#.../..#../...#./...#./...#./..#../.#...',   # )
    '...../..#../#.#.#/.###./#.#.#/..#../.....',   # *
    '...../..#../..#../#####/..#../..#../.....',   # +
    '...../...../...../...../.##../..#../.#...',   # ,
    '...../...../...../#####/...../...../.....',   # -
    '...../...../...../...../...../.##../.##..',   # .
    '....#/....#/...#./..#../.#.../#..../#....',   # /
    '.###./#...#/#..##/#.#.#/##..#/#...#/.###.',   # 0
    '..#../.##../..#../..#../..#../..#../.###.',   # 1
    '.###./#...#/....#/...#./..#../.#.../#####',   # 2
    '#####/...#./..#../...#./....#/#...#/.###.',   # 3
    '...#./..##./.#.#./#..#./#####/...#./...#.',   # 4
    '#####/#..../####./....#/....#/#...#/.###.',   # 5
    '..##./.#.../#..../####./#...#/#...#/.###.',   # 6
    '#####/....#/...#./..#../.#.../.#.../.#...',   # 7
    '.###./#...#/#...#/.###./#...#/#...#/.###.',   # 8
    '.###./#...#/#...#/.####/....#/...#./.##..',   # 9
    '...../.##../.##../...../.##../.##../.....',   # :
    '...../.##../.##../...../.##../..#../.#...',   # ;
    '...#./..#../.#.../#..../.#.../..#../...#.',   # <
    '...../...../#####/...../#####/...../.....',   # =
    '.#.../..#../...#./....#/...#./..#../.#...',   # >
    '.###./#...#/....#/...#./..#../...../..#..',   # ?
    '.###./#...#/#.###/#.#.#/#.###/#..../.####',   # @
    '.###./#...#/#...#/#####/#...#/#...#/#...#',   # A
    '####./#...#/#...#/####./#...#/#...#/####.',   # B
    '.###./#...#/#..../#..../#..../#...#/.###.',   # C
    '###../#..#./#...#/#...#/#...#/#..#./###..',   # D
    '#####/#..../#..../####./#..../#..../#####',   # E
    '#####/#..../#..../####./#..../#..../#....',   # F
    '.###./#...#/#..../#.###/#...#/#...#/.####',   # G
    '#...#/#...#/#...#/#####/#...#/#...#/#...#',   # H
    '.###./..#../..#../..#../..#../..#../.###.',   # I
    '..###/...#./...#./...#./...#./#..#./.##..',   # J
    '#...#/#..#./#.#../##.../#.#../#..#./#...#',   # K
    '#..../#..../#..../#..../#..../#..../#####',   # L
    '#...#/##.##/#.#.#/#.#.#/#...#/#...#/#...#',   # M
    '#...#/##..#/#.#.#/#..##/#...#/#...#/#...#',   # N
    '.###./#...#/#...#/#...#/#...#/#...#/.###.',   # O
    '####./#...#/#...#/####./#..../#..../#....',   # P
    '.###./#...#/#...#/#...#/#.#.#/#..#./.##.#',   # Q
    '####./#...#/#...#/####./#.#../#..#./#...#',   # R
    '.####/#..../#..../.###./....#/....#/####.',   # S
    '#####/..#../..#../..#../..#../..#../..#..',   # T
    '#...#/#...#/#...#/#...#/#...#/#...#/.###.',   # U
    '#...#/#...#/#...#/#...#/#...#/.#.#./..#..',   # V
    '#...#/#...#/#...#/#.#.#/#.#.#/##.##/#...#',   # W
    '#...#/#...#/.#.#./..#../.#.#./#...#/#...#',   # X
    '#...#/#...#/.#.#./..#../..#../..#../..#..',   # Y
    '#####/....#/...#./..#../.#.../#..../#####',   # Z
    '.###./.#.../.#.../.#.../.#.../.#.../.###.',   # [
    '#..../#..../.#.../..#../...#./....#/....#',   # backslash
    '.###./...#./...#./...#./...#./...#./.###.',   # ]
    '..#../.#.#./#...#/...../...../...../.....',   # ^
    '...../...../...../...../...../...../#####',   # _
    '.#.../..#../...#./...../...../...../.....',   # `
    '...../...../.###./....#/.####/#...#/.####',   # a
    '#..../#..../#.##./##..#/#...#/#...#/####.',   # b
    '...../...../.###./#..../#..../#...#/.###.',   # c
    '....#/....#/.##.#/#..##/#...#/#...#/.####',   # d
    '...../...../.###./#...#/#####/#..../.###.',   # e
    '..##./.#..#/.#.../###../.#.../.#.../.#...',   # f
    '...../.####/#...#/#...#/.####/....#/.###.',   # g
    '#..../#..../#.##./##..#/#...#/#...#/#...#',   # h
    '..#../...../.##../..#../..#../..#../.###.',   # i
    '...#./...../..##./...#./...#./#..#./.##..',   # j
    '#..../#..../#..#./#.#../##.../#.#../#..#.',   # k
    '.##../..#../..#../..#../..#../..#../.###.',   # l
    '...../...../##.#./#.#.#/#.#.#/#...#/#...#',   # m
    '...../...../#.##./##..#/#...#/#...#/#...#',   # n
    '...../...../.###./#...#/#...#/#...#/.###.',   # o
    '...../####./#...#/#...#/####./#..../#....',   # p
    '...../.####/#...#/#...#/.####/....#/....#',   # q
    '...../...../#.##./##..#/#..../#..../#....',   # r
    '...../...../.####/#..../.###./....#/####.',   # s
    '.#.../.#.../###../.#.../.#.../.#..#/..##.',   # t
    '...../...../#...#/#...#/#...#/#..##/.##.#',   # u
    '...../...../#...#/#...#/#...#/.#.#./..#..',   # v
    '...../...../#...#/#...#/#.#.#/#.#.#/.#.#.',   # w
    '...../...../#...#/.#.#./..#../.#.#./#...#',   # x
    '...../#...#/#...#/#...#/.####/....#/.###.',   # y
    '...../...../#####/...#./..#../.#.../#####',   # z
    '...#./..#../..#../.#.../..#../..#../...#.',   # {
    '..#../..#../..#../..#../..#../..#../..#..',   # |
    '.#.../..#../..#../...#./..#../..#../.#...',   # }
    '...../...../.#.../#.#.#/...#./...../.....',   # ~
)


def _label_font():
    font = np.zeros((96, 8), dtype=np.uint8)                     # entry 95 is spare: the codes end at 126
    for g, rows in enumerate(_GLYPHS):
        for r, bits in enumerate(rows.split('/')):
            font[g, r] = sum(1 << c for c, b in enumerate(bits) if b == '#')
    return font


LABEL_FONT = _label_font()                                       # uint8 [96][8]: one byte per glyph row, bit c (from the least significant) is column c from the left
LABEL_FONT.setflags(write=False)


def glyph_sheet(font=LABEL_FONT, per_line=16):
    """The font as text art, ``per_line`` glyphs side by side: what INTEGRATION.md shows."""
    lines = []
    for first in range(0, 95, per_line):
        lines += [' '.join(''.join('#' if font[g, r] >> c & 1 else '.' for c in range(5)) for g in range(first, min(first + per_line, 95))) for r in range(7)]
        lines.append('')
    return '\n'.join(lines[:-1])


def encode_labels(strings):
    """Strings -> the text table uint8 [n][24] of the label entries: Latin-1 codes, zero behind the end.  ValueError for a string longer than
    24 characters or with a character outside Latin-1.  (A code outside 32 .. 126 is drawn as '?'.)"""
    out = np.zeros((len(strings), LABEL_CHARS), dtype=np.uint8)
    for k, s in enumerate(strings):
        try:
            codes = str(s).encode('latin-1')
        except UnicodeEncodeError:
            raise ValueError(f'label {k} {s!r} holds a character outside Latin-1') from None
        if len(codes) > LABEL_CHARS:
            raise ValueError(f'label {k} {s!r} is longer than {LABEL_CHARS} characters')
        out[k, :len(codes)] = np.frombuffer(codes, dtype=np.uint8)
    return out


def _label_rate(rate):
    """rate = (num, den) frames per second, validated (ValueError) -> (num, den): integers with 1 <= den <= num <= 2^20."""
    try:
        num, den = rate
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (num, den)) and 1 <= den <= num <= 1 << 20
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'rate must be (num, den), integers with 1 <= den <= num <= 2^20 frames per second; got {rate!r}')
    return int(num), int(den)


def _label_params(scale=2, advance=6, pad=1):
    """scale, advance and pad of the label entries, validated (ValueError) -> ints."""
    for name, v, lo, hi in (('scale', scale, 1, 16), ('advance', advance, 1, 8), ('pad', pad, 0, 8)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f'{name} must be an integer in {lo} .. {hi}, got {v!r}')
    return int(scale), int(advance), int(pad)


def _label_options(who, labels, draw):
    """The ``labels=`` option of LiveGaze and of run_head_video's draw dict, validated (ValueError) -> None (off) or dict(scale, advance, pad,
    background, fps, region_names), the defaults filled in.  It needs ``draw``."""
    if labels is None or labels is False:
        return None
    if labels is not True and not isinstance(labels, dict):
        raise ValueError(f'{who}: labels is None, True or a dict of scale, advance, pad, background, fps and region_names; got {labels!r}')
    opts = dict(scale=2, advance=6, pad=1, background=(0, 0, 0), fps=(30, 1), region_names=None)
    given = {} if labels is True else dict(labels)
    if set(given) - set(opts):
        raise ValueError(f'{who}: labels takes {sorted(opts)}; got {sorted(given)}')
    if not draw:
        raise ValueError(f'{who}: labels writes into the frames draw hands out: it needs draw')
    opts.update(given)
    opts['scale'], opts['advance'], opts['pad'] = _label_params(opts['scale'], opts['advance'], opts['pad'])
    opts['fps'] = _label_rate(opts['fps'])
    _label_background(opts['background'], False, 'bt601')
    return opts


def _label_ints(name, t, n=None):
    a = np.asarray(_host_array(t)).reshape(-1)
    if a.size and a.dtype.kind not in 'iu':
        raise TypeError(f'{name} must hold integers, got {a.dtype}')
    if n is not None and a.shape != (n,):
        raise ValueError(f'{name} must be [{n}], one per row; got {a.shape}')
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError(f'{name} must fit int32')
    return np.ascontiguousarray(a, dtype=np.int32)


def format_labels_host(ids, values=None, rate=(30, 1)):
    """mcg_format_labels on the host, bit for bit (include/mcgaze_hip.h, "text labels") -> uint8 [n][24].  ids [n] int32: id <= 0 gives an
    empty row, else '#' + decimal(id); with values [n] int32 (frames) and a value > 0, ' ' + seconds in tenths + 's' at rate = (num, den)
    frames per second, floored.  A text of 25 characters -- ten digits on both sides -- loses its 's'."""
    num, den = _label_rate(rate)
    ids = _label_ints('ids', ids)
    values = None if values is None else _label_ints('values', values, len(ids))
    out = np.zeros((len(ids), LABEL_CHARS), dtype=np.uint8)
    for k, v in enumerate(ids.tolist()):
        if v <= 0:
            continue
        s = '#' + str(v)
        f = 0 if values is None else int(values[k])
        if f > 0:
            q = f * 10 * den // num
            s += f' {q // 10}.{q % 10}s'
        codes = s.encode('ascii')[:LABEL_CHARS]
        out[k, :len(codes)] = np.frombuffer(codes, dtype=np.uint8)
    return out


def _label_text(text, n):
    t = np.asarray(_host_array(text))
    t = t.reshape(0, LABEL_CHARS) if t.size == 0 else t
    if t.dtype != np.uint8 or t.shape != (n, LABEL_CHARS):
        raise ValueError(f'text must be uint8 [{n}, {LABEL_CHARS}] (encode_labels, format_labels), got {t.dtype} {t.shape}')
    return np.ascontiguousarray(t)


def _label_font_table(font):
    f = np.asarray(LABEL_FONT if font is None else _host_array(font))
    if f.dtype != np.uint8 or f.shape != (96, 8):
        raise ValueError(f'font must be uint8 [96, 8], got {f.dtype} {f.shape}')
    return np.ascontiguousarray(f)


def _label_background(background, nv12, matrix):
    """-> uint8 [3] as the entries take it (NV12: converted once by bgr_to_yuv), or None: no plates."""
    if background is None:
        return None
    c = np.asarray(_host_array(background))
    if c.dtype.kind not in 'iu' or c.shape != (3,) or c.min() < 0 or c.max() > 255:
        raise ValueError(f'background must be one (B, G, R) triple of integers in [0, 255] or None, got {background!r}')
    c = c.astype(np.uint8)
    return np.asarray(bgr_to_yuv(c, matrix), dtype=np.uint8).reshape(3) if nv12 else c


def label_plan(boxes, image_of, text, sizes, place=None, scale=2, advance=6, pad=1, nv12=False):
    """The label plan on the host (include/mcgaze_hip.h, "text labels"; label_plan_kernel line for line): boxes [n,4] read as f32, image_of
    [n], text uint8 [n,24], place [n] or None, sizes [(h, w), ...] of the frames -> a dict of int64 [n] arrays x, y (the text origin), x0,
    y0, x1, y1 (the plate clipped to the frame), image, flag, len.  Flag 2: image_of outside the table, an image without pixels, larger than
    8192 a side or (nv12) of odd size, a box that is not finite or beyond +-8191 once truncated; flag 1: an empty text.  A flagged row is
    zero but for image = -1."""
    scale, advance, pad = _label_params(scale, advance, pad)
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    n = len(b)
    image_of = _label_ints('image_of', image_of, n).astype(np.int64)
    text = _label_text(text, n)
    place = np.zeros(n, dtype=np.int64) if place is None else _label_ints('place', place, n).astype(np.int64)
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    ok = (image_of >= 0) & (image_of < len(hw)) & np.isfinite(b).all(axis=1)
    h, w = (np.where(ok, hw[np.where(ok, image_of, 0), c] if len(hw) else 0, 0) for c in (0, 1))
    ok &= (h > 0) & (w > 0) & (h <= ARROW_SIDE) & (w <= ARROW_SIDE)
    if nv12:
        ok &= ((h | w) & 1) == 0
    bt = np.trunc(np.where(np.isfinite(b), b, 0.0))
    ok &= (np.abs(bt) <= ARROW_COORD).all(axis=1)
    bt = np.where(ok[:, None], bt, 0.0).astype(np.int64)
    zero = text == 0
    length = np.where(zero.any(axis=1), zero.argmax(axis=1), LABEL_CHARS).astype(np.int64)
    flag = np.where(~ok, 2, np.where(length == 0, 1, 0))
    live = flag == 0
    P = pad * scale
    PW, PH = length * advance * scale + 2 * P, 8 * scale + 2 * P
    X, Y = bt[:, 0], np.where(place == 1, bt[:, 1], np.where(bt[:, 1] - PH < 0, bt[:, 3] + 1, bt[:, 1] - PH))
    X, Y = np.maximum(0, np.minimum(X, w - PW)), np.maximum(0, np.minimum(Y, h - PH))
    plan = dict(x=X + P, y=Y + P, x0=X, y0=Y, x1=np.minimum(X + PW, w), y1=np.minimum(Y + PH, h), image=image_of, len=length)
    plan = {k: np.where(live, v, -1 if k == 'image' else 0).astype(np.int64) for k, v in plan.items()}
    plan['flag'] = flag.astype(np.int64)
    return plan


def label_coverage(plan, k, text, font=None, scale=2, advance=6):
    """(plate's y0, x0, bool [y1 - y0, x1 - x0]): which pixels of the clipped plate of row k are glyph pixels -- COVERAGE of "text labels"."""
    font = _label_font_table(font)
    x0, y0, x1, y1 = (int(plan[f][k]) for f in ('x0', 'y0', 'x1', 'y1'))
    py, px = np.mgrid[y0:y1, x0:x1]
    fx, fy = px - int(plan['x'][k]), py - int(plan['y'][k])
    cell, n = advance * scale, int(plan['len'][k])
    inside = (fx >= 0) & (fx < n * cell) & (fy >= 0) & (fy < 8 * scale)
    fx, fy = np.where(inside, fx, 0), np.where(inside, fy, 0)
    codes = np.asarray(text[k], dtype=np.int64)[fx // cell]
    glyph = np.where((codes >= 32) & (codes <= 126), codes - 32, 31)
    return y0, x0, inside & ((font[glyph, fy // scale] >> ((fx % cell) // scale).astype(np.uint8)) & 1).astype(bool)


def draw_labels_host(frames, boxes, image_of, text, colors=None, color=None, background=(0, 0, 0), scale=2, advance=6, pad=1, place=None, font=None,
                     pixel_format='bgr', matrix='bt601', strict=False):
    """Text labels drawn with numpy: what DevicePipeline.draw_labels (mcg_draw_labels / mcg_draw_labels_nv12) writes on the device, bit for
    bit (include/mcgaze_hip.h, "text labels": the plan, the coverage, the plate of row k as stroke 2 k under its glyphs as stroke 2 k + 1,
    the highest stroke winning, the NV12 chroma rule).

    frames, pixel_format, matrix: as for draw_arrows_host.  boxes [n,4], image_of [n] (None: frame 0), text uint8 [n,24] (encode_labels,
    format_labels_host), place [n] or None (1: inside the box's top-left corner; else above the box, below it where there is no room).
    color: one (B, G, R) triple (None: the arrows' (230, 253, 11)); colors: one per row, [n,3], instead.  background: one triple, or None
    for no plates.  font: uint8 [96,8] (None: LABEL_FONT).
    -> (annotated COPIES in the form given, flags int32 [n]: 0 drawn, 1 an empty label, 2 unusable).  strict=True raises ValueError for a
    flag 2 row instead (what draw_labels does for host tables)."""
    nv12, _ = _pixel_format(pixel_format, matrix)
    scale, advance, pad = _label_params(scale, advance, pad)
    font = _label_font_table(font)
    single = not isinstance(frames, list)
    frames = [frames] if single else frames
    if nv12:
        out = [tuple(np.array(p) for p in _nv12_planes(k, f)[:2]) for k, f in enumerate(frames)]
        sizes = [y.shape for y, _ in out]
    else:
        out = [_bgr_frame(k, np.array(f)) for k, f in enumerate(frames)]
        sizes = [a.shape[:2] for a in out]
    n = len(np.asarray(_host_array(boxes)).reshape(-1, 4))
    image_of = np.zeros(n, dtype=np.int32) if image_of is None else _host_array(image_of)
    text = _label_text(text, n)
    plan = label_plan(_host_array(boxes), image_of, text, sizes, place, scale, advance, pad, nv12)
    flags = plan['flag'].astype(np.int32)
    if strict and (flags == 2).any():
        k = int(np.flatnonzero(flags == 2)[0])
        raise ValueError(f'label {k} cannot be drawn: box {np.asarray(_host_array(boxes)).reshape(-1, 4)[k].tolist()}, image_of {int(np.asarray(image_of).reshape(-1)[k])} of '
                         f'{len(sizes)} -- not finite, outside the image table, or a coordinate beyond +-{ARROW_COORD}')
    one, per_row = _arrow_colors(color if colors is None else colors, n, nv12, matrix)
    if colors is not None and per_row is None:
        raise ValueError(f'colors must be one (B, G, R) triple per row, [{n}, 3]')
    bg = _label_background(background, nv12, matrix)
    for p, (h, w) in enumerate(sizes):
        rows = np.flatnonzero((flags == 0) & (plan['image'] == p))
        if not len(rows):
            continue
        winner = np.full((h, w), -1, dtype=np.int64)             # the highest stroke that covers each pixel
        stroke_color = np.zeros((2 * n, 3), dtype=np.uint8)
        for k in rows:                                           # ascending: a later stroke overwrites an earlier one
            y0, x0, glyphs = label_coverage(plan, k, text, font, scale, advance)
            area = winner[y0:y0 + glyphs.shape[0], x0:x0 + glyphs.shape[1]]
            if bg is not None:
                area[:] = 2 * k
                stroke_color[2 * k] = bg
            area[glyphs] = 2 * k + 1
            stroke_color[2 * k + 1] = one if per_row is None else per_row[k]
        if nv12:
            y, uv = out[p]
            y[winner >= 0] = stroke_color[winner[winner >= 0], 0]
            top = winner.reshape(h // 2, 2, w // 2, 2).max(axis=(1, 3))   # the highest stroke among the four luma pixels of a chroma pair
            uv.reshape(h // 2, w // 2, 2)[top >= 0] = stroke_color[top[top >= 0], 1:]
        else:
            out[p][winner >= 0] = stroke_color[winner[winner >= 0]]
    return (out[0] if single else out), flags


# ---------------------------------------------------------------- gaze heat map (include/mcgaze_hip.h, "gaze heat map")
def _heat_ramp():
    """HEAT_LUT, made here by an integer formula: four stretches of 64 levels -- blue to cyan, to green, to yellow, to red -- with
    f = (level % 64) * 255 // 63 the way along a stretch, and an alpha of (level * 160 + 127) // 255: 0 at level 0, 160 at level 255."""
    lut = np.zeros((256, 4), dtype=np.uint8)
    for level in range(256):
        f = (level & 63) * 255 // 63
        lut[level, :3] = ((255, f, 0), (255 - f, 255, 0), (0, 255, f), (0, 255 - f, 255))[level >> 6]      # B, G, R
        lut[level, 3] = (level * 160 + 127) // 255
    return lut


HEAT_LUT = _heat_ramp()
HEAT_LUT.flags.writeable = False                                 # uint8 [256][4]: (B, G, R, alpha) per level; a convention, not tuned
_HEAT_LUTS = {}


def heat_lut(lut=None, nv12=False, matrix='bt601'):
    """The colour table as the entries take it -> uint8 [256, 4], contiguous.  lut: [256, 4] integers in [0, 255], (B, G, R, alpha) per
    level (None: HEAT_LUT); ValueError for anything else.  With nv12 each entry's colour is converted once by bgr_to_yuv(., matrix), as
    _overlay_palette does; the default ramp's conversion is kept per matrix and handed out READ-ONLY (as HEAT_LUT is): it is everybody's."""
    if lut is None and (nv12, matrix) in _HEAT_LUTS:
        return _HEAT_LUTS[nv12, matrix]
    c = np.asarray(HEAT_LUT if lut is None else _host_array(lut))
    if c.dtype.kind not in 'iu' or c.shape != (256, 4) or c.min() < 0 or c.max() > 255:
        raise ValueError(f'the heat colour table must be [256, 4] (B, G, R, alpha) integers in [0, 255]; got {c.dtype} {c.shape}')
    c = np.ascontiguousarray(c.astype(np.uint8))
    if nv12:
        uniq, inverse = np.unique(c[:, :3], axis=0, return_inverse=True)
        c[:, :3] = np.stack([bgr_to_yuv(v, matrix) for v in uniq]).reshape(-1, 3)[inverse.reshape(-1)]
    if lut is None:
        c.flags.writeable = False
        _HEAT_LUTS[nv12, matrix] = c
    return c


def heat_levels(grid, full, h, w, cell_shift):
    """The LEVEL of every pixel of an h x w picture over one camera's grid int32 [GH, GW] ("gaze heat map"): the interpolation between cell
    centres in 64-bit integers, edge cells repeated -> int64 [h, w] in 0 .. 255.  full: the scale; below 1 it is 1."""
    grid = np.maximum(np.asarray(grid, dtype=np.int64), 0)
    GH, GW = grid.shape
    S = 1 << cell_shift

    def axis(size, cells):
        u = 2 * np.arange(size, dtype=np.int64) + 1 - S
        i0 = u >> (cell_shift + 1)                                # arithmetic: floors
        return np.clip(i0, 0, cells - 1), np.clip(i0 + 1, 0, cells - 1), u - i0 * 2 * S

    y0, y1, fy = axis(h, GH)
    x0, x1, fx = axis(w, GW)
    fy, fx = fy[:, None], fx[None, :]
    v = (2 * S - fx) * (2 * S - fy) * grid[y0][:, x0] + fx * (2 * S - fy) * grid[y0][:, x1] + (2 * S - fx) * fy * grid[y1][:, x0] + \
        fx * fy * grid[y1][:, x1]
    return np.minimum(255, (v * 255) // (4 * S * S * max(int(full), 1)))


def _heat_blend(src, col, a):
    """(src (255 - a) + col a + 127) / 255 in integers, elementwise -> uint8."""
    return ((src.astype(np.int64) * (255 - a) + col * a + 127) // 255).astype(np.uint8)


def draw_heat_host(frames, heat, full, cell_shift, period=0, lut=None, min_level=1, pixel_format='bgr', matrix='bt601'):
    """The heat map blended into frames with numpy: what DevicePipeline.draw_heat (mcg_draw_heat / mcg_draw_heat_nv12) writes on the device,
    bit for bit (include/mcgaze_hip.h, "gaze heat map": the level of a pixel, the blend, the NV12 chroma rule).

    frames, pixel_format, matrix: as for draw_arrows_host.  heat: int32 [C, GH, GW] (gaze_heat_host); full: int [C], the scale of each
    camera -- gaze_heat_host's peak -- or one int for all; cell_shift 0 .. 6; picture p shows camera p, with a period p % period, and is
    left as it is where that camera is not below C.  lut: [256, 4] (B, G, R, alpha) per level (None: HEAT_LUT), converted once per entry for
    NV12.  A pixel whose level is below min_level (1 .. 255) keeps its bytes.
    -> annotated COPIES in the form given (NV12 frames as (y [H,W], uv [H/2,W]) pairs)."""
    who = 'draw_heat_host'
    nv12, _ = _pixel_format(pixel_format, matrix)
    cell_shift, _, _, period, _ = A._heat_params(who, cell_shift, 0, 0, period, 0)
    _, min_level = A._heat_scale(who, None, min_level)
    table = heat_lut(lut, nv12, matrix).astype(np.int64)
    heat = np.asarray(_host_array(heat))
    C, GH, GW = A._heat_grid(who, heat.shape)
    full = np.broadcast_to(np.asarray(_host_array(full), dtype=np.int64).reshape(-1), (C,)) if np.size(full) in (1, C) else None
    if full is None:
        raise ValueError(f'{who}: full is one int or one per camera, [{C}]')
    single = not isinstance(frames, list)
    frames = [frames] if single else frames
    if nv12:
        out = [tuple(np.array(p) for p in _nv12_planes(k, f)[:2]) for k, f in enumerate(frames)]
        sizes = [y.shape for y, _ in out]
    else:
        out = [_bgr_frame(k, np.array(f)) for k, f in enumerate(frames)]
        sizes = [a.shape[:2] for a in out]
    for p, (h, w) in enumerate(sizes):
        c = p % period if period else p
        if c >= C or h > ARROW_SIDE or w > ARROW_SIDE:
            continue
        level = heat_levels(heat[c], full[c], h, w, cell_shift)
        if nv12:
            y, uv = out[p]
            on = level >= min_level
            y[on] = _heat_blend(y[on], table[level[on], 0], table[level[on], 3])
            top = level.reshape(h // 2, 2, w // 2, 2).max(axis=(1, 3))    # the pair's level: the highest of its four luma pixels
            on = top >= min_level
            pairs = uv.reshape(h // 2, w // 2, 2)
            pairs[on] = _heat_blend(pairs[on], table[top[on], 1:3], table[top[on], 3:4])
        else:
            on = level >= min_level
            out[p][on] = _heat_blend(out[p][on], table[level[on], :3], table[level[on], 3:4])
    return out[0] if single else out


# ---------------------------------------------------------------- surface heat map (include/mcgaze_hip.h, "surface heat map")
def surface_cover(h, w, cam, charts, xyz, start, applies):
    """Which region every pixel of an h x w picture shows, by the header's RENDER rule -> (region int64 [h, w], -1: none; t float64 [h, w],
    the depth of its point).  cam: float64 fx fy cx cy; charts: surface_charts_host's; xyz float64 [V,3]; applies: the regions of this
    picture, ascending."""
    with np.errstate(all='ignore'):
        return _surface_cover(h, w, cam, charts, xyz, start, applies)


def _surface_cover(h, w, cam, charts, xyz, start, applies):
    fx, fy, cx, cy = cam
    dx, dy = ((np.arange(w, dtype=np.float64) - cx) / fx)[None, :], ((np.arange(h, dtype=np.float64) - cy) / fy)[:, None]
    best, region = np.full((h, w), np.inf), np.full((h, w), -1, dtype=np.int64)
    for j in applies:
        c = charts[j]
        if c[A.CHART_INDEX['usable']] == 0.0:
            continue
        v0, N, axis = c[0:3], c[9:12], int(c[A.CHART_INDEX['axis']])
        den = (N[0] * dx + N[1] * dy) + N[2] * 1.0
        tn = (N[0] * v0[0] + N[1] * v0[1]) + N[2] * v0[2]
        t = tn / den
        met = (den != 0.0) & np.isfinite(t) & (t > 0.0)
        P = (t * dx, t * dy, t * 1.0)
        iu, iv = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
        pu, pv = P[iu], P[iv]
        v = xyz[start[j]:start[j + 1]]
        inside = np.zeros((h, w), dtype=bool)
        for e in range(len(v)):
            (au, av), (bu, bv) = v[e, [iu, iv]], v[(e + 1) % len(v), [iu, iv]]
            inside ^= ((av > pv) != (bv > pv)) & (pu < au + ((pv - av) * (bu - au)) / (bv - av))
        won = met & inside & (t < best)                           # ascending j and a strict <: the lower index keeps an equal t
        best, region = np.where(won, t, best), np.where(won, j, region)
    return region, best


def surface_levels(h, w, cam, charts, region, t, heat, full):
    """The LEVEL of every pixel from ``surface_cover``'s (region, t): the winner's grid interpolated between cell centres in 64-bit
    integers -> int64 [h, w] in 0 .. 255, 0 where no region covers the pixel or a grid coordinate is not finite."""
    with np.errstate(all='ignore'):
        return _surface_levels(h, w, cam, charts, region, t, heat, full)


def _surface_levels(h, w, cam, charts, region, t, heat, full):
    fx, fy, cx, cy = cam
    M, GH, GW = heat.shape
    dx, dy = np.broadcast_to(((np.arange(w, dtype=np.float64) - cx) / fx)[None, :], (h, w)), \
        np.broadcast_to(((np.arange(h, dtype=np.float64) - cy) / fy)[:, None], (h, w))
    level = np.zeros((h, w), dtype=np.int64)
    on = region >= 0
    if not on.any():
        return level
    j, tt = region[on], t[on]
    P = np.stack([tt * dx[on], tt * dy[on], tt * 1.0], axis=-1)
    fu, fv = A.surface_coords(charts, j, P, GW, GH)
    ok = np.isfinite(fu) & np.isfinite(fv)

    def axis(f, cells):
        g = np.clip(np.floor(np.where(ok, f, 0.0) * 256.0), -2.0 ** 30, 2.0 ** 30)
        U = g.astype(np.int64) - 128
        i0 = U >> 8                                               # arithmetic: floors
        return np.clip(i0, 0, cells - 1), np.clip(i0 + 1, 0, cells - 1), U - i0 * 256

    x0, x1, wx = axis(fu, GW)
    y0, y1, wy = axis(fv, GH)
    grid = np.maximum(heat.astype(np.int64), 0)
    val = (256 - wx) * (256 - wy) * grid[j, y0, x0] + wx * (256 - wy) * grid[j, y0, x1] + (256 - wx) * wy * grid[j, y1, x0] + wx * wy * grid[j, y1, x1]
    L = np.minimum(255, (val * 255) // (65536 * np.maximum(full[j], 1)))
    level[on] = np.where(ok, L, 0)
    return level


def draw_surface_heat_host(frames, heat, full, cam, regions, region_image=None, region_period=0, cam_period=0, lut=None, min_level=1,
                           pixel_format='bgr', matrix='bt601'):
    """The surface heat maps drawn back onto their regions with numpy: what DevicePipeline.draw_surface_heat (mcg_draw_surface_heat /
    mcg_draw_surface_heat_nv12) writes on the device, bit for bit (include/mcgaze_hip.h, "surface heat map": the ray of a pixel, the
    nearest region that covers it, the level from that region's grid; the blend and the NV12 chroma rule are draw_heat_host's).

    frames, pixel_format, matrix, lut, min_level: as for draw_heat_host.  heat: int32 [M, GH, GW] (surface_heat_host); full: int [M], the
    scale of each region -- surface_heat_host's peak -- or one int for all.  cam: [fx, fy, cx, cy] or [C, 4]; picture p has camera p, with
    cam_period p % cam_period, and is left as it is where that camera is not below C, is not finite or has fx, fy <= 0.  regions: the list
    of ``regions_3d`` or a PolyRegions3D, in camera coordinates; region_image [M] (None: -1, every picture) and region_period as
    gaze_targets takes them, with the picture's index in image_of's place.
    -> annotated COPIES in the form given (NV12 frames as (y [H,W], uv [H/2,W]) pairs)."""
    who = 'draw_surface_heat_host'
    nv12, _ = _pixel_format(pixel_format, matrix)
    _, _, region_period = A._target_params(0.0, None, region_period, who)
    _, _, cam_period = A._target3d_params(A.HEAD_SIZE, 'eye', cam_period, who)
    _, min_level = A._heat_scale(who, None, min_level)
    table = heat_lut(lut, nv12, matrix).astype(np.int64)
    xyz32, start = A._surface_regions(who, regions)
    _, _, ri = A._poly3d_tables(who, A.PolyRegions3D(xyz32, start), region_image)
    heat = np.asarray(_host_array(heat))
    M, GH, GW = A._surface_grid(who, heat.shape)
    if M != len(start) - 1:
        raise ValueError(f'{who}: heat holds {M} grids for {len(start) - 1} regions')
    full = np.broadcast_to(np.asarray(_host_array(full), dtype=np.int64).reshape(-1), (M,)) if np.size(full) in (1, M) else None
    if full is None:
        raise ValueError(f'{who}: full is one int or one per region, [{M}]')
    cam64 = A._camera_table(who, cam).astype(np.float64)
    charts, xyz = A.surface_charts_host(A.PolyRegions3D(xyz32, start)), xyz32.astype(np.float64)
    single = not isinstance(frames, list)
    frames = [frames] if single else frames
    if nv12:
        out = [tuple(np.array(p) for p in _nv12_planes(k, f)[:2]) for k, f in enumerate(frames)]
        sizes = [y.shape for y, _ in out]
    else:
        out = [_bgr_frame(k, np.array(f)) for k, f in enumerate(frames)]
        sizes = [a.shape[:2] for a in out]
    for p, (h, w) in enumerate(sizes):
        c = p % cam_period if cam_period else p
        if c >= len(cam64) or h > ARROW_SIDE or w > ARROW_SIDE:
            continue
        k = cam64[c]
        if not (np.isfinite(k).all() and k[0] > 0.0 and k[1] > 0.0):
            continue
        key = p % region_period if region_period else p
        applies = np.flatnonzero((ri < 0) | (ri == key))
        region, t = surface_cover(h, w, k, charts, xyz, start, applies)
        level = surface_levels(h, w, k, charts, region, t, heat, full)
        if nv12:
            y, uv = out[p]
            on = level >= min_level
            y[on] = _heat_blend(y[on], table[level[on], 0], table[level[on], 3])
            top = level.reshape(h // 2, 2, w // 2, 2).max(axis=(1, 3))    # the pair's level: the highest of its four luma pixels
            on = top >= min_level
            pairs = uv.reshape(h // 2, w // 2, 2)
            pairs[on] = _heat_blend(pairs[on], table[top[on], 1:3], table[top[on], 3:4])
        else:
            on = level >= min_level
            out[p][on] = _heat_blend(out[p][on], table[level[on], :3], table[level[on], 3:4])
    return out[0] if single else out


# ---------------------------------------------------------------- anonymised heads (include/mcgaze_hip.h, "anonymised heads")
ANON_SHAPES, ANON_MODES = ('box', 'ellipse'), ('mosaic', 'fill')


def _anon_params(who, expand=0.125, shape='ellipse', cell=None, blocks=8, mode='mosaic'):
    """The options of the anonymising calls, validated (ValueError) -> (expand, shape, cell_shift, blocks, mode) as the entries take them:
    shape 0 box / 1 ellipse, cell_shift 0 (automatic, from ``blocks``) or log2 of ``cell``, mode 0 mosaic / 1 fill.  The defaults are
    conventions, not tuned on data."""
    expand = float(expand)
    if not 0.0 <= expand <= 4.0:
        raise ValueError(f'{who}: expand must lie in 0 .. 4, got {expand!r}')
    if shape not in ANON_SHAPES or mode not in ANON_MODES:
        raise ValueError(f'{who}: shape is one of {ANON_SHAPES} and mode one of {ANON_MODES}, got {shape!r}, {mode!r}')
    if cell is not None and (int(cell) != cell or int(cell) not in (2, 4, 8, 16, 32, 64)):
        raise ValueError(f'{who}: cell must be None or a power of two in 2 .. 64, got {cell!r}')
    if int(blocks) != blocks or not 1 <= int(blocks) <= 64:
        raise ValueError(f'{who}: blocks must be an integer in 1 .. 64, got {blocks!r}')
    return expand, ANON_SHAPES.index(shape), 0 if cell is None else int(cell).bit_length() - 1, int(blocks), ANON_MODES.index(mode)


_ANON_COLORS = {}


def _anon_color(who, color, nv12, matrix):
    """One (B, G, R) triple -> uint8 [3] as the entries take it: with nv12 the (Y, U, V) of bgr_to_yuv, worked out once per colour and
    matrix and kept -- the live path hands in the same colour every tick."""
    one = _arrow_colors(color, 0, False, matrix)[0]
    if color is None or one is None:
        raise ValueError(f'{who}: color must be one (B, G, R) triple')
    if not nv12:
        return np.asarray(one, dtype=np.uint8).reshape(3)
    key = (int(one[0]), int(one[1]), int(one[2]), matrix)
    if key not in _ANON_COLORS:
        _ANON_COLORS[key] = np.asarray(bgr_to_yuv(one, matrix), dtype=np.uint8).reshape(3)
    return _ANON_COLORS[key]


def anonymize_plan_host(boxes, image_of, sizes, expand=0.125, shape='ellipse', cell=None, blocks=8, nv12=False):
    """The plan of "anonymised heads" on the host (anonymize_plan_kernel line for line): boxes [n,4] read as f32 and widened to double,
    image_of [n], sizes [(h, w), ...] of the frames -> a dict of int64 [n] arrays image, flag, x0, y0, x1, y1 (the integer rectangle
    clipped to the frame, half open, possibly empty), cx2, cy2, W, H, shift, shape -- the fields of mcg_anon_desc.  Flag 2: image_of
    outside the table, a coordinate that is not finite, x2 <= x1 or y2 <= y1, an image without pixels, larger than 8192 a side or (nv12)
    of odd size, a rectangle beyond +-8191.  A flagged row is zero but for image = -1."""
    expand, shape, cell_shift, blocks, _ = _anon_params('anonymize_plan_host', expand, shape, cell, blocks)
    b = np.asarray(_host_array(boxes), dtype=np.float32).astype(np.float64).reshape(-1, 4)
    n = len(b)
    image_of = _label_ints('image_of', image_of, n).astype(np.int64)
    hw = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    ok = (image_of >= 0) & (image_of < len(hw)) & np.isfinite(b).all(axis=1)
    b = np.where(ok[:, None], b, 0.0)
    ok &= (b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])
    h, w = (np.where(ok, hw[np.where(ok, image_of, 0), c] if len(hw) else 0, 0) for c in (0, 1))
    ok &= (h > 0) & (w > 0) & (h <= ARROW_SIDE) & (w <= ARROW_SIDE)
    if nv12:
        ok &= ((h | w) & 1) == 0
    # numpy rounds every elementwise product and difference on its own: nothing is contracted, as in the kernel
    ex, ey = expand * (b[:, 2] - b[:, 0]), expand * (b[:, 3] - b[:, 1])
    X0, X1, Y0, Y1 = np.floor(b[:, 0] - ex), np.ceil(b[:, 2] + ex), np.floor(b[:, 1] - ey), np.ceil(b[:, 3] + ey)
    ok &= np.logical_and.reduce([np.abs(v) <= ARROW_COORD for v in (X0, X1, Y0, Y1)])
    X0, X1, Y0, Y1 = (np.where(ok, v, 0.0).astype(np.int64) for v in (X0, X1, Y0, Y1))
    W, H = X1 - X0, Y1 - Y0
    if cell_shift:
        shift = np.full(n, cell_shift, dtype=np.int64)
    else:
        shift = np.full(n, 6, dtype=np.int64)
        for c in range(5, 0, -1):
            shift = np.where((blocks << c) >= np.maximum(W, H), c, shift)
    plan = dict(image=image_of, x0=np.maximum(X0, 0), y0=np.maximum(Y0, 0), x1=np.minimum(X1, w), y1=np.minimum(Y1, h), cx2=X0 + X1, cy2=Y0 + Y1,
                W=W, H=H, shift=shift, shape=np.full(n, shape, dtype=np.int64))
    plan = {k: np.where(ok, v, -1 if k == 'image' else 0).astype(np.int64) for k, v in plan.items()}
    plan['flag'] = np.where(ok, 0, 2).astype(np.int64)
    return plan


def anonymize_coverage(plan, k):
    """(y0, x0, bool [y1 - y0, x1 - x0]): which pixels of the clipped rectangle of row k are covered -- COVERAGE of "anonymised heads", the
    inscribed ellipse tested at pixel centres in 64-bit integers (every pixel of the rectangle for a box)."""
    x0, y0, x1, y1, W, H = (int(plan[f][k]) for f in ('x0', 'y0', 'x1', 'y1', 'W', 'H'))
    py, px = np.mgrid[y0:max(y1, y0), x0:max(x1, x0)].astype(np.int64)
    if not int(plan['shape'][k]):
        return y0, x0, np.ones(py.shape, dtype=bool)
    dx, dy = 2 * px + 1 - int(plan['cx2'][k]), 2 * py + 1 - int(plan['cy2'][k])
    return y0, x0, dx * dx * (H * H) + dy * dy * (W * W) <= W * W * H * H


def _anon_cell_means(plane, s):
    """The mean of every cell of 2^s x 2^s samples of plane [h, w, c], cells aligned to the origin and cut at the right and bottom edges,
    (sum + (count >> 1)) / count in integers -> int64 [h, w, c], each sample's own cell's mean."""
    S = 1 << s
    h, w = plane.shape[:2]
    edges_y, edges_x = np.arange(0, h, S), np.arange(0, w, S)
    sums = np.add.reduceat(np.add.reduceat(plane.astype(np.int64), edges_y, axis=0), edges_x, axis=1)
    count = (np.minimum(edges_y + S, h) - edges_y)[:, None, None] * (np.minimum(edges_x + S, w) - edges_x)[None, :, None]
    mean = (sums + (count >> 1)) // count
    return np.repeat(np.repeat(mean, S, axis=0), S, axis=1)[:h, :w]


def anonymize_heads_host(frames, boxes, image_of=None, expand=0.125, shape='ellipse', cell=None, blocks=8, mode='mosaic', color=(0, 0, 0),
                         pixel_format='bgr', matrix='bt601'):
    """Heads anonymised with numpy: what DevicePipeline.anonymize_heads (mcg_anonymize_heads / mcg_anonymize_heads_nv12) writes on the
    device, bit for bit (include/mcgaze_hip.h, "anonymised heads": the plan, the coverage, the largest shift winning, the cell means of
    the frame as it was, the NV12 chroma rule).  It hides the heads it is given: a head the detector missed stays visible.

    frames, pixel_format, matrix: as for draw_arrows_host.  boxes [n,4] x1 y1 x2 y2, image_of [n] (None: frame 0).  expand: the box grows
    by this share of its size on every side, 0 .. 4; shape 'ellipse' (inscribed in the grown box) or 'box'; cell: None -- about ``blocks``
    (1 .. 64) cells across each head, a power of two of 2 .. 64 pixels -- or that power of two for every head; mode 'mosaic' or 'fill'
    with ``color``, one (B, G, R) triple.  The defaults are conventions, not tuned on data.
    -> (anonymised COPIES in the form given -- NV12 frames as (y [H,W], uv [H/2,W]) pairs --, flags int32 [n]: 0 usable, 2 unusable; a row
    flagged 2 changes no byte)."""
    who = 'anonymize_heads_host'
    nv12, _ = _pixel_format(pixel_format, matrix)
    fill = _anon_params(who, expand, shape, cell, blocks, mode)[4]
    c = _anon_color(who, color, nv12, matrix)
    single = not isinstance(frames, list)
    frames = [frames] if single else frames
    if nv12:
        out = [tuple(np.array(p) for p in _nv12_planes(k, f)[:2]) for k, f in enumerate(frames)]
        sizes = [y.shape for y, _ in out]
    else:
        out = [_bgr_frame(k, np.array(f)) for k, f in enumerate(frames)]
        sizes = [a.shape[:2] for a in out]
    n = len(np.asarray(_host_array(boxes)).reshape(-1, 4))
    image_of = np.zeros(n, dtype=np.int32) if image_of is None else _host_array(image_of)
    plan = anonymize_plan_host(boxes, image_of, sizes, expand, shape, cell, blocks, nv12)
    for p, (h, w) in enumerate(sizes):
        rows = np.flatnonzero((plan['flag'] == 0) & (plan['image'] == p))
        top = np.zeros((h, w), dtype=np.int64)                    # s(p): the largest shift that covers each pixel, 0 for none
        for k in rows:
            y0, x0, covered = anonymize_coverage(plan, k)
            area = top[y0:y0 + covered.shape[0], x0:x0 + covered.shape[1]]
            area[covered] = np.maximum(area[covered], plan['shift'][k])
        if not top.any():
            continue
        if nv12:
            y, uv = out[p]
            pairs, pair_top = uv.reshape(h // 2, w // 2, 2), top.reshape(h // 2, 2, w // 2, 2).max(axis=(1, 3))
            planes = [(y.reshape(h, w, 1), top, 0, c[:1]), (pairs, pair_top, 1, c[1:])]
        else:
            planes = [(out[p], top, 0, c)]
        for plane, level, finer, col in planes:                   # a chroma cell of shift s is 2^(s-1) pairs a side
            before = plane.copy()
            for s in np.unique(level[level > 0]):
                on = level == s
                plane[on] = col if fill else _anon_cell_means(before, int(s) - finer)[on]
    return (out[0] if single else out), plan['flag'].astype(np.int32)
