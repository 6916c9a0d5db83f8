// The attention overlay drawn on the device: what gaze_targets found, made visible in the frames it was found in -- the outlines of the marked
// regions (rectangles and polygons, lit where somebody looks at them), a sight line from every head to the point its look landed on, and the
// demo's arrows coloured by what they point at.  mcg_draw_attention draws into packed BGR frames, mcg_draw_attention_nv12 into a decoder's
// NV12 surfaces, in place.  The arithmetic is stated once, in include/mcgaze_hip.h ("attention overlay");
// mcgaze_amd/arrows.py::draw_attention_host is the same on the host.
//
// draw.hip's design, kept.  Three launches.  overlay_clear_kernel zeroes region_active.  overlay_plan_kernel: thread k plans row k (the arrow
// through arrow_plan_row, the plan of mcg_draw_gaze_arrows term for term; then its sight line) and region k (the usability rules of
// gaze_targets_poly_kernel's staging thread, offsets checked before the first vertex load, then every vertex rounded in double), in double
// and uncontracted, and writes one mcg_stroke_desc per region, per sight line and per arrow -- in that order, which IS the layer order --
// plus the rounded integer vertices of every usable region.  It sets region_active[image_of][target] = 1 for a row that looks at a region:
// no atomics, every writer of a word stores the same value.  overlay_raster_kernel is the GATHER of arrow_raster_kernel over
// (image, pixel tile): each wave ballots 64 records at a time against its strip (flag, picture, bounding box) and walks the hits in
// ASCENDING record order, every lane testing its own pixels against the record's capsules in 64-bit integers, branch-free.  The record of a
// hit is wave-uniform, so its end points -- the 1 or 3 segments of a row, the vertices of a region -- are read through ONE address for the
// whole wave (poly_entry's way): no per-lane array, no LDS.  A lane remembers the LAST record that covered a pixel and stores once after the
// walk: the highest (layer, index) wins whatever the launch geometry, only covered bytes are written, no two threads write the same byte.
// Cost: every wave reads (m + 2 n) / 64 slices of the plan whatever it draws, and a large region's box covers many tiles, each of which
// tests up to 32 capsules per pixel for it (no per-edge reject): made for the tens of heads and regions of a video frame.
#include <climits>

#include "draw_common.hpp"

#define MCG_OVERLAY_REGIONS 4096
#define MCG_OVERLAY_VERTICES 65536
#define MCG_OVERLAY_ACTIVE (1 << 20)   // num_images * m
#define MCG_OVERLAY_POLY_VERTS 32      // = MCG_ATTEND_POLY_VERTS
#define MCG_OVERLAY_VERT_WORDS 64      // per region, in the workspace: 32 vertices x (x, y)

static_assert(sizeof(mcg_stroke_desc) == 24 * sizeof(int), "mcg_stroke_desc is 24 words: the workspace formula of the header");
static_assert(MCG_OVERLAY_POLY_VERTS == MCG_ATTEND_POLY_VERTS, "a region is usable by the rules of mcg_gaze_targets_poly");

struct OverlayPalette {
  unsigned c[7];                                                 // c0 | c1 << 8 | c2 << 16
};

// palette[i] without a dynamic index into a by-value struct (which would live in scratch)
__device__ __forceinline__ unsigned palette_entry(const OverlayPalette& p, int i) {
  unsigned c = p.c[0];
#pragma unroll
  for (int k = 1; k < 7; ++k) c = i == k ? p.c[k] : c;
  return c;
}

__global__ __launch_bounds__(256) void overlay_clear_kernel(int32_t* __restrict__ region_active, int words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < words) region_active[i] = 0;
}

template <class Target>
__global__ __launch_bounds__(256) void overlay_plan_kernel(const typename Target::Image* __restrict__ images, int num_images, int max_h, int max_w,
                                                           const float* __restrict__ boxes, const float* __restrict__ gaze, int gaze_stride,
                                                           const int32_t* __restrict__ image_of, int n, const int32_t* __restrict__ kind,
                                                           const int32_t* __restrict__ target, const float* __restrict__ hit,
                                                           const int32_t* __restrict__ mutual, const float* __restrict__ region_xy, int num_vertices,
                                                           const int32_t* __restrict__ region_start, const int32_t* __restrict__ region_image, int m,
                                                           OverlayPalette palette, double length, int min_thickness, double thickness_ratio,
                                                           double tip_length, int line_thickness, int region_thickness,
                                                           mcg_stroke_desc* __restrict__ strokes, int* __restrict__ ivert, int32_t* __restrict__ flags,
                                                           int32_t* __restrict__ region_flags, int32_t* __restrict__ region_active) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 256 + threadIdx.x;
  const double lim = (double)MCG_DRAW_COORD;
  if (k < n) {
    const mcg_arrow_desc a = arrow_plan_row<Target>(images, num_images, max_h, max_w, boxes, gaze, gaze_stride, image_of, k, length,
                                                    (double)min_thickness, thickness_ratio, tip_length);
    const int kd = kind[k], tg = target[k], io = image_of[k];
    const unsigned color = palette_entry(palette, mutual[k] != 0 ? 4 : (kd >= 1 && kd <= 3 ? kd : 0));
    mcg_stroke_desc arrow = {}, line = {};
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        arrow.seg[s][e][0] = a.seg[s][e][0];
        arrow.seg[s][e][1] = a.seg[s][e][1];
      }
    arrow.thickness = a.thickness;
    arrow.x0 = a.x0; arrow.y0 = a.y0; arrow.x1 = a.x1; arrow.y1 = a.y1;
    arrow.image = a.image;
    arrow.flag = (a.flag == 0 && min_thickness > 0) ? 0 : 2;      // min_thickness 0: the layer is off, the flag of the row is still the plan's
    arrow.layer = 2;
    arrow.count = 3;
    arrow.color = arrow.color_active = color;
    line.image = -1;
    line.flag = 2;
    line.layer = 1;
    line.count = 1;
    line.color = line.color_active = color;
    if (a.flag == 0 && line_thickness > 0 && (kd == 1 || kd == 2)) {
      const double hx = rint((double)hit[2 * (size_t)k]), hy = rint((double)hit[2 * (size_t)k + 1]);
      if (fabs(hx) <= lim && fabs(hy) <= lim) {                  // (a NaN fails every comparison, an infinity this one)
        const typename Target::Image im = images[a.image];      // flag 0: a.image = image_of[k] lies inside the table
        const int cx = a.seg[0][0][0], cy = a.seg[0][0][1], ex = (int)hx, ey = (int)hy;
        const int r = (line_thickness + 1) / 2;
        line.seg[0][0][0] = cx; line.seg[0][0][1] = cy;
        line.seg[0][1][0] = ex; line.seg[0][1][1] = ey;
        line.thickness = line_thickness;
        line.x0 = max(min(cx, ex) - r, 0); line.y0 = max(min(cy, ey) - r, 0);
        line.x1 = min(max(cx, ex) + r + 1, im.w); line.y1 = min(max(cy, ey) + r + 1, im.h);
        line.image = a.image;
        line.flag = 0;
      }
    }
    strokes[m + k] = line;
    strokes[m + n + k] = arrow;
    flags[k] = a.flag;
    // (cleared by the launch before; every writer stores 1)
    if (kd == 2 && tg >= 0 && tg < m && io >= 0 && io < num_images) region_active[(size_t)io * m + tg] = 1;
  }
  if (k < m) {
    const int s = region_start[k], e = region_start[k + 1];       // (k + 1 <= m: the table has m + 1 words)
    const int c = 0 <= s && s <= e && e <= num_vertices ? e - s : 0;          // (whatever the words hold, the difference cannot overflow)
    bool ok = c >= 2 && c <= MCG_OVERLAY_POLY_VERTS;
    const float* xy = region_xy + 2 * (size_t)(ok ? s : 0);       // every vertex below lies inside region_xy[0 .. num_vertices)
    int lo_x = INT_MAX, lo_y = INT_MAX, hi_x = INT_MIN, hi_y = INT_MIN;
    if (ok) {
      for (int v = 0; v < c; ++v) {
        const double x = rint((double)xy[2 * v]), y = rint((double)xy[2 * v + 1]);
        ok = ok && fabs(x) <= lim && fabs(y) <= lim;             // finite, and within the bound of the coverage test
      }
      if (ok && c == 2) ok = !(xy[2] < xy[0]) && !(xy[3] < xy[1]);   // a rectangle is not inverted (the floats, as mcg_gaze_targets_poly reads them)
    }
    mcg_stroke_desc d = {};
    d.image = -1;
    d.flag = 2;
    d.layer = 0;
    d.color = palette_entry(palette, 5);
    d.color_active = palette_entry(palette, 6);
    if (ok) {
      int* out = ivert + (size_t)MCG_OVERLAY_VERT_WORDS * k;
      if (c == 2) {                                              // (x1, y1) (x2, y1) (x2, y2) (x1, y2)
        const int x1 = (int)rint((double)xy[0]), y1 = (int)rint((double)xy[1]), x2 = (int)rint((double)xy[2]), y2 = (int)rint((double)xy[3]);
        out[0] = x1; out[1] = y1; out[2] = x2; out[3] = y1; out[4] = x2; out[5] = y2; out[6] = x1; out[7] = y2;
        lo_x = min(x1, x2); hi_x = max(x1, x2); lo_y = min(y1, y2); hi_y = max(y1, y2);      // (rounding keeps x1 <= x2; min / max cost nothing)
        d.count = 4;
      } else {
        for (int v = 0; v < c; ++v) {
          const int x = (int)rint((double)xy[2 * v]), y = (int)rint((double)xy[2 * v + 1]);
          out[2 * v] = x; out[2 * v + 1] = y;
          lo_x = min(lo_x, x); hi_x = max(hi_x, x); lo_y = min(lo_y, y); hi_y = max(hi_y, y);
        }
        d.count = c;
      }
      // one region may apply to pictures of different sizes: the box is NOT clipped to a frame here, the raster kernel bounds every pixel
      const int r = (region_thickness + 1) / 2;
      d.thickness = region_thickness;
      d.x0 = max(lo_x - r, 0); d.y0 = max(lo_y - r, 0);
      d.x1 = hi_x + r + 1; d.y1 = hi_y + r + 1;
      d.image = region_image[k];
      d.flag = region_thickness > 0 ? 0 : 2;
    }
    strokes[k] = d;
    region_flags[k] = ok ? 0 : 2;
  }
}

template <class Target>
__global__ __launch_bounds__(MCG_DRAW_THREADS) void overlay_raster_kernel(const typename Target::Image* __restrict__ images, int tiles_x, int max_h,
                                                                          int max_w, const mcg_stroke_desc* __restrict__ strokes, int total, int m,
                                                                          int region_period, const int* __restrict__ ivert,
                                                                          const int32_t* __restrict__ region_active) {
  constexpr int S = Target::CELL;
  const int img = blockIdx.y;
  const typename Target::Image im = images[img];
  if (!Target::writable(im) || im.h > max_h || im.w > max_w) return;      // max_h, max_w <= 8192: what the grid covers
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the strip of this wave, in pixels: [sx0, sx1) x [sy0, sy1)
  const int sx0 = tile_x * MCG_DRAW_TILE_W * S, sy0 = (tile_y * MCG_DRAW_TILE_H + 2 * wave) * S;
  const int sx1 = sx0 + MCG_DRAW_TILE_W * S, sy1 = sy0 + 2 * S;
  if (sx0 >= im.w || sy0 >= im.h) return;                       // wave-uniform: the whole strip lies outside this image
  const int px0 = sx0 + (lane & 31) * S, py0 = sy0 + (lane >> 5) * S;   // this lane's cell
  const int img_key = region_period > 0 ? img % region_period : img;
  int win[S * S];
#pragma unroll
  for (int i = 0; i < S * S; ++i) win[i] = -1;
  for (int base = 0; base < total; base += 64) {
    const int r = base + lane;
    bool hit = false;
    if (r < total) {
      const mcg_stroke_desc* d = strokes + r;
      const int key = d->image;
      // a region: every picture, this picture, or this picture's place in the period; a row: its own picture
      const bool here = d->layer == 0 ? (key < 0 || key == img || (region_period > 0 && key == img_key)) : key == img;
      hit = d->flag == 0 && here && d->x0 < sx1 && d->x1 > sx0 && d->y0 < sy1 && d->y1 > sy0;
    }
    unsigned long long mask = __ballot(hit);
    while (mask) {                                              // ascending records: a later one overwrites an earlier one
      const int j = base + __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const mcg_stroke_desc* d = strokes + j;                   // one address for the wave, and so is every end point below
      const int x0 = d->x0, y0 = d->y0, x1 = d->x1, y1 = d->y1, count = d->count;
      const long long tt = (long long)d->thickness * d->thickness;
      int any[S * S];
#pragma unroll
      for (int i = 0; i < S * S; ++i) any[i] = 0;
      if (d->layer == 0) {                                      // uniform: the closed outline v[k] -> v[(k + 1) % count], the closing edge first
        const int* v = ivert + (size_t)MCG_OVERLAY_VERT_WORDS * j;          // (layer 0: j < m)
        int ax = v[2 * (count - 1)], ay = v[2 * (count - 1) + 1];
        for (int k = 0; k < count; ++k) {
          const int bx = v[2 * k], by = v[2 * k + 1];
#pragma unroll
          for (int i = 0; i < S * S; ++i) any[i] |= capsule(px0 + (i % S), py0 + (i / S), ax, ay, bx, by, tt);
          ax = bx;
          ay = by;
        }
      } else {                                                  // 1 segment (a sight line) or 3 (an arrow)
        const int* v = &d->seg[0][0][0];
        for (int g = 0; g < count; ++g) {
          const int ax = v[4 * g], ay = v[4 * g + 1], bx = v[4 * g + 2], by = v[4 * g + 3];
#pragma unroll
          for (int i = 0; i < S * S; ++i) any[i] |= capsule(px0 + (i % S), py0 + (i / S), ax, ay, bx, by, tt);
        }
      }
#pragma unroll
      for (int i = 0; i < S * S; ++i) {
        const int px = px0 + (i % S), py = py0 + (i / S);
        // a row's box is clipped to its frame; a region's is not, so the frame is tested here: a covered pixel has px < w and py < h
        const int in = (int)(px >= x0) & (int)(px < x1) & (int)(py >= y0) & (int)(py < y1) & (int)(px < im.w) & (int)(py < im.h);
        win[i] = (in & any[i]) ? j : win[i];
      }
    }
  }
  int top = -1;
#pragma unroll
  for (int i = 0; i < S * S; ++i) top = max(top, win[i]);
  if (top < 0) return;
  // the colour of record w in this picture: an outline (w < m) is lit where a row of the picture looks at it
  auto color_of = [&](int w) -> unsigned {
    const bool lit = w < m && region_active[(size_t)img * m + w] != 0;
    return lit ? strokes[w].color_active : strokes[w].color;
  };
  if constexpr (S == 1) {
    unsigned char* q = (unsigned char*)im.src + (size_t)py0 * im.pitch + (size_t)px0 * 3;
    const unsigned c = color_of(top);
    q[0] = (unsigned char)c; q[1] = (unsigned char)(c >> 8); q[2] = (unsigned char)(c >> 16);
  } else {
#pragma unroll
    for (int i = 0; i < S * S; ++i)
      if (win[i] >= 0) ((unsigned char*)im.y)[(size_t)(py0 + i / S) * im.pitch_y + px0 + (i % S)] = (unsigned char)color_of(win[i]);
    // px0, py0 even, and some pixel of the block is inside the frame, so (py0, px0) is: py0 >> 1 <= h / 2 - 1, px0 + 1 <= w - 1
    unsigned char* c = (unsigned char*)im.uv + (size_t)(py0 >> 1) * im.pitch_uv + px0;
    const unsigned t = color_of(top);
    c[0] = (unsigned char)(t >> 8);
    c[1] = (unsigned char)(t >> 16);
  }
}

template <class Target>
static int draw_attention(const char* what, mcg_stream stream, const typename Target::Image* images_dev, int num_images, int max_h, int max_w,
                          const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n, const int32_t* kind_dev,
                          const int32_t* target_dev, const float* hit_dev, const int32_t* mutual_dev, const float* region_xy_dev, int num_vertices,
                          const int32_t* region_start_dev, const int32_t* region_image_dev, int m, int region_period, const unsigned char* palette,
                          double length, int min_thickness, double thickness_ratio, double tip_length, int line_thickness, int region_thickness,
                          void* workspace_dev, size_t workspace_bytes, int32_t* flags_dev, int32_t* region_flags_dev, int32_t* region_active_dev) {
  MCG_CHECK_ARG(n >= 0 && n <= 65535, "%s: 0 .. 65535 rows per call (got %d)", what, n);
  MCG_CHECK_ARG(m >= 0 && m <= MCG_OVERLAY_REGIONS, "%s: 0 .. %d regions per call (got %d)", what, MCG_OVERLAY_REGIONS, m);
  MCG_CHECK_ARG(num_vertices >= 0 && num_vertices <= MCG_OVERLAY_VERTICES, "%s: 0 .. %d vertices per call (got %d)", what, MCG_OVERLAY_VERTICES,
                num_vertices);
  MCG_CHECK_ARG(num_images >= 1 && num_images <= 65535 && gaze_stride >= 2 && region_period >= 0,
                "%s: bad sizes images=%d gaze_stride=%d region_period=%d", what, num_images, gaze_stride, region_period);
  MCG_CHECK_ARG((long long)num_images * m <= MCG_OVERLAY_ACTIVE, "%s: num_images * m <= %d (got %d x %d)", what, MCG_OVERLAY_ACTIVE, num_images, m);
  MCG_CHECK_ARG(max_h >= 1 && max_h <= MCG_DRAW_SIDE && max_w >= 1 && max_w <= MCG_DRAW_SIDE, "%s: frames of 1 .. 8192 pixels a side (got max %dx%d)",
                what, max_h, max_w);
  MCG_CHECK_ARG(min_thickness >= 0 && min_thickness <= 255 && line_thickness >= 0 && line_thickness <= 255 && region_thickness >= 0 &&
                    region_thickness <= 255,
                "%s: min_thickness, line_thickness and region_thickness in 0 .. 255 (got %d, %d, %d)", what, min_thickness, line_thickness,
                region_thickness);
  MCG_CHECK_ARG(length - length == 0.0 && thickness_ratio - thickness_ratio == 0.0 && tip_length - tip_length == 0.0,
                "%s: length, thickness_ratio and tip_length must be finite", what);
  MCG_CHECK_ARG(images_dev && palette, "%s: null pointer", what);
  MCG_CHECK_ARG(n == 0 || (boxes_dev && gaze_dev && image_of_dev && kind_dev && target_dev && hit_dev && mutual_dev && flags_dev),
                "%s: null row table with n=%d", what, n);
  MCG_CHECK_ARG(m == 0 || (region_start_dev && region_image_dev && region_flags_dev && region_active_dev), "%s: null region table with m=%d", what, m);
  MCG_CHECK_ARG(num_vertices == 0 || region_xy_dev, "%s: null vertex table with num_vertices=%d", what, num_vertices);
  const int total = m + 2 * n;
  if (total == 0) return MCG_OK;
  const size_t need = sizeof(mcg_stroke_desc) * (size_t)total + sizeof(int) * MCG_OVERLAY_VERT_WORDS * (size_t)m;
  MCG_CHECK_ARG(workspace_dev && workspace_bytes >= need, "%s: workspace of %zu bytes, need %zu", what, workspace_bytes, need);
  mcg_stroke_desc* strokes = (mcg_stroke_desc*)workspace_dev;
  int* ivert = (int*)(strokes + total);
  OverlayPalette pal;
  for (int k = 0; k < 7; ++k) pal.c[k] = palette[3 * k] | (unsigned)palette[3 * k + 1] << 8 | (unsigned)palette[3 * k + 2] << 16;
  if (m) {
    const int words = num_images * m;
    hipLaunchKernelGGL(overlay_clear_kernel, dim3((words + 255) / 256), dim3(256), 0, (hipStream_t)stream, region_active_dev, words);
    MCG_CHECK_LAUNCH("mcg_draw_attention (clear)");
  }
  hipLaunchKernelGGL(overlay_plan_kernel<Target>, dim3((max(n, m) + 255) / 256), dim3(256), 0, (hipStream_t)stream, images_dev, num_images, max_h,
                     max_w, boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, kind_dev, target_dev, hit_dev, mutual_dev, region_xy_dev, num_vertices,
                     region_start_dev, region_image_dev, m, pal, length, min_thickness, thickness_ratio, tip_length, line_thickness, region_thickness,
                     strokes, ivert, flags_dev, region_flags_dev, region_active_dev);
  MCG_CHECK_LAUNCH("mcg_draw_attention (plan)");
  constexpr int S = Target::CELL;
  const int tiles_x = (max_w + MCG_DRAW_TILE_W * S - 1) / (MCG_DRAW_TILE_W * S), tiles_y = (max_h + MCG_DRAW_TILE_H * S - 1) / (MCG_DRAW_TILE_H * S);
  hipLaunchKernelGGL(overlay_raster_kernel<Target>, dim3(tiles_x * tiles_y, num_images), dim3(MCG_DRAW_THREADS), 0, (hipStream_t)stream, images_dev,
                     tiles_x, max_h, max_w, strokes, total, m, region_period, ivert, region_active_dev);
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

#define MCG_OVERLAY_ENTRY(NAME, TARGET, IMAGE)                                                                                                  \
  extern "C" int NAME(mcg_stream s, const IMAGE* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev, const float* gaze_dev,    \
                      int gaze_stride, const int32_t* image_of_dev, int n, const int32_t* kind_dev, const int32_t* target_dev, const float* hit_dev,  \
                      const int32_t* mutual_dev, const float* region_xy_dev, int num_vertices, const int32_t* region_start_dev,                        \
                      const int32_t* region_image_dev, int m, int region_period, const unsigned char* palette, double length, int min_thickness,       \
                      double thickness_ratio, double tip_length, int line_thickness, int region_thickness, void* workspace_dev,                        \
                      size_t workspace_bytes, int32_t* flags_dev, int32_t* region_flags_dev, int32_t* region_active_dev) {                             \
    return draw_attention<TARGET>(#NAME, s, images_dev, num_images, max_h, max_w, boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, kind_dev,        \
                                  target_dev, hit_dev, mutual_dev, region_xy_dev, num_vertices, region_start_dev, region_image_dev, m, region_period, \
                                  palette, length, min_thickness, thickness_ratio, tip_length, line_thickness, region_thickness, workspace_dev,        \
                                  workspace_bytes, flags_dev, region_flags_dev, region_active_dev);                                                    \
  }
MCG_OVERLAY_ENTRY(mcg_draw_attention, PackedTarget, mcg_image_desc)
MCG_OVERLAY_ENTRY(mcg_draw_attention_nv12, Nv12Target, mcg_nv12_image_desc)
