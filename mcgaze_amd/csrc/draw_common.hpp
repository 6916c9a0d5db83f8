// What draw.hip (gaze arrows) and overlay.hip (attention overlay) share: the bounds under which the coverage test is exact, the tile of the
// gather kernels, the two kinds of frame a stroke is drawn into, and the capsule test itself; and what the whole-frame kernels (heat.hip,
// anonymize.hip) share: how a thread reads and writes the 16 pixels of a row it owns.  The arithmetic is stated once, in
// include/mcgaze_hip.h ("annotated frames out").
#pragma once
#include "common.hpp"

#define MCG_DRAW_COORD 8191     // |end point coordinate| <= 8191
#define MCG_DRAW_SIDE 8192      // frames of at most 8192 pixels a side
#define MCG_DRAW_THREADS 256    // 4 waves: a tile of 32 x 8 cells, wave v owns cell rows 2 v and 2 v + 1 (a cell: one pixel; NV12: 2 x 2 pixels)
#define MCG_DRAW_TILE_W 32
#define MCG_DRAW_TILE_H 8

struct PackedTarget {
  using Image = mcg_image_desc;
  static constexpr int CELL = 1;
  static __device__ __forceinline__ bool writable(const Image& im) { return im.h > 0 && im.w > 0; }
};

struct Nv12Target {
  using Image = mcg_nv12_image_desc;
  static constexpr int CELL = 2;
  static __device__ __forceinline__ bool writable(const Image& im) { return im.h > 0 && im.w > 0 && !((im.h | im.w) & 1); }
};

// 4 * (squared distance of p to the segment a -> b) <= t^2, exactly: with |coordinates| <= 8191 and 0 <= p <= 8191 every difference is
// below 2^14 in magnitude, L and |u| below 2^29, |p - a|^2 L and u^2 below 2^58, the left side below 2^60; t^2 L <= 255^2 2^29 < 2^45.
// Branch-free: both sides of the comparison are selected, the result is an int, and the raster kernels combine the box test and the
// segments with & and | -- no divergent control flow inside the row walk.  Keep it so: profiles/draw_capsule_branching_form.md records the
// form with early returns and ||, which this compiler turned into code that tested only the first segment in the 2 x 2 instantiation.
__device__ __forceinline__ int capsule(int px, int py, int ax, int ay, int bx, int by, long long tt) {
  const long long dx = bx - ax, dy = by - ay, qx = px - ax, qy = py - ay, rx = px - bx, ry = py - by;
  const long long L = dx * dx + dy * dy, u = qx * dx + qy * dy, qq = qx * qx + qy * qy, rr = rx * rx + ry * ry;
  const bool before = u <= 0, after = u >= L;
  const long long lhs = before ? qq : after ? rr : qq * L - u * u;
  const long long rhs = (before || after) ? tt : tt * L;
  return (int)(4 * lhs <= rhs);
}

// The ARROW PLAN of one row (include/mcgaze_hip.h, "annotated frames out"), in double and uncontracted: the three segments, the thickness, the
// bounding box clipped to the row's frame and the flag.  arrow_plan_kernel (draw.hip) and overlay_plan_kernel (overlay.hip) are this, so the
// overlay's arrows are the arrows of mcg_draw_gaze_arrows term for term.
template <class Target>
__device__ __forceinline__ mcg_arrow_desc arrow_plan_row(const typename Target::Image* __restrict__ images, int num_images, int max_h, int max_w,
                                                         const float* __restrict__ boxes, const float* __restrict__ gaze, int gaze_stride,
                                                         const int32_t* __restrict__ image_of, int k, double length, double min_thickness,
                                                         double thickness_ratio, double tip_length) {
#pragma clang fp contract(off)
  const double x1 = boxes[4 * k], y1 = boxes[4 * k + 1], x2 = boxes[4 * k + 2], y2 = boxes[4 * k + 3];   // f32 -> double: exact
  const double g0 = gaze[(size_t)k * gaze_stride], g1 = gaze[(size_t)k * gaze_stride + 1];
  const int io = image_of[k];
  mcg_arrow_desc d = {};
  d.image = -1;
  d.flag = 2;
  bool usable = io >= 0 && io < num_images && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && isfinite(g0) && isfinite(g1);
  int h = 0, w = 0;
  if (usable) {
    const typename Target::Image im = images[io];
    h = im.h;
    w = im.w;
    usable = Target::writable(im) && h <= max_h && w <= max_w;   // max_h, max_w <= 8192: what the raster grid covers
  }
  if (usable) {
    // harness.head_arrows: cx = int(x1 + x2) // 2 (truncate, then floor-divide), l = int(max(y2 - y1, x2 - x1) * length), tip = int(c - l * g)
    const double cx = floor(trunc(x1 + x2) / 2.0), cy = floor(trunc(y1 + y2) / 2.0);
    const double l = trunc(fmax(y2 - y1, x2 - x1) * length);
    const double tx = trunc(cx - l * g0), ty = trunc(cy - l * g1);
    const double t = fmax(min_thickness, trunc(l * thickness_ratio));
    const double lim = (double)MCG_DRAW_COORD;
    usable = fabs(cx) <= lim && fabs(cy) <= lim && fabs(tx) <= lim && fabs(ty) <= lim && t <= 255.0;    // (a NaN fails every comparison)
    if (usable) {
      // cv2.arrowedLine's head strokes, p = tip + tip_length * |pt1 - pt2| * (cos, sin)(angle -+ pi / 4), with the angle of pt1 - pt2:
      // |.| (cos, sin)(a -+ pi/4) = sqrt(1/2) (dx +- dy, dy -+ dx) -- no atan2, cos or sin; every product and sum rounded on its own
      const double dx = cx - tx, dy = cy - ty;
      const double kk = tip_length * 0.7071067811865476;
      const double ax = rint(tx + kk * (dx - dy)), ay = rint(ty + kk * (dx + dy));
      const double bx = rint(tx + kk * (dx + dy)), by = rint(ty + kk * (dy - dx));
      usable = fabs(ax) <= lim && fabs(ay) <= lim && fabs(bx) <= lim && fabs(by) <= lim;
      if (usable) {
        const int pt[4][2] = {{(int)cx, (int)cy}, {(int)tx, (int)ty}, {(int)ax, (int)ay}, {(int)bx, (int)by}};
        const int from[3] = {0, 2, 3};                            // shaft pt1 -> pt2, then the two strokes into pt2
        int lo_x = pt[0][0], hi_x = lo_x, lo_y = pt[0][1], hi_y = lo_y;
        for (int s = 0; s < 3; ++s) {
          d.seg[s][0][0] = pt[from[s]][0]; d.seg[s][0][1] = pt[from[s]][1];
          d.seg[s][1][0] = pt[1][0]; d.seg[s][1][1] = pt[1][1];
        }
        for (int p = 1; p < 4; ++p) {
          lo_x = min(lo_x, pt[p][0]); hi_x = max(hi_x, pt[p][0]);
          lo_y = min(lo_y, pt[p][1]); hi_y = max(hi_y, pt[p][1]);
        }
        d.thickness = (int)t;
        const int r = (d.thickness + 1) / 2;                      // >= t / 2: no covered pixel lies outside the box
        d.x0 = max(lo_x - r, 0); d.y0 = max(lo_y - r, 0);
        d.x1 = min(hi_x + r + 1, w); d.y1 = min(hi_y + r + 1, h); // half open; empty (x1 <= x0 or y1 <= y0) for an arrow outside its frame
        d.image = io;
        d.flag = 0;
      }
    }
  }
  return d;
}

// ---------------------------------------------------------------- a thread's span of a pixel row (heat.hip, anonymize.hip)
// W 32-bit words at p, which holds `bytes` bytes this thread may touch.  mode 2: 16-byte accesses, 1: 4-byte accesses (both: bytes == 4 W and
// p aligned to the access), 0: byte by byte, nothing read or written at or behind p + bytes.
template <int W>
__device__ __forceinline__ void span_load(const unsigned char* __restrict__ p, unsigned (&w)[W], int mode, int bytes) {
  if (mode == 2) {
#pragma unroll
    for (int i = 0; i < W / 4; ++i) {
      const uint4 v = ((const uint4*)p)[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
  } else if (mode == 1) {
#pragma unroll
    for (int i = 0; i < W; ++i) w[i] = ((const unsigned*)p)[i];
  } else {
#pragma unroll
    for (int i = 0; i < W; ++i) {
      unsigned v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * i + b < bytes) v |= (unsigned)p[4 * i + b] << (8 * b);
      w[i] = v;
    }
  }
}

template <int W>
__device__ __forceinline__ void span_store(unsigned char* __restrict__ p, const unsigned (&w)[W], int mode, int bytes) {
  if (mode == 2) {
#pragma unroll
    for (int i = 0; i < W / 4; ++i) ((uint4*)p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  } else if (mode == 1) {
#pragma unroll
    for (int i = 0; i < W; ++i) ((unsigned*)p)[i] = w[i];
  } else {
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * i + b < bytes) p[4 * i + b] = (unsigned char)(w[i] >> (8 * b));
  }
}

__device__ __forceinline__ int span_mode(const void* base, int pitch, bool whole) {
  const unsigned long long a = (unsigned long long)base | (unsigned long long)(unsigned)pitch;
  return !whole ? 0 : !(a & 15) ? 2 : !(a & 3) ? 1 : 0;
}

__device__ __forceinline__ unsigned span_byte(const unsigned* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }
__device__ __forceinline__ void span_set_byte(unsigned* w, int i, unsigned v) {
  w[i >> 2] = (w[i >> 2] & ~(255u << (8 * (i & 3)))) | (v << (8 * (i & 3)));
}
