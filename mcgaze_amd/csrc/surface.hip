// Surface heat maps on the device (include/mcgaze_hip.h, "surface heat map"): where ON a planar region -- a screen, a shelf, a poster -- looks
// have landed, as a grid in the region's own coordinates.  hit3d of "gaze targets, 3-D" is taken into the region's CHART and accumulated
// (mcg_surface_heat_add); the grids are drawn back onto their regions in packed BGR frames (mcg_draw_surface_heat) or NV12 surfaces
// (mcg_draw_surface_heat_nv12) with the right perspective, in place.  Everything up to the first floor is double and uncontracted, everything
// behind it integer, stated once, in the header; mcgaze_amd/attention.py::surface_heat_host and mcgaze_amd/arrows.py::draw_surface_heat_host
// are the same on the host, bit for bit.
//
// surface_plan_kernel, one thread per region, is the first launch of both entries: it writes each region's chart as 20 doubles into the
// caller's workspace, and the scatter and the render read that table -- the chart is worked out once, by one piece of code.  Accumulating is
// then heat.hip's three launches with the region in the camera's place: clear, a scatter of one thread per (row, tap row) with integer vector
// atomics, the per-cell update (heat_common.hpp).
//
// surface_render_kernel: a block owns a tile of 256 x 16 pixels (NV12: 256 x 32) of one picture, as heat_render_kernel does.  It first lists
// in LDS the regions that apply to the picture, have a usable chart and whose projected bounding box -- of the vertices moved along the dropped
// axis onto the plane, grown by a pixel -- touches the tile (a region with such a point at z <= 0 has no such box and is listed for every
// tile); the list is a cull only, the exact test per pixel decides.  A thread owns 16 pixels of a row (NV12: 16 x 2 and their 8 chroma pairs).  For every pixel it walks the list -- the list entry is the same in
// every lane, so a region's chart and vertices come through uniform addresses --, keeps the nearest region that covers the pixel, takes the
// pixel's level from that region's grid, and packs the levels into 64-bit words (no array with a dynamic index: no scratch).  A tile with an
// empty list and a thread whose levels are all below min_level read no pixel; the others blend through heat_blend_span.  No atomics in
// global memory, no scratch.  LDS: the list (4096 ints), the ramp (256 words) and a counter.
#include "heat_common.hpp"   // the clear and update launches, the blend, a thread's span of pixels (shared with heat.hip)
#include "region3d.hpp"      // a 3-D region: usable, normal, dropped axis, the even-odd test (shared with attend.hip)

#define MCG_SURF_ROWS 65536
#define MCG_SURF_REGIONS 4096
#define MCG_SURF_VERTICES 65536
#define MCG_SURF_CAMERAS 4096
#define MCG_SURF_SIDE 1024                  // cells a side of a grid
#define MCG_SURF_COORD 16384.0              // |fu|, |fv| of a row that counts
#define MCG_SURF_TILE_W (16 * MCG_HEAT_SPAN)
// a chart: v0 (0 1 2), a (3 4 5), b (6 7 8), N (9 10 11), aa, bb, smin, ws, rmin, hr, usable (1 / 0), the dropped axis (0 1 2)
#define MCG_SURF_CHART 20
static_assert(MCG_SURF_CHART * sizeof(double) == MCG_SURFACE_CHART_BYTES, "the workspace formula of the header");

// ---------------------------------------------------------------- the chart
__global__ __launch_bounds__(256) void surface_plan_kernel(const float* __restrict__ xyz, int num_vertices, const int32_t* __restrict__ region_start,
                                                           int M, double* __restrict__ charts) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  const region3d r = region3d_load(xyz, num_vertices, region_start, j);
  bool ok = r.usable;
  double ax = 0.0, ay = 0.0, az = 0.0, bx = 0.0, by = 0.0, bz = 0.0, aa = 0.0, bb = 0.0, smin = 0.0, smax = 0.0, rmin = 0.0, rmax = 0.0;
  if (ok) {
    const float* v = xyz + 3 * (size_t)r.start;
    ax = (double)v[3] - r.v0x, ay = (double)v[4] - r.v0y, az = (double)v[5] - r.v0z;
    bx = r.Ny * az - r.Nz * ay, by = r.Nz * ax - r.Nx * az, bz = r.Nx * ay - r.Ny * ax;
    aa = (ax * ax + ay * ay) + az * az;
    bb = (bx * bx + by * by) + bz * bz;
    for (int k = 0; k < r.count; ++k) {                          // the region's own vertices, ascending
      const double wx = (double)v[3 * k] - r.v0x, wy = (double)v[3 * k + 1] - r.v0y, wz = (double)v[3 * k + 2] - r.v0z;
      const double s = ((wx * ax + wy * ay) + wz * az) / aa, q = ((wx * bx + wy * by) + wz * bz) / bb;
      smin = k == 0 ? s : s < smin ? s : smin;
      smax = k == 0 ? s : s > smax ? s : smax;
      rmin = k == 0 ? q : q < rmin ? q : rmin;
      rmax = k == 0 ? q : q > rmax ? q : rmax;
    }
  }
  const double ws = smax - smin, hr = rmax - rmin;
  ok = ok && isfinite(aa) && aa > 0.0 && isfinite(bb) && bb > 0.0 && isfinite(ws) && ws > 0.0 && isfinite(hr) && hr > 0.0;
  double* c = charts + (size_t)MCG_SURF_CHART * j;               // a chart that is not usable is all zero
  c[0] = ok ? r.v0x : 0.0; c[1] = ok ? r.v0y : 0.0; c[2] = ok ? r.v0z : 0.0;
  c[3] = ok ? ax : 0.0; c[4] = ok ? ay : 0.0; c[5] = ok ? az : 0.0;
  c[6] = ok ? bx : 0.0; c[7] = ok ? by : 0.0; c[8] = ok ? bz : 0.0;
  c[9] = ok ? r.Nx : 0.0; c[10] = ok ? r.Ny : 0.0; c[11] = ok ? r.Nz : 0.0;
  c[12] = ok ? aa : 0.0; c[13] = ok ? bb : 0.0;
  c[14] = ok ? smin : 0.0; c[15] = ok ? ws : 0.0; c[16] = ok ? rmin : 0.0; c[17] = ok ? hr : 0.0;
  c[18] = ok ? 1.0 : 0.0;
  c[19] = ok ? (double)r.axis : 0.0;
}

// The grid coordinates of Q in the usable chart c.
__device__ __forceinline__ void surface_coords(const double* __restrict__ c, double Qx, double Qy, double Qz, int GW, int GH, double& fu, double& fv) {
#pragma clang fp contract(off)
  const double wx = Qx - c[0], wy = Qy - c[1], wz = Qz - c[2];
  const double s = ((wx * c[3] + wy * c[4]) + wz * c[5]) / c[12];
  const double q = ((wx * c[6] + wy * c[7]) + wz * c[8]) / c[13];
  fu = ((s - c[14]) / c[15]) * (double)GW;
  fv = ((q - c[16]) / c[17]) * (double)GH;
}

// ---------------------------------------------------------------- accumulate
__global__ __launch_bounds__(256) void surface_scatter_kernel(const float* __restrict__ hit3d, const int32_t* __restrict__ kind,
                                                              const int32_t* __restrict__ target, const int32_t* __restrict__ flags,
                                                              const int32_t* __restrict__ mask, int n, const double* __restrict__ charts,
                                                              int32_t* __restrict__ work, int M, int GH, int GW, int radius) {
#pragma clang fp contract(off)
  const int T = 2 * radius + 1;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int k = t / T;
  if (k >= n) return;
  const int dy = t - k * T - radius;
  // THE ROW RULE, in the header's order
  if (flags && flags[k] != 0) return;
  if (mask && mask[k] == 0) return;
  if (kind[k] != 2) return;
  const int j = target[k];
  if (j < 0 || j >= M) return;
  const double* c = charts + (size_t)MCG_SURF_CHART * j;
  if (c[18] == 0.0) return;
  const double Qx = hit3d[3 * (size_t)k], Qy = hit3d[3 * (size_t)k + 1], Qz = hit3d[3 * (size_t)k + 2];   // f32 -> double: exact
  if (!(isfinite(Qx) && isfinite(Qy) && isfinite(Qz))) return;
  double fu, fv;
  surface_coords(c, Qx, Qy, Qz, GW, GH, fu, fv);
  if (!(fabs(fu) <= MCG_SURF_COORD && fabs(fv) <= MCG_SURF_COORD)) return;     // (a NaN fails the test)
  const int ix = (int)floor(fu), iy = (int)floor(fv);
  const int y = iy + dy;
  if (y < 0 || y >= GH) return;
  const int wy = radius + 1 - abs(dy);
  int32_t* row = work + ((size_t)j * GH + y) * GW;
  for (int dx = -radius; dx <= radius; ++dx) {
    const int x = ix + dx;
    if (x >= 0 && x < GW) atomicAdd(row + x, wy * (radius + 1 - abs(dx)));      // at most 65536 rows of 81: the sum stays below 2^23
  }
}

static int surface_regions_ok(const char* what, const float* xyz, int num_vertices, const int32_t* region_start, int M, int GH, int GW) {
  MCG_CHECK_ARG(M >= 1 && M <= MCG_SURF_REGIONS && GH >= 1 && GH <= MCG_SURF_SIDE && GW >= 1 && GW <= MCG_SURF_SIDE,
                "%s: 1 .. 4096 regions with grids of 1 .. 1024 cells a side (got %d x %d x %d)", what, M, GH, GW);
  MCG_CHECK_ARG((long long)M * GH * GW <= MCG_HEAT_MAX_CELLS, "%s: at most 2^24 cells (got %d x %d x %d)", what, M, GH, GW);
  MCG_CHECK_ARG(num_vertices >= 0 && num_vertices <= MCG_SURF_VERTICES, "%s: 0 .. %d vertices per call (got %d)", what, MCG_SURF_VERTICES, num_vertices);
  MCG_CHECK_ARG(region_start && (num_vertices == 0 || xyz), "%s: null region table", what);
  return MCG_OK;
}

extern "C" int mcg_surface_heat_add(mcg_stream s, const float* hit3d_dev, const int32_t* kind_dev, const int32_t* target_dev, const int32_t* flags_dev,
                                    const int32_t* mask_dev, int n, const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev, int M,
                                    int32_t* heat_dev, int32_t* peak_dev, int GH, int GW, int radius, int decay_shift, void* workspace_dev,
                                    size_t workspace_bytes) {
  const char* what = "mcg_surface_heat_add";
  MCG_CHECK_ARG(n >= 0 && n <= MCG_SURF_ROWS, "%s: at most 65536 rows per call (got %d)", what, n);
  MCG_CHECK_ARG(heat_dev && peak_dev && workspace_dev && (n == 0 || (hit3d_dev && kind_dev && target_dev)), "%s: null pointer", what);
  MCG_TRY(surface_regions_ok(what, region_xyz_dev, num_vertices, region_start_dev, M, GH, GW));
  MCG_CHECK_ARG(radius >= 0 && radius <= 8 && decay_shift >= 0 && decay_shift <= 30, "%s: radius in 0 .. 8, decay_shift in 0 .. 30 (got %d, %d)", what,
                radius, decay_shift);
  const int cells = GH * GW, all = M * cells;
  const size_t need = (size_t)MCG_SURFACE_CHART_BYTES * M + 4 * (size_t)all;
  MCG_CHECK_ARG(((uintptr_t)workspace_dev & 7) == 0, "%s: the workspace must be aligned to 8 bytes", what);
  MCG_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed", what, workspace_bytes, need);
  double* charts = (double*)workspace_dev;
  int32_t* work = (int32_t*)(charts + (size_t)MCG_SURF_CHART * M);
  hipLaunchKernelGGL(surface_plan_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)s, region_xyz_dev, num_vertices, region_start_dev, M, charts);
  MCG_CHECK_LAUNCH("mcg_surface_heat_add (plan)");
  hipLaunchKernelGGL(heat_clear_kernel, dim3((max(all, M) + 255) / 256), dim3(256), 0, (hipStream_t)s, work, all, peak_dev, M);
  MCG_CHECK_LAUNCH("mcg_surface_heat_add (clear)");
  // n == 0: one block whose threads all leave -- the number of launches does not depend on the tables' sizes
  hipLaunchKernelGGL(surface_scatter_kernel, dim3((max(n, 1) * (2 * radius + 1) + 255) / 256), dim3(256), 0, (hipStream_t)s, hit3d_dev, kind_dev,
                     target_dev, flags_dev, mask_dev, n, charts, work, M, GH, GW, radius);
  MCG_CHECK_LAUNCH("mcg_surface_heat_add (scatter)");
  hipLaunchKernelGGL(heat_update_kernel, dim3((cells + 255) / 256, M), dim3(256), 0, (hipStream_t)s, heat_dev, work, peak_dev, cells, decay_shift);
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

// ---------------------------------------------------------------- render
// floor(f * 256) - 128 as an integer; f is finite.  Beyond +-2^30 the floor is held there: both cells are then the same edge cell, so no
// level changes, and the conversion is defined for every finite f.
__device__ __forceinline__ long long surface_fixed(double f) {
#pragma clang fp contract(off)
  double g = floor(f * 256.0);
  g = g < -1073741824.0 ? -1073741824.0 : g > 1073741824.0 ? 1073741824.0 : g;
  return (long long)g - 128;
}

template <class Target>
__global__ __launch_bounds__(256) void surface_render_kernel(const typename Target::Image* __restrict__ images, int tiles_x, int max_h, int max_w,
                                                             const float* __restrict__ cam, int C, int cam_period, const float* __restrict__ xyz,
                                                             const int32_t* __restrict__ region_start, const int32_t* __restrict__ region_image, int M,
                                                             int region_period, const double* __restrict__ charts, const int32_t* __restrict__ heat,
                                                             const int32_t* __restrict__ full_dev, int GH, int GW, const unsigned* __restrict__ lut,
                                                             int min_level) {
#pragma clang fp contract(off)
  constexpr int R = Target::CELL;                                 // pixel rows of a thread: 1, NV12 2
  constexpr int TILE_H = 16 * R;
  __shared__ int list[MCG_SURF_REGIONS];
  __shared__ unsigned colour[256];
  __shared__ int listed;
  const int img = blockIdx.y;
  const int c = cam_period == 0 ? img : img % cam_period;
  if (c >= C) return;
  const typename Target::Image im = images[img];
  if (!Target::writable(im) || im.h > max_h || im.w > max_w) return;
  const double fx = cam[4 * (size_t)c], fy = cam[4 * (size_t)c + 1], cx = cam[4 * (size_t)c + 2], cy = cam[4 * (size_t)c + 3];      // f32 -> double: exact
  if (!(isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy) && fx > 0.0 && fy > 0.0)) return;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int tx0 = tile_x * MCG_SURF_TILE_W, ty0 = tile_y * TILE_H;
  if (tx0 >= im.w || ty0 >= im.h) return;                         // block-uniform, like every return above: nobody waits at the barrier
  if (threadIdx.x == 0) listed = 0;
  colour[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  // ---- the regions of this tile.  A cull: it may list a region that covers no pixel here, never drop one that covers one.  The exact test
  // takes the polygon along the dropped axis, on the plane through v0: a covered pixel's point lies in the polygon of the vertices MOVED
  // ALONG THAT AXIS ONTO THE PLANE (the vertices themselves need not be coplanar), so with every moved vertex in front of the lens the
  // pixel lies in the box of their projections.
  const int rkey = region_period > 0 ? img % region_period : img;
  const double lo_x = (double)tx0, hi_x = (double)(tx0 + MCG_SURF_TILE_W - 1), lo_y = (double)ty0, hi_y = (double)(ty0 + TILE_H - 1);
  for (int base = 0; base < M; base += 256) {
    const int j = base + threadIdx.x;
    const double* ch = charts + (size_t)MCG_SURF_CHART * min(j, M - 1);
    if (j < M && ch[18] != 0.0) {
      const int ri = region_image[j];
      if (ri < 0 || ri == rkey) {
        const int s = region_start[j], cnt = region_start[j + 1] - s;        // (a usable chart: the offsets were checked by the plan launch)
        const float* v = xyz + 3 * (size_t)s;
        const double Nx = ch[9], Ny = ch[10], Nz = ch[11];
        const int axis = (int)ch[19];
        const double Na = axis == 0 ? Nx : axis == 1 ? Ny : Nz;   // the largest |N| component: not zero
        double u0 = 0.0, u1 = 0.0, v0 = 0.0, v1 = 0.0;
        bool behind = false;
        for (int k = 0; k < cnt; ++k) {
          double x = v[3 * k], y = v[3 * k + 1], z = v[3 * k + 2];
          const double off = ((Nx * (x - ch[0]) + Ny * (y - ch[1])) + Nz * (z - ch[2])) / Na;      // how far the vertex is off the plane, along the axis
          x = axis == 0 ? x - off : x;
          y = axis == 1 ? y - off : y;
          z = axis == 2 ? z - off : z;
          if (!(z > 0.0)) behind = true;                          // (a NaN counts as behind)
          const double pu = fx * (x / z) + cx, pv = fy * (y / z) + cy;
          u0 = k == 0 || pu < u0 ? pu : u0;
          u1 = k == 0 || pu > u1 ? pu : u1;
          v0 = k == 0 || pv < v0 ? pv : v0;
          v1 = k == 0 || pv > v1 ? pv : v1;
        }
        const bool miss = u1 + 1.0 < lo_x || u0 - 1.0 > hi_x || v1 + 1.0 < lo_y || v0 - 1.0 > hi_y;      // (a NaN misses nothing)
        if (behind || !miss) list[atomicAdd(&listed, 1)] = j;     // (an LDS atomic; the order of the list cannot show: see the choice below)
      }
    }
  }
  __syncthreads();
  const int count = listed;
  if (count == 0) return;                                         // uniform: nothing can cover a pixel of this tile, none is read

  const int px0 = tx0 + (threadIdx.x & 15) * MCG_HEAT_SPAN, py0 = ty0 + (threadIdx.x >> 4) * R;
  if (px0 >= im.w || py0 >= im.h) return;                         // (no barrier below)
  // the levels of the thread's pixels, 8 to a word, pixel p = 16 r + i in word p >> 3
  unsigned long long lv0 = 0, lv1 = 0, lv2 = 0, lv3 = 0;
  int most = 0;
  const int pixels = min(MCG_HEAT_SPAN, im.w - px0);
  for (int p = 0; p < MCG_HEAT_SPAN * R; ++p) {
    const int i = p & (MCG_HEAT_SPAN - 1), r = p >> 4;            // (NV12: py0 even and < h, h even: both rows are inside)
    if (i >= pixels) continue;
    const double dx = ((double)(px0 + i) - cx) / fx, dy = ((double)(py0 + r) - cy) / fy, dz = 1.0;
    double best = HUGE_VAL;
    int best_j = -1;
    for (int e = 0; e < count; ++e) {
      const int j = __builtin_amdgcn_readfirstlane(list[e]);      // the same word in every lane: the chart and the vertices through uniform addresses
      const double* ch = charts + (size_t)MCG_SURF_CHART * j;
      const double Nx = ch[9], Ny = ch[10], Nz = ch[11];
      const double den = (Nx * dx + Ny * dy) + Nz * dz;
      const double tn = (Nx * ch[0] + Ny * ch[1]) + Nz * ch[2];
      const double t = tn / den;
      if (!(den != 0.0 && isfinite(t) && t > 0.0)) continue;
      if (!(t < best || (t == best && j < best_j))) continue;     // the smallest t, then the lower index: whatever the order of the list
      const int s = region_start[j], cnt = region_start[j + 1] - s;
      if (region3d_inside(xyz + 3 * (size_t)s, cnt, (int)ch[19], t * dx, t * dy, t * dz)) {
        best = t;
        best_j = j;
      }
    }
    int L = 0;
    if (best_j >= 0) {
      double fu, fv;
      surface_coords(charts + (size_t)MCG_SURF_CHART * best_j, best * dx, best * dy, best * dz, GW, GH, fu, fv);
      if (isfinite(fu) && isfinite(fv)) {
        const long long U = surface_fixed(fu), V = surface_fixed(fv);
        const int i0 = (int)(U >> 8), j0 = (int)(V >> 8);         // arithmetic shifts: floors
        const long long wx = U - (long long)i0 * 256, wy = V - (long long)j0 * 256;
        const int ia = min(max(i0, 0), GW - 1), ib = min(max(i0 + 1, 0), GW - 1), ja = min(max(j0, 0), GH - 1), jb = min(max(j0 + 1, 0), GH - 1);
        const int32_t* grid = heat + (size_t)best_j * GH * GW;
        const long long h00 = max(grid[(size_t)ja * GW + ia], 0), h01 = max(grid[(size_t)ja * GW + ib], 0), h10 = max(grid[(size_t)jb * GW + ia], 0),
                        h11 = max(grid[(size_t)jb * GW + ib], 0);
        const long long val = (256 - wx) * (256 - wy) * h00 + wx * (256 - wy) * h01 + (256 - wx) * wy * h10 + wx * wy * h11;    // below 2^47
        L = heat_level((val * 255) >> 16, (long long)max(full_dev[best_j], 1));
      }
    }
    most = max(most, L);
    const unsigned long long bits = (unsigned long long)L << (8 * (p & 7));
    const int word = p >> 3;
    lv0 |= word == 0 ? bits : 0ull;
    lv1 |= word == 1 ? bits : 0ull;
    if constexpr (R == 2) {
      lv2 |= word == 2 ? bits : 0ull;
      lv3 |= word == 3 ? bits : 0ull;
    }
  }
  if (most < min_level) return;                                   // none of this thread's pixels is written: none is read either
  int level[R][MCG_HEAT_SPAN];
#pragma unroll
  for (int i = 0; i < MCG_HEAT_SPAN; ++i) {
    level[0][i] = (int)(((i < 8 ? lv0 : lv1) >> (8 * (i & 7))) & 255ull);
    if constexpr (R == 2) level[1][i] = (int)(((i < 8 ? lv2 : lv3) >> (8 * (i & 7))) & 255ull);
  }
  heat_blend_span<Target>(im, px0, py0, level, colour, min_level);
}

template <class Target>
static int draw_surface_heat(const char* what, mcg_stream stream, const typename Target::Image* images_dev, int num_images, int max_h, int max_w,
                             const float* cam_dev, int C, int cam_period, const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev,
                             const int32_t* region_image_dev, int M, int region_period, const int32_t* heat_dev, const int32_t* full_dev, int GH, int GW,
                             const unsigned char* lut_dev, int min_level, void* workspace_dev, size_t workspace_bytes) {
  MCG_CHECK_ARG(images_dev && cam_dev && region_image_dev && heat_dev && full_dev && lut_dev && workspace_dev, "%s: null pointer", what);
  MCG_CHECK_ARG(num_images >= 1 && num_images <= 65535, "%s: 1 .. 65535 images (got %d)", what, num_images);
  MCG_CHECK_ARG(max_h >= 1 && max_h <= MCG_DRAW_SIDE && max_w >= 1 && max_w <= MCG_DRAW_SIDE, "%s: frames of 1 .. 8192 pixels a side (got max %dx%d)",
                what, max_h, max_w);
  MCG_CHECK_ARG(C >= 1 && C <= MCG_SURF_CAMERAS && cam_period >= 0 && region_period >= 0, "%s: 1 .. 4096 cameras, periods >= 0 (got %d, %d, %d)", what, C,
                cam_period, region_period);
  MCG_TRY(surface_regions_ok(what, region_xyz_dev, num_vertices, region_start_dev, M, GH, GW));
  MCG_CHECK_ARG(min_level >= 1 && min_level <= 255, "%s: min_level in 1 .. 255 (got %d)", what, min_level);
  MCG_CHECK_ARG(((uintptr_t)lut_dev & 3) == 0, "%s: the colour table must be aligned to 4 bytes", what);
  const size_t need = (size_t)MCG_SURFACE_CHART_BYTES * M;
  MCG_CHECK_ARG(((uintptr_t)workspace_dev & 7) == 0, "%s: the workspace must be aligned to 8 bytes", what);
  MCG_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed", what, workspace_bytes, need);
  double* charts = (double*)workspace_dev;
  hipLaunchKernelGGL(surface_plan_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, region_xyz_dev, num_vertices, region_start_dev, M,
                     charts);
  MCG_CHECK_LAUNCH("mcg_draw_surface_heat (plan)");
  constexpr int TILE_H = 16 * Target::CELL;
  const int tiles_x = (max_w + MCG_SURF_TILE_W - 1) / MCG_SURF_TILE_W, tiles_y = (max_h + TILE_H - 1) / TILE_H;
  hipLaunchKernelGGL(surface_render_kernel<Target>, dim3(tiles_x * tiles_y, num_images), dim3(256), 0, (hipStream_t)stream, images_dev, tiles_x, max_h,
                     max_w, cam_dev, C, cam_period, region_xyz_dev, region_start_dev, region_image_dev, M, region_period, charts, heat_dev, full_dev, GH,
                     GW, (const unsigned*)lut_dev, min_level);
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

extern "C" int mcg_draw_surface_heat(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* cam_dev, int C,
                                     int cam_period, const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev,
                                     const int32_t* region_image_dev, int M, int region_period, const int32_t* heat_dev, const int32_t* full_dev, int GH,
                                     int GW, const unsigned char* lut_dev, int min_level, void* workspace_dev, size_t workspace_bytes) {
  return draw_surface_heat<PackedTarget>("mcg_draw_surface_heat", s, images_dev, num_images, max_h, max_w, cam_dev, C, cam_period, region_xyz_dev,
                                         num_vertices, region_start_dev, region_image_dev, M, region_period, heat_dev, full_dev, GH, GW, lut_dev, min_level,
                                         workspace_dev, workspace_bytes);
}

extern "C" int mcg_draw_surface_heat_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const float* cam_dev,
                                          int C, int cam_period, const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev,
                                          const int32_t* region_image_dev, int M, int region_period, const int32_t* heat_dev, const int32_t* full_dev,
                                          int GH, int GW, const unsigned char* lut_dev, int min_level, void* workspace_dev, size_t workspace_bytes) {
  return draw_surface_heat<Nv12Target>("mcg_draw_surface_heat_nv12", s, images_dev, num_images, max_h, max_w, cam_dev, C, cam_period, region_xyz_dev,
                                       num_vertices, region_start_dev, region_image_dev, M, region_period, heat_dev, full_dev, GH, GW, lut_dev, min_level,
                                       workspace_dev, workspace_bytes);
}
