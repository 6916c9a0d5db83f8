// Gaze targets on the device: what every head looks at -- another head of its picture, a marked region, the lens, or nothing.  The ray is the
// demo's arrow (MCGaze_demo/demo.ipynb, cell 5: from the head's centre towards centre - l * gaze[:2]) followed until it meets something.  The
// arithmetic is stated once, in include/mcgaze_hip.h ("gaze targets"); mcgaze_amd/attention.py::gaze_targets_host is the same on the host.
//
// Two launches.  gaze_targets_kernel: one thread per SOURCE row, 256-thread workgroups, everything in double and uncontracted like
// arrow_plan_kernel.  Candidate rows go through LDS in tiles of 256 (the grown box and image_of; -1 for a row that cannot be looked at) and
// while a tile is staged the workgroup takes the min and max image_of of its usable rows: a tile whose range cannot contain a picture of any
// searching row of the workgroup is skipped in a workgroup-uniform branch, which is what makes the [k, Q, S] tables of live gaze (pictures in
// ascending row order) cost one picture per row, not n.  Regions are staged the same way, keyed by region_image.  A thread walks the
// candidates in ASCENDING index, heads before regions, and replaces its best only on a strictly smaller t: the winner is a function of the
// inputs alone -- a skipped tile holds no candidate of the workgroup, so the launch geometry cannot show.  gaze_mutual_kernel needs every
// target and is a second launch.  No atomics in global memory, no scratch; LDS: 256 x (4 doubles + 1 int) and a few words.
//
// Polygonal regions ("gaze targets, polygonal regions" in the header; mcg_gaze_targets_poly -> gaze_targets_poly_kernel).  Rows, head phase,
// choice and outputs are those above -- gaze_targets_body<POLY> states them once and both kernels are that body.  A region is a run of
// vertices of region_xy named by region_start.  The staging thread of a region checks its two offsets BEFORE its first vertex load, walks its
// vertices once for finiteness and puts key, start and count into LDS (a 2-vertex region also its rectangle, for the slab test as it is); a
// region that is not usable is "no candidate" and none of its vertices is read again.  The searching threads walk the tile's regions in
// ascending order and a polygon's vertices through a UNIFORM ADDRESS: start and count come out of LDS at an index every thread shares, so
// every lane of a wave loads the same region_xy word at the same time (one cache line, broadcast) -- no LDS staging of vertices.  The
// previous vertex is carried in registers; there is no local array.  No bounding-box reject: every edge is tested.  LDS: + 2 x 256 ints.
#include <climits>

#include "common.hpp"
#include "region3d.hpp"   // a 3-D region: usable, normal, dropped axis, the even-odd test (shared with surface.hip)

#define MCG_ATTEND_ROWS 65536
#define MCG_ATTEND_REGIONS 4096
#define MCG_ATTEND_THREADS 256   // the tile of candidates is one per thread
#define MCG_ATTEND_VERTICES 65536 // (at most MCG_ATTEND_POLY_VERTS a polygon: the header)
#define MCG_ATTEND_CAMERAS 4096   // rows of the camera table of mcg_gaze_targets_3d

// The slab test of one candidate rectangle against the ray o + t d, t >= 0 (d not both zero).  -> the entry t, or -1 for a miss.
__device__ __forceinline__ double slab_entry(double ox, double oy, double dx, double dy, double lox, double loy, double hix, double hiy) {
#pragma clang fp contract(off)
  double near = -HUGE_VAL, far = HUGE_VAL;
  bool pass = true;
  if (dx == 0.0) {
    pass = lox <= ox && ox <= hix;
  } else {
    const double t1 = (lox - ox) / dx, t2 = (hix - ox) / dx;
    near = t1 < t2 ? t1 : t2;
    far = t1 < t2 ? t2 : t1;
  }
  if (dy == 0.0) {
    pass = pass && loy <= oy && oy <= hiy;
  } else {
    const double t1 = (loy - oy) / dy, t2 = (hiy - oy) / dy;
    const double lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1;
    near = lo > near ? lo : near;
    far = hi < far ? hi : far;
  }
  const double t = near > 0.0 ? near : 0.0;
  return (pass && near <= far && far >= 0.0 && isfinite(t)) ? t : -1.0;
}

// One polygon (c >= 3 finite vertices at xy, checked by the staging thread) against the ray: even-odd INSIDE -> +0, else the smallest t of
// the CROSSED edges.  -> the entry t, or -1 for a miss.  xy is the same address in every lane.
__device__ __forceinline__ double poly_entry(double ox, double oy, double dx, double dy, const float* __restrict__ xy, int c) {
#pragma clang fp contract(off)
  const double fx = xy[0], fy = xy[1];
  double ax = fx, ay = fy, best = HUGE_VAL;
  bool inside = false;
  for (int k = 1; k <= c; ++k) {                                 // edge k - 1: a = v[k - 1] -> b = v[k mod c]
    const double bx = k < c ? (double)xy[2 * k] : fx, by = k < c ? (double)xy[2 * k + 1] : fy;
    const double ex = bx - ax, ey = by - ay, wx = ax - ox, wy = ay - oy;
    if ((ay > oy) != (by > oy) && ox < ax + ((oy - ay) * ex) / ey) inside = !inside;
    const double den = dx * ey - dy * ex, tn = wx * ey - wy * ex, sn = wx * dy - wy * dx;
    if ((den > 0.0 && tn >= 0.0 && sn >= 0.0 && sn <= den) || (den < 0.0 && tn <= 0.0 && sn <= 0.0 && sn >= den)) {
      const double q = tn / den;
      const double t = q > 0.0 ? q : 0.0;
      if (isfinite(t) && t < best) best = t;
    }
    ax = bx;
    ay = by;
  }
  return inside ? 0.0 : best < HUGE_VAL ? best : -1.0;
}

// Both kernels.  POLY false: regions is f32 [m][4] rectangles (region_start and num_vertices are not read).  POLY true: regions is region_xy
// f32 [num_vertices][2] and region j owns the vertices region_start[j] .. region_start[j + 1] - 1.
template <bool POLY>
__device__ __forceinline__ void gaze_targets_body(const float* __restrict__ boxes, const float* __restrict__ gaze, int gaze_stride,
                                                  const int32_t* __restrict__ image_of, int n, const float* __restrict__ regions, int num_vertices,
                                                  const int32_t* __restrict__ region_start, const int32_t* __restrict__ region_image, int m,
                                                  int region_period, double expand, double camera_cos2, int32_t* __restrict__ kind,
                                                  int32_t* __restrict__ target, float* __restrict__ t_out, float* __restrict__ hit,
                                                  int32_t* __restrict__ flags) {
#pragma clang fp contract(off)
  __shared__ double c_lox[MCG_ATTEND_THREADS], c_loy[MCG_ATTEND_THREADS], c_hix[MCG_ATTEND_THREADS], c_hiy[MCG_ATTEND_THREADS];
  __shared__ int c_key[MCG_ATTEND_THREADS];                      // a head's image_of / a region's region_image; INT_MIN: no candidate
  __shared__ int c_start[POLY ? MCG_ATTEND_THREADS : 1], c_count[POLY ? MCG_ATTEND_THREADS : 1];      // a region's first vertex and their number
  __shared__ int src_lo, src_hi, srk_lo, srk_hi, tile_lo, tile_hi, tile_any;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * MCG_ATTEND_THREADS + tid;
  if (tid == 0) {
    src_lo = srk_lo = INT_MAX;
    src_hi = srk_hi = INT_MIN;
  }
  // ---- this thread's own row
  int io = -1, my_kind = 0, my_flag = 2;
  double ox = 0.0, oy = 0.0, dx = 0.0, dy = 0.0;
  bool searching = false;
  if (i < n) {
    const double x1 = boxes[4 * (size_t)i], y1 = boxes[4 * (size_t)i + 1], x2 = boxes[4 * (size_t)i + 2], y2 = boxes[4 * (size_t)i + 3];
    const float* g = gaze + (size_t)i * gaze_stride;
    const double gx = g[0], gy = g[1], gz = g[2];                // f32 -> double: exact
    io = image_of[i];
    const bool usable = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && isfinite(gx) && isfinite(gy) && isfinite(gz) && !(x2 < x1) &&
                        !(y2 < y1) && io >= 0;
    if (usable) {
      my_flag = 0;
      if (gz < 0.0 && gz * gz >= camera_cos2 * ((gx * gx + gy * gy) + gz * gz)) {
        my_kind = 3;
      } else {
        ox = (x1 + x2) * 0.5;
        oy = (y1 + y2) * 0.5;
        dx = -gx;
        dy = -gy;
        searching = !(dx == 0.0 && dy == 0.0);
      }
    } else {
      io = -1;
    }
  }
  const int my_rkey = region_period > 0 && io >= 0 ? io % region_period : io;
  __syncthreads();
  if (searching) {                                               // the pictures this workgroup asks about (LDS atomics: order-free results)
    atomicMin(&src_lo, io);
    atomicMax(&src_hi, io);
    atomicMin(&srk_lo, my_rkey);
    atomicMax(&srk_hi, my_rkey);
  }
  __syncthreads();
  const int wg_lo = src_lo, wg_hi = src_hi, wgr_lo = srk_lo, wgr_hi = srk_hi;
  double best = HUGE_VAL;
  int best_target = -1;
  if (wg_lo <= wg_hi) {                                          // uniform: somebody searches
    // ---- heads, in tiles of 256 rows
    for (int base = 0; base < n; base += MCG_ATTEND_THREADS) {
      __syncthreads();                                           // the tile before has been read
      if (tid == 0) {
        tile_lo = INT_MAX;
        tile_hi = INT_MIN;
      }
      const int j = base + tid;
      int key = INT_MIN;
      if (j < n) {
        const double x1 = boxes[4 * (size_t)j], y1 = boxes[4 * (size_t)j + 1], x2 = boxes[4 * (size_t)j + 2], y2 = boxes[4 * (size_t)j + 3];
        const float* g = gaze + (size_t)j * gaze_stride;
        const double gx = g[0], gy = g[1], gz = g[2];
        const int jo = image_of[j];
        if (isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && isfinite(gx) && isfinite(gy) && isfinite(gz) && !(x2 < x1) && !(y2 < y1) &&
            jo >= 0) {
          const double w = x2 - x1, h = y2 - y1;
          const double e = expand * (w > h ? w : h);
          c_lox[tid] = x1 - e;
          c_loy[tid] = y1 - e;
          c_hix[tid] = x2 + e;
          c_hiy[tid] = y2 + e;
          key = jo;
        }
      }
      c_key[tid] = key;
      __syncthreads();
      if (key != INT_MIN) {
        atomicMin(&tile_lo, key);
        atomicMax(&tile_hi, key);
      }
      __syncthreads();
      if (tile_hi < wg_lo || tile_lo > wg_hi) continue;          // uniform: no row of this tile is in a picture this workgroup asks about
      if (searching) {
        const int count = min(MCG_ATTEND_THREADS, n - base);
        for (int c = 0; c < count; ++c) {
          if (c_key[c] != io || base + c == i) continue;
          const double t = slab_entry(ox, oy, dx, dy, c_lox[c], c_loy[c], c_hix[c], c_hiy[c]);
          if (t >= 0.0 && t < best) {
            best = t;
            best_target = base + c;
            my_kind = 1;
          }
        }
      }
    }
    // ---- regions, the same way; a head wins an equal t, so a region replaces only on a strictly smaller one
    for (int base = 0; base < m; base += MCG_ATTEND_THREADS) {
      __syncthreads();
      if (tid == 0) {
        tile_lo = INT_MAX;
        tile_hi = INT_MIN;
        tile_any = 0;
      }
      const int j = base + tid;
      int key = INT_MIN;
      if (j < m) {
        size_t first = 4 * (size_t)j;                            // the rectangle's four floats: x1 y1 x2 y2
        bool ok = true;
        if constexpr (POLY) {
          const int s = region_start[j], e = region_start[j + 1];     // (j + 1 <= m: the table has m + 1 words)
          const int c = 0 <= s && s <= e && e <= num_vertices ? e - s : 0;      // (whatever the words hold, the difference cannot overflow)
          ok = c >= 2 && c <= MCG_ATTEND_POLY_VERTS;
          if (ok) {                                              // every vertex below lies inside region_xy[0 .. num_vertices)
            first = 2 * (size_t)s;
            for (int k = 0; k < 2 * c; ++k) ok = ok && isfinite(regions[first + k]);
            c_start[tid] = s;
            c_count[tid] = c;
          }
        }
        if (ok && (!POLY || c_count[tid] == 2)) {
          const double x1 = regions[first], y1 = regions[first + 1], x2 = regions[first + 2], y2 = regions[first + 3];
          ok = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && !(x2 < x1) && !(y2 < y1);
          c_lox[tid] = x1;
          c_loy[tid] = y1;
          c_hix[tid] = x2;
          c_hiy[tid] = y2;
        }
        if (ok) key = region_image[j] < 0 ? -1 : region_image[j];
      }
      c_key[tid] = key;
      __syncthreads();
      if (key == -1) {
        tile_any = 1;                                            // (every writer stores the same value)
      } else if (key != INT_MIN) {
        atomicMin(&tile_lo, key);
        atomicMax(&tile_hi, key);
      }
      __syncthreads();
      if (!tile_any && (tile_hi < wgr_lo || tile_lo > wgr_hi)) continue;   // uniform
      if (searching) {
        const int count = min(MCG_ATTEND_THREADS, m - base);
        for (int c = 0; c < count; ++c) {
          const int rk = c_key[c];
          if (rk == INT_MIN || (rk != -1 && rk != my_rkey)) continue;
          double t;
          if (POLY && c_count[POLY ? c : 0] != 2) {              // (c_start, c_count: one LDS word for the whole workgroup -> a uniform address)
            t = poly_entry(ox, oy, dx, dy, regions + 2 * (size_t)c_start[POLY ? c : 0], c_count[POLY ? c : 0]);
          } else {
            t = slab_entry(ox, oy, dx, dy, c_lox[c], c_loy[c], c_hix[c], c_hiy[c]);
          }
          if (t >= 0.0 && t < best) {
            best = t;
            best_target = base + c;
            my_kind = 2;
          }
        }
      }
    }
  }
  if (i >= n) return;
  const bool found = my_kind == 1 || my_kind == 2;
  kind[i] = my_kind;
  target[i] = found ? best_target : -1;
  t_out[i] = found ? (float)best : 0.0f;
  hit[2 * (size_t)i] = found ? (float)(ox + best * dx) : 0.0f;
  hit[2 * (size_t)i + 1] = found ? (float)(oy + best * dy) : 0.0f;
  flags[i] = my_flag;
}

__global__ __launch_bounds__(MCG_ATTEND_THREADS) void gaze_targets_kernel(const float* __restrict__ boxes, const float* __restrict__ gaze,
                                                                          int gaze_stride, const int32_t* __restrict__ image_of, int n,
                                                                          const float* __restrict__ regions,
                                                                          const int32_t* __restrict__ region_image, int m, int region_period,
                                                                          double expand, double camera_cos2, int32_t* __restrict__ kind,
                                                                          int32_t* __restrict__ target, float* __restrict__ t_out,
                                                                          float* __restrict__ hit, int32_t* __restrict__ flags) {
  gaze_targets_body<false>(boxes, gaze, gaze_stride, image_of, n, regions, 0, nullptr, region_image, m, region_period, expand, camera_cos2, kind, target,
                           t_out, hit, flags);
}

__global__ __launch_bounds__(MCG_ATTEND_THREADS) void gaze_targets_poly_kernel(const float* __restrict__ boxes, const float* __restrict__ gaze,
                                                                               int gaze_stride, const int32_t* __restrict__ image_of, int n,
                                                                               const float* __restrict__ region_xy, int num_vertices,
                                                                               const int32_t* __restrict__ region_start,
                                                                               const int32_t* __restrict__ region_image, int m, int region_period,
                                                                               double expand, double camera_cos2, int32_t* __restrict__ kind,
                                                                               int32_t* __restrict__ target, float* __restrict__ t_out,
                                                                               float* __restrict__ hit, int32_t* __restrict__ flags) {
  gaze_targets_body<true>(boxes, gaze, gaze_stride, image_of, n, region_xy, num_vertices, region_start, region_image, m, region_period, expand,
                          camera_cos2, kind, target, t_out, hit, flags);
}

__global__ __launch_bounds__(MCG_ATTEND_THREADS) void gaze_mutual_kernel(const int32_t* __restrict__ kind, const int32_t* __restrict__ target, int n,
                                                                         int32_t* __restrict__ mutual) {
  const int i = blockIdx.x * MCG_ATTEND_THREADS + threadIdx.x;
  if (i >= n) return;
  int v = 0;
  if (kind[i] == 1) {
    const int r = target[i];
    if (r >= 0 && r < n) v = kind[r] == 1 && target[r] == i;     // (r is a row index the first launch wrote: always in range)
  }
  mutual[i] = v;
}

// Both entries: their checks, then the two launches.  poly false: regions_dev is [m][4] rectangles; true: region_xy [num_vertices][2].
static int gaze_targets_launch(const char* what, bool poly, mcg_stream stream, const float* boxes_dev, const float* gaze_dev, int gaze_stride,
                               const int32_t* image_of_dev, int n, const float* regions_dev, int num_vertices, const int32_t* region_start_dev,
                               const int32_t* region_image_dev, int m, int region_period, double expand, double camera_cos2, int32_t* kind_dev,
                               int32_t* target_dev, float* t_dev, float* hit_dev, int32_t* mutual_dev, int32_t* flags_dev) {
  MCG_CHECK_ARG(n >= 0 && n <= MCG_ATTEND_ROWS, "%s: 0 .. %d rows per call (got %d)", what, MCG_ATTEND_ROWS, n);
  MCG_CHECK_ARG(m >= 0 && m <= MCG_ATTEND_REGIONS, "%s: 0 .. %d regions per call (got %d)", what, MCG_ATTEND_REGIONS, m);
  MCG_CHECK_ARG(gaze_stride >= 3 && region_period >= 0, "%s: bad sizes gaze_stride=%d region_period=%d", what, gaze_stride, region_period);
  MCG_CHECK_ARG(expand >= 0.0 && expand - expand == 0.0 && camera_cos2 == camera_cos2, "%s: expand must be finite and not negative, camera_cos2 a number",
                what);
  MCG_CHECK_ARG(n == 0 || (boxes_dev && gaze_dev && image_of_dev && kind_dev && target_dev && t_dev && hit_dev && mutual_dev && flags_dev),
                "%s: null pointer", what);
  if (poly) {
    MCG_CHECK_ARG(num_vertices >= 0 && num_vertices <= MCG_ATTEND_VERTICES, "%s: 0 .. %d vertices per call (got %d)", what, MCG_ATTEND_VERTICES,
                  num_vertices);
    MCG_CHECK_ARG(m == 0 || (region_start_dev && region_image_dev), "%s: null region table with m=%d", what, m);
    MCG_CHECK_ARG(num_vertices == 0 || regions_dev, "%s: null vertex table with num_vertices=%d", what, num_vertices);
  } else {
    MCG_CHECK_ARG(m == 0 || (regions_dev && region_image_dev), "%s: null region table with m=%d", what, m);
  }
  if (n == 0) return MCG_OK;
  const dim3 grid((n + MCG_ATTEND_THREADS - 1) / MCG_ATTEND_THREADS), block(MCG_ATTEND_THREADS);
  if (poly) {
    hipLaunchKernelGGL(gaze_targets_poly_kernel, grid, block, 0, (hipStream_t)stream, boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, regions_dev,
                       num_vertices, region_start_dev, region_image_dev, m, region_period, expand, camera_cos2, kind_dev, target_dev, t_dev, hit_dev,
                       flags_dev);
  } else {
    hipLaunchKernelGGL(gaze_targets_kernel, grid, block, 0, (hipStream_t)stream, boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, regions_dev,
                       region_image_dev, m, region_period, expand, camera_cos2, kind_dev, target_dev, t_dev, hit_dev, flags_dev);
  }
  MCG_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(gaze_mutual_kernel, grid, block, 0, (hipStream_t)stream, kind_dev, target_dev, n, mutual_dev);
  MCG_CHECK_LAUNCH(poly ? "mcg_gaze_targets_poly (mutual)" : "mcg_gaze_targets (mutual)");
  return MCG_OK;
}

extern "C" int mcg_gaze_targets(mcg_stream stream, const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n,
                                const float* regions_dev, const int32_t* region_image_dev, int m, int region_period, double expand, double camera_cos2,
                                int32_t* kind_dev, int32_t* target_dev, float* t_dev, float* hit_dev, int32_t* mutual_dev, int32_t* flags_dev) {
  return gaze_targets_launch("mcg_gaze_targets", false, stream, boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, regions_dev, 0, nullptr,
                             region_image_dev, m, region_period, expand, camera_cos2, kind_dev, target_dev, t_dev, hit_dev, mutual_dev, flags_dev);
}

extern "C" int mcg_gaze_targets_poly(mcg_stream stream, const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev,
                                     int n, const float* region_xy_dev, int num_vertices, const int32_t* region_start_dev,
                                     const int32_t* region_image_dev, int m, int region_period, double expand, double camera_cos2, int32_t* kind_dev,
                                     int32_t* target_dev, float* t_dev, float* hit_dev, int32_t* mutual_dev, int32_t* flags_dev) {
  return gaze_targets_launch("mcg_gaze_targets_poly", true, stream, boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, region_xy_dev, num_vertices,
                             region_start_dev, region_image_dev, m, region_period, expand, camera_cos2, kind_dev, target_dev, t_dev, hit_dev, mutual_dev,
                             flags_dev);
}

// ---------------------------------------------------------------- gaze targets, 3-D ("gaze targets, 3-D" in the header; mcg_gaze_targets_3d)
// The same search in CAMERA SPACE: a row is lifted to O = (X, Y, Z) with the intrinsics of its camera and a depth (the caller's, or from the
// size of the head), its gaze becomes a direction D there, the candidates are boxes around the other rows' O and planar polygons.  One thread
// per source row, candidates through LDS in tiles of 256 (6 doubles and a key: a head's lo / hi corners, a region's normal and first vertex),
// the min / max image_of tile skip, a polygon's vertices through a uniform address with the previous vertex in registers -- the scheme of
// gaze_targets_body.  gaze_mutual_kernel is the second launch.  No global atomics, no scratch.
struct row3d {
  bool usable;
  int io;
  double x1, y1, x2, y2, gx, gy, gz, fx, fy, cx, cy, X, Y, Z;
};

// Row j in camera space (the header's UNUSABLE, CAMERA TABLE, DEPTH and ORIGIN).  Nothing but row j of the row tables and row c < num_cameras
// of cam is read.
__device__ __forceinline__ row3d lift_row(const float* __restrict__ boxes, const float* __restrict__ gaze, int gaze_stride,
                                          const int32_t* __restrict__ image_of, const float* __restrict__ cam, int num_cameras, int cam_period,
                                          const float* __restrict__ depth, double head_size, int j) {
#pragma clang fp contract(off)
  row3d r;
  r.usable = false;
  r.x1 = boxes[4 * (size_t)j], r.y1 = boxes[4 * (size_t)j + 1], r.x2 = boxes[4 * (size_t)j + 2], r.y2 = boxes[4 * (size_t)j + 3];
  const float* g = gaze + (size_t)j * gaze_stride;
  r.gx = g[0], r.gy = g[1], r.gz = g[2];                         // f32 -> double: exact
  r.io = image_of[j];
  r.fx = r.fy = r.cx = r.cy = r.X = r.Y = r.Z = 0.0;
  if (!(isfinite(r.x1) && isfinite(r.y1) && isfinite(r.x2) && isfinite(r.y2) && isfinite(r.gx) && isfinite(r.gy) && isfinite(r.gz) && !(r.x2 < r.x1) &&
        !(r.y2 < r.y1) && r.io >= 0))
    return r;
  const int c = cam_period > 0 ? r.io % cam_period : r.io;
  if (c >= num_cameras) return r;
  r.fx = cam[4 * (size_t)c], r.fy = cam[4 * (size_t)c + 1], r.cx = cam[4 * (size_t)c + 2], r.cy = cam[4 * (size_t)c + 3];
  if (!(isfinite(r.fx) && isfinite(r.fy) && isfinite(r.cx) && isfinite(r.cy) && r.fx > 0.0 && r.fy > 0.0)) return r;
  double Z = depth ? (double)depth[j] : 0.0;
  if (!(depth && isfinite(Z) && Z > 0.0)) {
    const double w = r.x2 - r.x1, h = r.y2 - r.y1;
    Z = (r.fx * head_size) / (w > h ? w : h);
  }
  if (!(isfinite(Z) && Z > 0.0)) return r;
  r.Z = Z;
  r.X = ((((r.x1 + r.x2) * 0.5) - r.cx) * Z) / r.fx;
  r.Y = ((((r.y1 + r.y2) * 0.5) - r.cy) * Z) / r.fy;
  r.usable = isfinite(r.X) && isfinite(r.Y);
  return r;
}

// One axis of the slab test: d == 0 passes iff lo <= o <= hi and gives no bound.
__device__ __forceinline__ void slab_axis(double o, double d, double lo, double hi, double& near, double& far, bool& pass) {
#pragma clang fp contract(off)
  if (d == 0.0) {
    pass = pass && lo <= o && o <= hi;
  } else {
    const double t1 = (lo - o) / d, t2 = (hi - o) / d;
    const double l = t1 < t2 ? t1 : t2, h = t1 < t2 ? t2 : t1;
    near = l > near ? l : near;
    far = h < far ? h : far;
  }
}

__global__ __launch_bounds__(MCG_ATTEND_THREADS) void gaze_targets_3d_kernel(
    const float* __restrict__ boxes, const float* __restrict__ gaze, int gaze_stride, const int32_t* __restrict__ image_of, int n,
    const float* __restrict__ cam, int num_cameras, int cam_period, const float* __restrict__ depth, double head_size, int frame,
    const float* __restrict__ xyz, int num_vertices, const int32_t* __restrict__ region_start, const int32_t* __restrict__ region_image, int m,
    int region_period, double expand, double camera_cos2, int32_t* __restrict__ kind, int32_t* __restrict__ target, float* __restrict__ t_out,
    float* __restrict__ hit, int32_t* __restrict__ flags, float* __restrict__ hit3d) {
#pragma clang fp contract(off)
  // a head: lo (a b c) and hi (d e f) of its box; a region: its normal (a b c) and first vertex (d e f)
  __shared__ double c_a[MCG_ATTEND_THREADS], c_b[MCG_ATTEND_THREADS], c_c[MCG_ATTEND_THREADS], c_d[MCG_ATTEND_THREADS], c_e[MCG_ATTEND_THREADS],
      c_f[MCG_ATTEND_THREADS];
  __shared__ int c_key[MCG_ATTEND_THREADS];                      // a head's image_of / a region's region_image; INT_MIN: no candidate
  __shared__ int c_start[MCG_ATTEND_THREADS], c_count[MCG_ATTEND_THREADS], c_axis[MCG_ATTEND_THREADS];
  __shared__ int src_lo, src_hi, srk_lo, srk_hi, tile_lo, tile_hi, tile_any;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * MCG_ATTEND_THREADS + tid;
  if (tid == 0) {
    src_lo = srk_lo = INT_MAX;
    src_hi = srk_hi = INT_MIN;
  }
  // ---- this thread's own row
  int io = -1, my_kind = 0, my_flag = 2;
  double X = 0.0, Y = 0.0, Z = 0.0, Dx = 0.0, Dy = 0.0, Dz = 0.0, fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0;
  bool searching = false;
  if (i < n) {
    const row3d r = lift_row(boxes, gaze, gaze_stride, image_of, cam, num_cameras, cam_period, depth, head_size, i);
    if (r.usable) {
      my_flag = 0;
      io = r.io;
      X = r.X, Y = r.Y, Z = r.Z, fx = r.fx, fy = r.fy, cx = r.cx, cy = r.cy;
      const double gx = r.gx, gy = r.gy, gz = r.gz;
      bool lens;
      if (frame == 0) {
        Dx = -gx, Dy = -gy, Dz = gz;
        const double s = -((Dx * X + Dy * Y) + Dz * Z);
        lens = s > 0.0 && s * s >= camera_cos2 * (((Dx * Dx + Dy * Dy) + Dz * Dz) * ((X * X + Y * Y) + Z * Z));
      } else {
        const double a2 = X * X + Z * Z;
        const double a = (double)sqrtf((float)a2), rr = (double)sqrtf((float)(a2 + Y * Y));
        const double p = gx * rr, q = gz * a;
        Dx = ((q * X) - (p * Z)) + (gy * (X * Y));
        Dy = (q * Y) - (gy * a2);
        Dz = ((q * Z) + (p * X)) + (gy * (Y * Z));
        lens = gz < 0.0 && gz * gz >= camera_cos2 * ((gx * gx + gy * gy) + gz * gz);
      }
      if (lens) {
        my_kind = 3;
      } else {
        searching = isfinite(Dx) && isfinite(Dy) && isfinite(Dz) && !(Dx == 0.0 && Dy == 0.0 && Dz == 0.0);
      }
    }
  }
  const int my_rkey = region_period > 0 && io >= 0 ? io % region_period : io;
  __syncthreads();
  if (searching) {                                               // the pictures this workgroup asks about (LDS atomics: order-free results)
    atomicMin(&src_lo, io);
    atomicMax(&src_hi, io);
    atomicMin(&srk_lo, my_rkey);
    atomicMax(&srk_hi, my_rkey);
  }
  __syncthreads();
  const int wg_lo = src_lo, wg_hi = src_hi, wgr_lo = srk_lo, wgr_hi = srk_hi;
  double best = HUGE_VAL;
  int best_target = -1;
  if (wg_lo <= wg_hi) {                                          // uniform: somebody searches
    // ---- heads, in tiles of 256 rows
    for (int base = 0; base < n; base += MCG_ATTEND_THREADS) {
      __syncthreads();                                           // the tile before has been read
      if (tid == 0) {
        tile_lo = INT_MAX;
        tile_hi = INT_MIN;
      }
      const int j = base + tid;
      int key = INT_MIN;
      if (j < n) {
        const row3d r = lift_row(boxes, gaze, gaze_stride, image_of, cam, num_cameras, cam_period, depth, head_size, j);
        if (r.usable) {
          const double w = r.x2 - r.x1, h = r.y2 - r.y1;
          const double e = expand * (w > h ? w : h);
          const double hw = (((w * 0.5) + e) * r.Z) / r.fx, hh = (((h * 0.5) + e) * r.Z) / r.fy;
          const double hd = hw > hh ? hw : hh;
          c_a[tid] = r.X - hw;
          c_b[tid] = r.Y - hh;
          c_c[tid] = r.Z - hd;
          c_d[tid] = r.X + hw;
          c_e[tid] = r.Y + hh;
          c_f[tid] = r.Z + hd;
          key = r.io;
        }
      }
      c_key[tid] = key;
      __syncthreads();
      if (key != INT_MIN) {
        atomicMin(&tile_lo, key);
        atomicMax(&tile_hi, key);
      }
      __syncthreads();
      if (tile_hi < wg_lo || tile_lo > wg_hi) continue;          // uniform: no row of this tile is in a picture this workgroup asks about
      if (searching) {
        const int count = min(MCG_ATTEND_THREADS, n - base);
        for (int c = 0; c < count; ++c) {
          if (c_key[c] != io || base + c == i) continue;
          double near = -HUGE_VAL, far = HUGE_VAL;
          bool pass = true;
          slab_axis(X, Dx, c_a[c], c_d[c], near, far, pass);
          slab_axis(Y, Dy, c_b[c], c_e[c], near, far, pass);
          slab_axis(Z, Dz, c_c[c], c_f[c], near, far, pass);
          const double t = near > 0.0 ? near : 0.0;
          if (pass && near <= far && far >= 0.0 && isfinite(t) && t < best) {
            best = t;
            best_target = base + c;
            my_kind = 1;
          }
        }
      }
    }
    // ---- regions, the same way; a head wins an equal t, so a region replaces only on a strictly smaller one
    for (int base = 0; base < m; base += MCG_ATTEND_THREADS) {
      __syncthreads();
      if (tid == 0) {
        tile_lo = INT_MAX;
        tile_hi = INT_MIN;
        tile_any = 0;
      }
      const int j = base + tid;
      int key = INT_MIN;
      if (j < m) {
        const region3d r = region3d_load(xyz, num_vertices, region_start, j);    // (the offsets are checked before the first vertex load)
        const bool ok = r.usable;
        if (ok) {
          c_a[tid] = r.Nx;
          c_b[tid] = r.Ny;
          c_c[tid] = r.Nz;
          c_d[tid] = r.v0x;
          c_e[tid] = r.v0y;
          c_f[tid] = r.v0z;
          c_start[tid] = r.start;
          c_count[tid] = r.count;
          c_axis[tid] = r.axis;
        }
        if (ok) key = region_image[j] < 0 ? -1 : region_image[j];
      }
      c_key[tid] = key;
      __syncthreads();
      if (key == -1) {
        tile_any = 1;                                            // (every writer stores the same value)
      } else if (key != INT_MIN) {
        atomicMin(&tile_lo, key);
        atomicMax(&tile_hi, key);
      }
      __syncthreads();
      if (!tile_any && (tile_hi < wgr_lo || tile_lo > wgr_hi)) continue;   // uniform
      if (searching) {
        const int count = min(MCG_ATTEND_THREADS, m - base);
        for (int c = 0; c < count; ++c) {
          const int rk = c_key[c];
          if (rk == INT_MIN || (rk != -1 && rk != my_rkey)) continue;
          const double Nx = c_a[c], Ny = c_b[c], Nz = c_c[c];
          const double den = (Nx * Dx + Ny * Dy) + Nz * Dz;
          const double tn = (Nx * (c_d[c] - X) + Ny * (c_e[c] - Y)) + Nz * (c_f[c] - Z);
          if (!(den != 0.0)) continue;
          const double q = tn / den;
          if (!(isfinite(q) && q >= 0.0)) continue;
          const double t = q > 0.0 ? q : 0.0;
          if (!(t < best)) continue;                             // (it could not win: its polygon need not be walked)
          const double Px = X + t * Dx, Py = Y + t * Dy, Pz = Z + t * Dz;
          // (c_axis, c_count, c_start: one LDS word for the whole workgroup -> uniform addresses in the walk)
          const bool inside = region3d_inside(xyz + 3 * (size_t)c_start[c], c_count[c], c_axis[c], Px, Py, Pz);
          if (inside) {
            best = t;
            best_target = base + c;
            my_kind = 2;
          }
        }
      }
    }
  }
  if (i >= n) return;
  const bool found = my_kind == 1 || my_kind == 2;
  const double Px = X + best * Dx, Py = Y + best * Dy, Pz = Z + best * Dz;
  const float nan32 = __int_as_float(0x7fc00000);
  float hx = 0.0f, hy = 0.0f;
  if (found) {
    const double u = fx * (Px / Pz) + cx, v = fy * (Py / Pz) + cy;
    hx = Pz > 0.0 && u == u ? (float)u : nan32;                  // one NaN: the quiet one, whatever the arithmetic made
    hy = Pz > 0.0 && v == v ? (float)v : nan32;
  }
  kind[i] = my_kind;
  target[i] = found ? best_target : -1;
  t_out[i] = found ? (float)best : 0.0f;
  hit[2 * (size_t)i] = hx;
  hit[2 * (size_t)i + 1] = hy;
  flags[i] = my_flag;
  hit3d[3 * (size_t)i] = found ? (float)Px : 0.0f;
  hit3d[3 * (size_t)i + 1] = found ? (float)Py : 0.0f;
  hit3d[3 * (size_t)i + 2] = found ? (float)Pz : 0.0f;
}

extern "C" int mcg_gaze_targets_3d(mcg_stream stream, const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev,
                                   int n, const float* cam_dev, int num_cameras, int cam_period, const float* depth_dev, double head_size, int frame,
                                   const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev,
                                   const int32_t* region_image_dev, int m, int region_period, double expand, double camera_cos2, int32_t* kind_dev,
                                   int32_t* target_dev, float* t_dev, float* hit_dev, int32_t* mutual_dev, int32_t* flags_dev, float* hit3d_dev) {
  const char* what = "mcg_gaze_targets_3d";
  MCG_CHECK_ARG(n >= 0 && n <= MCG_ATTEND_ROWS, "%s: 0 .. %d rows per call (got %d)", what, MCG_ATTEND_ROWS, n);
  MCG_CHECK_ARG(m >= 0 && m <= MCG_ATTEND_REGIONS, "%s: 0 .. %d regions per call (got %d)", what, MCG_ATTEND_REGIONS, m);
  MCG_CHECK_ARG(num_vertices >= 0 && num_vertices <= MCG_ATTEND_VERTICES, "%s: 0 .. %d vertices per call (got %d)", what, MCG_ATTEND_VERTICES,
                num_vertices);
  MCG_CHECK_ARG(num_cameras >= 1 && num_cameras <= MCG_ATTEND_CAMERAS, "%s: 1 .. %d cameras per call (got %d)", what, MCG_ATTEND_CAMERAS, num_cameras);
  MCG_CHECK_ARG(gaze_stride >= 3 && region_period >= 0 && cam_period >= 0, "%s: bad sizes gaze_stride=%d region_period=%d cam_period=%d", what,
                gaze_stride, region_period, cam_period);
  MCG_CHECK_ARG(frame == 0 || frame == 1, "%s: frame is 0 (camera) or 1 (eye), got %d", what, frame);
  MCG_CHECK_ARG(expand >= 0.0 && expand - expand == 0.0 && camera_cos2 == camera_cos2 && head_size > 0.0 && head_size - head_size == 0.0,
                "%s: expand must be finite and not negative, camera_cos2 a number, head_size finite and positive", what);
  MCG_CHECK_ARG(cam_dev != nullptr, "%s: null camera table", what);
  MCG_CHECK_ARG(n == 0 || (boxes_dev && gaze_dev && image_of_dev && kind_dev && target_dev && t_dev && hit_dev && mutual_dev && flags_dev && hit3d_dev),
                "%s: null pointer", what);
  MCG_CHECK_ARG(m == 0 || (region_start_dev && region_image_dev), "%s: null region table with m=%d", what, m);
  MCG_CHECK_ARG(num_vertices == 0 || region_xyz_dev, "%s: null vertex table with num_vertices=%d", what, num_vertices);
  if (n == 0) return MCG_OK;
  const dim3 grid((n + MCG_ATTEND_THREADS - 1) / MCG_ATTEND_THREADS), block(MCG_ATTEND_THREADS);
  hipLaunchKernelGGL(gaze_targets_3d_kernel, grid, block, 0, (hipStream_t)stream, boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, cam_dev, num_cameras,
                     cam_period, depth_dev, head_size, frame, region_xyz_dev, num_vertices, region_start_dev, region_image_dev, m, region_period, expand,
                     camera_cos2, kind_dev, target_dev, t_dev, hit_dev, flags_dev, hit3d_dev);
  MCG_CHECK_LAUNCH(what);
  hipLaunchKernelGGL(gaze_mutual_kernel, grid, block, 0, (hipStream_t)stream, kind_dev, target_dev, n, mutual_dev);
  MCG_CHECK_LAUNCH("mcg_gaze_targets_3d (mutual)");
  return MCG_OK;
}
