// Gaze heat maps on the device (include/mcgaze_hip.h, "gaze heat map"): where in the picture looks have landed, accumulated over calls into a
// grid of cells per camera (mcg_gaze_heat_add) and blended, colour-mapped, into packed BGR frames (mcg_draw_heat) or NV12 surfaces
// (mcg_draw_heat_nv12) in place.  Everything behind the first rounding of `hit` is integer arithmetic, stated once, in the header;
// mcgaze_amd/attention.py::gaze_heat_host and mcgaze_amd/arrows.py::draw_heat_host are the same on the host, bit for bit.
//
// Accumulating is three launches: the workspace and `peak` cleared; a SCATTER, one thread per (row, tap row), that adds the taps into the
// workspace with integer vector atomics -- integer sums commute, so the order does not matter --; and a per-cell pass that decays, adds,
// saturates and takes the camera's maximum (an integer atomic max, which commutes too).
//
// heat_render_kernel is the one whole-frame kernel of the project: a block owns a tile of 256 x 16 pixels (NV12: 256 x 32) of one picture,
// brings the cells its pixels interpolate between -- the tile's cells and one cell of apron, edge cells repeated -- and the 256 colours into
// LDS, and every thread then owns 16 pixels of a row (NV12: a 16 x 2 block and its 8 chroma pairs): it works out their levels from LDS,
// leaves if none reaches min_level, and otherwise reads, blends and writes its 48 bytes (NV12: 16 + 16 + 16) in 16-byte accesses where the
// plane's address and pitch allow, in 4-byte accesses where only those are aligned, byte by byte at the right edge and for any other
// pitch.  A tile whose cells are all zero leaves before any pixel is read.  No atomics, no scratch.
#include "heat_common.hpp"   // the clear and update launches, the blend, a thread's span of pixels (shared with surface.hip)

#define MCG_HEAT_TILE_W (16 * MCG_HEAT_SPAN) // 16 threads side by side
#define MCG_HEAT_LDS_W (MCG_HEAT_TILE_W + 2) // cell_shift 0: the tile's 256 columns and the one to their right; one spare

// ---------------------------------------------------------------- accumulate (heat_clear_kernel and heat_update_kernel: heat_common.hpp)
__global__ __launch_bounds__(256) void heat_scatter_kernel(const float* __restrict__ hit, const int32_t* __restrict__ kind,
                                                           const int32_t* __restrict__ image_of, const int32_t* __restrict__ flags,
                                                           const int32_t* __restrict__ mask, int n, int32_t* __restrict__ work, int C, int GH, int GW,
                                                           int cell_shift, int radius, int kinds, int period) {
  const int T = 2 * radius + 1;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int k = t / T;
  if (k >= n) return;
  const int dy = t - k * T - radius;
  // THE ROW RULE, in the header's order
  if (flags && flags[k] != 0) return;
  if (mask && mask[k] == 0) return;
  const int kd = kind[k];
  if (kd < 0 || kd > 3 || !((kinds >> kd) & 1)) return;
  const int io = image_of[k];
  if (io < 0) return;
  const int c = period == 0 ? io : io % period;
  if (c >= C) return;
  const double hx = rint((double)hit[2 * k]), hy = rint((double)hit[2 * k + 1]), lim = (double)MCG_DRAW_COORD;   // half to even; a NaN fails the test
  if (!(fabs(hx) <= lim && fabs(hy) <= lim)) return;
  const int ix = (int)hx >> cell_shift, iy = (int)hy >> cell_shift;     // arithmetic shifts: floors
  const int y = iy + dy;
  if (y < 0 || y >= GH) return;
  const int wy = radius + 1 - abs(dy);
  int32_t* row = work + ((size_t)c * GH + y) * GW;
  for (int dx = -radius; dx <= radius; ++dx) {
    const int x = ix + dx;
    if (x >= 0 && x < GW) atomicAdd(row + x, wy * (radius + 1 - abs(dx)));   // at most 65536 rows of 81: the sum stays below 2^23
  }
}

static int heat_grid_ok(const char* what, int C, int GH, int GW, int cell_shift, int period) {
  MCG_CHECK_ARG(C >= 1 && C <= 4096 && GH >= 1 && GH <= 8192 && GW >= 1 && GW <= 8192, "%s: 1 .. 4096 cameras of 1 .. 8192 cells a side (got %d x %d x %d)",
                what, C, GH, GW);
  MCG_CHECK_ARG((long long)C * GH * GW <= MCG_HEAT_MAX_CELLS, "%s: at most 2^24 cells (got %d x %d x %d)", what, C, GH, GW);
  MCG_CHECK_ARG(cell_shift >= 0 && cell_shift <= 6 && period >= 0, "%s: cell_shift in 0 .. 6 and period >= 0 (got %d, %d)", what, cell_shift, period);
  return MCG_OK;
}

extern "C" int mcg_gaze_heat_add(mcg_stream s, const float* hit_dev, const int32_t* kind_dev, const int32_t* image_of_dev, const int32_t* flags_dev,
                                 const int32_t* mask_dev, int n, int32_t* heat_dev, int32_t* peak_dev, int C, int GH, int GW, int cell_shift, int radius,
                                 int kinds, int period, int decay_shift, void* workspace_dev, size_t workspace_bytes) {
  MCG_CHECK_ARG(n >= 0 && n <= 65536, "mcg_gaze_heat_add: at most 65536 rows per call (got %d)", n);
  MCG_CHECK_ARG(heat_dev && peak_dev && workspace_dev && (n == 0 || (hit_dev && kind_dev && image_of_dev)), "mcg_gaze_heat_add: null pointer");
  MCG_TRY(heat_grid_ok("mcg_gaze_heat_add", C, GH, GW, cell_shift, period));
  MCG_CHECK_ARG(radius >= 0 && radius <= 8 && decay_shift >= 0 && decay_shift <= 30, "mcg_gaze_heat_add: radius in 0 .. 8, decay_shift in 0 .. 30 (got %d, %d)",
                radius, decay_shift);
  const int cells = GH * GW, all = C * cells;
  MCG_CHECK_ARG(workspace_bytes >= 4 * (size_t)all, "mcg_gaze_heat_add: the workspace holds %zu bytes, %zu are needed", workspace_bytes, 4 * (size_t)all);
  int32_t* work = (int32_t*)workspace_dev;
  hipLaunchKernelGGL(heat_clear_kernel, dim3((max(all, C) + 255) / 256), dim3(256), 0, (hipStream_t)s, work, all, peak_dev, C);
  MCG_CHECK_LAUNCH("mcg_gaze_heat_add (clear)");
  // n == 0: one block whose threads all leave -- the number of launches does not depend on the tables' sizes
  hipLaunchKernelGGL(heat_scatter_kernel, dim3((max(n, 1) * (2 * radius + 1) + 255) / 256), dim3(256), 0, (hipStream_t)s, hit_dev, kind_dev, image_of_dev,
                     flags_dev, mask_dev, n, work, C, GH, GW, cell_shift, radius, kinds, period);
  MCG_CHECK_LAUNCH("mcg_gaze_heat_add (scatter)");
  hipLaunchKernelGGL(heat_update_kernel, dim3((cells + 255) / 256, C), dim3(256), 0, (hipStream_t)s, heat_dev, work, peak_dev, cells, decay_shift);
  MCG_CHECK_LAUNCH("mcg_gaze_heat_add");
  return MCG_OK;
}

// ---------------------------------------------------------------- render
template <class Target>
__global__ __launch_bounds__(256) void heat_render_kernel(const typename Target::Image* __restrict__ images, int tiles_x, int max_h, int max_w,
                                                          const int32_t* __restrict__ heat, const int32_t* __restrict__ full_dev, int C, int GH, int GW,
                                                          int cell_shift, int period, const unsigned* __restrict__ lut, int min_level) {
  constexpr int R = Target::CELL;                                 // pixel rows of a thread: 1, NV12 2
  constexpr int TILE_H = 16 * R, LDS_H = TILE_H + 2;
  __shared__ int cell[LDS_H][MCG_HEAT_LDS_W];
  __shared__ unsigned colour[256];
  const int img = blockIdx.y;
  const int cam = period == 0 ? img : img % period;
  if (cam >= C) return;
  const typename Target::Image im = images[img];
  if (!Target::writable(im) || im.h > max_h || im.w > max_w) return;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int tx0 = tile_x * MCG_HEAT_TILE_W, ty0 = tile_y * TILE_H;
  if (tx0 >= im.w || ty0 >= im.h) return;                         // block-uniform, like every return above: nobody waits at the barrier
  const int S = 1 << cell_shift, S2 = 2 * S, sh = cell_shift + 1;
  // the first cell the tile's pixels interpolate from; the last one is at most 256 / S + 1 columns (16 R / S + 1 rows) further
  const int cx0 = (2 * tx0 + 1 - S) >> sh, cy0 = (2 * ty0 + 1 - S) >> sh;
  const int ncx = ((2 * (tx0 + MCG_HEAT_TILE_W - 1) + 1 - S) >> sh) + 2 - cx0, ncy = ((2 * (ty0 + TILE_H - 1) + 1 - S) >> sh) + 2 - cy0;
  const int32_t* grid = heat + (size_t)cam * GH * GW;
  int any = 0;
  for (int i = threadIdx.x; i < ncx * ncy; i += 256) {
    const int ly = i / ncx, lx = i - ly * ncx;
    const int gy = min(max(cy0 + ly, 0), GH - 1), gx = min(max(cx0 + lx, 0), GW - 1);   // a grid smaller than the picture repeats its edge cells
    const int h = max(grid[(size_t)gy * GW + gx], 0);
    cell[ly][lx] = h;
    any |= h;
  }
  colour[threadIdx.x] = lut[threadIdx.x];
  if (!__syncthreads_or(any)) return;                             // nothing but zeros under this tile: every level is 0 < min_level

  const int px0 = tx0 + (threadIdx.x & 15) * MCG_HEAT_SPAN, py0 = ty0 + (threadIdx.x >> 4) * R;
  if (px0 >= im.w || py0 >= im.h) return;
  const long long full = max(full_dev[cam], 1);
  int level[R][MCG_HEAT_SPAN];
  int most = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int uy = 2 * (py0 + r) + 1 - S, iy = uy >> sh, fy = uy - iy * S2, ly = iy - cy0;      // (iy, ix may be -1: a product, not a shift of a negative int)
#pragma unroll
    for (int j = 0; j < MCG_HEAT_SPAN; ++j) {
      const int ux = 2 * (px0 + j) + 1 - S, ix = ux >> sh, fx = ux - ix * S2, lx = ix - cx0;
      const long long h00 = cell[ly][lx], h01 = cell[ly][lx + 1], h10 = cell[ly + 1][lx], h11 = cell[ly + 1][lx + 1];
      const long long v = (long long)((S2 - fx) * (S2 - fy)) * h00 + (long long)(fx * (S2 - fy)) * h01 + (long long)((S2 - fx) * fy) * h10 +
                          (long long)(fx * fy) * h11;                                   // below 2^45
      // L = min(255, floor(v 255 / (4 S S full))): 4 S S is a power of two, and the quotient by full is found bit by bit -- eight
      // multiplications in place of a 64-bit division
      const int L = heat_level((v * 255) >> (2 * cell_shift + 2), full);
      level[r][j] = L;
      most = max(most, L);
    }
  }
  if (most < min_level) return;                                   // none of this thread's pixels is written: none is read either

  heat_blend_span<Target>(im, px0, py0, level, colour, min_level);
}

template <class Target>
static int draw_heat(const char* what, mcg_stream stream, const typename Target::Image* images_dev, int num_images, int max_h, int max_w,
                     const int32_t* heat_dev, const int32_t* full_dev, int C, int GH, int GW, int cell_shift, int period, const unsigned char* lut_dev,
                     int min_level) {
  MCG_CHECK_ARG(images_dev && heat_dev && full_dev && lut_dev, "%s: null pointer", what);
  MCG_CHECK_ARG(num_images >= 1 && num_images <= 65535, "%s: 1 .. 65535 images (got %d)", what, num_images);
  MCG_CHECK_ARG(max_h >= 1 && max_h <= MCG_DRAW_SIDE && max_w >= 1 && max_w <= MCG_DRAW_SIDE, "%s: frames of 1 .. 8192 pixels a side (got max %dx%d)",
                what, max_h, max_w);
  MCG_TRY(heat_grid_ok(what, C, GH, GW, cell_shift, period));
  MCG_CHECK_ARG(min_level >= 1 && min_level <= 255, "%s: min_level in 1 .. 255 (got %d)", what, min_level);
  MCG_CHECK_ARG(((uintptr_t)lut_dev & 3) == 0, "%s: the colour table must be aligned to 4 bytes", what);
  constexpr int TILE_H = 16 * Target::CELL;
  const int tiles_x = (max_w + MCG_HEAT_TILE_W - 1) / MCG_HEAT_TILE_W, tiles_y = (max_h + TILE_H - 1) / TILE_H;
  hipLaunchKernelGGL(heat_render_kernel<Target>, dim3(tiles_x * tiles_y, num_images), dim3(256), 0, (hipStream_t)stream, images_dev, tiles_x, max_h,
                     max_w, heat_dev, full_dev, C, GH, GW, cell_shift, period, (const unsigned*)lut_dev, min_level);
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

extern "C" int mcg_draw_heat(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const int32_t* heat_dev,
                             const int32_t* full_dev, int C, int GH, int GW, int cell_shift, int period, const unsigned char* lut_dev, int min_level) {
  return draw_heat<PackedTarget>("mcg_draw_heat", s, images_dev, num_images, max_h, max_w, heat_dev, full_dev, C, GH, GW, cell_shift, period, lut_dev,
                                 min_level);
}

extern "C" int mcg_draw_heat_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const int32_t* heat_dev,
                                  const int32_t* full_dev, int C, int GH, int GW, int cell_shift, int period, const unsigned char* lut_dev,
                                  int min_level) {
  return draw_heat<Nv12Target>("mcg_draw_heat_nv12", s, images_dev, num_images, max_h, max_w, heat_dev, full_dev, C, GH, GW, cell_shift, period, lut_dev,
                               min_level);
}
