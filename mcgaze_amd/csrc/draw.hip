// Gaze arrows drawn on the device (MCGaze_demo/demo.ipynb, cell 5): head boxes and gaze vectors, both in device memory, become arrows in
// the frames they belong to -- packed BGR frames (mcg_draw_gaze_arrows) or a video decoder's NV12 surfaces (mcg_draw_gaze_arrows_nv12),
// written in place, so that "decoder surface in, annotated surface out to the encoder" never touches the host.  The arithmetic is stated
// once, in include/mcgaze_hip.h ("Annotated frames out") and DESIGN.md; mcgaze_amd/pipeline.py::draw_arrows_host is the same on the host.
//
// Two launches.  arrow_plan_kernel: one thread per row, in double and uncontracted like head_crop_plan_kernel, writes a mcg_arrow_desc --
// the three segments (shaft and the two head strokes, OpenCV's published arrowedLine rule restated without atan2 / cos / sin; not linked,
// and parity with cv2's own rasteriser is not claimed), the thickness, the bounding box clipped to the frame, the flag.
// arrow_raster_kernel is a GATHER: the grid runs over (image, pixel tile); each wave owns a strip of its tile, scans the rows 64 at a
// time (lane i tests row base + i against the strip: image, flag, bounding box), and walks the hits in ASCENDING row order, every lane
// testing its own pixels against the three capsules in 64-bit integers.  A lane remembers the LAST row that covered a pixel and stores
// once, after the walk: the highest row wins whatever the launch geometry or the scheduling, no two threads ever write the same byte, and
// only covered pixels are stored (vector byte stores; no LDS, no atomics).  For NV12 a thread owns one 2 x 2 luma block and with it the one
// chroma pair those four pixels share: the pair is written iff any of the four is covered, with the colour of the highest such row.
// Cost: every wave reads n / 64 slices of the plan whatever it draws -- made for the tens of heads of a video frame, not for 65535 rows on
// large frames.
#include "draw_common.hpp"   // the bounds, the tile, PackedTarget / Nv12Target and capsule(): shared with overlay.hip

template <class Target>
__global__ __launch_bounds__(256) void arrow_plan_kernel(const typename Target::Image* __restrict__ images, int num_images, int max_h, int max_w,
                                                         const float* __restrict__ boxes, const float* __restrict__ gaze, int gaze_stride,
                                                         const int32_t* __restrict__ image_of, int n, double length, double min_thickness,
                                                         double thickness_ratio, double tip_length, mcg_arrow_desc* __restrict__ plan,
                                                         int32_t* __restrict__ flags) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const mcg_arrow_desc d = arrow_plan_row<Target>(images, num_images, max_h, max_w, boxes, gaze, gaze_stride, image_of, k, length, min_thickness,
                                                  thickness_ratio, tip_length);
  plan[k] = d;
  if (flags) flags[k] = d.flag;
}

template <class Target>
__global__ __launch_bounds__(MCG_DRAW_THREADS) void arrow_raster_kernel(const typename Target::Image* __restrict__ images, int tiles_x,
                                                                        const mcg_arrow_desc* __restrict__ plan, int n, unsigned c0, unsigned c1,
                                                                        unsigned c2, const unsigned char* __restrict__ colors) {
  constexpr int S = Target::CELL;
  const int img = blockIdx.y;
  const typename Target::Image im = images[img];
  if (!Target::writable(im) || im.h > MCG_DRAW_SIDE || im.w > MCG_DRAW_SIDE) return;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the strip of this wave, in pixels: [sx0, sx1) x [sy0, sy1)
  const int sx0 = tile_x * MCG_DRAW_TILE_W * S, sy0 = (tile_y * MCG_DRAW_TILE_H + 2 * wave) * S;
  const int sx1 = sx0 + MCG_DRAW_TILE_W * S, sy1 = sy0 + 2 * S;
  if (sx0 >= im.w || sy0 >= im.h) return;                       // wave-uniform: the whole strip lies outside this image
  const int px0 = sx0 + (lane & 31) * S, py0 = sy0 + (lane >> 5) * S;   // this lane's cell
  int win[S * S];
#pragma unroll
  for (int i = 0; i < S * S; ++i) win[i] = -1;
  for (int base = 0; base < n; base += 64) {
    const int r = base + lane;
    bool hit = false;
    if (r < n) {
      const mcg_arrow_desc* d = plan + r;
      hit = d->flag == 0 && d->image == img && d->x0 < sx1 && d->x1 > sx0 && d->y0 < sy1 && d->y1 > sy0;
    }
    unsigned long long mask = __ballot(hit);
    while (mask) {                                              // ascending rows: a later row overwrites an earlier one
      const int j = base + __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const mcg_arrow_desc d = plan[j];                         // one address for the wave
      const long long tt = (long long)d.thickness * d.thickness;
#pragma unroll
      for (int i = 0; i < S * S; ++i) {
        const int px = px0 + (i % S), py = py0 + (i / S);
        // the box is clipped to the frame: a covered pixel has px < w and py < h
        int in = (int)(px >= d.x0) & (int)(px < d.x1) & (int)(py >= d.y0) & (int)(py < d.y1);
        int any = 0;
#pragma unroll
        for (int g = 0; g < 3; ++g) any |= capsule(px, py, d.seg[g][0][0], d.seg[g][0][1], d.seg[g][1][0], d.seg[g][1][1], tt);
        win[i] = (in & any) ? j : win[i];
      }
    }
  }
  int top = -1;
#pragma unroll
  for (int i = 0; i < S * S; ++i) top = max(top, win[i]);
  if (top < 0) return;
  if constexpr (S == 1) {
    // (a covered pixel lies inside its row's clipped box, hence inside the frame)
    unsigned char* q = (unsigned char*)im.src + (size_t)py0 * im.pitch + (size_t)px0 * 3;
    if (colors) { c0 = colors[3 * top]; c1 = colors[3 * top + 1]; c2 = colors[3 * top + 2]; }
    q[0] = (unsigned char)c0; q[1] = (unsigned char)c1; q[2] = (unsigned char)c2;
  } else {
#pragma unroll
    for (int i = 0; i < S * S; ++i)
      if (win[i] >= 0) ((unsigned char*)im.y)[(size_t)(py0 + i / S) * im.pitch_y + px0 + (i % S)] = colors ? colors[3 * win[i]] : (unsigned char)c0;
    // px0, py0 even, and some pixel of the block is inside the frame, so (py0, px0) is: py0 >> 1 <= h / 2 - 1, px0 + 1 <= w - 1
    unsigned char* c = (unsigned char*)im.uv + (size_t)(py0 >> 1) * im.pitch_uv + px0;
    c[0] = colors ? colors[3 * top + 1] : (unsigned char)c1;
    c[1] = colors ? colors[3 * top + 2] : (unsigned char)c2;
  }
}

template <class Target>
static int draw_gaze_arrows(const char* what, const char* what_plan, mcg_stream stream, const typename Target::Image* images_dev, int num_images,
                            int max_h, int max_w, const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev,
                            int n, double length, int min_thickness, double thickness_ratio, double tip_length, const unsigned char* color,
                            const unsigned char* colors_dev, mcg_arrow_desc* plan_out_dev, int32_t* flags_dev) {
  MCG_CHECK_ARG(images_dev && boxes_dev && gaze_dev && image_of_dev && plan_out_dev && (color || colors_dev), "%s: null pointer", what);
  MCG_CHECK_ARG(n >= 0 && num_images >= 1 && num_images <= 65535 && gaze_stride >= 2, "%s: bad sizes n=%d images=%d gaze_stride=%d", what, n,
                num_images, gaze_stride);
  MCG_CHECK_ARG(n <= 65535, "%s: at most 65535 rows per call (got %d)", what, n);
  MCG_CHECK_ARG(max_h >= 1 && max_h <= MCG_DRAW_SIDE && max_w >= 1 && max_w <= MCG_DRAW_SIDE, "%s: frames of 1 .. 8192 pixels a side (got max %dx%d)",
                what, max_h, max_w);
  MCG_CHECK_ARG(min_thickness >= 1 && min_thickness <= 255, "%s: min_thickness in 1 .. 255 (got %d)", what, min_thickness);
  MCG_CHECK_ARG(length - length == 0.0 && thickness_ratio - thickness_ratio == 0.0 && tip_length - tip_length == 0.0,
                "%s: length, thickness_ratio and tip_length must be finite", what);
  if (n == 0) return MCG_OK;
  hipLaunchKernelGGL(arrow_plan_kernel<Target>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, images_dev, num_images, max_h, max_w,
                     boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, length, (double)min_thickness, thickness_ratio, tip_length, plan_out_dev,
                     flags_dev);
  MCG_CHECK_LAUNCH(what_plan);
  constexpr int S = Target::CELL;
  const int tiles_x = (max_w + MCG_DRAW_TILE_W * S - 1) / (MCG_DRAW_TILE_W * S), tiles_y = (max_h + MCG_DRAW_TILE_H * S - 1) / (MCG_DRAW_TILE_H * S);
  const unsigned c0 = color ? color[0] : 0, c1 = color ? color[1] : 0, c2 = color ? color[2] : 0;
  hipLaunchKernelGGL(arrow_raster_kernel<Target>, dim3(tiles_x * tiles_y, num_images), dim3(MCG_DRAW_THREADS), 0, (hipStream_t)stream, images_dev,
                     tiles_x, plan_out_dev, n, c0, c1, c2, colors_dev);
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

extern "C" int mcg_draw_gaze_arrows(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                                    const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n, double length, int min_thickness,
                                    double thickness_ratio, double tip_length, const unsigned char* color, const unsigned char* colors_dev,
                                    mcg_arrow_desc* plan_out_dev, int32_t* flags_dev) {
  return draw_gaze_arrows<PackedTarget>("mcg_draw_gaze_arrows", "mcg_draw_gaze_arrows (plan)", s, images_dev, num_images, max_h, max_w, boxes_dev,
                                        gaze_dev, gaze_stride, image_of_dev, n, length, min_thickness, thickness_ratio, tip_length, color, colors_dev,
                                        plan_out_dev, flags_dev);
}

extern "C" int mcg_draw_gaze_arrows_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w,
                                         const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n,
                                         double length, int min_thickness, double thickness_ratio, double tip_length, const unsigned char* yuv,
                                         const unsigned char* yuvs_dev, mcg_arrow_desc* plan_out_dev, int32_t* flags_dev) {
  return draw_gaze_arrows<Nv12Target>("mcg_draw_gaze_arrows_nv12", "mcg_draw_gaze_arrows_nv12 (plan)", s, images_dev, num_images, max_h, max_w,
                                      boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, length, min_thickness, thickness_ratio, tip_length, yuv,
                                      yuvs_dev, plan_out_dev, flags_dev);
}
