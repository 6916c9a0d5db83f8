// Test-time frame preprocessing on the device: one launch turns a batch of decoded uint8 BGR frames
// into the model's input tensor.  Fuses, per frame, what the reference does on the CPU one frame and one transform at a time:
//   CenterCrop window        mmdet/datasets/pipelines/transforms.py:1036-1052 (window chosen by the host: mcgaze_amd/pipeline.py)
//   Resize(keep_ratio=True)  transforms.py:216-242 -> mmcv.imrescale -> cv2.resize(INTER_LINEAR), 8-bit fixed-point bilinear
//   Normalize(to_rgb=True)   transforms.py:739-755 -> mmcv.imnormalize: (float(rgb) - mean) * (1 / std) in float32
//   Pad(size_divisor=32) + collate of the clip: zeros to the right / below (transforms.py:665-683)
//   DefaultFormatBundle      formatting.py:229-231: HWC -> CHW
// The resize arithmetic is OpenCV's published INTER_LINEAR path for 8-bit images, restated (not linked): source coordinate
// (d + 0.5) * (src / dst) - 0.5 in double, cast to float, floor + fraction, clamped to the image with zero fraction at the
// borders; coefficients rounded to 11-bit fixed point (round half to even); horizontal pass in 32-bit integers; vertical pass
// uchar((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2).  Integer work is bit-exact against
// oracle/preprocess_oracle.py by construction; floating-point contraction is disabled so the float steps are too.
// Memory-bound and tiny (a 64-clip batch reads <= 0.3 GB of pixels and writes 270 MB): one thread per output pixel, channel
// planes written coalesced.
//
// Head crops (mcg_preprocess_head_crops): the WINDOW is chosen on the device too.  head_crop_plan_kernel restates, one thread per crop, what
// the reference's demo does per person and frame on the host (MCGaze_demo/demo.ipynb, cell 4: head centre, half side, the numpy slice
// that clips at the frame border) and mmcv's rescale_size behind Resize(keep_ratio=True) (transforms.py:216-242), and writes the
// mcg_frame_desc rows preprocess_kernel reads -- so video frames and a detector's head boxes, both already in device memory, become the
// model's input without a word going to the host.
#include "common.hpp"

struct LinCoef {
  int s0, s1, a0, a1;
};

__device__ __forceinline__ LinCoef lin_coef(int d, int dst, int src) {
#pragma clang fp contract(off)
  const double scale = 1.0 / ((double)dst / (double)src);
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= src - 1) { f = 0.f; s = src - 1; }
  LinCoef c;
  c.s0 = s;
  c.s1 = min(s + 1, src - 1);
  c.a1 = __float2int_rn(f * 2048.f);
  c.a0 = __float2int_rn((1.f - f) * 2048.f);
  return c;
}

__global__ __launch_bounds__(256) void preprocess_kernel(const mcg_frame_desc* __restrict__ frames, float* __restrict__ dst, int pad_h,
                                                         int pad_w, float m0, float m1, float m2, float s0, float s1, float s2, int to_rgb) {
#pragma clang fp contract(off)
  const mcg_frame_desc fd = frames[blockIdx.y];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= pad_h * pad_w) return;
  const int y = idx / pad_w, x = idx - y * pad_w;
  float* out = dst + (size_t)blockIdx.y * 3 * pad_h * pad_w + idx;
  const size_t plane = (size_t)pad_h * pad_w;
  if (y >= fd.out_h || x >= fd.out_w) {
    out[0] = 0.f; out[plane] = 0.f; out[2 * plane] = 0.f;
    return;
  }
  const LinCoef cx = lin_coef(x, fd.out_w, fd.crop_w), cy = lin_coef(y, fd.out_h, fd.crop_h);
  const unsigned char* base = (const unsigned char*)fd.src + (size_t)fd.crop_y * fd.src_pitch + (size_t)fd.crop_x * 3;
  const unsigned char* r0 = base + (size_t)cy.s0 * fd.src_pitch;
  const unsigned char* r1 = base + (size_t)cy.s1 * fd.src_pitch;
  int v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = (int)r0[cx.s0 * 3 + c] * cx.a0 + (int)r0[cx.s1 * 3 + c] * cx.a1;
    const int h1 = (int)r1[cx.s0 * 3 + c] * cx.a0 + (int)r1[cx.s1 * 3 + c] * cx.a1;
    v[c] = (((cy.a0 * (h0 >> 4)) >> 16) + ((cy.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
  }
  const int c0 = to_rgb ? 2 : 0, c2 = to_rgb ? 0 : 2;  // source is BGR
  out[0] = ((float)v[c0] - m0) * s0;
  out[plane] = ((float)v[1] - m1) * s1;
  out[2 * plane] = ((float)v[c2] - m2) * s2;
}

extern "C" int mcg_preprocess_frames(mcg_stream stream, const mcg_frame_desc* frames_dev, int num_frames, float* dst, int pad_h, int pad_w,
                                     const float mean[3], const float stdinv[3], int to_rgb) {
  MCG_CHECK_ARG(frames_dev && dst && mean && stdinv, "mcg_preprocess_frames: null pointer");
  MCG_CHECK_ARG(num_frames >= 0 && pad_h > 0 && pad_w > 0, "mcg_preprocess_frames: bad sizes n=%d pad=%dx%d", num_frames, pad_h, pad_w);
  MCG_CHECK_ARG(num_frames <= 65535, "mcg_preprocess_frames: at most 65535 frames per call (got %d)", num_frames);
  if (num_frames == 0) return MCG_OK;
  dim3 grid((pad_h * pad_w + 255) / 256, num_frames);
  hipLaunchKernelGGL(preprocess_kernel, grid, dim3(256), 0, (hipStream_t)stream, frames_dev, dst, pad_h, pad_w, mean[0], mean[1], mean[2],
                     stdinv[0], stdinv[1], stdinv[2], to_rgb);
  MCG_CHECK_LAUNCH("mcg_preprocess_frames");
  return MCG_OK;
}

// MCGaze_demo/demo.ipynb, cell 4, per (person, frame) -- in double, uncontracted: python floats, and int(w * f + 0.5) must not fuse.
//   head_center = [int(y1 + y2) // 2, int(x1 + x2) // 2];  l = int(max(y2 - y1, x2 - x1) * 0.8)
//   head_crop = img[max(0, cy - l):min(cy + l, rows), max(0, cx - l):min(cx + l, cols)]
// Every bound is clamped to the frame while still a double, so no box, however large, overflows an int; what the slice would leave empty
// becomes ONE pixel inside the frame (flag 1), and a row whose box or image index cannot be used reads pixel (0, 0) of image 0 (flag 2).
struct Span {
  int lo, len;
  bool empty;
};

__device__ __forceinline__ Span head_span(double a, double b, double l, int size) {
#pragma clang fp contract(off)
  const double c = floor(trunc(a + b) / 2.0);             // int(a + b) // 2: truncate, then floor-divide (they differ below zero)
  const double lo = fmax(0.0, c - l), hi = fmin(c + l, (double)size);
  Span s;
  s.empty = !(hi > lo);
  s.lo = (int)fmin(lo, (double)(size - 1));               // 0 <= lo; the clamp only acts on an empty span
  s.len = s.empty ? 1 : (int)hi - s.lo;
  return s;
}

__global__ __launch_bounds__(256) void head_crop_plan_kernel(const mcg_image_desc* __restrict__ images, int num_images,
                                                             const float* __restrict__ boxes, const int32_t* __restrict__ image_of, int n,
                                                             double expand, int scale_long, int scale_short, int pad_h, int pad_w,
                                                             mcg_frame_desc* __restrict__ desc, int32_t* __restrict__ img_hw,
                                                             float* __restrict__ scale_factor, int32_t* __restrict__ flags) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double x1 = boxes[4 * k], y1 = boxes[4 * k + 1], x2 = boxes[4 * k + 2], y2 = boxes[4 * k + 3];   // f32 -> double: exact
  const int io = image_of[k];
  bool usable = io >= 0 && io < num_images && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
  mcg_image_desc im = images[usable ? io : 0];
  if (usable && (im.h <= 0 || im.w <= 0)) {               // an image row with no pixels names nothing to read either
    usable = false;
    im = images[0];
  }
  int flag = usable ? 0 : 2;
  Span ys = {0, 1, false}, xs = {0, 1, false};
  if (usable) {
    const double l = trunc(fmax(y2 - y1, x2 - x1) * expand);
    ys = head_span(y1, y2, l, im.h);
    xs = head_span(x1, x2, l, im.w);
    if (ys.empty || xs.empty) {                           // the demo's slice is empty as soon as one axis is: one pixel, inside the frame
      ys.len = xs.len = 1;
      flag = 1;
    }
  }
  // mmcv rescale_size: f = min(long / max(h, w), short / min(h, w)); new = int(side * f + 0.5)
  const int h = ys.len, w = xs.len;
  const double f = fmin((double)scale_long / (double)max(h, w), (double)scale_short / (double)min(h, w));
  // at least one pixel (a 1 x 1000 sliver would round to zero columns, which cv2.resize refuses), at most the padded frame
  const int new_w = min(max((int)((double)w * f + 0.5), 1), pad_w), new_h = min(max((int)((double)h * f + 0.5), 1), pad_h);
  mcg_frame_desc d;
  d.src = im.src;
  d.src_h = im.h; d.src_w = im.w; d.src_pitch = im.pitch;
  d.crop_y = ys.lo; d.crop_x = xs.lo; d.crop_h = h; d.crop_w = w;
  d.out_h = new_h; d.out_w = new_w;
  desc[k] = d;
  img_hw[2 * k] = new_h;
  img_hw[2 * k + 1] = new_w;
  const float fw = (float)((double)new_w / (double)w), fh = (float)((double)new_h / (double)h);
  scale_factor[4 * k] = fw; scale_factor[4 * k + 1] = fh; scale_factor[4 * k + 2] = fw; scale_factor[4 * k + 3] = fh;
  if (flags) flags[k] = flag;
}

extern "C" int mcg_preprocess_head_crops(mcg_stream stream, const mcg_image_desc* images_dev, int num_images, const float* boxes_dev,
                                         const int32_t* image_of_dev, int n, double expand, int scale_w, int scale_h,
                                         mcg_frame_desc* desc_out_dev, int32_t* img_hw_dev, float* scale_factor_dev, int32_t* flags_dev,
                                         float* dst, int pad_h, int pad_w, const float mean[3], const float stdinv[3], int to_rgb) {
  MCG_CHECK_ARG(images_dev && boxes_dev && image_of_dev && desc_out_dev && img_hw_dev && scale_factor_dev && dst && mean && stdinv,
                "mcg_preprocess_head_crops: null pointer");
  MCG_CHECK_ARG(n >= 0 && num_images >= 1 && scale_w > 0 && scale_h > 0, "mcg_preprocess_head_crops: bad sizes n=%d images=%d scale=%dx%d", n,
                num_images, scale_w, scale_h);
  MCG_CHECK_ARG(n <= 65535, "mcg_preprocess_head_crops: at most 65535 crops per call (got %d)", n);
  MCG_CHECK_ARG(expand == expand && expand - expand == 0.0, "mcg_preprocess_head_crops: expand must be finite");
  // keep_ratio puts the LONG edge of img_scale on the window's long side, whichever that is: a non-square scale needs room for it both ways
  const int need_h = scale_w == scale_h ? scale_h : max(scale_w, scale_h), need_w = scale_w == scale_h ? scale_w : max(scale_w, scale_h);
  MCG_CHECK_ARG(pad_h >= need_h && pad_w >= need_w, "mcg_preprocess_head_crops: pad %dx%d cannot hold img_scale (%d, %d)", pad_h, pad_w, scale_w,
                scale_h);
  if (n == 0) return MCG_OK;
  hipLaunchKernelGGL(head_crop_plan_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, images_dev, num_images, boxes_dev,
                     image_of_dev, n, expand, max(scale_w, scale_h), min(scale_w, scale_h), pad_h, pad_w, desc_out_dev, img_hw_dev,
                     scale_factor_dev, flags_dev);
  MCG_CHECK_LAUNCH("mcg_preprocess_head_crops (plan)");
  return mcg_preprocess_frames(stream, desc_out_dev, n, dst, pad_h, pad_w, mean, stdinv, to_rgb);
}
