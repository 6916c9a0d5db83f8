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
//
// Both kernels are templates over the pixel SOURCE: packed 8-bit BGR (the entries above), or a video decoder's NV12 surface
// (mcg_preprocess_frames_nv12, mcg_preprocess_head_crops_nv12), whose four taps are converted to BGR where they are read -- the frame is
// never converted whole.
//
// The detector's input (mcg_letterbox_frames, mcg_letterbox_frames_nv12; at the end of this file): the same taps and the same resize, placed
// inside a border of 114 and written as bytes, or as byte / 255 in float or half -- what the demo's head detector reads.
#include <hip/hip_fp16.h>

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

// Where the pixels come from.  A source names its descriptor types, reads ONE tap -- source pixel (sy, sx) of the crop window -- as three
// uint8 values in cv2's order (B, G, R), and tells the plan kernel which image rows it can read and how to point a descriptor at one.
// Everything after the taps (the two fixed-point passes, the normalisation, the channel swap) is the same code for every source.
struct PackedSource {                                       // 3 interleaved 8-bit channels
  using Frame = mcg_frame_desc;
  using Image = mcg_image_desc;
  using Letterbox = mcg_letterbox_desc;
  struct Window {
    const unsigned char* base;
    size_t pitch;
  };
  __device__ __forceinline__ Window window(const Frame& fd) const {
    return {(const unsigned char*)fd.src + (size_t)fd.crop_y * fd.src_pitch + (size_t)fd.crop_x * 3, (size_t)fd.src_pitch};
  }
  __device__ __forceinline__ void tap(const Window& w, int sy, int sx, int p[3]) const {
    const unsigned char* q = w.base + (size_t)sy * w.pitch + sx * 3;
    p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
  }
  static __device__ __forceinline__ bool readable(const Image& im) { return im.h > 0 && im.w > 0; }
  static __device__ __forceinline__ void point(Frame& d, const Image& im) {
    d.src = im.src;
    d.src_pitch = im.pitch;
  }
};

// NV12: a Y plane and a half-resolution plane of interleaved (U, V) pairs.  The tap is converted where it is read, in 32-bit integers:
// OpenCV's published COLOR_YUV2BGR_NV12 arithmetic restated (not linked; parity with cv2 is not pinned on any machine this was built on)
//   yy = max(0, Y - y_off) * cy;  R = sat8((yy + cvr * v + 2^19) >> 20), G = sat8((yy + cvg * v + cug * u + 2^19) >> 20), B = sat8((yy + cub * u + 2^19) >> 20)
// with u = U - 128, v = V - 128 and chroma taken from the NEAREST sample, UV[y >> 1][2 * (x >> 1)] -- (y, x) in FRAME coordinates, so an odd
// crop origin lands on the right chroma phase.  Largest intermediate, BT.601: 239 * 1220542 + 127 * 2116026 + 2^19 = 560,969,128; BT.709:
// 239 * 1220945 + 127 * 2215014 + 2^19 = 573,636,921; most negative -128 * 2215014 = -283,521,792: all far inside an int (the entry refuses
// coefficients for which they could leave it).  h and w even and the window inside the frame: y >> 1 <= h / 2 - 1 and 2 * (x >> 1) + 1 <= w - 1.
struct Nv12Source {
  using Frame = mcg_nv12_frame_desc;
  using Image = mcg_nv12_image_desc;
  using Letterbox = mcg_nv12_letterbox_desc;
  mcg_yuv_coef k;
  struct Window {
    const unsigned char *y, *uv;
    size_t pitch_y, pitch_uv;
    int y0, x0;
  };
  __device__ __forceinline__ Window window(const Frame& fd) const {
    return {(const unsigned char*)fd.src, (const unsigned char*)fd.uv, (size_t)fd.src_pitch, (size_t)fd.uv_pitch, fd.crop_y, fd.crop_x};
  }
  static __device__ __forceinline__ int sat8(int v) { return min(max(v >> 20, 0), 255); }
  __device__ __forceinline__ void tap(const Window& w, int sy, int sx, int p[3]) const {
    const int y = w.y0 + sy, x = w.x0 + sx;
    const unsigned char* c = w.uv + (size_t)(y >> 1) * w.pitch_uv + 2 * (x >> 1);
    const int yy = max(0, (int)w.y[(size_t)y * w.pitch_y + x] - k.y_off) * k.cy + (1 << 19);
    const int u = (int)c[0] - 128, v = (int)c[1] - 128;
    p[0] = sat8(yy + k.cub * u);
    p[1] = sat8(yy + k.cvg * v + k.cug * u);
    p[2] = sat8(yy + k.cvr * v);
  }
  // an odd size has no whole chroma sample for its last row / column: such a row is not read (flag 2), like one without pixels.  (A flag-2
  // crop reads pixel (0, 0) of image 0, i.e. Y[0] and UV[0..1]: image 0 has to be a surface with even sizes -- the header says so.)
  static __device__ __forceinline__ bool readable(const Image& im) { return im.h > 0 && im.w > 0 && !((im.h | im.w) & 1); }
  static __device__ __forceinline__ void point(Frame& d, const Image& im) {
    d.src = im.y;
    d.src_pitch = im.pitch_y;
    d.uv = im.uv;
    d.uv_pitch = im.pitch_uv;
  }
};

template <class Source>
__global__ __launch_bounds__(256) void preprocess_kernel(const typename Source::Frame* __restrict__ frames, float* __restrict__ dst, int pad_h,
                                                         int pad_w, float m0, float m1, float m2, float s0, float s1, float s2, int to_rgb,
                                                         const Source source) {
#pragma clang fp contract(off)
  const typename Source::Frame fd = frames[blockIdx.y];
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
  const typename Source::Window win = source.window(fd);
  int p00[3], p01[3], p10[3], p11[3];
  source.tap(win, cy.s0, cx.s0, p00);
  source.tap(win, cy.s0, cx.s1, p01);
  source.tap(win, cy.s1, cx.s0, p10);
  source.tap(win, cy.s1, cx.s1, p11);
  int v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h0 = p00[c] * cx.a0 + p01[c] * cx.a1;
    const int h1 = p10[c] * cx.a0 + p11[c] * cx.a1;
    v[c] = (((cy.a0 * (h0 >> 4)) >> 16) + ((cy.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
  }
  const int c0 = to_rgb ? 2 : 0, c2 = to_rgb ? 0 : 2;  // taps are BGR
  out[0] = ((float)v[c0] - m0) * s0;
  out[plane] = ((float)v[1] - m1) * s1;
  out[2 * plane] = ((float)v[c2] - m2) * s2;
}

template <class Source>
static int preprocess_frames(const char* what, const Source& source, mcg_stream stream, const typename Source::Frame* frames_dev, int num_frames,
                             float* dst, int pad_h, int pad_w, const float mean[3], const float stdinv[3], int to_rgb) {
  MCG_CHECK_ARG(frames_dev && dst && mean && stdinv, "%s: null pointer", what);
  MCG_CHECK_ARG(num_frames >= 0 && pad_h > 0 && pad_w > 0, "%s: bad sizes n=%d pad=%dx%d", what, num_frames, pad_h, pad_w);
  MCG_CHECK_ARG(num_frames <= 65535, "%s: at most 65535 frames per call (got %d)", what, num_frames);
  if (num_frames == 0) return MCG_OK;
  dim3 grid((pad_h * pad_w + 255) / 256, num_frames);
  hipLaunchKernelGGL(preprocess_kernel<Source>, grid, dim3(256), 0, (hipStream_t)stream, frames_dev, dst, pad_h, pad_w, mean[0], mean[1], mean[2],
                     stdinv[0], stdinv[1], stdinv[2], to_rgb, source);
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

extern "C" int mcg_preprocess_frames(mcg_stream stream, const mcg_frame_desc* frames_dev, int num_frames, float* dst, int pad_h, int pad_w,
                                     const float mean[3], const float stdinv[3], int to_rgb) {
  return preprocess_frames("mcg_preprocess_frames", PackedSource{}, stream, frames_dev, num_frames, dst, pad_h, pad_w, mean, stdinv, to_rgb);
}

// 255 * 2^22 + 2 * 128 * 2^22 + 2^19 < 2^31: with these limits no sum of the conversion leaves an int
static int check_yuv_coef(const char* what, const mcg_yuv_coef* k) {
  MCG_CHECK_ARG(k, "%s: null coef", what);
  constexpr int lim = 1 << 22;
  const auto inside = [](int c) { return c > -lim && c < lim; };      // (not abs(): abs(INT_MIN) is not a positive number)
  MCG_CHECK_ARG(k->y_off >= 0 && k->y_off <= 255 && inside(k->cy) && inside(k->cub) && inside(k->cug) && inside(k->cvg) && inside(k->cvr),
                "%s: coef {%d, %d, %d, %d, %d, %d} outside y_off in [0, 255], |c| < 2^22", what, k->y_off, k->cy, k->cub, k->cug, k->cvg, k->cvr);
  return MCG_OK;
}

extern "C" int mcg_preprocess_frames_nv12(mcg_stream stream, const mcg_nv12_frame_desc* frames_dev, int num_frames, float* dst, int pad_h,
                                          int pad_w, const float mean[3], const float stdinv[3], int to_rgb, const mcg_yuv_coef* coef) {
  if (int rc = check_yuv_coef("mcg_preprocess_frames_nv12", coef)) return rc;
  return preprocess_frames("mcg_preprocess_frames_nv12", Nv12Source{*coef}, stream, frames_dev, num_frames, dst, pad_h, pad_w, mean, stdinv, to_rgb);
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

template <class Source>
__global__ __launch_bounds__(256) void head_crop_plan_kernel(const typename Source::Image* __restrict__ images, int num_images,
                                                             const float* __restrict__ boxes, const int32_t* __restrict__ image_of, int n,
                                                             double expand, int scale_long, int scale_short, int pad_h, int pad_w,
                                                             typename Source::Frame* __restrict__ desc, int32_t* __restrict__ img_hw,
                                                             float* __restrict__ scale_factor, int32_t* __restrict__ flags) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double x1 = boxes[4 * k], y1 = boxes[4 * k + 1], x2 = boxes[4 * k + 2], y2 = boxes[4 * k + 3];   // f32 -> double: exact
  const int io = image_of[k];
  bool usable = io >= 0 && io < num_images && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
  typename Source::Image im = images[usable ? io : 0];
  if (usable && !Source::readable(im)) {                  // an image row with no pixels names nothing to read either
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
  typename Source::Frame d;
  Source::point(d, im);
  d.src_h = im.h; d.src_w = im.w;
  d.crop_y = ys.lo; d.crop_x = xs.lo; d.crop_h = h; d.crop_w = w;
  d.out_h = new_h; d.out_w = new_w;
  desc[k] = d;
  img_hw[2 * k] = new_h;
  img_hw[2 * k + 1] = new_w;
  const float fw = (float)((double)new_w / (double)w), fh = (float)((double)new_h / (double)h);
  scale_factor[4 * k] = fw; scale_factor[4 * k + 1] = fh; scale_factor[4 * k + 2] = fw; scale_factor[4 * k + 3] = fh;
  if (flags) flags[k] = flag;
}

template <class Source>
static int preprocess_head_crops(const char* what, const char* what_plan, const Source& source, mcg_stream stream, const typename Source::Image* images_dev, int num_images,
                                 const float* boxes_dev, const int32_t* image_of_dev, int n, double expand, int scale_w, int scale_h,
                                 typename Source::Frame* desc_out_dev, int32_t* img_hw_dev, float* scale_factor_dev, int32_t* flags_dev, float* dst,
                                 int pad_h, int pad_w, const float mean[3], const float stdinv[3], int to_rgb) {
  MCG_CHECK_ARG(images_dev && boxes_dev && image_of_dev && desc_out_dev && img_hw_dev && scale_factor_dev && dst && mean && stdinv,
                "%s: null pointer", what);
  MCG_CHECK_ARG(n >= 0 && num_images >= 1 && scale_w > 0 && scale_h > 0, "%s: bad sizes n=%d images=%d scale=%dx%d", what, n, num_images, scale_w,
                scale_h);
  MCG_CHECK_ARG(n <= 65535, "%s: at most 65535 crops per call (got %d)", what, n);
  MCG_CHECK_ARG(expand == expand && expand - expand == 0.0, "%s: expand must be finite", what);
  // keep_ratio puts the LONG edge of img_scale on the window's long side, whichever that is: a non-square scale needs room for it both ways
  const int need_h = scale_w == scale_h ? scale_h : max(scale_w, scale_h), need_w = scale_w == scale_h ? scale_w : max(scale_w, scale_h);
  MCG_CHECK_ARG(pad_h >= need_h && pad_w >= need_w, "%s: pad %dx%d cannot hold img_scale (%d, %d)", what, pad_h, pad_w, scale_w, scale_h);
  if (n == 0) return MCG_OK;
  hipLaunchKernelGGL(head_crop_plan_kernel<Source>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, images_dev, num_images, boxes_dev,
                     image_of_dev, n, expand, max(scale_w, scale_h), min(scale_w, scale_h), pad_h, pad_w, desc_out_dev, img_hw_dev,
                     scale_factor_dev, flags_dev);
  MCG_CHECK_LAUNCH(what_plan);
  return preprocess_frames(what, source, stream, desc_out_dev, n, dst, pad_h, pad_w, mean, stdinv, to_rgb);
}

extern "C" int mcg_preprocess_head_crops(mcg_stream stream, const mcg_image_desc* images_dev, int num_images, const float* boxes_dev,
                                         const int32_t* image_of_dev, int n, double expand, int scale_w, int scale_h,
                                         mcg_frame_desc* desc_out_dev, int32_t* img_hw_dev, float* scale_factor_dev, int32_t* flags_dev,
                                         float* dst, int pad_h, int pad_w, const float mean[3], const float stdinv[3], int to_rgb) {
  return preprocess_head_crops("mcg_preprocess_head_crops", "mcg_preprocess_head_crops (plan)", PackedSource{}, stream, images_dev, num_images, boxes_dev, image_of_dev, n, expand, scale_w,
                               scale_h, desc_out_dev, img_hw_dev, scale_factor_dev, flags_dev, dst, pad_h, pad_w, mean, stdinv, to_rgb);
}

extern "C" int mcg_preprocess_head_crops_nv12(mcg_stream stream, const mcg_nv12_image_desc* images_dev, int num_images, const float* boxes_dev,
                                              const int32_t* image_of_dev, int n, double expand, int scale_w, int scale_h,
                                              mcg_nv12_frame_desc* desc_out_dev, int32_t* img_hw_dev, float* scale_factor_dev,
                                              int32_t* flags_dev, float* dst, int pad_h, int pad_w, const float mean[3], const float stdinv[3],
                                              int to_rgb, const mcg_yuv_coef* coef) {
  if (int rc = check_yuv_coef("mcg_preprocess_head_crops_nv12", coef)) return rc;
  return preprocess_head_crops("mcg_preprocess_head_crops_nv12", "mcg_preprocess_head_crops_nv12 (plan)", Nv12Source{*coef}, stream, images_dev, num_images, boxes_dev, image_of_dev, n, expand,
                               scale_w, scale_h, desc_out_dev, img_hw_dev, scale_factor_dev, flags_dev, dst, pad_h, pad_w, mean, stdinv, to_rgb);
}

// The detector's input (mcg_letterbox_frames, mcg_letterbox_frames_nv12): the header comment "the detector's input" states the arithmetic.
// The taps, lin_coef and the two integer passes are preprocess_kernel's; what differs is the rectangle (anywhere inside the output, the
// rest 114), the value written (the byte, or byte / 255 as float or half) and PX adjacent pixels of a row per thread, so that the 8- and
// 16-bit outputs leave as 4-byte stores.  Nothing of a descriptor is trusted: the window is the whole frame whatever its crop fields say,
// a frame that cannot be read is all border, and the rectangle is compared in 64 bits -- so no table makes a thread read outside a frame
// (lin_coef clamps every tap to [0, src - 1]) or write outside dst (a thread owns output pixels, not source pixels).
__device__ __forceinline__ bool whole_frame(const mcg_frame_desc& fd) { return fd.src_h > 0 && fd.src_w > 0; }
__device__ __forceinline__ bool whole_frame(const mcg_nv12_frame_desc& fd) { return fd.src_h > 0 && fd.src_w > 0 && !((fd.src_h | fd.src_w) & 1); }

// byte / 255: an IEEE f32 division (HIP's default; the test over all 256 bytes decides), then ONE rounding to half
__device__ __forceinline__ float unit_value(int v) {
#pragma clang fp contract(off)
  return (float)v / 255.0f;
}

template <int PX>
__device__ __forceinline__ void store_values(unsigned char* p, const int v[PX]) {
  if constexpr (PX == 4) *reinterpret_cast<unsigned int*>(p) = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16 | (unsigned)v[3] << 24;
  else p[0] = (unsigned char)v[0];
}
template <int PX>
__device__ __forceinline__ void store_values(__half* p, const int v[PX]) {
  if constexpr (PX == 2) *reinterpret_cast<__half2*>(p) = __halves2half2(__float2half_rn(unit_value(v[0])), __float2half_rn(unit_value(v[1])));
  else p[0] = __float2half_rn(unit_value(v[0]));
}
template <int PX>
__device__ __forceinline__ void store_values(float* p, const int v[PX]) {
  p[0] = unit_value(v[0]);
}

template <class Source, class T, int PX>
__global__ __launch_bounds__(256) void letterbox_kernel(const typename Source::Letterbox* __restrict__ frames, T* __restrict__ dst, int out_h,
                                                        int out_w, int swap_rb, const Source source) {
#pragma clang fp contract(off)
  const typename Source::Letterbox ld = frames[blockIdx.y];
  typename Source::Frame fd = ld.frame;
  fd.crop_y = 0; fd.crop_x = 0; fd.crop_h = fd.src_h; fd.crop_w = fd.src_w;      // the whole frame
  const int groups = out_w / PX;                                                    // the entry picks a PX that divides out_w
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= out_h * groups) return;
  const int y = idx / groups, x0 = (idx - y * groups) * PX;
  const long long ry = (long long)y - ld.top;
  const bool row_inside = whole_frame(fd) && fd.out_h > 0 && fd.out_w > 0 && ry >= 0 && ry < fd.out_h;
  const typename Source::Window win = source.window(fd);
  LinCoef cy = {0, 0, 0, 0};
  if (row_inside) cy = lin_coef((int)ry, fd.out_h, fd.src_h);
  int v[3][PX];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    const long long rx = (long long)(x0 + i) - ld.left;
    if (row_inside && rx >= 0 && rx < fd.out_w) {
      const LinCoef cx = lin_coef((int)rx, fd.out_w, fd.src_w);
      int p00[3], p01[3], p10[3], p11[3];
      source.tap(win, cy.s0, cx.s0, p00);
      source.tap(win, cy.s0, cx.s1, p01);
      source.tap(win, cy.s1, cx.s0, p10);
      source.tap(win, cy.s1, cx.s1, p11);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int h0 = p00[c] * cx.a0 + p01[c] * cx.a1;
        const int h1 = p10[c] * cx.a0 + p11[c] * cx.a1;
        v[c][i] = (((cy.a0 * (h0 >> 4)) >> 16) + ((cy.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
      }
    } else {
      v[0][i] = v[1][i] = v[2][i] = 114;
    }
  }
  const size_t plane = (size_t)out_h * out_w;
  T* out = dst + (size_t)blockIdx.y * 3 * plane + (size_t)y * out_w + x0;
  store_values<PX>(out, v[swap_rb ? 2 : 0]);
  store_values<PX>(out + plane, v[1]);
  store_values<PX>(out + 2 * plane, v[swap_rb ? 0 : 2]);
}

template <class Source, class T, int PX>
static void letterbox_launch(const Source& source, mcg_stream stream, const void* frames_dev, int num_frames, void* dst, int out_h, int out_w, int swap_rb) {
  dim3 grid((out_h * (out_w / PX) + 255) / 256, num_frames);
  hipLaunchKernelGGL((letterbox_kernel<Source, T, PX>), grid, dim3(256), 0, (hipStream_t)stream,
                     (const typename Source::Letterbox*)frames_dev, (T*)dst, out_h, out_w, swap_rb, source);
}

template <class Source>
static int letterbox_frames(const char* what, const Source& source, mcg_stream stream, const void* frames_dev, int num_frames, void* dst, int out_h,
                            int out_w, int out_type, int swap_rb) {
  MCG_CHECK_ARG(frames_dev && dst, "%s: null pointer", what);
  MCG_CHECK_ARG(num_frames >= 0 && out_h > 0 && out_w > 0 && (long long)out_h * out_w <= 0x7fffffffLL, "%s: bad sizes n=%d out=%dx%d", what,
                num_frames, out_h, out_w);
  MCG_CHECK_ARG(num_frames <= 65535, "%s: at most 65535 frames per call (got %d)", what, num_frames);
  MCG_CHECK_ARG(out_type == MCG_LETTERBOX_U8 || out_type == MCG_LETTERBOX_F16 || out_type == MCG_LETTERBOX_F32, "%s: unknown out_type %d", what, out_type);
  const size_t elem = out_type == MCG_LETTERBOX_U8 ? 1 : out_type == MCG_LETTERBOX_F16 ? 2 : 4;
  MCG_CHECK_ARG((uintptr_t)dst % elem == 0, "%s: dst is not aligned to its %zu-byte elements", what, elem);
  if (num_frames == 0) return MCG_OK;
  // 4-byte stores need every row of every plane to start on 4 bytes: dst does and out_w is a multiple of the pixels per store
  const bool wide = (uintptr_t)dst % 4 == 0;
  if (out_type == MCG_LETTERBOX_U8) {
    if (wide && out_w % 4 == 0) letterbox_launch<Source, unsigned char, 4>(source, stream, frames_dev, num_frames, dst, out_h, out_w, swap_rb);
    else letterbox_launch<Source, unsigned char, 1>(source, stream, frames_dev, num_frames, dst, out_h, out_w, swap_rb);
  } else if (out_type == MCG_LETTERBOX_F16) {
    if (wide && out_w % 2 == 0) letterbox_launch<Source, __half, 2>(source, stream, frames_dev, num_frames, dst, out_h, out_w, swap_rb);
    else letterbox_launch<Source, __half, 1>(source, stream, frames_dev, num_frames, dst, out_h, out_w, swap_rb);
  } else {
    letterbox_launch<Source, float, 1>(source, stream, frames_dev, num_frames, dst, out_h, out_w, swap_rb);
  }
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

extern "C" int mcg_letterbox_frames(mcg_stream stream, const mcg_letterbox_desc* frames_dev, int num_frames, void* dst, int out_h, int out_w,
                                    int out_type, int swap_rb) {
  return letterbox_frames("mcg_letterbox_frames", PackedSource{}, stream, frames_dev, num_frames, dst, out_h, out_w, out_type, swap_rb);
}

extern "C" int mcg_letterbox_frames_nv12(mcg_stream stream, const mcg_nv12_letterbox_desc* frames_dev, int num_frames, void* dst, int out_h,
                                         int out_w, int out_type, int swap_rb, const mcg_yuv_coef* coef) {
  if (int rc = check_yuv_coef("mcg_letterbox_frames_nv12", coef)) return rc;
  return letterbox_frames("mcg_letterbox_frames_nv12", Nv12Source{*coef}, stream, frames_dev, num_frames, dst, out_h, out_w, out_type, swap_rb);
}
