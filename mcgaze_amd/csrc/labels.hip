// Text labels on the device (include/mcgaze_hip.h, "text labels"): track ids, dwell seconds and region names become words in the frames
// they belong to -- packed BGR frames (mcg_draw_labels) or NV12 surfaces (mcg_draw_labels_nv12), written in place.  mcg_format_labels makes
// the text of a row ('#12 3.4s') from the id and the frame count that are in device memory already; the font is DATA the caller brings, a
// device uint8 [96][8] table.  The arithmetic is stated once, in the header; mcgaze_amd/arrows.py::draw_labels_host / format_labels_host
// are the same on the host, bit for bit.
//
// Drawing is two launches, draw.hip's design.  label_plan_kernel: one thread per row writes a mcg_label_desc -- the text origin, the plate
// clipped to the frame, the length, the packed colour, the codes.  label_raster_kernel is a GATHER over (image, pixel tile): each wave owns a
// strip of its tile, ballots the plan 64 records at a time against the strip, and walks the hits in ASCENDING order; a lane remembers the
// highest STROKE (2 k: the plate of row k, 2 k + 1: its glyph pixels) that covered each of its pixels and stores once, after the walk.  No
// LDS, no atomics; the code of a pixel's character and its font row are two dependent byte loads from tables of 24 n and 768 bytes that stay
// in the cache.  Cost, as for the arrows: every wave reads n / 64 slices of the plan -- made for the tens of labels of a video frame.
#include "draw_common.hpp"   // the bounds, the tile, PackedTarget / Nv12Target

// decimal(v) at row[pos ..], cut at the row's end -> the position behind it
__device__ __forceinline__ int label_decimal(unsigned char* __restrict__ row, int pos, unsigned v) {
  int digits = 1;
  for (unsigned t = v; t >= 10; t /= 10) ++digits;
  for (int i = digits - 1; i >= 0; --i, v /= 10)
    if (pos + i < MCG_LABEL_CHARS) row[pos + i] = (unsigned char)('0' + v % 10);
  return pos + digits;
}

__device__ __forceinline__ int label_char(unsigned char* __restrict__ row, int pos, char c) {
  if (pos < MCG_LABEL_CHARS) row[pos] = (unsigned char)c;
  return pos + 1;
}

__global__ __launch_bounds__(256) void format_labels_kernel(const int32_t* __restrict__ id, const int32_t* __restrict__ value, int n, int num, int den,
                                                            unsigned char* __restrict__ text) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  unsigned char* row = text + (size_t)k * MCG_LABEL_CHARS;
  int pos = 0;
  const int v = id[k];
  if (v > 0) {
    pos = label_decimal(row, label_char(row, pos, '#'), (unsigned)v);
    const int f = value ? value[k] : 0;
    if (f > 0) {
      const long long q = (long long)f * 10 * den / num;          // f < 2^31, den <= 2^20: below 2^55; q / 10 <= f since den <= num
      pos = label_decimal(row, label_char(row, pos, ' '), (unsigned)(q / 10));
      pos = label_char(row, pos, '.');
      pos = label_char(row, pos, (char)('0' + (int)(q % 10)));
      pos = label_char(row, pos, 's');
    }
  }
  for (int i = min(pos, MCG_LABEL_CHARS); i < MCG_LABEL_CHARS; ++i) row[i] = 0;
}

template <class Target>
__global__ __launch_bounds__(256) void label_plan_kernel(const typename Target::Image* __restrict__ images, int num_images, int max_h, int max_w,
                                                         const float* __restrict__ boxes, const int32_t* __restrict__ image_of,
                                                         const unsigned char* __restrict__ text, const int32_t* __restrict__ place, int n, int scale,
                                                         int advance, int pad, unsigned color, const unsigned char* __restrict__ colors,
                                                         mcg_label_desc* __restrict__ plan, int32_t* __restrict__ flags) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double x1 = boxes[4 * k], y1 = boxes[4 * k + 1], x2 = boxes[4 * k + 2], y2 = boxes[4 * k + 3];   // f32 -> double: exact
  const int io = image_of[k];
  mcg_label_desc d = {};
  d.image = -1;
  d.flag = 2;
  bool usable = io >= 0 && io < num_images && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
  int h = 0, w = 0;
  if (usable) {
    const typename Target::Image im = images[io];
    h = im.h;
    w = im.w;
    usable = Target::writable(im) && h <= max_h && w <= max_w;     // max_h, max_w <= 8192: what the raster grid covers
  }
  const double bx1 = trunc(x1), by1 = trunc(y1), bx2 = trunc(x2), by2 = trunc(y2), lim = (double)MCG_DRAW_COORD;
  usable = usable && fabs(bx1) <= lim && fabs(by1) <= lim && fabs(bx2) <= lim && fabs(by2) <= lim;
  if (usable) {
    const unsigned char* t = text + (size_t)k * MCG_LABEL_CHARS;
    int len = 0;
    while (len < MCG_LABEL_CHARS && t[len]) ++len;
    d.flag = len ? 0 : 1;                                         // an empty label: nothing is written
    if (len) {
      const int P = pad * scale, PW = len * advance * scale + 2 * P, PH = 8 * scale + 2 * P;
      int X = (int)bx1, Y = (int)by1;
      if ((place ? place[k] : 0) != 1) {                          // above the box, else below it
        Y -= PH;
        if (Y < 0) Y = (int)by2 + 1;
      }
      X = max(0, min(X, w - PW));                                 // a plate wider than the frame starts at 0 and is clipped
      Y = max(0, min(Y, h - PH));
      d.x = X + P; d.y = Y + P;
      d.x0 = X; d.y0 = Y;
      d.x1 = min(X + PW, w); d.y1 = min(Y + PH, h);               // half open, inside the frame, never empty
      d.image = io;
      d.len = len;
      d.color = colors ? (unsigned)colors[3 * k] | (unsigned)colors[3 * k + 1] << 8 | (unsigned)colors[3 * k + 2] << 16 : color;
      for (int i = 0; i < len; ++i) d.text[i] = t[i];
    }
  }
  plan[k] = d;
  if (flags) flags[k] = d.flag;
}

template <class Target>
__global__ __launch_bounds__(MCG_DRAW_THREADS) void label_raster_kernel(const typename Target::Image* __restrict__ images, int tiles_x,
                                                                        const mcg_label_desc* __restrict__ plan, int n,
                                                                        const unsigned char* __restrict__ font, int scale, int cell, int plates,
                                                                        unsigned background) {
  constexpr int S = Target::CELL;
  const int img = blockIdx.y;
  const typename Target::Image im = images[img];
  if (!Target::writable(im) || im.h > MCG_DRAW_SIDE || im.w > MCG_DRAW_SIDE) return;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the strip of this wave, in pixels: [sx0, sx1) x [sy0, sy1)
  const int sx0 = tile_x * MCG_DRAW_TILE_W * S, sy0 = (tile_y * MCG_DRAW_TILE_H + 2 * wave) * S;
  const int sx1 = sx0 + MCG_DRAW_TILE_W * S, sy1 = sy0 + 2 * S;
  if (sx0 >= im.w || sy0 >= im.h) return;                         // wave-uniform: the whole strip lies outside this image
  const int px0 = sx0 + (lane & 31) * S, py0 = sy0 + (lane >> 5) * S;   // this lane's cell
  const int th = 8 * scale;
  int win[S * S];                                                 // the highest stroke over each pixel: 2 j the plate of row j, 2 j + 1 its glyphs
#pragma unroll
  for (int i = 0; i < S * S; ++i) win[i] = -1;
  for (int base = 0; base < n; base += 64) {
    const int r = base + lane;
    bool hit = false;
    if (r < n) {
      const mcg_label_desc* d = plan + r;
      hit = d->flag == 0 && d->image == img && d->x0 < sx1 && d->x1 > sx0 && d->y0 < sy1 && d->y1 > sy0;
    }
    unsigned long long mask = __ballot(hit);
    while (mask) {                                                // ascending rows: a later label overwrites an earlier one
      const int j = base + __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const mcg_label_desc* d = plan + j;                         // one address for the wave
      const int x0 = d->x0, y0 = d->y0, x1 = d->x1, y1 = d->y1, tx = d->x, ty = d->y, tw = d->len * cell;
#pragma unroll
      for (int i = 0; i < S * S; ++i) {
        const int px = px0 + (i % S), py = py0 + (i / S);
        // the plate is clipped to the frame: a covered pixel has px < w and py < h
        const bool in = px >= x0 && px < x1 && py >= y0 && py < y1;
        const int fx = px - tx, fy = py - ty;
        int glyph = 0;
        if (in && fx >= 0 && fx < tw && fy >= 0 && fy < th) {     // then ci < len <= 24, row < 8, col < advance <= 8
          const int ci = fx / cell, col = (fx - ci * cell) / scale, row = fy / scale;
          const int c = d->text[ci];
          const int g = (c >= 32 && c <= 126) ? c - 32 : 31;      // anything else: the '?' glyph
          glyph = (font[g * 8 + row] >> col) & 1;
        }
        win[i] = glyph ? 2 * j + 1 : (in && plates) ? 2 * j : win[i];
      }
    }
  }
  int top = -1;
#pragma unroll
  for (int i = 0; i < S * S; ++i) top = max(top, win[i]);
  if (top < 0) return;
  const unsigned ctop = (top & 1) ? plan[top >> 1].color : background;
  if constexpr (S == 1) {
    // (a covered pixel lies inside its row's clipped plate, hence inside the frame)
    unsigned char* q = (unsigned char*)im.src + (size_t)py0 * im.pitch + (size_t)px0 * 3;
    q[0] = (unsigned char)ctop; q[1] = (unsigned char)(ctop >> 8); q[2] = (unsigned char)(ctop >> 16);
  } else {
#pragma unroll
    for (int i = 0; i < S * S; ++i)
      if (win[i] >= 0)
        ((unsigned char*)im.y)[(size_t)(py0 + i / S) * im.pitch_y + px0 + (i % S)] = (unsigned char)((win[i] & 1) ? plan[win[i] >> 1].color : background);
    // px0, py0 even, and some pixel of the block is inside the frame, so (py0, px0) is: py0 >> 1 <= h / 2 - 1, px0 + 1 <= w - 1
    unsigned char* c = (unsigned char*)im.uv + (size_t)(py0 >> 1) * im.pitch_uv + px0;
    c[0] = (unsigned char)(ctop >> 8);
    c[1] = (unsigned char)(ctop >> 16);
  }
}

template <class Target>
static int draw_labels(const char* what, const char* what_plan, mcg_stream stream, const typename Target::Image* images_dev, int num_images, int max_h,
                       int max_w, const float* boxes_dev, const int32_t* image_of_dev, const unsigned char* text_dev, const int32_t* place_dev, int n,
                       const unsigned char* font_dev, int scale, int advance, int pad, const unsigned char* color, const unsigned char* colors_dev,
                       const unsigned char* background, mcg_label_desc* plan_out_dev, int32_t* flags_dev) {
  MCG_CHECK_ARG(images_dev && boxes_dev && image_of_dev && text_dev && font_dev && plan_out_dev && (color || colors_dev), "%s: null pointer", what);
  MCG_CHECK_ARG(n >= 0 && num_images >= 1 && num_images <= 65535, "%s: bad sizes n=%d images=%d", what, n, num_images);
  MCG_CHECK_ARG(n <= 65535, "%s: at most 65535 rows per call (got %d)", what, n);
  MCG_CHECK_ARG(max_h >= 1 && max_h <= MCG_DRAW_SIDE && max_w >= 1 && max_w <= MCG_DRAW_SIDE, "%s: frames of 1 .. 8192 pixels a side (got max %dx%d)",
                what, max_h, max_w);
  MCG_CHECK_ARG(scale >= 1 && scale <= 16 && advance >= 1 && advance <= 8 && pad >= 0 && pad <= 8,
                "%s: scale in 1 .. 16, advance in 1 .. 8, pad in 0 .. 8 (got %d, %d, %d)", what, scale, advance, pad);
  if (n == 0) return MCG_OK;
  const auto pack = [](const unsigned char* c) { return c ? (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16 : 0u; };
  hipLaunchKernelGGL(label_plan_kernel<Target>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, images_dev, num_images, max_h, max_w,
                     boxes_dev, image_of_dev, text_dev, place_dev, n, scale, advance, pad, pack(color), colors_dev, plan_out_dev, flags_dev);
  MCG_CHECK_LAUNCH(what_plan);
  constexpr int S = Target::CELL;
  const int tiles_x = (max_w + MCG_DRAW_TILE_W * S - 1) / (MCG_DRAW_TILE_W * S), tiles_y = (max_h + MCG_DRAW_TILE_H * S - 1) / (MCG_DRAW_TILE_H * S);
  hipLaunchKernelGGL(label_raster_kernel<Target>, dim3(tiles_x * tiles_y, num_images), dim3(MCG_DRAW_THREADS), 0, (hipStream_t)stream, images_dev,
                     tiles_x, plan_out_dev, n, font_dev, scale, advance * scale, background ? 1 : 0, pack(background));
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

extern "C" int mcg_format_labels(mcg_stream s, const int32_t* id_dev, const int32_t* value_dev, int n, int num, int den, unsigned char* text_out_dev) {
  MCG_CHECK_ARG(id_dev && text_out_dev, "mcg_format_labels: null pointer");
  MCG_CHECK_ARG(n >= 0 && n <= 65535, "mcg_format_labels: at most 65535 rows per call (got %d)", n);
  MCG_CHECK_ARG(den >= 1 && den <= num && num <= (1 << 20), "mcg_format_labels: a rate num / den with 1 <= den <= num <= 2^20 (got %d / %d)", num, den);
  if (n == 0) return MCG_OK;
  hipLaunchKernelGGL(format_labels_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, id_dev, value_dev, n, num, den, text_out_dev);
  MCG_CHECK_LAUNCH("mcg_format_labels");
  return MCG_OK;
}

extern "C" int mcg_draw_labels(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                               const int32_t* image_of_dev, const unsigned char* text_dev, const int32_t* place_dev, int n,
                               const unsigned char* font_dev, int scale, int advance, int pad, const unsigned char* color,
                               const unsigned char* colors_dev, const unsigned char* background, mcg_label_desc* plan_out_dev, int32_t* flags_dev) {
  return draw_labels<PackedTarget>("mcg_draw_labels", "mcg_draw_labels (plan)", s, images_dev, num_images, max_h, max_w, boxes_dev, image_of_dev,
                                   text_dev, place_dev, n, font_dev, scale, advance, pad, color, colors_dev, background, plan_out_dev, flags_dev);
}

extern "C" int mcg_draw_labels_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                                    const int32_t* image_of_dev, const unsigned char* text_dev, const int32_t* place_dev, int n,
                                    const unsigned char* font_dev, int scale, int advance, int pad, const unsigned char* yuv,
                                    const unsigned char* yuvs_dev, const unsigned char* background, mcg_label_desc* plan_out_dev, int32_t* flags_dev) {
  return draw_labels<Nv12Target>("mcg_draw_labels_nv12", "mcg_draw_labels_nv12 (plan)", s, images_dev, num_images, max_h, max_w, boxes_dev,
                                 image_of_dev, text_dev, place_dev, n, font_dev, scale, advance, pad, yuv, yuvs_dev, background, plan_out_dev,
                                 flags_dev);
}
