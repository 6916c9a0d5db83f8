// Anonymised heads on the device (include/mcgaze_hip.h, "anonymised heads"): the faces under the head boxes removed IN PLACE from packed BGR
// frames (mcg_anonymize_heads) or NV12 surfaces (mcg_anonymize_heads_nv12) -- every covered pixel becomes the mean of a coarse cell of the
// frame (mosaic) or one colour (fill).  The arithmetic is stated once, in the header; mcgaze_amd/arrows.py::anonymize_plan_host and
// anonymize_heads_host are the same on the host, bit for bit.
//
// Two launches, the arrows' design.  anonymize_plan_kernel: one thread per row, in double and uncontracted, writes a mcg_anon_desc -- the
// integer rectangle that contains the expanded box, clipped to the frame, twice its centre, its size, the shift of its cells, the flag.
//
// anonymize_render_kernel is the second whole-frame kernel of the project, and unlike heat_render_kernel it reads NEIGHBOURS of the pixels
// it writes, in place.  A block owns a frame-aligned tile of 64 x 64 pixels: the cells of every shift (2 .. 64 pixels a side, aligned to
// the frame's origin) lie inside exactly one tile, so a block reads only its own tile, reads all of it before it writes any of it, and no
// other block touches those bytes -- no second buffer, no atomics on the image.  The block walks the plan in chunks of 256 descriptors,
// keeps those of its image whose rectangle meets the tile in LDS (any number of them: a chunk is used up before the next is read) and
// every thread works out s(p), the largest shift that covers each of its 16 pixels of a row (NV12: 16 x 2).  A tile under no head leaves
// before any pixel is read.  Mosaic: the tile's 2 x 2 sums go into LDS, are folded upward to the largest shift the tile needs, and the
// levels that are read become means; then every thread with a covered pixel rewrites its span.  Pixel accesses are heat_render_kernel's:
// 16-byte wide where the plane's address and pitch allow, 4-byte wide where only those are aligned, byte by byte otherwise and at the
// right edge.  The sums are integers, so any order of adding gives the same bits.  No scratch.
#include "draw_common.hpp"   // the bounds, PackedTarget / Nv12Target, the span accesses

#define MCG_ANON_TILE 64                    // pixels a side: the largest cell
#define MCG_ANON_SPAN 16                    // pixels of a row a thread owns; 4 threads side by side
#define MCG_ANON_CHUNK 256                  // descriptors a block looks at between two barriers: one per thread
#define MCG_ANON_WORDS 1368                 // the levels 1 .. 6 of one channel, 32 x 32 + 16 x 16 + ... + 1 = 1365 words, kept 16-byte aligned

// where level s (cells of 2^s pixels, 64 >> s of them a side) starts among a channel's words: 0, 1024, 1280, 1344, 1360, 1364, (1365)
__host__ __device__ __forceinline__ constexpr int anon_level(int s) { return (4096 - (16384 >> (2 * s))) / 3; }

// ---------------------------------------------------------------- plan
template <class Target>
__global__ __launch_bounds__(256) void anonymize_plan_kernel(const typename Target::Image* __restrict__ images, int num_images, int max_h, int max_w,
                                                             const float* __restrict__ boxes, const int32_t* __restrict__ image_of, int n, double expand,
                                                             int shape, int cell_shift, int blocks, mcg_anon_desc* __restrict__ plan,
                                                             int32_t* __restrict__ flags) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double x1 = boxes[4 * k], y1 = boxes[4 * k + 1], x2 = boxes[4 * k + 2], y2 = boxes[4 * k + 3];   // f32 -> double: exact
  const int io = image_of[k];
  mcg_anon_desc d = {};
  d.image = -1;
  d.flag = 2;
  bool usable = io >= 0 && io < num_images && isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && x2 > x1 && y2 > y1;
  int h = 0, w = 0;
  if (usable) {
    const typename Target::Image im = images[io];
    h = im.h;
    w = im.w;
    usable = Target::writable(im) && h <= max_h && w <= max_w;   // max_h, max_w <= 8192: what the tile grid covers
  }
  if (usable) {
    const double ex = expand * (x2 - x1), ey = expand * (y2 - y1);
    // floor / ceil outward: the integer rectangle contains the float box, and x2 > x1 makes it at least one pixel wide
    const double X0 = floor(x1 - ex), X1 = ceil(x2 + ex), Y0 = floor(y1 - ey), Y1 = ceil(y2 + ey);
    const double lim = (double)MCG_DRAW_COORD;
    usable = fabs(X0) <= lim && fabs(X1) <= lim && fabs(Y0) <= lim && fabs(Y1) <= lim;
    if (usable) {
      const int ix0 = (int)X0, ix1 = (int)X1, iy0 = (int)Y0, iy1 = (int)Y1;
      d.W = ix1 - ix0;
      d.H = iy1 - iy0;
      int s = cell_shift;
      if (s == 0) {                                               // about `blocks` cells across the head, whatever its distance
        s = 6;
        for (int c = 5; c >= 1; --c)
          if ((blocks << c) >= max(d.W, d.H)) s = c;
      }
      d.shift = s;
      d.shape = shape;
      d.cx2 = ix0 + ix1;
      d.cy2 = iy0 + iy1;
      d.x0 = max(ix0, 0); d.y0 = max(iy0, 0);
      d.x1 = min(ix1, w); d.y1 = min(iy1, h);                     // half open; empty for a head outside its frame
      d.image = io;
      d.flag = 0;
    }
  }
  plan[k] = d;
  if (flags) flags[k] = d.flag;
}

// ---------------------------------------------------------------- render
// s(p) of the 16 pixels from px0 on in row py under row r, merged into sh.  Exactly, in 64-bit integers: |2 p + 1 - c2| < 2^15 (p <= 8191 + 15,
// |c2| <= 16382), so its square fits an int; W, H < 2^14, so W^2 and H^2 are below 2^28, each product below 2^58 and their sum below 2^59.
// Branch-free, as capsule() is: the tests are combined with & and |.
__device__ __forceinline__ void anon_cover(const mcg_anon_desc& r, int px0, int py, int (&sh)[MCG_ANON_SPAN]) {
  const long long WW = (long long)r.W * r.W, HH = (long long)r.H * r.H;
  const int dy = 2 * py + 1 - r.cy2;
  const long long rest = WW * HH - (long long)(dy * dy) * WW;     // what the x term may use up
  const int in_y = (py >= r.y0) & (py < r.y1), box = r.shape == 0;
#pragma unroll
  for (int j = 0; j < MCG_ANON_SPAN; ++j) {
    const int px = px0 + j, dx = 2 * px + 1 - r.cx2;
    const int covered = in_y & (px >= r.x0) & (px < r.x1) & (box | (int)((long long)(dx * dx) * HH <= rest));
    sh[j] = covered ? max(sh[j], r.shift) : sh[j];
  }
}

template <class Target>
__global__ __launch_bounds__(256) void anonymize_render_kernel(const typename Target::Image* __restrict__ images, int tiles_x, int max_h, int max_w,
                                                               const mcg_anon_desc* __restrict__ plan, int n, int mode, unsigned c0, unsigned c1,
                                                               unsigned c2) {
  constexpr int R = Target::CELL;                                 // pixel rows of a thread: 1, NV12 2
  __shared__ mcg_anon_desc rows[MCG_ANON_CHUNK];
  __shared__ __align__(16) int pyr[3][MCG_ANON_WORDS];           // B, G, R (NV12: Y, U, V): sums, then means, of the cells of levels 1 .. 6
  __shared__ int kept, used;
  const int img = blockIdx.y;
  const typename Target::Image im = images[img];
  if (!Target::writable(im) || im.h > max_h || im.w > max_w) return;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int tx0 = tile_x * MCG_ANON_TILE, ty0 = tile_y * MCG_ANON_TILE;
  if (tx0 >= im.w || ty0 >= im.h) return;                         // block-uniform, like every return above: nobody waits at a barrier
  const int t = threadIdx.x;
  const int lx0 = (t & 3) * MCG_ANON_SPAN, ly0 = (t >> 2) * R;    // inside the tile; NV12: threads 128 .. 255 have ly0 >= 64 and own no pixel
  const int px0 = tx0 + lx0, py0 = ty0 + ly0;
  const bool owner = ly0 < MCG_ANON_TILE && px0 < im.w && py0 < im.h;

  // 1. the rows of this tile, chunk by chunk: s(p) of the thread's pixels
  int sh[R][MCG_ANON_SPAN] = {};
  int any = 0;
  if (t == 0) used = 0;
  for (int c = 0; c < n; c += MCG_ANON_CHUNK) {
    if (t == 0) kept = 0;
    __syncthreads();
    if (c + t < n) {
      const mcg_anon_desc d = plan[c + t];
      if (d.image == img && d.flag == 0 && max(d.x0, tx0) < min(d.x1, tx0 + MCG_ANON_TILE) && max(d.y0, ty0) < min(d.y1, ty0 + MCG_ANON_TILE)) {
        rows[atomicAdd(&kept, 1)] = d;                            // in any order: a maximum commutes
        atomicOr(&used, 1 << d.shift);
        any = 1;
      }
    }
    __syncthreads();
    const int m = kept;
    if (owner)
      for (int j = 0; j < m; ++j) {
        const mcg_anon_desc r = rows[j];                          // one address for the whole wave: a broadcast
#pragma unroll
        for (int q = 0; q < R; ++q) anon_cover(r, px0, py0 + q, sh[q]);
      }
    __syncthreads();                                              // everybody is through with this chunk before `kept` and `rows` are reused
  }
  if (!__syncthreads_or(any)) return;                             // no head over this tile: no pixel of it is read

  int mine = 0;
#pragma unroll
  for (int q = 0; q < R; ++q)
#pragma unroll
    for (int j = 0; j < MCG_ANON_SPAN; ++j) mine |= sh[q][j];

  // 2. the thread's bytes: everybody's for the mosaic (a cell's mean is over all of its pixels), for the fill those of a span that is written
  const int span = owner ? min(MCG_ANON_SPAN, im.w - px0) : 0;    // pixels of the thread inside the picture
  const bool whole = span == MCG_ANON_SPAN, take = owner && (mode == 0 || mine);
  unsigned w[R == 1 ? 12 : 4] = {}, w1[4] = {}, wc[4] = {};       // BGR: 48 bytes; NV12: w, w1 the two luma rows, wc the chroma pairs
  int md = 0, md_uv = 0;
  unsigned char *p = nullptr, *pc = nullptr;
  if constexpr (R == 1) {
    md = span_mode(im.src, im.pitch, whole);
    p = (unsigned char*)im.src + (size_t)py0 * im.pitch + (size_t)px0 * 3;
    if (take) span_load<12>(p, w, md, 3 * span);
  } else {
    // py0 even and < h, h even: both rows are inside; px0 even, w even: span is even and the pairs are whole
    md = span_mode(im.y, im.pitch_y, whole);
    md_uv = span_mode(im.uv, im.pitch_uv, whole);
    p = (unsigned char*)im.y + (size_t)py0 * im.pitch_y + px0;
    pc = (unsigned char*)im.uv + (size_t)(py0 >> 1) * im.pitch_uv + px0;
    if (take) {
      span_load<4>(p, w, md, span);
      span_load<4>(p + im.pitch_y, w1, md, span);
      span_load<4>(pc, wc, md_uv, span);
    }
  }

  if (mode == 0) {
    // 3. level 1, the sums of 2 x 2 pixels; a pixel outside the frame counts 0.  BGR: the two rows of a cell belong to lanes l and l ^ 4
    // of one wave, and the even row writes.  NV12: the thread has both rows, and a chroma pair is its own cell.
    const int at = (ly0 >> 1) * 32 + (lx0 >> 1);
    if constexpr (R == 1) {
#pragma unroll
      for (int i = 0; i < MCG_ANON_SPAN / 2; ++i)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          int v = (int)(span_byte(w, 6 * i + ch) + span_byte(w, 6 * i + 3 + ch));
          v += __shfl_xor(v, 4);
          if (!(ly0 & 1)) pyr[ch][at + i] = v;
        }
    } else if (ly0 < MCG_ANON_TILE) {
#pragma unroll
      for (int i = 0; i < MCG_ANON_SPAN / 2; ++i) {
        pyr[0][at + i] = (int)(span_byte(w, 2 * i) + span_byte(w, 2 * i + 1) + span_byte(w1, 2 * i) + span_byte(w1, 2 * i + 1));
        pyr[1][at + i] = (int)span_byte(wc, 2 * i);
        pyr[2][at + i] = (int)span_byte(wc, 2 * i + 1);
      }
    }
    __syncthreads();
    // 4. folded upward, no further than the largest shift a row of this tile has.  Consecutive threads read consecutive 8-byte pairs of a
    // row (ds_read_b64: no two lanes of a group on one bank) and write consecutive words.
    const int top = 31 - __clz(used);
    for (int s = 2; s <= top; ++s) {
      const int side = MCG_ANON_TILE >> s, cells = side * side;
      for (int i = t; i < 3 * cells; i += 256) {
        const int ch = i / cells, e = i - ch * cells, y = e >> (6 - s), x = e & (side - 1);
        const int* src = &pyr[ch][anon_level(s - 1) + 4 * y * side + 2 * x];
        const int2 a = *(const int2*)src, b = *(const int2*)(src + 2 * side);
        pyr[ch][anon_level(s) + e] = a.x + a.y + b.x + b.y;
      }
      __syncthreads();
    }
    // 5. the levels that are read become means, (sum + (count >> 1)) / count over the cell's pixels inside the frame: at most 255 * 4096 + 2048
    const int words = anon_level(top + 1);
    for (int i = t; i < 3 * words; i += 256) {
      const int ch = i / words, e = i - ch * words;
      int s = 1;
      while (e >= anon_level(s + 1)) ++s;
      if (!((used >> s) & 1)) continue;
      const int idx = e - anon_level(s), gx = tx0 + ((idx & ((MCG_ANON_TILE >> s) - 1)) << s), gy = ty0 + ((idx >> (6 - s)) << s);
      const int cw = min(gx + (1 << s), im.w) - gx, chh = min(gy + (1 << s), im.h) - gy;
      if (cw <= 0 || chh <= 0) continue;                          // a cell of the tile that lies outside the frame
      const int count = (R == 2 && ch > 0) ? (cw * chh) >> 2 : cw * chh;   // NV12: w, h and the cell are even, a pair stands for four pixels
      pyr[ch][e] = (pyr[ch][e] + (count >> 1)) / count;
    }
    __syncthreads();                                              // the one barrier between the block's last read of the frame and its first write
  }
  if (!owner || !mine) return;                                    // no covered pixel in this span: it is not written

  // 6. the covered pixels take their value, and the span goes back
  const unsigned col[3] = {c0, c1, c2};
  const int row_at = ly0 & (MCG_ANON_TILE - 1);
  if constexpr (R == 1) {
#pragma unroll
    for (int j = 0; j < MCG_ANON_SPAN; ++j) {
      const int s = sh[0][j];
      if (s) {
        const int e = anon_level(s) + ((row_at >> s) << (6 - s)) + ((lx0 + j) >> s);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) span_set_byte(w, 3 * j + ch, mode ? col[ch] : (unsigned)pyr[ch][e]);
      }
    }
    span_store<12>(p, w, md, 3 * span);
  } else {
#pragma unroll
    for (int j = 0; j < MCG_ANON_SPAN; ++j) {
      const int s0 = sh[0][j], s1 = sh[1][j];
      if (s0) span_set_byte(w, j, mode ? c0 : (unsigned)pyr[0][anon_level(s0) + ((row_at >> s0) << (6 - s0)) + ((lx0 + j) >> s0)]);
      if (s1) span_set_byte(w1, j, mode ? c0 : (unsigned)pyr[0][anon_level(s1) + ((row_at >> s1) << (6 - s1)) + ((lx0 + j) >> s1)]);
    }
#pragma unroll
    for (int j = 0; j < MCG_ANON_SPAN; j += 2) {
      const int s = max(max(sh[0][j], sh[0][j + 1]), max(sh[1][j], sh[1][j + 1]));   // the pair's shift: the largest of its four
      if (s) {
        const int e = anon_level(s) + ((row_at >> s) << (6 - s)) + ((lx0 + j) >> s);
        span_set_byte(wc, j, mode ? c1 : (unsigned)pyr[1][e]);
        span_set_byte(wc, j + 1, mode ? c2 : (unsigned)pyr[2][e]);
      }
    }
    span_store<4>(p, w, md, span);
    span_store<4>(p + im.pitch_y, w1, md, span);
    span_store<4>(pc, wc, md_uv, span);
  }
}

template <class Target>
static int anonymize_heads(const char* what, const char* what_plan, mcg_stream stream, const typename Target::Image* images_dev, int num_images,
                           int max_h, int max_w, const float* boxes_dev, const int32_t* image_of_dev, int n, double expand, int shape, int cell_shift,
                           int blocks, int mode, const unsigned char* color, mcg_anon_desc* plan_out_dev, int32_t* flags_dev) {
  MCG_CHECK_ARG(n >= 0 && n <= 65536, "%s: at most 65536 rows per call (got %d)", what, n);
  MCG_CHECK_ARG(images_dev && (n == 0 || (boxes_dev && image_of_dev && plan_out_dev)) && (mode != 1 || color), "%s: null pointer", what);
  MCG_CHECK_ARG(num_images >= 1 && num_images <= 65535, "%s: 1 .. 65535 images (got %d)", what, num_images);
  MCG_CHECK_ARG(max_h >= 1 && max_h <= MCG_DRAW_SIDE && max_w >= 1 && max_w <= MCG_DRAW_SIDE, "%s: frames of 1 .. 8192 pixels a side (got max %dx%d)",
                what, max_h, max_w);
  MCG_CHECK_ARG(expand >= 0.0 && expand <= 4.0, "%s: expand in 0 .. 4 (got %g)", what, expand);   // a NaN fails
  MCG_CHECK_ARG((shape == 0 || shape == 1) && (mode == 0 || mode == 1), "%s: shape 0 (box) or 1 (ellipse), mode 0 (mosaic) or 1 (fill) (got %d, %d)", what,
                shape, mode);
  MCG_CHECK_ARG(cell_shift >= 0 && cell_shift <= 6, "%s: cell_shift 0 (automatic) or 1 .. 6 (got %d)", what, cell_shift);
  MCG_CHECK_ARG(cell_shift != 0 || (blocks >= 1 && blocks <= 64), "%s: blocks in 1 .. 64 (got %d)", what, blocks);
  if (n == 0) return MCG_OK;
  hipLaunchKernelGGL(anonymize_plan_kernel<Target>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, images_dev, num_images, max_h, max_w,
                     boxes_dev, image_of_dev, n, expand, shape, cell_shift, blocks, plan_out_dev, flags_dev);
  MCG_CHECK_LAUNCH(what_plan);
  const int tiles_x = (max_w + MCG_ANON_TILE - 1) / MCG_ANON_TILE, tiles_y = (max_h + MCG_ANON_TILE - 1) / MCG_ANON_TILE;
  const unsigned c0 = color ? color[0] : 0, c1 = color ? color[1] : 0, c2 = color ? color[2] : 0;
  hipLaunchKernelGGL(anonymize_render_kernel<Target>, dim3(tiles_x * tiles_y, num_images), dim3(256), 0, (hipStream_t)stream, images_dev, tiles_x,
                     max_h, max_w, plan_out_dev, n, mode, c0, c1, c2);
  MCG_CHECK_LAUNCH(what);
  return MCG_OK;
}

extern "C" int mcg_anonymize_heads(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                                   const int32_t* image_of_dev, int n, double expand, int shape, int cell_shift, int blocks, int mode,
                                   const unsigned char* color, mcg_anon_desc* plan_out_dev, int32_t* flags_dev) {
  return anonymize_heads<PackedTarget>("mcg_anonymize_heads", "mcg_anonymize_heads (plan)", s, images_dev, num_images, max_h, max_w, boxes_dev,
                                       image_of_dev, n, expand, shape, cell_shift, blocks, mode, color, plan_out_dev, flags_dev);
}

extern "C" int mcg_anonymize_heads_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w,
                                        const float* boxes_dev, const int32_t* image_of_dev, int n, double expand, int shape, int cell_shift, int blocks,
                                        int mode, const unsigned char* yuv, mcg_anon_desc* plan_out_dev, int32_t* flags_dev) {
  return anonymize_heads<Nv12Target>("mcg_anonymize_heads_nv12", "mcg_anonymize_heads_nv12 (plan)", s, images_dev, num_images, max_h, max_w, boxes_dev,
                                     image_of_dev, n, expand, shape, cell_shift, blocks, mode, yuv, plan_out_dev, flags_dev);
}
