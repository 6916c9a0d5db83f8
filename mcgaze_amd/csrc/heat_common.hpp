// What heat.hip (gaze heat map) and surface.hip (surface heat map) share: the clear and the per-cell update launches of an accumulation, the
// blend, and how a thread that knows the levels of its 16 pixels (NV12: 16 x 2 and their 8 chroma pairs) reads, blends and writes them.  The
// arithmetic is stated once, in include/mcgaze_hip.h ("gaze heat map").  The kernels are static: each unit that includes this launches its own.
#pragma once
#include "draw_common.hpp"   // the bounds, PackedTarget / Nv12Target, the span accesses

#define MCG_HEAT_MAX_CELLS (1 << 24)
#define MCG_HEAT_SPAN 16                    // pixels of a row a thread owns

// ---------------------------------------------------------------- accumulate: the first and the last launch (C grids of `cells` cells)
static __global__ __launch_bounds__(256) void heat_clear_kernel(int32_t* __restrict__ work, int cells, int32_t* __restrict__ peak, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < cells) work[i] = 0;
  if (i < C) peak[i] = 0;
}

static __global__ __launch_bounds__(256) void heat_update_kernel(int32_t* __restrict__ heat, const int32_t* __restrict__ work, int32_t* __restrict__ peak,
                                                          int cells, int decay_shift) {
  const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  int v = 0;
  if (i < cells) {
    const size_t at = (size_t)c * cells + i;
    int h = max(heat[at], 0);                                     // a negative value is taken as 0
    if (decay_shift > 0) h -= h >> decay_shift;
    v = (int)min((long long)h + work[at], 2147483647LL);
    heat[at] = v;
  }
  // the block's maximum: an xor-shuffle reduction inside each wave of 64, the four waves' maxima through four LDS words
  __shared__ int top[4];
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) top[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int m = max(max(top[0], top[1]), max(top[2], top[3]));
    if (m > 0) atomicMax(peak + c, m);                            // peak was cleared by the first launch; a maximum commutes
  }
}

// ---------------------------------------------------------------- render: a thread's pixels
// (src (255 - a) + col a + 127) / 255: at most 255 * 255 + 127, the division a multiply and a shift
__device__ __forceinline__ unsigned heat_blend(unsigned src, unsigned col, unsigned a) { return (src * (255u - a) + col * a + 127u) / 255u; }

// min(255, a / full) for a >= 0 and full >= 1, the quotient found bit by bit: eight multiplications in place of a 64-bit division
__device__ __forceinline__ int heat_level(long long a, long long full) {
  int L = 0;
  if (a >= full) {
#pragma unroll
    for (int b = 128; b; b >>= 1)
      if ((long long)(L | b) * full <= a) L |= b;
  }
  return L;
}

// The thread's pixels (px0 .. px0 + 15, py0 .. py0 + R - 1), px0 < im.w and py0 < im.h, whose levels it knows and at least one of which
// reaches min_level: read, blended with `colour` (the 256 entries of the ramp, in LDS) and written, in 16-byte accesses where the plane's
// address and pitch allow, in 4-byte accesses where only those are aligned, byte by byte at the right edge and for any other pitch.
template <class Target>
__device__ __forceinline__ void heat_blend_span(const typename Target::Image& im, int px0, int py0, const int (&level)[Target::CELL][MCG_HEAT_SPAN],
                                                const unsigned* colour, int min_level) {
  constexpr int R = Target::CELL;
  const int span = min(MCG_HEAT_SPAN, im.w - px0);                // pixels of the thread inside the picture
  const bool whole = span == MCG_HEAT_SPAN;
  if constexpr (R == 1) {
    const int mode = span_mode(im.src, im.pitch, whole);
    unsigned char* p = (unsigned char*)im.src + (size_t)py0 * im.pitch + (size_t)px0 * 3;
    unsigned w[12];
    span_load<12>(p, w, mode, 3 * span);
#pragma unroll
    for (int j = 0; j < MCG_HEAT_SPAN; ++j) {
      const int L = level[0][j];
      if (L >= min_level) {
        const unsigned c = colour[L], a = c >> 24;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) span_set_byte(w, 3 * j + ch, heat_blend(span_byte(w, 3 * j + ch), (c >> (8 * ch)) & 255u, a));
      }
    }
    span_store<12>(p, w, mode, 3 * span);
  } else {
    const int mode_y = span_mode(im.y, im.pitch_y, whole), mode_uv = span_mode(im.uv, im.pitch_uv, whole);
    // py0 even and < h, h even: both rows are inside; px0 even, w even: span is even and the pairs are whole
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      unsigned char* p = (unsigned char*)im.y + (size_t)(py0 + r) * im.pitch_y + px0;
      unsigned w[4];
      span_load<4>(p, w, mode_y, span);
#pragma unroll
      for (int j = 0; j < MCG_HEAT_SPAN; ++j) {
        const int L = level[r][j];
        if (L >= min_level) {
          const unsigned c = colour[L];
          span_set_byte(w, j, heat_blend(span_byte(w, j), c & 255u, c >> 24));
        }
      }
      span_store<4>(p, w, mode_y, span);
    }
    unsigned char* q = (unsigned char*)im.uv + (size_t)(py0 >> 1) * im.pitch_uv + px0;
    unsigned w[4];
    span_load<4>(q, w, mode_uv, span);
#pragma unroll
    for (int j = 0; j < MCG_HEAT_SPAN; j += 2) {
      const int L = max(max(level[0][j], level[0][j + 1]), max(level[1][j], level[1][j + 1]));   // the pair's level: the highest of its four
      if (L >= min_level) {
        const unsigned c = colour[L], a = c >> 24;
        span_set_byte(w, j, heat_blend(span_byte(w, j), (c >> 8) & 255u, a));
        span_set_byte(w, j + 1, heat_blend(span_byte(w, j + 1), (c >> 16) & 255u, a));
      }
    }
    span_store<4>(q, w, mode_uv, span);
  }
}
