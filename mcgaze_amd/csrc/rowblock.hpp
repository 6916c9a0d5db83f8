// What the decoder's row-block kernels (chain.hpp, attn_block.hpp, attn_block_x3.hpp) and its LayerNorm sites (decoder.hip: ln_kernel and the
// DynamicConv kernels) share, each piece stated once:
//   * the LayerNorm of one row, with its fused multiply-adds spelled out -- the fused kernels must give the bits of the launch sequences they
//     replace, and under the unit's default contraction WHICH multiply-adds fuse is the compiler's choice and moves with the surrounding code;
//   * the row-block linear "32 token rows in LDS . W^T (+ bias) -> f32 slab", per arithmetic: Ops16<T> (bf16 / fp16 storage, one MFMA per
//     product) and OpsX3 (f32 storage, operands split into fp16 high / low parts, three MFMAs per product).
#pragma once
#include "igemm_dma.hpp"

// ------------------------------------------------------------------------------------------------
// LayerNorm (eps = 1e-5, biased variance) of a row of width D held by one wave, every operation named: nothing here is left to contraction.
//   deviation  d = fma(-1/D, sum, v)          (for D = 64 / 256 the product is exact: the same value as v - sum / D)
//   rstd       1 / sqrt(fma(sum of d^2, 1/D, eps))    IEEE square root and division
//   output     fma(d * rstd, gamma, beta)
__device__ __forceinline__ float ln_dev(float v, float sum, float invD) { return __builtin_fmaf(-invD, sum, v); }
__device__ __forceinline__ float ln_rstd(float sqsum, float invD) { return 1.0f / sqrtf(__builtin_fmaf(sqsum, invD, 1e-5f)); }
__device__ __forceinline__ float ln_affine(float d, float rstd, float g, float b) {
#pragma clang fp contract(off)
  return __builtin_fmaf(d * rstd, g, b);
}

// How a lane sums the squares of its four deviations.  LN_SQ_FMA is ln_kernel's (q = d0 d0, then q = fma(d, d, q) in order) and what the
// f16x3 fused kernels run, so those agree with the launch sequence by construction.  The other two state what the compiler had chosen for
// the kernels that use them and keep those kernels' bits: the 16-bit fused kernels add the four ROUNDED squares in order (their output is
// rounded to 16 bits, which is what has hidden the last-place difference from ln_kernel), and the DynamicConv tails, which nothing
// cross-checks bit for bit, start the fma chain at d1.
enum LnSq { LN_SQ_FMA, LN_SQ_ROUNDED, LN_SQ_FMA_FROM_D1 };

// The 4 values this lane owns (columns 4 lane .. 4 lane + 3) of a 256-wide row -> normalised, affine, [ReLU]; g / b: the lane's gamma / beta
template <LnSq SQ>
__device__ __forceinline__ void ln256_row(float (&v)[4], const float4& g, const float4& b, bool relu) {
#pragma clang fp contract(off)
  constexpr float invD = 1.0f / 256;
  const float sum = wave_sum(v[0] + v[1] + v[2] + v[3]);
  const float d[4] = {ln_dev(v[0], sum, invD), ln_dev(v[1], sum, invD), ln_dev(v[2], sum, invD), ln_dev(v[3], sum, invD)};
  float q;
  if constexpr (SQ == LN_SQ_FMA) q = __builtin_fmaf(d[3], d[3], __builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0])));
  else if constexpr (SQ == LN_SQ_ROUNDED) q = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
  else q = __builtin_fmaf(d[3], d[3], __builtin_fmaf(d[2], d[2], __builtin_fmaf(d[0], d[0], d[1] * d[1])));
  const float rstd = ln_rstd(wave_sum(q), invD);
  const float gg[4] = {g.x, g.y, g.z, g.w}, bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = ln_affine(d[e], rstd, gg[e], bb[e]);
    v[e] = relu ? fmaxf(t, 0.f) : t;
  }
}

// DynamicConv's 64-wide form, lane = feature: this lane's value -> ReLU(LayerNorm).  Its sum of squares is not wave_sum(d * d): the first
// butterfly step had been contracted across the call, fma(d, d, the neighbour's rounded d * d), and that is what these kernels' bits are.
__device__ __forceinline__ float ln64_relu(float v, float g, float b) {
#pragma clang fp contract(off)
  constexpr float invD = 1.0f / 64;
  const float d = ln_dev(v, wave_sum(v), invD);
  const float q = wave_sum_rest(__builtin_fmaf(d, d, dpp_mov<0xB1>(d * d, 0.f)));
  return fmaxf(ln_affine(d, ln_rstd(q, invD), g, b), 0.f);
}

// ------------------------------------------------------------------------------------------------
// Row-block linear.  A workgroup of 4 waves holds RB_ROWS token rows of RB_D channels in LDS as the MFMA A operand, 16-byte chunks
// XOR-swizzled by the row (an unswizzled row stride would put all 32 rows of an A fragment on one bank group).  Wave w computes output
// columns [64 w, 64 w + 64) -- two 32x32 tiles -- over K = 256 in 16 steps, in the K order (and, split, the term order) of the igemm kernels,
// with the B fragments of both tiles and all 16 steps in registers, fetched straight from a fragment-major copy of W (1 KiB per wave load).
// An operand policy states, once per arithmetic:
//   Quad                four consecutive stored channels          ES / ROWB        bytes per element / per LDS row
//   swz(row, chunk)     byte offset of a 16-byte chunk of a row   stage_rows       global rows -> LDS (rows from `valid` on are zero)
//   quad / unquad       four f32 <-> Quad                         round_stored     f32 -> storage precision -> f32
//   park                a Quad of channels c .. c + 3 of a row -> its place in the A operand
//   Bfr, load_b(W, tile0)   the fragments of column tiles tile0, tile0 + 1         mma2    acc[2] = rows . those two tiles
//   kLnSq               the LayerNorm's sum-of-squares form (above)
constexpr int RB_D = 256, RB_ROWS = 32;

template <typename T>   // bf16_t or f16_t: W is [column tile][K-step 16][lane 64][8] (include/mcgaze_hip.h MCG_SW_*_WF)
struct Ops16 {
  typedef T Elem;
  typedef uint2 Quad;
  static constexpr int ES = 2, ROWB = RB_D * ES;
  static constexpr LnSq kLnSq = LN_SQ_ROUNDED;
  struct Bfr { uint4 f[2][16]; };   // [column tile][K-step]: 128 VGPRs
  __device__ static __forceinline__ int swz(int row, int chunk) { return row * ROWB + ((chunk ^ (row & 31)) << 4); }   // chunk = 8 channels
  __device__ static __forceinline__ int quad_off(int row, int c) { return swz(row, c >> 3) + (c & 7) * 2; }
  __device__ static __forceinline__ void stage_rows(char* s, const void* x, int valid, int tid) {
    for (int idx = tid; idx < RB_ROWS * 32; idx += 256) {
      const int r = idx >> 5, c = idx & 31;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r < valid) v = *(const uint4*)((const char*)x + (size_t)r * ROWB + c * 16);
      *(uint4*)(s + swz(r, c)) = v;
    }
  }
  __device__ static __forceinline__ Quad quad(const float (&v)[4]) { return make_uint2(H16<T>::pack2(v[0], v[1]), H16<T>::pack2(v[2], v[3])); }
  __device__ static __forceinline__ void unquad(const Quad& q, float (&v)[4]) {
    v[0] = H16<T>::lo(q.x); v[1] = H16<T>::hi(q.x); v[2] = H16<T>::lo(q.y); v[3] = H16<T>::hi(q.y);
  }
  __device__ static __forceinline__ void round_stored(float (&v)[4]) { unquad(quad(v), v); }
  __device__ static __forceinline__ void park(char* base, int row, int c, const Quad& q) { *(uint2*)(base + quad_off(row, c)) = q; }
  __device__ static __forceinline__ void load_b(Bfr& b, const void* W, int tile0, int lane) {
    const char* wb = (const char*)W + ((size_t)tile0 * 16 * 64 + lane) * 16;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      b.f[0][ks] = *(const uint4*)(wb + ks * 1024);
      b.f[1][ks] = *(const uint4*)(wb + 16 * 1024 + ks * 1024);
    }
  }
  __device__ static __forceinline__ void mma2(const char* A, const Bfr& b, f32x16 (&acc)[2], int lane) {
    const int arow = lane & 31, half = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const uint4 a = *(const uint4*)(A + swz(arow, 2 * ks + half));
      Mma<T>::run(acc[0], a, b.f[0][ks]);
      Mma<T>::run(acc[1], a, b.f[1][ks]);
    }
  }
};

// f16x3 (MCG_F16X3): f32 storage; a row sits in LDS SPLIT into fp16 high / low parts, split once when it is written, chunk = K-step * 4 +
// lane half * 2 + (0 high, 1 low): 64 chunks of 16 bytes per row.  W is the split fragment-major copy (packing.py::frag_major_split:
// [column tile][K-step 16][high, low][lane 64][8]); a step's fragments are 256 VGPRs -- one wave per SIMD, the 512-register file is the wave's.
struct OpsX3 {
  typedef float Elem;
  typedef float4 Quad;
  static constexpr int ES = 4, ROWB = RB_D * ES;
  static constexpr LnSq kLnSq = LN_SQ_FMA;
  struct Bfr { uint4 f[2][16][2]; };   // [column tile][K-step][high, low]
  __device__ static __forceinline__ int swz(int row, int chunk) { return row * ROWB + ((chunk ^ (row & 31)) << 4); }
  __device__ static __forceinline__ void stage_rows(char* s, const void* x, int valid, int tid) {
    for (int idx = tid; idx < RB_ROWS * 64; idx += 256) {
      const int r = idx >> 6, c = (idx & 63) * 4;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < valid) t = *(const float4*)((const float*)x + (size_t)r * RB_D + c);
      park(s, r, c, t);
    }
  }
  __device__ static __forceinline__ Quad quad(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }
  __device__ static __forceinline__ void unquad(const Quad& q, float (&v)[4]) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
  __device__ static __forceinline__ void round_stored(float (&)[4]) {}
  // 8 bytes of high parts and 8 bytes of low parts at their place
  __device__ static __forceinline__ void park(char* base, int row, int c, const Quad& q) {
    uint32_t h0, l0, h1, l1;
    split_pair(q.x, q.y, h0, l0);
    split_pair(q.z, q.w, h1, l1);
    const int chunk = (c >> 4) * 4 + ((c >> 3) & 1) * 2, pos = ((c >> 2) & 1) * 8;
    *(uint2*)(base + swz(row, chunk) + pos) = make_uint2(h0, h1);
    *(uint2*)(base + swz(row, chunk + 1) + pos) = make_uint2(l0, l1);
  }
  __device__ static __forceinline__ void load_b(Bfr& b, const void* W, int tile0, int lane) {
    const char* wb = (const char*)W + ((size_t)tile0 * 16 * 2 * 64 + lane) * 16;
    // opaque to loop-invariant code motion: left alone, the compiler hoists the 64-bit address of every 4 KiB group of every call site out of
    // attn_block_x3_kernel's loops and keeps them all alive -- 263 spilled registers of nothing but addresses
    asm volatile("" : "+v"(wb));
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        b.f[j][ks][0] = *(const uint4*)(wb + ((size_t)(j * 16 + ks) * 2) * 1024);
        b.f[j][ks][1] = *(const uint4*)(wb + ((size_t)(j * 16 + ks) * 2 + 1) * 1024);
      }
  }
  __device__ static __forceinline__ void mma2(const char* A, const Bfr& b, f32x16 (&acc)[2], int lane) {   // lo.hi + hi.lo + hi.hi per K-step
    const int arow = lane & 31, half = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const bf16x8 ah = __builtin_bit_cast(bf16x8, *(const uint4*)(A + swz(arow, ks * 4 + half * 2)));
      const bf16x8 al = __builtin_bit_cast(bf16x8, *(const uint4*)(A + swz(arow, ks * 4 + half * 2 + 1)));
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = x3_mfma(al, __builtin_bit_cast(bf16x8, b.f[j][ks][0]), acc[j]);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = x3_mfma(ah, __builtin_bit_cast(bf16x8, b.f[j][ks][1]), acc[j]);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = x3_mfma(ah, __builtin_bit_cast(bf16x8, b.f[j][ks][0]), acc[j]);
    }
  }
};

// acc (+ bias, null: none) of the wave's two tiles -> the f32 slab [RB_ROWS][RB_D] the LayerNorm phase reads
__device__ __forceinline__ void rb_slab(float* s_t, const f32x16 (&acc)[2], const float* __restrict__ bias, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wave * 64 + j * 32 + (lane & 31);
    const float bb = bias ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s_t[mfma32_row(r, lane) * RB_D + col] = acc[j][r] + bb;
  }
}
