// Attention block of one decoder stage as ONE launch in the MCG_F16X3 arithmetic (round 6; attn_block.hpp is the bf16 engine's): the
// spatial pass and the temporal pass of gaze_stqi_head.py:148-166 -- each "in_proj -> 8-head softmax attention -> out_proj + residual ->
// LayerNorm", with the SAME weights and LayerNorm in both passes -- for one clip per workgroup.  Replaces six launches per stage
// (2 x [in_proj igemm_dma, attn_core_kernel, mlp_chain_kernel<OpsX3> with one step]) of a few microseconds of work each.
//
// A clip's 3 T token rows (row = (frame, clue), frame-major) are contiguous and closed under both passes; with 3 T <= 32 they are one
// MFMA row tile and the whole block runs out of LDS (128 KiB, one workgroup of four waves per CU, one wave per SIMD: the 512-register file
// is the wave's -- a linear step's B fragments, high and low, are 256 of them):
//   s_x    32 rows x 1 KiB: the A operand of the next linear, SPLIT into fp16 high / low 16-byte chunks when it is written (rowblock.hpp: OpsX3's
//          layout: chunk = K-step * 4 + lane half * 2 + (0 high, 1 low), XOR-swizzled by the row) -- the pass's input rows for in_proj, then
//          (in_proj done, nobody reads the rows any more: the residual comes from global memory / registers) the attention output for out_proj
//   s_qkv  [32][768] f32 (q | k | v); a head's 32 floats are stored with their eight 16-byte chunks ROTATED by the head index, so that the
//          eight (row, head) threads of a quarter-wave read eight different bank groups (unrotated, a 128-byte head stride puts all of them
//          on the same four banks); the out-projection's f32 slab aliases its first 32 KiB
// Linears are the row-block linear of rowblock.hpp (OpsX3, as in chain.hpp): wave w owns 64 output columns, K = 256 in 16 steps of lo.hi + hi.lo + hi.hi, B fragments straight from the
// fragment-major SPLIT copy of the weights (packing.py::frag_major_split; 1 KiB per wave load), the next sub-step's in flight while this
// one's results are written.  The attention core is attend_row_head -- the device function attn_core_kernel runs -- and the LayerNorm is ln256_row in
// ln_kernel's form; every f32 rounding point of the six launches is kept (qkv, attention output, projection + bias,
// + residual), so the block is BIT-IDENTICAL to the sequence it replaces (tests/test_gpu_kernels.py::test_attn_block_x3_matches_unfused_bitwise).
// The pass-0 output rows stay in the registers of the lanes that normalised them (wave -> 8 rows, lane -> 4 columns): they ARE pass 1's residual.
#pragma once
#include "attn_block.hpp"

constexpr int kAttnBlockX3Lds = RB_ROWS * OpsX3::ROWB + RB_ROWS * 3 * RB_D * 4;   // 32 KiB + 96 KiB

__global__ __launch_bounds__(256, 1) void attn_block_x3_kernel(const AttnBlockParams p) {
  typedef OpsX3 Ops;
  constexpr int D = RB_D, ROWS = RB_ROWS, ROWB = Ops::ROWB, QKV_LD = 3 * D;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const s_x = smem;
  float* const s_qkv = (float*)(smem + ROWS * ROWB);
  float* const s_t = s_qkv;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int T_b = p.T;
  size_t m0 = (size_t)blockIdx.x * (3 * p.T);
  bool bad = false;
  if (p.clip_start) {                                         // ragged batch: this clip's span from the table (attn_block.hpp: clip_span)
    const ClipSpan cs = clip_span(p.clip_start, blockIdx.x, p.num_frames, p.T);
    T_b = cs.len; m0 = (size_t)cs.first * 3; bad = cs.bad;
  }
  const int rows = 3 * T_b;                                   // <= 32 (checked by the launcher; clip_span clamps)
  const float* const X = (const float*)p.x;
  Ops::stage_rows(s_x, X + m0 * D, rows, tid);                // token rows -> LDS, split (padding rows are zero; never stored)
  const int arow = lane & 31;
  Ops::Bfr bfr;
  Ops::load_b(bfr, p.w_in, wave * 2, lane);
  __syncthreads();
  float keep[8][4];                                           // pass 0's output rows of this lane: pass 1's residual
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) keep[a][e] = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    // ---- q | k | v = x . Win^T + b (f32, what the unfused path stores): three sub-steps of 256 columns = 8 heads; wave -> heads 2 w, 2 w + 1
#pragma unroll 1
    for (int u = 0; u < 3; ++u) {
      f32x16 acc[2];
      Ops::mma2(s_x, bfr, acc, lane);
      if (u < 2) Ops::load_b(bfr, p.w_in, (u + 1) * 8 + wave * 2, lane);   // (the out-projection's fragments are NOT fetched here: 256 registers live
                                                                           //  across the attention core put 310 of them into scratch; they are issued right behind it)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int head = wave * 2 + j;
        const float bb = p.b_in[u * D + head * 32 + arow];
        // element d = arow of the head: chunk (d >> 2) rotated by the head index
        float* dst = s_qkv + u * D + head * 32 + ((((arow >> 2) + head) & 7) << 2) + (arow & 3);
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[mfma32_row(r, lane) * QKV_LD] = acc[j][r] + bb;
      }
    }
    __syncthreads();   // qkv complete; every wave is done reading the input rows in s_x
    // ---- attention core: thread = (query row, head) (attend_row_head); rows * 8 <= 256 pairs; its output, split, becomes the next A operand
    {
      const int L = pass == 0 ? 3 : T_b;
      const int i = tid >> 3, h = tid & 7;
      __attribute__((aligned(16))) float o[32];
      if (i < rows) {
        const int kbase = pass == 0 ? (i / 3) * 3 : i % 3, kstep = pass == 0 ? 1 : 3;
        attend_row_head<float>(s_qkv + i * QKV_LD + h * 32,
                               [&](int j) { return (const float*)(s_qkv + (kbase + j * kstep) * QKV_LD + D + h * 32); },
                               [&](int j) { return (const float*)(s_qkv + (kbase + j * kstep) * QKV_LD + 2 * D + h * 32); }, L, p.scale, o,
                               [&](const float* base, int c) { return *(const uint4*)(base + (((c + h) & 7) << 2)); });
      } else {
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] = 0.f;
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) Ops::park(s_x, i, h * 32 + 4 * c, make_float4(o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]));
    }
    Ops::load_b(bfr, p.w_out, wave * 2, lane);
    __syncthreads();   // attention rows complete, s_qkv consumed (s_t aliases it)
    // ---- out-projection + bias (f32 slab), then + residual -> LayerNorm (chain.hpp's step)
    {
      f32x16 acc[2];
      Ops::mma2(s_x, bfr, acc, lane);
      if (pass == 0) Ops::load_b(bfr, p.w_in, wave * 2, lane);
      rb_slab(s_t, acc, p.b_out, wave, lane);
    }
    __syncthreads();   // the slab is complete; every wave is done reading the attention rows in s_x
    const int c0 = lane * 4;
    const float4 g4 = *(const float4*)(p.g + c0), b4 = *(const float4*)(p.b + c0);
#pragma unroll
    for (int rr8 = 0; rr8 < 8; ++rr8) {
      const int r = wave * 8 + rr8;
      const float4 t4 = *(const float4*)(s_t + r * D + c0);
      float v[4] = {t4.x, t4.y, t4.z, t4.w};
      if (r < rows) {  // residual = this pass's input row (the mmcv wrapper adds the identity, transformer.py MultiheadAttention)
        if (pass == 0) {
          const float4 rr = *(const float4*)(X + (m0 + r) * D + c0);
          v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += keep[rr8][e];
        }
      }
      ln256_row<Ops::kLnSq>(v, g4, b4, false);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = r < rows ? v[e] : 0.f;   // padding rows stay zero
      Ops::park(s_x, r, c0, Ops::quad(v));
#pragma unroll
      for (int e = 0; e < 4; ++e) keep[rr8][e] = v[e];
      if (pass == 1 && r < rows) *(float4*)((float*)p.y + (m0 + r) * D + c0) = Ops::quad(v);
    }
    __syncthreads();
  }
  if (bad) {   // a clip the table guard clamped: its rows become NaN, in a pass of its own behind the last barrier.  (It was put here when a
               // select at the store above changed how the compiler contracted the LayerNorm's multiply-adds; ln256_row now names every
               // fused operation, so that no longer follows -- the pass stays where it is all the same.)
    const float nan = __builtin_nanf("");
    for (int idx = threadIdx.x; idx < rows * 64; idx += 256) *(float4*)((float*)p.y + (m0 + (idx >> 6)) * D + (idx & 63) * 4) = make_float4(nan, nan, nan, nan);
  }
}

// Both passes of a stage's attention as one launch; dt: MCG_BF16 / MCG_F16 (attn_block_kernel) or MCG_F16X3 (attn_block_x3_kernel)
static inline int launch_attn_block(hipStream_t s, const AttnBlockParams& p, mcg_dtype dt) {
  if (dt == MCG_F16X3) {
    if (kernel_ready<attn_block_x3_kernel>(kAttnBlockX3Lds)) { mcg_set_error("attn_block: cannot raise the kernel's dynamic LDS limit"); return MCG_ERR_HIP; }
    hipLaunchKernelGGL(attn_block_x3_kernel, dim3(p.num_clips), dim3(256), kAttnBlockX3Lds, s, p);
  } else if (mcg_is16(dt)) {
    dispatch_elem16(dt, [&](auto e) { hipLaunchKernelGGL(attn_block_kernel<decltype(e)>, dim3(p.num_clips), dim3(256), 0, s, p); });
  } else { mcg_set_error("attn_block: unsupported dtype %d", (int)dt); return MCG_ERR_UNSUPPORTED; }
  MCG_CHECK_LAUNCH("attn_block");
  return MCG_OK;
}
