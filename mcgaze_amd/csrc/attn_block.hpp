// Attention block of one decoder stage as ONE launch (bf16 engine): the spatial pass and the temporal pass of
// gaze_stqi_head.py:148-166 -- each "in_proj -> 8-head softmax attention -> out_proj + residual -> LayerNorm", with the SAME weights
// and LayerNorm in both passes -- for one clip per workgroup.  Replaces six launches per stage (2 x [in_proj igemm, attn_core_kernel,
// out_proj + LN chain]) whose GPU work is a few microseconds each.
//
// A clip's 3 T token rows (row = (frame, clue), frame-major) are contiguous and closed under both passes: the spatial groups are
// the 3 clues of a frame, the temporal groups the T frames of a clue.  With 3 T <= 32 they are one MFMA row tile, so the whole
// block runs out of LDS:
//   s_a / s_b   token rows, bf16, 16-byte K-chunks XOR-swizzled by the row (A operand; ping-pong between the passes)
//   s_qkv       [32][768] bf16 row-major (q | k | v), aliased by the f32 slab of the out-projection
//   s_att       attention output rows (A operand)
// Linears are the row-block linear of rowblock.hpp (Ops16<T>, as in chain.hpp): wave w owns 64 output columns (two 32x32 tiles), K = 256
// in 16 MFMA steps, B fragments straight from a fragment-major copy of the weights, the next sub-step's fragments in flight while this
// one's results are written.  Rounding points and orders are those of the launches it replaces (qkv, attention output and the
// projection's output are rounded to bf16 where the unfused path stores them; K order of the igemm kernel; the attention core
// is the same device function; LayerNorm is ln256_row, with ln_kernel's lane -> column ownership), so the fused block reproduces the
// unfused sequence (tests/test_gpu_kernels.py::test_mlp_chain_matches_unfused_bitwise).
#pragma once
#include "rowblock.hpp"

// One (query row, head) of the 8-head / 32-dim attention: scores over the L keys of the row's group, softmax, weighted sum of the
// values.  One THREAD does the whole thing -- 32-term dot products as sequential fma chains, maximum first, then exp / sum /
// accumulate -- so there is no cross-lane reduction at all (the earlier (head, dim)-per-thread form spent its time in 32-lane
// butterflies: 5 LDS round trips per key with __shfl_xor).  Shared by attn_block_kernel (operands in LDS) and attn_core_kernel
// (operands in global memory), which therefore agree bit for bit.  key(j) / val(j) return a pointer to the 32 contiguous
// elements of key / value j for this head; out receives 32 elements.
// ld(base, c) loads 16-byte chunk c of the 32 elements at base: linear by default; attn_block_x3.hpp keeps a head's chunks rotated in LDS
// (bank conflicts) and passes its own -- where a value sits changes no arithmetic.
template <typename T, typename KeyF, typename ValF, typename LdF>
__device__ __forceinline__ void attend_row_head(const T* __restrict__ qp, KeyF key, ValF val, int L, float scale, T* __restrict__ out, LdF ld) {
  constexpr int EPC = Elem<T>::kPerChunk, HD = 32;
  float q[HD];
#pragma unroll
  for (int c = 0; c < HD / EPC; ++c) {
    float t[EPC];
    chunk_to_f32(ld(qp, c), t, (T*)nullptr);
#pragma unroll
    for (int e = 0; e < EPC; ++e) q[c * EPC + e] = t[e] * scale;
  }
  auto score = [&](int j) {
    const T* kp = key(j);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < HD / EPC; ++c) {
      float t[EPC];
      chunk_to_f32(ld(kp, c), t, (T*)nullptr);
#pragma unroll
      for (int e = 0; e < EPC; ++e) s = fmaf(q[c * EPC + e], t[e], s);
    }
    return s;
  };
  float m = -INFINITY;
  for (int j = 0; j < L; ++j) m = fmaxf(m, score(j));
  float l = 0.f, o[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) o[d] = 0.f;
  for (int j = 0; j < L; ++j) {
    const float pj = expf(score(j) - m);   // recomputed: the same bits as in the first sweep, and no L-sized register array
    l += pj;
    const T* vp = val(j);
#pragma unroll
    for (int c = 0; c < HD / EPC; ++c) {
      float t[EPC];
      chunk_to_f32(ld(vp, c), t, (T*)nullptr);
#pragma unroll
      for (int e = 0; e < EPC; ++e) o[c * EPC + e] = fmaf(pj, t[e], o[c * EPC + e]);
    }
  }
  const float inv = 1.0f / l;
#pragma unroll
  for (int c = 0; c < HD / EPC; ++c) {
    float t[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) t[e] = o[c * EPC + e] * inv;
    *(uint4*)(out + c * EPC) = f32_to_chunk(t, (T*)nullptr);
  }
}

template <typename T, typename KeyF, typename ValF>
__device__ __forceinline__ void attend_row_head(const T* __restrict__ qp, KeyF key, ValF val, int L, float scale, T* __restrict__ out) {
  attend_row_head<T>(qp, key, val, L, scale, out, [](const T* base, int c) { return *(const uint4*)(base + c * Elem<T>::kPerChunk); });
}

// Clips of different lengths in one batch (gaze_stqi_head.py:156-166 groups the temporal pass by clip; multiclue_gaze.py:77-78,119 fix
// ONE clip length per call): a device table clip_start[num_clips + 1] of frame indices, clip_start[0] = 0, strictly increasing,
// clip_start[num_clips] = num_frames; clip b holds frames [clip_start[b], clip_start[b + 1]).  Workgroup-uniform: one scalar load pair.
// Guard (like frame_of's, roi_align.hip): an entry that is out of range, not increasing, or a clip longer than max_len is CLAMPED so that
// the span lies inside [0, num_frames) and holds 1 .. max_len frames, and bad tells the kernel to write NaN for that clip.
struct ClipSpan { int first, len; bool bad; };
__device__ __forceinline__ ClipSpan clip_span(const int32_t* __restrict__ clip_start, int b, int num_frames, int max_len) {
  int a = clip_start[b], e = clip_start[b + 1];
  const bool bad = a < 0 || e > num_frames || e <= a || e - a > max_len;
  if (bad) {
    a = min(max(a, 0), num_frames - 1);
    e = min(max(e, a + 1), min(a + max_len, num_frames));
  }
  return ClipSpan{a, e - a, bad};
}

struct AttnBlockParams {
  const void* x;        // [num_frames * 3][256] bf16 token rows (attn_block_x3_kernel: f32)
  void* y;              // [num_frames * 3][256] bf16: rows after both passes (attn_block_x3_kernel: f32)
  const void* w_in;     // in_proj weight [768][256], MFMA-fragment-major (24 column tiles; attn_block_x3_kernel: the SPLIT fragment-major form)
  const float* b_in;    // [768]
  const void* w_out;    // out_proj weight [256][256], fragment-major
  const float* b_out;   // [256]
  const float* g;       // attention_norm gamma / beta [256]
  const float* b;
  int num_clips, T;     // T: frames per clip (clip_start == NULL), else the longest clip's (3 T <= 32 either way)
  float scale;          // 1 / sqrt(head_dim)
  const int32_t* clip_start;   // NULL: num_clips clips of T frames; else the clip table above
  int num_frames;              // read with clip_start only
};

template <typename T>   // bf16_t or f16_t
__global__ __launch_bounds__(256, 1) void attn_block_kernel(const AttnBlockParams p) {
  typedef Ops16<T> Ops;
  constexpr int D = RB_D, ROWS = RB_ROWS, ROWB = Ops::ROWB, QKV_LD = 3 * D;
  __shared__ __attribute__((aligned(16))) char s_a[ROWS * ROWB];
  __shared__ __attribute__((aligned(16))) char s_b[ROWS * ROWB];
  __shared__ __attribute__((aligned(16))) char s_att[ROWS * ROWB];
  __shared__ __attribute__((aligned(16))) char s_big[ROWS * QKV_LD * 2];   // qkv (bf16) | out-projection slab (f32, 32 KiB of the 48)
  T* s_qkv = (T*)s_big;
  float* s_t = (float*)s_big;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int T_b = p.T;
  size_t m0 = (size_t)blockIdx.x * (3 * p.T);
  bool bad = false;
  if (p.clip_start) {                                         // ragged batch: this clip's span from the table
    const ClipSpan cs = clip_span(p.clip_start, blockIdx.x, p.num_frames, p.T);
    T_b = cs.len; m0 = (size_t)cs.first * 3; bad = cs.bad;
  }
  const int rows = 3 * T_b;                                   // <= 32 (checked by the launcher; clip_span clamps)
  Ops::stage_rows(s_a, (const char*)p.x + m0 * ROWB, rows, tid);   // token rows -> LDS (padding rows are zero; never stored)
  const int arow = lane & 31;
  typename Ops::Bfr bfr;
  Ops::load_b(bfr, p.w_in, wave * 2, lane);
  __syncthreads();
  char* xin = s_a;
  char* xout = s_b;
  for (int pass = 0; pass < 2; ++pass) {
    // ---- q | k | v = x . Win^T + b, rounded to bf16 (the unfused path stores qkv): three sub-steps of 256 columns
#pragma unroll 1
    for (int u = 0; u < 3; ++u) {
      f32x16 acc[2];
      Ops::mma2(xin, bfr, acc, lane);
      if (u < 2) Ops::load_b(bfr, p.w_in, (u + 1) * 8 + wave * 2, lane);
      else Ops::load_b(bfr, p.w_out, wave * 2, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = u * D + wave * 64 + j * 32 + arow;
        const float bb = p.b_in[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) Elem<T>::st(s_qkv + mfma32_row(r, lane) * QKV_LD + col, acc[j][r] + bb);
      }
    }
    __syncthreads();
    // ---- attention core: thread = (query row, head) (attend_row_head); rows * 8 <= 256 pairs
    {
      const int L = pass == 0 ? 3 : T_b;
      const int i = tid >> 3, h = tid & 7;
      if (i < rows) {
        const int kbase = pass == 0 ? (i / 3) * 3 : i % 3, kstep = pass == 0 ? 1 : 3;
        __attribute__((aligned(16))) T o[32];
        attend_row_head<T>(s_qkv + i * QKV_LD + h * 32,
                           [&](int j) { return (const T*)(s_qkv + (kbase + j * kstep) * QKV_LD + D + h * 32); },
                           [&](int j) { return (const T*)(s_qkv + (kbase + j * kstep) * QKV_LD + 2 * D + h * 32); }, L, p.scale, o);
#pragma unroll
        for (int c = 0; c < 4; ++c) *(uint4*)(s_att + Ops::swz(i, h * 4 + c)) = *(const uint4*)(o + c * 8);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) *(uint4*)(s_att + Ops::swz(i, h * 4 + c)) = make_uint4(0, 0, 0, 0);
      }
    }
    __syncthreads();   // s_att complete, s_qkv consumed (s_t aliases it)
    // ---- out-projection + bias (f32 slab), then + residual -> bf16 -> LayerNorm (chain.hpp's step)
    {
      f32x16 acc[2];
      Ops::mma2(s_att, bfr, acc, lane);
      if (pass == 0) Ops::load_b(bfr, p.w_in, wave * 2, lane);
      rb_slab(s_t, acc, p.b_out, wave, lane);
    }
    __syncthreads();
    const int c0 = lane * 4;
    const float4 g4 = *(const float4*)(p.g + c0), b4 = *(const float4*)(p.b + c0);
#pragma unroll
    for (int rr8 = 0; rr8 < 8; ++rr8) {
      const int r = wave * 8 + rr8;
      const float4 t4 = *(const float4*)(s_t + r * D + c0);
      float v[4] = {t4.x, t4.y, t4.z, t4.w};
      {  // residual = this pass's input row (the mmcv wrapper adds the identity, transformer.py MultiheadAttention)
        float rr[4];
        Ops::unquad(*(const uint2*)(xin + Ops::quad_off(r, c0)), rr);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += rr[e];
      }
      Ops::round_stored(v);   // the unfused path stores the projection's output as bf16 before the LayerNorm kernel reads it
      ln256_row<Ops::kLnSq>(v, g4, b4, false);
      uint2 o = Ops::quad(v);
      if (r >= rows) o = make_uint2(0, 0);   // padding rows stay zero
      Ops::park(xout, r, c0, o);
      if (bad) o = make_uint2(0xffffffffu, 0xffffffffu);   // a clip the table guard clamped: NaN (bf16 and fp16 alike)
      if (pass == 1 && r < rows) *(uint2*)((char*)p.y + (m0 + r) * ROWB + c0 * 2) = o;
    }
    __syncthreads();
    char* t = xin; xin = xout; xout = t;
  }
}

static inline bool attn_block_applicable(int T) { return T >= 1 && 3 * T <= 32; }   // T: the longest clip of the call
