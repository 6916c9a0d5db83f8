// Row-block MLP chain for the decoder's 256-wide token features: up to four steps of
//     y = [ReLU] LayerNorm( src . W^T [+ bias] [+ residual] )        W: [256][256], src = the kernel's input rows or the previous y
// in ONE launch.  Replaces runs of (igemm linear -> ln_kernel) launch pairs on M = 3 x frames rows -- each pair is two launches of
// ~8 us for ~1 us of work (f16x3: 16.4 us per 1344 x 256 x 256 linear and 7.5 us per LayerNorm launch, profiles/r03_l_decoder_x3.md) --
// e.g. the classification / regression towers of gaze_stqi_head.py:185-188 (8 launches -> 1) and the attention output projection +
// residual + LayerNorm of :151-155 / :162-166 (2 -> 1).
//
// One kernel for the three storage formats, over an operand policy of rowblock.hpp: Ops16<bf16_t>, Ops16<f16_t> (rows in LDS in the storage
// type) or OpsX3 (MCG_F16X3: f32 storage, rows in LDS split into fp16 high / low parts, three MFMAs per product).  One workgroup (4 waves)
// owns 32 token rows.  Per step wave w computes output columns [64 w, 64 w + 64) with the policy's row-block linear; results (+ bias) go to
// an f32 LDS slab; each wave then takes 8 rows, adds the residual, rounds to the storage type exactly where the unfused linear stores its
// output, and normalises with ln256_row: ln_kernel's lane -> column ownership and reduction order.  K order, the order of the three split
// terms and the rounding points are the igemm kernels', so the chain reproduces the launch sequence it replaces
// (tests/test_gpu_kernels.py::test_mlp_chain_matches_unfused_bitwise, ::test_attn_block_x3_matches_unfused_bitwise).
#pragma once
#include "rowblock.hpp"

struct ChainStep {
  const void* W;        // 256x256, MFMA-fragment-major in the policy's form (include/mcgaze_hip.h MCG_SW_*_WF)
  const float* bias;    // [256] or null
  const void* res;      // residual rows [M][256] (storage type) added before the LayerNorm, or null
  const float* g;       // LayerNorm gamma / beta [256]
  const float* b;
  void* dst;            // [M][256] (storage type) or null (intermediate only)
  int from_input;       // 1: source rows are the kernel's input, 0: the previous step's output
  int relu;
};
struct ChainParams {
  const void* x;        // [M][256] (storage type)
  int M, steps;
  ChainStep st[4];
};

template <class Ops>
__global__ __launch_bounds__(256, 1) void mlp_chain_kernel(const ChainParams p) {
  constexpr int D = RB_D, ROWS = RB_ROWS, ROWB = Ops::ROWB;
  typedef typename Ops::Quad Quad;
  __shared__ __attribute__((aligned(16))) char s_x[ROWS * ROWB];    // kernel input rows (A operand)
  __shared__ __attribute__((aligned(16))) char s_y[ROWS * ROWB];    // previous step's output (A operand)
  __shared__ __attribute__((aligned(16))) float s_t[ROWS * D];      // linear output (+ bias), f32, row-major (LayerNorm input)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * ROWS;
  Ops::stage_rows(s_x, (const char*)p.x + (size_t)m0 * ROWB, p.M - m0, tid);   // rows beyond M are zero; never stored
  __syncthreads();
  // B fragments of a whole step live in registers (occupancy is irrelevant at 42 workgroups): all loads of a step are in flight together,
  // and the NEXT step's are issued as soon as this step's MFMAs have consumed theirs, so their L2 latency hides under the LayerNorm phase
  typename Ops::Bfr bfr;
  Ops::load_b(bfr, p.st[0].W, wave * 2, lane);
  for (int si = 0; si < p.steps; ++si) {
    const ChainStep& st = p.st[si];
    f32x16 acc[2];
    Ops::mma2(st.from_input ? s_x : s_y, bfr, acc, lane);
    if (si + 1 < p.steps) Ops::load_b(bfr, p.st[si + 1].W, wave * 2, lane);
    rb_slab(s_t, acc, st.bias, wave, lane);
    __syncthreads();
    // ---- [+ residual] LayerNorm [ReLU]: wave -> 8 rows, lane -> 4 consecutive columns (ln_kernel's order)
    const int c0 = lane * 4;
    const float4 g4 = *(const float4*)(st.g + c0), b4 = *(const float4*)(st.b + c0);
#pragma unroll
    for (int rr8 = 0; rr8 < 8; ++rr8) {  // unrolled: the 8 rows' residual loads and reductions overlap
      const int r = wave * 8 + rr8;
      const size_t at = ((size_t)(m0 + r) * D + c0) * Ops::ES;
      const float4 t4 = *(const float4*)(s_t + r * D + c0);
      float v[4] = {t4.x, t4.y, t4.z, t4.w};
      if (st.res && m0 + r < p.M) {  // (acc + bias) + residual in f32, as the igemm epilogue does
        float rr[4];
        Ops::unquad(*(const Quad*)((const char*)st.res + at), rr);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += rr[e];
      }
      Ops::round_stored(v);   // the unfused path stores the linear's output and the LayerNorm kernel reads that back: same rounding here
      ln256_row<Ops::kLnSq>(v, g4, b4, st.relu);
      const Quad o = Ops::quad(v);
      Ops::park(s_y, r, c0, o);
      if (st.dst && m0 + r < p.M) *(Quad*)((char*)st.dst + at) = o;
    }
    __syncthreads();
  }
}

// dt: MCG_BF16, MCG_F16 or MCG_F16X3
static inline int launch_mlp_chain(hipStream_t s, const ChainParams& p, mcg_dtype dt) {
  const dim3 grid((p.M + 31) / 32);
  if (dt == MCG_F16X3) hipLaunchKernelGGL(mlp_chain_kernel<OpsX3>, grid, dim3(256), 0, s, p);
  else if (mcg_is16(dt)) dispatch_elem16(dt, [&](auto e) { hipLaunchKernelGGL(mlp_chain_kernel<Ops16<decltype(e)>>, grid, dim3(256), 0, s, p); });
  else { mcg_set_error("mlp_chain: unsupported dtype %d", (int)dt); return MCG_ERR_UNSUPPORTED; }
  MCG_CHECK_LAUNCH("mlp_chain");
  return MCG_OK;
}
