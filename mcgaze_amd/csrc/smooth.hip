// Temporal smoothing on the device: the merged per-frame rows of a store (merge.hip) -> the gaze the reference's published accuracy is
// measured on.  tools/calculate_mae_gaze360.py:16-29 (smooth_filter) mixes every gaze vector with its neighbours in time -- alpha 0.6,
// three taps in the interior, two at a video's ends -- and re-normalises; a one-frame video is returned as it is.  The arithmetic is
// stated once, in include/mcgaze_hip.h (mcg_smooth_gaze); the host (harness.smooth_plan) names, per output frame, the store rows of the
// frame and of its neighbours, so a stream's ends and a frame whose predecessor was handed out a tick ago are table entries, not cases
// of the kernel.  Tiny and latency-bound: one thread per (output frame, vector), the fused gaze and the three clues' -- four per frame.
// f32 multiplies, adds, one exact halving, two explicit fma, one correctly rounded square root and division, uncontracted.
#include "common.hpp"

#define MCG_SMOOTH_THREADS 256  // 64 output frames x 4 vectors
#define MCG_SMOOTH_ROW 27       // the store row of merge.hip: det[3][5] | fused[3] | others[3][3]
#define MCG_SMOOTH_GAZE 15      // vector v of a row starts at float 15 + 3 v: fused, then the clues
#define MCG_SMOOTH_OUT 12       // fused[3] | others[3][3]

#pragma clang fp contract(off)
__global__ __launch_bounds__(MCG_SMOOTH_THREADS) void smooth_gaze_kernel(const float* __restrict__ store, int store_rows,
                                                                         const int32_t* __restrict__ plan, int num_out, float a, float b,
                                                                         float* __restrict__ out) {
  const int t = blockIdx.x * MCG_SMOOTH_THREADS + threadIdx.x;
  const int f = t >> 2, v = t & 3;
  if (f >= num_out) return;
  const int prev = plan[(size_t)f * 3], row = plan[(size_t)f * 3 + 1], next = plan[(size_t)f * 3 + 2];
  float* o = out + (size_t)f * MCG_SMOOTH_OUT + 3 * v;
  const bool in_p = prev >= 0 && prev < store_rows, in_n = next >= 0 && next < store_rows;
  if (row < 0 || row >= store_rows || (!in_p && prev != -1) || (!in_n && next != -1)) {   // never an address: the row says so
    for (int k = 0; k < 3; ++k) o[k] = __builtin_nanf("");
    return;
  }
  const int at = MCG_SMOOTH_GAZE + 3 * v;
  float x[3], r[3];
  for (int k = 0; k < 3; ++k) x[k] = store[(size_t)row * MCG_SMOOTH_ROW + at + k];
  if (!in_p && !in_n) {                                  // a one-frame stream: smooth_filter's size(0) < 2 branch, not normalised
    for (int k = 0; k < 3; ++k) o[k] = x[k];
    return;
  }
  if (in_p && in_n) {
    for (int k = 0; k < 3; ++k) {
      const float p = store[(size_t)prev * MCG_SMOOTH_ROW + at + k], q = store[(size_t)next * MCG_SMOOTH_ROW + at + k];
      r[k] = a * x[k];
      r[k] = r[k] + (b * (p + q)) / 2.0f;
    }
  } else {
    const int other = in_p ? prev : next;
    for (int k = 0; k < 3; ++k) r[k] = a * x[k] + b * store[(size_t)other * MCG_SMOOTH_ROW + at + k];
  }
  const float n = sqrtf(__builtin_fmaf(r[2], r[2], __builtin_fmaf(r[1], r[1], r[0] * r[0])));
  for (int k = 0; k < 3; ++k) o[k] = r[k] / n;           // IEEE division; n == 0 gives what it gives on the host
}

extern "C" int mcg_smooth_gaze(mcg_stream s, const float* store, int store_rows, const int32_t* plan, int num_out, double alpha,
                               float* out) {
  MCG_CHECK_ARG(num_out >= 0 && num_out <= (1 << 24), "mcg_smooth_gaze: 0 .. 2^24 output frames per call (got %d)", num_out);
  MCG_CHECK_ARG(store_rows > 0 && store_rows <= (1 << 24), "mcg_smooth_gaze: a store of 1 .. 2^24 rows (got store_rows=%d)", store_rows);
  MCG_CHECK_ARG(alpha - alpha == 0.0, "mcg_smooth_gaze: alpha must be finite (got %g)", alpha);
  if (num_out == 0) return MCG_OK;
  MCG_CHECK_ARG(store && plan && out, "mcg_smooth_gaze: null store, plan or out");
  const int blocks = (num_out * 4 + MCG_SMOOTH_THREADS - 1) / MCG_SMOOTH_THREADS;
  hipLaunchKernelGGL(smooth_gaze_kernel, dim3(blocks), dim3(MCG_SMOOTH_THREADS), 0, (hipStream_t)s, store, store_rows, plan, num_out,
                     (float)alpha, (float)(1.0 - alpha), out);
  MCG_CHECK_LAUNCH("mcg_smooth_gaze");
  return MCG_OK;
}
