// Overlap merge on the device: the decoder outputs of one call -> the per-frame result rows of a store that stays in device memory.
// harness.merge_window (tools/test_gaze360_gaze.py:129-206) applies windows one after the other, and the result is not associative -- at
// clip_len 7, stride 4, L = 12 the plan is (0,7), (4,11), (5,12) and frames 5 and 6 become ((a + b) / 2 + c) / 2 -- so WINDOWS cannot be
// applied in parallel, but destination FRAMES can: the host (harness.merge_plan) lists, per destination frame, the decoder-output frames
// that land on it in plan order, and a frame folds its list front to back.  The kernel also does harness.clip_outputs' rearrangement
// (fused = gaze[0], others[n][c] = gaze[1 + c][n], box / scale_factor as rescale=True does, multiclue_gaze_roi_head.py:360-363).
// Tiny and latency-bound: one thread per (destination frame, clue); thread c also carries component c of the fused gaze.  The arithmetic
// is f32 adds, exact halvings, compares and one correctly rounded division, uncontracted: the host merge's bits.
#include "common.hpp"

#define MCG_MERGE_THREADS 192   // 64 destination frames x 3 clues
#define MCG_MERGE_ROW 27        // det[3][5] (x1 y1 x2 y2 score) | fused[3] | others[3][3]

#pragma clang fp contract(off)
__global__ __launch_bounds__(MCG_MERGE_THREADS) void merge_windows_kernel(const float* __restrict__ gaze, const float* __restrict__ boxes,
                                                                          const float* __restrict__ scores, int n,
                                                                          const float* __restrict__ scale, int scale_stride,
                                                                          const int32_t* __restrict__ plan, int num_dst, int max_src,
                                                                          float* __restrict__ store, int store_rows, float thr) {
  const int t = blockIdx.x * MCG_MERGE_THREADS + threadIdx.x;
  const int d = t / 3, c = t - 3 * d;
  if (d >= num_dst) return;
  const int32_t* row = plan + (size_t)d * (2 + max_src);
  const int dst = row[0];
  if (dst < 0 || dst >= store_rows) return;              // a destination outside the store is skipped
  float* out = store + (size_t)dst * MCG_MERGE_ROW;
  bool have = row[1] != 0, changed = false;
  float box[4] = {0.f, 0.f, 0.f, 0.f}, score = 0.f, fused = 0.f, oth[3] = {0.f, 0.f, 0.f};
  if (have) {                                            // an earlier call wrote this frame
    for (int k = 0; k < 4; ++k) box[k] = out[c * 5 + k];
    score = out[c * 5 + 4];
    fused = out[15 + c];
    for (int k = 0; k < 3; ++k) oth[k] = out[18 + c * 3 + k];
  }
  for (int j = 0; j < max_src; ++j) {
    const int s = row[2 + j];
    if (s < 0 || s >= n) continue;                       // -1: no source; any other frame outside the call's outputs is skipped too
    const float sc = scores[s * 3 + c];
    const bool low = sc < thr;
    float b[4];
    for (int k = 0; k < 4; ++k) {
      float v = boxes[((size_t)s * 3 + c) * 4 + k];
      if (scale) v = v / scale[(size_t)s * scale_stride + k];   // IEEE division, as torch and numpy divide
      b[k] = low ? 0.f : v;
    }
    const float f = gaze[(size_t)s * 3 + c];
    float o[3];
    for (int k = 0; k < 3; ++k) o[k] = gaze[((size_t)(1 + c) * n + s) * 3 + k];
    if (!have) {
      for (int k = 0; k < 4; ++k) box[k] = b[k];
      score = sc;
      fused = f;
      for (int k = 0; k < 3; ++k) oth[k] = o[k];
      have = true;
    } else {
      const bool bad = (score < thr) | low;              // the stored score before it is averaged
      for (int k = 0; k < 4; ++k) box[k] = bad ? 0.f : (box[k] + b[k]) * 0.5f;
      score = (score + sc) * 0.5f;
      fused = (fused + f) * 0.5f;
      for (int k = 0; k < 3; ++k) oth[k] = (oth[k] + o[k]) * 0.5f;
    }
    changed = true;
  }
  if (!changed) return;
  for (int k = 0; k < 4; ++k) out[c * 5 + k] = box[k];
  out[c * 5 + 4] = score;
  out[15 + c] = fused;
  for (int k = 0; k < 3; ++k) out[18 + c * 3 + k] = oth[k];
}

extern "C" int mcg_merge_windows(mcg_stream s, const float* gaze, const float* boxes, const float* scores, int num_frames, const float* scale,
                                 int scale_per_frame, const int32_t* plan, int num_dst, int max_src, float* store, int store_rows,
                                 float person_threshold) {
  MCG_CHECK_ARG(num_frames >= 0 && num_frames <= (1 << 24), "mcg_merge_windows: 0 .. 2^24 output frames per call (got %d)", num_frames);
  MCG_CHECK_ARG(num_dst >= 0 && num_dst <= (1 << 24), "mcg_merge_windows: 0 .. 2^24 destination frames per call (got %d)", num_dst);
  MCG_CHECK_ARG(max_src >= 1 && max_src <= 4096, "mcg_merge_windows: 1 .. 4096 sources per destination frame (got max_src=%d)", max_src);
  MCG_CHECK_ARG(store_rows > 0 && store_rows <= (1 << 24), "mcg_merge_windows: a store of 1 .. 2^24 rows (got store_rows=%d)", store_rows);
  MCG_CHECK_ARG(scale_per_frame == 0 || scale_per_frame == 1, "mcg_merge_windows: scale_per_frame is 0 or 1 (got %d)", scale_per_frame);
  if (num_dst == 0) return MCG_OK;
  MCG_CHECK_ARG(plan && store, "mcg_merge_windows: null plan or store");
  MCG_CHECK_ARG(num_frames == 0 || (gaze && boxes && scores), "mcg_merge_windows: null decoder output");
  const int blocks = (num_dst * 3 + MCG_MERGE_THREADS - 1) / MCG_MERGE_THREADS;
  hipLaunchKernelGGL(merge_windows_kernel, dim3(blocks), dim3(MCG_MERGE_THREADS), 0, (hipStream_t)s, gaze, boxes, scores, num_frames, scale,
                     scale_per_frame ? 4 : 0, plan, num_dst, max_src, store, store_rows, person_threshold);
  MCG_CHECK_LAUNCH("mcg_merge_windows");
  return MCG_OK;
}
