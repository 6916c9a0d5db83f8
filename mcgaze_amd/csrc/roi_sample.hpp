// The sample arithmetic of roi_align_kernel (roi_align.hip), shared with roi_mark_kernel, which flags the blocks of a deferred pyramid
// level that RoIAlign will read: both take level and coordinates from these functions, so the flagged footprint is by construction the
// set of pixels read -- boxes outside the image, degenerate and NaN boxes included.  Checked against roi_align_kernel itself by
// tests/test_gpu_defer_blocks.py: a map that is NaN outside the flagged blocks gives the same RoIAlign bits, and the flagged set equals
// a host statement of the footprint (tests/defer_cases.py), so it is neither short of a block nor larger than the 8 x 8 cover.
#pragma once

// map_roi_levels (single_level_roi_extractor.py:51-54), with the NaN guard: a NaN box reads level 0
__device__ __forceinline__ int roi_level(float x1, float y1, float x2, float y2, float finest_scale) {
  const float sc = sqrtf((x2 - x1) * (y2 - y1));
  int level = (int)fminf(fmaxf(floorf(log2f(sc / finest_scale + 1e-6f)), 0.f), 3.f);
  if (!(sc == sc)) level = 0;
  return level;
}

// Sample i (0 .. 2 P - 1: bin i / 2, sample i % 2) along one axis of a box [a1, a2] (image coordinates) on a level of L pixels and
// scale ss: the two taps lo / hi, the weight l of hi, and whether the sample reads anything (y < -1 or y > L adds 0, and so does a
// NaN y: the comparisons below are ordered, so NaN is outside -- it has to be caught BEFORE the clamp, which turns NaN into 0).
template <int P, int S>
__device__ __forceinline__ void roi_axis_sample(float a1, float a2, float ss, int L, int i, int& lo_out, int& hi_out, float& l_out, int& valid_out) {
  const float start = a1 * ss - 0.5f, end = a2 * ss - 0.5f;
  const float bin = (end - start) / (float)P;
  float c = start + (float)(i / S) * bin + ((float)(i % S) + 0.5f) * bin / (float)S;
  const int valid = c >= -1.0f && c <= (float)L;
  c = fmaxf(c, 0.f);
  int lo = (int)c, hi;
  if (lo >= L - 1) {
    lo = hi = L - 1;
    c = (float)lo;
  } else {
    hi = lo + 1;
  }
  lo_out = lo; hi_out = hi; l_out = c - (float)lo; valid_out = valid;
}
