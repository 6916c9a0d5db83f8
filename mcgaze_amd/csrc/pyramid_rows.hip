// Pyramid rows (ABI 17): frame n of a contiguous NHWC pyramid (what mcg_backbone_fpn_forward writes) -> row row_of[n] of a pyramid STORE,
// all four levels in one launch.  The store of one stream is a ring the trunk writes at a row offset (mcgaze_amd/stream.py: PyramidRing);
// a store SHARED by many live streams (GazeStreamPool: the reference runs one clip per tracked person, MCGaze_demo/demo.ipynb cell 4, and
// one sliding window per call, tools/test_gaze360_gaze.py:72-111) frees its rows out of order, so a batch of new frames lands in
// arbitrary rows.  A copy after the trunk and not a remapped epilogue: the FPN output convs stay as measured.
// Memory-bound and plain: one workgroup per (frame, slice of at most 16 KiB of one level of that frame), 16-byte loads and stores, up to
// four in flight per lane.  A level row is h * w * 256 * esize bytes, a multiple of 512: every slice is whole 16-byte chunks, no tail.
#include "common.hpp"

#define MCG_ROWS_SLICE 16384   // bytes of one level one workgroup moves: 256 lanes x 16 bytes x 4

struct RowLevels {
  const char* src[4];
  char* dst[4];
  size_t bytes[4];   // bytes of one frame of level i
  int first[4];      // first[i] = slices of the levels below i: blockIdx.x in [first[i], first[i + 1]) works on level i
};

__global__ __launch_bounds__(256) void pyramid_scatter_rows_kernel(RowLevels lv, const int32_t* __restrict__ row_of, int store_rows) {
  const int frame = blockIdx.y;
  const int row = __builtin_amdgcn_readfirstlane(row_of[frame]);   // one row per workgroup: a scalar from here on
  if (row < 0 || row >= store_rows) return;                        // a frame without a row is skipped
  const int bx = blockIdx.x;
  const int l = (bx >= lv.first[1]) + (bx >= lv.first[2]) + (bx >= lv.first[3]);
  const size_t bytes = l == 0 ? lv.bytes[0] : l == 1 ? lv.bytes[1] : l == 2 ? lv.bytes[2] : lv.bytes[3];
  const int first = l == 0 ? 0 : l == 1 ? lv.first[1] : l == 2 ? lv.first[2] : lv.first[3];
  const char* sbase = l == 0 ? lv.src[0] : l == 1 ? lv.src[1] : l == 2 ? lv.src[2] : lv.src[3];
  char* dbase = l == 0 ? lv.dst[0] : l == 1 ? lv.dst[1] : l == 2 ? lv.dst[2] : lv.dst[3];
  const size_t at = (size_t)(bx - first) * MCG_ROWS_SLICE;         // of this slice inside the frame's level
  const size_t left = bytes - at;
  const int n = left < (size_t)MCG_ROWS_SLICE ? (int)left : MCG_ROWS_SLICE;
  const uint4* src = (const uint4*)(sbase + (size_t)frame * bytes + at);
  uint4* dst = (uint4*)(dbase + (size_t)row * bytes + at);
  const int chunks = n >> 4, t = threadIdx.x;
  // every load issued before the first store; a lane past the slice's end re-reads the slice's last chunk and stores nothing
  const int last = chunks - 1;
  const uint4 v0 = src[min(t, last)], v1 = src[min(t + 256, last)], v2 = src[min(t + 512, last)], v3 = src[min(t + 768, last)];
  if (t < chunks) dst[t] = v0;
  if (t + 256 < chunks) dst[t + 256] = v1;
  if (t + 512 < chunks) dst[t + 512] = v2;
  if (t + 768 < chunks) dst[t + 768] = v3;
}

extern "C" int mcg_pyramid_scatter_rows(mcg_stream s, mcg_dtype dt, const void* const src[4], void* const dst[4], int num_frames,
                                        int store_rows, int H, int W, const int32_t* row_of) {
  MCG_CHECK_ARG(src && dst && row_of, "mcg_pyramid_scatter_rows: null pointer");
  MCG_CHECK_ARG(dt == MCG_F32 || dt == MCG_BF16 || dt == MCG_F16X3 || dt == MCG_F16, "mcg_pyramid_scatter_rows: unknown dtype %d", (int)dt);
  MCG_CHECK_ARG(num_frames >= 0 && num_frames <= 65535, "mcg_pyramid_scatter_rows: 0 .. 65535 frames per call (got %d)", num_frames);
  MCG_CHECK_ARG(store_rows > 0, "mcg_pyramid_scatter_rows: empty store (store_rows=%d)", store_rows);
  MCG_CHECK_ARG(H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0, "mcg_pyramid_scatter_rows: frame size %dx%d must be a multiple of 32", H, W);
  if (num_frames == 0) return MCG_OK;
  RowLevels lv;
  int slices = 0;
  for (int i = 0; i < 4; ++i) {
    MCG_CHECK_ARG(src[i] && dst[i] && ((uintptr_t)src[i] & 15) == 0 && ((uintptr_t)dst[i] & 15) == 0,
                  "mcg_pyramid_scatter_rows: level %d must be a non-null, 16-byte aligned pointer on both sides", i);
    lv.src[i] = (const char*)src[i];
    lv.dst[i] = (char*)dst[i];
    lv.bytes[i] = (size_t)((H / 4) >> i) * ((W / 4) >> i) * 256 * MCG_ELEM_BYTES(dt);
    lv.first[i] = slices;
    slices += (int)((lv.bytes[i] + MCG_ROWS_SLICE - 1) / MCG_ROWS_SLICE);
  }
  hipLaunchKernelGGL(pyramid_scatter_rows_kernel, dim3(slices, num_frames), dim3(256), 0, (hipStream_t)s, lv, row_of, store_rows);
  MCG_CHECK_LAUNCH("mcg_pyramid_scatter_rows");
  return MCG_OK;
}
