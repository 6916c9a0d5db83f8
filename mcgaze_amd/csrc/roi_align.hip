// RoIAlign over all pyramid levels in ONE launch, level chosen per box on the device (no host
// nonzero()/sync per level as in single_level_roi_extractor.py:86-104).
//
// Definition implemented (mmcv.ops.RoIAlign, pool_mode='avg', aligned=True, sampling_ratio=2,
// output 7x7 -- the published mmcv-full 1.4.x / Detectron2 kernel):
//   start = coord*spatial_scale - 0.5; bin = (end-start)/7; sample (iy,ix) of bin (ph,pw) at
//   y = start_h + ph*bin_h + (iy+.5)*bin_h/2;  a sample with y < -1 or y > H (x likewise) adds 0;
//   otherwise y = max(y,0); y_low = int(y); if y_low >= H-1: y_low = y_high = H-1, y = y_low;
//   value = bilinear; output = mean of the 4 samples.
// Features are NHWC so one sample touches C contiguous channels; output is [box][49][C].
//
// Indexed form (frame_of != NULL, mcg_roi_align_indexed / mcg_decoder_forward_indexed): the features are a pyramid STORE of
// pyramid_frames rows and box b of window frame n = b / boxes_per_frame reads row frame_of[n] -- the gather of a window's frames out of
// a store that holds each distinct video frame once happens here, in the 49 x 4 sample reads of a box, instead of as a copy of whole
// pyramid rows.  The index is uniform per workgroup (one box per workgroup): read once, as a scalar.  An index outside
// [0, pyramid_frames) reads nothing: the address is clamped to row 0 and the box's output is NaN.  frame_of == NULL is the plain
// path (row = n) with the same code and bits as before.
#include "common.hpp"
#include "roi_sample.hpp"

struct RoiLevels {
  const void* feat[4];
  int h[4], w[4];
  float scale[4];
};

template <typename T>
__global__ __launch_bounds__(256) void roi_align_kernel(RoiLevels lv, int C, const float* __restrict__ boxes, int boxes_per_frame,
                                                        const int32_t* __restrict__ frame_of, int pyramid_frames,
                                                        T* __restrict__ out, int32_t* __restrict__ levels_out, float finest_scale) {
  constexpr int EPC = Elem<T>::kPerChunk;
  constexpr int P = 7, S = 2, NS = P * S;
  __shared__ int s_lo[2][NS], s_hi[2][NS];
  __shared__ float s_l[2][NS], s_h[2][NS];
  __shared__ int s_valid[2][NS];
  const int box = blockIdx.x, tid = threadIdx.x;
  const float x1 = boxes[box * 4 + 0], y1 = boxes[box * 4 + 1], x2 = boxes[box * 4 + 2], y2 = boxes[box * 4 + 3];
  const int level = roi_level(x1, y1, x2, y2, finest_scale);
  const int H = lv.h[level], W = lv.w[level];
  const float ss = lv.scale[level];
  if (tid < 2 * NS) {
    const int axis = tid / NS, i = tid % NS;  // axis 0 = y, 1 = x
    int lo, hi, valid;
    float l;
    roi_axis_sample<P, S>(axis == 0 ? y1 : x1, axis == 0 ? y2 : x2, ss, axis == 0 ? H : W, i, lo, hi, l, valid);
    s_lo[axis][i] = lo; s_hi[axis][i] = hi; s_l[axis][i] = l; s_h[axis][i] = 1.f - l; s_valid[axis][i] = valid;
  }
  if (tid == 0) {
    if (levels_out) levels_out[box] = level;
  }
  __syncthreads();
  int frame = box / boxes_per_frame;
  bool bad_row = false;
  if (frame_of) {
    frame = __builtin_amdgcn_readfirstlane(frame_of[frame]);   // uniform per workgroup: one scalar load
    bad_row = frame < 0 || frame >= pyramid_frames;
    if (bad_row) frame = 0;                                     // never address outside the store
  }
  const T* __restrict__ F = (const T*)lv.feat[level] + (long long)frame * H * W * C;
  const int groups = C / EPC, bins_per_pass = 256 / groups;
  const int cg = tid % groups, slot = tid / groups;
  if (bad_row) {
    float nan[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) nan[e] = __builtin_nanf("");
    for (int bin = slot; bin < P * P; bin += bins_per_pass)
      *(uint4*)(out + ((long long)box * (P * P) + bin) * C + cg * EPC) = f32_to_chunk(nan, (T*)nullptr);
    return;
  }
  for (int bin = slot; bin < P * P; bin += bins_per_pass) {
    const int ph = bin / P, pw = bin % P;
    float acc[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
#pragma unroll
    for (int iy = 0; iy < S; ++iy) {
      const int yi = ph * S + iy;
#pragma unroll
      for (int ix = 0; ix < S; ++ix) {
        const int xi = pw * S + ix;
        if (!(s_valid[0][yi] && s_valid[1][xi])) continue;
        const int yl = s_lo[0][yi], yh = s_hi[0][yi], xl = s_lo[1][xi], xh = s_hi[1][xi];
        const float ly = s_l[0][yi], hy = s_h[0][yi], lx = s_l[1][xi], hx = s_h[1][xi];
        const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
        float v1[EPC], v2[EPC], v3[EPC], v4[EPC];
        chunk_to_f32(*(const uint4*)(F + ((long long)yl * W + xl) * C + cg * EPC), v1, (T*)nullptr);
        chunk_to_f32(*(const uint4*)(F + ((long long)yl * W + xh) * C + cg * EPC), v2, (T*)nullptr);
        chunk_to_f32(*(const uint4*)(F + ((long long)yh * W + xl) * C + cg * EPC), v3, (T*)nullptr);
        chunk_to_f32(*(const uint4*)(F + ((long long)yh * W + xh) * C + cg * EPC), v4, (T*)nullptr);
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] += w1 * v1[e] + w2 * v2[e] + w3 * v3[e] + w4 * v4[e];
      }
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] *= (1.0f / (float)(S * S));
    *(uint4*)(out + ((long long)box * (P * P) + bin) * C + cg * EPC) = f32_to_chunk(acc, (T*)nullptr);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Deferred pyramid level (engine.hip): before a stage's RoIAlign, flag the 8 x 8-pixel output blocks of the deferred
// level that its boxes read and list those not yet listed.  One workgroup per box; a box routed to another level does nothing.  The
// pixels a box reads are {lo, hi of every valid y sample} x {lo, hi of every valid x sample} (a sample pair is read iff both samples are
// valid): the blocks are that product of block rows and columns.  state[b]: 0 = not listed, 1 = listed (by this or an earlier stage;
// stream order computes a listed block before the RoIAlign that follows).  Vector atomics only.
//
// Levels deferred by whole FRAMES (engine option fpn_levels_deferred: P3 .. P5, whose maps are too small for blocks): fm.state[l] != NULL
// names level l's flag per frame, fm.list[l] / fm.count[l] this stage's frame list.  A box routed to such a level lists its frame unless an
// earlier box or stage did -- the flag flip is the only way onto a list, so a frame is listed once over all stages and a list never holds
// more than one entry per frame.  Same launch, same rule (roi_level), no second kernel.
constexpr int kMarkMaxBlocks = 64;   // block rows / columns of the deferred level (512 pixels)
struct FrameMark { int *state[4], *list[4], *count[4]; };
__global__ __launch_bounds__(256) void roi_mark_kernel(const float* __restrict__ boxes, int boxes_per_frame, int level_deferred, int H, int W,
                                                       float ss, int* __restrict__ state, int* __restrict__ list, int* __restrict__ count,
                                                       float finest_scale, const FrameMark fm) {
  constexpr int P = 7, S = 2, NS = P * S;
  __shared__ int s_hit[2][kMarkMaxBlocks];
  const int box = blockIdx.x, tid = threadIdx.x;
  const float x1 = boxes[box * 4 + 0], y1 = boxes[box * 4 + 1], x2 = boxes[box * 4 + 2], y2 = boxes[box * 4 + 3];
  const int level = roi_level(x1, y1, x2, y2, finest_scale);               // 0 .. 3, uniform per workgroup
  if (tid == 0 && fm.state[level]) {
    const int f = box / boxes_per_frame;
    if (atomicCAS(&fm.state[level][f], 0, 1) == 0) fm.list[level][atomicAdd(fm.count[level], 1)] = f;
  }
  if (level != level_deferred) return;
  const int by_n = (H + 7) / 8, bx_n = (W + 7) / 8;
  if (tid < 2 * kMarkMaxBlocks) s_hit[tid / kMarkMaxBlocks][tid % kMarkMaxBlocks] = 0;
  __syncthreads();
  if (tid < 2 * NS) {
    const int axis = tid / NS, i = tid % NS;
    int lo, hi, valid;
    float l;
    roi_axis_sample<P, S>(axis == 0 ? y1 : x1, axis == 0 ? y2 : x2, ss, axis == 0 ? H : W, i, lo, hi, l, valid);
    if (valid) { s_hit[axis][lo >> 3] = 1; s_hit[axis][hi >> 3] = 1; }
  }
  __syncthreads();
  const int frame = box / boxes_per_frame;
  for (int t = tid; t < by_n * bx_n; t += 256) {
    const int by = t / bx_n, bx = t - by * bx_n;
    if (s_hit[0][by] && s_hit[1][bx]) {
      const int id = frame * (by_n * bx_n) + t;
      if (atomicCAS(&state[id], 0, 1) == 0) list[atomicAdd(count, 1)] = id;
    }
  }
}
// Deferred P2 lateral (engine option fpn_lateral_deferred): the 3 x 3 conv of an 8 x 8 output block reads a 10 x 10 window of the inner map,
// so the inner blocks a stage needs are its newly listed output blocks and their neighbours inside the SAME frame (up to nine; beyond the
// image border the conv pads with zeros and reads nothing).  One thread per (listed block, neighbour): whoever flips the neighbour's flag
// 0 -> 1 appends it to the stage's inner list -- a flag flip is the only way onto a list, so no block is listed twice, in this stage or a
// later one.  The grid is fixed by the map's size; the list length is read on the device.  Vector atomics only.
__host__ __device__ inline int inner_neighbour(int id, int k, int by_n, int bx_n) {   // k = 0 .. 8 -> block id, or -1 outside the frame
  const int bpf = by_n * bx_n, f = id / bpf, rem = id - f * bpf, by = rem / bx_n + k / 3 - 1, bx = rem % bx_n + k % 3 - 1;
  return (by < 0 || by >= by_n || bx < 0 || bx >= bx_n) ? -1 : f * bpf + by * bx_n + bx;
}
__global__ __launch_bounds__(256) void inner_mark_kernel(const int* __restrict__ out_list, const int* __restrict__ out_count, int by_n, int bx_n,
                                                         int nblk, int* __restrict__ state, int* __restrict__ list, int* __restrict__ count) {
  const int n = min(*out_count, nblk) * 9;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const int src = out_list[t / 9];
    if (src < 0 || src >= nblk) continue;
    const int id = inner_neighbour(src, t % 9, by_n, bx_n);
    if (id >= 0 && atomicCAS(&state[id], 0, 1) == 0) list[atomicAdd(count, 1)] = id;
  }
}
int launch_inner_mark(hipStream_t s, const int* out_list, const int* out_count, int H, int W, int nblk, int* state, int* list, int* count) {
  const long long threads = (long long)nblk * 9;
  const int blocks = (int)((threads + 255) / 256 < 1024 ? (threads + 255) / 256 : 1024);
  hipLaunchKernelGGL(inner_mark_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, s, out_list, out_count, (H + 7) / 8, (W + 7) / 8, nblk, state,
                     list, count);
  MCG_CHECK_LAUNCH("inner_mark");
  return MCG_OK;
}
// Host twin of inner_mark_kernel's rule (tests): the neighbours of block id inside its frame, id itself included; returns how many
extern "C" int mcg_inner_block_neighbours(int id, int H, int W, int out[9]) {
  int n = 0;
  for (int k = 0; k < 9; ++k) {
    const int v = inner_neighbour(id, k, (H + 7) / 8, (W + 7) / 8);
    if (v >= 0) out[n++] = v;
  }
  return n;
}
__global__ void defer_clear_kernel(int* __restrict__ p, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0;
}
bool roi_mark_supported(int H, int W) { return (H + 7) / 8 <= kMarkMaxBlocks && (W + 7) / 8 <= kMarkMaxBlocks; }
int launch_defer_clear(hipStream_t s, int* p, int n) {
  const int blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  hipLaunchKernelGGL(defer_clear_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, s, p, n);
  MCG_CHECK_LAUNCH("defer_clear");
  return MCG_OK;
}
// level < 0: no level is deferred by blocks (state / list / count unused); frame_state etc. [4], NULL entries (or NULL arrays) = that level
// is not deferred by frames
int launch_roi_mark(hipStream_t s, const float* boxes, int num_boxes, int boxes_per_frame, int level, int H, int W, int stride, int* state,
                    int* list, int* count, int* const* frame_state, int* const* frame_list, int* const* frame_count) {
  MCG_CHECK_ARG(roi_mark_supported(H, W), "roi_mark: deferred level of %dx%d pixels exceeds %d blocks per axis", H, W, kMarkMaxBlocks);
  FrameMark fm;
  for (int l = 0; l < 4; ++l) {
    const bool on = frame_state && frame_list && frame_count && frame_state[l] && frame_list[l] && frame_count[l];
    fm.state[l] = on ? frame_state[l] : nullptr; fm.list[l] = on ? frame_list[l] : nullptr; fm.count[l] = on ? frame_count[l] : nullptr;
  }
  hipLaunchKernelGGL(roi_mark_kernel, dim3(num_boxes), dim3(256), 0, s, boxes, boxes_per_frame, level, H, W, 1.0f / (float)stride, state, list,
                     count, 56.f, fm);
  MCG_CHECK_LAUNCH("roi_mark");
  return MCG_OK;
}
// The two marking kernels as stand-alone operators (tests and measurements): the launchers above over the caller's device buffers
extern "C" int mcg_roi_mark_blocks(mcg_stream s, const float* boxes, int num_boxes, int boxes_per_frame, int level, int H, int W, int stride,
                                   int* state, int* list, int* count) {
  MCG_CHECK_ARG(boxes && state && list && count, "mcg_roi_mark_blocks: null pointer");
  MCG_CHECK_ARG(num_boxes > 0 && boxes_per_frame > 0, "mcg_roi_mark_blocks: empty box set");
  MCG_CHECK_ARG(level >= 0 && level <= 3 && H > 0 && W > 0 && stride > 0, "mcg_roi_mark_blocks: bad level (level=%d %dx%d stride=%d)", level, H, W, stride);
  return launch_roi_mark((hipStream_t)s, boxes, num_boxes, boxes_per_frame, level, H, W, stride, state, list, count, nullptr, nullptr, nullptr);
}
// The frame marking alone: boxes routed to `level` list their frames (state [frames], list [frames], count [1]); no block level
extern "C" int mcg_roi_mark_frames(mcg_stream s, const float* boxes, int num_boxes, int boxes_per_frame, int level, int* state, int* list,
                                   int* count) {
  MCG_CHECK_ARG(boxes && state && list && count, "mcg_roi_mark_frames: null pointer");
  MCG_CHECK_ARG(num_boxes > 0 && boxes_per_frame > 0 && num_boxes % boxes_per_frame == 0,
                "mcg_roi_mark_frames: whole frames of boxes (num_boxes=%d boxes_per_frame=%d)", num_boxes, boxes_per_frame);
  MCG_CHECK_ARG(level >= 0 && level <= 3, "mcg_roi_mark_frames: bad level %d", level);
  int *fs[4] = {nullptr, nullptr, nullptr, nullptr}, *fl[4] = {nullptr, nullptr, nullptr, nullptr}, *fc[4] = {nullptr, nullptr, nullptr, nullptr};
  fs[level] = state; fl[level] = list; fc[level] = count;
  return launch_roi_mark((hipStream_t)s, boxes, num_boxes, boxes_per_frame, -1, 8, 8, 1, nullptr, nullptr, nullptr, fs, fl, fc);
}
extern "C" int mcg_inner_mark_blocks(mcg_stream s, const int* out_list, const int* out_count, int H, int W, int nblk, int* state, int* list,
                                     int* count) {
  MCG_CHECK_ARG(out_list && out_count && state && list && count, "mcg_inner_mark_blocks: null pointer");
  MCG_CHECK_ARG(H > 0 && W > 0 && nblk > 0 && nblk % (((H + 7) / 8) * ((W + 7) / 8)) == 0,
                "mcg_inner_mark_blocks: nblk = frames * blocks per frame (nblk=%d, %dx%d pixels)", nblk, H, W);
  return launch_inner_mark((hipStream_t)s, out_list, out_count, H, W, nblk, state, list, count);
}

int launch_roi_align(hipStream_t s, mcg_dtype dt, const void* const feats[4], const int feat_h[4], const int feat_w[4],
                     const int strides[4], int C, const float* boxes, int num_boxes, int boxes_per_frame, const int32_t* frame_of,
                     int pyramid_frames, void* out, int32_t* levels_out) {
  RoiLevels lv;
  for (int i = 0; i < 4; ++i) {
    lv.feat[i] = feats[i]; lv.h[i] = feat_h[i]; lv.w[i] = feat_w[i];
    lv.scale[i] = 1.0f / (float)strides[i];
  }
  const int epc = mcg_is16(dt) ? 8 : 4;
  MCG_CHECK_ARG(C % epc == 0 && C / epc <= 256 && 256 % (C / epc) == 0, "roi_align: unsupported channel count %d", C);
  dispatch_elem(dt, [&](auto e) {
    hipLaunchKernelGGL(roi_align_kernel<decltype(e)>, dim3(num_boxes), dim3(256), 0, s, lv, C, boxes, boxes_per_frame, frame_of, pyramid_frames, (decltype(e)*)out, levels_out, 56.f);
  });
  MCG_CHECK_LAUNCH("roi_align");
  return MCG_OK;
}

extern "C" int mcg_roi_align(mcg_stream s, mcg_dtype dt, const void* const feats[4], const int feat_h[4], const int feat_w[4],
                             const int strides[4], int C, const float* boxes, int num_boxes, int boxes_per_frame,
                             void* out, int32_t* levels_out) {
  MCG_CHECK_ARG(feats && feat_h && feat_w && strides && boxes && out, "mcg_roi_align: null pointer");
  MCG_CHECK_ARG(num_boxes > 0 && boxes_per_frame > 0, "mcg_roi_align: empty box set");
  for (int i = 0; i < 4; ++i) MCG_CHECK_ARG(feats[i] && feat_h[i] > 0 && feat_w[i] > 0 && strides[i] > 0, "mcg_roi_align: bad level %d", i);
  return launch_roi_align((hipStream_t)s, dt, feats, feat_h, feat_w, strides, C, boxes, num_boxes, boxes_per_frame, nullptr, 0, out, levels_out);
}

extern "C" int mcg_roi_align_indexed(mcg_stream s, mcg_dtype dt, const void* const feats[4], const int feat_h[4], const int feat_w[4],
                                     const int strides[4], int C, const float* boxes, int num_boxes, int boxes_per_frame,
                                     const int32_t* frame_of, int pyramid_frames, void* out, int32_t* levels_out) {
  MCG_CHECK_ARG(feats && feat_h && feat_w && strides && boxes && out && frame_of, "mcg_roi_align_indexed: null pointer");
  MCG_CHECK_ARG(num_boxes > 0 && boxes_per_frame > 0 && pyramid_frames > 0, "mcg_roi_align_indexed: empty box set or pyramid");
  for (int i = 0; i < 4; ++i) MCG_CHECK_ARG(feats[i] && feat_h[i] > 0 && feat_w[i] > 0 && strides[i] > 0, "mcg_roi_align_indexed: bad level %d", i);
  return launch_roi_align((hipStream_t)s, dt, feats, feat_h, feat_w, strides, C, boxes, num_boxes, boxes_per_frame, frame_of, pyramid_frames,
                          out, levels_out);
}
