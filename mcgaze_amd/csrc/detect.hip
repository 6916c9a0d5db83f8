// Head boxes from a detector's raw output, on the device: the post-processing of the demo's YOLOv5 head detector
// (MCGaze_demo/yolo_head/detect.py:74,95 -- non_max_suppression, then scale_coords(...).round(); utils/general.py:291-312, 393-481) on a
// [B, N, 5 + nc] f32 prediction that is already in device memory, so that "decoder surface in, annotated surface out" has no host round
// trip at the detector boundary.  The arithmetic is stated once, in include/mcgaze_hip.h ("head boxes from raw detector output");
// mcgaze_amd/pipeline.py::detect_heads_host is the same on the host.  Everything is f32 and uncontracted but the letterbox gain and pads.
//
// One launch, one workgroup of 1024 threads (16 waves) per image, four phases separated by barriers:
//   filter   the anchors in index order, 1024 per step: a row that passes becomes a 64-bit key (its score's bits, inverted so that a
//            higher score is a smaller key, over its anchor index) and is compacted into the workspace by a wave ballot and a prefix over
//            the 16 wave counts -- capacity num_anchors, so nothing overflows; no atomics, the order is the anchor order
//   order    rank by counting: the rank of a key is the number of smaller keys (keys are distinct: they hold the anchor).  Tiles of the
//            keys go through LDS and every thread ranks four keys per pass.  O(M^2) on one CU: right for the hundreds of candidates a 0.25
//            threshold leaves, slow (milliseconds) but correct at num_anchors candidates.  A row of rank r < min(M, max_nms) stores its
//            offset box and anchor at position r
//   greedy   row j belongs to thread j % 1024 for good, so its suppressed mark is read and written by one thread only.  Per KEPT row: all
//            threads mark the later rows it suppresses and report the first of their rows still standing into an LDS slot by an integer
//            minimum (order-free); one barrier; that minimum is the next kept row.  Three slots in rotation make the one barrier enough.
//            At most max_det rounds
//   output   thread k < count recomputes row k's box from the prediction (the same operations: the same bits), scales it back into its
//            frame and writes it; the rows from count up are zeroed
// The result does not depend on launch geometry or scheduling: every decision above is a pure function of the sorted order.
#include "common.hpp"

#pragma clang fp contract(off)

#define MCG_DET_THREADS 1024
#define MCG_DET_WAVES (MCG_DET_THREADS / MCG_WAVE)
#define MCG_DET_TILE 2048        // keys per LDS tile of the ranking pass (16 KB)
#define MCG_DET_OWN 4            // keys a thread ranks per pass
#define MCG_DET_MAX_DET 300
#define MCG_DET_MAX_ANCHORS (1 << 24)
#define MCG_DET_NONE 0x7fffffff

// bytes of one image's part of the workspace: keys u64 [n] | offset boxes float4 [n] | anchors int32 [n] | suppressed int32 [n]
static inline size_t detect_image_bytes(int num_anchors) { return (size_t)((num_anchors + 63) / 64 * 64) * 32; }

struct DetRow {
  float x1, y1, x2, y2, conf;
  int cls;
  bool keep;
};

// steps 1 and 2 of the header: one prediction row -> box, score, class, and whether it is a candidate
__device__ __forceinline__ DetRow detect_row(const float* __restrict__ p, int nc, float thr, int only_class) {
  DetRow r;
  const float obj = p[4];
  float conf = p[5] * obj;
  int cls = 0;
  for (int c = 1; c < nc; ++c) {                                  // max over the classes: the lowest class that reaches it; the first NaN stays
    const float s = p[5 + c] * obj;
    if (conf == conf && (s > conf || s != s)) { conf = s; cls = c; }
  }
  const float hw = p[2] / 2.0f, hh = p[3] / 2.0f;
  r.x1 = p[0] - hw; r.y1 = p[1] - hh; r.x2 = p[0] + hw; r.y2 = p[1] + hh;
  r.conf = conf;
  r.cls = cls;
  const bool finite = isfinite(r.x1) && isfinite(r.y1) && isfinite(r.x2) && isfinite(r.y2) && isfinite(conf);
  r.keep = obj > thr && conf > thr && (only_class < 0 || cls == only_class) && finite;
  return r;
}

// ascending keys = descending scores, ties by ascending anchor; -0 and +0 are one score
__device__ __forceinline__ unsigned long long detect_key(float conf, int anchor) {
  const uint32_t u = __float_as_uint(conf + 0.0f);
  const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending with the float
  return ((unsigned long long)(~ord) << 32) | (uint32_t)anchor;
}

__global__ __launch_bounds__(MCG_DET_THREADS) void detect_heads_kernel(const float* __restrict__ pred, int num_anchors, int nc, long long image_stride,
                                                                       int row_stride, int in_h, int in_w, const int32_t* __restrict__ frame_hw, float thr,
                                                                       float it, int only_class, int agnostic, int max_nms, int max_det,
                                                                       float* __restrict__ boxes, float* __restrict__ scores, int32_t* __restrict__ classes,
                                                                       int32_t* __restrict__ image_of, int32_t* __restrict__ counts,
                                                                       int32_t* __restrict__ flags, unsigned char* ws, size_t ws_image_bytes) {
  __shared__ int s_wave[2][MCG_DET_WAVES];
  __shared__ unsigned long long s_tile[MCG_DET_TILE];
  __shared__ int s_next[3];
  __shared__ int s_keep[MCG_DET_MAX_DET];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = num_anchors, cap = (n + 63) / 64 * 64;
  const float* p_img = pred + (size_t)b * image_stride;
  unsigned char* base = ws + (size_t)b * ws_image_bytes;
  unsigned long long* keys = (unsigned long long*)base;
  float4* obox = (float4*)(base + (size_t)cap * 8);
  int32_t* sidx = (int32_t*)(base + (size_t)cap * 24);
  int32_t* sup = (int32_t*)(base + (size_t)cap * 28);
  const int h0 = frame_hw[2 * b], w0 = frame_hw[2 * b + 1];
  float* o_box = boxes + (size_t)b * max_det * 4;
  float* o_score = scores + (size_t)b * max_det;
  int32_t* o_cls = classes + (size_t)b * max_det;
  int32_t* o_img = image_of + (size_t)b * max_det;

  int count = 0, flag = 0;
  if (h0 <= 0 || w0 <= 0) {
    flag = 2;                                                     // block-uniform: nothing of this image is read or divided
  } else {
    // ---------------------------------------------------------------- filter
    int m = 0;
    for (int a0 = 0, step = 0; a0 < n; a0 += MCG_DET_THREADS, ++step) {
      const int a = a0 + tid;
      DetRow r;
      r.keep = false;
      if (a < n) r = detect_row(p_img + (size_t)a * row_stride, nc, thr, only_class);
      const unsigned long long mask = __ballot(r.keep);
      if (lane == 0) s_wave[step & 1][wave] = __popcll(mask);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < MCG_DET_WAVES; ++w) {
        const int c = s_wave[step & 1][w];
        before += w < wave ? c : 0;
        total += c;
      }
      if (r.keep) keys[m + before + __popcll(mask & ((1ull << lane) - 1ull))] = detect_key(r.conf, a);   // m + ... < n: one slot per anchor
      m += total;
    }
    const int L = min(m, max_nms);
    flag = m > max_nms ? 1 : 0;
    __syncthreads();                                              // the keys are written
    // ---------------------------------------------------------------- order
    for (int j0 = 0; j0 < m; j0 += MCG_DET_THREADS * MCG_DET_OWN) {
      unsigned long long mine[MCG_DET_OWN];
      int rank[MCG_DET_OWN];
#pragma unroll
      for (int q = 0; q < MCG_DET_OWN; ++q) {
        const int j = j0 + q * MCG_DET_THREADS + tid;
        mine[q] = j < m ? keys[j] : 0ull;
        rank[q] = 0;
      }
      for (int t0 = 0; t0 < m; t0 += MCG_DET_TILE) {
        const int tn = min(MCG_DET_TILE, m - t0);
        for (int i = tid; i < tn; i += MCG_DET_THREADS) s_tile[i] = keys[t0 + i];
        __syncthreads();
        for (int i = 0; i < tn; ++i) {
          const unsigned long long k = s_tile[i];                 // one address for the block: a broadcast
#pragma unroll
          for (int q = 0; q < MCG_DET_OWN; ++q) rank[q] += k < mine[q] ? 1 : 0;
        }
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < MCG_DET_OWN; ++q) {
        const int j = j0 + q * MCG_DET_THREADS + tid;
        if (j < m && rank[q] < L) {                               // ranks are a permutation of 0 .. m - 1: rank < L <= n
          const int a = (int)(uint32_t)mine[q];
          const DetRow r = detect_row(p_img + (size_t)a * row_stride, nc, thr, only_class);
          const float o = agnostic ? 0.0f : (float)r.cls * 4096.0f;
          obox[rank[q]] = make_float4(r.x1 + o, r.y1 + o, r.x2 + o, r.y2 + o);
          sidx[rank[q]] = a;
          sup[rank[q]] = 0;
        }
      }
    }
    if (tid == 0) {
      s_next[0] = L > 0 ? 0 : MCG_DET_NONE;
      s_next[1] = MCG_DET_NONE;
      s_next[2] = MCG_DET_NONE;
    }
    __syncthreads();                                              // the sorted rows are written
    // ---------------------------------------------------------------- greedy
    int slot = 0;
    while (count < max_det) {
      const int i = s_next[slot];
      if (i == MCG_DET_NONE) break;                               // block-uniform
      const int nslot = slot == 2 ? 0 : slot + 1, rslot = nslot == 2 ? 0 : nslot + 1;
      if (tid == 0) {
        s_keep[count] = i;
        s_next[rslot] = MCG_DET_NONE;                             // read last a round ago, written next a round from now
      }
      const float4 bi = obox[i];
      const float area_i = (bi.z - bi.x) * (bi.w - bi.y);
      int j = (i + 1) / MCG_DET_THREADS * MCG_DET_THREADS + tid;  // this thread's first row behind i
      if (j <= i) j += MCG_DET_THREADS;
      int first = MCG_DET_NONE;
      for (; j < L; j += MCG_DET_THREADS) {
        if (sup[j]) continue;
        const float4 bj = obox[j];
        const float area_j = (bj.z - bj.x) * (bj.w - bj.y);
        const float dw = fminf(bi.z, bj.z) - fmaxf(bi.x, bj.x), dh = fminf(bi.w, bj.w) - fmaxf(bi.y, bj.y);   // finite boxes: no NaN enters
        const float w = dw < 0.0f ? 0.0f : dw, h = dh < 0.0f ? 0.0f : dh;
        const float inter = w * h;
        const float iou = inter / (area_i + area_j - inter);
        if (iou > it) sup[j] = 1;                                 // NaN (0 / 0, inf - inf) suppresses nothing
        else if (first == MCG_DET_NONE) first = j;
      }
      if (first != MCG_DET_NONE) atomicMin(&s_next[nslot], first);
      ++count;
      slot = nslot;
      __syncthreads();
    }
    __syncthreads();                                              // s_keep is complete
    // ---------------------------------------------------------------- output: scale_coords(...).round()
    if (tid < count) {
      const int a = sidx[s_keep[tid]];
      const DetRow r = detect_row(p_img + (size_t)a * row_stride, nc, thr, only_class);
      const double gain = fmin((double)in_h / (double)h0, (double)in_w / (double)w0);
      const double pad_x = ((double)in_w - (double)w0 * gain) / 2.0, pad_y = ((double)in_h - (double)h0 * gain) / 2.0;
      const float g = (float)gain, px = (float)pad_x, py = (float)pad_y, fw = (float)w0, fh = (float)h0;
      const float v[4] = {(r.x1 - px) / g, (r.y1 - py) / g, (r.x2 - px) / g, (r.y2 - py) / g};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float hi = (c & 1) ? fh : fw;
        float x = v[c] < 0.0f ? 0.0f : v[c];
        x = x > hi ? hi : x;
        o_box[4 * tid + c] = rintf(x);                            // half to even
      }
      o_score[tid] = r.conf;
      o_cls[tid] = r.cls;
      o_img[tid] = b;
    }
  }
  for (int k = count + tid; k < max_det; k += MCG_DET_THREADS) {  // count is block-uniform
    o_box[4 * k] = 0.0f; o_box[4 * k + 1] = 0.0f; o_box[4 * k + 2] = 0.0f; o_box[4 * k + 3] = 0.0f;
    o_score[k] = 0.0f;
    o_cls[k] = 0;
    o_img[k] = -1;
  }
  if (tid == 0) {
    counts[b] = count;
    if (flags) flags[b] = flag;
  }
}

extern "C" size_t mcg_detect_heads_workspace_bytes(int num_images, int num_anchors) {
  if (num_images < 0 || num_anchors < 1 || num_anchors > MCG_DET_MAX_ANCHORS) return 0;
  return (size_t)num_images * detect_image_bytes(num_anchors);
}

extern "C" int mcg_detect_heads(mcg_stream s, const float* pred_dev, int num_images, int num_anchors, int num_classes, long long image_stride,
                                int row_stride, int in_h, int in_w, const int32_t* frame_hw_dev, double conf_thres, double iou_thres, int only_class,
                                int agnostic, int max_nms, int max_det, float* boxes_dev, float* scores_dev, int32_t* classes_dev,
                                int32_t* image_of_dev, int32_t* counts_dev, int32_t* flags_dev, void* ws_dev, size_t ws_bytes) {
  MCG_CHECK_ARG(num_images >= 0 && num_images <= 65535, "mcg_detect_heads: 0 .. 65535 images per call (got %d)", num_images);
  MCG_CHECK_ARG(num_anchors >= 1 && num_anchors <= MCG_DET_MAX_ANCHORS, "mcg_detect_heads: 1 .. 2^24 anchors per image (got %d)", num_anchors);
  MCG_CHECK_ARG(num_classes >= 1, "mcg_detect_heads: num_classes must be at least 1 (got %d)", num_classes);
  MCG_CHECK_ARG(row_stride >= 5 && row_stride - 5 >= num_classes && image_stride >= 0,
                "mcg_detect_heads: bad strides row_stride=%d (a row holds 5 + %d floats) image_stride=%lld", row_stride, num_classes, image_stride);
  MCG_CHECK_ARG(in_h >= 1 && in_w >= 1, "mcg_detect_heads: the detector's input is at least 1 x 1 (got %d x %d)", in_h, in_w);
  MCG_CHECK_ARG(max_det >= 1 && max_det <= MCG_DET_MAX_DET, "mcg_detect_heads: max_det in 1 .. 300 (got %d)", max_det);
  MCG_CHECK_ARG(max_nms >= 1 && max_nms <= num_anchors, "mcg_detect_heads: max_nms in 1 .. num_anchors = %d (got %d)", num_anchors, max_nms);
  MCG_CHECK_ARG(conf_thres - conf_thres == 0.0 && iou_thres - iou_thres == 0.0, "mcg_detect_heads: conf_thres and iou_thres must be finite");
  if (num_images == 0) return MCG_OK;
  MCG_CHECK_ARG(pred_dev && frame_hw_dev && boxes_dev && scores_dev && classes_dev && image_of_dev && counts_dev && ws_dev,
                "mcg_detect_heads: null pointer");
  const size_t need = mcg_detect_heads_workspace_bytes(num_images, num_anchors);
  MCG_CHECK_ARG(ws_bytes >= need, "mcg_detect_heads: workspace too small (%zu bytes, need %zu)", ws_bytes, need);
  MCG_CHECK_ARG(((uintptr_t)ws_dev & 15) == 0, "mcg_detect_heads: the workspace must be 16-byte aligned");
  hipLaunchKernelGGL(detect_heads_kernel, dim3(num_images), dim3(MCG_DET_THREADS), 0, (hipStream_t)s, pred_dev, num_anchors, num_classes, image_stride,
                     row_stride, in_h, in_w, frame_hw_dev, (float)conf_thres, (float)iou_thres, only_class, agnostic ? 1 : 0, max_nms, max_det,
                     boxes_dev, scores_dev, classes_dev, image_of_dev, counts_dev, flags_dev, (unsigned char*)ws_dev, detect_image_bytes(num_anchors));
  MCG_CHECK_LAUNCH("mcg_detect_heads");
  return MCG_OK;
}
