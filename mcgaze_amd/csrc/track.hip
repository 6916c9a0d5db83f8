// Head identities across frames, on the device: which box of frame t is the person of which box of frame t - 1.  The demo decides that by
// the number of heads and their x1 order (MCGaze_demo/demo.ipynb, cell 1; harness.segment_tracks) on the host; this is a greedy match by
// overlap on the boxes mcg_detect_heads leaves in device memory.  The arithmetic is stated once, in include/mcgaze_hip.h ("head identities
// across frames"); mcgaze_amd/head_detect.py::track_heads_host is the same on the host.  Everything is f32 and uncontracted.
//
// One launch, one workgroup of 256 threads (4 waves) per sequence.  The sequence's slots live in LDS for the whole call and the frames are
// walked inside the kernel, so frame t sees the state frame t - 1 left; the state goes back to memory once, at the end.  Per frame:
//   load     the frame's n detections into LDS (16 bytes each, at most 1024), each marked usable (-1) or not (-2)
//   match    lane = slot in every wave, and wave w owns the detections d = w, w + 4, ...: a round is one pass over the pairs whose slot
//            and detection are both open, the IoU recomputed (64 x 1024 floats would not fit beside the rest, and a frame of a few heads
//            has a few rounds), reduced to the maximum of a 64-bit key -- the IoU's bits (it is >= 0: they order as the float does) over
//            0xffff - slot over 0xffff - detection -- by shuffles inside a wave and one 64-bit LDS atomicMax per wave.  A maximum is
//            order-free.  One barrier per round: three key cells in rotation, as in detect.hip.  The wave that owns the matched detection
//            marks it, so the mark is read and written by one wave only
//   age      wave 0, lane = slot: matched slots take their box, the others age and may be freed
//   births   wave 0: the open usable detections in index order, 64 per step, ranked by a ballot; rank r takes the r-th free slot of the
//            ballot of free slots
//   output   thread s writes row s of the frame
// No decision depends on which thread made it.
//
// mcg_track_heads_motion is the same kernel with MOTION = true ("head identities with a constant-velocity motion model" in the header):
// a slot carries a centre velocity, two f32 in the reserved words of its record and 512 bytes of LDS here.  Thread s moves slot s by its
// velocity while the frame's detections are loaded -- the barrier that ends the load makes the predicted box visible to the four waves of the
// match, so the frame has no barrier more --, and the age step, still wave 0 / lane = slot, corrects the velocity of a matched slot by the
// distance between the detection's centre and the predicted one, decays that of a coasting slot, which keeps the predicted box, and zeroes
// that of a freed one; a birth starts at rest.  The plain instantiation holds none of it and is what mcg_track_heads launches.
#include "common.hpp"

#pragma clang fp contract(off)

#define MCG_TRK_THREADS 256
#define MCG_TRK_WAVES (MCG_TRK_THREADS / MCG_WAVE)
#define MCG_TRK_MAX_SLOTS 64
#define MCG_TRK_MAX_DET 1024
#define MCG_TRK_MAX_SEQUENCES 65535

static_assert(sizeof(mcg_track_header) == 16 && sizeof(mcg_track_slot) == 32, "the published state layout");
static_assert(MCG_TRK_MAX_SLOTS == MCG_WAVE, "lane = slot");

static inline size_t track_sequence_bytes(int slots) { return sizeof(mcg_track_header) + (size_t)slots * sizeof(mcg_track_slot); }

// the index of the k-th set bit of m, which has more than k
__device__ __forceinline__ int track_kth_bit(unsigned long long m, int k) {
  for (int i = 0; i < k; ++i) m &= m - 1ull;
  return __builtin_ctzll(m);
}

// MOTION: gain and decay are g and k of the header; state_boxes may be null.  Without MOTION the three are not read.
template <bool MOTION>
__global__ __launch_bounds__(MCG_TRK_THREADS) void track_heads_kernel(const float* __restrict__ boxes, long long frame_stride,
                                                                      const int32_t* __restrict__ counts, int T, int D, int S, float thr, int max_age,
                                                                      unsigned char* state, size_t seq_bytes, float* __restrict__ slot_boxes,
                                                                      int32_t* __restrict__ image_of, int32_t* __restrict__ track_id,
                                                                      int32_t* __restrict__ age_out, int32_t* __restrict__ det_of,
                                                                      int32_t* __restrict__ flags, float gain, float decay,
                                                                      float* __restrict__ state_boxes) {
  __shared__ float s_det[MCG_TRK_MAX_DET][4];
  __shared__ int s_det_slot[MCG_TRK_MAX_DET];                     // -2 not usable, -1 open, else the slot it went to
  __shared__ float s_box[MCG_TRK_MAX_SLOTS][4];
  __shared__ int s_id[MCG_TRK_MAX_SLOTS], s_age[MCG_TRK_MAX_SLOTS], s_slot_det[MCG_TRK_MAX_SLOTS];
  __shared__ unsigned long long s_best[3];
  __shared__ int s_flag, s_next_id;
  __shared__ float s_vel[MOTION ? MCG_TRK_MAX_SLOTS : 1][2];      // the slot's centre velocity, pixels a frame
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  mcg_track_header* hdr = (mcg_track_header*)(state + (size_t)q * seq_bytes);
  mcg_track_slot* slots = (mcg_track_slot*)(hdr + 1);

  if (tid < S) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s_box[tid][c] = slots[tid].box[c];
    s_id[tid] = slots[tid].id;
    s_age[tid] = slots[tid].age;
    if constexpr (MOTION) {
      s_vel[tid][0] = __int_as_float(slots[tid].reserved[0]);
      s_vel[tid][1] = __int_as_float(slots[tid].reserved[1]);
    }
  }
  if (tid == 0) {
    s_best[0] = 0ull; s_best[1] = 0ull; s_best[2] = 0ull;
    s_flag = 0;
    s_next_id = hdr->next_id;
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const int frame = q * T + t;                                  // < 2^31 / S: checked by the entry
    const int c = counts[frame];
    const int n = c < 0 ? 0 : (c > D ? D : c);
    const float* fb = boxes + (size_t)frame * frame_stride;
    // ---------------------------------------------------------------- load
    bool bad = false;
    for (int d = tid; d < n; d += MCG_TRK_THREADS) {              // d < n <= D <= 1024
      const float x1 = fb[4 * d], y1 = fb[4 * d + 1], x2 = fb[4 * d + 2], y2 = fb[4 * d + 3];   // 4 * d + 3 < 4 * D <= frame_stride
      s_det[d][0] = x1; s_det[d][1] = y1; s_det[d][2] = x2; s_det[d][3] = y2;
      const bool ok = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
      s_det_slot[d] = ok ? -1 : -2;
      bad |= !ok;
    }
    if (bad) atomicOr(&s_flag, 2);
    if (tid < S) s_slot_det[tid] = -1;
    if constexpr (MOTION) {                                       // predict: s_box[tid] is read and written by thread tid only until the barrier
      if (tid < S && s_id[tid] > 0) {
        const float vx = s_vel[tid][0], vy = s_vel[tid][1];
        if (!(vx == 0.0f && vy == 0.0f)) {                        // a slot at rest is not touched: no + 0.0f
          const float px1 = s_box[tid][0] + vx, py1 = s_box[tid][1] + vy, px2 = s_box[tid][2] + vx, py2 = s_box[tid][3] + vy;
          if (isfinite(px1) && isfinite(py1) && isfinite(px2) && isfinite(py2)) {
            s_box[tid][0] = px1; s_box[tid][1] = py1; s_box[tid][2] = px2; s_box[tid][3] = py2;
          } else {
            s_vel[tid][0] = 0.0f; s_vel[tid][1] = 0.0f;
          }
        }
      }
    }
    __syncthreads();
    // ---------------------------------------------------------------- match
    {
      bool open = lane < S && s_id[lane] > 0;                     // lane = slot, in every wave
      const float ax1 = s_box[lane][0], ay1 = s_box[lane][1], ax2 = s_box[lane][2], ay2 = s_box[lane][3];
      const float area_a = (ax2 - ax1) * (ay2 - ay1);
      int cell = 0;
      for (;;) {                                                  // at most min(S, n) + 1 rounds: every round but the last matches a pair
        unsigned long long best = 0ull;
        for (int d = wave; d < n; d += MCG_TRK_WAVES) {
          if (s_det_slot[d] != -1) continue;                      // wave-uniform; written by this wave only
          if (open) {
            const float bx1 = s_det[d][0], by1 = s_det[d][1], bx2 = s_det[d][2], by2 = s_det[d][3];   // one address per wave: a broadcast
            const float area_b = (bx2 - bx1) * (by2 - by1);
            const float dw = fminf(ax2, bx2) - fmaxf(ax1, bx1), dh = fminf(ay2, by2) - fmaxf(ay1, by1);   // finite boxes: no NaN enters
            const float w = dw < 0.0f ? 0.0f : dw, h = dh < 0.0f ? 0.0f : dh;
            const float inter = w * h;
            const float iou = inter / (area_a + area_b - inter) + 0.0f;
            if (iou > thr) {                                      // not for a NaN; iou >= +0 here
              const unsigned long long key =
                  ((unsigned long long)__float_as_uint(iou) << 32) | ((unsigned long long)(0xffff - lane) << 16) | (unsigned long long)(0xffff - d);
              best = key > best ? key : best;
            }
          }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned long long other = __shfl_xor(best, off);
          best = other > best ? other : best;
        }
        if (lane == 0 && best != 0ull) atomicMax(&s_best[cell], best);
        __syncthreads();
        const unsigned long long k = s_best[cell];
        const int next = cell == 2 ? 0 : cell + 1, reset = next == 2 ? 0 : next + 1;
        if (tid == 0) s_best[reset] = 0ull;                       // read last a round ago, written next a round from now
        if (k == 0ull) break;                                     // block-uniform; all three cells are zero again
        const int ws = 0xffff - (int)((k >> 16) & 0xffffull), wd = 0xffff - (int)(k & 0xffffull);   // ws < S, wd < n: they were written from such a pair
        if (lane == ws) open = false;
        if ((wd & (MCG_TRK_WAVES - 1)) == wave && lane == 0) {
          s_det_slot[wd] = ws;
          s_slot_det[ws] = wd;
        }
        cell = next;
      }
    }
    __syncthreads();                                              // the marks of every wave are written
    // ---------------------------------------------------------------- age, births
    if (wave == 0) {
      int id = lane < S ? s_id[lane] : -1;                        // lanes behind the slots are neither live nor free
      if (lane < S) {
        const int d = s_slot_det[lane];
        if (d >= 0) {
          if constexpr (MOTION) {                                 // the detection's centre against the predicted one, before the box is taken
            const float rx = ((s_det[d][0] + s_det[d][2]) - (s_box[lane][0] + s_box[lane][2])) * 0.5f;
            const float ry = ((s_det[d][1] + s_det[d][3]) - (s_box[lane][1] + s_box[lane][3])) * 0.5f;
            const float gx = gain * rx, gy = gain * ry;
            const float vx = s_vel[lane][0] + gx, vy = s_vel[lane][1] + gy;
            const bool ok = isfinite(vx) && isfinite(vy);
            s_vel[lane][0] = ok ? vx : 0.0f;
            s_vel[lane][1] = ok ? vy : 0.0f;
          }
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) s_box[lane][c4] = s_det[d][c4];
          s_age[lane] = 0;
        } else if (id > 0) {
          const int a = s_age[lane] + 1;
          if (a > max_age) {
            id = 0;
            s_id[lane] = 0;
            s_age[lane] = 0;
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) s_box[lane][c4] = 0.0f;
            if constexpr (MOTION) { s_vel[lane][0] = 0.0f; s_vel[lane][1] = 0.0f; }
          } else {
            s_age[lane] = a;                                      // with MOTION the box it keeps is the predicted one
            if constexpr (MOTION) { s_vel[lane][0] = s_vel[lane][0] * decay; s_vel[lane][1] = s_vel[lane][1] * decay; }
          }
        }
      }
      const unsigned long long free_mask = __ballot(id == 0);
      const int nfree = __popcll(free_mask), first_id = s_next_id;
      int seen = 0;
      for (int d0 = 0; d0 < n; d0 += MCG_WAVE) {
        const int d = d0 + lane;
        const bool want = d < n && s_det_slot[d] == -1;
        const unsigned long long m = __ballot(want);
        const int rank = seen + __popcll(m & ((1ull << lane) - 1ull));
        if (want && rank < nfree) {
          const int sl = track_kth_bit(free_mask, rank);          // a set bit of free_mask: sl < S
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) s_box[sl][c4] = s_det[d][c4];
          s_id[sl] = first_id + 1 + rank;
          s_age[sl] = 0;
          s_slot_det[sl] = d;
          if constexpr (MOTION) { s_vel[sl][0] = 0.0f; s_vel[sl][1] = 0.0f; }   // at rest, also in a slot freed in this frame
        }
        seen += __popcll(m);
      }
      if (lane == 0) {
        s_next_id = first_id + (seen < nfree ? seen : nfree);
        if (seen > nfree) s_flag |= 1;                            // the atomics on s_flag ended at the barrier after the load
      }
    }
    __syncthreads();
    // ---------------------------------------------------------------- output
    if (tid < S) {
      const size_t o = (size_t)frame * S + tid;
      const int d = s_slot_det[tid], id = s_id[tid];
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) slot_boxes[4 * o + c4] = d >= 0 ? s_det[d][c4] : 0.0f;
      image_of[o] = d >= 0 ? frame : -1;
      det_of[o] = d;                                              // -1 unless matched or born
      track_id[o] = id;
      age_out[o] = id != 0 ? s_age[tid] : -1;
      if constexpr (MOTION) {
        if (state_boxes) {
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) state_boxes[4 * o + c4] = id > 0 ? s_box[tid][c4] : 0.0f;
        }
      }
    }
    if (tid == 0) {
      flags[frame] = s_flag | (c != n ? 4 : 0);
      s_flag = 0;
    }
    __syncthreads();                                              // the frame's detections and marks are read
  }

  if (tid < S) {
#pragma unroll
    for (int c = 0; c < 4; ++c) slots[tid].box[c] = s_box[tid][c];
    slots[tid].id = s_id[tid];
    slots[tid].age = s_age[tid];
    if constexpr (MOTION) {
      slots[tid].reserved[0] = __float_as_int(s_vel[tid][0]);
      slots[tid].reserved[1] = __float_as_int(s_vel[tid][1]);
    }
  }
  if (tid == 0) {
    hdr->next_id = s_next_id;
    hdr->frames_seen += T;
  }
}

extern "C" size_t mcg_track_state_bytes(int num_sequences, int slots) {
  if (num_sequences < 0 || num_sequences > MCG_TRK_MAX_SEQUENCES || slots < 1 || slots > MCG_TRK_MAX_SLOTS) return 0;
  return (size_t)num_sequences * track_sequence_bytes(slots);
}

// The one launch under both entries: `who` names the entry in the messages.
template <bool MOTION>
static int track_launch(const char* who, mcg_stream s, const float* boxes_dev, long long frame_stride, const int32_t* counts_dev, int num_sequences,
                        int num_frames, int max_det, int slots, double match_iou, int max_age, float gain, float decay, void* state_dev,
                        float* slot_boxes_dev, int32_t* image_of_dev, int32_t* track_id_dev, int32_t* age_dev, int32_t* det_of_dev, int32_t* flags_dev,
                        float* state_boxes_dev) {
  MCG_CHECK_ARG(num_sequences >= 0 && num_sequences <= MCG_TRK_MAX_SEQUENCES, "%s: 0 .. 65535 sequences per call (got %d)", who, num_sequences);
  MCG_CHECK_ARG(slots >= 1 && slots <= MCG_TRK_MAX_SLOTS, "%s: slots in 1 .. 64 (got %d)", who, slots);
  MCG_CHECK_ARG(max_det >= 1 && max_det <= MCG_TRK_MAX_DET, "%s: max_det in 1 .. 1024 (got %d)", who, max_det);
  MCG_CHECK_ARG(num_frames >= 1, "%s: num_frames must be at least 1 (got %d)", who, num_frames);
  MCG_CHECK_ARG((long long)num_sequences * num_frames * slots < (1ll << 31), "%s: sequences x frames x slots must stay below 2^31", who);
  MCG_CHECK_ARG(max_age >= 0, "%s: max_age must not be negative (got %d)", who, max_age);
  MCG_CHECK_ARG(match_iou - match_iou == 0.0, "%s: match_iou must be finite", who);
  MCG_CHECK_ARG(frame_stride >= 4ll * max_det, "%s: bad frame_stride %lld (a frame holds %d boxes of 4 floats)", who, frame_stride, max_det);
  if (num_sequences == 0) return MCG_OK;
  MCG_CHECK_ARG(boxes_dev && counts_dev && state_dev && slot_boxes_dev && image_of_dev && track_id_dev && age_dev && det_of_dev && flags_dev,
                "%s: null pointer", who);
  MCG_CHECK_ARG(((uintptr_t)state_dev & 15) == 0, "%s: the state must be 16-byte aligned", who);
  hipLaunchKernelGGL(track_heads_kernel<MOTION>, dim3(num_sequences), dim3(MCG_TRK_THREADS), 0, (hipStream_t)s, boxes_dev, frame_stride, counts_dev,
                     num_frames, max_det, slots, (float)match_iou, max_age, (unsigned char*)state_dev, track_sequence_bytes(slots), slot_boxes_dev,
                     image_of_dev, track_id_dev, age_dev, det_of_dev, flags_dev, gain, decay, state_boxes_dev);
  MCG_CHECK_LAUNCH(who);
  return MCG_OK;
}

extern "C" int mcg_track_heads(mcg_stream s, const float* boxes_dev, long long frame_stride, const int32_t* counts_dev, int num_sequences,
                               int num_frames, int max_det, int slots, double match_iou, int max_age, void* state_dev, float* slot_boxes_dev,
                               int32_t* image_of_dev, int32_t* track_id_dev, int32_t* age_dev, int32_t* det_of_dev, int32_t* flags_dev) {
  return track_launch<false>("mcg_track_heads", s, boxes_dev, frame_stride, counts_dev, num_sequences, num_frames, max_det, slots, match_iou, max_age,
                             0.0f, 0.0f, state_dev, slot_boxes_dev, image_of_dev, track_id_dev, age_dev, det_of_dev, flags_dev, nullptr);
}

extern "C" int mcg_track_heads_motion(mcg_stream s, const float* boxes_dev, long long frame_stride, const int32_t* counts_dev, int num_sequences,
                                      int num_frames, int max_det, int slots, double match_iou, int max_age, double velocity_gain,
                                      double coast_decay, void* state_dev, float* slot_boxes_dev, int32_t* image_of_dev, int32_t* track_id_dev,
                                      int32_t* age_dev, int32_t* det_of_dev, int32_t* flags_dev, float* state_boxes_dev) {
  const char* who = "mcg_track_heads_motion";
  MCG_CHECK_ARG(velocity_gain >= 0.0 && velocity_gain <= 1.0, "%s: velocity_gain must lie in 0 .. 1 (got %g)", who, velocity_gain);   // not for a NaN
  MCG_CHECK_ARG(coast_decay >= 0.0 && coast_decay <= 1.0, "%s: coast_decay must lie in 0 .. 1 (got %g)", who, coast_decay);
  return track_launch<true>(who, s, boxes_dev, frame_stride, counts_dev, num_sequences, num_frames, max_det, slots, match_iou, max_age,
                            (float)velocity_gain, (float)coast_decay, state_dev, slot_boxes_dev, image_of_dev, track_id_dev, age_dev, det_of_dev,
                            flags_dev, state_boxes_dev);
}
