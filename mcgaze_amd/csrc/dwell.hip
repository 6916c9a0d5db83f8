// Gaze dwell on the device: how long each person looks at what.  The per-frame targets of mcg_gaze_targets become debounced EPISODES with a
// start, a length and an end, and the person-frames every region collected.  The arithmetic is stated once, in include/mcgaze_hip.h ("gaze
// dwell"); mcgaze_amd/attention.py::gaze_dwell_host is the same on the host, bit for bit.
//
// Two launches.  gaze_dwell_kernel: one thread per COLUMN, 256-thread workgroups; the 16 state words of the column stay in registers across
// the frame loop, loaded once and stored once as four 16-byte vectors.  The [F][R] tables are read coalesced across the columns, four
// frames ahead of the walk (the loads do not depend on the state, so one memory latency is paid per four frames, not per frame), and
// `dwell` / `ended` go out as 16-byte stores.  The one atomic in global memory is the integer add into region_frames: its sum does not
// depend on the order of arrival, and its index is range-checked first.  gaze_dwell_events_kernel: ONE workgroup of 1024 threads walks
// the F * R rows of `ended` in tiles; a row's place among the events is a rank -- a wave64 ballot and popcount within the wave, the waves'
// counts through LDS, a running base carried from tile to tile --, so the order is ascending (frame, column) whatever the timing.  Every
// sum is unsigned (modulo 2^32); every index is a thread index below a checked bound or was range-checked.  No scratch; LDS: 2 x 16 words.
#include "common.hpp"

#define MCG_DWELL_COLUMNS 4096
#define MCG_DWELL_ROWS 65536
#define MCG_DWELL_REGIONS 4096
#define MCG_DWELL_EVENTS 65536
#define MCG_DWELL_FRAMES 65536   // the bound of enter and exit
#define MCG_DWELL_THREADS 256
#define MCG_DWELL_AHEAD 4        // frames whose inputs are in flight
#define MCG_DWELL_EVENT_THREADS 1024
#define MCG_DWELL_EVENT_WAVES (MCG_DWELL_EVENT_THREADS / 64)

__global__ __launch_bounds__(MCG_DWELL_THREADS) void gaze_dwell_kernel(const int32_t* __restrict__ person, const int32_t* __restrict__ tag,
                                                                       const int32_t* __restrict__ kind, const int32_t* __restrict__ ident,
                                                                       const int32_t* __restrict__ mutual, int F, int R, uint32_t frame0,
                                                                       int enter, int exit_, int32_t* __restrict__ state,
                                                                       int32_t* __restrict__ region_frames, int M, int32_t* __restrict__ dwell,
                                                                       int32_t* __restrict__ ended) {
  const int c = blockIdx.x * MCG_DWELL_THREADS + threadIdx.x;
  if (c >= R) return;                                            // (no barrier below)
  int4* srow = reinterpret_cast<int4*>(state) + 4 * (size_t)c;
  const int4 s0 = srow[0], s1 = srow[1], s2 = srow[2], s3 = srow[3];
  int s_person = s0.x, s_tag = s0.y, cur_kind = s0.z, cur_ident = s0.w;
  uint32_t cur_start = s1.x, cur_frames = s1.y, cur_mutual = s1.z, gap = s1.w;
  int cand_kind = s2.x, cand_ident = s2.y;
  uint32_t cand_start = s2.z, cand_frames = s2.w, cand_mutual = s3.x, seen = s3.y;
  for (int f0 = 0; f0 < F; f0 += MCG_DWELL_AHEAD) {
    int in_p[MCG_DWELL_AHEAD], in_g[MCG_DWELL_AHEAD], in_k[MCG_DWELL_AHEAD], in_i[MCG_DWELL_AHEAD], in_m[MCG_DWELL_AHEAD];
#pragma unroll
    for (int a = 0; a < MCG_DWELL_AHEAD; ++a) {
      const size_t at = (size_t)(f0 + a) * R + c;                // f0 + a < F is checked: at < F * R <= 65536
      const bool in = f0 + a < F;
      in_p[a] = in ? person[at] : 0;
      in_g[a] = in && tag != nullptr ? tag[at] : 0;
      in_k[a] = in ? kind[at] : 0;
      in_i[a] = in ? ident[at] : 0;
      in_m[a] = in ? mutual[at] : 0;
    }
#pragma unroll
    for (int a = 0; a < MCG_DWELL_AHEAD; ++a) {
      if (f0 + a >= F) break;
      const size_t at = (size_t)(f0 + a) * R + c;
      const uint32_t n = frame0 + (uint32_t)(f0 + a);
      const int p = in_p[a] > 0 ? in_p[a] : 0, g = p ? in_g[a] : 0;
      const int k = in_k[a] >= 1 && in_k[a] <= 3 ? in_k[a] : 0;
      const int i = k == 1 || k == 2 ? in_i[a] : 0;
      const uint32_t m = k == 1 && in_m[a] != 0;
      int4 e0 = make_int4(0, 0, 0, 0), e1 = make_int4(0, 0, 0, 0);
      // ---- A. owner
      if (s_person != 0 && (s_person != p || s_tag != g)) {
        if (cur_kind != 0) {
          e0 = make_int4(s_person, s_tag, cur_kind, cur_ident);
          e1 = make_int4((int)cur_start, (int)cur_frames, (int)cur_mutual, 2);
        }
        s_person = s_tag = cur_kind = cur_ident = cand_kind = cand_ident = 0;
        cur_start = cur_frames = cur_mutual = gap = cand_start = cand_frames = cand_mutual = seen = 0u;
      }
      if (p != 0) {
        s_person = p;
        s_tag = g;
        // ---- B. raw person-frames
        seen += 1u;
        if (k == 2 && i >= 0 && i < M) atomicAdd(reinterpret_cast<unsigned int*>(region_frames) + i, 1u);
        // ---- C. the current target
        bool is_current = false;
        if (cur_kind != 0) {
          if (k == cur_kind && i == cur_ident) {
            cur_frames += 1u + gap;
            gap = 0u;
            cur_mutual += m;
            cand_kind = cand_ident = 0;
            cand_start = cand_frames = cand_mutual = 0u;
            is_current = true;
          } else {
            gap += 1u;
            if ((int)gap > exit_) {
              e0 = make_int4(s_person, s_tag, cur_kind, cur_ident);
              e1 = make_int4((int)cur_start, (int)cur_frames, (int)cur_mutual, 1);
              cur_kind = cur_ident = 0;
              cur_start = cur_frames = cur_mutual = gap = 0u;
            }
          }
        }
        // ---- D. the candidate
        if (!is_current) {
          if (k == 0) {
            cand_kind = cand_ident = 0;
            cand_start = cand_frames = cand_mutual = 0u;
          } else if (k == cand_kind && i == cand_ident) {
            cand_frames += 1u;
            cand_mutual += m;
          } else {
            cand_kind = k;
            cand_ident = i;
            cand_start = n;
            cand_frames = 1u;
            cand_mutual = m;
          }
          if ((int)cand_frames >= enter) {
            if (cur_kind != 0) {                                 // (C ended nothing: it would have cleared cur_kind)
              e0 = make_int4(s_person, s_tag, cur_kind, cur_ident);
              e1 = make_int4((int)cur_start, (int)cur_frames, (int)cur_mutual, 3);
            }
            cur_kind = cand_kind;
            cur_ident = cand_ident;
            cur_start = cand_start;
            cur_frames = cand_frames;
            cur_mutual = cand_mutual;
            gap = 0u;
            cand_kind = cand_ident = 0;
            cand_start = cand_frames = cand_mutual = 0u;
          }
        }
      }
      // ---- E. outputs
      reinterpret_cast<int4*>(dwell)[at] = p != 0 ? make_int4(cur_kind, cur_ident, (int)cur_start, (int)cur_frames) : make_int4(0, 0, 0, 0);
      reinterpret_cast<int4*>(ended)[2 * at] = e0;
      reinterpret_cast<int4*>(ended)[2 * at + 1] = e1;
    }
  }
  srow[0] = make_int4(s_person, s_tag, cur_kind, cur_ident);
  srow[1] = make_int4((int)cur_start, (int)cur_frames, (int)cur_mutual, (int)gap);
  srow[2] = make_int4(cand_kind, cand_ident, (int)cand_start, (int)cand_frames);
  srow[3] = make_int4((int)cand_mutual, (int)seen, 0, 0);
}

__global__ __launch_bounds__(MCG_DWELL_EVENT_THREADS) void gaze_dwell_events_kernel(const int32_t* __restrict__ ended, int rows, int R, uint32_t frame0,
                                                                                    int32_t* __restrict__ events, int E,
                                                                                    int32_t* __restrict__ num_events) {
  __shared__ int s_wave[2][MCG_DWELL_EVENT_WAVES];               // double-buffered: one barrier per tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0, step = 0;
  for (int r0 = 0; r0 < rows; r0 += MCG_DWELL_EVENT_THREADS, ++step) {     // uniform: every thread walks every tile
    const int r = r0 + tid;
    int4 e0 = make_int4(0, 0, 0, 0), e1 = make_int4(0, 0, 0, 0);
    if (r < rows) {
      e0 = reinterpret_cast<const int4*>(ended)[2 * (size_t)r];
      e1 = reinterpret_cast<const int4*>(ended)[2 * (size_t)r + 1];
    }
    const bool flag = (e0.x | e0.y | e0.z | e0.w | e1.x | e1.y | e1.z | e1.w) != 0;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) s_wave[step & 1][wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < MCG_DWELL_EVENT_WAVES; ++w) {
      const int n = s_wave[step & 1][w];
      before += w < wave ? n : 0;
      total += n;
    }
    const int rank = base + before + __popcll(mask & ((1ull << lane) - 1ull));
    if (flag && rank < E) {                                      // rank < E <= 65536: inside events [E][10]
      const int f = r / R;
      int2* out = reinterpret_cast<int2*>(events + 10 * (size_t)rank);
      out[0] = make_int2((int)(frame0 + (uint32_t)f), r - f * R);
      out[1] = make_int2(e0.x, e0.y);
      out[2] = make_int2(e0.z, e0.w);
      out[3] = make_int2(e1.x, e1.y);
      out[4] = make_int2(e1.z, e1.w);
    }
    base += total;
  }
  if (tid == 0) num_events[0] = base;
}

extern "C" int mcg_gaze_dwell(mcg_stream stream, const int32_t* person_dev, const int32_t* tag_dev, const int32_t* kind_dev, const int32_t* ident_dev,
                              const int32_t* mutual_dev, int num_frames, int columns, int frame0, int enter, int exit_frames, int32_t* state_dev,
                              int32_t* region_frames_dev, int num_regions, int32_t* dwell_dev, int32_t* ended_dev, int32_t* events_dev, int max_events,
                              int32_t* num_events_dev) {
  const char* what = "mcg_gaze_dwell";
  MCG_CHECK_ARG(columns >= 1 && columns <= MCG_DWELL_COLUMNS, "%s: 1 .. %d columns per call (got %d)", what, MCG_DWELL_COLUMNS, columns);
  MCG_CHECK_ARG(num_frames >= 0 && (long long)num_frames * columns <= MCG_DWELL_ROWS, "%s: frames >= 0 and frames x columns <= %d (got %d x %d)", what,
                MCG_DWELL_ROWS, num_frames, columns);
  MCG_CHECK_ARG(num_regions >= 0 && num_regions <= MCG_DWELL_REGIONS, "%s: 0 .. %d regions per call (got %d)", what, MCG_DWELL_REGIONS, num_regions);
  MCG_CHECK_ARG(max_events >= 0 && max_events <= MCG_DWELL_EVENTS, "%s: 0 .. %d events per call (got %d)", what, MCG_DWELL_EVENTS, max_events);
  MCG_CHECK_ARG(frame0 >= 0, "%s: frame0 must not be negative (got %d)", what, frame0);
  MCG_CHECK_ARG(enter >= 1 && enter <= MCG_DWELL_FRAMES && exit_frames >= 0 && exit_frames <= MCG_DWELL_FRAMES,
                "%s: enter in 1 .. %d and exit in 0 .. %d (got %d, %d)", what, MCG_DWELL_FRAMES, MCG_DWELL_FRAMES, enter, exit_frames);
  MCG_CHECK_ARG(state_dev, "%s: null pointer (state)", what);
  MCG_CHECK_ARG((region_frames_dev == nullptr) == (num_regions == 0), "%s: region_frames is NULL iff there are no regions (num_regions=%d)", what,
                num_regions);
  MCG_CHECK_ARG(num_frames == 0 || (person_dev && kind_dev && ident_dev && mutual_dev && dwell_dev && ended_dev), "%s: null pointer", what);
  MCG_CHECK_ARG(events_dev != nullptr || max_events == 0, "%s: null events table with max_events=%d", what, max_events);
  MCG_CHECK_ARG(events_dev == nullptr || num_events_dev != nullptr, "%s: null pointer (num_events)", what);
  MCG_CHECK_ARG((((uintptr_t)state_dev | (uintptr_t)dwell_dev | (uintptr_t)ended_dev) & 15) == 0 && ((uintptr_t)events_dev & 7) == 0,
                "%s: state, dwell and ended must be 16-byte aligned, events 8-byte aligned", what);
  if (num_frames == 0) return MCG_OK;
  hipLaunchKernelGGL(gaze_dwell_kernel, dim3((columns + MCG_DWELL_THREADS - 1) / MCG_DWELL_THREADS), dim3(MCG_DWELL_THREADS), 0, (hipStream_t)stream,
                     person_dev, tag_dev, kind_dev, ident_dev, mutual_dev, num_frames, columns, (uint32_t)frame0, enter, exit_frames, state_dev,
                     region_frames_dev, num_regions, dwell_dev, ended_dev);
  MCG_CHECK_LAUNCH(what);
  if (events_dev == nullptr) return MCG_OK;
  hipLaunchKernelGGL(gaze_dwell_events_kernel, dim3(1), dim3(MCG_DWELL_EVENT_THREADS), 0, (hipStream_t)stream, ended_dev, num_frames * columns, columns,
                     (uint32_t)frame0, events_dev, max_events, num_events_dev);
  MCG_CHECK_LAUNCH("mcg_gaze_dwell (events)");
  return MCG_OK;
}
