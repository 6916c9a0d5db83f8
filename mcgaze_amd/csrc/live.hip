// Live multi-person gaze with no host step: the tracker's slots as streams of a pool.  mcg_track_heads (track.hip) decides on the device
// who is in which slot, and a pool's planning is a host function of the frames each stream was given -- so every slot of every camera is a
// stream that gets one crop per tick, and which result rows are a person's is decided here, afterwards, from a ring of the slots' ids.
// The arithmetic is stated once, in include/mcgaze_hip.h ("live: tracker slots as streams"); mcgaze_amd/live.py::live_slots_host and
// live_gate_host are the same on the host.  Two table kernels, tiny and latency-bound: one thread per row, integer compares and copies.
// A tick enters an address only as t % R after the entry that names it was found usable (every tick it names lies in the ring); q and s
// come from the thread index, below the host-checked Q and S.
#include "common.hpp"

#define MCG_LIVE_THREADS 256
#define MCG_LIVE_MAX_SLOTS 64
#define MCG_LIVE_MAX_CAMERAS 65535
#define MCG_LIVE_MAX_RING 65536
#define MCG_LIVE_MAX_ENTRIES 65536
#define MCG_LIVE_ENTRY 5        // tick, lo, hi, prev, next

static_assert(sizeof(mcg_track_header) == 16 && sizeof(mcg_track_slot) == 32, "the published state layout");

__global__ __launch_bounds__(MCG_LIVE_THREADS) void live_slots_kernel(const unsigned char* __restrict__ state, size_t seq_bytes, int Q, int S,
                                                                      int ring_row, float* __restrict__ crop_boxes,
                                                                      int32_t* __restrict__ image_of, int32_t* __restrict__ ring_id,
                                                                      float* __restrict__ ring_box, int32_t* __restrict__ matched) {
  const int row = blockIdx.x * MCG_LIVE_THREADS + threadIdx.x;    // < Q * S <= 65535 * 64
  if (row >= Q * S) return;
  const int q = row / S, s = row - q * S;
  const mcg_track_slot* slot = (const mcg_track_slot*)(state + (size_t)q * seq_bytes + sizeof(mcg_track_header)) + s;
  const int id = slot->id;
  const bool live = id > 0;
  const size_t at = (size_t)ring_row * Q * S + row;              // ring_row < R
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float v = live ? slot->box[c] : 0.0f;
    crop_boxes[4 * (size_t)row + c] = v;
    ring_box[4 * at + c] = v;
  }
  image_of[row] = live ? q : -1;
  ring_id[at] = live ? id : 0;
  matched[row] = live && slot->age == 0 ? 1 : 0;
}

struct live_entry {
  int tick, lo, hi, prev, next;
};

__device__ __forceinline__ live_entry live_load(const int32_t* __restrict__ table, int e) {
  const int32_t* p = table + (size_t)e * MCG_LIVE_ENTRY;
  return {p[0], p[1], p[2], p[3], p[4]};
}

// id and valid of entry e for the slot whose ring column is `col`; 64-bit compares: tick - R may pass below INT_MIN for no valid input only
__device__ __forceinline__ bool live_state(const live_entry& e, const int32_t* __restrict__ ring_id, int R, size_t cols, size_t col, int tick,
                                           int* id_out) {
  const long long old = (long long)tick - R;                       // ticks at or below it have left the ring
  const bool usable = e.tick > old && e.tick <= tick && e.lo >= 0 && e.lo <= e.hi && (long long)e.hi <= (long long)tick + 1 &&
                      (e.hi == e.lo || e.lo > old) && e.prev >= -1 && e.next >= -1;
  if (!usable) {
    *id_out = 0;
    return false;
  }
  const int id = ring_id[(size_t)(e.tick % R) * cols + col];
  *id_out = id;
  bool valid = id != 0;
  for (int t = e.lo; t < e.hi; ++t) valid = valid && ring_id[(size_t)(t % R) * cols + col] == id;   // at most R steps
  return valid;
}

// whether neighbour tick n (not -1) is a valid row of the same person: the first entry that names it decides
__device__ __forceinline__ bool live_neighbour(int n, int id, const int32_t* __restrict__ table, int num_entries,
                                               const int32_t* __restrict__ ring_id, int R, size_t cols, size_t col, int tick) {
  for (int j = 0; j < num_entries; ++j) {
    if (table[(size_t)j * MCG_LIVE_ENTRY] != n) continue;
    int idn;
    const bool vn = live_state(live_load(table, j), ring_id, R, cols, col, tick, &idn);
    return vn && idn == id;
  }
  return false;
}

__global__ __launch_bounds__(MCG_LIVE_THREADS) void live_gate_kernel(const int32_t* __restrict__ ring_id, const float* __restrict__ ring_box, int R,
                                                                     int Q, int S, int tick, const int32_t* __restrict__ table, int num_entries,
                                                                     int first_out, int num_out, const float* __restrict__ fused,
                                                                     const float* __restrict__ others, float* __restrict__ fused_smooth,
                                                                     float* __restrict__ others_smooth, int32_t* __restrict__ track_id,
                                                                     int32_t* __restrict__ valid_out, float* __restrict__ head_box,
                                                                     int32_t* __restrict__ image_of, int32_t* __restrict__ smooth_valid) {
  const size_t cols = (size_t)Q * S;
  const size_t row = (size_t)blockIdx.x * MCG_LIVE_THREADS + threadIdx.x;   // < num_out * Q * S < 2^31
  if (row >= (size_t)num_out * cols) return;
  const int i = (int)(row / cols);
  const size_t col = row - (size_t)i * cols;
  const int q = (int)(col / S);
  const live_entry e = live_load(table, first_out + i);            // first_out + i < num_entries
  int id;
  const bool valid = live_state(e, ring_id, R, cols, col, tick, &id);
  track_id[row] = id;
  valid_out[row] = valid ? 1 : 0;
  image_of[row] = valid ? i * Q + q : -1;
  const size_t at = valid ? (size_t)(e.tick % R) * cols + col : 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) head_box[4 * row + c] = valid ? ring_box[4 * at + c] : 0.0f;
  if (fused_smooth == nullptr) {
    if (smooth_valid != nullptr) smooth_valid[row] = valid ? 1 : 0;
    return;
  }
  bool ok = valid;
  if (ok && e.prev != -1) ok = live_neighbour(e.prev, id, table, num_entries, ring_id, R, cols, col, tick);
  if (ok && e.next != -1) ok = live_neighbour(e.next, id, table, num_entries, ring_id, R, cols, col, tick);
  smooth_valid[row] = ok ? 1 : 0;
  if (valid && !ok) {
#pragma unroll
    for (int c = 0; c < 3; ++c) fused_smooth[3 * row + c] = fused[3 * row + c];
#pragma unroll
    for (int c = 0; c < 9; ++c) others_smooth[9 * row + c] = others[9 * row + c];
  }
}

extern "C" int mcg_live_slots(mcg_stream s, const void* state_dev, int num_cameras, int slots, int tick, int ring_depth, float* crop_boxes_dev,
                              int32_t* image_of_dev, int32_t* ring_id_dev, float* ring_box_dev, int32_t* matched_dev) {
  MCG_CHECK_ARG(num_cameras >= 0 && num_cameras <= MCG_LIVE_MAX_CAMERAS, "mcg_live_slots: 0 .. 65535 cameras per call (got %d)", num_cameras);
  MCG_CHECK_ARG(slots >= 1 && slots <= MCG_LIVE_MAX_SLOTS, "mcg_live_slots: slots in 1 .. 64 (got %d)", slots);
  MCG_CHECK_ARG(tick >= 0, "mcg_live_slots: tick must not be negative (got %d)", tick);
  MCG_CHECK_ARG(ring_depth >= 1 && ring_depth <= MCG_LIVE_MAX_RING, "mcg_live_slots: ring_depth in 1 .. 65536 (got %d)", ring_depth);
  if (num_cameras == 0) return MCG_OK;
  MCG_CHECK_ARG(state_dev && crop_boxes_dev && image_of_dev && ring_id_dev && ring_box_dev && matched_dev, "mcg_live_slots: null pointer");
  MCG_CHECK_ARG(((uintptr_t)state_dev & 15) == 0, "mcg_live_slots: the state must be 16-byte aligned");
  const int rows = num_cameras * slots;                            // <= 65535 * 64
  hipLaunchKernelGGL(live_slots_kernel, dim3((rows + MCG_LIVE_THREADS - 1) / MCG_LIVE_THREADS), dim3(MCG_LIVE_THREADS), 0, (hipStream_t)s,
                     (const unsigned char*)state_dev, sizeof(mcg_track_header) + (size_t)slots * sizeof(mcg_track_slot), num_cameras, slots,
                     tick % ring_depth, crop_boxes_dev, image_of_dev, ring_id_dev, ring_box_dev, matched_dev);
  MCG_CHECK_LAUNCH("mcg_live_slots");
  return MCG_OK;
}

extern "C" int mcg_live_gate(mcg_stream s, const int32_t* ring_id_dev, const float* ring_box_dev, int ring_depth, int num_cameras, int slots,
                             int tick, const int32_t* table_dev, int num_entries, int first_out, int num_out, const float* fused_dev,
                             const float* others_dev, float* fused_smooth_dev, float* others_smooth_dev, int32_t* track_id_dev,
                             int32_t* valid_dev, float* head_box_dev, int32_t* image_of_dev, int32_t* smooth_valid_dev) {
  MCG_CHECK_ARG(num_cameras >= 0 && num_cameras <= MCG_LIVE_MAX_CAMERAS, "mcg_live_gate: 0 .. 65535 cameras per call (got %d)", num_cameras);
  MCG_CHECK_ARG(slots >= 1 && slots <= MCG_LIVE_MAX_SLOTS, "mcg_live_gate: slots in 1 .. 64 (got %d)", slots);
  MCG_CHECK_ARG(tick >= 0, "mcg_live_gate: tick must not be negative (got %d)", tick);
  MCG_CHECK_ARG(ring_depth >= 1 && ring_depth <= MCG_LIVE_MAX_RING, "mcg_live_gate: ring_depth in 1 .. 65536 (got %d)", ring_depth);
  MCG_CHECK_ARG(num_entries >= 0 && num_entries <= MCG_LIVE_MAX_ENTRIES, "mcg_live_gate: 0 .. 65536 table entries (got %d)", num_entries);
  MCG_CHECK_ARG(first_out >= 0 && num_out >= 0 && (long long)first_out + num_out <= num_entries,
                "mcg_live_gate: the frames handed out must be entries of the table (first_out %d, num_out %d, %d entries)", first_out, num_out,
                num_entries);
  MCG_CHECK_ARG((long long)num_out * num_cameras * slots < (1ll << 31), "mcg_live_gate: frames x cameras x slots must stay below 2^31");
  if (num_out == 0 || num_cameras == 0) return MCG_OK;
  MCG_CHECK_ARG(ring_id_dev && ring_box_dev && table_dev && track_id_dev && valid_dev && head_box_dev && image_of_dev, "mcg_live_gate: null pointer");
  const int given = (fused_dev != nullptr) + (others_dev != nullptr) + (fused_smooth_dev != nullptr) + (others_smooth_dev != nullptr);
  MCG_CHECK_ARG(given == 0 || (given == 4 && smooth_valid_dev), "mcg_live_gate: smoothing takes fused, others, both smoothed tables and smooth_valid, or none");
  const long long rows = (long long)num_out * num_cameras * slots;
  hipLaunchKernelGGL(live_gate_kernel, dim3((unsigned)((rows + MCG_LIVE_THREADS - 1) / MCG_LIVE_THREADS)), dim3(MCG_LIVE_THREADS), 0, (hipStream_t)s,
                     ring_id_dev, ring_box_dev, ring_depth, num_cameras, slots, tick, table_dev, num_entries, first_out, num_out, fused_dev,
                     others_dev, fused_smooth_dev, others_smooth_dev, track_id_dev, valid_dev, head_box_dev, image_of_dev, smooth_valid_dev);
  MCG_CHECK_LAUNCH("mcg_live_gate");
  return MCG_OK;
}
