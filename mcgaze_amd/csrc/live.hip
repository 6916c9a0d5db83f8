// Live multi-person gaze with no host step: the tracker's slots as streams of a pool.  mcg_track_heads (track.hip) decides on the device
// who is in which slot, and a pool's planning is a host function of the frames each stream was given -- so every slot of every camera is a
// stream that gets one crop per tick, and which result rows are a person's is decided here, afterwards, from a ring of the slots' ids.
// The arithmetic is stated once, in include/mcgaze_hip.h ("live: tracker slots as streams"); mcgaze_amd/live.py::live_slots_host and
// live_gate_host are the same on the host.  Two table kernels, tiny and latency-bound: one thread per row, integer compares and copies.
// A tick enters an address only as t % R after the entry that names it was found usable (every tick it names lies in the ring); q and s
// come from the thread index, below the host-checked Q and S.
// The GATE is stated once, over a ring of `cols` columns: live_gate_kernel serves mcg_live_gate (the slot ring: one column per (camera,
// slot), a column's identity is its own index) and mcg_live_gate_lanes (the lane ring: the identity is read from ring_col), and every
// argument bound of the four entries is stated once, in live_check and live_gate.
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

// id and valid of entry e for the ring column `col` (a slot, or a lane); 64-bit compares: tick - R may pass below INT_MIN for no valid input
// only.  The column is the second half of a row's identity (ids are per camera) and has to hold over the span as the id does: the lane
// ring reads it from ring_col; in the slot ring (ring_col null) it is `col` itself, and the compares on it are trivially true.
__device__ __forceinline__ bool live_state(const live_entry& e, const int32_t* __restrict__ ring_id, const int32_t* __restrict__ ring_col, int R,
                                           size_t cols, size_t col, int tick, int* id_out, int* column_out) {
  const long long old = (long long)tick - R;                       // ticks at or below it have left the ring
  const bool usable = e.tick > old && e.tick <= tick && e.lo >= 0 && e.lo <= e.hi && (long long)e.hi <= (long long)tick + 1 &&
                      (e.hi == e.lo || e.lo > old) && e.prev >= -1 && e.next >= -1;
  if (!usable) {
    *id_out = 0;
    *column_out = -1;
    return false;
  }
  const size_t own = (size_t)(e.tick % R) * cols + col;
  const int id = ring_id[own], column = ring_col != nullptr ? ring_col[own] : (int)col;    // col < cols <= 65535 * 64
  *id_out = id;
  *column_out = column;
  bool valid = id != 0;
  for (int t = e.lo; t < e.hi; ++t) {                              // at most R steps
    const size_t at = (size_t)(t % R) * cols + col;
    valid = valid && ring_id[at] == id && (ring_col == nullptr || ring_col[at] == column);
  }
  return valid;
}

// whether neighbour tick n (not -1) is a valid row of the same person: the first entry that names it decides
__device__ __forceinline__ bool live_neighbour(int n, int id, int column, const int32_t* __restrict__ table, int num_entries,
                                               const int32_t* __restrict__ ring_id, const int32_t* __restrict__ ring_col, int R, size_t cols,
                                               size_t col, int tick) {
  for (int j = 0; j < num_entries; ++j) {
    if (table[(size_t)j * MCG_LIVE_ENTRY] != n) continue;
    int idn, cn;
    const bool vn = live_state(live_load(table, j), ring_id, ring_col, R, cols, col, tick, &idn, &cn);
    return vn && idn == id && cn == column;
  }
  return false;
}

// the smoothing half of a gate row: smooth_valid, and the raw gaze where the row is valid next to a neighbour that is not
__device__ __forceinline__ void live_gate_smooth(const live_entry& e, bool valid, int id, int column, size_t row, const int32_t* __restrict__ table,
                                                 int num_entries, const int32_t* __restrict__ ring_id, const int32_t* __restrict__ ring_col, int R,
                                                 size_t cols, size_t col, int tick, const float* __restrict__ fused,
                                                 const float* __restrict__ others, float* __restrict__ fused_smooth,
                                                 float* __restrict__ others_smooth, int32_t* __restrict__ smooth_valid) {
  if (fused_smooth == nullptr) {
    if (smooth_valid != nullptr) smooth_valid[row] = valid ? 1 : 0;
    return;
  }
  bool ok = valid;
  if (ok && e.prev != -1) ok = live_neighbour(e.prev, id, column, table, num_entries, ring_id, ring_col, R, cols, col, tick);
  if (ok && e.next != -1) ok = live_neighbour(e.next, id, column, table, num_entries, ring_id, ring_col, R, cols, col, tick);
  smooth_valid[row] = ok ? 1 : 0;
  if (valid && !ok) {
#pragma unroll
    for (int c = 0; c < 3; ++c) fused_smooth[3 * row + c] = fused[3 * row + c];
#pragma unroll
    for (int c = 0; c < 9; ++c) others_smooth[9 * row + c] = others[9 * row + c];
  }
}

// The gate over a ring of `num_cols` columns: Q * S of them without ring_col (mcg_live_gate), P lanes with it (mcg_live_gate_lanes).
// camera / slot_out: null, or where to write the slot the row names.
__global__ __launch_bounds__(MCG_LIVE_THREADS) void live_gate_kernel(const int32_t* __restrict__ ring_id, const float* __restrict__ ring_box,
                                                                     const int32_t* __restrict__ ring_col, int R, int num_cols, int Q, int S, int tick,
                                                                     const int32_t* __restrict__ table, int num_entries, int first_out, int num_out,
                                                                     const float* __restrict__ fused, const float* __restrict__ others,
                                                                     float* __restrict__ fused_smooth, float* __restrict__ others_smooth,
                                                                     int32_t* __restrict__ track_id, int32_t* __restrict__ valid_out,
                                                                     int32_t* __restrict__ camera, int32_t* __restrict__ slot_out,
                                                                     float* __restrict__ head_box, int32_t* __restrict__ image_of,
                                                                     int32_t* __restrict__ smooth_valid) {
  const size_t cols = (size_t)num_cols;
  const size_t row = (size_t)blockIdx.x * MCG_LIVE_THREADS + threadIdx.x;   // < num_out * cols < 2^31
  if (row >= (size_t)num_out * cols) return;
  const int i = (int)(row / cols);
  const size_t col = row - (size_t)i * cols;
  const live_entry e = live_load(table, first_out + i);            // first_out + i < num_entries
  int id, column;
  const bool valid = live_state(e, ring_id, ring_col, R, cols, col, tick, &id, &column);
  const bool named = valid && column >= 0 && column < Q * S;       // the column is a value here, never an address; a slot ring names every valid row
  const int q = named ? column / S : -1;
  track_id[row] = id;
  valid_out[row] = valid ? 1 : 0;
  if (camera != nullptr) camera[row] = q;
  if (slot_out != nullptr) slot_out[row] = named ? column - q * S : -1;
  image_of[row] = named ? i * Q + q : -1;                          // < num_out * Q: below 2^31 for either ring
  const size_t at = valid ? (size_t)(e.tick % R) * cols + col : 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) head_box[4 * row + c] = valid ? ring_box[4 * at + c] : 0.0f;
  live_gate_smooth(e, valid, id, column, row, table, num_entries, ring_id, ring_col, R, cols, col, tick, fused, others, fused_smooth, others_smooth,
                   smooth_valid);
}

// ---------------------------------------------------------------- lanes: the occupied slots compacted into P streams
// The arithmetic is stated in include/mcgaze_hip.h ("live: occupied slots compacted into lanes"); live.py::live_lanes_host and
// live_gate_lanes_host are the same on the host.  live_lanes_kernel is ONE workgroup: the lane table (<= 1024) and the column table
// (<= 4096) live in LDS, and who takes which lane is a rank -- a wave ballot and a prefix over the waves' counts, as detect.hip compacts its
// anchors -- over ascending lanes and ascending columns, so no timing can change it.  The one atomic, a min in LDS, picks the lowest of the
// lanes that claim one column; its result does not depend on the order of arrival either.  A column enters an address only after it was
// checked against Q * S, or as a thread index.
#define MCG_LIVE_WAVES (MCG_LIVE_THREADS / 64)
#define MCG_LIVE_MAX_LANES 1024
#define MCG_LIVE_MAX_COLUMNS 4096
#define MCG_LIVE_NO_LANE 0x7fffffff

__device__ __forceinline__ const mcg_track_slot* live_slot_at(const unsigned char* __restrict__ state, size_t seq_bytes, int S, int column) {
  const int q = column / S, s = column - q * S;                    // 0 <= column < Q * S
  return (const mcg_track_slot*)(state + (size_t)q * seq_bytes + sizeof(mcg_track_header)) + s;
}

// The number of threads below this one whose flag is set, and the workgroup's total.  Every thread calls it with the same `step`, which
// counts the calls: the waves' counts are double-buffered, so one barrier per call is enough.
__device__ __forceinline__ int live_rank(bool flag, int step, int (*s_wave)[MCG_LIVE_WAVES], int* total_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(flag);
  if (lane == 0) s_wave[step & 1][wave] = __popcll(mask);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < MCG_LIVE_WAVES; ++w) {
    const int c = s_wave[step & 1][w];
    before += w < wave ? c : 0;
    total += c;
  }
  *total_out = total;
  return before + __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(MCG_LIVE_THREADS) void live_lanes_kernel(const unsigned char* __restrict__ state, size_t seq_bytes, int Q, int S, int P,
                                                                      int ring_row, int32_t* __restrict__ lane_state,
                                                                      float* __restrict__ crop_boxes, int32_t* __restrict__ image_of,
                                                                      int32_t* __restrict__ ring_id, float* __restrict__ ring_box,
                                                                      int32_t* __restrict__ ring_col, int32_t* __restrict__ lane_of,
                                                                      int32_t* __restrict__ matched, int32_t* __restrict__ overflow) {
  __shared__ int s_lane_of[MCG_LIVE_MAX_COLUMNS];                  // per column: the lane that holds it, or MCG_LIVE_NO_LANE
  __shared__ int s_id[MCG_LIVE_MAX_LANES], s_col[MCG_LIVE_MAX_LANES], s_free[MCG_LIVE_MAX_LANES];
  __shared__ int s_wave[2][MCG_LIVE_WAVES];
  const int tid = threadIdx.x, cols = Q * S;                       // P <= 1024, cols <= 4096: checked by the host
  for (int c = tid; c < cols; c += MCG_LIVE_THREADS) s_lane_of[c] = MCG_LIVE_NO_LANE;
  __syncthreads();
  // ---------------------------------------------------------------- 1. release: a lane claims its column if the slot there still has its id
  for (int p = tid; p < P; p += MCG_LIVE_THREADS) {
    const int id = lane_state[2 * p], column = lane_state[2 * p + 1];
    bool claim = id > 0 && column >= 0 && column < cols;
    if (claim) claim = live_slot_at(state, seq_bytes, S, column)->id == id;
    s_id[p] = claim ? id : 0;
    s_col[p] = claim ? column : 0;
    if (claim) atomicMin(&s_lane_of[column], p);                   // the lowest claimant keeps the slot
  }
  __syncthreads();
  int step = 0, num_free = 0;
  for (int p0 = 0; p0 < P; p0 += MCG_LIVE_THREADS, ++step) {       // the free lanes, ascending
    const int p = p0 + tid;
    bool is_free = false;
    if (p < P) {
      is_free = s_id[p] == 0 || s_lane_of[s_col[p]] != p;
      if (is_free) s_id[p] = s_col[p] = 0;
    }
    int total;
    const int k = num_free + live_rank(is_free, step, s_wave, &total);
    if (is_free) s_free[k] = p;                                    // k < P: one entry per lane
    num_free += total;
  }
  __syncthreads();                                                 // s_free, s_id and s_col are complete
  // ---------------------------------------------------------------- 2. assign: the k-th waiting slot takes the k-th free lane
  int waiting = 0;
  for (int c0 = 0; c0 < cols; c0 += MCG_LIVE_THREADS, ++step) {
    const int c = c0 + tid;
    int id = 0;
    bool waits = false;
    if (c < cols) {
      id = live_slot_at(state, seq_bytes, S, c)->id;
      waits = id > 0 && s_lane_of[c] == MCG_LIVE_NO_LANE;
    }
    int total;
    const int k = waiting + live_rank(waits, step, s_wave, &total);
    if (waits && k < num_free) {
      const int p = s_free[k];                                     // < P
      s_lane_of[c] = p;
      s_id[p] = id;
      s_col[p] = c;
    }
    waiting += total;
  }
  __syncthreads();
  // ---------------------------------------------------------------- 3. outputs
  for (int p = tid; p < P; p += MCG_LIVE_THREADS) {
    const int id = s_id[p], column = s_col[p];                     // column < cols; 0 for a free lane
    const bool held = id != 0;
    const mcg_track_slot* slot = live_slot_at(state, seq_bytes, S, column);
    const size_t at = (size_t)ring_row * P + p;                    // ring_row < R
    lane_state[2 * p] = id;
    lane_state[2 * p + 1] = column;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v = held ? slot->box[c] : 0.0f;
      crop_boxes[4 * (size_t)p + c] = v;
      ring_box[4 * at + c] = v;
    }
    image_of[p] = held ? column / S : -1;
    ring_id[at] = id;
    ring_col[at] = held ? column : -1;
    matched[p] = held && slot->age == 0 ? 1 : 0;
  }
  for (int c = tid; c < cols; c += MCG_LIVE_THREADS) lane_of[c] = s_lane_of[c] == MCG_LIVE_NO_LANE ? -1 : s_lane_of[c];
  if (tid == 0) overflow[0] = waiting > num_free ? waiting - num_free : 0;
}

// ---------------------------------------------------------------- the entries
// The bounds the four entries share, each stated once, in the order the entries always checked them; `who` opens every message.
// lanes: null for the entries of the fixed schedule.
static int live_check(const char* who, int num_cameras, int slots, const int* lanes, int tick, int ring_depth) {
  MCG_CHECK_ARG(num_cameras >= 0 && num_cameras <= MCG_LIVE_MAX_CAMERAS, "%s: 0 .. 65535 cameras per call (got %d)", who, num_cameras);
  MCG_CHECK_ARG(slots >= 1 && slots <= MCG_LIVE_MAX_SLOTS, "%s: slots in 1 .. 64 (got %d)", who, slots);
  if (lanes != nullptr) {
    MCG_CHECK_ARG((long long)num_cameras * slots <= MCG_LIVE_MAX_COLUMNS, "%s: cameras x slots must not exceed 4096 (got %d x %d)", who, num_cameras,
                  slots);
    MCG_CHECK_ARG(*lanes >= 1 && *lanes <= MCG_LIVE_MAX_LANES, "%s: lanes in 1 .. 1024 (got %d)", who, *lanes);
  }
  MCG_CHECK_ARG(tick >= 0, "%s: tick must not be negative (got %d)", who, tick);
  MCG_CHECK_ARG(ring_depth >= 1 && ring_depth <= MCG_LIVE_MAX_RING, "%s: ring_depth in 1 .. 65536 (got %d)", who, ring_depth);
  return MCG_OK;
}

extern "C" int mcg_live_slots(mcg_stream s, const void* state_dev, int num_cameras, int slots, int tick, int ring_depth, float* crop_boxes_dev,
                              int32_t* image_of_dev, int32_t* ring_id_dev, float* ring_box_dev, int32_t* matched_dev) {
  MCG_TRY(live_check("mcg_live_slots", num_cameras, slots, nullptr, tick, ring_depth));
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

extern "C" int mcg_live_lanes(mcg_stream s, const void* state_dev, int num_cameras, int slots, int lanes, int tick, int ring_depth,
                              int32_t* lane_state_dev, float* crop_boxes_dev, int32_t* image_of_dev, int32_t* ring_id_dev, float* ring_box_dev,
                              int32_t* ring_col_dev, int32_t* lane_of_dev, int32_t* matched_dev, int32_t* overflow_dev) {
  MCG_TRY(live_check("mcg_live_lanes", num_cameras, slots, &lanes, tick, ring_depth));
  if (num_cameras == 0) return MCG_OK;
  MCG_CHECK_ARG(state_dev && lane_state_dev && crop_boxes_dev && image_of_dev && ring_id_dev && ring_box_dev && ring_col_dev && lane_of_dev &&
                    matched_dev && overflow_dev,
                "mcg_live_lanes: null pointer");
  MCG_CHECK_ARG(((uintptr_t)state_dev & 15) == 0, "mcg_live_lanes: the state must be 16-byte aligned");
  hipLaunchKernelGGL(live_lanes_kernel, dim3(1), dim3(MCG_LIVE_THREADS), 0, (hipStream_t)s, (const unsigned char*)state_dev,
                     sizeof(mcg_track_header) + (size_t)slots * sizeof(mcg_track_slot), num_cameras, slots, lanes, tick % ring_depth,
                     lane_state_dev, crop_boxes_dev, image_of_dev, ring_id_dev, ring_box_dev, ring_col_dev, lane_of_dev, matched_dev, overflow_dev);
  MCG_CHECK_LAUNCH("mcg_live_lanes");
  return MCG_OK;
}

// Both gates: the bounds of the table and the launch.  lanes null: the slot ring of Q * S columns, no ring_col, no camera / slot outputs;
// otherwise the lane ring of *lanes columns, and all three are required.
static int live_gate(const char* who, mcg_stream s, const int32_t* ring_id, const float* ring_box, const int32_t* ring_col, int ring_depth,
                     int num_cameras, int slots, const int* lanes, int tick, const int32_t* table, int num_entries, int first_out, int num_out,
                     const float* fused, const float* others, float* fused_smooth, float* others_smooth, int32_t* track_id, int32_t* valid,
                     int32_t* camera, int32_t* slot, float* head_box, int32_t* image_of, int32_t* smooth_valid) {
  MCG_TRY(live_check(who, num_cameras, slots, lanes, tick, ring_depth));
  MCG_CHECK_ARG(num_entries >= 0 && num_entries <= MCG_LIVE_MAX_ENTRIES, "%s: 0 .. 65536 table entries (got %d)", who, num_entries);
  MCG_CHECK_ARG(first_out >= 0 && num_out >= 0 && (long long)first_out + num_out <= num_entries,
                "%s: the frames handed out must be entries of the table (first_out %d, num_out %d, %d entries)", who, first_out, num_out, num_entries);
  const int cols = lanes != nullptr ? *lanes : num_cameras * slots;          // <= 65535 * 64
  const long long rows = (long long)num_out * cols;
  MCG_CHECK_ARG(rows < (1ll << 31), "%s: frames x %s must stay below 2^31", who, lanes != nullptr ? "lanes" : "cameras x slots");
  if (num_out == 0 || num_cameras == 0) return MCG_OK;
  MCG_CHECK_ARG(ring_id && ring_box && table && track_id && valid && head_box && image_of && (lanes == nullptr || (ring_col && camera && slot)),
                "%s: null pointer", who);
  const int given = (fused != nullptr) + (others != nullptr) + (fused_smooth != nullptr) + (others_smooth != nullptr);
  MCG_CHECK_ARG(given == 0 || (given == 4 && smooth_valid), "%s: smoothing takes fused, others, both smoothed tables and smooth_valid, or none", who);
  hipLaunchKernelGGL(live_gate_kernel, dim3((unsigned)((rows + MCG_LIVE_THREADS - 1) / MCG_LIVE_THREADS)), dim3(MCG_LIVE_THREADS), 0, (hipStream_t)s,
                     ring_id, ring_box, ring_col, ring_depth, cols, num_cameras, slots, tick, table, num_entries, first_out, num_out, fused, others,
                     fused_smooth, others_smooth, track_id, valid, camera, slot, head_box, image_of, smooth_valid);
  MCG_CHECK_LAUNCH(who);
  return MCG_OK;
}

extern "C" int mcg_live_gate(mcg_stream s, const int32_t* ring_id_dev, const float* ring_box_dev, int ring_depth, int num_cameras, int slots,
                             int tick, const int32_t* table_dev, int num_entries, int first_out, int num_out, const float* fused_dev,
                             const float* others_dev, float* fused_smooth_dev, float* others_smooth_dev, int32_t* track_id_dev,
                             int32_t* valid_dev, float* head_box_dev, int32_t* image_of_dev, int32_t* smooth_valid_dev) {
  return live_gate("mcg_live_gate", s, ring_id_dev, ring_box_dev, nullptr, ring_depth, num_cameras, slots, nullptr, tick, table_dev, num_entries,
                   first_out, num_out, fused_dev, others_dev, fused_smooth_dev, others_smooth_dev, track_id_dev, valid_dev, nullptr, nullptr,
                   head_box_dev, image_of_dev, smooth_valid_dev);
}

extern "C" int mcg_live_gate_lanes(mcg_stream s, const int32_t* ring_id_dev, const float* ring_box_dev, const int32_t* ring_col_dev, int ring_depth,
                                   int num_cameras, int slots, int lanes, int tick, const int32_t* table_dev, int num_entries, int first_out,
                                   int num_out, const float* fused_dev, const float* others_dev, float* fused_smooth_dev, float* others_smooth_dev,
                                   int32_t* track_id_dev, int32_t* valid_dev, int32_t* camera_dev, int32_t* slot_dev, float* head_box_dev,
                                   int32_t* image_of_dev, int32_t* smooth_valid_dev) {
  return live_gate("mcg_live_gate_lanes", s, ring_id_dev, ring_box_dev, ring_col_dev, ring_depth, num_cameras, slots, &lanes, tick, table_dev,
                   num_entries, first_out, num_out, fused_dev, others_dev, fused_smooth_dev, others_smooth_dev, track_id_dev, valid_dev, camera_dev,
                   slot_dev, head_box_dev, image_of_dev, smooth_valid_dev);
}
