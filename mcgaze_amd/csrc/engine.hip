// Engine: enqueues the whole per-clip forward path (trunk -> query init -> 4 x [RoIAlign + decoder
// stage] -> gaze head) from a single C-ABI call, ordered on the caller's HIP stream.  No allocation, no host sync:
// every intermediate lives in the caller-provided workspace.
//
// The trunk of a large batch runs as `trunk_streams` (option, default 2) frame ranges on concurrent streams -- the caller's plus
// side streams the engine owns, forked and joined with events so the call still behaves as one operation on the caller's
// stream.  Frames are independent, so results do not change; what changes is that the last, partly filled round of
// workgroups of one range's kernel (layer3 at 14x14 has 343 output tiles for 256 CUs) overlaps with the other range's
// kernels: 448 frames 9.36 -> 8.75 ms (tools/lab/trunk_two_streams.py).
#include "igemm.hpp"
#include "pw_pair.hpp"
#include "pw_single.hpp"
#include "bneck_x3.hpp"
#include "pw_single_x3.hpp"
#include "wino_x3.hpp"

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

int launch_roi_align(hipStream_t s, mcg_dtype dt, const void* const feats[4], const int feat_h[4], const int feat_w[4],
                     const int strides[4], int C, const float* boxes, int num_boxes, int boxes_per_frame, const int32_t* frame_of,
                     int pyramid_frames, void* out, int32_t* levels_out);
int launch_init_queries(hipStream_t s, mcg_dtype dt, const float* init_boxes, const void* init_feats, const int* img_hw,
                        const int32_t* frame_of, int pyramid_frames, int H, int W, float* boxes, void* obj, int N);
bool roi_mark_supported(int H, int W);
int launch_defer_clear(hipStream_t s, int* p, int n);
int launch_roi_mark(hipStream_t s, const float* boxes, int num_boxes, int boxes_per_frame, int level, int H, int W, int stride, int* state,
                    int* list, int* count, int* const* frame_state, int* const* frame_list, int* const* frame_count);
int launch_inner_mark(hipStream_t s, const int* out_list, const int* out_count, int H, int W, int nblk, int* state, int* list, int* count);

struct mcg_engine {
  mcg_dtype dt;
  int blocks[4];
  mcg_conv_weights stem;
  std::vector<mcg_conv_weights> convs;
  mcg_conv_weights lateral[4], fpn_out[4], c3_ds[4];
  std::vector<mcg_fused_block> fused;   // f16x3: fused bottleneck tails (bneck_x3.hpp), looked up by conv2 index
  bool bneck_fused = true;
  bool bneck_blocked = true;            // tensors that only travel between two fused tails use the kernel's blocked layout (bneck_x3.hpp)
  int winograd = 1;            // f16x3: stride-1 3x3 convs with a Winograd-packed weight copy run wino_x3.hpp: 0 off, 1 (default) F(2,3) (mcg_conv_weights.wf),
                               // 2 F(4,3) where the layer's shape allows it and the weights carry that copy (wf4), F(2,3) elsewhere: 6 % faster on
                               // the 56-wide maps for four times the operator error -- opt-in
  int wino_tile = -1;          // tile of the F(2,3) kernel: -1 (default) by grid size (the one-wave-per-SIMD tile on grids >= 130 workgroups), 0 / 1 / 2 = the 8- and
                               // 4-wave tiles of wino_x3_kernel forced, 3 = wino_x3w_kernel forced.  Every tile gives the same bits; 0 is the run-time
                               // fallback for wino_x3w_kernel, whose hand-issued register loads depend on a spill-free build (csrc/check_resources.py)
  int fpn_deferred = 1;        // f16x3: the FPN P2 output conv is deferred to the decoder and computed per 8 x 8 block where RoIAlign reads
                               // (mcg_*_deferred, mcg_clip_forward); 0 = every level dense in the trunk.  Same bits either way
  int fpn_lateral_deferred = 1; // with fpn_deferred: the P2 lateral (+ top-down add) is left to the decoder too and computed for the listed blocks
                               // and their neighbours only (pw_single_x3_blocks_kernel); 0 = the dense lateral in the trunk.  Same bits either way
  int fpn_levels_deferred = 1; // with fpn_deferred: output convs of P3 .. P5 left to the decoder and computed per FRAME, for the frames some box of a stage
                               // reads on that level (wino_x3w_frames_kernel).  0 = dense in the trunk, 1 = the default set kDeferLevelsDefault,
                               // >= 2 = a mask of levels (2 = P3, 4 = P4, 8 = P5).  Same bits either way
  static constexpr int kDeferLevelsDefault = 8;   // P5: the only level a 224-pixel frame's boxes leave unread (profiles/fpn_levels_deferred_*.md)
  // range audit (debug option, f32-storage engines): per activation tensor the trunk writes, how many values lie beyond the fp16 range
  // (|x| > 65504: an f16x3 operand half would saturate) and how many are not finite.  Counters live on the device; read by mcg_engine_range_audit.
  static constexpr int kAuditCap = 256;
  unsigned long long* audit_dev = nullptr;       // [kAuditCap][2]
  std::vector<std::string> audit_names;          // filled by the first chunk that runs with the audit on
  const float* init_boxes;
  const void* init_feats;
  int num_stages;
  std::vector<const void*> stage_w;  // [num_stages][MCG_SW_COUNT]
  const void* gaze_w[MCG_GW_COUNT];
  float stds[4];
  static constexpr int kMaxSplit = 4, kCandidates = 8;
  struct StreamPool* pool = nullptr;             // this device's side-stream candidates (shared by every engine on the device)
  hipStream_t* cand = nullptr;                   // = pool->cand
  hipEvent_t ev_fork = nullptr, ev_join[kMaxSplit - 1] = {};
  // options (mcg_engine_set_option) and observers: read at create time or set explicitly, never from the environment
  McgCtx ctx;                  // kernel-variant switches + profiling sink handed to every launcher
  Prof prof;                   // per-launch event records (mcg_engine_profile_start / _stop)
  int trunk_streams = 2;       // concurrent frame ranges of the trunk
  int max_range_frames = 0;    // 0 = what fits the 2 GiB descriptor window
  bool pw_single = true;       // HBM-bound 1x1 convs of layer2 / the P2 lateral (bf16): persistent register-resident-weight kernel (pw_single.hpp)
  bool pw_pair = true;         // layer1 / layer2 (bf16): conv3 (+ residual) and the next block's conv1 as one kernel (pw_pair.hpp)
  std::mutex mu;               // one forward at a time per engine: the fork/join events and side streams are shared state
};
// Side-stream candidates are created ONCE per device and shared by every engine of the process.  Measured (tools/lab/leg_order_probe.py):
// streams created later in a process's life land on hardware queues that serialise against the earlier ones -- a second engine
// with its own fresh streams ran its trunk 20 % slower than the first (bf16 9.7 -> 11.7 ms per 64 clips) no matter whether the
// first had been destroyed.  The pool is immutable after creation (guarded by a mutex while it is built and while the per-caller-
// stream probe result is cached); it lives until process exit.
struct StreamPool {
  hipStream_t cand[mcg_engine::kCandidates] = {};
  hipEvent_t ev_probe[3] = {};
  std::map<hipStream_t, std::vector<int>> side_of;  // caller stream -> candidates on OTHER hardware queues (probed once)
  std::mutex mu;
  bool ok = false;
};
static StreamPool* stream_pool_for_current_device() {
  static std::mutex g_mu;
  static std::map<int, StreamPool*> g_pools;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_pools.find(dev);
  if (it != g_pools.end()) return it->second;
  StreamPool* p = new StreamPool();
  bool ok = true;
  // The ROCm runtime packs the streams of a priority level onto at most GPU_MAX_HW_QUEUES (4) hardware queues, and two streams on
  // one hardware queue execute in submission order INCLUDING each other's event waits: a frame range on a stream that shares a
  // queue with the caller's runs after it, not beside it (10.1 ms instead of 8.75 for 448 frames).  Which streams share a queue
  // depends on every stream the process has created, so the pool keeps several candidates and, the first time it sees a caller
  // stream, measures which of them actually run concurrently with it (side_streams_for).
  for (int i = 0; i < mcg_engine::kCandidates; ++i) ok = ok && hipStreamCreateWithFlags(&p->cand[i], hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; i < 3; ++i) ok = ok && hipEventCreate(&p->ev_probe[i]) == hipSuccess;
  p->ok = ok;
  g_pools[dev] = p;
  return p;
}
// ~150 us of wall clock (s_memrealtime ticks at 100 MHz), one wave
__global__ void probe_spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) {}
}
// Candidates that run CONCURRENTLY with caller stream s, best effort and cached per stream.  A first-call cost of about a
// millisecond and a host wait (set-up, not the hot path).
static const std::vector<int>& side_streams_for(mcg_engine* e, hipStream_t s) {
  StreamPool* p = e->pool;
  std::lock_guard<std::mutex> lock(p->mu);
  auto it = p->side_of.find(s);
  if (it != p->side_of.end()) return it->second;
  std::vector<int> good, rest;
  const long long ticks = 15000;
  for (int c = 0; c < mcg_engine::kCandidates; ++c) {
    bool concurrent = false;
    if (hipEventRecord(p->ev_probe[0], s) == hipSuccess) {
      hipLaunchKernelGGL(probe_spin_kernel, dim3(1), dim3(64), 0, s, ticks);
      hipLaunchKernelGGL(probe_spin_kernel, dim3(1), dim3(64), 0, p->cand[c], ticks);
      float ms = 0.f;
      if (hipEventRecord(p->ev_probe[1], s) == hipSuccess && hipEventRecord(p->ev_probe[2], p->cand[c]) == hipSuccess &&
          hipEventSynchronize(p->ev_probe[1]) == hipSuccess && hipEventSynchronize(p->ev_probe[2]) == hipSuccess &&
          hipEventElapsedTime(&ms, p->ev_probe[0], p->ev_probe[2]) == hipSuccess)
        concurrent = ms < 0.15f * 1.6f;  // both spins inside ~1.6 spin lengths: they overlapped
    }
    (concurrent ? good : rest).push_back(c);
  }
  (void)hipGetLastError();
  good.insert(good.end(), rest.begin(), rest.end());  // fall back to serialised candidates rather than fail
  return p->side_of.emplace(s, good).first->second;
}
// Frames per launch sequence are capped so that the largest activation of a range ([n, H/4, W/4, 256]) stays inside the 2 GiB
// window of the contraction kernel's buffer descriptors (beyond it every conv would fall back to the slower register-staged
// kernel): 1337 frames at 224x224 bf16.  The `max_range_frames` option lowers the cap (tests).
static int range_frame_cap(const mcg_engine* e, int H, int W) {
  const long long per_frame = (long long)(H / 4) * (W / 4) * 256 * (mcg_is16(e->dt) ? 2 : 4);
  long long cap = 0x7FFFFF00ll / (per_frame > 0 ? per_frame : 1);
  if (e->max_range_frames > 0 && e->max_range_frames < cap) cap = e->max_range_frames;
  return cap < 1 ? 1 : (cap > 0x7fffffff ? 0x7fffffff : (int)cap);
}
static const int kMinFramesPerRange = 56;  // below this a range's kernels no longer fill the chip on their own
static int trunk_ranges(const mcg_engine* e, int frames) {
  int k = e->trunk_streams;
  if (k > mcg_engine::kMaxSplit) k = mcg_engine::kMaxSplit;
  while (k > 1 && frames / k < kMinFramesPerRange) --k;
  return k < 1 ? 1 : k;
}

static inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }
static inline size_t esize(mcg_dtype dt) { return mcg_is16(dt) ? 2 : 4; }

extern "C" void mcg_engine_destroy(mcg_engine* e);
extern "C" int mcg_engine_create(mcg_engine** out, const mcg_model_weights* w, mcg_dtype dt) {
  MCG_CHECK_ARG(out && w, "mcg_engine_create: null pointer");
  MCG_CHECK_ARG(dt == MCG_F32 || dt == MCG_BF16 || dt == MCG_F16X3 || dt == MCG_F16, "mcg_engine_create: unknown dtype %d", (int)dt);
  int expect = 0;
  for (int l = 0; l < 4; ++l) {
    MCG_CHECK_ARG(w->blocks[l] > 0, "mcg_engine_create: blocks[%d]=%d", l, w->blocks[l]);
    expect += 3 * w->blocks[l] + 1;
  }
  MCG_CHECK_ARG(w->num_convs == expect && w->convs, "mcg_engine_create: expected %d bottleneck convs, got %d", expect, w->num_convs);
  MCG_CHECK_ARG(w->num_stages > 0 && w->stage_weights && w->gaze_weights && w->init_boxes && w->init_feats, "mcg_engine_create: decoder tables missing");
  for (int i = 0; i < w->num_convs; ++i)
    MCG_CHECK_ARG(w->convs[i].w && w->convs[i].bias, "mcg_engine_create: conv %d has a null pointer", i);
  mcg_engine* e = new mcg_engine();
  e->dt = dt;
  memcpy(e->blocks, w->blocks, sizeof(e->blocks));
  e->stem = w->stem;
  e->convs.assign(w->convs, w->convs + w->num_convs);
  memcpy(e->lateral, w->lateral, sizeof(e->lateral));
  memcpy(e->fpn_out, w->fpn_out, sizeof(e->fpn_out));
  memcpy(e->c3_ds, w->c3_ds, sizeof(e->c3_ds));
  if (w->fused && w->num_fused > 0 && dt == MCG_F16X3) e->fused.assign(w->fused, w->fused + w->num_fused);
  e->init_boxes = w->init_boxes;
  e->init_feats = w->init_feats;
  e->num_stages = w->num_stages;
  e->stage_w.assign(w->stage_weights, w->stage_weights + (size_t)w->num_stages * MCG_SW_COUNT);
  memcpy(e->gaze_w, w->gaze_weights, sizeof(e->gaze_w));
  memcpy(e->stds, w->bbox_stds, sizeof(e->stds));
  bool ok = hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) == hipSuccess;
  e->pool = stream_pool_for_current_device();
  ok = ok && e->pool && e->pool->ok;
  if (e->pool) e->cand = e->pool->cand;
  for (int i = 0; i < mcg_engine::kMaxSplit - 1; ++i) ok = ok && hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    mcg_engine_destroy(e);
    mcg_set_error("mcg_engine_create: could not create the side streams / events");
    return MCG_ERR_HIP;
  }
  *out = e;
  return MCG_OK;
}

// Options.  Everything that used to be an environment switch of the lab bench is an explicit, per-engine setting.
extern "C" int mcg_engine_set_option(mcg_engine* e, const char* name, int value) {
  MCG_CHECK_ARG(e && name, "mcg_engine_set_option: null pointer");
  std::lock_guard<std::mutex> lock(e->mu);
  if (!strcmp(name, "trunk_streams")) { MCG_CHECK_ARG(value >= 1 && value <= mcg_engine::kMaxSplit, "trunk_streams must be 1..%d", mcg_engine::kMaxSplit); e->trunk_streams = value; }
  else if (!strcmp(name, "max_range_frames")) { MCG_CHECK_ARG(value >= 0, "max_range_frames must be >= 0"); e->max_range_frames = value; }
  else if (!strcmp(name, "tile")) e->ctx.tile = value > 0 ? value : -1;
  else if (!strcmp(name, "staged_gemm")) e->ctx.staged = value != 0;
  else if (!strcmp(name, "conv3x3_c64")) e->ctx.c64 = value != 0;
  else if (!strcmp(name, "stem_fused")) e->ctx.stem_fused = value != 0;
  else if (!strcmp(name, "decoder_chain")) e->ctx.chain = value != 0;
  else if (!strcmp(name, "decoder_attn_block")) e->ctx.attn_block = value != 0;
  else if (!strcmp(name, "pointwise_pair")) e->pw_pair = value != 0;
  else if (!strcmp(name, "pointwise_stream")) e->pw_single = value != 0;
  else if (!strcmp(name, "bottleneck_fused")) e->bneck_fused = value != 0;
  else if (!strcmp(name, "bottleneck_blocked")) e->bneck_blocked = value != 0;
  else if (!strcmp(name, "winograd")) { MCG_CHECK_ARG(value >= 0 && value <= 2, "winograd must be 0, 1 or 2"); e->winograd = value; }
  else if (!strcmp(name, "fpn_deferred")) e->fpn_deferred = value != 0;
  else if (!strcmp(name, "fpn_lateral_deferred")) e->fpn_lateral_deferred = value != 0;
  else if (!strcmp(name, "fpn_levels_deferred")) {
    MCG_CHECK_ARG(value >= 0 && value <= 15 && !(value & 1 && value > 1), "fpn_levels_deferred: 0, 1 or a mask of 2 (P3) | 4 (P4) | 8 (P5) (got %d)", value);
    e->fpn_levels_deferred = value;
  }
  else if (!strcmp(name, "wino_tile")) { MCG_CHECK_ARG(value >= -1 && value <= 3, "wino_tile must be -1 (by grid size) .. 3"); e->wino_tile = value; }
  else if (!strcmp(name, "range_audit")) {
    MCG_CHECK_ARG(!mcg_is16(e->dt) || !value, "range_audit: f32-storage engines only (MCG_F32, MCG_F16X3)");
    if (value && !e->audit_dev) {   // set-up, not the hot path: the only allocation the library ever makes
      if (hipMalloc((void**)&e->audit_dev, sizeof(unsigned long long) * 2 * mcg_engine::kAuditCap) != hipSuccess) { e->audit_dev = nullptr; mcg_set_error("range_audit: hipMalloc failed"); return MCG_ERR_HIP; }
    }
    if (value && hipMemset(e->audit_dev, 0, sizeof(unsigned long long) * 2 * mcg_engine::kAuditCap) != hipSuccess) { mcg_set_error("range_audit: hipMemset failed"); return MCG_ERR_HIP; }
    if (!value && e->audit_dev) { (void)hipFree(e->audit_dev); e->audit_dev = nullptr; }
    e->audit_names.clear();
  }
  else { mcg_set_error("mcg_engine_set_option: unknown option '%s'", name); return MCG_ERR_ARG; }
  return MCG_OK;
}

// Per-launch profiling, owned by the engine: while armed, every contraction launch the engine makes is bracketed by an event pair.
extern "C" int mcg_engine_profile_start(mcg_engine* e, int capacity) {
  MCG_CHECK_ARG(e, "mcg_engine_profile_start: null engine");
  std::lock_guard<std::mutex> lock(e->mu);
  if (e->prof.recs) { mcg_set_error("mcg_engine_profile_start: already armed"); return MCG_ERR_ARG; }
  MCG_CHECK_ARG(capacity > 0 && capacity <= (1 << 20), "mcg_engine_profile_start: bad capacity %d", capacity);
  e->prof.recs = new ProfRec[capacity];
  for (int i = 0; i < capacity; ++i) { e->prof.recs[i].a = nullptr; e->prof.recs[i].b = nullptr; }
  for (int i = 0; i < capacity; ++i) {
    if (hipEventCreate(&e->prof.recs[i].a) != hipSuccess || hipEventCreate(&e->prof.recs[i].b) != hipSuccess) {
      for (int j = 0; j <= i; ++j) {   // undo: the engine must stay re-armable
        if (e->prof.recs[j].a) (void)hipEventDestroy(e->prof.recs[j].a);
        if (e->prof.recs[j].b) (void)hipEventDestroy(e->prof.recs[j].b);
      }
      delete[] e->prof.recs;
      e->prof = Prof();
      mcg_set_error("mcg_engine_profile_start: hipEventCreate failed");
      return MCG_ERR_HIP;
    }
  }
  e->prof.cap = capacity; e->prof.n = 0;
  e->ctx.prof = &e->prof;
  return MCG_OK;
}
extern "C" int mcg_engine_profile_stop(mcg_engine* e, int* count, float* ms, double* flops, double* bytes, int* cfg, int* shape, int capacity) {
  MCG_CHECK_ARG(e, "mcg_engine_profile_stop: null engine");
  std::lock_guard<std::mutex> lock(e->mu);
  if (!e->prof.recs) { mcg_set_error("mcg_engine_profile_stop: not armed"); return MCG_ERR_ARG; }
  const int n = e->prof.n;
  int rc = MCG_OK;
  for (int i = 0; i < n; ++i) {
    const ProfRec& r = e->prof.recs[i];
    float t = 0.f;
    if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) rc = MCG_ERR_HIP;
    if (i < capacity) {
      if (ms) ms[i] = t;
      if (flops) flops[i] = r.flops;
      if (bytes) bytes[i] = r.bytes;
      if (cfg) cfg[i] = r.cfg;
      if (shape) { shape[3 * i] = r.shape[0]; shape[3 * i + 1] = r.shape[1]; shape[3 * i + 2] = r.shape[2]; }
    }
  }
  for (int i = 0; i < e->prof.cap; ++i) { (void)hipEventDestroy(e->prof.recs[i].a); (void)hipEventDestroy(e->prof.recs[i].b); }
  delete[] e->prof.recs;
  e->prof = Prof();
  e->ctx.prof = nullptr;
  if (count) *count = n < capacity ? n : capacity;
  if (rc != MCG_OK) mcg_set_error("mcg_engine_profile_stop: event query failed");
  return rc;
}
extern "C" void mcg_engine_destroy(mcg_engine* e) {
  if (!e) return;
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  for (int i = 0; i < mcg_engine::kMaxSplit - 1; ++i)
    if (e->ev_join[i]) (void)hipEventDestroy(e->ev_join[i]);
  if (e->prof.recs) {
    for (int i = 0; i < e->prof.cap; ++i) { (void)hipEventDestroy(e->prof.recs[i].a); (void)hipEventDestroy(e->prof.recs[i].b); }
    delete[] e->prof.recs;
  }
  if (e->audit_dev) (void)hipFree(e->audit_dev);
  delete e;
}

// ---------------------------------------------------------------- range audit (debug option)
__global__ void range_audit_kernel(const float* __restrict__ x, long long n, unsigned long long* __restrict__ cnt) {
  unsigned long long big = 0, bad = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v = x[i];
    if (!(fabsf(v) <= 3.4028235e38f)) ++bad;       // inf or nan
    else if (fabsf(v) > 65504.f) ++big;
  }
  big = (unsigned long long)wave_sum((float)big) ;  // counts per wave stay far below 2^24: exact in f32
  bad = (unsigned long long)wave_sum((float)bad);
  if ((threadIdx.x & 63) == 0) {
    if (big) atomicAdd(cnt, big);
    if (bad) atomicAdd(cnt + 1, bad);
  }
}
// One audited tensor: slot idx of the chunk's sequence (the same for every chunk and frame range, so the counters add up over the batch)
struct AuditCursor { mcg_engine* e; hipStream_t s; int idx; bool naming; };
__attribute__((format(printf, 4, 5))) static void audit_tensor(AuditCursor& a, const void* p, long long elements, const char* fmt, ...) {
  if (!a.e->audit_dev || a.idx >= mcg_engine::kAuditCap) return;
  if (a.naming) {
    char name[64];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
    a.e->audit_names.push_back(name);
  }
  const long long per_thread = 16;
  long long blocks = (elements + 256 * per_thread - 1) / (256 * per_thread);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(range_audit_kernel, dim3((int)blocks), dim3(256), 0, a.s, (const float*)p, elements, a.e->audit_dev + 2 * a.idx);
  ++a.idx;
}

// ---------------------------------------------------------------- trunk workspace for one chunk of n frames
struct TrunkWs {
  char *stem_ws, *x0, *xa, *xb, *o1, *o2, *ds, *c[4], *l[4];
  size_t stem_bytes, big, total;   // big: bytes of xa / xb / ds
};
static TrunkWs trunk_layout(mcg_dtype dt, int n, int H, int W, char* base) {
  const size_t es = esize(dt);
  const size_t h2 = H / 4, w2 = W / 4;
  TrunkWs t;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
  t.stem_bytes = mcg_stem_workspace_bytes(dt, n, H, W);
  t.stem_ws = take(t.stem_bytes);
  t.big = (size_t)n * h2 * w2 * 256 * es;  // the largest activation: C2 = [n, H/4, W/4, 256]
  t.x0 = take((size_t)n * h2 * w2 * 64 * es);
  t.xa = take(t.big); t.xb = take(t.big);
  t.o1 = take(t.big / 2); t.o2 = take(t.big / 2);
  t.ds = take(t.big);
  for (int i = 0; i < 4; ++i) {
    const size_t hi = (H / 4) >> i, wi = (W / 4) >> i;
    t.c[i] = take((size_t)n * hi * wi * (256u << i) * es);
    t.l[i] = take((size_t)n * hi * wi * 256 * es);
  }
  t.total = off;
  return t;
}

// Which Winograd form conv_call runs a conv in (0: none) -- by the layer's SHAPE only
static int wino_kind(const mcg_engine* e, mcg_dtype dt, const mcg_conv_weights& cw, int n, int h, int w, int rm) {
  return (dt == MCG_F16X3 && e->winograd && e->ctx.tile < 0 && cw.k == 3 && cw.stride == 1 && cw.pad == 1 && rm == MCG_RES_NONE)
             ? ((cw.wf4 && e->winograd >= 2 && wino_x3_applicable(n, h, w, cw.cin, cw.cout, 4)) ? 4 : ((cw.wf && wino_x3_applicable(n, h, w, cw.cin, cw.cout, 2)) ? 2 : 0))
             : 0;
}
// f16x3: a 3x3 / stride 1 conv as a 1-D Winograd F(g,3) contraction (wino_x3.hpp) on x [n, h, w, cin] -> y
static WinoParams wino_params(const mcg_conv_weights& cw, int g, const void* x, int n, int h, int w, void* y, int relu) {
  WinoParams wp;
  memset(&wp, 0, sizeof(wp));
  wp.x = (const float*)x; wp.u = g == 4 ? cw.wf4 : cw.wf; wp.bias = cw.bias; wp.y = (float*)y;
  wp.H = h; wp.W = w; wp.frames = n; wp.Cin = cw.cin; wp.Cout = cw.cout; wp.relu = relu; wp.wscale = cw.wscale;
  return wp;
}
// A Winograd launch of conv cw over M output pixels is booked as the DIRECT convolution's FLOPs and bytes: the roofline
// keeps counting the reference's arithmetic.  book = false: 0 / 0 (a launch whose work an earlier record already counts)
static ProfRec* prof_begin_wino(const McgCtx& ctx, hipStream_t s, const mcg_conv_weights& cw, long long M, bool book = true) {
  return prof_begin(ctx, s, 73, (int)M, cw.cout, 9 * cw.cin, book ? 2.0 * M * 9.0 * cw.cin * cw.cout : 0.0,
                    book ? 4.0 * ((double)M * (cw.cin + cw.cout) + 9.0 * cw.cin * cw.cout) : 0.0);
}
// Closes the profile record of a launch that returned rc: a failed launch is MCG_ERR_HIP ("<what> launch failed")
static int launch_done(ProfRec* rec, hipStream_t s, int rc, const char* what) {
  prof_end(rec, s);
  if (rc) { mcg_set_error("%s launch failed", what); return MCG_ERR_HIP; }
  return MCG_OK;
}
// The contraction kernel's descriptor of conv cw on x [n, h, w, cin] -> y, with an optional residual (res_mode; [n, hr, wr] for UPSAMPLE_ADD)
static mcg_conv_desc conv_desc(mcg_dtype dt, const mcg_conv_weights& cw, const void* x, int n, int h, int w, void* y, int relu,
                               const void* res, int res_mode, int hr, int wr) {
  mcg_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.x = x; d.w = cw.w; d.bias = cw.bias; d.residual = res; d.y = y;
  d.N = n; d.H = h; d.W = w; d.Cin = cw.cin; d.Cout = cw.cout; d.KH = cw.k; d.KW = cw.k; d.stride = cw.stride; d.pad = cw.pad;
  d.relu = relu; d.residual_mode = res_mode; d.Hr = hr; d.Wr = wr;
  d.wscale = dt == MCG_F16X3 ? cw.wscale : 0.f;
  return d;
}
static int conv_call(const mcg_engine* e, hipStream_t s, mcg_dtype dt, const mcg_conv_weights& cw, const void* x, int n, int h, int w, void* y,
                     int relu, const void* res, int res_mode, int hr, int wr) {
  const long long M = (long long)n * h * w;
  const int rm = res ? res_mode : MCG_RES_NONE;
  const long long res_m = rm == MCG_RES_UPSAMPLE_ADD ? (long long)n * hr * wr : M;   // residual rows
  const bool x3 = dt == MCG_F16X3;
  // the HBM-bound 1x1 convs by the persistent register-resident-weight kernel: 16-bit pw_single.hpp, f16x3 pw_single_x3.hpp (256 -> 256 / 1024)
  if ((x3 || mcg_is16(dt)) && e->pw_single && e->ctx.tile < 0 && cw.wf && cw.bias && cw.k == 1 && cw.stride == 1 && cw.pad == 0 && M < 0x7fffffffll &&
      (x3 ? pw_single_x3_applicable(cw.cin, cw.cout, rm, M, res_m) : !e->ctx.staged && pw_single_applicable(cw.cin, cw.cout, rm, M, res_m))) {
    PwSingleParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.a = x; pp.res = res; pp.wf = cw.wf; pp.bias = cw.bias; pp.y = y;
    pp.M = (int)M; pp.relu = relu; pp.Ho = h; pp.Wo = w; pp.wscale = x3 ? cw.wscale : 0.f;
    if (rm == MCG_RES_UPSAMPLE_ADD) { pp.Hr = hr; pp.Wr = wr; pp.rscale_h = (float)hr / (float)h; pp.rscale_w = (float)wr / (float)w; }
    ProfRec* rec = prof_begin(e->ctx, s, x3 ? 71 : 61, pp.M, cw.cout, cw.cin, 2.0 * M * cw.cin * cw.cout,
                              (double)esize(dt) * ((double)M * (cw.cin + cw.cout) + (rm == MCG_RES_NONE ? 0.0 : (double)res_m) * cw.cout + (double)cw.cin * cw.cout));
    const int rmode = rm == MCG_RES_NONE ? 0 : (rm == MCG_RES_ADD ? 1 : 2);
    return launch_done(rec, s, x3 ? launch_pw_single_x3(s, pp, cw.cout, rmode) : launch_pw_single(s, pp, cw.cin, cw.cout, rmode, dt),
                       x3 ? "pw_single_x3" : "pw_single");
  }
  // F(4,3) where the layer's shape allows it and the weights carry that copy, else F(2,3) (FPN outputs, layer3's conv2), else the direct kernel
  const int wg = wino_kind(e, dt, cw, n, h, w, rm);
  if (wg) {
    ProfRec* rec = prof_begin_wino(e->ctx, s, cw, M);
    return launch_done(rec, s, launch_wino_x3(s, wino_params(cw, wg, x, n, h, w, y, relu), e->wino_tile, wg), "wino_x3");
  }
  const mcg_conv_desc d = conv_desc(dt, cw, x, n, h, w, y, relu, res, res_mode, hr, wr);
  return conv2d_ctx(s, dt, &d, e->ctx);
}

// The trunk's walk over its bottleneck blocks: the current block's input and the buffers of its conv1 / conv2 outputs
struct TrunkCursor {
  const void* x;     // block input [n, h, w, *]
  int h, w, ci;      // convs[ci] = the block's conv1
  char *o1, *o2;     // conv1 / conv2 outputs; the fused tail writes the NEXT conv1 output into o2 and the two swap
  bool o1_ready;     // o1 already holds this block's conv1 output (written by the previous block's pointwise-pair / fused-tail kernel)
  bool x_blocked;    // x is in the fused tail's blocked layout (written by the previous block's fused tail for the next one's only)
};
// f16x3: the fused tail (bneck_x3.hpp: conv2 -> conv3 (+ downsample / + residual) -> the next block's conv1 as ONE kernel) of the block whose
// conv1 is convs[ci] (block index b), if one was handed over and every shape matches
static const mcg_fused_block* fused_tail_at(const mcg_engine* e, int ci, int b) {
  if (!(e->dt == MCG_F16X3 && e->bneck_fused && e->ctx.tile < 0) || ci + 2 >= (int)e->convs.size()) return nullptr;
  const mcg_fused_block* f = nullptr;
  for (const mcg_fused_block& q : e->fused)
    if (q.conv2_index == ci + 1) f = &q;
  if (!f) return nullptr;
  const bool ds = b == 0;
  const mcg_conv_weights &d2 = e->convs[ci + 1], &d3 = e->convs[ci + 2];
  const int kk = ds ? e->convs[ci + 3].cin : 0, ss = ds ? e->convs[ci + 3].stride : 1;
  const int cn_i = ci + (ds ? 4 : 3);
  const bool nx = f->cn == 0 || (cn_i < (int)e->convs.size() && e->convs[cn_i].k == 1 && e->convs[cn_i].stride == 1 && e->convs[cn_i].cout == f->cn && e->convs[cn_i].cin == f->c);
  return (d2.k == 3 && d2.stride == 1 && d2.pad == 1 && d2.cin == f->cm && d2.cout == f->cm && d3.cout == f->c && f->nsrc == (ds ? 2 : 1) && nx &&
          bneck_x3_applicable(f->cm, f->c, f->cn, f->nsrc, kk, ss)) ? f : nullptr;
}
// Block (l, b) from o1 by its fused tail fb into y (same size: conv2 has stride 1), and the next conv1 into o2
static int fused_tail_step(const mcg_engine* e, hipStream_t s, const TrunkWs& t, AuditCursor& au, TrunkCursor& c, const mcg_fused_block* fb,
                           int n, int l, int b, void* y) {
  const bool has_ds = b == 0;
  const int k2 = has_ds ? e->convs[c.ci + 3].cin : 0;
  BneckParams bp;
  memset(&bp, 0, sizeof(bp));
  bp.x = (const float*)c.o1; bp.res = (const float*)c.x; bp.wstream = (const char*)fb->wstream; bp.bias = fb->bias;
  bp.y = (float*)y; bp.z = (float*)c.o2; bp.H = c.h; bp.W = c.w;
  // y goes to the NEXT block's fused tail only (as its residual; its conv1 is this kernel's z, cn > 0): both sides use the kernel's blocked
  // layout -- whole-line stores and loads (bneck_x3.hpp) -- where the block grid fits the ping-pong buffer; not under range_audit,
  // which reads tensors as [M][C]
  const long long blk_bytes = (long long)n * ((c.h + bnx::TH - 1) / bnx::TH) * ((c.w + bnx::TW - 1) / bnx::TW) * bnx::NPIX * fb->c * (long long)esize(e->dt);
  const mcg_fused_block* fnext = (b + 1 < e->blocks[l]) ? fused_tail_at(e, c.ci + (has_ds ? 4 : 3), b + 1) : nullptr;
  bp.res_blocked = c.x_blocked ? 1 : 0;
  bp.y_blocked = (e->bneck_blocked && !e->audit_dev && y != (void*)t.c[l] && fb->cn > 0 && fnext && fnext->nsrc == 1 && fnext->c == fb->c &&
                  blk_bytes <= (long long)t.big) ? 1 : 0;
  const double M = (double)n * c.h * c.w;
  ProfRec* rec = prof_begin(e->ctx, s, 70, n * c.h * c.w, fb->c + fb->cn, 9 * fb->cm + fb->cm + k2 + fb->c,
                            2.0 * M * (9.0 * fb->cm * fb->cm + (double)(fb->cm + k2) * fb->c + (double)fb->c * fb->cn),
                            4.0 * (M * (fb->cm + (has_ds ? k2 : fb->c) + fb->c + fb->cn) + 9.0 * fb->cm * fb->cm + (double)(fb->cm + k2) * fb->c + (double)fb->c * fb->cn));
  MCG_TRY(launch_done(rec, s, launch_bneck_x3(s, bp, n, fb->cm, fb->nsrc, fb->cn), "bneck_x3"));
  audit_tensor(au, y, (long long)n * c.h * c.w * fb->c, "layer%d.%d.out (fused tail)", l + 1, b);
  if (fb->cn > 0) {
    audit_tensor(au, c.o2, (long long)n * c.h * c.w * fb->cn, "layer%d.%d.next_conv1 (fused tail)", l + 1, b);
    std::swap(c.o1, c.o2);
    c.o1_ready = true;
  }
  c.x_blocked = bp.y_blocked != 0;
  return MCG_OK;
}
// pw_pair.hpp: conv3 (+ downsample / + residual) of block (l, b) and the NEXT block's conv1 -- the following block's, or the next layer's
// first (1x1, stride 1 on this block's output) -- as one kernel: layer1 of the 16-bit engines, where both are HBM-bound.  -> that conv1's
// weights, or NULL where the pair does not apply (M = output pixels)
static const mcg_conv_weights* pw_pair_next(const mcg_engine* e, int ci, int l, int b, long long M) {
  const bool has_ds = b == 0;
  const mcg_conv_weights& c3 = e->convs[ci + 2];
  const mcg_conv_weights* c3w = has_ds ? (e->c3_ds[l].w ? &e->c3_ds[l] : nullptr) : &c3;
  const int ci_next = ci + (has_ds ? 4 : 3);
  const mcg_conv_weights* c1n = ci_next < (int)e->convs.size() ? &e->convs[ci_next] : nullptr;
  const int k2 = has_ds ? e->convs[ci + 3].cin : 0;
  return (mcg_is16(e->dt) && e->pw_pair && l == 0 && c3w && c1n && c3w->wf && c1n->wf && c3w->bias && c1n->bias && c1n->k == 1 && c1n->stride == 1 &&
          c1n->cin == c3.cout && pw_pair_applicable(c3.cin, k2, has_ds ? e->convs[ci + 3].stride : 1, c3.cout, c1n->cout, M) && M < 0x7fffffffll)
             ? c1n : nullptr;
}
static int pw_pair_step(const mcg_engine* e, hipStream_t s, TrunkCursor& c, const mcg_conv_weights& c1n, int n, int l, int b, void* y, int ho, int wo) {
  const bool has_ds = b == 0;
  const mcg_conv_weights& c3 = e->convs[c.ci + 2];
  const mcg_conv_weights& c3w = has_ds ? e->c3_ds[l] : c3;
  PwPairParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.a1 = c.o2; pp.K1 = c3.cin;
  if (has_ds) { pp.a2 = c.x; pp.K2 = e->convs[c.ci + 3].cin; pp.stride2 = e->convs[c.ci + 3].stride; pp.H2 = c.h; pp.W2 = c.w; }
  else pp.res = c.x;
  pp.w3f = c3w.wf; pp.b3 = c3w.bias; pp.y = y;
  pp.w1f = c1n.wf; pp.b1 = c1n.bias; pp.z = c.o1;
  pp.M = n * ho * wo; pp.C = c3.cout; pp.C2 = c1n.cout; pp.Ho = ho; pp.Wo = wo;
  // cfg 60: both contractions of the pair count (2 M (K C + C C2))
  ProfRec* rec = prof_begin(e->ctx, s, 60, pp.M, pp.C + pp.C2, pp.K1 + pp.K2, 2.0 * pp.M * ((double)(pp.K1 + pp.K2) * pp.C + (double)pp.C * pp.C2),
                            2.0 * ((double)pp.M * (pp.K1 + pp.K2 + (has_ds ? 0 : pp.C) + pp.C + pp.C2) + (double)(pp.K1 + pp.K2) * pp.C + (double)pp.C * pp.C2));
  MCG_TRY(launch_done(rec, s, launch_pw_pair(s, pp, e->dt), "pw_pair"));
  c.o1_ready = true;
  return MCG_OK;
}
// conv3 (+ downsample / + residual) of block (l, b) from o2 into y [n, ho, wo]
static int conv3_step(const mcg_engine* e, hipStream_t s, const TrunkWs& t, AuditCursor& au, const TrunkCursor& c, int n, int l, int b, void* y,
                      int ho, int wo) {
  const mcg_conv_weights& c3 = e->convs[c.ci + 2];
  if (b == 0 && e->c3_ds[l].w) {
    // conv3 and the downsample conv as ONE K-concatenated GEMM: relu([o2 | x@stride] . [W3 | Wd]^T + b3 + bd);
    // the downsample output never goes to HBM and conv3 reads no residual.
    const mcg_conv_weights& ds = e->convs[c.ci + 3];
    mcg_conv_desc d = conv_desc(e->dt, e->c3_ds[l], c.o2, n, ho, wo, y, 1, nullptr, MCG_RES_NONE, 0, 0);
    d.Cin = c3.cin;   // o2's share of the weights' K = c3.cin + ds.cin
    d.x2 = c.x; d.Cin2 = ds.cin; d.stride2 = ds.stride; d.H2 = c.h; d.W2 = c.w;
    MCG_TRY(conv2d_ctx(s, e->dt, &d, e->ctx));
  } else {
    const void* identity = c.x;
    if (b == 0) {
      MCG_TRY(conv_call(e, s, e->dt, e->convs[c.ci + 3], c.x, n, c.h, c.w, t.ds, 0, nullptr, MCG_RES_NONE, 0, 0));
      identity = t.ds;
    }
    MCG_TRY(conv_call(e, s, e->dt, c3, c.o2, n, ho, wo, y, 1, identity, MCG_RES_ADD, 0, 0));
  }
  audit_tensor(au, y, (long long)n * ho * wo * c3.cout, "layer%d.%d.out", l + 1, b);
  return MCG_OK;
}

// Backbone + FPN over frames [f0, f0+n): writes pyramid level i at frame offset f0.
// tk.inner != NULL (deferred P2): the P2 top-down inner map goes to tk.inner (frame offset f0) and the P2 output conv is left to the decoder.
// tk.c2 != NULL (deferred P2 lateral): C2 and the P3 inner map are written straight to tk.c2 / tk.l1 (frame offset f0) -- in place of the
// workspace, no copy -- and the P2 lateral is left to the decoder as well; every reader follows t.c[0] / t.l[1]
// tk.lin[i] != NULL, i = 1 .. 3 (level i deferred by frames): the inner map of level i is written straight to tk.lin[i] in the same way and
// its output conv is left to the decoder
struct TrunkKeep { char *inner, *c2, *l1, *lin[4]; };
static const TrunkKeep kNoKeep = {nullptr, nullptr, nullptr, {nullptr, nullptr, nullptr, nullptr}};
static int trunk_chunk(mcg_engine* e, hipStream_t s, const float* img, int f0, int n, int H, int W, void* const pyr[4], char* wsbase,
                       bool backbone_only = false, const TrunkKeep tk = kNoKeep) {
  const mcg_dtype dt = e->dt;
  const size_t es = esize(dt);
  TrunkWs t = trunk_layout(dt, n, H, W, wsbase);
  char* const inner0 = tk.inner;
  if (inner0) t.l[0] = inner0 + (size_t)f0 * (H / 4) * (W / 4) * 256 * es;
  const bool lateral_deferred = inner0 && tk.c2 && tk.l1;
  if (lateral_deferred) {
    t.c[0] = tk.c2 + (size_t)f0 * (H / 4) * (W / 4) * 256 * es;
    t.l[1] = tk.l1 + (size_t)f0 * (H / 8) * (W / 8) * 256 * es;
  }
  for (int i = 1; i < 4; ++i)
    if (tk.lin[i]) t.l[i] = tk.lin[i] + (size_t)f0 * ((H / 4) >> i) * ((W / 4) >> i) * 256 * es;
  MCG_TRY(stem_forward_ctx(s, dt, img + (size_t)f0 * 3 * H * W, e->stem.w, e->stem.bias, t.x0, n, H, W, t.stem_ws, t.stem_bytes, e->ctx));
  AuditCursor au{e, s, 0, e->audit_dev != nullptr && e->audit_names.empty()};
  audit_tensor(au, t.x0, (long long)n * (H / 4) * (W / 4) * 64, "stem");
  TrunkCursor c{t.x0, H / 4, W / 4, 0, t.o1, t.o2, false, false};
  for (int l = 0; l < 4; ++l) {
    for (int b = 0; b < e->blocks[l]; ++b) {
      const mcg_conv_weights &c1 = e->convs[c.ci], &c2 = e->convs[c.ci + 1];
      const int ho = (c.h + 2 * c2.pad - c2.k) / c2.stride + 1, wo = (c.w + 2 * c2.pad - c2.k) / c2.stride + 1;
      void* y = (b == e->blocks[l] - 1) ? (void*)t.c[l] : (c.x == t.xa ? (void*)t.xb : (void*)t.xa);
      if (!c.o1_ready) {
        MCG_TRY(conv_call(e, s, dt, c1, c.x, n, c.h, c.w, c.o1, 1, nullptr, MCG_RES_NONE, 0, 0));
        audit_tensor(au, c.o1, (long long)n * c.h * c.w * c1.cout, "layer%d.%d.conv1", l + 1, b);
      }
      c.o1_ready = false;
      const mcg_fused_block* fb = fused_tail_at(e, c.ci, b);
      if (c.x_blocked && !(fb && fb->nsrc == 1)) { mcg_set_error("trunk: a blocked tensor reached a kernel that does not read that layout"); return MCG_ERR_UNSUPPORTED; }
      if (fb) {
        MCG_TRY(fused_tail_step(e, s, t, au, c, fb, n, l, b, y));
      } else {
        MCG_TRY(conv_call(e, s, dt, c2, c.o1, n, c.h, c.w, c.o2, 1, nullptr, MCG_RES_NONE, 0, 0));
        audit_tensor(au, c.o2, (long long)n * ho * wo * c2.cout, "layer%d.%d.conv2", l + 1, b);
        const mcg_conv_weights* c1n = pw_pair_next(e, c.ci, l, b, (long long)n * ho * wo);
        MCG_TRY(c1n ? pw_pair_step(e, s, c, *c1n, n, l, b, y, ho, wo) : conv3_step(e, s, t, au, c, n, l, b, y, ho, wo));
      }
      c.x = y; c.h = ho; c.w = wo;
      c.ci += b == 0 ? 4 : 3;
    }
  }
  if (backbone_only) return MCG_OK;  // mcg_bench_backbone_forward: C2..C5 only
  // FPN (fpn.py:157-180): laterals top-down with the nearest-upsample add fused into the epilogue
  int hs[4], wsz[4];
  for (int i = 0; i < 4; ++i) { hs[i] = (H / 4) >> i; wsz[i] = (W / 4) >> i; }
  for (int i = 3; i >= (lateral_deferred ? 1 : 0); --i) {
    const void* res = i == 3 ? nullptr : t.l[i + 1];
    MCG_TRY(conv_call(e, s, dt, e->lateral[i], t.c[i], n, hs[i], wsz[i], t.l[i], 0, res, res ? MCG_RES_UPSAMPLE_ADD : MCG_RES_NONE,
                      i == 3 ? 0 : hs[i + 1], i == 3 ? 0 : wsz[i + 1]));
    audit_tensor(au, t.l[i], (long long)n * hs[i] * wsz[i] * 256, "fpn.lateral%d (+ top-down)", i);
  }
  for (int i = inner0 ? 1 : 0; i < 4; ++i) {
    if (tk.lin[i]) continue;
    char* dst = (char*)pyr[i] + (size_t)f0 * hs[i] * wsz[i] * 256 * es;
    MCG_TRY(conv_call(e, s, dt, e->fpn_out[i], t.l[i], n, hs[i], wsz[i], dst, 0, nullptr, MCG_RES_NONE, 0, 0));
    audit_tensor(au, dst, (long long)n * hs[i] * wsz[i] * 256, "fpn.P%d", i + 2);
  }
  return MCG_OK;
}

// Debug read-out of the range audit (engine option range_audit = 1): synchronises the device, copies the counters to the host and
// resets them.  counts[2 i] = values with |x| > 65504, counts[2 i + 1] = non-finite values of audited tensor i over every frame processed
// since the last read; names[i] (optional) points at the engine-owned name of tensor i (valid until the option changes).
extern "C" int mcg_engine_range_audit(mcg_engine* e, unsigned long long* counts, const char** names, int capacity, int* n_out) {
  MCG_CHECK_ARG(e && counts && n_out && capacity > 0, "mcg_engine_range_audit: bad argument");
  std::lock_guard<std::mutex> lock(e->mu);
  if (!e->audit_dev) { mcg_set_error("mcg_engine_range_audit: the range_audit option is off"); return MCG_ERR_ARG; }
  const int n = (int)e->audit_names.size() < capacity ? (int)e->audit_names.size() : capacity;
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(counts, e->audit_dev, sizeof(unsigned long long) * 2 * n, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemset(e->audit_dev, 0, sizeof(unsigned long long) * 2 * mcg_engine::kAuditCap) != hipSuccess) {
    mcg_set_error("mcg_engine_range_audit: device read failed");
    return MCG_ERR_HIP;
  }
  if (names) for (int i = 0; i < n; ++i) names[i] = e->audit_names[i].c_str();
  *n_out = n;
  return MCG_OK;
}

// Decoder scratch for N frames (RoI features, query state, per-stage and gaze-head workspaces).
struct DecWs {
  char *roi, *obj_a, *obj_b, *stage_ws, *gaze_ws;
  float *boxes_a, *boxes_b, *cls;
  size_t stage_bytes, gaze_bytes, total;
};
static DecWs dec_layout(mcg_dtype dt, int N, char* base) {
  const size_t es = esize(dt), R = (size_t)N * 3;
  DecWs c;
  memset(&c, 0, sizeof(c));
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
  c.roi = take(R * 49 * 256 * es);
  c.obj_a = take(R * 256 * es); c.obj_b = take(R * 256 * es);
  c.boxes_a = (float*)take(R * 4 * 4); c.boxes_b = (float*)take(R * 4 * 4); c.cls = (float*)take(R * 4);
  c.stage_bytes = mcg_stage_workspace_bytes(dt, N); c.stage_ws = take(c.stage_bytes);
  c.gaze_bytes = mcg_gaze_head_workspace_bytes(dt, N); c.gaze_ws = take(c.gaze_bytes);
  c.total = off;
  return c;
}
static bool check_shape_ok(int N, int H, int W) { return N > 0 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0; }
static size_t pyramid_bytes(mcg_dtype dt, int N, int H, int W, int level) {
  return al256((size_t)N * ((H / 4) >> level) * ((W / 4) >> level) * 256 * esize(dt));
}

// Deferred pyramid slot (mcg_*_deferred): P2..P5 outputs, then -- when the engine defers P2 -- the P2 inner map the trunk leaves for the
// decoder, one int per 8 x 8 output block of P2 (0 = not yet listed) followed by one list count per decoder stage, and one block list
// per stage.  Without deferral the slot is the four pyramid levels and the pair runs the dense launches.
// When the P2 lateral is deferred as well (option fpn_lateral_deferred), the slot also carries what that lateral reads -- C2 and the P3
// inner map, written there by the trunk: the next batch's trunk overwrites its workspace while this batch's decoder runs -- and a second
// set of flags, counts and lists for the INNER blocks (the listed output blocks and their neighbours).  The inner flags and counts follow
// the output ones, so one clear covers both.
struct DeferSlot {
  void* p[4];
  char* inner;
  int *state, *count, *list;
  int nblk;
  bool deferred;
  bool lateral;                      // the P2 lateral is deferred too
  char *c2, *l1;                     // C2 [N, H/4, W/4, 256], P3 inner map [N, H/8, W/8, 256]
  int *istate, *icount, *ilist;      // inner blocks: flag per block, count per stage, list per stage
  // levels deferred by frames (option fpn_levels_deferred), i = 1 .. 3 where bit i of level_mask is set: the level's inner map, written there by
  // the trunk (lin[1] is l1 where the P2 lateral is deferred too), a flag per frame + a count per stage (behind the block flags and counts: the
  // slot's one clear covers all clear_n ints) and a frame list per stage
  int level_mask;
  char* lin[4];
  int *fstate[4], *fcount[4], *flist[4];
  int clear_n;
  size_t total;
};
static bool fpn_deferred_on(const mcg_engine* e, int N, int H, int W) {
  const mcg_conv_weights& cw = e->fpn_out[0];
  const int h = H / 4, w = W / 4;
  return e->fpn_deferred && e->dt == MCG_F16X3 && !e->audit_dev && e->num_stages > 0 && wino_kind(e, e->dt, cw, N, h, w, MCG_RES_NONE) == 2 &&
         wino_x3_blocks_applicable(N, h, w, cw.cin, cw.cout) && roi_mark_supported(h, w);
}
// The P2 lateral goes to the decoder too: only where P2 is deferred, for a lateral the list kernel serves (the streaming kernel's weights)
static bool fpn_lateral_deferred_on(const mcg_engine* e, int N, int H, int W) {
  const mcg_conv_weights& cw = e->lateral[0];
  const int h = H / 4, w = W / 4;
  return e->fpn_lateral_deferred && fpn_deferred_on(e, N, H, W) && e->pw_single && e->ctx.tile < 0 && cw.wf && cw.bias && cw.k == 1 && cw.stride == 1 &&
         cw.pad == 0 && h % 2 == 0 && w % 2 == 0 &&
         pw_single_x3_blocks_applicable(cw.cin, cw.cout, h, w, (long long)N * h * w, (long long)N * (h / 2) * (w / 2));
}
// P3 .. P5 by frames: only where P2 is deferred, for the levels the option names whose dense conv is the F(2,3) Winograd kernel and whose map the
// frame-list tile serves -> mask of levels (bit i = level i)
static int fpn_levels_deferred_mask(const mcg_engine* e, int N, int H, int W) {
  if (!e->fpn_levels_deferred || !fpn_deferred_on(e, N, H, W)) return 0;
  const int want = e->fpn_levels_deferred == 1 ? mcg_engine::kDeferLevelsDefault : e->fpn_levels_deferred;
  int mask = 0;
  for (int i = 1; i < 4; ++i) {
    const mcg_conv_weights& cw = e->fpn_out[i];
    const int h = (H / 4) >> i, w = (W / 4) >> i;
    if (((want >> i) & 1) && wino_kind(e, e->dt, cw, N, h, w, MCG_RES_NONE) == 2 && wino_x3_frames_applicable(N, h, w, cw.cin, cw.cout)) mask |= 1 << i;
  }
  return mask;
}
static DeferSlot defer_layout(const mcg_engine* e, int N, int H, int W, char* base) {
  DeferSlot d;
  memset(&d, 0, sizeof(d));
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
  for (int i = 0; i < 4; ++i) d.p[i] = take(pyramid_bytes(e->dt, N, H, W, i));
  d.deferred = fpn_deferred_on(e, N, H, W);
  if (d.deferred) {
    d.inner = take((size_t)N * (H / 4) * (W / 4) * 256 * esize(e->dt));
    d.nblk = N * wino_x3_blocks_per_frame(H / 4, W / 4);
    d.lateral = fpn_lateral_deferred_on(e, N, H, W);
    d.level_mask = fpn_levels_deferred_mask(e, N, H, W);
    const size_t per = (size_t)d.nblk + e->num_stages, fper = (size_t)N + e->num_stages;
    size_t ints = per * (d.lateral ? 2 : 1);
    const size_t fints0 = ints;
    for (int i = 1; i < 4; ++i) ints += ((d.level_mask >> i) & 1) ? fper : 0;
    d.clear_n = (int)ints;
    d.state = (int*)take(sizeof(int) * ints);
    d.count = d.state ? d.state + d.nblk : nullptr;
    for (int i = 1, k = 0; i < 4; ++i) {
      if (!((d.level_mask >> i) & 1)) continue;
      d.fstate[i] = d.state ? d.state + fints0 + fper * k : nullptr;
      d.fcount[i] = d.fstate[i] ? d.fstate[i] + N : nullptr;
      d.flist[i] = (int*)take(sizeof(int) * (size_t)N * e->num_stages);
      ++k;
    }
    d.list = (int*)take(sizeof(int) * (size_t)d.nblk * e->num_stages);
    if (d.lateral) {
      d.istate = d.state ? d.state + per : nullptr;
      d.icount = d.istate ? d.istate + d.nblk : nullptr;
      d.ilist = (int*)take(sizeof(int) * (size_t)d.nblk * e->num_stages);
      d.c2 = take((size_t)N * (H / 4) * (W / 4) * 256 * esize(e->dt));
      d.l1 = take((size_t)N * (H / 8) * (W / 8) * 256 * esize(e->dt));
    }
    for (int i = 1; i < 4; ++i)
      if ((d.level_mask >> i) & 1) d.lin[i] = (i == 1 && d.lateral) ? d.l1 : take((size_t)N * ((H / 4) >> i) * ((W / 4) >> i) * 256 * esize(e->dt));
  }
  d.total = off;
  return d;
}

extern "C" size_t mcg_trunk_workspace_bytes(const mcg_engine* e, int N, int H, int W, int chunk) {
  if (!e || N <= 0) return 0;
  if (chunk <= 0 || chunk > N) chunk = N;
  if (chunk < N) return trunk_layout(e->dt, chunk, H, W, nullptr).total;
  // whole batch: one layout per concurrent frame range, sized for the maximum split so the answer does not depend on the environment
  size_t total = 0;
  const int cap = range_frame_cap(e, H, W);
  for (int k = 1; k <= mcg_engine::kMaxSplit; ++k) {
    const int per = (N + k - 1) / k < cap ? (N + k - 1) / k : cap;
    const size_t t = (size_t)k * al256(trunk_layout(e->dt, per, H, W, nullptr).total);
    if (t > total) total = t;
  }
  return total;
}
extern "C" size_t mcg_decoder_workspace_bytes(const mcg_engine* e, int N) {
  if (!e || N <= 0) return 0;
  return dec_layout(e->dt, N, nullptr).total;
}
extern "C" size_t mcg_engine_workspace_bytes(const mcg_engine* e, int N, int H, int W, int chunk) {
  if (!e || N <= 0) return 0;
  return mcg_trunk_workspace_bytes(e, N, H, W, chunk) + mcg_decoder_workspace_bytes(e, N) + defer_layout(e, N, H, W, nullptr).total;
}
extern "C" size_t mcg_deferred_pyramid_bytes(const mcg_engine* e, int N, int H, int W) {
  if (!e || N <= 0 || check_shape_ok(N, H, W) == false) return 0;
  return defer_layout(e, N, H, W, nullptr).total;
}

static int check_shape(int N, int H, int W) {
  MCG_CHECK_ARG(N > 0, "num_frames must be positive (got %d)", N);
  MCG_CHECK_ARG(H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0, "frame size %dx%d must be a multiple of 32 (Pad(size_divisor=32))", H, W);
  return MCG_OK;
}

static int trunk_forward(mcg_engine* e, mcg_stream s_, const float* img, int N, int H, int W, int chunk,
                         void* const pyramid[4], void* ws, size_t ws_bytes, bool backbone_only, const TrunkKeep tk = kNoKeep) {
  MCG_CHECK_ARG(e && img && (pyramid || backbone_only) && ws, "mcg_backbone_fpn_forward: null pointer");
  MCG_TRY(check_shape(N, H, W));
  std::lock_guard<std::mutex> lock(e->mu);
  if (chunk <= 0 || chunk > N) chunk = N;
  const size_t need = mcg_trunk_workspace_bytes(e, N, H, W, chunk);
  if (ws_bytes < need) { mcg_set_error("mcg_backbone_fpn_forward: workspace too small (%zu < %zu)", ws_bytes, need); return MCG_ERR_WORKSPACE; }
  // chunk < N: sequential frame chunks in a small workspace; else k concurrent frame ranges of at most the capped share
  const int k = chunk < N ? 1 : trunk_ranges(e, N), cap = range_frame_cap(e, H, W);
  const int per = chunk < N ? chunk : ((N + k - 1) / k < cap ? (N + k - 1) / k : cap);
  // fork: the side streams start after everything already queued on the caller's stream (the input, the previous consumer of
  // the pyramid buffers); join: the caller's stream continues after every range.  Range i owns stream i and workspace slot i;
  // a batch larger than k capped ranges takes several rounds on the same streams and slots (in order per stream).
  const hipStream_t s = (hipStream_t)s_;
  hipStream_t si[mcg_engine::kMaxSplit] = {s};
  if (k > 1) {
    const std::vector<int>& sides = side_streams_for(e, s);
    for (int i = 1; i < k; ++i) si[i] = e->cand[sides[i - 1]];
    if (hipEventRecord(e->ev_fork, s) != hipSuccess) { mcg_set_error("mcg_backbone_fpn_forward: hipEventRecord failed"); return MCG_ERR_HIP; }
    for (int i = 1; i < k; ++i)
      if (hipStreamWaitEvent(si[i], e->ev_fork, 0) != hipSuccess) { mcg_set_error("mcg_backbone_fpn_forward: hipStreamWaitEvent failed"); return MCG_ERR_HIP; }
  }
  const size_t part_ws = k > 1 ? al256(trunk_layout(e->dt, per, H, W, nullptr).total) : 0;
  int rc = MCG_OK;
  for (int f0 = 0, i = 0; f0 < N && rc == MCG_OK; f0 += per, i = (i + 1) % k)
    rc = trunk_chunk(e, si[i], img, f0, (N - f0) < per ? (N - f0) : per, H, W, pyramid, (char*)ws + (size_t)i * part_ws, backbone_only, tk);
  for (int i = 1; i < k; ++i) {  // joined even after a failed launch, so the caller's stream never runs ahead of a side stream
    if (hipEventRecord(e->ev_join[i - 1], si[i]) != hipSuccess || hipStreamWaitEvent(s, e->ev_join[i - 1], 0) != hipSuccess) {
      mcg_set_error("mcg_backbone_fpn_forward: join failed");
      rc = rc == MCG_OK ? MCG_ERR_HIP : rc;
    }
  }
  return rc;
}

extern "C" int mcg_bottleneck_x3(mcg_stream s, const float* x, const float* src2, const void* wstream, const float* bias, float* y, float* z,
                                 int frames, int H, int W, int cm, int nsrc, int cn, void* trace) {
  MCG_CHECK_ARG(x && src2 && wstream && bias && y && (z || cn == 0), "mcg_bottleneck_x3: null pointer");
  MCG_CHECK_ARG(frames > 0 && H > 0 && W > 0, "mcg_bottleneck_x3: empty problem");
  MCG_CHECK_ARG(bneck_x3_applicable(cm, 4 * cm, cn, nsrc, 64, 1), "mcg_bottleneck_x3: unsupported shape (cm=%d nsrc=%d cn=%d)", cm, nsrc, cn);
  BneckParams bp;
  memset(&bp, 0, sizeof(bp));
  bp.x = x; bp.res = src2; bp.wstream = (const char*)wstream; bp.bias = bias; bp.y = y; bp.z = z; bp.H = H; bp.W = W; bp.trace = (unsigned long long*)trace;
  if (launch_bneck_x3((hipStream_t)s, bp, frames, cm, nsrc, cn)) { mcg_set_error("mcg_bottleneck_x3: launch failed"); return MCG_ERR_HIP; }
  return MCG_OK;
}

extern "C" size_t mcg_conv3x3_wino_x3_weight_bytes(int Cin, int Cout, int g) {
  return (Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % wnx::UNT == 0 && (g == 2 || g == 4)) ? wino_x3_weight_bytes(Cin, Cout, g) : 0;
}
extern "C" int mcg_conv3x3_wino_x3(mcg_stream s, const float* x, const void* u, const float* bias, float* y, int frames, int H, int W,
                                   int Cin, int Cout, int relu, int tile, float wscale, int g) {
  MCG_CHECK_ARG(x && u && y, "mcg_conv3x3_wino_x3: null pointer");
  MCG_CHECK_ARG(tile >= 0 && tile <= 4, "mcg_conv3x3_wino_x3: tile must be 0 (by grid size) .. 4");
  if (!wino_x3_applicable(frames, H, W, Cin, Cout, g)) {
    mcg_set_error("mcg_conv3x3_wino_x3: unsupported shape (frames=%d %dx%d, %d -> %d channels, F(%d,3)): Cin %% 32, Cout %% 128, W <= 62 (F(4,3): W %% 4 == 0, W >= 16), a tile's window within its buffer", frames, H, W, Cin, Cout, g);
    return MCG_ERR_UNSUPPORTED;
  }
  WinoParams wp;
  memset(&wp, 0, sizeof(wp));
  wp.x = x; wp.u = u; wp.bias = bias; wp.y = y; wp.H = H; wp.W = W; wp.frames = frames; wp.Cin = Cin; wp.Cout = Cout; wp.relu = relu;
  wp.wscale = wscale;
  if (launch_wino_x3((hipStream_t)s, wp, tile - 1, g)) { mcg_set_error("mcg_conv3x3_wino_x3: launch failed"); return MCG_ERR_HIP; }
  return MCG_OK;
}
// The block tile as a stand-alone operator (tests and measurements): launch_wino_x3_blocks over the caller's list, never another kernel
extern "C" int mcg_conv3x3_wino_x3_blocks(mcg_stream s, const float* x, const void* u, const float* bias, float* y, int frames, int H, int W,
                                          int Cin, int Cout, int relu, float wscale, const int* block_list, const int* block_count,
                                          int max_blocks, int grid_cap) {
  MCG_CHECK_ARG(x && u && y && block_list && block_count, "mcg_conv3x3_wino_x3_blocks: null pointer");
  MCG_CHECK_ARG(max_blocks > 0 && grid_cap >= 0, "mcg_conv3x3_wino_x3_blocks: max_blocks must be positive and grid_cap >= 0 (max_blocks=%d grid_cap=%d)",
                max_blocks, grid_cap);
  if (H <= 0 || W <= 0 || H % 8 != 0 || W % 8 != 0 || !wino_x3_blocks_applicable(frames, H, W, Cin, Cout)) {
    mcg_set_error("mcg_conv3x3_wino_x3_blocks: unsupported shape (frames=%d %dx%d, %d -> %d channels): H %% 8, W %% 8, Cin %% 32, Cout %% 128, operands within 2 GiB",
                  frames, H, W, Cin, Cout);
    return MCG_ERR_UNSUPPORTED;
  }
  WinoParams wp;
  memset(&wp, 0, sizeof(wp));
  wp.x = x; wp.u = u; wp.bias = bias; wp.y = y; wp.H = H; wp.W = W; wp.frames = frames; wp.Cin = Cin; wp.Cout = Cout; wp.relu = relu;
  wp.wscale = wscale;
  if (launch_wino_x3_blocks((hipStream_t)s, wp, block_list, block_count, max_blocks, grid_cap)) {
    mcg_set_error("mcg_conv3x3_wino_x3_blocks: launch failed");
    return MCG_ERR_HIP;
  }
  return MCG_OK;
}

// The frame-list tile as a stand-alone operator (tests and measurements): launch_wino_x3_frames over the caller's list, never another kernel
extern "C" int mcg_conv3x3_wino_x3_frames(mcg_stream s, const float* x, const void* u, const float* bias, float* y, int frames, int H, int W,
                                          int Cin, int Cout, const int* frame_list, const int* frame_count, int grid_cap) {
  MCG_CHECK_ARG(x && u && y && frame_list && frame_count, "mcg_conv3x3_wino_x3_frames: null pointer");
  MCG_CHECK_ARG(grid_cap >= 0, "mcg_conv3x3_wino_x3_frames: grid_cap >= 0 (got %d)", grid_cap);
  if (H <= 0 || W <= 0 || !wino_x3_frames_applicable(frames, H, W, Cin, Cout)) {
    mcg_set_error("mcg_conv3x3_wino_x3_frames: unsupported shape (frames=%d %dx%d, %d -> %d channels): Cin %% 32, Cout %% 128, 2 <= W <= 30, a frame's rows of a tile within the window buffer, operands within 2 GiB",
                  frames, H, W, Cin, Cout);
    return MCG_ERR_UNSUPPORTED;
  }
  WinoParams wp;
  memset(&wp, 0, sizeof(wp));
  wp.x = x; wp.u = u; wp.bias = bias; wp.y = y; wp.H = H; wp.W = W; wp.frames = frames; wp.Cin = Cin; wp.Cout = Cout;
  if (launch_wino_x3_frames((hipStream_t)s, wp, frame_list, frame_count, grid_cap)) {
    mcg_set_error("mcg_conv3x3_wino_x3_frames: launch failed");
    return MCG_ERR_HIP;
  }
  return MCG_OK;
}

// The streaming 1x1 kernels as stand-alone operators: the launchers' own dispatch tables at any M >= 1, never another kernel
extern "C" int mcg_pointwise_stream(mcg_stream s, mcg_dtype dt, const void* a, const void* wf, const float* bias, const void* res, void* y,
                                    int M, int K, int N, int relu, int res_mode, int Ho, int Wo, int Hr, int Wr, float wscale,
                                    const int* block_list, const int* block_count, int grid_cap) {
  MCG_CHECK_ARG(a && wf && bias && y, "mcg_pointwise_stream: null pointer");
  MCG_CHECK_ARG(M > 0 && grid_cap >= 0, "mcg_pointwise_stream: M must be positive and grid_cap >= 0 (M=%d grid_cap=%d)", M, grid_cap);
  MCG_CHECK_ARG(res_mode >= MCG_RES_NONE && res_mode <= MCG_RES_UPSAMPLE_ADD && (res != nullptr) == (res_mode != MCG_RES_NONE),
                "mcg_pointwise_stream: res_mode %d needs %s residual", res_mode, res_mode == MCG_RES_NONE ? "no" : "a");
  MCG_CHECK_ARG((block_list != nullptr) == (block_count != nullptr), "mcg_pointwise_stream: block_list and block_count come together");
  const bool x3 = dt == MCG_F16X3, up = res_mode == MCG_RES_UPSAMPLE_ADD;
  if (up) MCG_CHECK_ARG(Ho > 0 && Wo > 0 && Hr > 0 && Wr > 0 && M % ((long long)Ho * Wo) == 0,
                        "mcg_pointwise_stream: upsample residual: M = frames * Ho * Wo (M=%d, %dx%d from %dx%d)", M, Ho, Wo, Hr, Wr);
  const long long res_rows = up ? M / ((long long)Ho * Wo) * Hr * Wr : M;
  bool ok = x3 ? pw_single_x3_dispatched(K, N, M, res_rows) : mcg_is16(dt) && pw_single_dispatched(K, N, res_mode, M, res_rows);
  if (block_list) ok = x3 && up && pw_single_x3_blocks_applicable(K, N, Ho, Wo, M, res_rows);
  if (!ok) {
    mcg_set_error("mcg_pointwise_stream: unsupported (dtype %d, %d -> %d channels, res_mode %d, M=%d%s): see include/mcgaze_hip.h for the table", (int)dt, K, N,
                  res_mode, M, block_list ? ", block list" : "");
    return MCG_ERR_UNSUPPORTED;
  }
  PwSingleParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.a = a; pp.res = res; pp.wf = wf; pp.bias = bias; pp.y = y;
  pp.M = M; pp.relu = relu; pp.Ho = up ? Ho : 1; pp.Wo = up ? Wo : 1; pp.wscale = x3 ? wscale : 0.f;
  if (up) { pp.Hr = Hr; pp.Wr = Wr; pp.rscale_h = (float)Hr / (float)Ho; pp.rscale_w = (float)Wr / (float)Wo; }
  const int rc = block_list ? launch_pw_single_x3_blocks((hipStream_t)s, pp, block_list, block_count, M / 64, grid_cap)
                 : x3       ? launch_pw_single_x3((hipStream_t)s, pp, N, res_mode, grid_cap)
                            : launch_pw_single((hipStream_t)s, pp, K, N, res_mode, dt, grid_cap);
  if (rc) { mcg_set_error("mcg_pointwise_stream: launch failed"); return MCG_ERR_HIP; }
  return MCG_OK;
}

extern "C" int mcg_pointwise_pair(mcg_stream s, mcg_dtype dt, const void* a1, const void* a2, const void* res, const void* w3f, const float* b3,
                                  void* y, const void* w1f, const float* b1, void* z, int M, int K2, int C2, int grid_cap) {
  MCG_CHECK_ARG(a1 && w3f && b3 && y && w1f && b1 && z, "mcg_pointwise_pair: null pointer");
  MCG_CHECK_ARG(M > 0 && grid_cap >= 0, "mcg_pointwise_pair: M must be positive and grid_cap >= 0 (M=%d grid_cap=%d)", M, grid_cap);
  MCG_CHECK_ARG((a2 != nullptr) == (K2 != 0), "mcg_pointwise_pair: a second source comes with K2 = 64, none with K2 = 0");
  // the two-source form has ONE y tile (pw_pair.hpp): a residual's next tile would land in the tile being read
  if (!mcg_is16(dt) || !pw_pair_applicable(64, K2, 1, 256, C2, M) || (K2 != 0 && res)) {
    mcg_set_error("mcg_pointwise_pair: unsupported (dtype %d, K2=%d, C2=%d, M=%d%s): bf16 / fp16, K2 0 or 64, C2 64 or 128, a residual only without a second source",
                  (int)dt, K2, C2, M, res ? ", residual" : "");
    return MCG_ERR_UNSUPPORTED;
  }
  PwPairParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.a1 = a1; pp.K1 = 64; pp.a2 = a2; pp.K2 = K2; pp.stride2 = 1; pp.res = res;
  pp.w3f = w3f; pp.b3 = b3; pp.y = y; pp.w1f = w1f; pp.b1 = b1; pp.z = z;
  pp.M = M; pp.C = 256; pp.C2 = C2; pp.Ho = 1; pp.Wo = M; pp.H2 = 1; pp.W2 = M;
  if (launch_pw_pair((hipStream_t)s, pp, dt, grid_cap)) { mcg_set_error("mcg_pointwise_pair: launch failed"); return MCG_ERR_HIP; }
  return MCG_OK;
}

extern "C" int mcg_backbone_fpn_forward(mcg_engine* e, mcg_stream s, const float* img, int N, int H, int W, int chunk,
                                        void* const pyramid[4], void* ws, size_t ws_bytes) {
  return trunk_forward(e, s, img, N, H, W, chunk, pyramid, ws, ws_bytes, false);
}
// Measurement entry point (bench.py --workload backbone, BASELINE.json configs[1] "R-50 backbone-only"): the trunk up to C5,
// no FPN; C2..C5 stay in the workspace.
extern "C" int mcg_bench_backbone_forward(mcg_engine* e, mcg_stream s, const float* img, int N, int H, int W, void* ws, size_t ws_bytes) {
  return trunk_forward(e, s, img, N, H, W, 0, nullptr, ws, ws_bytes, true);
}

// Where mcg_bench_backbone_forward left C2..C5 (NHWC, engine dtype) for a batch that ran as ONE frame range (trunk_streams = 1, or fewer
// than 112 frames): pointers into the caller's workspace.  Test / measurement aid.
extern "C" int mcg_bench_backbone_levels(const mcg_engine* e, void* ws, int N, int H, int W, void* levels[4]) {
  MCG_CHECK_ARG(e && ws && levels, "mcg_bench_backbone_levels: null pointer");
  MCG_TRY(check_shape(N, H, W));
  MCG_CHECK_ARG(trunk_ranges(e, N) == 1 && N <= range_frame_cap(e, H, W), "mcg_bench_backbone_levels: the batch runs as several frame ranges (set trunk_streams = 1)");
  const TrunkWs t = trunk_layout(e->dt, N, H, W, (char*)ws);
  for (int i = 0; i < 4; ++i) levels[i] = t.c[i];
  return MCG_OK;
}

// Deferred P2 before stage st's RoIAlign: list the 8 x 8 blocks of P2 [N, h, w] that the stage's boxes read and no earlier stage listed
// (roi_mark_kernel), then compute them from the inner map (wino_x3w_blocks_kernel: same bits as the dense conv).  Booked once, at stage 0.
// d.lateral: the inner map is computed here as well, between the two -- the listed blocks and their in-frame neighbours that no earlier
// stage computed (inner_mark_kernel), by the streaming lateral's per-pixel code over that list (pw_single_x3_blocks_kernel)
// d.level_mask: the same mark launch lists, per level deferred by frames, the frames one of the stage's boxes reads there and no earlier stage
// listed; each such level's output conv then runs over its list (wino_x3w_frames_kernel: the dense conv's bits), booked once, at stage 0.
static int defer_stage_forward(const mcg_engine* e, hipStream_t s, const DeferSlot& d, int st, const float* boxes, int N, const int fh[4],
                               const int fw[4]) {
  const mcg_conv_weights& cw = e->fpn_out[0];
  const int h = fh[0], w = fw[0];
  int* list = d.list + (size_t)st * d.nblk;
  int *fstate[4] = {nullptr, nullptr, nullptr, nullptr}, *flist[4] = {nullptr, nullptr, nullptr, nullptr}, *fcount[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 1; i < 4; ++i)
    if ((d.level_mask >> i) & 1) { fstate[i] = d.fstate[i]; flist[i] = d.flist[i] + (size_t)st * N; fcount[i] = d.fcount[i] + st; }
  MCG_TRY(launch_roi_mark(s, boxes, N * 3, 3, 0, h, w, 4, d.state, list, d.count + st, fstate, flist, fcount));
  for (int i = 1; i < 4; ++i) {
    if (!fstate[i]) continue;
    const mcg_conv_weights& fc = e->fpn_out[i];
    ProfRec* frec = prof_begin_wino(e->ctx, s, fc, (long long)N * fh[i] * fw[i], st == 0);
    MCG_TRY(launch_done(frec, s, launch_wino_x3_frames(s, wino_params(fc, 2, d.lin[i], N, fh[i], fw[i], d.p[i], 0), flist[i], fcount[i]), "wino_x3 frames"));
  }
  if (d.lateral) {
    const mcg_conv_weights& lw = e->lateral[0];
    int* ilist = d.ilist + (size_t)st * d.nblk;
    MCG_TRY(launch_inner_mark(s, list, d.count + st, h, w, d.nblk, d.istate, ilist, d.icount + st));
    const long long M = (long long)N * h * w, res_m = (long long)N * (h / 2) * (w / 2);
    PwSingleParams pp;
    memset(&pp, 0, sizeof(pp));
    pp.a = d.c2; pp.res = d.l1; pp.wf = lw.wf; pp.bias = lw.bias; pp.y = d.inner;
    pp.M = (int)M; pp.relu = 0; pp.Ho = h; pp.Wo = w; pp.wscale = lw.wscale;
    pp.Hr = h / 2; pp.Wr = w / 2; pp.rscale_h = (float)pp.Hr / (float)h; pp.rscale_w = (float)pp.Wr / (float)w;
    const bool book = st == 0;   // the dense lateral's FLOPs and bytes, once
    ProfRec* lrec = prof_begin(e->ctx, s, 71, pp.M, lw.cout, lw.cin, book ? 2.0 * M * lw.cin * lw.cout : 0.0,
                               book ? 4.0 * ((double)M * (lw.cin + lw.cout) + (double)res_m * lw.cout + (double)lw.cin * lw.cout) : 0.0);
    MCG_TRY(launch_done(lrec, s, launch_pw_single_x3_blocks(s, pp, ilist, d.icount + st, d.nblk), "pw_single_x3 block"));
  }
  ProfRec* rec = prof_begin_wino(e->ctx, s, cw, (long long)N * h * w, st == 0);
  return launch_done(rec, s, launch_wino_x3_blocks(s, wino_params(cw, 2, d.inner, N, h, w, d.p[0], 0), list, d.count + st, d.nblk), "wino_x3 block");
}

// The decoder over an existing pyramid; frame_of != NULL: window frame n reads pyramid row frame_of[n] of a store of pyramid_frames rows
// (RoIAlign and the query init gather through the table, roi_align.hip / decoder.hip), img_hw is then indexed by pyramid row.
// d != NULL and deferred: pyramid[0] is computed here, block by block, from d->inner -- before each stage's RoIAlign, the blocks its boxes
// read that no earlier stage listed (roi_mark_kernel, then wino_x3w_blocks_kernel: same bits as the dense conv).
// ct: how the N frames split into clips (igemm.hpp: ClipTable) -- read by the stages' temporal attention pass only.
static int decoder_forward(mcg_engine* e, hipStream_t s, const void* const pyramid[4], int pyramid_frames, const int32_t* frame_of, int N,
                           const ClipTable& ct, int H, int W, const int* img_hw, float* gaze_out, float* boxes_out, float* scores_out, void* ws,
                           size_t ws_bytes, const DeferSlot* d = nullptr) {
  MCG_CHECK_ARG(e && pyramid && gaze_out && boxes_out && scores_out && ws, "mcg_decoder_forward: null pointer");
  MCG_TRY(check_shape(N, H, W));
  MCG_TRY(check_clips("mcg_decoder_forward", N, ct));
  DecWs c = dec_layout(e->dt, N, (char*)ws);
  if (ws_bytes < c.total) { mcg_set_error("mcg_decoder_forward: workspace too small (%zu < %zu)", ws_bytes, c.total); return MCG_ERR_WORKSPACE; }
  MCG_TRY(launch_init_queries(s, e->dt, e->init_boxes, e->init_feats, img_hw, frame_of, pyramid_frames, H, W, c.boxes_a, c.obj_a, N));
  int fh[4], fw[4];
  const int strides[4] = {4, 8, 16, 32};
  for (int i = 0; i < 4; ++i) { fh[i] = (H / 4) >> i; fw[i] = (W / 4) >> i; }
  char* obj_in = c.obj_a; char* obj_out = c.obj_b;
  float* b_in = c.boxes_a; float* b_out = c.boxes_b;
  const bool defer = d && d->deferred;
  if (defer) MCG_TRY(launch_defer_clear(s, d->state, d->clear_n));
  for (int st = 0; st < e->num_stages; ++st) {
    if (defer) MCG_TRY(defer_stage_forward(e, s, *d, st, b_in, N, fh, fw));
    MCG_TRY(launch_roi_align(s, e->dt, pyramid, fh, fw, strides, 256, b_in, N * 3, 3, frame_of, pyramid_frames, c.roi, nullptr));
    float* bdst = (st == e->num_stages - 1) ? boxes_out : b_out;
    MCG_TRY(stage_forward_ctx(s, e->dt, &e->stage_w[(size_t)st * MCG_SW_COUNT], c.roi, obj_in, b_in, N, ct, obj_out, bdst,
                              c.cls, e->stds, c.stage_ws, c.stage_bytes, e->ctx));
    char* t = obj_in; obj_in = obj_out; obj_out = t;
    if (st != e->num_stages - 1) { float* tb = b_in; b_in = b_out; b_out = tb; }
  }
  MCG_TRY(gaze_head_ctx(s, e->dt, e->gaze_w, obj_in, N, gaze_out, c.gaze_ws, c.gaze_bytes, e->ctx, c.cls, scores_out));
  return MCG_OK;
}

extern "C" int mcg_decoder_forward(mcg_engine* e, mcg_stream s_, const void* const pyramid[4], int N, int clip_length, int H, int W,
                                   const int* img_hw, float* gaze_out, float* boxes_out, float* scores_out, void* ws, size_t ws_bytes) {
  return decoder_forward(e, (hipStream_t)s_, pyramid, N, nullptr, N, ClipTable::uniform(N, clip_length), H, W, img_hw, gaze_out, boxes_out, scores_out, ws,
                         ws_bytes);
}

extern "C" int mcg_decoder_forward_indexed(mcg_engine* e, mcg_stream s_, const void* const pyramid[4], int pyramid_frames, const int32_t* frame_of,
                                           int N, int clip_length, int H, int W, const int* img_hw, float* gaze_out, float* boxes_out,
                                           float* scores_out, void* ws, size_t ws_bytes) {
  MCG_CHECK_ARG(frame_of, "mcg_decoder_forward_indexed: null frame_of (mcg_decoder_forward is the plain path)");
  MCG_CHECK_ARG(pyramid_frames > 0, "mcg_decoder_forward_indexed: empty pyramid store (pyramid_frames=%d)", pyramid_frames);
  return decoder_forward(e, (hipStream_t)s_, pyramid, pyramid_frames, frame_of, N, ClipTable::uniform(N, clip_length), H, W, img_hw, gaze_out, boxes_out,
                         scores_out, ws, ws_bytes);
}

extern "C" int mcg_decoder_forward_ragged(mcg_engine* e, mcg_stream s_, const void* const pyramid[4], int pyramid_frames, const int32_t* frame_of,
                                          int N, const int* clip_start, int num_clips, int max_clip_length, int H, int W, const int* img_hw,
                                          float* gaze_out, float* boxes_out, float* scores_out, void* ws, size_t ws_bytes) {
  MCG_CHECK_ARG(clip_start, "mcg_decoder_forward_ragged: null clip_start (mcg_decoder_forward is the equal-length path)");
  MCG_CHECK_ARG(pyramid_frames > 0, "mcg_decoder_forward_ragged: empty pyramid store (pyramid_frames=%d)", pyramid_frames);
  MCG_CHECK_ARG(frame_of || pyramid_frames == N, "mcg_decoder_forward_ragged: without frame_of the pyramid holds one row per frame (%d rows, %d frames)",
                pyramid_frames, N);
  return decoder_forward(e, (hipStream_t)s_, pyramid, pyramid_frames, frame_of, N, ClipTable{clip_start, num_clips, max_clip_length}, H, W, img_hw,
                         gaze_out, boxes_out, scores_out, ws, ws_bytes);
}

extern "C" int mcg_deferred_pyramid_levels(const mcg_engine* e, void* slot, int N, int H, int W, void* levels[4], int* deferred) {
  MCG_CHECK_ARG(e && slot && levels, "mcg_deferred_pyramid_levels: null pointer");
  MCG_TRY(check_shape(N, H, W));
  const DeferSlot d = defer_layout(e, N, H, W, (char*)slot);
  for (int i = 0; i < 4; ++i) levels[i] = d.p[i];
  if (deferred) *deferred = d.deferred ? 1 : 0;
  return MCG_OK;
}

extern "C" int mcg_backbone_fpn_forward_deferred(mcg_engine* e, mcg_stream s, const float* img, int N, int H, int W, int chunk, void* slot,
                                                 size_t slot_bytes, void* ws, size_t ws_bytes) {
  MCG_CHECK_ARG(e && slot, "mcg_backbone_fpn_forward_deferred: null pointer");
  MCG_TRY(check_shape(N, H, W));
  const DeferSlot d = defer_layout(e, N, H, W, (char*)slot);
  if (slot_bytes < d.total) { mcg_set_error("mcg_backbone_fpn_forward_deferred: slot too small (%zu < %zu)", slot_bytes, d.total); return MCG_ERR_WORKSPACE; }
  return trunk_forward(e, s, img, N, H, W, chunk, d.p, ws, ws_bytes, false,
                       TrunkKeep{d.deferred ? d.inner : nullptr, d.lateral ? d.c2 : nullptr, d.lateral ? d.l1 : nullptr, {nullptr, d.lin[1], d.lin[2], d.lin[3]}});
}

// Test / measurement aid: where a deferred slot keeps the P2 inner map and the inner-block bookkeeping of the deferred lateral
// (flags [blocks], counts [stages], lists [stages][blocks]); *lateral_deferred = whether the engine defers the P2 lateral for this shape
// (else the bookkeeping pointers are NULL; inner is NULL where P2 is not deferred at all)
extern "C" int mcg_deferred_pyramid_state(const mcg_engine* e, void* slot, int N, int H, int W, void** inner, int** flags, int** counts, int** lists,
                                          int* blocks, int* lateral_deferred) {
  MCG_CHECK_ARG(e && slot, "mcg_deferred_pyramid_state: null pointer");
  MCG_TRY(check_shape(N, H, W));
  const DeferSlot d = defer_layout(e, N, H, W, (char*)slot);
  if (inner) *inner = d.inner;
  if (flags) *flags = d.istate;
  if (counts) *counts = d.icount;
  if (lists) *lists = d.ilist;
  if (blocks) *blocks = d.nblk;
  if (lateral_deferred) *lateral_deferred = d.lateral ? 1 : 0;
  return MCG_OK;
}

// Test / measurement aid: the frame bookkeeping of level (1 .. 3 = P3 .. P5) in a deferred slot (flags [N], counts [stages], lists [stages][N]);
// *frame_deferred = whether the engine defers that level by frames for this shape (else the pointers are NULL)
extern "C" int mcg_deferred_pyramid_frame_state(const mcg_engine* e, void* slot, int N, int H, int W, int level, int** flags, int** counts,
                                                int** lists, int* frame_deferred) {
  MCG_CHECK_ARG(e && slot && level >= 1 && level <= 3, "mcg_deferred_pyramid_frame_state: null pointer or level outside 1 .. 3");
  MCG_TRY(check_shape(N, H, W));
  const DeferSlot d = defer_layout(e, N, H, W, (char*)slot);
  if (flags) *flags = d.fstate[level];
  if (counts) *counts = d.fcount[level];
  if (lists) *lists = d.flist[level];
  if (frame_deferred) *frame_deferred = (d.level_mask >> level) & 1;
  return MCG_OK;
}

static int decoder_forward_deferred(mcg_engine* e, mcg_stream s, void* slot, size_t slot_bytes, int N, const ClipTable& ct, int H, int W,
                                    const int* img_hw, float* gaze_out, float* boxes_out, float* scores_out, void* ws, size_t ws_bytes) {
  MCG_CHECK_ARG(e && slot, "mcg_decoder_forward_deferred: null pointer");
  MCG_TRY(check_shape(N, H, W));
  const DeferSlot d = defer_layout(e, N, H, W, (char*)slot);
  if (slot_bytes < d.total) { mcg_set_error("mcg_decoder_forward_deferred: slot too small (%zu < %zu)", slot_bytes, d.total); return MCG_ERR_WORKSPACE; }
  return decoder_forward(e, (hipStream_t)s, d.p, N, nullptr, N, ct, H, W, img_hw, gaze_out, boxes_out, scores_out, ws, ws_bytes, &d);
}

extern "C" int mcg_decoder_forward_deferred(mcg_engine* e, mcg_stream s, void* slot, size_t slot_bytes, int N, int clip_length, int H, int W,
                                            const int* img_hw, float* gaze_out, float* boxes_out, float* scores_out, void* ws, size_t ws_bytes) {
  return decoder_forward_deferred(e, s, slot, slot_bytes, N, ClipTable::uniform(N, clip_length), H, W, img_hw, gaze_out, boxes_out, scores_out, ws, ws_bytes);
}

extern "C" int mcg_decoder_forward_deferred_ragged(mcg_engine* e, mcg_stream s, void* slot, size_t slot_bytes, int N, const int* clip_start,
                                                   int num_clips, int max_clip_length, int H, int W, const int* img_hw, float* gaze_out,
                                                   float* boxes_out, float* scores_out, void* ws, size_t ws_bytes) {
  MCG_CHECK_ARG(clip_start, "mcg_decoder_forward_deferred_ragged: null clip_start (mcg_decoder_forward_deferred is the equal-length path)");
  return decoder_forward_deferred(e, s, slot, slot_bytes, N, ClipTable{clip_start, num_clips, max_clip_length}, H, W, img_hw, gaze_out, boxes_out,
                                  scores_out, ws, ws_bytes);
}

static int clip_forward(mcg_engine* e, mcg_stream s_, const float* img, int N, const ClipTable& ct, int H, int W, const int* img_hw, int chunk,
                        float* gaze_out, float* boxes_out, float* scores_out, void* ws, size_t ws_bytes) {
  MCG_CHECK_ARG(e && img && gaze_out && boxes_out && scores_out && ws, "mcg_clip_forward: null pointer");
  MCG_TRY(check_shape(N, H, W));
  MCG_TRY(check_clips("mcg_clip_forward", N, ct));
  const size_t need = mcg_engine_workspace_bytes(e, N, H, W, chunk);
  if (ws_bytes < need) { mcg_set_error("mcg_clip_forward: workspace too small (%zu < %zu)", ws_bytes, need); return MCG_ERR_WORKSPACE; }
  char* base = (char*)ws;
  const size_t trunk_bytes = mcg_trunk_workspace_bytes(e, N, H, W, chunk);
  const size_t slot_bytes = defer_layout(e, N, H, W, nullptr).total;
  const size_t off = trunk_bytes + slot_bytes;
  MCG_TRY(mcg_backbone_fpn_forward_deferred(e, s_, img, N, H, W, chunk, base + trunk_bytes, slot_bytes, base, trunk_bytes));
  return decoder_forward_deferred(e, s_, base + trunk_bytes, slot_bytes, N, ct, H, W, img_hw, gaze_out, boxes_out, scores_out, base + off,
                                  ws_bytes - off);
}

extern "C" int mcg_clip_forward(mcg_engine* e, mcg_stream s_, const float* img, int N, int clip_length, int H, int W,
                                const int* img_hw, int chunk, float* gaze_out, float* boxes_out, float* scores_out,
                                void* ws, size_t ws_bytes) {
  return clip_forward(e, s_, img, N, ClipTable::uniform(N, clip_length), H, W, img_hw, chunk, gaze_out, boxes_out, scores_out, ws, ws_bytes);
}

extern "C" int mcg_clip_forward_ragged(mcg_engine* e, mcg_stream s_, const float* img, int N, const int* clip_start, int num_clips,
                                       int max_clip_length, int H, int W, const int* img_hw, int chunk, float* gaze_out, float* boxes_out,
                                       float* scores_out, void* ws, size_t ws_bytes) {
  MCG_CHECK_ARG(clip_start, "mcg_clip_forward_ragged: null clip_start (mcg_clip_forward is the equal-length path)");
  return clip_forward(e, s_, img, N, ClipTable{clip_start, num_clips, max_clip_length}, H, W, img_hw, chunk, gaze_out, boxes_out, scores_out, ws,
                      ws_bytes);
}
