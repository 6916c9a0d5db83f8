// HBM-bound 1x1 convolutions of the bf16 engine -- layer2's conv1 512 -> 128 and conv3 128 -> 512 + residual, layer3's conv3
// 256 -> 1024 + residual and first conv1 512 -> 256, the FPN laterals P2 / P3 with their nearest-upsampled top-down term, and the
// decoder's `dynamic_layer` (256 -> 32768 on 1344 tokens) -- as a persistent streaming kernel: pw_pair.hpp's structure with one
// contraction,
//
//     y = [relu]( A . W^T + b (+ res | + up(res)) )        A [M][K], W [N][K]; per workgroup a slice of W of N_wg * K * 2 B <= 128 KB
//
// The generic contraction kernel runs these at 3.2-4.6 TB/s (a fresh prologue / epilogue per 256-row tile, K of 2-8 K-tiles); here a
// workgroup keeps the whole weight matrix in REGISTERS (128 VGPRs per wave), walks 32-pixel tiles with a grid-stride loop, and the
// next tile's A rows and residual rows travel HBM -> LDS by `buffer_load ... lds` while the current tile is contracted and stored:
// two workgroups per CU, no global load inside the loop other than those DMAs (biases sit in LDS -- a load queued behind the next
// tile's DMA would drain the prefetch, pw_pair.hpp), transposed MFMAs so that bias / residual / ReLU / bf16 rounding work on 8-byte
// pieces in the LDS tile that the coalesced store reads.  K order and rounding points are the generic kernel's: bit-identical.
#pragma once
#include "igemm_dma.hpp"

struct PwSingleParams {
  const void* a;            // [M][K] bf16, rows contiguous
  const void* res;          // RES 1: [M][N]; RES 2: [frames][Hr][Wr][N] gathered at (y * Hr / Ho, x * Wr / Wo) (F.interpolate nearest)
  const void* wf;           // [N/32][K/16][64][8] fragment-major
  const float* bias;        // [N]
  void* y;                  // [M][N]
  int M, relu, Ho, Wo, Hr, Wr;
  float rscale_h, rscale_w;
  int many_slices;          // 1: far more channel slices than XCDs (dynamic_layer: 128): workgroup id = walker * NSPLIT + slice
  float wscale;             // f16x3 (pw_single_x3.hpp): accumulators x this power of two before the bias (pre-scaled weights); 0 = 1
};

// What pw_single_kernel and pw_single_x3.hpp's kernels share, each piece stated once: the LDS layout that kernel and launcher both read,
// the workgroup placement, the swizzle, the tile movers, the tile store, the persistent grids and the launch.
namespace pwx {
constexpr int LDS_BUDGET = 80 * 1024;   // half a CU's LDS: two workgroups per CU

// LDS chunk (16 bytes) that holds chunk `chunk` of tile row `row`, rows of CH chunks: bank-conflict-free fragment reads and row reads
template <int CH>
__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ (row & (CH >= 32 ? 31 : 15)); }

// A workgroup's LDS: [NYB y / residual tiles][NAB A tiles][biases]; a tile is PX = 32 pixel rows, row r's chunk c at swz(r, c).  EB: bytes
// per element; K = 16 KS; N = 128 TPW output channels per workgroup (TPW 32-channel tiles per wave, 4 waves); RES != 0: two y tiles (the
// residual of the next tile lands early); NAB_ARG: the number of A tiles where the rule below is not to decide it
template <int EB, int KS, int TPW, int RES, int NAB_ARG = 0>
struct Layout {
  using Elem = std::conditional_t<EB == 2, bf16_t, float>;   // a type of the element's size (the store's pointer arithmetic)
  static constexpr int PX = 32, K = 16 * KS, N = 128 * TPW, EPC = 16 / EB;
  static constexpr int AROWB = EB * K, YROWB = EB * N, ACH = AROWB / 16, YCH = YROWB / 16;   // bytes and chunks per row
  static constexpr int ABYTES = PX * AROWB, YBYTES = PX * YROWB;
  static constexpr int A_PIECES = ABYTES / 1024 / 4, Y_PIECES = YBYTES / 1024 / 4;            // 1 KiB DMA pieces per wave
  static constexpr int A_LPR = ACH < 64 ? ACH : 64, Y_LPR = YCH < 64 ? YCH : 64;              // lanes per row within a piece
  static constexpr int A_RPP = 64 / A_LPR, Y_RPP = 64 / Y_LPR;                                // rows per piece (1 KiB = 64 chunks)
  static constexpr int NYB = RES ? 2 : 1;
  static constexpr bool BIAS_REGS = TPW == 1;   // one channel tile per wave: its 16 biases stay in registers (read before any DMA)
  static constexpr int BIASB = BIAS_REGS ? 0 : N * 4;
  static constexpr int NAB = NAB_ARG ? NAB_ARG : (2 * ABYTES + NYB * YBYTES + BIASB <= LDS_BUDGET ? 2 : 1);   // A tiles: double-buffered when two workgroups still fit a CU
  static constexpr int AOFF = NYB * YBYTES, BOFF = AOFF + NAB * ABYTES, kLds = BOFF + BIASB;
  static_assert(ACH <= 64 && YCH <= 64, "rows longer than 1 KiB are not laid out here");
  static_assert(A_PIECES >= 1 && Y_PIECES >= 1, "tile geometry");
  static_assert(kLds <= LDS_BUDGET, "two workgroups per CU");
  __device__ static __forceinline__ int a_off(int r, int chunk) { return r * AROWB + (swz<ACH>(r, chunk) << 4); }
  __device__ static __forceinline__ int y_off(int r, int chunk) { return r * YROWB + (swz<YCH>(r, chunk) << 4); }
};

// Workgroup id -> (channel slice, walker, walkers per slice).  Workgroups go round-robin over the 8 XCDs, so ids 8 apart sit on the same
// XCD (one L2): the NSPLIT slices of a walker take such ids, the A tile comes from HBM once and from L2 for the others.  many_slices (far
// more slices than XCDs, dynamic_layer): id = walker * NSPLIT + slice
struct Place { int nsp, walker, nwalkers; };
template <int NSPLIT>
__device__ __forceinline__ Place place(int many_slices) {
  const int bid = blockIdx.x;
  return {many_slices ? bid % NSPLIT : (bid >> 3) % NSPLIT, many_slices ? bid / NSPLIT : (bid / (8 * NSPLIT)) * 8 + (bid & 7), (int)(gridDim.x / NSPLIT)};
}

// "Row r of a tile -> pixel of [0, M)", what the movers and the store ask of a tile: pixel(r) = base() (uniform: it travels as the DMA's
// scalar offset) + rel(r); rows(): the tile's rows below this exist (the DMAs' test), has(r) (the store's).  Dense: tile t = pixels 32 t ..
// 32 t + 31
struct DenseRows {
  int tile, M;
  __device__ __forceinline__ int rows() const { return M - tile * 32; }
  __device__ __forceinline__ long long base() const { return (long long)tile * 32; }
  __device__ __forceinline__ int rel(int r) const { return r; }
  __device__ __forceinline__ int pixel(int r) const { return tile * 32 + r; }
  __device__ __forceinline__ bool has(int r) const { return base() + r < M; }
};

// Tile movers, HBM -> LDS in 1 KiB pieces: lane-linear on the LDS side, the swizzle on the source chunk; a row the tile does not have reads
// as zeros (MCG_OOB_OFFSET).  The A rows into A buffer `buf` (M * AROWB fits the descriptor window: the launchers' predicates)
template <typename L, typename Rows>
__device__ __forceinline__ void issue_a(const Rows& t, int buf, const u32x4& srd, uint32_t lds_base, int wave, int lane) {
  const int rows_left = t.rows();
  const uint32_t so = (uint32_t)t.base() * L::AROWB;
  static_for<L::A_PIECES>([&](auto jc) {
    constexpr int J = decltype(jc)::value;
    const int row = (wave * L::A_PIECES + J) * L::A_RPP + lane / L::A_LPR, pos = lane % L::A_LPR;
    const uint32_t vo = row < rows_left ? (uint32_t)t.rel(row) * L::AROWB + (uint32_t)(swz<L::ACH>(row, pos) << 4) : MCG_OOB_OFFSET;
    lds_dma16<L::AOFF + J * 1024>(vo, srd, so, lds_base + buf * L::ABYTES + wave * (L::A_PIECES * 1024));
  });
}
// The residual rows of slice nsp into y tile `buf`.  RES 1: the tile's own rows of [M][N NSPLIT]; RES 2: the nearest-upsample gather
template <typename L, int RES, int NSPLIT, typename Rows>
__device__ __forceinline__ void issue_res(const Rows& t, int buf, const PwSingleParams& p, int nsp, const u32x4& srd, uint32_t lds_base, int wave, int lane) {
  constexpr int GROWB = L::YROWB * NSPLIT;
  const int rows_left = t.rows();
  static_for<L::Y_PIECES>([&](auto jc) {
    constexpr int J = decltype(jc)::value;
    const int row = (wave * L::Y_PIECES + J) * L::Y_RPP + lane / L::Y_LPR, pos = lane % L::Y_LPR;
    const int chunk = swz<L::YCH>(row, pos);
    uint32_t vo = MCG_OOB_OFFSET, so = 0;
    if (RES == 1) {
      so = (uint32_t)t.base() * GROWB + nsp * L::YROWB;
      if (row < rows_left) vo = (uint32_t)(t.rel(row) * GROWB + (chunk << 4));
    } else if (row < rows_left) {
      const long long src = nearest_src_row(t.pixel(row), p.Ho * p.Wo, p.Wo, p.Hr, p.Wr, p.rscale_h, p.rscale_w);
      vo = (uint32_t)(src * GROWB + nsp * L::YROWB + (chunk << 4));
    }
    lds_dma16<J * 1024>(vo, srd, so, lds_base + buf * L::YBYTES + wave * (L::Y_PIECES * 1024));
  });
}
// The finished y tile s_y -> slice nsp of y [M][N NSPLIT], 16 bytes per lane, coalesced along rows
template <typename L, int NSPLIT, typename Rows>
__device__ __forceinline__ void store_tile(const Rows& t, const char* s_y, void* y, int nsp, int tid) {
  for (int idx = tid; idx < L::PX * L::YCH; idx += 256) {
    const int r = idx / L::YCH, c = idx - r * L::YCH;
    if (t.has(r)) *(uint4*)((typename L::Elem*)y + (t.base() + t.rel(r)) * (L::N * NSPLIT) + nsp * L::N + c * L::EPC) = *(const uint4*)(s_y + L::y_off(r, c));
  }
}

// Persistent grids.  Sliced: two workgroups per CU in whole groups of NSPLIT slices x 8 XCDs, no more groups than there are tiles.
// cap (here and below; 0 = none): a host-side limit for the stand-alone entry points (mcg_pointwise_*), which walk many tiles per workgroup
// on a small problem with it; the engine and the decoder pass 0.  Sliced: at most cap groups
static inline int sliced_grid(int cus, int ntiles, int nsplit, int cap = 0) {
  const int unit = 8 * nsplit, need = (ntiles + 7) / 8 * unit;
  int wgs = 2 * cus / unit * unit;
  if (wgs < unit) wgs = unit;
  if (need < wgs) wgs = need;
  return cap > 0 && (long long)cap * unit < wgs ? cap * unit : wgs;
}
// many_slices: walkers per slice, two workgroups per CU (dynamic_layer's 128 slices: 4 walkers per slice on 256 CUs; 2, 3, 6, 8 measured
// slower); at most cap walkers
static inline int slice_walkers(int cus, int ntiles, int nsplit, int cap = 0) {
  int walkers = 2 * cus / nsplit < 1 ? 1 : 2 * cus / nsplit;
  if (walkers > ntiles) walkers = ntiles;
  return cap > 0 && cap < walkers ? cap : walkers;
}
// Kernel with layout L over ntiles tiles: dynamic LDS from the layout, the grid by the form the kernel will read in p.many_slices
template <auto Kernel, typename L, int NSPLIT, typename... Args>
static inline int launch(hipStream_t s, int ntiles, int many_slices, int cap, const Args&... args) {
  int cus;
  if (kernel_ready<Kernel>(L::kLds, &cus)) return 1;
  const int wgs = many_slices ? slice_walkers(cus, ntiles, NSPLIT, cap) * NSPLIT : sliced_grid(cus, ntiles, NSPLIT, cap);
  hipLaunchKernelGGL(Kernel, dim3(wgs), dim3(256), L::kLds, s, args...);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
// res_mode 0 / 1 / 2 -> f(RES as a compile-time constant)
template <typename Fn>
static inline int dispatch_res(int res_mode, Fn&& f) {
  if (res_mode == 0) return f(std::integral_constant<int, 0>{});
  if (res_mode == 1) return f(std::integral_constant<int, 1>{});
  return f(std::integral_constant<int, 2>{});
}
}  // namespace pwx

// K = 16 KS; a workgroup owns N = 128 TPW output channels (TPW 32-channel tiles per wave, 4 waves) of the NSPLIT * N the layer has:
// NSPLIT workgroups on one XCD (one L2) walk the same pixel tiles, each with its own slice of the weights in registers (pwx::place).
// RES: 0 none, 1 same-shape add, 2 nearest-upsample add.
template <int KS, int TPW, int RES> using PwLayout = pwx::Layout<2, KS, TPW, RES>;
template <typename F, int KS, int TPW, int RES, int NSPLIT>
__global__ __launch_bounds__(256, 2) void pw_single_kernel(const PwSingleParams p) {
  using L = PwLayout<KS, TPW, RES>;
  constexpr int N = L::N, YBYTES = L::YBYTES, ABYTES = L::ABYTES, NAB = L::NAB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_bias = (float*)(smem + L::BOFF);
  const int tid = threadIdx.x, lane = tid & 63, px = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const pwx::Place at = pwx::place<NSPLIT>(p.many_slices);
  const int nsp = at.nsp, walker = at.walker, nwalkers = at.nwalkers;
  float4 breg[4];
  if constexpr (L::BIAS_REGS) {
#pragma unroll
    for (int q = 0; q < 4; ++q) breg[q] = *(const float4*)(p.bias + nsp * N + wave * 32 + 8 * q + 4 * (lane >> 5));
  } else {
    for (int i = tid; i < N; i += 256) s_bias[i] = p.bias[nsp * N + i];
  }
  // ---- weights, once per workgroup: wave -> channel tiles wave * TPW + i
  uint4 w[TPW][KS];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const char* wb = (const char*)p.wf + ((size_t)((nsp * 4 + wave) * TPW + i) * KS * 64 + lane) * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) w[i][ks] = *(const uint4*)(wb + (size_t)ks * 1024);
  }
  const u32x4 srd_a = make_srd(p.a), srd_r = make_srd(RES ? p.res : p.a);
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int ntiles = (p.M + L::PX - 1) / L::PX;
  auto issue_a = [&](int tile, int buf) { pwx::issue_a<L>(pwx::DenseRows{tile, p.M}, buf, srd_a, lds_base, wave, lane); };
  auto issue_res = [&](int tile, int buf) { pwx::issue_res<L, RES, NSPLIT>(pwx::DenseRows{tile, p.M}, buf, p, nsp, srd_r, lds_base, wave, lane); };
  if (walker < ntiles) {
    if (RES) issue_res(walker, 0);
    issue_a(walker, 0);
  }
  __syncthreads();   // biases in LDS (the loop's first wait covers the register copies)
  int it = 0;
  for (int tile = walker; tile < ntiles; tile += nwalkers, ++it) {
    char* s_y = smem + (RES ? (it & 1) * YBYTES : 0);
    const char* s_a = smem + L::AOFF + (NAB == 2 ? (it & 1) * ABYTES : 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of the tile have landed (and its earlier stores left)
    __syncthreads();                                           // everyone's pieces landed; the other buffers are free
    const bool more = tile + nwalkers < ntiles;
    if (more) {
      if (RES) issue_res(tile + nwalkers, (it + 1) & 1);
      if (NAB == 2) issue_a(tile + nwalkers, (it + 1) & 1);
    }
    // ---- contraction: wave -> TPW channel tiles x one pixel tile, K ascending
    f32x16 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint4 x = *(const uint4*)(s_a + L::a_off(px, 2 * ks + half));
#pragma unroll
      for (int i = 0; i < TPW; ++i) Mma<F>::run(acc[i], w[i][ks], x);
    }
    if (RES == 0) __syncthreads();                             // previous tile's y staging fully stored (single y tile)
    // ---- epilogue: (acc + bias) (+ res) -> [relu] -> bf16, 8 bytes (4 channels of one pixel) at a time, into the y tile
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = (wave * TPW + i) * 32 + 8 * q + 4 * half;
        float4 b4;
        if constexpr (L::BIAS_REGS) b4 = breg[q]; else b4 = *(const float4*)(s_bias + c0);
        char* slot = s_y + L::y_off(px, c0 >> 3) + (c0 & 7) * 2;
        float v[4] = {acc[i][4 * q] + b4.x, acc[i][4 * q + 1] + b4.y, acc[i][4 * q + 2] + b4.z, acc[i][4 * q + 3] + b4.w};
        if (RES) {
          const uint2 rr = *(const uint2*)slot;
          v[0] += H16<F>::lo(rr.x); v[1] += H16<F>::hi(rr.x);
          v[2] += H16<F>::lo(rr.y); v[3] += H16<F>::hi(rr.y);
        }
        *(uint2*)slot = p.relu ? relu_pack4<F>(v) : make_uint2(H16<F>::pack2(v[0], v[1]), H16<F>::pack2(v[2], v[3]));
      }
    }
    __syncthreads();                                           // y tile complete; the A tile has been consumed by every wave
    if (NAB == 1 && more) issue_a(tile + nwalkers, 0);        // single A tile: refill it now
    pwx::store_tile<L, NSPLIT>(pwx::DenseRows{tile, p.M}, s_y, p.y, nsp, tid);
  }
}

// (K, N) pairs of the R-50 trunk whose weights -- or a 128 / 256-channel slice of them -- fit the registers of one workgroup (128 KB):
// what launch_pw_single_f dispatches, for any M >= 1 whose operands fit the DMA descriptors (mcg_pointwise_stream) ...
static inline bool pw_single_dispatched(int K, int N, int res_mode, long long M, long long res_rows) {
  const bool shape = (K == 256 && N == 256) || (K == 512 && N == 128 && res_mode == 0) || (K == 128 && N == 512) ||
                     (K == 256 && N == 1024) || (K == 512 && N == 256 && res_mode != 1);
  return shape && M * 2 * (K > N ? K : N) < MCG_DMA_MAX_BYTES && res_rows * 2 * N < MCG_DMA_MAX_BYTES;
}
// ... and where the engine takes it: from 64 Ki rows on
static inline bool pw_single_applicable(int K, int N, int res_mode, long long M, long long res_rows) {
  return M >= 64 * 1024 && pw_single_dispatched(K, N, res_mode, M, res_rows);
}
template <typename F, int KS, int TPW, int RES, int NSPLIT>
static inline int launch_pw_single_t(hipStream_t s, const PwSingleParams& p, int cap = 0) {
  return pwx::launch<pw_single_kernel<F, KS, TPW, RES, NSPLIT>, PwLayout<KS, TPW, RES>, NSPLIT>(s, (p.M + 31) / 32, p.many_slices, cap, p);
}
template <typename F>
static inline int launch_pw_single_f(hipStream_t s, const PwSingleParams& p, int K, int N, int res_mode, int cap) {
  if (K == 512 && N == 128) return launch_pw_single_t<F, 32, 1, 0, 1>(s, p, cap);
  if (K == 512 && N == 256) return res_mode == 0 ? launch_pw_single_t<F, 32, 1, 0, 2>(s, p, cap) : launch_pw_single_t<F, 32, 1, 2, 2>(s, p, cap);
  return pwx::dispatch_res(res_mode, [&](auto rc) {
    constexpr int RES = decltype(rc)::value;
    if (K == 256 && N == 256) return launch_pw_single_t<F, 16, 2, RES, 1>(s, p, cap);
    if (K == 256 && N == 1024) return launch_pw_single_t<F, 16, 2, RES, 4>(s, p, cap);
    return launch_pw_single_t<F, 8, 4, RES, 1>(s, p, cap);
  });
}
static inline int launch_pw_single(hipStream_t s, const PwSingleParams& p, int K, int N, int res_mode, mcg_dtype dt, int cap = 0) {
  return dispatch_elem16(dt, [&](auto e) { return launch_pw_single_f<decltype(e)>(s, p, K, N, res_mode, cap); });
}

// DynamicConv's `dynamic_layer` (transformer.py:1131-1134): y[M][32768] = x[M][256] . W^T + b with FEW rows (1344 tokens at 64 clips) and
// 88 MB of output.  The generic kernel spends it in prologues and epilogues (4 K-tiles per 256x128 output tile: 55 us, 1.6 TB/s of
// writes).  Here: 128 slices of 256 columns, each slice's weights resident in the registers of a few workgroups ("walkers") that
// split the token tiles between them; the tokens (688 KB) stream out of L2.  Same arithmetic as every pw_single launch: bit-identical.
static inline bool pw_dyn_applicable(int M) { return M >= 256 && (long long)M * 512 < MCG_DMA_MAX_BYTES; }
static inline int launch_pw_dyn(hipStream_t s, const PwSingleParams& p, mcg_dtype dt, int cap = 0) {
  PwSingleParams q = p;
  q.many_slices = 1;
  return dispatch_elem16(dt, [&](auto e) { return launch_pw_single_t<decltype(e), 16, 2, 0, 128>(s, q, cap); });
}
