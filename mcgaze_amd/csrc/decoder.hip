// Decoder-side kernels: multi-clue spatial/temporal attention core, fused LayerNorm chains,
// the DynamicConv instance-interaction core, per-clue box/score heads with delta2bbox, the
// gaze head tail, and query initialisation.  GEMM-shaped work goes through igemm.hpp.
#include "igemm.hpp"
#include "chain.hpp"
#include "attn_block.hpp"
#include "pw_single.hpp"
#include "igemm_dma.hpp"
#include "attn_block_x3.hpp"
#include "pw_single_x3.hpp"

#include <string.h>

// ------------------------------------------------------------------------------------------------
// Attention core (nn.MultiheadAttention inside mmcv's wrapper, gaze_stqi_head.py:151,162):
// 8 heads x 32 dims, softmax over the L tokens of one group.  One workgroup per group; thread =
// (query token, head), no cross-lane reduction (attn_block.hpp: attend_row_head).
// The bf16 engine runs both attention passes of a stage in attn_block_kernel instead whenever a clip's 3 T rows fit one MFMA tile.
//   spatial : group = frame,        tokens r = g*3 + i            (L = 3 clues)
//   temporal: group = (clip, clue), tokens r = (b*T + i)*3 + c    (L = T frames)
// Ragged batch (clip_start != NULL, temporal only): clip b spans frames [clip_start[b], clip_start[b + 1]) -- base and L come from the table
// (attn_block.hpp: clip_span, one scalar load pair per workgroup; L is then the longest clip's length, the guard's cap).
template <typename T>
__global__ __launch_bounds__(256) void attn_core_kernel(const T* __restrict__ qkv, T* __restrict__ out, int L, int temporal, int clip_len, float scale,
                                                        const int32_t* __restrict__ clip_start, int num_frames) {
  const int g = blockIdx.x;
  long long base; int step;
  bool bad = false;
  if (temporal) {
    const int b = g / 3, c = g - b * 3;
    step = 3;
    if (clip_start) {
      const ClipSpan cs = clip_span(clip_start, b, num_frames, L);
      base = (long long)cs.first * 3 + c; L = cs.len; bad = cs.bad;
    } else {
      base = (long long)b * clip_len * 3 + c;
    }
  }
  else { base = (long long)g * 3; step = 1; }
  const int D = 256;
  for (int pair = threadIdx.x; pair < L * 8; pair += 256) {   // thread = (query token of the group, head)
    const int i = pair >> 3, h = pair & 7;
    const long long ri = base + (long long)i * step;
    if (bad) {                                                // a clip the table guard clamped: NaN rows, nothing read
      for (int d = 0; d < 32; ++d) Elem<T>::st(out + ri * D + h * 32 + d, __builtin_nanf(""));
      continue;
    }
    attend_row_head<T>(qkv + ri * (3 * D) + h * 32,
                       [&](int j) { return qkv + (base + (long long)j * step) * (3 * D) + D + h * 32; },
                       [&](int j) { return qkv + (base + (long long)j * step) * (3 * D) + 2 * D + h * 32; }, L, scale, out + ri * D + h * 32);
  }
}

// ------------------------------------------------------------------------------------------------
// LayerNorm chain over rows of width D (64 <= D <= 256, D % 64 == 0), one wave per row:
//   v = src row (T)  or  sum of split-K slabs (f32)  [+ bias]
//   if ln1: v = LN1(v) [ReLU]          if res: v += res row          if ln2: v = LN2(v) [ReLU]
// LN parameters may differ per row group (rows_per_group rows share one parameter set).
struct LnParams {
  const void* src; const float* partial; int slabs; long long slab_stride;
  const float* bias;
  const float* g1; const float* b1; int relu1;
  const void* res;
  const float* g2; const float* b2; int relu2;
  void* dst;
  int M, D; long long src_ld, res_ld, dst_ld;
  int rows_per_group; int param_stride;
};

template <typename T>
__global__ __launch_bounds__(256) void ln_kernel(const LnParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= p.M) return;
  const int per = p.D / 64;  // elements per lane (<= 4), lane owns columns lane*per .. +per
  const int c0 = lane * per;
  const int grp = row / p.rows_per_group;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e >= per) { v[e] = 0.f; continue; }
    float t;
    if (p.partial) {
      t = 0.f;
      for (int s = 0; s < p.slabs; ++s) t += p.partial[(long long)s * p.slab_stride + (long long)row * p.D + c0 + e];
    } else {
      t = Elem<T>::ld((const T*)p.src + (long long)row * p.src_ld + c0 + e);
    }
    if (p.bias) t += p.bias[c0 + e];
    v[e] = t;
  }
  const float invD = 1.0f / (float)p.D;
  auto norm = [&](const float* g, const float* b, int relu) {   // rowblock.hpp's pinned expressions on this lane's `per` values (LN_SQ_FMA)
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < per) s += v[e];
    const float sum = wave_sum(s);
    float d[4], q = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < per) { d[e] = ln_dev(v[e], sum, invD); q = e ? __builtin_fmaf(d[e], d[e], q) : d[0] * d[0]; }
    const float rstd = ln_rstd(wave_sum(q), invD);
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < per) {
      const float t = ln_affine(d[e], rstd, g[grp * p.param_stride + c0 + e], b[grp * p.param_stride + c0 + e]);
      v[e] = relu ? fmaxf(t, 0.f) : t;
    }
  };
  if (p.g1) norm(p.g1, p.b1, p.relu1);
  if (p.res) {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (e < per) v[e] += Elem<T>::ld((const T*)p.res + (long long)row * p.res_ld + c0 + e);
  }
  if (p.g2) norm(p.g2, p.b2, p.relu2);
#pragma unroll
  for (int e = 0; e < 4; ++e) if (e < per) Elem<T>::st((T*)p.dst + (long long)row * p.dst_ld + c0 + e, v[e]);
}

static int launch_ln(hipStream_t s, mcg_dtype dt, const LnParams& p) {
  MCG_CHECK_ARG(p.D % 64 == 0 && p.D <= 256 && p.M > 0, "layernorm: unsupported width %d", p.D);
  dim3 grid((p.M + 3) / 4);
  dispatch_elem(dt, [&](auto e) { hipLaunchKernelGGL(ln_kernel<decltype(e)>, grid, dim3(256), 0, s, p); });
  MCG_CHECK_LAUNCH("layernorm");
  return MCG_OK;
}

static LnParams ln_simple(const void* src, const float* g, const float* b, int relu, void* dst, int M, int D) {
  LnParams p;
  memset(&p, 0, sizeof(p));
  p.src = src; p.g1 = g; p.b1 = b; p.relu1 = relu; p.dst = dst; p.M = M; p.D = D;
  p.src_ld = D; p.res_ld = D; p.dst_ld = D; p.rows_per_group = 1 << 30; p.param_stride = 0;
  return p;
}
// The epilogue of a split-K linear: sum the f32 slabs [slabs][M][256] + bias, LN1 (g1 null: none), + res, LN2 -> dst (deterministic, no atomics)
static LnParams ln_splitk(const float* partial, int slabs, const float* bias, const float* g1, const float* b1, int relu1, const void* res,
                          const float* g2, const float* b2, void* dst, int M) {
  LnParams p = ln_simple(nullptr, g1, b1, relu1, dst, M, 256);
  p.partial = partial; p.slabs = slabs; p.slab_stride = (long long)M * 256; p.bias = bias; p.res = res; p.g2 = g2; p.b2 = b2;
  return p;
}

// ------------------------------------------------------------------------------------------------
// DynamicConv core (transformer.py:1131-1148), one workgroup (4 waves) per token:
//   F1 = ReLU(LN64 (F[49x256]  . Win[256x64]))     Win^T  = params[r][0     .. 16384): [64][256] in MFMA-fragment-major order
//   F2 = ReLU(LN256(F1[49x64]  . Wout[64x256]))    Wout^T = params[r][16384 .. 32768): [256][64] likewise (packing.py::dyn_permutation)
// The 49 positions are padded to 64 rows (2 MFMA row tiles).  MFMA operand fragments for F and
// the generated weights are read straight from global/L2 (each is used by one token only);
// F1 goes through LDS (f32 for the LayerNorm, then dtype, chunk-swizzled, as the next A operand).
// What the two kernels below share: the geometry and LDS budget, the D1 / D2 tile stores, the 64-wide LayerNorm (rowblock.hpp: ln64_relu)
// and the tail.  The contraction loops and the layout of A2 (F1 as the next A operand) are each kernel's own.
namespace dyn {
constexpr int P = 49, DI = 256, DF = 64;
constexpr int D1_LD = DF + 4, D2_LD = DI + 4;
constexpr int D1_BYTES = 64 * D1_LD * 4;
constexpr int D2_BYTES = P * D2_LD * 4;                    // D2 aliases D1 and A2 (barrier in between)
constexpr int lds_bytes(int a2_bytes) { return D2_BYTES > D1_BYTES + a2_bytes ? D2_BYTES : D1_BYTES + a2_bytes; }
// stage 1: the wave's 32x32 tile (tm, tn) of D1[64][64]
__device__ __forceinline__ void store_d1(float* D1, const f32x16& acc, int tm, int tn, int lane) {
#pragma unroll
  for (int i = 0; i < 16; ++i) D1[(tm * 32 + mfma32_row(i, lane)) * D1_LD + tn * 32 + (lane & 31)] = acc[i];
}
// stage 2: the wave's 2x2 tiles, columns [wave*64, +64) of D2[49][256] (the padding rows are not stored)
__device__ __forceinline__ void store_d2(float* D2, const f32x16 (&acc)[2][2], int wave, int lane) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = a * 32 + mfma32_row(i, lane);
        if (row < P) D2[row * D2_LD + wave * 64 + b * 32 + (lane & 31)] = acc[a][b][i];
      }
}
// LN over 256 channels + ReLU, one wave per position, lane owns 4 consecutive channels -> out_tok[49][256].  LN_SQ_FMA_FROM_D1: these tails
// sum the squares from d1 on, not ln_kernel's order (rowblock.hpp); nothing compares them with ln_kernel bit for bit, and their bits stay.
template <typename T>
__device__ __forceinline__ void tail(const float* D2, const float* __restrict__ g_out, const float* __restrict__ b_out, T* __restrict__ out_tok,
                                     int wave, int lane) {
  for (int row = wave; row < P; row += 4) {
    const float4 t = *(const float4*)(D2 + row * D2_LD + lane * 4);
    float v[4] = {t.x, t.y, t.z, t.w};
    ln256_row<LN_SQ_FMA_FROM_D1>(v, *(const float4*)(g_out + lane * 4), *(const float4*)(b_out + lane * 4), true);
    T* dst = out_tok + row * DI + lane * 4;
    if constexpr (sizeof(T) == 4) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    else *(uint2*)dst = make_uint2(H16<T>::pack2(v[0], v[1]), H16<T>::pack2(v[2], v[3]));
  }
}
}  // namespace dyn

template <typename T>
__global__ __launch_bounds__(256) void dynconv_kernel(const T* __restrict__ roi, const T* __restrict__ params,
                                                      const float* __restrict__ g_in, const float* __restrict__ b_in,
                                                      const float* __restrict__ g_out, const float* __restrict__ b_out,
                                                      T* __restrict__ out) {
  using namespace dyn;
  constexpr int EPC = Elem<T>::kPerChunk;
  constexpr int A2_ROWB = DF * (int)sizeof(T);            // bytes per F1 row as next A operand
  constexpr int A2_CPR = A2_ROWB / 16;
  constexpr int A2_RPB = (256 / A2_ROWB) > 0 ? (256 / A2_ROWB) : 1;
  __shared__ __attribute__((aligned(16))) char smem[lds_bytes(64 * A2_ROWB)];
  float* D1 = (float*)smem;
  float* D2 = (float*)smem;
  char* A2 = smem + D1_BYTES;

  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* __restrict__ F = roi + (long long)r * P * DI;
  const T* __restrict__ Win = params + (long long)r * (2 * DI * DF);
  const T* __restrict__ Wout = Win + DI * DF;

  // ---- stage 1: wave -> one 32x32 tile of D1[64][64]
  {
    const int tm = wave >> 1, tn = wave & 1;
    const int prow = tm * 32 + (lane & 31);
    const bool pv = prow < P;
    const T* ap = F + (long long)prow * DI + (lane >> 5) * EPC;
    // the generated weights arrive MFMA-fragment-major (packing.py::dyn_permutation): chunk pair j of column tile tn = one contiguous KiB
    const T* bp = Win + ((long long)tn * (DI / (2 * EPC)) * 64 + lane) * EPC;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    constexpr int PAIRS = DI / (2 * EPC);
    // all operand fragments of a group of K-steps are in flight together (one L2 latency per group, not one per step): the
    // kernel is latency-bound -- every operand is used by one token only and comes straight from L2
    constexpr int GRP = PAIRS < 8 ? PAIRS : 8;
#pragma unroll
    for (int j0 = 0; j0 < PAIRS; j0 += GRP) {
      uint4 a[GRP], b[GRP];
#pragma unroll
      for (int j = 0; j < GRP; ++j) {
        a[j] = pv ? *(const uint4*)(ap + (j0 + j) * 2 * EPC) : make_uint4(0, 0, 0, 0);
        b[j] = *(const uint4*)(bp + (j0 + j) * 64 * EPC);
      }
#pragma unroll
      for (int j = 0; j < GRP; ++j) Mma<T>::run(acc, a[j], b[j]);
    }
    store_d1(D1, acc, tm, tn, lane);
  }
  // stage 2's weight fragments (wave -> columns [wave*64, +64) of Wout^T, K = 64): issued now, consumed after the LayerNorm below
  constexpr int PAIRS2 = DF / (2 * EPC);
  uint4 bf2[PAIRS2][2];
#pragma unroll
  for (int j = 0; j < PAIRS2; ++j)
#pragma unroll
    for (int b = 0; b < 2; ++b) bf2[j][b] = *(const uint4*)(Wout + ((long long)((wave * 2 + b) * PAIRS2 + j) * 64 + lane) * EPC);
  __syncthreads();
  // ---- LN over 64 features + ReLU, one wave per row, lane = feature; write F1 as dtype A operand
  for (int row = wave; row < 64; row += 4) {
    const float v = ln64_relu(D1[row * D1_LD + lane], g_in[lane], b_in[lane]);
    const int chunk = lane / EPC, within = lane % EPC;
    T* dst = (T*)(A2 + row * A2_ROWB + ((chunk ^ ((row / A2_RPB) % A2_CPR)) << 4)) + within;
    Elem<T>::st(dst, v);
  }
  __syncthreads();  // D1 fully consumed, A2 complete
  // ---- stage 2: wave -> columns [wave*64, +64) of D2[64][256], 2x2 tiles, K = 64
  {
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
    constexpr int PAIRS = DF / (2 * EPC);
#pragma unroll
    for (int j = 0; j < PAIRS; ++j) {
      const int ch = 2 * j + (lane >> 5);
      uint4 af[2], bf[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int row = a * 32 + (lane & 31);
        af[a] = *(const uint4*)(A2 + row * A2_ROWB + ((ch ^ ((row / A2_RPB) % A2_CPR)) << 4));
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) bf[b] = bf2[j][b];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) Mma<T>::run(acc[a][b], af[a], bf[b]);
    }
    __syncthreads();  // every wave is done reading A2 before D2 (which aliases it) is written
    store_d2(D2, acc, wave, lane);
  }
  __syncthreads();
  tail(D2, g_out, b_out, out + (long long)r * P * DI, wave, lane);
}

// The same in the f16x3 arithmetic (MCG_F16X3 engine; round 5): f32 storage, both operands of both contractions split into fp16 high / low
// parts, three v_mfma_f32_32x32x16_f16 per product (lo.hi + hi.lo + hi.hi, the contraction kernels' order) instead of f32 MFMAs at 1/16 of
// the rate.  The generated weights arrive in THIS kernel's fragment order (packing.py::dyn_permutation(epc = 8): a lane's eight K elements of a
// 32x32x16 step are 32 contiguous bytes, a wave's two loads 2 KiB) and are split in registers; F1 is split ONCE when the LayerNorm writes
// it and parked in LDS as fp16 high / low planes (its four readers would each split it again).  Round 3 measured an x3 DynamicConv with
// K-contiguous parameter rows (a load touched 32 rows x 32 bytes) as slower than the f32 kernel; with whole-KiB loads it is the faster one.
__global__ __launch_bounds__(256) void dynconv_x3_kernel(const float* __restrict__ roi, const float* __restrict__ params,
                                                         const float* __restrict__ g_in, const float* __restrict__ b_in,
                                                         const float* __restrict__ g_out, const float* __restrict__ b_out,
                                                         float* __restrict__ out) {
  using namespace dyn;
  constexpr int A2_ROWB = DF * 2;                          // bytes per F1 row of one fp16 plane
  constexpr int A2_PLANE = 64 * A2_ROWB;                   // 8 KiB
  __shared__ __attribute__((aligned(16))) char smem[lds_bytes(2 * A2_PLANE)];
  float* D1 = (float*)smem;
  float* D2 = (float*)smem;
  char* A2h = smem + D1_BYTES;
  char* A2l = A2h + A2_PLANE;

  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  const float* __restrict__ F = roi + (long long)r * P * DI;
  const float* __restrict__ Win = params + (long long)r * (2 * DI * DF);
  const float* __restrict__ Wout = Win + DI * DF;

  // ---- stage 1: wave -> one 32x32 tile of D1[64][64], K = 256 = 16 steps
  {
    const int tm = wave >> 1, tn = wave & 1;
    const int prow = tm * 32 + (lane & 31);
    const bool pv = prow < P;
    const float* ap = F + (long long)prow * DI + 8 * h;
    const float* bp = Win + ((long long)tn * 16 * 64 + lane) * 8;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    constexpr int GRP = 4;                                 // K steps whose operand fragments are in flight together
#pragma unroll
    for (int s0 = 0; s0 < 16; s0 += GRP) {
      uint4 a[GRP][2], b[GRP][2];
#pragma unroll
      for (int j = 0; j < GRP; ++j) {
        a[j][0] = pv ? *(const uint4*)(ap + (s0 + j) * 16) : make_uint4(0, 0, 0, 0);
        a[j][1] = pv ? *(const uint4*)(ap + (s0 + j) * 16 + 4) : make_uint4(0, 0, 0, 0);
        b[j][0] = *(const uint4*)(bp + (s0 + j) * 512);
        b[j][1] = *(const uint4*)(bp + (s0 + j) * 512 + 4);
      }
#pragma unroll
      for (int j = 0; j < GRP; ++j) {
        bf16x8 ah, al, bh, bl;
        split_f32x8(a[j][0], a[j][1], ah, al);
        split_f32x8(b[j][0], b[j][1], bh, bl);
        acc = x3_mfma(al, bh, acc);
        acc = x3_mfma(ah, bl, acc);
        acc = x3_mfma(ah, bh, acc);
      }
    }
    store_d1(D1, acc, tm, tn, lane);
  }
  // stage 2's weight fragments (wave -> columns [wave*64, +64) of Wout^T, K = 64 = 4 steps): issued now, consumed after the LayerNorm
  uint4 bf2[4][2][2];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float* q = Wout + ((long long)((wave * 2 + b) * 4 + s) * 64 + lane) * 8;
      bf2[s][b][0] = *(const uint4*)q;
      bf2[s][b][1] = *(const uint4*)(q + 4);
    }
  __syncthreads();
  // ---- LN over 64 features + ReLU, one wave per row, lane = feature; F1 split once into the fp16 planes (16-byte chunks XOR-swizzled
  // by row pair: a fragment read's 16 lanes hit 16 distinct bank groups)
  for (int row = wave; row < 64; row += 4) {
    const float v = ln64_relu(D1[row * D1_LD + lane], g_in[lane], b_in[lane]);
    uint32_t hh, ll;
    split_pair(v, 0.f, hh, ll);                            // (the packed pair's second half is not stored)
    const int chunk = lane >> 3, within = lane & 7;
    const int off = row * A2_ROWB + ((chunk ^ ((row >> 1) & 7)) << 4) + within * 2;
    *(uint16_t*)(A2h + off) = (uint16_t)(hh & 0xffffu);
    *(uint16_t*)(A2l + off) = (uint16_t)(ll & 0xffffu);
  }
  __syncthreads();  // D1 fully consumed, the planes complete
  // ---- stage 2: wave -> columns [wave*64, +64) of D2[64][256], 2x2 tiles, K = 64
  {
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ch = 2 * s + h;
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int row = a * 32 + (lane & 31);
        const int off = row * A2_ROWB + ((ch ^ ((row >> 1) & 7)) << 4);
        ah[a] = __builtin_bit_cast(bf16x8, *(const uint4*)(A2h + off));
        al[a] = __builtin_bit_cast(bf16x8, *(const uint4*)(A2l + off));
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) split_f32x8(bf2[s][b][0], bf2[s][b][1], bh[b], bl[b]);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = x3_mfma(al[a], bh[b], acc[a][b]);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = x3_mfma(ah[a], bl[b], acc[a][b]);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = x3_mfma(ah[a], bh[b], acc[a][b]);
    }
    __syncthreads();  // every wave is done reading the planes before D2 (which aliases them) is written
    store_d2(D2, acc, wave, lane);
  }
  __syncthreads();
  tail(D2, g_out, b_out, out + (long long)r * P * DI, wave, lane);
}

// ------------------------------------------------------------------------------------------------
// Per-clue score / box heads + delta2bbox (gaze_stqi_head.py:191-201, delta_xywh_bbox_coder.py:224-260),
// one wave per token; token r uses clue r % 3's weights.
template <typename T>
__global__ __launch_bounds__(256) void heads_kernel(const T* __restrict__ cls_feat, const T* __restrict__ reg_feat,
                                                    const float* __restrict__ wc, const float* __restrict__ bc,
                                                    const float* __restrict__ wr, const float* __restrict__ br,
                                                    const float* __restrict__ boxes_in, float* __restrict__ boxes_out,
                                                    float* __restrict__ cls_out, int R, float s0, float s1, float s2, float s3, float max_ratio) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= R) return;
  const int c = r % 3;
  float cf[4], rf[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cf[e] = Elem<T>::ld(cls_feat + (long long)r * 256 + lane * 4 + e);
    rf[e] = Elem<T>::ld(reg_feat + (long long)r * 256 + lane * 4 + e);
  }
  float dots[5];
  {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += cf[e] * wc[c * 256 + lane * 4 + e];
    dots[0] = wave_sum(s) + bc[c];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) s += rf[e] * wr[(c * 4 + k) * 256 + lane * 4 + e];
    dots[1 + k] = wave_sum(s) + br[c * 4 + k];
  }
  if (lane == 0) {
    cls_out[r] = dots[0];
    const float x1 = boxes_in[r * 4], y1 = boxes_in[r * 4 + 1], x2 = boxes_in[r * 4 + 2], y2 = boxes_in[r * 4 + 3];
    const float dx = dots[1] * s0, dy = dots[2] * s1;
    const float dw = fminf(fmaxf(dots[3] * s2, -max_ratio), max_ratio), dh = fminf(fmaxf(dots[4] * s3, -max_ratio), max_ratio);
    const float px = (x1 + x2) * 0.5f, py = (y1 + y2) * 0.5f, pw = x2 - x1, ph = y2 - y1;
    const float gx = px + pw * dx, gy = py + ph * dy, gw = pw * expf(dw), gh = ph * expf(dh);
    boxes_out[r * 4] = gx - gw * 0.5f; boxes_out[r * 4 + 1] = gy - gh * 0.5f;
    boxes_out[r * 4 + 2] = gx + gw * 0.5f; boxes_out[r * 4 + 3] = gy + gh * 0.5f;
  }
}

// ------------------------------------------------------------------------------------------------
// Gaze head tail (gaze_head.py:172-200): feats [6][N][256] (branch = k*3 + clue, k=0 gaze, 1 confidence)
// -> per-clue gaze / confidence 3-vectors, confidence-weighted fusion, L2 normalisation (no eps).
template <typename T>
__global__ __launch_bounds__(256) void gaze_tail_kernel(const T* __restrict__ feats, const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                        const float* __restrict__ w_fuse, const float* __restrict__ b_fuse,
                                                        float* __restrict__ gaze_out, int N,
                                                        const float* __restrict__ cls_logits, float* __restrict__ scores_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave;
  if (n >= N) return;
  // scores = sigmoid(last stage's logits) (multiclue_gaze_roi_head.py:351-352): the path's other tail, three values per frame
  if (scores_out && lane < 3) scores_out[n * 3 + lane] = 1.0f / (1.0f + expf(-cls_logits[n * 3 + lane]));
  float o[6][3];
#pragma unroll
  for (int br = 0; br < 6; ++br) {
    float f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = Elem<T>::ld(feats + ((long long)br * N + n) * 256 + lane * 4 + e);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s += f[e] * w_out[(br * 3 + k) * 256 + lane * 4 + e];
      o[br][k] = wave_sum(s) + b_out[br * 3 + k];
    }
  }
  if (lane == 0) {
    float cat[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k) cat[c * 3 + k] = o[3 + c][k] * o[c][k];  // confidence * gaze
    float fused[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float s = b_fuse[k];
#pragma unroll
      for (int j = 0; j < 9; ++j) s += w_fuse[k * 9 + j] * cat[j];
      fused[k] = s;
    }
    auto put = [&](int slot, const float* v) {
      const float nrm = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) gaze_out[((long long)slot * N + n) * 3 + k] = v[k] / nrm;
    };
    put(0, fused); put(1, o[0]); put(2, o[1]); put(3, o[2]);
  }
}

// ------------------------------------------------------------------------------------------------
// Query init (fixed_embedding_rpn_head.py:76-94): boxes = cxcywh->xyxy(E) * (w,h,w,h) per frame,
// object features = E_feat broadcast to every frame.  img_hw (device, [N][2]) may be null = (H, W).
// Indexed form (frame_of != NULL, mcg_decoder_forward_indexed): img_shape is a property of the FRAME, so window frame n reads
// img_hw[frame_of[n]] of a table with one row per pyramid row; an index outside [0, pyramid_frames) reads no table row and gives the
// frame NaN boxes (its RoIAlign output is NaN too, roi_align.hip).
template <typename T>
__global__ void init_queries_kernel(const float* __restrict__ init_boxes, const T* __restrict__ init_feats, const int* __restrict__ img_hw,
                                    const int32_t* __restrict__ frame_of, int pyramid_frames,
                                    int H, int W, float* __restrict__ boxes, T* __restrict__ obj, int N) {
  const long long total = (long long)N * 3 * 256;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(i % 256), q = (int)((i / 256) % 3);
    const int n = (int)(i / (3 * 256));
    obj[i] = init_feats[q * 256 + d];
    if (d < 4) {
      int r = n;
      bool bad_row = false;
      if (frame_of) {
        r = frame_of[n];
        bad_row = r < 0 || r >= pyramid_frames;
        if (bad_row) r = 0;
      }
      const float h = img_hw ? (float)img_hw[r * 2] : (float)H, w = img_hw ? (float)img_hw[r * 2 + 1] : (float)W;
      const float cx = init_boxes[q * 4], cy = init_boxes[q * 4 + 1], bw = init_boxes[q * 4 + 2], bh = init_boxes[q * 4 + 3];
      const float v = d == 0 ? (cx - 0.5f * bw) * w : d == 1 ? (cy - 0.5f * bh) * h : d == 2 ? (cx + 0.5f * bw) * w : (cy + 0.5f * bh) * h;
      boxes[((long long)n * 3 + q) * 4 + d] = bad_row ? __builtin_nanf("") : v;
    }
  }
}

// ================================================================================================
// Host orchestration of one decoder stage and of the gaze head.
static inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }
static inline size_t elem_bytes(mcg_dtype dt) { return MCG_ELEM_BYTES(dt); }   // activation storage (MCG_F16X3: f32)

// `dynamic_layer` (256 -> 32768 on M token rows, no residual) through the streaming kernels: pw_single.hpp's launch_pw_dyn (bf16 / fp16) or
// pw_single_x3.hpp's launch_pw_dyn_x3 (f16x3, whose weights carry wscale)
static PwSingleParams pw_dyn_params(const void* a, const void* wf, const float* bias, void* y, int M, float wscale) {
  PwSingleParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.a = a; pp.wf = wf; pp.bias = bias; pp.y = y; pp.M = M; pp.Ho = 1; pp.Wo = 1; pp.wscale = wscale;
  return pp;
}
static int launch_dyn_layer(hipStream_t s, const PwSingleParams& pp, mcg_dtype dt, int grid_cap) {
  const bool x3 = dt == MCG_F16X3;
  int failed;
  if (x3) failed = launch_pw_dyn_x3(s, pp, grid_cap);
  else failed = launch_pw_dyn(s, pp, dt, grid_cap);
  if (failed) { mcg_set_error("dynamic_layer (%s) launch failed", x3 ? "pw_single_x3" : "pw_single"); return MCG_ERR_HIP; }
  return MCG_OK;
}
// One chain step: dst = [ReLU] LN(src . W^T [+ bias] [+ res]) (chain.hpp)
static ChainStep chain_step(const void* W, const float* bias, const void* res, const float* g, const float* b, void* dst, int from_input, int relu) {
  ChainStep st;
  st.W = W; st.bias = bias; st.res = res; st.g = g; st.b = b; st.dst = dst; st.from_input = from_input; st.relu = relu;
  return st;
}

struct StageWs {
  char *qkv, *att, *t, *x1, *x2, *x3, *params, *feat2, *h, *c1, *clsf, *r1, *r2;
  float* partial;
  size_t total;
};
static const int kFcSlices = 16;
static StageWs stage_layout(mcg_dtype dt, int N, char* base) {
  const size_t es = elem_bytes(dt), R = (size_t)N * 3;
  StageWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
  w.qkv = take(R * 768 * es); w.att = take(R * 256 * es); w.t = take(R * 256 * es);
  w.x1 = take(R * 256 * es); w.x2 = take(R * 256 * es); w.x3 = take(R * 256 * es);
  w.params = take(R * 32768 * es); w.feat2 = take(R * 12544 * es);
  w.partial = (float*)take((size_t)(kFcSlices + 1) * R * 256 * 4);
  w.h = take(R * 2048 * es); w.c1 = take(R * 256 * es); w.clsf = take(R * 256 * es);
  w.r1 = take(R * 256 * es); w.r2 = take(R * 256 * es);
  w.total = off;
  return w;
}

extern "C" size_t mcg_stage_workspace_bytes(mcg_dtype dt, int num_frames) { return stage_layout(dt, num_frames, nullptr).total; }

int launch_roi_align(hipStream_t s, mcg_dtype dt, const void* const feats[4], const int feat_h[4], const int feat_w[4],
                     const int strides[4], int C, const float* boxes, int num_boxes, int boxes_per_frame, const int32_t* frame_of,
                     int pyramid_frames, void* out, int32_t* levels_out);

// What the C-ABI accepts as a batch's split into clips (igemm.hpp: ClipTable).  The table itself lives on the device and is not read here
// (no sync); the kernels clamp what it says (attn_block.hpp: clip_span).
int check_clips(const char* what, int N, const ClipTable& ct) {
  if (!ct.start) {
    MCG_CHECK_ARG(N > 0 && ct.max_len > 0 && N % ct.max_len == 0, "%s: num_frames=%d is not a multiple of clip_length=%d", what, N, ct.max_len);
    return MCG_OK;
  }
  MCG_CHECK_ARG(N > 0 && ct.num_clips > 0 && ct.max_len > 0, "%s: num_frames=%d, num_clips=%d, max_clip_length=%d must be positive", what, N,
                ct.num_clips, ct.max_len);
  // one clip holds max_clip_length frames, every other at least one and at most as many
  MCG_CHECK_ARG((long long)ct.num_clips - 1 + ct.max_len <= N && (long long)ct.num_clips * ct.max_len >= N,
                "%s: %d clips of at most %d frames (one of exactly that many) cannot hold num_frames=%d", what, ct.num_clips, ct.max_len, N);
  return MCG_OK;
}

extern "C" int mcg_stage_forward(mcg_stream s, mcg_dtype dt, const void* const W[MCG_SW_COUNT], const void* roi_feat,
                                 const void* obj_in, const float* boxes_in, int N, int clip_length, void* obj_out,
                                 float* boxes_out, float* cls_out, const float stds[4], void* ws, size_t ws_bytes, int flags) {
  return stage_forward_ctx((hipStream_t)s, dt, W, roi_feat, obj_in, boxes_in, N, ClipTable::uniform(N, clip_length), obj_out, boxes_out, cls_out, stds, ws,
                           ws_bytes, McgCtx::from_flags(0, flags));
}
extern "C" int mcg_stage_forward_ragged(mcg_stream s, mcg_dtype dt, const void* const W[MCG_SW_COUNT], const void* roi_feat,
                                        const void* obj_in, const float* boxes_in, int N, const int* clip_start, int num_clips,
                                        int max_clip_length, void* obj_out, float* boxes_out, float* cls_out, const float stds[4], void* ws,
                                        size_t ws_bytes, int flags) {
  MCG_CHECK_ARG(clip_start, "mcg_stage_forward_ragged: null clip_start (mcg_stage_forward is the equal-length path)");
  return stage_forward_ctx((hipStream_t)s, dt, W, roi_feat, obj_in, boxes_in, N, ClipTable{clip_start, num_clips, max_clip_length}, obj_out, boxes_out,
                           cls_out, stds, ws, ws_bytes, McgCtx::from_flags(0, flags));
}
// `dynamic_layer`'s streaming kernels as a stand-alone operator, through this unit's own launcher (launch_dyn_layer) at any M >= 1
extern "C" int mcg_pointwise_dyn(mcg_stream s, mcg_dtype dt, const void* a, const void* wf, const float* bias, void* y, int M, float wscale,
                                 int grid_cap) {
  MCG_CHECK_ARG(a && wf && bias && y, "mcg_pointwise_dyn: null pointer");
  MCG_CHECK_ARG(M > 0 && grid_cap >= 0, "mcg_pointwise_dyn: M must be positive and grid_cap >= 0 (M=%d grid_cap=%d)", M, grid_cap);
  const bool x3 = dt == MCG_F16X3;
  if (!(x3 || mcg_is16(dt)) || (long long)M * elem_bytes(dt) * 256 >= MCG_DMA_MAX_BYTES) {   // the A rows travel through a DMA descriptor
    mcg_set_error("mcg_pointwise_dyn: unsupported (dtype %d, M=%d): bf16 / fp16 / f16x3, M rows of 256 inputs below 2 GiB", (int)dt, M);
    return MCG_ERR_UNSUPPORTED;
  }
  return launch_dyn_layer((hipStream_t)s, pw_dyn_params(a, wf, bias, y, M, x3 ? wscale : 0.f), dt, grid_cap);
}

int stage_forward_ctx(hipStream_t s, mcg_dtype dt, const void* const W[MCG_SW_COUNT], const void* roi_feat, const void* obj_in,
                      const float* boxes_in, int N, const ClipTable& ct, void* obj_out, float* boxes_out, float* cls_out,
                      const float stds[4], void* ws, size_t ws_bytes, const McgCtx& ctx) {
  MCG_CHECK_ARG(W && roi_feat && obj_in && boxes_in && obj_out && boxes_out && cls_out && stds && ws, "mcg_stage_forward: null pointer");
  MCG_TRY(check_clips("mcg_stage_forward", N, ct));
  const int clip_length = ct.max_len;   // the longest clip (every clip, without a table)
  for (int i = 0; i < MCG_SW_COUNT; ++i) MCG_CHECK_ARG(W[i], "mcg_stage_forward: weight table entry %d is null", i);
  StageWs w = stage_layout(dt, N, (char*)ws);
  if (ws_bytes < w.total) { mcg_set_error("mcg_stage_forward: workspace too small (%zu < %zu)", ws_bytes, w.total); return MCG_ERR_WORKSPACE; }
  const int R = N * 3, B = ct.num_clips;
  const float* f32w[MCG_SW_COUNT];
  for (int i = 0; i < MCG_SW_COUNT; ++i) f32w[i] = (const float*)W[i];
  const bool bf = mcg_is16(dt);   // 2-byte storage (MCG_BF16 or MCG_F16: the same launch sequence, instantiated per number format)
  const size_t es = elem_bytes(dt);

  // --- spatial then temporal self-attention with SHARED weights and LayerNorm (gaze_stqi_head.py:148-166)
  const void* xin = obj_in;
  char* xout[2] = {w.x1, w.x2};
  const bool chain_attn = bf && ctx.chain;
  const bool chain_x3 = dt == MCG_F16X3 && ctx.chain;   // f16x3: the row-block chains in the split arithmetic (chain.hpp over OpsX3)
  // both passes as ONE launch, one clip per workgroup (bf16: attn_block.hpp; f16x3: attn_block_x3.hpp, round 6); bit-identical to the loop below
  const bool block_attn = (chain_attn || (chain_x3 && ctx.attn_block)) && attn_block_applicable(clip_length);
  if (block_attn) {
    AttnBlockParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.x = obj_in; ap.y = w.x2; ap.w_in = W[MCG_SW_IN_PROJ_WF]; ap.b_in = f32w[MCG_SW_IN_PROJ_B];
    ap.w_out = W[MCG_SW_OUT_PROJ_WF]; ap.b_out = f32w[MCG_SW_OUT_PROJ_B]; ap.g = f32w[MCG_SW_ATTN_LN_G]; ap.b = f32w[MCG_SW_ATTN_LN_B];
    ap.num_clips = B; ap.T = clip_length; ap.scale = 1.0f / sqrtf(32.f); ap.clip_start = ct.start; ap.num_frames = N;
    MCG_TRY(launch_attn_block(s, ap, dt));
  }
  for (int pass = 0; pass < 2 && !block_attn; ++pass) {
    MCG_TRY(launch_linear(s, dt, xin, 256, W[MCG_SW_IN_PROJ_W], f32w[MCG_SW_IN_PROJ_B], nullptr, 0, w.qkv, 768, R, 256, 768, 0, ctx));
    dispatch_elem(dt, [&](auto e) {   // pass 0: over a frame's 3 tokens; pass 1: over a clue's tokens across its clip
      using T = decltype(e);
      hipLaunchKernelGGL(attn_core_kernel<T>, dim3(pass == 0 ? N : B * 3), dim3(256), 0, s, (const T*)w.qkv, (T*)w.att, pass == 0 ? 3 : clip_length, pass,
                         clip_length, 1.0f / sqrtf(32.f), pass ? ct.start : nullptr, N);
    });
    MCG_CHECK_LAUNCH("attn_core");
    if (chain_attn || chain_x3) {  // out_proj + residual + LayerNorm as one launch
      ChainParams cp;
      memset(&cp, 0, sizeof(cp));
      cp.x = w.att; cp.M = R; cp.steps = 1;
      cp.st[0] = chain_step(W[MCG_SW_OUT_PROJ_WF], f32w[MCG_SW_OUT_PROJ_B], xin, f32w[MCG_SW_ATTN_LN_G], f32w[MCG_SW_ATTN_LN_B], xout[pass], 1, 0);
      MCG_TRY(launch_mlp_chain(s, cp, dt));
    } else {
      MCG_TRY(launch_linear(s, dt, w.att, 256, W[MCG_SW_OUT_PROJ_W], f32w[MCG_SW_OUT_PROJ_B], xin, 256, w.t, 256, R, 256, 256, 0, ctx));
      MCG_TRY(launch_ln(s, dt, ln_simple(w.t, f32w[MCG_SW_ATTN_LN_G], f32w[MCG_SW_ATTN_LN_B], 0, xout[pass], R, 256)));
    }
    xin = xout[pass];
  }
  // --- DynamicConv (transformer.py:1116-1164)
  // few rows, 32768 columns: 256-column weight slices resident in registers, tokens streamed (16-bit: pw_single.hpp; f16x3: split weights,
  // 256 slices of 128 columns, pw_single_x3.hpp); bit-identical to the generic kernel
  if (ctx.chain && ctx.tile < 0 && pw_dyn_applicable(R) && (chain_x3 ? (long long)R * 1024 < MCG_DMA_MAX_BYTES : bf && !ctx.staged)) {
    ProfRec* rec = prof_begin(ctx, s, chain_x3 ? 72 : 62, R, 32768, 256, 2.0 * R * 32768 * 256, (double)es * ((double)R * (256 + 32768) + 32768.0 * 256));
    const int rc = launch_dyn_layer(s, pw_dyn_params(w.x2, W[MCG_SW_DYN_WF], f32w[MCG_SW_DYN_B], w.params, R, 0.f), dt, 0);
    prof_end(rec, s);
    MCG_TRY(rc);
  } else {
    MCG_TRY(launch_linear(s, dt, w.x2, 256, W[MCG_SW_DYN_W], f32w[MCG_SW_DYN_B], nullptr, 0, w.params, 32768, R, 256, 32768, 0, ctx));
  }
  auto dynconv = [&](auto kernel, auto e) {   // a kernel and (e) the element type of its three tensors
    using T = decltype(e);
    hipLaunchKernelGGL(kernel, dim3(R), dim3(256), 0, s, (const T*)roi_feat, (const T*)w.params, f32w[MCG_SW_NORM_IN_G], f32w[MCG_SW_NORM_IN_B],
                       f32w[MCG_SW_NORM_OUT_G], f32w[MCG_SW_NORM_OUT_B], (T*)w.feat2);
  };
  if (dt == MCG_F16X3) dynconv(dynconv_x3_kernel, float{});
  else dispatch_elem(dt, [&](auto e) { dynconv(dynconv_kernel<decltype(e)>, e); });
  MCG_CHECK_LAUNCH("dynconv");
  int slabs = 1;
  MCG_TRY(launch_linear_splitk(s, dt, w.feat2, 12544, W[MCG_SW_FC_W], w.partial, R, 12544, 256, kFcSlices, &slabs, ctx));
  MCG_TRY(launch_ln(s, dt, ln_splitk(w.partial, slabs, f32w[MCG_SW_FC_B], f32w[MCG_SW_FC_LN_G], f32w[MCG_SW_FC_LN_B], 1, w.x2, f32w[MCG_SW_IIC_LN_G], f32w[MCG_SW_IIC_LN_B], w.x3, R)));
  // --- FFN (mmcv FFN with add_identity, gaze_stqi_head.py:179-180)
  MCG_TRY(launch_linear(s, dt, w.x3, 256, W[MCG_SW_FFN1_W], f32w[MCG_SW_FFN1_B], nullptr, 0, w.h, 2048, R, 256, 2048, 1, ctx));
  {  // 2048 -> 256 at M = R rows is only a couple of dozen output tiles: split K so the whole chip works on it; the
     // LayerNorm kernel sums the slabs, adds bias and the residual, and normalises (deterministic, no atomics)
    int ffn_slabs = 1;
    MCG_TRY(launch_linear_splitk(s, dt, w.h, 2048, W[MCG_SW_FFN2_W], w.partial, R, 2048, 256, 8, &ffn_slabs, ctx));
    MCG_TRY(launch_ln(s, dt, ln_splitk(w.partial, ffn_slabs, f32w[MCG_SW_FFN2_B], nullptr, nullptr, 0, w.x3, f32w[MCG_SW_FFN_LN_G], f32w[MCG_SW_FFN_LN_B], obj_out, R)));
  }
  // --- towers (gaze_stqi_head.py:185-188)
  const void* rin = obj_out;
  const bool chain = (bf || dt == MCG_F16X3) && ctx.chain;
  if (chain) {  // cls tower + 3-layer reg tower: eight launches as one (chain.hpp: bit-identical)
    ChainParams cp;
    memset(&cp, 0, sizeof(cp));
    cp.x = obj_out; cp.M = R; cp.steps = 4;
    cp.st[0] = chain_step(W[MCG_SW_CLS_FC_WF], nullptr, nullptr, f32w[MCG_SW_CLS_LN_G], f32w[MCG_SW_CLS_LN_B], w.clsf, 1, 1);
    for (int j = 0; j < 3; ++j)
      cp.st[1 + j] = chain_step((const char*)W[MCG_SW_REG_FC_WF] + (size_t)j * 65536 * es, nullptr, nullptr, f32w[MCG_SW_REG_LN_G] + j * 256,
                                f32w[MCG_SW_REG_LN_B] + j * 256, j == 2 ? w.r1 : nullptr, j == 0, 1);
    MCG_TRY(launch_mlp_chain(s, cp, dt));
    rin = w.r1;
  } else {
    MCG_TRY(launch_linear(s, dt, obj_out, 256, W[MCG_SW_CLS_FC_W], nullptr, nullptr, 0, w.c1, 256, R, 256, 256, 0, ctx));
    MCG_TRY(launch_ln(s, dt, ln_simple(w.c1, f32w[MCG_SW_CLS_LN_G], f32w[MCG_SW_CLS_LN_B], 1, w.clsf, R, 256)));
    char* rbuf[3] = {w.r1, w.r2, w.r1};
    for (int j = 0; j < 3; ++j) {
      MCG_TRY(launch_linear(s, dt, rin, 256, (const char*)W[MCG_SW_REG_FC_W] + (size_t)j * 65536 * es, nullptr, nullptr, 0, w.c1, 256, R, 256, 256, 0, ctx));
      MCG_TRY(launch_ln(s, dt, ln_simple(w.c1, f32w[MCG_SW_REG_LN_G] + j * 256, f32w[MCG_SW_REG_LN_B] + j * 256, 1, rbuf[j], R, 256)));
      rin = rbuf[j];
    }
  }
  const float max_ratio = 4.135166556742356f;  // |log(16/1000)|, delta_xywh_bbox_coder.py:236
  dispatch_elem(dt, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(heads_kernel<T>, dim3((R + 3) / 4), dim3(256), 0, s, (const T*)w.clsf, (const T*)rin, f32w[MCG_SW_HEAD_CLS_W], f32w[MCG_SW_HEAD_CLS_B],
                       f32w[MCG_SW_HEAD_REG_W], f32w[MCG_SW_HEAD_REG_B], boxes_in, boxes_out, cls_out, R, stds[0], stds[1], stds[2], stds[3], max_ratio);
  });
  MCG_CHECK_LAUNCH("heads");
  return MCG_OK;
}

extern "C" size_t mcg_gaze_head_workspace_bytes(mcg_dtype dt, int num_frames) {
  return 3 * al256((size_t)6 * num_frames * 256 * elem_bytes(dt));
}

extern "C" int mcg_gaze_head(mcg_stream s, mcg_dtype dt, const void* const W[MCG_GW_COUNT], const void* obj, int N,
                             float* gaze_out, void* ws, size_t ws_bytes) {
  return gaze_head_ctx((hipStream_t)s, dt, W, obj, N, gaze_out, ws, ws_bytes, McgCtx(), nullptr, nullptr);
}
int gaze_head_ctx(hipStream_t s, mcg_dtype dt, const void* const W[MCG_GW_COUNT], const void* obj, int N, float* gaze_out,
                  void* ws, size_t ws_bytes, const McgCtx& ctx, const float* cls_logits, float* scores_out) {
  MCG_CHECK_ARG(W && obj && gaze_out && ws && N > 0, "mcg_gaze_head: bad argument");
  for (int i = 0; i < MCG_GW_COUNT; ++i) MCG_CHECK_ARG(W[i], "mcg_gaze_head: weight table entry %d is null", i);
  if (ws_bytes < mcg_gaze_head_workspace_bytes(dt, N)) { mcg_set_error("mcg_gaze_head: workspace too small"); return MCG_ERR_WORKSPACE; }
  const size_t es = elem_bytes(dt);
  const size_t buf = al256((size_t)6 * N * 256 * es);
  char* raw = (char*)ws; char* h1 = raw + buf; char* h2 = h1 + buf;
  const char* fcw = (const char*)W[MCG_GW_FC_W];  // [6 branches = k*3+clue][2 layers][256][256]
  const float* lg = (const float*)W[MCG_GW_LN_G];
  const float* lb = (const float*)W[MCG_GW_LN_B];
  for (int layer = 0; layer < 2; ++layer) {
    {  // six branches (3 gaze MLPs, 3 confidence MLPs; branch = 3 k + clue) as ONE grouped launch: layer 0 reads token `clue` of
       // every frame for both k (x_g_period = 3), layer 1 its own branch's hidden rows
      IgemmParams p;
      memset(&p, 0, sizeof(p));
      p.M = N; p.Ho = 1; p.Wo = 1; p.H = 1; p.W = 1; p.Cin = 256; p.KH = 1; p.KW = 1; p.stride = 1; p.Cout = 256; p.nocheck = 1;
      p.splitk = 1; p.tiles_per_slice = 1 << 30;
      if (layer == 0) { p.x = obj; p.xs_n = 768; p.x_g = 256; p.x_g_period = 3; }
      else { p.x = h1; p.xs_n = 256; p.x_g = (long long)N * 256; }
      p.w = fcw + (size_t)layer * 65536 * es; p.w_g = 2 * 65536;
      p.y = raw; p.y_g = (long long)N * 256; p.y_row_stride = 256;
      MCG_TRY(launch_igemm(s, dt, p, 6, ctx));
    }
    LnParams q = ln_simple(raw, lg + layer * 256, lb + layer * 256, 1, layer == 0 ? h1 : h2, 6 * N, 256);
    q.rows_per_group = N; q.param_stride = 2 * 256;  // LN params are [6][2][256]
    MCG_TRY(launch_ln(s, dt, q));
  }
  dispatch_elem(dt, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(gaze_tail_kernel<T>, dim3((N + 3) / 4), dim3(256), 0, s, (const T*)h2, (const float*)W[MCG_GW_OUT_W], (const float*)W[MCG_GW_OUT_B],
                       (const float*)W[MCG_GW_FUSE_W], (const float*)W[MCG_GW_FUSE_B], gaze_out, N, cls_logits, scores_out);
  });
  MCG_CHECK_LAUNCH("gaze_tail");
  return MCG_OK;
}

// exported to engine.hip
int launch_init_queries(hipStream_t s, mcg_dtype dt, const float* init_boxes, const void* init_feats, const int* img_hw,
                        const int32_t* frame_of, int pyramid_frames, int H, int W, float* boxes, void* obj, int N) {
  const long long total = (long long)N * 3 * 256;
  const int grid = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  dispatch_elem(dt, [&](auto e) {
    using T = decltype(e);
    hipLaunchKernelGGL(init_queries_kernel<T>, dim3(grid), dim3(256), 0, s, init_boxes, (const T*)init_feats, img_hw, frame_of, pyramid_frames, H, W, boxes, (T*)obj, N);
  });
  MCG_CHECK_LAUNCH("init_queries");
  return MCG_OK;
}
