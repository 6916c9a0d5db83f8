// pw_single.hpp's persistent streaming kernel for the HBM-bound 1x1 convolutions, in the MCG_F16X3 arithmetic (f32 activations, weights
// as fp16 high / low fragments, three fp16 MFMAs per product): the P2 lateral 256 -> 256 with its nearest-upsampled top-down term
// (fpn.py:164-174) and layer3's conv3 256 -> 1024 + residual (resnet.py:283-298) of the f16x3 engine,
//
//     y = [relu]( A . W^T + b (+ res | + up(res)) )        A [M][256] f32, W [N][256]; per workgroup 128 output channels
//
// The generic x3 contraction kernel runs these at 3.3 - 3.5 TB/s of algorithmic bytes (one workgroup per CU; a 256 x 256 tile's
// 8 K-tiles sit between a cold prologue and a 512 KB epilogue).  Here a workgroup keeps its 128 x 256 slice of the weights -- high and
// low fragments, 128 VGPRs per wave -- in registers and walks 32-pixel tiles; the next tile's A rows and residual rows travel HBM -> LDS by
// `buffer_load ... lds` while the current tile is contracted and stored; two workgroups per CU; N / 128 workgroups on one XCD share
// an A tile through L2.  The A fragment (eight f32 from the swizzled LDS tile) is split in registers -- 24 VALU per three MFMAs, far
// under what the tile's bytes take.  K order, term order and f32 rounding points are the contraction kernel's.
#pragma once
#include "pw_single.hpp"

// A device list of 8 x 8-pixel blocks of the output map [frames][Ho][Wo] (Ho, Wo multiples of 8): block id = (frame * (Ho / 8) + block row)
// * (Wo / 8) + block column, the numbering of wino_x3w_blocks_kernel.  LISTED form of the kernel below
struct PwBlockList {
  const int* list;
  const int* count;         // entries of list (device)
  int bxn, bpf, nblk;       // blocks per row, per frame, in the map
};

// LISTED: the tiles are not 32 consecutive pixels of [0, M) but the two halves (4 rows x 8 pixels) of the *bl.count listed blocks: tile t =
// rows 4 (t & 1) .. + 3 of block bl.list[t >> 1], tile row r = its pixel (r >> 3, r & 7).  Everything a pixel's value depends on -- its A
// row, its residual row, the K order, the three-term order, the epilogue -- is the dense form's: which tile or workgroup computes a pixel
// does not enter its bits.  Pixels of unlisted blocks are neither read nor written.
template <int KS, int RES> using PwX3Layout = pwx::Layout<4, KS, 1, RES, 1>;   // one A tile: two would not leave room for two workgroups per CU
// rows of a listed tile whose first pixel is org (tile_origin below; -1: the tile has no rows), in a map Wo pixels wide
struct PwListedRows {
  int org, Wo;
  __device__ __forceinline__ int rows() const { return org >= 0 ? 32 : 0; }
  __device__ __forceinline__ long long base() const { return 0; }
  __device__ __forceinline__ int rel(int r) const { return org + (r >> 3) * Wo + (r & 7); }
  __device__ __forceinline__ int pixel(int r) const { return rel(r); }
  __device__ __forceinline__ bool has(int) const { return org >= 0; }
};
template <int KS, int RES, int NSPLIT, bool LISTED>
__device__ __forceinline__ void pw_single_x3_body(const PwSingleParams& p, const PwBlockList& bl) {
  using L = PwX3Layout<KS, RES>;
  constexpr int N = L::N, YBYTES = L::YBYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, px = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const pwx::Place at = pwx::place<NSPLIT>(p.many_slices);   // dynamic_layer: 256 slices
  const int nsp = at.nsp, walker = at.walker, nwalkers = at.nwalkers;
  int listed_tiles = 0;
  if constexpr (LISTED) {
    listed_tiles = 2 * __builtin_amdgcn_readfirstlane(*bl.count);
    if (walker >= listed_tiles) return;                // uniform per workgroup, before the weights are read
  }
  const float wsc = p.wscale > 0.f ? p.wscale : 1.f;   // exact power of two: the weights were packed pre-scaled by its inverse
  float4 breg[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) breg[q] = *(const float4*)(p.bias + nsp * N + wave * 32 + 8 * q + 4 * half);
  // weights of this wave's 32 channels, once per workgroup: split fragment-major [tile][K-step][high, low][lane][8] (packing.frag_major_split)
  uint4 w[KS][2];
  {
    const char* wb = (const char*)p.wf + ((size_t)(nsp * 4 + wave) * KS * 2 * 64 + lane) * 16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      w[ks][0] = *(const uint4*)(wb + (size_t)(2 * ks) * 1024);
      w[ks][1] = *(const uint4*)(wb + (size_t)(2 * ks + 1) * 1024);
    }
  }
  const u32x4 srd_a = make_srd(p.a), srd_r = make_srd(RES ? p.res : p.a);
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int ntiles = LISTED ? listed_tiles : (p.M + L::PX - 1) / L::PX;
  // LISTED: pixel index of a tile's first pixel (uniform; -1 for an id outside the map: nothing read, nothing written)
  auto tile_origin = [&](int tile) {
    const int blk = __builtin_amdgcn_readfirstlane(bl.list[tile >> 1]);
    if (blk < 0 || blk >= bl.nblk) return -1;
    const int f = blk / bl.bpf, rem = blk - f * bl.bpf, by = rem / bl.bxn, bx = rem - by * bl.bxn;
    return (f * p.Ho + by * 8 + (tile & 1) * 4) * p.Wo + bx * 8;
  };
  auto rows = [&](int tile, int org) {
    if constexpr (LISTED) return PwListedRows{org, p.Wo}; else return pwx::DenseRows{tile, p.M};
  };
  auto issue_a = [&](int tile, int org) { pwx::issue_a<L>(rows(tile, org), 0, srd_a, lds_base, wave, lane); };
  auto issue_res = [&](int tile, int buf, int org) { pwx::issue_res<L, RES, NSPLIT>(rows(tile, org), buf, p, nsp, srd_r, lds_base, wave, lane); };
  int org = 0, org_next = 0;
  if (walker < ntiles) {
    if constexpr (LISTED) org = tile_origin(walker);
    if (RES) issue_res(walker, 0, org);
    issue_a(walker, org);
  }
  int it = 0;
  for (int tile = walker; tile < ntiles; tile += nwalkers, ++it) {
    char* s_y = smem + (RES ? (it & 1) * YBYTES : 0);
    const char* s_a = smem + L::AOFF;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of the tile have landed (and its earlier stores left)
    __syncthreads();                                           // everyone's pieces landed; the other y buffer is free
    const bool more = tile + nwalkers < ntiles;
    if constexpr (LISTED) { if (more) org_next = tile_origin(tile + nwalkers); }
    if (more && RES) issue_res(tile + nwalkers, (it + 1) & 1, org_next);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 xh, xl;
      split_f32x8(*(const uint4*)(s_a + L::a_off(px, 4 * ks + 2 * half)), *(const uint4*)(s_a + L::a_off(px, 4 * ks + 2 * half + 1)), xh, xl);
      acc = x3_mfma(__builtin_bit_cast(bf16x8, w[ks][0]), xl, acc);   // activation low x weight high first: the contraction kernel's order
      acc = x3_mfma(__builtin_bit_cast(bf16x8, w[ks][1]), xh, acc);
      acc = x3_mfma(__builtin_bit_cast(bf16x8, w[ks][0]), xh, acc);
    }
    __syncthreads();                                           // the A tile has been consumed by every wave (and, RES == 0: the previous y tile is stored)
    if (more) issue_a(tile + nwalkers, org_next);              // single A tile: refilled under the epilogue
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c0 = wave * 32 + 8 * q + 4 * half;
      char* slot = s_y + L::y_off(px, c0 >> 2);
      float4 v = make_float4(acc[4 * q] * wsc + breg[q].x, acc[4 * q + 1] * wsc + breg[q].y, acc[4 * q + 2] * wsc + breg[q].z, acc[4 * q + 3] * wsc + breg[q].w);
      if (RES) {
        const float4 rr = *(const float4*)slot;
        v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w;
      }
      if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      *(float4*)slot = v;
    }
    __syncthreads();                                           // y tile complete
    pwx::store_tile<L, NSPLIT>(rows(tile, org), s_y, p.y, nsp, tid);
    if constexpr (LISTED) org = org_next;
  }
}
template <int KS, int RES, int NSPLIT>
__global__ __launch_bounds__(256, 2) void pw_single_x3_kernel(const PwSingleParams p) {
  pw_single_x3_body<KS, RES, NSPLIT, false>(p, PwBlockList{});
}
// The P2 lateral + nearest-upsampled top-down term over a device list of 8 x 8 blocks (deferred FPN P2 lateral): a fixed
// persistent grid, no host read of the count.  Bit for bit pw_single_x3_kernel<KS, 2, NSPLIT> on the listed pixels
template <int KS, int NSPLIT>
__global__ __launch_bounds__(256, 2) void pw_single_x3_blocks_kernel(const PwSingleParams p, const PwBlockList bl) {
  pw_single_x3_body<KS, 2, NSPLIT, true>(p, bl);
}

// (K, N) of the f16x3 trunk served here: 256 -> 256 (P2 lateral) and 256 -> 1024 (layer3's conv3)
// what launch_pw_single_x3 dispatches, for any M >= 1 whose operands fit the DMA descriptors (mcg_pointwise_stream) ...
static inline bool pw_single_x3_dispatched(int K, int N, long long M, long long res_rows) {
  return K == 256 && (N == 256 || N == 1024) && M * 4 * (K > N ? K : N) < MCG_DMA_MAX_BYTES && res_rows * 4 * N < MCG_DMA_MAX_BYTES;
}
// ... and where the engine takes it: from 64 Ki rows on
static inline bool pw_single_x3_applicable(int K, int N, int res_mode, long long M, long long res_rows) {
  return M >= 64 * 1024 && pw_single_x3_dispatched(K, N, M, res_rows);
}
template <int KS, int RES, int NSPLIT>
static inline int launch_pw_single_x3_t(hipStream_t s, const PwSingleParams& p, int cap = 0) {
  return pwx::launch<pw_single_x3_kernel<KS, RES, NSPLIT>, PwX3Layout<KS, RES>, NSPLIT>(s, (p.M + 31) / 32, p.many_slices, cap, p);
}
static inline int launch_pw_single_x3(hipStream_t s, const PwSingleParams& p, int N, int res_mode, int cap = 0) {
  return pwx::dispatch_res(res_mode, [&](auto rc) {
    constexpr int RES = decltype(rc)::value;
    return N == 256 ? launch_pw_single_x3_t<16, RES, 2>(s, p, cap) : launch_pw_single_x3_t<16, RES, 8>(s, p, cap);
  });
}

// The list form serves the P2 lateral (256 -> 256 + upsampled residual) on maps of whole 8 x 8 blocks whose operands fit the descriptors
static inline bool pw_single_x3_blocks_applicable(int K, int N, int Ho, int Wo, long long M, long long res_rows) {
  return K == 256 && N == 256 && Ho > 0 && Wo > 0 && Ho % 8 == 0 && Wo % 8 == 0 && M * 4 * K < MCG_DMA_MAX_BYTES && res_rows * 4 * N < MCG_DMA_MAX_BYTES;
}
// p as for launch_pw_single_x3(.., 256, 2) (M = frames * Ho * Wo); list / count: the blocks to compute; max_blocks = blocks of the map
static inline int launch_pw_single_x3_blocks(hipStream_t s, const PwSingleParams& p, const int* list, const int* count, int max_blocks, int cap = 0) {
  PwBlockList bl;
  bl.list = list; bl.count = count; bl.bxn = p.Wo / 8; bl.bpf = (p.Ho / 8) * (p.Wo / 8); bl.nblk = max_blocks;
  return pwx::launch<pw_single_x3_blocks_kernel<16, 2>, PwX3Layout<16, 2>, 2>(s, 2 * max_blocks, 0, cap, p, bl);   // two tiles per block
}

// DynamicConv's `dynamic_layer` for the f16x3 engine (transformer.py:1131-1134): y[M][32768] = x[M][256] . W^T + b on M = 1344 tokens,
// 176 MB of f32 output: 256 slices of 128 columns, each slice's split weights resident in the registers of two workgroups that share
// the token tiles (pw_single.hpp's launch_pw_dyn).  Bit-identical to the x3 contraction kernel.
static inline int launch_pw_dyn_x3(hipStream_t s, PwSingleParams p, int cap = 0) {
  p.many_slices = 1;
  return launch_pw_single_x3_t<16, 0, 256>(s, p, cap);
}
