/*
 * mcgaze_hip.h -- C-ABI of libmcgaze_hip.so, the MI355X (gfx950) implementation of the
 * MCGaze per-clip forward path.
 *
 * The reference has NO in-tree native code and no FFI for this path:
 * the arithmetic is reached through torch / mmcv Python calls.  Each entry point below
 * therefore cites the reference *Python* interface (file:line, relative to the upstream
 * repo root) whose work it replaces; INTEGRATION.md shows the ctypes binding a maintainer
 * of the reference would add at that call site.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless named host_*
 *   - every call enqueues work on the caller's HIP stream and returns without host sync
 *   - no allocation on the hot path: scratch comes from a caller-provided workspace
 *   - return value: MCG_OK or an MCG_ERR_* code; mcg_last_error() gives the message
 *   - activations are NHWC ("channels last"): [frame][y][x][channel]; dtype is MCG_F32
 *     (reference mode, f32 MFMA, exact f32 accumulate chains), MCG_F16X3 (parity-grade fast
 *     mode: f32 storage, split-fp16 x 3 MFMA contraction) or MCG_BF16 (throughput mode,
 *     bf16 storage and MFMA, f32 accumulate).  Bias / LayerNorm parameters / boxes are always f32.
 *   - conv / linear weights are "OHWI": [Cout][KH][KW][Cin] (K contiguous), BN folded in.
 */
#ifndef MCGAZE_HIP_H
#define MCGAZE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCG_ABI_VERSION 20

enum { MCG_OK = 0, MCG_ERR_ARG = 1, MCG_ERR_HIP = 2, MCG_ERR_UNSUPPORTED = 3, MCG_ERR_WORKSPACE = 4 };
/* MCG_F16X3: the parity-grade fast mode.  Activations, biases and every non-GEMM kernel are exactly those of MCG_F32 (4-byte
 * f32 storage); only the contraction differs: every conv / linear weight matrix is handed over SPLIT-PACKED -- per 8 consecutive
 * K elements a 16-byte chunk of fp16 HIGH parts followed by a 16-byte chunk of fp16 LOW parts (w = hi + lo, lo = f16(w - hi):
 * 22 significant bits for |w| >= 0.125; below that the low half is an fp16 SUBNORMAL with an absolute error of 2^-25, so a weight of
 * magnitude 1e-2 keeps ~18 bits and one of 1e-3 ~15 -- tests/test_gpu_kernels.py::test_f16x3_small_weights measures it; 4 bytes per
 * element like f32) -- the f32 activations are split the same way in registers (round toward zero,
 * x - hi exact), and each product runs as three fp16 MFMAs (lo.hi + hi.lo + hi.hi) with f32 accumulation.  Operands beyond
 * +-65504 saturate per half (the reference's activations are orders of magnitude below); parts below 6e-8 flush to zero.
 * The 22-bit figure is the TRUNK's: its matrices arrive pre-scaled by a power of two (mcg_conv_weights.wscale).  The DECODER's matrices
 * (mcg_stage_forward, mcg_gaze_head) are NOT pre-scaled and take no descale factor, and DynamicConv's two products split data on both sides
 * (theta = dynamic_layer's output, and the RoI features).  What a stage keeps, measured against float64 as a fraction of the output's
 * scale (tests/test_gpu_decoder.py): theta and RoI features of magnitude 1: 2e-6; RoI features x 2^-6: 2e-6, x 2^-10:
 * 7e-6 (the format's own figure: subnormal low halves are kept, not flushed); theta x 2^-6 / 2^-10 reached by scaling dynamic_layer's
 * weights: 2e-5 / 2.5e-4, of which 2e-6 / 2e-5 is the DynamicConv products' and the rest the unscaled packing of dynamic_layer.weight.
 * Measured: 1e-5 rad on (yaw, pitch) against the reference (north_star: 1e-3), within a factor 2 of the MCG_F32 engine. */
/* MCG_F16 (round 6, ABI 13): the 16-bit throughput mode in fp16 -- activations and weights stored as fp16 (11 significant bits instead of
 * bf16's 8; range +-65504), v_mfma_f32_32x32x16_f16, f32 accumulate, f32 LayerNorm / softmax / boxes.  Every layout, kernel and workspace size
 * is MCG_BF16's with "bf16" read as "fp16".  Outside north_star's 1e-3 rad on random-weight nets like MCG_BF16, but eight times closer. */
typedef enum { MCG_F32 = 0, MCG_BF16 = 1, MCG_F16X3 = 2, MCG_F16 = 3 } mcg_dtype;
/* bytes per activation element */
#define MCG_ELEM_BYTES(dt) (((dt) == MCG_BF16 || (dt) == MCG_F16) ? 2 : 4)
typedef void* mcg_stream; /* hipStream_t */

int mcg_abi_version(void);
/* First 16 hex digits of the sha256 over the library's kernel sources + this header at build time (csrc/Makefile); profiles/ files carry
 * it so that a reader can tell which build a measurement belongs to. */
const char* mcg_build_id(void);
const char* mcg_last_error(void);
/* Fills CU count, HBM bytes and the gcnArchName of the current HIP device. */
int mcg_device_info(int* cu_count, size_t* hbm_bytes, char* arch, int arch_len);

/* ---------------------------------------------------------------- layout helpers */
/* [N,C,H,W] f32 (the tensor the reference hands to backbone(img), multiclue_gaze.py:35)
 * -> NHWC dtype. */
int mcg_nchw_to_nhwc(mcg_stream s, mcg_dtype dt, const float* src, void* dst, int N, int C, int H, int W);
/* NHWC dtype -> [N,C,H,W] f32 (for handing a pyramid level back to NCHW consumers). */
int mcg_nhwc_to_nchw(mcg_stream s, mcg_dtype dt, const void* src, float* dst, int N, int C, int H, int W);

/* ---------------------------------------------------------------- conv / linear (implicit GEMM on MFMA)
 * Replaces, with BN folded and the activation fused:
 *   conv+BN+ReLU of Bottleneck.forward            mmdet/models/backbones/resnet.py:263-302
 *   downsample conv+BN                             mmdet/models/utils/res_layer.py:51-61
 *   FPN lateral / output convs + top-down add      mmdet/models/necks/fpn.py:157-180
 *   every nn.Linear of the decoder (H=W=1)         gaze_stqi_head.py:151-201, transformer.py:1131-1162
 */
enum { MCG_RES_NONE = 0, MCG_RES_ADD = 1, MCG_RES_UPSAMPLE_ADD = 2 };
/* Variant switches of the stand-alone operator entry points (an engine takes the same through mcg_engine_set_option).  The library
 * reads no environment variable; the default (0) is the product path.  Every variant computes the same function -- the bf16 ones
 * bit-identically (tests/test_gpu_kernels.py) -- they exist for A/B measurements and for those tests. */
enum {
  MCG_FLAG_STAGED_GEMM = 1,     /* bf16: register-staged contraction kernel instead of the LDS-DMA one */
  MCG_FLAG_NO_SPECIALISED = 2,  /* generic launch sequences instead of conv3x3_c64 / the fused stem / the decoder row-block chains */
  MCG_FLAG_NO_ATTN_BLOCK = 4    /* MCG_F16X3 mcg_stage_forward: the attention passes as in_proj / attention core / out_proj + LayerNorm launches instead of
                                 * ONE attention-block launch (attn_block_x3.hpp); same bits.  The block reads MCG_SW_IN_PROJ_WF (ABI 13) */
};
typedef struct {
  const void* x;        /* NHWC [N,H,W,Cin]                                         */
  const void* w;        /* OHWI [Cout,KH,KW,Cin]                                    */
  const float* bias;    /* [Cout] or NULL                                           */
  const void* residual; /* MCG_RES_ADD: [N,Ho,Wo,Cout]; UPSAMPLE_ADD: [N,Hr,Wr,Cout] */
  void* y;              /* NHWC [N,Ho,Wo,Cout]                                      */
  int N, H, W, Cin, Cout, KH, KW, stride, pad;
  int relu;             /* 1: y = max(y, 0) after bias and residual                 */
  int residual_mode;    /* MCG_RES_*                                                */
  int Hr, Wr;           /* residual spatial size for UPSAMPLE_ADD (nearest, F.interpolate size=) */
  /* Optional second input, K-concatenated after the first (needs KH=KW=1, stride 1, pad 0):
   *   y = [x | x2 sampled at stride2] . [w1 | w2]^T,  w = [Cout][Cin + Cin2].
   * Fuses a bottleneck's conv3 with its downsample conv (mmdet/models/utils/res_layer.py:51-61,
   * resnet.py:289-298): x2 = the block input, w2 = the BN-folded downsample weight. */
  const void* x2;       /* NHWC [N,H2,W2,Cin2] or NULL */
  int Cin2, stride2, H2, W2;
  int tile;             /* 0 = heuristic; else force this tile id of the contraction kernel (igemm.hip: 9, 11, 12, 14, 15; f16x3: 50, 51, 53) */
  int flags;            /* MCG_FLAG_* */
  float wscale;         /* MCG_F16X3 only, 0 = 1: y = wscale * (x . w) + bias ...  A power of two: the caller packs w PRE-SCALED by 1 / wscale so that
                           max |w| sits in (2^13, 2^14] and every fp16 low half down to 2^-17 of the largest weight is a NORMAL number (22 significant
                           bits for weights of any magnitude; unscaled, a weight of 1e-3 keeps 15).  mcgaze_amd/packing.py::pow2_prescale, then split_pack. */
} mcg_conv_desc;
int mcg_conv2d(mcg_stream s, mcg_dtype dt, const mcg_conv_desc* d);

/* The fused bottleneck tail as a stand-alone operator (MCG_F16X3 arithmetic; resnet.py:263-302): x = conv2's input
 * [frames][H][W][64] f32; src2 = the residual [frames][H][W][256] (nsrc = 1) or the downsample conv's input [frames][H][W][64]
 * (nsrc = 2); y [..][4 cm]; z [..][cn] (cn = 0: not written); cm = 64 or 128 mid channels (x then has cm channels, the residual 4 cm).
 * trace: NULL, or (measurement aid) a device buffer of 4096 uint64 that workgroup 0 fills with shader-clock stamps of its phases.
 * See* mcg_fused_block for wstream / bias. */
int mcg_bottleneck_x3(mcg_stream s, const float* x, const float* src2, const void* wstream, const float* bias, float* y, float* z,
                      int frames, int H, int W, int cm, int nsrc, int cn, void* trace);

/* 3x3 / stride 1 / pad 1 convolution as a ONE-DIMENSIONAL Winograd F(2,3) contraction along x (MCG_F16X3 arithmetic; wino_x3.hpp): the
 * FPN output convs (mmdet/models/necks/fpn.py:178-180) and a bottleneck's stride-1 conv2 (mmdet/models/backbones/resnet.py:263-302,
 * layer3 / layer4) with 6 instead of 9 matrix products per output.  x [frames][H][W][Cin] f32, y [frames][H][W][Cout] f32 = conv + bias
 * (+ ReLU); u = the weight in the kernel's transformed, split, fragment-major layout (mcgaze_amd/packing.py::wino_pack:
 * fp16 [Cout / 128][3 Cin / 16 K steps (16-channel slice major, y tap minor)][position 4][32-channel tile 4][high, low][lane 64][8],
 * mcg_conv3x3_wino_x3_weight_bytes(Cin, Cout) bytes = 16 / 9 of the f32 OHWI tensor).  Needs Cin % 32 == 0, Cout % 128 == 0,
 * 2 <= W <= 62 and a 128-pair tile's input window (its rows + halo rows, 16 channels) within 48 KiB -- every level of a 224 x 224
 * input; MCG_ERR_UNSUPPORTED otherwise (use mcg_conv2d).  The result differs from mcg_conv2d's in rounding only (both within 1e-6 of
 * scale of the f64 convolution); it does not depend on how the frames are batched.  tile: 0 = chosen by grid size; 1 / 2 / 3 force the
 * 128 x 128 / 64 x 64 / 32 x 64 (pairs x channels) workgroup tile of the 8-wave kernel, 4 the 128 x 128 tile with one wave per SIMD and the
 * weight fragments read straight from global memory (g = 2 only; what tile 0 picks for grids of >= 130 workgroups) -- all give the same bits.  wscale: as mcg_conv_desc.wscale (u packed
 * pre-scaled by its inverse; 0 = 1).  g: output pixels per transform group -- 2 = F(2,3) (the description above), 4 = F(4,3): six positions for
 * four outputs, 4.5 products per output; u = wino_pack(w, g=4) (24 / 9 of the OHWI tensor); additionally needs W % 4 == 0 and W >= 16; tile 1 = 64
 * groups x 128 channels, 2 / 3 = 32 x 64.  Its transform constants cost about 1.5 bits against the direct kernel (measured: tests). */
size_t mcg_conv3x3_wino_x3_weight_bytes(int Cin, int Cout, int g);
int mcg_conv3x3_wino_x3(mcg_stream s, const float* x, const void* u, const float* bias, float* y, int frames, int H, int W,
                        int Cin, int Cout, int relu, int tile, float wscale, int g);
/* ABI 20: the BLOCK tile of the same conv as a stand-alone operator (wino_x3w_blocks_kernel through launch_wino_x3_blocks, the deferred FPN
 * P2 conv of mcg_decoder_forward_deferred), for tests and measurements.  x, u (g = 2), bias, y, relu, wscale as above.  block_list (device)
 * holds *block_count (device) ids of 8 x 8-pixel output blocks, id = (frame * (H / 8) + block row) * (W / 8) + block column, in any order;
 * the pixels of the listed blocks are written with the bits mcg_conv3x3_wino_x3 writes there, every other pixel of y is left alone;
 * *block_count == 0 writes nothing.  max_blocks: the capacity of block_list (>= *block_count, >= 1); it sizes the persistent grid and is
 * not compared with the count on the device.  THE IDS MUST BE DISTINCT AND INSIDE [0, frames * (H / 8) * (W / 8)): the kernel does not guard
 * them (an id outside addresses outside x and y; a repeated id is two workgroups storing the same pixels), and the marking kernels below
 * produce no others.  H and W must be multiples of 8, Cin % 32 == 0, Cout % 128 == 0 and the operands within 2 GiB, W is not limited to 62:
 * MCG_ERR_UNSUPPORTED otherwise (the engine reaches multiples of 8 only: frames are multiples of 32).  grid_cap: 0 = the product's
 * persistent grid (one workgroup per unit of four blocks x 128 channels up to the compute units); else a host-side limit on the number of
 * workgroups, so that a short list walks several units per workgroup.  No kernel reads it. */
int mcg_conv3x3_wino_x3_blocks(mcg_stream s, const float* x, const void* u, const float* bias, float* y, int frames, int H, int W,
                               int Cin, int Cout, int relu, float wscale, const int* block_list, const int* block_count, int max_blocks,
                               int grid_cap);
/* Addition to ABI 20 (nothing that existed changes): the FRAME-LIST tile of the same conv as a stand-alone operator (wino_x3w_frames_kernel through launch_wino_x3_frames, the deferred
 * FPN P3 .. P5 convs of mcg_decoder_forward_deferred), for tests and measurements.  x, u (g = 2), bias, y as above; no ReLU, wscale = 1.
 * frame_list (device, capacity `frames`) holds *frame_count (device) frame indices in any order: every pixel of a listed frame is written
 * with the bits mcg_conv3x3_wino_x3 writes there, every other frame of y is left alone; *frame_count == 0 writes nothing.  The count is
 * clamped to `frames` and an index outside [0, frames) is skipped on the device; THE INDICES MUST BE DISTINCT (a repeated one is two
 * workgroups storing the same pixels; the marking kernel below produces no others).  Maps of 2 <= W <= 30 whose rows of one 128-pair tile
 * fit the window buffer, Cin % 32 == 0, Cout % 128 == 0, operands within 2 GiB: MCG_ERR_UNSUPPORTED otherwise.  grid_cap as above (units
 * are (list entry, 128-pair tile of the frame, 128 channels)). */
int mcg_conv3x3_wino_x3_frames(mcg_stream s, const float* x, const void* u, const float* bias, float* y, int frames, int H, int W,
                               int Cin, int Cout, const int* frame_list, const int* frame_count, int grid_cap);

/* The streaming 1x1 kernels as stand-alone operators (ABI 19; pw_single.hpp, pw_single_x3.hpp, pw_pair.hpp): the engine takes them from
 * 64 Ki rows on and the decoder from 256 tokens on; these entries run the same launchers at ANY M >= 1, for tests and measurements.  They
 * never fall back to another kernel: what the launchers do not dispatch is MCG_ERR_UNSUPPORTED.
 *
 * mcg_pointwise_stream: y [M][N] = [relu](a [M][K] . W^T + bias (+ res)), f32 accumulate, bias / residual / ReLU in f32, ONE store.
 *   dt MCG_BF16 / MCG_F16: a, res, y 16-bit; wf = the fragment-major copy of W [N][K] (packing.py::frag_major; mcg_conv_weights.wf);
 *     (K, N) = (512, 128) without a residual; (512, 256) with res_mode NONE or UPSAMPLE_ADD; (256, 256), (256, 1024), (128, 512) with
 *     every res_mode.
 *   dt MCG_F16X3: a, res, y f32; wf = frag_major_split of W pre-scaled by a power of two (packing.py::pow2_prescale), wscale its inverse
 *     (0 = 1, unscaled); (K, N) = (256, 256), (256, 1024) with every res_mode.
 *   res_mode MCG_RES_ADD: res [M][N].  MCG_RES_UPSAMPLE_ADD: M = frames * Ho * Wo and res [frames][Hr][Wr][N], gathered by
 *     F.interpolate(mode='nearest')'s rule, per axis src = min(floor(dst * f32(in / out)), in - 1).  MCG_RES_NONE: res NULL; Ho .. Wr unread.
 *   block_list / block_count (device; both or neither): MCG_F16X3, K = N = 256, UPSAMPLE_ADD, Ho and Wo multiples of 8 only -- the LIST form:
 *     block_list holds *block_count ids of 8 x 8-pixel blocks, id = (frame * (Ho / 8) + block row) * (Wo / 8) + block column, in any order;
 *     the pixels of the listed blocks are written, bit for bit as the dense form writes them, every other pixel of y is left alone and an id
 *     outside [0, M / 64) is skipped (nothing read, nothing written).  block_list must hold at least *block_count entries.
 *   Operands must fit the 2 GiB window of a DMA descriptor (M * max(K, N) and the residual's rows * N elements).
 * mcg_pointwise_dyn: DynamicConv's dynamic_layer, y [M][32768] = a [M][256] . W^T + bias, by the decoder's two forms (128 slices of 256
 *   columns for bf16 / fp16, 256 slices of 128 for MCG_F16X3); wf / wscale as above (the decoder itself hands MCG_SW_DYN_WF over unscaled).
 * mcg_pointwise_pair: y [M][256] = relu([a1 | a2] . W3^T + b3 (+ res)) rounded ONCE to the 16-bit type, and z [M][C2] = relu(y . W1^T + b1)
 *   from that ROUNDED y, rounded once (pw_pair.hpp; bf16 / fp16).  a1 [M][64]; a2 [M][64] with K2 = 64, or NULL with K2 = 0; res [M][256] or
 *   NULL, only without a second source; w3f = frag_major of W3 [256][64 + K2], w1f of W1 [C2][256]; C2 = 64 or 128.
 * grid_cap: 0 = the product's persistent grid.  Else a host-side limit on it, so that a small problem walks several tiles per workgroup:
 *   mcg_pointwise_stream: at most grid_cap groups of 8 * (N / channels per workgroup) workgroups (8 walkers per channel slice and group);
 *   mcg_pointwise_dyn: at most grid_cap walkers per channel slice; mcg_pointwise_pair: at most grid_cap workgroups.  No kernel reads it. */
int mcg_pointwise_stream(mcg_stream s, mcg_dtype dt, const void* a, const void* wf, const float* bias, const void* res, void* y,
                         int M, int K, int N, int relu, int res_mode, int Ho, int Wo, int Hr, int Wr, float wscale,
                         const int* block_list, const int* block_count, int grid_cap);
int mcg_pointwise_dyn(mcg_stream s, mcg_dtype dt, const void* a, const void* wf, const float* bias, void* y, int M, float wscale, int grid_cap);
int mcg_pointwise_pair(mcg_stream s, mcg_dtype dt, const void* a1, const void* a2, const void* res, const void* w3f, const float* b3,
                       void* y, const void* w1f, const float* b1, void* z, int M, int K2, int C2, int grid_cap);

/* Stem: conv 7x7 s2 p3 (3->64) + BN + ReLU then max-pool 3x3 s2 p1 (resnet.py:636-639).
 * img is the reference's NCHW f32 frame tensor.  w_stem is the packed stem weight
 * [64][7][8][4] (kw and channel zero-padded, BN folded).  ws >= mcg_stem_workspace_bytes. */
size_t mcg_stem_workspace_bytes(mcg_dtype dt, int N, int H, int W);
int mcg_stem_forward(mcg_stream s, mcg_dtype dt, const float* img, const void* w_stem, const float* bias,
                     void* y, int N, int H, int W, void* ws, size_t ws_bytes, int flags);

/* ---------------------------------------------------------------- RoIAlign, all levels, one launch
 * Replaces SingleRoIExtractor.forward (roi_extractors/single_level_roi_extractor.py:57-115:
 * map_roi_levels + per-level mmcv.ops.RoIAlign(7, 1/stride, sampling_ratio=2, 'avg', aligned=True))
 * and bbox2roi (mmdet/core/bbox/transforms.py:75-94).
 * boxes [N*P,4] f32 xyxy in image pixels, P boxes per frame, frame index = row / P.
 * out is [N*P][49][C] dtype (position-major, channel-minor: the layout DynamicConv consumes,
 * transformer.py:1131-1133).  levels_out (optional) receives the chosen pyramid level per box. */
int mcg_roi_align(mcg_stream s, mcg_dtype dt, const void* const feats[4], const int feat_h[4], const int feat_w[4],
                  const int strides[4], int C, const float* boxes, int num_boxes, int boxes_per_frame,
                  void* out, int32_t* levels_out);
/* ABI 14: mcg_roi_align over window frames gathered from a pyramid STORE -- box row r reads pyramid row frame_of[r / boxes_per_frame]
 * of feats [pyramid_frames][h][w][C] (frame_of: DEVICE int32 [num_boxes / boxes_per_frame]).  Replaces the same call site as
 * mcg_roi_align, for a caller that holds each distinct video frame once although windows overlap (the reference's harness runs the whole
 * model per window: tools/test_gaze360_gaze.py:72-111).  An entry outside [0, pyramid_frames) reads nothing (the address is clamped)
 * and that box's output is NaN: a guard for callers, not a feature.  Bits equal mcg_roi_align's on the gathered rows. */
int mcg_roi_align_indexed(mcg_stream s, mcg_dtype dt, const void* const feats[4], const int feat_h[4], const int feat_w[4],
                          const int strides[4], int C, const float* boxes, int num_boxes, int boxes_per_frame,
                          const int32_t* frame_of, int pyramid_frames, void* out, int32_t* levels_out);
/* ABI 20: roi_mark_kernel as a stand-alone operator (launch_roi_mark, the first step of a deferred decoder stage), for tests and
 * measurements: which 8 x 8-pixel blocks of ONE pyramid level mcg_roi_align reads for these boxes.  boxes as above; level, H, W, stride: the
 * deferred level (the engine: 0, P2's size, 4), at most 64 blocks per axis.  state [frames * by_n * bx_n] (by_n = ceil(H / 8), bx_n =
 * ceil(W / 8), frames = ceil(num_boxes / boxes_per_frame)), list of the same capacity and count (one int) are DEVICE buffers of the caller.
 * A box that map_roi_levels routes to another level does nothing.  Otherwise the box's blocks are {lo >> 3, hi >> 3 of every valid y sample}
 * x {the same of every valid x sample} of frame = box row / boxes_per_frame, with lo, hi and valid as mcg_roi_align computes them
 * (roi_sample.hpp: a tap of weight zero counts, a box without a valid sample on either axis has none); block id = (frame * by_n + block row)
 * * bx_n + block column.  A block whose state is 0 gets state 1 and is appended, list[(*count)++] = id; a block whose state is already
 * non-zero is not listed again -- so no id appears twice, within a call or over calls that share state.  The order of the list is
 * unspecified.  *count is added to, not reset: the caller zeroes state and count. */
int mcg_roi_mark_blocks(mcg_stream s, const float* boxes, int num_boxes, int boxes_per_frame, int level, int H, int W, int stride,
                        int* state, int* list, int* count);
/* Addition to ABI 20: the frame marking of the same kernel alone (levels deferred by whole frames, engine option fpn_levels_deferred), for tests and
 * measurements.  num_boxes is a multiple of boxes_per_frame; state [frames], list [frames] and count (one int) are DEVICE buffers of the
 * caller.  A box that map_roi_levels routes to `level` (0 .. 3) lists its frame = box row / boxes_per_frame: a frame whose state is 0 gets
 * state 1 and is appended, list[(*count)++] = frame; a frame whose state is non-zero is not listed again.  Order unspecified; *count is
 * added to, not reset. */
int mcg_roi_mark_frames(mcg_stream s, const float* boxes, int num_boxes, int boxes_per_frame, int level, int* state, int* list, int* count);

/* ---------------------------------------------------------------- decoder stage / gaze head / whole path
 * Weight tables are arrays of device pointers indexed by the enums below.  Matrices are
 * dtype, [out][in] row-major exactly as in the checkpoint unless noted; vectors are f32.
 */
enum {
  MCG_SW_IN_PROJ_W = 0, MCG_SW_IN_PROJ_B, MCG_SW_OUT_PROJ_W, MCG_SW_OUT_PROJ_B, MCG_SW_ATTN_LN_G, MCG_SW_ATTN_LN_B,
  MCG_SW_DYN_W,      /* dynamic_layer.weight rows permuted (mcgaze_amd/packing.py::dyn_permutation(epc = elements per 16-byte chunk)) so that a token's
                        param_in^T [64][256] and param_out^T [256][64] come out in the MFMA-fragment-major order dynconv_kernel reads */
  MCG_SW_DYN_B,      /* permuted the same way, f32 */
  MCG_SW_NORM_IN_G, MCG_SW_NORM_IN_B, MCG_SW_NORM_OUT_G, MCG_SW_NORM_OUT_B,
  MCG_SW_FC_W, MCG_SW_FC_B, MCG_SW_FC_LN_G, MCG_SW_FC_LN_B, MCG_SW_IIC_LN_G, MCG_SW_IIC_LN_B,
  MCG_SW_FFN1_W, MCG_SW_FFN1_B, MCG_SW_FFN2_W, MCG_SW_FFN2_B, MCG_SW_FFN_LN_G, MCG_SW_FFN_LN_B,
  MCG_SW_CLS_FC_W, MCG_SW_CLS_LN_G, MCG_SW_CLS_LN_B,
  MCG_SW_REG_FC_W,   /* [3][256][256] */
  MCG_SW_REG_LN_G,   /* [3][256] */
  MCG_SW_REG_LN_B,
  MCG_SW_HEAD_CLS_W, /* f32 [3 clues][256]      (face, eyes, head)_fc_cls.weight */
  MCG_SW_HEAD_CLS_B, /* f32 [3]                                                  */
  MCG_SW_HEAD_REG_W, /* f32 [3 clues][4][256]   (face, eyes, head)_fc_reg.weight */
  MCG_SW_HEAD_REG_B, /* f32 [3][4]                                               */
  /* MFMA-fragment-major copies of [32 t][256] matrices for the fused row-block chain / attention block.
   *   MCG_BF16:  bf16 WF[t][ks][lane][e] = W[32 t + (lane & 31)][16 ks + 8 (lane >> 5) + e], t < rows / 32, ks < 16, lane < 64, e < 8 --
   *              one wave-wide 16-byte load per (column tile, K-step) is then 1 KiB contiguous.
   *   MCG_F16X3: REQUIRED for OUT_PROJ / CLS_FC / REG_FC / DYN and -- since ABI 13 -- IN_PROJ (the default stage path -- chain_x3.hpp,
   *              attn_block_x3.hpp, pw_single_x3.hpp -- reads them;
   *              passing the row-major split-packed pointer again gives WRONG results, not an error): the SPLIT fragment-major form
   *              fp16 WF[t][ks][hl][lane][e], hl = 0 the fp16 high parts, hl = 1 the low parts of the same elements as above
   *              (mcgaze_amd/packing.py::frag_major_split; 4 bytes per weight).  IN_PROJ_WF ([768][256], t < 24) is read by the attention block whenever
   *              3 x clip_length <= 32 (ABI <= 12: not read); flags = MCG_FLAG_NO_ATTN_BLOCK keeps the launch sequence that does not need it.
   *              mcg_stage_forward(flags = MCG_FLAG_NO_SPECIALISED) runs the generic launch sequence, which reads only the row-major
   *              split-packed matrices.
   *   MCG_F32:   ignored (may be given the row-major pointers again). */
  MCG_SW_OUT_PROJ_WF, MCG_SW_CLS_FC_WF,
  MCG_SW_REG_FC_WF,  /* [3] x fragment-major */
  MCG_SW_IN_PROJ_WF, /* in_proj_weight [768][256] fragment-major (t < 24 column tiles) for the fused attention block (attn_block.hpp) */
  MCG_SW_DYN_WF,     /* dynamic_layer.weight [32768][256] (rows permuted like the row-major entry) fragment-major, t < 1024 (pw_single.hpp) */
  MCG_SW_COUNT
};
enum {
  MCG_GW_FC_W = 0,   /* [6 branches][2 layers][256][256]; branch = 3*k + clue, k = 0 gaze MLP, 1 confidence MLP */
  MCG_GW_LN_G,       /* f32 [6][2][256] */
  MCG_GW_LN_B,
  MCG_GW_OUT_W,      /* f32 [6][3][256]: fc_{clue} (gaze) / fc_{clue}_confidence */
  MCG_GW_OUT_B,      /* f32 [6][3] */
  MCG_GW_FUSE_W,     /* f32 [3][9]  fc_gaze */
  MCG_GW_FUSE_B,     /* f32 [3] */
  MCG_GW_COUNT
};

/* One GazeSTQIHead.forward + refine_bboxes (gaze_stqi_head.py:119-202, bbox_head.py:380-457,
 * delta_xywh_bbox_coder.py:224-260 with stds (.5,.5,1,1), clip_border=False).
 *   roi_feat [R][49][256] dtype (from mcg_roi_align), obj_in/obj_out [N][3][256] dtype,
 *   boxes_in/boxes_out [N][3][4] f32, cls_out [N][3] f32 (logits, pre-sigmoid).
 *   N = num_clips * clip_length frames; temporal attention spans clip_length frames. */
size_t mcg_stage_workspace_bytes(mcg_dtype dt, int num_frames);
int mcg_stage_forward(mcg_stream s, mcg_dtype dt, const void* const weights[MCG_SW_COUNT], const void* roi_feat,
                      const void* obj_in, const float* boxes_in, int num_frames, int clip_length,
                      void* obj_out, float* boxes_out, float* cls_out, const float bbox_stds[4],
                      void* ws, size_t ws_bytes, int flags);
/* ABI 16: clips of DIFFERENT lengths in one call (the mcg_*_ragged entry points).  The reference fixes one clip length per call
 * (multiclue_gaze.py:77-78, :119: num_clips = frames / clip_length), but only ONE step of the path looks at where clips begin and end: the
 * temporal attention pass of a stage (gaze_stqi_head.py:156-166, which regroups the tokens as [clip x clue][frames of the clip]); everything
 * else is per frame or per token.  So a ragged call takes, in place of clip_length,
 *   clip_start       DEVICE int32 [num_clips + 1]: frame indices, clip_start[0] = 0, strictly increasing, clip_start[num_clips] =
 *                    num_frames; clip b holds frames [clip_start[b], clip_start[b + 1])
 *   num_clips        HOST integer
 *   max_clip_length  HOST integer: the length of the longest clip (exactly: it selects the attention path and bounds what a kernel reads)
 * The two integers are host values so that the call reads nothing back: no sync, graph-capturable like every other call.  Every clip's
 * results are bit for bit those of a call that holds this clip alone; they depend neither on its place in the batch nor on its
 * neighbours' lengths (MCG_F16: as long as the SAME attention path runs -- the fused block when max_clip_length <= 10, else the launch
 * sequence; the two differ by one fp16 ulp there, tests/test_gpu_kernels.py::test_mlp_chain_matches_unfused_bitwise -- so a short clip
 * batched with one longer than 10 frames may differ in the last bit from the same clip run alone.  MCG_F32 / MCG_F16X3 / MCG_BF16: the two
 * paths give the same bits).  The existing entry points are the clip_start = NULL case of the same code.
 * The table is not read on the host.  Guard (like frame_of's): an entry outside [0, num_frames], a span that is not increasing or one
 * longer than max_clip_length is clamped -- no kernel reads or writes outside rows [0, 3 num_frames) -- and that clip's attention output
 * is NaN: for callers' bugs, not a feature; mcgaze_amd/engine.py::check_clip_lengths builds a valid table from a list of lengths. */
int mcg_stage_forward_ragged(mcg_stream s, mcg_dtype dt, const void* const weights[MCG_SW_COUNT], const void* roi_feat,
                             const void* obj_in, const float* boxes_in, int num_frames, const int* clip_start, int num_clips,
                             int max_clip_length, void* obj_out, float* boxes_out, float* cls_out, const float bbox_stds[4],
                             void* ws, size_t ws_bytes, int flags);

/* GazeHead.forward (mask_heads/gaze_head.py:138-202): obj [N][3][256] dtype -> gaze [4][N][3] f32
 * unit vectors in the order fused, face, eyes, head. */
size_t mcg_gaze_head_workspace_bytes(mcg_dtype dt, int num_frames);
int mcg_gaze_head(mcg_stream s, mcg_dtype dt, const void* const weights[MCG_GW_COUNT], const void* obj,
                  int num_frames, float* gaze_out, void* ws, size_t ws_bytes);

/* ---------------------------------------------------------------- engine: the whole path in one call
 * Replaces MultiClueGaze.simple_test (mmdet/models/detectors/multiclue_gaze.py:105-131) with
 * the batched semantics of forward_train (:77-78): N = num_clips*clip_length frames.
 */
typedef struct {
  const void* w;      /* OHWI dtype, BN folded */
  const float* bias;  /* f32 [Cout] */
  int cin, cout, k, stride, pad;
  const void* wf;     /* optional second copy of w for a specialised kernel; NULL -> the contraction kernel on w (always correct):
                         MCG_BF16, 1x1 convs: MFMA-fragment-major bf16 [cout/32][cin/16][64 lanes][8],
                           wf[t][ks][lane][e] = w[32 t + (lane & 31)][16 ks + 8 (lane >> 5) + e] (pw_pair.hpp, pw_single.hpp);
                         MCG_F16X3, 1x1 convs 256 -> 256 / 256 -> 1024: the SPLIT fragment-major form fp16 [cout/32][cin/16][high, low][64][8]
                           (packing.py::frag_major_split; pw_single_x3.hpp).  A row-major pointer here gives wrong results;
                         MCG_F16X3, 3x3 / stride 1 / pad 1 convs with cin % 32 == 0, cout % 128 == 0: the Winograd F(2,3) operand of
                           mcg_conv3x3_wino_x3 (packing.py::wino_pack; wino_x3.hpp);
                         MCG_F32: ignored */
  float wscale;       /* MCG_F16X3: the power of two w AND wf were pre-scaled by the inverse of (mcg_conv_desc.wscale); 0 = 1 = unscaled */
  const void* wf4;    /* optional, MCG_F16X3, 3x3 / stride 1 / pad 1 convs: the F(4,3) operand of mcg_conv3x3_wino_x3 (wino_pack(w, g=4), same pre-scale);
                         used on maps whose width is a multiple of 4 and at least 16, wf (F(2,3)) elsewhere; NULL -> wf only */
} mcg_conv_weights;

/* A fused bottleneck tail of the MCG_F16X3 engine (bneck_x3.hpp): conv2 (3x3) -> conv3 (1x1, + downsample as a second K source or
 * + residual) -> the NEXT block's conv1 (1x1) in one kernel; the 64-channel intermediates never leave the CU and the block output is
 * read from HBM once less.  wstream: the three weight matrices as 16 KiB MFMA-fragment-major slabs of fp16 high / low parts in
 * the order the kernel consumes them (mcgaze_amd/packing.py::bneck_stream gives the exact layout; bytes =
 * 16384 * (9 (cm / 64)^2 + (cm / 16) (cm / 64 + nsrc - 1 + cn / 64))).  bias: f32 [cm | c | cn | 4]: the three bias vectors, then the
 * power-of-two descale factors of conv2's, conv3's (+ downsample) and the next conv1's matrix (each packed pre-scaled by the inverse,
 * see mcg_conv_desc.wscale) and one pad float.  Applies when cm = 64, c = 256, cn in
 * {0, 64, 128} (layer1 of a ResNet-50) or cm = 128, c = 512, cn in {0, 128}, nsrc = 1 (layer2's identity blocks); other layers keep
 * the layer-granular launches. */
typedef struct {
  const void* wstream;
  const float* bias;
  int conv2_index;                  /* index into convs[] of the conv2 this unit replaces (its conv3 [+ downsample] follow) */
  int cm, c, cn;                    /* mid channels, output channels, output channels of the next block's conv1 (0 = none) */
  int nsrc;                         /* 1: identity block (residual = block input); 2: first block (conv3 | downsample, no residual) */
} mcg_fused_block;

typedef struct {
  int blocks[4];                    /* bottlenecks per layer, (3,4,6,3) for R-50 */
  mcg_conv_weights stem;            /* packed stem, see mcg_stem_forward */
  const mcg_conv_weights* convs;    /* host array, execution order: per block conv1, conv2, conv3[, downsample] */
  int num_convs;
  mcg_conv_weights lateral[4];
  mcg_conv_weights fpn_out[4];
  mcg_conv_weights c3_ds[4];        /* per layer: first block's conv3 and downsample fused ([Cout][planes + inplanes], bias summed); w = NULL -> unfused */
  const float* init_boxes;          /* f32 [3][4] normalised cxcywh (rpn_head.init_proposal_bboxes.weight) */
  const void* init_feats;           /* dtype [3][256] */
  int num_stages;
  const void* const* stage_weights; /* host array [num_stages][MCG_SW_COUNT] of device pointers */
  const void* const* gaze_weights;  /* host array [MCG_GW_COUNT]: the LAST stage's gaze head */
  float bbox_stds[4];
  const mcg_fused_block* fused;     /* optional (MCG_F16X3): host array of fused bottleneck tails, or NULL */
  int num_fused;
} mcg_model_weights;

typedef struct mcg_engine mcg_engine;
/* Threading and streams (what a host that drives the library from several threads may rely on)
 *   - The stand-alone operators (mcg_conv2d ... mcg_gaze_head, mcg_preprocess_frames, mcg_preprocess_head_crops) keep no state: any thread, any stream.
 *     mcg_last_error() is thread-local.
 *   - An ENGINE runs ONE forward at a time.  mcg_backbone_fpn_forward / mcg_clip_forward / mcg_bench_backbone_forward /
 *     mcg_engine_set_option / mcg_engine_profile_* take the engine's mutex for the duration of the ENQUEUE (they never wait for
 *     the GPU): two host threads calling into the same engine are serialised silently, in lock order, and both calls are
 *     correct -- but they share the engine's fork / join events and the caller-provided workspace, so they must not pass the
 *     same workspace unless they also enqueue on the same stream.  mcg_decoder_forward(_indexed) touches no engine state beyond the
 *     (immutable) weight tables and does not take the mutex: it may run on another thread / stream beside the trunk of the
 *     next batch (mcgaze_amd/engine.py: PipelinedRunner) as long as its workspace and pyramid are its own.
 *     For concurrent forwards on one device use one engine per thread (weights may be shared: the engine copies only the
 *     tables); tests/test_gpu_forward.py::test_two_threads_two_engines_one_device asserts bit-identical results.
 *   - Streams: every call is ordered on the caller's stream `s` -- work queued on `s` before the call is visible to it, work
 *     queued on `s` after the call sees its results.  With trunk_streams > 1 the trunk forks frame ranges onto side streams
 *     and joins them back into `s` with events before returning, so this still holds; the side streams come from a
 *     per-DEVICE pool of 8 non-blocking streams created once per process and shared by every engine on that device (streams
 *     created later in a process's life serialise against earlier ones on this runtime), chosen per caller stream by a
 *     one-off concurrency probe (a ~1 ms host wait on the first call that sees a new caller stream; never on the hot path
 *     afterwards).  Two engines driven concurrently on one device therefore share side streams: results are unaffected,
 *     their trunks' frame ranges may serialise against each other.
 *   - The library reads no environment variable and never synchronises the device on the hot path; mcg_engine_profile_stop,
 *     mcg_engine_range_audit (debug) and the first-call probe are the only host waits. */
/* The engine copies the weight TABLES (not the weights); device buffers stay caller-owned. */
int mcg_engine_create(mcg_engine** out, const mcg_model_weights* w, mcg_dtype dt);
void mcg_engine_destroy(mcg_engine* e);
/* Per-engine options (integers; unknown names are an error).  An engine is driven by one host thread at a time.
 *   trunk_streams     1..4  concurrent frame ranges of the trunk (default 2: one range's kernel tails overlap the other's kernels)
 *   max_range_frames  >= 0  lowers the frames-per-range cap (0 = what fits the 2 GiB descriptor window)
 *   tile              forces a contraction tile id (0 = heuristic), see mcg_conv_desc.tile
 *   staged_gemm, conv3x3_c64, stem_fused, decoder_chain   0/1 kernel-variant switches (defaults 0, 1, 1, 1)
 *   decoder_attn_block 0/1 f16x3: both attention passes of a decoder stage (in_proj, attention core, out_proj + residual + LayerNorm, twice) as ONE
 *                     launch per stage, one clip per workgroup (attn_block_x3.hpp; calls whose longest clip has at most 10 frames); bit-identical to the six launches (default 1)
 *   pointwise_pair    0/1 conv3 (+ residual) of a block and conv1 of the next as one kernel in layer1 (bf16; default 1)
 *   pointwise_stream  0/1 HBM-bound 1x1 convs (layer2, layer3 conv3, P2 / P3 laterals) by the persistent register-resident-weight
 *                     kernel pw_single.hpp (bf16; default 1)
 *   bottleneck_fused  0/1 the fused bottleneck tails handed over in mcg_model_weights.fused (f16x3; default 1)
 *   bottleneck_blocked 0/1 a tensor that only travels from one fused tail to the next (the residual inside layer1 / layer2) is kept in that
 *                     kernel's blocked layout (whole-line stores and loads) instead of [M][C]; internal workspace only, results bit-identical (default 1)
 *   winograd          0/1/2 stride-1 3x3 convs that carry a Winograd copy by wino_x3.hpp (f16x3): 0 off, 1 (default) F(2,3) (mcg_conv_weights.wf), 2 F(4,3)
 *                     on maps whose shape allows it (mcg_conv_weights.wf4; 6 % faster there, four times the operator error), F(2,3) elsewhere
 *   wino_tile         -1..3 tile of the F(2,3) kernel: -1 (default) by grid size -- the one-wave-per-SIMD tile wino_x3w_kernel on grids of >= 130
 *                     workgroups --, 0 / 1 / 2 force the 8- / 4-wave tiles of wino_x3_kernel, 3 forces wino_x3w_kernel.  Every tile gives the same
 *                     bits; 0 is the run-time fallback for wino_x3w_kernel (its hand-issued register loads need a spill-free build, which
 *                     csrc/check_resources.py enforces at build time)
 *   fpn_deferred      0/1 MCG_F16X3 (default 1): the FPN P2 output conv is left to the decoder and computed per 8 x 8-pixel block, only where the
 *                     RoIAlign of some stage reads (mcg_backbone_fpn_forward_deferred / mcg_decoder_forward_deferred, mcg_clip_forward); bit-identical
 *                     to the dense conv.  0 = every level dense in the trunk, launch for launch.  Off for other precisions, under range_audit
 *                     (which audits whole P tensors) and for levels beyond 512 x 512 pixels.  Not to be changed between the two calls of a pair
 *   fpn_lateral_deferred 0/1 (default 1), honoured only where fpn_deferred holds: the P2 lateral conv (+ nearest-upsampled P3 term) is left to the
 *                     decoder as well and computed only for the 8 x 8 blocks the deferred output conv reads -- the listed blocks and their
 *                     neighbours inside the frame.  The trunk then writes C2 and the P3 inner map into the slot.  Bit-identical; 0 = the dense
 *                     lateral in the trunk, launch for launch.  Not to be changed between the two calls of a pair
 *   fpn_levels_deferred 0 / 1 / mask (default 1), honoured only where fpn_deferred holds: the output convs of P3 .. P5 are left to the decoder and
 *                     computed per FRAME, for the frames in which a box of some stage reads the level.  1 = the default set (P5 alone: the only level
 *                     a 224-pixel frame's boxes leave unread, profiles/fpn_levels_deferred_*.md); a mask of 2 (P3) | 4 (P4) | 8 (P5) names the
 *                     levels; 0 = dense in the trunk, launch for launch.  Bit-identical.  Not to be changed between the two calls of a pair
 *   range_audit      0/1 DEBUG (MCG_F32 / MCG_F16X3; default 0): after every activation tensor the trunk writes, a counting kernel tallies the
 *                     values beyond the fp16 range (|x| > 65504: an f16x3 operand half would saturate there) and the non-finite ones;
 *                     read and reset with mcg_engine_range_audit.  Turning it on allocates the counters (the library's only allocation,
 *                     at option time); it costs a pass over every activation, so it is off in the product path. */
int mcg_engine_set_option(mcg_engine* e, const char* name, int value);
/* Read-out of the range_audit option: synchronises the device (a debug call), copies the counters of the first min(capacity, tensors)
 * audited tensors to the host and resets them.  counts[2 i] = values with |x| > 65504, counts[2 i + 1] = non-finite values of tensor i,
 * summed over every frame processed since the last read; names (optional, [capacity]) receives engine-owned tensor names ("stem",
 * "layer3.2.conv1", "fpn.P2", ...) valid until the option changes.  A real checkpoint whose activations leave the fp16 range shows up
 * here layer by layer instead of as a silently saturated gaze vector. */
int mcg_engine_range_audit(mcg_engine* e, unsigned long long* counts, const char** names, int capacity, int* n_out);
/* chunk_frames: the trunk runs in chunks of this many frames so that layer outputs stay
 * resident in the 256 MiB Infinity Cache (0 = all frames in one pass). */
size_t mcg_engine_workspace_bytes(const mcg_engine* e, int num_frames, int H, int W, int chunk_frames);
/* Backbone + FPN only: img NCHW f32 [N,3,H,W] -> P2..P5 NHWC dtype. */
int mcg_backbone_fpn_forward(mcg_engine* e, mcg_stream s, const float* img, int num_frames, int H, int W,
                             int chunk_frames, void* const pyramid[4], void* ws, size_t ws_bytes);
/* Decoder only: 4 x (RoIAlign + GazeSTQIHead + box refinement) + GazeHead over an existing pyramid
 * (MultiClueGazeROIHead.simple_test, multiclue_gaze_roi_head.py:287-384).  Separate from the trunk so a caller can
 * overlap the decoder of batch k with the trunk of batch k+1 on a second stream (mcgaze_amd/engine.py: PipelinedRunner).
 * img_hw: DEVICE int [num_frames][2] = img_shape (h, w) per frame, or NULL when every frame fills the padded H x W
 * (query boxes scale with img_shape, fixed_embedding_rpn_head.py:80-89).  Outputs (device, f32):
 *   gaze_out [4][N][3] (fused, face, eyes, head), boxes_out [N][3][4], scores_out [N][3] (sigmoid). */
size_t mcg_trunk_workspace_bytes(const mcg_engine* e, int num_frames, int H, int W, int chunk_frames);
size_t mcg_decoder_workspace_bytes(const mcg_engine* e, int num_frames);
int mcg_decoder_forward(mcg_engine* e, mcg_stream s, const void* const pyramid[4], int num_frames, int clip_length, int H, int W,
                        const int* img_hw, float* gaze_out, float* boxes_out, float* scores_out, void* ws, size_t ws_bytes);
/* ABI 14: mcg_decoder_forward over window frames gathered from a pyramid STORE: pyramid[i] holds pyramid_frames rows
 * [pyramid_frames][(H/4) >> i][(W/4) >> i][256] (e.g. one row per distinct frame of overlapping windows, each written once by
 * mcg_backbone_fpn_forward at a row offset), and window frame n (n < num_frames = windows * clip_length) reads row frame_of[n]
 * (DEVICE int32 [num_frames]).  img_hw, when given, is indexed by pyramid ROW: [pyramid_frames][2].  Replaces, like mcg_decoder_forward,
 * MultiClueGazeROIHead.simple_test (multiclue_gaze_roi_head.py:287-384) -- per window of the reference's sliding-window harness
 * (tools/test_gaze360_gaze.py:72-111), whose trunk it no longer repeats for the frames windows share.  The gather is done by the
 * RoIAlign reads and the query init; workspace = mcg_decoder_workspace_bytes(e, num_frames).  Outputs are bit for bit those of
 * mcg_decoder_forward on a pyramid holding the gathered rows in window order.  An entry outside [0, pyramid_frames) is read as no row
 * (clamped address) and gives that frame NaN boxes and features: a guard, callers range-check (mcgaze_amd/engine.py::HipEngine.decode).
 * mcg_decoder_forward is this call with frame_of = NULL (row n for frame n, pyramid_frames = num_frames). */
int mcg_decoder_forward_indexed(mcg_engine* e, mcg_stream s, const void* const pyramid[4], int pyramid_frames, const int32_t* frame_of,
                                int num_frames, int clip_length, int H, int W, const int* img_hw, float* gaze_out, float* boxes_out,
                                float* scores_out, void* ws, size_t ws_bytes);
/* ABI 16: the decoder over clips of different lengths (see mcg_stage_forward_ragged for clip_start / num_clips / max_clip_length and the
 * guard; generalises multiclue_gaze.py:77-78,119 and gaze_stqi_head.py:156-166).  frame_of may be NULL: then pyramid_frames = num_frames
 * and frame n reads row n (mcg_decoder_forward's case); else it is mcg_decoder_forward_indexed's table. */
int mcg_decoder_forward_ragged(mcg_engine* e, mcg_stream s, const void* const pyramid[4], int pyramid_frames, const int32_t* frame_of,
                               int num_frames, const int* clip_start, int num_clips, int max_clip_length, int H, int W, const int* img_hw,
                               float* gaze_out, float* boxes_out, float* scores_out, void* ws, size_t ws_bytes);
/* ABI 15: the same pair over a DEFERRED pyramid.  slot: caller-owned device memory of mcg_deferred_pyramid_bytes(e, N, H, W) bytes that
 * carries one batch from the trunk to the decoder (double-buffer it to overlap batches, mcgaze_amd/engine.py: PipelinedRunner): P2..P5,
 * and, when the engine defers P2 (option fpn_deferred), the P2 top-down inner map, a flag per 8 x 8 output block of P2 and one block list
 * per stage.  The trunk then writes P3..P5 and the inner map; before each stage's RoIAlign the decoder flags the P2 blocks that stage's
 * boxes read (the RoIAlign sample arithmetic itself, roi_sample.hpp) and computes those not yet computed (no host sync: graph-capturable).
 * P2 pixels no box reads are never written.  Outputs are bit for bit those of mcg_backbone_fpn_forward + mcg_decoder_forward.
 * With the P2 lateral deferred too (option fpn_lateral_deferred) the slot also holds C2, the P3 inner map, a flag per 8 x 8 INNER block and
 * one inner-block list per stage: the trunk writes C2 and the P3 inner map there, and the decoder computes, before a stage's output blocks,
 * the inner blocks they read (themselves and their in-frame neighbours) that no earlier stage computed.  Inner pixels nobody reads are
 * never written.
 * mcg_deferred_pyramid_levels: where the slot's P2..P5 lie; *deferred (optional) = whether the engine defers P2 for this shape.
 * mcg_deferred_pyramid_state (test / measurement aid): where the slot's P2 inner map [N][H/4][W/4][256] lies (NULL: P2 not deferred) and,
 * where *lateral_deferred is 1, the inner-block flags [*blocks], counts [stages] and lists [stages][*blocks] (else NULL); any output
 * pointer may be NULL.  mcg_inner_block_neighbours: the host twin of the inner-block rule -- the blocks (id itself included, at most nine)
 * whose inner pixels output block id of a [.][H][W] map reads; returns how many were written to out.
 * mcg_inner_mark_blocks (ABI 20; tests and measurements): inner_mark_kernel as a stand-alone operator (launch_inner_mark).  out_list holds
 * min(*out_count, nblk) output block ids (device; an id outside [0, nblk) is skipped); every block mcg_inner_block_neighbours names for one
 * of them whose state is 0 gets state 1 and is appended, list[(*count)++] = id, in unspecified order; a block whose state is non-zero is not
 * listed.  nblk = frames * ceil(H / 8) * ceil(W / 8): the length of state and the capacity of out_list and list.  *count is added to.
 * Addition to ABI 20, option fpn_levels_deferred (0 = off, 1 = the engine's default set -- P5 --, else a mask of 2 = P3 | 4 = P4 | 8 = P5; only where P2
 * is deferred): the output conv of each such level is left to the decoder as well, by whole FRAMES.  The slot then holds that level's inner
 * map (written there by the trunk), a flag per frame and one frame list per stage; before a stage's RoIAlign the mark launch lists the frames
 * one of the stage's boxes reads on the level that no earlier stage listed, and the conv runs over that list.  Frames of a level nobody reads
 * are never written.  mcg_deferred_pyramid_frame_state (test / measurement aid): level 1 .. 3's flags [N], counts [stages] and lists
 * [stages][N] where *frame_deferred is 1 (else NULL). */
size_t mcg_deferred_pyramid_bytes(const mcg_engine* e, int num_frames, int H, int W);
int mcg_deferred_pyramid_levels(const mcg_engine* e, void* slot, int num_frames, int H, int W, void* levels[4], int* deferred);
int mcg_deferred_pyramid_state(const mcg_engine* e, void* slot, int num_frames, int H, int W, void** inner, int** flags, int** counts,
                               int** lists, int* blocks, int* lateral_deferred);
int mcg_deferred_pyramid_frame_state(const mcg_engine* e, void* slot, int num_frames, int H, int W, int level, int** flags, int** counts,
                                     int** lists, int* frame_deferred);
int mcg_inner_block_neighbours(int id, int H, int W, int out[9]);
int mcg_inner_mark_blocks(mcg_stream s, const int* out_list, const int* out_count, int H, int W, int nblk, int* state, int* list, int* count);
int mcg_backbone_fpn_forward_deferred(mcg_engine* e, mcg_stream s, const float* img, int num_frames, int H, int W, int chunk_frames,
                                      void* slot, size_t slot_bytes, void* ws, size_t ws_bytes);
int mcg_decoder_forward_deferred(mcg_engine* e, mcg_stream s, void* slot, size_t slot_bytes, int num_frames, int clip_length, int H, int W,
                                 const int* img_hw, float* gaze_out, float* boxes_out, float* scores_out, void* ws, size_t ws_bytes);
/* ABI 16: mcg_decoder_forward_deferred over clips of different lengths (mcg_stage_forward_ragged: the table, its contract and the guard;
 * multiclue_gaze.py:77-78,119, gaze_stqi_head.py:156-166). */
int mcg_decoder_forward_deferred_ragged(mcg_engine* e, mcg_stream s, void* slot, size_t slot_bytes, int num_frames, const int* clip_start,
                                        int num_clips, int max_clip_length, int H, int W, const int* img_hw, float* gaze_out,
                                        float* boxes_out, float* scores_out, void* ws, size_t ws_bytes);
/* Whole path = mcg_backbone_fpn_forward_deferred + mcg_decoder_forward_deferred on one stream (the slot inside ws);
 * ws >= mcg_engine_workspace_bytes. */
int mcg_clip_forward(mcg_engine* e, mcg_stream s, const float* img, int num_frames, int clip_length, int H, int W,
                     const int* img_hw, int chunk_frames, float* gaze_out, float* boxes_out, float* scores_out,
                     void* ws, size_t ws_bytes);
/* ABI 16: the whole path over clips of different lengths -- e.g. one clip per person per segment, each as long as the person stays in
 * view (MCGaze_demo/demo.ipynb, cell 4), in ONE call instead of one per clip (multiclue_gaze.py:77-78,119 take one clip_length;
 * gaze_stqi_head.py:156-166 is the only step that groups by clip).  mcg_stage_forward_ragged states the table's contract and the guard. */
int mcg_clip_forward_ragged(mcg_engine* e, mcg_stream s, const float* img, int num_frames, const int* clip_start, int num_clips,
                            int max_clip_length, int H, int W, const int* img_hw, int chunk_frames, float* gaze_out, float* boxes_out,
                            float* scores_out, void* ws, size_t ws_bytes);
/* ABI 17: a pyramid store SHARED by many live streams.  The reference's harness runs one sliding window of one video per call
 * (tools/test_gaze360_gaze.py:72-111) and its demo one clip per tracked person (MCGaze_demo/demo.ipynb, cell 4); with S cameras or
 * people that is S trunk calls of one new frame each per tick.  Batched across streams, one trunk call takes every stream's new frames --
 * and their rows in the shared store are whatever rows are free, in no order (streams of different pace free rows out of order).
 * Copies frame n of src (a contiguous NHWC pyramid of num_frames frames, as mcg_backbone_fpn_forward writes it) to row row_of[n] of dst
 * (a store of store_rows frames per level), all four levels in one launch.  row_of: DEVICE int32[num_frames].  A row outside
 * [0, store_rows) is skipped (nothing is written for that frame); two frames naming one row is the caller's error (host-checked in Python,
 * mcgaze_amd/engine.py::check_row_table).  Level pointers 16-byte aligned; H, W multiples of 32; at most 65535 frames per call.
 * No allocation, no host sync, graph-capturable. */
int mcg_pyramid_scatter_rows(mcg_stream s, mcg_dtype dt, const void* const src[4], void* const dst[4],
                             int num_frames, int store_rows, int H, int W, const int32_t* row_of);
/* The overlap merge on the device (an addition to ABI 18: nothing that existed changes).  The reference's harness averages the frames two
 * sliding windows share on the host, window after window (tools/test_gaze360_gaze.py:129-206), after rescale=True has divided every box by
 * its frame's scale_factor (multiclue_gaze_roi_head.py:360-363).  Here the outputs of ONE decoder call -- any number of windows of any
 * number of streams -- are folded into a store of per-frame result rows that stays in device memory.  The merge is sequential per frame
 * and not associative (three windows on one frame give ((a + b) / 2 + c) / 2), so the table is per DESTINATION frame: the decoder-output
 * frames that land on it, in plan order (mcgaze_amd/harness.py::merge_plan).
 *   gaze [4][n][3], boxes [n][3][4], scores [n][3]   DEVICE f32: the decoder's outputs over n = num_frames frames
 *   scale            NULL, DEVICE f32 [4] (scale_per_frame = 0) or [n][4] (scale_per_frame = 1): every box is divided by it, IEEE f32
 *   plan             DEVICE int32 [num_dst][2 + max_src]: dst_row, cont, src[max_src] (-1 = none).  cont = 1: an earlier call wrote
 *                    row dst_row and the fold starts from it; cont = 0: the first source starts it
 *   store            DEVICE f32 [store_rows][27]: det[3][5] (x1 y1 x2 y2 score) | fused[3] | others[3][3], clues in the order face, eyes, head
 * Per (destination frame, clue), for its sources in order: the box of a source whose score is < person_threshold is zeroed; the first
 * state is the source itself; afterwards box = (old score < threshold or new score < threshold) ? 0 : (old + new) / 2 and score, fused
 * and per-clue gaze = (old + new) / 2 -- f32, uncontracted: the bits of the host merge.  A dst_row outside [0, store_rows) skips that
 * row and a source outside [0, n) skips that source: defined, never a stray access (the Python side rejects such a table first); two
 * rows naming one dst_row is the caller's error.  num_dst and max_src are host integers; no allocation, no host sync, graph-capturable. */
int mcg_merge_windows(mcg_stream s, const float* gaze, const float* boxes, const float* scores, int num_frames, const float* scale,
                      int scale_per_frame, const int32_t* plan, int num_dst, int max_src, float* store, int store_rows,
                      float person_threshold);
/* Temporal smoothing on the device (an addition to ABI 18: nothing that existed changes).  The reference's published accuracy is measured
 * on smoothed predictions: tools/calculate_mae_gaze360.py:16-29 (smooth_filter) mixes every gaze vector of a video with its neighbours in
 * time -- alpha 0.6, three taps in the interior, two at the ends -- and re-normalises; a video of one frame is returned as it is.  Here the
 * rows are those of the store mcg_merge_windows keeps, and one launch covers any number of frames of any number of streams: the table
 * names, per output frame, the store rows of the frame and of its neighbours (mcgaze_amd/harness.py::smooth_plan).
 *   store  DEVICE f32 [store_rows][27], the rows of mcg_merge_windows: floats 15..17 the fused gaze, 18..26 the three clues' gazes
 *   plan   DEVICE int32 [num_out][3]: previous row, row, next row; -1 = no such neighbour (the stream's first / last frame)
 *   out    DEVICE f32 [num_out][12]: the smoothed fused gaze [3] | the smoothed clues' gazes [3][3]
 * THE ARITHMETIC, for each of a frame's four vectors: x the vector of the frame, p and q the same vector of the previous and the next
 * frame, a = (float)alpha, b = (float)(1.0 - (double)alpha); every operation f32 and uncontracted.  Per component
 *   both neighbours:   o = a * x;  o = o + (b * (p + q)) / 2
 *   only the next:     o = a * x + b * q
 *   only the previous: o = a * x + b * p
 *   neither:           the output is x itself, NOT normalised (smooth_filter's size(0) < 2 branch)
 * and in the first three cases n = sqrtf(fmaf(o2, o2, fmaf(o1, o1, o0 * o0))) -- the two fma explicit, what torch.norm computes on the CPUs
 * this was compared on -- and the output is o / n, an IEEE division.  No guard for n == 0 or input that is not finite: the reference
 * has none, the IEEE result stands.
 * A row outside [0, store_rows), or a neighbour that is neither -1 nor inside it, is never used as an address: that output row (all four
 * vectors) is written as NaN.  num_out = 0 returns MCG_OK without a launch.  alpha must be finite (the Python side takes (0, 1]).
 * No allocation, no host sync, graph-capturable. */
int mcg_smooth_gaze(mcg_stream s, const float* store, int store_rows, const int32_t* plan, int num_out, double alpha, float* out);

/* ---------------------------------------------------------------- test-time preprocessing
 * One launch replaces the per-frame CPU transforms the reference's test pipeline applies between image decode and the model
 * (configs/_base_/datasets/gaze360.py:27-36): CenterCrop (mmdet/datasets/pipelines/transforms.py:1036-1052; the window is
 * chosen by the caller, who owns the RNG draw of :1126-1130) -> Resize(keep_ratio) (transforms.py:216-242, cv2 INTER_LINEAR on
 * 8-bit pixels) -> Normalize(to_rgb) (:739-755) -> Pad + batch collate (zeros right/below, :665-683) -> HWC->CHW
 * (formatting.py:229-231).  frames_dev: DEVICE array of num_frames descriptors; every src points at a decoded uint8 frame in
 * device memory, 3 interleaved channels in cv2 order (BGR), rows src_pitch bytes apart.  The crop window must lie inside the
 * frame; (out_h, out_w) is the resized size, <= (pad_h, pad_w).  dst: [num_frames][3][pad_h][pad_w] f32 = the `img` tensor
 * mcg_clip_forward takes.  mean / stdinv: host arrays, channel order of the OUTPUT (RGB when to_rgb).  to_rgb is a plain swap of
 * channels 0 and 2 on the way out: a caller whose decoder already delivers RGB passes the frames as they are and to_rgb = 0. */
typedef struct mcg_frame_desc {
  const void* src;
  int src_h, src_w, src_pitch;
  int crop_y, crop_x, crop_h, crop_w;
  int out_h, out_w;
} mcg_frame_desc;
int mcg_preprocess_frames(mcg_stream stream, const mcg_frame_desc* frames_dev, int num_frames, float* dst, int pad_h, int pad_w,
                          const float mean[3], const float stdinv[3], int to_rgb);
/* ABI 18: head crops -- video frames and one head box per person per frame in, the model's `img` tensor and the decoder's per-frame tables
 * out.  Replaces what the reference's demo does on the host for every (person, frame) before its Compose(cfg.data.test.pipeline[1:])
 * (MCGaze_demo/demo.ipynb, cell 4): head_center = [int(y1 + y2) // 2, int(x1 + x2) // 2], l = int(max(y2 - y1, x2 - x1) * 0.8), the slice
 * img[max(0, cy - l):min(cy + l, rows), max(0, cx - l):min(cx + l, cols)] -- then Resize(keep_ratio=True)'s size rule (transforms.py:216-242
 * -> mmcv rescale_size: f = min(long / max(h, w), short / min(h, w)), int(side * f + 0.5)) and the `scale_factor` / `img_shape` metas
 * (transforms.py:236-242).  Two launches: head_crop_plan_kernel (one thread per crop, double arithmetic, uncontracted) writes
 * desc_out_dev, then the pixel kernel of mcg_preprocess_frames runs over it unchanged.  Crops may share an image: each frame is in device
 * memory once however many heads it shows.
 *   images_dev   DEVICE array of num_images (>= 1) frames: uint8, 3 interleaved channels, rows pitch bytes apart
 *   boxes_dev    DEVICE f32 [n][4] x1 y1 x2 y2 in pixels of the crop's image (a detector's output as it is)
 *   image_of_dev DEVICE int32 [n]: the image each crop is cut from
 *   expand       the demo's 0.8 (finite);  scale_w, scale_h: Resize's img_scale
 *   desc_out_dev DEVICE [n]: the window (crop_y, crop_x, crop_h, crop_w) and resized size (out_h, out_w) chosen per crop
 *   img_hw_dev   DEVICE int32 [n][2] (out_h, out_w): what the forward and decoder entries take as img_hw
 *   scale_factor_dev DEVICE f32 [n][4] (w, h, w, h) factors, (float)((double)new / (double)old): rescale=True divides the boxes by it
 *   flags_dev    DEVICE int32 [n] or NULL.  0: the demo's window.  1: the demo's slice would be empty (a box of no extent, or one wholly
 *                outside the frame) -- the window is ONE pixel, moved inside the frame.  2: a box that is not finite, an image_of outside
 *                [0, num_images) or an image without pixels -- the crop reads pixel (0, 0) of image 0 as a 1 x 1 window.
 *   dst          [n][3][pad_h][pad_w] f32; pad_h >= scale_h and pad_w >= scale_w (a non-square img_scale: both >= its long edge, keep_ratio
 *                puts the long edge on the window's long side).  A resized side that would round to 0 is 1.
 * Nothing is read outside an image for ANY box or index, and nothing is read on the host: no allocation, no host sync,
 * graph-capturable; at most 65535 crops per call.  mean / stdinv / to_rgb as in mcg_preprocess_frames. */
typedef struct mcg_image_desc {
  const void* src;
  int h, w, pitch;
} mcg_image_desc;
int mcg_preprocess_head_crops(mcg_stream s, const mcg_image_desc* images_dev, int num_images, const float* boxes_dev,
                              const int32_t* image_of_dev, int n, double expand, int scale_w, int scale_h, mcg_frame_desc* desc_out_dev,
                              int32_t* img_hw_dev, float* scale_factor_dev, int32_t* flags_dev, float* dst, int pad_h, int pad_w,
                              const float mean[3], const float stdinv[3], int to_rgb);
/* NV12 surfaces in (additions to ABI 18; nothing above changes): the two pixel entries again, reading what a hardware video decoder
 * delivers -- a full-resolution Y plane and a half-resolution plane of interleaved (U, V) pairs, each with its own pitch -- instead of
 * packed BGR.  The colour conversion runs per TAP: each of the four source pixels an output pixel interpolates between is converted to
 * three uint8 values (B, G, R) in 32-bit integers and handed to the unchanged fixed-point resize, normalisation and channel swap, so the
 * result equals "convert the whole frame to BGR, then call the entry above" bit for bit, and no packed frame is ever written.  Tap (y, x) in
 * frame coordinates reads Y[y][x], U = UV[y >> 1][2 * (x >> 1)], V = UV[y >> 1][2 * (x >> 1) + 1] (chroma is the NEAREST sample, not
 * interpolated, as in cv2's COLOR_YUV2BGR_NV12), and with u = U - 128, v = V - 128, >> an arithmetic shift and sat8 a clamp to [0, 255]:
 *   yy = max(0, Y - y_off) * cy
 *   R = sat8((yy + cvr * v + (1 << 19)) >> 20);  G = sat8((yy + cvg * v + cug * u + (1 << 19)) >> 20);  B = sat8((yy + cub * u + (1 << 19)) >> 20)
 * coef: HOST pointer to the six integers (20 fractional bits).  Limited-range BT.601, OpenCV's published constants restated (not linked;
 * parity with cv2 is not pinned on any machine this was built on): {16, 1220542, 2116026, -409993, -852492, 1673527}.  Limited-range
 * BT.709 (Kr = 0.2126, Kb = 0.0722, luma 255/219, chroma 255/224, each round(c * 2^20)): {16, 1220945, 2215014, -223607, -558796, 1879825}.
 * The entries accept any coef whose sums stay inside an int: y_off in [0, 255] and |cy|, |cub|, |cug|, |cvg|, |cvr| < 2^22
 * (255 * 2^22 + 2 * 128 * 2^22 + 2^19 < 2^31).
 * h and w of every surface are EVEN; the UV plane is h / 2 rows of w bytes, rows pitch_uv apart.  With even sizes and a window inside the
 * frame nothing is read outside either plane.  mcg_nv12_frame_desc holds the fields of mcg_frame_desc, src and src_pitch naming the Y plane,
 * followed by the UV plane and its pitch; mcg_preprocess_head_crops_nv12 takes the arguments of mcg_preprocess_head_crops with the NV12 image table
 * and descriptor output, writes the same img_hw / scale_factor / flags, and flags an image row whose h or w is odd 2 like one without
 * pixels.  A flag-2 crop reads pixel (0, 0) of image 0 (Y[0] and UV[0..1] of it): whatever the other rows hold, images_dev[0] must be a
 * valid surface with even h and w.  to_rgb as above: the converted taps are in BGR order.  No allocation, no host sync, graph-capturable; at most 65535 rows. */
typedef struct mcg_yuv_coef {
  int y_off, cy, cub, cug, cvg, cvr;
} mcg_yuv_coef;
typedef struct mcg_nv12_image_desc {
  const void* y;
  const void* uv;
  int h, w, pitch_y, pitch_uv;
} mcg_nv12_image_desc;
typedef struct mcg_nv12_frame_desc {
  const void* src;
  int src_h, src_w, src_pitch;
  int crop_y, crop_x, crop_h, crop_w;
  int out_h, out_w;
  const void* uv;
  int uv_pitch;
} mcg_nv12_frame_desc;
int mcg_preprocess_frames_nv12(mcg_stream stream, const mcg_nv12_frame_desc* frames_dev, int num_frames, float* dst, int pad_h, int pad_w,
                               const float mean[3], const float stdinv[3], int to_rgb, const mcg_yuv_coef* coef);
int mcg_preprocess_head_crops_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, const float* boxes_dev,
                                   const int32_t* image_of_dev, int n, double expand, int scale_w, int scale_h,
                                   mcg_nv12_frame_desc* desc_out_dev, int32_t* img_hw_dev, float* scale_factor_dev, int32_t* flags_dev,
                                   float* dst, int pad_h, int pad_w, const float mean[3], const float stdinv[3], int to_rgb,
                                   const mcg_yuv_coef* coef);

/* ---------------------------------------------------------------- annotated frames out (additions to ABI 18; nothing above changes)
 * The last step of the reference's demo (MCGaze_demo/demo.ipynb, cell 5): for every head on every frame
 *   cv2.arrowedLine(frame, centre, tip, (230, 253, 11), thickness=max(5, int(l * 0.01)))
 * drawn on the device, IN PLACE, into packed BGR frames (mcg_draw_gaze_arrows) or into a decoder's NV12 surfaces (mcg_draw_gaze_arrows_nv12):
 * the image tables are those of the head-crop entries, and the planes they name are WRITTEN (the const of their pointers notwithstanding),
 * honouring each plane's pitch.  Two launches: a plan kernel (one thread per row, double, uncontracted) writes one mcg_arrow_desc per row,
 * then a gather kernel over (image, pixel tile) walks the rows of each tile in ascending order and stores the covered pixels.
 * ARROW PLAN, per row, from a head box x1 y1 x2 y2 and a gaze g0 g1 (f32, widened to double; int() truncates, // floors):
 *   cx = int(x1 + x2) // 2;  cy = int(y1 + y2) // 2;  l = int(max(y2 - y1, x2 - x1) * length);  tip = (int(cx - l * g0), int(cy - l * g1))
 *   t = max(min_thickness, int(l * thickness_ratio))             -- mcgaze_amd/harness.py::head_arrows' steps; the demo: 1.0, 5, 0.01
 * HEAD STROKES, as OpenCV's published arrowedLine computes them (tip_length, the demo's default 0.1), restated without atan2, cos or sin so
 * that two libms cannot disagree: pt1 = (cx, cy), pt2 = tip, dx = pt1.x - pt2.x, dy = pt1.y - pt2.y, k = tip_length * 0.7071067811865476
 * (the double nearest sqrt(0.5)); the strokes start at
 *   (rint(pt2.x + k * (dx - dy)), rint(pt2.y + k * (dx + dy)))   and   (rint(pt2.x + k * (dx + dy)), rint(pt2.y + k * (dy - dx)))
 * rint rounding half to even, every product and every sum rounded on its own (no FMA).  An arrow is three segments of thickness t: the
 * shaft pt1 -> pt2 and the two strokes into pt2 -- seg[0], seg[1], seg[2] of the descriptor, each (from, to) x (x, y).
 * This is OpenCV's rule restated, not linked: parity with cv2's own rasteriser (a polygon fill with its own end caps) is NOT claimed and is
 * not pinned on any machine this was built on.
 * COVERAGE: the pixel with integer centre p belongs to segment a -> b iff its squared distance to the segment is at most (t / 2)^2 -- a
 * capsule; a segment of no length gives a disc.  Exactly, in 64-bit integers: d = b - a, L = d . d, u = (p - a) . d;
 *   u <= 0: 4 |p - a|^2 <= t^2;   u >= L: 4 |p - b|^2 <= t^2;   otherwise 4 (|p - a|^2 L - u^2) <= t^2 L
 * The bound under which this is exact: every end point coordinate in [-8191, 8191], frames of at most 8192 pixels a side, t <= 255 -- then
 * every difference is below 2^14, L and |u| below 2^29 and the left side below 2^60.
 * FLAGS (int32 per row, the head-crop convention).  0: drawn -- zero covered pixels is allowed (an arrow wholly outside its frame).
 * 2: an unusable row, and NOTHING is written for it: a box or gaze that is not finite, an image_of outside [0, num_images), an image
 * without pixels (NV12: with an odd size) or larger than (max_h, max_w), an end point or thickness beyond the bound.  Its descriptor is
 * zero but for image = -1 and flag = 2.
 * OVERLAP: where arrows overlap the HIGHEST ROW INDEX wins, whatever the launch geometry or the scheduling (each pixel is written once, by
 * one thread, after it has seen every row).
 * NV12: the Y plane gets the colour's Y at every covered pixel; the chroma pair UV[y >> 1][2 (x >> 1) .. + 1] gets the colour's (U, V) iff
 * ANY of its four luma pixels is covered -- by several rows: the highest of them.  The colour is given as (Y, U, V)
 * (mcgaze_amd/pipeline.py::bgr_to_yuv); read back through the conversion above, every covered pixel shows exactly that triple's BGR.
 *   images_dev   DEVICE table as for the head-crop entries, num_images in 1 .. 65535
 *   max_h, max_w the largest frame of the table, each 1 .. 8192: the raster grid is sized from them (a larger image is flagged, not drawn)
 *   boxes_dev    DEVICE f32 [n][4];  image_of_dev DEVICE int32 [n]
 *   gaze_dev     DEVICE f32, row k at gaze_dev + k * gaze_stride (floats, >= 2): g0, g1 -- e.g. the [n][3] fused gaze as it is
 *   length, thickness_ratio, tip_length: finite;  min_thickness in 1 .. 255
 *   color        HOST uint8[3] (B, G, R; NV12: Y, U, V), used for every row when colors_dev is NULL;  colors_dev DEVICE uint8 [n][3], one per row
 *   plan_out_dev DEVICE [n] descriptors (written);  flags_dev DEVICE int32 [n] or NULL
 * No byte outside [0, h) x [0, w) of any plane is touched, padding included, for ANY box, gaze or index.  No allocation, no host sync,
 * graph-capturable; at most 65535 rows per call; n = 0 returns MCG_OK without a launch.  Every wave of the raster grid reads the plan in
 * n / 64 slices: made for the tens of heads of video frames. */
typedef struct mcg_arrow_desc {
  int seg[3][2][2];         /* shaft, stroke, stroke: (from, to) x (x, y) */
  int thickness;
  int x0, y0, x1, y1;       /* bounding box of the covered pixels clipped to the frame, half open; may be empty */
  int image, flag;
  int reserved;
} mcg_arrow_desc;
int mcg_draw_gaze_arrows(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                         const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n, double length, int min_thickness,
                         double thickness_ratio, double tip_length, const unsigned char* color, const unsigned char* colors_dev,
                         mcg_arrow_desc* plan_out_dev, int32_t* flags_dev);
int mcg_draw_gaze_arrows_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                              const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n, double length, int min_thickness,
                              double thickness_ratio, double tip_length, const unsigned char* yuv, const unsigned char* yuvs_dev,
                              mcg_arrow_desc* plan_out_dev, int32_t* flags_dev);

/* ---------------------------------------------------------------- head boxes from raw detector output (additions to ABI 18; nothing above changes)
 * What a detector hands over is not head boxes: the demo's YOLOv5 head detector emits a raw [B][N][5 + nc] prediction (25 200 anchors per
 * 640-pixel frame, nc = 2: person, head), and boxes only exist after non_max_suppression and scale_coords(...).round()
 * (MCGaze_demo/yolo_head/detect.py:74,95; utils/general.py:291-312, 393-481).  mcg_detect_heads is that post-processing on a prediction in
 * device memory: ONE launch, one workgroup per image, no allocation, no host sync, no state, graph-capturable.  The network itself stays
 * outside this library.
 * THE ARITHMETIC.  It is the reference function on a float32 prediction with classes=[only_class] (or None) and multi_label=False, then
 * scale_coords(...).round().  Every operation is f32 and uncontracted (no FMA) unless it says double; thr = (float)conf_thres,
 * it = (float)iou_thres.  Row a of image b is p = pred_dev + b * image_stride + a * row_stride (floats): x, y, w, h, objectness, nc classes.
 *  1. p is a candidate iff p[4] > thr.  sc[c] = p[5 + c] * p[4];  conf = max over c of sc[c] and cls the LOWEST c that reaches it (a NaN
 *     score makes conf NaN, as torch's max does).  The row is kept iff conf > thr and (only_class < 0 or cls == only_class).
 *  2. x1 = p[0] - p[2] / 2, y1 = p[1] - p[3] / 2, x2 = p[0] + p[2] / 2, y2 = p[1] + p[3] / 2.  A row whose four box values or conf are not
 *     all finite is DROPPED here -- a stated deviation: it is the reference's commented-out "finite constraint" (the IEEE result of a NaN
 *     box differs between fmaxf and torch.clamp, and the head-crop entries would flag such a box anyway).
 *  3. Candidate order: conf descending, ties by the LOWER anchor index (the reference leaves ties to its sort; -0 and +0 are one score).
 *     If more than max_nms rows remain only the first max_nms in that order take part and the image's flag is 1: greedy NMS decides a row
 *     from the rows before it only, so the result on the prefix is the full result restricted to it.
 *  4. NMS offset o = agnostic ? 0 : (float)cls * 4096.0f, added to all four coordinates, each an f32 add (the reference's max_wh trick;
 *     the rounding it introduces is part of the decision).
 *  5. Greedy NMS walks that order; a row j is kept iff no earlier KEPT row i has iou(i, j) > it, with, on the offset boxes,
 *       area = (x2 - x1) * (y2 - y1);  w = max(0, min(x2i, x2j) - max(x1i, x1j)), h likewise;  inter = w * h;
 *       iou = inter / (area_i + area_j - inter)                    -- an IEEE division; 0 / 0 is NaN and suppresses nothing
 *     This is torchvision's published nms rule restated, not linked: parity with its binary is not claimed or pinned, nor is the demo's
 *     fp16 arithmetic (model.half()) -- the claim is the reference function on pred.float() with the CPU's arithmetic.
 *  6. The first max_det kept rows are the image's detections, in that order.
 *  7. Scale-back of the UN-offset box from the detector's letterboxed input (in_h, in_w) into the frame (h0, w0), in double:
 *       gain = min(in_h / h0, in_w / w0);  pad_x = (in_w - w0 * gain) / 2;  pad_y = (in_h - h0 * gain) / 2
 *     then g = (float)gain, px = (float)pad_x, py = (float)pad_y and per coordinate v = (v - px) / g (py for y; an IEEE division, not a
 *     reciprocal multiply), clamped to [0, w0] (x) or [0, h0] (y): v < 0 ? 0 : v, then v > hi ? hi : v; then rintf, half to even.
 *  8. Row k < counts[b] of image b: boxes = x1 y1 x2 y2, scores = conf, classes = cls, image_of = b.  Rows from counts[b] up are zero with
 *     image_of = -1 -- what the head-crop and draw entries flag as an unusable row, so boxes as [B * max_det][4] and image_of as
 *     [B * max_det] feed them with no read-back, inside one graph.
 * FLAGS (int32 per image): 0; 1: more than max_nms candidates, the prefix was used; 2: h0 <= 0 or w0 <= 0 -- count 0, nothing is read or
 * divided for that image.
 *   pred_dev      DEVICE f32; row_stride >= 5 + num_classes, image_stride >= 0 (floats); fp16 predictions are widened by the caller (exact)
 *   frame_hw_dev  DEVICE int32 [B][2]: h0, w0 of each image's frame;  in_h, in_w >= 1
 *   conf_thres, iou_thres finite;  only_class: -1 for every class;  max_det in 1 .. 300;  max_nms in 1 .. num_anchors
 *   boxes_dev [B][max_det][4] f32, scores_dev [B][max_det] f32, classes_dev, image_of_dev [B][max_det] int32, counts_dev [B] int32,
 *   flags_dev [B] int32 or NULL: all written in full
 *   ws_dev, ws_bytes: DEVICE scratch of at least mcg_detect_heads_workspace_bytes(num_images, num_anchors) bytes, 16-byte aligned (32 bytes
 *   per anchor: keys, sorted offset boxes, anchors, marks); the workspace function returns 0 for sizes the entry refuses
 * num_images in 0 .. 65535 (0: MCG_OK without a launch), num_anchors in 1 .. 2^24.  Argument errors (num_classes < 1, max_det or max_nms out of
 * range, a small workspace, a threshold that is not finite, bad strides, a null pointer) return MCG_ERR_ARG before any launch.  The result
 * does not depend on launch geometry or scheduling.  Ordering costs O(M^2) for M candidates on one compute unit: made for the hundreds a 0.25
 * threshold leaves; at num_anchors candidates it stays correct and takes milliseconds. */
size_t mcg_detect_heads_workspace_bytes(int num_images, int num_anchors);
int mcg_detect_heads(mcg_stream s, const float* pred_dev, int num_images, int num_anchors, int num_classes, long long image_stride, int row_stride,
                     int in_h, int in_w, const int32_t* frame_hw_dev /* [B][2] h0, w0 */, double conf_thres, double iou_thres,
                     int only_class /* -1: every class */, int agnostic, int max_nms, int max_det,
                     float* boxes_dev /* [B][max_det][4] */, float* scores_dev /* [B][max_det] */, int32_t* classes_dev /* [B][max_det] */,
                     int32_t* image_of_dev /* [B][max_det] */, int32_t* counts_dev /* [B] */, int32_t* flags_dev /* [B] or NULL */,
                     void* ws_dev, size_t ws_bytes);

/* ---------------------------------------------------------------- the detector's input (additions to ABI 18; nothing above changes)
 * What the demo's head detector reads is not a frame: LoadImages letterboxes it (MCGaze_demo/yolo_head/utils/datasets.py:185-189, 810-840),
 * reverses the channels into planes (:188) and detect.py:64-65 turns the bytes into half or float in [0, 1].  mcg_letterbox_frames does all of
 * that for a batch of frames in device memory in ONE launch; mcg_letterbox_frames_nv12 reads a decoder's NV12 surfaces through the per-tap
 * conversion above.  cv2.resize and cv2.copyMakeBorder are restated, not linked: parity with cv2's binary is NOT claimed and is not pinned on
 * any machine this was built on (the caveat the resize of mcg_preprocess_frames carries).
 * GEOMETRY, on the host, in python floats (IEEE doubles; round() rounds half to even) -- mcgaze_amd/head_detect.py::letterbox_geometry is
 * letterbox(img, new_shape, color=(114, 114, 114), auto, scaleFill=False, scaleup, stride) line for line:
 *   r = min(new_h / h, new_w / w);  scaleup false: r = min(r, 1.0)
 *   unpad_w = int(round(w * r));  unpad_h = int(round(h * r))
 *   dw = new_w - unpad_w;  dh = new_h - unpad_h;  auto: dw %= stride, dh %= stride;  dw /= 2;  dh /= 2
 *   top = int(round(dh - 0.1));  bottom = int(round(dh + 0.1));  left = int(round(dw - 0.1));  right = int(round(dw + 0.1))
 *   out_h = top + unpad_h + bottom;  out_w = left + unpad_w + right
 * An integer new_shape is a square.  scaleFill is not offered.  The entry takes the RESULT per frame: (unpad_h, unpad_w) as the out_h / out_w
 * of the frame descriptor, and top, left.
 * PIXELS.  dst is [num_frames][3][out_h][out_w].  Output pixel (y, x) of a frame lies inside its rectangle iff top <= y < top + unpad_h and
 * left <= x < left + unpad_w.  Inside, it is the WHOLE frame (the descriptor's crop fields are not read) resized to (unpad_h, unpad_w) by the
 * fixed-point bilinear of mcg_preprocess_frames: coefficients of column x - left for unpad_w <- w and of row y - top for unpad_h <- h
 * (source coordinate (d + 0.5) * (src / dst) - 0.5 in double, cast to float, floor + fraction, clamped to the frame with a zero fraction at
 * the borders, 11-bit coefficients rounded half to even), the horizontal pass in 32-bit integers, then
 * uchar((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2).  Everywhere else it is 114.  Two facts that follow, and are not
 * special cases of the code: where the frame already has the unpadded size the reference skips cv2.resize -- every fraction is then zero, one
 * coefficient 2048, and the two passes reproduce the byte; and where cv2 turns an exact 2x INTER_LINEAR reduction into its area path,
 * (a + b + c + d + 2) >> 2, the formula gives the same value because both coefficients are 1024.
 * CHANNELS.  The taps are in the frame's order; plane c of dst is channel 2 - c of the tap when swap_rb (img[:, :, ::-1].transpose(2, 0, 1):
 * RGB planes from BGR frames, and from NV12, whose converted taps are BGR), channel c otherwise (frames that already are RGB).
 * VALUE, by out_type, of the byte v:
 *   MCG_LETTERBOX_U8   v                                              -- LoadImages' own output
 *   MCG_LETTERBOX_F32  (float)v / 255.0f, an IEEE division            -- img.float(); img /= 255.0  (detect.py:64-65)
 *   MCG_LETTERBOX_F16  that float rounded to the nearest half, ties to even.  For all 256 bytes this is what img.half(); img /= 255.0 gives
 *                      (torch divides halves in float and rounds once).  v * (1 / 255) is NOT the same value: it differs for 126 bytes.
 * A descriptor whose rectangle is empty, reaches outside the output or whose frame has no pixels (NV12: an odd size) is not an error of the
 * launch: the rectangle is clipped to the output, a frame that cannot be read gives 114 everywhere.  The table is in device memory and the
 * entry does not read it back; mcgaze_amd checks the geometry on the host before it writes the table.  So for ANY table nothing is read
 * outside [0, h) x [0, w) of a frame (rows pitch bytes apart) and nothing is written outside dst.
 *   frames_dev  DEVICE array of num_frames descriptors: frame.src (.uv), frame.src_pitch (.uv_pitch), frame.src_h, frame.src_w,
 *               frame.out_h = unpad_h, frame.out_w = unpad_w, then top, left
 *   dst         DEVICE, aligned to its element; out_h, out_w >= 1 with out_h * out_w < 2^31
 *   coef        HOST, as for mcg_preprocess_frames_nv12
 * num_frames in 0 .. 65535 (0: MCG_OK without a launch).  A null pointer, a bad size, an unknown out_type, a misaligned dst or a coef outside
 * its bounds return MCG_ERR_ARG before any launch.  One launch, one thread per output pixel (four adjacent pixels for u8 and two for f16 where
 * out_w and dst allow 4-byte stores); no allocation, no host sync, no state, graph-capturable. */
enum { MCG_LETTERBOX_U8 = 0, MCG_LETTERBOX_F16 = 1, MCG_LETTERBOX_F32 = 2 };
typedef struct mcg_letterbox_desc {
  mcg_frame_desc frame;
  int top, left;
} mcg_letterbox_desc;
typedef struct mcg_nv12_letterbox_desc {
  mcg_nv12_frame_desc frame;
  int top, left;
} mcg_nv12_letterbox_desc;
int mcg_letterbox_frames(mcg_stream stream, const mcg_letterbox_desc* frames_dev, int num_frames, void* dst, int out_h, int out_w, int out_type,
                         int swap_rb);
int mcg_letterbox_frames_nv12(mcg_stream stream, const mcg_nv12_letterbox_desc* frames_dev, int num_frames, void* dst, int out_h, int out_w,
                              int out_type, int swap_rb, const mcg_yuv_coef* coef);

/* ---------------------------------------------------------------- head identities across frames (additions to ABI 18; nothing above changes)
 * mcg_detect_heads gives the heads of each frame; which box of frame t is the person of which box of frame t - 1 the demo decides by the
 * NUMBER of heads and their x1 order (harness.segment_tracks, cell 1), on the host.  mcg_track_heads is that decision on the device, by
 * overlap: ONE launch, one workgroup per sequence, the frames of the call walked in order inside the kernel, no allocation, no host sync,
 * graph-capturable.  The result is a pure function of (state, boxes, counts); it does not depend on launch geometry or scheduling.
 * A SEQUENCE is one camera.  Its state is a mcg_track_header followed by `slots` mcg_track_slot records (1 <= slots <= 64); sequence q of a
 * state lies mcg_track_state_bytes(1, slots) bytes behind sequence q - 1.  A slot is LIVE iff id > 0 and FREE iff id == 0; ids are handed
 * out per sequence as 1, 2, 3, ...: a birth gets ++next_id.  All zero bytes are the empty state.  The reserved words are neither read nor
 * written.
 * THE ARITHMETIC, per sequence q and per frame t = 0 .. num_frames - 1 in order.  Every operation is f32 and uncontracted (no FMA);
 * thr = (float)match_iou.  c = counts_dev[q * T + t], n = min(max(c, 0), D); detection d < n is the box
 * boxes_dev + (q * T + t) * frame_stride + 4 * d (floats), x1 y1 x2 y2, in the order mcg_detect_heads emits them: best first.
 *  1. Detection d is USABLE iff its four coordinates are finite.  Rows d >= n are never read.
 *  2. For a live slot a and a usable detection b, with the operations of mcg_detect_heads' NMS:
 *       area = (x2 - x1) * (y2 - y1) of each;  w = max(0, min(a.x2, b.x2) - max(a.x1, b.x1)), h likewise;  inter = w * h;
 *       iou = inter / (area_a + area_b - inter) + 0.0f         -- an IEEE division; the + 0.0f makes -0 and +0 one value
 *     The pair is a CANDIDATE iff iou > thr.  A NaN (0 / 0) never is.  A candidate's iou is >= 0.
 *  3. Greedy match: while a candidate exists whose slot and detection are both unmatched, the one with the largest iou, ties by the LOWER
 *     slot, then the LOWER detection, is matched.  A matched slot takes the detection's box and age = 0.
 *  4. Every live slot left unmatched gets age += 1 and, if age > max_age, is freed: id = 0, age = 0, box zeroed.  A slot that coasts keeps
 *     its last box: there is no motion model.
 *  5. Births: the unmatched usable detections, in index order, each take the LOWEST free slot -- those freed in step 4 of this frame
 *     included: id = ++next_id, age = 0, the detection's box.  A detection that finds no free slot is dropped.
 *  6. Row s of frame (q, t) of the outputs, for a slot matched or born in this frame by detection d: slot_boxes = d's box,
 *     image_of = q * T + t, det_of = d; for every other slot a zero box, image_of = -1, det_of = -1 -- the rows the head-crop and draw entries
 *     flag as unusable, so slot_boxes as [Q * T * S][4] and image_of as [Q * T * S] feed them with no read-back when the frames of the
 *     call are their images.  For every slot: track_id = its id after the frame (0: free), age = its age (-1: free).
 *     flags (q, t): bit 1 a detection was dropped for want of a slot, bit 2 a row d < n was not usable, bit 4 c lay outside 0 .. D.
 * After the call: header.frames_seen += num_frames.
 *   boxes_dev   DEVICE f32 [Q][T][D][4]: frames frame_stride >= 4 * D floats apart, sequence q at q * T * frame_stride
 *   counts_dev  DEVICE int32 [Q][T]
 *   state_dev   DEVICE, 16-byte aligned, mcg_track_state_bytes(Q, slots) bytes: read and updated in place
 *   slot_boxes_dev [Q][T][S][4] f32; image_of_dev, track_id_dev, age_dev, det_of_dev [Q][T][S] int32; flags_dev [Q][T] int32: written in full
 * num_sequences in 0 .. 65535 (0: MCG_OK without a launch) with Q * T * S < 2^31.  slots outside 1 .. 64, max_det outside 1 .. 1024,
 * num_frames < 1, max_age < 0, a match_iou that is not finite, a null pointer, a misaligned state or a frame_stride below 4 * D return
 * MCG_ERR_ARG before any launch.  A match round costs one pass over the slots x detections pairs on one compute unit; there are at most
 * min(slots, n) rounds per frame.  mcgaze_amd/head_detect.py::track_heads_host is the same on the host, bit for bit. */
typedef struct mcg_track_header {
  int32_t next_id;      /* ids handed out so far: the next birth gets next_id + 1 */
  int32_t frames_seen;
  int32_t reserved[2];
} mcg_track_header;
typedef struct mcg_track_slot {
  float box[4];         /* x1 y1 x2 y2 of the last match; zero while free */
  int32_t id;           /* 0: free */
  int32_t age;          /* frames since the last match; 0 while free */
  int32_t reserved[2];  /* mcg_track_heads: neither read nor written; mcg_track_heads_motion: the bits of vx, vy (f32) */
} mcg_track_slot;
size_t mcg_track_state_bytes(int num_sequences, int slots);   /* 0 for sizes the entry refuses */
int mcg_track_heads(mcg_stream s, const float* boxes_dev, long long frame_stride, const int32_t* counts_dev, int num_sequences, int num_frames,
                    int max_det, int slots, double match_iou, int max_age, void* state_dev,
                    float* slot_boxes_dev /* [Q][T][S][4] */, int32_t* image_of_dev /* [Q][T][S] */, int32_t* track_id_dev /* [Q][T][S] */,
                    int32_t* age_dev /* [Q][T][S] */, int32_t* det_of_dev /* [Q][T][S] */, int32_t* flags_dev /* [Q][T] */);

/* ---------------------------------------------------------------- head identities with a constant-velocity motion model (additions to ABI 18;
 * nothing above changes)
 * mcg_track_heads_motion is mcg_track_heads with one thing more: a slot carries the velocity (vx, vy) of its box's centre, in pixels a frame,
 * and its box is moved by it before every frame's match.  A head that is missed for a few frames is then looked for where it has gone, and
 * the box of a coasting slot -- which mcg_live_slots / mcg_live_lanes cut the crop at -- follows the person.  The velocity is two f32 kept,
 * as bits, in reserved[0] (vx) and reserved[1] (vy) of the slot's mcg_track_slot: the state layout, mcg_track_state_bytes and every reader
 * of the state are as they were, and all zero bytes are still the empty state.  mcg_track_heads neither reads nor writes those words, so a
 * state may pass between the two entries; the plain entry leaves the velocities as it found them.  The launch shape (ONE launch, one
 * workgroup per sequence, no allocation, no host sync, graph-capturable), the limits, the argument checks and the six outputs are those of
 * mcg_track_heads; velocity_gain and coast_decay must each lie in [0, 1] (a NaN does not), else MCG_ERR_ARG before any launch.
 * THE ARITHMETIC, in terms of the numbered steps above.  Every operation is f32 and uncontracted; g = (float)velocity_gain,
 * k = (float)coast_decay.  Per sequence and per frame, in order:
 *  0. PREDICT.  For every live slot whose (vx, vy) is not (0, 0) -- compared as values: a -0 is a zero --:
 *       p = (x1 + vx, y1 + vy, x2 + vx, y2 + vy);  if the four are finite the slot's box is now p; otherwise the slot keeps its box and
 *       its velocity becomes (0, 0).  A slot with zero velocity is not touched at all (no + 0.0f): its box keeps its bits, negative zeros
 *       included.
 *  1 - 3 run exactly as they stand, on the predicted boxes.
 *  4. A MATCHED slot with predicted box p and detection d:
 *       rx = ((d.x1 + d.x2) - (p.x1 + p.x2)) * 0.5f, ry likewise in y;  vx = vx + g * rx, vy = vy + g * ry -- the product is rounded, then
 *       the sum;  if either is not finite, both become 0.  The slot takes d's box and age = 0, as above.
 *     An UNMATCHED live slot gets age += 1.  If age > max_age it is freed as above and its velocity becomes (0, 0).  Otherwise it KEEPS THE
 *     PREDICTED BOX -- the coasting box moves -- and its velocity becomes (vx * k, vy * k).
 *  5. Births as above, with velocity (0, 0): a slot freed in step 4 and born again in the same frame does not inherit a velocity.
 *  6. The six outputs as above.  state_boxes_dev, where not NULL, row s of frame (q, t): the slot's box after the frame -- the detection's
 *     for a slot matched or born, the predicted box for a coasting slot, zeros for a free one.
 * Consequences: with velocity_gain == 0 on a state whose velocity words are zero, every output and the state are mcg_track_heads', bit for
 * bit (no velocity ever leaves zero, and a slot at rest is not touched).  The result is a pure function of (state, boxes, counts, the
 * parameters): T frames in one call are T calls of one frame, and the velocity goes through the state words exactly.  The box SIZE has no
 * dynamics: a prediction moves the box and keeps its width and height.
 * velocity_gain = 0.5, coast_decay = 1.0 are what the Python layer defaults to: conventional alpha-beta values, not tuned on data.
 * mcgaze_amd/head_detect.py::track_heads_host(motion=...) is the same on the host, bit for bit. */
int mcg_track_heads_motion(mcg_stream s, const float* boxes_dev, long long frame_stride, const int32_t* counts_dev, int num_sequences,
                           int num_frames, int max_det, int slots, double match_iou, int max_age, double velocity_gain, double coast_decay,
                           void* state_dev, float* slot_boxes_dev /* [Q][T][S][4] */, int32_t* image_of_dev /* [Q][T][S] */,
                           int32_t* track_id_dev /* [Q][T][S] */, int32_t* age_dev /* [Q][T][S] */, int32_t* det_of_dev /* [Q][T][S] */,
                           int32_t* flags_dev /* [Q][T] */, float* state_boxes_dev /* [Q][T][S][4] or NULL */);

/* ---------------------------------------------------------------- live: tracker slots as streams (additions to ABI 18; nothing above changes)
 * mcg_track_heads decides on the device who is in which slot; the planning of a stream pool is a host function of how many frames each
 * stream was given.  So a live chain makes every slot of every camera a stream that gets ONE crop per tick, person or not, and decides on
 * the device, afterwards, which result rows belong to a person.  Two table kernels, one thread per row; no allocation, no host sync,
 * graph-capturable; the results are pure functions of the inputs and do not depend on launch geometry.  A TICK is one frame per camera;
 * ticks count from 0.  The identity RING keeps the last `ring_depth` ticks: tick t lives in ring row t % ring_depth.
 *
 * mcg_live_slots, after mcg_track_heads with one frame per camera: reads the tracker state of Q = num_cameras sequences of S = slots
 * (mcg_track_header + mcg_track_slot, the layout above) and writes, for every (q, s), row = q * S + s:
 *   a LIVE slot (id > 0, matched or coasting):  crop_boxes[row] = slot.box, image_of[row] = q      -- a coasting slot's box is its last match,
 *                                                                                                     or what mcg_track_heads_motion predicted
 *   a FREE slot:                                crop_boxes[row] = 0 0 0 0,  image_of[row] = -1     -- the row the head-crop entries flag 2
 *   ring_id[tick % R][q][s] = the slot's id or 0;  ring_box[tick % R][q][s] = crop_boxes[row];  matched[q][s] = (id > 0 and age == 0)
 * crop_boxes / image_of are the tables of mcg_preprocess_head_crops over the Q frames of the tick.
 *   state_dev DEVICE, 16-byte aligned, mcg_track_state_bytes(Q, S) bytes, read only
 *   crop_boxes_dev [Q][S][4] f32, image_of_dev [Q][S] int32, matched_dev [Q][S] int32, ring_id_dev [R][Q][S] int32, ring_box_dev [R][Q][S][4] f32
 * num_cameras in 0 .. 65535 (0: MCG_OK without a launch); slots outside 1 .. 64, tick < 0, ring_depth outside 1 .. 65536, a null pointer
 * or a misaligned state return MCG_ERR_ARG before any launch.
 *
 * mcg_live_gate: which result rows are a person.  The slots run in lockstep, so ONE host-built table serves all of them: entry e is five
 * int32 (tick, lo, hi, prev, next) -- the tick of a frame, [lo, hi) the union of the ticks of every window that covered the frame in the
 * overlap merge, prev / next the ticks the temporal filter read for it or -1.  Entries first_out .. first_out + num_out - 1 are the frames
 * handed out, in order; the other entries are there as neighbours only.  `tick` is the newest tick mcg_live_slots wrote.
 *   entry e is USABLE iff  tick - R < e.tick <= tick,  0 <= e.lo <= e.hi <= tick + 1,  e.hi - e.lo <= R,  e.lo > tick - R where hi > lo,
 *                          e.prev >= -1 and e.next >= -1     -- so every t it names has its ring row: an index is never an address
 *   id(e, q, s)    = e usable ? ring_id[e.tick % R][q][s] : 0
 *   valid(e, q, s) = id != 0 and ring_id[t % R][q][s] == id for every t in [e.lo, e.hi)
 *        -- a row is a person's only if every frame of every window merged into it was a crop of that person
 * Per output row (i, q, s), e = first_out + i:
 *   track_id = id(e);  valid = valid(e);  head_box = valid ? ring_box[e.tick % R][q][s] : 0 0 0 0;  image_of = valid ? i * Q + q : -1
 *        -- image_of is the row table of the arrow entries over the num_out * Q frames handed out, frame (i, q) at i * Q + q: an invalid
 *           row has no image and is skipped there (a zero box alone would still be drawn, as a dot at the origin)
 *   with smoothing (fused_smooth_dev given):  a neighbour tick n in (e.prev, e.next) that is not -1 is GOOD iff some entry j has j.tick == n
 *        (the first such j) and valid(j, q, s) and id(j, q, s) == id(e, q, s);
 *        smooth_valid = valid and every neighbour that is not -1 is good;
 *        where valid and not smooth_valid, row (i, q, s) of fused_smooth / others_smooth is REPLACED by the same row of fused / others;
 *        every other row of them keeps its bits.  fused / others (and the detections) are never written: the masks say what they are.
 *   table_dev DEVICE int32 [num_entries][5];  ring_id_dev, ring_box_dev as mcg_live_slots wrote them
 *   fused_dev [num_out][Q][S][3], others_dev [num_out][Q][S][9] f32 (read), fused_smooth_dev, others_smooth_dev the same shapes (updated in
 *   place): all four given, or all four NULL (no smoothing; smooth_valid_dev may then be NULL too)
 *   track_id_dev, valid_dev, image_of_dev, smooth_valid_dev [num_out][Q][S] int32, head_box_dev [num_out][Q][S][4] f32: written in full
 * num_out = 0 or num_cameras = 0 returns MCG_OK without a launch.  slots outside 1 .. 64, num_cameras outside 0 .. 65535, ring_depth
 * outside 1 .. 65536, tick < 0, num_entries outside 0 .. 65536, first_out < 0, num_out < 0, first_out + num_out > num_entries,
 * num_out * Q * S >= 2^31, a null pointer or smoothing pointers given in part return MCG_ERR_ARG before any launch.
 * mcgaze_amd/live.py::live_slots_host and live_gate_host are the same on the host, bit for bit. */
int mcg_live_slots(mcg_stream s, const void* state_dev, int num_cameras, int slots, int tick, int ring_depth, float* crop_boxes_dev,
                   int32_t* image_of_dev, int32_t* ring_id_dev, float* ring_box_dev, int32_t* matched_dev);
int mcg_live_gate(mcg_stream s, const int32_t* ring_id_dev, const float* ring_box_dev, int ring_depth, int num_cameras, int slots, int tick,
                  const int32_t* table_dev, int num_entries, int first_out, int num_out, const float* fused_dev, const float* others_dev,
                  float* fused_smooth_dev, float* others_smooth_dev, int32_t* track_id_dev, int32_t* valid_dev, float* head_box_dev,
                  int32_t* image_of_dev, int32_t* smooth_valid_dev);

/* ---------------------------------------------------------------- live: occupied slots compacted into lanes (additions to ABI 18; nothing above changes)
 * The fixed schedule above sends all Q * S slots through the network every tick.  A slot table is sized for the worst case per camera; the
 * people present at once over all cameras are far fewer.  So a pool gets a fixed number P = `lanes` of streams, and which live slot holds
 * which LANE is decided on the device, each tick.  A person keeps the lane for as long as they keep the slot, so a lane is a contiguous
 * stream of one person's crops, and the ring-of-ids gate decides validity as above, over P ring columns.  Host work per tick is the same
 * whoever is in the picture; no allocation, no host sync, graph-capturable; the results are pure functions of the inputs and do not depend
 * on launch geometry or scheduling.  COLUMN = q * S + s names a slot.
 *
 * mcg_live_lanes, after mcg_track_heads with one frame per camera: ONE launch of ONE workgroup.
 *   lane_state_dev DEVICE int32 [P][2] = (id, column) per lane, read and updated in place.  A lane is FREE iff id == 0: all zero bytes are
 *   "every lane free".  id(c) below is the id of the tracker slot at column c after the tick's frame; the slot is live iff id(c) > 0.
 *   1. RELEASE.  Lane p = (id, column) stays HELD iff id > 0, 0 <= column < Q * S, id(column) == id, and no lane below p is held with the
 *      same column (a state no call leaves behind; the lowest lane keeps the slot).  Every other lane becomes free: a freed slot, a slot
 *      handed to another person, a column out of range.  The column is range-checked before it is used as an index.
 *   2. ASSIGN.  The WAITING slots are the live slots no held lane names, in ascending column order; the free lanes are taken in ascending
 *      lane order, those released in step 1 included.  The k-th waiting slot takes the k-th free lane: lane = (id(c), c).  Waiting slots
 *      beyond the number of free lanes get no lane in this tick and wait again in the next, by the same rule.  Ranks come from ballots and
 *      prefix sums over ascending indices, so the order does not depend on timing.
 *   3. OUTPUTS, lane p, ring row r = tick % R:
 *        held by (id, c):  lane_state[p] = id, c;  crop_boxes[p] = box of slot c (matched or coasting);  image_of[p] = c / S;
 *                          ring_id[r][p] = id;  ring_col[r][p] = c;  ring_box[r][p] = crop_boxes[p];  matched[p] = (age of slot c == 0)
 *        free:             lane_state[p] = 0, 0;  crop_boxes[p] = 0 0 0 0;  image_of[p] = -1  -- the row the head-crop entries flag 2;
 *                          ring_id[r][p] = 0;  ring_col[r][p] = -1;  ring_box[r][p] = 0 0 0 0;  matched[p] = 0
 *      lane_of[q][s] = the lane that holds slot (q, s), or -1: the slot is free, or live and left out.
 *      overflow[0] = max(0, waiting slots - free lanes): the live slots left without a lane in this tick.
 *   state_dev DEVICE, 16-byte aligned, mcg_track_state_bytes(Q, S) bytes, read only
 *   crop_boxes_dev [P][4] f32, image_of_dev [P], matched_dev [P] int32, ring_id_dev, ring_col_dev [R][P] int32, ring_box_dev [R][P][4] f32,
 *   lane_of_dev [Q][S] int32, overflow_dev [1] int32: written in full (of the rings, row tick % R)
 * num_cameras in 0 .. 65535 with Q * S <= 4096 (0 cameras: MCG_OK without a launch); lanes outside 1 .. 1024, slots outside 1 .. 64,
 * tick < 0, ring_depth outside 1 .. 65536, a null pointer or a misaligned state return MCG_ERR_ARG before any launch.  Every index into
 * global memory is a thread index below a checked bound, or a column that was range-checked.
 *
 * mcg_live_gate_lanes: mcg_live_gate over lanes, with the same table (tick, lo, hi, prev, next), the same USABLE rule and `tick`.
 * Ids are per camera, so a lane's identity is the pair (ring_id, ring_col):
 *   id(e, p)    = e usable ? ring_id[e.tick % R][p] : 0;   col(e, p) = e usable ? ring_col[e.tick % R][p] : -1
 *   valid(e, p) = id != 0 and ring_id[t % R][p] == id and ring_col[t % R][p] == col for every t in [e.lo, e.hi)
 * Per output row (i, p), e = first_out + i:
 *   track_id = id(e);  valid = valid(e);  head_box = valid ? ring_box[e.tick % R][p] : 0 0 0 0
 *   where valid and 0 <= col < Q * S:  camera = col / S, slot = col % S, image_of = i * Q + camera;  everywhere else all three are -1
 *   with smoothing: a neighbour tick n is GOOD iff the first entry j with j.tick == n has valid(j, p), id(j, p) == id(e, p) and
 *        col(j, p) == col(e, p);  smooth_valid and the replacement of rows of fused_smooth / others_smooth are those of mcg_live_gate.
 *   ring_col_dev [R][P] as mcg_live_lanes wrote it;  fused_dev [num_out][P][3], others_dev [num_out][P][9] and the smoothed tables: all
 *   four or none;  track_id_dev, valid_dev, camera_dev, slot_dev, image_of_dev, smooth_valid_dev [num_out][P] int32, head_box_dev
 *   [num_out][P][4] f32: written in full
 * num_out = 0 or num_cameras = 0 returns MCG_OK without a launch.  lanes outside 1 .. 1024, slots outside 1 .. 64, num_cameras outside
 * 0 .. 65535, Q * S > 4096, ring_depth outside 1 .. 65536, tick < 0, num_entries outside 0 .. 65536, first_out < 0, num_out < 0,
 * first_out + num_out > num_entries, num_out * P >= 2^31, a null pointer or smoothing pointers given in part return MCG_ERR_ARG before any
 * launch.  mcgaze_amd/live.py::live_lanes_host and live_gate_lanes_host are the same on the host, bit for bit. */
int mcg_live_lanes(mcg_stream s, const void* state_dev, int num_cameras, int slots, int lanes, int tick, int ring_depth,
                   int32_t* lane_state_dev, float* crop_boxes_dev, int32_t* image_of_dev, int32_t* ring_id_dev, float* ring_box_dev,
                   int32_t* ring_col_dev, int32_t* lane_of_dev, int32_t* matched_dev, int32_t* overflow_dev);
int mcg_live_gate_lanes(mcg_stream s, const int32_t* ring_id_dev, const float* ring_box_dev, const int32_t* ring_col_dev, int ring_depth,
                        int num_cameras, int slots, int lanes, int tick, const int32_t* table_dev, int num_entries, int first_out, int num_out,
                        const float* fused_dev, const float* others_dev, float* fused_smooth_dev, float* others_smooth_dev,
                        int32_t* track_id_dev, int32_t* valid_dev, int32_t* camera_dev, int32_t* slot_dev, float* head_box_dev,
                        int32_t* image_of_dev, int32_t* smooth_valid_dev);

/* ---------------------------------------------------------------- gaze targets (additions to ABI 18; nothing above changes)
 * What each head looks at: another head of its picture (and whether that head looks back), a rectangle marked in the picture, the lens, or
 * nothing.  The reference stops at the arrow (MCGaze_demo/demo.ipynb, cell 5: from the head's centre towards centre - l * gaze[:2]);
 * mcg_gaze_targets follows THAT ray until it meets something.  Targets are decided in the IMAGE PLANE: no camera intrinsics, no depth.
 * Two launches (one thread per row; then `mutual`, which needs every target), no allocation, no host sync, graph-capturable.
 * Everything is double and uncontracted (no FMA), every product, quotient and sum rounded on its own; inputs are read as f32 and widened,
 * as the arrow plan does.  min / max below never see a NaN.
 * INPUTS.  Rows: boxes [n][4] x1 y1 x2 y2, gaze (gx, gy, gz) at gaze_dev + i * gaze_stride, image_of [n]: rows with equal image_of are in
 * one picture.  Regions: regions [m][4] rectangles and region_image [m].  Region j APPLIES to row i iff region_image[j] < 0 (every
 * picture), or region_period == 0 and region_image[j] == image_of[i], or region_period > 0 and region_image[j] == image_of[i] %
 * region_period (LiveGaze numbers the pictures of a call i * Q + camera: region_period = Q gives regions per camera).
 * UNUSABLE.  A row is unusable (flag 2) iff one of its four box values or three gaze values is not finite, or x2 < x1, or y2 < y1, or
 * image_of < 0.  It gets kind 0, target -1 and zeros elsewhere; it looks at nothing and nothing looks at it.  A region that is not finite
 * or inverted is never hit and flags nothing.  Every other row has flag 0.
 * CAMERA.  A usable row has kind 3 iff gz < 0 and gz * gz >= camera_cos2 * ((gx * gx + gy * gy) + gz * gz): -z is towards the lens
 * (mcgaze_amd/metric.py::vector_to_yaw_pitch), camera_cos2 = cos(angle)^2 of the cone's half angle; a camera_cos2 above 1 never holds.
 * This test comes before everything below.
 * RAY.  o = ((x1 + x2) * 0.5, (y1 + y2) * 0.5), d = (-gx, -gy): the arrow's direction from the box's REAL centre -- not the arrow's own
 * start, which the plan above truncates to whole pixels.  If both components of d compare equal to zero the kind is 0.
 * CANDIDATES.  Every OTHER usable row of the same picture, its box grown on each side by e = expand * max(x2 - x1, y2 - y1):
 * [x1 - e, x2 + e] x [y1 - e, y2 + e]; and every usable region that applies, as it is.
 * SLAB TEST of a rectangle [lo_x, hi_x] x [lo_y, hi_y].  An axis a with d_a == 0 (+0 or -0) passes iff lo_a <= o_a <= hi_a and gives no
 * bound.  Otherwise t1 = (lo_a - o_a) / d_a, t2 = (hi_a - o_a) / d_a; near = max over such axes of min(t1, t2), far = min over them of
 * max(t1, t2) (one axis: its own pair).  A hit iff every axis passes, near <= far and far >= 0; the entry is t = near if near > 0 else +0
 * -- 0 when o lies inside.  A hit whose t is not finite is a miss.
 * CHOICE.  The smallest t wins; on equal t a head comes before a region, then the lower index.  Kind 1 (head: target = its row index) or 2
 * (region: target = its index), else kind 0.
 * OUTPUTS, per row: kind int32 (0 none, 1 head, 2 region, 3 camera), target int32 (-1 unless kind is 1 or 2), t f32 -- the double rounded
 * once --, hit [n][2] f32 = o + t * d per component (product and sum each rounded in double, then once to f32), mutual int32, flags int32.
 * t and hit are 0 unless kind is 1 or 2.  mutual[i] = 1 iff kind[i] == 1 and, with r = target[i], kind[r] == 1 and target[r] == i.
 * The result is a function of the inputs alone, whatever the launch geometry.
 *   boxes_dev, image_of_dev, regions_dev, region_image_dev   DEVICE f32 [n][4], int32 [n], f32 [m][4], int32 [m]; the region tables may be
 *                NULL iff m == 0
 *   gaze_dev     DEVICE f32, row i at gaze_dev + i * gaze_stride (floats, >= 3) -- the [n][3] fused gaze as it is
 *   expand       finite, >= 0 (Python default 0.25);  camera_cos2 not NaN (Python: cos(10 degrees)^2; 2.0 switches the test off).  Both
 *                defaults are CONVENTIONS, not tuned on data.
 *   kind_dev .. flags_dev   DEVICE, written: int32 [n], int32 [n], f32 [n], f32 [n][2], int32 [n], int32 [n]
 * 0 <= n <= 65536, 0 <= m <= 4096, region_period >= 0; n == 0 returns MCG_OK without a launch.  A wrong count, stride or parameter or a
 * null pointer returns MCG_ERR_ARG before any launch; the CONTENTS of the device tables never are an error, are never read back, and
 * whatever they hold nothing outside the given arrays is read or written.  Heads are searched in tiles of 256 rows and a tile whose
 * image_of range holds no picture a workgroup asks about is skipped: tables whose pictures come in ascending row order (LiveGaze's
 * [k, Q, S]) cost one picture per row.  mcgaze_amd/attention.py::gaze_targets_host is the same on the host, bit for bit.
 * Out of scope: camera intrinsics or depth, arrows cut at the hit point.  (Coloured arrows: "attention overlay" below.  How long a target is looked at: "gaze dwell" below;
 * regions that are polygons: "gaze targets, polygonal regions" below.) */
int mcg_gaze_targets(mcg_stream s, const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n,
                     const float* regions_dev, const int32_t* region_image_dev, int m, int region_period, double expand, double camera_cos2,
                     int32_t* kind_dev, int32_t* target_dev, float* t_dev, float* hit_dev, int32_t* mutual_dev, int32_t* flags_dev);

/* ---------------------------------------------------------------- gaze dwell (additions to ABI 19; nothing above changes)
 * How long each person looks at what: the per-frame targets of mcg_gaze_targets, which flicker, become debounced EPISODES -- a target, a
 * start, a length, an end and why it ended -- and every region collects its person-frames.  mcg_gaze_dwell walks F frames of R COLUMNS (a
 * column is a tracker slot or a lane) in frame order, one thread per column, with a 16-word state record per column that the caller keeps
 * between calls: the caller reads nothing back per tick and keeps no state per person.  A second launch compacts the episodes that ended
 * into an event table.  No allocation, no host sync, graph-capturable; the result is a function of the inputs alone.
 * ARITHMETIC.  Everything is int32.  Every sum below (`+=`, and n = frame0 + f) is computed UNSIGNED, modulo 2^32, and stored back as
 * int32; the two comparisons `gap > exit` and `cand_frames >= enter` compare the stored int32 values, signed.  So whatever the tables
 * and the state hold nothing overflows, and nothing outside the given arrays is read or written.
 * INPUTS, each [F][R] int32; frame f has the number n = frame0 + f.
 *   person   > 0: the id of the person with a usable result in that column and frame; <= 0: nobody
 *   tag      the second half of the identity (ids are per camera: LiveGaze's lanes pass the ring column); NULL: all zero
 *   kind, ident, mutual   what the person looks at: kind in mcg_gaze_targets' values, ident the identity of the target -- the Python
 *            layer passes the looked-at person's track id for a head (stable over frames where the slot is not) and the region's index
 *            for a region --, mutual as mcg_gaze_targets writes it
 *   enter >= 1: the consecutive frames an observation must repeat before it becomes the current target;  exit >= 0: the consecutive
 *   frames the current target may go unobserved before its episode ends.  (Python defaults 3 and 2: CONVENTIONS, not tuned on data.)
 * OBSERVATION, normalised: a kind outside 1 .. 3 gives (k, i) = (0, 0); kind 3 gives (3, 0); otherwise (kind, ident).  m = 1 iff k == 1
 * and mutual != 0, else 0.
 * STATE, per column 16 int32 words, read and updated in place; all zero is the empty state:
 *   0 person  1 tag  2 cur_kind  3 cur_ident  4 cur_start  5 cur_frames  6 cur_mutual  7 gap
 *   8 cand_kind  9 cand_ident  10 cand_start  11 cand_frames  12 cand_mutual  13 seen  14, 15 reserved, written 0
 * An episode that is still open is (words 0 .. 6) of a record whose cur_kind != 0: the kernel does not flush it, the layout is public.
 * PER FRAME AND COLUMN, in this order.  END(reason) records (person, tag, cur_kind, cur_ident, cur_start, cur_frames, cur_mutual, reason)
 * of the state as it stands, as this row of `ended`.
 *   A. OWNER.  p = person > 0 ? person : 0;  g = p ? tag : 0.  If state.person != 0 and (state.person, state.tag) != (p, g): when
 *      cur_kind != 0, END(2: the owner left); then all 16 words become zero.  If p == 0 the step is done: the row of `dwell` is zero
 *      (the row of `ended` holds the END of the line before, if there was one).  Otherwise (state.person, state.tag) = (p, g).
 *   B. seen += 1.  If k == 2 and 0 <= i < M: region_frames[i] += 1 -- RAW person-frames, before any debouncing; an integer atomic, so
 *      the sum does not depend on the order; the index is range-checked before it is used.
 *   C. CURRENT.  If cur_kind != 0: if (k, i) == (cur_kind, cur_ident): cur_frames += 1 + gap (the bridged frames count), gap = 0,
 *      cur_mutual += m, and the five cand_ words become zero.  Otherwise gap += 1, and if gap > exit: END(1: looked away) -- cur_frames
 *      as it stands, the trailing gap not counted --, then the five cur_ words and gap become zero.
 *   D. CANDIDATE, unless C found the observation to be the current target.  If k == 0 the five cand_ words become zero.  Else if
 *      (k, i) == (cand_kind, cand_ident): cand_frames += 1, cand_mutual += m.  Else the candidate becomes (k, i) with cand_start = n,
 *      cand_frames = 1, cand_mutual = m.  Then, if cand_frames >= enter: when cur_kind != 0, END(3: replaced); the five cur_ words take
 *      the five cand_ words, gap = 0, the five cand_ words become zero.
 *   E. OUTPUTS.  dwell [F][R][4] = (cur_kind, cur_ident, cur_start, cur_frames) after the step (zero where p == 0);
 *      ended [F][R][8] = the END of this step, else all zero.  A reason is never 0, so an END row is never all zero.
 * AT MOST ONE END happens per row and frame: A zeroes the record, so C and D find cur_kind == 0 behind an END(2); C clears cur_kind
 * with its END(1), so D's END(3), which needs cur_kind != 0, cannot follow it.
 * EVENTS.  With events_dev given a second launch (one workgroup) compacts the non-zero rows of `ended` into events [E][10] = (frame
 * number n, column, the 8 words), in ascending (frame, column) order -- ranks from ballots and prefix sums over ascending rows, never from
 * timing.  num_events[0] = the number of non-zero rows of this call; rows beyond E are dropped and still counted, so the caller sees the
 * overflow; rows of `events` behind the count are left as they were.  events_dev == NULL (then E must be 0) skips the launch and
 * writes no count.
 *   person_dev .. mutual_dev   DEVICE int32 [F][R], read only; tag_dev may be NULL
 *   state_dev    DEVICE int32 [R][16], 16-byte aligned, updated in place
 *   region_frames_dev   DEVICE int32 [M], accumulated in place; NULL iff M == 0
 *   dwell_dev, ended_dev   DEVICE int32 [F][R][4] and [F][R][8], 16-byte aligned, written in full
 *   events_dev, num_events_dev   DEVICE int32 [E][10] (8-byte aligned) and [1]; both or neither
 * 1 <= R <= 4096, F >= 0 with F * R <= 65536 (F == 0 returns MCG_OK without a launch and writes nothing), 0 <= M <= 4096,
 * 0 <= E <= 65536, frame0 >= 0, 1 <= enter <= 65536, 0 <= exit <= 65536.  A wrong count or parameter, a null pointer or a misaligned
 * table returns MCG_ERR_ARG before any launch; the CONTENTS of the tables and of the state never are an error.
 * mcgaze_amd/attention.py::gaze_dwell_host is the same on the host, bit for bit.
 * (A polygonal region of mcg_gaze_targets_poly is a region index like any other.)
 * Out of scope: camera intrinsics or depth, re-identifying a person who comes back after the tracker's max_age (a new id is a new
 * owner). */
int mcg_gaze_dwell(mcg_stream s, const int32_t* person_dev, const int32_t* tag_dev, const int32_t* kind_dev, const int32_t* ident_dev,
                   const int32_t* mutual_dev, int num_frames, int columns, int frame0, int enter, int exit_frames, int32_t* state_dev,
                   int32_t* region_frames_dev, int num_regions, int32_t* dwell_dev, int32_t* ended_dev, int32_t* events_dev, int max_events,
                   int32_t* num_events_dev);

/* ---------------------------------------------------------------- gaze targets, polygonal regions (additions to ABI 19; nothing above changes)
 * A marked region is rarely a rectangle in the picture: a screen seen off-axis is a quadrilateral, a shelf beside a pillar an L.
 * mcg_gaze_targets_poly is mcg_gaze_targets with regions that are rectangles OR polygons.  Rows, UNUSABLE, CAMERA, RAY, the head
 * candidates, CHOICE and OUTPUTS are word for word those of "gaze targets" above; only the regions differ.  Two launches, no allocation,
 * no host sync, graph-capturable, no atomics in global memory.
 * TABLES.  region_xy f32 [V][2] vertices (x, y), region_start int32 [m + 1], region_image int32 [m] (as above, with region_period).  Region
 * j owns the vertices region_start[j] .. region_start[j + 1] - 1; c is their number.
 * USABLE REGION.  Region j is usable iff 0 <= region_start[j] <= region_start[j + 1] <= V, and c == 2 or 3 <= c <= 32
 * (MCG_ATTEND_POLY_VERTS), and every coordinate it owns is finite, and for c == 2 neither x2 < x1 nor y2 < y1.  Any other region is never
 * hit and flags nothing, as a bad rectangle above.  The tables are device contents and their contents never are an error: whatever
 * region_start holds, nothing outside region_xy[0 .. V) is read -- the offsets are checked before the first vertex load.
 * c == 2.  The two vertices are (x1, y1) and (x2, y2) of a rectangle, tested by the SLAB TEST above unchanged: a table of only such regions
 * gives the bits of mcg_gaze_targets.
 * c >= 3.  Edge k runs from a = v_k to b = v_((k + 1) mod c), k ascending.  Everything is double and uncontracted; every product, quotient
 * and sum is rounded on its own.
 *   INSIDE (even-odd rule).  Edge k toggles iff (a_y > o_y) != (b_y > o_y) and o_x < a_x + ((o_y - a_y) * (b_x - a_x)) / (b_y - a_y).  An
 *   odd number of toggles is a hit with t = +0.
 *   CROSSINGS, otherwise.  e = b - a, w = a - o;  den = d_x * e_y - d_y * e_x,  tn = w_x * e_y - w_y * e_x,  sn = w_x * d_y - w_y * d_x.  The
 *   edge is crossed iff (den > 0 and tn >= 0 and sn >= 0 and sn <= den) or (den < 0 and tn <= 0 and sn <= 0 and sn >= den): no division
 *   in the decision.  With q = tn / den its t is q if q > 0, else +0; a t that is not finite is no crossing.  The region's t is the smallest
 *   over its crossed edges; with no crossed edge it is a miss.
 *   A parallel edge (den == 0) gives nothing by itself: its end points belong to its neighbours.  Self-intersecting and zero-area polygons
 *   are whatever these rules give.  Winding does not matter.
 * CHOICE is unchanged: the smallest t wins; on equal t a head comes before a region, then the lower index.  Rectangles and polygons share
 * one index space, in the caller's order.
 *   region_xy_dev      DEVICE f32 [V][2]; NULL iff V == 0
 *   region_start_dev, region_image_dev   DEVICE int32 [m + 1] and int32 [m]; NULL iff m == 0
 *   every other argument as mcg_gaze_targets takes it
 * 0 <= n <= 65536, 0 <= m <= 4096, 0 <= V = num_vertices <= 65536; n == 0 returns MCG_OK without a launch.  A count outside these or a
 * null table returns MCG_ERR_ARG before any launch.  The regions are searched in tiles of 256 with the picture-range skip of the heads; a
 * polygon's vertices are read through an address that is the same in every thread of the workgroup.  No bounding-box reject: every edge
 * is tested.  mcgaze_amd/attention.py::gaze_targets_host(region_start=...) is the same on the host, bit for bit.
 * Out of scope: arrows cut at the hit point, camera intrinsics or depth.  (Region outlines and coloured arrows: "attention overlay" below.) */
#define MCG_ATTEND_POLY_VERTS 32
int mcg_gaze_targets_poly(mcg_stream s, const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n,
                          const float* region_xy_dev, int num_vertices, const int32_t* region_start_dev, const int32_t* region_image_dev, int m,
                          int region_period, double expand, double camera_cos2, int32_t* kind_dev, int32_t* target_dev, float* t_dev,
                          float* hit_dev, int32_t* mutual_dev, int32_t* flags_dev);

/* ---------------------------------------------------------------- attention overlay (additions to ABI 19; nothing above changes)
 * What "gaze targets" found, drawn where it was found: the outlines of the marked regions (lit where somebody looks at them), a sight line
 * from every head to the point its look landed on, and the arrows of "annotated frames out" coloured by what they point at -- IN PLACE into
 * packed BGR frames (mcg_draw_attention) or NV12 surfaces (mcg_draw_attention_nv12), from tables that are all in device memory: the frame
 * table and rows of mcg_draw_gaze_arrows, kind / target / hit / mutual as mcg_gaze_targets(_poly) writes them, and the region tables of
 * mcg_gaze_targets_poly (a rectangle is a 2-vertex region).  Three launches (region_active cleared; a plan kernel, double and uncontracted;
 * a gather kernel over (image, pixel tile)), no allocation, no host sync, graph-capturable, no atomics.
 * STROKES.  Every stroke is a set of segments of one thickness t under COVERAGE of "annotated frames out" (the capsule test in 64-bit
 * integers; every end point within [-8191, 8191], frames of at most 8192 a side, t <= 255).  The strokes of a call are numbered: region j
 * is stroke j, the sight line of row k stroke m + k, the arrow of row k stroke m + n + k -- three LAYERS, low to high, ascending index in
 * each.  A pixel takes the colour of the HIGHEST-numbered stroke that covers it, whatever the launch geometry; a pixel no stroke covers is
 * not written.  Each layer may be empty, and a thickness of 0 switches its layer off (nothing of it is drawn; flags, region_flags and
 * region_active are written as ever).
 * 1. REGION OUTLINES.  Region j is usable iff it is a USABLE REGION of "gaze targets, polygonal regions" (offsets checked before the first
 * vertex load; c == 2 or 3 <= c <= 32; every coordinate finite; a rectangle not inverted) AND every rounded coordinate rint((double)x)
 * (half to even) lies in [-8191, 8191].  Otherwise region_flags[j] = 2, nothing is drawn for it and nothing outside region_xy[0 .. V) is
 * read: what the tables hold is never an error.  The corners of a rectangle are (x1, y1) (x2, y1) (x2, y2) (x1, y2), those of a polygon
 * its vertices, all rounded; the outline is the c edges v[k] -> v[(k + 1) % c] (4 for a rectangle) with t = region_thickness.  It is drawn
 * into picture p iff region_image[j] < 0, or == p, or region_period > 0 and == p % region_period.  Its pixels are bounded by the h, w of
 * the picture drawn into (one region may apply to pictures of different sizes).
 * region_active[p][j] = 1 iff some row k has image_of[k] == p, kind[k] == 2 and target[k] == j (whatever the row's flag), else 0; it is
 * written for every (p, j), drawable or not.  The outline's colour in picture p is palette[6] where region_active[p][j], else palette[5].
 * 2. SIGHT LINES.  Row k gets one iff its arrow is drawable (flags[k] == 0), kind[k] is 1 or 2, and hx = rint((double)hit[k][0]),
 * hy = rint((double)hit[k][1]) are finite and in [-8191, 8191]: one segment from the arrow plan's centre (cx, cy) to (hx, hy) with
 * t = line_thickness, in the row's colour.  A row that fails only the hit test keeps its arrow.  target[k] is read only where kind[k] == 2.
 * 3. ARROWS.  The ARROW PLAN, HEAD STROKES and FLAGS of "annotated frames out", term for term; flags[k] is that flag.  min_thickness == 0
 * switches the layer off: the plan is then made with a minimum of 0 and serves the flags and the sight lines only.
 * The row's colour is palette[mutual[k] != 0 ? 4 : (1 <= kind[k] <= 3 ? kind[k] : 0)]: any other kind word is "none".
 * NV12 follows "annotated frames out": every covered luma pixel gets the Y of ITS highest stroke; a chroma pair is written iff any of its
 * four luma pixels is covered, with the (U, V) of the highest stroke among the four.
 * ANCHOR.  With m == 0, kind all zero and palette[0] = color the call writes the bytes and flags of mcg_draw_gaze_arrows(_nv12).
 *   images_dev, num_images, max_h, max_w, boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, length, thickness_ratio, tip_length: as
 *                mcg_draw_gaze_arrows takes them; an image that is not writable or larger than (max_h, max_w) gets no stroke at all
 *   kind_dev, target_dev, mutual_dev DEVICE int32 [n];  hit_dev DEVICE f32 [n][2]
 *   region_xy_dev DEVICE f32 [V][2] (NULL iff V == 0);  region_start_dev int32 [m + 1], region_image_dev int32 [m] (NULL iff m == 0)
 *   palette      HOST uint8 [7][3]: B, G, R (NV12: Y, U, V) of none, head, region, camera, mutual, region outline, region outline looked at
 *   min_thickness, line_thickness, region_thickness: each 0 .. 255
 *   workspace_dev DEVICE, written: the plan -- (m + 2 n) mcg_stroke_desc in stroke order, then the rounded vertices int32 [m][32][2];
 *                workspace_bytes >= 96 * (m + 2 n) + 256 * m
 *   flags_dev DEVICE int32 [n];  region_flags_dev DEVICE int32 [m];  region_active_dev DEVICE int32 [num_images][m]  (all written)
 * n <= 65535, m <= 4096, V <= 65536, num_images * m <= 2^20, frames of at most 8192 a side: anything else, a null table or a workspace too
 * small returns MCG_ERR_ARG before any launch; n == 0 and m == 0 returns MCG_OK without one.  No byte outside [0, h) x [0, w) of any plane
 * is touched, padding included, for ANY table contents.  Every wave of the gather grid reads the plan in (m + 2 n) / 64 slices, and a large
 * region's box covers many tiles that each test up to 32 capsules per pixel: made for the tens of heads and regions of a video frame.
 * mcgaze_amd/arrows.py::draw_attention_host is the same on the host, bit for bit.  Out of scope: arrows cut at the hit point, filled
 * regions.  (Text: "text labels" below.) */
typedef struct mcg_stroke_desc {
  int seg[3][2][2];         /* a sight line: seg[0]; an arrow: shaft, stroke, stroke -- (from, to) x (x, y); a region: unused (its vertices follow the plan) */
  int thickness;
  int x0, y0, x1, y1;       /* bounding box of the covered pixels, half open; a row's is clipped to its frame, a region's only at 0 */
  int image, flag;          /* a row: image_of; a region: region_image.  flag 0: drawn; 2: not */
  int layer, count;         /* 0 region outline, 1 sight line, 2 arrow; the number of corners (layer 0) or segments */
  unsigned color, color_active;   /* c0 | c1 << 8 | c2 << 16; color_active: a region outline that is looked at */
  int reserved;
} mcg_stroke_desc;
int mcg_draw_attention(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                       const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n, const int32_t* kind_dev, const int32_t* target_dev,
                       const float* hit_dev, const int32_t* mutual_dev, const float* region_xy_dev, int num_vertices,
                       const int32_t* region_start_dev, const int32_t* region_image_dev, int m, int region_period, const unsigned char* palette,
                       double length, int min_thickness, double thickness_ratio, double tip_length, int line_thickness, int region_thickness,
                       void* workspace_dev, size_t workspace_bytes, int32_t* flags_dev, int32_t* region_flags_dev, int32_t* region_active_dev);
int mcg_draw_attention_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                            const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n, const int32_t* kind_dev,
                            const int32_t* target_dev, const float* hit_dev, const int32_t* mutual_dev, const float* region_xy_dev, int num_vertices,
                            const int32_t* region_start_dev, const int32_t* region_image_dev, int m, int region_period, const unsigned char* palette,
                            double length, int min_thickness, double thickness_ratio, double tip_length, int line_thickness, int region_thickness,
                            void* workspace_dev, size_t workspace_bytes, int32_t* flags_dev, int32_t* region_flags_dev, int32_t* region_active_dev);

/* ---------------------------------------------------------------- text labels (additions to ABI 19; nothing above changes)
 * Words on the frame: '#12 3.4s' next to a head, 'SHELF A' in a region -- drawn IN PLACE into packed BGR frames (mcg_draw_labels) or NV12
 * surfaces (mcg_draw_labels_nv12) from tables that are all in device memory.  The library holds NO font: font_dev is a DEVICE uint8 [96][8]
 * table for the codes 32 .. 126 and one spare entry, one byte per glyph row, bit c (from the least significant) the glyph's column c from
 * the left -- any 8-row bitmap font (mcgaze_amd/arrows.py::LABEL_FONT is a 5 x 7 one drawn for this project).
 * TEXT.  A row's text is MCG_LABEL_CHARS = 24 bytes; its length len is the index of its first zero byte, 24 if there is none.
 * mcg_format_labels writes such rows, one launch, one thread per row, 24 bytes each: id <= 0 gives all zeros; otherwise '#' decimal(id), and
 * where value_dev is given and value > 0, with q = (int64)value * 10 * den / num (a floor), ' ' decimal(q / 10) '.' ('0' + q % 10) 's' --
 * the seconds of `value` frames at num / den frames per second, in tenths, never rounded up; the rest of the row is zero.
 * 1 <= den <= num <= 2^20 is required: then q / 10 <= value, and every text of at most 24 characters is written whole.  The one longer
 * text has 25: an id of ten digits with a seconds part of ten digits (value >= 10^9 frames at a rate below 2.15 frames per second); it is
 * cut after 24 bytes, losing its 's'.  Nothing is ever written outside the row.
 * PLAN, per row k (one thread per row; coordinates f32 widened to double, then integers).  USABLE: image_of in [0, num_images); the image
 * writable (pixels; NV12: even sizes) and no larger than (max_h, max_w); the four box coordinates finite; bx1 = trunc(x1), by1, bx2, by2
 * all in [-8191, 8191].  Anything else: flag 2, nothing written.  A usable row with len == 0: flag 1, an EMPTY LABEL, nothing written --
 * how a row with nobody in it stays silent.  The descriptor of a flagged row is zero but for image = -1 and the flag.
 * With s = scale, a = advance, P = pad * s:  TW = len * a * s, TH = 8 * s, PW = TW + 2 P, PH = TH + 2 P.
 * PLACEMENT (the place word is 0 where place_dev is NULL).  place == 1: X = bx1, Y = by1 -- inside the top-left corner, for regions.  Any
 * other word: X = bx1, Y = by1 - PH, and if Y < 0 then Y = by2 + 1 -- above the box, else below it.  Then X = max(0, min(X, w - PW)) and
 * Y = max(0, min(Y, h - PH)): a plate wider than the frame starts at 0 and is clipped.  The PLATE is [X, X + PW) x [Y, Y + PH) clipped to
 * the frame, the TEXT ORIGIN (X + P, Y + P).
 * COVERAGE.  Pixel (px, py) is a glyph pixel of row k iff fx = px - (X + P) lies in [0, TW), fy = py - (Y + P) in [0, TH), and with
 * ci = fx / (a s), col = (fx % (a s)) / s, r = fy / s, c = text[k][ci], g = c - 32 if 32 <= c <= 126 else 31 (the '?' glyph):
 * (font[g][r] >> col) & 1.  (A glyph pixel lies inside the plate.)
 * STROKES.  With a background the plate of row k is stroke 2 k, in the call's one background colour; the glyph pixels of row k are stroke
 * 2 k + 1, in colors_dev[k], else color.  A pixel takes the colour of the HIGHEST-numbered stroke that covers it, whatever the launch
 * geometry; a pixel no stroke covers is not written.  Without a background only the glyph strokes exist.  NV12 follows "annotated frames
 * out": every covered luma pixel gets the Y of ITS highest stroke; a chroma pair is written iff any of its four luma pixels is covered,
 * with the (U, V) of the highest stroke among the four; colours are (Y, U, V).
 *   images_dev, num_images, max_h, max_w, boxes_dev, image_of_dev: as mcg_draw_gaze_arrows takes them
 *   text_dev     DEVICE uint8 [n][24];  place_dev DEVICE int32 [n] or NULL;  font_dev DEVICE uint8 [96][8]
 *   scale 1 .. 16 (pixels per font bit), advance 1 .. 8 (font columns per character), pad 0 .. 8 (font bits around the text)
 *   color        HOST uint8[3], used for every row when colors_dev is NULL;  colors_dev DEVICE uint8 [n][3] or NULL
 *   background   HOST uint8[3] or NULL (no plates)
 *   plan_out_dev DEVICE [n] descriptors (written);  flags_dev DEVICE int32 [n] or NULL
 * Two launches (plan; a gather kernel over (image, pixel tile) that ballots 64 plan records at a time against a wave's strip, walks the
 * hits in ascending order and stores each covered pixel once), no allocation, no host sync, no atomics, graph-capturable.  n <= 65535 and
 * the ranges above: anything else, or a null required table, returns MCG_ERR_ARG before any launch; n == 0 returns MCG_OK without one.  No
 * byte outside [0, h) x [0, w) of any plane is touched, padding included, for ANY table contents.  Every wave of the gather grid reads the
 * plan in n / 64 slices: made for the tens of labels of a video frame.  mcgaze_amd/arrows.py::format_labels_host and draw_labels_host are
 * the same on the host, bit for bit.  Out of scope: scalable or anti-aliased fonts, glyphs beyond the '?' fallback, a scale per row. */
#define MCG_LABEL_CHARS 24
typedef struct mcg_label_desc {
  int x, y;                 /* the text origin (X + P, Y + P) */
  int x0, y0, x1, y1;       /* the plate clipped to the frame, half open */
  int image, flag;          /* flag 0: drawn; 1: an empty label; 2: unusable */
  int len;
  unsigned color;           /* the glyphs' colour, c0 | c1 << 8 | c2 << 16 */
  unsigned char text[MCG_LABEL_CHARS];   /* the first len codes, then zeros */
} mcg_label_desc;
int mcg_format_labels(mcg_stream s, const int32_t* id_dev, const int32_t* value_dev, int n, int num, int den, unsigned char* text_out_dev);
int mcg_draw_labels(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                    const int32_t* image_of_dev, const unsigned char* text_dev, const int32_t* place_dev, int n, const unsigned char* font_dev,
                    int scale, int advance, int pad, const unsigned char* color, const unsigned char* colors_dev, const unsigned char* background,
                    mcg_label_desc* plan_out_dev, int32_t* flags_dev);
int mcg_draw_labels_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                         const int32_t* image_of_dev, const unsigned char* text_dev, const int32_t* place_dev, int n, const unsigned char* font_dev,
                         int scale, int advance, int pad, const unsigned char* yuv, const unsigned char* yuvs_dev, const unsigned char* background,
                         mcg_label_desc* plan_out_dev, int32_t* flags_dev);

/* ---------------------------------------------------------------- gaze heat map (additions to ABI 19; nothing above changes)
 * Where in the picture looks have landed, over the calls so far: `hit` of "gaze targets" accumulated into a grid of cells per camera
 * (mcg_gaze_heat_add) and that grid blended, colour-mapped, into packed BGR frames (mcg_draw_heat) or NV12 surfaces (mcg_draw_heat_nv12)
 * IN PLACE.  Every table is in device memory.  Behind the first rounding of `hit` everything is integer arithmetic; >> is an arithmetic
 * shift (a floor), / a floor of non-negative integers.
 * GRID.  heat is int32 [C][GH][GW], one grid per camera, a cell 2^cell_shift pixels square (cell_shift 0 .. 6); the caller keeps it between
 * calls.  A negative value found in it is read as 0, by both entries.
 * 1. ACCUMULATE, mcg_gaze_heat_add.  THE ROW RULE: row k counts iff ALL of
 *   flags_dev is NULL or flags[k] == 0;  mask_dev is NULL or mask[k] != 0;
 *   0 <= kind[k] <= 3 and bit kind[k] of `kinds` is set;
 *   image_of[k] >= 0, and with c = image_of[k] where period == 0, else image_of[k] % period:  c < C;
 *   hx = rint((double)hit[k][0]), hy = rint((double)hit[k][1]) (half to even) are finite and in [-8191, 8191] -- the sight line's test of
 *   "attention overlay".
 * Any other row is skipped: what the tables hold is never an error.
 * THE SPLAT.  The row's cell is (ix, iy) = (hx >> cell_shift, hy >> cell_shift).  For every |dx| <= radius, |dy| <= radius it adds
 * w = (radius + 1 - |dx|) * (radius + 1 - |dy|) to cell (ix + dx, iy + dy) of camera c; a tap outside [0, GW) x [0, GH) is dropped, so a
 * hit outside the picture still lights the edge cells within its radius.
 * THE UPDATE, per cell, once per CALL:  h = max(heat, 0);  if decay_shift > 0, h -= h >> decay_shift (before anything is added);
 * heat = min((int64)h + the sum of the cell's taps, 2^31 - 1).  peak[c] = the maximum of camera c's updated cells (0 for a grid of zeros).
 * SHAPE.  Three launches: the workspace and peak cleared; a SCATTER, one thread per (row, tap row), with integer vector atomics into the
 * workspace; a per-cell pass that decays, adds, saturates and takes the camera's maximum with an integer atomic max.  Integer sums and
 * maxima commute, so the result is a function of the inputs alone, whatever the launch geometry.  (A gather per cell tile would read all n
 * rows in every tile of up to 2^24 cells for splats that touch at most 289 cells each: the scatter's work is n * (2 radius + 1)^2.)  One
 * call's taps sum to at most 65536 * 81 < 2^23 per cell: the workspace cannot overflow.
 *   hit_dev DEVICE f32 [n][2];  kind_dev, image_of_dev DEVICE int32 [n] (the three may be NULL iff n == 0);  flags_dev, mask_dev DEVICE int32 [n] or NULL
 *   heat_dev DEVICE int32 [C][GH][GW], read and written;  peak_dev DEVICE int32 [C], written
 *   radius 0 .. 8 (cells);  kinds: bits 0 .. 3 are read;  period >= 0;  decay_shift 0 .. 30, 0: off
 *   workspace_dev DEVICE, workspace_bytes >= 4 * C * GH * GW; what it holds on entry does not matter
 * n <= 65536, 1 <= C <= 4096, 1 <= GH, GW <= 8192, C * GH * GW <= 2^24: anything else, a null required table or a workspace too small
 * returns MCG_ERR_ARG before any launch.  With n == 0 the call still decays and writes peak.  A fixed number of launches, no allocation, no
 * host sync, graph-capturable.  mcgaze_amd/attention.py::gaze_heat_host is the same on the host, bit for bit.
 * 2. RENDER, mcg_draw_heat / mcg_draw_heat_nv12, over the image table of mcg_draw_gaze_arrows.  Picture p shows camera c = p where
 * period == 0, else p % period.  A picture is left untouched, byte for byte, if c >= C, if it is not writable (no pixels; NV12: an odd
 * size), or if it is larger than (max_h, max_w).
 * LEVEL of pixel (px, py), with S = 2^cell_shift -- an interpolation between cell centres:
 *   u = 2 px + 1 - S;  i0 = u >> (cell_shift + 1);  fx = u - i0 * 2 S (in [0, 2 S));  i1 = i0 + 1;  both clamped to [0, GW - 1]
 *   the same in y: j0, fy, j1, clamped to [0, GH - 1];  hab = max(heat[c][ja][ib], 0)
 *   v = (2 S - fx) (2 S - fy) h00 + fx (2 S - fy) h01 + (2 S - fx) fy h10 + fx fy h11      (int64; v < 2^45)
 *   full = max(full_dev[c], 1);  L = min(255, (v * 255) / (4 S S full))                    (int64; the product is below 2^53)
 * At cell_shift == 0 this is the cell's own value; a grid smaller than the picture repeats its edge cells, so every pixel has a level.
 * full_dev is the peak table of mcg_gaze_heat_add, or the caller's own fixed scale.
 * COLOUR.  lut_dev is a DEVICE uint8 [256][4] table, 4-byte aligned, the ramp as DATA: entry L is (B, G, R, alpha), for NV12 (Y, U, V,
 * alpha).  A BGR pixel with L >= min_level becomes (src * (255 - a) + col * a + 127) / 255 per channel with a = lut[L][3]; a pixel with
 * L < min_level keeps its bytes.  NV12: every luma pixel is blended like that with the Y of ITS level; a chroma pair takes Lc, the maximum
 * of its four luma pixels' levels, and is blended with the (U, V, alpha) of lut[Lc] iff Lc >= min_level, that is, iff any of the four is
 * -- the rule of "annotated frames out".
 *   images_dev, num_images, max_h, max_w: as mcg_draw_gaze_arrows takes them
 *   heat_dev DEVICE int32 [C][GH][GW], full_dev DEVICE int32 [C] (both read);  min_level 1 .. 255
 * ONE launch over (image, tile of 256 x 16 pixels; NV12: 256 x 32): a block keeps its tile's cells and one cell of apron, edge cells
 * repeated, and the 256 colours in LDS; a thread owns 16 pixels of a row (NV12: 16 x 2 and their 8 chroma pairs), and reads and writes
 * them in 16-byte accesses where the plane's address and pitch are multiples of 16, in 4-byte accesses where they are multiples of 4, byte
 * by byte at the right edge and for any other pitch.  A tile over nothing but zero cells reads no pixel.  No allocation, no host sync, no
 * atomics, graph-capturable.  The limits of the grid above, num_images in 1 .. 65535, frames of at most 8192 a side: anything else or a
 * null table returns MCG_ERR_ARG before the launch.  No byte outside [0, h) x [0, w) of any plane is touched, padding included, for ANY
 * table contents.  mcgaze_amd/arrows.py::draw_heat_host is the same on the host, bit for bit.  Out of scope: per-person maps, perspective
 * or depth (the grid is the image plane; "surface heat map" below keeps a grid ON a planar region), a decay per frame inside a multi-frame
 * call, Gaussian kernels. */
int mcg_gaze_heat_add(mcg_stream s, const float* hit_dev, const int32_t* kind_dev, const int32_t* image_of_dev, const int32_t* flags_dev,
                      const int32_t* mask_dev, int n, int32_t* heat_dev, int32_t* peak_dev, int C, int GH, int GW, int cell_shift, int radius,
                      int kinds, int period, int decay_shift, void* workspace_dev, size_t workspace_bytes);
int mcg_draw_heat(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const int32_t* heat_dev,
                  const int32_t* full_dev, int C, int GH, int GW, int cell_shift, int period, const unsigned char* lut_dev, int min_level);
int mcg_draw_heat_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const int32_t* heat_dev,
                       const int32_t* full_dev, int C, int GH, int GW, int cell_shift, int period, const unsigned char* lut_dev, int min_level);

/* ---------------------------------------------------------------- anonymised heads (additions to ABI 19; nothing above changes)
 * The faces under the head boxes removed IN PLACE from packed BGR frames (mcg_anonymize_heads) or NV12 surfaces (mcg_anonymize_heads_nv12),
 * after the network has read them and before anything is drawn on top: every covered pixel becomes the mean of a coarse cell of the frame
 * (mosaic) or one colour (fill).  The image table and the rows are those of mcg_draw_gaze_arrows.  Two launches: a plan kernel (one thread
 * per row, double, uncontracted) writes one mcg_anon_desc per row, then a render kernel over (tile of 64 x 64 pixels, image).  The call
 * hides the heads it is GIVEN: a head the detector missed stays visible.
 * 1. PLAN, per row, from a box x1 y1 x2 y2 (f32, widened to double) and image_of.  A row is USABLE iff image_of is in [0, num_images), the
 * four coordinates are finite with x2 > x1 and y2 > y1, its picture is writable (it has pixels; NV12: of even size) and no larger than
 * (max_h, max_w), and, with
 *   ex = expand * (x2 - x1);  ey = expand * (y2 - y1);  X0 = floor(x1 - ex);  X1 = ceil(x2 + ex);  Y0 = floor(y1 - ey);  Y1 = ceil(y2 + ey)
 * (every product and difference rounded on its own), |X0|, |X1|, |Y0|, |Y1| <= 8191.  The integer rectangle always contains the float
 * box: rounding never uncovers a face.  W = X1 - X0 and H = Y1 - Y0 are at least 1 and below 2^14.
 * The SHIFT s of the row is cell_shift where that is not 0; otherwise the smallest s in 1 .. 6 with (blocks << s) >= max(W, H), and 6 if
 * there is none -- a far head gets small cells and a near head large ones, about `blocks` cells across either.
 * The descriptor holds the rectangle clipped to the picture, half open, [max(X0, 0), min(X1, w)) x [max(Y0, 0), min(Y1, h)) -- it may be
 * empty: the row then writes nothing and its flag is still 0 --, cx2 = X0 + X1, cy2 = Y0 + Y1, W, H, the shift and the shape.
 * FLAGS.  0: usable.  2: unusable; NOTHING is written for the row, and its descriptor is zero but for image = -1 and flag = 2.
 * 2. COVERAGE, exact, in 64-bit integers.  Pixel (px, py) is covered by a row iff it lies in the row's clipped rectangle and, with shape 1,
 *   (2 px + 1 - cx2)^2 H^2 + (2 py + 1 - cy2)^2 W^2 <= W^2 H^2
 * -- the ellipse inscribed in the integer rectangle, tested at pixel centres.  |2 px + 1 - cx2| and |2 py + 1 - cy2| are below 2^15 and
 * W, H below 2^14: each product is below 2^58 and the sum below 2^59.
 * 3. VALUE, mode 0 (mosaic).  For every s the frame carries a grid of cells of 2^s x 2^s pixels aligned to the frame's origin; the cells at
 * the right and bottom edges are cut to the frame.  A covered pixel takes s(p), the LARGEST shift among the rows that cover it, and becomes
 * the mean of its cell at that shift, per channel, (sum + (count >> 1)) / count in integers, over ALL of the cell's pixels inside the
 * frame, covered or not, AS THEY WERE BEFORE THE CALL.  A cell has one value, so overlapping boxes cannot disagree.  A second call reads
 * what the first one wrote: where the coverage cuts through cells the call is NOT idempotent.
 * Mode 1 (fill): a covered pixel becomes `color`; the result does not depend on what the frame held.
 * A pixel that no row covers keeps its bytes, pitch padding included (the kernel writes whole spans of 16 pixels that hold a covered
 * pixel, the others with the bytes it read, and touches no span without one).
 * NV12 follows "annotated frames out": a luma pixel is treated as above, over the Y plane.  A chroma pair is written iff ANY of its four
 * luma pixels is covered; its shift is the largest s(p) of those four, and U and V each become the rounded mean of the chroma samples of
 * the pair's cell at that shift -- 2^(s-1) x 2^(s-1) pairs (s >= 1), aligned to the origin, cut to the frame.  Fill: (Y, U, V) of `color`.
 * No claim is made that the NV12 result equals the BGR result converted.
 * THE RENDER KERNEL.  A tile is a frame-aligned block of 64 x 64 pixels, so every cell of every shift lies inside exactly one tile: a
 * workgroup reads only its own tile, all of its reads come before its writes with a barrier between, and no other workgroup touches those
 * bytes -- in place needs neither a second buffer nor atomics on the image.  A workgroup walks the descriptors in chunks of 256 and keeps
 * those of its image whose rectangle meets the tile (no cap on their number); a tile under no head is never read.  A thread owns 16 pixels
 * of a row (NV12: 16 x 2 and their 8 chroma pairs), read and written as mcg_draw_heat does.  Cell sums are integers: their order does not
 * matter.
 *   images_dev, num_images, max_h, max_w, boxes_dev, image_of_dev: as mcg_draw_gaze_arrows takes them;  n in 0 .. 65536
 *   expand 0 .. 4;  shape 0 box, 1 ellipse;  cell_shift 0 (automatic) or 1 .. 6;  blocks 1 .. 64, read only where cell_shift == 0
 *   mode 0 mosaic, 1 fill;  color HOST uint8[3] (B, G, R; NV12: Y, U, V), read only with mode 1
 *   plan_out_dev DEVICE [n] descriptors (written);  flags_dev DEVICE int32 [n] or NULL
 * Anything else or a null required pointer returns MCG_ERR_ARG before any launch; n == 0 returns MCG_OK without one.  No byte outside
 * [0, h) x [0, w) of any plane is touched for ANY table contents.  No allocation, no host sync, graph-capturable.
 * mcgaze_amd/arrows.py::anonymize_plan_host and anonymize_heads_host are the same on the host, bit for bit.  The defaults of the python
 * layer (expand 0.125, ellipse, 8 blocks) are CONVENTIONS, not tuned on data. */
typedef struct mcg_anon_desc {
  int image, flag;
  int x0, y0, x1, y1;       /* the covered rectangle clipped to the frame, half open; may be empty */
  int cx2, cy2;             /* X0 + X1, Y0 + Y1 of the unclipped rectangle: twice its centre */
  int W, H;                 /* its unclipped size */
  int shift, shape;
} mcg_anon_desc;
int mcg_anonymize_heads(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                        const int32_t* image_of_dev, int n, double expand, int shape, int cell_shift, int blocks, int mode,
                        const unsigned char* color, mcg_anon_desc* plan_out_dev, int32_t* flags_dev);
int mcg_anonymize_heads_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const float* boxes_dev,
                             const int32_t* image_of_dev, int n, double expand, int shape, int cell_shift, int blocks, int mode,
                             const unsigned char* yuv, mcg_anon_desc* plan_out_dev, int32_t* flags_dev);

/* ---------------------------------------------------------------- gaze targets, 3-D (additions to ABI 20; nothing above changes)
 * "gaze targets" decides in the image plane and reads only (gx, gy): a head behind another along the image ray is the farther one in
 * pixels whatever its depth, and a look at a region lands on the region's rim.  mcg_gaze_targets_3d decides in CAMERA SPACE (x right, y
 * down, z away from the lens, metres): every row is lifted to a point with the intrinsics of its camera and a depth, its gaze becomes a
 * direction there, heads are boxes around those points and regions are planar polygons.  The output tables keep the names, shapes and
 * meanings of "gaze targets", so dwell, heat, overlay and labels run on them unchanged; hit3d is added.  Two launches (the second is the
 * `mutual` launch of "gaze targets"), no allocation, no host sync, graph-capturable, no atomics in global memory.
 * Everything is double and uncontracted (no FMA): every product, quotient, sum and difference below is rounded on its own, in the order
 * the parentheses give; f32 tables are widened exactly.  The only square roots are two sqrtf of a value rounded to f32 (correctly rounded
 * on host and device).  Comparisons with a NaN are false, and every min / max below is written as the comparison it stands for.
 * CAMERA TABLE.  cam f32 [C][4] = fx, fy, cx, cy (pixels).  Row k belongs to camera c = image_of[k] if cam_period == 0, else image_of[k] %
 * cam_period.
 * UNUSABLE (flag 2).  A row is unusable iff it is unusable under "gaze targets", or c >= C, or one of the camera's four numbers is not
 * finite, or not (fx > 0 and fy > 0), or its Z or its origin below is not finite and positive / finite.  cam is read only at a c < C.
 * DEPTH.  If depth is given and depth[k] is finite and > 0:  Z = depth[k].  Otherwise  Z = (fx * head_size) / max(x2 - x1, y2 - y1),
 * (max: w > h ? w : h).  head_size is the size of a head in metres (Python default 0.24: a CONVENTION, not tuned on data).  Not (Z finite
 * and Z > 0): flag 2.
 * ORIGIN.  u = (x1 + x2) * 0.5, v = (y1 + y2) * 0.5 as in "gaze targets";  X = ((u - cx) * Z) / fx,  Y = ((v - cy) * Z) / fy,  O = (X, Y, Z).
 * X or Y not finite (only a head_size beyond the f32 range can do that): flag 2.
 * DIRECTION.  frame 0 ('camera'):  D = (-gx, -gy, gz) -- the arrow's (-gx, -gy), and gz < 0 towards the lens.
 * frame 1 ('eye', the Python default): the gaze is relative to the line from the lens to the head, as Gaze360 states it and as the CAMERA
 * rule of "gaze targets" assumes.  With the basis  right = (Z, 0, -X) / a,  down = (-X Y, a2, -Y Z) / (a r),  forward = (X, Y, Z) / r,
 * scaled by a r > 0:
 *   a2 = X * X + Z * Z;   a = (double)sqrtf((float)a2);   r = (double)sqrtf((float)(a2 + Y * Y));   p = gx * r;   q = gz * a;
 *   Dx = ((q * X) - (p * Z)) + (gy * (X * Y));   Dy = (q * Y) - (gy * a2);   Dz = ((q * Z) + (p * X)) + (gy * (Y * Z))
 * i.e. D = -gx r (Z, 0, -X) - gy (-X Y, a2, -Y Z) + gz a (X, Y, Z).  D is NOT normalised: t below is its ray parameter, and distances in
 * metres come from hit3d.
 * AT THE CAMERA (kind 3), before everything below.  frame 1: the CAMERA rule of "gaze targets" on (gx, gy, gz), unchanged.  frame 0:
 *   s = -((Dx * X + Dy * Y) + Dz * Z);   s > 0  and  s * s >= camera_cos2 * (((Dx * Dx + Dy * Dy) + Dz * Dz) * ((X * X + Y * Y) + Z * Z)).
 * Otherwise, if a component of D is not finite or all three compare equal to zero, the kind is 0.
 * HEADS.  Every OTHER usable row j of the same picture, as the box [O_j - (hw, hh, hd), O_j + (hw, hh, hd)] with w = x2 - x1, h = y2 - y1,
 * e = expand * max(w, h):   hw = (((w * 0.5) + e) * Z_j) / fx_j;   hh = (((h * 0.5) + e) * Z_j) / fy_j;   hd = hw > hh ? hw : hh.
 * The SLAB TEST of "gaze targets" with a third axis: near starts at -inf and far at +inf; an axis with D_a == 0 passes iff lo_a <= O_a <=
 * hi_a; any other gives t1 = (lo_a - O_a) / D_a, t2 = (hi_a - O_a) / D_a, l = t1 < t2 ? t1 : t2, h = the other, near = l > near ? l :
 * near, far = h < far ? h : far, axes in the order x, y, z.  A hit iff every axis passes, near <= far, far >= 0 and t = (near > 0 ? near :
 * +0) is finite.
 * REGIONS.  region_xyz f32 [V][3] vertices in camera coordinates, region_start int32 [m + 1], region_image / region_period as in "gaze
 * targets".  Region j is USABLE iff 0 <= region_start[j] <= region_start[j + 1] <= V, its vertex count c is 3 .. 32, every coordinate it
 * owns is finite, and N is not all zero:  e1 = v1 - v0,  e2 = v2 - v0,
 *   Nx = e1y * e2z - e1z * e2y;   Ny = e1z * e2x - e1x * e2z;   Nz = e1x * e2y - e1y * e2x.
 * The offsets are checked before the first vertex load: whatever the tables hold, nothing outside them is read.  An unusable region is
 * never hit and flags nothing.
 *   den = (Nx * Dx + Ny * Dy) + Nz * Dz;   tn = (Nx * (v0x - X) + Ny * (v0y - Y)) + Nz * (v0z - Z);   q = tn / den.
 * The plane is met iff den != 0, q is finite and q >= 0;  t = q > 0 ? q : +0;  P = (X + t * Dx, Y + t * Dy, Z + t * Dz).  The region is
 * hit iff P is INSIDE by the even-odd rule of "gaze targets, polygonal regions" (its toggle test, edges in ascending order) applied to the
 * two coordinates (pu, pv) left, in the order x y z, after the axis of the largest |N| component is dropped (|Nx| >= |Ny| and |Nx| >=
 * |Nz|: x; else |Ny| >= |Nz|: y; else z).  There is no "inside means t = 0" case in 3-D, and a region is two-sided.
 * CHOICE.  The smallest t wins; on equal t a head comes before a region, then the lower index -- the rule of "gaze targets".
 * OUTPUTS.  kind, target, t, mutual and flags as in "gaze targets".  For kind 1 or 2, P = O + t * D per component as above;
 * hit3d [n][3] = P rounded once to f32;  hit [n][2] = (fx * (Px / Pz) + cx, fy * (Py / Pz) + cy) rounded once to f32 where Pz > 0 and the
 * value is a number, else the quiet NaN 0x7fc00000 (per component) -- the row rules of the overlay and of the heat map skip a hit that is
 * not finite.  Every other row writes what "gaze targets" writes (zeros, target -1) and zeros to hit3d.
 *   boxes_dev, gaze_dev, gaze_stride, image_of_dev, n, region_image_dev, m, region_period, expand, camera_cos2, kind_dev .. flags_dev
 *                  as mcg_gaze_targets takes them
 *   cam_dev        DEVICE f32 [num_cameras][4], 1 <= num_cameras <= 4096;  cam_period >= 0
 *   depth_dev      DEVICE f32 [n] or NULL
 *   head_size      finite, > 0;   frame 0 or 1
 *   region_xyz_dev DEVICE f32 [num_vertices][3], NULL iff num_vertices == 0;  region_start_dev int32 [m + 1], NULL iff m == 0
 *   hit3d_dev      DEVICE f32 [n][3], written
 * 0 <= n <= 65536, 0 <= m <= 4096, 0 <= num_vertices <= 65536; n == 0 returns MCG_OK without a launch.  Anything else, or a null required
 * table, returns MCG_ERR_ARG before any launch; the CONTENTS of the device tables never are an error and are never read back.  Heads and
 * regions are searched in tiles of 256 with the picture-range skip of "gaze targets".
 * mcgaze_amd/attention.py::gaze_targets_3d_host is the same on the host, bit for bit.  head_size, frame, expand and camera_cos2 are
 * CONVENTIONS, not tuned on data.
 * Out of scope: lens distortion, a region's pose from four image corners, one-sided regions, depth from anything but the size of the head
 * or the caller's table. */
int mcg_gaze_targets_3d(mcg_stream s, const float* boxes_dev, const float* gaze_dev, int gaze_stride, const int32_t* image_of_dev, int n,
                        const float* cam_dev, int num_cameras, int cam_period, const float* depth_dev, double head_size, int frame,
                        const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev, const int32_t* region_image_dev, int m,
                        int region_period, double expand, double camera_cos2, int32_t* kind_dev, int32_t* target_dev, float* t_dev,
                        float* hit_dev, int32_t* mutual_dev, int32_t* flags_dev, float* hit3d_dev);

/* ---------------------------------------------------------------- surface heat map (additions to ABI 20; nothing above changes)
 * Where ON a planar region -- a screen, a shelf, a poster -- looks have landed, over the calls so far, as a grid in the region's OWN
 * coordinates: hit3d of "gaze targets, 3-D" is taken into the region's chart and accumulated into one grid per region
 * (mcg_surface_heat_add); the grids are drawn back onto their regions, with the right perspective, into packed BGR frames
 * (mcg_draw_surface_heat) or NV12 surfaces (mcg_draw_surface_heat_nv12) IN PLACE.  The grid does not move when the camera does: a caller
 * whose camera moves hands in the region's vertices in the new camera coordinates and keeps the grid.  Every table is in device memory.
 * Everything up to the first floor is double and uncontracted (no FMA): every product, quotient, sum and difference below is rounded on
 * its own, in the order the parentheses give; f32 tables are widened exactly; there is no square root.  Comparisons with a NaN are false,
 * and every min / max is written as the comparison it stands for.  Behind the first floor everything is integer arithmetic; >> is an
 * arithmetic shift (a floor), / a floor of non-negative integers.
 * REGIONS are the PolyRegions3D tables of "gaze targets, 3-D" (region_xyz f32 [V][3], region_start int32 [M + 1]) under its USABLE rule,
 * unchanged: the offsets checked before any vertex load, 3 .. 32 vertices, every coordinate finite, N = e1 x e2 not all zero.
 * CHART of region j.  a = v1 - v0;  N as in "gaze targets, 3-D";  b = N x a, written as N is:
 *   bx = Ny * az - Nz * ay;   by = Nz * ax - Nx * az;   bz = Nx * ay - Ny * ax;
 *   aa = (ax * ax + ay * ay) + az * az;   bb = (bx * bx + by * by) + bz * bz.
 * For a point Q, with w = Q - v0:   s(Q) = ((wx * ax + wy * ay) + wz * az) / aa;   r(Q) = ((wx * bx + wy * by) + wz * bz) / bb.
 * smin, smax, rmin, rmax over the region's OWN vertices k = 0, 1, ... in ascending order: the first vertex gives the start value, every
 * later one replaces it on  s < smin  (s > smax; r likewise).  ws = smax - smin;  hr = rmax - rmin.
 * The chart is USABLE iff the region is usable and aa, bb, ws, hr are finite and > 0.  The grid coordinates of Q in a GW x GH grid:
 *   fu = ((s - smin) / ws) * GW;   fv = ((r - rmin) / hr) * GH.
 * The chart is the bounding rectangle of the polygon in the (a, N x a) frame stretched over GW x GH cells: the aspect ratio is the
 * caller's choice of grid (mcgaze_amd/attention.py::surface_extent gives the rectangle's sides in metres).  WINDING: for a screen listed
 * CLOCKWISE from its top-left corner as the camera sees it (x right, y down), fu runs right and fv runs down, so grid row 0 is the top;
 * the other winding flips the map vertically.
 * 1. ACCUMULATE, mcg_surface_heat_add.  The state is heat int32 [M][GH][GW] and peak int32 [M].  THE ROW RULE: row k counts iff ALL of
 *   flags_dev is NULL or flags[k] == 0;  mask_dev is NULL or mask[k] != 0;  kind[k] == 2;  0 <= target[k] < M;
 *   region target[k] has a usable chart;  the three values of hit3d[k] are finite;
 *   with Q = hit3d[k]:  fu and fv are finite and |fu|, |fv| <= 16384.
 * Any other row is skipped: what the tables hold is never an error.  The row's cell is (ix, iy) = (floor(fu), floor(fv)) -- a hit on the
 * far edge (fu == GW) has its cell just off the grid and still lights the edge cells within its radius.  THE SPLAT (radius 0 .. 8,
 * weights (radius + 1 - |dx|) (radius + 1 - |dy|), taps off the grid dropped), THE UPDATE once per call (max(h, 0), decay_shift,
 * saturation at 2^31 - 1) and peak[j] are those of "gaze heat map" with the region index in the camera's place; the clear and the update
 * launches ARE that section's kernels.
 *   hit3d_dev DEVICE f32 [n][3];  kind_dev, target_dev DEVICE int32 [n] (the three may be NULL iff n == 0);  flags_dev, mask_dev DEVICE int32 [n] or NULL
 *   region_xyz_dev DEVICE f32 [num_vertices][3], NULL iff num_vertices == 0;  region_start_dev DEVICE int32 [M + 1]
 *   heat_dev DEVICE int32 [M][GH][GW], read and written;  peak_dev DEVICE int32 [M], written
 *   radius 0 .. 8 (cells);  decay_shift 0 .. 30, 0: off
 *   workspace_dev DEVICE, aligned to 8 bytes, workspace_bytes >= MCG_SURFACE_CHART_BYTES * M + 4 * M * GH * GW; what it holds on entry
 *   does not matter
 * Four launches: a PLAN launch, one thread per region, writes each region's chart (v0, a, b, N, aa, bb, smin, ws, rmin, hr, a usable
 * word, the dropped axis: 20 doubles, all zero for a chart that is not usable) into the workspace -- the scatter and the render read that
 * table, so the chart is worked out once, by one piece of code --; the rest of the workspace and peak cleared; a SCATTER, one thread per
 * (row, tap row), with integer vector atomics; the per-cell update over M regions.  Integer sums and maxima commute, so the result is a
 * function of the inputs alone.  With n == 0 the call still decays and writes peak.
 * 2. RENDER, mcg_draw_surface_heat / mcg_draw_surface_heat_nv12, over the image table of mcg_draw_gaze_arrows.  Picture p has camera
 * c = p where cam_period == 0, else p % cam_period; cam f32 [C][4] as in "gaze targets, 3-D".  A picture is left untouched, byte for byte,
 * if c >= C, if one of its camera's four numbers is not finite or not (fx > 0 and fy > 0), if it is not writable (no pixels; NV12: an odd
 * size), or if it is larger than (max_h, max_w).  Region j APPLIES to picture p by the region_image / region_period rule of "gaze
 * targets" with p in place of image_of[i]: region_image[j] < 0, or region_image[j] == p (region_period == 0), == p % region_period.
 * For pixel (px, py):   d = ((px - cx) / fx, (py - cy) / fy, 1).  For every applying region with a usable chart:
 *   den = (Nx * dx + Ny * dy) + Nz * dz;   tn = (Nx * v0x + Ny * v0y) + Nz * v0z;   t = tn / den.
 * The plane is met iff den != 0, t is finite and t > 0;  then P = (t * dx, t * dy, t).  The region COVERS the pixel iff P is inside by the
 * even-odd rule of "gaze targets, 3-D" (the axis of the largest |N| dropped).  The smallest t wins; on equal t the lower index.
 * LEVEL, for the winner j, from fu, fv of P in j's chart; a pixel that no region covers, or whose fu or fv is not finite, keeps its bytes:
 *   U = (int64)floor(fu * 256) - 128  (the floor is first held to [-2^30, 2^30]: both cells are then the same edge cell, no level changes);
 *   i0 = U >> 8;  fx = U - i0 * 256;  i1 = i0 + 1;  both clamped to [0, GW - 1];  the same in v: j0, fy, j1, clamped to [0, GH - 1]
 *   hab = max(heat[j][ja][ib], 0)
 *   val = (256 - fx) (256 - fy) h00 + fx (256 - fy) h01 + (256 - fx) fy h10 + fx fy h11      (int64; val < 2^47)
 *   full = max(full_dev[j], 1);  L = min(255, (val * 255) / (65536 * full))                  (int64)
 * -- an interpolation between cell centres, edge cells repeated.  COLOUR, alpha, min_level, the BGR blend and the NV12 luma / chroma-pair
 * rule are those of mcg_draw_heat, word for word; lut_dev is the same [256][4] table; full_dev is peak or the caller's own scale, int32 [M].
 *   images_dev, num_images, max_h, max_w: as mcg_draw_gaze_arrows takes them
 *   cam_dev DEVICE f32 [C][4], 1 <= C <= 4096;  cam_period, region_period >= 0;  region_image_dev DEVICE int32 [M]
 *   heat_dev DEVICE int32 [M][GH][GW], full_dev DEVICE int32 [M] (both read);  min_level 1 .. 255
 *   workspace_dev DEVICE, aligned to 8 bytes, workspace_bytes >= MCG_SURFACE_CHART_BYTES * M
 * Two launches: the PLAN launch above, then ONE launch over (image, tile of 256 x 16 pixels; NV12: 256 x 32).  A workgroup first lists in
 * LDS the applying regions with a usable chart whose projected bounding box, grown by one pixel, touches its tile.  The box is that of
 * the vertices MOVED ALONG THE DROPPED AXIS ONTO THE PLANE through v0 -- a region's vertices need not be coplanar, and those are the
 * points between which the exact test decides --; a region with such a point at z <= 0 counts as touching every tile.  The list is a cull: the exact
 * test per pixel decides, and the result is that of the test made for every applying region.  A thread owns 16 pixels of a row (NV12:
 * 16 x 2 and their 8 chroma pairs); a tile with an empty list, and a thread whose pixels are all uncovered or below min_level, read no
 * pixel; the others read and write as mcg_draw_heat does (16-byte, 4-byte or byte accesses by the plane's address and pitch).  No atomics
 * in global memory.  No byte outside [0, h) x [0, w) of any plane is touched, padding included, for ANY table contents.
 * LIMITS.  n <= 65536, 1 <= M <= 4096, num_vertices <= 65536, 1 <= GH, GW <= 1024, M * GH * GW <= 2^24, num_images in 1 .. 65535, frames
 * of at most 8192 a side: anything else, a null required table, a workspace that is too small or not aligned returns MCG_ERR_ARG before
 * any launch, with nothing written.  A fixed number of launches, no allocation, no host sync, graph-capturable.
 * mcgaze_amd/attention.py::surface_charts_host and surface_heat_host and mcgaze_amd/arrows.py::draw_surface_heat_host are the same on the
 * host, bit for bit.  The python defaults (a grid of 32 x 32, radius 1) are CONVENTIONS, not tuned on data.
 * Out of scope: curved surfaces, one-sided regions, lens distortion, a chart other than the bounding rectangle, per-person maps. */
#define MCG_SURFACE_CHART_BYTES 160
int mcg_surface_heat_add(mcg_stream s, const float* hit3d_dev, const int32_t* kind_dev, const int32_t* target_dev, const int32_t* flags_dev,
                         const int32_t* mask_dev, int n, const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev, int M,
                         int32_t* heat_dev, int32_t* peak_dev, int GH, int GW, int radius, int decay_shift, void* workspace_dev,
                         size_t workspace_bytes);
int mcg_draw_surface_heat(mcg_stream s, const mcg_image_desc* images_dev, int num_images, int max_h, int max_w, const float* cam_dev, int C,
                          int cam_period, const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev,
                          const int32_t* region_image_dev, int M, int region_period, const int32_t* heat_dev, const int32_t* full_dev, int GH, int GW,
                          const unsigned char* lut_dev, int min_level, void* workspace_dev, size_t workspace_bytes);
int mcg_draw_surface_heat_nv12(mcg_stream s, const mcg_nv12_image_desc* images_dev, int num_images, int max_h, int max_w, const float* cam_dev,
                               int C, int cam_period, const float* region_xyz_dev, int num_vertices, const int32_t* region_start_dev,
                               const int32_t* region_image_dev, int M, int region_period, const int32_t* heat_dev, const int32_t* full_dev, int GH,
                               int GW, const unsigned char* lut_dev, int min_level, void* workspace_dev, size_t workspace_bytes);

/* ---------------------------------------------------------------- measurement aids (bench.py)
 * While armed, every launch of the contraction kernel made by THIS engine is bracketed by a hipEvent pair on its launch stream.
 * mcg_engine_profile_stop synchronises, returns per-launch duration (ms), algorithmic FLOPs, algorithmic HBM bytes (inputs and
 * residual read once, output written once, weights once -- what a layer-granular schedule cannot go below), tile-configuration id
 * (bench.py CFG_NAMES) and the GEMM shape (M, N, K) of every recorded launch (any output array may be NULL), and disarms. */
int mcg_engine_profile_start(mcg_engine* e, int capacity);
int mcg_engine_profile_stop(mcg_engine* e, int* count, float* ms, double* flops, double* algo_bytes, int* cfg, int* shape_mnk, int capacity);
/* BASELINE.json configs[1] "R-50 backbone-only": stem + layer1..4 (C2..C5 stay in the workspace), no FPN.  Not a product entry
 * point; ws >= mcg_trunk_workspace_bytes(e, num_frames, H, W, 0). */
int mcg_bench_backbone_forward(mcg_engine* e, mcg_stream s, const float* img, int num_frames, int H, int W, void* ws, size_t ws_bytes);
/* Where that call left C2..C5 (NHWC [num_frames][H/4 >> i][W/4 >> i][256 << i], engine dtype) inside ws, for a batch that ran as ONE
 * frame range (engine option trunk_streams = 1): tests/test_gpu_forward.py::test_backbone_only_matches_the_oracle. */
int mcg_bench_backbone_levels(const mcg_engine* e, void* ws, int num_frames, int H, int W, void* levels[4]);

#ifdef __cplusplus
}
#endif
#endif /* MCGAZE_HIP_H */
