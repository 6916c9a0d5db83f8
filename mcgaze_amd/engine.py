"""Host-side driver of ``libmcgaze_hip.so``: owns the packed weights, the workspace and the
C engine handle, and exposes the path (and its individual operators, for the parity tests)
over torch device tensors.  PyTorch is used for device memory and streams only; all
arithmetic runs in the hand-written HIP kernels behind the C-ABI.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import lib as L
from .packing import PackedWeights

# precision -> (storage dtype of activations, mcg_dtype code).  'f16x3': f32 storage, split-fp16 x 3 MFMA contraction (parity-grade
# fast mode, include/mcgaze_hip.h MCG_F16X3)
# 'f16' (round 6): the 16-bit throughput mode in fp16 -- bf16's kernels and layouts with 11 significant bits instead of 8 (MCG_F16)
_TORCH_DT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'fp16': torch.float16, 'fp32': torch.float32, 'f32': torch.float32, 'f16x3': torch.float32, 'bf16x3': torch.float32}
_CODE = {'bf16': L.MCG_BF16, 'f16': L.MCG_F16, 'fp16': L.MCG_F16, 'fp32': L.MCG_F32, 'f32': L.MCG_F32, 'f16x3': L.MCG_F16X3,
         'bf16x3': L.MCG_F16X3}   # 'bf16x3': the engine's name while its halves were bf16 -- accepted, runs the fp16-halves engine


def _code(dtype):
    return L.MCG_BF16 if dtype == torch.bfloat16 else (L.MCG_F16 if dtype == torch.float16 else L.MCG_F32)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device=None):
    """The caller's current HIP stream on ``device`` (default: the current device)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_gpu():
    if not torch.cuda.is_available():
        raise L.McgError('mcgaze_amd needs a HIP device (MI355X / gfx950); there is no CPU fallback path')


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------ operators
def to_nhwc(x_nchw, dtype):
    """[N,C,H,W] f32 device tensor -> NHWC ``dtype`` via mcg_nchw_to_nhwc."""
    _require_gpu()
    lib = L.load()
    N, Cc, H, W = x_nchw.shape
    x = x_nchw.contiguous().float()
    out = torch.empty(N, H, W, Cc, dtype=dtype, device=x.device)
    L.check(lib.mcg_nchw_to_nhwc(_stream(), _code(dtype), _ptr(x), _ptr(out), N, Cc, H, W), 'mcg_nchw_to_nhwc')
    return out


def to_nchw(x_nhwc):
    _require_gpu()
    lib = L.load()
    N, H, W, Cc = x_nhwc.shape
    out = torch.empty(N, Cc, H, W, dtype=torch.float32, device=x_nhwc.device)
    L.check(lib.mcg_nhwc_to_nchw(_stream(), _code(x_nhwc.dtype), _ptr(x_nhwc.contiguous()), _ptr(out), N, Cc, H, W), 'mcg_nhwc_to_nchw')
    return out


def conv2d(x, w, bias=None, stride=1, pad=0, relu=False, residual=None, residual_mode=L.RES_NONE, x2=None, stride2=1, split=False,
           tile=0, flags=0, prescale=True):
    """x NHWC, w OHWI (same dtype), bias f32 -> NHWC.  mcg_conv2d.  With x2: w = [Cout,1,1,Cin+Cin2], x2 sampled at stride2.
    split=True: the MCG_F16X3 contraction -- x / residual f32, w given as f32 OHWI and split-packed here (packing.split_pack), pre-scaled
    by a power of two unless prescale=False (packing.pow2_prescale; mcg_conv_desc.wscale).
    tile / flags: mcg_conv_desc.tile (force a contraction tile) and MCG_FLAG_* (lib.FLAG_*)."""
    _require_gpu()
    lib = L.load()
    N, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    wscale = 0.0
    if split:
        from .packing import pow2_prescale, split_pack
        assert x.dtype == torch.float32 and w.dtype == torch.float32
        ws, wscale = pow2_prescale(w.reshape(Cout, -1).cpu()) if prescale else (w.reshape(Cout, -1).cpu(), 0.0)
        w = split_pack(ws).to(x.device)
    Cin2 = x2.shape[3] if x2 is not None else 0
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    y = torch.empty(N, Ho, Wo, Cout, dtype=x.dtype, device=x.device)
    d = L.ConvDesc(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None,
                   residual.data_ptr() if residual is not None else None, y.data_ptr(),
                   N, H, W, Cin, Cout, KH, KW, stride, pad, int(relu), residual_mode if residual is not None else L.RES_NONE,
                   residual.shape[1] if residual is not None else 0, residual.shape[2] if residual is not None else 0,
                   x2.data_ptr() if x2 is not None else None, Cin2, stride2, x2.shape[1] if x2 is not None else 0,
                   x2.shape[2] if x2 is not None else 0, tile, flags, wscale)
    L.check(lib.mcg_conv2d(_stream(), L.MCG_F16X3 if split else _code(x.dtype), C.byref(d)), 'mcg_conv2d')
    return y


def pointwise_weights(w, dtype, split=False, device='cuda'):
    """W [N, K] -> (wf, wscale): the weight operand of the streaming 1x1 kernels (pointwise_stream / pointwise_pair).  16-bit ``dtype``:
    packing.frag_major; split=True (MCG_F16X3): packing.frag_major_split of the pow2_prescale'd matrix and the descale factor."""
    from .packing import frag_major, frag_major_split, pow2_prescale
    if split:
        ws, wscale = pow2_prescale(w.cpu())
        return frag_major_split(ws).to(device), wscale
    return frag_major(w.cpu().to(dtype)).contiguous().to(device), 0.0


def _rows_out(out, M, N, dtype, device):
    """The output [M, N]: fresh, or the first M rows of a caller's buffer (which may hold more rows: the tests' guard rows)."""
    if out is None:
        return torch.empty(M, N, dtype=dtype, device=device)
    assert out.is_contiguous() and out.dtype == dtype and out.shape[0] >= M and tuple(out.shape[1:]) == (N,), (tuple(out.shape), M, N)
    return out


def pointwise_stream(a, wf, bias, N, relu=False, residual=None, residual_mode=L.RES_NONE, out_hw=None, split=False, wscale=0.0,
                     many_slices=False, blocks=None, grid_cap=0, out=None):
    """The streaming 1x1 kernels at any M (mcg_pointwise_stream; many_slices=True: dynamic_layer's forms, mcg_pointwise_dyn, N = 32768):
    a [M, K] (16-bit, or f32 with split=True), wf / wscale from pointwise_weights, bias f32 [N] -> y [M, N].  residual [M, N] (RES_ADD) or
    [frames, Hr, Wr, N] with out_hw = (Ho, Wo) and M = frames * Ho * Wo (RES_UPSAMPLE_ADD).  blocks: a sequence of 8 x 8 block ids, or a
    (list, count) pair of device int32 tensors as inner_mark_blocks returns -- the list form, which writes the listed blocks only (give
    ``out``).  grid_cap: include/mcgaze_hip.h.  out: a buffer of at least M rows."""
    _require_gpu()
    lib = L.load()
    M, K = a.shape
    code = L.MCG_F16X3 if split else _code(a.dtype)
    y = _rows_out(out, M, N, a.dtype, a.device)
    a = a.contiguous()
    if many_slices:
        assert residual is None and blocks is None and N == 32768 and K == 256
        L.check(lib.mcg_pointwise_dyn(_stream(), code, _ptr(a), _ptr(wf), _ptr(bias), _ptr(y), M, wscale, grid_cap), 'mcg_pointwise_dyn')
        return y
    mode = residual_mode if residual is not None else L.RES_NONE
    Ho, Wo = out_hw if out_hw is not None else (1, M)
    Hr, Wr = (residual.shape[1], residual.shape[2]) if mode == L.RES_UPSAMPLE_ADD else (Ho, Wo)
    blist = bcount = None
    if blocks is not None:
        blist, bcount = _block_list(blocks, a.device)
    L.check(lib.mcg_pointwise_stream(_stream(), code, _ptr(a), _ptr(wf), _ptr(bias), _ptr(residual.contiguous() if residual is not None else None),
                                     _ptr(y), M, K, N, int(relu), mode, Ho, Wo, Hr, Wr, wscale, _ptr(blist), _ptr(bcount), grid_cap),
            'mcg_pointwise_stream')
    return y


def pointwise_pair(a1, w3f, b3, w1f, b1, C2, a2=None, residual=None, grid_cap=0, out=None):
    """pw_pair.hpp's kernel at any M (mcg_pointwise_pair): a1 [M, 64], a2 [M, 64] or None, residual [M, 256] or None (16-bit), w3f / w1f
    from pointwise_weights (W3 [256, 64 (+ 64)], W1 [C2, 256]) -> (y [M, 256], z [M, C2]).  out: (y, z) buffers of at least M rows."""
    _require_gpu()
    lib = L.load()
    M = a1.shape[0]
    y = _rows_out(out[0] if out else None, M, 256, a1.dtype, a1.device)
    z = _rows_out(out[1] if out else None, M, C2, a1.dtype, a1.device)
    cont = lambda t: t.contiguous() if t is not None else None
    L.check(lib.mcg_pointwise_pair(_stream(), _code(a1.dtype), _ptr(a1.contiguous()), _ptr(cont(a2)), _ptr(cont(residual)), _ptr(w3f), _ptr(b3),
                                   _ptr(y), _ptr(w1f), _ptr(b1), _ptr(z), M, a2.shape[1] if a2 is not None else 0, C2, grid_cap), 'mcg_pointwise_pair')
    return y, z


def conv3x3_wino(x, w, bias=None, relu=False, tile=0, g=2):
    """3x3 / stride 1 / pad 1 conv by the 1-D Winograd F(2,3) kernel of the MCG_F16X3 engine (mcg_conv3x3_wino_x3, wino_x3.hpp):
    x NHWC f32, w OHWI f32 [Cout,3,3,Cin] (packed here by packing.wino_pack), bias f32 -> NHWC f32.  tile: 0 = by grid size, 1..4 forced
    (4 = the one-wave-per-SIMD 128 x 128 tile).
    g = 4: the F(4,3) form of the same kernel (maps whose width is a multiple of 4, at least 16)."""
    _require_gpu()
    lib = L.load()
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    u, wscale = wino_weights(w, g, x.device)
    assert u.numel() * 2 == lib.mcg_conv3x3_wino_x3_weight_bytes(Cin, Cout, g), (u.numel(), Cin, Cout)
    y = torch.empty(N, H, W, Cout, dtype=torch.float32, device=x.device)
    L.check(lib.mcg_conv3x3_wino_x3(_stream(), _ptr(x.contiguous()), _ptr(u), _ptr(bias), _ptr(y), N, H, W, Cin, Cout, int(relu), tile, wscale, g), 'mcg_conv3x3_wino_x3')
    return y


def _block_list(blocks, device):
    """A host sequence of block ids, or a (list, count) pair of device int32 tensors (count: one element; the kernels read *count entries
    of list) -> that pair on ``device``."""
    if isinstance(blocks, tuple) and len(blocks) == 2 and all(isinstance(t, torch.Tensor) for t in blocks):
        blist, bcount = blocks
        for t in (blist, bcount):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.device == torch.device(device), (t.dtype, t.device)
        assert blist.dim() == 1 and blist.numel() >= 1 and bcount.numel() == 1
        return blist, bcount
    ids = _flat_ints(blocks, 'blocks must be a flat sequence', 'blocks must be integers', False)
    blist = torch.zeros(max(len(ids), 1), dtype=torch.int32, device=device)
    blist[:len(ids)] = torch.from_numpy(ids.astype(np.int32)).to(device)
    return blist, torch.tensor([len(ids)], dtype=torch.int32, device=device)


def wino_weights(w, g=2, device='cuda'):
    """w OHWI f32 [Cout,3,3,Cin] -> (u, wscale): the weight operand of conv3x3_wino / conv3x3_wino_blocks (packing.wino_pack of the
    pow2_prescale'd tensor) and the descale factor."""
    from .packing import pow2_prescale, wino_pack
    ws, wscale = pow2_prescale(w.cpu())
    return wino_pack(ws, g=g).to(device), wscale


def conv3x3_wino_blocks(x, packed, blocks, out, bias=None, relu=False, grid_cap=0):
    """The block tile of conv3x3_wino (mcg_conv3x3_wino_x3_blocks; wino_x3w_blocks_kernel): x NHWC f32 with H and W multiples of 8, packed =
    wino_weights(w) (g = 2), out NHWC f32 [N,H,W,Cout] -- the listed 8 x 8 blocks of it are written, the rest is left alone.  blocks: a
    sequence of block ids or a (list, count) pair of device int32 tensors (roi_mark_blocks); the capacity of list sizes the grid.  THE IDS
    MUST BE DISTINCT AND INSIDE [0, N * (H / 8) * (W / 8)) and count at most the capacity: the kernel does not guard them."""
    _require_gpu()
    lib = L.load()
    N, H, W, Cin = x.shape
    u, wscale = packed
    Cout = out.shape[-1]
    assert x.dtype == torch.float32 and x.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (N, H, W, Cout)
    assert u.numel() * 2 == lib.mcg_conv3x3_wino_x3_weight_bytes(Cin, Cout, 2), (u.numel(), Cin, Cout)
    blist, bcount = _block_list(blocks, x.device)
    L.check(lib.mcg_conv3x3_wino_x3_blocks(_stream(), _ptr(x), _ptr(u), _ptr(bias), _ptr(out), N, H, W, Cin, Cout, int(relu), wscale,
                                           _ptr(blist), _ptr(bcount), blist.numel(), grid_cap), 'mcg_conv3x3_wino_x3_blocks')
    return out


def conv3x3_wino_frames(x, u, frames, out, bias=None, grid_cap=0):
    """The frame-list tile of conv3x3_wino (mcg_conv3x3_wino_x3_frames; wino_x3w_frames_kernel): x NHWC f32, u = packing.wino_pack(w) of the
    UNSCALED weight (the entry takes no descale factor), out NHWC f32 [N,H,W,Cout] -- the listed frames of it are written, the rest is left
    alone.  frames: a sequence of frame indices or a (list, count) pair of device int32 tensors (roi_mark_frames), list N long.  THE
    INDICES MUST BE DISTINCT; one outside [0, N) is skipped and a count above N is clamped on the device."""
    _require_gpu()
    lib = L.load()
    N, H, W, Cin = x.shape
    Cout = out.shape[-1]
    assert x.dtype == torch.float32 and x.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (N, H, W, Cout)
    assert u.numel() * 2 == lib.mcg_conv3x3_wino_x3_weight_bytes(Cin, Cout, 2), (u.numel(), Cin, Cout)
    flist, fcount = _block_list(frames, x.device)
    if flist.numel() < N:
        flist = torch.cat([flist, torch.zeros(N - flist.numel(), dtype=torch.int32, device=x.device)])
    L.check(lib.mcg_conv3x3_wino_x3_frames(_stream(), _ptr(x), _ptr(u), _ptr(bias), _ptr(out), N, H, W, Cin, Cout, _ptr(flist), _ptr(fcount),
                                           grid_cap), 'mcg_conv3x3_wino_x3_frames')
    return out


def roi_mark_frames(boxes, level, state=None, flist=None, count=None):
    """Which frames read pyramid level ``level`` (0 .. 3) for these boxes (mcg_roi_mark_frames; roi_mark_kernel's frame marking): boxes
    [N,P,4] f32 -> (state, list, count), int32 device tensors: state [N] flags, list the frames newly flagged in unspecified order, count
    [1] how many.  Given buffers are added to (a frame whose state is set is not listed again; count is not reset); None: fresh zeroed
    ones."""
    _require_gpu()
    lib = L.load()
    N, P, _ = boxes.shape
    assert boxes.dtype == torch.float32
    state, flist, count = _mark_buffers(N, state, flist, count, boxes.device)
    L.check(lib.mcg_roi_mark_frames(_stream(), _ptr(boxes.contiguous()), N * P, P, int(level), _ptr(state), _ptr(flist), _ptr(count)),
            'mcg_roi_mark_frames')
    return state, flist, count


def bottleneck_x3(x, src2, wstream, bias, cn, nsrc, trace=None):
    """The fused bottleneck tail (mcg_bottleneck_x3): x [N,H,W,cm] f32 = conv2's input (cm = 64 / 128), src2 = residual [N,H,W,4 cm]
    (nsrc 1) or the downsample conv's input [N,H,W,64] (nsrc 2); wstream / bias from packing.bneck_stream.
    -> (y [N,H,W,4 cm], z [N,H,W,cn] or None)."""
    _require_gpu()
    lib = L.load()
    N, H, W, cm = x.shape
    y = torch.empty(N, H, W, 4 * cm, dtype=torch.float32, device=x.device)
    z = torch.empty(N, H, W, cn, dtype=torch.float32, device=x.device) if cn else None
    L.check(lib.mcg_bottleneck_x3(_stream(), _ptr(x.contiguous()), _ptr(src2.contiguous()), _ptr(wstream), _ptr(bias), _ptr(y), _ptr(z),
                                  N, H, W, cm, nsrc, cn, _ptr(trace)), 'mcg_bottleneck_x3')
    return y, z


def stem(img, w_stem, bias, dtype, flags=0, split=False):
    """img [N,3,H,W] f32 -> [N,H/4,W/4,64] NHWC.  mcg_stem_forward."""
    _require_gpu()
    lib = L.load()
    N, _, H, W = img.shape
    code = L.MCG_F16X3 if split else _code(dtype)
    ws = _ws(lib.mcg_stem_workspace_bytes(code, N, H, W), img.device)
    y = torch.empty(N, H // 4, W // 4, 64, dtype=dtype, device=img.device)
    L.check(lib.mcg_stem_forward(_stream(), code, _ptr(img.contiguous()), _ptr(w_stem), _ptr(bias), _ptr(y), N, H, W,
                                 _ptr(ws), ws.numel(), flags), 'mcg_stem_forward')
    return y


def roi_align(feats, boxes, strides=(4, 8, 16, 32)):
    """feats: 4 NHWC levels; boxes [N,P,4] f32 -> ([N*P,49,C], levels int32 [N*P]).  mcg_roi_align."""
    return roi_align_indexed(feats, boxes, None, strides)


def _mark_buffers(nblk, state, blist, count, device):
    """The caller's (state, list, count) of a marking call, or fresh zeroed ones: int32 device tensors, state and list nblk long."""
    z = lambda n: torch.zeros(n, dtype=torch.int32, device=device)
    state, blist, count = (z(nblk) if state is None else state), (z(nblk) if blist is None else blist), (z(1) if count is None else count)
    for t in (state, blist, count):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.device == torch.device(device), (t.dtype, t.device)
    assert state.numel() == nblk and blist.numel() >= nblk and count.numel() == 1, (state.numel(), blist.numel(), nblk)
    return state, blist, count


def roi_mark_blocks(boxes, hw, level=0, stride=4, state=None, blist=None, count=None):
    """Which 8 x 8 blocks of ONE pyramid level roi_align reads for these boxes (mcg_roi_mark_blocks; roi_mark_kernel): boxes [N,P,4] f32,
    hw = (H, W) of the level -> (state, list, count), int32 device tensors: state [N * by_n * bx_n] flags, list the ids newly flagged in
    unspecified order, count [1] how many.  Given buffers are added to (a block whose state is set is not listed again; count is not
    reset; list must have room for count + the new ids); None: fresh zeroed ones."""
    _require_gpu()
    lib = L.load()
    N, P = boxes.shape[:2]
    H, W = hw
    b = boxes.contiguous().float()
    state, blist, count = _mark_buffers(N * ((H + 7) // 8) * ((W + 7) // 8), state, blist, count, b.device)
    L.check(lib.mcg_roi_mark_blocks(_stream(), _ptr(b), N * P, P, level, H, W, stride, _ptr(state), _ptr(blist), _ptr(count)), 'mcg_roi_mark_blocks')
    return state, blist, count


def inner_mark_blocks(out_list, out_count, hw, frames, state=None, blist=None, count=None):
    """The inner blocks the listed output blocks' 3 x 3 convs read (mcg_inner_mark_blocks; inner_mark_kernel): out_list / out_count as
    roi_mark_blocks returns them (out_list at least frames * by_n * bx_n long), hw = (H, W) of the map -> (state, list, count) as there:
    the listed blocks and their in-frame neighbours that ``state`` did not hold."""
    _require_gpu()
    lib = L.load()
    H, W = hw
    nblk = frames * ((H + 7) // 8) * ((W + 7) // 8)
    state, blist, count = _mark_buffers(nblk, state, blist, count, out_list.device)
    _mark_buffers(nblk, state, out_list, out_count, out_list.device)
    L.check(lib.mcg_inner_mark_blocks(_stream(), _ptr(out_list), _ptr(out_count), H, W, nblk, _ptr(state), _ptr(blist), _ptr(count)), 'mcg_inner_mark_blocks')
    return state, blist, count


def roi_align_indexed(feats, boxes, frame_of, strides=(4, 8, 16, 32)):
    """roi_align over window frames gathered from a pyramid store: box row r reads pyramid row frame_of[r // P].
    feats: 4 NHWC levels [K,h,w,C]; boxes [N,P,4] f32; frame_of: N row indices (host, range-checked) -> ([N*P,49,C], levels).
    mcg_roi_align_indexed.  frame_of None: frame n reads row n (roi_align)."""
    _require_gpu()
    lib = L.load()
    N, P = boxes.shape[:2]
    K, Cc = feats[0].shape[0], feats[0].shape[-1]
    name, gather = 'mcg_roi_align', ()
    if frame_of is not None:
        table = torch.from_numpy(check_frame_table(frame_of, K, 1)).to(boxes.device)
        if table.numel() != N:
            raise L.McgError(f'frame_of holds {table.numel()} entries for {N} frames of boxes')
        name, gather = 'mcg_roi_align_indexed', (_ptr(table), K)
    out = torch.empty(N * P, 49, Cc, dtype=feats[0].dtype, device=boxes.device)
    lv = torch.empty(N * P, dtype=torch.int32, device=boxes.device)
    fp = (C.c_void_p * 4)(*[f.data_ptr() for f in feats])
    fh = (C.c_int * 4)(*[f.shape[1] for f in feats])
    fw = (C.c_int * 4)(*[f.shape[2] for f in feats])
    st = (C.c_int * 4)(*strides)
    b = boxes.contiguous().float()
    L.check(getattr(lib, name)(_stream(), _code(feats[0].dtype), fp, fh, fw, st, Cc, _ptr(b), N * P, P, *gather, _ptr(out), _ptr(lv)), name)
    return out, lv


def _flat_ints(seq, must, must_int, nonempty):
    """A sequence (or CPU tensor) -> 1-D numpy array of integers; McgError(must ...) if it is no flat sequence, McgError(must_int ...) if
    it is not one of integers (or is empty where nonempty)."""
    t = seq.numpy() if isinstance(seq, torch.Tensor) else seq
    try:
        a = np.asarray(t)
    except Exception as ex:                          # ragged input
        raise L.McgError(f'{must} ({ex})')
    if a.ndim != 1 or (nonempty and a.size == 0) or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise L.McgError(f'{must_int} (got {a.dtype} of shape {a.shape})')
    return a


def check_frame_table(frame_of, pyramid_frames, clip_length):
    """Host-side check of a window-frame -> pyramid-row table: a sequence (or CPU tensor) of integers, a positive multiple of
    clip_length long, every entry in [0, pyramid_frames).  -> int32 numpy array.  McgError otherwise (nothing reaches the device)."""
    a = _flat_ints(frame_of, 'frame_of must be a flat sequence of row indices', 'frame_of must be a flat sequence of integer row indices', False)
    if clip_length < 1 or a.size == 0 or a.size % clip_length:
        raise L.McgError(f'frame_of holds {a.size} entries, not a positive multiple of clip_length={clip_length}')
    if pyramid_frames < 1 or int(a.min()) < 0 or int(a.max()) >= pyramid_frames:
        raise L.McgError(f'frame_of entries must lie in [0, {pyramid_frames}) (got {int(a.min())} .. {int(a.max())})')
    return a.astype(np.int32)


def check_row_table(rows, store_rows, num_frames):
    """Host-side check of a frame -> store-row table (backbone_fpn_rows): a sequence (or CPU tensor) of num_frames integers, every entry in
    [0, store_rows), no row named twice.  -> int32 numpy array.  McgError otherwise (nothing reaches the device)."""
    a = _flat_ints(rows, 'rows must be a flat sequence of row indices', 'rows must be a flat sequence of integer row indices', False)
    if a.size != int(num_frames):
        raise L.McgError(f'rows holds {a.size} entries for {int(num_frames)} frames')
    if a.size and (store_rows < 1 or int(a.min()) < 0 or int(a.max()) >= store_rows):
        raise L.McgError(f'rows entries must lie in [0, {store_rows}) (got {int(a.min())} .. {int(a.max())})')
    if a.size > 1 and len(set(a.tolist())) != a.size:
        u, n = np.unique(a, return_counts=True)
        raise L.McgError(f'rows names row {int(u[n.argmax()])} for {int(n.max())} frames: every frame needs a row of its own')
    return a.astype(np.int32)


def check_clip_lengths(lengths, num_frames):
    """Host-side check of a ragged batch's clip lengths: a non-empty flat sequence of positive integers summing to num_frames
    (None: any sum).
    -> int32 numpy array clip_start [len(lengths) + 1] (0, cumulative sums: the table the mcg_*_ragged entry points take).
    McgError otherwise (nothing reaches the device)."""
    a = _flat_ints(lengths, 'clip lengths must be a flat sequence of integers', 'clip lengths must be a non-empty flat sequence of integers', True)
    if int(a.min()) < 1:
        raise L.McgError(f'every clip must hold at least one frame (got a length of {int(a.min())})')
    total = int(a.astype(np.int64).sum())
    if num_frames is not None and total != int(num_frames):
        raise L.McgError(f'clip lengths sum to {total} frames, the batch holds {int(num_frames)}')
    start = np.zeros(a.size + 1, dtype=np.int32)
    np.cumsum(a, out=start[1:])
    return start


class ClipTable:
    """The clip lengths of a ragged batch, checked and uploaded ONCE: what forward / decode / stage_forward build per call from a sequence
    of lengths, for a caller who repeats a batch layout -- and the form to use under HIP-graph capture, where a per-call upload from a
    temporary host buffer must not be recorded (GraphedForward builds one).  The upload is complete when the constructor returns."""

    def __init__(self, lengths, device='cuda:0'):
        self.start = check_clip_lengths(lengths, None)
        self.num_frames, self.num_clips, self.max_len = int(self.start[-1]), self.start.size - 1, int(np.diff(self.start).max())
        self.device = torch.device(device)
        self.table = torch.from_numpy(self.start).to(self.device)


def _upload_table(table, device):
    """A small host table (numpy array or CPU tensor: clip starts, frame rows, img_shape, scale_factor) -> device tensor, pinned +
    non-blocking on the current stream: a pageable upload would make the host wait for the work already queued (the host then idles for
    the previous batch instead of preparing the next).  A CPU ``device`` (the oracle behind harness.run_videos) gets the tensor itself."""
    t = torch.as_tensor(table)
    return t.pin_memory().to(device, non_blocking=True) if torch.device(device).type == 'cuda' else t.to(device)


def _outputs(N, device, alloc=torch.empty):
    """The result dict of forward / decode over N frames: f32 device tensors."""
    return dict(gaze=alloc(4, N, 3, dtype=torch.float32, device=device), boxes=alloc(N, 3, 4, dtype=torch.float32, device=device),
                scores=alloc(N, 3, dtype=torch.float32, device=device))


class _Clips:
    """clip_length of forward / decode / stage_forward, as the C-ABI takes it.  An int (one length for every clip): ``args`` is that int,
    for the mcg_* entry point.  A sequence of lengths or a ClipTable: ``args`` is (device int32 clip_start, num_clips, max_clip_length) for
    the mcg_*_ragged one (which rejects a null table).  A sequence is checked (McgError before anything reaches the device) and uploaded
    per call (_upload_table); ``pick(fixed, ragged)`` names the entry point that takes ``args`` in the clip position."""

    def __init__(self, clip_length, num_frames, device):
        self.ragged = not isinstance(clip_length, (int, np.integer))
        if not self.ragged:
            self.args = (clip_length,)
        elif isinstance(clip_length, ClipTable):
            ct = clip_length
            if ct.num_frames != num_frames or ct.device != torch.device(device):
                raise L.McgError(f'the ClipTable holds {ct.num_frames} frames on {ct.device}, the batch {num_frames} on {device}')
            self.table, self.args = ct.table, (_ptr(ct.table), ct.num_clips, ct.max_len)
        else:
            start = check_clip_lengths(clip_length, num_frames)
            self.table = _upload_table(start, device)           # held: args carries its address only
            self.args = (_ptr(self.table), start.size - 1, int(np.diff(start).max()))

    def pick(self, fixed, ragged):
        return ragged if self.ragged else fixed


def _table(d, keys):
    return (C.c_void_p * len(keys))(*[d[k].data_ptr() for k in keys])


def stage_forward(stage_w, roi_feat, obj, boxes, clip_length, stds=(0.5, 0.5, 1.0, 1.0), split=False, flags=0):
    """One decoder stage.  roi_feat [R,49,256], obj [N,3,256], boxes [N,3,4] f32
    -> (obj' [N,3,256], boxes' [N,3,4], cls logits [N,3]).  mcg_stage_forward; clip_length: an int, or a sequence of per-clip lengths
    summing to N (mcg_stage_forward_ragged)."""
    _require_gpu()
    lib = L.load()
    N = obj.shape[0]
    dt = L.MCG_F16X3 if split else _code(obj.dtype)   # split: stage_w from PackedWeights(split=True), f32 activations
    ws = _ws(lib.mcg_stage_workspace_bytes(dt, N), obj.device)
    obj_out = torch.empty_like(obj)
    boxes_out = torch.empty(N, 3, 4, dtype=torch.float32, device=obj.device)
    cls = torch.empty(N, 3, dtype=torch.float32, device=obj.device)
    sd = (C.c_float * 4)(*stds)
    clips = _Clips(clip_length, N, obj.device)
    name = clips.pick('mcg_stage_forward', 'mcg_stage_forward_ragged')
    L.check(getattr(lib, name)(_stream(), dt, _table(stage_w, L.STAGE_KEYS), _ptr(roi_feat.contiguous()), _ptr(obj.contiguous()),
                               _ptr(boxes.contiguous().float()), N, *clips.args, _ptr(obj_out), _ptr(boxes_out), _ptr(cls), sd, _ptr(ws), ws.numel(),
                               flags), name)
    return obj_out, boxes_out, cls


def gaze_head(gaze_w, obj, split=False):
    """obj [N,3,256] -> [4,N,3] f32 unit vectors (fused, face, eyes, head).  mcg_gaze_head."""
    _require_gpu()
    lib = L.load()
    N = obj.shape[0]
    dt = L.MCG_F16X3 if split else _code(obj.dtype)
    ws = _ws(lib.mcg_gaze_head_workspace_bytes(dt, N), obj.device)
    out = torch.empty(4, N, 3, dtype=torch.float32, device=obj.device)
    L.check(lib.mcg_gaze_head(_stream(), dt, _table(gaze_w, L.GAZE_KEYS), _ptr(obj.contiguous()), N, _ptr(out), _ptr(ws), ws.numel()), 'mcg_gaze_head')
    return out


# ------------------------------------------------------------------------------------ engine
class HipEngine:
    """The whole per-clip forward path behind one C call (mcg_clip_forward)."""

    def __init__(self, state_dict, depth=50, num_stages=4, precision='f16x3', device='cuda:0', bbox_stds=(0.5, 0.5, 1.0, 1.0), fuse_downsample=True):
        _require_gpu()
        self.lib = L.load()
        self.device = torch.device(device)
        self.dtype = _TORCH_DT[precision]
        self.code = _CODE[precision]
        self.precision = precision
        self.weights = PackedWeights(state_dict, depth=depth, num_stages=num_stages, dtype=self.dtype, device=self.device,
                                     fuse_downsample=fuse_downsample, split=self.code == L.MCG_F16X3)
        w = self.weights
        mk = lambda c: L.ConvWeights(c['w'].data_ptr(), c['bias'].data_ptr(), c['cin'], c['cout'], c['k'], c['stride'], c['pad'],
                                     c['wf'].data_ptr() if c.get('wf') is not None else None, float(c.get('wscale', 0.0)),
                                     c['wf4'].data_ptr() if c.get('wf4') is not None else None)
        self._convs = (L.ConvWeights * len(w.convs))(*[mk(c) for c in w.convs])
        self._stage_tab = (C.c_void_p * (num_stages * L.SW_COUNT))(*[st[k].data_ptr() for st in w.stages for k in L.STAGE_KEYS])
        self._gaze_tab = _table(w.gaze, L.GAZE_KEYS)
        mw = L.ModelWeights()
        mw.blocks = (C.c_int * 4)(*w.blocks)
        mw.stem = mk(w.stem)
        mw.convs = C.cast(self._convs, C.POINTER(L.ConvWeights))
        mw.num_convs = len(w.convs)
        mw.lateral = (L.ConvWeights * 4)(*[mk(c) for c in w.lateral])
        mw.fpn_out = (L.ConvWeights * 4)(*[mk(c) for c in w.fpn_out])
        if len(w.c3_ds) == 4:
            mw.c3_ds = (L.ConvWeights * 4)(*[mk(c) for c in w.c3_ds])
        mw.init_boxes = w.init_boxes.data_ptr()
        mw.init_feats = w.init_feats.data_ptr()
        mw.num_stages = num_stages
        mw.stage_weights = C.cast(self._stage_tab, C.POINTER(C.c_void_p))
        mw.gaze_weights = C.cast(self._gaze_tab, C.POINTER(C.c_void_p))
        mw.bbox_stds = (C.c_float * 4)(*bbox_stds)
        if w.fused:
            self._fused = (L.FusedBlock * len(w.fused))(*[L.FusedBlock(f['wstream'].data_ptr(), f['bias'].data_ptr(), f['conv2_index'], f['cm'], f['c'],
                                                                      f['cn'], f['nsrc']) for f in w.fused])
            mw.fused, mw.num_fused = C.cast(self._fused, C.POINTER(L.FusedBlock)), len(w.fused)
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):   # the engine's side streams and events belong to THIS device
            L.check(self.lib.mcg_engine_create(C.byref(self._handle), C.byref(mw), self.code), 'mcg_engine_create')
        self._ws = None
        self._dec_ws = None
        self._row_ws = None

    def set_option(self, name, value):
        """mcg_engine_set_option: 'trunk_streams', 'max_range_frames', 'tile', 'staged_gemm', 'conv3x3_c64', 'stem_fused',
        'decoder_chain', 'decoder_attn_block', 'pointwise_pair', 'pointwise_stream', 'bottleneck_fused', 'bottleneck_blocked', 'winograd',
        'wino_tile', 'fpn_deferred', 'fpn_lateral_deferred', 'fpn_levels_deferred', 'range_audit'; values and defaults in include/mcgaze_hip.h."""
        L.check(self.lib.mcg_engine_set_option(self._handle, name.encode(), int(value)), f'mcg_engine_set_option({name})')

    def range_audit(self, capacity=256):
        """Read and reset the range audit (set_option('range_audit', 1) first): [(tensor name, values with |x| > 65504, non-finite values)]
        over every frame the trunk processed since the last read.  mcg_engine_range_audit (a debug call: it synchronises the device)."""
        counts = (C.c_ulonglong * (2 * capacity))()
        names = (C.c_char_p * capacity)()
        n = C.c_int()
        L.check(self.lib.mcg_engine_range_audit(self._handle, counts, names, capacity, C.byref(n)), 'mcg_engine_range_audit')
        return [(names[i].decode(), int(counts[2 * i]), int(counts[2 * i + 1])) for i in range(n.value)]

    def profile_start(self, capacity=4096):
        L.check(self.lib.mcg_engine_profile_start(self._handle, capacity), 'mcg_engine_profile_start')

    def profile_stop(self, capacity=4096):
        """-> list of (ms, algorithmic flops, cfg id, (M, N, K), algorithmic HBM bytes) per contraction launch recorded since profile_start."""
        cnt = C.c_int()
        ms = (C.c_float * capacity)(); fl = (C.c_double * capacity)(); by = (C.c_double * capacity)()
        cf = (C.c_int * capacity)(); sh = (C.c_int * (3 * capacity))()
        L.check(self.lib.mcg_engine_profile_stop(self._handle, C.byref(cnt), ms, fl, by, cf, sh, capacity), 'mcg_engine_profile_stop')
        return [(ms[i], fl[i], cf[i], (sh[3 * i], sh[3 * i + 1], sh[3 * i + 2]), by[i]) for i in range(cnt.value)]

    def backbone_only(self, img, return_levels=False):
        """BASELINE.json configs[1] measurement: the trunk up to C5 (mcg_bench_backbone_forward).  return_levels: C2..C5 as NHWC views
        into the engine's workspace (valid until the next call; needs the batch to run as one frame range: set_option('trunk_streams', 1))."""
        self._check_img(img)
        N, _, H, W = img.shape
        with torch.cuda.device(self.device):
            ws = self._workspace(N, H, W, 0)
            L.check(self.lib.mcg_bench_backbone_forward(self._handle, _stream(self.device), _ptr(img), N, H, W, _ptr(ws), ws.numel()), 'mcg_bench_backbone_forward')
            if not return_levels:
                return None
            tab = (C.c_void_p * 4)()
            L.check(self.lib.mcg_bench_backbone_levels(self._handle, _ptr(ws), N, H, W, tab), 'mcg_bench_backbone_levels')
            es = ws.element_size() * (2 if self.dtype in (torch.bfloat16, torch.float16) else 4)
            out = []
            for i in range(4):
                shape = (N, (H // 4) >> i, (W // 4) >> i, 256 << i)
                n = shape[0] * shape[1] * shape[2] * shape[3]
                off = tab[i] - ws.data_ptr()
                out.append(ws[off:off + n * es].view(self.dtype).view(shape))
            return out

    def __del__(self):
        h = getattr(self, '_handle', None)
        if h is not None and h.value:
            self.lib.mcg_engine_destroy(h)
            self._handle = None

    def _grown(self, name, need):
        """The engine's grow-only buffer ``name`` (_ws: whole forward; _dec_ws: decode), at least ``need`` bytes."""
        if getattr(self, name) is None or getattr(self, name).numel() < need:
            setattr(self, name, None)                  # release the old block before asking for the larger one
            setattr(self, name, _ws(need, self.device))
        return getattr(self, name)

    def _workspace(self, N, H, W, chunk):
        return self._grown('_ws', self.lib.mcg_engine_workspace_bytes(self._handle, N, H, W, chunk))

    def _check_img(self, img):
        if not (img.is_cuda and img.device == self.device and img.dtype == torch.float32 and img.is_contiguous() and img.dim() == 4):
            raise L.McgError(f'img must be a contiguous float32 [N,3,H,W] tensor on {self.device} (got {img.dtype} {tuple(img.shape)} on {img.device})')

    def backbone_fpn(self, img, chunk_frames=0, out=None, row=0):
        """img [N,3,H,W] f32 on the device -> [P2..P5] NHWC in the engine dtype.
        out: four per-level tensors [K, H/4 >> i, W/4 >> i, 256] (engine dtype, contiguous) -- a pyramid STORE: the frames are written to
        rows [row, row + N) of it (the trunk of a frame does not depend on its batch, so a row holds the bits a whole-batch call gives)
        and ``out`` is returned."""
        self._check_img(img)
        N, _, H, W = img.shape
        shapes = [((H // 4) >> i, (W // 4) >> i, 256) for i in range(4)]
        if out is not None:
            K = self._check_pyramid(out, shapes)
            if not (0 <= row and row + N <= K):
                raise L.McgError(f'backbone_fpn: rows [{row}, {row + N}) do not fit a pyramid store of {K} rows')
        with torch.cuda.device(self.device):
            ws = self._workspace(N, H, W, chunk_frames)
            if out is None:
                pyr, row = [torch.empty((N,) + s, dtype=self.dtype, device=self.device) for s in shapes], 0
            else:
                pyr = out
            es = pyr[0].element_size()
            tab = (C.c_void_p * 4)(*[p.data_ptr() + row * s[0] * s[1] * s[2] * es for p, s in zip(pyr, shapes)])
            L.check(self.lib.mcg_backbone_fpn_forward(self._handle, _stream(self.device), _ptr(img), N, H, W, chunk_frames, tab, _ptr(ws), ws.numel()),
                    'mcg_backbone_fpn_forward')
        return pyr

    def backbone_fpn_rows(self, img, store_levels, rows, chunk_frames=0):
        """backbone_fpn into ARBITRARY rows of a pyramid store: frame n of img [N,3,H,W] is written to row rows[n] of store_levels (four
        per-level tensors like backbone_fpn's ``out``).  rows: a host sequence of N distinct rows, checked here (check_row_table: McgError
        before anything reaches the device).  The trunk runs into a scratch pyramid the engine owns (grown on demand, reused), then ONE
        launch copies every frame to its row (mcg_pyramid_scatter_rows) on the same stream: a row holds the bits backbone_fpn(out=, row=)
        writes.  Rows that are one ascending run (a single frame always is) need no copy: the trunk writes them in place, at the run's row
        offset.  -> store_levels."""
        K = store_levels[0].shape[0] if len(store_levels) else 0
        table = check_row_table(rows, K, img.shape[0])
        if table.size and bool((np.diff(table) == 1).all()):
            return self.backbone_fpn(img, chunk_frames, out=store_levels, row=int(table[0]))
        self._check_img(img)
        N, _, H, W = img.shape
        shapes = [((H // 4) >> i, (W // 4) >> i, 256) for i in range(4)]
        self._check_pyramid(store_levels, shapes)
        if N == 0:
            return store_levels
        with torch.cuda.device(self.device):
            es = store_levels[0].element_size()
            sizes = [N * s[0] * s[1] * s[2] * es for s in shapes]          # multiples of 512: every level of the scratch stays aligned
            scratch = self._grown('_row_ws', sum(sizes))
            src = (C.c_void_p * 4)(*[scratch.data_ptr() + sum(sizes[:i]) for i in range(4)])
            dst = (C.c_void_p * 4)(*[p.data_ptr() for p in store_levels])
            ws = self._workspace(N, H, W, chunk_frames)
            L.check(self.lib.mcg_backbone_fpn_forward(self._handle, _stream(self.device), _ptr(img), N, H, W, chunk_frames, src, _ptr(ws), ws.numel()),
                    'mcg_backbone_fpn_forward')
            dev_rows = _upload_table(table, self.device)
            L.check(self.lib.mcg_pyramid_scatter_rows(_stream(self.device), self.code, src, dst, N, K, H, W, _ptr(dev_rows)), 'mcg_pyramid_scatter_rows')
        return store_levels

    def _check_pyramid(self, pyramid, shapes=None):
        """-> rows K of a pyramid store (four contiguous [K,h,w,256] tensors of the engine dtype on its device, h, w halving per level)."""
        if len(pyramid) != 4:
            raise L.McgError(f'a pyramid is four levels (got {len(pyramid)})')
        K = pyramid[0].shape[0]
        if shapes is None:
            h, w = pyramid[0].shape[1], pyramid[0].shape[2]
            shapes = [(h >> i, w >> i, 256) for i in range(4)]
        for i, (p, s) in enumerate(zip(pyramid, shapes)):
            if not (p.dtype == self.dtype and p.device == self.device and p.is_contiguous() and tuple(p.shape) == (K,) + tuple(s)):
                raise L.McgError(f'pyramid level {i} must be a contiguous {self.dtype} [{K},{s[0]},{s[1]},256] tensor on {self.device} '
                                 f'(got {p.dtype} {tuple(p.shape)} on {p.device})')
        return K

    def decode(self, pyramid, frame_of, clip_length, img_hw=None, out=None):
        """The decoder over window frames gathered from a pyramid STORE (mcg_decoder_forward_indexed): window frame n reads pyramid row
        frame_of[n].  pyramid: four [K,h,w,256] tensors (backbone_fpn(..., out=)); frame_of: N = windows * clip_length row indices, a host
        sequence (range-checked here, McgError) or an int32 tensor (a DEVICE table is the caller's responsibility: the kernels clamp
        the address of an index outside [0, K) and write NaN for that frame); img_hw: img_shape (h, w) per pyramid ROW [K,2] or None.
        clip_length: an int, or a sequence of per-clip lengths summing to N -- clips of different lengths (mcg_decoder_forward_ragged).
        Returns dict(gaze [4,N,3], boxes [N,3,4], scores [N,3]) like forward -- bit for bit forward's on the stacked window frames."""
        K = pyramid[0].shape[0] if len(pyramid) else 0
        H, W = (pyramid[0].shape[1] * 4, pyramid[0].shape[2] * 4) if len(pyramid) else (0, 0)
        dev_table = isinstance(frame_of, torch.Tensor) and frame_of.device.type != 'cpu'
        ragged = not isinstance(clip_length, (int, np.integer))
        host = None if dev_table else check_frame_table(frame_of, K, 1 if ragged else clip_length)
        clips = _Clips(clip_length, frame_of.numel() if dev_table else host.size, self.device)
        self._check_pyramid(pyramid)
        with torch.cuda.device(self.device):
            if dev_table:
                if not (frame_of.dtype == torch.int32 and frame_of.device == self.device and frame_of.dim() == 1):
                    raise L.McgError(f'a device frame_of must be a 1-D int32 tensor on {self.device} (got {frame_of.dtype} {tuple(frame_of.shape)} on {frame_of.device})')
                table = frame_of.contiguous()
                if not ragged and (table.numel() == 0 or table.numel() % clip_length):
                    raise L.McgError(f'frame_of holds {table.numel()} entries, not a positive multiple of clip_length={clip_length}')
            else:
                table = _upload_table(host, self.device)
            N = table.numel()
            out = _outputs(N, self.device) if out is None else out
            hw = self.img_hw_tensor(img_hw, K)
            ws = self._grown('_dec_ws', self.lib.mcg_decoder_workspace_bytes(self._handle, N))
            tab = (C.c_void_p * 4)(*[p.data_ptr() for p in pyramid])
            name = clips.pick('mcg_decoder_forward_indexed', 'mcg_decoder_forward_ragged')
            L.check(getattr(self.lib, name)(self._handle, _stream(self.device), tab, K, _ptr(table), N, *clips.args, H, W, _ptr(hw), _ptr(out['gaze']),
                                            _ptr(out['boxes']), _ptr(out['scores']), _ptr(ws), ws.numel()), name)
        return out

    def forward(self, img, clip_length, img_hw=None, chunk_frames=0, out=None):
        """img [N,3,H,W] f32 (device, contiguous), N = clips*clip_length.
        clip_length: an int (every clip that long: mcg_clip_forward), or a sequence of per-clip lengths summing to N -- clips of different
        lengths, stacked in order (mcg_clip_forward_ragged; or a ClipTable built once); every clip's results are those of forward(img[a:b], b - a) bit for bit.
        Returns dict(gaze [4,N,3], boxes [N,3,4], scores [N,3]) -- f32 device tensors."""
        self._check_img(img)
        N, _, H, W = img.shape
        clips = _Clips(clip_length, N, self.device)
        name = clips.pick('mcg_clip_forward', 'mcg_clip_forward_ragged')
        with torch.cuda.device(self.device):
            ws = self._workspace(N, H, W, chunk_frames)
            out = _outputs(N, self.device) if out is None else out
            hw = self.img_hw_tensor(img_hw, N)
            L.check(getattr(self.lib, name)(self._handle, _stream(self.device), _ptr(img), N, *clips.args, H, W, _ptr(hw), chunk_frames, _ptr(out['gaze']),
                                            _ptr(out['boxes']), _ptr(out['scores']), _ptr(ws), ws.numel()), name)
        return out

    def img_hw_tensor(self, img_hw, N):
        """img_shape (h, w) per frame -> the device int32 [N,2] tensor the C-ABI takes (None stays None = every frame fills H x W)."""
        if img_hw is None:
            return None
        if not isinstance(img_hw, torch.Tensor):
            img_hw = torch.as_tensor(np.asarray(img_hw, dtype=np.int32).reshape(N, 2))
        hw = img_hw.to(device=self.device, dtype=torch.int32).contiguous()
        if hw.numel() != 2 * N:
            raise L.McgError(f'img_hw must hold {N} (h, w) pairs, got {tuple(hw.shape)}')
        return hw


class GraphedForward:
    """Latency path (BASELINE.json configs[0], the reference harness's usage: ONE clip per forward, tools/test_gaze360_gaze.py:107-111).
    A single 7-frame clip is ~170 short launches whose GPU time is far below their launch cost, so the whole forward --
    trunk, 4 x (RoIAlign + decoder stage), gaze head -- is captured ONCE into a HIP graph for a fixed (N, H, W, clip_length) and
    replayed: one graph launch per clip.  Inputs are copied into the graph's static buffer on the caller's stream; the
    returned tensors are the graph's static outputs (valid until the next call).  Results are bit-identical to engine.forward
    (tests/test_gpu_forward.py::test_graphed_forward_is_bit_identical).  clip_length may be a sequence of per-clip lengths: the clip table
    is then uploaded once, before the capture (ClipTable), and the graph holds the ragged call."""

    def __init__(self, engine, num_frames, H, W, clip_length, with_img_hw=False):
        e = self.e = engine
        dev = e.device
        if not isinstance(clip_length, (int, np.integer, ClipTable)):
            clip_length = ClipTable(clip_length, dev)
        self.N, self.T = num_frames, clip_length
        with torch.cuda.device(dev):
            self.img = torch.zeros(num_frames, 3, H, W, dtype=torch.float32, device=dev)
            self.hw = torch.zeros(num_frames, 2, dtype=torch.int32, device=dev) if with_img_hw else None
            if self.hw is not None:
                self.hw[:, 0], self.hw[:, 1] = H, W
            self.out = _outputs(num_frames, dev, torch.zeros)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):          # eager warm-up on the capture stream: workspace allocation, side-stream probe
                for _ in range(2):
                    e.forward(self.img, clip_length, img_hw=self.hw, out=self.out)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side):
                e.forward(self.img, clip_length, img_hw=self.hw, out=self.out)

    def __call__(self, img, img_hw=None):
        self.e._check_img(img)
        if tuple(img.shape) != tuple(self.img.shape):
            raise L.McgError(f'GraphedForward was captured for {tuple(self.img.shape)}, got {tuple(img.shape)}')
        self.img.copy_(img, non_blocking=True)
        if img_hw is not None:
            if self.hw is None:
                raise L.McgError('GraphedForward was captured without img_hw (with_img_hw=True to enable)')
            self.hw.copy_(self.e.img_hw_tensor(img_hw, self.N), non_blocking=True)
        self.graph.replay()
        return self.out


_PIPELINE_STREAMS = {}


def pipeline_streams(device, decoder_priority=-1):
    """The two streams of the batch pipeline, created ONCE per (device, priority) and shared by every runner of the process:
    streams created later in a process's life land on hardware queues that serialise against earlier ones (engine.hip,
    StreamPool), so a second runner with fresh streams loses the overlap the first one had."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), decoder_priority)
    if key not in _PIPELINE_STREAMS:
        _PIPELINE_STREAMS[key] = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev, priority=decoder_priority))
    return _PIPELINE_STREAMS[key]


class PipelinedRunner:
    """Two-deep software pipeline over successive batches (throughput serving): the decoder of batch k
    (4 x [RoIAlign + stage] + gaze head: ~110 short, latency-bound launches) runs on a second HIP stream and
    overlaps the trunk of batch k+1, whose large contraction kernels leave CUs idle only at their tails.
    Pyramid slots (mcg_deferred_pyramid_bytes: P2..P5, and the P2 inner map when the engine defers the P2 output conv to the decoder)
    are double-buffered; trunks serialise on stream A, decoders on stream B, ordered by events.
    Every submitted batch is fully processed once ``flush()`` returns control to the caller's stream.  A loop that owns the runner
    should submit from ``runner.sa`` itself (``with torch.cuda.stream(runner.sa): ...``): the caller-stream -> trunk-stream hand-over
    of each submit is then no cross-queue dependency (2 ms per pipeline fill + drain when the queues are idle; bench.py does this).
    clip_length: an int, or a sequence of per-clip lengths / a ClipTable -- every batch then holds clips of those lengths (the table is
    uploaded once, here; mcg_decoder_forward_deferred_ragged)."""

    def __init__(self, engine, num_frames, H, W, clip_length, chunk_frames=0, decoder_priority=-1):
        self.e, self.N, self.H, self.W, self.T, self.chunk = engine, num_frames, H, W, clip_length, chunk_frames
        dev, lib, h = engine.device, engine.lib, engine._handle
        if not isinstance(clip_length, (int, np.integer, ClipTable)):
            self.T = ClipTable(clip_length, dev)
        self.clips = _Clips(self.T, num_frames, dev)
        # the decoder's short launches get the high-priority queue so they slot in between the trunk's long kernels
        self.sa, self.sb = pipeline_streams(dev, decoder_priority)
        self.slots = [_ws(lib.mcg_deferred_pyramid_bytes(h, num_frames, H, W), dev) for _ in range(2)]
        self.trunk_ws = _ws(lib.mcg_trunk_workspace_bytes(h, num_frames, H, W, chunk_frames), dev)
        self.dec_ws = _ws(lib.mcg_decoder_workspace_bytes(h, num_frames), dev)
        self.trunk_done = [torch.cuda.Event() for _ in range(2)]
        self.dec_done = [torch.cuda.Event() for _ in range(2)]
        self.used = [False, False]
        self._hw_keep = [None, None]
        self.k = 0

    def submit(self, img, out, img_hw=None):
        """Enqueue one batch: img [N,3,H,W] f32 (must stay valid until its trunk ran), out = dict(gaze, boxes, scores)."""
        with torch.cuda.device(self.e.device):
            return self._submit(img, out, img_hw)

    def _submit(self, img, out, img_hw):
        e, lib, slot = self.e, self.e.lib, self.k & 1
        e._check_img(img)
        img_hw = e.img_hw_tensor(img_hw, self.N)
        if img_hw is not None:
            img_hw.record_stream(self.sb)       # allocated on the caller's stream, read by the decoder on sb: the caching allocator must
                                                # not hand the block out again before that read has happened
        self._hw_keep[slot] = img_hw
        cur = torch.cuda.current_stream(e.device)
        self.sa.wait_stream(cur)                       # input produced on the caller's stream
        if self.used[slot]:
            self.sa.wait_event(self.dec_done[slot])    # the decoder that read this pyramid slot has finished
        L.check(lib.mcg_backbone_fpn_forward_deferred(e._handle, C.c_void_p(self.sa.cuda_stream), _ptr(img), self.N, self.H, self.W, self.chunk,
                                                      _ptr(self.slots[slot]), self.slots[slot].numel(), _ptr(self.trunk_ws), self.trunk_ws.numel()),
                'mcg_backbone_fpn_forward_deferred')
        self.trunk_done[slot].record(self.sa)
        self.sb.wait_event(self.trunk_done[slot])
        name = self.clips.pick('mcg_decoder_forward_deferred', 'mcg_decoder_forward_deferred_ragged')
        L.check(getattr(lib, name)(e._handle, C.c_void_p(self.sb.cuda_stream), _ptr(self.slots[slot]), self.slots[slot].numel(), self.N, *self.clips.args,
                                   self.H, self.W, _ptr(img_hw), _ptr(out['gaze']), _ptr(out['boxes']), _ptr(out['scores']), _ptr(self.dec_ws),
                                   self.dec_ws.numel()), name)
        self.dec_done[slot].record(self.sb)
        self.used[slot] = True
        self.k += 1
        return self.dec_done[slot]

    def flush(self):
        """Make the caller's stream wait for every submitted batch."""
        cur = torch.cuda.current_stream(self.e.device)
        for slot in range(2):
            if self.used[slot]:
                cur.wait_event(self.dec_done[slot])
