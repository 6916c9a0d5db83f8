"""ctypes binding of ``libmcgaze_hip.so`` (C-ABI declared in ``include/mcgaze_hip.h``).

The product path has no CPU fallback: if the shared library is missing or fails to load,
``load()`` raises and every model built on it refuses to run.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MCGAZE_LIB') or os.path.join(_HERE, 'libmcgaze_hip.so')   # MCGAZE_LIB: A/B a second build on one box

MCG_OK = 0
MCG_F32, MCG_BF16, MCG_F16X3, MCG_F16 = 0, 1, 2, 3
ABI_VERSION = 20
RES_NONE, RES_ADD, RES_UPSAMPLE_ADD = 0, 1, 2
FLAG_STAGED_GEMM, FLAG_NO_SPECIALISED, FLAG_NO_ATTN_BLOCK = 1, 2, 4

# enum order of include/mcgaze_hip.h
STAGE_KEYS = [
    'IN_PROJ_W', 'IN_PROJ_B', 'OUT_PROJ_W', 'OUT_PROJ_B', 'ATTN_LN_G', 'ATTN_LN_B', 'DYN_W', 'DYN_B',
    'NORM_IN_G', 'NORM_IN_B', 'NORM_OUT_G', 'NORM_OUT_B', 'FC_W', 'FC_B', 'FC_LN_G', 'FC_LN_B', 'IIC_LN_G', 'IIC_LN_B',
    'FFN1_W', 'FFN1_B', 'FFN2_W', 'FFN2_B', 'FFN_LN_G', 'FFN_LN_B', 'CLS_FC_W', 'CLS_LN_G', 'CLS_LN_B',
    'REG_FC_W', 'REG_LN_G', 'REG_LN_B', 'HEAD_CLS_W', 'HEAD_CLS_B', 'HEAD_REG_W', 'HEAD_REG_B', 'OUT_PROJ_WF', 'CLS_FC_WF', 'REG_FC_WF', 'IN_PROJ_WF', 'DYN_WF']
GAZE_KEYS = ['FC_W', 'LN_G', 'LN_B', 'OUT_W', 'OUT_B', 'FUSE_W', 'FUSE_B']
SW_COUNT, GW_COUNT = len(STAGE_KEYS), len(GAZE_KEYS)

# every symbol include/mcgaze_hip.h declares
EXPORTS = ['mcg_abi_version', 'mcg_build_id', 'mcg_last_error', 'mcg_device_info', 'mcg_nchw_to_nhwc', 'mcg_nhwc_to_nchw', 'mcg_conv2d',
           'mcg_stem_workspace_bytes', 'mcg_stem_forward', 'mcg_roi_align', 'mcg_stage_workspace_bytes', 'mcg_stage_forward',
           'mcg_gaze_head_workspace_bytes', 'mcg_gaze_head', 'mcg_engine_create', 'mcg_engine_destroy',
           'mcg_engine_workspace_bytes', 'mcg_trunk_workspace_bytes', 'mcg_decoder_workspace_bytes', 'mcg_backbone_fpn_forward',
           'mcg_decoder_forward', 'mcg_clip_forward', 'mcg_preprocess_frames', 'mcg_engine_set_option', 'mcg_engine_profile_start',
           'mcg_engine_profile_stop', 'mcg_bench_backbone_forward', 'mcg_bottleneck_x3', 'mcg_bench_backbone_levels', 'mcg_conv3x3_wino_x3',
           'mcg_conv3x3_wino_x3_weight_bytes', 'mcg_engine_range_audit', 'mcg_roi_align_indexed', 'mcg_decoder_forward_indexed',
           'mcg_deferred_pyramid_bytes', 'mcg_deferred_pyramid_levels', 'mcg_backbone_fpn_forward_deferred', 'mcg_decoder_forward_deferred',
           'mcg_stage_forward_ragged', 'mcg_decoder_forward_ragged', 'mcg_decoder_forward_deferred_ragged', 'mcg_clip_forward_ragged',
           'mcg_pyramid_scatter_rows', 'mcg_preprocess_head_crops', 'mcg_merge_windows', 'mcg_smooth_gaze', 'mcg_preprocess_frames_nv12',
           'mcg_preprocess_head_crops_nv12', 'mcg_draw_gaze_arrows', 'mcg_draw_gaze_arrows_nv12',
           'mcg_detect_heads_workspace_bytes', 'mcg_detect_heads', 'mcg_letterbox_frames', 'mcg_letterbox_frames_nv12',
           'mcg_track_state_bytes', 'mcg_track_heads', 'mcg_track_heads_motion', 'mcg_live_slots', 'mcg_live_gate', 'mcg_live_lanes', 'mcg_live_gate_lanes',
           'mcg_deferred_pyramid_state', 'mcg_inner_block_neighbours', 'mcg_gaze_targets', 'mcg_gaze_dwell', 'mcg_gaze_targets_poly',
           'mcg_pointwise_stream', 'mcg_pointwise_dyn', 'mcg_pointwise_pair', 'mcg_draw_attention', 'mcg_draw_attention_nv12',
           'mcg_format_labels', 'mcg_draw_labels', 'mcg_draw_labels_nv12', 'mcg_gaze_heat_add', 'mcg_draw_heat', 'mcg_draw_heat_nv12',
           'mcg_anonymize_heads', 'mcg_anonymize_heads_nv12', 'mcg_roi_mark_blocks', 'mcg_inner_mark_blocks', 'mcg_conv3x3_wino_x3_blocks',
           'mcg_conv3x3_wino_x3_frames', 'mcg_roi_mark_frames', 'mcg_deferred_pyramid_frame_state', 'mcg_gaze_targets_3d', 'mcg_surface_heat_add',
           'mcg_draw_surface_heat', 'mcg_draw_surface_heat_nv12']
LABEL_CHARS = 24                                                 # MCG_LABEL_CHARS
SURFACE_CHART_BYTES = 160                                        # MCG_SURFACE_CHART_BYTES: a region's chart in the workspace of the surface entries
LETTERBOX_U8, LETTERBOX_F16, LETTERBOX_F32 = 0, 1, 2             # enum order of include/mcgaze_hip.h


class ConvDesc(C.Structure):
    _fields_ = [('x', C.c_void_p), ('w', C.c_void_p), ('bias', C.c_void_p), ('residual', C.c_void_p), ('y', C.c_void_p),
                ('N', C.c_int), ('H', C.c_int), ('W', C.c_int), ('Cin', C.c_int), ('Cout', C.c_int), ('KH', C.c_int),
                ('KW', C.c_int), ('stride', C.c_int), ('pad', C.c_int), ('relu', C.c_int), ('residual_mode', C.c_int),
                ('Hr', C.c_int), ('Wr', C.c_int), ('x2', C.c_void_p), ('Cin2', C.c_int), ('stride2', C.c_int), ('H2', C.c_int),
                ('W2', C.c_int), ('tile', C.c_int), ('flags', C.c_int), ('wscale', C.c_float)]


class ConvWeights(C.Structure):
    _fields_ = [('w', C.c_void_p), ('bias', C.c_void_p), ('cin', C.c_int), ('cout', C.c_int), ('k', C.c_int),
                ('stride', C.c_int), ('pad', C.c_int), ('wf', C.c_void_p), ('wscale', C.c_float), ('wf4', C.c_void_p)]


class FusedBlock(C.Structure):
    _fields_ = [('wstream', C.c_void_p), ('bias', C.c_void_p), ('conv2_index', C.c_int), ('cm', C.c_int), ('c', C.c_int), ('cn', C.c_int),
                ('nsrc', C.c_int)]


class ModelWeights(C.Structure):
    _fields_ = [('blocks', C.c_int * 4), ('stem', ConvWeights), ('convs', C.POINTER(ConvWeights)), ('num_convs', C.c_int),
                ('lateral', ConvWeights * 4), ('fpn_out', ConvWeights * 4), ('c3_ds', ConvWeights * 4), ('init_boxes', C.c_void_p),
                ('init_feats', C.c_void_p), ('num_stages', C.c_int), ('stage_weights', C.POINTER(C.c_void_p)),
                ('gaze_weights', C.POINTER(C.c_void_p)), ('bbox_stds', C.c_float * 4), ('fused', C.POINTER(FusedBlock)), ('num_fused', C.c_int)]


class FrameDesc(C.Structure):
    _fields_ = [('src', C.c_void_p), ('src_h', C.c_int), ('src_w', C.c_int), ('src_pitch', C.c_int), ('crop_y', C.c_int),
                ('crop_x', C.c_int), ('crop_h', C.c_int), ('crop_w', C.c_int), ('out_h', C.c_int), ('out_w', C.c_int)]


class ImageDesc(C.Structure):
    _fields_ = [('src', C.c_void_p), ('h', C.c_int), ('w', C.c_int), ('pitch', C.c_int)]


class YuvCoef(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('y_off', 'cy', 'cub', 'cug', 'cvg', 'cvr')]


class Nv12ImageDesc(C.Structure):
    _fields_ = [('y', C.c_void_p), ('uv', C.c_void_p), ('h', C.c_int), ('w', C.c_int), ('pitch_y', C.c_int), ('pitch_uv', C.c_int)]


class Nv12FrameDesc(C.Structure):
    _fields_ = FrameDesc._fields_ + [('uv', C.c_void_p), ('uv_pitch', C.c_int)]


class LetterboxDesc(C.Structure):
    _fields_ = [('frame', FrameDesc), ('top', C.c_int), ('left', C.c_int)]


class Nv12LetterboxDesc(C.Structure):
    _fields_ = [('frame', Nv12FrameDesc), ('top', C.c_int), ('left', C.c_int)]


class ArrowDesc(C.Structure):
    _fields_ = [('seg', C.c_int * 2 * 2 * 3), ('thickness', C.c_int), ('x0', C.c_int), ('y0', C.c_int), ('x1', C.c_int), ('y1', C.c_int),
                ('image', C.c_int), ('flag', C.c_int), ('reserved', C.c_int)]


class StrokeDesc(C.Structure):
    _fields_ = [('seg', C.c_int * 2 * 2 * 3), ('thickness', C.c_int), ('x0', C.c_int), ('y0', C.c_int), ('x1', C.c_int), ('y1', C.c_int),
                ('image', C.c_int), ('flag', C.c_int), ('layer', C.c_int), ('count', C.c_int), ('color', C.c_uint), ('color_active', C.c_uint),
                ('reserved', C.c_int)]


class LabelDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('x', 'y', 'x0', 'y0', 'x1', 'y1', 'image', 'flag', 'len')] + [('color', C.c_uint), ('text', C.c_ubyte * LABEL_CHARS)]


class AnonDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('image', 'flag', 'x0', 'y0', 'x1', 'y1', 'cx2', 'cy2', 'W', 'H', 'shift', 'shape')]


class McgError(RuntimeError):
    pass


_lib = None


def load():
    """Load the shared library (once).  Raises if it is absent: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise McgError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                       f'(or `make -C mcgaze_amd/csrc`); mcgaze_amd has no CPU fallback')
    lib = C.CDLL(LIB_PATH)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.mcg_abi_version.restype = i
    lib.mcg_last_error.restype = C.c_char_p
    lib.mcg_build_id.restype = C.c_char_p
    lib.mcg_device_info.argtypes = [C.POINTER(i), C.POINTER(sz), C.c_char_p, i]
    lib.mcg_nchw_to_nhwc.argtypes = [vp, i, vp, vp, i, i, i, i]
    lib.mcg_nhwc_to_nchw.argtypes = [vp, i, vp, vp, i, i, i, i]
    lib.mcg_conv2d.argtypes = [vp, i, C.POINTER(ConvDesc)]
    lib.mcg_stem_workspace_bytes.restype = sz
    lib.mcg_stem_workspace_bytes.argtypes = [i, i, i, i]
    lib.mcg_stem_forward.argtypes = [vp, i, vp, vp, vp, vp, i, i, i, vp, sz, i]
    lib.mcg_roi_align.argtypes = [vp, i, C.POINTER(vp), C.POINTER(i), C.POINTER(i), C.POINTER(i), i, vp, i, i, vp, vp]
    lib.mcg_roi_align_indexed.argtypes = [vp, i, C.POINTER(vp), C.POINTER(i), C.POINTER(i), C.POINTER(i), i, vp, i, i, vp, i, vp, vp]
    lib.mcg_stage_workspace_bytes.restype = sz
    lib.mcg_stage_workspace_bytes.argtypes = [i, i]
    lib.mcg_stage_forward.argtypes = [vp, i, C.POINTER(vp), vp, vp, vp, i, i, vp, vp, vp, C.POINTER(C.c_float), vp, sz, i]
    lib.mcg_gaze_head_workspace_bytes.restype = sz
    lib.mcg_gaze_head_workspace_bytes.argtypes = [i, i]
    lib.mcg_gaze_head.argtypes = [vp, i, C.POINTER(vp), vp, i, vp, vp, sz]
    lib.mcg_engine_create.argtypes = [C.POINTER(vp), C.POINTER(ModelWeights), i]
    lib.mcg_engine_destroy.argtypes = [vp]
    lib.mcg_engine_destroy.restype = None
    lib.mcg_engine_workspace_bytes.restype = sz
    lib.mcg_engine_workspace_bytes.argtypes = [vp, i, i, i, i]
    lib.mcg_trunk_workspace_bytes.restype = sz
    lib.mcg_trunk_workspace_bytes.argtypes = [vp, i, i, i, i]
    lib.mcg_decoder_workspace_bytes.restype = sz
    lib.mcg_decoder_workspace_bytes.argtypes = [vp, i]
    lib.mcg_decoder_forward.argtypes = [vp, vp, C.POINTER(vp), i, i, i, i, vp, vp, vp, vp, vp, sz]
    lib.mcg_decoder_forward_indexed.argtypes = [vp, vp, C.POINTER(vp), i, vp, i, i, i, i, vp, vp, vp, vp, vp, sz]
    lib.mcg_backbone_fpn_forward.argtypes = [vp, vp, vp, i, i, i, i, C.POINTER(vp), vp, sz]
    lib.mcg_deferred_pyramid_bytes.restype = sz
    lib.mcg_deferred_pyramid_bytes.argtypes = [vp, i, i, i]
    lib.mcg_deferred_pyramid_levels.argtypes = [vp, vp, i, i, i, C.POINTER(vp), C.POINTER(i)]
    lib.mcg_deferred_pyramid_state.argtypes = [vp, vp, i, i, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i), C.POINTER(i)]
    lib.mcg_inner_block_neighbours.argtypes = [i, i, i, C.POINTER(i)]
    lib.mcg_backbone_fpn_forward_deferred.argtypes = [vp, vp, vp, i, i, i, i, vp, sz, vp, sz]
    lib.mcg_decoder_forward_deferred.argtypes = [vp, vp, vp, sz, i, i, i, i, vp, vp, vp, vp, vp, sz]
    lib.mcg_clip_forward.argtypes = [vp, vp, vp, i, i, i, i, vp, i, vp, vp, vp, vp, sz]
    # ragged forms: (clip_start (device), num_clips, max_clip_length) in place of clip_length
    lib.mcg_stage_forward_ragged.argtypes = [vp, i, C.POINTER(vp), vp, vp, vp, i, vp, i, i, vp, vp, vp, C.POINTER(C.c_float), vp, sz, i]
    lib.mcg_decoder_forward_ragged.argtypes = [vp, vp, C.POINTER(vp), i, vp, i, vp, i, i, i, i, vp, vp, vp, vp, vp, sz]
    lib.mcg_decoder_forward_deferred_ragged.argtypes = [vp, vp, vp, sz, i, vp, i, i, i, i, vp, vp, vp, vp, vp, sz]
    lib.mcg_clip_forward_ragged.argtypes = [vp, vp, vp, i, vp, i, i, i, i, vp, i, vp, vp, vp, vp, sz]
    lib.mcg_pyramid_scatter_rows.argtypes = [vp, i, C.POINTER(vp), C.POINTER(vp), i, i, i, i, vp]
    lib.mcg_merge_windows.argtypes = [vp, vp, vp, vp, i, vp, i, vp, i, i, vp, i, C.c_float]
    lib.mcg_smooth_gaze.argtypes = [vp, vp, i, vp, i, C.c_double, vp]
    lib.mcg_preprocess_frames.argtypes =[vp, vp, i, vp, i, i, C.POINTER(C.c_float), C.POINTER(C.c_float), i]
    lib.mcg_preprocess_head_crops.argtypes = [vp, vp, i, vp, vp, i, C.c_double, i, i, vp, vp, vp, vp, vp, i, i, C.POINTER(C.c_float), C.POINTER(C.c_float), i]
    lib.mcg_preprocess_frames_nv12.argtypes = lib.mcg_preprocess_frames.argtypes + [C.POINTER(YuvCoef)]
    lib.mcg_preprocess_head_crops_nv12.argtypes = lib.mcg_preprocess_head_crops.argtypes + [C.POINTER(YuvCoef)]
    u8p = C.POINTER(C.c_ubyte)
    lib.mcg_draw_gaze_arrows.argtypes = [vp, vp, i, i, i, vp, vp, i, vp, i, C.c_double, i, C.c_double, C.c_double, u8p, vp, vp, vp]
    lib.mcg_draw_gaze_arrows_nv12.argtypes = lib.mcg_draw_gaze_arrows.argtypes
    lib.mcg_detect_heads_workspace_bytes.restype = sz
    lib.mcg_detect_heads_workspace_bytes.argtypes = [i, i]
    lib.mcg_detect_heads.argtypes = [vp, vp, i, i, i, C.c_longlong, i, i, i, vp, C.c_double, C.c_double, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, sz]
    lib.mcg_letterbox_frames.argtypes = [vp, vp, i, vp, i, i, i, i]
    lib.mcg_letterbox_frames_nv12.argtypes = lib.mcg_letterbox_frames.argtypes + [C.POINTER(YuvCoef)]
    lib.mcg_track_state_bytes.restype = sz
    lib.mcg_track_state_bytes.argtypes = [i, i]
    lib.mcg_track_heads.argtypes = [vp, vp, C.c_longlong, vp, i, i, i, i, C.c_double, i, vp, vp, vp, vp, vp, vp, vp]
    lib.mcg_track_heads_motion.argtypes = [vp, vp, C.c_longlong, vp, i, i, i, i, C.c_double, i, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mcg_live_slots.argtypes = [vp, vp, i, i, i, i, vp, vp, vp, vp, vp]
    lib.mcg_live_gate.argtypes = [vp, vp, vp, i, i, i, i, vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mcg_live_lanes.argtypes = [vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mcg_live_gate_lanes.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mcg_gaze_targets.argtypes = [vp, vp, vp, i, vp, i, vp, vp, i, i, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]
    lib.mcg_gaze_targets_poly.argtypes = [vp, vp, vp, i, vp, i, vp, i, vp, vp, i, i, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]
    lib.mcg_gaze_targets_3d.argtypes = [vp, vp, vp, i, vp, i, vp, i, i, vp, C.c_double, i, vp, i, vp, vp, i, i, C.c_double, C.c_double, vp, vp, vp, vp,
                                        vp, vp, vp]
    lib.mcg_draw_attention.argtypes = [vp, vp, i, i, i, vp, vp, i, vp, i, vp, vp, vp, vp, vp, i, vp, vp, i, i, u8p, C.c_double, i, C.c_double, C.c_double,
                                       i, i, vp, sz, vp, vp, vp]
    lib.mcg_draw_attention_nv12.argtypes = lib.mcg_draw_attention.argtypes
    lib.mcg_format_labels.argtypes = [vp, vp, vp, i, i, i, vp]
    lib.mcg_draw_labels.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp, i, vp, i, i, i, u8p, vp, u8p, vp, vp]
    lib.mcg_draw_labels_nv12.argtypes = lib.mcg_draw_labels.argtypes
    lib.mcg_gaze_heat_add.argtypes = [vp, vp, vp, vp, vp, vp, i, vp, vp, i, i, i, i, i, i, i, i, vp, sz]
    lib.mcg_draw_heat.argtypes = [vp, vp, i, i, i, vp, vp, i, i, i, i, i, vp, i]
    lib.mcg_draw_heat_nv12.argtypes = lib.mcg_draw_heat.argtypes
    lib.mcg_surface_heat_add.argtypes = [vp, vp, vp, vp, vp, vp, i, vp, i, vp, i, vp, vp, i, i, i, i, vp, sz]
    lib.mcg_draw_surface_heat.argtypes = [vp, vp, i, i, i, vp, i, i, vp, i, vp, vp, i, i, vp, vp, i, i, vp, i, vp, sz]
    lib.mcg_draw_surface_heat_nv12.argtypes = lib.mcg_draw_surface_heat.argtypes
    lib.mcg_anonymize_heads.argtypes = [vp, vp, i, i, i, vp, vp, i, C.c_double, i, i, i, i, u8p, vp, vp]
    lib.mcg_anonymize_heads_nv12.argtypes = lib.mcg_anonymize_heads.argtypes
    lib.mcg_gaze_dwell.argtypes =[vp, vp, vp, vp, vp, vp, i, i, i, i, i, vp, vp, i, vp, vp, vp, i, vp]
    lib.mcg_engine_set_option.argtypes = [vp, C.c_char_p, i]
    lib.mcg_engine_profile_start.argtypes = [vp, i]
    lib.mcg_engine_profile_stop.argtypes = [vp, C.POINTER(i), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i), C.POINTER(i), i]
    lib.mcg_bench_backbone_forward.argtypes = [vp, vp, vp, i, i, i, vp, sz]
    lib.mcg_bench_backbone_levels.argtypes = [vp, vp, i, i, i, C.POINTER(vp)]
    lib.mcg_bottleneck_x3.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, i, i, vp]
    lib.mcg_conv3x3_wino_x3.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, i, C.c_float, i]
    lib.mcg_conv3x3_wino_x3_blocks.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, i, C.c_float, vp, vp, i, i]
    lib.mcg_roi_mark_blocks.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp, vp]
    lib.mcg_roi_mark_frames.argtypes = [vp, vp, i, i, i, vp, vp, vp]
    lib.mcg_conv3x3_wino_x3_frames.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, vp, vp, i]
    lib.mcg_deferred_pyramid_frame_state.argtypes = [vp, vp, i, i, i, i, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i)]
    lib.mcg_inner_mark_blocks.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp]
    lib.mcg_conv3x3_wino_x3_weight_bytes.restype = sz
    lib.mcg_pointwise_stream.argtypes = [vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, C.c_float, vp, vp, i]
    lib.mcg_pointwise_dyn.argtypes = [vp, i, vp, vp, vp, vp, i, C.c_float, i]
    lib.mcg_pointwise_pair.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i]
    lib.mcg_engine_range_audit.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_char_p), i, C.POINTER(i)]
    lib.mcg_conv3x3_wino_x3_weight_bytes.argtypes = [i, i, i]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int and name not in ('mcg_abi_version',):
            fn.restype = i
    if lib.mcg_abi_version() != ABI_VERSION:
        raise McgError(f'ABI mismatch: library reports {lib.mcg_abi_version()}, binding expects {ABI_VERSION}')
    _lib = lib
    return lib


def build_id():
    """The build id compiled into the loaded library (csrc/Makefile: sha256 over the kernel sources + the public header, 16 hex digits)."""
    return load().mcg_build_id().decode()


def source_id():
    """The same hash over the sources in THIS tree: differs from build_id() when the shared library is stale."""
    import hashlib
    src = os.path.join(_HERE, 'csrc')
    names = sorted(n for n in os.listdir(src) if n.endswith('.hip') or n.endswith('.hpp'))
    h = hashlib.sha256()
    for n in names:
        h.update(open(os.path.join(src, n), 'rb').read())
    h.update(open(os.path.join(_HERE, '..', 'include', 'mcgaze_hip.h'), 'rb').read())
    return h.hexdigest()[:16]


def check(rc, what):
    if rc != MCG_OK:
        msg = load().mcg_last_error().decode(errors='replace')
        raise McgError(f'{what} failed (code {rc}): {msg}')
