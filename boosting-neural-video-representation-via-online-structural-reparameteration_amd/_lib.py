"""ctypes binding of liborn.so (include/orn.h).  Fails loudly when the library is missing."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
ORN_MAX_LAYERS = 8
ORN_MAX_BATCH = 16
# ORN_LOSS_* of include/orn.h: every loss of the reference's loss_fn (utils.py:139-189) but the two FFT ones (Fusion13, Fusion15)
LOSS_TYPES = {'L2': 0, 'L1': 1, 'Fusion6': 2, 'SSIM': 3, 'Fusion1': 4, 'Fusion2': 5, 'Fusion3': 6, 'Fusion4': 7, 'Fusion5': 8,
              'Fusion7': 9, 'Fusion8': 10, 'Fusion9': 11, 'Fusion10': 12, 'Fusion11': 13, 'Fusion12': 14}
LOSS_KIND_NONE, LOSS_KIND_SSIM, LOSS_KIND_MSSSIM = 0, 1, 2


def loss_id(loss_type: str) -> int:
    """ORN_LOSS_* of a loss_fn name; NotImplementedError (with what is built) for Fusion13 / Fusion15 and unknown names."""
    if loss_type not in LOSS_TYPES:
        raise NotImplementedError(f'loss_type {loss_type!r} is not built (utils.py:139-189): the library has '
                                  f'{", ".join(LOSS_TYPES)}; the FFT losses Fusion13 and Fusion15 are out of scope')
    return LOSS_TYPES[loss_type]


def loss_spec(loss_type: str):
    """((w_l1, w_l2, w_struct), kind) of a loss name, from the library's one table (orn_loss_spec)."""
    w = (c_float * 3)()
    kind = c_int(0)
    check(lib().orn_loss_spec(loss_id(loss_type), w, ctypes.byref(kind)), 'orn_loss_spec')
    return tuple(float(x) for x in w), kind.value


class OrnError(RuntimeError):
    pass


def lib_path() -> str:
    # ORN_LIB_PATH: A/B timing of two builds on one GPU box (tools/probes); the default is the in-tree library
    return os.environ.get('ORN_LIB_PATH') or os.path.join(HERE, 'liborn.so')


class LayerDesc(ctypes.Structure):
    _fields_ = [('C', c_int32), ('O', c_int32), ('s', c_int32), ('H', c_int32), ('W', c_int32),
                ('w3x3', c_int64), ('b3x3', c_int64), ('w3x1', c_int64), ('b3x1', c_int64),
                ('w1x3', c_int64), ('b1x3', c_int64), ('w1', c_int64), ('w2', c_int64), ('w3', c_int64)]


# ORN_BRANCH_* of include/orn.h: the blocks trained through the online merge of orn_merge_lin.hip (ERB has its own path, `erb`)
BRANCH_KINDS = {'ACB': 2, 'RepVGG': 3, 'ECB': 4}
ECB_SEQ = ('sbx', 'sby', 'lpl')          # orn_branch_ptrs.sb[t] / orn_branch_desc.sb[t]: rbr_conv1x1_<t>_branch
SEQ_FIELDS = ('k0', 'b0', 'scale', 'bias', 'mask')


class SeqDesc(ctypes.Structure):
    _fields_ = [(f, c_int64) for f in SEQ_FIELDS]


class BranchDesc(ctypes.Structure):
    _fields_ = [('w1x1', c_int64), ('b1x1', c_int64), ('sb', SeqDesc * 3)]


class SeqPtrs(ctypes.Structure):
    _fields_ = [(f, c_void_p) for f in SEQ_FIELDS]


class BranchPtrs(ctypes.Structure):
    """orn_branch_ptrs: device pointers of a block's parameters, or of where their gradients go."""
    _fields_ = [(f, c_void_p) for f in ('w3x3', 'b3x3', 'w3x1', 'b3x1', 'w1x3', 'b1x3', 'w1x1', 'b1x1', 'wA', 'wB')] + [('sb', SeqPtrs * 3)]


class EngineDesc(ctypes.Structure):
    _fields_ = [('n_layers', c_int32), ('erb', c_int32), ('embed_len', c_int32), ('stem_dim', c_int32),
                ('fc_h', c_int32), ('fc_w', c_int32), ('fc_dim', c_int32), ('sigmoid', c_int32),
                ('loss_type', c_int32), ('precision', c_int32),
                ('beta1', c_double), ('beta2', c_double), ('eps', c_double),
                ('stem_w0', c_int64), ('stem_b0', c_int64), ('stem_w1', c_int64), ('stem_b1', c_int64),
                ('head_w', c_int64), ('head_b', c_int64), ('n_params', c_int64),
                ('layer', LayerDesc * ORN_MAX_LAYERS),
                # appended (all zero: the engine `erb` describes)
                ('branch_kind', c_int32), ('reserved_', c_int32), ('branch', BranchDesc * ORN_MAX_LAYERS),
                # appended (multi-resolution heads; all zero: a single-resolution engine)
                ('multi_res', c_int32), ('lw', c_float), ('side_head_w', c_int64 * ORN_MAX_LAYERS), ('side_head_b', c_int64 * ORN_MAX_LAYERS),
                # appended (--act; all zero: swish)
                ('act', c_int32), ('reserved2_', c_int32)]


class StageOut(ctypes.Structure):
    """orn_stage_out (include/orn.h, N9): what one stage of orn_engine_eval_stages leaves behind; all NULL = stage not wanted."""
    _fields_ = [(f, c_void_p) for f in ('targets', 'rgb8', 'img', 'stats', 'msssim')]


class Wgrad16Job(ctypes.Structure):
    """orn_debug_wgrad16_job (include/orn_debug.h): one problem of the batched weight-gradient launch and its reduction."""
    _fields_ = [('xpad', c_void_p), ('dypad', c_void_p)] + [(f, c_int32) for f in ('H', 'W', 'C', 'O', 's', 'smax')] + \
               [('slabs', c_void_p), ('dwf', c_void_p), ('dbf', c_void_p)]


class Wgrad16Head(ctypes.Structure):
    """orn_debug_wgrad16_head: the head's dW / db finish riding on the batched launch."""
    _fields_ = [('partial', c_void_p), ('blocks', c_int32), ('C', c_int32), ('dw', c_void_p), ('db', c_void_p)]


class Wgrad16Stem(ctypes.Structure):
    """orn_debug_wgrad16_stem: the deferred B == 1 stem backward riding on both launches."""
    _fields_ = [(f, c_void_p) for f in ('embed', 'w1', 'pre1', 'h1', 'pre2', 'dh2_slabs')] + \
               [(f, c_int32) for f in ('nslab', 'E', 'Hd', 'Nout')] + \
               [(f, c_void_p) for f in ('dw0', 'db0', 'dw1', 'db1', 'ws')] + [('ws_bytes', c_size_t)]


P = c_void_p
_SIGS = {
    'orn_version': (c_int, []),
    'orn_last_error': (c_int, [c_char_p, c_size_t]),
    'orn_pe_fwd': (c_int, [P, c_int, P, c_int, P, P]),
    'orn_stem_fwd': (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P]),
    'orn_stem_bwd_ws_bytes': (c_size_t, [c_int] * 3),
    'orn_stem_bwd': (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P]),
    'orn_erb_merge_fwd': (c_int, [P] * 9 + [c_int, c_int, P, P, P, P]),
    'orn_erb_merge_bwd_ws_bytes': (c_size_t, [c_int, c_int]),
    'orn_erb_merge_bwd': (c_int, [P] * 6 + [c_int, c_int] + [P] * 9 + [P, c_size_t, P]),
    'orn_branch_merge_fwd': (c_int, [c_int, POINTER(BranchPtrs), c_int, c_int, P, P, P]),
    'orn_branch_merge_bwd_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'orn_branch_merge_bwd': (c_int, [c_int, POINTER(BranchPtrs), P, P, c_int, c_int, POINTER(BranchPtrs), P, c_size_t, P]),
    'orn_conv3x3_ps_silu_fwd': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P]),
    'orn_conv3x3_ps_silu_bwd_ws_bytes': (c_size_t, [c_int] * 5),
    'orn_conv3x3_ps_silu_bwd': (c_int, [P, P, P, P] + [c_int] * 6 + [P, P, P, P, c_size_t, P]),
    'orn_conv3x3_ps_silu_bf16_ws_bytes': (c_size_t, [c_int] * 5),
    'orn_conv3x3_ps_silu_fwd_bf16': (c_int, [P, P, P] + [c_int] * 5 + [P, P, P, c_size_t, P]),
    'orn_conv3x3_ps_silu_bwd_bf16': (c_int, [P, P, P, P] + [c_int] * 5 + [P, P, P, P, c_size_t, P]),
    'orn_conv_nhwc_bf16_fwd': (c_int, [P, P, P] + [c_int] * 5 + [P, P, P]),
    'orn_conv_nhwc_f16_fwd': (c_int, [P, P, P] + [c_int] * 5 + [P, P, P]),
    'orn_dgrad_nhwc_bf16': (c_int, [P, P] + [c_int] * 4 + [P, P, c_int, P]),
    'orn_wgrad_nhwc_bf16_ws_bytes': (c_size_t, [c_int] * 3),
    'orn_wgrad_nhwc_bf16': (c_int, [P, P] + [c_int] * 5 + [P, P, P, P]),
    'orn_dgrad_nhwc_f16': (c_int, [P, P] + [c_int] * 4 + [P, P, c_int, P]),
    'orn_wgrad_nhwc_f16': (c_int, [P, P] + [c_int] * 5 + [P, P, P, P]),
    'orn_conv3x3_ps_silu_fwd_f16': (c_int, [P, P, P] + [c_int] * 5 + [P, P, P, c_size_t, P]),
    'orn_conv3x3_ps_silu_bwd_f16': (c_int, [P, P, P, P] + [c_int] * 5 + [P, P, P, P, c_size_t, P]),
    'orn_head_fwd': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P, P]),
    'orn_head_bwd_ws_bytes': (c_size_t, [c_int] * 4),
    'orn_head_bwd': (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, P, P, c_size_t, P]),
    'orn_loss_spec': (c_int, [c_int, POINTER(c_float), POINTER(c_int)]),
    'orn_loss_ws_bytes': (c_size_t, [c_int] * 4),
    'orn_loss_ws_bytes_for': (c_size_t, [c_int] * 5),
    'orn_loss_fwd_bwd': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_float, P, P, P, c_size_t, P]),
    'orn_loss_target_stats_bytes': (c_size_t, [c_int] * 4),
    'orn_loss_target_stats': (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    'orn_msssim_ws_bytes': (c_size_t, [c_int] * 4),
    'orn_msssim': (c_int, [P, P, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    'orn_msssim_frames_ws_bytes': (c_size_t, [c_int] * 4),
    'orn_msssim_frames': (c_int, [P, P, P, c_int, c_int, c_int, c_int, P, P, c_size_t, P]),
    'orn_frames_ingest_u8': (c_int, [P, c_int, c_int, c_int, P, c_int, c_int, P]),
    'orn_frames_pool_f32': (c_int, [P, c_int, c_int, c_int, P, c_int, c_int, P]),
    'orn_adam_step': (c_int, [P, P, P, P, c_size_t, c_double, c_double, c_double, c_double, c_int, P]),
    'orn_engine_ws_bytes': (c_size_t, [POINTER(EngineDesc)]),
    'orn_engine_create': (c_int, [POINTER(EngineDesc), P, P, P, P, P, c_size_t, POINTER(c_void_p)]),
    'orn_engine_destroy': (None, [P]),
    'orn_engine_decode': (c_int, [P, P, P, P]),
    'orn_engine_decode_frames': (c_int, [P, P, P, c_int32, P, P, P, P, P]),
    'orn_engine_eval_frames_ws_bytes': (c_size_t, [POINTER(EngineDesc), c_int]),
    'orn_engine_eval_frames': (c_int, [P, P, P, c_int32, P, P, P, P, P, P, c_size_t, P]),
    'orn_engine_eval_stages_ws_bytes': (c_size_t, [POINTER(EngineDesc), c_uint32, c_int]),
    'orn_engine_eval_stages': (c_int, [P, P, P, c_int32, POINTER(StageOut), P, c_size_t, P]),
    'orn_engine_train_step': (c_int, [P, P, P, P, P, P, c_int32, P]),
    'orn_engine_train_steps_graph': (c_int, [P, P, P, P, P, P, c_int32, c_int32, P]),
    'orn_engine_train_steps': (c_int, [P, P, P, P, P, P, c_int32, c_int32, P]),
    'orn_engine_batch_ws_bytes': (c_size_t, [POINTER(EngineDesc), c_int]),
    'orn_engine_set_batch_ws': (c_int, [P, P, c_size_t, c_int]),
    'orn_engine_train_steps_batch': (c_int, [P, P, P, P, P, P, c_int32, c_int32, c_int32, P]),
    'orn_engine_step_forward': (c_int, [P, P, P, P, P, c_int32, POINTER(c_void_p), P]),
    'orn_engine_step_backward': (c_int, [P, P, P, P, P, P, c_int32, P]),
    'orn_engine_profile_step': (c_int, [P, P, P, P, P, P, c_int32, P, P]),
    'orn_engine_set_grad_mask': (c_int, [P, P]),
    'orn_engine_set_target_stats': (c_int, [P, P]),
    'orn_engine_set_stage_targets': (c_int, [P, c_int32, P]),
    'orn_engine_set_stage_target_stats': (c_int, [P, c_int32, P]),
    'orn_engine_set_stage_stats': (c_int, [P, P, c_int32]),
    'orn_engine_fused_kernel': (c_int, [P, c_int, POINTER(c_void_p), POINTER(c_void_p)]),
    'orn_engine_scale_state': (c_int, [P, P]),
    'orn_engine_set_grad_scale': (c_int, [P, c_float, c_float]),
    # the entries above that evaluate the block activation, with ORN_ACT_* as one more trailing int
    'orn_stem_fwd_act': (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, c_int]),
    'orn_stem_bwd_act': (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P, c_int]),
    'orn_conv3x3_ps_silu_fwd_act': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int]),
    'orn_conv3x3_ps_silu_bwd_act': (c_int, [P, P, P, P] + [c_int] * 6 + [P, P, P, P, c_size_t, P, c_int]),
    'orn_conv3x3_ps_silu_fwd_bf16_act': (c_int, [P, P, P] + [c_int] * 5 + [P, P, P, c_size_t, P, c_int]),
    'orn_conv3x3_ps_silu_bwd_bf16_act': (c_int, [P, P, P, P] + [c_int] * 5 + [P, P, P, P, c_size_t, P, c_int]),
    'orn_conv3x3_ps_silu_fwd_f16_act': (c_int, [P, P, P] + [c_int] * 5 + [P, P, P, c_size_t, P, c_int]),
    'orn_conv3x3_ps_silu_bwd_f16_act': (c_int, [P, P, P, P] + [c_int] * 5 + [P, P, P, P, c_size_t, P, c_int]),
}
ACT_SWISH, ACT_GELU = 0, 1          # ORN_ACT_* of include/orn.h
EXPORTS = tuple(_SIGS.keys())
# test and probe entry points (include/orn_debug.h): resolved if present, never required
_DEBUG_SIGS = {'orn_debug_set': (None, [c_int]), 'orn_debug_set_stamps': (None, [c_void_p]),
               'orn_debug_conv_fwd_bf16': (c_int, [P, P, P] + [c_int] * 5 + [P, P, c_int, P]),
               'orn_debug_conv_fwd_f16': (c_int, [P, P, P] + [c_int] * 5 + [P, P, c_int, P]),
               'orn_debug_conv_dgrad_bf16': (c_int, [P, P] + [c_int] * 4 + [P, P, c_int, P, c_int, P]),
               'orn_debug_conv_dgrad_f16': (c_int, [P, P] + [c_int] * 4 + [P, P, c_int, P, c_int, P]),
               'orn_debug_merge_h16_bwd': (c_int, [c_int, P, P, P, P, P]),
               'orn_debug_decode_out_ws_bytes': (c_size_t, []),
               'orn_debug_decode_out_f32': (c_int, [P, c_int, c_int, P, P, P, P, P, c_size_t, P]),
               'orn_debug_stage_out_bf16': (c_int, [P, P, P] + [c_int] * 4 + [P, P, P, P, P, c_size_t, P]),
               'orn_debug_stage_out_f16': (c_int, [P, P, P] + [c_int] * 4 + [P, P, P, P, P, c_size_t, P]),
               'orn_debug_stage0_supported': (c_int, [c_int] * 5),
               'orn_debug_stage0_slabs': (c_int, [c_int] * 2),
               'orn_debug_stage0_fwd': (c_int, [P, P, P] + [c_int] * 5 + [P, P, c_int, c_int, P]),
               'orn_debug_stage0_bwd': (c_int, [P, P, P, P, c_int, c_int, c_float] + [c_int] * 5 + [P, P, P, P, P]),
               'orn_debug_stem_bwd_slabs': (c_int, [P] * 6 + [c_int] * 4 + [P] * 5 + [c_size_t, P]),
               'orn_debug_gauss_taps': (None, [P]),
               'orn_debug_msssim_level_fwd_tiles': (c_int, [c_int] * 2),
               'orn_debug_msssim_level_bwd_tiles': (c_int, [c_int] * 2),
               'orn_debug_msssim_level_fwd': (c_int, [P, P, c_int, c_int, c_int, P, P, P, P]),
               'orn_debug_msssim_level_bwd': (c_int, [c_int, P, P, P, P, P, c_size_t, c_int, c_int, c_int, c_float, c_float, P, P, P]),
               'orn_debug_loss_msssim_layout': (c_int, [c_int] * 5 + [POINTER(c_int64)]),
               'orn_debug_loss_launch': (c_int, [P, P, P, c_size_t] + [c_int] * 5 + [c_float, P, P, P, P, c_size_t, P]),
               'orn_debug_loss_layout': (c_int, [c_int] * 4 + [POINTER(c_int64)]),
               'orn_debug_side_head_bwd_ws_bytes': (c_size_t, [c_int] * 3),
               'orn_debug_side_head_fwd_bf16': (c_int, [P, P, P] + [c_int] * 4 + [P, P]),
               'orn_debug_side_head_fwd_f16': (c_int, [P, P, P] + [c_int] * 4 + [P, P]),
               'orn_debug_side_head_fwd_f32': (c_int, [P, P, P] + [c_int] * 4 + [P, P]),
               'orn_debug_side_head_bwd_bf16': (c_int, [P] * 4 + [c_int] * 5 + [c_float, c_float, P, P, P, P, c_size_t, P]),
               'orn_debug_side_head_bwd_f16': (c_int, [P] * 4 + [c_int] * 5 + [c_float, c_float, P, P, P, P, c_size_t, P]),
               'orn_debug_side_head_bwd_f32': (c_int, [P] * 4 + [c_int] * 4 + [c_float, P, P, P, P, c_size_t, P]),
               'orn_debug_head16_bwd_blocks': (c_int, [c_int] * 2),
               'orn_debug_head16_bwd_ws_bytes': (c_size_t, [c_int]),
               'orn_debug_head16_bwd_rider_ws_bytes': (c_size_t, [c_int] * 4),
               'orn_debug_head_fwd_bf16': (c_int, [P, P, P] + [c_int] * 4 + [P, P]),
               'orn_debug_head_fwd_f16': (c_int, [P, P, P] + [c_int] * 4 + [P, P]),
               'orn_debug_head_bwd_bf16': (c_int, [P] * 4 + [c_int] * 5 + [c_float, P, P, P, P, c_size_t, P, P, c_int, P, P]),
               'orn_debug_head_bwd_f16': (c_int, [P] * 4 + [c_int] * 5 + [c_float, P, P, P, P, c_size_t, P, P, c_int, P, P]),
               'orn_debug_conv_f32_plan': (c_int, [c_int] * 5 + [POINTER(c_int32)]),
               'orn_debug_conv_fwd_f32': (c_int, [P, P, P] + [c_int] * 6 + [P, P, P]),
               'orn_debug_head_fwd_z': (c_int, [P, P, P] + [c_int] * 5 + [P, P]),
               'orn_debug_conv_bwd_f32_head_ws_bytes': (c_size_t, [c_int] * 4),
               'orn_debug_conv_bwd_f32_head': (c_int, [P] * 6 + [c_int] * 6 + [P] * 6 + [c_size_t, P]),
               'orn_debug_act_eval': (c_int, [c_int, c_int, P, c_size_t, P, P, P]),
               'orn_debug_wgrad16_split': (c_int, [c_int] * 4),
               'orn_debug_wgrad16_ws_floats': (c_size_t, [c_int] * 3),
               'orn_debug_wgrad16_step_bf16': (c_int, [c_int, POINTER(Wgrad16Job), POINTER(Wgrad16Head), POINTER(Wgrad16Stem), c_float,
                                                       c_int, c_int, c_int, POINTER(c_int), P]),
               'orn_debug_wgrad16_step_f16': (c_int, [c_int, POINTER(Wgrad16Job), POINTER(Wgrad16Head), POINTER(Wgrad16Stem), c_float,
                                                      c_int, c_int, c_int, POINTER(c_int), P])}
# the *_act twins of the debug entries that evaluate the block activation: the same arguments + a trailing int
for _n in ('conv_fwd_bf16', 'conv_fwd_f16', 'conv_dgrad_bf16', 'conv_dgrad_f16', 'head_fwd_bf16', 'head_fwd_f16', 'head_bwd_bf16', 'head_bwd_f16',
           'side_head_fwd_bf16', 'side_head_fwd_f16', 'side_head_bwd_bf16', 'side_head_bwd_f16', 'stage_out_bf16', 'stage_out_f16', 'stage0_fwd', 'stage0_bwd', 'stem_bwd_slabs',
           'conv_fwd_f32', 'head_fwd_z', 'conv_bwd_f32_head'):
    _DEBUG_SIGS[f'orn_debug_{_n}_act'] = (_DEBUG_SIGS[f'orn_debug_{_n}'][0], _DEBUG_SIGS[f'orn_debug_{_n}'][1] + [c_int])
del _n

_lib = None


def lib():
    """The loaded library.  Raises OrnError (never falls back) if liborn.so has not been built."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise OrnError(f'{path} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                           '(hipcc --offload-arch=gfx950).  There is no CPU fallback.')
        L = ctypes.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)          # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in _DEBUG_SIGS.items():
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype = res
                fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    buf = ctypes.create_string_buffer(512)
    lib().orn_last_error(buf, 512)
    return buf.value.decode('utf-8', 'replace')


def check(rc: int, what: str = ''):
    if rc != 0:
        raise OrnError(f'{what or "liborn"} failed (rc={rc}): {last_error()}')


def ptr(t):
    """Raw device pointer of a contiguous CUDA (HIP) fp32 tensor, or NULL for None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise OrnError('liborn ops need tensors on the GPU (there is no CPU path)')
    if not t.is_contiguous():
        raise OrnError('liborn ops need contiguous tensors')
    return c_void_p(t.data_ptr())


def stream():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)
