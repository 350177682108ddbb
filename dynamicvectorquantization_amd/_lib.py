"""ctypes binding of libdvq_hip.so (include/dvq_hip.h).  There is no CPU fallback: if the library
is missing the product path fails loudly here."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdvq_hip.so")

F32, BF16 = 0, 1
# DVQ_IMPL_* of include/dvq_hip.h: kernel choice of ConvDesc.impl, dvq_gemm_nt and dvq_gemm_tn
(IMPL_AUTO, IMPL_NAIVE, IMPL_MFMA, IMPL_REGSTAGE, IMPL_HALO, IMPL_WIDE, IMPL_WIDE_PIPE, IMPL_WIDE_PIPE_4WAVE, IMPL_WIDE_PIPE_192,
 IMPL_CONV_PIPE, IMPL_8PHASE) = range(11)

vp, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t


class ConvDesc(C.Structure):
    _fields_ = [("N", i64), ("H", i64), ("W", i64), ("Cin", i64), ("OH", i64), ("OW", i64), ("Cout", i64),
                ("KH", i32), ("KW", i32), ("stride", i32), ("pad_t", i32), ("pad_l", i32), ("upsample", i32),
                ("dtype", i32), ("impl", i32)]


class DecodeLayer(C.Structure):
    """dvq_decode_layer of include/dvq_hip.h"""
    _fields_ = [(n, vp) for n in ("wq", "wk", "wv", "wo", "w1", "w2", "bq", "bk", "bv", "bo", "b1", "b2", "ln1_g", "ln1_b", "ln2_g", "ln2_b",
                                  "kcache", "vcache")]


class LinPackEntry(C.Structure):
    """LinPackEntry of csrc/misc.hip (dvq_linear_pack_multi)"""
    _fields_ = [("master", vp), ("w", vp), ("wt", vp), ("out", i64), ("in_", i64), ("out_p", i64), ("tile_begin", i64),
                ("wt_ld", i64), ("bias_src", vp), ("bias_dst", vp)]


class PackEntry(C.Structure):
    _fields_ = [("master", vp), ("w", vp), ("wt", vp), ("Cout", i64), ("Cin", i64), ("taps", i64), ("Cin_p", i64),
                ("Cout_p", i64), ("begin", i64), ("dtype", i64)]


class ScalarRecord(C.Structure):
    """dvq_scalar_record of include/dvq_hip.h (dvq_scalar_push): 64 (address | fp64 bits, type code) pairs, passed by value"""
    _fields_ = [("addr", C.c_uint64 * 64), ("code", C.c_uint8 * 64)]


class TokenRule(C.Structure):
    """dvq_token_rule of include/dvq_hip.h (forbid_idx and finished are device pointers); MAXV: its DVQ_TOKEN_RULE_MAXV"""
    _fields_ = [("forbid_idx", vp), ("n_forbid", i64), ("forbid_ld", i64), ("forbid_from", i64), ("forbid_codes4", i64 * 4),
                ("keep_code", i64), ("late_forbid_code", i64), ("pad_code", i64), ("finished", vp)]
    MAXV = 2048


class JpegInfo(C.Structure):
    """dvq_jpeg_info_t of include/dvq_hip.h"""
    _fields_ = [("width", i32), ("height", i32), ("components", i32), ("restart_interval", i32), ("h_samp", i32 * 4), ("v_samp", i32 * 4),
                ("qtab_index", i32 * 4), ("supported", i32), ("reserved", i32), ("coef_count", i64)]


# DVQ_JPEG_* of include/dvq_hip.h: why dvq_jpeg_info leaves a file to another decoder
(JPEG_SUPPORTED, JPEG_NOT_JPEG, JPEG_MALFORMED, JPEG_PROGRESSIVE, JPEG_ARITHMETIC, JPEG_SOF_KIND, JPEG_PRECISION, JPEG_COMPONENTS,
 JPEG_SAMPLING, JPEG_COLORSPACE, JPEG_MULTISCAN) = range(11)

# DVQ_SCALAR_* of include/dvq_hip.h: element types of dvq_scalar_push and dvq_codebook_health
SCALAR_F32, SCALAR_BF16, SCALAR_F64, SCALAR_I32, SCALAR_I64, SCALAR_IMM, SCALAR_SKIP = range(7)
SCALAR_PUSH_MAX, SCALAR_COLUMNS_MAX = 64, 256


# name -> (restype, argtypes); mirrors include/dvq_hip.h one to one
SIGNATURES = {
    "dvq_last_error": (C.c_char_p, []),
    "dvq_last_kernel": (C.c_char_p, []),
    "dvq_version": (i32, []),
    "dvq_check_device": (i32, []),
    "dvq_set_deterministic": (i32, [i32]),
    "dvq_deterministic": (i32, []),
    "dvq_unordered_launches": (C.c_longlong, []),
    "dvq_set_fp32_split": (i32, [i32]),
    "dvq_fp32_split": (i32, []),
    "dvq_probe_mfma_rate": (i32, [i32, vp, vp, vp]),
    "dvq_vq_prep_bytes": (sz, [i64, i64]),
    "dvq_vq_prepare": (i32, [vp, i64, i64, vp, vp]),
    "dvq_vq_argmin_workspace_bytes": (sz, [i64]),
    "dvq_vq_argmin": (i32, [vp, i32, vp, vp, i64, i64, i64, vp, vp, i32, vp]),
    "dvq_vq_distances": (i32, [vp, i32, vp, i64, i64, i64, vp, vp]),
    "dvq_vq_gather_loss": (i32, [vp, i32, vp, vp, vp, i64, i64, vp, vp, vp]),
    "dvq_vq_backward": (i32, [vp, vp, i32, vp, vp, vp, vp, i64, i64, vp, vp]),
    "dvq_vq_embed": (i32, [vp, vp, i64, i64, i32, vp, vp]),
    "dvq_vq_ema_stats": (i32, [vp, i32, vp, i64, i64, i64, vp, vp]),
    "dvq_vq_ema_apply": (i32, [vp, vp, f32, f32, i64, i64, vp, vp, vp, vp, vp]),
    "dvq_patch_entropy_gate": (i32, [vp, i64, i64, i64, i32, f32, vp, vp, vp]),
    "dvq_patch_entropy_gate_range": (i32, [vp, i64, i64, i64, i32, f32, f32, f32, vp, vp, vp]),
    "dvq_gn_stats": (i32, [vp, i32, i64, i64, i64, i32, vp, vp]),
    "dvq_gn_apply": (i32, [vp, i32, i64, i64, i64, i32, f32, vp, vp, vp, i32, vp, vp, vp]),
    "dvq_gn_bwd_partial_bytes": (sz, [i64, i64, i64]),
    "dvq_gn_bwd_reduce": (i32, [vp, vp, i32, i64, i64, i64, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
    "dvq_gn_bwd_dx": (i32, [vp, vp, i32, i64, i64, i64, i32, vp, vp, vp, i32, vp, vp, vp, vp]),
    "dvq_conv2d_fwd": (i32, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, i64, vp]),
    "dvq_conv3x3_fused_ok": (i32, [C.POINTER(ConvDesc)]),
    "dvq_conv3x3_subpixel_ok": (i32, [C.POINTER(ConvDesc)]),
    "dvq_split_bf16_planes": (i32, [vp, vp, vp, i64, i64, i64, vp]),
    "dvq_conv2d_scratch_bytes": (i64, [C.POINTER(ConvDesc), i32]),
    "dvq_gn_scale_shift": (i32, [vp, vp, vp, i64, i64, i64, i32, f32, vp, vp, vp]),
    "dvq_conv2d_dgrad": (i32, [C.POINTER(ConvDesc), vp, vp, vp, vp, vp, i32, vp, i64, vp]),
    "dvq_set_workspace": (i32, [vp, i64]),
    "dvq_workspace_release": (i32, [vp]),
    "dvq_cmdlist_create": (i32, [vp, C.POINTER(vp)]),
    "dvq_cmdlist_replay": (i32, [vp, vp, vp]),
    "dvq_cmdlist_info": (i32, [vp, vp]),
    "dvq_cmdlist_destroy": (i32, [vp]),
    "dvq_permute_dual": (i32, [vp, vp, i64, i32, i32, i32, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp, vp]),
    "dvq_permute_dual_back": (i32, [vp, vp, vp, vp, i64, i64, i64, i32, i32, i64, i64, vp, vp]),
    "dvq_avgpool_slice": (i32, [vp, i32, i64, i64, i64, i64, i32, vp, i64, i64, vp]),
    "dvq_avgpool_slice_bwd": (i32, [vp, i32, i64, i64, i64, i64, i64, i64, i32, vp, vp]),
    "dvq_silu": (i32, [vp, i32, i64, vp, vp]),
    "dvq_silu_bwd": (i32, [vp, vp, i32, i64, vp, vp]),
    "dvq_relu": (i32, [vp, i32, i64, vp, vp]),
    "dvq_relu_bwd": (i32, [vp, vp, i32, i64, vp, vp]),
    "dvq_upsample_nearest2x": (i32, [vp, i32, i64, i64, i64, i64, vp, vp]),
    "dvq_upsample_nearest2x_bwd": (i32, [vp, i32, i64, i64, i64, i64, vp, vp]),
    "dvq_grain_merge": (i32, [vp, i32, vp, vp, i32, i64, i64, i64, i64, vp, vp, vp]),
    "dvq_grain_merge_bwd": (i32, [vp, vp, i32, vp, vp, i32, i64, i64, i64, i64, vp, vp, vp]),
    "dvq_affine_channels": (i32, [vp, i32, i64, i64, vp, vp, vp, vp]),
    "dvq_axpy_dev": (i32, [vp, vp, vp, i32, i64, vp, vp]),
    "dvq_maxpool2x2": (i32, [vp, i32, i64, i64, i64, i64, vp, vp]),
    "dvq_maxpool2x2_relu_bwd": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp]),
    "dvq_lpips_head": (i32, [vp, vp, vp, i32, i64, i64, i64, vp, f32, vp, vp]),
    "dvq_lpips_head_drop": (i32, [vp, vp, vp, i32, i64, i64, i64, vp, f32, vp, f32, C.c_uint64, vp]),
    "dvq_conv2d_wgrad": (i32, [C.POINTER(ConvDesc), vp, vp, i64, i64, vp, vp, i32, vp, vp, i64, vp]),
    "dvq_pack_weights_multi": (i32, [vp, i64, i64, vp]),
    "dvq_linear_pack_multi": (i32, [vp, i64, i64, vp]),
    "dvq_pack_weight": (i32, [vp, i64, i64, i64, i64, i64, i64, i32, vp, vp, vp]),
    "dvq_unpack_wgrad": (i32, [vp, i64, i64, i64, i64, i64, vp, vp]),
    "dvq_nchw_to_nhwc_pad": (i32, [vp, i64, i64, i64, i64, i64, i32, vp, vp]),
    "dvq_nhwc_pad_to_nchw": (i32, [vp, i32, i64, i64, i64, i64, i64, vp, vp]),
    "dvq_gemm_nt": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, f32, vp, i32, i32, vp]),
    "dvq_gemm_tn": (i32, [vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i32, vp]),
    "dvq_softmax_rows": (i32, [vp, i32, i64, i64, f32, vp, vp]),
    "dvq_softmax_rows_bwd": (i32, [vp, vp, i32, i64, i64, f32, vp, vp]),
    "dvq_transpose": (i32, [vp, i32, i64, i64, i64, vp, vp]),
    "dvq_dual_merge": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, vp]),
    "dvq_dual_merge_bwd": (i32, [vp, vp, i32, i64, i64, i64, i64, vp, vp, vp]),
    "dvq_add": (i32, [vp, vp, i32, i64, vp, vp]),
    "dvq_add_bias_bcast": (i32, [vp, vp, i32, i64, i64, vp, vp]),
    "dvq_channel_shift_add8": (i32, [vp, vp, i32, i64, i32, vp, vp]),
    "dvq_sum_batch": (i32, [vp, i32, i64, i64, vp, vp]),
    "dvq_sumpool2x2": (i32, [vp, i32, i64, i64, i64, i64, vp, vp]),
    "dvq_cast": (i32, [vp, i32, vp, i32, i64, vp]),
    "dvq_l1_loss": (i32, [vp, vp, i64, vp, vp, vp, vp]),
    "dvq_adam": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i32, vp]),
    "dvq_adamw": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, vp]),
    "dvq_layernorm_fwd": (i32, [vp, i32, i64, i64, f32, vp, vp, vp, vp, vp]),
    "dvq_layernorm_bwd": (i32, [vp, vp, i32, i64, i64, vp, vp, vp, vp, vp, vp]),
    "dvq_layernorm_bwd_res": (i32, [vp, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp, vp]),
    "dvq_layernorm_bwd_res_drop": (i32, [vp, vp, vp, i32, i64, i64, vp, vp, vp, vp, vp, vp, f32, C.c_uint64, vp]),
    "dvq_gelu": (i32, [vp, i32, i64, vp, vp]),
    "dvq_gelu_bwd": (i32, [vp, vp, i32, i64, vp, vp]),
    "dvq_softmax_causal": (i32, [vp, i32, i64, i64, i64, i64, f32, vp, vp]),
    "dvq_embed_gather": (i32, [vp, i64, vp, i32, i64, i64, i64, i64, i64, i32, vp, vp]),
    "dvq_embed_scatter_add": (i32, [vp, i64, vp, i32, i64, i64, i64, i64, i64, i64, i64, vp, vp]),
    "dvq_cross_entropy": (i32, [vp, i32, i64, i64, i64, vp, i64, vp, vp, vp, vp, vp]),
    "dvq_attn_decode": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, i64, f32, vp, vp]),
    "dvq_attn_causal_ok": (i32, [i32, i64, i64, i32, i32]),
    "dvq_attn_causal_scratch_bytes": (i64, [i64, i64, i32, i32, i32]),
    "dvq_attn_causal_mask_bytes": (i64, [i64, i64, i32]),
    "dvq_attn_causal_fwd": (i32, [vp, vp, vp, i64, i32, i64, i64, i32, i32, f32, f32, C.c_uint64, vp, vp, vp, vp, vp]),
    "dvq_attn_causal_bwd": (i32, [vp, vp, vp, i64, vp, vp, vp, i32, i64, i64, i32, i32, f32, f32, C.c_uint64, vp, vp, vp, vp, vp, vp]),
    "dvq_attn_full_ok": (i32, [i32, i64, i64, i32]),
    "dvq_attn_full_fwd": (i32, [vp, vp, vp, i32, i64, i64, i32, f32, vp, vp, vp, vp]),
    "dvq_attn_full_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i64, i64, i32, f32, vp, vp, vp, vp, vp]),
    "dvq_attn_decode_dev": (i32, [vp, vp, vp, vp, vp, i32, i64, i64, i64, vp, i64, f32, vp, vp]),
    "dvq_rows_dev": (i32, [vp, vp, i32, i64, i64, i64, vp, i32, vp]),
    "dvq_decode_stack_scratch_bytes": (sz, [i64, i64, i64]),
    "dvq_decode_stack_ok": (i32, [i64, i64, i32, i64, i64]),
    "dvq_decode_stack_status": (i32, [vp, i64, i64, i64, i32, vp]),
    "dvq_decode_stack": (i32, [vp, i32, i64, i64, i32, i64, i64, vp, C.c_float, vp, vp, i32, vp, vp]),
    "dvq_dropout": (i32, [vp, i32, i64, f32, C.c_uint64, vp, vp]),
    "dvq_dropout_add": (i32, [vp, vp, i32, i64, f32, C.c_uint64, vp, vp]),
    "dvq_fill_f32": (i32, [vp, f32, i64, vp]),
    "dvq_image_desc_bytes": (sz, []),
    "dvq_image_batch_transform": (i32, [vp, vp, vp, vp, i64, i32, i32, vp, vp]),
    "dvq_jpeg_info": (i32, [vp, sz, C.POINTER(JpegInfo)]),
    "dvq_jpeg_entropy_decode": (i32, [vp, sz, vp, i64, vp]),
    "dvq_jpeg_desc_bytes": (sz, []),
    "dvq_jpeg_batch_decode": (i32, [vp, vp, i64, vp, vp, vp]),
    "dvq_png_desc_bytes": (sz, []),
    "dvq_png_batch_unfilter": (i32, [vp, vp, i64, vp, vp]),
    "dvq_adamw_dev": (i32, [vp, vp, vp, vp, i64, vp, vp]),
    "dvq_grad_sqnorm_workspace_bytes": (sz, [i64]),
    "dvq_grad_sqnorm": (i32, [vp, i64, f32, i32, vp, sz, vp, vp]),
    "dvq_adamw_clip_dev": (i32, [vp, vp, vp, vp, i64, vp, vp, vp]),
    "dvq_ema_update": (i32, [vp, vp, i64, vp, vp, vp]),
    "dvq_swap_f32": (i32, [vp, vp, i64, vp]),
    "dvq_segment_stats_workspace_bytes": (sz, [i64, i64]),
    "dvq_segment_stats_state_bytes": (sz, [i64]),
    "dvq_segment_plan_bytes": (sz, [vp, i64, i64]),
    "dvq_segment_plan_build": (i32, [vp, i64, i64, vp, sz]),
    "dvq_segment_stats": (i32, [vp, vp, i64, vp, i64, vp, sz, vp, sz, vp, i32, vp, vp]),
    "dvq_copy_f32_armed": (i32, [vp, vp, i64, vp, vp]),
    "dvq_set_f32x8": (i32, [vp, f32, f32, f32, f32, f32, f32, f32, f32, vp]),
    "dvq_sample_rows": (i32, [vp, i64, i64, vp, vp]),
    "dvq_add_uniform": (i32, [vp, i64, f32, vp, vp]),
    "dvq_sample_constrained": (i32, [vp, i32, i64, i64, i64, f32, C.POINTER(TokenRule), i32, f32, i32, vp, vp, vp]),
    "dvq_sample_guided": (i32, [vp, i32, i64, i64, i64, f32, f32, C.POINTER(TokenRule), i32, f32, i32, vp, vp, vp]),
    "dvq_label_dropout": (i32, [vp, i64, f32, i64, C.c_uint64, vp, vp]),
    "dvq_recon_metrics_workspace_bytes": (sz, [i64, i64, i64]),
    "dvq_recon_metrics": (i32, [vp, vp, i64, i64, i64, i32, vp, vp, vp, vp, sz, vp]),
    "dvq_code_histogram": (i32, [vp, vp, i64, i64, i64, i64, i64, i64, i32, vp, vp, vp, vp]),
    "dvq_recon_cells_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "dvq_recon_cells": (i32, [vp, vp, i64, i64, i64, i64, i64, i32, vp, vp, sz, vp]),
    "dvq_token_nll": (i32, [vp, i32, i64, i64, i64, vp, i64, vp, vp, vp]),
    "dvq_nll_segment_sums": (i32, [vp, vp, i64, i64, i64, vp, vp]),
    "dvq_nll_cell_sums": (i32, [vp, vp, vp, i64, i64, i64, i32, i32, i32, i32, vp, vp, vp]),
    "dvq_tokens_pack": (i32, [vp, vp, i64, i32, i32, i64, vp, vp, vp, vp, vp]),
    "dvq_tokens_unpack": (i32, [vp, vp, i64, i32, i32, i32, i64, i64, i64, i64, i64, i64, i64, i64, vp, vp, vp, vp, vp]),
    "dvq_vq_trained_prep_bytes": (sz, [i64, i64]),
    "dvq_vq_trained_prepare": (i32, [vp, i64, i64, i32, vp, vp]),
    "dvq_vq_sample_argmax": (i32, [vp, i32, vp, vp, i64, i64, i64, i32, f32, vp, vp, vp]),
    "dvq_vq_gumbel_noise": (i32, [C.c_uint64, C.c_uint64, i64, i64, vp, vp]),
    "dvq_vq_codebook_grad": (i32, [vp, i32, vp, vp, vp, vp, i64, i64, i64, vp, vp]),
    "dvq_vq_mask_ratio": (i32, [vp, i64, vp, vp]),
    "dvq_vq_rownorm": (i32, [vp, i64, i64, vp, vp, vp]),
    "dvq_vq_ortho_scratch_bytes": (sz, []),
    "dvq_vq_ortho_sumsq": (i32, [vp, i64, f32, vp, vp, vp]),
    "dvq_vq_rownorm_bwd": (i32, [vp, vp, vp, vp, f32, i64, i64, vp, vp]),
    "dvq_imagelog_workspace_bytes": (sz, [i64]),
    "dvq_grain_overlay": (i32, [vp, vp, vp, i32, i64, i64, i64, i64, i64, C.c_uint32, C.c_uint32, f32, vp, vp, sz, vp]),
    "dvq_grain_lines": (i32, [vp, vp, i32, i64, i64, i64, i64, i64, vp]),
    "dvq_image_grid_shape": (i32, [i64, i64, i64, i64, i64, C.POINTER(i64), C.POINTER(i64)]),
    "dvq_image_grid_u8": (i32, [vp, i64, i64, i64, i64, i64, i64, i32, vp, sz, vp, sz, vp]),
    "dvq_scalar_push_state_bytes": (sz, [i64]),
    "dvq_scalar_push": (i32, [C.POINTER(ScalarRecord), i32, i32, i32, vp, vp]),
    "dvq_codebook_health": (i32, [vp, i32, i64, i64, vp, vp, vp, vp]),
    "dvq_codec_tables": (i32, [vp, i32, i64, i64, i64, C.POINTER(TokenRule), vp, vp]),
    "dvq_codec_record": (i32, [vp, i32, i64, i64, i64, C.POINTER(TokenRule), vp, vp, i64, i64, vp, vp, vp]),
    "dvq_codec_encode": (i32, [vp, i64, i64, i64, vp, vp, vp, i64, vp, vp, vp]),
    "dvq_codec_decode_step": (i32, [vp, i32, i64, i64, i64, C.POINTER(TokenRule), vp, vp, i64, vp, vp, vp]),
    "dvq_feat_moments": (i32, [vp, i64, i64, i64, vp, vp, vp, vp, vp]),
    "dvq_pair_scan_workspace_bytes": (sz, [i64, i64, i32]),
    "dvq_pair_scan": (i32, [vp, i64, vp, i64, i64, i64, i64, vp, i32, i32, vp, vp, vp, vp, sz, vp]),
}


class DvqError(RuntimeError):
    pass


_lib = None


def load():
    """Load libdvq_hip.so and declare every signature.  Raises DvqError if the library is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64.so.7; it must be the HIP runtime of the process (streams and
    # device pointers come from torch), so load torch BEFORE libdvq_hip.so resolves its dependency
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise DvqError(
            f"{LIB_PATH} not found. Build it with `python -m dynamicvectorquantization_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for the DQ-VAE hot path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the .so is stale w.r.t. the header
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_launch_hook = None          # debugging (runtime.StepGraph, DVQ_GRAPH_DEBUG): called with the entry-point name after every call


def check(rc: int, what: str = ""):
    if _launch_hook is not None:
        _launch_hook(what)
    if rc != 0:
        msg = load().dvq_last_error().decode("utf-8", "replace")
        raise DvqError(f"{what or 'libdvq_hip'} failed (code {rc}): {msg}")
