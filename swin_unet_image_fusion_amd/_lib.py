"""ctypes binding of libswinfuse.so (include/swinfuse.h).

No torch types cross this boundary: tensors are handed over as `data_ptr()` integers and the
current HIP stream as a `void*`.  The library is built in-tree by `__graft_entry__.build()`
(hipcc --offload-arch=gfx950); if it is missing, importing anything that computes fails loudly —
there is no CPU fallback in the product path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWF_LIB_PATH") or os.path.join(_HERE, "libswinfuse.so")   # SWF_LIB_PATH: A/B builds of the library

SWF_MAX_LEVELS = 8
PREC_FP32, PREC_FAST = 0, 1

# status codes (swf_status)
OK, ERR_NULL, ERR_BAD_SHAPE, ERR_PAD, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_HIP = 0, -1, -2, -3, -4, -5, -6

c_float_p = C.c_void_p  # device pointers travel as integers


class Linear(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p)]


class Norm(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p)]


class Activation(C.Structure):   # swf_activation: zero-initialised = ELU(alpha = 1), param ignored
    _fields_ = [("kind", C.c_int32), ("param", C.c_float)]


# swf_act_kind
ACT_ELU1, ACT_ELU, ACT_RELU, ACT_LEAKY_RELU, ACT_GELU, ACT_GELU_TANH, ACT_SILU = range(7)


class AttnDesc(C.Structure):
    _fields_ = [("channels", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
                ("win_h", C.c_int32), ("win_w", C.c_int32), ("shift", C.c_int32)]


class AttnParams(C.Structure):
    _fields_ = [("q", Linear), ("k", Linear), ("v", Linear), ("proj", Linear), ("bias_table", C.c_void_p)]


class BlockDesc(C.Structure):
    _fields_ = [("attn", AttnDesc), ("hidden", C.c_int32), ("cross", C.c_int32), ("precision", C.c_int32), ("schedule", C.c_int32),
                ("act", Activation)]


class BlockStreamParams(C.Structure):
    _fields_ = [("ln1", Norm), ("attn", AttnParams), ("ln2", Norm), ("fc1", Linear), ("fc2", Linear)]


class Dropout(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("attn_p", C.c_float), ("proj_p", C.c_float), ("mlp_p", C.c_float)]


class BwdOptions(C.Structure):   # swf_bwd_options: the kernel families of a backward call
    _fields_ = [("gemm", C.c_int32), ("attention", C.c_int32)]


class BwdRoute(C.Structure):     # swf_bwd_route: what the call launched
    _fields_ = [("dx_fma", C.c_int32), ("dx_mfma", C.c_int32), ("dw_fma", C.c_int32), ("dw_mfma", C.c_int32), ("attention", C.c_int32)]


BWD_GEMM_FMA, BWD_GEMM_MFMA = 0, 1                                   # swf_bwd_gemm
BWD_ATTN_THREAD, BWD_ATTN_PHASED = 0, 3                              # swf_bwd_attn (1 and 2 are refused)
BWD_ATTN_RAN_NONE, BWD_ATTN_RAN_RESIDENT, BWD_ATTN_RAN_RECOMPUTE, BWD_ATTN_RAN_PHASED = 0, 1, 2, 3   # swf_bwd_attn_ran


class PatchParams(C.Structure):
    _fields_ = [("conv", Linear), ("ln", Norm)]


class PatchLn1(C.Structure):    # swf_patch_ln1: the next block's LN1 and caller-owned uint16 planes
    _fields_ = [("ln", Norm), ("hi", C.c_void_p), ("lo", C.c_void_p)]


# swf_patch_route
ROUTE_GENERIC, ROUTE_FUSED, ROUTE_RR, ROUTE_DEEP_ROW, ROUTE_DEEP_SLICED, ROUTE_LN1 = 0, 1, 2, 3, 4, 0x100


# swf_block_route: a family in the low byte, OR-ed with the flags of every choice the block dispatch made
BLOCK_GENERIC, BLOCK_WINDOW, BLOCK_DEEP, BLOCK_FAMILY_MASK = 0, 1, 2, 0xFF
BLOCK_WIN_X8, BLOCK_WIN_W16, BLOCK_VIA_TMP, BLOCK_PREPACKED = 0x100, 0x200, 0x400, 0x800
BLOCK_DEEP_QKVATTN, BLOCK_DEEP_FOLD_PROJ, BLOCK_DEEP_QKV = 0x1000, 0x2000, 0x4000
BLOCK_DEEP_ATTNPROJ, BLOCK_DEEP_PROJ, BLOCK_DEEP_CORE16 = 0x8000, 0x10000, 0x20000
BLOCK_MLP_FUSED, BLOCK_MLP_TOK32, BLOCK_MLP_TOK64, BLOCK_MLP_WIDE8, BLOCK_MLP_SPLIT = 0x40000, 0x80000, 0x100000, 0x200000, 0x400000
BLOCK_LN1_GIVEN, BLOCK_LN1_WRITTEN = 0x800000, 0x1000000
SCHED_LATENCY, SCHED_THROUGHPUT = 0, 1


class HeadParams(C.Structure):
    _fields_ = [("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p), ("bn_gamma", C.c_void_p), ("bn_beta", C.c_void_p),
                ("bn_mean", C.c_void_p), ("bn_var", C.c_void_p), ("conv2_w", C.c_void_p), ("conv2_b", C.c_void_p)]


class HeadGrads(C.Structure):
    _fields_ = [("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p), ("bn_gamma", C.c_void_p), ("bn_beta", C.c_void_p),
                ("conv2_w", C.c_void_p), ("conv2_b", C.c_void_p)]


class ModelDesc(C.Structure):
    _fields_ = [("levels", C.c_int32), ("in_dims", C.c_int32 * SWF_MAX_LEVELS), ("out_dims", C.c_int32 * SWF_MAX_LEVELS),
                ("heads", C.c_int32), ("head_dim", C.c_int32 * SWF_MAX_LEVELS), ("mlp_ratio", C.c_int32),
                ("win_h", C.c_int32), ("win_w", C.c_int32), ("merge_h", C.c_int32), ("merge_w", C.c_int32),
                ("head_ksize", C.c_int32), ("precision", C.c_int32), ("schedule", C.c_int32), ("act", Activation)]


class LossDesc(C.Structure):
    _fields_ = [("ssim_mode", C.c_int32), ("use_psnr", C.c_int32), ("ir_ssim_weight", C.c_float), ("ir_psnr_weight", C.c_float),
                ("ssim_scale", C.c_float), ("texture_scale", C.c_float), ("intensity_scale", C.c_float), ("psnr_scale", C.c_float),
                ("ssim_ratio", C.c_float), ("texture_ratio", C.c_float), ("intensity_ratio", C.c_float), ("psnr_ratio", C.c_float)]


class MetricsDesc(C.Structure):   # swf_metrics_desc: the Qabf constants
    _fields_ = [("Tg", C.c_double), ("kg", C.c_double), ("Dg", C.c_double), ("Ta", C.c_double), ("ka", C.c_double), ("Da", C.c_double)]


METRIC_COUNT = 10   # SWF_METRIC_COUNT


class FidelityDesc(C.Structure):   # swf_fidelity_desc: the constants of VIF (sigma_nsq, eps) and Nabf
    _fields_ = [(n, C.c_double) for n in ("sigma_nsq", "eps", "Td", "wt_min", "Nrg", "kg", "sg", "Nra", "ka", "sa")]


FIDELITY_COUNT = 5   # SWF_FIDELITY_COUNT


class StructureDesc(C.Structure):   # swf_structure_desc: the SSIM constants K1, K2, Piella's edge exponent alpha, Yang's threshold Ty
    _fields_ = [(n, C.c_double) for n in ("K1", "K2", "alpha", "Ty")]


STRUCTURE_COUNT = 9   # SWF_STRUCTURE_COUNT


class PerceptionDesc(C.Structure):   # swf_perception_desc: Q_CB's filter (f0, f1, a) and contrast map (p, q, Z), Q_CV's saliency exponent alpha
    _fields_ = [(n, C.c_double) for n in ("f0", "f1", "a", "p", "q", "Z", "alpha")]


PERCEPTION_COUNT = 5   # SWF_PERCEPTION_COUNT


class ComparativeDesc(C.Structure):   # swf_comparative_desc: Q_TE's order q, Q_M's exponents, Q_P's log-Gabor bank, noise, weighting and exponents
    _fields_ = [(n, C.c_double) for n in ("q", "alpha1", "alpha2", "min_wavelength", "mult", "sigma_onf", "k", "cutoff", "g", "eps", "C",
                                          "ep", "eM", "em")]


COMPARATIVE_COUNT = 6   # SWF_COMPARATIVE_COUNT


class FeatureDesc(C.Structure):   # swf_feature_desc: the window's side (3 or 5) and the snap of the DCT coefficients
    _fields_ = [(n, C.c_double) for n in ("window", "dct_step")]


FEATURE_COUNT = 4   # SWF_FEATURE_COUNT


class JpegDesc(C.Structure):   # swf_jpeg_desc
    _fields_ = [("channels", C.c_int32), ("subsampling", C.c_int32), ("quality", C.c_int32)]


JPEG_444, JPEG_420 = 0, 1   # SWF_JPEG_444, SWF_JPEG_420


class PngDesc(C.Structure):   # swf_png_desc
    _fields_ = [("channels", C.c_int32), ("rows_per_block", C.c_int32), ("reserved", C.c_int32)]


class JpegHuff(C.Structure):   # swf_jpeg_huff
    _fields_ = [("mincode", C.c_int32 * 17), ("maxcode", C.c_int32 * 17), ("valptr", C.c_int32 * 17), ("vals", C.c_uint8 * 256),
                ("look", C.c_uint16 * 256), ("defined", C.c_int32)]


class JpegFile(C.Structure):   # swf_jpeg_file: written by swf_jpeg_parse; data_off and out_off are the caller's
    _fields_ = [("data_off", C.c_uint64), ("out_off", C.c_uint64), ("data_bytes", C.c_uint32), ("scan_off", C.c_uint32),
                ("scan_end", C.c_uint32), ("H", C.c_int32), ("W", C.c_int32), ("components", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("blocks", C.c_int32), ("restart_interval", C.c_int32),
                ("intervals", C.c_int32), ("comp_quant", C.c_int32 * 3), ("comp_dc", C.c_int32 * 3), ("comp_ac", C.c_int32 * 3),
                ("quant", (C.c_uint16 * 64) * 4), ("dc", JpegHuff * 4), ("ac", JpegHuff * 4)]


class PngFile(C.Structure):   # swf_png_file: written by swf_png_parse; data_off and out_off are the caller's
    _fields_ = [("data_off", C.c_uint64), ("out_off", C.c_uint64), ("data_bytes", C.c_uint32), ("H", C.c_int32), ("W", C.c_int32),
                ("color_type", C.c_int32), ("bpp", C.c_int32), ("palette_entries", C.c_int32), ("idat_ranges", C.c_uint32),
                ("idat_bytes", C.c_uint32), ("palette", C.c_uint8 * 768)]


# SWF_PNG_STREAM_*; the layouts are SWF_JPEG_OUT_*'s values
PNG_STREAM_OK, PNG_STREAM_TRUNCATED, PNG_STREAM_CODE, PNG_STREAM_DISTANCE, PNG_STREAM_LONG, PNG_STREAM_ADLER, PNG_STREAM_FILTER = range(7)

JPEG_OUT_BGR, JPEG_OUT_RGB, JPEG_OUT_GRAY = 0, 1, 2                              # SWF_JPEG_OUT_*
JPEG_STREAM_OK, JPEG_STREAM_TRUNCATED, JPEG_STREAM_RUN, JPEG_STREAM_CODE = 0, 1, 2, 3   # SWF_JPEG_STREAM_*


class AdamDesc(C.Structure):
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_grad_norm", C.c_double), ("norm_ready", C.c_int32)]


class AdamTensor(C.Structure):   # one table row (swf_adam_tensor); written by swf_adam_table_fill, declared here for its size
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float), ("first_chunk", C.c_int32), ("reserved", C.c_int32)]


class CropRow(C.Structure):      # one table row (swf_crop_row): one output sample of swf_paired_crop_resize_fwd
    _fields_ = [("ir_off", C.c_uint64), ("vis_off", C.c_uint64), ("H", C.c_int32), ("W", C.c_int32), ("top", C.c_int32),
                ("left", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("flip", C.c_int32), ("pad_", C.c_int32)]


P = C.POINTER
_i32, _i64, _sz, _vp = C.c_int32, C.c_int64, C.c_size_t, C.c_void_p

# name -> (restype, argtypes); this table is also what tests check against include/swinfuse.h
SIGNATURES = {
    "swf_version": (C.c_int, []),
    "swf_last_error_string": (C.c_char_p, []),
    "swf_status_string": (C.c_char_p, [C.c_int]),
    "swf_window_attention_fwd": (C.c_int, [P(AttnDesc), P(AttnParams), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_window_attention_fwd_prec": (C.c_int, [P(AttnDesc), _i32, P(AttnParams), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_window_attention_workspace_bytes": (_sz, [P(AttnDesc), _i32, _i32, _i32]),
    "swf_attn_halfblock_fwd": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_mlp_halfblock_fwd": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_basic_block_fwd": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_basic_block_fwd_route": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                            P(_i32), _vp, _sz, _vp]),
    "swf_basic_block_workspace_bytes": (_sz, [P(BlockDesc), _i32, _i32, _i32]),
    "swf_basic_block_packed_bytes": (_sz, [P(BlockDesc)]),
    "swf_basic_block_pack": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _sz, _vp]),
    "swf_basic_block_fwd_packed": (C.c_int, [P(BlockDesc), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "swf_basic_block_bwd_workspace_bytes": (_sz, [P(BlockDesc), _i32, _i32, _i32]),
    "swf_basic_block_bwd": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _vp, _vp,
                                      P(BlockStreamParams), P(BlockStreamParams), _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_window_attention_bwd_workspace_bytes": (_sz, [P(AttnDesc), _i32, _i32, _i32]),
    "swf_window_attention_bwd": (C.c_int, [P(AttnDesc), P(AttnParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, P(AttnParams), _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_mlp_bwd_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "swf_mlp_bwd": (C.c_int, [P(Linear), P(Linear), _vp, _vp, _vp, P(Linear), P(Linear), _i64, _i32, _i32, _vp, _sz, _vp]),
    "swf_dropout_mask": (C.c_int, [C.c_uint64, _i32, _i32, _i64, C.c_float, _vp, _vp]),
    "swf_basic_block_drop_workspace_bytes": (_sz, [P(BlockDesc), _i32, _i32, _i32]),
    "swf_basic_block_fwd_drop": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                           P(Dropout), _vp, _sz, _vp]),
    "swf_basic_block_bwd_drop": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _vp, _vp,
                                           P(BlockStreamParams), P(BlockStreamParams), _i32, _i32, _i32, P(Dropout), _vp, _sz, _vp]),
    "swf_window_attention_drop_workspace_bytes": (_sz, [P(AttnDesc), _i32, _i32, _i32]),
    "swf_window_attention_fwd_drop": (C.c_int, [P(AttnDesc), P(AttnParams), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, P(Dropout), _i32,
                                                _vp, _sz, _vp]),
    "swf_window_attention_bwd_drop": (C.c_int, [P(AttnDesc), P(AttnParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, P(AttnParams), _i32, _i32,
                                                _i32, P(Dropout), _i32, _vp, _sz, _vp]),
    "swf_mlp_drop_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "swf_mlp_fwd_drop": (C.c_int, [P(Linear), P(Linear), _vp, _vp, _i64, _i32, _i32, P(Dropout), _i32, _vp, _sz, _vp]),
    "swf_mlp_bwd_drop": (C.c_int, [P(Linear), P(Linear), _vp, _vp, _vp, P(Linear), P(Linear), _i64, _i32, _i32, P(Dropout), _i32,
                                   _vp, _sz, _vp]),
    "swf_basic_block_bwd_opt": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _vp, _vp,
                                          P(BlockStreamParams), P(BlockStreamParams), _i32, _i32, _i32, P(Dropout), P(BwdOptions), P(BwdRoute),
                                          _vp, _sz, _vp]),
    "swf_window_attention_bwd_opt": (C.c_int, [P(AttnDesc), P(AttnParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, P(AttnParams), _i32, _i32,
                                               _i32, P(Dropout), _i32, P(BwdOptions), P(BwdRoute), _vp, _sz, _vp]),
    "swf_mlp_bwd_opt": (C.c_int, [P(Linear), P(Linear), _vp, _vp, _vp, P(Linear), P(Linear), _i64, _i32, _i32, P(Dropout), _i32,
                                  P(BwdOptions), P(BwdRoute), _vp, _sz, _vp]),
    "swf_attention_bwd_lds_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "swf_linear_bwd_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "swf_linear_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, P(BwdOptions), P(BwdRoute), _vp, _sz, _vp]),
    "swf_layernorm_bwd_workspace_bytes": (_sz, [_i64, _i32]),
    "swf_layernorm_bwd": (C.c_int, [P(Norm), _vp, _vp, _vp, P(Norm), _i64, _i32, _vp, _sz, _vp]),
    "swf_patch_layer_bwd_workspace_bytes": (_sz, [_i32] * 8),
    "swf_patch_layer_bwd": (C.c_int, [P(PatchParams), _vp, _vp, _vp, P(PatchParams), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_patch_layer_bwd_opt": (C.c_int, [P(PatchParams), _vp, _vp, _vp, P(PatchParams), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                          P(BwdOptions), P(BwdRoute), _vp, _sz, _vp]),
    "swf_reflect_pad_bwd": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "swf_final_head_bwd_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "swf_final_head_bwd": (C.c_int, [P(HeadParams), _vp, _vp, _vp, _vp, _vp, P(HeadGrads), _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_final_head_batch_stats": (C.c_int, [P(HeadParams), _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_add_fwd": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "swf_block_pair4_fwd": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_block_stage_prec_workspace_bytes": (_sz, [P(BlockDesc), _i32, _i32, _i32, _i32]),
    "swf_block_stage_fwd_prec": (C.c_int, [P(BlockDesc), P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                           P(PatchLn1), P(PatchLn1), P(_i32), _vp, _sz, _vp]),
    "swf_patch_merge_fwd": (C.c_int, [P(PatchParams), _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_merge_out_shape": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, P(_i32), P(_i32), P(_i32), P(_i32)]),
    "swf_patch_unmerge_fwd": (C.c_int, [P(PatchParams), _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_patch_workspace_bytes": (_sz, [_i32] * 10),
    "swf_patch_merge_prec_workspace_bytes": (_sz, [_i32] * 11),
    "swf_patch_merge_fwd_prec": (C.c_int, [_i32, P(PatchParams), P(PatchParams), _vp, _vp, _vp, _vp] + [_i32] * 9
                                 + [P(PatchLn1), P(PatchLn1), P(_i32), _vp, _sz, _vp]),
    "swf_patch_unmerge_prec_workspace_bytes": (_sz, [_i32] * 13),
    "swf_patch_unmerge_fwd_prec": (C.c_int, [_i32, P(PatchParams), P(PatchParams), _vp, _vp, _vp, _vp, _vp, _vp] + [_i32] * 11
                                   + [P(PatchLn1), P(PatchLn1), P(_i32), _vp, _sz, _vp]),
    "swf_final_head_fwd": (C.c_int, [P(HeadParams), _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_linear_fwd": (C.c_int, [P(Linear), _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "swf_mlp_workspace_bytes": (_sz, [_i32, _i64, _i32, _i32]),
    "swf_mlp_fwd": (C.c_int, [_i32, P(BlockStreamParams), P(BlockStreamParams), _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _sz, _vp]),
    "swf_linear_workspace_bytes": (_sz, [_i32, _i64, _i32, _i32]),
    "swf_linear_fwd_prec": (C.c_int, [P(Linear), _i32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_layernorm_fwd": (C.c_int, [P(Norm), _vp, _vp, _i64, _i32, _i32, _vp]),
    "swf_reflect_pad_fwd": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "swf_crop_fwd": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "swf_nchw_to_nhwc": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "swf_nhwc_to_nchw": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "swf_bgr8_to_ycrcb_fwd": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "swf_gray8_to_unit_fwd": (C.c_int, [_vp, _vp, _i64, _vp]),
    "swf_ycrcb_to_rgb_fwd": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "swf_jpeg_header_bytes": (_sz, [P(JpegDesc)]),
    "swf_jpeg_header": (C.c_int, [P(JpegDesc), _i32, _i32, _vp, _sz]),
    "swf_jpeg_capacity_bytes": (_sz, [P(JpegDesc), _i32, _i32]),
    "swf_jpeg_workspace_bytes": (_sz, [P(JpegDesc), _i32, _i32, _i32]),
    "swf_jpeg_encode": (C.c_int, [P(JpegDesc), _vp, _vp, _vp, _sz, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_png_capacity_bytes": (_sz, [P(PngDesc), _i32, _i32]),
    "swf_png_workspace_bytes": (_sz, [P(PngDesc), _i32, _i32, _i32]),
    "swf_png_encode": (C.c_int, [P(PngDesc), _vp, _vp, _sz, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_jpeg_parse": (C.c_int, [_vp, _sz, P(JpegFile), _vp, _sz, P(_sz)]),
    "swf_jpeg_decode_workspace_bytes": (_sz, [_vp, _i32]),
    "swf_jpeg_decode": (C.c_int, [_vp, _sz, _vp, _vp, _i32, _vp, _vp, _sz, _vp, _i32, _vp, _sz, _vp]),
    "swf_jpeg_decode_split_workspace_bytes": (_sz, [_vp, _i32, _vp, _i32]),
    "swf_jpeg_decode_split": (C.c_int, [_vp, _sz, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _sz, _vp, _i32, _vp, _sz, _vp]),
    "swf_png_parse": (C.c_int, [_vp, _sz, P(PngFile), _vp, _sz, P(_sz)]),
    "swf_png_decode_workspace_bytes": (_sz, [_vp, _i32]),
    "swf_png_decode": (C.c_int, [_vp, _sz, _vp, _vp, _i32, _vp, _vp, _sz, _vp, _i32, _vp, _sz, _vp]),
    "swf_paired_crop_rows_bytes": (_sz, [_i32]),
    "swf_paired_crop_rows_check": (C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64]),
    "swf_paired_crop_resize_fwd": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "swf_model_param_count": (_i32, [P(ModelDesc)]),
    "swf_model_param_info": (C.c_int, [P(ModelDesc), _i32, C.c_char_p, _sz, P(_i64), P(_i64)]),
    "swf_model_arena_elems": (_i64, [P(ModelDesc)]),
    "swf_model_workspace_bytes": (_sz, [P(ModelDesc), _i32, _i32, _i32]),
    "swf_model_forward": (C.c_int, [P(ModelDesc), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_model_packed_bytes": (_sz, [P(ModelDesc)]),
    "swf_model_pack_weights": (C.c_int, [P(ModelDesc), _vp, _vp, _sz, _vp]),
    "swf_model_forward_packed": (C.c_int, [P(ModelDesc), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_model_forward_checked": (C.c_int, [P(ModelDesc), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp, _vp]),
    "swf_model_forward_profiled": (C.c_int, [P(ModelDesc), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, P(C.c_float), _i32, _vp]),
    "swf_tensors_equal": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "swf_fusion_loss_workspace_bytes": (_sz, [P(LossDesc), _i32, _i32, _i32, _i32]),
    "swf_fusion_loss": (C.c_int, [P(LossDesc), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_fusion_metrics_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "swf_fusion_metrics": (C.c_int, [P(MetricsDesc), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_fusion_fidelity_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "swf_fusion_fidelity": (C.c_int, [P(FidelityDesc), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_fusion_structure_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "swf_fusion_structure": (C.c_int, [P(StructureDesc), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_fusion_perception_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "swf_fusion_perception": (C.c_int, [P(PerceptionDesc), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_fusion_comparative_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "swf_fusion_comparative": (C.c_int, [P(ComparativeDesc), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_fusion_feature_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "swf_fusion_feature": (C.c_int, [P(FeatureDesc), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_adam_table_bytes": (_sz, [_i32, _i64]),
    "swf_adam_table_fill": (C.c_int, [_vp, _sz, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "swf_adam_grad_norm": (C.c_int, [C.c_double, _vp, _vp, _sz, _i32, _vp, _vp]),
    "swf_adam_step": (C.c_int, [P(AdamDesc), _vp, _vp, _sz, _i32, _vp, _vp]),
    "swf_tensors_gather": (C.c_int, [_vp, _vp, _sz, _i32, _vp, _i64, C.c_float, _vp]),
    "swf_tensors_scatter": (C.c_int, [_vp, _vp, _sz, _i32, _vp, _i64, _vp]),
    "swf_final_head_stats_pass": (C.c_int, [P(HeadParams), _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_final_head_stats_finish": (C.c_int, [_vp, _sz, _i64, _i32, _vp, _vp, _vp, _vp, C.c_float, _vp]),
    "swf_final_head_bwd_sums": (C.c_int, [P(HeadParams), _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "swf_final_head_bwd_synced": (C.c_int, [P(HeadParams), _vp, _vp, _vp, _vp, _i64, _vp, _vp, P(HeadGrads), _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
}

# swf_<entry>_act: the activation (NULL = ELU(alpha = 1)) in front of the arguments of swf_<entry>
for _name in ("swf_mlp_fwd", "swf_mlp_fwd_drop", "swf_mlp_bwd_opt", "swf_patch_merge_fwd", "swf_patch_unmerge_fwd", "swf_patch_merge_fwd_prec",
              "swf_patch_unmerge_fwd_prec", "swf_patch_layer_bwd_opt", "swf_final_head_fwd", "swf_final_head_bwd", "swf_final_head_bwd_sums",
              "swf_final_head_bwd_synced", "swf_linear_fwd", "swf_linear_fwd_prec", "swf_layernorm_fwd"):
    SIGNATURES[_name + "_act"] = (SIGNATURES[_name][0], [P(Activation)] + SIGNATURES[_name][1])
del _name

_lib: Optional[C.CDLL] = None


class SwinFuseLibraryMissing(ImportError):
    pass


def lib() -> C.CDLL:
    """Load libswinfuse.so (once).  Raises — never falls back — when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SwinFuseLibraryMissing(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(status: int) -> None:
    """Map swf_status to the exception classes the reference raises:
    bad shapes -> ValueError (einops / mode errors), reflect pad >= dim -> RuntimeError
    (torch, a006:128), everything else -> RuntimeError."""
    if status == OK:
        return
    msg = lib().swf_last_error_string().decode(errors="replace")
    kind = lib().swf_status_string(status).decode()
    text = f"libswinfuse: {kind}: {msg}"
    if status == ERR_BAD_SHAPE:
        raise ValueError(text)
    if status == ERR_UNSUPPORTED:
        raise NotImplementedError(text)
    raise RuntimeError(text)
