"""ctypes binding of ``libgg.so`` (C-ABI in ``include/gg.h``).  No torch types cross the boundary: tensors are
passed as raw device pointers + sizes.  There is no fallback path: a missing library or a host tensor raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GG_LIB") or os.path.join(_HERE, "lib", "libgg.so")   # GG_LIB: dev override (A/B builds)
_lib = None


class GgError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("B", C.c_void_p), ("ldb", C.c_int64), ("C", C.c_void_p),
                ("ldc", C.c_int64), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("bias", C.c_void_p),
                ("act", C.c_int), ("preact", C.c_void_p), ("rowscale", C.c_void_p), ("rows_per_scale", C.c_int),
                ("residual", C.c_void_p), ("ldr", C.c_int64), ("dact_preact", C.c_void_p), ("dact", C.c_int),
                ("colstats", C.c_void_p), ("out_f32", C.c_int), ("split_k", C.c_int), ("A2", C.c_void_p), ("k_split", C.c_int),
                ("bn_y", C.c_void_p), ("bn_stat", C.c_void_p), ("bn_gamma", C.c_void_p), ("bn_beta", C.c_void_p),
                ("bn_act", C.c_int), ("a_bn_stat", C.c_void_p), ("a_bn_gamma", C.c_void_p), ("a_bn_beta", C.c_void_p),
                ("a_bn_act", C.c_int)]


class Split3Args(C.Structure):          # GgSplit3Args (the fp32_split mode's GEMM: fp32-accurate from three bf16 planes per operand)
    _fields_ = [("a_planes", C.c_void_p), ("lda", C.c_int64), ("b_planes", C.c_void_p), ("ldb", C.c_int64), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("C", C.c_void_p), ("ldc", C.c_int64), ("c_planes", C.c_void_p), ("ldp", C.c_int64), ("bias", C.c_void_p), ("act", C.c_int),
                ("preact", C.c_void_p), ("rowscale", C.c_void_p), ("rows_per_scale", C.c_int), ("residual", C.c_void_p), ("ldr", C.c_int64),
                ("dact_preact", C.c_void_p), ("dact", C.c_int),
                ("groups_dev", C.c_void_p), ("group_rows", C.c_int), ("a_map", C.c_void_p), ("c_map", C.c_void_p)]      # row compaction (device-side live row count, row maps)


class Split3Route(C.Structure):         # GgSplit3Route (gg_gemm_nt_split3_route: kernel, tile width, epilogue class, mapped form, tile grid, dynamic LDS)
    _fields_ = [("kernel", C.c_int), ("tile_n", C.c_int), ("epilogue", C.c_int), ("mapped", C.c_int), ("tilesM", C.c_int), ("tilesN", C.c_int), ("lds_bytes", C.c_int64)]


class AttnArgs(C.Structure):
    _fields_ = [("qkv", C.c_void_p), ("ld", C.c_int64), ("q_off", C.c_int), ("k_off", C.c_int), ("v_off", C.c_int),
                ("head_stride", C.c_int), ("head_dim", C.c_int), ("num_heads", C.c_int), ("num_windows", C.c_int),
                ("tokens_per_window", C.c_int), ("window_size", C.c_int), ("map_h", C.c_int), ("map_w", C.c_int),
                ("bias", C.c_void_p), ("scale", C.c_float), ("out", C.c_void_p), ("ldo", C.c_int64),
                ("dout", C.c_void_p), ("lddo", C.c_int64), ("dqkv", C.c_void_p), ("dbias", C.c_void_p), ("dbias_scratch", C.c_void_p),
                ("lse", C.c_void_p), ("bias_table", C.c_void_p), ("ds_scratch", C.c_void_p),
                ("window_map", C.c_void_p), ("num_windows_dev", C.c_void_p)]


class GeoHeadArgs(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("ldl", C.c_int64), ("N", C.c_int), ("K", C.c_int), ("labels", C.c_void_p),
                ("centroids", C.c_void_p), ("labels_clf", C.c_void_p), ("mode", C.c_int), ("smoothing_km", C.c_float),
                ("grad_scale", C.c_float), ("loss_rows", C.c_void_p), ("loss", C.c_void_p), ("dlogits", C.c_void_p),
                ("ldd", C.c_int64), ("preds", C.c_void_p), ("llh", C.c_void_p), ("topk_vals", C.c_void_p),
                ("topk_idx", C.c_void_p), ("num_candidates", C.c_int), ("nearest", C.c_void_p), ("dlogits_f32", C.c_int)]


class ProtoRefineArgs(C.Structure):
    _fields_ = [("embedding", C.c_void_p), ("B", C.c_int), ("V", C.c_int), ("D", C.c_int), ("initial_preds", C.c_void_p),
                ("candidate_cells", C.c_void_p), ("candidate_probs", C.c_void_p), ("num_candidates", C.c_int),
                ("topk", C.c_int), ("cell_ptr", C.c_void_p), ("num_cells", C.c_int), ("proto_emb", C.c_void_p),
                ("proto_lnglat", C.c_void_p), ("max_refinement", C.c_float), ("temperature", C.c_float),
                ("out_llh", C.c_void_p), ("out_cell", C.c_void_p), ("out_idx", C.c_void_p),
                ("member_ptr", C.c_void_p), ("member_emb", C.c_void_p), ("member_lnglat", C.c_void_p)]


class TinyVitCfg(C.Structure):
    _fields_ = [("img_size", C.c_int), ("in_chans", C.c_int), ("embed_dims", C.c_int * 4), ("depths", C.c_int * 4),
                ("num_heads", C.c_int * 4), ("window_sizes", C.c_int * 4), ("mlp_ratio", C.c_float),
                ("mbconv_expand_ratio", C.c_float), ("bn_eps", C.c_float), ("ln_eps", C.c_float),
                ("bn_momentum", C.c_float), ("act_dtype", C.c_int), ("features_only", C.c_int),
                ("recompute", C.c_int)]


class ClipCfg(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int),
                ("image_size", C.c_int), ("patch_size", C.c_int), ("ln_eps", C.c_float), ("act_dtype", C.c_int),
                ("recompute", C.c_int), ("input_h", C.c_int), ("input_w", C.c_int)]      # input_h / input_w: the size of the call, 0 = image_size (include/gg_clip_interp.h)


class ClipTextCfg(C.Structure):          # GgClipTextCfg (include/gg_clip_text.h)
    _fields_ = [("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int),
                ("vocab_size", C.c_int), ("max_positions", C.c_int), ("ln_eps", C.c_float), ("act_dtype", C.c_int)]


class ContrastiveArgs(C.Structure):      # GgContrastiveArgs
    _fields_ = [("img", C.c_void_p), ("ldi", C.c_int64), ("txt", C.c_void_p), ("ldt", C.c_int64), ("Bi", C.c_int), ("Bt", C.c_int), ("P", C.c_int),
                ("logit_scale", C.c_void_p), ("img_n", C.c_void_p), ("txt_n", C.c_void_p), ("logits_per_text", C.c_void_p),
                ("logits_per_image", C.c_void_p), ("want_loss", C.c_int), ("d_loss_scale", C.c_float), ("loss", C.c_void_p),
                ("d_logit_scale", C.c_void_p), ("d_img", C.c_void_p), ("d_txt", C.c_void_p), ("scratch", C.c_void_p)]


class ClsHeadArgs(C.Structure):          # GgClsHeadArgs (include/gg_cls.h)
    _fields_ = [("logits", C.c_void_p), ("ldl", C.c_int64), ("N", C.c_int), ("C", C.c_int), ("labels", C.c_void_p), ("grad_scale", C.c_float),
                ("upstream", C.c_void_p), ("loss_rows", C.c_void_p), ("loss", C.c_void_p), ("dlogits", C.c_void_p), ("ldd", C.c_int64),
                ("dlogits_f32", C.c_int), ("rank", C.c_void_p), ("preds", C.c_void_p)]


AUG_MAX_LAYERS = 4                        # GG_AUG_MAX_LAYERS (include/gg_aug.h)


class AugOp(C.Structure):                # GgAugOp: one RandAugment op slot with its resolved arguments
    _fields_ = [("op", C.c_int32), ("applied", C.c_int32), ("iarg", C.c_int32), ("factor", C.c_float), ("m", C.c_double * 6), ("resample", C.c_int32),
                ("fill", C.c_uint8 * 3), ("reserved", C.c_uint8)]


class AugRecord(C.Structure):            # GgAugRecord: crop box, flip flag and the op slots of one image
    _fields_ = [("top", C.c_int32), ("left", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("flip", C.c_int32), ("num_layers", C.c_int32),
                ("ops", AugOp * AUG_MAX_LAYERS)]


class AugArgs(C.Structure):              # GgAugArgs
    _fields_ = [("src", C.c_void_p), ("src_bytes", C.c_int64), ("offsets", C.c_void_p), ("heights", C.c_void_p), ("widths", C.c_void_p), ("B", C.c_int), ("S", C.c_int),
                ("filter", C.c_int), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("records", C.c_void_p), ("dst", C.c_void_p), ("dst_u8", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class EvalGeom(C.Structure):             # GgEvalGeom (include/gg_eval.h): resized size of the whole image, crop origin inside it
    _fields_ = [("Hr", C.c_int32), ("Wr", C.c_int32), ("top", C.c_int32), ("left", C.c_int32)]


class EvalArgs(C.Structure):             # GgEvalArgs
    _fields_ = [("src", C.c_void_p), ("src_bytes", C.c_int64), ("offsets", C.c_void_p), ("heights", C.c_void_p), ("widths", C.c_void_p), ("geom", C.c_void_p),
                ("B", C.c_int), ("Hc", C.c_int), ("Wc", C.c_int), ("filter", C.c_int), ("mul_rescale", C.c_int), ("normalize", C.c_int), ("mean", C.c_float * 3),
                ("std", C.c_float * 3), ("dst", C.c_void_p), ("dst_u8", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class PanoArgs(C.Structure):             # GgPanoArgs (include/gg_pano.h)
    _fields_ = [("src", C.c_void_p), ("src_bytes", C.c_int64), ("offsets", C.c_void_p), ("heights", C.c_void_p), ("widths", C.c_void_p), ("num_images", C.c_int),
                ("num_slots", C.c_int), ("slot_image", C.c_void_p), ("resize", C.c_int), ("Ht", C.c_int), ("Wt", C.c_int), ("normalize", C.c_int), ("mean", C.c_float * 3),
                ("std", C.c_float * 3), ("dst", C.c_void_p), ("dst_u8", C.c_void_p), ("u8_offsets", C.c_void_p), ("dst_u8_bytes", C.c_int64), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64)]


class JpegInfo(C.Structure):             # GgJpegInfo (include/gg_jpeg.h): what the host-side plan found out about one file
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("components", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32), ("segments", C.c_int32),
                ("refusal", C.c_int32), ("reserved", C.c_int32), ("out_offset", C.c_int64), ("stream_offset", C.c_int64)]


STAGE_DONE_FN = C.CFUNCTYPE(None, C.c_int, C.c_void_p)      # GgStageDoneFn (host callback of gg_tinyvit_backward)

# every exported symbol of include/gg.h: name -> (restype, argtypes)
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "gg_version": (_I, []),
    "gg_last_error": (C.c_char_p, []),
    "gg_gemm_nt": (_I, [C.POINTER(GemmArgs), _P]),
    "gg_gemm_colstats_rows": (_I, [_I]),
    "gg_gemm_nt_route": (_I, [C.POINTER(GemmArgs), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "gg_stat_rows_capacity": (_I, [_I]),
    "gg_gemm_tn_splits": (_I, [_I, _I, _I]),
    "gg_gemm_tn": (_I, [_P, _L, _P, _L, _I, _I, _I, _P, _I, _P, _I, _P]),
    "gg_gemm_tn_bn": (_I, [_P, _P, _L, _P, _P, _L, _I, _I, _I, _P, _I, _P]),
    "gg_gemm_tn_bn_f32": (_I, [_P, _P, _L, _P, _P, _L, _I, _I, _I, _P, _I, _P]),
    "gg_splitk_reduce": (_I, [_P, _P, _L, _I, _I, _F, _P]),
    "gg_transpose_bf16": (_I, [_P, _L, _P, _L, _I, _I, _P, _I, _P]),
    "gg_cast_transpose_f32": (_I, [_P, _I, _I, _P, _L, _P, _L, _P]),
    "gg_cast_f32_to_bf16": (_I, [_P, _P, _L, _P]),
    "gg_cast_bf16_to_f32": (_I, [_P, _P, _L, _P]),
    "gg_colsum_scratch_floats": (_L, [_I, _I]),
    "gg_colsum_bf16": (_I, [_P, _L, _I, _I, _P, _I, _P, _P, _I, _P]),
    "gg_im2col_nchw3_f32": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "gg_im2col_nhwc_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "gg_im2col_nhwc_bn_bf16": (_I, [_P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "gg_col2im_nhwc_bf16": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "gg_col2im_nhwc_bnbwd_bf16": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "gg_col2im_nhwc_bnbwd_f32": (_I, [_P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "gg_dwconv_stat_rows": (_I, [_I, _I, _I, _I, _I]),
    "gg_dwconv_fused_stat_rows": (_I, [_I, _I, _I, _I, _I]),
    "gg_dwconv_fwd_fused_stat_rows": (_I, [_I, _I, _I, _I, _I]),
    "gg_dwconv3x3_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "gg_dwconv3x3_fwd_fused": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "gg_dwconv3x3_bwd_data_fused": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P]),
    "gg_dwconv_s2_fused_stat_rows": (_I, [_I, _I, _I, _I]),
    "gg_dwconv3x3_s2_bwd_data_fused": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P]),
    "gg_dwconv3x3_bwd_data": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "gg_dwconv_wgrad_scratch_floats": (_L, [_I, _I, _I, _I, _I]),
    "gg_dwconv3x3_bwd_weight": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "gg_bn_finalize": (_I, [_P, _I, _I, _L, _F, _F, _P, _P, _P, _P]),
    "gg_bn_eval_stat": (_I, [_P, _P, _I, _F, _P, _P]),
    "gg_bn_apply": (_I, [_P, _P, _P, _P, _L, _I, _I, _P, _P, _I, _P, _P]),
    "gg_bn_bwd_scratch_floats": (_L, [_L, _I]),
    "gg_bn_bwd_rows": (_I, [_L, _I]),
    "gg_bn_bwd_reduce": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _I, _P, _P, _P]),
    "gg_bn_bwd_finalize": (_I, [_P, _I, _I, _L, _P, _P, _P, _P, _P, _I, _P]),
    "gg_bn_bwd_apply": (_I, [_P, _P, _P, _L, _I, _P, _I, _P, _P]),
    "gg_bn_bwd_fold_weights": (_I, [_P, _P, _P, _I, _I, _P, _P, _P]),
    "gg_bn_bwd": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _I, _P]),
    "gg_layernorm_fwd": (_I, [_P, _I, _P, _P, _L, _I, _F, _P, _I, _P, _P, _P]),
    "gg_layernorm_fwd_bn": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P]),
    "gg_gemm_f32_set_trace": (_I, [_P]),
    "gg_layernorm_fwd_bn_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P]),
    "gg_layernorm_bwd_scratch_floats": (_L, [_L, _I]),
    "gg_layernorm_bwd": (_I, [_P, _P, _I, _P, _P, _P, _L, _I, _P, _P, _P, _P, _P, _I, _P]),
    "gg_layernorm_bwd_colsum_rows": (_I, [_L]),
    "gg_layernorm_bwd_colsum": (_I, [_P, _P, _I, _P, _P, _P, _L, _I, _P, _P, _P, _P]),
    "gg_bn_bwd_coef_from_x": (_I, [_P, _I, _I, _L, _P, _P, _P, _P, _P]),
    "gg_token_mean_fwd": (_I, [_P, _P, _I, _I, _I, _P]),
    "gg_token_mean_bwd": (_I, [_P, _P, _I, _I, _I, _P]),
    "gg_view_mean_fwd": (_I, [_P, _P, _L, _I, _I, _I, _P]),
    "gg_view_mean_bwd": (_I, [_P, _L, _P, _I, _I, _I, _P]),
    "gg_attention_padded_tokens": (_I, [_I]),
    "gg_attention_expand_bias": (_I, [_P, _I, _I, _F, _P, _P]),
    "gg_attention_fwd": (_I, [C.POINTER(AttnArgs), _P]),
    "gg_attention_fwd_f16": (_I, [C.POINTER(AttnArgs), _P]),
    "gg_attention_bwd": (_I, [C.POINTER(AttnArgs), _P]),
    "gg_attention_flash_fwd": (_I, [C.POINTER(AttnArgs), _I, _P]),
    "gg_attention_flash_bwd": (_I, [C.POINTER(AttnArgs), _I, _P]),
    "gg_attention_flash_dbias_rows": (_L, [_I, _I]),
    "gg_attention_flash_ds_scratch_floats": (_L, [_I, _I, _I]),
    "gg_attention_flash_single_pass": (_I, [_I, _I, _I, _I]),
    "gg_split3_bf16": (_I, [_P, _L, _I, _L, _P, _P]),
    "gg_layernorm_fwd_split3": (_I, [_P, _P, _P, _L, _I, _F, _P, _P, _P, _P]),
    "gg_layernorm_fwd_bn_split3": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P]),
    "gg_gemm_nt_split3": (_I, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _P, _P]),
    "gg_gemm_nt_split3_ex": (_I, [C.POINTER(Split3Args), _P]),
    "gg_gemm_nt_split3_af32": (_I, [C.POINTER(Split3Args), _P, _L, _L, _P]),
    "gg_gemm_nt_split3_af32_stats": (_I, [C.POINTER(Split3Args), _P, _L, _L, _P, _P]),
    "gg_gemm_nt_split3_af32_pro": (_I, [C.POINTER(Split3Args), _P, _L, _L, _P, _P, _P, _I, _P, _P]),
    "gg_gemm_nt_split3_route": (_I, [C.POINTER(Split3Args), _I, _I, _I, C.POINTER(Split3Route)]),
    "gg_gemm_tn_split3_splits": (_I, [_I, _I, _I]),
    "gg_gemm_tn_split3": (_I, [_P, _L, _P, _L, _I, _I, _I, _P, _I, _P, _I, _P]),
    "gg_gemm_nt_f32": (_I, [C.POINTER(GemmArgs), _P]),
    "gg_gemm_tn_f32_splits": (_I, [_I, _I, _I]),
    "gg_gemm_tn_f32": (_I, [_P, _L, _P, _L, _I, _I, _I, _P, _I, _P, _I, _P]),
    "gg_colsum_f32": (_I, [_P, _L, _I, _I, _P, _I, _P, _P, _I, _P]),
    "gg_im2col_nchw3_f32_f32": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "gg_im2col_nhwc_f32": (_I, [_P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
    "gg_col2im_nhwc_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "gg_dwconv_f32_stat_rows": (_I, [_I, _I, _I, _I, _I]),
    "gg_dwconv3x3_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "gg_dwconv3x3_bwd_data_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "gg_dwconv_f32_wgrad_scratch_floats": (_L, [_I, _I, _I, _I, _I]),
    "gg_dwconv3x3_bwd_weight_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "gg_bn_apply_f32": (_I, [_P, _P, _P, _P, _L, _I, _I, _P, _P, _I, _P, _P]),
    "gg_bn_bwd_f32": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _I, _P]),
    "gg_bn_bwd_reduce_f32": (_I, [_P, _P, _P, _P, _P, _L, _I, _I, _P, _P, _I, _P, _P, _P]),
    "gg_bn_bwd_apply_f32": (_I, [_P, _P, _P, _L, _I, _P, _I, _P, _P]),
    "gg_dwconv3x3_fwd_fused_f32": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "gg_dwconv3x3_bwd_data_fused_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P]),
    "gg_dwconv_f32_s2_fused_stat_rows": (_I, [_I, _I, _I, _I]),
    "gg_dwconv3x3_s2_bwd_data_fused_f32": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P, _P]),
    "gg_gemm_nt_f16": (_I, [C.POINTER(GemmArgs), _P]),
    "gg_layernorm_fwd_f16": (_I, [_P, _P, _P, _L, _I, _F, _P, _P]),
    "gg_token_mean_fwd_f16": (_I, [_P, _P, _I, _I, _I, _P]),
    "gg_cast_f32_to_f16": (_I, [_P, _P, _L, _P]),
    "gg_cast_f16_to_f32": (_I, [_P, _P, _L, _P]),
    "gg_token_mean_fwd_f32": (_I, [_P, _P, _I, _I, _I, _P]),
    "gg_token_mean_bwd_f32": (_I, [_P, _P, _I, _I, _I, _P]),
    "gg_view_mean_fwd_f32": (_I, [_P, _P, _L, _I, _I, _I, _P]),
    "gg_view_mean_bwd_f32": (_I, [_P, _L, _P, _I, _I, _I, _P]),
    "gg_geo_head": (_I, [C.POINTER(GeoHeadArgs), _P]),
    "gg_haversine_matrix": (_I, [_P, _P, _P, _I, _I, _P]),
    "gg_pe_add_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "gg_mha_q0_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "gg_mha_q0_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "gg_proto_refine": (_I, [C.POINTER(ProtoRefineArgs), _P]),
    "gg_geoguessr_score": (_I, [_P, _P, _I, _P, _P, _P]),      # (pred, truth, N, double* dist_km, int32* score, stream)
    "gg_geoguessr_score_f64": (_I, [_P, _P, _I, _P, _P, _P]),  # same with double* coordinates
    "gg_adamw_step": (_I, [_P, _P, _P, _P, _L, _I, _F, _F, _F, _F, _F, _F, _P]),
    "gg_fill_f32": (_I, [_P, _L, _F, _P]),
    "gg_comm_unique_id": (_I, [_P]),
    "gg_comm_create": (_I, [C.POINTER(_P), _P, _I, _I, _I]),
    "gg_comm_destroy": (_I, [_P]),
    "gg_comm_rank": (_I, [_P]),
    "gg_comm_world": (_I, [_P]),
    "gg_comm_allreduce_sum_f32": (_I, [_P, _P, _L, _P]),
    "gg_comm_broadcast": (_I, [_P, _P, _L, _I, _P]),
    "gg_comm_barrier": (_I, [_P, _P, _I]),
    "gg_prof_enable": (_I, [_I]),
    "gg_prof_reset": (_I, []),
    "gg_prof_read": (_I, [_I, C.POINTER(C.c_double), C.POINTER(_L), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gg_prof_count": (_I, []),
    "gg_prof_record": (_I, [_I, C.POINTER(_I), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gg_graph_set_mode": (_I, [_I]),
    "gg_graph_stats": (_I, [C.POINTER(_L), C.POINTER(_L), C.POINTER(_L)]),
    "gg_graph_clear": (_I, []),
    "gg_tinyvit_num_tensors": (_I, [C.POINTER(TinyVitCfg)]),
    "gg_tinyvit_tensor_info": (_I, [C.POINTER(TinyVitCfg), _I, C.c_char_p, _I, C.POINTER(_L), C.POINTER(_L), C.POINTER(_I),
                                    C.POINTER(_L), C.POINTER(_I)]),
    "gg_tinyvit_param_floats": (_L, [C.POINTER(TinyVitCfg)]),
    "gg_tinyvit_buffer_floats": (_L, [C.POINTER(TinyVitCfg)]),
    "gg_tinyvit_num_counters": (_I, [C.POINTER(TinyVitCfg)]),
    "gg_tinyvit_num_drop_slots": (_I, [C.POINTER(TinyVitCfg)]),
    "gg_drop_path_scales": (_I, [_P, _I, _I, C.c_uint64, C.c_uint64, _P, _P]),
    "gg_transpose_f32": (_I, [_P, _I, _I, _P, _L, _P]),
    "gg_tinyvit_wcache_bytes": (_L, [C.POINTER(TinyVitCfg)]),
    "gg_tinyvit_workspace_bytes": (_L, [C.POINTER(TinyVitCfg), _I, _I]),
    "gg_tinyvit_workspace_bytes_masked": (_L, [C.POINTER(TinyVitCfg), _I, _I, _P]),
    "gg_tinyvit_refresh_weights": (_I, [C.POINTER(TinyVitCfg), _P, _P, _P]),
    "gg_tinyvit_refresh_weights_masked": (_I, [C.POINTER(TinyVitCfg), _P, _P, C.c_char_p, _P]),
    "gg_preprocess_bilinear": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "gg_preprocess_pil_workspace_bytes": (C.c_int64, [_I, _I, _I, _I, _I, _I]),
    "gg_preprocess_pil": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P, _P, _P]),
    "gg_segment_mean": (_I, [_P, _L, _P, _P, _I, _I, _P, _P]),
    "gg_tinyvit_forward": (_I, [C.POINTER(TinyVitCfg), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, _P]),
    "gg_tinyvit_backward": (_I, [C.POINTER(TinyVitCfg), _I, _P, _P, _P, _P, _P, _P, C.c_char_p, _P, STAGE_DONE_FN, _P]),
    "gg_tinyvit_activation_info": (_I, [C.POINTER(TinyVitCfg), _I, C.c_char_p, C.POINTER(_L), C.POINTER(_L)]),
    "gg_tinyvit_activation_info_masked": (_I, [C.POINTER(TinyVitCfg), _I, C.c_char_p, _P, C.POINTER(_L), C.POINTER(_L)]),
    "gg_clip_num_tensors": (_I, [C.POINTER(ClipCfg)]),
    "gg_clip_tensor_info": (_I, [C.POINTER(ClipCfg), _I, C.c_char_p, _I, C.POINTER(_L), C.POINTER(_L), C.POINTER(_I),
                                 C.POINTER(_L)]),
    "gg_clip_param_floats": (_L, [C.POINTER(ClipCfg)]),
    "gg_clip_wcache_bytes": (_L, [C.POINTER(ClipCfg)]),
    "gg_clip_workspace_bytes": (_L, [C.POINTER(ClipCfg), _I, _I, C.c_char_p]),
    "gg_clip_first_trained_layer": (_I, [C.POINTER(ClipCfg), C.c_char_p]),
    "gg_clip_refresh_weights": (_I, [C.POINTER(ClipCfg), _P, _P, _P]),
    "gg_clip_forward": (_I, [C.POINTER(ClipCfg), _I, _I, _P, _P, _P, _P, _P, _P, C.c_char_p, _P]),
    "gg_clip_backward": (_I, [C.POINTER(ClipCfg), _I, _P, _P, _P, _P, _P, _P, C.c_char_p, _P]),
}
SYMBOLS = list(SIGNATURES)

# every exported symbol of include/gg_clip_text.h (the contrastive pre-training stage), bound from the same libgg.so
TEXT_SIGNATURES = {
    "gg_attention_causal_fwd": (_I, [C.POINTER(AttnArgs), _I, _P]),
    "gg_clip_text_num_tensors": (_I, [C.POINTER(ClipTextCfg)]),
    "gg_clip_text_tensor_info": (_I, [C.POINTER(ClipTextCfg), _I, C.c_char_p, _I, C.POINTER(_L), C.POINTER(_L), C.POINTER(_I), C.POINTER(_L)]),
    "gg_clip_text_param_floats": (_L, [C.POINTER(ClipTextCfg)]),
    "gg_clip_text_wcache_bytes": (_L, [C.POINTER(ClipTextCfg)]),
    "gg_clip_text_workspace_bytes": (_L, [C.POINTER(ClipTextCfg), _I, _I]),
    "gg_clip_text_refresh_weights": (_I, [C.POINTER(ClipTextCfg), _P, _P, _P]),
    "gg_clip_text_forward": (_I, [C.POINTER(ClipTextCfg), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gg_clip_contrastive_scratch_floats": (_L, [_I, _I, _I]),
    "gg_clip_contrastive": (_I, [C.POINTER(ContrastiveArgs), _P]),
    "gg_row_gather_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "gg_row_scatter_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "gg_grad_sq_norm_scratch_doubles": (_L, [_L]),
    "gg_grad_sq_norm": (_I, [_P, _L, _P, _P, _I, _P]),
}
TEXT_SYMBOLS = list(TEXT_SIGNATURES)

# every exported symbol of include/gg_clip_text_train.h (training the text tower), bound from the same libgg.so
TEXT_TRAIN_SIGNATURES = {
    "gg_attention_causal_bwd": (_I, [C.POINTER(AttnArgs), _I, _P]),
    "gg_embedding_scatter_add_scratch_bytes": (_L, [_L]),
    "gg_embedding_scatter_add_f32": (_I, [_P, _P, _P, _L, _I, _I, _P, _P]),
    "gg_clip_text_train_workspace_bytes": (_L, [C.POINTER(ClipTextCfg), _I, _I, C.c_char_p]),
    "gg_clip_text_first_trained_layer": (_I, [C.POINTER(ClipTextCfg), C.c_char_p]),
    "gg_clip_text_forward_train": (_I, [C.POINTER(ClipTextCfg), _I, _I, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, _P]),
    "gg_clip_text_backward": (_I, [C.POINTER(ClipTextCfg), _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, C.c_char_p, _P]),
}
TEXT_TRAIN_SYMBOLS = list(TEXT_TRAIN_SIGNATURES)

# every exported symbol of include/gg_cls.h (the TinyViT classifier fine-tune), bound from the same libgg.so
CLS_SIGNATURES = {
    "gg_cls_head": (_I, [C.POINTER(ClsHeadArgs), _P]),
    "gg_tinyvit_last_map_info": (_I, [C.POINTER(TinyVitCfg), _I, C.POINTER(_L), C.POINTER(_L), C.POINTER(_I), C.POINTER(_I)]),
}
CLS_SYMBOLS = list(CLS_SIGNATURES)

# every exported symbol of include/gg_drop.h (DropPath row compaction of the fp32_split TinyViT step), bound from the same libgg.so
DROP_LIST_HEAD = 4                        # GG_DROP_LIST_HEAD: a kept list is [count, batch, 0, 0][kept: batch][pos: batch] int32
DROP_SIGNATURES = {
    "gg_drop_list_ints": (_I, [_I]),
    "gg_drop_kept_lists": (_I, [_P, _I, _I, _P, _P]),
    "gg_layernorm_fwd_bn_f32_map": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P, _I, _P, _P]),
    "gg_layernorm_bwd_map": (_I, [_P, _P, _P, _P, _P, _L, _I, _P, _P, _P, _P, _I, _P]),
    "gg_tinyvit_set_drop_compact": (_I, [_I]),
}
DROP_SYMBOLS = list(DROP_SIGNATURES)

# every exported symbol of include/gg_pad.h (padded attention windows of TinyViT: a token map the window does not divide), bound from the same libgg.so
PAD_SIGNATURES = {
    "gg_window_pad": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "gg_window_crop_add": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
}
PAD_SYMBOLS = list(PAD_SIGNATURES)
PROF_CAT_PAD = 7                          # GG_CAT_PAD (csrc/prof.h): the launch profiler's category of the two kernels

# every exported symbol of include/gg_aug.h (the device-side training transform of the classifier fine-tune: crop, flip, RandAugment, normalise), bound from the same libgg.so
AUG_SIGNATURES = {
    "gg_aug_workspace_bytes": (_L, [C.POINTER(AugArgs)]),
    "gg_aug_batch": (_I, [C.POINTER(AugArgs), _P]),
}
AUG_SYMBOLS = list(AUG_SIGNATURES)

# every exported symbol of include/gg_fp8.h (the CLIP tower's fp8 inference mode: W8A8 e4m3 GEMM, row quantiser, LayerNorm + quantiser), bound from the same libgg.so
FP8_SIGNATURES = {
    "gg_gemm_nt_e4m3": (_I, [C.POINTER(GemmArgs), _P, _P, _P]),
    "gg_quant_rows_e4m3": (_I, [_P, _I, _L, _L, _I, _P, _L, _P, _P]),
    "gg_layernorm_fwd_e4m3": (_I, [_P, _P, _P, _L, _I, _F, _P, _L, _P, _P]),
}
FP8_SYMBOLS = list(FP8_SIGNATURES)

# every exported symbol of include/gg_eval.h (the eval transform of the raw-image path for whole batches: Pillow resize, crop, 1/255, normalise), bound from the same libgg.so
EVAL_SIGNATURES = {
    "gg_eval_workspace_bytes": (_L, [C.POINTER(EvalArgs)]),
    "gg_eval_batch": (_I, [C.POINTER(EvalArgs), _P]),
}
EVAL_SYMBOLS = list(EVAL_SIGNATURES)

# every exported symbol of include/gg_jpeg.h (baseline JPEG decoding of whole batches: host-side plan, entropy decode, inverse DCT, upsample + colour + pack), bound from the same libgg.so
JPEG_MAX_B = 4096                         # GG_JPEG_MAX_B
JPEG_SIGNATURES = {
    "gg_jpeg_refusal_name": (C.c_char_p, [_I]),
    "gg_jpeg_plan_create": (_I, [_P, _P, _I, C.POINTER(_P)]),
    "gg_jpeg_plan_destroy": (_I, [_P]),
    "gg_jpeg_plan_info": (_I, [_P, _I, C.POINTER(JpegInfo)]),
    "gg_jpeg_plan_first_refused": (_I, [_P]),
    "gg_jpeg_plan_stream_bytes": (_L, [_P]),
    "gg_jpeg_plan_table_bytes": (_L, [_P]),
    "gg_jpeg_plan_output_bytes": (_L, [_P]),
    "gg_jpeg_plan_fill": (_I, [_P, _P, _P]),
    "gg_jpeg_workspace_bytes": (_L, [_P]),
    "gg_jpeg_decode": (_I, [_P, _P, _L, _P, _L, _P, _P, _L, _P]),
}
JPEG_SYMBOLS = list(JPEG_SIGNATURES)

# every exported symbol of include/gg_jscan.h (the JPEG decoder's opt-in mode with many lanes inside one scan: a plan with a sub-segment table, speculate / resolve / write / DC passes), bound from the same libgg.so
JSCAN_MIN_SPLIT, JSCAN_MAX_SPLIT = 8, 1 << 20        # GG_JSCAN_MIN_SPLIT, GG_JSCAN_MAX_SPLIT
JSCAN_SIGNATURES = {
    "gg_jscan_plan_create": (_I, [_P, _P, _I, _I, C.POINTER(_P)]),
    "gg_jscan_plan_subsegments": (_I, [_P, _I]),
    "gg_jscan_plan_total_subsegments": (_L, [_P]),
    "gg_jscan_workspace_bytes": (_L, [_P]),
    "gg_jscan_decode": (_I, [_P, _P, _L, _P, _L, _P, _P, _P, _L, _P]),
}
JSCAN_SYMBOLS = list(JSCAN_SIGNATURES)

# every exported symbol of include/gg_jprog.h (the JPEG decoder's opt-in mode for progressive files: a plan that also takes SOF2, with a scan table; the entropy decode in rounds of scans), bound from the same libgg.so
JPROG_MAX_SCANS = 64                      # GG_JPROG_MAX_SCANS
JPROG_SIGNATURES = {
    "gg_jprog_refusal_name": (C.c_char_p, [_I]),
    "gg_jprog_plan_create": (_I, [_P, _P, _I, C.POINTER(_P)]),
    "gg_jprog_plan_scans": (_I, [_P, _I]),
    "gg_jprog_plan_rounds": (_I, [_P]),
    "gg_jprog_workspace_bytes": (_L, [_P]),
    "gg_jprog_decode": (_I, [_P, _P, _L, _P, _L, _P, _P, _L, _P]),
}
JPROG_SYMBOLS = list(JPROG_SIGNATURES)

# every exported symbol of include/gg_pano.h (the panorama fine-tune's input path for whole batches: Pillow resize, ToTensor, bilinear interpolation, normalise, slot table), bound from the same libgg.so
PANO_MAX_SLOTS, PANO_MAX_IMAGES, PANO_MAX_TARGET = 4096, 4096, 2048        # GG_PANO_MAX_SLOTS, GG_PANO_MAX_IMAGES, GG_PANO_MAX_TARGET
PANO_SIGNATURES = {
    "gg_pano_resized_size": (_I, [_I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "gg_pano_workspace_bytes": (_L, [C.POINTER(PanoArgs)]),
    "gg_pano_batch": (_I, [C.POINTER(PanoArgs), _P]),
}
PANO_SYMBOLS = list(PANO_SIGNATURES)

# every exported symbol of include/gg_attn16.h (the long-sequence attention forward on the 16-bit MFMA and the CLIP tower's opt-in switch to it), bound from the same libgg.so
ATTN16_SIGNATURES = {
    "gg_attention_flash16_fwd": (_I, [C.POINTER(AttnArgs), _I, _P]),
    "gg_attention_flash16_calls": (_L, []),
    "gg_clip_set_attention16": (_I, [_I]),
}
ATTN16_SYMBOLS = list(ATTN16_SIGNATURES)

# every exported symbol of include/gg_attn16w.h (the same forward for TinyViT's windows beyond 256 tokens -- head dim 32, window gather, relative-position bias -- and TinyViT's opt-in switch to it)
ATTN16W_SIGNATURES = {
    "gg_attention_flash16_win_fwd": (_I, [C.POINTER(AttnArgs), _I, _P]),
    "gg_attention_flash16_win_calls": (_L, []),
    "gg_tinyvit_set_attention16": (_I, [_I]),
}
ATTN16W_SYMBOLS = list(ATTN16W_SIGNATURES)

# every exported symbol of include/gg_attn16b.h (the long-sequence attention backward on the 16-bit MFMA and the bf16 CLIP tower's opt-in switch that sends its training step to the 16-bit-MFMA pair)
ATTN16B_SIGNATURES = {
    "gg_attention_flash16_bwd": (_I, [C.POINTER(AttnArgs), _I, _P]),
    "gg_attention_flash16_bwd_calls": (_L, []),
    "gg_clip_set_attention16_train": (_I, [_I]),
}
ATTN16B_SYMBOLS = list(ATTN16B_SIGNATURES)

# every exported symbol of include/gg_attn16wb.h (the same backward for TinyViT's windows beyond 256 tokens -- head dim 32, window gather, relative-position bias and its gradient -- and the bf16 TinyViT's opt-in switch that sends its training step to the 16-bit-MFMA kernels)
ATTN16WB_SIGNATURES = {
    "gg_attention_flash16_win_bwd": (_I, [C.POINTER(AttnArgs), _I, _P]),
    "gg_attention_flash16_win_bwd_calls": (_L, []),
    "gg_attention_flash16_win_dbias_rows": (_L, [_I, _I]),
    "gg_tinyvit_set_attention16_train": (_I, [_I]),
}
ATTN16WB_SYMBOLS = list(ATTN16WB_SIGNATURES)

# every exported symbol of include/gg_wgrad_resident.h (the fp32_split weight gradient of a small dense convolution with the whole output resident in one workgroup), bound from the same libgg.so
WGRAD_RESIDENT_SIGNATURES = {
    "gg_gemm_tn_split3_resident_fits": (_I, [_I, _I]),
    "gg_gemm_tn_split3_resident_splits": (_I, [_I, _I, _I]),
    "gg_gemm_tn_split3_resident": (_I, [_P, _L, _P, _L, _I, _I, _I, _P, _I, _P]),
}
WGRAD_RESIDENT_SYMBOLS = list(WGRAD_RESIDENT_SIGNATURES)

# every exported symbol of include/gg_conv_dgrad_parity.h (the fp32_split data gradient of a 3 x 3 stride-2 convolution by input parity with the BatchNorm-backward epilogue), bound from the same libgg.so
DGRAD_PARITY_SIGNATURES = {
    "gg_conv3x3s2_dgrad_fits": (_I, [_I, _I, _I, _I]),
    "gg_conv3x3s2_dgrad_planes_bytes": (_L, [_I, _I]),
    "gg_conv3x3s2_dgrad_bnbwd_split3": (_I, [_P, _P, _L, _P, _P, _P, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P]),
}
DGRAD_PARITY_SYMBOLS = list(DGRAD_PARITY_SIGNATURES)

# every exported symbol of include/gg_clip_interp.h (the CLIP position table resampled to the grid of a foreign input size, and the adjoint), bound from the same libgg.so
CLIP_INTERP_MAX_SIDE = 64                # GG_CLIP_INTERP_MAX_SIDE
CLIP_INTERP_SIGNATURES = {
    "gg_clip_pos_interp_fwd": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "gg_clip_pos_interp_bwd": (_I, [_P, _I, _I, _I, _I, _P, _P]),
}
CLIP_INTERP_SYMBOLS = list(CLIP_INTERP_SIGNATURES)

# every exported symbol of include/gg_attn_dbias.h (the relative-position bias gradient as a kernel of its own that adds in a fixed order, and TinyViT's opt-in switch that makes the training step use it), bound from the same libgg.so
ATTN_DBIAS_SIGNATURES = {
    "gg_attention_dbias_rows": (_L, [C.POINTER(AttnArgs), _I]),
    "gg_attention_dbias": (_I, [C.POINTER(AttnArgs), _I, _I, _P]),
    "gg_attention_dbias_calls": (_L, []),
    "gg_tinyvit_set_deterministic_dbias": (_I, [_I]),
}
ATTN_DBIAS_SYMBOLS = list(ATTN_DBIAS_SIGNATURES)
PROF_CAT_ATTN_DBIAS = 8                   # GG_CAT_ATTN_DBIAS (csrc/prof.h): the launch profiler's category of gg_attention_dbias


# every exported symbol of include/gg_attn_route.h (the route report of the attention entry points: host arithmetic, no device), its struct and its two enums
class AttnRoutePass(C.Structure):
    _fields_ = [("grid", C.c_uint32), ("block", C.c_uint32), ("lds", C.c_uint32)]


class AttnRoute(C.Structure):           # GgAttnRoute
    _fields_ = [("kernel", C.c_int), ("variant", C.c_int), ("passes", C.c_int), ("pass_", AttnRoutePass * 2), ("dbias_rows", C.c_int64),
                ("reads_ds_scratch", C.c_int), ("rounded_bias", C.c_int)]


ATTN_ENTRIES = ("FWD", "FWD_F16", "BWD", "FLASH_FWD", "FLASH_BWD", "CAUSAL_FWD", "CAUSAL_BWD", "FLASH16_FWD", "FLASH16_WIN_FWD", "FLASH16_BWD", "FLASH16_WIN_BWD")      # GG_ATTN_ENTRY_*
ATTN_KERNELS = ("NONE", "FWD", "FWD_GROUPED", "BWD", "BWD_GROUPED", "FLASH_FWD_RESIDENT", "FLASH_FWD_STREAM", "FLASH_FWD_SPLIT", "FLASH64_FWD_SPLIT", "FLASH_BWD_SPLIT",
                "FLASH_BWD_FUSED", "FLASH_BWD_STREAM", "FLASH_BWD_STREAM_DS", "FLASH64_BWD_SPLIT", "FLASH16_FWD", "FLASH16_WIN_FWD", "FLASH16_BWD", "FLASH16_WIN_BWD")      # GG_ATTN_KERNEL_*
ATTN_ENTRY = {n: i for i, n in enumerate(ATTN_ENTRIES)}
ATTN_KERNEL = {n: i for i, n in enumerate(ATTN_KERNELS)}
ATTN_ROUTE_SIGNATURES = {
    "gg_attention_route": (_I, [C.POINTER(AttnArgs), _I, _I, C.POINTER(AttnRoute)]),
}
ATTN_ROUTE_SYMBOLS = list(ATTN_ROUTE_SIGNATURES)


def attention_route(args: "AttnArgs", entry: str, dtype: int = 0) -> "AttnRoute":
    """What ``gg_attention_route`` reports for exactly these arguments (``entry``: a name of ATTN_ENTRIES); a refusal raises with the entry point's own text."""
    r = AttnRoute()
    if lib().gg_attention_route(C.byref(args), ATTN_ENTRY[entry], dtype, C.byref(r)) != 0:
        raise GgError(lib().gg_last_error().decode(errors="replace"))
    return r


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GgError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(TEXT_SIGNATURES.items()) + list(TEXT_TRAIN_SIGNATURES.items()) + list(CLS_SIGNATURES.items()) + list(DROP_SIGNATURES.items()) + list(PAD_SIGNATURES.items()) + list(AUG_SIGNATURES.items()) + list(FP8_SIGNATURES.items()) + list(EVAL_SIGNATURES.items()) + list(JPEG_SIGNATURES.items()) + list(JSCAN_SIGNATURES.items()) + list(JPROG_SIGNATURES.items()) + list(PANO_SIGNATURES.items()) + list(ATTN16_SIGNATURES.items()) + list(ATTN16W_SIGNATURES.items()) + list(ATTN16B_SIGNATURES.items()) + list(ATTN16WB_SIGNATURES.items()) + list(ATTN_ROUTE_SIGNATURES.items()) + list(WGRAD_RESIDENT_SIGNATURES.items()) + list(DGRAD_PARITY_SIGNATURES.items()) + list(CLIP_INTERP_SIGNATURES.items()) + list(ATTN_DBIAS_SIGNATURES.items()):
            fn = getattr(l, name)           # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise GgError(f"{what or 'libgg'} failed ({rc}): {lib().gg_last_error().decode(errors='replace')}")


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise GgError("no HIP device visible: the geoguessr_ai_amd hot path only runs on an MI355X (gfx950); "
                      "there is no CPU fallback")


def ptr(t: Optional[torch.Tensor], dtype: Optional[torch.dtype] = None, name: str = "tensor") -> Optional[int]:
    """Device pointer of a contiguous GPU tensor (None passes through as NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise GgError(f"{name} must live on the GPU (got device {t.device}); there is no CPU fallback")
    if not t.is_contiguous():
        raise GgError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise GgError(f"{name} must be {dtype}, got {t.dtype}")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def f32(x: float) -> C.c_float:
    return C.c_float(float(x))


def source_hash() -> str:
    """sha256 over the sources libgg.so is built from (csrc/* and include/gg.h, in name order): identifies the build that a committed profile
    (profiles/*_hbm_traffic_pmc_*.json) was measured on -- bench.py marks its traffic figure stale when the running tree differs."""
    import hashlib
    root = os.path.dirname(os.path.abspath(__file__))
    files = sorted(os.path.join(root, "csrc", f) for f in os.listdir(os.path.join(root, "csrc")) if f.endswith((".hip", ".h", ".cpp", "Makefile")))
    files.append(os.path.join(os.path.dirname(root), "include", "gg.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_clip_text.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_clip_text_train.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_cls.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_drop.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_pad.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_aug.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_fp8.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_eval.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_jpeg.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_jscan.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_jprog.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_pano.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_attn16.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_attn16w.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_attn16b.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_attn16wb.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_attn_route.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_wgrad_resident.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_conv_dgrad_parity.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_clip_interp.h"))
    files.append(os.path.join(os.path.dirname(root), "include", "gg_attn_dbias.h"))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()
