"""ctypes binding of libanyref_hip.so (include/anyref_hip.h, include/anyref_hip_ops.h).

The shared library is built in-tree by `__graft_entry__.build()` / `make -C anyref_amd/csrc`.
There is no fallback: if it is missing, importing the compute path raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  -- BEFORE the library: torch brings its own HIP runtime, and a process that loads
# libanyref_hip.so (and with it /opt/rocm's runtime) first ends with "no HIP device visible" in anyref_create

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libanyref_hip.so")

ABI_VERSION = 2
F32, BF16, F16 = 0, 1, 2
MODE_PARITY, MODE_PERF, MODE_PERF_FP8W, MODE_PARITY16, MODE_PERF_F16, MODE_PARITY16_F16 = 0, 1, 2, 3, 4, 5
MODE_PERF_INT4W = 6


class AnyrefConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("mode", C.c_int32),
        ("clip_image", C.c_int32), ("clip_patch", C.c_int32), ("clip_dim", C.c_int32),
        ("clip_heads", C.c_int32), ("clip_layers_run", C.c_int32), ("clip_mlp", C.c_int32),
        ("clip_eps", C.c_float),
        ("llm_vocab", C.c_int32), ("llm_dim", C.c_int32), ("llm_heads", C.c_int32),
        ("llm_layers", C.c_int32), ("llm_mlp", C.c_int32), ("llm_max_seq", C.c_int32),
        ("llm_rms_eps", C.c_float), ("llm_rope_theta", C.c_float),
        ("sam_img", C.c_int32), ("sam_patch", C.c_int32), ("sam_dim", C.c_int32), ("sam_depth", C.c_int32),
        ("sam_heads", C.c_int32), ("sam_mlp_ratio", C.c_int32), ("sam_window", C.c_int32),
        ("sam_n_global", C.c_int32), ("sam_global_idx", C.c_int32 * 8),
        ("sam_out_chans", C.c_int32), ("dec_heads", C.c_int32), ("dec_mlp", C.c_int32),
        ("dec_depth", C.c_int32), ("num_mask_tokens", C.c_int32),
        ("out_dim", C.c_int32), ("audio_dim", C.c_int32),
        ("seg_lo", C.c_int32), ("seg_hi", C.c_int32),
        ("rephrase_weight", C.c_float),
        ("max_batch", C.c_int32), ("max_seg", C.c_int32),
        ("aud_dim", C.c_int32), ("aud_blocks", C.c_int32), ("aud_heads", C.c_int32), ("aud_mel", C.c_int32),
        ("aud_len", C.c_int32), ("aud_kernel", C.c_int32), ("aud_stride", C.c_int32), ("aud_clips", C.c_int32),
    ]


_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_L = C.c_int64


class GemmEx(C.Structure):
    """anyref_gemm_ex (include/anyref_hip_ops.h)"""
    _fields_ = ([(n, _P) for n in ("A", "W", "bias", "C", "resid", "row_map", "a_row_map", "norm_gain", "norm_bias",
                                   "norm_out", "slabs_out")] +
                [(n, _L) for n in ("sA", "sW", "sC", "sR", "sBias")] +
                [(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldw", "ldc", "ldr", "norm_ld", "act", "c_f32",
                                          "swiglu_pairs", "slabs", "max_wg", "batch")] +
                [("alpha", _F), ("norm_eps", _F), ("norm_done", C.c_int32)])


class NormEx(C.Structure):
    """anyref_norm_ex"""
    _fields_ = ([(n, _P) for n in ("x", "gain", "bias", "y", "row_map", "fill_dst", "fill_rows", "fill_bias")] +
                [(n, C.c_int32) for n in ("M", "D", "ldx", "ldy", "rms", "y_f32", "act", "fill_ld", "fill_n", "fill_N",
                                          "fill_fallback")] +
                [("eps", _F), ("fill_done", C.c_int32)])


class AttnEx(C.Structure):
    """anyref_attn_ex"""
    _fields_ = ([(n, _P) for n in ("q", "k", "v", "o", "q_pos0", "kv_len", "q_len", "rel_h", "rel_w", "rel_p",
                                   "rel_tab_h", "rel_tab_w")] +
                [(n, _L) for n in ("q_bs", "q_rs", "q_hs", "k_bs", "k_rs", "k_hs", "v_bs", "v_rs", "v_hs", "o_bs", "o_rs",
                                   "o_hs", "rel_hs")] +
                [(n, C.c_int32) for n in ("B", "H", "Sq", "Sk", "hd", "causal", "kh", "kw", "rel_ld", "rel_tab_ld",
                                          "max_wg")] +
                [("scale", _F)])


class SpatialPrompts(C.Structure):
    """anyref_spatial_prompts (include/anyref_hip.h)"""
    _fields_ = [("points", _P), ("labels", _P), ("n_points", C.c_int32), ("boxes", _P), ("mask_input", _P),
                ("multimask", C.c_int32)]


class LoraPair(C.Structure):
    """anyref_lora_pair (include/anyref_hip.h)"""
    _fields_ = [("weight_name", C.c_char_p), ("A", _P), ("B", _P), ("r", C.c_int32), ("is_device", C.c_int32),
                ("transposed", C.c_int32)]


# projection bits of anyref_adapter_reserve (ANYREF_LORA_*)
LORA_Q, LORA_K, LORA_V, LORA_O, LORA_GATE, LORA_UP, LORA_DOWN = 1, 2, 4, 8, 16, 32, 64

# name -> (restype, argtypes): every symbol the two headers declare
SYMBOLS = {
    "anyref_create": (_I, [C.POINTER(AnyrefConfig), _I, C.POINTER(_P)]),
    "anyref_destroy": (None, [_P]),
    "anyref_last_error": (C.c_char_p, [_P]),
    "anyref_set_weight": (_I, [_P, C.c_char_p, _P, _I, _I, C.POINTER(_L), _I]),
    "anyref_finalize": (_I, [_P]),
    "anyref_generate": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P, _L, _P,
                             _P, _P]),
    "anyref_forward_teacher": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _L, _P, _P,
                                    _P, _P]),
    "anyref_encode_images": (_I, [_P, _P, _P, _I, _P, _P]),
    "anyref_sam_encode": (_I, [_P, _P, _P, _I, _P]),
    "anyref_mask_decode": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P]),
    "anyref_prompt_reserve": (_I, [_P, _I]),
    "anyref_mask_decode_prompted": (_I, [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]),
    "anyref_refine_masks": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "anyref_refine_embedding": (_I, [_P, _P, _I, _I, _P]),
    "anyref_llm_forward": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "anyref_llm_extend": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "anyref_set_draft": (_I, [_P, _P, _P, _I, _I]),
    "anyref_draft_stats": (_I, [_P, _P, _P, _I, _P, _P]),
    "anyref_set_token_scores": (_I, [_P, _I]),
    "anyref_token_scores": (_I, [_P, _I, _I, _P, _P, _P]),
    "anyref_set_mask_reports": (_I, [_P, _I, _F]),
    "anyref_set_packed_masks": (_I, [_P, _P, _L]),
    "anyref_mask_reports": (_I, [_P, _I, _I, _P, _P, _P]),
    "anyref_session_open": (_I, [_P, _P, _P, _P, _P, _I, _P, _P]),
    "anyref_session_generate": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _L, _P, _P, _P]),
    "anyref_session_close": (_I, [_P]),
    "anyref_session_pool_reserve": (_I, [_P, _I, _I]),
    "anyref_session_store": (_I, [_P, _P, _I]),
    "anyref_session_generate_pooled": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _L, _P, _P, _P]),
    "anyref_session_slot_close": (_I, [_P, _I]),
    "anyref_session_pool_stats": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_L), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "anyref_adapter_reserve": (_I, [_P, C.c_uint32]),
    "anyref_adapter_apply": (_I, [_P, _P, _P, _I, _F]),
    "anyref_update_weight": (_I, [_P, _P, C.c_char_p, _P, _I, _I, C.POINTER(_L), _I]),
    "anyref_adapter_stats": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(_L), C.POINTER(C.c_double)]),
    "anyref_project_audio": (_I, [_P, _P, _P, _I, _P]),
    "anyref_audio_encode": (_I, [_P, _P, _P, _I, _P]),
    "anyref_seg_tail": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _L, _P, _P]),
    "anyref_set_seg_range": (_I, [_P, _I, _I]),
    "anyref_set_overlap": (_I, [_P, _I]),
    "anyref_set_early_tail": (_I, [_P, _I]),
    "anyref_early_masks_done": (_I, [_P]),
    "anyref_set_rephrase_paths": (_I, [_P, _I]),
    "anyref_set_extra_event": (_I, [_P, _P]),
    "anyref_set_graphs": (_I, [_P, _I]),
    "anyref_set_side_share": (_I, [_P, _I, _I]),
    "anyref_profile_enable": (_I, [_P, _I]),
    "anyref_profile_config": (_I, [_P, C.c_char_p, _I]),
    "anyref_profile_collect": (_I, [_P]),
    "anyref_profile_calibrate": (_I, [_P, _P, C.POINTER(C.c_double)]),
    "anyref_profile_read": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(C.c_double), C.POINTER(_L),
                                C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "anyref_stamps_enable": (_I, [_P, _I]),
    "anyref_stamps_collect": (_I, [_P, C.POINTER(_L)]),
    "anyref_stamps_dropped": (_I, [_P, C.POINTER(_L)]),
    "anyref_stamps_read": (_I, [_P, _L, C.c_char_p, _I, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_double), C.POINTER(_I)]),
    "anyref_stamps_spread": (_I, [_P, _L, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "anyref_device_bytes": (_L, [_P]),
    "anyref_mode_name": (C.c_char_p, [_P]),
    "anyref_inexact_weights": (_I, [_P, C.POINTER(_L)]),
    # kernel-level test entry points (anyref_hip_ops.h)
    "anyref_op_gemm": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "anyref_op_gemm_fp8": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "anyref_op_quant_fp8": (_I, [_P, _P, _I, _I, _P, _P]),
    "anyref_op_gemv_fp8": (_I, [_P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I, _I, _I]),
    "anyref_op_quant_int4": (_I, [_P, _P, _I, _I, _P, _P]),
    "anyref_op_lora_merge": (_I, [_I, _P, _P, _I, _I, _I, _P, _P, _I, _F, _P, _I, _I, _P]),
    "anyref_op_dequant_int4": (_I, [_P, _P, _P, _I, _I, _P]),
    "anyref_op_gemm_int4": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I]),
    "anyref_op_gemv_int4": (_I, [_P, _P, _P, _F, _P, _P, _P, _P, _P, _P, _I, _I, _I]),
    "anyref_op_iou_counts": (_I, [_P, _P, _P, _I, _L, _P]),
    "anyref_op_avs_counts": (_I, [_P, _P, _P, _I, _L, _P, _I, _F, _P, _P]),
    "anyref_op_sam_preprocess": (_I, [_P, _P, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "anyref_op_pil_resample_u8": (_I, [_P, _P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _I, _P, _P, _I]),
    "anyref_op_pool_ref_tokens": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "anyref_op_kaldi_fbank": (_I, [_P, _P, _I, _I, _I, _I, _I, C.c_float, _P, _I, _P, _P, _I, C.c_float, C.c_float, _P]),
    "anyref_op_clip_finish": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "anyref_op_gemv": (_I, [_I, _P, _P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "anyref_op_gemv_xn": (_I, [_I, _P, _P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _I]),
    "anyref_op_split_roundtrip": (_I, [_I, _P, _P, _P, _P, _I, _I]),
    "anyref_op_rope_table": (_I, [_I, _I, _F, _P]),
    "anyref_op_decode_attn": (_I, [_I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _F, _P, _P, _I]),
    "anyref_op_seg_rephrase": (_I, [_I, _P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _F, _F, _P, _P]),
    "anyref_op_rephrase_chain": (_I, [_I, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _F, _F, _P]),
    "anyref_op_rope_cache": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P]),
    "anyref_op_argmax": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "anyref_op_token_scores": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "anyref_op_mask_report": (_I, [_P, _P, _I, _I, _I, _F, _P, _P]),
    "anyref_op_draft_accept": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "anyref_op_kv_broadcast": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I]),
    "anyref_op_kv_gather": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _I, _P, _I, _I]),
    "anyref_op_norm": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _F, _I]),
    "anyref_op_attention": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _P, _P, _P, _I, _I]),
    "anyref_op_attention_tab": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _I, _I, _I]),
    "anyref_op_gemm_gather": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "anyref_op_attention_relp": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _I, _I, _I]),
    "anyref_op_rel_pos": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "anyref_op_postprocess": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "anyref_op_last_error": (C.c_char_p, []),
    "anyref_op_gemm_ex": (_I, [_I, _P, C.POINTER(GemmEx)]),
    "anyref_op_norm_ex": (_I, [_I, _P, C.POINTER(NormEx)]),
    "anyref_op_attention_ex": (_I, [_I, _P, C.POINTER(AttnEx)]),
    "anyref_op_last_tags": (C.c_char_p, []),
    # glue kernels and the skinny f32 GEMV (tests/test_gpu_glue_ops.py)
    "anyref_op_gemv_skinny": (_I, [_P, _P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I]),
    "anyref_op_upscale1": (_I, [_I, _P, _P, _I, _I, _I, _P, _P, _F, _P]),
    "anyref_op_upscale2_masks": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "anyref_op_dense_pe": (_I, [_P, _P, _I, _I, _P]),
    "anyref_op_build_tokens": (_I, [_P, _P, _I, _P, _I, _I, _P]),
    "anyref_op_prompt_tokens": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _P, _I]),
    "anyref_op_mask_prompt_embed": (_I, [_P] * 13 + [_I, _I, _I, _I, _I, _P, _I]),
    "anyref_op_add_rows": (_I, [_P, _P, _P, _I, _P, _I, _I]),
    "anyref_op_add_vec": (_I, [_P, _P, _P, _P, _I, _I]),
    "anyref_op_embed_splice": (_I, [_P, _P, _P, _I, _I, _P, _I, _I, _P, _I, _P, _I, _I, _P]),
    "anyref_op_scatter_rows": (_I, [_P, _P, _P, _P, _I, _P, _I, _I]),
    "anyref_op_gather_rows": (_I, [_P, _P, _I, _I, _P, _P, _I, _P]),
    "anyref_op_embed_rows": (_I, [_P, _P, _I, _P, _I, _I, _P]),
    "anyref_op_im2col_patch": (_I, [_I, _P, _P, _I, _I, _I, _P, _I]),
    "anyref_op_im2col_3x3": (_I, [_I, _P, _P, _I, _I, _I, _P]),
    "anyref_op_im2col_conv1": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "anyref_op_clip_assemble": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "anyref_op_l2norm_scale": (_I, [_P, _P, _I, _I, _F, _P]),
    "anyref_op_to_f32": (_I, [_P, _P, _I, _P, _L]),
    "anyref_op_dequant_fp8": (_I, [_P, _P, _I, _P, _I, _I, _P, _I]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP backend; raises (never falls back) when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP backend first "
            "(`python -c 'import __graft_entry__ as g; g.build()'` or `make -C anyref_amd/csrc`). "
            "anyref_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
