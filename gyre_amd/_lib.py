"""ctypes binding of libgyre_hip.so (C ABI: include/gyre_hip.h).

There is NO fallback: if the HIP library is missing or fails to load, every entry
point raises.  A silent PyTorch/CPU path would void the parity claims.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch  # noqa: F401  (must be imported first: maps torch's libamdhip64.so.7, which our .so then shares)

_HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LEVELS = 8

F32, BF16, F16 = 0, 1, 2
_TORCH_DTYPE = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
# One library per 16-bit STORAGE type, same sources and same ABI (csrc/common.h, gyre_storage_dtype()): bf16 (default) and fp16 - the
# reference's own GPU arithmetic (manager.py:146-151 loads fp16).  A module picks its library by the dtype of its parameters
# (modules._NativeModule._storage): float16 -> F16, bfloat16 -> BF16, float32 -> the process default, which is BF16 unless
# GYRE_STORAGE=f16 is set (how the test suite runs every raw-operator test on the fp16 flavour) or set_default_storage() is called.
# (GYRE_HIP_LIB / GYRE_HIP_LIB_F16: tuning / reproducer builds of the same ABI.)
LIB_PATHS = {BF16: os.environ.get("GYRE_HIP_LIB") or os.path.join(_HERE, "libgyre_hip.so"),
             F16: os.environ.get("GYRE_HIP_LIB_F16") or os.path.join(_HERE, "libgyre_hip_f16.so")}
LIB_PATH = LIB_PATHS[BF16]
_default_storage = F16 if os.environ.get("GYRE_STORAGE", "").lower() in ("f16", "fp16", "float16", "half") else BF16
STORAGE_TORCH_DTYPE = {BF16: torch.bfloat16, F16: torch.float16}


def default_storage() -> int:
    return _default_storage


def set_default_storage(storage: int) -> int:
    """Process-wide default storage flavour (BF16 / F16) for float32-parameter modules, lib() without an argument and the
    profiler helpers.  Returns the previous value."""
    global _default_storage
    if storage not in LIB_PATHS:
        raise ValueError("storage must be _lib.BF16 or _lib.F16")
    old, _default_storage = _default_storage, storage
    return old


def storage_for(dtype: torch.dtype) -> int:
    return F16 if dtype == torch.float16 else BF16 if dtype == torch.bfloat16 else _default_storage


class GyreError(RuntimeError):
    pass


class UNetCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32), ("n_levels", C.c_int32),
                ("block_out_channels", C.c_int32 * MAX_LEVELS), ("layers_per_block", C.c_int32),
                ("attn_levels", C.c_int32 * MAX_LEVELS), ("num_heads", C.c_int32 * MAX_LEVELS),
                ("transformer_depth", C.c_int32 * MAX_LEVELS), ("cross_attention_dim", C.c_int32),
                ("norm_num_groups", C.c_int32), ("use_linear_projection", C.c_int32),
                ("flip_sin_to_cos", C.c_int32), ("freq_shift", C.c_float)]


class VAECfg(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32), ("latent_channels", C.c_int32),
                ("n_levels", C.c_int32), ("block_out_channels", C.c_int32 * MAX_LEVELS),
                ("layers_per_block", C.c_int32), ("norm_num_groups", C.c_int32)]


class T2ICfg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("cin", C.c_int32), ("channels", C.c_int32 * 4), ("n_levels", C.c_int32),
                ("nums_rb", C.c_int32), ("ksize", C.c_int32), ("sk", C.c_int32), ("use_conv", C.c_int32)]


class T2ISeqCfg(C.Structure):
    """gyre_t2i_seq_cfg (include/gyre_hip.h): kind 0 = style adapter, 1 = co-adapter fuser."""
    _fields_ = [("kind", C.c_int32), ("width", C.c_int32), ("num_head", C.c_int32), ("n_layers", C.c_int32), ("num_token", C.c_int32),
                ("context_dim", C.c_int32), ("unet_channels", C.c_int32 * 4)]


class FuserInput(C.Structure):
    """gyre_fuser_input (include/gyre_hip.h): one co-adapter's four spatial states (tokens == 0) or its token tensor."""
    _fields_ = [("task", C.c_int32), ("tokens", C.c_int32), ("in_", C.c_void_p * 4), ("h", C.c_int32 * 4), ("w", C.c_int32 * 4)]


class CtrlCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("n_levels", C.c_int32), ("block_out_channels", C.c_int32 * MAX_LEVELS),
                ("layers_per_block", C.c_int32), ("attn_levels", C.c_int32 * MAX_LEVELS), ("num_heads", C.c_int32 * MAX_LEVELS),
                ("transformer_depth", C.c_int32 * MAX_LEVELS), ("cross_attention_dim", C.c_int32), ("norm_num_groups", C.c_int32),
                ("use_linear_projection", C.c_int32), ("flip_sin_to_cos", C.c_int32), ("freq_shift", C.c_float),
                ("cond_channels", C.c_int32), ("cond_embed_channels", C.c_int32 * 4)]


class RRDBCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_in_ch", "num_out_ch", "num_feat", "num_block", "num_grow_ch", "scale", "plus")]


class SwinIRCfg(C.Structure):
    """gyre_swinir_cfg (include/gyre_hip.h)."""
    _fields_ = [("in_chans", C.c_int32), ("embed_dim", C.c_int32), ("num_layers", C.c_int32), ("depths", C.c_int32 * 16),
                ("num_heads", C.c_int32 * 16), ("window_size", C.c_int32), ("mlp_hidden", C.c_int32), ("upscale", C.c_int32),
                ("img_range", C.c_float), ("resi_3conv", C.c_int32)]


class HATCfg(C.Structure):
    """gyre_hat_cfg (include/gyre_hip.h)."""
    _fields_ = [("in_chans", C.c_int32), ("embed_dim", C.c_int32), ("num_layers", C.c_int32), ("depths", C.c_int32 * 16),
                ("num_heads", C.c_int32 * 16), ("window_size", C.c_int32), ("mlp_hidden", C.c_int32), ("upscale", C.c_int32),
                ("img_range", C.c_float), ("compress_ratio", C.c_int32), ("squeeze_factor", C.c_int32), ("conv_scale", C.c_float),
                ("overlap_ratio", C.c_float)]


class LineartCfg(C.Structure):
    """gyre_lineart_cfg (include/gyre_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("input_nc", "output_nc", "n_residual_blocks", "sigmoid")]


class HedCfg(C.Structure):
    """gyre_hed_cfg (include/gyre_hip.h): the network has no constructor arguments."""
    _fields_ = [("reserved", C.c_int32)]


class MlsdCfg(C.Structure):
    """gyre_mlsd_cfg (include/gyre_hip.h): the network has no constructor arguments."""
    _fields_ = [("reserved", C.c_int32)]


class MlsdFoldArgs(C.Structure):
    """gyre_mlsd_fold_args (include/gyre_hip.h): one launch of the BatchNorm fold, for tests."""
    _fields_ = [(n, C.c_void_p) for n in ("w", "conv_bias", "gamma", "beta", "mean", "var", "out", "bias")] + \
               [(n, C.c_int32) for n in ("kind", "O", "I", "taps", "o_pad", "i_pad")]


class HedFuseArgs(C.Structure):
    """gyre_hed_fuse_args (include/gyre_hip.h): one launch of the HED fuse kernel, for tests."""
    _fields_ = [("so", C.c_void_p * 5)] + [(n, C.c_int32 * 5) for n in ("Hk", "Wk", "oy", "ox")] + \
               [("wf", C.c_void_p), ("bf", C.c_void_p), ("out", C.c_void_p), ("out_dtype", C.c_int32)] + \
               [(n, C.c_int32) for n in ("B", "H", "W")]


class InormApplyArgs(C.Structure):
    """gyre_inorm_apply_args (include/gyre_hip.h): one launch of the instance-normalisation apply pass, for tests."""
    _fields_ = [(n, C.c_void_p) for n in ("x", "stats", "res", "out")] + \
               [(n, C.c_int32) for n in ("B", "H", "W", "C", "shuffled", "relu", "res_pad", "pad", "patch")]


class RdbEpilogue(C.Structure):
    """gyre_rdb_epilogue (include/gyre_hip.h): v = alpha (acc + bias); leaky-relu(0.2) if act; + beta1 r1; + beta2 r2."""
    _fields_ = [("bias", C.c_void_p), ("alpha", C.c_float), ("act", C.c_int32), ("r1", C.c_void_p), ("ldr1", C.c_int32),
                ("beta1", C.c_float), ("r2", C.c_void_p), ("ldr2", C.c_int32), ("beta2", C.c_float)]


class RdbConvArgs(C.Structure):
    """gyre_rdb_conv_args (include/gyre_hip.h): one launch of the dense-block convolution, for tests and tuning."""
    _fields_ = [("x", C.c_void_p)] + [(n, C.c_int32) for n in ("ldx", "Cin", "B", "H", "W", "ups")] + [("w", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("w_rows", "NT", "N_live")] + [("out", C.c_void_p), ("c0", C.c_int32), ("ldo", C.c_int32),
                                                                        ("epi", C.POINTER(RdbEpilogue)), ("wpack", C.c_void_p),
                                                                        ("wpack_bytes", C.c_size_t)]


class GemmTestArgs(C.Structure):
    """gyre_gemm_test_args (include/gyre_hip.h): one GEMM / conv launch field by field, for tests and tuning."""
    _fields_ = [(n, C.c_int32) for n in ("conv", "M", "K", "N", "geglu", "B", "Hi", "Wi", "Cin", "stride", "pad", "ups", "Hup", "Wup",
                                         "wrap", "C1", "lda", "lda2", "ldc", "ldr", "rows_per_sample", "ld_rowbias", "samples",
                                         "out_mode", "out_dtype", "tokens", "ldt", "colstat_unit")] + \
               [(n, C.c_void_p) for n in ("A", "A2", "W", "bias", "rowbias", "residual", "out", "ws")] + [("ws_bytes", C.c_size_t)] + \
               [("sc_A", C.c_void_p), ("sc_A2", C.c_void_p)] + [(n, C.c_int32) for n in ("sc_K", "sc_C1", "sc_lda", "sc_lda2")]


class UpsampleConvTestArgs(C.Structure):
    """gyre_upsample_conv_test_args (include/gyre_hip.h): an upsampler conv in the four-parity 2x2 form, for tests and tuning."""
    _fields_ = [(n, C.c_int32) for n in ("B", "Hi", "Wi", "Cin", "N", "splits", "colstat_unit")] + \
               [(n, C.c_void_p) for n in ("x", "w", "bias", "out", "colstat_out", "scratch")] + [("scratch_bytes", C.c_size_t)] + \
               [("ws", C.c_void_p), ("ws_bytes", C.c_size_t)]


class LoraPair(C.Structure):
    """gyre_lora_pair (include/gyre_hip.h): one up / down factor pair of a LoRA, device pointers."""
    _fields_ = [("up", C.c_void_p), ("down", C.c_void_p), ("dtype", C.c_int), ("rank", C.c_int), ("scale", C.c_float)]


class DeltaTerm(C.Structure):
    """gyre_delta_term (include/gyre_hip.h): one LyCORIS term of a delta-merge repack, device pointers."""
    _fields_ = [("kind", C.c_int), ("up", C.c_void_p * 2), ("down", C.c_void_p * 2), ("dtype", C.c_int * 2), ("rank", C.c_int * 2),
                ("w1", C.c_void_p), ("O1", C.c_int), ("I1", C.c_int), ("scale", C.c_float)]


DELTA_MAX_TERMS = 8
DELTA_LORA, DELTA_HADA, DELTA_KRON, DELTA_FULL = 0, 1, 2, 3
_vp, _i, _sz, _f = C.c_void_p, C.c_int, C.c_size_t, C.c_float
_SIGS = {
    "gyre_abi_version": (C.c_int, []),
    "gyre_storage_dtype": (C.c_int, []),
    "gyre_last_error": (C.c_char_p, []),
    "gyre_last_launch_count": (C.c_int64, []),
    "gyre_unet_create": (_i, [C.POINTER(UNetCfg), _i, C.POINTER(_vp)]),
    "gyre_unet_destroy": (None, [_vp]),
    "gyre_unet_num_params": (_i, [_vp]),
    "gyre_unet_param_key": (C.c_char_p, [_vp, _i]),
    "gyre_unet_set_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _vp]),
    "gyre_unet_set_weight_lora": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _i, C.POINTER(LoraPair), _vp]),
    "gyre_unet_set_weight_delta": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _i, C.POINTER(DeltaTerm), _vp]),
    "gyre_unet_finalize": (_i, [_vp, _vp]),
    "gyre_unet_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "gyre_unet_forward": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i]),
    "gyre_unet_set_context": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "gyre_unet_set_context_slot": (_i, [_vp, _vp, _vp, _i, _i, _i, _i]),
    "gyre_unet_select_context": (_i, [_vp, _i]),
    "gyre_unet_hint_uniform_timestep": (_i, [_vp, _i]),
    "gyre_unet_hint_cfg_pairs": (_i, [_vp, _i]),
    "gyre_unet_set_tome": (_i, [_vp, _i]),
    "gyre_unet_set_tiling": (_i, [_vp, _i]),
    "gyre_vae_set_tiling": (_i, [_vp, _i]),
    "gyre_unet_debug_tap": (_i, [_vp, C.c_char_p, _vp, _sz]),
    "gyre_unet_debug_grad_tap": (_i, [_vp, C.c_char_p, _vp, _sz]),
    "gyre_vae_debug_tap": (_i, [_vp, C.c_char_p, _vp, _sz]),
    "gyre_vae_debug_grad_tap": (_i, [_vp, C.c_char_p, _vp, _sz]),
    "gyre_unet_forward_ex": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i, _vp]),
    "gyre_unet_forward_ctrl": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i, _vp,
                                    C.POINTER(_vp), _i, _i, _vp, C.POINTER(_vp), _i]),
    "gyre_unet_vjp_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "gyre_unet_vjp": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _sz, _vp, _i, _vp, _i, _vp]),
    "gyre_unet_vjp_begin": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i, _vp]),
    "gyre_unet_vjp_finish": (_i, [_vp, _vp, _vp, _i, _vp, _i]),
    "gyre_unet_vjp_finish_range": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i]),
    "gyre_unet_vjp_pending": (_i, [_vp]),
    "gyre_vae_create": (_i, [C.POINTER(VAECfg), _i, C.POINTER(_vp)]),
    "gyre_vae_destroy": (None, [_vp]),
    "gyre_vae_num_params": (_i, [_vp]),
    "gyre_vae_param_key": (C.c_char_p, [_vp, _i]),
    "gyre_vae_set_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _vp]),
    "gyre_vae_finalize": (_i, [_vp, _vp]),
    "gyre_vae_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "gyre_vae_encode": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i]),
    "gyre_vae_decode": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i]),
    "gyre_vae_decode_vjp_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "gyre_vae_decode_vjp": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _sz, _vp, _i, _vp, _i]),
    "gyre_t2i_create": (_i, [C.POINTER(T2ICfg), _i, C.POINTER(_vp)]),
    "gyre_t2i_destroy": (None, [_vp]),
    "gyre_t2i_num_params": (_i, [_vp]),
    "gyre_t2i_param_key": (C.c_char_p, [_vp, _i]),
    "gyre_t2i_set_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _vp]),
    "gyre_t2i_finalize": (_i, [_vp, _vp]),
    "gyre_t2i_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "gyre_t2i_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, C.POINTER(_vp), _i, _i]),
    "gyre_t2i_seq_create": (_i, [C.POINTER(T2ISeqCfg), _i, C.POINTER(_vp)]),
    "gyre_t2i_seq_destroy": (None, [_vp]),
    "gyre_t2i_seq_num_params": (_i, [_vp]),
    "gyre_t2i_seq_param_key": (C.c_char_p, [_vp, _i]),
    "gyre_t2i_seq_set_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _vp]),
    "gyre_t2i_seq_finalize": (_i, [_vp, _vp]),
    "gyre_t2i_seq_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "gyre_t2i_style_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp, _i]),
    "gyre_t2i_fuser_forward": (_i, [_vp, _vp, C.POINTER(FuserInput), _i, _i, _i, _vp, _sz, C.POINTER(_vp), _vp]),
    "gyre_rrdb_set_path": (_i, [_vp, _i]),
    "gyre_ctrl_create": (_i, [C.POINTER(CtrlCfg), _i, C.POINTER(_vp)]),
    "gyre_ctrl_destroy": (None, [_vp]),
    "gyre_ctrl_num_params": (_i, [_vp]),
    "gyre_ctrl_param_key": (C.c_char_p, [_vp, _i]),
    "gyre_ctrl_set_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _vp]),
    "gyre_ctrl_finalize": (_i, [_vp, _vp]),
    "gyre_ctrl_bind_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "gyre_ctrl_bind": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _sz]),
    "gyre_ctrl_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "gyre_ctrl_forward": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _sz, C.POINTER(_f), _i, _i, _i, C.POINTER(_vp), _i, _i]),
    "gyre_ctrl_bind_slot_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i, _i]),
    "gyre_ctrl_bind_slot": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(C.c_int32), _i, _i, _vp, _sz]),
    "gyre_ctrl_forward_slot": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _sz, C.POINTER(_f), _i, _i, _i, C.POINTER(_vp), _i,
                                    _i]),
    "gyre_prof_set_mask": (_i, [C.c_uint64]),
    "gyre_prof_num_classes": (_i, []),
    "gyre_prof_class_name": (C.c_char_p, [_i]),
    "gyre_prof_collect": (_i, [C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "gyre_debug_force_gemm_cfg": (_i, [_i]),
    "gyre_debug_set_splitk_workspace": (_i, [_vp, _sz]),
    "gyre_debug_set_ar_workspace": (_i, [_vp, _sz]),
    "gyre_debug_set_wblk_workspace": (_i, [_vp, _sz]),
    "gyre_debug_attn_redo_count": (C.c_long, []),
    "gyre_debug_attn_plan": (_i, [_i] * 10 + [C.POINTER(C.c_int32)]),
    "gyre_debug_attn_bwd_plan": (_i, [_i] * 6 + [C.POINTER(C.c_int32)]),
    "gyre_debug_attn_tables": (_i, [_i, C.POINTER(C.c_int32), _i]),
    "gyre_debug_xattn_stamps": (_i, [_vp]),
    "gyre_debug_force_attn_variant": (_i, [_i]),
    "gyre_debug_gemm_ablation": (_i, [_i]),
    "gyre_debug_ln_linear_folds": (_i, [_i, _i, _i, _i]),
    "gyre_debug_gn_uses_small": (_i, [_i, _i, _i, _i]),
    "gyre_op_gemm_test": (_i, [_vp, C.POINTER(GemmTestArgs)]),
    "gyre_debug_gemm_plan": (_i, [C.POINTER(GemmTestArgs), C.POINTER(C.c_int32)]),
    "gyre_debug_gemm_tiles": (_i, [C.POINTER(C.c_int32), _i]),
    "gyre_debug_ups4_plan": (_i, [_i] * 9 + [C.POINTER(C.c_int32)]),
    "gyre_op_upsample_conv_test": (_i, [_vp, C.POINTER(UpsampleConvTestArgs)]),
    "gyre_set_batch_invariant": (_i, [_i]),
    "gyre_get_batch_invariant": (_i, []),
    "gyre_op_groupnorm": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _sz, _vp]),
    "gyre_op_groupnorm_workspace": (_sz, [_i, _i, _i, _i]),
    "gyre_op_gemm_splitk_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "gyre_op_conv3x3_colstats": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "gyre_op_linear_colstats": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "gyre_op_groupnorm_colstats": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _i, _vp, _i, _i, _vp, _sz, _vp]),
    "gyre_op_gn_fold": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _i, _vp, _i, _i, _vp, _sz, _vp, _vp]),
    "gyre_op_layernorm": (_i, [_vp, _vp, _i, _i, _vp, _vp, _f, _vp]),
    "gyre_op_linear": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp]),
    "gyre_op_linear_t": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _i, _vp]),
    "gyre_op_ln_linear_workspace": (_sz, [_i, _i, _i]),
    "gyre_op_ln_linear": (_i, [_vp, _vp, _i, _i, _vp, _vp, _f, _vp, _i, _vp, _i, _i, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "gyre_op_linear_rowstats_parts": (_i, [_i, _i, _i, _i]),
    "gyre_op_linear_rowstats": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "gyre_op_conv3x3": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    "gyre_op_conv3x3_shortcut": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "gyre_op_compose_proj_out": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "gyre_op_conv3x3_nchw": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _i]),
    "gyre_op_repack_conv_weight": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gyre_op_repack_conv_weight_scaled": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "gyre_op_repack_linear_weight": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "gyre_op_repack_bias": (_i, [_vp, _vp, _i, _i, _vp]),
    "gyre_op_repack_lora": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, C.POINTER(LoraPair), _vp]),
    "gyre_op_repack_delta": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, C.POINTER(DeltaTerm), _vp]),
    "gyre_op_lyco_core": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "gyre_op_merge_delta": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(DeltaTerm), _vp, _i]),
    "gyre_op_attention": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _i]),
    "gyre_op_qkv": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _i]),
    "gyre_op_attention_ex": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i]),
    "gyre_op_groupnorm_bwd_workspace": (_sz, [_i, _i, _i, _i]),
    "gyre_op_groupnorm_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
    "gyre_op_layernorm_bwd": (_i, [_vp, _vp, _vp, _i, _i, _vp, _f, _vp, _vp]),
    "gyre_op_geglu_bwd": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "gyre_op_attention_bwd_workspace": (_sz, [_i, _i, _i, _i, _i]),
    "gyre_op_attention_bwd": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz,
                                   _vp, _i, _vp, _i, _vp, _i]),
    "gyre_op_tome_workspace": (_sz, [_i, _i, _i]),
    "gyre_op_tome_merge": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _i, _vp, _vp]),
    "gyre_op_tome_merge_ex": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "gyre_op_tome_unmerge": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i]),
    "gyre_op_timestep_embedding": (_i, [_vp, _vp, _i, _i, _i, _f, _vp]),
    "gyre_op_rowvec_linear": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _i]),
    "gyre_op_timestep_linear": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp, _vp, _i, _vp, _i]),
    "gyre_op_cross_attention_block": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
    "gyre_op_nchw_to_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gyre_op_copy_probe": (_i, [_vp, _vp, _vp, _sz]),
    "gyre_op_pixel_unshuffle8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "gyre_op_avgpool2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "gyre_op_relu": (_i, [_vp, _vp, _sz]),
    "gyre_op_silu": (_i, [_vp, _vp, _sz]),
    "gyre_op_rdb_tile": (_i, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gyre_op_rdb_conv": (_i, [_vp, C.POINTER(RdbConvArgs)]),
    "gyre_op_rdb_epilogue": (_i, [_vp, _vp, _i, _i, _i, _sz, C.POINTER(RdbEpilogue)]),
    "gyre_op_pixel_unshuffle": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "gyre_op_win_bias": (_i, [_vp, _vp, _i, _vp]),
    "gyre_op_win_attn": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i]),
    "gyre_op_ln_live": (_i, [_vp, _vp, _i, _sz, _i, _vp, _vp, _f, _vp, _i]),
    "gyre_op_swin_act": (_i, [_vp, _vp, _sz, _i, _f]),
    "gyre_op_swin_entry": (_i, [_vp, _vp, _i, _i, _sz, _vp, _f, _vp]),
    "gyre_op_swin_exit": (_i, [_vp, _vp, _i, _i, _sz, _vp, _f, _vp, _i]),
    "gyre_op_hat_attn": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i]),
    "gyre_op_chan_pool_workspace": (_sz, [_i, _sz, _i]),
    "gyre_op_chan_pool": (_i, [_vp, _vp, _i, _i, _sz, _i, _vp, _vp]),
    "gyre_op_chan_gate": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _i]),
    "gyre_op_scale_add": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _sz, _i]),
    "gyre_op_pixel_shuffle2": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _i]),
    "gyre_op_ctrl_emit": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _i, _i, _i]),
    "gyre_op_ctrl_emit_masked": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _i, _i, _i, _vp, _i]),
    "gyre_op_nchw_to_nhwc_masked": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "gyre_op_conv3x3_valid": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp]),
    "gyre_op_inorm_workspace": (_sz, [_i, _sz, _i]),
    "gyre_op_inorm_stats": (_i, [_vp, _vp, _i, _i, _sz, _i, _f, _vp, _vp]),
    "gyre_op_inorm_apply": (_i, [_vp, C.POINTER(InormApplyArgs)]),
    "gyre_op_tconv_compose": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "gyre_op_conv7_in": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "gyre_op_conv7_out": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i]),
    "gyre_hed_geometry": (_i, [_i, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gyre_op_hed_entry": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "gyre_op_hed_tail": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "gyre_op_hed_fuse": (_i, [_vp, C.POINTER(HedFuseArgs)]),
    "gyre_op_mlsd_fold": (_i, [_vp, C.POINTER(MlsdFoldArgs)]),
    "gyre_op_mlsd_entry": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "gyre_op_dwconv3": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    "gyre_op_upsample2_ac": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i]),
    "gyre_op_dconv3_d5": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "gyre_op_mlsd_act": (_i, [_vp, _vp, _sz, _i, _i, _i]),
    "gyre_op_mlsd_relu_add": (_i, [_vp, _vp, _vp, _sz]),
    "gyre_op_mlsd_exit": (_i, [_vp, _vp, _i, _i, _i, _vp, _i]),
    "gyre_op_seq_attn_max_len": (_i, [_i]),
    "gyre_op_seq_attn": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i]),
    "gyre_op_quick_gelu": (_i, [_vp, _vp, _sz]),
    "gyre_op_fuser_pool": (_i, [_vp, _vp, _i, _i, _sz, _vp, _i]),
    "gyre_op_fuser_gain": (_i, [_vp, _vp, _vp, _i, _i, _i, _sz, _vp, _i]),
}
# the handle surface of the three upscaler families and of the three hinters: image in, image out
for _kind, _cfg in (("rrdb", RRDBCfg), ("swinir", SwinIRCfg), ("hat", HATCfg), ("lineart", LineartCfg), ("hed", HedCfg),
                    ("mlsd", MlsdCfg)):
    _SIGS.update({f"gyre_{_kind}_create": (_i, [C.POINTER(_cfg), _i, C.POINTER(_vp)]),
                  f"gyre_{_kind}_destroy": (None, [_vp]),
                  f"gyre_{_kind}_num_params": (_i, [_vp]),
                  f"gyre_{_kind}_param_key": (C.c_char_p, [_vp, _i]),
                  f"gyre_{_kind}_set_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i, _vp]),
                  f"gyre_{_kind}_finalize": (_i, [_vp, _vp]),
                  f"gyre_{_kind}_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
                  f"gyre_{_kind}_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp, _i])})
EXPORTED_SYMBOLS = tuple(_SIGS)

_libs: dict = {}
import threading as _threading
_tls = _threading.local()          # .last = the library this thread asked for last (check() reads ITS thread-local error string)


def lib(storage: Optional[int] = None) -> C.CDLL:
    """Load (once) and return the native library of the given storage flavour (None = the process default).  Raises GyreError if
    it is not built."""
    storage = _default_storage if storage is None else storage
    l = _libs.get(storage)
    if l is None:
        path = LIB_PATHS[storage]
        if not os.path.exists(path):
            raise GyreError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            f"(hipcc --offload-arch=gfx950).  There is no non-HIP fallback.")
        try:
            # local scope: both flavours export the same symbol names (each is linked -Bsymbolic and binds its own)
            l = C.CDLL(path, mode=getattr(os, "RTLD_LOCAL", 0) | getattr(os, "RTLD_NOW", 2))
        except OSError as e:  # pragma: no cover
            raise GyreError(f"cannot load {path}: {e}") from e
        missing = [name for name in _SIGS if not hasattr(l, name)]
        if missing:      # a library built from older sources: the ABI number has stayed 1 over additions, so say it here and not at a call
            raise GyreError(f"{path} is stale: it lacks {len(missing)} entry point(s) ({', '.join(missing[:4])}"
                            f"{', ...' if len(missing) > 4 else ''}); run `python -c 'import __graft_entry__ as g; g.build()'`")
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        if l.gyre_abi_version() != 1:
            raise GyreError("libgyre_hip ABI version mismatch")
        if l.gyre_storage_dtype() != storage:
            raise GyreError(f"{path} stores dtype code {l.gyre_storage_dtype()}, expected {storage}")
        _libs[storage] = l
    _tls.last = l
    return l


def all_libs():
    """Both flavours (loading them): for process-/thread-wide planner switches that must hold whichever library a module uses."""
    return [lib(BF16), lib(F16)]


_EXC = {-1: ValueError, -2: KeyError, -3: GyreError, -4: GyreError, -5: GyreError, -6: NotImplementedError}


def check(rc: int, L: Optional[C.CDLL] = None) -> None:
    """Map a gyre_status to the Python exception the reference's error plumbing expects
    (services/exception_to_grpc: NotImplementedError -> UNIMPLEMENTED, ValueError -> generic).  L = the library the failing
    call went to (its thread-local error string; default: the library this thread asked lib() for last)."""
    if rc != 0:
        msg = (L or getattr(_tls, "last", None) or lib()).gyre_last_error().decode(errors="replace")
        raise _EXC.get(rc, GyreError)(f"libgyre_hip: {msg} (status {rc})")


def dtype_code(t: torch.Tensor) -> int:
    try:
        return _TORCH_DTYPE[t.dtype]
    except KeyError:
        raise ValueError(f"unsupported dtype {t.dtype}; use float32, bfloat16 or float16") from None


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_gpu_tensor(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise GyreError(f"{name} must live on the GPU: the native path has no CPU fallback (got {t.device})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def prof_enable(class_prefixes=None) -> None:
    """Enable HIP-event timing for the kernel classes whose name starts with one of the prefixes
    (None = all, [] = off)."""
    L = lib()
    n = L.gyre_prof_num_classes()
    mask = 0
    for k in range(n):
        name = L.gyre_prof_class_name(k).decode()
        if class_prefixes is None or any(name.startswith(p) for p in class_prefixes):
            mask |= 1 << k
    L.gyre_prof_set_mask(mask)


def prof_collect() -> dict:
    """{class name: dict(launches, ms, flops, bytes)}; call after synchronising the stream."""
    L = lib()
    n = L.gyre_prof_num_classes()
    la, ms, fl, by = (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)(), (C.c_double * n)()
    L.gyre_prof_collect(la, ms, fl, by)
    return {L.gyre_prof_class_name(k).decode(): dict(launches=int(la[k]), ms=float(ms[k]), flops=float(fl[k]),
                                                       bytes=float(by[k])) for k in range(n) if la[k]}
