"""ctypes binding of libdexbotic_amd.so (C ABI declared in include/dexbotic_amd.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent this module
raises at import; every kernel call checks the status code and raises ``DxaError`` with
``dxa_last_error()``.  Build the library with ``python -m dexbotic_amd.build`` (done by
``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

# torch first: the PyTorch-ROCm wheel bundles its own libamdhip64.so.7; whichever copy of that soname is
# mapped first serves the whole process, and device pointers / streams handed to our kernels belong to
# torch's runtime.  Loading libdexbotic_amd.so before torch would bind everything to /opt/rocm's copy,
# which then fails to see the device torch initialised ("no ROCm-capable device").
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DXA_LIB") or os.path.join(_HERE, "libdexbotic_amd.so")   # DXA_LIB: kernel-tuning builds

F32, BF16 = 0, 1
ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_QUICK_GELU, ACT_SILU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3, 4, 5, 6
NT, NN, TN = 0, 1, 2
FILTER_BICUBIC = 3
FILTER_BILINEAR = 2
JITTER_BRIGHTNESS, JITTER_CONTRAST, JITTER_SATURATION, JITTER_HUE = 0, 1, 2, 3
FUSE_NONE, FUSE_SWIGLU = 0, 1

_vp, _i64, _i32, _f32, _sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
_int = C.c_int


class DxaError(RuntimeError):
    pass


class GemmDesc(C.Structure):
    _fields_ = [
        ("layout", _i32), ("in_dtype", _i32), ("out_dtype", _i32), ("act", _i32),
        ("M", _i64), ("N", _i64), ("K", _i64),
        ("A", _vp), ("lda", _i64), ("B", _vp), ("ldb", _i64), ("C", _vp), ("ldc", _i64),
        ("bias", _vp), ("residual", _vp), ("ldr", _i64), ("aux_out", _vp), ("mulgrad", _vp), ("ldg", _i64),
        ("alpha", _f32), ("accumulate", _i32), ("nb", _i32 * 3),
        ("sA", _i64 * 3), ("sB", _i64 * 3), ("sC", _i64 * 3), ("sR", _i64 * 3), ("sG", _i64 * 3),
        ("epi_f32", _i32), ("mirror", _vp), ("sumsq", _vp),
        ("A2", _vp), ("B2", _vp), ("K2", _i64),
        ("fuse", _i32), ("ld_aux", _i64),
    ]


class GemmStepInfo(C.Structure):
    _fields_ = [
        ("kernel", C.c_char_p), ("grid", _i32 * 3), ("block", _i32), ("lds", _i32),
        ("K", _i64), ("K2", _i64), ("a_off", _i64), ("b_off", _i64), ("seg2", _i32),
        ("accumulate", _i32), ("bias", _i32), ("residual", _i32),
        ("tm", _i32), ("tn", _i32), ("full", _i32), ("tail_r", _i32), ("split_s", _i32), ("group_m", _i32),
        ("vecA", _i32), ("vecB", _i32), ("vecC", _i32), ("vecR", _i32), ("vecG", _i32), ("vecBias", _i32),
        ("ksplit", _i32), ("kper", _i32), ("split_ws", _i32), ("mirror", _i32), ("sumsq", _i32),
    ]


class GemmPlanInfo(C.Structure):
    _fields_ = [("nsteps", _i32), ("mirror_pass", _i32), ("sumsq_pass", _i32), ("step", GemmStepInfo * 2)]


class Split3Op(C.Structure):
    _fields_ = [("src", _vp), ("ld", _i64), ("dst", _vp), ("rows", _i64), ("cols", _i64), ("pad", _i64), ("side", _i32), ("transposed", _i32)]


class AttnDesc(C.Structure):
    _fields_ = [
        ("dtype", _i32), ("B", _i32), ("Hq", _i32), ("Hkv", _i32), ("Sq", _i32), ("Sk", _i32), ("D", _i32),
        ("causal", _i32), ("scale", _f32),
        ("q", _vp), ("q_sb", _i64), ("q_sh", _i64), ("q_ss", _i64),
        ("k", _vp), ("k_sb", _i64), ("k_sh", _i64), ("k_ss", _i64),
        ("v", _vp), ("v_sb", _i64), ("v_sh", _i64), ("v_ss", _i64),
        ("o", _vp), ("o_sb", _i64), ("o_sh", _i64), ("o_ss", _i64),
        ("lse", _vp), ("kv_start", _vp), ("kv_end", _vp),
        ("d_o", _vp), ("do_sb", _i64), ("do_sh", _i64), ("do_ss", _i64),
        ("dq", _vp), ("dq_sb", _i64), ("dq_sh", _i64), ("dq_ss", _i64),
        ("dk", _vp), ("dk_sb", _i64), ("dk_sh", _i64), ("dk_ss", _i64),
        ("dv", _vp), ("dv_sb", _i64), ("dv_sh", _i64), ("dv_ss", _i64),
        ("force_generic", _i32),
        ("q_limit", _vp), ("key_valid", _vp), ("drop_mask", _vp),
    ]


class AttnPlanInfo(C.Structure):
    _fields_ = [("family", C.c_char_p), ("D", _i32), ("DV", _i32), ("nw", _i32), ("nw_dkv", _i32), ("pf", _i32), ("nsplit", _i32),
                ("vec", _i32), ("workspace", C.c_uint64)]


NORM_ENTRIES = ("rmsnorm_fwd", "rmsnorm_bwd", "layernorm_fwd", "layernorm_bwd", "add_layernorm_fwd", "add_layernorm_bwd", "colsum",
                "downsample_layernorm_fwd", "downsample_layernorm_bwd", "adarms_fwd", "adarms_bwd", "gated_residual_fwd",
                "gated_residual_bwd")     # enum dxa_norm_entry, in order


class NormDesc(C.Structure):
    _fields_ = [("entry", _i32), ("dtype", _i32), ("w_dtype", _i32), ("accumulate", _i32), ("rows", _i64), ("cols", _i64),
                ("G", _i64), ("rows_per_sample", _i64), ("ld", _i64), ("gate_ld", _i64), ("dgate_ld", _i64),
                ("partial_bytes", _sz)] + [(n, _vp) for n in ("x", "x2", "w", "b", "y", "dy", "dx", "residual", "partial", "mean",
                                                             "rstd", "gate", "mod", "aux", "dgate", "dmod")] + \
               [("have_counters", _i32), ("capturing", _i32)]


class NormPlanInfo(C.Structure):
    _fields_ = [("kernel", C.c_char_p), ("kernel2", C.c_char_p), ("mode", C.c_char_p), ("vec", _i32), ("grid", _i32 * 3),
                ("block", _i32), ("lds", _i32), ("nsplit", _i32), ("trips", _i64)]


class AdamWDesc(C.Structure):
    _fields_ = [
        ("p", _vp), ("g", _vp), ("m", _vp), ("v", _vp), ("shadow", _vp),
        ("chunk_start", _vp), ("chunk_len", _vp), ("chunk_grp", _vp), ("n_chunks", _i32),
        ("lr", _f32 * 8), ("wd", _f32 * 8),
        ("beta1", _f32), ("beta2", _f32), ("eps", _f32), ("bc1", _f32), ("bc2", _f32),
        ("clip_coef", _vp), ("g_dtype", _i32), ("chunk_state", _vp), ("chunk_mv_start", _vp),
    ]


class ImageDesc(C.Structure):
    _fields_ = [
        ("src", _vp), ("n", _i32), ("h", _i32), ("w", _i32), ("pad", _i32), ("bg", C.c_ubyte * 4),
        ("res_h", _i32), ("res_w", _i32), ("crop_top", _i32), ("crop_left", _i32), ("out_h", _i32), ("out_w", _i32),
        ("row0", _i32), ("rows", _i32), ("hb", _vp), ("hk", _vp), ("hks", _i32), ("vb", _vp), ("vk", _vp), ("vks", _i32),
        ("tmp", _vp), ("out", _vp), ("out_dtype", _i32), ("out_u8", _vp), ("rescale", C.c_double),
        ("mean", _f32 * 3), ("std", _f32 * 3),
    ]


class JitterParams(C.Structure):
    _fields_ = [("apply", _i32), ("order", _i32 * 4), ("brightness", _f32), ("contrast", _f32), ("saturation", _f32), ("hue", _f32)]


class DecodeDesc(C.Structure):
    _fields_ = [
        ("layers", _vp), ("x_in", _vp), ("out", _vp), ("final_norm_w", _vp), ("cos_row", _vp), ("sin_row", _vp),
        ("workspace", _vp), ("workspace_bytes", _sz),
        ("n_layers", _i32), ("d", _i32), ("Hq", _i32), ("Hkv", _i32), ("D", _i32), ("F", _i32), ("slot", _i32), ("kv_lo", _i32),
        ("max_len", _i32), ("eps", _f32), ("qk_norm", _vp),
    ]


# name -> (restype, argtypes); must list EVERY symbol declared in include/dexbotic_amd.h
SIGNATURES = {
    "dxa_last_error": (C.c_char_p, []),
    "dxa_version": (_int, []),
    "dxa_gemm": (_int, [C.POINTER(GemmDesc), _vp]),
    "dxa_gemm_plan": (_int, [C.POINTER(GemmDesc), C.POINTER(GemmPlanInfo)]),
    "dxa_gemm_kernel_name": (C.c_char_p, [_int]),
    "dxa_split3": (_int, [_vp, _i64, _vp, _i64, _i64, _int, _vp]),
    "dxa_split3_t": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _int, _vp]),
    "dxa_split3_pair": (_int, [C.POINTER(Split3Op), C.POINTER(Split3Op), _vp]),
    "dxa_rmsnorm_fwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _f32, _int, _int, _vp]),
    "dxa_rmsnorm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _vp]),
    "dxa_layernorm_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _int, _int, _vp]),
    "dxa_layernorm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _vp]),
    "dxa_norm_bwd_blocks": (_int, [_i64]),
    "dxa_add_layernorm_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _int, _int, _vp]),
    "dxa_add_layernorm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _vp]),
    "dxa_downsample_layernorm_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _f32, _int, _int, _vp]),
    "dxa_downsample_layernorm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_action_put_fwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_action_put_bwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _vp]),
    "dxa_action_layernorm_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _f32, _int, _int, _vp]),
    "dxa_action_layernorm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _vp]),
    "dxa_action_layernorm_bwd_blocks": (_int, [_i64]),
    "dxa_l1_loss": (_int, [_vp, _vp, _vp, _vp, _i64, _f32, _vp]),
    "dxa_action_rows_fwd": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_action_rows_bwd": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_action_fill_fwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_action_fill_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _vp]),
    "dxa_action_fill_bwd_blocks": (_int, [_i64]),
    "dxa_action_bins_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _i64, _int, _vp]),
    "dxa_action_bins_counters": (_int, [_i64]),
    "dxa_bin_logprob_fwd": (_int, [_vp, _i64, _vp, _f32, _vp, _vp, _vp, _i64, _i64, _int, _vp]),
    "dxa_bin_logprob_bwd": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _f32, _vp, _i64, _i64, _int, _vp]),
    "dxa_ppo_clip_fwd": (_int, [_vp, _vp, _vp, _vp, _int, _i64, _f32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "dxa_noisy_embed_fwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _vp]),
    "dxa_noisy_embed_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _vp]),
    "dxa_noisy_embed_bwd_blocks": (_int, [_i64]),
    "dxa_diffusion_put_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_diffusion_put_bwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_ddim_step_embed": (_int, [_vp, _vp, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _vp]),
    "dxa_flow_suffix_in": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_flow_euler_tail": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _int, _f32, _f32, _int, _vp]),
    "dxa_adarms_fwd": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _f32, _int, _vp]),
    "dxa_gated_residual_fwd": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _int, _vp]),
    "dxa_adarms_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _sz, _i64, _i64, _i64, _int, _vp]),
    "dxa_gated_residual_bwd": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _sz, _i64, _i64, _i64, _int, _vp]),
    "dxa_adarms_bwd_groups": (_int, [_i64]),
    "dxa_colsum": (_int, [_vp, _i64, _vp, _i64, _i64, _int, _int, _vp, _sz, _vp]),
    "dxa_norm_plan": (_int, [C.POINTER(NormDesc), C.POINTER(NormPlanInfo)]),
    "dxa_norm_kernel_name": (C.c_char_p, [_int]),
    "dxa_rope_split": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_rope_merge": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_rope_split_at": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_rope_merge_at": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_qknorm_rope_split": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_qknorm_rope_merge": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_qknorm_rope_merge_blocks": (_int, [_i64, _int, _int, _int, _int]),
    "dxa_qknorm_rope_split_at": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_qknorm_rope_merge_from": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_attn_fwd": (_int, [C.POINTER(AttnDesc), _vp]),
    "dxa_attn_fwd_workspace": (_sz, [C.POINTER(AttnDesc)]),
    "dxa_attn_fwd_ws": (_int, [C.POINTER(AttnDesc), _vp, _sz, _vp]),
    "dxa_attn_bwd_workspace": (_sz, [C.POINTER(AttnDesc)]),
    "dxa_attn_bwd": (_int, [C.POINTER(AttnDesc), _vp, _sz, _vp]),
    "dxa_attn_plan": (_int, [C.POINTER(AttnDesc), _int, C.POINTER(AttnPlanInfo)]),
    "dxa_swiglu_fwd": (_int, [_vp, _vp, _i64, _i64, _int, _vp]),
    "dxa_swiglu_bwd": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _vp]),
    "dxa_axpby": (_int, [_vp, _vp, _vp, _i64, _f32, _f32, _int, _vp]),
    "dxa_mul": (_int, [_vp, _vp, _vp, _i64, _int, _vp]),
    "dxa_mul_rows": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp]),
    "dxa_glu_fwd": (_int, [_vp, _vp, _i64, _i64, _int, _int, _vp]),
    "dxa_glu_bwd": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _int, _vp]),
    "dxa_act_fwd": (_int, [_vp, _vp, _i64, _int, _int, _vp]),
    "dxa_act_bwd": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp]),
    "dxa_add": (_int, [_vp, _vp, _vp, _i64, _int, _vp]),
    "dxa_cast": (_int, [_vp, _vp, _i64, _int, _int, _vp]),
    "dxa_copy2d": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_transpose": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_permute_bshd": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _int, _vp]),
    "dxa_splice_fwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _vp]),
    "dxa_splice_bwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _vp]),
    "dxa_zero_rows": (_int, [_vp, _vp, _i64, _i64, _vp]),
    "dxa_gather_rows": (_int, [_vp, _vp, _vp, _i64, _i64, _int, _int, _vp]),
    "dxa_scatter_rows": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _int, _vp]),
    "dxa_im2col": (_int, [_vp, _vp, _int, _int, _int, _int, _i64, _int, _int, _vp]),
    "dxa_vit_embed_fwd": (_int, [_vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _vp]),
    "dxa_vit_embed_bwd": (_int, [_vp, _vp, _int, _int, _int, _int, _vp]),
    "dxa_rope2d_fwd": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp]),
    "dxa_rope2d_bwd": (_int, [_vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp]),
    "dxa_layerscale_residual_fwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _vp]),
    "dxa_layerscale_residual_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _sz, _i64, _i64, _int, _vp]),
    "dxa_layerscale_bwd_rows": (_int, [_i64]),
    "dxa_conv3x3s2_im2col": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp]),
    "dxa_conv3x3s2_col2im": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp]),
    "dxa_qsample": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "dxa_timestep_embedding": (_int, [_vp, _vp, _vp, _i64, _int, _vp]),
    "dxa_dit_assemble_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _vp]),
    "dxa_dit_assemble_bwd": (_int, [_vp, _vp, _vp, _int, _int, _int, _vp]),
    "dxa_token_drop": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "dxa_token_drop_bwd": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _int, _vp]),
    "dxa_dropout_mask": (_int, [_vp, _i64, _f32, C.c_uint64, C.c_uint64, _int, _vp]),
    "dxa_bank_consolidate": (_int, [_vp, _vp, _int, _i64, _i64, _int, _int, _vp, _vp]),
    "dxa_bank_stage_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_bank_stage_bwd": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_bank_append": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_bank_consolidate_batched": (_int, [_vp, _vp, _vp, _int, _int, _int, _vp, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_bank_stage_fwd_at": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_bank_append_at": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_bank_consolidate_batched_at": (_int, [_vp, _vp, _vp, _vp, _int, _int, _int, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_add_rows": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _f32, _int, _vp]),
    "dxa_token_sum": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _int, _vp]),
    "dxa_mse_loss": (_int, [_vp, _vp, _vp, _vp, _i64, _f32, _vp]),
    "dxa_mse_loss_rows": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _vp]),
    "dxa_expectile_loss": (_int, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _vp]),
    "dxa_ddim_step": (_int, [_vp, _vp, _i64, _i64, _int, _f32, _f32, _f32, _f32, _vp]),
    "dxa_adamw": (_int, [C.POINTER(AdamWDesc), _vp]),
    "dxa_sumsq": (_int, [_vp, _i64, _int, _vp, _vp, _int, _vp]),
    "dxa_sumsq_ranges": (_int, [_vp, _int, _vp, _vp, _int, _vp, _vp, _int, _vp]),
    "dxa_sum_f32": (_int, [_vp, _i64, _vp, _int, _vp]),
    "dxa_gemm_sumsq_slots": (_i64, [_i64, _i64]),
    "dxa_cross_entropy_fwd": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp]),
    "dxa_cross_entropy_bwd": (_int, [_vp, _i64, _vp, _vp, _vp, _f32, _vp, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_cross_entropy_rows_bwd": (_int, [_vp, _i64, _vp, _vp, _vp, _f32, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp]),
    "dxa_ce_sample_reduce": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp]),
    "dxa_soft_cross_entropy_fwd": (_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _int, _f32, _int, _vp]),
    "dxa_soft_cross_entropy_bwd": (_int, [_vp, _i64, _vp, _vp, _vp, _f32, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _int, _f32,
                                          _int, _vp]),
    "dxa_argmax_rows": (_int, [_vp, _i64, _vp, _i64, _i64, _int, _vp]),
    "dxa_sample_rows": (_int, [_vp, _i64, _i64, _i64, _int, _f32, _i64, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dxa_resample_ksize":(_int, [_int, _int]),
    "dxa_resample_coeffs": (_int, [_int, _int, _int, _vp, _vp]),
    "dxa_image_preprocess": (_int, [C.POINTER(ImageDesc), _vp]),
    "dxa_resample_ksize_filter": (_int, [_int, _int, _int]),
    "dxa_image_crop_resize": (_int, [_vp, _int, _int, _int, _int, C.c_uint32, _vp, _vp, _int, _vp, _vp, _vp, _int, _int, _vp, _int, _vp, _vp]),
    "dxa_color_jitter": (_int, [_vp, _int, _int, _int, _vp, _vp, _vp, _vp]),
    "dxa_color_jitter_pixels_host": (_int, [_vp, _i64, _vp, _int]),
    "dxa_image_affine": (_int, [_vp, _vp, _int, _int, _int, _vp, _vp, C.c_uint32, _vp]),
    "dxa_image_affine_host": (_int, [_vp, _vp, _int, _int, _int, _vp, C.c_uint32]),
    "dxa_dit_blocks_workspace": (_sz, [_int, _int, _int]),
    "dxa_dit_blocks_fwd": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _int, _f32, _vp, _sz, _vp]),
    "dxa_dit_blocks_status": (_int, [_vp, _vp]),
    "dxa_dit_sample_workspace": (_sz, [_int, _int, _int]),
    "dxa_dit_sample_fwd": (_int, [_vp] * 9 + [_int, _int, _int, _int, _f32, _vp, _int, _int, _int, _int, _int, _int, _f32, _vp, _sz, _vp]),
    "dxa_dit_bf16_pack_bytes": (_sz, [_int, _int, _int]),
    "dxa_dit_bf16_pack": (_int, [_vp, _int, _int, _int, _vp, _sz, _vp, _vp]),
    "dxa_dit_bf16_pack_per_bytes": (_sz, [_int, _int, _int]),
    "dxa_dit_bf16_pack_per": (_int, [_vp, _int, _int, _int, _vp, _sz, _vp, _vp]),
    "dxa_dit_sample_bf16_per_fwd": (_int, [_vp] * 9 + [_int, _int, _int, _int, _f32, _vp, _vp, _int, _int, _int, _int, _int, _int, _int, _f32, _vp, _sz, _vp]),
    "dxa_dit_sample_bf16_workspace": (_sz, [_int, _int, _int]),
    "dxa_dit_sample_bf16_fwd": (_int, [_vp] * 9 + [_int, _int, _int, _int, _f32, _vp, _int, _int, _int, _int, _int, _int, _f32, _vp, _sz, _vp]),
    "dxa_dit_sample_bf16_batched_workspace": (_sz, [_int, _int, _int, _int]),
    "dxa_dit_sample_bf16_batched_fwd": (_int, [_vp] * 9 + [_int, _int, _int, _int, _int, _f32, _vp, _int, _int, _int, _int, _int, _int, _f32, _vp, _sz, _vp]),
    "dxa_dit_sample_bf16_per_batched_fwd": (_int, [_vp] * 9 + [_int, _int, _int, _int, _int, _f32, _vp, _vp, _int, _int, _int, _int, _int, _int, _int, _f32, _vp, _sz, _vp]),
    "dxa_decode_step_workspace": (_sz, [_int, _int, _int, _int, _int]),
    "dxa_decode_step": (_int, [C.POINTER(DecodeDesc), _vp]),
    "dxa_decode_status": (_int, [_vp, _vp]),
    "dxa_clip_coef": (_int, [_vp, _f32, _vp, _vp, _vp]),
    "dxa_clip_coef_scaled": (_int, [_vp, _f32, _f32, _vp, _vp, _vp]),
    "dxa_scale": (_int, [_vp, _i64, _f32, _vp]),
    "dxa_scale_dev": (_int, [_vp, _i64, _vp, _vp]),
}


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"dexbotic_amd: native library {LIB_PATH} not found. Build it with "
            "`python -m dexbotic_amd.build` (hipcc --offload-arch=gfx950); there is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"dexbotic_amd: symbol {name} missing from {LIB_PATH} (stale build?)") from e
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def last_error() -> str:
    return (lib.dxa_last_error() or b"").decode()


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise DxaError(f"{what}: status {rc}: {last_error()}")
