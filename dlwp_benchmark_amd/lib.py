"""ctypes binding of libdlwp_hip.so (the C ABI declared in include/dlwp_hip.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C dlwp_benchmark_amd/csrc`.
There is NO fallback: if the shared object is missing or a symbol is absent, importing the
compute path raises -- the product never routes around the HIP kernels.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int32, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DLWP_HIP_LIB") or os.path.join(_HERE, "libdlwp_hip.so")   # override: A/B builds of the same ABI

c_float_p = POINTER(c_float)
c_int32_p = POINTER(c_int32)


class FNO2dDesc(ctypes.Structure):
    """mirror of struct dlwp_fno2d_desc (include/dlwp_hip.h)"""
    _fields_ = [
        ("in_channels", c_int32), ("hidden_channels", c_int32), ("lifting_channels", c_int32),
        ("projection_channels", c_int32), ("out_channels", c_int32), ("n_layers", c_int32),
        ("height", c_int32), ("width", c_int32), ("n_rows", c_int32), ("n_cols", c_int32),
        ("rows_in", c_int32_p), ("rows_out", c_int32_p),
        ("fwd_scale", c_float), ("inv_scale", c_float),
        ("lift_w1", c_void_p), ("lift_b1", c_void_p), ("lift_w2", c_void_p), ("lift_b2", c_void_p),
        ("spec_w", POINTER(c_void_p)), ("spec_b", c_void_p), ("skip_w", POINTER(c_void_p)),
        ("proj_w1", c_void_p), ("proj_b1", c_void_p), ("proj_w2", c_void_p), ("proj_b2", c_void_p),
        ("precision_form", c_int32), ("launch_form", c_int32), ("on_timeout", c_int32), ("unchecked", c_int32),
        ("debug_spin_limit", c_int32), ("lift_table", c_int32),
    ]


class WAttnDesc(ctypes.Structure):
    """mirror of struct dlwp_wattn_desc (include/dlwp_hip.h)"""
    _fields_ = [
        ("grid", c_int32 * 3), ("padded", c_int32 * 3), ("pad_lead", c_int32 * 3), ("window", c_int32 * 3),
        ("shift_fwd", c_int32 * 3), ("shift_back", c_int32 * 3), ("use_mask", c_int32),
        ("mask_b1", c_int32 * 3), ("mask_b2", c_int32 * 3), ("bias_mode", c_int32),
        ("heads", c_int32), ("head_dim", c_int32), ("scale", c_float), ("form", c_int32),
    ]


class MgnMlpDesc(ctypes.Structure):
    """mirror of struct dlwp_mgn_mlp_desc (include/dlwp_hip.h)"""
    _fields_ = [
        ("n_linear", c_int32), ("dims", c_int32 * 6), ("wt", c_void_p * 5), ("bias", c_void_p * 5),
        ("ln_gamma", c_void_p), ("ln_beta", c_void_p), ("ln_eps", c_float),
    ]


class GcLinearArgs(ctypes.Structure):
    """mirror of struct dlwp_gc_linear_args (include/dlwp_hip.h)"""
    _fields_ = [
        ("a_mode", c_int32), ("a", c_void_p), ("a_batch_stride", ctypes.c_int64), ("lda", c_int32),
        ("agg_e", c_void_p), ("agg_batch_stride", ctypes.c_int64), ("agg_width", c_int32), ("row_ptr", c_void_p),
        ("agg_mean", c_int32), ("wt", c_void_p), ("bias", c_void_p), ("k", c_int32), ("n", c_int32), ("batch", c_int32),
        ("rows", c_int32), ("src_products", c_void_p), ("src_index", c_void_p), ("src_products_batch_stride", ctypes.c_int64),
        ("ld_src_products", c_int32), ("dst_products", c_void_p), ("dst_index", c_void_p),
        ("dst_products_batch_stride", ctypes.c_int64), ("ld_dst_products", c_int32), ("act", c_int32), ("out", c_void_p),
        ("out_layout", c_int32), ("ldo", c_int32), ("res", c_void_p), ("res_batch_stride", ctypes.c_int64),
        ("a_act", c_int32), ("act_grad_z", c_void_p), ("act_grad", c_int32), ("ld_act_grad_z", c_int32),
    ]


# name -> (restype, argtypes); every symbol include/dlwp_hip.h declares
SIGNATURES = {
    "dlwp_version": (c_int32, []),
    "dlwp_last_error": (c_char_p, []),
    "dlwp_device_count": (c_int32, []),
    "dlwp_fno2d_plan_create": (c_int32, [POINTER(c_void_p), POINTER(FNO2dDesc), c_void_p]),
    "dlwp_fno2d_plan_destroy": (c_int32, [c_void_p]),
    "dlwp_fno2d_workspace_bytes": (c_size_t, [c_void_p, c_int32]),
    "dlwp_fno2d_status": (c_int32, [c_void_p, c_void_p]),
    "dlwp_fno2d_timeouts": (ctypes.c_uint32, [c_void_p]),
    "dlwp_fno2d_range_reruns": (ctypes.c_uint32, [c_void_p]),
    "dlwp_fno2d_lift_table_state": (c_int32, [c_void_p]),
    "dlwp_fno2d_lift_table_build": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                              c_size_t, POINTER(ctypes.c_double), c_int32_p]),
    "dlwp_fno2d_lift_table_eval_host": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, ctypes.c_int64, c_void_p, c_void_p,
                                                  c_void_p]),
    "dlwp_fno2d_forward_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "dlwp_fno2d_rollout_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                         c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dlwp_fno2d_rollout_range_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                               c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p,
                                               c_int32, c_int32]),
    "dlwp_fno2d_rollout_profiled_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                                  c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p,
                                                  POINTER(ctypes.c_double), c_int32_p]),
    "dlwp_spectral_conv2d_plan_create": (c_int32, [POINTER(c_void_p), c_int32, c_int32, c_int32, c_int32,
                                                   c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "dlwp_spectral_conv2d_plan_create_ex": (c_int32, [POINTER(c_void_p), c_int32, c_int32, c_int32, c_int32, c_int32,
                                                      c_int32, c_void_p, c_void_p, c_float, c_float, c_void_p]),
    "dlwp_spectral_conv2d_set_weights_dev": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p]),
    "dlwp_spectral_conv2d_plan_destroy": (c_int32, [c_void_p]),
    "dlwp_spectral_conv2d_workspace_bytes": (c_size_t, [c_void_p, c_int32]),
    "dlwp_spectral_conv2d_wgrad_workspace_bytes": (c_size_t, [c_void_p, c_int32]),
    "dlwp_spectral_conv2d_wgrad_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t,
                                                 c_void_p]),
    "dlwp_window_attn_workspace_bytes": (c_size_t, [POINTER(WAttnDesc), c_int32, c_int32]),
    "dlwp_window_attn_fallbacks": (c_int32, [POINTER(WAttnDesc), c_int32, c_int32, c_void_p, c_void_p, c_int32_p]),
    "dlwp_window_attn_f32": (c_int32, [POINTER(WAttnDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                       c_size_t, c_void_p]),
    "dlwp_window_attn_bf16": (c_int32, [POINTER(WAttnDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                        c_size_t, c_void_p]),
    "dlwp_window_attn_bf16_io": (c_int32, [POINTER(WAttnDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                           c_size_t, c_void_p]),
    "dlwp_window_attn_bwd_workspace_bytes": (c_size_t, [POINTER(WAttnDesc), c_int32]),
    "dlwp_window_attn_bwd_f32": (c_int32, [POINTER(WAttnDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    # hard_thresholding_fraction is a DOUBLE in the three mixing entry points: int(total * fraction) must be the reference's
    "dlwp_afno2d_mix_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                      c_int32, c_int32, c_int32, c_float, ctypes.c_double, c_void_p]),
    "dlwp_afno2d_mix_scaled_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                             c_int32, c_int32, c_int32, c_float, ctypes.c_double, c_float, c_float, c_void_p]),
    "dlwp_afno2d_mix_bwd_f32": (c_int32, [c_void_p] * 11 + [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_float,
                                          ctypes.c_double, c_float, c_float, c_void_p]),
    "dlwp_fft2_plan_create": (c_int32, [ctypes.POINTER(c_void_p), c_int32, c_int32, c_int32]),
    "dlwp_fft2_plan_destroy": (c_int32, [c_void_p]),
    "dlwp_rfft2_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "dlwp_irfft2_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "dlwp_afno_fft_supported": (c_int32, [c_int32, c_int32, c_int32]),
    "dlwp_afno_fft_plan_create": (c_int32, [ctypes.POINTER(c_void_p), c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_afno_fft_plan_destroy": (c_int32, [c_void_p]),
    "dlwp_afno_rfft2_kept_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "dlwp_afno_irfft2_kept_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "dlwp_conv3x3_cyl_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                       c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_conv3x3_ex_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                      c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "dlwp_conv3x3_mfma_packed_bytes": (c_size_t, [c_int32, c_int32]),
    "dlwp_conv3x3_mfma_variant": (c_int32, [c_int32, c_int32, c_int32, c_int32]),
    "dlwp_conv3x3_mfma_pack_f32": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "dlwp_conv3x3_mfma_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                        c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "dlwp_conv2d_mfma_packed_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "dlwp_conv2d_mfma_variant": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "dlwp_conv2d_mfma_pack_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "dlwp_conv2d_mfma_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                       c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_conv_transpose2d_mfma_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                                 c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_conv2d_mfma_pack_ex_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "dlwp_conv2d_dgrad_mfma_variant": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "dlwp_conv2d_dgrad_mfma_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                             c_int32, c_int32, c_void_p]),
    "dlwp_linear_packed_bytes": (c_size_t, [c_int32, c_int32]),
    "dlwp_linear_pack_f32": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "dlwp_linear_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32,
                                  c_void_p]),
    "dlwp_linear_bf16": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32,
                                   c_void_p]),
    "dlwp_linear_bf16_io": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32,
                                      c_int32, c_int32, c_void_p]),
    "dlwp_linear_pack_f16x3": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "dlwp_linear_f16x3": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32,
                                    c_void_p]),
    "dlwp_groupnorm_act_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float,
                                         c_int32, c_void_p]),
    "dlwp_groupnorm_act_fwd_stats_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                                   c_int32, c_float, c_int32, c_void_p]),
    "dlwp_groupnorm_act_bwd_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "dlwp_groupnorm_act_bwd_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_layernorm_bwd_partials": (c_int32, [ctypes.c_int64, c_int32]),
    "dlwp_layernorm_bwd_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int32]),
    "dlwp_layernorm_bwd_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                         ctypes.c_int64, c_int32, c_float, c_void_p]),
    "dlwp_act_f32": (c_int32, [c_void_p, c_void_p, ctypes.c_int64, c_int32, c_void_p]),
    "dlwp_bias_act_bwd_workspace_bytes": (c_size_t, [ctypes.c_int64, c_int32]),
    "dlwp_bias_act_bwd_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, ctypes.c_int64, c_int32,
                                        c_int32, c_void_p]),
    "dlwp_conv2d_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                  c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_conv_transpose2d_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                            c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_avgpool2x2_f32": (c_int32, [c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_void_p]),
    "dlwp_avgpool2x2_bwd_f32": (c_int32, [c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_void_p]),
    "dlwp_conv3x3_hpx_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                       c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "dlwp_healpix_pad_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_healpix_pad_bwd_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                           c_int32, c_void_p]),
    "dlwp_conv3x3_hpx_bwd_data_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "dlwp_conv3x3_hpx_bwd_data_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dlwp_healpix_to_latlon_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_void_p]),
    "dlwp_conv3x3_wgrad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "dlwp_conv3x3_wgrad_slices": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "dlwp_conv3x3_wgrad_f32": (c_int32, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                         c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dlwp_conv2d_wgrad_workspace_bytes": (c_size_t, [c_int32] * 9),
    "dlwp_conv2d_wgrad_slices": (c_int32, [c_int32] * 9),
    "dlwp_conv2d_wgrad_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int32] * 10 + [c_void_p, c_size_t, c_void_p]),
    "dlwp_convlstm_gates_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                          c_void_p]),
    "dlwp_convlstm_gates_bwd_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                              c_int32, c_int32, c_void_p]),
    "dlwp_layernorm_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_float, c_void_p]),
    "dlwp_layernorm_prebias_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_float,
                                             c_void_p]),
    "dlwp_layernorm_prebias_bf16out": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_float,
                                                 c_void_p]),
    "dlwp_layernorm_nhwc_to_nchw_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_int64, c_int32,
                                                  c_float, c_void_p]),
    "dlwp_afno_merge_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                      ctypes.c_int64, c_int32, c_float, c_void_p]),
    "dlwp_patch_embed_1x1_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, ctypes.c_int64,
                                           c_int32, c_void_p]),
    "dlwp_concat_channels_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, ctypes.c_int64, c_void_p]),
    "dlwp_patch_recover_1x1_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_int64, c_int32, c_int32, c_void_p]),
    "dlwp_token_mlp_packed_bytes": (c_size_t, [c_int32, c_int32]),
    "dlwp_token_mlp_pack_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                          c_void_p]),
    "dlwp_afno_block_tail_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_int64,
                                           c_int32, c_int32, c_float, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "dlwp_token_mlp_pack_f16x3": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                            c_void_p]),
    "dlwp_afno_block_tail_f16x3": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_int64,
                                             c_int32, c_int32, c_float, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "dlwp_token_mlp_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32,
                                     c_int32, c_float, c_void_p]),
    "dlwp_token_mlp_emit_norm_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64,
                                               c_int32, c_int32, c_float, c_void_p, c_void_p, c_float, c_void_p,
                                               ctypes.c_int64, c_void_p]),
    "dlwp_weighted_error_sums_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                               c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_weighted_error_sums_acc_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                                   c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_zonal_power_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "dlwp_zonal_power_sums_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                            c_int32, c_void_p, c_size_t, c_void_p]),
    "dlwp_zonal_power_sums_acc_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                                c_int32, c_void_p, c_size_t, c_void_p]),
    "dlwp_climate_sums_acc_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                            c_int32, c_int32, c_void_p]),
    "dlwp_ensemble_sums_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "dlwp_ensemble_sums_acc_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_int64,
                                             c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_size_t,
                                             c_void_p]),
    "dlwp_insolation_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, ctypes.c_int64, ctypes.c_double, c_int32, c_int32,
                                      c_float, c_float, c_void_p]),
    "dlwp_spectral_conv2d_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "dlwp_global_attn_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "dlwp_global_attn_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_void_p, c_size_t,
                                       c_void_p]),
    "dlwp_global_attn_bwd_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "dlwp_global_attn_bwd_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float,
                                           c_void_p, c_size_t, c_void_p]),
    "dlwp_mgn_mlp_f32": (c_int32, [POINTER(MgnMlpDesc), c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_gc_linear_f32": (c_int32, [POINTER(GcLinearArgs), c_void_p]),
    "dlwp_gc_layernorm_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p,
                                        ctypes.c_int64, c_void_p]),
    "dlwp_gc_weight_grad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "dlwp_gc_weight_grad_f32": (c_int32, [POINTER(GcLinearArgs), c_void_p, c_int32, c_int32, c_void_p, c_int32, c_void_p,
                                          c_void_p, c_size_t, c_void_p]),
    "dlwp_gc_layernorm_bwd_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "dlwp_gc_layernorm_bwd_f32": (c_int32, [c_void_p, c_void_p, c_float, c_void_p, c_void_p, ctypes.c_int64, c_void_p,
                                            c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_size_t, c_void_p]),
    "dlwp_gc_segment_sum_f32": (c_int32, [c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                          c_void_p, c_void_p]),
    "dlwp_mgn_processor_layer_f32": (c_int32, [POINTER(MgnMlpDesc), POINTER(MgnMlpDesc), c_int32, c_void_p, c_void_p, c_void_p,
                                               c_int32,
                                               c_int32, c_int32, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_void_p,
                                               c_void_p]),
    "dlwp_mgn_mlp_bwd_workspace_bytes": (c_size_t, [POINTER(MgnMlpDesc), c_int32, c_int32]),
    "dlwp_mgn_mlp_bwd_f32": (c_int32, [POINTER(MgnMlpDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                       c_int32, c_void_p, c_size_t, c_void_p]),
    "dlwp_mgn_processor_layer_bwd_workspace_bytes": (c_size_t, [POINTER(MgnMlpDesc), POINTER(MgnMlpDesc), c_int32, c_int32,
                                                                c_int32, c_int32]),
    "dlwp_mgn_processor_layer_bwd_f32": (c_int32, [POINTER(MgnMlpDesc), POINTER(MgnMlpDesc), c_int32, c_void_p, c_void_p,
                                                   c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                                   ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                   c_void_p, c_size_t, c_void_p]),
    "dlwp_mt_chunk_elems": (c_int32, []),
    "dlwp_mse_loss_partials": (c_int32, [ctypes.c_int64]),
    "dlwp_mse_loss_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, ctypes.c_int64,
                                    ctypes.c_int64, c_void_p]),
    "dlwp_mse_loss_scale_grad_f32": (c_int32, [c_void_p, c_void_p, c_int32, ctypes.c_int64, c_void_p]),
    "dlwp_mt_grad_norm_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_float, c_void_p, c_void_p]),
    "dlwp_mt_scale_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "dlwp_mt_zero_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "dlwp_mt_adamw_f32": (c_int32, [c_void_p] * 8 + [c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "dlwp_mt_ema_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_float, c_float,
                                  c_void_p]),
    "dlwp_refiner_grid_span": (ctypes.c_int64, []),
    "dlwp_philox_normal_f32": (c_int32, [c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_void_p]),
    "dlwp_ddpm_step_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, POINTER(ctypes.c_double),
                                     ctypes.c_int64, ctypes.c_int64, c_void_p]),
    "dlwp_refiner_pair_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, c_float, c_float, ctypes.c_int64,
                                        ctypes.c_int64, c_void_p]),
    "dlwp_philox_normal_members_f32": (c_int32, [c_void_p, ctypes.c_int64, c_int32, c_int32, ctypes.c_int64, ctypes.c_int64,
                                                 c_void_p]),
    "dlwp_ddpm_step_members_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32,
                                             POINTER(ctypes.c_double), ctypes.c_int64, ctypes.c_int64, c_void_p]),
    "dlwp_dataset_grid_blocks": (c_int32, []),
    "dlwp_dataset_gather_f32": (c_int32, [c_void_p, ctypes.c_int64, c_int32, ctypes.c_int64, c_void_p, c_void_p, c_int32, c_int32,
                                          c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                          c_float, ctypes.c_int64, ctypes.c_int64, c_void_p]),
    "dlwp_dataset_stats_workspace_bytes": (c_size_t, [c_int32]),
    "dlwp_dataset_stats_f64": (c_int32, [c_void_p, ctypes.c_int64, c_int32, ctypes.c_int64, c_void_p, ctypes.c_int64, c_void_p,
                                         c_void_p, c_size_t, c_void_p]),
    "dlwp_dataset_group_mean_f32": (c_int32, [c_void_p, ctypes.c_int64, c_int32, ctypes.c_int64, c_void_p, c_void_p,
                                              ctypes.c_int64, c_int32, c_void_p, c_void_p]),
    "dlwp_coarsen_mean_f32": (c_int32, [c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32, c_void_p]),
    # spherical harmonic transforms + Driscoll-Healy channel mix (csrc/sht.hip)
    "dlwp_sht_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_isht_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_sph_mix_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_sph_mix_packed_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_sph_mix_pack_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    # their backwards
    "dlwp_sht_bwd_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_isht_bwd_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_sph_mix_dgrad_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_sph_mix_pack_adjoint_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_sph_mix_wgrad_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_sph_mix_wgrad_packed_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    "dlwp_sph_mix_unpack_f32": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    # spherical power spectra of a rollout and its targets (csrc/sph_power.hip)
    "dlwp_sph_power_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "dlwp_sph_power_sums_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                          c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    "dlwp_sph_power_sums_acc_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                              c_int32, c_int32, c_int32, c_void_p, c_size_t, c_void_p]),
    # 2-D Navier-Stokes trajectories from one LDS-resident workgroup each (csrc/navier_stokes.hip)
    "dlwp_ns2d_rollout_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                        ctypes.c_double, ctypes.c_double, c_void_p]),
}

_lib = None


ERR_UNSUPPORTED = -2      # DLWP_ERR_UNSUPPORTED (include/dlwp_hip.h): the shape lies outside the kernel's envelope


class DlwpError(RuntimeError):
    """`status`: the library's status where check() raised the error, None where Python code did."""

    def __init__(self, *args, status=None):
        super().__init__(*args)
        self.status = status


def load():
    """Loads libdlwp_hip.so and types every entry point.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DlwpError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C dlwp_benchmark_amd/csrc`.  There is no CPU fallback for the HIP path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise DlwpError(f"libdlwp_hip.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().dlwp_last_error().decode(errors="replace")
        raise DlwpError(f"{what or 'libdlwp_hip'} failed with status {rc}: {msg}", status=int(rc))


def require_cuda_tensor(t, name: str):
    import torch

    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DlwpError(
            f"{name} must be a tensor on an MI355X device (got {'cpu tensor' if isinstance(t, torch.Tensor) else type(t)}); "
            "the HIP path has no CPU fallback -- the CPU restatement lives in oracle/ and is test-only")
    if t.dtype != torch.float32:
        raise DlwpError(f"{name} must be float32 (got {t.dtype})")


def require_running_sums(into, shape, device):
    """`into`: the running sums an `*_acc` entry point adds to, a contiguous double tensor of `shape` on `device`."""
    import torch

    if (not isinstance(into, torch.Tensor) or not into.is_cuda or tuple(into.shape) != tuple(shape) or into.dtype != torch.float64
            or not into.is_contiguous() or into.device != device):
        raise DlwpError(f"running sums must be a contiguous double {list(shape)} tensor on the MI355X device {device}")


def stream_ptr():
    import torch

    return c_void_p(torch.cuda.current_stream().cuda_stream)


_CTYPES_VALUE = (ctypes._SimpleCData, ctypes.Array, ctypes._Pointer, type(ctypes.byref(ctypes.c_int())))


def marshal(args):
    """The C arguments of a call from its Python ones: a tensor gives its data_ptr(), None stays None (a null pointer), a
    ctypes.Structure goes by reference, numbers and ctypes values stay as they are.  Layout is the caller's business: nothing
    here makes a tensor contiguous or checks that it is (some callers pass strided blocks with their leading dimension)."""
    import torch

    Tensor, Parameter = torch.Tensor, torch.nn.Parameter
    out = []
    for a in args:
        t = type(a)
        if t is int or a is None or t is float or t is bool:           # exact types first: this loop runs at every launch
            out.append(a)
        elif t is Tensor or t is Parameter or isinstance(a, Tensor):
            out.append(a.data_ptr())
        elif isinstance(a, ctypes.Structure):
            out.append(ctypes.byref(a))
        elif isinstance(a, (int, float)) or isinstance(a, _CTYPES_VALUE):
            out.append(a)
        else:
            raise DlwpError(f"argument {len(out)} of a library call is a {type(a).__name__}: "
                            "a tensor, None, a ctypes structure or value, or a number is needed")
    return out


def workspace(nbytes: int, device):
    """A uint8 workspace tensor of `nbytes` on `device` from torch's caching allocator, or None for 0 bytes (a null workspace
    means something to several entry points; a wrapper that needs a floor asks for max(n, FLOOR))."""
    import torch

    return torch.empty(int(nbytes), dtype=torch.uint8, device=device) if nbytes else None


def kept_workspace(bufs: dict, nbytes: int, device, floor: int = 8):
    """The kernel workspace an owner keeps per device, shared by every shape it runs: `bufs` is the owner's dictionary
    str(device) -> uint8 tensors, the last one the largest and the one in use.  Returns that one if it holds max(nbytes, floor)
    bytes; otherwise appends one of that size, or twice the last one's if that is more, and returns it.  The replaced ones
    stay allocated because a recorded step (sharding.CapturedStep) replays against the address it was recorded with: freed,
    the caching allocator may hand the block to another tensor under a recording that still writes to it.  With the doubling
    the replaced ones add up to less than the one in use, and an owner that sees one size allocates exactly that size."""
    import torch

    nbytes = max(int(nbytes), int(floor))
    kept = bufs.setdefault(str(device), [])
    if not kept or kept[-1].numel() < nbytes:
        kept.append(torch.empty(max(nbytes, 2 * kept[-1].numel()) if kept else nbytes, dtype=torch.uint8, device=device))
    return kept[-1]


def launch(name: str, device, *args, accept=()):
    """The one way Python reaches an entry point whose last parameter is the stream: calls `name` with marshal(args) and
    the current stream of `device`, with `device` current (the guard is entered only when it is not).  Returns the status;
    one that is neither 0 nor in `accept` raises DlwpError labelled with `name`.  The entry point is looked up on the library
    object at every call, which is where KernelTimer puts its wrappers."""
    import torch

    fn = getattr(load(), name)
    argv = marshal(args)
    if getattr(device, "index", None) == torch.cuda.current_device():      # the usual case: no guard to pay for
        rc = fn(*argv, torch.cuda.current_stream().cuda_stream)
    else:
        with torch.cuda.device(device):
            rc = fn(*argv, torch.cuda.current_stream().cuda_stream)
    if rc != 0 and rc not in accept:
        check(rc, name)
    return rc


class KernelTimer:
    """Measurement aid (bench.py): brackets every call of the chosen C-ABI entry points with HIP events on the stream
    the call launches on (torch's current stream = the `stream` argument every wrapper passes) and sums the elapsed
    time per (entry point, tag).  `tagger(name, args) -> hashable` separates calls of one entry point by shape.
    An EMPTY bracket is recorded beside every call; half of its mean (one marker latency) is subtracted per call,
    which reproduces rocprofv3 --kernel-trace averages within a few per cent (bench.py).
    The product path never uses this class."""

    def __init__(self, names=None, tagger=None):
        self.names = names
        self.tagger = tagger
        self.records = []
        self._empty = []
        self._saved = {}

    def __enter__(self):
        import torch

        lib = load()
        names = self.names or [n for n in SIGNATURES if n.endswith(("_f32", "_bf16", "_f16x3", "_bf16_io", "_bf16out"))]
        for name in names:
            fn = getattr(lib, name)
            self._saved[name] = fn

            def wrapped(*a, _fn=fn, _name=name):
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                rc = _fn(*a)
                e1.record()
                e2.record()
                self.records.append((_name, self.tagger(_name, a) if self.tagger else None, e0, e1))
                self._empty.append((e1, e2))
                return rc

            setattr(lib, name, wrapped)
        return self

    def __exit__(self, *exc):
        lib = load()
        for name, fn in self._saved.items():
            setattr(lib, name, fn)
        self._saved = {}
        return False

    def summary(self):
        """{(name, tag): {"calls": n, "total_ms": t, "avg_ms": t / n}} after a device synchronisation."""
        import torch

        torch.cuda.synchronize()
        marker = 0.0
        if self._empty:
            marker = 0.5 * sum(a.elapsed_time(b) for a, b in self._empty) / len(self._empty)
        out = {}
        for name, tag, e0, e1 in self.records:
            d = out.setdefault((name, tag), {"calls": 0, "total_ms": 0.0})
            d["calls"] += 1
            d["total_ms"] += max(e0.elapsed_time(e1) - marker, 0.0)
        for d in out.values():
            d["avg_ms"] = d["total_ms"] / d["calls"]
        return out, marker
