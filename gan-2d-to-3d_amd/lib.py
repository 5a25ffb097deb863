"""ctypes binding of libg2s.so (include/g2s.h).  No fallback: if the library is missing or a call
fails, this raises — the product has no CPU path."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libg2s.so")

G2S_F32, G2S_F16 = 0, 1
CONV_PLAIN, CONV_UP2, CONV_DOWN2 = 0, 1, 2

_lib = None

# name: (restype, argtypes) — exactly the declarations of include/g2s.h
_p, _i, _f, _sz, _i64, _d = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64, C.c_double
SIGNATURES = {
    "g2s_abi_version": (_i, []),
    "g2s_last_error": (C.c_char_p, []),
    "g2s_clamp": (_i, [_p, _p, _p, _i64, _f, _f, _i, _p]),
    "g2s_avg_pyramid": (_i, [_p, _p, _i, _i64, _i, _i, _p]),
    "g2s_res_split_fwd": (_i, [_p, _p, _p, _i64, _i, _i, _p]),
    "g2s_res_split_bwd": (_i, [_p, _p, _p, _p, _i64, _i, _i, _p]),
    "g2s_depth_head_fwd": (_i, [_p, _p, _p, _i64, _i, _f, _f, _i, _f, _p]),
    "g2s_depth_head_bwd": (_i, [_p, _p, _p, _p, _p, _i64, _i, _f, _f, _i, _f, _i, _p]),
    "g2s_grid_sample_fwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _p]),
    "g2s_grid_sample_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "g2s_grid_sample_bwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _p, _sz, _i, _p]),
    "g2s_set_deterministic": (_i, [_i]),
    "g2s_get_deterministic": (_i, []),
    "g2s_raster_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "g2s_raster_tune": (_i, [_i]),
    "g2s_raster_get_tune": (_i, []),
    "g2s_raster_depth_fwd": (_i, [_p, _p, _i, _i, _i, _i, _p, _f, _i, _i, _f, _f, _p, _p, _p, _p, _sz, _p]),
    "g2s_raster_depth_bwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _f, _i, _p, _p]),
    "g2s_raster_bwd_workspace_bytes": (_sz, [_i, _i]),
    "g2s_raster_depth_bwd_ex": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _f, _i, _p, _p, _sz, _i, _p]),
    "g2s_raster_rgb_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p, _f, _p, _p]),
    "g2s_raster_rgb_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "g2s_raster_rgb_bwd": (_i, [_p] * 6 + [_i, _i, _i, _i, _p, _f, _i, _i, _i, _f, _p, _p, _p, _sz, _i, _p]),
    "g2s_face_light_fwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p]),
    "g2s_face_light_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _sz, _i, _p]),
    "g2s_raster_rgba_fwd": (_i, [_p] * 6 + [_i, _i, _i, _i, _i, _i, _i, _i, _p, _f, _p, _p, _p]),
    "g2s_raster_rgba_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "g2s_raster_rgba_bwd": (_i, [_p] * 7 + [_i, _i, _i, _i, _p, _f, _i, _i, _i, _i, _f, _p, _p, _p, _p, _sz, _i, _p]),
    "g2s_sweep_verts": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "g2s_sweep_shade": (_i, [_p] * 8 + [_i] * 9 + [_p, _f, _p, _p, _p]),
    "g2s_sweep_pseudo": (_i, [_p] * 8 + [_f, _f, _i, _i, _i, _i, _p, _p, _p]),
    "g2s_mapping_tile": (_i, []),
    "g2s_mapping_fwd": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _f, _f, _f, _p]),
    "g2s_rows_mean": (_i, [_p, _p, _i64, _i, _i64, _p]),
    "g2s_image_to_u8": (_i, [_p, _p, _i64, _i, _i, _p]),
    "g2s_fused_bias_act": (_i, [_p, _p, _p, _p, _i64, _i64, _i64, _i, _i, _f, _f, _i, _p]),
    "g2s_maxpool2x2_fwd": (_i, [_p, _p, _i64, _i, _i, _p]),
    "g2s_maxpool2x2_bwd": (_i, [_p, _p, _p, _i64, _i, _i, _p]),
    "g2s_add_bias_scale": (_i, [_p, _p, _p, _p, _i64, _i64, _i, _f, _p]),
    "g2s_noise_bias_act": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _p]),
    "g2s_noise_bias_act_ps": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _f, _f, _p]),
    "g2s_upfirdn2d": (_i, [_p, _p, _p] + [_i] * 14 + [_p]),
    "g2s_modconv": (_i, [_p] * 8 + [_i] * 9 + [_f, _f, _i, _p]),
    "g2s_modconv_needs_zero": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "g2s_upfirdn2d_nba": (_i, [_p, _p, _p] + [_i] * 12 + [_p, _p, _p, _f, _f, _p]),
    "g2s_synth_bwd_rows": (_i, [_p] * 13 + [_i, _i, _i, _f, _f, _p]),
    "g2s_upfirdn2d_nba_ps": (_i, [_p, _p, _p] + [_i] * 12 + [_p, _p, _p, _f, _f, _p]),
    "g2s_synth_bwd_rows_ps": (_i, [_p] * 13 + [_i, _i, _i, _f, _f, _p]),
    "g2s_channel_sum": (_i, [_p, _p, _i, _i, _i, _p]),
    "g2s_noise_grad": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "g2s_noise_regularize_workspace_bytes": (_sz, [_p, _i, _i]),
    "g2s_noise_regularize": (_i, [_p, _p, _p, _i, _i, _p, _p, _sz, _p]),
    "g2s_noise_normalize_workspace_bytes": (_sz, [_p, _i, _i]),
    "g2s_noise_normalize": (_i, [_p, _p, _i, _i, _p, _sz, _p]),
    "g2s_demod_fwd_multi": (_i, [_p, _p, _p, _p, _p, _i, _i, _f, _p]),
    "g2s_demod_bwd_multi": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _p]),
    "g2s_modconv_f16": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _p]),
    "g2s_modconv_tune": (_i, [_i, _i]),
    "g2s_mfma_probe": (_i, [_p, _i, _i, _i, _p]),
    "g2s_mfma_lds_probe": (_i, [_p, _i, _i, _i, _i, _p]),
    "g2s_wino_weights_floats": (_sz, [_i, _i]),
    "g2s_wino4_weights_floats": (_sz, [_i, _i]),
    "g2s_wino4_weights": (_i, [_p, _p, _i, _i, _i, _p]),
    "g2s_wino4_supported": (_i, [_i] * 5),
    "g2s_conv3x3_wino4": (_i, [_p] * 8 + [_i] * 6 + [_f, _f, _i, _p, _i64, _p]),
    "g2s_wino_weights": (_i, [_p, _p, _i, _i, _i, _p]),
    "g2s_conv3x3_wino": (_i, [_p] * 8 + [_i] * 6 + [_f, _f, _i, _p, _i64, _p]),
    "g2s_conv2d": (_i, [_p, _p, _p, _p] + [_i] * 12 + [_i, _f, _f, _i, _i, _p]),
    "g2s_conv2d_wgrad": (_i, [_p, _p, _p] + [_i] * 10 + [_i, _i, _p]),
    "g2s_conv2d_bwd": (_i, [_p, _p, _p] + [_i] * 13 + [_p, _p, _p] + [_i] * 8 + [_p]),
    "g2s_adam_chunk": (_i64, []),
    "g2s_adam_step": (_i, [_p, _p, _p, _i, _i, _f, _f, _f, _f, _f, _p]),
    "g2s_rows_dot_scale": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _p]),
    "g2s_demod_fwd": (_i, [_p, _p, _p, _i, _i, _i, _f, _p]),
    "g2s_demod_bwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_demod_bwd_add": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_lpips_layer_fwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_lpips_layer_bwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_lpips_layer_bwd_ex": (_i, [_p, _p, _p, _p, _p, _i, _p, _i, _i, _i, _p]),
    "g2s_weighted_l1_fwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_weighted_l1_bwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_weighted_l1_fwd2": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_weighted_l1_bwd3": (_i, [_p] * 7 + [_f, _p, _p, _f, _f, _p, _i, _i, _i, _p]),
    "g2s_weighted_l1_bwd2": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_view_transform_fwd": (_i, [_p, _f, _f, _f, _p, _p, _i, _p]),
    "g2s_view_transform_bwd": (_i, [_p, _f, _f, _f, _p, _p, _p, _i, _p]),
    "g2s_warp_verts_fwd": (_i, [_p, _p, _p, _p, _f, _p, _i, _i, _p]),
    "g2s_warp_verts_bwd": (_i, [_p, _p, _p, _p, _f, _p, _p, _i, _i, _i, _p]),
    "g2s_inv_warp_grid_fwd": (_i, [_p, _p, _p, _p, _p, _f, _p, _i, _i, _i, _p]),
    "g2s_inv_warp_grid_bwd": (_i, [_p, _p, _p, _p, _p, _f, _p, _p, _p, _i, _i, _i, _i, _p]),
    "g2s_normal_fwd": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "g2s_normal_bwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_shading_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "g2s_shading_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_smooth_loss_fwd": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "g2s_smooth_loss_bwd": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "g2s_groupnorm_workspace_floats": (_sz, [_i, _i, _i, _i]),
    "g2s_groupnorm_act_fwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _f, _i, _f, _p]),
    "g2s_groupnorm_act_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p]),
    "g2s_prior_map": (_i, [_p, _i, _i, _i, _d, _d, _p, _p]),
    "g2s_prior_smooth_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "g2s_prior_smooth": (_i, [_p, _i, _i, _i, _i, _d, _d, _p, _p, _sz, _p]),
    "g2s_prior_ellipsoid_workspace_bytes": (_sz, [_i]),
    "g2s_prior_ellipsoid": (_i, [_p, _i, _i, _d, _d, _d, _d, _p, _p, _sz, _p]),
    "g2s_conv_stem7": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_maxpool3x3s2": (_i, [_p, _p, _i, _i, _i, _p]),
    "g2s_adaptive_avgpool": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_resize_bilinear": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "g2s_gate_add_act": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_parse_head_workspace_bytes": (_sz, [_i]),
    "g2s_parse_head": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, C.c_uint32, _p, _p, _p, _p, _sz, _p]),
    "g2s_depth_metrics_workspace_bytes": (_sz, [_i, _i, _i]),
    "g2s_depth_metrics": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _sz, _p]),
    "g2s_image_metrics_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "g2s_image_metrics": (_i, [_p, _p, _p, _i, _i, _i, _i, _f, _p, _p, _sz, _p]),
    "g2s_ada_up2": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "g2s_ada_up2_bwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "g2s_ada_warp_down": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "g2s_ada_warp_down_bwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "g2s_ada_warp_down_bwd_gather": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "g2s_mbstd_fwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_mbstd_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_mbstd_bwd2": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_d_logistic": (_i, [_p, _p, _p, _p, _p, _i, _i, _p]),
    "g2s_r1_penalty_chunks": (_i64, [_i64]),
    "g2s_r1_penalty": (_i, [_p, _p, _p, _p, _i, _i64, _p]),
    "g2s_modconv_wgrad": (_i, [_p, _p, _p, _p, _p] + [_i] * 10 + [_i, _p]),
    "g2s_path_penalty": (_i, [_p, _p, _f, _p, _p, _p, _i, _i, _i, _p]),
    "g2s_g_nonsaturating": (_i, [_p, _p, _p, _i, _p]),
    "g2s_ema_chunk": (_i64, []),
    "g2s_ema_accumulate": (_i, [_p, _p, _i, _i, _f, _f, _p]),
    "g2s_u8_batch": (_i, [_p, _i64, _p, _p, _p, _i, _i, _p]),
    "g2s_resize_u8": (_i, [_p, _p, _p] + [_i] * 5 + [_p, _p, _i, _p, _p, _i] + [_i] * 6 + [_p]),
    "g2s_mirror_pair_fwd": (_i, [_p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_mirror_pair_bwd": (_i, [_p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p]),
    "g2s_canon_mask": (_i, [_p, _p, _p, _p, _p, _f, _p, _p, _i, _i, _i, _i, _p]),
    "g2s_resample_max_taps": (_i, []),
    "g2s_resample_tile_rows": (_i, [_i] * 6),
    "g2s_resample_bands_check": (_i, [_p, _p, _i, _i, _i]),
    "g2s_resample_sep": (_i, [_p, _p] + [_i] * 5 + [_p, _p, _p, _i, _p, _p, _p, _i, _p]),
    "g2s_bank_gather": (_i, [_p, _p, _i64, _p, _i, _i, _p, _i, _p, _p, _i, _p, _p]),
    "g2s_mvn_fit": (_i, [_p, _i64, _i, _i64, _p, _i, _d, _p, _p, _p, _p, _p]),
    "g2s_image_grid_u8": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _f, _p]),
    "g2s_ppl_latents": (_i, [_p, _p, _f, _i, _p, _i, _i, _p]),
}


class G2SError(RuntimeError):
    pass


def load():
    """Load libg2s.so; raises if it has not been built (python gan-2d-to-3d_amd/build.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise G2SError(f"{LIB_PATH} not found: build it with `python gan-2d-to-3d_amd/build.py` "
                           "(no CPU fallback exists)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the ABI lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if lib.g2s_abi_version() != 1:
            raise G2SError(f"libg2s ABI version {lib.g2s_abi_version()} != 1")
        _lib = lib
    return _lib


def set_deterministic(on=True):
    """g2s_set_deterministic (include/g2s.h): reproducible launch partitions for the whole process —
    bit-identical network forwards from run to run, at the cost of the split-K speedups.  Returns
    the previous setting."""
    L = load()
    prev = bool(L.g2s_get_deterministic())
    check(L.g2s_set_deterministic(int(bool(on))))
    return prev


def check(rc):
    if rc != 0:
        raise G2SError(f"libg2s error {rc}: {load().g2s_last_error().decode()}")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Scratch of the split-K Winograd launches (include/g2s.h, `ws`): one buffer per (device, stream) —
# launches on one stream are ordered, so they can share it.  64 MB hold 8 slices of the largest output
# such a launch writes in the workload (9 x 512 x 16 x 16 floats).
SPLIT_WS_FLOATS = 16 * 1024 * 1024
_split_ws = {}


def split_ws():
    """(pointer, floats) of the current stream's split workspace, allocated on first use."""
    st = torch.cuda.current_stream()
    key = (st.device_index, st.cuda_stream)
    t = _split_ws.get(key)
    if t is None:
        t = _split_ws[key] = torch.empty(SPLIT_WS_FLOATS, dtype=torch.float32,
                                         device=torch.device("cuda", st.device_index))
    return C.c_void_p(t.data_ptr()), t.numel()


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libg2s kernels need CUDA (ROCm) tensors; there is no CPU fallback")
