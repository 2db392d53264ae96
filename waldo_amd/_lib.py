"""ctypes binding of the C-ABI HIP library (include/waldo_hip.h).

The product path has NO CPU fallback: if ``libwaldo_hip.so`` is missing or fails to load, every
op raises.  ``torch`` is imported before the library is opened so that the HIP runtime the
library binds to (SONAME libamdhip64.so.7) is the one PyTorch-ROCm already loaded -- device
pointers and streams are then shared between the two.
"""
import ctypes
import os
import threading

import torch  # noqa: F401  (must precede CDLL: see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libwaldo_hip.so")
# ABI this binding was written against (include/waldo_hip.h: waldo_version() = major * 1000 + minor); a
# library of another version has other prototypes behind the same names and is refused by load()
ABI_VERSION = 1020

_c_f = ctypes.c_void_p  # device pointers travel as integers
_i64 = ctypes.c_int64
_int = ctypes.c_int
_flt = ctypes.c_float
_u32 = ctypes.c_uint32
_stream = ctypes.c_void_p

# name -> argtypes; mirrors include/waldo_hip.h one to one (tests check the header against this)
SIGNATURES = {
    "waldo_tps_mapping_fwd": [_c_f, _c_f, _c_f, _i64, _int, _stream],
    "waldo_tps_mapping_bwd": [_c_f, _c_f, _c_f, _i64, _int, _stream],
    "waldo_tps_grid_fwd": [_c_f, _c_f, _c_f, _i64, _i64, _int, _stream],
    "waldo_tps_grid_bwd": [_c_f, _c_f, _c_f, _i64, _i64, _int, _stream],
    "waldo_inverse_warp_fwd": [_c_f] * 14 + [_i64, _int, _int, _int, _int, _int, _int, _int, _stream],
    "waldo_inverse_warp_order_fwd": [_c_f] * 16 + [_i64, _int, _int, _int, _int, _int, _int, _int, _stream],
    "waldo_inverse_warp_bwd": [_c_f] * 9 + [_i64, _int, _int, _int, _int, _int, _int, _stream],
    "waldo_grid_sample2d_fwd": [_c_f, _c_f, _c_f, _i64, _int, _int, _int, _int, _int, _flt, _i64,
                                _i64, _i64, _i64, _stream],
    "waldo_grid_sample2d_ex_fwd": [_c_f, _c_f, _c_f, _c_f, _i64, _int, _int, _int, _int, _int, _flt, _i64,
                                   _i64, _i64, _i64, _i64, _i64, _i64, _flt, _flt, _stream],
    "waldo_grid_sample2d_bwd": [_c_f, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, _int, _int, _int,
                                _flt, _i64, _i64, _stream],
    "waldo_grid_sample2d_ex_bwd": [_c_f, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, _int, _int, _int,
                                   _flt, _i64, _i64, _i64, _i64, _i64, _flt, _flt, _stream],
    "waldo_occ_composite_fwd": [_c_f, _c_f, _c_f, _i64, _int, _i64, _i64, _stream],
    "waldo_occ_composite_bwd": [_c_f, _c_f, _c_f, _c_f, _c_f, _i64, _int, _i64, _i64, _stream],
    "waldo_compute_occ_fwd": [_c_f, _c_f, _i64, _int, _flt, _stream],
    "waldo_compute_occ_bwd": [_c_f, _c_f, _c_f, _i64, _int, _flt, _stream],
    "waldo_alpha_head_fwd": [_c_f] * 4 + [_i64, _int, _int, _int, _int, _flt, _int, _int, _stream],
    "waldo_alpha_head_bwd": [_c_f] * 5 + [_i64, _int, _int, _int, _int, _flt, _int, _int, _stream],
    "waldo_pose_affine_fwd": [_c_f] * 5 + [_i64, _int, _flt, _flt, _stream],
    "waldo_pose_affine_bwd": [_c_f] * 6 + [_i64, _int, _flt, _flt, _stream],
    "waldo_disocc_test_fwd": [_c_f, _c_f, _i64, _int, _int, _i64, _stream],
    "waldo_flow_ctx_alpha_fwd": [_c_f] * 7 + [_int] * 10 + [_stream],
    "waldo_flow_ctx_warp_fwd": [_c_f] * 12 + [_int] * 9 + [_stream],
    "waldo_frame_warp_fuse_fwd": [_c_f] * 7 + [_int] * 9 + [_flt, _stream],
    "waldo_flow_ctx_warp_raw_fwd": [_c_f] * 13 + [_int] * 11 + [_stream],
    "waldo_frame_warp_fuse_raw_fwd": [_c_f] * 7 + [_int] * 9 + [_flt, _stream],
    # the *_dt forms: the retyped buffers as void* plus WALDO_DTYPE_* codes (include/waldo_hip.h: enum waldo_dtype)
    "waldo_flow_ctx_warp_raw_fwd_dt": [_c_f] * 13 + [_int] * 12 + [_stream],
    "waldo_frame_warp_fuse_raw_fwd_dt": [_c_f] * 7 + [_int] * 9 + [_flt, _int, _stream],
    # the packed clip (include/waldo_hip.h: "Packed clip"): uint8 (B, T, Hd, Wd, 4) in place of the fp32 input
    "waldo_unpack_clip_fwd": [_c_f] * 3 + [_int] * 5 + [_stream],
    "waldo_downscale_frames_packed_fwd": [_c_f, _c_f] + [_int] * 7 + [_stream],
    "waldo_flow_ctx_alpha_packed_fwd": [_c_f] * 7 + [_int] * 8 + [_stream],
    "waldo_frame_warp_fuse_raw_packed_fwd": [_c_f] * 8 + [_int] * 9 + [_flt, _int, _stream],
    # frame metrics (include/waldo_hip.h "Frame metrics"): two operand descriptors, then the shared arguments
    "waldo_frame_metrics_fwd": ([_c_f, _int] + [_i64] * 4) * 2 + [_c_f] + [_int] * 4 + [_flt, _flt, _int, _int]
                               + [_c_f] * 5 + [_stream],
    "waldo_flow_ctx_alpha_bwd": [_c_f] * 10 + [_int] * 10 + [_stream],
    "waldo_flow_ctx_warp_bwd": [_c_f] * 13 + [_int] * 9 + [_stream],
    "waldo_frame_warp_fuse_bwd": [_c_f] * 8 + [_int] * 9 + [_flt, _stream],
    "waldo_lyt_dist_fwd": [_c_f, _c_f, _i64, _i64, _c_f, _flt] + [_c_f] * 4 + [_i64] + [_int] * 7 + [_stream],
    "waldo_lyt_dist_bwd": [_c_f] * 3 + [_i64, _i64, _c_f, _flt] + [_c_f] * 6 + [_i64] + [_int] * 7 + [_stream],
    "waldo_wif_fuse_fwd": [_c_f, _c_f, _c_f, _i64, _int, _int, _int, _i64, _int, _stream],
    "waldo_wif_fuse_bwd": [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, _int, _i64, _int,
                           _stream],
    "waldo_wif_fuse_fwd_dt": [_c_f, _c_f, _c_f, _i64, _int, _int, _int, _i64, _int, _int, _int, _stream],
    "waldo_wif_fuse_bwd_dt": [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, _int, _i64, _int, _int, _int,
                              _stream],
    # byte output (include/waldo_hip.h "Byte output"): source descriptor, table, destination, shape, span, codes
    "waldo_frames_to_bytes_fwd": [_c_f, _int, _i64, _i64, _i64, _c_f, _c_f, _i64, _int, _i64, _int, _int, _int, _flt,
                                  _flt, _int, _stream],
    "waldo_wif_fuse_bytes_fwd": [_c_f, _c_f, _c_f, _i64, _int, _int, _int, _i64, _int, _flt, _flt, _int, _int, _stream],
    "waldo_wif_fuse_bytes_fwd_dt": [_c_f, _c_f, _c_f, _i64, _int, _int, _int, _i64, _int, _flt, _flt, _int, _int, _int,
                                    _int, _stream],
    # renders (include/waldo_hip.h "Renders"): source descriptor, table, destination(s), codes, shape
    "waldo_render_argmax_fwd": [_c_f, _int, _i64, _i64, _i64, _c_f, _c_f, _i64, _c_f, _i64, _int, _i64, _int, _int, _int,
                                _stream],
    "waldo_render_flow_fwd": [_c_f, _int, _i64, _i64, _i64, _c_f, _int, _flt, _c_f, _i64, _int, _int, _i64, _int, _int,
                              _stream],
    # supervision targets (include/waldo_hip.h "Supervision targets")
    "waldo_flow_edges_fwd": [_c_f] * 3 + [_i64, _int, _int, _int, _int, _flt, _stream],
    "waldo_gaussian_blur_fwd": [_c_f, _c_f, _i64, _int, _int, _int, _flt, _stream],
    "waldo_mov_props_fwd": [_c_f, _c_f, _u32, _u32, _u32] + [_c_f] * 4 + [_i64, _int, _i64, _stream],
    "waldo_mov_finish_fwd": [_c_f] * 7 + [_flt] * 4 + [_int] + [_c_f] * 4 + [_i64, _i64, _stream],
    "waldo_cell_distance_fwd": [_c_f] * 8 + [_i64, _i64, _int, _int, _int, _flt, _flt, _stream],
    "waldo_cell_distance_bwd": [_c_f] * 10 + [_i64, _i64, _int, _int, _int, _flt, _flt, _stream],
    # pose objective (include/waldo_hip.h "Pose objective"): the three (real, pred) pairs, the mask, ...
    "waldo_pose_l1_fwd": [_c_f] * 10 + [_i64] * 5 + [_stream],
    "waldo_pose_l1_bwd": [_c_f] * 17 + [_i64] * 4 + [_stream],
    # LPIPS level distance (include/waldo_hip.h "LPIPS level distance"): f0, f1, w, out, saved, workspace and its size,
    # N, C, P, eps; the backward: f0, f1, w, saved, grad_out, grad_f0, N, C, P
    "waldo_lpips_level_fwd": [_c_f] * 6 + [_i64] * 4 + [_flt, _stream],
    "waldo_lpips_level_bwd": [_c_f] * 6 + [_i64] * 3 + [_stream],
    # the same with 16-bit f0, f1 and grad_f0 (w, out, saved, grad_out stay fp32): a WALDO_DTYPE_* code before the stream
    "waldo_lpips_level_fwd_dt": [_c_f] * 6 + [_i64] * 4 + [_flt, _int, _stream],
    "waldo_lpips_level_bwd_dt": [_c_f] * 6 + [_i64] * 3 + [_int, _stream],
    # clip augmentation (include/waldo_hip.h "Clip augmentation"): clip, flow, the five tables, out, flow_out, B, T, Nl,
    # Hd, Wd, Hf, Wf, Ho, Wo
    "waldo_augment_clip_fwd": [_c_f] * 9 + [_int] * 9 + [_stream],
    # optimizer step (include/waldo_hip.h "Optimizer step"): the four HOST arrays of device pointers, the host arrays of
    # sizes and decays, n_tensors, state, hyper, loss, workspace and its size, adamw, the host launch count
    "waldo_adam_step": [_c_f] * 6 + [_i64] + [_c_f] * 4 + [_i64, _int, _c_f, _stream],
    "waldo_time_gather_fwd": [_c_f, _c_f, _c_f, _c_f, _c_f, _int, _int, _int, _int, _i64, _i64, _int, _stream],
    "waldo_time_gather_bwd": [_c_f, _c_f, _c_f, _c_f, _int, _int, _int, _int, _i64, _i64, _int, _stream],
    "waldo_downscale_frames_fwd": [_c_f, _c_f] + [_int] * 8 + [_stream],
    "waldo_mask_expand_fwd": [_c_f, _c_f, _c_f, _i64, _int, _int, _int, _int, _int, _flt, _stream],
    "waldo_points_in_polygon_fwd": [_c_f, _c_f, _int, _c_f, _i64, _stream],
    "waldo_points_in_polygon_dev_fwd": [_c_f, _c_f, _i64, _c_f, _i64, _int, _c_f, _i64, _i64, _stream],
    "waldo_border_objects_fwd": [_c_f, _i64, _i64, _c_f, _c_f, _i64, _i64, _i64, _i64, _c_f, _c_f, _c_f, _c_f, _i64, _int,
                                 _int, _int, _int, _int, _stream],
    "waldo_inpaint_propagate_fwd": [_c_f] * 8 + [_int] + [_c_f] * 7 + [_i64, _int, _int, _int, _int, _stream],
    "waldo_inpaint_blend_fwd": [_c_f] * 4 + [_i64, _i64, _stream],
    "waldo_inpaint_holes_fwd": [_c_f, _i64, _i64, _i64, _i64, _c_f, _c_f, _i64, _int, _int, _int, _i64, _int, _flt, _stream],
    "waldo_warp_composite_fwd": [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, _int, _int,
                                 _flt, _stream],
    "waldo_warp_composite_pts_fwd": [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _int, _int, _int, _int,
                                     _flt, _stream],
    "waldo_warp_composite_bwd": [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i64,
                                 _i64, _int, _int, _int, _int, _flt, _stream],
    # the same with a 16-bit layer stack (and grad_layers): a WALDO_DTYPE_* code before the stream
    "waldo_warp_composite_fwd_dt": [_c_f] * 6 + [_i64, _int, _int, _int, _int, _flt, _int, _stream],
    "waldo_warp_composite_pts_fwd_dt": [_c_f] * 7 + [_i64, _int, _int, _int, _int, _flt, _int, _stream],
    "waldo_warp_composite_bwd_dt": [_c_f] * 10 + [_i64, _i64, _int, _int, _int, _int, _flt, _int, _stream],
    # deterministic mode (include/waldo_hip.h "Reproducible gradients"): the backward entry points whose sums do not
    # depend on the order of arrival; outputs overwritten, one workspace each (DET_QUERIES)
    "waldo_grid_sample2d_bwd_det": [_c_f] * 5 + [_i64, _i64, _int, _int, _int, _int, _int, _flt, _i64, _i64, _c_f, _i64,
                                                 _stream],
    "waldo_grid_sample2d_ex_bwd_det": [_c_f] * 5 + [_i64, _i64, _int, _int, _int, _int, _int, _flt, _i64, _i64, _i64,
                                                    _i64, _i64, _flt, _flt, _c_f, _i64, _stream],
    "waldo_occ_composite_bwd_det": [_c_f] * 5 + [_i64, _int, _i64, _i64, _c_f, _i64, _stream],
    "waldo_tps_grid_bwd_det": [_c_f, _c_f, _c_f, _i64, _i64, _int, _c_f, _i64, _stream],
    "waldo_flow_ctx_alpha_bwd_det": [_c_f] * 10 + [_i64] + [_int] * 10 + [_stream],
    "waldo_flow_ctx_warp_bwd_det": [_c_f] * 13 + [_i64] + [_int] * 9 + [_stream],
    "waldo_warp_composite_bwd_det": [_c_f] * 10 + [_i64, _i64, _int, _int, _int, _int, _flt, _int, _stream],
    # plane norm (include/waldo_hip.h "Plane norm"): x and its strides, the affine, ..., workspace and its size, shape
    "waldo_plane_norm_gelu_fwd": [_c_f, _i64, _i64, _c_f, _c_f, _flt, _c_f, _i64, _i64, _c_f, _i64, _c_f, _c_f, _c_f, _i64,
                                  _i64, _int, _int, _int, _int, _stream],
    "waldo_plane_norm_gelu_bwd": [_c_f, _i64, _i64, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _c_f, _c_f, _c_f, _i64, _i64,
                                  _int, _int, _int, _stream],
    # the same with 16-bit tensor-sized buffers: a WALDO_DTYPE_* code before the stream
    "waldo_plane_norm_gelu_fwd_dt": [_c_f, _i64, _i64, _c_f, _c_f, _flt, _c_f, _i64, _i64, _c_f, _i64, _c_f, _c_f, _c_f, _i64,
                                     _i64, _int, _int, _int, _int, _int, _stream],
    "waldo_plane_norm_gelu_bwd_dt": [_c_f, _i64, _i64, _c_f, _c_f, _c_f, _c_f, _c_f, _i64, _i64, _c_f, _c_f, _c_f, _i64, _i64,
                                     _int, _int, _int, _int, _stream],
    # token attention (include/waldo_hip.h "Token attention"): q, k1, v1, k2, v2 with a batch and a token stride each,
    # out, scale, B, H, D, Nq, Nk1, Nk2
    "waldo_token_attention_fwd": [_c_f, _i64, _i64] * 5 + [_c_f, _flt, _i64, _int, _int, _int, _int, _int, _stream],
    # the same with lse (B, H, Nq) after out; the backward: the five views, out, grad_out, lse, delta, the five
    # gradients (None: not wanted), scale, B, H, D, Nq, Nk1, Nk2
    "waldo_token_attention_fwd_lse": [_c_f, _i64, _i64] * 5 + [_c_f, _c_f, _flt, _i64, _int, _int, _int, _int, _int,
                                                               _stream],
    "waldo_token_attention_bwd": [_c_f, _i64, _i64] * 5 + [_c_f] * 9 + [_flt, _i64, _int, _int, _int, _int, _int, _stream],
    # token attention over clips (include/waldo_hip.h "Token attention over clips"): q, k, v with a token stride each,
    # the two offset tables, out (, lse), scale, B, H, D, Rq, Rk, max_q_len, max_k_len; the backward: ..., the tables,
    # out, grad_out, lse, delta, the three gradients (None: not wanted), scale, ...
    "waldo_token_attention_clips_fwd": [_c_f, _i64] * 3 + [_c_f] * 3 + [_flt, _i64, _int, _int, _i64, _i64, _int, _int,
                                                                        _stream],
    "waldo_token_attention_clips_fwd_lse": [_c_f, _i64] * 3 + [_c_f] * 4 + [_flt, _i64, _int, _int, _i64, _i64, _int, _int,
                                                                            _stream],
    "waldo_token_attention_clips_bwd": [_c_f, _i64] * 3 + [_c_f] * 9 + [_flt, _i64, _int, _int, _i64, _i64, _int, _int,
                                                                        _stream],
    # the two forwards on 16-bit operands and out: a WALDO_DTYPE_* code before the stream
    "waldo_token_attention_fwd_dt": [_c_f, _i64, _i64] * 5 + [_c_f, _flt, _i64, _int, _int, _int, _int, _int, _int,
                                                              _stream],
    # the dense form's forward with lse (fp32) after out, and its backward: waldo_token_attention_bwd's arguments
    "waldo_token_attention_fwd_lse_dt": [_c_f, _i64, _i64] * 5 + [_c_f, _c_f, _flt, _i64, _int, _int, _int, _int, _int,
                                                                  _int, _stream],
    "waldo_token_attention_bwd_dt": [_c_f, _i64, _i64] * 5 + [_c_f] * 9 + [_flt, _i64, _int, _int, _int, _int, _int, _int,
                                                                          _stream],
    "waldo_token_attention_clips_fwd_dt": [_c_f, _i64] * 3 + [_c_f] * 3 + [_flt, _i64, _int, _int, _i64, _i64, _int, _int,
                                                                           _int, _stream],
}
# workspace size of each *_det entry point (0: no deterministic kernel for the shape)
DET_QUERIES = {
    "waldo_grid_sample2d_bwd_det_workspace_bytes": [_i64, _i64, _int, _int, _int, _int, _int],
    "waldo_occ_composite_bwd_det_workspace_bytes": [_i64, _int, _i64],
    "waldo_tps_grid_bwd_det_workspace_bytes": [_i64, _i64, _int],
    "waldo_flow_ctx_alpha_bwd_det_workspace_bytes": [_int] * 7,
    "waldo_flow_ctx_warp_bwd_det_workspace_bytes": [_int] * 8,
    "waldo_warp_composite_bwd_det_workspace_bytes": [_i64, _int, _int, _int, _int],
}
PLAIN = {"waldo_version": (_int, []), "waldo_max_layers": (_int, []),
         "waldo_warp_composite_bwd_workspace_bytes": (_i64, [_i64, _int, _int, _int, _int]),
         "waldo_lyt_dist_workspace_bytes": (_i64, [_i64, _int, _int, _int, _int, _int]),
         "waldo_border_objects_workspace_bytes": (_i64, [_i64]),
         "waldo_cell_distance_workspace_bytes": (_i64, [_i64, _int, _i64]),
         "waldo_pose_l1_workspace_bytes": (_i64, [_i64] * 4),
         "waldo_lpips_level_workspace_bytes": (_i64, [_i64] * 3),
         "waldo_lpips_level_saved_bytes": (_i64, [_i64] * 3),
         "waldo_frame_metrics_partial_bytes": (_i64, [_int] * 5),
         "waldo_frame_metrics_scratch_bytes": (_i64, [_int] * 5),
         "waldo_plane_norm_workspace_bytes": (_i64, [_i64, _int, _int, _int]),
         "waldo_plane_norm_limits": (_int, [ctypes.POINTER(ctypes.c_int), _int]),
         "waldo_adam_limits": (_int, [ctypes.POINTER(ctypes.c_int), _int]),
         "waldo_adam_workspace_bytes": (_i64, [_i64, ctypes.POINTER(_i64)]),
         "waldo_token_attention_limits": (_int, [ctypes.POINTER(ctypes.c_int), _int]),
         "waldo_token_attention_bwd_limits": (_int, [ctypes.POINTER(ctypes.c_int), _int]),
         "waldo_token_attention_dt_limits": (_int, [ctypes.POINTER(ctypes.c_int), _int]),
         "waldo_warp_composite_pts_supported": (_int, [_int, _int, _int, _int]),
         "waldo_last_error_string": (ctypes.c_char_p, []),
         "waldo_set_debug_option": (_int, [_int, _int]),
         "waldo_host_device_pointer": (_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)])}
PLAIN.update({name: (_i64, argtypes) for name, argtypes in DET_QUERIES.items()})

# include/waldo_hip.h: test-only switches between kernel variants (waldo_set_debug_option: the library's one piece of
# process-global state)
DEBUG_FWD_PLAIN = 0
DEBUG_IW_PASSES = 1
DEBUG_BWD_GENERIC = 2
INDEX_STATUS_WORDS = 4

_lock = threading.Lock()
_lib = None


class WaldoHipError(RuntimeError):
    pass


def use_library(path):
    """Bind another build of the library (developer A/B runs: tools_dev/).  Only before the first call
    of any op -- the process keeps ONE library; nothing reads the environment.  load() holds it to the same ABI
    version as the product library."""
    global LIB_PATH
    with _lock:
        if _lib is not None:
            raise WaldoHipError(f"use_library({path!r}): {LIB_PATH} is already loaded")
        LIB_PATH = os.path.abspath(path)


def load():
    """Open the library (once) and declare every prototype.  Raises if it is absent or of another ABI."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise WaldoHipError(
                f"{LIB_PATH} not found: build it with `python -m waldo_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_LOCAL)
        lib.waldo_version.restype = _int
        lib.waldo_version.argtypes = []
        if lib.waldo_version() != ABI_VERSION:
            raise WaldoHipError(
                f"{LIB_PATH} has ABI version {lib.waldo_version()}, this binding needs {ABI_VERSION}: "
                "rebuild it with `python -m waldo_amd.build --force`")
        for name, argtypes in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = _int
        for name, (res, argtypes) in PLAIN.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = res
        _lib = lib
    return _lib


class IndexStatus:
    """The caller's side of include/waldo_hip.h's "Frame-index status": four sticky int32 words in PINNED HOST memory
    that the kernels write, through the words' device address, when ``ctx_ts`` / ``pred_ts`` hold a frame index
    outside its time axis (they clamp it for memory safety and report; the reference's ``gather_time``,
    models/nets/lvd.py:462-467, fails with a device-side assert there).  Reading the words costs no device
    synchronisation, so an owner (``Warper``: one per module) checks them at every call for what EARLIER launches
    reported, and ``check(sync=True)`` gives the raise-at-once behaviour.  Replaces the host-side index bookkeeping
    of rounds 3-5 (one device -> host read per distinct index tensor and version)."""

    _live = None  # weak set of every IndexStatus of the process (check_all: after a HIP-graph replay)

    def __init__(self):
        import weakref
        self.words = torch.zeros(INDEX_STATUS_WORDS, dtype=torch.int32).pin_memory()
        dev = ctypes.c_void_p()
        if load().waldo_host_device_pointer(self.words.data_ptr(), ctypes.byref(dev)) != 0:
            msg = load().waldo_last_error_string()
            raise WaldoHipError(f"IndexStatus: {msg.decode() if msg else '?'}")
        self.ptr = dev.value
        self._np = self.words.numpy()
        if IndexStatus._live is None:
            IndexStatus._live = weakref.WeakSet()
        IndexStatus._live.add(self)

    def __deepcopy__(self, memo):  # (a copied module gets words of its own: the device address is not copyable)
        return IndexStatus()

    def __reduce__(self):
        return (IndexStatus, ())

    def check(self, sync=False):
        """Raise ``WaldoHipError`` if a kernel has reported an index outside its range since the last check (and clear
        the words).  ``sync``: wait for the current stream first, so that every launch queued so far has run.  A no-op
        while a HIP graph is being captured."""
        if torch.cuda.is_current_stream_capturing():
            return
        if sync:
            torch.cuda.current_stream().synchronize()
        if self._np[0] or self._np[2]:
            lim_c, bad_c, lim_p, bad_p = (int(v) for v in self._np)
            self._np[:] = 0
            what = [f"{name} holds the index {bad}, valid range is [0, {lim - 1}]"
                    for name, lim, bad in (("ctx_ts", lim_c, bad_c), ("pred_ts", lim_p, bad_p)) if lim]
            raise WaldoHipError("frame index outside its time axis (reported by a kernel; the frame was clamped): "
                                + "; ".join(what))

    @staticmethod
    def check_all(sync=False):
        for st in list(IndexStatus._live or ()):
            st.check(sync)
            sync = False


_default_status = None


def default_index_status():
    """The status words of callers that pass none: ``functional`` checks them with a synchronisation before it
    returns (the strict mode of a stand-alone call)."""
    global _default_status
    if _default_status is None:
        _default_status = IndexStatus()
    return _default_status


def ptr(t):
    """Device pointer of a tensor (None -> NULL), as the integer ctypes converts to ``void*`` itself."""
    if t is None:
        return None
    return t.data_ptr()


def check_cuda(*tensors, half=False):
    """GPU tensors of fp32 -- or, with ``half`` (the buffers an entry point with a dtype code retypes), of fp32, fp16
    or bf16."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise WaldoHipError("waldo_amd ops need tensors on the GPU (cuda device); "
                                "there is no CPU fallback")
        if t.dtype != torch.float32 and not (half and t.dtype in (torch.float16, torch.bfloat16)):
            raise WaldoHipError(f"waldo_amd ops are fp32-only, got {t.dtype}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream(device):
    """The ``hipStream_t`` PyTorch launches on for ``device`` right now (inside ``torch.cuda.stream(...)``: that one).
    The raw query when the build has it: a library call is ~20 us of interpreter time around a ~5 us launch, and the
    LVD training step makes ~45 of them -- building a ``torch.cuda.Stream`` object per call was a quarter of that."""
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


class on_device:
    """``with on_device(dev):`` = ``with torch.cuda.device(dev):`` (the kernels launch on the CURRENT device) that
    costs nothing when ``dev`` already is the current device -- the one-GPU-per-process case."""
    __slots__ = ("guard",)

    def __init__(self, device):
        self.guard = None if device.index is None or device.index == torch.cuda.current_device() else torch.cuda.device(device)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *exc):
        if self.guard is not None:
            return self.guard.__exit__(*exc)
        return False


class KernelTimer:
    """Optional per-entry-point device timing: records an event pair on the launch stream around
    every C-ABI call (bench.py uses it for the live roofline numbers).  Off by default."""

    def __init__(self):
        self.pairs = {}

    def __enter__(self):
        global _timer
        _timer = self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = None
        return False

    def summary(self):
        """name -> (launches, mean milliseconds); call after torch.cuda.synchronize()."""
        out = {}
        for name, evs in self.pairs.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[name] = (len(ms), sum(ms) / max(len(ms), 1))
        return out


_timer = None


def call(name, *args):
    """Call an entry point; raise WaldoHipError with the library's message on failure."""
    lib = load()
    if _timer is not None:
        start = torch.cuda.Event(enable_timing=True)
        stop = torch.cuda.Event(enable_timing=True)
        start.record()
        rc = getattr(lib, name)(*args)
        stop.record()
        _timer.pairs.setdefault(name, []).append((start, stop))
    else:
        rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.waldo_last_error_string()
        raise WaldoHipError(f"{name} failed ({rc}): {msg.decode() if msg else '?'}")


def query(name, *args):
    """A size query of the library (``*_workspace_bytes``): launches nothing."""
    return getattr(load(), name)(*args)


_Tensor = torch.Tensor
_AS_IS = frozenset((int, float, type(None)))


def pointers(args):
    """``args`` as an entry point takes them: every tensor (subclasses too) as its ``data_ptr()``; None (NULL), ints and
    floats as they are -- addresses that already travel as integers (status words, host arrays) among them.  (Most
    arguments are plain ints: their exact type is looked up first, ``isinstance`` of a tensor class goes through its
    metaclass.)"""
    return [a if type(a) in _AS_IS else a.data_ptr() if isinstance(a, _Tensor) else a for a in args]


def launch(name, device, *args):
    """THE way an op launches: entry point ``name`` on ``device`` (entered only when it is not the current one), tensors
    passed as themselves (``pointers``), on the stream PyTorch launches on for that very device, appended as the last
    argument -- where every prototype of SIGNATURES has it.  No checks of the arguments: strided views are passed on
    purpose, and this is the host's hot path (see ``current_stream``)."""
    if device.index is None or device.index == torch.cuda.current_device():
        call(name, *pointers(args), current_stream(device))
    else:
        with torch.cuda.device(device):
            call(name, *pointers(args), current_stream(device))
