"""ctypes binding of the C ABI in ``include/fastscnn.h`` (libfastscnn_hip.so).

There is no fallback: if the library is missing or fails to load, every entry point raises
``RuntimeError`` — the HIP path is the product, never a CPU restatement.
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FSCNN_LIB", os.path.join(_HERE, "libfastscnn_hip.so"))

DT_F32, DT_BF16, DT_F16 = 0, 1, 2
DT_U8 = 3  # frames of the deployment front end only (fscnn_e2e_pre)

c_int, c_ll, c_float, c_vp, c_char_p = (ctypes.c_int, ctypes.c_longlong, ctypes.c_float,
                                        ctypes.c_void_p, ctypes.c_char_p)
c_ull, c_double = ctypes.c_ulonglong, ctypes.c_double
P_int, P_ll, P_vp = ctypes.POINTER(c_int), ctypes.POINTER(c_ll), ctypes.POINTER(c_vp)
P_float = ctypes.POINTER(c_float)
P_double = ctypes.POINTER(c_double)
c_uint, P_ubyte = ctypes.c_uint, ctypes.POINTER(ctypes.c_ubyte)


class AuxHead(ctypes.Structure):
    """``fscnn_aux_head`` of include/fastscnn.h (the aux loss heads' criterion)."""
    _fields_ = [("head", c_int), ("aux_weight", c_float), ("ignore_index", c_ll),
                ("smooth", c_float), ("dice_weight", c_float), ("focal_weight", c_float),
                ("alpha", c_float), ("gamma", c_float), ("thresh", c_float), ("min_kept", c_ll),
                ("class_weight", c_vp)]


P_aux_head = ctypes.POINTER(AuxHead)


class PathParams(ctypes.Structure):
    """``fscnn_path_params`` of include/fastscnn.h (the steering tail's law)."""
    _fields_ = [("degree", c_int), ("num_waypoints", c_int), ("fast", c_int), ("min_width", c_int),
                ("skip_rows", c_int), ("scan_from_bottom", c_int), ("force_bottom_center", c_int),
                ("reserved", c_int),
                ("min_x", c_double), ("min_y", c_double), ("max_y", c_double),
                ("pixels_per_unit", c_double), ("anchor_x", c_double), ("anchor_y", c_double),
                ("car_x", c_double), ("car_y", c_double), ("steering_gain", c_double),
                ("base_pwm", c_double), ("curvature_damping", c_double),
                ("preview_distance", c_double), ("max_pwm", c_double), ("min_pwm", c_double),
                ("ema_alpha", c_double)]


P_path_params = ctypes.POINTER(PathParams)

# name -> (restype, argtypes)
SIGNATURES = {
    "fscnn_version": (c_char_p, []),
    "fscnn_last_error": (c_char_p, []),
    "fscnn_net_create": (c_int, [c_int, c_int, P_vp]),
    "fscnn_net_destroy": (None, [c_vp]),
    "fscnn_net_param_count": (c_int, [c_vp, P_int, P_ll]),
    "fscnn_net_param_info": (c_int, [c_vp, c_int, ctypes.POINTER(c_char_p), P_ll, P_ll]),
    "fscnn_net_buffer_count": (c_int, [c_vp, P_int, P_ll, P_int]),
    "fscnn_net_buffer_info": (c_int, [c_vp, c_int, ctypes.POINTER(c_char_p), P_ll, P_ll]),
    "fscnn_net_stage_range": (c_int, [c_vp, c_int, P_ll, P_ll]),
    "fscnn_plan_create": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, P_vp]),
    "fscnn_plan_destroy": (None, [c_vp]),
    "fscnn_plan_workspace": (c_int, [c_vp, P_ll, P_ll]),
    "fscnn_plan_shapes": (c_int, [c_vp, P_int]),
    "fscnn_plan_buffer": (c_int, [c_vp, c_char_p, P_ll, P_ll, P_int, P_int, P_int]),
    "fscnn_forward": (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_ull,
                              c_float, c_float, c_vp]),
    "fscnn_backward": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_ull, c_float,
                               c_int, c_int, c_vp]),
    "fscnn_normalize_u8": (c_int, [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp]),
    "fscnn_remap_labels": (c_int, [c_vp, c_ll, c_vp, c_int, c_int, c_ll, c_vp, c_vp]),
    "fscnn_sync_tables": (c_int, [c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, P_int]),
    "fscnn_sync_blur_weights": (c_int, [c_float, ctypes.POINTER(ctypes.c_uint),
                                        ctypes.POINTER(ctypes.c_uint)]),
    "fscnn_sync_transform": (c_int, [c_vp, c_vp, c_ll, c_int, c_int, c_vp, c_int, c_int, c_vp,
                                     c_vp, c_vp, c_int, c_vp, c_vp, c_vp]),
    "fscnn_ohem_prob": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_ll, c_ll, c_float, c_vp, c_vp,
                                c_vp]),
    "fscnn_ohem_threshold": (c_int, [c_vp, c_ll, c_vp, c_ll, c_float, c_vp, c_vp, c_vp]),
    "fscnn_ce_weighted_fwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_ll, c_ll, c_vp, c_vp,
                                      c_vp, c_vp, c_vp, c_vp]),
    "fscnn_ce_weighted_bwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_ll, c_ll, c_vp, c_vp,
                                      c_vp, c_vp, c_vp, c_vp, c_vp]),
    "fscnn_dice_fwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_ll, c_float, c_float, c_int,
                               c_vp, c_vp, c_vp]),
    "fscnn_dice_bwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_ll, c_float, c_float, c_int,
                               c_vp, c_vp, c_float, c_float, c_float, c_vp, c_vp]),
    "fscnn_predict": (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "fscnn_validate_ws_bytes": (c_ll, [c_vp]),
    "fscnn_validate": (c_int, [c_vp, c_vp, c_int, c_vp, c_int, c_ll, c_float, c_float, c_float,
                               c_float, c_float, c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                               c_vp]),
    "fscnn_e2e_pre": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P_float, P_float,
                              c_vp, c_int, c_vp]),
    "fscnn_e2e_head": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                               c_int, c_vp, c_int, c_vp, c_int, c_vp]),
    "fscnn_e2e_ws_bytes": (c_ll, [c_vp]),
    "fscnn_forward_e2e": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, P_float, P_float,
                                  c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp,
                                  c_vp, c_vp]),
    "fscnn_bev_mask": (c_int, [c_vp, c_int, c_int, c_int, P_double, c_int, c_int, c_int, c_vp, c_vp,
                               c_vp]),
    "fscnn_e2e_bev": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_int, P_double, c_int, c_int, c_int, c_vp, c_vp, c_vp]),
    "fscnn_forward_e2e_bev": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, P_float,
                                      P_float, c_int, c_int, c_int, P_double, c_int, c_int, c_int,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "fscnn_bev_image": (c_int, [c_vp, c_int, c_int, c_int, c_int, P_double, c_int, c_int, c_vp,
                                c_vp, P_ubyte, c_float, c_float, c_float, c_vp, c_vp]),
    "fscnn_path_plan": (c_int, [c_vp, c_int, c_int, P_path_params, c_vp, c_vp, c_vp]),
    "fscnn_overlay_mask": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_int,
                                   P_ubyte, c_vp, c_int, c_float, c_float, c_float, c_vp, c_vp,
                                   c_vp]),
    "fscnn_e2e_overlay": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_int, c_int, c_vp, c_int, c_int, c_int, c_int, P_ubyte, c_uint,
                                  c_float, c_float, c_float, c_vp, c_vp, c_vp]),
    "fscnn_forward_e2e_overlay": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, P_float,
                                          P_float, c_int, c_int, c_int, P_ubyte, c_uint, c_float,
                                          c_float, c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                          c_vp]),
    "fscnn_seg_metric": (c_int, [c_vp, c_int, c_vp, c_ll, c_int, c_vp, c_vp]),
    "fscnn_forward_aux": (c_int, [c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp,
                                  c_ull, c_float, c_float, c_vp]),
    "fscnn_backward_aux": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_ull,
                                   c_float, c_int, c_int, c_vp]),
    "fscnn_forward_loss": (c_int, [c_vp, c_vp, c_int, c_vp, c_ll, c_vp, c_vp, c_vp, c_vp, c_vp,
                                   c_ull, c_float, c_float, c_vp]),
    "fscnn_backward_loss": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_ull,
                                    c_float, c_int, c_int, c_vp]),
    "fscnn_dice_head_ws_bytes": (c_ll, [c_vp]),
    "fscnn_forward_loss_dice": (c_int, [c_vp, c_vp, c_int, c_vp, c_float, c_float, c_float,
                                        c_float, c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                        c_ull, c_float, c_float, c_vp]),
    "fscnn_backward_loss_dice": (c_int, [c_vp, c_vp, c_vp, c_float, c_float, c_float, c_vp, c_int,
                                         c_vp, c_vp, c_vp, c_vp, c_vp, c_ull, c_float, c_int,
                                         c_int, c_vp]),
    "fscnn_forward_loss_ohem": (c_int, [c_vp, c_vp, c_int, c_vp, c_ll, c_float, c_ll, c_vp, c_vp,
                                        c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_ull,
                                        c_float, c_float, c_vp]),
    "fscnn_aux_head_ws_bytes": (c_ll, [c_vp, c_int]),
    "fscnn_aux_head_ws_offset": (c_ll, [c_vp, c_int, c_char_p, c_int]),
    "fscnn_forward_loss_aux": (c_int, [c_vp, c_vp, c_int, c_vp, P_aux_head, c_vp, c_vp, c_vp, c_vp,
                                       c_vp, c_vp, c_ull, c_float, c_float, c_vp]),
    "fscnn_backward_loss_aux": (c_int, [c_vp, c_vp, P_aux_head, c_vp, c_int, c_vp, c_int, c_vp,
                                        c_vp, c_vp, c_vp, c_vp, c_ull, c_float, c_int, c_int,
                                        c_vp]),
    "fscnn_backward_dx": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp,
                                  c_vp, c_vp, c_vp, c_ull, c_float, c_int, c_int, c_vp]),
    "fscnn_prof_begin": (c_int, [c_int, c_int]),
    "fscnn_prof_end": (c_int, [ctypes.POINTER(ctypes.c_double), P_ll, ctypes.POINTER(ctypes.c_double),
                               ctypes.POINTER(ctypes.c_double)]),
    "fscnn_prof_launch": (c_int, [c_ll, ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_float),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(c_char_p)]),
    "fscnn_prof_kind_name": (c_char_p, [c_int]),
    "fscnn_ce_parts": (c_ll, [c_int, c_ll]),
    "fscnn_ce_fwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_ll, c_ll, c_vp, c_vp, c_vp]),
    "fscnn_ce_bwd": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_ll, c_ll, c_vp, c_vp, c_vp,
                             c_vp]),
    "fscnn_sgd": (c_int, [c_vp, c_vp, c_vp, c_ll, c_float, c_float, c_float, c_float, c_int,
                          c_int, c_float, c_vp]),
    "fscnn_adamw": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_ll, c_double, c_double, c_double,
                            c_double, c_double, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp]),
    "fscnn_adamw_segments": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_int,
                                     c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp, c_vp]),
    "fscnn_conv0_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp,
                                c_int, c_vp]),
    "fscnn_conv0_wgrad_slab_floats": (c_ll, [c_int, c_int, c_int]),
    "fscnn_conv0_wgrad": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp]),
    "fscnn_dw3x3_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                                c_int, c_vp, c_vp]),
    "fscnn_dw3x3_dgrad": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                  c_vp]),
    "fscnn_dw3x3_wgrad_slab_floats": (c_ll, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "fscnn_dw3x3_wgrad": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                                  c_vp, c_vp]),
    "fscnn_pw_gemm": (c_int, [c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_int, c_vp, c_vp,
                              c_vp, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp]),
    "fscnn_pw_dgrad_bnbwd": (c_int, [c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_int,
                                     c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_int,
                                     c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, P_int, c_vp]),
    "fscnn_kth_smallest": (c_int, [c_vp, c_ll, c_ll, c_vp, c_vp, c_vp]),
    "fscnn_debug_stamps": (c_int, [c_vp, c_int]),
    "fscnn_debug_stamp_count": (c_int, []),
    "fscnn_debug_stamp_tag": (c_char_p, [c_int]),
    "fscnn_pw_wgrad_slab_floats": (c_ll, [c_int, c_int, c_int]),
    "fscnn_pw_gemm_stats_parts": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "fscnn_pw_wgrad": (c_int, [c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_int,
                               c_vp]),
    "fscnn_bn_finalize": (c_int, [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_float,
                                  c_vp, c_vp, c_vp, c_vp, c_vp]),
    "fscnn_bilinear_ac_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_vp, c_int, c_int, c_vp]),
    "fscnn_bilinear_ac_bwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_vp, c_vp, c_vp]),
    "fscnn_pyramid_pool_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                                       c_vp]),
    "fscnn_block_ir_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                   c_vp, c_int, c_vp]),
    "fscnn_pyramid_pool_bwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_int,
                                       c_int, c_vp]),
    # train-only kernels in the executor's form (tests/test_gpu_train_kernels.py)
    "fscnn_bn_apply": (c_int, [c_ll, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp,
                               c_int, c_int, c_vp, c_int, c_int, c_vp]),
    "fscnn_bn_bwd": (c_int, [c_ll, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp,
                             c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                             c_vp, c_vp, c_vp, c_vp, c_int, P_int, P_int, c_vp]),
    "fscnn_ppm_branches_ok": (c_int, [c_int, c_int, c_int]),
    "fscnn_ppm_branches_fwd": (c_int, [c_int, P_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                       c_vp, c_float, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp,
                                       c_int, c_vp]),
    "fscnn_ppm_branches_bwd": (c_int, [c_int, P_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp,
                                       c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                       c_vp]),
    "fscnn_ppm_up_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_vp, c_int, c_int, c_vp]),
    "fscnn_ppm_up_bwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp]),
    "fscnn_dropout": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_ull, c_vp, c_ull,
                              c_float, c_vp, c_vp, c_vp, c_int, c_vp]),
    "fscnn_dw3x3_parts": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "fscnn_dw3x3_ct_width": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "fscnn_dw3x3_fwd_train": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                      c_float, c_vp, c_vp, c_vp, c_vp, P_int, c_vp]),
    "fscnn_dw3x3_dgrad_bn": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                     c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp,
                                     c_vp, c_vp, P_int, c_vp]),
    "fscnn_dw3x3_wgrad_train": (c_int, [c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_vp, c_vp, c_vp, c_vp, c_vp]),
    "fscnn_pw_fwd_train_route": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, P_int]),
    "fscnn_pw_fwd_train": (c_int, [c_int, c_int, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_vp,
                                   c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                   c_float, c_vp, c_vp, c_vp, c_vp, c_int, P_int, P_int, c_vp]),
    "fscnn_pw_wgrad_train": (c_int, [c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_vp,
                                     c_vp, c_vp, c_vp, c_vp, c_int, P_int, c_vp]),
    "fscnn_pw_dgrad_train_route": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                           P_int]),
    "fscnn_pw_dgrad_train": (c_int, [c_int, c_int, c_int, c_vp, c_int, c_vp, c_int, c_vp, c_int,
                                     c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_int,
                                     c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_float,
                                     c_ull, c_ull, c_vp, c_int, P_int, P_int, c_vp]),
    "fscnn_im2col3": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "fscnn_col2im3": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_int, c_int,
                              c_vp]),
    "fscnn_block_ir_s2_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                      c_int, c_vp]),
    "fscnn_block_ltd_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp,
                                    c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    "fscnn_block_dsconv_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp,
                                       c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    "fscnn_block_dsconv_res_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                           c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                                           c_vp, c_int, c_vp]),
    "fscnn_block_cls_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int] + [c_vp] * 14 + [c_int, c_vp, c_vp,
                                                                              c_int, c_vp]),
    "fscnn_block_ffm_fwd": (c_int, [c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_int,
                                    c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                    c_int, c_vp]),
}

_lib = None
_lock = threading.Lock()


def load():
    """Load (once) and return the ctypes library; raises RuntimeError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libfastscnn_hip.so not found at %s — build it with "
                "`python -c 'import __graft_entry__; __graft_entry__.build()'` "
                "(there is no CPU fallback)" % LIB_PATH)
        # torch must be imported first so its bundled HIP runtime (same soname) is the one used
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().fscnn_last_error().decode(errors="replace")
        raise RuntimeError("fastscnn HIP error %d in %s: %s" % (rc, what, msg))


def call(name, *args):
    rc = getattr(load(), name)(*args)
    check(rc, name)
    return rc


def ptr(t):
    """Device pointer of a tensor (None → NULL)."""
    return None if t is None else c_vp(t.data_ptr())


def stream_ptr(device=None):
    import torch
    return c_vp(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(dt):
    import torch
    if dt == torch.float32:
        return DT_F32
    if dt == torch.bfloat16:
        return DT_BF16
    if dt == torch.float16:
        return DT_F16
    raise RuntimeError("fastscnn: unsupported dtype %s (fp32 / bf16 / fp16)" % (dt,))
