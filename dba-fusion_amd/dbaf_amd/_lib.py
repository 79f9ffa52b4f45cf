"""Loader for the gfx950 C-ABI library (dba-fusion_amd/lib/libdba_hip.so, include/dba_hip.h).

The library is built in-tree by `make lib` / `__graft_entry__.build()`.  There is NO fallback: if the
shared object is missing or a call fails, the product path raises -- it never computes on the CPU.
"""
import ctypes
import os
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DBA_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libdba_hip.so")

DBA_F32, DBA_F16, DBA_F64, DBA_U8 = 0, 1, 2, 3
_ERR = {-1: "DBA_ERR_ARG", -2: "DBA_ERR_WORKSPACE", -3: "DBA_ERR_HIP", -4: "DBA_ERR_UNSUPPORTED"}

c_int, c_float, c_size_t, c_void_p = ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p


class BaLayout(ctypes.Structure):
    _fields_ = [(n, c_size_t) for n in ("H", "b", "dx", "meta", "E", "Q", "w", "kx")] + \
               [("P", c_int), ("Mmax", c_int), ("nchunks", c_int)]


class ShardExchange(ctypes.Structure):
    """dba_shard_exchange of include/dba_hip.h"""
    _fields_ = [("world", c_int), ("rank", c_int), ("comm", c_void_p), ("peer_regions", c_void_p),
                ("peer_epoch", ctypes.POINTER(ctypes.c_uint)), ("peer_max_doubles", c_size_t), ("peer_status", c_void_p),
                ("band_idx", c_void_p), ("band_len", c_size_t), ("band_buf", c_void_p),
                ("my_rows", c_void_p), ("n_mine", c_int), ("kmax", c_int), ("all_rows", c_void_p), ("all_slots", c_void_p),
                ("n_all", c_int), ("send", c_void_p), ("recv", c_void_p)]


class RowJob(ctypes.Structure):
    """dba_row_job of include/dba_hip.h"""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("pos", c_void_p), ("row_bytes", ctypes.c_int64),
                ("count", c_int), ("dst_row0", c_int), ("src_rows", c_int), ("dst_rows", c_int)]


class AfJob(ctypes.Structure):
    """dba_af_job of include/dba_hip.h"""
    _fields_ = [("kind", c_int), ("reserved", c_int), ("rows", RowJob)]


class AfGeometry(ctypes.Structure):
    """dba_af_geometry of include/dba_hip.h"""
    _fields_ = [("poses", c_void_p), ("disps", c_void_p), ("intrinsics_b4", c_void_p), ("ii", c_void_p), ("jj", c_void_p),
                ("n_frames", c_int), ("ht", c_int), ("wd", c_int), ("reserved", c_int)]


class UpdHead(ctypes.Structure):
    """dba_upd_head_t of include/dba_hip.h"""
    _fields_ = [("x", c_void_p), ("weight", c_void_p), ("bias", c_void_p), ("out", c_void_p), ("sum", c_void_p),
                ("k", c_int), ("relu_in", c_int), ("act", c_int), ("scale", c_float), ("out_f32", c_int)]


class FrameItem(ctypes.Structure):
    """dba_frame_item of include/dba_hip.h"""
    _fields_ = [(n, c_void_p) for n in ("tstamp", "images", "poses", "disps", "disps_sens", "intrinsics", "fmaps", "nets",
                                        "inps")] + \
               [(n, c_int) for n in ("rows", "row", "ht", "wd")] + \
               [(n, ctypes.c_int64) for n in ("fmap_row_bytes", "net_row_bytes", "inp_row_bytes")] + \
               [("tstamp_value", ctypes.c_double)] + \
               [(n, c_void_p) for n in ("image", "fmap", "net", "inp", "pose_dev", "intr_dev", "disp_dev", "depth")] + \
               [(n, c_int) for n in ("pose_mode", "intr_mode", "disp_mode", "seed_disps")] + \
               [("pose", c_float * 7), ("intr", c_float * 4), ("disp_fill", c_float)]


class InertialState(ctypes.Structure):
    """dba_inertial_state of include/dba_hip.h"""
    _fields_ = [(n, c_void_p) for n in ("R", "p", "vel", "bias", "prior_R", "prior_p", "prior_vel", "prior_bias", "prior_w")] + \
               [("gravity", ctypes.c_double * 3)] + \
               [(n, c_void_p) for n in ("dense_R", "dense_p", "dense_vel", "dense_bias", "dense_H", "dense_b")] + [("dense_K", c_int)]


# every exported symbol of include/dba_hip.h with its (restype, argtypes); pointers are void*
_P = c_void_p
SYMBOLS = {
    "dba_version": (ctypes.c_char_p, []),
    "dba_last_error": (ctypes.c_char_p, []),
    "dba_ba_workspace_bytes": (c_size_t, [c_int] * 6),
    "dba_ba_get_layout": (c_int, [c_int] * 6 + [ctypes.POINTER(BaLayout)]),
    "dba_ba_prepare": (c_int, [_P, _P] + [c_int] * 6 + [_P, c_size_t, _P]),
    "dba_ba_prepare_keyed": (c_int, [_P, _P] + [c_int] * 8 + [_P, c_size_t, _P]),
    "dba_ba_workspace_init": (c_int, [c_int] * 6 + [_P, c_size_t, _P]),
    "dba_ba_solver_verdict": (c_int, [c_int] * 6 + [_P, c_size_t]),
    "dba_ba_poll_eta_error": (c_int, [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "dba_ba_poll_eta_error_ws": (c_int, [c_int] * 6 + [_P, c_size_t, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "dba_ba_gather_edges": (c_int, [_P] * 4 + [c_int, _P, c_int] + [_P] * 4 + [c_int] * 3 + [_P] * 5),
    "dba_ba_linearize": (c_int, [_P] * 7 + [c_int] + [_P] * 3 + [c_int] * 6 + [c_float, _P, c_size_t, _P]),
    "dba_ba_reduce": (c_int, [_P] * 3 + [c_int] * 7 + [_P, c_size_t, _P]),
    "dba_ba_schur_select": (c_int, [c_int]),
    "dba_ba_schur_select_thread": (c_int, [c_int]),
    "dba_ba_schur_auto_form": (c_int, [c_int, c_int]),
    "dba_ba_schur_thread_form": (c_int, []),
    "dba_ba_schur_generation": (c_int, []),
    "dba_ba_schur_sparse_select": (c_int, [c_int]),
    "dba_ba_pairs_table": (c_int, [c_int] * 6 + [ctypes.POINTER(c_size_t), ctypes.POINTER(c_int)]),
    "dba_ba_set_deterministic": (c_int, [c_int]),
    "dba_ba_set_solve_check": (c_int, [c_int]),
    "dba_ba_solve_check": (c_int, [c_int] * 6 + [c_float, c_float, _P, c_size_t, _P]),
    "dba_ba_symmetrize": (c_int, [c_int] * 6 + [_P, c_size_t, _P]),
    "dba_ba_solve": (c_int, [c_int] * 6 + [c_float, c_float, _P, c_size_t, _P]),
    "dba_ba_solve_skyline": (c_int, [c_int] * 6 + [c_float, c_float, _P, _P, c_size_t, _P]),
    "dba_ba_update": (c_int, [_P] * 5 + [c_int] * 8 + [_P, _P, c_size_t, _P]),
    "dba_ba_shard_front": (c_int, [_P] * 7 + [c_int] + [_P] * 3 + [c_int] * 6 + [c_float, c_int, _P, c_size_t, _P]),
    "dba_ba_shard_back": (c_int, [_P] * 5 + [c_int] * 6 + [c_float, c_float, c_int, _P, c_int, _P, c_size_t, _P]),
    "dba_comm_unique_id": (c_int, [_P]),
    "dba_comm_create": (c_int, [_P, c_int, c_int, ctypes.POINTER(_P)]),
    "dba_comm_destroy": (c_int, [_P]),
    "dba_comm_info": (c_int, [_P, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "dba_comm_allreduce_f64": (c_int, [_P, c_size_t, _P]),
    "dba_ba_sharded_run": (c_int, [_P] * 7 + [c_int] + [_P] * 3 + [c_int] * 7 + [c_float, c_float, c_float, c_int, _P, c_int,
                                                                                  c_int, ctypes.POINTER(ShardExchange), _P,
                                                                                  c_size_t, _P]),
    "dba_ba": (c_int, [_P] * 7 + [c_int] + [_P, _P] + [c_int] * 7 + [c_float, c_float, c_int, _P, _P, _P,
                                                                     c_size_t, _P]),
    "dba_ba_prepared": (c_int, [_P] * 7 + [c_int] + [_P, _P] + [c_int] * 7 + [c_float, c_float, c_int, _P, _P, _P,
                                                                              c_size_t, _P, c_int]),
    "dba_ba_run": (c_int, [_P] * 7 + [c_int] + [_P, _P] + [c_int] * 7 + [c_float, c_float, c_int, _P, _P, _P,
                                                                         c_size_t, _P, c_int, c_int, c_float]),
    "dba_bacore_hessian": (c_int, [_P] * 7 + [c_int] + [_P, _P] + [c_int] * 6 + [_P, _P, _P, c_size_t, _P]),
    "dba_bacore_hessian_run": (c_int, [_P] * 7 + [c_int] + [_P, _P] + [c_int] * 6 + [_P, _P, _P, c_size_t, _P, c_int]),
    "dba_bacore_staging": (c_int, [c_int] * 6 + [_P, c_size_t, ctypes.POINTER(ctypes.c_void_p)]),
    "dba_bacore_export_host": (c_int, [c_int] * 6 + [_P, c_size_t, _P, c_int, _P, ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)]),
    "dba_bacore_hessian_host": (c_int, [_P] * 7 + [c_int] + [_P, _P] + [c_int] * 6 + [_P, c_size_t, _P, c_int, c_int, _P,
                                        ctypes.c_double, ctypes.POINTER(ctypes.c_void_p)]),
    "dba_bacore_retract": (c_int, [_P] * 4 + [c_int] * 6 + [_P, _P, _P, _P, c_size_t, _P]),
    "dba_bacore_optimize": (c_int, [_P, _P] + [c_int] * 6 + [c_float, c_float, _P, _P, c_size_t, _P]),
    "dba_ba_depth_variance_scratch_bytes": (c_size_t, [c_int]),
    "dba_ba_depth_variance": (c_int, [c_int] * 6 + [c_float, c_float, _P, c_int, _P, c_size_t, _P, c_size_t, _P]),
    "dba_ba_depth_variance_parts": (c_int, [c_int] * 6 + [c_float, c_float, _P, c_int, _P, c_size_t, _P, c_size_t, _P, c_int]),
    "dba_ba_pose_covariance": (c_int, [_P] + [c_int] * 6 + [c_float, c_float, _P, c_int, _P, c_int, _P, _P, c_int, _P, c_int,
                                       _P, c_size_t, _P, c_size_t, _P]),
    "dba_bacore_retract_device": (c_int, [_P] * 4 + [c_int] * 6 + [_P, _P, _P, _P, _P, c_size_t, _P]),
    "dba_inertial_scratch_bytes": (c_size_t, [c_int]),
    "dba_inertial_linearize": (c_int, [ctypes.POINTER(InertialState), c_int, _P, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "dba_inertial_step": (c_int, [ctypes.POINTER(InertialState), c_int, _P, c_int, _P, ctypes.c_double, c_float, c_float,
                                  _P, _P, _P, _P] + [c_int] * 6 + [_P, _P, _P, c_size_t, _P, c_size_t, _P]),
    "dba_inertial_marg_scratch_bytes": (c_size_t, [c_int]),
    "dba_inertial_marginalize": (c_int, [ctypes.POINTER(InertialState), c_int, _P, c_int, _P, ctypes.c_double] + [c_int] * 7 +
                                 [_P, c_size_t, _P, c_int, _P, c_int, _P, _P, _P, _P, c_int, _P, _P, c_size_t, _P]),
    "dba_ba_cost_scratch_bytes": (c_size_t, [c_int] * 3),
    "dba_ba_cost": (c_int, [_P] * 7 + [c_int] * 4 + [_P, c_int, _P, c_size_t, _P]),
    "dba_corr_index_forward": (c_int, [_P, _P, _P] + [c_int] * 7 + [_P]),
    "dba_corr_lookup_pyramid": (c_int, [_P, _P, _P] + [c_int] * 8 + [_P]),
    "dba_corr_volume_build_sheared_supported": (c_int, [c_int] * 6),
    "dba_corr_volume_build_route": (c_int, [c_int] * 6),
    "dba_corr_volume_build_sheared": (c_int, [_P, _P, _P] + [c_int] * 7 + [_P, c_size_t, _P]),
    "dba_corr_sheared_plane_elems": (c_int, [c_int, c_int]),
    "dba_corr_sheared_tiled": (c_int, [c_int, c_int]),
    "dba_corr_sheared_grid": (c_int, [c_int, c_int, _P, _P]),
    "dba_corr_lookup_select": (c_int, [c_int]),
    "dba_corr_lookup_arm_timing": (c_int, [_P, _P]),
    "dba_corr_shear_level": (c_int, [_P, _P] + [c_int] * 6 + [_P]),
    "dba_corr_lookup_pyramid_sheared": (c_int, [_P, _P, _P] + [c_int] * 7 + [_P]),
    "dba_corr_lookup_level_sheared": (c_int, [_P, _P, _P] + [c_int] * 7 + [_P]),
    "dba_corr_lookup_level_sheared_slots": (c_int, [_P, _P, _P, _P] + [c_int] * 7 + [_P]),
    "dba_corr_shear_level_slots": (c_int, [_P, _P, _P, _P] + [c_int] * 6 + [_P]),
    "dba_corr_volume_build_sheared_slots": (c_int, [_P, _P, _P, _P] + [c_int] * 7 + [_P, c_size_t, _P]),
    "dba_corr_lookup_pyramid_sheared_slots": (c_int, [_P, _P, _P, _P] + [c_int] * 7 + [_P]),
    "dba_corr_lookup_pyramid_slots": (c_int, [_P, _P, _P, _P] + [c_int] * 8 + [_P]),
    "dba_corr_lookup_reproject_sheared": (c_int, [_P] * 10 + [c_int] * 7 + [_P]),
    "dba_corr_lookup_reproject_motion_sheared": (c_int, [_P] * 12 + [c_int] * 7 + [_P]),
    "dba_corr_index_backward": (c_int, [_P, _P, _P] + [c_int] * 6 + [_P]),
    "dba_corr_volume_scratch_bytes": (c_size_t, [c_int] * 6),
    "dba_corr_once_pyramid_bytes": (c_size_t, [c_int] * 6),
    "dba_corr_build_lookup_once_sheared": (c_int, [_P, _P, _P, _P, _P, c_size_t, _P, c_size_t] + [c_int] * 8 + [_P]),
    "dba_corr_volume_build": (c_int, [_P, _P, _P] + [c_int] * 7 + [_P, c_size_t, _P]),
    "dba_altcorr_forward": (c_int, [_P] * 4 + [c_int] * 8 + [_P]),
    "dba_altcorr_forward_t": (c_int, [_P] * 4 + [c_int] * 9 + [_P]),
    "dba_altcorr_pyramid_forward": (c_int, [_P] * 6 + [c_int] * 8 + [_P]),
    "dba_altcorr_pyramid_forward_f16maps": (c_int, [_P] * 6 + [c_int] * 7 + [_P]),
    "dba_altcorr_backward": (c_int, [_P] * 6 + [c_int] * 8 + [_P]),
    "dba_reproject": (c_int, [_P] * 5 + [c_int] * 3 + [_P, _P, _P]),
    "dba_frame_distance": (c_int, [_P] * 5 + [c_int] * 3 + [c_float, _P, _P]),
    "dba_projmap": (c_int, [_P] * 5 + [c_int] * 3 + [_P, _P, _P]),
    "dba_iproj": (c_int, [_P] * 3 + [c_int] * 3 + [_P, _P]),
    "dba_depth_filter": (c_int, [_P] * 5 + [c_int] * 4 + [_P, _P]),
    "dba_peer_exchange_bytes": (c_size_t, [c_size_t]),
    "dba_peer_exchange_create": (c_int, [c_size_t, ctypes.POINTER(_P), _P]),
    "dba_peer_exchange_open": (c_int, [_P, ctypes.POINTER(_P)]),
    "dba_peer_exchange_close": (c_int, [_P, c_int]),
    "dba_peer_allreduce_f64": (c_int, [_P, c_size_t, _P, c_int, c_int, ctypes.c_uint, c_size_t, _P, _P]),
    "dba_cvx_upsample_disp": (c_int, [_P, c_int, _P, _P] + [c_int] * 4 + [_P, c_int, _P, _P]),
    "dba_segment_reduce": (c_int, [_P, c_int, _P, c_int, ctypes.c_int64, ctypes.c_int64, c_int, c_int, _P, _P]),
    "dba_upmask_upsample_disp": (c_int, [_P] * 4 + [c_int, _P] + [c_int] * 3 + [_P, c_int, _P, _P, _P]),
    "dba_frame_plan_max_rows": (c_int, []),
    "dba_frame_plan": (c_int, [_P] + [c_int] * 3 + [_P, _P, _P, c_int, _P]),
    "dba_frame_plan_poll": (c_int, [ctypes.POINTER(c_int)]),
    "dba_frame_distance_bidir": (c_int, [_P] * 5 + [c_int] * 4 + [c_float, _P, _P]),
    "dba_proximity_edges_capacity": (c_int, [c_int] * 5),
    "dba_proximity_edges": (c_int, [_P] * 3 + [c_int] * 7 + [c_float, ctypes.c_double, c_int, c_int, _P, c_int, c_int]
                            + [_P, _P, c_int, _P, _P, c_int, _P, _P]),
    "dba_filter_repeated_edges": (c_int, [_P, _P, c_int, _P, _P, c_int, _P, _P, _P, _P]),
    "dba_select_edges": (c_int, [_P, _P, _P, c_int, c_int, _P, ctypes.c_int64, ctypes.c_int64, _P, _P, c_int, _P, _P, _P,
                                 _P]),
    "dba_move_rows": (c_int, [ctypes.POINTER(RowJob), c_int, _P]),
    "dba_shift_rows": (c_int, [ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), c_int,
                               ctypes.c_int64, _P]),
    "dba_roll_rows": (c_int, [ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), c_int,
                              ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), c_int, _P]),
    "dba_add_factors_plan": (c_int, [_P, _P, _P, c_int, _P, _P, c_int, _P, _P, c_int] + [c_int] * 4 + [_P, _P, _P, _P]),
    "dba_add_factors_payload": (c_int, [ctypes.POINTER(AfJob), c_int, ctypes.POINTER(AfGeometry), _P]),
    "dba_update_inputs_edges": (c_int, [_P, _P, c_int, _P, _P, c_int, _P, c_int, c_int, ctypes.c_int64, ctypes.c_int64,
                                        c_float, c_int] + [_P] * 7),
    "dba_update_inputs_payload": (c_int, [_P, _P, c_int, _P, _P, c_int, _P, _P, c_int, c_int, c_int, c_float, c_int,
                                          c_float] + [_P] * 5 + [c_int] * 3 + [_P] * 4),
    "dba_update_inputs_payload_op": (c_int, [_P, _P, c_int, _P, _P, _P, c_int, c_int, _P, _P, c_int, c_int, c_int, c_float,
                                             c_int, c_float] + [_P] * 5 + [c_int] * 3 + [_P] * 6),
    "dba_update_inputs_poll": (c_int, [ctypes.POINTER(c_int)]),
    "dba_vio_window_plan": (c_int, [_P, _P, c_int] + [ctypes.c_int64] * 3 + [_P, _P, c_int, ctypes.c_int64] + [_P] * 8),
    "dba_vio_window_payload": (c_int, [ctypes.POINTER(RowJob), c_int, _P, ctypes.POINTER(c_int), _P]),
    "dba_vio_window_poll": (c_int, [ctypes.POINTER(c_int)]),
    "dba_keyframe_report_words": (c_int, []),
    "dba_keyframe_report": (c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(c_int)]),
    "dba_keyframe_check": (c_int, [_P] * 3 + [c_int] * 4 + [c_float, _P, c_int, _P]),
    "dba_keyframe_flow_magnitude": (c_int, [_P, c_int, c_int, _P, c_int, _P]),
    "dba_keyframe_wait": (c_int, [_P, c_int]),
    "dba_gru_pack": (c_int, [ctypes.POINTER(_P), ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, _P, _P]),
    "dba_gru_pack_relu": (c_int, [ctypes.POINTER(_P), ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, _P, ctypes.c_uint, _P]),
    "dba_gru_context": (c_int, [_P, _P] + [c_int] * 4 + [_P, _P]),
    "dba_gru_reset": (c_int, [_P, c_int, _P, _P, _P] + [c_int] * 4 + [_P]),
    "dba_gru_blend": (c_int, [_P] * 5 + [c_int] * 4 + [_P, _P]),
    "dba_conv3x3_tile": (c_int, []),
    "dba_conv3x3_f16": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, _P] + [c_int] * 5 + [_P, _P]),
    "dba_conv3x3_gates_f16": (c_int, [_P, c_int, _P, c_int, c_int, c_int] + [_P] * 5 + [c_int] * 4 + [_P, _P, _P]),
    "dba_conv3x3_blend_f16": (c_int, [_P, c_int, _P, c_int, c_int, c_int] + [_P] * 5 + [c_int] * 4 + [_P, _P]),
    "dba_conv3x3_pair_f16": (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, _P] + [c_int] * 5 + [_P, _P, _P]),
    "dba_frame_members_max_slots": (c_int, []),
    "dba_frame_members": (c_int, [_P, c_int, c_int, _P, _P, _P]),
    "dba_conv3x3_mean_f16": (c_int, [_P, c_int, _P, _P] + [c_int] * 4 + [_P, _P, c_int, _P, c_int, _P]),
    "dba_conv1x1_tile": (c_int, []),
    "dba_conv1x1_f16": (c_int, [_P, c_int, _P, _P] + [c_int] * 4 + [_P, _P]),
    "dba_conv1x1_context_workspace_bytes": (c_size_t, [c_int] * 3),
    "dba_conv1x1_context_f16": (c_int, [_P] * 5 + [c_int] * 3 + [_P, c_size_t] + [_P] * 5),
    "dba_conv7x7_tile": (c_int, []),
    "dba_conv7x7_f16": (c_int, [_P, c_int, _P, _P] + [c_int] * 5 + [_P, _P]),
    "dba_conv3x3s_tile_rows": (c_int, [c_int]),
    "dba_conv3x3s_tile_cols": (c_int, []),
    "dba_conv7x7s2_tile": (c_int, []),
    "dba_conv3x3s_f16": (c_int, [_P, _P, _P] + [c_int] * 7 + [_P, _P]),
    "dba_conv3x3s_down_f16": (c_int, [_P] * 4 + [c_int] * 6 + [_P, _P, _P]),
    "dba_conv7x7s2_f16": (c_int, [_P, c_int, _P, _P] + [c_int] * 5 + [_P, _P]),
    "dba_enc_norm": (c_int, [_P, c_int, c_int, c_float, c_int, c_int, _P, _P, _P]),
    "dba_enc_norm_skip": (c_int, [_P, _P, _P, c_int, c_int, c_float, c_int, _P, _P, _P, _P]),
    "dba_enc_relu_skip": (c_int, [_P, _P, ctypes.c_longlong, c_int, _P, _P]),
    "dba_enc_image": (c_int, [_P] + [c_int] * 5 + [_P, _P]),
    "dba_enc_context_split": (c_int, [_P] + [c_int] * 5 + [_P, _P, _P]),
    "dba_upd_heads": (c_int, [ctypes.POINTER(UpdHead)] + [c_int] * 6 + [_P]),
    "dba_upd_heads_tile": (c_int, [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "dba_archive_frames": (c_int, [_P] * 10 + [c_int] * 9 + [ctypes.c_int64, _P]),
    "dba_map_plan": (c_int, [_P] * 3 + [c_int] * 5 + [_P] * 9 + [ctypes.POINTER(c_int), _P]),
    "dba_map_payload": (c_int, [_P] * 6 + [c_int] * 4 + [ctypes.c_int64, _P, _P, _P]),
    "dba_frame_append": (c_int, [ctypes.POINTER(FrameItem), _P]),
    "dba_frame_seed_next": (c_int, [_P, _P, _P] + [c_int] * 6 + [_P, ctypes.c_int64, _P]),
    "dba_world_poses": (c_int, [_P, c_int, c_int, _P, _P]),
    "dba_set_world_poses": (c_int, [_P, _P, c_int, c_int, ctypes.c_int64, c_int, c_int, _P, c_float, ctypes.POINTER(c_int),
                                    _P]),
}

_lib = None


def load():
    """dlopen the HIP library and type every entry point. Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "dba_hip: %s not found -- build it with `make lib` (hipcc --offload-arch=gfx950); "
                "there is no CPU fallback for the DBA hot path" % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def schur_generation():
    """what decides which Schur form (and therefore which stage-0 tables) is in force besides the graph itself: the
    process-wide selection's generation and the calling thread's pin"""
    lib = load()
    return (lib.dba_ba_schur_generation(), lib.dba_ba_schur_thread_form())


def check(rc, what):
    if rc != 0:
        msg = _ERR.get(rc, str(rc))
        detail = load().dba_last_error().decode() if rc == -3 else ""
        raise RuntimeError("dba_hip: %s failed with %s %s" % (what, msg, detail))


# ---- what every ctypes caller of the edge-management entry points needs (factors, proximity, update_inputs, vio_window) ----

def ptr(x):
    """the tensor's address as a void*; a null pointer for None and for an empty tensor"""
    return ctypes.c_void_p(x.data_ptr()) if x is not None and x.numel() else None


def require(cond, op, msg):
    if not cond:
        raise ValueError("%s (MI355X): %s" % (op, msg))


def stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def check_edge_list(op, dev, x, nm):
    """x must be a contiguous 1-D int64 device tensor, on `dev` unless that is None"""
    require(isinstance(x, torch.Tensor) and x.is_cuda and (dev is None or x.device == dev), op,
            "%s must be a HIP device tensor%s; no CPU path" % (nm, "" if dev is None else " on %s" % dev))
    require(x.dtype == torch.int64 and x.dim() == 1 and x.is_contiguous(), op,
            "%s must be a contiguous 1-D int64 tensor" % nm)


def dev_tensor(op, x, nm, dev, dtype, aligned=False):
    """x must be a contiguous device tensor of `dtype`, on `dev` unless that is None; aligned: at a 16-byte boundary"""
    require(isinstance(x, torch.Tensor) and x.is_cuda and (dev is None or x.device == dev), op,
            "%s must be a HIP device tensor%s; no CPU path" % (nm, "" if dev is None else " on %s" % dev))
    require(x.dtype == dtype, op, "%s must be %s, got %s" % (nm, dtype, x.dtype))
    require(x.is_contiguous(), op, "%s must be contiguous" % nm)
    require(not aligned or x.data_ptr() % 16 == 0, op, "%s must be 16-byte aligned" % nm)


def edge_list(op, x, nm, dev, max_edges, aligned=False):
    """dev_tensor for a 1-D int64 list of at most max_edges entries (update_inputs, vio_window; factors and proximity
    keep check_edge_list, whose message texts are other ones)"""
    dev_tensor(op, x, nm, dev, torch.int64, aligned)
    require(x.dim() == 1, op, "%s must be 1-D, got %s" % (nm, tuple(x.shape)))
    require(x.shape[0] <= max_edges, op, "%s: %d edges exceed the supported %d" % (nm, x.shape[0], max_edges))


class EdgeSetMemo:
    """What the first call on an edge set read from the device, for the later calls that read nothing.
    An edge set is the identity of its list tensors (held weakly), their in-place versions and a key of host scalars.
    The newest `capacity` sets are kept.  One instance per module: a report of the size guard clears its module's alone."""

    def __init__(self, capacity=8):
        self.capacity = capacity
        self._entries = []   # (((weakref, _version), ...), key, value), newest last

    def __len__(self):
        return len(self._entries)

    def lookup(self, lists, key):
        """the value remembered for these tensor objects at these versions under `key` (the newest such), or None"""
        for refs, k, value in reversed(self._entries):
            if k == key and len(refs) == len(lists) and all(r() is x and v == x._version for (r, v), x in zip(refs, lists)):
                return value
        return None

    def remember(self, lists, key, value):
        live = [e for e in self._entries if all(r() is not None for r, _ in e[0])]
        self._entries = live[max(0, len(live) - (self.capacity - 1)):]   # dead sets go, then all but the newest
        self._entries.append((tuple((weakref.ref(x), x._version) for x in lists), key, value))

    def clear(self):
        del self._entries[:]
