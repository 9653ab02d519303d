"""ctypes binding of libdspgn.so (the C ABI in include/dsp_gn.h).

No fallback: if the library is missing or a call fails this raises -- the product path never runs on
the CPU oracle or on PyTorch ops.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

c_f32p = C.POINTER(C.c_float)
c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_f64p = C.POINTER(C.c_double)

CODE_LEN = 64
GRAD_DIM = 67

OBJ_GOOD, OBJ_FEW_SAMPLES, OBJ_NAN = 0, 1, 2
PREPASS_OFF, PREPASS_F16, PREPASS_BF16 = 0, 1, 2
MESH_REGULAR_GRID, MESH_PREPASS_F16, MESH_PREPASS_BF16 = 1, 2, 4     # dsp_extract_mesh(es) flags
QUERY_NORMALS = 1                                                    # dsp_map_query flags
RAYCAST_NORMALS = 1                                                  # dsp_map_raycast flags
RAYCAST_MISS, RAYCAST_HIT, RAYCAST_UNDECIDED = 0, 1, 2               # ... a ray's status
ALIGN_OK, ALIGN_CONVERGED, ALIGN_NO_SUPPORT, ALIGN_SINGULAR = 0, 1, 2, 3      # dsp_map_align: a hypothesis' status
ALIGN_RECORD, ALIGN_TRACE = 50, 53                                   # ... doubles per record / per traced evaluation
SHAPES_CODE, SHAPES_POSE, SHAPES_DIM = 1, 2, 70                      # dsp_map_align_shapes: the unknowns asked for, unknowns per object
SHAPES_RECORD, SHAPES_TRACE, SHAPES_NSUM = 8 + 70 * 70 + 70, 16 + 64 + 4 + 70, 2558
PREPASS_SMALL_TILES = 0x100
COMPUTE_F32, COMPUTE_F16, COMPUTE_BF16 = 0, 1, 2
POSTERIOR_MEAN, POSTERIOR_SUM = 0, 1                       # dsp_batch_posterior: weights
POSTERIOR_OK, POSTERIOR_NONE, POSTERIOR_SINGULAR = 0, 1, 2     # ... the record's status
# keys of dsp_batch_set_debug (include/dsp_gn.h: DSP_DBG_*)
(DBG_MASK_REUSE, DBG_SPLIT_ROWS, DBG_TAIL_SPLIT, DBG_WAVE_BOOKKEEPING, DBG_SPECULATIVE_BAND, DBG_MIXED_REUSE, DBG_CLUSTER_TILES, DBG_DIRECT_TILES,
 DBG_PREPASS_TILE, DBG_PREPASS_AUDIT, DBG_CLUSTER_FAULT, DBG_LP_SMALL_BATCHES) = range(1, 13)
ABI_VERSION = 6


class DecoderDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("code_len", C.c_int32), ("latent_in", C.c_int32),
                ("out_dims", c_i32p), ("in_dims", c_i32p),
                ("weights", C.POINTER(c_f32p)), ("biases", C.POINTER(c_f32p))]


class GnParams(C.Structure):
    _fields_ = [("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float), ("k4", C.c_float),
                ("b1", C.c_float), ("b2", C.c_float), ("lr", C.c_float), ("s_damp", C.c_float),
                ("num_iterations", C.c_int32), ("num_depth_samples", C.c_int32), ("cut_off", C.c_float),
                ("pose_only_iterations", C.c_int32)]


class AlignParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("min_points", C.c_int32), ("max_dist", C.c_double), ("huber", C.c_double), ("damp", C.c_double),
                ("trans_tol", C.c_double), ("rot_tol", C.c_double),
                ("lambda0", C.c_double), ("up", C.c_double), ("down", C.c_double), ("lambda_min", C.c_double), ("lambda_max", C.c_double)]


class ShapesParams(C.Structure):
    _fields_ = [("unknowns", C.c_int32), ("code_reg", C.c_double), ("code_anchor", C.c_double), ("code_tol", C.c_double)]


class RaycastParams(C.Structure):
    _fields_ = [("t_min", C.c_float), ("t_max", C.c_float), ("eps", C.c_float), ("relax", C.c_float), ("max_steps", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("n_fwd_points", C.c_double), ("n_jac_points", C.c_double), ("ms_total", C.c_double),
                ("ms_mlp_fwd", C.c_double), ("ms_mlp_jac", C.c_double),
                ("n_mlp_fwd_launches", C.c_int32), ("n_mlp_jac_launches", C.c_int32), ("n_insphere_points", C.c_double), ("n_render_rows", C.c_double),
                ("n_prepass_points", C.c_double), ("ms_mlp_prepass", C.c_double), ("n_mlp_prepass_launches", C.c_int32),
                ("prepass_mode", C.c_int32), ("prepass_delta", C.c_float), ("prepass_max_err", C.c_float),
                ("prepass_misclassified", C.c_double), ("prepass_audited", C.c_double),
                ("prepass_guard_trips", C.c_double), ("prepass_guard_objects", C.c_double), ("prepass_guard_max_err", C.c_float),
                ("prepass_guard_rerun", C.c_int32), ("n_cluster_tiles", C.c_double), ("cluster_fallback", C.c_int32), ("cluster_cooldown", C.c_int32)]


class DspError(RuntimeError):
    pass


_lib = None

# every symbol include/dsp_gn.h declares: (name, restype, argtypes)
_VP = C.c_void_p
SYMBOLS = [
    ("dsp_abi_version", C.c_int, []),
    ("dsp_device_count", C.c_int, []),
    ("dsp_build_info", C.c_char_p, []),
    ("dsp_runtime_versions", C.c_int, [c_i32p, c_i32p]),
    ("dsp_create", C.c_int, [C.POINTER(DecoderDesc), C.c_int, C.POINTER(_VP)]),
    ("dsp_destroy", None, [_VP]),
    ("dsp_last_error", C.c_char_p, [_VP]),
    ("dsp_decode_sdf", C.c_int, [_VP, c_f32p, c_f32p, C.c_int64, c_f32p]),
    ("dsp_decode_sdf_multi", C.c_int, [_VP, c_f32p, C.c_int64, c_f32p, C.c_int64, c_f32p]),
    ("dsp_decode_sdf_prepass", C.c_int, [_VP, C.c_int, c_f32p, c_f32p, C.c_int64, c_f32p]),
    ("dsp_debug_pack_prepass", C.c_int, [C.POINTER(DecoderDesc), C.c_int, C.POINTER(C.c_uint16), c_i64p, c_i32p, c_i32p]),
    ("dsp_debug_pack_lpj", C.c_int, [C.POINTER(DecoderDesc), C.c_int, C.POINTER(C.c_uint16), c_i64p, c_i32p, c_i32p]),
    ("dsp_sdf_jacobian", C.c_int, [_VP, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p]),
    ("dsp_compute_sdf_loss", C.c_int, [_VP, c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p]),
    ("dsp_compute_render_loss", C.c_int, [_VP, c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, C.c_int32, c_f32p, C.c_float,
                                          c_i64p, c_f32p, c_f32p, c_f32p, c_i64p, c_i64p]),
    ("dsp_reconstruct_batch", C.c_int, [_VP, C.POINTER(GnParams), C.c_int32, c_i64p, c_f32p, c_i64p, c_f32p, c_i64p, c_f32p,
                                        c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i32p]),
    ("dsp_estimate_pose_batch", C.c_int, [_VP, C.POINTER(GnParams), C.c_int32, c_i64p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p]),
    ("dsp_batch_create", C.c_int, [_VP, C.POINTER(GnParams), C.c_int32, c_i64p, c_f32p, c_i64p, c_f32p, c_i64p, c_f32p,
                                   c_f32p, c_f32p, C.POINTER(_VP)]),
    ("dsp_batch_create_pose", C.c_int, [_VP, C.POINTER(GnParams), C.c_int32, c_i64p, c_f32p, c_f32p, c_f32p, c_f32p, C.POINTER(_VP)]),
    ("dsp_batch_run", C.c_int, [_VP]),
    ("dsp_batch_results", C.c_int, [_VP, c_f32p, c_f32p, c_f32p, c_i32p]),
    ("dsp_batch_stats", C.c_int, [_VP, C.POINTER(Stats)]),
    ("dsp_batch_set_ray_passes", C.c_int, [_VP, C.c_int]),
    ("dsp_batch_set_prepass", C.c_int, [_VP, C.c_int, C.c_float]),
    ("dsp_batch_set_prepass_guard", C.c_int, [_VP, C.c_int]),
    ("dsp_batch_set_kernel_timing", C.c_int, [_VP, C.c_int]),
    ("dsp_batch_set_iterations", C.c_int, [_VP, C.c_int32]),
    ("dsp_batch_set_compute", C.c_int, [_VP, C.c_int]),
    ("dsp_batch_convergence", C.c_int, [_VP, C.c_float, C.c_float, C.c_int32]),
    ("dsp_batch_iterations_used", C.c_int, [_VP, c_i32p]),
    ("dsp_batch_posterior", C.c_int, [_VP, C.c_int, C.c_int]),
    ("dsp_batch_posterior_fetch", C.c_int, [_VP, c_i32p, c_f64p, c_f64p, c_f64p, c_f32p, c_i64p, c_i64p, c_i64p, c_f64p, c_f64p, c_f32p, c_f32p, c_f32p]),
    ("dsp_batch_prior", C.c_int, [_VP, c_f32p, c_f32p, c_f64p]),
    ("dsp_batch_prior_fetch", C.c_int, [_VP, c_f64p, c_f64p]),
    ("dsp_debug_prior_check", C.c_int, [C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_f64p]),
    ("dsp_debug_prior_terms", C.c_int, [C.c_int, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p, c_f64p, c_f64p, c_f64p, c_f64p]),
    ("dsp_batch_step_control", C.c_int, [_VP, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    ("dsp_batch_step_log", C.c_int, [_VP, C.POINTER(C.c_int32), c_f64p, c_f64p]),
    ("dsp_debug_step_rule", C.c_int, [C.c_int32, c_f64p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int32), c_f64p]),
    ("dsp_batch_report", C.c_int, [_VP, C.c_int]),
    ("dsp_batch_report_sizes", C.c_int, [_VP, c_i64p, c_i64p, c_i64p]),
    ("dsp_batch_report_fetch", C.c_int, [_VP, c_f32p, C.POINTER(C.c_uint8), c_f32p, c_f32p, c_f32p, c_i32p, c_f64p]),
    ("dsp_debug_report_ray", C.c_int, [C.c_int32, c_f32p, c_f32p, C.c_float, C.c_float, C.c_int, c_f32p, c_i32p]),
    ("dsp_batch_observation_weights", C.c_int, [_VP, c_f32p, c_f32p]),
    ("dsp_debug_observation_weights_check", C.c_int, [C.c_int64, C.c_int64, c_f32p, c_f32p]),
    ("dsp_batch_unknowns", C.c_int, [_VP, C.POINTER(C.c_uint8)]),
    ("dsp_debug_unknowns_check", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    ("dsp_sdf_jacobian_lp", C.c_int, [_VP, C.c_int, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p]),
    ("dsp_batch_set_debug", C.c_int, [_VP, C.c_int, C.c_int]),
    ("dsp_prepass_calibration", C.c_int, [_VP, C.c_int, c_f32p, c_f32p]),
    ("dsp_prepass_calibration_table", C.c_int, [_VP, C.c_int, c_f32p, c_f32p, c_f32p, c_f32p]),
    ("dsp_batch_debug_ray_pass_bounds", C.c_int, [_VP, c_i32p, C.c_int]),
    ("dsp_batch_debug_start_state", C.c_int, [_VP, c_f32p, c_f32p, c_f32p]),
    ("dsp_batch_debug_depth_schedule", C.c_int, [_VP, c_f32p, C.c_int32]),
    ("dsp_batch_debug_samples", C.c_int, [_VP, C.c_int32, C.POINTER(C.c_uint64), c_f32p, c_f32p, C.c_int64]),
    ("dsp_debug_fail_alloc", C.c_int, [_VP, C.c_int]),
    ("dsp_prepass_reset_guard", C.c_int, [_VP]),
    ("dsp_trim", C.c_int, [_VP]),
    ("dsp_set_stream_priority", C.c_int, [_VP, C.c_int]),
    ("dsp_debug_lie", C.c_int, [_VP, C.c_int, c_f32p, C.c_int32, c_f32p]),
    ("dsp_batch_enable_trace", C.c_int, [_VP, C.c_int]),
    ("dsp_batch_trace", C.c_int, [_VP, C.c_int32, c_f32p, c_f32p, c_f32p, c_i64p, c_i64p, c_i64p, c_f32p, c_f32p, C.POINTER(C.c_uint32), c_f32p]),
    ("dsp_reconstruct_multiview", C.c_int, [_VP, C.POINTER(GnParams), C.c_int32, c_i64p, c_f32p, c_i64p, c_f32p, c_i64p, c_f32p, c_i64p, c_f32p,
                                            c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i32p]),
    ("dsp_batch_create_multiview", C.c_int, [_VP, C.POINTER(GnParams), C.c_int32, c_i64p, c_f32p, c_i64p, c_f32p, c_i64p, c_f32p, c_i64p, c_f32p,
                                             c_f32p, c_f32p, C.POINTER(_VP)]),
    ("dsp_batch_trace_views", C.c_int, [_VP, C.c_int32, c_i64p, c_i64p, c_i64p, c_f32p, C.POINTER(C.c_uint32), c_f32p]),
    ("dsp_batch_destroy", None, [_VP]),
    ("dsp_pack_results", None, [C.c_int32, c_f32p, c_f32p, c_f32p, c_i32p, c_f32p]),
    ("dsp_gather_results", C.c_int, [C.POINTER(_VP), C.c_int32, C.POINTER(c_f32p), c_i32p, c_f32p]),
    ("dsp_gather_batch_results", C.c_int, [C.POINTER(_VP), C.c_int32, c_f32p]),
    ("dsp_batch_results_packed_dev", C.c_int, [_VP, C.c_void_p]),
    ("dsp_extract_mesh", C.c_int, [_VP, c_f32p, C.c_int32, C.c_int32, c_i64p, c_i64p]),
    ("dsp_marching_cubes", C.c_int, [_VP, c_f32p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, c_i64p, c_i64p]),
    ("dsp_mesh_fetch", C.c_int, [_VP, c_f32p, C.c_int64, c_i32p, C.c_int64]),
    ("dsp_extract_meshes", C.c_int, [_VP, c_f32p, C.c_int64, C.c_int32, C.c_int32, C.c_float, c_i64p, c_i64p]),
    ("dsp_meshes_fetch", C.c_int, [_VP, C.c_int64, c_i64p, c_i64p, c_f32p, c_i32p]),
    ("dsp_mesh_last_stats", C.c_int, [_VP, c_i64p, c_f32p]),
    ("dsp_surface_points", C.c_int, [_VP, c_f32p, C.c_int64, c_i64p, c_f32p, C.c_int32, C.c_float, c_f64p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p]),
    ("dsp_meshes_refine", C.c_int, [_VP, C.c_int64, c_i64p, C.c_int32, C.c_float, c_f64p]),
    ("dsp_meshes_fetch_attributes", C.c_int, [_VP, C.c_int64, c_i64p, c_f32p, c_f32p, c_f32p, c_f32p]),
    ("dsp_debug_surface_step", C.c_int, [C.c_int64, c_f32p, c_f32p, c_f32p, C.c_float, c_f32p]),
    ("dsp_debug_surface_attributes", C.c_int, [C.c_int64, c_f32p, c_f64p, c_f32p, c_f32p, c_f32p, c_f32p]),
    ("dsp_debug_surface_chunk_rows", C.c_int, [_VP, C.c_int64]),
    ("dsp_map_query", C.c_int, [_VP, c_f32p, c_f32p, C.c_int64, c_f32p, C.c_int64, C.c_int32, c_i32p, c_f32p, c_f32p, c_f32p]),
    ("dsp_map_query_last_stats", C.c_int, [_VP, c_i64p]),
    ("dsp_debug_query_invert", C.c_int, [C.c_int64, c_f32p, c_f32p, c_f32p]),
    ("dsp_debug_query_candidates", C.c_int, [C.c_int64, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p, C.POINTER(C.c_uint8), c_f32p]),
    ("dsp_debug_query_select", C.c_int, [C.c_int64, c_f32p, c_f32p, c_i32p, c_i32p, C.c_int64, c_i32p, c_f32p]),
    ("dsp_debug_query_chunk_rows", C.c_int, [_VP, C.c_int64]),
    ("dsp_debug_query_plan", C.c_int, [C.c_int64, c_i32p, C.c_int64, C.c_int64, c_i64p, c_i32p, c_i32p, c_i32p, c_i64p]),
    ("dsp_debug_query_timing", C.c_int, [_VP, C.c_int, c_f64p]),
    ("dsp_raycast_params_default", None, [C.POINTER(RaycastParams)]),
    ("dsp_map_raycast", C.c_int, [_VP, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, C.POINTER(RaycastParams), C.c_int32, c_i32p, c_f32p, c_f32p,
                                  c_i32p, c_f32p]),
    ("dsp_map_raycast_last_stats", C.c_int, [_VP, c_i64p]),
    ("dsp_debug_raycast_check", C.c_int, [C.POINTER(RaycastParams)]),
    ("dsp_debug_raycast_segments", C.c_int, [C.c_int64, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p, C.c_float, C.c_float, C.POINTER(C.c_uint8),
                                             C.POINTER(C.c_uint8), c_f32p, c_f32p, c_f32p, c_f32p]),
    ("dsp_debug_raycast_step", C.c_int, [C.c_int64, c_f32p, c_f32p, c_f32p, c_f32p, C.POINTER(RaycastParams), c_i32p, c_f32p, c_f32p]),
    ("dsp_align_params_default", None, [C.POINTER(AlignParams)]),
    ("dsp_map_align", C.c_int, [_VP, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p, C.c_int64, c_f64p, C.c_int64, C.POINTER(AlignParams), c_f64p, c_f64p,
                                c_i32p, c_f32p, c_f64p]),
    ("dsp_map_align_last_stats", C.c_int, [_VP, c_i64p]),
    ("dsp_debug_align_check", C.c_int, [C.POINTER(AlignParams), c_f64p, C.c_int64, c_f32p, C.c_int64]),
    ("dsp_debug_align_rows", C.c_int, [C.c_int64, c_f32p, c_i32p, c_f32p, c_f32p, c_f32p, C.c_double, C.c_double, c_f64p]),
    ("dsp_debug_align_step", C.c_int, [c_f64p, c_f64p, C.c_double, C.c_double, c_f64p, c_i32p, c_f64p, c_f64p]),
    ("dsp_align_rays_default_max_gap", C.c_double, [C.POINTER(AlignParams)]),
    ("dsp_map_align_rays", C.c_int, [_VP, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, C.c_int64, c_f64p, C.c_int64, C.POINTER(AlignParams),
                                     C.POINTER(RaycastParams), C.c_double, c_f64p, c_f64p, c_i32p, c_f32p, c_f32p, c_i32p, c_f64p]),
    ("dsp_map_align_rays_last_stats", C.c_int, [_VP, c_i64p]),
    ("dsp_debug_align_ray_rows", C.c_int, [C.c_int64, c_f32p, c_f32p, c_i32p, c_f32p, c_f32p, c_i32p, c_f32p, c_f32p, C.c_double, C.c_double, C.c_double,
                                           c_i32p, c_f32p, c_f64p]),
    ("dsp_debug_align_rays_check", C.c_int, [C.POINTER(AlignParams), C.POINTER(RaycastParams), C.c_double, c_f64p, C.c_int64, c_f32p, C.c_int64,
                                             C.c_int64]),
    ("dsp_map_align_objects", C.c_int, [_VP, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(AlignParams),
                                        C.POINTER(RaycastParams), C.c_double, c_f32p, c_f64p, c_f64p, c_i32p, c_f32p, c_f32p, c_i32p, c_f64p]),
    ("dsp_map_align_objects_last_stats", C.c_int, [_VP, c_i64p]),
    ("dsp_debug_align_objects_rows", C.c_int, [C.c_int64, c_f32p, c_i32p, c_i32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_double, C.c_double, c_f64p]),
    ("dsp_debug_align_objects_compose", C.c_int, [C.c_int64, c_f64p, c_f32p, c_f32p]),
    ("dsp_debug_align_objects_check", C.c_int, [C.POINTER(AlignParams), C.POINTER(RaycastParams), C.c_double, c_f32p, c_f32p, C.c_int64, C.c_int64]),
    ("dsp_shapes_params_default", None, [C.POINTER(AlignParams), C.POINTER(ShapesParams)]),
    ("dsp_map_align_shapes", C.c_int, [_VP, c_f32p, c_f32p, C.c_int64, c_f32p, c_f32p, c_f32p, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(AlignParams),
                                       C.POINTER(ShapesParams), C.POINTER(RaycastParams), C.c_double, c_f32p, c_f32p, c_f64p, c_f64p, c_i32p, c_f32p, c_f32p,
                                       c_i32p, c_f64p]),
    ("dsp_map_align_shapes_last_stats", C.c_int, [_VP, c_i64p]),
    ("dsp_debug_align_shapes_rows", C.c_int, [C.c_int64, c_f32p, c_i32p, c_i32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int64, C.c_double, C.c_double,
                                              c_f64p]),
    ("dsp_debug_align_shapes_step", C.c_int, [c_f64p, c_f64p, C.c_double, c_f64p, c_f32p, C.c_int32, C.POINTER(ShapesParams), C.c_double, C.c_double,
                                              c_f64p, c_i32p, c_f64p, c_f64p, c_f64p]),
    ("dsp_debug_align_shapes_check", C.c_int, [C.POINTER(AlignParams), C.POINTER(ShapesParams), C.POINTER(RaycastParams), C.c_double, c_f32p, c_f32p,
                                               C.c_int64, C.c_int64]),
    ("dsp_debug_split_layout", C.c_int, [C.POINTER(DecoderDesc), c_i32p, c_i32p, c_i64p]),
    ("dsp_debug_mc_table", C.c_int, [C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    ("dsp_debug_code_bias", C.c_int, [C.POINTER(DecoderDesc), c_f32p, c_f32p]),
    ("dsp_debug_pack", C.c_int, [C.POINTER(DecoderDesc), c_f32p, c_i64p, c_f32p, c_i64p, c_i32p, c_i32p, c_f32p]),
    # include/dsp_pose_graph.h (host fp64; no handle)
    ("dsp_pg_from_matrix", C.c_int, [C.c_int64, c_f64p, c_f64p]),
    ("dsp_pg_to_matrix", C.c_int, [C.c_int64, c_f64p, c_f64p]),
    ("dsp_pg_log", C.c_int, [C.c_int64, c_f64p, c_f64p]),
    ("dsp_pg_exp", C.c_int, [C.c_int64, c_f64p, c_f64p]),
    ("dsp_pg_edge_error", C.c_int, [C.c_int64, c_f64p, c_f64p, c_f64p, c_f64p]),
    ("dsp_pg_edge_linearize", C.c_int, [C.c_int64, c_f64p, c_f64p, c_f64p, c_f64p]),
    ("dsp_pg_edge_chi2", C.c_int, [C.c_int64, c_f64p, C.c_double, C.c_double, c_f64p, c_f64p, c_f64p]),
    ("dsp_pg_edge_information", C.c_int, [C.c_int64, C.c_int, c_f64p, c_f64p, C.c_double, c_f64p]),
    ("dsp_pg_edge_chi2_info", C.c_int, [C.c_int64, c_f64p, c_f64p, C.c_double, c_f64p, c_f64p, c_f64p]),
    ("dsp_pg_vertex_oplus", C.c_int, [C.c_int64, C.c_int, c_f64p, c_f64p, c_f64p]),
    # test hook, not in dsp_gn.h: the launch plan of one row of inputs, on the host (tests/test_launch_plan.py)
    ("dsp_debug_launch_plan", C.c_int, [c_i32p, C.c_int, c_i32p, C.c_int]),
]


def lib_path():
    return os.environ.get("DSPGN_LIB", _build.LIB_PATH)


def load():
    """Load libdspgn.so (building it first if hipcc is available and the .so is missing or stale)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if path == _build.LIB_PATH and _build.is_stale():
        try:
            _build.build_locked()     # one rank builds, the others wait on the lock file and find it fresh
        except Exception as e:  # stale-but-present is usable on a box without hipcc
            if not os.path.exists(path):
                raise DspError("libdspgn.so is not built and cannot be built here: %s" % e)
    lib = C.CDLL(path)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)       # AttributeError => the .so does not match include/dsp_gn.h
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def code64(code):
    """A shape code as the C ABI carries it: DSP_CODE_LEN (64) floats; a 32-D code occupies the first 32 entries, the rest is zero
    (the decoder has no weights for them and the optimiser leaves them alone)."""
    c = np.asarray(code, np.float32).reshape(-1)
    out = np.zeros(CODE_LEN, np.float32)
    n = min(c.shape[0], CODE_LEN)
    out[:n] = c[:n]
    return out


def ptr(a, typ=c_f32p):
    return None if a is None else a.ctypes.data_as(typ)


def check(rc, handle=None, what=""):
    if rc != 0:
        msg = load().dsp_last_error(handle)
        raise DspError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


class DecoderDescHolder(object):
    """Keeps the numpy arrays referenced by a DecoderDesc alive."""

    def __init__(self, layers, latent_in, code_len):
        self.w = [f32(w) for w, _ in layers]
        self.b = [f32(b) for _, b in layers]
        n = len(layers)
        self.out_dims = (C.c_int32 * n)(*[w.shape[0] for w in self.w])
        self.in_dims = (C.c_int32 * n)(*[w.shape[1] for w in self.w])
        self.wp = (c_f32p * n)(*[ptr(w) for w in self.w])
        self.bp = (c_f32p * n)(*[ptr(b) for b in self.b])
        lat = [int(x) for x in latent_in]
        self.desc = DecoderDesc(n, int(code_len), lat[0] if len(lat) == 1 else -1,
                                C.cast(self.out_dims, c_i32p), C.cast(self.in_dims, c_i32p),
                                C.cast(self.wp, C.POINTER(c_f32p)), C.cast(self.bp, C.POINTER(c_f32p)))
