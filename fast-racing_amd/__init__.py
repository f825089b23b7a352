"""fast-racing_amd — MI355X-native back-end for Fast-Racing's SE(3) MINCO trajectory optimiser.

Python here is plumbing only: a ctypes mirror of the C ABI in include/frx.h (the drop-in
boundary) plus the synthetic scenario generator.  All arithmetic of the hot path runs in
libfrx.so (HIP kernels for gfx950 + the host L-BFGS driver); there is no Python or CPU fallback,
and importing this package fails loudly when the library has not been built.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import scenario  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libfrx.so")

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


class FrxConfig(C.Structure):
    """struct frx_config (include/frx.h) = scalar arguments of SE3GCOPTER::setup (CPU.hpp:1076-1092)."""
    _fields_ = [
        ("rho", C.c_double), ("total_t", C.c_double), ("grid_res", C.c_double),
        ("qd_intervals", C.c_int), ("c2_diffeo", C.c_int),
        ("horiz_half_len", C.c_double), ("vert_half_len", C.c_double), ("safe_margin", C.c_double),
        ("vel_max", C.c_double), ("thr_acc_min", C.c_double), ("thr_acc_max", C.c_double),
        ("body_rate_max", C.c_double), ("grav_acc", C.c_double),
        ("penalty_pvtb", C.c_double * 4),
    ]

    @classmethod
    def from_params(cls, params: dict, **override):
        p = dict(params); p.update(override)
        c = cls()
        for name, _ in cls._fields_:
            if name == "penalty_pvtb":
                c.penalty_pvtb = (C.c_double * 4)(*p["penalty_pvtb"])
            else:
                setattr(c, name, p[name])
        return c


class LbfgsParams(C.Structure):
    """struct frx_lbfgs_params = lbfgs::lbfgs_parameter_t (lbfgs.hpp:18-140)."""
    _fields_ = [
        ("mem_size", C.c_int), ("g_epsilon", C.c_double), ("past", C.c_int), ("delta", C.c_double),
        ("max_iterations", C.c_int), ("max_linesearch", C.c_int), ("min_step", C.c_double), ("max_step", C.c_double),
        ("f_dec_coeff", C.c_double), ("s_curv_coeff", C.c_double), ("xtol", C.c_double),
    ]


BATCH_EVAL_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                            C.POINTER(C.c_double))

# every symbol include/frx.h declares (tests check that the library exports all of them)
ABI_SYMBOLS = [
    "frx_version", "frx_last_error", "frx_device_count", "frx_lbfgs_default_params", "frx_lbfgs_gcopter_params",
    "frx_problem_create", "frx_problem_destroy", "frx_problem_set_solver", "frx_problem_set_lbfgs_mode", "frx_problem_totals", "frx_problem_layout", "frx_initial_guess",
    "frx_objective_eval", "frx_objective_eval_device", "frx_penalty_eval", "frx_penalty_eval_device", "frx_forward",
    "frx_optimize", "frx_optimize_stats", "frx_lbfgs_minimize_batch",
    "frx_problem_create_from_h", "frx_enumerate_vertices", "frx_traj_to_msg", "frx_msg_sample", "frx_line_segment_dilate", "frx_corridor_generate", "frx_traj_max_rates", "frx_objective_eval_async", "frx_wait",
    "frx_problem_set_resident", "frx_optimize_path", "frx_penalty_problem_create", "frx_eval_status",
    "frx_dilate_batch", "frx_multi_create", "frx_multi_destroy", "frx_multi_info", "frx_multi_layout", "frx_multi_initial_guess", "frx_multi_optimize", "frx_multi_last_exchange",
    "frx_map_mark_cloud", "frx_map_is_blocked", "frx_grid_search", "frx_jps_plan", "frx_route_plan",
    "frx_trajectory_check", "frx_trajectory_check_device", "frx_trajectory_sample", "frx_trajectory_sample_device",
    "frx_trajectory_extrema", "frx_trajectory_extrema_device",
    "frx_gate_from_corners", "frx_trajectory_gates", "frx_trajectory_gates_device", "frx_gate_flags",
    "frx_trajectory_contain", "frx_trajectory_contain_device", "frx_contain_fold",
    "frx_trajectory_clearance", "frx_trajectory_clearance_workspace", "frx_trajectory_clearance_device",
    "frx_trajectory_clearance_exact", "frx_trajectory_clearance_exact_workspace", "frx_trajectory_clearance_exact_device", "frx_clearance_exact_fold",
    "frx_corridor_generate_batch", "frx_corridor_generate_batch_device",
    "frx_enumerate_vertices_batch", "frx_enumerate_vertices_batch_device", "frx_corridor_slots_to_tasks_device",
    "frx_map_esdf", "frx_map_esdf_workspace", "frx_map_esdf_device", "frx_map_esdf_on_device", "frx_map_mark_cloud_device",
    "frx_trajectory_map_distance", "frx_trajectory_map_distance_device", "frx_map_distance_fold",
    "frx_grid_search_levels", "frx_route_plan_levels_batch", "frx_route_search_workspace", "frx_route_plan_batch_device", "frx_route_plan_batch",
    "frx_route_plan_levels_window_batch", "frx_route_window_workspace", "frx_route_plan_window_batch_device", "frx_route_plan_window_batch",
]
# diagnostics, include/frx_debug.h: not part of the drop-in boundary
DEBUG_SYMBOLS = [
    "frx_debug_trace", "frx_resident_profile", "frx_debug_direction_log", "frx_debug_direction_log_read", "frx_debug_set_resident_retry",
    "frx_debug_resident_counts", "frx_debug_resident_clusters", "frx_debug_resident_predictions", "frx_eval_stage_times", "frx_profile_phases", "frx_dv_selftest", "frx_jps_tables", "frx_debug_host_cpu_share", "frx_debug_taken_over", "frx_debug_compact_from_history",
    "frx_debug_set_eval_fused", "frx_debug_eval_fused", "frx_debug_eval_geometry", "frx_debug_eval_front", "frx_debug_eval_prelude", "frx_debug_eval_adjoint", "frx_debug_set_eval_solo", "frx_debug_eval_solo", "frx_debug_penalty_kernel", "frx_debug_mailbox_numa", "frx_eval_launch_time", "frx_debug_profile_eval_cluster", "frx_debug_profile_eval_tail", "frx_debug_profile_eval_forward", "frx_debug_set_takeover_at", "frx_debug_shader_clock",
    "frx_debug_set_clear_chunk", "frx_debug_map_blocked_device", "frx_debug_dv_layout", "frx_debug_dv_round", "frx_debug_fold_rows", "frx_debug_lane_exchange",
    "frx_debug_set_clear_exact", "frx_debug_clear_exact_counts",
]

# frx_trajectory_check (include/frx.h): fields of a row and flag bits
CHECK_FIELDS = ("corridor", "speed", "thrust_min", "thrust_max", "body_rate", "acc", "worst_t", "worst_k")
CHECK_MAX_INTERVALS = 16384
CHECK_FLAG_CORRIDOR, CHECK_FLAG_SPEED, CHECK_FLAG_THRUST_MIN, CHECK_FLAG_THRUST_MAX, CHECK_FLAG_BODY_RATE, CHECK_FLAG_NONFINITE = 1, 2, 4, 8, 16, 32
# frx_trajectory_extrema (include/frx.h): fields of a row; its flags are the CHECK_FLAG_* bits (no CORRIDOR bit)
EXTREMA_FIELDS = ("speed", "acc", "thrust_min", "thrust_max", "body_rate", "t_speed", "t_acc", "t_thrust_min", "t_thrust_max", "t_body_rate")
# frx_trajectory_gates (include/frx.h): fields of a gate's row and flag bits
GATE_FIELDS = ("n_cross", "n_pass", "margin", "time", "piece", "u", "v", "reach_u", "reach_v", "normal_speed")
GATE_FLAG_MISSED, GATE_FLAG_REPEAT, GATE_FLAG_ORDER, GATE_FLAG_NONFINITE = 1, 2, 4, 8
# frx_trajectory_contain (include/frx.h): fields of a row; its flags are CHECK_FLAG_CORRIDOR and CHECK_FLAG_NONFINITE
CONTAIN_FIELDS = ("n_contact", "outside", "t_exit", "t_enter", "k_exit", "centre", "t_centre", "k_centre")
# frx_trajectory_clearance (include/frx.h): fields of a row, flag bits, the largest cloud; CLEAR_TILE sample states and CLEAR_PASS cloud points are what a
# workgroup of the kernel holds at a time (fast-racing_amd/csrc/frx_device.hpp), the sizes at which it takes another turn of a loop
CLEAR_FIELDS = ("ell", "dist", "worst_t", "worst_i")
CLEAR_MAX_POINTS = 1 << 24
CLEAR_FLAG_COLLISION, CLEAR_FLAG_NONFINITE = 1, 2
CLEAR_TILE, CLEAR_PASS = 64, 1024
# frx_trajectory_clearance_exact (include/frx.h): fields of a row; its flags are the CLEAR_FLAG_* bits
CLEAR_EXACT_FIELDS = ("ell", "dist", "t_ell", "i_ell", "t_dist", "i_dist")
# frx_trajectory_map_distance (include/frx.h): fields of a row and flag bits
MAPDIST_FIELDS = ("dist", "worst_t", "worst_cell", "outside")
MAPDIST_FLAG_BELOW, MAPDIST_FLAG_OUTSIDE, MAPDIST_FLAG_NONFINITE = 1, 2, 4
# frx_map_esdf (include/frx.h, fast-racing_amd/csrc/frx_esdf_plan.hpp): the most cells along x and along y or z, the lanes of a workgroup of every pass
ESDF_MAX_LINE, ESDF_MAX_DIM, ESDF_THREADS = 8192, 16384, 256
# frx_trajectory_sample (include/frx.h): doubles of a row and the named parts of it (FRX_SAMPLE_*)
SAMPLE_FIELDS = 20
SAMPLE_VIEWS = dict(pos=slice(0, 3), vel=slice(3, 6), acc=slice(6, 9), jerk=slice(9, 12), thrust=12, quat=slice(13, 17), omega=slice(17, 20))

_lib = None


def lib():
    """Load libfrx.so (built in-tree by __graft_entry__.build() / make -C fast-racing_amd/csrc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                               "There is no fallback implementation.")
        L = C.CDLL(LIB_PATH)
        L.frx_version.restype = C.c_int
        L.frx_last_error.restype = C.c_char_p
        L.frx_device_count.restype = C.c_int
        L.frx_lbfgs_default_params.argtypes = [C.POINTER(LbfgsParams)]
        L.frx_lbfgs_gcopter_params.argtypes = [C.POINTER(LbfgsParams), C.c_double]
        L.frx_problem_create.argtypes = [C.POINTER(FrxConfig), C.c_int, C.c_int, _ip, _dp, _dp, _ip, _dp, _ip, _dp, C.POINTER(C.c_void_p)]
        L.frx_problem_create_from_h.argtypes = [C.POINTER(FrxConfig), C.c_int, C.c_int, _ip, _dp, _dp, _ip, _dp, C.POINTER(C.c_void_p)]
        L.frx_enumerate_vertices.argtypes = [C.c_int, _dp, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        _up = np.ctypeslib.ndpointer(dtype=np.uint32, flags='C_CONTIGUOUS')
        L.frx_traj_to_msg.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _up]
        L.frx_msg_sample.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _up, C.c_double, _dp, _dp, _dp, _dp]
        L.frx_dv_selftest.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.frx_debug_dv_layout.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.frx_debug_dv_round.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 17
        L.frx_line_segment_dilate.argtypes = [_dp, _dp, _dp, C.c_int, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_corridor_generate.argtypes = [C.c_int, _dp, C.c_int, C.c_void_p, _dp, C.c_double, C.c_double, BLOCKED_FN, C.c_void_p, C.c_int, C.c_int,
                                            C.POINTER(C.c_int), _ip, _dp]
        L.frx_traj_max_rates.argtypes = [C.c_int, _dp, _dp, _dp, _dp]
        L.frx_objective_eval_async.argtypes = [C.c_void_p, _dp, _dp, _dp]
        L.frx_wait.argtypes = [C.c_void_p]
        L.frx_problem_set_resident.argtypes = [C.c_void_p, C.c_int]
        L.frx_optimize_path.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint)]
        L.frx_debug_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.frx_resident_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.frx_debug_direction_log.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.frx_debug_direction_log_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.frx_debug_set_resident_retry.argtypes = [C.c_void_p, C.c_int]
        L.frx_debug_resident_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.frx_debug_resident_predictions.argtypes = [C.c_void_p, C.c_void_p]
        L.frx_debug_resident_clusters.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.frx_dilate_batch.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, C.c_void_p, C.c_double, C.c_int, _ip, _dp, _dp, _dp]
        L.frx_eval_stage_times.argtypes = [C.c_void_p, _dp, C.c_int, _dp]
        L.frx_eval_launch_time.argtypes = [C.c_void_p, _dp, C.c_int, _dp]
        L.frx_debug_set_eval_fused.argtypes = [C.c_void_p, C.c_int]
        L.frx_debug_eval_fused.argtypes = [C.c_void_p]
        L.frx_debug_eval_geometry.argtypes = [C.c_void_p]
        L.frx_debug_eval_front.argtypes = [C.c_void_p]
        L.frx_debug_eval_prelude.argtypes = [C.c_void_p]
        L.frx_debug_eval_adjoint.argtypes = [C.c_void_p]
        L.frx_debug_set_eval_solo.argtypes = [C.c_void_p, C.c_int]
        L.frx_debug_eval_solo.argtypes = [C.c_void_p]
        L.frx_debug_penalty_kernel.argtypes = [C.c_void_p]
        L.frx_debug_mailbox_numa.argtypes = [C.c_void_p, C.c_void_p]
        L.frx_debug_profile_eval_cluster.argtypes = [C.c_void_p, _dp, C.c_void_p]
        L.frx_debug_profile_eval_tail.argtypes = [C.c_void_p, _dp, C.c_void_p]
        L.frx_debug_profile_eval_forward.argtypes = [C.c_void_p, _dp, C.c_void_p]
        L.frx_multi_create.argtypes = [C.POINTER(FrxConfig), C.c_int, C.c_void_p, C.c_int, _ip, _dp, _dp, _ip, _dp, _ip, _dp, C.POINTER(C.c_void_p)]
        L.frx_multi_destroy.argtypes = [C.c_void_p]
        L.frx_multi_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        L.frx_multi_layout.argtypes = [C.c_void_p, _ip, _ip]
        L.frx_multi_initial_guess.argtypes = [C.c_void_p, _dp]
        L.frx_multi_optimize.argtypes = [C.c_void_p, C.POINTER(LbfgsParams), _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                         _dp, _dp, C.POINTER(C.c_int)]
        L.frx_multi_last_exchange.argtypes = [C.c_void_p]
        L.frx_problem_destroy.argtypes = [C.c_void_p]
        L.frx_problem_set_solver.argtypes = [C.c_void_p, C.c_int]
        L.frx_problem_set_lbfgs_mode.argtypes = [C.c_void_p, C.c_int]
        L.frx_profile_phases.argtypes = [C.c_void_p, _dp, np.ctypeslib.ndpointer(dtype=np.int64, flags='C_CONTIGUOUS')]
        L.frx_problem_totals.argtypes = [C.c_void_p, _ip]
        L.frx_problem_layout.argtypes = [C.c_void_p, _ip, _ip, _ip, _ip]
        L.frx_initial_guess.argtypes = [C.c_void_p, _dp]
        L.frx_objective_eval.argtypes = [C.c_void_p, _dp, _dp, _dp]
        L.frx_objective_eval_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_penalty_eval.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp]
        L.frx_penalty_eval_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_forward.argtypes = [C.c_void_p, _dp, _dp, _dp]
        L.frx_trajectory_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_check_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.frx_trajectory_extrema.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_extrema_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_gate_from_corners.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_gates.argtypes = [C.c_void_p] * 7
        L.frx_trajectory_gates_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_gate_flags.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_contain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_contain_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        L.frx_contain_fold.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        L.frx_trajectory_sample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_clearance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_clearance_workspace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.frx_trajectory_clearance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_debug_set_clear_chunk.argtypes = [C.c_void_p, C.c_int]
        L.frx_trajectory_clearance_exact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_trajectory_clearance_exact_workspace.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
        L.frx_trajectory_clearance_exact_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_clearance_exact_fold.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_debug_set_clear_exact.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.frx_debug_clear_exact_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_debug_fold_rows.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
        L.frx_debug_lane_exchange.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_corridor_generate_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_corridor_generate_batch_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_enumerate_vertices_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.frx_enumerate_vertices_batch_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_corridor_slots_to_tasks_device.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_debug_map_blocked_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.frx_optimize.argtypes = [C.c_void_p, C.POINTER(LbfgsParams), _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip]
        L.frx_optimize_stats.argtypes = [C.c_void_p, _dp]
        L.frx_lbfgs_minimize_batch.argtypes = [C.c_int, _ip, _dp, _dp, _ip, _ip, _ip, C.POINTER(LbfgsParams), BATCH_EVAL_FN,
                                               C.c_void_p, C.c_int]
        _vp = C.c_void_p
        L.frx_map_mark_cloud.argtypes = [C.c_double * 3, C.c_int * 3, C.c_double, C.c_int, _vp, _vp]
        L.frx_map_is_blocked.argtypes = [_vp, _vp, _vp]
        L.frx_grid_search.argtypes = [_vp, _vp, _vp, _vp, C.c_double, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]
        L.frx_jps_tables.argtypes = [_vp] * 6
        L.frx_jps_plan.argtypes = [_vp, _vp, _vp, C.c_double, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.frx_route_plan.argtypes = [_vp, _vp, _vp, C.c_int, _vp, C.c_double, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]
        L.frx_map_esdf.argtypes = [_vp] * 4
        L.frx_map_esdf_workspace.argtypes = [_vp, C.POINTER(C.c_size_t)]
        L.frx_map_esdf_device.argtypes = [_vp] * 6
        L.frx_map_esdf_on_device.argtypes = [C.c_int] + [_vp] * 4
        L.frx_map_mark_cloud_device.argtypes = [_vp, _vp, C.c_int, _vp, _vp, _vp]
        L.frx_trajectory_map_distance.argtypes = [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_double, _vp, _vp, _vp]
        L.frx_trajectory_map_distance_device.argtypes = [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp]
        L.frx_map_distance_fold.argtypes = [C.c_int, _vp, _vp, _vp, C.c_double, _vp, _vp]
        L.frx_grid_search_levels.argtypes = [_vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp]
        L.frx_route_plan_levels_batch.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 7
        L.frx_route_search_workspace.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.frx_route_plan_batch_device.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 8
        L.frx_route_plan_batch.argtypes = [C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 7
        L.frx_route_plan_levels_window_batch.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 8
        L.frx_route_window_workspace.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_size_t)]
        L.frx_route_plan_window_batch_device.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 9
        L.frx_route_plan_window_batch.argtypes = [C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 8
        for name in ABI_SYMBOLS + DEBUG_SYMBOLS:
            fn = getattr(L, name)
            if name not in ("frx_version", "frx_last_error", "frx_device_count", "frx_lbfgs_default_params",
                            "frx_lbfgs_gcopter_params", "frx_problem_destroy"):
                fn.restype = C.c_int
        _lib = L
    return _lib


class FrxError(RuntimeError):
    """A non-zero frx_status; `.code` is the status (include/frx.h), the text is frx_last_error()."""
    code = 0


def _check(rc: int):
    if rc != 0:
        e = FrxError(f"frx error {rc}: {lib().frx_last_error().decode()}")
        e.code = rc
        raise e


def shader_clock(device: int = 0, ms: float = 2.0):
    """frx_debug_shader_clock: (min, mean, max) MHz the device sustains under a latency-bound FP64 load."""
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    _check(lib().frx_debug_shader_clock(device, C.c_double(ms), C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def lane_exchange(stride: int, values, device: int = 0):
    """frx_debug_lane_exchange: one wave's neighbour exchange by `stride` lanes as the one-launch evaluation does it (lane_exchange, csrc/frx_wave.hpp).
    values: 64 words of 64 bits (uint64 patterns, moved as they are) -> (below, above) with below[i] = values[i - stride], above[i] = values[i + stride];
    a lane without a source lane holds anything."""
    v = np.ascontiguousarray(values, dtype=np.uint64)
    assert v.shape == (64,)
    below, above = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
    _check(lib().frx_debug_lane_exchange(device, int(stride), v.ctypes.data, below.ctypes.data, above.ctypes.data))
    return below, above


def gcopter_lbfgs_params(rel_cost_tol: float, max_iterations: int = 0) -> LbfgsParams:
    p = LbfgsParams()
    lib().frx_lbfgs_gcopter_params(C.byref(p), rel_cost_tol)
    p.max_iterations = max_iterations
    return p


def pack_batch(cands):
    """Pack a list of scenario.Candidate into the CSR arrays of frx_problem_create."""
    coarse_n = np.array([c.coarse_n for c in cands], dtype=np.int32)
    ini = np.concatenate([c.ini_state.T.reshape(-1) for c in cands]).astype(np.float64)
    fin = np.concatenate([c.fin_state.T.reshape(-1) for c in cands]).astype(np.float64)
    h_off = [0]; v_off = [0]; h_rec = []; v_rec = []
    for c in cands:
        for h in c.h_polys:
            h_off.append(h_off[-1] + h.shape[1]); h_rec.append(h.T.reshape(-1))
        for v in c.v_polys:
            v_off.append(v_off[-1] + v.shape[1]); v_rec.append(v.T.reshape(-1))
    v_all = np.concatenate(v_rec).astype(np.float64) if v_rec else np.zeros(0)      # no vertices: frx_problem_create_from_h
    return (coarse_n, ini, fin, np.array(h_off, dtype=np.int32), np.concatenate(h_rec).astype(np.float64),
            np.array(v_off, dtype=np.int32), v_all)


def enumerate_vertices(hpoly: np.ndarray) -> np.ndarray:
    """Vertices (3 x nv) of a 6 x K H-polytope through the library (frx_enumerate_vertices)."""
    rec = np.ascontiguousarray(hpoly.T.reshape(-1), dtype=np.float64)
    nv = C.c_int()
    _check(lib().frx_enumerate_vertices(hpoly.shape[1], rec, None, 0, C.byref(nv)))
    out = np.zeros(3 * nv.value)
    _check(lib().frx_enumerate_vertices(hpoly.shape[1], rec, out.ctypes.data, nv.value, C.byref(nv)))
    return out.reshape(-1, 3).T.copy()


BLOCKED_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)


def line_segment_dilate(p1, p2, bbox, obs, offset: float = 0.0):
    """Corridor cell of one segment (frx_line_segment_dilate): (H 6 x K as [n; p] columns, ellipsoid C 3x3, centre d)."""
    p1 = np.ascontiguousarray(p1, dtype=np.float64); p2 = np.ascontiguousarray(p2, dtype=np.float64); bbox = np.ascontiguousarray(bbox, dtype=np.float64)
    obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 3)
    n = C.c_int()
    op = obs.ctypes.data if len(obs) else None
    _check(lib().frx_line_segment_dilate(p1, p2, bbox, len(obs), op, offset, 0, C.byref(n), None, None, None))
    rec = np.zeros(6 * n.value); Cm = np.zeros(9); d = np.zeros(3)
    _check(lib().frx_line_segment_dilate(p1, p2, bbox, len(obs), op, offset, n.value, C.byref(n), rec.ctypes.data, Cm.ctypes.data, d.ctypes.data))
    return rec.reshape(-1, 6).T.copy(), Cm.reshape(3, 3), d


def dilate_batch(p1, p2, bbox, obs, offset: float = 0.0, cap_planes: int = 96, device: int = 0):
    """Corridor cells of a batch of segments on the device (frx_dilate_batch): list of (H 6 x K, C 3x3, d) per segment."""
    p1 = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, 3); p2 = np.ascontiguousarray(p2, dtype=np.float64).reshape(-1, 3)
    obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 3)
    S = len(p1)
    npl = np.zeros(S, np.int32); rec = np.zeros(S * cap_planes * 6); Cm = np.zeros(S * 9); d = np.zeros(S * 3)
    _check(lib().frx_dilate_batch(device, S, p1.reshape(-1), p2.reshape(-1), np.ascontiguousarray(bbox, dtype=np.float64), len(obs),
                                  obs.ctypes.data if len(obs) else None, offset, cap_planes, npl, rec, Cm, d))
    rec = rec.reshape(S, cap_planes, 6)
    return [(rec[s, :npl[s]].T.copy(), Cm[9 * s:9 * s + 9].reshape(3, 3).copy(), d[3 * s:3 * s + 3].copy()) for s in range(S)]


def corridor_generate(path, obs, bbox, map_height: float, max_seg: float = 4.0, blocked=None, cap_polys: int = 4096, cap_planes: int = 1 << 18):
    """Greedy safe-flight corridor along `path` (n x 3) in the point cloud `obs` (frx_corridor_generate): list of 6 x K_i arrays."""
    path = np.ascontiguousarray(path, dtype=np.float64).reshape(-1, 3); obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 3)
    user = None
    if isinstance(blocked, VoxelMap):  # MapUtil::isBlocked on the grid, without a round trip through Python
        cb = C.cast(lib().frx_map_is_blocked, BLOCKED_FN); user = C.cast(C.pointer(blocked._s), C.c_void_p)
    else:
        cb = BLOCKED_FN(lambda a, b, u: int(bool(blocked(np.array(a[:3]), np.array(b[:3]))))) if blocked else C.cast(None, BLOCKED_FN)
    n = C.c_int(); h_off = np.zeros(cap_polys + 1, dtype=np.int32); h_rec = np.zeros(6 * cap_planes)
    _check(lib().frx_corridor_generate(len(path), path.reshape(-1), len(obs), obs.ctypes.data if len(obs) else None, np.ascontiguousarray(bbox, dtype=np.float64),
                                       map_height, max_seg, cb, user, cap_polys, cap_planes, C.byref(n), h_off, h_rec))
    return [h_rec[6 * h_off[k]:6 * h_off[k + 1]].reshape(-1, 6).T.copy() for k in range(n.value)]


# frx_corridor_generate_batch (include/frx.h): a path's status
CHAIN_OK, CHAIN_BOX_POINTS, CHAIN_PLANES, CHAIN_POLYS = 0, 1, 2, 3


def unpack_corridors(n_polys, h_off, h_rec):
    """The CSR of frx_corridor_generate_batch (n_polys per path, h_off over all cells in path order, records of 6 doubles) as a list per path of 6 x K arrays."""
    h_rec = np.asarray(h_rec, dtype=np.float64).reshape(-1); out = []; c = 0
    for n in n_polys:
        out.append([h_rec[6 * h_off[c + k]:6 * h_off[c + k + 1]].reshape(-1, 6).T.copy() for k in range(int(n))])
        c += int(n)
    return out


def corridor_generate_batch(paths, obs, bbox, map_height: float, max_seg: float = 4.0, blocked=None, cap_polys: int = 128, cap_planes: int = 96, device: int = 0,
                            raw: bool = False):
    """Greedy safe-flight corridors of a batch of paths on the device (frx_corridor_generate_batch), what corridor_generate gives path by path with
    blocked = a VoxelMap (or None: nothing blocks).  Returns (list per path of 6 x K_i arrays, status per path: CHAIN_*); a path with a non-zero status has no
    cells.  raw=True: (n_polys, h_off, h_rec, status) as the library packs them, ready for Problem(..., enumerate_v=True, packed=...)."""
    assert blocked is None or isinstance(blocked, VoxelMap), "the device walks sight lines on a VoxelMap; a Python callable cannot run there"
    paths = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3) for p in paths]
    obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 3); bbox = np.ascontiguousarray(bbox, dtype=np.float64)
    B = len(paths)
    off = np.zeros(B + 1, np.int32); off[1:] = np.cumsum([len(p) for p in paths])
    flat = np.ascontiguousarray(np.concatenate(paths).reshape(-1)) if B else np.zeros(0)
    n_polys = np.zeros(max(B, 1), np.int32); status = np.zeros(max(B, 1), np.int32); h_off = np.zeros(max(B, 1) * cap_polys + 1, np.int32); need = C.c_int()
    mp = C.cast(C.pointer(blocked._s), C.c_void_p) if blocked is not None else None
    cap_rec = 32 * int(off[-1]) + 64                                  # a first guess; the library reports the need when it is too small
    for _ in range(2):
        h_rec = np.zeros(6 * cap_rec)
        rc = lib().frx_corridor_generate_batch(device, B, off.ctypes.data, flat.ctypes.data, len(obs), obs.ctypes.data if len(obs) else None, bbox.ctypes.data,
                                               map_height, max_seg, mp, cap_polys, cap_planes, n_polys.ctypes.data, status.ctypes.data, cap_rec, C.byref(need),
                                               h_off.ctypes.data, h_rec.ctypes.data)
        if rc != -5 or need.value <= cap_rec:                             # FRX_ERR_CAPACITY with a larger need: once more with that room
            break
        cap_rec = need.value
    _check(rc)
    n_cells = int(n_polys.sum())
    if raw:
        return n_polys[:B].copy(), h_off[:n_cells + 1].copy(), h_rec[:6 * h_off[n_cells]].copy(), status[:B].copy()
    return unpack_corridors(n_polys[:B], h_off, h_rec), status[:B].copy()


def corridor_generate_batch_device(n_paths, path_off_dev, path_dev, n_obs, obs_dev, bbox, map_height, max_seg, map_struct, cap_polys, cap_planes, h_slot_dev,
                                   cell_planes_dev, n_polys_dev, status_dev, stream=0):
    """frx_corridor_generate_batch_device: one launch on `stream`; device addresses as integers, map_struct = a VoxelMapStruct whose cells point to device
    memory, or None.  Slots: h_slot [n_paths][cap_polys][cap_planes][6], cell_planes [n_paths][cap_polys], n_polys, status."""
    bbox = np.ascontiguousarray(bbox, dtype=np.float64)
    _check(lib().frx_corridor_generate_batch_device(n_paths, path_off_dev, path_dev, n_obs, obs_dev, bbox.ctypes.data, map_height, max_seg,
                                                    C.cast(C.pointer(map_struct), C.c_void_p) if map_struct is not None else None, cap_polys, cap_planes,
                                                    h_slot_dev, cell_planes_dev, n_polys_dev, status_dev, stream))


# frx_enumerate_vertices_batch (include/frx.h): a task's status, the most planes of a task, the range of cap_v
HV_OK, HV_UNBOUNDED, HV_FLAT, HV_PLANES, HV_VERTICES, HV_NONFINITE, HV_SKIPPED = 0, 1, 2, 3, 4, 5, 6
HV_MAX_PLANES, HV_MIN_CAP_V, HV_MAX_CAP_V = 256, 4, 512


def enumerate_vertices_batch(coarse_n, h_off, h_rec, cap_v: int = 64, device: int = 0):
    """V-polytopes of a batch of corridors on the device (frx_enumerate_vertices_batch): coarse_n, h_off, h_rec as frx_problem_create_from_h takes them (the
    raw output of corridor_generate_batch, or pack_batch(cands)[0, 3, 4]).  Returns (v_off, v_rec, status): the CSR frx_problem_create takes over the
    2 coarse_n[b] - 1 polytopes of every candidate in the order [cell 0, overlap 0|1, cell 1, ...], and HV_* per polytope (the vertices of an unbounded or
    flat polytope are included as the host computes them; a polytope with another non-zero status has none)."""
    coarse_n = np.ascontiguousarray(coarse_n, dtype=np.int32); h_off = np.ascontiguousarray(h_off, dtype=np.int32)
    h_rec = np.ascontiguousarray(h_rec, dtype=np.float64).reshape(-1)
    B = len(coarse_n)
    n_tasks = max(int(2 * coarse_n.sum() - B), 1) if B else 1
    status = np.zeros(n_tasks, np.int32); v_off = np.zeros(n_tasks + 1, np.int32); need = C.c_int()
    cap_vert = 24 * n_tasks                                               # a first guess; the library reports the need when it is too small
    for _ in range(2):
        v_rec = np.zeros(3 * cap_vert)
        rc = lib().frx_enumerate_vertices_batch(device, B, coarse_n.ctypes.data, h_off.ctypes.data, h_rec.ctypes.data, cap_v, status.ctypes.data, v_off.ctypes.data,
                                                cap_vert, C.byref(need), v_rec.ctypes.data)
        if rc != -5 or need.value <= cap_vert:                            # FRX_ERR_CAPACITY with a larger need: once more with that room
            break
        cap_vert = need.value
    _check(rc)
    return v_off, v_rec[:3 * need.value].copy(), status


def enumerate_vertices_batch_device(n_tasks, tasks_dev, h_rec_dev, cap_v, v_slot_dev, nv_dev, status_dev, stream=0):
    """frx_enumerate_vertices_batch_device: one launch on `stream`; device addresses as integers.  tasks [n_tasks][4] int (begin0, count0, begin1, count1 in
    records of h_rec); outputs v_slot [n_tasks][cap_v][3], nv [n_tasks], status [n_tasks]."""
    _check(lib().frx_enumerate_vertices_batch_device(n_tasks, tasks_dev, h_rec_dev, cap_v, v_slot_dev, nv_dev, status_dev, stream))


def corridor_slots_to_tasks_device(n_paths, cap_polys, cap_planes, cell_planes_dev, n_polys_dev, tasks_dev, stream=0):
    """frx_corridor_slots_to_tasks_device: one launch on `stream` that fills tasks [n_paths][2 cap_polys - 1][4] from the slotted outputs of
    corridor_generate_batch_device (record indices into its h_slot)."""
    _check(lib().frx_corridor_slots_to_tasks_device(n_paths, cap_polys, cap_planes, cell_planes_dev, n_polys_dev, tasks_dev, stream))


class VoxelMapStruct(C.Structure):
    """frx_voxel_map (include/frx.h)."""
    _fields_ = [("origin", C.c_double * 3), ("dim", C.c_int * 3), ("res", C.c_double), ("cells", C.c_void_p)]


class VoxelMap:
    """The occupancy grid of JPS::MapUtil<3> (map_util.h): origin, dim (cells per axis), res, cells[z][y][x] int8
    (0 free, 100 occupied, -1 unknown)."""

    def __init__(self, origin, dim, res: float, cells=None):
        self.origin = np.asarray(origin, dtype=np.float64).copy(); self.dim = np.asarray(dim, dtype=np.int32).copy(); self.res = float(res)
        n = int(self.dim[0]) * int(self.dim[1]) * int(self.dim[2])
        self.cells = np.zeros(n, dtype=np.int8) if cells is None else np.ascontiguousarray(cells, dtype=np.int8).reshape(-1)
        assert self.cells.size == n
        self._s = VoxelMapStruct((C.c_double * 3)(*self.origin), (C.c_int * 3)(*[int(d) for d in self.dim]), self.res, self.cells.ctypes.data)

    @classmethod
    def from_params(cls, x_size: float, y_size: float, z_size: float, res: float = 0.1):
        """MapUtil::setParam (map_util.h:48-70): origin (-x_size/2, -10, 0), dim = int(size / res)."""
        return cls([-x_size / 2, -10.0, 0.0], [int(x_size / res), int(y_size / res), int(z_size / res)], res)

    def mark_cloud(self, pts) -> int:
        """frx_map_mark_cloud: the cells holding the points become occupied; returns how many points were inside."""
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        rc = lib().frx_map_mark_cloud(self._s.origin, self._s.dim, self.res, len(pts), pts.ctypes.data if len(pts) else None, self.cells.ctypes.data)
        if rc < 0:
            _check(rc)
        return rc

    def is_blocked(self, a, b) -> bool:
        a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
        return bool(lib().frx_map_is_blocked(a.ctypes.data, b.ctypes.data, C.byref(self._s)))

    def is_blocked_device(self, a, b, device: int = 0):
        """frx_debug_map_blocked_device: the device's sight line on pairs a[i], b[i] (n x 3 each) -> bool array."""
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3); b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(len(a), np.int32)
        _check(lib().frx_debug_map_blocked_device(device, C.byref(self._s), len(a), a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out.astype(bool)

    def _esdf(self, fields, call):
        n = self.cells.size
        out = {k: np.empty(n) for k in fields}
        if not out or set(out) - {"pos", "neg", "all"}:
            raise ValueError(f"esdf: fields must name some of pos, neg, all, got {tuple(fields)}")
        _check(call(*[out[k].ctypes.data if k in out else None for k in ("pos", "neg", "all")]))
        return out

    def esdf(self, fields=("pos", "neg", "all")):
        """frx_map_esdf on the host: dict of the named fields, each a float64 array over the cells (x fastest); a field not named is not computed."""
        return self._esdf(fields, lambda *o: lib().frx_map_esdf(C.byref(self._s), *o))

    def esdf_on_device(self, fields=("pos", "neg", "all"), device: int = 0):
        """frx_map_esdf_on_device: the same fields from the device (upload, five launches, download)."""
        return self._esdf(fields, lambda *o: lib().frx_map_esdf_on_device(int(device), C.byref(self._s), *o))

    def device_struct(self, cells_dev: int = 0) -> VoxelMapStruct:
        """A frx_voxel_map with this map's origin, dim and res whose cells point to device memory at cells_dev (the device forms take such a struct)."""
        return VoxelMapStruct((C.c_double * 3)(*self.origin), (C.c_int * 3)(*[int(d) for d in self.dim]), self.res, cells_dev or None)

    def plan(self, start, goal, eps: float = 1.0, use_jps: bool = False, cap: int = 1 << 16):
        """frx_jps_plan -> dict(status, raw_path, path, sample_path, expanded)."""
        start = np.ascontiguousarray(start, dtype=np.float64); goal = np.ascontiguousarray(goal, dtype=np.float64)
        bufs = [np.zeros((cap, 3)) for _ in range(3)]; ns = [C.c_int() for _ in range(3)]; st = C.c_int(); ex = C.c_int()
        _check(lib().frx_jps_plan(C.byref(self._s), start.ctypes.data, goal.ctypes.data, float(eps), int(use_jps), cap,
                                  C.byref(ns[0]), bufs[0].ctypes.data, C.byref(ns[1]), bufs[1].ctypes.data, C.byref(ns[2]), bufs[2].ctypes.data,
                                  C.byref(st), C.byref(ex)))
        return dict(status=st.value, raw_path=bufs[0][:ns[0].value].copy(), path=bufs[1][:ns[1].value].copy(),
                    sample_path=bufs[2][:ns[2].value].copy(), expanded=ex.value)

    def route(self, start, goal, gates=(), eps: float = 1.0, use_jps: bool = False, threads: int = 0, cap: int = 1 << 18):
        """frx_route_plan -> (path n x 3 (empty when a leg failed), leg_status, leg_expanded)."""
        start = np.ascontiguousarray(start, dtype=np.float64); goal = np.ascontiguousarray(goal, dtype=np.float64)
        gates = np.ascontiguousarray(gates, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((cap, 3)); n = C.c_int(); st = np.zeros(len(gates) + 1, dtype=np.int32); ex = np.zeros(len(gates) + 1, dtype=np.int32)
        _check(lib().frx_route_plan(C.byref(self._s), start.ctypes.data, goal.ctypes.data, len(gates), gates.ctypes.data if len(gates) else None,
                                    float(eps), int(use_jps), int(threads), cap, C.byref(n), out.ctypes.data, st.ctypes.data, ex.ctypes.data))
        return out[:n.value].copy(), st, ex

    def _route_batch(self, routes, call, cap_level, cap_raw, cap_pts, cap_total):
        off, pts = pack_routes(routes)
        R = len(routes); NL = max(int(off[-1]) - R, 1)
        cap_total = int(cap_total) if cap_total is not None else max(2 * R, NL * int(cap_pts))
        path_off = np.zeros(R + 1, np.int32); path = np.zeros((max(cap_total, 1), 3)); rst = np.zeros(max(R, 1), np.int32)
        lst = np.zeros(NL, np.int32); lev = np.zeros(NL, np.int32); mx = np.zeros(NL, np.int32); need = C.c_int()
        rc = call(C.byref(self._s), R, off.ctypes.data, pts.ctypes.data, int(cap_level), int(cap_raw), int(cap_pts), cap_total, path_off.ctypes.data, path.ctypes.data,
                  rst.ctypes.data, lst.ctypes.data, lev.ctypes.data, mx.ctypes.data, C.addressof(need))
        if rc != -5:                                                      # FRX_ERR_CAPACITY: every output is valid, `need` says what the routes would take
            _check(rc)
        n_legs = int(off[-1]) - R
        return dict(path_off=path_off, path=path[:path_off[-1]].copy(), paths=[path[path_off[r]:path_off[r + 1]].copy() for r in range(R)], route_status=rst[:R],
                    leg_status=lst[:n_legs], levels=lev[:n_legs], max_level_cells=mx[:n_legs], need=need.value, fits=rc == 0)

    def route_batch_host(self, routes, cap_level: int = 1 << 16, cap_raw: int = 1 << 16, cap_pts: int = 1 << 12, cap_total=None):
        """frx_route_plan_levels_batch on one host thread, the referee of route_batch: routes = a list of (n_i, 3) waypoint arrays (start, gates, goal).
        dict(path_off, path, paths (per route), route_status, leg_status, levels, max_level_cells, need, fits); cap_total None: room for every leg's cap_pts."""
        return self._route_batch(routes, lib().frx_route_plan_levels_batch, cap_level, cap_raw, cap_pts, cap_total)

    def route_batch(self, routes, device: int = 0, cap_level: int = 1 << 16, cap_raw: int = 1 << 16, cap_pts: int = 1 << 12, cap_total=None):
        """frx_route_plan_batch: the same batch searched on the device (upload, four launches, download); the same dict, bit for bit."""
        return self._route_batch(routes, lambda *a: lib().frx_route_plan_batch(int(device), *a), cap_level, cap_raw, cap_pts, cap_total)

    def _route_batch_window(self, routes, call, pad, cap_window, cap_level, cap_raw, cap_pts, cap_total):
        off, _ = pack_routes(routes)
        win = np.zeros((max(int(off[-1]) - len(routes), 1), 8), np.int32)
        out = self._route_batch(routes, lambda m, R, o, p, cl, cr, cp, ct, *rest: call(m, R, o, p, int(pad), int(cap_window), cl, cr, cp, ct, *rest[:6], win.ctypes.data,
                                                                                   rest[6]), cap_level, cap_raw, cap_pts, cap_total)
        out["leg_window"] = win[:len(out["leg_status"])]
        return out

    def route_batch_window_host(self, routes, pad: int, cap_window: int, cap_level: int = 1 << 16, cap_raw: int = 1 << 16, cap_pts: int = 1 << 12, cap_total=None):
        """frx_route_plan_levels_window_batch on one host thread, the referee of route_batch_window: every leg searched inside the box of its two end cells widened
        by `pad` cells (at most cap_window cells).  The dict of route_batch_host plus leg_window (n_legs x 8: lo xyz, size xyz, limit or -1 for a whole-map
        window, 0).  leg_status 0: bit for bit the leg of route_batch_host; 6: the window holds more than cap_window cells; 7: the window certifies nothing."""
        return self._route_batch_window(routes, lib().frx_route_plan_levels_window_batch, pad, cap_window, cap_level, cap_raw, cap_pts, cap_total)

    def route_batch_window(self, routes, pad: int, cap_window: int, device: int = 0, cap_level: int = 1 << 16, cap_raw: int = 1 << 16, cap_pts: int = 1 << 12,
                           cap_total=None, fallback: bool = False):
        """frx_route_plan_window_batch: the same batch on the device (upload, three launches, download); the same dict, bit for bit.  fallback=True reruns
        through route_batch, the whole-map form, exactly the routes that have a leg with status 6 or 7 and puts their rows in place, in route order: paths,
        path, path_off, route_status, levels and max_level_cells are then those of route_batch on the same routes, and leg_status keeps 6 or 7 on the legs
        that needed the whole map and found their path there (a leg the whole map fails as well shows the whole map's status).  `need` is the points of the
        result and `fits` compares it with cap_total where one was given."""
        out = self._route_batch_window(routes, lambda *a: lib().frx_route_plan_window_batch(int(device), *a), pad, cap_window, cap_level, cap_raw, cap_pts, cap_total)
        if not fallback:
            return out
        first = np.concatenate([[0], np.cumsum([len(np.asarray(r).reshape(-1, 3)) - 1 for r in routes])]).astype(int)
        again = [r for r in range(len(routes)) if np.isin(out["leg_status"][first[r]:first[r + 1]], (6, 7)).any()]
        if not again:
            return out
        whole = self.route_batch([routes[r] for r in again], device=device, cap_level=cap_level, cap_raw=cap_raw, cap_pts=cap_pts)
        paths = list(out["paths"])
        rst, lst, lev, mx = (out[k].copy() for k in ("route_status", "leg_status", "levels", "max_level_cells"))
        at = 0
        for i, r in enumerate(again):
            n = first[r + 1] - first[r]
            paths[r] = whole["paths"][i]
            rst[r] = whole["route_status"][i]
            w = whole["leg_status"][at:at + n]
            seg = lst[first[r]:first[r + 1]]
            lst[first[r]:first[r + 1]] = np.where(np.isin(seg, (6, 7)) & (w == 0), seg, w)
            lev[first[r]:first[r + 1]] = whole["levels"][at:at + n]
            mx[first[r]:first[r + 1]] = whole["max_level_cells"][at:at + n]
            at += n
        path_off = np.zeros(len(routes) + 1, np.int32); path_off[1:] = np.cumsum([len(p) for p in paths])
        need = int(path_off[-1])
        return dict(path_off=path_off, path=np.concatenate(paths).reshape(-1, 3), paths=paths, route_status=rst, leg_status=lst, levels=lev, max_level_cells=mx,
                    need=need, fits=cap_total is None or need <= int(cap_total), leg_window=out["leg_window"])


def pack_routes(routes):
    """(pt_off int32 [n + 1], pts float64 [sum, 3]) of a list of routes, each an (n_i, 3) array of waypoints: start, gates in order, goal."""
    routes = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 3) for r in routes]
    off = np.zeros(len(routes) + 1, np.int32); off[1:] = np.cumsum([len(r) for r in routes])
    return off, (np.ascontiguousarray(np.concatenate(routes)) if routes else np.zeros((0, 3)))


def route_search_workspace(dim, n_legs: int, cap_level: int, cap_raw: int, cap_pts: int) -> int:
    """frx_route_search_workspace: bytes of device scratch route_plan_batch_device needs; FrxError with code -1 / -5 for arguments it refuses."""
    d = (C.c_int * 3)(*[int(v) for v in dim])
    n = C.c_size_t(0)
    _check(lib().frx_route_search_workspace(d, int(n_legs), int(cap_level), int(cap_raw), int(cap_pts), C.byref(n)))
    return int(n.value)


def route_plan_batch_device(map_struct: VoxelMapStruct, n_routes: int, n_legs: int, pt_off_dev: int, pts_dev: int, cap_level: int, cap_raw: int, cap_pts: int,
                            cap_total: int, work_dev: int, path_off_dev: int, path_dev: int, route_status_dev: int, leg_status_dev: int, leg_levels_dev: int,
                            leg_max_level_dev: int, stream: int = 0):
    """frx_route_plan_batch_device: four launches on `stream`; map_struct's cells and the other addresses (integers) are device memory.  Outputs: the CSR
    path_off [n_routes + 1] / path [cap_total][3] that corridor_generate_batch_device takes, route_status [n_routes], and per leg status, levels, max level."""
    _check(lib().frx_route_plan_batch_device(C.byref(map_struct), int(n_routes), int(n_legs), pt_off_dev or None, pts_dev or None, int(cap_level), int(cap_raw),
                                             int(cap_pts), int(cap_total), work_dev or None, path_off_dev or None, path_dev or None, route_status_dev or None,
                                             leg_status_dev or None, leg_levels_dev or None, leg_max_level_dev or None, stream))


def route_window_workspace(n_legs: int, cap_level: int, cap_raw: int, cap_pts: int, cap_window: int) -> int:
    """frx_route_window_workspace: bytes of device scratch route_plan_window_batch_device needs, whatever the map's size; FrxError with code -1 / -5 for
    arguments it refuses."""
    n = C.c_size_t(0)
    _check(lib().frx_route_window_workspace(int(n_legs), int(cap_level), int(cap_raw), int(cap_pts), int(cap_window), C.byref(n)))
    return int(n.value)


def route_plan_window_batch_device(map_struct: VoxelMapStruct, n_routes: int, n_legs: int, pt_off_dev: int, pts_dev: int, pad: int, cap_window: int, cap_level: int,
                                   cap_raw: int, cap_pts: int, cap_total: int, work_dev: int, path_off_dev: int, path_dev: int, route_status_dev: int,
                                   leg_status_dev: int, leg_levels_dev: int, leg_max_level_dev: int, leg_window_dev: int, stream: int = 0):
    """frx_route_plan_window_batch_device: three launches on `stream`; the arguments of route_plan_batch_device with the pad and cap_window of the windows, a
    workspace of route_window_workspace bytes and leg_window [n_legs][8]."""
    _check(lib().frx_route_plan_window_batch_device(C.byref(map_struct), int(n_routes), int(n_legs), pt_off_dev or None, pts_dev or None, int(pad), int(cap_window),
                                                    int(cap_level), int(cap_raw), int(cap_pts), int(cap_total), work_dev or None, path_off_dev or None,
                                                    path_dev or None, route_status_dev or None, leg_status_dev or None, leg_levels_dev or None,
                                                    leg_max_level_dev or None, leg_window_dev or None, stream))


def grid_search_levels(cmap, dim, start, goal, cap: int = 1 << 20):
    """frx_grid_search_levels on an int8 occupancy array (x fastest, 3-D): (path START-first k x 3 int, levels, max_level_cells) of the canonical level search;
    an empty path and levels = -1 when there is none."""
    cmap = np.ascontiguousarray(cmap, dtype=np.int8).reshape(-1)
    dim = np.asarray(dim, dtype=np.int32); start = np.asarray(start, dtype=np.int32); goal = np.asarray(goal, dtype=np.int32)
    path = np.zeros((cap, 3), dtype=np.int32); n = C.c_int(); lev = C.c_int(); mx = C.c_int()
    _check(lib().frx_grid_search_levels(cmap.ctypes.data, dim.ctypes.data, start.ctypes.data, goal.ctypes.data, cap, C.byref(n), path.ctypes.data, C.byref(lev),
                                        C.byref(mx)))
    return path[:n.value].copy(), lev.value, mx.value


def map_esdf(vmap: VoxelMap, fields=("pos", "neg", "all")):
    """frx_map_esdf: the distance field of a VoxelMap on the host (VoxelMap.esdf)."""
    return vmap.esdf(fields)


def map_esdf_on_device(vmap: VoxelMap, fields=("pos", "neg", "all"), device: int = 0):
    """frx_map_esdf_on_device: the same field from the device (VoxelMap.esdf_on_device)."""
    return vmap.esdf_on_device(fields, device)


def map_esdf_workspace(dim) -> int:
    """frx_map_esdf_workspace: bytes of device scratch map_esdf_device needs for a grid of dim cells; FrxError with code -1 / -5 for a grid it refuses."""
    d = (C.c_int * 3)(*[int(v) for v in dim])
    n = C.c_size_t(0)
    _check(lib().frx_map_esdf_workspace(d, C.byref(n)))
    return int(n.value)


def map_esdf_device(map_struct: VoxelMapStruct, pos_dev: int, neg_dev: int, all_dev: int, work_dev: int, stream: int = 0):
    """frx_map_esdf_device: five launches on `stream`; map_struct's cells and the other addresses (integers, 0 = that field is not computed) are device memory."""
    _check(lib().frx_map_esdf_device(C.byref(map_struct), pos_dev or None, neg_dev or None, all_dev or None, work_dev or None, stream))


def map_mark_cloud_device(map_struct: VoxelMapStruct, cells_dev: int, n_pts: int, pts_dev: int, n_inside_dev: int, stream: int = 0):
    """frx_map_mark_cloud_device: the cells (int8 at cells_dev) holding the n_pts points at pts_dev become 100, the int32 at n_inside_dev the number of points
    inside; launches on `stream`, device addresses as integers."""
    _check(lib().frx_map_mark_cloud_device(C.byref(map_struct), cells_dev or None, int(n_pts), pts_dev or None, n_inside_dev or None, stream))


def map_distance_fold(piece_rows, T, piece_off, margin: float):
    """Candidate rows (B, 4) and MAPDIST_FLAG_* words (B,) uint32 from the piece rows (P, 4) of trajectory_map_distance_device (frx_map_distance_fold, host
    only): candidate b owns the pieces piece_off[b] .. piece_off[b + 1] - 1.  A candidate without pieces keeps a row of zeros."""
    piece_off = np.ascontiguousarray(piece_off, dtype=np.int32).reshape(-1)
    rows = np.ascontiguousarray(piece_rows, dtype=np.float64).reshape(-1, len(MAPDIST_FIELDS))
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
    B = piece_off.size - 1
    if B >= 1 and (rows.shape[0] < int(piece_off.max()) or T.size < int(piece_off.max())):
        raise ValueError(f"map_distance_fold: {rows.shape[0]} rows and {T.size} durations for piece_off up to {int(piece_off.max())}")
    cand = np.zeros((max(B, 0), len(MAPDIST_FIELDS))); flags = np.zeros(max(B, 0), np.uint32)
    pad = np.zeros(1)
    _check(lib().frx_map_distance_fold(B, piece_off.ctypes.data, (T if T.size else pad).ctypes.data, (rows if rows.size else pad).ctypes.data, float(margin),
                                       cand.ctypes.data, flags.ctypes.data))
    return cand, flags


def grid_search(cmap, dim, start, goal, eps: float = 1.0, use_jps: bool = False, max_expand: int = -1, cap: int = 1 << 20):
    """frx_grid_search on an int8 occupancy array (x fastest; dim[2] = 0 for 2-D): (path goal-first k x 3 int, expanded, cost)."""
    cmap = np.ascontiguousarray(cmap, dtype=np.int8).reshape(-1)
    dim = np.asarray(dim, dtype=np.int32); start = np.asarray(start, dtype=np.int32); goal = np.asarray(goal, dtype=np.int32)
    path = np.zeros((cap, 3), dtype=np.int32); n = C.c_int(); ex = C.c_int(); cost = C.c_double()
    _check(lib().frx_grid_search(cmap.ctypes.data, dim.ctypes.data, start.ctypes.data, goal.ctypes.data, float(eps), int(use_jps), int(max_expand),
                                 cap, C.byref(n), path.ctypes.data, C.byref(ex), C.byref(cost)))
    return path[:n.value].copy(), ex.value, cost.value


def jps_tables():
    """The jump-point neighbour tables in the reference's storage order (frx_jps_tables)."""
    t = [np.zeros(s, dtype=np.int32) for s in ((27, 3, 26), (27, 3, 12), (27, 3, 12), (9, 2, 8), (9, 2, 2), (9, 2, 2))]
    _check(lib().frx_jps_tables(*[a.ctypes.data for a in t]))
    return t


def dv_selftest(n, B=4, m=128, iters=140, geom=None, seed=0, device=0):
    """(worst relative error of the device search direction vs a host two-loop recursion, mean us of the last launches)."""
    err, us = C.c_double(), C.c_double()
    gp = (C.c_int * 4)(*geom) if geom else None
    _check(lib().frx_dv_selftest(device, n, B, m, iters, gp, seed, C.byref(err), C.byref(us)))
    return err.value, us.value


# struct DvCommand / DvResult and the command bits of the device-vector L-BFGS (csrc/frx_lbfgs.hpp)
DV_COMMAND = np.dtype([("flags", np.int32), ("slot", np.int32), ("bound", np.int32), ("newest", np.int32), ("step", np.float64)])
DV_RESULT = np.dtype([("f", np.float64), ("dg", np.float64), ("xx", np.float64), ("gg", np.float64), ("dginit", np.float64), ("pad", np.float64, 3)])
DV_EVAL, DV_INIT, DV_ADVANCE, DV_TRIAL, DV_RESTORE = 1, 2, 4, 8, 16


def dv_layout(n_max, geom=None, tight=True):
    """frx_debug_dv_layout: ((E, W, PF, BLK), row stride hs) of k_lbfgs_pre for a batch whose longest vector has n_max elements."""
    out = np.zeros(5, np.int32)
    gp = np.ascontiguousarray(geom, dtype=np.int32) if geom is not None else None
    _check(lib().frx_debug_dv_layout(int(n_max), gp.ctypes.data if gp is not None else None, int(bool(tight)), out.ctypes.data))
    return tuple(int(v) for v in out[:4]), int(out[4])


def dv_round(st, cmd, f=None, device=0):
    """frx_debug_dv_round: one launch of k_lbfgs_pre (and of k_lbfgs_post when f is given) on the state `st`, IN PLACE.  st: geom (E, W, PF, BLK), hs, m,
    xoff int32 [B+1]; x, g, xp, gp, d float64 of one length; S, Y of one length (>= B m hs); ys; gt; res (DV_RESULT records); optionally poff int32 [B+1] with
    dflags and pflags int32.  Arrays may be longer than the batch needs: their whole length goes to the device and comes back.  cmd: DV_COMMAND [B]."""
    B = len(st["xoff"]) - 1
    geom = np.ascontiguousarray(st["geom"], dtype=np.int32)
    for k in ("x", "g", "xp", "gp", "d", "S", "Y", "ys", "gt"):
        a = st[k]
        assert a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable, k
    assert len({st[k].size for k in ("x", "g", "xp", "gp", "d")}) == 1 and st["S"].size == st["Y"].size
    assert st["xoff"].dtype == np.int32 and cmd.dtype == DV_COMMAND and len(cmd) == B and st["res"].dtype == DV_RESULT and cmd.flags.c_contiguous
    with_p = st.get("poff") is not None
    if with_p:
        assert st["poff"].dtype == np.int32 and st["pflags"].dtype == np.int32 and len(st["poff"]) == B + 1
    with_d = st.get("dflags") is not None
    if with_d:
        assert st["dflags"].dtype == np.int32
    lens = np.array([st["x"].size, st["S"].size, st["ys"].size, st["gt"].size, st["dflags"].size if with_d else 0, st["pflags"].size if with_p else 0,
                     len(st["res"])], dtype=np.int64)
    fa = None if f is None else np.ascontiguousarray(f, dtype=np.float64)
    assert fa is None or fa.size == B
    ptr = lambda a: a.ctypes.data
    _check(lib().frx_debug_dv_round(device, B, int(st["m"]), ptr(geom), int(st["hs"]), ptr(lens), ptr(st["xoff"]), ptr(st["x"]), ptr(st["g"]), ptr(st["xp"]),
                                    ptr(st["gp"]), ptr(st["d"]), ptr(st["S"]), ptr(st["Y"]), ptr(st["ys"]), ptr(st["gt"]), ptr(cmd), ptr(st["res"]),
                                    ptr(st["poff"]) if with_p else None, ptr(st["dflags"]) if with_d else None, ptr(st["pflags"]) if with_p else None,
                                    ptr(fa) if fa is not None else None))


def traj_max_rates(T, Cf):
    """(max |v|, max |a|) per piece (frx_traj_max_rates)."""
    n = len(T); mv = np.zeros(n); ma = np.zeros(n)
    _check(lib().frx_traj_max_rates(n, np.ascontiguousarray(T, dtype=np.float64), np.ascontiguousarray(Cf, dtype=np.float64).reshape(-1), mv, ma))
    return mv, ma


def gate_from_corners(corners, with_fit: bool = False):
    """Gate records (n, 9) {c, a, b} from corners (n, 4, 3) in order round each opening (frx_gate_from_corners, host only); with_fit adds the
    (n, 2) fit {a.b / (|a| |b|), largest distance of a corner from the record's rectangle}."""
    corners = np.ascontiguousarray(corners, dtype=np.float64)
    if corners.size == 0 or corners.size % 12 != 0 or corners.shape[-1] not in (3, 12):
        raise ValueError(f"gate_from_corners: corners must have shape (n, 4, 3), got {corners.shape}")
    n = corners.size // 12
    gates = np.zeros((n, 9)); fit = np.zeros((n, 2))
    _check(lib().frx_gate_from_corners(n, corners.ctypes.data, gates.ctypes.data, fit.ctypes.data if with_fit else None))
    return (gates, fit) if with_fit else gates


def gate_flags(gate_rows, gate_off):
    """GATE_FLAG_* words (B,) uint32 of the candidates from their gate rows (n_gates, 10) (frx_gate_flags, host only)."""
    gate_off = np.ascontiguousarray(gate_off, dtype=np.int32).reshape(-1)
    rows = np.ascontiguousarray(gate_rows, dtype=np.float64).reshape(-1, len(GATE_FIELDS))
    B = gate_off.size - 1
    if B >= 1 and rows.shape[0] < int(gate_off.max()):
        raise ValueError(f"gate_flags: {rows.shape[0]} rows for gate_off up to {int(gate_off.max())}")
    flags = np.zeros(max(B, 0), np.uint32)
    _check(lib().frx_gate_flags(B, gate_off.ctypes.data, rows.ctypes.data if rows.size else flags.ctypes.data, flags.ctypes.data))
    return flags


def contain_fold(piece_rows, T, piece_off):
    """Candidate rows (B, 8) and CHECK_FLAG_* words (B,) uint32 from the piece rows (P, 8) of trajectory_contain_device (frx_contain_fold, host only):
    candidate b owns the pieces piece_off[b] .. piece_off[b + 1] - 1.  A candidate without pieces keeps a row of zeros."""
    piece_off = np.ascontiguousarray(piece_off, dtype=np.int32).reshape(-1)
    rows = np.ascontiguousarray(piece_rows, dtype=np.float64).reshape(-1, len(CONTAIN_FIELDS))
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
    B = piece_off.size - 1
    if B >= 1 and (rows.shape[0] < int(piece_off.max()) or T.size < int(piece_off.max())):
        raise ValueError(f"contain_fold: {rows.shape[0]} rows and {T.size} durations for piece_off up to {int(piece_off.max())}")
    cand = np.zeros((max(B, 0), len(CONTAIN_FIELDS))); flags = np.zeros(max(B, 0), np.uint32)
    pad = np.zeros(1)
    _check(lib().frx_contain_fold(B, piece_off.ctypes.data, (T if T.size else pad).ctypes.data, (rows if rows.size else pad).ctypes.data,
                                  cand.ctypes.data, flags.ctypes.data))
    return cand, flags


def clearance_exact_fold(piece_rows, T, piece_off):
    """Candidate rows (B, 6) and CLEAR_FLAG_* words (B,) uint32 from the piece rows (P, 6) of trajectory_clearance_exact_device (frx_clearance_exact_fold, host
    only): candidate b owns the pieces piece_off[b] .. piece_off[b + 1] - 1.  A candidate without pieces keeps a row of zeros."""
    piece_off = np.ascontiguousarray(piece_off, dtype=np.int32).reshape(-1)
    rows = np.ascontiguousarray(piece_rows, dtype=np.float64).reshape(-1, len(CLEAR_EXACT_FIELDS))
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1)
    B = piece_off.size - 1
    if B >= 1 and (rows.shape[0] < int(piece_off.max()) or T.size < int(piece_off.max())):
        raise ValueError(f"clearance_exact_fold: {rows.shape[0]} rows and {T.size} durations for piece_off up to {int(piece_off.max())}")
    cand = np.zeros((max(B, 0), len(CLEAR_EXACT_FIELDS))); flags = np.zeros(max(B, 0), np.uint32)
    pad = np.zeros(1)
    _check(lib().frx_clearance_exact_fold(B, piece_off.ctypes.data, (T if T.size else pad).ctypes.data, (rows if rows.size else pad).ctypes.data,
                                          cand.ctypes.data, flags.ctypes.data))
    return cand, flags


def traj_to_msg(T, Cf):
    """PolynomialTrajectory array fields of one trajectory: (coef_x, coef_y, coef_z, time, order)."""
    n = len(T)
    cx = np.zeros(6 * n); cy = np.zeros(6 * n); cz = np.zeros(6 * n); tm = np.zeros(n); od = np.zeros(n, np.uint32)
    _check(lib().frx_traj_to_msg(n, np.ascontiguousarray(T, dtype=np.float64), np.ascontiguousarray(Cf, dtype=np.float64).reshape(-1), cx, cy, cz, tm, od))
    return cx, cy, cz, tm, od


def msg_sample(msg, t: float):
    cx, cy, cz, tm, od = msg
    p = np.zeros(3); v = np.zeros(3); a = np.zeros(3); j = np.zeros(3)
    _check(lib().frx_msg_sample(len(tm), cx, cy, cz, tm, od, float(t), p, v, a, j))
    return p, v, a, j


class MultiProblem:
    """A batch sharded over several devices behind the C ABI (frx_multi_*): one host thread and handle per device, RCCL winner exchange."""

    def __init__(self, cands, params: dict, devices=None, n_devices: int = 0, **override):
        self.cfg = FrxConfig.from_params(params, **override)
        coarse_n, ini, fin, h_off, h_rec, v_off, v_rec = pack_batch(cands)
        h = C.c_void_p()
        dev = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        nd = n_devices if devices is None else len(devices)
        _check(lib().frx_multi_create(C.byref(self.cfg), nd, None if dev is None else dev.ctypes.data, len(cands), coarse_n, ini, fin, h_off, h_rec, v_off, v_rec, C.byref(h)))
        self.h = h
        self.B = len(cands)
        g = C.c_int(); r = C.c_int()
        _check(lib().frx_multi_info(self.h, C.byref(g), C.byref(r), None, None))
        self.n_shards, self.uses_rccl = int(g.value), bool(r.value)
        self.shard_lo = np.zeros(self.n_shards + 1, np.int32); self.shard_device = np.zeros(self.n_shards, np.int32)
        _check(lib().frx_multi_info(self.h, None, None, self.shard_lo.ctypes.data, self.shard_device.ctypes.data))
        self.piece_off = np.zeros(self.B + 1, np.int32); self.x_off = np.zeros(self.B + 1, np.int32)
        _check(lib().frx_multi_layout(self.h, self.piece_off, self.x_off))
        self.P, self.NX = int(self.piece_off[-1]), int(self.x_off[-1])
        self.maxN = int(np.diff(self.piece_off).max())

    def close(self):
        if getattr(self, "h", None):
            lib().frx_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def initial_guess(self):
        x = np.zeros(self.NX)
        _check(lib().frx_multi_initial_guess(self.h, x))
        return x

    def optimize(self, rel_cost_tol: float, x0=None, max_iterations: int = 0):
        x = self.initial_guess() if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        pm = gcopter_lbfgs_params(rel_cost_tol, max_iterations)
        Cf = np.zeros(self.P * 18); T = np.zeros(self.P); jc = np.zeros(self.B); obj = np.zeros(self.B)
        st = np.zeros(self.B, np.int32); it = np.zeros(self.B, np.int32); ev = np.zeros(self.B, np.int32)
        wid = C.c_int(); wobj = C.c_double(); wn = C.c_int()
        wC = np.zeros(self.maxN * 18); wT = np.zeros(self.maxN)
        _check(lib().frx_multi_optimize(self.h, C.byref(pm), x, Cf, T, jc, obj, st, it, ev, C.byref(wid), C.byref(wobj), wC, wT, C.byref(wn)))
        n = int(wn.value)
        return dict(x=x, C=Cf.reshape(-1, 3), T=T, jerk_cost=jc, objective=obj, status=st, iters=it, evals=ev, winner_id=int(wid.value),
                    winner_objective=float(wobj.value), winner_C=wC[:18 * n].reshape(-1, 3).copy(), winner_T=wT[:n].copy(),
                    exchange="rccl" if lib().frx_multi_last_exchange(self.h) else "host")


class Problem:
    """A batch of candidate trajectories resident on one MI355X: the SE3GCOPTER::setup / optimize
    pair (CPU.hpp:1076, :1230) behind the C ABI."""

    def __init__(self, cands, params: dict, device: int = 0, enumerate_v: bool = False, packed=None, **override):
        self.cfg = FrxConfig.from_params(params, **override)
        self.kappa = int(self.cfg.qd_intervals)
        coarse_n, ini, fin, h_off, h_rec, v_off, v_rec = packed if packed is not None else pack_batch(cands)   # packed: pack_batch(cands) done by the caller (timing)
        h = C.c_void_p()
        if enumerate_v:      # V-polytopes from the library's own H->V enumeration (frx_problem_create_from_h)
            _check(lib().frx_problem_create_from_h(C.byref(self.cfg), device, len(cands), coarse_n, ini, fin, h_off, h_rec, C.byref(h)))
        else:
            _check(lib().frx_problem_create(C.byref(self.cfg), device, len(cands), coarse_n, ini, fin, h_off, h_rec, v_off, v_rec,
                                            C.byref(h)))
        self.h = h
        t = np.zeros(6, dtype=np.int32)
        _check(lib().frx_problem_totals(self.h, t))
        self.B, self.P, self.Pc, self.NX, self.Kmax, self.sum_K = (int(v) for v in t)
        self.piece_off = np.zeros(self.B + 1, np.int32); self.coarse_off = np.zeros(self.B + 1, np.int32)
        self.x_off = np.zeros(self.B + 1, np.int32); self.dim_t = np.zeros(self.B, np.int32)
        _check(lib().frx_problem_layout(self.h, self.piece_off, self.coarse_off, self.x_off, self.dim_t))

    def close(self):
        if getattr(self, "h", None):
            lib().frx_problem_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:          # interpreter shutdown: module globals may already be gone
            pass

    def set_solver(self, name: str):
        """'knot_pcr' (default) or 'banded_lu' (reference elimination order, cross-check)."""
        _check(lib().frx_problem_set_solver(self.h, {"knot_pcr": 0, "banded_lu": 1}[name]))

    def set_lbfgs_mode(self, name: str):
        """'device' (default: vectors on the GPU, decisions on the host) or 'host' (reference-exact host vectors)."""
        _check(lib().frx_problem_set_lbfgs_mode(self.h, {"device": 0, "host": 1}[name]))

    def set_resident(self, enable):
        """0 / False: one launch per stage and round; 1 / True: resident round kernel when the batch fits the chip, its work queue for batches up
        to a few times that size (default); 2: the work queue for every batch that exceeds the chip."""
        _check(lib().frx_problem_set_resident(self.h, int(enable)))

    def resident_clusters(self):
        """Clusters of the last resident plan (< B: the candidates went through the work queue)."""
        a = C.c_int()
        _check(lib().frx_debug_resident_clusters(self.h, C.byref(a)))
        return int(a.value)

    def optimize_path(self):
        """(resident_used, device_status) of the last optimize()."""
        u = C.c_int(); st = C.c_uint()
        _check(lib().frx_optimize_path(self.h, C.byref(u), C.byref(st)))
        return int(u.value), int(st.value)

    def trace(self):
        """Rows {flags, step, f, g.d, gp.d_new, x.x, g.g} of candidate 0's evaluated commands (needs FRX_TRACE in the environment)."""
        n = lib().frx_debug_trace(self.h, None, 0)
        out = np.zeros((max(n, 0), 7))
        if n > 0:
            lib().frx_debug_trace(self.h, out.ctypes.data, n)
        return out

    def direction_log(self, cap_steps: int, n_cands: int = 1):
        """Record (s, y, g, d) of every accepted step of later resident plans (frx_debug_direction_log); 0 switches it off."""
        _check(lib().frx_debug_direction_log(self.h, int(cap_steps), int(n_cands)))

    def read_direction_log(self, cand: int = 0):
        """dict(s, y, g, d: rows x nxp arrays; slot, bound: rows) of candidate `cand`'s accepted steps in the last resident plan."""
        rows = C.c_int(); rd = C.c_int()
        _check(lib().frx_debug_direction_log_read(self.h, cand, None, 0, C.byref(rows), C.byref(rd)))
        out = np.zeros((rows.value, rd.value))
        if rows.value:
            _check(lib().frx_debug_direction_log_read(self.h, cand, out.ctypes.data, rows.value, C.byref(rows), C.byref(rd)))
        nxp = (rd.value - 2) // 4
        return dict(s=out[:, :nxp], y=out[:, nxp:2 * nxp], g=out[:, 2 * nxp:3 * nxp], d=out[:, 3 * nxp:4 * nxp],
                    slot=out[:, 4 * nxp].astype(int), bound=out[:, 4 * nxp + 1].astype(int))

    def set_resident_retry(self, enable: bool):
        """Diagnostic: re-run candidates that fail on the resident kernel on the per-stage rounds (round-2 behaviour; default off)."""
        _check(lib().frx_debug_set_resident_retry(self.h, 1 if enable else 0))

    def set_takeover_at(self, rounds: int):
        """Tests (frx_debug_set_takeover_at): rounds > 0 = every plan starts as per-stage rounds and hands its candidates to the resident kernel after so many."""
        _check(lib().frx_debug_set_takeover_at(self.h, C.c_long(int(rounds))))

    def eval_status(self):
        """frx_eval_status: has a wait inside a one-launch evaluation expired since the last check?  Raises FrxError (FRX_ERR_TIMEOUT) if so; the caller's stream must be synchronised."""
        _check(lib().frx_eval_status(self.h))

    def taken_over(self) -> int:
        """Candidates of the last plan that began as per-stage rounds and finished on the resident round kernel (frx_debug_taken_over)."""
        n = C.c_int(0)
        _check(lib().frx_debug_taken_over(self.h, C.byref(n)))
        return int(n.value)

    def resident_predictions(self):
        """(rounds on a predicted ADVANCE, rounds on a predicted trial step, predictions redone) of the last resident plan, all candidates."""
        out = np.zeros(3, dtype=np.uint64)
        _check(lib().frx_debug_resident_predictions(self.h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def resident_counts(self):
        """(failed, retried) candidates of the last resident plan."""
        a = C.c_int(); b = C.c_int()
        _check(lib().frx_debug_resident_counts(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def resident_profile(self):
        """[S][G][16] microseconds per segment of the last resident plan, S clusters (needs FRX_RESIDENT_PROF in the environment)."""
        n = lib().frx_resident_profile(self.h, None, 0)
        if n <= 0:
            return None
        out = np.zeros(n, dtype=np.uint64)
        lib().frx_resident_profile(self.h, out.ctypes.data, n)
        self.last_stamps = out[-32:].astype(np.int64)                  # shader-clock stamps of candidate 0's forward (0..6) / adjoint (16..24) bodies
        body = out[:-32]
        S = self.resident_clusters()
        self.last_host_wait_hist = body[-16 * S:].reshape(S, 16).astype(np.int64)   # per leader: waits for a host command, bin k = shorter than 2^k us
        return body[:-16 * S].reshape(S, -1, 16).astype(np.float64) / 100.0

    def initial_guess(self):
        x = np.zeros(self.NX)
        _check(lib().frx_initial_guess(self.h, x))
        return x

    def objective(self, x):
        f = np.zeros(self.B); g = np.zeros(self.NX)
        _check(lib().frx_objective_eval(self.h, np.ascontiguousarray(x, dtype=np.float64), f, g))
        return f, g

    def objective_device(self, x_ptr: int, f_ptr: int, g_ptr: int, stream: int = 0):
        _check(lib().frx_objective_eval_device(self.h, x_ptr, f_ptr, g_ptr, stream))

    def penalty(self, T, Cf):
        cost = np.zeros(self.B); gdT = np.zeros(self.P); gdC = np.zeros(self.P * 18)
        _check(lib().frx_penalty_eval(self.h, np.ascontiguousarray(T, dtype=np.float64),
                                      np.ascontiguousarray(Cf, dtype=np.float64).reshape(-1), cost, gdT, gdC))
        return cost, gdT, gdC.reshape(-1, 3)

    def penalty_device(self, T_ptr: int, C_ptr: int, out_ptr: int, stream: int = 0):
        _check(lib().frx_penalty_eval_device(self.h, T_ptr, C_ptr, out_ptr, stream))

    def _traj_TC(self, who, T, Cf):
        """(T, Cf) of a trajectory_* call as flat float64 arrays of the handle's sizes"""
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1); Cf = np.ascontiguousarray(Cf, dtype=np.float64).reshape(-1)
        if T.size != self.P or Cf.size != 18 * self.P:
            raise ValueError(f"{who}: expected {self.P} durations and {18 * self.P} coefficients, got {T.size} and {Cf.size}")
        return T, Cf

    def _traj_folded(self, fields, cand_key, entry, *args):
        """dict(piece (P, n), <cand_key> (B, n), flags (B,) uint32) plus the candidate rows' n fields by name, filled by entry(handle, *args, piece, cand, flags)"""
        piece = np.zeros((self.P, len(fields))); cand = np.zeros((self.B, len(fields))); flags = np.zeros(self.B, np.uint32)
        _check(entry(self.h, *args, piece.ctypes.data, cand.ctypes.data, flags.ctypes.data))
        out = {"piece": piece, cand_key: cand, "flags": flags}
        out.update({name: cand[:, i] for i, name in enumerate(fields)})
        return out

    def trajectory_check(self, T, Cf, intervals: int = 256):
        """Dense feasibility certificate of the batch (T, C) against the handle's corridors and limits (frx_trajectory_check):
        dict(piece (P, 8), candidate (B, 8), flags (B,) uint32) plus the candidate rows' fields by name (CHECK_FIELDS)."""
        T, Cf = self._traj_TC("trajectory_check", T, Cf)
        return self._traj_folded(CHECK_FIELDS, "candidate", lib().frx_trajectory_check, T.ctypes.data, Cf.ctypes.data, int(intervals))

    def trajectory_check_device(self, T_ptr: int, C_ptr: int, out_ptr: int, intervals: int = 256, stream: int = 0):
        """frx_trajectory_check_device: the piece rows (P x 8 doubles at out_ptr) as one launch on `stream`, device pointers, no synchronisation."""
        _check(lib().frx_trajectory_check_device(self.h, T_ptr, C_ptr, int(intervals), out_ptr, stream))

    def trajectory_extrema(self, T, Cf):
        """Exact per-piece extrema of speed, acceleration, thrust and body rate of the batch (T, C) with the times they are attained at
        (frx_trajectory_extrema; nothing is sampled, the corridor is not covered): dict(piece (P, 10), cand (B, 10), flags (B,) uint32 of
        CHECK_FLAG_* bits) plus the candidate rows' fields by name (EXTREMA_FIELDS)."""
        T, Cf = self._traj_TC("trajectory_extrema", T, Cf)
        return self._traj_folded(EXTREMA_FIELDS, "cand", lib().frx_trajectory_extrema, T.ctypes.data, Cf.ctypes.data)

    def trajectory_extrema_device(self, T_ptr: int, C_ptr: int, out_ptr: int, stream: int = 0):
        """frx_trajectory_extrema_device: the piece rows (P x 10 doubles at out_ptr) as one launch on `stream`, device pointers, no synchronisation."""
        _check(lib().frx_trajectory_extrema_device(self.h, T_ptr, C_ptr, out_ptr, stream))

    def trajectory_contain(self, T, Cf, slack: float = 0.0):
        """Exact corridor containment certificate of the batch (T, C) (frx_trajectory_contain; nothing is sampled): every face pulled in by slack
        (0: the face of the check's CORRIDOR, safe_margin: the face the penalty aims at).  dict(piece (P, 8), cand (B, 8), flags (B,) uint32 of
        CHECK_FLAG_CORRIDOR / _NONFINITE) plus the candidate rows' fields by name (CONTAIN_FIELDS)."""
        T, Cf = self._traj_TC("trajectory_contain", T, Cf)
        return self._traj_folded(CONTAIN_FIELDS, "cand", lib().frx_trajectory_contain, T.ctypes.data, Cf.ctypes.data, float(slack))

    def trajectory_contain_device(self, T_ptr: int, C_ptr: int, out_ptr: int, slack: float = 0.0, stream: int = 0):
        """frx_trajectory_contain_device: the piece rows (P x 8 doubles at out_ptr) as one launch on `stream`, device pointers, no synchronisation;
        contain_fold gives its callers the candidate rows and flags."""
        _check(lib().frx_trajectory_contain_device(self.h, T_ptr, C_ptr, float(slack), out_ptr, stream))

    def trajectory_gates(self, T, Cf, gates, gate_off):
        """Exact gate passage certificate of the batch (T, C) (frx_trajectory_gates): gates (n_gates, 9) records {c, a, b}, candidate b owning the
        gates gate_off[b] .. gate_off[b + 1] - 1 in the order they are to be flown.  dict(gate (n_gates, 10), flags (B,) uint32 of GATE_FLAG_* bits)
        plus the rows' fields by name (GATE_FIELDS)."""
        T, Cf = self._traj_TC("trajectory_gates", T, Cf)
        gate_off = np.ascontiguousarray(gate_off, dtype=np.int32).reshape(-1)
        gates = np.ascontiguousarray(gates, dtype=np.float64)
        if gate_off.size != self.B + 1:
            raise ValueError(f"trajectory_gates: gate_off must hold {self.B + 1} offsets, got {gate_off.size}")
        if gates.ndim != 2 or gates.shape[1] != 9 or gates.shape[0] != int(gate_off[-1]):
            raise ValueError(f"trajectory_gates: gates must have shape ({int(gate_off[-1])}, 9), got {gates.shape}")
        rows = np.zeros((gates.shape[0], len(GATE_FIELDS))); flags = np.zeros(self.B, np.uint32)
        _check(lib().frx_trajectory_gates(self.h, T.ctypes.data, Cf.ctypes.data, gate_off.ctypes.data, gates.ctypes.data, rows.ctypes.data, flags.ctypes.data))
        out = {"gate": rows, "flags": flags}
        out.update({name: rows[:, i] for i, name in enumerate(GATE_FIELDS)})
        return out

    def trajectory_gates_device(self, T_ptr: int, C_ptr: int, n_gates: int, gate_off_ptr: int, gates_ptr: int, out_ptr: int, stream: int = 0):
        """frx_trajectory_gates_device: the gate rows (n_gates x 10 doubles at out_ptr) as one launch on `stream`, device pointers (gate_off_ptr: B + 1
        int32), no copy, no synchronisation, no allocation."""
        _check(lib().frx_trajectory_gates_device(self.h, T_ptr, C_ptr, int(n_gates), gate_off_ptr, gates_ptr, out_ptr, stream))

    def trajectory_sample(self, T, Cf, n_samples: int, dt: float = 0.0, t0: float = 0.0, times=None):
        """Every candidate of the batch (T, C) at n_samples times with its SE(3) outputs (frx_trajectory_sample): times (B, n_samples) from each
        candidate's start, else t0 + s dt (dt > 0) or n_samples points over each duration (dt == 0).  dict(rows (B, S, 20)) plus the named
        views of the rows (SAMPLE_VIEWS: pos, vel, acc, jerk (B, S, 3), thrust (B, S), quat (B, S, 4) as w, x, y, z, omega (B, S, 3))."""
        T, Cf = self._traj_TC("trajectory_sample", T, Cf)
        S = int(n_samples)
        tp = None
        if times is not None:
            times = np.ascontiguousarray(times, dtype=np.float64)
            if times.shape != (self.B, S):
                raise ValueError(f"trajectory_sample: times must have shape ({self.B}, {S}), got {times.shape}")
            tp = times.ctypes.data
        rows = np.empty((self.B, max(S, 0), SAMPLE_FIELDS))
        _check(lib().frx_trajectory_sample(self.h, T.ctypes.data, Cf.ctypes.data, S, float(t0), float(dt), tp, rows.ctypes.data))
        out = dict(rows=rows)
        out.update({name: rows[..., sl] for name, sl in SAMPLE_VIEWS.items()})
        return out

    def trajectory_sample_device(self, T_ptr: int, C_ptr: int, out_ptr: int, n_samples: int, dt: float = 0.0, t0: float = 0.0, times_ptr: int = 0,
                                 stream: int = 0):
        """frx_trajectory_sample_device: the rows (B x n_samples x 20 doubles at out_ptr, 16-byte aligned) as one launch on `stream`, device pointers
        (times_ptr = 0: no times array), no copy, no synchronisation."""
        _check(lib().frx_trajectory_sample_device(self.h, T_ptr, C_ptr, int(n_samples), float(t0), float(dt), times_ptr or None, out_ptr, stream))

    def trajectory_clearance(self, T, Cf, obs, intervals: int = 256):
        """Clearance of the batch (T, C) against the obstacle cloud obs (n_obs, 3) (frx_trajectory_clearance): dict(piece (P, 4), cand (B, 4),
        flags (B,) uint32) plus the candidate rows' fields by name (CLEAR_FIELDS: ell >= 1 means free, dist in metres, worst_t, worst_i)."""
        T, Cf = self._traj_TC("trajectory_clearance", T, Cf)
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 2 or obs.shape[1] != 3:
            raise ValueError(f"trajectory_clearance: obs must have shape (n_obs, 3), got {obs.shape}")
        return self._traj_folded(CLEAR_FIELDS, "cand", lib().frx_trajectory_clearance, T.ctypes.data, Cf.ctypes.data, int(intervals), obs.shape[0], obs.ctypes.data)

    def trajectory_clearance_workspace(self, n_obs: int, intervals: int = 256) -> int:
        """frx_trajectory_clearance_workspace: bytes of scratch trajectory_clearance_device needs for a cloud of n_obs points (0: none)."""
        n = C.c_size_t(0)
        _check(lib().frx_trajectory_clearance_workspace(self.h, int(intervals), int(n_obs), C.byref(n)))
        return int(n.value)

    def trajectory_clearance_device(self, T_ptr: int, C_ptr: int, obs_ptr: int, n_obs: int, work_ptr: int, out_ptr: int, intervals: int = 256, stream: int = 0):
        """frx_trajectory_clearance_device: the piece rows (P x 4 doubles at out_ptr) as pure launches on `stream`, device pointers (work_ptr: the scratch
        trajectory_clearance_workspace asks for, 0 when that is 0), no copy, no synchronisation, no allocation."""
        _check(lib().frx_trajectory_clearance_device(self.h, T_ptr, C_ptr, int(intervals), int(n_obs), obs_ptr, work_ptr or None, out_ptr, stream))

    def trajectory_clearance_exact(self, T, Cf, obs):
        """Exact clearance certificate of the batch (T, C) against the obstacle cloud obs (n_obs, 3) (frx_trajectory_clearance_exact; nothing is sampled):
        dict(piece (P, 6), cand (B, 6), flags (B,) uint32 of CLEAR_FLAG_*) plus the candidate rows' fields by name (CLEAR_EXACT_FIELDS)."""
        T, Cf = self._traj_TC("trajectory_clearance_exact", T, Cf)
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 2 or obs.shape[1] != 3:
            raise ValueError(f"trajectory_clearance_exact: obs must have shape (n_obs, 3), got {obs.shape}")
        return self._traj_folded(CLEAR_EXACT_FIELDS, "cand", lib().frx_trajectory_clearance_exact, T.ctypes.data, Cf.ctypes.data, obs.shape[0], obs.ctypes.data)

    def trajectory_clearance_exact_workspace(self, n_obs: int) -> int:
        """frx_trajectory_clearance_exact_workspace: bytes of scratch trajectory_clearance_exact_device needs for a cloud of n_obs points."""
        n = C.c_size_t(0)
        _check(lib().frx_trajectory_clearance_exact_workspace(self.h, int(n_obs), C.byref(n)))
        return int(n.value)

    def trajectory_clearance_exact_device(self, T_ptr: int, C_ptr: int, obs_ptr: int, n_obs: int, work_ptr: int, out_ptr: int, stream: int = 0):
        """frx_trajectory_clearance_exact_device: the piece rows (P x 6 doubles at out_ptr) as pure launches on `stream`, device pointers (work_ptr: the
        scratch trajectory_clearance_exact_workspace asks for), no copy, no synchronisation, no allocation; clearance_exact_fold gives the candidate rows."""
        _check(lib().frx_trajectory_clearance_exact_device(self.h, T_ptr, C_ptr, int(n_obs), obs_ptr, work_ptr or None, out_ptr, stream))

    def trajectory_map_distance(self, T, Cf, vmap, field, margin: float = 0.0, intervals: int = 256):
        """The batch (T, C) screened against `field`, a float64 array over the cells of the VoxelMap vmap - pos or all of its esdf(), or the caller's own
        (frx_trajectory_map_distance): dict(piece (P, 4), cand (B, 4), flags (B,) uint32 of MAPDIST_FLAG_*) plus the candidate rows' fields by name
        (MAPDIST_FIELDS: dist, worst_t, worst_cell, outside)."""
        T, Cf = self._traj_TC("trajectory_map_distance", T, Cf)
        field = np.ascontiguousarray(field, dtype=np.float64).reshape(-1)
        if field.size != vmap.cells.size:
            raise ValueError(f"trajectory_map_distance: field must hold {vmap.cells.size} values, got {field.size}")
        return self._traj_folded(MAPDIST_FIELDS, "cand", lib().frx_trajectory_map_distance, T.ctypes.data, Cf.ctypes.data, int(intervals), C.cast(C.pointer(vmap._s), C.c_void_p),
                                 field.ctypes.data, float(margin))

    def trajectory_map_distance_device(self, T_ptr: int, C_ptr: int, map_struct, field_ptr: int, out_ptr: int, intervals: int = 256, stream: int = 0):
        """frx_trajectory_map_distance_device: the piece rows (P x 4 doubles at out_ptr) as one launch on `stream`, device pointers (map_struct: a VoxelMapStruct,
        its cells are not read), no copy, no synchronisation, no allocation; map_distance_fold gives the candidate rows."""
        _check(lib().frx_trajectory_map_distance_device(self.h, T_ptr, C_ptr, int(intervals), C.byref(map_struct), field_ptr or None, out_ptr or None, stream))

    def set_clear_exact(self, chunk_points: int = 0, cull_on: bool = True):
        """Tests (frx_debug_set_clear_exact): cloud points per chunk of every later exact clearance call on the handle (0 = the library's own split) and
        whether points are culled at all."""
        _check(lib().frx_debug_set_clear_exact(self.h, int(chunk_points), int(bool(cull_on))))

    def clear_exact_counts(self):
        """Tests (frx_debug_clear_exact_counts): (survivors (P,), degree-21 tasks (P,)) int32 of the last exact clearance call on the handle."""
        s = np.zeros(self.P, np.int32); e = np.zeros(self.P, np.int32)
        _check(lib().frx_debug_clear_exact_counts(self.h, s.ctypes.data, e.ctypes.data))
        return s, e

    def set_clear_chunk(self, points: int):
        """Tests (frx_debug_set_clear_chunk): cloud points per chunk of every later clearance call on the handle, 0 = the library's own split."""
        _check(lib().frx_debug_set_clear_chunk(self.h, int(points)))

    def forward(self, x):
        T = np.zeros(self.P); Cf = np.zeros(self.P * 18)
        _check(lib().frx_forward(self.h, np.ascontiguousarray(x, dtype=np.float64), T, Cf))
        return T, Cf.reshape(-1, 3)

    def optimize(self, rel_cost_tol: float, x0=None, max_iterations: int = 0):
        x = self.initial_guess() if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        pm = gcopter_lbfgs_params(rel_cost_tol, max_iterations)
        Cf = np.zeros(self.P * 18); T = np.zeros(self.P)
        jc = np.zeros(self.B); obj = np.zeros(self.B)
        st = np.zeros(self.B, np.int32); it = np.zeros(self.B, np.int32); ev = np.zeros(self.B, np.int32)
        _check(lib().frx_optimize(self.h, C.byref(pm), x, Cf, T, jc, obj, st, it, ev))
        stats = np.zeros(4)
        _check(lib().frx_optimize_stats(self.h, stats))
        resident, dev_status = self.optimize_path()
        return dict(x=x, C=Cf.reshape(-1, 3), T=T, jerk_cost=jc, objective=obj, status=st, iters=it, evals=ev,
                    ms_total=stats[0], ms_device=stats[1], ms_host=stats[2], rounds=int(stats[3]), resident=resident, device_status=dev_status,
                    resident_failed=self.resident_counts()[0], resident_retried=self.resident_counts()[1], predictions=self.resident_predictions(),
                    clusters=self.resident_clusters() if resident else 0, taken_over=self.taken_over())

    def stage_times(self, x, reps: int = 100):
        """Average microseconds of the forward, penalty and adjoint kernels at x (HIP events inside the library)."""
        out = np.zeros(3)
        _check(lib().frx_eval_stage_times(self.h, np.ascontiguousarray(x, dtype=np.float64), reps, out))
        return {"forward": float(out[0]), "penalty": float(out[1]), "adjoint": float(out[2])}

    def eval_launch_time(self, x, reps: int = 100) -> float:
        """Average microseconds of one evaluation at x in the form frx_objective_eval_device takes (HIP events inside the library)."""
        out = np.zeros(1)
        _check(lib().frx_eval_launch_time(self.h, np.ascontiguousarray(x, dtype=np.float64), reps, out))
        return float(out[0])

    def profile_eval_cluster(self, x):
        """Shader-clock stamps of cluster 0 during one evaluation in the one-launch form (frx_debug.h: frx_debug_profile_eval_cluster)."""
        out = np.zeros(64, np.int64)
        _check(lib().frx_debug_profile_eval_cluster(self.h, np.ascontiguousarray(x, dtype=np.float64), out.ctypes.data))
        return out

    def profile_eval_tail(self, x):
        """The same with the stamps of the evaluation's tail in [64..68] and of the hand-off of the penalty partials in [69..74] (frx_debug.h: frx_debug_profile_eval_tail);
        100 MHz ticks from [40] on, except [75] and [76], which are spin counts and no times."""
        out = np.zeros(80, np.int64)
        _check(lib().frx_debug_profile_eval_tail(self.h, np.ascontiguousarray(x, dtype=np.float64), out.ctypes.data))
        return out

    def profile_eval_forward(self, x):
        """The same with the stamps of the forward map's prelude in [80..110] (frx_debug.h: frx_debug_profile_eval_forward): wave 0 of the leader [80..84] and of the last
        member with a task [88..92], axis wave 1 of the leader [96..110]; 100 MHz ticks."""
        out = np.zeros(112, np.int64)
        _check(lib().frx_debug_profile_eval_forward(self.h, np.ascontiguousarray(x, dtype=np.float64), out.ctypes.data))
        return out

    def set_eval_fused(self, on: bool):
        """Diagnostic: False = evaluations as three stage launches, True = the default (one launch where it applies, frx_eval_kernel.hpp)."""
        _check(lib().frx_debug_set_eval_fused(self.h, int(on)))          # (2: test mode - every wait inside the launch expires at once)

    def eval_fused(self) -> int:
        """Workgroups per candidate of the one-launch evaluation in use, 0 = one launch per stage."""
        return int(lib().frx_debug_eval_fused(self.h))

    def eval_geometry(self) -> int:
        """1 = the one-launch evaluation of this handle launches the compile-time geometry class (frx_eval_kernel.hpp, EvalGeomK16), 0 = the run-time form."""
        return int(lib().frx_debug_eval_geometry(self.h))

    def eval_front(self) -> int:
        """1 = the one-launch evaluation of this handle takes the two-trip front (frx_eval_kernel.hpp, FR: front records and the argument block's leading lines), 0 = the
        front that walks the offset tables (FRX_EVAL_FRONT=0, or a form without it)."""
        return int(lib().frx_debug_eval_front(self.h))

    def eval_prelude(self) -> int:
        """1 = the forward map of this handle's one-launch evaluation takes the shortened prelude (frx_eval_kernel.hpp, PRE), 0 = the form before (FRX_EVAL_PRELUDE=0, or
        a form without the two-trip front and the value-major hand-off)."""
        return int(lib().frx_debug_eval_prelude(self.h))

    def eval_adjoint(self) -> int:
        """1 = the leader of this handle's one-launch evaluation runs the adjoint with its operands in front of the poll (frx_eval_kernel.hpp, ADJ), 0 = the form before
        (FRX_EVAL_ADJOINT=0, or a form without the shortened prelude)."""
        return int(lib().frx_debug_eval_adjoint(self.h))

    def set_eval_solo(self, mode: int):
        """Diagnostic: 0 = never the solo form (one workgroup per candidate, one launch per evaluation, frx_solo_kernel.hpp), 1 = from the handle's batch-size
        threshold on (default), 2 = at every batch size."""
        _check(lib().frx_debug_set_eval_solo(self.h, int(mode)))

    def solo_applies(self) -> bool:
        """Does the solo form exist for this handle's geometry (<= 64 pieces and samples per piece, knot solver)?"""
        was = int(lib().frx_debug_set_eval_solo(self.h, 2))
        if was != 0: return False
        ok = self.eval_solo() >= 1
        _check(lib().frx_debug_set_eval_solo(self.h, 1))
        return ok

    def eval_solo(self) -> int:
        """Workgroups of the solo kernel a CU holds if the next evaluation takes that form, 0 = it does not."""
        return int(lib().frx_debug_eval_solo(self.h))

    def mailbox_numa(self):
        """{NUMA node of the resident plan's command / result mailbox pages, the device's node, the caller's CPU}; -1 = unknown."""
        out = np.zeros(4, np.int32)
        _check(lib().frx_debug_mailbox_numa(self.h, out.ctypes.data))
        return {"cmd_node": int(out[0]), "res_node": int(out[1]), "device_node": int(out[2]), "caller_cpu": int(out[3])}

    def penalty_kernel(self) -> str:
        """Name of the penalty kernel a stage launch of this handle takes."""
        return {0: "frx::k_penalty", 1: "frx::k_penalty_lat", 2: "frx::k_penalty_lat2"}.get(int(lib().frx_debug_penalty_kernel(self.h)), "?")

    def algorithmic_bytes(self) -> int:
        """Penalty-kernel bytes per evaluation, SURVEY.md §8d: sum over pieces of 312 + 48 K_i."""
        return 312 * self.P + 48 * self.sum_K

    def samples(self) -> int:
        """constraint samples per evaluation: pieces x (kappa + 1)."""
        return self.P * (self.kappa + 1)


class PenaltyProblem(Problem):
    """The inner boundary on its own (frx_penalty_problem_create): a handle built from what cuda_computer::compute receives on every call - per piece the index of
    its H-polytope (idxHs), the polytopes (cfgHs), the scalar limits and weights - serving `penalty` / `penalty_device` only (cuda_computer.cuh:118-134)."""

    def __init__(self, params: dict, piece_n, piece_poly, h_polys, device: int = 0, **override):
        self.cfg = FrxConfig.from_params(params, **override)
        self.kappa = int(self.cfg.qd_intervals)
        piece_n = np.ascontiguousarray(piece_n, dtype=np.int32); piece_poly = np.ascontiguousarray(piece_poly, dtype=np.int32)
        h_off = np.zeros(len(h_polys) + 1, dtype=np.int32)
        for i, hp in enumerate(h_polys):
            h_off[i + 1] = h_off[i] + hp.shape[1]
        h_rec = np.ascontiguousarray(np.concatenate([hp.T.reshape(-1) for hp in h_polys]), dtype=np.float64)
        h = C.c_void_p()
        _check(lib().frx_penalty_problem_create(C.byref(self.cfg), device, len(piece_n), C.c_void_p(piece_n.ctypes.data), C.c_void_p(piece_poly.ctypes.data),
                                                C.c_void_p(h_off.ctypes.data), C.c_void_p(h_rec.ctypes.data), C.byref(h)))
        self.h = h
        t = np.zeros(6, dtype=np.int32)
        _check(lib().frx_problem_totals(self.h, t))
        self.B, self.P, self.Pc, self.NX, self.Kmax, self.sum_K = (int(v) for v in t)
        self.piece_off = np.zeros(self.B + 1, np.int32); self.coarse_off = np.zeros(self.B + 1, np.int32)
        self.x_off = np.zeros(self.B + 1, np.int32); self.dim_t = np.zeros(self.B, np.int32)
        _check(lib().frx_problem_layout(self.h, self.piece_off, self.coarse_off, self.x_off, self.dim_t))
