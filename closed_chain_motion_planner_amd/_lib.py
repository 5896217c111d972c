"""ctypes binding of libccmp.so (include/ccmp.h).  Fails loudly when the library is missing:
there is no CPU implementation of the hot path in this package."""
import ctypes as C
import os

from .build import LIBPATH


class CcmpError(RuntimeError):
    def __init__(self, code, what, detail=""):
        self.code = code
        super().__init__("%s failed: %s (%d)%s" % (what, _strerror(code), code, (" — " + detail) if detail else ""))


class CcmpProblem(C.Structure):
    """ccmp_problem of include/ccmp.h (row-major matrices)."""

    _fields_ = [
        ("axis", C.c_double * 42),
        ("offset", C.c_double * 42),
        ("ee", C.c_double * 6),
        ("R_tool", C.c_double * 18),
        ("base_R", C.c_double * 18),
        ("base_p", C.c_double * 6),
        ("init_R", C.c_double * 9),
        ("init_p", C.c_double * 3),
        ("lb", C.c_double * 7),
        ("ub", C.c_double * 7),
        ("joint_eps", C.c_double),
        ("tol_pos", C.c_double),
        ("tol_rot", C.c_double),
        ("step", C.c_double),
        ("delta", C.c_double),
        ("lambda_", C.c_double),
        ("start_joint", C.c_double * 14),
        ("obj_start_R", C.c_double * 9),
        ("obj_start_p", C.c_double * 3),
        ("obj_goal_R", C.c_double * 9),
        ("obj_goal_p", C.c_double * 3),
        ("t_o7_R", C.c_double * 18),
        ("t_o7_p", C.c_double * 6),
        ("max_iter", C.c_int32),
        ("jacobian_mode", C.c_int32),
        ("arm_index", C.c_int32 * 2),
    ]

    def copy(self):
        return CcmpProblem.from_buffer_copy(bytes(self))


class CcmpIkOpts(C.Structure):
    """ccmp_ik_opts of include/ccmp.h"""
    _fields_ = [("restarts", C.c_int32), ("max_rounds", C.c_int32), ("eps", C.c_double), ("lambda_", C.c_double), ("err_clamp", C.c_double),
                ("sigma", C.c_double)]


class CcmpSphere(C.Structure):
    """ccmp_sphere of include/ccmp.h"""
    _fields_ = [("frame", C.c_int32), ("group", C.c_int32), ("c", C.c_double * 3), ("r", C.c_double)]


class CcmpBox(C.Structure):
    """ccmp_box of include/ccmp.h"""
    _fields_ = [("group", C.c_int32), ("reserved", C.c_int32), ("c", C.c_double * 3), ("R", C.c_double * 9), ("half", C.c_double * 3)]


class CcmpDenseOpts(C.Structure):
    """ccmp_dense_opts of include/ccmp.h"""
    _fields_ = [("flags", C.c_int), ("chunk_states", C.c_int), ("round_budget", C.c_int), ("max_calls", C.c_int)]


class CcmpShortcutOpts(C.Structure):
    """ccmp_shortcut_opts of include/ccmp.h"""
    _fields_ = [("max_span", C.c_int), ("chunk_states", C.c_int), ("round_budget", C.c_int), ("max_calls", C.c_int), ("tile_edges", C.c_int)]


class CcmpSmoothOpts(C.Structure):
    """ccmp_smooth_opts of include/ccmp.h"""
    _fields_ = [("max_steps", C.c_int), ("min_change", C.c_double), ("chunk_states", C.c_int), ("round_budget", C.c_int), ("max_calls", C.c_int),
                ("tile_edges", C.c_int)]


class CcmpResampleOpts(C.Structure):
    """ccmp_resample_opts of include/ccmp.h"""
    _fields_ = [("count", C.c_int), ("spacing", C.c_double), ("max_rows", C.c_int)]


class CcmpSetpointOpts(C.Structure):
    """ccmp_setpoint_opts of include/ccmp.h"""
    _fields_ = [("period", C.c_double), ("max_ticks", C.c_int)]


class CcmpFitOpts(C.Structure):
    """ccmp_fit_opts of include/ccmp.h"""
    _fields_ = [("period", C.c_double), ("max_ticks", C.c_int), ("aim", C.c_double), ("max_passes", C.c_int)]


class CcmpJerkOpts(C.Structure):
    """ccmp_jerk_opts of include/ccmp.h"""
    _fields_ = [("period", C.c_double), ("max_ticks", C.c_int), ("window", C.c_int), ("max_window", C.c_int), ("aim", C.c_double), ("tile_ticks", C.c_int)]


class CcmpPlanOpts(C.Structure):
    """ccmp_plan_opts of include/ccmp.h"""
    _fields_ = [("width", C.c_int32), ("k", C.c_int32), ("attempts", C.c_int32), ("max_states", C.c_int32), ("t", C.c_double), ("sigma", C.c_double),
                ("inflate", C.c_double), ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("max_vertices", C.c_uint64)]


class CcmpPlanCounters(C.Structure):
    """ccmp_plan_counters of include/ccmp.h"""
    _fields_ = [(n, C.c_int32) for n in ("proposals", "valid_proposals", "ik_successes", "vertices_kept", "mid_stones", "unsettled", "checks", "goal_pushes",
                                         "start_pushes", "ladder_vertices", "push_refused", "reserved")]


class CcmpPlanState(C.Structure):
    """ccmp_plan_state of include/ccmp.h"""
    _fields_ = [("n_starts", C.c_int32), ("n_goals", C.c_int32), ("starts", C.c_int32 * 8), ("goals", C.c_int32 * 8), ("nearest", C.c_int32),
                ("sprevious", C.c_int32), ("status", C.c_int32), ("cycle", C.c_int32), ("solved_start", C.c_int32), ("solved_goal", C.c_int32),
                ("size_at_check", C.c_int32), ("reserved", C.c_int32), ("next_index", C.c_uint64), ("nearest_pose", C.c_double * 8),
                ("prev_from_goal", C.c_double), ("prev_from_start", C.c_double), ("counters", CcmpPlanCounters)]


class CcmpPlanReport(C.Structure):
    """ccmp_plan_report of include/ccmp.h"""
    _fields_ = [("status", C.c_int32), ("cycles_run", C.c_int32), ("cycles_total", C.c_int32), ("reserved", C.c_int32), ("size", C.c_uint64),
                ("edges", C.c_uint64), ("solved_start", C.c_int32), ("solved_goal", C.c_int32), ("nearest", C.c_int32), ("reserved2", C.c_int32),
                ("prev_from_goal", C.c_double), ("prev_from_start", C.c_double), ("counters", CcmpPlanCounters)]


class CcmpRrtcOpts(C.Structure):
    """ccmp_rrtc_opts of include/ccmp.h"""
    _fields_ = [("width", C.c_int32), ("max_states", C.c_int32), ("round_budget", C.c_int32), ("reserved", C.c_int32), ("range", C.c_double),
                ("max_vertices", C.c_uint64)]


class CcmpRrtcCounters(C.Structure):
    """ccmp_rrtc_counters of include/ccmp.h"""
    _fields_ = [(n, C.c_int32) for n in ("samples", "projected", "trapped", "advanced", "reached", "unsettled", "connect_reached", "connect_added",
                                         "connect_nothing", "vertices", "edges", "reserved")]


class CcmpRrtcState(C.Structure):
    """ccmp_rrtc_state of include/ccmp.h"""
    _fields_ = [("n_starts", C.c_int32), ("n_goals", C.c_int32), ("starts", C.c_int32 * 8), ("goals", C.c_int32 * 8), ("status", C.c_int32), ("cycle", C.c_int32),
                ("next_index", C.c_uint64), ("solved_start", C.c_int32), ("solved_goal", C.c_int32), ("best_a", C.c_int32), ("best_b", C.c_int32),
                ("best_gap", C.c_double), ("counters", CcmpRrtcCounters)]


class CcmpRrtcReport(C.Structure):
    """ccmp_rrtc_report of include/ccmp.h"""
    _fields_ = [("status", C.c_int32), ("cycles_run", C.c_int32), ("cycles_total", C.c_int32), ("reserved", C.c_int32), ("size", C.c_uint64),
                ("edges", C.c_uint64), ("solved_start", C.c_int32), ("solved_goal", C.c_int32), ("best_a", C.c_int32), ("best_b", C.c_int32),
                ("best_gap", C.c_double), ("counters", CcmpRrtcCounters)]


CCMP_JAC_FD = 0
CCMP_JAC_ANALYTIC = 1

# every symbol include/ccmp.h declares (tests check the library exports all of them)
EXPORTS = [
    "ccmp_problem_from_yaml", "ccmp_problem_init", "ccmp_set_arms", "ccmp_set_base_frame", "ccmp_set_start", "ccmp_set_tolerance", "ccmp_set_calibration",
    "ccmp_ctx_create", "ccmp_ctx_destroy", "ccmp_ctx_set_waves_per_cu", "ccmp_ctx_set_schedule", "ccmp_ctx_set_option", "ccmp_ctx_get_option", "ccmp_ctx_option_info", "ccmp_ctx_describe", "ccmp_ctx_set_lpt", "ccmp_ctx_device", "ccmp_ctx_num_cus",
    "ccmp_function_batch", "ccmp_project_batch", "ccmp_is_satisfied_batch", "ccmp_joint_valid_batch",
    "ccmp_sample_project_batch", "ccmp_sample_near_project_batch", "ccmp_sample_gaussian_project_batch",
    "ccmp_compute_t_wo_batch", "ccmp_geodesic_batch", "ccmp_check_motion_batch", "ccmp_geodesic_batch_ex", "ccmp_geodesic_host_ex", "ccmp_check_motion_host", "ccmp_ambient_uniform_batch", "ccmp_enforce_bounds_batch", "ccmp_compact_valid", "ccmp_compact_valid_capped",
    "ccmp_project_host", "ccmp_function_host", "ccmp_is_satisfied_host", "ccmp_joint_valid_host", "ccmp_sample_project_host", "ccmp_sample_ref_project_host", "ccmp_geodesic_host", "ccmp_project_sharded_host", "ccmp_sample_project_sharded_host", "ccmp_sharded_host_last_timing",
    "ccmp_comm_create", "ccmp_comm_destroy", "ccmp_comm_last_timing", "ccmp_project_sharded", "ccmp_sample_project_sharded",
    "ccmp_scene_create", "ccmp_scene_destroy", "ccmp_scene_num_pairs", "ccmp_clearance_batch", "ccmp_clearance_host",
    "ccmp_geodesic_scene_batch", "ccmp_geodesic_scene_host",
    "ccmp_knn_batch", "ccmp_knn_host", "ccmp_connect_batch", "ccmp_connect_host",
    "ccmp_pose_distance", "ccmp_pose_from_t_wo",
    "ccmp_roadmap_create", "ccmp_roadmap_destroy", "ccmp_roadmap_size", "ccmp_roadmap_reserve", "ccmp_roadmap_append", "ccmp_roadmap_set_joints",
    "ccmp_roadmap_truncate", "ccmp_roadmap_read", "ccmp_roadmap_knn", "ccmp_roadmap_connect",
    "ccmp_roadmap_append_host", "ccmp_roadmap_set_joints_host", "ccmp_roadmap_read_host", "ccmp_roadmap_knn_host", "ccmp_roadmap_connect_host",
    "ccmp_ik_opts_default", "ccmp_pose_ik_batch", "ccmp_pose_ik_host", "ccmp_pose_ik_ref", "ccmp_roadmap_grow", "ccmp_roadmap_grow_host",
    "ccmp_arm_clearance_batch", "ccmp_arm_clearance_host", "ccmp_arm_clearance_ref", "ccmp_pose_ik_vetted_batch", "ccmp_pose_ik_vetted_host",
    "ccmp_pose_ik_vetted_ref", "ccmp_roadmap_grow_vetted", "ccmp_roadmap_grow_vetted_host",
    "ccmp_pose_interpolate", "ccmp_object_create", "ccmp_object_destroy", "ccmp_object_num_triangles",
    "ccmp_object_valid_batch", "ccmp_object_valid_host", "ccmp_object_valid_ref", "ccmp_object_propose_batch", "ccmp_object_propose_host", "ccmp_object_propose_ref",
    "ccmp_joint_distance", "ccmp_graph_labels_ref", "ccmp_roadmap_commit", "ccmp_roadmap_commit_host", "ccmp_roadmap_commit_ref",
    "ccmp_roadmap_add_edges", "ccmp_roadmap_add_edges_host", "ccmp_roadmap_num_edges", "ccmp_roadmap_read_edges", "ccmp_roadmap_read_edges_host",
    "ccmp_roadmap_read_labels", "ccmp_roadmap_read_labels_host", "ccmp_roadmap_closest", "ccmp_roadmap_closest_host", "ccmp_roadmap_closest_ref",
    "ccmp_roadmap_shortest_paths", "ccmp_roadmap_shortest_paths_host", "ccmp_graph_shortest_paths_ref", "ccmp_roadmap_path_rounds_host",
    "ccmp_dense_opts_default", "ccmp_path_densify", "ccmp_path_densify_host", "ccmp_dense_paths_info", "ccmp_dense_paths_copy", "ccmp_dense_paths_copy_host",
    "ccmp_dense_paths_destroy", "ccmp_dense_layout_ref", "ccmp_dense_arc_ref",
    "ccmp_shortcut_opts_default", "ccmp_path_shortcut", "ccmp_path_shortcut_host", "ccmp_shortcut_select", "ccmp_shortcut_select_host",
    "ccmp_shortcut_select_ref", "ccmp_shortcut_pairs_ref",
    "ccmp_smooth_opts_default", "ccmp_path_smooth", "ccmp_path_smooth_host", "ccmp_smooth_mid_ref", "ccmp_smooth_len_after",
    "ccmp_smooth_last_counts",
    "ccmp_resample_opts_default", "ccmp_path_resample", "ccmp_sampled_paths_info", "ccmp_sampled_paths_copy", "ccmp_sampled_paths_copy_host",
    "ccmp_sampled_paths_destroy", "ccmp_path_timestamps", "ccmp_path_timestamps_host", "ccmp_path_timestamps_ref", "ccmp_arc_bracket_ref",
    "ccmp_resample_targets_ref",
    "ccmp_setpoint_opts_default", "ccmp_path_setpoints", "ccmp_path_setpoints_host", "ccmp_setpoints_info", "ccmp_setpoints_copy", "ccmp_setpoints_copy_host",
    "ccmp_setpoints_destroy", "ccmp_setpoints_ref", "ccmp_setpoint_tangents_ref",
    "ccmp_fit_opts_default", "ccmp_path_fit_timestamps", "ccmp_path_fit_timestamps_host", "ccmp_path_fit_timestamps_ref",
    "ccmp_jerk_opts_default", "ccmp_path_jerk_setpoints", "ccmp_path_jerk_setpoints_host", "ccmp_jerk_setpoints_info", "ccmp_jerk_setpoints_copy",
    "ccmp_jerk_setpoints_copy_host", "ccmp_jerk_setpoints_destroy", "ccmp_jerk_setpoints_ref", "ccmp_jerk_next_window_ref",
    "ccmp_plan_default_opts", "ccmp_plan_create", "ccmp_plan_run", "ccmp_plan_state_read", "ccmp_plan_destroy", "ccmp_plan_check_ref", "ccmp_plan_prefix_ref",
    "ccmp_plan_connected_ref",
    "ccmp_rrtc_default_opts", "ccmp_rrtc_create", "ccmp_rrtc_run", "ccmp_rrtc_state_read", "ccmp_rrtc_destroy", "ccmp_roadmap_nearest_in_tree",
    "ccmp_roadmap_nearest_in_tree_host", "ccmp_roadmap_nearest_in_tree_ref", "ccmp_rrtc_nearest_shape", "ccmp_rrtc_pick_ref", "ccmp_rrtc_connected_ref",
    "ccmp_rrtc_pick_batch",
    "ccmp_strerror",
    "ccmp_last_hip_error", "ccmp_version", "ccmp_problem_sizeof",
]

_lib = None
# include/ccmp_debug.h: exported by lib/libccmp_debug.so only (the same sources with -DCCMP_DEBUG_HOOKS; select it with CCMP_LIBRARY)
DEBUG_EXPORTS = ["ccmp_detmath_probe", "ccmp_detmath_div_probe", "ccmp_ctx_set_order_experimental", "ccmp_ctx_debug_lpt_pred", "ccmp_debug_fail_calls",
                 "ccmp_ctx_debug_lpt_order", "ccmp_debug_sort_probe", "ccmp_debug_split_probe", "ccmp_detmath_round_facts_probe", "ccmp_ctx_debug_fd_state"]
DEBUG_LIBPATH = os.path.join(os.path.dirname(LIBPATH), "libccmp_debug.so")


def lib():
    """The loaded libccmp.so; raises if it has not been built (python -m closed_chain_motion_planner_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIBPATH):
        raise ImportError(
            "libccmp.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc, gfx950). There is no CPU fallback." % LIBPATH)
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7 and must be the one that
    # initialises the device if it is going to own the memory we launch on.  Loading libccmp.so first
    # would pull /opt/rocm's copy in, and the device then fails to open for whichever comes second
    # (seen on the GPU box: "no usable HIP device").  Importing torch first makes the loader resolve
    # libccmp's libamdhip64.so.7 dependency to the already-loaded runtime.
    try:
        import torch  # noqa: F401
    except ImportError:  # C-only consumers link libccmp.so against the system ROCm directly
        pass
    L = C.CDLL(LIBPATH)
    dp, u8p, u16p, vp = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.c_void_p
    pp, i32p = C.POINTER(CcmpProblem), C.POINTER(C.c_int32)
    sig = {
        "ccmp_problem_from_yaml": ([C.c_char_p, pp], C.c_int),
        "ccmp_problem_init": ([pp, C.c_char_p, C.c_int, C.c_char_p, C.c_int, dp, dp, dp, dp, dp], C.c_int),
        "ccmp_set_arms": ([pp, C.c_char_p, C.c_int, C.c_char_p, C.c_int], C.c_int),
        "ccmp_set_start": ([pp, dp], C.c_int),
        "ccmp_set_tolerance": ([pp, C.c_double, C.c_double], C.c_int),
        "ccmp_set_base_frame": ([pp, C.c_int, dp, dp], C.c_int),
        "ccmp_set_calibration": ([pp, C.c_int, dp], C.c_int),
        "ccmp_ctx_create": ([C.c_int, C.POINTER(vp)], C.c_int),
        "ccmp_ctx_destroy": ([vp], None),
        "ccmp_ctx_set_waves_per_cu": ([vp, C.c_int], C.c_int),
        "ccmp_ctx_set_schedule": ([vp, C.c_int, C.c_size_t], C.c_int),
        "ccmp_ctx_set_option": ([vp, C.c_char_p, C.c_long], C.c_int),
        "ccmp_ctx_get_option": ([vp, C.c_char_p, C.POINTER(C.c_long)], C.c_int),
        "ccmp_ctx_option_info": ([C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long),
                                  C.POINTER(C.c_char_p)], C.c_int),
        "ccmp_ctx_describe": ([vp, C.c_int, C.c_size_t, C.c_char_p, C.c_size_t], C.c_int),
        "ccmp_ctx_set_lpt": ([vp, C.c_int, C.c_size_t], C.c_int),
        "ccmp_ctx_device": ([vp], C.c_int),
        "ccmp_ctx_num_cus": ([vp], C.c_int),
        "ccmp_function_batch": ([vp, pp, vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_project_batch": ([vp, pp, vp, vp, vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_is_satisfied_batch": ([vp, pp, vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_joint_valid_batch": ([vp, pp, vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_sample_project_batch": ([vp, pp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_sample_near_project_batch": ([vp, pp, C.c_uint64, C.c_uint64, vp, C.c_int, C.c_double, vp, vp, vp, vp,
                                            C.c_size_t, vp], C.c_int),
        "ccmp_sample_gaussian_project_batch": ([vp, pp, C.c_uint64, C.c_uint64, vp, C.c_int, C.c_double, vp, vp, vp, vp,
                                                C.c_size_t, vp], C.c_int),
        "ccmp_compute_t_wo_batch": ([vp, pp, vp, C.c_int, vp, C.c_size_t, vp], C.c_int),
        "ccmp_geodesic_batch": ([vp, pp, vp, vp, C.c_size_t, C.c_int, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_check_motion_batch": ([vp, pp, vp, vp, C.c_size_t, C.c_int, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_geodesic_batch_ex": ([vp, pp, vp, vp, C.c_size_t, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp], C.c_int),
        "ccmp_geodesic_host_ex": ([vp, pp, dp, dp, C.c_size_t, C.c_int, dp, C.POINTER(C.c_int32), u8p, dp, dp, C.c_int, C.c_int], C.c_int),
        "ccmp_check_motion_host": ([vp, pp, dp, dp, C.c_size_t, C.c_int, dp, C.POINTER(C.c_int32), u8p], C.c_int),
        "ccmp_ambient_uniform_batch": ([vp, pp, C.c_uint64, C.c_uint64, vp, C.c_size_t, vp], C.c_int),
        "ccmp_enforce_bounds_batch": ([vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_compact_valid": ([vp, vp, vp, C.c_size_t, vp, vp, vp], C.c_int),
        "ccmp_compact_valid_capped": ([vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp], C.c_int),
        "ccmp_project_host": ([vp, pp, dp, dp, u8p, u16p, C.c_size_t], C.c_int),
        "ccmp_function_host": ([vp, pp, dp, dp, C.c_size_t], C.c_int),
        "ccmp_is_satisfied_host": ([vp, pp, dp, u8p, C.c_size_t], C.c_int),
        "ccmp_joint_valid_host": ([vp, pp, dp, u8p, C.c_size_t], C.c_int),
        "ccmp_sample_project_host": ([vp, pp, C.c_uint64, C.c_uint64, dp, u8p, u16p, C.c_size_t], C.c_int),
        "ccmp_sample_ref_project_host": ([vp, pp, C.c_int, C.c_uint64, C.c_uint64, dp, C.c_double, dp, u8p, u16p, C.c_size_t], C.c_int),
        "ccmp_geodesic_host": ([vp, pp, dp, dp, C.c_size_t, C.c_int, dp, C.POINTER(C.c_int32), u8p], C.c_int),
        "ccmp_project_sharded_host": ([C.POINTER(vp), C.c_int, pp, dp, dp, u8p, u16p, C.c_size_t], C.c_int),
        "ccmp_sample_project_sharded_host": ([C.POINTER(vp), C.c_int, pp, C.c_uint64, C.c_uint64, dp, u8p, u16p, C.c_size_t], C.c_int),
        "ccmp_sharded_host_last_timing": ([C.POINTER(vp), C.c_int, dp, dp], C.c_int),
        "ccmp_comm_create": ([C.POINTER(vp), C.c_int, C.POINTER(vp)], C.c_int),
        "ccmp_comm_destroy": ([vp], None),
        "ccmp_comm_last_timing": ([vp, dp, dp], C.c_int),
        "ccmp_project_sharded": ([vp, pp, dp, C.c_size_t, dp, u8p, u16p, C.c_size_t, dp, C.c_size_t, C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64)], C.c_int),
        "ccmp_sample_project_sharded": ([vp, pp, C.c_uint64, C.c_uint64, C.c_size_t, dp, u8p, u16p, C.c_size_t, dp, C.c_size_t,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
        "ccmp_scene_create": ([vp, C.POINTER(CcmpSphere), C.c_int, C.POINTER(CcmpBox), C.c_int, C.POINTER(C.c_uint32), C.POINTER(vp)], C.c_int),
        "ccmp_scene_destroy": ([vp], None),
        "ccmp_scene_num_pairs": ([vp], C.c_int),
        "ccmp_clearance_batch": ([vp, pp, vp, vp, vp, C.c_size_t, C.c_double, vp, vp, vp, vp], C.c_int),
        "ccmp_clearance_host": ([vp, pp, vp, dp, C.c_size_t, C.c_double, dp, C.POINTER(C.c_int32), u8p], C.c_int),
        "ccmp_geodesic_scene_batch": ([vp, pp, vp, C.c_double, vp, vp, C.c_size_t, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp],
                                      C.c_int),
        "ccmp_geodesic_scene_host": ([vp, pp, vp, C.c_double, dp, dp, C.c_size_t, C.c_int, dp, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_int32), u8p,
                                      dp, dp, dp, C.c_int, C.c_int], C.c_int),
        "ccmp_knn_batch": ([vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, vp, vp, vp], C.c_int),
        "ccmp_knn_host": ([vp, dp, C.c_size_t, dp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int32), dp], C.c_int),
        "ccmp_connect_batch": ([vp, pp, vp, C.c_double, vp, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_connect_host": ([vp, pp, vp, C.c_double, dp, C.c_size_t, dp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int,
                               C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_int32), u8p, dp], C.c_int),
        "ccmp_pose_distance": ([dp, dp], C.c_double),
        "ccmp_pose_from_t_wo": ([dp, dp], None),
        "ccmp_roadmap_create": ([vp, C.c_size_t], vp),
        "ccmp_roadmap_destroy": ([vp], None),
        "ccmp_roadmap_size": ([vp], C.c_size_t),
        "ccmp_roadmap_reserve": ([vp, C.c_size_t], C.c_int),
        "ccmp_roadmap_append": ([vp, pp, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp], C.c_int),
        "ccmp_roadmap_set_joints": ([vp, C.c_size_t, vp, vp], C.c_int),
        "ccmp_roadmap_truncate": ([vp, C.c_size_t], C.c_int),
        "ccmp_roadmap_read": ([vp, C.c_size_t, C.c_size_t, vp, vp, vp], C.c_int),
        "ccmp_roadmap_knn": ([vp, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, vp, vp, vp], C.c_int),
        "ccmp_roadmap_connect": ([vp, pp, vp, C.c_double, C.c_int, vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                  vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_roadmap_append_host": ([vp, pp, dp, dp, C.c_size_t, C.POINTER(C.c_size_t)], C.c_int),
        "ccmp_roadmap_set_joints_host": ([vp, C.c_size_t, dp], C.c_int),
        "ccmp_roadmap_read_host": ([vp, C.c_size_t, C.c_size_t, dp, dp], C.c_int),
        "ccmp_roadmap_knn_host": ([vp, C.c_int, dp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int32), dp], C.c_int),
        "ccmp_roadmap_connect_host": ([vp, pp, vp, C.c_double, C.c_int, dp, dp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_int32), dp, dp, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_int32), u8p, dp], C.c_int),
        "ccmp_ik_opts_default": ([C.POINTER(CcmpIkOpts)], None),
        "ccmp_pose_ik_batch": ([vp, pp, C.POINTER(CcmpIkOpts), vp, vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_pose_ik_host": ([vp, pp, C.POINTER(CcmpIkOpts), dp, dp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, dp, u8p, C.POINTER(C.c_int32), dp,
                               C.POINTER(C.c_int32)], C.c_int),
        "ccmp_pose_ik_ref": ([pp, C.POINTER(CcmpIkOpts), dp, dp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, dp, u8p, C.POINTER(C.c_int32), dp,
                              C.POINTER(C.c_int32)], C.c_int),
        "ccmp_roadmap_grow": ([vp, pp, vp, C.c_double, C.POINTER(CcmpIkOpts), vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int,
                               C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_roadmap_grow_host": ([vp, pp, vp, C.c_double, C.POINTER(CcmpIkOpts), dp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64,
                                    C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), dp, dp, u8p, C.POINTER(C.c_int32), dp, C.POINTER(C.c_int32), u8p,
                                    C.POINTER(C.c_int32), u8p, dp], C.c_int),
        "ccmp_arm_clearance_batch": ([vp, pp, vp, C.c_int, vp, C.c_size_t, C.c_double, vp, vp, vp], C.c_int),
        "ccmp_arm_clearance_host": ([vp, pp, vp, C.c_int, dp, C.c_size_t, C.c_double, dp, u8p], C.c_int),
        "ccmp_arm_clearance_ref": ([pp, C.POINTER(CcmpSphere), C.c_int, C.POINTER(CcmpBox), C.c_int, C.POINTER(C.c_uint32), C.c_int, dp, C.c_size_t, C.c_double,
                                    dp, u8p], C.c_int),
        "ccmp_pose_ik_vetted_batch": ([vp, pp, C.POINTER(CcmpIkOpts), vp, vp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp, C.c_double, vp, vp, vp, vp, vp, vp,
                                       vp, vp, vp], C.c_int),
        "ccmp_pose_ik_vetted_host": ([vp, pp, C.POINTER(CcmpIkOpts), dp, dp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, vp, C.c_double, dp, u8p, i32p, dp, i32p,
                                      dp, dp, dp], C.c_int),
        "ccmp_pose_ik_vetted_ref": ([pp, C.POINTER(CcmpIkOpts), dp, dp, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(CcmpSphere), C.c_int,
                                     C.POINTER(CcmpBox), C.c_int, C.POINTER(C.c_uint32), C.c_double, dp, u8p, i32p, dp, i32p, dp, dp, dp], C.c_int),
        "ccmp_roadmap_grow_vetted": ([vp, pp, vp, C.c_double, C.POINTER(CcmpIkOpts), vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64,
                                      C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_roadmap_grow_vetted_host": ([vp, pp, vp, C.c_double, C.POINTER(CcmpIkOpts), dp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_uint64, C.c_uint64,
                                           C.c_int, C.c_int, C.c_int, i32p, dp, dp, u8p, i32p, dp, dp, i32p, u8p, i32p, u8p, dp], C.c_int),
        "ccmp_pose_interpolate": ([dp, dp, C.c_double, dp], None),
        "ccmp_object_create": ([vp, dp, C.c_int, C.POINTER(CcmpBox), C.c_int, C.POINTER(vp)], C.c_int),
        "ccmp_object_destroy": ([vp], None),
        "ccmp_object_num_triangles": ([vp], C.c_int),
        "ccmp_object_valid_batch": ([vp, vp, vp, C.c_size_t, C.c_double, vp, vp, vp], C.c_int),
        "ccmp_object_valid_host": ([vp, vp, dp, C.c_size_t, C.c_double, u8p, C.POINTER(C.c_uint32)], C.c_int),
        "ccmp_object_valid_ref": ([dp, C.c_int, C.POINTER(CcmpBox), C.c_int, dp, C.c_size_t, C.c_double, C.c_int, u8p, C.POINTER(C.c_uint32)], C.c_int),
        "ccmp_object_propose_batch": ([vp, vp, vp, vp, C.c_int, C.c_size_t, C.c_double, C.c_double, dp, dp, C.c_int, C.c_uint64, C.c_uint64, C.c_double,
                                       vp, vp, vp, vp, vp], C.c_int),
        "ccmp_object_propose_host": ([vp, vp, dp, dp, C.c_int, C.c_size_t, C.c_double, C.c_double, dp, dp, C.c_int, C.c_uint64, C.c_uint64, C.c_double,
                                      dp, C.POINTER(C.c_int32), dp, u8p], C.c_int),
        "ccmp_object_propose_ref": ([dp, C.c_int, C.POINTER(CcmpBox), C.c_int, dp, dp, C.c_int, C.c_size_t, C.c_double, C.c_double, dp, dp, C.c_int, C.c_uint64,
                                     C.c_uint64, C.c_double, dp, C.POINTER(C.c_int32), dp, u8p], C.c_int),
        "ccmp_joint_distance": ([dp, dp], C.c_double),
        "ccmp_graph_labels_ref": ([i32p, C.c_size_t, C.c_size_t, i32p], C.c_int),
        "ccmp_roadmap_commit": ([vp, pp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_size_t, C.c_int, dp, i32p, C.c_int, C.c_uint, vp, vp, vp,
                                 C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), vp], C.c_int),
        "ccmp_roadmap_commit_host": ([vp, pp, i32p, u8p, i32p, dp, C.c_int, dp, dp, u8p, C.c_size_t, C.c_int, dp, i32p, C.c_int, C.c_uint, i32p, i32p, i32p,
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "ccmp_roadmap_commit_ref": ([pp, dp, dp, i32p, C.c_size_t, i32p, u8p, i32p, dp, C.c_int, dp, dp, u8p, C.c_size_t, C.c_int, dp, i32p, C.c_int, C.c_uint,
                                     i32p, i32p, i32p, dp, dp, i32p, dp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "ccmp_roadmap_add_edges": ([vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp], C.c_int),
        "ccmp_roadmap_add_edges_host": ([vp, i32p, C.c_size_t], C.c_int),
        "ccmp_roadmap_num_edges": ([vp], C.c_size_t),
        "ccmp_roadmap_read_edges": ([vp, C.c_size_t, C.c_size_t, vp, vp, vp], C.c_int),
        "ccmp_roadmap_read_edges_host": ([vp, C.c_size_t, C.c_size_t, i32p, dp], C.c_int),
        "ccmp_roadmap_read_labels": ([vp, C.c_size_t, C.c_size_t, vp, vp], C.c_int),
        "ccmp_roadmap_read_labels_host": ([vp, C.c_size_t, C.c_size_t, i32p], C.c_int),
        "ccmp_roadmap_closest": ([vp, vp, C.c_size_t, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_roadmap_closest_host": ([vp, i32p, C.c_size_t, dp, i32p, dp, dp], C.c_int),
        "ccmp_roadmap_closest_ref": ([dp, i32p, C.c_size_t, i32p, C.c_size_t, dp, i32p, dp, dp], C.c_int),
        "ccmp_roadmap_shortest_paths": ([vp, vp, vp, C.c_size_t, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_roadmap_shortest_paths_host": ([vp, i32p, i32p, C.c_size_t, C.c_int, dp, i32p, i32p, dp, dp, dp, i32p], C.c_int),
        "ccmp_graph_shortest_paths_ref": ([i32p, dp, C.c_size_t, C.c_size_t, i32p, i32p, C.c_size_t, C.c_int, dp, i32p, i32p, dp, i32p], C.c_int),
        "ccmp_roadmap_path_rounds_host": ([vp, C.c_size_t, i32p], C.c_int),
        "ccmp_dense_opts_default": ([C.POINTER(CcmpDenseOpts)], None),
        "ccmp_path_densify": ([vp, pp, vp, C.c_double, vp, vp, C.c_size_t, C.c_int, C.POINTER(CcmpDenseOpts), C.POINTER(vp), vp], C.c_int),
        "ccmp_path_densify_host": ([vp, pp, vp, C.c_double, dp, i32p, C.c_size_t, C.c_int, C.POINTER(CcmpDenseOpts), C.POINTER(vp)], C.c_int),
        "ccmp_dense_paths_info": ([vp, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)], C.c_int),
        "ccmp_dense_paths_copy": ([vp] + [vp] * 11 + [vp], C.c_int),
        "ccmp_dense_paths_copy_host": ([vp, dp, i32p, i32p, u8p, i32p, dp, dp, dp, dp, i32p, i32p], C.c_int),
        "ccmp_dense_paths_destroy": ([vp], None),
        "ccmp_dense_layout_ref": ([i32p, C.c_size_t, C.c_int, i32p, C.c_int, i32p, i32p, C.POINTER(C.c_size_t)], C.c_int),
        "ccmp_dense_arc_ref": ([dp, i32p, C.c_size_t, dp, dp], C.c_int),
        "ccmp_shortcut_opts_default": ([C.POINTER(CcmpShortcutOpts)], None),
        "ccmp_path_shortcut": ([vp, pp, vp, C.c_double, vp, vp, C.c_size_t, C.c_int, C.POINTER(CcmpShortcutOpts), vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_path_shortcut_host": ([vp, pp, vp, C.c_double, dp, i32p, C.c_size_t, C.c_int, C.POINTER(CcmpShortcutOpts), dp, i32p, i32p, dp, dp, u8p, i32p, i32p],
                                    C.c_int),
        "ccmp_shortcut_select": ([vp, vp, vp, C.c_size_t, C.c_int, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_shortcut_select_host": ([vp, dp, i32p, C.c_size_t, C.c_int, u8p, dp, i32p, i32p, dp, dp], C.c_int),
        "ccmp_shortcut_select_ref": ([dp, i32p, C.c_size_t, C.c_int, u8p, dp, i32p, i32p, dp, dp], C.c_int),
        "ccmp_shortcut_pairs_ref": ([dp, i32p, C.c_size_t, C.c_int, C.c_int, i32p, C.c_size_t, C.POINTER(C.c_size_t)], C.c_int),
        "ccmp_smooth_opts_default": ([C.POINTER(CcmpSmoothOpts)], None),
        "ccmp_path_smooth": ([vp, pp, vp, C.c_double, vp, vp, C.c_size_t, C.c_int, C.POINTER(CcmpSmoothOpts), C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_path_smooth_host": ([vp, pp, vp, C.c_double, dp, i32p, C.c_size_t, C.c_int, C.POINTER(CcmpSmoothOpts), C.c_int, dp, i32p, i32p, i32p, i32p, dp, dp,
                                   i32p], C.c_int),
        "ccmp_smooth_mid_ref": ([dp, dp, C.c_int, C.POINTER(C.c_int), dp, dp, C.POINTER(C.c_int)], C.c_int),
        "ccmp_smooth_len_after": ([C.c_int, C.c_int], C.c_int),
        "ccmp_smooth_last_counts": ([C.POINTER(C.c_longlong)] * 3, None),
        "ccmp_resample_opts_default": ([pp, C.POINTER(CcmpResampleOpts)], None),
        "ccmp_path_resample": ([vp, pp, vp, C.POINTER(CcmpResampleOpts), C.POINTER(vp), vp], C.c_int),
        "ccmp_sampled_paths_info": ([vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "ccmp_sampled_paths_copy": ([vp] + [vp] * 7 + [vp], C.c_int),
        "ccmp_sampled_paths_copy_host": ([vp, dp, i32p, dp, dp, u8p, i32p, i32p], C.c_int),
        "ccmp_sampled_paths_destroy": ([vp], None),
        "ccmp_path_timestamps": ([vp, vp, vp, C.c_size_t, C.c_size_t, dp, dp, C.c_double, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_path_timestamps_host": ([vp, dp, i32p, C.c_size_t, C.c_size_t, dp, dp, C.c_double, dp, dp, dp, dp, i32p], C.c_int),
        "ccmp_path_timestamps_ref": ([dp, i32p, C.c_size_t, C.c_size_t, dp, dp, C.c_double, dp, dp, dp, dp, i32p], C.c_int),
        "ccmp_arc_bracket_ref": ([dp, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)], C.c_int),
        "ccmp_resample_targets_ref": ([C.c_double, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int), dp], C.c_int),
        "ccmp_setpoint_opts_default": ([C.POINTER(CcmpSetpointOpts)], None),
        "ccmp_path_setpoints": ([vp, pp, vp, C.c_double, vp, vp, vp, C.c_size_t, C.c_size_t, dp, dp, C.POINTER(CcmpSetpointOpts), C.POINTER(vp), vp], C.c_int),
        "ccmp_path_setpoints_host": ([vp, pp, vp, C.c_double, dp, i32p, dp, C.c_size_t, C.c_size_t, dp, dp, C.POINTER(CcmpSetpointOpts), C.POINTER(vp)], C.c_int),
        "ccmp_setpoints_info": ([vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "ccmp_setpoints_copy": ([vp] + [vp] * 12 + [vp], C.c_int),
        "ccmp_setpoints_copy_host": ([vp, dp, dp, dp, i32p, dp, u8p, dp, i32p, dp, i32p, i32p, dp], C.c_int),
        "ccmp_setpoints_destroy": ([vp], None),
        "ccmp_setpoints_ref": ([dp, i32p, dp, C.c_size_t, C.c_size_t, dp, dp, C.POINTER(CcmpSetpointOpts), i32p, i32p, dp, dp, dp, dp, i32p, dp], C.c_int),
        "ccmp_setpoint_tangents_ref": ([dp, dp, C.c_size_t, dp], C.c_int),
        "ccmp_fit_opts_default": ([C.POINTER(CcmpFitOpts)], None),
        "ccmp_path_fit_timestamps": ([vp, vp, vp, vp, C.c_size_t, C.c_size_t, dp, dp, C.POINTER(CcmpFitOpts), vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_path_fit_timestamps_host": ([vp, dp, i32p, dp, C.c_size_t, C.c_size_t, dp, dp, C.POINTER(CcmpFitOpts), dp, i32p, i32p, dp, dp, dp], C.c_int),
        "ccmp_path_fit_timestamps_ref": ([dp, i32p, dp, C.c_size_t, C.c_size_t, dp, dp, C.POINTER(CcmpFitOpts), dp, i32p, i32p, dp, dp, dp], C.c_int),
        "ccmp_jerk_opts_default": ([C.POINTER(CcmpJerkOpts)], None),
        "ccmp_path_jerk_setpoints": ([vp, pp, vp, C.c_double, vp, vp, vp, C.c_size_t, C.c_size_t, dp, dp, dp, C.POINTER(CcmpJerkOpts), C.POINTER(vp), vp], C.c_int),
        "ccmp_path_jerk_setpoints_host": ([vp, pp, vp, C.c_double, dp, i32p, dp, C.c_size_t, C.c_size_t, dp, dp, dp, C.POINTER(CcmpJerkOpts), C.POINTER(vp)], C.c_int),
        "ccmp_jerk_setpoints_info": ([vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "ccmp_jerk_setpoints_copy": ([vp] + [vp] * 13 + [vp], C.c_int),
        "ccmp_jerk_setpoints_copy_host": ([vp, dp, dp, dp, i32p, dp, u8p, dp, i32p, i32p, i32p, dp, i32p, i32p], C.c_int),
        "ccmp_jerk_setpoints_destroy": ([vp], None),
        "ccmp_jerk_next_window_ref": ([C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "ccmp_jerk_setpoints_ref": ([dp, i32p, dp, C.c_size_t, C.c_size_t, dp, dp, dp, C.POINTER(CcmpJerkOpts), i32p, i32p, i32p, i32p, dp, dp, dp, dp, i32p], C.c_int),
        "ccmp_plan_default_opts": ([C.POINTER(CcmpPlanOpts)], None),
        "ccmp_plan_create": ([vp, pp, vp, vp, C.c_double, C.POINTER(CcmpIkOpts), C.POINTER(CcmpPlanOpts), dp, C.c_uint64, C.c_uint64, C.POINTER(vp)], C.c_int),
        "ccmp_plan_run": ([vp, C.c_int, C.POINTER(CcmpPlanReport)], C.c_int),
        "ccmp_plan_state_read": ([vp, C.POINTER(CcmpPlanState)], C.c_int),
        "ccmp_plan_destroy": ([vp], None),
        "ccmp_plan_check_ref": ([C.POINTER(CcmpPlanState), C.c_size_t, i32p, dp, dp, i32p, dp, dp, dp, i32p], C.c_int),
        "ccmp_plan_prefix_ref": ([u8p, u8p, u8p, i32p], C.c_int),
        "ccmp_plan_connected_ref": ([i32p, C.c_size_t, C.POINTER(CcmpPlanState)], C.c_int),
        "ccmp_rrtc_default_opts": ([C.POINTER(CcmpRrtcOpts)], None),
        "ccmp_rrtc_create": ([vp, pp, vp, C.c_double, C.POINTER(CcmpRrtcOpts), i32p, C.c_int, i32p, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(vp)], C.c_int),
        "ccmp_rrtc_run": ([vp, C.c_int, C.POINTER(CcmpRrtcReport)], C.c_int),
        "ccmp_rrtc_state_read": ([vp, C.POINTER(CcmpRrtcState)], C.c_int),
        "ccmp_rrtc_destroy": ([vp], None),
        "ccmp_roadmap_nearest_in_tree": ([vp, vp, C.c_int, vp, C.c_size_t, vp, vp, vp], C.c_int),
        "ccmp_roadmap_nearest_in_tree_host": ([vp, i32p, C.c_int, dp, C.c_size_t, i32p, dp], C.c_int),
        "ccmp_roadmap_nearest_in_tree_ref": ([dp, i32p, C.c_size_t, i32p, C.c_int, dp, C.c_size_t, i32p, dp], C.c_int),
        "ccmp_rrtc_nearest_shape": ([vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_uint)], C.c_int),
        "ccmp_rrtc_pick_ref": ([C.c_int, dp, i32p, u8p, u8p, dp, dp, C.c_size_t, C.c_int, C.c_double, i32p, i32p, dp, dp], C.c_int),
        "ccmp_rrtc_connected_ref": ([i32p, C.c_size_t, C.POINTER(CcmpRrtcState)], C.c_int),
        "ccmp_rrtc_pick_batch": ([vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int, C.c_double, vp, vp, vp, vp, vp], C.c_int),
        "ccmp_strerror": ([C.c_int], C.c_char_p),
        "ccmp_last_hip_error": ([], C.c_char_p),
        "ccmp_version": ([], C.c_int),
        "ccmp_problem_sizeof": ([], C.c_size_t),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)  # AttributeError here = library out of date with the header
        fn.argtypes = args
        fn.restype = res
    debug_sig = {
        "ccmp_ctx_set_order_experimental": ([vp, vp], C.c_int),
        "ccmp_ctx_debug_lpt_pred": ([vp, vp, C.c_size_t], C.c_int),
        "ccmp_detmath_probe": ([vp, vp, vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_detmath_div_probe": ([vp, vp, vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_detmath_round_facts_probe": ([vp, vp, vp, vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_debug_fail_calls": ([vp, C.c_int], C.c_int),
        "ccmp_ctx_debug_lpt_order": ([vp, vp, C.c_size_t, vp, vp, C.c_size_t], C.c_int),
        "ccmp_ctx_debug_fd_state": ([vp, vp, C.c_size_t, vp], C.c_int),
        "ccmp_debug_sort_probe": ([vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, vp], C.c_int),
        "ccmp_debug_split_probe": ([vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_uint, vp, vp], C.c_int),
    }
    for name, (args, res) in debug_sig.items():  # present in the debug build only (include/ccmp_debug.h)
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
    if L.ccmp_problem_sizeof() != C.sizeof(CcmpProblem):
        raise ImportError("ccmp_problem layout mismatch between libccmp.so and the Python binding")
    _lib = L
    return L


CALL_PROJECT, CALL_SAMPLE_PROJECT, CALL_PROJECT_ANALYTIC, CALL_GEODESIC, CALL_GEODESIC_BUDGET, CALL_GEODESIC_ANALYTIC = range(6)  # ccmp.h: CCMP_CALL_*
CALL_GEODESIC_SCENE, CALL_KNN, CALL_CONNECT = 6, 7, 8
CALL_ROADMAP_KNN, CALL_ROADMAP_CONNECT = 10, 11  # (9 is not assigned)
CALL_POSE_IK = 13  # (12 is not assigned)
CALL_OBJECT_PROPOSE = 15  # (14 is not assigned)
OBJECT_MAX_TRIANGLES, OBJECT_MAX_ATTEMPTS, MAX_BOXES = 16384, 16, 8  # ccmp.h: CCMP_OBJECT_MAX_*, CCMP_MAX_BOXES
IK_MAX_SEEDS, IK_MAX_RESTARTS, IK_MAX_ROUNDS = 16, 31, 256  # ccmp.h: CCMP_IK_MAX_*
METRIC_JOINT, METRIC_OBJECT = 0, 1  # ccmp.h: CCMP_METRIC_*
KNN_ALL, KNN_NOT_SELF, KNN_EARLIER = 0, 1, 2  # ccmp.h: CCMP_KNN_*
KNN_MAX_K = 16
GROW_TRAPPED, GROW_SREACHED, GROW_GREACHED, GROW_UNSETTLED = range(4)  # ccmp.h: CCMP_GROW_*
COMMIT_KEEP_ISOLATED = 1  # ccmp.h: CCMP_COMMIT_*
GRAPH_MAX_ROOTS, CLOSEST_MAX_FROM = 32, 64  # ccmp.h: CCMP_GRAPH_MAX_ROOTS, CCMP_CLOSEST_MAX_FROM
PATH_MAX_PAIRS = 64  # ccmp.h: CCMP_PATH_MAX_PAIRS
PLAN_OPEN, PLAN_SOLVED, PLAN_BUDGET, PLAN_FULL, PLAN_INVALID_GOAL = range(5)  # ccmp.h: CCMP_PLAN_*
PLAN_MAX_STARTS, PLAN_MAX_GOALS, PLAN_MAX_WIDTH, PLAN_LADDER = 8, 8, 256, 9  # ccmp.h: CCMP_PLAN_MAX_*, CCMP_PLAN_LADDER
RRTC_OPEN, RRTC_SOLVED, RRTC_BUDGET, RRTC_FULL = range(4)  # ccmp.h: CCMP_RRTC_* (statuses)
RRTC_NONE, RRTC_TRAPPED, RRTC_ADVANCED, RRTC_REACHED, RRTC_UNSETTLED = -1, 0, 1, 2, 3  # ccmp.h: CCMP_RRTC_* (step 2's outcomes)
RRTC_CONNECT_NOTHING, RRTC_CONNECT_ADDED, RRTC_CONNECT_JOINED = range(3)  # ccmp.h: CCMP_RRTC_CONNECT_*
RRTC_MAX_ROOTS = 8  # ccmp.h: CCMP_RRTC_MAX_ROOTS
DENSE_DISTINCT = 1  # ccmp.h: CCMP_DENSE_DISTINCT
SHORTCUT_MAX_LEN = 1024  # ccmp.h: CCMP_SHORTCUT_MAX_LEN
RETIME_OK, RETIME_EMPTY, RETIME_BROKEN, RETIME_NONFINITE, RETIME_POINT, RETIME_FULL = range(6)  # ccmp.h: CCMP_RETIME_*
SAMPLE_PROJECTED, SAMPLE_FALLBACK, SAMPLE_DEGENERATE, SAMPLE_COPIED = range(4)  # ccmp.h: CCMP_SAMPLE_*
SETPOINTS_OK, SETPOINTS_EMPTY, SETPOINTS_NONFINITE, SETPOINTS_UNORDERED, SETPOINTS_POINT, SETPOINTS_FULL = range(6)  # ccmp.h: CCMP_SETPOINTS_*
JERK_OK, JERK_FULL, JERK_WINDOW = 0, 5, 6  # ccmp.h: CCMP_JERK_* (1 .. 4: the setpoints values)
FIT_FITTED, FIT_PASSES = 0, 6  # ccmp.h: CCMP_FIT_* (1 .. 5: the setpoints values)


def option_table():
    """every tuning option of a context as the library itself states it (ccmp_ctx_option_info): name, built-in default, range,
    meaning — no device needed"""
    L = lib()
    out, i = [], 0
    while True:
        name, doc = C.c_char_p(), C.c_char_p()
        d, lo, hi = C.c_long(), C.c_long(), C.c_long()
        if L.ccmp_ctx_option_info(i, C.byref(name), C.byref(d), C.byref(lo), C.byref(hi), C.byref(doc)) != 0:
            return out
        out.append({"name": name.value.decode(), "default": d.value, "lo": lo.value, "hi": hi.value, "doc": doc.value.decode()})
        i += 1


def get_option(ctx_handle, name):
    """ccmp_ctx_get_option; ctx_handle None = the built-in default"""
    v = C.c_long()
    check(lib().ccmp_ctx_get_option(ctx_handle, name.encode(), C.byref(v)), "ccmp_ctx_get_option(%s)" % name)
    return v.value


def describe(ctx_handle, call_kind, n):
    """ccmp_ctx_describe: one line naming the kernels and thresholds the policy takes for a call of n samples / edges
    (ctx_handle None = the built-in policy on a 256-CU device)"""
    buf = C.create_string_buffer(2048)
    rc = lib().ccmp_ctx_describe(ctx_handle, int(call_kind), int(n), buf, len(buf))
    if rc < 0:
        check(rc, "ccmp_ctx_describe")
    return buf.value.decode()


def _strerror(code):
    try:
        return lib().ccmp_strerror(code).decode()
    except Exception:  # pragma: no cover
        return "error"


def check(code, what):
    if code != 0:
        detail = ""
        if code == -2:
            detail = lib().ccmp_last_hip_error().decode()
        raise CcmpError(code, what, detail)
