"""ctypes binding of libikflow_amd.so (the C-ABI declared in include/ikflow_amd.h).

There is no fallback: if the in-tree shared library is missing or does not load, importing the binding raises.
"""
from __future__ import annotations

import ctypes as C
import os

from ikflow_amd import build as _build

IKF_ABI_VERSION = 3
IKF_MAX_DOF = 8
IKF_MAX_DIM = 16
IKF_MAX_ROUNDS = 8
IKF_MAX_CAPSULES = 24
IKF_RANK_MAX_KEEP = 16
IKF_PATH_MAX_K = 256
IKF_DIVERSE_MAX_K = 1024
IKF_DIVERSE_MAX_KEEP = 16
IKF_WORLD_MAX_OBSTACLES = 64
IKF_CLOUD_MAX_POINTS = 1 << 20
IKF_SWEEP_MAX_SAMPLES = 16
IKF_REFINE_MAX_STEPS = 16
IKF_WORLD_TRACK_MAX_FRAMES = 1024
IKF_OBSTACLE_SPHERE, IKF_OBSTACLE_CAPSULE, IKF_OBSTACLE_HALF_SPACE, IKF_OBSTACLE_BOX = 0, 1, 2, 3

IKF_OK = 0
IKF_ERR_NULL_POINTER = 1
IKF_ERR_BAD_SHAPE = 2
IKF_ERR_NOT_LOADED = 3
IKF_ERR_MISSING_TENSOR = 4
IKF_ERR_HIP = 5
IKF_ERR_NO_DEVICE = 6
IKF_ERR_BAD_ARGUMENT = 7


class ikf_joint(C.Structure):
    _fields_ = [("kind", C.c_int32), ("axis", C.c_float * 3), ("pre", C.c_float * 12)]


class ikf_model_desc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("nb_nodes", C.c_int32),
        ("dim", C.c_int32),
        ("dim_cond", C.c_int32),
        ("width", C.c_int32),
        ("n_hidden", C.c_int32),
        ("clamp", C.c_float),
        ("leaky_slope", C.c_float),
        ("ndof", C.c_int32),
        ("joint_lo", C.c_float * IKF_MAX_DOF),
        ("joint_hi", C.c_float * IKF_MAX_DOF),
        ("chain", ikf_joint * IKF_MAX_DOF),
        ("tool", C.c_float * 12),
        ("sigmoid_on_output", C.c_int32),
    ]


class ikf_capsule(C.Structure):
    _fields_ = [("frame", C.c_int32), ("p0", C.c_float * 3), ("p1", C.c_float * 3), ("radius", C.c_float)]


class ikf_rank_options(C.Structure):
    _fields_ = [
        ("n_keep", C.c_int32),
        ("rot_weight", C.c_float),
        ("ref_weight", C.c_float),
        ("max_pos_err", C.c_float),
        ("max_rot_err", C.c_float),
        ("reject_limits", C.c_int32),
        ("reject_collisions", C.c_int32),
        ("min_clearance", C.c_float),
    ]


class ikf_path_options(C.Structure):
    _fields_ = [
        ("rot_weight", C.c_float),
        ("max_pos_err", C.c_float),
        ("max_rot_err", C.c_float),
        ("reject_limits", C.c_int32),
        ("reject_collisions", C.c_int32),
        ("min_clearance", C.c_float),
        ("node_weight", C.c_float),
        ("max_joint_step", C.c_float),
    ]


class ikf_diverse_options(C.Structure):
    _fields_ = [
        ("n_keep", C.c_int32),
        ("rot_weight", C.c_float),
        ("max_pos_err", C.c_float),
        ("max_rot_err", C.c_float),
        ("reject_limits", C.c_int32),
        ("reject_collisions", C.c_int32),
        ("min_clearance", C.c_float),
        ("min_separation", C.c_float),
    ]


class ikf_obstacle(C.Structure):
    _fields_ = [("kind", C.c_int32), ("a", C.c_float * 3), ("b", C.c_float * 3), ("quat", C.c_float * 4), ("radius", C.c_float)]


class ikf_tensor(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("h_data", C.c_void_p),
        ("dtype", C.c_int32),
        ("ndim", C.c_int32),
        ("shape", C.c_int64 * 4),
    ]


LATENT_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int)
SEED_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int)

# name -> (restype, argtypes); every symbol include/ikflow_amd.h and include/ikflow_amd_debug.h declare
SIGNATURES = {
    "ikf_create": (C.c_int, [C.POINTER(ikf_model_desc), C.c_int, C.POINTER(C.c_void_p)]),
    "ikf_destroy": (None, [C.c_void_p]),
    "ikf_last_error": (C.c_char_p, []),
    "ikf_abi_version": (C.c_int, []),
    "ikf_load_weights": (C.c_int, [C.c_void_p, C.POINTER(ikf_tensor), C.c_int]),
    "ikf_weights_loaded": (C.c_int, [C.c_void_p]),
    "ikf_reserve": (C.c_int, [C.c_void_p, C.c_int64]),
    "ikf_reserve_exact": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "ikf_set_exact_upfront_rows": (C.c_int, [C.c_void_p, C.c_int64]),
    "ikf_generate_approx": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p],
    ),
    "ikf_flow_forward": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "ikf_flow_inverse": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "ikf_forward_kinematics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ikf_pose_error": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ikf_lm_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ikf_jacobian": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ikf_clamp_to_joint_limits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ikf_joint_limits_exceeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ikf_set_collision_model": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "ikf_self_collision": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ikf_pose_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ikf_limits_exceeded": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ikf_generate_exact": (
        C.c_int,
        [
            C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_float, C.c_float,
            LATENT_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
        ],
    ),
    "ikf_generate_exact_seeded": (
        C.c_int,
        [
            C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_float, C.c_float,
            SEED_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
        ],
    ),
    "ikf_refine_exact": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "ikf_time_gemm": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_void_p]),
    "ikf_profile_begin": (C.c_int, [C.c_void_p]),
    "ikf_profile_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_void_p]),
    "ikf_profile_event_overhead_ms": (C.c_double, [C.c_void_p]),
    "ikf_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "ikf_get_precision": (C.c_int, [C.c_void_p]),
    "ikf_set_lm_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "ikf_get_lm_precision": (C.c_int, [C.c_void_p]),
    "ikf_set_split_guard": (C.c_int, [C.c_void_p, C.c_int]),
    "ikf_split_fallback_count": (C.c_int64, [C.c_void_p]),
    "ikf_split_overflow_pending": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ikf_split_kernel_name": (C.c_char_p, []),
    "ikf_dominant_kernel_name": (C.c_char_p, []),
    "ikf_dominant_kernel_for": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "ikf_cluster_repairs": (C.c_int64, [C.c_void_p]),
    "ikf_cluster_backoff": (C.c_int64, [C.c_void_p]),
    "ikf_load_time_ms": (C.c_double, [C.c_void_p]),
    "ikf_frag_image_time_ms": (C.c_double, [C.c_void_p]),
    "ikf_probes_build": (C.c_int, []),
    "ikf_plan_describe": (C.c_int, [C.c_void_p, C.c_int64, C.c_char_p, C.c_int]),
    "ikf_cluster_local": (C.c_int, [C.c_void_p]),
    "ikf_plan_describe_for": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "ikf_set_gemm_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "ikf_rank_chunks": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    # m, d_poses, d_idx, n_mod, d_latent, n, clamp_to_limits, softflow_scale, d_q_out, stream
    "ikf_generate_approx_tiled": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p],
    ),
}

# ... every symbol include/ikflow_amd_rank.h declares (best-of-K ranking: not part of the boundary a binding of the reference needs)
_RANK_OUTPUTS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # q_out, score_out, index_out, count_out, row_score_out
RANK_SIGNATURES = {
    "ikf_rank_candidates": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ikf_rank_options)] + _RANK_OUTPUTS + [C.c_void_p],
    ),
    "ikf_generate_ranked": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(ikf_rank_options)] + _RANK_OUTPUTS + [C.c_void_p],
    ),
    "ikf_reserve_ranked": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
}

# ... every symbol include/ikflow_amd_path.h declares (path IK: the cheapest path through k candidates per waypoint)
_PATH_OUTPUTS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]  # path_out, index_out, cost_out, reachable_out, node_cost_out
PATH_SIGNATURES = {
    "ikf_path_search": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ikf_path_options)] + _PATH_OUTPUTS + [C.c_void_p],
    ),
    "ikf_generate_path": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(ikf_path_options)] + _PATH_OUTPUTS + [C.c_void_p],
    ),
    "ikf_reserve_path": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
}

# ... every symbol include/ikflow_amd_path_batch.h declares (path IK for P paths per call: the candidate layout over P * T waypoints)
PATH_BATCH_SIGNATURES = {
    # m, waypoints, P, T, k, q, q_start, opt, outputs, stream
    "ikf_path_search_batch": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ikf_path_options)] + _PATH_OUTPUTS + [C.c_void_p],
    ),
    # m, waypoints, P, T, k, latent, shared_latent, clamp_to_limits, q_start, opt, outputs, stream
    "ikf_generate_path_batch": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(ikf_path_options)] + _PATH_OUTPUTS + [C.c_void_p],
    ),
    "ikf_reserve_path_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int]),
}

# ... every symbol include/ikflow_amd_path_opt.h declares (path IK, third stage: a least-squares pass over whole paths behind the lattice)
IKF_PATH_OPT_MAX_ITERS = 32
PATH_OPT_REASONS = {0: "committed", 1: "no step lowered F", 2: "node inadmissible", 3: "edge forbidden", 4: "cost not lower"}
PATH_OPT_SIGNATURES = {
    # waypoints, P, T, path_in, q_start, opt, n_iters, smooth_weight, validate, path_out, cost_out, info_out, stream
    "ikf_path_optimize": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(ikf_path_options), C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_void_p],
    ),
    # waypoints, P, T, path, q_start, opt, cost_out, info_out, stream
    "ikf_path_cost": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(ikf_path_options), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ikf_set_path_optimize": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "ikf_get_path_optimize": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    # P, h_info [P x 4]
    "ikf_path_optimize_info": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]),
    "ikf_reserve_path_opt": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64]),
}

# ... every symbol include/ikflow_amd_diverse.h declares (diverse-of-K IK: a far-apart set of each pose's admissible candidates)
# q_out, score_out, index_out, separation_out, kept_out, count_out, row_score_out
_DIVERSE_OUTPUTS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
DIVERSE_SIGNATURES = {
    "ikf_diverse_select": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ikf_diverse_options)] + _DIVERSE_OUTPUTS + [C.c_void_p],
    ),
    "ikf_generate_diverse": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(ikf_diverse_options)] + _DIVERSE_OUTPUTS + [C.c_void_p],
    ),
    "ikf_reserve_diverse": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
}

# ... every symbol include/ikflow_amd_world.h declares (world collision: the caller's obstacles against the robot's capsules)
WORLD_SIGNATURES = {
    "ikf_set_world": (C.c_int, [C.c_void_p, C.POINTER(ikf_obstacle), C.c_int, C.c_float]),
    "ikf_world_size": (C.c_int, [C.c_void_p]),
    # q, n, clearance_out, obstacle_out, capsule_out, colliding_out, stream
    "ikf_world_clearance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# ... every symbol include/ikflow_amd_cloud.h declares (world point cloud: the sensed scene as points against the robot's capsules)
CLOUD_SIGNATURES = {
    # h_points, n_points, point_radius, min_clearance
    "ikf_set_world_cloud": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float]),
    "ikf_world_cloud_size": (C.c_int64, [C.c_void_p]),
    # q, n, clearance_out, colliding_out, stream
    "ikf_cloud_clearance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# ... every symbol include/ikflow_amd_sweep.h declares (swept collision checks along edges: the caller's, and those of a path lattice)
SWEEP_SIGNATURES = {
    "ikf_set_path_sweep": (C.c_int, [C.c_void_p, C.c_int]),
    "ikf_get_path_sweep": (C.c_int, [C.c_void_p]),
    # q_a, q_b, n, n_samples, reject_self, self_min_clearance, blocked_out, first_out, stream
    "ikf_sweep_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# ... every symbol include/ikflow_amd_refine.h declares (refined candidates: LM steps on every candidate row before it is scored)
REFINE_SIGNATURES = {
    "ikf_set_candidate_refine": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "ikf_get_candidate_refine": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    # target_poses, n_poses, k, q, n_steps, pos_tol, rot_tol, q_out, steps_out, converged_out, stream
    "ikf_refine_candidates": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
}

# ... every symbol include/ikflow_amd_exact_world.h declares (exact IK that obeys the world: collision-free solutions from the retry loop)
EXACT_WORLD_SIGNATURES = {
    # on, reject_self, self_min_clearance
    "ikf_set_exact_collision": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float]),
    "ikf_get_exact_collision": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    # h_rows[IKF_MAX_ROUNDS]
    "ikf_exact_collision_rejected": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
}

# ... every symbol include/ikflow_amd_track.h declares (a world that moves along a path: one frame of obstacles per waypoint of path IK)
TRACK_SIGNATURES = {
    # h_frames [F][n], n_frames, n_obstacles, min_clearance
    "ikf_set_world_track": (C.c_int, [C.c_void_p, C.POINTER(ikf_obstacle), C.c_int, C.c_int, C.c_float]),
    "ikf_world_track_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    # t, i, h_out [n]
    "ikf_world_track_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(ikf_obstacle)]),
    # q, T, k, clearance_out, obstacle_out, capsule_out, colliding_out, stream
    "ikf_world_track_clearance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # q, T, k, q_start, reject_self, self_min_clearance, edge_free_out, stream
    "ikf_sweep_lattice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
}

# ... every symbol include/ikflow_amd_manip.h declares (singularity rule: a floor under the manipulability measure of a candidate)
IKF_MANIP_FULL, IKF_MANIP_LINEAR, IKF_MANIP_ANGULAR = 0, 1, 2
MANIP_PARTS = {"full": IKF_MANIP_FULL, "linear": IKF_MANIP_LINEAR, "angular": IKF_MANIP_ANGULAR}
MANIP_SIGNATURES = {
    # part, min_manipulability
    "ikf_set_min_manipulability": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "ikf_min_manipulability": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    # q, n, part, min_manipulability, w_out, below_out, stream
    "ikf_manipulability": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
}

LIB_PATH = _build.LIB_PATH
_libs = {}


def load(flavour: str = "") -> C.CDLL:
    """dlopen the in-tree library and bind every declared symbol. Raises if anything is missing.
    flavour "probes": lib/libikflow_amd_probes.so (-DIKF_PROBES: the product plus the priced-and-rejected forms of rounds 2 - 3; tests and
    tools only - both flavours may be loaded in one process, each handle belongs to the library that created it)."""
    if flavour in _libs:
        return _libs[flavour]
    LIB_PATH = _build.lib_path(flavour)
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP engine has not been built (run `python -m ikflow_amd.build{' --probes' if flavour else ''}`). "
            "ikflow_amd has no CPU path."
        )
    # torch FIRST: it ships its own copy of the HIP runtime (torch/lib/libamdhip64.so); if this library were loaded before
    # torch, the loader would bind it to /opt/rocm's copy and the process would hold two HIP runtimes, the second of which sees
    # no device ("ikf_create: no HIP device visible" although torch.cuda.is_available()).  With torch's copy already mapped, this
    # library's libamdhip64.so.7 dependency resolves to it.  (A C / C++ client without torch links /opt/rocm's copy alone.)
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in list(SIGNATURES.items()) + list(RANK_SIGNATURES.items()) + list(PATH_SIGNATURES.items()) + list(PATH_BATCH_SIGNATURES.items()) + list(PATH_OPT_SIGNATURES.items()) + list(DIVERSE_SIGNATURES.items()) + list(WORLD_SIGNATURES.items()) + list(CLOUD_SIGNATURES.items()) + list(SWEEP_SIGNATURES.items()) + list(REFINE_SIGNATURES.items()) + list(EXACT_WORLD_SIGNATURES.items()) + list(TRACK_SIGNATURES.items()) + list(MANIP_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.ikf_abi_version()
    if got != IKF_ABI_VERSION:
        raise ImportError(f"libikflow_amd.so ABI {got} != binding ABI {IKF_ABI_VERSION}; rebuild the library")
    if bool(lib.ikf_probes_build()) != (flavour == "probes"):
        raise ImportError(f"{LIB_PATH} is not the {'probes' if flavour else 'product'} flavour; rebuild it")
    _libs[flavour] = lib
    return lib


def last_error(lib: C.CDLL = None) -> str:
    return (lib or load()).ikf_last_error().decode("utf-8", "replace")
