"""ctypes binding of libbenchpush_hip.so (C ABI: include/benchpush_amd.h).

There is no CPU fallback: if the HIP library is missing or no GPU is usable, loading / bp_create raise.
"""
import ctypes as C
import os

from .build import LIB_PATH

MAXV = 20
MAX_SHIP_VERTS = 32
MAX_WHEELS = 4
ENV_SHIP_ICE, ENV_MAZE, ENV_BOX = 0, 1, 2
BD_MAXBOX, BD_MAXWP = 24, 64
BD_INFO_KEYS = ["x", "y", "theta", "cumulative_distance", "cumulative_boxes", "cumulative_reward", "total_work", "ministeps", "inactivity",
                "robot_hit_obstacle", "substeps", "robot_distance", "boxes_distance", "num_waypoints", "num_boxes_left", "work"]
INFO_COUNT = 16
EPM_COUNT, EPM_RING = 6, 8
INFO_KEYS = ["x", "y", "theta", "total_work", "work", "collision_reward", "scaled_collision_reward", "dist_reward",
             "trial_success", "boundary_violated", "yaw_violated", "total_ke", "total_impulse", "n_post_solve",
             "n_contact_pts", "n_first_contact"]
ERRORS = {0: "BP_OK", -1: "BP_EINVAL", -2: "BP_ENOMEM", -3: "BP_EHIP", -4: "BP_ENODEVICE", -5: "BP_ESTATE", -6: "BP_ECAPACITY"}
GTSP_OK, GTSP_NOTHING_TO_PUSH, GTSP_SKIPPED, GTSP_CAP, GTSP_INVALID = range(5)
GTSP_STATUS_MASK, GTSP_FLAG_VANISHED, GTSP_FLAG_DEGENERATE = 0xFF, 0x100, 0x200   # status = code | flags
GTSP_MAX_BOXES, GTSP_MAX_GOALS, GTSP_MAX_SLOTS = 12, 8, 64
RRT_FOUND, RRT_FOUND_IGNORING_BOXES, RRT_FALLBACK, RRT_BLOCKED, RRT_CAP, RRT_BAD_INPUT, RRT_SKIPPED = range(7)
RRT_MAX_WALLS, RRT_MAX_BOX_VERTS = 128, 1280   # bp_rrt_plan: walls, and box slots times vertices per slot, at most
TRACK_NONE, TRACK_GENTLE, TRACK_PID, TRACK_NEAR = 0, 1, 2, 3
LATTICE_FOUND, LATTICE_NO_PATH, LATTICE_CAP, LATTICE_SKIPPED = 0, 1, 2, 3
LATTICE_MAX_EDGES = 32   # bp_lattice_search: edges per base heading at most
SWATH_CLIP, SWATH_REJECT = 0, 1
SWATH_MAX_WORDS = 4096   # bp_swath_cost: H * ceil(W / 64) at most (the swath's bit image lives in LDS)
QUEUE_FULL_ONLY = 1   # BP_QUEUE_FULL_ONLY: bp_bd_queue_recv takes nothing while fewer than M ids are queued and an env is still busy
STATE_TRUSTED = 1    # BP_STATE_TRUSTED: bp_load_state / bp_clone_state skip the argument checks and the synchronisation


class BpCostmapConfig(C.Structure):
    _fields_ = [("scale", C.c_double), ("m", C.c_int32), ("n", C.c_int32), ("alpha", C.c_double), ("ship_mass", C.c_double),
                ("horizon", C.c_double), ("margin", C.c_int32), ("pad_", C.c_int32)]


class BpSwathConfig(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("P", C.c_int32), ("nv", C.c_int32), ("outside", C.c_int32),
                ("map_stride", C.c_int64)]


class BpReplayDesc(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("num_envs", C.c_int32), ("device", C.c_int32), ("action_dim", C.c_int32), ("row_bytes", C.c_int64),
                ("max_rows", C.c_int32), ("pad_", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("state", "next_state", "action", "reward", "ministeps", "nonfinal", "env", "pend_obs", "pend_action",
                                          "pend_flags", "hdr", "row_slot", "win")]


class BpReplayBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("state", "next_state", "action", "reward", "ministeps", "nonfinal", "slot", "valid")]


class BpRolloutDesc(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("num_envs", C.c_int32), ("device", C.c_int32), ("action_dim", C.c_int32), ("row_bytes", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("obs", "action", "reward", "value", "logp", "advantage", "ret", "episode_start", "last_done", "hdr")]


class BpRolloutBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "action", "value", "logp", "advantage", "ret", "index", "valid")]


class BpTransitionsDesc(C.Structure):
    _fields_ = [("steps", C.c_int32), ("num_envs", C.c_int32), ("device", C.c_int32), ("action_dim", C.c_int32), ("row_bytes", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("obs", "next_obs", "action", "reward", "done", "timeout", "hdr")]


class BpTransitionsBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "next_obs", "action", "reward", "done", "slot", "valid")]


class BpLatticeConfig(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("S", C.c_int32), ("nh", C.c_int32), ("nb", C.c_int32), ("ne_max", C.c_int32), ("den", C.c_int32),
                ("margin", C.c_int32), ("h_baseline", C.c_int32), ("max_expansions", C.c_int32), ("node_capacity", C.c_int32),
                ("queue_capacity", C.c_int32), ("max_path_nodes", C.c_int32), ("pad_", C.c_int32), ("map_stride", C.c_int64),
                ("mask_stride", C.c_int64), ("unit", C.c_double), ("weight", C.c_double), ("turning_radius", C.c_double)]


class BpTrackConfig(C.Structure):
    _fields_ = [("P", C.c_int32), ("pad_", C.c_int32)] + [(n, C.c_double) for n in (
        "thresh", "look_car", "d_back", "d_ahead", "kp", "ki", "kd", "i_cap", "dead", "straight_ang", "yaw_big", "omega_small", "kp_v", "ki_v", "v_max",
        "omega_max", "dt", "action_scale")]


class BpRrtConfig(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("step", "goal_radius", "goal_bias", "densify_ds", "prune_min_dist", "inflate_radius")] + [
        ("seed", C.c_uint64), ("max_nodes", C.c_int32), ("max_waypoints", C.c_int32), ("passes", C.c_int32), ("pad_", C.c_int32)]


class BpTrackWpConfig(C.Structure):
    _fields_ = [("P", C.c_int32), ("pad_", C.c_int32), ("Lfc", C.c_double), ("dt", C.c_double), ("action_scale", C.c_double)]


class BpGtspConfig(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("shrink", "extend", "lin_vel", "ang_vel", "Lfc", "dt", "target_speed", "switch_dist", "v_scale", "w_scale")] + [
        ("round_decimals", C.c_int32), ("max_boxes", C.c_int32), ("num_goals", C.c_int32), ("pad_", C.c_int32)]


class BpConfig(C.Structure):
    _fields_ = [("dt", C.c_double), ("steps", C.c_int32), ("iterations", C.c_int32), ("persistence", C.c_int32),
                ("settle_steps", C.c_int32), ("damping_pow", C.c_double), ("bias_coef", C.c_double), ("slop", C.c_double),
                ("target_speed", C.c_double), ("max_yaw_rate", C.c_double), ("map_w", C.c_double), ("map_h", C.c_double),
                ("goal_y", C.c_double), ("m_to_pix", C.c_double), ("density", C.c_double), ("poly_radius", C.c_double),
                ("elasticity", C.c_double), ("friction", C.c_double), ("beta", C.c_double),
                ("boundary_penalty", C.c_double), ("terminal_reward", C.c_double), ("local_w", C.c_double),
                ("local_h", C.c_double), ("vshift", C.c_double), ("obs_range", C.c_double),
                ("num_ship_verts", C.c_int32), ("_pad", C.c_int32),
                ("ship_verts", (C.c_double * 2) * MAX_SHIP_VERTS), ("ship_head", C.c_double * 2),
                ("ship_tail", C.c_double * 2),
                ("env_kind", C.c_int32), ("num_wheels", C.c_int32), ("wheel_verts", ((C.c_double * 2) * 4) * MAX_WHEELS),
                ("goal_x", C.c_double), ("goal_reach", C.c_double), ("k_increment", C.c_double), ("wall_radius", C.c_double),
                ("obstacle_size", C.c_double),
                ("random_start", C.c_int32), ("_pad2", C.c_int32), ("start_x_range", C.c_double), ("start_seed", C.c_uint64),
                ("ship_mass", C.c_double)]


class BpBdConfig(C.Structure):
    _fields_ = [("ctrl_dt", C.c_double), ("steps", C.c_int32), ("iterations", C.c_int32), ("persistence", C.c_int32), ("settle_steps", C.c_int32),
                ("damping_pow", C.c_double), ("bias_coef", C.c_double), ("slop", C.c_double),
                ("room_length", C.c_double), ("room_width", C.c_double), ("recept_x", C.c_double), ("recept_y", C.c_double),
                ("recept_size", C.c_double), ("ppm", C.c_double), ("local_w", C.c_double), ("local_px", C.c_int32),
                ("use_correct_direction_reward", C.c_int32), ("robot_radius", C.c_double), ("robot_half_width", C.c_double),
                ("step_size", C.c_double), ("target_speed", C.c_double), ("partial_rewards_scale", C.c_double), ("goal_reward", C.c_double),
                ("collision_penalty", C.c_double), ("non_movement_penalty", C.c_double), ("correct_direction_reward_scale", C.c_double),
                ("ministep_size", C.c_double), ("sp_channel_scale", C.c_double), ("inactivity_cutoff", C.c_int32),
                ("invert_receptacle_map", C.c_int32), ("num_boxes", C.c_int32), ("step_limit", C.c_int32),
                ("action_type", C.c_int32), ("task", C.c_int32), ("omega_scale", C.c_double), ("v_scale", C.c_double), ("lfc", C.c_double),
                ("yaw_rate_step", C.c_double), ("t_max", C.c_int32), ("num_goal_points", C.c_int32), ("num_boundary_verts", C.c_int32),
                ("num_outer_verts", C.c_int32), ("boundary_penalty", C.c_double), ("box_cleared_reward", C.c_double),
                ("box_putback_penalty", C.c_double), ("truncation_penalty", C.c_double), ("terminal_reward", C.c_double),
                ("pushing_mult", C.c_double), ("distance_scale_max", C.c_double), ("boundary", (C.c_double * 2) * 8),
                ("outer_boundary", (C.c_double * 2) * 8), ("footprint_verts", (C.c_double * 2) * 4), ("goal_points", (C.c_double * 2) * 128),
                ("box_half", C.c_double), ("box_density", C.c_double), ("robot_verts", (C.c_double * 2) * 4),
                ("wheel_verts", ((C.c_double * 2) * 4) * 4), ("bumper_verts", (C.c_double * 2) * 4), ("robot_mass", C.c_double)]


def _abi():
    """The C ABI as one table: name -> (restype, argtypes, group).  group None: every supported library has the symbol; otherwise the probe symbol of
    the feature it came with -- a library without the probe (an older build loaded for a same-box comparison) goes without the whole group.
    tests/test_host_cpu.py holds the table against the prototypes of include/benchpush_amd.h."""
    from .render import RenderArgs, RenderPrim
    P, I, vp, i32, i64, u64, f64 = C.POINTER, C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    step_out = [vp] * 5                                          # obs, reward, terminated, truncated, info
    groups = {
        None: {
            "bp_abi_version": (i32, []), "bp_last_error": (C.c_char_p, [vp]),
            "bp_create": (I, [P(BpConfig), i32, i64, i32, P(vp)]), "bp_destroy": (I, [vp]),
            "bp_load_scenarios": (I, [vp, i32, i32, i32, vp, vp, vp, vp, vp]), "bp_load_maze": (I, [vp, i32, i32, vp, i32, vp, vp]),
            "bp_get_goal_map": (I, [vp, vp, P(i32), P(i32)]),
            "bp_reset": (I, [vp, vp, vp, vp, vp]), "bp_step": (I, [vp, vp] + step_out + [vp]), "bp_step_physics": (I, [vp, vp, vp, vp, vp, vp, vp]),
            "bp_observe": (I, [vp, vp, vp, vp]), "bp_observe_global": (I, [vp, vp, vp, vp]), "bp_set_resettle": (I, [vp, i32]),
            "bp_get_world_polys": (I, [vp, vp, vp, vp]), "bp_get_body_state": (I, [vp, vp, vp]), "bp_get_low_dim_obs": (I, [vp, vp, vp]),
            "bp_costmap_update": (I, [vp, P(BpCostmapConfig), vp, f64, vp, vp]),
            "bp_get_episode_metrics": (I, [vp, vp, vp, vp]), "bp_start_uniform": (f64, [u64, i64, i64]),
            "bp_debug_round2": (I, [vp, vp, i32, vp]), "bp_copy_rows_masked": (I, [vp, vp, vp, vp, i64, i64, vp]),
            "bp_nb_cap": (i32, [vp]), "bp_obs_height": (i32, [vp]), "bp_obs_width": (i32, [vp]),
            "bp_get_num_bodies": (I, [vp, vp]), "bp_check_errors": (I, [vp, vp]),
            "bp_kernel_time_ms": (I, [vp, P(f64), P(f64), P(i32)]), "bp_enable_timing": (I, [vp, i32]),
            "bp_get_step_cycles": (I, [vp, vp]), "bp_set_step_cost_hint": (I, [vp, vp]),
            "bp_sched_chunk": (i32, [vp]), "bp_sched_resident": (i32, [vp]), "bp_pair_mode": (i32, [vp]), "bp_get_pair_stats": (I, [vp, vp]),
            "bp_bd_create": (I, [P(BpBdConfig), i32, i64, i32, P(vp)]), "bp_bd_load": (I, [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
            "bp_bd_get_maps": (I, [vp, i32, vp, vp, vp, vp, vp, vp]), "bp_bd_get_state": (I, [vp, vp, vp, vp]), "bp_bd_get_stragglers": (I, [vp, vp]),
        },
        "bp_get_episode_history": {"bp_get_episode_history": (I, [vp, vp, vp, vp, vp])},
        "bp_debug_scramble_hints": {"bp_debug_scramble_hints": (I, [vp, u64, vp])},
        "bp_device_shared": {   # ABI 11
            "bp_device_shared": (i32, [vp]), "bp_bd_budget": (i32, [vp]), "bp_launch_policy_query": (I, [i32, i32, i32, i32, vp]),
            "bp_get_cost_stats": (I, [vp, vp, i32, P(i32)])},
        "bp_bd_get_cycle_skips": {"bp_bd_get_cycle_skips": (I, [vp, vp])},
        "bp_get_clock_stamps": {"bp_get_clock_stamps": (I, [vp, vp])},
        "bp_sched_warnings": {"bp_sched_warnings": (I, [vp, vp])},   # absent from libraries of ABI 6
        "bp_bd_step_async": {   # asynchronous step
            "bp_bd_step_async": (I, [vp, vp, i32] + step_out + [vp, vp, vp]), "bp_bd_async_drain": (I, [vp] + step_out + [vp, vp, vp]),
            "bp_bd_async_open": (i32, [vp])},
        "bp_bd_queue_open": {   # ready queue of the asynchronous step
            "bp_bd_queue_open": (I, [vp, i32, vp]), "bp_bd_queue_recv": (I, [vp, i32, i32] + [vp] * 16), "bp_bd_queue_send": (I, [vp] * 7),
            "bp_bd_queue_close": (I, [vp] * 9), "bp_bd_queue_batch": (i32, [vp])},
        "bp_task_metric_row": {   # episode metrics of box handles
            "bp_bd_get_episode_boxes": (I, [vp, vp, vp]), "bp_bd_get_completed": (I, [vp, vp]),
            "bp_task_metric_row": (I, [i32, vp, vp, i32, vp, vp, f64, f64, f64, f64, f64, vp])},
        "bp_render": {
            "bp_set_render_table": (I, [vp, i32, i32, vp, vp, i32, vp]), "bp_render": (I, [vp, P(RenderArgs), vp, i32, vp, vp, vp, vp])},
        "bp_save_state": {   # state records
            "bp_state_bytes": (i64, [vp]), "bp_state_layout_id": (u64, [vp]), "bp_save_state": (I, [vp, vp, i32, vp, vp]),
            "bp_load_state": (I, [vp, vp, i32, vp, i32, vp]), "bp_clone_state": (I, [vp, vp, vp, i32, i32, vp]),
            "bp_state_layout_query": (I, [i32, i32, i32, i32, i32, vp, vp, vp, P(i64), P(u64)])},
        "bp_swath_cost": {"bp_swath_cost": (I, [vp, P(BpSwathConfig)] + [vp] * 8)},
        "bp_lattice_search": {
            "bp_lattice_workspace_bytes": (i64, [P(BpLatticeConfig), i32]),
            "bp_lattice_search": (I, [vp, P(BpLatticeConfig)] + [vp] * 10 + [i64] + [vp] * 7)},
        "bp_track_path": {"bp_track_path": (I, [vp, P(BpTrackConfig), vp, i64] + [vp] * 8)},
        "bp_rrt_plan": {   # batched RRT and its waypoint controller
            "bp_rrt_workspace_bytes": (i64, [P(BpRrtConfig), i32]), "bp_rrt_uniform": (f64, [u64, i64, i32, i32, i32]),
            "bp_rrt_plan": (I, [vp, P(BpRrtConfig), vp, vp, vp, i32, vp, vp, i32, i32, vp, vp, vp, i64] + [vp] * 6),
            "bp_track_waypoints": (I, [vp, P(BpTrackWpConfig)] + [vp] * 7)},
        "bp_gtsp_plan": {   # the GTSP push planner and its controller
            "bp_gtsp_workspace_bytes": (i64, [P(BpGtspConfig), i32]),
            "bp_gtsp_plan": (I, [vp, P(BpGtspConfig), vp, vp, vp, i32, i32, vp, vp, vp, i64] + [vp] * 10),
            "bp_gtsp_track": (I, [vp, P(BpGtspConfig)] + [vp] * 9)},
        "bp_replay_observe": {   # replay buffer on the ready queue
            "bp_replay_index": (i64, [u64, i64, i32, i64]), "bp_replay_observe": (I, [P(BpReplayDesc)] + [vp] * 7 + [i32, i32, vp]),
            "bp_replay_record": (I, [P(BpReplayDesc), vp, vp, vp, i32, vp]),
            "bp_replay_sample": (I, [P(BpReplayDesc), i32, u64, P(BpReplayBatch), vp])},
        "bp_rollout_begin": {   # on-policy rollout buffer with GAE
            "bp_rollout_index": (i64, [u64, i64, i64, i64]), "bp_rollout_begin": (I, [P(BpRolloutDesc), i32, vp, vp, vp, vp, vp]),
            "bp_rollout_pick_rows": (I, [P(BpRolloutDesc), vp, vp, i32, vp, vp, vp]),
            "bp_rollout_end": (I, [P(BpRolloutDesc), i32, vp, vp, vp, vp, i32, f64, vp]),
            "bp_rollout_finish": (I, [P(BpRolloutDesc), vp, f64, f64, vp]),
            "bp_rollout_minibatch": (I, [P(BpRolloutDesc), u64, i64, i32, i32, P(BpRolloutBatch), vp])},
        "bp_transitions_add": {   # transition buffer for lock-step envs
            "bp_transitions_add": (I, [P(BpTransitionsDesc)] + [vp] * 8),
            "bp_transitions_sample": (I, [P(BpTransitionsDesc), u64, i32, P(BpTransitionsBatch), vp])},
    }
    # (sizeof function, the struct it measures, group, the error when the two disagree); the functions join their groups in the table
    layouts = [("bp_sizeof_config", BpConfig, None, "bp_config layout mismatch between _lib.BpConfig and the library"),
               ("bp_bd_sizeof_config", BpBdConfig, None, "bp_bd_config layout mismatch between _lib.BpBdConfig and the library"),
               ("bp_sizeof_render_args", RenderArgs, "bp_render", "bp_render_args / bp_render_prim layout mismatch between benchpush_amd.render and the library"),
               ("bp_sizeof_render_prim", RenderPrim, "bp_render", "bp_render_args / bp_render_prim layout mismatch between benchpush_amd.render and the library"),
               ("bp_sizeof_swath_config", BpSwathConfig, "bp_swath_cost", "bp_swath_config layout mismatch between _lib.BpSwathConfig and the library"),
               ("bp_sizeof_lattice_config", BpLatticeConfig, "bp_lattice_search", "bp_lattice_config layout mismatch between _lib.BpLatticeConfig and the library"),
               ("bp_sizeof_track_config", BpTrackConfig, "bp_track_path", "bp_track_config layout mismatch between _lib.BpTrackConfig and the library"),
               ("bp_sizeof_rrt_config", BpRrtConfig, "bp_rrt_plan", "bp_rrt_config / bp_track_wp_config layout mismatch between _lib and the library"),
               ("bp_sizeof_track_wp_config", BpTrackWpConfig, "bp_rrt_plan", "bp_rrt_config / bp_track_wp_config layout mismatch between _lib and the library"),
               ("bp_sizeof_gtsp_config", BpGtspConfig, "bp_gtsp_plan", "bp_gtsp_config layout mismatch between _lib.BpGtspConfig and the library"),
               ("bp_sizeof_replay_desc", BpReplayDesc, "bp_replay_observe", "bp_replay_desc / bp_replay_batch layout mismatch between _lib and the library"),
               ("bp_sizeof_replay_batch", BpReplayBatch, "bp_replay_observe", "bp_replay_desc / bp_replay_batch layout mismatch between _lib and the library"),
               ("bp_sizeof_rollout_desc", BpRolloutDesc, "bp_rollout_begin", "bp_rollout_desc / bp_rollout_batch layout mismatch between _lib and the library"),
               ("bp_sizeof_rollout_batch", BpRolloutBatch, "bp_rollout_begin", "bp_rollout_desc / bp_rollout_batch layout mismatch between _lib and the library"),
               ("bp_sizeof_transitions_desc", BpTransitionsDesc, "bp_transitions_add",
                "bp_transitions_desc / bp_transitions_batch layout mismatch between _lib and the library"),
               ("bp_sizeof_transitions_batch", BpTransitionsBatch, "bp_transitions_add",
                "bp_transitions_desc / bp_transitions_batch layout mismatch between _lib and the library")]
    table = {name: decl + (group,) for group, fns in groups.items() for name, decl in fns.items()}
    table.update((name, (i32, [], group)) for name, _, group, _ in layouts)
    # entry points of the library that the header does not declare: the diagnostic twins' hooks (tools/, tests of the twins)
    diagnostic = {"bp_debug_trace": (I, [vp, vp, i32], None), "bp_debug_prof": (I, [vp, vp], None)}
    return table, diagnostic, [(name, struct, what) for name, struct, _, what in layouts]


ABI, DIAGNOSTIC_ABI, LAYOUTS = _abi()
EXPORTS = list(ABI)


class BpError(RuntimeError):
    pass


_lib = None


def load():
    """Load the HIP library; raises if it has not been built (python -m benchpush_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BpError("libbenchpush_hip.so not found at %s -- build it with `python -m benchpush_amd.build` "
                      "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    try:  # torch ships its own HIP runtime: load it first so that this library binds to the same copy (device memory and
        import torch  # noqa: F401   streams are shared with torch; two runtimes in one process do not see each other's devices)
    except ImportError:
        pass
    path = LIB_PATH
    if os.environ.get("BP_PROF") == "1":  # diagnostic build with in-kernel phase timers (tools/prof_phases.py)
        path = os.environ.get("BP_PROF_LIB", LIB_PATH.replace(".so", "_prof.so"))
    L = C.CDLL(path)
    for name, (restype, argtypes, group) in list(ABI.items()) + list(DIAGNOSTIC_ABI.items()):
        if group is None or hasattr(L, group):   # (a symbol that is missing although its group is there: AttributeError)
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    for sizeof, struct, what in LAYOUTS:
        if hasattr(L, sizeof):
            sizes = {C.sizeof(struct)}
            if struct is BpBdConfig and not hasattr(L, "bp_task_metric_row"):
                sizes.add(C.sizeof(struct) - 8)   # a build from before the episode metrics of these handles has no robot_mass at the end and reads the rest
            if getattr(L, sizeof)() not in sizes:
                raise BpError(what)
    _lib = L
    return L


def state_layout(env_kind, nbcap, task=0, map_cells=0):
    """The state-record layout as a pure function of the shapes (bp_state_layout_query; no GPU, no handle): dict of offsets / bytes / widths per segment
    (segment 0 is the header), the record size and the structural part of the layout id."""
    import numpy as np
    L = load()
    n = L.bp_state_layout_query(int(env_kind), int(task), int(nbcap), int(map_cells), 0, None, None, None, None, None)
    if n < 0:
        raise BpError("bp_state_layout_query failed: %s (%d)" % (ERRORS.get(n, "?"), n))
    off, nbytes, width = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
    total, sid = C.c_int64(), C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    L.bp_state_layout_query(int(env_kind), int(task), int(nbcap), int(map_cells), n, p(off), p(nbytes), p(width), C.byref(total), C.byref(sid))
    return {"offsets": off, "bytes": nbytes, "widths": width, "total": int(total.value), "structure_id": int(sid.value)}


def check(L, h, rc, what):
    if rc != 0:
        msg = L.bp_last_error(h).decode() if h else ""
        raise BpError("%s failed: %s (%d) %s" % (what, ERRORS.get(rc, "?"), rc, msg))


def make_config(params, ship_vertices, head, tail, env_kind=ENV_SHIP_ICE, wheel_vertices=None, obstacle_size=0.0):
    cfg = BpConfig()
    fields = {f[0] for f in BpConfig._fields_}
    for k, v in params.items():
        if k in fields:
            setattr(cfg, k, v)
    cfg.env_kind = env_kind
    cfg.obstacle_size = float(obstacle_size)
    wheels = [] if wheel_vertices is None else wheel_vertices
    if len(wheels) > MAX_WHEELS:
        raise ValueError("too many wheels")
    cfg.num_wheels = len(wheels)
    for w, quad in enumerate(wheels):
        if len(quad) != 4:
            raise ValueError("wheel outlines must have 4 vertices")
        for i, (x, y) in enumerate(quad):
            cfg.wheel_verts[w][i][0] = float(x)
            cfg.wheel_verts[w][i][1] = float(y)
    sv = [list(map(float, v)) for v in ship_vertices]
    if len(sv) > MAX_SHIP_VERTS:
        raise ValueError("too many ship vertices")
    cfg.num_ship_verts = len(sv)
    for i, (x, y) in enumerate(sv):
        cfg.ship_verts[i][0] = x
        cfg.ship_verts[i][1] = y
    cfg.ship_head[0], cfg.ship_head[1] = float(head[0]), float(head[1])
    cfg.ship_tail[0], cfg.ship_tail[1] = float(tail[0]), float(tail[1])
    return cfg


def make_bd_config(phys, bd, cfg):
    """bp_bd_config from box_delivery_scenario.box_delivery_physics_params / box_delivery_params and the merged cfg."""
    c = BpBdConfig()
    fields = {f[0] for f in BpBdConfig._fields_}
    for src in (phys, bd):
        for k, v in src.items():
            if k in fields:
                setattr(c, k, v)
    c.ctrl_dt = float(phys["dt"])
    c.robot_mass = float(cfg.agent.mass)     # TaskDrivenMetric(robot_mass=cfg.agent.mass) in the reference's baselines
    if bd.get("task", 0) == 1:      # area-clearing: boxes are squares of half-size obstacle_size, density sim.obstacle_density
        c.box_half = float(cfg.obstacle_size)
        c.box_density = float(cfg.sim.obstacle_density)
    else:
        c.box_half = float(cfg.boxes.box_size) / 2
        c.box_density = float(cfg.boxes.box_density)
    for i, (x, y) in enumerate(cfg.agent.vertices):
        c.robot_verts[i][0], c.robot_verts[i][1] = float(x), float(y)
    for w, quad in enumerate(cfg.agent.wheel_vertices):
        for i, (x, y) in enumerate(quad):
            c.wheel_verts[w][i][0], c.wheel_verts[w][i][1] = float(x), float(y)
    for i, (x, y) in enumerate(cfg.agent.front_bumper_vertices):
        c.bumper_verts[i][0], c.bumper_verts[i][1] = float(x), float(y)
    return c


def fill_area_geometry(c, boundary, outer_boundary, footprint, goal_points):
    """area-clearing geometry of bp_bd_config (convex boundary polygons with at most 8 vertices, at most 128 goal points)."""
    if len(boundary) > 8 or len(outer_boundary) > 8 or len(goal_points) > 128 or len(footprint) != 4:
        raise ValueError("area-clearing geometry exceeds the ABI capacities")
    c.num_boundary_verts, c.num_outer_verts, c.num_goal_points = len(boundary), len(outer_boundary), len(goal_points)
    for i, (x, y) in enumerate(boundary):
        c.boundary[i][0], c.boundary[i][1] = float(x), float(y)
    for i, (x, y) in enumerate(outer_boundary):
        c.outer_boundary[i][0], c.outer_boundary[i][1] = float(x), float(y)
    for i, (x, y) in enumerate(footprint):
        c.footprint_verts[i][0], c.footprint_verts[i][1] = float(x), float(y)
    for i, (x, y) in enumerate(goal_points):
        c.goal_points[i][0], c.goal_points[i][1] = float(x), float(y)
    return c
