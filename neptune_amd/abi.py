"""ctypes mirror of include/neptune_backend.h (the C ABI of the back-end path).

Only layouts and constants live here; no compute.  Field order and sizes must match the header
exactly (tests/test_abi.py checks sizeof() against the values the C library reports).
"""
import ctypes as C

import numpy as np

NEP_MAX_POL = 8
NEP_TRAJ_MAX_SEG = 16
NEP_HULL_MAX_V = 16
NEP_HULL_MAX_CP = 16
NEP_MAX_BEND = 8
NEP_STATE_DOUBLES = 12

NEP_OK, NEP_RELAXED, NEP_FAILED = 0, 1, 2
NEP_SKIPPED = 3          # nep_stats.status of a slot outside the active set (nep_batch_set_active)
NEP_GUESS = 4            # nep_stats.status: both solves failed and nep_batch_guess_fallback published the front end's guess
NEP_FE_SKIPPED = 4       # nep_fe_result.status of a slot outside the active set
NEP_FE_PAD_GATED, NEP_FE_PAD_GOAL_TAKEN = 32, 64      # nep_fe_result._pad bits 5 and 6: turned down / let through by nep_batch_goal_gate
GOAL_GATE_COUNTS = ("examined", "goal_taken", "gated", "unused")      # nep_batch_goal_gate's d_count [n_scenes][4]
# nep_batch_guess_fallback's ([0], [1]) and nep_batch_guess_fallback_tally's ([2], [3]) d_count [n_scenes][4]
GUESS_FALLBACK_COUNTS = ("qp_failed_seen", "guess_published", "guess_flown", "guess_not_flown")


class nep_pwp(C.Structure):
    """mt::PieceWisePol (reference neptune/include/mader_types.hpp:462-548)."""
    _fields_ = [("n_seg", C.c_int32), ("_pad", C.c_int32),
                ("times", C.c_double * (NEP_TRAJ_MAX_SEG + 1)),
                ("coeff", ((C.c_double * 4) * NEP_TRAJ_MAX_SEG) * 3)]


class nep_traj_rec(C.Structure):
    """mader_msgs/DynTraj (reference mader_msgs/msg/DynTraj.msg:1-9) as a fixed-size record."""
    _fields_ = [("id", C.c_int32), ("is_agent", C.c_int32), ("n_bend", C.c_int32),
                ("valid", C.c_int32),
                ("bbox", C.c_double * 3), ("pos", C.c_double * 3),
                ("bend", (C.c_double * 2) * NEP_MAX_BEND),
                ("pwp", nep_pwp)]


class nep_backend_cfg(C.Structure):
    _fields_ = [("num_pol", C.c_int32), ("deg_pol", C.c_int32), ("id", C.c_int32),
                ("num_agents", C.c_int32),
                ("T_span", C.c_double), ("weight_term", C.c_double), ("rad_term", C.c_double),
                ("use_linear_constraints", C.c_int32), ("_pad", C.c_int32),
                ("pb", C.POINTER(C.c_double))]


class nep_ent_view(C.Structure):
    _fields_ = [("n_states", C.c_int32), ("n_active", C.c_int32),
                ("alpha_off", C.POINTER(C.c_int32)), ("alphas", C.POINTER(C.c_int32)),
                ("active_cases", C.POINTER(C.c_int32)),
                ("bend_off", C.POINTER(C.c_int32)), ("bend_xy", C.POINTER(C.c_double))]


class nep_stats(C.Structure):
    _fields_ = [("status", C.c_int32), ("iters", C.c_int32), ("iters_first", C.c_int32),
                ("n_lines", C.c_int32), ("n_lp", C.c_int32), ("n_lp_failed", C.c_int32),
                ("n_rows", C.c_int32), ("qc_active", C.c_int32),
                ("objective", C.c_double), ("solve_us", C.c_double)]


class nep_batch_cfg(C.Structure):
    _fields_ = [("num_agents", C.c_int32), ("first_local", C.c_int32), ("n_local", C.c_int32),
                ("num_pol", C.c_int32), ("n_static", C.c_int32), ("enable_entangle", C.c_int32),
                ("max_states", C.c_int32), ("n_scenes", C.c_int32),
                ("T_span", C.c_double), ("weight_term", C.c_double), ("dc", C.c_double),
                ("drone_radius", C.c_double),
                ("x_min", C.c_double), ("x_max", C.c_double), ("y_min", C.c_double),
                ("y_max", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double),
                ("v_max", C.c_double), ("a_max", C.c_double),
                ("pb", C.POINTER(C.c_double)), ("static_off", C.POINTER(C.c_int32)),
                ("static_xy", C.POINTER(C.c_double))]


class nep_guess(C.Structure):
    _fields_ = [("K", C.c_int32), ("n_alpha", C.c_int32), ("t_start", C.c_double),
                ("coeff", ((C.c_double * 4) * NEP_MAX_POL) * 3)]


class nep_solution(C.Structure):
    _fields_ = [("stats", nep_stats), ("K", C.c_int32), ("n_states", C.c_int32),
                ("times", C.c_double * (NEP_MAX_POL + 1)),
                ("coeff", ((C.c_double * 4) * NEP_MAX_POL) * 3)]


# numpy structured dtypes with identical layout (used for device<->host staging through torch)
class nep_wire_header(C.Structure):
    """ROS Header fields of a DynTraj message on the wire (include/neptune_plan.h)."""
    _fields_ = [("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
                ("_pad", C.c_uint32), ("frame_id", C.c_char_p)]


class nep_plan_cfg(C.Structure):
    """The yaml parameters replanFull's plan handling reads (neptune.cpp:1366-1425,1713-1720)."""
    _fields_ = [("dc", C.c_double), ("T_span", C.c_double), ("lower_bound_runtime", C.c_double),
                ("upper_bound_runtime", C.c_double), ("runtime_opt", C.c_double),
                ("factor_alpha", C.c_double), ("deltaT0", C.c_int32), ("_pad", C.c_int32)]


class nep_point_a(C.Structure):
    _fields_ = [("A", C.c_double * 12), ("k_index", C.c_int32), ("k_index_end", C.c_int32),
                ("runtime_search", C.c_double), ("t_start", C.c_double)]


class nep_ent_cfg(C.Structure):
    """include/neptune_entangle.h: what KinodynamicSearch holds for the entangle check."""
    _fields_ = [("num_agents", C.c_int32), ("id", C.c_int32), ("num_pol", C.c_int32), ("num_samples", C.c_int32),
                ("T_span", C.c_double), ("cable_length", C.c_double), ("n_static", C.c_int32), ("_pad", C.c_int32),
                ("pb", C.POINTER(C.c_double)), ("static_rep", C.POINTER(C.c_double)), ("static_longest", C.POINTER(C.c_double))]


class nep_ent_inputs(C.Structure):
    _fields_ = [("sampled", C.POINTER(C.c_double)), ("present", C.POINTER(C.c_int32)),
                ("bend_off", C.POINTER(C.c_int32)), ("bend_xy", C.POINTER(C.c_double))]


class nep_ent_state(C.Structure):
    _fields_ = [("n_alpha", C.c_int32), ("n_bend", C.c_int32), ("cap", C.c_int32), ("n_active", C.c_int32),
                ("alphas", C.POINTER(C.c_int32)), ("betas", C.POINTER(C.c_double)), ("bend_idx", C.POINTER(C.c_int32)),
                ("active_cases", C.POINTER(C.c_int32))]


class nep_ent_track_inputs(C.Structure):
    """include/neptune_entangle.h: the other agents at one tracking check (nep_ent_track_step)."""
    _fields_ = [("pik", C.POINTER(C.c_double)), ("pik1", C.POINTER(C.c_double)), ("present", C.POINTER(C.c_int32)),
                ("bend_off", C.POINTER(C.c_int32)), ("bend_xy", C.POINTER(C.c_double)),
                ("bend_off_prev", C.POINTER(C.c_int32)), ("bend_xy_prev", C.POINTER(C.c_double))]


# nep_ent_track_step / nep_batch_track_ent flags (include/neptune_entangle.h)
NEP_ENT_TRACK_ENTANGLED, NEP_ENT_TRACK_TWO_CASES, NEP_ENT_TRACK_TOO_LONG, NEP_ENT_TRACK_CAP, NEP_ENT_TRACK_ABORT = 1, 2, 4, 8, 16
NEP_ENT_TRACK_ADD_CAP = 32
NEP_ENT_TRACK_HELD = 32      # (a flag of the device's list form: the state at A does not fit the fixed record)


class nep_fe_cfg(C.Structure):
    """include/neptune_frontend.h: the KinodynamicSearch setters the batched front end needs."""
    _fields_ = [("j_max", C.c_double), ("voxel_size", C.c_double), ("bias", C.c_double), ("goal_size", C.c_double),
                ("cable_length", C.c_double), ("num_samples", C.c_int32), ("beam_width", C.c_int32),
                ("pad_hold", C.c_int32), ("enable_entangle", C.c_int32), ("ent_samples", C.c_int32), ("_pad", C.c_int32)]


NEP_FE_ENT_CAP = 40
NEP_FE_ASTAR_TEAMS = (1, 4)      # nep_batch_set_fe_astar_team: waves per search of nep_batch_frontend_astar_ent (anything else NEP_E_ARG)


class nep_fe_ent_state(C.Structure):
    """eu::ent_state of a search node / of point A in a fixed-size record (include/neptune_frontend.h)."""
    _fields_ = [("n_alpha", C.c_int32), ("n_bend", C.c_int32), ("id", C.c_int16 * NEP_FE_ENT_CAP), ("cs", C.c_int8 * NEP_FE_ENT_CAP),
                ("beta", C.c_double * NEP_FE_ENT_CAP), ("bend", C.c_int8 * 8)]


NEP_ENT_LISTS_MAX_CAP = 4096


class nep_ent_lists(C.Structure):
    """the tracked tether states as a struct of arrays, `cap` entries per slot (include/neptune_frontend.h)"""
    _fields_ = [("cap", C.c_int32), ("_pad", C.c_int32), ("n_alpha", C.POINTER(C.c_int32)), ("n_bend", C.POINTER(C.c_int32)),
                ("id", C.POINTER(C.c_int16)), ("cs", C.POINTER(C.c_int8)), ("beta", C.POINTER(C.c_double)), ("bend", C.POINTER(C.c_int16))]


ENT_LISTS_FIELDS = (("n_alpha", np.int32, 0), ("n_bend", np.int32, 0), ("id", np.int16, 1), ("cs", np.int8, 1), ("beta", np.float64, 1),
                    ("bend", np.int16, 2))      # (name, dtype, per slot: 0 = one, 1 = cap, 2 = NEP_MAX_BEND)


class EntLists:
    """nep_ent_lists in host arrays: n_alpha / n_bend [slots], id / cs / beta [slots][cap], bend [slots][NEP_MAX_BEND]; .c is the struct"""

    def __init__(self, slots, cap):
        self.slots, self.cap = int(slots), int(cap)
        for name, dt, kind in ENT_LISTS_FIELDS:
            setattr(self, name, np.zeros((self.slots,) + ((), (self.cap,), (NEP_MAX_BEND,))[kind], dtype=dt))
        self.c = nep_ent_lists(self.cap, 0, *[C.cast(getattr(self, name).ctypes.data, t) for (name, _, _), (_, t) in
                                               zip(ENT_LISTS_FIELDS, nep_ent_lists._fields_[2:])])

    def set_state(self, slot, st):
        """slot <- a host eu::ent_state (entangle.State)"""
        al, be_, bi, _ = st.as_lists()
        assert len(al) <= self.cap and len(bi) <= NEP_MAX_BEND
        for name, _, _ in ENT_LISTS_FIELDS[2:]:
            getattr(self, name)[slot] = 0
        self.n_alpha[slot], self.n_bend[slot] = len(al), len(bi)
        if al:
            self.id[slot, :len(al)] = [a[0] for a in al]; self.cs[slot, :len(al)] = [a[1] for a in al]; self.beta[slot, :len(al)] = be_
        self.bend[slot, :len(bi)] = bi

    def tobytes(self):
        return b"".join(getattr(self, name).tobytes() for name, _, _ in ENT_LISTS_FIELDS)


class nep_fe_start(C.Structure):
    _fields_ = [("pos", C.c_double * 3), ("vel", C.c_double * 3), ("accel", C.c_double * 3), ("goal", C.c_double * 3),
                ("t_start", C.c_double)]


class nep_fe_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("K", C.c_int32), ("depth", C.c_int32), ("n_children", C.c_int32),
                ("n_feasible", C.c_int32), ("n_collision_free", C.c_int32), ("goal_occupied", C.c_int32), ("_pad", C.c_int32),
                ("cost", C.c_double), ("dist_to_goal", C.c_double), ("n_entangled", C.c_int32), ("ent_overflow", C.c_int32)]


class nep_audit(C.Structure):
    """include/neptune_frontend.h: the flight audit of one (scene, agent); calls accumulate into it."""
    _fields_ = [("min_center_dist", C.c_double), ("t_center", C.c_double), ("min_box_clear", C.c_double), ("t_box", C.c_double),
                ("min_static_dist", C.c_double), ("t_static", C.c_double), ("path_len", C.c_double), ("max_speed", C.c_double),
                ("center_d2", C.c_double), ("last_xy", C.c_double * 2),
                ("center_partner", C.c_int32), ("box_partner", C.c_int32), ("static_index", C.c_int32),
                ("n_ticks", C.c_int32), ("n_pair_viol", C.c_int32), ("n_static_viol", C.c_int32)]


class nep_span_audit(C.Structure):
    """include/neptune_frontend.h: the span audit of one (scene, agent): the flight audit's minima over whole windows; calls accumulate."""
    _fields_ = [("min_center_dist", C.c_double), ("t_center", C.c_double), ("min_box_clear", C.c_double), ("t_box", C.c_double),
                ("min_static_dist", C.c_double), ("t_static", C.c_double), ("center_d2", C.c_double), ("span", C.c_double),
                ("gap_box", C.c_double), ("gap_static", C.c_double),
                ("center_partner", C.c_int32), ("box_partner", C.c_int32), ("static_index", C.c_int32),
                ("n_spans", C.c_int32), ("n_pair_viol", C.c_int32), ("n_static_viol", C.c_int32)]


class nep_tether_audit(C.Structure):
    """include/neptune_entangle.h: the tether audit of one (scene, agent); the tracking calls accumulate one tick per move into it."""
    _fields_ = [("max_len", C.c_double), ("t_max_len", C.c_double), ("sum_len", C.c_double), ("last_len", C.c_double),
                ("t_first_too_long", C.c_double), ("t_first_entangled", C.c_double), ("t_max_wind", C.c_double),
                ("tick_max_len", C.c_int32), ("n_ticks", C.c_int32), ("n_too_long", C.c_int32), ("n_entangled", C.c_int32),
                ("n_two_cases", C.c_int32), ("n_abort", C.c_int32), ("n_dropped", C.c_int32), ("tick_first_too_long", C.c_int32),
                ("tick_first_entangled", C.c_int32), ("entangled_partner", C.c_int32), ("max_alpha", C.c_int32), ("max_bend", C.c_int32),
                ("max_wind", C.c_int32), ("wind_partner", C.c_int32), ("tick_max_wind", C.c_int32), ("crossings_added", C.c_int32)]


class nep_fleet_cfg(C.Structure):
    """include/neptune_fleet.h: nep_plan_cfg's fields plus what a bulk-synchronous round needs (nep_batch_fleet_init)."""
    _fields_ = [("dc", C.c_double), ("T_span", C.c_double), ("lower_bound_runtime", C.c_double),
                ("upper_bound_runtime", C.c_double), ("runtime_opt", C.c_double), ("factor_alpha", C.c_double),
                ("deltaT0", C.c_int32), ("k_a", C.c_int32), ("round_ticks", C.c_int32), ("ring_cap", C.c_int32),
                ("goal_radius", C.c_double), ("t0", C.c_double)]


# nep_batch_fleet_commit's outcomes, the per-scene counters' order (include/neptune_fleet.h)
NEP_FLEET_SKIPPED, NEP_FLEET_FE_NO_SOLUTION, NEP_FLEET_QP_FAILED, NEP_FLEET_REJECTED, NEP_FLEET_ACCEPTED, NEP_FLEET_CAP = range(6)
NEP_FLEET_N_COUNTERS = 8
FLEET_OUTCOMES = ("skipped", "fe_no_solution", "qp_failed", "rejected_by_safety", "accepted", "cap")
NEP_FLEET_FLAG_SEG, NEP_FLEET_FLAG_RING, NEP_FLEET_FLAG_SPLICE = 1, 2, 4
NEP_FLEET_FLAG_GOAL = 8
NEP_FLEET_FLAG_WAY_BACK = 16      # not sticky, no error: the slot is on its way back to its base (nep_batch_fleet_moveback)
NEP_FLEET_FLAG_ERRORS = NEP_FLEET_FLAG_SEG | NEP_FLEET_FLAG_RING | NEP_FLEET_FLAG_SPLICE | NEP_FLEET_FLAG_GOAL      # the sticky bits: something overflowed


# ---- missions (include/neptune_fleet.h) ----
NEP_MISSION_PER_AGENT, NEP_MISSION_FLEET_RUNS, NEP_MISSION_FLEET_TOGETHER = 1, 2, 3
NEP_MISSION_REACHED, NEP_MISSION_TIMED_OUT, NEP_MISSION_NO_GOAL = 1, 2, 3
NEP_MISSION_MAX_POLY, NEP_MISSION_MAX_VERT = 64, 512
MISSION_COUNTS = ("issued", "reached", "timed_out", "no_goal")


class nep_mission_cfg(C.Structure):
    """include/neptune_fleet.h: the mission controller's configuration (nep_batch_fleet_mission_init, nep_mission_step)."""
    _fields_ = [("mode", C.c_int32), ("max_goals", C.c_int32), ("max_attempts", C.c_int32), ("log_cap", C.c_int32),
                ("seed", C.c_uint64), ("lo", C.c_double * 2), ("hi", C.c_double * 2),
                ("goal_z", C.c_double), ("arrive_radius", C.c_double), ("min_interval", C.c_double), ("timeout", C.c_double),
                ("rest_v", C.c_double), ("rest_a", C.c_double),
                ("min_dist_self", C.c_double), ("tether_max", C.c_double), ("close_pos", C.c_double), ("close_goal", C.c_double)]


class nep_mission_leg(C.Structure):
    """include/neptune_fleet.h: one record of the mission log (a leg of a slot, or a run of a scene)."""
    _fields_ = [("who", C.c_int32), ("index", C.c_int32), ("outcome", C.c_int32), ("attempts", C.c_int32),
                ("t_issue", C.c_double), ("t_end", C.c_double), ("length", C.c_double), ("goal", C.c_double * 3)]


class nep_mission_scene(C.Structure):
    """include/neptune_fleet.h: one scene's mission state and inputs in host memory (nep_mission_step)."""
    _fields_ = [("n_agents", C.c_int32), ("scene", C.c_int32), ("round_ticks", C.c_int32), ("n_poly", C.c_int32),
                ("t_now", C.c_double), ("dc", C.c_double),
                ("pos", C.c_void_p), ("s_end", C.c_void_p), ("pb", C.c_void_p), ("poly_off", C.c_void_p), ("poly_xy", C.c_void_p),
                ("goal", C.c_void_p), ("done", C.c_void_p), ("flags", C.c_void_p), ("t_issue", C.c_void_p), ("length", C.c_void_p),
                ("completed", C.c_void_p), ("counts", C.c_void_p), ("sums", C.c_void_p), ("scene_i", C.c_void_p), ("t_run", C.c_void_p),
                ("log", C.c_void_p), ("log_n", C.c_void_p)]


class nep_moveback_cfg(C.Structure):
    """include/neptune_fleet.h: the move-back rule's two parameters (nep_batch_fleet_moveback, nep_moveback_step)."""
    _fields_ = [("radius", C.c_double), ("timeout", C.c_double)]


class nep_fleet_effort(C.Structure):
    """include/neptune_fleet.h: a slot's effort record (nep_batch_fleet_effort, nep_effort_step)."""
    _fields_ = [("jerk_sum", C.c_double), ("max_v", C.c_double * 3), ("max_a", C.c_double * 3), ("max_j", C.c_double * 3),
                ("n_ticks", C.c_int32), ("n_v_viol", C.c_int32), ("n_a_viol", C.c_int32), ("n_j_viol", C.c_int32)]


# ---- the recorder (include/neptune_fleet.h) ----
NEP_SNAPSHOT_MAGIC, NEP_SNAPSHOT_VERSION, NEP_SNAPSHOT_HDR_BYTES, NEP_SNAPSHOT_N_SECTIONS = 0x5046454e, 1, 80, 41
SNAPSHOT_SECTIONS = ("origin", "round", "ring", "head", "size", "k_end", "state", "goal", "pwp", "flown", "done", "outcome", "sflags", "period", "phase",
                     "t_now", "counters", "ent", "l_n_alpha", "l_n_bend", "l_id", "l_cs", "l_beta", "l_bend", "held", "pub_n", "pub_xy", "pub_prev_n",
                     "pub_prev_xy", "ent_flags", "ent_ever", "ent_walked", "t_issue", "length", "completed", "counts", "sums", "scene_i", "t_run", "log", "log_n")


class nep_fleet_snapshot_hdr(C.Structure):
    """include/neptune_fleet.h: what a fleet snapshot starts with."""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_int32), ("hdr_bytes", C.c_int32), ("n_scenes", C.c_int32), ("N", C.c_int32),
                ("num_pol", C.c_int32), ("ring_cap", C.c_int32), ("max_states", C.c_int32), ("tether_form", C.c_int32), ("tether_cap", C.c_int32),
                ("mission_mode", C.c_int32), ("log_cap", C.c_int32), ("timers", C.c_int32), ("_pad", C.c_int32 * 3),
                ("scene_bytes", C.c_int64), ("cfg_hash", C.c_uint64)]


class nep_fleet_snapshot_info(C.Structure):
    """include/neptune_fleet.h: nep_fleet_snapshot_describe's answer — the header, and every section's offset in a block and size."""
    _fields_ = [("hdr", nep_fleet_snapshot_hdr), ("offset", C.c_int64 * NEP_SNAPSHOT_N_SECTIONS), ("bytes", C.c_int64 * NEP_SNAPSHOT_N_SECTIONS)]


NEP_HASTAR_FLAG_HSIG, NEP_HASTAR_FLAG_CONT, NEP_HASTAR_FLAG_PATH, NEP_HASTAR_FLAG_POOL, NEP_HASTAR_FLAG_STATE = 1, 2, 4, 8, 16
NEP_HASTAR_MAX_REP = 256
NEP_HASTAR_POOL_PER_NODE = 8


class nep_hastar_cfg(C.Structure):
    """include/neptune_hastar.h: the homotopic grid A* of the single-agent benchmark (AstarPathFinder::init and this build's caps)."""
    _fields_ = [("resolution", C.c_double), ("x_min", C.c_double), ("x_max", C.c_double), ("y_min", C.c_double), ("y_max", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("cable_length", C.c_double), ("bias", C.c_double),
                ("max_pops", C.c_int32), ("max_nodes", C.c_int32), ("hsig_cap", C.c_int32), ("cont_cap", C.c_int32), ("path_cap", C.c_int32)]


class nep_hastar_result(C.Structure):
    """include/neptune_hastar.h: one search's outcome and counters."""
    _fields_ = [("status", C.c_int32), ("n_path", C.c_int32), ("nodes_used", C.c_int32), ("pops", C.c_int32), ("n_updates", C.c_int32),
                ("n_length_checks", C.c_int32), ("n_cable_pruned", C.c_int32), ("flags", C.c_int32),
                ("g_cells", C.c_double), ("length_m", C.c_double)]


class nep_hastar_state(C.Structure):
    """include/neptune_hastar.h: eu::ent_state_orig of many searches as a struct of arrays (host struct, host or device arrays)."""
    _fields_ = [("hsig_cap", C.c_int32), ("cont_cap", C.c_int32), ("n_hsig", C.c_void_p), ("hsig_id", C.c_void_p), ("hsig_sign", C.c_void_p),
                ("n_cont", C.c_void_p), ("cont", C.c_void_p)]


HASTAR_RESULT_DTYPE = np.dtype(nep_hastar_result)

NEP_MTLP_FLAG_PATH, NEP_MTLP_FLAG_STATE, NEP_MTLP_FLAG_DEGEN = 1, 2, 4
NEP_MTLP_MAX_ROBOTS = 64


class nep_mtlp_cfg(C.Structure):
    """include/neptune_mtlp.h: the MTLP comparator's set-up (mtlp::mtlp and this build's budgets)."""
    _fields_ = [("resolution", C.c_double), ("x_min", C.c_double), ("x_max", C.c_double), ("y_min", C.c_double), ("y_max", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("radius", C.c_double), ("bias", C.c_double),
                ("n_robots", C.c_int32), ("max_nodes", C.c_int32), ("max_pops", C.c_int32), ("path_cap", C.c_int32)]


class nep_mtlp_result(C.Structure):
    """include/neptune_mtlp.h: one robot's search: outcome and counters."""
    _fields_ = [("status", C.c_int32), ("n_path", C.c_int32), ("nodes_used", C.c_int32), ("pops", C.c_int32), ("n_updates", C.c_int32),
                ("flags", C.c_int32), ("n_degenerate", C.c_int64), ("n_ball_only", C.c_int64), ("g_cells", C.c_double)]


MTLP_RESULT_DTYPE = np.dtype(nep_mtlp_result)
SNAPSHOT_STAMP_DTYPE = np.dtype([("used", np.int32), ("round", np.int32), ("origin", np.int32), ("_pad", np.int32)])


def np_dtype(struct):
    return np.dtype(struct)


TRAJ_REC_DTYPE = np.dtype(nep_traj_rec)
GUESS_DTYPE = np.dtype(nep_guess)
SOLUTION_DTYPE = np.dtype(nep_solution)
FE_START_DTYPE = np.dtype(nep_fe_start)
FE_RESULT_DTYPE = np.dtype(nep_fe_result)
FE_ENT_STATE_DTYPE = np.dtype(nep_fe_ent_state)
AUDIT_DTYPE = np.dtype(nep_audit)
TETHER_AUDIT_DTYPE = np.dtype(nep_tether_audit)
SPAN_AUDIT_DTYPE = np.dtype(nep_span_audit)
PWP_DTYPE = np.dtype(nep_pwp)
MISSION_LEG_DTYPE = np.dtype(nep_mission_leg)
EFFORT_DTYPE = np.dtype(nep_fleet_effort)


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))
