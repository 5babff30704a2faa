/* neptune_fleet.h — the committed plan of every agent of every scene on the device (SURVEY §8 f, rank 3, device form).
 *
 * include/neptune_plan.h keeps the plan deque, point A, the splice and the trajectory composition of Neptune::replanFull
 * (neptune.cpp:860-891, 1366-1425, 1661-1687) in host memory, one agent per handle: a closed loop built on it makes a host round
 * trip per agent and round.  Here the same state lives in the batched handle (include/neptune_backend.h: nep_batch_t), per
 * (scene, agent) slot, and three asynchronous calls move it — so a faithful round
 *
 *   nep_batch_fleet_select [-> nep_batch_fleet_moveback] -> nep_batch_frontend [-> nep_batch_goal_gate] -> nep_batch_replan
 *     [-> nep_batch_guess_fallback] -> nep_batch_safety_commit -> nep_batch_fleet_commit [-> nep_batch_guess_fallback_tally]
 *     [-> nep_batch_audit] [-> nep_batch_fleet_mission] [-> nep_batch_fleet_effort] -> nep_batch_fleet_tick
 *
 * is a fixed launch sequence on fixed buffers: one HIP graph for all scenes, no host synchronisation in it.  The arithmetic is the
 * host library's own (neptune_amd/csrc/plan_common.h is compiled into both), so the plans, tracked states and trajectories on the
 * device equal, bit for bit, what nep_plan_select_a / nep_plan_splice / nep_plan_next_goal / nep_pwp_compose_exact leave when they
 * are driven with the same solver outputs.
 *
 * State of a slot (owned by the handle, allocated by nep_batch_fleet_init):
 *   plan ring        [ring_cap][12] doubles with head and size: mt::committedTrajectory plan_.  ring_cap = deltaT0 + max_states
 *                    holds the longest plan a splice can leave (at most deltaT - 1 states stay in front of A, n_states are appended)
 *   last selection   k_index_end of the last nep_batch_fleet_select (what the splice erases)
 *   tracked state    12 doubles: the goal the perfect tracker took last (Neptune::getNextGoal)
 *   trajectory       the composed committed trajectory (pwp_prev_) and whether the agent has committed one yet
 *   bookkeeping      sticky `done` (arrived; a mission's new goal clears it), the last round's outcome, the NEP_FLEET_FLAG_* bits
 *                    (sticky, but for NEP_FLEET_FLAG_WAY_BACK)
 * State of a scene: the clock t_now, a round counter, and counters of every outcome.
 *
 * What differs from the reference:
 *   deltaT_          is the saturate of deltaT0 into [lower_bound_runtime/dc, upper_bound_runtime/dc] (ints, as mu::saturate
 *                    truncates them) at every selection.  There is NO nep_plan_update_delta on the device: it feeds the wall-clock
 *                    duration of the last replan back, and a simulated bulk-synchronous loop has no wall clock.  Pin deltaT with
 *                    lower_bound_runtime == upper_bound_runtime, as neptune_amd.loop.FleetLoop does.
 *   composition      nep_pwp_compose_exact, not mu::composePieceWisePol (nep_pwp_compose): what the others must avoid is the path
 *                    actually flown, and the reference routine describes the stretch up to point A with the wrong interval
 *                    (include/neptune_plan.h).
 *   timers           the reference replans every agent on its own ROS timer; here a round is bulk-synchronous and an agent's timer
 *                    is a period and a phase in rounds (see nep_batch_fleet_select's mask).
 * Unsharded handles only (n_local == num_agents), else NEP_E_STATE.  Without a HIP device every call returns NEP_E_HIP.
 *
 * Tethered fleets (nep_batch_fleet_init_ent, on a handle created with enable_entangle).  The handle then also owns, per slot, the
 * entangle state of the tether at the TRACKED position (NeptuneRos's entangle_state_), the bend list the agent published at the
 * last selection and the one before it (bendPtsForAgents_ / bendPtsForAgents_prev_ as the others see them: a count and
 * NEP_MAX_BEND points each), the NEP_ENT_TRACK_* flags of the last tracked round and their sticky OR; per scene, counter [7] =
 * slots ever flagged NEP_ENT_TRACK_ENTANGLED.  The round becomes
 *
 *   nep_batch_fleet_select [-> nep_batch_fleet_moveback] -> nep_batch_fleet_predict_ent -> nep_batch_frontend_ent ->
 *     nep_batch_replan (entangle rows) -> nep_batch_safety_commit_ent -> nep_batch_fleet_commit [-> nep_batch_audit] ->
 *     nep_batch_fleet_track_ent -> nep_batch_fleet_tick
 *
 * with the state at A (Neptune::PredictAlphasBetas, neptune.cpp:976-1008) made on the device and the state at the tracked
 * position moved once per control tick flown (NeptuneRos::odomCB -> updateEntStateStaticObs, neptune_ros.cpp:781-850).  Both equal,
 * bit for bit, the host chain of nep_ent_predict_a / nep_ent_track_step (include/neptune_entangle.h).  What differs from the
 * reference: every agent's bend list changes at the round's select and nowhere else (one trajCB per agent and round), so the
 * nine-argument crossing test can only run at a round's first tick.                                                          */
#ifndef NEPTUNE_FLEET_H_
#define NEPTUNE_FLEET_H_

#include <stdint.h>

#include "neptune_frontend.h"
#include "neptune_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* outcome of a slot's round (nep_batch_fleet_commit), in the order the rules are tried */
#define NEP_FLEET_SKIPPED 0             /* outside the active set, or arrived: the agent keeps its plan                      */
#define NEP_FLEET_FE_NO_SOLUTION 1      /* nep_fe_result.status == NEP_FE_NO_SOLUTION or the solution's K == 0              */
#define NEP_FLEET_QP_FAILED 2           /* nep_stats.status == NEP_FAILED (after nep_batch_guess_fallback, include/neptune_backend.h,
                                           a failed replan with a usable guess is NEP_GUESS and goes by d_accept like a solved one) */
#define NEP_FLEET_REJECTED 3            /* turned down by nep_batch_safety_commit                                           */
#define NEP_FLEET_ACCEPTED 4            /* plan spliced, trajectory composed                                                 */
#define NEP_FLEET_CAP 5                 /* accepted, but the plan or the trajectory would outgrow its storage: nothing changed */
#define NEP_FLEET_N_COUNTERS 8          /* per scene: one per outcome above, [6] accepted solves with NEP_RELAXED, [7] slots ever entangled (tethered fleets, else 0) */

#define NEP_FLEET_FLAG_SEG 1            /* sticky per slot: a composition needed more than NEP_TRAJ_MAX_SEG intervals        */
#define NEP_FLEET_FLAG_RING 2           /* a splice needed more than ring_cap states (or n_states > max_states)              */
#define NEP_FLEET_FLAG_SPLICE 4         /* a splice with size - 1 - k_index_end < 0 ("Already published the point A")        */
/* (8: NEP_FLEET_FLAG_GOAL, with the missions.)  Bits 1, 2, 4, 8 are sticky and say that something overflowed.  Bit 16 is neither: */
#define NEP_FLEET_FLAG_WAY_BACK 16      /* NOT sticky, no error: the slot is on its way back to its base (nep_batch_fleet_moveback) */

/* nep_abi_sizeof(18).  The first eight fields are nep_plan_cfg's (runtime_opt and factor_alpha are carried for symmetry: the
 * front end's run-time budget and nep_plan_update_delta have no device form).                                               */
typedef struct nep_fleet_cfg {
  double dc, T_span, lower_bound_runtime, upper_bound_runtime, runtime_opt, factor_alpha;
  int32_t deltaT0;                /* initial deltaT_, saturated at every selection                                           */
  int32_t k_a;                    /* the round's clock: every slot's t_start = t_now + (k_a + 1)*dc (plan[k] is k + 1 control
                                     ticks ahead of the tracked state; FleetLoop: deltaT0 - 1)                              */
  int32_t round_ticks;            /* control periods nep_batch_fleet_tick flies (the replan timer / dc), >= 1               */
  int32_t ring_cap;               /* 0: deltaT0 + max_states.  > 0: that many states — a smaller ring than a splice can need
                                     exercises the NEP_FLEET_CAP path; nothing is ever written past it                       */
  double goal_radius;             /* arrival: within it of the goal in x-y and slower than 0.05 m/s                         */
  double t0;                      /* every scene's clock at the start                                                        */
} nep_fleet_cfg;

/* Allocates (first call) or re-seeds the fleet state: every plan holds the one state d_state0[slot] (nep_plan_reset), which is
 * also the tracked state; nobody has flown or arrived; clocks t0, round counters and outcome counters 0.  d_state0 [slots][12],
 * d_goal [slots][3] doubles, d_period / d_phase [slots] int32 in device memory (both NULL: every agent replans every round; a
 * period < 1 counts as 1); all four are copied.  Synchronises; not capturable.  Returns NEP_E_ARG on a bad configuration.     */
int nep_batch_fleet_init(nep_batch_t* h, const nep_fleet_cfg* cfg, const double* d_state0, const double* d_goal,
                         const int32_t* d_period, const int32_t* d_phase, void* stream);

/* First half of a round, one thread per slot.  Point A by nep_plan_select_a's rule from the slot's plan and tracked position ->
 * d_start[slot] (pos / vel / accel of A, the slot's goal, t_start = t_now + (k_a + 1)*dc — ONE clock per scene, written to
 * every slot: an inactive slot's t_start is read for the hull grid).  The record the agent publishes -> d_records[slot]: id =
 * agent + 1, is_agent, valid, n_bend = 1, bbox = 2*drone_radius, pos = the tracked position, bend[0] = the agent's base, and as
 * pwp the composed trajectory, or — until the agent first commits — a one-interval hover [t_now, t_now + 1000] on the tracked
 * position; every other byte 0.
 * d_active ([n_scenes][num_agents] int32, may be NULL): the round's mask, !done && (round - phase) mod period == 0 — the buffer
 * the caller handed to nep_batch_set_active, so that the front end, the replan and the safety pass of the same graph skip the
 * others.  d_clock ([slots] nep_fe_start, may be NULL): t_start = t_now + dc in every entry, the clock of a nep_batch_audit of
 * d_records over the round_ticks ticks about to be flown (they lie before A, so the records published now describe them).
 * On a handle with tether state (nep_batch_fleet_init_ent) the record publishes the bend points of the state at the tracked
 * position (publishOwnTraj, neptune_ros.cpp:457-476: entangle_state_, not the state at A): n_bend = 1 + state.n_bend, bend[0] the
 * base, then the anchor of every bend index — an agent's base, or the static representative's column — and the list published at
 * the previous select becomes the "previous" one first.  Without tether state every byte is as described above.
 * Asynchronous on `stream`, capturable.                                                                                      */
int nep_batch_fleet_select(nep_batch_t* h, nep_fe_start* d_start, nep_traj_rec* d_records, int32_t* d_active,
                           nep_fe_start* d_clock, void* stream);

/* Second half, one wave per slot.  The outcome (NEP_FLEET_*) of every slot from the round's results — d_solution, d_states
 * ([slots][max_states][12]) of nep_batch_replan, d_fe_result of nep_batch_frontend, d_accept of nep_batch_safety_commit; "outside
 * the active set" is the handle's mask (nep_batch_set_active) as it stands when the kernel runs.  An accepted slot erases A and
 * what follows from its plan and appends d_states[slot][:n_states] (nep_plan_splice), and its trajectory becomes the solution's
 * (times[:K + 1], coeff[:, :K]) the first time, nep_pwp_compose_exact(t_now, previous, new) afterwards.  A slot whose plan or
 * trajectory would not fit changes nothing, comes out NEP_FLEET_CAP, raises its sticky flag and makes nep_batch_check return
 * NEP_E_CAP.  d_outcome ([slots], may be NULL) receives the outcomes; the scene's counters accumulate them (a second small launch,
 * no atomics).  Asynchronous, capturable.                                                                                    */
int nep_batch_fleet_commit(nep_batch_t* h, const nep_solution* d_solution, const double* d_states, const nep_fe_result* d_fe_result,
                           const int32_t* d_accept, int32_t* d_outcome, void* stream);

/* Flies round_ticks control periods, one thread per slot: per period the tracked state becomes the front of the plan, popped when
 * more than one state is left (nep_plan_next_goal), and the scene's clock does t += dc (repeated additions, as a host loop does).
 * Then the sticky arrival test — sqrt(dx*dx + dy*dy) < goal_radius && sqrt(vx*vx + vy*vy) < 0.05 on the tracked state, the
 * expression of nep_batch_next_starts — and the round counter's increment.  Asynchronous, capturable.                         */
int nep_batch_fleet_tick(nep_batch_t* h, void* stream);

/* ---- tethers ---------------------------------------------------------------------------------------------------------------- */
/* Allocates (first call) or re-seeds the tether state: every slot's state d_ent0[slot] (device memory; NULL: empty), nothing
 * published yet, flags and counts 0.  After nep_batch_fleet_init (which drops the tether state: call this again after a re-seed)
 * and, with static obstacles, nep_batch_set_static_reps; on a handle created with enable_entangle.  Otherwise NEP_E_STATE.
 * Up to 4096 agents and 2048 statics per scene (NEP_E_CAP).  Synchronises; not capturable.                                   */
int nep_batch_fleet_init_ent(nep_batch_t* h, double cable_length, const nep_fe_ent_state* d_ent0, void* stream);

/* After the select: d_ent_a[slot] = nep_ent_predict_a of the slot's state with pk = the tracked position, pk1 = d_start[slot].pos,
 * and of every other agent i pik = its tracked position, pik1 = its record in d_records at the slot's t_start (the first sample of
 * nep_ent_sample_points: the front end's sampled[i][0][0]) and its bend list in d_records; present = the record is valid, an
 * agent's, and has a trajectory.  The handle's state is not touched.  d_flags_a ([slots], may be NULL): the NEP_ENT_TRACK_* bits;
 * a CAP leaves d_ent_a[slot] = the state as it is and raises NEP_FLAG_ENT_TRACK (nep_batch_check).  d_ent_a is the d_ent_init of
 * nep_batch_frontend_ent and nep_batch_safety_commit_ent.  Asynchronous, capturable.                                          */
int nep_batch_fleet_predict_ent(nep_batch_t* h, const nep_fe_start* d_start, const nep_traj_rec* d_records, nep_fe_ent_state* d_ent_a,
                                int32_t* d_flags_a, void* stream);

/* Between nep_batch_fleet_commit and nep_batch_fleet_tick: for the ticks q = 1..round_ticks about to be flown, every slot's state
 * takes one nep_ent_track_step.  A slot stands, after tick q, at ring[(head + min(q - 1, size - 1)) mod cap][0:2] and before tick 1
 * at the tracked state (nep_batch_fleet_tick's pop rule: a plan down to one state stays put); the rings are read as the commit left
 * them.  The others' bend lists are d_records' (published this round); at the first tick only, the list an agent published a round
 * ago counts as the previous check's (an empty one: as the current one).  Every slot is tracked — active or not, arrived or not.
 * The flags are ORed over the ticks into d_flags ([slots], may be NULL) and into the sticky word; a CAP (that tick's move is
 * dropped) raises NEP_FLAG_ENT_TRACK.  Asynchronous, capturable.
 * With a buffer registered by nep_batch_set_tether_audit (include/neptune_frontend.h) every tick is also one tick of the slot's
 * nep_tether_audit (include/neptune_entangle.h) — taut length, windings, list and bend counts, flag and drop counts — at
 * t_now + q * dc, t_now the scene's clock as nep_batch_fleet_counters reports it before the round's nep_batch_fleet_tick; states,
 * flags and records are those of the call without it.  nep_batch_fleet_predict_ent never audits: it flies nothing.           */
int nep_batch_fleet_track_ent(nep_batch_t* h, const nep_traj_rec* d_records, int32_t* d_flags, void* stream);

/* Blocking reader (host memory, each may be NULL): the states at the tracked positions, the last tracked round's flags, the sticky
 * flags, and per slot the (other agent, tick) pairs the tracking has actually walked since nep_batch_fleet_init_ent — the rest was
 * proven to add no crossing (nep_batch_debug_set_option "fleet_ent_proof" 0: everything is walked; same states).               */
int nep_batch_fleet_ent_state(nep_batch_t* h, nep_fe_ent_state* states_out, int32_t* flags_round_out, int32_t* flags_ever_out,
                              int32_t* walked_out);

/* ---- tethers beyond NEP_FE_ENT_CAP crossings: the list form (nep_ent_lists, include/neptune_frontend.h) ------------------------
 * nep_batch_fleet_init_ent_lists   like nep_batch_fleet_init_ent, but the states come from HOST arrays in the list form (all arrays
 *                         NULL: empty states) and host_lists->cap (NEP_FE_ENT_CAP < cap <= NEP_ENT_LISTS_MAX_CAP, else NEP_E_CAP) is
 *                         the handle's capacity from then on: nep_batch_fleet_track_ent, the bend points nep_batch_fleet_select
 *                         publishes and nep_batch_fleet_predict_ent run on lists of that many entries, bit-identical to the host
 *                         chain with state->cap = cap.  nep_batch_fleet_init_ent puts the handle back on the fixed record.
 *                         Synchronises; not capturable.
 * Point A: the front end and the safety re-check take the fixed record.  nep_batch_fleet_predict_ent on such a handle predicts in
 * the list form; where the result holds at most NEP_FE_ENT_CAP crossings d_ent_a[slot] receives it as before.  Where it holds
 * more the slot is HELD for the round: d_ent_a[slot] is zeroed, d_flags_a[slot] gets NEP_ENT_TRACK_HELD, the slot's held rounds
 * count up, and its entry in the mask registered with nep_batch_set_active is cleared — it takes the inactive-slot path
 * (NEP_FE_SKIPPED, NEP_SKIPPED, record kept, NEP_FLEET_SKIPPED), keeps flying its plan, its tether keeps being tracked exactly,
 * and it plans again in the first round whose state at A fits.  The caller refills (or nep_batch_fleet_select rewrites) the mask
 * before the next prediction; no registered mask is NEP_E_STATE.  A hold is no capacity: nep_batch_check reports nothing.
 * nep_batch_fleet_ent_lists   blocking reader: host_out's arrays (host_out->cap == the handle's, else NEP_E_ARG; may be NULL) and
 *                         held_rounds_out ([slots], may be NULL).  NEP_E_STATE on a handle that is not on the list form.
 * nep_batch_fleet_ent_state on such a handle fills states_out for the slots that fit a fixed record; a slot that does not gets
 * n_alpha = -1 and zeros.
 * The tether audit (nep_batch_set_tether_audit) runs on the list form as on the fixed record: nep_batch_fleet_track_ent folds every
 * tick into the registered buffer, and max_alpha is the headroom against the handle's capacity.                                  */
int nep_batch_fleet_init_ent_lists(nep_batch_t* h, double cable_length, const nep_ent_lists* host_lists, void* stream);
int nep_batch_fleet_ent_lists(nep_batch_t* h, nep_ent_lists* host_out, int32_t* held_rounds_out);

/* ---- missions: successive goals, timeouts, leg records -------------------------------------------------------------------------
 * The two goal generators of the reference's experiments as a controller inside the round, so that a campaign of any length
 * needs no host round trip:
 *   NEP_MISSION_PER_AGENT    NeptuneRos::autoCMD (neptune_ros.cpp:1047-1102, yaml auto_cmd): every agent for itself.  Once
 *                            min_interval has passed since its goal was issued and the agent is at rest — (el < timeout && v_xy >
 *                            rest_v) || a_xy > rest_a holds it off, the reference's precedence — its leg ends when it is within
 *                            arrive_radius of the goal (reached) or older than timeout (timed out), and it gets a new goal.
 *   NEP_MISSION_FLEET_RUNS   scripts/benchmark_mtlp.py:167-281: the whole scene.  A run ends when every agent is `completed`
 *                            (within arrive_radius of its goal; the flag is re-evaluated at every tick, in both directions) —
 *                            a success — or after timeout — a failure; then every agent gets a new goal, in agent order.
 * The round becomes  fleet_select -> [fleet_moveback] -> ... fleet_commit -> [audit] -> [fleet_track_ent] -> nep_batch_fleet_mission
 * -> fleet_tick.
 *
 * The call looks at the round_ticks ticks about to be flown by nep_batch_fleet_track_ent's rule: p_0 the tracked state, p_q =
 * ring[(head + min(q - 1, size - 1)) mod cap], the end state s_end = the 12 doubles of p_round_ticks, the end clock t_end = t_now
 * after round_ticks times t += dc.  Per tick the slot's leg grows by |p_q - p_(q-1)| (3-D) while the agent is not arrived — mode
 * PER_AGENT: |p_q - goal| > arrive_radius (neptune_ros.cpp:620); mode FLEET_RUNS: `completed` is 0 before the step — and in mode
 * FLEET_RUNS completed = |p_q - goal| < arrive_radius afterwards.  The triggers are evaluated once per call on s_end and t_end.
 *
 * A leg that ends writes a record (nep_mission_leg) and its slot's totals.  max_goals is the number of legs per slot (runs per
 * scene) that may end: the leg that uses the quota up draws nothing — the slot keeps its last goal and its `done` — and a scene
 * is `finished` when every slot (mode FLEET_RUNS: the scene) has used its quota; the call does nothing on a finished scene.
 * Otherwise a new goal is drawn, goal and t_issue are set (mode FLEET_RUNS: t_run, and every slot's t_issue), the leg length
 * (and `completed`) zeroed, done[slot] cleared and `issued` incremented, so that issued == reached + timed_out + (1 while a leg
 * is open) at all times.  The next select publishes the new goal; fleet_tick tests arrival against it.
 *
 * Drawing.  Candidate k = 0, 1, 2, ... of (global slot, goal index = the slot's `issued`) is (x, y) = lo + (hi - lo) * u with
 * u = (bits >> 11) * 2^-53 and the splitmix64 finaliser
 *   sm(x):  z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
 *   h1 = sm(sm(seed ^ sm(global_slot)) + goal_index);   bits_x = sm(h1 + 2k);   bits_y = sm(h1 + 2k + 1)
 * (all in 64-bit unsigned arithmetic).  A candidate is accepted when (a parameter of 0 switches its test off)
 *   1. it is at least min_dist_self (x-y) from the agent's s_end position (neptune_ros.cpp:1074),
 *   2. at most tether_max (x-y) from the agent's base pb[a] (:1076; benchmark_mtlp.py:233),
 *   3. on or inside none of the scene's keep-out polygons (counter-clockwise convex: every edge cross product >= 0 is inside,
 *      boundary included, as cu::check_inside counts ON_BOUNDARY),
 *   4. |(x, y, goal_z) - pos_j| >= close_pos for every agent j of the scene (the own one included) at its s_end position,
 *   5. |new - new_j| >= close_goal for every j < a that received a goal in this same call.
 * The goal is the accepted candidate of lowest k < max_attempts.  Without one the slot keeps its goal (it is issued again:
 * t_issue reset, a new leg), its no_goal total and the sticky NEP_FLEET_FLAG_GOAL are raised, mode PER_AGENT logs a record with
 * outcome NEP_MISSION_NO_GOAL, and nep_batch_check returns NEP_E_CAP.
 *
 * What differs from the reference:
 *   randomness       the reference seeds from the wall clock (autoCMD) and numpy's global state (benchmark_mtlp): nothing
 *                    deterministic to match.  The rules are kept one for one; the draws come from the counter-based generator above.
 *   when it runs     autoCMD runs on its own timer, benchmark_mtlp on agent 0's odometry messages; here both are evaluated once per
 *                    round, on the state the round's last tick will leave.
 *   no gate          benchmark_mtlp waits for the MTLP comparator's acknowledgement before the next run; there is no comparator here.
 *   one rule set     both modes share the five tests (autoCMD has 1-3, benchmark_mtlp 2, 4, 5); a test is off at parameter 0.
 *   quota            max_goals ends a campaign (the reference's scripts are stopped from outside or after 100 runs).
 *   use_moveback_    is nep_batch_fleet_moveback, below.  The single-agent A* benchmark branch of replanCB: include/neptune_hastar.h.
 *   given goals      auto_commands_together.py's fixed lists are nep_batch_fleet_mission_script with mode
 *                    NEP_MISSION_FLEET_TOGETHER, and benchmark_multi_direct.py's mean jerk is nep_batch_fleet_effort, both below.
 * Limits: the kernel stages a scene's end positions, new goals and keep-outs in 64 KB of LDS, sized once at
 * nep_batch_fleet_mission_init for 52 B per agent and a full keep-out set (NEP_MISSION_MAX_POLY polygons, NEP_MISSION_MAX_VERT
 * vertices in all per scene), so that keep-outs uploaded later fit a round captured earlier: up to 1 097 agents; beyond: NEP_E_CAP. */
#define NEP_MISSION_PER_AGENT 1
#define NEP_MISSION_FLEET_RUNS 2
#define NEP_MISSION_FLEET_TOGETHER 3    /* scripts/auto_commands_together.py: see "scripted goals" below                      */
#define NEP_MISSION_REACHED 1           /* nep_mission_leg.outcome (mode FLEET_RUNS: the run succeeded)                      */
#define NEP_MISSION_TIMED_OUT 2         /* (mode FLEET_RUNS: the run failed)                                                 */
#define NEP_MISSION_NO_GOAL 3           /* no candidate of max_attempts passed: the slot keeps its goal                      */
#define NEP_FLEET_FLAG_GOAL 8           /* sticky per slot (nep_batch_fleet_state's flags): a draw found no goal             */
#define NEP_MISSION_MAX_POLY 64
#define NEP_MISSION_MAX_VERT 512

/* nep_abi_sizeof(20) */
typedef struct nep_mission_cfg {
  int32_t mode;                   /* NEP_MISSION_PER_AGENT, NEP_MISSION_FLEET_RUNS or NEP_MISSION_FLEET_TOGETHER             */
  int32_t max_goals;              /* legs per slot (runs per scene) that may end, >= 1                                       */
  int32_t max_attempts;           /* candidates per draw: a multiple of 64, 64 .. 4096                                       */
  int32_t log_cap;                /* records kept per slot (per scene in mode FLEET_RUNS), >= 0                              */
  uint64_t seed;
  double lo[2], hi[2];            /* the box goals are drawn in (the caller shrinks the world)                               */
  double goal_z, arrive_radius, min_interval, timeout, rest_v, rest_a;      /* (min_interval, rest_*: mode PER_AGENT only;
                                                                               timeout = +infinity: none)                   */
  double min_dist_self, tether_max, close_pos, close_goal;                  /* the tests 1, 2, 4, 5; 0: off                 */
} nep_mission_cfg;

/* nep_abi_sizeof(21): 64 bytes.  Mode FLEET_RUNS: who = scene, index = run, t_issue = t_run, length = the mean of the slots'
 * leg lengths summed in agent order, goal = 0, attempts = candidates examined by all the run's draws.                          */
typedef struct nep_mission_leg {
  int32_t who;                    /* global slot (mode PER_AGENT) or scene                                                   */
  int32_t index;                  /* goal index of the leg (0: the goal given to nep_batch_fleet_init) or run index          */
  int32_t outcome;                /* NEP_MISSION_*                                                                           */
  int32_t attempts;               /* candidates examined by the draw that followed (accepted k + 1, or max_attempts)         */
  double t_issue, t_end, length;
  double goal[3];
} nep_mission_leg;

/* One scene's mission state and inputs in host memory, for nep_mission_step (slots are the scene's agents, in order). */
typedef struct nep_mission_scene {
  int32_t n_agents, scene;        /* global slot = scene * n_agents + agent; the scene's ORIGIN index (see the recorder)     */
  int32_t round_ticks, n_poly;
  double t_now, dc;
  const double* pos;              /* [n_agents][round_ticks + 1][3]: p_0 .. p_round_ticks                                    */
  const double* s_end;            /* [n_agents][12]                                                                          */
  const double* pb;               /* [n_agents][2]                                                                           */
  const int32_t* poly_off;        /* [n_poly + 1] */
  const double* poly_xy;          /* counter-clockwise convex keep-outs                                                      */
  double* goal;                   /* [n_agents][3]                                                                           */
  int32_t* done;                  /* [n_agents]                                                                              */
  int32_t* flags;                 /* [n_agents] sticky NEP_FLEET_FLAG_*                                                      */
  double* t_issue;                /* [n_agents]                                                                              */
  double* length;                 /* [n_agents]                                                                              */
  int32_t* completed;             /* [n_agents]                                                                              */
  int32_t* counts;                /* [n_agents][4]: issued, reached, timed out, no goal                                      */
  double* sums;                   /* [n_agents][2]: leg time, leg length of the ended legs                                   */
  int32_t* scene_i;               /* [4]: run index, runs succeeded, runs failed, finished                                   */
  double* t_run;                  /* [1]                                                                                     */
  nep_mission_leg* log;           /* [n_agents][log_cap] (mode FLEET_RUNS: [log_cap]); record i of an owner sits at i mod log_cap */
  int32_t* log_n;                 /* [n_agents] (mode FLEET_RUNS: [1]) records ever written                                  */
} nep_mission_scene;

/* Host data, like nep_batch_set_scene_statics: the keep-out polygons of one scene (off [n_poly + 1], xy [off[n_poly]][2]).
 * Clockwise input is reversed, non-convex input or a polygon of fewer than 3 vertices refused (NEP_E_ARG); more than
 * NEP_MISSION_MAX_POLY polygons or NEP_MISSION_MAX_VERT vertices: NEP_E_CAP.  Convexity is judged with the tolerance of
 * nep_batch_set_scene_statics (a turn of -1e-9 (1 + scale)^2 passes), test 3 is exact: at a vertex that is reflex within that
 * tolerance, points within the same margin of it may fall on either side.  Hulls (scene.keepout_polygons) have no such vertex.
 * Callable before nep_batch_fleet_init and before nep_batch_fleet_mission_init, and between rounds afterwards (also after a
 * round was captured: the kernel reads the set from the handle's buffers); survives both inits.  Synchronises.                */
int nep_batch_fleet_mission_keepout(nep_batch_t* h, int32_t scene, int32_t n_poly, const int32_t* off, const double* xy);

/* Allocates (first call) or re-seeds the mission state, after nep_batch_fleet_init (which drops it, like the tether state): the
 * first leg / run is on the goals given to nep_batch_fleet_init with t_issue = t_run = the scenes' clocks, issued = 1, everything
 * else 0.  NEP_E_ARG on a bad configuration (mode PER_AGENT: min_dist_self <= goal_radius is one — a fresh goal must not count as
 * reached), NEP_E_STATE without fleet state, NEP_E_CAP beyond the limits above.  Synchronises; not capturable.                  */
int nep_batch_fleet_mission_init(nep_batch_t* h, const nep_mission_cfg* cfg, void* stream);

/* The controller, one wave per scene; between nep_batch_fleet_commit (and the audit / tether tracking) and nep_batch_fleet_tick.
 * Asynchronous, capturable.  NEP_E_STATE before nep_batch_fleet_mission_init.                                                  */
int nep_batch_fleet_mission(nep_batch_t* h, void* stream);

/* Blocking readers (host memory, each may be NULL).  Per slot: goal [slots][3], t_issue, length [slots], completed [slots], counts
 * [slots][4] (issued, reached, timed out, no goal), sums [slots][2] (leg time, leg length).  Per scene: scene_i [n_scenes][4] (run
 * index, runs succeeded, runs failed, finished), t_run [n_scenes].                                                              */
int nep_batch_fleet_mission_state(nep_batch_t* h, double* goal_out, double* t_issue_out, double* length_out, int32_t* completed_out,
                                  int32_t* counts_out, double* sums_out, int32_t* scene_out, double* t_run_out);
/* The log: log_out [owners][log_cap] records as stored (record i of an owner at i mod log_cap), n_out [owners] records ever
 * written; owners = slots (mode PER_AGENT) or scenes.  Returns log_cap.                                                          */
int nep_batch_fleet_mission_log(nep_batch_t* h, nep_mission_leg* log_out, int32_t* n_out);

/* Host form of nep_batch_fleet_mission for one scene (mission_host.cpp; no HIP call): the arithmetic is the kernel's
 * (neptune_amd/csrc/mission_common.h) and the device equals a chain of these calls byte for byte.  NEP_E_ARG on a bad
 * configuration or null pointers.                                                                                               */
int nep_mission_step(const nep_mission_cfg* cfg, nep_mission_scene* sc);

/* ---- scripted goals and the position-exchange driver ---------------------------------------------------------------------------
 * nep_batch_fleet_mission_script hands the controller a table of goals per slot: host data, goals [slots][n_goals][3] (slot =
 * scene * num_agents + agent), in the style of nep_batch_fleet_mission_keepout.  Wherever the controller would draw a goal for a
 * slot and a script is set, the goal is row (i - 1) mod n_goals of the slot's table, i being the slot's `issued` count at that
 * moment — the goal index the generator hashes; leg 0 is the goal given to nep_batch_fleet_init — with all three coordinates
 * (cfg.goal_z is not used).  No candidate is generated and none of the five tests is applied: the leg record's attempts is 0 (mode
 * FLEET_RUNS / FLEET_TOGETHER: the run's), the goal counts as found, and the no-goal path cannot be taken.  Triggers, quotas, logs,
 * t_issue, done and the move-back rule are what they are without a script.  The row follows from `issued`, which a snapshot
 * carries: the snapshot's layout, sizes and version do not change, and the table itself — like the keep-outs — is not in it.
 *
 * The table and its length live in the handle's device buffers and are read by the kernel when it runs.  Capacity: the n_goals of
 * the first upload with n_goals > 0 fixes the rows per slot for the handle's life; a later table of at most that many rows
 * replaces it in place (also between replays of a captured round, which then honours it), a longer one is NEP_E_CAP and changes
 * nothing.  n_goals = 0 switches the script off (and allocates nothing).  A non-finite coordinate is NEP_E_ARG.  The table
 * survives nep_batch_fleet_init and nep_batch_fleet_mission_init.  Synchronises; not capturable; nep_batch_fleet_mission itself
 * never allocates.  A round captured BEFORE the first upload with n_goals > 0 was recorded without the table's address: it keeps
 * drawing whatever is uploaded later.  Upload first, then capture.  Unsharded handles only (NEP_E_STATE).
 *
 * NEP_MISSION_FLEET_TOGETHER is scripts/auto_commands_together.py:154-182, the driver of the position exchange: like mode
 * FLEET_RUNS, except that `completed` is STICKY within a run — set at a tick where dx*dx < r*r && dy*dy < r*r (x-y only, r =
 * arrive_radius; the script's `< 0.5` on the squares is r = sqrt(0.5)) and cleared only by the next run — and that the leg grows
 * while completed is 0 before the tick's test, as in mode FLEET_RUNS.  The run is over when every slot is completed, or after
 * `timeout` (a failure; the script has no timeout: give +infinity).  Modes PER_AGENT and FLEET_RUNS take a script too, and mode
 * FLEET_TOGETHER without one draws.
 *
 * What differs from the reference (auto_commands_together.py):
 *   when it runs     the script compares every odometry message of every agent on wall-clock callbacks; here every flown tick is
 *                    tested, once per round, and the next goals are issued at the round's end.
 *   who advances     the script publishes the next list when its `completed` list is all true, then sleeps; here that is the run's
 *                    end, with a leg record (time, mean distance) the script does not keep.
 *   how long         the script alternates goals1 / goals0 while currentrun < 3; here max_goals runs (the first on the goals
 *                    given to nep_batch_fleet_init) over a table of any length, taken in a circle.
 *
 * nep_mission_step_script   the host form with a script: script [n_agents][n_goals][3], the scene's rows.  n_goals = 0 (script
 *                    may be NULL) is nep_mission_step for modes PER_AGENT and FLEET_RUNS, byte for byte.  nep_mission_step keeps
 *                    its contract — those two modes, anything else NEP_E_ARG —; mode FLEET_TOGETHER goes through this call.       */
int nep_batch_fleet_mission_script(nep_batch_t* h, int32_t n_goals, const double* goals);
int nep_mission_step_script(const nep_mission_cfg* cfg, nep_mission_scene* sc, int32_t n_goals, const double* script);

/* ---- effort: what the flown ticks cost, and whether they keep the limits ------------------------------------------------------------
 * scripts/benchmark_multi_direct.py judges a journey by its mean jerk (cmdCB: jerkSum += |j| * 0.05 per command, until completion).
 * nep_batch_fleet_effort accumulates that per slot over the ticks about to be flown, with the largest |component| of velocity,
 * acceleration and jerk and counts of the ticks that break a limit — the trajectories flown include guesses the QP never optimised
 * (nep_batch_guess_fallback), and nep_batch_audit judges positions only.
 *
 * The call goes where nep_batch_fleet_mission goes: after nep_batch_fleet_commit, before nep_batch_fleet_tick.  It walks the ticks
 * q = 1..round_ticks by the rule of nep_batch_fleet_mission and nep_batch_fleet_track_ent: s_q = ring[(head + min(q - 1, size - 1))
 * mod cap], 12 doubles (position, velocity, acceleration, jerk).  A tick is COUNTED when it pops a fresh state (q - 1 <= size - 1)
 * and the slot's done flag is clear: a repeated last state and an arrived agent add nothing.  Per counted tick, in tick order:
 *   n_ticks += 1;   jerk_sum = jerk_sum + sqrt((jx*jx + jy*jy) + jz*jz) * dc;   max_v[i] = max(max_v[i], |v_i|), likewise max_a, max_j;
 *   n_v_viol += 1 when |v_i| > v_max + slack for some i; n_a_viol with a_max; n_j_viol with j_max.
 * v_max and a_max are the handle's (nep_batch_cfg: one value for every axis); the handle keeps no j_max — it is a parameter of
 * the front end's configuration (nep_fe_cfg.j_max) — so the caller gives it.  slack is absolute and >= 0, the limits finite and
 * > 0, else NEP_E_ARG.  d_effort [slots] is the caller's, accumulated into (zero it first); chained calls equal one long call bit
 * for bit.  One thread per slot, no LDS, no atomics; reads the fleet state and writes d_effort only.  Asynchronous, capturable,
 * allocates nothing.  NEP_E_STATE without fleet state and on sharded handles.
 *
 * What differs from the reference (benchmark_multi_direct.py): the sum runs over the flown ticks at dc, not over command messages
 * at an assumed 0.05 s; it stops at the sticky arrival of nep_batch_fleet_tick (a mission's new goal starts it again), where the
 * script stops at its own completion test on agent 0's callbacks; the maxima and the violation counts are not in the script.
 *
 * nep_effort_step    host form for one slot (effort_host.cpp; no HIP call): ring [cap][12] with head and size, as the handle holds
 *                    them.  Shares effort_common.h with the kernel; the device equals a chain of these calls byte for byte.       */
/* nep_abi_sizeof(29): 96 bytes; 28 stays unassigned: tests/test_fleet_moveback_cpu.py pins it to -1 */
typedef struct nep_fleet_effort {
  double jerk_sum;                     /* sum over counted ticks of |jerk|_2 (3-D) * dc, added in tick order                  */
  double max_v[3], max_a[3], max_j[3]; /* largest |component| at a counted tick                                               */
  int32_t n_ticks, n_v_viol, n_a_viol, n_j_viol;
} nep_fleet_effort;
int nep_batch_fleet_effort(nep_batch_t* h, double j_max, double slack, nep_fleet_effort* d_effort, void* stream);
int nep_effort_step(double v_max, double a_max, double j_max, double dc, int32_t round_ticks, const double* ring, int32_t head,
                    int32_t size, int32_t cap, int32_t done, double slack, nep_fleet_effort* out);

/* ---- move-back: a new goal is approached by way of the agent's own base ---------------------------------------------------------
 * The reference's use_moveback_strategy (neptune_mtlp_benchmark.yaml: true; neptune_ros.cpp:1626-1636, :1291-1305): an agent that
 * receives a new terminal goal does not head for it.  It first plans towards (pb.x, pb.y, the goal's z), a point at its own base,
 * which unwinds its tether, and gets the real goal once it is within a radius of the base (yaml: 6.33 - (N - 4) * 0.33 m) or after
 * 10 s.  One slot, in this order (moveback_common.h is the one statement, shared by the kernel and the host form):
 *
 *   t_iss = the slot's t_issue (missions), else nep_fleet_cfg.t0;   f = the slot's NEP_FLEET_FLAG_* word
 *   if (t_iss == t_now)  f |= NEP_FLEET_FLAG_WAY_BACK
 *   if (f & NEP_FLEET_FLAG_WAY_BACK) { d = sqrt(dx*dx + dy*dy) of the tracked (x, y) less pb[agent];
 *                                      if (d < radius || t_now - t_iss > timeout)  f &= ~NEP_FLEET_FLAG_WAY_BACK }      (both strict)
 *   the word = f;   if (f & NEP_FLEET_FLAG_WAY_BACK)  d_start[slot].goal = (pb.x, pb.y, d_start[slot].goal[2])
 *
 * t_iss == t_now is exact: nep_batch_fleet_mission issues a goal with t_issue = t_end, round_ticks repeated additions of dc to the
 * clock, the very additions nep_batch_fleet_tick then makes, and nep_batch_fleet_mission_init starts t_issue at the scenes' clocks.
 * So a goal issued at the end of round r is seen by the call of round r + 1 and by no other, the first goal by the first round, and
 * a goal issued again (the no-goal path resets t_issue) starts a move-back again, as a re-published goal does in the reference.
 * The only state is the bit, in the slot's flag word (nep_batch_fleet_state's flags, section SFLAGS of a snapshot; T_ISSUE and T_NOW
 * are sections too: a snapshot carries a move-back in progress, and its layout, sizes and version are what they were).  The slot's
 * goal stays the real one: the mission's leg tests, nep_batch_fleet_tick's arrival test and the log do not change; only the goal the
 * search is given does.  A handle that never makes the call is what it was, byte for byte.
 *
 * What differs from the reference:
 *   when it runs     the release test runs once per round, on the tracked state at the select; the reference runs it at every
 *                    control tick (pubCB).
 *   timer            the simulated clock: 10 000 ms of wall clock become timeout = 10.0 s.
 *   radius           a parameter (neptune_amd.mission.MoveBack.reference(N) gives the yaml's formula).  It is <= 0 from N = 24 up,
 *                    and then only the timer releases.
 *   the own base     the back end treats the agent's own base square as an obstacle (solver_gurobi_poly.cpp:521-553), so an agent
 *                    approaches its base and does not reach it — the reference's behaviour too.
 *   move_when_goal_occupied, the yaml's other switch, is nep_batch_goal_gate (include/neptune_frontend.h), behind the front end: a
 *                    slot on its way back is tested at its base, the goal its search got.
 *
 * nep_batch_fleet_moveback   between nep_batch_fleet_select and the front end (tethered rounds: before or after
 *                    nep_batch_fleet_predict_ent, which does not read the goal).  One thread per slot, every slot whatever the
 *                    active mask.  Reads the handle's tracked states, bases, clocks and flag words, and the mission state's t_issue
 *                    when nep_batch_fleet_mission_init has run; writes the flag words and d_start[slot].goal, nothing else.
 *                    Asynchronous, allocates nothing, capturable.  NEP_E_STATE before nep_batch_fleet_init and on sharded handles;
 *                    NEP_E_ARG for a null pointer, a timeout that is negative or not finite, a radius that is not finite.
 * nep_moveback_step  host form for n slots of one scene (moveback_host.cpp; no HIP call): state [n][12], pb [n][2], t_issue [n] or
 *                    NULL (every goal was issued at t_first), flags [n] and start [n] updated in place.  The device equals a chain
 *                    of these calls byte for byte.  NEP_E_ARG as above.                                                           */
/* nep_abi_sizeof(27): 16 bytes */
typedef struct nep_moveback_cfg { double radius, timeout; } nep_moveback_cfg;
int nep_batch_fleet_moveback(nep_batch_t* h, const nep_moveback_cfg* cfg, nep_fe_start* d_start, void* stream);
int nep_moveback_step(const nep_moveback_cfg* cfg, int32_t n, const double* state, const double* pb, const double* t_issue,
                      double t_first, double t_now, int32_t* flags, nep_fe_start* start);

/* ---- recorder: snapshot, restore and replay ------------------------------------------------------------------------------------
 * A snapshot is the complete fleet state of a handle as one blob: whatever decides what the fleet calls do next.  A handle restored
 * from it continues byte for byte like the flight the snapshot was taken from (what that leaves out: nep_stats.solve_us, a measured
 * time, and the order in which slots are launched).
 *
 * Blob layout.  nep_fleet_snapshot_hdr (NEP_SNAPSHOT_HDR_BYTES = 80), then n_scenes scene blocks of scene_bytes each, scene 0
 * first.  A block is self-contained and contiguous — one scene of a blob is a slice — and is a sequence of NEP_SNAPSHOT_N_SECTIONS
 * sections in the order of the NEP_SNAP_* indices below.  A section holds the scene's part of one array of the handle, raw
 * ([N] slots of the scene, or one per-scene entry), padded with zeros to a multiple of 16 bytes: every section starts on a 16-byte
 * boundary (relative to the blob, which itself must be 16-byte aligned in device memory), scene_bytes is a multiple of 16, and the
 * same state gives the same bytes.  A section the state does not have is 0 bytes long.  The sizes follow from the header's
 * fields alone (nep_fleet_snapshot_describe gives offsets and sizes; neptune_amd/csrc/recorder_common.h is the one statement of
 * the arithmetic, shared by the library's host code and its kernels):
 *   the block's header  ORIGIN 4 (the scene's origin index, below), ROUND 4 (the round counter)
 *   fleet               RING N*ring_cap*96 (raw: stale entries included), HEAD SIZE K_END N*4, STATE N*96, GOAL N*24, PWP N*sizeof(nep_pwp),
 *                       FLOWN DONE OUTCOME SFLAGS N*4, PERIOD PHASE N*4 (timers != 0), T_NOW 8, COUNTERS 4*NEP_FLEET_N_COUNTERS
 *   tethers             form 1: ENT N*sizeof(nep_fe_ent_state).  form 2 (lists of tether_cap entries): L_N_ALPHA L_N_BEND N*4,
 *                       L_ID N*cap*2, L_CS N*cap, L_BETA N*cap*8, L_BEND N*NEP_MAX_BEND*2, HELD N*4.  Both: PUB_N N*4, PUB_XY
 *                       N*NEP_MAX_BEND*16 (the list published at the last select), PUB_PREV_N, PUB_PREV_XY (the one before), ENT_FLAGS
 *                       (last tracked round) ENT_EVER (sticky) ENT_WALKED N*4
 *   missions            T_ISSUE LENGTH N*8, COMPLETED N*4, COUNTS N*16, SUMS N*16, SCENE_I 16, T_RUN 8, LOG owners*log_cap*64,
 *                       LOG_N owners*4 with owners = N (mode PER_AGENT) or 1 (mode FLEET_RUNS)
 * cfg_hash is FNV-1a 64 (offset basis 0xcbf29ce484222325, prime 0x100000001b3) over the bytes of the nep_fleet_cfg given to
 * nep_batch_fleet_init, the 8 bytes of the cable length (0.0 without tethers) and the bytes of the nep_mission_cfg (zeros without
 * missions), in that order.
 *
 * Not in a snapshot: the scene geometry (statics, static representatives, keep-outs, bases); the handle's options; the handle-wide
 * sticky word nep_batch_check reports; the launch-order keys and other history that only changes the order of launches; the scratch
 * of the calls; and every buffer the caller owns — the audit records among them: nep_audit accumulates, so who resumes a flight
 * saves and restores that buffer himself.
 *
 * Origin.  The mission generator hashes the global slot, and a scene flown alone in a one-scene handle sits at scene 0 whatever
 * it was in its batch.  Every scene of the fleet state therefore carries an origin index: nep_batch_fleet_init sets it to the
 * scene's own index, a restore copies it from the block, and the mission controller uses origin * N + agent as the generator's
 * global slot and as `who` of a leg record (mode FLEET_RUNS: the origin), as nep_mission_scene.scene does on the host side.
 *
 * nep_batch_fleet_snapshot_bytes       header + n_scenes blocks for the state the handle has now (it grows when tethers or missions
 *                          are initialised afterwards).
 * nep_batch_fleet_snapshot             writes the blob to d_blob (device memory, 16-byte aligned) with one kernel, header included.
 *                          Asynchronous, capturable.  NEP_E_STATE before nep_batch_fleet_init; unsharded handles only.
 * nep_batch_fleet_snapshot_ring        the same kernel into a ring of the last n_entries rounds: d_ring is a header (n_scenes as the
 *                          handle's), a stamp table [n_entries][n_scenes] of nep_fleet_snapshot_stamp, then [n_entries][n_scenes]
 *                          scene blocks.  Scene s goes to entry round[s] mod n_entries, read on the device from the handle's round
 *                          counter, and its stamp becomes {1, round, origin, 0}; a table zeroed by the caller means empty.  The header
 *                          followed by the n_scenes blocks of one entry is a blob.  Asynchronous, capturable.
 * nep_batch_fleet_restore              puts a blob (host or device memory) back.  The handle has been through nep_batch_fleet_init,
 *                          the tether init of the blob's form and capacity and nep_batch_fleet_mission_init when the blob has mission
 *                          state, with the same configurations: the header is checked against the handle (N, num_pol, ring_cap,
 *                          max_states, timers, tether form and capacity, mission mode, log_cap, scene_bytes, cfg_hash) and `bytes`
 *                          against the header; any mismatch is NEP_E_ARG and leaves the handle's state exactly as it was.
 *                          src_scene = dst_scene = -1: all scenes (equal scene counts).  Otherwise block src_scene of the blob goes
 *                          into scene dst_scene of the handle.  Blocking; NEP_E_STATE while the calling thread's stream capture is on.
 * nep_fleet_snapshot_describe          host only: checks a header (magic, version, sizes, bytes >= header + blocks, scene_bytes a
 *                          multiple of 16 that holds every section: else NEP_E_ARG) and gives the sections' offsets in a block.   */
#define NEP_SNAPSHOT_MAGIC 0x5046454eu   /* "NEFP" */
#define NEP_SNAPSHOT_VERSION 1
#define NEP_SNAPSHOT_HDR_BYTES 80
#define NEP_SNAPSHOT_N_SECTIONS 41
enum {
  NEP_SNAP_ORIGIN = 0, NEP_SNAP_ROUND, NEP_SNAP_RING, NEP_SNAP_HEAD, NEP_SNAP_SIZE, NEP_SNAP_K_END, NEP_SNAP_STATE, NEP_SNAP_GOAL, NEP_SNAP_PWP,
  NEP_SNAP_FLOWN, NEP_SNAP_DONE, NEP_SNAP_OUTCOME, NEP_SNAP_SFLAGS, NEP_SNAP_PERIOD, NEP_SNAP_PHASE, NEP_SNAP_T_NOW, NEP_SNAP_COUNTERS,
  NEP_SNAP_ENT, NEP_SNAP_L_N_ALPHA, NEP_SNAP_L_N_BEND, NEP_SNAP_L_ID, NEP_SNAP_L_CS, NEP_SNAP_L_BETA, NEP_SNAP_L_BEND, NEP_SNAP_HELD,
  NEP_SNAP_PUB_N, NEP_SNAP_PUB_XY, NEP_SNAP_PUB_PREV_N, NEP_SNAP_PUB_PREV_XY, NEP_SNAP_ENT_FLAGS, NEP_SNAP_ENT_EVER, NEP_SNAP_ENT_WALKED,
  NEP_SNAP_T_ISSUE, NEP_SNAP_LENGTH, NEP_SNAP_COMPLETED, NEP_SNAP_COUNTS, NEP_SNAP_SUMS, NEP_SNAP_SCENE_I, NEP_SNAP_T_RUN, NEP_SNAP_LOG, NEP_SNAP_LOG_N
};

/* nep_abi_sizeof(25): NEP_SNAPSHOT_HDR_BYTES */
typedef struct nep_fleet_snapshot_hdr {
  uint32_t magic;                 /* NEP_SNAPSHOT_MAGIC                                                                      */
  int32_t version, hdr_bytes;     /* NEP_SNAPSHOT_VERSION, NEP_SNAPSHOT_HDR_BYTES                                            */
  int32_t n_scenes, N, num_pol, ring_cap, max_states;
  int32_t tether_form;            /* 0 none, 1 the fixed record, 2 lists                                                     */
  int32_t tether_cap;             /* form 1: NEP_FE_ENT_CAP, form 2: the lists' capacity, else 0                             */
  int32_t mission_mode;           /* 0 none, else NEP_MISSION_*                                                              */
  int32_t log_cap;
  int32_t timers;                 /* 1: the handle has periods and phases                                                    */
  int32_t _pad[3];
  int64_t scene_bytes;
  uint64_t cfg_hash;
} nep_fleet_snapshot_hdr;

/* one (entry, scene) of a ring's stamp table: 16 bytes */
typedef struct nep_fleet_snapshot_stamp { int32_t used, round, origin, _pad; } nep_fleet_snapshot_stamp;

typedef struct nep_fleet_snapshot_info {
  nep_fleet_snapshot_hdr hdr;
  int64_t offset[NEP_SNAPSHOT_N_SECTIONS];      /* of a section in its block                                                */
  int64_t bytes[NEP_SNAPSHOT_N_SECTIONS];       /* unpadded; 0: the state has no such section                               */
} nep_fleet_snapshot_info;

int64_t nep_batch_fleet_snapshot_bytes(const nep_batch_t* h);
int nep_batch_fleet_snapshot(nep_batch_t* h, void* d_blob, void* stream);
int64_t nep_batch_fleet_snapshot_ring_bytes(const nep_batch_t* h, int32_t n_entries);
int nep_batch_fleet_snapshot_ring(nep_batch_t* h, void* d_ring, int32_t n_entries, void* stream);
int nep_batch_fleet_restore(nep_batch_t* h, const void* blob, int64_t bytes, int32_t src_scene, int32_t dst_scene);
int nep_fleet_snapshot_describe(const void* host_blob, int64_t bytes, nep_fleet_snapshot_info* out);

/* ---- readers: blocking (they wait for the device), for tests and reports; every output is host memory and may be NULL ------ */
/* ring_cap of the handle's fleet state (NEP_E_STATE before nep_batch_fleet_init)                                              */
int nep_batch_fleet_ring_cap(nep_batch_t* h);
/* plans of slots first .. first + n - 1, front first: states_out [n][ring_cap][12] (entries beyond a plan's size are 0), sizes [n] */
int nep_batch_fleet_plans(nep_batch_t* h, int32_t first, int32_t n, double* states_out, int32_t* sizes);
/* per slot: tracked state [slots][12], trajectory [slots], has-flown / done / last outcome / sticky flags / last k_index_end [slots] */
int nep_batch_fleet_state(nep_batch_t* h, double* state_out, nep_pwp* pwp_out, int32_t* flown_out, int32_t* done_out,
                          int32_t* outcome_out, int32_t* flags_out, int32_t* k_end_out);
/* per scene: counters [n_scenes][NEP_FLEET_N_COUNTERS], clocks [n_scenes], round counters [n_scenes]                            */
int nep_batch_fleet_counters(nep_batch_t* h, int32_t* counters_out, double* t_now_out, int32_t* round_out);

#ifdef __cplusplus
}
#endif
#endif /* NEPTUNE_FLEET_H_ */
