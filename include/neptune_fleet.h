/* neptune_fleet.h — the committed plan of every agent of every scene on the device (SURVEY §8 f, rank 3, device form).
 *
 * include/neptune_plan.h keeps the plan deque, point A, the splice and the trajectory composition of Neptune::replanFull
 * (neptune.cpp:860-891, 1366-1425, 1661-1687) in host memory, one agent per handle: a closed loop built on it makes a host round
 * trip per agent and round.  Here the same state lives in the batched handle (include/neptune_backend.h: nep_batch_t), per
 * (scene, agent) slot, and three asynchronous calls move it — so a faithful round
 *
 *   nep_batch_fleet_select -> nep_batch_frontend -> nep_batch_replan -> nep_batch_safety_commit -> nep_batch_fleet_commit
 *     [-> nep_batch_audit] -> nep_batch_fleet_tick
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
 *   bookkeeping      sticky `done` (arrived), the last round's outcome, sticky NEP_FLEET_FLAG_* bits
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
 *   nep_batch_fleet_select -> nep_batch_fleet_predict_ent -> nep_batch_frontend_ent -> nep_batch_replan (entangle rows) ->
 *     nep_batch_safety_commit_ent -> nep_batch_fleet_commit [-> nep_batch_audit] -> nep_batch_fleet_track_ent -> nep_batch_fleet_tick
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
#define NEP_FLEET_QP_FAILED 2           /* nep_stats.status == NEP_FAILED                                                    */
#define NEP_FLEET_REJECTED 3            /* turned down by nep_batch_safety_commit                                           */
#define NEP_FLEET_ACCEPTED 4            /* plan spliced, trajectory composed                                                 */
#define NEP_FLEET_CAP 5                 /* accepted, but the plan or the trajectory would outgrow its storage: nothing changed */
#define NEP_FLEET_N_COUNTERS 8          /* per scene: one per outcome above, [6] accepted solves with NEP_RELAXED, [7] slots ever entangled (tethered fleets, else 0) */

#define NEP_FLEET_FLAG_SEG 1            /* sticky per slot: a composition needed more than NEP_TRAJ_MAX_SEG intervals        */
#define NEP_FLEET_FLAG_RING 2           /* a splice needed more than ring_cap states (or n_states > max_states)              */
#define NEP_FLEET_FLAG_SPLICE 4         /* a splice with size - 1 - k_index_end < 0 ("Already published the point A")        */

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
 * dropped) raises NEP_FLAG_ENT_TRACK.  Asynchronous, capturable.                                                              */
int nep_batch_fleet_track_ent(nep_batch_t* h, const nep_traj_rec* d_records, int32_t* d_flags, void* stream);

/* Blocking reader (host memory, each may be NULL): the states at the tracked positions, the last tracked round's flags, the sticky
 * flags, and per slot the (other agent, tick) pairs the tracking has actually walked since nep_batch_fleet_init_ent — the rest was
 * proven to add no crossing (nep_batch_debug_set_option "fleet_ent_proof" 0: everything is walked; same states).               */
int nep_batch_fleet_ent_state(nep_batch_t* h, nep_fe_ent_state* states_out, int32_t* flags_round_out, int32_t* flags_ever_out,
                              int32_t* walked_out);

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
