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
 * Unsharded handles only (n_local == num_agents), else NEP_E_STATE.  Without a HIP device every call returns NEP_E_HIP.        */
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
#define NEP_FLEET_N_COUNTERS 8          /* per scene: one per outcome above, [6] accepted solves with NEP_RELAXED, [7] unused */

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
