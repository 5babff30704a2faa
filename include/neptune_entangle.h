/* neptune_entangle.h — tether entanglement-state propagation along a trajectory (SURVEY §8 f, rank 4).
 *
 * Host-only C ABI (no HIP call), exported by libneptune_backend.so.  It produces the REAL inputs of
 * the back end's entangle rows — PolySolverGurobi::setEntStateVector's eu::ent_state per knot
 * (solver_gurobi_poly.cpp:307-314, read at :620-637) — from a guess trajectory, the other agents'
 * committed trajectories and the tether bend points, the way the front end accumulates them node by
 * node:
 *
 *   nep_ent_sample_points      Neptune::SamplePointsOfIntervals          neptune/src/neptune.cpp:500-565
 *   nep_ent_propagate_segment  KinodynamicSearch::entanglesWithOtherAgents  kinodynamic_search.cpp:707-895
 *                              with eu::entangleHSigToAddAgentInd        entangle_utils.cpp:1129-1228
 *                                   eu::entangleHSigToAddStatic          :1231-1277
 *                                   eu::addAlphaBetaToList / breakcondition   :1402-1534, :1608-1647
 *                                   eu::updateBendPts                    :1536-1604
 *                                   eu::getBendPt2d / calculateBetaForCase / getTetherLength  :1649-1743
 *   nep_ent_propagate_guess    the chain of node states KinodynamicSearch::recoverEntStateVector
 *                              returns for a path (kinodynamic_search.cpp:582-603), for a given guess
 *   nep_ent_case_ids           the (knot, agent) -> case id reduction of solver_gurobi_poly.cpp:624-631
 *                              in the dense layout nep_batch_replan consumes
 *   nep_ent_track_step         NeptuneRos::updateEntStateStaticObs (neptune_ros.cpp:800-850): the state of the
 *                              vehicle's own tether after one move, with eu::entangleHSigToAddAgentInd's nine-argument
 *                              form (entangle_utils.cpp:820-1127) for an agent whose bend points changed
 *   nep_ent_predict_a          Neptune::PredictAlphasBetas (neptune.cpp:976-1008): the state forwarded to point A in one
 *                              move with the eight-argument form throughout, into a copy
 */
#ifndef NEPTUNE_ENTANGLE_H_
#define NEPTUNE_ENTANGLE_H_

#include <stdint.h>

#include "neptune_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What KinodynamicSearch holds for the check: constructor arguments (kinodynamic_search.cpp:95-128),
 * setTetherLength (:259), setStaticObstRep (:385-390).                                            */
typedef struct nep_ent_cfg {
  int32_t num_agents;             /* pb.size()                                                      */
  int32_t id;                     /* 1-based id of the planning agent                               */
  int32_t num_pol;                /* planning intervals                                             */
  int32_t num_samples;            /* num_sample_per_interval (yaml: 3)                              */
  double T_span;
  double cable_length;            /* tether length (cablelength_)                                   */
  int32_t n_static;               /* staticObsRep_.size()                                           */
  int32_t _pad;
  const double* pb;               /* [num_agents][2] bases                                          */
  const double* static_rep;       /* [n_static][2][2]: col(0) = (x,y), col(1) = (x,y)               */
  const double* static_longest;   /* [n_static][2] staticObsLongestDist_                            */
} nep_ent_cfg;

/* Per-replan inputs: SampledPtsForAll_ and bendPtsForAgents_ (setUp, kinodynamic_search.cpp:190-257). */
typedef struct nep_ent_inputs {
  const double* sampled;          /* [num_agents][num_pol][num_samples+1][2]                        */
  const int32_t* present;         /* [num_agents]; 0 = SampledPtsForAll_[i].empty()                 */
  const int32_t* bend_off;        /* [num_agents+1] CSR offsets into bend_xy                        */
  const double* bend_xy;          /* [bend_off[num_agents]][2]                                      */
} nep_ent_inputs;

/* eu::ent_state (entangle_utils.hpp:23-29) in caller-owned arrays of capacity `cap` entries.       */
typedef struct nep_ent_state {
  int32_t n_alpha;                /* alphas.size() == betas.size()                                  */
  int32_t n_bend;                 /* bendPointsIdx.size()                                           */
  int32_t cap;
  int32_t n_active;               /* active_cases.size() (>= num_agents + n_static)                 */
  int32_t* alphas;                /* [cap][2] (agent or static id, case)                            */
  double* betas;                  /* [cap]                                                          */
  int32_t* bend_idx;              /* [cap]                                                          */
  int32_t* active_cases;          /* [n_active]                                                     */
} nep_ent_state;

/* Positions of one committed trajectory sampled on the planning grid; out: [num_pol][num_samples+1][2]. */
int nep_ent_sample_points(const nep_pwp* traj, double t_start, double t_end, int32_t num_pol,
                          int32_t num_samples, double* out);

/* One node expansion's entangle update for the segment with coefficients coeff_x/coeff_y ([a b c d],
 * local time) ending at end_xy, `index` = 1-based segment number.  Updates *state in place and adds
 * the sampled arc length to *arc_length.  Returns 1 when the reference's function returns true
 * (too many crossings, a second active case for an agent, tether too short), 0 otherwise,
 * NEP_E_ARG / NEP_E_CAP on bad input / capacity.                                                  */
int nep_ent_propagate_segment(const nep_ent_cfg* cfg, const nep_ent_inputs* in, nep_ent_state* state,
                              const double coeff_x[4], const double coeff_y[4], const double end_xy[2],
                              int32_t index, double* arc_length);

/* States at every knot of a K-segment guess, starting from *init (knot 0), in the flattened form
 * nep_backend_set_ent_state_vector takes (nep_ent_view): alpha_off [K+2], alphas [alpha_cap][2],
 * active_cases [K+1][n_active].  *entangled_at = first 1-based segment whose update returned 1
 * (the states from there on repeat the last good one), 0 if none.  *final receives the state at
 * the last propagated knot (may be NULL).                                                          */
int nep_ent_propagate_guess(const nep_ent_cfg* cfg, const nep_ent_inputs* in, const nep_ent_state* init,
                            const nep_guess* guess, int32_t alpha_cap, int32_t* alpha_off,
                            int32_t* alphas, int32_t* active_cases, int32_t* entangled_at,
                            nep_ent_state* final_state);

/* case_id[i][j] for knots i < NEP_MAX_POL, agents j < num_agents (0 = no single active case).     */
int nep_ent_case_ids(int32_t n_states, int32_t n_active, const int32_t* alpha_off, const int32_t* alphas,
                     const int32_t* active_cases, int32_t num_agents, int32_t* case_id);

/* ---- Tracking the tether between rounds (nep_batch_track_ent is its device form, include/neptune_frontend.h) ---------------
 * What updateEntStateStaticObs reads of the other agents at one check: previousCheckingPosAgent_ / latestCheckingPosAgent_
 * and the bend points their trajectory messages carried at the previous check and now (bendPtsForAgents_prev_ /
 * bendPtsForAgents_, base first).  An agent i with present[i] == 0 or no bend point is skipped, as there (:810).         */
typedef struct nep_ent_track_inputs {
  const double* pik;              /* [num_agents][2] every agent at the previous check                                  */
  const double* pik1;             /* [num_agents][2] ... now                                                            */
  const int32_t* present;         /* [num_agents]                                                                       */
  const int32_t* bend_off;        /* [num_agents+1] CSR offsets into bend_xy: the current bend points                   */
  const double* bend_xy;
  const int32_t* bend_off_prev;   /* [num_agents+1] CSR offsets into bend_xy_prev: those of the previous check          */
  const double* bend_xy_prev;
} nep_ent_track_inputs;

#define NEP_ENT_TRACK_ENTANGLED 1   /* some active_cases[i] > 2 (agents): what the reference reports as entangled (:842-849)   */
#define NEP_ENT_TRACK_TWO_CASES 2   /* some active_cases[i] >= 2 (agents): a state the search never creates                    */
#define NEP_ENT_TRACK_TOO_LONG 4    /* the tether is longer than cfg->cable_length (eu::getTetherLength)                      */
#define NEP_ENT_TRACK_CAP 8         /* a capacity was exceeded: the state is left as it was before the move                    */
#define NEP_ENT_TRACK_ABORT 16      /* the nine-argument form reached a branch after which the reference stops the process
                                       (exit(-1), "stop1".."stop4"): its crossing is added as there and the update goes on   */
#define NEP_ENT_TRACK_HELD 32       /* device, list form only (nep_batch_fleet_predict_ent): the state at point A holds more than
                                       NEP_FE_ENT_CAP crossings, the slot does not plan this round.  Not a capacity: nothing is lost */

/* Capacity (not a flag): new crossings one move may add — the device's list of a step's crossings (kEntAddCap, ent_device.h) */
#define NEP_ENT_TRACK_ADD_CAP 32

/* One check of the vehicle's own tether for the move pk -> pk1, updating *state in place: the crossings of the move with
 * every other agent's tether (their move pik[i] -> pik1[i]; the nine-argument form when their bend-point count changed
 * since the previous check) and with the static representatives, addAlphaBetaToList, updateBendPts.  No test stops the
 * update (the reference's updateEntStateStaticObs has none).  cfg: num_agents, id, cable_length and the statics are
 * read (num_pol, num_samples and T_span are not).  Capacities: state->cap list entries, NEP_MAX_BEND - 1 bend points (what
 * a published record holds besides the base), NEP_ENT_TRACK_ADD_CAP new crossings; beyond any of them the state is left
 * as it was and NEP_ENT_TRACK_CAP is returned alone.  Returns the NEP_ENT_TRACK_* bits of the updated state (>= 0), or
 * NEP_E_ARG.                                                                                                            */
int nep_ent_track_step(const nep_ent_cfg* cfg, const nep_ent_track_inputs* in, nep_ent_state* state, const double pk[2],
                       const double pk1[2]);

/* Neptune::PredictAlphasBetas for one agent: the entangle_state_A the front end and the safety re-check start from.  The
 * vehicle goes from where it is (pk) to point A (pk1) in one move while every other agent i goes from where it was last seen
 * (pik[i]) to its first sampled point (pik1[i]); the CURRENT bend lists serve as the previous check's too, so the
 * eight-argument crossing test runs for every agent.  *in (entangle_state_) is not touched; *out — caller-owned arrays like
 * *in's, out->cap and out->n_active set by the caller, n_active == in->n_active — receives the result.  Exactly one
 * nep_ent_track_step on a copy: the same flags, the same capacities (in->cap bounds the list as there, out->cap must hold it);
 * on NEP_ENT_TRACK_CAP *out equals *in.  nep_batch_fleet_predict_ent (include/neptune_fleet.h) is its device form.          */
int nep_ent_predict_a(const nep_ent_cfg* cfg, const double* pik, const double* pik1, const int32_t* present, const int32_t* bend_off,
                      const double* bend_xy, const nep_ent_state* in, const double pk[2], const double pk1[2], nep_ent_state* out);

/* ---- The tether audit: taut length, slack and winding of every flown tick --------------------------------
 * eu::getTetherLength of *state with the vehicle at pk1: base -> the anchors of the bend indices, + 2 x static_longest per static
 * anchor, -> pk1, summed in that order — the very expression nep_ent_track_step compares with cfg->cable_length.  What the
 * reference prints from pubCB every 100 ms (neptune_ros.cpp:1264-1267).  cfg: num_agents, id, pb and the statics are read.
 * Returns NEP_OK, or NEP_E_ARG (a null argument, a malformed state, a bend index that names nobody).                        */
int nep_ent_tether_length(const nep_ent_cfg* cfg, const nep_ent_state* state, const double pk1[2], double* len);

/* One record per (scene, agent); nep_abi_sizeof(37): 120 bytes.  One tracked move is one tick.  Calls accumulate into it; the
 * ticks of a whole flight are numbered from 1 (`tick_*` fields and `entangled_partner`, `wind_partner`: 0 = never / nobody).
 * The length of a tick is taken on the state after its move with the vehicle at that tick's position; on a dropped move
 * (NEP_ENT_TRACK_CAP) on the state that was kept — it lies behind the tether, n_dropped says so — and the other flag counters
 * stand still.  A maximum is replaced only by a strictly larger value: ties go to the earlier tick and, within a tick, to the
 * lower agent id.  Initial values (nep_tether_audit_init): max_len -inf, every time 0.0, everything else 0.                  */
typedef struct nep_tether_audit {
  double max_len;                 /* the largest taut length after a tracked move                                       */
  double t_max_len;               /* ... the time of that tick                                                          */
  double sum_len;                 /* running sum over the audited ticks, added in tick order (mean = sum_len / n_ticks)  */
  double last_len;                /* the length at the last audited tick                                                */
  double t_first_too_long;
  double t_first_entangled;
  double t_max_wind;
  int32_t tick_max_len;           /* the value of n_ticks after counting that tick                                      */
  int32_t n_ticks;                /* ticks audited                                                                      */
  int32_t n_too_long;             /* ticks whose move returned NEP_ENT_TRACK_TOO_LONG                                   */
  int32_t n_entangled;            /* ... NEP_ENT_TRACK_ENTANGLED                                                        */
  int32_t n_two_cases;            /* ... NEP_ENT_TRACK_TWO_CASES                                                        */
  int32_t n_abort;                /* ... NEP_ENT_TRACK_ABORT                                                            */
  int32_t n_dropped;              /* ticks whose move was dropped (NEP_ENT_TRACK_CAP)                                   */
  int32_t tick_first_too_long;
  int32_t tick_first_entangled;
  int32_t entangled_partner;      /* 1-based id of the lowest agent i with active_cases[i] > 2 at that tick              */
  int32_t max_alpha;              /* the largest n_alpha / n_bend the state held after a tick                           */
  int32_t max_bend;
  int32_t max_wind;               /* the largest active_cases[i] over the agents i, as the ENTANGLED rule reads it        */
  int32_t wind_partner;           /* ... 1-based id of the lowest such i                                                */
  int32_t tick_max_wind;
  int32_t crossings_added;        /* sum over ticks of the new crossings the moves produced (the step list before the merge;
                                     a move with more than NEP_ENT_TRACK_ADD_CAP counts NEP_ENT_TRACK_ADD_CAP)            */
} nep_tether_audit;

/* out[0..n) = the initial values.  NEP_E_ARG for a null pointer or n < 0.                                                    */
int nep_tether_audit_init(nep_tether_audit* out, int64_t n);

/* nep_ent_track_step plus one tick accumulated into *a, `t` the tick's time (t0 + (double)q * dt for tick q = 1.. of a stretch):
 * the same return value, the same *state.  A call that returns NEP_E_ARG audits nothing.  nep_batch_set_tether_audit
 * (include/neptune_frontend.h) is the device form; the two are equal byte for byte.                                         */
int nep_ent_track_step_audit(const nep_ent_cfg* cfg, const nep_ent_track_inputs* in, nep_ent_state* state, const double pk[2],
                             const double pk1[2], double t, nep_tether_audit* a);

#ifdef __cplusplus
}
#endif
#endif /* NEPTUNE_ENTANGLE_H_ */
