/* neptune_frontend.h — batched front-end initial-guess generator (SURVEY §8 f, rank 2).
 *
 * GPU counterpart of KinodynamicSearch (reference neptune/src/kinodynamic_search.cpp) for the batched
 * pipeline: every (scene, agent) slot searches the jerk lattice for a kinodynamically feasible,
 * collision-free K-segment cubic from its point A toward its goal and writes the nep_guess the back
 * end starts from, so that hulls -> guess -> separator -> QP runs on the device without a host
 * round trip (Neptune::replanFull, neptune.cpp:1302-1725, between point-A selection and commit).
 *
 * What is kept from the reference, rule by rule (kinodynamic_search.cpp):
 *   motion primitives   constant jerk on a num_samples x num_samples lattice in [-j_max, j_max]^2 over
 *                       T_span (:1045-1097, :1240-1275); primitive [a b c d] = [j/6, a0/2, v0, p0]
 *   pruning of a child  |end - start| < 1e-5, acceleration bounds, MINVO position control points in
 *                       the box and within the tether length of the base, MINVO velocity control points
 *                       in bounds (not for the first segment, as in the reference's initial overload),
 *                       the four "cannot brake in time" tests (:1079-1152, :1262-1330)
 *   collision           gjk::collision of the child's control polygon with the hull of every other
 *                       agent's committed trajectory over the child's interval (index clamped to
 *                       num_pol) and with every inflated static obstacle (:1514-1553)
 *   costs               g = travelled chord length, h = distance to the goal, order by g + bias*h
 *                       (:1177-1179, CompareCost); one node per voxel of size voxel_size (:1170-1173)
 *   termination         a node within goal_size of the goal ends the search (:1719-1737); the plan is
 *                       the first num_pol segments of the path (:521-553); z = Neptune::getInitialZPwp's clamped B-spline
 *                       ramp from A's height state to the goal height (neptune.cpp:1727-1810; as there,
 *                       the first three control points are placed for a clamped basis but evaluated with
 *                       the uniform one, so only a start at rest is reproduced exactly)
 * What differs — the default search is a level-synchronous BEAM over the same lattice, not the reference's A*:
 *   the reference's open list is a wall-clock-bounded best-first search whose expansion order is
 *   shuffled with a time seed (:321-322, :1462-1463) and whose closed-set update toggles with a call
 *   counter (:1190-1203); it is not reproducible even against itself.  In the beam depth d keeps the
 *   beam_width best children (ties by parent rank, then lattice index), a voxel holds one node per
 *   depth and is closed to later depths, the depth is num_pol, and without reaching the goal the best
 *   node of the last depth is returned.  The deterministic rule is stated in oracle/ and the kernel
 *   matches it bit for bit.
 * The reference's own strategy is available next to it (nep_batch_set_fe_astar, nep_batch_frontend_astar
 *   below): best-first on g + bias*h over a binary heap, unbounded depth, one node per voxel with the
 *   in-place update of an open node on every second such event, the "nearest the start" fallback node —
 *   with the two things that make the reference irreproducible turned into parameters (the lattice
 *   order, and a budget of pops in place of the wall clock).  Bit-identical to oracle/'s
 *   orc_frontend_astar.  With the entangle check on it is nep_batch_frontend_astar_ent (below): the same search with a tether
 *   state per node, bit-identical to its Python restatement, tests/astar_ent_ref.py.
 */
#ifndef NEPTUNE_FRONTEND_H_
#define NEPTUNE_FRONTEND_H_

#include <stdint.h>

#include "neptune_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NEP_FE_MAX_BEAM 64
#define NEP_FE_MAX_SAMPLES 5
#define NEP_FE_ENT_CAP 40        /* (a fixed ABI constant: nep_fe_ent_state's layout depends on it; nep_abi_sizeof(14) lets a client verify)
                                     crossings of the FIXED entangle-state record (nep_fe_ent_state: the state at point A
                                     the caller passes in, and a search node's state on the fast path).  It is not a
                                     limit of the search: the reference prunes a node at num_agents + statics crossings
                                     (kinodynamic_search.cpp:850-854) and so does the front end — a node whose list, new
                                     crossings of one sampled step (more than 32) or bend points (more than NEP_MAX_BEND)
                                     outgrow the fixed record is carried, with all its descendants, in a "big record" of
                                     a per-handle pool in device memory that is sized by that very bound (round 4; before,
                                     such a node was pruned and flagged).  nep_fe_result.ent_overflow now only says that
                                     the POOL ran out (nep_batch_set_fe_ent_big_records)                              */

#define NEP_FE_GOAL_REACHED 1     /* status codes of KinodynamicSearch::run (:1637-1639)          */
#define NEP_FE_DEPTH_REACHED 0    /* (RUNTIME_REACHED there): best node of the last depth         */
#define NEP_FE_EMPTY 2            /* the beam died out: best node of the last non-empty depth     */
#define NEP_FE_NO_SOLUTION 3      /* no feasible first segment: K = 0, nothing to optimise        */
#define NEP_FE_SKIPPED 4          /* slot not in the active set (nep_batch_set_active): no search  */

/* setMaxValuesAndSamples / setXYZMinMaxAndRa / setBias / setGoalSize / setTetherLength
 * (call sites neptune.cpp:92-97); bounds, bases and T_span come from the batch handle.          */
typedef struct nep_fe_cfg {
  double j_max;                   /* par_.j_max                                                    */
  double voxel_size;              /* par_.a_star_fraction_voxel_size                               */
  double bias;                    /* 1.1 (neptune.cpp:96)                                          */
  double goal_size;               /* par_.goal_radius                                              */
  double cable_length;            /* par_.tetherLength                                             */
  int32_t num_samples;            /* par_.a_star_samp_x, <= NEP_FE_MAX_SAMPLES                     */
  int32_t beam_width;             /* <= NEP_FE_MAX_BEAM (this build's search width)                */
  int32_t pad_hold;               /* 1: a guess shorter than num_pol (goal reached early, beam died out) is
                                     extended with segments that hold its end point, so that the back end
                                     also separates the place where the vehicle will WAIT from everybody's
                                     committed trajectory (the reference leaves that unchecked,
                                     kinodynamic_search.cpp:1805-1813)                               */
  int32_t enable_entangle;        /* par_.enable_entangle_check: nep_batch_frontend_ent only                       */
  int32_t ent_samples;            /* num_sample_per_interval (yaml: 3), 1..8                                       */
  int32_t _pad;
} nep_fe_cfg;

/* eu::ent_state of one search node / of point A (entangle_utils.hpp:23-29) in a fixed-size record: the crossing list
 * (agent or static id, case), its betas and the bend-point indices; active_cases[i] is the number of list entries of
 * agent i and is not stored.  beta of an AGENT crossing (id <= num_agents) is 0.0, as the reference's calculateBetaForCase
 * returns it (entangle_utils.cpp:1713-1719); only static crossings carry one.  States made by nep_ent_propagate_* honour that;
 * a state that does not is flagged by nep_batch_check (the search does not read such betas).                              */
typedef struct nep_fe_ent_state {
  int32_t n_alpha, n_bend;
  int16_t id[NEP_FE_ENT_CAP];
  int8_t cs[NEP_FE_ENT_CAP];
  double beta[NEP_FE_ENT_CAP];
  int8_t bend[NEP_MAX_BEND];
} nep_fe_ent_state;

/* Point A and the goal of one slot (setUp, kinodynamic_search.cpp:190-227).                      */
typedef struct nep_fe_start {
  double pos[3], vel[3], accel[3];   /* A; x,y enter the search, z the height profile               */
  double goal[3];                    /* G_term.pos                                                  */
  double t_start;                    /* neptune.cpp:1422-1423                                       */
} nep_fe_start;

typedef struct nep_fe_result {
  int32_t status;                 /* NEP_FE_*                                                      */
  int32_t K;                      /* segments of the guess (<= num_pol)                            */
  int32_t depth;                  /* depth at which the search stopped                             */
  int32_t n_children;             /* lattice children generated                                    */
  int32_t n_feasible;             /* ... that passed the kinodynamic tests                         */
  int32_t n_collision_free;       /* ... and the collision tests                                   */
  int32_t goal_occupied;          /* setUp's goal_occupied_ (:210-226)                             */
  int32_t _pad;                   /* entangle check on: bit 3 = the pool of big records ran out (ent_overflow); bits 8
                                     and up = children of this search whose state went into a big record; nep_batch_frontend_astar and
                                     nep_batch_frontend_astar_ent: bit 4 = the search ran into a node pool smaller than the
                                     reference's; nep_batch_goal_gate: bits 5 and 6 (NEP_FE_PAD_GATED, NEP_FE_PAD_GOAL_TAKEN); else 0 */
  double cost;                    /* g + bias*h of the returned node                               */
  double dist_to_goal;
  int32_t n_entangled;            /* children pruned by entanglesWithOtherAgents (entangle check on)        */
  int32_t ent_overflow;           /* 1: a child needed a big record and the handle's pool had none left (pruned), or
                                     more than 256 searches of one launch needed big records (the ones beyond keep
                                     the fixed record's limits: _pad bits 0-2 say which) — deviations from the
                                     reference's rule; 0 in every test and bench leg.  nep_batch_frontend_astar_ent: 1 = a
                                     child's state outgrew the fixed record and was dropped (it has no big records)  */
} nep_fe_result;

/* Front end of every slot of the batch handle, asynchronous on `stream`.
 *   d_committed : device, [n_scenes][N] nep_traj_rec (as nep_batch_replan)
 *   d_start     : device, [n_scenes][n_local] nep_fe_start
 *   d_guess     : device, [n_scenes][n_local] nep_guess     (out: what nep_batch_replan consumes)
 *   d_result    : device, [n_scenes][n_local] nep_fe_result (out, may be NULL)
 * The interval hulls are rebuilt into the handle's scratch exactly as nep_batch_replan does.      */
int nep_batch_frontend(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed,
                       const nep_fe_start* d_start, nep_guess* d_guess, nep_fe_result* d_result,
                       void* stream);

/* ---- The reference's best-first search (KinodynamicSearch::run, kinodynamic_search.cpp:1629-1827) -------------------------------
 * One wave per slot runs the search orc_frontend_astar (oracle/neptune_oracle.c) states, entangle check off:
 *   root expansion       without the velocity-control-point test (the reference's initial overload); later ones with it
 *   lattice order        children are visited in the order q = 0 .. num_samples^2 - 1, child q being lattice point order[q]
 *                        (jx = order[q] / num_samples, jy = order[q] % num_samples); the reference shuffles that list
 *   open list            a binary heap with libstdc++'s push_heap / pop_heap mechanics under CompareCost
 *                        (|cl - cr| < 1e-5 ? h_l > h_r : cl > cr), so ties pop as they do there
 *   voxel table          one node per voxel, the first insert wins; a child that hits an open node of its own index
 *                        overwrites it in place on every second such event when its g + bias*h is smaller, and the heap is
 *                        NOT re-ordered (:1190-1203); any other child of an occupied voxel is dropped
 *   pop                  budget first (max_pops pops: NEP_FE_DEPTH_REACHED), then the collision test of the node (:1514-1553),
 *                        the closest-so-far rule (:1683-1690), the goal test, the expansion
 *   result               the goal node, else the closest-so-far node; none: NEP_FE_NO_SOLUTION, K = 0.  The path's nodes of
 *                        index <= num_pol are the guess, z as in nep_batch_frontend.  nep_fe_result: n_children = pops,
 *                        n_feasible = nodes created, depth = index of the returned node (it may exceed num_pol),
 *                        n_collision_free = n_entangled = ent_overflow = 0, cost / dist_to_goal of the returned node
 *   pad_hold             as in nep_batch_frontend (the oracle's A* ignores it): segments beyond the plan hold the returned
 *                        node's end point, K = num_pol
 * nep_batch_set_fe_astar   the budget, the order and the per-slot pools.  Eager (it allocates and uploads): not capturable.
 *   max_pops >= 0; order: host, n_order = num_samples^2 entries, a permutation of 0 .. n_order - 1 (else NEP_E_ARG), or NULL:
 *   lattice order 0, 1, 2, ...  max_nodes: nodes per slot, 2 .. NEP_FE_ASTAR_MAX_NODES; 0 = min(NEP_FE_ASTAR_MAX_NODES,
 *   25 * (max_pops + 1) + 1), which no search of that budget can fill.  The reference stops creating nodes at 19 999
 *   (node_num_max_, kinodynamic_search.hpp:345); a smaller pool is a budget in the same sense — an expansion stops creating
 *   nodes at max_nodes - 1 and the search goes on with what it has — and a search cut that way says so: bit 4 of
 *   nep_fe_result._pad, and NEP_E_CAP from nep_batch_check.  Nothing is written past a pool.  Device memory per slot:
 *   max_nodes * (NEP_FE_ASTAR_NODE_BYTES + 4) bytes of nodes and heap plus 12 bytes per entry of the voxel table (the power of
 *   two at or above 2 * max_nodes): 4.1 MB at 20 000 nodes, 0.5 MB at the default of max_pops = 100.
 * nep_batch_frontend_astar asynchronous on `stream`, allocates nothing, capturable; arguments, hulls, active set
 *   (nep_batch_set_active: an inactive slot gets what nep_batch_frontend gives it), agent shards and several scenes per launch as
 *   nep_batch_frontend.  cfg->beam_width is not read.  NEP_E_STATE before nep_batch_set_fe_astar; NEP_E_ARG with
 *   cfg->enable_entangle != 0, or when an order is set and cfg->num_samples^2 != n_order.                                        */
#define NEP_FE_ASTAR_MAX_NODES 20000
#define NEP_FE_ASTAR_NODE_BYTES 160
int nep_batch_set_fe_astar(nep_batch_t* h, int32_t max_pops, int32_t max_nodes, const int32_t* order, int32_t n_order);
int nep_batch_frontend_astar(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start,
                             nep_guess* d_guess, nep_fe_result* d_result, void* stream);

/* ---- The reference's best-first search with enable_entangle_check -------------------------------------------------------------
 * nep_batch_frontend_astar with what "enable_entangle_check on" (below) adds to a search node, as the reference's run does:
 *   child        the parent's entangle state (the root: d_ent_init[slot], NULL = empty) through entanglesWithOtherAgents; true drops
 *                the child (n_entangled).  g = parent g + sampled arc length, h = distance to the goal + 0.3 per crossing + 1.0 per
 *                bend point
 *   voxel table  the key is (ix, iy, getIz(state)), for the root expansion's inserts too; an open node updated in place keeps its
 *                own entangle state (kinodynamic_search.cpp:1204 is commented out)
 *   pop          after the hulls and statics, the other agents' 0.7 m base squares; the closest-so-far rule and the goal test both
 *                ask for a valid end point (every active case count <= 1): an invalid node at the goal is expanded like any other
 *   result       as nep_batch_frontend_astar, with n_entangled; d_case_out [slots][NEP_MAX_POL][N] (may be NULL) as
 *                nep_batch_frontend_ent: row i from the state at the START of segment i of the returned path, rows at and beyond K
 *                zero; with pad_hold the held segments keep the returned node's state
 *   capacity     a node's state is the fixed record: a child whose list would outgrow NEP_FE_ENT_CAP entries, whose sampled step
 *                adds more than 32 crossings or whose bend points would exceed NEP_MAX_BEND is DROPPED, not counted in n_entangled,
 *                and the search says so: nep_fe_result.ent_overflow = 1 and NEP_E_CAP from nep_batch_check (a flag of its own, next
 *                to the pool's bit 4 of _pad).  Where num_agents + n_static <= NEP_FE_ENT_CAP the reference's own prune binds first.
 *                No big records here.  A malformed state at A (counts beyond the record, a bend index off the list) is flagged the
 *                same way and the search starts from the empty state.
 * Budget, order and node pool come from nep_batch_set_fe_astar (NEP_E_STATE before it).  Unsharded handle created with
 * enable_entangle (else NEP_E_STATE); cfg->enable_entangle != 0 (else NEP_E_ARG); cfg->num_samples^2 == n_order when an order is
 * set (else NEP_E_ARG); with static obstacles nep_batch_set_static_reps first.  Active sets and several scenes per launch as
 * nep_batch_frontend_astar (an inactive slot's case rows are not written, as by nep_batch_frontend_ent).
 * The FIRST call (and the first after a nep_batch_set_fe_astar that enlarges the pools) allocates, so it must be made eagerly, which
 * is nep_batch_frontend_ent's contract; later calls allocate nothing and can be captured.  Device memory per slot, beside
 * nep_batch_set_fe_astar's: max_nodes * NEP_FE_ASTAR_ENT_NODE_BYTES bytes of node states and 4 bytes per entry of the voxel table —
 * 9.1 MB more at 20 000 nodes (13.2 MB in all), 1.2 MB more at the default of max_pops = 100.                                   */
#define NEP_FE_ASTAR_ENT_NODE_BYTES 456
int nep_batch_frontend_astar_ent(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start, const nep_fe_ent_state* d_ent_init,
                                 nep_guess* d_guess, nep_fe_result* d_result, int32_t* d_case_out, void* stream);

/* ---- ... on four waves per search -------------------------------------------------------------------------------------------------
 * nep_batch_frontend_astar_ent runs one wave per search by default.  Its latency is one search's, nine tenths of it the children's
 * entangle propagation, and a launch of a few dozen searches leaves the GPU empty.  nep_batch_set_fe_astar_team(h, 4) makes the
 * calls that follow run a workgroup of four waves per search, which finds the children's new crossings in a dense pass over (child,
 * sampled step, chunk of obstacles) and leaves the list surgery to the children's lanes.  Measured on an MI355X (DESIGN.md section
 * 37): 3.0 to 3.3 times shorter launches up to 512 searches, 1.7 times from 1 024 to 4 096 (a CU holds two such workgroups).
 *   results     bit-identical to the one-wave form: every byte of every output
 *   scope       nep_batch_frontend_astar_ent only.  nep_batch_frontend_astar (check off) keeps its one wave whatever the setting
 *   setter      waves 1 (the default) or 4, anything else NEP_E_ARG.  Eager, allocates nothing, legal before or after
 *               nep_batch_set_fe_astar in any order; a later nep_batch_set_fe_astar leaves it alone
 *   graphs      a captured graph keeps the form it was captured with; the setter does not reach into it.  As for the entry point
 *               itself, the first call of a form on a process is made eagerly
 *   storage     pools, budget, order, voxel table, active sets, several scenes per launch, the eager first call and the NEP_E_*
 *               conditions are nep_batch_frontend_astar_ent's: both forms read and write the same per-slot memory, so calls with
 *               waves 1 and 4 may alternate on one handle
 *   reader      nep_batch_fe_astar_team: the waves per search of the last nep_batch_frontend_astar_ent call on this handle, 0
 *               when there has been none (no other call changes it)                                                               */
int nep_batch_set_fe_astar_team(nep_batch_t* h, int32_t waves);   /* 1 (default) or 4; anything else NEP_E_ARG */
int nep_batch_fe_astar_team(nep_batch_t* h);

/* ---- move_when_goal_occupied: a plan that does not reach its goal is flown only when somebody is on the goal --------------------
 * The reference's benchmark yaml sets move_when_goal_occupied next to use_not_reaching_soln.  Neptune::replanFull (neptune.cpp:1480-1500):
 * a search that did not reach the goal (search_result != 1) has returned its closest-so-far node; that node is flown only if
 * gjk::collision finds the square goal +- drone_radius on the LAST interval hull of some entry of hulls2d (the other agents' committed
 * trajectories; the statics are not in it).  Otherwise replanFull returns false and the vehicle keeps its committed plan.
 *
 * nep_batch_goal_gate   goes between ANY front-end call and nep_batch_replan and reads only d_result[slot].status, so it serves the
 *   beam and both best-first searches alike.  One wave per slot (goal_gate.h).  A slot whose status is NEP_FE_GOAL_REACHED,
 *   NEP_FE_NO_SOLUTION or NEP_FE_SKIPPED is not touched.  A slot with NEP_FE_DEPTH_REACHED or NEP_FE_EMPTY is examined:
 *     the goal      d_start[slot].goal, the goal the search got (a slot on its way back, nep_batch_fleet_moveback, is tested at its
 *                   base, as setTerminalGoal(near_base) makes the reference do)
 *     the box       (gx+r, gy+r), (gx+r, gy-r), (gx-r, gy+r), (gx-r, gy-r), r = half_side: the column order of neptune.cpp:1485-1488
 *     occupied      some agent j != own has hull_nv > 0 and gjk_collision true on its hull of interval num_pol - 1: the obstacle set
 *                   and indexing of the searches' own goal_occupied_ test.  The hulls are the ones the preceding front-end call left
 *                   in the handle's scratch; the gate builds none.
 *     occupied      _pad |= NEP_FE_PAD_GOAL_TAKEN; nothing else is written.
 *     free          the slot becomes what a search without a first primitive leaves: d_guess[slot] K = 0, n_alpha = 0, every
 *                   coefficient 0.0, t_start kept; d_result[slot] status = NEP_FE_NO_SOLUTION, K = 0, _pad |= NEP_FE_PAD_GATED, every
 *                   other field kept (the search that was turned down stays visible); with d_case the slot's NEP_MAX_POL x N case
 *                   rows are zeroed.  The replan, the safety pass and nep_batch_fleet_commit (NEP_FLEET_FE_NO_SOLUTION) know these bytes.
 *   d_count         [n_scenes][4] or NULL: {examined, let through, turned down, 0} per scene, ADDED to with integer atomics; the
 *                   caller owns and zeroes it.  A second call on the same buffers examines the let-through slots again (and counts
 *                   them again); the slots it turned down are NEP_FE_NO_SOLUTION now.
 *   What differs from the reference: the test runs once per bulk-synchronous round, against the hulls every agent's search saw;
 *   nep_fe_result.goal_occupied stays setUp's other box (kinodynamic_search.cpp:210-226, half side 0.5 hard-coded).
 *   Asynchronous on `stream`, allocates nothing, capturable.  NEP_E_ARG: a null h, d_start, d_guess or d_result, a half_side that
 *   is not finite or <= 0.  NEP_E_STATE: no nep_batch_frontend / _ent / _astar / _astar_ent call has been made on the handle, or the
 *   last front-end call was a _hulls one (no hulls in the scratch); a sharded handle (n_local != num_agents).  The _hulls / sharded
 *   form and a host form are not built.                                                                                          */
#define NEP_FE_PAD_GATED      32   /* nep_fe_result._pad bit 5: turned down by nep_batch_goal_gate */
#define NEP_FE_PAD_GOAL_TAKEN 64   /* bit 6: examined by the gate, goal occupied, let through      */
int nep_batch_goal_gate(nep_batch_t* h, double half_side, const nep_fe_start* d_start, nep_guess* d_guess,
                        nep_fe_result* d_result, int32_t* d_case /* [slots][NEP_MAX_POL][N] or NULL */,
                        int32_t* d_count /* [n_scenes][4], accumulating, or NULL */, void* stream);

/* The same against all-gathered hull blocks (multi-GPU rounds, include/neptune_backend.h:
 * nep_batch_hulls -> all-gather -> nep_batch_frontend_hulls -> nep_batch_replan_hulls).            */
int nep_batch_frontend_hulls(nep_batch_t* h, const nep_fe_cfg* cfg, const void* d_blocks, int32_t n_blocks,
                             const nep_fe_start* d_start, nep_guess* d_guess, nep_fe_result* d_result,
                             void* stream);

/* ---- enable_entangle_check on ---------------------------------------------------------------------------------
 * The search node carries the tether's entangle state (eu::ent_state) the way the reference's does:
 *   pruning     entanglesWithOtherAgents on every child (kinodynamic_search.cpp:1160-1164, :1345-1353, body :707-895):
 *               crossings of the child's sampled step with every other agent's tether polyline (its committed
 *               trajectory sampled ent_samples times per interval, Neptune::SamplePointsOfIntervals neptune.cpp:500-565,
 *               and its bend points from the record) and with the static representatives; cancellation against the
 *               accumulated list; a second active case for an agent, too many crossings or a tether longer than
 *               cable_length prune the child
 *   costs       g = sampled arc length, h = distance to the goal + 0.3 per crossing + 1.0 per bend point (:1177-1182)
 *   voxel       (ix, iy, getIz(state)) (:1170-1173, :2006-2031)
 *   collision   additionally the other agents' 0.7 m base squares (collidesWithBases2d, :1583-1628, :1675)
 *   end point   only a node whose active cases are all <= 1 may end the plan (:1693-1700)
 * and the states along the returned path give the dense case block nep_batch_replan's d_ent takes (the case of
 * (segment i, agent j) from the state at the START of segment i, solver_gurobi_poly.cpp:624-631) — guesses AND entangle
 * cases are then device-made.  Bit-identical to oracle/'s orc_frontend_beam_ent.
 *
 * nep_batch_set_static_reps   staticObsRep_ / staticObsLongestDist_ (setStaticObstRep, kinodynamic_search.cpp:385-390):
 *                             rep [n_static][2][2] (col(0), col(1)), longest [n_static][2]; scene = -1: every scene
 * nep_batch_frontend_ent      d_ent_init: [slots] state at point A or NULL (empty); d_case_out: [slots][NEP_MAX_POL][N]
 *                             (out, may be NULL).  Unsharded handle (n_local == num_agents), created with enable_entangle;
 *                             sharded handles: nep_batch_frontend_ent_hulls below.
 * nep_batch_safety_commit_ent nep_batch_safety_commit plus KinodynamicSearch::entangleCheckGivenPwp (:897-985) as
 *                             Neptune::safetyCheckAfterReplan calls it (neptune.cpp:746-754): every new trajectory is
 *                             re-checked from the state at its start against everybody's NEW trajectories and bend
 *                             points; as in the reference only its FIRST interval is examined (the loop returns at the
 *                             end of its first pass, :983), with three times the search's crossing capacity and no
 *                             tether-length test.  An entangling trajectory is turned down like a colliding one.   */
int nep_batch_set_static_reps(nep_batch_t* h, int32_t scene, const double* rep, const double* longest);
/* Big records of the entangle-aware front end (see NEP_FE_ENT_CAP above).
 * nep_batch_set_fe_ent_big_records   records in the handle's pool (0: the default, 4 per slot and at least 4 096); a record
 *                                    holds num_agents + statics crossings (13 bytes each) and the scratch of one sampled
 *                                    step; takes effect at the next front-end call (not while a stream is capturing).
 * nep_batch_set_fe_ent_fast_caps     (neptune_backend_debug.h) what the fixed record's path accepts before a child goes to a big record: list
 *                                    entries (<= NEP_FE_ENT_CAP), new crossings per sampled step (<= 32), bend points
 *                                    (<= NEP_MAX_BEND).  The results do not depend on these — the tests set them to
 *                                    0 / 1 / 2 to drive ordinary scenes through the big records.
 * The FIRST entangle-aware front-end call of a handle (and the first after a setting that changes a size) allocates the search's
 * device scratch — per-child states, the big-record pool and its betas, ≈ 0.3 GB at BASELINE configs[4] with 32 scenes — so it
 * must be made eagerly, before any stream capture: inside a capture the allocation fails with NEP_E_HIP.  Later calls with the
 * same sizes allocate nothing and can be captured (bench_legs/ does exactly that: warm-up steps first, then the graph).       */
int nep_batch_set_fe_ent_big_records(nep_batch_t* h, int64_t records);
int nep_batch_frontend_ent(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start,
                           const nep_fe_ent_state* d_ent_init, nep_guess* d_guess, nep_fe_result* d_result,
                           int32_t* d_case_out, void* stream);
/* nep_batch_frontend_ent against all-gathered hull blocks (multi-GPU rounds: the blocks of a handle created with
 * enable_entangle carry every agent's samples and presence flag next to its hulls and bend points, nep_batch_hulls);
 * cfg->ent_samples must equal the handle's nep_batch_set_ent_samples value (3 by default).  Bit-identical to
 * nep_batch_frontend_ent on an unsharded handle.                                                                      */
int nep_batch_frontend_ent_hulls(nep_batch_t* h, const nep_fe_cfg* cfg, const void* d_blocks, int32_t n_blocks, const nep_fe_start* d_start,
                                 const nep_fe_ent_state* d_ent_init, nep_guess* d_guess, nep_fe_result* d_result,
                                 int32_t* d_case_out, void* stream);
/* On a sharded handle nep_batch_safety_commit_ent takes, like the records, the entangle states of ALL agents:
 * d_ent_init [n_scenes][N] (gather them with nep_batch_exchange_slots); d_guess stays [n_scenes][n_local] (it supplies the
 * round's clock).  Every rank then computes the same accept vector.                                                   */
int nep_batch_safety_commit_ent(nep_batch_t* h, const nep_traj_rec* d_prev, const nep_traj_rec* d_new, const nep_guess* d_guess,
                                const nep_fe_ent_state* d_ent_init, int32_t ent_samples, double cable_length,
                                nep_traj_rec* d_final, int32_t* d_accept, void* stream);

/* ---- Tracking the tethers between rounds (NeptuneRos::odomCB -> updateEntStateStaticObs, neptune_ros.cpp:781-850) ---------
 * nep_batch_track_ent     every agent of every scene flies intervals 1..n_intervals (1 <= n_intervals <= num_pol) of the
 *                         round's grid (t_start + i T_span, t_start from d_guess as in the safety pass) along its record in
 *                         d_records (normally nep_batch_safety_commit_ent's d_final); each interval is cut into ent_samples
 *                         steps, sampled like Neptune::SamplePointsOfIntervals (nep_ent_sample_points), and all agents move
 *                         at once.  At every step each agent's state takes one nep_ent_track_step (include/neptune_entangle.h):
 *                         its own move and every other agent's, the other agents' bend points from d_records and, at the
 *                         round's FIRST step only (one trajectory message per round), from d_prev as the previous check's
 *                         (an empty list there counts as the current one).  No test stops the update.
 *   d_ent                 [n_scenes][N]: in, the state at this round's A (zeroed = empty); out, at the next round's A — the
 *                         d_ent_init of the next nep_batch_frontend_ent / nep_batch_safety_commit_ent
 *   d_records             [n_scenes][N] (in/out): afterwards every tracked agent's record publishes n_bend = 1 + state.n_bend,
 *                         bend[0] = its base, then the anchors of its bend indices (publishOwnTraj, :457-476); nothing else
 *                         in the record changes
 *   d_flags               [n_scenes][N] (out, may be NULL): the NEP_ENT_TRACK_* bits of the round, ORed over its steps
 * An agent without a valid record (valid, is_agent, n_seg >= 1) is neither tracked nor published.  The active mask does
 * not apply: an inactive agent flies its kept record, and its tether moves with it.  A state that would outgrow
 * NEP_FE_ENT_CAP crossings or NEP_MAX_BEND - 1 bend points, or a step with more than NEP_ENT_TRACK_ADD_CAP new crossings,
 * keeps the state before that step: NEP_ENT_TRACK_CAP in d_flags and NEP_E_CAP from nep_batch_check; nothing is written past
 * the record.  Bit-identical to chaining nep_ent_track_step on the host.  Unsharded handles created with enable_entangle
 * only (else NEP_E_STATE); NEP_E_CAP beyond 4096 agents or 2048 static obstacles per scene.  Asynchronous; the first call
 * allocates per-slot scratch, sized for the largest call, later ones nothing: capturable.
 * A tracked slot's state comes back with id / cs / beta beyond n_alpha and bend beyond n_bend ZEROED (the bytes of a state
 * depend on the state alone, as with nep_batch_fleet_track_ent, whose kernel this call runs); earlier versions left there
 * what the list surgery had left.  Nothing reads those entries.  The debug option fleet_ent_proof applies (same states).
 * (The faithful fleet loop tracks per control tick instead: nep_batch_fleet_track_ent, include/neptune_fleet.h.)
 * With a buffer registered by nep_batch_set_tether_audit (below) every sampled step of a tracked slot is also one tick of the
 * slot's nep_tether_audit, at t_start + q * dt, q = 1..n_intervals * ent_samples; the call's other outputs do not change.       */
int nep_batch_track_ent(nep_batch_t* h, const nep_traj_rec* d_prev, nep_traj_rec* d_records, const nep_guess* d_guess,
                        int32_t n_intervals, int32_t ent_samples, double cable_length, nep_fe_ent_state* d_ent,
                        int32_t* d_flags, void* stream);

/* ---- The tracked state beyond NEP_FE_ENT_CAP crossings: a list form ------------------------------------------------------
 * The reference's updateEntStateStaticObs keeps its list in a std::vector; the fixed record above drops a tracked move that
 * would outgrow NEP_FE_ENT_CAP entries (NEP_ENT_TRACK_CAP) and the state lies behind the tether from then on.  nep_ent_lists
 * is the same state as a struct of arrays with `cap` entries per slot, NEP_FE_ENT_CAP < cap <= NEP_ENT_LISTS_MAX_CAP
 * (else NEP_E_CAP).  The struct itself lives in host memory; its members point to arrays of `slots` = n_scenes * N slots:
 *   n_alpha, n_bend       [slots]
 *   id, cs, beta          [slots][cap]   the crossing list (agent or static id, case, beta: as in nep_fe_ent_state)
 *   bend                  [slots][NEP_MAX_BEND]   indices into the list, 16 bit
 * Entries beyond the counts are zero, on the way in and on the way out: the bytes of a state depend on the state alone.
 * The other two capacities are the fixed record's and the host form's: NEP_MAX_BEND - 1 bend points (a published record
 * holds no more) and NEP_ENT_TRACK_ADD_CAP new crossings per move.  nep_abi_sizeof(23) is the struct's size.                */
#define NEP_ENT_LISTS_MAX_CAP 4096
typedef struct nep_ent_lists {
  int32_t cap;
  int32_t _pad;
  int32_t* n_alpha;
  int32_t* n_bend;
  int16_t* id;
  int8_t* cs;
  double* beta;
  int16_t* bend;
} nep_ent_lists;

/* nep_batch_track_ent on the list form: d_lists (a host struct) names DEVICE arrays, updated in place; everything else —
 * the steps flown, d_prev / d_records / d_guess, the published bend points, d_flags, the validation and its error codes, the
 * first call allocating and later ones being capturable (with the same cap), fleet_ent_proof — is nep_batch_track_ent's.  A move that
 * would outgrow d_lists->cap crossings, NEP_MAX_BEND - 1 bend points or NEP_ENT_TRACK_ADD_CAP new crossings is dropped:
 * NEP_ENT_TRACK_CAP in d_flags, NEP_E_CAP from nep_batch_check.  A slot whose counts or bend indices are out of range on the way
 * in keeps its state and gets NEP_ENT_TRACK_CAP, like a malformed fixed record.  Bit-identical to chaining nep_ent_track_step
 * with state->cap = d_lists->cap.  The working list of a slot sits in LDS: 11 bytes per entry (45 KB at the largest cap).
 * The tether audit (nep_batch_set_tether_audit, below) counts its steps like nep_batch_track_ent's; max_alpha is then the
 * headroom against d_lists->cap.                                                                                            */
int nep_batch_track_ent_lists(nep_batch_t* h, const nep_traj_rec* d_prev, nep_traj_rec* d_records, const nep_guess* d_guess,
                              int32_t n_intervals, int32_t ent_samples, double cable_length, const nep_ent_lists* d_lists,
                              int32_t* d_flags, void* stream);

/* The tether audit (include/neptune_entangle.h: nep_tether_audit).  Registers d_audit, a [n_scenes][N] device
 * buffer holding nep_tether_audit_init's values or an earlier flight's records; d_audit == NULL switches the audit off again.
 * While a buffer is registered, nep_batch_track_ent, nep_batch_track_ent_lists and nep_batch_fleet_track_ent (fixed records and
 * the list form, include/neptune_fleet.h) accumulate one tick per tracked move into it, inside the launch that tracks: tick
 * q = 1.. of a call lies at t0 + (double)q * dt, t0 the scene's t_start as the call reads it from d_guess (between rounds) or the
 * scene's fleet clock (nep_batch_fleet_counters' t_now), and dt the value given here — 0: the call's own step, T_span / ent_samples
 * or the fleet's dc.  A slot the tracking skips (no trajectory, a malformed state or list) audits nothing, and the predictions
 * (nep_batch_fleet_predict_ent, nep_batch_ent_lists_at_a) never audit: they fly nothing.  Equal byte for byte to chaining
 * nep_ent_track_step_audit on the host.  States, flags, bend points and records are those of a call without the audit, and
 * without a registered buffer the step kernels that run are the plain ones.  Synchronises nothing; call it outside a capture (a
 * captured graph keeps the buffer it was captured with).  NEP_E_ARG: dt < 0 or NaN; NEP_E_STATE: a sharded handle.              */
struct nep_tether_audit;
int nep_batch_set_tether_audit(nep_batch_t* h, struct nep_tether_audit* d_audit, double dt);

/* The state at A the front end and the safety re-check take, from the list form, for a loop that tracks between rounds (the
 * fleet's nep_batch_fleet_predict_ent has the same rule, include/neptune_fleet.h): d_ent_a[slot] receives the slot's list as a
 * fixed record where it holds at most NEP_FE_ENT_CAP crossings and d_mask_out[slot] = d_mask_in[slot] (1 with d_mask_in NULL).
 * Where it holds more the slot is HELD: a zeroed record, NEP_ENT_TRACK_HELD in d_flags_a[slot] (may be NULL; else 0),
 * d_held[slot] += 1 (may be NULL) and d_mask_out[slot] = 0 — registered with nep_batch_set_active, the mask takes the slot out of
 * the round's front end, replan and safety pass; it keeps flying its record and nep_batch_track_ent_lists keeps tracking it.
 * d_lists as in nep_batch_track_ent_lists (not changed); a malformed list gives a zeroed record and is not held.  Same handles
 * and error codes as nep_batch_track_ent_lists.  Asynchronous, allocates nothing, capturable.                                   */
int nep_batch_ent_lists_at_a(nep_batch_t* h, const nep_ent_lists* d_lists, nep_fe_ent_state* d_ent_a, int32_t* d_flags_a,
                             const int32_t* d_mask_in, int32_t* d_mask_out, int32_t* d_held, void* stream);

/* Point A of the NEXT round for every slot, on the device: d_start[slot].t_start advances by dt and pos / vel / accel become
 * the state of the agent's committed trajectory (d_records [n_scenes][N], e.g. nep_batch_safety_commit's d_final) at that
 * time — Neptune::replanFull's choice of A "deltaT ahead on the committed plan" (neptune.cpp:1366-1399) for a
 * bulk-synchronous loop in which every agent replans from the same clock.  Evaluated like generatePwpOut's samples
 * (solver_gurobi_poly.cpp:921-929); beyond the trajectory's last knot the vehicle rests at its end point; an agent without a
 * valid record keeps its state.  The goal is left alone unless d_alt_goal ([slots][3], may be NULL) is given: then an agent
 * that has arrived (within switch_radius of its goal, slower than 0.05 m/s) swaps goal and alternate goal, so that a fleet
 * keeps flying back and forth (what bench.py's `moving` leg runs).  Asynchronous on `stream`; with it a whole round
 * (front end -> lines + QP -> safety check + commit -> next point A) is a fixed launch sequence on fixed buffers, i.e. one
 * HIP graph.                                                                                                          */
int nep_batch_next_starts(nep_batch_t* h, const nep_traj_rec* d_records, double dt, nep_fe_start* d_start,
                          double* d_alt_goal, double switch_radius, void* stream);

/* ---- Flight audit: what the fleets actually fly, measured on the device -----------------------------------------------------
 * Every stage above plans; the audit looks at the committed records as a perfect tracker flies them.  For every (scene, agent) it
 * evaluates the records at control ticks and accumulates how close the agent came to every other agent and to every static
 * polygon of its scene, at which tick and to whom.  Only the ticks are looked at — no continuous-time minimum: the loops' perfect
 * tracker (and FleetLoop's host log) is only ever at the control ticks.
 *
 * nep_audit               one entry per (scene, agent); calls ACCUMULATE into it.  Initial values (nep_audit_init): the minima
 *                         and center_d2 +inf, partners and index -1, everything else 0.  nep_abi_sizeof(17) is its size.
 *   min_center_dist, center_partner, t_center   smallest x-y distance between this agent's centre and another agent's; the
 *                         partner as 1-based id; the tick's time
 *   min_box_clear, box_partner, t_box           the planner's own invariant: against agent j,
 *                         max(|dx| - (bbox_j[0]/2 + drone_radius), |dy| - (bbox_j[1]/2 + drone_radius)) — how far this centre
 *                         lies outside j's inflated box (neptune.cpp:340, the box the hull kernels build).  >= 0: the invariant
 *                         held.  Asymmetric when bboxes differ, so every agent keeps its own.
 *   min_static_dist, static_index, t_static     signed x-y distance from the centre to the nearest static polygon (0-based
 *                         index) of the agent's scene AS THE HANDLE HOLDS IT (already inflated by nep_inflate_static, made
 *                         counter-clockwise): negative inside.  >= 0 is the invariant.
 *   path_len              sum of the x-y step lengths between consecutive ticks, added in tick order (over calls too)
 *   max_speed             largest x-y speed at a tick
 *   n_ticks, n_pair_viol, n_static_viol         ticks audited; ticks with a box clearance < 0; ticks with a static distance < 0
 *   center_d2, last_xy    carried from call to call: min_center_dist squared (centre distances are compared squared, with one
 *                         root per call) and the position at the last audited tick (path_len's next step)
 * Ties go to the earlier tick, then to the lower partner id or static index, so a minimum does not depend on the order of
 * evaluation.  Records are evaluated like nep_batch_next_starts does: u clamped to 0 before the first knot, at rest on the end
 * point beyond the last.  A record that is not (valid && is_agent && n_seg >= 1) is not audited and is nobody's partner (the rule
 * of nep_batch_track_ent); the active mask does not apply: an inactive agent flies its kept record and can be hit.
 *
 * nep_audit_records       host form (no HIP call): one scene of n records at t0 + k*tick, k = 0 .. n_ticks-1, accumulated into
 *                         out[n].  static_off / static_xy: the scene's (inflated) polygons in the CSR form of nep_batch_create.
 * nep_batch_audit         device form, bit-identical to the host form.  d_records [n_scenes][N] (e.g. nep_batch_safety_commit's
 *                         d_final); d_start [slots]: a scene's clock is the t_start of its first slot (as the safety pass reads
 *                         d_guess), the value nep_batch_next_starts advances on the device — so a replayed graph audits the right
 *                         stretch with no time written by the host.  The ticks are t_start + k*tick, k = 0 .. n_ticks-1 (n_ticks
 *                         = 0: nothing happens): when a round lasts n_ticks*tick the rounds tile the time axis and no tick counts
 *                         twice.  The call goes after the round's records are final and before nep_batch_next_starts.  The static
 *                         polygons are the handle's (nep_batch_set_scene_statics), no second copy is made.  Unsharded handles
 *                         only (else NEP_E_STATE; enable_entangle is not needed); up to 1024 agents.  Asynchronous on `stream`;
 *                         the FIRST call allocates the handle's per-slot scratch, later ones nothing: capturable, the contract of
 *                         nep_batch_track_ent.
 * (Chained calls reproduce one long call bit for bit when they visit the same tick times as doubles — t0 + k*tick is rounded.) */
typedef struct nep_audit {
  double min_center_dist, t_center;
  double min_box_clear, t_box;
  double min_static_dist, t_static;
  double path_len, max_speed;
  double center_d2, last_xy[2];
  int32_t center_partner, box_partner, static_index;
  int32_t n_ticks, n_pair_viol, n_static_viol;
} nep_audit;
int nep_audit_init(nep_audit* out, int64_t n);
int nep_audit_records(const nep_traj_rec* recs, int32_t n, const int32_t* static_off, const double* static_xy, int32_t n_static,
                      double drone_radius, double t0, double tick, int32_t n_ticks, nep_audit* out);
int nep_batch_audit(nep_batch_t* h, const nep_traj_rec* d_records, const nep_fe_start* d_start, double tick, int32_t n_ticks,
                    nep_audit* d_audit, void* stream);

/* ---- Span audit: the same three clearances between the ticks ----------------------------------------------
 * nep_audit looks at the control ticks; the planner promises its box clearance for every t.  The span audit takes the minima of
 * the centre distance, the box clearance and the signed static distance over the whole closed window
 * [t_start, t_start + n_ticks * tick] of a call — exactly: the records are cubics, so the window is cut at the ticks and at every
 * knot of the records involved, and on each piece the minima lie at its ends or at real roots of polynomials of degree <= 5.
 * Those polynomials only find candidate TIMES; every value is taken by nep_audit's own expressions at the candidate time, so the
 * ticks are among the candidates, evaluated identically: a call's span minimum is <= the minimum nep_audit finds over the same
 * call's ticks, as doubles, and where the tick is the earliest time at which the value is attained, time and partner agree too.
 *
 * nep_span_audit          one entry per (scene, agent); calls ACCUMULATE into it.  Initial values (nep_span_audit_init): the
 *                         minima and center_d2 +inf, partners and index -1, everything else 0.  nep_abi_sizeof(39) is its size.
 *   min_center_dist, center_partner, t_center   as in nep_audit, over the window; the time is the candidate's
 *   min_box_clear, box_partner, t_box           likewise
 *   min_static_dist, static_index, t_static     likewise
 *   center_d2             min_center_dist squared, carried from call to call
 *   span                  seconds audited: the sum of the calls' window lengths
 *   n_spans, n_pair_viol, n_static_viol         calls; calls whose box minimum was < 0; calls whose static minimum was < 0
 *   gap_box, gap_static   the largest amount by which a call's span minimum lay below the minimum over that call's ticks: what
 *                         the tick audit missed
 * A minimum is the least (value, time, partner id or static index), in that order: ties go to the earlier time, then to the lower
 * partner or index; across calls the earlier call keeps a tie.  Records are read by nep_audit's rules (present = valid &&
 * is_agent && n_seg >= 1; at rest before the first knot and beyond the last; x-y only; the active mask does not apply).
 *
 * nep_span_audit_records  host form (no HIP call), the arguments of nep_audit_records; tick must be finite.
 * nep_batch_audit_span    device form, byte-identical to the host form; the contract of nep_batch_audit: a scene's clock is the
 *                         t_start of its first slot in d_start, n_ticks = 0 does nothing, the handle's static polygons are used,
 *                         unsharded handles only (else NEP_E_STATE), asynchronous on `stream` and capturable: the FIRST call
 *                         (n_ticks = 0 will do) sets the kernel's LDS size up, later ones nothing; no call allocates (a wave
 *                         merges its lanes in registers, there is no scratch).  NEP_E_CAP when the scene's agents and polygons
 *                         do not fit into 160 KB of LDS (about 700 agents with 100 four-edge polygons).                       */
typedef struct nep_span_audit {
  double min_center_dist, t_center;
  double min_box_clear, t_box;
  double min_static_dist, t_static;
  double center_d2, span;
  double gap_box, gap_static;
  int32_t center_partner, box_partner, static_index;
  int32_t n_spans, n_pair_viol, n_static_viol;
} nep_span_audit;
int nep_span_audit_init(nep_span_audit* out, int64_t n);
int nep_span_audit_records(const nep_traj_rec* recs, int32_t n, const int32_t* static_off, const double* static_xy, int32_t n_static,
                           double drone_radius, double t0, double tick, int32_t n_ticks, nep_span_audit* out);
int nep_batch_audit_span(nep_batch_t* h, const nep_traj_rec* d_records, const nep_fe_start* d_start, double tick, int32_t n_ticks,
                         nep_span_audit* d_span, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEPTUNE_FRONTEND_H_ */
