// nep_device.h — device-side views shared by the HIP kernels and the host launcher.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "nep_tables.h"
#include "launch_plan.h"
#include "lds_layout.h"
#include "../../include/neptune_frontend.h"
#include "../../include/neptune_fleet.h"
#include "../../include/neptune_entangle.h"
#include "../../include/neptune_backend_debug.h"

namespace nep {

constexpr int kHullV = NEP_HULL_MAX_V;   // 16
constexpr int kHullCP = NEP_HULL_MAX_CP; // 16
constexpr int kBend = NEP_MAX_BEND;      // 8

// Process-wide A/B knobs of the launchers (nep_debug_set_global_option, include/neptune_backend_debug.h): scheduling and placement
// only — results do not depend on them — and never read from the environment (the library behaves the same under any environment).
// One exception, a test hook's: bit 9 of a slot's polish flag word (nep_batch_debug_polish_flags: "the pass read the parked lines back")
// says what polish_impl and parked_bound made the pass do, and so differs with them; every result of a replan is the same.
struct DebugGlobals { bool fe_three = false; int fe_xcd = 1; int polish_grid = 256; int polish_impl = 1; int parked_bound = 1; int hull_sort = 1; };      // (fe_three, fe_xcd: read where a front-end call's facts are filled, backend.hip)
extern DebugGlobals g_debug;

// Scene-level constants (setMaxValues, ctor arguments; solver_gurobi_poly.cpp:25-175)
constexpr int kCorrFromItDefault = 10, kCorrMaxCountDefault = 8;      // (qp_common.h: kCorrFromIt, kCorrMaxCount)
struct SceneParams {
  int num_agents;     // N (pb.size())
  int num_pol;        // planning intervals
  int n_static;       // S
  int n_hull;         // hull lists per scene: N in batch mode, n_obst in per-agent mode
  int ent_enabled;
  int hull_mode;      // 0: pick the hull kernel by batch size; 1: one hull per wave (hull_kernel); 2: eight per wave (hull_group_kernel)
  int max_states;
  int lines_cap;      // capacity of one (slot, segment) line bucket
  int n_local;        // slots per scene
  int first_local;    // index of first local agent (batch); per-agent mode: id-1
  int skip_own;       // 1: hull list is indexed by agent, own entry skipped
  int static_stride;  // 0: one static-obstacle set for every scene; S: scene s reads polygons [s*S, (s+1)*S) (nep_batch_set_scene_statics)
  double T_span, weight, dc, drone_radius;
  double mins[3], maxs[3], v_max, a_max;
  double long_length; // solver_gurobi_poly.cpp:173
  double cull_radius; // > 0: separating lines farther than this from the guess are presolved away (verified after the solve)
  long long time_limit_ticks;   // > 0: wall-clock budget of ONE solve in wall_clock64() ticks (setMaxRuntime -> Gurobi TimeLimit, solver_gurobi_poly.cpp:812)
  int corr_from_it, corr_max_count;      // the interior point's give-up rule (qp_common.h: kCorrFromIt, kCorrMaxCount; NEP_CORR_FROM / NEP_CORR_MAX: development A/B)
  double tol_res, tol_gap, tol_res_inv, tol_gap_inv, tol_gap_floor;      // (tol_gap_floor = 0.1 tol_gap: the centring target's floor)      // the interior point's strict tests: residuals (absolute, the dual one scaled), relative gap; their reciprocals for the merit (nep_batch_set_tolerances)
  int sep_rule;                 // which vertex of the separator LP is returned: 0 the largest-gap one (default), 1 the one a primal simplex of GLPK's default class reaches (nep_batch_set_separator_rule)
  int qp_key_decay;             // the same for the QP workgroups' key (8 us bins; 2: chain QP launch 1.63 -> 1.55 ms, crossing 2.29 -> 2.26; NEP_QP_KEY_DECAY for A/Bs, 0 = the last solve's bin)
  int fe_key_decay;             // front end's launch-order key: bins an old key loses per launch (0: the key is the last search's bin)
  double us_per_tick;           // microseconds per wall_clock64() tick of this device (hipDeviceAttributeWallClockRate; 0.01 on gfx950: 100 MHz)
};

// Buffers of one problem set (n_scenes x n_local slots).  All device pointers.
struct ProblemSet {
  // inputs
  const nep_guess* guess;        // [slots]
  const double* pb;              // [N][2]
  const double* static_xy;       // [S][kHullV][2]   (x n_scenes when sp.static_stride != 0)
  const int* static_nv;          // [S]
  const double* static_el;       // [S][kHullV] length of edge v -> v+1 (the proximity cull's square roots, taken once at upload)
  const int* case_id;            // [slots][NEP_MAX_POL][N] or null
  // per scene (batch: written by the hull kernel; per-agent: uploaded by setHulls)
  double* hull_xy;               // [scenes][n_hull][num_pol][kHullV][2]
  int* hull_nv;                  // [scenes][n_hull][num_pol]
  double* hull0_xy;              // [scenes][N][num_pol][2]  col(0) of the uninflated hull
  int* hull0_nv;                 // [scenes][N][num_pol]
  double* bend_xy;               // [scenes][N][kBend][2]
  int* bend_n;                   // [scenes][N]
  // Sharded hulls (nep_batch_replan_hulls): the six arrays above are the first of N / hull_pb
  // equal blocks, hull_bstride bytes apart, each holding hull_pb agents per scene — the layout an
  // all-gather of per-rank blocks produces.  hull_pb == 0: one block (everything above as stated).
  int hull_pb;
  unsigned long long hull_pb_magic;   // 2^32 / hull_pb + 1 (host): j / hull_pb = (j * magic) >> 32 for j < 65536; 0: divide
  long hull_bstride;
  // separator output
  double* line_nd;               // [slots][NEP_MAX_POL][lines_cap][3]
  int* line_cnt;                 // [slots][NEP_MAX_POL]  lines at the front of the bucket (all of them, or the near ones); -1 - n: the bucket overflowed (line_count())
  int* line_far;                 // [slots][NEP_MAX_POL]  presolved-away lines parked at the back of the bucket, or null
  int* lp_stats;                 // [slots][NEP_MAX_POL][2]  (LPs attempted, LPs without a line) per segment, written by the separator
  // spatial presolve (line presolve on, largest-gap rule, batched hull layout): LPs whose line is known to be far from the guess
  // without solving them are skipped; a replan whose solution does not verify them is listed for the redo pass
  const double* skip_box;        // = fe_box when LPs may be skipped, else null
  int* line_skip;                // [slots][NEP_MAX_POL] LPs skipped per segment, or null
  int* redo_list;                // [slots] replans to solve again with every LP and every row, or null
  int* redo_count;               // [1]
  const int* order_count;        // [1] or null: only the first *order_count workgroups of the QP launch have work (the redo pass)
  int lines_override;            // 1: line buckets were filled by the host (test hook)
  int sep_pack;                  // host only: segments per wave of the presolve's separator — 0 picked by launch size, -1 the unpacked kernel, 1..NEP_MAX_POL forced (nep_batch_debug_set_separator_pack; NEP_SEP_PACK / NEP_SEP_UNPACKED at create)
  const int* order;              // [slots] workgroup -> slot (longest expected solve first, see order_kernel) or null: identity
  int* order_key;                // [slots] this launch's measured device time in 8 us bins (the next launch's ordering key) or null
  // front end: the same for the searches (frontend_kernel: longest expected search first; key bins of 8 us, 256 us with the entangle check)
  const int* fe_order;           // [slots] workgroup -> slot or null: identity
  int* fe_order_key;             // [slots] or null
  float* fe_us;                  // [slots] device time of the last search of every slot, microseconds, or null
  // QP scratch when the row state does not fit LDS
  double* row_scratch;           // [slots or scratch_chunks][11][rows_cap / 4 + 2]
  int scratch_chunks;            // 0: one scratch area per slot.  > 0 (presolve with the redo pass): that many areas, used by the redo pass only, by launch index
  int scratch_by_block;          // 1: this launch addresses the scratch by blockIdx.x (the redo pass)
  int rows_cap;
  int lds_rows;                  // rows that fit the dynamic LDS carve
  int lds_lines;
  // outputs
  nep_solution* solution;        // [slots]
  double* states;                // [slots][max_states][12] or null
  nep_traj_rec* commit;          // [slots] or null
  const nep_traj_rec* prev_commit; // [scenes][N] records before this round, or null: what a failed replan's commit slot carries over
  // active-set polish (qp_polish_kernel.hip): solves that ended without the strict tests leave their last iterate and are listed
  double* polish_z;              // [slots][2][24] last iterate of the first / relaxed solve (axis stride nz), or null: no polish
  int* polish_flag;              // [slots] bit m: mode m's solve ended on the loose snapshot or gave up
  int* polish_list; int* polish_count;      // [slots] listed slots; counters (see qp_polish_kernel)
  int* presolved;                // [slots] 1: the zero-iteration certificate finished this replan (qp_presolve.h: qp_presolve_kernel, or the separator's wave); the interior-point kernel returns at once.  Null: the certificate did not run ahead of that kernel
  // the certificate in the separator's wave: non-null only for a launch of separator_packed_kernel in which one wave holds every segment
  // of a slot, with the line cull on and `presolved` given (Engine::run); the wave then writes presolved[slot] = 0 or 1 for every slot it reaches
  const QpTable* pre_tables;     // the QP tables (indexed by K), or null: the separator makes lines only
  const int* pre_sched_n;        // SampleSched::n (states of the schedule of K)
  long long* dbg;                // [slots][16] phase cycle counters (development aid) or null
  int* flags;                    // [1] sticky NEP_FLAG_* bits raised by the kernels (capacity overflows), or null
  double* fe_box;                // [scenes][num_agents + n_static][num_pol][4] (x0, x1, y0, y1) of the front end's obstacles (fe_box_kernel)
  // active set (nep_batch_set_active): [scenes][num_agents] int32 by GLOBAL agent index, nonzero = the agent replans; null = every slot.
  // Inactive slots never reach the QP or front-end workgroups (they run over active_list_kernel's list: order / order_count, fe_order /
  // fe_count) and the separators return at their first line; skipped_replan_kernel / skipped_fe_kernel write their outputs.
  const int* active;
  const int* fe_count;           // [1] or null: only the first *fe_count workgroups of the front-end launch have work
};
// slot -> is it in the active set (see ProblemSet::active)
__device__ __forceinline__ bool slot_active(const SceneParams& sp, const int* active, int slot) {
  return active == nullptr || active[(long)(slot / sp.n_local) * sp.num_agents + sp.first_local + slot % sp.n_local] != 0;
}
constexpr int NEP_FLAG_FE_ASTAR_ENT_REC = 512;   // nep_batch_frontend_astar_ent: a child's entangle state outgrew the fixed record (list, a step's crossings or bend points; the child was dropped: nep_fe_result.ent_overflow), or a state at A was malformed
constexpr int NEP_FLAG_FE_ASTAR_POOL = 256;   // nep_batch_frontend_astar: a search ran into a node pool smaller than the reference's 20 000 (nep_batch_set_fe_astar's max_nodes): it stopped creating nodes there
constexpr int NEP_FLAG_MISSION = 128;       // nep_batch_fleet_mission: a draw found no goal among max_attempts candidates (the slot kept its goal; NEP_FLEET_FLAG_GOAL)
constexpr int NEP_FLAG_FLEET = 64;           // nep_batch_fleet_commit: an accepted slot's plan or composed trajectory would have outgrown its storage (the slot kept both; NEP_FLEET_CAP)
constexpr int NEP_FLAG_ENT_TRACK = 32;      // nep_batch_track_ent: a tracked state outgrew the fixed record (list, bend points or a step's crossings; the step was dropped) or was handed in malformed
constexpr int NEP_FLAG_ENT_POOL = 16;       // the safety pass's entangle re-check needed a big record and the pool had none left (nep_batch_set_fe_ent_big_records): the trajectory was turned down
constexpr int NEP_FLAG_LINES = 8;           // a segment got more separating lines than its bucket holds (nep_batch_set_line_capacity)
constexpr int NEP_FLAG_SCRATCH = 4;         // more replans went through the presolve's redo pass with rows beyond the register slots than the handle has scratch areas for (nep_batch_reserve_row_scratch)
constexpr int NEP_FLAG_ENT_BETA = 2;        // an entangle state handed to the front end carries a non-zero beta for an agent crossing (the reference's rule makes it 0.0)
constexpr int NEP_FLAG_HULL_OVERFLOW = 1;   // an interval overlapped more committed segments than NEP_HULL_MAX_CP / 4, or its hull has more than NEP_HULL_MAX_V vertices

// a (slot, segment) line count as the separator stores it: n, or -1 - n when the bucket overflowed (the replan then fails)
__host__ __device__ inline int line_count(int stored) { return stored < 0 ? -1 - stored : stored; }
// entry index (scene-major inside its block) and byte offset of the block of agent j's hull data
struct HullRef { long e; long boff; };
__host__ __device__ inline HullRef hull_ref(const ProblemSet& ps, int per_scene, int scene, int j) {
  if (ps.hull_pb <= 0) return HullRef{(long)scene * per_scene + j, 0L};
  // (j / hull_pb by the host's magic number, exact for j, hull_pb < 65536: an integer division is a forty-instruction float
  // sequence on the VALU, and the separator takes a hull reference per candidate)
  const int b = ps.hull_pb_magic ? (int)(((unsigned long long)(unsigned)j * ps.hull_pb_magic) >> 32) : j / ps.hull_pb;
  return HullRef{(long)scene * ps.hull_pb + (j - b * ps.hull_pb), (long)b * ps.hull_bstride};
}
template <typename T> __host__ __device__ inline T* blk(T* base, long boff) { return (T*)((char*)base + boff); }

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a (device, function) pair: the size configured so far is kept
// per device (handles may live on several GPUs of one process) and updated under a lock (handles may be driven from
// several host threads).
struct DynLdsAttr {
  std::mutex mu; size_t configured[64] = {};
  hipError_t ensure(const void* fn, size_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    std::lock_guard<std::mutex> lk(mu);
    if (bytes <= configured[dev]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) configured[dev] = bytes;
    return e;
  }
};

struct SampleSched {             // per K: n, seg[], dt[]
  const int* n;                  // [kMaxK+1]
  const int* seg;                // [kMaxK+1][max_states]
  const double* dt;              // [kMaxK+1][max_states]
};

// grouped: the eight-hulls-per-wave kernel (launch_plan.h: eight_hulls_per_wave).  boxes: that kernel also writes the hulls' boxes (ps.fe_box, entries
// of the agents: what fe_box_kernel would make of them) and zeroes the presolve's redo counters — one hull list per agent of the scene; ord: and
// its block 0 makes the QP launch order (ps.order_key -> ps.order) and zeroes the polish counters.  Both are the launch plan's, with grouped only
void launch_hulls(const nep_traj_rec* recs, int n_scenes, int n_rec, const nep_guess* guess,
                  const SceneParams& sp, const ProblemSet& ps, hipStream_t st, bool grouped, bool boxes = false, bool ord = false);
void launch_hulls_ts(const nep_traj_rec* recs, int n_scenes, int n_rec, const double* ts0, long ts_slot_stride,
                     const SceneParams& sp, const ProblemSet& ps, hipStream_t st, bool grouped, bool boxes = false, bool ord = false);
void launch_hulls_explicit(const nep_traj_rec* recs, int n_traj, double t_start, int num_pol,
                           double T_span, double drone_radius, double* hull_xy, int* hull_nv,
                           double* hull0_xy, int* hull0_nv, int* flags, hipStream_t st);
void launch_separator(int n_slots, const SceneParams& sp, const ProblemSet& ps, int pack, bool cert, hipStream_t st);
void launch_separator_redo(int n_slots, const SceneParams& sp, const ProblemSet& ps, hipStream_t st);
void launch_boxes(int n_scenes, const SceneParams& sp, const ProblemSet& ps, hipStream_t st);
void launch_active_rows(int n_slots, const SceneParams& sp, const ProblemSet& ps, double tol, int* out, hipStream_t st);
void launch_separator_explicit(int n_prob, const int* a_off, const double* a_xy, const int* b_off,
                               const double* b_xy, double* nd, int* solved, int rule, hipStream_t st);
void launch_qp(int n_slots, const SceneParams& sp, const ProblemSet& ps, const QpTable* tables,
               const SampleSched& sched, size_t lds_bytes, hipStream_t st);
size_t qp_lds_fixed_bytes();
// the register-resident placement of the same solver (qp_reg_kernel.hip)
void launch_qp_order(int n_slots, const int* key, int* order, hipStream_t st, int* zero_these = nullptr);      // (zero_these: four ints zeroed on the way, or null)
void launch_qp_polish_zero(int* counters, hipStream_t st);
void launch_order_xcd(int n_slots, const int* key, int* order, hipStream_t st);      // (key may be null: the XCD placement alone; n_slots % 8 == 0)
void launch_qp_reg(int n_slots, const SceneParams& sp, const ProblemSet& ps, QpKernel inst, const QpTable* tables,
                   const SampleSched& sched, size_t lds_bytes, hipStream_t st);
void launch_qp_polish(int n_slots, const SceneParams& sp, const ProblemSet& ps, const QpTable* tables, const SampleSched& sched, hipStream_t st);
void launch_qp_presolve(int n_slots, const SceneParams& sp, const ProblemSet& ps, const QpTable* tables, const SampleSched& sched, int* presolved, hipStream_t st);
int qp_reg_slots();
size_t qp_reg_lds_bytes();
// pool of big records (ent_device.h: a search node's entangle state beyond the fixed record's capacities), claimed by atomic
// increments of *count during a launch; the launch's first kernel zeroes the counter
struct EntBigPool { unsigned char* base; int* count; int n_rec; int rec_bytes; int cap; int add_lim; };
// (mult: 1 for the search, 3 for the safety pass's re-check — entangleCheckGivenPwp prunes at three times the search's bound, kinodynamic_search.cpp:944-948)
__host__ __device__ inline int ent_big_cap(int N, int S, int mult = 1) { int c = (N + S) * mult; if (c < NEP_FE_ENT_CAP) c = NEP_FE_ENT_CAP; return (c + 3) & ~3; }      // (any fixed record can be copied into one)
__host__ __device__ inline int ent_big_add_lim(int N, int S, int mult = 1) { return ((N + S) * mult + 2 + 31) & ~31; }
__host__ __device__ inline int ent_big_rec_bytes(int N, int S, int mult = 1) { const int c = ent_big_cap(N, S, mult), a = ent_big_add_lim(N, S, mult); return (((8 + 13 * c + 3) & ~3) + 4 * a + a / 8 + 7) & ~7; }
// entangle inputs / scratch of the front end and of the safety pass's entangle re-check (device pointers)
struct FeEntArgs {
  const double* sampled;         // [scenes][N][num_pol][ns+1][2]   SampledPtsForAll_ (ent_sample_kernel); with sharded hulls: block 0's
  const int* present;            // [scenes][N]                     (both indexed through hull_ref: they travel in the hull blocks)
  const double* srep;            // [S][2][2] staticObsRep_ (x n_scenes with per-scene statics)
  const double* slong;           // [S][2]    staticObsLongestDist_
  const nep_fe_ent_state* init;  // [slots] entangle state at point A, or null (empty)
  nep_fe_ent_state* nodes;       // [slots][num_pol+1][beam_width] states of the installed nodes
  nep_fe_ent_state* work;        // [scenes * N] one working record per thread of ent_check_kernel
  nep_fe_ent_state* saved;       // [slots][children cap] the state every surviving child of the depth at hand arrived with (fe_sizes' cap)
  double* saved_arc;             // [slots][children cap] and its sampled arc length
  double* st_f; long long* st_vox;      // [slots][children cap] f and voxel key of the children that survive the propagation pass: parked here while the LDS arrays that hold them (s_f, s_vox) are lent to the crossing lists
  int* case_out;                 // [slots][NEP_MAX_POL][N] (out) or null
  int ns;                        // num_sample_per_interval
  double* packed;                // [scenes][N][num_pol][pk_stride] one record per (agent, interval) of what the check reads (ent_pack_kernel), or null
  int pk_stride;
  EntBigPool big;                // front end: where states beyond the fixed record go (base == null: such children are pruned and flagged)
  EntBigPool big_check;          // the same for the safety pass's re-check (records of three times the bound; its counter is zeroed by ent_sample_kernel)
  int big_lds_off;               // big-record instantiation: byte offset, in the dynamic LDS, of its per-thread lists (kEntBigLdsBytes each), or 0: none (the launch's LDS would not hold them) — FeLayout::big_lds_off
  double* big_beta;              // [redo_cap][256][kEntBigLdsCap] betas of those lists
  int* redo_list; int* redo_count; int redo_cap;      // front end: searches in which a child outgrew the fixed record, listed by frontend_kernel<true, W> for frontend_kernel<true, 2, true> (beyond redo_cap: they stay flagged)
  unsigned* xpool; int xpool_stride;      // front end (fast instantiation): per slot, room for the lists of new crossings of a round's (child, step) pairs that do not fit the LDS pool ([slots][xpool_stride] words: kEntAddCap per pair), see cross_round
  int fast_cap, fast_add, fast_bend;      // front end: what the fixed record's path accepts (<= NEP_FE_ENT_CAP, 32, NEP_MAX_BEND; nep_batch_set_fe_ent_fast_caps — the tests shrink them to drive ordinary scenes through the big records)
};
// the best-first front end (fe_astar.h, nep_batch_set_fe_astar): budget, lattice order and the per-slot pools (device pointers)
struct FeAstarArgs {
  int max_pops, pool, tab_cap;   // pops per search; nodes per slot; entries of a slot's voxel table (a power of two >= 2 * pool)
  const int* order;              // [num_samples^2] the lattice order (all_combinations_), or null: 0, 1, 2, ...
  unsigned char* nodes;          // [slots][pool] nodes of NEP_FE_ASTAR_NODE_BYTES
  int* heap;                     // [slots][pool] the open list's heap (its first entries live in LDS)
  unsigned long long* tab_key; int* tab_val;      // [slots][tab_cap] voxel -> first node
};
// the same search with the entangle check (nep_batch_frontend_astar_ent): what it needs beyond FeAstarArgs and FeEntArgs
struct FeAstarEntArgs {
  unsigned* tab_iz;              // [slots][tab_cap] the third word of a voxel's key: getIz of the node's state
  unsigned char* states;         // [slots][pool] a node's entangle state, NEP_FE_ASTAR_ENT_NODE_BYTES each, beside the node pool
};
// one front-end call behind its hull launch, as its plan says (launch_plan.h: plan_frontend); order_buf [slots], active_buf [slots + 1]
void launch_frontend(const FrontendPlan& plan, int n_slots, int n_scenes, const SceneParams& sp, const ProblemSet& ps, const nep_fe_cfg& fc,
                     const FeAstarArgs& aa, const FeAstarEntArgs& xa, const FeEntArgs& ea, const nep_fe_start* starts, nep_guess* guess_out,
                     nep_fe_result* res_out, hipStream_t st, int* order_buf, int* active_buf);
// nep_batch_goal_gate (goal_gate.h): one wave per slot behind a front end; the hulls are the ones ps points at.  case_out
// [slots][NEP_MAX_POL][N] and count [n_scenes][4] may be null
void launch_goal_gate(int n_slots, const SceneParams& sp, const ProblemSet& ps, double half_side, const nep_fe_start* starts, nep_guess* guess,
                      nep_fe_result* res, int* case_out, int* count, hipStream_t st);
// nep_batch_guess_fallback / _tally (guess_fallback_kernels.hip): one wave per slot behind the replan — a NEP_FAILED slot with a usable
// guess gets the guess's record in `commit` and status NEP_GUESS; one wave per scene after nep_batch_fleet_commit.  count [n_scenes][4]
// (null allowed in the first)
void launch_guess_fallback(int n_slots, const SceneParams& sp, const double* pb, const nep_guess* guess, nep_solution* sol, nep_traj_rec* commit,
                           int* count, hipStream_t st);
void launch_guess_fallback_tally(int n_scenes, int n_local, const nep_solution* sol, const int* outcome, int* count, hipStream_t st);
void launch_ent_sample(const nep_traj_rec* recs, int n_scenes, int N, const double* ts0, long ts_scene_stride, int num_pol, int ns, double T_span,
                       double* sampled, int* present, hipStream_t st, int* zero_this = nullptr);
// nep_batch_audit (audit_kernels.hip): the minima of one (scene, run of ticks, agent), ticks as indices of the call
struct AuditPart { double c_d2, box, stat; int c_k, c_p, b_k, b_p, s_k, s_i, n_pair, n_stat; };
struct AuditArgs {
  int N, S, n_scenes, static_stride, vstride, n_ticks, chunk_len, n_chunks;
  double tick, drone_radius;
  const nep_traj_rec* recs;      // [scenes][N]
  const nep_fe_start* starts;    // [scenes][N]: a scene's clock is its first slot's t_start
  const double* static_xy;       // [scenes or 1][S][kHullV][2]
  const int* static_nv;          // [scenes or 1][S]
  AuditPart* part;               // [scenes][n_chunks][N] scratch
  nep_audit* out;                // [scenes][N] accumulated into
};
void launch_audit(const AuditArgs& aa, hipStream_t st);
// nep_batch_audit_span (audit_span_kernels.hip): the span audit of every (scene, agent), one wave per agent
struct SpanAuditArgs {
  int N, S, n_scenes, static_stride, vstride, n_ticks;
  double tick, drone_radius;
  const nep_traj_rec* recs;      // [scenes][N]
  const nep_fe_start* starts;    // [scenes][N]: a scene's clock is its first slot's t_start
  const double* static_xy;       // [scenes or 1][S][kHullV][2]
  const int* static_nv;          // [scenes or 1][S]
  nep_span_audit* out;           // [scenes][N] accumulated into
};
long long span_audit_lds_bytes(int N, int S, int vstride);
hipError_t prepare_audit_span(long long lds_bytes);
void launch_audit_span(const SpanAuditArgs& sa, hipStream_t st);
// nep_batch_fleet_* (fleet_kernels.hip, include/neptune_fleet.h): the committed plans of every slot.  All device pointers.
struct FleetArgs {
  int N, n_scenes, cap, max_states;
  nep_fleet_cfg cfg;
  double drone_radius;
  const double* pb;              // [N][2]
  // state of the slots and of the scenes (owned by the handle)
  double* ring;                  // [slots][cap][12]
  int* head; int* size; int* k_end;      // [slots]
  double* state;                 // [slots][12]
  double* goal;                  // [slots][3]
  nep_pwp* pwp;                  // [slots]
  int* flown; int* done; int* outcome; int* sflags;      // [slots]
  const int* period; const int* phase;   // [slots] or both null
  double* t_now; int* round;     // [scenes]
  int* origin;                   // [scenes] the scene's index in the flight it comes from (its own, until a restore says otherwise): the mission generator's global slot
  int* counters;                 // [scenes][NEP_FLEET_N_COUNTERS]
  int* gflags;                   // sticky NEP_FLAG_FLEET
  // select
  nep_fe_start* start; nep_traj_rec* recs; int* active_out; nep_fe_start* clock;
  // commit
  const nep_solution* sol; const double* states_in; const nep_fe_result* fres; const int* accept; int* outcome_out;
  const int* active;             // the handle's mask ([scenes][N]) or null
};
void launch_fleet_seed(const FleetArgs& fa, const double* state0, hipStream_t st);
void launch_fleet_select(const FleetArgs& fa, hipStream_t st);
void launch_fleet_commit(const FleetArgs& fa, hipStream_t st);
void launch_fleet_tick(const FleetArgs& fa, hipStream_t st);
// the mission controller of the fleet state (fleet_mission_kernels.hip): nep_batch_fleet_mission.  Goals, done and the slots' sticky
// flags are FleetArgs'; everything else is the handle's mission state.  All device pointers.
struct FleetMissionArgs {
  nep_mission_cfg cfg;
  size_t lds_bytes;              // mission_layout's bytes for the handle's agents and the largest keep-out set
  double* t_issue; double* length; int* completed;      // [slots]
  int* counts;                   // [slots][4]: issued, reached, timed out, no goal
  double* sums;                  // [slots][2]: leg time, leg length
  int* scene_i;                  // [scenes][4]: run index, runs succeeded, runs failed, finished
  double* t_run;                 // [scenes]
  nep_mission_leg* log; int* log_n;      // [owners][log_cap], [owners]: owners = slots (mode PER_AGENT) or scenes
  const int* kn;                 // [scenes] keep-out polygons of the scene
  const int* koff;               // [scenes][NEP_MISSION_MAX_POLY + 1]
  const double* kxy;             // [scenes][NEP_MISSION_MAX_VERT][2]
  const double* script;          // [slots][*script_n][3] the scripted goals (nep_batch_fleet_mission_script), or null: never uploaded
  const int* script_n;           // [1] rows per slot now (0: off); read when the kernel runs, so a replaced table reaches a captured round
};
void launch_fleet_mission_seed(const FleetMissionArgs& ma, const FleetArgs& fa, hipStream_t st);
void launch_fleet_mission(const FleetMissionArgs& ma, const FleetArgs& fa, hipStream_t st);
// the move-back rule (fleet_moveback_kernels.hip): nep_batch_fleet_moveback.  State, bases, clocks and the slots' flags are FleetArgs',
// fa.start the round's start records; t_issue is the mission state's [slots], or null (every goal was issued at fa.cfg.t0)
void launch_fleet_moveback(const nep_moveback_cfg& c, const FleetArgs& fa, const double* t_issue, hipStream_t st);
// the effort record (fleet_effort_kernels.hip): nep_batch_fleet_effort.  Rings, heads, sizes and done flags are FleetArgs'; out [slots]
void launch_fleet_effort(const FleetArgs& fa, double v_max, double a_max, double j_max, double slack, nep_fleet_effort* out, hipStream_t st);
// the fleet recorder (fleet_recorder_kernels.hip): nep_batch_fleet_snapshot / _snapshot_ring / _restore.  Section i of a scene block
// (recorder_common.h) is the scene's part — `bytes` bytes — of the handle's array `p`, at `off` in the block.  All device pointers.
struct RecorderSection { char* p; long off; unsigned bytes; unsigned pad_; };
struct RecorderArgs {
  nep_fleet_snapshot_hdr hdr;    // what the snapshot kernel writes in front (hdr.n_scenes: the handle's)
  int n_entries;                 // 0: a plain blob; > 0: a ring, scene s goes to entry round[s] mod n_entries
  int src_scene, dst_scene;      // restore: block src_scene of the blob into scene dst_scene (-1, -1: every scene into its own)
  int parts;                     // workgroups that share a scene
  const int* round; const int* origin;      // [scenes] the handle's (the ring's entry and stamp)
  char* blob;                    // the blob or ring (16-byte aligned)
  RecorderSection sec[NEP_SNAPSHOT_N_SECTIONS];
};
void launch_fleet_snapshot(const RecorderArgs& ra, hipStream_t st);
void launch_fleet_restore(const RecorderArgs& ra, hipStream_t st);
// the tethers' entangle states (tether_kernels.hip): nep_batch_track_ent between two rounds; on the fleet state nep_batch_fleet_select's
// bend points, _predict_ent, _track_ent
struct TetherArgs {
  int N, S, n_scenes, static_stride, num_pol;
  int n_steps;                   // moves of the call: n_intervals * ns (between rounds), round_ticks (the fleet's tracking) or 1 (prediction)
  int proof;                     // 0: every other agent and static is walked at every step (debug option fleet_ent_proof)
  int skip_absent;               // 1 (between rounds): a slot whose own record holds no trajectory gets flags 0 and keeps its state
  int ns;                        // with `sampled`: steps per interval
  double cable, T_span;
  const double* pb;              // [N][2]
  const double* srep;            // [scenes or 1][S][2][2]
  const double* slong;           // [scenes or 1][S][2]
  double* pos;                   // [slots][n_steps + 1][2] scratch: every slot's positions of the call (tether_pos_kernel)
  const double* sampled;         // between rounds: [slots][num_pol][ns + 1][2], every record on the round's grid (ent_sample_kernel); else null
  const nep_fe_start* start;     // prediction: [slots] point A and the clock; null: tracking
  const nep_traj_rec* recs;      // [slots] the records published this round
  nep_traj_rec* recs_out;        // the publish kernels: the records the bend points are published into
  int* pub_n; double* pub_xy;              // [slots], [slots][NEP_MAX_BEND][2] the list published at the last select
  int* pub_prev_n; double* pub_prev_xy;    // and the one before it (the fleet's publish kernel rotates the two)
  // the step kernel: every slot's bend list at the previous check, count and points a byte stride apart — the fleet's pub_prev_*, or
  // the previous round's records between rounds; null for a prediction
  const char* prev_n; const char* prev_xy; long prev_n_stride, prev_xy_stride;
  const nep_fe_ent_state* in;    // [slots] the state at the tracked position
  nep_fe_ent_state* out;         // [slots] tracking: the same buffer; prediction: the state at A
  nep_fe_ent_state* save;        // [slots] scratch: the state before a step that may outgrow the record
  // the list form (tether_step_lists_kernel, the publish kernels): lists.cap != 0 = the state is there, not in `in` — tracked in place;
  // a prediction reads it and writes the fixed record at A into `out`
  nep_ent_lists lists;           // device arrays, [slots] and [slots][cap]
  nep_ent_lists lsave;           // scratch of the same form (id, cs, beta, bend; the counts stay in registers)
  int* held;                     // [slots] prediction in the list form: rounds the slot's state at A did not fit the fixed record, or null
  int* hold_mask;                // [slots] ... the round's active mask, cleared for such a slot, or null
  int* flags;                    // [slots] NEP_ENT_TRACK_* bits of the call
  int* ever;                     // [slots] sticky OR (the fleet's tracking) or null
  int* walked;                   // [slots] (other agent, step) pairs walked, accumulated (the fleet's tracking) or null
  int* counters;                 // [scenes][NEP_FLEET_N_COUNTERS]: [7] = slots ever flagged NEP_ENT_TRACK_ENTANGLED
  int* gflags;                   // sticky NEP_FLAG_ENT_TRACK
  // the tether audit (nep_batch_set_tether_audit): null = off, the plain step kernels run.  Else [slots] records the tracking calls
  // accumulate one tick per move into; tick q = 1..n_steps of a call lies at t0 + (double)q * audit_dt, t0 the scene's clock
  // *(const double*)(audit_t0 + scene * audit_t0_stride).  A prediction never audits.
  nep_tether_audit* audit; const char* audit_t0; long audit_t0_stride; double audit_dt;
};
bool fleet_ent_fits(int N, int S);
void launch_tether_publish(const TetherArgs& ea, bool fleet, hipStream_t st);      // (fleet: nep_batch_fleet_select's contract, else nep_batch_track_ent's)
void launch_ent_lists_at_a(const TetherArgs& ea, const int* mask_in, hipStream_t st);      // (reads lists, n_scenes, N; writes out, flags, held, hold_mask)
void launch_tether_steps(const TetherArgs& ea, const FleetArgs& fa, hipStream_t st);      // (fa: read by the fleet's two position modes only)
void launch_ent_check(const SceneParams& sp, const ProblemSet& ps, const FeEntArgs& ea, const nep_traj_rec* fresh, int n_scenes, double cable, int* entangles, hipStream_t st);
void launch_next_starts(const nep_traj_rec* recs, int n_scenes, int N, int first_local, int n_local, double dt, nep_fe_start* starts,
                        double* alt, double r_switch, hipStream_t st);
void launch_gjk_explicit(int n_prob, const int* a_off, const double* a_xy, const double* b_xy, int* hit, hipStream_t st);
void launch_safety(const nep_traj_rec* prev, const nep_traj_rec* fresh, int n_scenes, int N, const SceneParams& sp, const ProblemSet& ps,
                   unsigned char* conflict, unsigned char* conflict_prev, const int* entangles, nep_traj_rec* final_out, int* accept_out, hipStream_t st,
                   const int* active = nullptr);      // (active: the inactive agents are accepted before the id-ordered pass, ProblemSet::active)
// active set (ProblemSet::active): the compacted list of the active slots, in the order of `order_in` (null: slot order), with the count
// at list[n_slots]; zero_these (four ints or null) are zeroed on the way.  One workgroup, no host synchronisation.
void launch_active_list(int n_slots, const SceneParams& sp, const int* active, const int* order_in, int* list, int* zero_these, hipStream_t st);
// the outputs of the inactive slots of a replan (d_solution: NEP_SKIPPED; d_commit: the previous record when ps.prev_commit is known)
void launch_skipped_replan(int n_slots, const SceneParams& sp, const ProblemSet& ps, hipStream_t st);
// the records the safety pass judges: recs[s][j] = active ? fresh : prev
void launch_select_records(int n_scenes, int N, const int* active, const nep_traj_rec* prev, const nep_traj_rec* fresh, nep_traj_rec* out, hipStream_t st);

}  // namespace nep
