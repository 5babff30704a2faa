// backend.hip — host side of the C ABI declared in include/neptune_backend.h.
//
// Owns device memory, tables and launch sequencing; all arithmetic of the path runs in the HIP
// kernels (geom_kernels.hip, qp_kernels.hip).  There is no CPU fallback: without a HIP device
// every compute entry point returns NEP_E_HIP.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "nep_device.h"
#include "qp_outputs.h"
#include "audit_common.h"
#include "mission_common.h"
#include "effort_common.h"
#include "moveback_common.h"
#include "recorder_common.h"
#include "../../include/neptune_plan.h"
#include "../../include/neptune_entangle.h"
#include "../../include/neptune_hastar.h"
#include "../../include/neptune_mtlp.h"

using namespace nep;

namespace nep { DebugGlobals g_debug; }

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(NEP_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define HIPCHK_NULL(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_err = std::string(#x) + ": " + hipGetErrorString(e_); return nullptr; } } while (0)

// bytes the process's DevBufs and PinnedArenas hold right now (nep_debug_live_bytes: what the ownership tests read)
std::atomic<long long> g_live_device{0}, g_live_pinned{0};

// Device memory with one owner: the destructor frees, a move hands the memory over, there is no copy.
template <class T> struct DevBuf {
  T* p = nullptr; size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
  ~DevBuf() { release(); }
  int ensure(size_t count) {
    if (count <= n && p) return 0;
    release();
    if (count == 0) count = 1;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) { p = nullptr; g_err = std::string("hipMalloc: ") + hipGetErrorString(e); return NEP_E_HIP; }
    n = count; g_live_device += (long long)(n * sizeof(T));
    return 0;
  }
  void release() { if (p) { hipFree(p); g_live_device -= (long long)(n * sizeof(T)); } p = nullptr; n = 0; }
};

// The list form of the tracked tether states (nep_ent_lists) in device memory: `slots` slots of `cap` entries
struct ListBuf {
  DevBuf<int> n_alpha, n_bend; DevBuf<int16_t> id, bend; DevBuf<int8_t> cs; DevBuf<double> beta; int cap = 0;
  int ensure(size_t slots, int cap_) {
    if (int e = n_alpha.ensure(slots)) return e;
    if (int e = n_bend.ensure(slots)) return e;
    if (int e = id.ensure(slots * cap_)) return e;
    if (int e = cs.ensure(slots * cap_)) return e;
    if (int e = beta.ensure(slots * cap_)) return e;
    if (int e = bend.ensure(slots * NEP_MAX_BEND)) return e;
    cap = cap_;
    return 0;
  }
  nep_ent_lists view() const { nep_ent_lists v{}; v.cap = cap; v.n_alpha = n_alpha.p; v.n_bend = n_bend.p; v.id = id.p; v.cs = cs.p; v.beta = beta.p; v.bend = bend.p; return v; }
};

// Page-locked host memory (the per-agent handle's staging arenas: one DMA in, one out per replan), owned like a DevBuf.  Growth keeps
// the contents.
struct PinnedArena {
  char* p = nullptr; size_t n = 0;
  PinnedArena() = default;
  PinnedArena(const PinnedArena&) = delete;
  PinnedArena& operator=(const PinnedArena&) = delete;
  PinnedArena(PinnedArena&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  PinnedArena& operator=(PinnedArena&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
  ~PinnedArena() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= n && p) return 0;
    char* q = nullptr;
    hipError_t e = hipHostMalloc((void**)&q, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) { g_err = std::string("hipHostMalloc: ") + hipGetErrorString(e); return NEP_E_HIP; }
    if (p) std::memcpy(q, p, n);
    if (bytes > n) std::memset(q + n, 0, bytes - n);
    release();
    p = q; n = bytes; g_live_pinned += (long long)(bytes ? bytes : 1);
    return 0;
  }
  void release() { if (p) { hipHostFree(p); g_live_pinned -= (long long)(n ? n : 1); } p = nullptr; n = 0; }
};

constexpr size_t kLdsBudget = 150 * 1024;  // of the 160 KiB per CU

// The separator treats hull lists and static obstacles as counter-clockwise convex polygons (only their edges are
// candidate lines and the polygon's own rows hold by convexity, geom_kernels.hip::separator_impl) — the order CGAL's
// convex_hull_2 and setStaticObst produce.  The reference LP itself is order-independent (separator_glpk.cpp:248-373),
// so anything a caller may legally pass is brought to that form at upload: clockwise input is reversed (the first
// vertex stays first: col(0) feeds the proximity cull, solver_gurobi_poly.cpp:559), non-convex input is refused.
// Returns false for a polygon that is not convex.
bool normalize_ccw(double* xy, int n) {
  if (n < 3) return true;
  double area2 = 0, scale = 0;
  for (int v = 0; v < n; v++) {
    const double* a = xy + 2 * v; const double* b = xy + 2 * ((v + 1) % n);
    area2 += a[0] * b[1] - a[1] * b[0];
    scale = std::fmax(scale, std::fmax(std::fabs(a[0]), std::fabs(a[1])));
  }
  if (area2 < 0) for (int lo = 1, hi = n - 1; lo < hi; lo++, hi--) { std::swap(xy[2 * lo], xy[2 * hi]); std::swap(xy[2 * lo + 1], xy[2 * hi + 1]); }
  const double tol = 1e-9 * (1.0 + scale) * (1.0 + scale);
  for (int v = 0; v < n; v++) {
    const double* o = xy + 2 * v; const double* a = xy + 2 * ((v + 1) % n); const double* b = xy + 2 * ((v + 2) % n);
    if ((a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0]) < -tol) return false;
  }
  return true;
}

// wall_clock64() ticks per second of the current device (the constant-rate counter behind nep_stats.solve_us, the launch
// order's keys and the TimeLimit emulation): 100 MHz on gfx950, asked of the runtime rather than assumed
double wall_clock_hz() {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0) return (double)khz * 1e3;
  return 1e8;
}

// Everything both handle kinds share: tables, scratch and the launch sequence of one replan.
struct Engine {
  SceneParams sp{};
  int n_scenes = 1;
  DevBuf<QpTable> d_tables;
  DevBuf<int> d_sched_n, d_sched_seg; DevBuf<double> d_sched_dt;
  DevBuf<double> d_pb, d_static_xy, d_static_el; DevBuf<int> d_static_nv;
  DevBuf<double> d_hull_xy, d_hull0_xy, d_bend_xy, d_line_nd, d_row_scratch;
  DevBuf<int> d_hull_nv, d_hull0_nv, d_bend_n, d_line_cnt, d_line_far, d_lp_stats;
  DevBuf<int> d_presolved; bool presolve_kernel = true, presolve_fused = true;      // the zero-iteration certificate's marks (one per slot); debug option "presolve_kernel" = 0: the test runs inside qp_reg_kernel<true> as in rounds 3-5; "presolve_fused" = 0: always as qp_presolve_kernel, never in the separator's wave
  DevBuf<int> d_line_skip, d_redo_list, d_redo_count;   // spatial presolve: skipped LPs per segment, replans listed for the redo pass
  DevBuf<double> d_polish_z; DevBuf<int> d_polish_flag, d_polish_list, d_polish_count; bool polish = true, polish_presolve = true;      // the active-set polish of solves that end without the strict tests (qp_polish_kernel.hip; nep_*_set_polish)
  DevBuf<long long> d_dbg; bool profile_phases = false;
  DevBuf<int> d_flags;
  // entangle-aware front end / safety re-check (nep_batch_frontend_ent, nep_batch_safety_commit_ent)
  DevBuf<double> d_sampled, d_srep, d_slong; DevBuf<int> d_present, d_entangles;
  DevBuf<nep_fe_ent_state> d_fe_nodes, d_fe_work, d_fe_saved; DevBuf<double> d_fe_arc, d_fe_packed; bool have_reps = false;
  // big records of the entangle-aware front end (ent_device.h): a pool per handle, 0 = the default budget (4 per slot, at least 4 096)
  DevBuf<double> d_fe_big_beta, d_fe_stf; DevBuf<long long> d_fe_stvox; DevBuf<unsigned> d_fe_xpool;
  DevBuf<unsigned char> d_fe_big, d_fe_big_check; DevBuf<int> d_fe_big_count, d_fe_big_check_count; long fe_big_records = 0;
  int fe_fast_cap = NEP_FE_ENT_CAP, fe_fast_add = 32, fe_fast_bend = NEP_MAX_BEND;
  DevBuf<unsigned char> d_conflict, d_conflict_prev;
  bool safety_check_prev = false;
  int lds_lines = 0, lds_rows = 0, rows_cap = 0; size_t lds_bytes = 0;
  DevBuf<double> d_fe_box;          // boxes of the front end's obstacles, made before every search launch
  DevBuf<int> d_fe_order, d_fe_order_key; DevBuf<float> d_fe_us; bool fe_history = false, fe_lpt = true;      // the same for the front end's searches (frontend_kernel)
  DevBuf<int> d_order, d_order_key; bool have_history = false, lpt = true;   // QP workgroups launched longest-expected-first (order_kernel)
  const int* active = nullptr;       // the active set (nep_batch_set_active): device [scenes][N], or null
  // the best-first front end (nep_batch_set_fe_astar): per-slot node pools, heaps and voxel tables; the budget and the lattice order
  DevBuf<unsigned char> d_as_nodes; DevBuf<int> d_as_heap, d_as_val, d_as_order; DevBuf<unsigned long long> d_as_key;
  DevBuf<unsigned> d_as_iz; DevBuf<unsigned char> d_as_states;      // nep_batch_frontend_astar_ent: the voxel key's third word, the nodes' entangle states
  bool as_ready = false; int as_max_pops = 0, as_pool = 0, as_tab = 0, as_n_order = 0;
  int as_team = 1, as_team_last = 0;      // nep_batch_set_fe_astar_team: waves per search of nep_batch_frontend_astar_ent; what its last call launched (0: none yet)
  DevBuf<int> d_act, d_fe_act;       // [slots + 1] compacted active slots + count (active_list_kernel): the QP launches', the front end's
  ListBuf d_track_lsave;      // nep_batch_track_ent_lists: the same scratch in the list form, of the largest cap seen
  DevBuf<nep_fe_ent_state> d_track_save; DevBuf<int> d_track_flags; DevBuf<double> d_track_pos;      // nep_batch_track_ent: per-slot scratch, flags when the caller passes none, the positions of the largest call
  DevBuf<AuditPart> d_audit_part;      // nep_batch_audit: per (scene, run of ticks, agent) minima, sized once for the most runs a call can have
  int static_nv_max = 0;               // most vertices of a static polygon uploaded so far (nep_batch_audit's LDS stride)
  DevBuf<nep_traj_rec> d_safety_recs;      // [scenes][N] the records an active-set safety pass judges (select_records_kernel)
  bool use_reg = false;        // the QP runs as qp_reg_kernel (row state in registers, four workgroups per CU)
  double clock_hz = 1e8;       // wall_clock64() rate of the handle's device (set_clock)
  // (the short-step give-up rule's two numbers: run-time values for A/B, nep_*_debug_set_option "corr_from" / "corr_max"; never read from the environment)
  void set_clock() { clock_hz = wall_clock_hz(); sp.us_per_tick = 1e6 / clock_hz; sp.corr_from_it = opt_corr_from; sp.corr_max_count = opt_corr_max; if (!(sp.tol_res > 0.0)) { sp.tol_res = 1e-10; sp.tol_gap = 1e-11; sp.tol_res_inv = 1e10; sp.tol_gap_inv = 1e11; sp.tol_gap_floor = 0.1 * 1e-11; } }      // (called by both create paths: the strict tests' defaults with it)
  double sched_dc = -1, tab_T = -1, tab_w = -1; int sched_cap = 0;
  std::vector<int> h_sched_n, h_sched_seg; std::vector<double> h_sched_dt;
  // timing
  bool timing = false; std::vector<hipEvent_t> ev; size_t ev_used = 0;

  int build_tables() {
    if (tab_T == sp.T_span && tab_w == sp.weight && d_tables.p) return 0;
    std::vector<QpTable> t(2 * (kMaxK + 1));
    std::memset(t.data(), 0, t.size() * sizeof(QpTable));
    for (int mode = 0; mode < 2; mode++) for (int K = 1; K <= kMaxK; K++) build_qp_table(K, sp.T_span, sp.weight, mode, &t[mode * (kMaxK + 1) + K]);
    if (int e = d_tables.ensure(t.size())) return e;
    HIPCHK(hipMemcpy(d_tables.p, t.data(), t.size() * sizeof(QpTable), hipMemcpyHostToDevice));
    tab_T = sp.T_span; tab_w = sp.weight;
    return 0;
  }
  int build_schedule(double dc, int cap) {
    if (dc == sched_dc && cap == sched_cap && d_sched_n.p) return 0;
    h_sched_n.assign(kMaxK + 1, 0); h_sched_seg.assign((size_t)(kMaxK + 1) * cap, 0); h_sched_dt.assign((size_t)(kMaxK + 1) * cap, 0.0);
    for (int K = 1; K <= kMaxK; K++) h_sched_n[K] = build_sample_schedule(K, sp.T_span, dc, cap, &h_sched_seg[(size_t)K * cap], &h_sched_dt[(size_t)K * cap]);
    if (int e = d_sched_n.ensure(h_sched_n.size())) return e;
    if (int e = d_sched_seg.ensure(h_sched_seg.size())) return e;
    if (int e = d_sched_dt.ensure(h_sched_dt.size())) return e;
    HIPCHK(hipMemcpy(d_sched_n.p, h_sched_n.data(), h_sched_n.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_sched_seg.p, h_sched_seg.data(), h_sched_seg.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_sched_dt.p, h_sched_dt.data(), h_sched_dt.size() * sizeof(double), hipMemcpyHostToDevice));
    sched_dc = dc; sched_cap = cap; sp.max_states = cap; sp.dc = dc;
    return 0;
  }
  // which interior-point kernel the next replan launches, and its LDS carve (see size_scratch)
  static constexpr double kAutoCullRadius = 4.0;
  bool fits_reg = true, cull_user_set = false, skip_lps = true, no_redo = false; int lds_lines_lds = 0, sep_pack = 0, force_kernel = 0, opt_qp_key_decay = 2, opt_fe_key_decay = 1, opt_corr_from = kCorrFromItDefault, opt_corr_max = kCorrMaxCountDefault, opt_fleet_ent_proof = 1;      // (skip_lps, no_redo, sep_pack, force_kernel: development aids behind nep_*_debug_set_option, include/neptune_backend_debug.h)
  // Row scratch (rows and coefficients beyond the register slots / the LDS carve): one area per slot in general.  With the presolve's
  // redo pass (skip_mode(), launch_plan.h) the first pass never needs one — a replan whose near lines exceed the slots is sent to the redo pass —
  // so the handle keeps a pool of kScratchPool areas for that pass (config 5: 1.9 GB instead of 15.3 per 32 scenes);
  // nep_batch_reserve_row_scratch asks for the worst case.
  static constexpr int kScratchPool = 1024;
  bool scratch_full = false; int scratch_chunks = 0;
  // The static polygons' entries of d_fe_box ([scene][N + S][num_pol][4]: one box per polygon, the same in every interval) are written
  // from the host at every upload and whenever the buffer or its layout changes — never by a launch of run(), which may be recorded
  // into a graph and not execute — so that a replan without fe_box_kernel (the fused hull launch, eager or replayed) reads the boxes of
  // the polygons now uploaded.  static_boxes_ok: they are in place (push_static_boxes).
  std::vector<double> h_static_box;      // [n_scenes][S][4] (x0, x1, y0, y1) of the polygons now uploaded
  const double* box_buf = nullptr; int box_N = -1, box_S = -1, box_np = -1;      // the buffer and layout they were written into
  bool static_boxes_ok = false;
  bool static_boxes_placed() const { return static_boxes_ok && box_buf == d_fe_box.p && box_N == sp.num_agents && box_S == sp.n_static && box_np == sp.num_pol; }
  // the boxes fe_box_kernel makes of n packed polygons (min / max over the vertices: the same doubles on the host) -> out [n][4]
  static void static_boxes_of(int n, const std::vector<double>& sx, const std::vector<int>& nv, double* out) {
    for (int j = 0; j < n; j++) {
      const double* q = &sx[(size_t)j * kHullV * 2];
      double x0 = HUGE_VAL, x1 = -HUGE_VAL, y0 = HUGE_VAL, y1 = -HUGE_VAL;
      if (nv[j] > 0) { x0 = x1 = q[0]; y0 = y1 = q[1]; }
      for (int v = 1; v < nv[j]; v++) { x0 = std::fmin(x0, q[2 * v]); x1 = std::fmax(x1, q[2 * v]); y0 = std::fmin(y0, q[2 * v + 1]); y1 = std::fmax(y1, q[2 * v + 1]); }
      out[4 * j] = x0; out[4 * j + 1] = x1; out[4 * j + 2] = y0; out[4 * j + 3] = y1;
    }
  }
  // h_static_box -> the static entries of d_fe_box: every scene, or scene `scene` alone when the buffer and layout are those of the last
  // write.  Blocking (a copy from pageable memory); without a buffer of the full size yet it writes nothing (size_scratch calls again).
  int push_static_boxes(int scene = -1) {
    const bool placed = static_boxes_placed();
    static_boxes_ok = false;
    const int N = sp.num_agents, S = sp.n_static, np = sp.num_pol;
    const size_t row = (size_t)(N + S) * np * 4, blk = (size_t)S * np * 4;
    if (!d_fe_box.p || d_fe_box.n < (size_t)n_scenes * row || h_static_box.size() < (size_t)n_scenes * S * 4) return 0;
    if (S > 0) {
      const int s0 = (scene >= 0 && placed) ? scene : 0, s1 = (scene >= 0 && placed) ? scene + 1 : n_scenes;
      std::vector<double> b((size_t)(s1 - s0) * blk);
      for (int s = s0; s < s1; s++)
        for (int j = 0; j < S; j++)
          for (int i = 0; i < np; i++) std::memcpy(&b[(((size_t)(s - s0) * S + j) * np + i) * 4], &h_static_box[((size_t)s * S + j) * 4], 4 * sizeof(double));
      HIPCHK(hipMemcpy2D(d_fe_box.p + (size_t)s0 * row + (size_t)N * np * 4, row * sizeof(double), b.data(), blk * sizeof(double), blk * sizeof(double), (size_t)(s1 - s0), hipMemcpyHostToDevice));
    }
    box_buf = d_fe_box.p; box_N = N; box_S = S; box_np = np; static_boxes_ok = true;
    return 0;
  }
  ReplanPlan last_plan;        // what the last run() launched (launch_plan.h; the nep_batch_debug_launch_* and _polish_* calls read it)
  int lines_cap_user = 0;      // 0: the default budget; -1: the reference's worst case; n > 0: n lines per segment (nep_batch_set_line_capacity)
  // what the launch plan reads of the handle (launch_plan.h); run() adds the call's own facts
  ReplanFacts facts() const {
    ReplanFacts f;
    f.num_agents = sp.num_agents; f.num_pol = sp.num_pol; f.n_hull = sp.n_hull; f.n_static = sp.n_static; f.ent_enabled = sp.ent_enabled;
    f.hull_mode = sp.hull_mode; f.skip_own = sp.skip_own; f.sep_rule = sp.sep_rule; f.cull_radius = sp.cull_radius;
    f.use_reg = use_reg; f.lpt = lpt; f.have_history = have_history; f.presolve_kernel = presolve_kernel; f.presolve_fused = presolve_fused;
    f.skip_lps = skip_lps; f.no_redo = no_redo; f.statics_boxy = statics_boxy; f.static_boxes_ok = static_boxes_ok; f.sep_pack = sep_pack;
    f.polish = polish; f.polish_presolve = polish_presolve; f.polish_buffers = d_polish_z.p != nullptr;
    f.n_scenes = n_scenes; f.slots = n_scenes * sp.n_local;
    f.order_ok = d_order.n >= (size_t)f.slots; f.order_key_ok = d_order_key.n >= (size_t)f.slots; f.presolved_ok = d_presolved.n >= (size_t)f.slots;
    f.scratch_chunks = scratch_chunks;
    return f;
  }
  int size_row_scratch() {
    const long slots = (long)n_scenes * sp.n_local;
    const bool pooled = skip_mode(facts()) && !scratch_full && slots > kScratchPool;
    scratch_chunks = pooled ? kScratchPool : 0;
    return d_row_scratch.ensure((size_t)(pooled ? kScratchPool : slots) * (11L * (rows_cap / 4 + 2)));
  }
  void choose_placement() {
    use_reg = fits_reg || sp.cull_radius > 0.0;
    if (force_kernel == 1) use_reg = true; else if (force_kernel == 2) use_reg = false;      // (nep_*_debug_set_option "qp_kernel": tests, A/B)
    if (use_reg) { lds_lines = NEP_MAX_POL * 8 * qp_reg_slots(); lds_rows = 4 * lds_lines; lds_bytes = qp_reg_lds_bytes(); }
    else { lds_lines = lds_lines_lds; lds_rows = 4 * lds_lines; lds_bytes = qp_lds_fixed_bytes() + (size_t)(lds_lines + 2) * 11 * 8; }   // + the dummy line of the padded row groups
  }
  // sizes the scratch for (n_scenes x n_local) slots with sp.n_hull hull lists per scene
  int size_scratch() {
    const int N = sp.num_agents, np = sp.num_pol;
    const long slots = (long)n_scenes * sp.n_local;
    // Lines a segment's bucket holds.  The reference's worst case is one line per other agent's hull, per base, per static and per
    // (agent, bend segment) pair of the entangle rows — n_hull + N + S + 8 N.  The last term is by far the largest (2 048 of 2 660 at
    // config 5) and an entangle line needs an ACTIVE case for that agent and segment, which a tenth of the pairs have in the
    // survey's scenes: by default the buckets budget 2 N entangle lines per segment (config 5: 1 124 instead of 2 660, 1.8 GB
    // instead of 4.2 per 32 scenes).  A segment that gets more is flagged (nep_batch_check: NEP_E_CAP), never written past its
    // bucket; nep_batch_set_line_capacity(h, -1) restores the worst case, (h, n) sets n.
    const int worst_lines = sp.n_hull + N + sp.n_static + (sp.ent_enabled ? N * kBend : 0);
    if ((long)NEP_MAX_POL * worst_lines > 65535) return fail(NEP_E_CAP, "more than 65535 separator candidates per agent");
    sp.lines_cap = lines_cap_user < 0 ? worst_lines : (lines_cap_user > 0 ? lines_cap_user : sp.n_hull + N + sp.n_static + (sp.ent_enabled ? std::min(N * kBend, std::max(2 * N, 64)) : 0));
    if (sp.lines_cap > worst_lines) sp.lines_cap = worst_lines;
    if (sp.lines_cap < 8) sp.lines_cap = 8;
    const long lines_total = (long)NEP_MAX_POL * sp.lines_cap;
    // LDS carve of the QP kernel: 11 doubles per line (n1, n2, h + 4 x (s, lambda)).  The worst case
    // (every base and every obstacle close to every segment) almost never happens, so the carve is
    // sized for the expected count and the rest spills to global scratch; when the expectation
    // fits half a CU's LDS two workgroups share a CU.
    const size_t fixed = qp_lds_fixed_bytes();
    const long per_line = 11 * 8;
    const long l_half = ((long)(160 * 1024 / 2) - (long)fixed) / per_line - 2;
    const long l_full = ((long)kLdsBudget - (long)fixed) / per_line - 2;
    // expected lines per segment: every other agent's hull, plus a few nearby bases / statics / entangle lines
    const long expect = (long)NEP_MAX_POL * (sp.n_hull + 4 + sp.n_static / 8 + (sp.ent_enabled ? sp.num_agents / 8 : 0));
    long ll = expect <= l_half ? l_half : l_full;
    if (ll > lines_total) ll = lines_total;
    lds_lines_lds = (int)((ll + 1) & ~1L);
    // Placement of the row state.  When the expected lines per segment fit the register slots of qp_reg_kernel (8 per slot;
    // a few more only cost a trip through the global scratch) the row state lives in registers and four workgroups share a
    // CU.  Bigger problems (config 5: ~260 lines per segment) get the verified line presolve by default (kAutoCullRadius,
    // nep_batch_set_line_cull): the few dozen near lines fit the register slots, the parked ones are checked at the solution,
    // and only a replan that violates one is solved again with every row, the rows beyond the slots going through the per-slot
    // global scratch.  With the presolve turned off (radius 0) such problems keep the LDS placement of qp_kernel.
    // nep_*_debug_set_option(h, "qp_kernel", 1 | 2) overrides the choice (tests, A/B).
    fits_reg = expect / NEP_MAX_POL <= 8L * qp_reg_slots() + 8;
    // The verified line presolve is the handle's default at EVERY size (round 6; until then only where the lines did not fit the
    // register slots): it is what the reference's solver does inside optimize() (Gurobi's presolve drops redundant rows before the
    // barrier, solver_gurobi_poly.cpp:823), its result is the full problem's optimum by construction (parked lines and skipped LPs
    // are verified at the solution, a replan that fails the verification is solved again with every row), and the polish pass runs
    // under it by default, so that one handle has one optimum whatever path its solves take.  nep_batch_set_line_cull(h, 0) turns it off.
    if (!cull_user_set) sp.cull_radius = kAutoCullRadius;
    sp.fe_key_decay = opt_fe_key_decay; sp.qp_key_decay = opt_qp_key_decay;      // (nep_*_debug_set_option "qp_key_decay" / "fe_key_decay": A/B)
    // (the keys remember — a new key is the maximum of the measured bin and the old key less a decay — so a fresh buffer starts at zero;
    // only a fresh one: the per-agent handle sizes its scratch on every replan and a memset there was 30 us of its 100)
    if (lpt) { if (int e = d_order.ensure((size_t)slots)) return e; const int* was = d_order_key.p; if (int e = d_order_key.ensure((size_t)slots)) return e; if (d_order_key.p != was) hipMemset(d_order_key.p, 0, d_order_key.n * sizeof(int)); }
    if (lpt) { if (int e = d_fe_order.ensure((size_t)slots)) return e; const int* was = d_fe_order_key.p; if (int e = d_fe_order_key.ensure((size_t)slots)) return e; if (d_fe_order_key.p != was) hipMemset(d_fe_order_key.p, 0, d_fe_order_key.n * sizeof(int)); }
    if (int e = d_fe_us.ensure((size_t)slots)) return e;
    choose_placement();
    rows_cap = 4 * (int)lines_total; rows_cap = (rows_cap + 3) & ~3;
    if (int e = d_hull_xy.ensure((size_t)n_scenes * sp.n_hull * np * kHullV * 2)) return e;
    if (int e = d_fe_box.ensure((size_t)n_scenes * (N + (sp.n_static > 0 ? sp.n_static : 0)) * np * 4)) return e;
    if (!static_boxes_placed()) { if (int e = push_static_boxes()) return e; }      // (a new buffer or another layout)
    if (int e = d_hull_nv.ensure((size_t)n_scenes * sp.n_hull * np)) return e;
    if (int e = d_hull0_xy.ensure((size_t)n_scenes * N * np * 2)) return e;
    if (int e = d_hull0_nv.ensure((size_t)n_scenes * N * np)) return e;
    if (int e = d_bend_xy.ensure((size_t)n_scenes * N * kBend * 2)) return e;
    if (int e = d_bend_n.ensure((size_t)n_scenes * N)) return e;
    if (int e = d_line_nd.ensure((size_t)slots * lines_total * 3)) return e;
    if (int e = d_line_cnt.ensure((size_t)slots * NEP_MAX_POL)) return e;
    if (int e = d_line_far.ensure((size_t)slots * NEP_MAX_POL)) return e;
    if (int e = d_lp_stats.ensure((size_t)slots * NEP_MAX_POL * 2)) return e;   // per (slot, segment): LPs attempted, LPs without a line
    if (int e = d_line_skip.ensure((size_t)slots * NEP_MAX_POL)) return e;
    if (int e = d_redo_list.ensure((size_t)slots)) return e;
    if (int e = d_presolved.ensure((size_t)slots)) return e;
    if (!d_redo_count.p) { if (int e = d_redo_count.ensure(4)) return e; HIPCHK(hipMemset(d_redo_count.p, 0, 4 * sizeof(int))); }      // [0] listed replans, [1] parked line violated, [2] moved beyond the radius
    if (!d_flags.p) { if (int e = d_flags.ensure(1)) return e; HIPCHK(hipMemset(d_flags.p, 0, sizeof(int))); }
    if (int e = d_polish_z.ensure((size_t)slots * 2 * 24)) return e;
    if (int e = d_polish_flag.ensure((size_t)slots)) return e;
    if (int e = d_polish_list.ensure((size_t)slots)) return e;
    if (!d_polish_count.p) { if (int e = d_polish_count.ensure(8)) return e; HIPCHK(hipMemset(d_polish_count.p, 0, 8 * sizeof(int))); }
    if (!profile_phases) profile_phases = getenv("NEP_QP_PROFILE") != nullptr;      // (profiling only: the per-phase cycle counters of make PROFILE=1; also nep_*_debug_set_option "qp_profile")
    if (profile_phases) { if (int e = d_dbg.ensure((size_t)slots * 32)) return e; }      // (the QP kernels use 16 per slot, the front end 32)
    if (int e = size_row_scratch()) return e;
    return 0;
  }
  void fill(ProblemSet& ps) {
    ps.pb = d_pb.p; ps.static_xy = d_static_xy.p; ps.static_nv = d_static_nv.p; ps.static_el = d_static_el.p;
    ps.hull_xy = d_hull_xy.p; ps.hull_nv = d_hull_nv.p; ps.hull0_xy = d_hull0_xy.p; ps.hull0_nv = d_hull0_nv.p;
    ps.bend_xy = d_bend_xy.p; ps.bend_n = d_bend_n.p;
    ps.fe_order = nullptr; ps.fe_order_key = (lpt && fe_lpt && d_fe_order_key.n >= (size_t)n_scenes * (size_t)sp.n_local) ? d_fe_order_key.p : nullptr; ps.fe_us = d_fe_us.p;
    ps.line_nd = d_line_nd.p; ps.line_cnt = d_line_cnt.p; ps.lp_stats = d_lp_stats.p;
    ps.line_far = sp.cull_radius > 0.0 ? d_line_far.p : nullptr;
    const ReplanFacts f = facts();
    const bool skip = can_skip_lps(f);      // (launch_plan.h, as pol below)
    ps.scratch_chunks = skip_mode(f) ? scratch_chunks : 0; ps.scratch_by_block = 0;
    ps.skip_box = skip ? d_fe_box.p : nullptr; ps.line_skip = skip ? d_line_skip.p : nullptr;
    ps.redo_list = skip ? d_redo_list.p : nullptr; ps.redo_count = skip ? d_redo_count.p : nullptr; ps.order_count = nullptr;
    ps.sep_pack = sep_pack;
    ps.row_scratch = d_row_scratch.p; ps.rows_cap = rows_cap; ps.lds_rows = lds_rows; ps.lds_lines = lds_lines;
    ps.dbg = profile_phases ? d_dbg.p : nullptr;
    ps.presolved = nullptr; ps.pre_tables = nullptr; ps.pre_sched_n = nullptr;      // (run() gives them to the launches of a sequence in which the zero-iteration certificate goes first)
    ps.flags = d_flags.p;
    ps.fe_box = d_fe_box.p;
    ps.active = active; ps.fe_count = nullptr;
    const bool pol = polish_armed(f);
    ps.polish_z = pol ? d_polish_z.p : nullptr; ps.polish_flag = pol ? d_polish_flag.p : nullptr;
    ps.polish_list = pol ? d_polish_list.p : nullptr; ps.polish_count = pol ? d_polish_count.p : nullptr;
  }
  // packs n polygons into the fixed-stride device layout (vertices, vertex counts, edge lengths)
  bool statics_boxy = true;      // every static polygon uploaded so far has an edge on each side of its bounding box (see pack_statics)
  int pack_statics(int n, const int32_t* off, const double* xy, std::vector<double>& sx, std::vector<int>& nv, std::vector<double>& el) {
    sx.assign((size_t)(n > 0 ? n : 1) * kHullV * 2, 0.0); nv.assign(n > 0 ? n : 1, 0);
    for (int j = 0; j < n; j++) {
      int c = off[j + 1] - off[j];
      if (c > kHullV) return fail(NEP_E_CAP, "static obstacle with more than NEP_HULL_MAX_V vertices");
      if (c < 0) return fail(NEP_E_ARG, "static obstacle offsets must not decrease");
      nv[j] = c;
      if (c > static_nv_max) static_nv_max = c;
      for (int v = 0; v < c; v++) { sx[((size_t)j * kHullV + v) * 2] = xy[2 * (off[j] + v)]; sx[((size_t)j * kHullV + v) * 2 + 1] = xy[2 * (off[j] + v) + 1]; }
      if (!normalize_ccw(&sx[(size_t)j * kHullV * 2], c)) return fail(NEP_E_ARG, "static obstacle polygon is not convex");
      // The spatial presolve skips the LP of an obstacle whose BOX is far (box_far, geom_kernels.hip): sound only when every side of
      // the box carries an edge of the polygon — true of inflated statics and interval hulls (hulls of axis-aligned squares), not of
      // an arbitrary convex polygon (a diamond's nearest edge line can lie at 0.71 of the box distance).  One polygon without that
      // property turns LP skipping off for the handle (parked lines and the zero-iteration test stay: they evaluate real lines).
      if (c > 0) {
        const double* q = &sx[(size_t)j * kHullV * 2];
        double lo[2] = {q[0], q[1]}, hi[2] = {q[0], q[1]};
        for (int v = 1; v < c; v++) for (int a = 0; a < 2; a++) { lo[a] = std::min(lo[a], q[2 * v + a]); hi[a] = std::max(hi[a], q[2 * v + a]); }
        const double tol = 1e-9 * (1.0 + (hi[0] - lo[0]) + (hi[1] - lo[1]));
        for (int a = 0; a < 2; a++) {
          int n_lo = 0, n_hi = 0;
          for (int v = 0; v < c; v++) { n_lo += q[2 * v + a] - lo[a] <= tol; n_hi += hi[a] - q[2 * v + a] <= tol; }
          if (n_lo < 2 || n_hi < 2) statics_boxy = false;
        }
      }
    }
    // edge lengths for the proximity cull (solver_gurobi_poly.cpp:566-572), the same IEEE operations the kernel used to
    // repeat per candidate: squares, one sum, sqrt (no contraction: three separate roundings)
    el.assign(sx.size() / 2, 0.0);
    for (int j = 0; j < n; j++)
      for (int v = 0; v + 1 < nv[j]; v++) {
        const double* q = &sx[((size_t)j * kHullV + v) * 2];
        volatile double ex = q[2] - q[0], ey = q[3] - q[1];
        volatile double a = ex * ex, b = ey * ey;
        volatile double c = a + b;
        el[(size_t)j * kHullV + v] = std::sqrt(c);
      }
    return 0;
  }
  int upload_statics(int n, const int32_t* off, const double* xy) {
    static_boxes_ok = false;
    std::vector<double> sx, el; std::vector<int> nv;
    statics_boxy = true;       // (a new shared set replaces every earlier polygon)
    if (int e = pack_statics(n, off, xy, sx, nv, el)) return e;
    if (int e = d_static_xy.ensure(sx.size())) return e;
    if (int e = d_static_el.ensure(el.size())) return e;
    if (int e = d_static_nv.ensure(nv.size())) return e;
    HIPCHK(hipMemcpy(d_static_el.p, el.data(), el.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_static_xy.p, sx.data(), sx.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_static_nv.p, nv.data(), nv.size() * sizeof(int), hipMemcpyHostToDevice));
    sp.n_static = n; sp.static_stride = 0;
    h_static_box.resize((size_t)n_scenes * n * 4);      // (the shared set: the same boxes in every scene)
    for (int s = 0; s < n_scenes; s++) static_boxes_of(n, sx, nv, &h_static_box[(size_t)s * n * 4]);
    if (n_scenes > 0 && sp.num_agents > 0 && sp.num_pol > 0)      // (the front end's obstacle boxes: one per agent or static polygon and interval)
      if (int e = d_fe_box.ensure((size_t)n_scenes * (sp.num_agents + n) * sp.num_pol * 4)) return e;
    return push_static_boxes();
  }
  // One static-obstacle set per scene (same polygon count S in every scene): the first call replicates the handle's
  // shared set into [n_scenes][S] arrays, then scene `scene` gets its own polygons.
  int upload_scene_statics(int scene, int n, const int32_t* off, const double* xy) {
    const int S = sp.n_static;
    if (n != S) return fail(NEP_E_ARG, "every scene must have the handle's n_static polygons");
    if (S == 0) return 0;
    std::vector<double> sx, el; std::vector<int> nv;
    if (int e = pack_statics(n, off, xy, sx, nv, el)) return e;
    if (sp.static_stride == 0) {
      DevBuf<double> nxy, nel; DevBuf<int> nnv;
      if (int e = nxy.ensure((size_t)n_scenes * S * kHullV * 2)) return e;
      if (int e = nel.ensure((size_t)n_scenes * S * kHullV)) return e;
      if (int e = nnv.ensure((size_t)n_scenes * S)) return e;
      for (int s = 0; s < n_scenes; s++) {
        HIPCHK(hipMemcpy(nxy.p + (size_t)s * S * kHullV * 2, d_static_xy.p, (size_t)S * kHullV * 2 * sizeof(double), hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(nel.p + (size_t)s * S * kHullV, d_static_el.p, (size_t)S * kHullV * sizeof(double), hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(nnv.p + (size_t)s * S, d_static_nv.p, (size_t)S * sizeof(int), hipMemcpyDeviceToDevice));
      }
      d_static_xy = std::move(nxy); d_static_el = std::move(nel); d_static_nv = std::move(nnv);
      sp.static_stride = S;
      // the entangle check's representatives (nep_batch_set_static_reps) are indexed like the polygons: one set per scene from
      // now on.  A set uploaded while the statics were shared is replicated; every scene can then be given its own.
      if (have_reps && d_srep.p && d_srep.n >= (size_t)S * 4 && d_slong.n >= (size_t)S * 2) {
        DevBuf<double> nr, nl;
        if (int e = nr.ensure((size_t)n_scenes * S * 4)) return e;
        if (int e = nl.ensure((size_t)n_scenes * S * 2)) return e;
        for (int s = 0; s < n_scenes; s++) {
          HIPCHK(hipMemcpy(nr.p + (size_t)s * S * 4, d_srep.p, (size_t)S * 4 * sizeof(double), hipMemcpyDeviceToDevice));
          HIPCHK(hipMemcpy(nl.p + (size_t)s * S * 2, d_slong.p, (size_t)S * 2 * sizeof(double), hipMemcpyDeviceToDevice));
        }
        d_srep = std::move(nr); d_slong = std::move(nl);
      } else have_reps = false;
    }
    HIPCHK(hipMemcpy(d_static_xy.p + (size_t)scene * S * kHullV * 2, sx.data(), (size_t)S * kHullV * 2 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_static_el.p + (size_t)scene * S * kHullV, el.data(), (size_t)S * kHullV * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_static_nv.p + (size_t)scene * S, nv.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice));
    static_boxes_of(S, sx, nv, &h_static_box[(size_t)scene * S * 4]);
    return push_static_boxes(scene);
  }
  hipEvent_t next_event() {
    if (ev_used == ev.size()) { hipEvent_t e; hipEventCreate(&e); ev.push_back(e); }
    return ev[ev_used++];
  }
  // separator + QP (+ hulls when recs != nullptr) on `st`
  // phases: 1 = the geometry half (hulls, boxes, separating lines into the handle's scratch), 2 = the QP half on the lines that are there,
  // 3 = both (nep_batch_replan); the halves of one round may be enqueued on different streams, ordered by the caller (nep_batch_replan_lines)
  // The launch topology is plan_replan's (launch_plan.h: every condition and its reason); here the facts are copied out, the plan is
  // followed in order, and each launch's ProblemSet is derived from the caller's (`base`, as fill() and the caller made it) and the plan.
  int run(const nep_traj_rec* d_recs, int n_rec, const ProblemSet& base, hipStream_t st, int phases = 3) {
    ReplanFacts f = facts();
    f.n_rec = n_rec; f.phases = phases; f.hull_pb = base.hull_pb; f.have_recs = d_recs != nullptr; f.lines_override = base.lines_override != 0;
    f.active = base.active != nullptr;
    const ReplanPlan plan = plan_replan(f);
    const int slots = f.slots;
    SampleSched sc{d_sched_n.p, d_sched_seg.p, d_sched_dt.p};
    last_plan = record_of(plan, last_plan);
    if (timing) hipEventRecord(next_event(), st);
    if (plan.hulls) {      // (fused_order: the launch order and the polish counters' zeroes come out of the launch's block 0)
      ProblemSet ph = base;
      if (plan.fused_order) { ph.order = d_order.p; ph.order_key = d_order_key.p; }
      launch_hulls(d_recs, n_scenes, n_rec, ph.guess, sp, ph, st, plan.grouped_hulls, plan.fused_boxes, plan.fused_order);
    }
    if (timing) hipEventRecord(next_event(), st);
    if (plan.grow_scratch) {
      scratch_full = true;
      HIPCHK(hipStreamSynchronize(st));
      if (int e = size_row_scratch()) return e;
    }
    // the geometry half's set: no skipped LPs with lines from the host
    ProblemSet pg = base;
    pg.row_scratch = d_row_scratch.p;
    if (!plan.skip) { pg.skip_box = nullptr; pg.line_skip = nullptr; pg.redo_list = nullptr; pg.redo_count = nullptr; }
    if (plan.box_kernel) launch_boxes(n_scenes, sp, pg, st);
    if (plan.separator) {      // (the certificate in its wave: the marks, the tables, and the keys, which decay for the slots it certifies)
      ProblemSet psep = pg;
      if (plan.certificate == kCertWave) { psep.presolved = d_presolved.p; psep.pre_tables = d_tables.p; psep.pre_sched_n = d_sched_n.p; psep.order_key = plan.keyed ? d_order_key.p : nullptr; }
      launch_separator(slots, sp, psep, plan.sep_pack, plan.certificate == kCertWave, st);
    }
    if (timing) hipEventRecord(next_event(), st);
    if (!plan.qp) { if (timing) hipEventRecord(next_event(), st); HIPCHK(hipGetLastError()); return 0; }
    if (plan.order_kernel) launch_qp_order(slots, d_order_key.p, d_order.p, st, pg.polish_count);
    if (plan.polish_zero) launch_qp_polish_zero(pg.polish_count, st);
    if (plan.active_list) {
      if (int e = d_act.ensure((size_t)slots + 1)) return e;
      launch_active_list(slots, sp, pg.active, plan.ordered_qp ? d_order.p : nullptr, d_act.p, pg.polish_count, st);      // (zeroes the polish counters as well: a one-workgroup launch whose slot is inactive does not)
    }
    // the QP half's set: the keys, the certificate's marks, and the workgroup -> slot order (the active list, the launch order, or slot order)
    ProblemSet pq = pg;
    pq.presolved = plan.certificate != kCertNone ? d_presolved.p : nullptr;
    pq.order_key = plan.keyed ? d_order_key.p : nullptr;
    pq.order = plan.active_list ? d_act.p : plan.ordered_qp ? d_order.p : nullptr;
    pq.order_count = plan.active_list ? d_act.p + slots : nullptr;
    if (plan.active_list) launch_skipped_replan(slots, sp, pq, st);
    if (plan.certificate == kCertKernel) launch_qp_presolve(slots, sp, pq, d_tables.p, sc, d_presolved.p, st);      // one wave per replan
    if (plan.qp_kernel == kQpLds) launch_qp(slots, sp, pq, d_tables.p, sc, lds_bytes, st);
    else launch_qp_reg(slots, sp, pq, plan.qp_kernel, d_tables.p, sc, lds_bytes, st);
    if (plan.redo_pass) {
      launch_separator_redo(slots, sp, pq, st);
      ProblemSet pr = pq;      // every row, no parked lines, no marks; over the redo list
      pr.line_far = nullptr; pr.line_skip = nullptr; pr.order = d_redo_list.p; pr.order_count = d_redo_count.p;      // (lists active slots only: no other slot ran)
      pr.presolved = nullptr;      // (every listed replan is solved again, whatever the presolve kernel marked)
      pr.scratch_by_block = pq.scratch_chunks > 0 ? 1 : 0;
      launch_qp_reg(slots, sp, pr, kQpReg, d_tables.p, sc, lds_bytes, st);
    }
    if (plan.polish_pass) launch_qp_polish(slots, sp, pq, d_tables.p, sc, st);
    have_history = plan.have_history;
    if (timing) hipEventRecord(next_event(), st);
    HIPCHK(hipGetLastError());
    return 0;
  }
  ~Engine() { for (auto e : ev) hipEventDestroy(e); }      // (the buffers free themselves)
};

bool grouped_hulls(const SceneParams& sp, int n_scenes, int n_rec) { return eight_hulls_per_wave(sp.num_pol, sp.hull_mode, n_scenes, n_rec); }      // (the hull launches outside run(): the same rule, launch_plan.h)
bool have_device() { int n = 0; return hipGetDeviceCount(&n) == hipSuccess && n > 0; }


__global__ void sample_kernel(const nep_solution* __restrict__ sol, int K, const int* __restrict__ seg, const double* __restrict__ dt, int ns, double* __restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ns) return;
  sample_state(&sol->coeff[0][0][0], seg[s], dt[s], out + (long)s * NEP_STATE_DOUBLES);
}

// Test hook behind both debug line readers: the lines of one slot in row order — per segment the lines at the front of the
// bucket (all of them, or with the presolve on the near ones) and then the parked far ones, which the separator writes from
// the back of the bucket in order of appearance.  LPs without a separating line left (0, 0, 0) and are skipped.
int read_lines(Engine& E, size_t slot, int n_seg, int32_t cap, int32_t* seg, double* nd, int32_t* n_out) {
  std::vector<int> cnt(NEP_MAX_POL), far(NEP_MAX_POL, 0); std::vector<double> buf((size_t)NEP_MAX_POL * E.sp.lines_cap * 3);
  HIPCHK(hipMemcpy(cnt.data(), E.d_line_cnt.p + slot * NEP_MAX_POL, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (E.sp.cull_radius > 0.0) HIPCHK(hipMemcpy(far.data(), E.d_line_far.p + slot * NEP_MAX_POL, far.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(buf.data(), E.d_line_nd.p + slot * NEP_MAX_POL * E.sp.lines_cap * 3, buf.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int& c : cnt) c = line_count(c);      // (an overflowed bucket's count is stored as -1 - n)
  // (a slot no separator has written yet — inactive under an active set since the handle was made — holds whatever the allocation
  // held: the counts are kept inside the bucket, so that this reader never leaves its copy of it)
  const int lc = E.sp.lines_cap > 0 ? E.sp.lines_cap : 0;
  for (int s = 0; s < NEP_MAX_POL; s++) {
    cnt[s] = cnt[s] < 0 ? 0 : cnt[s] > lc ? lc : cnt[s];
    far[s] = far[s] < 0 ? 0 : far[s] > lc - cnt[s] ? lc - cnt[s] : far[s];
  }
  int n = 0;
  for (int s = 0; s < n_seg && s < NEP_MAX_POL; s++)
    for (int c = 0; c < cnt[s] + far[s]; c++) {
      const size_t q = c < cnt[s] ? (size_t)c : (size_t)E.sp.lines_cap - 1 - (size_t)(c - cnt[s]);
      const double* e = &buf[((size_t)s * E.sp.lines_cap + q) * 3];
      if (e[0] == 0.0 && e[1] == 0.0 && e[2] == 0.0) continue;   // LP without a separating line
      if (n < cap) { seg[n] = s; for (int k = 0; k < 3; k++) nd[3 * n + k] = e[k]; }
      n++;
    }
  *n_out = n;
  return 0;
}

}  // namespace

// =================================================================================================
// per-agent handle
// =================================================================================================
// One replan through this handle is ONE host-to-device copy, two kernels (separator, QP with generatePwpOut's samples in its
// tail) and ONE device-to-host copy: the setters write straight into a page-locked arena whose layout the device mirrors,
//   [guess][hull vertex counts: cap x num_pol][entangle block: cases, col(0) of the uninflated hulls, bend points][hull vertices: used],
// (the copy ends with the vertices of the hull lists actually set; the entangle block travels only after setEntStateVector),
// and the solution comes back together with its sampled states.  neptune.cpp:1504-1528 is the call sequence this serves.
struct InLayout { size_t guess, nv, cas, h0xy, h0nv, bend, bendn, xy, cap_end; };
static InLayout in_layout(int N, int np, int cap) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  InLayout L{};
  size_t o = 0;
  L.guess = o; o = up(o + sizeof(nep_guess));
  L.nv = o; o = up(o + (size_t)cap * np * sizeof(int));
  L.cas = o; o = up(o + (size_t)NEP_MAX_POL * N * sizeof(int));
  L.h0xy = o; o = up(o + (size_t)N * np * 2 * sizeof(double));
  L.h0nv = o; o = up(o + (size_t)N * np * sizeof(int));
  L.bend = o; o = up(o + (size_t)N * kBend * 2 * sizeof(double));
  L.bendn = o; o = up(o + (size_t)N * sizeof(int));
  L.xy = o; o = up(o + (size_t)cap * np * kHullV * 2 * sizeof(double));
  L.cap_end = o;
  return L;
}
struct nep_backend {
  Engine eng;
  nep_backend_cfg cfg{};
  std::vector<double> pb;
  double max_runtime = 0.05, tether = 0, j_max = 0;
  bool have_bounds = false, have_init = false, have_hulls = false, solved = false;
  nep_guess guess{}; std::vector<double> guess_times;
  int n_obst = 0;
  PinnedArena hin, hout; DevBuf<char> d_in, d_out;
  int in_cap = 0; InLayout L{};                 // hull lists the arenas are laid out for
  bool have_h0 = false, have_ent = false, states_fresh = false;
  int override_n = -1; std::vector<int> ov_seg; std::vector<double> ov_nd;
  nep_solution h_sol{}; nep_stats stats{};
  hipStream_t stream = nullptr;
  ~nep_backend() { if (stream) hipStreamDestroy(stream); }      // (work a failed call left on it still completes; the buffers free themselves after this, and hipFree synchronizes)
  // (re)lays the input arena out for `cap` hull lists, keeping what the setters have written
  int lay_out(int cap) {
    const int N = cfg.num_agents, np = cfg.num_pol;
    if (cap <= in_cap && hin.p) return 0;
    if (cap < 8) cap = 8;
    const InLayout nl = in_layout(N, np, cap);
    PinnedArena fresh;
    if (int e = fresh.ensure(nl.cap_end)) return e;
    std::memset(fresh.p, 0, nl.cap_end);
    if (hin.p) {
      std::memcpy(fresh.p + nl.guess, hin.p + L.guess, sizeof(nep_guess));
      std::memcpy(fresh.p + nl.nv, hin.p + L.nv, (size_t)in_cap * np * sizeof(int));
      std::memcpy(fresh.p + nl.cas, hin.p + L.cas, L.xy - L.cas);                    // the whole entangle block (same sizes: they depend on N only)
      std::memcpy(fresh.p + nl.xy, hin.p + L.xy, (size_t)in_cap * np * kHullV * 2 * sizeof(double));
    }
    hin = std::move(fresh); L = nl; in_cap = cap;
    return d_in.ensure(nl.cap_end);
  }
  template <class T> T* in(size_t off) { return (T*)(hin.p + off); }
};

extern "C" {

const char* nep_last_error(void) { return g_err.c_str(); }
const char* nep_version(void) { return "neptune-amd-backend 0.1 (gfx950)"; }

nep_backend_t* nep_backend_create(const nep_backend_cfg* cfg) {
  if (!cfg || !cfg->pb) { g_err = "null cfg"; return nullptr; }
  if (cfg->deg_pol != 3) { g_err = "deg_pol must be 3 (reference yaml: only 3 is supported)"; return nullptr; }
  if (!cfg->use_linear_constraints) { g_err = "use_linear_constraints=false (bilinear variant) is out of scope"; return nullptr; }
  if (cfg->num_pol < 1 || cfg->num_pol > NEP_MAX_POL) { g_err = "num_pol out of range"; return nullptr; }
  if (cfg->id < 1 || cfg->id > cfg->num_agents) { g_err = "id out of range"; return nullptr; }
  if (!have_device()) { g_err = "no HIP device: the back end has no CPU path"; return nullptr; }
  std::unique_ptr<nep_backend> h(new nep_backend());      // (every return below but the last deletes it, and with it what it owns)
  h->cfg = *cfg; h->pb.assign(cfg->pb, cfg->pb + 2 * cfg->num_agents); h->cfg.pb = nullptr;
  Engine& E = h->eng;
  E.sp.num_agents = cfg->num_agents; E.sp.num_pol = cfg->num_pol; E.sp.n_static = 0; E.sp.n_hull = 0; E.sp.ent_enabled = 0;
  E.sp.n_local = 1; E.sp.first_local = cfg->id - 1; E.sp.skip_own = 0; E.sp.T_span = cfg->T_span; E.sp.weight = cfg->weight_term;
  E.sp.drone_radius = 0; E.n_scenes = 1;
  E.lines_cap_user = -1;      // (one replan at a time: the buckets are sized for the reference's worst case, there is no flag to poll)
  E.set_clock();
  HIPCHK_NULL(hipStreamCreate(&h->stream));
  if (h->lay_out(cfg->num_agents > 8 ? cfg->num_agents : 8)) return nullptr;
  if (E.d_pb.ensure(h->pb.size())) return nullptr;
  HIPCHK_NULL(hipMemcpy(E.d_pb.p, h->pb.data(), h->pb.size() * sizeof(double), hipMemcpyHostToDevice));
  int32_t off0[1] = {0};
  if (E.upload_statics(0, off0, nullptr)) return nullptr;
  if (E.build_tables()) return nullptr;
  return h.release();
}

void nep_backend_destroy(nep_backend_t* h) { if (h) delete h; }

int nep_backend_set_max_values(nep_backend_t* h, double x_min, double x_max, double y_min, double y_max, double z_min,
                               double z_max, double v_max, double a_max, double j_max) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  SceneParams& sp = h->eng.sp;
  sp.mins[0] = x_min; sp.mins[1] = y_min; sp.mins[2] = z_min; sp.maxs[0] = x_max; sp.maxs[1] = y_max; sp.maxs[2] = z_max;
  sp.v_max = v_max; sp.a_max = a_max; h->j_max = j_max;
  sp.long_length = std::sqrt((x_max - x_min) * (x_max - x_min) + (y_max - y_min) * (y_max - y_min));
  h->have_bounds = true;
  return 0;
}
int nep_backend_set_max_runtime(nep_backend_t* h, double s) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  h->max_runtime = s;
  h->eng.sp.time_limit_ticks = s > 0 ? (long long)(s * h->eng.clock_hz) : 0;
  return 0;
}
int nep_backend_set_tether_length(nep_backend_t* h, double t) { if (!h) return fail(NEP_E_ARG, "null handle"); h->tether = t; return 0; }

int nep_backend_set_static_obst_vert(nep_backend_t* h, int32_t n, const int32_t* off, const double* xy) {
  if (!h || n < 0 || (n > 0 && (!off || !xy))) return fail(NEP_E_ARG, "bad static obstacle arguments");
  int32_t off0[1] = {0};
  return h->eng.upload_statics(n, n ? off : off0, xy);
}

int nep_backend_set_init_trajectory(nep_backend_t* h, const nep_pwp* p) {
  if (!h || !p) return fail(NEP_E_ARG, "null argument");
  if (p->n_seg < 1 || p->n_seg > h->cfg.num_pol) return fail(NEP_E_CAP, "initial trajectory must have 1..num_pol intervals");
  std::memset(&h->guess, 0, sizeof(h->guess));
  h->guess.K = p->n_seg; h->guess.t_start = 0.0;
  for (int ax = 0; ax < 3; ax++) for (int i = 0; i < p->n_seg; i++) for (int j = 0; j < 4; j++) h->guess.coeff[ax][i][j] = p->coeff[ax][i][j];
  h->guess_times.assign(p->times, p->times + p->n_seg + 1);
  *h->in<nep_guess>(h->L.guess) = h->guess;
  h->have_init = true; h->solved = false; h->states_fresh = false;
  return 0;
}

int nep_backend_set_hulls(nep_backend_t* h, int32_t n_obst, const int32_t* off, const double* xy) {
  if (!h || n_obst < 0 || (n_obst > 0 && (!off || !xy))) return fail(NEP_E_ARG, "bad hull arguments");
  const int np = h->cfg.num_pol;
  if (int e = h->lay_out(n_obst)) return e;
  int* nv = h->in<int>(h->L.nv); double* hx = h->in<double>(h->L.xy);
  for (int p = 0; p < n_obst * np; p++) {
    const int c = off[p + 1] - off[p];
    if (c > kHullV) return fail(NEP_E_CAP, "hull with more than NEP_HULL_MAX_V vertices");
    if (c < 0) return fail(NEP_E_ARG, "hull offsets must not decrease");
    nv[p] = c;
    double* q = hx + (size_t)p * kHullV * 2;
    std::memcpy(q, xy + 2 * (size_t)off[p], (size_t)c * 2 * sizeof(double));
    if (c < kHullV) std::memset(q + 2 * c, 0, (size_t)(kHullV - c) * 2 * sizeof(double));
    if (!normalize_ccw(q, c)) return fail(NEP_E_ARG, "hull polygon is not convex");
  }
  h->n_obst = n_obst; h->have_hulls = true;
  return 0;
}

int nep_backend_set_hulls_no_inflation(nep_backend_t* h, int32_t n_agents, const int32_t* off, const double* xy) {
  if (!h || n_agents != h->cfg.num_agents || !off) return fail(NEP_E_ARG, "hullsNoInflation must be indexed by agent id (num_agents lists)");
  const int np = h->cfg.num_pol;
  double* x0 = h->in<double>(h->L.h0xy); int* n0 = h->in<int>(h->L.h0nv);
  for (int p = 0; p < n_agents * np; p++) {
    const int c = off[p + 1] - off[p];
    n0[p] = c;
    if (c > 0) { x0[(size_t)p * 2] = xy[2 * off[p]]; x0[(size_t)p * 2 + 1] = xy[2 * off[p] + 1]; }  // only col(0) is read (:722-734)
    else { x0[(size_t)p * 2] = 0.0; x0[(size_t)p * 2 + 1] = 0.0; }
  }
  h->have_h0 = true;
  return 0;
}

int nep_backend_set_ent_state_vector(nep_backend_t* h, const nep_ent_view* e) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  if (!e) { h->have_ent = false; return 0; }
  const int N = h->cfg.num_agents;
  if (e->n_active < N) return fail(NEP_E_ARG, "active_cases rows shorter than num_agents");
  int* cas = h->in<int>(h->L.cas);
  std::memset(cas, 0, (size_t)NEP_MAX_POL * N * sizeof(int));
  // case id of (knot i, agent j): solver_gurobi_poly.cpp:624-631 (last matching alpha wins)
  for (int i = 0; i < e->n_states && i < NEP_MAX_POL; i++)
    for (int j = 0; j < N; j++) {
      if (e->active_cases[(size_t)i * e->n_active + j] != 1) continue;
      int cid = 0;
      for (int a = e->alpha_off[i]; a < e->alpha_off[i + 1]; a++) if (e->alphas[2 * a] == j + 1) cid = e->alphas[2 * a + 1];
      cas[(size_t)i * N + j] = cid;
    }
  double* bend = h->in<double>(h->L.bend); int* bend_n = h->in<int>(h->L.bendn);
  std::memset(bend, 0, (size_t)N * kBend * 2 * sizeof(double));
  for (int j = 0; j < N; j++) {
    const int nb = e->bend_off[j + 1] - e->bend_off[j];
    if (nb > kBend) return fail(NEP_E_CAP, "more than NEP_MAX_BEND bend points");
    bend_n[j] = nb;
    for (int b = 0; b < nb; b++) { bend[((size_t)j * kBend + b) * 2] = e->bend_xy[2 * (e->bend_off[j] + b)]; bend[((size_t)j * kBend + b) * 2 + 1] = e->bend_xy[2 * (e->bend_off[j] + b) + 1]; }
  }
  h->have_ent = true;
  return 0;
}

int nep_backend_debug_set_lines(nep_backend_t* h, int32_t n, const int32_t* seg, const double* nd) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  h->override_n = n;
  if (n > 0) { h->ov_seg.assign(seg, seg + n); h->ov_nd.assign(nd, nd + 3 * n); } else { h->ov_seg.clear(); h->ov_nd.clear(); }
  return 0;
}

int nep_backend_optimize(nep_backend_t* h, double* objective_value) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  if (!h->have_bounds) return fail(NEP_E_STATE, "optimize before setMaxValues");
  if (!h->have_init) return fail(NEP_E_STATE, "optimize before setInitTrajectory");
  Engine& E = h->eng;
  const int N = h->cfg.num_agents, np = h->cfg.num_pol;
  E.sp.n_hull = h->have_hulls ? h->n_obst : 0;
  E.sp.ent_enabled = h->have_ent ? 1 : 0;
  {
    // the samples generatePwpOut returns are made by the QP kernel's tail at the schedule's dc: the schedule must hold every state of the
    // horizon (ceil(num_pol T_span / dc) + 1, as generatePwpOut's own path sizes it) — a fixed cap of 128 cut trajectories longer than
    // 6.3 s short of what the reference's time walk returns (solver_gurobi_poly.cpp:911-934)
    const double dc0 = E.sched_dc > 0 ? E.sched_dc : 0.05;
    const int need = (int)std::ceil(np * E.sp.T_span / dc0) + 3;
    if (int e = E.build_schedule(dc0, need)) return e;
  }
  if (h->override_n >= 0) {  // line buckets sized for the override
    int per_seg[NEP_MAX_POL] = {0}; for (int l = 0; l < h->override_n; l++) { int s = h->ov_seg[l]; if (s < 0 || s >= NEP_MAX_POL) return fail(NEP_E_ARG, "override line segment out of range"); per_seg[s]++; }
    int mx = 8; for (int s = 0; s < NEP_MAX_POL; s++) if (per_seg[s] > mx) mx = per_seg[s];
    E.sp.n_hull = mx;  // only used to size lines_cap below
  }
  if (int e = E.size_scratch()) return e;
  if (h->override_n >= 0) E.sp.n_hull = 0;
  const auto t_host0 = std::chrono::steady_clock::now();
  ProblemSet ps{};
  E.fill(ps);
  const InLayout& L = h->L;
  const bool with_hulls = h->have_hulls && h->n_obst > 0 && h->override_n < 0;
  // one copy in: the guess, the vertex counts and — the arena's tail — the vertices of the hull lists in use; with the entangle
  // rows the block between them goes along (one contiguous range from the start), without them the two ends travel separately
  // only when the block in between is bigger than what it would cost to carry it
  const size_t xy_used = with_hulls ? (size_t)h->n_obst * np * kHullV * 2 * sizeof(double) : 0;
  if (h->have_ent) {
    if (!h->have_h0) return fail(NEP_E_STATE, "setEntStateVector without setHullsNoInflation");
    HIPCHK(hipMemcpyAsync(h->d_in.p, h->hin.p, L.xy + xy_used, hipMemcpyHostToDevice, h->stream));
  } else {
    HIPCHK(hipMemcpyAsync(h->d_in.p, h->hin.p, L.cas, hipMemcpyHostToDevice, h->stream));
    if (xy_used) HIPCHK(hipMemcpyAsync(h->d_in.p + L.xy, h->hin.p + L.xy, xy_used, hipMemcpyHostToDevice, h->stream));
  }
  const size_t out_states = (sizeof(nep_solution) + 255) & ~(size_t)255;
  const size_t out_bytes = out_states + (size_t)E.sp.max_states * NEP_STATE_DOUBLES * sizeof(double);
  if (int e = h->d_out.ensure(out_bytes)) return e;
  if (int e = h->hout.ensure(out_bytes)) return e;
  ps.guess = (const nep_guess*)(h->d_in.p + L.guess); ps.solution = (nep_solution*)h->d_out.p;
  ps.states = (double*)(h->d_out.p + out_states); ps.commit = nullptr; ps.case_id = nullptr;
  if (with_hulls) { ps.hull_xy = (double*)(h->d_in.p + L.xy); ps.hull_nv = (int*)(h->d_in.p + L.nv); }
  if (h->have_ent) {
    ps.case_id = (const int*)(h->d_in.p + L.cas);
    ps.hull0_xy = (double*)(h->d_in.p + L.h0xy); ps.hull0_nv = (int*)(h->d_in.p + L.h0nv);
    ps.bend_xy = (double*)(h->d_in.p + L.bend); ps.bend_n = (int*)(h->d_in.p + L.bendn);
  }
  ps.lines_override = 0;
  if (h->override_n >= 0) {
    std::vector<double> nd((size_t)NEP_MAX_POL * E.sp.lines_cap * 3, 0.0); std::vector<int> cnt(NEP_MAX_POL, 0);
    for (int l = 0; l < h->override_n; l++) { int s = h->ov_seg[l]; int c = cnt[s]++; for (int k = 0; k < 3; k++) nd[((size_t)s * E.sp.lines_cap + c) * 3 + k] = h->ov_nd[3 * l + k]; }
    HIPCHK(hipMemcpyAsync(E.d_line_nd.p, nd.data(), nd.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(E.d_line_cnt.p, cnt.data(), cnt.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // host vectors go out of scope
    ps.lines_override = 1;
  }
  if (int e = E.run(nullptr, 0, ps, h->stream)) return e;
  // one copy out: the solution and generatePwpOut's samples at the schedule's dc (the QP kernel's tail wrote them)
  HIPCHK(hipMemcpyAsync(h->hout.p, h->d_out.p, out_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->h_sol = *(const nep_solution*)h->hout.p;
  h->stats = h->h_sol.stats;
  h->stats.solve_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_host0).count();   // what the caller's clock around optimize() sees (neptune.cpp:1504,1528), set-up checks excluded
  h->solved = true; h->states_fresh = true;
  if (h->stats.status != NEP_FAILED && objective_value) *objective_value = h->stats.objective;  // :882 (untouched on failure)
  return h->stats.status;
}

int nep_backend_generate_pwp_out(nep_backend_t* h, double t_start, double dc, nep_pwp* pwp_out, double* states_out,
                                 int32_t states_cap, int32_t* n_states_out) {
  if (!h || !pwp_out) return fail(NEP_E_ARG, "null argument");
  if (!h->have_init) return fail(NEP_E_STATE, "generatePwpOut before setInitTrajectory");
  const int K = h->guess.K;
  std::memset(pwp_out, 0, sizeof(*pwp_out));
  pwp_out->n_seg = K;
  for (int i = 0; i <= K; i++) pwp_out->times[i] = h->guess_times[i] + t_start;  // :898
  const double (*co)[NEP_MAX_POL][4] = h->solved ? h->h_sol.coeff : h->guess.coeff;   // pwp_out_ = pwp_init_ until solved
  for (int ax = 0; ax < 3; ax++) for (int i = 0; i < K; i++) for (int j = 0; j < 4; j++) pwp_out->coeff[ax][i][j] = co[ax][i][j];
  if (n_states_out) *n_states_out = 0;
  if (states_out && states_cap > 0 && h->solved && h->states_fresh && dc == h->eng.sched_dc) {
    // the samples came back with the solution (the QP kernel's tail made them at this dc): no device work here
    int ns = h->h_sol.n_states; if (ns > states_cap) ns = states_cap;
    const size_t out_states = (sizeof(nep_solution) + 255) & ~(size_t)255;
    std::memcpy(states_out, h->hout.p + out_states, (size_t)ns * NEP_STATE_DOUBLES * sizeof(double));
    if (n_states_out) *n_states_out = ns;
    return 0;
  }
  if (states_out && states_cap > 0) {
    Engine& E = h->eng;
    DevBuf<nep_solution> d_sol_tmp; DevBuf<double> d_states_tmp;
    if (int e = d_sol_tmp.ensure(1)) return e;
    {  // another dc than the schedule's, or no solve yet: stage the trajectory to sample (the solution, else the guess)
      nep_solution s{}; s.K = K; std::memcpy(s.coeff, h->solved ? h->h_sol.coeff : h->guess.coeff, sizeof(s.coeff));
      HIPCHK(hipMemcpy(d_sol_tmp.p, &s, sizeof(s), hipMemcpyHostToDevice));
    }
    int cap = (int)std::ceil(h->cfg.num_pol * h->cfg.T_span / dc) + 3;
    if (int e = E.build_schedule(dc, cap)) return e;
    int ns = E.h_sched_n[K]; if (ns > states_cap) ns = states_cap;
    if (int e = d_states_tmp.ensure((size_t)cap * NEP_STATE_DOUBLES)) return e;
    hipLaunchKernelGGL(sample_kernel, dim3((ns + 63) / 64), dim3(64), 0, h->stream, d_sol_tmp.p, K, E.d_sched_seg.p + (size_t)K * cap, E.d_sched_dt.p + (size_t)K * cap, ns, d_states_tmp.p);
    HIPCHK(hipMemcpyAsync(states_out, d_states_tmp.p, (size_t)ns * NEP_STATE_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->states_fresh = false;      // (the schedule now belongs to this dc: the next optimize samples at it)
    if (n_states_out) *n_states_out = ns;
  }
  return 0;
}

// Measurement aid (bench.py's per_agent_api leg): the drop-in call sequence of one replan, as Neptune::replanFull issues it
// (neptune.cpp:1514-1527: setInitTrajectory -> setHulls -> setHullsNoInflation -> setEntStateVector -> optimize ->
// generatePwpOut), n_iter times from one host thread with the caller's buffers; us_out[i] = wall time of iteration i as a C++
// caller's clock around the six calls sees it, us_optimize_out[i] (may be NULL) = of optimize() alone.  h0_off / ent may be
// NULL (entangle check off).  Returns the status of the last optimize, or < 0.
int nep_backend_debug_time_sequence(nep_backend_t* h, const nep_pwp* init, int32_t n_obst, const int32_t* hull_off, const double* hull_xy,
                                    const int32_t* h0_off, const double* h0_xy, const nep_ent_view* ent, double t_start, double dc,
                                    int32_t n_iter, double* us_out, double* us_optimize_out) {
  if (!h || !init || n_iter < 1 || !us_out) return fail(NEP_E_ARG, "bad arguments");
  const int cap = (int)std::ceil(h->cfg.num_pol * h->cfg.T_span / dc) + 3;
  std::vector<double> states((size_t)cap * NEP_STATE_DOUBLES);
  nep_pwp out; int32_t ns = 0; int status = 0;
  for (int it = 0; it < n_iter; it++) {
    const auto t0 = std::chrono::steady_clock::now();
    if (int e = nep_backend_set_init_trajectory(h, init)) return e;
    if (int e = nep_backend_set_hulls(h, n_obst, hull_off, hull_xy)) return e;
    if (h0_off) if (int e = nep_backend_set_hulls_no_inflation(h, h->cfg.num_agents, h0_off, h0_xy)) return e;
    if (int e = nep_backend_set_ent_state_vector(h, ent)) return e;
    const auto t1 = std::chrono::steady_clock::now();
    double obj = 0.0;
    status = nep_backend_optimize(h, &obj);
    if (status < 0) return status;
    const auto t2 = std::chrono::steady_clock::now();
    if (int e = nep_backend_generate_pwp_out(h, t_start, dc, &out, states.data(), cap, &ns)) return e;
    const auto t3 = std::chrono::steady_clock::now();
    us_out[it] = std::chrono::duration<double, std::micro>(t3 - t0).count();
    if (us_optimize_out) us_optimize_out[it] = std::chrono::duration<double, std::micro>(t2 - t1).count();
  }
  return status;
}

int nep_backend_get_stats(nep_backend_t* h, nep_stats* out) { if (!h || !out) return fail(NEP_E_ARG, "null argument"); *out = h->stats; return 0; }

int nep_backend_debug_get_lines(nep_backend_t* h, int32_t cap, int32_t* seg, double* nd, int32_t* n_out) {
  if (!h || !n_out) return fail(NEP_E_ARG, "null argument");
  return read_lines(h->eng, 0, h->guess.K, cap, seg, nd, n_out);
}

// =================================================================================================
// stand-alone kernels
// =================================================================================================
int nep_separator_batch_rule(int32_t rule, int32_t n_prob, const int32_t* a_off, const double* a_xy, const int32_t* b_off, const double* b_xy,
                             double* nd_out, int32_t* solved_out) {
  if (rule != 0 && rule != 1) return fail(NEP_E_ARG, "separator rule: 0 largest gap, 1 GLPK-class simplex");
  if (n_prob < 0 || !a_off || !b_off || !nd_out || !solved_out) return fail(NEP_E_ARG, "bad arguments");
  if (!have_device()) return fail(NEP_E_HIP, "no HIP device: the back end has no CPU path");
  if (n_prob == 0) return 0;
  for (int p = 0; p < n_prob; p++) {
    if (b_off[p + 1] - b_off[p] != 4) return fail(NEP_E_ARG, "set B must be the 4 control points of a segment");
    if (a_off[p + 1] - a_off[p] > kHullV) return fail(NEP_E_CAP, "set A has more than NEP_HULL_MAX_V points");
  }
  DevBuf<int> da, db, ds; DevBuf<double> dax, dbx, dnd;
  const int na = a_off[n_prob], nb = b_off[n_prob];
  int e = 0;
  if ((e = da.ensure(n_prob + 1)) || (e = db.ensure(n_prob + 1)) || (e = ds.ensure(n_prob)) || (e = dax.ensure((size_t)2 * na)) || (e = dbx.ensure((size_t)2 * nb)) || (e = dnd.ensure((size_t)3 * n_prob))) return e;
  HIPCHK(hipMemcpy(da.p, a_off, (n_prob + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db.p, b_off, (n_prob + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (na) HIPCHK(hipMemcpy(dax.p, a_xy, (size_t)2 * na * sizeof(double), hipMemcpyHostToDevice));
  if (nb) HIPCHK(hipMemcpy(dbx.p, b_xy, (size_t)2 * nb * sizeof(double), hipMemcpyHostToDevice));
  launch_separator_explicit(n_prob, da.p, dax.p, db.p, dbx.p, dnd.p, ds.p, rule, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(nd_out, dnd.p, (size_t)3 * n_prob * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(solved_out, ds.p, (size_t)n_prob * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int nep_separator_batch(int32_t n_prob, const int32_t* a_off, const double* a_xy, const int32_t* b_off, const double* b_xy,
                        double* nd_out, int32_t* solved_out) {
  return nep_separator_batch_rule(0, n_prob, a_off, a_xy, b_off, b_xy, nd_out, solved_out);
}

int nep_gjk_batch(int32_t n_prob, const int32_t* a_off, const double* a_xy, const double* b_xy, int32_t* hit_out) {
  if (n_prob < 0 || !a_off || !b_xy || !hit_out) return fail(NEP_E_ARG, "bad arguments");
  if (!have_device()) return fail(NEP_E_HIP, "no HIP device: the back end has no CPU path");
  if (n_prob == 0) return 0;
  DevBuf<int> da, dh; DevBuf<double> dax, dbx;
  const int na = a_off[n_prob];
  int e = 0;
  if ((e = da.ensure(n_prob + 1)) || (e = dh.ensure(n_prob)) || (e = dax.ensure((size_t)2 * (na > 0 ? na : 1))) || (e = dbx.ensure((size_t)8 * n_prob))) return e;
  HIPCHK(hipMemcpy(da.p, a_off, (n_prob + 1) * sizeof(int), hipMemcpyHostToDevice));
  if (na) HIPCHK(hipMemcpy(dax.p, a_xy, (size_t)2 * na * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dbx.p, b_xy, (size_t)8 * n_prob * sizeof(double), hipMemcpyHostToDevice));
  launch_gjk_explicit(n_prob, da.p, dax.p, dbx.p, dh.p, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(hit_out, dh.p, (size_t)n_prob * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int nep_hulls_batch(int32_t n_traj, const nep_traj_rec* trajs, double t_start, int32_t num_pol, double T_span, double drone_radius,
                    double* hull_xy, int32_t* hull_nv, double* hull0_xy, int32_t* hull0_nv) {
  if (n_traj < 0 || !trajs || !hull_xy || !hull_nv || !hull0_xy || !hull0_nv || num_pol < 1) return fail(NEP_E_ARG, "bad arguments");
  if (!have_device()) return fail(NEP_E_HIP, "no HIP device: the back end has no CPU path");
  if (n_traj == 0) return 0;
  DevBuf<nep_traj_rec> dr; DevBuf<double> dh, dh0; DevBuf<int> dn, dn0, dfl;
  const size_t np = (size_t)n_traj * num_pol;
  int e = 0;
  if ((e = dr.ensure(n_traj)) || (e = dh.ensure(np * kHullV * 2)) || (e = dh0.ensure(np * kHullV * 2)) || (e = dn.ensure(np)) || (e = dn0.ensure(np)) || (e = dfl.ensure(1))) return e;
  HIPCHK(hipMemset(dfl.p, 0, sizeof(int)));
  HIPCHK(hipMemcpy(dr.p, trajs, (size_t)n_traj * sizeof(nep_traj_rec), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dh.p, 0, np * kHullV * 2 * sizeof(double))); HIPCHK(hipMemset(dh0.p, 0, np * kHullV * 2 * sizeof(double)));
  launch_hulls_explicit(dr.p, n_traj, t_start, num_pol, T_span, drone_radius, dh.p, dn.p, dh0.p, dn0.p, dfl.p, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(hull_xy, dh.p, np * kHullV * 2 * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hull0_xy, dh0.p, np * kHullV * 2 * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hull_nv, dn.p, np * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hull0_nv, dn0.p, np * sizeof(int), hipMemcpyDeviceToHost));
  int flags = 0;
  HIPCHK(hipMemcpy(&flags, dfl.p, sizeof(int), hipMemcpyDeviceToHost));
  if (flags & NEP_FLAG_HULL_OVERFLOW) return fail(NEP_E_CAP, "an interval overlaps more than NEP_HULL_MAX_CP/4 committed segments (or its hull has more than NEP_HULL_MAX_V vertices)");
  return 0;
}

}  // extern "C"

// =================================================================================================
// batched handle
// =================================================================================================
struct nep_batch {
  Engine eng;
  nep_batch_cfg cfg{};
  int slots = 0;
  const nep_traj_rec* fe_committed = nullptr;   // the records nep_batch_frontend built this round's hulls from
  int ent_ns = 3;                               // num_sample_per_interval the hull blocks reserve room for (nep_batch_set_ent_samples; yaml: 3)
  bool replanned = false;                       // a replan with a QP half has been enqueued (nep_batch_guess_fallback needs one before it)
  // nep_batch_set_tether_audit: the caller's [slots] records the tracking calls accumulate into (null: off) and the tick's length
  nep_tether_audit* tether_audit = nullptr; double tether_audit_dt = 0.0;
  // nep_batch_fleet_* (include/neptune_fleet.h): the committed plans of every slot, allocated by nep_batch_fleet_init
  struct Fleet {
    bool ready = false, timers = false; int cap = 0; nep_fleet_cfg cfg{};
    DevBuf<double> ring, state, goal, t_now; DevBuf<nep_pwp> pwp;
    DevBuf<int> head, size, k_end, flown, done, outcome, sflags, period, phase, round, counters, origin;
    // the tethers (nep_batch_fleet_init_ent): state at the tracked position, the published bend lists, flags, scratch
    bool ent_ready = false; double cable = 0.0;
    DevBuf<nep_fe_ent_state> ent, ent_save; DevBuf<double> pub_xy, pub_prev_xy, ent_pos;
    DevBuf<int> pub_n, pub_prev_n, ent_flags, ent_ever, ent_walked, ent_flags_a;
    // the list form of the same (nep_batch_fleet_init_ent_lists): ent_cap != 0 = the state lives in ent_lists, not in ent
    int ent_cap = 0; ListBuf ent_lists, ent_lsave; DevBuf<int> ent_held;
    // the missions (nep_batch_fleet_mission_init): legs, totals, runs, the log; the keep-outs are staged by
    // nep_batch_fleet_mission_keepout (before or after either init: no init drops them)
    bool mis_ready = false; nep_mission_cfg mis_cfg{}; size_t mis_lds = 0;
    DevBuf<double> mis_t_issue, mis_length, mis_sums, mis_t_run; DevBuf<int> mis_completed, mis_counts, mis_scene, mis_log_n; DevBuf<nep_mission_leg> mis_log;
    DevBuf<int> keep_n, keep_off; DevBuf<double> keep_xy;
    // the scripted goals (nep_batch_fleet_mission_script): [slots][*script_n][3] and the rows per slot now; script_cap rows per slot
    // were allocated by the first upload (0: none yet) and no init drops them
    int script_cap = 0; DevBuf<double> script; DevBuf<int> script_n;
    DevBuf<char> rec_stage;      // nep_batch_fleet_restore: the blob (or the one block of it) on its way in
    std::vector<hipStream_t> seen;      // the streams nep_batch_fleet_select and the snapshot calls were given (restore refuses while one captures)
    void saw(void* stream) { hipStream_t st = (hipStream_t)stream; if (!st) return; for (hipStream_t q : seen) if (q == st) return; if (seen.size() < 16) seen.push_back(st); }      // (the null stream cannot capture)
  } fleet;
};

namespace {
// the handle's scratch plus the caller's buffers of one round (each may be null: not every call has all of them)
ProblemSet round_set(nep_batch* h, const nep_guess* d_guess = nullptr, nep_solution* d_solution = nullptr, double* d_states = nullptr,
                     nep_traj_rec* d_commit = nullptr, const nep_traj_rec* d_prev_commit = nullptr, const void* d_ent = nullptr) {
  ProblemSet ps{};
  h->eng.fill(ps);
  ps.guess = d_guess; ps.solution = d_solution; ps.states = d_states; ps.commit = d_commit; ps.prev_commit = d_prev_commit;
  ps.case_id = (h->eng.sp.ent_enabled && d_ent) ? (const int*)d_ent : nullptr;
  ps.lines_override = 0;
  return ps;
}
// nep_batch_replan (phases 3) and its two halves (1: hulls + separating lines, 2: the QP on them) behind their own argument checks
int replan_phases(nep_batch* h, int phases, const nep_traj_rec* d_committed, const nep_guess* d_guess, const void* d_ent,
                  nep_solution* d_solution, double* d_states, nep_traj_rec* d_commit, void* stream) {
  // d_committed == NULL (nep_batch_replan alone): the interval hulls of this round are already in the handle's scratch, made by
  // nep_batch_frontend, whose records are this round's previous ones
  ProblemSet ps = round_set(h, d_guess, d_solution, d_states, d_commit, d_committed ? d_committed : h->fe_committed, d_ent);
  if (phases & 2) h->replanned = true;
  return h->eng.run(d_committed, h->cfg.num_agents, ps, (hipStream_t)stream, phases);
}
}  // namespace

extern "C" {

nep_batch_t* nep_batch_create(const nep_batch_cfg* c) {
  if (!c || !c->pb) { g_err = "null cfg"; return nullptr; }
  if (c->num_pol < 1 || c->num_pol > NEP_MAX_POL || c->num_agents < 1 || c->n_local < 1 || c->first_local < 0 ||
      c->first_local + c->n_local > c->num_agents || c->n_scenes < 1 || c->max_states < 1) { g_err = "bad batch configuration"; return nullptr; }
  if (!have_device()) { g_err = "no HIP device: the back end has no CPU path"; return nullptr; }
  std::unique_ptr<nep_batch> h(new nep_batch());
  h->cfg = *c; h->cfg.pb = nullptr; h->cfg.static_off = nullptr; h->cfg.static_xy = nullptr;
  Engine& E = h->eng; SceneParams& sp = E.sp;
  sp.num_agents = c->num_agents; sp.num_pol = c->num_pol; sp.n_hull = c->num_agents; sp.ent_enabled = c->enable_entangle;
  sp.n_local = c->n_local; sp.first_local = c->first_local; sp.skip_own = 1;
  sp.T_span = c->T_span; sp.weight = c->weight_term; sp.drone_radius = c->drone_radius;
  sp.mins[0] = c->x_min; sp.mins[1] = c->y_min; sp.mins[2] = c->z_min; sp.maxs[0] = c->x_max; sp.maxs[1] = c->y_max; sp.maxs[2] = c->z_max;
  sp.v_max = c->v_max; sp.a_max = c->a_max;
  sp.long_length = std::sqrt((c->x_max - c->x_min) * (c->x_max - c->x_min) + (c->y_max - c->y_min) * (c->y_max - c->y_min));
  E.n_scenes = c->n_scenes; h->slots = c->n_scenes * c->n_local;
  E.set_clock();
  bool ok = true;
  ok = ok && !E.d_pb.ensure((size_t)2 * c->num_agents);
  if (ok) ok = hipMemcpy(E.d_pb.p, c->pb, (size_t)2 * c->num_agents * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  int32_t off0[1] = {0};
  if (ok) ok = !E.upload_statics(c->n_static, c->n_static ? c->static_off : off0, c->static_xy);
  if (ok) ok = !E.build_tables();
  if (ok) ok = !E.build_schedule(c->dc, c->max_states);
  if (ok) ok = !E.size_scratch();
  if (!ok) { if (g_err.empty()) g_err = "batch setup failed"; return nullptr; }
  return h.release();
}

void nep_batch_destroy(nep_batch_t* h) { if (h) delete h; }

int64_t nep_batch_ent_bytes(const nep_batch_t* h) { return h ? (int64_t)h->slots * NEP_MAX_POL * h->cfg.num_agents * sizeof(int32_t) : 0; }

int nep_batch_replan(nep_batch_t* h, const nep_traj_rec* d_committed, const nep_guess* d_guess, const void* d_ent,
                     nep_solution* d_solution, double* d_states, nep_traj_rec* d_commit, void* stream) {
  if (!h || !d_guess || !d_solution) return fail(NEP_E_ARG, "null argument");
  return replan_phases(h, 3, d_committed, d_guess, d_ent, d_solution, d_states, d_commit, stream);
}
// The two halves of nep_batch_replan as calls of their own (include/neptune_backend.h): hulls + separating lines, then the QP on them
int nep_batch_replan_lines(nep_batch_t* h, const nep_traj_rec* d_committed, const nep_guess* d_guess, const void* d_ent, void* stream) {
  if (!h || !d_guess || !d_committed) return fail(NEP_E_ARG, "null argument");
  return replan_phases(h, 1, d_committed, d_guess, d_ent, nullptr, nullptr, nullptr, stream);
}
int nep_batch_replan_solve(nep_batch_t* h, const nep_traj_rec* d_committed, const nep_guess* d_guess, const void* d_ent,
                           nep_solution* d_solution, double* d_states, nep_traj_rec* d_commit, void* stream) {
  if (!h || !d_guess || !d_solution || !d_committed) return fail(NEP_E_ARG, "null argument");
  return replan_phases(h, 2, d_committed, d_guess, d_ent, d_solution, d_states, d_commit, stream);
}

// ---- sharded hulls: a rank computes the interval hulls of its own agents' committed trajectories
// into one block, the blocks of all ranks are all-gathered, and every rank runs separator + QP
// against the gathered blocks (kernels address them through hull_ref, nep_device.h) -------------
namespace {
struct HullBlock { size_t xy, nv, xy0, nv0, bend, bend_n, samp, present, bytes; };
// ent_ns > 0 (handle created with enable_entangle): the block also carries what the entangle check reads of a committed
// trajectory — its ent_ns + 1 samples per interval (Neptune::SamplePointsOfIntervals) and whether it exists — so that the
// entangle-aware front end and the safety pass's re-check run against gathered blocks like everything else
HullBlock hull_block_layout(int n_scenes, int per, int np, int ent_ns = 0) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  HullBlock b{};
  const size_t e = (size_t)n_scenes * per;
  size_t o = 0;
  b.xy = o; o = up(o + e * np * kHullV * 2 * sizeof(double));
  b.nv = o; o = up(o + e * np * sizeof(int));
  b.xy0 = o; o = up(o + e * np * 2 * sizeof(double));
  b.nv0 = o; o = up(o + e * np * sizeof(int));
  b.bend = o; o = up(o + e * kBend * 2 * sizeof(double));
  b.bend_n = o; o = up(o + e * sizeof(int));
  b.samp = o; b.present = o;
  if (ent_ns > 0) { o = up(o + e * np * (ent_ns + 1) * 2 * sizeof(double)); b.present = o; o = up(o + e * sizeof(int)); }
  b.bytes = o;
  return b;
}
HullBlock block_of(const nep_batch* h) { return hull_block_layout(h->cfg.n_scenes, h->cfg.n_local, h->cfg.num_pol, h->cfg.enable_entangle ? h->ent_ns : 0); }
void point_at_block(ProblemSet& ps, const HullBlock& b, void* base) {
  char* p = (char*)base;
  ps.hull_xy = (double*)(p + b.xy); ps.hull_nv = (int*)(p + b.nv); ps.hull0_xy = (double*)(p + b.xy0); ps.hull0_nv = (int*)(p + b.nv0);
  ps.bend_xy = (double*)(p + b.bend); ps.bend_n = (int*)(p + b.bend_n);
}
// ps reads its hulls from n_blocks all-gathered blocks of n_local agents each
int use_blocks(ProblemSet& ps, const nep_batch* h, const void* d_blocks, int n_blocks) {
  if (n_blocks < 1 || n_blocks * h->cfg.n_local != h->cfg.num_agents) return fail(NEP_E_ARG, "n_blocks * n_local must equal num_agents");
  const HullBlock b = block_of(h);
  point_at_block(ps, b, const_cast<void*>(d_blocks));
  ps.hull_pb = h->cfg.n_local; ps.hull_bstride = (long)b.bytes;
  ps.hull_pb_magic = (h->cfg.n_local > 0 && h->cfg.num_agents < 65536) ? (1ull << 32) / (unsigned long long)h->cfg.n_local + 1ull : 0ull;
  return 0;
}

// (beam: with the beam's width, which the best-first search does not read)
bool fe_cfg_ok(const nep_fe_cfg* cfg, bool beam = true) {
  return cfg->num_samples >= 2 && cfg->num_samples <= NEP_FE_MAX_SAMPLES && (!beam || (cfg->beam_width >= 1 && cfg->beam_width <= NEP_FE_MAX_BEAM)) &&
         cfg->voxel_size > 0.0 && cfg->j_max > 0.0;
}
}  // namespace

int64_t nep_batch_hull_block_bytes(const nep_batch_t* h) {
  return h ? (int64_t)block_of(h).bytes : 0;
}

int nep_batch_hulls(nep_batch_t* h, const nep_traj_rec* d_committed_local, const nep_guess* d_guess, void* d_block, void* stream) {
  if (!h || !d_committed_local || !d_guess || !d_block) return fail(NEP_E_ARG, "null argument");
  Engine& E = h->eng;
  const HullBlock b = block_of(h);
  ProblemSet ps = round_set(h, d_guess);
  point_at_block(ps, b, d_block);
  launch_hulls(d_committed_local, h->cfg.n_scenes, h->cfg.n_local, d_guess, E.sp, ps, (hipStream_t)stream, grouped_hulls(E.sp, h->cfg.n_scenes, h->cfg.n_local));
  if (h->cfg.enable_entangle)      // what the entangle check reads of my agents' trajectories travels in the same block
    launch_ent_sample(d_committed_local, h->cfg.n_scenes, h->cfg.n_local, &d_guess->t_start, (long)sizeof(nep_guess) * h->cfg.n_local, h->cfg.num_pol, h->ent_ns,
                      E.sp.T_span, (double*)((char*)d_block + b.samp), (int*)((char*)d_block + b.present), (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_set_ent_samples(nep_batch_t* h, int32_t ns) {
  if (!h || ns < 1 || ns > 8) return fail(NEP_E_ARG, "ent_samples out of range (1..8)");
  h->ent_ns = ns;
  return 0;
}

int nep_batch_replan_hulls(nep_batch_t* h, const void* d_blocks, int32_t n_blocks, const nep_guess* d_guess, const void* d_ent,
                           nep_solution* d_solution, double* d_states, nep_traj_rec* d_commit, void* stream) {
  if (!h || !d_blocks || !d_guess || !d_solution) return fail(NEP_E_ARG, "null argument");
  ProblemSet ps = round_set(h, d_guess, d_solution, d_states, d_commit, nullptr, d_ent);
  if (int e = use_blocks(ps, h, d_blocks, n_blocks)) return e;
  h->replanned = true;
  return h->eng.run(nullptr, 0, ps, (hipStream_t)stream);
}

// ---- the reference's best-first search (fe_astar.h) ----
int nep_batch_set_fe_astar(nep_batch_t* h, int32_t max_pops, int32_t max_nodes, const int32_t* order, int32_t n_order) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  if (max_pops < 0) return fail(NEP_E_ARG, "max_pops must not be negative");
  if (max_nodes != 0 && (max_nodes < 2 || max_nodes > NEP_FE_ASTAR_MAX_NODES)) return fail(NEP_E_ARG, "max_nodes must be 0 or 2 .. NEP_FE_ASTAR_MAX_NODES");
  if (order) {
    bool square = false;
    for (int ns = 2; ns <= NEP_FE_MAX_SAMPLES; ns++) square |= n_order == ns * ns;
    if (!square) return fail(NEP_E_ARG, "n_order must be num_samples^2 of a lattice (4, 9, 16 or 25)");
    bool seen[NEP_FE_MAX_SAMPLES * NEP_FE_MAX_SAMPLES] = {};
    for (int q = 0; q < n_order; q++) {
      if (order[q] < 0 || order[q] >= n_order || seen[order[q]]) return fail(NEP_E_ARG, "order is not a permutation of 0 .. n_order - 1");
      seen[order[q]] = true;
    }
  }
  Engine& E = h->eng;
  // (no search of max_pops pops creates more than 25 nodes per expansion, the root's included; + 1 because node creation stops one short of the pool)
  const long long dflt = 25LL * ((long long)max_pops + 1) + 1;
  const int pool = max_nodes ? max_nodes : (int)std::min<long long>(NEP_FE_ASTAR_MAX_NODES, dflt);
  int tab = 64; while (tab < 2 * pool) tab *= 2;
  E.as_ready = false;
  if (int e = E.d_as_nodes.ensure((size_t)h->slots * pool * NEP_FE_ASTAR_NODE_BYTES)) return e;
  if (int e = E.d_as_heap.ensure((size_t)h->slots * pool)) return e;
  if (int e = E.d_as_key.ensure((size_t)h->slots * tab)) return e;
  if (int e = E.d_as_val.ensure((size_t)h->slots * tab)) return e;
  if (int e = E.d_as_order.ensure((size_t)NEP_FE_MAX_SAMPLES * NEP_FE_MAX_SAMPLES)) return e;
  if (order) HIPCHK(hipMemcpy(E.d_as_order.p, order, (size_t)n_order * sizeof(int), hipMemcpyHostToDevice));
  E.as_max_pops = max_pops; E.as_pool = pool; E.as_tab = tab; E.as_n_order = order ? n_order : 0;
  E.as_ready = true;
  return 0;
}

// waves per search of nep_batch_frontend_astar_ent (fe_astar.h: frontend_astar_kernel<true>, frontend_astar_team_kernel): a number kept
// on the handle, nothing else — the two forms share every buffer
int nep_batch_set_fe_astar_team(nep_batch_t* h, int32_t waves) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  if (waves != 1 && waves != kAsTeamWaves) return fail(NEP_E_ARG, "nep_batch_set_fe_astar_team: waves must be 1 or 4");
  h->eng.as_team = waves;
  return 0;
}
int nep_batch_fe_astar_team(nep_batch_t* h) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  return h->eng.as_team_last;
}

// budget, order and pools as nep_batch_set_fe_astar left them
static FeAstarArgs fe_astar_args(const Engine& E) {
  FeAstarArgs aa{};
  aa.max_pops = E.as_max_pops; aa.pool = E.as_pool; aa.tab_cap = E.as_tab; aa.order = E.as_n_order ? E.d_as_order.p : nullptr;
  aa.nodes = E.d_as_nodes.p; aa.heap = E.d_as_heap.p; aa.tab_key = E.d_as_key.p; aa.tab_val = E.d_as_val.p;
  return aa;
}

// ---- the reference's move_when_goal_occupied gate (goal_gate.h): between any front-end call and nep_batch_replan ----
int nep_batch_goal_gate(nep_batch_t* h, double half_side, const nep_fe_start* d_start, nep_guess* d_guess, nep_fe_result* d_result,
                        int32_t* d_case, int32_t* d_count, void* stream) {
  if (!h || !d_start || !d_guess || !d_result) return fail(NEP_E_ARG, "null argument");
  if (!std::isfinite(half_side) || !(half_side > 0.0)) return fail(NEP_E_ARG, "nep_batch_goal_gate: half_side must be finite and positive");
  if (h->cfg.n_local != h->cfg.num_agents) return fail(NEP_E_STATE, "nep_batch_goal_gate runs on an unsharded handle (n_local == num_agents)");
  if (h->eng.sp.n_hull != h->cfg.num_agents) return fail(NEP_E_STATE, "nep_batch_goal_gate needs the batched (all-agent) hull layout");
  if (!h->fe_committed) return fail(NEP_E_STATE, "nep_batch_goal_gate: no front-end call has left this round's hulls in the handle's scratch");
  launch_goal_gate(h->slots, h->eng.sp, round_set(h), half_side, d_start, d_guess, d_result, d_case, d_count, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the reference's degrade-to-initial-guess rule (guess_fallback_kernels.hip): behind nep_batch_replan / _solve / _hulls; the tally
// behind nep_batch_fleet_commit ----
int nep_batch_guess_fallback(nep_batch_t* h, const nep_guess* d_guess, nep_solution* d_solution, nep_traj_rec* d_commit, int32_t* d_count, void* stream) {
  if (!h || !d_guess || !d_solution || !d_commit) return fail(NEP_E_ARG, "null argument");
  if (!h->replanned) return fail(NEP_E_STATE, "nep_batch_guess_fallback: no replan has been made on the handle");
  launch_guess_fallback(h->slots, h->eng.sp, h->eng.d_pb.p, d_guess, d_solution, d_commit, d_count, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}
int nep_batch_guess_fallback_tally(nep_batch_t* h, const nep_solution* d_solution, const int32_t* d_outcome, int32_t* d_count, void* stream) {
  if (!h || !d_solution || !d_outcome || !d_count) return fail(NEP_E_ARG, "null argument");
  launch_guess_fallback_tally(h->cfg.n_scenes, h->cfg.n_local, d_solution, d_outcome, d_count, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_set_active(nep_batch_t* h, const int32_t* d_active) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  Engine& E = h->eng;
  if (d_active) {
    if (int e = E.d_act.ensure((size_t)h->slots + 1)) return e;
    if (int e = E.d_fe_act.ensure((size_t)h->slots + 1)) return e;
    if (int e = E.d_safety_recs.ensure((size_t)h->cfg.n_scenes * h->cfg.num_agents)) return e;
  }
  E.active = d_active;
  return 0;
}

// ---- the safety pass, without and with the entangle re-check ----
namespace {
// what both passes start with: the conflict matrices, the round's ProblemSet and, with an active set, the records judged — an inactive
// agent's record this round is its previous one (d_new of it is not read)
int safety_begin(nep_batch* h, const nep_traj_rec* d_prev, const nep_traj_rec*& d_new, const nep_guess* d_guess, ProblemSet& ps, hipStream_t st) {
  Engine& E = h->eng;
  const int N = h->cfg.num_agents;
  if (int e = E.d_conflict.ensure((size_t)h->cfg.n_scenes * N * N)) return e;
  if (E.safety_check_prev) { if (int e = E.d_conflict_prev.ensure((size_t)h->cfg.n_scenes * N * N)) return e; }
  ps = round_set(h, d_guess);
  if (E.active) {
    launch_select_records(h->cfg.n_scenes, N, E.active, d_prev, d_new, E.d_safety_recs.p, st);
    d_new = E.d_safety_recs.p;
  }
  return 0;
}
// ... and end with (d_entangles: the re-check's verdicts, or null)
int safety_end(nep_batch* h, const ProblemSet& ps, const nep_traj_rec* d_prev, const nep_traj_rec* d_new, const int* d_entangles, nep_traj_rec* d_final,
               int32_t* d_accept, hipStream_t st) {
  Engine& E = h->eng;
  launch_safety(d_prev, d_new, h->cfg.n_scenes, h->cfg.num_agents, E.sp, ps, E.d_conflict.p, E.safety_check_prev ? E.d_conflict_prev.p : nullptr, d_entangles, d_final, d_accept, st, E.active);
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace

int nep_batch_safety_commit(nep_batch_t* h, const nep_traj_rec* d_prev, const nep_traj_rec* d_new, const nep_guess* d_guess,
                            nep_traj_rec* d_final, int32_t* d_accept, void* stream) {
  if (!h || !d_prev || !d_new || !d_guess || !d_final) return fail(NEP_E_ARG, "null argument");
  if (h->eng.sp.n_hull != h->cfg.num_agents) return fail(NEP_E_STATE, "safety check needs the batched (all-agent) hull layout");
  ProblemSet ps{};
  if (int e = safety_begin(h, d_prev, d_new, d_guess, ps, (hipStream_t)stream)) return e;
  return safety_end(h, ps, d_prev, d_new, nullptr, d_final, d_accept, (hipStream_t)stream);
}

// ---- entangle check on: front end with per-node entangle states, safety pass with entangleCheckGivenPwp ----
namespace {
// what every entangle-aware call asks of the static representatives (nep_batch_set_static_reps); a handle without static obstacles
// gets placeholders for the kernels' arguments
int ent_ready(nep_batch* h, const char* no_reps = "entangle check with static obstacles needs nep_batch_set_static_reps first") {
  Engine& E = h->eng;
  if (E.sp.n_static > 0 && !E.have_reps) return fail(NEP_E_STATE, no_reps);
  if (E.sp.n_static > 0 && E.d_srep.n < (size_t)(E.sp.static_stride ? h->cfg.n_scenes : 1) * E.sp.n_static * 4) return fail(NEP_E_STATE, "static representatives do not cover every scene's obstacle set: call nep_batch_set_static_reps after nep_batch_set_scene_statics");
  if (!E.d_srep.p) { if (int e = E.d_srep.ensure(4)) return e; if (int e = E.d_slong.ensure(2)) return e; }
  return 0;
}
// what the entangle check reads besides the trajectories' samples, and the threads' working records (beam_width > 0: the beam's node states too)
int ent_common(nep_batch* h, int ns, int beam_width, FeEntArgs& ea) {
  Engine& E = h->eng;
  if (int e = E.d_fe_work.ensure((size_t)std::max(h->slots * 256, h->cfg.n_scenes * h->cfg.num_agents))) return e;
  if (beam_width > 0) { if (int e = E.d_fe_nodes.ensure((size_t)h->slots * (h->cfg.num_pol + 1) * beam_width)) return e; }
  ea.srep = E.d_srep.p; ea.slong = E.d_slong.p; ea.nodes = E.d_fe_nodes.p; ea.work = E.d_fe_work.p; ea.ns = ns;
  ea.fast_cap = E.fe_fast_cap; ea.fast_add = E.fe_fast_add; ea.fast_bend = E.fe_fast_bend;
  return 0;
}
// ... with the samples and presence flags of the records' trajectories (ent_sample_kernel, which zeroes the re-check's pool on its way)
int ent_prepare(nep_batch* h, int ns, int beam_width, const nep_traj_rec* d_recs, const double* ts0, long ts_scene_stride, FeEntArgs& ea, hipStream_t st) {
  Engine& E = h->eng;
  const int N = h->cfg.num_agents, S = h->cfg.n_scenes, np = h->cfg.num_pol;
  if (ns < 1 || ns > 8) return fail(NEP_E_ARG, "ent_samples out of range");
  if (int e = ent_ready(h)) return e;
  if (int e = ent_common(h, ns, beam_width, ea)) return e;
  if (int e = E.d_sampled.ensure((size_t)S * N * np * (ns + 1) * 2)) return e;
  if (int e = E.d_present.ensure((size_t)S * N)) return e;
  {   // the re-check's big records (three times the search's bound: entangleCheckGivenPwp); a sixteenth of the search's pool, at least 256
    const long n_rec = std::max(256L, (E.fe_big_records > 0 ? E.fe_big_records : std::max(4096L, 4L * h->slots)) / 16);
    const size_t rec = (size_t)ent_big_rec_bytes(N, E.sp.n_static, 3);
    if (int e = E.d_fe_big_check.ensure(rec * (size_t)n_rec)) return e;
    if (int e = E.d_fe_big_check_count.ensure(1)) return e;
    ea.big_check = EntBigPool{E.d_fe_big_check.p, E.d_fe_big_check_count.p, (int)n_rec, (int)rec, ent_big_cap(N, E.sp.n_static, 3), ent_big_add_lim(N, E.sp.n_static, 3)};
  }
  launch_ent_sample(d_recs, S, N, ts0, ts_scene_stride, np, ns, E.sp.T_span, E.d_sampled.p, E.d_present.p, st, E.d_fe_big_check_count.p);
  ea.sampled = E.d_sampled.p; ea.present = E.d_present.p;
  return 0;
}
// the packed per-(agent, interval) records of the entangle check (ent_pack_kernel fills them), for ea.ns samples per interval
int ent_packed(nep_batch* h, FeEntArgs& ea) {
  ea.pk_stride = 2 + 2 * kBend + 2 * (ea.ns + 1);      // (kEntPkHead + the samples: an even number of doubles)
  if (int e = h->eng.d_fe_packed.ensure((size_t)h->cfg.n_scenes * h->cfg.num_agents * h->cfg.num_pol * ea.pk_stride)) return e;
  ea.packed = h->eng.d_fe_packed.p;
  return 0;
}
}  // namespace

int nep_batch_set_static_reps(nep_batch_t* h, int32_t scene, const double* rep, const double* longest) {
  if (!h || !rep || !longest || scene < -1 || scene >= h->cfg.n_scenes) return fail(NEP_E_ARG, "bad arguments");
  Engine& E = h->eng;
  const int S = E.sp.n_static;
  if (S == 0) { E.have_reps = true; return 0; }
  const int sets = E.sp.static_stride ? h->cfg.n_scenes : 1;
  HIPCHK(hipDeviceSynchronize());
  if (E.d_srep.n < (size_t)sets * S * 4) {
    DevBuf<double> nr, nl;
    if (int e = nr.ensure((size_t)sets * S * 4)) return e;
    if (int e = nl.ensure((size_t)sets * S * 2)) return e;
    HIPCHK(hipMemset(nr.p, 0, (size_t)sets * S * 4 * sizeof(double))); HIPCHK(hipMemset(nl.p, 0, (size_t)sets * S * 2 * sizeof(double)));
    E.d_srep = std::move(nr); E.d_slong = std::move(nl);
  }
  for (int s = 0; s < sets; s++) {
    if (scene >= 0 && sets > 1 && s != scene) continue;
    HIPCHK(hipMemcpy(E.d_srep.p + (size_t)s * S * 4, rep, (size_t)S * 4 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(E.d_slong.p + (size_t)s * S * 2, longest, (size_t)S * 2 * sizeof(double), hipMemcpyHostToDevice));
  }
  E.have_reps = true;
  return 0;
}

// scratch of the entangle-aware front end: what every surviving child arrived with (kept for the depth's installs: the winners are
// not propagated twice) and the packed per-(agent, interval) records of the entangle check
static int fe_ent_scratch(nep_batch* h, const nep_fe_cfg& cfg, FeEntArgs& ea) {
  Engine& E = h->eng;
  const FeLayout fl = fe_layout(E.sp.num_agents, E.sp.n_static, cfg.beam_width, cfg.num_samples, E.sp.num_pol, true);      // (lds_layout.h)
  const size_t cap = (size_t)fl.z.cap;      // children per depth of one search (beam_width x lattice)
  if (int e = E.d_fe_saved.ensure((size_t)h->slots * cap)) return e;
  if (int e = E.d_fe_arc.ensure((size_t)h->slots * cap)) return e;
  ea.saved = E.d_fe_saved.p; ea.saved_arc = E.d_fe_arc.p;
  if (int e = E.d_fe_stf.ensure((size_t)h->slots * cap)) return e;
  if (int e = E.d_fe_stvox.ensure((size_t)h->slots * cap)) return e;
  ea.st_f = E.d_fe_stf.p; ea.st_vox = E.d_fe_stvox.p;
  {   // where a round's lists of new crossings go when the LDS pool is full (cross_round): one block of kEntAddCap words per (child, step)
    const size_t xw = (size_t)fe_xpool_words(fl, ea.ns);
    if (int e = E.d_fe_xpool.ensure((size_t)h->slots * xw)) return e;
    ea.xpool = E.d_fe_xpool.p; ea.xpool_stride = (int)xw;
  }
  if (int e = ent_packed(h, ea)) return e;
  // the pool of big records: states beyond the fixed record's capacities (rare: a handful of children in a few of 8 192 config-5
  // searches), sized by the reference's own bound on a list (num_agents + statics)
  const int N = h->cfg.num_agents, S = E.sp.n_static;
  const long n_rec = E.fe_big_records > 0 ? E.fe_big_records : std::max(4096L, 4L * h->slots);
  const size_t rec = (size_t)ent_big_rec_bytes(N, S);
  if (int e = E.d_fe_big.ensure(rec * (size_t)n_rec)) return e;
  if (int e = E.d_fe_big_count.ensure(2 + kFeRedoCap)) return e;      // [0] records claimed, [1] searches listed for the big-record instantiation, [2..] the list
  ea.redo_count = E.d_fe_big_count.p + 1; ea.redo_list = E.d_fe_big_count.p + 2; ea.redo_cap = kFeRedoCap;
  if (int e = E.d_fe_big_beta.ensure((size_t)ea.redo_cap * 256 * 120)) return e;      // (kEntBigLdsCap betas per thread of the big-record instantiation: 63 MB)
  ea.big_beta = E.d_fe_big_beta.p;
  ea.big = EntBigPool{E.d_fe_big.p, E.d_fe_big_count.p, (int)n_rec, (int)rec, ent_big_cap(N, S), ent_big_add_lim(N, S)};
  return 0;
}
int nep_batch_set_fe_ent_big_records(nep_batch_t* h, int64_t records) {
  if (!h || records < 0) return fail(NEP_E_ARG, "bad arguments");
  h->eng.fe_big_records = (long)records;
  return 0;
}
int nep_batch_set_fe_ent_fast_caps(nep_batch_t* h, int32_t list_cap, int32_t add_cap, int32_t bend_cap) {
  if (!h || list_cap < 0 || list_cap > NEP_FE_ENT_CAP || add_cap < 0 || add_cap > 32 || bend_cap < 0 || bend_cap > NEP_MAX_BEND) return fail(NEP_E_ARG, "fast-path capacities out of range");
  h->eng.fe_fast_cap = list_cap; h->eng.fe_fast_add = add_cap; h->eng.fe_fast_bend = bend_cap;
  return 0;
}

// ---- the six front-end entry points: one call, told which search, whether the entangle check is on and where its hulls come from ----
namespace {
constexpr bool kBeam = false, kBestFirst = true, kPlain = false, kEnt = true, kRecords = false, kBlocks = true;
struct FeCall {
  const char* who; bool best_first, ent, blocks;      // the entry point (for the error texts); kBeam | kBestFirst; kPlain | kEnt (the check); kRecords | kBlocks (where the hulls come from)
  const nep_fe_cfg* cfg;
  const nep_traj_rec* d_committed; const void* d_blocks; int n_blocks;      // the records (!blocks) or the gathered blocks
  const nep_fe_start* d_start; const nep_fe_ent_state* d_ent_init; nep_guess* d_guess; nep_fe_result* d_result; int32_t* d_case_out; void* stream;
};
// what the entry point asks of its configuration, the handle and the setters' state, in the order it always asked
int fe_call_checks(nep_batch* h, const FeCall& c) {
  const Engine& E = h->eng; const nep_fe_cfg* cfg = c.cfg; const std::string who = c.who;
  const bool unsharded = h->cfg.n_local == h->cfg.num_agents;
  if (!c.best_first) {
    if (!fe_cfg_ok(cfg)) return fail(NEP_E_ARG, "bad front-end configuration");
    if (!c.ent) return 0;
    if (!cfg->enable_entangle || !h->cfg.enable_entangle) return fail(NEP_E_STATE, who + " needs enable_entangle in the front-end configuration and in the handle");
    if (!c.blocks) return unsharded ? 0 : fail(NEP_E_STATE, "the entangle-aware front end runs on an unsharded handle (n_local == num_agents)");
    if (cfg->ent_samples != h->ent_ns) return fail(NEP_E_ARG, "ent_samples differs from what the hull blocks were made with (nep_batch_set_ent_samples)");
    return ent_ready(h);      // (ahead of everything the call changes, as this entry point always had it)
  }
  if (c.ent) {
    if (!h->cfg.enable_entangle) return fail(NEP_E_STATE, who + " needs a handle created with enable_entangle");
    if (!unsharded) return fail(NEP_E_STATE, who + " runs on an unsharded handle (n_local == num_agents)");
    if (!cfg->enable_entangle) return fail(NEP_E_ARG, who + ": enable_entangle must be set in the front-end configuration (without the check: nep_batch_frontend_astar)");
  }
  if (!E.as_ready) return fail(NEP_E_STATE, who + ": call nep_batch_set_fe_astar first (it allocates the searches' pools)");
  if (!c.ent && cfg->enable_entangle) return fail(NEP_E_ARG, who + ": the best-first search has no entangle check (enable_entangle must be 0)");
  if (!fe_cfg_ok(cfg, false)) return fail(NEP_E_ARG, "bad front-end configuration");
  if (E.as_n_order && cfg->num_samples * cfg->num_samples != E.as_n_order) return fail(NEP_E_ARG, who + ": num_samples^2 differs from the n_order of nep_batch_set_fe_astar");
  return 0;
}
// hulls (from the records) -> the searches of every slot; the guesses land where nep_batch_replan reads them.  The
// launches are plan_frontend's (launch_plan.h); every buffer is sized here, at the call (an entry point's first call allocates: eager)
int frontend_call(nep_batch* h, const FeCall& c) {
  if (!h || !c.cfg || !(c.blocks ? c.d_blocks : (const void*)c.d_committed) || !c.d_start || !c.d_guess) return fail(NEP_E_ARG, "null argument");
  Engine& E = h->eng;
  hipStream_t st = (hipStream_t)c.stream;
  ProblemSet ps = round_set(h);
  if (c.blocks) { if (int e = use_blocks(ps, h, c.d_blocks, c.n_blocks)) return e; }      // (the _hulls calls: ahead of the configuration's checks)
  if (int e = fe_call_checks(h, c)) return e;
  // the facts, the plan (launch_plan.h), and the plan followed: hulls, the entangle check's arguments and scratch, the searches
  FrontendFacts f;
  f.num_agents = E.sp.num_agents; f.n_static = E.sp.n_static; f.num_pol = E.sp.num_pol; f.hull_mode = E.sp.hull_mode;
  f.slots = h->slots; f.n_scenes = h->cfg.n_scenes; f.best_first = c.best_first; f.ent = c.ent;
  f.beam_width = c.cfg->beam_width; f.num_samples = c.cfg->num_samples; f.have_recs = !c.blocks; f.active = ps.active && E.d_fe_act.p;
  f.lpt = E.lpt && E.d_fe_order.p; f.order_key_ok = ps.fe_order_key != nullptr; f.fe_history = E.fe_history;
  f.big_beta = c.ent && !c.best_first;      // (fe_ent_scratch below sizes the betas' memory or fails the call)
  f.fe_three = g_debug.fe_three; f.fe_xcd = g_debug.fe_xcd;      // (A/B, nep_debug_set_global_option)
  f.team = E.as_team;
  const FrontendPlan plan = plan_frontend(f);
  h->fe_committed = c.blocks ? nullptr : c.d_committed;
  if (plan.hulls) launch_hulls_ts(c.d_committed, h->cfg.n_scenes, h->cfg.num_agents, &c.d_start->t_start, (long)sizeof(nep_fe_start), E.sp, ps, st, plan.grouped_hulls);
  // the entangle check's arguments: the trajectories' samples and presence flags are made here from the records, or lie in the blocks
  FeEntArgs ea{}; FeAstarEntArgs xa{};
  if (c.ent) {
    const int beam_width = c.best_first ? 0 : c.cfg->beam_width;
    if (plan.ent_sample) { if (int e = ent_prepare(h, c.cfg->ent_samples, beam_width, c.d_committed, &c.d_start->t_start, (long)sizeof(nep_fe_start) * E.sp.n_local, ea, st)) return e; }
    else {
      const HullBlock b = block_of(h);
      if (int e = ent_common(h, h->ent_ns, beam_width, ea)) return e;
      ea.sampled = (const double*)((const char*)c.d_blocks + b.samp); ea.present = (const int*)((const char*)c.d_blocks + b.present);
    }
    ea.init = c.d_ent_init; ea.case_out = c.d_case_out;
    // the searches' scratch: the beam's; the best-first search's packed records, voxel keys' third words and node states
    if (!c.best_first) { if (int e = fe_ent_scratch(h, *c.cfg, ea)) return e; }
    else {
      if (int e = ent_packed(h, ea)) return e;
      if (int e = E.d_as_iz.ensure((size_t)h->slots * E.as_tab)) return e;
      if (int e = E.d_as_states.ensure((size_t)h->slots * E.as_pool * NEP_FE_ASTAR_ENT_NODE_BYTES)) return e;
      xa = FeAstarEntArgs{E.d_as_iz.p, E.d_as_states.p};
    }
  }
  launch_frontend(plan, h->slots, h->cfg.n_scenes, E.sp, ps, *c.cfg, c.best_first ? fe_astar_args(E) : FeAstarArgs{}, xa, ea, c.d_start, c.d_guess, c.d_result, st, E.d_fe_order.p, E.d_fe_act.p);
  E.fe_history = plan.have_history;
  if (plan.kernel == kFeBestFirstEnt) E.as_team_last = plan.team;      // (nep_batch_fe_astar_team; every other call leaves it alone)
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace

int nep_batch_frontend(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start,
                       nep_guess* d_guess, nep_fe_result* d_result, void* stream) {
  return frontend_call(h, FeCall{"nep_batch_frontend", kBeam, kPlain, kRecords, cfg, d_committed, nullptr, 0, d_start, nullptr, d_guess, d_result, nullptr, stream});
}
// the same against all-gathered hull blocks (multi-GPU rounds: nep_batch_hulls -> all-gather -> this -> nep_batch_replan_hulls)
int nep_batch_frontend_hulls(nep_batch_t* h, const nep_fe_cfg* cfg, const void* d_blocks, int32_t n_blocks, const nep_fe_start* d_start,
                             nep_guess* d_guess, nep_fe_result* d_result, void* stream) {
  return frontend_call(h, FeCall{"nep_batch_frontend_hulls", kBeam, kPlain, kBlocks, cfg, nullptr, d_blocks, n_blocks, d_start, nullptr, d_guess, d_result, nullptr, stream});
}
// the front end with per-node entangle states: guesses and the dense case block of nep_batch_replan
int nep_batch_frontend_ent(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start,
                           const nep_fe_ent_state* d_ent_init, nep_guess* d_guess, nep_fe_result* d_result, int32_t* d_case_out, void* stream) {
  return frontend_call(h, FeCall{"nep_batch_frontend_ent", kBeam, kEnt, kRecords, cfg, d_committed, nullptr, 0, d_start, d_ent_init, d_guess, d_result, d_case_out, stream});
}
// the same against all-gathered hull blocks (which carry the samples and the presence flags of every agent's trajectory when the
// handle was created with enable_entangle: nep_batch_hulls): the entangle-aware front end of a sharded handle
int nep_batch_frontend_ent_hulls(nep_batch_t* h, const nep_fe_cfg* cfg, const void* d_blocks, int32_t n_blocks, const nep_fe_start* d_start,
                                 const nep_fe_ent_state* d_ent_init, nep_guess* d_guess, nep_fe_result* d_result, int32_t* d_case_out, void* stream) {
  return frontend_call(h, FeCall{"nep_batch_frontend_ent_hulls", kBeam, kEnt, kBlocks, cfg, nullptr, d_blocks, n_blocks, d_start, d_ent_init, d_guess, d_result, d_case_out, stream});
}
// the reference's best-first search (fe_astar.h) in place of the beam: nep_batch_set_fe_astar's budget, order and pools
int nep_batch_frontend_astar(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start,
                             nep_guess* d_guess, nep_fe_result* d_result, void* stream) {
  return frontend_call(h, FeCall{"nep_batch_frontend_astar", kBestFirst, kPlain, kRecords, cfg, d_committed, nullptr, 0, d_start, nullptr, d_guess, d_result, nullptr, stream});
}
// ... with the entangle check: nep_batch_frontend_ent's inputs, plus a state per node and the voxel key's third word
int nep_batch_frontend_astar_ent(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start,
                                 const nep_fe_ent_state* d_ent_init, nep_guess* d_guess, nep_fe_result* d_result, int32_t* d_case_out, void* stream) {
  return frontend_call(h, FeCall{"nep_batch_frontend_astar_ent", kBestFirst, kEnt, kRecords, cfg, d_committed, nullptr, 0, d_start, d_ent_init, d_guess, d_result, d_case_out, stream});
}

int nep_batch_safety_commit_ent(nep_batch_t* h, const nep_traj_rec* d_prev, const nep_traj_rec* d_new, const nep_guess* d_guess,
                                const nep_fe_ent_state* d_ent_init, int32_t ent_samples, double cable_length, nep_traj_rec* d_final,
                                int32_t* d_accept, void* stream) {
  if (!h || !d_prev || !d_new || !d_guess || !d_final) return fail(NEP_E_ARG, "null argument");
  Engine& E = h->eng;
  const int N = h->cfg.num_agents;
  if (E.sp.n_hull != N) return fail(NEP_E_STATE, "the entangle re-check needs the batched (all-agent) hull layout");
  if (!h->cfg.enable_entangle) return fail(NEP_E_STATE, "handle created without enable_entangle");
  if (int e = E.d_entangles.ensure((size_t)h->cfg.n_scenes * N)) return e;
  ProblemSet ps{};
  if (int e = safety_begin(h, d_prev, d_new, d_guess, ps, (hipStream_t)stream)) return e;
  // everybody's NEW trajectory counts as received while optimising: their samples and bend points feed the re-check
  FeEntArgs ea{};
  if (int e = ent_prepare(h, ent_samples, 0, d_new, &d_guess->t_start, (long)sizeof(nep_guess) * E.sp.n_local, ea, (hipStream_t)stream)) return e;
  ea.init = d_ent_init;
  if (int e = ent_packed(h, ea)) return e;
  launch_hulls(d_new, h->cfg.n_scenes, N, d_guess, E.sp, ps, (hipStream_t)stream, grouped_hulls(E.sp, h->cfg.n_scenes, N));     // (with the bend points: ent_enabled)
  launch_ent_check(E.sp, ps, ea, d_new, h->cfg.n_scenes, cable_length, E.d_entangles.p, (hipStream_t)stream);
  return safety_end(h, ps, d_prev, d_new, E.d_entangles.p, d_final, d_accept, (hipStream_t)stream);
}

namespace {
bool ent_lists_cap_ok(int cap) { return cap > NEP_FE_ENT_CAP && cap <= NEP_ENT_LISTS_MAX_CAP; }
bool ent_lists_complete(const nep_ent_lists* l) { return l->n_alpha && l->n_bend && l->id && l->cs && l->beta && l->bend; }
// nep_batch_track_ent / nep_batch_track_ent_lists: the state in d_ent (the fixed record) or in *lists
int track_ent_round(nep_batch_t* h, const nep_traj_rec* d_prev, nep_traj_rec* d_records, const nep_guess* d_guess, int32_t n_intervals,
                    int32_t ent_samples, double cable_length, nep_fe_ent_state* d_ent, const nep_ent_lists* lists, int32_t* d_flags, void* stream) {
  if (!h || !d_prev || !d_records || !d_guess || (!d_ent && !lists)) return fail(NEP_E_ARG, "null argument");
  if (lists && !ent_lists_complete(lists)) return fail(NEP_E_ARG, "null array in nep_ent_lists");
  if (n_intervals < 1 || n_intervals > h->cfg.num_pol) return fail(NEP_E_ARG, "n_intervals out of range (1..num_pol)");
  if (ent_samples < 1 || ent_samples > 8) return fail(NEP_E_ARG, "ent_samples out of range (1..8)");
  if (!h->cfg.enable_entangle) return fail(NEP_E_STATE, "handle created without enable_entangle");
  if (h->cfg.n_local != h->cfg.num_agents) return fail(NEP_E_STATE, "tether tracking runs on an unsharded handle (n_local == num_agents)");
  Engine& E = h->eng;
  const int N = h->cfg.num_agents, S = h->cfg.n_scenes, np = h->cfg.num_pol;
  if (int e = ent_ready(h, "tether tracking with static obstacles needs nep_batch_set_static_reps first")) return e;
  if (!fleet_ent_fits(N, E.sp.n_static)) return fail(NEP_E_CAP, "the tether kernels take up to 4096 agents and 2048 static obstacles per scene");
  if (lists && !ent_lists_cap_ok(lists->cap)) return fail(NEP_E_CAP, "nep_ent_lists: cap out of range (NEP_FE_ENT_CAP < cap <= NEP_ENT_LISTS_MAX_CAP)");
  const ProblemSet ps = round_set(h);
  if (int e = E.d_sampled.ensure((size_t)S * N * np * (ent_samples + 1) * 2)) return e;
  if (int e = E.d_present.ensure((size_t)S * N)) return e;
  if (lists) { if (E.d_track_lsave.cap < lists->cap) if (int e = E.d_track_lsave.ensure((size_t)S * N, lists->cap)) return e; }
  else if (int e = E.d_track_save.ensure((size_t)S * N)) return e;
  if (int e = E.d_track_flags.ensure((size_t)S * N)) return e;      // (whether or not this call passes d_flags: a later captured call may not)
  if (int e = E.d_track_pos.ensure((size_t)S * N * ((size_t)np * 8 + 1) * 2)) return e;      // (the largest call's: a later captured one may fly more steps)
  launch_ent_sample(d_records, S, N, &d_guess->t_start, (long)sizeof(nep_guess) * h->cfg.n_local, np, ent_samples, E.sp.T_span, E.d_sampled.p, E.d_present.p,
                    (hipStream_t)stream, nullptr);
  // the round's sampled steps side by side, the moves on them (the other agents' lists at the previous check: the previous round's
  // records), then the bend points of the states just tracked into the flown records
  TetherArgs ea{};
  ea.N = N; ea.S = E.sp.n_static; ea.n_scenes = S; ea.static_stride = E.sp.static_stride; ea.num_pol = np; ea.ns = ent_samples;
  ea.n_steps = n_intervals * ent_samples; ea.proof = E.opt_fleet_ent_proof; ea.skip_absent = 1; ea.cable = cable_length; ea.T_span = E.sp.T_span;
  ea.pb = ps.pb; ea.srep = E.d_srep.p; ea.slong = E.d_slong.p; ea.pos = E.d_track_pos.p; ea.sampled = E.d_sampled.p;
  ea.recs = d_records; ea.recs_out = d_records;
  ea.prev_n = (const char*)&d_prev->n_bend; ea.prev_xy = (const char*)&d_prev->bend[0][0]; ea.prev_n_stride = ea.prev_xy_stride = (long)sizeof(nep_traj_rec);
  ea.in = d_ent; ea.out = d_ent; ea.save = E.d_track_save.p; ea.flags = d_flags ? d_flags : E.d_track_flags.p; ea.gflags = ps.flags;
  if (lists) { ea.lists = *lists; ea.lsave = E.d_track_lsave.view(); ea.lsave.cap = lists->cap; }      // (the scratch is indexed at the call's cap)
  if (h->tether_audit) {      // one tick per sampled step, from the scene's t_start (the first agent's, as the sampling reads it)
    ea.audit = h->tether_audit; ea.audit_t0 = (const char*)&d_guess->t_start; ea.audit_t0_stride = (long)sizeof(nep_guess) * N;
    ea.audit_dt = h->tether_audit_dt > 0.0 ? h->tether_audit_dt : E.sp.T_span / ent_samples;
  }
  launch_tether_steps(ea, FleetArgs{}, (hipStream_t)stream);
  launch_tether_publish(ea, false, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace

int nep_batch_track_ent(nep_batch_t* h, const nep_traj_rec* d_prev, nep_traj_rec* d_records, const nep_guess* d_guess, int32_t n_intervals,
                        int32_t ent_samples, double cable_length, nep_fe_ent_state* d_ent, int32_t* d_flags, void* stream) {
  if (!d_ent) return fail(NEP_E_ARG, "null argument");
  return track_ent_round(h, d_prev, d_records, d_guess, n_intervals, ent_samples, cable_length, d_ent, nullptr, d_flags, stream);
}

int nep_batch_track_ent_lists(nep_batch_t* h, const nep_traj_rec* d_prev, nep_traj_rec* d_records, const nep_guess* d_guess, int32_t n_intervals,
                              int32_t ent_samples, double cable_length, const nep_ent_lists* d_lists, int32_t* d_flags, void* stream) {
  if (!d_lists) return fail(NEP_E_ARG, "null argument");
  return track_ent_round(h, d_prev, d_records, d_guess, n_intervals, ent_samples, cable_length, nullptr, d_lists, d_flags, stream);
}

int nep_batch_set_tether_audit(nep_batch_t* h, nep_tether_audit* d_audit, double dt) {
  if (!h || !(dt >= 0.0)) return fail(NEP_E_ARG, "bad arguments");
  if (h->cfg.n_local != h->cfg.num_agents) return fail(NEP_E_STATE, "tether tracking runs on an unsharded handle (n_local == num_agents)");
  h->tether_audit = d_audit; h->tether_audit_dt = d_audit ? dt : 0.0;
  return 0;
}

int nep_batch_ent_lists_at_a(nep_batch_t* h, const nep_ent_lists* d_lists, nep_fe_ent_state* d_ent_a, int32_t* d_flags_a, const int32_t* d_mask_in,
                             int32_t* d_mask_out, int32_t* d_held, void* stream) {
  if (!h || !d_lists || !d_ent_a || !d_mask_out) return fail(NEP_E_ARG, "null argument");
  if (!ent_lists_complete(d_lists)) return fail(NEP_E_ARG, "null array in nep_ent_lists");
  if (!h->cfg.enable_entangle) return fail(NEP_E_STATE, "handle created without enable_entangle");
  if (h->cfg.n_local != h->cfg.num_agents) return fail(NEP_E_STATE, "tether tracking runs on an unsharded handle (n_local == num_agents)");
  if (!ent_lists_cap_ok(d_lists->cap)) return fail(NEP_E_CAP, "nep_ent_lists: cap out of range (NEP_FE_ENT_CAP < cap <= NEP_ENT_LISTS_MAX_CAP)");
  TetherArgs ea{};
  ea.N = h->cfg.num_agents; ea.n_scenes = h->cfg.n_scenes; ea.lists = *d_lists; ea.out = d_ent_a; ea.flags = d_flags_a; ea.held = d_held; ea.hold_mask = d_mask_out;
  launch_ent_lists_at_a(ea, d_mask_in, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_audit(nep_batch_t* h, const nep_traj_rec* d_records, const nep_fe_start* d_start, double tick, int32_t n_ticks, nep_audit* d_audit,
                    void* stream) {
  if (!h || !d_records || !d_start || !d_audit || n_ticks < 0 || !(tick >= 0.0)) return fail(NEP_E_ARG, "bad arguments");
  if (h->cfg.n_local != h->cfg.num_agents) return fail(NEP_E_STATE, "the flight audit runs on an unsharded handle (n_local == num_agents)");
  Engine& E = h->eng;
  const int N = h->cfg.num_agents, S = h->cfg.n_scenes;
  if (N > 1024) return fail(NEP_E_CAP, "the flight audit takes up to 1024 agents per scene");
  const int vs = E.sp.n_static > 0 ? std::max(E.static_nv_max, 1) : 1;
  if (audit_layout(N, E.sp.n_static, vs).bytes > 64 * 1024) return fail(NEP_E_CAP, "the flight audit's agents and static polygons do not fit into 64 KB of LDS");
  if (int e = E.d_audit_part.ensure((size_t)S * nep_audit_impl::kAuditMaxChunks * N)) return e;      // (before the n_ticks == 0 return: the first call allocates)
  if (n_ticks == 0) return 0;
  const ProblemSet ps = round_set(h);
  AuditArgs aa{};
  aa.N = N; aa.S = E.sp.n_static; aa.n_scenes = S; aa.static_stride = E.sp.static_stride; aa.vstride = vs; aa.n_ticks = n_ticks;
  aa.chunk_len = nep_audit_impl::audit_chunk_len(n_ticks); aa.n_chunks = (n_ticks + aa.chunk_len - 1) / aa.chunk_len;
  aa.tick = tick; aa.drone_radius = E.sp.drone_radius;
  aa.recs = d_records; aa.starts = d_start; aa.static_xy = ps.static_xy; aa.static_nv = ps.static_nv; aa.part = E.d_audit_part.p; aa.out = d_audit;
  launch_audit(aa, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_audit_span(nep_batch_t* h, const nep_traj_rec* d_records, const nep_fe_start* d_start, double tick, int32_t n_ticks,
                         nep_span_audit* d_span, void* stream) {
  if (!h || !d_records || !d_start || !d_span || n_ticks < 0 || !(tick >= 0.0 && tick < HUGE_VAL)) return fail(NEP_E_ARG, "bad arguments");
  if (h->cfg.n_local != h->cfg.num_agents) return fail(NEP_E_STATE, "the span audit runs on an unsharded handle (n_local == num_agents)");
  Engine& E = h->eng;
  const int N = h->cfg.num_agents, S = h->cfg.n_scenes;
  const int vs = E.sp.n_static > 0 ? std::max(E.static_nv_max, 1) : 1;
  const long long lds = span_audit_lds_bytes(N, E.sp.n_static, vs);
  if (lds > kLdsPerCu) return fail(NEP_E_CAP, "the span audit's agents and static polygons do not fit into 160 KB of LDS");
  HIPCHK(prepare_audit_span(lds));      // (before the n_ticks == 0 return: what the first call has to set up; there is no scratch to allocate)
  if (n_ticks == 0) return 0;
  const ProblemSet ps = round_set(h);
  SpanAuditArgs sa{};
  sa.N = N; sa.S = E.sp.n_static; sa.n_scenes = S; sa.static_stride = E.sp.static_stride; sa.vstride = vs; sa.n_ticks = n_ticks;
  sa.tick = tick; sa.drone_radius = E.sp.drone_radius;
  sa.recs = d_records; sa.starts = d_start; sa.static_xy = ps.static_xy; sa.static_nv = ps.static_nv; sa.out = d_span;
  launch_audit_span(sa, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the committed plans on the device (include/neptune_fleet.h; kernels: fleet_kernels.hip) ----
namespace {
// a null handle without a device is "no device" (nothing could have made a handle), with one it is a bad argument
int fleet_guard(nep_batch_t* h, bool need_ready) {
  if (!h) return have_device() ? fail(NEP_E_ARG, "null handle") : fail(NEP_E_HIP, "no HIP device: the back end has no CPU path");
  if (h->cfg.n_local != h->cfg.num_agents) return fail(NEP_E_STATE, "the fleet state lives on an unsharded handle (n_local == num_agents)");
  if (need_ready && !h->fleet.ready) return fail(NEP_E_STATE, "nep_batch_fleet_init has not run on this handle");
  return 0;
}
void fleet_args(nep_batch_t* h, FleetArgs& fa) {
  nep_batch::Fleet& F = h->fleet;
  fa.N = h->cfg.num_agents; fa.n_scenes = h->cfg.n_scenes; fa.cap = F.cap; fa.max_states = h->cfg.max_states; fa.cfg = F.cfg;
  fa.drone_radius = h->eng.sp.drone_radius; fa.pb = h->eng.d_pb.p;
  fa.ring = F.ring.p; fa.head = F.head.p; fa.size = F.size.p; fa.k_end = F.k_end.p; fa.state = F.state.p; fa.goal = F.goal.p; fa.pwp = F.pwp.p;
  fa.flown = F.flown.p; fa.done = F.done.p; fa.outcome = F.outcome.p; fa.sflags = F.sflags.p;
  fa.period = F.timers ? F.period.p : nullptr; fa.phase = F.timers ? F.phase.p : nullptr;
  fa.t_now = F.t_now.p; fa.round = F.round.p; fa.origin = F.origin.p; fa.counters = F.counters.p; fa.gflags = h->eng.d_flags.p; fa.active = h->eng.active;
}
void fleet_ent_args(nep_batch_t* h, TetherArgs& ea) {
  nep_batch::Fleet& F = h->fleet; Engine& E = h->eng;
  ea.N = h->cfg.num_agents; ea.S = E.sp.n_static; ea.n_scenes = h->cfg.n_scenes; ea.static_stride = E.sp.static_stride; ea.num_pol = h->cfg.num_pol;
  ea.n_steps = F.cfg.round_ticks; ea.proof = E.opt_fleet_ent_proof; ea.cable = F.cable; ea.T_span = E.sp.T_span;
  ea.pb = E.d_pb.p; ea.srep = E.d_srep.p; ea.slong = E.d_slong.p; ea.pos = F.ent_pos.p;
  ea.pub_n = F.pub_n.p; ea.pub_xy = F.pub_xy.p; ea.pub_prev_n = F.pub_prev_n.p; ea.pub_prev_xy = F.pub_prev_xy.p;
  ea.prev_n = (const char*)F.pub_prev_n.p; ea.prev_n_stride = (long)sizeof(int); ea.prev_xy = (const char*)F.pub_prev_xy.p; ea.prev_xy_stride = (long)sizeof(double) * NEP_MAX_BEND * 2;
  ea.in = F.ent.p; ea.out = F.ent.p; ea.save = F.ent_save.p; ea.flags = F.ent_flags.p; ea.ever = F.ent_ever.p; ea.walked = F.ent_walked.p;
  ea.counters = F.counters.p; ea.gflags = E.d_flags.p;
  if (F.ent_cap) { ea.lists = F.ent_lists.view(); ea.lists.cap = F.ent_cap; ea.lsave = F.ent_lsave.view(); ea.lsave.cap = F.ent_cap; }
}
}  // namespace

int nep_batch_fleet_init(nep_batch_t* h, const nep_fleet_cfg* cfg, const double* d_state0, const double* d_goal, const int32_t* d_period,
                         const int32_t* d_phase, void* stream) {
  if (int e = fleet_guard(h, false)) return e;
  if (!cfg || !d_state0 || !d_goal || (d_period == nullptr) != (d_phase == nullptr)) return fail(NEP_E_ARG, "null argument (period and phase come together)");
  if (!(cfg->dc > 0.0) || !(cfg->T_span > 0.0) || cfg->deltaT0 < 1 || cfg->round_ticks < 1 || cfg->ring_cap < 0 || cfg->k_a < 0) return fail(NEP_E_ARG, "bad fleet configuration");
  nep_batch::Fleet& F = h->fleet;
  const size_t slots = (size_t)h->slots, S = (size_t)h->cfg.n_scenes;
  const int cap = cfg->ring_cap > 0 ? cfg->ring_cap : cfg->deltaT0 + h->cfg.max_states;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));      // (a re-seed: kernels of the previous flight may still read the state)
  F.ready = false; F.ent_ready = false;      // (a re-seeded fleet flies untethered until nep_batch_fleet_init_ent runs again)
  F.mis_ready = false;                       // (and without missions until nep_batch_fleet_mission_init does)
  if (int e = F.ring.ensure(slots * cap * 12)) return e;
  if (int e = F.state.ensure(slots * 12)) return e;
  if (int e = F.goal.ensure(slots * 3)) return e;
  if (int e = F.pwp.ensure(slots)) return e;
  if (int e = F.t_now.ensure(S)) return e;
  if (int e = F.round.ensure(S)) return e;
  if (int e = F.origin.ensure(S)) return e;
  if (int e = F.counters.ensure(S * NEP_FLEET_N_COUNTERS)) return e;
  for (DevBuf<int>* b : {&F.head, &F.size, &F.k_end, &F.flown, &F.done, &F.outcome, &F.sflags, &F.period, &F.phase})
    if (int e = b->ensure(slots)) return e;
  F.cap = cap; F.cfg = *cfg; F.timers = d_period != nullptr;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(F.ring.p, 0, slots * cap * 12 * sizeof(double), st));      // (a snapshot copies the rings raw: the entries no plan has reached yet are zeros)
  HIPCHK(hipMemcpyAsync(F.goal.p, d_goal, slots * 3 * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (F.timers) {
    HIPCHK(hipMemcpyAsync(F.period.p, d_period, slots * sizeof(int), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(F.phase.p, d_phase, slots * sizeof(int), hipMemcpyDeviceToDevice, st));
  }
  FleetArgs fa{};
  fleet_args(h, fa);
  launch_fleet_seed(fa, d_state0, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  F.ready = true;
  return 0;
}

int nep_batch_fleet_select(nep_batch_t* h, nep_fe_start* d_start, nep_traj_rec* d_records, int32_t* d_active, nep_fe_start* d_clock, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!d_start || !d_records) return fail(NEP_E_ARG, "null argument");
  h->fleet.saw(stream);
  FleetArgs fa{};
  fleet_args(h, fa);
  fa.start = d_start; fa.recs = d_records; fa.active_out = d_active; fa.clock = d_clock;
  launch_fleet_select(fa, (hipStream_t)stream);
  if (h->fleet.ent_ready) {      // the tethered fleet publishes its bend points (publishOwnTraj)
    TetherArgs ea{};
    fleet_ent_args(h, ea);
    ea.recs = d_records; ea.recs_out = d_records;
    launch_tether_publish(ea, true, (hipStream_t)stream);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

namespace {
// nep_batch_fleet_init_ent / nep_batch_fleet_init_ent_lists: the state from d_ent0 (device, fixed records; null = empty) or, with
// host_lists, from host arrays in the list form (null arrays = empty)
int fleet_init_ent_any(nep_batch_t* h, double cable_length, const nep_fe_ent_state* d_ent0, const nep_ent_lists* host_lists, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!h->cfg.enable_entangle) return fail(NEP_E_STATE, "handle created without enable_entangle");
  Engine& E = h->eng;
  if (int e = ent_ready(h, "the fleet's tethers with static obstacles need nep_batch_set_static_reps first")) return e;
  if (!fleet_ent_fits(h->cfg.num_agents, E.sp.n_static)) return fail(NEP_E_CAP, "the fleet's tether kernels take up to 4096 agents and 2048 static obstacles per scene");
  if (!(cable_length > 0.0)) return fail(NEP_E_ARG, "cable_length must be positive");
  const int cap = host_lists ? host_lists->cap : 0;
  if (host_lists && !ent_lists_cap_ok(cap)) return fail(NEP_E_CAP, "nep_ent_lists: cap out of range (NEP_FE_ENT_CAP < cap <= NEP_ENT_LISTS_MAX_CAP)");
  const bool seeded = host_lists && (host_lists->n_alpha || host_lists->n_bend || host_lists->id || host_lists->cs || host_lists->beta || host_lists->bend);
  if (seeded && !ent_lists_complete(host_lists)) return fail(NEP_E_ARG, "nep_ent_lists: all arrays or none");
  nep_batch::Fleet& F = h->fleet;
  const size_t slots = (size_t)h->slots;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(st));
  F.ent_ready = false; F.ent_cap = 0;
  if (cap) {
    if (F.ent_lists.cap < cap) if (int e = F.ent_lists.ensure(slots, cap)) return e;
    if (F.ent_lsave.cap < cap) if (int e = F.ent_lsave.ensure(slots, cap)) return e;
    if (int e = F.ent_held.ensure(slots)) return e;
    for (ListBuf* b : {&F.ent_lists, &F.ent_lsave}) {
      HIPCHK(hipMemsetAsync(b->n_alpha.p, 0, slots * sizeof(int), st)); HIPCHK(hipMemsetAsync(b->n_bend.p, 0, slots * sizeof(int), st));
      HIPCHK(hipMemsetAsync(b->id.p, 0, slots * cap * sizeof(int16_t), st)); HIPCHK(hipMemsetAsync(b->cs.p, 0, slots * cap, st));
      HIPCHK(hipMemsetAsync(b->beta.p, 0, slots * cap * sizeof(double), st)); HIPCHK(hipMemsetAsync(b->bend.p, 0, slots * NEP_MAX_BEND * sizeof(int16_t), st));
    }
    HIPCHK(hipMemsetAsync(F.ent_held.p, 0, slots * sizeof(int), st));
    if (seeded) {
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(F.ent_lists.n_alpha.p, host_lists->n_alpha, slots * sizeof(int), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(F.ent_lists.n_bend.p, host_lists->n_bend, slots * sizeof(int), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(F.ent_lists.id.p, host_lists->id, slots * cap * sizeof(int16_t), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(F.ent_lists.cs.p, host_lists->cs, slots * cap, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(F.ent_lists.beta.p, host_lists->beta, slots * cap * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(F.ent_lists.bend.p, host_lists->bend, slots * NEP_MAX_BEND * sizeof(int16_t), hipMemcpyHostToDevice));
    }
  }
  if (int e = F.ent.ensure(slots)) return e;
  if (int e = F.ent_save.ensure(slots)) return e;
  if (int e = F.pub_xy.ensure(slots * NEP_MAX_BEND * 2)) return e;
  if (int e = F.pub_prev_xy.ensure(slots * NEP_MAX_BEND * 2)) return e;
  if (int e = F.ent_pos.ensure(slots * ((size_t)F.cfg.round_ticks + 1) * 2)) return e;
  for (DevBuf<int>* b : {&F.pub_n, &F.pub_prev_n, &F.ent_flags, &F.ent_ever, &F.ent_walked, &F.ent_flags_a})
    if (int e = b->ensure(slots)) return e;
  if (d_ent0) HIPCHK(hipMemcpyAsync(F.ent.p, d_ent0, slots * sizeof(nep_fe_ent_state), hipMemcpyDeviceToDevice, st));
  else HIPCHK(hipMemsetAsync(F.ent.p, 0, slots * sizeof(nep_fe_ent_state), st));
  HIPCHK(hipMemsetAsync(F.ent_save.p, 0, slots * sizeof(nep_fe_ent_state), st));
  HIPCHK(hipMemsetAsync(F.pub_xy.p, 0, slots * NEP_MAX_BEND * 2 * sizeof(double), st));
  HIPCHK(hipMemsetAsync(F.pub_prev_xy.p, 0, slots * NEP_MAX_BEND * 2 * sizeof(double), st));
  for (DevBuf<int>* b : {&F.pub_n, &F.pub_prev_n, &F.ent_flags, &F.ent_ever, &F.ent_walked, &F.ent_flags_a})
    HIPCHK(hipMemsetAsync(b->p, 0, slots * sizeof(int), st));
  HIPCHK(hipStreamSynchronize(st));
  F.cable = cable_length; F.ent_cap = cap; F.ent_ready = true;
  return 0;
}
}  // namespace

int nep_batch_fleet_init_ent(nep_batch_t* h, double cable_length, const nep_fe_ent_state* d_ent0, void* stream) {
  return fleet_init_ent_any(h, cable_length, d_ent0, nullptr, stream);
}

int nep_batch_fleet_init_ent_lists(nep_batch_t* h, double cable_length, const nep_ent_lists* host_lists, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!host_lists) return fail(NEP_E_ARG, "null argument");
  return fleet_init_ent_any(h, cable_length, nullptr, host_lists, stream);
}

int nep_batch_fleet_predict_ent(nep_batch_t* h, const nep_fe_start* d_start, const nep_traj_rec* d_records, nep_fe_ent_state* d_ent_a,
                                int32_t* d_flags_a, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!h->fleet.ent_ready) return fail(NEP_E_STATE, "nep_batch_fleet_init_ent has not run on this handle");
  if (!d_start || !d_records || !d_ent_a) return fail(NEP_E_ARG, "null argument");
  if (h->fleet.ent_cap && !h->eng.active) return fail(NEP_E_STATE, "a prediction in the list form needs the round's mask (nep_batch_set_active): a state that does not fit the fixed record holds its slot");
  FleetArgs fa{};
  fleet_args(h, fa);
  TetherArgs ea{};
  fleet_ent_args(h, ea);
  if (h->fleet.ent_cap) { ea.held = h->fleet.ent_held.p; ea.hold_mask = const_cast<int*>(h->eng.active); }
  ea.n_steps = 1; ea.start = d_start; ea.recs = d_records; ea.out = d_ent_a; ea.flags = d_flags_a ? d_flags_a : h->fleet.ent_flags_a.p;
  ea.prev_n = nullptr; ea.prev_xy = nullptr; ea.ever = nullptr; ea.walked = nullptr; ea.counters = nullptr;
  launch_tether_steps(ea, fa, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_fleet_track_ent(nep_batch_t* h, const nep_traj_rec* d_records, int32_t* d_flags, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!h->fleet.ent_ready) return fail(NEP_E_STATE, "nep_batch_fleet_init_ent has not run on this handle");
  if (!d_records) return fail(NEP_E_ARG, "null argument");
  FleetArgs fa{};
  fleet_args(h, fa);
  TetherArgs ea{};
  fleet_ent_args(h, ea);
  ea.n_steps = h->fleet.cfg.round_ticks; ea.start = nullptr; ea.recs = d_records; ea.out = h->fleet.ent.p;
  ea.flags = d_flags ? d_flags : h->fleet.ent_flags.p;
  if (h->tether_audit) {      // one tick per control tick, from the scene's fleet clock
    ea.audit = h->tether_audit; ea.audit_t0 = (const char*)h->fleet.t_now.p; ea.audit_t0_stride = (long)sizeof(double);
    ea.audit_dt = h->tether_audit_dt > 0.0 ? h->tether_audit_dt : h->fleet.cfg.dc;
  }
  launch_tether_steps(ea, fa, (hipStream_t)stream);
  if (d_flags) HIPCHK(hipMemcpyAsync(h->fleet.ent_flags.p, d_flags, (size_t)h->slots * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  HIPCHK(hipGetLastError());
  return 0;
}

namespace {
int fleet_lists_to_host(const ListBuf& B, size_t slots, size_t cap, nep_ent_lists* out) {
  HIPCHK(hipMemcpy(out->n_alpha, B.n_alpha.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out->n_bend, B.n_bend.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out->id, B.id.p, slots * cap * sizeof(int16_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out->cs, B.cs.p, slots * cap, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out->beta, B.beta.p, slots * cap * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out->bend, B.bend.p, slots * NEP_MAX_BEND * sizeof(int16_t), hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace

// the handle's tether states in the list form (blocking): host_out's arrays of host_out->cap == the handle's cap entries per slot
int nep_batch_fleet_ent_lists(nep_batch_t* h, nep_ent_lists* host_out, int32_t* held_rounds_out) {
  if (int e = fleet_guard(h, true)) return e;
  nep_batch::Fleet& F = h->fleet;
  if (!F.ent_ready || !F.ent_cap) return fail(NEP_E_STATE, "nep_batch_fleet_init_ent_lists has not run on this handle");
  if (host_out && (host_out->cap != F.ent_cap || !ent_lists_complete(host_out))) return fail(NEP_E_ARG, "host_out: cap must be the handle's, every array present");
  HIPCHK(hipDeviceSynchronize());
  if (host_out) if (int e = fleet_lists_to_host(F.ent_lists, (size_t)h->slots, (size_t)F.ent_cap, host_out)) return e;
  if (held_rounds_out) HIPCHK(hipMemcpy(held_rounds_out, F.ent_held.p, (size_t)h->slots * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int nep_batch_fleet_ent_state(nep_batch_t* h, nep_fe_ent_state* states_out, int32_t* flags_round_out, int32_t* flags_ever_out, int32_t* walked_out) {
  if (int e = fleet_guard(h, true)) return e;
  nep_batch::Fleet& F = h->fleet;
  if (!F.ent_ready) return fail(NEP_E_STATE, "nep_batch_fleet_init_ent has not run on this handle");
  const size_t slots = (size_t)h->slots;
  HIPCHK(hipDeviceSynchronize());
  if (states_out && F.ent_cap) {      // the list form: the slots that fit as fixed records, the others marked n_alpha = -1
    const size_t cap = (size_t)F.ent_cap;
    std::vector<int> na(slots), nb(slots); std::vector<int16_t> id(slots * cap), bend(slots * NEP_MAX_BEND); std::vector<int8_t> cs(slots * cap); std::vector<double> beta(slots * cap);
    nep_ent_lists hl{}; hl.cap = F.ent_cap; hl.n_alpha = na.data(); hl.n_bend = nb.data(); hl.id = id.data(); hl.cs = cs.data(); hl.beta = beta.data(); hl.bend = bend.data();
    if (int e = fleet_lists_to_host(F.ent_lists, slots, cap, &hl)) return e;
    std::memset(states_out, 0, slots * sizeof(nep_fe_ent_state));
    for (size_t s = 0; s < slots; s++) {
      nep_fe_ent_state& o = states_out[s];
      if (na[s] < 0 || na[s] > NEP_FE_ENT_CAP || nb[s] < 0 || nb[s] > NEP_MAX_BEND) { o.n_alpha = -1; continue; }
      o.n_alpha = na[s]; o.n_bend = nb[s];
      for (int i = 0; i < na[s]; i++) { o.id[i] = id[s * cap + i]; o.cs[i] = cs[s * cap + i]; o.beta[i] = beta[s * cap + i]; }
      for (int i = 0; i < nb[s]; i++) o.bend[i] = (int8_t)bend[s * NEP_MAX_BEND + i];
    }
  } else
  if (states_out) HIPCHK(hipMemcpy(states_out, F.ent.p, slots * sizeof(nep_fe_ent_state), hipMemcpyDeviceToHost));
  if (flags_round_out) HIPCHK(hipMemcpy(flags_round_out, F.ent_flags.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  if (flags_ever_out) HIPCHK(hipMemcpy(flags_ever_out, F.ent_ever.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  if (walked_out) HIPCHK(hipMemcpy(walked_out, F.ent_walked.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

// ---- missions (include/neptune_fleet.h; kernels: fleet_mission_kernels.hip; host form: mission_host.cpp) ----
namespace {
int mission_keep_ensure(nep_batch_t* h) {
  nep_batch::Fleet& F = h->fleet;
  const size_t S = (size_t)h->cfg.n_scenes;
  if (F.keep_n.p) return 0;
  if (int e = F.keep_n.ensure(S)) return e;
  if (int e = F.keep_off.ensure(S * (NEP_MISSION_MAX_POLY + 1))) return e;
  if (int e = F.keep_xy.ensure(S * NEP_MISSION_MAX_VERT * 2)) return e;
  HIPCHK(hipMemset(F.keep_n.p, 0, S * sizeof(int)));
  HIPCHK(hipMemset(F.keep_off.p, 0, S * (NEP_MISSION_MAX_POLY + 1) * sizeof(int)));
  HIPCHK(hipMemset(F.keep_xy.p, 0, S * NEP_MISSION_MAX_VERT * 2 * sizeof(double)));
  return 0;
}
// the kernel's dynamic LDS, sized once per handle for the largest keep-out set a scene can hold: a captured graph keeps the size
// it was captured with, whatever is uploaded later
size_t mission_lds_need(nep_batch_t* h) { return (size_t)mission_layout(h->cfg.num_agents, NEP_MISSION_MAX_VERT, NEP_MISSION_MAX_POLY).bytes; }
void fleet_mission_args(nep_batch_t* h, FleetMissionArgs& ma) {
  nep_batch::Fleet& F = h->fleet;
  ma.cfg = F.mis_cfg; ma.lds_bytes = F.mis_lds;
  ma.t_issue = F.mis_t_issue.p; ma.length = F.mis_length.p; ma.completed = F.mis_completed.p; ma.counts = F.mis_counts.p; ma.sums = F.mis_sums.p;
  ma.scene_i = F.mis_scene.p; ma.t_run = F.mis_t_run.p; ma.log = F.mis_log.p; ma.log_n = F.mis_log_n.p;
  ma.kn = F.keep_n.p; ma.koff = F.keep_off.p; ma.kxy = F.keep_xy.p;
  ma.script = F.script_cap > 0 ? F.script.p : nullptr; ma.script_n = F.script_cap > 0 ? F.script_n.p : nullptr;
}
constexpr size_t kMissionLds = 64 * 1024;
}  // namespace

int nep_batch_fleet_mission_keepout(nep_batch_t* h, int32_t scene, int32_t n_poly, const int32_t* off, const double* xy) {
  if (int e = fleet_guard(h, false)) return e;
  if (scene < 0 || scene >= h->cfg.n_scenes || n_poly < 0 || (n_poly > 0 && (!off || !xy))) return fail(NEP_E_ARG, "bad arguments");
  if (n_poly > NEP_MISSION_MAX_POLY) return fail(NEP_E_CAP, "more than NEP_MISSION_MAX_POLY keep-out polygons in a scene");
  std::vector<int> o(NEP_MISSION_MAX_POLY + 1, 0);
  std::vector<double> q;
  for (int j = 0; j < n_poly; j++) {
    const int c = off[j + 1] - off[j];
    if (off[0] != 0 || c < 3) return fail(NEP_E_ARG, "keep-out offsets start at 0 and every polygon has at least 3 vertices");
    if (off[j + 1] > NEP_MISSION_MAX_VERT) return fail(NEP_E_CAP, "more than NEP_MISSION_MAX_VERT keep-out vertices in a scene");
    std::vector<double> v(xy + 2 * (size_t)off[j], xy + 2 * (size_t)off[j + 1]);
    if (!normalize_ccw(v.data(), c)) return fail(NEP_E_ARG, "a keep-out polygon is not convex");
    q.insert(q.end(), v.begin(), v.end());
    o[j + 1] = off[j + 1];
  }
  nep_batch::Fleet& F = h->fleet;
  HIPCHK(hipDeviceSynchronize());     // the previous set may still be read by kernels in flight
  if (int e = mission_keep_ensure(h)) return e;
  const int nv = n_poly ? o[n_poly] : 0;
  HIPCHK(hipMemcpy(F.keep_n.p + scene, &n_poly, sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(F.keep_off.p + (size_t)scene * (NEP_MISSION_MAX_POLY + 1), o.data(), o.size() * sizeof(int), hipMemcpyHostToDevice));
  if (nv) HIPCHK(hipMemcpy(F.keep_xy.p + (size_t)scene * NEP_MISSION_MAX_VERT * 2, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int nep_batch_fleet_mission_script(nep_batch_t* h, int32_t n_goals, const double* goals) {
  if (int e = fleet_guard(h, false)) return e;
  if (n_goals < 0 || (n_goals > 0 && !goals)) return fail(NEP_E_ARG, "bad arguments (n_goals >= 0, a table when n_goals > 0)");
  nep_batch::Fleet& F = h->fleet;
  const size_t slots = (size_t)h->slots;
  if (n_goals > (1 << 20)) return fail(NEP_E_CAP, "more than 2^20 scripted goals per slot");
  for (size_t i = 0; i < slots * (size_t)n_goals * 3; i++)
    if (!(goals[i] - goals[i] == 0.0)) return fail(NEP_E_ARG, "a scripted goal is not finite");
  if (F.script_cap > 0 && n_goals > F.script_cap) return fail(NEP_E_CAP, "the script is longer than the handle's capacity (the n_goals of the first upload)");
  if (F.script_cap == 0 && n_goals == 0) return 0;      // nothing uploaded yet, nothing to switch off
  HIPCHK(hipDeviceSynchronize());     // the previous table may still be read by kernels in flight
  if (F.script_cap == 0) {
    if (int e = F.script.ensure(slots * (size_t)n_goals * 3)) return e;
    if (int e = F.script_n.ensure(1)) return e;
    F.script_cap = n_goals;
  }
  if (n_goals > 0) HIPCHK(hipMemcpy(F.script.p, goals, slots * (size_t)n_goals * 3 * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(F.script_n.p, &n_goals, sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

int nep_batch_fleet_mission_init(nep_batch_t* h, const nep_mission_cfg* cfg, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!cfg) return fail(NEP_E_ARG, "null argument");
  if (!nep_mission_impl::mission_cfg_ok(*cfg)) return fail(NEP_E_ARG, "bad mission configuration (mode 1..3, max_goals >= 1, max_attempts a multiple of 64 in 64..4096, log_cap >= 0, lo < hi, arrive_radius and timeout > 0, nothing negative)");
  nep_batch::Fleet& F = h->fleet;
  if (cfg->mode == NEP_MISSION_PER_AGENT && !(cfg->min_dist_self > F.cfg.goal_radius)) return fail(NEP_E_ARG, "mode NEP_MISSION_PER_AGENT needs min_dist_self > the fleet's goal_radius: a fresh goal must not count as reached");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(st));
  F.mis_ready = false;
  if (int e = mission_keep_ensure(h)) return e;
  if (mission_lds_need(h) > kMissionLds) return fail(NEP_E_CAP, "the agents of a scene do not fit into the mission kernel's 64 KB of LDS next to NEP_MISSION_MAX_VERT keep-out vertices (52 B per agent: up to 1 097 agents)");
  const size_t slots = (size_t)h->slots, S = (size_t)h->cfg.n_scenes;
  const size_t owners = cfg->mode == NEP_MISSION_PER_AGENT ? slots : S;
  if (int e = F.mis_t_issue.ensure(slots)) return e;
  if (int e = F.mis_length.ensure(slots)) return e;
  if (int e = F.mis_sums.ensure(slots * 2)) return e;
  if (int e = F.mis_completed.ensure(slots)) return e;
  if (int e = F.mis_counts.ensure(slots * 4)) return e;
  if (int e = F.mis_scene.ensure(S * 4)) return e;
  if (int e = F.mis_t_run.ensure(S)) return e;
  if (int e = F.mis_log_n.ensure(owners)) return e;
  if (int e = F.mis_log.ensure(owners * (size_t)cfg->log_cap)) return e;
  F.mis_cfg = *cfg; F.mis_lds = mission_lds_need(h);
  HIPCHK(hipMemsetAsync(F.mis_log_n.p, 0, owners * sizeof(int), st));
  HIPCHK(hipMemsetAsync(F.mis_log.p, 0, std::max<size_t>(1, owners * (size_t)cfg->log_cap) * sizeof(nep_mission_leg), st));
  FleetArgs fa{};
  fleet_args(h, fa);
  FleetMissionArgs ma{};
  fleet_mission_args(h, ma);
  launch_fleet_mission_seed(ma, fa, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  F.mis_ready = true;
  return 0;
}

int nep_batch_fleet_mission(nep_batch_t* h, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!h->fleet.mis_ready) return fail(NEP_E_STATE, "nep_batch_fleet_mission_init has not run on this handle");
  FleetArgs fa{};
  fleet_args(h, fa);
  FleetMissionArgs ma{};
  fleet_mission_args(h, ma);
  launch_fleet_mission(ma, fa, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the effort record (include/neptune_fleet.h; kernel: fleet_effort_kernels.hip; host form: effort_host.cpp) ----
int nep_batch_fleet_effort(nep_batch_t* h, double j_max, double slack, nep_fleet_effort* d_effort, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!d_effort) return fail(NEP_E_ARG, "null argument");
  FleetArgs fa{};
  fleet_args(h, fa);
  const nep_effort_impl::EffortLimits l{h->eng.sp.v_max, h->eng.sp.a_max, j_max, slack};
  if (!nep_effort_impl::effort_args_ok(l, fa.cfg.dc, fa.cfg.round_ticks)) return fail(NEP_E_ARG, "bad effort arguments (v_max, a_max and j_max finite and > 0, slack finite and >= 0)");
  launch_fleet_effort(fa, l.v_max, l.a_max, l.j_max, l.slack, d_effort, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the move-back rule (include/neptune_fleet.h; kernel: fleet_moveback_kernels.hip; host form: moveback_host.cpp) ----
int nep_batch_fleet_moveback(nep_batch_t* h, const nep_moveback_cfg* cfg, nep_fe_start* d_start, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!cfg || !d_start) return fail(NEP_E_ARG, "null argument");
  if (!nep_moveback_impl::moveback_cfg_ok(*cfg)) return fail(NEP_E_ARG, "bad move-back configuration (radius finite, timeout finite and >= 0)");
  FleetArgs fa{};
  fleet_args(h, fa);
  fa.start = d_start;
  launch_fleet_moveback(*cfg, fa, h->fleet.mis_ready ? h->fleet.mis_t_issue.p : nullptr, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_fleet_mission_state(nep_batch_t* h, double* goal_out, double* t_issue_out, double* length_out, int32_t* completed_out,
                                  int32_t* counts_out, double* sums_out, int32_t* scene_out, double* t_run_out) {
  if (int e = fleet_guard(h, true)) return e;
  nep_batch::Fleet& F = h->fleet;
  if (!F.mis_ready) return fail(NEP_E_STATE, "nep_batch_fleet_mission_init has not run on this handle");
  const size_t slots = (size_t)h->slots, S = (size_t)h->cfg.n_scenes;
  HIPCHK(hipDeviceSynchronize());
  if (goal_out) HIPCHK(hipMemcpy(goal_out, F.goal.p, slots * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (t_issue_out) HIPCHK(hipMemcpy(t_issue_out, F.mis_t_issue.p, slots * sizeof(double), hipMemcpyDeviceToHost));
  if (length_out) HIPCHK(hipMemcpy(length_out, F.mis_length.p, slots * sizeof(double), hipMemcpyDeviceToHost));
  if (completed_out) HIPCHK(hipMemcpy(completed_out, F.mis_completed.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  if (counts_out) HIPCHK(hipMemcpy(counts_out, F.mis_counts.p, slots * 4 * sizeof(int), hipMemcpyDeviceToHost));
  if (sums_out) HIPCHK(hipMemcpy(sums_out, F.mis_sums.p, slots * 2 * sizeof(double), hipMemcpyDeviceToHost));
  if (scene_out) HIPCHK(hipMemcpy(scene_out, F.mis_scene.p, S * 4 * sizeof(int), hipMemcpyDeviceToHost));
  if (t_run_out) HIPCHK(hipMemcpy(t_run_out, F.mis_t_run.p, S * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int nep_batch_fleet_mission_log(nep_batch_t* h, nep_mission_leg* log_out, int32_t* n_out) {
  if (int e = fleet_guard(h, true)) return e;
  nep_batch::Fleet& F = h->fleet;
  if (!F.mis_ready) return fail(NEP_E_STATE, "nep_batch_fleet_mission_init has not run on this handle");
  const size_t owners = F.mis_cfg.mode == NEP_MISSION_PER_AGENT ? (size_t)h->slots : (size_t)h->cfg.n_scenes;
  HIPCHK(hipDeviceSynchronize());
  if (log_out && F.mis_cfg.log_cap > 0) HIPCHK(hipMemcpy(log_out, F.mis_log.p, owners * (size_t)F.mis_cfg.log_cap * sizeof(nep_mission_leg), hipMemcpyDeviceToHost));
  if (n_out) HIPCHK(hipMemcpy(n_out, F.mis_log_n.p, owners * sizeof(int), hipMemcpyDeviceToHost));
  return F.mis_cfg.log_cap;
}

// ---- the recorder (include/neptune_fleet.h; kernels: fleet_recorder_kernels.hip; layout: recorder_common.h) ----
namespace {
// the header of a snapshot of the state the handle has now
nep_fleet_snapshot_hdr recorder_header(const nep_batch_t* h) {
  const nep_batch::Fleet& F = h->fleet;
  nep_fleet_snapshot_hdr hd{};
  hd.magic = NEP_SNAPSHOT_MAGIC; hd.version = NEP_SNAPSHOT_VERSION; hd.hdr_bytes = NEP_SNAPSHOT_HDR_BYTES;
  hd.n_scenes = h->cfg.n_scenes; hd.N = h->cfg.num_agents; hd.num_pol = h->cfg.num_pol; hd.ring_cap = F.cap; hd.max_states = h->cfg.max_states;
  hd.tether_form = !F.ent_ready ? 0 : F.ent_cap ? 2 : 1; hd.tether_cap = !F.ent_ready ? 0 : F.ent_cap ? F.ent_cap : NEP_FE_ENT_CAP;
  hd.mission_mode = F.mis_ready ? F.mis_cfg.mode : 0; hd.log_cap = F.mis_ready ? F.mis_cfg.log_cap : 0;
  hd.timers = F.timers ? 1 : 0;
  hd.scene_bytes = nep_recorder::layout(hd, nullptr, nullptr);
  nep_mission_cfg none{};
  hd.cfg_hash = nep_recorder::config_hash(F.cfg, F.ent_ready ? F.cable : 0.0, F.mis_ready ? F.mis_cfg : none);
  return hd;
}
// the sections of hd's layout on the handle's arrays; every section is checked against its allocation
int recorder_args(nep_batch_t* h, const nep_fleet_snapshot_hdr& hd, RecorderArgs& ra) {
  nep_batch::Fleet& F = h->fleet;
  int64_t off[NEP_SNAPSHOT_N_SECTIONS], bytes[NEP_SNAPSHOT_N_SECTIONS];
  nep_recorder::layout(hd, off, bytes);
  struct Arr { void* p; size_t have; };
  auto arr = [](auto& b) { return Arr{(void*)b.p, b.n * sizeof(*b.p)}; };
  Arr a[NEP_SNAPSHOT_N_SECTIONS] = {};
  a[NEP_SNAP_ORIGIN] = arr(F.origin); a[NEP_SNAP_ROUND] = arr(F.round); a[NEP_SNAP_RING] = arr(F.ring); a[NEP_SNAP_HEAD] = arr(F.head); a[NEP_SNAP_SIZE] = arr(F.size);
  a[NEP_SNAP_K_END] = arr(F.k_end); a[NEP_SNAP_STATE] = arr(F.state); a[NEP_SNAP_GOAL] = arr(F.goal); a[NEP_SNAP_PWP] = arr(F.pwp); a[NEP_SNAP_FLOWN] = arr(F.flown);
  a[NEP_SNAP_DONE] = arr(F.done); a[NEP_SNAP_OUTCOME] = arr(F.outcome); a[NEP_SNAP_SFLAGS] = arr(F.sflags); a[NEP_SNAP_PERIOD] = arr(F.period); a[NEP_SNAP_PHASE] = arr(F.phase);
  a[NEP_SNAP_T_NOW] = arr(F.t_now); a[NEP_SNAP_COUNTERS] = arr(F.counters);
  a[NEP_SNAP_ENT] = arr(F.ent); a[NEP_SNAP_L_N_ALPHA] = arr(F.ent_lists.n_alpha); a[NEP_SNAP_L_N_BEND] = arr(F.ent_lists.n_bend); a[NEP_SNAP_L_ID] = arr(F.ent_lists.id);
  a[NEP_SNAP_L_CS] = arr(F.ent_lists.cs); a[NEP_SNAP_L_BETA] = arr(F.ent_lists.beta); a[NEP_SNAP_L_BEND] = arr(F.ent_lists.bend); a[NEP_SNAP_HELD] = arr(F.ent_held);
  a[NEP_SNAP_PUB_N] = arr(F.pub_n); a[NEP_SNAP_PUB_XY] = arr(F.pub_xy); a[NEP_SNAP_PUB_PREV_N] = arr(F.pub_prev_n); a[NEP_SNAP_PUB_PREV_XY] = arr(F.pub_prev_xy);
  a[NEP_SNAP_ENT_FLAGS] = arr(F.ent_flags); a[NEP_SNAP_ENT_EVER] = arr(F.ent_ever); a[NEP_SNAP_ENT_WALKED] = arr(F.ent_walked);
  a[NEP_SNAP_T_ISSUE] = arr(F.mis_t_issue); a[NEP_SNAP_LENGTH] = arr(F.mis_length); a[NEP_SNAP_COMPLETED] = arr(F.mis_completed); a[NEP_SNAP_COUNTS] = arr(F.mis_counts);
  a[NEP_SNAP_SUMS] = arr(F.mis_sums); a[NEP_SNAP_SCENE_I] = arr(F.mis_scene); a[NEP_SNAP_T_RUN] = arr(F.mis_t_run); a[NEP_SNAP_LOG] = arr(F.mis_log); a[NEP_SNAP_LOG_N] = arr(F.mis_log_n);
  ra = RecorderArgs{};
  ra.hdr = hd; ra.src_scene = -1; ra.dst_scene = -1; ra.round = F.round.p; ra.origin = F.origin.p;
  for (int i = 0; i < NEP_SNAPSHOT_N_SECTIONS; i++) {
    if (bytes[i] > (int64_t)0x7fffffff) return fail(NEP_E_CAP, "a scene's part of a fleet array is 2 GiB or more: the recorder copies up to 2 GiB per scene and section");
    // (a list buffer that was allocated for a larger capacity than the handle's has another stride: init allocates exactly, so this holds)
    if (bytes[i] && (!a[i].p || a[i].have < (size_t)bytes[i] * (size_t)h->cfg.n_scenes)) return fail(NEP_E_STATE, "the recorder's layout does not fit the handle's fleet arrays");
    ra.sec[i].p = (char*)a[i].p; ra.sec[i].off = (long)off[i]; ra.sec[i].bytes = (unsigned)bytes[i];
  }
  return 0;
}
int recorder_guard(const nep_batch_t* h) { return fleet_guard(const_cast<nep_batch_t*>(h), true); }
}  // namespace

int64_t nep_batch_fleet_snapshot_bytes(const nep_batch_t* h) {
  if (int e = recorder_guard(h)) return e;
  const nep_fleet_snapshot_hdr hd = recorder_header(h);
  return NEP_SNAPSHOT_HDR_BYTES + (int64_t)hd.n_scenes * hd.scene_bytes;
}

int64_t nep_batch_fleet_snapshot_ring_bytes(const nep_batch_t* h, int32_t n_entries) {
  if (int e = recorder_guard(h)) return e;
  if (n_entries < 1) return fail(NEP_E_ARG, "a ring has at least one entry");
  return nep_recorder::ring_bytes(recorder_header(h), n_entries);
}

int nep_batch_fleet_snapshot_ring(nep_batch_t* h, void* d_ring, int32_t n_entries, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!d_ring || n_entries < 1 || ((uintptr_t)d_ring & 15)) return fail(NEP_E_ARG, "the ring is device memory on a 16-byte boundary and has at least one entry");
  if (h->fleet.ent_ready && h->fleet.ent_cap && h->fleet.ent_lists.cap != h->fleet.ent_cap) return fail(NEP_E_STATE, "the handle's tether lists were allocated for another capacity: the recorder needs a handle whose list form was initialised once");
  RecorderArgs ra;
  if (int e = recorder_args(h, recorder_header(h), ra)) return e;
  ra.n_entries = n_entries; ra.blob = (char*)d_ring;
  h->fleet.saw(stream);
  launch_fleet_snapshot(ra, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_fleet_snapshot(nep_batch_t* h, void* d_blob, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!d_blob || ((uintptr_t)d_blob & 15)) return fail(NEP_E_ARG, "the blob is device memory on a 16-byte boundary");
  if (h->fleet.ent_ready && h->fleet.ent_cap && h->fleet.ent_lists.cap != h->fleet.ent_cap) return fail(NEP_E_STATE, "the handle's tether lists were allocated for another capacity: the recorder needs a handle whose list form was initialised once");
  RecorderArgs ra;
  if (int e = recorder_args(h, recorder_header(h), ra)) return e;
  ra.n_entries = 0; ra.blob = (char*)d_blob;
  h->fleet.saw(stream);
  launch_fleet_snapshot(ra, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_fleet_restore(nep_batch_t* h, const void* blob, int64_t bytes, int32_t src_scene, int32_t dst_scene) {
  if (int e = fleet_guard(h, true)) return e;
  for (hipStream_t st : h->fleet.seen) {      // a blocking call: not while a stream this handle's fleet calls run on is capturing
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return fail(NEP_E_STATE, "nep_batch_fleet_restore blocks: not while a stream of the handle's fleet calls is capturing");
  }
  (void)hipGetLastError();
  if (!blob || bytes < (int64_t)NEP_SNAPSHOT_HDR_BYTES) return fail(NEP_E_ARG, "a blob is at least a snapshot header");
  if ((src_scene < 0) != (dst_scene < 0) || src_scene < -1 || dst_scene < -1) return fail(NEP_E_ARG, "src_scene and dst_scene: both -1 (all scenes) or both a scene");
  nep_fleet_snapshot_hdr hb;
  HIPCHK(hipMemcpy(&hb, blob, sizeof(hb), hipMemcpyDefault));
  const char* why = nullptr;
  if (nep_recorder::check_header(hb, &why)) return fail(NEP_E_ARG, why);
  if ((bytes - NEP_SNAPSHOT_HDR_BYTES) / hb.scene_bytes < hb.n_scenes) return fail(NEP_E_ARG, "fewer bytes than the header and its scene blocks");
  const nep_fleet_snapshot_hdr hh = recorder_header(h);
  if (hb.N != hh.N || hb.num_pol != hh.num_pol || hb.ring_cap != hh.ring_cap || hb.max_states != hh.max_states || hb.timers != hh.timers)
    return fail(NEP_E_ARG, "the snapshot is of another fleet (agents, num_pol, ring_cap, max_states or timers differ from the handle's)");
  if (hb.tether_form != hh.tether_form || hb.tether_cap != hh.tether_cap) return fail(NEP_E_ARG, "the snapshot's tether state has another form or capacity than the handle's (run the same tether init first)");
  if (hb.mission_mode != hh.mission_mode || hb.log_cap != hh.log_cap) return fail(NEP_E_ARG, "the snapshot's mission state has another mode or log_cap than the handle's (run nep_batch_fleet_mission_init first)");
  if (hb.scene_bytes != hh.scene_bytes) return fail(NEP_E_ARG, "the snapshot's scene blocks have another size than the handle's state");
  if (hb.cfg_hash != hh.cfg_hash) return fail(NEP_E_ARG, "the snapshot was taken under another configuration (nep_fleet_cfg, cable length or nep_mission_cfg)");
  if (src_scene < 0 ? hb.n_scenes != hh.n_scenes : (src_scene >= hb.n_scenes || dst_scene >= hh.n_scenes)) return fail(NEP_E_ARG, "scene out of range (all scenes: the scene counts must be equal)");
  if (h->fleet.ent_ready && h->fleet.ent_cap && h->fleet.ent_lists.cap != h->fleet.ent_cap) return fail(NEP_E_STATE, "the handle's tether lists were allocated for another capacity: the recorder needs a handle whose list form was initialised once");
  nep_batch::Fleet& F = h->fleet;
  // the blocks on their way in: one block or all of them, behind a header, in a buffer of the handle's (16-byte aligned)
  const size_t n_blocks = src_scene < 0 ? (size_t)hb.n_scenes : 1, first = src_scene < 0 ? 0 : (size_t)src_scene;
  RecorderArgs ra;
  if (int e = recorder_args(h, hh, ra)) return e;
  HIPCHK(hipDeviceSynchronize());      // (kernels in flight may still read or write the state)
  if (int e = F.rec_stage.ensure(NEP_SNAPSHOT_HDR_BYTES + n_blocks * (size_t)hb.scene_bytes)) return e;
  HIPCHK(hipMemcpy(F.rec_stage.p + NEP_SNAPSHOT_HDR_BYTES, (const char*)blob + NEP_SNAPSHOT_HDR_BYTES + first * (size_t)hb.scene_bytes, n_blocks * (size_t)hb.scene_bytes, hipMemcpyDefault));
  ra.hdr = hb; ra.blob = F.rec_stage.p;
  if (src_scene >= 0) { ra.src_scene = 0; ra.dst_scene = dst_scene; ra.hdr.n_scenes = 1; }
  launch_fleet_restore(ra, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return 0;
}

int nep_batch_fleet_commit(nep_batch_t* h, const nep_solution* d_solution, const double* d_states, const nep_fe_result* d_fe_result,
                           const int32_t* d_accept, int32_t* d_outcome, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  if (!d_solution || !d_states || !d_fe_result || !d_accept) return fail(NEP_E_ARG, "null argument");
  FleetArgs fa{};
  fleet_args(h, fa);
  fa.sol = d_solution; fa.states_in = d_states; fa.fres = d_fe_result; fa.accept = d_accept; fa.outcome_out = d_outcome;
  launch_fleet_commit(fa, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_fleet_tick(nep_batch_t* h, void* stream) {
  if (int e = fleet_guard(h, true)) return e;
  FleetArgs fa{};
  fleet_args(h, fa);
  launch_fleet_tick(fa, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_fleet_ring_cap(nep_batch_t* h) {
  if (int e = fleet_guard(h, true)) return e;
  return h->fleet.cap;
}

int nep_batch_fleet_plans(nep_batch_t* h, int32_t first, int32_t n, double* states_out, int32_t* sizes) {
  if (int e = fleet_guard(h, true)) return e;
  if (first < 0 || n < 0 || first + n > h->slots) return fail(NEP_E_ARG, "slot range out of bounds");
  if (n == 0) return 0;
  nep_batch::Fleet& F = h->fleet;
  const size_t per = (size_t)F.cap * 12;
  std::vector<double> ring((size_t)n * per); std::vector<int> head(n), size(n);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(ring.data(), F.ring.p + (size_t)first * per, ring.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(head.data(), F.head.p + first, n * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(size.data(), F.size.p + first, n * sizeof(int), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) {
    if (head[i] < 0 || head[i] >= F.cap || size[i] < 0 || size[i] > F.cap) return fail(NEP_E_STATE, "a plan ring's head or size is out of range");
    if (sizes) sizes[i] = size[i];
    if (!states_out) continue;
    double* o = states_out + (size_t)i * per;
    std::memset(o, 0, per * sizeof(double));
    for (int k = 0; k < size[i]; k++) std::memcpy(o + (size_t)k * 12, ring.data() + (size_t)i * per + (size_t)((head[i] + k) % F.cap) * 12, 12 * sizeof(double));
  }
  return 0;
}

int nep_batch_fleet_state(nep_batch_t* h, double* state_out, nep_pwp* pwp_out, int32_t* flown_out, int32_t* done_out, int32_t* outcome_out,
                          int32_t* flags_out, int32_t* k_end_out) {
  if (int e = fleet_guard(h, true)) return e;
  nep_batch::Fleet& F = h->fleet;
  const size_t slots = (size_t)h->slots;
  HIPCHK(hipDeviceSynchronize());
  if (state_out) HIPCHK(hipMemcpy(state_out, F.state.p, slots * 12 * sizeof(double), hipMemcpyDeviceToHost));
  if (pwp_out) HIPCHK(hipMemcpy(pwp_out, F.pwp.p, slots * sizeof(nep_pwp), hipMemcpyDeviceToHost));
  if (flown_out) HIPCHK(hipMemcpy(flown_out, F.flown.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  if (done_out) HIPCHK(hipMemcpy(done_out, F.done.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  if (outcome_out) HIPCHK(hipMemcpy(outcome_out, F.outcome.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  if (flags_out) HIPCHK(hipMemcpy(flags_out, F.sflags.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  if (k_end_out) HIPCHK(hipMemcpy(k_end_out, F.k_end.p, slots * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int nep_batch_fleet_counters(nep_batch_t* h, int32_t* counters_out, double* t_now_out, int32_t* round_out) {
  if (int e = fleet_guard(h, true)) return e;
  nep_batch::Fleet& F = h->fleet;
  const size_t S = (size_t)h->cfg.n_scenes;
  HIPCHK(hipDeviceSynchronize());
  if (counters_out) HIPCHK(hipMemcpy(counters_out, F.counters.p, S * NEP_FLEET_N_COUNTERS * sizeof(int), hipMemcpyDeviceToHost));
  if (t_now_out) HIPCHK(hipMemcpy(t_now_out, F.t_now.p, S * sizeof(double), hipMemcpyDeviceToHost));
  if (round_out) HIPCHK(hipMemcpy(round_out, F.round.p, S * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int nep_batch_next_starts(nep_batch_t* h, const nep_traj_rec* d_records, double dt, nep_fe_start* d_start, double* d_alt_goal,
                          double switch_radius, void* stream) {
  if (!h || !d_records || !d_start || !(dt >= 0.0)) return fail(NEP_E_ARG, "bad arguments");
  launch_next_starts(d_records, h->cfg.n_scenes, h->cfg.num_agents, h->cfg.first_local, h->cfg.n_local, dt, d_start, d_alt_goal, switch_radius, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int nep_batch_set_scene_statics(nep_batch_t* h, int32_t scene, int32_t n_static, const int32_t* static_off, const double* static_xy) {
  if (!h || scene < 0 || scene >= h->cfg.n_scenes || n_static < 0 || (n_static > 0 && (!static_off || !static_xy))) return fail(NEP_E_ARG, "bad arguments");
  HIPCHK(hipDeviceSynchronize());     // the previous set may still be read by kernels in flight
  return h->eng.upload_scene_statics(scene, n_static, static_off, static_xy);
}

// Test hook: replans the last nep_batch_replan* sent through the presolve's redo pass (0 when LP skipping is off).
int nep_batch_debug_redo_count(nep_batch_t* h, int32_t* by_reason) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  int n[3] = {0, 0, 0};
  HIPCHK(hipDeviceSynchronize());
  if (h->eng.d_redo_count.p) HIPCHK(hipMemcpy(n, h->eng.d_redo_count.p, 3 * sizeof(int), hipMemcpyDeviceToHost));
  if (by_reason) { by_reason[0] = n[1]; by_reason[1] = n[2]; }
  return n[0];
}

// Test hook: the slots on the redo list of the last replan (at most cap).
int nep_batch_debug_redo_list(nep_batch_t* h, int32_t* slots_out, int32_t cap) {
  if (!h || !slots_out || cap < 0) return fail(NEP_E_ARG, "bad arguments");
  int n = 0;
  HIPCHK(hipDeviceSynchronize());
  if (!h->eng.d_redo_count.p) return 0;
  HIPCHK(hipMemcpy(&n, h->eng.d_redo_count.p, sizeof(int), hipMemcpyDeviceToHost));
  if (n > cap) n = cap;
  if (n > 0) HIPCHK(hipMemcpy(slots_out, h->eng.d_redo_list.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  return n;
}

// Test hook: segments per wave of the presolve's separator (0: by launch size, -1: the unpacked kernel, 1..NEP_MAX_POL: forced)
int nep_batch_debug_set_separator_pack(nep_batch_t* h, int32_t pack) {
  if (!h || pack < -1 || pack > NEP_MAX_POL) return fail(NEP_E_ARG, "pack must be -1, 0 or 1..NEP_MAX_POL");
  h->eng.sep_pack = pack;
  return 0;
}

int nep_batch_qp_placement(nep_batch_t* h) { return h ? (h->eng.use_reg ? 1 : 0) : NEP_E_ARG; }

int nep_batch_set_launch_order(nep_batch_t* h, int32_t enable) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  if (enable) { if (int e = h->eng.d_order.ensure((size_t)h->slots)) return e; if (int e = h->eng.d_order_key.ensure((size_t)h->slots)) return e; }
  if (enable) { if (int e = h->eng.d_fe_order.ensure((size_t)h->slots)) return e; if (int e = h->eng.d_fe_order_key.ensure((size_t)h->slots)) return e; }
  if (!enable) { h->eng.have_history = false; h->eng.fe_history = false; }
  if (enable && !h->eng.lpt) {      // (the keys remember: switched on, they start from zero)
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(h->eng.d_order_key.p, 0, h->eng.d_order_key.n * sizeof(int))); HIPCHK(hipMemset(h->eng.d_fe_order_key.p, 0, h->eng.d_fe_order_key.n * sizeof(int)));
    h->eng.have_history = false; h->eng.fe_history = false;
  }
  h->eng.lpt = enable != 0;
  return 0;
}
int nep_batch_fe_search_us(nep_batch_t* h, float* us, int32_t cap) {
  if (!h || !us || cap < h->slots) return fail(NEP_E_ARG, "bad arguments");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(us, h->eng.d_fe_us.p, (size_t)h->slots * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}
int nep_batch_debug_launch_order(nep_batch_t* h, int32_t* order, int32_t cap, int32_t* n_out) {
  if (!h || !order || !n_out || cap < 0) return fail(NEP_E_ARG, "bad arguments");
  *n_out = 0;
  if (!h->eng.last_plan.ordered_qp) return 0;
  if (cap < h->slots) return fail(NEP_E_CAP, "order buffer smaller than the slot count");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(order, h->eng.d_order.p, (size_t)h->slots * sizeof(int), hipMemcpyDeviceToHost));
  *n_out = h->slots;
  return 0;
}
// Test hooks of the launch sequence (include/neptune_backend_debug.h): what the last replan launched, the obstacle boxes, the ordering keys
int nep_batch_debug_launch_path(nep_batch_t* h, int32_t* bits) {
  if (!h || !bits) return fail(NEP_E_ARG, "bad arguments");
  *bits = path_bits(h->eng.last_plan);
  return 0;
}
int nep_batch_debug_boxes(nep_batch_t* h, int32_t scene, double* out, int32_t cap) {
  if (!h || !out || scene < 0 || scene >= h->cfg.n_scenes || cap < 0) return fail(NEP_E_ARG, "bad arguments");
  const Engine& E = h->eng;
  const size_t n = (size_t)(E.sp.num_agents + E.sp.n_static) * E.sp.num_pol * 4;
  if ((size_t)cap < n) return fail(NEP_E_CAP, "box buffer smaller than (num_agents + n_static) x num_pol x 4 doubles");
  if (!E.d_fe_box.p || E.d_fe_box.n < (size_t)h->cfg.n_scenes * n) return fail(NEP_E_STATE, "the handle has no obstacle boxes");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, E.d_fe_box.p + (size_t)scene * n, n * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
int nep_batch_debug_presolved(nep_batch_t* h, int32_t* marks, int32_t cap) {
  if (!h || !marks || cap < 0) return fail(NEP_E_ARG, "bad arguments");
  if (cap < h->slots) return fail(NEP_E_CAP, "mark buffer smaller than the slot count");
  if (!h->eng.d_presolved.p || h->eng.d_presolved.n < (size_t)h->slots) return fail(NEP_E_STATE, "the handle has no certificate marks");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(marks, h->eng.d_presolved.p, (size_t)h->slots * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int nep_batch_debug_order_keys(nep_batch_t* h, int32_t* keys, int32_t cap) {
  if (!h || !keys || cap < 0) return fail(NEP_E_ARG, "bad arguments");
  if (cap < h->slots) return fail(NEP_E_CAP, "key buffer smaller than the slot count");
  if (!h->eng.d_order_key.p || h->eng.d_order_key.n < (size_t)h->slots) return fail(NEP_E_STATE, "the handle has no ordering keys (nep_batch_set_launch_order)");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(keys, h->eng.d_order_key.p, (size_t)h->slots * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

// Development aids that used to be environment variables (rounds 2-5: NEP_QP_KERNEL, NEP_SEP_SKIP, NEP_SEP_NO_REDO, NEP_QP_LPT, NEP_FE_LPT,
// NEP_QP_KEY_DECAY, NEP_FE_KEY_DECAY, NEP_SEP_UNPACKED / NEP_SEP_PACK, NEP_CORR_FROM / NEP_CORR_MAX, NEP_FE_THREE, NEP_FE_XCD,
// NEP_POLISH_GRID, NEP_HULL_KERNEL): explicit setters now, so that a caller's environment cannot change what the library computes.
static int engine_option(Engine& E, const char* name, int32_t v) {
  if (!name) return fail(NEP_E_ARG, "null option name");
  const std::string n(name);
  if (n == "qp_kernel") { if (v < 0 || v > 2) return fail(NEP_E_ARG, "qp_kernel: 0 automatic, 1 register placement, 2 LDS placement"); E.force_kernel = v; E.choose_placement(); }
  else if (n == "sep_skip") E.skip_lps = v != 0;                 // 0: a presolved replan's far LPs are solved too (parked), none skipped
  else if (n == "sep_no_redo") E.no_redo = v != 0;               // 1: flagged replans keep their presolved result (inspection)
  else if (n == "qp_lpt") E.lpt = v != 0;
  else if (n == "fe_lpt") E.fe_lpt = v != 0;
  else if (n == "qp_key_decay") E.opt_qp_key_decay = v;
  else if (n == "fe_key_decay") E.opt_fe_key_decay = v;
  else if (n == "sep_pack") { if (v < -1 || v > NEP_MAX_POL) return fail(NEP_E_ARG, "sep_pack: -1 unpacked, 0 automatic, 1..NEP_MAX_POL"); E.sep_pack = v; }
  else if (n == "corr_from") { if (v < 1) return fail(NEP_E_ARG, "corr_from >= 1"); E.opt_corr_from = v; E.sp.corr_from_it = v; }
  else if (n == "corr_max") { if (v < 1) return fail(NEP_E_ARG, "corr_max >= 1"); E.opt_corr_max = v; E.sp.corr_max_count = v; }
  else if (n == "fleet_ent_proof") E.opt_fleet_ent_proof = v != 0;      // 0: nep_batch_fleet_predict_ent / _track_ent walk every other agent and static at every step (same states; A/B of the lanes' proofs)
  else if (n == "qp_profile") E.profile_phases = v != 0;
  else if (n == "presolve_fused") E.presolve_fused = v != 0;        // 0: the certificate always runs as qp_presolve_kernel, never in the separator's wave (A/B, tests; same bytes)
  else if (n == "presolve_kernel") E.presolve_kernel = v != 0;      // 0: the zero-iteration test only inside qp_reg_kernel<true> (rounds 3-5); same results up to the last place of the objective
  else return fail(NEP_E_ARG, "unknown debug option: " + n);
  return 0;
}
int nep_batch_debug_set_option(nep_batch_t* h, const char* name, int32_t value) { if (!h) return fail(NEP_E_ARG, "null handle"); return engine_option(h->eng, name, value); }
int nep_backend_debug_set_option(nep_backend_t* h, const char* name, int32_t value) { if (!h) return fail(NEP_E_ARG, "null handle"); return engine_option(h->eng, name, value); }
int nep_debug_set_global_option(const char* name, int32_t value) {
  if (!name) return fail(NEP_E_ARG, "null option name");
  const std::string n(name);
  if (n == "fe_three") g_debug.fe_three = value != 0;
  else if (n == "fe_xcd") g_debug.fe_xcd = value;
  else if (n == "polish_grid") { if (value < 1) return fail(NEP_E_ARG, "polish_grid >= 1"); g_debug.polish_grid = value; }
  else if (n == "polish_impl") { if (value < 0 || value > 1) return fail(NEP_E_ARG, "polish_impl: 0 the first form of the polish pass, 1 the batched one"); g_debug.polish_impl = value; }
  else if (n == "hull_sort") { if (value < 0 || value > 1) return fail(NEP_E_ARG, "hull_sort: 0 the full network over the corners, 1 stacked pairs"); g_debug.hull_sort = value; }      // (hull_group_kernel's sort of an inflated hull, read at launch; same hulls)
  else if (n == "parked_bound") g_debug.parked_bound = value != 0;     // 0: a certified slot always reads its parked lines back (same verdicts)
  else return fail(NEP_E_ARG, "unknown global debug option: " + n);
  return 0;
}

int nep_batch_set_hull_kernel(nep_batch_t* h, int32_t mode) {
  if (!h || mode < 0 || mode > 2) return fail(NEP_E_ARG, "mode: 0 automatic, 1 one hull per wave, 2 eight hulls per wave");
  h->eng.sp.hull_mode = mode;
  return 0;
}

int nep_batch_set_max_runtime(nep_batch_t* h, double seconds) {
  if (!h || !(seconds >= 0.0)) return fail(NEP_E_ARG, "bad arguments");
  h->eng.sp.time_limit_ticks = seconds > 0 ? (long long)(seconds * h->eng.clock_hz) : 0;
  return 0;
}

// Setters both handle kinds have (E: the handle's engine, or null for a null handle).  The batched handle's row scratch follows the
// mode — a pool with the presolve's redo pass, one area per slot without — so its setters re-size it (never inside a capture); the
// per-agent handle sizes its scratch and picks its placement at every optimize().
namespace {
int set_line_cull(Engine* E, double radius) {
  if (!E || !(radius >= 0.0)) return fail(NEP_E_ARG, "bad arguments");
  E->sp.cull_radius = radius; E->cull_user_set = true;
  return 0;
}
int set_separator_rule(Engine* E, int32_t rule) {
  if (!E || (rule != 0 && rule != 1)) return fail(NEP_E_ARG, "separator rule: 0 largest gap, 1 GLPK-class simplex");
  E->sp.sep_rule = rule;
  return 0;
}
int resize_row_scratch(Engine& E) { HIPCHK(hipDeviceSynchronize()); return E.size_row_scratch(); }
}  // namespace
int nep_batch_set_line_cull(nep_batch_t* h, double radius) {
  if (int e = set_line_cull(h ? &h->eng : nullptr, radius)) return e;
  h->eng.choose_placement();      // (a culled problem's near lines fit the register kernel whatever the scene size)
  return resize_row_scratch(h->eng);
}
double nep_batch_get_line_cull(nep_batch_t* h) { return h ? h->eng.sp.cull_radius : -1.0; }
int nep_backend_set_line_cull(nep_backend_t* h, double radius) { return set_line_cull(h ? &h->eng : nullptr, radius); }

int nep_batch_set_separator_rule(nep_batch_t* h, int32_t rule) {
  if (int e = set_separator_rule(h ? &h->eng : nullptr, rule)) return e;
  return resize_row_scratch(h->eng);
}
// Row scratch for the worst case (one area per slot) whatever the mode: nep_batch_check reports NEP_E_CAP when the pool of the
// presolve's redo pass ran out (more than 1 024 replans of one launch listed with rows beyond the register slots).
int nep_batch_reserve_row_scratch(nep_batch_t* h) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  h->eng.scratch_full = true;
  return resize_row_scratch(h->eng);
}
// Lines per (replan, segment) the line buckets hold: 0 the default budget, -1 the reference's worst case, n > 0 that many (see
// size_scratch).  Re-sizes the buffers: not inside a graph capture.
int nep_batch_set_line_capacity(nep_batch_t* h, int32_t lines_per_segment) {
  if (!h || lines_per_segment < -1) return fail(NEP_E_ARG, "bad arguments");
  HIPCHK(hipDeviceSynchronize());
  h->eng.lines_cap_user = lines_per_segment;
  return h->eng.size_scratch();
}
int64_t nep_batch_line_bucket_bytes(nep_batch_t* h) { return h ? (int64_t)h->slots * NEP_MAX_POL * h->eng.sp.lines_cap * 3 * (int64_t)sizeof(double) : 0; }
int64_t nep_batch_row_scratch_bytes(nep_batch_t* h) { return h ? (int64_t)(h->eng.d_row_scratch.n * sizeof(double)) : 0; }
int nep_backend_set_separator_rule(nep_backend_t* h, int32_t rule) { return set_separator_rule(h ? &h->eng : nullptr, rule); }

namespace { int set_tol(Engine& E, double res, double gap) {
  if (!(res >= 1e-12 && res <= 1e-6) || !(gap >= 1e-13 && gap <= 1e-7)) return fail(NEP_E_ARG, "tolerances: residuals in [1e-12, 1e-6], relative gap in [1e-13, 1e-7]");
  E.sp.tol_res = res; E.sp.tol_gap = gap;
  E.sp.tol_res_inv = res == 1e-10 ? 1e10 : (res == 1e-9 ? 1e9 : 1.0 / res); E.sp.tol_gap_inv = gap == 1e-11 ? 1e11 : (gap == 1e-10 ? 1e10 : 1.0 / gap); E.sp.tol_gap_floor = 0.1 * gap;      // (the defaults' reciprocals as the literals the kernels were validated with)
  return 0;
} }
int nep_batch_set_tolerances(nep_batch_t* h, double residual_tol, double gap_tol) { if (!h) return fail(NEP_E_ARG, "null handle"); return set_tol(h->eng, residual_tol, gap_tol); }
int nep_backend_set_tolerances(nep_backend_t* h, double residual_tol, double gap_tol) { if (!h) return fail(NEP_E_ARG, "null handle"); return set_tol(h->eng, residual_tol, gap_tol); }

// (on: 0 off; 1 — the default — and 2 everywhere, under the presolve as well; 3: every-row solves only, round 5's default)
namespace { int set_polish(Engine& E, int32_t on) { E.polish = on != 0; E.polish_presolve = on == 1 || on == 2; return 0; } }
int nep_batch_set_polish(nep_batch_t* h, int32_t on) { if (!h) return fail(NEP_E_ARG, "null handle"); return set_polish(h->eng, on); }
int nep_backend_set_polish(nep_backend_t* h, int32_t on) { if (!h) return fail(NEP_E_ARG, "null handle"); return set_polish(h->eng, on); }
// Test hook: the last replan's polish pass — replans listed for it (solves that ended without the strict tests), replans certified
int nep_batch_debug_polish_count(nep_batch_t* h, int32_t* listed, int32_t* certified) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipDeviceSynchronize());
  // (a launch whose pass was not armed — polish off, or the LDS-placement kernel, which has no hooks — leaves the counters of an earlier
  // launch behind: reported as (0, 0), round-5 advisor finding)
  if (h->eng.d_polish_count.p && h->eng.last_plan.polish_armed) HIPCHK(hipMemcpy(c, h->eng.d_polish_count.p, sizeof(c), hipMemcpyDeviceToHost));
  if (listed) *listed = c[0];
  if (certified) *certified = c[3];
  return 0;
}
// Test hook: per slot of the last replan, 0 = not listed for the polish pass, else the flag word — bit m: the solve of mode m (0 first
// problem, 1 relaxed) was left for the pass; bit 8: the pass certified an optimum and wrote the slot's result; bit 9: it read a
// certified point's parked lines back (with "parked_bound": only when a control point left the movement bound); bit 10: it dropped a
// certified point that failed the presolve's verification.
int nep_batch_debug_polish_flags(nep_batch_t* h, int32_t* flags, int32_t cap) {
  if (!h || !flags || cap < h->slots) return fail(NEP_E_ARG, "bad arguments");
  for (int i = 0; i < h->slots; i++) flags[i] = 0;
  if (!h->eng.d_polish_count.p || !h->eng.last_plan.polish_armed) return 0;
  int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(c, h->eng.d_polish_count.p, sizeof(c), hipMemcpyDeviceToHost));
  const int n = c[0] < h->slots ? c[0] : h->slots;
  if (n <= 0) return 0;
  std::vector<int> list(n), fl(h->slots);
  HIPCHK(hipMemcpy(list.data(), h->eng.d_polish_list.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(fl.data(), h->eng.d_polish_flag.p, (size_t)h->slots * sizeof(int), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) if (list[i] >= 0 && list[i] < h->slots) flags[list[i]] = fl[list[i]];
  return 0;
}
int nep_batch_set_safety_check_prev(nep_batch_t* h, int32_t on) { if (!h) return fail(NEP_E_ARG, "null handle"); h->eng.safety_check_prev = on != 0; return 0; }

int nep_batch_debug_conflicts(nep_batch_t* h, int32_t scene, uint8_t* conflict_out) {
  if (!h || !conflict_out || scene < 0 || scene >= h->cfg.n_scenes) return fail(NEP_E_ARG, "bad arguments");
  const size_t nn = (size_t)h->cfg.num_agents * h->cfg.num_agents;
  if (h->eng.d_conflict.n < (size_t)h->cfg.n_scenes * nn) return fail(NEP_E_STATE, "no safety check has run");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(conflict_out, h->eng.d_conflict.p + (size_t)scene * nn, nn, hipMemcpyDeviceToHost));
  return 0;
}
int nep_batch_debug_conflicts_prev(nep_batch_t* h, int32_t scene, uint8_t* conflict_out) {
  if (!h || !conflict_out || scene < 0 || scene >= h->cfg.n_scenes) return fail(NEP_E_ARG, "bad arguments");
  const size_t nn = (size_t)h->cfg.num_agents * h->cfg.num_agents;
  if (h->eng.d_conflict_prev.n < (size_t)h->cfg.n_scenes * nn) return fail(NEP_E_STATE, "no safety check with nep_batch_set_safety_check_prev has run");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(conflict_out, h->eng.d_conflict_prev.p + (size_t)scene * nn, nn, hipMemcpyDeviceToHost));
  return 0;
}

int nep_batch_wait(nep_batch_t* h, void* stream) { if (!h) return fail(NEP_E_ARG, "null handle"); HIPCHK(hipStreamSynchronize((hipStream_t)stream)); return 0; }

int nep_batch_check(nep_batch_t* h, void* stream) {
  if (!h) return fail(NEP_E_ARG, "null handle");
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  int flags = 0;
  if (h->eng.d_flags.p) {
    HIPCHK(hipMemcpy(&flags, h->eng.d_flags.p, sizeof(int), hipMemcpyDeviceToHost));
    if (flags) HIPCHK(hipMemset(h->eng.d_flags.p, 0, sizeof(int)));
  }
  if (flags & NEP_FLAG_LINES) return fail(NEP_E_CAP, "a segment got more separating lines than its bucket holds: nep_batch_set_line_capacity(h, -1) sizes the buckets for the reference's worst case");
  if (flags & NEP_FLAG_SCRATCH) return fail(NEP_E_CAP, "the presolve's redo pass listed more replans with rows beyond the register slots than the handle has scratch areas for: nep_batch_reserve_row_scratch");
  if (flags & NEP_FLAG_ENT_POOL) return fail(NEP_E_CAP, "the pool of big entangle-state records ran out (front end: children of a search were pruned for it, by claim order; safety re-check: a trajectory was turned down): nep_batch_set_fe_ent_big_records");
  if (flags & NEP_FLAG_ENT_TRACK) return fail(NEP_E_CAP, "nep_batch_track_ent: a tether's state outgrew NEP_FE_ENT_CAP crossings, NEP_MAX_BEND - 1 bend points or 32 new crossings in one step (the step was dropped), or a state handed in was malformed");
  if (flags & NEP_FLAG_FLEET) return fail(NEP_E_CAP, "nep_batch_fleet_commit: an accepted plan or composed trajectory would have outgrown the ring (ring_cap states), NEP_TRAJ_MAX_SEG intervals, or A was already flown (the slot kept its plan: outcome NEP_FLEET_CAP, flags in nep_batch_fleet_state)");
  if (flags & NEP_FLAG_MISSION) return fail(NEP_E_CAP, "nep_batch_fleet_mission: a draw found no goal among max_attempts candidates (the slot kept its goal: NEP_FLEET_FLAG_GOAL in nep_batch_fleet_state's flags, no_goal in nep_batch_fleet_mission_state's counts)");
  if (flags & NEP_FLAG_FE_ASTAR_POOL) return fail(NEP_E_CAP, "nep_batch_frontend_astar: a search ran into its node pool (it stopped creating nodes there: bit 4 of nep_fe_result._pad): nep_batch_set_fe_astar's max_nodes");
  if (flags & NEP_FLAG_FE_ASTAR_ENT_REC) return fail(NEP_E_CAP, "nep_batch_frontend_astar_ent: a child's entangle state outgrew the fixed record — NEP_FE_ENT_CAP crossings, 32 new crossings in one sampled step or NEP_MAX_BEND bend points — and was dropped (nep_fe_result.ent_overflow), or a state at A was malformed");
  if (flags & NEP_FLAG_ENT_BETA) return fail(NEP_E_ARG, "an entangle state passed to the front end has a non-zero beta for an agent crossing (the reference's calculateBetaForCase makes it 0.0)");
  if (flags & NEP_FLAG_HULL_OVERFLOW) return fail(NEP_E_CAP, "an interval overlaps more than NEP_HULL_MAX_CP/4 committed segments (or its hull has more than NEP_HULL_MAX_V vertices)");
  return 0;
}

int nep_batch_enable_timing(nep_batch_t* h, int32_t on) { if (!h) return fail(NEP_E_ARG, "null handle"); h->eng.timing = on != 0; h->eng.ev_used = 0; return 0; }

// which: 0 hull kernel, 1 separator kernel, 2 QP kernel, 3 whole sequence
int nep_batch_kernel_time(nep_batch_t* h, int32_t which, double* avg_ms, int32_t* n_launch) {
  if (!h || !avg_ms || which < 0 || which > 3) return fail(NEP_E_ARG, "bad arguments");
  Engine& E = h->eng;
  const size_t calls = E.ev_used / 4;
  double tot = 0;
  for (size_t c = 0; c < calls; c++) {
    float ms = 0;
    hipEvent_t a = E.ev[4 * c + (which == 3 ? 0 : which)], b = E.ev[4 * c + (which == 3 ? 3 : which + 1)];
    HIPCHK(hipEventSynchronize(b));
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    tot += ms;
  }
  *avg_ms = calls ? tot / calls : 0.0;
  if (n_launch) *n_launch = (int32_t)calls;
  return 0;
}

int nep_batch_reset_timing(nep_batch_t* h) { if (!h) return fail(NEP_E_ARG, "null handle"); h->eng.ev_used = 0; return 0; }

int nep_batch_debug_hulls(nep_batch_t* h, int32_t scene, double* hull_xy, int32_t* hull_nv) {
  if (!h || !hull_xy || !hull_nv || scene < 0 || scene >= h->cfg.n_scenes) return fail(NEP_E_ARG, "bad arguments");
  Engine& E = h->eng; const size_t np = (size_t)E.sp.n_hull * E.sp.num_pol;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(hull_xy, E.d_hull_xy.p + (size_t)scene * np * kHullV * 2, np * kHullV * 2 * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hull_nv, E.d_hull_nv.p + (size_t)scene * np, np * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int nep_batch_debug_lines(nep_batch_t* h, int32_t slot, int32_t cap, int32_t* seg, double* nd, int32_t* n_out) {
  if (!h || !n_out || slot < 0 || slot >= h->slots) return fail(NEP_E_ARG, "bad arguments");
  Engine& E = h->eng;
  HIPCHK(hipDeviceSynchronize());
  return read_lines(E, (size_t)slot, NEP_MAX_POL, cap, seg, nd, n_out);
}

// Diagnostic: active inequality rows (slack < tol) at the solutions of the last nep_batch_replan*, per slot: d_out [slots][2] =
// (box rows, separating-line rows).  Reads the handle's line buckets as that replan left them and d_solution as the caller got it.
int nep_batch_active_rows(nep_batch_t* h, const nep_solution* d_solution, double tol, int32_t* d_out, void* stream) {
  if (!h || !d_solution || !d_out || !(tol >= 0.0)) return fail(NEP_E_ARG, "bad arguments");
  const ProblemSet ps = round_set(h, nullptr, const_cast<nep_solution*>(d_solution));
  launch_active_rows(h->slots, h->eng.sp, ps, tol, d_out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// Test hook: the device and page-locked bytes this process's handles and calls hold right now (counted at every allocation and free
// of a DevBuf / PinnedArena; exchange.hip's staging buffers are not among them)
int nep_debug_live_bytes(int64_t* device_bytes, int64_t* pinned_bytes) {
  if (!device_bytes || !pinned_bytes) return fail(NEP_E_ARG, "null argument");
  *device_bytes = g_live_device.load(); *pinned_bytes = g_live_pinned.load();
  return 0;
}

// development aid: per-phase shader cycles of the QP kernel (only with NEP_QP_PROFILE set at create)
int nep_batch_debug_phase_cycles(nep_batch_t* h, int32_t slot, int64_t* out16) {
  if (!h || !out16 || slot < 0 || slot >= 2 * h->slots) return fail(NEP_E_ARG, "bad arguments");      // (the front end keeps 32 values per slot: rows 2 slot and 2 slot + 1)
  if (!h->eng.profile_phases) return fail(NEP_E_STATE, "NEP_QP_PROFILE was not set when the handle was created");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out16, h->eng.d_dbg.p + (size_t)slot * 16, 16 * sizeof(long long), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
// hooks for exchange.hip (the RCCL step lives in its own translation unit)
namespace nep {
void set_last_error(const std::string& msg) { g_err = msg; }
int64_t batch_hull_block_bytes(const struct ::nep_batch* h) { return nep_batch_hull_block_bytes(h); }
void batch_dims(const struct ::nep_batch* h, int* n_scenes, int* n_local, int* num_agents) { *n_scenes = h->cfg.n_scenes; *n_local = h->cfg.n_local; *num_agents = h->cfg.num_agents; }
}
extern "C" {

// layout self-description for the ctypes mirror (tests/test_abi.py)
int nep_abi_sizeof(int32_t which) {
  switch (which) {
    case 0: return (int)sizeof(nep_pwp);
    case 1: return (int)sizeof(nep_traj_rec);
    case 2: return (int)sizeof(nep_backend_cfg);
    case 3: return (int)sizeof(nep_stats);
    case 4: return (int)sizeof(nep_batch_cfg);
    case 5: return (int)sizeof(nep_guess);
    case 6: return (int)sizeof(nep_solution);
    case 7: return (int)sizeof(nep_ent_view);
    case 8: return (int)sizeof(nep_wire_header);
    case 9: return (int)sizeof(nep_plan_cfg);
    case 10: return (int)sizeof(nep_point_a);
    case 11: return (int)sizeof(nep_fe_cfg);
    case 12: return (int)sizeof(nep_fe_start);
    case 13: return (int)sizeof(nep_fe_result);
    case 14: return (int)sizeof(nep_fe_ent_state);
    case 15: return (int)sizeof(nep_ent_track_inputs);
    case 17: return (int)sizeof(nep_audit);      // (16 stays unassigned: tests/test_ent_track_cpu.py pins it to -1)
    case 18: return (int)sizeof(nep_fleet_cfg);
    case 20: return (int)sizeof(nep_mission_cfg);      // (19 stays unassigned: tests/test_fleet_plan_cpu.py pins it to -1)
    case 21: return (int)sizeof(nep_mission_leg);
    case 23: return (int)sizeof(nep_ent_lists);      // (22 stays unassigned: tests/test_fleet_mission_cpu.py pins it to -1)
    case 25: return (int)sizeof(nep_fleet_snapshot_hdr);      // (24 stays unassigned: tests/test_ent_lists_cpu.py pins it to -1)
    case 27: return (int)sizeof(nep_moveback_cfg);      // (26 stays unassigned: tests/test_fleet_recorder_cpu.py pins it to -1)
    case 29: return (int)sizeof(nep_fleet_effort);      // (28 stays unassigned: tests/test_fleet_moveback_cpu.py pins it to -1)
    case 31: return (int)sizeof(nep_hastar_cfg);      // (30 stays unassigned: a test pins it to -1)
    case 32: return (int)sizeof(nep_hastar_result);
    case 33: return (int)sizeof(nep_hastar_state);
    case 35: return (int)sizeof(nep_mtlp_cfg);      // (34 stays unassigned: tests/test_mtlp_cpu.py pins it to -1)
    case 36: return (int)sizeof(nep_mtlp_result);
    case 37: return (int)sizeof(nep_tether_audit);
    case 39: return (int)sizeof(nep_span_audit);      // (38 stays unassigned: tests/test_tether_audit_cpu.py pins it to -1)
    default: return -1;
  }
}

}  // extern "C"
