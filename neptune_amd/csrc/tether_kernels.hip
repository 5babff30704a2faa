// tether_kernels.hip — every tether's entangle state carried along what its agent flies: between two bulk-synchronous rounds
// (nep_batch_track_ent and, on lists of more than NEP_FE_ENT_CAP crossings, nep_batch_track_ent_lists / nep_batch_ent_lists_at_a;
// include/neptune_frontend.h) and in the device fleet loop (nep_batch_fleet_init_ent / _predict_ent /
// _track_ent and the bend points nep_batch_fleet_select publishes; include/neptune_fleet.h).
//
// Two steps of the reference:
//   NeptuneRos::odomCB -> updateEntStateStaticObs (neptune_ros.cpp:781-850) once per sampled step or control tick flown, and
//   Neptune::PredictAlphasBetas (neptune.cpp:976-1008): the state forwarded to point A in one move, into a copy.
// Both are chains of nep_ent_track_step (entangle_host.cpp), which the step kernel equals bit for bit: the crossing tests, the list
// surgery, one tracked move and the tether length are ent_device.h's, and this file is built -ffp-contract=off like
// geom_kernels.hip.  publishOwnTraj's bend points (:457-476) have a kernel per entry point: the two contracts differ.
//
// Layout: one wave (one 64-thread workgroup) per slot.  A pre-kernel writes every slot's positions of the call side by side
// (the round's sampled steps, round_ticks + 1 tick positions, or the pair a prediction needs), so nobody strides through the
// samples or the plan rings.  The 64 lanes then take the other agents 64 at a time and each PROVES that its agent adds no crossing at any step of the call (ent_side on the box of the
// slot's own positions: the same side of every tether segment, of the moving last segment at every tick, and the sweep over our base
// evaluated as is — ent_agent_may_cross's argument over ticks instead of samples); the statics likewise.  What the __ballot leaves
// is walked by lane 0 step by step and in increasing index, so the crossings enter the list in the host chain's order.  The working
// state sits in LDS behind LDS-typed pointers (ds_read / ds_write, not FLAT); it goes to global scratch before a step that can
// outgrow the record and comes back if it did.  Every barrier is reached by the whole wave: the branches around them depend on
// kernel arguments and on values every lane loads from the same address.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "nep_device.h"
#include "../../include/neptune_frontend.h"
#include "../../include/neptune_entangle.h"
#include "../../include/neptune_fleet.h"
#include "ent_device.h"

namespace nep {

static_assert(kEntAddCap == NEP_ENT_TRACK_ADD_CAP, "nep_ent_track_step's and the kernel's caps on a move's new crossings differ");
static_assert(kEntAddCap <= 32, "EntAdd's cancellation bits are one 32-bit word");
static_assert(sizeof(nep_fe_ent_state) % 4 == 0, "the state is copied in 4-byte units");

namespace {

constexpr int kMaskWords = 64;      // 64-bit ballot words of the candidates' mask: up to 4096 agents (fleet_ent_fits: refused beyond)
constexpr int kStatWords = 64;      // 32-bit words of the statics' mask (EntCtx::m_static): up to 2048 statics

// The working state: nep_fe_ent_state's members behind LDS-typed pointers (counts in registers).  Betas handled as written, like the
// fixed record: every byte of the result is compared with the host chain.
struct EntWork { int n_alpha, n_bend; ent_lds_short id; ent_lds_char cs; ent_lds_double beta; ent_lds_char bend; };

__device__ __forceinline__ int rec_nb(const nep_traj_rec* r) { return min(max(r->n_bend, 0), NEP_MAX_BEND); }
__device__ __forceinline__ bool rec_present(const nep_traj_rec* r) { return r->valid && r->is_agent && r->pwp.n_seg >= 1; }      // (ent_sample_kernel's rule)
// the bend list agent i showed at the previous check (TetherArgs::prev_n / prev_xy)
__device__ __forceinline__ int prev_nb(const TetherArgs& ea, long i) { return min(max(*(const int*)(ea.prev_n + i * ea.prev_n_stride), 0), NEP_MAX_BEND); }
__device__ __forceinline__ const double* prev_bends(const TetherArgs& ea, long i) { return (const double*)(ea.prev_xy + i * ea.prev_xy_stride); }
// what the publish kernels read of EntCtx (ent_publish_point)
__device__ __forceinline__ EntCtx publish_ctx(const TetherArgs& ea, int scene) {
  EntCtx ec{};
  ec.N = ea.N; ec.S = ea.S; ec.pb = ea.pb; ec.srep = ea.srep + (long)scene * ea.static_stride * 4;
  return ec;
}

// The bend anchors a slot publishes, from either form of its state (TetherArgs::lists.cap != 0: the list form): f(k, id, cs) for
// every bend index k in order -> the state's n_bend, or -1 for a state that is no valid input to the tracking.
template <class F> __device__ __forceinline__ int publish_bends(const TetherArgs& ea, long slot, F f) {
  if (ea.lists.cap) {
    const nep_ent_lists& L = ea.lists;
    if (!ent_lists_ok(L, slot)) return -1;
    const int nb = L.n_bend[slot];
    for (int k = 0; k < nb; k++) { const long e = slot * L.cap + L.bend[slot * NEP_MAX_BEND + k]; f(k, (int)L.id[e], (int)L.cs[e]); }
    return nb;
  }
  const nep_fe_ent_state* st = ea.in + slot;
  if (!ent_state_ok(st)) return -1;
  for (int k = 0; k < st->n_bend; k++) f(k, (int)st->id[st->bend[k]], (int)st->cs[st->bend[k]]);
  return st->n_bend;
}

// One thread per (slot, position).  Between rounds (sampled != null): position q = itv * ns + j of a slot is ent_sample_kernel's
// sample j of interval itv, q = 0 the first sample of all — the end of an interval stands for the start of the next one.  The fleet's
// tracking (start == null): position q of a slot is where it stands after tick q of the round —
// q = 0 the tracked state, q >= 1 ring[(head + min(q - 1, size - 1)) mod cap], fleet_tick_kernel's pop rule.  Prediction: position 0
// is the tracked state, position 1 the published record at the slot's t_start by nep_ent_sample_points' first sample (the front end's
// sampled[i][0][0]).
__global__ void tether_pos_kernel(TetherArgs ea, FleetArgs fa) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int np = ea.n_steps + 1;
  if (e >= (long)ea.n_scenes * ea.N * np) return;
  const long slot = e / np; const int q = (int)(e - slot * np);
  double x, y;
  if (ea.sampled) {
    const int itv = q == 0 ? 0 : (q - 1) / ea.ns, col = q == 0 ? 0 : (q - 1) % ea.ns + 1;
    const double* g = ea.sampled + ((slot * ea.num_pol + itv) * (ea.ns + 1) + col) * 2;
    x = g[0]; y = g[1];
  }
  else if (q == 0) { x = fa.state[slot * 12]; y = fa.state[slot * 12 + 1]; }
  else if (!ea.start) {
    const int size = fa.size[slot], head = fa.head[slot];
    if (size < 1) { x = fa.state[slot * 12]; y = fa.state[slot * 12 + 1]; }
    else {
      const int k = (head + min(q - 1, size - 1)) % fa.cap;
      const double* g = fa.ring + (slot * fa.cap + k) * 12;
      x = g[0]; y = g[1];
    }
  } else {
    const nep_traj_rec* rec = ea.recs + slot;
    x = 0.0; y = 0.0;
    if (rec_present(rec)) {
      const double t_start = ea.start[slot].t_start, t_end = t_start + ea.num_pol * ea.T_span;
      const double deltaT = (t_end - t_start) / (1.0 * ea.num_pol);
      const double ts = t_start;
      const int n = min(rec->pwp.n_seg, NEP_TRAJ_MAX_SEG);
      int low = 0;                                 // std::upper_bound: first knot > ts
      while (low <= n && !(rec->pwp.times[low] > ts)) low++;
      int seg; double te;
      if (low <= n) {
        seg = low - 1;
        if (seg < 0) seg = 0; else if (seg > n - 1) seg = n - 1;
        te = ts - rec->pwp.times[seg];
        if (te < 0) te = 0; else if (te > deltaT) te = deltaT;
      } else { seg = n - 1; te = rec->pwp.times[n] - rec->pwp.times[n - 1]; }
      const double t3 = te * te * te, t2 = te * te;
      const double* cxp = rec->pwp.coeff[0][seg]; const double* cyp = rec->pwp.coeff[1][seg];
      x = ((cxp[0] * t3 + cxp[1] * t2) + cxp[2] * te) + cxp[3] * 1.0; y = ((cyp[0] * t3 + cyp[1] * t2) + cyp[2] * te) + cyp[3] * 1.0;
    }
  }
  ea.pos[e * 2] = x; ea.pos[e * 2 + 1] = y;
}

// publishOwnTraj's bend points (neptune_ros.cpp:457-476) at the select: the list published at the last select becomes the previous
// one, and the record gets the base and the anchor of every bend index of the state at the tracked position; an invalid state
// publishes the base alone.  One thread per slot, after fleet_select_kernel has written the record.
__global__ void fleet_ent_publish_kernel(TetherArgs ea) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = ea.N;
  if (slot >= (long)ea.n_scenes * N) return;
  const int scene = (int)(slot / N), a = (int)(slot % N);
  double* cur = ea.pub_xy + slot * NEP_MAX_BEND * 2; double* prv = ea.pub_prev_xy + slot * NEP_MAX_BEND * 2;
  for (int k = 0; k < NEP_MAX_BEND * 2; k++) prv[k] = cur[k];
  ea.pub_prev_n[slot] = ea.pub_n[slot];
  const EntCtx ec = publish_ctx(ea, scene);
  nep_traj_rec* r = ea.recs_out + slot;
  cur[0] = ea.pb[2 * a]; cur[1] = ea.pb[2 * a + 1];
  const int nb = 1 + max(publish_bends(ea, slot, [&](int k, int id, int cs) {
    const Ev2 b = ent_publish_point(id, cs, ec);
    cur[2 * (k + 1)] = b.x; cur[2 * (k + 1) + 1] = b.y;
  }), 0);
  for (int k = nb; k < NEP_MAX_BEND; k++) { cur[2 * k] = 0.0; cur[2 * k + 1] = 0.0; }
  ea.pub_n[slot] = nb;
  r->n_bend = nb;
  for (int k = 0; k < NEP_MAX_BEND; k++) { r->bend[k][0] = cur[2 * k]; r->bend[k][1] = cur[2 * k + 1]; }
}

// The same between rounds (nep_batch_track_ent): the base, then the anchor of every bend index of the state just tracked, into
// bend[0..n_bend) and n_bend of the flown record and nothing else; a slot without a trajectory or with an invalid state keeps its
// record.  A kernel of its own: the tracking reads every record's current bend points, so none may change before all of them have run.
__global__ void ent_publish_kernel(TetherArgs ea) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = ea.N;
  if (slot >= (long)ea.n_scenes * N) return;
  nep_traj_rec* r = ea.recs_out + slot;
  if (!rec_present(r)) return;
  const int scene = (int)(slot / N), a = (int)(slot % N);
  const EntCtx ec = publish_ctx(ea, scene);
  // (an invalid state writes nothing: the walk below has not run, and the base is written after it)
  const int nbs = publish_bends(ea, slot, [&](int k, int id, int cs) {
    const Ev2 b = ent_publish_point(id, cs, ec);
    r->bend[k + 1][0] = b.x; r->bend[k + 1][1] = b.y;
  });
  if (nbs < 0) return;
  r->bend[0][0] = ea.pb[2 * a]; r->bend[0][1] = ea.pb[2 * a + 1];
  r->n_bend = 1 + nbs;
}

// One wave per slot: n_steps moves of the slot's own tether state (see the head of the file).  Two forms of the state, one body:
// LISTS = false, the fixed record (ea.in / out / save), copied whole into LDS; LISTS = true, the list form (ea.lists, in place; scratch
// ea.lsave), one slot's list of ea.lists.cap entries in dynamic LDS (EntListLds).  A prediction in the list form leaves the lists alone
// and writes the fixed record at A the front end takes — or, where the result holds more than NEP_FE_ENT_CAP crossings, a zeroed one
// with NEP_ENT_TRACK_HELD, and takes the slot out of the round's active mask.  AUDIT: lane 0 also folds every move into the slot's
// nep_tether_audit (tether_audit_common.h, the host form's arithmetic); a slot that returns early audits nothing.
extern __shared__ __attribute__((aligned(16))) unsigned char s_ent_list[];
template <bool LISTS, bool AUDIT> __device__ __forceinline__ void tether_step(const TetherArgs& ea) {
  __shared__ __attribute__((aligned(16))) nep_fe_ent_state s_st;      // (LISTS: unused)
  __shared__ int s_cnt[2];                                            // (LISTS: the counts after the walk)
  __shared__ unsigned long long s_mask[kMaskWords], s_chg[kMaskWords];
  __shared__ unsigned s_stat[kStatWords];
  const long slot = blockIdx.x;
  const int lane = threadIdx.x;
  const int N = ea.N, T = ea.n_steps, np = T + 1;
  const int scene = (int)(slot / N), a = (int)(slot - (long)scene * N);
  const long base = (long)scene * N;
  const bool predict = ea.start != nullptr;
  const nep_fe_ent_state* src = ea.in + slot;
  nep_fe_ent_state* dst = ea.out + slot;
  if (ea.skip_absent && !rec_present(ea.recs + slot)) {      // (no trajectory to fly: state and record stay.  Every lane reads the same record: a uniform branch)
    if (lane == 0) ea.flags[slot] = 0;
    return;
  }
  const nep_ent_lists& L = ea.lists;
  const int cap = LISTS ? L.cap : NEP_FE_ENT_CAP;
  int n_in = 0;
  EntListLds WL{};
  if constexpr (LISTS) {
    if (!ent_lists_ok(L, slot)) {      // (every lane reads the same counts and indices: a uniform branch.  The lists stay; a prediction plans from an empty record)
      if (predict) for (int i = lane; i < (int)(sizeof(nep_fe_ent_state) / 4); i += 64) ((int*)dst)[i] = 0;
      if (lane == 0) {
        ea.flags[slot] = NEP_ENT_TRACK_CAP;
        if (ea.ever) ea.ever[slot] |= NEP_ENT_TRACK_CAP;
        atomicOr(ea.gflags, NEP_FLAG_ENT_TRACK);
      }
      return;
    }
    n_in = L.n_alpha[slot];
    WL.n_alpha = n_in; WL.n_bend = L.n_bend[slot]; WL.cap = cap;
    WL.beta = (ent_lds_double)&s_ent_list[0]; WL.id = (ent_lds_short)&s_ent_list[8 * (size_t)cap];
    WL.bend = (ent_lds_short)&s_ent_list[10 * (size_t)cap]; WL.cs = (ent_lds_char)&s_ent_list[10 * (size_t)cap + 2 * NEP_MAX_BEND];
    for (int i = lane; i < n_in; i += 64) { const long e = slot * cap + i; WL.id[i] = L.id[e]; WL.cs[i] = L.cs[e]; WL.beta[i] = L.beta[e]; }
    if (lane < NEP_MAX_BEND) WL.bend[lane] = lane < WL.n_bend ? L.bend[slot * NEP_MAX_BEND + lane] : (short)0;
    // (lane 0 reads the list after the barrier that ends the proofs)
  } else {
  for (int i = lane; i < (int)(sizeof(nep_fe_ent_state) / 4); i += 64) ((int*)&s_st)[i] = ((const int*)src)[i];
  __syncthreads();
  if (!ent_state_ok(&s_st)) {      // (s_st is the same for every lane: a uniform branch.  The state stays; a prediction hands it on as it is)
    if (dst != src) for (int i = lane; i < (int)(sizeof(nep_fe_ent_state) / 4); i += 64) ((int*)dst)[i] = ((const int*)&s_st)[i];
    if (lane == 0) {
      ea.flags[slot] = NEP_ENT_TRACK_CAP;
      if (ea.ever) ea.ever[slot] |= NEP_ENT_TRACK_CAP;
      atomicOr(ea.gflags, NEP_FLAG_ENT_TRACK);
    }
    return;
  }
  }
  EntCtx ec;
  ec.N = N; ec.S = ea.S; ec.own = a; ec.num_pol = ea.num_pol; ec.ns = 1; ec.T_span = 0.0; ec.cable = ea.cable;
  ec.pb = ea.pb; ec.srep = ea.srep + (long)scene * ea.static_stride * 4; ec.slong = ea.slong + (long)scene * ea.static_stride * 2;
  ec.sampled = nullptr; ec.present = nullptr; ec.ps = nullptr; ec.scene = scene; ec.n_hull = N;
  const Ev2 pb_self = ent_pb(ec, a);
  const double* __restrict__ pos = ea.pos;
  // the slot's own position after step q (every lane reads the same addresses)
  auto own = [&](int q) { if (predict && q == 1) return Ev2{ea.start[slot].pos[0], ea.start[slot].pos[1]}; const double* p = pos + (slot * np + q) * 2; return Ev2{p[0], p[1]}; };
  auto at = [&](long j, int q) { const double* p = pos + ((base + j) * np + q) * 2; return Ev2{p[0], p[1]}; };
  // ---- the proofs: 64 agents, then 64 statics, at a time -------------------------------------------------------------------
  EntBox box;
  { const Ev2 p0 = own(0); box.x0 = box.x1 = p0.x; box.y0 = box.y1 = p0.y; }
  for (int q = 1; q <= T; q++) { const Ev2 p = own(q); box.x0 = fmin(box.x0, p.x); box.x1 = fmax(box.x1, p.x); box.y0 = fmin(box.y0, p.y); box.y1 = fmax(box.y1, p.y); }
  const int n_words = (N + 63) >> 6;
  for (int w = 0; w < n_words; w++) {
    const int i = (w << 6) + lane;
    bool maybe = false, changed = false;
    if (i < N && i != a) {
      const nep_traj_rec* ri = ea.recs + base + i;
      const int nb = rec_nb(ri);
      if (rec_present(ri) && nb >= 1) {
        if (!ea.proof) maybe = true;
        else {
          const double* bp = &ri->bend[0][0];
          for (int k = 0; k + 1 < nb; k++) maybe |= ent_side(box, Ev2{bp[2 * (k + 1)], bp[2 * (k + 1) + 1]}, Ev2{bp[2 * k], bp[2 * k + 1]}) == 0;
          const Ev2 bk{bp[2 * (nb - 1)], bp[2 * (nb - 1) + 1]};
          Ev2 pik = at(i, 0);
          const int s0 = ent_side(box, pik, bk);
          maybe |= s0 == 0;
          for (int q = 1; q <= T; q++) {
            const Ev2 pik1 = at(i, q);
            maybe |= ent_side(box, pik1, bk) != s0;
            const double f1 = ent_wedge(pb_self, pik, bk), f2 = ent_wedge(pb_self, pik1, bk);
            maybe |= f1 * f2 < 0;
            pik = pik1;
          }
        }
        // the proof covers the eight-argument form: an agent whose published bend count changed is walked at the first step
        if (ea.prev_n) { const int n0 = prev_nb(ea, base + i); changed = n0 >= 1 && n0 != nb; }
      }
    }
    const unsigned long long m = __ballot(maybe), c = __ballot(changed);
    if (lane == 0) { s_mask[w] = m; s_chg[w] = c & ~m; }
  }
  const int s_words = (ea.S + 31) >> 5;
  for (int w2 = 0; w2 < (ea.S + 63) >> 6; w2++) {
    const int s = (w2 << 6) + lane;
    const bool maybe = s < ea.S && (!ea.proof || ent_static_may_cross(ec, box, s));
    const unsigned long long m = __ballot(maybe);
    if (lane == 0) { s_stat[2 * w2] = (unsigned)m; if (2 * w2 + 1 < s_words) s_stat[2 * w2 + 1] = (unsigned)(m >> 32); }
  }
  __syncthreads();
  // ---- the walk: lane 0, step by step, the survivors in increasing index ---------------------------------------------------
  if (lane == 0) {
    ec.m_static = s_stat;
    typename std::conditional<LISTS, EntListLds, EntWork>::type W;
    // the scratch a dropped move comes back from: the fixed record's in ea.save, the list form's in ea.lsave (counts in registers)
    nep_fe_ent_state* B = nullptr;
    short* b_id = nullptr; signed char* b_cs = nullptr; double* b_beta = nullptr; short* b_bend = nullptr;
    int b_na = 0, b_nb = 0;
    if constexpr (LISTS) {
      W = WL;
      b_id = ea.lsave.id + slot * cap; b_cs = ea.lsave.cs + slot * cap; b_beta = ea.lsave.beta + slot * cap; b_bend = ea.lsave.bend + slot * NEP_MAX_BEND;
    } else {
      W.n_alpha = s_st.n_alpha; W.n_bend = s_st.n_bend;
      W.id = (ent_lds_short)&s_st.id[0]; W.cs = (ent_lds_char)&s_st.cs[0]; W.beta = (ent_lds_double)&s_st.beta[0]; W.bend = (ent_lds_char)&s_st.bend[0];
      B = ea.save + slot;
    }
    auto save = [&]() {
      if constexpr (LISTS) {
        b_na = W.n_alpha; b_nb = W.n_bend;
        for (int i = 0; i < W.n_alpha; i++) { b_id[i] = W.id[i]; b_cs[i] = W.cs[i]; b_beta[i] = W.beta[i]; }
        for (int i = 0; i < W.n_bend; i++) b_bend[i] = W.bend[i];
      } else {
      B->n_alpha = W.n_alpha; B->n_bend = W.n_bend;
      for (int i = 0; i < W.n_alpha; i++) { B->id[i] = W.id[i]; B->cs[i] = W.cs[i]; B->beta[i] = W.beta[i]; }
      for (int i = 0; i < W.n_bend; i++) B->bend[i] = W.bend[i];
      }
    };
    auto restore = [&]() {
      if constexpr (LISTS) {
        W.n_alpha = b_na; W.n_bend = b_nb;
        for (int i = 0; i < W.n_alpha; i++) { W.id[i] = b_id[i]; W.cs[i] = b_cs[i]; W.beta[i] = b_beta[i]; }
        for (int i = 0; i < W.n_bend; i++) W.bend[i] = b_bend[i];
      } else {
      W.n_alpha = B->n_alpha; W.n_bend = B->n_bend;
      for (int i = 0; i < W.n_alpha; i++) { W.id[i] = B->id[i]; W.cs[i] = B->cs[i]; W.beta[i] = B->beta[i]; }
      for (int i = 0; i < W.n_bend; i++) W.bend[i] = B->bend[i];
      }
    };
    unsigned add_tail[kEntAddCap - EntAdd::reg];
    int fl = 0, walked = 0;
    Ev2 pk = own(0);
    // the tether audit: the slot's record and its scene's clock, read once before the walk, written once after it
    nep_tether_audit A{};
    double t0 = 0.0;
    if constexpr (AUDIT) { A = ea.audit[slot]; t0 = *(const double*)(ea.audit_t0 + (long)scene * ea.audit_t0_stride); }
    for (int q = 1; q <= T; q++) {
      const bool first = q == 1;
      const Ev2 pk1 = own(q);
      EntAdd add; add.attach(EntAdd::Store{add_tail, kEntAddCap}); add.clear();
      bool abort = false;
      for (int w = 0; w < n_words; w++) {
        unsigned long long m = s_mask[w] | (first ? s_chg[w] : 0ull);
        while (m) {
          const int i = (w << 6) + __ffsll((long long)m) - 1; m &= m - 1ull;
          walked++;
          const nep_traj_rec* ri = ea.recs + base + i;
          const int nb = rec_nb(ri);
          const Ev2 pik = at(i, q - 1), pik1 = at(i, q);
          // the other agent's bend points at the previous check: the list it published a round ago at the call's first step (an empty
          // one is taken as the current one, as trajCB does for a first message, neptune_ros.cpp:423), later the same list
          int nq = nb;
          if (first && ea.prev_n) { const int n0 = prev_nb(ea, base + i); nq = n0 >= 1 ? n0 : nb; }
          if (nq == nb) ent_cross_agent(add, pk, pk1, pik, pik1, pb_self, nb, &ri->bend[0][0], i + 1);
          else abort |= ent_cross_agent_changed(add, pk, pk1, pik, pik1, pb_self, nb, &ri->bend[0][0], nq, prev_bends(ea, base + i), i + 1);
        }
      }
      ent_cross_static(add, pk, pk1, ec);
      if constexpr (AUDIT) {
        nep_tether_audit_impl::TetherTick tk;
        tk.t = t0 + (double)q * ea.audit_dt;
        fl |= ent_track_move_any<true>(add, &W, save, restore, pk, pk1, pb_self, ec, ea.cable, abort, &tk);
        nep_tether_audit_impl::tether_audit_tick(&A, tk);
      } else
      fl |= ent_track_move(add, &W, save, restore, pk, pk1, pb_self, ec, ea.cable, abort);
      pk = pk1;
    }
    if constexpr (AUDIT) ea.audit[slot] = A;
    if constexpr (LISTS) {
      for (int i = W.n_bend; i < NEP_MAX_BEND; i++) W.bend[i] = 0;
      s_cnt[0] = W.n_alpha; s_cnt[1] = W.n_bend;
      if (predict && W.n_alpha > NEP_FE_ENT_CAP) {      // the state at A does not fit the record the front end takes: the slot sits this round out
        fl |= NEP_ENT_TRACK_HELD;
        if (ea.held) ea.held[slot] += 1;
        if (ea.hold_mask) ea.hold_mask[slot] = 0;
      }
    } else {
    // what the record holds beyond its counts is zero: the bytes of a state depend on the state alone
    for (int i = W.n_alpha; i < NEP_FE_ENT_CAP; i++) { W.id[i] = 0; W.cs[i] = 0; W.beta[i] = 0.0; }
    for (int i = W.n_bend; i < NEP_MAX_BEND; i++) W.bend[i] = 0;
    s_st.n_alpha = W.n_alpha; s_st.n_bend = W.n_bend;
    }
    ea.flags[slot] = fl;
    if (ea.ever) ea.ever[slot] |= fl;
    if (ea.walked) ea.walked[slot] += walked;
    if (fl & NEP_ENT_TRACK_CAP) atomicOr(ea.gflags, NEP_FLAG_ENT_TRACK);
  }
  __syncthreads();
  if constexpr (LISTS) {
    const int n_out = s_cnt[0], nb_out = s_cnt[1];
    if (predict) {      // the fixed record at A: the list where it fits, zeros where it does not (and beyond the counts)
      const bool fits = n_out <= NEP_FE_ENT_CAP;
      for (int i = lane; i < NEP_FE_ENT_CAP; i += 64) {
        const bool on = fits && i < n_out;
        dst->id[i] = on ? (short)WL.id[i] : (short)0; dst->cs[i] = on ? (signed char)WL.cs[i] : (signed char)0; dst->beta[i] = on ? (double)WL.beta[i] : 0.0;
      }
      if (lane < NEP_MAX_BEND) dst->bend[lane] = fits && lane < nb_out ? (signed char)WL.bend[lane] : (signed char)0;
      if (lane == 0) { dst->n_alpha = fits ? n_out : 0; dst->n_bend = fits ? nb_out : 0; }
    } else {            // the lists in place; what a shorter list leaves behind is zeroed (beyond n_in they are zero as they came)
      for (int i = lane; i < max(n_out, n_in); i += 64) {
        const long e = slot * cap + i; const bool on = i < n_out;
        L.id[e] = on ? (short)WL.id[i] : (short)0; L.cs[e] = on ? (signed char)WL.cs[i] : (signed char)0; L.beta[e] = on ? (double)WL.beta[i] : 0.0;
      }
      if (lane < NEP_MAX_BEND) L.bend[slot * NEP_MAX_BEND + lane] = WL.bend[lane];
      if (lane == 0) { L.n_alpha[slot] = n_out; L.n_bend[slot] = nb_out; }
    }
  } else {
  for (int i = lane; i < (int)(sizeof(nep_fe_ent_state) / 4); i += 64) ((int*)dst)[i] = ((const int*)&s_st)[i];
  }
}
__global__ __launch_bounds__(64) void tether_step_kernel(TetherArgs ea) { tether_step<false, false>(ea); }
__global__ __launch_bounds__(64) void tether_step_lists_kernel(TetherArgs ea) { tether_step<true, false>(ea); }
// the audited twins (ea.audit != null): the same moves, and one tick per move into the slot's nep_tether_audit
__global__ __launch_bounds__(64) void tether_step_audit_kernel(TetherArgs ea) { tether_step<false, true>(ea); }
__global__ __launch_bounds__(64) void tether_step_lists_audit_kernel(TetherArgs ea) { tether_step<true, true>(ea); }

// The bulk-synchronous loop's state at A from the list form (nep_batch_ent_lists_at_a), one thread per slot: the fixed record where the
// list fits it; where it holds more than NEP_FE_ENT_CAP crossings a zeroed record, NEP_ENT_TRACK_HELD, one more held round and a
// cleared entry in the round's mask — the rule of the fleet's prediction.  A malformed list gives a zeroed record and is not held:
// the tracking flags it.
__global__ void ent_lists_at_a_kernel(TetherArgs ea, const int* mask_in) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (long)ea.n_scenes * ea.N) return;
  const nep_ent_lists& L = ea.lists;
  nep_fe_ent_state* dst = ea.out + slot;
  const bool ok = ent_lists_ok(L, slot);
  const int na = ok ? L.n_alpha[slot] : 0, nb = ok ? L.n_bend[slot] : 0;
  const bool fits = na <= NEP_FE_ENT_CAP;
  dst->n_alpha = fits ? na : 0; dst->n_bend = fits ? nb : 0;
  for (int i = 0; i < NEP_FE_ENT_CAP; i++) {
    const bool on = fits && i < na; const long e = slot * L.cap + i;
    dst->id[i] = on ? L.id[e] : (short)0; dst->cs[i] = on ? L.cs[e] : (signed char)0; dst->beta[i] = on ? L.beta[e] : 0.0;
  }
  for (int k = 0; k < NEP_MAX_BEND; k++) dst->bend[k] = fits && k < nb ? (signed char)L.bend[slot * NEP_MAX_BEND + k] : (signed char)0;
  if (ea.flags) ea.flags[slot] = fits ? 0 : NEP_ENT_TRACK_HELD;
  if (!fits && ea.held) ea.held[slot] += 1;
  ea.hold_mask[slot] = (mask_in ? mask_in[slot] != 0 : true) && fits ? 1 : 0;
}

// One wave per scene: the slots ever flagged NEP_ENT_TRACK_ENTANGLED, into the scene's counter [7] (no atomics: recounted per call)
__global__ __launch_bounds__(64) void fleet_ent_count_kernel(TetherArgs ea) {
  const long scene = blockIdx.x;
  int c = 0;
  for (int a = threadIdx.x; a < ea.N; a += 64) c += (ea.ever[scene * ea.N + a] & NEP_ENT_TRACK_ENTANGLED) != 0;
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
  if (threadIdx.x == 0) ea.counters[scene * NEP_FLEET_N_COUNTERS + 7] = c;
}

}  // namespace

bool fleet_ent_fits(int N, int S) { return N <= kMaskWords * 64 && S <= kStatWords * 32; }

void launch_tether_publish(const TetherArgs& ea, bool fleet, hipStream_t st) {
  const long slots = (long)ea.n_scenes * ea.N;
  if (slots <= 0) return;
  hipLaunchKernelGGL(fleet ? fleet_ent_publish_kernel : ent_publish_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, st, ea);
}
void launch_ent_lists_at_a(const TetherArgs& ea, const int* mask_in, hipStream_t st) {
  const long slots = (long)ea.n_scenes * ea.N;
  if (slots <= 0) return;
  hipLaunchKernelGGL(ent_lists_at_a_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, st, ea, mask_in);
}
void launch_tether_steps(const TetherArgs& ea, const FleetArgs& fa, hipStream_t st) {
  const long slots = (long)ea.n_scenes * ea.N;
  if (slots <= 0) return;
  const long total = slots * (ea.n_steps + 1);
  hipLaunchKernelGGL(tether_pos_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ea, fa);
  const bool audit = ea.audit != nullptr && ea.start == nullptr;      // (a prediction flies nothing)
  if (ea.lists.cap) hipLaunchKernelGGL(audit ? tether_step_lists_audit_kernel : tether_step_lists_kernel, dim3((unsigned)slots), dim3(64), ent_list_lds_bytes(ea.lists.cap), st, ea);
  else hipLaunchKernelGGL(audit ? tether_step_audit_kernel : tether_step_kernel, dim3((unsigned)slots), dim3(64), 0, st, ea);
  if (ea.ever && ea.counters) hipLaunchKernelGGL(fleet_ent_count_kernel, dim3((unsigned)ea.n_scenes), dim3(64), 0, st, ea);
}

}  // namespace nep
