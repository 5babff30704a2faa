// track_kernels.hip — the tether's entangle state carried from one bulk-synchronous round to the next (nep_batch_track_ent,
// include/neptune_frontend.h).
//
// NeptuneRos::odomCB -> updateEntStateStaticObs (reference neptune/src/neptune_ros.cpp:781-850) at every sampled step of the
// round's flown intervals, and publishOwnTraj's bend points (:457-476).  The crossing tests, the list surgery, the bend-point
// update and the tether length are ent_device.h's (the front end's and the safety pass's code); nep_ent_track_step
// (entangle_host.cpp) is the host restatement the kernel equals bit for bit — built -ffp-contract=off like geom_kernels.hip.
#include <hip/hip_runtime.h>

#include "nep_device.h"
#include "../../include/neptune_frontend.h"
#include "../../include/neptune_entangle.h"
#include "ent_device.h"

namespace nep {

// host and device drop a move at the same number of new crossings: the bit-exactness of an overflowing move rests on it
static_assert(kEntAddCap == NEP_ENT_TRACK_ADD_CAP, "nep_ent_track_step's and the kernel's caps on a move's new crossings differ");
static_assert(kEntAddCap <= 32, "EntAdd's cancellation bits are one 32-bit word");

namespace {

// one slot's state is valid input: counts within the fixed record and the bend points a record publishes, bend indices on the list
__device__ bool track_state_ok(const nep_fe_ent_state* st) {
  if (st->n_alpha < 0 || st->n_alpha > NEP_FE_ENT_CAP || st->n_bend < 0 || st->n_bend > NEP_MAX_BEND - 1) return false;
  for (int k = 0; k < st->n_bend; k++) if (st->bend[k] < 0 || st->bend[k] >= st->n_alpha) return false;
  return true;
}

// One thread per (scene, agent): the agent and everybody else fly the round's intervals 1..n_iv along d_records, cut into ns steps
// each; every step is one updateEntStateStaticObs of the agent's own state.  The working state sits in LDS (the surgery is a chain of
// dependent reads); a copy of it goes to global scratch before a step that can outgrow the record, and comes back if it did.
__global__ __launch_bounds__(64) void ent_track_kernel(TrackArgs ta) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tr_lds[];
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = ta.N;
  if (idx >= (long)ta.n_scenes * N) return;
  const int scene = (int)(idx / N), a = (int)(idx % N);
  const long base = (long)scene * N;
  int fl = 0;
  if (!ta.present[idx]) { ta.flags[idx] = 0; return; }      // (no trajectory to fly: state and record stay)
  nep_fe_ent_state* W = (nep_fe_ent_state*)tr_lds + threadIdx.x;
  nep_fe_ent_state* B = ta.save + idx;
  ent_copy(W, ta.ent + idx);
  if (!track_state_ok(W)) { ta.flags[idx] = NEP_ENT_TRACK_CAP; atomicOr(ta.gflags, NEP_FLAG_ENT_TRACK); return; }
  EntCtx ec;
  ec.N = N; ec.S = ta.S; ec.own = a; ec.num_pol = ta.num_pol; ec.ns = ta.ns; ec.T_span = 0.0; ec.cable = ta.cable;
  ec.pb = ta.pb; ec.srep = ta.srep + (long)scene * ta.static_stride * 4; ec.slong = ta.slong + (long)scene * ta.static_stride * 2;
  ec.sampled = ta.sampled; ec.present = ta.present; ec.ps = nullptr; ec.scene = scene; ec.n_hull = N;
  const Ev2 pb_self = ent_pb(ec, a);
  const int per = ta.num_pol * (ta.ns + 1);
  // the point of agent j after step q of the round (q = 0: the start): the samples of ent_sample_kernel, the end of an interval
  // standing for the start of the next one (what the previous check saw is where the next one starts)
  auto at = [&](long j, int itv, int col) { const double* p = ta.sampled + ((base + j) * per + (long)itv * (ta.ns + 1) + col) * 2; return Ev2{p[0], p[1]}; };
  unsigned add_tail[kEntAddCap - EntAdd::reg];
  Ev2 pk = at(a, 0, 0);
  for (int itv = 0; itv < ta.n_iv; itv++) {
    for (int j = 1; j <= ta.ns; j++) {
      const bool first = itv == 0 && j == 1;
      const Ev2 pk1 = at(a, itv, j);
      EntAdd add; add.attach(EntAdd::Store{add_tail, kEntAddCap}); add.clear();
      bool abort = false;
      for (int i = 0; i < N; i++) {
        if (i == a || !ta.present[base + i]) continue;
        const nep_traj_rec* ri = ta.recs + base + i;
        const int nb = min(max(ri->n_bend, 0), NEP_MAX_BEND);
        if (nb < 1) continue;
        const Ev2 pik = j == 1 && itv > 0 ? at(i, itv - 1, ta.ns) : at(i, itv, j - 1), pik1 = at(i, itv, j);
        // the other agent's bend points at the previous check: its previous record's at the round's first step (one trajCB per
        // round; an empty list is taken as the current one, as trajCB does for a first message, neptune_ros.cpp:423), later the same
        const nep_traj_rec* qi = ta.prev + base + i;
        int nq = nb;
        if (first) { const int n0 = min(max(qi->n_bend, 0), NEP_MAX_BEND); nq = n0 >= 1 ? n0 : nb; }
        if (nq == nb) ent_cross_agent(add, pk, pk1, pik, pik1, pb_self, nb, &ri->bend[0][0], i + 1);
        else abort |= ent_cross_agent_changed(add, pk, pk1, pik, pik1, pb_self, nb, &ri->bend[0][0], nq, &qi->bend[0][0], i + 1);
      }
      ent_cross_static(add, pk, pk1, ec);
      if (add.overflow) { fl |= NEP_ENT_TRACK_CAP; pk = pk1; continue; }
      const bool may_outgrow = add.n > 0 || W->n_bend >= NEP_MAX_BEND - 1;
      if (may_outgrow) ent_copy(B, W);
      bool over = add.n > 0 && ent_merge(add, W, pk, pb_self, ec);
      if (!over) { ent_update_bends(W, pk1, pb_self, ec); over = W->n_bend > NEP_MAX_BEND - 1; }
      if (over) { ent_copy(W, B); fl |= NEP_ENT_TRACK_CAP; pk = pk1; continue; }
      if (abort) fl |= NEP_ENT_TRACK_ABORT;
      for (int e = 0; e < W->n_alpha; e++) {      // active_cases of the agents: entries per id
        const int id_ = W->id[e];
        if (id_ > N) continue;
        const int k = ent_count(W->id, W->n_alpha, id_);
        if (k > 2) fl |= NEP_ENT_TRACK_ENTANGLED;
        if (k >= 2) fl |= NEP_ENT_TRACK_TWO_CASES;
      }
      if (ent_tether(W, pb_self, pk1, ec) > ta.cable) fl |= NEP_ENT_TRACK_TOO_LONG;
      pk = pk1;
    }
  }
  ent_copy(ta.ent + idx, W);
  ta.flags[idx] = fl;
  if (fl & NEP_ENT_TRACK_CAP) atomicOr(ta.gflags, NEP_FLAG_ENT_TRACK);
}

// publishOwnTraj's bend points (neptune_ros.cpp:457-476): the base, then the anchor of every bend index of the state just tracked.
// A kernel of its own: the tracking reads every record's current bend points, so none may change before all of them have run.
__global__ void ent_publish_kernel(TrackArgs ta) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int N = ta.N;
  if (idx >= (long)ta.n_scenes * N || !ta.present[idx]) return;
  const nep_fe_ent_state* st = ta.ent + idx;
  if (!track_state_ok(st)) return;
  const int scene = (int)(idx / N), a = (int)(idx % N);
  const double* srep = ta.srep + (long)scene * ta.static_stride * 4;
  nep_traj_rec* r = ta.recs + idx;
  r->bend[0][0] = ta.pb[2 * a]; r->bend[0][1] = ta.pb[2 * a + 1];
  for (int k = 0; k < st->n_bend; k++) {
    const int id = st->id[st->bend[k]], cs = st->cs[st->bend[k]];
    double x = 0.0, y = 0.0;
    if (id >= 1 && id <= N) { x = ta.pb[2 * (id - 1)]; y = ta.pb[2 * (id - 1) + 1]; }      // (an agent's base: its beta is 0.0, so it never becomes one)
    else if (id > N && id - N - 1 < ta.S && (cs == 0 || cs == 1)) { x = srep[((id - N - 1) * 2 + cs) * 2]; y = srep[((id - N - 1) * 2 + cs) * 2 + 1]; }
    r->bend[k + 1][0] = x; r->bend[k + 1][1] = y;
  }
  r->n_bend = 1 + st->n_bend;
}

}  // namespace

void launch_ent_track(const TrackArgs& ta, hipStream_t st) {
  const long total = (long)ta.n_scenes * ta.N;
  if (total <= 0) return;
  const unsigned blocks = (unsigned)((total + 63) / 64);
  hipLaunchKernelGGL(ent_track_kernel, dim3(blocks), dim3(64), 64 * sizeof(nep_fe_ent_state), st, ta);
  hipLaunchKernelGGL(ent_publish_kernel, dim3(blocks), dim3(64), 0, st, ta);
}

}  // namespace nep
