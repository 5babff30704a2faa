// fleet_kernels.hip — device form of the committed plan (nep_batch_fleet_*, include/neptune_fleet.h): plan ring, point A, splice,
// trajectory composition and the control tick of every (scene, agent) slot.  The arithmetic is plan_common.h's, which the host
// library (plan_host.cpp) shares; the device equals the host chain bit for bit — built -ffp-contract=off like audit_kernels.hip.
// Copy-and-index work: select and tick touch a ring at one or two states per slot (one thread each); commit moves up to
// max_states x 96 B per accepted slot and runs one wave per slot, the copies 16 B per lane on consecutive addresses.
#include <hip/hip_runtime.h>

#define NEP_PLAN_FN __device__ inline
#include "nep_device.h"
#include "plan_common.h"

namespace nep {

using namespace nep_plan_impl;

static_assert(sizeof(nep_pwp) == 1680 && sizeof(nep_pwp) % 16 == 0, "the trajectory is copied in 16-byte units");
static_assert(sizeof(nep_traj_rec) - sizeof(nep_pwp) == 192, "select_kernel writes the record's head field by field");
static_assert(sizeof(nep_fleet_cfg) == 80, "nep_fleet_cfg is mirrored by hand in neptune_amd/abi.py");

namespace {

constexpr int kPwpDoubles = (int)(sizeof(nep_pwp) / sizeof(double));      // 210: (n_seg, _pad), times[17], coeff[3][16][4]
constexpr int kPwpUnits = (int)(sizeof(nep_pwp) / 16);                    // 105

__device__ inline nep_plan_cfg plan_cfg(const nep_fleet_cfg& c) {
  nep_plan_cfg p;
  p.dc = c.dc; p.T_span = c.T_span; p.lower_bound_runtime = c.lower_bound_runtime; p.upper_bound_runtime = c.upper_bound_runtime;
  p.runtime_opt = c.runtime_opt; p.factor_alpha = c.factor_alpha; p.deltaT0 = c.deltaT0; p._pad = 0;
  return p;
}

// nep_plan_reset of every slot, and the scenes' clocks and counters
__global__ void fleet_seed_kernel(FleetArgs fa, const double* __restrict__ state0) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (long)fa.n_scenes * fa.N) return;
  double* r = fa.ring + slot * fa.cap * 12;
  for (int i = 0; i < 12; i++) { const double v = state0[slot * 12 + i]; r[i] = v; fa.state[slot * 12 + i] = v; }
  fa.head[slot] = 0; fa.size[slot] = 1; fa.k_end[slot] = 0;
  fa.flown[slot] = 0; fa.done[slot] = 0; fa.outcome[slot] = NEP_FLEET_SKIPPED; fa.sflags[slot] = 0;
  double* w = (double*)(fa.pwp + slot);
  for (int i = 0; i < kPwpDoubles; i++) w[i] = 0.0;
  if (slot % fa.N == 0) {
    const long scene = slot / fa.N;
    fa.t_now[scene] = fa.cfg.t0; fa.round[scene] = 0; fa.origin[scene] = (int)scene;
    for (int i = 0; i < NEP_FLEET_N_COUNTERS; i++) fa.counters[scene * NEP_FLEET_N_COUNTERS + i] = 0;
  }
}

// One thread per slot: point A (nep_plan_select_a's rule), the start of the search, the published record, the round's mask.
__global__ void fleet_select_kernel(FleetArgs fa) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (long)fa.n_scenes * fa.N) return;
  const long scene = slot / fa.N; const int a = (int)(slot - scene * fa.N);
  const double t_now = fa.t_now[scene];
  const int size = fa.size[slot], head = fa.head[slot], cap = fa.cap;
  const double* ring = fa.ring + slot * cap * 12;
  const double* st = fa.state + slot * 12;
  const nep_plan_cfg pc = plan_cfg(fa.cfg);
  const SelectA s = select_a_index(&pc, size, fa.cfg.deltaT0);
  int ia = head + s.k_index; if (ia >= cap) ia -= cap;
  double A[12];
  for (int i = 0; i < 12; i++) A[i] = ring[(long)ia * 12 + i];
  const double pos[3] = {st[0], st[1], st[2]};
  select_a_fix(A, s.future_index, ring + (long)head * 12, pos);
  fa.k_end[slot] = s.k_index_end;
  nep_fe_start* o = fa.start + slot;
  for (int i = 0; i < 3; i++) { o->pos[i] = A[i]; o->vel[i] = A[3 + i]; o->accel[i] = A[6 + i]; o->goal[i] = fa.goal[slot * 3 + i]; }
  o->t_start = t_now + (double)(fa.cfg.k_a + 1) * fa.cfg.dc;
  if (fa.clock) fa.clock[slot].t_start = t_now + fa.cfg.dc;
  if (fa.active_out) {
    bool on = !fa.done[slot];
    if (fa.period) { const int p = fa.period[slot] < 1 ? 1 : fa.period[slot]; on = on && (fa.round[scene] - fa.phase[slot]) % p == 0; }
    fa.active_out[slot] = on ? 1 : 0;
  }
  // the record the agent publishes (publishOwnTraj): every byte is written
  nep_traj_rec* r = fa.recs + slot;
  r->id = a + 1; r->is_agent = 1; r->n_bend = 1; r->valid = 1;
  for (int i = 0; i < 3; i++) { r->bbox[i] = 2 * fa.drone_radius; r->pos[i] = pos[i]; }
  r->bend[0][0] = fa.pb[2 * a]; r->bend[0][1] = fa.pb[2 * a + 1];
  for (int i = 1; i < NEP_MAX_BEND; i++) { r->bend[i][0] = 0.0; r->bend[i][1] = 0.0; }
  double* w = (double*)&r->pwp;
  if (fa.flown[slot]) {
    const double* src = (const double*)(fa.pwp + slot);
    for (int i = 0; i < kPwpDoubles; i++) w[i] = src[i];
  } else {                                  // not flying yet: a one-interval hover
    for (int i = 1; i < kPwpDoubles; i++) w[i] = 0.0;
    r->pwp.n_seg = 1; r->pwp._pad = 0;
    r->pwp.times[0] = t_now; r->pwp.times[1] = t_now + 1000.0;
    for (int ax = 0; ax < 3; ax++) r->pwp.coeff[ax][0][3] = pos[ax];
  }
}

// One wave (one 64-thread workgroup) per slot.  Everything that decides the outcome is loaded from addresses that are the same in
// every lane, so the outcome and every branch on it are wave-uniform.  The new trajectory is assembled in LDS by all lanes; lane 0
// composes it with the committed one (at most NEP_TRAJ_MAX_SEG intervals, serial) into a second LDS record; only when that and the
// ring's capacity hold is anything written: the trajectory and the states go out in 16-byte units, consecutive lanes on
// consecutive addresses.
__global__ __launch_bounds__(64) void fleet_commit_kernel(FleetArgs fa) {
  __shared__ __attribute__((aligned(16))) nep_pwp s_new;
  __shared__ __attribute__((aligned(16))) nep_pwp s_res;
  __shared__ int s_ok;
  const long slot = blockIdx.x;
  const int lane = threadIdx.x;
  const long scene = slot / fa.N;
  const nep_solution* sol = fa.sol + slot;
  const int K = sol->K, status = sol->stats.status;
  int oc;
  if ((fa.active && !fa.active[slot]) || fa.done[slot]) oc = NEP_FLEET_SKIPPED;
  else if (fa.fres[slot].status == NEP_FE_NO_SOLUTION || K == 0) oc = NEP_FLEET_FE_NO_SOLUTION;
  else if (status == NEP_FAILED) oc = NEP_FLEET_QP_FAILED;
  else if (!fa.accept[slot]) oc = NEP_FLEET_REJECTED;
  else oc = NEP_FLEET_ACCEPTED;
  if (oc == NEP_FLEET_ACCEPTED) {
    const int ns = sol->n_states, size = fa.size[slot], head = fa.head[slot], cap = fa.cap;
    const int keep = splice_keep(size, fa.k_end[slot]);
    const bool flown = fa.flown[slot] != 0;
    int bad = 0;
    if (keep < 0) bad |= NEP_FLEET_FLAG_SPLICE;
    else if (ns < 0 || ns > fa.max_states || keep + ns > cap || keep + ns < 1) bad |= NEP_FLEET_FLAG_RING;
    if (K < 1 || K > NEP_MAX_POL) bad |= NEP_FLEET_FLAG_SEG;
    if (!bad) {
      double* w = (double*)&s_new;
      for (int i = lane; i < kPwpDoubles; i += 64) {
        double v = 0.0;
        if (i >= 1 && i < 2 + NEP_TRAJ_MAX_SEG) { if (i - 1 <= K) v = sol->times[i - 1]; }
        else if (i >= 2 + NEP_TRAJ_MAX_SEG) {
          const int j = i - (2 + NEP_TRAJ_MAX_SEG), ax = j / (4 * NEP_TRAJ_MAX_SEG), r = j - ax * (4 * NEP_TRAJ_MAX_SEG), seg = r >> 2, c = r & 3;
          if (seg < K) v = sol->coeff[ax][seg][c];
        }
        if (i > 0) w[i] = v;
      }
      if (lane == 0) { s_new.n_seg = K; s_new._pad = 0; s_ok = 1; }
      __syncthreads();
      if (flown && lane == 0) s_ok = compose_exact(fa.t_now[scene], fa.pwp + slot, &s_new, &s_res) ? 1 : 0;
      __syncthreads();
      if (!s_ok) bad |= NEP_FLEET_FLAG_SEG;
    }
    if (bad) {
      oc = NEP_FLEET_CAP;
      if (lane == 0) { fa.sflags[slot] |= bad; atomicOr(fa.gflags, NEP_FLAG_FLEET); }      // (the capacity path: never taken by a loop sized as the header says)
    } else {
      const double2* src = (const double2*)(flown ? &s_res : &s_new);
      double2* dst = (double2*)(fa.pwp + slot);
      for (int u = lane; u < kPwpUnits; u += 64) dst[u] = src[u];
      // the splice: A and what follows go, the solution's states come (a state is six 16-byte units; the ring wraps at most once)
      const double2* sin = (const double2*)(fa.states_in + slot * fa.max_states * 12);
      double2* ring = (double2*)(fa.ring + slot * cap * 12);
      const int ru = cap * 6;
      int start = head + keep; if (start >= cap) start -= cap;
      start *= 6;
      for (int u = lane; u < ns * 6; u += 64) { int d = start + u; if (d >= ru) d -= ru; ring[d] = sin[u]; }
      if (lane == 0) { fa.size[slot] = keep + ns; fa.flown[slot] = 1; }
    }
  }
  if (lane == 0) { fa.outcome[slot] = oc; if (fa.outcome_out) fa.outcome_out[slot] = oc; }
}

// One wave per scene: the round's outcomes counted into the scene's counters (lanes stride over the agents, a butterfly sums them)
__global__ __launch_bounds__(64) void fleet_count_kernel(FleetArgs fa) {
  const long scene = blockIdx.x;
  const int lane = threadIdx.x;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
  for (int a = lane; a < fa.N; a += 64) {
    const long slot = scene * fa.N + a;
    const int oc = fa.outcome[slot];
    c0 += oc == NEP_FLEET_SKIPPED; c1 += oc == NEP_FLEET_FE_NO_SOLUTION; c2 += oc == NEP_FLEET_QP_FAILED; c3 += oc == NEP_FLEET_REJECTED;
    c4 += oc == NEP_FLEET_ACCEPTED; c5 += oc == NEP_FLEET_CAP;
    c6 += oc == NEP_FLEET_ACCEPTED && fa.sol[slot].stats.status == NEP_RELAXED;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    c0 += __shfl_xor(c0, m, 64); c1 += __shfl_xor(c1, m, 64); c2 += __shfl_xor(c2, m, 64); c3 += __shfl_xor(c3, m, 64);
    c4 += __shfl_xor(c4, m, 64); c5 += __shfl_xor(c5, m, 64); c6 += __shfl_xor(c6, m, 64);
  }
  if (lane == 0) {
    int* c = fa.counters + scene * NEP_FLEET_N_COUNTERS;
    c[0] += c0; c[1] += c1; c[2] += c2; c[3] += c3; c[4] += c4; c[5] += c5; c[6] += c6;
  }
}

// One thread per slot: round_ticks control periods of the perfect tracker (nep_plan_next_goal per period; only the last front is
// loaded), the scene's clock, the sticky arrival test, the round counter.
__global__ void fleet_tick_kernel(FleetArgs fa) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (long)fa.n_scenes * fa.N) return;
  const int cap = fa.cap;
  int head = fa.head[slot], size = fa.size[slot], front = head;
  for (int k = 0; k < fa.cfg.round_ticks; k++) {
    front = head;
    if (size > 1) { head = head + 1 == cap ? 0 : head + 1; size--; }
  }
  fa.head[slot] = head; fa.size[slot] = size;
  const double* g = fa.ring + (slot * cap + front) * 12;
  double s[12];
  for (int i = 0; i < 12; i++) { s[i] = g[i]; fa.state[slot * 12 + i] = s[i]; }
  const double dx = s[0] - fa.goal[slot * 3], dy = s[1] - fa.goal[slot * 3 + 1];
  if (sqrt(dx * dx + dy * dy) < fa.cfg.goal_radius && sqrt(s[3] * s[3] + s[4] * s[4]) < 0.05) fa.done[slot] = 1;
  if (slot % fa.N == 0) {
    const long scene = slot / fa.N;
    double t = fa.t_now[scene];
    for (int k = 0; k < fa.cfg.round_ticks; k++) t += fa.cfg.dc;
    fa.t_now[scene] = t;
    fa.round[scene] = fa.round[scene] + 1;
  }
}

}  // namespace

void launch_fleet_seed(const FleetArgs& fa, const double* state0, hipStream_t st) {
  const long slots = (long)fa.n_scenes * fa.N;
  hipLaunchKernelGGL(fleet_seed_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, fa, state0);
}
void launch_fleet_select(const FleetArgs& fa, hipStream_t st) {
  const long slots = (long)fa.n_scenes * fa.N;
  hipLaunchKernelGGL(fleet_select_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, st, fa);
}
void launch_fleet_commit(const FleetArgs& fa, hipStream_t st) {
  const long slots = (long)fa.n_scenes * fa.N;
  hipLaunchKernelGGL(fleet_commit_kernel, dim3((unsigned)slots), dim3(64), 0, st, fa);
  hipLaunchKernelGGL(fleet_count_kernel, dim3((unsigned)fa.n_scenes), dim3(64), 0, st, fa);
}
void launch_fleet_tick(const FleetArgs& fa, hipStream_t st) {
  const long slots = (long)fa.n_scenes * fa.N;
  hipLaunchKernelGGL(fleet_tick_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, fa);
}

}  // namespace nep
