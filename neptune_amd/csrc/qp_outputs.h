// qp_outputs.h — the writers of what a replan leaves behind: the trajectory (nep_solution: coefficients, knot times), generatePwpOut's
// sampled states, and the record the agent publishes (d_commit).  Called by NT cooperating threads of which the caller is thread `tid`;
// theta is the trajectory as [3][NEP_MAX_POL][4] (axis, segment, a b c d).  Callers: qp_kernel and skipped_replan_kernel (everything
// they write), the certificate of qp_presolve.h (write_trajectory, sched_states), qp_reg_kernel (everything but the exceptions below), polish_slot (sched_states,
// write_states), sample_kernel (sample_state).
// Sites that keep their own lines, each for a reason stated there (profiles/qp_outputs_kernel_resources.txt, profiles/qp_outputs_ab.txt):
// the carry-over loop in the main tails of qp_kernel and qp_reg_kernel (carry_commit serves skipped_replan_kernel), and the trajectory
// and record stores of polish_slot.  A field added to nep_traj_rec is added in write_commit and in polish_slot;
// tests/test_gpu_replan_outputs.py checks every site field by field.
// The translation units that sample states or write records through this compile with fp contraction on: the bracketing of the
// sampling expressions is what the oracle is compared against at 1e-12 and stays exactly as it is.  geom_kernels.hip (no contraction)
// includes it through qp_presolve.h for write_trajectory and sched_states alone, which do not depend on the flag.
#pragma once
#include "nep_device.h"

namespace nep {

// states of the schedule of K that fit the caller's buffer (sol->n_states)
__device__ __forceinline__ int sched_states(const SceneParams& sp, const SampleSched& sched, int K) {
  const int ns_all = sched.n[K];
  return ns_all < sp.max_states ? ns_all : sp.max_states;
}

// one state (pos, vel, accel, jerk: solver_gurobi_poly.cpp:921-929) of segment i at dt from its start
__device__ __forceinline__ void sample_state(const double* theta, int i, double dt, double* st) {
  for (int ax = 0; ax < 3; ax++) {
    const double* c = theta + (ax * NEP_MAX_POL + i) * 4;
    st[ax] = ((c[0] * (dt * dt * dt) + c[1] * (dt * dt)) + c[2] * dt) + c[3];
    st[3 + ax] = (c[0] * (3 * dt * dt) + c[1] * (2 * dt)) + c[2];
    st[6 + ax] = c[0] * (6 * dt) + c[1] * 2;
    st[9 + ax] = c[0] * 6;
  }
}

// generatePwpOut's samples (:911-934): the first ns states of the schedule of K
template <int NT>
__device__ __forceinline__ void write_states(const SceneParams& sp, const ProblemSet& ps, const SampleSched& sched, int slot, const double* theta, int K, int ns, int tid) {
  if (!ps.states) return;
  for (int s = tid; s < ns; s += NT)
    sample_state(theta, sched.seg[K * sp.max_states + s], sched.dt[K * sp.max_states + s], ps.states + ((long)slot * sp.max_states + s) * NEP_STATE_DOUBLES);
}

// the masked coefficients and the knot times of the solution (:898: times = i * T_span + t_start).  t_start is a pointer into the guess:
// only the threads that store a knot time load it, after the coefficient stores are issued
template <int NT>
__device__ __forceinline__ void write_trajectory(nep_solution* sol, const double* theta, int K, const double* t_start, double T, int tid) {
  for (int t = tid; t < 3 * NEP_MAX_POL * 4; t += NT) (&sol->coeff[0][0][0])[t] = ((t % (NEP_MAX_POL * 4)) / 4 < K) ? theta[t] : 0.0;
  // (the knot time as every contracting caller always compiled it, one fused operation, written out: the certificate's tail in
  // geom_kernels.hip, a translation unit without contraction, must store the same bytes — qp_presolve.h)
  if (tid <= NEP_MAX_POL) sol->times[tid] = (tid <= K) ? __builtin_fma((double)tid, T, *t_start) : 0.0;
}

// the record the agent would publish (neptune_ros.cpp:434-480)
template <int NT>
__device__ __forceinline__ void write_commit(const SceneParams& sp, const ProblemSet& ps, int slot, const double* theta, int K, const double* t_start, double T, int tid) {
  nep_traj_rec* cr = ps.commit + slot;
  const int own = sp.first_local + (slot % sp.n_local);
  if (tid == 0) {
    cr->id = own + 1; cr->is_agent = 1; cr->n_bend = 1; cr->valid = 1;
    for (int a = 0; a < 3; a++) { cr->bbox[a] = 2 * sp.drone_radius; cr->pos[a] = theta[(a * NEP_MAX_POL) * 4 + 3]; }
    cr->bend[0][0] = ps.pb[2 * own]; cr->bend[0][1] = ps.pb[2 * own + 1];
    cr->pwp.n_seg = K;
  }
  if (tid <= NEP_TRAJ_MAX_SEG) cr->pwp.times[tid] = (tid <= K) ? *t_start + tid * T : 0.0;
  for (int e = tid; e < 3 * NEP_TRAJ_MAX_SEG * 4; e += NT) {
    const int ax = e / (NEP_TRAJ_MAX_SEG * 4), r = e % (NEP_TRAJ_MAX_SEG * 4), seg = r / 4, j = r % 4;
    (&cr->pwp.coeff[0][0][0])[e] = (seg < K) ? theta[(ax * NEP_MAX_POL + seg) * 4 + j] : 0.0;
  }
}

// A slot that publishes nothing keeps its record: with the previous records at hand (nep_batch_replan's d_committed) the one of
// (scene, own) is carried over; otherwise d_commit[slot] is left as the caller passed it (the usual round loop hands the buffer that
// holds the previous round's records).
template <int NT>
__device__ __forceinline__ void carry_commit(const SceneParams& sp, const ProblemSet& ps, int slot, int tid) {
  if (!ps.prev_commit) return;
  const int own = sp.first_local + (slot % sp.n_local);
  const double* src = (const double*)(ps.prev_commit + (long)(slot / sp.n_local) * sp.num_agents + own);
  double* dst = (double*)(ps.commit + slot);
  for (int e = tid; e < (int)(sizeof(nep_traj_rec) / sizeof(double)); e += NT) dst[e] = src[e];
}

// LPs attempted and LPs without a separating line of the slot, over its segments (one thread)
__device__ __forceinline__ void lp_totals(const ProblemSet& ps, int slot, int& n_lp, int& n_lpf) {
  n_lp = 0; n_lpf = 0;
  if (ps.lp_stats && !ps.lines_override) {
    int v[2 * NEP_MAX_POL];
#pragma unroll
    for (int i = 0; i < 2 * NEP_MAX_POL; i++) v[i] = ps.lp_stats[(long)slot * NEP_MAX_POL * 2 + i];   // one round trip
#pragma unroll
    for (int i = 0; i < NEP_MAX_POL; i++) { n_lp += v[2 * i]; n_lpf += v[2 * i + 1]; }
  }
}

// the per-replan device time of an interior-point workgroup that started at tick t_wg0, and the next launch's ordering key (8 us bins;
// one thread)
__device__ __forceinline__ void write_solve_time(const SceneParams& sp, const ProblemSet& ps, nep_solution* sol, int slot, long long t_wg0) {
  const long long dt_ = (long long)wall_clock64() - t_wg0;
  const double us_ = (double)dt_ * sp.us_per_tick;
  sol->stats.solve_us = us_;
  if (ps.order_key) {
    const double k_ = us_ * 0.125;
    const int kn = k_ > 63.0 ? 63 : (int)k_, ko = ps.order_key[slot] - sp.qp_key_decay;
    ps.order_key[slot] = (sp.qp_key_decay > 0 && ko > kn) ? ko : kn;
  }
}

}  // namespace nep
