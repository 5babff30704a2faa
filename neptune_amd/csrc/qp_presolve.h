// qp_presolve.h — the zero-iteration certificate of the verified line presolve, in the pieces its two callers share: the kernel of
// its own (qp_presolve_kernel.hip: one wave per replan, after the separator) and the tail of separator_packed_kernel
// (geom_kernels.hip: the same wave that made the lines, when it holds every segment of the slot).
//
// The minimiser of the cost over the equality-reduced variables, z* = -Hax^-1 g per axis, is linear in v = (b0, c0, d0, f) of an
// axis (nep_tables.h: RowMap, ThMap, ObjQ).  When it satisfies every box row, every near separating line and the terminal ball, and
// its control points moved less than the radius that verifies the parked lines and the skipped LPs, it IS the optimum
// (solver_gurobi_poly.cpp:823-882) and the replan is finished here.
//
// The certificate only ever ACCEPTS or ABSTAINS: anything unusual — K < 3, an overflowed line bucket, a violated row, or a control
// point moved beyond the radius that verifies the parked lines and the skipped LPs — leaves the slot unmarked and untouched, and
// qp_reg_kernel<true> handles it exactly as before (iterations, second attempt, redo list, polish list).
//
// The two callers are compiled with different contraction flags (geom_kernels.hip without, the QP kernels with) and must give the
// same bytes: every floating-point expression here is written out — __builtin_fma where the stand-alone kernel always had a fused
// operation (the contracting build of `a * b + c * d` is fma(a, b, c * d), of `s + a * b` fma(a, b, s)), plain operations under
// `#pragma clang fp contract(off)` elsewhere — so that no translation unit's flag decides a rounding.
#pragma once
#include <hip/hip_runtime.h>

#include "nep_device.h"
#include "nep_tables.h"
#include "qp_outputs.h"

namespace nep {

// ((m0 v0 + m1 v1) + m2 v2) + m3 v3
__device__ __forceinline__ double pre_dot4(double m0, double m1, double m2, double m3, double v0, double v1, double v2, double v3) {
#pragma clang fp contract(off)
  return __builtin_fma(m3, v3, __builtin_fma(m2, v2, __builtin_fma(m0, v0, m1 * v1)));
}
// ((T^3 q0 + T^2 q1) + T q2) + q3
__device__ __forceinline__ double pre_cubic(double T, const double* q) {
#pragma clang fp contract(off)
  return __builtin_fma(T, q[2], __builtin_fma(T * T * T, q[0], (T * T) * q[1])) + q[3];
}

// What the certificate knows of a slot before a line is looked at (one wave; per lane unless stated)
struct PreStart {
  double viol;        // the lane's largest violation so far: its box row on the three axes, the terminal ball (-1: none)
  double th[3];       // lanes < 4 K: entry `lane` (segment lane / 4, power lane % 4) of the trajectory at z*, per axis
  double obj;         // the cost at z* (wave-uniform)
  bool moved;         // the lane's control point moved beyond the radius that verifies the parked lines and the skipped LPs
  bool has_qc, z_override;      // wave-uniform: the terminal ball row is posed (:697-702); z keeps the guess (:879-880)
};

// (a) the start point — everything that depends on the guess and the tables alone, its loads issued together: base row `lane` at z*
// on the three axes (positions of the 4 K control points, 3 K velocities, K accelerations; RowMap) against its box, the x, y of the
// position control points into xy[2][32] (the line rows read them), the trajectory's coefficients (ThMap), the terminal ball, the
// movement of the control points against the guess's (computed from the guess's coefficients with the same expression as z*'s),
// the cost.  theta: 96 doubles of LDS the wave may use until it returns; apos: the caller's __constant__ copy of the MINVO position basis
// inverse on [0, 1] (NEP_APOS_INV_LITERALS, nep_tables.h); 3 <= K <= NEP_MAX_POL.
// ---- the movement bound.  A parked line lies farther than the radius r from each of the guess's four control points of its segment
// (separator: -worst > r |n|), a skipped LP's line at least as far (its point sets' boxes are r apart and the box sides are polygon
// edges): a solution control point within r of the guess's is on the right side of every one of them —
// n . Q + d - 1 <= (n . B + d - 1) + |n| |Q - B| < 0 — so the movement bound verifies BOTH, and no parked line is read (qp_reg_kernel
// reads each of them: 96 MB per launch of 8 192 config-4 replans).  One part in 1e9 of slack for the roundings of the two tests; a
// replan that moved farther is the interior-point kernel's (which lists it for the redo pass if need be). ----
__device__ __forceinline__ PreStart pre_start(const SceneParams& sp, const QpTable* __restrict__ tb, const nep_guess* __restrict__ g, int K, int lane, double* xy, double* theta, const double (*apos)[4]) {
#pragma clang fp contract(off)
  PreStart S;
  const double T = sp.T_span;
  const double* gcoef = &g->coeff[0][0][0];
  double rm0 = 0, rm1 = 0, rm2 = 0, rm3 = 0, tm0 = 0, tm1 = 0, tm2 = 0, tm3 = 0, P0 = 0, P1 = 0, P2 = 0, P3 = 0;
  const int rho = lane >> 1, axm = lane & 1, sg = rho >> 2, k = rho & 3;      // the movement bound: lane = (control point rho = 4 sg + k, axis x / y)
  if (lane < 8 * K) { const double* q = tb->RowMap[lane]; rm0 = q[0]; rm1 = q[1]; rm2 = q[2]; rm3 = q[3]; }
  if (lane < 4 * K) { const double* q = tb->ThMap[lane]; tm0 = q[0]; tm1 = q[1]; tm2 = q[2]; tm3 = q[3]; }
  if (lane < 8 * K) { const double* q = gcoef + (axm * 8 + sg) * 4; P0 = q[0]; P1 = q[1]; P2 = q[2]; P3 = q[3]; }
  const double* oq = tb->ObjQ[lane & 3];
  const double oq0 = oq[0], oq1 = oq[1], oq2 = oq[2], oq3 = oq[3];
  const double a0 = apos[0][k], a1 = apos[1][k], a2 = apos[2][k], a3 = apos[3][k];
  double vv[3][4];      // v = (b0, c0, d0, f) per axis (wave-uniform addresses: scalar loads)
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    const double* c0 = g->coeff[ax][0]; const double* cK = g->coeff[ax][K - 1];
    vv[ax][0] = c0[1]; vv[ax][1] = c0[2]; vv[ax][2] = c0[3];      // b0, c0, d0 (:390-396)
    vv[ax][3] = pre_cubic(T, cK);                                  // final_pos_ (:226-228)
  }
  theta[lane] = 0.0; if (lane + 64 < 96) theta[lane + 64] = 0.0;
  S.viol = -1.0;
  if (lane < 8 * K) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      const double a = pre_dot4(rm0, rm1, rm2, rm3, vv[ax][0], vv[ax][1], vv[ax][2], vv[ax][3]);
      const double hi = lane < 4 * K ? sp.maxs[ax] : (lane < 7 * K ? sp.v_max : sp.a_max);
      const double lo = lane < 4 * K ? sp.mins[ax] : (lane < 7 * K ? -sp.v_max : -sp.a_max);
      S.viol = fmax(S.viol, fmax(a - hi, lo - a));
      if (ax < 2 && lane < 4 * K) xy[ax * 32 + lane] = a;
    }
  }
  __syncthreads();
#pragma unroll
  for (int ax = 0; ax < 3; ax++) S.th[ax] = pre_dot4(tm0, tm1, tm2, tm3, vv[ax][0], vv[ax][1], vv[ax][2], vv[ax][3]);
  if (lane < 4 * K) { theta[lane] = S.th[0]; theta[32 + lane] = S.th[1]; theta[64 + lane] = S.th[2]; }
  __syncthreads();
  const double dix = vv[0][2] - vv[0][3], diy = vv[1][2] - vv[1][3], diz = vv[2][2] - vv[2][3];
  const double dxy2 = __builtin_fma(dix, dix, diy * diy);
  S.has_qc = sqrt(__builtin_fma(diz, diz, dxy2)) < 1.0;      // the terminal ball row (:697-702)
  S.z_override = sqrt(dxy2) < 1.0;                           // :879-880
  if (S.has_qc) {      // the terminal ball (:697-702): |p(end) - f|^2 <= 0.1^2, p(end) from the returned coefficients
    double c = -0.10 * 0.10;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) { const double pe = pre_cubic(T, theta + (ax * 8 + (K - 1)) * 4) - vv[ax][3]; c = __builtin_fma(pe, pe, c); }
    S.viol = fmax(S.viol, c);
  }
  S.moved = false;
  {
    const double c0 = (T * T * T) * a0, c1 = (T * T) * a1, c2 = T * a2, c3 = a3;
    const double* Q = theta + (axm * 8 + (lane < 8 * K ? sg : 0)) * 4;
    const double v = pre_dot4(Q[0], Q[1], Q[2], Q[3], c0, c1, c2, c3);
    const double gq = pre_dot4(P0, P1, P2, P3, c0, c1, c2, c3);
    double d2 = (v - gq) * (v - gq);
    d2 += __shfl_xor(d2, 1);                            // (x and y of a control point sit on neighbouring lanes)
    if (lane < 8 * K) S.moved = !(d2 <= sp.cull_radius * sp.cull_radius * (1.0 - 1e-9));
  }
  // the cost at z*: v' ObjQ v per axis (the first problem's cost, :322-383), the twelve terms added in the order (axis, row); every
  // lane makes row `lane & 3` of ObjQ v for the three axes, the sum takes them from lanes 0..3
  double o = 0;
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    const double r_ = __builtin_fma(oq3, vv[ax][3], __builtin_fma(oq2, vv[ax][2], __builtin_fma(oq1, vv[ax][1], __builtin_fma(oq0, vv[ax][0], 0.0))));
#pragma unroll
    for (int a = 0; a < 4; a++) o = __builtin_fma(vv[ax][a], __shfl(r_, a), o);
  }
  S.obj = o;
  return S;
}

// (b) one near separating line against the four control points of its segment (px, py: the segment's four x and y of xy[]):
// the largest n . q + d - 1
__device__ __forceinline__ double pre_line_viol(double n1, double n2, double n3, const double* px, const double* py) {
#pragma clang fp contract(off)
  const double h = 1.0 - n3;
  double viol = -1.0;
#pragma unroll
  for (int k = 0; k < 4; k++) viol = fmax(viol, __builtin_fma(n1, px[k], n2 * py[k]) - h);
  return viol;
}

// (c) the closing: the wave's verdict and, when the certificate holds, the trajectory, the statistics and the mark.  One wave; S is
// pre_start's state with the lines of (b) folded into S.viol; theta: 96 doubles of LDS for the trajectory as [3][NEP_MAX_POL][4];
// L_near / n_far / n_skip the slot's near, parked and skipped lines (counts of buckets that did not overflow — the caller abstains
// on an overflow before it comes here); lpv: lanes 0..15 hold the slot's lp_stats entries.  Returns whether the slot was certified
// (wave-uniform).  It reads nothing from global memory before its verdict.
__device__ __forceinline__ bool pre_close(const SceneParams& sp, const ProblemSet& ps, const SampleSched& sched, int slot, int K, int lane, const PreStart& S,
                                          int L_near, int n_far, int n_skip, int lpv, double* theta, const nep_guess* __restrict__ g, long long t0, int* __restrict__ presolved) {
  const double T = sp.T_span;
  nep_solution* __restrict__ sol = ps.solution + slot;
  // (a lane's violation is never a NaN — it starts at -1 and fmax drops one — so "the largest is <= 0" is "no lane's is > 0")
  if (__ballot(S.viol > 0.0) != 0ull) return false;     // some row is violated at z*: the interior point's job
  if ((n_far > 0 || n_skip > 0) && __ballot(S.moved) != 0ull) return false;      // moved too far to be sure: qp_reg_kernel solves it and checks every parked line

  // ---- the certificate holds: this is the optimum ----
  int n_lp = (lane & 1) == 0 ? lpv : 0, n_lpf = (lane & 1) == 1 ? lpv : 0;
#pragma unroll
  for (int o_ = 8; o_ > 0; o_ >>= 1) { n_lp += __shfl_xor(n_lp, o_); n_lpf += __shfl_xor(n_lpf, o_); }      // (lanes 0..15 hold the values: the sums land in lane 0)
  theta[lane] = 0.0; if (lane + 64 < 96) theta[lane + 64] = 0.0;
  __syncthreads();
  if (lane < 4 * K) { theta[lane] = S.th[0]; theta[32 + lane] = S.th[1]; if (!S.z_override) theta[64 + lane] = S.th[2]; }
  if (S.z_override && lane < 32) theta[64 + lane] = (&g->coeff[2][0][0])[lane];      // :879-880
  __syncthreads();
  write_trajectory<64>(sol, theta, K, &g->t_start, T, lane);
  const int ns = sched_states(sp, sched, K);
  if (lane == 0) {
    const int L_all = L_near + n_far + n_skip;
    sol->stats.status = NEP_OK; sol->stats.iters = 0; sol->stats.iters_first = 0;
    sol->stats.n_lines = L_all - n_lpf; sol->stats.n_lp = n_lp; sol->stats.n_lp_failed = n_lpf;
    sol->stats.n_rows = 48 * K + 4 * (L_near < L_all ? L_near : L_near - n_lpf); sol->stats.qc_active = S.has_qc ? 1 : 0;
    sol->stats.objective = S.obj;
    sol->K = K; sol->n_states = ns;
  }
  // (the sampled states and the commit record — 9.7 KB per replan, 80 MB per launch of 8 192: a third of the stand-alone kernel's 70 us
  // when they were written there — are written from the returned coefficients by the slot's workgroup of the interior-point launch that
  // follows, qp_reg_kernel's first lines: there they overlap the iterating replans' arithmetic instead of standing alone)
  if (lane == 0) {
    const double us_ = (double)((long long)wall_clock64() - t0) * sp.us_per_tick;
    sol->stats.solve_us = us_;
    if (ps.order_key) { const int ko = ps.order_key[slot] - sp.qp_key_decay; ps.order_key[slot] = (sp.qp_key_decay > 0 && ko > 0) ? ko : 0; }      // (a slot solved here costs the interior-point launch nothing: its key decays to the back of the order)
    presolved[slot] = 1;
  }
  return true;
}

}  // namespace nep
