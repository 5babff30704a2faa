// plan_common.h — the arithmetic of the committed plan (include/neptune_plan.h: nep_plan_select_a, nep_plan_splice,
// nep_pwp_compose_exact), shared by its host form (plan_host.cpp) and its device form (fleet_kernels.hip, include/neptune_fleet.h).
// Both are built -ffp-contract=off and every number is computed by the expressions below in both, so a fleet flown on the device
// holds the plans and the trajectories the host chain would hold, bit for bit.  No library call but ceil and sqrt (correctly
// rounded in both forms); copies are plain loops.
#ifndef NEP_PLAN_COMMON_H_
#define NEP_PLAN_COMMON_H_

#include <math.h>

#include "../../include/neptune_plan.h"

#ifndef NEP_PLAN_FN
#define NEP_PLAN_FN static inline
#endif

namespace nep_plan_impl {

// ---- nep_pwp_compose_exact ---------------------------------------------------------------------------------------------------
NEP_PLAN_FN void pwp_clear(nep_pwp* p) {
  p->n_seg = 0; p->_pad = 0;
  for (int i = 0; i <= NEP_TRAJ_MAX_SEG; i++) p->times[i] = 0.0;
  for (int ax = 0; ax < 3; ax++)
    for (int i = 0; i < NEP_TRAJ_MAX_SEG; i++)
      for (int c = 0; c < 4; c++) p->coeff[ax][i][c] = 0.0;
}

NEP_PLAN_FN void rebase(const double c[4], double s, double o[4]) {      // q(w) = p(w + s)
  o[0] = c[0];
  o[1] = 3 * c[0] * s + c[1];
  o[2] = (3 * c[0] * s + 2 * c[1]) * s + c[2];
  o[3] = ((c[0] * s + c[1]) * s + c[2]) * s + c[3];
}

// p restricted to [t0, t1] appended to res (t0 < t1); beyond p's last knot the end point is held
NEP_PLAN_FN bool append_span(nep_pwp* res, const nep_pwp* p, double t0, double t1) {
  const int n = p->n_seg;
  double a = t0;
  while (a < t1) {
    int k = 0;
    while (k < n && p->times[k + 1] <= a) k++;
    if (res->n_seg >= NEP_TRAJ_MAX_SEG) return false;
    const int o = res->n_seg++;
    double b;
    if (k >= n) {                                   // past the end: hold the final point
      b = t1;
      const double T = p->times[n] - p->times[n - 1];
      for (int ax = 0; ax < 3; ax++) {
        double e[4]; rebase(p->coeff[ax][n - 1], T, e);
        res->coeff[ax][o][0] = res->coeff[ax][o][1] = res->coeff[ax][o][2] = 0.0; res->coeff[ax][o][3] = e[3];
      }
    } else {
      b = p->times[k + 1] < t1 ? p->times[k + 1] : t1;
      const double s = a - p->times[k] > 0 ? a - p->times[k] : 0.0;    // (a before p's first knot: p's start is extended backwards)
      for (int ax = 0; ax < 3; ax++) rebase(p->coeff[ax][k], a - p->times[k] < 0 ? a - p->times[k] : s, res->coeff[ax][o]);
    }
    res->times[o + 1] = b;
    a = b;
  }
  return true;
}

// The body of nep_pwp_compose_exact on checked arguments (1 <= n_seg <= NEP_TRAJ_MAX_SEG in both): res is cleared and filled.
// False: more than NEP_TRAJ_MAX_SEG intervals (res is then unfinished and the caller drops it).
NEP_PLAN_FN bool compose_exact(double t, const nep_pwp* p1, const nep_pwp* p2, nep_pwp* res) {
  pwp_clear(res);
  const double t2 = p2->times[0];
  res->times[0] = t;
  if (t < t2) {                                       // the old trajectory until the new one takes over
    if (!append_span(res, p1, t, t2)) return false;
    for (int i = 0; i < p2->n_seg; i++) {
      if (res->n_seg >= NEP_TRAJ_MAX_SEG) return false;
      const int o = res->n_seg++;
      res->times[o + 1] = p2->times[i + 1];
      for (int ax = 0; ax < 3; ax++)
        for (int c = 0; c < 4; c++) res->coeff[ax][o][c] = p2->coeff[ax][i][c];
    }
    return true;
  }
  // the new trajectory has already started: its part from t on
  return append_span(res, p2, t, p2->times[p2->n_seg] > t ? p2->times[p2->n_seg] : t + 1.0);
}

// ---- point A (neptune.cpp:1366-1399) -------------------------------------------------------------------------------------------
// mu::saturate(int&, const int, const int): the call sites pass doubles, which C++ truncates
// to int because deltaT_ is an int lvalue (utils.cpp:744-754, neptune.cpp:1374).
NEP_PLAN_FN int saturate_int(int v, double lo, double hi) {
  const int ilo = (int)lo, ihi = (int)hi;
  return v < ilo ? ilo : (v > ihi ? ihi : v);
}
NEP_PLAN_FN double saturate_dbl(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct SelectA { int delta_t, future_index, k_index, k_index_end; };

// which state of a plan of `size` states is A; delta_t comes back saturated (the caller keeps it: deltaT_ is a member)
NEP_PLAN_FN SelectA select_a_index(const nep_plan_cfg* c, int size, int delta_t) {
  SelectA s;
  s.delta_t = saturate_int(delta_t, c->lower_bound_runtime / c->dc, c->upper_bound_runtime / c->dc);
  s.future_index = size - s.delta_t;
  s.k_index_end = s.future_index > 0 ? s.future_index : 0;
  if ((double)size < ceil(c->T_span / c->dc)) s.k_index_end = 0;
  s.k_index = size - 1 - s.k_index_end;
  return s;
}

// A as planned -> A as handed to the search: at rest when the plan is shorter than deltaT, and at the measured position when the
// head of the plan is more than 1 m away from it (:1386-1398)
NEP_PLAN_FN void select_a_fix(double A[12], int future_index, const double* head, const double* state_pos) {
  if (future_index < 0)
    for (int i = 3; i < 9; ++i) A[i] = 0.0;
  const double dx = head[0] - state_pos[0], dy = head[1] - state_pos[1], dz = head[2] - state_pos[2];
  if (sqrt(dx * dx + dy * dy + dz * dz) > 1.0)
    for (int i = 0; i < 3; ++i) A[i] = state_pos[i];
}

NEP_PLAN_FN double select_a_runtime(const nep_plan_cfg* c, const SelectA& s) {      // (:1406-1419)
  const double rs = (s.k_index_end != 0) ? s.k_index * c->dc - c->runtime_opt : c->upper_bound_runtime;
  return saturate_dbl(rs, c->lower_bound_runtime - c->runtime_opt, c->upper_bound_runtime - c->runtime_opt);
}

// ---- splice (neptune.cpp:1661-1687) --------------------------------------------------------------------------------------------
// states a plan of `size` keeps when A and the k_index_end states after it are erased; negative: "Already published the point A"
NEP_PLAN_FN int splice_keep(int size, int k_index_end) { return size - 1 - k_index_end; }

}  // namespace nep_plan_impl
#endif  // NEP_PLAN_COMMON_H_
