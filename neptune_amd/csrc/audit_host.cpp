// audit_host.cpp — host form of the flight audit (include/neptune_frontend.h: nep_audit_records).  No HIP call; built like
// plan_host.cpp (-O2 -ffp-contract=off).  A serial walk by tick, agent, partner; the arithmetic is audit_common.h's, which the
// device form (audit_kernels.hip) shares, and the device equals this bit for bit.
#include <cmath>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "audit_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_audit_impl;

extern "C" {

int nep_audit_init(nep_audit* out, int64_t n) {
  if (n < 0 || (n > 0 && !out)) { nep::set_last_error("bad arguments"); return NEP_E_ARG; }
  const double inf = std::numeric_limits<double>::infinity();
  for (int64_t i = 0; i < n; i++) {
    nep_audit a{};
    a.min_center_dist = a.min_box_clear = a.min_static_dist = a.center_d2 = inf;
    a.center_partner = a.box_partner = a.static_index = -1;
    out[i] = a;
  }
  return 0;
}

int nep_audit_records(const nep_traj_rec* recs, int32_t n, const int32_t* static_off, const double* static_xy, int32_t n_static,
                      double drone_radius, double t0, double tick, int32_t n_ticks, nep_audit* out) {
  if (n < 0 || n_static < 0 || n_ticks < 0 || (n > 0 && (!recs || !out)) || (n_static > 0 && (!static_off || !static_xy)) || !(tick >= 0.0)) {
    nep::set_last_error("bad arguments"); return NEP_E_ARG;
  }
  if (n == 0 || n_ticks == 0) return 0;
  // the polygons as the handle holds them: counter-clockwise with the first vertex kept first (normalize_ccw, backend.hip), and one
  // reciprocal squared length per edge
  std::vector<int> off(n_static + 1, 0);
  std::vector<double> xy, inv;
  for (int j = 0; j < n_static; j++) {
    const int c = static_off[j + 1] - static_off[j];
    if (c < 0) { nep::set_last_error("static obstacle offsets must not decrease"); return NEP_E_ARG; }
    if (c > NEP_HULL_MAX_V) { nep::set_last_error("static obstacle with more than NEP_HULL_MAX_V vertices"); return NEP_E_CAP; }
    std::vector<double> q(static_xy + 2 * (size_t)static_off[j], static_xy + 2 * (size_t)(static_off[j] + c));
    if (c >= 3) {
      double area2 = 0;
      for (int v = 0; v < c; v++) { const double* a = &q[2 * v]; const double* b = &q[2 * ((v + 1) % c)]; area2 += a[0] * b[1] - a[1] * b[0]; }
      if (area2 < 0) for (int lo = 1, hi = c - 1; lo < hi; lo++, hi--) { std::swap(q[2 * lo], q[2 * hi]); std::swap(q[2 * lo + 1], q[2 * hi + 1]); }
    }
    xy.insert(xy.end(), q.begin(), q.end());
    for (int v = 0; v < c; v++) { const int w = v + 1 == c ? 0 : v + 1; inv.push_back(audit_edge_inv(q[2 * v], q[2 * v + 1], q[2 * w], q[2 * w + 1])); }
    off[j + 1] = off[j] + c;
  }
  std::vector<unsigned char> pres(n);
  std::vector<double> hx(n), hy(n);
  for (int a = 0; a < n; a++) {
    pres[a] = audit_present(recs + a);
    hx[a] = recs[a].bbox[0] / 2 + drone_radius; hy[a] = recs[a].bbox[1] / 2 + drone_radius;
  }
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<AuditState> st(n);
  for (int k = 0; k < n_ticks; k++) {
    const double t = t0 + (double)k * tick;
    for (int a = 0; a < n; a++) if (pres[a]) st[a] = audit_eval(recs + a, t);
    for (int a = 0; a < n; a++) {
      if (!pres[a]) continue;
      nep_audit& A = out[a];
      const double px = st[a].x, py = st[a].y;
      double tb = inf; int tbp = -1;
      for (int j = 0; j < n; j++) {
        if (j == a || !pres[j]) continue;
        const double dx = px - st[j].x, dy = py - st[j].y;
        const double d2 = dx * dx + dy * dy;
        if (d2 < A.center_d2) { A.center_d2 = d2; A.center_partner = j + 1; A.t_center = t; }
        const double bc = audit_box_clear(dx, dy, hx[j], hy[j]);
        if (bc < tb) { tb = bc; tbp = j + 1; }
      }
      if (tb < A.min_box_clear) { A.min_box_clear = tb; A.box_partner = tbp; A.t_box = t; }
      if (tb < 0.0) A.n_pair_viol++;
      double ts = inf; int tsi = -1;
      for (int j = 0; j < n_static; j++) {
        const int c = off[j + 1] - off[j];
        if (c < 1) continue;
        const double* q = &xy[2 * (size_t)off[j]];
        double d2 = inf; bool inside = true;
        for (int v = 0; v < c; v++) { const int w = v + 1 == c ? 0 : v + 1; audit_edge(px, py, q[2 * v], q[2 * v + 1], q[2 * w], q[2 * w + 1], inv[off[j] + v], d2, inside); }
        const double sd = audit_signed(d2, inside, c);
        if (sd < ts) { ts = sd; tsi = j; }
      }
      if (ts < A.min_static_dist) { A.min_static_dist = ts; A.static_index = tsi; A.t_static = t; }
      if (ts < 0.0) A.n_static_viol++;
    }
  }
  for (int a = 0; a < n; a++) {
    if (!pres[a]) continue;
    out[a].min_center_dist = std::sqrt(out[a].center_d2);
    audit_path(recs + a, t0, tick, n_ticks, out + a);
  }
  return 0;
}

}  // extern "C"
