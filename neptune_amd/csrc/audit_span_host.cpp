// audit_span_host.cpp — host form of the span audit (include/neptune_frontend.h: nep_span_audit_records).  No HIP call; built like
// audit_host.cpp (-O2 -ffp-contract=off).  A serial walk by agent, then partner, then polygon; the rule is audit_span_common.h's,
// which the device form (audit_span_kernels.hip) shares, and the device equals this byte for byte.
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "audit_span_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_span_impl;

extern "C" {

int nep_span_audit_init(nep_span_audit* out, int64_t n) {
  if (n < 0 || (n > 0 && !out)) { nep::set_last_error("bad arguments"); return NEP_E_ARG; }
  const double inf = std::numeric_limits<double>::infinity();
  for (int64_t i = 0; i < n; i++) {
    nep_span_audit a{};
    a.min_center_dist = a.min_box_clear = a.min_static_dist = a.center_d2 = inf;
    a.center_partner = a.box_partner = a.static_index = -1;
    out[i] = a;
  }
  return 0;
}

int nep_span_audit_records(const nep_traj_rec* recs, int32_t n, const int32_t* static_off, const double* static_xy, int32_t n_static,
                           double drone_radius, double t0, double tick, int32_t n_ticks, nep_span_audit* out) {
  if (n < 0 || n_static < 0 || n_ticks < 0 || (n > 0 && (!recs || !out)) || (n_static > 0 && (!static_off || !static_xy)) ||
      !(tick >= 0.0 && tick < std::numeric_limits<double>::infinity())) {      // (an infinite tick would put tick 0 at t0 + 0 * inf)
    nep::set_last_error("bad arguments"); return NEP_E_ARG;
  }
  // the polygons as the handle holds them (audit_host.cpp): counter-clockwise with the first vertex kept first, one reciprocal
  // squared length per edge.  Checked before the n_ticks == 0 return, so that a bad scene is refused by every call
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
  if (n == 0 || n_ticks == 0) return 0;
  const SpanWin w = span_win(t0, tick, n_ticks);
  std::vector<unsigned char> pres(n);
  std::vector<double> box(4 * (size_t)n);
  for (int a = 0; a < n; a++) {
    pres[a] = audit_present(recs + a);
    double ts[kSpanLdsPieces]; SpanPiece pc[kSpanLdsPieces];
    if (pres[a]) span_stage(recs + a, w.t0, w.t1, ts, pc, &box[4 * (size_t)a]);
  }
  for (int a = 0; a < n; a++) {
    if (!pres[a]) continue;
    SpanCall c;
    span_call_init(c);
    const SpanSrc A{recs + a, nullptr, nullptr, -1};
    // every partner and polygon at the ticks first; then, with the minima those gave, the whole window of whoever the bound does not rule out
    for (int pass = 0; pass < 2; pass++) {
      const SpanCall u = c;
      for (int j = 0; j < n; j++) {
        if (j == a || !pres[j]) continue;
        const double hx = recs[j].bbox[0] / 2 + drone_radius, hy = recs[j].bbox[1] / 2 + drone_radius;
        SpanPairWalk W{recs + a, recs + j, A, SpanSrc{recs + j, nullptr, nullptr, -1}, j + 1, hx, hy, &c};
        if (pass == 0) span_ticks(w, W);
        else if (!span_skip_pair(&box[4 * (size_t)a], &box[4 * (size_t)j], hx, hy, u.center.v, u.box.v)) span_intervals(w, W);
      }
      for (int j = 0; j < n_static; j++) {
        const int nv = off[j + 1] - off[j];
        if (nv < 1) continue;
        SpanPolyWalk W{recs + a, A, &xy[2 * (size_t)off[j]], &inv[off[j]], nv, j, &c};
        if (pass == 0) span_ticks(w, W);
        else if (!span_skip_poly(&box[4 * (size_t)a], &xy[2 * (size_t)off[j]], nv, u.stat.v)) span_intervals(w, W);
      }
    }
    span_fold(c, w, out + a);
  }
  return 0;
}

}  // extern "C"
