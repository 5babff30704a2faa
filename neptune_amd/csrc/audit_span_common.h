// audit_span_common.h — the rule of the span audit (include/neptune_frontend.h: nep_span_audit), shared by its
// host form (audit_span_host.cpp) and its device form (audit_span_kernels.hip).  Both are built -ffp-contract=off and use + - * /
// and sqrt only, so every candidate time and every value is the same double in both.
//
// The window [t0, t0 + n_ticks * tick] is cut at its ends, at the call's ticks and at every knot of the records involved; on an
// elementary interval [a, b] every curve is one cubic (or at rest), re-based to s = t - a.  The minima of the three audited
// quantities over the interval lie at its ends or at roots of polynomials of degree <= 5 in s (SpanPairWalk, SpanPolyWalk list them).
// The re-based polynomials only FIND candidate times: every value is taken by the tick audit's own expressions (audit_eval,
// audit_box_clear, audit_edge, audit_signed) at the candidate time, so a tick is a candidate evaluated as the tick audit
// evaluates it.  A minimum is the least (value, time, partner or polygon index) in that order — what "strictly smaller wins" gives
// a serial walk by time and then by partner, and what any parallel walk gives too.
#ifndef NEP_AUDIT_SPAN_COMMON_H_
#define NEP_AUDIT_SPAN_COMMON_H_

#include "audit_common.h"

#ifndef NEP_SPAN_MFN
#define NEP_SPAN_MFN inline      // (member functions: NEP_AUDIT_FN's `static` would mean something else)
#endif

namespace nep_span_impl {

using namespace nep_audit_impl;

constexpr int kSpanLdsPieces = 2;      // pieces of a record the device form stages per agent; a record with more in one window is read from global memory

// ---- pieces of a record ---------------------------------------------------------------------------------------------------------
// The cubic a record follows from time t to its next knot, as audit_eval chooses it: the segment's own coefficients c (highest
// power first) in u = t - org, or at rest (c[0..2] = 0) before the first knot and beyond the last.  next: the smallest knot > t
// (+inf when there is none): nothing about the record's regime changes before it.
struct SpanPiece { double org, c[2][4]; };

NEP_AUDIT_FN void span_piece(const nep_traj_rec* r, double t, SpanPiece& P, double& next) {
  const int n = r->pwp.n_seg < NEP_TRAJ_MAX_SEG ? r->pwp.n_seg : NEP_TRAJ_MAX_SEG;
  int i = 0;
  for (int k = 1; k < n; k++) if (t >= r->pwp.times[k]) i = k;
  const bool past = t >= r->pwp.times[n];
  const bool before = !past && (t - r->pwp.times[i] < 0.0);
  next = __builtin_huge_val();
  for (int k = 0; k <= n; k++) { const double tk = r->pwp.times[k]; if (tk > t && tk < next) next = tk; }
  const double u = r->pwp.times[n] - r->pwp.times[n - 1];
  for (int ax = 0; ax < 2; ax++) {
    const double* c = r->pwp.coeff[ax][i];
    if (past) { P.c[ax][0] = P.c[ax][1] = P.c[ax][2] = 0.0; P.c[ax][3] = ((c[0] * (u * u * u) + c[1] * (u * u)) + c[2] * u) + c[3]; }
    else if (before) { P.c[ax][0] = P.c[ax][1] = P.c[ax][2] = 0.0; P.c[ax][3] = c[3]; }
    else { P.c[ax][0] = c[0]; P.c[ax][1] = c[1]; P.c[ax][2] = c[2]; P.c[ax][3] = c[3]; }
  }
  P.org = (past || before) ? t : r->pwp.times[i];
}

// Where a record's pieces come from: the record itself (n < 0), or a staged list of n pieces starting at ts[0] < ts[1] < ... (the
// device form's LDS copy, made by span_stage with span_piece at every ts[i]) — the same piece either way.
struct SpanSrc { const nep_traj_rec* r; const double* ts; const SpanPiece* pc; int n; };

NEP_AUDIT_FN void span_fetch(const SpanSrc& S, double a, SpanPiece& P, double& next) {
  if (S.n < 0) { span_piece(S.r, a, P, next); return; }
  int i = 0;
  for (int k = 1; k < S.n; k++) if (a >= S.ts[k]) i = k;
  P = S.pc[i];
  next = i + 1 < S.n ? S.ts[i + 1] : __builtin_huge_val();
}

// the piece as a polynomial in s = t - a, lowest power first
NEP_AUDIT_FN void span_rebase(const SpanPiece& P, double a, double q[2][4]) {
  const double u = a - P.org;
  for (int ax = 0; ax < 2; ax++) {
    const double* c = P.c[ax];
    q[ax][3] = c[0];
    q[ax][2] = (3.0 * c[0]) * u + c[1];
    q[ax][1] = ((3.0 * c[0]) * (u * u) + (2.0 * c[1]) * u) + c[2];
    q[ax][0] = ((c[0] * (u * u * u) + c[1] * (u * u)) + c[2] * u) + c[3];
  }
}

// A box that holds the record's x-y position at every time of [t0, t1]: the Bezier control points of every piece (a cubic lies in
// their hull), widened by 1e-9 of their size (and 1e-9 m) — seven orders above the roundings that separate the re-based piece
// from what audit_eval computes.  box: xlo, xhi, ylo, yhi.  A coordinate that is no number leaves a box no test can pass.
NEP_AUDIT_FN void span_box_piece(const SpanPiece& P, double a, double b, double* box) {
  double q[2][4];
  span_rebase(P, a, q);
  const double L = b - a;
  for (int ax = 0; ax < 2; ax++) {
    const double b0 = q[ax][0], b1 = b0 + q[ax][1] * L / 3.0, b2 = b1 + (q[ax][1] * L + q[ax][2] * (L * L)) / 3.0;
    const double b3 = ((q[ax][3] * (L * L * L) + q[ax][2] * (L * L)) + q[ax][1] * L) + q[ax][0];
    double lo = b0, hi = b0;
    if (!(b1 >= lo)) lo = b1; if (!(b1 <= hi)) hi = b1;
    if (!(b2 >= lo)) lo = b2; if (!(b2 <= hi)) hi = b2;
    if (!(b3 >= lo)) lo = b3; if (!(b3 <= hi)) hi = b3;
    const double pad = 1e-9 * (1.0 + (fabs(lo) > fabs(hi) ? fabs(lo) : fabs(hi)));
    lo = lo - pad; hi = hi + pad;
    if (!(lo >= box[2 * ax])) box[2 * ax] = lo;
    if (!(hi <= box[2 * ax + 1])) box[2 * ax + 1] = hi;
  }
}

// the pieces of r that begin in [t0, t1): the first kSpanLdsPieces into ts / pc; -> their count, or -1 when there are more.
// box [4]: the record's box over the window (every piece, staged or not).
NEP_AUDIT_FN int span_stage(const nep_traj_rec* r, double t0, double t1, double* ts, SpanPiece* pc, double* box) {
  double cur = t0;
  int n = 0;
  box[0] = box[2] = __builtin_huge_val(); box[1] = box[3] = -__builtin_huge_val();
  for (int it = 0; it < NEP_TRAJ_MAX_SEG + 2; it++) {
    SpanPiece P;
    double next;
    span_piece(r, cur, P, next);
    if (n >= 0 && n < kSpanLdsPieces) { pc[n] = P; ts[n] = cur; n++; } else n = -1;
    const bool last = !(next < t1);
    span_box_piece(P, cur, last ? t1 : next, box);
    if (last) break;
    cur = next;
  }
  return n;
}

// Pruning: what a partner j (box bj, inflated half-widths hx, hy) can come to against the agent (box ba) anywhere in the window is
// at least: |dx| >= gx, |dy| >= gy, the gaps between the boxes.  So its centre distance squared is >= gx^2 + gy^2 and its box
// clearance >= max(gx - hx, gy - hy).  When both lie strictly above values the agent has already attained (u_c2, u_box: its minima
// over the call's ticks, which every partner goes through first), no candidate of j can win or tie either minimum, and j is skipped.
NEP_AUDIT_FN double span_gap(double alo, double ahi, double blo, double bhi) {
  const double g = alo - bhi > blo - ahi ? alo - bhi : blo - ahi;
  return g > 0.0 ? g : 0.0;
}
NEP_AUDIT_FN bool span_skip_pair(const double* ba, const double* bj, double hx, double hy, double u_c2, double u_box) {
  const double gx = span_gap(ba[0], ba[1], bj[0], bj[1]), gy = span_gap(ba[2], ba[3], bj[2], bj[3]);
  const double lb = gx - hx > gy - hy ? gx - hx : gy - hy;
  return (gx * gx + gy * gy) * (1.0 - 1e-9) > u_c2 && lb > u_box;
}
// Likewise a polygon whose vertices' box the agent's box stays clear of: outside it the signed distance is the distance, at least
// the gap between the boxes.  (Boxes that overlap bound nothing: the agent may be inside.)
NEP_AUDIT_FN bool span_skip_poly(const double* ba, const double* xy, int nv, double u_stat) {
  double lo[2] = {__builtin_huge_val(), __builtin_huge_val()}, hi[2] = {-__builtin_huge_val(), -__builtin_huge_val()};
  for (int v = 0; v < nv; v++) for (int ax = 0; ax < 2; ax++) { const double c = xy[2 * v + ax]; if (!(c >= lo[ax])) lo[ax] = c; if (!(c <= hi[ax])) hi[ax] = c; }
  const double gx = span_gap(ba[0], ba[1], lo[0], hi[0]), gy = span_gap(ba[2], ba[3], lo[1], hi[1]);
  if (!(gx > 0.0 || gy > 0.0)) return false;
  return sqrt(gx * gx + gy * gy) * (1.0 - 1e-9) > u_stat;
}

// ---- roots ----------------------------------------------------------------------------------------------------------------------
// the j-th derivative of p (lowest power first, degree deg) at s
NEP_AUDIT_FN double span_deriv(const double* p, int deg, int j, double s) {
  double v = 0.0;
  for (int i = deg; i >= j; i--) {
    double f = 1.0;
    for (int m = 0; m < j; m++) f = f * (double)(i - m);
    v = v * s + p[i] * f;
  }
  return v;
}

// The real roots of p in (0, L) at which p changes sign, degree <= 5, each as the two adjacent doubles lo <= hi the sign changes
// between (lo == hi where p is exactly 0): emit(lo), emit(hi).  The brackets of a level are cut at the roots of its derivative —
// found the same way, down to the quadratic, which is solved in closed form — so p is monotone on each and a sign change at a
// bracket's ends is one root, found by bisection.  A polynomial that is identically zero, or constant, has none.
template <class Emit> NEP_AUDIT_FN void span_roots(const double* p, int deg, double L, Emit&& emit) {
  while (deg >= 1 && p[deg] == 0.0) deg--;
  if (deg < 1 || !(L > 0.0)) return;
  double br[5], nr[5];
  int nb = 0, lvl;
  if (deg >= 3) {      // the quadratic at the bottom of the chain: p^(deg-2)
    const int j = deg - 2;
    const double c0 = span_deriv(p, deg, j, 0.0), c1 = span_deriv(p, deg, j + 1, 0.0), c2 = span_deriv(p, deg, j + 2, 0.0) / 2.0;
    const double disc = c1 * c1 - 4.0 * c2 * c0;
    if (disc > 0.0) {
      const double sq = sqrt(disc);
      double r0 = (-c1 - sq) / (2.0 * c2), r1 = (-c1 + sq) / (2.0 * c2);
      if (r1 < r0) { const double t = r0; r0 = r1; r1 = t; }
      if (r0 > 0.0 && r0 < L) br[nb++] = r0;
      if (r1 > 0.0 && r1 < L && r1 > r0) br[nb++] = r1;
    }
    lvl = j - 1;
  } else if (deg == 2) {
    const double r = -p[1] / (2.0 * p[2]);
    if (r > 0.0 && r < L) br[nb++] = r;
    lvl = 0;
  } else {
    lvl = 0;
  }
  for (; lvl >= 0; lvl--) {
    int cnt = 0;
    double left = 0.0, fl = span_deriv(p, deg, lvl, 0.0);
    for (int i = 0; i <= nb; i++) {
      const double right = i < nb ? br[i] : L;
      const double fr = span_deriv(p, deg, lvl, right);
      if ((fl < 0.0 && fr > 0.0) || (fl > 0.0 && fr < 0.0)) {
        const bool neg = fl < 0.0;
        double lo = left, hi = right;
        for (;;) {
          const double m = lo + (hi - lo) * 0.5;
          if (!(m > lo && m < hi)) break;
          const double fm = span_deriv(p, deg, lvl, m);
          if (fm == 0.0) { lo = hi = m; break; }
          if ((fm < 0.0) == neg) lo = m; else hi = m;
        }
        if (lvl == 0) { emit(lo); if (hi > lo) emit(hi); }
        else if (cnt < 5) nr[cnt++] = hi;
      } else if (fr == 0.0 && i < nb) {      // a bracket end that is itself a root
        if (lvl == 0) emit(right);
        else if (cnt < 5) nr[cnt++] = right;
      }
      left = right; fl = fr;
    }
    nb = 0;
    for (int i = 0; i < cnt; i++) if (nb == 0 || nr[i] > br[nb - 1]) br[nb++] = nr[i];
  }
}

// d/ds (x^2 + y^2) / 2 of the cubics x, y (lowest power first): a quintic
NEP_AUDIT_FN void span_dist_deriv(const double* x, const double* y, double* g) {
  for (int k = 0; k < 6; k++) g[k] = 0.0;
  for (int i = 0; i < 4; i++)
    for (int j = 1; j < 4; j++) g[i + j - 1] = g[i + j - 1] + (x[i] * ((double)j * x[j]) + y[i] * ((double)j * y[j]));
}

// ---- the window and the minima ---------------------------------------------------------------------------------------------------
struct SpanWin { double t0, tick, t1; int n_ticks; };
NEP_AUDIT_FN SpanWin span_win(double t0, double tick, int n_ticks) {
  SpanWin w; w.t0 = t0; w.tick = tick; w.n_ticks = n_ticks; w.t1 = t0 + (double)n_ticks * tick;
  return w;
}

struct SpanMin { double v, t; int who; };
NEP_AUDIT_FN void span_min_init(SpanMin& m) { m.v = __builtin_huge_val(); m.t = __builtin_huge_val(); m.who = 0x7fffffff; }
// the least (value, time, partner or index)
NEP_AUDIT_FN void span_take(SpanMin& m, double v, double t, int who) {
  if (v < m.v || (v == m.v && (t < m.t || (t == m.t && who < m.who)))) { m.v = v; m.t = t; m.who = who; }
}

// what one call finds for one agent: the three minima over the window, and the box and static minima over the call's ticks alone
struct SpanCall { SpanMin center, box, stat; double tick_box, tick_stat; };
NEP_AUDIT_FN void span_call_init(SpanCall& c) {
  span_min_init(c.center); span_min_init(c.box); span_min_init(c.stat);
  c.tick_box = __builtin_huge_val(); c.tick_stat = __builtin_huge_val();
}
NEP_AUDIT_FN void span_call_merge(SpanCall& c, const SpanCall& o) {
  span_take(c.center, o.center.v, o.center.t, o.center.who);
  span_take(c.box, o.box.v, o.box.t, o.box.who);
  span_take(c.stat, o.stat.v, o.stat.t, o.stat.who);
  if (o.tick_box < c.tick_box) c.tick_box = o.tick_box;
  if (o.tick_stat < c.tick_stat) c.tick_stat = o.tick_stat;
}

// The elementary intervals of the window for the sources A (and B, when given): f(a, b, a_is_tick) for every interval a < b in
// time order, then f(t1, t1, false) for the window's end (the only call of a window of length 0, whose one instant is tick 0).
template <class F> NEP_AUDIT_FN void span_intervals(const SpanWin& w, F&& f) {
  // the bound: every interval ends at a tick, a knot or the window's end (and a malformed clock must not loop for ever)
  int kn = 0;      // the first tick index whose time is > a
  double a = w.t0;
  bool a_tick = w.n_ticks > 0;
  const int most = w.n_ticks + 2 * (NEP_TRAJ_MAX_SEG + 1) + 2;
  for (int it = 0; it < most; it++) {
    while (kn <= w.n_ticks && !(w.t0 + (double)kn * w.tick > a)) kn++;
    double b = w.t1;
    const double tn = kn <= w.n_ticks ? w.t0 + (double)kn * w.tick : w.t1;
    if (tn < b) b = tn;
    const double kb = f.next_knot(a);
    if (kb < b) b = kb;
    if (!(b > a)) break;
    f(a, b, a_tick);
    a_tick = kn < w.n_ticks && b == tn;
    a = b;
  }
  f(a, a, a_tick && !(a > w.t0) && w.n_ticks > 0);
}

// the call's ticks and the window's end alone, for a walk W: what the tick audit looks at (and the one instant it does not)
template <class W> NEP_AUDIT_FN void span_ticks(const SpanWin& w, W&& walk) {
  for (int k = 0; k < w.n_ticks; k++) walk.at(w.t0 + (double)k * w.tick, true);
  walk.at(w.t1, false);
}

// ---- agent against partner ---------------------------------------------------------------------------------------------------------
// The candidates of agent (ra, A) against partner (rb, B; 1-based id pid, inflated half-widths hx, hy) over the window, folded
// into c: at every candidate time both centre distance (squared) and box clearance are taken.
struct SpanPairWalk {
  const nep_traj_rec* ra; const nep_traj_rec* rb; SpanSrc A, B; int pid; double hx, hy; SpanCall* c;
  SpanPiece pa, pb; double na, nb;
  NEP_SPAN_MFN double next_knot(double a) { span_fetch(A, a, pa, na); span_fetch(B, a, pb, nb); return na < nb ? na : nb; }
  NEP_SPAN_MFN void at(double t, bool is_tick) {
    const AuditState sa = audit_eval(ra, t), sb = audit_eval(rb, t);
    const double dx = sa.x - sb.x, dy = sa.y - sb.y;
    const double d2 = dx * dx + dy * dy;
    const double bc = audit_box_clear(dx, dy, hx, hy);
    span_take(c->center, d2, t, pid);
    span_take(c->box, bc, t, pid);
    if (is_tick && bc < c->tick_box) c->tick_box = bc;
  }
  NEP_SPAN_MFN void operator()(double a, double b, bool a_tick) {
    at(a, a_tick);
    if (!(b > a)) return;
    double qa[2][4], qb[2][4], d[2][4], g[6], e[4];
    span_rebase(pa, a, qa); span_rebase(pb, a, qb);
    for (int ax = 0; ax < 2; ax++) for (int k = 0; k < 4; k++) d[ax][k] = qa[ax][k] - qb[ax][k];
    const double L = b - a;
    auto emit = [&](double s) { at(a + s, false); };
    span_dist_deriv(d[0], d[1], g);
    span_roots(g, 5, L, emit);                                  // centre distance: d/ds (dx^2 + dy^2)
    for (int ax = 0; ax < 2; ax++) {
      span_roots(d[ax], 3, L, emit);                            // box: dx, dy (where |.| turns)
      e[0] = d[ax][1]; e[1] = 2.0 * d[ax][2]; e[2] = 3.0 * d[ax][3];
      span_roots(e, 2, L, emit);                                // dx', dy'
    }
    const double h = hx - hy;                                   // |dx| - hx == |dy| - hy: dx -+ dy == +-h, where the max switches sides
    for (int sg = 0; sg < 2; sg++) {
      for (int k = 0; k < 4; k++) e[k] = sg ? d[0][k] + d[1][k] : d[0][k] - d[1][k];
      const double e0 = e[0];
      e[0] = e0 - h; span_roots(e, 3, L, emit);
      e[0] = e0 + h; span_roots(e, 3, L, emit);
    }
  }
};

// ---- agent against polygon ---------------------------------------------------------------------------------------------------------
// The candidates of agent (ra, A) against polygon `index` (xy [nv][2] counter-clockwise, inv [nv] = audit_edge_inv per edge)
struct SpanPolyWalk {
  const nep_traj_rec* ra; SpanSrc A; const double* xy; const double* inv; int nv, index; SpanCall* c;
  SpanPiece pa; double na;
  NEP_SPAN_MFN double next_knot(double a) { span_fetch(A, a, pa, na); return na; }
  NEP_SPAN_MFN void at(double t, bool is_tick) {
    const AuditState s = audit_eval(ra, t);
    double d2 = __builtin_huge_val(); bool inside = true;
    for (int v = 0; v < nv; v++) { const int w = v + 1 == nv ? 0 : v + 1; audit_edge(s.x, s.y, xy[2 * v], xy[2 * v + 1], xy[2 * w], xy[2 * w + 1], inv[v], d2, inside); }
    const double sd = audit_signed(d2, inside, nv);
    span_take(c->stat, sd, t, index);
    if (is_tick && sd < c->tick_stat) c->tick_stat = sd;
  }
  // the line function e x (p - v) of edge v -> w over the interval's cubic q; ee = |e|^2; -> false for a repeated vertex
  NEP_SPAN_MFN bool line(const double q[2][4], int v, double* l, double& ex, double& ey, double& ee) const {
    const int w = v + 1 == nv ? 0 : v + 1;
    ex = xy[2 * w] - xy[2 * v]; ey = xy[2 * w + 1] - xy[2 * v + 1]; ee = ex * ex + ey * ey;
    if (!(ee > 0.0)) return false;
    l[0] = ex * (q[1][0] - xy[2 * v + 1]) - ey * (q[0][0] - xy[2 * v]);
    for (int k = 1; k < 4; k++) l[k] = ex * q[1][k] - ey * q[0][k];
    return true;
  }
  NEP_SPAN_MFN void operator()(double a, double b, bool a_tick) {
    at(a, a_tick);
    if (!(b > a)) return;
    double q[2][4], l[4], m[4], e[4], w[2][4], g[6];
    span_rebase(pa, a, q);
    const double L = b - a;
    auto emit = [&](double s) { at(a + s, false); };
    for (int v = 0; v < nv; v++) {
      for (int k = 0; k < 4; k++) { w[0][k] = q[0][k]; w[1][k] = q[1][k]; }
      w[0][0] = q[0][0] - xy[2 * v]; w[1][0] = q[1][0] - xy[2 * v + 1];
      span_dist_deriv(w[0], w[1], g);
      span_roots(g, 5, L, emit);                                // vertex: d/ds |p - v|^2
      double ex, ey, ee;
      if (!line(q, v, l, ex, ey, ee)) continue;
      span_roots(l, 3, L, emit);                                // edge: the line function's zeros
      e[0] = l[1]; e[1] = 2.0 * l[2]; e[2] = 3.0 * l[3];
      span_roots(e, 2, L, emit);                                // and its derivative
      for (int k = 0; k < 4; k++) e[k] = ex * w[0][k] + ey * w[1][k];
      span_roots(e, 3, L, emit);                                // projection boundaries e.(p - v) = 0, = |e|^2
      e[0] = e[0] - ee;
      span_roots(e, 3, L, emit);
      const double lv = sqrt(ee);
      for (int u = v + 1; u < nv; u++) {                        // ridges: the normalised line functions of two edges, sum and difference
        double fx, fy, ff;
        if (!line(q, u, m, fx, fy, ff)) continue;
        const double lu = sqrt(ff);
        for (int k = 0; k < 4; k++) e[k] = l[k] / lv + m[k] / lu;
        span_roots(e, 3, L, emit);
        for (int k = 0; k < 4; k++) e[k] = l[k] / lv - m[k] / lu;
        span_roots(e, 3, L, emit);
      }
    }
  }
};

// one call's findings of an agent into its record (strictly smaller wins: an earlier call keeps a tie)
NEP_AUDIT_FN void span_fold(const SpanCall& c, const SpanWin& w, nep_span_audit* A) {
  if (c.center.v < A->center_d2) { A->center_d2 = c.center.v; A->center_partner = c.center.who; A->t_center = c.center.t; }
  if (c.box.v < A->min_box_clear) { A->min_box_clear = c.box.v; A->box_partner = c.box.who; A->t_box = c.box.t; }
  if (c.stat.v < A->min_static_dist) { A->min_static_dist = c.stat.v; A->static_index = c.stat.who; A->t_static = c.stat.t; }
  A->min_center_dist = sqrt(A->center_d2);
  if (c.box.v < 0.0) A->n_pair_viol = A->n_pair_viol + 1;
  if (c.stat.v < 0.0) A->n_static_viol = A->n_static_viol + 1;
  if (c.box.v < c.tick_box) { const double gap = c.tick_box - c.box.v; if (gap > A->gap_box) A->gap_box = gap; }
  if (c.stat.v < c.tick_stat) { const double gap = c.tick_stat - c.stat.v; if (gap > A->gap_static) A->gap_static = gap; }
  A->n_spans = A->n_spans + 1;
  A->span = A->span + (w.t1 - w.t0);
}

}  // namespace nep_span_impl
#endif  // NEP_AUDIT_SPAN_COMMON_H_
