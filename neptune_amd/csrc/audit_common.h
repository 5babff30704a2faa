// audit_common.h — the arithmetic of the flight audit (include/neptune_frontend.h: nep_audit), shared by its host form
// (audit_host.cpp) and its device form (audit_kernels.hip).  Both are built -ffp-contract=off, every candidate is computed by the
// expressions below in both, and every minimum is taken with "strictly smaller wins" over candidates visited by rising tick and,
// within a tick, by rising partner id or polygon index — the tie rule that makes a parallel walk equal a serial one.
#ifndef NEP_AUDIT_COMMON_H_
#define NEP_AUDIT_COMMON_H_

#include <math.h>

#include "../../include/neptune_frontend.h"

#ifndef NEP_AUDIT_FN
#define NEP_AUDIT_FN static inline
#endif

namespace nep_audit_impl {

// A workgroup of the device form audits a run of consecutive ticks; the run's length depends on n_ticks only (and no result
// depends on it: minima do not care, and the sums are taken by one thread in tick order).
constexpr int kAuditMinChunk = 1;       // ticks per workgroup, at least (a round of 10 ticks and 32 scenes: 320 workgroups for 256 CUs)
constexpr int kAuditMaxChunks = 32;     // workgroups per scene, at most: the handle's scratch is sized by it once

// x, y of an agent at a tick, what it needs as somebody's partner (half-widths of its inflated box) and its x-y speed
struct AuditState { double x, y, speed; };

NEP_AUDIT_FN bool audit_present(const nep_traj_rec* r) { return r->valid && r->is_agent && r->pwp.n_seg >= 1; }

// The state of a record at time t, as next_starts_kernel evaluates it (geom_kernels.hip; generatePwpOut's samples,
// solver_gurobi_poly.cpp:921-929): u clamped to 0 before the first knot, at rest on the end point beyond the last.
NEP_AUDIT_FN AuditState audit_eval(const nep_traj_rec* r, double t) {
  const int n = r->pwp.n_seg < NEP_TRAJ_MAX_SEG ? r->pwp.n_seg : NEP_TRAJ_MAX_SEG;
  int i = 0;
  for (int k = 1; k < n; k++) if (t >= r->pwp.times[k]) i = k;
  const bool past = t >= r->pwp.times[n];
  double u = t - r->pwp.times[i];
  if (u < 0.0) u = 0.0;
  if (past) u = r->pwp.times[n] - r->pwp.times[n - 1];
  double p[2], v[2];
  for (int ax = 0; ax < 2; ax++) {
    const double* c = r->pwp.coeff[ax][i];
    p[ax] = ((c[0] * (u * u * u) + c[1] * (u * u)) + c[2] * u) + c[3];
    v[ax] = past ? 0.0 : (c[0] * (3 * u * u) + c[1] * (2 * u)) + c[2];
  }
  AuditState s;
  s.x = p[0]; s.y = p[1]; s.speed = sqrt(v[0] * v[0] + v[1] * v[1]);
  return s;
}

// 1 / |b - a|^2 of a polygon edge (0 for a repeated vertex): one division per edge, made when the polygons are staged
NEP_AUDIT_FN double audit_edge_inv(double ax, double ay, double bx, double by) {
  const double ex = bx - ax, ey = by - ay;
  const double ee = ex * ex + ey * ey;
  return ee > 0.0 ? 1.0 / ee : 0.0;
}

// One edge a -> b of a counter-clockwise polygon against the point p: the squared distance to the segment goes into d2 (a
// running minimum), and a point strictly right of the edge is outside the polygon.
NEP_AUDIT_FN void audit_edge(double px, double py, double ax, double ay, double bx, double by, double inv, double& d2, bool& inside) {
  const double ex = bx - ax, ey = by - ay, wx = px - ax, wy = py - ay;
  double s = (wx * ex + wy * ey) * inv;
  s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
  const double cx = wx - s * ex, cy = wy - s * ey;
  const double q = cx * cx + cy * cy;
  if (q < d2) d2 = q;
  if (ex * wy - ey * wx < 0.0) inside = false;
}

// signed distance of a polygon from the smallest squared edge distance: negative inside (fewer than three vertices have no inside)
NEP_AUDIT_FN double audit_signed(double d2, bool inside, int nv) {
  const double d = sqrt(d2);
  return (inside && nv >= 3 && d > 0.0) ? -d : d;
}

// how far the centre (dx, dy away from partner j's) lies outside j's inflated box (half-widths hx, hy)
NEP_AUDIT_FN double audit_box_clear(double dx, double dy, double hx, double hy) {
  const double a = fabs(dx) - hx, b = fabs(dy) - hy;
  return a > b ? a : b;
}

NEP_AUDIT_FN int audit_chunk_len(int n_ticks) {
  const int l = (n_ticks + kAuditMaxChunks - 1) / kAuditMaxChunks;
  return l > kAuditMinChunk ? l : kAuditMinChunk;
}

// Path length, top speed and tick count of one agent over a call's ticks, in tick order (the step from the previous call's last
// tick included).
NEP_AUDIT_FN void audit_path(const nep_traj_rec* r, double t0, double tick, int n_ticks, nep_audit* a) {
  for (int k = 0; k < n_ticks; k++) {
    const AuditState s = audit_eval(r, t0 + (double)k * tick);
    if (a->n_ticks > 0) {
      const double dx = s.x - a->last_xy[0], dy = s.y - a->last_xy[1];
      a->path_len = a->path_len + sqrt(dx * dx + dy * dy);
    }
    if (s.speed > a->max_speed) a->max_speed = s.speed;
    a->last_xy[0] = s.x; a->last_xy[1] = s.y;
    a->n_ticks = a->n_ticks + 1;
  }
}

}  // namespace nep_audit_impl
#endif  // NEP_AUDIT_COMMON_H_
