// span_audit_check.cpp — the span audit's host form (neptune_amd/csrc/audit_span_host.cpp) on inputs no flight produces, as a
// stand-alone program for -fsanitize=address,undefined (tests/test_span_audit_cpu.py builds and runs it): malformed records,
// zero-length windows, degenerate polygons and the capacities.  Every call must return, touch nothing outside its arrays and keep
// the audit's invariant where it has a meaning: the span minimum is <= the tick audit's over the same call.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "neptune_frontend.h"

namespace nep { void set_last_error(const std::string&) {} }

static int failures = 0, runs = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d (run %d): %s\n", __LINE__, runs, #c); failures++; } } while (0)

static nep_traj_rec line_rec(int id, double x, double y, double vx, double vy, double t0, int n_seg, double dur) {
  nep_traj_rec r;
  std::memset(&r, 0, sizeof r);
  r.id = id; r.is_agent = 1; r.valid = 1; r.n_bend = 1;
  r.bbox[0] = r.bbox[1] = r.bbox[2] = 0.6;
  r.pwp.n_seg = n_seg;
  for (int i = 0; i <= n_seg && i <= NEP_TRAJ_MAX_SEG; i++) r.pwp.times[i] = t0 + i * dur;
  for (int i = 0; i < n_seg && i < NEP_TRAJ_MAX_SEG; i++) {
    r.pwp.coeff[0][i][2] = vx; r.pwp.coeff[0][i][3] = x + vx * i * dur;
    r.pwp.coeff[1][i][2] = vy; r.pwp.coeff[1][i][3] = y + vy * i * dur;
  }
  return r;
}

static void run(const std::vector<nep_traj_rec>& recs, const std::vector<int32_t>& off, const std::vector<double>& xy, double t0, double tick, int n_ticks,
                int want = 0) {
  const int n = (int)recs.size(), ns = (int)off.size() - 1;
  runs++;
  std::vector<nep_span_audit> sp(n + 1);      // (one more than the call may touch)
  std::vector<nep_audit> tk(n + 1);
  CHECK(nep_span_audit_init(sp.data(), n + 1) == 0);
  CHECK(nep_audit_init(tk.data(), n + 1) == 0);
  const nep_span_audit fresh = sp[n];
  const int e = nep_span_audit_records(recs.data(), n, off.data(), xy.data(), ns, 0.3, t0, tick, n_ticks, sp.data());
  CHECK(e == want);
  CHECK(std::memcmp(&sp[n], &fresh, sizeof fresh) == 0);
  if (e != 0) { for (int a = 0; a < n; a++) CHECK(std::memcmp(&sp[a], &fresh, sizeof fresh) == 0); return; }
  CHECK(nep_audit_records(recs.data(), n, off.data(), xy.data(), ns, 0.3, t0, tick, n_ticks, tk.data()) == 0);
  for (int a = 0; a < n; a++) {
    if (tk[a].min_box_clear == tk[a].min_box_clear) CHECK(sp[a].min_box_clear <= tk[a].min_box_clear);
    if (tk[a].min_static_dist == tk[a].min_static_dist) CHECK(sp[a].min_static_dist <= tk[a].min_static_dist);
    if (tk[a].center_d2 == tk[a].center_d2) CHECK(sp[a].center_d2 <= tk[a].center_d2);
    CHECK(sp[a].n_spans == (tk[a].n_ticks > 0 ? 1 : 0));
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<int32_t> off0{0};
  const std::vector<double> xy0{0.0, 0.0};
  const std::vector<int32_t> sq_off{0, 4};
  const std::vector<double> sq{0, 0, 1, 0, 1, 1, 0, 1};
  std::vector<nep_traj_rec> two{line_rec(1, -1, 0, 1, 0, 0.0, 4, 0.5), line_rec(2, 0, -1.3, 0, 1, 0.0, 3, 0.7)};

  run(two, sq_off, sq, 0.0, 0.125, 16);
  // zero-length windows: no ticks (nothing happens), ticks of length 0 (one instant), a single tick
  run(two, sq_off, sq, 1.0, 0.125, 0);
  run(two, sq_off, sq, 1.0, 0.0, 5);
  run(two, sq_off, sq, 1.15, 1e-300, 3);
  run(two, sq_off, sq, 0.0, 0.125, 1);
  // windows before every record and beyond every record: everybody at rest
  run(two, sq_off, sq, -10.0, 0.125, 8);
  run(two, sq_off, sq, 100.0, 0.125, 8);
  // clocks and ticks that are no numbers
  run(two, sq_off, sq, nan, 0.125, 8);
  run(two, sq_off, sq, inf, 0.125, 8);
  run(two, sq_off, sq, 0.0, inf, 2, NEP_E_ARG);
  run(two, sq_off, sq, 0.0, nan, 2, NEP_E_ARG);
  run(two, sq_off, sq, 0.0, -0.125, 2, NEP_E_ARG);
  run(two, sq_off, sq, 0.0, 0.125, -1, NEP_E_ARG);
  // malformed records: more segments than the record holds, none, knots out of order, repeated, infinite, not a number;
  // coefficients that overflow
  {
    std::vector<nep_traj_rec> r = two;
    r[0].pwp.n_seg = 1000; run(r, sq_off, sq, 0.0, 0.125, 16);
    r[0].pwp.n_seg = NEP_TRAJ_MAX_SEG; run(r, sq_off, sq, 0.0, 0.125, 16);      // (knots 5..16 are zero: out of order)
    r[0].pwp.n_seg = 0; run(r, sq_off, sq, 0.0, 0.125, 16);
    r[0].pwp.n_seg = -3; run(r, sq_off, sq, 0.0, 0.125, 16);
    r = two; r[0].pwp.times[2] = 0.1; run(r, sq_off, sq, 0.0, 0.125, 16);
    r = two; r[0].pwp.times[2] = r[0].pwp.times[1]; run(r, sq_off, sq, 0.0, 0.125, 16);
    r = two; r[0].pwp.times[4] = inf; run(r, sq_off, sq, 0.0, 0.125, 16);
    r = two; r[1].pwp.times[1] = nan; run(r, sq_off, sq, 0.0, 0.125, 16);
    r = two; r[1].pwp.coeff[0][0][0] = 1e308; r[1].pwp.coeff[1][1][1] = -1e308; run(r, sq_off, sq, 0.0, 0.125, 16);
    r = two; r[0].pwp.coeff[1][0][3] = nan; run(r, sq_off, sq, 0.0, 0.125, 16);
    r = two; r[0].valid = 0; r[1].is_agent = 0; run(r, sq_off, sq, 0.0, 0.125, 16);
    r = two; r[0].bbox[0] = -5.0; r[1].bbox[1] = inf; run(r, sq_off, sq, 0.0, 0.125, 16);
  }
  // the most knots a window can hold: two records of NEP_TRAJ_MAX_SEG segments on grids that never coincide, many ticks
  {
    std::vector<nep_traj_rec> r{line_rec(1, -1, 0, 1, 0, 0.0, NEP_TRAJ_MAX_SEG, 0.11), line_rec(2, 0, -1.3, 0, 1, 0.003, NEP_TRAJ_MAX_SEG, 0.13)};
    run(r, sq_off, sq, 0.0, 0.007, 300);
  }
  // degenerate polygons: none, no vertices, one vertex, two, every vertex the same, a repeated vertex, collinear, clockwise
  run(two, off0, xy0, 0.0, 0.125, 16);
  run(two, {0, 0}, xy0, 0.0, 0.125, 16);
  run(two, {0, 1}, {0.5, 0.2}, 0.0, 0.125, 16);
  run(two, {0, 2}, {-0.5, -0.2, 0.5, 0.2}, 0.0, 0.125, 16);
  run(two, {0, 3}, {0.1, 0.1, 0.1, 0.1, 0.1, 0.1}, 0.0, 0.125, 16);
  run(two, {0, 4}, {0, 0, 1, 0, 1, 0, 0, 1}, 0.0, 0.125, 16);
  run(two, {0, 3}, {-1, 0, 0, 0, 1, 0}, 0.0, 0.125, 16);
  run(two, {0, 4}, {0, 1, 1, 1, 1, 0, 0, 0}, 0.0, 0.125, 16);
  run(two, {0, 0, 4, 4, 5}, {0, 0, 1, 0, 1, 1, 0, 1, 3, 3}, 0.0, 0.125, 16);
  // the capacities: a polygon of NEP_HULL_MAX_V vertices is taken, one more is NEP_E_CAP; offsets that decrease are refused
  {
    std::vector<double> ring;
    for (int v = 0; v <= NEP_HULL_MAX_V; v++) { const double a = 6.283185307179586 * v / (NEP_HULL_MAX_V + 1); ring.push_back(0.3 + std::cos(a)); ring.push_back(std::sin(a)); }
    run(two, {0, NEP_HULL_MAX_V}, ring, 0.0, 0.125, 4);
    run(two, {0, NEP_HULL_MAX_V + 1}, ring, 0.0, 0.125, 4, NEP_E_CAP);
    run(two, {0, NEP_HULL_MAX_V + 1}, ring, 0.0, 0.125, 0, NEP_E_CAP);      // (refused by a call without ticks too)
    run(two, {0, 3, 1}, ring, 0.0, 0.125, 4, NEP_E_ARG);
  }
  // no agents at all; null arrays
  run({}, sq_off, sq, 0.0, 0.125, 4);
  CHECK(nep_span_audit_records(nullptr, 2, sq_off.data(), sq.data(), 1, 0.3, 0.0, 0.125, 4, nullptr) == NEP_E_ARG);
  CHECK(nep_span_audit_records(two.data(), 2, nullptr, nullptr, 1, 0.3, 0.0, 0.125, 4, nullptr) == NEP_E_ARG);
  CHECK(nep_span_audit_init(nullptr, 3) == NEP_E_ARG);
  CHECK(nep_span_audit_init(nullptr, 0) == 0);
  if (failures) { std::printf("span_audit_check: %d failures\n", failures); return 1; }
  std::printf("span_audit_check ok\n");
  return 0;
}
