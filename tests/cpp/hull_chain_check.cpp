// hull_chain_check.cpp — drives neptune_amd/csrc/hull_chain.h on the host (its own main; tests/test_hull_chain_skip_cpu.py).
// Makes interval hulls the way hull_group_kernel does — 1-4 committed segments, control points V = (P C) A^-1 in the kernel's association,
// four inflated corners each, lexicographic sort, duplicate removal with the skip flags made on the way — and walks both chains twice:
// every point (the plain walk) and the to-do masks of the skip rule.  The final stacks must be the same masks.  A third walk takes the
// rule WITHOUT its gap condition (any point above its predecessor in a run is skipped): it must differ somewhere, or the input never
// reaches the hazard the gap is there for.
//   hull_chain_check fuzz N SEED   one line of counts
//   hull_chain_check edge N SEED   the same on coordinates of 1e9, 1e149, 1e151, 1e-149 ... 1e-320 (a magnitude per axis)
//   hull_chain_check dump N SEED   per hull: "n_seg dx dy | knots | coeff x | coeff y | k | vertices" (hexadecimal doubles): the
//                                  masked walk's hull, min(k, 16) vertices, for the oracle's hull_of_interval
// Segments: random cubics, constants (their control points are P * {1, 1, 1 - 4e-16, 1 - 7e-16}: clusters within ulps), straight and
// axis-aligned lines; positions at +-50 m, rounded to integers, below 1e-3, and |x| < 1e-9 beside y ~ 45; radii 0.05-0.3, one hull in
// twenty without inflation.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../neptune_amd/csrc/hull_chain.h"
#include "../../neptune_amd/csrc/nep_tables.h"

using namespace nep;
typedef unsigned long long u64;

struct Rng {
  uint64_t s;
  uint64_t next() { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }      // [0, 1)
  double sym(double a) { return (2.0 * uni() - 1.0) * a; }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Hull {
  int n_seg; double dx, dy;
  double knots[5]; double coeff[2][4][4];
  int np0, np; double cp[16][2]; double pts[64][2];
};

static double poly(const double* P, double t) { return ((P[0] * t + P[1]) * t + P[2]) * t + P[3]; }

// edge: magnitudes where the rule has to give way or hold by its floors — 1e9, either side of 1e150, around 1e-150, subnormals — per axis
static void make(Rng& r, Hull& h, bool edge) {
  std::memset(&h, 0, sizeof h);
  const int n = 1 + r.below(4);
  h.n_seg = n;
  for (int s = 0; s < n; s++) h.knots[s] = 0.1 * s;
  h.knots[n] = 0.5;
  const int regime = edge ? 4 : r.below(4);
  static const double kMag[8] = {1e9, 1e149, 1e151, 1e-149, 1e-151, 1e-160, 1e-300, 1e-320};
  const double mx = kMag[r.below(8)], my = kMag[r.below(8)];
  double sx = 1.0, sy = 1.0, pos[2];
  auto fresh = [&]() {
    switch (regime) {
      case 0: pos[0] = r.sym(50.0); pos[1] = r.sym(50.0); break;
      case 1: pos[0] = std::nearbyint(r.sym(50.0)); pos[1] = std::nearbyint(r.sym(50.0)); break;
      case 2: pos[0] = r.sym(1e-3); pos[1] = r.sym(1e-3); break;
      case 3: pos[0] = r.sym(1e-9); pos[1] = r.below(2) ? 45.0 : 45.0 + r.sym(0.5); break;
      default: pos[0] = r.below(4) ? r.sym(mx) : 0.0; pos[1] = r.below(4) ? r.sym(my) : 0.0; break;
    }
  };
  if (regime == 2) sx = sy = 1e-3;
  if (regime == 3) sx = 1e-9;
  if (regime == 4) { sx = mx; sy = my; }
  fresh();
  for (int s = 0; s < n; s++) {
    const int kind = r.below(4);
    const double sc[2] = {sx, sy};
    for (int ax = 0; ax < 2; ax++) {
      double* P = h.coeff[ax][s];
      P[3] = pos[ax];
      if (kind == 0) { P[0] = r.sym(0.05) * sc[ax]; P[1] = r.sym(0.1) * sc[ax]; P[2] = r.sym(0.5) * sc[ax]; }
      else if (kind == 2) P[2] = r.sym(0.5) * sc[ax];
    }
    if (kind == 3) h.coeff[r.below(2)][s][2] = r.sym(0.5) * (regime == 2 ? 1e-3 : regime == 4 ? mx : 1.0);      // (axis-aligned: one axis moves)
    const double dt = h.knots[s + 1] - h.knots[s];
    if (r.below(2)) { pos[0] = poly(h.coeff[0][s], dt); pos[1] = poly(h.coeff[1][s], dt); } else fresh();
  }
  if (r.below(20) == 0) h.dx = h.dy = 0.0;
  else { h.dx = 0.05 + 0.25 * r.uni(); h.dy = r.below(2) ? h.dx : 0.05 + 0.25 * r.uni(); }
  if (edge && r.below(2)) { h.dx *= mx; h.dy *= my; }
  // hull_group_kernel's interval [0, 0.5] with T_span 0.5: every segment, _t = its length (neptune.cpp:399-424)
  h.np0 = 4 * n;
  for (int s = 0; s < n; s++) {
    double _t = h.knots[s + 1] - h.knots[s];
    if (_t > 0.5) _t = 0.5; else if (_t < 0) _t = 0;
    const double c0 = _t * _t * _t, c1 = _t * _t, c2 = _t, c3 = 1.0;
    for (int k = 0; k < 4; k++)
      for (int ax = 0; ax < 2; ax++) {
        const double* P = h.coeff[ax][s];
        h.cp[4 * s + k][ax] = (((P[0] * c0) * kAPosInv[0][k] + (P[1] * c1) * kAPosInv[1][k]) + (P[2] * c2) * kAPosInv[2][k]) + (P[3] * c3) * kAPosInv[3][k];
      }
  }
  const bool inflate = !(std::sqrt(h.dx * h.dx + h.dy * h.dy) < 1e-6);
  h.np = 0;
  for (int c = 0; c < h.np0; c++) {
    const double x = h.cp[c][0], y = h.cp[c][1];
    if (!inflate) { h.pts[h.np][0] = x; h.pts[h.np][1] = y; h.np++; continue; }
    for (int q = 0; q < 4; q++) { h.pts[h.np][0] = (q < 2) ? x + h.dx : x - h.dx; h.pts[h.np][1] = (q == 0 || q == 3) ? y + h.dy : y - h.dy; h.np++; }
  }
}

struct Walks { int m; u64 plain[2], masked[2], nogap[2]; u64 todo[2]; bool off; };
alignas(16) static double g_sxy[128];

// the kernel's unique pass on the sorted points, then the walks
static void walk(const Hull& h, Walks& w) {
  struct P2 { double x, y; };
  P2 s[64];
  for (int i = 0; i < h.np; i++) s[i] = {h.pts[i][0], h.pts[i][1]};
  std::sort(s, s + h.np, [](const P2& a, const P2& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
  double cm0 = 0;
  for (int c = 0; c < h.np0; c++) cm0 = std::fmax(cm0, std::fmax(std::fabs(h.cp[c][0]), std::fabs(h.cp[c][1])));
  const bool inflate = h.np != h.np0;
  const double thr = chain_skip_threshold(inflate ? cm0 + std::fmax(std::fabs(h.dx), std::fabs(h.dy)) : cm0);
  u64 flg = 0, flg0 = 0; bool tiny = false; int m = 0;
  for (int p = 0; p < h.np; p++) {
    const bool keep = p == 0 || s[p].x != s[p - 1].x || s[p].y != s[p - 1].y;
    if (!keep) continue;
    if (p != 0) {
      if (chain_skip_flag(s[p].x, s[p].y, s[p - 1].x, s[p - 1].y, thr)) flg |= 1ull << m;
      if (chain_skip_flag(s[p].x, s[p].y, s[p - 1].x, s[p - 1].y, 0.0)) flg0 |= 1ull << m;
      tiny |= chain_gap_tiny(s[p].x, s[p - 1].x);
    }
    g_sxy[2 * m] = s[p].x; g_sxy[2 * m + 1] = s[p].y; m++;
  }
  if (tiny) flg = 0;
  w.m = m; w.off = tiny || !(thr < __builtin_huge_val());
  for (int c = 0; c < 2; c++) {
    w.plain[c] = w.masked[c] = w.nogap[c] = w.todo[c] = 0;
    if (m < 2) continue;
    const bool lower = c == 0;
    const u64 all = m >= 64 ? ~0ull : (1ull << m) - 1ull;
    w.todo[c] = chain_todo(flg, m, lower);
    w.plain[c] = chain_walk(g_sxy, m, lower, all);
    w.masked[c] = chain_walk(g_sxy, m, lower, w.todo[c]);
    w.nogap[c] = chain_walk(g_sxy, m, lower, chain_todo(flg0, m, lower));
  }
}

static int popc(u64 v) { return __builtin_popcountll(v); }

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: hull_chain_check fuzz|edge|dump N SEED\n"); return 2; }
  const bool dump = std::strcmp(argv[1], "dump") == 0, edge = std::strcmp(argv[1], "edge") == 0;
  const long N = std::atol(argv[2]);
  Rng r{(uint64_t)std::atoll(argv[3])};
  // the masks' index spaces on a case small enough to do by hand: m = 5, flags at sorted 1 and 4
  //   lower: 4 is the last point and stays; 1 goes -> 0b11101.  upper: sorted j goes iff j + 1 is flagged and j != 0 -> sorted 3, push index 1 -> 0b11101
  if (chain_todo(0x12, 5, true) != 0x1d || chain_todo(0x12, 5, false) != 0x1d || chain_todo(0x2, 5, false) != 0x1f || chain_todo(~0ull, 64, false) != ((1ull << 63) | 1ull)) {
    std::fprintf(stderr, "chain_todo: wrong masks\n"); return 1;
  }
  long bad = 0, bad0 = 0, visits = 0, visits_m = 0, off = 0, uninflated = 0, few = 0, kinds_m[65] = {0};
  Hull h; Walks w;
  for (long i = 0; i < N; i++) {
    make(r, h, edge);
    walk(h, w);
    kinds_m[w.m]++;
    if (w.off) off++;
    if (h.np == h.np0) uninflated++;
    if (w.m < 4) few++;
    if (w.plain[0] != w.masked[0] || w.plain[1] != w.masked[1]) bad++;
    if (w.plain[0] != w.nogap[0] || w.plain[1] != w.nogap[1]) bad0++;
    if (w.m >= 2) { visits += 2 * w.m; visits_m += popc(w.todo[0]) + popc(w.todo[1]); }
    if (dump) {
      std::printf("%d %a %a |", h.n_seg, h.dx, h.dy);
      for (int s = 0; s <= h.n_seg; s++) std::printf(" %a", h.knots[s]);
      for (int ax = 0; ax < 2; ax++) { std::printf(" |"); for (int s = 0; s < h.n_seg; s++) for (int j = 0; j < 4; j++) std::printf(" %a", h.coeff[ax][s][j]); }
      // the hull as group_hull writes it: the lower chain, then the upper chain without its two end points
      double v[130][2]; int k = 0;
      if (w.m == 1) { v[0][0] = g_sxy[0]; v[0][1] = g_sxy[1]; k = 1; }
      else if (w.m >= 2) {
        for (int p = 0; p < w.m; p++) if ((w.masked[0] >> p) & 1ull) { v[k][0] = g_sxy[2 * p]; v[k][1] = g_sxy[2 * p + 1]; k++; }
        for (int iu = 1; iu < w.m - 1; iu++) if ((w.masked[1] >> iu) & 1ull) { const int p = w.m - 1 - iu; v[k][0] = g_sxy[2 * p]; v[k][1] = g_sxy[2 * p + 1]; k++; }
      }
      std::printf(" | %d |", k);
      for (int j = 0; j < (k < 16 ? k : 16); j++) std::printf(" %a %a", v[j][0], v[j][1]);
      std::printf("\n");
    }
  }
  std::printf("hulls=%ld mismatches=%ld mismatches_without_gap=%ld visits_plain=%ld visits_masked=%ld skipping_off=%ld uninflated=%ld under_4_points=%ld full_64=%ld\n",
              N, bad, bad0, visits, visits_m, off, uninflated, few, kinds_m[64]);
  std::printf("hull_chain_check ok\n");
  return 0;
}
