// hull_pair_sort_check.cpp — drives neptune_amd/csrc/hull_pair_sort.h on the host (its own main; tests/test_hull_pair_sort_cpu.py).
// Makes interval hulls the way hull_group_kernel does — 1-4 committed segments, control points V = (P C) A^-1 in the kernel's
// association, four inflated corners each — and sorts every hull these ways:
//   ref      std::sort of the 4 np0 corners, lexicographic: what the full network (grp_bitonic<8, 64>) stores;
//   rule     what the kernel stores: the header's network over the 2 np0 stacked pairs (8 lanes x 4 registers), stored run by run
//            (pair_run_of, pair_store), where pair_sort_allowed, the key test and the run test say so; the corners' sort (ref) otherwise;
//   noruns   every sorted pair expanded where it stands, whatever its neighbours' keys;
//   norule   the run-by-run array of the hulls the rule refuses.
// rule must equal ref element for element, as bits, in every hull.  noruns and norule must differ somewhere, or the input never
// reaches the hazards the runs and the rule are there for.  (A NaN among the x or the y: refused, checked on its own.)  The eight lanes
// of a group are plain arrays here (HostLanes): a step across lanes reads a copy of the partner's registers, as the DPP moves of the
// kernel do.
//   hull_pair_sort_check N SEED    one line of counts per family, then a total
// Families: cubics (random cubics), constants (segments at rest: control points P * {1, 1, 1 - 4e-16, 1 - 7e-16}, clusters within ulps),
// lines (axis-aligned), mixed (hull_chain_check's mix of all of these at +-50 m, on integers, below 1e-3, |x| < 1e-9), big (magnitudes
// 1e9, 1e149, 1e151 per axis), tiny (1e-149 ... 1e-320, subnormals included), same_x (control points equal in x, different in y),
// dup (control points repeated), zeros (x = +-dx exactly: keys -0.0 and +0.0), collapse (x a few ulps apart at |x| << dx, so that
// x + dx rounds to one key), neg_dy (dy < 0: ylo > yhi, the pair path is refused).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../neptune_amd/csrc/hull_pair_sort.h"
#include "../../neptune_amd/csrc/nep_tables.h"

using namespace nep;

struct Rng {
  uint64_t s;
  uint64_t next() { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }      // [0, 1)
  double sym(double a) { return (2.0 * uni() - 1.0) * a; }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

enum Family { kCubics, kConstants, kLines, kMixed, kBig, kTiny, kSameX, kDup, kZeros, kCollapse, kNegDy, kFamilies };
static const char* const kFamilyName[kFamilies] = {"cubics", "constants", "lines", "mixed", "big", "tiny", "same_x", "dup", "zeros", "collapse", "neg_dy"};

struct Hull { int np0; double dx, dy; double cp[16][2]; };

static double poly(const double* P, double t) { return ((P[0] * t + P[1]) * t + P[2]) * t + P[3]; }
static double ulps(double v, int n) { for (int i = 0; i < std::abs(n); i++) v = std::nextafter(v, n > 0 ? HUGE_VAL : -HUGE_VAL); return v; }

// segments -> control points, as hull_group_kernel's interval [0, 0.5] with T_span 0.5 makes them (neptune.cpp:399-429)
static void control_points(Hull& h, int n, const double* knots, const double (&coeff)[2][4][4]) {
  h.np0 = 4 * n;
  for (int s = 0; s < n; s++) {
    double _t = knots[s + 1] - knots[s];
    if (_t > 0.5) _t = 0.5; else if (_t < 0) _t = 0;
    const double c0 = _t * _t * _t, c1 = _t * _t, c2 = _t, c3 = 1.0;
    for (int k = 0; k < 4; k++)
      for (int ax = 0; ax < 2; ax++) {
        const double* P = coeff[ax][s];
        h.cp[4 * s + k][ax] = (((P[0] * c0) * kAPosInv[0][k] + (P[1] * c1) * kAPosInv[1][k]) + (P[2] * c2) * kAPosInv[2][k]) + (P[3] * c3) * kAPosInv[3][k];
      }
  }
}

static void make(Rng& r, Hull& h, Family f) {
  std::memset(&h, 0, sizeof h);
  const int n = 1 + r.below(4);
  double knots[5] = {0}, coeff[2][4][4];
  std::memset(coeff, 0, sizeof coeff);
  for (int s = 0; s < n; s++) knots[s] = 0.1 * s;
  knots[n] = 0.5;
  const bool edge = f == kBig || f == kTiny;
  const int regime = edge ? 4 : f == kMixed ? r.below(4) : r.below(2);
  static const double kBigMag[3] = {1e9, 1e149, 1e151}, kTinyMag[5] = {1e-149, 1e-151, 1e-160, 1e-300, 1e-320};
  const double mx = f == kBig ? kBigMag[r.below(3)] : kTinyMag[r.below(5)], my = f == kBig ? kBigMag[r.below(3)] : kTinyMag[r.below(5)];
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
    const int kind = f == kCubics ? 0 : f == kConstants ? 1 : f == kLines ? 3 : r.below(4);      // 0 cubic, 1 constant, 2 straight, 3 axis-aligned
    const double sc[2] = {sx, sy};
    for (int ax = 0; ax < 2; ax++) {
      double* P = coeff[ax][s];
      P[3] = pos[ax];
      if (kind == 0) { P[0] = r.sym(0.05) * sc[ax]; P[1] = r.sym(0.1) * sc[ax]; P[2] = r.sym(0.5) * sc[ax]; }
      else if (kind == 2) P[2] = r.sym(0.5) * sc[ax];
    }
    if (kind == 3) coeff[r.below(2)][s][2] = r.sym(0.5) * (regime == 2 ? 1e-3 : regime == 4 ? mx : 1.0);
    const double dt = knots[s + 1] - knots[s];
    if (r.below(2)) { pos[0] = poly(coeff[0][s], dt); pos[1] = poly(coeff[1][s], dt); } else fresh();
  }
  h.dx = 0.05 + 0.25 * r.uni(); h.dy = r.below(2) ? h.dx : 0.05 + 0.25 * r.uni();
  if (edge && r.below(2)) { h.dx *= mx; h.dy *= my; }
  control_points(h, n, knots, coeff);
  // the families made on the control points themselves (what a trajectory's coefficients would have to give)
  const int np0 = h.np0;
  switch (f) {
    case kSameX: { const int a = r.below(np0); int b = r.below(np0 - 1); if (b >= a) b++; h.cp[b][0] = h.cp[a][0]; if (h.cp[b][1] == h.cp[a][1]) h.cp[b][1] += 1.0; } break;
    case kDup: { const int a = r.below(np0); int b = r.below(np0 - 1); if (b >= a) b++; h.cp[b][0] = h.cp[a][0]; h.cp[b][1] = h.cp[a][1]; } break;
    case kZeros: {      // x - dx = +0.0 here, x + dx = -0.0 there, and sometimes a plain 0 beside them
      const int a = r.below(np0); int b = r.below(np0 - 1); if (b >= a) b++;
      h.cp[a][0] = h.dx; h.cp[b][0] = -h.dx;
      if (r.below(2)) h.cp[r.below(np0)][0] = r.below(2) ? 0.0 : -0.0;
    } break;
    case kCollapse: {      // |x| << dx: x + dx has dx's spacing, a few ulps of x vanish in it (sometimes they straddle a rounding boundary and do not)
      const double x = r.sym(1e-6);
      const int a = r.below(np0); int b = r.below(np0 - 1); if (b >= a) b++;
      h.cp[a][0] = x; h.cp[b][0] = ulps(x, 1 + r.below(4)); h.cp[b][1] = h.cp[a][1] + r.sym(1.0);
      if (r.below(3) == 0) { const double big = r.sym(40.0); h.cp[a][0] = big; h.cp[b][0] = ulps(big, 1); }      // (a pair of keys that stay apart)
    } break;
    case kNegDy: h.dy = -h.dy; break;
    default: break;
  }
}

// The group's eight lanes as arrays: the network of the header, run lane by lane; a step across lanes reads a copy of every lane's
// registers made before the step.
constexpr int J = kPairJ;
struct HostLanes {
  double kx[8][J], ky[8][J];
  template <int K_, int JJ> void step() {
    if constexpr (JJ < J) { for (int sub = 0; sub < 8; sub++) pair_step_local<J, K_, JJ>(kx[sub], ky[sub], sub); }
    else {
      double ox[8][J], oy[8][J];
      std::memcpy(ox, kx, sizeof ox); std::memcpy(oy, ky, sizeof oy);
      for (int sub = 0; sub < 8; sub++) pair_step_cross<J, K_, JJ>(kx[sub], ky[sub], sub, ox[sub ^ (JJ / J)], oy[sub ^ (JJ / J)]);
    }
  }
};

// group_sort_pairs of the kernel: the pairs, the network, the key test, where runs begin, the store, the run test.
//   sxy     the array as the kernel stores it            -> kKeyBad, or kRunBad (sxy written all the same), or kOk
//   plain   every pair expanded where it stands (no runs): what the array would be without them
enum Verdict { kOk, kKeyBad, kRunBad };
static Verdict sort_pairs(const Hull& h, double* sxy, double* plain, bool& has_run) {
  HostLanes L;
  const int P = 2 * h.np0;
  for (int sub = 0; sub < 8; sub++)
    for (int r = 0; r < J; r++) {
      const int pi = sub * J + r;
      L.kx[sub][r] = pi < P ? pair_x(h.cp[pi >> 1][0], h.dx, pi & 1) : __builtin_huge_val();
      L.ky[sub][r] = pi < P ? h.cp[pi >> 1][1] : __builtin_huge_val();
    }
  pair_bitonic<J, 8 * J>(L);
  const double* X = &L.kx[0][0]; const double* Y = &L.ky[0][0];      // (element e = sub * J + r: the arrays in order)
  unsigned starts = 1u;
  for (int e = 0; e < 32; e++) {
    if (e < P && pair_key_bad(X[e])) return kKeyBad;
    if (e > 0 && X[e] != X[e - 1]) starts |= 1u << e;
  }
  has_run = false;
  bool bad = false;
  for (int e = 0; e < P; e++) {
    int s_, t_;
    pair_run_of(starts, e, s_, t_);
    has_run |= t_ - s_ > 1;
    pair_store(sxy, e, s_, t_, X[e], Y[e], h.dy);
    plain[4 * e] = X[e]; plain[4 * e + 1] = pair_ylo(Y[e], h.dy); plain[4 * e + 2] = X[e]; plain[4 * e + 3] = pair_yhi(Y[e], h.dy);
  }
  for (int e = 0; e < P; e++) {
    int s_, t_;
    pair_run_of(starts, e, s_, t_);
    if (e == s_) bad |= !pair_run_ok(sxy[pair_run_check_at(s_, t_)], pair_yhi(Y[e], h.dy));
  }
  return bad ? kRunBad : kOk;
}

struct Counts { long hulls, fast, fast_with_runs, refused, run_refused, bad, bad_noruns, bad_norule; };

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: hull_pair_sort_check N SEED\n"); return 2; }
  const long N = std::atol(argv[1]);
  Rng r{(uint64_t)std::atoll(argv[2])};
  Counts tot = {0, 0, 0, 0, 0, 0, 0, 0};
  alignas(16) static double sxy[128], plain[128];
  {      // a NaN among the x is invisible to cmax (fmin / fmax drop it): the key test must send the hull to the full network; a NaN among the y: the run test
    Hull h; make(r, h, kCubics);
    bool runs;
    for (int c = 0; c < h.np0; c++) {
      Hull g = h; g.cp[c][0] = __builtin_nan("");
      if (sort_pairs(g, sxy, plain, runs) != kKeyBad) { std::fprintf(stderr, "a NaN key was not refused\n"); return 1; }
      g = h; g.cp[c][1] = __builtin_nan("");
      if (sort_pairs(g, sxy, plain, runs) != kRunBad) { std::fprintf(stderr, "a NaN y was not refused\n"); return 1; }
    }
    // the runs' index arithmetic on a case small enough to do by hand: runs begin at 0, 1, 4, 31
    int s_, t_;
    const unsigned st = 1u | 2u | 16u | (1u << 31);
    pair_run_of(st, 0, s_, t_); if (s_ != 0 || t_ != 1) return 1;
    pair_run_of(st, 3, s_, t_); if (s_ != 1 || t_ != 4) return 1;
    pair_run_of(st, 30, s_, t_); if (s_ != 4 || t_ != 31) return 1;
    pair_run_of(st, 31, s_, t_); if (s_ != 31 || t_ != 32) return 1;
    pair_run_of(1u, 31, s_, t_); if (s_ != 0 || t_ != 32) return 1;
  }
  for (int f = 0; f < kFamilies; f++) {
    Counts c = {0, 0, 0, 0, 0, 0, 0, 0};
    Hull h;
    for (long i = 0; i < N; i++) {
      make(r, h, (Family)f);
      // the corners as the kernel's fallback builds them, and their lexicographic sort
      struct P2 { double x, y; };
      P2 ref[64]; const int np = 4 * h.np0;
      for (int p = 0; p < np; p++) {
        const int cc = p >> 2, q = p & 3;
        const double x = h.cp[cc][0], y = h.cp[cc][1];
        ref[p].x = (q < 2) ? x + h.dx : x - h.dx;
        ref[p].y = (q == 0 || q == 3) ? y + h.dy : y - h.dy;
      }
      std::sort(ref, ref + np, [](const P2& a, const P2& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
      double cm0 = 0;
      for (int cc = 0; cc < h.np0; cc++) cm0 = std::fmax(cm0, std::fmax(std::fabs(h.cp[cc][0]), std::fabs(h.cp[cc][1])));
      const double cmax = cm0 + std::fmax(std::fabs(h.dx), std::fabs(h.dy));
      c.hulls++;
      bool runs = false;
      const bool allowed = pair_sort_allowed(cmax, h.dy);
      const Verdict v = sort_pairs(h, sxy, plain, runs);      // (run for the refused ones too: what would have been stored)
      const bool same = v != kKeyBad && std::memcmp(sxy, ref, sizeof(double) * 2 * np) == 0;
      if (!allowed || v != kOk) {      // the corners' sort: ref itself
        if (!allowed || v == kKeyBad) c.refused++; else c.run_refused++;
        if (!same) c.bad_norule++;
        continue;
      }
      c.fast++;
      if (runs) c.fast_with_runs++;
      if (!same) c.bad++;
      if (std::memcmp(plain, ref, sizeof(double) * 2 * np) != 0) c.bad_noruns++;
    }
    std::printf("family=%s hulls=%ld fast=%ld fast_with_runs=%ld refused=%ld run_refused=%ld mismatches=%ld mismatches_without_runs=%ld mismatches_without_rule=%ld\n",
                kFamilyName[f], c.hulls, c.fast, c.fast_with_runs, c.refused, c.run_refused, c.bad, c.bad_noruns, c.bad_norule);
    tot.hulls += c.hulls; tot.fast += c.fast; tot.fast_with_runs += c.fast_with_runs; tot.refused += c.refused; tot.run_refused += c.run_refused;
    tot.bad += c.bad; tot.bad_noruns += c.bad_noruns; tot.bad_norule += c.bad_norule;
  }
  std::printf("family=all hulls=%ld fast=%ld fast_with_runs=%ld refused=%ld run_refused=%ld mismatches=%ld mismatches_without_runs=%ld mismatches_without_rule=%ld\n",
              tot.hulls, tot.fast, tot.fast_with_runs, tot.refused, tot.run_refused, tot.bad, tot.bad_noruns, tot.bad_norule);
  std::printf("hull_pair_sort_check ok\n");
  return 0;
}
