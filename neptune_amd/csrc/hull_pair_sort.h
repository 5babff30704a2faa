// hull_pair_sort.h — the sort of an INFLATED hull's corners in the grouped hull kernel (hull_group_kernel in geom_kernels.hip) as
// stacked pairs, with the rule for when the array it stores is the lexicographic sort of the corners.  Host and device:
// tests/cpp/hull_pair_sort_check.cpp runs the same code on the CPU against std::sort of the 64 corners.  Nothing in here multiplies,
// so there is nothing to contract; the pragmas are there all the same (the hulls are compared bit for bit with the CPU oracle).
//
// THE ELEMENTS.  The points of an inflated hull are the four corners (x +- dx, y +- dy) of np0 <= 16 control points.  The two corners
// on one side of a control point have the same first coordinate — the same double, from the same expression — so the input is
// P = 2 np0 <= 32 STACKED PAIRS: pair 2 c + side of control point c = (x, y) is
//     X = side ? x + dx : x - dx,   standing for the points (X, ylo) and (X, yhi),   ylo = y - dy,   yhi = y + dy
// — the expressions the kernel's corner build uses, so the same bits (pair_x, pair_ylo, pair_yhi).  A pair travels as (X, y).
//
// THE ARRAY.  The pairs are sorted by (X, y), lexicographically (pair_less: the comparison the full network makes on points).  A RUN
// is a maximal stretch of sorted pairs with equal X (==); run [s, t) of the pairs becomes the points 2 s .. 2 t - 1:
//     first the t - s points (X, ylo) in the run's order, then the t - s points (X, yhi) in the run's order            (pair_store)
// A run of one — the generic case — is (X, ylo), (X, yhi).  Longer runs are what committed trajectories bring every round: an
// interval whose end is a knot takes the next segment at length zero, whose control points are P * {1, 1, 1 - 4e-16, 1 - 7e-16} —
// one point twice and two more within ulps of it — and an agent at rest is nothing else.
//
// THE RULE.  The stored array is used when, for every hull of the wave,                (pair_sort_allowed, pair_key_bad, pair_run_ok)
//     cmax < 1e150   (cmax >= every |coordinate|: false for an infinity in x, y, dx or dy and for a NaN in dx or dy), dy > 0,
//     every one of the first P sorted keys X is a number below +inf (a NaN among the x would leave the pairs unsorted) and not a
//     zero (-0.0 and +0.0 would share a run, and which of two such points with one y comes first is the network's affair), and
//     in every run  ylo of its last pair < yhi of its first pair  (checked on the stored array: the point before the run's first
//     (X, yhi) against it; false for a NaN among the y).
// Otherwise the whole wave runs the full network (grp_bitonic<8, 64> on the 64 corners), which is always correct.
//
// WHY THE ARRAYS ARE EQUAL.  Under the rule every X is finite and every y a number, so (X, y) is totally ordered.  Within a run y
// ascends, and rounding is monotone, so ylo ascends (weakly) and so does yhi; with the last ylo below the first yhi the points of
// the run ascend in y.  Between runs X grows strictly.  So the stored array is sorted lexicographically, and it holds the same
// 4 np0 points as the corner array.  A lexicographically sorted arrangement of a multiset of points is unique as a sequence of
// VALUES, and points that are equal under == are the same bits here: no X is a zero; two equal ylo (or yhi) of a run come from one
// expression on equal y — y = -0.0 and +0.0 give the same sum with dy > 0 — and no ylo equals a yhi of its run.  So the array is the
// one the full network stores, element for element, and everything behind the sort — duplicate removal, skip flags, the chains, the
// output — sees the same bits.
// Without the runs — every pair expanded where it stands — a run of two stores (X, a), (X, b), (X, c), (X, d) with c < b: not sorted,
// and for a repeated control point the duplicate removal behind the sort no longer finds the copies side by side.
// tests/cpp/hull_pair_sort_check.cpp shows both: equality under the rule, differences without the runs and without the run test.
//
// THE NETWORK.  Bitonic over 8 lanes x 4 registers, element e = sub * 4 + r in register r of lane sub, like grp_bitonic: 15 steps, 9
// inside the lane.  Half the elements of the corners' network (21 steps over 8 registers), the same comparison.  Inside a lane one
// comparison decides an exchange (a descending run of the network swaps on "not less": equal elements change places, and equal
// elements are pads or equal pairs); across lanes both partners evaluate the same strict test, so that no element is lost or doubled.
// The steps are written once (pair_step_local, pair_step_cross) and driven by a `lanes` object that knows how to reach the partner
// lane: DPP moves and one ds_bpermute round in the kernel, plain arrays in the host check.
#pragma once

#if defined(__HIPCC__)
#define NEP_PAIR_HD __host__ __device__ __forceinline__
#else
#define NEP_PAIR_HD inline
#endif
#if defined(__clang__)
#define NEP_PAIR_UNROLL _Pragma("unroll")
#else
#define NEP_PAIR_UNROLL
#endif

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace nep {

constexpr int kPairJ = 4;                    // pairs per lane: 8 lanes x 4 = 32 pairs
constexpr double kPairMaxCoord = 1e150;      // coordinates from here on (and NaNs): the full network

NEP_PAIR_HD double pair_x(double x, double dx, int side) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return side ? x + dx : x - dx;
}
NEP_PAIR_HD double pair_ylo(double y, double dy) { return y - dy; }
NEP_PAIR_HD double pair_yhi(double y, double dy) { return y + dy; }
NEP_PAIR_HD bool pair_less(double ax, double ay, double bx, double by) { return (ax < bx) | ((ax == bx) & (ay < by)); }

// the part of the rule known before the network runs
NEP_PAIR_HD bool pair_sort_allowed(double cmax, double dy) { return (cmax < kPairMaxCoord) & (dy > 0.0); }
// the key at a real pair's sorted position is no number below +inf — some x is a NaN (the extremes cmax is made of are fmin / fmax
// results, which drop a NaN), the network has not sorted, and a pad or the NaN stands among the first P — or a zero
NEP_PAIR_HD bool pair_key_bad(double X) { return !(X < __builtin_huge_val()) | (X == 0.0); }
// the first (X, yhi) of a run against the point stored before it, the run's last (X, ylo)
NEP_PAIR_HD bool pair_run_ok(double ylo_last, double yhi_first) { return ylo_last < yhi_first; }

// One compare-exchange step at a distance inside the lane: registers r and r ^ JJ (JJ < J).
template <int J, int K_, int JJ> NEP_PAIR_HD void pair_step_local(double (&kx)[J], double (&ky)[J], int sub) {
  NEP_PAIR_UNROLL
  for (int r = 0; r < J; r++) {
    const int l = r ^ JJ;
    if (l > r) {
      const bool desc = ((sub * J + r) & K_) != 0;
      const bool sw = pair_less(kx[l], ky[l], kx[r], ky[r]) != desc;
      const double tx = kx[r], ty = ky[r];
      kx[r] = sw ? kx[l] : tx; ky[r] = sw ? ky[l] : ty;
      kx[l] = sw ? tx : kx[l]; ky[l] = sw ? ty : ky[l];
    }
  }
}
// ... and across lanes: ox, oy are the registers of lane sub ^ (JJ / J).  I keep the smaller element when I am the pair's lower index
// in an ascending run or the upper one in a descending run; both partners test "the would-be upper element < the would-be lower one".
template <int J, int K_, int JJ> NEP_PAIR_HD void pair_step_cross(double (&kx)[J], double (&ky)[J], int sub, const double (&ox)[J], const double (&oy)[J]) {
  constexpr int M = JJ / J;
  const bool asc = ((sub * J) & K_) == 0, lower = (sub & M) == 0;
  const bool want_min = lower == asc;
  NEP_PAIR_UNROLL
  for (int r = 0; r < J; r++) {
    const bool take = want_min ? pair_less(ox[r], oy[r], kx[r], ky[r]) : pair_less(kx[r], ky[r], ox[r], oy[r]);
    kx[r] = take ? ox[r] : kx[r]; ky[r] = take ? oy[r] : ky[r];
  }
}

// The network's steps in order: lanes.template step<K_, JJ>() for K_ = 2, 4 .. 8 J and JJ = K_ / 2 .. 1.
template <int J, int K_, int JJ, class Lanes> NEP_PAIR_HD void pair_bitonic_merge(Lanes& lanes) {
  lanes.template step<K_, JJ>();
  if constexpr (JJ > 1) pair_bitonic_merge<J, K_, JJ / 2>(lanes);
}
template <int J, int K_, class Lanes> NEP_PAIR_HD void pair_bitonic(Lanes& lanes) {
  if constexpr (K_ > 2) pair_bitonic<J, K_ / 2>(lanes);
  pair_bitonic_merge<J, K_, K_ / 2>(lanes);
}

// Runs.  `starts`: bit e set when sorted pair e begins a run (X differs from pair e - 1's; bit 0 always; the first pad, if there
// is one, begins a run too: +inf against a number).  -> s, the first pair of e's run, and t, the first pair behind it (<= 32).
NEP_PAIR_HD void pair_run_of(unsigned starts, int e, int& s, int& t) {
  const unsigned upto = starts & (0xffffffffu >> (31 - e));      // (bit 0 is set: never zero)
  const unsigned after = (starts >> e) >> 1;
#if defined(__HIP_DEVICE_COMPILE__)
  s = 31 - __clz((int)upto);
  t = after ? e + __ffs((int)after) : 32;
#else
  s = 31 - __builtin_clz(upto);
  t = after ? e + 1 + __builtin_ctz(after) : 32;
#endif
}

// The pair (X, y) at sorted position e of the run [s, t), as its two points of the sorted array sxy (interleaved x, y; 16-byte aligned)
NEP_PAIR_HD void pair_store(double* sxy, int e, int s, int t, double X, double y, double dy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double* lo = (double*)__builtin_assume_aligned(sxy + 2 * (s + e), 16);            // point 2 s + (e - s)
  double* hi = (double*)__builtin_assume_aligned(sxy + 2 * (t + e), 16);            // point 2 s + (t - s) + (e - s)
  lo[0] = X; lo[1] = pair_ylo(y, dy);
  hi[0] = X; hi[1] = pair_yhi(y, dy);
}
// where the run test of the run [s, t) reads: the y of the point before the run's first (X, yhi)
NEP_PAIR_HD int pair_run_check_at(int s, int t) { return 2 * (s + t) - 1; }

}  // namespace nep

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
