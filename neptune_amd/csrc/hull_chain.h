// hull_chain.h — the monotone chain walk of the grouped hull kernel (group_hull in geom_kernels.hip), with its rule for points that
// need not be visited at all.  Host and device: tests/cpp/hull_chain_check.cpp runs the same code on the CPU against the plain walk.
// No fused multiply-add anywhere in here (the hulls are compared bit for bit with the CPU oracle): contraction is switched off where
// there is a product to fuse, for clang (hipcc, device and host) and for GCC, whatever the command line says.
//
// THE RULE.  The chains walk the sorted (lexicographic), de-duplicated points s[0 .. m-1] of one hull: the corners (x +- dx, y +- dy)
// of 8-16 control points, so they come in runs of equal x.  Point j is FLAGGED when
//     s[j].x == s[j-1].x   and   fl(s[j].y - s[j-1].y) > thr                                  (chain_skip_flag; thr: chain_skip_threshold)
// and skipping is on for the hull (chain_skip_threshold's answer is finite, and no two consecutive x differ by less than
// kChainTinyGap: chain_gap_tiny).  The lower chain (ascending) does not visit a flagged j < m - 1; the upper chain (descending) does
// not visit a j > 0 whose successor j + 1 is flagged — its mirror image: the point right below its predecessor in the walk's order.
//
// WHY THE STACKS ARE THE SAME.  Lower chain; Q is any set of indices that holds every unflagged index and m - 1 (so: every run's first
// point), c is a flagged index < m - 1 outside Q.  The walk over Q + {c} leaves the stack the walk over Q leaves; adding the flagged
// points one by one, the masked walk (Q = the unflagged) equals the plain one (every index).
//  - Both walks are in the same state S when Q's points below c are done.  S's top is q, the largest index of Q below c; the run's
//    first point is in Q, so q is in c's run, and s[j-1] lies between: q.y <= s[j-1].y, every entry r of S in c's run has c.y - r.y
//    >= c.y - s[j-1].y =: g, and fl(g) > thr.
//  - Visiting c.  While the entry under the top is in the run as well, cross3 = 0 * (..) - (..) * 0 = 0 (every difference and product
//    is finite, see below): pop.  This leaves S' = [.., u, r1], r1 the lowest entry of the run, u (if any) with u.x < r1.x.
//      No u: one entry, c is pushed.
//      u:    cross3(u, r1, c) = fl(w A) - fl(B w),  w = fl(r1.x - u.x),  A = fl(c.y - u.y),  B = fl(r1.y - u.y).
//            w >= the smallest difference of consecutive x, >= kChainTinyGap (rounding is monotone); |A|, |B| <= 2 cmax (1 + 2^-53).
//            A - B >= g - 2 * 2^-53 * 2 cmax >= thr (1 - 2^-53) - 2^-51 cmax, and thr >= 2^-32 cmax: A - B >= thr / 2.
//            So the reals w A > w B differ by w (A - B) >= w thr / 2, which is both >= 2^-33 w cmax — 2^18 times the spacing of
//            doubles at w * 2 cmax — and >= kChainTinyGap * kChainMinThr / 2 = 5e-301 — 10^22 times the spacing of the subnormals.
//            Two reals further apart than twice the local spacing have two doubles between them: fl(w A) > fl(B w), cross3 > 0,
//            c pops nothing more and is pushed: [.., u, r1, c].
//  - The next visited point p (it exists: m - 1 is in Q) tests cross3(r1, c, p) first.
//      p in c's run:  0 * (..) - (..) * 0 = 0: c is popped.
//      p.x larger:    0 * (..) - fl(c.y - r1.y) * fl(p.x - r1.x); the first factor is >= thr (1 - 2^-53), the second
//                     >= kChainTinyGap, their product >= 9e-301 > 0: cross3 < 0, c is popped.
//    p now stands before S' with its test cross3(u, r1, p) (or one entry, no test).
//  - The walk over Q visits p in state S.  While the entry under the top is in the run: cross3 = 0 (p in the run) or
//    0 * (..) - fl(b.y - a.y) * fl(p.x - a.x) with both factors > 0, a product >= +0: cross3 <= 0 either way, pop.  That leaves p before
//    S' with the test cross3(u, r1, p): the same operands, the same state, and the walks go on together.
//  - Finite: chain_skip_threshold switches skipping off unless cmax < kChainMaxCoord = 1e150 (false for an infinity or a NaN too), so
//    every difference is below 2e150 and every product below 4e300.  Not skipping is always correct.
//  The upper chain is the same argument turned by 180 degrees: descending walk, u.x > r1.x, w < 0, c below r1, A < B, w A > w B.
//  Without the gap condition the argument breaks where it should: two points of a run an ulp apart give A == B against a far u,
//  cross3 = 0, and the plain walk pops r1 where the masked walk keeps it (the constant segments' clusters: P * {1, 1, 1 - 4e-16,
//  1 - 7e-16}).  tests/cpp/hull_chain_check.cpp shows both: no mismatch with the gap, mismatches without.
#pragma once

#if defined(__HIPCC__)
#define NEP_CHAIN_HD __host__ __device__ __forceinline__
#else
#define NEP_CHAIN_HD inline
#endif

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace nep {

constexpr double kChainRelGap = 1.0 / 4294967296.0;      // 2^-32: thr >= 2^-32 * (largest coordinate magnitude)
constexpr double kChainMinThr = 1e-150;                  // thr's floor, and
constexpr double kChainTinyGap = 1e-150;                 // the smallest difference of consecutive x with which a hull skips: their product is a normal number
constexpr double kChainMaxCoord = 1e150;                 // coordinates from here on: products could overflow, no skipping

NEP_CHAIN_HD double chain_cross3(double ox, double oy, double ax, double ay, double bx, double by) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox);
}

// The gap a flagged point keeps to its predecessor, from cmax >= |every coordinate of the hull's points| (a few ulps short is fine: the
// proof has a factor 2^18 to spare).  +inf (nothing is ever flagged) when cmax is not below kChainMaxCoord — infinities and NaNs included.
NEP_CHAIN_HD double chain_skip_threshold(double cmax) {
  if (!(cmax < kChainMaxCoord)) return __builtin_huge_val();
  const double t = cmax * kChainRelGap;
  return t > kChainMinThr ? t : kChainMinThr;
}
// (x, y) against its predecessor (xp, yp) in the sorted array
NEP_CHAIN_HD bool chain_skip_flag(double x, double y, double xp, double yp, double thr) { return (x == xp) & (y - yp > thr); }
// consecutive x closer than the proof allows: a hull with one such pair skips nothing
NEP_CHAIN_HD bool chain_gap_tiny(double x, double xp) { const double d = x - xp; return (d > 0.0) & (d < kChainTinyGap); }

NEP_CHAIN_HD int chain_top_bit(unsigned long long v) {       // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 63 - __clzll((long long)v);
#else
  return 63 - __builtin_clzll(v);
#endif
}
NEP_CHAIN_HD int chain_low_bit(unsigned long long v) {       // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((unsigned long long)v) - 1;
#else
  return __builtin_ctzll(v);
#endif
}
NEP_CHAIN_HD unsigned long long chain_reverse(unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __brevll(v);
#else
  v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
  v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
  v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
  return __builtin_bswap64(v);
#endif
}

// What a chain visits, as a mask in its PUSH order (bit i = the i-th point of the plain walk: sorted index i for the lower chain,
// m - 1 - i for the upper one), from the flags over the sorted indices.  2 <= m <= 64.
NEP_CHAIN_HD unsigned long long chain_todo(unsigned long long flags, int m, bool lower) {
  const unsigned long long all = m >= 64 ? ~0ull : (1ull << m) - 1ull;
  flags &= all;
  if (lower) return all & ~(flags & ~(1ull << (m - 1)));                  // never the last point
  // upper: sorted index j is skipped iff j + 1 is flagged, never j = 0; sorted index j is push index m - 1 - j
  const unsigned long long skip = (flags >> 1) & ~1ull;
  return all & ~(chain_reverse(skip) >> (64 - m));
}

// One chain over the sorted points sxy[2 j], sxy[2 j + 1] (j < m, 2 <= m <= 64; sxy aligned to 16 bytes), visiting the set bits of `todo` from the lowest up.
// Returns the stack as a mask in push order.  With todo = every index below m this is the plain walk.
// The stack is a subsequence of the sorted points: push = set a bit, pop = clear the top one.  The two top indices travel in registers,
// so that a pop clears a known bit and finds the entry under the new top with ONE 64-bit count-leading-zeros (three of them, each five
// instructions, when every pop searched the mask for the top, the new top and the entry under it: 0.1006 -> 0.0958 ms per 65 536
// hulls; the kernel is bound by the instructions its waves issue).  A `continue` on a skipped index would
// save nothing: the sixteen chain lanes of a wave run in lock-step and skip different indices.  Each lane takes the lowest set bit
// of its own to-do mask instead, and the wave's loop is as long as the longest list.
NEP_CHAIN_HD unsigned long long chain_walk(const double* sxy, int m, bool lower, unsigned long long todo) {
  unsigned long long mask = 0;
  int kc = 0;
  int i1 = 0, i2 = 0;                      // push indices of the top entry and of the one under it (valid from kc = 1 / kc = 2 on)
  double ax = 0, ay = 0, bx = 0, by = 0;   // the two top entries
  while (todo) {
    const int i = chain_low_bit(todo);
    todo &= todo - 1ull;
    const double* c = (const double*)__builtin_assume_aligned(sxy + 2 * (lower ? i : m - 1 - i), 16);      // (one 16-byte read)
    const double x = c[0], y = c[1];
    while (kc >= 2 && chain_cross3(ax, ay, bx, by, x, y) <= 0.0) {
      mask &= ~(1ull << i1);
      kc--; bx = ax; by = ay; i1 = i2;
      if (kc >= 2) {
        i2 = chain_top_bit(mask & ((1ull << i2) - 1ull));      // the highest entry under the new top
        const double* a = (const double*)__builtin_assume_aligned(sxy + 2 * (lower ? i2 : m - 1 - i2), 16);
        ax = a[0]; ay = a[1];
      }
    }
    mask |= 1ull << i; kc++;
    ax = bx; ay = by; bx = x; by = y;
    i2 = i1; i1 = i;
  }
  return mask;
}

}  // namespace nep

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
