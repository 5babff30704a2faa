// mtlp_common.h — the rule set of the MTLP comparator (include/neptune_mtlp.h), once, for the host form (mtlp_host.cpp) and the
// device form (mtlp_kernels.hip): mtlp::solveMultiTetherLinearPath and mtlp::AstarGraphSearch / AstarGetSucc / getPath
// (neptune/src/solveMultiLinearPath.cpp), with the CGAL tests of cgal_utils.cpp as exact predicates of our own.  Both translation
// units are compiled with -ffp-contract=off and agree on every output byte.
//
// Predicates.  Three signs carry everything: orient2 (a 2 x 2 determinant of differences), orient3 (3 x 3) and the four signs of
// the ball/segment test.  Each is evaluated in double together with M, the same expression with every product replaced by its
// absolute value.  At most K = 8 roundings lie on any path from an input to the value, so with e = 2^-53
//     |fl(S) - S| <= ((1 + e)^K - 1) sum|monomial|   and   fl(M) >= (1 - e)^K sum|monomial|,
// hence |fl(S) - S| <= ((1 + e)^8 - 1) / (1 - e)^8 M < 9 e M < 2^-49 M (exactly representable: a power of two times M; nothing
// underflows in the domain, where every non-zero monomial is at least 2^-240).  |fl(S)| > 2^-49 M decides the sign; otherwise the
// sign is that of the same polynomial in two's-complement integers of 192 (degree 2), 256 (degree 3) or 384 bits (degree 4) on
// the inputs times 2^60 (the radius squared times 2^120).  With |x| <= 2^20 a scaled input is below 2^80, a difference below 2^81,
// orient3 below 6 * 2^243, the degree-4 sign below 2^330: each fits its width, so the wrapped arithmetic is exact.
//
// One function, search<Ex>, is a whole search.  Ex is how an expansion's dense block — (26 neighbours) x (cable lines), each entry
// a segment/triangle test and a ball/segment test — is spread: the host runs it one entry at a time, the device 64 at a time on the
// lanes of one wave, and a ballot gathers the verdicts.  The heap, the node table and the commit are wave-uniform: every lane runs
// them on the same values and stores the same values to the same addresses.
#ifndef NEP_MTLP_COMMON_H_
#define NEP_MTLP_COMMON_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/neptune_mtlp.h"

#if defined(__HIPCC__)
#define MT_HD __host__ __device__ inline
#else
#define MT_HD inline
#endif
// the predicates are called from dozens of places (a triangle/triangle test alone is six segment/triangle tests of up to eight signs
// each): as real calls, not inlined copies, they compile in seconds instead of minutes, on the device too
#define MT_NI MT_HD __attribute__((noinline))

namespace nep_mtlp_impl {

struct Par {
  double res, inv_res, xl, yl, zl, r2, bias;
  int glx, gly, glz, n, max_nodes, max_pops, path_cap, hash_size;
};
// 32 bytes.  link: cameFrom + 1 in the low 30 bits (0: none), bit 30 set once the node is closed
struct Node { int32_t ix, iy, iz, link; double g, f; };
#define MT_CLOSED (1 << 30)
struct Work { Node* nodes; int32_t* heap; int32_t* hash; double* lines; };

MT_HD size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
MT_HD size_t work_bytes(const Par& p) {
  return up16((size_t)p.max_nodes * sizeof(Node)) + up16((size_t)p.max_nodes * 4) + up16((size_t)p.hash_size * 4) + up16((size_t)p.n * 6 * 8);
}
MT_HD Work carve(char* b, const Par& p) {
  Work w;
  w.nodes = (Node*)b; b += up16((size_t)p.max_nodes * sizeof(Node));
  w.heap = (int32_t*)b; b += up16((size_t)p.max_nodes * 4);
  w.hash = (int32_t*)b; b += up16((size_t)p.hash_size * 4);
  w.lines = (double*)b;
  return w;
}

// ---- the domain ------------------------------------------------------------------------------------------------------------------
MT_HD bool multiple_of_2m60(double x) {      // of a finite x
  if (fabs(x) >= 0.00390625) return true;      // ulp(2^-8) = 2^-60
  const double s = x * 1152921504606846976.0;      // exact: a power of two, |s| < 2^52
  return s == floor(s);
}
MT_HD bool in_domain(double x) { return fabs(x) <= NEP_MTLP_MAX_COORD && multiple_of_2m60(x); }      // (a NaN fails the comparison)

// ---- fixed-width integers: N words of 32 bits, two's complement, arithmetic modulo 2^(32 N) -----------------------------------------
template <int N> struct Big { uint32_t w[N]; };
template <int N> MT_HD Big<N> big_neg(const Big<N>& a) {
  Big<N> r; uint64_t c = 1;
  for (int i = 0; i < N; i++) { c += (uint64_t)(uint32_t)~a.w[i]; r.w[i] = (uint32_t)c; c >>= 32; }
  return r;
}
// x * 2^scale of a double for which that is an integer below 2^(32 N - 34) in magnitude
template <int N> MT_HD Big<N> big_from(double x, int scale) {
  Big<N> r;
  for (int i = 0; i < N; i++) r.w[i] = 0;
  uint64_t bits; __builtin_memcpy(&bits, &x, 8);
  int e = (int)((bits >> 52) & 0x7ff);
  uint64_t m = bits & (((uint64_t)1 << 52) - 1);
  if (e == 0) e = 1; else m |= (uint64_t)1 << 52;
  int sh = e - 1075 + scale;      // |x| = m 2^(e - 1075)
  if (sh < 0) { m = sh > -64 ? m >> (-sh) : 0; sh = 0; }      // the bits dropped are zero in the domain
  const int wi = sh >> 5, b = sh & 31;
  const uint64_t t0 = (uint64_t)(uint32_t)m << b, t1 = (m >> 32) << b;
  const uint64_t acc = (t0 >> 32) + t1;
  if (wi < N) r.w[wi] = (uint32_t)t0;
  if (wi + 1 < N) r.w[wi + 1] = (uint32_t)acc;
  if (wi + 2 < N) r.w[wi + 2] = (uint32_t)(acc >> 32);
  return bits >> 63 ? big_neg(r) : r;
}
template <int N> MT_HD Big<N> big_add(const Big<N>& a, const Big<N>& b) {
  Big<N> r; uint64_t c = 0;
  for (int i = 0; i < N; i++) { c += (uint64_t)a.w[i] + b.w[i]; r.w[i] = (uint32_t)c; c >>= 32; }
  return r;
}
template <int N> MT_HD Big<N> big_sub(const Big<N>& a, const Big<N>& b) { return big_add(a, big_neg(b)); }
template <int N> MT_HD Big<N> big_mul(const Big<N>& a, const Big<N>& b) {
  Big<N> r;
  for (int i = 0; i < N; i++) r.w[i] = 0;
  for (int i = 0; i < N; i++) {
    uint64_t c = 0;
    for (int j = 0; i + j < N; j++) { c += (uint64_t)a.w[i] * b.w[j] + r.w[i + j]; r.w[i + j] = (uint32_t)c; c >>= 32; }
  }
  return r;
}
template <int N> MT_HD int big_sign(const Big<N>& a) {
  if (a.w[N - 1] >> 31) return -1;
  for (int i = 0; i < N; i++) if (a.w[i]) return 1;
  return 0;
}

#define MT_FILTER 1.7763568394002505e-15 /* 2^-49 */
MT_HD int filtered(double s, double m) { const double b = MT_FILTER * m; return s > b ? 1 : (s < -b ? -1 : 0); }

// sign of | a[X]-c[X]  a[Y]-c[Y] ; b[X]-c[X]  b[Y]-c[Y] |
MT_NI int orient2_exact(const double* a, const double* b, const double* c, int X, int Y) {
  typedef Big<6> B;
  const B cx = big_from<6>(c[X], 60), cy = big_from<6>(c[Y], 60);
  const B Ax = big_sub(big_from<6>(a[X], 60), cx), Ay = big_sub(big_from<6>(a[Y], 60), cy);
  const B Bx = big_sub(big_from<6>(b[X], 60), cx), By = big_sub(big_from<6>(b[Y], 60), cy);
  return big_sign(big_sub(big_mul(Ax, By), big_mul(Ay, Bx)));
}
MT_HD int orient2(const double* a, const double* b, const double* c, int X, int Y, int& nex) {
  const double acx = a[X] - c[X], bcx = b[X] - c[X], acy = a[Y] - c[Y], bcy = b[Y] - c[Y];
  const double l = acx * bcy, r = acy * bcx;
  const int s = filtered(l - r, fabs(l) + fabs(r));
  if (s) return s;
  nex++;
  return orient2_exact(a, b, c, X, Y);
}
// sign of the determinant of (a - d, b - d, c - d)
MT_NI int orient3_exact(const double* a, const double* b, const double* c, const double* d) {
  typedef Big<8> B;
  B A[3], Bv[3], C[3];
  for (int k = 0; k < 3; k++) {
    const B dk = big_from<8>(d[k], 60);
    A[k] = big_sub(big_from<8>(a[k], 60), dk); Bv[k] = big_sub(big_from<8>(b[k], 60), dk); C[k] = big_sub(big_from<8>(c[k], 60), dk);
  }
  const B t1 = big_mul(A[0], big_sub(big_mul(Bv[1], C[2]), big_mul(Bv[2], C[1])));
  const B t2 = big_mul(Bv[0], big_sub(big_mul(C[1], A[2]), big_mul(C[2], A[1])));
  const B t3 = big_mul(C[0], big_sub(big_mul(A[1], Bv[2]), big_mul(A[2], Bv[1])));
  return big_sign(big_add(big_add(t1, t2), t3));
}
MT_HD int orient3(const double* a, const double* b, const double* c, const double* d, int& nex) {
  const double adx = a[0] - d[0], ady = a[1] - d[1], adz = a[2] - d[2];
  const double bdx = b[0] - d[0], bdy = b[1] - d[1], bdz = b[2] - d[2];
  const double cdx = c[0] - d[0], cdy = c[1] - d[1], cdz = c[2] - d[2];
  const double p1 = bdy * cdz, p2 = bdz * cdy, p3 = cdy * adz, p4 = cdz * ady, p5 = ady * bdz, p6 = adz * bdy;
  const double det = adx * (p1 - p2) + bdx * (p3 - p4) + cdx * (p5 - p6);
  const double m = fabs(adx) * (fabs(p1) + fabs(p2)) + fabs(bdx) * (fabs(p3) + fabs(p4)) + fabs(cdx) * (fabs(p5) + fabs(p6));
  const int s = filtered(det, m);
  if (s) return s;
  nex++;
  return orient3_exact(a, b, c, d);
}

// ---- closed segments in the plane of coordinates (X, Y): CGAL::do_intersect(Segment_2, Segment_2) -----------------------------------
MT_HD bool in_box2(const double* p, const double* q, const double* r, int X, int Y) {
  return (p[X] < q[X] ? p[X] <= r[X] && r[X] <= q[X] : q[X] <= r[X] && r[X] <= p[X]) &&
         (p[Y] < q[Y] ? p[Y] <= r[Y] && r[Y] <= q[Y] : q[Y] <= r[Y] && r[Y] <= p[Y]);
}
MT_NI bool seg_seg2(const double* p, const double* q, const double* u, const double* v, int X, int Y, int& nex) {
  const int d1 = orient2(p, q, u, X, Y, nex), d2 = orient2(p, q, v, X, Y, nex), d3 = orient2(u, v, p, X, Y, nex), d4 = orient2(u, v, q, X, Y, nex);
  if (d1 * d2 < 0 && d3 * d4 < 0) return true;
  if (d1 == 0 && in_box2(p, q, u, X, Y)) return true;
  if (d2 == 0 && in_box2(p, q, v, X, Y)) return true;
  if (d3 == 0 && in_box2(u, v, p, X, Y)) return true;
  if (d4 == 0 && in_box2(u, v, q, X, Y)) return true;
  return false;
}
// closed segments in space (either may be a point): coplanar, and meeting in all three coordinate projections — a projection
// along an axis that the points' plane (or line) does not contain is one to one on it, the other projections are necessary
MT_NI bool seg_seg3(const double* p, const double* q, const double* u, const double* v, int& nex) {
  if (orient3(p, q, u, v, nex) != 0) return false;
  return seg_seg2(p, q, u, v, 0, 1, nex) && seg_seg2(p, q, u, v, 1, 2, nex) && seg_seg2(p, q, u, v, 2, 0, nex);
}
MT_HD bool collinear3(const double* a, const double* b, const double* c, int& nex) {
  return orient2(a, b, c, 0, 1, nex) == 0 && orient2(a, b, c, 1, 2, nex) == 0 && orient2(a, b, c, 2, 0, nex) == 0;
}
// p, in the plane of the triangle: in the closed triangle?  false for a collinear triangle (its edges are tested as segments)
MT_NI bool in_tri_coplanar(const double* a, const double* b, const double* c, const double* p, int& nex) {
  bool any = false;
  for (int k = 0; k < 3; k++) {
    const int X = k, Y = (k + 1) % 3;
    if (orient2(a, b, c, X, Y, nex) == 0) continue;
    any = true;
    const int s1 = orient2(a, b, p, X, Y, nex), s2 = orient2(b, c, p, X, Y, nex), s3 = orient2(c, a, p, X, Y, nex);
    if (!((s1 >= 0 && s2 >= 0 && s3 >= 0) || (s1 <= 0 && s2 <= 0 && s3 <= 0))) return false;
  }
  return any;
}
// CGAL::do_intersect(Segment_3, Triangle_3) as point sets: the closed segment p q against the closed hull of a, b, c
MT_NI bool seg_tri(const double* p, const double* q, const double* a, const double* b, const double* c, int& nex) {
  const int sp = orient3(a, b, c, p, nex), sq = orient3(a, b, c, q, nex);
  if (sp * sq > 0) return false;
  if (sp != 0 || sq != 0) {      // a proper triangle, and the segment meets its plane in one point
    const int s1 = orient3(p, q, a, b, nex), s2 = orient3(p, q, b, c, nex), s3 = orient3(p, q, c, a, nex);
    return (s1 >= 0 && s2 >= 0 && s3 >= 0) || (s1 <= 0 && s2 <= 0 && s3 <= 0);
  }
  // the segment lies in the triangle's plane, or the triangle is collinear (then its hull is the union of its edges)
  return seg_seg3(p, q, a, b, nex) || seg_seg3(p, q, b, c, nex) || seg_seg3(p, q, c, a, nex) || in_tri_coplanar(a, b, c, p, nex);
}
// CGAL::do_intersect(Triangle_3, Triangle_3): six segment/triangle tests.  A triangle is T[0], T[1], T[2], three doubles each
MT_HD bool tri_tri(const double* const* A, const double* const* B, int& nex) {
  for (int k = 0; k < 3; k++) if (seg_tri(A[k], A[(k + 1) % 3], B[0], B[1], B[2], nex)) return true;
  for (int k = 0; k < 3; k++) if (seg_tri(B[k], B[(k + 1) % 3], A[0], A[1], A[2], nex)) return true;
  return false;
}

// ---- the ball of squared radius r2 about c against the closed segment p q: bit 0 they meet, bit 1 the segment is wholly inside -------
// which 0: |p - c|^2 - r2   1: |q - c|^2 - r2   2: t = (c - p).(q - p)   3: t - |q - p|^2   4: |c - p|^2 |q - p|^2 - t^2 - r2 |q - p|^2
MT_NI int ball_sign_exact(const double* c, double r2, const double* p, const double* q, int which) {
  typedef Big<12> B;
  B A, L, T, R = big_from<12>(r2, 120);
  for (int i = 0; i < 12; i++) A.w[i] = L.w[i] = T.w[i] = 0;
  const double* e = which == 1 ? q : p;
  for (int k = 0; k < 3; k++) {
    const B ck = big_from<12>(c[k], 60);
    const B ec = big_sub(ck, big_from<12>(e[k], 60)), pq = big_sub(big_from<12>(q[k], 60), big_from<12>(p[k], 60));
    A = big_add(A, big_mul(ec, ec)); L = big_add(L, big_mul(pq, pq)); T = big_add(T, big_mul(ec, pq));
  }
  if (which <= 1) return big_sign(big_sub(A, R));
  if (which == 2) return big_sign(T);
  if (which == 3) return big_sign(big_sub(T, L));
  return big_sign(big_sub(big_sub(big_mul(A, L), big_mul(T, T)), big_mul(R, L)));
}
MT_HD int ball_seg(const double* c, double r2, const double* p, const double* q, int& nex) {
  const double px = c[0] - p[0], py = c[1] - p[1], pz = c[2] - p[2], qx = c[0] - q[0], qy = c[1] - q[1], qz = c[2] - q[2];
  const double A = px * px + py * py + pz * pz, Aq = qx * qx + qy * qy + qz * qz;
  int sp = filtered(A - r2, A + r2), sq = filtered(Aq - r2, Aq + r2);
  if (!sp) { nex++; sp = ball_sign_exact(c, r2, p, q, 0); }
  if (!sq) { nex++; sq = ball_sign_exact(c, r2, p, q, 1); }
  if (sp < 0 && sq < 0) return 3;
  if (sp <= 0 || sq <= 0) return 1;
  // both ends outside: the closest point is interior when 0 < t < |q - p|^2
  const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
  const double t1 = px * dx, t2 = py * dy, t3 = pz * dz, t = t1 + t2 + t3, tm = fabs(t1) + fabs(t2) + fabs(t3);
  const double L = dx * dx + dy * dy + dz * dz;
  int st = filtered(t, tm);
  if (!st) { nex++; st = ball_sign_exact(c, r2, p, q, 2); }
  if (st <= 0) return 0;
  int su = filtered(t - L, tm + L);
  if (!su) { nex++; su = ball_sign_exact(c, r2, p, q, 3); }
  if (su >= 0) return 0;
  const double al = A * L, tt = t * t, rl = r2 * L;
  int s4 = filtered(al - tt - rl, al + tm * tm + rl);
  if (!s4) { nex++; s4 = ball_sign_exact(c, r2, p, q, 4); }
  return s4 <= 0 ? 1 : 0;
}

// ---- the order graph (solveMultiLinearPath.cpp:31-98) ---------------------------------------------------------------------------------
// what the visit (i, j) sets: bit 0 graph(i, j), bit 1 graph(j, i).  bases [N][3], sg [N][2][3]
MT_NI int graph_visit(const double* bases, const double* sg, int i, int j) {
  int nex = 0;
  const double* A[3] = {bases + 3 * i, sg + 6 * i, sg + 6 * i + 3};
  const double* B[3] = {bases + 3 * j, sg + 6 * j, sg + 6 * j + 3};
  if (!tri_tri(A, B, nex)) return 3;
  const bool baseline = seg_seg2(A[1], A[2], B[1], B[2], 0, 1, nex);
  const bool sA = seg_tri(A[0], A[1], B[0], B[1], B[2], nex), eA = seg_tri(A[0], A[2], B[0], B[1], B[2], nex);      // anchor_start_A, anchor_end_A against triB
  const bool sB = seg_tri(B[0], B[1], A[0], A[1], A[2], nex), eB = seg_tri(B[0], B[2], A[0], A[1], A[2], nex);
  if (!baseline) {
    if ((sA && eA) || (sB && eB)) return 0;      // type 1
    else if ((sA && sB) || (eB && eA)) return 0;      // type 2
    else if (sA && eB) return 1;      // type 3, A before B
    else if (sB && eA) return 2;
    return 0;
  }
  if (eA) return 2;
  else if (eB) return 1;
  else if (sA) return 1;
  else if (sB) return 2;
  return 0;
}
MT_HD bool run_in_domain(const double* bases, const double* sg, int n) {
  bool ok = true;
  for (int k = 0; k < 3 * n; k++) ok = ok && in_domain(bases[k]);
  for (int k = 0; k < 6 * n; k++) ok = ok && in_domain(sg[k]);
  return ok;
}
// graph(i, j): the identity, OR what the visits (i, j) and (j, i) set on it
MT_HD int graph_entry(const double* bases, const double* sg, int i, int j) {
  return (i == j) | (graph_visit(bases, sg, i, j) & 1) | (graph_visit(bases, sg, j, i) >> 1 & 1);
}

// ---- the search (:523-706) --------------------------------------------------------------------------------------------------------------
MT_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
MT_HD int to_int(double v) {      // int(v) of a finite double; saturating where C++ leaves it undefined
  if (!(v > -2147483648.0)) return -2147483647 - 1;
  if (!(v < 2147483647.0)) return 2147483647;
  return (int)v;
}
MT_HD int ctz64(uint64_t m) { return __builtin_ctzll(m); }
MT_HD int popc64(uint64_t m) { return __builtin_popcountll(m); }

struct SerialEx {
  static constexpr int W = 1;
  MT_HD int lane() const { return 0; }
  MT_HD uint64_t ballot(bool p) const { return p ? 1u : 0u; }
  MT_HD void sync() const {}
};

struct Searcher {
  Par p; Work w;
  double start[3];
  int gx, gy, gz;

  MT_HD void centre(int ix, int iy, int iz, double* pt) const {      // gridIndex2coord
    pt[0] = ((double)ix + 0.5) * p.res + p.xl; pt[1] = ((double)iy + 0.5) * p.res + p.yl; pt[2] = ((double)iz + 0.5) * p.res + p.zl;
  }
  MT_HD void coord(int v, double* pt) const {      // GridNode::coord: the start keeps its un-rounded point
    if (v == 0) { pt[0] = start[0]; pt[1] = start[1]; pt[2] = start[2]; } else centre(w.nodes[v].ix, w.nodes[v].iy, w.nodes[v].iz, pt);
  }
  MT_HD void index_of(const double* pt, int* ix, int* iy, int* iz) const {      // coord2gridIndex
    *ix = clampi(to_int((pt[0] - p.xl) * p.inv_res), 0, p.glx - 1);
    *iy = clampi(to_int((pt[1] - p.yl) * p.inv_res), 0, p.gly - 1);
    *iz = clampi(to_int((pt[2] - p.zl) * p.inv_res), 0, p.glz - 1);
  }
  MT_HD double heu(int ix, int iy, int iz) const {      // getHeu: Vector3d::lpNorm<2> of the index difference
    const double dx = (double)ix - (double)gx, dy = (double)iy - (double)gy, dz = (double)iz - (double)gz;
    return sqrt(dx * dx + (dy * dy + dz * dz));
  }
  MT_HD bool comp(int l, int r) const {      // CompareCost
    const Node& L = w.nodes[l]; const Node& R = w.nodes[r];
    if (fabs(L.f - R.f) < 1e-5) return L.f - L.g > R.f - R.g;
    return L.f > R.f;
  }
  // std::push_heap's __push_heap and std::pop_heap's __adjust_heap (libstdc++ bits/stl_heap.h), as hastar_common.h has them
  MT_HD void push_heap_(int hole, int top, int value) const {
    int parent = (hole - 1) / 2;
    while (hole > top && comp(w.heap[parent], value)) { w.heap[hole] = w.heap[parent]; hole = parent; parent = (hole - 1) / 2; }
    w.heap[hole] = value;
  }
  MT_HD void heap_push(int& n, int value) const { w.heap[n] = value; n++; push_heap_(n - 1, 0, value); }
  MT_HD int heap_pop(int& n) const {
    const int top = w.heap[0];
    if (n > 1) {
      const int value = w.heap[n - 1];
      w.heap[n - 1] = w.heap[0];
      const int len = n - 1;
      int hole = 0, second = 0;
      while (second < (len - 1) / 2) {
        second = 2 * (second + 1);
        if (comp(w.heap[second], w.heap[second - 1])) second--;
        w.heap[hole] = w.heap[second]; hole = second;
      }
      if ((len & 1) == 0 && second == (len - 2) / 2) { second = 2 * (second + 1); w.heap[hole] = w.heap[second - 1]; hole = second - 1; }
      push_heap_(hole, 0, value);
    }
    n--;
    return top;
  }
  // the node table: open addressing, exact match on the three indices
  MT_HD uint32_t slot_of(int ix, int iy, int iz) const {
    uint32_t h = (uint32_t)ix * 0x9e3779b1u ^ ((uint32_t)iy * 0x85ebca77u + 0x7f4a7c15u) ^ ((uint32_t)iz * 0xc2b2ae3du);
    h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
    return h & (uint32_t)(p.hash_size - 1);
  }
  MT_HD int find(int ix, int iy, int iz) const {
    for (uint32_t s = slot_of(ix, iy, iz);; s = (s + 1) & (uint32_t)(p.hash_size - 1)) {
      const int e = w.hash[s];
      if (e == 0) return -1;
      const Node& nd = w.nodes[e - 1];
      if (nd.ix == ix && nd.iy == iy && nd.iz == iz) return e - 1;
    }
  }
  MT_HD void insert(int ix, int iy, int iz, int v) const {
    uint32_t s = slot_of(ix, iy, iz);
    while (w.hash[s] != 0) s = (s + 1) & (uint32_t)(p.hash_size - 1);
    w.hash[s] = v + 1;
  }
};

// robot `me` of one run.  graph: the run's [N][N], already written.  run_ok: the run's inputs lie in the domain
template <class Ex>
MT_HD void search(const Ex& ex, const Par& p, const double* bases, const double* sg, const int32_t* graph, int me, bool run_ok,
                  char* work_mem, nep_mtlp_result* res_out, double* path) {
  nep_mtlp_result res;
  res.status = -1; res.n_path = 0; res.nodes_used = 0; res.pops = 0; res.n_updates = 0; res.flags = 0; res.n_degenerate = 0; res.n_ball_only = 0; res.g_cells = 0.0;
  Searcher S; S.p = p; S.w = carve(work_mem, p);
  const Work& w = S.w;
  int terminal = -1;
  double goal_c[3] = {0, 0, 0};
  if (!run_ok) res.flags |= NEP_MTLP_FLAG_STATE;
  else {
    for (int i = ex.lane(); i < p.hash_size; i += Ex::W) w.hash[i] = 0;
    // the cable lines of robot `me` (:169-194; the order of the robots is 0 .. N-1)
    int nl = 0;
    for (int j = 0; j < p.n; j++) {
      if (j == me) continue;
      const double* pt;
      if (j < me) { if (graph[j * p.n + me] == 1) continue; pt = sg + 6 * j + 3; } else pt = sg + 6 * j;
      for (int k = 0; k < 3; k++) { w.lines[6 * nl + k] = bases[3 * j + k]; w.lines[6 * nl + 3 + k] = pt[k]; }
      nl++;
    }
    ex.sync();
    const double* base = bases + 3 * me;
    const double* start_pt = sg + 6 * me; const double* goal_pt = sg + 6 * me + 3;
    for (int k = 0; k < 3; k++) S.start[k] = start_pt[k];
    int sx, sy, sz; S.index_of(start_pt, &sx, &sy, &sz); S.index_of(goal_pt, &S.gx, &S.gy, &S.gz);
    const double goal_height = goal_pt[2];
    S.centre(S.gx, S.gy, S.gz, goal_c);
    int heap_n = 0, used = 1;
    { Node& s = w.nodes[0]; s.ix = sx; s.iy = sy; s.iz = sz; s.link = 0; s.g = 0; s.f = p.bias * S.heu(sx, sy, sz); }
    S.heap_push(heap_n, 0);
    S.insert(sx, sy, sz, 0);
    const double cost1[4] = {0.0, 1.0, (double)1.41421356237f, (double)1.73205080757f};      // offsetIndex.cast<float>().lpNorm<2>()
    for (;;) {
      if (heap_n == 0) { res.status = -1; break; }
      if (res.pops >= p.max_pops) { res.status = 0; break; }
      const int cur = S.heap_pop(heap_n);
      res.pops++;
      w.nodes[cur].link |= MT_CLOSED;
      const Node C = w.nodes[cur];
      if (C.ix == S.gx && C.iy == S.gy && C.iz == S.gz) { res.status = 1; terminal = cur; break; }
      // ---- AstarGetSucc: neighbour m = 9 (i + 1) + 3 (j + 1) + (k + 1) ----
      double pk[3]; S.coord(cur, pk);
      uint32_t skip = 1u << 13, blocked = 0;
      for (int k = -1; k <= 1; k++) {
        const double z = ((double)(C.iz + k) + 0.5) * p.res + p.zl;
        if (z > goal_height) skip |= 0x1249249u << (k + 1);      // every m with m % 3 == k + 1
      }
      {      // collinear triangles (base, neighbour centre, current point), one neighbour per lane
        for (int b0 = 0; b0 < 27; b0 += Ex::W) {
          const int m = b0 + ex.lane();
          bool deg = false;
          if (m < 27 && !(skip >> m & 1)) {
            double c[3]; S.centre(C.ix + m / 9 - 1, C.iy + m / 3 % 3 - 1, C.iz + m % 3 - 1, c);
            int nex = 0; deg = collinear3(base, c, pk, nex);
          }
          res.n_degenerate += popc64(ex.ballot(deg));
        }
      }
      const int items = 27 * nl;
      for (int b0 = 0; b0 < items; b0 += Ex::W) {
        const int it = b0 + ex.lane();
        bool hit = false, inside = false;
        if (it < items) {
          const int m = it / nl, c_ = it - m * nl;
          if (!(skip >> m & 1)) {
            double c[3]; S.centre(C.ix + m / 9 - 1, C.iy + m / 3 % 3 - 1, C.iz + m % 3 - 1, c);
            const double* ln = w.lines + 6 * c_;
            int nex = 0;
            const bool tri = seg_tri(ln, ln + 3, base, c, pk, nex);
            const int bl = ball_seg(c, p.r2, ln + 3, ln, nex);
            hit = tri || (bl & 1); inside = bl == 3;
          }
        }
        res.n_ball_only += popc64(ex.ballot(inside));
        for (uint64_t b = ex.ballot(hit); b; b &= b - 1) blocked |= 1u << ((b0 + ctz64(b)) / nl);
      }
      for (int m = 0; m < 27; m++) {
        if ((skip | blocked) >> m & 1) continue;
        const int di = m / 9 - 1, dj = m / 3 % 3 - 1, dk = m % 3 - 1, nx = C.ix + di, ny = C.iy + dj, nz = C.iz + dk;
        const double cost = cost1[(di != 0) + (dj != 0) + (dk != 0)];
        int v = S.find(nx, ny, nz);
        if (v < 0) {
          if (used >= p.max_nodes) break;      // `return`: the expansion ends, the search goes on (:644)
          v = used++;
          Node& nd = w.nodes[v];
          nd.ix = nx; nd.iy = ny; nd.iz = nz; nd.link = cur + 1;
          nd.g = cost + C.g; nd.f = nd.g + p.bias * S.heu(nx, ny, nz);
          S.heap_push(heap_n, v); S.insert(nx, ny, nz, v);
        } else if (!(w.nodes[v].link & MT_CLOSED)) {
          const double g = cost + C.g;
          if (w.nodes[v].g > g) {      // overwritten in place; the heap is not re-ordered
            Node& nd = w.nodes[v];
            nd.g = g; nd.f = g + p.bias * S.heu(nx, ny, nz); nd.link = cur + 1;
            res.n_updates++;
          }
        }
      }
    }
    res.nodes_used = used;
    if (res.n_degenerate > 0) res.flags |= NEP_MTLP_FLAG_DEGEN;
  }
  // ---- getPath (:682-707): the terminal node's coordinate is the goal's cell centre; every lane stores the same values ----
  if (terminal >= 0) {
    int depth = 0;
    for (int u = terminal; (w.nodes[u].link & (MT_CLOSED - 1)) != 0; u = (w.nodes[u].link & (MT_CLOSED - 1)) - 1) depth++;
    const int n_nodes = depth + 1;
    if (n_nodes > p.path_cap) res.flags |= NEP_MTLP_FLAG_PATH;
    res.n_path = n_nodes < p.path_cap ? n_nodes : p.path_cap;
    int t = depth;
    for (int u = terminal; u >= 0; u = (w.nodes[u].link & (MT_CLOSED - 1)) - 1, t--) {
      if (t < p.path_cap) {
        if (u == terminal) { path[3 * t] = goal_c[0]; path[3 * t + 1] = goal_c[1]; path[3 * t + 2] = goal_c[2]; }
        else S.coord(u, path + 3 * t);
      }
    }
    res.g_cells = w.nodes[terminal].g;
  }
  for (int i = 3 * res.n_path + ex.lane(); i < 3 * p.path_cap; i += Ex::W) path[i] = 0.0;
  *res_out = res;
}

}  // namespace nep_mtlp_impl

// ---- the handle (mtlp_host.cpp), and what the device form hangs on it (mtlp_kernels.hip) ---------------------------------------------
#include <vector>
struct nep_mtlp {
  nep_mtlp_cfg cfg;
  nep_mtlp_impl::Par par;
  std::vector<char> host_work;
  int host_flags = 0;
  void* dev = nullptr;
  void (*dev_free)(void*) = nullptr;
};
#endif
