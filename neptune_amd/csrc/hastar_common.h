// hastar_common.h — the rule set of the homotopic grid A* (include/neptune_hastar.h), once, for the host form (hastar_host.cpp)
// and the device form (hastar_kernels.hip): AstarPathFinder (neptune/src/Astar_searcher.cpp) with eu::updateHSig_orig,
// eu::updateContPts_orig and eu::tetherLength_orig (entangle_utils.cpp) and gjk::collision (gjk.cpp), general in both vertex
// counts.  Both translation units are compiled with -ffp-contract=off and agree on every output byte.
//
// One function, search<Ex>, is the whole search.  Ex is how a step's dense parts are spread: the host runs them one item at a
// time (width 1), the device 64 at a time on the lanes of one wave, and a ballot gathers the verdicts — the (neighbour x inflated
// polygon) occupancy tests of an expansion, the (rep) crossing tests of a neighbour, and inside updateContPts_orig the obstacle loop
// of each sampled point.  Everything else — the heap walk, the table probe, the list surgery — is wave-uniform: every lane runs it
// on the same values and stores the same values to the same addresses, so a lane only ever reads what it has itself written and
// the serial parts need no barrier.
//
// Memory of a search (Work, carved from one block of work_bytes()):
//   nodes      [max_nodes] Node, 64 B: index, key, scores, cameFrom, and its two lists by reference
//   hs_id/sign [max_nodes][hsig_cap]: a node's signature in full (3 B per entry)
//   heap       [max_nodes] node indices, libstdc++'s binary heap
//   hash       [hash_size >= 2 max_nodes] node index + 1, linear probing, exact match on (ix, iy, iz)
//   pool       [NEP_HASTAR_POOL_PER_NODE max_nodes][2]: the initial contact list and every list updateContPts_orig shortened
//   work       [cont_cap][2]: the child's list, laid out for updateContPts_orig
// A node's contact list is "pool[base_off .. base_off + base_n) and then the coordinates along cameFrom since": n_cont - base_n
// cells back to the node whose list that pool entry is.  Only closed nodes have children and closed nodes never change, so the walk
// is safe; an open node overwritten in place changes its own references only.
#ifndef NEP_HASTAR_COMMON_H_
#define NEP_HASTAR_COMMON_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/neptune_hastar.h"

#if defined(__HIPCC__)
#define HA_HD __host__ __device__ inline
#else
#define HA_HD inline
#endif

namespace nep_hastar_impl {

struct Par {
  double res, inv_res, xl, yl, cable, bias;
  int glx, gly, max_pops, max_nodes, hsig_cap, cont_cap, path_cap, hash_size, pool_cap;
};
struct Scene {
  int n_infl; const int32_t* infl_off; const double* infl_xy;
  int n_un; const int32_t* un_off; const double* un_xy;
  int n_rep; const double* rep;
};
struct Node {
  int32_t ix, iy; uint32_t iz; int32_t id;      // id: 1 open, -1 closed
  double g, f, len;
  int32_t from, n_hsig, n_cont, base_off, base_n, _pad;
};
struct Work { double* pool; double* work; Node* nodes; int32_t* heap; int32_t* hash; int16_t* hs_id; int8_t* hs_sign; };
struct StateSlot { int32_t* n_hsig; int16_t* hsig_id; int8_t* hsig_sign; int32_t* n_cont; double* cont; };

HA_HD size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
HA_HD size_t work_bytes(const Par& p) {
  return up16((size_t)p.pool_cap * 16) + up16((size_t)p.cont_cap * 16) + up16((size_t)p.max_nodes * sizeof(Node)) + up16((size_t)p.max_nodes * 4) +
         up16((size_t)p.hash_size * 4) + up16((size_t)p.max_nodes * p.hsig_cap * 2) + up16((size_t)p.max_nodes * p.hsig_cap);
}
HA_HD Work carve(char* b, const Par& p) {
  Work w;
  w.pool = (double*)b; b += up16((size_t)p.pool_cap * 16);
  w.work = (double*)b; b += up16((size_t)p.cont_cap * 16);
  w.nodes = (Node*)b; b += up16((size_t)p.max_nodes * sizeof(Node));
  w.heap = (int32_t*)b; b += up16((size_t)p.max_nodes * 4);
  w.hash = (int32_t*)b; b += up16((size_t)p.hash_size * 4);
  w.hs_id = (int16_t*)b; b += up16((size_t)p.max_nodes * p.hsig_cap * 2);
  w.hs_sign = (int8_t*)b;
  return w;
}

// ---- gjk::collision (gjk.cpp:76-149), vertices1 = V1[n1][2], vertices2 = V2[n2][2] -------------------------------------------------
// averagePoint is the serial sum divided by the count; the reference's loop has no bound, here 64 simplex updates end it with
// "no collision" (the CPU oracle's restatement has the same cap).
HA_HD int gjk_furthest(const double* V, int n, double dx, double dy) {
  double mx = dx * V[0] + dy * V[1]; int idx = 0;
  for (int i = 1; i < n; i++) { const double pr = dx * V[2 * i] + dy * V[2 * i + 1]; if (pr > mx) { mx = pr; idx = i; } }
  return idx;
}
HA_HD void gjk_support(const double* V1, int n1, const double* V2, int n2, double dx, double dy, double* out) {
  const int i = gjk_furthest(V1, n1, dx, dy), j = gjk_furthest(V2, n2, -dx, -dy);
  out[0] = V1[2 * i] - V2[2 * j]; out[1] = V1[2 * i + 1] - V2[2 * j + 1];
}
HA_HD void gjk_triple(const double* a, const double* b, const double* c, double* out) {      // b (a.c) - a (b.c)
  const double ac = a[0] * c[0] + a[1] * c[1], bc = b[0] * c[0] + b[1] * c[1];
  out[0] = b[0] * ac - a[0] * bc; out[1] = b[1] * ac - a[1] * bc;
}
HA_HD bool gjk_collision(const double* V1, int n1, const double* V2, int n2) {
  if (n1 <= 0 || n2 <= 0) return false;
  double p1x = 0, p1y = 0, p2x = 0, p2y = 0;
  for (int i = 0; i < n1; i++) { p1x += V1[2 * i]; p1y += V1[2 * i + 1]; }
  for (int i = 0; i < n2; i++) { p2x += V2[2 * i]; p2y += V2[2 * i + 1]; }
  p1x /= n1; p1y /= n1; p2x /= n2; p2y /= n2;
  double d[2] = {p1x - p2x, p1y - p2y};
  if (d[0] == 0 && d[1] == 0) d[0] = 1.0;
  double s0[2], s1[2] = {0, 0}, s2[2] = {0, 0}, a[2], ab[2], ac[2], ao[2], t[2];
  gjk_support(V1, n1, V2, n2, d[0], d[1], s0);
  if (s0[0] * d[0] + s0[1] * d[1] <= 0) return false;
  d[0] = -s0[0]; d[1] = -s0[1];
  int index = 0;
  for (int iter = 0; iter < 64; iter++) {
    ++index;
    gjk_support(V1, n1, V2, n2, d[0], d[1], a);
    if (index == 1) { s1[0] = a[0]; s1[1] = a[1]; } else { s2[0] = a[0]; s2[1] = a[1]; }
    if (a[0] * d[0] + a[1] * d[1] <= 0) return false;
    ao[0] = -a[0]; ao[1] = -a[1];
    if (index < 2) {
      ab[0] = s0[0] - a[0]; ab[1] = s0[1] - a[1];
      gjk_triple(ab, ao, ab, d);
      if (sqrt(d[0] * d[0] + d[1] * d[1]) == 0) { d[0] = ab[1]; d[1] = -ab[0]; }
      continue;
    }
    ab[0] = s1[0] - a[0]; ab[1] = s1[1] - a[1]; ac[0] = s0[0] - a[0]; ac[1] = s0[1] - a[1];
    gjk_triple(ab, ac, ac, t);
    if (t[0] * ao[0] + t[1] * ao[1] >= 0) { d[0] = t[0]; d[1] = t[1]; }
    else {
      gjk_triple(ac, ab, ab, t);
      if (t[0] * ao[0] + t[1] * ao[1] < 0) return true;
      s0[0] = s1[0]; s0[1] = s1[1];
      d[0] = t[0]; d[1] = t[1];
    }
    s1[0] = s2[0]; s1[1] = s2[1];
    --index;
  }
  return false;
}

// ---- the grid (Astar_searcher.cpp:18-127) -------------------------------------------------------------------------------------------
HA_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
HA_HD int to_int(double v) {      // int(v) of a finite double; saturating where C++ leaves it undefined
  if (!(v > -2147483648.0)) return -2147483647 - 1;
  if (!(v < 2147483647.0)) return 2147483647;
  return (int)v;
}
HA_HD void coord2index(const Par& p, const double* pt, int* ix, int* iy) {
  *ix = clampi(to_int((pt[0] - p.xl) * p.inv_res), 0, p.glx - 1);
  *iy = clampi(to_int((pt[1] - p.yl) * p.inv_res), 0, p.gly - 1);
}
HA_HD void index2coord(const Par& p, int ix, int iy, double* pt) {
  pt[0] = ((double)ix + 0.5) * p.res + p.xl;
  pt[1] = ((double)iy + 0.5) * p.res + p.yl;
}
// isOccupied's polygon test of one (cell, inflated polygon) pair: Cps in the column order of :147-150
HA_HD bool cell_hits(const Par& p, const Scene& sc, int ix, int iy, int k) {
  double c[2]; index2coord(p, ix, iy, c);
  const double r = 0.05;
  const double cps[8] = {c[0] + r, c[1] + r, c[0] + r, c[1] - r, c[0] - r, c[1] + r, c[0] - r, c[1] - r};
  const int o = sc.infl_off[k];
  return gjk_collision(sc.infl_xy + 2 * (size_t)o, sc.infl_off[k + 1] - o, cps, 4);
}
// updateHSig_orig's test of one rep (entangle_utils.cpp:1286-1322): 0 no entry, +1 / -1 the entry's sign
HA_HD int crossing(const double* rep, const double* pk, const double* pk1) {
  const double bx = rep[0], by = rep[1], ix = rep[2], iy = rep[3];      // pbi = col(0), pik = col(1)
  const double ikx = ix - pk[0], iky = iy - pk[1], bkx = bx - pk[0], bky = by - pk[1];      // pik_pk, pbi_pk
  const double c1 = ikx * bky - bkx * iky;
  const double c2 = (ix - pk1[0]) * (by - pk1[1]) - (bx - pk1[0]) * (iy - pk1[1]);
  if (!(c1 * c2 < 0)) return 0;
  const double a = fabs(iky * bky) > fabs(ikx * bkx) ? iky / bky : ikx / bkx;
  if (a < 0) return 0;
  if (a < 1) return c1 < 0 ? 1 : -1;
  return 0;
}
HA_HD uint32_t power2(int id) { return id >= 0 && id < 32 ? (uint32_t)1 << id : 0u; }      // power_int(2, id) modulo 2^32
HA_HD double seg_norm(const double* a, const double* b) { const double dx = b[0] - a[0], dy = b[1] - a[1]; return sqrt(dx * dx + dy * dy); }
HA_HD double tether_length(const double* pts, int n) {      // tetherLength_orig
  double len = 0.0;
  for (int i = 0; i + 1 < n; i++) len += seg_norm(pts + 2 * i, pts + 2 * i + 2);
  return len;
}
HA_HD int ctz64(uint64_t m) { return __builtin_ctzll(m); }
HA_HD int popc64(uint64_t m) { return __builtin_popcountll(m); }

// how the host spreads a dense part: one item at a time
struct SerialEx {
  static constexpr int W = 1;
  HA_HD int lane() const { return 0; }
  HA_HD uint64_t ballot(bool p) const { return p ? 1u : 0u; }
  HA_HD void sync() const {}
};

template <class Ex> HA_HD bool any_hit(const Ex& ex, const Scene& sc, const double* a, const double* b) {
  const double line[4] = {a[0], a[1], b[0], b[1]};
  for (int base = 0; base < sc.n_un; base += Ex::W) {
    const int k = base + ex.lane();
    bool hit = false;
    if (k < sc.n_un) { const int o = sc.un_off[k]; hit = gjk_collision(sc.un_xy + 2 * (size_t)o, sc.un_off[k + 1] - o, line, 2); }
    if (ex.ballot(hit)) return true;
  }
  return false;
}

// updateContPts_orig (entangle_utils.cpp:1356-1401) from in[n] to out[cap]: the new list's length, or -1 when it outgrows cap
template <class Ex> HA_HD int update_cont_pts(const Ex& ex, const Scene& sc, const double* in, int n, double* out, int cap) {
  const double interval = 0.2;
  int m = 0;
  if (m >= cap) return -1;
  out[0] = in[0]; out[1] = in[1]; m = 1;
  double cur[2] = {in[0], in[1]}, prev[2] = {in[0], in[1]};
  for (int i = 0; i + 1 < n; i++) {
    const double* A = in + 2 * i; const double* B = in + 2 * i + 2;
    const double ex_ = A[0] - B[0], ey_ = A[1] - B[1];
    const double norm = sqrt(ex_ * ex_ + ey_ * ey_);
    const int ratio = to_int(floor(norm / interval));
    for (int j = 1; j <= ratio; j++) {
      const double s = (double)j * interval;
      const double pt[2] = {A[0] + (s * (B[0] - A[0])) / norm, A[1] + (s * (B[1] - A[1])) / norm};
      if (any_hit(ex, sc, cur, pt)) {
        cur[0] = prev[0]; cur[1] = prev[1];
        if (m >= cap) return -1;
        out[2 * m] = cur[0]; out[2 * m + 1] = cur[1]; m++;
      }
      prev[0] = pt[0]; prev[1] = pt[1];
    }
    if (any_hit(ex, sc, cur, B)) {
      cur[0] = prev[0]; cur[1] = prev[1];
      if (m >= cap) return -1;
      out[2 * m] = cur[0]; out[2 * m + 1] = cur[1]; m++;
    }
    prev[0] = B[0]; prev[1] = B[1];
  }
  if (m >= cap) return -1;
  out[2 * m] = in[2 * (n - 1)]; out[2 * m + 1] = in[2 * (n - 1) + 1]; m++;
  return m;
}

struct Searcher {
  Par p; Scene sc; Work w;
  double start[2];
  int gx, gy;

  HA_HD void coord(int v, double* pt) const {      // GridNode::coord: the start keeps its un-rounded point
    if (v == 0) { pt[0] = start[0]; pt[1] = start[1]; } else index2coord(p, w.nodes[v].ix, w.nodes[v].iy, pt);
  }
  HA_HD double heu(int ix, int iy) const {      // getHeu, type 2 with the tie breaker
    const double dx = (double)ix - (double)gx, dy = (double)iy - (double)gy;
    double h = sqrt(dx * dx + dy * dy);
    h *= 1.01;
    return h;
  }
  HA_HD bool comp(int l, int r) const {      // CompareCost
    const Node& L = w.nodes[l]; const Node& R = w.nodes[r];
    if (fabs(L.f - R.f) < 1e-5) return L.f - L.g > R.f - R.g;
    return L.f > R.f;
  }
  // std::push_heap's __push_heap and std::pop_heap's __adjust_heap (libstdc++ bits/stl_heap.h)
  HA_HD void push_heap_(int hole, int top, int value) const {
    int parent = (hole - 1) / 2;
    while (hole > top && comp(w.heap[parent], value)) { w.heap[hole] = w.heap[parent]; hole = parent; parent = (hole - 1) / 2; }
    w.heap[hole] = value;
  }
  HA_HD void heap_push(int& n, int value) const { w.heap[n] = value; n++; push_heap_(n - 1, 0, value); }
  HA_HD int heap_pop(int& n) const {
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
  HA_HD uint32_t slot_of(int ix, int iy, uint32_t iz) const {
    uint32_t h = (uint32_t)ix * 0x9e3779b1u ^ ((uint32_t)iy * 0x85ebca77u + 0x7f4a7c15u) ^ (iz * 0xc2b2ae3du);
    h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
    return h & (uint32_t)(p.hash_size - 1);
  }
  HA_HD int find(int ix, int iy, uint32_t iz) const {      // the node under (ix, iy, iz), or -1
    for (uint32_t s = slot_of(ix, iy, iz);; s = (s + 1) & (uint32_t)(p.hash_size - 1)) {
      const int e = w.hash[s];
      if (e == 0) return -1;
      const Node& nd = w.nodes[e - 1];
      if (nd.ix == ix && nd.iy == iy && nd.iz == iz) return e - 1;
    }
  }
  HA_HD void insert(int ix, int iy, uint32_t iz, int v) const {
    uint32_t s = slot_of(ix, iy, iz);
    while (w.hash[s] != 0) s = (s + 1) & (uint32_t)(p.hash_size - 1);
    w.hash[s] = v + 1;
  }
  // list(v) ++ [pk1] into w.work: pool[base_off, base_off + base_n) and the coordinates along cameFrom since
  HA_HD void materialize(int v, const double* tail, double* dst) const {
    const Node& nd = w.nodes[v];
    for (int i = 0; i < 2 * nd.base_n; i++) dst[i] = w.pool[2 * (size_t)nd.base_off + i];
    int u = v;
    for (int t = nd.n_cont - 1; t >= nd.base_n; t--) { coord(u, dst + 2 * t); u = w.nodes[u].from; }
    if (tail) { dst[2 * nd.n_cont] = tail[0]; dst[2 * nd.n_cont + 1] = tail[1]; }
  }
};

template <class Ex>
HA_HD void search(const Ex& ex, const Par& p, const Scene& sc, const double* start_pt, const double* goal_pt, const StateSlot& in,
                  char* work_mem, nep_hastar_result* res_out, double* path, const StateSlot& out, bool malformed) {
  nep_hastar_result res;
  res.status = -1; res.n_path = 0; res.nodes_used = 0; res.pops = 0; res.n_updates = 0; res.n_length_checks = 0; res.n_cable_pruned = 0;
  res.flags = 0; res.g_cells = 0.0; res.length_m = 0.0;
  Searcher S; S.p = p; S.sc = sc; S.w = carve(work_mem, p);
  const Work& w = S.w;
  int n0_hsig = 0, n0_cont = 0, terminal = -1;
  if (malformed) res.flags |= NEP_HASTAR_FLAG_STATE;
  else {
    n0_hsig = *in.n_hsig; n0_cont = *in.n_cont;
    bool bad = n0_hsig < 0 || n0_hsig > p.hsig_cap || n0_cont < 1 || n0_cont > p.cont_cap;
    // coordinates out of range (or not finite) would make updateContPts_orig sample a segment forever
    bad = bad || !(fabs(start_pt[0]) <= NEP_HASTAR_MAX_COORD) || !(fabs(start_pt[1]) <= NEP_HASTAR_MAX_COORD) || !(fabs(goal_pt[0]) <= NEP_HASTAR_MAX_COORD) ||
          !(fabs(goal_pt[1]) <= NEP_HASTAR_MAX_COORD);
    if (!bad) for (int i = 0; i < 2 * n0_cont; i++) bad = bad || !(fabs(in.cont[i]) <= NEP_HASTAR_MAX_COORD);
    if (bad) { res.flags |= NEP_HASTAR_FLAG_STATE; malformed = true; n0_hsig = 0; n0_cont = 0; }
  }
  if (!malformed) {
    // the initial state is copied before anything is written: state_out may name state_in's arrays
    for (int i = ex.lane(); i < p.hash_size; i += Ex::W) w.hash[i] = 0;
    for (int i = 0; i < n0_hsig; i++) { w.hs_id[i] = in.hsig_id[i]; w.hs_sign[i] = in.hsig_sign[i]; }
    for (int i = 0; i < 2 * n0_cont; i++) w.pool[i] = in.cont[i];
    ex.sync();
    S.start[0] = start_pt[0]; S.start[1] = start_pt[1];
    int sx, sy; coord2index(p, start_pt, &sx, &sy); coord2index(p, goal_pt, &S.gx, &S.gy);
    int pool_used = n0_cont, heap_n = 0, used = 1;
    {
      Node& s = w.nodes[0];
      s.ix = sx; s.iy = sy; s.iz = 0; s.id = 1; s.g = 0; s.f = p.bias * S.heu(sx, sy); s.len = tether_length(w.pool, n0_cont);
      s.from = -1; s.n_hsig = n0_hsig; s.n_cont = n0_cont; s.base_off = 0; s.base_n = n0_cont; s._pad = 0;
    }
    S.heap_push(heap_n, 0);
    S.insert(sx, sy, 0u, 0);      // the start goes in under homotopy index 0 whatever its signature (:361-362)
    const double diag = 1.41421353816986083984375;      // offsetIndex.cast<float>().lpNorm<2>(): (double)sqrtf(2.0f)
    for (;;) {
      if (heap_n == 0) { res.status = -1; break; }
      if (res.pops >= p.max_pops) { res.status = 0; break; }
      const int cur = S.heap_pop(heap_n);
      res.pops++;
      w.nodes[cur].id = -1;
      const Node C = w.nodes[cur];
      if (C.ix == S.gx && C.iy == S.gy) { res.status = 1; terminal = cur; break; }
      // ---- AstarGetSucc ----
      double pk[2]; S.coord(cur, pk);
      // occupancy of the eight neighbours: off the grid, or any (neighbour, inflated polygon) pair in collision
      unsigned occ = 0;
      for (int k = 0; k < 8; k++) {
        const int kk = k < 4 ? k : k + 1, nx = C.ix + kk / 3 - 1, ny = C.iy + kk % 3 - 1;
        if (nx < 0 || nx >= p.glx || ny < 0 || ny >= p.gly) occ |= 1u << k;
      }
      for (int base = 0; base < 8 * sc.n_infl; base += Ex::W) {
        const int item = base + ex.lane();
        bool hit = false;
        if (item < 8 * sc.n_infl) {
          const int k = item / sc.n_infl, kk = k < 4 ? k : k + 1;
          if (!(occ >> k & 1)) hit = cell_hits(p, sc, C.ix + kk / 3 - 1, C.iy + kk % 3 - 1, item % sc.n_infl);
        }
        for (uint64_t m = ex.ballot(hit); m; m &= m - 1) occ |= 1u << ((base + ctz64(m)) / sc.n_infl) << 8;
      }
      occ = (occ | occ >> 8) & 0xffu;
      for (int k = 0; k < 8; k++) {
        const int kk = k < 4 ? k : k + 1, di = kk / 3 - 1, dj = kk % 3 - 1, nx = C.ix + di, ny = C.iy + dj;
        const double cost = di != 0 && dj != 0 ? diag : 1.0;
        if (occ >> k & 1) continue;
        double pk1[2]; index2coord(p, nx, ny, pk1);
        // updateHSig_orig: the entries to add as two bit masks over the reps, then the cancellation against the list's last entry
        uint64_t cross[NEP_HASTAR_MAX_REP / 64], neg[NEP_HASTAR_MAX_REP / 64];
        for (int q = 0; q < NEP_HASTAR_MAX_REP / 64; q++) cross[q] = neg[q] = 0;
        for (int base = 0; base < sc.n_rep; base += Ex::W) {
          const int r = base + ex.lane();
          const int c = r < sc.n_rep ? crossing(sc.rep + 4 * (size_t)r, pk, pk1) : 0;
          const uint64_t mc = ex.ballot(c != 0), mn = ex.ballot(c < 0);
          cross[base >> 6] |= mc << (base & 63); neg[base >> 6] |= mn << (base & 63);
        }
        const int16_t* ph_id = w.hs_id + (size_t)cur * p.hsig_cap; const int8_t* ph_sign = w.hs_sign + (size_t)cur * p.hsig_cap;
        int n_keep = C.n_hsig;
        while (n_keep > 0) {
          const int r = (int)ph_id[n_keep - 1] - 1;
          if (r < 0 || r >= sc.n_rep || !(cross[r >> 6] >> (r & 63) & 1)) break;
          const int add_sign = neg[r >> 6] >> (r & 63) & 1 ? -1 : 1;
          if ((int)ph_sign[n_keep - 1] == add_sign) break;
          cross[r >> 6] &= ~((uint64_t)1 << (r & 63));
          n_keep--;
        }
        int n_add = 0;
        for (int q = 0; q < NEP_HASTAR_MAX_REP / 64; q++) n_add += popc64(cross[q]);
        const int n_hsig = n_keep + n_add;
        if (n_hsig > p.hsig_cap) { res.flags |= NEP_HASTAR_FLAG_HSIG; continue; }
        // contPts.push_back(pkplus1)
        if (C.n_cont + 1 > p.cont_cap) { res.flags |= NEP_HASTAR_FLAG_CONT; continue; }
        // the cable test: cells against metres, as the reference has it
        double len = C.len + cost;
        int short_n = 0;
        if (len > p.cable) {
          res.n_length_checks++;
          S.materialize(cur, pk1, w.work);
          const int room = p.pool_cap - pool_used, cap = room < p.cont_cap ? room : p.cont_cap;
          short_n = update_cont_pts(ex, sc, w.work, C.n_cont + 1, w.pool + 2 * (size_t)pool_used, cap);
          if (short_n < 0) { res.flags |= room < p.cont_cap ? NEP_HASTAR_FLAG_POOL : NEP_HASTAR_FLAG_CONT; continue; }
          len = tether_length(w.pool + 2 * (size_t)pool_used, short_n);
          if (len > p.cable) { res.n_cable_pruned++; continue; }
        }
        // getIz, modulo 2^32
        uint32_t iz = 0;
        for (int e = 0; e < n_keep; e++) iz += (uint32_t)(e + 1) * power2(ph_id[e]) + (uint32_t)(int32_t)ph_sign[e];
        {
          int e = n_keep;
          for (int q = 0; q < NEP_HASTAR_MAX_REP / 64; q++)
            for (uint64_t m = cross[q]; m; m &= m - 1, e++) {
              const int r = q * 64 + ctz64(m);
              iz += (uint32_t)(e + 1) * power2(r + 1) + (uint32_t)(int32_t)(neg[q] >> (r & 63) & 1 ? -1 : 1);
            }
        }
        int v = S.find(nx, ny, iz);
        const bool fresh = v < 0;
        if (fresh) {
          if (used >= p.max_nodes) break;      // `return`: the expansion ends, the search goes on (:240)
          v = used++;
        } else {
          if (w.nodes[v].id != 1) continue;      // closed: left alone
          if (!(w.nodes[v].g > cost + C.g)) continue;
          res.n_updates++;
        }
        Node& nd = w.nodes[v];
        if (fresh) { nd.ix = nx; nd.iy = ny; nd.iz = iz; nd.id = 1; nd._pad = 0; }
        nd.g = cost + C.g;
        nd.f = nd.g + p.bias * S.heu(nx, ny);
        nd.from = cur; nd.len = len; nd.n_hsig = n_hsig;
        if (short_n > 0) { nd.n_cont = short_n; nd.base_off = pool_used; nd.base_n = short_n; pool_used += short_n; }
        else { nd.n_cont = C.n_cont + 1; nd.base_off = C.base_off; nd.base_n = C.base_n; }
        int16_t* h_id = w.hs_id + (size_t)v * p.hsig_cap; int8_t* h_sign = w.hs_sign + (size_t)v * p.hsig_cap;
        for (int e = 0; e < n_keep; e++) { h_id[e] = ph_id[e]; h_sign[e] = ph_sign[e]; }
        {
          int e = n_keep;
          for (int q = 0; q < NEP_HASTAR_MAX_REP / 64; q++)
            for (uint64_t m = cross[q]; m; m &= m - 1, e++) {
              const int r = q * 64 + ctz64(m);
              h_id[e] = (int16_t)(r + 1); h_sign[e] = (int8_t)(neg[q] >> (r & 63) & 1 ? -1 : 1);
            }
        }
        if (fresh) { S.heap_push(heap_n, v); S.insert(nx, ny, iz, v); }
      }
    }
    res.nodes_used = used;
  }
  // ---- outputs: getPath (:412-438) and the terminal state; every lane stores the same values ----
  int n_hs = n0_hsig, n_ct = n0_cont;
  if (terminal >= 0) {
    int depth = 0;
    for (int u = terminal; w.nodes[u].from >= 0; u = w.nodes[u].from) depth++;
    const int n_nodes = depth + 1;
    if (n_nodes > p.path_cap) res.flags |= NEP_HASTAR_FLAG_PATH;
    res.n_path = n_nodes < p.path_cap ? n_nodes : p.path_cap;
    int t = depth;
    for (int u = terminal; u >= 0; u = w.nodes[u].from, t--) if (t < p.path_cap) S.coord(u, path + 2 * t);
    res.length_m = tether_length(path, res.n_path);
    res.g_cells = w.nodes[terminal].g;
    n_hs = w.nodes[terminal].n_hsig; n_ct = w.nodes[terminal].n_cont;
    for (int e = 0; e < n_hs; e++) { out.hsig_id[e] = w.hs_id[(size_t)terminal * p.hsig_cap + e]; out.hsig_sign[e] = w.hs_sign[(size_t)terminal * p.hsig_cap + e]; }
    S.materialize(terminal, nullptr, out.cont);
  } else if (!malformed) {
    for (int e = 0; e < n_hs; e++) { out.hsig_id[e] = w.hs_id[e]; out.hsig_sign[e] = w.hs_sign[e]; }
    for (int i = 0; i < 2 * n_ct; i++) out.cont[i] = w.pool[i];
  }
  for (int i = 2 * res.n_path + ex.lane(); i < 2 * p.path_cap; i += Ex::W) path[i] = 0.0;
  for (int e = n_hs + ex.lane(); e < p.hsig_cap; e += Ex::W) { out.hsig_id[e] = 0; out.hsig_sign[e] = 0; }
  for (int i = 2 * n_ct + ex.lane(); i < 2 * p.cont_cap; i += Ex::W) out.cont[i] = 0.0;
  *out.n_hsig = n_hs; *out.n_cont = n_ct;
  *res_out = res;
}

}  // namespace nep_hastar_impl

// ---- the handle: host copies of the statics (hastar_host.cpp), and what the device form hangs on it (hastar_kernels.hip) ----------
#include <vector>
namespace nep_hastar_impl {
struct SceneHost {
  std::vector<int32_t> infl_off{0}, un_off{0};
  std::vector<double> infl_xy, un_xy, rep;
};
inline Scene scene_view(const SceneHost& s) {
  Scene v;
  v.n_infl = (int)s.infl_off.size() - 1; v.infl_off = s.infl_off.data(); v.infl_xy = s.infl_xy.data();
  v.n_un = (int)s.un_off.size() - 1; v.un_off = s.un_off.data(); v.un_xy = s.un_xy.data();
  v.n_rep = (int)(s.rep.size() / 4); v.rep = s.rep.data();
  return v;
}
}  // namespace nep_hastar_impl
struct nep_hastar {
  nep_hastar_cfg cfg;
  nep_hastar_impl::Par par;
  int n_scenes = 0;
  std::vector<nep_hastar_impl::SceneHost> scenes;
  std::vector<char> host_work;
  int host_flags = 0;
  bool dirty = true;                      // the statics changed since the device's copy was made
  void* dev = nullptr;                    // the device form's memory, and how to release it
  void (*dev_free)(void*) = nullptr;
};
#endif
