// fe_astar.h — the reference's best-first search as a device kernel, without and with enable_entangle_check.
// Included by geom_kernels.hip, inside namespace nep, below the beam front end: it uses that file's fe_child, fe_lattice_fill,
// fe_pos_cps, gjk_collision, hull_ref and fe_initial_z (its launch is launch_frontend's, behind this header), ent_device.h's ent_propagate, ent_iz,
// ent_valid_endpoint and ent_copy, lds_layout.h's kAsNC, kAsHeapLds and astar_ent_layout, and that object's -ffp-contract=off.
//
// KinodynamicSearch::run (kinodynamic_search.cpp:1629-1827) as oracle/neptune_oracle.c restates it (orc_frontend_astar, entangle
// check off): best-first on g + bias h over a binary heap with libstdc++'s push_heap / pop_heap mechanics, one node per voxel
// (the first insert wins), the in-place update of an open node of the same index on every second such event, the
// closest-so-far fallback node, a pop budget in place of the wall clock and the lattice order as a parameter.  Bit-identical to
// the oracle.
//
// One kernel template, frontend_astar_kernel<kEnt>: the search exists once, and what the entangle check adds (tests/astar_ent_ref.py
// is its rule, bit for bit) sits behind `if constexpr (kEnt)`:
//   child       the parent's state (the root: the state at A) through entanglesWithOtherAgents (kinodynamic_search.cpp:1157-1182,
//               :1341-1360); true drops the child (n_entangled).  g = parent g + sampled arc length, h = (dist + 0.3 crossings) + 1.0 bends
//   voxel       (ix, iy, getIz(state)) (:2006-2031), for the root expansion's inserts too (:1367-1377)
//   update      an open node of the same index updated in place keeps ITS entangle state (:1204 is commented out)
//   pop         the hulls and statics, then the other agents' base squares (collidesWithBases2d, :1583-1628); closest-so-far and the
//               goal test both ask for a valid end point (every active_cases <= 1, :1693-1700); an invalid node at the goal is expanded
//   result      the case block from the states along the returned path (state at the START of segment i; with pad_hold the held
//               segments keep the returned node's); n_children = pops, n_feasible = nodes created
//   capacity    a node's state is a fixed record (nep_fe_ent_state): a child whose list would outgrow NEP_FE_ENT_CAP, whose sampled
//               step adds more than 32 crossings or whose bend points exceed NEP_MAX_BEND is dropped, not counted in n_entangled, and
//               sets nep_fe_result.ent_overflow and NEP_FLAG_FE_ASTAR_ENT_REC (NEP_E_CAP from nep_batch_check) — a stated deviation
//   LDS         the plain instantiation keeps static arrays (12 856 B); the check's carves astar_ent_layout() (lds_layout.h), whose
//               working records are what the carve is for
//
// One wave per search.  What is parallel: the ns^2 lattice children of an expansion (one lane each: fe_child, with the check the
// entangle propagation of the child in a working record in LDS copied from the parent's state, which the wave stages once per
// expansion, the child's voxel lookup with what the commit reads of the voxel's holder, the child's voxel group) and the popped
// node's collision test (one lane per obstacle, a ballot).  What is serial, on lane 0: the heap and the commit of an expansion's
// surviving children in lattice order — siblings see each other through the voxel table, the update toggle counts events in that
// order and the node cap cuts the expansion at a child (the counters of pruned children are kept there too: the children behind the
// cut were never looked at in the reference).  With the check the wave then copies the states of the nodes that commit created into
// the state pool, 8 bytes per lane; whether a node may end a plan was decided when its state was made (AsNode::_pad).
// Per slot, in global memory: the node pool (160 B per node), the heap beyond its first kAsHeapLds entries (those are in LDS)
// and the voxel -> node table (open addressing, a power of two >= twice the pool; the result does not depend on its hashing); with
// the check the state pool (NEP_FE_ASTAR_ENT_NODE_BYTES per node) and the table's third key word.
// The search with the check has a second form on four waves per search, frontend_astar_team_kernel, at the end of this file (§37).
#pragma once

constexpr int kAsMaxNodes = 20000;      // node_num_max_ (kinodynamic_search.hpp:345): an expansion stops creating nodes at kAsMaxNodes - 1
constexpr int kAsPadPool = 16;          // nep_fe_result._pad bit 4: the search ran into a pool smaller than kAsMaxNodes

// (h and cost first: the heap's comparisons read just these two, one 16-byte load; _pad: with the entangle check, may a plan end here)
struct AsNode { double h, cost, g, end[6], cx[4], cy[4]; int prev, state, index, vx, vy, _pad; };
static_assert(sizeof(AsNode) == NEP_FE_ASTAR_NODE_BYTES, "AsNode's size is part of nep_batch_set_fe_astar's memory contract");
static_assert(sizeof(nep_fe_ent_state) == NEP_FE_ASTAR_ENT_NODE_BYTES && sizeof(nep_fe_ent_state) % 8 == 0, "a node's state in the pool is the fixed record: part of nep_batch_frontend_astar_ent's memory contract");
constexpr int kAsEntWords = (int)(sizeof(nep_fe_ent_state) / 8);      // a state as 8-byte words: the wave copies one with its first 57 lanes
static_assert(kAsEntWords <= 64, "one lane per 8-byte word of a state");

// CompareCost(left, right) (kinodynamic_search.hpp:163-179)
__device__ __forceinline__ bool as_comp(double cl, double hl, double cr, double hr) { return fabs(cl - cr) < 1e-5 ? hl > hr : cl > cr; }

struct AsHeap {
  int* lds; int* glb;
  __device__ __forceinline__ int get(int i) const { return i < kAsHeapLds ? lds[i] : glb[i]; }
  __device__ __forceinline__ void set(int i, int v) const { if (i < kAsHeapLds) lds[i] = v; else glb[i] = v; }
};
// std::__push_heap(first, hole, top = 0, value); the comparisons read the nodes' CURRENT costs (an open node updated in place
// stays where it is in the heap, as in the reference)
__device__ __forceinline__ void as_push_heap(const AsHeap& hp, const AsNode* pool, int hole, int value, double vc, double vh) {
  while (hole > 0) {
    const int parent = (hole - 1) / 2, pn = hp.get(parent);
    if (!as_comp(pool[pn].cost, pool[pn].h, vc, vh)) break;
    hp.set(hole, pn); hole = parent;
  }
  hp.set(hole, value);
}
// top(); pop(): std::pop_heap + pop_back
__device__ __forceinline__ int as_pop(const AsHeap& hp, const AsNode* pool, int& heap_n) {
  const int top = hp.get(0), len = heap_n - 1, value = hp.get(len);
  int hole = 0, second = 0;
  while (second < (len - 1) / 2) {        // std::__adjust_heap(first, 0, len, value)
    second = 2 * (second + 1);
    const int a = hp.get(second), b = hp.get(second - 1);
    const double ah = pool[a].h, ac = pool[a].cost, bh = pool[b].h, bc = pool[b].cost;
    const bool left = as_comp(ac, ah, bc, bh);
    if (left) second--;
    hp.set(hole, left ? b : a); hole = second;
  }
  if ((len & 1) == 0 && second == (len - 2) / 2) { second = 2 * (second + 1); hp.set(hole, hp.get(second - 1)); hole = second - 1; }
  if (len > 0) as_push_heap(hp, pool, hole, value, pool[value].cost, pool[value].h);
  heap_n = len;
  return top;
}

__device__ __forceinline__ unsigned long long as_key(int vx, int vy) { return ((unsigned long long)(unsigned)vx << 32) | (unsigned long long)(unsigned)vy; }
// node of voxel `key` (with the check: (key, iz), the third word in tiz), or -1; pos: where it is / where it would go (the table is
// never more than half full: the walk ends)
template <bool kEnt>
__device__ __forceinline__ int as_find(const unsigned long long* tkey, const unsigned* tiz, const int* tval, int mask, unsigned long long key, unsigned iz, int start, int& pos) {
  int p = start;
  for (int it = 0; it <= mask; it++, p = (p + 1) & mask) {
    const int v = tval[p];
    if (v < 0 || (tkey[p] == key && (!kEnt || tiz[p] == iz))) { pos = p; return v < 0 ? -1 : v; }
  }
  pos = -1; return -1;
}

// The list of a sampled step's new crossings: EntAdd under a name of this kernel's own, so that ent_propagate and what it calls are
// instantiated for this kernel alone — sharing ent_check_kernel's instantiation changed that kernel's code (its callee got a second caller).
struct AsEntAdd : EntAdd { };
// a state at A the search can start from: counts within the fixed record, bend indices on the list
__device__ __forceinline__ bool as_ent_init_ok(const nep_fe_ent_state* s) {
  if (s->n_alpha < 0 || s->n_alpha > NEP_FE_ENT_CAP || s->n_bend < 0 || s->n_bend > NEP_MAX_BEND) return false;
  for (int k = 0; k < s->n_bend; k++) if (s->bend[k] < 0 || s->bend[k] >= s->n_alpha) return false;
  return true;
}

// kEnt: with the entangle check (xa, ea and the dynamic LDS of astar_ent_layout() are read under it alone)
template <bool kEnt>
__global__ __launch_bounds__(64) void frontend_astar_kernel(SceneParams sp, ProblemSet ps, nep_fe_cfg fc, FeAstarArgs aa, FeAstarEntArgs xa, FeEntArgs ea,
                                                            const nep_fe_start* __restrict__ starts, nep_guess* __restrict__ guess_out, nep_fe_result* __restrict__ res_out) {
  // s_ch: a child of the expansion at hand: end state [6], cx [4], cy [4], g, h, cost.  s_hcost: per voxel group (indexed by its first
  // child): g + bias h of the voxel's holder, kept current through the commit.  With the check: s_work [kAsNC] the children's states,
  // [kAsNC]: the parent's; s_path: the returned path's nodes by index
  double (*s_ch)[17]; double *s_lat, *s_hcost; int *s_heap, *s_vx, *s_vy, *s_f, *s_pos, *s_hst, *s_hidx, *s_new, *s_grp;
  nep_fe_ent_state* s_work = nullptr; unsigned* s_iz = nullptr; int *s_valid = nullptr, *s_path = nullptr;
  if constexpr (kEnt) {
    extern __shared__ __attribute__((aligned(16))) double as_smem[];
    const AstarEntLayout AL = astar_ent_layout();      // (lds_layout.h)
    s_work = lds_rec<nep_fe_ent_state>(as_smem, AL.work);
    s_ch = (double(*)[17])lds_at<double>(as_smem, AL.ch); s_hcost = lds_at<double>(as_smem, AL.hcost); s_lat = lds_at<double>(as_smem, AL.lat);
    s_heap = lds_at<int>(as_smem, AL.heap);
    s_vx = lds_at<int>(as_smem, AL.ints); s_vy = s_vx + kAsNC; s_iz = (unsigned*)(s_vy + kAsNC); s_f = s_vy + 2 * kAsNC; s_pos = s_f + kAsNC;
    s_hst = s_pos + kAsNC; s_hidx = s_hst + kAsNC; s_new = s_hidx + kAsNC; s_grp = s_new + kAsNC; s_valid = s_grp + kAsNC;
    s_path = lds_at<int>(as_smem, AL.path);
  } else {      // (static arrays, not a carve: separator_packed_kernel lost 1.8 % on a dynamic one with equal registers)
    __shared__ int heap_[kAsHeapLds];
    __shared__ double ch_[kAsNC][17], lat_[4 * NEP_FE_MAX_SAMPLES], hcost_[kAsNC];
    __shared__ int vx_[kAsNC], vy_[kAsNC], f_[kAsNC], pos_[kAsNC], hst_[kAsNC], hidx_[kAsNC], new_[kAsNC], grp_[kAsNC];
    s_heap = heap_; s_ch = ch_; s_lat = lat_; s_hcost = hcost_;
    s_vx = vx_; s_vy = vy_; s_f = f_; s_pos = pos_; s_hst = hst_; s_hidx = hidx_; s_new = new_; s_grp = grp_;
  }
  const int lane = threadIdx.x;
  if (ps.fe_count && (int)blockIdx.x >= *ps.fe_count) return;      // (an active set: fe_order is the list of active slots)
  const int slot = ps.fe_order ? ps.fe_order[blockIdx.x] : (int)blockIdx.x, scene = slot / sp.n_local, own = sp.first_local + (slot % sp.n_local);
  const int N = sp.num_agents, S = sp.n_static, ns = fc.num_samples, NC = ns * ns, D = sp.num_pol;
  const int cap = aa.pool, mask = aa.tab_cap - 1;
  AsNode* const pool = (AsNode*)aa.nodes + (size_t)slot * cap;
  const AsHeap hp{s_heap, aa.heap + (size_t)slot * cap};
  unsigned long long* const tkey = aa.tab_key + (size_t)slot * aa.tab_cap;
  int* const tval = aa.tab_val + (size_t)slot * aa.tab_cap;
  const nep_fe_start* st = starts + slot;
  const double gx = st->goal[0], gy = st->goal[1];
  const double bx = ps.pb[2 * own], by = ps.pb[2 * own + 1];
  const double init[6] = {st->pos[0], st->pos[1], st->vel[0], st->vel[1], st->accel[0], st->accel[1]};
  // with the check: the state pool, the table's third key word, the state at A and what ent_propagate reads
  nep_fe_ent_state* spool = nullptr; unsigned* tiz = nullptr; const nep_fe_ent_state* root_state = nullptr; bool root_ok = true;
  EntCtx ec;
  if constexpr (kEnt) {
    spool = (nep_fe_ent_state*)xa.states + (size_t)slot * cap;
    tiz = xa.tab_iz + (size_t)slot * aa.tab_cap;
    root_state = ea.init ? ea.init + slot : nullptr;
    root_ok = !root_state || as_ent_init_ok(root_state);      // (a malformed state at A: the search starts from the empty one, flagged)
    ec.N = N; ec.S = S; ec.own = own; ec.num_pol = D; ec.ns = ea.ns; ec.T_span = sp.T_span; ec.cable = fc.cable_length;
    ec.pb = ps.pb; ec.srep = ea.srep + (long)scene * sp.static_stride * 4; ec.slong = ea.slong + (long)scene * sp.static_stride * 2;
    ec.sampled = ea.sampled; ec.present = ea.present;
    ec.ps = &ps; ec.scene = scene; ec.n_hull = sp.n_hull;
    ec.packed = ea.packed; ec.pk_stride = ea.pk_stride;
  }
#ifdef NEP_PROFILE_PHASES
  long long tph[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long long tlast = clock64();      // pop, GJK (+ bases), fe_child, propagation, lookup + group, commit, state copy, (setup + result); without the check 3 and 6 stay zero
#define AS_TICK(k) do { const long long t_ = clock64(); tph[k] += t_ - tlast; tlast = t_; } while (0)
#else
#define AS_TICK(k) do { } while (0)
#endif
  for (int k = lane; k <= mask; k += 64) tval[k] = -1;
  if (lane < NEP_FE_MAX_SAMPLES) fe_lattice_fill(sp, fc, s_lat, lane);
  const FeLattice lat{s_lat, s_lat + NEP_FE_MAX_SAMPLES, s_lat + 2 * NEP_FE_MAX_SAMPLES, s_lat + 3 * NEP_FE_MAX_SAMPLES};
  // goal_occupied_ (setUp :210-226)
  bool occ = false;
  {
    Pts4 G; const double r = 0.5;
    G.x[0] = gx + r; G.y[0] = gy + r; G.x[1] = gx + r; G.y[1] = gy - r; G.x[2] = gx - r; G.y[2] = gy + r; G.x[3] = gx - r; G.y[3] = gy - r;
    for (int j = lane; j < N; j += 64) {
      if (j == own) continue;
      const HullRef hr = hull_ref(ps, sp.n_hull, scene, j);
      const long h = hr.e * sp.num_pol + (D - 1);
      const int nv = blk(ps.hull_nv, hr.boff)[h];
      if (nv > 0 && gjk_collision(nv, blk(ps.hull_xy, hr.boff) + h * kHullV * 2, G)) occ = true;
    }
  }
  const bool goal_occupied = __ballot(occ) != 0ull;
  __syncthreads();

  // what lane 0 keeps (the other lanes get what they need of it by __shfl): the heap's length, nodes created, the update toggle, with
  // the check the counters of the children it walked past
  int heap_n = 0, used = 0, ran_trigger = 0, capped = 0, n_entangled = 0, overflow = root_ok ? 0 : 1;
  int status = NEP_FE_EMPTY, cur = -1, closest = -1, pops = 0;
  double smallest = 1.7976931348623157e308;
  AS_TICK(7);

  // both expandAndAddToQueue overloads (:1045-1228, :1240-1385): e_cur < 0 = from the initial state
  auto expand = [&](int e_cur, const double* pe, double pg, int pindex) {
    const bool first = e_cur < 0;
    // (0) with the check: the parent's state, staged once for every lane's copy
    if constexpr (kEnt) {
      if (lane < kAsEntWords) {
        long v = 0;
        if (!first) v = ((const long*)(spool + e_cur))[lane];
        else if (root_state && root_ok) v = ((const long*)root_state)[lane];
        ((long*)(s_work + kAsNC))[lane] = v;
      }
      __syncthreads();
    }
    // (1) every lane its child (the kinodynamic tests; with the check the entangle propagation from the parent's state, the costs and
    // iz), the node that holds the child's voxel before this expansion (with what the commit reads of it) and the child's voxel
    // group: the first child of this expansion with the same voxel
    int my_f = -2, my_vx = 0, my_vy = 0; unsigned my_iz = 0u;      // -2: no child; with the check -3: entangled; -4: beyond the fixed record
    if (lane < NC) {
      const int comb = aa.order ? aa.order[lane] : lane;
      FeChild ch;
      const bool have = fe_child(sp, fc, lat, pe, pg, first, comb / ns, comb % ns, gx, gy, bx, by, ch);
      AS_TICK(2);
      // a surviving child into LDS with its costs, and its voxel's lookup
      auto stage = [&](double g, double h, double f) {
        double* o = s_ch[lane];
#pragma unroll
        for (int i = 0; i < 6; i++) o[i] = ch.e[i];
#pragma unroll
        for (int i = 0; i < 4; i++) { o[6 + i] = ch.cx[i]; o[10 + i] = ch.cy[i]; }
        o[14] = g; o[15] = h; o[16] = f;
        my_vx = ch.vx; my_vy = ch.vy;
        s_vx[lane] = ch.vx; s_vy[lane] = ch.vy;
        if constexpr (kEnt) { s_iz[lane] = my_iz; s_valid[lane] = ent_valid_endpoint(s_work + lane, N) ? 1 : 0; }
        const unsigned long long key = as_key(ch.vx, ch.vy);
        int pos = -1;
        my_f = as_find<kEnt>(tkey, tiz, tval, mask, key, my_iz, (int)(fe_hash((long long)(kEnt ? key ^ ((unsigned long long)my_iz * 0xC2B2AE3D27D4EB4Full) : key)) & (unsigned)mask), pos);
        s_pos[lane] = pos;
        // (state and index do not change during the commit below; the cost only by an update of that commit, which keeps the group's entry current)
        if (my_f >= 0) { s_hst[lane] = pool[my_f].state; s_hidx[lane] = pool[my_f].index; s_hcost[lane] = pool[my_f].cost; }
      };
      if (have) {
        if constexpr (kEnt) {
          nep_fe_ent_state* w = s_work + lane;
          ent_copy(w, s_work + kAsNC);
          double arc = 0.0;
          unsigned add_tail[kEntAddCap - EntAdd::reg];
          const int rc = ent_propagate<AsEntAdd>(ec, w, AsEntAdd::Store{add_tail, kEntAddCap}, ch.cx, ch.cy, Ev2{ch.e[0], ch.e[1]}, pindex + 1, arc, true, 1);
          AS_TICK(3);
          if (rc == 1) my_f = -3;
          else if (rc != 0) my_f = -4;
          else {
            const double g = pg + arc;
            const double h = (ch.dist + 0.3 * (double)w->n_alpha) + 1.0 * (double)w->n_bend;      // (:1177-1182)
            my_iz = ent_iz(w);
            stage(g, h, g + fc.bias * h);
          }
        } else stage(ch.g, ch.dist, ch.f);
      }
      s_f[lane] = my_f; s_new[lane] = -1;
    }
    {
      int grp = lane;
      for (int r = 0; r < NC; r++) {      // (r is wave-uniform: the shuffles are lane reads)
        const int fr = __shfl(my_f, r), xr = __shfl(my_vx, r), yr = __shfl(my_vy, r);
        bool same = fr >= -1 && xr == my_vx && yr == my_vy;
        if constexpr (kEnt) same = same && (unsigned)__shfl((int)my_iz, r) == my_iz;
        if (r < lane && grp == lane && same) grp = r;
      }
      if (lane < NC) s_grp[lane] = grp;
    }
    __syncthreads();
    AS_TICK(4);
    // (2) lane 0 commits the survivors in lattice order.  Nothing in this loop scans: what a child needs of its voxel's holder is
    // one LDS entry of its group.  (A version that found siblings and updated holders by scanning r < q per child, all in LDS, was
    // measured 19 % slower per launch than reading the holder's cost from memory: one lane's dependent LDS reads add up.)
    if (lane == 0) {
      for (int q = 0; q < NC; q++) {
        if (used >= cap - 1) { if (cap < kAsMaxNodes) capped = 1; break; }      // "run out of memory" (:1061-1065), at the handle's pool when that is smaller
        int f = s_f[q];
        if (f == -2) continue;
        if constexpr (kEnt) {
          if (f == -3) { n_entangled++; continue; }
          if (f == -4) { overflow = 1; continue; }
        }
        const double* c = s_ch[q];
        const int vx = s_vx[q], vy = s_vy[q], grp = s_grp[q];
        unsigned iz = 0u;
        if constexpr (kEnt) iz = s_iz[q];
        int pos = s_pos[q];
        if (!first) {
          int hst, hidx;
          if (f >= 0) { hst = s_hst[q]; hidx = s_hidx[q]; }
          else { hst = 1; hidx = pindex + 1; if (grp != q) f = s_new[grp]; }      // (the group's first child took the voxel in this commit: open, of this index)
          if (f >= 0) {
            if (hst == 1 && hidx == pindex + 1) {
              if (c[16] < s_hcost[grp] && (ran_trigger & 1) == 0) {      // update the open node in place (:1190-1203): not its entangle state (:1204), not the heap
                AsNode* o = pool + f;
                o->prev = e_cur; o->g = c[14]; o->h = c[15]; o->cost = c[16];
                for (int i = 0; i < 6; i++) o->end[i] = c[i];
                for (int i = 0; i < 4; i++) { o->cx[i] = c[6 + i]; o->cy[i] = c[10 + i]; }
                s_hcost[grp] = c[16];
              }
              ran_trigger++;
            }
            continue;
          }
        }
        AsNode* nb = pool + used;
        nb->h = c[15]; nb->cost = c[16]; nb->g = c[14];
        for (int i = 0; i < 6; i++) nb->end[i] = c[i];
        for (int i = 0; i < 4; i++) { nb->cx[i] = c[6 + i]; nb->cy[i] = c[10 + i]; }
        nb->prev = e_cur; nb->state = 1; nb->index = pindex + 1; nb->vx = vx; nb->vy = vy;
        if constexpr (kEnt) nb->_pad = s_valid[q]; else nb->_pad = 0;
        as_push_heap(hp, pool, heap_n, used, c[16], c[15]); heap_n++;
        // unordered_map::insert keeps the first: the walk goes on from where the lookup ended (entries are never removed)
        const unsigned long long key = as_key(vx, vy);
        if (as_find<kEnt>(tkey, tiz, tval, mask, key, iz, pos >= 0 ? pos : 0, pos) < 0 && pos >= 0) {
          tkey[pos] = key; tval[pos] = used;
          if constexpr (kEnt) tiz[pos] = iz;
        }
        s_new[q] = used; s_hcost[q] = c[16];
        used++;
      }
    }
    __syncthreads();
    AS_TICK(5);
    // (3) with the check: the states of the nodes this commit created, into the pool: the wave, 8 bytes per lane (s_new[q] < cap - 1: inside the pool)
    if constexpr (kEnt) {
      for (int q = 0; q < NC; q++) {
        const int n = s_new[q];
        if (n >= 0 && lane < kAsEntWords) ((long*)(spool + n))[lane] = ((const long*)(s_work + q))[lane];
      }
      __syncthreads();
      AS_TICK(6);
    }
  };

  expand(-1, init, 0.0, 0);
  const int max_pops = aa.max_pops;
  const double base_radius = 0.7, safe_dist = (sp.T_span * sp.v_max) * 2;
  for (;;) {
    if (__shfl(heap_n, 0) <= 0) break;
    if (pops >= max_pops) { status = NEP_FE_DEPTH_REACHED; break; }       // RUNTIME_REACHED: the budget (:1644-1651)
    if (lane == 0) { cur = as_pop(hp, pool, heap_n); pool[cur].state = -1; }
    cur = __shfl(cur, 0); pops++;
    __syncthreads();
    AS_TICK(0);
    const AsNode* nd = pool + cur;
    const int index = nd->index;
    const bool valid = !kEnt || nd->_pad != 0;
    double pe[6], cx[4], cy[4];
#pragma unroll
    for (int i = 0; i < 6; i++) pe[i] = nd->end[i];
#pragma unroll
    for (int i = 0; i < 4; i++) { cx[i] = nd->cx[i]; cy[i] = nd->cy[i]; }
    const double pg = nd->g;
    // collidesWithObstacles2dSolve (:1514-1553) and, with the check, collidesWithBases2d (:1583-1628): the control polygon against
    // every other agent's hull of the node's interval, every static polygon and every other agent's base square, one per lane
    Pts4 B;
    fe_pos_cps(cx, sp.T_span, B.x); fe_pos_cps(cy, sp.T_span, B.y);
    const int idx = (index > D ? D : index) - 1;
    bool hit = false;
    for (int o = lane; o < (kEnt ? N + S + N : N + S); o += 64) {
      if (!kEnt || o < N + S) {
        int nv; const double* V;
        if (o < N) {
          if (o == own) continue;
          const HullRef hr = hull_ref(ps, sp.n_hull, scene, o); const long h = hr.e * sp.num_pol + idx;
          nv = blk(ps.hull_nv, hr.boff)[h]; V = blk(ps.hull_xy, hr.boff) + h * kHullV * 2;
        } else { const long js = (long)scene * sp.static_stride + (o - N); nv = ps.static_nv[js]; V = ps.static_xy + js * kHullV * 2; }
        if (nv > 0 && gjk_collision(nv, V, B)) hit = true;
      } else {
        const int j = o - N - S;
        if (j == own) continue;
        const double pbx = ps.pb[2 * j], pby = ps.pb[2 * j + 1];
        const double d1 = sqrt((B.x[0] - pbx) * (B.x[0] - pbx) + (B.y[0] - pby) * (B.y[0] - pby));
        if (d1 > safe_dist) continue;
        const double sq[8] = {pbx + base_radius, pby + base_radius, pbx + base_radius, pby - base_radius, pbx - base_radius, pby - base_radius, pbx - base_radius, pby + base_radius};
        if (gjk_collision(4, sq, B)) hit = true;
      }
    }
    const bool collides = __ballot(hit) != 0ull;
    AS_TICK(1);
    if (collides) continue;
    const double dist = sqrt((pe[0] - gx) * (pe[0] - gx) + (pe[1] - gy) * (pe[1] - gy));
    const double dfi = sqrt((pe[0] - init[0]) * (pe[0] - init[0]) + (pe[1] - init[1]) * (pe[1] - init[1]));
    const double dtc = goal_occupied ? dist * dist : dfi;
    const double dti = dtc * (double)index;
    if (valid && dti < smallest) { smallest = dti; closest = cur; }      // (:1683-1700)
    if (valid && dist < fc.goal_size) { status = NEP_FE_GOAL_REACHED; break; }
    expand(cur, pe, pg, index);
  }

  const int best = status == NEP_FE_GOAL_REACHED ? cur : closest;        // use_not_reaching_soln (every lane holds cur and closest)
  if (lane == 0) {
    if (best < 0) status = NEP_FE_NO_SOLUTION;
    nep_guess* g = guess_out + slot;
    for (int e = 0; e < 3 * NEP_MAX_POL * 4; e++) (&g->coeff[0][0][0])[e] = 0.0;
    g->t_start = st->t_start; g->n_alpha = 0;
    int K = 0, depth = 0, rows = 0; double cost = 0.0, dtg = 0.0;
    if constexpr (kEnt) for (int d = 0; d <= NEP_MAX_POL; d++) s_path[d] = -1;
    if (best >= 0) {
      const AsNode* b = pool + best;
      depth = b->index; K = depth < D ? depth : D; cost = b->cost;
      dtg = sqrt((b->end[0] - gx) * (b->end[0] - gx) + (b->end[1] - gy) * (b->end[1] - gy));
      // recoverPwpOut (:521-553): the nodes of the path with index <= num_pol (a node's index is its place on its path)
      int k = best;
      for (int it = 0; it < cap && k >= 0; it++) {
        const AsNode* q = pool + k;
        const int d = q->index;
        if (d >= 1 && d <= D) {
          if constexpr (kEnt) s_path[d] = k;
          for (int c = 0; c < 4; c++) { g->coeff[0][d - 1][c] = q->cx[c]; g->coeff[1][d - 1][c] = q->cy[c]; }
        }
        k = q->prev;
      }
      int Kg = K;
      if (fc.pad_hold && K < D) {   // hold the end point for the rest of the horizon (as frontend_kernel does); the held segments keep the returned node's state
        for (int d = K + 1; d <= D; d++) {
          g->coeff[0][d - 1][3] = b->end[0]; g->coeff[1][d - 1][3] = b->end[1];
          if constexpr (kEnt) s_path[d] = best;
        }
        Kg = D;
      }
      fe_initial_z(st->pos[2], st->vel[2], st->accel[2], st->goal[2], sp.T_span, D, sp.v_max, sp.a_max, g->coeff[2]);   // coeffs_z_ (:540)
      for (int d = Kg + 1; d <= D; d++) for (int c = 0; c < 4; c++) g->coeff[2][d - 1][c] = 0.0;
      K = Kg; rows = Kg;
    }
    if constexpr (kEnt) s_path[NEP_MAX_POL + 1] = rows;
    g->K = K;
    if (capped && ps.flags) atomicOr(ps.flags, NEP_FLAG_FE_ASTAR_POOL);
    if (kEnt && overflow && ps.flags) atomicOr(ps.flags, NEP_FLAG_FE_ASTAR_ENT_REC);
    if (res_out) {
      nep_fe_result* o = res_out + slot;
      o->status = status; o->K = K; o->depth = depth; o->n_children = pops; o->n_feasible = used; o->n_collision_free = 0;
      o->goal_occupied = goal_occupied ? 1 : 0; o->_pad = capped ? kAsPadPool : 0;
      o->cost = cost; o->dist_to_goal = dtg; o->n_entangled = n_entangled; o->ent_overflow = kEnt ? overflow : 0;
    }
  }
  // with the check, the case block (solver_gurobi_poly.cpp:624-631): row i from the state at the START of segment i — the path's node
  // of index i, the state at A for i = 0 — for the rows of the guess, zero beyond; one agent per lane
  if constexpr (kEnt) {
    __syncthreads();
    if (ea.case_out) {
      const int rows = s_path[NEP_MAX_POL + 1];
      int* const co = ea.case_out + (size_t)slot * NEP_MAX_POL * N;
      for (int i = 0; i < NEP_MAX_POL; i++) {
        const nep_fe_ent_state* sn = nullptr;
        if (i < rows) { if (i == 0) sn = (root_state && root_ok) ? root_state : nullptr; else if (s_path[i] >= 0) sn = spool + s_path[i]; }
        const int na = sn ? sn->n_alpha : 0;
        for (int j = lane; j < N; j += 64) {
          int cs = 0, cnt = 0;
          for (int a = 0; a < na; a++) if (sn->id[a] == j + 1) { cnt++; cs = sn->cs[a]; }
          co[(size_t)i * N + j] = cnt == 1 ? cs : 0;
        }
      }
    }
  }
#ifdef NEP_PROFILE_PHASES
  AS_TICK(7);
  if (lane == 0 && ps.dbg) { for (int k = 0; k < 8; k++) ps.dbg[(long)slot * 32 + k] = tph[k]; ps.dbg[(long)slot * 32 + 8] = pops; ps.dbg[(long)slot * 32 + 9] = used; }
#endif
#undef AS_TICK
}

// ---- The same search on four waves (nep_batch_set_fe_astar_team) -------------------------------------------------------
// frontend_astar_kernel<true> spends 86 % of a search in the children's entangle propagation: 25 lanes of one wave, each walking
// ns steps x (N - 1) tethers in series.  Which crossings a sampled step adds does not depend on the entangle state (ent_device.h, the
// beam's two passes), so a workgroup of four waves, one per SIMD, finds them in a dense pass of its own and leaves the surgery alone to
// the children's lanes.  The search rule is frontend_astar_kernel<true>'s, statement for statement: heap, voxel table, commit order,
// update toggle, node cap, counters and the result are thread 0's, as they are lane 0's there; the same per-slot memory is read and
// written, so that calls of either form may alternate on a handle.  Bit-identical to the one-wave form.
//
// Per expansion:  (0) the parent's state staged, 57 threads.  (1a) wave 0, one lane per child: fe_child; end point and polynomial into
// s_ch, the children with "have" listed densely.  (1b) all 256 threads, one work item per (child with "have", sampled step j, chunk c of
// the obstacle index range [0, N + S)): the new crossings of the chunk's obstacles, exactly as ent_propagate finds them — the packed
// records of ent_pack_kernel through ent_cross_agent in index order, the statics through ent_cross_static behind the last agent — in a
// list of the item's own (AsTeamAdd).  (1c) a (child, step)'s list is the concatenation of its chunks' lists in index order, copied into
// the pool under a header word of ent_cross_step's format.  (1d) wave 0, one lane per child: the parent's state copied, ent_propagate_pre
// on the child's lists (merge, counts, bend points, tether length: ent_propagate's return codes in its order), costs, iz, valid end
// point, voxel lookup and group as in the one-wave form.  (2) thread 0 commits.  (3) the created nodes' states into the pool, 256 threads.
//
// Why the chunks are exact.  (a) The base-addition pop at the end of ent_cross_agent removes the list's last two entries when they
// carry the same id and the same case.  Agent i's visit pushes entries of id i + 1 only, and every agent is visited once per step.  If
// the visit pushed something, the last entry is its own and the one before it must carry its id: its own too.  If it pushed nothing, the
// last two entries are an earlier visit's, or two earlier visits': two visits' entries differ in id; one earlier visit b leaves no two
// equal entries behind — without its sweep test true, its pushes come from the c1 c2 < 0 tests of k = 0 .. nb - 1, whose cases are
// k + 2, 1 (k = nb - 1 only) and 0 (k = 0 only): pairwise different; with it, the sweep's push (case 1, or case 0 with nb = 1) can equal
// only the push of the crossing test of the same k = nb - 1, which follows it at once: the pair is the list's end and b's own pop took
// it.  So a pop never reaches into another agent's entries, the agents of a step may be cut anywhere, and ent_cross_static, which only
// pushes, follows the last agent.  (b) A step's capacity flag is set when a PUSH finds the running count at lim, not when the final list
// is long, and the pop shortens the list.  The running count in the serial walk is the length of the earlier chunks' final lists
// (base) plus the chunk's own running count, so the flag is raised iff for some chunk base + peak > lim, peak the highest count the
// chunk's list reached (AsTeamAdd::peak; a chunk whose own list overflowed has base + peak > lim by itself).  Without the flag every push
// succeeded in both walks and the lists are equal; with it the child is dropped whatever the lists hold.
//
// Loop control goes through LDS (a shuffle spans one wave): thread 0 publishes go / cur at the head of every pop, the collision
// verdict is an LDS word per pop parity, and every wave takes the same barriers.  Every loop is bounded as in the one-wave form.
struct AsTeamState : nep_fe_ent_state { };      // (a type of this kernel's own: the surgery's out-of-line functions are instantiated for it alone, see AsEntAdd)
struct AsTeamAdd : EntAdd {
  int peak;
  __device__ __forceinline__ void clear() { EntAdd::clear(); peak = 0; }
  __device__ __forceinline__ void set(int i, unsigned v) { EntAdd::set(i, v); peak = i + 1 > peak ? i + 1 : peak; }      // (ent_push: set(n, word) then n++)
};
enum { kTcGo = 0, kTcCur = 1, kTcHit = 2 /* and 3: per pop parity */, kTcOcc = 4, kTcHave = 5 };
static_assert(kTcHave < kAsTeamCtl, "control words");

__global__ __launch_bounds__(kAsTeamThreads) void frontend_astar_team_kernel(SceneParams sp, ProblemSet ps, nep_fe_cfg fc, FeAstarArgs aa, FeAstarEntArgs xa, FeEntArgs ea,
                                                                             const nep_fe_start* __restrict__ starts, nep_guess* __restrict__ guess_out, nep_fe_result* __restrict__ res_out) {
  extern __shared__ __attribute__((aligned(16))) double as_team_smem[];
  const AstarEntTeamLayout TL = astar_ent_team_layout();      // (lds_layout.h)
  const AstarEntLayout& AL = TL.one;
  AsTeamState* const s_work = lds_rec<AsTeamState>(as_team_smem, AL.work);
  double (*const s_ch)[17] = (double(*)[17])lds_at<double>(as_team_smem, AL.ch);
  double* const s_hcost = lds_at<double>(as_team_smem, AL.hcost); double* const s_lat = lds_at<double>(as_team_smem, AL.lat);
  int* const s_heap = lds_at<int>(as_team_smem, AL.heap);
  int* const s_vx = lds_at<int>(as_team_smem, AL.ints); int* const s_vy = s_vx + kAsNC; unsigned* const s_iz = (unsigned*)(s_vy + kAsNC);
  int* const s_f = s_vy + 2 * kAsNC; int* const s_pos = s_f + kAsNC; int* const s_hst = s_pos + kAsNC; int* const s_hidx = s_hst + kAsNC;
  int* const s_new = s_hidx + kAsNC; int* const s_grp = s_new + kAsNC; int* const s_valid = s_grp + kAsNC;
  int* const s_path = lds_at<int>(as_team_smem, AL.path);
  unsigned* const x_hdr = lds_at<unsigned>(as_team_smem, TL.x_hdr); unsigned* const x_pool = lds_at<unsigned>(as_team_smem, TL.x_pool);
  unsigned* const x_stage = lds_at<unsigned>(as_team_smem, TL.x_stage); unsigned* const x_cn = lds_at<unsigned>(as_team_smem, TL.x_cn);
  int* const s_have = lds_at<int>(as_team_smem, TL.have); int* const s_ctl = lds_at<int>(as_team_smem, TL.ctl);

  const int tid = threadIdx.x, lane = tid & 63;
  const bool w0 = tid < 64;      // wave 0: the children's lanes
  if (ps.fe_count && (int)blockIdx.x >= *ps.fe_count) return;      // (an active set: fe_order is the list of active slots)
  const int slot = ps.fe_order ? ps.fe_order[blockIdx.x] : (int)blockIdx.x, scene = slot / sp.n_local, own = sp.first_local + (slot % sp.n_local);
  const int N = sp.num_agents, S = sp.n_static, ns = fc.num_samples, NC = ns * ns, D = sp.num_pol;
  const int nse = ea.ns < kAsTeamSteps ? ea.ns : kAsTeamSteps;      // (ent_samples <= 8: the entry point's check)
  const int cap = aa.pool, mask = aa.tab_cap - 1;
  AsNode* const pool = (AsNode*)aa.nodes + (size_t)slot * cap;
  const AsHeap hp{s_heap, aa.heap + (size_t)slot * cap};
  unsigned long long* const tkey = aa.tab_key + (size_t)slot * aa.tab_cap;
  int* const tval = aa.tab_val + (size_t)slot * aa.tab_cap;
  const nep_fe_start* st = starts + slot;
  const double gx = st->goal[0], gy = st->goal[1];
  const double bx = ps.pb[2 * own], by = ps.pb[2 * own + 1];
  const double init[6] = {st->pos[0], st->pos[1], st->vel[0], st->vel[1], st->accel[0], st->accel[1]};
  AsTeamState* const spool = (AsTeamState*)xa.states + (size_t)slot * cap;
  unsigned* const tiz = xa.tab_iz + (size_t)slot * aa.tab_cap;
  const nep_fe_ent_state* const root_state = ea.init ? ea.init + slot : nullptr;
  const bool root_ok = !root_state || as_ent_init_ok(root_state);      // (a malformed state at A: the search starts from the empty one, flagged)
  EntCtx ec;
  ec.N = N; ec.S = S; ec.own = own; ec.num_pol = D; ec.ns = ea.ns; ec.T_span = sp.T_span; ec.cable = fc.cable_length;
  ec.pb = ps.pb; ec.srep = ea.srep + (long)scene * sp.static_stride * 4; ec.slong = ea.slong + (long)scene * sp.static_stride * 2;
  ec.sampled = ea.sampled; ec.present = ea.present;
  ec.ps = &ps; ec.scene = scene; ec.n_hull = sp.n_hull;
  ec.packed = ea.packed; ec.pk_stride = ea.pk_stride;
#ifdef NEP_PROFILE_PHASES
  long long tph[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long long tlast = clock64();      // thread 0's: pop, GJK (+ bases), fe_child, the dense crossing pass, surgery + lookup + group, commit, state copy, (setup + result)
#define AS_TICK(k) do { const long long t_ = clock64(); tph[k] += t_ - tlast; tlast = t_; } while (0)
#else
#define AS_TICK(k) do { } while (0)
#endif
  for (int k = tid; k <= mask; k += kAsTeamThreads) tval[k] = -1;
  if (tid < NEP_FE_MAX_SAMPLES) fe_lattice_fill(sp, fc, s_lat, tid);
  if (tid == 0) s_ctl[kTcOcc] = 0;
  const FeLattice lat{s_lat, s_lat + NEP_FE_MAX_SAMPLES, s_lat + 2 * NEP_FE_MAX_SAMPLES, s_lat + 3 * NEP_FE_MAX_SAMPLES};
  __syncthreads();
  // goal_occupied_ (setUp :210-226)
  {
    bool occ = false;
    Pts4 G; const double r = 0.5;
    G.x[0] = gx + r; G.y[0] = gy + r; G.x[1] = gx + r; G.y[1] = gy - r; G.x[2] = gx - r; G.y[2] = gy + r; G.x[3] = gx - r; G.y[3] = gy - r;
    for (int j = tid; j < N; j += kAsTeamThreads) {
      if (j == own) continue;
      const HullRef hr = hull_ref(ps, sp.n_hull, scene, j);
      const long h = hr.e * sp.num_pol + (D - 1);
      const int nv = blk(ps.hull_nv, hr.boff)[h];
      if (nv > 0 && gjk_collision(nv, blk(ps.hull_xy, hr.boff) + h * kHullV * 2, G)) occ = true;
    }
    if (occ) s_ctl[kTcOcc] = 1;
  }
  __syncthreads();
  const bool goal_occupied = s_ctl[kTcOcc] != 0;

  // what thread 0 keeps: the heap's length, nodes created, the update toggle, the counters of the children it walked past
  int heap_n = 0, used = 0, ran_trigger = 0, capped = 0, n_entangled = 0, overflow = root_ok ? 0 : 1;
  int status = NEP_FE_EMPTY, cur = -1, closest = -1, pops = 0;      // (uniform over the workgroup)
  double smallest = 1.7976931348623157e308;
  AS_TICK(7);

  // both expandAndAddToQueue overloads (:1045-1228, :1240-1385): e_cur < 0 = from the initial state
  auto expand = [&](int e_cur, const double* pe, double pg, int pindex) {
    const bool first = e_cur < 0;
    // (0) the parent's state, staged once for every child's copy
    if (tid < kAsEntWords) {
      long v = 0;
      if (!first) v = ((const long*)(spool + e_cur))[tid];
      else if (root_state && root_ok) v = ((const long*)root_state)[tid];
      ((long*)(s_work + kAsNC))[tid] = v;
    }
    // (1a) wave 0: every lane its child (the kinodynamic tests); the children with "have" in lattice order
    FeChild ch; bool have = false;
    if (w0 && lane < NC) {
      const int comb = aa.order ? aa.order[lane] : lane;
      have = fe_child(sp, fc, lat, pe, pg, first, comb / ns, comb % ns, gx, gy, bx, by, ch);
      if (have) {
        double* o = s_ch[lane];
#pragma unroll
        for (int i = 0; i < 6; i++) o[i] = ch.e[i];
#pragma unroll
        for (int i = 0; i < 4; i++) { o[6 + i] = ch.cx[i]; o[10 + i] = ch.cy[i]; }
      }
    }
    {      // (every wave takes the ballot: no wave-wide operation under a branch; wave 0's is the one that counts)
      const unsigned long long hm = __ballot(have);
      if (have) s_have[__popcll(hm & ((1ull << lane) - 1ull))] = lane;
      if (tid == 0) s_ctl[kTcHave] = __popcll(hm);
    }
    __syncthreads();
    AS_TICK(2);
    // (1b) the dense crossing pass: one work item per (child with "have", sampled step, chunk of [0, N + S))
    const int n_cs = s_ctl[kTcHave] * nse;      // <= kAsNC * kAsTeamSteps <= kAsTeamThreads
    int C = n_cs > 0 ? kAsTeamThreads / n_cs : 1;
    C = C > kAsTeamChunks ? kAsTeamChunks : C;
    const bool item = tid < n_cs * C;
    const int cs = tid / C, c = tid - cs * C;      // the (child, step) pair and the chunk
    AsTeamAdd add; add.attach(EntAdd::Store{x_stage + tid * (kEntAddCap - EntAdd::reg), kEntAddCap}); add.clear();
    add.r0 = add.r1 = add.r2 = add.r3 = 0u;
    if (item) {
      const int q = s_have[cs / nse], j = cs % nse + 1, index = pindex + 1;
      const double* o = s_ch[q];
      const double cxo[4] = {o[6], o[7], o[8], o[9]}, cyo[4] = {o[10], o[11], o[12], o[13]};
      const Ev2 end{o[0], o[1]};
      const Ev2 pk = ent_step_point(ec, cxo, cyo, end, j - 1), pk1 = ent_step_point(ec, cxo, cyo, end, j);
      const int U = N + S, u0 = (int)((long)c * U / C), u1 = (int)((long)(c + 1) * U / C);
      const int a0 = u0 < N ? u0 : N, a1 = u1 < N ? u1 : N, s0 = (u0 > N ? u0 : N) - N, s1 = (u1 > N ? u1 : N) - N;
      // the agents of the chunk: ent_propagate's visit of a packed record, operand for operand
      const Ev2 pb_self = ent_pb(ec, own);
      const int itv = index > D ? D - 1 : index - 1;
      const int jl = index > D ? ec.ns : j - 1, jr = index > D ? ec.ns : j;
      for (int i = a0; i < a1; i++) {
        if (i == own) continue;
        const double* r = ent_rec(ec, i, itv);
        const int2 hd = *(const int2*)r;
        if (!hd.x) continue;
        const double2 sa = *(const double2*)(r + kEntPkHead + 2 * jl), sb = *(const double2*)(r + kEntPkHead + 2 * jr), b0 = *(const double2*)(r + kEntPkBend), b1 = *(const double2*)(r + kEntPkBend + 2);
        ent_cross_agent(add, pk, pk1, Ev2{sa.x, sa.y}, Ev2{sb.x, sb.y}, pb_self, hd.y, r + kEntPkBend, i + 1, -1, true, Ev2{b0.x, b0.y}, Ev2{b1.x, b1.y});
      }
      // ... and its statics: ent_cross_static over [s0, s1) (it reads N for the ids, S and srep: a view of the context that starts at s0)
      if (s1 > s0) {
        EntCtx es = ec; es.N = N + s0; es.S = s1 - s0; es.srep = ec.srep + (long)s0 * 4;
        ent_cross_static(add, pk, pk1, es);
      }
      x_cn[tid] = (unsigned)add.n | ((unsigned)add.peak << 8) | ((unsigned)(add.overflow != 0) << 16);
    }
    __syncthreads();
    // (1c) a (child, step)'s list: its chunks' lists one behind the other; the capacity flag from base + peak (see the head of this kernel)
    if (item) {
      int base = 0, total = 0; bool ovf = false;
      for (int k = 0; k < C; k++) {
        const unsigned w = x_cn[cs * C + k];
        const int nk = (int)(w & 0xffu), pk_ = (int)((w >> 8) & 0xffu);
        if (k == c) base = total;
        ovf = ovf || ((w >> 16) & 1u) || total + pk_ > kEntAddCap;
        total += nk;
      }
      if (!ovf) for (int k = 0; k < add.n; k++) x_pool[cs * kEntAddCap + base + k] = add.get(k);      // (base + n <= total <= kEntAddCap)
      if (c == 0) x_hdr[s_have[cs / nse] * kAsTeamSteps + cs % nse] = ovf ? kEntHdrOvf : ((unsigned)(cs * kEntAddCap) | ((unsigned)total << 16));
    }
    __syncthreads();
    AS_TICK(3);
    // (1d) wave 0: every child its surgery from the parent's state, the costs and iz; the node that holds the child's voxel before
    // this expansion (with what the commit reads of it) and the child's voxel group: the first child of this expansion with the same voxel
    {
      int my_f = -2, my_vx = 0, my_vy = 0; unsigned my_iz = 0u;      // -2: no child; -3: entangled; -4: beyond the fixed record
      if (w0 && lane < NC) {
        if (have) {
          AsTeamState* w = s_work + lane;
          { const long* s_ = (const long*)(s_work + kAsNC); long* d_ = (long*)w;
#pragma unroll
            for (int i = 0; i < kAsEntWords; i++) d_[i] = s_[i]; }
          double arc = 0.0;
          // (no header of this kernel carries kEntHdrGlobal: the blocks' pointer is never read.  It is the pool, not null — with a
          // constant null the compiler sees loads from address zero on that path and its CFG simplification crashes)
          const int rc = ent_propagate_pre(ec, w, x_hdr + lane * kAsTeamSteps, x_pool, x_pool, kEntAddCap, ch.cx, ch.cy, Ev2{ch.e[0], ch.e[1]}, arc, true, 1);
          if (rc == 1) my_f = -3;
          else if (rc != 0) my_f = -4;
          else {
            const double g = pg + arc;
            const double h = (ch.dist + 0.3 * (double)w->n_alpha) + 1.0 * (double)w->n_bend;      // (:1177-1182)
            const double f = g + fc.bias * h;
            my_iz = ent_iz(w);
            double* o = s_ch[lane];      // (end state and polynomial are there since (1a))
            o[14] = g; o[15] = h; o[16] = f;
            my_vx = ch.vx; my_vy = ch.vy;
            s_vx[lane] = ch.vx; s_vy[lane] = ch.vy;
            s_iz[lane] = my_iz; s_valid[lane] = ent_valid_endpoint(w, N) ? 1 : 0;
            const unsigned long long key = as_key(ch.vx, ch.vy);
            int pos = -1;
            my_f = as_find<true>(tkey, tiz, tval, mask, key, my_iz, (int)(fe_hash((long long)(key ^ ((unsigned long long)my_iz * 0xC2B2AE3D27D4EB4Full))) & (unsigned)mask), pos);
            s_pos[lane] = pos;
            if (my_f >= 0) { s_hst[lane] = pool[my_f].state; s_hidx[lane] = pool[my_f].index; s_hcost[lane] = pool[my_f].cost; }
          }
        }
        s_f[lane] = my_f; s_new[lane] = -1;
      }
      int grp = lane;
      for (int r = 0; r < NC; r++) {      // (r is wave-uniform: the shuffles are lane reads; taken by every wave, used by wave 0)
        const int fr = __shfl(my_f, r), xr = __shfl(my_vx, r), yr = __shfl(my_vy, r);
        const bool same = fr >= -1 && xr == my_vx && yr == my_vy && (unsigned)__shfl((int)my_iz, r) == my_iz;
        if (r < lane && grp == lane && same) grp = r;
      }
      if (w0 && lane < NC) s_grp[lane] = grp;
    }
    __syncthreads();
    AS_TICK(4);
    // (2) thread 0 commits the survivors in lattice order (frontend_astar_kernel's loop)
    if (tid == 0) {
      for (int q = 0; q < NC; q++) {
        if (used >= cap - 1) { if (cap < kAsMaxNodes) capped = 1; break; }      // "run out of memory" (:1061-1065), at the handle's pool when that is smaller
        int f = s_f[q];
        if (f == -2) continue;
        if (f == -3) { n_entangled++; continue; }
        if (f == -4) { overflow = 1; continue; }
        const double* c_ = s_ch[q];
        const int vx = s_vx[q], vy = s_vy[q], grp = s_grp[q];
        const unsigned iz = s_iz[q];
        int pos = s_pos[q];
        if (!first) {
          int hst, hidx;
          if (f >= 0) { hst = s_hst[q]; hidx = s_hidx[q]; }
          else { hst = 1; hidx = pindex + 1; if (grp != q) f = s_new[grp]; }      // (the group's first child took the voxel in this commit: open, of this index)
          if (f >= 0) {
            if (hst == 1 && hidx == pindex + 1) {
              if (c_[16] < s_hcost[grp] && (ran_trigger & 1) == 0) {      // update the open node in place (:1190-1203): not its entangle state (:1204), not the heap
                AsNode* o = pool + f;
                o->prev = e_cur; o->g = c_[14]; o->h = c_[15]; o->cost = c_[16];
                for (int i = 0; i < 6; i++) o->end[i] = c_[i];
                for (int i = 0; i < 4; i++) { o->cx[i] = c_[6 + i]; o->cy[i] = c_[10 + i]; }
                s_hcost[grp] = c_[16];
              }
              ran_trigger++;
            }
            continue;
          }
        }
        AsNode* nb = pool + used;
        nb->h = c_[15]; nb->cost = c_[16]; nb->g = c_[14];
        for (int i = 0; i < 6; i++) nb->end[i] = c_[i];
        for (int i = 0; i < 4; i++) { nb->cx[i] = c_[6 + i]; nb->cy[i] = c_[10 + i]; }
        nb->prev = e_cur; nb->state = 1; nb->index = pindex + 1; nb->vx = vx; nb->vy = vy;
        nb->_pad = s_valid[q];
        as_push_heap(hp, pool, heap_n, used, c_[16], c_[15]); heap_n++;
        // unordered_map::insert keeps the first: the walk goes on from where the lookup ended (entries are never removed)
        const unsigned long long key = as_key(vx, vy);
        if (as_find<true>(tkey, tiz, tval, mask, key, iz, pos >= 0 ? pos : 0, pos) < 0 && pos >= 0) { tkey[pos] = key; tval[pos] = used; tiz[pos] = iz; }
        s_new[q] = used; s_hcost[q] = c_[16];
        used++;
      }
    }
    __syncthreads();
    AS_TICK(5);
    // (3) the states of the nodes this commit created, into the pool: 8 bytes per thread (s_new[q] < cap - 1: inside the pool)
    for (int k = tid; k < NC * kAsEntWords; k += kAsTeamThreads) {
      const int q = k / kAsEntWords, wd = k - q * kAsEntWords, n = s_new[q];
      if (n >= 0) ((long*)(spool + n))[wd] = ((const long*)(s_work + q))[wd];
    }
    __syncthreads();
    AS_TICK(6);
  };

  expand(-1, init, 0.0, 0);
  const int max_pops = aa.max_pops;
  const double base_radius = 0.7, safe_dist = (sp.T_span * sp.v_max) * 2;
  for (;;) {
    // thread 0 pops, or says why not; the verdict word of this pop's parity is cleared (its last reader is two barriers back)
    if (tid == 0) {
      int go = 1;
      if (heap_n <= 0) go = 0;
      else if (pops >= max_pops) go = 2;
      else { cur = as_pop(hp, pool, heap_n); pool[cur].state = -1; }
      s_ctl[kTcGo] = go; s_ctl[kTcCur] = cur; s_ctl[kTcHit + (pops & 1)] = 0;
    }
    __syncthreads();
    const int go = s_ctl[kTcGo];
    if (go == 0) break;
    if (go == 2) { status = NEP_FE_DEPTH_REACHED; break; }       // RUNTIME_REACHED: the budget (:1644-1651)
    cur = s_ctl[kTcCur];
    int* const s_hit = s_ctl + kTcHit + (pops & 1);
    pops++;
    AS_TICK(0);
    const AsNode* nd = pool + cur;
    const int index = nd->index;
    const bool valid = nd->_pad != 0;
    double pe[6], cx[4], cy[4];
#pragma unroll
    for (int i = 0; i < 6; i++) pe[i] = nd->end[i];
#pragma unroll
    for (int i = 0; i < 4; i++) { cx[i] = nd->cx[i]; cy[i] = nd->cy[i]; }
    const double pg = nd->g;
    // collidesWithObstacles2dSolve (:1514-1553) and collidesWithBases2d (:1583-1628): the control polygon against every other agent's
    // hull of the node's interval, every static polygon and every other agent's base square, strided over the workgroup
    Pts4 B;
    fe_pos_cps(cx, sp.T_span, B.x); fe_pos_cps(cy, sp.T_span, B.y);
    const int idx = (index > D ? D : index) - 1;
    bool hit = false;
    for (int o = tid; o < N + S + N; o += kAsTeamThreads) {
      if (o < N + S) {
        int nv; const double* V;
        if (o < N) {
          if (o == own) continue;
          const HullRef hr = hull_ref(ps, sp.n_hull, scene, o); const long h = hr.e * sp.num_pol + idx;
          nv = blk(ps.hull_nv, hr.boff)[h]; V = blk(ps.hull_xy, hr.boff) + h * kHullV * 2;
        } else { const long js = (long)scene * sp.static_stride + (o - N); nv = ps.static_nv[js]; V = ps.static_xy + js * kHullV * 2; }
        if (nv > 0 && gjk_collision(nv, V, B)) hit = true;
      } else {
        const int j = o - N - S;
        if (j == own) continue;
        const double pbx = ps.pb[2 * j], pby = ps.pb[2 * j + 1];
        const double d1 = sqrt((B.x[0] - pbx) * (B.x[0] - pbx) + (B.y[0] - pby) * (B.y[0] - pby));
        if (d1 > safe_dist) continue;
        const double sq[8] = {pbx + base_radius, pby + base_radius, pbx + base_radius, pby - base_radius, pbx - base_radius, pby - base_radius, pbx - base_radius, pby + base_radius};
        if (gjk_collision(4, sq, B)) hit = true;
      }
    }
    if (hit) *s_hit = 1;
    __syncthreads();
    const bool collides = *s_hit != 0;
    AS_TICK(1);
    if (collides) continue;
    const double dist = sqrt((pe[0] - gx) * (pe[0] - gx) + (pe[1] - gy) * (pe[1] - gy));
    const double dfi = sqrt((pe[0] - init[0]) * (pe[0] - init[0]) + (pe[1] - init[1]) * (pe[1] - init[1]));
    const double dtc = goal_occupied ? dist * dist : dfi;
    const double dti = dtc * (double)index;
    if (valid && dti < smallest) { smallest = dti; closest = cur; }      // (:1683-1700)
    if (valid && dist < fc.goal_size) { status = NEP_FE_GOAL_REACHED; break; }
    expand(cur, pe, pg, index);
  }

  const int best = status == NEP_FE_GOAL_REACHED ? cur : closest;        // use_not_reaching_soln (every thread holds cur and closest)
  if (tid == 0) {
    if (best < 0) status = NEP_FE_NO_SOLUTION;
    nep_guess* g = guess_out + slot;
    for (int e = 0; e < 3 * NEP_MAX_POL * 4; e++) (&g->coeff[0][0][0])[e] = 0.0;
    g->t_start = st->t_start; g->n_alpha = 0;
    int K = 0, depth = 0, rows = 0; double cost = 0.0, dtg = 0.0;
    for (int d = 0; d <= NEP_MAX_POL; d++) s_path[d] = -1;
    if (best >= 0) {
      const AsNode* b = pool + best;
      depth = b->index; K = depth < D ? depth : D; cost = b->cost;
      dtg = sqrt((b->end[0] - gx) * (b->end[0] - gx) + (b->end[1] - gy) * (b->end[1] - gy));
      // recoverPwpOut (:521-553): the nodes of the path with index <= num_pol (a node's index is its place on its path)
      int k = best;
      for (int it = 0; it < cap && k >= 0; it++) {
        const AsNode* q = pool + k;
        const int d = q->index;
        if (d >= 1 && d <= D) {
          s_path[d] = k;
          for (int c = 0; c < 4; c++) { g->coeff[0][d - 1][c] = q->cx[c]; g->coeff[1][d - 1][c] = q->cy[c]; }
        }
        k = q->prev;
      }
      int Kg = K;
      if (fc.pad_hold && K < D) {   // hold the end point for the rest of the horizon; the held segments keep the returned node's state
        for (int d = K + 1; d <= D; d++) { g->coeff[0][d - 1][3] = b->end[0]; g->coeff[1][d - 1][3] = b->end[1]; s_path[d] = best; }
        Kg = D;
      }
      fe_initial_z(st->pos[2], st->vel[2], st->accel[2], st->goal[2], sp.T_span, D, sp.v_max, sp.a_max, g->coeff[2]);   // coeffs_z_ (:540)
      for (int d = Kg + 1; d <= D; d++) for (int c = 0; c < 4; c++) g->coeff[2][d - 1][c] = 0.0;
      K = Kg; rows = Kg;
    }
    s_path[NEP_MAX_POL + 1] = rows;
    g->K = K;
    if (capped && ps.flags) atomicOr(ps.flags, NEP_FLAG_FE_ASTAR_POOL);
    if (overflow && ps.flags) atomicOr(ps.flags, NEP_FLAG_FE_ASTAR_ENT_REC);
    if (res_out) {
      nep_fe_result* o = res_out + slot;
      o->status = status; o->K = K; o->depth = depth; o->n_children = pops; o->n_feasible = used; o->n_collision_free = 0;
      o->goal_occupied = goal_occupied ? 1 : 0; o->_pad = capped ? kAsPadPool : 0;
      o->cost = cost; o->dist_to_goal = dtg; o->n_entangled = n_entangled; o->ent_overflow = overflow;
    }
  }
  // the case block (solver_gurobi_poly.cpp:624-631): row i from the state at the START of segment i, one agent per thread
  __syncthreads();
  if (ea.case_out) {
    const int rows = s_path[NEP_MAX_POL + 1];
    int* const co = ea.case_out + (size_t)slot * NEP_MAX_POL * N;
    for (int i = 0; i < NEP_MAX_POL; i++) {
      const nep_fe_ent_state* sn = nullptr;
      if (i < rows) { if (i == 0) sn = (root_state && root_ok) ? root_state : nullptr; else if (s_path[i] >= 0) sn = spool + s_path[i]; }
      const int na = sn ? sn->n_alpha : 0;
      for (int j = tid; j < N; j += kAsTeamThreads) {
        int cs = 0, cnt = 0;
        for (int a = 0; a < na; a++) if (sn->id[a] == j + 1) { cnt++; cs = sn->cs[a]; }
        co[(size_t)i * N + j] = cnt == 1 ? cs : 0;
      }
    }
  }
#ifdef NEP_PROFILE_PHASES
  AS_TICK(7);
  if (tid == 0 && ps.dbg) { for (int k = 0; k < 8; k++) ps.dbg[(long)slot * 32 + k] = tph[k]; ps.dbg[(long)slot * 32 + 8] = pops; ps.dbg[(long)slot * 32 + 9] = used; }
#endif
#undef AS_TICK
}
