// fe_astar_ent.h — the reference's best-first search WITH enable_entangle_check as a device kernel.  Included by
// geom_kernels.hip, inside namespace nep, below fe_astar.h: it uses that header's heap (AsHeap, as_comp, as_push_heap, as_pop), node
// (AsNode) and constants, the beam front end's fe_child, fe_lattice_fill, fe_pos_cps, gjk_collision, hull_ref, fe_initial_z,
// ent_pack_kernel and skipped_fe_kernel, ent_device.h's ent_propagate, ent_iz, ent_valid_endpoint and ent_copy, and that object's
// -ffp-contract=off.  frontend_astar_kernel itself is not touched: this is a second kernel, not an instantiation of it.
//
// KinodynamicSearch::run as fe_astar.h runs it, plus what enable_entangle_check adds (tests/astar_ent_ref.py is the rule, bit for bit):
//   child       the parent's state (the root: the state at A) through entanglesWithOtherAgents (kinodynamic_search.cpp:1157-1182,
//               :1341-1360); true drops the child (n_entangled).  g = parent g + sampled arc length, h = (dist + 0.3 crossings) + 1.0 bends
//   voxel       (ix, iy, getIz(state)) (:2006-2031), for the root expansion's inserts too (:1367-1377)
//   update      an open node of the same index updated in place keeps ITS entangle state (:1204 is commented out)
//   pop         the hulls and statics, then the other agents' base squares (collidesWithBases2d, :1583-1628); closest-so-far and the
//               goal test both ask for a valid end point (every active_cases <= 1, :1693-1700); an invalid node at the goal is expanded
//   result      the guess as fe_astar.h; the case block from the states along the returned path (state at the START of segment i;
//               with pad_hold the held segments keep the returned node's); n_children = pops, n_feasible = nodes created
//   capacity    a node's state is a fixed record (nep_fe_ent_state): a child whose list would outgrow NEP_FE_ENT_CAP, whose sampled
//               step adds more than 32 crossings or whose bend points exceed NEP_MAX_BEND is dropped, not counted in n_entangled, and
//               sets nep_fe_result.ent_overflow and NEP_FLAG_FE_ASTAR_ENT_REC (NEP_E_CAP from nep_batch_check) — a stated deviation
//
// One wave per search, fe_astar.h's split.  Per lane: fe_child, then the entangle propagation of its child in a working record in LDS
// (copied from the parent's state, which the wave stages once per expansion), iz, h and g, the voxel lookup and the voxel group —
// all before the commit.  Lane 0 commits in lattice order as before (the counters of pruned children are kept there too: the node
// cap cuts an expansion at a child, and the children behind it were never looked at in the reference).  The wave then copies the
// states of the nodes that commit created into the state pool, 8 bytes per lane.  At a pop the obstacle loop runs over the hulls,
// the statics and the base squares, one per lane; whether the node may end a plan was decided when its state was made (AsNode::_pad).
// Per slot, in global memory, beside fe_astar.h's pools: the state pool (NEP_FE_ASTAR_ENT_NODE_BYTES per node) and the table's third
// key word.
#pragma once

static_assert(kAsEntNC == kAsNC && kAsEntHeapLds == kAsHeapLds, "lds_layout.h states this kernel's carve with fe_astar.h's constants");
static_assert(sizeof(nep_fe_ent_state) == NEP_FE_ASTAR_ENT_NODE_BYTES && sizeof(nep_fe_ent_state) % 8 == 0, "a node's state in the pool is the fixed record: part of nep_batch_frontend_astar_ent's memory contract");
constexpr int kAsEntWords = (int)(sizeof(nep_fe_ent_state) / 8);      // a state as 8-byte words: the wave copies one with its first 57 lanes
static_assert(kAsEntWords <= 64, "one lane per 8-byte word of a state");

// The list of a sampled step's new crossings: EntAdd under a name of this kernel's own, so that ent_propagate and what it calls are
// instantiated for this kernel alone — sharing ent_check_kernel's instantiation changed that kernel's code (its callee got a second caller).
struct AsEntAdd : EntAdd { };
// node of voxel (key, iz), or -1; pos: where it is / where it would go (the table is never more than half full: the walk ends)
__device__ __forceinline__ int as_find3(const unsigned long long* tkey, const unsigned* tiz, const int* tval, int mask, unsigned long long key, unsigned iz, int start, int& pos) {
  int p = start;
  for (int it = 0; it <= mask; it++, p = (p + 1) & mask) {
    const int v = tval[p];
    if (v < 0 || (tkey[p] == key && tiz[p] == iz)) { pos = p; return v < 0 ? -1 : v; }
  }
  pos = -1; return -1;
}
// a state at A the search can start from: counts within the fixed record, bend indices on the list
__device__ __forceinline__ bool as_ent_init_ok(const nep_fe_ent_state* s) {
  if (s->n_alpha < 0 || s->n_alpha > NEP_FE_ENT_CAP || s->n_bend < 0 || s->n_bend > NEP_MAX_BEND) return false;
  for (int k = 0; k < s->n_bend; k++) if (s->bend[k] < 0 || s->bend[k] >= s->n_alpha) return false;
  return true;
}

__global__ __launch_bounds__(64) void frontend_astar_ent_kernel(SceneParams sp, ProblemSet ps, nep_fe_cfg fc, FeAstarArgs aa, FeAstarEntArgs xa, FeEntArgs ea,
                                                                const nep_fe_start* __restrict__ starts, nep_guess* __restrict__ guess_out, nep_fe_result* __restrict__ res_out) {
  extern __shared__ __attribute__((aligned(16))) double as_smem[];
  const AstarEntLayout AL = astar_ent_layout();      // (lds_layout.h)
  nep_fe_ent_state* s_work = lds_rec<nep_fe_ent_state>(as_smem, AL.work);      // [kAsNC] the children's states; [kAsNC]: the parent's
  double (*s_ch)[17] = (double(*)[17])lds_at<double>(as_smem, AL.ch);
  double* s_hcost = lds_at<double>(as_smem, AL.hcost);
  double* s_lat = lds_at<double>(as_smem, AL.lat);
  int* s_heap = lds_at<int>(as_smem, AL.heap);
  int* s_vx = lds_at<int>(as_smem, AL.ints); int* s_vy = s_vx + kAsNC; unsigned* s_iz = (unsigned*)(s_vy + kAsNC); int* s_f = s_vy + 2 * kAsNC; int* s_pos = s_f + kAsNC;
  int* s_hst = s_pos + kAsNC; int* s_hidx = s_hst + kAsNC; int* s_new = s_hidx + kAsNC; int* s_grp = s_new + kAsNC; int* s_valid = s_grp + kAsNC;
  int* s_path = lds_at<int>(as_smem, AL.path);
  const int lane = threadIdx.x;
  if (ps.fe_count && (int)blockIdx.x >= *ps.fe_count) return;      // (an active set: fe_order is the list of active slots)
  const int slot = ps.fe_order ? ps.fe_order[blockIdx.x] : (int)blockIdx.x, scene = slot / sp.n_local, own = sp.first_local + (slot % sp.n_local);
  const int N = sp.num_agents, S = sp.n_static, ns = fc.num_samples, NC = ns * ns, D = sp.num_pol;
  const int cap = aa.pool, mask = aa.tab_cap - 1;
  AsNode* const pool = (AsNode*)aa.nodes + (size_t)slot * cap;
  nep_fe_ent_state* const spool = (nep_fe_ent_state*)xa.states + (size_t)slot * cap;
  const AsHeap hp{s_heap, aa.heap + (size_t)slot * cap};
  unsigned long long* const tkey = aa.tab_key + (size_t)slot * aa.tab_cap;
  unsigned* const tiz = xa.tab_iz + (size_t)slot * aa.tab_cap;
  int* const tval = aa.tab_val + (size_t)slot * aa.tab_cap;
  const nep_fe_start* st = starts + slot;
  const double gx = st->goal[0], gy = st->goal[1];
  const double bx = ps.pb[2 * own], by = ps.pb[2 * own + 1];
  const double init[6] = {st->pos[0], st->pos[1], st->vel[0], st->vel[1], st->accel[0], st->accel[1]};
  const nep_fe_ent_state* const root_state = ea.init ? ea.init + slot : nullptr;
  const bool root_ok = !root_state || as_ent_init_ok(root_state);      // (a malformed state at A: the search starts from the empty one, flagged)
  EntCtx ec;
  ec.N = N; ec.S = S; ec.own = own; ec.num_pol = D; ec.ns = ea.ns; ec.T_span = sp.T_span; ec.cable = fc.cable_length;
  ec.pb = ps.pb; ec.srep = ea.srep + (long)scene * sp.static_stride * 4; ec.slong = ea.slong + (long)scene * sp.static_stride * 2;
  ec.sampled = ea.sampled; ec.present = ea.present;
  ec.ps = &ps; ec.scene = scene; ec.n_hull = sp.n_hull;
  ec.packed = ea.packed; ec.pk_stride = ea.pk_stride;
#ifdef NEP_PROFILE_PHASES
  long long tph[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long long tlast = clock64();      // pop, GJK + bases, fe_child, propagation, lookup + group, commit, state copy, (setup + result)
#define ASE_TICK(k) do { const long long t_ = clock64(); tph[k] += t_ - tlast; tlast = t_; } while (0)
#else
#define ASE_TICK(k) do { } while (0)
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

  // what lane 0 keeps: the heap's length, nodes created, the update toggle, the counters of the children it walked past
  int heap_n = 0, used = 0, ran_trigger = 0, capped = 0, n_entangled = 0, overflow = root_ok ? 0 : 1;
  int status = NEP_FE_EMPTY, cur = -1, closest = -1, pops = 0;
  double smallest = 1.7976931348623157e308;
  ASE_TICK(7);

  // both expandAndAddToQueue overloads (:1045-1228, :1240-1385): e_cur < 0 = from the initial state
  auto expand = [&](int e_cur, const double* pe, double pg, int pindex) {
    const bool first = e_cur < 0;
    // (0) the parent's state, staged once for every lane's copy
    if (lane < kAsEntWords) {
      long v = 0;
      if (!first) v = ((const long*)(spool + e_cur))[lane];
      else if (root_state && root_ok) v = ((const long*)root_state)[lane];
      ((long*)(s_work + kAsNC))[lane] = v;
    }
    __syncthreads();
    // (1) every lane its child: the kinodynamic tests, the entangle propagation from the parent's state, the costs and the voxel
    // with its iz, then the node that holds that voxel before this expansion and the child's voxel group
    int my_f = -2, my_vx = 0, my_vy = 0; unsigned my_iz = 0u;      // -2: no child; -3: entangled; -4: beyond the fixed record
    if (lane < NC) {
      const int comb = aa.order ? aa.order[lane] : lane;
      FeChild ch;
      const bool have = fe_child(sp, fc, lat, pe, pg, first, comb / ns, comb % ns, gx, gy, bx, by, ch);
      ASE_TICK(2);
      if (have) {
        nep_fe_ent_state* w = s_work + lane;
        ent_copy(w, s_work + kAsNC);
        double arc = 0.0;
        unsigned add_tail[kEntAddCap - EntAdd::reg];
        const int rc = ent_propagate<AsEntAdd>(ec, w, AsEntAdd::Store{add_tail, kEntAddCap}, ch.cx, ch.cy, Ev2{ch.e[0], ch.e[1]}, pindex + 1, arc, true, 1);
        ASE_TICK(3);
        if (rc == 1) my_f = -3;
        else if (rc != 0) my_f = -4;
        else {
          const double g = pg + arc;
          const double h = (ch.dist + 0.3 * (double)w->n_alpha) + 1.0 * (double)w->n_bend;      // (:1177-1182)
          const double f = g + fc.bias * h;
          my_iz = ent_iz(w);
          double* o = s_ch[lane];
#pragma unroll
          for (int i = 0; i < 6; i++) o[i] = ch.e[i];
#pragma unroll
          for (int i = 0; i < 4; i++) { o[6 + i] = ch.cx[i]; o[10 + i] = ch.cy[i]; }
          o[14] = g; o[15] = h; o[16] = f;
          my_vx = ch.vx; my_vy = ch.vy;
          s_vx[lane] = ch.vx; s_vy[lane] = ch.vy; s_iz[lane] = my_iz; s_valid[lane] = ent_valid_endpoint(w, N) ? 1 : 0;
          const unsigned long long key = as_key(ch.vx, ch.vy);
          int pos = -1;
          my_f = as_find3(tkey, tiz, tval, mask, key, my_iz, (int)(fe_hash((long long)(key ^ ((unsigned long long)my_iz * 0xC2B2AE3D27D4EB4Full))) & (unsigned)mask), pos);
          s_pos[lane] = pos;
          if (my_f >= 0) { s_hst[lane] = pool[my_f].state; s_hidx[lane] = pool[my_f].index; s_hcost[lane] = pool[my_f].cost; }
        }
      }
      s_f[lane] = my_f; s_new[lane] = -1;
    }
    {
      int grp = lane;
      for (int r = 0; r < NC; r++) {      // (r is wave-uniform: the shuffles are lane reads)
        const int fr = __shfl(my_f, r), xr = __shfl(my_vx, r), yr = __shfl(my_vy, r); const unsigned zr = (unsigned)__shfl((int)my_iz, r);
        if (r < lane && grp == lane && fr >= -1 && xr == my_vx && yr == my_vy && zr == my_iz) grp = r;
      }
      if (lane < NC) s_grp[lane] = grp;
    }
    __syncthreads();
    ASE_TICK(4);
    // (2) lane 0 commits the survivors in lattice order, as frontend_astar_kernel does
    if (lane == 0) {
      for (int q = 0; q < NC; q++) {
        if (used >= cap - 1) { if (cap < kAsMaxNodes) capped = 1; break; }      // "run out of memory" (:1061-1065), at the handle's pool when that is smaller
        int f = s_f[q];
        if (f == -2) continue;
        if (f == -3) { n_entangled++; continue; }
        if (f == -4) { overflow = 1; continue; }
        const double* c = s_ch[q];
        const int vx = s_vx[q], vy = s_vy[q], grp = s_grp[q]; const unsigned iz = s_iz[q];
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
        nb->prev = e_cur; nb->state = 1; nb->index = pindex + 1; nb->vx = vx; nb->vy = vy; nb->_pad = s_valid[q];      // (_pad: may a plan end here)
        as_push_heap(hp, pool, heap_n, used, c[16], c[15]); heap_n++;
        // unordered_map::insert keeps the first: the walk goes on from where the lookup ended (entries are never removed)
        const unsigned long long key = as_key(vx, vy);
        if (as_find3(tkey, tiz, tval, mask, key, iz, pos >= 0 ? pos : 0, pos) < 0 && pos >= 0) { tkey[pos] = key; tiz[pos] = iz; tval[pos] = used; }
        s_new[q] = used; s_hcost[q] = c[16];
        used++;
      }
    }
    __syncthreads();
    ASE_TICK(5);
    // (3) the states of the nodes this commit created, into the pool: the wave, 8 bytes per lane (s_new[q] < cap - 1: inside the pool)
    for (int q = 0; q < NC; q++) {
      const int n = s_new[q];
      if (n >= 0 && lane < kAsEntWords) ((long*)(spool + n))[lane] = ((const long*)(s_work + q))[lane];
    }
    __syncthreads();
    ASE_TICK(6);
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
    ASE_TICK(0);
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
    // hull of the node's interval, every static polygon and every other agent's base square, one per lane
    Pts4 B;
    fe_pos_cps(cx, sp.T_span, B.x); fe_pos_cps(cy, sp.T_span, B.y);
    const int idx = (index > D ? D : index) - 1;
    bool hit = false;
    for (int o = lane; o < N + S + N; o += 64) {
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
    const bool collides = __ballot(hit) != 0ull;
    ASE_TICK(1);
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
        if (d >= 1 && d <= D) { s_path[d] = k; for (int c = 0; c < 4; c++) { g->coeff[0][d - 1][c] = q->cx[c]; g->coeff[1][d - 1][c] = q->cy[c]; } }
        k = q->prev;
      }
      int Kg = K;
      if (fc.pad_hold && K < D) {   // hold the end point for the rest of the horizon (as frontend_kernel does); the held segments keep the returned node's state
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
  __syncthreads();
  // the case block (solver_gurobi_poly.cpp:624-631): row i from the state at the START of segment i — the path's node of index i, the
  // state at A for i = 0 — for the rows of the guess, zero beyond; one agent per lane
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
#ifdef NEP_PROFILE_PHASES
  ASE_TICK(7);
  if (lane == 0 && ps.dbg) { for (int k = 0; k < 8; k++) ps.dbg[(long)slot * 32 + k] = tph[k]; ps.dbg[(long)slot * 32 + 8] = pops; ps.dbg[(long)slot * 32 + 9] = used; }
#endif
#undef ASE_TICK
}

void launch_frontend_astar_ent(int n_slots, const SceneParams& sp, const ProblemSet& ps_in, const nep_fe_cfg& fc, const FeAstarArgs& aa, const FeAstarEntArgs& xa,
                               const FeEntArgs& ea, const nep_fe_start* starts, nep_guess* guess_out, nep_fe_result* res_out, hipStream_t st, int* active_buf) {
  if (n_slots <= 0) return;
  ProblemSet ps = ps_in;
  ps.fe_order = nullptr; ps.fe_count = nullptr;
  if (ps.active && active_buf) {      // an active set: the searches run over the list of active slots; the others get what the beam's launch gives them
    launch_active_list(n_slots, sp, ps.active, nullptr, active_buf, nullptr, st);
    ps.fe_order = active_buf; ps.fe_count = active_buf + n_slots;
    hipLaunchKernelGGL(skipped_fe_kernel, dim3((n_slots + 63) / 64), dim3(64), 0, st, sp, ps.active, n_slots, starts, guess_out, res_out);
  }
  {   // one record per (scene, agent, interval) of what the entangle check reads (ent_pack_kernel)
    const int n_scenes = n_slots / (sp.n_local > 0 ? sp.n_local : 1);
    const long np_ = (long)n_scenes * sp.num_agents * sp.num_pol;
    hipLaunchKernelGGL(ent_pack_kernel, dim3((unsigned)((np_ + 255) / 256)), dim3(256), 0, st, sp, ps, ea, n_scenes);
  }
  hipLaunchKernelGGL(frontend_astar_ent_kernel, dim3(n_slots), dim3(64), (size_t)astar_ent_layout().bytes, st, sp, ps, fc, aa, xa, ea, starts, guess_out, res_out);
}
