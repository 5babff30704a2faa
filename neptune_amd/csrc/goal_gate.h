// goal_gate.h — the reference's move_when_goal_occupied gate (nep_batch_goal_gate, include/neptune_frontend.h; Neptune::replanFull,
// neptune.cpp:1480-1500) as a kernel of its own behind any front end.  Included by geom_kernels.hip after gjk_collision, like fe_astar.h.
//
// A search that did not reach the goal has returned its closest-so-far node (use_not_reaching_soln).  That plan is flown only when the
// goal is occupied by somebody else: the square goal +- r against the LAST interval hull of every other agent, the hulls the preceding
// front-end call left in the handle's scratch.  Otherwise the slot becomes what a search without a first primitive leaves
// (fe_astar.h: best < 0): a zero guess with K = 0 and NEP_FE_NO_SOLUTION, which the replan, the safety pass and fleet_commit_kernel
// already know.
//
// Layout: one wave per slot.  The status is read by every lane from one address (a wave-uniform exit for the slots the gate does not
// examine, which in a flying fleet are most).  Lanes stride over the agents, one GJK per lane, one ballot.  A slot turned down has its
// guess (and its case rows) cleared by all lanes with 16-byte stores; lane 0 writes the words of the result and the counters.
// No LDS, no barrier.  The goal-box loops of frontend_astar_kernel and frontend_kernel stay their own copies: this kernel shares no
// instantiation with them (GateVtx below), so their code does not move.

// the hull's vertices behind a pointer type of this kernel's own: gjk_collision<GateVtx> and gjk_furthest<GateVtx> are instantiated
// for this kernel alone (a second caller of another kernel's out-of-line instantiation changes that kernel's code: fe_astar.h, AsEntAdd)
struct GateVtx {
  const double* p;
  __device__ __forceinline__ double operator[](int i) const { return p[i]; }
};

// n ints at p (4-byte aligned) to zero, by all 64 lanes: 16-byte stores between the first and the last 16-byte boundary
__device__ __forceinline__ void gate_zero(int* p, int n, int lane) {
  int head = (int)((0 - ((size_t)p >> 2)) & 3); if (head > n) head = n;
  if (lane < head) p[lane] = 0;
  int4* const q = (int4*)(p + head); const int nq = (n - head) >> 2;
  for (int e = lane; e < nq; e += 64) q[e] = make_int4(0, 0, 0, 0);
  const int done = head + 4 * nq;
  if (lane < n - done) p[done + lane] = 0;
}

__global__ __launch_bounds__(64) void goal_gate_kernel(SceneParams sp, ProblemSet ps, double r, const nep_fe_start* __restrict__ starts,
                                                       nep_guess* __restrict__ guess, nep_fe_result* __restrict__ res, int* __restrict__ case_out,
                                                       int* __restrict__ count) {
  const int lane = threadIdx.x, slot = blockIdx.x;
  nep_fe_result* const o = res + slot;
  const int status = o->status;
  if (status != NEP_FE_DEPTH_REACHED && status != NEP_FE_EMPTY) return;      // (goal reached, no solution, skipped: not the gate's)
  const int scene = slot / sp.n_local, own = sp.first_local + (slot % sp.n_local);
  const int N = sp.num_agents, D = sp.num_pol;
  const double gx = starts[slot].goal[0], gy = starts[slot].goal[1];
  // the box in the column order of neptune.cpp:1485-1488 (GJK's arithmetic depends on it); obstacle set and indexing: fe_astar.h's goal_occupied_
  bool occ = false;
  {
    Pts4 G;
    G.x[0] = gx + r; G.y[0] = gy + r; G.x[1] = gx + r; G.y[1] = gy - r; G.x[2] = gx - r; G.y[2] = gy + r; G.x[3] = gx - r; G.y[3] = gy - r;
    for (int j = lane; j < N; j += 64) {
      if (j == own) continue;
      const HullRef hr = hull_ref(ps, sp.n_hull, scene, j);
      const long h = hr.e * sp.num_pol + (D - 1);
      const int nv = blk(ps.hull_nv, hr.boff)[h];
      if (nv > 0 && gjk_collision(nv, GateVtx{blk(ps.hull_xy, hr.boff) + h * kHullV * 2}, G)) occ = true;
    }
  }
  const bool taken = __ballot(occ) != 0ull;
  if (taken) {      // somebody is on the goal: the closest-so-far plan goes on to the replan, marked
    if (lane == 0) {
      o->_pad |= NEP_FE_PAD_GOAL_TAKEN;
      if (count) { atomicAdd(count + 4 * scene, 1); atomicAdd(count + 4 * scene + 1, 1); }
    }
    return;
  }
  // the goal is free: replanFull returns false.  The slot becomes a search's NO_SOLUTION (t_start and the search's own figures stay)
  nep_guess* const g = guess + slot;
  gate_zero((int*)&g->coeff[0][0][0], 3 * NEP_MAX_POL * 4 * 2, lane);
  if (case_out) gate_zero(case_out + (size_t)slot * NEP_MAX_POL * N, NEP_MAX_POL * N, lane);
  if (lane == 0) {
    g->K = 0; g->n_alpha = 0;
    o->status = NEP_FE_NO_SOLUTION; o->K = 0; o->_pad |= NEP_FE_PAD_GATED;
    if (count) { atomicAdd(count + 4 * scene, 1); atomicAdd(count + 4 * scene + 2, 1); }
  }
}

void launch_goal_gate(int n_slots, const SceneParams& sp, const ProblemSet& ps, double half_side, const nep_fe_start* starts, nep_guess* guess,
                      nep_fe_result* res, int* case_out, int* count, hipStream_t st) {
  if (n_slots <= 0) return;
  hipLaunchKernelGGL(goal_gate_kernel, dim3(n_slots), dim3(64), 0, st, sp, ps, half_side, starts, guess, res, case_out, count);
}
