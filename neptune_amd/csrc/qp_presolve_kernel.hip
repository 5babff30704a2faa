// qp_presolve_kernel.hip — the zero-iteration half of the verified line presolve as a kernel of its own (round 6).
//
// Since the certificate moved into the separator's wave (qp_presolve.h; separator_packed_kernel's tail, chosen by Engine::run when one
// wave of that kernel holds every segment of a slot: launches of some 4 096 slots and more) this kernel is the small-launch and
// split-API form: fewer slots than that, the unpacked separator, an active set, nep_batch_replan_lines / _solve, the per-agent
// handle, and the debug option "presolve_fused" = 0.  Both forms run the same pieces of qp_presolve.h and write the same bytes.
//
// Under the presolve (nep_batch_set_line_cull, the handle's default) most replans need no interior-point iteration: the minimiser of
// the cost over the equality-reduced variables, z* = -Hax^-1 g per axis, satisfies every box row, every near separating line and
// the terminal ball; with zero multipliers that point meets the KKT conditions of the full problem, so it IS what
// PolySolverGurobi::optimize returns (solver_gurobi_poly.cpp:823-882) — 91 % of the replans of the bench's 64-agent scenes, 87 % at
// config 5.  Until round 5 that test ran at the top of qp_reg_kernel<true>: a workgroup of 256 threads with 36.7 KB of LDS and 128
// registers per lane — an interior point's resources — held one of a CU's four slots for ~20 us to do a 24-variable
// matrix-vector product and a pass over ~500 rows (profiles/r06_qp_phases_default.txt: line gather 26 %, start point 16 %, outputs
// 18 % of the workgroups' lifetime, the iteration loop a third).  Here ONE WAVE per replan does exactly that and nothing else, eight
// waves per SIMD deep (<= 64 registers, 6 KB of LDS): every replan of a launch is resident at once, the kernel lasts as long as one
// wave's chain of global round trips.  A replan whose certificate holds is finished here — trajectory and statistics
// written — and marked in ps.presolved; the slot's workgroup of the interior-point launch that follows only samples the states and writes
// the commit record from the returned coefficients (pure stores, overlapped with the iterating replans' arithmetic) and returns, so that
// launch's interior-point work is the replans that do iterate (one in eleven), all resident from the start.
//
// The kernel only ever ACCEPTS or ABSTAINS (qp_presolve.h).  Same formulas as qp_reg_kernel<true>'s own test (qp_reg_kernel.hip:
// "presolve: the minimiser without inequality rows"); the two may round differently in the last place, which decides nothing but
// who writes a result that both would accept.
#include <hip/hip_runtime.h>

#include "qp_presolve.h"

namespace nep {

namespace { __constant__ double cPreAPosInv[4][4] = NEP_APOS_INV_LITERALS; }      // (nep_tables.h)

#ifndef NEP_PRE_WAVES
#define NEP_PRE_WAVES 4      // (the small-launch form: up to 4 096 replans are resident at four waves per SIMD, and 128 registers hold the start point's loads without a spill; 6: 80 registers with 40 spilled.  Measured on the 64-slot single_scene leg, three pairs against the parent's kernel at six waves: inside the parent's range — profiles/presolve_fused_ab.txt section 5)
#endif
// The minimiser without inequality rows is linear in v = (b0, c0, d0, f) of an axis (nep_tables.h: RowMap, ThMap, ObjQ, built on the
// host from the same tables qp_reg_kernel uses: z* = -HaxInv (Gi init - 2 w ep f), row = U init + B z*, theta = ThU init + Th z*):
// a lane loads ONE 32-byte row of each map as soon as K is known — no chain g -> z* -> rows — and the guess's twelve numbers come
// through the scalar unit (wave-uniform addresses).
__global__ __launch_bounds__(64, NEP_PRE_WAVES) void qp_presolve_kernel(SceneParams sp, ProblemSet ps, const QpTable* __restrict__ tables, SampleSched sched, int* __restrict__ presolved) {
  __builtin_amdgcn_s_setprio(3);      // (latency-bound waves: when another scene group's hull / separator waves share the SIMD — bench.py's pipelined groups — these issue first)
  const int lane = threadIdx.x;
  if (ps.order_count && (int)blockIdx.x >= *ps.order_count) return;     // (an active set: the list of active slots, active_list_kernel)
  const int slot = ps.order_count ? ps.order[blockIdx.x] : (int)blockIdx.x;      // (without an active set: slot order, whatever the QP launch's order)
  const long long t0 = (long long)wall_clock64();
  __shared__ double sTheta[96], sA[2 * 32];
  __shared__ int sCnt[3 * NEP_MAX_POL + 4];
  const nep_guess* __restrict__ g = ps.guess + slot;
  const int K = g->K;
  // every exit before the certificate leaves the slot to the interior-point kernel
  if (lane == 0) presolved[slot] = 0;
  if (K < 3 || K > NEP_MAX_POL || K > sp.num_pol) return;
  const QpTable* __restrict__ tb = tables + K;      // mode 0: the first problem (terminal v = a = 0 eliminated)

  // ---- everything this wave reads that does not depend on anything but K and the slot, issued together ----
  int cn = 0, cf = 0, cs = 0; bool ovf = false;
  if (lane < NEP_MAX_POL && lane < K) {
    const int raw = ps.line_cnt[(long)slot * NEP_MAX_POL + lane];
    ovf = raw < 0; cn = line_count(raw);
    cf = ps.line_far[(long)slot * NEP_MAX_POL + lane];
    cs = ps.line_skip ? ps.line_skip[(long)slot * NEP_MAX_POL + lane] : 0;
  }
  int lpv = 0;
  if (ps.lp_stats && lane < 2 * NEP_MAX_POL) lpv = ps.lp_stats[(long)slot * NEP_MAX_POL * 2 + lane];
  // ---- (a) the start point: rows, coefficients, terminal ball, movement, cost (the table rows and the guess in one round trip) ----
  PreStart S = pre_start(sp, tb, g, K, lane, sA, sTheta, cPreAPosInv);
  if (__ballot(ovf) != 0ull) return;                    // a bucket overflowed: that replan fails (qp_reg_kernel: sI[27])
  if (lane < NEP_MAX_POL) { sCnt[lane] = cn; sCnt[NEP_MAX_POL + lane] = cf; sCnt[2 * NEP_MAX_POL + lane] = cs; }
  __syncthreads();
  int L_near = 0, n_far = 0, n_skip = 0;
#pragma unroll
  for (int i = 0; i < NEP_MAX_POL; i++) { L_near += sCnt[i]; n_far += sCnt[NEP_MAX_POL + i]; n_skip += sCnt[2 * NEP_MAX_POL + i]; }
  // ---- (b) the near separating lines, read where the separator left them ----
#pragma unroll 2
  for (int e = lane; e < L_near; e += 64) {
    int i = 0, off = 0, acc = 0;      // i = the segment whose bucket holds line e (the number of inclusive prefix sums <= e), off = lines before it
#pragma unroll
    for (int j = 0; j < NEP_MAX_POL - 1; j++) { acc += sCnt[j]; if (e >= acc) { i = j + 1; off = acc; } }
    const double* nd = ps.line_nd + (((long)slot * NEP_MAX_POL + i) * sp.lines_cap + (e - off)) * 3;
    S.viol = fmax(S.viol, pre_line_viol(nd[0], nd[1], nd[2], sA + 4 * i, sA + 32 + 4 * i));
  }
  // ---- (c) the verdict and what an accepted replan leaves behind ----
  pre_close(sp, ps, sched, slot, K, lane, S, L_near, n_far, n_skip, lpv, sTheta, g, t0, presolved);
}

void launch_qp_presolve(int n_slots, const SceneParams& sp, const ProblemSet& ps, const QpTable* tables, const SampleSched& sched, int* presolved, hipStream_t st) {
  if (n_slots <= 0 || !presolved) return;
  hipLaunchKernelGGL(qp_presolve_kernel, dim3(n_slots), dim3(64), 0, st, sp, ps, tables, sched, presolved);
}

}  // namespace nep
