// guess_fallback_kernels.hip — the reference's degrade-to-initial-guess rule for the batched path (nep_batch_guess_fallback and
// nep_batch_guess_fallback_tally, include/neptune_backend.h).  When both solves of PolySolverGurobi::optimize fail, pwp_out_ = pwp_init_
// (solver_gurobi_poly.cpp:856-859); Neptune::replanFull does not look at opt_success_ (the early return at neptune.cpp:1519-1527 is
// commented out), samples the guess (generatePwpOut), judges it (safetyCheckAfterReplan, :1644) and publishes it (:1661-1699).  The
// QP kernels leave everything that rule needs in a NEP_FAILED slot — nep_solution holds the guess (coefficients, knot times, K,
// n_states) and d_states its samples — and carry the PREVIOUS record into d_commit.  This kernel, behind the replan and optional,
// writes the record of the guess there instead and turns the status into NEP_GUESS, which the safety pass (records only),
// fleet_commit_kernel and fleet_count_kernel treat like a solved slot.  The QP kernels are not touched.
//
// Layout: one wave per slot.  Status and K are loaded from one address by every lane, so the exit — which in a flying fleet nearly
// every slot takes — is wave-uniform.  A published slot's record goes out in 16-byte units, one per lane: lanes 0-31 two units of
// coefficients, lanes 32-63 one, then lanes 32-47 the head of the record and the knot times.  put2 is two adjacent 8-byte stores in
// the source, which the compiler emits as one global_store_dwordx4 (7 of them in the kernel; global memory takes them at any 4-byte
// alignment, so a caller's 8-byte-aligned buffer is as good as an allocator's).  The bytes written are write_commit's
// (qp_outputs.h) and no others: bend[1..] and pwp._pad keep what the replan left.  The knot times are COPIED from the solution
// (write_trajectory's fused t_start + i T): this translation unit does no arithmetic, so its contraction setting cannot matter.
// No LDS, no barrier; the counters are integer atomics by lane 0.
#include <hip/hip_runtime.h>
#include <cstddef>

#include "nep_device.h"

namespace nep {

// the record's layout in 16-byte units (a field that moves breaks the build here, not a flight)
static_assert(sizeof(nep_traj_rec) % 16 == 0 && sizeof(nep_solution) % 16 == 0, "records are whole 16-byte units");
static_assert(offsetof(nep_traj_rec, bbox) == 16 && offsetof(nep_traj_rec, pos) == 40 && offsetof(nep_traj_rec, bend) == 64, "nep_traj_rec head");
static_assert(offsetof(nep_traj_rec, pwp) + offsetof(nep_pwp, times) == 200 && (offsetof(nep_traj_rec, pwp) + offsetof(nep_pwp, coeff)) % 16 == 0, "nep_pwp in nep_traj_rec");
static_assert(offsetof(nep_solution, coeff) % 16 == 0 && NEP_TRAJ_MAX_SEG % 2 == 0 && NEP_MAX_POL <= NEP_TRAJ_MAX_SEG, "nep_solution coefficients");

namespace {

constexpr int kCoefUnits = 3 * NEP_TRAJ_MAX_SEG * 4 / 2;      // 16-byte units of nep_pwp.coeff

__device__ __forceinline__ void put2(double* p, double a, double b) { p[0] = a; p[1] = b; }

__global__ __launch_bounds__(64) void guess_fallback_kernel(int n_local, int first_local, int num_pol, double bbox, const double* __restrict__ pb,
                                                            const nep_guess* __restrict__ guess, nep_solution* sols, nep_traj_rec* commit,
                                                            int* __restrict__ count) {
  const int lane = threadIdx.x, slot = blockIdx.x;
  nep_solution* const sol = sols + slot;
  if (sol->stats.status != NEP_FAILED) return;      // (solved, relaxed, skipped, already published: not this kernel's)
  const int K = sol->K, scene = slot / n_local;
  const bool publish = K >= 1 && K <= num_pol;      // (the replan set K = 0 for a front-end miss, a gated slot, K > num_pol)
  if (lane == 0 && count) { atomicAdd(count + 4 * scene, 1); if (publish) atomicAdd(count + 4 * scene + 1, 1); }
  if (!publish) return;
  nep_traj_rec* const cr = commit + slot;
  double* const cw = &cr->pwp.coeff[0][0][0];
  for (int u = lane; u < kCoefUnits; u += 64) {      // two coefficients of one (axis, segment) per unit; zero beyond K
    const int e = 2 * u, ax = e / (NEP_TRAJ_MAX_SEG * 4), r = e % (NEP_TRAJ_MAX_SEG * 4), seg = r >> 2, j = r & 3;
    double a = 0.0, b = 0.0;
    if (seg < K) { const double* s = &sol->coeff[ax][seg][j]; a = s[0]; b = s[1]; }
    put2(cw + e, a, b);
  }
  const int own = first_local + slot % n_local;
  const nep_guess* const g = guess + slot;
  switch (lane) {
    case 32:
      cr->id = own + 1; cr->is_agent = 1; cr->n_bend = 1; cr->valid = 1;
      break;
    case 33: put2(&cr->bbox[0], bbox, bbox); break;
    case 34: put2(&cr->bbox[2], bbox, g->coeff[0][0][3]); break;      // (bbox[2], pos[0]: the guess's start)
    case 35: put2(&cr->pos[1], g->coeff[1][0][3], g->coeff[2][0][3]); break;
    case 36: put2(&cr->bend[0][0], pb[2 * own], pb[2 * own + 1]); break;
    case 37: cr->pwp.n_seg = K; break;
    case 38: cr->pwp.times[0] = sol->times[0]; break;      // (times[0] sits 8 bytes past a 16-byte boundary)
    default:
      if (lane >= 40 && lane < 40 + NEP_TRAJ_MAX_SEG / 2) {      // times[1 + 2 q], times[2 + 2 q]
        const int i = 1 + 2 * (lane - 40);
        put2(&cr->pwp.times[i], i <= K ? sol->times[i] : 0.0, i + 1 <= K ? sol->times[i + 1] : 0.0);
      }
  }
  if (lane == 0) sol->stats.status = NEP_GUESS;
}

// one wave per scene: the published guesses of the round by what nep_batch_fleet_commit made of them
__global__ __launch_bounds__(64) void guess_fallback_tally_kernel(int n_local, const nep_solution* __restrict__ sols, const int* __restrict__ outcome,
                                                                  int* __restrict__ count) {
  const int lane = threadIdx.x, scene = blockIdx.x;
  int flown = 0, kept = 0;
  for (int a = lane; a < n_local; a += 64) {
    const long slot = (long)scene * n_local + a;
    if (sols[slot].stats.status != NEP_GUESS) continue;
    if (outcome[slot] == NEP_FLEET_ACCEPTED) flown++; else kept++;
  }
  for (int m = 32; m >= 1; m >>= 1) { flown += __shfl_xor(flown, m, 64); kept += __shfl_xor(kept, m, 64); }
  if (lane == 0) {
    if (flown) atomicAdd(count + 4 * scene + 2, flown);
    if (kept) atomicAdd(count + 4 * scene + 3, kept);
  }
}

}  // namespace

void launch_guess_fallback(int n_slots, const SceneParams& sp, const double* pb, const nep_guess* guess, nep_solution* sol, nep_traj_rec* commit,
                           int* count, hipStream_t st) {
  if (n_slots <= 0) return;
  hipLaunchKernelGGL(guess_fallback_kernel, dim3(n_slots), dim3(64), 0, st, sp.n_local, sp.first_local, sp.num_pol, 2 * sp.drone_radius, pb, guess, sol, commit, count);
}

void launch_guess_fallback_tally(int n_scenes, int n_local, const nep_solution* sol, const int* outcome, int* count, hipStream_t st) {
  if (n_scenes <= 0) return;
  hipLaunchKernelGGL(guess_fallback_tally_kernel, dim3(n_scenes), dim3(64), 0, st, n_local, sol, outcome, count);
}

}  // namespace nep
