// fleet_moveback_kernels.hip — the move-back rule of the device fleet loop (nep_batch_fleet_moveback, include/neptune_fleet.h): a
// slot with a new goal is sent to its own base first.  The arithmetic is moveback_common.h's, which the host form (moveback_host.cpp:
// nep_moveback_step) shares; the device equals the host chain byte for byte — built -ffp-contract=off like fleet_mission_kernels.hip.
//
// Layout: one thread per slot, like fleet_select_kernel, which it follows in the round.  A slot reads 16 B of its tracked state, its
// base, its scene's clock, its issue clock and its flag word, and writes the word and — on its way back — 16 B of its start record.
// Nothing is shared between slots: no LDS, no barrier, no atomic.
#include <hip/hip_runtime.h>

#define NEP_MOVEBACK_FN __device__ inline
#include "nep_device.h"
#include "moveback_common.h"

namespace nep {

using namespace nep_moveback_impl;

static_assert(sizeof(nep_moveback_cfg) == 16, "nep_moveback_cfg is mirrored by hand in neptune_amd/abi.py");

namespace {

__global__ __launch_bounds__(64) void fleet_moveback_kernel(nep_moveback_cfg c, FleetArgs fa, const double* __restrict__ t_issue) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (long)fa.n_scenes * fa.N) return;
  const long scene = slot / fa.N; const int a = (int)(slot - scene * fa.N);
  const double t_iss = t_issue ? t_issue[slot] : fa.cfg.t0;
  fa.sflags[slot] = moveback_slot(c, fa.state[slot * 12], fa.state[slot * 12 + 1], fa.pb + 2 * a, t_iss, fa.t_now[scene], fa.sflags[slot],
                                  fa.start[slot].goal);
}

}  // namespace

void launch_fleet_moveback(const nep_moveback_cfg& c, const FleetArgs& fa, const double* t_issue, hipStream_t st) {
  const long slots = (long)fa.n_scenes * fa.N;
  hipLaunchKernelGGL(fleet_moveback_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, st, c, fa, t_issue);
}

}  // namespace nep
