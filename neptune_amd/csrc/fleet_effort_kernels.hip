// fleet_effort_kernels.hip — the effort record of the device fleet loop (nep_batch_fleet_effort, include/neptune_fleet.h): per slot
// the jerk integral, the largest velocity, acceleration and jerk components and the limit violations of the ticks about to be flown.
// The arithmetic is effort_common.h's, which the host form (effort_host.cpp: nep_effort_step) shares; the device equals the host
// chain byte for byte — built -ffp-contract=off like fleet_kernels.hip.
//
// Layout: one thread per slot, like fleet_moveback_kernel.  A slot reads its head, size and done flag, up to round_ticks states of
// 96 B from its ring, and its 96-byte record, which it keeps in registers over the ticks and writes back once.  Nothing is shared
// between slots: no LDS, no barrier, no atomic; the sums are made in tick order.
#include <hip/hip_runtime.h>

#define NEP_EFFORT_FN __device__ inline
#include "nep_device.h"
#include "effort_common.h"

namespace nep {

using namespace nep_effort_impl;

static_assert(sizeof(nep_fleet_effort) == 96, "nep_fleet_effort is mirrored by hand in neptune_amd/abi.py");

namespace {

__global__ __launch_bounds__(64) void fleet_effort_kernel(EffortLimits l, FleetArgs fa, nep_fleet_effort* __restrict__ out) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (long)fa.n_scenes * fa.N) return;
  if (fa.done[slot]) return;
  nep_fleet_effort e = out[slot];
  effort_slot(l, fa.cfg.dc, fa.cfg.round_ticks, fa.ring + slot * fa.cap * 12, fa.head[slot], fa.size[slot], fa.cap, 0, e);
  out[slot] = e;
}

}  // namespace

void launch_fleet_effort(const FleetArgs& fa, double v_max, double a_max, double j_max, double slack, nep_fleet_effort* out, hipStream_t st) {
  const long slots = (long)fa.n_scenes * fa.N;
  hipLaunchKernelGGL(fleet_effort_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, st, EffortLimits{v_max, a_max, j_max, slack}, fa, out);
}

}  // namespace nep
