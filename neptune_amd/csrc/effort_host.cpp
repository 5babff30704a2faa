// effort_host.cpp — host form of the fleet's effort record (include/neptune_fleet.h: nep_effort_step).  No HIP call; built like
// mission_host.cpp (-O2 -ffp-contract=off).  The arithmetic is effort_common.h's, which the device form (fleet_effort_kernels.hip)
// shares, and the device equals a chain of these calls byte for byte.
#include <string>

#include "effort_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_effort_impl;

extern "C" int nep_effort_step(double v_max, double a_max, double j_max, double dc, int32_t round_ticks, const double* ring, int32_t head,
                               int32_t size, int32_t cap, int32_t done, double slack, nep_fleet_effort* out) {
  if (!ring || !out) { nep::set_last_error("null argument"); return NEP_E_ARG; }
  const EffortLimits l{v_max, a_max, j_max, slack};
  if (!effort_args_ok(l, dc, round_ticks)) { nep::set_last_error("bad effort arguments (limits and dc finite and > 0, slack finite and >= 0, round_ticks >= 1)"); return NEP_E_ARG; }
  if (cap < 1 || head < 0 || head >= cap || size < 0 || size > cap) { nep::set_last_error("bad ring (cap >= 1, 0 <= head < cap, 0 <= size <= cap)"); return NEP_E_ARG; }
  effort_slot(l, dc, round_ticks, ring, head, size, cap, done, *out);
  return 0;
}
