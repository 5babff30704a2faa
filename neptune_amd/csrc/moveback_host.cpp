// moveback_host.cpp — host form of the fleet loops' move-back rule (include/neptune_fleet.h: nep_moveback_step).  No HIP call; built
// like mission_host.cpp (-O2 -ffp-contract=off).  The arithmetic is moveback_common.h's, which the device form
// (fleet_moveback_kernels.hip) shares, and the device equals a chain of these calls byte for byte.
#include <string>

#include "moveback_common.h"

namespace nep { void set_last_error(const std::string& msg); }

using namespace nep_moveback_impl;

extern "C" int nep_moveback_step(const nep_moveback_cfg* cfg, int32_t n, const double* state, const double* pb, const double* t_issue,
                                 double t_first, double t_now, int32_t* flags, nep_fe_start* start) {
  if (!cfg || n < 0 || !state || !pb || !flags || !start) { nep::set_last_error("null argument"); return NEP_E_ARG; }
  if (!moveback_cfg_ok(*cfg)) { nep::set_last_error("bad move-back configuration (radius finite, timeout finite and >= 0)"); return NEP_E_ARG; }
  for (int a = 0; a < n; a++)
    flags[a] = moveback_slot(*cfg, state[12 * (size_t)a], state[12 * (size_t)a + 1], pb + 2 * (size_t)a, t_issue ? t_issue[a] : t_first, t_now,
                             flags[a], start[a].goal);
  return 0;
}
