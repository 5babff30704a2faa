// moveback_common.h — the move-back rule of the fleet loops (include/neptune_fleet.h: nep_batch_fleet_moveback), shared by its host
// form (moveback_host.cpp: nep_moveback_step) and its device form (fleet_moveback_kernels.hip).  Both are built -ffp-contract=off,
// sqrt is the only library call, and the rule below is written once.  A slot depends on nothing but its own inputs.
#ifndef NEP_MOVEBACK_COMMON_H_
#define NEP_MOVEBACK_COMMON_H_

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/neptune_fleet.h"

#ifndef NEP_MOVEBACK_FN
#define NEP_MOVEBACK_FN static inline
#endif

namespace nep_moveback_impl {

// finite radius (<= 0: only the timer releases), finite timeout >= 0 (a NaN fails both comparisons)
NEP_MOVEBACK_FN bool moveback_cfg_ok(const nep_moveback_cfg& c) {
  return fabs(c.radius) <= DBL_MAX && c.timeout >= 0.0 && c.timeout <= DBL_MAX;
}

// One slot of one round, at the select: (x, y) the tracked position, pb_a the slot's own base, t_iss the clock its goal was issued
// at, f its NEP_FLEET_FLAG_* word, goal the goal the search is given (nep_fe_start.goal).  Returns the new word.
//   set      a goal issued by the call that closed the last round — or the first goal — is as old as the clock, exactly
//   release  within the radius of the base, or older than the timeout: both strict, as neptune_ros.cpp:1291-1305
//   detour   while the bit stands the search heads for (pb.x, pb.y, the goal's z) (near_base.setPos, neptune_ros.cpp:1626-1636)
NEP_MOVEBACK_FN int moveback_slot(const nep_moveback_cfg& c, double x, double y, const double* pb_a, double t_iss, double t_now, int f, double* goal) {
  if (t_iss == t_now) f |= NEP_FLEET_FLAG_WAY_BACK;
  if (f & NEP_FLEET_FLAG_WAY_BACK) {
    const double dx = x - pb_a[0], dy = y - pb_a[1];
    const double d = sqrt(dx * dx + dy * dy);
    if (d < c.radius || t_now - t_iss > c.timeout) f &= ~NEP_FLEET_FLAG_WAY_BACK;
  }
  if (f & NEP_FLEET_FLAG_WAY_BACK) { goal[0] = pb_a[0]; goal[1] = pb_a[1]; }
  return f;
}

}  // namespace nep_moveback_impl

#endif  // NEP_MOVEBACK_COMMON_H_
