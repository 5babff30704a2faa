// effort_common.h — the arithmetic of the fleet's effort record (include/neptune_fleet.h: nep_batch_fleet_effort), shared by its host
// form (effort_host.cpp) and its device form (fleet_effort_kernels.hip).  Both are built -ffp-contract=off, sqrt and fabs are the
// only library calls, and every expression below is written once.  A slot is walked by one thread in tick order: nothing here
// depends on scheduling.
#ifndef NEP_EFFORT_COMMON_H_
#define NEP_EFFORT_COMMON_H_

#include <math.h>
#include <stdint.h>

#include "../../include/neptune_fleet.h"

#ifndef NEP_EFFORT_FN
#define NEP_EFFORT_FN static inline
#endif

namespace nep_effort_impl {

struct EffortLimits { double v_max, a_max, j_max, slack; };

NEP_EFFORT_FN bool effort_args_ok(const EffortLimits& l, double dc, int round_ticks) {
  const double big = 1.0e300;
  return l.v_max > 0.0 && l.v_max < big && l.a_max > 0.0 && l.a_max < big && l.j_max > 0.0 && l.j_max < big && l.slack >= 0.0 && l.slack < big && dc > 0.0 &&
         dc < big && round_ticks >= 1;
}

// the largest |component| so far, and whether this tick's breaks the limit by more than the slack
NEP_EFFORT_FN bool effort_axis(const double* x, double limit, double slack, double* worst) {
  bool viol = false;
  for (int i = 0; i < 3; i++) {
    const double m = fabs(x[i]);
    if (m > worst[i]) worst[i] = m;
    if (m > limit + slack) viol = true;
  }
  return viol;
}

// one counted tick: s = the 12 doubles of the state the tick pops (position, velocity, acceleration, jerk)
NEP_EFFORT_FN void effort_tick(const EffortLimits& l, double dc, const double* s, nep_fleet_effort& e) {
  e.n_ticks = e.n_ticks + 1;
  e.jerk_sum = e.jerk_sum + sqrt((s[9] * s[9] + s[10] * s[10]) + s[11] * s[11]) * dc;
  if (effort_axis(s + 3, l.v_max, l.slack, e.max_v)) e.n_v_viol = e.n_v_viol + 1;
  if (effort_axis(s + 6, l.a_max, l.slack, e.max_a)) e.n_a_viol = e.n_a_viol + 1;
  if (effort_axis(s + 9, l.j_max, l.slack, e.max_j)) e.n_j_viol = e.n_j_viol + 1;
}

// the round_ticks ticks a slot is about to fly (nep_batch_fleet_tick's pop rule): tick q pops ring[(head + q - 1) mod cap] while
// q - 1 <= size - 1; after that the last state repeats and nothing is counted.  An arrived slot adds nothing.
NEP_EFFORT_FN void effort_slot(const EffortLimits& l, double dc, int round_ticks, const double* ring, int head, int size, int cap, int done, nep_fleet_effort& e) {
  if (done) return;
  for (int q = 1; q <= round_ticks && q - 1 <= size - 1; q++) effort_tick(l, dc, ring + (long)((head + (q - 1)) % cap) * 12, e);
}

}  // namespace nep_effort_impl
#endif  // NEP_EFFORT_COMMON_H_
