// tether_audit_common.h — the arithmetic of the tether audit (include/neptune_entangle.h: nep_tether_audit), shared by its host
// form (entangle_host.cpp: nep_ent_track_step_audit) and its device form (tether_kernels.hip: tether_step<LISTS, true>).  Both are
// built -ffp-contract=off.  One tracked move is one tick; the caller measures the tick (the taut length and the windings of the
// state the move left, its NEP_ENT_TRACK_* bits, the step list's length before the merge) and tether_audit_tick folds it into the
// slot's record.  A maximum is replaced only by a strictly larger value, so ties go to the earlier tick; within a tick the caller
// visits the agents by rising id (or keeps the lower id at a tie), so ties go to the lower agent.
#ifndef NEP_TETHER_AUDIT_COMMON_H_
#define NEP_TETHER_AUDIT_COMMON_H_

#include "../../include/neptune_entangle.h"

#ifndef NEP_TETHER_AUDIT_FN
#define NEP_TETHER_AUDIT_FN static inline
#endif

namespace nep_tether_audit_impl {

// What one tick hands to the record.  On a dropped move (flags == NEP_ENT_TRACK_CAP) everything but n_add describes the state
// that was kept.
struct TetherTick {
  double len;          // base -> bend anchors -> vehicle: the expression the move compares with the cable
  double t;            // t0 + (double)q * dt, q = 1.. the tick's number within the call
  int flags;           // the move's NEP_ENT_TRACK_* bits
  int n_add;           // new crossings the move produced (the step list before the merge)
  int n_alpha, n_bend;
  int wind, wind_partner;      // the largest active_cases[i] over the agents, and the lowest 1-based id that has it (0, 0: none)
  int ent_partner;             // the lowest 1-based id with active_cases[i] > 2 (0: none)
};

// The running (wind, partner, entangled partner) of a tick over (1-based id, entries of that id): any visiting order gives the
// lowest id among equals.
NEP_TETHER_AUDIT_FN void tether_wind(TetherTick& k, int id, int cases) {
  if (cases > k.wind || (cases == k.wind && cases > 0 && id < k.wind_partner)) { k.wind = cases; k.wind_partner = id; }
  if (cases > 2 && (k.ent_partner == 0 || id < k.ent_partner)) k.ent_partner = id;
}

NEP_TETHER_AUDIT_FN void tether_audit_tick(nep_tether_audit* a, const TetherTick& k) {
  a->n_ticks = a->n_ticks + 1;
  const int ord = a->n_ticks;
  a->sum_len = a->sum_len + k.len;
  a->last_len = k.len;
  if (k.len > a->max_len) { a->max_len = k.len; a->t_max_len = k.t; a->tick_max_len = ord; }
  a->crossings_added = a->crossings_added + k.n_add;
  if (k.n_alpha > a->max_alpha) a->max_alpha = k.n_alpha;
  if (k.n_bend > a->max_bend) a->max_bend = k.n_bend;
  if (k.wind > a->max_wind) { a->max_wind = k.wind; a->wind_partner = k.wind_partner; a->tick_max_wind = ord; a->t_max_wind = k.t; }
  if (k.flags & NEP_ENT_TRACK_CAP) { a->n_dropped = a->n_dropped + 1; return; }
  if (k.flags & NEP_ENT_TRACK_TOO_LONG) {
    a->n_too_long = a->n_too_long + 1;
    if (a->tick_first_too_long == 0) { a->tick_first_too_long = ord; a->t_first_too_long = k.t; }
  }
  if (k.flags & NEP_ENT_TRACK_ENTANGLED) {
    a->n_entangled = a->n_entangled + 1;
    if (a->tick_first_entangled == 0) { a->tick_first_entangled = ord; a->t_first_entangled = k.t; a->entangled_partner = k.ent_partner; }
  }
  if (k.flags & NEP_ENT_TRACK_TWO_CASES) a->n_two_cases = a->n_two_cases + 1;
  if (k.flags & NEP_ENT_TRACK_ABORT) a->n_abort = a->n_abort + 1;
}

}  // namespace nep_tether_audit_impl
#endif  // NEP_TETHER_AUDIT_COMMON_H_
