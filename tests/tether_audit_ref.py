"""A Python accumulator of the tether audit's rules (include/neptune_entangle.h: nep_tether_audit), independent of
tether_audit_common.h: it takes each tick's length, flags and counts as inputs and folds them into one TETHER_AUDIT_DTYPE record.

  ticks are numbered from 1 over the whole flight (n_ticks after counting the tick);
  a maximum is replaced only by a strictly larger value (ties: the earlier tick; within a tick the lower agent id);
  a dropped tick (NEP_ENT_TRACK_CAP) advances n_dropped and no other flag counter;
  the time of tick q = 1.. of a stretch is t0 + float(q) * dt."""
import numpy as np

from neptune_amd import abi


def fresh(n=1):
    a = np.zeros(n, dtype=abi.TETHER_AUDIT_DTYPE)
    a["max_len"] = -np.inf
    return a


def wind_of(active, N):
    """(largest active_cases[i] over the agents, the lowest 1-based id that has it, the lowest 1-based id with more than 2)"""
    wind, who, ent = 0, 0, 0
    for i in range(N):
        if active[i] > wind:
            wind, who = int(active[i]), i + 1
        if active[i] > 2 and ent == 0:
            ent = i + 1
    return wind, who, ent


def tick(rec, length, t, flags, n_add, n_alpha, n_bend, active, N):
    """one tick into rec (a 0-d or one-element TETHER_AUDIT_DTYPE view): length the taut length of the state the move left (the kept
    one when it was dropped), flags the move's NEP_ENT_TRACK_* bits, n_add the step list's length before the merge, n_alpha / n_bend /
    active the state after the move"""
    r = rec.reshape(-1)[0:1]
    g = lambda f: r[f][0]      # noqa: E731

    def put(f, v):
        r[f] = v
    put("n_ticks", g("n_ticks") + 1)
    o = int(g("n_ticks"))
    put("sum_len", np.float64(g("sum_len")) + np.float64(length))
    put("last_len", length)
    if length > g("max_len"):
        put("max_len", length); put("t_max_len", t); put("tick_max_len", o)
    put("crossings_added", g("crossings_added") + n_add)
    put("max_alpha", max(int(g("max_alpha")), n_alpha))
    put("max_bend", max(int(g("max_bend")), n_bend))
    wind, who, ent = wind_of(active, N)
    if wind > g("max_wind"):
        put("max_wind", wind); put("wind_partner", who); put("tick_max_wind", o); put("t_max_wind", t)
    if flags & abi.NEP_ENT_TRACK_CAP:
        put("n_dropped", g("n_dropped") + 1)
        return
    if flags & abi.NEP_ENT_TRACK_TOO_LONG:
        put("n_too_long", g("n_too_long") + 1)
        if g("tick_first_too_long") == 0:
            put("tick_first_too_long", o); put("t_first_too_long", t)
    if flags & abi.NEP_ENT_TRACK_ENTANGLED:
        put("n_entangled", g("n_entangled") + 1)
        if g("tick_first_entangled") == 0:
            put("tick_first_entangled", o); put("t_first_entangled", t); put("entangled_partner", ent)
    if flags & abi.NEP_ENT_TRACK_TWO_CASES:
        put("n_two_cases", g("n_two_cases") + 1)
    if flags & abi.NEP_ENT_TRACK_ABORT:
        put("n_abort", g("n_abort") + 1)
