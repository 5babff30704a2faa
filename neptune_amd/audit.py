"""Flight audit (include/neptune_frontend.h: nep_audit): per-agent clearances of what the fleets fly, at the control ticks.

`audit_records` is the host form through ctypes (nep_audit_records, no HIP call behind it); the device form is
BatchBackend.audit and equals it bit for bit.  `summarize` turns the per-agent records into one line of facts per scene.

Span audit (include/neptune_frontend.h: nep_span_audit): the same three minima over the whole flown window, not
only at its ticks.  `span_audit_records` is the host form, BatchBackend.audit_span the device form, byte for byte the same;
`summarize_span` and `format_span_summary` give the facts and the lines, among them how much the ticks missed.

Tether audit (include/neptune_entangle.h: nep_tether_audit): taut length, slack and winding of every tracked move.
`tether_audit_records` is the host form (a chain of nep_ent_track_step_audit); the device form is BatchBackend.set_tether_audit and
equals it byte for byte.  `summarize_tethers` gives the facts per scene, `format_tether_summary` the lines the scripts print."""
import ctypes as C

import numpy as np

from . import abi, scene
from ._lib import check, lib


def new_audit(n):
    """n records with the initial values: minima +inf, partners and index -1, the rest 0 (nep_audit_init)"""
    out = np.zeros(n, dtype=abi.AUDIT_DTYPE)
    check(lib().nep_audit_init(out.ctypes.data_as(C.c_void_p), n))
    return out


def audit_records(recs, statics, drone_radius, t0, tick, n_ticks, out=None):
    """One scene: recs [n] TRAJ_REC_DTYPE, statics a list of (inflated) polygons, the ticks t0 + k*tick, k < n_ticks.
    Accumulates into `out` ([n] AUDIT_DTYPE, made fresh when None) and returns it."""
    recs = np.ascontiguousarray(recs, dtype=abi.TRAJ_REC_DTYPE).reshape(-1)
    n = len(recs)
    if out is None:
        out = new_audit(n)
    assert out.dtype == abi.AUDIT_DTYPE and out.shape == (n,) and out.flags["C_CONTIGUOUS"]
    off, xy = scene.statics_csr(statics)
    check(lib().nep_audit_records(recs.ctypes.data_as(C.c_void_p), n, abi.iptr(off), abi.dptr(xy), len(statics), float(drone_radius),
                                  float(t0), float(tick), int(n_ticks), out.ctypes.data_as(C.c_void_p)))
    return out


def _worst(a, field, partner, time):
    """the scene's smallest `field` with who, whom and when; None when nobody has one"""
    v = a[field]
    if not len(v) or not np.isfinite(v).any():
        return None
    i = int(np.argmin(v))
    return dict(value=float(v[i]), agent=i + 1, partner=int(a[partner][i]), t=float(a[time][i]))


def summarize(audit, n_scenes=1):
    """audit: [n_scenes*N] AUDIT_DTYPE (or the bytes of it) -> one dict per scene: the three minima with agent (1-based id),
    partner (1-based id; for the statics the 0-based polygon index) and time, and the violation counts"""
    a = np.asarray(audit)
    if a.dtype != abi.AUDIT_DTYPE:
        a = a.view(abi.AUDIT_DTYPE)
    a = a.reshape(n_scenes, -1)
    out = []
    for s in range(n_scenes):
        r = a[s]
        out.append(dict(min_center_dist=_worst(r, "min_center_dist", "center_partner", "t_center"),
                        min_box_clear=_worst(r, "min_box_clear", "box_partner", "t_box"),
                        min_static_dist=_worst(r, "min_static_dist", "static_index", "t_static"),
                        n_pair_viol=int(r["n_pair_viol"].sum()), n_static_viol=int(r["n_static_viol"].sum()),
                        n_ticks=int(r["n_ticks"].max()) if len(r) else 0,
                        path_len_mean=float(r["path_len"].mean()) if len(r) else 0.0,
                        max_speed=float(r["max_speed"].max()) if len(r) else 0.0))
    return out


def format_summary(summary):
    """the lines scripts/closed_loop.py and scripts/tether_loop.py print: the worst scene of each minimum, and the counts"""
    lines = []
    for key, whom in (("min_center_dist", "agent"), ("min_box_clear", "agent"), ("min_static_dist", "polygon")):
        best = None
        for s, sc in enumerate(summary):
            m = sc[key]
            if m is not None and (best is None or m["value"] < best[1]["value"]):
                best = (s, m)
        if best is None:
            lines.append("audit %-16s none" % key)
        else:
            s, m = best
            lines.append("audit %-16s %+.9f m  scene %d  agent %d  %s %d  t %.3f s" % (key, m["value"], s, m["agent"], whom, m["partner"], m["t"]))
    lines.append("audit ticks %d  pair violations %d (agent-ticks, in %d scenes)  static violations %d (in %d scenes)  of %d scenes"
                 % (max(sc["n_ticks"] for sc in summary), sum(sc["n_pair_viol"] for sc in summary), sum(sc["n_pair_viol"] > 0 for sc in summary),
                    sum(sc["n_static_viol"] for sc in summary), sum(sc["n_static_viol"] > 0 for sc in summary), len(summary)))
    return lines


# ---- the span audit ---------------------------------------------------------------------------------------------------------------
def new_span_audit(n):
    """n records with the initial values: minima +inf, partners and index -1, the rest 0 (nep_span_audit_init)"""
    out = np.zeros(n, dtype=abi.SPAN_AUDIT_DTYPE)
    check(lib().nep_span_audit_init(out.ctypes.data_as(C.c_void_p), n))
    return out


def span_audit_records(recs, statics, drone_radius, t0, tick, n_ticks, out=None):
    """One scene over the whole window [t0, t0 + n_ticks*tick], not only at its ticks (nep_span_audit_records):
    the arguments of audit_records.  Accumulates into `out` ([n] SPAN_AUDIT_DTYPE, made fresh when None) and returns it."""
    recs = np.ascontiguousarray(recs, dtype=abi.TRAJ_REC_DTYPE).reshape(-1)
    n = len(recs)
    if out is None:
        out = new_span_audit(n)
    assert out.dtype == abi.SPAN_AUDIT_DTYPE and out.shape == (n,) and out.flags["C_CONTIGUOUS"]
    off, xy = scene.statics_csr(statics)
    check(lib().nep_span_audit_records(recs.ctypes.data_as(C.c_void_p), n, abi.iptr(off), abi.dptr(xy), len(statics), float(drone_radius),
                                       float(t0), float(tick), int(n_ticks), out.ctypes.data_as(C.c_void_p)))
    return out


def summarize_span(span, n_scenes=1):
    """span: [n_scenes*N] SPAN_AUDIT_DTYPE (or the bytes of it) -> one dict per scene: the three minima as summarize gives them, the
    violation counts (agent-calls), the seconds audited and the largest gaps to the tick audit (what the sampler missed)"""
    a = np.asarray(span)
    if a.dtype != abi.SPAN_AUDIT_DTYPE:
        a = a.view(abi.SPAN_AUDIT_DTYPE)
    a = a.reshape(n_scenes, -1)
    out = []
    for s in range(n_scenes):
        r = a[s]
        out.append(dict(min_center_dist=_worst(r, "min_center_dist", "center_partner", "t_center"),
                        min_box_clear=_worst(r, "min_box_clear", "box_partner", "t_box"),
                        min_static_dist=_worst(r, "min_static_dist", "static_index", "t_static"),
                        n_pair_viol=int(r["n_pair_viol"].sum()), n_static_viol=int(r["n_static_viol"].sum()),
                        n_spans=int(r["n_spans"].max()) if len(r) else 0, span=float(r["span"].max()) if len(r) else 0.0,
                        gap_box=float(r["gap_box"].max()) if len(r) else 0.0, gap_static=float(r["gap_static"].max()) if len(r) else 0.0))
    return out


def format_span_summary(summary):
    """the lines the scripts print next to the tick audit's: the worst scene of each minimum over the whole flight, then the gaps"""
    lines = []
    for key, whom in (("min_center_dist", "agent"), ("min_box_clear", "agent"), ("min_static_dist", "polygon")):
        best = None
        for s, sc in enumerate(summary):
            m = sc[key]
            if m is not None and (best is None or m["value"] < best[1]["value"]):
                best = (s, m)
        if best is None:
            lines.append("span  %-16s none" % key)
        else:
            s, m = best
            lines.append("span  %-16s %+.9f m  scene %d  agent %d  %s %d  t %.6f s" % (key, m["value"], s, m["agent"], whom, m["partner"], m["t"]))
    lines.append("span  gaps to the ticks: box %.9f m  static %.9f m  over %.3f s in %d calls  pair violations %d (agent-calls, in %d scenes)  "
                 "static violations %d (in %d scenes)  of %d scenes"
                 % (max(sc["gap_box"] for sc in summary), max(sc["gap_static"] for sc in summary), max(sc["span"] for sc in summary),
                    max(sc["n_spans"] for sc in summary), sum(sc["n_pair_viol"] for sc in summary), sum(sc["n_pair_viol"] > 0 for sc in summary),
                    sum(sc["n_static_viol"] for sc in summary), sum(sc["n_static_viol"] > 0 for sc in summary), len(summary)))
    return lines


# ---- the tether audit ---------------------------------------------------------------------------------------------------------
def new_tether_audit(n):
    """n records with the initial values: max_len -inf, every partner, tick and time 0, the rest 0 (nep_tether_audit_init)"""
    out = np.zeros(n, dtype=abi.TETHER_AUDIT_DTYPE)
    check(lib().nep_tether_audit_init(out.ctypes.data_as(C.c_void_p), n))
    return out


def tether_audit_records(chk, state, moves, t0, dt, out=None):
    """One agent's tether over a stretch of tracked moves, on the host: chk its entangle.EntangleCheck, state its entangle.State
    (updated in place), moves a sequence of track_step's arguments (pk, pk1, pik, pik1, present, bendpts, bendpts_prev); move
    q = 1.. is the tick at t0 + q * dt.  Accumulates into `out` ([1] TETHER_AUDIT_DTYPE, made fresh when None);
    -> (out, the moves' NEP_ENT_TRACK_* bits)."""
    if out is None:
        out = new_tether_audit(1)
    flags = []
    for q, m in enumerate(moves, 1):
        flags.append(chk.track_step(state, *m, audit=out, t=t0 + float(q) * dt))
    return out, flags


def summarize_tethers(records, cable_length, n_scenes=1):
    """records: [n_scenes*N] TETHER_AUDIT_DTYPE (or the bytes of it) -> one dict per scene: the smallest slack cable_length - max_len
    with agent (1-based id) and time, the mean length, the largest list and bend counts, the largest wind with the pair
    (agent, partner; 1-based) and time, and the ticks too long / entangled / dropped (agent-ticks)"""
    a = np.asarray(records)
    if a.dtype != abi.TETHER_AUDIT_DTYPE:
        a = a.view(abi.TETHER_AUDIT_DTYPE)
    a = a.reshape(n_scenes, -1)
    out = []
    for s in range(n_scenes):
        r = a[s]
        seen = r["n_ticks"] > 0
        d = dict(min_slack=None, mean_len=None, max_alpha=int(r["max_alpha"].max()) if len(r) else 0, max_bend=int(r["max_bend"].max()) if len(r) else 0,
                 max_wind=None, n_ticks=int(r["n_ticks"].max()) if len(r) else 0, n_too_long=int(r["n_too_long"].sum()),
                 n_entangled=int(r["n_entangled"].sum()), n_two_cases=int(r["n_two_cases"].sum()), n_abort=int(r["n_abort"].sum()),
                 n_dropped=int(r["n_dropped"].sum()), crossings_added=int(r["crossings_added"].sum()))
        if seen.any():
            i = int(np.argmax(np.where(seen, r["max_len"], -np.inf)))
            d["min_slack"] = dict(value=float(cable_length - r["max_len"][i]), agent=i + 1, t=float(r["t_max_len"][i]), tick=int(r["tick_max_len"][i]))
            d["mean_len"] = float(r["sum_len"][seen].sum() / r["n_ticks"][seen].sum())
            w = int(np.argmax(r["max_wind"]))
            if r["max_wind"][w] > 0:
                d["max_wind"] = dict(value=int(r["max_wind"][w]), agent=w + 1, partner=int(r["wind_partner"][w]), t=float(r["t_max_wind"][w]),
                                     tick=int(r["tick_max_wind"][w]))
        out.append(d)
    return out


def format_tether_summary(summary, cap=None):
    """the lines scripts/fleet_loop.py, scripts/tether_loop.py and scripts/closed_loop.py print: the scene with the least slack, the
    scene with the largest wind, the largest counts (next to `cap`, the list capacity in force, when given) and the tick counts"""
    lines = []
    best = None
    for s, sc in enumerate(summary):
        m = sc["min_slack"]
        if m is not None and (best is None or m["value"] < best[1]["value"]):
            best = (s, m)
    if best is None:
        lines.append("tether min_slack        none")
    else:
        s, m = best
        lines.append("tether min_slack        %+.9f m  scene %d  agent %d  t %.3f s (tick %d)" % (m["value"], s, m["agent"], m["t"], m["tick"]))
    means = [sc["mean_len"] for sc in summary if sc["mean_len"] is not None]
    if means:
        lines.append("tether mean_len         %.6f m (mean over %d scenes)" % (float(np.mean(means)), len(means)))
    wind = None
    for s, sc in enumerate(summary):
        m = sc["max_wind"]
        if m is not None and (wind is None or m["value"] > wind[1]["value"]):
            wind = (s, m)
    if wind is None:
        lines.append("tether max_wind         0")
    else:
        s, m = wind
        lines.append("tether max_wind         %d  scene %d  agent %d round agent %d  t %.3f s (tick %d)" % (m["value"], s, m["agent"], m["partner"], m["t"], m["tick"]))
    lines.append("tether max_alpha %d%s  max_bend %d (of %d)" % (max(sc["max_alpha"] for sc in summary), " (cap %d)" % cap if cap is not None else "",
                                                                 max(sc["max_bend"] for sc in summary), abi.NEP_MAX_BEND - 1))
    lines.append("tether ticks %d  too long %d  entangled %d  dropped %d (agent-ticks)  crossings added %d  of %d scenes"
                 % (max(sc["n_ticks"] for sc in summary), sum(sc["n_too_long"] for sc in summary), sum(sc["n_entangled"] for sc in summary),
                    sum(sc["n_dropped"] for sc in summary), sum(sc["crossings_added"] for sc in summary), len(summary)))
    return lines
