"""Flight audit (include/neptune_frontend.h: nep_audit): per-agent clearances of what the fleets fly, at the control ticks.

`audit_records` is the host form through ctypes (nep_audit_records, no HIP call behind it); the device form is
BatchBackend.audit and equals it bit for bit.  `summarize` turns the per-agent records into one line of facts per scene."""
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
