"""Reference of the span-audit tests (tests/test_span_audit_cpu.py): dense sampling.  A numpy restatement with its own cubic
evaluation (Horner) and its own signed polygon distance samples a window at M points and takes the minima of the three audited
quantities per agent, together with a bound V on how fast any of them can change: the largest relative speed of two records (centre
distance and box clearance are 1-Lipschitz in the relative position) and the largest own speed (the static distance is 1-Lipschitz in
the position).  V is made an upper bound between the samples too: sampled speed + h * (sampled acceleration + h * largest jerk)."""
import numpy as np

M = 20001


def present(r):
    return bool(r["valid"]) and bool(r["is_agent"]) and int(r["pwp"]["n_seg"]) >= 1


def states(r, ts):
    """positions [M, 2], velocities [M, 2], accelerations [M, 2] and the largest jerk of a record at the times ts: clamped to the
    first knot before it, at rest on the end point beyond the last"""
    n = int(r["pwp"]["n_seg"])
    times = np.array(r["pwp"]["times"][: n + 1], dtype=np.float64)
    co = np.array(r["pwp"]["coeff"][:2, :n], dtype=np.float64)      # [2][n][4]
    past = ts >= times[n]
    i = np.clip(np.searchsorted(times[:n], ts, side="right") - 1, 0, n - 1)
    i = np.where(past, n - 1, i)
    before = (~past) & (ts < times[i])
    u = np.where(past, times[n] - times[n - 1], np.maximum(ts - times[i], 0.0))
    c = co[:, i, :]                                                 # [2][M][4]
    pos = ((c[..., 0] * u + c[..., 1]) * u + c[..., 2]) * u + c[..., 3]
    vel = (3.0 * c[..., 0] * u + 2.0 * c[..., 1]) * u + c[..., 2]
    acc = 6.0 * c[..., 0] * u + 2.0 * c[..., 1]
    still = past | before
    vel = np.where(still, 0.0, vel); acc = np.where(still, 0.0, acc)
    return pos.T, vel.T, acc.T, 6.0 * float(np.abs(co[..., 0]).max())


def signed_dist(p, poly):
    """signed distances of the points p [M, 2] to a convex polygon of either orientation: negative inside"""
    v = np.asarray(poly, dtype=np.float64)
    w = np.roll(v, -1, axis=0)
    e = w - v                                                       # [nv][2]
    rel = p[:, None, :] - v[None]                                   # [M][nv][2]
    ee = (e * e).sum(1)
    s = np.clip((rel * e[None]).sum(2) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
    d = np.hypot(*np.moveaxis(rel - s[..., None] * e[None], 2, 0)).min(1)
    cr = e[None, :, 0] * rel[..., 1] - e[None, :, 1] * rel[..., 0]
    inside = (len(v) >= 3) & (np.all(cr >= 0, axis=1) | np.all(cr <= 0, axis=1))
    return np.where(inside, -d, d)


def sample(recs, statics, radius, t0, t1, agents=None, m=M):
    """-> dict of [n] arrays: center, box, static (sampled minima, +inf where there is none), v_rel, v_own (speed bounds), and h,
    the sample step.  agents: the agents to take minima for (default: all); partners are always all."""
    n = len(recs)
    ts = np.linspace(t0, t1, m)
    h = (t1 - t0) / (m - 1)
    pres = [present(recs[a]) for a in range(n)]
    st = [states(recs[a], ts) if pres[a] else None for a in range(n)]
    out = dict(center=np.full(n, np.inf), box=np.full(n, np.inf), static=np.full(n, np.inf), v_rel=np.zeros(n), v_own=np.zeros(n), h=h)
    for a in (range(n) if agents is None else agents):
        if not pres[a]:
            continue
        pa, va, aa, ja = st[a]
        out["v_own"][a] = np.hypot(*va.T).max() + h * (np.hypot(*aa.T).max() + h * ja)
        for j in range(n):
            if j == a or not pres[j]:
                continue
            pj, vj, aj, jj = st[j]
            d = pa - pj
            out["center"][a] = min(out["center"][a], np.hypot(*d.T).min())
            half = np.array(recs[j]["bbox"][:2], dtype=np.float64) * 0.5 + radius
            out["box"][a] = min(out["box"][a], (np.abs(d) - half).max(1).min())
            out["v_rel"][a] = max(out["v_rel"][a], np.hypot(*(va - vj).T).max() + h * (np.hypot(*(aa - aj).T).max() + h * (ja + jj)))
        for poly in statics:
            out["static"][a] = min(out["static"][a], signed_dist(pa, poly).min())
    return out
