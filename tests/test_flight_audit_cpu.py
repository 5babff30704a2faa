"""Flight audit, host form (include/neptune_frontend.h: nep_audit_records) against a numpy restatement that lives here, the
accumulation contract, and the ABI mirror.  No GPU."""
import numpy as np
import pytest

from neptune_amd import abi, audit, scene
from neptune_amd._lib import lib

from audit_util import HAND_T0, HAND_TICK, HAND_TICKS, hand_scene

DIST_TOL = 1e-12      # m, absolute: coordinates stay within ~20 m, one fp64 rounding there is ~4e-15 m


# ---- the restatement: its own cubic evaluation, its own signed distance, its own order of arithmetic -------------------------
def _present(r):
    return bool(r["valid"]) and bool(r["is_agent"]) and int(r["pwp"]["n_seg"]) >= 1


def _state(r, t):
    """x-y position and velocity of a record at t: clamped to the first knot before it, at rest on the end point after the last"""
    n = int(r["pwp"]["n_seg"])
    times = np.array(r["pwp"]["times"][: n + 1])
    if t >= times[n]:
        u = times[n] - times[n - 1]
        return np.array([np.polyval(r["pwp"]["coeff"][ax, n - 1], u) for ax in range(2)]), np.zeros(2)
    i = max(int(np.searchsorted(times[:n], t, side="right")) - 1, 0)
    u = max(t - times[i], 0.0)
    pos = np.array([np.polyval(r["pwp"]["coeff"][ax, i], u) for ax in range(2)])
    vel = np.array([np.polyval(np.polyder(np.array(r["pwp"]["coeff"][ax, i])), u) for ax in range(2)])
    return pos, vel


def _signed_dist(p, poly):
    """signed distance of point p to a convex polygon of either orientation: negative inside"""
    v = np.asarray(poly, dtype=np.float64)
    w = np.roll(v, -1, axis=0)
    e = w - v
    rel = p - v
    s = np.clip((rel * e).sum(1) / (e * e).sum(1), 0.0, 1.0)
    d = np.hypot(*(rel - s[:, None] * e).T).min()
    cr = e[:, 0] * rel[:, 1] - e[:, 1] * rel[:, 0]
    inside = len(v) >= 3 and (np.all(cr >= 0) or np.all(cr <= 0))
    return -d if inside else d


def restate(recs, statics, radius, t0, tick, n_ticks):
    n = len(recs)
    out = audit.new_audit(n)
    pres = [_present(recs[a]) for a in range(n)]
    last = [None] * n
    for k in range(n_ticks):
        t = t0 + k * tick
        st = [(_state(recs[a], t) if pres[a] else None) for a in range(n)]
        for a in range(n):
            if not pres[a]:
                continue
            A = out[a]
            p, v = st[a]
            tb, ts = np.inf, np.inf
            for j in range(n):
                if j == a or not pres[j]:
                    continue
                d = p - st[j][0]
                dist = float(np.hypot(d[0], d[1]))
                if dist < A["min_center_dist"]:
                    A["min_center_dist"] = dist; A["center_partner"] = j + 1; A["t_center"] = t
                half = np.array(recs[j]["bbox"][:2]) * 0.5 + radius
                bc = float((np.abs(d) - half).max())
                if bc < tb:
                    tb, tbp = bc, j + 1
            if tb < A["min_box_clear"]:
                A["min_box_clear"] = tb; A["box_partner"] = tbp; A["t_box"] = t
            A["n_pair_viol"] += tb < 0
            for j, poly in enumerate(statics):
                sd = float(_signed_dist(p, poly))
                if sd < ts:
                    ts, tsi = sd, j
            if ts < A["min_static_dist"]:
                A["min_static_dist"] = ts; A["static_index"] = tsi; A["t_static"] = t
            A["n_static_viol"] += ts < 0
            if last[a] is not None:
                A["path_len"] += float(np.hypot(*(p - last[a])))
            last[a] = p
            A["max_speed"] = max(A["max_speed"], float(np.hypot(v[0], v[1])))
            A["n_ticks"] += 1
    return out


EXACT = ("center_partner", "box_partner", "static_index", "n_ticks", "n_pair_viol", "n_static_viol", "t_center", "t_box", "t_static")
CLOSE = ("min_center_dist", "min_box_clear", "min_static_dist", "path_len", "max_speed")


def assert_matches(got, want):
    for f in EXACT:
        assert np.array_equal(got[f], want[f]), (f, got[f], want[f])
    for f in CLOSE:
        g, w = got[f], want[f]
        assert np.array_equal(np.isinf(g), np.isinf(w)), (f, g, w)
        fin = np.isfinite(w)
        err = np.abs(g[fin] - w[fin]).max() if fin.any() else 0.0
        print("%s: max |host - restatement| = %.3e m" % (f, err))
        assert err <= DIST_TOL, (f, err)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_host_form_matches_restatement_on_scenes(seed):
    sc = scene.make_scene(16, 8, seed)
    p = sc["par"]
    t0 = float(sc["committed"]["pwp"]["times"][0, 0])
    n_ticks = int(round(p.num_pol * p.T_span / p.dc)) + 12      # past the records' last knot: everybody comes to rest
    got = audit.audit_records(sc["committed"], sc["statics"], p.drone_radius, t0, p.dc, n_ticks)
    want = restate(sc["committed"], sc["statics"], p.drone_radius, t0, p.dc, n_ticks)
    assert (got["n_ticks"] == n_ticks).all()
    assert_matches(got, want)


def test_host_form_matches_restatement_on_hand_made_scene():
    recs, statics, radius = hand_scene()
    got = audit.audit_records(recs, statics, radius, HAND_T0, HAND_TICK, HAND_TICKS)
    want = restate(recs, statics, radius, HAND_T0, HAND_TICK, HAND_TICKS)
    assert_matches(got, want)
    a = {i + 1: got[i] for i in range(len(got))}
    fresh = audit.new_audit(1)[0]
    # the straight lines meet at t = 4: centres coincide, each 0.6 inside the other's inflated box
    assert a[1]["center_partner"] == 2 and a[2]["center_partner"] == 1 and a[1]["t_center"] == 4.0 and a[1]["min_center_dist"] == 0.0
    assert a[1]["box_partner"] == 2 and a[1]["t_box"] == 4.0 and a[1]["min_box_clear"] == -0.6 and a[1]["n_pair_viol"] >= 1
    # an invalid record and a non-agent are not audited and are nobody's partner
    for i in (3, 4):
        assert a[i].tobytes() == fresh.tobytes()
        assert not (got["center_partner"] == i).any() and not (got["box_partner"] == i).any()
    # a record that ends inside the window: at rest on its end point, and the path is the 2 m it flew
    assert a[5]["n_ticks"] == HAND_TICKS and abs(a[5]["path_len"] - 2.0) < 1e-9 and a[5]["max_speed"] == 1.5
    # through polygon 0: one metre inside at t = 3
    assert a[6]["static_index"] == 0 and a[6]["t_static"] == 3.0 and a[6]["min_static_dist"] == -1.0 and a[6]["n_static_viol"] == 15
    # two partners at exactly the same distance: the lower id, at the first tick
    assert a[7]["center_partner"] == 8 and a[7]["min_center_dist"] == 1.0 and a[7]["t_center"] == HAND_T0
    # unequal bboxes: the box clearance is asymmetric
    assert a[7]["box_partner"] == 9 and abs(a[7]["min_box_clear"] + 0.3) < 1e-15 and a[9]["box_partner"] == 7 and abs(a[9]["min_box_clear"] - 0.4) < 1e-15
    # the clockwise triangle is polygon 1, half a metre below agent 10
    assert a[10]["static_index"] == 1 and a[10]["min_static_dist"] == 0.5 and a[10]["path_len"] == 0.0


def test_calls_accumulate():
    recs, statics, radius = hand_scene()
    sc = scene.make_scene(16, 8, 0)
    for rr, ss, rad, t0, tick, n in ((recs, statics, radius, HAND_T0, HAND_TICK, 24), (sc["committed"], sc["statics"], 0.6, 0.0, 0.0625, 40)):
        one = audit.audit_records(rr, ss, rad, t0, tick, 2 * n)
        two = audit.audit_records(rr, ss, rad, t0, tick, n)
        before = two.copy()
        audit.audit_records(rr, ss, rad, t0 + 17 * tick, tick, 0, out=two)      # no ticks: nothing changes
        assert two.tobytes() == before.tobytes()
        audit.audit_records(rr, ss, rad, t0 + n * tick, tick, n, out=two)       # (dyadic ticks: the same tick times as doubles)
        assert one.tobytes() == two.tobytes()
        assert (one["n_ticks"][one["n_ticks"] > 0] == 2 * n).all()


def test_abi_size():
    assert lib().nep_abi_sizeof(17) == abi.AUDIT_DTYPE.itemsize == 112      # (index 16 is pinned to "unassigned" by an earlier test)
    fresh = audit.new_audit(3)
    for f in ("min_center_dist", "min_box_clear", "min_static_dist"):
        assert np.isposinf(fresh[f]).all()
    for f in ("center_partner", "box_partner", "static_index"):
        assert (fresh[f] == -1).all()
    for f in ("t_center", "t_box", "t_static", "path_len", "max_speed", "n_ticks", "n_pair_viol", "n_static_viol"):
        assert (fresh[f] == 0).all()
