"""Span audit, host form (include/neptune_frontend.h: nep_span_audit_records): against dense sampling
(tests/span_audit_ref.py), against the closed-form answers of the directed cases (tests/span_audit_cases.py), against the tick audit
as bytes, the accumulation contract, the ABI mirror and the stand-alone sanitizer program.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from neptune_amd import abi, audit, scene
from neptune_amd._lib import lib

import span_audit_ref as ref
from span_audit_cases import FIELDS, big_scene, cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_TOL = 1e-12      # m: the tolerance tests/test_flight_audit_cpu.py uses for the same expressions
TIME_TOL = 1e-9       # s: at the slowest closing speed of a directed case (0.02 m/s near its stationary point) still far below DIST_TOL's reach;
                      # the candidate time itself is a root bisected to adjacent doubles of a polynomial re-based with a few roundings


def _scenes():
    out = []
    for seed, n_ticks in ((0, 5), (1, 37)):
        sc = scene.make_scene(16, 4, seed)
        out.append(("scene16_%d_ticks%d" % (seed, n_ticks), sc["committed"], sc["statics"], sc["par"].drone_radius, 0.0, sc["par"].dc, n_ticks, None))
    recs, statics, radius, dc = big_scene()
    out.append(("config5_size", recs, statics, radius, 0.0, dc, 10, list(range(0, len(recs), 16))))
    return out


SCENES = _scenes()
CASES = cases()


def _everything():
    for name, recs, statics, radius, t0, tick, n_ticks, _ in SCENES:
        yield name, recs, statics, radius, t0, tick, n_ticks
    for c in CASES:
        yield c["name"], c["recs"], c["statics"], c["radius"], c["t0"], c["tick"], c["n_ticks"]


@pytest.mark.parametrize("which", range(len(SCENES)), ids=[s[0] for s in SCENES])
def test_host_form_against_dense_sampling(which):
    """completeness: no sample lies below the span minimum (+ 1e-12 m); attainment: the span minimum is a value of the window, so it
    is not below the sampled minimum by more than V * h / 2 (nearest sample at most h / 2 away, V the speed bound of the reference).
    The config-5-size scene is audited whole and sampled for every 16th agent (against all 256 partners and all 100 polygons)."""
    name, recs, statics, radius, t0, tick, n_ticks, agents = SCENES[which]
    got = audit.span_audit_records(recs, statics, radius, t0, tick, n_ticks)
    want = ref.sample(recs, statics, radius, t0, t0 + n_ticks * tick, agents)
    for key, v in (("center", "v_rel"), ("box", "v_rel"), ("static", "v_own")):
        g, w = got[FIELDS[key][0]], want[key]
        sel = np.isfinite(w)
        assert sel.any() and np.isfinite(g[sel]).all()
        over = (g[sel] - w[sel]).max()
        under = (w[sel] - g[sel] - want[v][sel] * want["h"] / 2).max()
        print("%s %s: span - sampled <= %.3e m; sampled - span - V h / 2 <= %.3e m (V <= %.3f m/s, h = %.3e s)" % (name, key, over, under, want[v].max(), want["h"]))
        assert over <= DIST_TOL, (key, over)
        assert under <= 0.0, (key, under)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_directed_case(case):
    got = audit.span_audit_records(case["recs"], case["statics"], case["radius"], case["t0"], case["tick"], case["n_ticks"])
    for agent, key, value, t, who in case["expect"]:
        fv, ft, fw = FIELDS[key]
        r = got[agent - 1]
        print("%s agent %d %s: %.17g at %.17g (want %.17g at %.17g)" % (case["name"], agent, key, r[fv], r[ft], value, t))
        assert abs(r[fv] - value) <= DIST_TOL and abs(r[ft] - t) <= TIME_TOL and r[fw] == who, (case["doc"], agent, key, r[fv], r[ft], r[fw])


def test_directed_cases_records_and_gaps():
    by = {c["name"]: c for c in CASES}

    def both(name):
        c = by[name]
        args = (c["recs"], c["statics"], c["radius"], c["t0"], c["tick"], c["n_ticks"])
        return audit.span_audit_records(*args), audit.audit_records(*args)

    # an invalid record and a non-agent are not audited and are nobody's partner
    sp, tk = both("lines")
    fresh = audit.new_span_audit(1)[0]
    for i in (3, 4):
        assert sp[i - 1].tobytes() == fresh.tobytes()
        assert not (sp["center_partner"] == i).any() and not (sp["box_partner"] == i).any()
    assert sp["n_spans"][0] == 1 and sp["span"][0] == 2.0 and sp["n_pair_viol"][0] == 1
    # the closest approach lies between the ticks: the tick audit saw -0.425 at t = 1.125
    assert tk["t_box"][0] == 1.125 and abs(tk["min_box_clear"][0] + 0.425) <= DIST_TOL
    assert sp["gap_box"][0] == tk["min_box_clear"][0] - sp["min_box_clear"][0]
    # through the polygon between two ticks: the tick audit reports a positive distance, the span audit the depth at the ridge
    sp, tk = both("through_polygon")
    assert tk["min_static_dist"][0] > 0 and abs(tk["min_static_dist"][0] - 0.0125) <= DIST_TOL and tk["n_static_viol"][0] == 0
    assert sp["min_static_dist"][0] < 0 and sp["n_static_viol"][0] == 1
    assert sp["gap_static"][0] == tk["min_static_dist"][0] - sp["min_static_dist"][0] and abs(sp["gap_static"][0] - 0.0625) <= 2 * DIST_TOL
    # the same for a box breach
    sp, tk = both("box_breach")
    for a in (0, 1):
        assert tk["min_box_clear"][a] > 0 and abs(tk["min_box_clear"][a] - 0.025) <= DIST_TOL and tk["n_pair_viol"][a] == 0
        assert sp["min_box_clear"][a] < 0 and sp["n_pair_viol"][a] == 1
        assert sp["gap_box"][a] == tk["min_box_clear"][a] - sp["min_box_clear"][a] and abs(sp["gap_box"][a] - 0.04375) <= 2 * DIST_TOL


@pytest.mark.parametrize("which", [e[0] for e in _everything()])
def test_span_minimum_is_at_most_the_tick_minimum_as_bytes(which):
    """The ticks are candidates evaluated by the tick audit's own expressions: per agent the span minimum is <= the tick minimum as
    doubles.  Where the two are equal the span audit's time is never later, and where the time is the same so is the partner (a
    plateau that begins between two ticks is reported at its earliest time, before the tick that lies on it)."""
    name, recs, statics, radius, t0, tick, n_ticks = next(e for e in _everything() if e[0] == which)
    sp = audit.span_audit_records(recs, statics, radius, t0, tick, n_ticks)
    tk = audit.audit_records(recs, statics, radius, t0, tick, n_ticks)
    n_equal = n_same = 0
    for fv, ft, fw in FIELDS.values():
        s, t = sp[fv], tk[fv]
        assert np.array_equal(np.isinf(s), np.isinf(t))
        assert (s <= t).all(), (fv, s, t)
        eq = (s == t) & np.isfinite(s)
        assert (sp[ft][eq] <= tk[ft][eq]).all(), (fv, sp[ft][eq], tk[ft][eq])
        same = eq & (sp[ft] == tk[ft])
        assert (sp[fw][same] == tk[fw][same]).all(), (fv, sp[fw][same], tk[fw][same])
        n_equal += int(eq.sum()); n_same += int(same.sum())
    assert (sp["center_d2"] <= tk["center_d2"]).all()
    for fg, fv in (("gap_box", "min_box_clear"), ("gap_static", "min_static_dist")):      # one call: the gap is the difference
        fin = np.isfinite(tk[fv])
        assert np.array_equal(sp[fg][fin], tk[fv][fin] - sp[fv][fin]) and (sp[fg][~fin] == 0).all()
    print("%s: %d minima equal to the tick audit's, %d of them at the same time" % (name, n_equal, n_same))


def _merge_by_hand(one, two):
    out = one.copy()
    for fv, ft, fw in FIELDS.values():
        better = two[fv] < one[fv]      # strictly smaller wins: the earlier call keeps a tie
        for f in (fv, ft, fw):
            out[f][better] = two[f][better]
    better = two["center_d2"] < one["center_d2"]
    out["center_d2"][better] = two["center_d2"][better]
    for f in ("n_spans", "n_pair_viol", "n_static_viol"):
        out[f] = one[f] + two[f]
    out["span"] = one["span"] + two["span"]
    for f in ("gap_box", "gap_static"):
        out[f] = np.maximum(one[f], two[f])
    return out


def test_calls_accumulate():
    sc = scene.make_scene(16, 4, 0)
    c = next(c for c in CASES if c["name"] == "lines")
    for recs, statics, radius, t0, tick, n in ((c["recs"], c["statics"], c["radius"], 0.0, 0.125, 8), (sc["committed"], sc["statics"], 0.6, 0.0, 0.0625, 20)):
        one = audit.span_audit_records(recs, statics, radius, t0, tick, n)
        two = audit.span_audit_records(recs, statics, radius, t0 + n * tick, tick, n)
        acc = one.copy()
        before = acc.copy()
        audit.span_audit_records(recs, statics, radius, t0 + 17 * tick, tick, 0, out=acc)      # no ticks: nothing changes
        assert acc.tobytes() == before.tobytes()
        audit.span_audit_records(recs, statics, radius, t0 + n * tick, tick, n, out=acc)
        assert acc.tobytes() == _merge_by_hand(one, two).tobytes()
        seen = acc["n_spans"] > 0
        assert (acc["n_spans"][seen] == 2).all() and (acc["span"][seen] == 2 * n * tick).all()
        # the two windows share the instant between them, and together they cover the long window: the same minima (dyadic ticks)
        long = audit.span_audit_records(recs, statics, radius, t0, tick, 2 * n)
        for fv, ft, fw in FIELDS.values():
            for f in (fv, ft, fw):
                assert np.array_equal(acc[f], long[f]), f


def test_abi_size():
    assert lib().nep_abi_sizeof(39) == abi.SPAN_AUDIT_DTYPE.itemsize == 104
    assert lib().nep_abi_sizeof(38) == -1
    fresh = audit.new_span_audit(3)
    for f in ("min_center_dist", "min_box_clear", "min_static_dist", "center_d2"):
        assert np.isposinf(fresh[f]).all()
    for f in ("center_partner", "box_partner", "static_index"):
        assert (fresh[f] == -1).all()
    for f in ("t_center", "t_box", "t_static", "span", "gap_box", "gap_static", "n_spans", "n_pair_viol", "n_static_viol"):
        assert (fresh[f] == 0).all()


def test_summary_and_lines():
    c = next(c for c in CASES if c["name"] == "box_breach")
    sp = audit.span_audit_records(c["recs"], c["statics"], c["radius"], c["t0"], c["tick"], c["n_ticks"])
    summ = audit.summarize_span(sp)
    assert len(summ) == 1 and summ[0]["n_pair_viol"] == 2 and summ[0]["n_spans"] == 1 and summ[0]["span"] == 2.0
    assert summ[0]["min_box_clear"]["agent"] == 1 and summ[0]["min_box_clear"]["partner"] == 2 and abs(summ[0]["gap_box"] - 0.04375) <= 2 * DIST_TOL
    lines = audit.format_span_summary(summ)
    assert len(lines) == 4 and lines[3].startswith("span  gaps to the ticks: box 0.04375")


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/span_audit_check.cpp: malformed records, zero-length windows, degenerate polygons and the capacities, with the host
    form compiled into the program under -fsanitize=address,undefined (built as tests/cpp/hastar_host_check.cpp is)"""
    exe = str(tmp_path / "span_audit_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "span_audit_check.cpp"),
           os.path.join(ROOT, "neptune_amd", "csrc", "audit_span_host.cpp"), os.path.join(ROOT, "neptune_amd", "csrc", "audit_host.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout + out.stderr)
    assert out.returncode == 0 and "span_audit_check ok" in out.stdout
