"""CPU: the oracle away from the one parameter point every other test uses (tests/param_sets.py) — against the golden QPs of
tests/golden/qp_cases_params.npz (make_golden_params.py: independent SciPy optima with z motion at every set of the table), against
exact rational MINVO control points and a plain Horner sampling at other T_span / dc, and its hulls against scene.interval_hull
with non-square boxes.  The GPU twin is test_gpu_param_sweep.py."""
from fractions import Fraction as F

import numpy as np
import pytest

import helpers
import param_sets as PS
import param_util as PU
from neptune_amd import abi, scene

FIXTURE = "qp_cases_params.npz"


def test_oracle_against_golden_params(oracle):
    """Bars as for the earlier fixtures: certified cases 1e-8 in coefficients and 1e-8 relative in cost (test_qp_against_golden_r2),
    agreement-only cases helpers.theta_tol (the file as committed has none: every terminal-ball case it keeps has the ball inactive and
    carries the certificate).  Measured, worst coefficient error per set: default 2.1e-11, exp 3.5e-13, single 2.8e-13, fast_long 1.3e-11,
    heavy 2.1e-9, pol5 6.0e-12, pol6 7.8e-10."""
    worst = {}
    for c in helpers.load_qp_cases(FIXTURE):
        p = helpers.params_of_case(c)
        r = oracle.optimize(p, 1, c["coeff_init"], [], [], lines=(c["line_seg"], c["line_nd"]))
        assert r["status"] == c["status"], c["tag"]
        th = helpers.golden_theta_out(c)
        err = np.abs(r["coeff"] - th).max()
        key = (c["set"], c["certified"]); worst[key] = max(worst.get(key, 0.0), err)
        print("%-34s status %d certified %d  |oracle - golden| = %.2e" % (c["tag"], c["status"], c["certified"], err))
        assert err <= (1e-8 if c["certified"] else helpers.theta_tol(c)), (c["tag"], err)
        if c["status"] != 2:
            assert abs(r["objective"] - c["cost"]) <= (1e-8 if c["certified"] else 5e-6) * (1 + abs(c["cost"])), c["tag"]
    for (name, cert), e in sorted(worst.items()):
        print("set %-10s %s: worst oracle error %.2e" % (name, "certified" if cert else "agreement-only", e))


def test_golden_params_fixture_composition():
    cases = helpers.load_qp_cases(FIXTURE)
    sets = [c["set"] for c in cases]
    for name in PS.SWEPT:
        assert sets.count(name) >= 3, name
    assert {c["status"] for c in cases} == {0, 1, 2}
    assert {c["num_pol"] for c in cases} >= {5, 6, 8}
    assert {(c["num_pol"], c["K"]) for c in cases} >= {(5, 5), (6, 4), (6, 6)}
    for name in ("exp", "fast_long"):
        assert {c["status"] for c in cases if c["set"] == name} == {0, 1, 2}, name
    assert sum(c["n_active_z"] > 0 for c in cases) >= 4
    # the reference's z override (solver_gurobi_poly.cpp:879-880) on a z guess that is not flat
    n_override = 0
    for c in cases:
        ci = c["coeff_init"]
        moved = not np.array_equal(helpers.golden_theta_out(c)[2], c["theta"][2])
        n_override += c["status"] != 2 and moved and np.abs(ci[2, :, :3]).max() > 0
    assert n_override >= 2
    # exp: cases whose guess ends more than 1 m from its start (no terminal ball: certified)
    far = [c for c in cases if c["set"] == "exp" and c["status"] == 0 and not bool(c["qc"])]
    assert len(far) >= 2 and all(c["certified"] for c in far)
    assert any(abs(float(c["weight"]) - 1e5) < 1 for c in cases) and any(float(c["T"]) == 0.3 for c in cases) and any(float(c["T"]) == 1.0 for c in cases)
    assert any(float(c["mins"][2]) == -1.0 for c in cases)
    import os
    assert os.path.getsize(os.path.join(helpers.ROOT, "tests", "golden", FIXTURE)) < 400 * 1024


def test_reduced_model_matches_oracle_on_params(oracle):
    """reduced_ipm_ref (the numpy model of what the HIP kernels implement) against the oracle on the new fixture, at the bar of
    test_reduced_model_matches_oracle"""
    import reduced_ipm_ref as R
    for c in helpers.load_qp_cases(FIXTURE):
        p = helpers.params_of_case(c)
        r = oracle.optimize(p, 1, c["coeff_init"], [], [], lines=(c["line_seg"], c["line_nd"]))
        st, th, obj, it = R.optimize(c["K"], p.T_span, p.weight, c["coeff_init"], c["mins"], c["maxs"], p.v_max, p.a_max,
                                     c["line_seg"], c["line_nd"])
        assert st == r["status"], c["tag"]
        assert np.abs(th - r["coeff"]).max() < 1e-6, (c["tag"], np.abs(th - r["coeff"]).max())


def test_minvo_control_points_exact_at_other_spans(oracle):
    """MINVO position / velocity control points at T in {0.3, 1.0} against exact rational arithmetic on the reference's literal
    matrices (make_golden.frac_inv), the way minvo_kat.json's vectors are checked: 5e-14 relative"""
    import sys, os
    sys.path.insert(0, os.path.join(helpers.ROOT, "tests", "golden"))
    import make_golden as mg
    rng = np.random.default_rng(4321)
    for T in (0.3, 1.0):
        for _ in range(12):
            P = [float(x) for x in rng.normal(size=4) * 3]
            Tf = F(T); Pf = [F(x) for x in P]
            tp = [Tf ** 3, Tf ** 2, Tf, F(1)]; tv = [3 * Tf ** 2, 2 * Tf, F(1)]
            q = np.array([float(sum(Pf[j] * tp[j] * mg.APINV_F[j][k] for j in range(4))) for k in range(4)])
            v = np.array([float(sum(Pf[j] * tv[j] * mg.AVINV_F[j][k] for j in range(3))) for k in range(3)])
            np.testing.assert_allclose(oracle.pos_ctrl_pts(P, T), q, rtol=0, atol=5e-14 * (1 + np.abs(q).max()))
            np.testing.assert_allclose(oracle.vel_ctrl_pts(P, T), v, rtol=0, atol=5e-14 * (1 + np.abs(v).max()))


@pytest.mark.parametrize("T,dc", [(0.3, 0.02), (1.0, 0.05), (0.5, 0.05)])
def test_sampling_against_horner_at_other_spans(oracle, T, dc):
    """oracle.sample against a plain Horner evaluation on the time walk of solver_gurobi_poly.cpp:911-934 restated on its own;
    the number of states is what Params.max_states allows for"""
    K = 8
    co = np.random.default_rng(2).normal(size=(3, K, 4))
    p = scene.Params(T_span=T, dc=dc)
    st = oracle.sample(co, T, dc, cap=p.max_states)
    t = 0.0; i = 0; out = []
    while i < K:
        dt = t - i * T
        row = []
        for d in range(4):
            for ax in range(3):
                a, b, c_, e = co[ax, i]
                row.append([((a * dt + b) * dt + c_) * dt + e, (3 * a * dt + 2 * b) * dt + c_, 6 * a * dt + 2 * b, 6 * a][d])
        out.append(row)
        t += dc
        if t > (i + 1) * T:
            i += 1
    out = np.array(out)
    assert len(st) == len(out) <= p.max_states and len(st) >= p.max_states - 4
    np.testing.assert_allclose(st, out, rtol=0, atol=1e-12)


def _record(rng, n_seg, T, t0, bbox):
    r = np.zeros(1, dtype=abi.TRAJ_REC_DTYPE)[0]
    co = np.zeros((3, n_seg, 4))
    for ax in range(2):
        # (a start acceleration of its own per axis: a straight constant-speed segment has collinear control points, whose hull's
        #  vertex list is decided by rounding)
        co[ax] = scene._rollout_axis(rng.uniform(-5, 5), rng.uniform(-1, 1), rng.uniform(0.5, 2.0) * (1 - 2 * ax), rng.uniform(-8, 8), T, n_seg, 2.0, 3.0)
    r["id"] = 1; r["is_agent"] = 1; r["valid"] = 1; r["bbox"] = bbox
    r["pwp"]["n_seg"] = n_seg; r["pwp"]["times"][:n_seg + 1] = t0 + np.arange(n_seg + 1) * T
    r["pwp"]["coeff"][:, :n_seg, :] = co
    return r, co


@pytest.mark.parametrize("T", [0.3, 0.5, 1.0])
def test_oracle_hulls_with_mixed_boxes_and_window_positions(oracle, T):
    """orc_hull_of_interval against scene.interval_hull generalised to a rectangular inflation (the x and y half-boxes differ:
    bbox / 2 + drone_radius per axis, neptune.cpp:436-446) for windows that start before the first knot, lie inside, straddle the last
    knot and lie wholly after it, records of 1, 3 and 8 segments, knots off the query grid"""
    rng = np.random.default_rng(int(T * 10))
    n_checked = 0
    for n_seg in (1, 3, 8):
        for bbox in PU.MIXED_BOXES + ((0.7, 0.7, 0.7),):
            for radius in (0.35, 0.6):
                r, co = _record(rng, n_seg, T, t0=0.37 * T, bbox=np.array(bbox))
                pw = abi.nep_pwp.from_buffer_copy(r["pwp"].tobytes())
                times = np.array(r["pwp"]["times"])[:n_seg + 1]
                d = np.array([bbox[0] / 2 + radius, bbox[1] / 2 + radius])
                t_end = times[-1]
                for w0 in (0.0, times[0] + 0.5 * T, t_end - 0.5 * T, t_end + 0.25 * T, t_end + 3 * T):
                    h, h0 = oracle.hull_of_interval(pw, w0, w0 + T, T, d)
                    q = scene.interval_ctrl_pts(times, co[:2], w0, w0 + T, T)
                    c = np.array([[d[0], d[1]], [d[0], -d[1]], [-d[0], -d[1]], [-d[0], d[1]]])
                    want = scene.hull_ccw_lexmin((q[:, None, :] + c[None, :, :]).reshape(-1, 2))
                    # (numpy's matrix product and the C loop add a control point's four terms in different orders: the vertices agree
                    #  to 4 * 2^-53 * sum |terms| <= 1e-14 at these coordinates, not bit for bit; same vertices in the same order)
                    want0 = scene.hull_ccw_lexmin(q)
                    assert h.shape == want.shape and h0.shape == want0.shape, (n_seg, bbox, w0)
                    np.testing.assert_allclose(h, want, rtol=0, atol=1e-13, err_msg="n_seg %d bbox %r window %g" % (n_seg, bbox, w0))
                    np.testing.assert_allclose(h0, want0, rtol=0, atol=1e-13)
                    assert h[:, 0].max() - h[:, 0].min() >= 2 * d[0] and h[:, 1].max() - h[:, 1].min() >= 2 * d[1]
                    n_checked += 1
    assert n_checked == 3 * 5 * 2 * 5


@pytest.mark.parametrize("name", PS.SWEPT)
def test_swept_scenes_are_not_vacuous(oracle, name):
    """What the GPU sweep relies on, fixed by the oracle alone: every set's 8 agent + 6 obstacle scene has lines; with z motion at
    least one replan has an active z row (exp: the z override applies to a z guess that is not flat — its horizon covers less than
    the override's 1 m); fast_long has replans with an active separating-line row."""
    for K in PS.guess_lengths(name):
        sc = PU.with_z_motion(PS.make_scene(name, 8, 6, seed=5, K=K), np.random.default_rng(107))
        p = sc["par"]
        assert p.max_states == int(np.ceil(p.num_pol * p.T_span / p.dc)) + 3
        n_lines = n_z = n_line_act = n_over = 0
        for a in range(8):
            g = sc["guesses"][a]
            r = oracle.replan(p, a + 1, sc["committed"], g, sc["statics"])
            n_lines += r["n_lines"]
            if r["status"] != 2:
                n_z += PU.z_active_rows(p, r["coeff"], K) > 0
                n_line_act += scene.active_rows(p, r["coeff"], K, r["line_seg"], r["line_nd"])[1] > 0
                gz = np.array(g["coeff"])[2, :K]
                n_over += np.array_equal(r["coeff"][2], gz) and np.abs(gz[:, :3]).max() > 0
        assert n_lines > 0
        if name == "exp":
            assert n_over >= 1
        else:
            assert n_z >= 1
        if name == "fast_long":
            assert n_line_act >= 1


def test_modifiers_keep_the_problem(oracle):
    """translated: the translated problem's optimum is the translated optimum (two oracle solves, each held to 1e-8 by the golden sets: 2e-8) with the same statuses and counts;
    with_mixed_boxes: at most 20 % of the LPs of any replan fail in the scenes the GPU sweep flies"""
    for name in ("default", "fast_long"):
        sc = PU.with_z_motion(PS.make_scene(name, 8, 6, seed=5), np.random.default_rng(107))
        tr = PU.translated(sc, 23.0, -42.5)
        p, pt = sc["par"], tr["par"]
        assert (pt.x_min, pt.x_max) == (p.x_min + 23.0, p.x_max + 23.0) and pt.x_min > 0 and pt.y_max < 0
        for a in range(8):
            r0 = oracle.replan(p, a + 1, sc["committed"], sc["guesses"][a], sc["statics"])
            r1 = oracle.replan(pt, a + 1, tr["committed"], tr["guesses"][a], tr["statics"])
            assert (r0["status"], r0["n_lp"], r0["n_lp_failed"]) == (r1["status"], r1["n_lp"], r1["n_lp_failed"])
            want = r0["coeff"].copy(); want[0, :, 3] += 23.0; want[1, :, 3] -= 42.5
            err = np.abs(r1["coeff"] - want).max()
            print("%s agent %d: |translated optimum - optimum translated| = %.2e" % (name, a + 1, err))
            assert err <= 2e-8, (name, a, err)       # (two oracle solves, each within 1e-8 of its optimum by the golden bar)
    for name in ("default", "exp"):
        n_failed = 0
        for seed, sizes in ((5, PU.MIXED_BOXES), (6, PU.MIXED_BOXES), (10, PU.WIDE_BOXES)):      # (the scenes of test_gpu_param_sweep.py)
            sc = PU.with_mixed_boxes(PS.make_scene(name, 8, 6, seed=seed), np.random.default_rng(200 + seed), sizes=sizes)
            assert len({tuple(b) for b in np.array(sc["committed"]["bbox"])}) >= 3
            for a in range(8):
                r = oracle.replan(sc["par"], a + 1, sc["committed"], sc["guesses"][a], sc["statics"])
                assert r["n_lp"] > 0 and r["n_lp_failed"] <= 0.2 * r["n_lp"]
                n_failed += r["n_lp_failed"]
        assert n_failed >= 1 or name != "default"          # failed LPs are part of what the default set's sweep compares


def test_no_set_is_refused_and_a_ninth_interval_is():
    """A configuration the library refuses by design is an error with a message, never a wrong answer: nep_batch_create takes every set
    of the table (without a GPU it gets as far as "no HIP device": the configuration itself passed) and turns down num_pol = 9 (more
    intervals than NEP_MAX_POL) and a non-positive max_states with "bad batch configuration"."""
    import ctypes as C
    import dataclasses
    from neptune_amd import _lib
    L = _lib.lib()

    def create(p, max_states=None):
        pb = np.ascontiguousarray(p.pb, dtype=np.float64); off = np.zeros(1, dtype=np.int32); xy = np.zeros((1, 2))
        cfg = abi.nep_batch_cfg(p.num_agents, 0, p.num_agents, p.num_pol, 0, 0, p.max_states if max_states is None else max_states, 1,
                                p.T_span, p.weight, p.dc, p.drone_radius, p.x_min, p.x_max, p.y_min, p.y_max, p.z_min, p.z_max,
                                p.v_max, p.a_max, abi.dptr(pb), abi.iptr(off), abi.dptr(xy))
        h = L.nep_batch_create(C.byref(cfg))
        err = L.nep_last_error()
        if h:
            L.nep_batch_destroy(h)
        return bool(h), err
    import torch
    for name in PS.SWEPT:
        ok, err = create(PS.params(name, 8, 0))
        assert ok if torch.cuda.is_available() else (not ok and b"no HIP device" in err), (name, err)
    ok, err = create(dataclasses.replace(PS.params("default", 8, 0), num_pol=abi.NEP_MAX_POL + 1))
    assert not ok and b"bad batch configuration" in err
    ok, err = create(PS.params("exp", 8, 0), max_states=0)
    assert not ok and b"bad batch configuration" in err
