#!/usr/bin/env python3
"""Golden QP cases away from the default parameter point (tests/golden/qp_cases_params.npz).

The two earlier sets (make_golden.py, make_golden_r2.py) were all drawn at T_span 0.5, weight 1000, v_max 2, a_max 3, z box
(-0.2, 5.1), num_pol 8, with flat z guesses.  This one is built the same way — the reference's QP in its own 12K-variable space
(make_golden.build_qp), SciPy trust-constr + SLSQP with row generation, accepted on the KKT certificate
(make_golden_r2.solve_two_ways_rowgen); the oracle supplies only inputs (the separating lines of the scenes) — at every set of
tests/param_sets.py, with z guesses that climb or descend (tests/param_util.with_z_motion):

  per set    two replans of an 8 agent + 6 obstacle scene with z motion (preferring agents whose optimum, by the oracle, has an
             active separating-line row / an active z row) and one `tight_lines` case on a scene guess
  exp, fast_long   "nostop" (RELAXED) and "contradictory" (FAILED) re-derived for those bounds
  exp        a hover with a z climb and a short hop (terminal ball: where the ball row is inactive at the answer the QP
             certificate is taken on the linear rows, ball_inactive_certificate; otherwise the case is accepted on the agreement
             of the two solvers to 1e-7 in coefficients) and two guesses that end more than 1 m (3-D) from their start
  default    xy hops shorter than 1 m with a climb longer than 1 m: no ball, but the reference's z override applies to a non-flat z

Per case also: `num_pol` of the handle, `n_active_z` (z rows active at the optimum, before the z override), `certified`.
Cases without a certificate / agreement are dropped and listed at the end; the run fails if more than a quarter are dropped or a
set keeps fewer than three.

Oracle against this file (test_oracle_params.test_oracle_against_golden_params), measured when it was made: 33 attempted, one
dropped (exp nostop K2: ball active, solvers 1.6e-7 apart), all 32 kept cases certified; worst coefficient error 2.1e-9 (heavy;
every other set below 8e-10) against the bar of 1e-8.

Run from the repo root:  python tests/golden/make_golden_params.py      (a few minutes)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import make_golden_r2 as r2  # noqa: E402
import param_sets as PS  # noqa: E402
import param_util as PU  # noqa: E402

Z_SEED = 107
ATTEMPTED, DROPPED = [], []


def one_case(name, tag, p, K, ci, seg, nd, cases):
    tag = "%s %s" % (name, tag)
    ATTEMPTED.append(tag)
    before = len(cases)
    mg._one_case(tag, p, K, ci, seg, nd, cases)
    if len(cases) == before:
        DROPPED.append((tag, "no certificate / solvers disagree")); return None
    c = cases[-1]
    cert = c["status"] == 2 or not c["qc"]
    if not cert:
        Q = mg.build_qp(K, p.T_span, p.weight, c["mins"], c["maxs"], p.v_max, p.a_max, ci, c["line_seg"], c["line_nd"], relaxed=c["status"] == 1)
        cert = ball_inactive_certificate(Q, c["theta"])
    if not cert and c["dth"] > 1e-7:
        cases.pop(); DROPPED.append((tag, "terminal ball active, no certificate, and the two solvers stop %.1e apart" % c["dth"])); return None
    c["set"] = name; c["num_pol"] = p.num_pol
    c["certified"] = int(cert)
    c["n_active_z"] = PU.z_active_rows(p, c["theta"], K) if c["status"] != 2 else 0
    print("     set=%s num_pol=%d certified=%d n_active_z=%d" % (name, p.num_pol, c["certified"], c["n_active_z"]), flush=True)
    return c


def ball_inactive_certificate(Q, theta):
    """A terminal-ball problem (make_golden_r2.solve_certified leaves those to the agreement of the two solvers) whose ball row
    is INACTIVE at the answer is a QP there: the answer is the optimum if it is feasible to 1e-9, the ball has slack and
    non-negative multipliers of the active linear rows make the gradient vanish to 1e-8 relative (bounded least squares)."""
    from scipy.optimize import lsq_linear
    x = np.asarray(theta, dtype=np.float64).reshape(-1)
    G, h, E, e = Q["G"], Q["h"], Q["E"], Q["e"]
    nrm = np.linalg.norm(G, axis=1); nrm[nrm == 0] = 1.0
    slack = (h - G @ x) / nrm
    if np.abs(E @ x - e).max() > 1e-9 or slack.min() < -1e-9:
        return False
    if -(x @ Q["Cq"] @ x + 2 * Q["cq"] @ x + Q["cc"]) < 1e-6:
        return False
    act = np.where(slack < 1e-7)[0]
    A = np.concatenate([E, G[act] / nrm[act, None]]).T
    g = Q["P"] @ x + Q["q"]
    lb = np.concatenate([np.full(len(E), -np.inf), np.zeros(len(act))])
    r = lsq_linear(A, -g, bounds=(lb, np.full(len(lb), np.inf)), tol=1e-14, lsmr_tol="auto" if A.shape[1] > 2000 else None)
    res = np.abs(A @ r.x + g).max()
    ok = res <= 1e-8 * (1 + np.abs(Q["q"]).max())
    print("  (ball inactive: %d active linear rows, stationarity residual %.1e -> %s)" % (len(act), res, "certified" if ok else "not certified"), flush=True)
    return bool(ok)


def rollout3(p0, v0, goal, p, K):
    """scene.rollout with a rolled-out z as well"""
    from neptune_amd import scene
    co = scene.rollout(np.array(p0, dtype=float), np.array(v0, dtype=float), np.zeros(3), np.array(goal, dtype=float), p, K)
    co[2] = scene._rollout_axis(p0[2], v0[2], 0.0, goal[2], p.T_span, K, p.v_max, p.a_max)
    return co


def cases_params():
    from neptune_amd import scene
    from oracle import oracle
    cases = []
    for name in ("default",) + PS.SWEPT:
        for K in PS.guess_lengths(name):
            sc = PU.with_z_motion(PS.make_scene(name, 8, 6, seed=5, K=K), np.random.default_rng(Z_SEED))
            p = sc["par"]
            info = []
            for a in range(p.num_agents):
                r = oracle.replan(p, a + 1, sc["committed"], sc["guesses"][a], sc["statics"])   # inputs only: the lines
                nl = scene.active_rows(p, r["coeff"], K, r["line_seg"], r["line_nd"], tol=1e-5)[1] if r["status"] != 2 else 0
                nz = PU.z_active_rows(p, r["coeff"], K, tol=1e-5) if r["status"] != 2 else 0
                info.append((a, r, nl, nz))
            pick = [i for i in info if i[2] > 0][:1]
            pick += [i for i in info if i[3] > 0 and i not in pick][:2 - len(pick)]
            pick += [i for i in info if i not in pick][:2 - len(pick)]
            if name == "default" or len(PS.guess_lengths(name)) > 1:
                pick = pick[:1]
            for a, r, nl, nz in pick:
                ci = np.array(sc["guesses"][a]["coeff"])[:, :K, :]
                one_case(name, "scene z K%d a%d" % (K, a + 1), p, K, ci, r["line_seg"], r["line_nd"], cases)
            rng = np.random.default_rng(300 + K)
            a = int(rng.integers(0, p.num_agents))
            ci = np.array(sc["guesses"][a]["coeff"])[:, :K, :]
            seg, nd = mg.tight_lines(ci, p.T_span, rng, per_seg=2)
            one_case(name, "tight z K%d a%d" % (K, a + 1), p, K, ci, seg, nd, cases)
    for name in ("exp", "fast_long"):
        p = PS.params(name, 5, 0)
        v = 0.95 * p.v_max
        for K in (1, 2):       # cannot stop in time: the relaxed problem is the one that is solved
            ci = scene.rollout(np.array([0.0, 0.0, 1.0]), np.array([v, 0.5 * v, 0.0]), np.array([0.3 * p.a_max, 0.0, 0.0]),
                               np.array([8.0 * v, 3.0 * v, 1.0]), p, K)
            ci[2] = scene._rollout_axis(1.0, 0.3 * v, 0.0, p.z_max - 0.3, p.T_span, K, p.v_max, p.a_max)
            one_case(name, "nostop K%d" % K, p, K, ci, [], [], cases)
        ci = rollout3([0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [4.0 * v, 1.0 * v, 0.5 * (p.z_min + p.z_max)], p, 8)
        one_case(name, "contradictory", p, 8, ci, [2, 2], [[2.0, 0.0, 1 - 2.0 * 0.0], [-2.0, 0.0, 1 + 2.0 * 50.0]], cases)
    p = PS.params("exp", 5, 0)
    ci = np.zeros((3, 8, 4)); ci[0, :, 3] = 2.0; ci[1, :, 3] = -3.0
    ci[2] = scene._rollout_axis(0.6, 0.0, 0.0, 1.0, p.T_span, 8, p.v_max, p.a_max)
    one_case("exp", "hover climb K8", p, 8, ci, [], [], cases)
    ci = rollout3([1.0, 1.0, 1.0], [0.2, -0.1, 0.0], [1.4, 0.7, 1.3], p, 8)
    seg, nd = mg.tight_lines(ci, p.T_span, np.random.default_rng(31), per_seg=1)
    one_case("exp", "hop qc", p, 8, ci, seg, nd, cases)
    ci = rollout3([0.0, 0.0, 0.3], [0.5, 0.3, 0.3], [3.0, 2.0, p.z_max - 0.02], p, 8)
    one_case("exp", "far xy K8", p, 8, ci, [], [], cases)
    ci = rollout3([0.0, 0.0, 0.2], [0.4, 0.0, 0.4], [0.8, 0.1, p.z_max - 0.02], p, 8)
    seg, nd = mg.tight_lines(ci, p.T_span, np.random.default_rng(32), per_seg=1)
    one_case("exp", "far z override K8", p, 8, ci, seg, nd, cases)
    p = PS.params("default", 5, 0)
    for k, (goal, z0) in enumerate((([1.5, 0.6, p.z_max - 0.02], 3.0), ([0.6, 1.5, p.z_min + 0.02], 2.0))):
        ci = rollout3([1.0, 1.0, z0], [0.2, -0.1, 0.0], goal, p, 8)
        seg, nd = mg.tight_lines(ci, p.T_span, np.random.default_rng(33 + k), per_seg=1)
        one_case("default", "z override no ball %d" % k, p, 8, ci, seg, nd, cases)
    return cases


if __name__ == "__main__":
    mg.solve_two_ways = r2.solve_two_ways_rowgen
    cases = cases_params()
    print("attempted %d, kept %d, dropped %d:" % (len(ATTEMPTED), len(cases), len(DROPPED)))
    for tag, why in DROPPED:
        print("  dropped %s: %s" % (tag, why))
    assert len(DROPPED) * 4 <= len(ATTEMPTED), "more than a quarter of the attempted cases dropped"
    for name in PS.SWEPT:
        assert sum(c["set"] == name for c in cases) >= 3, name
    mg.save_qp_cases(cases, name="qp_cases_params.npz")
