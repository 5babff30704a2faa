"""Input modifiers of the parameter sweep, each applicable on top of any set of param_sets.py.  They live here and not in
neptune_amd/scene.py: the benchmark's workloads are that module's outputs and stay what they are.  Every modifier returns a
new scene (deep copy); the oracle decides the reference value of the modified scene as everywhere else."""
import copy
import dataclasses

import numpy as np

from neptune_amd import scene

MIXED_BOXES = ((0.4, 2.0, 0.6), (1.6, 0.5, 1.0), (1.0, 1.0, 2.0), (0.7, 1.4, 0.7))
# with two long thin ones: by the oracle the default set's 8 + 6 scene of seed 10 then has replans with failed LPs (2 of 70)
WIDE_BOXES = MIXED_BOXES + ((3.0, 0.6, 0.6), (0.6, 3.6, 0.6))


def with_z_motion(sc, rng):
    """The z coefficients of every guess and committed record replaced by a scene._rollout_axis climb or descent between heights
    INSIDE the z box: about a third aimed 2 cm from z_min / z_max (the optimum then tends to put a z control point on the bound),
    about a quarter starting with a vertical speed of 0.85 v_max where the box leaves room to brake (capped by
    sqrt(0.8 a_max * half the room) otherwise).  The separator is 2-D: the LPs of the scene are unchanged."""
    sc = copy.deepcopy(sc)
    p = sc["par"]; T = p.T_span
    lo, hi = p.z_min, p.z_max
    for a in range(p.num_agents):
        g = sc["guesses"][a]; K = int(g["K"])
        u = rng.uniform()
        z0 = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo))
        v0 = 0.0
        if u < 0.33:
            # within reach of the horizon, so that the guess ends next to the bound
            up = rng.uniform() < 0.5
            goal = hi - 0.02 if up else lo + 0.02
            dist = rng.uniform(0.1, 0.6) * min(0.2 * p.v_max * K * T, 0.6 * (hi - lo))
            z0 = goal - dist if up else goal + dist
        else:
            goal = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo))
        if rng.uniform() < 0.25:
            up = goal >= z0
            z0 = lo + 0.15 * (hi - lo) if up else hi - 0.15 * (hi - lo)
            room = 0.5 * (hi - lo)
            v0 = (1.0 if up else -1.0) * min(0.85 * p.v_max, np.sqrt(0.8 * p.a_max * 0.5 * room))
        co = scene._rollout_axis(z0, v0, 0.0, goal, T, K, p.v_max, p.a_max)
        g["coeff"][2][:, :] = 0.0
        g["coeff"][2][:K, :] = co
        r = sc["committed"][a]; n = int(r["pwp"]["n_seg"])
        r["pwp"]["coeff"][2][:, :] = 0.0
        r["pwp"]["coeff"][2][:min(n, K), :] = co[:min(n, K)]
        if n > K:
            r["pwp"]["coeff"][2][K:n, 3] = co[K - 1] @ np.array([T ** 3, T ** 2, T, 1.0])
        r["pos"][2] = z0
        sc["goals"][a][2] = goal
    return sc


def translated(sc, dx, dy):
    """The whole scene moved by (dx, dy): bases, statics, constant terms of every coefficient set, positions, bend points, starts,
    goals and the world box — a world that is neither centred on the origin nor symmetric about it."""
    sc = copy.deepcopy(sc)
    p0 = sc["par"]
    d = np.array([dx, dy], dtype=np.float64)
    sc["par"] = dataclasses.replace(p0, x_min=p0.x_min + dx, x_max=p0.x_max + dx, y_min=p0.y_min + dy, y_max=p0.y_max + dy,
                                    pb=np.asarray(p0.pb, dtype=np.float64) + d)
    sc["statics"] = [np.asarray(s, dtype=np.float64) + d for s in sc["statics"]]
    sc["statics_raw"] = [np.asarray(s, dtype=np.float64) + d for s in sc["statics_raw"]]
    sc["starts"] = np.asarray(sc["starts"], dtype=np.float64) + d
    sc["goals"] = np.array(sc["goals"], dtype=np.float64); sc["goals"][:, :2] += d
    for a in range(p0.num_agents):
        g = sc["guesses"][a]; K = int(g["K"])
        r = sc["committed"][a]; n = int(r["pwp"]["n_seg"]); nb = int(r["n_bend"])
        for ax in range(2):
            g["coeff"][ax][:K, 3] += d[ax]
            r["pwp"]["coeff"][ax][:n, 3] += d[ax]
            r["pos"][ax] += d[ax]
        r["bend"][:nb] += d
    return sc


def with_mixed_boxes(sc, rng, sizes=MIXED_BOXES):
    """Per-record bbox drawn from a few non-square sizes (every committed scene record has 2 * drone_radius on all axes).
    make_scene's acceptance test then no longer guarantees feasible LPs: failed LPs are part of what is compared."""
    sc = copy.deepcopy(sc)
    for a in range(sc["par"].num_agents):
        sc["committed"][a]["bbox"] = np.array(sizes[int(rng.integers(0, len(sizes)))])
    return sc


def z_active_rows(p, coeff, K, tol=1e-6):
    """z position / velocity / acceleration rows of the spline QP (solver_gurobi_poly.cpp:433-489) active at `coeff` [3][K][4]"""
    T = p.T_span
    M4 = scene.A_POS_INV * np.array([T ** 3, T ** 2, T, 1.0])[:, None]
    V3 = scene.A_VEL_INV * (np.array([3.0, 2.0, 1.0]) * np.array([T ** 2, T, 1.0]))[:, None]
    q = coeff[2, :K] @ M4; v = coeff[2, :K, :3] @ V3; a = 6 * T * coeff[2, :K, 0] + 2 * coeff[2, :K, 1]
    return int((q > p.z_max - tol).sum() + (q < p.z_min + tol).sum() + (np.abs(v) > p.v_max - tol).sum() + (np.abs(a) > p.a_max - tol).sum())
