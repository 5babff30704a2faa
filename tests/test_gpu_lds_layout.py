"""GPU: the kernels whose dynamic-LDS carve comes from csrc/lds_layout.h, at small shapes on both sides of the layouts' branches
(tests/test_lds_layout_cpu.py pins the byte counts; here the kernels run on what the layouts hand them).  One scene per case.

Cases here: the front end's r_f alias (beam 32: N + S = 7 | 8, beam 33: 14 | 15), the cap floor (beam 1, lattice 2), the entangle
tail at N = 33 (two mask words, N mod 4 = 1) with 0 and 33 statics; the unpacked separator's pool floor with the entangle rows
(N = 89 | 90).  (The packed separator keeps its own carve: DESIGN.md section 30.)

The entangle re-check with two ballots of agents and of statics (N = S = 65); the audit with an odd number of agents, with and without
static polygons; the mission kernel with no keep-out polygon and with NEP_MISSION_MAX_POLY of them.

The safety resolve at N = 33 (two words per conflict row) and N = 257 (nine words, the accepted set in LDS) against the host rule
of safety_cases.py; test_gpu_safety_sizes.py runs the same sides of both branches at N = 37 and 261 with more scenes and settings."""
import dataclasses
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers
from neptune_amd import abi, scene
from gpu_util import COEF_TOL, lines_match

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


# ---- the front end ----

@pytest.mark.parametrize("n_agents,n_static,W,ns", [(5, 2, 32, 5), (6, 2, 32, 5), (12, 2, 33, 5), (13, 2, 33, 5), (5, 2, 1, 2)])
def test_frontend_beam_on_both_sides_of_the_winners_alias(be, oracle, n_agents, n_static, W, ns):
    """results and guesses byte-equal to the oracle's beam (as gpu_util.check_frontend_beam compares them)"""
    sc = scene.make_scene(n_agents, n_static, seed=3)
    p = sc["par"]; N = n_agents
    assert len(sc["statics"]) == n_static
    fe = scene.frontend_cfg(p, beam_width=W, num_samples=ns)
    starts = scene.frontend_starts(sc)
    bb = be.BatchBackend(p, sc["statics"])
    T = bb.torch
    d_guess = T.zeros(N * abi.GUESS_DTYPE.itemsize, dtype=T.uint8, device=bb.device)
    d_res = T.zeros(N * abi.FE_RESULT_DTYPE.itemsize, dtype=T.uint8, device=bb.device)
    bb.frontend(fe, bb.to_device(sc["committed"]), bb.to_device(starts), d_guess, d_res)
    bb.check()
    got_g = d_guess.cpu().numpy().view(abi.GUESS_DTYPE); got_r = d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE)
    found = 0
    for a in range(N):
        hx, hn = oracle.hulls_of_scene(p, a + 1, sc["committed"], float(starts[a]["t_start"]), sc["statics"])
        g, r = oracle.frontend_beam(p, fe, a + 1, starts[a], hx, hn, sc["statics"])
        for f in abi.FE_RESULT_DTYPE.names:
            assert got_r[a][f] == r[f], (a, f, got_r[a][f], r[f])
        assert int(got_g[a]["K"]) == int(g["K"]) and got_g[a]["t_start"] == g["t_start"]
        np.testing.assert_array_equal(got_g[a]["coeff"], g["coeff"])
        found += int(g["K"]) > 0
    assert found >= 1
    bb.close()


@pytest.mark.parametrize("n_static", [0, 33])
def test_frontend_entangle_tail_at_33_agents(be, oracle, n_static):
    """two words of agents per rank mask, f_bits padded (33 mod 4 = 1), no and two words of statics: guesses, counters and case blocks
    against the oracle, as test_gpu_frontend_entangle.py compares them (every third agent)"""
    N = 33
    sc = scene.tether_crossing_scene(N, n_static, 71)
    assert len(sc["statics"]) == n_static
    p = sc["par"]
    fe = scene.frontend_cfg(p, beam_width=16, entangle=True)
    bb = be.BatchBackend(p, sc["statics"])
    reps, longest = scene.static_reps(sc["statics"]) if n_static else (np.zeros((0, 2, 2)), np.zeros((0, 2)))
    bb.set_static_reps(reps, longest)
    T = bb.torch
    starts = scene.frontend_starts(sc)
    d_g = T.zeros(N * abi.GUESS_DTYPE.itemsize, dtype=T.uint8, device=bb.device)
    d_r = T.zeros(N * abi.FE_RESULT_DTYPE.itemsize, dtype=T.uint8, device=bb.device)
    d_case = T.zeros(N * abi.NEP_MAX_POL * N, dtype=T.int32, device=bb.device)
    bb.frontend_ent(fe, bb.to_device(sc["committed"]), bb.to_device(starts), d_g, d_r, d_case)
    bb.check()
    got_g = d_g.cpu().numpy().view(abi.GUESS_DTYPE); got_r = d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE)
    got_case = d_case.cpu().numpy().reshape(N, abi.NEP_MAX_POL, N)
    for a in range(0, N, 3):
        hx, hn = oracle.hulls_of_scene(p, a + 1, sc["committed"], float(starts[a]["t_start"]), sc["statics"])
        ent = helpers.ent_inputs(sc, a, t0=float(starts[a]["t_start"]))
        g, res, case = oracle.frontend_beam_ent(p, fe, a + 1, starts[a], hx, hn, sc["statics"], ent)
        assert int(got_g[a]["K"]) == int(g["K"]), a
        np.testing.assert_array_equal(np.array(got_g[a]["coeff"]), np.array(g["coeff"]), err_msg="agent %d" % a)
        for f in ("status", "K", "n_children", "n_feasible", "n_collision_free", "n_entangled", "ent_overflow"):
            assert int(got_r[a][f]) == res[f], (a, f, int(got_r[a][f]), res[f])
        np.testing.assert_array_equal(got_case[a], case, err_msg="case block of agent %d" % a)
    bb.close()


# ---- the separators ----

def _ent_scene(N, seed):
    sc = scene.make_scene(N, 0, seed=seed)
    case_id = scene.synthetic_entangle(sc, seed=seed + 1, frac=0.1)
    return sc, case_id, dataclasses.replace(sc["par"], enable_entangle=True)


def _replan_outputs(bb, sc, case_id=None):
    d_ent = bb.torch.from_numpy(case_id.reshape(-1).copy()).to(bb.device) if case_id is not None else None
    bb.replan(bb.to_device(sc["committed"]), bb.to_device(sc["guesses"]), d_ent=d_ent)
    bb.check()
    sol = bb.solutions().copy(); sol["stats"]["solve_us"] = 0.0
    out = {"sol": sol, "states": bb.states().copy(), "commit": bb.commits().copy(), "marks": bb.debug_presolved()}
    for s in range(bb.slots):
        out["line_seg_%d" % s], out["line_nd_%d" % s] = bb.debug_lines(s)
    return out


@pytest.mark.parametrize("N", [89, 90])
def test_unpacked_separator_at_its_pool_floor_with_the_entangle_rows(be, oracle, N):
    """separator_pack = -1 on an entangle handle, no statics: N = 89 is the last size whose wave stays at 10 KiB, at 90 the pool is at
    its floor of 64 x 8 pairs.  Every slot's lines and counts against the oracle's separator, the solve as test_gpu_parity.py compares it."""
    sc, case_id, p = _ent_scene(N, 40)
    oracle.lib()
    with ThreadPoolExecutor(16) as ex:
        ref = list(ex.map(lambda a: oracle.replan(p, a + 1, sc["committed"], sc["guesses"][a], sc["statics"], case_id=case_id[a]), range(N)))
    for cull in (0.0, None):                       # every line in the reference's call order; the handle's default presolve
        bb = be.BatchBackend(p, sc["statics"])
        bb.set_separator_pack(-1)
        if cull is not None:
            bb.set_line_cull(cull)
        out = _replan_outputs(bb, sc, case_id)
        st = out["sol"]["stats"]
        for a, r in enumerate(ref):
            lines_match(bb, out["line_seg_%d" % a], out["line_nd_%d" % a], r)
            K = int(out["sol"][a]["K"])
            assert int(st[a]["status"]) == r["status"] and int(st[a]["n_lines"]) == r["n_lines"], (cull, a)
            assert int(st[a]["n_lp"]) == r["n_lp"] and int(st[a]["n_lp_failed"]) == r["n_lp_failed"], (cull, a)
            assert np.abs(np.array(out["sol"][a]["coeff"])[:, :K, :] - r["coeff"]).max() <= COEF_TOL, (cull, a)
        bb.close()
    assert sum(r["n_lp"] for r in ref) > 0


# ---- the entangle re-check of the safety pass ----

def test_entangle_recheck_with_two_mask_words_of_agents_and_statics(be, oracle):
    """nep_batch_safety_commit_ent at N = 65, S = 65 (two 64-bit ballots each): the flags equal the oracle's entangleCheckGivenPwp on
    every new trajectory, a flagged agent keeps its previous record (as test_gpu_frontend_entangle.py::test_safety_pass_entangle_recheck)"""
    N = 65
    sc = scene.tether_crossing_scene(N, 65, 72)
    assert len(sc["statics"]) == 65
    p = sc["par"]
    bb = be.BatchBackend(p, sc["statics"])
    reps, longest = scene.static_reps(sc["statics"])
    bb.set_static_reps(reps, longest)
    T = bb.torch
    d_prev = bb.to_device(sc["committed"]); d_guess = bb.to_device(sc["guesses"])
    bb.replan(d_prev, d_guess)
    fresh = bb.commits()
    inits = np.zeros(N, dtype=abi.FE_ENT_STATE_DTYPE)
    for a in range(N):
        j = (a + 3) % N
        inits[a]["n_alpha"] = 1; inits[a]["id"][0] = j + 1; inits[a]["cs"][0] = 1
    d_final = T.zeros_like(bb.d_commit); d_acc = T.zeros(N, dtype=T.int32, device=bb.device)
    bb.safety_commit_ent(d_prev, bb.d_commit, d_guess, d_final, d_acc, d_ent_init=bb.to_device(inits))
    bb.check()
    acc = d_acc.cpu().numpy(); fin = d_final.cpu().numpy().view(abi.TRAJ_REC_DTYPE)
    conflict = bb.debug_conflicts(0)
    want = []
    for a in range(N):
        ent = helpers.ent_inputs(sc, a, recs=fresh, t0=float(sc["guesses"][a]["t_start"]), init=inits[a])
        want.append(oracle.entangle_check_pwp(p, a + 1, p.tether_length, np.array(fresh[a]["pwp"]["coeff"])[0, 0], np.array(fresh[a]["pwp"]["coeff"])[1, 0], ent))
    accept = []
    for a in range(N):
        bad = want[a] or any(accept[j] and (conflict[a, j] or conflict[j, a]) for j in range(a))
        accept.append(0 if bad else 1)
    np.testing.assert_array_equal(acc, accept)
    for a in range(N):
        assert fin[a].tobytes() == (fresh[a] if accept[a] else sc["committed"][a]).tobytes()
    bb.close()


# ---- the safety resolve ----

@pytest.mark.parametrize("N", [33, 257])
def test_safety_resolve_at_two_and_nine_row_words(be, oracle, N):
    """one scene: conflict matrix, accept flags and every byte of the final records against the oracle's matrix and the host rule of
    safety_cases.py (resolve), as test_gpu_safety_sizes.py compares them"""
    import safety_cases as SC
    par, prev, _ = SC.fleet_records("default", N, 21)
    fresh = SC.perturbed(par, prev, 21)
    C, accept = oracle.safety_resolve(fresh, 0.0, par.T_span, par.drone_radius)
    np.testing.assert_array_equal(accept, SC.resolve(C, None, np.ones(N, dtype=np.int32)))
    assert 0 < accept.sum() < N
    bb = be.BatchBackend(par, [], n_scenes=1)
    T = bb.torch
    gue = np.zeros(N, dtype=abi.GUESS_DTYPE); gue["K"] = par.num_pol
    d_prev = bb.to_device(prev)
    d_fin = T.full_like(d_prev, 0x5A); d_acc = T.full((N,), -7, dtype=T.int32, device=bb.device)
    bb.safety_commit(d_prev, bb.to_device(fresh), bb.to_device(gue), d_fin, d_acc)
    bb.check()
    np.testing.assert_array_equal(bb.debug_conflicts(0), C)
    np.testing.assert_array_equal(d_acc.cpu().numpy(), accept)
    fin = d_fin.cpu().numpy().view(abi.TRAJ_REC_DTYPE)
    want = prev.copy(); want[accept == 1] = fresh[accept == 1]
    assert fin.tobytes() == np.ascontiguousarray(want).tobytes()
    bb.close()


# ---- the flight audit and the mission controller ----

@pytest.mark.parametrize("with_statics", [False, True])
def test_audit_with_five_agents(be, with_statics):
    """N = 5 (odd: the int arrays behind the agents' doubles), S = 0 and S = 3, against audit_host as test_gpu_flight_audit.py does"""
    from audit_util import HAND_T0, HAND_TICK, hand_scene
    from test_gpu_flight_audit import device_equals_host, hand_par
    recs, statics, radius = hand_scene()
    recs = recs[:5]; statics = list(statics)[:3] if with_statics else []
    assert len(statics) == (3 if with_statics else 0)
    import torch
    device_equals_host(torch, hand_par(5, len(statics), radius), recs[None], [statics], [HAND_T0], HAND_TICK, (10,))


@pytest.mark.parametrize("n_poly", [0, abi.NEP_MISSION_MAX_POLY])
def test_mission_kernel_without_and_with_every_keepout_polygon(be, n_poly):
    """one scene, five agents, no keep-out polygon and NEP_MISSION_MAX_POLY of them (3 .. 8 vertices each: up to NEP_MISSION_MAX_VERT):
    the state after every call equals mission_host's, as test_gpu_fleet_mission.py::test_kernel_alone_equals_host_chain compares it"""
    import mission_ref as mr
    from test_gpu_fleet_mission import Alone
    keep = mr.random_keepouts(np.random.default_rng(5), 1, n_poly) if n_poly else None
    cfg = mr.make_cfg(abi.NEP_MISSION_PER_AGENT, max_goals=3, log_cap=4, min_interval=0.5, timeout=2.0)
    import torch
    a = Alone(torch, cfg, 1, 5, 5, keep=keep, seed=9)
    try:
        for _ in range(12):
            a.call()
        if n_poly == 0:      # (with 64 polygons a draw may end without a goal: the flag that raises is the host's verdict too, compared in call())
            a.be.check()
    finally:
        a.close()
