"""Shared by the GPU parity test files: tolerances, the per-agent solver set up the way the reference sets it up, and the scene
checker (every replan of a scene against the oracle)."""
import numpy as np

from neptune_amd import abi, scene

COEF_TOL = 1e-6
COST_RTOL = 1e-6


def _bounds(p):
    return (p.x_min, p.x_max, p.y_min, p.y_max, p.z_min, p.z_max, p.v_max, p.a_max, p.j_max)


def _solver(be, p, agent_id=1):
    s = be.PolySolver(p.num_pol, 3, agent_id, p.T_span, p.pb, p.weight, 0.5, True)
    s.setMaxValues(*_bounds(p)); s.setMaxRuntime(0.05); s.setTetherLength(p.tether_length)
    return s


def lines_match(bb, seg, nd, r):
    """the lines a handle holds for one replan (debug_lines) against the oracle's (r = oracle.replan(...)): with every row through the
    interior point (line presolve off) the same lines bit for bit in the reference's call order; under the presolve (the default) the
    buckets hold the near lines first, then the parked ones, and LPs skipped by the box test made no line at all — every line present
    must be one of the oracle's, bit for bit, in the same segment"""
    if bb.line_cull() == 0.0:
        np.testing.assert_array_equal(seg, r["line_seg"])
        np.testing.assert_array_equal(nd, r["line_nd"])
        return
    want = {(int(s_), l.tobytes()) for s_, l in zip(r["line_seg"], r["line_nd"])}
    assert all((int(s_), np.ascontiguousarray(l).tobytes()) in want for s_, l in zip(seg, nd))


def solver_lines_match(s, r, ordered=False):
    """the per-agent handle's lines of the last optimize() (debugGetLines) against the oracle's: it never skips an LP (its hull lists
    are the caller's), so the same lines bit for bit — in the reference's call order with the presolve off (ordered=True after
    setLineCull(0)), as a multiset under the default presolve (near lines first, parked ones after)"""
    seg, nd = s.debugGetLines()
    if ordered:
        np.testing.assert_array_equal(seg, r["line_seg"]); np.testing.assert_array_equal(nd, r["line_nd"])
        return
    got = sorted((int(a), np.ascontiguousarray(l).tobytes()) for a, l in zip(seg, nd))
    want = sorted((int(a), np.ascontiguousarray(l).tobytes()) for a, l in zip(r["line_seg"], r["line_nd"]))
    assert got == want


def check_slot_outputs(oracle, p, own, guess, sol, states, com, prev=None):
    """What a replan leaves behind for ONE slot — the sampled states and the published record — against the slot's own nep_solution,
    which is taken as the truth for the trajectory.  own: the agent's global index; guess: the nep_guess the slot was given; sol, states
    [max_states][12], com: the slot's entries of solutions(), states(), commits(); prev: the record of (scene, own) handed to the replan
    as d_committed, or None when none was.  A slot that solved publishes its trajectory; a failed or skipped one keeps the previous
    record, byte for byte (without previous records its commit slot is left as passed: nothing to check here)."""
    status, K = int(sol["stats"]["status"]), int(sol["K"])
    if status == abi.NEP_SKIPPED:                          # nothing solved: the solution is zero apart from the status
        z = sol.copy(); z["stats"]["status"] = 0
        assert not np.frombuffer(z.tobytes(), dtype=np.uint8).any(), own
    else:
        co = np.array(sol["coeff"])[:, :K, :]
        assert not np.array(sol["coeff"])[:, K:, :].any() and not np.array(sol["times"])[K + 1:].any(), own
        t0 = float(guess["t_start"])
        if K > 0:
            np.testing.assert_allclose(np.array(sol["times"])[:K + 1], t0 + np.arange(K + 1) * p.T_span, atol=1e-12)
            ref = oracle.sample(co, p.T_span, p.dc, cap=4096)      # the whole schedule of K
            n = min(len(ref), p.max_states)
        else:
            ref, n = np.zeros((0, abi.NEP_STATE_DOUBLES)), 0
        assert int(sol["n_states"]) == n, (own, int(sol["n_states"]), len(ref), p.max_states)
        np.testing.assert_allclose(states[:n], ref[:n], rtol=0, atol=1e-12)
    if status in (abi.NEP_FAILED, abi.NEP_SKIPPED):
        if prev is not None:
            assert com.tobytes() == prev.tobytes(), (own, status)
        return
    assert int(com["id"]) == own + 1 and int(com["is_agent"]) == 1 and int(com["n_bend"]) == 1 and int(com["valid"]) == 1, own
    np.testing.assert_array_equal(com["bbox"], np.full(3, 2 * p.drone_radius))
    np.testing.assert_array_equal(com["pos"], co[:, 0, 3])
    np.testing.assert_array_equal(com["bend"][0], np.asarray(p.pb)[own])
    assert int(com["pwp"]["n_seg"]) == K
    rt = np.array(com["pwp"]["times"])
    np.testing.assert_array_equal(rt[:K + 1], np.array(sol["times"])[:K + 1])      # (= t_start + i T: the solution's, checked above)
    assert not rt[K + 1:].any()
    rc = np.array(com["pwp"]["coeff"])
    assert rc.shape == (3, abi.NEP_TRAJ_MAX_SEG, 4)
    assert rc[:, :K, :].tobytes() == co.tobytes()                                   # bit-equal to the solution's
    assert not rc[:, K:, :].any()


def _check_scene(be, oracle, sc, n_scenes=1, first_local=0, n_local=None, hull_kernel=0, replans=1, info=None):
    """Every replan of a scene against the oracle, on BOTH solve paths of the handle: `full` = every separating-line row through the
    interior point (nep_batch_set_line_cull(0): lines bit-exact in the reference's call order, LP / row counts), and the handle's
    default = the verified line presolve with the polish pass under it (statuses, coefficients, cost, samples, commit records to the
    same tolerances; its line buckets hold the near lines first and never-made lines are absent, so lines are checked as a subset).
    hull_kernel: nep_batch_set_hull_kernel on both handles; replans: the replan is enqueued that many times on the same handle and the
    last one is checked (what a handle does from its second round on); info: a dict that receives what the caller asserts on top —
    the oracle's results per agent id (`refs`), per mode the worst coefficient error (`worst`), the launch path (`path`) and the
    presolve's redo count (`redo`)."""
    p = sc["par"]
    worst = 0.0
    refs = {}
    for mode in ("full", "default"):
        bb = be.BatchBackend(p, sc["statics"], first_local=first_local, n_local=n_local)
        if mode == "full":
            bb.set_line_cull(0.0)
        else:
            assert bb.line_cull() == 4.0          # the default at every size (round 6)
        if hull_kernel:
            bb.set_hull_kernel(hull_kernel)
        nl = bb.n_local
        d_comm = bb.to_device(sc["committed"]); d_guess = bb.to_device(sc["guesses"][first_local:first_local + nl])
        for _ in range(replans):
            bb.replan(d_comm, d_guess)
        worst_mode = 0.0
        sol = bb.solutions(); states = bb.states(); com = bb.commits()
        hx, hn = bb.debug_hulls(0)
        for a in range(nl):
            aid = first_local + a + 1
            if aid not in refs:
                refs[aid] = oracle.replan(p, aid, sc["committed"], sc["guesses"][aid - 1], sc["statics"], want_hulls=True)
            r = refs[aid]
            K = int(sol[a]["K"])
            st = sol[a]["stats"]
            seg, nd = bb.debug_lines(a)
            if mode == "full":
                # hulls: oracle lists the present agents in id order (own skipped)
                others = [j for j in range(p.num_agents) if j != aid - 1]
                for oj, j in enumerate(others):
                    for i in range(p.num_pol):
                        nv = r["hull_nv"][oj * p.num_pol + i]
                        assert hn[j, i] == nv
                        np.testing.assert_array_equal(hx[j, i, :nv], r["hull_xy"][oj * p.num_pol + i, :nv])
                np.testing.assert_array_equal(seg, r["line_seg"])
                np.testing.assert_array_equal(nd, r["line_nd"])                 # bit-exact lines, reference loop order
                assert int(st["n_rows"]) == r["n_rows"]
            else:
                # every line the presolved handle holds is one of the oracle's, bit for bit, in the same segment
                want = {(int(s_), l.tobytes()) for s_, l in zip(r["line_seg"], r["line_nd"])}
                assert all((int(s_), l.tobytes()) in want for s_, l in zip(seg, nd)), aid
                assert int(st["n_rows"]) <= r["n_rows"]
            assert int(st["status"]) == r["status"] and int(st["n_lines"]) == r["n_lines"], (mode, aid)
            assert int(st["n_lp"]) == r["n_lp"] and int(st["n_lp_failed"]) == r["n_lp_failed"], (mode, aid)
            co = np.array(sol[a]["coeff"])[:, :K, :]
            err = np.abs(co - r["coeff"]).max(); worst = max(worst, err); worst_mode = max(worst_mode, err)
            assert err <= COEF_TOL, (mode, aid, err)
            if r["status"] != 2:
                assert abs(float(st["objective"]) - r["objective"]) <= COST_RTOL * (1 + abs(r["objective"])), (mode, aid)
            check_slot_outputs(oracle, p, aid - 1, sc["guesses"][aid - 1], sol[a], states[a], com[a], prev=sc["committed"][aid - 1])
        if info is not None:
            info.setdefault("worst", {})[mode] = worst_mode
            info.setdefault("path", {})[mode] = bb.debug_launch_path()
            info.setdefault("redo", {})[mode] = bb.redo_count() if mode == "default" else 0
            info["refs"] = refs
        bb.close()
    return worst


def check_replanned_handle(oracle, bb, guesses, committed, refs, mask=None):
    """_check_scene's per-slot rules for ONE handle that the caller prepared (options, scenes' statics, separator pack ...) and
    replanned: guesses, committed [n_scenes][N] as the replan got them, refs [n_scenes][N] the oracle's result per (scene, agent) —
    None where the guess has K = 0: such a slot reports NEP_FAILED with an empty solution, no line, no LP and no row —, mask
    [n_scenes][N] the active set in force (0: the slot is NEP_SKIPPED) or None.  The solve path is the handle's: with line_cull() == 0
    the lines bit for bit in the reference's call order and n_rows equal; otherwise every held line one of the oracle's in the same
    segment, bit for bit, and n_rows <= the oracle's.  Both: n_lines, n_lp, n_lp_failed, status, coefficients <= COEF_TOL, cost <=
    COST_RTOL, check_slot_outputs.  -> the worst coefficient error"""
    p = bb.par
    full = bb.line_cull() == 0.0
    nl = bb.n_local
    sol = bb.solutions(); states = bb.states(); com = bb.commits()
    worst = 0.0
    for s in range(bb.n_scenes):
        for a in range(nl):
            own = bb.first_local + a; slot = s * nl + a
            g = guesses[s][own]; r = refs[s][own]; st = sol[slot]["stats"]; tag = (s, own)
            skipped = mask is not None and not mask[s][own]
            seg, nd = (None, None) if skipped else bb.debug_lines(slot)      # (no separator ran for an inactive slot: its buckets are not a result)
            if skipped:
                assert int(st["status"]) == abi.NEP_SKIPPED, tag
            elif r is None:
                assert int(g["K"]) == 0 and int(st["status"]) == abi.NEP_FAILED and int(sol[slot]["K"]) == 0 and len(seg) == 0, tag
                assert (int(st["n_lines"]), int(st["n_lp"]), int(st["n_lp_failed"]), int(st["n_rows"])) == (0, 0, 0, 0), tag
            else:
                K = int(sol[slot]["K"])
                assert K == int(g["K"]), tag
                if full:
                    np.testing.assert_array_equal(seg, r["line_seg"], err_msg=str(tag))
                    np.testing.assert_array_equal(nd, r["line_nd"], err_msg=str(tag))
                    assert int(st["n_rows"]) == r["n_rows"], tag
                else:
                    want = {(int(s_), l.tobytes()) for s_, l in zip(r["line_seg"], r["line_nd"])}
                    assert all((int(s_), np.ascontiguousarray(l).tobytes()) in want for s_, l in zip(seg, nd)), tag
                    assert int(st["n_rows"]) <= r["n_rows"], tag
                assert int(st["status"]) == r["status"] and int(st["n_lines"]) == r["n_lines"], (tag, int(st["status"]), r["status"], int(st["n_lines"]), r["n_lines"])
                assert int(st["n_lp"]) == r["n_lp"] and int(st["n_lp_failed"]) == r["n_lp_failed"], tag
                err = np.abs(np.array(sol[slot]["coeff"])[:, :K, :] - r["coeff"]).max(); worst = max(worst, err)
                assert err <= COEF_TOL, (tag, err)
                if r["status"] != abi.NEP_FAILED:
                    assert abs(float(st["objective"]) - r["objective"]) <= COST_RTOL * (1 + abs(r["objective"])), tag
            check_slot_outputs(oracle, p, own, g, sol[slot], states[slot], com[slot], prev=committed[s][own])
    return worst


def check_frontend_beam(be, oracle, sc, W, near=(0.9, 0.3)):
    """The front-end kernel against the deterministic beam rule of the oracle: results and guesses (lattice primitives) identical,
    the same with pad_hold on goals `near` the starts (short searches), then the back end on the device-made guesses against the
    oracle.  -> (guesses found, short guesses padded)"""
    p = sc["par"]; N = p.num_agents
    fe = scene.frontend_cfg(p, beam_width=W)
    starts = scene.frontend_starts(sc)
    bb = be.BatchBackend(p, sc["statics"])
    d_com = bb.to_device(sc["committed"])
    d_start = bb.to_device(starts)
    d_guess = bb.torch.zeros(N * abi.GUESS_DTYPE.itemsize, dtype=bb.torch.uint8, device=bb.device)
    d_res = bb.torch.zeros(N * abi.FE_RESULT_DTYPE.itemsize, dtype=bb.torch.uint8, device=bb.device)
    bb.frontend(fe, d_com, d_start, d_guess, d_res)
    bb.torch.cuda.synchronize()
    got_g = d_guess.cpu().numpy().view(abi.GUESS_DTYPE)
    got_r = d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE)
    n_ok = 0
    for a in range(N):
        hx, hn = oracle.hulls_of_scene(p, a + 1, sc["committed"], float(starts[a]["t_start"]), sc["statics"])
        g, r = oracle.frontend_beam(p, fe, a + 1, starts[a], hx, hn, sc["statics"])
        for f in abi.FE_RESULT_DTYPE.names:
            assert got_r[a][f] == r[f], (a, f, got_r[a][f], r[f])
        assert int(got_g[a]["K"]) == int(g["K"]) and got_g[a]["t_start"] == g["t_start"]
        np.testing.assert_array_equal(got_g[a]["coeff"], g["coeff"])
        n_ok += int(g["K"]) > 0
    # pad_hold: short guesses extended with segments holding their end point — same on both sides
    fe_pad = scene.frontend_cfg(p, beam_width=W, pad_hold=1)
    starts_near = starts.copy()
    starts_near["goal"][:, :2] = starts_near["pos"][:, :2] + list(near)          # goals one or two segments away: short searches
    d_g2 = bb.torch.zeros_like(d_guess)
    bb.frontend(fe_pad, d_com, bb.to_device(starts_near), d_g2)
    bb.torch.cuda.synchronize()
    got2 = d_g2.cpu().numpy().view(abi.GUESS_DTYPE)
    n_short = 0
    for a in range(N):
        hx, hn = oracle.hulls_of_scene(p, a + 1, sc["committed"], float(starts[a]["t_start"]), sc["statics"])
        g, r = oracle.frontend_beam(p, fe_pad, a + 1, starts_near[a], hx, hn, sc["statics"])
        assert int(got2[a]["K"]) == int(g["K"])
        np.testing.assert_array_equal(got2[a]["coeff"], g["coeff"])
        if 0 < r["K"] < p.num_pol:
            n_short += 1
            assert int(g["K"]) == p.num_pol and (np.array(g["coeff"])[:2, r["K"]:, :3] == 0).all()
    # the back end on the device-made guesses
    bb.replan(d_com, d_guess)
    sol = bb.solutions()
    for a in range(N):
        K = int(got_g[a]["K"])
        if K == 0:
            continue
        r = oracle.replan(p, a + 1, sc["committed"], got_g[a], sc["statics"])
        assert int(sol[a]["stats"]["status"]) == r["status"], a
        assert np.abs(np.array(sol[a]["coeff"])[:, :K, :] - r["coeff"]).max() <= COEF_TOL
    bb.close()
    return n_ok, n_short


def check_safety_commit(be, oracle, scenes):
    """Conflict matrix (GJK on the new trajectories' hulls), id-ordered resolution and the committed records of two 8-agent scenes,
    bit for bit against the oracle.  Scene 0: agents 6 and 8 fly copies of agent 2's trajectory 0.5 / 0.6 m next to it; scene 1
    untouched.  -> (handle, prev, fresh, d_prev, d_gue, d_final, d_acc, accept [2][8]): the caller closes the handle."""
    p = scenes[0]["par"]
    prev = np.stack([s["committed"] for s in scenes])
    fresh = prev.copy()
    for tgt, dx in ((5, 0.5), (7, -0.6)):
        fresh[0, tgt] = fresh[0, 1]; fresh[0, tgt]["id"] = tgt + 1
        fresh[0, tgt]["pwp"]["coeff"][0, :, 3] += dx
    fresh["pos"][:] += 0.01                                      # make new != prev everywhere
    gue = np.stack([s["guesses"] for s in scenes])
    bb = be.BatchBackend(p, [], n_scenes=2)
    d_prev = bb.to_device(prev); d_new = bb.to_device(fresh); d_gue = bb.to_device(gue)
    d_final = bb.torch.zeros_like(d_prev); d_acc = bb.torch.zeros(2 * 8, dtype=bb.torch.int32, device=bb.device)
    bb.safety_commit(d_prev, d_new, d_gue, d_final, d_acc)
    acc = d_acc.cpu().numpy().reshape(2, 8)
    fin = d_final.cpu().numpy().view(abi.TRAJ_REC_DTYPE).reshape(2, 8)
    for s_ in range(2):
        conflict, accept = oracle.safety_resolve(fresh[s_], 0.0, p.T_span, p.drone_radius)
        np.testing.assert_array_equal(bb.debug_conflicts(s_), conflict)
        np.testing.assert_array_equal(acc[s_], accept)
        for a in range(8):
            want = fresh[s_, a] if accept[a] else prev[s_, a]
            assert fin[s_, a].tobytes() == want.tobytes()
    return bb, prev, fresh, d_prev, d_gue, d_final, d_acc, acc
