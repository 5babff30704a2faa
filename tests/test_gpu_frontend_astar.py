"""The reference's best-first search on the device (nep_batch_frontend_astar) against oracle.frontend_astar on the
hulls of oracle.hulls_of_scene: the whole nep_guess byte for byte, every named field of nep_fe_result with ==.  The oracle's own
outcomes are asserted next to every comparison, so that a test cannot pass by covering nothing."""
import functools

import numpy as np
import pytest

from neptune_amd import abi, scene

pytestmark = pytest.mark.gpu

EMPTY, GOAL, BUDGET, NO_SOLUTION, SKIPPED = 2, 1, 0, 3, 4      # NEP_FE_EMPTY, _GOAL_REACHED, _DEPTH_REACHED, _NO_SOLUTION, _SKIPPED
PAD_POOL = 16                                                  # nep_fe_result._pad bit 4


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


@functools.lru_cache(maxsize=None)
def _scene(n_agents, n_static, seed):
    return scene.make_scene(n_agents, n_static, seed=seed)


def _fe(p, num_samples=5, pad_hold=0, cable=None):
    fe = scene.frontend_cfg(p, num_samples=num_samples, pad_hold=pad_hold)
    if cable is not None:
        fe.cable_length = cable
    return fe


_ORACLE = {}


def _want(oracle, key, sc, fe, max_pops, order=None, agents=None, starts=None, com=None):
    """oracle.frontend_astar for the agents of a scene -> {agent: (guess record, result dict)}; computed once per key, never changed"""
    if key not in _ORACLE:
        p = sc["par"]
        starts = scene.frontend_starts(sc) if starts is None else starts
        com = sc["committed"] if com is None else com
        out = {}
        for a in (range(p.num_agents) if agents is None else agents):
            hx, hn = oracle.hulls_of_scene(p, a + 1, com, float(starts[a]["t_start"]), sc["statics"])
            out[a] = oracle.frontend_astar(p, fe, a + 1, starts[a], hx, hn, sc["statics"], order=order, max_pops=max_pops)
        _ORACLE[key] = out
    return _ORACLE[key]


def _run(bb, fe, com, starts, n_slots):
    d_guess = bb.torch.full((n_slots * abi.GUESS_DTYPE.itemsize,), 0xAB, dtype=bb.torch.uint8, device=bb.device)      # (stale bytes: every byte must be written)
    d_res = bb.torch.full((n_slots * abi.FE_RESULT_DTYPE.itemsize,), 0xAB, dtype=bb.torch.uint8, device=bb.device)
    bb.frontend_astar(fe, bb.to_device(com), bb.to_device(np.ascontiguousarray(starts)), d_guess, d_res)
    bb.torch.cuda.synchronize()
    return d_guess.cpu().numpy().view(abi.GUESS_DTYPE), d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE)


def _same(got_g, got_r, want, where):
    g, r = want
    for f in abi.FE_RESULT_DTYPE.names:
        assert got_r[f].item() == r[f], (where, f, got_r[f].item(), r[f])
    assert got_g.tobytes() == np.asarray(g).tobytes(), (where, "guess bytes", int(got_g["K"]), int(g["K"]))


def _device(be, sc, fe, max_pops, order=None, max_nodes=0):
    p = sc["par"]
    bb = be.BatchBackend(p, sc["statics"])
    bb.set_fe_astar(max_pops, max_nodes, order)
    got = _run(bb, fe, sc["committed"], scene.frontend_starts(sc), p.num_agents)
    return bb, got


def _col(want, f):
    return [want[a][1][f] for a in sorted(want)]


@pytest.mark.parametrize("max_pops", [1, 40, 300, 2000])
def test_budgets(be, oracle, max_pops):
    """Test 1: the pop budget, from one pop to a search that reaches the goal after 977; depths beyond num_pol, occupied goals."""
    sc = _scene(8, 6, 5); p = sc["par"]; fe = _fe(p)
    want = _want(oracle, ("budget", max_pops), sc, fe, max_pops)
    if max_pops == 300:
        assert _col(want, "status") == [1, 0, 1, 0, 0, 1, 1, 1] and _col(want, "K") == [8, 1, 4, 1, 1, 8, 7, 8]
        assert _col(want, "depth") == [26, 1, 4, 1, 1, 21, 7, 19]
        assert [a for a in range(8) if want[a][1]["goal_occupied"]] == [1, 3]
    if max_pops == 2000:
        assert want[1][1]["status"] == GOAL and want[1][1]["n_children"] == 977
        assert (want[3][1]["status"], want[3][1]["K"], want[3][1]["depth"]) == (BUDGET, 8, 24)
        assert (want[4][1]["status"], want[4][1]["K"]) == (BUDGET, 1)
    assert all(r["n_children"] <= max_pops for _, r in want.values())
    bb, (got_g, got_r) = _device(be, sc, fe, max_pops)
    for a in range(8):
        _same(got_g[a], got_r[a], want[a], ("agent", a))
    bb.check()
    bb.close()


@pytest.mark.parametrize("case", ["5x0", "16x8", "ns3", "ns4", "order"])
def test_other_shapes(be, oracle, case):
    """Test 2: a scene without statics, one with twice the agents, the 3 x 3 and 4 x 4 lattices, and a shuffled lattice order
    (which changes the outcome: the point of the parameter)."""
    order = None; ns = 5
    sc = _scene(8, 6, 5)
    if case == "5x0":
        sc = _scene(5, 0, 3)
    elif case == "16x8":
        sc = _scene(16, 8, 4)
    elif case == "ns3":
        ns = 3
    elif case == "ns4":
        ns = 4
    else:
        order = np.random.default_rng(4).permutation(25).astype(np.int32)
    p = sc["par"]; fe = _fe(p, num_samples=ns)
    want = _want(oracle, ("shape", case), sc, fe, 300, order=order)
    if case == "order":
        assert _col(want, "status") == [1, 0, 1, 0, 1, 1, 1, 1]
        assert _col(want, "status") != _col(_want(oracle, ("budget", 300), sc, _fe(p), 300), "status")
    assert any(r["n_children"] > 1 for _, r in want.values()) and any(r["K"] >= 1 for _, r in want.values())
    bb, (got_g, got_r) = _device(be, sc, fe, 300, order=order)
    for a in range(p.num_agents):
        _same(got_g[a], got_r[a], want[a], (case, "agent", a))
    bb.check()
    bb.close()


@pytest.mark.parametrize("cable", [3.0, 1.0])
def test_empty_and_no_solution(be, oracle, cable):
    """Test 3: a short tether exhausts the open list (NEP_FE_EMPTY: every created node popped) or leaves no first primitive
    (NEP_FE_NO_SOLUTION, K = 0)."""
    sc = _scene(8, 6, 5); p = sc["par"]; fe = _fe(p, cable=cable)
    want = _want(oracle, ("cable", cable), sc, fe, 3000)
    if cable == 3.0:
        assert _col(want, "status") == [2, 2, 3, 2, 2, 2, 2, 2] and _col(want, "K") == [1, 1, 0, 1, 1, 1, 8, 1]
        assert max(_col(want, "n_children")) <= 579
        assert all(r["n_children"] == r["n_feasible"] for _, r in want.values() if r["status"] == EMPTY)
    else:
        assert _col(want, "status") == [NO_SOLUTION] * 8 and _col(want, "K") == [0] * 8
    bb, (got_g, got_r) = _device(be, sc, fe, 3000)
    for a in range(8):
        _same(got_g[a], got_r[a], want[a], (cable, "agent", a))
    bb.close()


def test_deep_heap(be, oracle):
    """Test 4: twelve thousand nodes in one open list (the heap beyond its LDS part, the full-size pool and table), on a 2-agent shard."""
    sc = _scene(8, 6, 5); p = sc["par"]; fe = _fe(p)
    want = _want(oracle, ("deep",), sc, fe, 20000, agents=(3, 4))
    r3, r4 = want[3][1], want[4][1]
    assert (r3["status"], r3["n_children"], r3["n_feasible"], r3["K"], r3["depth"]) == (EMPTY, 11969, 11969, 8, 24)
    assert (r4["status"], r4["n_children"], r4["n_feasible"], r4["depth"]) == (GOAL, 4703, 5102, 35)
    bb = be.BatchBackend(p, sc["statics"], first_local=3, n_local=2)
    bb.set_fe_astar(20000)
    got_g, got_r = _run(bb, fe, sc["committed"], scene.frontend_starts(sc)[3:5], 2)
    for al, a in enumerate((3, 4)):
        _same(got_g[al], got_r[al], want[a], ("agent", a))
    bb.check()
    bb.close()


def test_multi_scene_and_agent_shard(be, oracle):
    """Test 5: several scenes per launch on their own clocks, agent shards, random height states (slot -> (scene, agent) bookkeeping)."""
    from neptune_amd import dist as ndist
    S, N = 3, 6
    scenes = [dict(scene.make_scene(N, 5, seed=80 + s)) for s in range(S)]
    for k, sc in enumerate(scenes):
        sc["statics"] = scenes[0]["statics"]
        sc["guesses"] = sc["guesses"].copy(); sc["committed"] = sc["committed"].copy()
        sc["guesses"]["t_start"] += 0.35 * k
        sc["committed"]["pwp"]["times"] += 0.35 * k
    p = scenes[0]["par"]
    com, _ = ndist.stack_scenes(scenes)
    fe = _fe(p)
    starts = np.stack([scene.frontend_starts(sc) for sc in scenes])
    rng = np.random.default_rng(8)
    starts["pos"][:, :, 2] = rng.uniform(0.5, 3.0, size=(S, N)); starts["vel"][:, :, 2] = rng.normal(scale=1.5, size=(S, N))
    starts["accel"][:, :, 2] = rng.normal(scale=2.5, size=(S, N)); starts["goal"][:, :, 2] = rng.uniform(0.5, 4.5, size=(S, N))
    want = [_want(oracle, ("multi", s_), scenes[s_], fe, 200, starts=starts[s_], com=com[s_]) for s_ in range(S)]
    assert len({r["status"] for w in want for _, r in w.values()}) >= 2 and any(r["K"] >= 3 for w in want for _, r in w.values())
    for first, nl in ((0, 6), (2, 2), (3, 3)):
        bb = be.BatchBackend(p, scenes[0]["statics"], first_local=first, n_local=nl, n_scenes=S)
        bb.set_fe_astar(200)
        got_g, got_r = _run(bb, fe, com, starts[:, first:first + nl], S * nl)
        got_g = got_g.reshape(S, nl); got_r = got_r.reshape(S, nl)
        for s_ in range(S):
            for al in range(nl):
                _same(got_g[s_, al], got_r[s_, al], want[s_][first + al], (first, s_, first + al))
        bb.close()


def test_active_set(be, oracle):
    """Test 6: an inactive slot gets exactly what the beam front end's launch gives it; active slots the oracle's search."""
    sc = _scene(8, 6, 5); p = sc["par"]; fe = _fe(p)
    want = _want(oracle, ("budget", 300), sc, fe, 300)
    bb = be.BatchBackend(p, sc["statics"])
    bb.set_fe_astar(300)
    torch = bb.torch
    on = [1, 0, 1, 1, 0, 0, 1, 0]
    mask = torch.tensor([on], dtype=torch.int32, device=bb.device)
    bb.set_active(mask)
    starts = scene.frontend_starts(sc)
    got_g, got_r = _run(bb, fe, sc["committed"], starts, 8)
    d_guess = torch.full((8 * abi.GUESS_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=bb.device)
    d_res = torch.full((8 * abi.FE_RESULT_DTYPE.itemsize,), 0xAB, dtype=torch.uint8, device=bb.device)
    bb.frontend(fe, bb.to_device(sc["committed"]), bb.to_device(starts), d_guess, d_res)
    torch.cuda.synchronize()
    beam_g = d_guess.cpu().numpy().view(abi.GUESS_DTYPE); beam_r = d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE)
    for a in range(8):
        if on[a]:
            _same(got_g[a], got_r[a], want[a], ("agent", a))
        else:
            assert int(got_r[a]["status"]) == SKIPPED
            assert got_g[a].tobytes() == beam_g[a].tobytes() and got_r[a].tobytes() == beam_r[a].tobytes(), a
    bb.set_active(None)
    got_g, got_r = _run(bb, fe, sc["committed"], starts, 8)
    for a in range(8):
        _same(got_g[a], got_r[a], want[a], ("all on again", a))
    bb.close()


def test_pool_budget(be, oracle):
    """Test 7: a 64-node pool.  A search that never holds 63 nodes is the oracle's; one that gets there stops creating nodes, says
    so (bit 4 of _pad, NEP_E_CAP from the check) and still returns a plan from A; nothing leaks into the neighbours' pools."""
    from neptune_amd._lib import BackendError
    sc = _scene(8, 6, 5); p = sc["par"]; fe = _fe(p)
    want = _want(oracle, ("budget", 300), sc, fe, 300)
    fits = [a for a in range(8) if want[a][1]["n_feasible"] < 63]
    assert want[6][1]["n_feasible"] == 49 and 6 in fits and len(fits) < 8
    assert all(want[a][1]["n_feasible"] > 63 for a in range(8) if a not in fits)      # (nobody sits on the boundary itself)
    bb, (got_g, got_r) = _device(be, sc, fe, 300, max_nodes=64)
    starts = scene.frontend_starts(sc)
    for a in range(8):
        if a in fits:
            _same(got_g[a], got_r[a], want[a], ("agent", a))
        else:
            assert int(got_r[a]["_pad"]) & PAD_POOL and int(got_r[a]["n_feasible"]) == 63 and int(got_r[a]["K"]) >= 1, (a, got_r[a])
            assert int(got_g[a]["K"]) == int(got_r[a]["K"])
            np.testing.assert_array_equal(np.array(got_g[a]["coeff"])[:2, 0, 3], starts[a]["pos"][:2])
    with pytest.raises(BackendError, match="error -4"):
        bb.check()
    bb.check()                                                                        # (the flag is reported once)
    bb2, (g2, r2) = _device(be, sc, fe, 300)
    for a in range(8):
        _same(g2[a], r2[a], want[a], ("default pool", a))
    bb2.check()
    bb2.close(); bb.close()


def test_capture(be, oracle):
    """Test 8: after the setter the call allocates nothing: captured and replayed twice it writes the eager call's bytes."""
    sc = _scene(8, 6, 5); p = sc["par"]; fe = _fe(p)
    want = _want(oracle, ("budget", 300), sc, fe, 300)
    bb = be.BatchBackend(p, sc["statics"])
    bb.set_fe_astar(300)
    torch = bb.torch
    d_com = bb.to_device(sc["committed"]); d_start = bb.to_device(scene.frontend_starts(sc))
    d_guess = torch.zeros(8 * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=bb.device)
    d_res = torch.zeros(8 * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=bb.device)
    bb.frontend_astar(fe, d_com, d_start, d_guess, d_res)
    torch.cuda.synchronize()
    eager = (d_guess.cpu().numpy().tobytes(), d_res.cpu().numpy().tobytes())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        bb.frontend_astar(fe, d_com, d_start, d_guess, d_res)
    for _ in range(2):
        d_guess.fill_(0xAB); d_res.fill_(0xAB)
        gr.replay()
        torch.cuda.synchronize()
        assert (d_guess.cpu().numpy().tobytes(), d_res.cpu().numpy().tobytes()) == eager
    got_g = d_guess.cpu().numpy().view(abi.GUESS_DTYPE); got_r = d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE)
    for a in range(8):
        _same(got_g[a], got_r[a], want[a], ("agent", a))
    del gr
    bb.close()


def test_pad_hold(be, oracle):
    """Test 9: pad_hold = 1 extends a plan shorter than num_pol with segments that hold the returned node's end point (the
    oracle's A* ignores pad_hold: its K segments are the device's first K)."""
    sc = _scene(8, 6, 5); p = sc["par"]; D = p.num_pol
    want = _want(oracle, ("budget", 300), sc, _fe(p), 300)
    assert want[2][1]["K"] == 4 and any(0 < r["K"] < D for _, r in want.values())
    bb, (got_g, got_r) = _device(be, sc, _fe(p, pad_hold=1), 300)
    T = p.T_span
    for a in range(8):
        g, r = want[a]
        K = r["K"]
        for f in abi.FE_RESULT_DTYPE.names:
            if f != "K":
                assert got_r[a][f].item() == r[f], (a, f)
        co = np.array(got_g[a]["coeff"]); ref = np.array(g["coeff"])
        if K == 0:
            assert int(got_g[a]["K"]) == 0 and int(got_r[a]["K"]) == 0 and not co.any()
            continue
        assert int(got_g[a]["K"]) == D and int(got_r[a]["K"]) == D, a
        np.testing.assert_array_equal(co[:2, :K], ref[:2, :K])
        for ax in range(2):
            e = co[ax, K:, 3]
            np.testing.assert_array_equal(co[ax, K:, :3], 0.0)
            assert np.all(np.abs(e - np.polyval(co[ax, K - 1], T)) <= 1e-12), (a, ax)
        assert float(got_g[a]["t_start"]) == float(g["t_start"])
    bb.close()


def test_loops(be):
    """Test 10: the fleet loops with search="astar": DeviceFleetLoop on one scene flies FleetLoop's flight (every replan's outcome, K
    and statuses, the counters), its captured rounds fly its eager ones, and the audit's invariants hold.  How many agents arrive
    within the rounds is not asserted: on its budget the reference's rule returns the node nearest the start."""
    from neptune_amd.loop import DeviceFleetLoop, FleetLoop
    sc = _scene(16, 8, 1)
    with pytest.raises(ValueError):
        FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), search="astar", tethers=True)
    with pytest.raises(ValueError):
        DeviceFleetLoop([sc], search="astar", tethers=True)
    ref = FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), audit=True, search="astar", max_pops=300)
    ref.trace = []
    st = ref.run(max_rounds=40)
    ref.close()
    flown = []
    for graph in (False, True):
        loop = DeviceFleetLoop([sc], audit=True, trace=True, graph=graph, search="astar", max_pops=300)
        rep = loop.run(max_rounds=40)[0]
        loop.be.check()
        assert (loop._g is not None) == graph
        trace, t = [], 0.0
        for row in loop.trace:
            for a, (oc, K, fe, qp) in enumerate(row):
                if oc != abi.NEP_FLEET_SKIPPED:
                    trace.append((t, a, abi.FLEET_OUTCOMES[oc], K, fe, qp))
            for _ in range(loop.replan_every):
                t += loop.p.dc
        flown.append((trace, rep, loop.audit_records()[0].tobytes()))
        loop.close()
    trace, rep, _ = flown[1]
    first = next((k for k, (x, y) in enumerate(zip(trace, ref.trace)) if x != y), None)
    assert first is None, ("traces part at entry", first, trace[first], ref.trace[first])
    assert len(trace) == len(ref.trace) and len(trace) > 16
    assert any(e[4] == BUDGET for e in trace) and any(e[4] == GOAL for e in trace)      # (both kinds of search were flown)
    assert rep["rounds"] == st["rounds"] and rep["reached"] == st["reached"]
    for k in ("replans", "accepted", "fe_no_solution", "qp_failed", "rejected_by_safety", "qp_relaxed", "solves"):
        assert rep[k] == st[k], (k, rep[k], st[k])
    assert flown[0] == flown[1]                                                         # captured == eager: trace, report, audit bytes
    print("astar flight, 40 rounds at 300 pops: reached %d of 16, accepted %d of %d replans, min_box_clear %r min_static_dist %r"
          % (rep["reached"], rep["accepted"], rep["replans"], rep["audit"]["min_box_clear"], rep["audit"]["min_static_dist"]))
    assert rep["audit"]["min_box_clear"]["value"] >= -1e-6, rep["audit"]
    assert rep["audit"]["min_static_dist"]["value"] >= -1e-6 and rep["audit"]["n_static_viol"] == 0, rep["audit"]


def test_contract(be):
    """Test 11: the argument and state checks of the two entry points."""
    from neptune_amd._lib import BackendError
    sc = _scene(8, 6, 5); p = sc["par"]
    bb = be.BatchBackend(p, sc["statics"])
    d_com = bb.to_device(sc["committed"]); d_start = bb.to_device(scene.frontend_starts(sc))
    d_guess = bb.torch.zeros(8 * abi.GUESS_DTYPE.itemsize, dtype=bb.torch.uint8, device=bb.device)
    with pytest.raises(BackendError, match="error -2"):                               # NEP_E_STATE: before the setter
        bb.frontend_astar(_fe(p), d_com, d_start, d_guess)
    with pytest.raises(BackendError, match="error -1"):                               # NEP_E_ARG: not a permutation
        bb.set_fe_astar(100, 0, [0] + list(range(24)))
    with pytest.raises(BackendError, match="error -1"):                               # ... not a lattice's size
        bb.set_fe_astar(100, 0, list(range(24)))
    with pytest.raises(BackendError, match="error -2"):                               # a refused setter sets nothing
        bb.frontend_astar(_fe(p), d_com, d_start, d_guess)
    bb.set_fe_astar(100, 0, list(range(25)))
    fe = scene.frontend_cfg(p, entangle=True)
    with pytest.raises(BackendError, match="error -1"):                               # enable_entangle
        bb.frontend_astar(fe, d_com, d_start, d_guess)
    with pytest.raises(BackendError, match="error -1"):                               # num_samples^2 != n_order
        bb.frontend_astar(_fe(p, num_samples=4), d_com, d_start, d_guess)
    bb.frontend_astar(_fe(p), d_com, d_start, d_guess)
    bb.check()
    bb.close()
