"""The reference's best-first search with the entangle check on the device (nep_batch_frontend_astar_ent) against
tests/astar_ent_ref.py: the whole nep_guess byte for byte, every named field of nep_fe_result with ==, the case block.  What pins the ref
is in tests/test_astar_ent_ref_cpu.py.  The ref's own outcomes are asserted next to every comparison, so that a test cannot pass by
covering nothing."""
import numpy as np
import pytest

import astar_ent_cases as cases
from neptune_amd import abi, scene

pytestmark = pytest.mark.gpu

BUDGET, GOAL, EMPTY, NO_SOLUTION, SKIPPED = 0, 1, 2, 3, 4
PAD_POOL = 16
SHUFFLED = np.random.default_rng(4).permutation(25).astype(np.int32)


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


def _handle(be, sc, n_scenes=1):
    bb = be.BatchBackend(sc["par"], sc["statics"], n_scenes=n_scenes)
    reps, longest = scene.static_reps(sc["statics"]) if len(sc["statics"]) else (np.zeros((0, 2, 2)), np.zeros((0, 2)))
    bb.set_static_reps(reps, longest)
    return bb


def _buffers(bb, n_slots, N):
    T = bb.torch
    d_g = T.full((n_slots * abi.GUESS_DTYPE.itemsize,), 0xAB, dtype=T.uint8, device=bb.device)      # (stale bytes: every byte must be written)
    d_r = T.full((n_slots * abi.FE_RESULT_DTYPE.itemsize,), 0xAB, dtype=T.uint8, device=bb.device)
    d_case = T.full((n_slots * abi.NEP_MAX_POL * N,), -7, dtype=T.int32, device=bb.device)
    return d_g, d_r, d_case


def _views(d_g, d_r, d_case, n_slots, N):
    return d_g.cpu().numpy().view(abi.GUESS_DTYPE), d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE), d_case.cpu().numpy().reshape(n_slots, abi.NEP_MAX_POL, N)


def _run(bb, fe, com, starts, inits, n_slots, N):
    d_g, d_r, d_case = _buffers(bb, n_slots, N)
    bb.frontend_astar_ent(fe, bb.to_device(np.ascontiguousarray(com)), bb.to_device(np.ascontiguousarray(starts)), d_g, d_r, d_case,
                          d_ent_init=bb.to_device(np.ascontiguousarray(inits)) if inits is not None else None)
    bb.torch.cuda.synchronize()
    return _views(d_g, d_r, d_case, n_slots, N)


def _same(got, a, want, where):
    got_g, got_r, got_case = got
    g, r, case, _ = want
    for f in abi.FE_RESULT_DTYPE.names:
        assert got_r[a][f].item() == r[f], (where, f, got_r[a][f].item(), r[f])
    assert got_g[a].tobytes() == np.asarray(g).tobytes(), (where, "guess bytes", int(got_g[a]["K"]), int(g["K"]))
    np.testing.assert_array_equal(got_case[a], case, err_msg="case block, %r" % (where,))


def _device(be, name, max_pops=None, order=None, num_samples=5, max_nodes=0):
    sc, inits, pops = cases.setup(name); p = sc["par"]
    bb = _handle(be, sc)
    bb.set_fe_astar(pops if max_pops is None else max_pops, max_nodes, order)
    got = _run(bb, cases.fe_cfg(p, num_samples), sc["committed"], cases.starts_of(name), inits, p.num_agents, p.num_agents)
    return bb, got


def _col(want, f):
    return [want[a][1][f] for a in sorted(want)]


@pytest.mark.parametrize("name", ["bends", "many_bends", "doubly"])
def test_scene_setups(be, oracle, name):
    """Tests 1 and 3: tethers with 2-4 and 5-8 bend points, searches that start with a crossing on the list, and searches that start
    doubly crossed — invalid end points until a crossing is undone, among them slots that end NEP_FE_NO_SOLUTION after the whole budget."""
    want = cases.want(oracle, name)
    N = len(want)
    st = _col(want, "status")
    assert len(set(st)) >= 3 and (name == "doubly" or sum(_col(want, "n_entangled")) > 0), st
    assert sum(c["updates"] for _, _, _, c in want.values()) > 0 and sum(c["iz_shared"] for _, _, _, c in want.values()) > 0
    if name == "bends":
        assert sum(_col(want, "n_entangled")) == 1068 and sum(int((w[2] != 0).sum()) for w in want.values()) > 0
    if name == "doubly":
        assert st == [3, 0, 3, 3, 1, 3, 1, 0] and sum(c["invalid_end_pops"] for _, _, _, c in want.values()) == 624
        assert [want[a][1]["n_children"] for a in (0, 2)] == [300, 300] and [want[a][1]["n_feasible"] for a in (0, 2)] == [419, 462]      # (no valid end point in the whole budget)
    assert all(r["ent_overflow"] == 0 for _, r, _, _ in want.values())
    bb, got = _device(be, name)
    for a in range(N):
        _same(got, a, want[a], (name, "agent", a))
    bb.check()
    bb.close()


@pytest.mark.parametrize("case", ["pops1", "pops40", "order", "ns3"])
def test_budgets_order_and_lattice(be, oracle, case):
    """Test 2: budgets 1 and 40, a shuffled lattice order and the 3 x 3 lattice on (8, 6, 60)."""
    kw = dict(pops1=dict(max_pops=1), pops40=dict(max_pops=40), order=dict(order=SHUFFLED), ns3=dict(num_samples=3))[case]
    want = cases.want(oracle, "plain", **kw)
    assert len(set(_col(want, "status"))) >= 2 and any(r["K"] >= 1 for _, r, _, _ in want.values())
    if case == "pops1":
        assert all(r["n_children"] <= 1 for _, r, _, _ in want.values())
    else:
        assert sum(_col(want, "n_entangled")) > 0
    if case == "order":
        assert _col(want, "n_feasible") != _col(cases.want(oracle, "plain"), "n_feasible")      # (the order changes the search: the point of the parameter)
    bb, got = _device(be, "plain", **kw)
    for a in range(8):
        _same(got, a, want[a], (case, "agent", a))
    bb.check()
    bb.close()


def test_pool_budget(be, oracle):
    """Test 4: a 64-node pool.  A search that gets there stops creating nodes and says so (bit 4 of _pad, NEP_E_CAP from the check); the
    ref with max_nodes=64 agrees on every slot, cut or not; nothing leaks into the neighbours' pools, and the default pool is unaffected."""
    from neptune_amd._lib import BackendError
    want = cases.want(oracle, "plain", max_nodes=64)
    assert _col(want, "_pad") == [16, 16, 16, 0, 16, 0, 0, 16] and _col(want, "n_feasible") == [63, 63, 63, 24, 63, 24, 54, 63]
    assert _col(want, "status") == [1, 2, 2, 3, 2, 3, 2, 2]
    bb, got = _device(be, "plain", max_nodes=64)
    for a in range(8):
        _same(got, a, want[a], ("64 nodes", "agent", a))
    with pytest.raises(BackendError, match="error -4"):
        bb.check()
    bb.check()                                                                        # (the flag is reported once)
    full = cases.want(oracle, "plain")
    bb2, got2 = _device(be, "plain")
    for a in range(8):
        _same(got2, a, full[a], ("default pool", a))
    bb2.check()
    bb2.close(); bb.close()


@pytest.mark.parametrize("n", [41, 44])
def test_fixed_record_overflow(be, oracle, n):
    """Test 5: helpers.bundle_scene.  Agent 7 flies through a bundle of n - 1 tethers.  40 tethers (n = 41) is the smallest bundle in
    which a 150-pop search outgrows the fixed record: children whose list would pass NEP_FE_ENT_CAP entries are dropped, the search goes
    on and returns an 8-segment plan.  With 43 (n = 44) every first step adds more than 32 crossings: every child of the root is dropped,
    no solution.  Both are flagged (ent_overflow, NEP_E_CAP) and equal the ref under the same caps, as do two searches that are not flagged."""
    from neptune_amd._lib import BackendError
    name = "bundle%d" % n
    agents = (7, 0, n // 2)
    want = cases.want(oracle, name, agents=agents)
    r7 = want[7][1]
    assert r7["ent_overflow"] == 1 and all(want[a][1]["ent_overflow"] == 0 for a in agents[1:])
    if n == 41:
        assert (r7["status"], r7["K"], r7["depth"], r7["n_children"], r7["n_feasible"]) == (BUDGET, 8, 13, 150, 670)
        assert want[7][3]["max_list"] == abi.NEP_FE_ENT_CAP and int((want[7][2] != 0).sum()) == 110
    else:
        assert (r7["status"], r7["K"], r7["n_feasible"]) == (NO_SOLUTION, 0, 0)
    bb, got = _device(be, name)
    for a in agents:
        _same(got, a, want[a], (name, "agent", a))
    assert int(got[1][7]["ent_overflow"]) == 1 and int(got[1][7]["_pad"]) == 0      # (a flag of its own, not the pool's bit)
    with pytest.raises(BackendError, match="error -4"):
        bb.check()
    bb.check()
    bb.close()


def test_three_scenes_and_an_active_set(be, oracle):
    """Test 6: three scenes in one launch on their own clocks; then an active set: an inactive slot gets exactly the bytes
    nep_batch_frontend_ent gives it (its case rows are not written by either), active slots the ref's search."""
    S, N = 3, 8
    sets = [cases.setup("multi%d" % k) for k in range(S)]
    want = [cases.want(oracle, "multi%d" % k) for k in range(S)]
    assert len({r["status"] for w in want for _, r, _, _ in w.values()}) >= 3 and any(r["K"] >= 5 for w in want for _, r, _, _ in w.values())
    sc0 = sets[0][0]; p = sc0["par"]
    com = np.stack([s[0]["committed"] for s in sets]); starts = np.stack([cases.starts_of("multi%d" % k) for k in range(S)])
    inits = np.stack([s[1] for s in sets])
    bb = _handle(be, sc0, n_scenes=S)
    bb.set_fe_astar(sets[0][2])
    fe = cases.fe_cfg(p)
    got = _run(bb, fe, com, starts, inits, S * N, N)
    for k in range(S):
        for a in range(N):
            _same(got, k * N + a, want[k][a], ("scene", k, "agent", a))
    T = bb.torch
    on = np.array([[1, 0, 1, 1, 0, 0, 1, 0], [0, 1, 1, 0, 1, 1, 0, 1], [1, 1, 0, 0, 0, 1, 1, 1]], dtype=np.int32)
    bb.set_active(T.from_numpy(on).to(bb.device))
    got = _run(bb, fe, com, starts, inits, S * N, N)
    d_g, d_r, d_case = _buffers(bb, S * N, N)
    bb.frontend_ent(fe, bb.to_device(np.ascontiguousarray(com)), bb.to_device(np.ascontiguousarray(starts)), d_g, d_r, d_case, d_ent_init=bb.to_device(np.ascontiguousarray(inits)))
    T.cuda.synchronize()
    beam = _views(d_g, d_r, d_case, S * N, N)
    for k in range(S):
        for a in range(N):
            s = k * N + a
            if on[k, a]:
                _same(got, s, want[k][a], ("active", k, a))
            else:
                assert int(got[1][s]["status"]) == SKIPPED
                assert got[0][s].tobytes() == beam[0][s].tobytes() and got[1][s].tobytes() == beam[1][s].tobytes(), s
                assert (got[2][s] == -7).all() and (beam[2][s] == -7).all()
    bb.set_active(None)
    got = _run(bb, fe, com, starts, inits, S * N, N)
    for k in range(S):
        for a in range(N):
            _same(got, k * N + a, want[k][a], ("all on again", k, a))
    bb.check()
    bb.close()


def test_both_searches_share_one_handle(be, oracle):
    """The two searches are one kernel template behind one launcher and share a handle's node pool, heap and voxel table (the check adds
    the key's third word): check off, check on, check off again on one handle, stale bytes in the outputs before each launch.  Each
    launch equals its own reference, and the two references differ, so that a mix-up cannot pass."""
    sc, inits, _ = cases.setup("plain"); p = sc["par"]; N = p.num_agents
    starts = cases.starts_of("plain")
    fe_off = scene.frontend_cfg(p)
    off = {}
    for a in range(N):
        hx, hn = oracle.hulls_of_scene(p, a + 1, sc["committed"], float(starts[a]["t_start"]), sc["statics"])
        off[a] = oracle.frontend_astar(p, fe_off, a + 1, starts[a], hx, hn, sc["statics"], max_pops=40)
    on = cases.want(oracle, "plain", max_pops=40)
    assert [off[a][1]["status"] for a in range(N)] == [1, 0, 0, 3, 1, 3, 1, 0] and _col(on, "status") == [0, 0, 0, 3, 0, 3, 0, 0]
    assert sum(np.asarray(off[a][0]).tobytes() != np.asarray(on[a][0]).tobytes() for a in range(N)) >= 4
    assert on[6][1]["n_entangled"] == 290 and all(off[a][1]["n_entangled"] == 0 for a in range(N))
    bb = _handle(be, sc)
    bb.set_fe_astar(40)
    d_com = bb.to_device(np.ascontiguousarray(sc["committed"])); d_start = bb.to_device(np.ascontiguousarray(starts))

    def check_off(where):
        d_g, d_r, _ = _buffers(bb, N, N)
        bb.frontend_astar(fe_off, d_com, d_start, d_g, d_r)
        bb.torch.cuda.synchronize()
        got_g, got_r = d_g.cpu().numpy().view(abi.GUESS_DTYPE), d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE)
        for a in range(N):
            g, r = off[a]
            for f in abi.FE_RESULT_DTYPE.names:
                assert got_r[a][f].item() == r[f], (where, a, f, got_r[a][f].item(), r[f])
            assert got_g[a].tobytes() == np.asarray(g).tobytes(), (where, a, "guess bytes")

    check_off("check off, first")
    got = _run(bb, cases.fe_cfg(p), sc["committed"], starts, inits, N, N)
    for a in range(N):
        _same(got, a, on[a], ("check on, between", "agent", a))
    check_off("check off, after the check")
    bb.check()
    bb.close()


def test_capture(be, oracle):
    """Test 7: after one eager call the call allocates nothing: captured and replayed twice it writes the eager call's bytes."""
    sc, inits, pops = cases.setup("plain"); p = sc["par"]
    want = cases.want(oracle, "plain")
    bb = _handle(be, sc)
    bb.set_fe_astar(pops)
    T = bb.torch
    fe = cases.fe_cfg(p)
    d_com = bb.to_device(sc["committed"]); d_start = bb.to_device(cases.starts_of("plain")); d_init = bb.to_device(inits)
    d_g, d_r, d_case = _buffers(bb, 8, 8)
    bb.frontend_astar_ent(fe, d_com, d_start, d_g, d_r, d_case, d_ent_init=d_init)
    T.cuda.synchronize()
    eager = (d_g.cpu().numpy().tobytes(), d_r.cpu().numpy().tobytes(), d_case.cpu().numpy().tobytes())
    gr = T.cuda.CUDAGraph()
    with T.cuda.graph(gr):
        bb.frontend_astar_ent(fe, d_com, d_start, d_g, d_r, d_case, d_ent_init=d_init)
    for _ in range(2):
        d_g.fill_(0xAB); d_r.fill_(0xAB); d_case.fill_(-7)
        gr.replay()
        T.cuda.synchronize()
        assert (d_g.cpu().numpy().tobytes(), d_r.cpu().numpy().tobytes(), d_case.cpu().numpy().tobytes()) == eager
    got = _views(d_g, d_r, d_case, 8, 8)
    for a in range(8):
        _same(got, a, want[a], ("agent", a))
    del gr
    bb.close()


def test_back_end_on_device_made_guesses_and_cases(be, oracle):
    """Test 8: nep_batch_replan on the search's guesses AND its case block: statuses and lines equal the oracle fed the same."""
    sc, inits, pops = cases.setup("bends"); p = sc["par"]; N = p.num_agents
    bb = _handle(be, sc)
    bb.set_fe_astar(pops)
    d_g, d_r, d_case = _buffers(bb, N, N)
    bb.frontend_astar_ent(cases.fe_cfg(p), bb.to_device(sc["committed"]), bb.to_device(cases.starts_of("bends")), d_g, d_r, d_case, d_ent_init=bb.to_device(inits))
    got_g, got_r, got_case = _views(d_g, d_r, d_case, N, N)
    assert int((got_case != 0).sum()) > 0
    bb.set_line_cull(0.0)        # (the lines are compared in the oracle's order)
    bb.replan(None, d_g, d_ent=d_case)
    sol = bb.solutions()
    solved = 0
    for a in range(N):
        K = int(got_g[a]["K"])
        if K < 1:
            assert int(sol[a]["stats"]["status"]) == 2
            continue
        r = oracle.replan(p, a + 1, sc["committed"], got_g[a], sc["statics"], case_id=got_case[a])
        seg, nd = bb.debug_lines(a)
        np.testing.assert_array_equal(nd, r["line_nd"])
        assert int(sol[a]["stats"]["status"]) == r["status"], a
        assert np.abs(np.array(sol[a]["coeff"])[:, :K, :] - r["coeff"]).max() <= 1e-6
        solved += r["status"] != 2
    assert solved >= 8
    bb.close()


def test_loops(be):
    """Test 9: the fleet loops with search="astar_ent": DeviceFleetLoop on one scene flies FleetLoop's flight (every replan's outcome, K
    and statuses, the counters), its captured rounds fly its eager ones, and the audit's invariants hold."""
    from neptune_amd.loop import DeviceFleetLoop, FleetLoop
    sc = scene.make_scene(8, 4, seed=1)
    with pytest.raises(ValueError):
        DeviceFleetLoop([sc], search="astar_ent")
    with pytest.raises(ValueError):
        FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), search="astar_ent")
    ref = FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), audit=True, tethers=True, search="astar_ent", max_pops=150)
    ref.trace = []
    st = ref.run(max_rounds=12)
    ref.close()
    flown = []
    for graph in (False, True):
        loop = DeviceFleetLoop([sc], audit=True, trace=True, graph=graph, tethers=True, search="astar_ent", max_pops=150)
        rep = loop.run(max_rounds=12)[0]
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
    assert len({e[4] for e in trace}) >= 2                                              # (not all one kind of search)
    assert rep["rounds"] == st["rounds"] and rep["reached"] == st["reached"]
    for k in ("replans", "accepted", "fe_no_solution", "qp_failed", "rejected_by_safety", "qp_relaxed", "solves"):
        assert rep[k] == st[k], (k, rep[k], st[k])
    assert flown[0] == flown[1]                                                         # captured == eager: trace, report, audit bytes
    print("astar_ent flight, 12 rounds at 150 pops: reached %d of 8, accepted %d of %d replans, min_box_clear %r min_static_dist %r"
          % (rep["reached"], rep["accepted"], rep["replans"], rep["audit"]["min_box_clear"], rep["audit"]["min_static_dist"]))
    assert rep["audit"]["min_box_clear"]["value"] >= -1e-6, rep["audit"]
    assert rep["audit"]["min_static_dist"]["value"] >= -1e-6 and rep["audit"]["n_static_viol"] == 0, rep["audit"]


def test_contract(be):
    """Test 10: the argument and state checks of the entry point."""
    from neptune_amd._lib import BackendError
    sc, inits, pops = cases.setup("plain"); p = sc["par"]
    fe = cases.fe_cfg(p)
    d_g = None
    plain = be.BatchBackend(scene.make_scene(8, 6, seed=5)["par"], sc["statics"])       # a handle created without enable_entangle
    plain.set_fe_astar(100)
    d_com = plain.to_device(sc["committed"]); d_start = plain.to_device(cases.starts_of("plain"))
    d_g = plain.torch.zeros(8 * abi.GUESS_DTYPE.itemsize, dtype=plain.torch.uint8, device=plain.device)
    with pytest.raises(BackendError, match="error -2"):                               # NEP_E_STATE
        plain.frontend_astar_ent(fe, d_com, d_start, d_g)
    plain.close()
    shard = be.BatchBackend(p, sc["statics"], first_local=2, n_local=2)               # a sharded handle
    shard.set_fe_astar(100)
    with pytest.raises(BackendError, match="error -2"):
        shard.frontend_astar_ent(fe, d_com, d_start, d_g)
    shard.close()
    bb = _handle(be, sc)
    with pytest.raises(BackendError, match="error -2"):                               # NEP_E_STATE: before the setter
        bb.frontend_astar_ent(fe, d_com, d_start, d_g)
    bb.set_fe_astar(100, 0, list(range(25)))
    with pytest.raises(BackendError, match="error -1"):                               # NEP_E_ARG: enable_entangle off in the configuration
        bb.frontend_astar_ent(scene.frontend_cfg(p), d_com, d_start, d_g)
    with pytest.raises(BackendError, match="error -1"):                               # num_samples^2 != n_order
        bb.frontend_astar_ent(cases.fe_cfg(p, num_samples=4), d_com, d_start, d_g)
    with pytest.raises(BackendError, match="error -1"):                               # nep_batch_frontend_astar keeps refusing the check
        bb.frontend_astar(fe, d_com, d_start, d_g)
    bb.frontend_astar_ent(fe, d_com, d_start, d_g)                                    # results and case block are optional
    bb.check()
    bb.close()
