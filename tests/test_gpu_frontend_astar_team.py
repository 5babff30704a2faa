"""The best-first search with the entangle check on four waves per search (nep_batch_set_fe_astar_team): bit-identical to
the one-wave kernel on the same handle and to tests/astar_ent_ref.py.  Every comparison covers the whole nep_guess byte for byte, every
field of nep_fe_result and the case block, asserts that the team kernel really ran (fe_astar_team() == 4) and asserts the ref's own
outcomes next to it, so that a test cannot pass by covering nothing.  The set-ups are tests/astar_ent_cases.py's (the ref's outcome is
computed once per set-up and shared with test_gpu_frontend_astar_ent.py); the shapes are the smallest at which each part of the team
form can go wrong: three fleet sizes (uneven chunks of the obstacle range), item counts other than 75, 1 and 8 sampled steps, the list
cap and a step that adds more than 32 crossings in every child (the peak-count rule), a pool that cuts an expansion, several scenes
and an active set, 2 N + S > 256 (the strided collision loop), and one handle switched between the forms."""
import numpy as np
import pytest

import astar_ent_cases as cases
from neptune_amd import abi, scene

pytestmark = pytest.mark.gpu

BUDGET, GOAL, EMPTY, NO_SOLUTION, SKIPPED = 0, 1, 2, 3, 4
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


def _run(bb, team, fe, com, starts, inits, n_slots, N):
    """one call with `team` waves per search on fresh 0xAB buffers -> (guesses, results, case block); the reader says which kernel ran"""
    bb.set_fe_astar_team(team)
    d_g, d_r, d_case = _buffers(bb, n_slots, N)
    bb.frontend_astar_ent(fe, bb.to_device(np.ascontiguousarray(com)), bb.to_device(np.ascontiguousarray(starts)), d_g, d_r, d_case,
                          d_ent_init=bb.to_device(np.ascontiguousarray(inits)) if inits is not None else None)
    bb.torch.cuda.synchronize()
    assert bb.fe_astar_team() == team
    return _views(d_g, d_r, d_case, n_slots, N)


def _bytes(got):
    return tuple(x.tobytes() for x in got)


def _both(bb, fe, com, starts, inits, n_slots, N, where):
    """the one-wave kernel, then the team kernel, same inputs, same handle: every output byte equal -> the team form's outputs"""
    one = _run(bb, 1, fe, com, starts, inits, n_slots, N)
    four = _run(bb, 4, fe, com, starts, inits, n_slots, N)
    for k, what in enumerate(("guess", "result", "case block")):
        assert _bytes(one)[k] == _bytes(four)[k], (where, what, "team form differs from the one-wave form")
    return four


def _same(got, a, want, where):
    got_g, got_r, got_case = got
    g, r, case, _ = want
    for f in abi.FE_RESULT_DTYPE.names:
        assert got_r[a][f].item() == r[f], (where, f, got_r[a][f].item(), r[f])
    assert got_g[a].tobytes() == np.asarray(g).tobytes(), (where, "guess bytes", int(got_g[a]["K"]), int(g["K"]))
    np.testing.assert_array_equal(got_case[a], case, err_msg="case block, %r" % (where,))


def _device(be, name, max_pops=None, order=None, num_samples=5, max_nodes=0, ent_samples=3):
    sc, inits, pops = cases.setup(name); p = sc["par"]
    bb = _handle(be, sc)
    bb.set_fe_astar(pops if max_pops is None else max_pops, max_nodes, order)
    fe = scene.frontend_cfg(p, num_samples=num_samples, pad_hold=0, entangle=True, ent_samples=ent_samples)
    got = _both(bb, fe, sc["committed"], cases.starts_of(name), inits, p.num_agents, p.num_agents, (name, max_pops, num_samples, max_nodes, ent_samples))
    return bb, got


def _col(want, f):
    return [want[a][1][f] for a in sorted(want)]


@pytest.mark.parametrize("name", ["bends", "many_bends", "doubly"])
def test_scene_setups(be, oracle, name):
    """16 + 8, 12 + 4 and 8 + 6 obstacles: three sizes of the index range, so uneven chunks; tethers of 2-4 and 5-8 bend points;
    searches that end NEP_FE_NO_SOLUTION after the whole budget."""
    want = cases.want(oracle, name)
    N = len(want)
    st = _col(want, "status")
    assert len(set(st)) >= 3 and (name == "doubly" or sum(_col(want, "n_entangled")) > 0), st
    assert sum(c["updates"] for _, _, _, c in want.values()) > 0 and sum(c["iz_shared"] for _, _, _, c in want.values()) > 0
    if name == "bends":
        assert sum(_col(want, "n_entangled")) == 1068 and sum(int((w[2] != 0).sum()) for w in want.values()) > 0
    if name == "doubly":
        assert st == [3, 0, 3, 3, 1, 3, 1, 0] and [want[a][1]["n_children"] for a in (0, 2)] == [300, 300]
    assert all(r["ent_overflow"] == 0 for _, r, _, _ in want.values())
    bb, got = _device(be, name)
    for a in range(N):
        _same(got, a, want[a], (name, "agent", a))
    bb.check()
    bb.close()


@pytest.mark.parametrize("case", ["pops1", "pops40", "order", "ns3"])
def test_budgets_order_and_lattice(be, oracle, case):
    """Budgets 1 and 40, a shuffled lattice order and the 3 x 3 lattice on (8, 6, 60): item counts other than 75."""
    kw = dict(pops1=dict(max_pops=1), pops40=dict(max_pops=40), order=dict(order=SHUFFLED), ns3=dict(num_samples=3))[case]
    want = cases.want(oracle, "plain", **kw)
    assert len(set(_col(want, "status"))) >= 2 and any(r["K"] >= 1 for _, r, _, _ in want.values())
    if case == "pops1":
        assert all(r["n_children"] <= 1 for _, r, _, _ in want.values())
    else:
        assert sum(_col(want, "n_entangled")) > 0
    bb, got = _device(be, "plain", **kw)
    for a in range(8):
        _same(got, a, want[a], (case, "agent", a))
    bb.check()
    bb.close()


@pytest.mark.parametrize("ent_samples", [1, 8])
def test_one_and_eight_sampled_steps(be, oracle, ent_samples):
    """ent_samples 1 and 8: 25 and 200 (child, step) pairs, against the one-wave kernel — and against the ref, which samples the
    trajectories at the same count (tests/test_fe_cfg_cases_cpu.py pins it away from the default configuration)."""
    bb, got = _device(be, "plain", max_pops=40, ent_samples=ent_samples)
    r = got[1]
    assert len({int(x) for x in r["status"]}) >= 2 and int(r["n_children"].max()) == 40 and int(r["n_entangled"].sum()) > 0, r
    want = cases.want(oracle, "plain", max_pops=40, ent_samples=ent_samples)
    for a in range(8):
        _same(got, a, want[a], ("ent_samples", ent_samples, "agent", a))
    bb.check()
    bb.close()


@pytest.mark.parametrize("n", [41, 44])
def test_fixed_record_overflow(be, oracle, n):
    """helpers.bundle_scene: with 40 tethers the list cap binds; with 43 every first step adds more than 32 crossings in every child —
    the capacity flag of a chunked list comes from base + peak, not from the final length.  Flags, NEP_E_CAP from check() once, _pad == 0."""
    from neptune_amd._lib import BackendError
    name = "bundle%d" % n
    agents = (7, 0, n // 2)
    want = cases.want(oracle, name, agents=agents)
    r7 = want[7][1]
    assert r7["ent_overflow"] == 1 and all(want[a][1]["ent_overflow"] == 0 for a in agents[1:])
    if n == 41:
        assert (r7["status"], r7["K"], r7["depth"], r7["n_children"], r7["n_feasible"]) == (BUDGET, 8, 13, 150, 670)
        assert want[7][3]["max_list"] == abi.NEP_FE_ENT_CAP
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


def test_pool_budget(be, oracle):
    """A 64-node pool: the cap cuts an expansion at a child; the children behind the cut are not counted."""
    from neptune_amd._lib import BackendError
    want = cases.want(oracle, "plain", max_nodes=64)
    assert _col(want, "_pad") == [16, 16, 16, 0, 16, 0, 0, 16] and _col(want, "n_feasible") == [63, 63, 63, 24, 63, 24, 54, 63]
    bb, got = _device(be, "plain", max_nodes=64)
    for a in range(8):
        _same(got, a, want[a], ("64 nodes", "agent", a))
    with pytest.raises(BackendError, match="error -4"):
        bb.check()
    bb.check()
    bb.close()


def test_three_scenes_and_an_active_set(be, oracle):
    """Three scenes in one launch, then an active set: an inactive slot carries nep_batch_frontend_ent's bytes."""
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
    got = _both(bb, fe, com, starts, inits, S * N, N, "three scenes")
    for k in range(S):
        for a in range(N):
            _same(got, k * N + a, want[k][a], ("scene", k, "agent", a))
    T = bb.torch
    on = np.array([[1, 0, 1, 1, 0, 0, 1, 0], [0, 1, 1, 0, 1, 1, 0, 1], [1, 1, 0, 0, 0, 1, 1, 1]], dtype=np.int32)
    bb.set_active(T.from_numpy(on).to(bb.device))
    got = _both(bb, fe, com, starts, inits, S * N, N, "active set")
    d_g, d_r, d_case = _buffers(bb, S * N, N)
    bb.frontend_ent(fe, bb.to_device(np.ascontiguousarray(com)), bb.to_device(np.ascontiguousarray(starts)), d_g, d_r, d_case, d_ent_init=bb.to_device(np.ascontiguousarray(inits)))
    T.cuda.synchronize()
    assert bb.fe_astar_team() == 4                                                     # (the beam leaves the reader alone)
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
    bb.check()
    bb.close()


def test_more_collision_items_than_threads(be):
    """90 agents and 80 statics: 2 N + S = 260 collision items per pop over 256 threads, and chunks of a 170-obstacle range; 40 pops,
    against the one-wave kernel."""
    sc = scene.tether_crossing_scene(90, 80, 7); p = sc["par"]; N = p.num_agents
    assert 2 * N + len(sc["statics"]) > 256
    bb = _handle(be, sc)
    bb.set_fe_astar(40)
    got = _both(bb, cases.fe_cfg(p), sc["committed"], scene.frontend_starts(sc), None, N, N, "90 + 80")
    r = got[1]
    assert len({int(x) for x in r["status"]}) >= 2 and int(r["n_children"].max()) == 40 and int(r["K"].max()) >= 1, r
    bb.close()


def test_one_handle_switched_between_the_forms_and_capture(be, oracle):
    """One handle 1 -> 4 -> 1 -> 4, fresh 0xAB buffers each time: every call equals the ref.  Then the team form captured after its
    eager call and replayed twice: the eager call's bytes, whatever the setter says afterwards (a graph keeps the form it was captured with)."""
    sc, inits, pops = cases.setup("plain"); p = sc["par"]
    want = cases.want(oracle, "plain")
    assert len(set(_col(want, "status"))) >= 2 and sum(_col(want, "n_entangled")) > 0
    bb = _handle(be, sc)
    bb.set_fe_astar(pops)
    fe = cases.fe_cfg(p)
    assert bb.fe_astar_team() == 0                                                     # (no call yet)
    for k, team in enumerate((1, 4, 1, 4)):
        got = _run(bb, team, fe, sc["committed"], cases.starts_of("plain"), inits, 8, 8)
        for a in range(8):
            _same(got, a, want[a], ("call", k, "team", team, "agent", a))
    T = bb.torch
    d_com = bb.to_device(sc["committed"]); d_start = bb.to_device(cases.starts_of("plain")); d_init = bb.to_device(inits)
    d_g, d_r, d_case = _buffers(bb, 8, 8)
    bb.frontend_astar_ent(fe, d_com, d_start, d_g, d_r, d_case, d_ent_init=d_init)
    T.cuda.synchronize()
    eager = (d_g.cpu().numpy().tobytes(), d_r.cpu().numpy().tobytes(), d_case.cpu().numpy().tobytes())
    gr = T.cuda.CUDAGraph()
    with T.cuda.graph(gr):
        bb.frontend_astar_ent(fe, d_com, d_start, d_g, d_r, d_case, d_ent_init=d_init)
    bb.set_fe_astar_team(1)                                                            # (does not reach into the graph)
    for _ in range(2):
        d_g.fill_(0xAB); d_r.fill_(0xAB); d_case.fill_(-7)
        gr.replay()
        T.cuda.synchronize()
        assert (d_g.cpu().numpy().tobytes(), d_r.cpu().numpy().tobytes(), d_case.cpu().numpy().tobytes()) == eager
    got = _views(d_g, d_r, d_case, 8, 8)
    for a in range(8):
        _same(got, a, want[a], ("replayed", "agent", a))
    del gr
    bb.check()
    bb.close()


def test_flight(be):
    """DeviceFleetLoop(tethers=True, search="astar_ent") on (8, 6), 60 pops, 10 rounds: team=4 leaves the states, plans, trajectories,
    tether states and counters of the team=1 flight, byte for byte."""
    from neptune_amd.loop import DeviceFleetLoop
    sc = scene.make_scene(8, 6, seed=1)
    flown = []
    for team in (1, 4):
        loop = DeviceFleetLoop([sc], trace=True, graph=False, tethers=True, search="astar_ent", max_pops=60, team=team)
        for _ in range(10):
            loop.round()
        rep = loop.report()[0]
        assert loop.be.fe_astar_team() == team
        snap = loop.be.fleet_snapshot()
        loop.torch.cuda.synchronize()
        flown.append(dict(snapshot=snap.cpu().numpy().tobytes(), trace=loop.trace, report=rep, fe_result=loop.d_res.cpu().numpy().tobytes(),
                          outcome=loop.d_outcome.cpu().numpy().tobytes(), solution=loop.be.solutions().tobytes()))
        loop.close()
    rep = flown[0]["report"]
    assert rep["rounds"] == 10 and rep["accepted"] > 0, rep
    for k in flown[0]:
        assert flown[0][k] == flown[1][k], ("team=4 flew another flight than team=1", k)


def test_contract(be):
    """waves 0, 2 and 5 are NEP_E_ARG; the setter is legal before set_fe_astar and survives it; frontend_astar (check off) keeps its one
    wave and its bytes after set_fe_astar_team(4), and leaves the reader's last value alone."""
    from neptune_amd._lib import BackendError
    from neptune_amd.loop import DeviceFleetLoop
    sc, inits, _ = cases.setup("plain"); p = sc["par"]; N = p.num_agents
    starts = cases.starts_of("plain")
    bb = _handle(be, sc)
    for waves in (0, 2, 5):
        with pytest.raises(BackendError, match="error -1"):
            bb.set_fe_astar_team(waves)
    bb.set_fe_astar_team(4)                                                            # before set_fe_astar: fine
    bb.set_fe_astar(40)                                                                # ... which leaves it alone
    fe_off = scene.frontend_cfg(p)
    d_com = bb.to_device(np.ascontiguousarray(sc["committed"])); d_start = bb.to_device(np.ascontiguousarray(starts))

    def off():
        d_g, d_r, _ = _buffers(bb, N, N)
        bb.frontend_astar(fe_off, d_com, d_start, d_g, d_r)
        bb.torch.cuda.synchronize()
        return d_g.cpu().numpy().tobytes(), d_r.cpu().numpy().tobytes()

    with_four = off()
    assert bb.fe_astar_team() == 0                                                     # (check off: no entangle-aware call yet)
    bb.set_fe_astar_team(1)
    assert off() == with_four
    bb.set_fe_astar_team(4)
    d_g, d_r, d_case = _buffers(bb, N, N)
    bb.frontend_astar_ent(cases.fe_cfg(p), d_com, d_start, d_g, d_r, d_case, d_ent_init=bb.to_device(inits))
    bb.torch.cuda.synchronize()
    assert bb.fe_astar_team() == 4                                                     # (set before set_fe_astar, still in force)
    assert off() == with_four and bb.fe_astar_team() == 4
    bb.check()
    bb.close()
    one = scene.make_scene(8, 4, seed=1)
    with pytest.raises(ValueError):
        DeviceFleetLoop([one], search="astar", team=4)
    with pytest.raises(ValueError):
        DeviceFleetLoop([one], tethers=True, search="astar_ent", team=3)
