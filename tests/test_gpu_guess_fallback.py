"""GPU: the reference's degrade-to-initial-guess rule (nep_batch_guess_fallback / _tally, include/neptune_backend.h)
against tests/guess_fallback_ref.py.  The kernel alone behind a replan (every byte it owes and every byte it must leave), the
safety pass downstream of it, other handles (an active mask, num_pol = 5, a shard, the contracts, a capture), and the rule in flight
in both fleet loops — eager with the rules after every round, captured, rewound, resumed — with the counts.  Every flight asserts
that guesses were actually flown, so that a test cannot pass by covering nothing."""
import ctypes as C
import dataclasses
import functools
import json

import numpy as np
import pytest

import guess_fallback_ref as ref
import test_gpu_fleet_recorder as tr
from neptune_amd import abi, mission, plan, scene

pytestmark = pytest.mark.gpu

REC, SOL = abi.TRAJ_REC_DTYPE, abi.SOLUTION_DTYPE
MASK = ref.written_mask(REC.itemsize, REC.fields)      # the bytes of a record the replan's writer writes
COUNTS = abi.GUESS_FALLBACK_COUNTS


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _np(t, dtype):
    return t.cpu().numpy().view(dtype).copy()


def _bytes(a):
    return np.frombuffer(a.tobytes(), dtype=np.uint8).reshape(len(a), -1)


def _marked(prev, marker):
    """the previous records with `marker` in every byte the writer of a new record leaves alone, and a z no new record carries"""
    prev = prev.copy()
    b = prev.view(np.uint8).reshape(len(prev), -1)
    b[:, ~MASK] = marker
    prev["pos"][:, 2] = 7.25
    return prev


def _raw(bb):
    """solutions (solve_us included), states and commit records as they lie on the device"""
    bb.torch.cuda.synchronize(bb.device)
    return _np(bb.d_solution, SOL), bb.states(), bb.commits()


# ---- 1. the kernel behind a replan -------------------------------------------------------------------------------------------------
def _launch(torch, bb, sc, gue, given, fill, marker):
    """replan (d_committed given, or None behind a front end) into a d_commit full of `fill`, then the call, then the call again"""
    p = sc["par"]
    prev = _marked(sc["committed"], marker)
    d_prev, d_gue = bb.to_device(prev), bb.to_device(gue)
    bb.d_commit.fill_(fill)
    if given:
        bb.replan(d_prev, d_gue)
    else:
        fe = scene.frontend_cfg(p, beam_width=32, pad_hold=1)
        d_g = torch.zeros(5 * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=bb.device)
        bb.frontend(fe, d_prev, bb.to_device(np.ascontiguousarray(scene.frontend_starts(sc))), d_g)
        bb.replan(None, d_gue)
    before = _raw(bb)
    d_count = torch.zeros((1, 4), dtype=torch.int32, device=bb.device)
    bb.guess_fallback(d_gue, d_count)
    after = _raw(bb)
    c1 = d_count.cpu().numpy().copy()
    bb.guess_fallback(d_gue, d_count)
    again = _raw(bb)
    return prev, before, after, c1, again, d_count.cpu().numpy().copy()


@pytest.mark.parametrize("given", [True, False])
def test_kernel_behind_a_replan(torch, given):
    from neptune_amd.backend import BatchBackend
    sc, gue = ref.fixture(scene)
    p = sc["par"]
    bb = BatchBackend(p, sc["statics"])
    try:
        runs = [_launch(torch, bb, sc, gue, given, fill, marker) for fill, marker in ((0xAB, 0x5A), (0x54, 0xA5))]
        bb.check()
    finally:
        bb.close()
    for (prev, (sol0, st0, com0), (sol1, st1, com1), c1, (sol2, st2, com2), c2), fill in zip(runs, (0xAB, 0x54)):
        assert sol0["stats"]["status"].tolist() == [0, 2, 2, 2, 0] and sol0["K"].tolist() == [8, 8, 0, 8, 8]
        for a in (1, 2, 3):      # today's rule: the previous record is carried over
            assert com0[a].tobytes() == prev[a].tobytes()
        want_sol, want_com, want_cnt = ref.fallback(sol0, gue, com0, p.num_pol, p.pb, p.drone_radius)
        assert sol1["stats"]["status"].tolist() == [0, 4, 2, 4, 0]
        assert sol1.tobytes() == want_sol.tobytes()      # status 4 in slots 1 and 3, every other byte of every nep_solution as it was
        assert st1.tobytes() == st0.tobytes()
        assert com1.tobytes() == want_com.tobytes()
        assert c1.tolist() == want_cnt.tolist() == [[3, 2, 0, 0]]
        for a in (1, 3):
            r, g = com1[a], gue[a]
            assert (int(r["id"]), int(r["is_agent"]), int(r["n_bend"]), int(r["valid"]), int(r["pwp"]["n_seg"])) == (a + 1, 1, 1, 1, 8)
            assert r["bbox"].tolist() == [2 * p.drone_radius] * 3 and r["pos"].tolist() == np.array(g["coeff"])[:, 0, 3].tolist()
            assert r["bend"][0].tolist() == np.asarray(p.pb).reshape(-1, 2)[a].tolist()
            assert r["pwp"]["times"][:9].tobytes() == sol1[a]["times"].tobytes() and not r["pwp"]["times"][9:].any()
            assert r["pwp"]["coeff"][:, :8].tobytes() == np.ascontiguousarray(g["coeff"]).tobytes() and not r["pwp"]["coeff"][:, 8:].any()
            assert sol1[a]["coeff"].tobytes() == np.ascontiguousarray(g["coeff"]).tobytes()      # (:856-859)
        assert com1[2].tobytes() == com0[2].tobytes() == prev[2].tobytes()      # K = 0: nothing to publish
        for a in (0, 4):
            assert com1[a].tobytes() == com0[a].tobytes() and sol1[a].tobytes() == sol0[a].tobytes()
        # the second call: no byte moves, the unpublishable slot is counted again
        assert sol2.tobytes() == sol1.tobytes() and st2.tobytes() == st1.tobytes() and com2.tobytes() == com1.tobytes()
        assert (c2 - c1).tolist() == [[1, 0, 0, 0]]
    # the bytes left alone, by two launches with other fills (a written byte may equal one fill by chance, not both): in a solved
    # slot what still holds d_commit's fill, in a published slot what still holds the carried record's marker — the same set
    (_, _, (_, _, ca), _, _, _), (_, _, (_, _, cb), _, _, _) = runs
    ba, bb_ = _bytes(ca), _bytes(cb)
    for solved, published in ((0, 1), (4, 3)):
        left_solved = (ba[solved] == 0xAB) & (bb_[solved] == 0x54)
        left_published = (ba[published] == 0x5A) & (bb_[published] == 0xA5)
        assert (left_solved == left_published).all() and (left_solved == ~MASK).all()


# ---- 2. downstream: the safety pass judges the guess ---------------------------------------------------------------------------------
@pytest.mark.parametrize("call", [True, False])
def test_safety_pass_downstream(torch, call):
    from neptune_amd.backend import BatchBackend
    sc, gue = ref.fixture(scene)
    p = sc["par"]
    prev = _marked(sc["committed"], 0x5A)
    bb = BatchBackend(p, sc["statics"])
    try:
        d_prev, d_gue = bb.to_device(prev), bb.to_device(gue)
        bb.replan(d_prev, d_gue)
        if call:
            bb.guess_fallback(d_gue)
        com = bb.commits()
        d_final = torch.zeros_like(bb.d_commit); d_acc = torch.zeros(5, dtype=torch.int32, device=bb.device)
        bb.safety_commit(d_prev, bb.d_commit, d_gue, d_final, d_acc)
        fin, acc = _np(d_final, REC), d_acc.cpu().numpy().tolist()
        bb.check()
    finally:
        bb.close()
    if call:      # the oracle's verdict (tests/test_guess_fallback_cpu.py): the two guesses collide, the higher id is turned down
        assert acc == [1, 1, 1, 0, 1]
        assert fin[1].tobytes() == com[1].tobytes() and int(com[1]["pwp"]["n_seg"]) == 8 and com[1]["pos"][0] == p.x_max + 5.0
        assert fin[3].tobytes() == prev[3].tobytes()
    else:         # today's assertion (test_failed_and_empty_replans_publish_nothing)
        assert acc == [1, 1, 1, 1, 1]
        assert fin[1].tobytes() == prev[1].tobytes() and fin[3].tobytes() == prev[3].tobytes()
    assert fin[2].tobytes() == prev[2].tobytes()


# ---- 3. other inputs -----------------------------------------------------------------------------------------------------------------
def _against_ref(bb, gue, p, first_local=0, n_local=None, d_count=None):
    """the call on what the last replan left, against the reference: -> (before, after)"""
    d_gue = bb.to_device(gue)
    before = _raw(bb)
    bb.guess_fallback(d_gue, d_count)
    after = _raw(bb)
    want_sol, want_com, want_cnt = ref.fallback(before[0], gue, before[2], p.num_pol, p.pb, p.drone_radius, first_local, n_local)
    assert after[0].tobytes() == want_sol.tobytes() and after[2].tobytes() == want_com.tobytes() and after[1].tobytes() == before[1].tobytes()
    if d_count is not None:
        assert d_count.cpu().numpy().tolist() == want_cnt.tolist()
    return before, after, want_cnt


def test_two_scenes_and_an_active_mask(torch):
    """scene 1 leaves its failing slot 1 out of the active set: NEP_SKIPPED, not examined, not touched"""
    from neptune_amd.backend import BatchBackend
    sc, gue = ref.fixture(scene)
    p = sc["par"]
    bb = BatchBackend(p, sc["statics"], n_scenes=2)
    try:
        mask = torch.ones((2, 5), dtype=torch.int32, device=bb.device); mask[1, 1] = 0
        bb.set_active(mask)
        g2 = np.concatenate([gue, gue]); prev = np.concatenate([sc["committed"]] * 2)
        bb.d_commit.fill_(0xAB)
        bb.replan(bb.to_device(prev), bb.to_device(g2))
        d_count = torch.zeros((2, 4), dtype=torch.int32, device=bb.device)
        (sol0, _, com0), (sol1, _, com1), cnt = _against_ref(bb, g2, p, n_local=5, d_count=d_count)
        bb.check()
    finally:
        bb.close()
    assert sol0["stats"]["status"].tolist() == [0, 2, 2, 2, 0, 0, 3, 2, 2, 0]
    assert sol1["stats"]["status"].tolist() == [0, 4, 2, 4, 0, 0, 3, 2, 4, 0]
    assert cnt.tolist() == [[3, 2, 0, 0], [2, 1, 0, 0]]
    assert com1[6].tobytes() == com0[6].tobytes() and sol1[6].tobytes() == sol0[6].tobytes()


def test_num_pol_5_and_a_guess_of_7_segments(torch):
    """a guess longer than the handle's num_pol is never solved and has nothing to publish; a failed guess of 5 segments is published
    with 5"""
    from neptune_amd.backend import BatchBackend
    sc, gue = ref.fixture(scene)
    p = dataclasses.replace(sc["par"], num_pol=5)
    gue = gue.copy()
    gue["K"][:] = [5, 5, 7, 0, 5]
    bb = BatchBackend(p, sc["statics"])
    try:
        bb.replan(bb.to_device(sc["committed"]), bb.to_device(gue))
        d_count = torch.zeros((1, 4), dtype=torch.int32, device=bb.device)
        (sol0, _, com0), (sol1, _, com1), cnt = _against_ref(bb, gue, p, d_count=d_count)
    finally:
        bb.close()
    assert sol0["stats"]["status"][1:4].tolist() == [2, 2, 2] and sol0["K"][1:4].tolist() == [5, 0, 0]
    assert sol1["stats"]["status"][1:4].tolist() == [4, 2, 2]
    assert cnt[0, 1] == int((sol1["stats"]["status"] == 4).sum()) and cnt[0, 0] == cnt[0, 1] + 2
    assert int(com1[1]["pwp"]["n_seg"]) == 5 and not com1[1]["pwp"]["times"][6:].any() and not com1[1]["pwp"]["coeff"][:, 5:].any()
    for a in (2, 3):
        assert com1[a].tobytes() == com0[a].tobytes()


def test_sharded_handle_publishes_the_global_agent(torch):
    """first_local = 2, n_local = 2 of N = 4: id and bend[0] are the global agent's"""
    from neptune_amd.backend import BatchBackend
    sc = scene.make_scene(4, 3, seed=4)
    p = sc["par"]
    gue = sc["guesses"][2:4].copy()
    gue[1] = ref.infeasible_guess(gue[1], p.x_max)
    bb = BatchBackend(p, sc["statics"], first_local=2, n_local=2)
    try:
        bb.d_commit.fill_(0xAB)
        bb.replan(bb.to_device(sc["committed"]), bb.to_device(gue))
        d_count = torch.zeros((1, 4), dtype=torch.int32, device=bb.device)
        (sol0, _, _), (sol1, _, com1), cnt = _against_ref(bb, gue, p, first_local=2, n_local=2, d_count=d_count)
    finally:
        bb.close()
    assert int(sol0[1]["stats"]["status"]) == 2 and int(sol1[1]["stats"]["status"]) == 4 and cnt[0, 1] >= 1
    assert int(com1[1]["id"]) == 4 and com1[1]["bend"][0].tolist() == np.asarray(p.pb).reshape(-1, 2)[3].tolist()


def test_contracts_and_capture(torch):
    from neptune_amd._lib import lib
    from neptune_amd.backend import BatchBackend
    L = lib()
    sc, gue = ref.fixture(scene)
    p = sc["par"]
    bb = BatchBackend(p, sc["statics"])
    try:
        dev = bb.device
        d_prev, d_gue = bb.to_device(sc["committed"]), bb.to_device(gue)
        st = torch.cuda.current_stream(dev).cuda_stream
        ptr = (d_gue.data_ptr(), bb.d_solution.data_ptr(), bb.d_commit.data_ptr())
        bb.d_commit.fill_(0xAB); bb.d_solution.fill_(0xAB)
        assert L.nep_batch_guess_fallback(None, *ptr, None, st) == -1         # NEP_E_ARG: a device and no handle
        assert L.nep_batch_guess_fallback(bb._h, *ptr, None, st) == -2        # NEP_E_STATE: no replan yet
        bb.replan_lines(d_prev, d_gue)
        assert L.nep_batch_guess_fallback(bb._h, *ptr, None, st) == -2        # (the geometry half alone is no replan)
        torch.cuda.synchronize()
        assert bool((bb.d_commit == 0xAB).all()) and bool((bb.d_solution == 0xAB).all())      # the refused calls wrote nothing
        bb.replan_solve(d_prev, d_gue)
        for i in range(3):
            bad = list(ptr); bad[i] = None
            assert L.nep_batch_guess_fallback(bb._h, *bad, None, st) == -1
        d_out = torch.zeros(5, dtype=torch.int32, device=dev); d_count = torch.zeros((1, 4), dtype=torch.int32, device=dev)
        for bad in ((None, d_out.data_ptr(), d_count.data_ptr()), (ptr[1], None, d_count.data_ptr()), (ptr[1], d_out.data_ptr(), None)):
            assert L.nep_batch_guess_fallback_tally(bb._h, *bad, st) == -1
        torch.cuda.synchronize()
        assert _np(bb.d_solution, SOL)["stats"]["status"].tolist() == [0, 2, 2, 2, 0]

        # eager once, then replan + the call + the tally inside a capture: nothing is allocated, and the replay leaves the eager bytes
        d_out.copy_(torch.tensor([4, 4, 4, 3, 4], dtype=torch.int32))      # (outcomes as a fleet commit would leave them)

        def ops():
            bb.replan(d_prev, d_gue)
            bb.guess_fallback(d_gue, d_count)
            bb.guess_fallback_tally(d_out, d_count)
        ops()
        sol1, st1, com1 = _raw(bb)
        assert sol1["stats"]["status"].tolist() == [0, 4, 2, 4, 0] and d_count.cpu().numpy().tolist() == [[3, 2, 1, 1]]
        dev0, dev1, pin = C.c_int64(), C.c_int64(), C.c_int64()
        L.nep_debug_live_bytes(C.byref(dev0), C.byref(pin))
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            ops()
            g.capture_end()
        torch.cuda.current_stream(dev).wait_stream(s)
        L.nep_debug_live_bytes(C.byref(dev1), C.byref(pin))
        assert dev1.value == dev0.value
        assert d_count.cpu().numpy().tolist() == [[3, 2, 1, 1]]      # (captured, not run)
        bb.d_commit.fill_(0xAB); bb.d_solution.fill_(0xAB)
        g.replay()
        sol2, st2, com2 = _raw(bb)
        sol1["stats"]["solve_us"] = 0.0; sol2["stats"]["solve_us"] = 0.0      # (the one field that is a measurement)
        assert sol2.tobytes() == sol1.tobytes() and st2.tobytes() == st1.tobytes() and com2.tobytes() == com1.tobytes()
        assert d_count.cpu().numpy().tolist() == [[6, 4, 2, 2]]
        bb.check()
        del g
    finally:
        bb.close()


# ---- 4. the chain to the fleet ---------------------------------------------------------------------------------------------------------
ROUNDS = 20
TICK = 1e-8      # set_max_runtime: one tick of the 100 MHz wall clock — every solve that iterates fails (test_wall_clock_time_limit)


@functools.lru_cache(maxsize=None)
def _scene(n, m, seed):
    return scene.make_scene(n, m, seed=seed)


def _fleet():
    """2 scenes of 8 + 4.  Seeds 21 and 33: on the default solve path, without a time limit, their first replan whose two solves
    fail comes in round 15 of either scene (found on the GPU among seeds 1..40: most have none in 20 rounds, some one by round 3)"""
    return (_scene(8, 4, 21), _scene(8, 4, 33))


def _before(lp):
    fs = lp.be.fleet_state(pwp=True)
    return dict(plans=lp.be.fleet_plans(), done=fs["done"] != 0, flown=fs["flown"] != 0, pwp=fs["pwp"].copy(), k_end=None,
                t_now=lp.be.fleet_counters()[1].copy())


def _rules(lp, before, seen):
    """after fleet_commit and the tally of an eager round, on the downloaded buffers: no publishable failure is left; every published
    slot's record is the reference's for the guess, its solution holds the guess; an accepted one was flown — its states at the end
    of the ring, its trajectory the composition of the guess; a gated slot is never published"""
    be, S, N, p = lp.be, lp.S, lp.N, lp.p
    sol, states, com = _raw(be)
    guess, res = _np(lp.d_guess, abi.GUESS_DTYPE), _np(lp.d_res, abi.FE_RESULT_DTYPE)
    rec = _np(lp.d_rec, REC)
    acc, outcome = lp.d_acc.cpu().numpy(), lp.d_outcome.cpu().numpy()
    plans, fs = be.fleet_plans(), be.fleet_state(pwp=True)
    cnt = np.zeros((S, 4), dtype=np.int64)
    for i in range(S * N):
        s, a = divmod(i, N)
        status, K = int(sol[i]["stats"]["status"]), int(sol[i]["K"])
        gated = bool(int(res[i]["_pad"]) & abi.NEP_FE_PAD_GATED)
        if gated:
            assert status == ref.FAILED and K == 0, ("a gated slot is never published", lp.rounds, i, status, K)
            seen["gated"] += 1
        if status == ref.FAILED:
            assert K == 0, ("a failure with a usable guess was left", lp.rounds, i, K)
            cnt[s] += (1, 0, 0, 0)
            assert outcome[i] in (abi.NEP_FLEET_SKIPPED, abi.NEP_FLEET_FE_NO_SOLUTION)
        if status != ref.GUESS:
            continue
        assert 1 <= K <= p.num_pol and int(guess[i]["K"]) == K and not gated
        assert sol[i]["coeff"][:, :K].tobytes() == guess[i]["coeff"][:, :K].tobytes()
        want = ref.record(com[i], sol[i], guess[i], a, p.pb, p.drone_radius)
        if lp.tethers:      # (the published bend points are stamped into the record behind the call: stamp_bends)
            want["n_bend"] = rec[i]["n_bend"]; want["bend"] = rec[i]["bend"]
        assert com[i].tobytes() == want.tobytes(), ("the published record", lp.rounds, i)
        flown = bool(acc[i]) and not before["done"][i] and outcome[i] != abi.NEP_FLEET_SKIPPED
        cnt[s] += (1, 1, 1, 0) if flown else (1, 1, 0, 1)
        if not flown:
            assert outcome[i] != abi.NEP_FLEET_ACCEPTED
            continue
        assert outcome[i] == abi.NEP_FLEET_ACCEPTED, (lp.rounds, i, outcome[i])
        ns = int(sol[i]["n_states"])
        assert ns >= 1 and plans[i][-ns:].tobytes() == states[i, :ns].tobytes(), ("the ring holds the guess's states", lp.rounds, i)
        new = plan.make_pwp(np.array(sol[i]["times"])[: K + 1], np.array(sol[i]["coeff"])[:, :K, :])
        if before["flown"][i]:
            new = plan.compose_exact(float(before["t_now"][s]), abi.nep_pwp.from_buffer_copy(before["pwp"][i].tobytes()), new)
        times, coeff = plan.pwp_arrays(new)
        got = fs["pwp"][i]
        assert int(got["n_seg"]) == new.n_seg and got["times"][: new.n_seg + 1].tobytes() == times.tobytes()
        assert np.ascontiguousarray(got["coeff"][:, : new.n_seg]).tobytes() == coeff.tobytes(), ("the composition of the guess", lp.rounds, i)
    seen["count"] = seen["count"] + cnt
    seen["per_round"].append(cnt.copy())


def _flight(graph, rounds=ROUNDS, tick=TICK, snapshots=False, **kw):
    from neptune_amd.loop import DeviceFleetLoop
    lp = DeviceFleetLoop(list(_fleet()), graph=graph, trace=True, **kw)
    rows, seen, before = [], dict(count=np.zeros((lp.S, 4), dtype=np.int64), per_round=[], gated=0), {}
    try:
        if tick:
            lp.be.set_max_runtime(tick)
        if not graph and lp.fly_guess:
            lp.after_commit = lambda lp: _rules(lp, before, seen)
        for _ in range(rounds):
            if not graph and lp.fly_guess:
                before.update(_before(lp))
            lp.round()
            fp = tr.fingerprint(lp)
            if snapshots:
                fp["snapshot"] = lp.be.fleet_snapshot().cpu().numpy().tobytes()
            rows.append(fp)
        lp.be.check()
        assert (lp._g is not None) == graph
        return rows, lp.trace, lp.report(), seen, lp.be.fleet_snapshot_bytes()
    finally:
        lp.close()


@functools.lru_cache(maxsize=None)
def _eager():
    return _flight(False, fly_guess=True)


def _counts(rep):
    return [[d[k] for k in COUNTS] for d in rep]


def test_in_flight_rules_and_counts(torch):
    """2 scenes of 8 + 4, 20 rounds under a time limit of one clock tick on the loop's default solve path (the line presolve at 4 m:
    the replans its zero-iteration certificate finishes succeed, every other one fails and publishes its guess).  The counts are the
    sums over the rounds; guesses are flown; and the same flight without the option accepts fewer replans by at least as many."""
    rows, trace, rep, seen, _ = _eager()
    cnt = seen["count"]
    print("counts per scene", cnt.tolist(), "report", _counts(rep))
    assert _counts(rep) == cnt.tolist()
    for d in rep:
        assert d["guess_published"] == d["guess_flown"] + d["guess_not_flown"] and d["qp_failed"] == 0
    flown = sum(d["guess_flown"] for d in rep)
    _, _, rep_off, _, _ = _flight(True, fly_guess=False)
    accepted_on, accepted_off = sum(d["accepted"] for d in rep), sum(d["accepted"] for d in rep_off)
    print("guess_flown", flown, "accepted with", accepted_on, "without", accepted_off, "qp_failed without", sum(d["qp_failed"] for d in rep_off))
    assert flown > 0
    assert accepted_off <= accepted_on - flown
    assert all(k not in rep_off[0] for k in COUNTS)


def test_graph_equals_eager(torch):
    want, trace_w, rep_w, _, bytes_w = _eager()
    got, trace_g, rep_g, _, bytes_g = _flight(True, fly_guess=True)
    assert trace_g == trace_w
    for r in range(ROUNDS):
        tr.same(got[r], want[r], ("round", r))
    assert _counts(rep_g) == _counts(rep_w) and bytes_g == bytes_w


def test_scene_0_equals_fleet_loop(torch):
    from neptune_amd.loop import FleetLoop
    sc = _fleet()[0]
    host = FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), fly_guess=True)
    host.trace = []
    try:
        host.be.set_max_runtime(TICK)
        for _ in range(ROUNDS):
            host.round()
        h_state, h_stats = host.state.copy(), dict(host.stats)
    finally:
        host.close()
    rows, dev_trace, rep, _, _ = _eager()
    N = sc["par"].num_agents
    trace, t = [], 0.0
    for row in dev_trace:
        for a, (oc, K, fe, qp) in enumerate(row[:N]):
            if oc != abi.NEP_FLEET_SKIPPED:      # (an arrived agent: solved and dropped on the device, no entry on the host)
                trace.append((t, a, abi.FLEET_OUTCOMES[oc], K, fe, qp))
        for _ in range(5):
            t += sc["par"].dc
    first = next((k for k, (x, y) in enumerate(zip(trace, host.trace)) if x != y), None)
    assert first is None and len(trace) == len(host.trace), (first, trace[first] if first is not None else None, host.trace[first] if first is not None else None)
    assert any(e[5] == abi.NEP_GUESS and e[2] == "accepted" for e in host.trace)
    assert np.frombuffer(rows[-1]["fleet_state"], dtype=np.float64).reshape(-1, 12)[:N].tobytes() == h_state.tobytes()
    assert [h_stats[k] for k in COUNTS] == [rep[0][k] for k in COUNTS] and h_stats["guess_flown"] > 0


def test_recorder_rewind_and_checkpoint(torch, tmp_path):
    """the rule keeps no state: a snapshot is as large as without it, a rewound scene continues byte for byte, a checkpoint carries
    the option and the counts, and a file from before the option resumes without"""
    from neptune_amd.loop import DeviceFleetLoop
    scenes = list(_fleet())
    plain = DeviceFleetLoop(scenes, graph=False)
    try:
        want_bytes = plain.be.fleet_snapshot_bytes()
    finally:
        plain.close()
    lp = DeviceFleetLoop(scenes, graph=False, recorder=8, fly_guess=True)
    path, old = str(tmp_path / "flight.npz"), str(tmp_path / "old.npz")
    try:
        lp.be.set_max_runtime(TICK)
        assert lp.be.fleet_snapshot_bytes() == want_bytes
        batch, whole = [], []
        for r in range(12):
            if r == 6:
                lp.save_checkpoint(path)
                mid = _counts(lp.report())
            lp.round()
            batch.append(tr.fingerprint(lp, 1)); whole.append(tr.fingerprint(lp))
        final = _counts(lp.report())
        assert sum(m[2] for m in mid) > 0 and sum(m[2] for m in final) > sum(m[2] for m in mid)      # guesses flown before and after the cut
        one = lp.rewind(1, 7)
        try:
            assert one.fly_guess and one.S == 1 and one.d_guess_count is not None
            one.be.set_max_runtime(TICK)
            for r in range(7, 12):
                one.round()
                tr.same(tr.fingerprint(one), batch[r], ("scene 1 alone", r))
        finally:
            one.close()
    finally:
        lp.close()
    with pytest.raises(ValueError):
        DeviceFleetLoop.resume(path, scenes, graph=False, fly_guess=False)
    with pytest.raises(ValueError):
        DeviceFleetLoop.resume(path, scenes, graph=False, fly_guess=1)
    lp2 = DeviceFleetLoop.resume(path, scenes, graph=False, fly_guess=True)
    try:
        lp2.be.set_max_runtime(TICK)
        assert lp2.fly_guess and lp2.rounds == 6 and _counts(lp2.report()) == mid      # the counts travelled
        for r in range(6, 12):
            lp2.round()
            tr.same(tr.fingerprint(lp2), whole[r], ("resumed", r))
        assert _counts(lp2.report()) == final
    finally:
        lp2.close()
    with np.load(path, allow_pickle=False) as z:
        data = {k: z[k] for k in z.files if k != "guess_count"}
    opts = json.loads(str(data["options"]))
    del opts["fly_guess"]
    data["options"] = np.array(json.dumps(opts))
    np.savez(old, **data)
    lp3 = DeviceFleetLoop.resume(old, scenes, graph=False)
    try:
        assert lp3.fly_guess is False and lp3.d_guess_count is None and "guess_flown" not in lp3.report()[0]
    finally:
        lp3.close()


# ---- 5. nothing to do, nothing changed -------------------------------------------------------------------------------------------------
def test_without_failures_the_option_changes_nothing(torch):
    """the same two scenes (make_scene(8, 4, seed) for seeds 21 and 33) without the time limit, fly_guess on against off, snapshot by
    snapshot: equal until the first round whose trace shows a NEP_FAILED slot with a guess, which for these seeds is round 15 — not
    before round 10 — and from there on the option has something to publish"""
    on, trace_on, rep_on, _, _ = _flight(True, tick=0.0, snapshots=True, fly_guess=True)
    off, trace_off, rep_off, _, _ = _flight(True, tick=0.0, snapshots=True, fly_guess=False)
    failed = [r for r, row in enumerate(trace_off) if any(qp == abi.NEP_FAILED and K > 0 for (_, K, _, qp) in row)]
    first = failed[0] if failed else ROUNDS
    print("first round with a failed QP:", failed[:1], "counts with the option:", _counts(rep_on))
    assert failed and first >= 10
    assert sum(c[1] for c in _counts(rep_on)) > 0
    for r in range(first):
        tr.same(on[r], off[r], ("round", r))
        assert trace_on[r] == trace_off[r]


# ---- 6. the tethered round ---------------------------------------------------------------------------------------------------------------
def test_tethered_round_with_every_switch(torch):
    """astar_ent, move-back, the goal gate and fly_guess — the reference's benchmark yaml as written — for 10 rounds under the one-tick
    limit: the rules after every eager round (the records carry the stamped bend points), gated slots are never published, and the
    captured flight equals the eager one"""
    kw = dict(tethers=True, search="astar_ent", max_pops=40, moveback=mission.MoveBack(1.5, 1.0), goal_gate=True, fly_guess=True)
    want, trace_w, rep_w, seen, _ = _flight(False, rounds=10, **kw)
    cnt = seen["count"]
    print("tethered counts", cnt.tolist(), "gated slot-rounds", seen["gated"])
    assert _counts(rep_w) == cnt.tolist()
    assert cnt[:, 1].sum() > 0 and seen["gated"] > 0
    got, trace_g, rep_g, _, _ = _flight(True, rounds=10, **kw)
    assert trace_g == trace_w
    for r in range(10):
        tr.same(got[r], want[r], ("round", r))
    assert _counts(rep_g) == _counts(rep_w)
