"""GPU: scripted goals, mission mode NEP_MISSION_FLEET_TOGETHER and the effort record (include/neptune_fleet.h).
(1) the mission kernel alone, fed with fabricated commits, equals the host chain of nep_mission_step_script byte for byte with a
script of 1, 2 and 3 rows in each mode, 1, 64 and 70 agents per scene; (2) a script switched off flies what a handle that never saw
one flies; (3) a captured round replays the eager bytes, honours a table replaced between replays, allocates nothing, and a table
beyond the capacity is refused; (4) snapshots keep their size and version, a rewind and a resumed checkpoint continue byte for byte,
a checkpoint from before the options resumes without them; (5) nep_batch_fleet_effort equals the host chain of nep_effort_step,
eager and captured, and disturbs nothing; (6) a position exchange of 8 agents."""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest

import mission_ref as mr
import mission_script_ref as msr
from neptune_amd import abi, mission, scene
from neptune_amd._lib import BackendError, lib
from test_gpu_fleet_mission import Alone, compare, tick_done

pytestmark = pytest.mark.gpu

PER_AGENT, RUNS, TOGETHER = abi.NEP_MISSION_PER_AGENT, abi.NEP_MISSION_FLEET_RUNS, 3


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _cfg(mode, max_goals):
    if mode == PER_AGENT:
        return mr.make_cfg(PER_AGENT, max_goals=max_goals, log_cap=4, min_interval=0.5, timeout=2.0)
    return mr.make_cfg(mode, max_goals=max_goals, log_cap=2, min_interval=0.0, timeout=1.5, rest_v=0.0, rest_a=0.0, min_dist_self=0.0, close_pos=0.5, close_goal=1.0)


class Scripted(Alone):
    """test_gpu_fleet_mission.Alone with a table of goals: uploaded to the handle and given to the host chain"""

    def __init__(self, torch, cfg, S, N, T, G, seed=0):
        super().__init__(torch, cfg, S, N, T, seed=seed)
        self.set_script(msr.random_script(np.random.default_rng(900 + seed), S * N, G) if G else None)

    def set_script(self, script):
        self.be.fleet_mission_script(script)
        new = mission.HostMission(self.cfg, self.S, self.N, self.p.pb, self.host.goal, script=script)
        for f in mr.FIELDS:
            getattr(new, f)[...] = getattr(self.host, f)
        self.host = new


# ---- (1) the kernel against the host chain ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,N,G", [(m, N, 1 + (i + j) % 3) for i, m in enumerate((PER_AGENT, RUNS, TOGETHER)) for j, N in enumerate((1, 64, 70))])
def test_kernel_alone_equals_host_chain_scripted(torch, mode, N, G):
    a = Scripted(torch, _cfg(mode, G + 3), 2, N, 5, G, seed=10 * mode + G)
    try:
        for _ in range(36):
            a.call()
        h = a.host
        assert (h.counts[:, 0] > G + 1).any()                                   # the table wrapped
        assert (h.log["attempts"] == 0).all() and h.counts[:, 3].sum() == 0 and (h.flags == 0).all()
        assert set(np.unique(h.goal[h.counts[:, 0] >= 2, 2])) <= set(np.unique(h.script[:, :, 2]))      # z from the table
        if mode != PER_AGENT:
            assert h.scene[:, 0].sum() >= 4                                     # runs ended (by their timeout, or with everybody completed)
        a.be.check()
    finally:
        a.close()


def test_kernel_alone_together_draws_without_script(torch):
    a = Scripted(torch, _cfg(TOGETHER, 4), 2, 5, 5, 0, seed=4)
    try:
        for _ in range(30):
            a.call()
        assert a.host.scene[:, 0].sum() >= 4 and a.host.log["attempts"].max() > 0
        a.be.check()
    finally:
        a.close()


# ---- (3) capture -------------------------------------------------------------------------------------------------------------------------
def _captured_call(a, g):
    """Alone.call with the three launches — fleet_commit, fleet_mission, fleet_tick — replayed from the graph g (None: eager)"""
    torch, be, n, T, N = a.torch, a.be, a.S * a.N, a.T, a.N
    before = a.walk.p.copy()
    pos, s_end = a.walk.call(a.host.goal)
    done = a.host.done != 0
    pos[done] = before[done][:, None, :]; s_end[done] = a.prev_end[done]; a.walk.p[done] = before[done]
    st = np.zeros((n, a.p.max_states, 12))
    st[:, :T, :3] = pos[:, 1:]; st[:, T - 1] = s_end; st[:, T] = s_end
    sol = np.zeros(n, dtype=abi.SOLUTION_DTYPE)
    sol["K"] = 1; sol["n_states"] = T + 1
    sol["times"][:, 0] = np.repeat(a.t, N); sol["times"][:, 1] = np.repeat(a.t, N) + 1.0
    sol["coeff"][:, :, 0, 3] = s_end[:, :3]
    be.d_solution.copy_(be.to_device(sol)); be.d_states.copy_(a.dt(st.reshape(-1), torch.float64))
    if g is None:
        be.fleet_commit(a.d_res, a.d_acc, a.d_outcome); be.fleet_mission(); be.fleet_tick()
    else:
        g.replay()
    a.prev_end = s_end.copy()
    a.host.step(pos, s_end, a.t, a.p.dc)
    tick_done(a.host, s_end, a.goal_radius)
    compare(be, a.host, ("captured" if g is not None else "eager", a.calls))
    for _ in range(T):
        a.t = a.t + a.p.dc
    a.calls += 1


@pytest.mark.parametrize("mode", [PER_AGENT, TOGETHER])
def test_captured_round_honours_a_replaced_table(torch, mode):
    L = lib()
    S, N, T = 2, 70, 5
    a = Scripted(torch, _cfg(mode, 9), S, N, T, 3, seed=21)
    try:
        for _ in range(2):
            _captured_call(a, None)
        torch.cuda.synchronize()
        dev0, dev1, pin = C.c_int64(), C.c_int64(), C.c_int64()
        L.nep_debug_live_bytes(C.byref(dev0), C.byref(pin))
        s = torch.cuda.Stream(a.be.device)
        s.wait_stream(torch.cuda.current_stream(a.be.device))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            g.capture_begin()
            a.be.fleet_commit(a.d_res, a.d_acc, a.d_outcome); a.be.fleet_mission(); a.be.fleet_tick()
            g.capture_end()
        torch.cuda.current_stream(a.be.device).wait_stream(s)
        # (the capture launched nothing: the state is what the two eager calls left)
        for _ in range(12):
            _captured_call(a, g)
        L.nep_debug_live_bytes(C.byref(dev1), C.byref(pin))
        assert dev1.value == dev0.value                                         # nothing was allocated by the captured calls
        issued = a.host.counts[:, 0].copy()
        # a shorter table with other goals, between two replays: the same graph takes its rows
        new = msr.random_script(np.random.default_rng(77), S * N, 2, z_lo=3.0, z_hi=4.0)
        a.set_script(new)
        for _ in range(14):
            _captured_call(a, g)
        fresh = a.host.counts[:, 0] > issued
        assert fresh.sum() > N // 2 and (a.host.goal[fresh, 2] >= 3.0).all()     # goals issued since then come from the new table
        # a table beyond the capacity the first upload allocated: refused, nothing changes
        with pytest.raises(BackendError, match="-4"):
            a.be.fleet_mission_script(msr.random_script(np.random.default_rng(1), S * N, 4))
        with pytest.raises(BackendError, match="-1"):
            bad = new.copy(); bad[-1, -1, -1] = np.inf
            a.be.fleet_mission_script(bad)
        for _ in range(3):
            _captured_call(a, g)
        # switched off between replays: the graph draws again
        a.set_script(None)
        for _ in range(8):
            _captured_call(a, g)
        assert a.host.log["attempts"].max() > 0
        L.nep_debug_live_bytes(C.byref(dev1), C.byref(pin))
        assert dev1.value == dev0.value
        a.be.check()
    finally:
        a.close()


def test_script_contracts(torch):
    """NEP_E_ARG for a bad length or a missing table; nothing to switch off allocates nothing; the table survives both inits"""
    L = lib()
    cfg = _cfg(PER_AGENT, 4)
    a = Alone(torch, cfg, 1, 5, 5, seed=3)
    try:
        dev0, dev1, pin = C.c_int64(), C.c_int64(), C.c_int64()
        L.nep_debug_live_bytes(C.byref(dev0), C.byref(pin))
        assert L.nep_batch_fleet_mission_script(a.be._h, -1, None) == -1
        assert L.nep_batch_fleet_mission_script(a.be._h, 2, None) == -1
        assert L.nep_batch_fleet_mission_script(a.be._h, 0, None) == 0
        L.nep_debug_live_bytes(C.byref(dev1), C.byref(pin))
        assert dev1.value == dev0.value
        script = msr.random_script(np.random.default_rng(5), 5, 2)
        a.be.fleet_mission_script(script)
        z = torch.zeros(5 * 12, dtype=torch.float64, device=a.be.device)
        a.be.fleet_init(a.fcfg, z, a.dt(a.host.goal.reshape(-1), torch.float64))      # re-seed: drops the mission state, keeps the table
        a.be.fleet_mission_init(cfg)
        a.host = mission.HostMission(cfg, 1, 5, a.p.pb, a.host.goal, script=script)
        a.walk.p[:] = 0.0; a.walk.p[:, 2] = 0.0; a.prev_end = np.zeros((5, 12)); a.t = np.zeros(1)
        for _ in range(20):
            a.call()
        assert (a.host.counts[:, 0] >= 2).any() and (a.host.log["attempts"] == 0).all()
    finally:
        a.close()


# ---- flights -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(n, m, seed):
    return scene.make_scene(n, m, seed=seed)


def _scenes():
    return [_scene(8, 4, 11), _scene(8, 4, 12)]


def _per_scene_script(G=3):
    """[2][8][G][3]: other goals in each scene, inside the world of 8 + 4, at the flight height"""
    rng = np.random.default_rng(31)
    p = _scene(8, 4, 11)["par"]
    g = np.zeros((2, 8, G, 3))
    g[..., :2] = rng.uniform(0.5 * p.x_min, 0.5 * p.x_max, (2, 8, G, 2)); g[..., 2] = p.goal_height
    return g


def _blob(lp):
    b = lp.be.fleet_snapshot()
    lp.torch.cuda.synchronize()
    return b.cpu().numpy().tobytes()


def _loop(**kw):
    from neptune_amd.loop import DeviceFleetLoop
    return DeviceFleetLoop(_scenes(), beam_width=32, **kw)


# ---- (2) script off --------------------------------------------------------------------------------------------------------------------------
def test_script_off_flies_the_unscripted_flight(torch):
    spec = mission.MissionSpec("runs", goals=4, seed=3, timeout=2.0, log_cap=8)
    plain = _loop(missions=spec)
    off = _loop(missions=spec)
    try:
        off.be.fleet_mission_script(_per_scene_script().reshape(16, 3, 3))      # a table is there ...
        off.be.fleet_mission_script(None)                                        # ... and switched off
        for r in range(24):
            plain.round(); off.round()
            assert _blob(plain) == _blob(off), r
        assert plain.be.fleet_mission_state()["scene"][:, 0].sum() >= 2          # runs ended and goals were drawn
        lg0, n0 = plain.be.fleet_mission_log(ordered=False); lg1, n1 = off.be.fleet_mission_log(ordered=False)
        assert lg0.tobytes() == lg1.tobytes() and (n0 == n1).all() and lg0["attempts"].max() > 0
    finally:
        plain.close(); off.close()


# ---- (4) snapshots ---------------------------------------------------------------------------------------------------------------------------
def test_snapshots_rewind_and_resume(torch, tmp_path):
    from neptune_amd.loop import DeviceFleetLoop
    script = _per_scene_script()
    spec = mission.MissionSpec("together", goals=6, seed=3, timeout=1.0, log_cap=8, script=script)
    plain = _loop(missions=dataclass_without_script(spec))
    lp = _loop(missions=spec, recorder=8, effort=True)
    try:
        # sizes and version as without a script
        assert lp.be.fleet_snapshot_bytes() == plain.be.fleet_snapshot_bytes()
        h0 = abi.nep_fleet_snapshot_hdr.from_buffer_copy(_blob(plain)[:80]); h1 = abi.nep_fleet_snapshot_hdr.from_buffer_copy(_blob(lp)[:80])
        assert h1.version == abi.NEP_SNAPSHOT_VERSION == 1 and h1.scene_bytes == h0.scene_bytes and h1.mission_mode == TOGETHER
        path = str(tmp_path / "mid.npz")
        for _ in range(7):
            lp.round()
        lp.save_checkpoint(path)
        for _ in range(7):
            lp.round()
        want, want_eff = _blob(lp), lp.effort_records().tobytes()
        ms = lp.be.fleet_mission_state()
        assert ms["scene"][:, 0].min() >= 2 and (ms["counts"][:, 0] >= 3).all()      # scripted goals were issued on both sides of the checkpoint
        assert (ms["goal"].reshape(2, 8, 3) == script[np.arange(2)[:, None], np.arange(8)[None, :], (ms["counts"][:, 0].reshape(2, 8) - 2) % 3]).all()
        # a resumed checkpoint continues byte for byte, effort records included
        re = DeviceFleetLoop.resume(path, _scenes())
        try:
            assert re.rounds == 7 and re.effort == 1e-6 and re.script.tobytes() == script.tobytes()
            for _ in range(7):
                re.round()
            assert _blob(re) == want and re.effort_records().tobytes() == want_eff
        finally:
            re.close()
        with pytest.raises(ValueError):
            DeviceFleetLoop.resume(path, _scenes(), effort=False)
        with pytest.raises(ValueError):
            DeviceFleetLoop.resume(path, _scenes(), missions=dataclass_without_script(spec))
        # a rewind flies scene 1 alone with scene 1's rows
        one = lp.rewind(1, 10)
        try:
            for _ in range(4):
                one.round()
            sb = h1.scene_bytes
            assert _blob(one)[80:80 + sb] == want[80 + sb:80 + 2 * sb]
            assert one.effort is not None and one.script.tobytes() == script[1:2].tobytes()
        finally:
            one.close()
        # a checkpoint from before the options: no "script", no "effort" among its options, no effort array — resumes without them
        for _ in range(5):
            plain.round()
        old = str(tmp_path / "old.npz")
        plain.save_checkpoint(old)
        with np.load(old, allow_pickle=False) as z:
            data = {k: z[k] for k in z.files}
        o = json.loads(str(data["options"]))
        assert o.pop("script") is None and o.pop("effort") is None and "effort" not in data
        data["options"] = np.array(json.dumps(o))
        with open(old, "wb") as f:
            np.savez(f, **data)
        for _ in range(5):
            plain.round()
        re = DeviceFleetLoop.resume(old, _scenes())
        try:
            assert re.script is None and re.d_effort is None
            for _ in range(5):
                re.round()
            assert _blob(re) == _blob(plain)
        finally:
            re.close()
    finally:
        plain.close(); lp.close()


def dataclass_without_script(spec):
    import dataclasses
    return dataclasses.replace(spec, script=None)


# ---- (5) the effort record against the host chain ----------------------------------------------------------------------------------------------
EFFORT_SPEC = mission.MissionSpec("agent", goals=4, seed=3, min_interval=0.5, timeout=6.0, min_dist_self=3.0, log_cap=8)
EFFORT_ROUNDS = 20


def _effort_flight(graph, effort):
    lp = _loop(missions=EFFORT_SPEC, graph=graph, effort=effort)
    try:
        host = msr.new_effort(lp.S * lp.N); ref = msr.new_effort(lp.S * lp.N)
        p, T = lp.p, lp.replan_every
        if not graph:
            def after_mission(lp):      # the state the effort kernel is about to read: plans as the commit left them, done as the mission left it
                plans = lp.be.fleet_plans(); done = lp.be.fleet_done()
                for i in range(lp.S * lp.N):
                    mission.effort_step(p.v_max, p.a_max, p.j_max, p.dc, T, plans[i], 0, len(plans[i]), done[i], lp.effort, host[i:i + 1])
                    msr.effort_ref(p.v_max, p.a_max, p.j_max, p.dc, T, plans[i], 0, len(plans[i]), done[i], lp.effort, ref[i:i + 1])
            if effort:
                lp.after_mission = after_mission
        for r in range(EFFORT_ROUNDS):
            lp.round()
            if effort and not graph:
                got = lp.effort_records()
                assert got.tobytes() == host.tobytes(), (r, got, host)
        return _blob(lp), lp.effort_records() if effort else None, host, ref, lp.be.fleet_done()
    finally:
        lp.close()


def test_effort_equals_host_chain_and_disturbs_nothing(torch):
    blob_e, eff_e, host, ref, done = _effort_flight(False, True)
    assert host.tobytes() == ref.tobytes()                                       # (the host form against the restatement, on flown states)
    n = eff_e["n_ticks"]
    assert n.sum() > 0 and n.max() <= EFFORT_ROUNDS * 5 and (eff_e["jerk_sum"] > 0).sum() >= 8 and (eff_e["max_v"].max(axis=1) > 0.5).any()
    print("effort of 2 x (8 + 4), %d rounds: counted ticks %s, max |v| %.9f |a| %.9f |j| %.9f, violations v %d a %d j %d" % (
        EFFORT_ROUNDS, n.tolist(), eff_e["max_v"].max(), eff_e["max_a"].max(), eff_e["max_j"].max(), eff_e["n_v_viol"].sum(), eff_e["n_a_viol"].sum(),
        eff_e["n_j_viol"].sum()))
    blob_g, eff_g, _, _, _ = _effort_flight(True, True)
    assert eff_g.tobytes() == eff_e.tobytes() and blob_g == blob_e               # captured = eager
    blob_n, _, _, _, _ = _effort_flight(True, False)
    assert blob_n == blob_e                                                      # with and without the call: the same fleet


def test_effort_contracts(torch):
    L = lib()
    lp = _loop(effort=0.5)
    try:
        assert lp.effort == 0.5 and lp.d_effort.numel() == 16 * 96
        h = lp.be._h
        assert L.nep_batch_fleet_effort(h, 5.0, -1e-9, lp.d_effort.data_ptr(), None) == -1
        assert L.nep_batch_fleet_effort(h, 5.0, math.nan, lp.d_effort.data_ptr(), None) == -1
        assert L.nep_batch_fleet_effort(h, 0.0, 0.0, lp.d_effort.data_ptr(), None) == -1
        assert L.nep_batch_fleet_effort(h, 5.0, 0.0, None, None) == -1
        lp.round()
        rep = lp.report()
        for k in ("jerk_sum_mean", "max_v", "max_a", "max_j", "v_viol", "a_viol", "j_viol"):
            assert k in rep[0] and "longest_leg_time" not in rep[0]
    finally:
        lp.close()
    from neptune_amd.backend import BatchBackend
    p = scene.scaled_params(5, 0)
    be = BatchBackend(p, [], n_scenes=1)
    try:
        d = be.new_effort()
        assert L.nep_batch_fleet_effort(be._h, 5.0, 0.0, d.data_ptr(), None) == -2      # NEP_E_STATE: no fleet state
    finally:
        be.close()


# ---- (6) a position exchange -------------------------------------------------------------------------------------------------------------------
def test_exchange_of_eight(torch):
    """8 + 0, mode "together", auto_commands_together.py's two lists, 2 legs: the hop onto the circle, then the exchange proper —
    everybody through the middle at once.

    Measured on an MI355X: both runs succeed in 87 rounds of the 482 allowed (longest run 18.5 s, mean leg
    12.46 m, mean jerk integral 24.14).  max |v| = 1.999924627 (75 um/s BELOW v_max = 2), max |a| = 2.999999999999994 (below a_max =
    3): both inside the 1e-6 bar, no tick beyond it.  max |j| = 8.272425299, 3.27 ABOVE j_max = 5, on 45 of the 3 310 counted ticks: a
    flown violation of the yaml's j_max, and the reference's too — its QP has velocity and acceleration rows and no jerk row
    (solver_gurobi_poly.cpp stores j_max and never uses it; the lattice of the search is the only place it acts), so an optimised
    trajectory is held to j_max by nothing.  What does bound it: acceleration is linear over an interval of T_span and within
    +-a_max at both ends, so |j| <= 2 a_max / T_span = 12 per component.  That is the bound asserted for the jerk; velocity and
    acceleration are asserted at the limits plus 1e-6."""
    from neptune_amd.loop import DeviceFleetLoop
    sc = _scene(8, 0, 5)
    p = sc["par"]
    script = mission.exchange_script(8, z=p.goal_height)
    spec = mission.MissionSpec("together", goals=2, script=script, timeout=60.0, log_cap=4)
    lp = DeviceFleetLoop([sc], beam_width=32, missions=spec, goals=[script[:, -1]], effort=True)
    try:
        budget = 2 * (int(math.ceil(60.0 / (lp.replan_every * p.dc))) + 1)      # a run ends at the first round end past its timeout
        rep = lp.run(max_rounds=budget)[0]
        print("exchange of 8:", lp.rounds, "rounds of", budget, json.dumps({k: v for k, v in rep.items() if k != "audit"}))
        assert rep["mission"]["finished"] and rep["mission"]["runs"] == 2 and lp.rounds <= budget
        for k in ("jerk_sum_mean", "max_v", "max_a", "max_j", "v_viol", "a_viol", "j_viol", "longest_leg_time"):
            assert k in rep, k
        assert rep["jerk_sum_mean"] > 0.0 and 0.0 < rep["longest_leg_time"] <= 60.0 + lp.replan_every * p.dc
        print("excess over the limits: v %.3e a %.3e j %.3e" % (rep["max_v"] - p.v_max, rep["max_a"] - p.a_max, rep["max_j"] - p.j_max))
        assert rep["max_v"] <= p.v_max + EXCESS and rep["max_a"] <= p.a_max + EXCESS and rep["v_viol"] == 0 and rep["a_viol"] == 0      # (effort=True: slack 1e-6)
        assert rep["max_j"] <= 2.0 * p.a_max / p.T_span + EXCESS                  # (not j_max: see above; j_viol counts the ticks beyond j_max)
        assert rep["j_viol"] <= rep["effort_ticks"]
        g = lp.be.fleet_mission_state()["goal"]
        assert g.tobytes() == script[:, 0].tobytes()                             # leg 1 is goals1, the list the driver publishes first
    finally:
        lp.close()


EXCESS = 1e-6      # the flight-audit tests' bar
