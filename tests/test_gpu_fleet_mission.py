"""GPU: the mission controller of the device fleet loop (include/neptune_fleet.h "missions", neptune_amd.loop.DeviceFleetLoop's
missions=).  The kernel alone, fed with fabricated commits so that the ticks move, equals the host chain of nep_mission_step byte
for byte after every call — both modes, N = 70 (lanes stride, last chunk partial) and N = 5, five keep-outs of unequal vertex
counts, a draw that needs a second batch of 64 candidates, the no-goal path, the log's wrap; the same in flight behind the real
planner (also tethered); a captured graph flies what the eager calls fly; campaigns with the reference's timings keep their
accounts; and a loop without missions allocates and launches nothing of it."""
import functools
import math

import numpy as np
import pytest

import mission_ref as mr
from neptune_amd import abi, mission, scene
from neptune_amd._lib import BackendError

pytestmark = pytest.mark.gpu

PER_AGENT, RUNS = abi.NEP_MISSION_PER_AGENT, abi.NEP_MISSION_FLEET_RUNS
STATE_FIELDS = ("goal", "t_issue", "length", "completed", "counts", "sums", "scene", "t_run")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def compare(be, host, what):
    """goals, done, flags, every mission field and the log of the device against the host chain, byte for byte"""
    ms = be.fleet_mission_state(); fs = be.fleet_state(pwp=False)
    for f in STATE_FIELDS:
        assert ms[f].tobytes() == getattr(host, f).tobytes(), (what, f, ms[f], getattr(host, f))
    assert (fs["done"] == host.done).all(), (what, "done", fs["done"], host.done)
    assert (fs["flags"] == host.flags).all(), (what, "flags", fs["flags"], host.flags)
    log, n = be.fleet_mission_log(ordered=False)
    assert (n == host.log_n).all(), (what, "log_n", n, host.log_n)
    assert log.tobytes() == host.log[:, :log.shape[1]].tobytes(), (what, "log")


def tick_done(host, s_end, goal_radius):
    """nep_batch_fleet_tick's sticky arrival test on the state the round leaves, against the goals the mission call left"""
    for i in range(len(host.done)):
        dx, dy = float(s_end[i, 0]) - float(host.goal[i, 0]), float(s_end[i, 1]) - float(host.goal[i, 1])
        if math.sqrt(dx * dx + dy * dy) < goal_radius and math.sqrt(float(s_end[i, 3]) ** 2 + float(s_end[i, 4]) ** 2) < 0.05:
            host.done[i] = 1


class Alone:
    """fleet_init with hand-placed states and goals, then per call a fabricated accepted commit (T + 1 states per slot: the ticks
    about to be flown and one to stay on), fleet_mission, the comparison, fleet_tick.  No planner."""

    def __init__(self, torch, cfg, S, N, T, keep=None, pb=None, seed=0, goals=None, start=None):
        from neptune_amd.backend import BatchBackend
        self.torch, self.cfg, self.S, self.N, self.T = torch, cfg, S, N, T
        p = scene.scaled_params(N, 0)
        p.pb = np.ascontiguousarray(mr.circle_bases(N) if pb is None else pb, dtype=np.float64)
        self.p = p
        be = self.be = BatchBackend(p, [], n_scenes=S)
        n = S * N
        self.walk = mr.Walk(seed, S, N, T, goal_z=cfg.goal_z)
        if start is not None:
            self.walk.p[:] = start
        rng = np.random.default_rng(500 + seed)
        if goals is None:
            goals = np.zeros((n, 3)); goals[:, :2] = rng.uniform(-8.0, 8.0, (n, 2)); goals[:, 2] = cfg.goal_z
        lo = 6.5 * p.dc
        self.goal_radius = 0.2
        self.fcfg = abi.nep_fleet_cfg(p.dc, p.T_span, lo, lo, 0.0, 1.0, 6, 5, T, 0, self.goal_radius, 0.0)
        dev = be.device
        self.dt = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=t)
        state0 = np.zeros((n, 12)); state0[:, :3] = self.walk.p
        self.prev_end = state0.copy()
        if keep is not None:      # (before either init: the keep-outs survive both)
            for s in range(S):
                be.fleet_mission_keepout(s, keep[s])
        be.fleet_init(self.fcfg, self.dt(state0.reshape(-1), torch.float64), self.dt(np.asarray(goals).reshape(-1), torch.float64))
        be.fleet_mission_init(cfg)
        self.host = mission.HostMission(cfg, S, N, p.pb, goals, keepouts=keep)
        self.d_res = torch.zeros(n * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_acc = torch.ones(n, dtype=torch.int32, device=dev)
        self.d_outcome = torch.zeros(n, dtype=torch.int32, device=dev)
        self.t = np.zeros(S)
        self.calls = 0

    def call(self, pos_s_end=None):
        torch, be, n, T, N = self.torch, self.be, self.S * self.N, self.T, self.N
        before = self.walk.p.copy()
        pos, s_end = self.walk.call(self.host.goal) if pos_s_end is None else pos_s_end
        done = self.host.done != 0      # an arrived slot's commit is skipped (NEP_FLEET_SKIPPED): it stays on the one state its plan holds
        pos[done] = before[done][:, None, :]; s_end[done] = self.prev_end[done]; self.walk.p[done] = before[done]
        st = np.zeros((n, self.p.max_states, 12))
        st[:, :T, :3] = pos[:, 1:]; st[:, T - 1] = s_end; st[:, T] = s_end
        sol = np.zeros(n, dtype=abi.SOLUTION_DTYPE)
        sol["K"] = 1; sol["n_states"] = T + 1
        sol["times"][:, 0] = np.repeat(self.t, N); sol["times"][:, 1] = np.repeat(self.t, N) + 1.0
        sol["coeff"][:, :, 0, 3] = s_end[:, :3]
        be.d_solution.copy_(be.to_device(sol)); be.d_states.copy_(self.dt(st.reshape(-1), torch.float64))
        be.fleet_commit(self.d_res, self.d_acc, self.d_outcome)
        be.fleet_mission()
        assert (self.d_outcome.cpu().numpy() == np.where(done, abi.NEP_FLEET_SKIPPED, abi.NEP_FLEET_ACCEPTED)).all()
        self.prev_end = s_end.copy()
        self.host.step(pos, s_end, self.t, self.p.dc)
        compare(be, self.host, ("call", self.calls))
        be.fleet_tick()
        tick_done(self.host, s_end, self.goal_radius)
        assert (be.fleet_done() == self.host.done).all(), ("done after the tick", self.calls)
        for _ in range(T):
            self.t = self.t + self.p.dc
        self.calls += 1

    def close(self):
        self.be.close()


def _keepouts(S, seed=3):
    return mr.random_keepouts(np.random.default_rng(seed), S, 5)


@pytest.mark.parametrize("mode,N", [(PER_AGENT, 70), (PER_AGENT, 5), (RUNS, 70), (RUNS, 5)])
def test_kernel_alone_equals_host_chain(torch, mode, N):
    S, T = 3, 5
    keep = _keepouts(S)
    assert len({len(q) for q in keep[0]}) > 1      # unequal vertex counts
    if mode == PER_AGENT:
        cfg = mr.make_cfg(PER_AGENT, max_goals=3, log_cap=4, min_interval=0.5, timeout=2.0)
    else:
        cfg = mr.make_cfg(RUNS, max_goals=3, log_cap=2, min_interval=0.0, timeout=1.5, rest_v=0.0, rest_a=0.0, min_dist_self=0.0,
                          close_pos=0.5 if N == 70 else 0.75, close_goal=1.0 if N == 70 else 3.0)
    a = Alone(torch, cfg, S, N, T, keep=keep, seed=N + mode)
    try:
        for _ in range(30 if mode == PER_AGENT else 24):
            a.call()
        h = a.host
        if mode == PER_AGENT:
            assert h.counts[:, 1].sum() > 0 and h.counts[:, 2].sum() > 0 and (h.counts[:, 1] + h.counts[:, 2] == cfg.max_goals).any()
        else:
            assert h.scene[:, 2].sum() > 0 and h.scene[:, 3].all()      # failed runs; every scene's campaign over
        assert h.counts[:, 3].sum() == 0
        a.be.check()
    finally:
        a.close()


def test_kernel_alone_successful_run(torch):
    """mode FLEET_RUNS with every agent flown onto its goal: the run succeeds on the device as on the host"""
    cfg = mr.make_cfg(RUNS, max_goals=2, log_cap=2, timeout=50.0, min_dist_self=0.0, close_pos=0.5, close_goal=2.0)
    S, N, T = 2, 5, 2
    goals = np.array([[-4.0 + 2 * a, 1.0 + s, 1.0] for s in range(S) for a in range(N)])
    a = Alone(torch, cfg, S, N, T, goals=goals, start=goals + [3.0, 4.0, 0.0])
    try:
        for _ in range(2):
            g = a.host.goal.copy()
            pos = np.zeros((S * N, T + 1, 3)); pos[:, 0] = a.walk.p; pos[:, 1] = g + [0.0, 0.1, 0.0]; pos[:, 2] = g
            s_end = np.zeros((S * N, 12)); s_end[:, :3] = g
            a.walk.p[:] = g
            a.call((pos, s_end))
        assert a.host.scene.tolist() == [[2, 2, 0, 1]] * S
    finally:
        a.close()


def test_kernel_alone_second_batch_no_goal_and_wrap(torch):
    # a draw whose first accepted candidate has k >= 64: the wave goes into its second batch
    cfg, pb0, k_win = mr.second_batch_case()
    cfg.min_dist_self = 0.25
    N = 5
    pb = mr.circle_bases(N); pb[0] = pb0[0]
    goals = np.zeros((N, 3)); goals[:, 2] = cfg.goal_z; goals[0, :2] = pb0[0] + [20.0, 0.0]; goals[1:, :2] = 100.0
    start = goals.copy(); start[1:, :2] = -100.0      # agent 0 sits on its goal, the others are far from theirs
    a = Alone(torch, cfg, 1, N, 1, pb=pb, goals=goals, start=start)
    try:
        pos = np.repeat(start[:, None, :], 2, axis=1); s_end = np.zeros((N, 12)); s_end[:, :3] = start
        a.call((pos, s_end))
        assert a.host.log[0, 0]["attempts"] == k_win + 1 and tuple(a.host.goal[0, :2]) == mr.candidate(cfg, 0, 1, k_win)
        assert a.host.counts[:, 0].tolist() == [2, 1, 1, 1, 1]
        a.be.check()
    finally:
        a.close()
    # no candidate passes: the goal stays, the flags rise, nep_batch_check reports NEP_E_CAP (once: the flag is read and cleared)
    cfg = mr.make_cfg(PER_AGENT, max_goals=3, max_attempts=64, min_interval=0.0, min_dist_self=1.0, tether_max=1e-9, close_pos=0.0, close_goal=0.0, log_cap=4)
    pb = mr.circle_bases(N) + 50.0
    goals = np.zeros((N, 3)); goals[:, 2] = cfg.goal_z; goals[1:, :2] = 100.0
    start = goals.copy(); start[1:, :2] = -100.0
    a = Alone(torch, cfg, 1, N, 1, pb=pb, goals=goals, start=start)
    try:
        pos = np.repeat(start[:, None, :], 2, axis=1); s_end = np.zeros((N, 12)); s_end[:, :3] = start
        a.call((pos, s_end))
        assert a.host.flags.tolist() == [abi.NEP_FLEET_FLAG_GOAL, 0, 0, 0, 0] and a.host.counts[0].tolist() == [2, 1, 0, 1]
        assert a.host.goal[0].tolist() == [0.0, 0.0, cfg.goal_z]
        with pytest.raises(BackendError, match="-4"):
            a.be.check()
        a.be.check()
    finally:
        a.close()
    # log_cap = 2 under five legs
    cfg = mr.make_cfg(PER_AGENT, max_goals=6, log_cap=2, min_interval=0.0, min_dist_self=1.0, tether_max=0.0, close_pos=0.0, close_goal=0.0)
    a = Alone(torch, cfg, 1, N, 1, goals=goals, start=start)
    try:
        for _ in range(5):
            g = a.host.goal.copy(); g[1:] = start[1:]
            pos = np.repeat(g[:, None, :], 2, axis=1); pos[:, 0] = a.walk.p; s_end = np.zeros((N, 12)); s_end[:, :3] = g
            a.walk.p[:] = g
            a.call((pos, s_end))
        assert a.host.log_n[0] == 5 and sorted(int(r["index"]) for r in a.host.log[0]) == [3, 4]
        recs, n = a.be.fleet_mission_log()
        assert [int(r["index"]) for r in recs[0]] == [3, 4] and n[0] == 5
    finally:
        a.close()


# ---- in flight ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(n, m, seed):
    return scene.make_scene(n, m, seed=seed)


FLIGHTS = dict(agent=dict(spec=mission.MissionSpec("agent", goals=4, seed=3, min_interval=0.5, timeout=6.0, min_dist_self=3.0, log_cap=8), tethers=False),
               runs=dict(spec=mission.MissionSpec("runs", goals=4, seed=3, timeout=8.0, log_cap=8), tethers=False),
               tethered=dict(spec=mission.MissionSpec("agent", goals=4, seed=4, min_interval=0.5, timeout=6.0, min_dist_self=3.0, log_cap=8), tethers=True))
ROUNDS = 80


def _snapshot(lp):
    be = lp.be
    ms = be.fleet_mission_state(); fs = be.fleet_state(pwp=True); log, n = be.fleet_mission_log(ordered=False)
    cnt, t_now, rnd = be.fleet_counters()
    out = {k: v.tobytes() for k, v in ms.items()}
    out.update({"fleet_" + k: v.tobytes() for k, v in fs.items()})
    out.update(log=log.tobytes(), log_n=n.tobytes(), counters=cnt.tobytes(), t_now=t_now.tobytes(), rounds=rnd.tobytes(),
               plans=b"".join(p.tobytes() for p in be.fleet_plans()))
    if lp.tethers:
        out["ent"] = be.fleet_ent_state()["state"].tobytes()
    return out, ms


def _fly(name, graph):
    from neptune_amd.loop import DeviceFleetLoop
    f = FLIGHTS[name]
    scenes = [_scene(8, 4, 11), _scene(8, 4, 12)]
    lp = DeviceFleetLoop(scenes, beam_width=32, graph=graph, missions=f["spec"], tethers=f["tethers"])
    try:
        if graph:
            for _ in range(ROUNDS):
                lp.round()
            return _snapshot(lp)
        S, N, T, p = lp.S, lp.N, lp.replan_every, lp.p
        keep = [scene.keepout_polygons(sc) for sc in scenes] if mission.uses_keepouts(f["spec"]) else None
        host = mission.HostMission(lp.mission_cfg, S, N, p.pb, lp.goals.reshape(-1, 3), keepouts=keep)

        def after_mission(lp):
            be = lp.be
            got = lp.d_start.cpu().numpy().view(abi.FE_START_DTYPE)["goal"]
            assert got.tobytes() == host.goal.tobytes(), ("the select publishes the goals the last mission call left", lp.rounds)
            plans = be.fleet_plans(); st = be.fleet_state(pwp=False)["state"]
            _, t_now, _ = be.fleet_counters()
            pos = np.zeros((S * N, T + 1, 3)); s_end = np.zeros((S * N, 12))
            for i in range(S * N):
                pos[i, 0] = st[i, :3]
                for q in range(1, T + 1):
                    pos[i, q] = plans[i][min(q - 1, len(plans[i]) - 1), :3]
                s_end[i] = plans[i][min(T - 1, len(plans[i]) - 1)]
            host.step(pos, s_end, t_now, p.dc)
            compare(be, host, (name, lp.rounds))
            tick_done(host, s_end, lp.cfg.goal_radius)
        lp.after_mission = after_mission
        for _ in range(ROUNDS):
            lp.round()
        assert (lp.be.fleet_done() == host.done).all()
        return _snapshot(lp)
    finally:
        lp.close()


@functools.lru_cache(maxsize=None)
def _eager(name):
    return _fly(name, False)


@pytest.mark.parametrize("name", ["agent", "runs", "tethered"])
def test_in_flight_equals_host_chain(torch, name):
    _, ms = _eager(name)
    c = ms["counts"]
    print(name, "issued/reached/timed out/no goal:", c.sum(axis=0).tolist(), "scenes:", ms["scene"].tolist())
    if FLIGHTS[name]["spec"].mode == "agent":
        assert c[:, 1].sum() >= 2 and c[:, 2].sum() >= 2      # several legs end both ways
    else:
        assert ms["scene"][:, 0].sum() >= 2                    # runs ended
    assert c[:, 3].sum() == 0
    assert (c[:, 0] >= c[:, 1] + c[:, 2]).all() and (c[:, 0] <= c[:, 1] + c[:, 2] + 1).all()


@pytest.mark.parametrize("name", ["agent", "runs", "tethered"])
def test_graph_equals_eager(torch, name):
    want, _ = _eager(name)
    got, _ = _fly(name, True)
    for k in want:
        assert got[k] == want[k], (name, k)


def _campaign(scenes, spec, audit):
    from neptune_amd.loop import DeviceFleetLoop
    lp = DeviceFleetLoop(scenes, beam_width=32, audit=audit, missions=spec)
    try:
        c = lp.mission_cfg
        round_dt = lp.replan_every * lp.p.dc
        allowed = spec.goals * (int(math.ceil(c.timeout / round_dt)) + 1)      # a leg (run) ends at the first round end past its timeout
        rep = lp.run(max_rounds=allowed)
        lp.be.check()
        ms = lp.be.fleet_mission_state()
        return lp.rounds, allowed, rep, ms, lp.be.fleet_mission_log()
    finally:
        lp.close()


def test_campaign_per_agent_reference_timings(torch):
    """4 scenes of 16 + 8, autoCMD's own timings, 2 goals per agent, audit on.  Reported, not asserted: min_box_clear and the share
    of legs reached."""
    spec = mission.MissionSpec("agent", goals=2, seed=1)
    scenes = [_scene(16, 8, 21 + s) for s in range(4)]
    rounds, allowed, rep, ms, (log, n) = _campaign(scenes, spec, audit=True)
    c = ms["counts"].reshape(4, 16, 4)
    ended = c[..., 1] + c[..., 2]
    for s in range(4):
        m = rep[s]["mission"]
        print("scene", s, "rounds", rounds, "of", allowed, m, "min_box_clear", rep[s]["audit"]["min_box_clear"], "min_static_dist", rep[s]["min_static_dist"])
    assert (c[..., 3] == 0).all()
    assert (c[..., 0] == ended + (ended < spec.goals)).all()      # issued = reached + timed out + open legs
    assert (n == ended.reshape(-1)).all() and all(len(r) == e for r, e in zip(log, ended.reshape(-1)))
    assert ms["scene"][:, 3].all() and (ended == spec.goals).all(), (rounds, allowed, ended)
    for s in range(4):
        assert rep[s]["min_static_dist"] >= -1e-6
        m = rep[s]["mission"]
        assert m["legs_reached"] + m["legs_timed_out"] == 32 and m["finished"]


def test_campaign_fleet_runs_reference_timings(torch):
    spec = mission.MissionSpec("runs", goals=3, seed=1)
    scenes = [_scene(8, 4, 31 + s) for s in range(2)]
    rounds, allowed, rep, ms, (log, n) = _campaign(scenes, spec, audit=True)
    c = ms["counts"].reshape(2, 8, 4)
    for s in range(2):
        print("scene", s, "rounds", rounds, "of", allowed, rep[s]["mission"], "min_box_clear", rep[s]["audit"]["min_box_clear"])
        assert ms["scene"][s, 0] == 3 == ms["scene"][s, 1] + ms["scene"][s, 2] and ms["scene"][s, 3] == 1
        assert n[s] == 3 and [int(r["index"]) for r in log[s]] == [0, 1, 2]
        assert rep[s]["min_static_dist"] >= -1e-6
    assert (c[..., 3] == 0).all() and (c[..., 0] == 3).all() and (c[..., 1] + c[..., 2] == 3).all()


def test_unchanged_without_missions(torch):
    """a loop without missions has no mission state — its fleet_mission and the readers are refused — until
    nep_batch_fleet_mission_init allocates it; the init's and the keep-outs' contracts"""
    from neptune_amd.loop import DeviceFleetLoop
    from neptune_amd._lib import lib
    import ctypes as C
    scenes = [_scene(8, 4, 11)]
    lp = DeviceFleetLoop(scenes, beam_width=32)
    try:
        assert lp.missions is None and lp.after_mission is None
        L = lib()
        assert L.nep_batch_fleet_mission(lp.be._h, None) == -2                                        # NEP_E_STATE
        assert L.nep_batch_fleet_mission_state(lp.be._h, None, None, None, None, None, None, None, None) == -2
        assert L.nep_batch_fleet_mission_log(lp.be._h, None, None) == -2
        for _ in range(3):
            lp.round()
        assert L.nep_batch_fleet_mission(lp.be._h, None) == -2
        dev0, dev1, pin = C.c_int64(), C.c_int64(), C.c_int64()
        # bad configurations and the init contract, on the same handle
        cfg = mission.mission_cfg(mission.MissionSpec("agent"), lp.p)
        bad = mission.mission_cfg(mission.MissionSpec("agent", min_dist_self=lp.cfg.goal_radius), lp.p)
        assert L.nep_batch_fleet_mission_init(lp.be._h, C.byref(bad), None) == -1                     # NEP_E_ARG: min_dist_self <= goal_radius
        bad = mission.mission_cfg(mission.MissionSpec("agent", max_attempts=100), lp.p)
        assert L.nep_batch_fleet_mission_init(lp.be._h, C.byref(bad), None) == -1
        tri = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
        assert L.nep_batch_fleet_mission_keepout(lp.be._h, 1, 0, None, None) == -1                    # no such scene
        with pytest.raises(BackendError):      # not convex
            lp.be.fleet_mission_keepout(0, [np.array([[0.0, 0.0], [2.0, 0.0], [0.5, 0.5], [0.0, 2.0]])])
        with pytest.raises(BackendError, match="-4"):
            lp.be.fleet_mission_keepout(0, [tri] * (abi.NEP_MISSION_MAX_POLY + 1))
        lp.be.fleet_mission_keepout(0, [tri[::-1]])      # clockwise: reversed, accepted
        L.nep_debug_live_bytes(C.byref(dev0), C.byref(pin))
        lp.be.fleet_mission_init(cfg)
        L.nep_debug_live_bytes(C.byref(dev1), C.byref(pin))
        assert dev1.value > dev0.value      # (only now does mission state exist)
        lp.be.fleet_mission()
        lp.be.check()
        assert lp.be.fleet_mission_state()["counts"][:, 0].tolist() == [1] * 8
    finally:
        lp.close()


def test_init_contracts_state_and_cap(torch):
    """nep_batch_fleet_mission_init without fleet state: NEP_E_STATE.  One agent more than the LDS carve holds next to a full keep-out
    set (1 098): NEP_E_CAP; the largest handle that fits (1 097 agents, NEP_MISSION_MAX_POLY polygons of NEP_MISSION_MAX_VERT vertices
    in all, uploaded partly before and partly after the init) equals the host chain."""
    import ctypes as C
    from neptune_amd._lib import lib
    from neptune_amd.backend import BatchBackend
    L = lib()
    cfg = mr.make_cfg(PER_AGENT, max_goals=3, log_cap=2, min_interval=0.0, timeout=0.2, min_dist_self=1.0, close_pos=0.0, close_goal=0.25)
    tri = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    p = scene.scaled_params(5, 0)
    be = BatchBackend(p, [], n_scenes=1)
    try:
        be.fleet_mission_keepout(0, [tri])                                                            # callable before either init
        assert L.nep_batch_fleet_mission_init(be._h, C.byref(cfg), None) == -2                        # NEP_E_STATE: no fleet state
        assert L.nep_batch_fleet_mission(be._h, None) == -2
    finally:
        be.close()
    N = 1098
    p = scene.scaled_params(N, 0)
    be = BatchBackend(p, [], n_scenes=1)
    try:
        z = torch.zeros(N * 12, dtype=torch.float64, device=be.device)
        be.fleet_init(abi.nep_fleet_cfg(p.dc, p.T_span, 6.5 * p.dc, 6.5 * p.dc, 0.0, 1.0, 6, 5, 1, 0, 0.2, 0.0), z, z[:N * 3])
        assert L.nep_batch_fleet_mission_init(be._h, C.byref(cfg), None) == -4                        # NEP_E_CAP
        assert L.nep_batch_fleet_mission(be._h, None) == -2                                           # (and no mission state came of it)
    finally:
        be.close()
    # the largest carve: 64 octagons = 512 vertices; the first half of them staged before the init, all of them after it
    rng = np.random.default_rng(9)
    th = 2 * np.pi * np.arange(8) / 8
    polys = [np.stack([cx + 0.3 * np.cos(th), cy + 0.3 * np.sin(th)], axis=1) for cx, cy in rng.uniform(-8.0, 8.0, (abi.NEP_MISSION_MAX_POLY, 2))]
    assert sum(len(q) for q in polys) == abi.NEP_MISSION_MAX_VERT
    a = Alone(torch, cfg, 1, N - 1, 1, keep=[polys[:32]], seed=2)
    try:
        a.call()
        a.be.fleet_mission_keepout(0, polys)
        a.host = _with_keepouts(a.host, [polys])
        for _ in range(3):
            a.call()
        with pytest.raises(BackendError, match="-4"):
            a.be.fleet_mission_keepout(0, polys + [tri])                                             # a 65th polygon
        assert a.host.counts[:, 1].sum() + a.host.counts[:, 2].sum() > 100 and a.host.counts[:, 3].sum() == 0
        a.be.check()
    finally:
        a.close()


def _with_keepouts(host, keep):
    """the same host chain with another keep-out set (what nep_batch_fleet_mission_keepout does to the handle between rounds)"""
    new = mission.HostMission(host.cfg, host.S, host.N, host.pb, host.goal, keepouts=keep)
    for f in mr.FIELDS:
        getattr(new, f)[...] = getattr(host, f)
    return new
