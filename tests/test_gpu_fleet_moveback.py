"""GPU: the move-back rule of the device fleet loop (include/neptune_fleet.h "move-back", neptune_amd.loop.DeviceFleetLoop's
moveback=).  The kernel alone equals the host form nep_moveback_step byte for byte after every call, with the reference's outcomes
(tests/moveback_ref.py) asserted next to it; with missions (fabricated commits, both modes) a new goal raises the bit in the next
round and the device equals the host chain nep_mission_step + nep_moveback_step; in flight behind the real planner a captured
graph flies what the eager calls fly and one scene flies what FleetLoop(moveback=) flies; tethered runs; the recorder carries a
move-back in progress; the contracts."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import mission_ref as mr
import moveback_ref as ref
import test_gpu_fleet_mission as tm
import test_gpu_fleet_recorder as tr
from neptune_amd import abi, mission, scene

pytestmark = pytest.mark.gpu

WB = abi.NEP_FLEET_FLAG_WAY_BACK
PER_AGENT, RUNS = abi.NEP_MISSION_PER_AGENT, abi.NEP_MISSION_FLEET_RUNS


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@functools.lru_cache(maxsize=None)
def _scene(n, m, seed):
    return scene.make_scene(n, m, seed=seed)


def _starts(t):
    return t.cpu().numpy().view(abi.FE_START_DTYPE).copy()


def host_moveback(cfg, S, N, state, pb, t_issue, t_first, t_now, flags, start):
    """nep_moveback_step scene by scene, in place on flags [S*N] and start [S*N]; the reference's events per slot"""
    events = []
    for s in range(S):
        sl = slice(s * N, (s + 1) * N)
        ti = None if t_issue is None else t_issue[sl]
        rf, rg, ev = ref.step(cfg.radius, cfg.timeout, state[sl], pb, ti, t_first, float(t_now[s]), flags[sl], start["goal"][sl])
        mission.moveback_step(cfg, state[sl], pb, ti, t_first, float(t_now[s]), flags[sl], start[sl])
        assert flags[sl].tolist() == rf and start["goal"][sl].tobytes() == np.array(rg).tobytes(), ("the host form against the reference", s)
        events += ev
    return events


# ---- 1. the kernel alone ----------------------------------------------------------------------------------------------------------
OFFS = np.array([[3.0, 4.0], [3.0, 3.875], [3.0, 4.125], [0.0, 0.0], [6.0, 8.0], [4.0, 3.0], [1.5, 2.0], [2.5, 6.0]])      # |.| = 5, <, >, 0, 10, 5, 2.5, 6.5


@pytest.mark.parametrize("N", [70, 5])
def test_kernel_alone_equals_host_form(torch, N):
    """3 scenes of hovering vehicles on a 1/8 grid around integer bases, radius 5, timeout 0.6 s, rounds of 0.25 s: select -> moveback
    -> tick.  Who starts strictly inside the radius is released in round 0, everybody else — the slots at exactly 5 m among them — in
    the first round whose clock exceeds 0.6 s."""
    from neptune_amd.backend import BatchBackend
    S, T, n = 3, 5, 3 * N
    p = scene.scaled_params(N, 0)
    p.pb = np.array([[(a % 10) * 2.0 - 9.0, (a // 10) * 2.0 - 7.0] for a in range(N)])
    be = BatchBackend(p, [], n_scenes=S)
    try:
        dev = be.device
        dt = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=t)      # noqa: E731
        state0 = np.zeros((n, 12))
        state0[:, :2] = np.tile(p.pb, (S, 1)) + OFFS[(np.arange(n) * 3 + np.arange(n) // N) % 8]
        state0[:, 2] = 1.0
        goals = np.zeros((n, 3)); goals[:, 0] = 0.5 + np.arange(n) % 7; goals[:, 1] = -3.0; goals[:, 2] = 1.25
        d = np.sqrt(((state0[:, :2] - np.tile(p.pb, (S, 1))) ** 2).sum(axis=1))
        assert (d < 5.0).any() and (d == 5.0).any() and (d > 5.0).any()
        lo = 6.5 * p.dc
        be.fleet_init(abi.nep_fleet_cfg(p.dc, p.T_span, lo, lo, 0.0, 1.0, 6, 5, T, 0, 0.2, 0.0), dt(state0.reshape(-1), torch.float64), dt(goals.reshape(-1), torch.float64))
        cfg = mission.MoveBack(5.0, 0.6).cfg()
        d_start = torch.zeros(n * abi.FE_START_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(n * abi.TRAJ_REC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        flags = np.zeros(n, dtype=np.int32)
        released = {}
        for r in range(5):
            be.fleet_select(d_start, d_rec)
            start = _starts(d_start)
            assert start["goal"].tobytes() == goals.tobytes()
            be.fleet_moveback(cfg, d_start)
            fs = be.fleet_state(pwp=False)
            _, t_now, rnd = be.fleet_counters()
            assert fs["state"].tobytes() == state0.tobytes() and (rnd == r).all()      # they hover
            before = flags.copy()
            ev = host_moveback(cfg, S, N, fs["state"], p.pb, None, 0.0, t_now, flags, start)
            assert fs["flags"].tobytes() == flags.tobytes(), ("flags", r)
            assert d_start.cpu().numpy().tobytes() == start.tobytes(), ("d_start", r)
            for i in range(n):
                assert ("set" in ev[i]) == (r == 0)
                if (before[i] & WB or r == 0) and not flags[i] & WB:
                    released[i] = (r, ev[i] - {"set"})
            be.fleet_tick()
        first_late = next(r for r in range(5) if sum([p.dc] * (T * r)) > 0.6)
        assert first_late == 3
        for i in range(n):
            assert released[i] == ((0, {"radius"}) if d[i] < 5.0 else (first_late, {"timeout"})), (i, d[i], released[i])
        assert (flags == 0).all()
        be.check()
    finally:
        be.close()


# ---- 2. with missions, fabricated commits -------------------------------------------------------------------------------------------
class AloneBack(tm.Alone):
    """test_gpu_fleet_mission's fabricated rounds with select -> moveback in front: the host chain shares the mission's flag word"""

    def __init__(self, torch, cfg, S, N, T, mb, **kw):
        super().__init__(torch, cfg, S, N, T, **kw)
        n = S * N
        self.mb = mb.cfg()
        self.d_start = torch.zeros(n * abi.FE_START_DTYPE.itemsize, dtype=torch.uint8, device=self.be.device)
        self.d_rec = torch.zeros(n * abi.TRAJ_REC_DTYPE.itemsize, dtype=torch.uint8, device=self.be.device)
        self.sets = self.on_base_goal = 0

    def call(self, pos_s_end=None):
        be, S, N = self.be, self.S, self.N
        be.fleet_select(self.d_start, self.d_rec)
        start = _starts(self.d_start)
        assert start["goal"].tobytes() == self.host.goal.tobytes()
        be.fleet_moveback(self.mb, self.d_start)
        fs = be.fleet_state(pwp=False)
        _, t_now, _ = be.fleet_counters()
        assert t_now.tobytes() == self.t.tobytes()
        ev = host_moveback(self.mb, S, N, fs["state"], self.p.pb, self.host.t_issue, 0.0, t_now, self.host.flags, start)
        assert fs["flags"].tobytes() == self.host.flags.tobytes(), ("flags after moveback", self.calls)
        assert self.d_start.cpu().numpy().tobytes() == start.tobytes(), ("d_start", self.calls)
        new = self.host.t_issue == np.repeat(self.t, N)      # the goals the last call issued (call 0: the first goals)
        assert [("set" in e) for e in ev] == new.tolist(), ("a new goal raises the bit in the next round, and nothing else does", self.calls)
        on = (self.host.flags & WB) != 0
        assert (start["goal"][on, :2] == np.tile(self.p.pb, (S, 1))[on]).all() and (start["goal"][~on] == self.host.goal[~on]).all()
        assert (start["goal"][:, 2] == self.host.goal[:, 2]).all()
        self.sets += int(new.sum()); self.on_base_goal += int(on.sum())
        super().call(pos_s_end)      # commit -> mission -> (the comparison of everything, the flag words among it) -> tick


@pytest.mark.parametrize("mode,N", [(PER_AGENT, 70), (PER_AGENT, 5), (RUNS, 70), (RUNS, 5)])
def test_with_missions_equals_host_chain(torch, mode, N):
    S, T = 3, 5
    if mode == PER_AGENT:
        cfg = mr.make_cfg(PER_AGENT, max_goals=3, log_cap=4, min_interval=0.5, timeout=2.0)
    else:
        cfg = mr.make_cfg(RUNS, max_goals=3, log_cap=2, min_interval=0.0, timeout=1.5, rest_v=0.0, rest_a=0.0, min_dist_self=0.0,
                          close_pos=0.5 if N == 70 else 0.75, close_goal=1.0 if N == 70 else 3.0)
    a = AloneBack(torch, cfg, S, N, T, mission.MoveBack(6.0, 0.6), keep=tm._keepouts(S), seed=N + mode)
    try:
        for _ in range(30 if mode == PER_AGENT else 24):
            a.call()
        h = a.host
        assert a.sets > S * N and a.on_base_goal > 0      # goals beyond the first ones raised the bit; slots searched towards their bases
        ended = h.counts[:, 1] + h.counts[:, 2]
        assert ended.sum() > 0 and h.counts[:, 3].sum() == 0
        # no leg ends "reached" at a base: every record's goal is a goal the generator drew (or the first one), never a base
        log, n = a.be.fleet_mission_log()
        pb = np.tile(a.p.pb, (S, 1))
        if mode == PER_AGENT:
            assert h.counts[:, 1].sum() > 0
            for i, recs in enumerate(log):
                for rec in recs:
                    if rec["outcome"] == abi.NEP_MISSION_REACHED:
                        assert (rec["goal"][0], rec["goal"][1]) != (pb[i, 0], pb[i, 1]), (i, rec)
        assert (np.hypot(*(h.goal[:, :2] - pb).T) > 1e-9).all()
        a.be.check()
    finally:
        a.close()


# ---- 3. in flight behind the real planner -------------------------------------------------------------------------------------------
ROUNDS = 40
BACK = mission.MoveBack(1.5, 2.0)      # the vehicles start 2.5 m from their bases: outside; the timer releases in round 9 at the latest


def _flight(graph, scenes, **kw):
    from neptune_amd.loop import DeviceFleetLoop
    lp = DeviceFleetLoop(scenes, beam_width=32, graph=graph, moveback=BACK, trace=True, **kw)
    rows = []
    try:
        for _ in range(ROUNDS):
            lp.round()
            fs = lp.be.fleet_state(pwp=True)
            rows.append(dict(state=fs["state"].tobytes(), flags=fs["flags"].copy(), pwp=fs["pwp"].tobytes(), done=fs["done"].tobytes(),
                             start=_starts(lp.d_start), plans=b"".join(p.tobytes() for p in lp.be.fleet_plans())))
        lp.be.check()
        assert (lp._g is not None) == graph
        return rows, lp.trace, lp.report(), np.tile(lp.p.pb, (lp.S, 1)), lp.goals.reshape(-1, 3)
    finally:
        lp.close()


@functools.lru_cache(maxsize=None)
def _eager():
    return _flight(False, (_scene(8, 4, 11), _scene(8, 4, 12)))


def test_in_flight_search_goal_is_the_base(torch):
    rows, _, rep, pb, goals = _eager()
    on0 = (rows[0]["flags"] & WB) != 0
    assert on0.all()      # round 0 raised every bit and released none: everybody starts 2.5 m from its base
    last = 0
    for r, row in enumerate(rows):
        on = (row["flags"] & WB) != 0
        g = row["start"]["goal"]
        assert (g[on, :2] == pb[on]).all() and (g[~on] == goals[~on]).all() and (g[:, 2] == goals[:, 2]).all(), r
        assert not (row["flags"] & ~WB).any()
        if on.any():
            last = r
    t = 0.0
    first_late = 0
    while not t > BACK.timeout:
        first_late += 1
        t = sum([_scene(8, 4, 11)["par"].dc] * (5 * first_late))
    assert 0 < last < first_late <= 9, (last, first_late)      # some flew back for a while; the timer's round released the rest
    assert not (rows[-1]["flags"] & WB).any() and all(x["way_back"] == 0 for x in rep)


def test_graph_equals_eager(torch):
    want, trace_w, _, _, _ = _eager()
    got, trace_g, _, _, _ = _flight(True, (_scene(8, 4, 11), _scene(8, 4, 12)))
    assert trace_g == trace_w
    for r in range(ROUNDS):
        for k in want[r]:
            a, b = got[r][k], want[r][k]
            assert (a.tobytes() if hasattr(a, "tobytes") else a) == (b.tobytes() if hasattr(b, "tobytes") else b), (r, k)


def test_one_scene_equals_fleet_loop(torch):
    from neptune_amd.loop import FleetLoop
    sc = _scene(8, 4, 11)
    host = FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), beam_width=32, moveback=BACK)
    host.trace = []
    h_goals, h_flags = [], []
    try:
        for _ in range(ROUNDS):
            host.round()
            h_goals.append(host.last_starts["goal"].copy()); h_flags.append(host.sflags.copy())
        h_state = host.state.copy()
    finally:
        host.close()
    rows, dev_trace, _, _, _ = _flight(True, (sc,))
    trace, t = [], 0.0
    for r, row in enumerate(dev_trace):
        assert rows[r]["start"]["goal"].tobytes() == h_goals[r].tobytes(), ("search goals", r)
        assert rows[r]["flags"].tolist() == h_flags[r].tolist(), ("flags", r)
        for a, (oc, K, fe, qp) in enumerate(row):
            if oc != abi.NEP_FLEET_SKIPPED:      # (an arrived agent: solved and dropped on the device, no entry on the host)
                trace.append((t, a, abi.FLEET_OUTCOMES[oc], K, fe, qp))
        for _ in range(5):
            t += sc["par"].dc
    first = next((k for k, (x, y) in enumerate(zip(trace, host.trace)) if x != y), None)
    assert first is None and len(trace) == len(host.trace), (first, trace[first] if first is not None else None, host.trace[first] if first is not None else None)
    assert rows[-1]["state"] == h_state.tobytes()


# ---- 4. tethered, missions in mode runs, shortened timings ---------------------------------------------------------------------------
def test_tethered_runs_equal_host_chain(torch):
    from neptune_amd.loop import DeviceFleetLoop
    spec = mission.MissionSpec("runs", goals=4, seed=3, timeout=3.0, log_cap=8)
    back = mission.MoveBack(1.5, 1.0)
    scenes = [_scene(8, 4, 11), _scene(8, 4, 12)]
    lp = DeviceFleetLoop(scenes, beam_width=32, graph=False, missions=spec, tethers=True, moveback=back)
    try:
        S, N, T, p = lp.S, lp.N, lp.replan_every, lp.p
        host = mission.HostMission(lp.mission_cfg, S, N, p.pb, lp.goals.reshape(-1, 3))
        cfg = back.cfg()
        seen = dict(sets=0, on=0)

        def after_mission(lp):
            be = lp.be
            plans = be.fleet_plans(); st = be.fleet_state(pwp=False)["state"]
            _, t_now, _ = be.fleet_counters()
            # the select's half: the starts as fleet_select wrote them are A of every slot with the real goals
            start = _starts(lp.d_start)
            want = start.copy(); want["goal"] = host.goal
            new = host.t_issue == np.repeat(t_now, N)
            ev = host_moveback(cfg, S, N, st, p.pb, host.t_issue, 0.0, t_now, host.flags, want)
            assert start.tobytes() == want.tobytes(), ("d_start", lp.rounds)
            assert [("set" in e) for e in ev] == new.tolist(), lp.rounds
            seen["sets"] += int(new.sum()); seen["on"] += int(((host.flags & WB) != 0).sum())
            pos = np.zeros((S * N, T + 1, 3)); s_end = np.zeros((S * N, 12))
            for i in range(S * N):
                pos[i, 0] = st[i, :3]
                for q in range(1, T + 1):
                    pos[i, q] = plans[i][min(q - 1, len(plans[i]) - 1), :3]
                s_end[i] = plans[i][min(T - 1, len(plans[i]) - 1)]
            host.step(pos, s_end, t_now, p.dc)
            tm.compare(be, host, ("tethered runs", lp.rounds))
            tm.tick_done(host, s_end, lp.cfg.goal_radius)
        lp.after_mission = after_mission
        for _ in range(60):
            lp.round()
        assert (lp.be.fleet_done() == host.done).all()
        assert host.scene[:, 0].sum() >= 2 and seen["sets"] > S * N and seen["on"] > seen["sets"]      # runs ended; new goals flew back for rounds
        assert "way_back" in lp.report()[0]
    finally:
        lp.close()


# ---- 5. the recorder ----------------------------------------------------------------------------------------------------------------
def test_recorder_carries_a_moveback_in_progress(torch):
    from neptune_amd.loop import DeviceFleetLoop
    scenes = [_scene(6, 3, 41), _scene(6, 3, 42)]
    spec = mission.MissionSpec("agent", goals=20, seed=3, min_interval=0.0, timeout=1.0, rest_v=100.0, rest_a=100.0, min_dist_self=3.0, log_cap=2)
    back = mission.MoveBack(1.0, 0.6)
    kw = dict(beam_width=16, graph=False, missions=spec)
    plain = DeviceFleetLoop(scenes, **kw)
    try:
        want_bytes = plain.be.fleet_snapshot_bytes()
    finally:
        plain.close()
    lp = DeviceFleetLoop(scenes, recorder=8, moveback=back, **kw)
    try:
        assert lp.be.fleet_snapshot_bytes() == want_bytes      # the bit lives in a word the snapshot already had
        batch, starts, flags = [], [], []
        for r in range(12):
            flags.append(lp.be.fleet_state(pwp=False)["flags"].reshape(lp.S, lp.N)[1].copy())      # before round r
            lp.round()
            batch.append(tr.fingerprint(lp, 1)); starts.append(_starts(lp.d_start).reshape(lp.S, lp.N)[1].tobytes())
        cut = next(r for r in range(5, 12) if (flags[r] & WB).any())      # a round before which somebody is on its way back
        one = lp.rewind(1, cut)
        try:
            assert one.moveback == back and one.S == 1
            for r in range(cut, 12):
                one.round()
                tr.same(tr.fingerprint(one), batch[r], ("scene 1 alone", r))
                assert _starts(one.d_start).tobytes() == starts[r], ("d_start", r)
        finally:
            one.close()
    finally:
        lp.close()


# ---- 6. contracts -------------------------------------------------------------------------------------------------------------------
def test_contracts_and_capture(torch):
    from neptune_amd._lib import lib
    from neptune_amd.backend import BatchBackend
    L = lib()
    N = 5
    p = scene.scaled_params(N, 0)
    cfg = abi.nep_moveback_cfg(1.0, 10.0)
    be = BatchBackend(p, [], n_scenes=2)
    sh = BatchBackend(p, [], first_local=0, n_local=2)
    try:
        dev = be.device
        n = 2 * N
        d_start = torch.zeros(n * abi.FE_START_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(n * abi.TRAJ_REC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        assert L.nep_batch_fleet_moveback(None, C.byref(cfg), d_start.data_ptr(), None) == -1      # NEP_E_ARG: a device and no handle
        assert L.nep_batch_fleet_moveback(be._h, C.byref(cfg), d_start.data_ptr(), None) == -2     # NEP_E_STATE: before nep_batch_fleet_init
        assert L.nep_batch_fleet_moveback(sh._h, C.byref(cfg), d_start.data_ptr(), None) == -2     # a sharded handle
        state0 = np.zeros((n, 12)); state0[:, :2] = np.tile(p.pb, (2, 1)) + [3.0, 0.0]; state0[:, 2] = 1.0
        goals = np.zeros((n, 3)); goals[:, 2] = 1.0
        dt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=torch.float64)      # noqa: E731
        lo = 6.5 * p.dc
        be.fleet_init(abi.nep_fleet_cfg(p.dc, p.T_span, lo, lo, 0.0, 1.0, 6, 5, 5, 0, 0.2, 0.0), dt(state0.reshape(-1)), dt(goals.reshape(-1)))
        assert L.nep_batch_fleet_moveback(be._h, None, d_start.data_ptr(), None) == -1
        assert L.nep_batch_fleet_moveback(be._h, C.byref(cfg), None, None) == -1
        for radius, timeout in ((math.nan, 10.0), (math.inf, 10.0), (1.0, -0.5), (1.0, math.nan), (1.0, math.inf)):
            assert L.nep_batch_fleet_moveback(be._h, C.byref(abi.nep_moveback_cfg(radius, timeout)), d_start.data_ptr(), None) == -1, (radius, timeout)
        assert (be.fleet_state(pwp=False)["flags"] == 0).all()      # a refused call wrote nothing
        # one eager round, then the same three calls inside a capture: nothing is allocated, and the replay is the rule's round
        flags = np.zeros(n, dtype=np.int32)

        def ops():
            be.fleet_select(d_start, d_rec)
            be.fleet_moveback(cfg, d_start)
            be.fleet_tick()

        def round_(run, r):
            _, t_before, _ = be.fleet_counters()
            run()
            torch.cuda.synchronize()
            start = _starts(d_start)
            want = start.copy(); want["goal"] = goals
            host_moveback(cfg, 2, N, state0, p.pb, None, 0.0, t_before, flags, want)
            assert start.tobytes() == want.tobytes() and be.fleet_state(pwp=False)["flags"].tobytes() == flags.tobytes(), r
        round_(ops, 0)
        assert (flags == WB).all()
        torch.cuda.synchronize()
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
        assert be.fleet_counters()[2].tolist() == [1, 1]      # (captured, not run)
        round_(g.replay, 1)
        assert (flags == WB).all() and be.fleet_counters()[2].tolist() == [2, 2]
        be.check()
        del g
    finally:
        be.close(); sh.close()
