"""CPU: scripted goals, mission mode NEP_MISSION_FLEET_TOGETHER and the effort record (include/neptune_fleet.h) as far as they can
be checked without a GPU — the host forms nep_mission_step_script and nep_effort_step against restatements in Python ints and
floats (tests/mission_script_ref.py), every field exact; the exchange driver's lists; the ABI; the argument errors."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import mission_ref as mr
import mission_script_ref as msr
from neptune_amd import _lib, abi, mission

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_AGENT, RUNS, TOGETHER = abi.NEP_MISSION_PER_AGENT, abi.NEP_MISSION_FLEET_RUNS, 3


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def mode_cfg(mode, max_goals, **kw):
    if mode == PER_AGENT:
        d = dict(max_goals=max_goals, log_cap=4, min_interval=0.5, timeout=2.0)
    else:
        d = dict(max_goals=max_goals, log_cap=3, min_interval=0.0, timeout=1.5, rest_v=0.0, rest_a=0.0, min_dist_self=0.0, close_pos=0.75, close_goal=3.0)
    d.update(kw)
    return mr.make_cfg(mode, **d)


def _walk(cfg, S, N, T, calls, seed, G, dc=0.1):
    rng = np.random.default_rng(2000 + seed)
    pb = mr.circle_bases(N)
    goals = np.zeros((S * N, 3)); goals[:, :2] = rng.uniform(-8.0, 8.0, (S * N, 2)); goals[:, 2] = cfg.goal_z
    script = msr.random_script(rng, S * N, G) if G else None
    host = mission.HostMission(cfg, S, N, pb, goals, script=script)
    ref = msr.RefScriptMission(cfg, S, N, pb, goals, script=script)
    w = mr.Walk(seed, S, N, T, goal_z=cfg.goal_z)
    t = np.zeros(S)
    for r in range(calls):
        pos, s_end = w.call(host.goal)
        host.step(pos, s_end, t, dc)
        ref.step(pos, s_end, t, dc)
        mr.assert_same(host, ref, (r,))
        for _ in range(T):
            t = t + dc
    return host, ref, script


@pytest.mark.parametrize("mode", [PER_AGENT, RUNS, TOGETHER])
@pytest.mark.parametrize("G", [1, 2, 3])
def test_host_equals_restatement_scripted(L, mode, G):
    """seeded walks with a quota beyond G (the table wraps), z from the table, attempts 0, no no-goal path"""
    cfg = mode_cfg(mode, max_goals=G + 3)
    ev = dict()
    for seed in range(3):
        host, ref, script = _walk(cfg, 2, 5, 5, 60, seed, G)
        for k, v in ref.ev.items():
            ev[k] = ev.get(k, 0) + int(v)
        assert (host.log["attempts"] == 0).all() and host.counts[:, 3].sum() == 0 and (host.flags == 0).all()
        # every goal issued is a row of its slot's table, z included: row (issued - 2) mod G — issued counts the open leg too
        for i in range(len(host.goal)):
            if host.counts[i, 0] >= 2:
                assert host.goal[i].tobytes() == script[i, (host.counts[i, 0] - 2) % G].tobytes()
    assert ev["scripted"] > 0 and ev["wrapped"] > 0 and ev["quota"] > 0, ev
    assert ev["reached" if mode == PER_AGENT else "run_failed"] > 0, ev


@pytest.mark.parametrize("mode", [PER_AGENT, RUNS])
def test_no_script_equals_mission_step(L, mode):
    """n_goals = 0 is nep_mission_step, byte for byte: the same walk through both entry points"""
    cfg = mode_cfg(mode, max_goals=4)
    S, N, T = 2, 5, 5
    rng = np.random.default_rng(7)
    goals = np.zeros((S * N, 3)); goals[:, :2] = rng.uniform(-8.0, 8.0, (S * N, 2)); goals[:, 2] = cfg.goal_z
    keep = mr.random_keepouts(rng, S, 3)
    a = mission.HostMission(cfg, S, N, mr.circle_bases(N), goals, keepouts=keep)
    b = mission.HostMission(cfg, S, N, mr.circle_bases(N), goals, keepouts=keep)
    w = mr.Walk(3, S, N, T, goal_z=cfg.goal_z)
    t = np.zeros(S)
    vp = lambda x, i0=0: x[i0:].ctypes.data      # noqa: E731
    for r in range(40):
        pos, s_end = w.call(a.goal)
        a.step(pos, s_end, t, 0.1)
        for s in range(S):
            npoly, off, xy = b.keep[s]
            lo = s * N; o = lo if b.per_agent else s
            sc = abi.nep_mission_scene(N, s, T, npoly, float(t[s]), 0.1, vp(pos, lo), vp(s_end, lo), b.pb.ctypes.data, off.ctypes.data, xy.ctypes.data,
                                       vp(b.goal, lo), vp(b.done, lo), vp(b.flags, lo), vp(b.t_issue, lo), vp(b.length, lo), vp(b.completed, lo),
                                       vp(b.counts, lo), vp(b.sums, lo), vp(b.scene, s), vp(b.t_run, s), vp(b.log, o), vp(b.log_n, o))
            assert L.nep_mission_step_script(C.byref(cfg), C.byref(sc), 0, None) == 0
        mr.assert_same(a, b, (r,))
        for _ in range(T):
            t = t + 0.1
    assert a.counts[:, 0].max() > 1 and (a.log["attempts"] > 0).any()      # goals were drawn


def test_together_without_script_draws(L):
    """mode 3 without a script is legal and draws, by the rules of the other two modes"""
    cfg = mode_cfg(TOGETHER, max_goals=4)
    ev = dict()
    for seed in range(3):
        host, ref, _ = _walk(cfg, 2, 5, 5, 60, seed, 0)
        for k, v in ref.ev.items():
            ev[k] = ev.get(k, 0) + int(v)
    assert ev["scripted"] == 0 and ev["run_failed"] > 0 and host.log["attempts"].max() > 0


def test_scripted_goal_equal_to_the_position(L):
    """a scripted goal may be where the agent stands (test 1, min_dist_self, is not applied): it is issued and then reached at once"""
    cfg = mr.make_cfg(PER_AGENT, max_goals=3, min_interval=0.0, min_dist_self=3.0, log_cap=4)
    here = np.array([[2.0, -1.0, 1.5]])
    script = here.reshape(1, 1, 3).copy()
    goals = here.copy()
    host = mission.HostMission(cfg, 1, 1, np.zeros((1, 2)), goals, script=script)
    ref = msr.RefScriptMission(cfg, 1, 1, np.zeros((1, 2)), goals, script=script)
    pos = np.repeat(here[:, None, :], 2, axis=1); s_end = np.zeros((1, 12)); s_end[:, :3] = here
    for r in range(3):
        for m in (host, ref):
            m.step(pos, s_end, np.full(1, 0.1 * r), 0.1)
        mr.assert_same(host, ref, r)
    assert host.counts[0].tolist() == [3, 3, 0, 0] and host.scene[0, 3] == 1 and host.goal[0].tolist() == [2.0, -1.0, 1.5]
    assert [int(x["attempts"]) for x in host.log[0, :3]] == [0, 0, 0] and host.flags[0] == 0


def test_together_is_sticky_where_runs_is_not(L):
    """a path that enters the goal's square and leaves it again: mode 3 stays completed and the run succeeds, mode 2 does not.  The
    square is x-y only: an agent 5 m above the goal is inside it, and outside mode 2's ball."""
    N, r = 2, math.sqrt(0.5)
    goals = np.array([[0.0, 0.0, 1.0], [4.0, 0.0, 1.0]])
    script = np.array([[[1.0, 1.0, 2.0]], [[5.0, 1.0, 2.5]]])
    out = {}
    for mode in (RUNS, TOGETHER):
        cfg = mr.make_cfg(mode, max_goals=2, log_cap=2, timeout=50.0, arrive_radius=r, min_dist_self=0.0)
        host = mission.HostMission(cfg, 1, N, mr.circle_bases(N), goals, script=script)
        ref = msr.RefScriptMission(cfg, 1, N, mr.circle_bases(N), goals, script=script)
        # agent 0: 3 m away -> 0.7 m off in x and y (inside the square, outside a ball of r) -> away again; agent 1: onto its goal, 5 m above it
        pos = np.zeros((N, 4, 3))
        pos[0] = [[3.0, 0.0, 1.0], [0.7, 0.7, 1.0], [0.7, 0.7, 1.0], [3.0, 0.0, 1.0]]
        pos[1] = [[7.0, 0.0, 1.0], [4.0, 0.0, 6.0], [4.0, 0.0, 6.0], [4.0, 0.0, 6.0]]
        s_end = np.zeros((N, 12)); s_end[:, :3] = pos[:, -1]
        for m in (host, ref):
            m.step(pos, s_end, np.zeros(1), 0.1)
        mr.assert_same(host, ref, mode)
        out[mode] = host
    assert 0.7 * 0.7 < r * r < 0.7 * 0.7 * 2
    assert out[TOGETHER].scene.tolist() == [[1, 1, 0, 0]] and out[TOGETHER].counts[:, :3].tolist() == [[2, 1, 0]] * 2
    assert out[TOGETHER].goal.tolist() == [[1.0, 1.0, 2.0], [5.0, 1.0, 2.5]]                       # z from the table
    rec = out[TOGETHER].log[0, 0]
    # lengths: agent 0 grows until the tick that completes it (that tick included), agent 1 likewise
    want = ((0.0 + mr.n3(0.7 - 3.0, 0.7 - 0.0, 0.0)) + mr.n3(4.0 - 7.0, 0.0, 6.0 - 1.0)) / 2.0
    assert rec["outcome"] == abi.NEP_MISSION_REACHED and rec["attempts"] == 0 and rec["length"] == want
    assert out[RUNS].scene.tolist() == [[0, 0, 0, 0]] and out[RUNS].completed.tolist() == [0, 0]
    assert out[TOGETHER].completed.tolist() == [0, 0]                     # (zeroed by the new run)


def test_together_timeout_none_and_finite(L):
    cfg = mr.make_cfg(TOGETHER, max_goals=2, log_cap=2, timeout=math.inf, min_dist_self=0.0)
    goals = np.array([[0.0, 0.0, 1.0]])
    script = np.array([[[1.0, 1.0, 1.0]]])
    host = mission.HostMission(cfg, 1, 1, np.zeros((1, 2)), goals, script=script)
    pos = np.full((1, 2, 3), 5.0); s_end = np.zeros((1, 12)); s_end[:, :3] = 5.0
    host.step(pos, s_end, np.full(1, 1e9), 0.1)
    assert host.scene.tolist() == [[0, 0, 0, 0]]      # no timeout: a blocked fleet waits
    cfg.timeout = 2.0
    host.step(pos, s_end, np.full(1, 1e9), 0.1)
    assert host.scene.tolist() == [[1, 0, 1, 0]] and host.goal[0].tolist() == [1.0, 1.0, 1.0] and host.counts[0].tolist() == [2, 0, 1, 0]


# ---- the effort record ------------------------------------------------------------------------------------------------------------
LIM = dict(v_max=2.0, a_max=3.0, j_max=5.0)


def _both(ring, head, size, done, slack, T, dc=0.05, rec=None):
    a = msr.new_effort() if rec is None else rec[0]
    b = msr.new_effort() if rec is None else rec[1]
    mission.effort_step(LIM["v_max"], LIM["a_max"], LIM["j_max"], dc, T, ring, head, size, done, slack, a)
    n = msr.effort_ref(LIM["v_max"], LIM["a_max"], LIM["j_max"], dc, T, ring, head, size, done, slack, b)
    assert a.tobytes() == b.tobytes(), (a, b)
    return a, b, n


def test_effort_host_equals_restatement(L):
    rng = np.random.default_rng(5)
    seen = set()
    for case in range(200):
        cap = int(rng.integers(1, 12)); T = int(rng.integers(1, 9))
        ring = msr.random_ring(rng, cap)
        head = int(rng.integers(0, cap)); size = int(rng.integers(0, cap + 1)); done = int(rng.uniform() < 0.15)
        a, _, n = _both(ring, head, size, done, 1e-6, T)
        assert int(a["n_ticks"][0]) == n == (0 if done else min(T, size))
        seen.add(("done", done)); seen.add(("short", size < T)); seen.add(("wrap", head + min(T, size) > cap))
        seen.add(("viol", bool(a["n_v_viol"][0] or a["n_a_viol"][0] or a["n_j_viol"][0])))
    assert seen >= {("done", 1), ("done", 0), ("short", True), ("short", False), ("wrap", True), ("viol", True), ("viol", False)}


def test_effort_ring_runs_out_and_done(L):
    ring = np.zeros((6, 12)); ring[:, 9] = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]      # jerk x per entry
    a, _, n = _both(ring, 4, 3, 0, 0.0, 5)      # entries 4, 5, 0; ticks 4 and 5 repeat the last state: not counted
    assert n == 3 and a["jerk_sum"][0] == ((0.0 + 5.0 * 0.05) + 6.0 * 0.05) + 1.0 * 0.05 and a["max_j"][0].tolist() == [6.0, 0.0, 0.0]
    assert a["n_j_viol"][0] == 1      # 6 > 5
    a, _, n = _both(ring, 4, 3, 1, 0.0, 5)      # an arrived slot adds nothing
    assert n == 0 and a.tobytes() == msr.new_effort().tobytes()
    a, _, n = _both(ring, 0, 0, 0, 0.0, 5)      # an empty plan neither
    assert n == 0 and a.tobytes() == msr.new_effort().tobytes()


def test_effort_limit_edges(L):
    """a component exactly at the limit, at limit + slack, and one ulp beyond: only the last is a violation"""
    slack = 0.25
    for off, lim, cnt in ((3, 2.0, "n_v_viol"), (6, 3.0, "n_a_viol"), (9, 5.0, "n_j_viol")):
        for axis in range(3):
            for sign in (1.0, -1.0):
                for value, want in ((lim, 0), (lim + slack, 0), (np.nextafter(lim + slack, 100.0), 1), (np.nextafter(lim, 100.0), 0)):
                    ring = np.zeros((1, 12)); ring[0, off + axis] = sign * value
                    a, _, _ = _both(ring, 0, 1, 0, slack, 1)
                    assert int(a[cnt][0]) == want and sum(int(a[c][0]) for c in ("n_v_viol", "n_a_viol", "n_j_viol")) == want
        ring = np.zeros((1, 12)); ring[0, off] = np.nextafter(lim, 100.0)
        a, _, _ = _both(ring, 0, 1, 0, 0.0, 1)
        assert int(a[cnt][0]) == 1
    # a tick with two components beyond the same limit counts once
    ring = np.zeros((1, 12)); ring[0, 3:6] = [2.5, -2.5, 0.0]
    a, _, _ = _both(ring, 0, 1, 0, 0.0, 1)
    assert int(a["n_v_viol"][0]) == 1 and a["max_v"][0].tolist() == [2.5, 2.5, 0.0]


def test_effort_chained_calls_equal_one(L):
    """n ticks in one call against the same ticks in two calls (the ring popped in between, as nep_batch_fleet_tick does)"""
    rng = np.random.default_rng(11)
    cap = 16
    ring = msr.random_ring(rng, cap)
    one, _, n = _both(ring, 13, 12, 0, 1e-6, 9)
    assert n == 9
    two = (msr.new_effort(), msr.new_effort())
    _both(ring, 13, 12, 0, 1e-6, 4, rec=two)
    _both(ring, (13 + 4) % cap, 12 - 4, 0, 1e-6, 5, rec=two)
    assert two[0].tobytes() == one.tobytes()


# ---- the exchange driver's lists ----------------------------------------------------------------------------------------------------
def test_exchange_script():
    for N in (5, 8, 12):
        e = mission.exchange_script(N, radius=10.0, z=1.5)
        assert e.shape == (N, 2, 3) and (e[:, :, 2] == 1.5).all()
        for x in range(N):
            R = 10.7 if N == 8 and x % 2 == 1 else 10.0
            th = 2 * math.pi / N * x
            # goals1 first: the driver publishes goals[currentrun % 2] with currentrun = 1
            assert e[x, 0, :2].tolist() == [-R * math.cos(th + math.pi), -R * math.sin(th + math.pi)]
            assert e[x, 1, :2].tolist() == [-R * math.cos(th), -R * math.sin(th)]
            assert np.allclose(e[x, 0, :2], -e[x, 1, :2], atol=1e-12) and abs(np.hypot(*e[x, 0, :2]) - R) < 1e-12      # antipodal
    assert mission.exchange_script(8, radius=4.0)[1, 0, 0] == -4.7 * math.cos(2 * math.pi / 8 + math.pi)
    assert mission.exchange_script(6, radius=4.0)[1, 0, 0] == -4.0 * math.cos(2 * math.pi / 6 + math.pi)


def test_spec_together_and_script_shapes():
    from neptune_amd import scene
    p = scene.scaled_params(8, 4)
    c = mission.mission_cfg(mission.MissionSpec("together"), p)
    assert c.mode == TOGETHER and c.arrive_radius == math.sqrt(0.5) and c.timeout == math.inf and c.tether_max == p.tether_length
    assert mission.mission_cfg(mission.MissionSpec("together", timeout=30.0), p).timeout == 30.0
    with pytest.raises(ValueError):
        mission.mission_cfg(mission.MissionSpec("apart"), p)
    e = mission.exchange_script(8)
    assert mission.script_rows(mission.MissionSpec("together"), 2, 8) is None
    r = mission.script_rows(mission.MissionSpec("together", script=e), 2, 8)
    assert r.shape == (2, 8, 2, 3) and (r[0] == e).all() and (r[1] == e).all()
    r = mission.script_rows(mission.MissionSpec("runs", script=np.stack([e, 2 * e])), 2, 8)
    assert (r[1] == 2 * e).all()
    bad = e.copy(); bad[3, 1, 0] = np.nan
    for s in (e[:7], np.stack([e] * 3), e[:, :0], e[:, :, :2], bad):
        with pytest.raises(ValueError):
            mission.script_rows(mission.MissionSpec("together", script=s), 2, 8)
    d, sc = mission.spec_plain(mission.MissionSpec("together", script=e))
    assert "script" not in d and sc == e.tolist() and mission.MissionSpec(**d, script=sc).mode == "together"
    assert mission.effort_slack(False) is None and mission.effort_slack(None) is None and mission.effort_slack(True) == 1e-6 and mission.effort_slack(0.5) == 0.5
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            mission.effort_slack(bad)


# ---- the ABI and the argument errors --------------------------------------------------------------------------------------------------
SIZES = {18: 80, 20: 136, 21: 64, 25: 80, 27: 16}


def test_abi(L):
    assert abi.NEP_MISSION_FLEET_TOGETHER == 3
    assert L.nep_abi_sizeof(29) == C.sizeof(abi.nep_fleet_effort) == abi.EFFORT_DTYPE.itemsize == 96
    assert L.nep_abi_sizeof(28) == -1 and L.nep_abi_sizeof(30) == -1
    # every earlier size: what the Python mirrors say (checked against the library at load), and the literals other tests pin
    for which, struct in ((1, abi.nep_traj_rec), (5, abi.nep_guess), (6, abi.nep_solution), (11, abi.nep_fe_cfg), (12, abi.nep_fe_start), (13, abi.nep_fe_result),
                          (14, abi.nep_fe_ent_state), (17, abi.nep_audit), (18, abi.nep_fleet_cfg), (20, abi.nep_mission_cfg), (21, abi.nep_mission_leg),
                          (23, abi.nep_ent_lists), (25, abi.nep_fleet_snapshot_hdr), (27, abi.nep_moveback_cfg)):
        assert L.nep_abi_sizeof(which) == C.sizeof(struct), which
    for which, size in SIZES.items():
        assert L.nep_abi_sizeof(which) == size, which
    for which in (16, 19, 22, 24, 26):
        assert L.nep_abi_sizeof(which) == -1
    assert all(L.nep_abi_sizeof(w) > 0 for w in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17))
    hdr = open(os.path.join(ROOT, "include", "neptune_fleet.h")).read()
    assert re.search(r"#define NEP_MISSION_FLEET_TOGETHER 3\b", hdr) and re.search(r"#define NEP_SNAPSHOT_VERSION 1\b", hdr)
    for name in ("nep_batch_fleet_mission_script", "nep_mission_step_script", "nep_batch_fleet_effort", "nep_effort_step"):
        assert name in _lib.FLEET_EXPORTS and getattr(L, name) and name in hdr


def test_argument_errors(L):
    cfg = mr.make_cfg(TOGETHER, min_dist_self=0.0)
    goals = np.zeros((1, 3)); script = np.zeros((1, 2, 3))
    host = mission.HostMission(cfg, 1, 1, np.zeros((1, 2)), goals, script=script)
    pos = np.zeros((1, 2, 3)); s_end = np.zeros((1, 12))
    host.step(pos, s_end, np.zeros(1), 0.1)
    for bad in (np.nan, np.inf, -np.inf):
        host.script[0, 1, 2] = bad
        with pytest.raises(_lib.BackendError, match="-1"):
            host.step(pos, s_end, np.zeros(1), 0.1)
    host.script[0, 1, 2] = 0.0
    assert L.nep_mission_step_script(None, None, 0, None) == -1
    vp = lambda x: x.ctypes.data      # noqa: E731
    sc = abi.nep_mission_scene(1, 0, 1, 0, 0.0, 0.1, vp(pos), vp(s_end), vp(host.pb), None, None, vp(host.goal), vp(host.done), vp(host.flags), vp(host.t_issue),
                               vp(host.length), vp(host.completed), vp(host.counts), vp(host.sums), vp(host.scene), vp(host.t_run), vp(host.log), vp(host.log_n))
    assert L.nep_mission_step_script(C.byref(cfg), C.byref(sc), -1, None) == -1
    assert L.nep_mission_step_script(C.byref(cfg), C.byref(sc), 2, None) == -1            # a length without a table
    assert L.nep_mission_step_script(C.byref(cfg), C.byref(sc), 0, None) == 0
    c4 = mr.make_cfg(4)
    assert L.nep_mission_step_script(C.byref(c4), C.byref(sc), 0, None) == -1             # no mode 4
    # nep_effort_step
    ring = np.zeros((4, 12)); out = msr.new_effort()
    ok = dict(v_max=2.0, a_max=3.0, j_max=5.0, dc=0.05, T=5, head=0, size=4, cap=4, done=0, slack=0.0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.nep_effort_step(a["v_max"], a["a_max"], a["j_max"], a["dc"], a["T"], ring.ctypes.data, a["head"], a["size"], a["cap"], a["done"], a["slack"],
                                 out.ctypes.data)
    assert call() == 0
    for kw in (dict(slack=-1e-9), dict(slack=math.nan), dict(slack=math.inf), dict(v_max=0.0), dict(a_max=math.nan), dict(j_max=-5.0), dict(dc=0.0), dict(T=0),
               dict(head=4), dict(head=-1), dict(size=5), dict(size=-1), dict(cap=0)):
        assert call(**kw) == -1, kw
    assert L.nep_effort_step(2.0, 3.0, 5.0, 0.05, 5, None, 0, 4, 4, 0, 0.0, out.ctypes.data) == -1
    assert L.nep_effort_step(2.0, 3.0, 5.0, 0.05, 5, ring.ctypes.data, 0, 4, 4, 0, 0.0, None) == -1
    # the device entry points fail loudly without a handle (no device: NEP_E_HIP; a device and no handle: NEP_E_ARG)
    import torch
    want = -1 if torch.cuda.is_available() else -3
    assert L.nep_batch_fleet_mission_script(None, 0, None) == want
    assert L.nep_batch_fleet_effort(None, 5.0, 0.0, None, None) == want


def test_host_forms_under_sanitizers(tmp_path):
    """tests/cpp/mission_script_check.cpp drives mission_host.cpp and effort_host.cpp (host code only, its own main) through seeded
    walks in the three modes with tables of 0 to 3 rows and through rings of every head and size, built with
    -fsanitize=address,undefined"""
    import subprocess
    exe = str(tmp_path / "mission_script_check")
    src = [os.path.join(ROOT, "tests", "cpp", "mission_script_check.cpp"), os.path.join(ROOT, "neptune_amd", "csrc", "mission_host.cpp"),
           os.path.join(ROOT, "neptune_amd", "csrc", "effort_host.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include")] + src + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "mission_script_check ok" in r.stdout, (r.stdout, r.stderr)
