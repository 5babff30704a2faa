"""CPU: the fleet's mission controller (include/neptune_fleet.h, "missions") as far as it can be checked without a GPU — the host
form nep_mission_step against a restatement in Python ints and floats (tests/mission_ref.py), every field exact, over seeded walks
in both modes; the generator's known answers; the polygon boundary; a draw that needs a second batch of 64 candidates; the no-goal
path; the log's wrap; the ABI; the entry points' contracts without a device; and a stand-alone sanitizer build of the host form."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mission_ref as mr
from neptune_amd import _lib, abi, mission

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_AGENT, RUNS = abi.NEP_MISSION_PER_AGENT, abi.NEP_MISSION_FLEET_RUNS


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _walk(cfg, S, N, T, n_poly, calls, seed, dc=0.1):
    rng = np.random.default_rng(1000 + seed)
    keep = mr.random_keepouts(rng, S, n_poly)
    pb = mr.circle_bases(N)
    goals = np.zeros((S * N, 3)); goals[:, :2] = rng.uniform(-8.0, 8.0, (S * N, 2)); goals[:, 2] = cfg.goal_z
    host = mission.HostMission(cfg, S, N, pb, goals, keepouts=keep)
    ref = mr.RefMission(cfg, S, N, pb, goals, keepouts=keep)
    w = mr.Walk(seed, S, N, T, goal_z=cfg.goal_z)
    t = np.zeros(S)
    for r in range(calls):
        pos, s_end = w.call(host.goal)
        host.step(pos, s_end, t, dc)
        ref.step(pos, s_end, t, dc)
        mr.assert_same(host, ref, (r,))
        for _ in range(T):
            t = t + dc
    return host, ref


@pytest.mark.parametrize("N,T,n_poly", [(5, 1, 0), (5, 5, 5), (70, 5, 5), (70, 1, 0)])
def test_host_equals_restatement_per_agent(L, N, T, n_poly):
    cfg = mr.make_cfg(PER_AGENT, max_goals=3, log_cap=4, min_interval=0.5, timeout=2.0)
    ev = dict()
    for seed in range(2 if N == 70 else 6):
        _, ref = _walk(cfg, 3, N, T, n_poly, 90 if T == 1 else 30, seed)
        for k, v in ref.ev.items():
            ev[k] = ev.get(k, 0) + int(v)
    # the walk has exercised: legs reached and timed out, the min_interval hold-off, the rest test with the reference's precedence
    # (a moving agent is held before the timeout and not after it; an accelerating one always), quota exhaustion
    for k in ("reached", "timed_out", "held_interval", "held_v", "held_a", "timeout_moving", "quota"):
        assert ev[k] > 0, (k, ev)
    assert ev["no_goal"] == 0


@pytest.mark.parametrize("T,n_poly", [(1, 0), (5, 5)])
def test_host_equals_restatement_fleet_runs(L, T, n_poly):
    cfg = mr.make_cfg(RUNS, max_goals=4, log_cap=3, min_interval=0.0, timeout=1.5, rest_v=0.0, rest_a=0.0, min_dist_self=0.0, close_pos=0.75, close_goal=3.0)
    ev = dict()
    for seed in range(8):
        host, ref = _walk(cfg, 3, 5, T, n_poly, 120 if T == 1 else 40, seed)
        for k, v in ref.ev.items():
            ev[k] = ev.get(k, 0) + int(v)
    for k in ("run_failed", "uncompleted", "quota"):
        assert ev[k] > 0, (k, ev)
    assert ev["no_goal"] == 0


def test_fleet_run_success(L):
    """every agent driven onto its goal: the run succeeds, the record carries the mean length, the next run's goals keep close_goal"""
    cfg = mr.make_cfg(RUNS, max_goals=2, log_cap=2, timeout=50.0, min_dist_self=0.0, close_pos=0.5, close_goal=2.0)
    N = 5
    goals = np.array([[-4.0 + 2 * a, 1.0, 1.0] for a in range(N)])
    host = mission.HostMission(cfg, 1, N, mr.circle_bases(N), goals)
    ref = mr.RefMission(cfg, 1, N, mr.circle_bases(N), goals)
    pos = np.zeros((N, 3, 3)); pos[:, 0] = goals + [3.0, 4.0, 0.0]; pos[:, 1] = goals + [0.0, 0.1, 0.0]; pos[:, 2] = goals
    s_end = np.zeros((N, 12)); s_end[:, :3] = goals
    for m in (host, ref):
        m.step(pos, s_end, np.zeros(1), 0.1)
    mr.assert_same(host, ref)
    assert host.scene.tolist() == [[1, 1, 0, 0]] and host.log_n[0] == 1
    r = host.log[0, 0]
    # the first step is flown un-completed (5 m), the second starts completed: the leg does not grow
    assert r["outcome"] == abi.NEP_MISSION_REACHED and r["t_end"] == 0.1 + 0.1 and r["length"] == (5 * np.sqrt(3.0 * 3.0 + 3.9 * 3.9)) / 5.0
    assert (host.counts[:, :3] == [2, 1, 0]).all() and (host.completed == 0).all() and (host.length == 0).all()
    g = host.goal
    for a in range(N):
        for j in range(a):
            assert np.sqrt(((g[a] - g[j]) ** 2).sum()) >= 2.0
    # the second run ends the campaign: nothing is drawn
    pos2 = np.repeat(g[:, None, :], 3, axis=1); s2 = np.zeros((N, 12)); s2[:, :3] = g
    for m in (host, ref):
        m.step(pos2, s2, np.full(1, 0.2), 0.1)
    mr.assert_same(host, ref)
    assert host.scene.tolist() == [[2, 2, 0, 1]] and (host.goal == g).all() and (host.counts[:, :3] == [2, 2, 0]).all()
    before = [getattr(host, f).copy() for f in mr.FIELDS]
    host.step(pos2, s2, np.full(1, 0.4), 0.1)      # a finished scene: nothing happens
    assert all((getattr(host, f) == b).all() for f, b in zip(mr.FIELDS, before))


# (seed, global slot, goal index, k) -> h1, bits_x, bits_y of the header's text, and x, y in the unit box: worked once by hand from
# sm() — whose own first outputs are splitmix64's published ones — and frozen here, so that a change of the composition of h1, of
# the counters 2k / 2k + 1 or of the mapping to [0, 1) cannot pass unnoticed in both forms at once
KNOWN = ((7, 0, 1, 0, 0x0A71140F7CEBD982, 0xCA4D9F8C88871CF1, 0x7E635E8A78D485F1, '0x1.949b3f19110e3p-1', '0x1.f98d7a29e3520p-2'),
         (7, 69, 2, 63, 0x8B5052CC23EDCBB1, 0x9A858D51327B79D4, 0x70C12774A47BC2D6, '0x1.350b1aa264f6fp-1', '0x1.c3049dd291ef0p-2'),
         (123456789, 209, 1, 64, 0x1D7E870251F7992F, 0xB60108FFA0EAE7E0, 0xE383CFD64FCCFA91, '0x1.6c0211ff41d5cp-1', '0x1.c7079fac9f99fp-1'))


def _host_draw(seed, slot, index, k):
    """nep_mission_step's goal and attempts for the draw (slot, index) when only candidate k passes among 0..k: a tether disc
    around it that holds none of the earlier ones (k = 0: every test off)"""
    N = 70
    S, a = slot // N + 1, slot % N
    cfg = mr.make_cfg(PER_AGENT, seed=seed, lo=(0.0, 0.0), hi=(1.0, 1.0), max_goals=10, min_interval=0.0, timeout=1e9, min_dist_self=0.0, tether_max=0.0,
                      close_pos=0.0, close_goal=0.0)
    c = [mr.candidate(cfg, slot, index, q) for q in range(k + 1)]
    pb = np.full((N, 2), 9.0)
    if k:
        pb[a] = c[k]
        cfg.tether_max = 0.5 * min(np.hypot(q[0] - c[k][0], q[1] - c[k][1]) for q in c[:k])
    goals = np.zeros((S * N, 3)); goals[:, 2] = 1.0
    host = mission.HostMission(cfg, S, N, pb, goals)
    host.counts[:, 0] = index
    pos = np.full((S * N, 2, 3), 50.0); pos[:, :, 2] = 1.0; pos[slot] = goals[slot]      # only this slot sits on its goal
    s_end = np.zeros((S * N, 12)); s_end[:, :3] = pos[:, 1]
    host.step(pos, s_end, np.zeros(S), 0.1)
    assert host.counts[:, 0].sum() == index * S * N + 1 and host.counts[slot, 0] == index + 1
    return float(host.goal[slot, 0]), float(host.goal[slot, 1]), int(host.log[slot, 0]["attempts"])


def test_generator_known_answers(L):
    """three (seed, slot, index, k) as literals; the restatement and the host's draw give exactly them"""
    assert mr.sm(0) == 0xE220A8397B1DCDAF and mr.sm(1) == 0x910A2DEC89025CC1      # splitmix64's published first outputs for states 0 and 1
    cfg = mr.make_cfg(PER_AGENT, lo=(0.0, 0.0), hi=(1.0, 1.0))
    for seed, slot, index, k, h1, bx, by, xh, yh in KNOWN:
        cfg.seed = seed
        assert mr.sm((mr.sm(seed ^ mr.sm(slot)) + index) & mr.M64) == h1
        assert mr.sm((h1 + 2 * k) & mr.M64) == bx and mr.sm((h1 + 2 * k + 1) & mr.M64) == by
        x, y = float.fromhex(xh), float.fromhex(yh)
        assert x == (bx >> 11) / 2.0 ** 53 and y == (by >> 11) / 2.0 ** 53
        assert mr.candidate(cfg, slot, index, k) == (x, y)
        assert _host_draw(seed, slot, index, k) == (x, y, k + 1)
    # all tests off: the host takes candidate 0 of (slot 3, index 1)
    cfg = mr.make_cfg(PER_AGENT, seed=99, max_goals=2, min_interval=0.0, min_dist_self=0.0, tether_max=0.0, close_pos=0.0, close_goal=0.0)
    N = 5
    goals = np.zeros((N, 3)); goals[:, 2] = 1.0
    host = mission.HostMission(cfg, 1, N, mr.circle_bases(N), goals)
    pos = np.zeros((N, 2, 3)); pos[:, :, 2] = 1.0; pos[:3] += 5.0
    s_end = np.zeros((N, 12)); s_end[:, :3] = pos[:, 1]
    host.step(pos, s_end, np.zeros(1), 0.1)
    assert host.counts[:, 0].tolist() == [1, 1, 1, 2, 2]
    for a in (3, 4):
        assert tuple(host.goal[a]) == mr.candidate(cfg, a, 1, 0) + (1.0,)
        assert host.log[a, 0]["attempts"] == 1 and host.log[a, 0]["outcome"] == abi.NEP_MISSION_REACHED and host.log[a, 0]["index"] == 0


def _one_agent_reaching(cfg, keep=None, N=1, pb=None):
    goals = np.zeros((N, 3)); goals[:, 2] = cfg.goal_z
    pb = np.zeros((N, 2)) if pb is None else pb
    host = mission.HostMission(cfg, 1, N, pb, goals, keepouts=keep)
    ref = mr.RefMission(cfg, 1, N, pb, goals, keepouts=keep)
    pos = np.zeros((N, 2, 3)); pos[:, :, 2] = cfg.goal_z
    s_end = np.zeros((N, 12)); s_end[:, 2] = cfg.goal_z
    return host, ref, pos, s_end


def test_candidate_on_an_edge_is_refused(L):
    """a keep-out polygon with candidate 0 exactly on an edge (a vertical edge through its x): refused, the goal is candidate k > 0"""
    cfg = mr.make_cfg(PER_AGENT, seed=5, max_goals=2, min_interval=0.0, min_dist_self=1.0, tether_max=0.0, close_pos=0.0, close_goal=0.0)
    x0, y0 = mr.candidate(cfg, 0, 1, 0)
    assert np.hypot(x0, y0) >= 1.0
    far = [np.array([[x0 - 0.5, y0 - 3.0], [x0 - 0.25, y0 - 3.0], [x0 - 0.25, y0 - 2.0]])]      # does not hold the candidate: accepted
    host, ref, pos, s_end = _one_agent_reaching(cfg, [far])
    host.step(pos, s_end, np.zeros(1), 0.1)
    assert tuple(host.goal[0, :2]) == (x0, y0)
    edge = [np.array([[x0, y0 - 1.0], [x0, y0 + 1.0], [x0 - 1.0, y0]])]      # counter-clockwise; the edge x = x0 holds the candidate
    assert mr.in_polygon(x0, y0, edge[0]) and not mr.in_polygon(np.nextafter(x0, 100.0), y0, edge[0])
    host, ref, pos, s_end = _one_agent_reaching(cfg, [edge])
    for m in (host, ref):
        m.step(pos, s_end, np.zeros(1), 0.1)
    mr.assert_same(host, ref)
    assert tuple(host.goal[0, :2]) != (x0, y0) and host.log[0, 0]["attempts"] > 1 and host.counts[0].tolist() == [2, 1, 0, 0]


def test_draw_needs_a_second_batch(L):
    cfg, pb, k_win = mr.second_batch_case()
    cfg.min_dist_self = 0.25
    goals = np.array([[pb[0, 0] + 20.0, pb[0, 1], cfg.goal_z]])
    host = mission.HostMission(cfg, 1, 1, pb, goals); ref = mr.RefMission(cfg, 1, 1, pb, goals)
    pos = np.repeat(goals[:, None, :], 2, axis=1); s_end = np.zeros((1, 12)); s_end[:, :3] = goals
    for m in (host, ref):
        m.step(pos, s_end, np.zeros(1), 0.1)
    mr.assert_same(host, ref)
    assert ref.ev["second_batch"] == 1 and host.log[0, 0]["attempts"] == k_win + 1 >= 65
    assert tuple(host.goal[0, :2]) == mr.candidate(cfg, 0, 1, k_win)


def test_no_goal_keeps_the_goal_and_raises_the_flag(L):
    cfg = mr.make_cfg(PER_AGENT, max_goals=3, max_attempts=64, min_interval=0.0, min_dist_self=1.0, tether_max=1e-9, close_pos=0.0, close_goal=0.0, log_cap=4)
    host, ref, pos, s_end = _one_agent_reaching(cfg, pb=np.array([[50.0, 50.0]]))
    for m in (host, ref):
        m.step(pos, s_end, np.zeros(1), 0.1)
    mr.assert_same(host, ref)
    assert host.goal[0].tolist() == [0.0, 0.0, cfg.goal_z] and host.flags[0] == abi.NEP_FLEET_FLAG_GOAL == 8
    assert host.counts[0].tolist() == [2, 1, 0, 1] and host.t_issue[0] == 0.1 and host.log_n[0] == 2
    assert [int(r["outcome"]) for r in host.log[0, :2]] == [abi.NEP_MISSION_REACHED, abi.NEP_MISSION_NO_GOAL]
    assert host.log[0, 0]["attempts"] == 64 and host.log[0, 1]["index"] == 1 and host.log[0, 1]["goal"].tolist() == [0.0, 0.0, cfg.goal_z]


def test_log_wraps(L):
    cfg = mr.make_cfg(PER_AGENT, max_goals=6, log_cap=2, min_interval=0.0, min_dist_self=1.0, tether_max=0.0, close_pos=0.0, close_goal=0.0)
    host, ref, pos, s_end = _one_agent_reaching(cfg)
    t = np.zeros(1)
    for r in range(5):
        pos[:] = host.goal[:, None, :]; s_end[:, :3] = host.goal      # jumps onto every new goal
        for m in (host, ref):
            m.step(pos, s_end, t, 0.1)
        t = t + 0.1
    mr.assert_same(host, ref)
    assert host.log_n[0] == 5 and host.counts[0].tolist() == [6, 5, 0, 0]
    assert sorted(int(r["index"]) for r in host.log[0]) == [3, 4] and host.log[0, 4 % 2]["index"] == 4 and host.log[0, 3 % 2]["index"] == 3


def test_mission_abi(L):
    assert L.nep_abi_sizeof(20) == C.sizeof(abi.nep_mission_cfg) == 136
    assert L.nep_abi_sizeof(21) == C.sizeof(abi.nep_mission_leg) == abi.MISSION_LEG_DTYPE.itemsize == 64
    assert L.nep_abi_sizeof(16) == -1 and L.nep_abi_sizeof(19) == -1 and L.nep_abi_sizeof(22) == -1
    assert L.nep_abi_sizeof(18) == 80 and abi.NEP_FLEET_N_COUNTERS == 8
    hdr = open(os.path.join(ROOT, "include", "neptune_fleet.h")).read()
    for name in ("NEP_MISSION_PER_AGENT", "NEP_MISSION_FLEET_RUNS", "NEP_MISSION_REACHED", "NEP_MISSION_TIMED_OUT", "NEP_MISSION_NO_GOAL",
                 "NEP_FLEET_FLAG_GOAL", "NEP_MISSION_MAX_POLY", "NEP_MISSION_MAX_VERT"):
        import re
        m = re.search(r"#define %s (\d+)\b" % name, hdr)
        assert m and int(m.group(1)) == getattr(abi, name), name
    for name in ("nep_batch_fleet_mission_keepout", "nep_batch_fleet_mission_init", "nep_batch_fleet_mission", "nep_batch_fleet_mission_state",
                 "nep_batch_fleet_mission_log", "nep_mission_step"):
        assert name in _lib.FLEET_EXPORTS and getattr(L, name)


def test_contracts_without_a_handle(L):
    """nep_mission_step's argument checks; the device entry points fail loudly (no device: NEP_E_HIP; a device and no handle: NEP_E_ARG)"""
    cfg = mr.make_cfg(PER_AGENT)
    host, _, pos, s_end = _one_agent_reaching(cfg)
    assert L.nep_mission_step(None, None) == -1
    for field, bad in (("mode", 3), ("max_goals", 0), ("max_attempts", 100), ("max_attempts", 8192), ("log_cap", -1), ("timeout", 0.0), ("arrive_radius", -1.0),
                       ("close_pos", -0.5)):
        c = mr.make_cfg(PER_AGENT)
        setattr(c, field, bad)
        host.cfg = c
        with pytest.raises(_lib.BackendError):
            host.step(pos, s_end, np.zeros(1), 0.1)
    c = mr.make_cfg(PER_AGENT); c.hi[0] = c.lo[0]
    host.cfg = c
    with pytest.raises(_lib.BackendError):
        host.step(pos, s_end, np.zeros(1), 0.1)
    import torch
    want = -1 if torch.cuda.is_available() else -3      # NEP_E_ARG / NEP_E_HIP
    assert L.nep_batch_fleet_mission_init(None, C.byref(cfg), None) == want
    assert L.nep_batch_fleet_mission(None, None) == want
    assert L.nep_batch_fleet_mission_keepout(None, 0, 0, None, None) == want
    assert L.nep_batch_fleet_mission_state(None, None, None, None, None, None, None, None, None) == want
    assert L.nep_batch_fleet_mission_log(None, None, None) == want


def test_mission_spec_defaults():
    """the reference's values per mode (neptune_ros.cpp:1047-1102; benchmark_mtlp.py:167-281)"""
    from neptune_amd import scene
    p = scene.scaled_params(8, 4)
    a = mission.mission_cfg(mission.MissionSpec("agent"), p)
    assert (a.mode, a.min_interval, a.timeout, a.rest_v, a.rest_a, a.min_dist_self, a.arrive_radius) == (PER_AGENT, 5.0, 45.0, 0.1, 0.1, 5.0, 0.5)
    assert a.tether_max == 0.85 * p.tether_length and a.lo[0] == p.x_min + 3 * p.drone_radius and a.hi[1] == p.y_max - 3 * p.drone_radius
    assert a.close_pos == 0.0 and a.close_goal == 0.0 and mission.uses_keepouts(mission.MissionSpec("agent"))
    r = mission.mission_cfg(mission.MissionSpec("runs"), p)
    assert (r.mode, r.timeout, r.arrive_radius, r.close_pos, r.close_goal, r.min_dist_self) == (RUNS, 40.0, 0.5, 0.75, 3.0, 0.0)
    assert r.tether_max == p.tether_length and r.lo[0] == p.x_min + 4.0 and not mission.uses_keepouts(mission.MissionSpec("runs"))
    sc = scene.make_scene(5, 3, seed=0)
    ko = scene.keepout_polygons(sc)
    assert len(ko) == 3
    for q, raw in zip(ko, sc["statics_raw"]):
        d = 4 * sc["par"].drone_radius
        assert np.allclose(q.min(0), np.asarray(raw).min(0) - d) and np.allclose(q.max(0), np.asarray(raw).max(0) + d)
        assert all(mr.in_polygon(float(v[0]), float(v[1]), q) for v in np.asarray(raw))      # counter-clockwise, holds the footprint


def test_rules_alone_need_few_attempts(L):
    """The rules alone, with the reference's values, in worlds of 8 + 4, 16 + 8 and 64 + 20: 20 000 draws per rule set, every one
    within the FIRST batch of 64 candidates (a cap of 256 is then four times what is ever used) and no draw without a goal.  Why
    64 is a safe bound: the keep-outs and the other agents' discs cover well under half of the box the goals are drawn in, so a
    candidate passes with p > 1/2 under autoCMD's rules and — with up to 63 goals of 3 m already drawn — p > 1/4 under
    benchmark_mtlp's; 64 candidates all failing has probability below 0.75^64 = 1e-8 per draw, 2e-4 over 20 000.  Both rule sets are
    drawn in mode PER_AGENT (one rule set for both modes), where the log holds the attempts of every single draw."""
    from neptune_amd import scene
    worst = {}
    for rules in ("agent", "runs"):
        draws = 0
        for N, M, calls in ((8, 4, 300), (16, 8, 300), (64, 20, 200)):
            p = scene.scaled_params(N, M)
            raw, _ = scene.random_static_obstacles(p, np.random.default_rng(N))
            cfg = mission.mission_cfg(mission.MissionSpec(rules, goals=10 ** 6, seed=5, log_cap=1), p)
            cfg.mode, cfg.min_interval, cfg.timeout, cfg.rest_v, cfg.rest_a = PER_AGENT, 0.0, 1e9, 0.1, 0.1
            keep = [scene.keepout_polygons(dict(par=p, statics_raw=raw))] if rules == "agent" else None
            goals = np.zeros((N, 3)); goals[:, :2] = 0.8 * p.pb; goals[:, 2] = p.goal_height
            host = mission.HostMission(cfg, 1, N, p.pb, goals, keepouts=keep)
            for r in range(calls):      # every agent jumps onto its goal: every call ends every leg and draws N goals
                pos = np.repeat(host.goal[:, None, :], 2, axis=1); s_end = np.zeros((N, 12)); s_end[:, :3] = host.goal
                host.step(pos, s_end, np.full(1, 0.1 * r), 0.1)
                worst[rules] = max(worst.get(rules, 0), int(host.log["attempts"].max()))
            assert host.counts[:, 3].sum() == 0 and (host.counts[:, 0] == calls + 1).all()
            draws += N * calls
        assert draws == 20000
    print("most attempts of a draw:", worst)
    assert worst["agent"] <= 64 and worst["runs"] <= 64, worst


def test_host_form_under_sanitizers(tmp_path):
    """tests/cpp/mission_check.cpp drives mission_host.cpp (host code only, its own main) through seeded walks in both modes, built
    with -fsanitize=address,undefined"""
    exe = str(tmp_path / "mission_check")
    src = [os.path.join(ROOT, "tests", "cpp", "mission_check.cpp"), os.path.join(ROOT, "neptune_amd", "csrc", "mission_host.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include")] + src + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "mission_check ok" in r.stdout, (r.stdout, r.stderr)
