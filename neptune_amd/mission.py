"""Missions of the device fleet loop (include/neptune_fleet.h: nep_batch_fleet_mission): successive goals, timeouts and leg
records.  MissionSpec carries the reference's values per mode — NeptuneRos::autoCMD (neptune_ros.cpp:1047-1102) and
scripts/benchmark_mtlp.py:167-281, and "together", scripts/auto_commands_together.py:154-182, the position-exchange driver, whose
goals come from a table (MissionSpec.script, exchange_script) —, mission_cfg turns it into the C record for a scene's world, and HostMission is the host chain
of nep_mission_step that the device is compared with byte for byte."""
import ctypes as C
import dataclasses
import math

import numpy as np

from . import abi
from ._lib import check, lib


@dataclasses.dataclass
class MissionSpec:
    """mode "agent" (autoCMD), "runs" (benchmark_mtlp) or "together" (auto_commands_together); None takes the reference's value
    for the mode ("together": "runs"'s wherever the driver has none).  script: None (goals are drawn) or the goals every new leg
    takes in turn, [N][G][3] (every scene the same) or [S][N][G][3]: leg i >= 1 of an agent gets row (i - 1) mod G."""
    mode: str = "agent"
    goals: int = 2                    # legs per agent ("agent") or runs per scene ("runs")
    seed: int = 1
    max_attempts: int = 256
    log_cap: int = 16
    arrive_radius: float = None       # 0.5 m in both scripts; "together": sqrt(0.5), the half side of its square
    min_interval: float = None        # "agent": 5 s
    timeout: float = None             # "agent": 45 s, "runs": 40 s, "together": none (+infinity in the C record)
    rest_v: float = None              # "agent": 0.1 m/s
    rest_a: float = None              # "agent": 0.1 m/s^2
    min_dist_self: float = None       # "agent": 5 m
    tether_factor: float = None       # tether_max = factor * tether_length; "agent": 0.85, "runs": 1.0
    shrink: float = None              # the world less this on every side; "agent": 3 * drone_radius, "runs": 4 m
    close_range: float = None         # "runs": 3 m -> close_pos = close_range / 4, close_goal = close_range
    keepouts: bool = None             # "agent": the scene's keep-out polygons (scene.keepout_polygons); "runs": none
    script: object = None             # see above


def mission_cfg(spec, par):
    """MissionSpec + a scene's Params -> abi.nep_mission_cfg"""
    if spec.mode not in MODES:
        raise ValueError("mission mode must be 'agent', 'runs' or 'together'")
    agent, together = spec.mode == "agent", spec.mode == "together"
    pick = lambda v, a, r: (a if agent else r) if v is None else v      # noqa: E731
    shrink = pick(spec.shrink, 3.0 * par.drone_radius, 4.0)
    close = pick(spec.close_range, 0.0, 3.0)
    c = abi.nep_mission_cfg()
    c.mode = MODES[spec.mode]
    c.max_goals, c.max_attempts, c.log_cap, c.seed = spec.goals, spec.max_attempts, spec.log_cap, spec.seed
    c.lo[0], c.lo[1], c.hi[0], c.hi[1] = par.x_min + shrink, par.y_min + shrink, par.x_max - shrink, par.y_max - shrink
    c.goal_z = par.goal_height
    c.arrive_radius = pick(spec.arrive_radius, 0.5, math.sqrt(0.5) if together else 0.5)
    c.min_interval = pick(spec.min_interval, 5.0, 0.0)
    c.timeout = pick(spec.timeout, 45.0, math.inf if together else 40.0)
    c.rest_v, c.rest_a = pick(spec.rest_v, 0.1, 0.0), pick(spec.rest_a, 0.1, 0.0)
    c.min_dist_self = pick(spec.min_dist_self, 5.0, 0.0)
    c.tether_max = pick(spec.tether_factor, 0.85, 1.0) * par.tether_length
    c.close_pos, c.close_goal = close / 4.0, close
    return c


MODES = dict(agent=abi.NEP_MISSION_PER_AGENT, runs=abi.NEP_MISSION_FLEET_RUNS, together=abi.NEP_MISSION_FLEET_TOGETHER)


def script_rows(spec, S, N):
    """MissionSpec.script for S scenes of N agents -> [S][N][G][3] float64, or None.  ValueError for another shape, G = 0 or a
    coordinate that is not finite."""
    if spec is None or spec.script is None:
        return None
    g = np.asarray(spec.script, dtype=np.float64)
    if g.ndim == 3:
        g = np.broadcast_to(g, (S,) + g.shape)
    if g.ndim != 4 or g.shape[0] != S or g.shape[1] != N or g.shape[2] < 1 or g.shape[3] != 3:
        raise ValueError("MissionSpec.script must be [N][G][3] or [S][N][G][3] with G >= 1 (S = %d, N = %d)" % (S, N))
    if not np.isfinite(g).all():
        raise ValueError("MissionSpec.script holds a coordinate that is not finite")
    return np.ascontiguousarray(g)


def spec_plain(spec):
    """a MissionSpec as plain data (a checkpoint's options): (the fields but the script, the script as nested lists or None)"""
    if spec is None:
        return None, None
    d = {f.name: getattr(spec, f.name) for f in dataclasses.fields(spec) if f.name != "script"}
    return d, None if spec.script is None else np.asarray(spec.script, dtype=np.float64).tolist()


def exchange_script(N, radius=10.0, z=1.0):
    """The two goal lists of auto_commands_together.py with init_pos_as_circle, in the order the driver publishes them — goals1
    first —, as a script [N][2][3]: agent x gets (-R cos(2 pi x / N + pi), -R sin(2 pi x / N + pi)), then the antipode
    (-R cos(2 pi x / N), -R sin(2 pi x / N)), with R = radius, and radius + 0.7 for the odd x of a fleet of 8."""
    out = np.zeros((N, 2, 3))
    one = 2 * math.pi / N
    for x in range(N):
        r = radius + 0.7 if N == 8 and x % 2 == 1 else radius
        out[x, 0, :2] = -r * math.cos(one * x + math.pi), -r * math.sin(one * x + math.pi)
        out[x, 1, :2] = -r * math.cos(one * x), -r * math.sin(one * x)
    out[:, :, 2] = z
    return out


def effort_slack(effort):
    """DeviceFleetLoop's effort option — False / None, True (1e-6, the flight-audit tests' bar) or a slack >= 0 -> the slack or None"""
    if effort is None or effort is False:
        return None
    s = 1e-6 if effort is True else float(effort)
    if not (math.isfinite(s) and s >= 0.0):
        raise ValueError("effort must be False, True or a finite slack >= 0")
    return s


def effort_step(v_max, a_max, j_max, dc, round_ticks, ring, head, size, done, slack, out):
    """nep_effort_step, the host form of one slot: ring [cap][12] float64; out a 1-element abi.EFFORT_DTYPE array, accumulated into"""
    ring = np.ascontiguousarray(ring, dtype=np.float64)
    assert ring.ndim == 2 and ring.shape[1] == 12 and out.dtype == abi.EFFORT_DTYPE and out.size == 1 and out.flags.c_contiguous
    check(lib().nep_effort_step(float(v_max), float(a_max), float(j_max), float(dc), int(round_ticks), ring.ctypes.data, int(head), int(size), ring.shape[0],
                                int(done), float(slack), out.ctypes.data))


def summarize_effort(eff, N):
    """per scene, from a [slots] abi.EFFORT_DTYPE array: the mean jerk integral per agent (benchmark_multi_direct.py's "average jerk"),
    the largest velocity / acceleration / jerk component flown, and the counted ticks that broke a limit"""
    e = eff.reshape(-1, N)
    return [dict(jerk_sum_mean=float(r["jerk_sum"].mean()), max_v=float(r["max_v"].max()), max_a=float(r["max_a"].max()), max_j=float(r["max_j"].max()),
                 v_viol=int(r["n_v_viol"].sum()), a_viol=int(r["n_a_viol"].sum()), j_viol=int(r["n_j_viol"].sum()), effort_ticks=int(r["n_ticks"].sum())) for r in e]


@dataclasses.dataclass
class MoveBack:
    """The reference's use_moveback_strategy (neptune_ros.cpp:1626-1636, 1291-1305; include/neptune_fleet.h:
    nep_batch_fleet_moveback): an agent with a new goal first plans towards its own base and gets the goal once it is within
    `radius` of the base or `timeout` seconds have passed.  radius <= 0: only the timer releases."""
    radius: float
    timeout: float = 10.0

    def __post_init__(self):
        import math
        self.radius, self.timeout = float(self.radius), float(self.timeout)
        if not math.isfinite(self.radius) or not math.isfinite(self.timeout) or self.timeout < 0.0:
            raise ValueError("MoveBack: radius must be finite, timeout finite and >= 0")

    @classmethod
    def reference(cls, num_agents, timeout=10.0):
        """neptune_mtlp_benchmark.yaml's radius for a fleet of num_agents: 6.33 - (N - 4) * 0.33 (<= 0 from N = 24 up)"""
        return cls(6.33 - (num_agents - 4) * 0.33, timeout)

    def cfg(self):
        return abi.nep_moveback_cfg(self.radius, self.timeout)


def check_moveback(moveback):
    """None or a MoveBack, else TypeError -> its abi.nep_moveback_cfg or None"""
    if moveback is None:
        return None
    if not isinstance(moveback, MoveBack):
        raise TypeError("moveback must be None or a neptune_amd.mission.MoveBack")
    return moveback.cfg()


def moveback_step(cfg, state, pb, t_issue, t_first, t_now, flags, start):
    """nep_moveback_step, the host form of one scene: state [n][12] float64, pb [n][2], t_issue [n] or None, flags [n] int32 and
    start [n] FE_START_DTYPE updated in place"""
    n = len(flags)
    state = np.ascontiguousarray(state, dtype=np.float64); pb = np.ascontiguousarray(pb, dtype=np.float64)
    ti = None if t_issue is None else np.ascontiguousarray(t_issue, dtype=np.float64)
    assert state.size == 12 * n and pb.size == 2 * n and (ti is None or ti.size == n) and len(start) == n
    assert flags.dtype == np.int32 and flags.flags.c_contiguous and start.dtype == abi.FE_START_DTYPE and start.flags.c_contiguous
    check(lib().nep_moveback_step(C.byref(cfg), n, state.ctypes.data, pb.ctypes.data, None if ti is None else ti.ctypes.data, float(t_first),
                                  float(t_now), flags.ctypes.data, start.ctypes.data))


def uses_keepouts(spec):
    return (spec.mode == "agent") if spec.keepouts is None else bool(spec.keepouts)


def summarize(state, log_n, N, mode):
    """per scene, from BatchBackend.fleet_mission_state(): legs (or runs) reached / timed out / without a goal, mean leg time and
    length over the ended legs, the success rate"""
    cnt = state["counts"].reshape(-1, N, 4); sums = state["sums"].reshape(-1, N, 2)
    out = []
    for s in range(cnt.shape[0]):
        ended = int(cnt[s, :, 1].sum() + cnt[s, :, 2].sum())
        d = dict(legs_issued=int(cnt[s, :, 0].sum()), legs_reached=int(cnt[s, :, 1].sum()), legs_timed_out=int(cnt[s, :, 2].sum()),
                 no_goal=int(cnt[s, :, 3].sum()), mean_leg_time=float(sums[s, :, 0].sum() / ended) if ended else None,
                 mean_leg_length=float(sums[s, :, 1].sum() / ended) if ended else None, finished=bool(state["scene"][s, 3]))
        if mode != abi.NEP_MISSION_PER_AGENT:
            ok, bad = int(state["scene"][s, 1]), int(state["scene"][s, 2])
            d.update(runs=int(state["scene"][s, 0]), runs_succeeded=ok, runs_failed=bad, success_rate=ok / (ok + bad) if ok + bad else None)
        else:
            d["success_rate"] = d["legs_reached"] / ended if ended else None
        out.append(d)
    return out


class HostMission:
    """The mission state of S scenes of N agents in host arrays, moved by nep_mission_step — the host chain.  goals [S*N][3],
    keepouts: per scene a list of counter-clockwise convex (n, 2) arrays; script: None, or [S*N][G][3] scripted goals
    (nep_mission_step_script; mode FLEET_TOGETHER goes through it with or without a script)."""

    def __init__(self, cfg, S, N, pb, goals, t0=0.0, keepouts=None, script=None):
        self.cfg, self.S, self.N = cfg, S, N
        self.script = None if script is None else np.ascontiguousarray(script, dtype=np.float64).reshape(S * N, -1, 3)
        self.by_script_call = script is not None or cfg.mode == abi.NEP_MISSION_FLEET_TOGETHER      # which entry point the chain is made of
        n = S * N
        self.pb = np.ascontiguousarray(pb, dtype=np.float64).reshape(N, 2)
        self.goal = np.ascontiguousarray(goals, dtype=np.float64).reshape(n, 3).copy()
        self.done = np.zeros(n, dtype=np.int32); self.flags = np.zeros(n, dtype=np.int32)
        self.t_issue = np.full(n, float(t0)); self.length = np.zeros(n); self.completed = np.zeros(n, dtype=np.int32)
        self.counts = np.zeros((n, 4), dtype=np.int32); self.counts[:, 0] = 1
        self.sums = np.zeros((n, 2))
        self.scene = np.zeros((S, 4), dtype=np.int32); self.t_run = np.full(S, float(t0))
        self.per_agent = cfg.mode == abi.NEP_MISSION_PER_AGENT
        self.owners = n if self.per_agent else S
        self.log = np.zeros((self.owners, max(int(cfg.log_cap), 1)), dtype=abi.MISSION_LEG_DTYPE)
        self.log_n = np.zeros(self.owners, dtype=np.int32)
        self.keep = []
        for s in range(S):
            polys = [] if keepouts is None else keepouts[s]
            off = np.zeros(len(polys) + 1, dtype=np.int32)
            for k, q in enumerate(polys):
                off[k + 1] = off[k] + len(q)
            xy = np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.float64).reshape(-1, 2) for q in polys]) if len(polys) else np.zeros((1, 2)))
            self.keep.append((len(polys), off, xy))

    def step(self, pos, s_end, t_now, dc):
        """one call for every scene: pos [S*N][T+1][3] tick positions, s_end [S*N][12], t_now [S] the scenes' clocks"""
        N = self.N
        pos = np.ascontiguousarray(pos, dtype=np.float64); s_end = np.ascontiguousarray(s_end, dtype=np.float64)
        T = pos.shape[1] - 1
        vp = lambda a, i0=0: a[i0:].ctypes.data      # noqa: E731
        for s in range(self.S):
            npoly, off, xy = self.keep[s]
            lo = s * N
            o = lo if self.per_agent else s
            sc = abi.nep_mission_scene(N, s, T, npoly, float(t_now[s]), float(dc), vp(pos, lo), vp(s_end, lo), self.pb.ctypes.data, off.ctypes.data,
                                       xy.ctypes.data, vp(self.goal, lo), vp(self.done, lo), vp(self.flags, lo), vp(self.t_issue, lo), vp(self.length, lo),
                                       vp(self.completed, lo), vp(self.counts, lo), vp(self.sums, lo), vp(self.scene, s), vp(self.t_run, s),
                                       vp(self.log, o), vp(self.log_n, o))
            if not self.by_script_call:
                check(lib().nep_mission_step(C.byref(self.cfg), C.byref(sc)))
            else:
                G = 0 if self.script is None else self.script.shape[1]
                check(lib().nep_mission_step_script(C.byref(self.cfg), C.byref(sc), G, None if self.script is None else vp(self.script, lo)))

    def state(self):
        return dict(goal=self.goal, t_issue=self.t_issue, length=self.length, completed=self.completed, counts=self.counts, sums=self.sums,
                    scene=self.scene, t_run=self.t_run)
