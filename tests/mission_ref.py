"""A restatement of the fleet's mission controller (include/neptune_fleet.h, "missions") in Python ints and floats — IEEE doubles,
one rounding per operation, the header's text as the specification — and the seeded walks both the CPU and the GPU tests drive the
host form (nep_mission_step) and the kernel through.  Not a test module."""
import math

import numpy as np

from neptune_amd import abi

M64 = (1 << 64) - 1


def sm(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def candidate(cfg, gslot, index, k):
    h1 = sm((sm(cfg.seed ^ sm(gslot)) + index) & M64)
    ux = float(sm((h1 + 2 * k) & M64) >> 11) * 2.0 ** -53
    uy = float(sm((h1 + 2 * k + 1) & M64) >> 11) * 2.0 ** -53
    return cfg.lo[0] + (cfg.hi[0] - cfg.lo[0]) * ux, cfg.lo[1] + (cfg.hi[1] - cfg.lo[1]) * uy


def n2(dx, dy):
    return math.sqrt(dx * dx + dy * dy)


def n3(dx, dy, dz):
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def in_polygon(x, y, q):
    """on or inside a counter-clockwise convex polygon: every edge cross product >= 0"""
    n = len(q)
    for v in range(n):
        ax, ay = float(q[v][0]), float(q[v][1]); bx, by = float(q[(v + 1) % n][0]), float(q[(v + 1) % n][1])
        ex, ey, wx, wy = bx - ax, by - ay, x - ax, y - ay
        if not (ex * wy - ey * wx >= 0.0):
            return False
    return True


class RefMission:
    """the same arrays as neptune_amd.mission.HostMission, moved by Python arithmetic; `ev` counts what the walk has exercised"""

    def __init__(self, cfg, S, N, pb, goals, t0=0.0, keepouts=None):
        self.cfg, self.S, self.N = cfg, S, N
        n = S * N
        self.pb = np.asarray(pb, dtype=np.float64).reshape(N, 2)
        self.goal = np.array(goals, dtype=np.float64).reshape(n, 3)
        self.done = np.zeros(n, dtype=np.int32); self.flags = np.zeros(n, dtype=np.int32)
        self.t_issue = np.full(n, float(t0)); self.length = np.zeros(n); self.completed = np.zeros(n, dtype=np.int32)
        self.counts = np.zeros((n, 4), dtype=np.int32); self.counts[:, 0] = 1
        self.sums = np.zeros((n, 2))
        self.scene = np.zeros((S, 4), dtype=np.int32); self.t_run = np.full(S, float(t0))
        self.per_agent = cfg.mode == abi.NEP_MISSION_PER_AGENT
        owners = n if self.per_agent else S
        self.log = np.zeros((owners, max(int(cfg.log_cap), 1)), dtype=abi.MISSION_LEG_DTYPE)
        self.log_n = np.zeros(owners, dtype=np.int32)
        self.keep = [[] if keepouts is None else keepouts[s] for s in range(S)]
        self.ev = dict(reached=0, timed_out=0, held_interval=0, held_v=0, held_a=0, timeout_moving=0, uncompleted=0, quota=0, no_goal=0,
                       second_batch=0, run_ok=0, run_failed=0, max_k=0)

    def _log(self, owner, who, index, outcome, attempts, t_issue, t_end, length, g):
        cap = int(self.cfg.log_cap)
        if cap > 0:
            r = self.log[owner, int(self.log_n[owner]) % cap]
            r["who"], r["index"], r["outcome"], r["attempts"] = who, index, outcome, attempts
            r["t_issue"], r["t_end"], r["length"] = t_issue, t_end, length
            r["goal"] = g
        self.log_n[owner] += 1

    def _draw(self, s, a, end, new):
        c, N = self.cfg, self.N
        i = s * N + a
        index = int(self.counts[i, 0])
        for k in range(c.max_attempts):
            x, y = candidate(c, i, index, k)
            if c.min_dist_self != 0.0 and not n2(x - end[a][0], y - end[a][1]) >= c.min_dist_self:
                continue
            if c.tether_max != 0.0 and not n2(x - float(self.pb[a, 0]), y - float(self.pb[a, 1])) <= c.tether_max:
                continue
            if any(in_polygon(x, y, q) for q in self.keep[s]):
                continue
            if c.close_pos != 0.0 and any(not n3(x - end[j][0], y - end[j][1], c.goal_z - end[j][2]) >= c.close_pos for j in range(N)):
                continue
            if c.close_goal != 0.0 and any(j in new and not n3(x - new[j][0], y - new[j][1], c.goal_z - new[j][2]) >= c.close_goal for j in range(a)):
                continue
            self.ev["second_batch"] += k >= 64
            self.ev["max_k"] = max(self.ev["max_k"], k)
            return k, x, y
        return -1, 0.0, 0.0

    def _issue(self, i, t_end, k, x, y):
        if k < 0:
            self.counts[i, 3] += 1; self.flags[i] |= abi.NEP_FLEET_FLAG_GOAL; self.ev["no_goal"] += 1
        else:
            self.goal[i] = [x, y, self.cfg.goal_z]
        self.counts[i, 0] += 1
        self.t_issue[i] = t_end; self.length[i] = 0.0; self.completed[i] = 0; self.done[i] = 0

    def step(self, pos, s_end, t_now, dc):
        c, N = self.cfg, self.N
        T = pos.shape[1] - 1
        for s in range(self.S):
            if self.scene[s, 3]:
                continue
            t_end = float(t_now[s])
            for _ in range(T):
                t_end += float(dc)
            end = [[float(v) for v in s_end[s * N + a, :3]] for a in range(N)]
            trig = {}
            for a in range(N):
                i = s * N + a
                if self.per_agent and int(self.counts[i, 1] + self.counts[i, 2]) >= c.max_goals:
                    continue
                g = [float(v) for v in self.goal[i]]
                ln, comp = float(self.length[i]), int(self.completed[i])
                for q in range(1, T + 1):
                    p, pp = [float(v) for v in pos[i, q]], [float(v) for v in pos[i, q - 1]]
                    d = n3(p[0] - g[0], p[1] - g[1], p[2] - g[2]); step = n3(p[0] - pp[0], p[1] - pp[1], p[2] - pp[2])
                    if self.per_agent:
                        if d > c.arrive_radius:
                            ln = ln + step
                    else:
                        if not comp:
                            ln = ln + step
                        was = comp
                        comp = 1 if d < c.arrive_radius else 0
                        self.ev["uncompleted"] += was and not comp
                self.length[i] = ln; self.completed[i] = comp
                if not self.per_agent:
                    continue
                e = [float(v) for v in s_end[i]]
                el = t_end - float(self.t_issue[i])
                v_xy, a_xy = n2(e[3], e[4]), n2(e[6], e[7])
                at_goal = n3(e[0] - g[0], e[1] - g[1], e[2] - g[2]) < c.arrive_radius
                if el < c.min_interval:
                    self.ev["held_interval"] += at_goal and v_xy <= c.rest_v and a_xy <= c.rest_a
                    continue
                if (el < c.timeout and v_xy > c.rest_v) or a_xy > c.rest_a:
                    self.ev["held_v"] += at_goal and a_xy <= c.rest_a
                    self.ev["held_a"] += a_xy > c.rest_a and (at_goal or el > c.timeout)
                    continue
                if at_goal:
                    trig[a] = abi.NEP_MISSION_REACHED
                elif el > c.timeout:
                    trig[a] = abi.NEP_MISSION_TIMED_OUT
                    self.ev["timeout_moving"] += v_xy > c.rest_v
            if self.per_agent:
                new = {}
                for a in sorted(trig):
                    i = s * N + a
                    oc = trig[a]
                    self.ev["reached" if oc == abi.NEP_MISSION_REACHED else "timed_out"] += 1
                    el = t_end - float(self.t_issue[i])
                    index = int(self.counts[i, 0]) - 1
                    self.counts[i, 1 if oc == abi.NEP_MISSION_REACHED else 2] += 1
                    self.sums[i, 0] = float(self.sums[i, 0]) + el; self.sums[i, 1] = float(self.sums[i, 1]) + float(self.length[i])
                    draws = int(self.counts[i, 1] + self.counts[i, 2]) < c.max_goals
                    k, x, y = self._draw(s, a, end, new) if draws else (-1, 0.0, 0.0)
                    self._log(i, i, index, oc, 0 if not draws else (k + 1 if k >= 0 else c.max_attempts), float(self.t_issue[i]), t_end, float(self.length[i]),
                              self.goal[i].copy())
                    if not draws:
                        self.ev["quota"] += 1
                        continue
                    if k < 0:
                        self._log(i, i, index + 1, abi.NEP_MISSION_NO_GOAL, c.max_attempts, t_end, t_end, 0.0, self.goal[i].copy())
                    else:
                        new[a] = (x, y, c.goal_z)
                    self._issue(i, t_end, k, x, y)
                if all(int(self.counts[s * N + a, 1] + self.counts[s * N + a, 2]) >= c.max_goals for a in range(N)):
                    self.scene[s, 3] = 1
                continue
            el = t_end - float(self.t_run[s])
            ok = all(int(self.completed[s * N + a]) for a in range(N))
            if not (ok or el > c.timeout):
                continue
            self.ev["run_ok" if ok else "run_failed"] += 1
            total = 0.0
            for a in range(N):
                total = total + float(self.length[s * N + a])
            draws = int(self.scene[s, 0]) + 1 < c.max_goals
            new, attempts = {}, 0
            for a in range(N):
                i = s * N + a
                self.counts[i, 1 if self.completed[i] else 2] += 1
                self.sums[i, 0] = float(self.sums[i, 0]) + el; self.sums[i, 1] = float(self.sums[i, 1]) + float(self.length[i])
                if not draws:
                    continue
                k, x, y = self._draw(s, a, end, new)
                attempts += k + 1 if k >= 0 else c.max_attempts
                if k >= 0:
                    new[a] = (x, y, c.goal_z)
                self._issue(i, t_end, k, x, y)
            self._log(s, s, int(self.scene[s, 0]), abi.NEP_MISSION_REACHED if ok else abi.NEP_MISSION_TIMED_OUT, attempts, float(self.t_run[s]), t_end,
                      total / float(N), np.zeros(3))
            self.scene[s, 1 if ok else 2] += 1
            self.scene[s, 0] += 1
            if int(self.scene[s, 0]) >= c.max_goals:
                self.scene[s, 3] = 1
                self.ev["quota"] += 1
            self.t_run[s] = t_end

    def state(self):
        return dict(goal=self.goal, t_issue=self.t_issue, length=self.length, completed=self.completed, counts=self.counts, sums=self.sums,
                    scene=self.scene, t_run=self.t_run)


FIELDS = ("goal", "done", "flags", "t_issue", "length", "completed", "counts", "sums", "scene", "t_run", "log", "log_n")


def assert_same(a, b, what=""):
    """every field of two mission chains (HostMission / RefMission), byte for byte"""
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.tobytes() == y.tobytes(), (what, f, x, y)


def make_cfg(mode, max_goals=3, max_attempts=256, log_cap=4, seed=7, lo=(-9.0, -9.0), hi=(9.0, 9.0), goal_z=1.0, arrive_radius=0.5, min_interval=0.5,
             timeout=2.0, rest_v=0.1, rest_a=0.1, min_dist_self=3.0, tether_max=14.0, close_pos=0.5, close_goal=1.0):
    c = abi.nep_mission_cfg()
    c.mode, c.max_goals, c.max_attempts, c.log_cap, c.seed = mode, max_goals, max_attempts, log_cap, seed
    c.lo[0], c.lo[1], c.hi[0], c.hi[1] = lo[0], lo[1], hi[0], hi[1]
    c.goal_z, c.arrive_radius, c.min_interval, c.timeout, c.rest_v, c.rest_a = goal_z, arrive_radius, min_interval, timeout, rest_v, rest_a
    c.min_dist_self, c.tether_max, c.close_pos, c.close_goal = min_dist_self, tether_max, close_pos, close_goal
    return c


def second_batch_case():
    """a configuration whose first draw of slot 0 passes only at a candidate k >= 64: a tether disc that the first 64 candidates miss"""
    cfg = make_cfg(abi.NEP_MISSION_PER_AGENT, seed=11, max_goals=2, min_interval=0.0, min_dist_self=1.0, tether_max=1.0, close_pos=0.0, close_goal=0.0)
    c = [candidate(cfg, 0, 1, k) for k in range(256)]
    k_win = 100
    others = np.array(c[:k_win])
    r = 0.5 * np.hypot(others[:, 0] - c[k_win][0], others[:, 1] - c[k_win][1]).min()
    cfg.tether_max = float(r)
    pb = np.array([[c[k_win][0], c[k_win][1]]])
    return cfg, pb, k_win


def random_keepouts(rng, S, n_poly):
    """n_poly counter-clockwise convex polygons of 3..8 vertices per scene (vertices of a circle: convex by construction)"""
    out = []
    for _ in range(S):
        polys = []
        for j in range(n_poly):
            nv = 3 + (j + int(rng.integers(0, 6))) % 6
            c = rng.uniform(-7.0, 7.0, 2); r = rng.uniform(0.8, 2.0)
            th = np.sort(rng.uniform(0.0, 2 * np.pi, nv))
            th = th + np.arange(nv) * 1e-3      # (no repeated vertex)
            polys.append(np.stack([c[0] + r * np.cos(th), c[1] + r * np.sin(th)], axis=1))
        out.append(polys)
    return out


def circle_bases(N, radius=10.0):
    th = 2 * np.pi * np.arange(N) / N
    return np.stack([radius * np.cos(th), radius * np.sin(th)], axis=1)


class Walk:
    """A seeded walk of S*N agents: per call every agent either heads for its goal (the chain's current one), sits on it — at rest,
    still moving, or still accelerating —, drifts off it again, or wanders.  Gives the tick positions and end states of one call."""

    def __init__(self, seed, S, N, T, goal_z=1.0):
        self.rng = np.random.default_rng(seed)
        self.S, self.N, self.T = S, N, T
        self.lazy = np.arange(S * N) % 4 == 3      # every fourth agent never heads for its goal: its legs time out
        self.p = np.zeros((S * N, 3)); self.p[:, :2] = self.rng.uniform(-8.0, 8.0, (S * N, 2)); self.p[:, 2] = goal_z

    def call(self, goal):
        n, T, rng = self.S * self.N, self.T, self.rng
        pos = np.zeros((n, T + 1, 3)); s_end = np.zeros((n, 12))
        for i in range(n):
            pos[i, 0] = self.p[i]
            kind = rng.choice(6, p=[0.25, 0.35, 0.1, 0.1, 0.1, 0.1])
            if self.lazy[i]:
                kind = 4 + kind % 2
            target = goal[i] if kind < 4 else self.p[i] + np.append(rng.uniform(-2.0, 2.0, 2), 0.0)
            if kind == 0:      # part of the way
                target = self.p[i] + (goal[i] - self.p[i]) * rng.uniform(0.2, 0.9)
            for q in range(1, T + 1):
                pos[i, q] = self.p[i] + (target - self.p[i]) * (q / T)
            if kind == 1 and rng.uniform() < 0.5:      # stops just short of / just past the goal: inside the radius, not on it
                pos[i, T, :2] += rng.uniform(-0.2, 0.2, 2)
            s_end[i, :3] = pos[i, T]
            if kind == 2 or kind == 4:
                s_end[i, 3:5] = rng.uniform(0.2, 1.0, 2)
            if kind == 3 or (kind == 5 and rng.uniform() < 0.5):
                s_end[i, 6:8] = rng.uniform(0.2, 1.0, 2)
            if kind in (0, 5) and rng.uniform() < 0.3:
                s_end[i, 3:5] = rng.uniform(0.0, 0.05, 2)
            self.p[i] = pos[i, T]
        return pos, s_end
