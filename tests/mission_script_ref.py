"""A restatement of the scripted goals, of mission mode NEP_MISSION_FLEET_TOGETHER and of the effort record (include/neptune_fleet.h,
"scripted goals" and "effort") in Python ints and floats — IEEE doubles, one rounding per operation, the header's text as the
specification.  It shares no code with the library; the unscripted draws are tests/mission_ref.py's.  Not a test module."""
import math

import numpy as np

import mission_ref as mr
from neptune_amd import abi

TOGETHER = 3


class RefScriptMission(mr.RefMission):
    """mr.RefMission with a table of goals per slot (script [S*N][G][3] or None) and the third mode.  One call = one step() of every scene."""

    def __init__(self, cfg, S, N, pb, goals, t0=0.0, keepouts=None, script=None):
        super().__init__(cfg, S, N, pb, goals, t0=t0, keepouts=keepouts)
        self.script = None if script is None else np.array(script, dtype=np.float64).reshape(S * N, -1, 3)
        self.ev.update(scripted=0, wrapped=0, stuck=0)

    def _next(self, s, a, end, new):
        """the goal of a new leg of agent a: (k, x, y, z, attempts)"""
        c = self.cfg
        i = s * self.N + a
        if self.script is not None:
            G = self.script.shape[1]
            issued = int(self.counts[i, 0])
            row = (issued - 1) % G
            self.ev["scripted"] += 1
            self.ev["wrapped"] += issued - 1 >= G
            g = self.script[i, row]
            return 0, float(g[0]), float(g[1]), float(g[2]), 0
        k, x, y = self._draw(s, a, end, new)
        return k, x, y, c.goal_z, (k + 1 if k >= 0 else c.max_attempts)

    def _issue3(self, i, t_end, k, x, y, z):
        if k < 0:
            self.counts[i, 3] += 1; self.flags[i] |= abi.NEP_FLEET_FLAG_GOAL; self.ev["no_goal"] += 1
        else:
            self.goal[i] = [x, y, z]
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
                    d = mr.n3(p[0] - g[0], p[1] - g[1], p[2] - g[2]); st = mr.n3(p[0] - pp[0], p[1] - pp[1], p[2] - pp[2])
                    if self.per_agent:
                        if d > c.arrive_radius:
                            ln = ln + st
                    elif c.mode == abi.NEP_MISSION_FLEET_RUNS:
                        if not comp:
                            ln = ln + st
                        was = comp
                        comp = 1 if d < c.arrive_radius else 0
                        self.ev["uncompleted"] += was and not comp
                    else:
                        assert c.mode == TOGETHER
                        if not comp:
                            ln = ln + st
                        dx, dy, rr = p[0] - g[0], p[1] - g[1], c.arrive_radius * c.arrive_radius
                        inside = dx * dx < rr and dy * dy < rr
                        self.ev["stuck"] += comp and not inside      # left the square again: stays completed
                        if inside:
                            comp = 1
                self.length[i] = ln; self.completed[i] = comp
                if not self.per_agent:
                    continue
                e = [float(v) for v in s_end[i]]
                el = t_end - float(self.t_issue[i])
                v_xy, a_xy = mr.n2(e[3], e[4]), mr.n2(e[6], e[7])
                if el < c.min_interval or (el < c.timeout and v_xy > c.rest_v) or a_xy > c.rest_a:
                    continue
                if mr.n3(e[0] - g[0], e[1] - g[1], e[2] - g[2]) < c.arrive_radius:
                    trig[a] = abi.NEP_MISSION_REACHED
                elif el > c.timeout:
                    trig[a] = abi.NEP_MISSION_TIMED_OUT
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
                    k, x, y, z, att = self._next(s, a, end, new) if draws else (-1, 0.0, 0.0, 0.0, 0)
                    self._log(i, i, index, oc, att, float(self.t_issue[i]), t_end, float(self.length[i]), self.goal[i].copy())
                    if not draws:
                        self.ev["quota"] += 1
                        continue
                    if k < 0:
                        self._log(i, i, index + 1, abi.NEP_MISSION_NO_GOAL, c.max_attempts, t_end, t_end, 0.0, self.goal[i].copy())
                    else:
                        new[a] = (x, y, z)
                    self._issue3(i, t_end, k, x, y, z)
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
                k, x, y, z, att = self._next(s, a, end, new)
                attempts += att
                if k >= 0:
                    new[a] = (x, y, z)
                self._issue3(i, t_end, k, x, y, z)
            self._log(s, s, int(self.scene[s, 0]), abi.NEP_MISSION_REACHED if ok else abi.NEP_MISSION_TIMED_OUT, attempts, float(self.t_run[s]), t_end,
                      total / float(N), np.zeros(3))
            self.scene[s, 1 if ok else 2] += 1
            self.scene[s, 0] += 1
            if int(self.scene[s, 0]) >= c.max_goals:
                self.scene[s, 3] = 1
                self.ev["quota"] += 1
            self.t_run[s] = t_end


def random_script(rng, n_slots, G, z_lo=0.5, z_hi=2.0):
    """[n_slots][G][3]: x, y in the walks' box and a z of its own per row (cfg.goal_z is not what a scripted goal takes)"""
    g = np.zeros((n_slots, G, 3))
    g[:, :, :2] = rng.uniform(-8.0, 8.0, (n_slots, G, 2)); g[:, :, 2] = rng.uniform(z_lo, z_hi, (n_slots, G))
    return g


# ---- the effort record ----------------------------------------------------------------------------------------------------------
def new_effort(n=1):
    return np.zeros(n, dtype=abi.EFFORT_DTYPE)


def effort_ref(v_max, a_max, j_max, dc, T, ring, head, size, done, slack, rec):
    """one slot, one call, into the 1-element record `rec`; returns the ticks counted"""
    cap = ring.shape[0]
    if done:
        return 0
    n = 0
    for q in range(1, T + 1):
        if not q - 1 <= size - 1:
            break
        s = [float(v) for v in ring[(head + q - 1) % cap]]
        n += 1
        rec["n_ticks"][0] += 1
        rec["jerk_sum"][0] = float(rec["jerk_sum"][0]) + math.sqrt((s[9] * s[9] + s[10] * s[10]) + s[11] * s[11]) * float(dc)
        for name, cnt, off, lim in (("max_v", "n_v_viol", 3, v_max), ("max_a", "n_a_viol", 6, a_max), ("max_j", "n_j_viol", 9, j_max)):
            viol = False
            for i in range(3):
                m = abs(s[off + i])
                if m > float(rec[name][0, i]):
                    rec[name][0, i] = m
                if m > float(lim) + float(slack):
                    viol = True
            rec[cnt][0] += viol
    return n


def random_ring(rng, cap, scale=(1.0, 1.5, 2.0, 4.0)):
    """[cap][12]: positions, velocities, accelerations and jerks of about the limits' size (v 2, a 3, j 5: some beyond them)"""
    r = np.zeros((cap, 12))
    for k, sc in enumerate(scale):
        r[:, 3 * k:3 * k + 3] = rng.normal(0.0, sc, (cap, 3))
    return r
