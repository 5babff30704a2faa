"""A Neptune-like receding-horizon loop for a whole fleet on the batched device path — what
Neptune::replanFull (reference neptune/src/neptune.cpp:1302-1725) does per agent and per timer tick,
run as bulk-synchronous rounds: point A from the committed plan (include/neptune_plan.h) -> front-end
guess (include/neptune_frontend.h) -> separating lines + spline QP (include/neptune_backend.h) ->
post-solve safety check -> plan splice + trajectory composition -> publish.  The reference's goal
follower is its perfect tracker (scripts/perfect_tracker.py: the state is the commanded goal).

Host side only orchestrates: every numeric step is a C-ABI call (device kernels or the host library)."""
import numpy as np

from . import abi, plan, scene
from . import audit as audit_mod
from ._lib import BackendError
from .backend import BatchBackend


def ent_state_record(st):
    """an entangle.State as one FE_ENT_STATE_DTYPE record (what the front end and the safety pass take as d_ent_init)"""
    al, be_, bi, _ = st.as_lists()
    r = np.zeros(1, dtype=abi.FE_ENT_STATE_DTYPE)
    r["n_alpha"] = len(al); r["n_bend"] = len(bi)
    for k, (i, c) in enumerate(al):
        r["id"][0, k] = i; r["cs"][0, k] = c; r["beta"][0, k] = be_[k]
    for k, b in enumerate(bi):
        r["bend"][0, k] = b
    return r[0]


def ent_published_bends(st, pb, a, reps):
    """publishOwnTraj's bend points of agent a's state: its base, then the anchor of every bend index (an agent's base or a static
    representative's column) -> [1 + n_bend][2]"""
    al, _, bi, _ = st.as_lists()
    N = len(pb)
    return np.array([pb[a]] + [pb[al[b][0] - 1] if al[b][0] <= N else reps[al[b][0] - N - 1][al[b][1]] for b in bi], dtype=np.float64).reshape(-1, 2)


def static_reps(statics):
    """scene.static_reps, or empty arrays for a scene without static obstacles"""
    return scene.static_reps(statics) if len(statics) else (np.zeros((0, 2, 2)), np.zeros((0, 2)))


def upload_statics(be, scenes, tethers):
    """every scene's static obstacles, and with tethers their representatives, into the handle"""
    for s, sc in enumerate(scenes):
        be.set_scene_statics(s, sc["statics"])
        if tethers:
            be.set_static_reps(*static_reps(sc["statics"]), scene=s)


_REC = abi.TRAJ_REC_DTYPE.itemsize
_F = abi.TRAJ_REC_DTYPE.fields
_BEND_COLS = (_F["n_bend"][1], _F["n_bend"][1] + 4), (_F["bend"][1], _F["bend"][1] + _F["bend"][0].itemsize)      # byte ranges of a record


def stamp_bends(d_new, d_rec):
    """stamp the bend points every agent published in its record (d_rec: publishOwnTraj at replan time) into its commit record
    (d_new: the QP's records carry the base only): the safety pass judges the new trajectories with the tethers the others see"""
    vn, vr = d_new.view(-1, _REC), d_rec.view(-1, _REC)
    for lo, hi in _BEND_COLS:
        vn[:, lo:hi].copy_(vr[:, lo:hi])


def check_search(search, max_pops, tethers):
    """the front end's strategy: "beam" (the default), "astar", the reference's best-first search with a budget of max_pops pops
    per search (BatchBackend.set_fe_astar / frontend_astar), which has no entangle check, or "astar_ent", the same search with the
    check (frontend_astar_ent), which flies tethers=True only.  -> does the handle need set_fe_astar"""
    if search not in ("beam", "astar", "astar_ent"):
        raise ValueError("search must be 'beam', 'astar' or 'astar_ent'")
    if search == "astar" and tethers:
        raise ValueError("search='astar' has no entangle check: it cannot fly tethers=True (search='astar_ent' does)")
    if search == "astar_ent" and not tethers:
        raise ValueError("search='astar_ent' is the best-first search with the entangle check: it needs tethers=True (without: search='astar')")
    if search != "beam" and int(max_pops) < 1:
        raise ValueError("max_pops must be at least 1")
    return search != "beam"


def check_team(team, search):
    """waves per search of search="astar_ent" (BatchBackend.set_fe_astar_team): 1 (the default) or 4.  A launch choice like graph=:
    the flight does not depend on it.  ValueError for another value, or for 4 with a search that has no such form"""
    if isinstance(team, bool) or not isinstance(team, (int, np.integer)) or int(team) not in abi.NEP_FE_ASTAR_TEAMS:
        raise ValueError("team must be 1 or 4, not %r" % (team,))
    if int(team) != 1 and search != "astar_ent":
        raise ValueError("team=4 is a form of search='astar_ent' only (search=%r keeps one wave per search)" % (search,))
    return int(team)


def check_goal_gate(goal_gate, search, drone_radius):
    """the reference's move_when_goal_occupied gate (BatchBackend.goal_gate): False / None (off), True (the box
    goal +- drone_radius, the reference's) or a half side in metres -> the half side, or None.  Not with the beam, whose ordinary
    outcome for a far goal is DEPTH_REACHED: the gate would ground the fleet."""
    if goal_gate is None or goal_gate is False:
        return None
    if not isinstance(goal_gate, (bool, int, float, np.integer, np.floating)):
        raise ValueError("goal_gate must be False, True or a half side in metres")
    r = float(drone_radius if goal_gate is True else goal_gate)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError("goal_gate: the half side must be finite and positive, not %r" % (r,))
    if search == "beam":
        raise ValueError("goal_gate needs search='astar' or 'astar_ent': the beam's ordinary outcome for a far goal is DEPTH_REACHED, "
                         "and the gate would ground the fleet")
    return r


def check_fly_guess(fly_guess):
    """the reference's degrade-to-initial-guess rule (BatchBackend.guess_fallback): a boolean, nothing else (a
    count, a string or None is a mistake worth hearing about before a flight) -> bool"""
    if not isinstance(fly_guess, (bool, np.bool_)):
        raise ValueError("fly_guess must be True or False, not %r" % (fly_guess,))
    return bool(fly_guess)


def plan_round(be, fe, d_rec, d_start, d_guess, d_res, d_final, d_acc, tethers=False, d_case=None, d_ent=None, ent_samples=3, astar=False, gate=None,
               fallback=None):
    """the plan half of a round: front end -> lines + QP -> safety pass, from the records d_rec and the starts d_start into d_final
    and d_acc.  With d_case the entangle check is on (d_ent: every tether's state at A): the QP gets the entangle rows and the safety
    pass re-checks.  Tethered rounds stamp the published bend points into the commit records before the safety pass.  astar: the
    best-first search in place of the beam (check_search) — with d_case that is search="astar_ent", frontend_astar_ent.
    gate: (half side, d_count or None) — the move_when_goal_occupied gate right behind the front end (check_goal_gate).
    fallback: a d_count (int32 [n_scenes][4], abi.GUESS_FALLBACK_COUNTS) — the degrade-to-initial-guess rule right behind the replan
    (BatchBackend.guess_fallback, before the bend points are stamped); None: a failed replan publishes nothing."""
    if d_case is not None:
        (be.frontend_astar_ent if astar else be.frontend_ent)(fe, d_rec, d_start, d_guess, d_res, d_case, d_ent_init=d_ent)
        if gate is not None:
            be.goal_gate(d_start, d_guess, d_res, gate[0], d_case=d_case, d_count=gate[1])
        be.replan(None, d_guess, d_ent=d_case)
        if fallback is not None:
            be.guess_fallback(d_guess, fallback)
        stamp_bends(be.d_commit, d_rec)
        be.safety_commit_ent(d_rec, be.d_commit, d_guess, d_final, d_acc, d_ent_init=d_ent, ent_samples=ent_samples)
    else:
        (be.frontend_astar if astar else be.frontend)(fe, d_rec, d_start, d_guess, d_res)      # (astar: the handle's set_fe_astar was called)
        if gate is not None:
            be.goal_gate(d_start, d_guess, d_res, gate[0], d_count=gate[1])
        be.replan(None, d_guess)
        if fallback is not None:
            be.guess_fallback(d_guess, fallback)
        if tethers:
            stamp_bends(be.d_commit, d_rec)
        be.safety_commit(d_rec, be.d_commit, d_guess, d_final, d_acc)


def run_round_ops(lp, eager):
    """lp._round_ops() of one round: eagerly when `eager` (the first round allocates), else as the graph lp._g, captured at the
    first such round and replayed from then on"""
    if eager:
        return lp._round_ops()
    torch, dev = lp.torch, lp.be.device
    if lp._g is None:
        torch.cuda.synchronize()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        lp._g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            lp._g.capture_begin()
            lp._round_ops()
            lp._g.capture_end()
        torch.cuda.current_stream(dev).wait_stream(s)
    lp._g.replay()


class _Audited:
    def audit_records(self):
        """the flight audit so far: AUDIT_DTYPE, [N] (FleetLoop) or [S, N]"""
        return self.d_audit.cpu().numpy().view(abi.AUDIT_DTYPE).reshape(self._audit_shape)

    def span_audit_records(self):
        """the span audit so far: SPAN_AUDIT_DTYPE, [N] (FleetLoop) or [S, N]; span_audit= must be on"""
        return self.d_span.cpu().numpy().view(abi.SPAN_AUDIT_DTYPE).reshape(self._audit_shape)

    def tether_audit_records(self):
        """the tether audit so far: TETHER_AUDIT_DTYPE, [N] (FleetLoop) or [S, N]; tether_audit= must be on"""
        if isinstance(self.d_tether_audit, np.ndarray):      # (FleetLoop: the host form)
            return self.d_tether_audit.copy().reshape(self._audit_shape)
        return self.d_tether_audit.cpu().numpy().view(abi.TETHER_AUDIT_DTYPE).reshape(self._audit_shape)


def check_span_audit(span_audit, audit):
    if span_audit and not audit:
        raise ValueError("span_audit=True audits the stretch between the tick audit's ticks: it needs audit=True")
    return bool(span_audit)


def check_tether_audit(tether_audit, tethers):
    if tether_audit and not tethers:
        raise ValueError("tether_audit=True audits the tethers: it needs tethers=True")
    return bool(tether_audit)


class FleetLoop(_Audited):
    def __init__(self, par, statics, starts, goals, beam_width=32, delta_t_states=6, replan_every=5, device=None, skip_arrived=False, audit=False,
                 tethers=False, check=True, ent_samples=3, search="beam", max_pops=300, moveback=None, goal_gate=False, fly_guess=False, team=1,
                 tether_audit=False, span_audit=False):
        import torch
        from . import mission
        # span_audit (with audit=True, else ValueError): right behind the tick audit the same records go through nep_batch_audit_span
        # over the same window — the minima between the ticks too.  stats then carries its summary
        self.span_audit = check_span_audit(span_audit, audit)
        # tether_audit: every tracked control tick also goes into a nep_tether_audit per agent (nep_ent_track_step_audit in the chain
        # below) — the host form of DeviceFleetLoop(tether_audit=True).  stats then carries its summary
        self.tether_audit = check_tether_audit(tether_audit, tethers)
        self.team = check_team(team, search)      # (waves per search of search="astar_ent": same flight either way)
        self.torch = torch
        self.tethers, self.check, self.ent_samples = tethers, check, ent_samples
        # fly_guess: the reference's rule for a replan whose two QP solves failed (True is the reference) — the
        # front end's guess is judged by the safety pass and flown when accepted (BatchBackend.guess_fallback; Neptune::replanFull
        # does not look at opt_success_, neptune.cpp:1519-1527).  False, the default, is this library's own rule: such an agent keeps
        # its committed plan.  stats then gets abi.GUESS_FALLBACK_COUNTS, and qp_failed counts only the failures with nothing to publish
        self.fly_guess = check_fly_guess(fly_guess)
        # goal_gate: the reference's move_when_goal_occupied — a plan that does not reach the goal is flown only
        # when somebody else is on the goal; a gated replan counts as fe_no_solution (stats: gate_examined, goal_taken, gated)
        self.goal_gate = check_goal_gate(goal_gate, search, par.drone_radius)
        # moveback: the reference's move-back strategy for the loop's one (first) goal — nep_moveback_step after every selection
        self.moveback_cfg = mission.check_moveback(moveback)
        self.sflags = np.zeros(par.num_agents, dtype=np.int32)      # NEP_FLEET_FLAG_WAY_BACK per agent
        self.astar = check_search(search, max_pops, tethers)
        if tethers:
            import dataclasses
            par = dataclasses.replace(par, enable_entangle=True)
        self.p, self.statics = par, statics
        self.N = N = par.num_agents
        self.goals = np.asarray(goals, dtype=np.float64).reshape(N, 3)
        self.be = BatchBackend(par, statics, n_scenes=1, device=device)
        self.be.set_safety_check_prev(True)    # nobody commits a trajectory that crosses what somebody else may keep flying
        self.be.set_line_cull(4.0)             # presolve: far separating lines are verified, not solved for (same optimum)
        if self.astar:
            self.be.set_fe_astar(max_pops)     # (allocates the searches' pools)
            self.be.set_fe_astar_team(self.team)
        self.fe = scene.frontend_cfg(par, beam_width=beam_width, pad_hold=1, entangle=tethers and check, ent_samples=ent_samples)
        if tethers:
            # the one-scene host form of DeviceFleetLoop(tethers=True): entangle_state_ of every agent at its tracked position is kept
            # here (nep_ent_track_step per control tick), the state at A comes from nep_ent_predict_a every round
            from . import entangle
            self._reps, self._longest = static_reps(statics)
            self.be.set_static_reps(self._reps, self._longest)
            self._chk = [entangle.EntangleCheck(N, a + 1, par.num_pol, ent_samples, par.T_span, par.tether_length, par.pb, self._reps, self._longest)
                         for a in range(N)]
            self.ent = [entangle.State(N + len(self._reps), cap=abi.NEP_FE_ENT_CAP) for _ in range(N)]
            self._bends_prev = None            # the lists published a round ago (bendPtsForAgents_prev_)
            self.ent_ever = np.zeros(N, dtype=np.int32)
            self.ent_flags = np.zeros(N, dtype=np.int32)
        self.dc, self.T = par.dc, par.T_span
        self.k_a = delta_t_states - 1          # index of point A in the plan (neptune.cpp:1376-1385 with deltaT_ states ahead)
        self.replan_every = replan_every       # control ticks between rounds (replan timer / dc)
        self.t = 0.0
        lo = (delta_t_states + 0.5) * par.dc   # pins deltaT_ (mu::saturate truncates its bounds to int)
        self.plans = [plan.CommittedPlan(par.dc, par.T_span, lo, lo, 0.0, 1.0, deltaT0=delta_t_states) for _ in range(N)]
        self.state = np.zeros((N, 12))
        for a in range(N):
            self.state[a, :3] = [starts[a][0], starts[a][1], par.goal_height]
            self.plans[a].reset(self.state[a])
        self.prev_pwp = [None] * N             # composed committed trajectory (pwp_prev_)
        self.done = np.zeros(N, dtype=bool)
        # skip_arrived: arrived agents leave the active set of the front end, the replan and the safety pass (nep_batch_set_active) —
        # the reference's replanCB returns early for them (neptune.cpp:1701-1711) and their committed trajectory stays an obstacle.
        # Off: every agent is solved every round and the arrived ones' results are discarded here.
        self.skip_arrived = skip_arrived
        self._d_active = torch.ones((1, N), dtype=torch.int32, device=self.be.device) if skip_arrived else None
        if skip_arrived:
            self.be.set_active(self._d_active)
        self.trace = None                      # set to a list to record (t, agent, outcome, K) of every replan
        self.stats = dict(rounds=0, replans=0, accepted=0, fe_no_solution=0, qp_failed=0, qp_relaxed=0, rejected_by_safety=0,
                          min_pair_dist=np.inf, min_static_dist=np.inf, solves=0)
        self._d_gate_count = None
        if self.goal_gate is not None:
            self._d_gate_count = torch.zeros((1, 4), dtype=torch.int32, device=self.be.device)
            self.stats.update(gate_examined=0, goal_taken=0, gated=0)
        self._d_guess_count = None
        if self.fly_guess:
            self._d_guess_count = torch.zeros((1, 4), dtype=torch.int32, device=self.be.device)
            self.stats.update({k: 0 for k in abi.GUESS_FALLBACK_COUNTS})
        self._static_pts = [np.asarray(s, dtype=np.float64) for s in scene_raw(statics, par)]
        # audit: every round also audits, on the device, the records it uploads anyway over the replan_every ticks about to be flown
        # (nep_batch_audit; those ticks lie before the round's point A, so the uploaded records describe them); _tick keeps its host log
        self.d_audit = self.be.new_audit() if audit else None
        self.d_span = self.be.new_span_audit() if self.span_audit else None
        self._audit_shape = (N,)
        self.d_tether_audit = audit_mod.new_tether_audit(N) if self.tether_audit else None      # (host memory: the chain runs here)

    # ---- records every agent publishes (publishOwnTraj) ----
    def _records(self, t_from):
        rec = np.zeros(self.N, dtype=abi.TRAJ_REC_DTYPE)
        for a in range(self.N):
            r = rec[a]
            r["id"] = a + 1; r["is_agent"] = 1; r["valid"] = 1; r["n_bend"] = 1
            r["bbox"] = 2 * self.p.drone_radius
            r["pos"] = self.state[a, :3]
            r["bend"][0] = self.p.pb[a]
            if self.tethers:                    # the bend points of entangle_state_ (publishOwnTraj, neptune_ros.cpp:457-476)
                b = ent_published_bends(self.ent[a], self.p.pb, a, self._reps)
                r["n_bend"] = len(b); r["bend"][: len(b)] = b
            pw = self.prev_pwp[a]
            if pw is None:                      # not flying yet: a one-interval hover
                r["pwp"]["n_seg"] = 1
                r["pwp"]["times"][:2] = [t_from, t_from + 1000.0]
                r["pwp"]["coeff"][:, 0, 3] = self.state[a, :3]
            else:
                times, coeff = plan.pwp_arrays(pw)
                n = pw.n_seg
                r["pwp"]["n_seg"] = n
                r["pwp"]["times"][: n + 1] = times
                r["pwp"]["coeff"][:, :n, :] = coeff
        return rec

    def _tick(self):
        """one control period: every agent's tracker takes the next goal (Neptune::getNextGoal)"""
        for a in range(self.N):
            g, _last = self.plans[a].next_goal()
            self.state[a] = g
        self.t += self.dc
        xy = self.state[:, :2]
        d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)) + np.eye(self.N) * 1e9
        self.stats["min_pair_dist"] = min(self.stats["min_pair_dist"], float(d.min()))
        for pts in self._static_pts:
            c = pts.mean(axis=0); half = (pts.max(axis=0) - pts.min(axis=0)) / 2
            q = np.maximum(np.abs(xy - c) - half, 0.0)
            self.stats["min_static_dist"] = min(self.stats["min_static_dist"], float(np.sqrt((q ** 2).sum(-1)).min()))

    def round(self):
        """one bulk-synchronous replanning round for every agent that is not at its goal"""
        N, p, torch, be = self.N, self.p, self.torch, self.be
        t_now = self.t
        t_start = t_now + (self.k_a + 1) * self.dc      # plan[k] is k+1 control ticks ahead of the tracked state
        starts = np.zeros(N, dtype=abi.FE_START_DTYPE)
        k_end = np.zeros(N, dtype=np.int64)
        for a in range(N):
            pa = self.plans[a].select_a(self.state[a, :3], t_now)
            A = np.array([pa.A[i] for i in range(12)])
            k_end[a] = pa.k_index_end
            starts[a]["pos"] = A[0:3]; starts[a]["vel"] = A[3:6]; starts[a]["accel"] = A[6:9]
            starts[a]["goal"] = self.goals[a]
            starts[a]["t_start"] = t_start      # one clock per round; an agent whose plan is shorter rests at its end
        if self.moveback_cfg is not None:       # the agents on their way back search towards their base (the goal was issued at t = 0)
            from . import mission
            mission.moveback_step(self.moveback_cfg, self.state, p.pb, None, 0.0, t_now, self.sflags, starts)
        self.last_starts = starts
        rec = self._records(t_now)
        if self.skip_arrived:
            self._d_active.copy_(torch.from_numpy((~self.done).astype(np.int32)).reshape(1, N))
        self.stats["solves"] += int((~self.done).sum()) if self.skip_arrived else N
        d_com = be.to_device(rec); d_start = be.to_device(starts)
        if self.d_audit is not None:
            clock = np.zeros(N, dtype=abi.FE_START_DTYPE)
            clock["t_start"] = t_now + self.dc      # the first tick about to be flown
            d_clock = be.to_device(clock)
            be.audit(d_com, d_clock, self.dc, self.replan_every, self.d_audit)
            if self.d_span is not None:
                be.audit_span(d_com, d_clock, self.dc, self.replan_every, self.d_span)
        d_guess = torch.zeros(N * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
        d_fres = torch.zeros(N * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
        d_final = torch.empty_like(d_com); d_acc = torch.zeros(N, dtype=torch.int32, device=be.device)
        if self.tethers:
            bends = self._predict_a(rec, starts, t_start)
        d_case = d_ent_a = None
        if self.tethers and self.check:
            d_ent_a = be.to_device(self.ent_a)
            d_case = torch.zeros(N * abi.NEP_MAX_POL * N, dtype=torch.int32, device=be.device)
        plan_round(be, self.fe, d_com, d_start, d_guess, d_fres, d_final, d_acc, self.tethers, d_case, d_ent_a, self.ent_samples, self.astar,
                   gate=(self.goal_gate, self._d_gate_count) if self.goal_gate is not None else None, fallback=self._d_guess_count)
        sol = be.solutions(); states = be.states(); fres = d_fres.cpu().numpy().view(abi.FE_RESULT_DTYPE)
        self.last_fres = fres
        if self._d_gate_count is not None:
            gc = self._d_gate_count.cpu().numpy()[0]
            self.stats.update(gate_examined=int(gc[0]), goal_taken=int(gc[1]), gated=int(gc[2]))
        if self._d_guess_count is not None:
            fc = self._d_guess_count.cpu().numpy()[0]
            self.stats.update(qp_failed_seen=int(fc[0]), guess_published=int(fc[1]))
        acc = d_acc.cpu().numpy()
        self.stats["rounds"] += 1
        for a in range(N):
            if self.done[a]:
                if int(sol[a]["stats"]["status"]) == abi.NEP_GUESS:      # (an arrived agent's results are dropped, a published guess included)
                    self.stats["guess_not_flown"] += 1
                if self.skip_arrived and self.trace is not None:
                    self.trace.append((t_now, a, "skipped", int(sol[a]["K"]), int(fres[a]["status"]), int(sol[a]["stats"]["status"])))
                continue
            self.stats["replans"] += 1
            K = int(sol[a]["K"]); status = int(sol[a]["stats"]["status"])
            outcome = ("fe_no_solution" if int(fres[a]["status"]) == 3 or K == 0 else
                       "qp_failed" if status == abi.NEP_FAILED else
                       "rejected_by_safety" if not acc[a] else "accepted")
            if self.trace is not None:
                self.trace.append((t_now, a, outcome, K, int(fres[a]["status"]), status))
            self.stats[outcome] += 1
            if status == abi.NEP_GUESS:         # (fly_guess: a failed QP's guess went through the safety pass like a solution)
                self.stats["guess_flown" if outcome == "accepted" else "guess_not_flown"] += 1
            if outcome != "accepted":
                # the agent keeps its plan.  For fe_no_solution and rejected_by_safety that is the reference's replanFull() == false
                # (neptune_ros.cpp:651-663); for qp_failed it is this library's default and NOT the reference, which flies the
                # guess after a failed optimize (neptune.cpp:1519-1527: the early return is commented out) — fly_guess=True
                continue
            self.stats["qp_relaxed"] += status == abi.NEP_RELAXED
            ns = int(sol[a]["n_states"])
            self.plans[a].splice(int(k_end[a]), states[a, :ns])
            new = plan.make_pwp(np.array(sol[a]["times"])[: K + 1], np.array(sol[a]["coeff"])[:, :K, :])
            if self.prev_pwp[a] is None:
                self.prev_pwp[a] = new
            else:
                # what the others must avoid is the path actually flown: nep_pwp_compose_exact.  (mu::composePieceWisePol,
                # nep_pwp_compose, describes the stretch up to point A with the wrong interval; include/neptune_plan.h)
                self.prev_pwp[a] = plan.compose_exact(t_now, self.prev_pwp[a], new)
        if self.tethers:
            self.ent_flags[:] = 0
        for q in range(self.replan_every):
            before = self.state[:, :2].copy()
            self._tick()
            if self.tethers:                    # odomCB -> updateEntStateStaticObs, once per control tick
                self._track_tick(before, self.state[:, :2].copy(), bends, q == 0, t_now + float(q + 1) * self.dc)
        if self.tethers:
            self._bends_prev = bends
        # arrived (sticky): inside the goal radius and practically at rest; such an agent stops replanning and its
        # committed trajectory keeps it where it is (DroneStatus GOAL_REACHED, neptune.cpp:1701-1711)
        slow = np.sqrt((self.state[:, 3:5] ** 2).sum(axis=1)) < 0.05
        self.done |= (np.hypot(*(self.state[:, :2] - self.goals[:, :2]).T) < p_goal_radius(self.fe)) & slow
        return self.done.all()

    # ---- tethers (host form of nep_batch_fleet_predict_ent / nep_batch_fleet_track_ent) ----
    def _predict_a(self, rec, starts, t_start):
        """Neptune::PredictAlphasBetas per agent -> self.ent_a ([N] FE_ENT_STATE_DTYPE), self.flags_a; returns the round's published bend lists"""
        from . import entangle
        N, p = self.N, self.p
        bends = [np.array(rec[j]["bend"][: int(rec[j]["n_bend"])], dtype=np.float64) for j in range(N)]
        pik = self.state[:, :2].copy()
        pik1 = np.stack([entangle.sample_points(rec[j]["pwp"], t_start, t_start + p.num_pol * p.T_span, p.num_pol, self.ent_samples)[0, 0] for j in range(N)])
        present = np.ones(N, dtype=np.int32)
        self.ent_a = np.zeros(N, dtype=abi.FE_ENT_STATE_DTYPE); self.flags_a = np.zeros(N, dtype=np.int32)
        for a in range(N):
            out, fl = self._chk[a].predict_a(self.ent[a], pik[a], starts[a]["pos"][:2], pik, pik1, present, bends)
            self.ent_a[a] = ent_state_record(out); self.flags_a[a] = fl
        return bends

    def _track_tick(self, before, after, bends, first, t=0.0):
        N = self.N
        old = bends
        if first and self._bends_prev is not None:      # the previous check saw the lists published a round ago
            old = [self._bends_prev[j] if len(self._bends_prev[j]) else bends[j] for j in range(N)]
        present = np.ones(N, dtype=np.int32)
        for a in range(N):
            rec = self.d_tether_audit[a:a + 1] if self.d_tether_audit is not None else None
            fl = self._chk[a].track_step(self.ent[a], before[a], after[a], before, after, present, bends, old, audit=rec, t=t)
            self.ent_flags[a] |= fl; self.ent_ever[a] |= fl

    def run(self, max_rounds=400):
        for _ in range(max_rounds):
            if self.round():
                break
        if self.tethers:
            self.stats["ever_entangled"] = int(((self.ent_ever & abi.NEP_ENT_TRACK_ENTANGLED) != 0).sum())
            self.stats["too_long"] = int(((self.ent_ever & abi.NEP_ENT_TRACK_TOO_LONG) != 0).sum())
            self.stats["track_cap"] = int(((self.ent_ever & abi.NEP_ENT_TRACK_CAP) != 0).sum())
        self.stats["sim_time"] = self.t
        self.stats["reached"] = int(self.done.sum())
        self.stats["dist_to_goal_mean"] = float(np.hypot(*(self.state[:, :2] - self.goals[:, :2]).T).mean())
        if self.d_audit is not None:
            self.stats["audit"] = audit_mod.summarize(self.audit_records())[0]
        if self.d_span is not None:
            self.stats["span_audit"] = audit_mod.summarize_span(self.span_audit_records())[0]
        if self.d_tether_audit is not None:
            self.stats["tether_audit"] = audit_mod.summarize_tethers(self.tether_audit_records(), self.p.tether_length)[0]
        return self.stats

    def close(self):
        self.be.close()
        for pl in self.plans:
            pl.close()


def p_goal_radius(fe):
    return fe.goal_size


def scene_raw(statics, par):
    """un-inflated footprints of the static obstacles (for the simulation's distance log only)"""
    sd = 2 * par.drone_radius + 0.2
    out = []
    for s in statics:
        v = np.asarray(s, dtype=np.float64)
        c = v.mean(axis=0)
        out.append(c + (v - c) * np.maximum(1.0 - sd / np.maximum(np.abs(v - c), 1e-9), 0.0))
    return out


class DeviceFleetLoop(_Audited):
    """FleetLoop's rounds for S scenes at once with nothing on the host (include/neptune_fleet.h): the plan deques, point A, the
    splice, the composition and the control ticks of every (scene, agent) live in the batched handle, and a round

        fleet_select -> [fleet_moveback] -> frontend -> replan [-> guess_fallback] -> safety_commit -> fleet_commit -> [audit] -> fleet_tick

    is one captured graph (graph=True: captured after the first eager round, replayed afterwards).  `scenes` are make_scene
    dicts with the same agent and obstacle counts, each with its own statics; `goals` ([S][N][3], default: every scene's
    scene.reachable_goals).  set_safety_check_prev(True) and set_line_cull(4.0) as in FleetLoop.  periods / phases (ints or
    [S][N] arrays, in rounds): an agent replans in round r when it has not arrived and (r - phase) mod period == 0 — the mask is
    written on the device by fleet_select into the buffer set_active got once; without them every agent is solved every round
    and the results of the arrived ones are dropped (FleetLoop's default).  audit=True audits the records published at the
    round's start over the replan_every ticks about to be flown, from t_now + dc: FleetLoop's placement and clock.  ring_cap: a
    smaller plan ring than a splice can need (tests of the capacity path).  tether_audit=True (with tethers=True, else ValueError):
    fleet_track_ent also folds every control tick it tracks into a nep_tether_audit per slot — taut length, slack, windings, list
    and bend counts (tether_audit_records(), report()'s tether_audit; a checkpoint carries the buffer).
    run() downloads the slots' arrival flags (4 bytes per slot) after every round to know when to stop; nothing else leaves the
    device before report().  trace=True additionally downloads outcome, K and the two statuses per round (FleetLoop.trace).
    search="astar" plans with the reference's best-first search, max_pops pops per search, in place of the beam
    (BatchBackend.frontend_astar; not with tethers=True: ValueError); search="astar_ent" is that search with the entangle check
    (BatchBackend.frontend_astar_ent) in place of frontend_ent in the tethered round below (only with tethers=True).

    tethers=True flies tethered agents: the handle is created with enable_entangle and carries every tether's
    entangle state at the tracked position, and the round becomes

        fleet_select -> [fleet_moveback] -> fleet_predict_ent -> frontend_ent -> replan (entangle rows) -> safety_commit_ent
          -> fleet_commit -> [audit] -> fleet_track_ent -> fleet_tick

    with the state at A (d_ent_a) predicted on the device and the commit records stamped with the published bend points before the
    safety pass (stamp_bends).  check=False keeps the plain front end and safety pass and leaves the tracking on: what the
    same fleet does to its tethers when nobody looks.  report() then also gives ever_entangled, too_long and track_cap per scene.
    ent_cap=K (or "auto": 2 (N + statics)) carries the tether states in the list form of K entries per slot (DESIGN section 24;
    ent_lists0: an abi.EntLists to seed them from) instead of the 40-entry record; the default None is the fixed record's round,
    unchanged.  A slot whose state at A holds more than 40 crossings is held for the round: fleet_predict_ent clears its entry in
    the round's mask — fleet_select's with periods or phases, else an all-ones mask of the loop's own that is refilled inside the
    round before the prediction — and it comes out skipped.  report() then adds `held` (slot-rounds), `max_list` (the longest list now) and `bend_full` (tethers at the bend-point limit) per scene.

    missions=mission.MissionSpec(...) flies a campaign: fleet_mission goes between the commit (audit, tether
    tracking) and fleet_tick, ends legs (mode "agent": NeptuneRos::autoCMD) or runs (mode "runs": benchmark_mtlp.py) and draws
    the next goals on the device, inside the graph.  run() then stops when every scene's campaign is finished (it downloads the
    scenes' flags instead of the slots' arrival flags), and report() adds `mission` per scene: legs or runs reached / timed out /
    without a goal, mean leg time and length, the success rate.  Without missions nothing of this is allocated or launched.
    MissionSpec(mode="together", script=mission.exchange_script(N)) flies the position exchange: the goals of
    every new leg come from the table (uploaded per scene before the capture; rewind twins and resume upload the origin scenes'
    rows), a run ends when every agent has been inside its goal's square once; report() adds `longest_leg_time` from the log.

    effort=True | slack adds fleet_effort behind fleet_mission: per slot the jerk integral, the largest velocity,
    acceleration and jerk component and the ticks that break v_max / a_max / j_max by more than the slack (True: 1e-6) over every
    tick flown before arrival.  The records belong to the loop (d_effort) and travel in a checkpoint; report() adds jerk_sum_mean,
    max_v, max_a, max_j, v_viol, a_viol, j_viol per scene.  With effort=False nothing of it is allocated or launched.

    recorder=R keeps the complete fleet state before each of the last R rounds in a device ring: fleet_snapshot_ring
    is the first call of the round, inside the graph, and entry r mod R holds the state before round r.  rewind(scene, round)
    then gives a one-scene eager loop with tracing on, restored to the state before that round; save_checkpoint(path) and
    resume(path, scenes) carry a flight over the end of the process.  With recorder=None nothing is allocated or launched.

    moveback=mission.MoveBack(radius, timeout) flies the reference's use_moveback_strategy: fleet_moveback goes
    after fleet_select, and a slot with a new goal — the first one, or one a mission issued at the end of the last round — searches
    towards its own base until it is within `radius` of it or `timeout` seconds have passed.  The slot's goal, the arrival test and
    the missions' leg tests stay on the real goal.  report() adds `way_back`, the slots on their way back now, per scene; rewind
    twins, checkpoints and resume carry the option, and a snapshot carries a move-back in progress.  With moveback=None nothing
    is launched.

    goal_gate=True (or a half side in metres) flies the reference's move_when_goal_occupied: BatchBackend.goal_gate
    goes right behind the front end, and a slot whose search did not reach its goal keeps its closest-so-far plan only when another
    agent's committed trajectory ends on the square goal +- drone_radius (the goal the search got: a slot on its way back is tested
    at its base); otherwise the slot is turned down and keeps flying its committed plan.  Not with search="beam" (ValueError).
    report() adds gate_examined, goal_taken and gated per scene, and fe_no_solution now INCLUDES the gated replans (they reach
    fleet_commit as NEP_FE_NO_SOLUTION).  The gate keeps no state: snapshots are what they were; the counts belong to the loop
    (d_gate_count) and travel in a checkpoint; rewind twins and resume carry the option (a file from before it resumes without).

    fly_guess=True flies the reference's rule for a replan whose two QP solves failed — True is the reference,
    False, the default, this library's own rule (such a slot keeps its committed plan).  BatchBackend.guess_fallback goes right
    behind the replan: a NEP_FAILED slot with a usable guess gets the guess's record and status NEP_GUESS, the safety pass judges
    it and fleet_commit splices the guess's states and composes its trajectory when it is accepted; guess_fallback_tally goes behind
    fleet_commit.  report() adds qp_failed_seen, guess_published, guess_flown and guess_not_flown per scene (slot-rounds), and
    qp_failed then counts only the failures that had nothing to publish.  The rule keeps no state: snapshots are what they were; the
    counts belong to the loop (d_guess_count) and travel in a checkpoint; rewind twins and resume carry the option (a file from
    before it resumes without)."""

    # the options a restored flight must share with the flight the snapshot was taken from
    _MUST_MATCH = ("beam_width", "delta_t_states", "replan_every", "audit", "ring_cap", "tethers", "check", "ent_samples", "ent_cap", "moveback", "goal_gate", "fly_guess",
                   "script", "effort", "tether_audit", "span_audit")

    def __init__(self, scenes, beam_width=32, delta_t_states=6, replan_every=5, periods=None, phases=None, audit=False, graph=True,
                 goals=None, device=None, ring_cap=0, trace=False, tethers=False, check=True, ent_samples=3, missions=None, ent_cap=None,
                 ent_lists0=None, recorder=None, search="beam", max_pops=300, moveback=None, goal_gate=False, fly_guess=False, effort=False, team=1,
                 tether_audit=False, span_audit=False):
        import torch
        from . import mission as mission_mod
        self.tether_audit = check_tether_audit(tether_audit, tethers)
        self.span_audit = check_span_audit(span_audit, audit)
        self.team = check_team(team, search)      # (waves per search of search="astar_ent"; not among the options a checkpoint carries: the flight does not depend on it)
        self.torch = torch
        self.scenes = scenes
        self.effort = mission_mod.effort_slack(effort)      # the slack, or None
        self.script = mission_mod.script_rows(missions, len(scenes), scenes[0]["par"].num_agents)      # [S][N][G][3], or None
        self.fly_guess = check_fly_guess(fly_guess)
        self.goal_gate = check_goal_gate(goal_gate, search, scenes[0]["par"].drone_radius)      # the half side, or None
        if isinstance(moveback, dict):      # (a checkpoint's options carry it as plain data)
            moveback = mission_mod.MoveBack(**moveback)
        self.moveback, self.moveback_cfg = moveback, mission_mod.check_moveback(moveback)
        self.astar = check_search(search, max_pops, tethers)
        self._opts = dict(beam_width=beam_width, delta_t_states=delta_t_states, replan_every=replan_every, audit=audit, ring_cap=ring_cap,
                          tethers=tethers, check=check, ent_samples=ent_samples, ent_cap=ent_cap, missions=missions, goals=goals,
                          search=search, max_pops=max_pops, moveback=moveback, goal_gate=self.goal_gate, fly_guess=self.fly_guess,
                          script=mission_mod.spec_plain(missions)[1], effort=self.effort, team=self.team, tether_audit=self.tether_audit,
                          span_audit=self.span_audit)
        S = self.S = len(scenes)
        p = self.p = scenes[0]["par"]
        self.tethers, self.check, self.ent_samples = tethers, check, ent_samples
        if tethers:
            import dataclasses
            p = self.p = dataclasses.replace(p, enable_entangle=True)
        N = self.N = p.num_agents
        self.graph, self.replan_every = graph, replan_every
        be = self.be = BatchBackend(p, scenes[0]["statics"], n_scenes=S, device=device)
        upload_statics(be, scenes, tethers)
        be.set_safety_check_prev(True)
        be.set_line_cull(4.0)
        if self.astar:
            be.set_fe_astar(max_pops)      # (allocates the searches' pools: here, before any capture)
            be.set_fe_astar_team(self.team)
        self.fe = scene.frontend_cfg(p, beam_width=beam_width, pad_hold=1, entangle=tethers and check, ent_samples=ent_samples)
        self.goals = np.stack([np.asarray(scene.reachable_goals(sc) if goals is None else goals[s], dtype=np.float64).reshape(N, 3)
                               for s, sc in enumerate(scenes)])
        state0 = np.zeros((S, N, 12))
        for s, sc in enumerate(scenes):
            state0[s, :, :2] = np.asarray(sc["starts"], dtype=np.float64)[:, :2]
        state0[:, :, 2] = p.goal_height
        lo = (delta_t_states + 0.5) * p.dc      # pins deltaT_ (mu::saturate truncates its bounds to int)
        self.cfg = abi.nep_fleet_cfg(p.dc, p.T_span, lo, lo, 0.0, 1.0, delta_t_states, delta_t_states - 1, replan_every, ring_cap,
                                     self.fe.goal_size, 0.0)
        dev = be.device
        dt = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=t)      # noqa: E731
        self.masked = periods is not None or phases is not None
        d_per = d_pha = None
        if self.masked:
            self.periods = np.broadcast_to(np.asarray(1 if periods is None else periods, dtype=np.int32), (S, N)).copy()
            self.phases = np.broadcast_to(np.asarray(0 if phases is None else phases, dtype=np.int32), (S, N)).copy()
            d_per, d_pha = dt(self.periods.reshape(-1), torch.int32), dt(self.phases.reshape(-1), torch.int32)
        be.fleet_init(self.cfg, dt(state0.reshape(-1), torch.float64), dt(self.goals.reshape(-1), torch.float64), d_per, d_pha)
        n = S * N
        self.d_rec = torch.zeros(n * abi.TRAJ_REC_DTYPE.itemsize, dtype=torch.uint8, device=dev); self.d_final = torch.empty_like(self.d_rec)
        self.d_start = torch.zeros(n * abi.FE_START_DTYPE.itemsize, dtype=torch.uint8, device=dev); self.d_clock = torch.zeros_like(self.d_start)
        self.d_guess = torch.zeros(n * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_res = torch.zeros(n * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_acc = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_outcome = torch.zeros(n, dtype=torch.int32, device=dev)
        self.d_active = None
        if self.masked:
            self.d_active = torch.ones((S, N), dtype=torch.int32, device=dev)
            be.set_active(self.d_active)
        self.d_audit, self._audit_shape = None, (S, N)
        if audit:
            self.d_audit = be.new_audit()
            be.audit(self.d_rec, self.d_clock, p.dc, 0, self.d_audit)      # (the call that allocates: made here, outside any capture)
        # span_audit: the tick audit's records and window through nep_batch_audit_span, right behind it in the round
        self.d_span = None
        if self.span_audit:
            self.d_span = be.new_span_audit()
            be.audit_span(self.d_rec, self.d_clock, p.dc, 0, self.d_span)      # (checks the capacities here, outside any capture)
        self.ent_cap = None
        self.d_hold = None
        if tethers and ent_cap is not None:
            self.ent_cap = 2 * (N + len(scenes[0]["statics"])) if ent_cap == "auto" else int(ent_cap)
            if not self.masked:      # the mask a held slot is cleared in: the loop's own, refilled inside the round
                self.d_hold = torch.ones((S, N), dtype=torch.int32, device=dev)
                be.set_active(self.d_hold)
        if tethers:
            if self.ent_cap is not None:
                be.fleet_init_ent_lists(self.ent_cap, host=ent_lists0)
            else:
                be.fleet_init_ent()
            self.d_ent_a = torch.zeros(n * abi.FE_ENT_STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            self.d_flags_a = torch.zeros(n, dtype=torch.int32, device=dev)
            self.d_flags = torch.zeros(n, dtype=torch.int32, device=dev)
            self.d_case = torch.zeros(n * abi.NEP_MAX_POL * N, dtype=torch.int32, device=dev)
        # tether_audit: fleet_track_ent also accumulates every control tick it tracks into a nep_tether_audit per slot, inside its
        # launch (registered here, outside any capture)
        self.d_tether_audit = None
        if self.tether_audit:
            self.d_tether_audit = be.new_tether_audit()
            be.set_tether_audit(self.d_tether_audit, p.dc)
        self.d_gate_count = torch.zeros((S, 4), dtype=torch.int32, device=dev) if self.goal_gate is not None else None      # abi.GOAL_GATE_COUNTS
        self.d_guess_count = torch.zeros((S, 4), dtype=torch.int32, device=dev) if self.fly_guess else None      # abi.GUESS_FALLBACK_COUNTS
        self.missions = missions
        if missions is not None:
            from . import mission
            self.mission_cfg = mission.mission_cfg(missions, p)
            if mission.uses_keepouts(missions):
                for s, sc in enumerate(scenes):
                    be.fleet_mission_keepout(s, scene.keepout_polygons(sc))
            if self.script is not None:      # (before any capture: the first upload allocates and fixes the capacity)
                be.fleet_mission_script(self.script.reshape(S * N, -1, 3))
            be.fleet_mission_init(self.mission_cfg)
        self.d_effort = be.new_effort() if self.effort is not None else None      # [slots] abi.EFFORT_DTYPE: the loop's, like d_gate_count
        self.recorder, self.d_ring = None, None
        if recorder is not None:      # (allocated here, outside any capture, for the state the handle has now: tethers and missions included)
            self.recorder = int(recorder)
            self.d_ring = be.new_snapshot_ring(self.recorder)
        self.rounds = 0
        self._flown = 0               # rounds this object has flown (rounds: the flight's, which a restore sets)
        self._g = None
        self.trace = [] if trace else None
        self.after_commit = None      # test hook: called between fleet_commit and fleet_tick of an eager round
        self.after_select = None      # test hook (tethered rounds): called after fleet_predict_ent of an eager round
        self.after_mission = None     # test hook (missions): called between fleet_mission and fleet_tick of an eager round
        self.done = np.zeros((S, N), dtype=bool)

    def _round_ops(self):
        be = self.be
        if self.d_ring is not None:      # the state before this round -> entry round mod R
            be.fleet_snapshot_ring(self.d_ring, self.recorder)
        be.fleet_select(self.d_start, self.d_rec, self.d_active, self.d_clock if self.d_audit is not None else None)
        if self.moveback_cfg is not None:      # the slots on their way back search towards their base
            be.fleet_moveback(self.moveback_cfg, self.d_start)
        if self.tethers:
            if self.d_hold is not None:
                self.d_hold.fill_(1)
            be.fleet_predict_ent(self.d_start, self.d_rec, self.d_ent_a, self.d_flags_a)
            if self.after_select is not None:
                self.after_select(self)
        ent = (self.d_case, self.d_ent_a) if self.tethers and self.check else (None, None)
        plan_round(be, self.fe, self.d_rec, self.d_start, self.d_guess, self.d_res, self.d_final, self.d_acc, self.tethers, *ent, self.ent_samples, self.astar,
                   gate=(self.goal_gate, self.d_gate_count) if self.goal_gate is not None else None, fallback=self.d_guess_count)
        be.fleet_commit(self.d_res, self.d_acc, self.d_outcome)
        if self.d_guess_count is not None:
            be.guess_fallback_tally(self.d_outcome, self.d_guess_count)
        if self.after_commit is not None:
            self.after_commit(self)
        if self.d_audit is not None:
            be.audit(self.d_rec, self.d_clock, self.p.dc, self.replan_every, self.d_audit)
            if self.d_span is not None:
                be.audit_span(self.d_rec, self.d_clock, self.p.dc, self.replan_every, self.d_span)
        if self.tethers:
            be.fleet_track_ent(self.d_rec, self.d_flags)
        if self.missions is not None:
            be.fleet_mission()
            if self.after_mission is not None:
                self.after_mission(self)
        if self.d_effort is not None:
            be.fleet_effort(self.p.j_max, self.effort, self.d_effort)
        be.fleet_tick()

    def round(self):
        """one bulk-synchronous round of every scene; True when every agent of every scene has arrived"""
        hooked = self.after_commit is not None or self.after_select is not None or self.after_mission is not None
        run_round_ops(self, not self.graph or self._flown < 1 or hooked)      # (_flown, not rounds: a restored loop's first round allocates too)
        self._flown += 1
        if self.trace is not None:
            oc = self.d_outcome.cpu().numpy()
            sol = self.be.solutions(); fres = self.d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE)
            self.trace.append([(int(oc[i]), int(sol[i]["K"]), int(fres[i]["status"]), int(sol[i]["stats"]["status"])) for i in range(self.S * self.N)])
        self.rounds += 1
        if self.missions is not None:      # a campaign ends with its scenes, not with an arrival (the one download: 16 bytes per scene)
            self.finished = self.be.fleet_mission_finished()
            return bool(self.finished.all())
        self.done = self.be.fleet_done().reshape(self.S, self.N) != 0      # (the one download of a round: 4 bytes per slot)
        return bool(self.done.all())

    def run(self, max_rounds=400):
        for _ in range(max_rounds):
            if self.round():
                break
        return self.report()

    def report(self):
        """per scene FleetLoop.stats' keys (min_pair_dist / min_static_dist come from the audit when it is on), plus `cap` and the
        audit's summary.  With goal_gate: gate_examined, goal_taken (let through) and gated (turned down) — slot-rounds; fe_no_solution
        includes the gated ones.  With fly_guess: abi.GUESS_FALLBACK_COUNTS — slot-rounds whose QP failed, whose guess was published,
        flown (accepted) and not flown; qp_failed is then what had nothing to publish"""
        be = self.be
        try:
            be.check()
        except BackendError:      # (a tether that dropped a move at a capacity is reported as track_cap, not raised)
            if not (self.tethers and (be.fleet_ent_state(states=False)["ever"] & abi.NEP_ENT_TRACK_CAP).any()):
                raise
        cnt, t_now, rnd = be.fleet_counters()
        st = be.fleet_state(pwp=False)
        state = st["state"].reshape(self.S, self.N, 12); done = st["done"].reshape(self.S, self.N)
        flags = st["flags"].reshape(self.S, self.N)
        summ = audit_mod.summarize(self.audit_records(), self.S) if self.d_audit is not None else None
        ssum = audit_mod.summarize_span(self.span_audit_records(), self.S) if self.d_span is not None else None
        ever = be.fleet_ent_state(states=False)["ever"].reshape(self.S, self.N) if self.tethers else None
        lists = held = None
        if self.ent_cap is not None:
            lists, held = be.fleet_ent_lists(self.ent_cap)
            held = held.reshape(self.S, self.N)
        gate = self.d_gate_count.cpu().numpy() if self.d_gate_count is not None else None
        gcount = self.d_guess_count.cpu().numpy() if self.d_guess_count is not None else None
        msum, goals_now, longest = None, self.goals, None
        from . import mission
        if self.missions is not None:
            ms = be.fleet_mission_state()
            msum = mission.summarize(ms, None, self.N, self.mission_cfg.mode)
            goals_now = ms["goal"].reshape(self.S, self.N, 3)      # (dist_to_goal_mean below: to the goals the agents have now)
            recs, _ = be.fleet_mission_log()      # the longest leg (run) the log still holds, per scene: benchmark_multi_direct's longest time
            per = len(recs) // self.S
            longest = [max([float(r["t_end"] - r["t_issue"]) for o in range(s * per, (s + 1) * per) for r in recs[o] if r["outcome"] != abi.NEP_MISSION_NO_GOAL],
                           default=None) for s in range(self.S)]
        esum = mission.summarize_effort(self.effort_records(), self.N) if self.d_effort is not None else None
        tsum = audit_mod.summarize_tethers(self.tether_audit_records(), self.p.tether_length, self.S) if self.d_tether_audit is not None else None
        out = []
        for s in range(self.S):
            c = cnt[s]
            d = dict(rounds=int(rnd[s]), replans=int(c[1] + c[2] + c[3] + c[4] + c[5]), accepted=int(c[4]), fe_no_solution=int(c[1]), qp_failed=int(c[2]),
                     qp_relaxed=int(c[6]), rejected_by_safety=int(c[3]), cap=int(c[5]), skipped=int(c[0]),
                     solves=int(c[1] + c[2] + c[3] + c[4] + c[5] + (0 if self.masked else c[0])), sim_time=float(t_now[s]), reached=int(done[s].sum()),
                     dist_to_goal_mean=float(np.hypot(*(state[s, :, :2] - goals_now[s, :, :2]).T).mean()))
            if self.moveback_cfg is not None:      # the slots on their way back to their base now (the bit is no error and not sticky)
                d["way_back"] = int(((flags[s] & abi.NEP_FLEET_FLAG_WAY_BACK) != 0).sum())
            if gate is not None:       # slot-rounds the gate examined, let through (somebody on the goal) and turned down
                d["gate_examined"], d["goal_taken"], d["gated"] = int(gate[s, 0]), int(gate[s, 1]), int(gate[s, 2])
            if gcount is not None:     # slot-rounds whose QP failed, whose guess was published, flown and not flown
                d.update({k: int(gcount[s, i]) for i, k in enumerate(abi.GUESS_FALLBACK_COUNTS)})
            if lists is not None:      # slot-rounds held at point A and the longest list now
                d["held"] = int(held[s].sum()); d["max_list"] = int(lists.n_alpha.reshape(self.S, self.N)[s].max())
                d["bend_full"] = int((lists.n_bend.reshape(self.S, self.N)[s] >= abi.NEP_MAX_BEND - 1).sum())      # (tethers at the bend-point limit)
            if ever is not None:      # agents whose tether was ever entangled / longer than the cable / dropped a move at a capacity
                d["ever_entangled"] = int(c[7])
                d["too_long"] = int(((ever[s] & abi.NEP_ENT_TRACK_TOO_LONG) != 0).sum())
                d["track_cap"] = int(((ever[s] & abi.NEP_ENT_TRACK_CAP) != 0).sum())
            if msum is not None:
                d["mission"] = msum[s]
                d["longest_leg_time"] = longest[s]
            if esum is not None:
                d.update(esum[s])
            if tsum is not None:
                d["tether_audit"] = tsum[s]
            if summ is not None:
                d["audit"] = summ[s]
                d["min_pair_dist"] = summ[s]["min_center_dist"]["value"] if summ[s]["min_center_dist"] else np.inf
                d["min_static_dist"] = summ[s]["min_static_dist"]["value"] if summ[s]["min_static_dist"] else np.inf
            if ssum is not None:
                d["span_audit"] = ssum[s]
            out.append(d)
        return out

    def effort_records(self):
        """[S*N] abi.EFFORT_DTYPE: every slot's effort record as it stands (blocking); effort= must be on"""
        return self.d_effort.cpu().numpy().view(abi.EFFORT_DTYPE).copy()

    # ---- the recorder ---------------------------------------------------------------------------------------
    def _options(self):
        """the options a snapshot's flight and the flight restored from it must share, as plain data"""
        import dataclasses
        o = {k: self._opts[k] for k in self._MUST_MATCH}
        o["ent_cap"] = self.ent_cap
        from . import mission
        o["missions"] = mission.spec_plain(self.missions)[0]      # (the script travels as o["script"])
        o["moveback"] = dataclasses.asdict(self.moveback) if self.moveback is not None else None
        o["masked"] = bool(self.masked)
        o["search"], o["max_pops"] = self._opts["search"], int(self._opts["max_pops"])
        o["N"], o["n_statics"] = int(self.N), len(self.scenes[0]["statics"])
        return o

    def _twin(self, scenes, rows, **kw):
        """a loop with this one's options over `scenes` (this loop's scenes `rows`)"""
        o = dict(self._opts)
        o["ent_cap"] = self.ent_cap
        if o["goals"] is not None:
            o["goals"] = [o["goals"][s] for s in rows]
        if self.masked:
            o.update(periods=self.periods[rows], phases=self.phases[rows])
        if self.script is not None:      # the origin scenes' rows, as the keep-outs are the origin scenes'
            import dataclasses
            o["missions"] = dataclasses.replace(o["missions"], script=self.script[rows])
        del o["script"]
        o.update(kw)
        return DeviceFleetLoop(scenes, device=self.be.device, **o)

    def rewind(self, scene, round):
        """a new DeviceFleetLoop over scene `scene` alone — eager, trace on, this loop's options, the scene's statics and keep-outs —
        restored to the state before round `round` from the recorder's ring.  ValueError when the ring does not hold that round
        (overwritten, or not flown yet)."""
        if self.d_ring is None:
            raise ValueError("rewind needs DeviceFleetLoop(recorder=R)")
        if not 0 <= scene < self.S:
            raise ValueError("scene out of range")
        self.torch.cuda.synchronize(self.be.device)
        e = round % self.recorder
        st = self.be.snapshot_ring_stamps(self.d_ring, self.recorder)[e, scene]
        if round < 0 or not st["used"] or int(st["round"]) != round:
            held = sorted(int(x["round"]) for x in self.be.snapshot_ring_stamps(self.d_ring, self.recorder)[:, scene] if x["used"])
            raise ValueError("the recorder does not hold the state before round %d of scene %d (it holds rounds %s)" % (round, scene, held))
        lp = self._twin([self.scenes[scene]], [scene], graph=False, trace=True)
        try:
            lp.be.fleet_restore(self.be.snapshot_ring_entry(self.d_ring, self.recorder, e), scene, 0)
        except Exception:
            lp.close()
            raise
        lp.rounds = round
        return lp

    def save_checkpoint(self, path):
        """the flight as it stands into one .npz: the snapshot, the audit buffer when auditing, the loop's round count and the
        options a resumed flight must share"""
        import json
        blob = self.be.fleet_snapshot()
        self.torch.cuda.synchronize(self.be.device)
        data = dict(blob=blob.cpu().numpy(), rounds=np.int64(self.rounds), options=np.array(json.dumps(self._options())))
        if self.d_audit is not None:
            data["audit"] = self.d_audit.cpu().numpy()
        if self.d_span is not None:
            data["span_audit"] = self.d_span.cpu().numpy()
        if self.d_gate_count is not None:
            data["gate_count"] = self.d_gate_count.cpu().numpy()
        if self.d_guess_count is not None:
            data["guess_count"] = self.d_guess_count.cpu().numpy()
        if self.d_effort is not None:
            data["effort"] = self.d_effort.cpu().numpy()
        if self.d_tether_audit is not None:
            data["tether_audit"] = self.d_tether_audit.cpu().numpy()
        with open(path, "wb") as f:
            np.savez(f, **data)

    @classmethod
    def resume(cls, path, scenes, **kw):
        """the flight of save_checkpoint(path) over the same `scenes`, continued: a loop built with the file's options (kw: graph,
        trace, recorder, device; periods / phases / goals as the first flight got them) and restored.  ValueError for a file whose
        options differ from kw's or from the scenes."""
        import json
        from . import mission
        with np.load(path, allow_pickle=False) as z:
            blob, rounds, opts = z["blob"], int(z["rounds"]), json.loads(str(z["options"]))
            aud = z["audit"] if "audit" in z.files else None
            gcnt = z["gate_count"] if "gate_count" in z.files else None
            fcnt = z["guess_count"] if "guess_count" in z.files else None
            eff = z["effort"] if "effort" in z.files else None
            taud = z["tether_audit"] if "tether_audit" in z.files else None
            saud = z["span_audit"] if "span_audit" in z.files else None
        opts.setdefault("script", None)        # (a file from before the options flew without them)
        opts.setdefault("effort", None)
        opts.setdefault("tether_audit", False)
        opts.setdefault("span_audit", False)
        if "effort" in kw:
            kw = dict(kw, effort=mission.effort_slack(kw["effort"]))
        opts.setdefault("moveback", None)      # (a file from before the option flew without it)
        opts.setdefault("goal_gate", None)     # (likewise)
        opts.setdefault("fly_guess", False)    # (likewise)
        if "fly_guess" in kw:
            kw = dict(kw, fly_guess=check_fly_guess(kw["fly_guess"]))
        if "goal_gate" in kw:                  # (False, True or a half side -> what the file holds: the half side, or None)
            kw = dict(kw, goal_gate=check_goal_gate(kw["goal_gate"], opts.get("search", "beam") if kw["goal_gate"] else "astar", scenes[0]["par"].drone_radius))
        if isinstance(kw.get("moveback"), mission.MoveBack):
            kw = dict(kw, moveback=__import__("dataclasses").asdict(kw["moveback"]))
        for k in cls._MUST_MATCH:
            if k in kw and kw[k] != opts[k] and not (k == "ent_cap" and kw[k] == "auto"):
                raise ValueError("checkpoint %s was flown with %s=%r, not %r" % (path, k, opts[k], kw[k]))
        if "missions" in kw and (mission.spec_plain(kw["missions"])[0] != opts["missions"] or mission.spec_plain(kw["missions"])[1] != opts["script"]):
            raise ValueError("checkpoint %s was flown with other missions" % path)
        if scenes[0]["par"].num_agents != opts["N"] or len(scenes[0]["statics"]) != opts["n_statics"]:
            raise ValueError("checkpoint %s was flown with %d agents and %d statics per scene" % (path, opts["N"], opts["n_statics"]))
        if opts["masked"] != ("periods" in kw or "phases" in kw):
            raise ValueError("checkpoint %s was flown %s periods / phases" % (path, "with" if opts["masked"] else "without"))
        for k, dflt in (("search", "beam"), ("max_pops", 300)):      # (a file from before the option has the beam)
            if k in kw and kw[k] != opts.get(k, dflt) and (k == "search" or opts.get("search", "beam") != "beam"):
                raise ValueError("checkpoint %s was flown with %s=%r, not %r" % (path, k, opts.get(k, dflt), kw[k]))
        o = {k: opts[k] for k in cls._MUST_MATCH}
        o["search"], o["max_pops"] = opts.get("search", "beam"), opts.get("max_pops", 300)
        o["missions"] = mission.MissionSpec(**opts["missions"], script=opts["script"]) if opts["missions"] is not None else None
        del o["script"]
        o.update({k: v for k, v in kw.items() if k not in o})
        lp = cls(scenes, **o)
        try:
            lp.be.fleet_restore(blob)      # (refuses another scene count, another configuration, another state)
            if aud is not None:
                lp.d_audit.copy_(lp.torch.from_numpy(aud))
            if gcnt is not None and lp.d_gate_count is not None:
                lp.d_gate_count.copy_(lp.torch.from_numpy(gcnt))
            if fcnt is not None and lp.d_guess_count is not None:
                lp.d_guess_count.copy_(lp.torch.from_numpy(fcnt))
            if eff is not None and lp.d_effort is not None:
                lp.d_effort.copy_(lp.torch.from_numpy(eff))
            if taud is not None and lp.d_tether_audit is not None:
                lp.d_tether_audit.copy_(lp.torch.from_numpy(taud))
            if saud is not None and lp.d_span is not None:
                lp.d_span.copy_(lp.torch.from_numpy(saud))
        except Exception:
            lp.close()
            raise
        lp.rounds = rounds
        return lp

    def close(self):
        self._g = None
        self.d_ring = None
        self.be.close()


class TetherLoop(_Audited):
    """S tethered scenes flown on the device, one captured graph per round (include/neptune_frontend.h):
    frontend_ent -> lines + QP with the entangle rows -> safety_commit_ent -> track_ent -> next_starts, every tether's entangle
    state carried from round to round in `d_ent` ([S*N] FE_ENT_STATE_DTYPE bytes, the front end's and the safety pass's d_ent_init).
    A round flies `n_intervals` planning intervals.  Every record is published with the bend points of its agent's state at the
    round's A (publishOwnTraj at replan time); the tracking then sees the previous round's lists as the previous check's and
    writes the bend points of the next A into the flown records.  `active` ([S, N] int32 device tensor) is the handle's active set
    (nep_batch_set_active).  check=False flies the same rounds with the entangle check of
    the front end and of the safety pass off (plain nep_batch_frontend / nep_batch_safety_commit) and the tracking still on.
    tether_audit=True makes the tracking fold every sampled step it tracks into a nep_tether_audit per slot (DESIGN section 41;
    tether_audit_records(), report()'s tether_audit).
    audit=True adds the flight audit (nep_batch_audit) of the round's final records over the control ticks of the stretch the round
    flies, inside the graph, after the copy into d_rec and before next_starts; report() then carries its summary.
    ent_cap=K (or "auto": 2 (N + statics); ent_lists0: an abi.EntLists to start from) tracks the states in the list form of K entries
    per slot (`lists`, nep_batch_track_ent_lists).  d_ent is then written at the start of every round: a slot's
    list where it fits the fixed record, and a slot whose list holds more than 40 crossings is held for the round through the
    handle's mask (`d_mask` = `active` and the fit; nep_batch_ent_lists_at_a), flying its record on.  report() adds held, max_list."""

    def __init__(self, scenes, beam_width=16, n_intervals=1, ent_samples=3, check=True, device=None, graph=True, active=None, audit=False,
                 ent_cap=None, ent_lists0=None, tether_audit=False, span_audit=False):
        import dataclasses
        import torch
        from neptune_amd import dist as ndist
        self.torch = torch
        self.span_audit = check_span_audit(span_audit, audit)
        self.scenes = scenes
        S = self.S = len(scenes)
        p = self.p = dataclasses.replace(scenes[0]["par"], enable_entangle=True)
        N = self.N = p.num_agents
        self.n_intervals, self.ent_samples, self.check, self.graph = n_intervals, ent_samples, check, graph
        be = self.be = BatchBackend(p, scenes[0]["statics"], n_scenes=S, device=device)
        upload_statics(be, scenes, True)
        if active is not None:      # (torch int32 [S, N]: the front end, the replan and the safety pass skip the inactive agents,
            be.set_active(active)   # who keep flying their records; the tracking moves every tether)
        self.fe = scene.frontend_cfg(p, beam_width=beam_width, entangle=check, ent_samples=ent_samples)
        com, _ = ndist.stack_scenes(scenes)
        starts = np.stack([scene.frontend_starts(sc) for sc in scenes]).reshape(-1)
        self.goals = np.stack([np.asarray(sc["goals"], dtype=np.float64).reshape(N, 3) for sc in scenes])
        dev = be.device
        self.d_rec = be.to_device(com); self.d_rec_prev = self.d_rec.clone(); self.d_final = torch.empty_like(self.d_rec)
        self.d_start = be.to_device(starts)
        self.d_guess = torch.zeros(S * N * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_res = torch.zeros(S * N * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_case = torch.zeros(S * N * abi.NEP_MAX_POL * N, dtype=torch.int32, device=dev)
        self.d_acc = torch.zeros(S * N, dtype=torch.int32, device=dev)
        self.d_ent = torch.zeros(S * N * abi.FE_ENT_STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_flags = torch.zeros(S * N, dtype=torch.int32, device=dev)
        # ent_cap: the states tracked in the list form; d_ent is then each round's state at A where the list fits
        # the fixed record, and a slot where it does not is held through the handle's mask (the caller's `active` and the fit)
        self.ent_cap = None
        if ent_cap is not None:
            self.ent_cap = 2 * (N + len(scenes[0]["statics"])) if ent_cap == "auto" else int(ent_cap)
            self.lists = be.new_ent_lists(self.ent_cap, ent_lists0)
            self.d_active_in = active
            self.d_mask = torch.ones((S, N), dtype=torch.int32, device=dev)
            be.set_active(self.d_mask)
            self.d_flags_a = torch.zeros(S * N, dtype=torch.int32, device=dev)
            self.d_held = torch.zeros(S * N, dtype=torch.int32, device=dev)
        self.rounds = 0
        self.ever_flagged = np.zeros((S, N), dtype=np.int32)
        self._g = None
        self.audit_ticks = int(round(n_intervals * p.T_span / p.dc))
        self.d_audit, self._audit_shape = None, (S, N)
        if audit:
            self.d_audit = be.new_audit()
            be.audit(self.d_rec, self.d_start, p.dc, 0, self.d_audit)      # (the call that allocates: made here, outside any capture)
        # span_audit: the stretch the round flies, [t_start, t_start + n_intervals * T_span], between the ticks too
        self.d_span = None
        if self.span_audit:
            self.d_span = be.new_span_audit()
            be.audit_span(self.d_rec, self.d_start, p.dc, 0, self.d_span)      # (checks the capacities here, outside any capture)
        # tether_audit: track_ent / track_ent_lists also accumulate every sampled step they track into a nep_tether_audit per slot,
        # the steps T_span / ent_samples apart from the round's t_start
        self.d_tether_audit = None
        if tether_audit:
            self.d_tether_audit = be.new_tether_audit()
            be.set_tether_audit(self.d_tether_audit, p.T_span / ent_samples)

    def _round_ops(self):
        be = self.be
        # the safety pass judges the new records with the tethers the others published (d_final inherits them: accepted agents
        # from the commit records, rejected and inactive ones from d_rec)
        if self.ent_cap is not None:
            be.ent_lists_at_a(self.lists, self.d_ent, self.d_mask, self.d_flags_a, self.d_active_in, self.d_held)
        plan_round(be, self.fe, self.d_rec, self.d_start, self.d_guess, self.d_res, self.d_final, self.d_acc, True,
                   self.d_case if self.check else None, self.d_ent, self.ent_samples)
        if self.ent_cap is not None:
            be.track_ent_lists(self.d_rec_prev, self.d_final, self.d_guess, self.lists, self.d_flags, n_intervals=self.n_intervals,
                               ent_samples=self.ent_samples)
        else:
            be.track_ent(self.d_rec_prev, self.d_final, self.d_guess, self.d_ent, self.d_flags, n_intervals=self.n_intervals,
                         ent_samples=self.ent_samples)
        self.d_rec_prev.copy_(self.d_rec)
        self.d_rec.copy_(self.d_final)
        if self.d_audit is not None:
            be.audit(self.d_rec, self.d_start, self.p.dc, self.audit_ticks, self.d_audit)
            if self.d_span is not None:
                be.audit_span(self.d_rec, self.d_start, self.p.dc, self.audit_ticks, self.d_span)
        be.next_starts(self.d_rec, self.n_intervals * self.p.T_span, self.d_start)

    def round(self):
        run_round_ops(self, not self.graph or self.rounds < 1)
        self.rounds += 1
        self.ever_flagged |= (self.d_flags.cpu().numpy().reshape(self.S, self.N) & abi.NEP_ENT_TRACK_ENTANGLED) != 0

    def run(self, rounds):
        for _ in range(rounds):
            self.round()
        self.torch.cuda.synchronize(self.be.device)
        return self.report()

    def states(self):
        return self.d_ent.cpu().numpy().view(abi.FE_ENT_STATE_DTYPE).reshape(self.S, self.N)

    def report(self):
        st = self.d_start.cpu().numpy().view(abi.FE_START_DTYPE).reshape(self.S, self.N)
        d = np.hypot(st["pos"][..., 0] - self.goals[..., 0], st["pos"][..., 1] - self.goals[..., 1])
        nb = self.states()["n_bend"] if self.ent_cap is None else self.lists.n_bend.cpu().numpy().reshape(self.S, self.N)
        rep = dict(rounds=self.rounds, arrived=[int(x) for x in (d < 2 * self.fe.goal_size).sum(axis=1)],
                   ever_entangled=[int(x) for x in self.ever_flagged.sum(axis=1)],
                   bend_hist=[int(x) for x in np.bincount(nb.reshape(-1), minlength=abi.NEP_MAX_BEND)[:abi.NEP_MAX_BEND]])
        if self.ent_cap is not None:      # slot-rounds held at A and the longest list now, per scene
            rep["held"] = [int(x) for x in self.d_held.cpu().numpy().reshape(self.S, self.N).sum(axis=1)]
            rep["max_list"] = [int(x) for x in self.lists.n_alpha.cpu().numpy().reshape(self.S, self.N).max(axis=1)]
        if self.d_audit is not None:
            rep["audit"] = audit_mod.summarize(self.audit_records(), self.S)
        if self.d_span is not None:
            rep["span_audit"] = audit_mod.summarize_span(self.span_audit_records(), self.S)
        if self.d_tether_audit is not None:
            rep["tether_audit"] = audit_mod.summarize_tethers(self.tether_audit_records(), self.p.tether_length, self.S)
        return rep

    def close(self):
        self._g = None
        self.be.close()
