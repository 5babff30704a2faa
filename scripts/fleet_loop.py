"""The faithful closed loop on the device (neptune_amd.loop.DeviceFleetLoop, include/neptune_fleet.h): plan deques, point A, splice,
composition and control ticks of every agent of every scene in the batched handle, one captured graph per round:
fleet_select -> front end -> lines + QP -> safety pass -> fleet_commit -> [audit] -> fleet_tick; with --tethers the tethered round
fleet_select -> fleet_predict_ent -> entangle-aware front end -> lines + QP with the entangle rows -> safety pass with the entangle
re-check -> fleet_commit -> [audit] -> fleet_track_ent -> fleet_tick (--no-check: the plain front end and safety pass, tracking on).  Prints the per-scene report (FleetLoop's
stats), the totals, the wall time per round and, with --audit, the worst clearances over all scenes.

  python scripts/fleet_loop.py --agents 64 --obstacles 20 --scenes 128 --rounds 30 [--stagger 5] [--audit [--span-audit]] [--host] [--tethers [--no-check] [--tether-audit]]

--missions {agent,runs} --goals G: fleet_mission joins the round before fleet_tick and flies a campaign of G goals per agent (runs per
scene); the report gains the legs' accounts.

--record R keeps the fleet state before each of the last R rounds in a device ring, written inside the graph.
--rewind SCENE:ROUND flies the recorded flight for ROUND + 1 rounds, takes that scene alone back to the state before ROUND, flies the
one round eagerly with tracing on and prints every agent's outcome, K and statuses next to what the batch's round gave.  With --audit
the summary names the --rewind argument of the round in which the worst box clearance was flown.  --save PATH writes a checkpoint
when the flight stops (at --rounds); --resume PATH continues one, up to --rounds rounds of the whole flight.

--moveback [RADIUS|ref] [--moveback-timeout S]: fleet_moveback joins the round after fleet_select: an agent with a
new goal plans towards its own base first, as the reference's use_moveback_strategy does.

--goal-gate [HALF_SIDE]: goal_gate joins the round right behind the front end: a plan that does not reach its goal
is flown only when another agent's committed trajectory ends on the square goal +- HALF_SIDE (default: the drone radius), as the
reference's move_when_goal_occupied does.  Only with --search astar / astar_ent.

--fly-guess: guess_fallback joins the round right behind the replan and guess_fallback_tally behind fleet_commit:
a replan whose two QP solves failed publishes the front end's guess, which the safety pass judges and fleet_commit flies when it is
accepted, as the reference's replanFull does.  Off by default: such a slot keeps its committed plan.

--cross: every agent's goal is its start mirrored through the middle of the world, so the whole fleet crosses the middle at once —
where failed QPs are common.

--stagger P: every agent replans every P-th round, agent a in the rounds with (round - a) mod P == 0, and a round flies one control
tick (FleetLoop's cadence at P = 5 with the agents' timers spread over the ticks).  --host flies scene 0 with FleetLoop as well and
prints its wall time per round next to the device loop's (one scene each)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=16)
    ap.add_argument("--obstacles", type=int, default=8)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--seed0", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=400, help="at most; the flight stops when every agent of every scene has arrived")
    ap.add_argument("--beam", type=int, default=32)
    ap.add_argument("--stagger", type=int, default=0, metavar="P")
    ap.add_argument("--search", choices=("beam", "astar", "astar_ent"), default="beam", help="front end: the beam (default), the reference's best-first search (nep_batch_frontend_astar; not with --tethers) or that search with the entangle check (astar_ent: nep_batch_frontend_astar_ent; only with --tethers)")
    ap.add_argument("--max-pops", type=int, default=300, help="with --search astar / astar_ent: pops per search")
    ap.add_argument("--team", type=int, choices=(1, 4), default=1, help="with --search astar_ent: waves per search (4: a workgroup of four waves per search, for fleets of few agents; the flight is the same)")
    ap.add_argument("--audit", action="store_true", help="flight audit of every round, inside the graph")
    ap.add_argument("--span-audit", action="store_true", help="with --audit: the span audit (DESIGN section 43) right behind it in the round — the same minima over the whole flown stretch, between the ticks too, and how much the ticks missed")
    ap.add_argument("--tether-audit", action="store_true", help="with --tethers: the tether audit (DESIGN section 41) — taut length, slack, windings, list and bend counts of every tracked control tick, inside the tracking's launch")
    ap.add_argument("--eager", action="store_true", help="no graph capture")
    ap.add_argument("--tethers", action="store_true", help="tethered agents: entangle states tracked per control tick, predicted at A, checked by the front end and the safety pass")
    ap.add_argument("--no-check", action="store_true", help="with --tethers: plain front end and safety pass, the tracking stays on")
    ap.add_argument("--no-proof", action="store_true", help="with --tethers: debug option fleet_ent_proof 0 (every other agent walked at every tick)")
    ap.add_argument("--ent-cap", metavar="K", help="with --tethers: the tracked states in the list form of K entries per slot (DESIGN section 24) instead of the 40-entry record; 'auto' = 2 (agents + obstacles)")
    ap.add_argument("--fe-big-records", type=int, default=0, metavar="R", help="with --tethers: records in the front end's pool of big entangle-state records (nep_batch_set_fe_ent_big_records; 0: the default, 4 per slot)")
    ap.add_argument("--missions", choices=("agent", "runs", "together"), help="a campaign (DESIGN section 23): per-agent successive goals (NeptuneRos::autoCMD), fleet-wide runs (benchmark_mtlp.py) or the position-exchange driver's runs (auto_commands_together.py, DESIGN section 35), drawn on the device inside the graph or taken from --script; the flight stops when every scene's campaign is over")
    ap.add_argument("--script", metavar="exchange[:RADIUS]|PATH.npy", help="with --missions: the goals of every new leg from a table instead of the generator (DESIGN section 35). exchange: auto_commands_together.py's two lists on a circle of RADIUS m (default 10), antipodes in turn, and the first leg onto the circle; PATH.npy: an array [agents][G][3] or [scenes][agents][G][3]")
    ap.add_argument("--effort", nargs="?", const="1e-6", metavar="SLACK", help="the effort record of every flown tick (DESIGN section 35): mean jerk integral, largest velocity / acceleration / jerk component, ticks beyond v_max / a_max / j_max by more than SLACK (default 1e-6)")
    ap.add_argument("--goals", type=int, default=2, metavar="G", help="with --missions: legs per agent / runs per scene")
    ap.add_argument("--moveback", nargs="?", const="ref", metavar="RADIUS|ref", help="the reference's move-back strategy (DESIGN section 32): an agent with a new goal first plans towards its own base, until it is within RADIUS m of it (ref, the default: 6.33 - (agents - 4) * 0.33) or --moveback-timeout has passed")
    ap.add_argument("--moveback-timeout", type=float, default=10.0, metavar="S", help="with --moveback: seconds of simulated time after which the goal is released anyway")
    ap.add_argument("--goal-gate", nargs="?", const="radius", metavar="HALF_SIDE", help="the reference's move_when_goal_occupied gate (DESIGN section 33): a search that did not reach its goal is flown only when somebody else is on the goal's square of this half side (default: the drone radius); not with --search beam")
    ap.add_argument("--fly-guess", action="store_true", help="the reference's rule for a replan whose two QP solves failed (DESIGN section 34): the front end's guess is judged by the safety pass and flown when accepted; off (the default): the slot keeps its committed plan")
    ap.add_argument("--cross", action="store_true", help="every agent's goal is its start mirrored through the middle of the world (scene.crossing_scene's goals): the whole fleet crosses the middle at once; not with --missions")
    ap.add_argument("--record", type=int, default=0, metavar="R", help="flight recorder: the state before each of the last R rounds in a device ring, inside the graph")
    ap.add_argument("--rewind", metavar="SCENE:ROUND", help="fly ROUND + 1 rounds recorded (default --record 8), then that scene alone from the state before ROUND: one eager round, traced")
    ap.add_argument("--save", metavar="PATH", help="write a checkpoint (.npz) when the flight stops")
    ap.add_argument("--resume", metavar="PATH", help="continue the flight of a checkpoint up to --rounds rounds in all")
    ap.add_argument("--host", action="store_true", help="also fly scene 0 with FleetLoop and with DeviceFleetLoop(S = 1): wall time per round of both")
    a = ap.parse_args()
    import numpy as np
    import torch
    from neptune_amd import abi, audit, scene
    from neptune_amd._lib import BackendError
    from neptune_amd.loop import DeviceFleetLoop, FleetLoop
    seeds = [a.seed0 + k for k in range(a.scenes)]
    scenes = scene.make_scenes(a.agents, a.obstacles, seeds, workers=min(len(seeds), len(os.sched_getaffinity(0)), 16))
    if a.span_audit and not a.audit:
        ap.error("--span-audit goes with the flight audit: only with --audit")
    kw = dict(beam_width=a.beam, audit=a.audit, span_audit=a.span_audit, graph=not a.eager, search=a.search, max_pops=a.max_pops, team=a.team)
    if a.tether_audit and not a.tethers:
        ap.error("--tether-audit audits the tethers: only with --tethers")
    if a.tethers:
        kw.update(tethers=True, check=not a.no_check, tether_audit=a.tether_audit)
        if a.ent_cap:
            kw.update(ent_cap="auto" if a.ent_cap == "auto" else int(a.ent_cap))
    if a.missions:
        from neptune_amd import mission
        script = None
        if a.script:
            if a.script.split(":")[0] == "exchange":
                script = mission.exchange_script(a.agents, float(a.script.split(":")[1]) if ":" in a.script else 10.0, scenes[0]["par"].goal_height)
                kw.update(goals=[script[:, -1] for _ in scenes])      # the first leg: onto the circle, where the driver's vehicles start
            else:
                script = np.load(a.script, allow_pickle=False)
        kw.update(missions=mission.MissionSpec(a.missions, goals=a.goals, seed=a.seed0 + 1, script=script))
    elif a.script:
        ap.error("--script gives the goals of a campaign: only with --missions")
    if a.effort:
        kw.update(effort=float(a.effort))
    mb = None
    if a.moveback:
        from neptune_amd import mission
        mb = mission.MoveBack.reference(a.agents, a.moveback_timeout) if a.moveback == "ref" else mission.MoveBack(float(a.moveback), a.moveback_timeout)
        kw.update(moveback=mb)
    gg = False
    if a.goal_gate:
        gg = True if a.goal_gate == "radius" else float(a.goal_gate)
        kw.update(goal_gate=gg)
    if a.fly_guess:
        kw.update(fly_guess=True)
    if a.cross:
        if a.missions:
            ap.error("--cross sets every agent's one goal: not with --missions")
        kw.update(goals=[np.array([[-s[0], -s[1], sc["par"].goal_height] for s in sc["starts"]], dtype=np.float64) for sc in scenes])
    if a.stagger > 0:
        kw.update(replan_every=1, periods=a.stagger, phases=np.tile(np.arange(a.agents) % a.stagger, (a.scenes, 1)))

    if a.record or a.rewind:
        kw.update(recorder=a.record if a.record else 8)

    def make(scs, resume=None):
        lp = DeviceFleetLoop.resume(resume, scs, **kw) if resume else DeviceFleetLoop(scs, **kw)
        if a.tethers and a.no_proof:
            lp.be.debug_option("fleet_ent_proof", 0)
        if a.tethers and a.fe_big_records:
            lp.be.set_fe_ent_big_records(a.fe_big_records)
        return lp

    if a.rewind:
        sc_i, rnd = (int(x) for x in a.rewind.split(":"))
        lp = make(scenes)
        for _ in range(rnd + 1):
            lp.round()
        N = lp.N
        sol = lp.be.solutions()[sc_i * N:(sc_i + 1) * N]
        fres = lp.d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE)[sc_i * N:(sc_i + 1) * N]
        batch = [(int(o), int(q["K"]), int(f["status"]), int(q["stats"]["status"])) for o, q, f in zip(lp.d_outcome.cpu().numpy()[sc_i * N:(sc_i + 1) * N], sol, fres)]
        one = lp.rewind(sc_i, rnd)
        one.round()
        print("scene %d (seed %d), round %d, flown alone from the recorder's ring (agent: outcome, K, front-end status, QP status):" % (sc_i, seeds[sc_i], rnd))
        for i, (got, want) in enumerate(zip(one.trace[0], batch)):
            print("  agent %2d: %-18s K %d  fe %d  qp %d   %s" % (i + 1, abi.FLEET_OUTCOMES[got[0]], got[1], got[2], got[3], "= the batch's round" if got == want else "the batch's round gave %s" % (want,)))
        print("the round %s" % ("reproduces the batch's outcomes" if list(one.trace[0]) == batch else "DIFFERS from the batch's"))
        one.close(); lp.close()
        return

    def fly(scs, rounds, resume=None):
        lp = make(scs, resume)
        for _ in range(2):      # the eager round and the capture
            if lp.rounds < rounds:
                lp.round()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while lp.rounds < rounds:
            n += 1
            if lp.round():
                break
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if a.save and scs is scenes:
            lp.save_checkpoint(a.save)
            print("checkpoint after round %d: %s" % (lp.rounds, a.save))
        try:
            rep = lp.report()
        except BackendError as e:      # (a capacity other than the tracking's: said, not hidden — the read has cleared the sticky flags)
            print("nep_batch_check after the flight:", e)
            rep = lp.report()
        if a.tethers:
            w = lp.be.fleet_ent_state(states=False)["walked"]
            print("tether tracking: %d of %d (other agent, tick) pairs walked, the rest proven free of crossings"
                  % (int(w.sum()), len(scs) * lp.N * (lp.N - 1) * lp.replan_every * lp.rounds))
        flown = lp.rounds
        lp.close()
        return rep, dt / max(n, 1), flown

    rep, per_round, n = fly(scenes, a.rounds, a.resume)
    for s, r in enumerate(rep):
        print("scene %d (seed %d): %s" % (s, seeds[s], json.dumps({k: v for k, v in r.items() if k not in ("audit", "tether_audit", "span_audit")})))
    tot = {k: int(sum(r[k] for r in rep)) for k in ("replans", "accepted", "fe_no_solution", "qp_failed", "qp_relaxed", "rejected_by_safety", "cap", "skipped", "reached")}
    if a.tethers:
        tot.update({k: int(sum(r[k] for r in rep)) for k in ("ever_entangled", "too_long", "track_cap")})
        if a.ent_cap:
            tot.update(held=int(sum(r["held"] for r in rep)), max_list=int(max(r["max_list"] for r in rep)), bend_full=int(sum(r["bend_full"] for r in rep)))
    print("total over %d scenes x %d agents, %d rounds: %s" % (a.scenes, a.agents, n, json.dumps(tot)))
    if a.moveback:
        print("move-back (radius %.2f m, timeout %.1f s): %d slots on their way back at the end" % (mb.radius, mb.timeout, sum(r["way_back"] for r in rep)))
    if a.goal_gate:
        print("goal gate (half side %s): %d slot-rounds examined, %d let through (goal taken), %d turned down (counted in fe_no_solution)"
              % ("drone radius" if gg is True else "%.2f m" % gg, sum(r["gate_examined"] for r in rep), sum(r["goal_taken"] for r in rep), sum(r["gated"] for r in rep)))
    if a.fly_guess:
        print("fly guess: %d slot-rounds with both QP solves failed, %d guesses published, %d flown, %d not flown (turned down by the safety pass, arrived)"
              % tuple(sum(r[k] for r in rep) for k in ("qp_failed_seen", "guess_published", "guess_flown", "guess_not_flown")))
    if a.missions:
        ms = [r["mission"] for r in rep]
        ended = sum(m["legs_reached"] + m["legs_timed_out"] for m in ms)
        print("missions (%s, %d goals): legs issued %d, reached %d, timed out %d, no goal %d; share reached %s; scenes finished %d of %d"
              % (a.missions, a.goals, sum(m["legs_issued"] for m in ms), sum(m["legs_reached"] for m in ms), sum(m["legs_timed_out"] for m in ms),
                 sum(m["no_goal"] for m in ms), "%.3f" % (sum(m["legs_reached"] for m in ms) / ended) if ended else "-", sum(m["finished"] for m in ms), len(ms)))
        if a.missions != "agent":
            lt = [r["longest_leg_time"] for r in rep if r["longest_leg_time"] is not None]
            print("runs: %d ok, %d failed; longest run %s s; mean leg time %s s, mean leg length %s m"
                  % (sum(m["runs_succeeded"] for m in ms), sum(m["runs_failed"] for m in ms), "%.2f" % max(lt) if lt else "-",
                     "%.2f" % np.mean([m["mean_leg_time"] for m in ms if m["mean_leg_time"] is not None]) if ended else "-",
                     "%.2f" % np.mean([m["mean_leg_length"] for m in ms if m["mean_leg_length"] is not None]) if ended else "-"))
    if a.effort:
        p0 = scenes[0]["par"]
        print("effort (slack %g): mean jerk integral per agent %.3f; max |v| %.9f of %.3f, max |a| %.9f of %.3f, max |j| %.9f of %.3f; ticks beyond the limits: v %d, a %d, j %d of %d"
              % (float(a.effort), np.mean([r["jerk_sum_mean"] for r in rep]), max(r["max_v"] for r in rep), p0.v_max, max(r["max_a"] for r in rep), p0.a_max,
                 max(r["max_j"] for r in rep), p0.j_max, sum(r["v_viol"] for r in rep), sum(r["a_viol"] for r in rep), sum(r["j_viol"] for r in rep), sum(r["effort_ticks"] for r in rep)))
    print("wall time per round (rounds 3..%d, %s, %s downloaded every round): %.3f ms = %.1f rounds/s, %.0f scene-rounds/s"
          % (n, "eager" if a.eager else "one graph", "the scenes' finished flags" if a.missions else "arrival flags", per_round * 1e3, 1.0 / per_round, a.scenes / per_round))
    if a.tether_audit:      # (with --ent-cap: the largest list next to the capacity in force)
        cap_now = None if not a.ent_cap else 2 * (a.agents + a.obstacles) if a.ent_cap == "auto" else int(a.ent_cap)
        for line in audit.format_tether_summary([r["tether_audit"] for r in rep], cap=cap_now):
            print(line)
    if a.audit:
        for line in audit.format_summary([r["audit"] for r in rep]):
            print(line)
        if a.span_audit:
            for line in audit.format_span_summary([r["span_audit"] for r in rep]):
                print(line)
        worst = min(r["audit"]["min_box_clear"]["value"] for r in rep if r["audit"]["min_box_clear"])
        print("scenes with min_box_clear < 0: %d of %d; worst %.9f m" % (sum(1 for r in rep if r["audit"]["min_box_clear"] and r["audit"]["min_box_clear"]["value"] < 0), len(rep), worst))
        # the round that flew the worst box clearance: the audit's ticks of round r are t0 + (r T + 1 .. r T + T) dc
        s_w, m_w = min(((s, r["audit"]["min_box_clear"]) for s, r in enumerate(rep) if r["audit"]["min_box_clear"]), key=lambda x: x[1]["value"])
        par = scenes[0]["par"]
        ticks = kw.get("replan_every", 5)
        print("to look at that round (scene %d, agent %d, partner %d, t %.3f s): --rewind %d:%d"
              % (s_w, m_w["agent"], m_w["partner"], m_w["t"], s_w, (int(round(m_w["t"] / par.dc)) - 1) // ticks))
    if a.host:
        sc = scenes[0]
        _, dev1, n1 = fly([sc], a.rounds)
        ref = FleetLoop(sc["par"], sc["statics"], sc["starts"], kw["goals"][0] if a.cross else scene.reachable_goals(sc), beam_width=a.beam, audit=a.audit, tethers=a.tethers, check=not a.no_check, search=a.search, max_pops=a.max_pops, moveback=mb, goal_gate=gg, fly_guess=a.fly_guess, team=a.team)
        ref.round(); ref.round()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = 0
        for _ in range(a.rounds - 2):
            m += 1
            if ref.round():
                break
        torch.cuda.synchronize()
        host = (time.perf_counter() - t0) / max(m, 1)
        ref.close()
        print("one scene (seed %d): DeviceFleetLoop %.3f ms per round over %d rounds, FleetLoop %.3f ms per round over %d rounds"
              % (seeds[0], dev1 * 1e3, n1, host * 1e3, m + 2))


if __name__ == "__main__":
    main()
