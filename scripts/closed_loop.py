#!/usr/bin/env python3
"""Closed-loop flight of a fleet on the device path (neptune_amd/loop.py): every agent flies from its
start next to its base to a random goal, replanning in bulk-synchronous rounds, the way the reference's
benchmark driver logs a run (scripts/benchmark_mtlp.py:215-223: elapsed time, distance, success).
  python scripts/closed_loop.py [--agents 16 --obstacles 8 --seed 0 --beam 32 --skip-arrived --audit [--span-audit] --tethers [--no-check] [--tether-audit] --search astar --max-pops 300 --team 4]
--tethers: tethered agents, the one-scene host form of DeviceFleetLoop(tethers=True) (entangle states kept on the host with
nep_ent_track_step per control tick, nep_ent_predict_a per round).  --search astar: the reference's best-first search, --max-pops
pops per search, in place of the beam (not with --tethers).  --moveback [RADIUS|ref] [--moveback-timeout S]: every agent first plans
towards its own base (the reference's use_moveback_strategy).  --goal-gate [HALF_SIDE]: a plan that does not reach its
goal is flown only when somebody else is on the goal (the reference's move_when_goal_occupied; not with the beam).
--fly-guess: a replan whose two QP solves failed flies the front end's guess when the safety pass accepts it (the reference's rule,
DESIGN section 34; off by default: such an agent keeps its committed plan)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neptune_amd import scene
from neptune_amd.loop import FleetLoop

ap = argparse.ArgumentParser()
ap.add_argument("--agents", type=int, default=16); ap.add_argument("--obstacles", type=int, default=8)
ap.add_argument("--seed", type=int, default=0); ap.add_argument("--beam", type=int, default=32); ap.add_argument("--max-rounds", type=int, default=400)
ap.add_argument("--skip-arrived", action="store_true", help="arrived agents leave the active set (nep_batch_set_active) instead of being solved and discarded")
ap.add_argument("--audit", action="store_true", help="flight audit on the device (nep_batch_audit) next to the host's distance log")
ap.add_argument("--span-audit", action="store_true", help="with --audit: the span audit (DESIGN section 43; nep_batch_audit_span) — the same minima over the whole flown stretch, between the ticks too, and how much the ticks missed")
ap.add_argument("--tethers", action="store_true", help="tethered agents: entangle-aware front end and safety pass, tether states tracked per control tick")
ap.add_argument("--tether-audit", action="store_true", help="with --tethers: the tether audit (DESIGN section 41; the host form, nep_ent_track_step_audit per control tick)")
ap.add_argument("--no-check", action="store_true", help="with --tethers: plain front end and safety pass, the tracking stays on")
ap.add_argument("--search", choices=("beam", "astar", "astar_ent"), default="beam", help="front end: the beam (default), the reference's best-first search (nep_batch_frontend_astar; not with --tethers) or that search with the entangle check (astar_ent: nep_batch_frontend_astar_ent; only with --tethers)")
ap.add_argument("--max-pops", type=int, default=300, help="with --search astar / astar_ent: pops per search")
ap.add_argument("--team", type=int, choices=(1, 4), default=1, help="with --search astar_ent: waves per search (4: a workgroup of four waves per search; the flight is the same)")
ap.add_argument("--moveback", nargs="?", const="ref", metavar="RADIUS|ref", help="the reference's move-back strategy (DESIGN section 32): an agent with a new goal first plans towards its own base, until it is within RADIUS m of it (ref, the default: 6.33 - (agents - 4) * 0.33) or --moveback-timeout has passed")
ap.add_argument("--moveback-timeout", type=float, default=10.0, metavar="S", help="with --moveback: seconds of simulated time after which the goal is released anyway")
ap.add_argument("--goal-gate", nargs="?", const="radius", metavar="HALF_SIDE", help="the reference's move_when_goal_occupied gate (DESIGN section 33): a search that did not reach its goal is flown only when somebody else is on the goal's square of this half side (default: the drone radius); not with --search beam")
ap.add_argument("--fly-guess", action="store_true", help="the reference's rule for a replan whose two QP solves failed (DESIGN section 34): the front end's guess is judged by the safety pass and flown when accepted; off (the default): the agent keeps its committed plan")
a = ap.parse_args()
if a.tether_audit and not a.tethers:
    ap.error("--tether-audit audits the tethers: only with --tethers")
if a.span_audit and not a.audit:
    ap.error("--span-audit goes with the flight audit: only with --audit")
gg = False if not a.goal_gate else True if a.goal_gate == "radius" else float(a.goal_gate)
mb = None
if a.moveback:
    from neptune_amd import mission
    mb = mission.MoveBack.reference(a.agents, a.moveback_timeout) if a.moveback == "ref" else mission.MoveBack(float(a.moveback), a.moveback_timeout)
sc = scene.make_scene(a.agents, a.obstacles, seed=a.seed)
t0 = time.perf_counter()
loop = FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), beam_width=a.beam, skip_arrived=a.skip_arrived, audit=a.audit, tethers=a.tethers,
                 check=not a.no_check, search=a.search, max_pops=a.max_pops, moveback=mb, goal_gate=gg, fly_guess=a.fly_guess, team=a.team, tether_audit=a.tether_audit, span_audit=a.span_audit)
if a.audit:
    loop.trace = []
st = loop.run(a.max_rounds)
st["wall_s"] = time.perf_counter() - t0
st["success"] = bool(st["reached"] == a.agents)
summary = st.pop("audit", None)
tethers = st.pop("tether_audit", None)
span = st.pop("span_audit", None)
print(json.dumps({k: (float(v) if hasattr(v, "dtype") else v) for k, v in st.items()}))
if tethers is not None:
    from neptune_amd import audit
    for line in audit.format_tether_summary([tethers]):
        print(line)
if summary is not None:
    from neptune_amd import audit
    for line in audit.format_summary([summary]):
        print(line)
    if span is not None:
        for line in audit.format_span_summary([span]):
            print(line)
    # the replans of the round the smallest box clearance fell into, for the agent and its partner: (round start, agent, outcome, K, fe, qp)
    m = summary["min_box_clear"]
    if m is not None:
        rounds = sorted({t for t, *_ in loop.trace})
        t_r = max([t for t in rounds if t < m["t"] - 1e-9], default=rounds[0])
        print("audit min_box_clear fell into the round at t = %.3f s:" % t_r, [e[1:] for e in loop.trace if e[0] == t_r and e[1] + 1 in (m["agent"], m["partner"])])
