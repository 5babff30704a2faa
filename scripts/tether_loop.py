"""Tethered fleets on the device (neptune_amd.loop.TetherLoop): front end with the entangle check -> lines + QP with the entangle rows ->
safety pass with the entangle re-check -> tether tracking -> next point A, one captured graph per round, every tether's entangle state
carried from round to round.  Prints, per scene, the agents that arrived, the agents ever flagged entangled (active_cases > 2) and the
bend-point histogram of the final states, and the mean time of a replayed round.

With --audit every round also runs the flight audit (nep_batch_audit) inside the graph; the summary names the worst scene of each
minimum and, for the smallest box clearance and static distance, the round it fell into and what the replans of the agent and of its
partner came to in that round (front-end status, QP status, accepted by the safety pass).

  python scripts/tether_loop.py --agents 16 --obstacles 8 --scenes 4 --rounds 40 --crossing [--audit [--span-audit]] [--tether-audit]"""
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
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--seed", type=int, default=61)
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--intervals", type=int, default=1, help="planning intervals flown per round")
    ap.add_argument("--crossing", action="store_true", help="scene.tether_crossing_scene: agents hover beyond each other's paths")
    ap.add_argument("--no-check", action="store_true", help="the front end and the safety pass without the entangle check")
    ap.add_argument("--ent-cap", metavar="K", help="the tracked states in the list form of K entries per slot (DESIGN section 24); 'auto' = 2 (agents + obstacles)")
    ap.add_argument("--tether-audit", action="store_true", help="the tether audit (DESIGN section 41): taut length, slack, windings, list and bend counts of every tracked step, inside the tracking's launch")
    ap.add_argument("--audit", action="store_true", help="flight audit of every round, inside the graph (reads each round's replan outcomes back)")
    ap.add_argument("--span-audit", action="store_true", help="with --audit: the span audit (DESIGN section 43) right behind it in the graph — the same minima over the whole flown stretch, between the ticks too, and how much the ticks missed")
    a = ap.parse_args()
    if a.span_audit and not a.audit:
        ap.error("--span-audit goes with the flight audit: only with --audit")
    import numpy as np
    import torch
    from neptune_amd import abi, audit, scene
    from neptune_amd.loop import TetherLoop
    seeds = [a.seed + k for k in range(a.scenes)]
    scenes = [scene.tether_crossing_scene(a.agents, a.obstacles, s) for s in seeds] if a.crossing else \
        scene.make_scenes(a.agents, a.obstacles, seeds, workers=min(len(seeds), len(os.sched_getaffinity(0))))
    lp = TetherLoop(scenes, beam_width=a.beam, n_intervals=a.intervals, check=not a.no_check, audit=a.audit, tether_audit=a.tether_audit, span_audit=a.span_audit,
                    ent_cap=None if not a.ent_cap else "auto" if a.ent_cap == "auto" else int(a.ent_cap))
    t_first = float(lp.d_start.cpu().numpy().view(abi.FE_START_DTYPE)["t_start"][0])
    outcomes = []                               # --audit: per round [S, N, 3] front-end status, QP status, accepted
    # The scenes' initial records are part of the input, and an agent whose first replans fail keeps flying them: the audit of the
    # rounds that can still fly one (the first num_pol intervals) is reported apart from the audit of the rounds after them.
    split = -(-lp.p.num_pol // a.intervals)
    early, early_span = [], []

    def run(n):
        if not a.audit:
            return lp.run(n)
        for _ in range(n):
            lp.round()
            S, N = lp.S, lp.N
            outcomes.append(np.stack([lp.d_res.cpu().numpy().view(abi.FE_RESULT_DTYPE)["status"].reshape(S, N),
                                      lp.be.solutions()["stats"]["status"].reshape(S, N), lp.d_acc.cpu().numpy().reshape(S, N)], axis=-1))
            if lp.rounds == split and a.rounds > split:
                early.append(audit.summarize(lp.audit_records(), S))
                lp.d_audit.copy_(lp.be.new_audit())      # (in place: the captured graph keeps its buffer)
                if a.span_audit:
                    early_span.append(audit.summarize_span(lp.span_audit_records(), S))
                    lp.d_span.copy_(lp.be.new_span_audit())
        torch.cuda.synchronize()
        return lp.report()
    run(2)                                      # eager round (allocations) + capture
    t0 = time.perf_counter()
    rep = run(a.rounds - 2)
    dt = (time.perf_counter() - t0) / max(a.rounds - 2, 1)
    summary = rep.pop("audit", None)
    tethers = rep.pop("tether_audit", None)
    spans = rep.pop("span_audit", None)
    rep.update(agents=a.agents, obstacles=a.obstacles, scenes=a.scenes, crossing=a.crossing, check=not a.no_check,
               intervals=a.intervals, round_ms=dt * 1e3, note="round_ms includes one flag read-back per round")
    print(json.dumps(rep))
    if tethers is not None:      # (with --ent-cap: the largest list next to the capacity in force)
        for line in audit.format_tether_summary(tethers, cap=lp.ent_cap):
            print(line)
    span = a.intervals * lp.p.T_span
    for name, summary, between in ([("rounds 0..%d (an initial record of the scene can still be flown)" % (split - 1), early[0], early_span[0] if early_span else None),
                                    ("rounds %d..%d" % (split, a.rounds - 1), summary, spans)] if early else [("all rounds", summary, spans)] if summary is not None else []):
        print("audit of", name)
        for line in audit.format_summary(summary):
            print(line)
        if between is not None:
            for line in audit.format_span_summary(between):
                print(line)
        for key, is_pair in (("min_box_clear", True), ("min_static_dist", False)):
            cand = [(sc[key]["value"], s) for s, sc in enumerate(summary) if sc[key] is not None]
            if not cand:
                continue
            _, s = min(cand)
            m = summary[s][key]
            r = min(max(int((m["t"] - t_first) / span + 1e-9), 0), len(outcomes) - 1)
            who = [("agent", m["agent"])] + ([("partner", m["partner"])] if is_pair else [])
            print("audit %-16s fell into round %d of scene %d: " % (key, r, s)
                  + "; ".join("%s %d fe %d qp %d accepted %d" % ((w, i) + tuple(int(x) for x in outcomes[r][s, i - 1])) for w, i in who))
        viol = [s for s, sc in enumerate(summary) if sc["n_pair_viol"] or sc["n_static_viol"]]
        print("audit scenes with a violation:", viol if viol else "none")
    if outcomes:
        failed = np.stack(outcomes)[..., 2] == 0
        print("replans not accepted: %.2f %% of all, %.2f %% in rounds %d.." % (100 * failed.mean(), 100 * failed[min(split, len(outcomes) - 1):].mean(), split))
    lp.close()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
