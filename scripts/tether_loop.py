"""Tethered fleets on the device (neptune_amd.loop.TetherLoop): front end with the entangle check -> lines + QP with the entangle rows ->
safety pass with the entangle re-check -> tether tracking -> next point A, one captured graph per round, every tether's entangle state
carried from round to round.  Prints, per scene, the agents that arrived, the agents ever flagged entangled (active_cases > 2) and the
bend-point histogram of the final states, and the mean time of a replayed round.

  python scripts/tether_loop.py --agents 16 --obstacles 8 --scenes 4 --rounds 40 --crossing"""
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
    a = ap.parse_args()
    import torch
    from neptune_amd import scene
    from neptune_amd.loop import TetherLoop
    seeds = [a.seed + k for k in range(a.scenes)]
    scenes = [scene.tether_crossing_scene(a.agents, a.obstacles, s) for s in seeds] if a.crossing else \
        scene.make_scenes(a.agents, a.obstacles, seeds, workers=min(len(seeds), len(os.sched_getaffinity(0))))
    lp = TetherLoop(scenes, beam_width=a.beam, n_intervals=a.intervals, check=not a.no_check)
    lp.run(2)                                   # eager round (allocations) + capture
    t0 = time.perf_counter()
    rep = lp.run(a.rounds - 2)
    dt = (time.perf_counter() - t0) / max(a.rounds - 2, 1)
    rep.update(agents=a.agents, obstacles=a.obstacles, scenes=a.scenes, crossing=a.crossing, check=not a.no_check,
               intervals=a.intervals, round_ms=dt * 1e3, note="round_ms includes one flag read-back per round")
    print(json.dumps(rep))
    lp.close()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
