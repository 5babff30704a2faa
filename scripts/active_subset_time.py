#!/usr/bin/env python3
"""Step time of the headline scenes (128 x 64 agents, 20 static obstacles, the handle's default solve path, one replan per step
replayed from a captured graph) with an active set (nep_batch_set_active) of 100 / 50 / 25 / 10 / 1 % of the agents and without one,
plus the per-phase device times (hulls, separator, QP) of eager launches.  Two passes over the masks in opposite order (the spread
between them is the noise of the figure).  Prints one JSON document.
  python scripts/active_subset_time.py [--scenes 128 --agents 64 --statics 20 --steps 200]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import torch
from neptune_amd import scene, dist as ndist
from neptune_amd.backend import BatchBackend


def time_graph(be, d_com, d_gue, steps):
    for _ in range(3):
        be.replan(d_com, d_gue)
    st = torch.cuda.Stream(be.device)
    st.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(st):
        be.replan(d_com, d_gue)
    torch.cuda.current_stream(be.device).wait_stream(st)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        be.replan(d_com, d_gue)
    for _ in range(10):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        g.replay()
    e1.record()
    torch.cuda.synchronize(be.device)
    del g
    return e0.elapsed_time(e1) / steps


def phases(be, d_com, d_gue, n=20):
    be.enable_timing(True); be.reset_timing()
    for _ in range(n):
        be.replan(d_com, d_gue)
    torch.cuda.synchronize(be.device)
    t = [be.kernel_time_ms(i)[0] for i in range(4)]
    be.enable_timing(False)
    return dict(hulls=round(t[0], 4), separator=round(t[1], 4), qp=round(t[2], 4), sequence=round(t[3], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=128); ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--statics", type=int, default=20); ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    S, N = a.scenes, a.agents
    scs = scene.make_scenes(N, a.statics, range(S), workers=min(S, 16))
    com, gue = ndist.stack_scenes(scs)
    be = BatchBackend(scs[0]["par"], scs[0]["statics"], n_scenes=S)
    for s in range(1, S):
        be.set_scene_statics(s, scs[s]["statics"])
    d_com, d_gue = be.to_device(com), be.to_device(gue)
    rng = np.random.default_rng(0)
    fracs = [None, 1.0, 0.5, 0.25, 0.1, 0.01]
    masks = {}
    for f in fracs[1:]:
        m = np.zeros((S, N), np.int32)
        k = max(1, int(round(f * N)))
        for s in range(S):
            m[s, rng.choice(N, k, replace=False)] = 1
        masks[f] = torch.from_numpy(m).to(be.device)
    res = {}
    for order in (fracs, fracs[::-1]):
        for f in order:
            be.set_active(masks[f] if f is not None else None)
            ms = time_graph(be, d_com, d_gue, a.steps)
            key = "no_mask" if f is None else "%g%%" % (100 * f)
            r = res.setdefault(key, dict(step_ms=[], active_slots=int(masks[f].sum()) if f is not None else S * N))
            r["step_ms"].append(round(ms, 4))
            if "phases_ms" not in r:
                r["phases_ms"] = phases(be, d_com, d_gue)
    be.set_active(None)
    for r in res.values():
        r["step_ms_mean"] = round(float(np.mean(r["step_ms"])), 4)
        r["replans_per_s"] = round(r["active_slots"] / (r["step_ms_mean"] * 1e-3), 0)
    base = res["no_mask"]["step_ms_mean"]
    for r in res.values():
        r["vs_no_mask"] = round(r["step_ms_mean"] / base, 4)
    print(json.dumps(dict(what="replan step time with an active set (nep_batch_set_active), %d scenes x %d agents, %d statics, graph replay, "
                          "%d steps per figure, two passes" % (S, N, a.statics, a.steps), device=torch.cuda.get_device_name(be.device),
                          results=res), indent=1))
    be.close()


if __name__ == "__main__":
    main()
