"""Development aid: what one eager front-end call costs the host — no graph, so the entry point's checks, plan_frontend and the
launches are inside the timed region.  129 scenes of 8 agents and 2 statics (1 032 searches: the launch order is made), every entry
point that takes records.  Per entry point, over CALLS calls after a warm-up: the median time of the call itself (enqueue only) and
of the call with the wait for its kernels, in microseconds.   python scripts/fe_host_time.py [calls=300]"""
import dataclasses, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from neptune_amd import scene, abi
from neptune_amd.backend import BatchBackend

N, S = 8, 129


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    base = scene.make_scenes(N, 2, range(4), workers=1)
    for k, sc in enumerate(base):
        scene.synthetic_entangle(sc, seed=1041 + k, frac=0.25)
    scs = [base[s % 4] for s in range(S)]
    p = dataclasses.replace(base[0]["par"], enable_entangle=True)
    be = BatchBackend(p, scs[0]["statics"], n_scenes=S)
    for s in range(S):
        be.set_scene_statics(s, scs[s]["statics"])
        reps, longest = scene.static_reps(scs[s]["statics"]); be.set_static_reps(reps, longest, scene=s)
    be.set_fe_astar(12)
    d_c = be.to_device(np.stack([sc["committed"] for sc in scs])); d_s = be.to_device(np.stack([scene.frontend_starts(sc) for sc in scs]))
    d_g = torch.zeros(S * N * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_r = torch.zeros(S * N * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_case = torch.zeros(S * N * abi.NEP_MAX_POL * N, dtype=torch.int32, device=be.device)
    plain, ent = scene.frontend_cfg(p, beam_width=32), scene.frontend_cfg(p, beam_width=32, entangle=True)
    entries = (("frontend", lambda: be.frontend(plain, d_c, d_s, d_g, d_r)), ("frontend_ent", lambda: be.frontend_ent(ent, d_c, d_s, d_g, d_r, d_case)),
               ("frontend_astar", lambda: be.frontend_astar(plain, d_c, d_s, d_g, d_r)), ("frontend_astar_ent", lambda: be.frontend_astar_ent(ent, d_c, d_s, d_g, d_r, d_case)))
    for name, call in entries:
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        host, wall = [], []
        for _ in range(calls):
            t0 = time.perf_counter(); call(); t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
            host.append(t1 - t0); wall.append(t2 - t0)
        print("%s: call %.2f us, call and wait %.1f us (medians of %d)" % (name, 1e6 * np.median(host), 1e6 * np.median(wall), calls), flush=True)
    be.close()


if __name__ == "__main__":
    main()
