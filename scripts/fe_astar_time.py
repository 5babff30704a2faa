"""Development aid: device time of frontend_astar_kernel (the reference's best-first search, one wave per search) on S seeded scenes of
N agents + M obstacles at several pop budgets, next to the beam front end (width 32) on the same inputs and to the oracle's
orc_frontend_astar on 16 host threads for a sample of the same slots.  Per launch: hipEvent time of a captured graph replayed (hulls +
search), after a warm-up.  With a PROFILE=1 library (NEP_BACKEND_LIB) and NEP_QP_PROFILE set, the wave's cycles per phase as well.
   python scripts/fe_astar_time.py [scenes=128] [agents=64] [obstacles=20] [pops=100,300,1000] [host_sample=256]"""
import os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch
from neptune_amd import scene, abi
from neptune_amd.backend import BatchBackend


def replay_ms(fn, reps=5):
    """fn() captured once (after two eager warm-up calls), replayed reps times: the median milliseconds of a replay"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin(); fn(); g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    g.replay(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del g
    return float(np.median(ms)), ms


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    M = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    budgets = [int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else "100,300,1000").split(",")]
    n_host = int(sys.argv[5]) if len(sys.argv) > 5 else 256
    made = scene.make_scenes(N, M, range(S), workers=min(S, 16))
    p = made[0]["par"]
    be = BatchBackend(p, made[0]["statics"], n_scenes=S)
    for s in range(S):
        be.set_scene_statics(s, made[s]["statics"])
    com = np.stack([m["committed"] for m in made]); starts = np.stack([scene.frontend_starts(m) for m in made])
    d_c = be.to_device(com); d_s = be.to_device(starts)
    d_g = torch.zeros(S * N * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_r = torch.zeros(S * N * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    cfg = scene.frontend_cfg(p, beam_width=32)
    n = S * N
    ms, all_ms = replay_ms(lambda: be.frontend(cfg, d_c, d_s, d_g, d_r))
    print("%d searches (%d scenes of %d agents + %d obstacles)" % (n, S, N, M))
    print("beam, width 32: %.3f ms per launch (replays: %s)" % (ms, " ".join("%.3f" % x for x in all_ms)), flush=True)
    profile = os.environ.get("NEP_QP_PROFILE") is not None
    sample = np.linspace(0, n - 1, min(n_host, n)).astype(int)
    from oracle import oracle
    oracle.lib()
    hulls = {}
    for pops in budgets:
        be.set_fe_astar(pops)
        free0, _ = torch.cuda.mem_get_info()
        ms, all_ms = replay_ms(lambda: be.frontend_astar(cfg, d_c, d_s, d_g, d_r))
        be.check()
        res = d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy()
        tot = int(res["n_children"].sum()); mx = int(res["n_children"].max())
        print("A*, %d pops: %.3f ms per launch (replays: %s); pops per search mean %.1f max %d, nodes mean %.1f max %d; %.2f us per pop of the longest search (launch / max pops), %.0f searches per second, %.1f M pops per second"
              % (pops, ms, " ".join("%.3f" % x for x in all_ms), tot / n, mx, res["n_feasible"].mean(), int(res["n_feasible"].max()), 1e3 * ms / max(mx, 1), n / (ms * 1e-3), tot / ms * 1e-3), flush=True)
        if profile:
            rows = np.array([be.debug_phase_cycles(2 * int(s_)) for s_ in sample[:64]], dtype=np.float64)
            names = ("pop", "GJK", "fe_child + lookup", "commit + push", "setup", "result")
            tot_c = rows[:, :6].sum(axis=1).mean()
            print("   cycles per search (mean of %d slots): %s; per pop %.0f" % (len(rows), ", ".join("%s %.0f (%.0f %%)" % (nm, rows[:, k].mean(), 100 * rows[:, k].mean() / max(tot_c, 1)) for k, nm in enumerate(names)),
                                                                                 rows[:, :4].sum() / max(rows[:, 8].sum(), 1)), flush=True)
        # the oracle on 16 host threads, a sample of the same slots
        for i in sample:
            s_ = int(i) // N
            if s_ not in hulls:
                hulls[s_] = be.debug_hulls(s_)

        def one(i):
            s_, a = int(i) // N, int(i) % N
            hx, hn = hulls[s_]
            _, r = oracle.frontend_astar(p, cfg, a + 1, starts[s_, a], hx, hn, made[s_]["statics"], max_pops=pops)
            return r["n_children"], r["status"]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            out = np.array(list(ex.map(one, sample)))
        dt = time.perf_counter() - t0
        same = int((out[:, 0] == res["n_children"][sample]).sum())
        print("   oracle, 16 host threads, %d of the slots: %.3f s, %.0f searches per second, %.2f us per pop per thread; pops equal to the device's in %d of %d"
              % (len(sample), dt, len(sample) / dt, 16 * dt * 1e6 / max(int(out[:, 0].sum()), 1), same, len(sample)), flush=True)
    be.close()


if __name__ == "__main__":
    main()
