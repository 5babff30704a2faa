"""Launch times of the MTLP comparator (include/neptune_mtlp.h) on the device against its host form on one
core, for 4 to 4 096 searches per launch (runs of 4 robots) in the world of the reference's neptune_mtlp_benchmark.yaml: 24 m x
24 m x 5.3 m, resolution 0.2 (120 x 120 x 26 cells), drone_radius 0.6, bases on the reference's circle, starts and goals uniform in
the inner 12 m at the benchmark's height of 5 m, rounded to float32 as its message carries them.

Budgets (the reference has neither; GLX * GLY * GLZ would be 374 400 nodes): max_nodes and max_pops below, printed with the result.

  python scripts/mtlp_time.py [runs=1,4,16,64,256,1024] [reps=3] [max_nodes=8192] [max_pops=2000] [host=1]   ->  stdout (kept under profiles/)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
from neptune_amd import mtlp  # noqa: E402

N, RES, RADIUS, HEIGHT = 4, 0.2, 0.6, 5.0
BOUNDS = (-12.0, 12.0, -12.0, 12.0, -0.2, 5.1)


def draw(r, rng):
    bases = np.broadcast_to(mtlp.circle_bases(N), (r, N, 3)).copy()
    sg = np.zeros((r, N, 2, 3))
    sg[..., :2] = rng.uniform(-6.0, 6.0, (r, N, 2, 2)).astype(np.float32)
    sg[..., 2] = HEIGHT
    return bases, sg


def main():
    runs = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,4,16,64,256,1024").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    max_nodes = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
    max_pops = int(sys.argv[4]) if len(sys.argv) > 4 else 2000
    host = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    import torch
    m = mtlp.Mtlp(mtlp.make_cfg(RES, *BOUNDS, radius=RADIUS, n_robots=N, max_pops=max_pops, max_nodes=max_nodes, path_cap=256))
    rng = np.random.default_rng(0)
    print("world 24 x 24 x 5.3 m, resolution %.1f, radius %.1f, %d robots per run; budgets: max_nodes %d, max_pops %d; %.2f MB of working memory per search"
          % (RES, RADIUS, N, max_nodes, max_pops, m.search_bytes() / 1e6))
    print("%8s %8s %12s %12s %9s %8s %8s %10s %10s %8s" % ("searches", "runs", "device ms", "host ms", "reached", "budget", "empty", "pops mean", "pops max", "equal"))
    for r in runs:
        bases, sg = draw(r, rng)
        d_b, d_s = torch.from_numpy(bases).cuda(), torch.from_numpy(sg).cuda()
        out = m.solve_device(d_b, d_s)      # the eager first call: allocates
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); m.solve_device(d_b, d_s, out=out); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        got = m.from_device(out)
        th, same = float("nan"), "-"
        if host:
            t0 = time.perf_counter()
            want = m.solve(bases, sg, device=False)
            th = (time.perf_counter() - t0) * 1e3
            same = "yes" if all(got[k].tobytes() == want[k].tobytes() for k in ("graph", "run_status", "result", "path")) else "NO"
        st = got["result"]["status"]
        print("%8d %8d %12.3f %12.3f %9d %8d %8d %10.0f %10d %8s" % (r * N, r, float(np.median(ts)), th, int((st == 1).sum()), int((st == 0).sum()), int((st == -1).sum()),
                                                                  got["result"]["pops"].mean(), got["result"]["pops"].max(), same), flush=True)
    try:
        m.check()
    except Exception as e:
        print("flags:", e)


if __name__ == "__main__":
    main()
