"""The MTLP side of the reference's main benchmark (neptune_mtlp_benchmark: mtlp_node.cpp, scripts/benchmark_mtlp.py) on the
device: seeded runs of five robots in the yaml's world (24 m x 24 m, z from -0.2 to 5.1, resolution 0.2, drone_radius 0.6), bases
on the reference's circle (nep_mtlp_circle_bases).  A seed is a sequence of runs as the benchmark script makes them: every run
starts where the last one's goals were, and its goals are drawn by updateGoalsRandom's rule — uniform in [-6, 6]^2 (the script's own
x_min + 4 .. x_max - 4 with x_min = -10), at most tether_length 15 from the robot's base, at least close_range / 4 from every robot's
position and close_range 3 from the goals drawn before it — at goal_height 5, rounded to float32 as the message carries them.  The
first run starts on the circle of radius 10 the robots take off from.

All runs of all seeds go to the device in one launch.  Per run the reference logs on /mtlp_log the solve time and the mean path
length; here: the launch's time divided by the runs, and per run the mean length over the robots that were planned, and their share.

Budgets (the reference has neither): max_nodes and max_pops below, printed with the result.

  python scripts/mtlp_benchmark.py [seeds=8] [runs=10] [max_nodes=16384] [max_pops=4000] [device=1]   ->  stdout (kept under profiles/)
"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
from neptune_amd import mtlp  # noqa: E402

N, RES, RADIUS, HEIGHT, TETHER, CLOSE = 5, 0.2, 0.6, 5.0, 15.0, 3.0
BOUNDS = (-12.0, 12.0, -12.0, 12.0, -0.2, 5.1)


def goals_random(rng, bases, pos):
    """benchmark_mtlp.py:225-241"""
    goals = []
    for i in range(N):
        while True:
            g = np.array([rng.uniform(-6.0, 6.0), rng.uniform(-6.0, 6.0), HEIGHT])
            if np.linalg.norm(g[:2] - bases[i][:2]) > TETHER:
                continue
            if any(np.linalg.norm(g - pos[j]) < CLOSE / 4 for j in range(N)) or any(np.linalg.norm(g - q) < CLOSE for q in goals):
                continue
            goals.append(g)
            break
    return np.array(goals)


def main():
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    max_nodes = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
    max_pops = int(sys.argv[4]) if len(sys.argv) > 4 else 4000
    device = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    m = mtlp.Mtlp(mtlp.make_cfg(RES, *BOUNDS, radius=RADIUS, n_robots=N, max_pops=max_pops, max_nodes=max_nodes, path_cap=512))
    bases = mtlp.circle_bases(N)
    all_sg = np.zeros((seeds * runs, N, 2, 3))
    for s in range(seeds):
        rng = np.random.default_rng(s)
        pos = np.array([[-10.0 * math.cos(2 * math.pi / N * i), -10.0 * math.sin(2 * math.pi / N * i), HEIGHT] for i in range(N)])
        for r in range(runs):
            goals = goals_random(rng, bases, pos)
            all_sg[s * runs + r, :, 0] = pos; all_sg[s * runs + r, :, 1] = goals
            pos = goals
    all_sg = all_sg.astype(np.float32).astype(np.float64)
    all_b = np.broadcast_to(bases, (seeds * runs, N, 3)).copy()
    if device:
        import torch
        d_b, d_s = torch.from_numpy(all_b).cuda(), torch.from_numpy(all_sg).cuda()
        out = m.solve_device(d_b, d_s)      # the eager first call: allocates
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); m.solve_device(d_b, d_s, out=out); e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        got = m.from_device(out)
    else:
        t0 = time.perf_counter()
        got = m.solve(all_b, all_sg, device=False)
        ms = (time.perf_counter() - t0) * 1e3
    res, path = got["result"], got["path"]
    print("%d seeds x %d runs of %d robots, %s form; budgets: max_nodes %d, max_pops %d; launch %.1f ms = %.3f ms per run"
          % (seeds, runs, N, "device" if device else "host", max_nodes, max_pops, ms, ms / (seeds * runs)))
    print("%5s %4s %10s %14s %8s %9s %6s" % ("seed", "run", "solve ms", "mean length m", "planned", "pops max", "edges"))
    planned_all, length_all = [], []
    for k in range(seeds * runs):
        ok = res["status"][k] == 1
        lens = [float(np.linalg.norm(np.diff(path[k, i, :res["n_path"][k, i]], axis=0), axis=1).sum()) for i in range(N) if ok[i]]
        planned_all.append(ok.mean()); length_all += lens
        if k % runs < 3 or seeds * runs <= 40:
            print("%5d %4d %10.3f %14.3f %8.2f %9d %6d" % (k // runs, k % runs, ms / (seeds * runs), float(np.mean(lens)) if lens else float("nan"), ok.mean(),
                                                       res["pops"][k].max(), int(got["graph"][k].sum()) - N))
    st = res["status"].ravel()
    print("all: planned %.3f of %d robots (budget %d, empty list %d), mean path length %.3f m, runs outside the domain %d, collinear triangles %d, ball-only tests %d"
          % (float(np.mean(planned_all)), st.size, int((st == 0).sum()), int((st == -1).sum()), float(np.mean(length_all)) if length_all else float("nan"),
             int((got["run_status"] != 1).sum()), int(res["n_degenerate"].sum()), int(res["n_ball_only"].sum())))


if __name__ == "__main__":
    main()
