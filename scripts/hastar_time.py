"""Launch times of the homotopic grid A* (include/neptune_hastar.h) on the device against its host form, for 1
to 4 096 searches per launch at the size of the reference's neptune_single_benchmark.yaml: a 26 m world, resolution 0.4
(a_star_fraction_voxel_size 0.2 x 2), 15 random 0.5 m squares (neptune_ros.cpp:212-250), cable 27 m.  Every search has its own
start and goal (uniform, at least 8 m apart, clear of the inflated squares); 16 seeded scenes are shared round robin.

  python scripts/hastar_time.py [counts=1,4,16,64,256,1024,4096] [reps=5] [max_nodes=8192] [host=1]   ->  stdout (kept under profiles/)
"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
from neptune_amd import hastar  # noqa: E402

SIDE, RES, N_OBST, CABLE, RADIUS, VOXEL, N_SCENES = 26.0, 0.4, 15, 27.0, 0.5, 0.2, 16      # drone_radius 0.5: the squares are inflated by 1 m
X0, Y0, Z0, Z1 = -11.0, -13.0, -1.0, 2.5      # the yaml's x_min, y_min, z_min, z_max
BASE = (-9.0, 0.0)


def squares(rng):
    """neptune_ros.cpp:212-250"""
    pts = []
    while len(pts) < N_OBST:
        x, y = rng.uniform(X0, X0 + SIDE), rng.uniform(Y0, Y0 + SIDE)
        d = [math.hypot(x - q[0], y - q[1]) for q in pts]
        if any(v < 3 * VOXEL or (2 * RADIUS < v < VOXEL * 2.83 + 8 * RADIUS) for v in d) or math.hypot(x - BASE[0], y - BASE[1]) < 6.0:
            continue
        pts.append((float(x), float(y)))
    return pts


def reps_of(centres, rng):
    """a rep per square in the manner of neptune_ros.cpp:929-984: where a line of one common angle through the centre leaves it"""
    th = float(rng.uniform(0.2, 1.3))
    return [[(x - 0.25 * math.cos(th), y - 0.25 * math.sin(th)), (x + 0.25 * math.cos(th), y + 0.25 * math.sin(th))] for x, y in centres]


def make(n_scenes, max_nodes, seed=0):
    rng = np.random.default_rng(seed)
    cfg = hastar.make_cfg(RES, X0, X0 + SIDE, Y0, Y0 + SIDE, Z0, Z1, CABLE, max_pops=1 << 20, max_nodes=max_nodes,
                          hsig_cap=32, cont_cap=160, path_cap=160)
    ha = hastar.HomotopicAstar(cfg, n_scenes, base=BASE)
    worlds = []
    for s in range(n_scenes):
        c = squares(rng)
        un = [[(x + .25, y + .25), (x + .25, y - .25), (x - .25, y - .25), (x - .25, y + .25)] for x, y in c]
        ha.set_statics(s, un, reps_of(c, rng), drone_radius=RADIUS)
        worlds.append(c)
    return ha, worlds, rng


def draw(n, worlds, rng):
    scene = (np.arange(n) % len(worlds)).astype(np.int32)
    start = np.zeros((n, 2)); goal = np.zeros((n, 2))
    for k in range(n):
        c = worlds[scene[k]]
        free = lambda p: all(abs(p[0] - q[0]) > 1.6 or abs(p[1] - q[1]) > 1.6 for q in c)      # noqa: E731
        while True:
            a, b = rng.uniform(0.5, SIDE - 0.5, 2) + (X0, Y0), rng.uniform(0.5, SIDE - 0.5, 2) + (X0, Y0)
            if free(a) and free(b) and math.hypot(*(a - b)) > 8.0:
                break
        start[k], goal[k] = a, b
    return scene, start, goal


def main():
    counts = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,4,16,64,256,1024,4096").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    max_nodes = int(sys.argv[3]) if len(sys.argv) > 3 else 8192      # (0: the reference's pool, 65 x 65 x 8 = 33 800 nodes, 10.4 MB per search)
    host = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    import torch
    ha, worlds, rng = make(N_SCENES, max_nodes)
    print("world %.0f m, resolution %.1f (%d x %d cells), %d squares, cable %.0f m, node pool %d, %.2f MB of working memory per search"
          % (SIDE, RES, int(SIDE / RES), int(SIDE / RES), N_OBST, CABLE, max_nodes, ha.search_bytes() / 1e6))
    print("%8s %12s %12s %10s %10s %10s %10s %8s" % ("searches", "device ms", "host ms", "reached", "pops mean", "pops max", "nodes max", "equal"))
    for n in counts:
        scene, start, goal = draw(n, worlds, rng)
        st = ha.initial_state(n, BASE)
        d_state = ha.to_device_state(st)
        d_in = [torch.from_numpy(a).cuda() for a in (scene, start, goal)]
        out = ha.search_device(*d_in, d_state)      # the eager first call: allocates
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); ha.search_device(*d_in, d_state, out=out); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        res, path, state = ha.from_device(out)
        th, same = float("nan"), "-"
        if host:
            t0 = time.perf_counter()
            want = ha.search(scene, start, goal, state=st, device=False)
            th = (time.perf_counter() - t0) * 1e3
            same = "yes" if all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip((res, path, state), want)) else "NO"
        print("%8d %12.3f %12.3f %10d %10.0f %10d %10d %8s" % (n, float(np.median(ts)), th, int((res["status"] == 1).sum()), res["pops"].mean(), res["pops"].max(), res["nodes_used"].max(), same), flush=True)
    try:
        ha.check()
    except Exception as e:
        print("capacity:", e)


if __name__ == "__main__":
    main()
