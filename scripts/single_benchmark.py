"""The reference's single-agent comparison (NeptuneRos::replanCB with enable_single_benchmark, neptune_ros.cpp:491-613 and
:1650-1676) for S seeded scenes at once: one agent, 15 random 0.5 m squares (neptune_ros.cpp:212-250), G successive random goals.
Per goal two searches start from the same point, both on the device:

  homotopic A*   AstarPathFinder (nep_hastar_search): from the previous goal's cell centre and the tether state the previous
                 search ended with
  kinodynamic    KinodynamicSearch::run with the entangle check (nep_batch_frontend_astar_ent, N = 1), from rest at the same point
                 and the empty entangle state (the reference hands it the flown state, which no flight makes here)

and when both succeed the terminal state and the goal become the initial state and start of the next pair (:1667-1670); otherwise
the scene stays where it is and draws another goal.  Printed: the reference's log fields of both searches — nodes used, path
length — and the success counts.

  python scripts/single_benchmark.py [scenes=64] [goals=8] [obstacles=15] [pops=20000]   ->  stdout
"""
import dataclasses
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch          # noqa: E402
from neptune_amd import abi, hastar, scene  # noqa: E402
from neptune_amd.backend import BatchBackend  # noqa: E402


def reps_of(raw, theta):
    """neptune_ros.cpp:929-984: the two points where the line of angle theta through a square's centre leaves it"""
    out = []
    for q in raw:
        c = q.mean(0)
        r = 0.25 / max(abs(math.cos(theta)), abs(math.sin(theta)))
        out.append([(c[0] - r * math.cos(theta), c[1] - r * math.sin(theta)), (c[0] + r * math.cos(theta), c[1] + r * math.sin(theta))])
    return out


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    n_obst = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    pops = int(sys.argv[4]) if len(sys.argv) > 4 else 20000
    # neptune_single_benchmark.yaml: a 26 m world, cable 27 m, drone_radius 0.5
    p = dataclasses.replace(scene.scaled_params(1, n_obst), x_min=-11.0, x_max=15.0, y_min=-13.0, y_max=13.0, z_min=-1.0, z_max=2.5, drone_radius=0.5,
                            enable_entangle=True, tether_length=27.0)
    rng = np.random.default_rng(0)
    worlds = [scene.random_static_obstacles(p, np.random.default_rng(1000 + s)) for s in range(S)]
    be = BatchBackend(p, worlds[0][1], n_scenes=S)
    cfg = hastar.make_cfg(0.2 * 2.0, p.x_min, p.x_max, p.y_min, p.y_max, p.z_min, p.z_max, p.tether_length, max_nodes=8192, hsig_cap=32, cont_cap=160, path_cap=160)
    ha = hastar.HomotopicAstar(cfg, S, base=tuple(p.pb[0]))
    for s, (raw, infl) in enumerate(worlds):
        be.set_scene_statics(s, infl)
        r, l = scene.static_reps(infl); be.set_static_reps(r, l, scene=s)
        ha.set_statics(s, raw, reps_of(raw, float(rng.uniform(0.2, 1.3))), drone_radius=p.drone_radius)
    be.set_fe_astar(pops)
    fe = scene.frontend_cfg(p, entangle=True)
    _, start0 = scene.bases_on_circle(1, 10.0)
    pos = np.repeat(start0, S, axis=0)                      # [S][2]: where every scene's agent stands
    state = ha.to_device_state(ha.initial_state(S, p.pb[0]))
    d_scene = torch.arange(S, dtype=torch.int32, device="cuda")
    d_com = be.to_device(np.zeros(S, dtype=abi.TRAJ_REC_DTYPE))      # nobody else flies
    d_g = torch.zeros(S * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_r = torch.zeros(S * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    print("%4s | %-52s | %-52s | %s" % ("goal", "homotopic A*: success, nodes mean/max, length mean m", "kinodynamic: plans, goal reached, nodes mean/max, length mean m", "both"))
    tot = np.zeros(3, dtype=int)
    for g in range(G):
        goal = np.zeros((S, 2))
        for s in range(S):
            while True:
                q = rng.uniform(p.x_min + 1.0, p.x_max - 1.0, 2)
                if all(np.abs(q - w.mean(0)).max() > 1.6 for w in worlds[s][0]) and np.hypot(*(q - pos[s])) > 4.0 and np.hypot(*(q - p.pb[0])) < p.tether_length - 2.0:
                    break
            goal[s] = q
        out = ha.search_device(d_scene, pos, goal, state)
        st = np.zeros(S, dtype=abi.FE_START_DTYPE)
        st["pos"][:, :2] = pos; st["pos"][:, 2] = p.goal_height; st["goal"][:, :2] = goal; st["goal"][:, 2] = p.goal_height
        be.frontend_astar_ent(fe, d_com, be.to_device(st), d_g, d_r)
        torch.cuda.synchronize()
        res, path, _ = ha.from_device(out)
        kin = d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy()
        ok_a = res["status"] == 1
        ok_k = kin["K"] > 0
        both = ok_a & ok_k
        tot += [ok_a.sum(), ok_k.sum(), both.sum()]
        fa = "%3d/%d, %6.0f /%5d, %6.2f" % (ok_a.sum(), S, res["nodes_used"].mean(), res["nodes_used"].max(), res["length_m"][ok_a].mean() if ok_a.any() else 0.0)
        fk = "%3d/%d, %3d, %6.0f /%5d, %6.2f" % (ok_k.sum(), S, (kin["status"] == 1).sum(), kin["n_feasible"].mean(), kin["n_feasible"].max(), kin["cost"][ok_k].mean() if ok_k.any() else 0.0)
        print("%4d | %-52s | %-52s | %d" % (g, fa, fk, both.sum()), flush=True)
        # :1667-1670 — the terminal state and the goal are the next initial state and start, where both searches succeeded
        keep = torch.from_numpy(both).cuda()
        for t_old, t_new in zip(state, out["state"]):
            m = keep.view(-1, *([1] * (t_old.dim() - 1)))
            t_old.copy_(torch.where(m, t_new, t_old))
        last = path[np.arange(S), np.maximum(res["n_path"], 1) - 1]
        pos = np.where(both[:, None], last, pos)
    print("searches %d: homotopic A* reached %d, kinodynamic planned %d, both %d" % (S * G, tot[0], tot[1], tot[2]))
    for h, name in ((ha, "homotopic A*"), (be, "kinodynamic")):
        try:
            h.check()
        except Exception as e:
            print("%s: %s" % (name, e))


if __name__ == "__main__":
    main()
