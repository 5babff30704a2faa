"""Why does the config-5 chain leg end 16 % of its front-end searches with "no solution" (round-3 review, item 3b)?  The same chain step
as bench.py's config5.chain leg is run for a few rounds on the GPU; then, on the hulls of the LAST round and from the same points A, the
oracle's restatement of the reference's best-first search (orc_frontend_astar: KinodynamicSearch::run without the entangle pruning,
20 000 pops) and the oracle's beam without the entangle check are run on the host for every search of the first scenes, and the
outcomes are tabulated next to the device's (beam WITH the entangle check).  A search the reference's own A* cannot start either
(no collision-free first primitive from point A) is a property of the scenario, not of the beam.

Next to them the device's own best-first search (nep_batch_frontend_astar, entangle check off) runs EVERY search of every scene in one
launch per budget — what the host loop cannot do at scale — and is tabulated against the device beam without the check: outcomes, K
and the progress towards the goal ((|A - goal| - dist_to_goal) / |A - goal| of the returned node).

Last, the attribution the entangle-aware comparator allows: the device's best-first search WITH the check
(nep_batch_frontend_astar_ent) at every budget against the device beam with the check on the same inputs, and whether the searches
without a first primitive are the same set for every strategy.

  python scripts/fe_success_rates.py [scenes=4] [rounds=6] [host_scenes=2] [agents=256] [obstacles=100] [pops=100,300,1000]   ->  stdout (kept under profiles/)
"""
import dataclasses
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np, torch          # noqa: E402
from neptune_amd import abi, scene  # noqa: E402
from neptune_amd.backend import BatchBackend  # noqa: E402
from oracle import oracle          # noqa: E402

NAMES = {0: "depth reached", 1: "goal reached", 2: "beam died out", 3: "no solution"}


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    SH = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    N = int(sys.argv[4]) if len(sys.argv) > 4 else 256
    n_obst = int(sys.argv[5]) if len(sys.argv) > 5 else 100
    budgets = [int(x) for x in (sys.argv[6] if len(sys.argv) > 6 else "100,300,1000").split(",")]
    made = scene.make_scenes(N, n_obst, range(S), workers=min(S, 16))
    p = dataclasses.replace(made[0]["par"], enable_entangle=True)
    be = BatchBackend(p, made[0]["statics"], n_scenes=S)
    for s in range(S):
        be.set_scene_statics(s, made[s]["statics"])
        reps, long_ = scene.static_reps(made[s]["statics"]); be.set_static_reps(reps, long_, scene=s)
    com = np.stack([m["committed"] for m in made]); starts = np.stack([scene.frontend_starts(m) for m in made])
    d_c = be.to_device(com); d_s = be.to_device(starts)
    d_g = torch.zeros(S * N * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_r = torch.zeros(S * N * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_case = torch.zeros(S * N * abi.NEP_MAX_POL * N, dtype=torch.int32, device=be.device)
    d_nx = torch.empty_like(d_c); d_ac = torch.zeros(S * N, dtype=torch.int32, device=be.device)
    cfg = scene.frontend_cfg(p, beam_width=32, entangle=True)
    cfg_plain = scene.frontend_cfg(p, beam_width=32, entangle=False)
    for r in range(rounds):
        be.frontend_ent(cfg, d_c, d_s, d_g, d_r, d_case)
        res = d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy()
        if r == rounds - 1:
            hulls = [be.debug_hulls(s) for s in range(min(SH, S))]
            break
        be.replan(None, d_g, d_ent=d_case)
        be.safety_commit_ent(d_c, be.d_commit, d_g, d_nx, d_ac)
        d_c.copy_(d_nx)
        st = be.solutions()["stats"]["status"]
        print("round %d: front end %s | back end ok %d relaxed %d failed %d | accepted %.3f"
              % (r, {NAMES[k]: int((res["status"] == k).sum()) for k in NAMES}, (st == 0).sum(), (st == 1).sum(), (st == 2).sum(), float(d_ac.float().mean().item())), flush=True)
    print("device beam WITH the entangle check, last round, all %d searches: %s; children pruned by the check %d; ent_overflow %d"
          % (S * N, {NAMES[k]: int((res["status"] == k).sum()) for k in NAMES}, int(res["n_entangled"].sum()), int(res["ent_overflow"].sum())))
    # the same searches once more with the widest beam this build has (64): how many of the lost ones would a wider-beam retry find?
    cfg64 = scene.frontend_cfg(p, beam_width=abi.NEP_FE_MAX_BEAM if hasattr(abi, "NEP_FE_MAX_BEAM") else 64, entangle=True)
    d_g2 = torch.zeros_like(d_g); d_r2 = torch.zeros_like(d_r); d_case2 = torch.zeros_like(d_case)
    be.frontend_ent(cfg64, d_c, d_s, d_g2, d_r2, d_case2)
    res64 = d_r2.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy()
    lost32 = (res["status"] >= 2)
    print("device beam of width 64 WITH the entangle check, same inputs: %s; of the %d searches the width-32 beam ended without a plan (died out / no solution), width 64 finds a plan for %d"
          % ({NAMES[k]: int((res64["status"] == k).sum()) for k in NAMES}, int(lost32.sum()), int((lost32 & (res64["status"] < 2)).sum())))
    try:
        be.check()      # (a sticky capacity flag of the rounds above is reported here, once, and not charged to the searches below)
    except Exception as e:
        print("after the rounds: %s" % e)
    device_astar(be, p, cfg_plain, d_c, d_s, starts, S, N, budgets)
    device_astar_ent(be, p, cfg, d_c, d_s, res, S, N, budgets)
    if SH <= 0:
        return
    oracle.lib()
    jobs = [(s, a) for s in range(min(SH, S)) for a in range(N)]

    def one(job):
        s, a = job
        hx, hn = hulls[s]
        g1, r1 = oracle.frontend_astar(p, cfg_plain, a + 1, starts[s, a], hx, hn, made[s]["statics"], max_pops=20000)
        g2, r2 = oracle.frontend_beam(p, cfg_plain, a + 1, starts[s, a], hx, hn, made[s]["statics"])
        return r1["status"], int(g1["K"]), r2["status"], int(g2["K"])
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        out = np.array(list(ex.map(one, jobs)))
    dev = res["status"].reshape(S, N)[:min(SH, S)].reshape(-1); devK = res["K"].reshape(S, N)[:min(SH, S)].reshape(-1)
    n = len(jobs)
    print("\nsame hulls, same points A, first %d scenes (%d searches):" % (min(SH, S), n))
    print("  %-46s %s" % ("device beam, entangle check ON (what the leg runs)", {NAMES[k]: int((dev == k).sum()) for k in NAMES}))
    print("  %-46s %s" % ("oracle beam, entangle check off", {NAMES[k]: int((out[:, 2] == k).sum()) for k in NAMES}))
    print("  %-46s %s" % ("oracle A* (reference's search, 20 000 pops), off", {NAMES[k]: int((out[:, 0] == k).sum()) for k in NAMES}))
    both_none = int(((dev == 3) & (out[:, 0] == 3)).sum())
    print("  searches with no solution on the device: %d; of these the reference's A* has no solution either: %d (no collision-free first primitive from point A: "
          "the scenario's, not the beam's); found by the A* but not by the device beam: %d" % (int((dev == 3).sum()), both_none, int(((dev == 3) & (out[:, 0] != 3)).sum())))
    print("  plans the device returns (K > 0): %d; the A* returns: %d; A* plans shorter than num_pol: %d" % (int((devK > 0).sum()), int((out[:, 1] > 0).sum()), int(((out[:, 1] > 0) & (out[:, 1] < p.num_pol)).sum())))


def device_astar(be, p, cfg_plain, d_c, d_s, starts, S, N, budgets):
    """the device beam (width 32) and the device A* at every budget, entangle check off, all S * N searches per launch"""
    d_g = torch.zeros(S * N * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_r = torch.zeros(S * N * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d0 = np.hypot(*(starts["pos"][..., :2] - starts["goal"][..., :2]).reshape(-1, 2).T)

    def row(name, res):
        far = d0 > 1.0      # (a search that starts at its goal has no progress to make)
        prog = np.where(res["K"] > 0, (d0 - res["dist_to_goal"]) / np.maximum(d0, 1.0), 0.0)[far]
        print("  %-34s %s; plans (K > 0) %d, mean K %.2f, plans shorter than num_pol %d; progress towards the goal of the %d searches that start more than 1 m from it: mean %.3f median %.3f"
              % (name, {NAMES[k]: int((res["status"] == k).sum()) for k in NAMES}, int((res["K"] > 0).sum()), float(res["K"].mean()),
                 int(((res["K"] > 0) & (res["K"] < p.num_pol)).sum()), int(far.sum()), float(prog.mean()), float(np.median(prog))), flush=True)
    print("\ndevice searches WITHOUT the entangle check, last round's records, all %d searches per launch:" % (S * N))
    be.frontend(cfg_plain, d_c, d_s, d_g, d_r); torch.cuda.synchronize()
    row("beam, width 32", d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy())
    for pops in budgets:
        be.set_fe_astar(pops)
        be.frontend_astar(cfg_plain, d_c, d_s, d_g, d_r); be.check()
        res = d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy()
        row("A*, %d pops (0: on the budget)" % pops, res)
        print("  %-34s pops mean %.0f max %d; nodes mean %.0f max %d; returned depth max %d" % ("", res["n_children"].mean(), res["n_children"].max(),
              res["n_feasible"].mean(), res["n_feasible"].max(), res["depth"].max()), flush=True)


def device_astar_ent(be, p, cfg, d_c, d_s, res_beam, S, N, budgets):
    """the attribution: the reference's best-first search WITH the entangle check (nep_batch_frontend_astar_ent) at every budget against
    the device beam with the check (res_beam), same records, same points A — are the searches without a first primitive the same set?"""
    d_g = torch.zeros(S * N * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_r = torch.zeros(S * N * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    none_beam = res_beam["status"] == 3
    print("\ndevice searches WITH the entangle check, last round's records, all %d searches per launch:" % (S * N))
    print("  %-34s %s; plans (K > 0) %d" % ("beam, width 32", {NAMES[k]: int((res_beam["status"] == k).sum()) for k in NAMES}, int((res_beam["K"] > 0).sum())))
    sets = [("beam 32", none_beam)]
    for pops in budgets:
        be.set_fe_astar(pops)
        be.frontend_astar_ent(cfg, d_c, d_s, d_g, d_r)
        flagged = ""
        try:
            be.check()
        except Exception as e:
            flagged = " [%s]" % e
        res = d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy()
        none = res["status"] == 3
        sets.append(("A* %d" % pops, none))
        print("  %-34s %s; plans (K > 0) %d, mean K %.2f; children dropped by the check %d; ent_overflow in %d searches%s"
              % ("A*, %d pops (0: on the budget)" % pops, {NAMES[k]: int((res["status"] == k).sum()) for k in NAMES}, int((res["K"] > 0).sum()), float(res["K"].mean()),
                 int(res["n_entangled"].sum()), int((res["ent_overflow"] != 0).sum()), flagged), flush=True)
        print("  %-34s without a first primitive: beam %d, A* %d, both %d, beam only %d, A* only %d; of the A*-only ones, with the whole budget spent (no valid end point found) %d, with an empty open list %d"
              % ("", int(none_beam.sum()), int(none.sum()), int((none_beam & none).sum()), int((none_beam & ~none).sum()), int((~none_beam & none).sum()),
                 int((~none_beam & none & (res["n_children"] >= pops)).sum()), int((~none_beam & none & (res["n_children"] < pops)).sum())), flush=True)
    same = all((m == sets[0][1]).all() for _, m in sets[1:])
    print("  the searches without a first primitive are %s for every strategy (%s)" % ("the SAME set" if same else "NOT the same set", ", ".join("%s: %d" % (nm, int(m.sum())) for nm, m in sets)))


if __name__ == "__main__":
    main()
