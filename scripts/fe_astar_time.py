"""Development aid: device time of frontend_astar_kernel<false> (the reference's best-first search, one wave per search) on S seeded scenes of
N agents + M obstacles at several pop budgets, next to the beam front end (width 32) on the same inputs and to the oracle's
orc_frontend_astar on 16 host threads for a sample of the same slots.  Per launch: hipEvent time of a captured graph replayed (hulls +
search), after a warm-up.  With a PROFILE=1 library (NEP_BACKEND_LIB) and NEP_QP_PROFILE set, the wave's cycles per phase as well (one
phase numbering for both instantiations, PHASES; without the check "entangle propagation" and "state copy" stay zero).
--ent: frontend_astar_kernel<true> (the same search with the entangle check) next to the plain A* and to the beam with
the check, on the same scenes with config-5 style tethers (scene.synthetic_entangle), and tests/astar_ent_ref.py on host processes for a
sample of the slots (its pop counts must equal the device's).
--ent --team: frontend_astar_kernel<true> (one wave per search) next to frontend_astar_team_kernel (four waves per search)
on the same inputs in one run: one captured graph per form, replayed in alternation; per size (searches = scenes x agents) and budget the
time per launch of both, their spread, the us per pop of the longest search and whether every output byte is equal.
   python scripts/fe_astar_time.py [--ent] [scenes=128] [agents=64] [obstacles=20] [pops=100,300,1000] [host_sample=256]
   python scripts/fe_astar_time.py --ent --team [searches=64,256,1024] [agents=64] [obstacles=20] [pops=100,300] [rounds=7]"""
import os, sys, time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
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


PHASES = ("pop", "GJK + bases", "fe_child", "entangle propagation", "lookup + group", "commit", "state copy", "setup + result")      # AS_TICK's numbering (fe_astar.h)


def print_phases(rows):
    """rows: debug_phase_cycles of a sample of slots ([8]: pops)"""
    tot_c = rows[:, :8].sum(axis=1).mean()
    print("   cycles per search (mean of %d slots): %s; per pop %.0f" % (len(rows), ", ".join("%s %.0f (%.0f %%)" % (nm, rows[:, k].mean(), 100 * rows[:, k].mean() / max(tot_c, 1)) for k, nm in enumerate(PHASES)),
                                                                         rows[:, :7].sum() / max(rows[:, 8].sum(), 1)), flush=True)


def _ref_pops(job):
    """tests/astar_ent_ref.py on one slot (a host process): pops, status"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import astar_ent_ref, helpers
    sc, a, cfg_t, start, hulls, pops = job
    cfg = abi.nep_fe_cfg(*cfg_t)
    ent = helpers.ent_inputs(sc, a, t0=float(start["t_start"]))
    _, r, _, _ = astar_ent_ref.astar(sc["par"], cfg, a + 1, start, hulls, sc["statics"], pops, ent=ent)
    return r["n_children"], r["status"], r["n_entangled"]


def main_ent(argv):
    import dataclasses
    S = int(argv[0]) if len(argv) > 0 else 128
    N = int(argv[1]) if len(argv) > 1 else 64
    M = int(argv[2]) if len(argv) > 2 else 20
    budgets = [int(x) for x in (argv[3] if len(argv) > 3 else "100,300").split(",")]
    n_host = int(argv[4]) if len(argv) > 4 else 64
    made = scene.make_scenes(N, M, range(S), workers=min(S, 16))
    for s, m in enumerate(made):
        m["par"] = dataclasses.replace(m["par"], enable_entangle=True)
        scene.synthetic_entangle(m, seed=900 + s)
    p = made[0]["par"]
    be = BatchBackend(p, made[0]["statics"], n_scenes=S)
    for s in range(S):
        be.set_scene_statics(s, made[s]["statics"])
        reps, long_ = scene.static_reps(made[s]["statics"]); be.set_static_reps(reps, long_, scene=s)
    com = np.stack([m["committed"] for m in made]); starts = np.stack([scene.frontend_starts(m) for m in made])
    d_c = be.to_device(com); d_s = be.to_device(starts)
    n = S * N
    d_g = torch.zeros(n * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_r = torch.zeros(n * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=be.device)
    d_case = torch.zeros(n * abi.NEP_MAX_POL * N, dtype=torch.int32, device=be.device)
    cfg = scene.frontend_cfg(p, beam_width=32); cfg_e = scene.frontend_cfg(p, beam_width=32, entangle=True)
    print("%d searches (%d scenes of %d agents + %d obstacles), tethers with 2-4 bend points" % (n, S, N, M))
    ms_b, all_ms = replay_ms(lambda: be.frontend(cfg, d_c, d_s, d_g, d_r))
    print("beam, width 32, check off: %.3f ms per launch (replays: %s)" % (ms_b, " ".join("%.3f" % x for x in all_ms)), flush=True)
    ms_be, all_ms = replay_ms(lambda: be.frontend_ent(cfg_e, d_c, d_s, d_g, d_r, d_case))
    print("beam, width 32, check on:  %.3f ms per launch (replays: %s): %.1f x" % (ms_be, " ".join("%.3f" % x for x in all_ms), ms_be / ms_b), flush=True)
    profile = os.environ.get("NEP_QP_PROFILE") is not None
    sample = np.linspace(0, n - 1, min(n_host, n)).astype(int)
    hulls = {}
    for pops in budgets:
        be.set_fe_astar(pops)
        ms_p, all_p = replay_ms(lambda: be.frontend_astar(cfg, d_c, d_s, d_g, d_r))
        be.check()
        res_p = d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy()
        ms, all_ms = replay_ms(lambda: be.frontend_astar_ent(cfg_e, d_c, d_s, d_g, d_r, d_case))
        flagged = None
        try:
            be.check()
        except Exception as e:      # (a fixed-record overflow is reported, not fatal here)
            flagged = str(e)
        res = d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE).copy()
        for nm, m_, am, r_, conc in (("A*, check off", ms_p, all_p, res_p, 256 * 12), ("A*, check on ", ms, all_ms, res, 256 * 4)):      # (waves a 256-CU chip holds: three per SIMD, one per SIMD)
            tot = int(r_["n_children"].sum()); mx = int(r_["n_children"].max())
            print("%s, %d pops: %.3f ms per launch (replays: %s); pops per search mean %.1f max %d, nodes mean %.1f max %d; %.2f us per pop of the longest search (launch / max pops), %.2f us per pop per wave (launch x concurrent waves / all pops: see DESIGN section 31), %.0f searches per second"
                  % (nm, pops, m_, " ".join("%.3f" % x for x in am), tot / n, mx, r_["n_feasible"].mean(), int(r_["n_feasible"].max()), 1e3 * m_ / max(mx, 1),
                     1e3 * m_ * min(n, conc) / max(tot, 1), n / (m_ * 1e-3)), flush=True)
        print("   check on / check off: %.1f x per launch; statuses on %s off %s; children dropped by the check %d; searches with ent_overflow %d%s"
              % (ms / ms_p, {k: int((res["status"] == k).sum()) for k in range(4)}, {k: int((res_p["status"] == k).sum()) for k in range(4)},
                 int(res["n_entangled"].sum()), int((res["ent_overflow"] != 0).sum()), " (%s)" % flagged if flagged else ""), flush=True)
        if profile:
            rows = np.array([be.debug_phase_cycles(2 * int(s_)) for s_ in np.linspace(0, n - 1, min(64, n)).astype(int)], dtype=np.float64)
            print_phases(rows)
        if n_host > 0:
            for i in sample:
                s_ = int(i) // N
                if s_ not in hulls:
                    hulls[s_] = be.debug_hulls(s_)
            cfg_t = tuple(getattr(cfg_e, f) for f, _ in abi.nep_fe_cfg._fields_)
            jobs = [(made[int(i) // N], int(i) % N, cfg_t, starts[int(i) // N, int(i) % N], hulls[int(i) // N], pops) for i in sample]
            t0 = time.perf_counter()
            with ProcessPoolExecutor(16) as ex:
                out = np.array(list(ex.map(_ref_pops, jobs)))
            dt = time.perf_counter() - t0
            same = int(((out[:, 0] == res["n_children"][sample]) & (out[:, 1] == res["status"][sample]) & (out[:, 2] == res["n_entangled"][sample])).sum())
            print("   tests/astar_ent_ref.py, 16 host processes, %d of the slots: %.1f s; pops, status and n_entangled equal to the device's in %d of %d"
                  % (len(sample), dt, same, len(sample)), flush=True)
    be.close()


PHASES_TEAM = ("pop", "GJK + bases", "fe_child", "dense crossing pass", "surgery + lookup + group", "commit", "state copy", "setup + result")      # frontend_astar_team_kernel's AS_TICK


def capture(fn):
    """fn() captured after two eager calls -> the graph"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin(); fn(); g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    g.replay(); torch.cuda.synchronize()
    return g


def timed(g):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main_team(argv):
    import dataclasses
    sizes = [int(x) for x in (argv[0] if len(argv) > 0 else "64,256,1024").split(",")]
    N = int(argv[1]) if len(argv) > 1 else 64
    M = int(argv[2]) if len(argv) > 2 else 20
    budgets = [int(x) for x in (argv[3] if len(argv) > 3 else "100,300").split(",")]
    rounds = int(argv[4]) if len(argv) > 4 else 7
    S_max = max(1, max(sizes) // N)
    made = scene.make_scenes(N, M, range(S_max), workers=min(S_max, 16))
    for s, m in enumerate(made):
        m["par"] = dataclasses.replace(m["par"], enable_entangle=True)
        scene.synthetic_entangle(m, seed=900 + s)
    p = made[0]["par"]
    profile = os.environ.get("NEP_QP_PROFILE") is not None
    cfg_e = scene.frontend_cfg(p, beam_width=32, entangle=True)
    print("one wave per search against four (hulls + search, a captured graph each, replayed in alternation, %d rounds); %d agents + %d obstacles, tethers with 2-4 bend points" % (rounds, N, M))
    for size in sizes:
        S = max(1, size // N); n = S * N
        be = BatchBackend(p, made[0]["statics"], n_scenes=S)
        for s in range(S):
            be.set_scene_statics(s, made[s]["statics"])
            reps, long_ = scene.static_reps(made[s]["statics"]); be.set_static_reps(reps, long_, scene=s)
        d_c = be.to_device(np.stack([m["committed"] for m in made[:S]])); d_s = be.to_device(np.stack([scene.frontend_starts(m) for m in made[:S]]))
        out = {t: (torch.zeros(n * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=be.device), torch.zeros(n * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=be.device),
                   torch.zeros(n * abi.NEP_MAX_POL * N, dtype=torch.int32, device=be.device)) for t in (1, 4)}
        for pops in budgets:
            be.set_fe_astar(pops)
            graphs = {}
            for t in (1, 4):
                be.set_fe_astar_team(t)
                graphs[t] = capture(lambda: be.frontend_astar_ent(cfg_e, d_c, d_s, *out[t]))
                assert be.fe_astar_team() == t
            ms = {1: [], 4: []}
            for _ in range(rounds):
                for t in (1, 4):
                    ms[t].append(timed(graphs[t]))
            try:
                be.check()
            except Exception:      # (a fixed-record overflow is reported by both forms alike)
                pass
            same = all(bool((a == b).all()) for a, b in zip(out[1], out[4]))
            res = out[4][1].cpu().numpy().view(abi.FE_RESULT_DTYPE)
            mx = int(res["n_children"].max())
            m1, m4 = float(np.median(ms[1])), float(np.median(ms[4]))
            print("%5d searches, %4d pops: one wave %.3f ms (min %.3f max %.3f), four waves %.3f ms (min %.3f max %.3f): %.2f x; us per pop of the longest search (%d pops) %.1f against %.1f; outputs %s"
                  % (n, pops, m1, min(ms[1]), max(ms[1]), m4, min(ms[4]), max(ms[4]), m1 / m4, mx, 1e3 * m1 / max(mx, 1), 1e3 * m4 / max(mx, 1), "equal byte for byte" if same else "DIFFER"), flush=True)
            if profile:
                for t, names in ((1, PHASES), (4, PHASES_TEAM)):
                    graphs[t].replay(); torch.cuda.synchronize()
                    rows = np.array([be.debug_phase_cycles(2 * int(s_)) for s_ in np.linspace(0, n - 1, min(64, n)).astype(int)], dtype=np.float64)
                    tot_c = rows[:, :8].sum(axis=1).mean()
                    print("   %d wave(s), cycles per search (mean of %d slots): %s; per pop %.0f" % (t, len(rows), ", ".join("%s %.0f (%.0f %%)" % (nm, rows[:, k].mean(), 100 * rows[:, k].mean() / max(tot_c, 1)) for k, nm in enumerate(names)),
                                                                                                  rows[:, :7].sum() / max(rows[:, 8].sum(), 1)), flush=True)
            del graphs
        be.close()


def main():
    if "--ent" in sys.argv and "--team" in sys.argv:
        return main_team([x for x in sys.argv[1:] if x not in ("--ent", "--team")])
    if "--ent" in sys.argv:
        return main_ent([x for x in sys.argv[1:] if x != "--ent"])
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
            print_phases(rows)
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
