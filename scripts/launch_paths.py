"""The launch topology of the batched handle's replan over a table of small cases, through the public Python API alone.

Every case is one handle over `scenes` scenes of 8 agents and 2 square statics (K = 8) and three consecutive replans.  After each
replan the script records the launch-path bits (debug_launch_path), whether launch_order() is None, whether the polish counters were
seen armed, and qp_kernel_name().  The scene counts sit on both sides of the thresholds of the launch sequence: 1 024 slots (the
launch order), 2 048 records (the hull kernel), 4 096 slots (eight segments per wave of the packed separator, and with it the
certificate in the separator's wave).

The polish counters: nep_batch_debug_polish_count reports (0, 0) both for a replan whose pass was not armed and for an armed one that
listed nothing, so "armed" is only visible when a replan lists one.  The handles run with the strictest tolerances the setter takes
(more solves then end without the strict tests); `polish_armed` is true when the counters were non-zero — a lower bound of the
handle's own flag, never above it.  (In scenes this small no replan lists one: the recorded answer is false throughout.)

    python scripts/launch_paths.py --out tests/golden/launch_paths.json       # record
    python scripts/launch_paths.py --check tests/golden/launch_paths.json     # compare, exit status 1 on a difference
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_AGENTS, N_STATIC, SEEDS = 8, 2, (0, 1, 2, 3)
SIZES = (1, 128, 129, 256, 257, 511, 512)


def cases():
    """[(name, scenes, variant)]: the default handle at every size, each variant at the sizes where it matters"""
    t = [("default", s, {}) for s in SIZES]
    def add(name, sizes, **v):
        t.extend((name, s, v) for s in sizes)
    add("hull_kernel_1", (257, 512), hull_kernel=1)
    add("hull_kernel_2", (1, 129, 256), hull_kernel=2)
    add("line_cull_0", (1, 129, 512), line_cull=0.0)
    add("separator_rule_1", (129, 512), separator_rule=1)
    add("separator_pack_unpacked", (129, 512), separator_pack=-1)
    add("separator_pack_8", (129, 511), separator_pack=8)
    add("launch_order_off", (129, 512), launch_order=False)
    add("polish_0", (1, 129), polish=0)
    add("polish_2", (129,), polish=2)
    add("polish_0_line_cull_0", (129,), polish=0, line_cull=0.0)
    add("presolve_kernel_0", (129, 512), options={"presolve_kernel": 0})
    add("presolve_fused_0", (511, 512), options={"presolve_fused": 0})
    add("qp_kernel_2", (1, 129, 512), options={"qp_kernel": 2})
    add("qp_kernel_2_line_cull_0", (129,), options={"qp_kernel": 2}, line_cull=0.0)
    add("active_set", (129, 257, 512), active=True)
    add("two_calls", (129, 257, 512), two_calls=True)
    add("two_calls_hull_kernel_1", (512,), two_calls=True, hull_kernel=1)
    add("scene_statics_before_third", (257, 512), upload_before_third="square")
    add("diamond_before_third", (257, 512), upload_before_third="diamond")
    add("diamond", (1, 257, 512), diamond=True)
    add("entangle", (129, 257, 512), entangle=True)
    add("entangle_hull_kernel_2", (129,), entangle=True, hull_kernel=2)
    return t


def _square(cx, cy, h):
    return np.array([[cx - h, cy - h], [cx + h, cy - h], [cx + h, cy + h], [cx - h, cy + h]])


def _diamond(cx, cy, h):
    return np.array([[cx, cy - h], [cx + h, cy], [cx, cy + h], [cx - h, cy]])


def run_case(be, scene, torch, base, scenes, v):
    """three replans of one handle -> [{bits, launch_order_none, polish_armed, qp_kernel}]"""
    scs = [base[s % len(base)] for s in range(scenes)]
    p = scs[0]["par"]
    cases_ent = None
    if v.get("entangle"):
        p = dataclasses.replace(p, enable_entangle=True)
        base = [dict(sc, committed=sc["committed"].copy()) for sc in base]      # (synthetic_entangle writes bend points into the records)
        scs = [base[s % len(base)] for s in range(scenes)]
        per = [scene.synthetic_entangle(sc, seed=1041 + k, frac=0.25) for k, sc in enumerate(base)]
        cases_ent = [per[s % len(base)] for s in range(scenes)]
    statics = [[np.asarray(q) for q in sc["statics"]] for sc in scs]
    if v.get("diamond"):
        c = np.asarray(statics[0][0]).mean(axis=0)
        statics[0] = [_diamond(c[0], c[1], 1.0), statics[0][1]]
    bb = be.BatchBackend(p, statics[0], n_scenes=scenes)
    for s in range(1, scenes):
        bb.set_scene_statics(s, statics[s])
    bb.set_tolerances(1e-12, 1e-13)             # (see the module's docstring: makes armed polish counters visible)
    if "hull_kernel" in v:
        bb.set_hull_kernel(v["hull_kernel"])
    if "line_cull" in v:
        bb.set_line_cull(v["line_cull"])
    if "separator_rule" in v:
        bb.set_separator_rule(v["separator_rule"])
    if "separator_pack" in v:
        bb.set_separator_pack(v["separator_pack"])
    if "launch_order" in v:
        bb.set_launch_order(v["launch_order"])
    if "polish" in v:
        bb.set_polish(v["polish"])
    for name, value in v.get("options", {}).items():
        bb.debug_option(name, value)
    if v.get("active"):
        mask = (np.random.default_rng(5).random((scenes, N_AGENTS)) < 0.5).astype(np.int32)
        mask[0, :] = 1
        bb.set_active(torch.from_numpy(mask).to(bb.device))
    d_ent = None
    if cases_ent is not None:
        for s in range(scenes):
            reps, longest = scene.static_reps(statics[s])
            bb.set_static_reps(reps, longest, scene=s)
        d_ent = torch.from_numpy(np.ascontiguousarray(np.stack(cases_ent)).reshape(-1)).to(bb.device)
    d_com = bb.to_device(np.stack([sc["committed"] for sc in scs]))
    d_gue = bb.to_device(np.stack([sc["guesses"] for sc in scs]))
    out = []
    for r in range(3):
        if r == 2 and v.get("upload_before_third"):
            c = np.asarray(statics[0][0]).mean(axis=0)
            first = _square(c[0] + 0.5, c[1] - 0.25, 1.0) if v["upload_before_third"] == "square" else _diamond(c[0], c[1], 1.0)
            bb.set_scene_statics(0, [first, statics[0][1]])
        if v.get("two_calls"):
            bb.replan_lines(d_com, d_gue, d_ent)
            bb.replan_solve(d_com, d_gue, d_ent)
        else:
            bb.replan(d_com, d_gue, d_ent)
        torch.cuda.synchronize(bb.device)
        path = bb.debug_launch_path()
        bits = sum(bit for name, bit in bb.LAUNCH_PATH if path[name])
        listed, certified = bb.polish_count()
        out.append(dict(bits=bits, launch_order_none=bb.launch_order() is None, polish_armed=bool(listed or certified), qp_kernel=bb.qp_kernel_name()))
    bb.close()
    return out


def per_agent(be, scene):
    """one optimize() of the per-agent handle with the other agents' hulls (the handle has no launch-path call: run under a kernel
    trace, its launches are its record)"""
    sc = scene.make_scene(5, 3, seed=7)
    p = sc["par"]
    aid = 2
    hx, hn, h0, n0 = be.hulls_batch(sc["committed"], 0.0, p.num_pol, p.T_span, p.drone_radius)
    s = be.PolySolver(p.num_pol, 3, aid, p.T_span, p.pb, p.weight, 0.5, True)
    s.setMaxValues(p.x_min, p.x_max, p.y_min, p.y_max, p.z_min, p.z_max, p.v_max, p.a_max, p.j_max)
    s.setMaxRuntime(0.05); s.setTetherLength(p.tether_length)
    s.setStaticObstVert(sc["statics"])
    g = sc["guesses"][aid - 1]; K = int(g["K"])
    s.setInitTrajectory(np.arange(K + 1) * p.T_span, np.array(g["coeff"])[:, :K, :])
    s.setHulls([[hx[j, i, :hn[j, i]] for i in range(p.num_pol)] for j in range(5) if j != aid - 1])
    s.setHullsNoInflation([[h0[j, i, :n0[j, i]] for i in range(p.num_pol)] if j != aid - 1 else [] for j in range(5)])
    ok, obj = s.optimize()
    print("per-agent optimize:", bool(ok), flush=True)
    s.close()


def write_fixture(doc, f):
    """the table's answers as JSON, one case per line"""
    head = {k: v for k, v in doc.items() if k != "cases"}
    f.write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": [\n')
    f.write(",\n".join(json.dumps(c, sort_keys=True) for c in doc["cases"]) + "\n]}\n")


ANSWERS = ("bits", "launch_order_none", "polish_armed", "qp_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table's answers to this file")
    ap.add_argument("--check", default=None, help="compare the answers with this file's")
    ap.add_argument("--only", default=None, help="name:scenes of one case")
    ap.add_argument("--per-agent", action="store_true", help="after the table, one optimize() of the per-agent handle with hulls")
    a = ap.parse_args()
    import torch
    from neptune_amd import backend, scene
    base = scene.make_scenes(N_AGENTS, N_STATIC, SEEDS, workers=1)
    rows = []
    for name, scenes, v in cases():
        if a.only and a.only != "%s:%d" % (name, scenes):
            continue
        calls = run_case(backend, scene, torch, base, scenes, v)
        rows.append(dict(name=name, scenes=scenes, slots=scenes * N_AGENTS, variant=v, calls=calls))
        print(name, scenes, [(c["bits"], c["launch_order_none"], c["polish_armed"], c["qp_kernel"]) for c in calls], flush=True)
    if a.per_agent:
        per_agent(backend, scene)
    doc = dict(agents=N_AGENTS, statics=N_STATIC, K=8, cases=rows)
    if a.out:
        with open(a.out, "w") as f:
            write_fixture(doc, f)
    bad = 0
    if a.check:
        with open(a.check) as f:
            want = {(c["name"], c["scenes"]): c["calls"] for c in json.load(f)["cases"]}
        for row in rows:
            w = want.get((row["name"], row["scenes"]))
            for r, c in enumerate(row["calls"]):
                if w is None or any(c[k] != w[r][k] for k in ANSWERS):
                    bad += 1
                    print("DIFFERS", row["name"], row["scenes"], r, c, None if w is None else w[r])
        if not a.only and len(want) != len(rows):
            bad += 1
            print("DIFFERS: %d cases recorded, %d run" % (len(want), len(rows)))
        print("launch paths: %d cases, %d differences" % (len(rows), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
