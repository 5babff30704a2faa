"""The launch sequence of the batched handle's front ends over a table of small cases, through the public Python API alone.

Every case is one handle over `scenes` scenes of 8 (or 5) agents and 2 square statics and two consecutive calls of one front-end entry
point, so that the handle has no history of search times in the first and has it in the second.  The scene counts sit on both sides
of the thresholds of the sequence: 1 024 slots (any launch order) and 2 048 records (the hull kernel) with 8 agents; with 5 agents
205 scenes are 1 025 slots — no multiple of 8: the keyed order without the XCD placement — and 208 scenes 1 040, a multiple of 8.
The beam runs at two (beam_width, num_samples) pairs, one on each side of the 40 KB of LDS that decide between its four- and its
three-workgroups-per-CU instantiation (fe_layout, lds_layout.h, 2 statics): (32, 5) is 35 952 B with 8 agents and 42 240 B with 5,
(48, 5) is 67 072 B and 66 960 B, (16, 5) is 24 144 B with 5.

Each call records a SHA-256 over the bytes of d_guess, d_result and, where the entry point has one, d_case_out (the searches'
measured times are not part of them).  Between the calls the script launches a delimiter — a stand-alone gjk_batch over 64 (i + 1)
problems in front of call i / 2 and behind it — so that a kernel trace of the run can be cut into calls:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/fe_launch_paths.py --out cases.json
    python scripts/launch_trace_list.py --calls cases.json DIR/<host>/kt_kernel_trace.csv --fixture tests/golden/fe_launch_paths.json > launches.txt
    python scripts/fe_launch_paths.py --check tests/golden/fe_launch_paths.json      # the digests alone, exit status 1 on a difference
"""
import argparse
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_STATIC, SEEDS, MAX_POPS = 2, (0, 1, 2, 3), 12
BEAM_SMALL, BEAM_LARGE, BEAM_SMALL_5 = (32, 5), (48, 5), (16, 5)      # (beam_width, num_samples): see the module's docstring


def cases():
    """[(name, agents, scenes, variant)]: the beam at every size, each variant at the sizes where it matters"""
    t = []
    def add(name, agents, sizes, **v):
        t.extend((name, agents, s, v) for s in sizes)
    add("beam", 8, (1, 128, 129, 256, 257))
    add("beam", 5, (205, 208))
    add("beam_large", 8, (1, 129), beam=BEAM_LARGE)
    add("beam_small_5", 5, (208,), beam=BEAM_SMALL_5)
    add("fe_three", 8, (129,), fe_three=1)
    add("fe_xcd_0", 8, (129,), fe_xcd=0)
    add("fe_xcd_0", 5, (208,), fe_xcd=0)
    add("launch_order_off", 8, (129,), launch_order=False)
    add("active_set", 8, (128, 129, 257), active=True)
    add("active_set", 5, (205,), active=True)
    add("active_set_fe_xcd_0", 8, (129,), active=True, fe_xcd=0)
    add("hull_kernel_1", 8, (257,), hull_kernel=1)
    add("hull_kernel_2", 8, (1, 129), hull_kernel=2)
    add("hulls", 8, (129, 257), entry="frontend_hulls")
    add("hulls_active_set", 8, (129,), entry="frontend_hulls", active=True)
    add("ent", 8, (1, 129, 257), entry="frontend_ent")
    add("ent", 5, (205,), entry="frontend_ent")
    add("ent_large", 8, (129,), entry="frontend_ent", beam=BEAM_LARGE)
    add("ent_active_set", 8, (129,), entry="frontend_ent", active=True)
    add("ent_hulls", 8, (129,), entry="frontend_ent_hulls")
    add("ent_hulls_active_set", 8, (129,), entry="frontend_ent_hulls", active=True)
    add("ent_hulls_active_set", 5, (205,), entry="frontend_ent_hulls", active=True)
    add("astar", 8, (1, 129, 257), entry="frontend_astar")
    add("astar_active_set", 8, (129,), entry="frontend_astar", active=True)
    add("astar_ent", 8, (1, 129), entry="frontend_astar_ent")
    add("astar_ent_active_set", 8, (129,), entry="frontend_astar_ent", active=True)
    return t


class Delimiter:
    """a stand-alone gjk_batch whose grid encodes how many went before it"""

    def __init__(self, be):
        self.be, self.n = be, 0
        self.tri = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])

    def __call__(self):
        self.n += 1
        k = 64 * self.n
        self.be.gjk_batch([self.tri] * k, np.zeros((k, 4, 2)))


def run_case(be, scene, abi, torch, base, agents, scenes, v, mark=None):
    """two calls of one handle -> [sha256 of the call's outputs]"""
    entry = v.get("entry", "frontend")
    ent = "ent" in entry.split("_")
    base = [dict(sc, committed=sc["committed"].copy()) for sc in base]
    p = base[0]["par"]
    if ent:
        p = dataclasses.replace(p, enable_entangle=True)
        for k, sc in enumerate(base):                      # (bend points into the records)
            scene.synthetic_entangle(sc, seed=1041 + k, frac=0.25)
    scs = [base[s % len(base)] for s in range(scenes)]
    bb = be.BatchBackend(p, scs[0]["statics"], n_scenes=scenes)
    L = bb_lib(be)
    try:
        for s in range(1, scenes):
            bb.set_scene_statics(s, scs[s]["statics"])
        if ent:
            for s in range(scenes):
                reps, longest = scene.static_reps(scs[s]["statics"])
                bb.set_static_reps(reps, longest, scene=s)
        if "hull_kernel" in v:
            bb.set_hull_kernel(v["hull_kernel"])
        if "launch_order" in v:
            bb.set_launch_order(v["launch_order"])
        for name in ("fe_three", "fe_xcd"):
            if name in v:
                assert L.nep_debug_set_global_option(name.encode(), int(v[name])) == 0
        if v.get("active"):
            mask = (np.random.default_rng(5).random((scenes, agents)) < 0.5).astype(np.int32)
            mask[0, :] = 1
            bb.set_active(torch.from_numpy(mask).to(bb.device))
        if "astar" in entry:
            bb.set_fe_astar(MAX_POPS)
        bw, ns = v.get("beam", BEAM_SMALL)
        cfg = scene.frontend_cfg(p, beam_width=bw, num_samples=ns, entangle=ent)
        starts = np.stack([scene.frontend_starts(sc) for sc in scs])
        d_com = bb.to_device(np.stack([sc["committed"] for sc in scs]))
        d_start = bb.to_device(starts)
        S = scenes * agents
        d_guess = torch.zeros(S * abi.GUESS_DTYPE.itemsize, dtype=torch.uint8, device=bb.device)
        d_res = torch.zeros(S * abi.FE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=bb.device)
        d_case = torch.zeros(S * abi.NEP_MAX_POL * agents, dtype=torch.int32, device=bb.device) if ent else None
        first = d_com
        if entry.endswith("_hulls"):                      # (one block: the whole fleet's hulls, made once for both calls)
            clock = np.zeros((scenes, agents), dtype=abi.GUESS_DTYPE); clock["t_start"] = starts["t_start"]
            first = torch.zeros(bb.hull_block_bytes(), dtype=torch.uint8, device=bb.device)
            bb.hulls(d_com, bb.to_device(clock), first)
        out = []
        for r in range(2):
            torch.cuda.synchronize(bb.device)
            if mark:
                mark()
            if ent:
                getattr(bb, entry)(cfg, first, d_start, d_guess, d_res, d_case)
            else:
                getattr(bb, entry)(cfg, first, d_start, d_guess, d_res)
            torch.cuda.synchronize(bb.device)
            if mark:
                mark()
            h = hashlib.sha256()
            for t in (d_guess, d_res) + ((d_case,) if ent else ()):
                h.update(t.cpu().numpy().tobytes())
            out.append(h.hexdigest())
    finally:
        L.nep_debug_set_global_option(b"fe_three", 0); L.nep_debug_set_global_option(b"fe_xcd", 1)
        bb.close()
    return out


def bb_lib(be):
    from neptune_amd import _lib
    return _lib.lib()


def base_scenes(scene):
    return {n: scene.make_scenes(n, N_STATIC, SEEDS, workers=1) for n in (8, 5)}


def run_table(only=None, mark=None, say=None):
    """-> [{name, agents, scenes, variant, calls: [{sha}]}] of the whole table (only: name:agents:scenes of one case)"""
    import torch
    from neptune_amd import abi, backend, scene
    base = base_scenes(scene)
    rows = []
    for name, agents, scenes, v in cases():
        if only and only != "%s:%d:%d" % (name, agents, scenes):
            continue
        shas = run_case(backend, scene, abi, torch, base[agents], agents, scenes, v, mark)
        rows.append(dict(name=name, agents=agents, scenes=scenes, slots=scenes * agents, variant=v, calls=[dict(sha=s) for s in shas]))
        if say:
            say(name, agents, scenes, [s[:12] for s in shas])
    return rows


def write_fixture(doc, f):
    """the table's answers as JSON, one case per line"""
    head = {k: v for k, v in doc.items() if k != "cases"}
    f.write(json.dumps(head, sort_keys=True)[:-1] + ', "cases": [\n')
    f.write(",\n".join(json.dumps(c, sort_keys=True) for c in doc["cases"]) + "\n]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the table's digests to this file")
    ap.add_argument("--check", default=None, help="compare the digests with this file's")
    ap.add_argument("--only", default=None, help="name:agents:scenes of one case")
    ap.add_argument("--commit", default="", help="the commit the run is of (recorded in --out)")
    a = ap.parse_args()
    from neptune_amd import backend
    rows = run_table(a.only, Delimiter(backend), lambda *w: print(*w, flush=True))
    if a.out:
        with open(a.out, "w") as f:
            write_fixture(dict(statics=N_STATIC, max_pops=MAX_POPS, commit=a.commit, cases=rows), f)
    bad = 0
    if a.check:
        with open(a.check) as f:
            want = {(c["name"], c["agents"], c["scenes"]): c["calls"] for c in json.load(f)["cases"]}
        for row in rows:
            w = want.get((row["name"], row["agents"], row["scenes"]))
            for r, c in enumerate(row["calls"]):
                if w is None or c["sha"] != w[r]["sha"]:
                    bad += 1
                    print("DIFFERS", row["name"], row["agents"], row["scenes"], r)
        if not a.only and len(want) != len(rows):
            bad += 1
            print("DIFFERS: %d cases recorded, %d run" % (len(want), len(rows)))
        print("front-end launch paths: %d cases, %d differences" % (len(rows), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
