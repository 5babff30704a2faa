"""CPU: the front end's launch plan (plan_frontend, neptune_amd/csrc/launch_plan.h) against the launches recorded on the GPU at the
commit before the plan existed (tests/golden/fe_launch_paths.json: scripts/fe_launch_paths.py under a kernel trace, reduced by
scripts/launch_trace_list.py --calls).  tests/cpp/fe_launch_plan_check.cpp — host code, its own main, nothing but the header — gets
every case's facts call by call and must print the launch list the trace showed for that call: kernel names, grids, workgroup sizes,
in order, none left out.  Built plain and with -fsanitize=address,undefined.

The trace's LDS column holds a kernel's static LDS only (the dynamic bytes of a launch are not in it), so the plan's lds_bytes are
checked here against fe_layout's figures for the table's shapes, which scripts/fe_launch_paths.py states."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fe_launch_paths.json")


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def call_facts(doc, case):
    """the facts of a fixture case's calls, as scripts/fe_launch_paths.py set the handle up (fe_history is the program's to carry)"""
    v = case["variant"]
    entry = v.get("entry", "frontend")
    words = entry.split("_")
    bw, ns = v.get("beam", (32, 5))
    return dict(num_agents=case["agents"], n_static=doc["statics"], num_pol=8, hull_mode=v.get("hull_kernel", 0), slots=case["scenes"] * case["agents"],
                n_scenes=case["scenes"], best_first=int("astar" in words), ent=int("ent" in words), beam_width=bw, num_samples=ns, ent_samples=3,
                have_recs=int("hulls" not in words), active=int(bool(v.get("active"))), lpt=int(v.get("launch_order", True)),
                order_key_ok=int(v.get("launch_order", True)), big_beta=int("ent" in words and "astar" not in words),
                fe_three=v.get("fe_three", 0), fe_xcd=v.get("fe_xcd", 1))


def script(doc):
    lines, keys = [], []
    for case in doc["cases"]:
        lines.append("new")
        for r in range(len(case["calls"])):
            lines.append(" ".join("%s=%s" % kv for kv in call_facts(doc, case).items()))
            keys.append((case["name"], case["agents"], case["scenes"], r))
    return "\n".join(lines) + "\n", keys


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fe_launch_plan") / ("fe_launch_plan_check_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                       [os.path.join(ROOT, "tests", "cpp", "fe_launch_plan_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("fe_launch_plan_check ok\n"), (r.stdout[-400:], r.stderr[-2000:])
    return r.stdout.splitlines()[:-1]


def test_fixture_covers_the_table():
    """sizes on both sides of every threshold, every entry point, two calls each, launches and digests for every call"""
    doc = load()
    assert doc["commit"] and doc["statics"] == 2
    sizes = {(c["agents"], c["scenes"]) for c in doc["cases"] if c["name"] == "beam"}
    assert sizes == {(8, 1), (8, 128), (8, 129), (8, 256), (8, 257), (5, 205), (5, 208)}
    names = {c["name"] for c in doc["cases"]}
    for want in ("beam_large", "fe_three", "fe_xcd_0", "launch_order_off", "active_set", "hull_kernel_1", "hull_kernel_2", "hulls", "ent", "ent_active_set",
                 "ent_hulls", "ent_hulls_active_set", "astar", "astar_active_set", "astar_ent", "astar_ent_active_set"):
        assert want in names, want
    assert {c["variant"].get("entry", "frontend") for c in doc["cases"]} == {"frontend", "frontend_hulls", "frontend_ent", "frontend_ent_hulls", "frontend_astar", "frontend_astar_ent"}
    assert all(len(c["calls"]) == 2 and all(len(k["sha"]) == 64 and k["launches"] for k in c["calls"]) for c in doc["cases"])
    assert len({(c["name"], c["agents"], c["scenes"]) for c in doc["cases"]}) == len(doc["cases"])


def test_plan_implies_the_launches_the_trace_showed(exe):
    doc = load()
    text, keys = script(doc)
    answers = run(exe, text)
    assert len(answers) == len(keys)
    ids = doc["launch_ids"]
    want = {(c["name"], c["agents"], c["scenes"], r): [ids[k] for k in call["launches"].split()] for c in doc["cases"] for r, call in enumerate(c["calls"])}
    seen, bad = set(), []
    for key, line in zip(keys, answers):
        got = line.split(" # ")[0].split(" ; ")
        seen.add(key)
        if got != want[key]:
            bad.append((key, got, want[key]))
    assert not bad, bad[:4]
    assert seen == set(want)                              # none left out


def test_lds_bytes_and_history(exe):
    """the dynamic LDS of the table's shapes (fe_layout, 2 statics, 8 intervals: the figures scripts/fe_launch_paths.py states, and the
    entangle-aware and big-record ones of the same shapes), and what a call leaves behind: a beam call history, a best-first call
    what it found"""
    base = "n_static=2 num_pol=8 n_scenes=129 have_recs=1 lpt=1 order_key_ok=1 "
    rows = [("num_agents=8 slots=1032 beam_width=32 num_samples=5", (35952, 0, 0, 1)), ("num_agents=8 slots=1032 beam_width=48 num_samples=5", (67072, 0, 0, 1)),
            ("num_agents=5 slots=645 beam_width=32 num_samples=5", (42240, 0, 0, 1)), ("num_agents=5 slots=645 beam_width=16 num_samples=5", (24144, 0, 0, 1)),
            ("num_agents=8 slots=1032 beam_width=32 num_samples=5 ent=1 big_beta=1", (36352, 133632, 36352, 1)),
            ("num_agents=8 slots=1032 beam_width=32 num_samples=5 ent=1 big_beta=0", (36352, 36352, 0, 1)),
            ("num_agents=8 slots=1032 beam_width=48 num_samples=5 ent=1 big_beta=1", (67856, 67856, 0, 1)),      # (the lists would not fit the CU's 160 KB)
            ("num_agents=8 slots=1032 best_first=1 beam_width=32 num_samples=5", (0, 0, 0, 0)),
            ("num_agents=8 slots=1032 best_first=1 ent=1 beam_width=32 num_samples=5 fe_history=1", (24848, 0, 0, 1))]
    answers = run(exe, "".join("new\n" + base + facts + "\n" for facts, _ in rows))
    got = [tuple(int(w) for w in line.split(" # ")[1].split()) for line in answers]
    assert got == [w for _, w in rows], (got, rows)
