"""CPU: the replan's launch plan (neptune_amd/csrc/launch_plan.h) against the launch paths recorded on the GPU at the commit before the
plan existed (tests/golden/launch_paths.json, written by scripts/launch_paths.py).  tests/cpp/launch_plan_check.cpp — host code, its own
main, nothing but the header — gets every case's facts call by call and must answer what the handle answered then: the launch-path
bits, whether the QP ran in launch order, the polish counters, the interior-point kernel.  Built plain and with
-fsanitize=address,undefined.

The polish counters: the fixture holds what nep_batch_debug_polish_count showed, which is a lower bound of "armed" (an armed pass that
lists nothing reads (0, 0) as an unarmed one does): the plan must be armed wherever the fixture saw counts, and the fixture must have
seen none wherever the plan is not armed."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_paths.json")
POOL = 1024                     # Engine::kScratchPool


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def call_facts(doc, case, r):
    """the facts of call r (0..2) of a fixture case, as scripts/launch_paths.py set the handle up -> [{fact: value}] (one per run())"""
    v = case["variant"]
    N, S, scenes = doc["agents"], doc["statics"], case["scenes"]
    opt = v.get("options", {})
    cull = v.get("line_cull", 4.0)                        # (kAutoCullRadius)
    polish = v.get("polish", 1)
    boxy = not v.get("diamond") and not (v.get("upload_before_third") == "diamond" and r == 2)
    f = dict(num_agents=N, num_pol=8, n_hull=N, n_static=S, ent_enabled=int(bool(v.get("entangle"))), hull_mode=v.get("hull_kernel", 0), skip_own=1,
             sep_rule=v.get("separator_rule", 0), cull_radius=cull, use_reg=int(opt.get("qp_kernel", 0) != 2), lpt=int(v.get("launch_order", True)),
             presolve_kernel=opt.get("presolve_kernel", 1), presolve_fused=opt.get("presolve_fused", 1), skip_lps=1, no_redo=0,
             statics_boxy=int(boxy), static_boxes_ok=1, sep_pack=v.get("separator_pack", 0), polish=int(polish != 0), polish_presolve=int(polish in (1, 2)),
             polish_buffers=1, order_ok=1, order_key_ok=1, presolved_ok=1,
             slots=scenes * N, n_scenes=scenes, n_rec=N, hull_pb=0, have_recs=1, lines_override=0, active=int(bool(v.get("active"))))
    # the pool of row-scratch areas, as the handle's last sizing left it (create, set_line_cull, set_separator_rule; not the debug options)
    sized_skip = cull > 0 and f["sep_rule"] == 0 and not v.get("diamond")
    f["scratch_chunks"] = POOL if (sized_skip and scenes * N > POOL) else 0
    if v.get("two_calls"):
        return [dict(f, phases=1), dict(f, phases=2)]
    return [dict(f, phases=3)]


def script(doc):
    """stdin of the check program, and the (case, call) of every answer line that is compared"""
    lines, keys = [], []
    for case in doc["cases"]:
        lines.append("new")
        for r in range(len(case["calls"])):
            runs = call_facts(doc, case, r)
            for k, f in enumerate(runs):
                lines.append(" ".join("%s=%s" % kv for kv in f.items()))
                keys.append((case["name"], case["scenes"], r) if k == len(runs) - 1 else None)
    return "\n".join(lines) + "\n", keys


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("launch_plan") / ("launch_plan_check_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                       [os.path.join(ROOT, "tests", "cpp", "launch_plan_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_fixture_covers_the_table():
    """every size on both sides of the three thresholds, every variant, three calls each"""
    doc = load()
    assert (doc["agents"], doc["statics"], doc["K"]) == (8, 2, 8)
    assert {c["scenes"] for c in doc["cases"] if c["name"] == "default"} == {1, 128, 129, 256, 257, 511, 512}
    names = {c["name"] for c in doc["cases"]}
    for want in ("hull_kernel_1", "hull_kernel_2", "line_cull_0", "separator_rule_1", "separator_pack_unpacked", "separator_pack_8", "launch_order_off",
                 "polish_0", "polish_2", "presolve_kernel_0", "presolve_fused_0", "qp_kernel_2", "active_set", "two_calls", "scene_statics_before_third",
                 "diamond", "diamond_before_third", "entangle"):
        assert want in names, want
    assert all(len(c["calls"]) == 3 for c in doc["cases"])
    assert len({(c["name"], c["scenes"]) for c in doc["cases"]}) == len(doc["cases"])


def test_plan_answers_what_the_handle_answered(exe):
    doc = load()
    text, keys = script(doc)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("launch_plan_check ok\n"), (r.stdout[-400:], r.stderr[-2000:])
    answers = r.stdout.splitlines()[:-1]
    assert len(answers) == len(keys)
    want = {(c["name"], c["scenes"], k): call for c in doc["cases"] for k, call in enumerate(c["calls"])}
    seen, bad = set(), []
    for key, line in zip(keys, answers):
        if key is None:                                   # (the geometry half of a two-call replan: the fixture records the round)
            continue
        bits, order_none, armed, kernel = line.split()[:4]
        w = want[key]
        seen.add(key)
        if int(bits) != w["bits"] or bool(int(order_none)) != w["launch_order_none"] or kernel != w["qp_kernel"] or (w["polish_armed"] and not int(armed)):
            bad.append((key, line, w))
    assert not bad, bad[:6]
    assert seen == set(want)                              # none left out


def test_polish_is_armed_by_the_settings_alone(exe):
    """the fixture's scenes list no replan for the polish pass, so the armed flag is checked here against nep_*_set_polish's contract:
    off -> never; 1 / 2 -> with the register kernel; 3 -> only without the line presolve; never with the LDS-placement kernel"""
    base = "num_agents=8 num_pol=8 n_hull=8 n_static=2 skip_own=1 polish_buffers=1 slots=8 n_scenes=1 n_rec=8 have_recs=1 phases=3 "
    rows = [("polish=0 polish_presolve=0 use_reg=1 cull_radius=4", 0), ("polish=1 polish_presolve=1 use_reg=1 cull_radius=4", 1),
            ("polish=1 polish_presolve=0 use_reg=1 cull_radius=4", 0), ("polish=1 polish_presolve=0 use_reg=1 cull_radius=0", 1),
            ("polish=1 polish_presolve=1 use_reg=0 cull_radius=0", 0), ("polish=1 polish_presolve=1 use_reg=1 cull_radius=4 polish_buffers=0", 0)]
    text = "".join("new\n" + base + facts + "\n" for facts, _ in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(line.split()[2]) for line in r.stdout.splitlines()[:-1]]
    assert got == [w for _, w in rows], (got, rows)
