"""CPU: the launch plan of the best-first search on four waves per search (FrontendFacts::team, neptune_amd/csrc/launch_plan.h) and
the LDS layout of its kernel (astar_ent_team_layout, lds_layout.h).  tests/cpp/fe_team_plan_check.cpp — host code, its own main, nothing
but the headers, built plain and with -fsanitize=address,undefined and run as a stand-alone program — gets the facts of every call of
tests/golden/fe_launch_paths.json (the launches recorded on the GPU before the team form existed) and checks for each: team = 1 is the
plan as it was, field for field; team = 4 changes the workgroup size and the team form's LDS bytes alone, and only for the best-first
search with the check; then the layout: sections inside the launch, aligned, disjoint, the byte count the launch uses.  Here the
searches' launch of the team = 1 plan is compared with the recorded one."""
import os
import subprocess

import pytest

from test_fe_launch_plan_cpu import call_facts, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fe_team_plan") / ("fe_team_plan_check_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                       [os.path.join(ROOT, "tests", "cpp", "fe_team_plan_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("fe_team_plan_check ok\n"), (r.stdout[-400:], r.stderr[-2000:])
    return r.stdout.splitlines()[:-1]


def test_team_one_is_the_plan_as_it_was_and_team_four_changes_two_fields(exe):
    doc = load()
    cases = [c for c in doc["cases"]]
    assert sum(c["name"].startswith("astar_ent") for c in cases) >= 2 and any(not c["name"].startswith("astar") for c in cases)
    text = "".join(" ".join("%s=%s" % kv for kv in call_facts(doc, c).items()) + "\n" for c in cases)
    out = run(exe, text)
    assert len(out) == 2 * len(cases) + 1
    ids = doc["launch_ids"]
    team_lds = None
    for k, c in enumerate(cases):
        t1, t4 = out[2 * k], out[2 * k + 1]
        assert t1.startswith("T1 ") and t4.startswith("T4 ")
        f1, l1 = t1[3:].split(" # "); f4, l4 = t4[3:].split(" # ")
        ent = c["variant"].get("entry", "frontend") == "frontend_astar_ent"
        slots = c["scenes"] * c["agents"]
        assert f1.endswith("team=1 team_lds=0") and l1 == "%dx1x1 | 64x1x1" % (slots * 64)
        if ent:
            # the recorded launch of the searches: the last launch of the call, one wave per slot
            last = ids[c["calls"][0]["launches"].split()[-1]]
            assert last == "void nep::frontend_astar_kernel<true> | %s | 0" % l1, (last, l1)
            assert f4.rsplit(" team=", 1)[0] == f1.rsplit(" team=", 1)[0] and l4 == "%dx1x1 | 256x1x1" % (slots * 256)
            lds = int(f4.rsplit("team_lds=", 1)[1])
            assert f4.endswith("team=4 team_lds=%d" % lds) and lds > 24848
            team_lds = lds
        else:
            assert f4 == f1 and l4 == l1, (c["name"], f1, f4)      # every other call keeps its form whatever the setting
    # the layout: its byte count is the one the launch uses, the one-wave carve is inside it, within a CU's LDS
    assert out[-1] == "layout bytes=%d one=24848" % team_lds and team_lds <= 160 * 1024
