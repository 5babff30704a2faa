"""CPU: the kernels' dynamic-LDS layouts (neptune_amd/csrc/lds_layout.h) against the byte counts and derived counts the launchers
computed at the commit before the header existed (tests/golden/lds_bytes.json: recorded there by calling that commit's own size
functions — separator_lds_bytes, frontend_lds_bytes, ... — and its launchers' inline expressions hoisted verbatim; the fixture names the
commit and holds the grid).  tests/cpp/lds_layout_check.cpp — host code, its own main, nothing but the header — first checks every
layout over a grid of its own (inside the launch, aligned, disjoint but for the declared aliases, counts consistent with the offsets),
then answers the fixture's rows.  Built plain and with -fsanitize=address,undefined."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "lds_bytes.json")


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def rows_of(doc, kind, **match):
    return [r for r in doc["rows"] if r["kind"] == kind and all(r["in"][k] == v for k, v in match.items())]


def one(doc, kind, **match):
    r = rows_of(doc, kind, **match)
    assert len(r) == 1, (kind, match, len(r))
    return r[0]["out"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lds_layout") / ("lds_layout_check_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                       [os.path.join(ROOT, "tests", "cpp", "lds_layout_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_layouts_answer_what_the_launchers_computed(exe):
    doc = load()
    lines = [" ".join([r["kind"]] + [str(r["in"][k]) for k in doc["fields"][r["kind"]]["in"]]) for r in doc["rows"]]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("lds_layout_check ok\n"), (r.stdout[-600:], r.stderr[-2000:])
    answers = r.stdout.splitlines()[:-2]
    assert len(answers) == len(doc["rows"])               # every row answered, none left out
    bad = []
    for row, asked, line in zip(doc["rows"], lines, answers):
        echo, _, vals = line.partition(" : ")
        assert echo == asked, (echo, asked)
        want = [row["out"][k] for k in doc["fields"][row["kind"]]["out"]]
        if [int(v) for v in vals.split()] != want:
            bad.append((asked, vals, want))
    assert not bad, bad[:8]


def test_fixture_is_the_parents_and_holds_the_bench_shapes():
    doc = load()
    assert len(doc["parent_commit"]) == 40 and "hoisted verbatim" in doc["recorded_with"]
    assert len({json.dumps([r["kind"], r["in"]], sort_keys=True) for r in doc["rows"]}) == len(doc["rows"])
    for ent in (0, 1):                                    # the headline's 64 agents + 20 statics, config 5's 256 + 100
        for N, S in ((64, 20), (256, 100)):
            one(doc, "sep", n_hull=N, N=N, S=S, ent=ent)
            one(doc, "frontend", N=N, S=S, W=32, ns=5, num_pol=8, ent=ent, ent_ns=3 * ent)
    one(doc, "ent_check", N=256, S=100), one(doc, "resolve", N=64), one(doc, "audit", N=64, S=20, vstride=16), one(doc, "mission", N=64, n_vert=512, n_poly=64)


def test_flip_points_lie_where_the_issue_lists_them():
    """both sides of every branch of the layouts, at NEP_SEP_LDS = 10 KiB and NEP_MAX_POL = 8: the recorded values change there and only as
    the branch says"""
    doc = load()
    # front end, rf_alias (4 (N + S) + 768 >= cap): without it r_f has cap doubles of its own
    for W, cap, (lo, hi) in ((32, 800, ((5, 2), (6, 2))), (33, 825, ((12, 2), (13, 2))), (64, 1600, ((187, 20), (188, 20)))):
        for ent in (0, 1):
            a = one(doc, "frontend", N=lo[0], S=lo[1], W=W, ns=5, num_pol=8, ent=ent, ent_ns=3 * ent)
            b = one(doc, "frontend", N=hi[0], S=hi[1], W=W, ns=5, num_pol=8, ent=ent, ent_ns=3 * ent)
            assert a["children_cap"] == b["children_cap"] == cap
            assert 4 * sum(lo) + 768 < cap <= 4 * sum(hi) + 768
            assert a["bytes"] - b["bytes"] > 8 * cap - 128, (W, a, b)      # (one agent more costs 40-odd bytes, the alias saves 8 cap)
    # the per-rank stride: beam width 32 | 33; the cap floor of 64
    assert one(doc, "frontend", N=12, S=2, W=33, ns=5, num_pol=8, ent=0, ent_ns=0)["bytes"] - one(doc, "frontend", N=8, S=2, W=32, ns=5, num_pol=8, ent=0, ent_ns=0)["bytes"] > 32 * 8 * 20
    assert one(doc, "frontend", N=8, S=2, W=1, ns=2, num_pol=8, ent=0, ent_ns=0)["children_cap"] == 64
    # the entangle tail: mask words per rank, N = 32 | 33 (MW), S = 0 | 32 | 33 (SW); f_bits padded to 4 bytes
    tail = lambda N, S: (one(doc, "frontend", N=N, S=S, W=32, ns=5, num_pol=8, ent=1, ent_ns=3)["bytes"] - one(doc, "frontend", N=N, S=S, W=32, ns=5, num_pol=8, ent=0, ent_ns=0)["bytes"])
    words = lambda N, S: 32 * 4 * (2 * ((N + 31) // 32) + (S + 31) // 32) + (N + 3) // 4 * 4 + 8 * ((N + 31) // 32)
    for N, S in ((32, 0), (33, 0), (8, 0), (8, 32), (8, 33), (7, 33), (9, 33), (33, 33)):
        assert abs(tail(N, S) - words(N, S)) < 16, (N, S, tail(N, S), words(N, S))      # (both totals are rounded up to 16)
    # the big-record lists: granted when the launch stays within 160 KiB, then they start where the plain launch ends
    fits = [r["out"] for r in rows_of(doc, "frontend", ent=1)]
    assert any(o["big_lds_off"] for o in fits) and any(not o["big_lds_off"] for o in fits)
    for o in fits:
        assert (o["big_lds_off"], o["big_bytes"]) == ((o["bytes"], o["bytes"] + 256 * 380) if o["bytes"] + 256 * 380 <= 160 * 1024 else (0, o["bytes"]))
    # unpacked separator, pool floor (64 x 8 pairs): entangle on N = 89 | 90, off N = 492 | 493 (S = 0)
    for ent, lo, hi in ((1, 89, 90), (0, 492, 493)):
        a, b = one(doc, "sep", n_hull=lo, N=lo, S=0, ent=ent), one(doc, "sep", n_hull=hi, N=hi, S=0, ent=ent)
        assert a["bytes"] == 10240 and a["pool_pairs"] >= 512 and b["bytes"] > 10240 and b["pool_pairs"] == 512, (a, b)
    # safety resolve: W = 1 | 2 at N = 32 | 33, sBits in use from N = 257, past 64 KB at N = 682
    res = lambda N: one(doc, "resolve", N=N)["bytes"]
    assert res(32) == 4 * (64 + 33) and res(33) == 4 * (66 + 34 * 2) and res(256) == 4 * (512 + 257 * 8) and res(257) == 4 * (514 + 258 * 9)
    assert res(681) <= 65536 < res(682)
    # entangle re-check: one 64-bit mask more at N, S = 64 | 65
    ec = lambda N, S: one(doc, "ent_check", N=N, S=S)["bytes"]
    assert ec(65, 64) - ec(64, 64) == 8 and ec(64, 65) - ec(64, 64) == 8 and ec(65, 65) - ec(64, 64) == 16
    # audit: S = 0 and S > 0 with N odd; mission: no keep-out polygon and NEP_MISSION_MAX_POLY
    assert one(doc, "audit", N=5, S=0, vstride=1)["bytes"] == 5 * 36 and one(doc, "audit", N=5, S=3, vstride=16)["bytes"] == 5 * 36 + 3 * 16 * 24 + 12
    assert one(doc, "mission", N=8, n_vert=0, n_poly=0)["bytes"] == 8 * 52 + 4 and one(doc, "mission", N=8, n_vert=512, n_poly=64)["bytes"] == 8 * 52 + 8192 + 260
    assert one(doc, "mission", N=1097, n_vert=512, n_poly=64)["bytes"] <= 65536 < one(doc, "mission", N=1098, n_vert=512, n_poly=64)["bytes"]
