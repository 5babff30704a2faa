"""CPU: the hull kernel's chain walk and its skip rule (neptune_amd/csrc/hull_chain.h) on the host.  tests/cpp/hull_chain_check.cpp — its
own main, the header, the basis table — makes interval hulls the way hull_group_kernel does (1-4 segments: random cubics, constants with
their control points within ulps of each other, straight and axis-aligned lines; positions at +-50 m, rounded to integers, below 1e-3,
and |x| < 1e-9 beside y ~ 45; radii 0.05-0.3, one hull in twenty without inflation) and walks both chains over every point and over
the rule's to-do masks.  Built plain and with -fsanitize=address,undefined.

 - 450 000 hulls: the masked walk's final stacks are the plain walk's, all of them.
 - The rule without its gap condition differs on the same input: the fuzz reaches the hazard the gap is there for.
 - 3 000 of the hulls, as the masked walk leaves them, against the oracle's hull_of_interval: counts and vertices byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from neptune_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FUZZ = 450000
N_ORACLE = 3000


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hull_chain") / ("hull_chain_check_" + request.param))
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                       [os.path.join(ROOT, "tests", "cpp", "hull_chain_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _counts(stdout):
    lines = stdout.splitlines()
    assert lines[-1] == "hull_chain_check ok", lines[-3:]
    return {k: int(v) for k, v in (kv.split("=") for kv in lines[-2].split())}


def test_masked_walk_leaves_the_plain_walks_stacks(exe):
    r = subprocess.run([exe, "fuzz", str(N_FUZZ), "20261"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    c = _counts(r.stdout)
    print(c)
    assert c["hulls"] == N_FUZZ >= 400000
    assert c["mismatches"] == 0, c
    # the input reaches the cluster hazard (two points of a run within ulps against a far entry under them), ...
    assert c["mismatches_without_gap"] > 0, c
    # ... every shape of input is there, and the rule does skip: close to half of all visits at these shapes
    assert c["uninflated"] > N_FUZZ // 40 and c["under_4_points"] > 0 and c["full_64"] > N_FUZZ // 40, c
    assert c["skipping_off"] == 0, c
    assert c["visits_masked"] < 0.55 * c["visits_plain"], c


def test_magnitudes_where_the_rule_gives_way(exe):
    """coordinates of 1e9, on either side of 1e150 (products could overflow: no skipping), around 1e-150 (the floors of the gap and of
    the difference of consecutive x) and subnormal: the rule switches itself off for some hulls, skips in others, never a mismatch"""
    r = subprocess.run([exe, "edge", "100000", "20263"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    c = _counts(r.stdout)
    print(c)
    assert c["mismatches"] == 0, c
    assert 0 < c["skipping_off"] < c["hulls"] and c["visits_masked"] < 0.9 * c["visits_plain"], c


def test_masked_walks_hulls_are_the_oracles(exe, oracle):
    r = subprocess.run([exe, "dump", str(N_ORACLE), "20262"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    c = _counts(r.stdout)
    assert c["mismatches"] == 0, c
    rows = r.stdout.splitlines()[:-2]
    assert len(rows) == N_ORACLE
    V = abi.NEP_HULL_MAX_V
    most, cut = 0, 0
    for row in rows:
        head, knots, cx, cy, k, verts = [[float.fromhex(t) if "x" in t or "inf" in t or "nan" in t else int(t) for t in part.split()] for part in row.split("|")]
        n = head[0]
        pw = abi.nep_pwp()
        pw.n_seg = n
        for s in range(n + 1):
            pw.times[s] = knots[s]
        for ax, co in enumerate((cx, cy)):
            for s in range(n):
                for j in range(4):
                    pw.coeff[ax][s][j] = co[4 * s + j]
        h, _h0, ov = oracle.hull_of_interval(pw, 0.0, 0.5, 0.5, np.array([head[1], head[2]]), with_overflow=True)
        k = k[0]
        assert ov == (k > V), (row, k)
        assert len(h) == min(k, V), (row, len(h), k)
        assert h.tobytes() == np.array(verts, dtype=np.float64).tobytes(), row
        most = max(most, k); cut += k > V
    assert most >= 8
