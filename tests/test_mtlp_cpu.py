"""CPU: the MTLP comparator (include/neptune_mtlp.h) — the host form against the Python restatement of the reference
(tests/mtlp_ref.py) on the directed worlds and the seeded family of tests/mtlp_worlds.py, byte for byte; the order graph's rule set
on seeded pairs that sit on every branch of its else-if chains; the exact predicates against Fractions on near-degenerate inputs;
the header, the exports, the ABI; and a stand-alone sanitizer build of the host code (tests/cpp/mtlp_host_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mtlp_ref as ref
import mtlp_worlds as W
from neptune_amd import _lib, abi, mtlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.mark.parametrize("case", W.directed(), ids=lambda c: c["name"])
def test_directed_event_happens(case):
    """on the Python restatement alone: the rule the world was built for is exercised"""
    assert case["event"](W.reference(case))


def test_family_is_not_vacuous():
    """On the Python restatement alone (seed W.FAMILY_SEED): of the family's 47 searches 27 reach their goal, 12 end on the budget,
    8 with an empty list, 13 take an in-place update."""
    counts = W.family_counts()
    print(counts)
    assert counts["searches"] >= 40 and 2 * counts["reached"] >= counts["searches"]
    assert counts["budget"] >= 1 and counts["empty"] >= 1 and counts["updates"] >= 1
    assert {c["cfg"]["resolution"] for c in W.family()} == {0.2, 0.25} and {c["cfg"]["n_robots"] for c in W.family()} == {2, 3, 4}


def test_worlds_are_small():
    for c in W.all_cases():
        f = c["cfg"]
        cells = [int((f[a + "_max"] - f[a + "_min"]) / f["resolution"]) for a in "xyz"]
        assert cells[0] <= 16 and cells[1] <= 16 and cells[2] <= 4 and f["n_robots"] <= 4 and f["max_nodes"] <= 512 and f["max_pops"] <= 300, c["name"]


@pytest.mark.parametrize("cases", [W.directed(), W.family()], ids=["directed", "family"])
def test_host_equals_reference(cases):
    for cfgd, g in W.groups(cases):
        m = W.make_handle(cfgd)
        got = m.solve(*W.pack(g), device=False)
        diff = W.same_bytes(got, W.expected(cfgd, g))
        assert diff is None, ([c["name"] for c in g], diff)
        m.close()


def graph_pairs():
    """200 pairs (seed 7): random triangles over a 1/4 lattice (so that touching and coplanar pairs occur), and pairs made from
    two templates — crossing baselines at chosen heights, and parallel baselines with anchors through the other's triangle — that
    reach the branches random pairs seldom do"""
    rng = np.random.default_rng(7)
    pairs = []
    lat = lambda hi: float(rng.integers(0, 4 * hi + 1)) / 4.0      # noqa: E731
    for _ in range(120):
        pairs.append(([(lat(4), lat(4), 0.0) for _ in range(2)], [((lat(4), lat(4), lat(1)), (lat(4), lat(4), lat(1))) for _ in range(2)]))
    for _ in range(40):      # baselines cross at (2, 2); the heights decide which anchor pierces which triangle
        za, zb = lat(1), lat(1)
        pairs.append(([(0.5, 2.0, 0.0), (2.0, 0.5, 0.0)], [((lat(1) + 0.5, 2.0, za), (lat(1) + 2.5, 2.0, za)), ((2.0, lat(1) + 0.5, zb), (2.0, lat(1) + 2.5, zb))]))
    for _ in range(40):      # baselines apart (parallel in xy), bases on the far side of each other's baseline
        ya, yb = 1.0 + lat(1), 1.0 + lat(1)
        pairs.append(([(lat(4), 3.5, 0.0), (lat(4), 0.25, 0.0)], [((lat(2), ya, lat(1)), (2.0 + lat(2), ya, lat(1))), ((lat(2), yb + 0.25, lat(1)), (2.0 + lat(2), yb + 0.25, lat(1)))]))
    return pairs


def test_graph_rule_set_on_seeded_pairs():
    pairs = graph_pairs()
    assert len(pairs) == 200
    m = W.make_handle(W.cfg(max_pops=1, max_nodes=4))
    got = m.solve(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]), device=False)
    seen = set()
    for k, (bases, sg) in enumerate(pairs):
        g, branches = ref.order_graph(bases, sg)
        seen.update(branches.values())
        assert (got["graph"][k] == g).all(), (k, bases, sg, g, got["graph"][k])
    print(sorted(seen))
    # every branch of both else-if chains, and the fall-through of each
    assert seen >= {"apart", "type1", "type2", "type3_a_first", "type3_b_first", "no_type", "cross_end_a", "cross_end_b", "cross_start_a", "cross_start_b"}, sorted(seen)
    m.close()


def test_predicates_against_fractions(L):
    """The filter: a sign is taken from the double evaluation when it exceeds 2^-49 times the sum of the absolute monomials (at most
    8 roundings lie on any path: ((1 + e)^8 - 1) / (1 - e)^8 < 9 e < 16 e = 2^-49, e = 2^-53); otherwise from the integer path.  The
    inputs are fixed in tests/mtlp_worlds.py (queries exactly on the primitive, one coordinate moved by 0, +-1, +-2 ulp), so how
    many take the exact path depends on the filter alone."""
    which, rec = W.predicate_records()
    assert len(rec) == 10000
    n_exact = 0
    seen = set()
    for w in (0, 1, 2):
        idx = np.nonzero(which == w)[0]
        v, e = mtlp.predicates(w, rec[idx], device=False)
        n_exact += int((e > 0).sum())
        for k, i in enumerate(idx):
            want = W.predicate_truth(w, rec[i])
            seen.add((w, want))
            assert v[k] == want, (w, list(rec[i]), v[k], want)
    print(n_exact, sorted(seen))
    assert 4 * n_exact >= len(rec), n_exact
    assert seen >= {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)}


def test_malformed_runs_and_arguments(L):
    c = W.directed()[0]
    m = W.make_handle(c["cfg"])
    b, s = W.pack([c, c, c])
    b[1, 0, 0] = np.nan; s[2, 1, 1, 2] = 2.0 ** -62
    out = m.solve(b, s, device=False)
    assert list(out["run_status"]) == [1, -2, -2] and not out["graph"][1:].any() and not out["path"][1:].any()
    assert (out["result"]["flags"][1:] == abi.NEP_MTLP_FLAG_STATE).all() and (out["result"]["status"][1:] == -1).all() and (out["result"]["pops"][1:] == 0).all()
    assert ref.solve(c["cfg"], b[1], s[1])["run_status"] == -2 and ref.solve(c["cfg"], b[2], s[2])["results"][0]["flags"] == ref.FLAG_STATE
    with pytest.raises(_lib.BackendError):
        m.check(stream=0)
    assert m.check(stream=0) == 0      # cleared by the check
    d = [x for x in W.directed() if x["name"] == "collinear_triangle"][0]
    md = W.make_handle(d["cfg"])
    assert md.solve(*W.pack([d]), device=False)["result"]["flags"][0, 0] == abi.NEP_MTLP_FLAG_DEGEN and md.check(stream=0) == 0      # DEGEN is no error
    assert m.search_bytes() > 32 * c["cfg"]["max_nodes"]
    for bad in (dict(max_pops=0), dict(max_pops=-1), dict(resolution=0.0), dict(z_max=0.0), dict(n_robots=65), dict(radius=2.0 ** -70), dict(x_min=-2e5), dict(bias=0.0)):
        assert not L.nep_mtlp_create(C.byref(mtlp.make_cfg(**dict(c["cfg"], **bad)))) and L.nep_last_error(), bad
    m.close(); md.close()


def test_circle_bases():
    """mtlp_node.cpp:295-313 in float32, as the reference's cosf / sinf give them up to the last place of a float"""
    for n in (1, 5, 8):
        got = mtlp.circle_bases(n)
        theta = 3.1415927 * 2 / n * np.arange(n)
        x = -10 * np.cos(theta.astype(np.float32)).astype(np.float64) - 2.5 * np.cos((1.571 - theta).astype(np.float32)).astype(np.float64)
        y = -10 * np.sin(theta.astype(np.float32)).astype(np.float64) + 2.5 * np.sin((1.571 - theta).astype(np.float32)).astype(np.float64)
        assert np.abs(got[:, 0] - x).max() < 1e-5 and np.abs(got[:, 1] - y).max() < 1e-5 and not got[:, 2].any()


def test_header_is_c99_and_exports_match(L, tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "neptune_mtlp.h"\nint main(void) { nep_mtlp_cfg c; nep_mtlp_result r; (void)c; (void)r; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c99.o")])
    src.write_text('#include "neptune_mtlp.h"\n#include "neptune_backend.h"\n#include "neptune_hastar.h"\n#include "neptune_mtlp.h"\nint main(void) { return NEP_E_CAP == -4 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c99b.o")])
    hdr = open(os.path.join(ROOT, "include", "neptune_mtlp.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|void|nep_mtlp_t\*)\s+(nep_mtlp_[a-z_0-9]+)\(", hdr, re.M))
    assert declared == set(_lib.MTLP_EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    for name in ("NEP_MTLP_FLAG_PATH", "NEP_MTLP_FLAG_STATE", "NEP_MTLP_FLAG_DEGEN", "NEP_MTLP_MAX_ROBOTS"):
        assert int(re.search(r"#define %s (\d+)\b" % name, hdr).group(1)) == getattr(abi, name), name
    assert "0 .. N-1" in hdr and "multiple of 2^-60" in hdr      # the order of the robots and the domain are stated


def test_mtlp_abi(L):
    assert L.nep_abi_sizeof(35) == C.sizeof(abi.nep_mtlp_cfg) == 88
    assert L.nep_abi_sizeof(36) == C.sizeof(abi.nep_mtlp_result) == abi.MTLP_RESULT_DTYPE.itemsize == 48
    assert L.nep_abi_sizeof(34) == -1


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/mtlp_host_check.cpp: capacities, malformed inputs and the exact arithmetic at the domain's edges, as a stand-alone
    executable built from mtlp_host.cpp alone"""
    exe = str(tmp_path / "mtlp_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "mtlp_host_check.cpp"),
                           os.path.join(ROOT, "neptune_amd", "csrc", "mtlp_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mtlp_host_check ok" in out.stdout
