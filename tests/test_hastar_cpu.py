"""CPU: the homotopic grid A* of the single-agent benchmark (include/neptune_hastar.h) — the host form against the Python
restatement of the reference (tests/hastar_ref.py) on the directed worlds and the seeded family of tests/hastar_worlds.py, byte for
byte; its two-set GJK against oracle.gjk_collision; properties of what it returns; the header, the exports, the ABI; and a
stand-alone sanitizer build of the host code (tests/cpp/hastar_host_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hastar_ref as ref
import hastar_worlds as W
from neptune_amd import _lib, abi, hastar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def host_results():
    """every case through the host form, once: name -> (result, path, state) rows"""
    out = {}
    for cfgd, g in W.groups(W.all_cases()):
        ha = W.make_handle(cfgd, [c["world"] for c in g])
        start, goal, st = W.pack_inputs(ha, g)
        res, path, state = ha.search(np.arange(len(g)), start, goal, state=st, device=False)
        for k, c in enumerate(g):
            out[c["name"]] = (res[k], path[k], state[k])
        ha.close()
    return out


@pytest.mark.parametrize("case", W.directed(), ids=lambda c: c["name"])
def test_directed_event_happens(case):
    """on the Python reference alone: the rule the world was built for is exercised"""
    assert case["event"](W.reference(case)), W.reference(case)


def test_family_covers_every_event():
    """On the Python reference alone.  Counts over the 48 searches of the family (seed 20261020): reached 28, open_list_empty 17,
    budget 3, signature 19, cancelled 1, inplace_update 22, cable_lives 13, cable_prunes 5, node_pool 3, power_int_wraps 4,
    cap_hsig 1, cap_cont 3, cap_path 3, cap_pool 3, same_cell 3, goal_in_polygon 3, shortened_terminal 14."""
    assert len(W.family()) >= 48
    counts = W.family_counts()
    print(counts)
    assert all(v > 0 for v in counts.values()), counts
    sizes = {(c["cfg"]["x_max"], len(c["world"]["uninflated"])) for c in W.family()}
    assert {s[0] for s in sizes} == {6.0, 6.5, 7.0, 7.5, 8.0} and {s[1] for s in sizes} == {1, 2, 3}


@pytest.mark.parametrize("cases", [W.directed(), W.family()], ids=["directed", "family"])
def test_host_equals_reference(cases):
    for cfgd, g in W.groups(cases):
        ha = W.make_handle(cfgd, [c["world"] for c in g])
        start, goal, st = W.pack_inputs(ha, g)
        got = ha.search(np.arange(len(g)), start, goal, state=st, device=False)
        diff = W.same_bytes(got, W.expected(ha, g))
        assert diff is None, ([c["name"] for c in g], diff)
        ha.close()


def test_gjk_two_sets_equals_oracle(L, oracle):
    import safety_cases as SC
    polys, quads, _, _ = SC.gjk_grid_cases()
    n_hit = 0
    for A, B in zip(polys, quads):
        A = np.ascontiguousarray(A, dtype=np.float64).reshape(-1, 2); B = np.ascontiguousarray(B, dtype=np.float64).reshape(-1, 2)
        want = oracle.gjk_collision(A, B)
        n_hit += want
        assert bool(L.nep_hastar_gjk(len(A), abi.dptr(A), len(B), abi.dptr(B))) == want
    assert 0 < n_hit < len(polys)
    # segments against rectangles: crossing, apart, touching a corner, lying on an edge, ending on an edge, degenerate (a point)
    rect = np.array([[1.0, 1.0], [3.0, 1.0], [3.0, 2.0], [1.0, 2.0]])
    rng = np.random.default_rng(5)
    segs = [[(0, 0), (4, 3)], [(0, 0), (0.5, 3)], [(0, 0), (1, 1)], [(0, 3), (1, 2)], [(1, 0.5), (1, 2.5)], [(0, 2), (4, 2)], [(2, 1.5), (2, 1.5)],
            [(0, 1.5), (1, 1.5)], [(5, 5), (5, 5)], [(3, 2), (3, 2)], [(2, 0), (2, 1)], [(1.5, 1.25), (2.5, 1.75)]]
    segs += [[tuple(rng.integers(0, 33, 2) / 8.0), tuple(rng.integers(0, 33, 2) / 8.0)] for _ in range(400)]
    seen = set()
    for seg in segs:
        S = np.array(seg, dtype=np.float64)
        for P in (rect, rect[::-1].copy(), rect[:1].copy(), rect[:2].copy()):
            want = oracle.gjk_collision(P, S)
            seen.add(want)
            assert bool(L.nep_hastar_gjk(len(P), abi.dptr(P), 2, abi.dptr(S))) == want, (P, seg)
    assert seen == {True, False}
    assert L.nep_hastar_gjk(0, abi.dptr(rect), 2, abi.dptr(rect)) == -1


def _replay_signature(case, path, n_path):
    hsig = list(case["hsig0"])
    for k in range(n_path - 1):
        ref.update_hsig(hsig, tuple(path[k]), tuple(path[k + 1]), case["world"]["reps"])
    return hsig


def test_properties_of_returned_paths(host_results):
    n_replayed = n_checked_cable = 0
    for c in W.all_cases():
        res, path, state = host_results[c["name"]]
        if res["status"] != 1:
            assert res["n_path"] == 0 and res["length_m"] == 0 and res["g_cells"] == 0 and not path.any()
            continue
        n = int(res["n_path"])
        cfgd = c["cfg"]
        assert tuple(path[0]) == c["start"] and not path[n:].any()
        idx = np.floor((path[:n] - [cfgd["x_min"], cfgd["y_min"]]) / cfgd["resolution"]).astype(int)
        step = np.abs(np.diff(idx, axis=0))
        assert (step.max(axis=1) == 1).all() if n > 1 else True, "8-connected"
        for k in range(1, n):      # no occupied cell after the start
            ctr = (idx[k] + 0.5) * cfgd["resolution"] + [cfgd["x_min"], cfgd["y_min"]]
            assert tuple(ctr) == tuple(path[k])
            box = [(ctr[0] + 0.05, ctr[1] + 0.05), (ctr[0] + 0.05, ctr[1] - 0.05), (ctr[0] - 0.05, ctr[1] + 0.05), (ctr[0] - 0.05, ctr[1] - 0.05)]
            assert not any(ref.gjk(q, box) for q in c["world"]["inflated"])
        if not res["flags"] & abi.NEP_HASTAR_FLAG_PATH:
            # replay: the path pushed through updateHSig_orig from the initial state gives the terminal signature
            want = _replay_signature(c, path, n)
            got = [(int(state["hsig_id"][e]), int(state["hsig_sign"][e])) for e in range(int(state["n_hsig"]))]
            assert got == want, c["name"]
            n_replayed += 1
            assert res["g_cells"] == sum(W.DIAG if step[k].sum() == 2 else 1.0 for k in range(n - 1))
        if res["n_length_checks"] > 0 and int(state["n_cont"]) < n:      # the terminal list went through updateContPts_orig
            pts = [tuple(p) for p in state["cont"][:int(state["n_cont"])]]
            assert ref.tether_length(pts) <= cfgd["cable_length"], c["name"]
            n_checked_cable += 1
        assert not state["cont"][int(state["n_cont"]):].any() and not state["hsig_id"][int(state["n_hsig"]):].any() and not state["hsig_sign"][int(state["n_hsig"]):].any()
    assert n_replayed > 20 and n_checked_cable > 5


def test_chaining_through_the_state_equals_the_reference():
    """neptune_ros.cpp:1667-1670: the terminal state and goal of one search are the initial state and start of the next"""
    chained = 0
    for c in [W.directed()[3], W.directed()[7]] + W.family()[:16]:
        r1 = W.reference(c)
        if r1["status"] != 1:
            continue
        goal2 = (c["start"][0] + 0.1, c["start"][1] - 0.05)      # and back
        start2 = r1["path"][-1]
        r2 = ref.search(c["cfg"], c["world"], start2, goal2, r1["hsig"], r1["cont"])
        ha = W.make_handle(c["cfg"], [c["world"]])
        s, g, st = W.pack_inputs(ha, [c])
        res1, path1, st1 = ha.search(0, s, g, state=st, device=False)
        n1 = int(res1["n_path"][0])
        got = ha.search(0, path1[:, n1 - 1], np.array([goal2]), state=st1, device=False)
        c2 = dict(c, start=start2, goal=goal2, hsig0=r1["hsig"], cont0=r1["cont"])
        diff = W.same_bytes(got, W.expected(ha, [c2], [r2]))
        assert diff is None, (c["name"], diff)
        chained += 1
        ha.close()
    assert chained >= 8


def test_malformed_slots_and_arguments(L):
    c = W.directed()[0]
    ha = W.make_handle(c["cfg"], [c["world"]])
    s, g, st = W.pack_inputs(ha, [c, c, c])
    st["n_cont"][1] = 0
    st["n_hsig"][2] = c["cfg"]["hsig_cap"] + 1
    res, path, out = ha.search(np.array([0, 0, 0]), s, g, state=st, device=False)
    assert res["status"][0] == 1 and res["flags"][0] == 0
    for k in (1, 2):
        assert res["status"][k] == -1 and res["flags"][k] == abi.NEP_HASTAR_FLAG_STATE and res["pops"][k] == 0 and out["n_cont"][k] == 0 and not path[k].any()
    res, _, _ = ha.search(np.array([0, 1, -1]), s, g, state=W.pack_inputs(ha, [c, c, c])[2], device=False)
    assert list(res["flags"]) == [0, abi.NEP_HASTAR_FLAG_STATE, abi.NEP_HASTAR_FLAG_STATE]
    s_bad = s.copy(); s_bad[1, 0] = np.nan; s_bad[2, 1] = 2e5      # a point updateContPts_orig could not sample in finite time
    res, _, _ = ha.search(np.array([0, 0, 0]), s_bad, g, state=W.pack_inputs(ha, [c, c, c])[2], device=False)
    assert list(res["flags"]) == [0, abi.NEP_HASTAR_FLAG_STATE, abi.NEP_HASTAR_FLAG_STATE]
    r = ref.search(c["cfg"], c["world"], (float("nan"), 1.0), c["goal"], [], [c["start"]])
    assert r["flags"] == ref.FLAG_STATE and r["status"] == -1
    with pytest.raises(_lib.BackendError):
        ha.check(stream=0)
    assert ha.check(stream=0) == 0      # cleared by the check
    assert ha.search_bytes() > 0
    bad = hastar.make_cfg(**dict(c["cfg"], resolution=0.0))
    assert not L.nep_hastar_create(C.byref(bad), 1) and L.nep_last_error()
    bad = hastar.make_cfg(**dict(c["cfg"], z_max=0.0))      # GLZ = 0: the reference's pool would be empty
    assert not L.nep_hastar_create(C.byref(bad), 1)
    reps = np.zeros((abi.NEP_HASTAR_MAX_REP + 1, 2, 2))
    assert L.nep_hastar_set_reps(ha.h, 0, len(reps), abi.dptr(reps)) == -4
    assert L.nep_hastar_set_reps(ha.h, 1, 0, None) == -1
    ha.close()


def test_inflate_is_two_drone_radii():
    q = W.square(2.0, 3.0)
    got = hastar.inflate(q, W.RADIUS)
    assert [tuple(p) for p in got] == W.inflate(q)
    tri = hastar.inflate([(0, 0), (1, 0), (0, 1)], 0.25)
    assert len(tri) == 5 and tuple(tri[0]) == (-0.5, -0.5)


def test_header_is_c99_and_exports_match(L, tmp_path):
    hdr_path = os.path.join(ROOT, "include", "neptune_hastar.h")
    src = tmp_path / "c99.c"
    src.write_text('#include "neptune_hastar.h"\nint main(void) { nep_hastar_cfg c; nep_hastar_result r; nep_hastar_state s; (void)c; (void)r; (void)s; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c99.o")])
    # ... and next to the other headers, in either order
    src.write_text('#include "neptune_hastar.h"\n#include "neptune_backend.h"\n#include "neptune_hastar.h"\nint main(void) { return NEP_E_CAP == -4 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "c99b.o")])
    hdr = open(hdr_path).read()
    declared = set(re.findall(r"^(?:int|int64_t|void|nep_hastar_t\*)\s+(nep_hastar_[a-z_0-9]+)\(", hdr, re.M))
    assert declared == set(_lib.HASTAR_EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    for name in ("NEP_HASTAR_FLAG_HSIG", "NEP_HASTAR_FLAG_CONT", "NEP_HASTAR_FLAG_PATH", "NEP_HASTAR_FLAG_POOL", "NEP_HASTAR_FLAG_STATE", "NEP_HASTAR_MAX_REP",
                 "NEP_HASTAR_POOL_PER_NODE"):
        assert int(re.search(r"#define %s (\d+)\b" % name, hdr).group(1)) == getattr(abi, name), name


def test_hastar_abi(L):
    assert L.nep_abi_sizeof(31) == C.sizeof(abi.nep_hastar_cfg) == 96
    assert L.nep_abi_sizeof(32) == C.sizeof(abi.nep_hastar_result) == abi.HASTAR_RESULT_DTYPE.itemsize == 48
    assert L.nep_abi_sizeof(33) == C.sizeof(abi.nep_hastar_state) == 48


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/hastar_host_check.cpp: the cap and pool cases as a stand-alone executable built from hastar_host.cpp alone"""
    exe = str(tmp_path / "hastar_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "hastar_host_check.cpp"),
                           os.path.join(ROOT, "neptune_amd", "csrc", "hastar_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hastar_host_check ok" in out.stdout
