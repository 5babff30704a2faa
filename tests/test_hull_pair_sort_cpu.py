"""CPU: the hull kernel's sort of an inflated hull's corners as stacked pairs (neptune_amd/csrc/hull_pair_sort.h) on the host.
tests/cpp/hull_pair_sort_check.cpp — its own main, the header, the basis table — makes interval hulls the way hull_group_kernel does
and stores every hull's sorted array as the kernel would: the header's network over the pairs, stored run by run, where the rule
allows it, the corners' lexicographic sort where it does not.  Built plain and with -fsanitize=address,undefined.

 - The stored array equals std::sort of the corners element for element, as bits, in every hull of every family.
 - Expanding every pair where it stands (no runs), and storing the hulls the rule refuses all the same, both differ on the same
   input: the hazards are reached.
 - How many hulls of each family took the pair path is printed, and bounded where the family is made to take it or to refuse it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PER_FAMILY = 40000
FAMILIES = ("cubics", "constants", "lines", "mixed", "big", "tiny", "same_x", "dup", "zeros", "collapse", "neg_dy")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def counts(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hull_pair_sort") / ("hull_pair_sort_check_" + request.param))
    flags = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                       [os.path.join(ROOT, "tests", "cpp", "hull_pair_sort_check.cpp"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([out, str(N_PER_FAMILY), "20271"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "hull_pair_sort_check ok", lines[-3:]
    c = {}
    for line in lines[:-1]:
        kv = dict(t.split("=") for t in line.split())
        family = kv.pop("family")
        c[family] = {k: int(v) for k, v in kv.items()}
    print(r.stdout)
    return c


def test_stored_array_is_the_lexicographic_sort(counts):
    assert set(counts) == set(FAMILIES) | {"all"}
    for f in FAMILIES:
        c = counts[f]
        assert c["hulls"] == N_PER_FAMILY == c["fast"] + c["refused"] + c["run_refused"], (f, c)
        assert c["mismatches"] == 0, (f, c)
    assert counts["all"]["hulls"] == N_PER_FAMILY * len(FAMILIES) >= 400000


def test_the_runs_and_the_rule_are_needed(counts):
    for f in FAMILIES:
        c = counts[f]
        # every hull with a run of two or more is wrong when its pairs are expanded where they stand
        assert c["mismatches_without_runs"] == c["fast_with_runs"], (f, c)
    # the families made to have equal keys have them, every time
    for f in ("constants", "same_x", "dup"):
        assert counts[f]["fast_with_runs"] == counts[f]["fast"] > 0.6 * N_PER_FAMILY, (f, counts[f])
    for f in ("collapse", "lines", "mixed", "tiny"):
        assert counts[f]["fast_with_runs"] > 0.3 * N_PER_FAMILY, (f, counts[f])
    # what the rule refuses would be wrong: runs whose y span more than 2 dy, keys of zero, a negative dy
    for f in ("same_x", "collapse"):
        assert counts[f]["run_refused"] > 0.2 * N_PER_FAMILY and counts[f]["mismatches_without_rule"] == counts[f]["run_refused"], (f, counts[f])
    for f in ("zeros", "neg_dy"):
        assert counts[f]["refused"] == N_PER_FAMILY == counts[f]["mismatches_without_rule"], (f, counts[f])


def test_which_families_take_the_pair_path(counts):
    # generic trajectories always do, without a run; records at rest nearly always, with runs; magnitudes from 1e150 on never
    assert counts["cubics"]["fast"] == N_PER_FAMILY and counts["cubics"]["fast_with_runs"] == 0
    assert counts["constants"]["fast"] > 0.99 * N_PER_FAMILY and counts["dup"]["fast"] > 0.99 * N_PER_FAMILY
    assert 0 < counts["big"]["refused"] < N_PER_FAMILY and counts["big"]["fast"] > 0
    for f in ("lines", "mixed", "tiny"):
        assert counts[f]["fast"] > 0.9 * N_PER_FAMILY, (f, counts[f])
