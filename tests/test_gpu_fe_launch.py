"""GPU: the table of front-end cases of scripts/fe_launch_paths.py through the library — every entry point, launch orders with and
without an active set, scene counts on both sides of the thresholds of the launch sequence, two consecutive calls per case (without
and with the searches' history) — against the digests of d_guess, d_result and d_case_out recorded at the commit before the front
end's launch plan existed (tests/golden/fe_launch_paths.json).  Largest case: 257 x 8 searches.  The digests show that every
path computes what it computed; they do not show which launch order a call took (an order changes no output: that is what the traced
run of the script records)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    spec = importlib.util.spec_from_file_location("fe_launch_paths", os.path.join(ROOT, "scripts", "fe_launch_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "tests", "golden", "fe_launch_paths.json")) as f:
        want = json.load(f)
    return mod, want, mod.run_table()


def test_every_case_of_the_fixture_was_run(table):
    mod, want, rows = table
    key = lambda c: (c["name"], c["agents"], c["scenes"])
    assert [key(c) for c in rows] == [key(c) for c in want["cases"]] == [(n, a, s) for n, a, s, _ in mod.cases()]
    assert max(c["slots"] for c in rows) == 257 * 8


def test_outputs_are_the_recorded_ones(table):
    """both calls of every case: the second runs in the launch order the first one's search times give, over the active list where
    there is one"""
    _, want, rows = table
    bad = [(c["name"], c["agents"], c["scenes"], r) for c, w in zip(rows, want["cases"]) for r in range(2) if c["calls"][r]["sha"] != w["calls"][r]["sha"]]
    assert not bad, bad
