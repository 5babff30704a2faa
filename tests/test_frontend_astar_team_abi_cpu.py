"""The four-waves-per-search switch of the best-first search with the entangle check, without a GPU: the library exports the setter
and the reader, _lib.py declares their signatures as include/neptune_frontend.h states them, the header says what the switch concerns,
and the loops refuse a team they cannot fly."""
import ctypes as C
import inspect
import os
import re

import pytest

from neptune_amd import _lib, backend, loop, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_two_calls_with_the_headers_signatures():
    L = _lib.lib()
    vp, i = C.c_void_p, C.c_int32
    assert {"nep_batch_set_fe_astar_team", "nep_batch_fe_astar_team"} <= set(_lib.FE_EXPORTS)
    assert L.nep_batch_set_fe_astar_team.argtypes == [vp, i]
    assert L.nep_batch_fe_astar_team.argtypes == [vp]
    with open(os.path.join(ROOT, "include", "neptune_frontend.h")) as f:
        hdr = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", f.read()))      # (a comment's lines joined)
    assert "int nep_batch_set_fe_astar_team(nep_batch_t* h, int32_t waves);" in hdr
    assert "int nep_batch_fe_astar_team(nep_batch_t* h);" in hdr
    # what the header must say: the scope, the captured graphs, the shared storage
    assert "nep_batch_frontend_astar (check off) keeps its one wave whatever the setting" in hdr
    assert "a captured graph keeps the form it was captured with" in hdr
    assert "calls with waves 1 and 4 may alternate on one handle" in hdr


def test_null_handle_is_an_argument_error():
    L = _lib.lib()
    assert L.nep_batch_set_fe_astar_team(None, 4) == -1            # NEP_E_ARG (no HIP call is made for it)
    assert L.nep_batch_fe_astar_team(None) == -1


def test_python_mirror():
    assert list(inspect.signature(backend.BatchBackend.set_fe_astar_team).parameters) == ["self", "waves"]
    assert list(inspect.signature(backend.BatchBackend.fe_astar_team).parameters) == ["self"]
    for cls in (loop.FleetLoop, loop.DeviceFleetLoop):
        assert inspect.signature(cls.__init__).parameters["team"].default == 1
    assert "team" not in loop.DeviceFleetLoop._MUST_MATCH           # a launch choice: not among the options a checkpoint carries


def test_loops_refuse_a_team_they_cannot_fly():
    assert loop.check_team(1, "beam") == 1 and loop.check_team(1, "astar") == 1 and loop.check_team(4, "astar_ent") == 4
    for team, search in ((4, "beam"), (4, "astar"), (3, "astar_ent"), (0, "astar_ent"), (2, "astar_ent"), ("4", "astar_ent"), (True, "astar_ent"), (4.0, "astar_ent")):
        with pytest.raises(ValueError):
            loop.check_team(team, search)
    sc = scene.make_scene(5, 3, seed=0)
    # (the loops check before they touch the GPU)
    with pytest.raises(ValueError):
        loop.DeviceFleetLoop([sc], search="astar", team=4)
    with pytest.raises(ValueError):
        loop.DeviceFleetLoop([sc], tethers=True, search="astar_ent", team=3)
    with pytest.raises(ValueError):
        loop.FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), search="beam", team=4)
    with pytest.raises(ValueError):
        loop.FleetLoop(sc["par"], sc["statics"], sc["starts"], scene.reachable_goals(sc), tethers=True, search="astar_ent", team=3)
