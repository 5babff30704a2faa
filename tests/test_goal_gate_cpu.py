"""The move_when_goal_occupied gate without a GPU: the Python reference (tests/goal_gate_ref.py) on the oracle's searches and hulls
gives the outcomes DESIGN section 33 states, the C entry point refuses a null handle before it touches a device, the constants of the
header and of abi.py agree, and both loops refuse the option where it cannot fly."""
import math
import os
import re

import numpy as np
import pytest

import goal_gate_ref as ref
from neptune_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


@pytest.mark.parametrize("name", list(ref.CASES))
def test_reference_outcomes(oracle, name):
    """the table: who is let through (and by whom the goal is taken), who is turned down, who is not the gate's business"""
    sc, fe, pops, r, out = ref.case(oracle, name)      # (asserts the sets)
    p = sc["par"]
    if name == "r0.6_p300":
        assert p.drone_radius == 0.6
    for a, (v, occ, g, res, g0, res0) in out.items():
        assert (res0["status"] in (ref.DEPTH_REACHED, ref.EMPTY)) == (v != ref.UNTOUCHED)
        if v == ref.UNTOUCHED:
            assert res == res0 and g.tobytes() == g0.tobytes()
        elif v == ref.TAKEN:
            assert occ and a not in occ and g.tobytes() == g0.tobytes()
            assert {k for k in res if res[k] != res0[k]} == {"_pad"} and res["_pad"] == res0["_pad"] | 64
        else:
            assert not occ and res0["K"] >= 1      # a plan was there, and it was turned down
            assert (res["status"], res["K"], res["_pad"]) == (3, 0, res0["_pad"] | 32)
            assert {k for k in res if res[k] != res0[k]} == {"status", "K", "_pad"}
            assert int(g["K"]) == 0 and int(g["n_alpha"]) == 0 and not g["coeff"].any() and g["t_start"] == g0["t_start"]
            assert g.tobytes() == ref.gated_guess(g0).tobytes() and g0["coeff"].any()


def test_reference_box_and_self():
    """the box's column order, and an agent's own hull never occupies its goal"""
    assert ref.goal_box([1.0, 2.0, 9.0], 0.5).tolist() == [[1.5, 2.5], [1.5, 1.5], [0.5, 2.5], [0.5, 1.5]]

    class Always:
        @staticmethod
        def gjk_collision(a, b):
            return True
    hx = np.zeros((3, 2, 16, 2)); hn = np.array([[4, 4], [4, 0], [4, 4]], dtype=np.int32)
    assert ref.occupiers(Always, hx, hn, 0, [0.0, 0.0], 0.6) == [2]      # (0 is own, 1 has no last hull)
    assert ref.verdict(ref.GOAL_REACHED, [2]) == ref.verdict(ref.NO_SOLUTION, []) == ref.verdict(ref.SKIPPED, []) == ref.UNTOUCHED
    assert ref.verdict(ref.DEPTH_REACHED, [2]) == ref.verdict(ref.EMPTY, [1]) == ref.TAKEN
    assert ref.verdict(ref.DEPTH_REACHED, []) == ref.verdict(ref.EMPTY, []) == ref.GATED


def test_null_handle_is_an_argument_error(L):
    """before any HIP call: the same answer with and without a device"""
    assert L.nep_batch_goal_gate(None, 0.6, None, None, None, None, None, None) == -1      # NEP_E_ARG


def test_constants_and_prototype(L):
    assert (abi.NEP_FE_PAD_GATED, abi.NEP_FE_PAD_GOAL_TAKEN) == (32, 64) == (ref.PAD_GATED, ref.PAD_GOAL_TAKEN)
    hdr = open(os.path.join(ROOT, "include", "neptune_frontend.h")).read()
    assert int(re.search(r"#define NEP_FE_PAD_GATED\s+(\d+)\b", hdr).group(1)) == 32
    assert int(re.search(r"#define NEP_FE_PAD_GOAL_TAKEN\s+(\d+)\b", hdr).group(1)) == 64
    assert re.search(r"^int nep_batch_goal_gate\(nep_batch_t\* h, double half_side, const nep_fe_start\* d_start, nep_guess\* d_guess,", hdr, re.M)
    assert "nep_batch_goal_gate" in _lib.FE_EXPORTS and L.nep_batch_goal_gate
    assert abi.GOAL_GATE_COUNTS[:3] == ("examined", "goal_taken", "gated")
    assert (ref.DEPTH_REACHED, ref.GOAL_REACHED, ref.EMPTY, ref.NO_SOLUTION, ref.SKIPPED) == (0, 1, 2, 3, abi.NEP_FE_SKIPPED)


def test_loops_refuse_what_cannot_fly():
    """before anything touches a device: the beam, and half sides that are not positive and finite"""
    from neptune_amd import scene
    from neptune_amd.loop import DeviceFleetLoop, FleetLoop, check_goal_gate
    sc = scene.make_scene(5, 3, seed=0)
    p = sc["par"]
    bad = [dict(search="beam", goal_gate=True), dict(goal_gate=True), dict(search="beam", goal_gate=0.5)]
    bad += [dict(search="astar", goal_gate=r) for r in (0.0, -0.6, 0, math.nan, math.inf, -math.inf, "0.6")]
    for kw in bad:
        with pytest.raises(ValueError):
            DeviceFleetLoop([sc], **kw)
        with pytest.raises(ValueError):
            FleetLoop(p, sc["statics"], sc["starts"], sc["goals"], **kw)
    assert "goal_gate" in DeviceFleetLoop._MUST_MATCH
    assert check_goal_gate(False, "beam", 0.6) is None and check_goal_gate(None, "beam", 0.6) is None
    assert check_goal_gate(True, "astar", 0.6) == 0.6 and check_goal_gate(0.25, "astar_ent", 0.6) == 0.25
    assert check_goal_gate(np.float64(1.5), "astar", 0.6) == 1.5
