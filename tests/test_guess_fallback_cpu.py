"""The degrade-to-initial-guess rule without a GPU: the header declares the two calls and NEP_GUESS, no record changed its size, the
C entry points refuse a null handle before they touch a device, both fleet loops refuse a fly_guess that is not a boolean (and
TetherLoop the option), and the Python reference (tests/guess_fallback_ref.py) on the oracle's replans and safety pass gives the
outcomes DESIGN section 34 states for the fixture the GPU tests fly."""
import os
import re

import numpy as np
import pytest

import guess_fallback_ref as ref
from neptune_amd import _lib, abi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# nep_abi_sizeof(which) before the rule was built: no record grew for it
SIZES = {0: 1680, 1: 1872, 2: 56, 3: 48, 4: 152, 5: 784, 6: 896, 7: 48, 8: 24, 9: 56, 10: 120, 11: 64, 12: 104, 13: 56, 14: 456, 15: 56,
         17: 112, 18: 80, 20: 136, 21: 64, 23: 56, 25: 80, 27: 16}


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_header_declares_the_calls_and_the_status():
    hdr = open(os.path.join(ROOT, "include", "neptune_backend.h")).read()
    assert int(re.search(r"#define NEP_GUESS\s+(\d+)\b", hdr).group(1)) == 4 == abi.NEP_GUESS == ref.GUESS
    assert re.search(r"^int nep_batch_guess_fallback\(nep_batch_t\* h, const nep_guess\* d_guess, nep_solution\* d_solution,\s*"
                     r"nep_traj_rec\* d_commit, int32_t\* d_count[^,]*, void\* stream\);", hdr, re.M)
    assert re.search(r"^int nep_batch_guess_fallback_tally\(nep_batch_t\* h, const nep_solution\* d_solution, const int32_t\* d_outcome[^,]*,\s*"
                     r"int32_t\* d_count[^,]*, void\* stream\);", hdr, re.M)
    # declared next to nep_batch_replan, before the two-enqueue form
    assert hdr.index("int nep_batch_replan(") < hdr.index("int nep_batch_guess_fallback(") < hdr.index("int nep_batch_replan_lines(")
    assert abi.GUESS_FALLBACK_COUNTS == ("qp_failed_seen", "guess_published", "guess_flown", "guess_not_flown")
    assert (abi.NEP_OK, abi.NEP_RELAXED, abi.NEP_FAILED, abi.NEP_SKIPPED) == (ref.OK, ref.RELAXED, ref.FAILED, ref.SKIPPED) == (0, 1, 2, 3)
    assert {"nep_batch_guess_fallback", "nep_batch_guess_fallback_tally"} <= set(_lib.EXPORTS)


def test_no_record_changed_its_size(L):
    for which, size in SIZES.items():
        assert L.nep_abi_sizeof(which) == size, which
    assert abi.SOLUTION_DTYPE.itemsize == 896 and abi.TRAJ_REC_DTYPE.itemsize == 1872 and abi.GUESS_DTYPE.itemsize == 784


def test_null_handle_is_an_argument_error(L):
    """before any HIP call: the same answer with and without a device"""
    assert L.nep_batch_guess_fallback(None, None, None, None, None, None) == -1      # NEP_E_ARG
    assert L.nep_batch_guess_fallback_tally(None, None, None, None, None) == -1


def test_loops_refuse_what_is_not_a_boolean():
    """before anything touches a device"""
    from neptune_amd.loop import DeviceFleetLoop, FleetLoop, TetherLoop, check_fly_guess
    sc = scene.make_scene(5, 3, seed=0)
    for bad in (1, 0, None, "yes", 1.0, [True]):
        with pytest.raises(ValueError):
            DeviceFleetLoop([sc], fly_guess=bad)
        with pytest.raises(ValueError):
            FleetLoop(sc["par"], sc["statics"], sc["starts"], sc["goals"], fly_guess=bad)
    with pytest.raises(TypeError):
        TetherLoop([sc], fly_guess=True)
    assert "fly_guess" in DeviceFleetLoop._MUST_MATCH
    assert check_fly_guess(True) is True and check_fly_guess(False) is False and check_fly_guess(np.bool_(True)) is True


def test_reference_rule_on_plain_arrays():
    """who is examined, who is published, what is written and what is not, the second call, the tally"""
    sol = np.zeros(6, dtype=abi.SOLUTION_DTYPE); gue = np.zeros(6, dtype=abi.GUESS_DTYPE)
    rng = np.random.default_rng(0)
    com = np.frombuffer(rng.integers(0, 256, 6 * abi.TRAJ_REC_DTYPE.itemsize, dtype=np.uint8).tobytes(), dtype=abi.TRAJ_REC_DTYPE).copy()
    sol["stats"]["status"][:] = [0, 2, 2, 3, 2, 1]
    sol["K"][:] = [8, 3, 0, 0, 7, 8]
    sol["coeff"][:] = rng.normal(size=(6, 3, 8, 4)); sol["times"][:] = rng.normal(size=(6, 9)); gue["coeff"][:] = sol["coeff"]
    pb = rng.normal(size=(3, 2))
    s2, c2, cnt = ref.fallback(sol, gue, com, 5, pb, 0.6, first_local=0, n_local=3)      # num_pol = 5: K = 7 is unpublishable
    assert cnt.tolist() == [[2, 1, 0, 0], [1, 0, 0, 0]]
    assert s2["stats"]["status"].tolist() == [0, 4, 2, 3, 2, 1]
    s2["stats"]["status"][1] = 2
    assert s2.tobytes() == sol.tobytes()      # nothing else of the solutions moved
    m = ref.written_mask(abi.TRAJ_REC_DTYPE.itemsize, abi.TRAJ_REC_DTYPE.fields)
    assert int((~m).sum()) == 7 * 16 + 4
    b0, b1 = (np.frombuffer(x.tobytes(), dtype=np.uint8).reshape(6, -1) for x in (com, c2))
    assert (b0[[0, 2, 3, 4, 5]] == b1[[0, 2, 3, 4, 5]]).all() and (b0[1][~m] == b1[1][~m]).all()
    r = c2[1]
    assert (int(r["id"]), int(r["is_agent"]), int(r["n_bend"]), int(r["valid"]), int(r["pwp"]["n_seg"])) == (2, 1, 1, 1, 3)
    assert r["bbox"].tolist() == [1.2] * 3 and r["pos"].tolist() == sol["coeff"][1][:, 0, 3].tolist() and r["bend"][0].tolist() == pb[1].tolist()
    assert r["pwp"]["times"][:4].tolist() == sol["times"][1][:4].tolist() and not r["pwp"]["times"][4:].any()
    assert r["pwp"]["coeff"][:, :3].tolist() == sol["coeff"][1][:, :3].tolist() and not r["pwp"]["coeff"][:, 3:].any()
    s2["stats"]["status"][1] = 4
    s3, c3, cnt3 = ref.fallback(s2, gue, c2, 5, pb, 0.6, n_local=3, count=cnt)
    assert s3.tobytes() == s2.tobytes() and c3.tobytes() == c2.tobytes() and cnt3.tolist() == [[3, 1, 0, 0], [2, 0, 0, 0]]
    assert ref.tally(s2, [4, 3, 4, 4, 4, 4], 3, cnt).tolist() == [[2, 1, 0, 1], [1, 0, 0, 0]]
    assert ref.tally(s2, [4, 4, 4, 4, 4, 4], 3, cnt).tolist() == [[2, 1, 1, 0], [1, 0, 0, 0]]


def test_fixture_against_the_oracle(oracle):
    """scene.make_scene(5, 3, seed=4), guesses[1] outside the world, guesses[3] the same bytes, guesses[2].K = 0.  The oracle's
    replans of slots 0..4 end 0, 2, 0, 2, 0 (slot 2 is replanned with the K its guess was made with: a K = 0 guess is never solved,
    by the oracle no more than by the library); its safety pass over the solved records of 0, 2, 4 and the GUESS records of 1, 3
    finds the one conflict (1, 3) and turns agent 3 down; with the previous records in 1 and 3 — what a handle without the rule
    leaves there — it finds none."""
    sc, gue = ref.fixture(scene)
    p = sc["par"]
    assert gue[3].tobytes() == gue[1].tobytes() and int(gue[2]["K"]) == 0 and np.array(gue[1]["coeff"])[0, 0, 3] == p.x_max + 5.0
    gor = gue.copy(); gor["K"][2] = sc["guesses"]["K"][2]
    rs = [oracle.replan(p, a + 1, sc["committed"], gor[a], sc["statics"]) for a in range(5)]
    assert [r["status"] for r in rs] == [0, 2, 0, 2, 0]
    t0 = float(gue["t_start"][0])
    prev = sc["committed"].copy()
    sol = np.zeros(5, dtype=abi.SOLUTION_DTYPE)
    for a in range(5):
        K = int(gor["K"][a])
        sol["K"][a] = K; sol["stats"]["status"][a] = rs[a]["status"]
        sol["coeff"][a][:, :K] = rs[a]["coeff"] if rs[a]["status"] != 2 else np.array(gue["coeff"][a])[:, :K]      # (:856-859)
        sol["times"][a][: K + 1] = t0 + np.arange(K + 1) * p.T_span
    solved = prev.copy()
    for a in (0, 2, 4):
        solved[a] = ref.record(prev[a], sol[a], dict(coeff=sol["coeff"][a]), a, p.pb, p.drone_radius)
    s2, fresh, cnt = ref.fallback(sol, gue, solved, p.num_pol, p.pb, p.drone_radius)
    assert cnt.tolist() == [[2, 2, 0, 0]] and s2["stats"]["status"].tolist() == [0, 4, 0, 4, 0]
    for a in (1, 3):
        assert fresh[a]["pos"].tolist() == [p.x_max + 5.0] + np.array(gue["coeff"][a])[1:, 0, 3].tolist()
        assert int(fresh[a]["id"]) == a + 1 and fresh[a]["bend"][0].tolist() == np.asarray(p.pb).reshape(-1, 2)[a].tolist()
    conflict, accept = oracle.safety_resolve(fresh, t0, p.T_span, p.drone_radius)
    assert np.argwhere(conflict).tolist() == [[1, 3], [3, 1]] and accept.tolist() == [1, 1, 1, 0, 1]
    conflict, accept = oracle.safety_resolve(solved, t0, p.T_span, p.drone_radius)      # (slots 1 and 3: the previous records)
    assert not conflict.any() and accept.tolist() == [1, 1, 1, 1, 1]
