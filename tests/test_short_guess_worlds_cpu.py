"""CPU: what test_gpu_short_guess_paths.py relies on in its inputs (tests/short_guess_worlds.py), fixed by the oracle alone, on the
seeds the GPU file imports.  truncated(D, seed): over a D's seeds the statuses include OK, RELAXED and FAILED, a slot with K < D has
an active separating-line row, a slot has an active box row, and no LP fails.  at_rest(D, seed): for every K in 3..D a slot ends OK
with no active row at all (what the zero-iteration certificate can accept), K = 1 is OK and K = 2 RELAXED in every slot.  Every
world: lines in every slot with a guess."""
import numpy as np
import pytest

import helpers  # noqa: F401
import short_guess_worlds as W
from neptune_amd import abi

OK, RELAXED, FAILED = abi.NEP_OK, abi.NEP_RELAXED, abi.NEP_FAILED


def _lines_everywhere(w, rs):
    for a, r in enumerate(rs):
        assert (r is None) == (int(w["guesses"][a]["K"]) == 0)
        if r is not None:
            assert r["n_lines"] > 0, (w["name"], a)


@pytest.mark.parametrize("D", W.DS)
def test_truncated_worlds_iterate_relax_and_fail(oracle, D):
    statuses, line_act_short, box_act, n_lines = set(), 0, 0, []
    for seed in W.TRUNCATED_SEEDS[D]:
        w = W.truncated(D, seed)
        assert w["par"].num_pol == D and w["par"].T_span == 1.0 and w["par"].v_max == 5.0
        assert [int(k) for k in w["guesses"]["K"]] == [(a % D) + 1 for a in range(W.N)]
        rs = W.oracle_results(oracle, w)
        _lines_everywhere(w, rs)
        for a, r in enumerate(rs):
            K = int(w["guesses"][a]["K"])
            assert not np.array(w["guesses"][a]["coeff"])[:, K:, :].any()
            assert r["n_lp_failed"] == 0, (D, seed, a)
            statuses.add(r["status"]); n_lines.append(r["n_lines"])
            if r["status"] != FAILED:
                nb, nl = W.active_rows(w, a, r)
                box_act += nb > 0
                line_act_short += nl > 0 and K < D
    print("truncated D%d: statuses %r, slots with an active line row at K < D %d, with an active box row %d, n_lines %d..%d" %
          (D, sorted(statuses), line_act_short, box_act, min(n_lines), max(n_lines)))
    assert statuses == {OK, RELAXED, FAILED}
    assert line_act_short >= 1 and box_act >= 1


@pytest.mark.parametrize("D", W.DS)
def test_at_rest_worlds_have_an_untouched_optimum_at_every_length(oracle, D):
    free = {K: 0 for K in range(1, D + 1)}
    for seed in W.AT_REST_SEEDS[D]:
        w = W.at_rest(D, seed)
        assert w["par"].num_pol == D
        full = W.full_length(D, seed)
        assert w["committed"].tobytes() == full["committed"].tobytes() and (full["guesses"]["K"] == D).all()
        rs = W.oracle_results(oracle, w)
        _lines_everywhere(w, rs)
        for a, r in enumerate(rs):
            K = int(w["guesses"][a]["K"])
            assert K == W.guess_length(a, D)
            if K == 1:
                assert r["status"] == OK, (D, seed, a)
            if K == 2:
                assert r["status"] == RELAXED, (D, seed, a)
            if r["status"] == OK and W.active_rows(w, a, r) == (0, 0):
                free[K] += 1
    print("at_rest D%d: slots ending OK with no active row, per K: %r" % (D, free))
    assert all(free[K] >= 1 for K in range(3, D + 1)), free


@pytest.mark.parametrize("D", W.DS)
def test_variants_keep_their_lines(oracle, D):
    """the K = 0 / infeasible variants (both placements), the rotated K assignment and the full-length round of the three-round
    handles: misses have no guess, the infeasible slot fails, every other slot has lines"""
    for kind, seeds in ((W.truncated, W.TRUNCATED_SEEDS[D]), (W.at_rest, W.AT_REST_SEEDS[D])):
        for k, seed in enumerate(seeds[:2]):
            for shift in (0, 3):
                w = W.with_misses(kind(D, seed, shift), k)
                assert sorted(np.flatnonzero(w["guesses"]["K"] == 0)) == sorted(W.MISSES[k])
                rs = W.oracle_results(oracle, w)
                _lines_everywhere(w, rs)
                b = W.bad_agent(D, k)
                assert b not in W.MISSES[k] and rs[b]["status"] == FAILED
                if shift == 0:
                    assert int(w["guesses"][b]["K"]) == D - k      # (long enough for the certificate to have to abstain on it)
    for seed in W.AT_REST_SEEDS[D]:
        w = W.full_length(D, seed)
        _lines_everywhere(w, W.oracle_results(oracle, w))


@pytest.mark.parametrize("D", W.ENT_DS)
def test_entangle_variants_pose_entangle_lps(oracle, D):
    """with_entangle adds LPs (segment against a tether's piece) to slots with K < D, some of them infeasible: counted, absent lines"""
    added_short = failed = 0
    for seed in W.TRUNCATED_SEEDS[D]:
        w = W.truncated(D, seed)
        we = W.with_entangle(w, W.ent_seed(seed))
        assert we["par"].enable_entangle and we["case"].shape == (W.N, abi.NEP_MAX_POL, W.N) and w["case"] is None
        assert (np.array(we["committed"]["n_bend"]) >= 2).all() and (np.array(w["committed"]["n_bend"]) == 1).all()
        rs, re = W.oracle_results(oracle, w), W.oracle_results(oracle, we)
        _lines_everywhere(we, re)
        for a, (r0, r1) in enumerate(zip(rs, re)):
            assert r1["n_lp"] >= r0["n_lp"]
            added_short += r1["n_lp"] > r0["n_lp"] and int(w["guesses"][a]["K"]) < D
            failed += r1["n_lp_failed"]
    print("entangle D%d: slots with K < D and entangle LPs %d, failed LPs %d" % (D, added_short, failed))
    assert added_short >= 2
