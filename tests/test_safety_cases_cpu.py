"""CPU: the cases of safety_cases.py are not vacuous and their references agree — what test_gpu_safety_sizes.py holds the device
to.  Everything here is the oracle's (orc_safety_resolve, orc_safety_resolve_prev, orc_gjk_collision) or plain numpy.

configuration          what it reaches in safety_conflict_kernel / safety_resolve_kernel
default, N = 5, 6      N % 4 != 0 (waves without an agent), one partial staging round
default, N = 13        two rounds (8 agents each at num_pol 8), the second partial
default, N = 37        five rounds, two 32-bit words per conflict row
pol5, N = 26           12 agents per round, 4 idle lanes in the ballot
pol6, N = 70, K = 4    10 agents per round, three words, records shorter than num_pol
default, N = 261       33 rounds, nine words: the accepted set in LDS — tiled apart, and stacked (a dense matrix)"""
import numpy as np
import pytest

import safety_cases as SC


def _stats(sc):
    C, acc = sc["C"], sc["accept"]
    N = len(acc)
    sym = (C | C.T).astype(bool)
    chains = sum(1 for a in range(N) if not acc[a] and (sym[a, a + 1:] & (acc[a + 1:] == 1)).any())
    return dict(conflicts=int(C.sum()), one_directional=int((C != C.T).sum()) // 2, rejected=int((acc == 0).sum()), chains=chains)


@pytest.mark.parametrize("key", list(SC.CONFIGS))
def test_fleet_cases_reach_what_they_are_for(oracle, key):
    name, N, stacked, _ = SC.CONFIGS[key]
    scs = SC.config(key)
    assert len(scs) == 3 and len({sc["t_start"] for sc in scs}) == 3
    ones = np.ones(N, np.int32)
    tot = dict(conflicts=0, one_directional=0, rejected=0, chains=0)
    for k, sc in enumerate(scs):
        p, C, Cp = sc["par"], sc["C"], sc["Cp"]
        assert p.num_agents == N and len(sc["fresh"]) == N and list(sc["fresh"]["id"]) == list(range(1, N + 1))
        assert all(sc["fresh"][a].tobytes() != sc["prev"][a].tobytes() for a in range(N))
        # 1. the rule in numpy is the oracle's, without and with the previous-record check
        np.testing.assert_array_equal(SC.resolve(C, None, ones), sc["accept"])
        np.testing.assert_array_equal(SC.resolve(C, Cp, ones), sc["accept_prev"])
        assert not np.diag(C).any() and not np.diag(Cp).any()
        # 2. something to find, somebody accepted, somebody turned down
        assert C.any() and sc["accept"].any() and not sc["accept"].all()
        # 3. conflicts beyond the first staging round, the first row word, the eight register words
        cols = np.nonzero(C)[1]
        if N >= 13:
            assert cols.max() >= 64 // p.num_pol, (key, k)
        if N > 32:
            assert cols.max() >= 32
        if N == 261:
            assert cols.max() >= 256
        # 5. each flag alone changes the oracle's matrix: the flagged agent's row or column against the unflagged records'
        assert sorted(sc["where"]) == sorted(SC.FLAGS) and len(set(sc["where"].values())) == 3
        for flag, a in sc["where"].items():
            row0, col0 = SC.row_and_column(oracle, p, sc["unflagged"], a, sc["t_start"])
            one = sc["unflagged"].copy(); SC.set_flag(one, a, flag)
            row1, col1 = SC.row_and_column(oracle, p, one, a, sc["t_start"])
            assert row0.any() and col0.any(), (key, k, flag)
            assert (row0 != row1).any() or (col0 != col1).any(), (key, k, flag)
        for t, v in _stats(sc).items():
            tot[t] += v
    # 6. a scene's own clock matters: the matrix on the grid of its t_start is not the matrix on the grid of 0
    at0 = SC._in_threads([(oracle.safety_resolve, (sc["fresh"], 0.0, sc["par"].T_span, sc["par"].drone_radius)) for sc in scs[1:]])
    for sc, (C_at0, _) in zip(scs[1:], at0):
        assert sc["t_start"] > 0 and (C_at0 != sc["C"]).any(), (key, sc["t_start"])
    print("\n%s: %s" % (key, tot))


def test_fleet_cases_together_hold_one_directional_conflicts_and_chains():
    """4. C[a, j] != C[j, a] somewhere, and a rejected agent that conflicts with a later, accepted one: what tells "conflicts with an
    accepted lower id" from "conflicts with any lower id" """
    per = {key: [_stats(sc) for sc in SC.config(key)] for key in SC.CONFIGS}
    assert sum(s["one_directional"] for v in per.values() for s in v) >= 1
    assert sum(s["chains"] for v in per.values() for s in v) >= 1


def _wrong_walk(C, variant):
    """safety_resolve_kernel's id-ordered walk with one mistake: "row" = the symmetric OR dropped (only C[a, j] counts), "lower" = a
    conflict with ANY lower id turns down, "regs" = beyond eight row words the accepted set is never seen"""
    N = len(C)
    row = C.astype(bool) if variant == "row" else (C | C.T).astype(bool)
    acc = np.zeros(N, np.int32)
    for a in range(N):
        seen = np.arange(N) < a if variant == "lower" else acc == 1
        bad = (row[a] & seen).any() and not (variant == "regs" and N > 256)
        acc[a] = 0 if bad else 1
    return acc


@pytest.mark.parametrize("variant", ["row", "lower", "regs"])
def test_wrong_resolution_rules_are_told_apart(variant):
    """the accept flags of the cases separate the rule from three plausible mistakes in the kernel that applies it"""
    differ = [key for key in SC.CONFIGS if any((_wrong_walk(sc["C"], variant) != sc["accept"]).any() for sc in SC.config(key))]
    print("\n%s: differs at %s" % (variant, differ))
    assert differ
    if variant == "regs":
        assert differ == ["default-261", "default-261-stacked"]


def test_masked_cases_put_accepted_first_bits_in_two_words():
    for key in SC.MASKED:
        N = SC.CONFIGS[key][1]
        m = SC.masks(N)
        assert m[0].all() and 0 < m[1].sum() < N and not m[2][:40].any() and m[2][40:].all()
        for sc, mc in zip(SC.config(key), SC.masked_config(key)):
            ina = mc["mask"] == 0
            assert mc["judged"][ina].tobytes() == sc["prev"][ina].tobytes() and mc["judged"][~ina].tobytes() == sc["fresh"][~ina].tobytes()
            want = SC.resolve(mc["C"], mc["Cp"], mc["mask"])
            assert want[ina].all()
            if ina.any() and not ina.all():          # (N = 37 under the third mask: nobody is active, everybody is accepted first)
                # an inactive agent turns an active one down: the accepted-first bits are read
                sym = (mc["C"] | mc["C"].T).astype(bool)
                assert (sym[np.ix_(~ina, ina)].any(axis=1) & (want[~ina] == 0)).any(), key


def test_resolve_is_the_rule_on_a_hand_made_matrix():
    C = np.zeros((5, 5), np.uint8)
    C[1, 0] = 1; C[3, 1] = 1; C[2, 4] = 1            # 1 turned down by 0; 3 meets only 1 (rejected): accepted; 4 meets 2 (accepted) one way
    np.testing.assert_array_equal(SC.resolve(C, None, np.ones(5, np.int32)), [1, 0, 1, 1, 0])
    np.testing.assert_array_equal(SC.resolve(C, None, np.array([1, 0, 1, 1, 1], np.int32)), [0, 1, 1, 0, 0])      # 1 held: accepted first
    Cp = np.zeros((5, 5), np.uint8); Cp[2, 3] = 1
    np.testing.assert_array_equal(SC.resolve(C, Cp, np.ones(5, np.int32)), [1, 0, 0, 1, 1])


def test_gjk_grid_cases_exact_verdicts_and_the_oracle(oracle):
    polys, quads, verdict, decisive = SC.gjk_grid_cases(0)
    fam = SC.gjk_grid_families(0)
    assert 5500 <= len(polys) <= 6500 and quads.shape == (len(polys), 4, 2)
    assert all((P * SC.GRID == np.round(P * SC.GRID)).all() and np.abs(P).max() <= 8 for P in polys)
    assert (quads * SC.GRID == np.round(quads * SC.GRID)).all() and np.abs(quads).max() <= 8
    assert {len(P) for P in polys} >= set(range(1, 17))
    got = np.array([oracle.gjk_collision(P, Q) for P, Q in zip(polys, quads)])
    np.testing.assert_array_equal(got[decisive], verdict[decisive])
    touching = ~decisive
    assert touching.any() and verdict[touching].all()                 # (a touching pair intersects; what gjk::collision says there is pinned by the oracle)
    for f, name in enumerate(SC.FAMILIES):
        m = fam == f
        assert (m & decisive).any(), name
        print("\n%-17s %4d cases: %4d decisive (%4d hit), %4d touching (%d reported as hit)" %
              (name, m.sum(), (m & decisive).sum(), (m & decisive & verdict).sum(), (m & touching).sum(), (m & touching & got).sum()))
    # both answers among the decisive cases of the families that can miss
    for name in ("random", "point_or_segment", "boxes", "small_hull"):
        m = (fam == SC.FAMILIES.index(name)) & decisive
        assert verdict[m].any() and not verdict[m].all(), name
    # equal centroids: the start direction falls back to (1, 0)
    conc = fam == SC.FAMILIES.index("concentric")
    assert all((P.mean(axis=0) == Q.mean(axis=0)).all() for P, Q in zip([polys[i] for i in np.flatnonzero(conc)], quads[conc]))
    print("decisive %d, touching %d" % (decisive.sum(), touching.sum()))


def test_exact_verdicts_on_known_pairs():
    sq = np.array([[0, 0], [8, 0], [8, 8], [0, 8]])
    assert SC.exact_verdicts(sq, sq + [4, 4]) == (True, True)
    assert SC.exact_verdicts(sq, sq + [8, 0]) == (True, False)         # a common edge
    assert SC.exact_verdicts(sq, sq + [8, 8]) == (True, False)         # a common corner
    assert SC.exact_verdicts(sq, sq + [9, 0]) == (False, False)
    assert SC.exact_verdicts(sq[:1], sq[:1]) == (True, False)
    assert SC.exact_verdicts(np.array([[0, 0], [8, 8]]), np.array([[0, 8], [8, 0]])) == (True, True)       # crossing segments
    assert SC.exact_verdicts(np.array([[0, 0], [8, 0]]), np.array([[4, 0], [12, 0]])) == (True, False)      # collinear, overlapping
    assert SC.exact_verdicts(np.array([[0, 0], [8, 0]]), np.array([[9, 0], [12, 0]])) == (False, False)
