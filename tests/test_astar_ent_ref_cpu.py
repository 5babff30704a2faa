"""tests/astar_ent_ref.py, the Python restatement of the reference's best-first search, held to what pins it (no GPU):
with ent=None it is oracle.frontend_astar byte for byte — which pins fe_child, the heap arithmetic, the voxel table, the update toggle
and the closest-so-far node — and with the check on every path it returns is un-entangled by the oracle's own C propagation, with the
case block that propagation gives, on scenes whose searches exercise every rule the check adds."""
import numpy as np
import pytest

import astar_ent_cases as cases
import astar_ent_ref as ref
import helpers
from neptune_amd import abi, scene

SCENES = [(8, 6, 60), (16, 8, 66), (5, 0, 64)]
SHUFFLED = np.random.default_rng(4).permutation(25).astype(np.int32)


@pytest.mark.parametrize("n_agents,n_static,seed", SCENES)
def test_without_the_check_the_ref_is_the_oracles_astar_byte_for_byte(oracle, n_agents, n_static, seed):
    sc = scene.tether_crossing_scene(n_agents, n_static, seed); p = sc["par"]
    starts = scene.frontend_starts(sc)
    n = 0; statuses = set(); pops = set()
    for a in range(n_agents):
        hulls = oracle.hulls_of_scene(p, a + 1, sc["committed"], float(starts[a]["t_start"]), sc["statics"])
        for max_pops, order, ns in ((1, None, 5), (40, None, 5), (150, None, 5), (150, SHUFFLED, 5), (150, None, 3)):
            fe = scene.frontend_cfg(p, num_samples=ns)
            g, r = oracle.frontend_astar(p, fe, a + 1, starts[a], hulls[0], hulls[1], sc["statics"], order=order, max_pops=max_pops)
            g2, r2, case, _ = ref.astar(p, fe, a + 1, starts[a], hulls, sc["statics"], max_pops, order=order)
            for f in abi.FE_RESULT_DTYPE.names:
                assert r2[f] == r[f], (a, max_pops, ns, f, r2[f], r[f])
            assert g2.tobytes() == np.asarray(g).tobytes(), (a, max_pops, ns)
            assert not case.any()
            n += 1; statuses.add(r["status"]); pops.add(r["n_children"])
    assert n == 5 * n_agents and len(statuses) >= 2 and max(pops) > 40      # (not all one outcome; searches that used their budget)


def test_with_the_check_every_returned_path_is_unentangled_and_every_rule_is_exercised(oracle):
    tot = dict(n_entangled=0, updates=0, iz_shared=0, invalid_end_pops=0, cases=0, max_list=0, max_bend=0)
    per = {}
    for name in ("bends", "many_bends", "doubly"):
        sc, inits, _ = cases.setup(name); p = sc["par"]
        starts = scene.frontend_starts(sc)
        want = cases.want(oracle, name)
        per[name] = dict(n_entangled=0, updates=0, invalid_end_pops=0, max_list=0, max_bend=0)
        plans = 0
        for a, (g, r, case, cnt) in want.items():
            assert r["ent_overflow"] == 0 and r["_pad"] == 0, (name, a)
            assert r["n_entangled"] == cnt["n_entangled"]
            for k in ("n_entangled", "updates", "iz_shared", "invalid_end_pops"):
                tot[k] += cnt[k]
            for k in ("n_entangled", "updates", "invalid_end_pops"):
                per[name][k] += cnt[k]
            for k in ("max_list", "max_bend"):
                tot[k] = max(tot[k], cnt[k]); per[name][k] = max(per[name][k], cnt[k])
            tot["cases"] += int((case != 0).sum())
            if r["K"] < 1:
                assert not case.any() and r["status"] == ref.NO_SOLUTION
                continue
            plans += 1
            ent = helpers.ent_inputs(sc, a, t0=float(starts[a]["t_start"]), init=inits[a])
            c_case, hit, _ = oracle.ent_propagate_guess(p, a + 1, p.tether_length, g, ent)
            assert hit == 0, (name, a, hit)
            np.testing.assert_array_equal(case, c_case, err_msg="%s agent %d" % (name, a))
        assert plans >= 3 and len({r["status"] for _, r, _, _ in want.values()}) >= 2, name
    print("coverage:", tot, per)
    for k in ("n_entangled", "updates", "iz_shared", "invalid_end_pops", "cases"):
        assert tot[k] > 0, (k, tot)
    # the figures of the CPU try the issue records, on the same seeds
    assert (per["bends"]["n_entangled"], per["bends"]["updates"], per["bends"]["max_list"]) == (1068, 2427, 5)
    assert (per["doubly"]["invalid_end_pops"], per["doubly"]["max_list"], per["doubly"]["max_bend"]) == (624, 8, 1)
    assert per["many_bends"]["n_entangled"] > 0
