"""tests/fe_cfg_cases.py's settings, checked with the references alone (no GPU): on every (set-up, setting) pair the device is held to
in tests/test_gpu_fe_cfg_sweep.py the reference's outcome differs from the default setting's on the same set-up — in some agent's
guess bytes, case block or n_entangled; for goal_size in K or the status, which is all that knob can move — and is not degenerate
(two statuses at least, a search that returns a plan).  A kernel that read a constant in place of the field would fail there.
Each case prints what it found.  The pairs of the *_SAME lists are the ones on which the reference cannot tell the setting from the
default: that is asserted too, and the setting is told apart on another set-up of the *_PAIRS lists.  Then: which pairs reach the
beam's x_hdr_cap clamp, and tests/astar_ent_ref.py against the C oracle's best-first search at every setting a search without the
check reads, byte for byte — what pins the restatement before the device is held to it."""
import os
import subprocess

import numpy as np
import pytest

import astar_ent_cases as cases
import astar_ent_ref as ref
import fe_cfg_cases as fc
from neptune_amd import abi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _uniq(pairs):
    return list(dict.fromkeys(pairs))


def _told_apart(what, key, setting, want, base, two_statuses=True):
    goal = "goal_size" in fc.SETTINGS[setting] and len(fc.SETTINGS[setting]) == 1
    kinds = fc.differs(want, base, goal_only=goal)
    statuses, plans, n_ent = fc.outline(want)
    print("%s, %s at %s: differs from the default setting in %s; statuses %s, %d of %d searches return a plan, n_entangled %d (default %d)"
          % (what, key, setting, sorted(kinds), statuses, plans, len(want), n_ent, fc.outline(base)[2]))
    assert kinds, (what, key, setting, "the reference cannot tell this setting from the default one on this set-up")
    assert plans >= 1 and (len(statuses) >= 2 or not two_statuses), (what, key, setting, statuses, plans)


@pytest.mark.parametrize("key,setting", _uniq(fc.BEAM_ENT_PAIRS + fc.BEAM_BIG_PAIRS + fc.BEAM_TABLE_PAIRS))
def test_beam_with_the_check(oracle, key, setting):
    _told_apart("beam, check on", key, setting, fc.beam_want(oracle, key, setting), fc.beam_want(oracle, key, "default"))


@pytest.mark.parametrize("key,setting", fc.BEAM_PLAIN_PAIRS)
def test_beam_without_the_check(oracle, key, setting):
    """(the 5-agent scene without statics has searches of one status at some settings: there a plan and a difference are asked for)"""
    _told_apart("beam, check off", key, setting, fc.beam_want(oracle, key, setting, check=False), fc.beam_want(oracle, key, "default", check=False),
                two_statuses=key != "5+0 wide")


@pytest.mark.parametrize("name,setting", fc.ASTAR_PLAIN_PAIRS)
def test_best_first_without_the_check(oracle, name, setting):
    _told_apart("best-first, check off", name, setting, fc.astar_plain_want(oracle, name, setting), fc.astar_plain_want(oracle, name, "default"))


@pytest.mark.parametrize("name,setting", fc.ASTAR_ENT_PAIRS)
def test_best_first_with_the_check(oracle, name, setting):
    want = fc.astar_ent_want(oracle, name, setting)
    _told_apart("best-first, check on", name, setting, want, fc.astar_ent_want(oracle, name, "default"))
    assert all(r["ent_overflow"] == 0 and r["_pad"] == 0 for _, r, _, _ in want.values())      # (no capacity in the way: bb.check() stays clean)


def test_pairs_on_which_a_setting_equals_the_default(oracle):
    """the *_SAME pairs: run on the device all the same, but no test of the setting — the reference's outcome is the default one's
    there in everything the setting could be told by"""
    for key, setting in fc.BEAM_PLAIN_SAME:
        assert not fc.differs(fc.beam_want(oracle, key, setting, check=False), fc.beam_want(oracle, key, "default", check=False), goal_only=True), (key, setting)
        assert any(s == setting and k != key for k, s in fc.BEAM_PLAIN_PAIRS), (key, setting)
    for name, setting in fc.ASTAR_ENT_SAME:
        assert not fc.differs(fc.astar_ent_want(oracle, name, setting), fc.astar_ent_want(oracle, name, "default"), goal_only=setting.startswith("goal")), (name, setting)
        assert any(s == setting and k != name for k, s in fc.ASTAR_ENT_PAIRS), (name, setting)


def test_which_pairs_reach_the_clamp(tmp_path):
    """frontend_kernel<true> re-partitions its propagation pass when n_merge * ent_samples outgrows x_hdr_cap = x_words = twice the
    children cap; a depth merges up to 256 children.  From the layout header itself (tests/cpp/lds_layout_check.cpp): the pairs of the
    device sweep with 256 * ent_samples > x_words — on the 5 x 5 lattice at beam width 16 (800 words) every ent_samples 5 and 8 pair
    and none below; the 2 x 2 and 4 x 4 lattices have 128 and 512 words, below 256 * 3."""
    exe = str(tmp_path / "lds_layout_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "lds_layout_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pairs = _uniq(fc.BEAM_ENT_PAIRS + fc.BEAM_BIG_PAIRS)
    rows = []
    for key, setting in pairs:
        N, S, _, W, _, _ = fc.BEAM_SETUPS[key]
        fe = fc.fe_of(fc.beam_setup(key)[0]["par"], setting, beam_width=W)
        rows.append("frontend %d %d %d %d %d 1 %d" % (N, S, W, fe.num_samples, abi.NEP_MAX_POL, fe.ent_samples))
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("lds_layout_check ok\n"), (r.stdout[-600:], r.stderr[-2000:])
    answers = r.stdout.splitlines()[:-2]
    assert len(answers) == len(rows)
    clamped = []
    for (key, setting), asked, line in zip(pairs, rows, answers):
        echo, _, vals = line.partition(" : ")
        assert echo == asked
        cap = int(vals.split()[1])
        ns = int(asked.split()[-1])
        if 256 * ns > 2 * cap:
            clamped.append((key, setting, ns, 2 * cap))
    print("pairs with 256 * ent_samples > x_words (set-up, setting, ent_samples, x_words):", clamped)
    small_lattice = {(k, s) for k, s in pairs if "num_samples" in fc.SETTINGS[s]}       # (a children cap of 64 or 256: the bound is below 256 * 3 there)
    assert {(k, s) for k, s, _, _ in clamped} - small_lattice == {(k, s) for k, s in pairs if fc.SETTINGS[s].get("ent_samples", 3) >= 5} - small_lattice
    assert ("8+6", "ent5", 5, 800) in clamped and ("8+6", "ent8", 8, 800) in clamped and ("8+6", "combined", 5, 512) in clamped


@pytest.mark.parametrize("setting", fc.NO_CHECK)
def test_without_the_check_the_ref_is_the_oracles_astar_at_every_setting(oracle, setting):
    """tests/test_astar_ent_ref_cpu.py's comparison away from the default configuration: voxel_size (the voxel table and the in-place
    update of open nodes), bias (every f), goal_size (the termination test) and the 2 x 2 and 4 x 4 lattices — guess, result and
    counters byte for byte, at budgets of 40 and 150 pops on (8, 6, 60) and (16, 8, 66)"""
    n = 0; statuses = set(); pops = set()
    for N, M, seed in ((8, 6, 60), (16, 8, 66)):
        sc = scene.tether_crossing_scene(N, M, seed); p = sc["par"]
        starts = scene.frontend_starts(sc)
        fe = fc.fe_of(p, setting, entangle=False)
        for a in range(N):
            hulls = oracle.hulls_of_scene(p, a + 1, sc["committed"], float(starts[a]["t_start"]), sc["statics"])
            for max_pops in (40, fc.ASTAR_POPS):
                g, r = oracle.frontend_astar(p, fe, a + 1, starts[a], hulls[0], hulls[1], sc["statics"], order=fc.lattice_order(fe), max_pops=max_pops)
                g2, r2, case, _ = ref.astar(p, fe, a + 1, starts[a], hulls, sc["statics"], max_pops, order=fc.lattice_order(fe))
                for f in abi.FE_RESULT_DTYPE.names:
                    assert r2[f] == r[f], (setting, seed, a, max_pops, f, r2[f], r[f])
                assert g2.tobytes() == np.asarray(g).tobytes(), (setting, seed, a, max_pops)
                assert not case.any()
                n += 1; statuses.add(r["status"]); pops.add(r["n_children"])
    assert n == 48 and len(statuses) >= 2 and max(pops) > 40, (statuses, pops)


def test_the_rechecks_inputs_give_both_verdicts_at_every_count(oracle):
    """fe_cfg_cases.recheck_inputs: entangleCheckGivenPwp says "entangled" for some new trajectories and "free" for others at
    ent_samples 1, 2, 3, 5 and 8, and not the same ones at 1 and 2 as at 3, 5 and 8 — what test_safety_pass_entangle_recheck holds
    ent_check_kernel to.  (On the back end's own new trajectories of tether_crossing_scene(8, 6, 60) every verdict is "free": the
    guesses pass the tethers between their second and sixth knot, and the re-check reads the first interval alone.)"""
    import helpers
    sc = scene.tether_crossing_scene(*fc.RECHECK_SCENE); p = sc["par"]; N = p.num_agents
    fresh, inits = fc.recheck_inputs(sc)
    for k, expected in fc.RECHECK_VERDICTS.items():
        got = []
        for a in range(N):
            ent = helpers.ent_inputs(sc, a, num_samples=k, recs=fresh, t0=float(sc["guesses"][a]["t_start"]), init=inits[a])
            got.append(int(oracle.entangle_check_pwp(p, a + 1, p.tether_length, np.array(fresh[a]["pwp"]["coeff"])[0, 0], np.array(fresh[a]["pwp"]["coeff"])[1, 0], ent)))
        print("re-check, ent_samples %d: verdicts %r" % (k, got))
        assert got == expected and 0 < sum(got) < N, (k, got)
    assert fc.RECHECK_VERDICTS[2] != fc.RECHECK_VERDICTS[3]


def test_the_cache_keys_carry_the_setting(oracle):
    """astar_ent_cases.want: a result computed at one setting is never served for another, and the callers from before the setting
    existed get what they got"""
    a = cases.want(oracle, "plain", max_pops=5, agents=(0, 6))
    b = cases.want(oracle, "plain", max_pops=5, agents=(0, 6), ent_samples=1)
    c = cases.want(oracle, "plain", max_pops=5, agents=(0, 6), setting=(("ent_samples", 1),))
    d = cases.want(oracle, "plain", max_pops=5, agents=(0, 6), setting=(("voxel_size", 0.45),))
    assert a is not b and a is not c and a is not d and c is not d
    assert a is cases.want(oracle, "plain", max_pops=5, agents=(0, 6), ent_samples=3, setting=())
    assert cases.fe_cfg(cases.setup("plain")[0]["par"]).ent_samples == 3 and cases.fe_cfg(cases.setup("plain")[0]["par"], setting=fc.overrides("combined")).num_samples == 4
    for x, y in ((b, c),):
        for k in x:
            assert np.asarray(x[k][0]).tobytes() == np.asarray(y[k][0]).tobytes() and x[k][1] == y[k][1]
