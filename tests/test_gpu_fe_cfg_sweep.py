"""GPU: the front-end kernels away from the one search configuration scene.frontend_cfg gives (voxel_size 0.2, bias 1.1, goal_size
0.2, cable_length = tether_length, ent_samples 3, the 5 x 5 lattice).  tests/fe_cfg_cases.py names the settings and the set-ups;
tests/test_fe_cfg_cases_cpu.py shows on the references alone that each pair run here differs from the default setting and is not
degenerate.  Every comparison is with an independent reference and bit for bit: the beam against the C oracle (frontend_beam,
frontend_beam_ent), the best-first search without the check against the C oracle's (frontend_astar), with the check against
tests/astar_ent_ref.py — the one-wave kernel and the four-wave kernel each on its own.  Then the handle's own sample count
(nep_batch_set_ent_samples: the hull blocks' size, frontend_ent_hulls at 5, the refusals) and one fleet loop flown at ent_samples 2."""
import numpy as np
import pytest

import astar_ent_cases as cases
import fe_cfg_cases as fc
from neptune_amd import abi, scene

pytestmark = pytest.mark.gpu

BEAM_FIELDS = ("status", "K", "n_children", "n_feasible", "n_collision_free", "n_entangled", "ent_overflow")


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


def _handle(be, sc, **kw):
    bb = be.BatchBackend(sc["par"], sc["statics"], **kw)
    reps, longest = scene.static_reps(sc["statics"]) if len(sc["statics"]) else (np.zeros((0, 2, 2)), np.zeros((0, 2)))
    bb.set_static_reps(reps, longest)
    return bb


def _buffers(bb, n_slots, N):
    T = bb.torch
    d_g = T.full((n_slots * abi.GUESS_DTYPE.itemsize,), 0xAB, dtype=T.uint8, device=bb.device)      # (stale bytes: every byte must be written)
    d_r = T.full((n_slots * abi.FE_RESULT_DTYPE.itemsize,), 0xAB, dtype=T.uint8, device=bb.device)
    d_case = T.zeros(n_slots * abi.NEP_MAX_POL * N, dtype=T.int32, device=bb.device)
    return d_g, d_r, d_case


def _views(d_g, d_r, d_case, n_slots, N):
    return d_g.cpu().numpy().view(abi.GUESS_DTYPE), d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE), d_case.cpu().numpy().reshape(n_slots, abi.NEP_MAX_POL, N)


def _beam_ent(be, key, setting, fast_caps=None, big_records=None):
    """one nep_batch_frontend_ent launch of set-up `key` at `setting` -> (guesses, results, case blocks); bb.check() clean"""
    sc, inits = fc.beam_setup(key); p = sc["par"]; N = p.num_agents
    bb = _handle(be, sc)
    if fast_caps is not None:
        bb.set_fe_ent_fast_caps(*fast_caps)
    if big_records is not None:
        bb.set_fe_ent_big_records(big_records)
    fe = fc.fe_of(p, setting, beam_width=fc.BEAM_SETUPS[key][3])
    d_g, d_r, d_case = _buffers(bb, N, N)
    bb.frontend_ent(fe, bb.to_device(sc["committed"]), bb.to_device(scene.frontend_starts(sc)), d_g, d_r, d_case, d_ent_init=bb.to_device(inits))
    bb.torch.cuda.synchronize()
    got = _views(d_g, d_r, d_case, N, N)
    bb.check()
    bb.close()
    return got


def _beam_same(got, a, want, where, fields=BEAM_FIELDS):
    """as test_entangle_front_end_matches_the_oracle_bit_for_bit compares: K and every coefficient, the counters, the cost, the case block"""
    got_g, got_r, got_case = got
    g, res, case = want
    assert int(got_g[a]["K"]) == int(g["K"]), (where, a, int(got_g[a]["K"]), int(g["K"]))
    np.testing.assert_array_equal(np.array(got_g[a]["coeff"]), np.array(g["coeff"]), err_msg="%r agent %d" % (where, a))
    assert got_g[a]["t_start"] == g["t_start"]
    for f in fields:
        assert int(got_r[a][f]) == res[f], (where, a, f, int(got_r[a][f]), res[f])
    assert float(got_r[a]["cost"]) == res["cost"], (where, a)
    if case is not None:
        np.testing.assert_array_equal(got_case[a], case, err_msg="case block, %r agent %d" % (where, a))


@pytest.mark.parametrize("key,setting", fc.BEAM_ENT_PAIRS)
def test_beam_with_the_check(be, oracle, key, setting):
    """frontend_kernel<true, ...>: every setting on (8, 6, 60); ent_samples 1, 2, 5 and 8 also with tethers of 2-4 and of 5-8 bend
    points and on 72 agents + 40 statics (two mask words of each).  ent_samples != 3 leaves the register fast path of the per-parent
    proof; 5 and 8 at beam width 16 bind the x_hdr_cap clamp; the packed records' stride, the staging cap, the crossing pool and
    d_sampled are all sized by it."""
    want = fc.beam_want(oracle, key, setting)
    got = _beam_ent(be, key, setting)
    for a in fc.beam_agents(key):
        _beam_same(got, a, want[a], (key, setting))
    assert all(w[1]["ent_overflow"] == 0 for w in want.values())


@pytest.mark.parametrize("fast_caps", [(2, 32, 8), (40, 1, 8)])
@pytest.mark.parametrize("setting", ["ent5", "ent8"])
def test_big_record_instantiation(be, oracle, setting, fast_caps):
    """frontend_kernel<true, BIG>: with the fixed record's limits shrunk (list entries; new crossings per sampled step) the searches
    of (16, 8, 61) run on big records at ent_samples 5 and 8: the default-limits run's outputs and the oracle's, bit for bit"""
    key = "16+8"
    want = fc.beam_want(oracle, key, setting)
    ref = _beam_ent(be, key, setting)
    got = _beam_ent(be, key, setting, fast_caps=fast_caps, big_records=1 << 16)
    big = got[1]["_pad"].astype(np.int64) >> 8
    assert big.sum() > 0, big                                                          # (big records were used)
    assert (got[1]["ent_overflow"] == 0).all() and (ref[1]["ent_overflow"] == 0).all()
    assert got[0].tobytes() == ref[0].tobytes()
    np.testing.assert_array_equal(got[2], ref[2])
    for f in ("status", "K", "depth", "n_children", "n_feasible", "n_collision_free", "n_entangled", "cost", "dist_to_goal"):
        np.testing.assert_array_equal(got[1][f], ref[1][f], err_msg=f)
    for a in fc.beam_agents(key):
        _beam_same(got, a, want[a], (key, setting, fast_caps))
        _beam_same(ref, a, want[a], (key, setting, "default limits"))


@pytest.mark.parametrize("key,setting", fc.BEAM_PLAIN_PAIRS + fc.BEAM_PLAIN_SAME)
def test_beam_without_the_check(be, oracle, key, setting):
    """frontend_kernel<false, ...> at beam widths 16 and 64: voxel_size (the per-depth voxel table), bias (every f), goal_size (the
    termination test), the 2 x 2 and 4 x 4 lattices (no child of zero jerk) and all of them at once"""
    sc, _ = fc.beam_setup(key); p = sc["par"]; N = p.num_agents
    want = fc.beam_want(oracle, key, setting, check=False)
    bb = _handle(be, sc)
    fe = fc.fe_of(p, setting, beam_width=fc.BEAM_SETUPS[key][3], entangle=False)
    d_g, d_r, d_case = _buffers(bb, N, N)
    bb.frontend(fe, bb.to_device(sc["committed"]), bb.to_device(scene.frontend_starts(sc)), d_g, d_r)
    bb.torch.cuda.synchronize()
    got = _views(d_g, d_r, d_case, N, N)
    bb.check()
    bb.close()
    for a in fc.beam_agents(key):
        _beam_same(got, a, want[a], (key, setting, "check off"), fields=("status", "K", "n_children", "n_feasible", "n_collision_free"))


def _astar_same(got_g, got_r, a, g, r, where):
    for f in abi.FE_RESULT_DTYPE.names:
        assert got_r[a][f].item() == r[f], (where, a, f, got_r[a][f].item(), r[f])
    assert got_g[a].tobytes() == np.asarray(g).tobytes(), (where, a, "guess bytes", int(got_g[a]["K"]), int(g["K"]))


@pytest.mark.parametrize("name,setting", fc.ASTAR_PLAIN_PAIRS)
def test_best_first_without_the_check(be, oracle, name, setting):
    """frontend_astar_kernel<false>: the open-addressing voxel table and the in-place update of open nodes at other voxel sizes, f at
    other biases, the goal test at other radii, lattices of 4 and 16 children — the whole guess and every result field"""
    sc = cases.setup(name)[0]; p = sc["par"]; N = p.num_agents
    want = fc.astar_plain_want(oracle, name, setting)
    fe = fc.fe_of(p, setting, entangle=False)
    bb = _handle(be, sc)
    bb.set_fe_astar(fc.ASTAR_POPS, 0, fc.lattice_order(fe))
    d_g, d_r, _ = _buffers(bb, N, N)
    bb.frontend_astar(fe, bb.to_device(sc["committed"]), bb.to_device(cases.starts_of(name)), d_g, d_r)
    bb.torch.cuda.synchronize()
    got_g, got_r = d_g.cpu().numpy().view(abi.GUESS_DTYPE), d_r.cpu().numpy().view(abi.FE_RESULT_DTYPE)
    bb.check()
    bb.close()
    for a in range(N):
        _astar_same(got_g, got_r, a, want[a][0], want[a][1], (name, setting, "check off"))


@pytest.mark.parametrize("name,setting", fc.ASTAR_ENT_PAIRS + fc.ASTAR_ENT_SAME)
def test_best_first_with_the_check(be, oracle, name, setting):
    """frontend_astar_kernel<true> (one wave per search), then frontend_astar_team_kernel (four) on the same handle: each against
    tests/astar_ent_ref.py at the setting, on its own — guess bytes, every result field, the case block"""
    sc, inits, _ = cases.setup(name); p = sc["par"]; N = p.num_agents
    want = fc.astar_ent_want(oracle, name, setting)
    fe = fc.fe_of(p, setting)
    bb = _handle(be, sc)
    bb.set_fe_astar(fc.ASTAR_POPS, 0, fc.lattice_order(fe))
    d_com = bb.to_device(sc["committed"]); d_start = bb.to_device(cases.starts_of(name)); d_init = bb.to_device(inits)
    for team in (1, 4):
        bb.set_fe_astar_team(team)
        d_g, d_r, d_case = _buffers(bb, N, N)
        d_case.fill_(-7)
        bb.frontend_astar_ent(fe, d_com, d_start, d_g, d_r, d_case, d_ent_init=d_init)
        bb.torch.cuda.synchronize()
        assert bb.fe_astar_team() == team
        got_g, got_r, got_case = _views(d_g, d_r, d_case, N, N)
        for a in range(N):
            g, r, case, _ = want[a]
            _astar_same(got_g, got_r, a, g, r, (name, setting, "team", team))
            np.testing.assert_array_equal(got_case[a], case, err_msg="case block, %r" % ((name, setting, "team", team, "agent", a),))
    bb.check()
    bb.close()


def test_the_handles_sample_count(be, oracle):
    """nep_batch_set_ent_samples on two "ranks" of four agents each (the scene of the "8+6" set-up): the hull blocks grow by two
    samples per interval, frontend_ent_hulls against blocks made at 5 is the single handle's frontend_ent at 5 and the oracle's, and a
    configuration whose ent_samples is not the handle's is refused, as are 0 and 9 everywhere"""
    from neptune_amd._lib import BackendError
    key, world = "8+6", 2
    sc, inits = fc.beam_setup(key); p = sc["par"]; N = p.num_agents; nl = N // world
    fe3 = fc.fe_of(p, "default", beam_width=16); fe5 = fc.fe_of(p, "ent5", beam_width=16)
    starts = scene.frontend_starts(sc)
    full = _handle(be, sc)
    T = full.torch
    ranks = [_handle(be, sc, first_local=r * nl, n_local=nl) for r in range(world)]
    at3 = [h.hull_block_bytes() for h in ranks]
    for h in ranks:
        h.set_ent_samples(5)
    at5 = [h.hull_block_bytes() for h in ranks]
    up = lambda v: (v + 255) & ~255
    samples = lambda ns: up(nl * p.num_pol * (ns + 1) * 2 * 8)                          # (hull_block_layout: [n_local][num_pol][ns + 1][2] doubles, rounded to 256)
    assert len(set(at3)) == 1 and len(set(at5)) == 1 and at5[0] % 256 == 0 and at3[0] % 256 == 0
    assert at5[0] - at3[0] == samples(5) - samples(3) == nl * p.num_pol * 2 * 2 * 8, (at3, at5)
    # the single handle at 5, and the oracle
    want = fc.beam_want(oracle, key, "ent5")
    d_g, d_r, d_case = _buffers(full, N, N)
    d_com = full.to_device(sc["committed"])
    full.frontend_ent(fe5, d_com, full.to_device(starts), d_g, d_r, d_case, d_ent_init=full.to_device(inits))
    T.cuda.synchronize()
    one = _views(d_g, d_r, d_case, N, N)
    for a in range(N):
        _beam_same(one, a, want[a], ("single handle", "ent5"))
    # the ranks: blocks made at 5, searched at 5
    bb5 = at5[0]
    blocks = T.zeros(world * bb5, dtype=T.uint8, device=full.device)
    clock = np.zeros(N, dtype=abi.GUESS_DTYPE); clock["t_start"] = starts["t_start"]      # (nep_batch_hulls reads the round's clock from the guess records)
    for r, h in enumerate(ranks):
        sl = slice(r * nl, (r + 1) * nl)
        h.hulls(h.to_device(sc["committed"][sl]), h.to_device(clock[sl]), blocks[r * bb5:(r + 1) * bb5])
    for r, h in enumerate(ranks):
        sl = slice(r * nl, (r + 1) * nl)
        g_l, r_l, c_l = _buffers(h, nl, N)
        h.frontend_ent_hulls(fe5, blocks, h.to_device(starts[sl]), g_l, r_l, c_l, d_ent_init=h.to_device(inits[sl]))
        T.cuda.synchronize()
        assert g_l.cpu().numpy().tobytes() == one[0][sl].tobytes(), "guesses of rank %d" % r
        assert r_l.cpu().numpy().tobytes() == one[1][sl].tobytes(), "search results of rank %d" % r
        assert np.array_equal(c_l.cpu().numpy().reshape(nl, abi.NEP_MAX_POL, N), one[2][sl]), "case block of rank %d" % r
        with pytest.raises(BackendError, match="error -1"):                            # NEP_E_ARG: 3 on a handle set to 5
            h.frontend_ent_hulls(fe3, blocks, h.to_device(starts[sl]), g_l, r_l, c_l, d_ent_init=h.to_device(inits[sl]))
        h.check()
    left = _handle(be, sc, first_local=0, n_local=nl)                                  # ... and 5 on a handle left at 3
    g_l, r_l, c_l = _buffers(left, nl, N)
    with pytest.raises(BackendError, match="error -1"):
        left.frontend_ent_hulls(fe5, blocks, left.to_device(starts[:nl]), g_l, r_l, c_l, d_ent_init=left.to_device(inits[:nl]))
    # 0 and 9
    d_guess = full.to_device(sc["guesses"]); d_final = T.zeros_like(d_com); d_state = full.to_device(inits)
    for ns in (0, 9):
        bad = fc.fe_of(p, "default", beam_width=16); bad.ent_samples = ns
        with pytest.raises(BackendError, match="error -1"):
            full.set_ent_samples(ns)
        with pytest.raises(BackendError, match="error -1"):
            full.frontend_ent(bad, d_com, full.to_device(starts), d_g, d_r, d_case)
        with pytest.raises(BackendError, match="error -1"):
            full.safety_commit_ent(d_com, d_com, d_guess, d_final, ent_samples=ns)
        with pytest.raises(BackendError, match="error -1"):
            full.track_ent(d_com, d_final, d_guess, d_state, ent_samples=ns)
    T.cuda.synchronize()
    full.check()
    for h in ranks + [left, full]:
        h.close()


def test_a_fleet_loop_at_two_samples(be):
    """DeviceFleetLoop(tethers=True, search="astar_ent", ent_samples=2) on the 5-agent circle swap of tests/test_gpu_fleet_tether.py,
    for the six rounds of that file's shortest flight: after every predict, commit and track the device equals that file's host
    chain (which reads loop.ent_samples), and the captured round flies the eager rounds' bytes"""
    import test_gpu_fleet_tether as ft
    kw = dict(replan_every=5, search="astar_ent", max_pops=60, ent_samples=2)
    loop = ft._loop([ft._scene(5, 0, 1)], graph=False, **kw)
    assert loop.ent_samples == 2 and loop.fe.ent_samples == 2
    host = ft._fly(loop, 6)
    rep = loop.report()[0]
    assert rep["rounds"] == 6 and rep["accepted"] > 0, rep
    loop.be.check()
    host.close(); loop.close()
    flown = []
    for graph in (False, True):
        loop = ft._loop([ft._scene(5, 0, 1)], graph=graph, **kw)
        flown.append(ft._flight_bytes(loop, 6)[0])
        loop.be.check()
        assert (loop._g is not None) == graph
        loop.close()
    assert flown[0] == flown[1]
