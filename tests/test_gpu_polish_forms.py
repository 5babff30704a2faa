"""GPU tests of the polish pass's two forms (qp_polish_kernel.hip): the batched form (the default) against the first one ("polish_impl" 0),
and the movement bound that spares a certified slot its parked lines against always reading them ("parked_bound" 0).  Every comparison is
between fresh handles on the same inputs and asks for ZERO differing bytes in the solutions (stats.solve_us blanked: a device time), the
sampled states, the commit records, the certificate's marks, the polish flags, the polish counts and the redo count with its reasons.
The cases assert what they contain — a slot certified in mode 0, one certified in the relaxed mode, one listed and left alone, listed
slots whose certified point left the bound so that their parked lines ARE read (bit 9 of the flag word, per variant) — so that none of
them can pass on an empty list.  "A parked line really violated" is asserted through qp_reg_kernel's redo reason, that is from the
interior point's own verification and NOT from the pass: a slot reaches the pass only after the interior point's iterate passed every
parked line, and the polished point lies within 1e-4 of it, so no scene tried (32, seven radii) has a slot the pass refuses.  The
pass's refusal (bit 10) is therefore compared between the forms — equal, and zero on these inputs — but never exercised."""
import numpy as np
import pytest

import helpers  # noqa: F401
import short_guess_worlds as W
from neptune_amd import abi, scene
from neptune_amd import dist as ndist

pytestmark = pytest.mark.gpu

VARIANTS = ((1, 1), (0, 1), (1, 0))          # (polish_impl, parked_bound): the default first
S, N = 2, 64


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


def _set(impl=1, bound=1, grid=256):
    from neptune_amd import _lib
    L = _lib.lib()
    assert L.nep_debug_set_global_option(b"polish_impl", impl) == 0 and L.nep_debug_set_global_option(b"parked_bound", bound) == 0
    assert L.nep_debug_set_global_option(b"polish_grid", grid) == 0


@pytest.fixture(autouse=True)
def _defaults_again():
    yield
    _set()


READ = 0x200          # bit 9 of a slot's flag word: the pass read a certified point's parked lines back; bit 10: it refused the point


def _same(a, b):
    """zero differing bytes (keys with a leading underscore are a case's own notes)"""
    keys = [k for k in a if not k.startswith("_")]
    assert keys == [k for k in b if not k.startswith("_")]
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _all(bb):
    """everything a replan left in the handle, as bytes-comparable arrays (stats.solve_us blanked: a device time); of the flag words the
    READ bit is kept apart: it is what "parked_bound" and the first form change"""
    sol = bb.solutions().copy()
    sol["stats"]["solve_us"] = 0.0
    fl = bb.polish_flags().copy()
    out = {"sol": sol, "states": bb.states().copy(), "commit": bb.commits().copy(), "marks": bb.debug_presolved(),
           "redo": np.asarray(bb.redo_count()), "polish": np.asarray(bb.polish_count()), "flags": fl & ~READ, "_read": int(((fl & READ) != 0).sum())}
    out["redo_reasons"] = np.asarray([bb.redo_reasons["parked_line_violated"], bb.redo_reasons["moved_beyond_radius"]])
    return out


def _live(out):
    """the outputs with the state rows behind each slot's n_states blanked: a replan does not write them, so on a handle that has
    replanned before they hold an earlier round's"""
    out = dict(out, states=out["states"].copy())
    for k, ns in enumerate(out["sol"]["n_states"].reshape(-1)):
        out["states"][k, int(ns):] = 0.0
    return out


def _classes(out):
    """what a replan's outputs contain, per class of listed slot"""
    fl, st = out["flags"], out["sol"]["stats"]["status"].reshape(-1).astype(int)
    cert = (fl & 0x100) != 0
    return {"listed": int((fl != 0).sum()), "refused": int(((fl & 0x400) != 0).sum()), "both_modes": int(((fl & 3) == 3).sum()), "certified_mode0": int((cert & (st == abi.NEP_OK)).sum()),
            "certified_relaxed": int((cert & (st == abi.NEP_RELAXED)).sum()), "left_alone": int(((fl != 0) & ~cert).sum()),
            "redo": int(out["redo"]), "parked_violated": int(out["redo_reasons"][0]), "moved": int(out["redo_reasons"][1])}


def _variants(make, replan, variants=VARIANTS, grid=256):
    """the same replan on a fresh handle per variant -> the default's outputs, every other one compared with it byte for byte"""
    outs = []
    for impl, bound in variants:
        _set(impl, bound, grid)
        bb = make()
        replan(bb)
        outs.append(_all(bb))
        bb.close()
    for o in outs[1:]:
        _same(outs[0], o)
    outs[0]["_reads"] = [o["_read"] for o in outs]      # (slots whose parked lines were read back, per variant)
    assert tuple(int(v) for v in outs[0]["polish"]) == (int((outs[0]["flags"] != 0).sum()), int(((outs[0]["flags"] & 0x100) != 0).sum()))
    return outs[0]


# ---- front-end guesses: two 64-agent + 20-static scenes ----

@pytest.fixture(scope="module")
def fe(be):
    """-> (scenes, committed [S][N], front-end guesses [S][N] as the device left them); never modified by a case"""
    scs = [scene.make_scene(N, 20, seed=200 + s) for s in range(S)]
    com, gue = ndist.stack_scenes(scs)
    bb = _fe_handle(be, scs)
    d_g = bb.to_device(gue)
    bb.frontend(scene.frontend_cfg(scs[0]["par"], beam_width=32), bb.to_device(com), bb.to_device(np.stack([scene.frontend_starts(s) for s in scs])), d_g, None)
    g = d_g.cpu().numpy().view(abi.GUESS_DTYPE).reshape(S, N).copy()
    bb.close()
    return scs, com, gue, g


def _fe_handle(be, scs):
    bb = be.BatchBackend(scs[0]["par"], scs[0]["statics"], n_scenes=len(scs))
    for s in range(1, len(scs)):
        bb.set_scene_statics(s, scs[s]["statics"])
    return bb


def _fe_replan(com, g, radius):
    def run(bb):
        bb.set_line_cull(radius)
        bb.replan(bb.to_device(com), bb.to_device(g))
    return run


@pytest.mark.parametrize("radius", [4.0, 0.3, 0.0])
def test_front_end_guesses(be, fe, radius):
    """radius 4: the bound holds and the parked lines are not read; 0.3: most replans move farther — lines read, redo pass; 0: every
    row, ~510 staged lines per slot"""
    scs, com, _, g = fe
    out = _variants(lambda: _fe_handle(be, scs), _fe_replan(com, g, radius))
    c = _classes(out)
    print("front-end guesses, radius %.1f: %r" % (radius, c))
    assert c["listed"] >= 2 and c["certified_mode0"] >= 1 and c["left_alone"] >= 1
    reads = out["_reads"]          # (default, first form, "parked_bound" 0)
    print("  slots whose parked lines were read back: %r" % (reads,))
    assert reads[1] == reads[2]
    if radius == 4.0:              # certified points stay within the bound: the default reads no parked line, the other two those of every certified candidate
        assert reads[0] == 0 and reads[1] >= c["certified_mode0"] >= 1
    if radius == 0.3:              # the bound fails: listed slots' certified points moved farther than r^2 (1 - 1e-9) and their lines ARE read
        assert 1 <= reads[0] <= reads[1]
        assert c["redo"] > S * N // 2 and c["moved"] >= 1 and c["parked_violated"] >= 1      # (the interior point's own verification: a parked line really violated)
    if radius == 0.0:              # no presolve, nothing parked
        assert reads == [0, 0, 0]


@pytest.mark.parametrize("radius", [4.0, 0.0])
def test_small_grid_walks_several_slots_per_workgroup(be, fe, radius):
    """"polish_grid" 2: a workgroup walks half the list — nothing of one slot may survive into the next"""
    scs, com, _, g = fe
    want = _variants(lambda: _fe_handle(be, scs), _fe_replan(com, g, radius), variants=VARIANTS[:1])
    out = _variants(lambda: _fe_handle(be, scs), _fe_replan(com, g, radius), grid=2)
    assert _classes(out)["listed"] > 4
    _same(want, out)


def test_one_slot_launch(be, fe):
    """the per-agent handle's launch of one workgroup is its own list (gridDim.x == 1)"""
    scs, com, _, g = fe
    sc = scs[0]
    full = _variants(lambda: _fe_handle(be, scs[:1]), _fe_replan(com[:1], g[:1], 4.0), variants=VARIANTS[:1])
    listed = np.flatnonzero(full["flags"] != 0)
    assert len(listed) >= 1
    n_listed = n_cert = 0
    for a in [int(a) for a in listed[:3]] + [int(np.flatnonzero(full["flags"] == 0)[0])]:
        def run(bb):
            bb.replan(bb.to_device(sc["committed"][None]), bb.to_device(g[0, a:a + 1]))
        out = _variants(lambda: be.BatchBackend(sc["par"], sc["statics"], first_local=a, n_local=1), run)
        n_listed += int(out["polish"][0]); n_cert += int(out["polish"][1])
        np.testing.assert_array_equal(np.array(out["sol"].reshape(-1)[0]["coeff"]), np.array(full["sol"].reshape(-1)[a]["coeff"]))
    assert n_listed >= 1 and n_cert >= 1


# ---- short guesses: every K, K < 3 among them, relaxed and failing solves, entangle rows ----

def _short(be, worlds, path):
    """-> (the default variant's outputs, guesses [S][N]) of the worlds as the scenes of one handle, the variants compared"""
    p, statics, gue, com, case = W.stack(worlds)

    def make():
        bb = be.BatchBackend(p, statics[0], n_scenes=len(worlds))
        for s in range(1, len(worlds)):
            bb.set_scene_statics(s, statics[s])
        return bb

    def run(bb):
        if path == "every_row":
            bb.set_line_cull(0.0)
        d_ent = bb.torch.from_numpy(case.reshape(-1)).to(bb.device) if case is not None else None
        bb.replan(bb.to_device(com), bb.to_device(gue), d_ent=d_ent)
    return _variants(make, run), gue


@pytest.mark.parametrize("path", ["default", "every_row"])
@pytest.mark.parametrize("kind", ["truncated", "truncated+ent"])
@pytest.mark.parametrize("D", [6, 8])
def test_short_guesses(be, D, kind, path):
    """the worlds of test_gpu_short_guess_paths: their listed slot has both modes listed and is left alone"""
    worlds = [W.truncated(D, s) for s in W.TRUNCATED_SEEDS[D]]
    if kind.endswith("+ent"):
        worlds = [W.with_entangle(w, W.ent_seed(s)) for w, s in zip(worlds, W.TRUNCATED_SEEDS[D])]
    out, gue = _short(be, worlds, path)
    c = _classes(out)
    print("short guesses D %d %s %s: %r, K of the listed slots %r" % (D, kind, path, c, sorted(set(gue["K"].reshape(-1)[out["flags"] != 0].tolist()))))
    st = out["sol"]["stats"]["status"].reshape(-1).astype(int)
    assert (gue["K"] < 3).any() and (st == abi.NEP_FAILED).any() and (st == abi.NEP_RELAXED).any()
    assert c["listed"] >= 1 and c["both_modes"] >= 1 and c["left_alone"] >= 1


# (seed, shift) of truncated worlds in which the oracle's own polish ends a RELAXED solve (orc_set_polish, oracle.last_polished()): at
# D = 6 agent 5 of (3, 1) with K = 1 and of (3, 2) with K = 2 — no first problem to polish at all: nz = 0 — and agent 1 of (14, 1) with K = 3
RELAXED_WORLDS = {6: ((3, 1), (3, 2), (14, 1)), 8: ((14, 1),)}


@pytest.mark.parametrize("path", ["default", "every_row"])
@pytest.mark.parametrize("D", [6, 8])
def test_short_guesses_certified_in_the_relaxed_mode(be, D, path):
    out, gue = _short(be, [W.truncated(D, seed, shift) for seed, shift in RELAXED_WORLDS[D]], path)
    c = _classes(out)
    print("short guesses D %d relaxed worlds %s: %r, K of the listed slots %r" % (D, path, c, sorted(set(gue["K"].reshape(-1)[out["flags"] != 0].tolist()))))
    assert c["certified_relaxed"] >= 1
    if D == 6:
        assert (gue["K"].reshape(-1)[(out["flags"] & 0x100) != 0] < 3).any()      # K < 3: the relaxed problem alone


# ---- three rounds on one handle, eager and as a replayed graph ----

def test_rounds_on_one_handle_and_replayed_graph(be, fe):
    """front-end guesses, the scenes' own guesses, front-end guesses again: no list, flag or count of one round may reach the next.
    The references are fresh handles in the first form; the eager and the replayed handle run the default and the always-read variant."""
    import torch
    scs, com, gue, g = fe
    rounds = (g, gue.reshape(S, N), g)
    want = []
    for r in rounds:
        want.append(_variants(lambda: _fe_handle(be, scs), _fe_replan(com, r, 4.0), variants=VARIANTS[1:2]))
    assert _classes(want[0])["listed"] >= 2
    for impl, bound in (VARIANTS[0], VARIANTS[2]):
        _set(impl, bound)
        bb = _fe_handle(be, scs)
        d_com = bb.to_device(com)
        for r, w in zip(rounds, want):
            bb.replan(d_com, bb.to_device(r))
            _same(_live(_all(bb)), _live(w))
        bb.close()
        bb = _fe_handle(be, scs)
        d_com = bb.to_device(com); d_g = bb.to_device(g)
        s_ = torch.cuda.Stream(bb.device)
        s_.wait_stream(torch.cuda.current_stream(bb.device))
        with torch.cuda.stream(s_):
            bb.replan(d_com, d_g)
        torch.cuda.current_stream(bb.device).wait_stream(s_)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            bb.replan(d_com, d_g)
        for r, w in zip(rounds, want):
            d_g.copy_(bb.to_device(r))
            gr.replay()
            torch.cuda.synchronize()
            _same(_live(_all(bb)), _live(w))
        del gr
        bb.close()


# ---- a climbing world: certified slots whose output z is the guess's (solver_gurobi_poly.cpp:879-880) ----

@pytest.mark.parametrize("path", ["default", "every_row"])
def test_certified_slot_with_the_z_override(be, path):
    """test_gpu_param_sweep's fast_long world at 64 agents with z motion: a certified slot whose start lies within 1 m (x, y) of the
    guess's end returns the guess's z — the objective is the optimum's, z included, and must be summed before the z rows are replaced"""
    import param_sets as PS
    import param_util as PU
    sc = PU.with_z_motion(PS.make_scene("fast_long", 64, 20, seed=5), np.random.default_rng(107))
    p = sc["par"]

    def run(bb):
        if path == "every_row":
            bb.set_line_cull(0.0)
        bb.replan(bb.to_device(sc["committed"][None]), bb.to_device(sc["guesses"][None]))
    out = _variants(lambda: be.BatchBackend(p, sc["statics"]), run)
    g = sc["guesses"]
    T = p.T_span
    n_over = 0
    for a in np.flatnonzero((out["flags"] & 0x100) != 0):
        K = int(g[a]["K"]); co = np.array(g[a]["coeff"])
        end = ((T ** 3) * co[:, K - 1, 0] + (T ** 2) * co[:, K - 1, 1] + T * co[:, K - 1, 2]) + co[:, K - 1, 3]
        if np.hypot(co[0, 0, 3] - end[0], co[1, 0, 3] - end[1]) < 1.0:
            n_over += 1
            np.testing.assert_array_equal(np.array(out["sol"][a]["coeff"])[2], co[2])
    print("z motion, %s: %r, certified with the z override %d" % (path, _classes(out), n_over))
    assert n_over >= 1
