"""GPU: the default replan path at short guesses and num_pol < 8, held to the oracle.  The inputs are tests/short_guess_worlds.py's
(8 agents, num_pol D in 5..8, every slot of a scene with a guess length K of its own, K = 0 and infeasible slots, entangle cases;
test_short_guess_worlds_cpu.py fixes by the oracle alone that they are not vacuous).  Small handles reach the large-launch forms of
the separator through the separator-pack hook (-1 the unpacked kernel, 1..8 segments of a slot per wave; at 8 the zero-iteration
certificate runs in the separator's wave).

  A  every slot against the oracle by gpu_util._check_scene's rules, on the every-row path and on the default path, at every pack
  B  the packed separator against the unpacked one on the same handle, byte for byte
  C  the certificate at every K and D: in the separator's wave == as a kernel of its own (bytes), against no certificate (tolerance),
     against the oracle; which slots it marks
  D  K changing under a live handle, eager and as a replayed graph, against fresh handles (bytes); active sets

The pack itself is not among the launch path's bits: a case proves from debug_launch_path() / qp_kernel_name() the solve path, that
the spatial presolve is on (box_kernel: the condition under which a pack >= 0 takes the packed kernel, launch_plan.h) and, at pack 8,
the certificate's place (fused_presolve is only ever set with eight segments a wave).  Tolerances: gpu_util's, nothing new.

What of separator_packed_kernel each part holds in place (argued from the assertions, not by running broken kernels):
  the clamp of seg_end to num_pol   B's +overlong world: a slot with K = num_pol + 1.  Without the clamp the packed kernel would solve
      LPs for segment num_pol (at D < 8) and store their counts; the unpacked kernel returns zero counts for it (seg >= sp.num_pol), so
      the slot's stats.n_lp in the solution bytes and its line buckets differ between pack >= 1 and pack -1.
  the zeroing of sCnt for absent segments   the wave stores line_cnt, line_far, line_skip and lp_stats of EVERY segment of its group
      from sCnt.  Unzeroed entries of segments >= K are what the last wave left in LDS: debug_lines (which reads all eight buckets)
      would return lines in segments >= K, which A refuses on both paths (not the oracle's lines), B refuses against the unpacked
      kernel and D against a fresh handle; a K = 0 slot would report n_lp != 0 (check_replanned_handle asserts zeros).
  the unconditional write of presolved[slot]   D: round 1 marks full-length slots, round 2 gives some of them K < 3, K = 0 or an
      infeasible guess (asserted: at least one marked slot gets K < 3).  A mark left standing makes qp_reg_kernel return at once for
      the slot: its solution, states and record are round 1's, the marks differ from the fresh handle's, and
      marks[K < 3] == 0 fails — eager and replayed.
  pre_tables + K   C: a certified slot's coefficients ARE table K's minimiser.  With another K's table every marked slot with K < D
      misses the oracle's coefficients (COEF_TOL), and C asserts that every K in 3..D has a marked slot; the kernel of its own
      (tables + K on its side) would differ in bytes as well.
The cases print the worst device-vs-oracle coefficient error and the certificate's counts per K (pytest -s)."""
import numpy as np
import pytest

import helpers  # noqa: F401
import short_guess_worlds as W
from neptune_amd import abi
from gpu_util import check_replanned_handle
from test_gpu_presolve_fused import _outputs, _same, _close, _fused

pytestmark = pytest.mark.gpu

PACKS = {"default": (-1, 1, 2, 3, 4, 8), "every_row": (-1, 1, 2, 4, 8)}
ENT_PACKS = (-1, 2, 8)
B_PACKS = (1, 2, 3, 4, 5, 8)
KINDS = ("truncated", "truncated+misses", "at_rest", "at_rest+misses")
ENT_KINDS = ("truncated+ent", "at_rest+ent")

_REFS = {}          # world name -> the oracle's results, computed once and never modified


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


def _worlds(kind, D, shift=0, flip=0):
    """the scenes of one handle: the kind's world at each of its seeds for D; +misses: K = 0 and infeasible slots (placement
    (scene + flip) % 2), +overlong, +ent"""
    name, *mods = kind.split("+")
    seeds = (W.TRUNCATED_SEEDS if name == "truncated" else W.AT_REST_SEEDS)[D]
    ws = [(W.truncated if name == "truncated" else W.at_rest)(D, s, shift) for s in seeds]
    if "misses" in mods:
        ws = [W.with_misses(w, (k + flip) % 2) for k, w in enumerate(ws)]
    if "overlong" in mods:
        ws = [W.with_overlong(w) for w in ws]
    if "ent" in mods:
        ws = [W.with_entangle(w, W.ent_seed(s)) for w, s in zip(ws, seeds)]
    return ws


def _refs(oracle, worlds):
    for w in worlds:
        if w["name"] not in _REFS:
            _REFS[w["name"]] = W.oracle_results(oracle, w)
    return [_REFS[w["name"]] for w in worlds]


def _handle(be, worlds):
    """-> (handle, guesses [S][N], committed [S][N], entangle cases on the device or None)"""
    p, statics, gue, com, case = W.stack(worlds)
    bb = be.BatchBackend(p, statics[0], n_scenes=len(worlds))
    for s in range(1, len(worlds)):
        bb.set_scene_statics(s, statics[s])
    d_ent = bb.torch.from_numpy(case.reshape(-1)).to(bb.device) if case is not None else None
    return bb, gue, com, d_ent


def _assert_path(bb, path, pack, active=False):
    lp = bb.debug_launch_path()
    assert bb.qp_kernel_name() == "qp_reg_kernel"
    if path == "every_row":
        assert bb.line_cull() == 0.0 and not (lp["presolve_kernel"] or lp["fused_presolve"] or lp["box_kernel"] or lp["redo_pass"]), lp
    else:
        assert bb.line_cull() == 4.0 and lp["box_kernel"] and lp["redo_pass"] and lp["presolve_kernel"], lp
        assert lp["fused_presolve"] == (pack == 8 and not active), (pack, lp)
    assert not (lp["grouped_hulls"] or lp["fused_boxes"] or lp["ordered_qp"]), lp


# ---- A. against the oracle, per slot ----

def _against_the_oracle(be, oracle, worlds, path, packs):
    refs = _refs(oracle, worlds)
    bb, gue, com, d_ent = _handle(be, worlds)
    if path == "every_row":
        bb.set_line_cull(0.0)
    d_com, d_gue = bb.to_device(com), bb.to_device(gue)
    worst = 0.0
    for pack in packs:
        bb.set_separator_pack(pack)
        bb.replan(d_com, d_gue, d_ent=d_ent)
        _assert_path(bb, path, pack)
        worst = max(worst, check_replanned_handle(oracle, bb, gue, com, refs))
    bb.close()
    st = [r["status"] for rs in refs for r in rs if r is not None]
    print("%-40s %-9s packs %r: worst |device - oracle| %.2e   (oracle: %d OK, %d RELAXED, %d FAILED, %d without a guess)" %
          (" / ".join(w["name"] for w in worlds[:1]), path, packs, worst, st.count(0), st.count(1), st.count(2), sum(r is None for rs in refs for r in rs)))
    return worst


@pytest.mark.parametrize("path", list(PACKS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", W.DS)
def test_against_the_oracle(be, oracle, D, kind, path):
    _against_the_oracle(be, oracle, _worlds(kind, D), path, PACKS[path])


@pytest.mark.parametrize("path", list(PACKS))
@pytest.mark.parametrize("kind", ENT_KINDS)
@pytest.mark.parametrize("D", W.ENT_DS)
def test_against_the_oracle_with_entangle_rows(be, oracle, D, kind, path):
    """entangle candidates: the packed kernel keeps its ballots in LDS rather than in lanes"""
    worlds = _worlds(kind, D)
    assert all(w["par"].enable_entangle and w["case"].any() for w in worlds)
    _against_the_oracle(be, oracle, worlds, path, ENT_PACKS)


# ---- B. packed against unpacked on the same handle ----

@pytest.mark.parametrize("D,kind", [(D, k) for D in W.DS for k in KINDS + ("truncated+overlong",)] + [(D, k) for D in W.ENT_DS for k in ENT_KINDS])
def test_packed_separator_gives_the_unpacked_kernels_lines_at_short_guesses(be, D, kind):
    """test_gpu_parity.test_packed_separator_gives_the_unpacked_kernels_lines on these worlds: solutions, redo count and both arrays
    of every slot's line buckets, packs 1, 2, 3, 4, 5 and 8 against the unpacked kernel, under the default cull radius and with
    every row (where a forced pack runs the packed kernel too).  +overlong: a slot with K = num_pol + 1 — the packed kernel must stop
    at the handle's num_pol as the unpacked one does"""
    worlds = _worlds(kind, D)
    bb, gue, com, d_ent = _handle(be, worlds)
    d_com, d_gue = bb.to_device(com), bb.to_device(gue)
    for path in ("default", "every_row"):
        if path == "every_row":
            bb.set_line_cull(0.0)

        def run(pack):
            bb.set_separator_pack(pack)
            bb.replan(d_com, d_gue, d_ent=d_ent)
            _assert_path(bb, path, pack)
            return bb.solutions().copy(), [bb.debug_lines(a, cap=4096) for a in range(bb.slots)], bb.redo_count()
        ref_sol, ref_lines, ref_redo = run(-1)
        assert int(ref_sol["stats"]["n_lines"].sum()) > 0
        if "overlong" in kind:
            over = ref_sol.reshape(len(worlds), W.N)[:, D - 1]
            assert (over["stats"]["status"] == abi.NEP_FAILED).all() and (over["K"] == 0).all() and (over["stats"]["n_lp"] > 0).all()
            for s in range(len(worlds)):
                seg = ref_lines[s * W.N + D - 1][0]
                assert len(seg) > 0 and seg.max() < D
        for pack in B_PACKS:
            sol, lines, redo = run(pack)
            assert sol.tobytes() == ref_sol.tobytes(), (path, pack, np.flatnonzero([sol[a].tobytes() != ref_sol[a].tobytes() for a in range(bb.slots)]))
            assert redo == ref_redo, (path, pack)
            for a in range(bb.slots):
                np.testing.assert_array_equal(lines[a][0], ref_lines[a][0], err_msg="%s pack %s slot %d" % (path, pack, a))
                np.testing.assert_array_equal(lines[a][1], ref_lines[a][1], err_msg="%s pack %s slot %d" % (path, pack, a))
    bb.close()


# ---- C. the certificate at every K and D ----

@pytest.mark.parametrize("D", W.DS)
def test_certificate_at_every_length(be, oracle, D):
    """at_rest(D) and its K = 0 / infeasible variant as the four scenes of one handle, the three-handle comparison of
    test_gpu_presolve_fused._pair: the certificate in the separator's wave (pack 8) == as a kernel of its own, zero differing bytes;
    against a handle without it, the tolerances; the fused handle against the oracle.  The marks: a marked slot has status OK and no
    iteration; K < 3, K = 0 and failed slots are never marked; and every K in 3..D has a marked slot — the oracle says these optima
    touch no row (test_short_guess_worlds_cpu.py), whether the movement bound accepts is the device's to say."""
    worlds = _worlds("at_rest", D) + _worlds("at_rest+misses", D)
    refs = _refs(oracle, worlds)
    outs = []
    for mode in ("fused", "kernel", "none"):
        bb, gue, com, _ = _handle(be, worlds)
        bb.set_separator_pack(8)
        if mode == "kernel":
            bb.debug_option("presolve_fused", 0)
        if mode == "none":
            bb.debug_option("presolve_kernel", 0)
        bb.replan(bb.to_device(com), bb.to_device(gue))
        assert _fused(bb) == {"fused": (True, True), "kernel": (False, True), "none": (False, False)}[mode], (mode, bb.debug_launch_path())
        if mode == "fused":
            _assert_path(bb, "default", 8)
            worst = check_replanned_handle(oracle, bb, gue, com, refs)
        outs.append(_outputs(bb))
        bb.close()
    _same(outs[0], outs[1])
    _close(outs[0], outs[2])
    sol, marks = outs[0]["sol"], outs[0]["marks"]
    K = gue["K"].reshape(-1); st = sol["stats"]
    assert set(np.unique(marks)) <= {0, 1}
    assert (st["iters"][marks == 1] == 0).all() and (st["status"][marks == 1] == abi.NEP_OK).all()
    assert (marks[K < 3] == 0).all() and (marks[st["status"] == abi.NEP_FAILED] == 0).all()
    assert (K == 0).sum() == 4 and (st["status"][K > 0] == abi.NEP_FAILED).sum() >= 2
    per_k = {k: (int(marks[K == k].sum()), int((K == k).sum())) for k in range(0, D + 1)}
    print("at_rest D%d certificate: marked / slots per K %r, worst |device - oracle| %.2e" % (D, per_k, worst))
    assert {k for k in per_k if per_k[k][0] > 0} == set(range(3, D + 1)), per_k


# ---- D. K changing under a live handle ----

def _rounds(D):
    """three rounds on the same committed records and statics: every slot at K = D; the mixed world with K = 0 and infeasible slots;
    the mixed world with the K assignment rotated by 3 agents and the other placement of the K = 0 / infeasible slots"""
    seeds = W.AT_REST_SEEDS[D]
    return [[W.full_length(D, s) for s in seeds], _worlds("at_rest+misses", D), _worlds("at_rest+misses", D, shift=3, flip=1)]


def _prepared(be, worlds, pack):
    bb, gue, com, _ = _handle(be, worlds)
    bb.set_separator_pack(pack)
    return bb, gue, com


@pytest.mark.parametrize("pack", (8, 2))
@pytest.mark.parametrize("D", W.DS)
def test_lengths_change_under_a_live_handle(be, D, pack):
    """after each round every output of the live handle (solutions, states, commits, marks, redo and polish counts, every slot's line
    buckets) equals, byte for byte, a fresh handle's on that round's inputs alone: stale per-segment counts, far / skip counts or
    marks of segments >= K would show.  Then the same rounds as a replayed graph, the guesses overwritten in place.
    (The states buffer is the caller's and a replan writes n_states rows per slot of it, nothing behind them: it is zeroed before
    each round, as a fresh handle's is.  The solution and commit buffers are not: every byte of them is rewritten.)"""
    import torch
    rounds = _rounds(D)
    coms = [W.stack(ws)[3] for ws in rounds]
    assert all(c.tobytes() == coms[0].tobytes() for c in coms)
    live, _, com = _prepared(be, rounds[0], pack)
    d_com = live.to_device(com)
    eager = []
    for ws in rounds:
        gue = W.stack(ws)[2]
        live.d_states.zero_()
        live.replan(d_com, live.to_device(gue))
        _assert_path(live, "default", pack)
        eager.append(_outputs(live))
        fresh, _, _ = _prepared(be, ws, pack)
        fresh.replan(fresh.to_device(com), fresh.to_device(gue))
        _assert_path(fresh, "default", pack)
        _same(eager[-1], _outputs(fresh))
        fresh.close()
    live.close()
    k1, k2 = W.stack(rounds[1])[2]["K"].reshape(-1), W.stack(rounds[2])[2]["K"].reshape(-1)
    assert eager[0]["marks"].sum() >= 2 and (eager[1]["marks"][k1 < 3] == 0).all() and (eager[2]["marks"][k2 < 3] == 0).all()
    assert ((eager[0]["marks"] == 1) & (k1 < 3)).sum() >= 1          # (a slot marked in round 1 has to lose its mark in round 2)
    assert ((k1 == 0) & (k2 > 0)).sum() >= 2 and ((k1 > 0) & (k2 == 0)).sum() >= 2
    # the same rounds as a captured replan (captured the way test_graph_replay_never_reads_a_stale_mark captures)
    bb, gue0, _ = _prepared(be, rounds[0], pack)
    d_com = bb.to_device(com); d_g = bb.to_device(gue0)
    s_ = torch.cuda.Stream(bb.device)
    s_.wait_stream(torch.cuda.current_stream(bb.device))
    with torch.cuda.stream(s_):
        bb.replan(d_com, d_g)
    torch.cuda.current_stream(bb.device).wait_stream(s_)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        bb.replan(d_com, d_g)
    _assert_path(bb, "default", pack)
    for ws, want in zip(rounds, eager):
        d_g.copy_(bb.to_device(W.stack(ws)[2]))
        bb.d_states.zero_()
        gr.replay()
        torch.cuda.synchronize()
        _same(_outputs(bb), want)
    del gr
    bb.close()


@pytest.mark.parametrize("kind", ("truncated+misses", "at_rest+misses"))
@pytest.mark.parametrize("D", W.DS)
def test_active_sets_on_mixed_lengths(be, oracle, D, kind):
    """an active set on the mixed worlds at 2 and 8 segments a wave: the inactive slots are NEP_SKIPPED and keep their records,
    the active ones pass part A's check (with an active set the certificate is a kernel of its own at every pack)"""
    import torch
    worlds = _worlds(kind, D)
    refs = _refs(oracle, worlds)
    bb, gue, com, _ = _handle(be, worlds)
    mask = np.ones((len(worlds), W.N), dtype=np.int32)
    mask[0, [1, 5]] = 0; mask[1, [2, D - 1]] = 0          # (short and long guesses; the K = 0 and infeasible slots stay active)
    bb.set_active(torch.from_numpy(mask).to(bb.device))
    d_com, d_gue = bb.to_device(com), bb.to_device(gue)
    for pack in (2, 8):
        bb.set_separator_pack(pack)
        bb.replan(d_com, d_gue)
        _assert_path(bb, "default", pack, active=True)
        check_replanned_handle(oracle, bb, gue, com, refs, mask=mask)
        st = bb.solutions()["stats"]["status"].reshape(mask.shape)
        np.testing.assert_array_equal(st == abi.NEP_SKIPPED, mask == 0)
        assert bb.commits().reshape(mask.shape)[mask == 0].tobytes() == com[mask == 0].tobytes()
        for slot in np.flatnonzero(mask.reshape(-1) == 0):      # (no separator has ever written these slots' counts: the reader keeps to the bucket whatever they hold)
            seg, nd = bb.debug_lines(int(slot))
            assert len(seg) == len(nd) and (len(seg) == 0 or (0 <= seg.min() and seg.max() < abi.NEP_MAX_POL))
    bb.close()
