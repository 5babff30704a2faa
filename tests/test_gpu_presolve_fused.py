"""GPU: the presolve's zero-iteration certificate in the separator's wave (csrc/qp_presolve.h; separator_packed_kernel's tail)
against the same certificate as a kernel of its own (qp_presolve_kernel).  Every comparison is between two handles on the same
inputs — the default (fused) one and one with the debug option "presolve_fused" = 0 — and asks for ZERO differing bytes in the
solutions (stats.solve_us blanked: a device time), the sampled states, the commit records, the certificate's marks, the line
buckets, and the redo and polish counts.  Small handles get one wave per slot through the separator-pack option (8 segments a
wave); every case proves the path it ran from debug_launch_path()."""
import dataclasses

import numpy as np
import pytest

import helpers  # noqa: F401
from neptune_amd import abi, scene
from neptune_amd import dist as ndist
from gpu_util import COEF_TOL, COST_RTOL

pytestmark = pytest.mark.gpu

# the 2 x 8-agent world that tests/test_gpu_replan_outputs.py describes, built here so that this file stands on its own: two scenes,
# guesses of 8, 3 and 5 segments, 60 state rows per slot (below the 81 samples of K = 8), whole handle and a shard with own != slot
S, N = 2, 8
KS = (8, 3, 5)                                   # agent a replans with KS[a % 3] segments
SHARDS = {"all": (0, 8), "shard": (4, 4)}        # first_local, n_local


@dataclasses.dataclass
class _CappedParams(scene.Params):
    """scene.Params with a states buffer of 60 rows per slot instead of the derived ceil(num_pol T / dc) + 3"""
    max_states = 60


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


@pytest.fixture(scope="module")
def world():
    """-> (params, statics per scene, guesses [S][N], previous records [S][N]); never modified by a case"""
    p = _CappedParams(**dataclasses.asdict(scene.scaled_params(N, 3)))
    scs = [scene.make_scene(N, 3, seed=11 + s, par=p) for s in range(S)]
    gue = np.stack([sc["guesses"] for sc in scs])
    for a in range(N):                           # the first K segments of the 8-segment guess
        K = KS[a % 3]
        gue["K"][:, a] = K
        gue["coeff"][:, a, :, K:, :] = 0.0
    prev = np.stack([sc["committed"] for sc in scs])
    return p, [sc["statics"] for sc in scs], gue, prev


def _handle(be, world, shard):
    p, statics, _, _ = world
    first, nl = SHARDS[shard]
    bb = be.BatchBackend(p, statics[0], first_local=first, n_local=nl, n_scenes=S)
    for s in range(1, S):
        bb.set_scene_statics(s, statics[s])
    return bb


def _infeasible_guess(g, p):
    """start outside the world box: the position rows of the first control point cannot hold in either solve"""
    g = g.copy()
    co = np.array(g["coeff"])
    co[0, :, 3] += (p.x_max + 5.0) - co[0, 0, 3]
    g["coeff"] = co
    return g


def _outputs(bb, lines_of=None):
    """everything a replan left in the handle, as bytes-comparable arrays"""
    sol = bb.solutions().copy()
    sol["stats"]["solve_us"] = 0.0
    out = {"sol": sol, "states": bb.states().copy(), "commit": bb.commits().copy(), "marks": bb.debug_presolved(),
           "redo": np.asarray(bb.redo_count()), "polish": np.asarray(bb.polish_count())}
    for s in (range(bb.slots) if lines_of is None else lines_of):
        seg, nd = bb.debug_lines(int(s))
        out["line_seg_%d" % s] = seg; out["line_nd_%d" % s] = nd
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _close(a, c):
    """against a handle without the certificate ahead of the interior point ("presolve_kernel" = 0): the existing tolerances"""
    sa, sc_ = a["sol"], c["sol"]
    np.testing.assert_array_equal(sa["stats"]["status"], sc_["stats"]["status"])
    np.testing.assert_array_equal(sa["K"], sc_["K"])
    assert np.abs(np.array(sa["coeff"]) - np.array(sc_["coeff"])).max() <= COEF_TOL
    ok = sa["stats"]["status"] != abi.NEP_FAILED
    oa, oc = sa["stats"]["objective"][ok], sc_["stats"]["objective"][ok]
    assert (np.abs(oa - oc) <= COST_RTOL * (1 + np.abs(oc))).all()


def _fused(bb):
    p = bb.debug_launch_path()
    return p["fused_presolve"], p["presolve_kernel"]


def _pair(make, replan, lines_of=None, third=False, pack=8):
    """the same replans on a fused handle and on one with the certificate as its own kernel (and, third, on one without either)
    -> their outputs; the paths are asserted here"""
    outs = []
    for mode in ("fused", "kernel") + (("none",) if third else ()):
        bb = make()
        if pack:
            bb.set_separator_pack(pack)
        if mode == "kernel":
            bb.debug_option("presolve_fused", 0)
        if mode == "none":
            bb.debug_option("presolve_kernel", 0)
        replan(bb)
        assert _fused(bb) == {"fused": (True, True), "kernel": (False, True), "none": (False, False)}[mode], (mode, bb.debug_launch_path())
        outs.append(_outputs(bb, lines_of))
        bb.close()
    _same(outs[0], outs[1])
    if third:
        _close(outs[0], outs[2])
    return outs[0]


# ---- 1. the 2 x 8-agent world of test_gpu_replan_outputs.py ----

def _world_guesses(world):
    p, _, gue, prev = world
    gue = gue.copy()
    gue["K"][0, 2] = 0; gue["coeff"][0, 2] = 0.0                      # a front-end miss
    gue["K"][1, 4] = 0; gue["coeff"][1, 4] = 0.0
    for s, o in ((0, 6), (1, 5)):                                     # failed replans (K = 8 and K = 5, both inside the shard)
        gue[s, o] = _infeasible_guess(gue[s, o], p)
    return gue, prev


@pytest.mark.parametrize("shard", list(SHARDS))
def test_small_world_same_bytes(be, world, shard):
    gue, prev = _world_guesses(world)
    own = np.arange(SHARDS[shard][0], SHARDS[shard][0] + SHARDS[shard][1])

    def replan(bb):
        bb.replan(bb.to_device(prev), bb.to_device(gue[:, own]))
    out = _pair(lambda: _handle(be, world, shard), replan, third=True)
    sol = out["sol"].reshape(S, len(own)); marks = out["marks"].reshape(S, len(own))
    assert set(np.unique(sol["K"])) == {0, 3, 5, 8} and (sol["n_states"][sol["K"] == 8] == 60).all()
    assert (sol["stats"]["status"] == abi.NEP_FAILED).sum() >= 2
    assert marks.sum() >= 1 and (marks[gue["K"][:, own] == 0] == 0).all()
    assert (marks[sol["stats"]["status"] == abi.NEP_FAILED] == 0).all()
    assert (sol["stats"]["iters"][marks == 1] == 0).all()


def test_an_active_set_keeps_the_kernel_of_its_own(be, world):
    """the tail does not serve active sets: such a handle falls back to qp_presolve_kernel"""
    import torch
    gue, prev = _world_guesses(world)
    mask = np.ones((S, N), dtype=np.int32); mask[0, [1, 5]] = 0; mask[1, [7]] = 0
    bb = _handle(be, world, "all")
    bb.set_separator_pack(8)
    bb.set_active(torch.from_numpy(mask).to(bb.device))
    bb.replan(bb.to_device(prev), bb.to_device(gue))
    assert _fused(bb) == (False, True)
    assert (bb.solutions()["stats"]["status"].reshape(S, N)[mask == 0] == abi.NEP_SKIPPED).all()
    bb.close()


# ---- 2. slots that must abstain ----

@pytest.fixture(scope="module")
def small():
    """one 8-agent scene whose every replan certifies as it stands -> (scene, baseline marks are asserted by the case)"""
    return scene.make_scene(8, 3, seed=11)


def test_abstentions_small_scene(be, small):
    sc = small; p = sc["par"]; T = p.T_span
    base = sc["guesses"]

    def make():
        return be.BatchBackend(p, sc["statics"])

    def run(gue, **kw):
        def replan(bb):
            for k, v in kw.items():
                getattr(bb, k)(v)
            bb.replan(bb.to_device(sc["committed"]), bb.to_device(gue))
        return _pair(make, replan, third=True)
    out0 = run(base)
    cert = np.flatnonzero(out0["marks"] == 1)
    assert len(cert) >= 5, out0["marks"]                            # (the unmodified guesses certify: what follows makes them abstain)
    a_k2, a_box, a_ball, a_zov = (int(x) for x in cert[:4])
    gue = base.copy()
    # K = 2
    gue["K"][a_k2] = 2; gue["coeff"][a_k2][:, 2:, :] = 0.0
    # a box row violated at z*: twice the speed limit at the start (z* keeps the guess's start state)
    gue["coeff"][a_box][0, 0, 2] = 2.0 * p.v_max
    # within 1 m of the goal: the guess shrunk toward its start, ending 0.5 m from it — the terminal ball row is posed and z keeps
    # the guess (a_ball) ...
    # ... and within 1 m in x, y only: the same in x, y with a steady climb of 1.2 m in z on top (a_zov: z keeps the guess, no ball)
    def ends(co, K):
        return co[:, 0, 3].copy(), np.array([np.polyval(co[ax, K - 1], T) for ax in range(3)])
    for a, climb in ((a_ball, 0.0), (a_zov, 1.2)):
        co = np.array(gue["coeff"][a]); K = int(gue["K"][a])
        start, end = ends(co, K)
        s_ = 0.5 / np.linalg.norm(end - start)
        for ax in range(3):
            co[ax, :, :3] *= s_; co[ax, :, 3] = start[ax] + s_ * (co[ax, :, 3] - start[ax])
        co[2, :K, 2] += climb / (K * T); co[2, :K, 3] += climb * np.arange(K) / K
        gue["coeff"][a] = co
        start, end = ends(co, K)
        assert np.linalg.norm((end - start)[:2]) < 1.0 and (np.linalg.norm(end - start) < 1.0) == (climb == 0.0)
        assert p.z_min + 0.3 < co[2, 0, 3] and end[2] < p.z_max - 0.3
    out = run(gue)
    sol = out["sol"]
    assert out["marks"][a_k2] == 0 and out["marks"][a_box] == 0
    assert int(sol[a_box]["stats"]["iters"]) > 0 or int(sol[a_box]["stats"]["status"]) == abi.NEP_FAILED     # the interior point decided
    # both stay a short, slow flight inside what the unshrunk guess had certified: z* ends at f (the ball holds with 0.01 to spare),
    # so both certify, with the ball posed or not, and both return the guess's z coefficients (the z-override)
    for a, qc in ((a_ball, 1), (a_zov, 0)):
        K = int(gue["K"][a])
        assert out["marks"][a] == 1 and int(sol[a]["stats"]["iters"]) == 0 and int(sol[a]["stats"]["status"]) == abi.NEP_OK, a
        assert int(sol[a]["stats"]["qc_active"]) == qc, a
        assert np.array(sol[a]["coeff"])[2, :K].tobytes() == np.array(gue["coeff"][a])[2, :K].tobytes(), a
        assert np.array(sol[a]["coeff"])[:2, :K].tobytes() != np.array(gue["coeff"][a])[:2, :K].tobytes(), a      # (x, y are z*'s, not the guess's)
    untouched = [int(x) for x in cert[4:]]
    assert (out["marks"][untouched] == 1).all()
    # a cull radius of 0.05 m: the movement bound fails wherever a line was parked or an LP skipped
    out_r = run(base, set_line_cull=0.05)
    lines = out0["sol"]["stats"]["n_lines"]
    assert out_r["marks"].sum() < out0["marks"].sum() and (out_r["marks"][lines == 0] == out0["marks"][lines == 0]).all()


# ---- 3. 4 scenes x 64 agents + 20 obstacles ----

S3, N3 = 4, 64


@pytest.fixture(scope="module")
def big():
    scs = [scene.make_scene(N3, 20, seed=200 + s) for s in range(S3)]
    com, gue = ndist.stack_scenes(scs)
    return scs, np.ascontiguousarray(com), np.ascontiguousarray(gue)


def _big_handle(be, big, tiles=1):
    scs = big[0]
    bb = be.BatchBackend(scs[0]["par"], scs[0]["statics"], n_scenes=S3 * tiles)
    for s in range(S3 * tiles):
        bb.set_scene_statics(s, scs[s % S3]["statics"])
    return bb


def test_256_slots_two_replans(be, big):
    scs, com, gue = big
    p = scs[0]["par"]

    def replan(bb):
        d_com, d_gue = bb.to_device(com), bb.to_device(gue)
        bb.replan(d_com, d_gue)
        bb.replan(d_com, d_gue)                                       # (the second is launch-ordered by the first one's keys where the handle orders)
    out = _pair(lambda: _big_handle(be, big), replan, third=True)
    sol, marks = out["sol"], out["marks"]
    st = sol["stats"]
    print("certified %d of %d, iterating %d, certified with failed LPs %d" % (marks.sum(), len(marks), ((marks == 0) & (st["iters"] > 0)).sum(),
                                                                           ((marks == 1) & (st["n_lp_failed"] > 0)).sum()))
    assert marks.sum() > len(marks) // 2 and ((marks == 0) & (st["iters"] > 0)).sum() >= 1
    assert (st["iters"][marks == 1] == 0).all() and (st["status"][marks == 1] == abi.NEP_OK).all()
    # a replan with failed LPs that still certifies: the counts as the kernel of its own writes them (_same above), and consistent
    lpf = np.flatnonzero((marks == 1) & (st["n_lp_failed"] > 0))
    assert len(lpf) >= 1
    for a in lpf:
        assert int(st["n_lines"][a]) >= 0 and int(st["n_rows"][a]) >= 48 * int(sol["K"][a]) and int(st["n_lp"][a]) >= int(st["n_lines"][a]) + int(st["n_lp_failed"][a])
    # a slot whose z* crosses a near line: z* (what the same guess returns in an empty world, where it certifies) stays within the cull
    # radius of the guess, satisfies the box rows there, and is on the wrong side of one of the slot's lines
    M4 = scene.A_POS_INV * np.array([p.T_span ** 3, p.T_span ** 2, p.T_span, 1.0])[:, None]
    far_com = com.copy(); far_com["pwp"]["coeff"][..., 0, :, 3] += 1.0e4; far_com["pos"][..., 0] += 1.0e4
    found = 0
    for a in np.flatnonzero((marks == 0) & (st["iters"] > 0) & (st["status"] == abi.NEP_OK))[:8]:
        s, o = divmod(int(a), N3)
        be1 = be.BatchBackend(p, [], first_local=o, n_local=1)
        be1.set_separator_pack(8)
        be1.replan(be1.to_device(far_com[s]), be1.to_device(gue[s, o:o + 1]))
        if int(be1.debug_presolved()[0]) == 1:
            z = np.array(be1.solutions()[0]["coeff"]); K = int(gue[s, o]["K"]); g = np.array(gue[s, o]["coeff"])
            qz = np.einsum("xkj,jc->xkc", z[:2, :K], M4); qg = np.einsum("xkj,jc->xkc", g[:2, :K], M4)      # [axis][segment][control point]
            moved = np.sqrt(((qz - qg) ** 2).sum(axis=0)).max()
            seg, nd = out["line_seg_%d" % a], out["line_nd_%d" % a]
            worst = max((nd[i, 0] * qz[0, seg[i]] + nd[i, 1] * qz[1, seg[i]] + nd[i, 2] - 1.0).max() for i in range(len(seg))) if len(seg) else -1.0
            if moved < 4.0 and worst > 0.0:
                found += 1
        be1.close()
    assert found >= 1


def test_overflowed_buckets_abstain(be, big):
    """buckets of eight lines under a cull radius of 30 m (hardly an LP is skipped, so a segment gets dozens of lines): the
    segments overflow (NEP_FLAG_LINES), those replans fail, the certificate abstains"""
    from neptune_amd._lib import BackendError
    scs, com, gue = big

    def replan(bb):
        bb.set_line_cull(30.0)
        bb.set_line_capacity(8)
        bb.replan(bb.to_device(com), bb.to_device(gue))
        with pytest.raises(BackendError):
            bb.check()
    out = _pair(lambda: _big_handle(be, big), replan, lines_of=range(0, S3 * N3, 8))
    failed = out["sol"]["stats"]["status"] == abi.NEP_FAILED
    assert failed.sum() >= 1 and (out["marks"][failed] == 0).all()


# ---- 4. automatic selection ----

def test_automatic_selection_at_4096_slots(be, big):
    scs, com, gue = big
    tiles = 16
    com_t, gue_t = np.ascontiguousarray(np.tile(com, (tiles, 1))), np.ascontiguousarray(np.tile(gue, (tiles, 1)))

    def replan(bb):
        bb.replan(bb.to_device(com_t), bb.to_device(gue_t))
        assert bb.debug_launch_path()["fused_boxes"]
    out = _pair(lambda: _big_handle(be, big, tiles), replan, lines_of=range(0, S3 * N3 * tiles, 61), pack=0)
    marks = out["marks"].reshape(tiles, S3 * N3)
    assert (marks == marks[0]).all() and marks[0].sum() > S3 * N3 // 2
    sol = out["sol"].reshape(tiles, S3 * N3)
    assert all(sol[t].tobytes() == sol[0].tobytes() for t in range(tiles))
    bb = _big_handle(be, big, tiles // 2)                             # 2 048 slots: four segments a wave, the kernel of its own
    bb.replan(bb.to_device(com_t[:S3 * tiles // 2]), bb.to_device(gue_t[:S3 * tiles // 2]))
    assert _fused(bb) == (False, True)
    bb.close()


# ---- 5. stale marks ----

def test_graph_replay_never_reads_a_stale_mark(be, big):
    import torch
    scs, com, gue = big
    p = scs[0]["par"]
    # two sets of guesses: B swaps in, for a few slots, what makes a certified slot iterate (twice the speed limit at the start)
    ref = _big_handle(be, big); ref.set_separator_pack(8)
    d_com = ref.to_device(com)
    ref.replan(d_com, ref.to_device(gue)); m_a = ref.debug_presolved()
    cert = np.flatnonzero(m_a == 1)[:6]
    gue_b = gue.copy().reshape(-1)
    for a in cert:
        gue_b[a]["coeff"][0, 0, 2] = 2.0 * p.v_max
    gue_b = gue_b.reshape(gue.shape)
    eager = []
    for g in (gue, gue_b, gue):
        ref.replan(d_com, ref.to_device(g)); eager.append(_outputs(ref, lines_of=cert))
    assert _fused(ref) == (True, True)
    assert (eager[0]["marks"][cert] == 1).all() and (eager[1]["marks"][cert] == 0).all()
    ref.close()
    bb = _big_handle(be, big); bb.set_separator_pack(8)
    d_com = bb.to_device(com); d_g = bb.to_device(gue)
    s_ = torch.cuda.Stream(bb.device)
    s_.wait_stream(torch.cuda.current_stream(bb.device))
    with torch.cuda.stream(s_):
        bb.replan(d_com, d_g)
    torch.cuda.current_stream(bb.device).wait_stream(s_)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        bb.replan(d_com, d_g)
    assert _fused(bb) == (True, True)
    for g, want in zip((gue, gue_b, gue), eager):                     # certified -> iterates -> certified again, and the reverse in between
        d_g.copy_(bb.to_device(g))
        gr.replay()
        torch.cuda.synchronize()
        _same(_outputs(bb, lines_of=cert), want)
    del gr
    bb.close()
