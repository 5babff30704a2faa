"""GPU: the eight-hulls-per-wave hull kernel (hull_group_kernel), where its LDS indexing and its chain walk can go wrong.  Every
case forces the kernel (set_hull_kernel(2)) on a handful of committed trajectories made for one such place — a full point area,
groups of different sizes in one wave, long runs of pops, degenerate points, no inflation, both group_hull instantiations,
inactive groups, the order block in the same LDS — and compares vertex counts and vertices BIT FOR BIT with the oracle's
hull_of_interval and with the one-hull-per-wave kernel on the same inputs."""
import dataclasses

import numpy as np
import pytest

import param_sets as PS
from neptune_amd import abi, scene

pytestmark = pytest.mark.gpu

T = 0.5
A_POS = np.linalg.inv(scene.A_POS_INV)          # control points -> coefficients (the kernel goes the other way: V = (P C) A^-1)


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


# ---- committed trajectories made to order ------------------------------------------------------------------------------------

def _coeff_of_ctrl(V, dt):
    """[4][2] control points of a segment of length dt -> coeff[2][4] (up to rounding: the tests compare device and oracle, both of
    which start from the coefficients)"""
    return ((A_POS.T @ np.asarray(V, dtype=np.float64)) / np.array([dt ** 3, dt ** 2, dt, 1.0])[:, None]).T


def _record(base, knots, coeff_xy, bbox=1.2):
    """`base` (a scene's record: id, bend points) with the knots and the x, y coefficients [2][n][4] given"""
    r = base.copy()
    n = len(knots) - 1
    assert 1 <= n <= abi.NEP_TRAJ_MAX_SEG and np.shape(coeff_xy) == (2, n, 4)
    r["bbox"] = bbox
    r["pwp"]["n_seg"] = n
    r["pwp"]["times"][:] = 0.0
    r["pwp"]["times"][: n + 1] = knots
    r["pwp"]["coeff"][:] = 0.0
    r["pwp"]["coeff"][:2, :n, :] = coeff_xy
    r["pwp"]["coeff"][2, :n, 3] = 1.0
    return r


def _random_coeff(rng, n):
    return rng.normal(size=(2, n, 4)) * np.array([0.05, 0.1, 0.5, 3.0])


def _n_overlapped(knots, t0, t1):
    """segments the kernels take for [t0, t1] (neptune.cpp:379-389: lower_bound / upper_bound on the knots)"""
    k = np.asarray(knots); n = len(k) - 1
    first = min(max(int((k < t0).sum()) - 1, 0), n - 1)
    last = min(max(int((k <= t1).sum()) - 1, 0), n - 1)
    return max(last - first + 1, 0)


def _ctrl_record(base, pts, bbox):
    """a record whose interval 0 holds the control points `pts` [4 n][2] (n <= 4 segments of 0.1 s, all inside [0, 0.5])"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 4, 2)
    n = len(pts)
    knots = [0.1 * k for k in range(n)] + [0.5]
    dts = np.diff(knots)
    co = np.stack([_coeff_of_ctrl(pts[s], dts[s]) for s in range(n)], axis=1)
    return _record(base, knots, co, bbox)


# ---- device against oracle -----------------------------------------------------------------------------------------------------

def _device_hulls(be, p, statics, com, gue, mode):
    """hulls of every scene after one replan of a handle with hull kernel `mode` -> [(hx, hn)] per scene"""
    com = np.asarray(com); gue = np.asarray(gue)
    if com.ndim == 1:
        com, gue = com[None], gue[None]
    bb = be.BatchBackend(p, statics, n_scenes=len(com))
    bb.set_hull_kernel(mode)
    bb.replan(bb.to_device(com), bb.to_device(gue))
    path = bb.debug_launch_path()
    assert path["grouped_hulls"] == (mode == 2), (mode, path)
    out = [bb.debug_hulls(s) for s in range(len(com))]
    bb.close()
    return out


def _oracle_hulls(oracle, p, com, t0):
    """[(vertices, overflow)] per (record, interval): what hull_of_interval gives, nothing for a record that makes no hulls"""
    want = []
    for r in com:
        row = []
        makes = int(r["valid"]) and int(r["is_agent"]) and int(r["pwp"]["n_seg"]) > 0
        pw = abi.nep_pwp.from_buffer_copy(r["pwp"].tobytes())
        d = np.array([r["bbox"][0] / 2 + p.drone_radius, r["bbox"][1] / 2 + p.drone_radius])
        for i in range(p.num_pol):
            if not makes:
                row.append((np.zeros((0, 2)), False))
            else:
                h, _h0, ov = oracle.hull_of_interval(pw, t0 + i * p.T_span, t0 + (i + 1) * p.T_span, p.T_span, d, with_overflow=True)
                row.append((h, ov))
        want.append(row)
    return want


def _check(be, oracle, p, statics, com, gue, min_vertices=3):
    """one scene or several ([S][N] records): the grouped kernel == the oracle == the one-hull-per-wave kernel, bit for bit"""
    com = np.asarray(com); gue = np.asarray(gue)
    if com.ndim == 1:
        com, gue = com[None], gue[None]
    got2 = _device_hulls(be, p, statics, com, gue, 2)
    got1 = _device_hulls(be, p, statics, com, gue, 1)
    most = 0
    for s in range(len(com)):
        want = _oracle_hulls(oracle, p, com[s], float(gue[s][0]["t_start"]))
        (hx2, hn2), (hx1, hn1) = got2[s], got1[s]
        np.testing.assert_array_equal(hn2, hn1)
        for j in range(len(com[s])):
            for i in range(p.num_pol):
                h, ov = want[j][i]
                assert not ov, ("the case's input overflows a hull", s, j, i)
                assert hn2[j, i] == len(h), (s, j, i, hn2[j, i], len(h))
                assert hx2[j, i, :len(h)].tobytes() == h.tobytes(), (s, j, i)
                assert hx2[j, i, :len(h)].tobytes() == hx1[j, i, :len(h)].tobytes(), (s, j, i)
                most = max(most, len(h))
    assert most >= min_vertices
    return got2


def _base(N=4, M=1, seed=3, **kw):
    sc = scene.make_scene(N, M, seed=seed, **kw)
    return sc, sc["par"], sc["committed"].copy(), sc["guesses"].copy()


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def test_full_point_area(be, oracle):
    """Knots every T / 2 from -T / 2 on (and from +T / 2 on): an interval overlaps the segment before it, two inside and the one
    after — four segments, 64 inflated points, in groups 0-6 of the first record and 1-7 of the second: every position of every
    group's point area is used."""
    sc, p, com, gue = _base(4)
    rng = np.random.default_rng(11)
    for j, start in enumerate((-0.25, 0.25, -0.25, 0.25)):
        knots = start + 0.25 * np.arange(17)
        com[j] = _record(com[j], knots, _random_coeff(rng, 16))
        full = [i for i in range(8) if _n_overlapped(knots, i * T, (i + 1) * T) == 4]
        assert full == (list(range(7)) if start < 0 else list(range(1, 8)))
    _check(be, oracle, p, sc["statics"], com, gue, min_vertices=6)


def test_groups_of_different_sizes_in_one_wave(be, oracle):
    """Irregular knots: the eight intervals of one trajectory overlap 1, 2, 3 and 4 segments side by side, so the chain lanes of one
    wave walk 16, 32, 48 and 64 points and leave the chain loop at different trips."""
    sc, p, com, gue = _base(6, t_jitter=0.3)
    rng = np.random.default_rng(12)
    t0 = float(gue[0]["t_start"])
    seen = set()
    for j in range(6):
        while True:
            knots = t0 + np.concatenate([[0.0], np.cumsum(rng.choice([0.13, 0.21, 0.34, 0.55, 0.8], size=16))]) - rng.uniform(0, 0.2)
            ns = [_n_overlapped(knots, t0 + i * T, t0 + (i + 1) * T) for i in range(8)]
            if max(ns) <= 4 and len(set(ns)) >= 3:
                break
        seen |= set(ns)
        com[j] = _record(com[j], knots, _random_coeff(rng, 16))
    assert seen == {1, 2, 3, 4}
    _check(be, oracle, p, sc["statics"], com, gue, min_vertices=6)


def _arc_and_far_point(sign):
    """15 control points on a convex arc, ascending in x, and one far point below and beyond them: the lower chain keeps all
    fifteen until the far point pops thirteen in one run.  sign = -1: the same turned by 180 degrees — the upper chain's run."""
    x = 0.1 * np.arange(15)
    pts = np.concatenate([np.stack([x, 0.05 * x * x], axis=1), [[3.0, -5.0]]])
    return sign * pts


@pytest.mark.parametrize("sign", [1, -1], ids=["lower_chain", "upper_chain"])
def test_long_pop_runs(be, oracle, sign):
    """without inflation (the sixteen points themselves) and with two box sizes (64 points: the corners' arcs pop in runs too)"""
    sc, p, com, gue = _base(4)
    p = dataclasses.replace(p, drone_radius=0.0)
    pts = _arc_and_far_point(sign)
    for j, bbox in enumerate((0.0, 0.002, 0.02, 1.2)):
        com[j] = _ctrl_record(com[j], pts, bbox)
    _check(be, oracle, p, sc["statics"], com, gue, min_vertices=4)


def test_degenerate_input(be, oracle):
    """a straight trajectory (every control point on one line), a zero-length last segment (its control points are the end point
    times 1, 1, 1 - 4e-16, 1 - 7e-16: a cluster within ulps), and identical control points (two segments with the same
    coefficients; a trajectory at rest), inflated and not"""
    sc, p, com, gue = _base(8)
    p = dataclasses.replace(p, drone_radius=0.0)
    rng = np.random.default_rng(13)
    knots = 0.25 * np.arange(17) - 0.25
    line = np.zeros((2, 16, 4)); line[0, :, 2] = 0.7; line[1, :, 2] = -0.35
    line[0, :, 3] = 1.0 + 0.7 * 0.25 * np.arange(16); line[1, :, 3] = 2.0 - 0.35 * 0.25 * np.arange(16)
    co = _random_coeff(rng, 8)
    zero_last = np.concatenate([0.5 * np.arange(8), [3.5]])                    # (the last of the eight segments has no length)
    twice = _random_coeff(rng, 16); twice[:, 1::2] = twice[:, 0::2]           # segments 2 k and 2 k + 1: the same coefficients
    rest = np.zeros((2, 16, 4)); rest[0, :, 3] = 1.7; rest[1, :, 3] = -2.3
    for j, (kn, c) in enumerate(((knots, line), (zero_last, co), (knots, twice), (knots, rest))):
        com[j] = _record(com[j], kn, c, bbox=1.2)
        com[j + 4] = _record(com[j + 4], kn, c, bbox=0.0)
    _check(be, oracle, p, sc["statics"], com, gue, min_vertices=4)


def test_no_inflation(be, oracle):
    """bbox = 0 and drone_radius = 0: the hull of the control points themselves (np = np0), up to sixteen points a group"""
    sc, p, com, gue = _base(4)
    p = dataclasses.replace(p, drone_radius=0.0)
    rng = np.random.default_rng(14)
    for j, start in enumerate((-0.25, 0.25, 0.0, -0.1)):
        com[j] = _record(com[j], start + 0.25 * np.arange(17), _random_coeff(rng, 16), bbox=0.0)
    _check(be, oracle, p, sc["statics"], com, gue, min_vertices=5)


def _hull_block(bb, com, gue):
    """nep_batch_hulls into a block of its own -> (hx [N][np][V][2], hn, first uninflated vertex [N][np][2], uninflated counts)"""
    import torch
    N, npol, V = bb.N, bb.par.num_pol, abi.NEP_HULL_MAX_V
    up = lambda v: (v + 255) & ~255
    o_xy = 0; o_nv = up(N * npol * V * 16); o_xy0 = up(o_nv + N * npol * 4); o_nv0 = up(o_xy0 + N * npol * 16)
    blk = torch.zeros(bb.hull_block_bytes(), dtype=torch.uint8, device=bb.device)
    bb.hulls(bb.to_device(com), bb.to_device(gue), blk)
    bb.check()
    raw = blk.cpu().numpy()
    hx = raw[o_xy:o_xy + N * npol * V * 16].view(np.float64).reshape(N, npol, V, 2)
    hn = raw[o_nv:o_nv + N * npol * 4].view(np.int32).reshape(N, npol)
    h0 = raw[o_xy0:o_xy0 + N * npol * 16].view(np.float64).reshape(N, npol, 2)
    n0 = raw[o_nv0:o_nv0 + N * npol * 4].view(np.int32).reshape(N, npol)
    return hx, hn, h0, n0


def test_entangle_rows_on(be, oracle):
    """a handle with the entangle rows runs both instantiations of group_hull (64 inflated points, then the <= 16 control points in
    the same LDS): the inflated hulls, the uninflated hulls' counts and their first vertex (all the entangle rows read) against the
    oracle, for the full-area trajectories and the degenerate ones"""
    sc, p, com, gue = _base(6)
    p = dataclasses.replace(p, enable_entangle=True)
    rng = np.random.default_rng(15)
    knots = 0.25 * np.arange(17) - 0.25
    twice = _random_coeff(rng, 16); twice[:, 1::2] = twice[:, 0::2]
    rest = np.zeros((2, 16, 4)); rest[0, :, 3] = 1.7; rest[1, :, 3] = -2.3
    for j, c in enumerate((_random_coeff(rng, 16), _random_coeff(rng, 16), twice, rest)):
        com[j] = _record(com[j], knots + 0.5 * (j == 1), c)
    com[4] = _ctrl_record(com[4], _arc_and_far_point(1), 1.2)
    com[5] = _ctrl_record(com[5], _arc_and_far_point(-1), 1.2)
    got = {}
    for mode in (2, 1):
        bb = be.BatchBackend(p, sc["statics"])
        bb.set_hull_kernel(mode)
        got[mode] = _hull_block(bb, com, gue)
        bb.close()
    hx, hn, h0, n0 = got[2]
    for a, b in zip(got[2][1:], got[1][1:]):
        np.testing.assert_array_equal(a, b)
    t0 = float(gue[0]["t_start"])
    for j in range(6):
        pw = abi.nep_pwp.from_buffer_copy(com[j]["pwp"].tobytes())
        d = np.array([com[j]["bbox"][0] / 2 + p.drone_radius, com[j]["bbox"][1] / 2 + p.drone_radius])
        for i in range(p.num_pol):
            h, hu, ov = oracle.hull_of_interval(pw, t0 + i * T, t0 + (i + 1) * T, T, d, with_overflow=True)
            assert not ov
            assert hn[j, i] == len(h) and hx[j, i, :len(h)].tobytes() == h.tobytes(), (j, i)
            assert hx[j, i, :len(h)].tobytes() == got[1][0][j, i, :len(h)].tobytes(), (j, i)
            assert n0[j, i] == len(hu) and h0[j, i].tobytes() == hu[0].tobytes(), (j, i, n0[j, i], len(hu))


def test_inactive_groups_and_skipped_records(be, oracle):
    """num_pol = 5 (groups 5-7 of every wave have no interval), an invalid record and a record that is no agent between the others
    (their waves leave early, counts 0), and two scenes with different t_start in one launch"""
    scs = [PS.make_scene("pol5", 6, 1, seed=s, t_jitter=0.3) for s in (21, 22)]
    p = scs[0]["par"]
    assert p.num_pol == 5
    com = np.stack([sc["committed"] for sc in scs]); gue = np.stack([sc["guesses"] for sc in scs])
    rng = np.random.default_rng(16)
    for s in range(2):
        gue[s]["t_start"] = 0.1 + 0.45 * s                                      # (one t_start per scene: that of its first slot)
        for j in range(6):
            com[s, j] = _record(com[s, j], float(gue[s][0]["t_start"]) - 0.25 + 0.25 * np.arange(17) + 0.03 * (j + 1), _random_coeff(rng, 16))
    com[0, 2]["valid"] = 0
    com[1, 3]["is_agent"] = 0
    statics = scs[0]["statics"]
    got = _check(be, oracle, p, statics, com, gue, min_vertices=6)
    assert (got[0][1][2] == 0).all() and (got[1][1][3] == 0).all() and (got[0][1][[0, 1, 3, 4, 5]] > 0).all()


def test_fused_launch(be):
    """More than 1 024 slots and a static obstacle: from the second replan on block 0 of the hull launch sorts the QP launch order in
    the point area's LDS while the other waves use theirs for hulls.  After two replans: the hulls' boxes equal fe_box_kernel's (a
    handle on the one-hull-per-wave kernel), the order is a permutation of the slots with non-increasing keys, and the redo and
    polish counters are what one round leaves (zeroed by the launch: they would have doubled)."""
    N, S = 8, 136
    four = scene.make_scenes(N, 1, range(31, 35), workers=4, t_jitter=0.3)
    scs = [four[s % 4] for s in range(S)]
    p = scs[0]["par"]
    com = np.stack([sc["committed"] for sc in scs]); gue = np.stack([sc["guesses"] for sc in scs])
    seen = {}
    for mode in (2, 1):
        bb = be.BatchBackend(p, scs[0]["statics"], n_scenes=S)
        for s in range(S):
            bb.set_scene_statics(s, scs[s]["statics"])
        bb.set_hull_kernel(mode)
        bb.set_line_cull(0.05)                                                   # (a 5 cm presolve radius: many replans on the redo list)
        d_com, d_gue = bb.to_device(com), bb.to_device(gue)
        rounds = []
        for r in range(2):
            keys = bb.debug_order_keys() if r else None                         # (as round 1 left them: what round 2's order sorts)
            bb.replan(d_com, d_gue)
            bb.check()
            rounds.append((bb.redo_count(), sorted(bb.redo_list().tolist()), bb.polish_count()))
        path = bb.debug_launch_path()
        assert path["fused_boxes"] == (mode == 2) and path["fused_order"] == (mode == 2) and path["box_kernel"] == (mode == 1), (mode, path)
        assert path["ordered_qp"] and path["redo_pass"], (mode, path)
        order = bb.launch_order()
        assert order is not None and np.array_equal(np.sort(order), np.arange(S * N))
        assert (np.diff(keys[order] & 63) <= 0).all()
        assert rounds[0][0] > 0 and rounds[1] == rounds[0], (mode, rounds[0][0], rounds[1][0], rounds[0][2], rounds[1][2])
        seen[mode] = (rounds[1], [bb.debug_boxes(s) for s in range(4)], [bb.debug_hulls(s) for s in range(4)])
        bb.close()
    assert seen[2][0] == seen[1][0]
    for s in range(4):
        np.testing.assert_array_equal(seen[2][1][s], seen[1][1][s])
        np.testing.assert_array_equal(seen[2][2][s][1], seen[1][2][s][1])
        hx, hn = seen[2][2][s]
        for j in range(N):
            for i in range(p.num_pol):
                v = hx[j, i, :hn[j, i]]
                np.testing.assert_array_equal(seen[2][1][s][j, i], [v[:, 0].min(), v[:, 0].max(), v[:, 1].min(), v[:, 1].max()])
