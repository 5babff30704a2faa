"""GPU: the hull kernel's chain walk with its skip rule (hull_group_kernel, neptune_amd/csrc/hull_chain.h), on the smallest inputs
where the rule can go wrong.  Every case forces the eight-hulls-per-wave kernel (set_hull_kernel(2)) on four committed trajectories
and compares vertex counts and vertices BIT FOR BIT with the one-hull-per-wave kernel (set_hull_kernel(1), which walks every point)
and with the oracle's hull_of_interval.  A model of the rule in numpy states what each case is there for — which sorted points are
flagged, where in their chain they lie, whether the hull skips at all — so that a case cannot lose its point silently.

(helpers after tests/test_gpu_hull_group_layout.py)"""
import dataclasses

import numpy as np
import pytest

from neptune_amd import abi, scene

pytestmark = pytest.mark.gpu

T = 0.5
A_POS = np.linalg.inv(scene.A_POS_INV)
REL_GAP, MIN_THR, TINY_GAP, MAX_COORD = 2.0 ** -32, 1e-150, 1e-150, 1e150      # hull_chain.h


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


# ---- committed trajectories made to order ------------------------------------------------------------------------------------

def _record(base, knots, coeff_xy, bbox):
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


def _axis_of_ctrl(v, dt):
    """four control values of a segment of length dt -> its coefficients (up to rounding)"""
    return (A_POS.T @ np.asarray(v, dtype=np.float64)) / np.array([dt ** 3, dt ** 2, dt, 1.0])


def _segments(base, xs, ys, bbox):
    """a record of len(xs) <= 4 segments of 0.1 s (all inside interval 0).  xs[s], ys[s]: a number — the axis is CONSTANT there (only the
    last coefficient: its control values are that number times 1, 1, 1 - 4e-16, 1 - 7e-16) — or four control values"""
    n = len(xs)
    knots = [0.1 * k for k in range(n)] + [0.5]
    co = np.zeros((2, n, 4))
    for s in range(n):
        dt = knots[s + 1] - knots[s]
        for ax, v in enumerate((xs[s], ys[s])):
            if np.ndim(v) == 0:
                co[ax, s, 3] = v
            else:
                co[ax, s] = _axis_of_ctrl(v, dt)
    return _record(base, knots, co, bbox)


def _random_coeff(rng, n):
    return rng.normal(size=(2, n, 4)) * np.array([0.05, 0.1, 0.5, 3.0])


# ---- the rule, modelled ------------------------------------------------------------------------------------------------------

def _model(rec, p, t0, i):
    """the sorted, de-duplicated points of interval i's inflated hull and the rule's verdict on them -> dict(m, flags [m] bool, off,
    thr, xy [m][2]); the control points in the kernel's association"""
    k = np.asarray(rec["pwp"]["times"][: int(rec["pwp"]["n_seg"]) + 1]); n = len(k) - 1
    a, b = t0 + i * T, t0 + (i + 1) * T
    first = min(max(int((k < a).sum()) - 1, 0), n - 1); last = min(max(int((k <= b).sum()) - 1, 0), n - 1)
    cps = []
    for s in range(first, last + 1):
        _t = k[s + 1] - k[s] if (s != last or b > k[s + 1]) else b - k[s]
        _t = min(max(_t, 0.0), T)
        c = np.array([_t * _t * _t, _t * _t, _t, 1.0])
        for kk in range(4):
            v = []
            for ax in range(2):
                P = rec["pwp"]["coeff"][ax][s]
                Ai = scene.A_POS_INV[:, kk]
                v.append((((P[0] * c[0]) * Ai[0] + (P[1] * c[1]) * Ai[1]) + (P[2] * c[2]) * Ai[2]) + (P[3] * c[3]) * Ai[3])
            cps.append(v)
    cps = np.array(cps)
    d = np.array([rec["bbox"][0] / 2 + p.drone_radius, rec["bbox"][1] / 2 + p.drone_radius])
    inflate = not np.sqrt(d[0] * d[0] + d[1] * d[1]) < 1e-6
    pts = np.concatenate([cps + d * sg for sg in ((1, 1), (1, -1), (-1, -1), (-1, 1))]) if inflate else cps
    xy = np.array(sorted(set(map(tuple, pts))))
    cmax = np.abs(cps).max() + (np.abs(d).max() if inflate else 0.0)
    thr = max(cmax * REL_GAP, MIN_THR) if cmax < MAX_COORD else np.inf
    dxs = np.diff(xy[:, 0])
    off = bool(((dxs > 0) & (dxs < TINY_GAP)).any()) or not np.isfinite(thr)
    flags = np.zeros(len(xy), dtype=bool)
    if not off:
        flags[1:] = (dxs == 0) & (np.diff(xy[:, 1]) > thr)
    return dict(m=len(xy), flags=flags, off=off, thr=thr, xy=xy)


# ---- device against device against oracle ----------------------------------------------------------------------------------

def _hull_block(bb, com, gue):
    """nep_batch_hulls into a block of its own -> (hx [N][np][V][2], hn, first uninflated vertex [N][np][2], uninflated counts)"""
    import torch
    N, npol, V = bb.N, bb.par.num_pol, abi.NEP_HULL_MAX_V
    up = lambda v: (v + 255) & ~255
    o_xy = 0; o_nv = up(N * npol * V * 16); o_xy0 = up(o_nv + N * npol * 4); o_nv0 = up(o_xy0 + N * npol * 16)
    blk = torch.zeros(bb.hull_block_bytes(), dtype=torch.uint8, device=bb.device)
    bb.hulls(bb.to_device(com), bb.to_device(gue), blk)
    raw = blk.cpu().numpy()
    hx = raw[o_xy:o_xy + N * npol * V * 16].view(np.float64).reshape(N, npol, V, 2)
    hn = raw[o_nv:o_nv + N * npol * 4].view(np.int32).reshape(N, npol)
    h0 = raw[o_xy0:o_xy0 + N * npol * 16].view(np.float64).reshape(N, npol, 2)
    n0 = raw[o_nv0:o_nv0 + N * npol * 4].view(np.int32).reshape(N, npol)
    return hx, hn, h0, n0


def _check(be, oracle, p, statics, com, gue, entangle=False):
    """the hull launch alone (nep_batch_hulls: no boxes asked for), grouped kernel == one-hull-per-wave kernel == oracle, bit for bit;
    with the entangle rows the uninflated hull's count and first vertex too"""
    if entangle:
        p = dataclasses.replace(p, enable_entangle=True)
    got = {}
    for mode in (2, 1):
        bb = be.BatchBackend(p, statics)
        bb.set_hull_kernel(mode)
        got[mode] = _hull_block(bb, com, gue)
        bb.close()
    hx, hn, h0, n0 = got[2]
    np.testing.assert_array_equal(hn, got[1][1])
    t0 = float(gue[0]["t_start"])
    V = abi.NEP_HULL_MAX_V
    for j in range(len(com)):
        pw = abi.nep_pwp.from_buffer_copy(com[j]["pwp"].tobytes())
        d = np.array([com[j]["bbox"][0] / 2 + p.drone_radius, com[j]["bbox"][1] / 2 + p.drone_radius])
        for i in range(p.num_pol):
            h, hu, _ov = oracle.hull_of_interval(pw, t0 + i * T, t0 + (i + 1) * T, T, d, with_overflow=True)
            assert hn[j, i] == len(h), (j, i, hn[j, i], len(h))
            assert hx[j, i, :len(h)].tobytes() == h.tobytes(), (j, i)
            assert hx[j, i, :len(h)].tobytes() == got[1][0][j, i, :len(h)].tobytes(), (j, i)
            if entangle:
                assert n0[j, i] == got[1][3][j, i] == min(len(hu), V) and h0[j, i].tobytes() == hu[0].tobytes() == got[1][2][j, i].tobytes(), (j, i)
    return got[2]


def _base(N=4, M=1, seed=3, radius=0.6):
    sc = scene.make_scene(N, M, seed=seed)
    assert float(sc["guesses"][0]["t_start"]) == 0.0
    return sc, dataclasses.replace(sc["par"], drone_radius=radius), sc["committed"].copy(), sc["guesses"].copy()


def _skipped(md):
    """(sorted indices the lower chain does not visit, ... the upper chain does not visit)"""
    m, f = md["m"], md["flags"]
    return [j for j in range(m - 1) if f[j]], [j for j in range(1, m - 1) if f[j + 1]]


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def test_hovering_records(be, oracle):
    """every control point of a segment in one cluster within ulps (a record at rest: only the constant coefficient), inflated: the four
    corner clusters are runs of equal or nearly equal x whose y differ by ulps — below the gap, never flagged — and by 2 dy"""
    sc, p, com, gue = _base()
    for j, (x, y) in enumerate(((1.7, -2.3), (0.0, 45.0), (3e-10, 45.0), (-48.0, 1e-10))):
        com[j] = _segments(com[j], [x] * 4, [y] * 4, bbox=1.2)
    for j in range(4):
        md = _model(com[j], p, 0.0, 0)
        assert 4 < md["m"] <= 36 and md["flags"].any() and not md["off"], j
    md = _model(com[1], p, 0.0, 0)                            # (x = 0: two runs; in each the cluster's y an ulp or two apart, twice)
    same = np.diff(md["xy"][:, 0]) == 0; gaps = np.diff(md["xy"][:, 1])
    assert len(set(md["xy"][:, 0])) == 2 and (gaps[same] < 1e-13).sum() >= 4 and not md["flags"][1:][same & (gaps < 1e-13)].any() and md["flags"].sum() == 2
    _check(be, oracle, p, sc["statics"], com, gue)
    _check(be, oracle, p, sc["statics"], com, gue, entangle=True)


def test_straight_lines_one_run_per_side(be, oracle):
    """vertical lines (x = 0 exactly in every control point: one run of up to 32 points on either side, all but the ends skipped by one
    chain or the other — in either chain a skipped point right after the first and one second-to-last) and
    horizontal lines (every run has two points)"""
    sc, p, com, gue = _base()
    ramp = [np.array([0.0, 0.31, 0.73, 1.0]) + 1.07 * s for s in range(4)]
    com[0] = _segments(com[0], [0.0] * 4, ramp, bbox=1.2)
    com[1] = _segments(com[1], [0.0], [ramp[0]], bbox=0.4)
    com[2] = _segments(com[2], ramp, [0.0] * 4, bbox=1.2)
    com[3] = _segments(com[3], [r * -2.0 for r in ramp], [2.5] * 4, bbox=0.4)
    md = _model(com[0], p, 0.0, 0)
    lo, up = _skipped(md)
    assert md["m"] == 64 and len(set(md["xy"][:, 0])) == 2 and md["m"] - 2 in lo and 1 in lo and 1 in up and md["m"] - 2 in up and len(lo) == len(up) == 61
    md = _model(com[2], p, 0.0, 0)
    assert md["m"] > 40 and md["flags"].sum() >= md["m"] // 2 - 2
    _check(be, oracle, p, sc["statics"], com, gue)


def test_runs_with_gaps_on_both_sides_of_the_threshold(be, oracle):
    """x constant within a segment and small enough for its cluster to vanish in x +- dx (0.001 s: eight runs of eight points and more), y values 1e-12,
    1e-10 (below the gap of 2^-32 x the largest coordinate, about 6e-10 here), 1e-8, 1e-6 and more apart in one run: flagged and
    unflagged points side by side, with and without inflation (x = 0: one run of sixteen; x of 1e-300: the hull skips nothing)"""
    sc, p, com, gue = _base(radius=0.0)
    ys = [np.array([0.0, 1e-12, 1e-12 + 1e-8, 0.5]), np.array([0.5 + 1e-10, 0.5 + 1e-6, 1.0, 1.0 + 3e-10]),
          np.array([-0.3, -0.3 + 2e-9, 0.2, 0.2 + 1e-10]), np.array([2.0, 2.0 - 1e-12, 1.5, 1.5 + 1e-9])]
    com[0] = _segments(com[0], [0.001, 0.002, 0.003, 0.004], ys, bbox=1.4)
    com[1] = _segments(com[1], [0.0] * 4, ys, bbox=1.4)
    com[2] = _segments(com[2], [0.0] * 4, ys, bbox=0.0)
    com[3] = _segments(com[3], [1e-300, 0.0, 1e-300, 0.0], ys[::-1], bbox=0.0)
    md = _model(com[0], p, 0.0, 0)
    runs = np.unique(md["xy"][:, 0], return_counts=True)[1]
    assert len(runs) == 8 and runs.min() >= 3, runs
    same = np.diff(md["xy"][:, 0]) == 0; gaps = np.diff(md["xy"][:, 1])[same]
    assert 5e-10 < md["thr"] < 8e-10 and ((gaps > 0) & (gaps < md["thr"])).sum() >= 4 and (gaps > md["thr"]).sum() >= 20
    for x in np.unique(md["xy"][:, 0]):                         # (in one run: both kinds)
        f = md["flags"][md["xy"][:, 0] == x][1:]
        assert f.any() and not f.all(), x
    for j in (1, 2):
        md = _model(com[j], p, 0.0, 0)
        assert md["flags"].any() and not md["flags"][1:].all() and not md["off"], j
    assert _model(com[3], p, 0.0, 0)["off"]                  # (x of 0 and of 1e-300 times 1, 1 - 4e-16, ...: closer than the rule allows)
    _check(be, oracle, p, sc["statics"], com, gue)
    _check(be, oracle, p, sc["statics"], com, gue, entangle=True)


def test_cluster_beside_far_points(be, oracle):
    """what breaks the rule without its gap: points of one run an ulp apart in y, near y = 0 and near y = 45, with entries far below and
    above them on the stack (runs at other x) — their differences against the far entry round to the same number"""
    sc, p, com, gue = _base(radius=0.1)
    com[0] = _segments(com[0], [3e-10, -2e-10, 5.0, -5.0], [45.0, 1e-10, 45.0, 20.0], bbox=0.2)
    com[1] = _segments(com[1], [1e-12, 1e-12, -3.0, 3.0], [45.0, 44.0, 1e-10, 45.0], bbox=0.2)
    com[2] = _segments(com[2], [3e-10, -2e-10, 5.0, -5.0], [45.0, 1e-10, 45.0, 20.0], bbox=0.0)
    com[3] = _segments(com[3], [0.0, 0.0, -3.0, 3.0], [45.0, 6e-10, 0.0, 45.0], bbox=0.0)
    p0 = dataclasses.replace(p, drone_radius=0.0)
    for j, pj in ((0, p), (1, p), (3, p0)):
        md = _model(com[j], pj, 0.0, 0)
        same = np.diff(md["xy"][:, 0]) == 0; gaps = np.diff(md["xy"][:, 1])[same]
        assert (gaps < 1e-13).any() and md["flags"].any() and not md["off"], j
    md = _model(com[3], p0, 0.0, 0)
    assert (np.abs(md["xy"][:, 1]) < 1e-9).sum() >= 3 and (md["xy"][:, 1] > 44.0).sum() >= 3
    _check(be, oracle, p, sc["statics"], com[:2].repeat(2), gue)
    _check(be, oracle, p0, sc["statics"], com[2:].repeat(2), gue)


def test_coordinates_of_1e9(be, oracle):
    """the gap grows with the coordinates (2^-32 x 1e9 = 0.23 m): corners 2 dy = 0.3 m apart are still skipped, 0.1 m apart no more,
    and control points a few ulps of 1e9 apart (1.2e-7 m) cluster"""
    sc, p, com, gue = _base(radius=0.05)
    rng = np.random.default_rng(41)
    big = _random_coeff(rng, 4); big[:, :, 3] += 1e9
    com[0] = _record(com[0], [0.0, 0.1, 0.2, 0.3, 0.5], big, bbox=0.2)
    com[1] = _segments(com[1], [1e9] * 4, [-1e9, -1e9 + 1.0, -1e9, -1e9 + 1.0], bbox=0.2)
    com[2] = _segments(com[2], [1e9] * 4, [-1e9, -1e9 + 1.0, -1e9, -1e9 + 1.0], bbox=0.0)
    com[3] = _segments(com[3], [-1e9, 1e9, -1e9, 1e9], [np.array([0.0, 0.2, 0.25, 1.0]) + 1e9] * 4, bbox=0.2)
    md1, md2 = _model(com[1], p, 0.0, 0), _model(com[2], p, 0.0, 0)
    assert 0.2 < md1["thr"] < 0.25 and md1["flags"].any() and not md1["off"]
    same = np.diff(md2["xy"][:, 0]) == 0
    assert md2["m"] > 8 and same.any() and (md2["flags"][1:][same] == (np.diff(md2["xy"][:, 1])[same] > md2["thr"])).all()
    assert (np.diff(md2["xy"][:, 1])[same] < md2["thr"]).any() and not md2["flags"].all()
    _check(be, oracle, p, sc["statics"], com, gue)


def test_hulls_of_one_two_and_three_points(be, oracle):
    """no inflation, control points that are exactly equal (a constant of 0, or subnormal constants: times 1 - 4e-16 they round to
    themselves): m = 1, 2 and 3.  Two x a subnormal apart: closer than the rule's proof allows, the hull skips nothing."""
    sc, p, com, gue = _base(radius=0.0)
    tiny = 5e-324
    com[0] = _segments(com[0], [0.0] * 4, [0.0] * 4, bbox=0.0)
    com[1] = _segments(com[1], [0.0, 0.0], [0.0, tiny], bbox=0.0)
    com[2] = _segments(com[2], [0.0, 0.0, tiny], [0.0, tiny, 0.0], bbox=0.0)
    com[3] = _segments(com[3], [0.0, tiny], [0.0, 0.0], bbox=0.0)
    ms = [_model(com[j], p, 0.0, 0) for j in range(4)]
    assert [md["m"] for md in ms] == [1, 2, 3, 2] and [md["off"] for md in ms] == [False, False, True, True]
    _check(be, oracle, p, sc["statics"], com, gue)
    _check(be, oracle, p, sc["statics"], com, gue, entangle=True)


def test_full_areas_and_groups_of_different_sizes(be, oracle):
    """random cubics: knots every T / 2 (four segments an interval, 64 points in every group) and irregular knots (the eight groups of a
    wave walk 16 to 64 points: their to-do lists end at different trips), both group_hull instantiations"""
    sc, p, com, gue = _base()
    rng = np.random.default_rng(42)
    com[0] = _record(com[0], -0.25 + 0.25 * np.arange(17), _random_coeff(rng, 16), bbox=1.2)
    com[1] = _record(com[1], 0.25 + 0.25 * np.arange(17), _random_coeff(rng, 16), bbox=0.3)
    sizes = set()
    for j in (2, 3):
        while True:
            knots = np.concatenate([[0.0], np.cumsum(rng.choice([0.13, 0.21, 0.34, 0.55, 0.8], size=16))]) - rng.uniform(0, 0.2)
            k = np.asarray(knots)
            per = [min(max(int((k <= (i + 1) * T).sum()) - 1, 0), 15) - min(max(int((k < i * T).sum()) - 1, 0), 15) + 1 for i in range(8)]
            if max(per) <= 4 and len(set(per)) >= 3:
                break
        sizes |= set(per)
        com[j] = _record(com[j], knots, _random_coeff(rng, 16), bbox=1.2)
    assert sizes == {1, 2, 3, 4}
    md = _model(com[0], p, 0.0, 2)
    assert md["m"] >= 56 and md["flags"].sum() >= 24 and _model(com[1], p, 0.0, 2)["m"] >= 56      # (64 points in the area; the interval's last segment has no length inside it, and its cluster partly coincides)
    _check(be, oracle, p, sc["statics"], com, gue)
    _check(be, oracle, p, sc["statics"], com, gue, entangle=True)


def test_replan_path_with_boxes(be, oracle):
    """the same kernel inside a replan (the launch that also makes the hulls' boxes, from the extremes the gap is taken from): two scenes,
    hulls of both kernels and of the oracle, and the boxes against the vertices"""
    scs = [scene.make_scene(4, 1, seed=s) for s in (3, 4)]
    p = scs[0]["par"]
    com = np.stack([sc["committed"] for sc in scs]); gue = np.stack([sc["guesses"] for sc in scs])
    rng = np.random.default_rng(43)
    ramp = [np.array([0.0, 0.3, 0.7, 1.0]) + s for s in range(4)]
    for s in range(2):
        for j in range(3):
            com[s, j] = _record(com[s, j], -0.25 + 0.25 * np.arange(17) + 0.05 * j, _random_coeff(rng, 16), bbox=1.2)
        com[s, 3] = _segments(com[s, 3], [0.0] * 4, ramp, bbox=1.2)
    got = {}
    for mode in (2, 1):
        bb = be.BatchBackend(p, scs[0]["statics"], n_scenes=2)
        bb.set_hull_kernel(mode)
        bb.replan(bb.to_device(com), bb.to_device(gue))
        path = bb.debug_launch_path()
        assert path["grouped_hulls"] == (mode == 2) and path["fused_boxes"] == (mode == 2), (mode, path)
        got[mode] = ([bb.debug_hulls(s) for s in range(2)], [bb.debug_boxes(s) for s in range(2)])
        bb.close()
    for s in range(2):
        (hx, hn), (hx1, hn1) = got[2][0][s], got[1][0][s]
        np.testing.assert_array_equal(hn, hn1)
        np.testing.assert_array_equal(got[2][1][s], got[1][1][s])
        t0 = float(gue[s][0]["t_start"])
        for j in range(4):
            pw = abi.nep_pwp.from_buffer_copy(com[s, j]["pwp"].tobytes())
            d = np.array([com[s, j]["bbox"][0] / 2 + p.drone_radius, com[s, j]["bbox"][1] / 2 + p.drone_radius])
            for i in range(p.num_pol):
                h, _hu, ov = oracle.hull_of_interval(pw, t0 + i * T, t0 + (i + 1) * T, T, d, with_overflow=True)
                assert not ov and hn[j, i] == len(h) and hx[j, i, :len(h)].tobytes() == h.tobytes() == hx1[j, i, :len(h)].tobytes(), (s, j, i)
                np.testing.assert_array_equal(got[2][1][s][j, i], [h[:, 0].min(), h[:, 0].max(), h[:, 1].min(), h[:, 1].max()])
