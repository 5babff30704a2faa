"""GPU: the hull kernel's sort of an inflated hull's corners as stacked pairs (hull_group_kernel, neptune_amd/csrc/hull_pair_sort.h).
Every case is one scene of eight committed trajectories, num_pol 8, on the eight-hulls-per-wave kernel (set_hull_kernel(2)) under
"hull_sort" 1 (pairs) and 0 (always the full network over the corners): vertex counts and vertices BIT FOR BIT against the
one-hull-per-wave kernel (set_hull_kernel(1), a rank sort) and against the oracle's hull_of_interval.  A model of the rule in numpy
states which path each record's wave takes and whether its pairs have runs of equal keys — the decision is per wave: one hull that
is refused sends the wave's eight hulls through the full network — so that no case silently tests only the fallback.

(helpers after tests/test_gpu_hull_chain_skip.py)"""
import dataclasses

import numpy as np
import pytest

from neptune_amd import abi, scene

pytestmark = pytest.mark.gpu

T = 0.5
N_REC = 8
A_POS = np.linalg.inv(scene.A_POS_INV)
MAX_COORD = 1e150      # hull_pair_sort.h
SORTS = (1, 0)      # "hull_sort": the default first


@pytest.fixture(scope="module")
def be():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from neptune_amd import backend
    return backend


@pytest.fixture()
def hull_sort():
    """sets the process-wide option; the default is back when the test ends"""
    from neptune_amd import _lib
    L = _lib.lib()

    def set_(v):
        assert L.nep_debug_set_global_option(b"hull_sort", int(v)) == 0
    yield set_
    set_(1)


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
    """a record of len(xs) <= 4 segments of 0.1 s (all inside interval 0; the LAST one is every later interval's only segment).  xs[s], ys[s]: a
    number — the axis is CONSTANT there (only the last coefficient: its control values are that number times 1, 1, 1 - 4e-16, 1 - 7e-16)
    — or four control values"""
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


def _random_coeff(rng, n, offset=0.0):
    co = rng.normal(size=(2, n, 4)) * np.array([0.05, 0.1, 0.5, 3.0])
    co[:, :, 3] += offset
    return co


def _generic(base, rng, spacing, start, bbox=1.2, offset=0.0):
    """sixteen random cubics on knots start + spacing * k"""
    return _record(base, start + spacing * np.arange(17), _random_coeff(rng, 16, offset), bbox)


# ---- the rule, modelled ------------------------------------------------------------------------------------------------------

def _ctrl(rec, t0, i):
    """control points of interval i in the kernel's association -> [np0][2]"""
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
    return np.array(cps)


def _hull_verdict(rec, p, t0, i):
    """one hull under the rule -> dict(np0, inflate, allowed, key_bad, runs: lengths of the runs of equal keys longer than one, run_bad,
    xs_distinct)"""
    cps = _ctrl(rec, t0, i)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.array([rec["bbox"][0] / 2 + p.drone_radius, rec["bbox"][1] / 2 + p.drone_radius])
        inflate = not np.sqrt(d[0] * d[0] + d[1] * d[1]) < 1e-6
        cmax = np.abs(cps).max() + np.abs(d).max()
        pairs = sorted([(x - d[0], y) for x, y in cps] + [(x + d[0], y) for x, y in cps])
        runs, run_bad, s = [], False, 0
        for e in range(1, len(pairs) + 1):
            if e == len(pairs) or pairs[e][0] != pairs[s][0]:
                if e - s > 1:
                    runs.append(e - s)
                run_bad |= not (pairs[e - 1][1] - d[1] < pairs[s][1] + d[1])
                s = e
        key_bad = any(not (X < np.inf) or X == 0.0 for X, _ in pairs)
    return dict(np0=len(cps), inflate=inflate, allowed=bool(cmax < MAX_COORD and d[1] > 0.0), key_bad=key_bad, runs=runs, run_bad=run_bad,
                xs_distinct=len(set(cps[:, 0])) == len(cps))


def _wave_path(rec, p, t0=0.0):
    """what hull_group_kernel's wave does with this record under "hull_sort" 1: 'pairs' ('pairs, runs' when some hull has a run longer
    than one) or 'full' with the reason"""
    vs = [_hull_verdict(rec, p, t0, i) for i in range(p.num_pol)]
    if not vs[0]["inflate"]:
        return "full: not inflated", vs
    if not all(v["allowed"] for v in vs):
        return "full: refused", vs
    if any(v["key_bad"] for v in vs):
        return "full: key", vs
    if any(v["run_bad"] for v in vs):
        return "full: run", vs
    return ("pairs, runs" if any(v["runs"] for v in vs) else "pairs, none"), vs


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


def _check(be, oracle, hull_sort, p, statics, com, gue, paths, entangle=False):
    """`paths`: per record, what the model must say its wave does (_wave_path's answer).  Then the hull launch alone
    (nep_batch_hulls): the grouped kernel under every "hull_sort" == the one-hull-per-wave kernel == the oracle, bit for bit; with
    the entangle rows the uninflated hull's count and first vertex too"""
    assert len(com) == N_REC == len(paths) and p.num_pol == 8
    got_paths = [_wave_path(com[j], p)[0] for j in range(N_REC)]
    for j in range(N_REC):
        assert got_paths[j] == paths[j], (j, got_paths)
    if entangle:
        p = dataclasses.replace(p, enable_entangle=True)
    got = {}
    for key, mode, srt in [("one", 1, 1)] + [(s, 2, s) for s in SORTS]:
        hull_sort(srt)
        bb = be.BatchBackend(p, statics)
        bb.set_hull_kernel(mode)
        got[key] = _hull_block(bb, com, gue)
        bb.close()
    hx1, hn1, h01, n01 = got["one"]
    t0 = float(gue[0]["t_start"])
    V = abi.NEP_HULL_MAX_V
    for j in range(N_REC):
        pw = abi.nep_pwp.from_buffer_copy(com[j]["pwp"].tobytes())
        d = np.array([com[j]["bbox"][0] / 2 + p.drone_radius, com[j]["bbox"][1] / 2 + p.drone_radius])
        for i in range(p.num_pol):
            h, hu, _ov = oracle.hull_of_interval(pw, t0 + i * T, t0 + (i + 1) * T, T, d, with_overflow=True)
            for s in SORTS:
                hx, hn, h0, n0 = got[s]
                assert hn[j, i] == len(h) == hn1[j, i], (s, j, i, hn[j, i], len(h), hn1[j, i])
                assert hx[j, i, :len(h)].tobytes() == h.tobytes(), (s, j, i)
                assert hx[j, i, :len(h)].tobytes() == hx1[j, i, :len(h)].tobytes(), (s, j, i)
                if entangle:
                    assert n0[j, i] == n01[j, i] == min(len(hu), V) and h0[j, i].tobytes() == hu[0].tobytes() == h01[j, i].tobytes(), (s, j, i)
    return got_paths


def _base(seed=3, radius=0.6):
    sc = scene.make_scene(N_REC, 1, seed=seed)
    assert float(sc["guesses"][0]["t_start"]) == 0.0
    return sc, dataclasses.replace(sc["par"], drone_radius=radius), sc["committed"].copy(), sc["guesses"].copy()


# ---- the cases -----------------------------------------------------------------------------------------------------------------

NONE, RUNS = "pairs, none", "pairs, runs"


def test_intervals_of_one_two_and_four_segments(be, oracle, hull_sort):
    """random cubics with 4, 8 and 12-16 control points an interval, knots off the intervals' grid: one long segment; knots every T, off
    by T / 2 (an interval straddles two segments); knots every 0.17 s (three or four segments): no two keys are equal.  Both group_hull
    instantiations behind the sort (the entangle rows' uninflated hull)"""
    sc, p, com, gue = _base()
    rng = np.random.default_rng(51)
    for j in (0, 3):
        com[j] = _record(com[j], [0.0, 4.0], _random_coeff(rng, 1), bbox=1.2)
    for j in (1, 4, 6):
        com[j] = _generic(com[j], rng, 0.5, -0.25 + 0.01 * j)
    for j in (2, 5, 7):
        com[j] = _generic(com[j], rng, 0.17, -0.1 - 0.01 * j, bbox=0.3 * j)
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, [NONE] * 8)
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, [NONE] * 8, entangle=True)
    sizes = lambda j: {v["np0"] for v in _wave_path(com[j], p)[1]}
    assert sizes(0) == {4} and sizes(1) == {8} and 16 in sizes(2)


def test_knots_on_the_grid(be, oracle, hull_sort):
    """what a committed trajectory looks like every round: knots at the intervals' ends.  An interval takes the segment before it, its own
    and the next one at length zero (12 control points), whose four control points are one point twice and two more within ulps: runs of
    two and more in every hull, the pair path all the same"""
    sc, p, com, gue = _base()
    rng = np.random.default_rng(58)
    for j in range(8):
        com[j] = _generic(com[j], rng, 0.5, 0.0 if j < 4 else -0.5, bbox=1.2 if j % 2 else 0.4)
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, [RUNS] * 8)
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, [RUNS] * 8, entangle=True)
    vs = _wave_path(com[0], p)[1]
    assert [v["np0"] for v in vs] == [8] + [12] * 7 and all(v["runs"] and max(v["runs"]) >= 2 for v in vs)


def test_records_at_rest_and_straight_lines(be, oracle, hull_sort):
    """a hovering record (every control point within ulps of one point: runs of eight pairs and more whose y differ by ulps) and a short
    vertical line (one x, y within 2 dy): the pair path with long runs.  A long vertical line (one x, y over more than 2 dy: the run's ylo
    and yhi interleave): the full network.  A horizontal line (distinct x, one y): no run.  Generic records beside them: the decision is
    per wave"""
    sc, p, com, gue = _base()
    rng = np.random.default_rng(52)
    ramp = [np.array([0.0, 0.31, 0.73, 1.0]) + 1.07 * s for s in range(4)]
    com[0] = _segments(com[0], [1.7] * 4, [-2.3] * 4, bbox=1.2)
    com[1] = _segments(com[1], [3e-10], [45.0], bbox=1.2)
    com[2] = _segments(com[2], [0.25] * 4, ramp, bbox=1.2)
    com[3] = _segments(com[3], [2.5], [ramp[0]], bbox=1.2)
    com[4] = _segments(com[4], ramp, [0.5] * 4, bbox=1.2)
    com[5] = _segments(com[5], [r * -2.0 for r in ramp[:2]], [2.5] * 2, bbox=0.5)
    com[6] = _generic(com[6], rng, 0.5, -0.2)
    com[7] = _generic(com[7], rng, 0.17, -0.1)
    paths = [RUNS, RUNS, "full: run", RUNS, NONE, NONE, NONE, NONE]
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, paths)
    assert max(_wave_path(com[0], p)[1][0]["runs"]) >= 8 and max(_wave_path(com[3], p)[1][0]["runs"]) >= 2
    v = _wave_path(com[2], p)[1]
    assert max(v[0]["runs"]) >= 8 and v[0]["run_bad"] and not any(w["run_bad"] for w in v[1:])      # (interval 0 alone holds all four segments)


def test_shared_x_and_collapsing_pairs(be, oracle, hull_sort):
    """two control points with one x and different y (a segment that moves in y only; the other segments are generic), closer than 2 dy
    and farther — and control points whose x are all different, a few ulps apart at |x| << dx, so that x + dx rounds to one key"""
    sc, p, com, gue = _base()
    rng = np.random.default_rng(53)
    gx = lambda: rng.normal(size=4) * 3.0
    near, far = np.array([0.0, 0.3, 0.6, 0.9]), np.array([0.0, 3.0, 6.0, 9.0])
    com[0] = _segments(com[0], [gx(), 0.75], [gx(), near], bbox=1.2)
    com[1] = _segments(com[1], [0.75, gx()], [far, gx()], bbox=1.2)
    com[2] = _segments(com[2], [gx(), gx(), -1.25, gx()], [gx(), gx(), near * 0.5, gx()], bbox=0.4)
    # x = 1e-10 + (a slope of 1e-24) t: four different doubles within a few ulps of 1e-10 (ulp 1.3e-26); dx = 1.2 swallows them
    for j, x0, ys in ((3, 1e-10, near), (4, -3e-9, far)):
        r = _segments(com[j], [gx(), gx()], [gx(), ys], bbox=1.2)
        r["pwp"]["coeff"][0, 1, :] = [0.0, 0.0, 2e-24 * (j - 2), x0]
        com[j] = r
    for j in (5, 6, 7):
        com[j] = _generic(com[j], rng, 0.5, -0.2 - 0.01 * j)
    paths = [RUNS, "full: run", RUNS, RUNS, "full: run", NONE, NONE, NONE]
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, paths)
    v = _wave_path(com[1], p)[1]
    assert v[0]["run_bad"] and not v[0]["xs_distinct"] and not any(w["run_bad"] or w["runs"] for w in v[1:])      # (the y-only segment is the first: interval 0 alone)
    for j in (3, 4):
        v = _wave_path(com[j], p)[1]
        assert v[0]["xs_distinct"] and v[0]["runs"], (j, v[0])                                # (different x, equal keys)


def test_exactly_one_group_of_the_wave_is_refused(be, oracle, hull_sort):
    """records whose FIRST segment is a long vertical line and whose last one is generic: interval 0's run fails its test, intervals 1-7
    (the last segment alone) have no run at all — the whole wave takes the full network, and its seven generic hulls are the same
    bits.  Beside them the same records with a short line: one group with runs, seven without, the pair path"""
    sc, p, com, gue = _base()
    rng = np.random.default_rng(54)
    gx = lambda: rng.normal(size=4) * 3.0
    far = np.array([0.0, 3.0, 6.0, 9.0])
    com[0] = _segments(com[0], [1.5, gx()], [far, gx()], bbox=1.2)
    com[1] = _segments(com[1], [0.5, gx(), gx()], [far - 4.0, gx(), gx()], bbox=1.2)
    com[2] = _segments(com[2], [gx(), -2.0, gx(), gx()], [gx(), far * -1.0, gx(), gx()], bbox=0.4)
    com[3] = _segments(com[3], [1.5, gx()], [far * 0.1, gx()], bbox=1.2)
    com[4] = _segments(com[4], [gx(), -2.0, gx(), gx()], [gx(), 4.0, gx(), gx()], bbox=0.4)
    for j in range(5, 8):
        com[j] = _generic(com[j], rng, 0.5 if j % 2 else 0.17, -0.1 - 0.01 * j)
    paths = ["full: run"] * 3 + [RUNS] * 2 + [NONE] * 3
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, paths)
    for j in range(5):
        v = _wave_path(com[j], p)[1]
        assert [bool(w["runs"]) for w in v] == [True] + [False] * 7 and [w["run_bad"] for w in v] == [j < 3] + [False] * 7, j


def test_coordinates_of_1e9_and_1e151(be, oracle, hull_sort):
    """1e9: the pair path holds (keys 1.2e-7 apart at the closest); 1e151 in x, in y, in the radius: refused before the network runs —
    for the whole wave, also where only the first interval reaches that magnitude; 1e149 with a radius of 0.1: x + dx = x, every pair
    in a run with its twin"""
    sc, p, com, gue = _base(radius=0.05)
    rng = np.random.default_rng(55)
    gx = lambda s=3.0: rng.normal(size=4) * s
    com[0] = _generic(com[0], rng, 0.5, -0.2, bbox=0.2, offset=1e9)
    com[1] = _generic(com[1], rng, 0.17, -0.1, bbox=0.2, offset=-1e9)
    com[2] = _segments(com[2], [gx(1e151), gx(1e151)], [gx(), gx()], bbox=0.2)
    com[3] = _segments(com[3], [gx(), gx()], [gx(1e151), gx()], bbox=0.2)                 # (y, interval 0 alone)
    com[4] = _segments(com[4], [gx(), gx()], [gx(), gx()], bbox=[0.2, 4e151, 0.2])
    com[5] = _segments(com[5], [gx(1e148), gx(1e148)], [gx(1e148), gx(1e148)], bbox=[2e149, 2e149, 0.2])      # (below the limit: pairs)
    com[6] = _segments(com[6], [gx(1e149), gx(1e149)], [gx(1e149), gx(1e149)], bbox=0.2)      # (... and x + dx = x, y + dy = y)
    com[7] = _generic(com[7], rng, 0.5, -0.27, bbox=0.2)
    paths = [NONE, NONE, "full: refused", "full: refused", "full: refused", NONE, "full: run", NONE]
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, paths)
    assert [w["allowed"] for w in _wave_path(com[3], p)[1]] == [False] + [True] * 7


def test_radius_zero_and_keys_of_zero(be, oracle, hull_sort):
    """no inflation (radius 0 and an empty box): the corners are the control points, the full network as before; a record with a box
    beside them is inflated and takes the pairs; a box in x alone (dy = 0) is refused; x = dx exactly (a key of zero) is refused"""
    sc, p, com, gue = _base(radius=0.0)
    rng = np.random.default_rng(56)
    for j in range(8):
        com[j] = _generic(com[j], rng, 0.5 if j % 2 else 0.17, -0.1 - 0.01 * j, bbox=0.0 if j < 4 else 0.8)
    com[6] = _segments(com[6], [rng.normal(size=4), 0.4], [rng.normal(size=4), rng.normal(size=4)], bbox=0.8)
    com[7]["bbox"] = [0.8, 0.0, 0.8]
    paths = ["full: not inflated"] * 4 + [NONE, NONE, "full: key", "full: refused"]
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, paths)
    _check(be, oracle, hull_sort, p, sc["statics"], com, gue, paths, entangle=True)


def test_replan_on_the_fused_path(be, oracle, hull_sort):
    """the same kernel inside a replan (the launch that also makes the hulls' boxes and the QP launch order): hulls and boxes under either
    "hull_sort", of both kernels and of the oracle; the replan's trajectories are the same bytes"""
    sc, p, com, gue = _base()
    rng = np.random.default_rng(57)
    for j in range(6):
        com[j] = _generic(com[j], rng, 0.5, 0.0 if j % 2 else -0.1 - 0.01 * j)
    com[6] = _segments(com[6], [0.25] * 4, [np.array([0.0, 0.3, 0.7, 1.0]) + s for s in range(4)], bbox=1.2)
    com[7] = _segments(com[7], [-7.5] * 2, [6.5] * 2, bbox=1.2)
    want = [NONE, RUNS] * 3 + ["full: run", RUNS]
    assert [_wave_path(com[j], p)[0] for j in range(N_REC)] == want
    got = {}
    for key, mode, srt in [("one", 1, 1)] + [(s, 2, s) for s in SORTS]:
        hull_sort(srt)
        bb = be.BatchBackend(p, sc["statics"])
        bb.set_hull_kernel(mode)
        bb.replan(bb.to_device(com), bb.to_device(gue))
        path = bb.debug_launch_path()
        assert path["grouped_hulls"] == (mode == 2) and path["fused_boxes"] == (mode == 2), (key, path)
        sol = bb.solutions()
        got[key] = (bb.debug_hulls(0), bb.debug_boxes(0), np.array(sol["coeff"]).tobytes() + sol["stats"]["status"].tobytes())
        bb.close()
    (hx1, hn1), box1, sol1 = got["one"]
    for s in SORTS:
        (hx, hn), box, sol = got[s]
        np.testing.assert_array_equal(hn, hn1)
        np.testing.assert_array_equal(box, box1)
        assert sol == got[SORTS[0]][2], s
        for j in range(N_REC):
            pw = abi.nep_pwp.from_buffer_copy(com[j]["pwp"].tobytes())
            d = np.array([com[j]["bbox"][0] / 2 + p.drone_radius, com[j]["bbox"][1] / 2 + p.drone_radius])
            for i in range(p.num_pol):
                h, _hu, ov = oracle.hull_of_interval(pw, i * T, (i + 1) * T, T, d, with_overflow=True)
                assert not ov and hn[j, i] == len(h) and hx[j, i, :len(h)].tobytes() == h.tobytes() == hx1[j, i, :len(h)].tobytes(), (s, j, i)
                np.testing.assert_array_equal(box[j, i], [h[:, 0].min(), h[:, 0].max(), h[:, 1].min(), h[:, 1].max()])
