"""Worlds for the MTLP comparator (include/neptune_mtlp.h): directed runs, each built for one rule of the reference or one edge of
the exact predicates, and a seeded family.  Every world of all_cases() is small — the exact restatement (tests/mtlp_ref.py) is slow:
a grid of at most 16 x 16 x 4 cells, at most 4 robots, max_nodes <= 512, max_pops <= 300.  wide() is a list of its own, with bounds
of its own: the benchmark's five robots and grid, 16 and 64 robots, one robot, pools of up to 8 192 nodes.  A case is
dict(name, cfg, bases [N][3], sg [N][2][3], event); event(reference_result) says that what the world was built for happened, on
the restatement alone.  predicate_records() are near-degenerate inputs of the three predicates in [-8, 8], predicate_records_wide()
over the whole stated domain."""
import functools
from fractions import Fraction as Fr

import numpy as np

import mtlp_ref as ref

# 16 x 16 x 4 cells of 0.25: every cell centre is dyadic, so a point can be put exactly on a triangle, an edge or a sphere
CFG = dict(resolution=0.25, x_min=0.0, x_max=4.0, y_min=0.0, y_max=4.0, z_min=0.0, z_max=1.0, radius=0.25, bias=1.1, n_robots=2,
           max_nodes=512, max_pops=200, path_cap=32)
FAMILY_SEED = 20261023      # of 20261021 .. 26 the one with the most searches that reach their goal (27 of 47; 12 budget, 8 empty, 13 with updates)
FAMILY_RUNS = 16


def cfg(**kw):
    return dict(CFG, **kw)


def _any(key):
    return lambda r: any(key in x["events"] for x in r["results"])


def directed():
    far = ((3.875, 3.875, 0.0), ((3.75, 3.875, 0.875), (3.875, 3.75, 0.875)))      # a robot out of everybody's way
    D = []
    add = lambda name, c, bases, sg, event: D.append(dict(name=name, cfg=cfg(n_robots=len(bases), **c), bases=bases, sg=sg, event=event))      # noqa: E731
    # rule 1: the run ends with the paths (no motion profile): two robots whose cable surfaces cross, both planned
    add("rule1_paths_only", {}, [(0.5, 0.5, 0.0), (3.5, 0.5, 0.0)], [((1.0, 1.0, 0.5), (2.0, 2.0, 0.7)), ((3.0, 1.0, 0.5), (2.0, 1.0, 0.7))],
        lambda r: all(x["status"] == 1 for x in r["results"]))
    # rule 2: triangles apart set both entries; a crossing pair goes down the else-if chain
    add("rule2_apart", {}, [(0.5, 0.5, 0.0), (3.5, 3.5, 0.0)], [((1.0, 0.5, 0.5), (0.5, 1.0, 0.5)), ((3.0, 3.5, 0.5), (3.5, 3.0, 0.5))],
        lambda r: r["branches"][(0, 1)] == "apart" and r["graph"].all())
    # (robot 0 high, robot 1 low: the baselines cross in xy, base_0 -> goal_0 pierces robot 1's triangle and nothing else does)
    hi_lo = ([(0.5, 2.0, 0.0), (2.0, 0.5, 0.0)], [((1.0, 2.0, 0.875), (3.5, 2.0, 0.875)), ((2.0, 1.0, 0.625), (2.0, 3.5, 0.625))])
    add("rule2_chain", {}, hi_lo[0], hi_lo[1], lambda r: r["branches"][(0, 1)] == "cross_end_a" and r["branches"][(1, 0)] == "cross_end_b" and r["graph"].sum() == 3)
    # rule 3: graph(1, 0) = 1 alone (an ordering would move robot 1 first); the order stays 0, 1: robot 0 sees robot 1's start line
    add("rule3_order_is_index", {}, hi_lo[0], hi_lo[1],
        lambda r: r["graph"][1, 0] == 1 and r["graph"][0, 1] == 0 and r["lines"][0] == [((2.0, 0.5, 0.0), (2.0, 1.0, 0.625))] and r["lines"][1] == [((0.5, 2.0, 0.0), (3.5, 2.0, 0.875))])
    # rule 4: j < i with graph(j, i) == 1 gives no line (robot 1 of the pair low, high); without it the line is base_j -> goal_j (robot 3
    # of the pair high, low); the pairs are apart from each other
    P = lambda dx, dy, order: ([[(0.25 + dx, 1.0 + dy, 0.0), (1.0 + dx, 0.25 + dy, 0.0)][k] for k in order],      # noqa: E731
                               [[((0.5 + dx, 1.0 + dy, 0.875), (1.75 + dx, 1.0 + dy, 0.875)), ((1.0 + dx, 0.5 + dy, 0.625), (1.0 + dx, 1.75 + dy, 0.625))][k] for k in order])
    b01, s01 = P(0.0, 0.0, (1, 0)); b23, s23 = P(2.0, 2.0, (0, 1))
    add("rule4_lines", dict(max_pops=60), b01 + b23, s01 + s23,
        lambda r: r["graph"][0, 1] == 1 and [ln[0] for ln in r["lines"][1]] == [b23[0], b23[1]] and r["graph"][2, 3] == 0 and r["lines"][3] == [(b23[0], s23[0][1])])
    # rule 5: the start keeps its point, the goal becomes its (clamped) cell's centre
    add("rule5_setup", {}, [(0.5, 0.5, 0.0), far[0]], [((1.0625, 1.03125, 0.3), (5.0, 2.0, 0.45)), far[1]],
        lambda r: r["results"][0]["path"][0] == (1.0625, 1.03125, 0.3) and r["results"][0]["path"][-1] == (3.875, 2.125, 0.375))
    # rule 6: a neighbour off the grid is an ordinary node; one above the goal height is skipped
    add("rule6_offgrid", {}, [(2.0, 2.0, 0.0), far[0]], [((0.125, 0.125, 0.125), (0.125, 1.125, 0.2)), far[1]], _any("offgrid"))
    add("rule6_above_goal", {}, [(2.0, 2.0, 0.0), far[0]], [((1.0, 1.0, 0.6), (1.5, 1.0, 0.6)), far[1]], _any("above_goal"))
    add("rule6_pool_fills", dict(max_nodes=40), [(0.5, 0.5, 0.0), far[0]], [((1.0, 1.0, 0.5), (3.0, 3.0, 0.5)), far[1]], _any("pool_full"))
    # rule 7: an in-place update leaves the heap out of order
    add("rule7_update_in_place", dict(max_pops=60), [(0.5, 0.5, 0.0), (3.5, 0.5, 0.0)], [((1.0, 1.0, 0.5), (3.0, 3.0, 0.5)), ((3.0, 1.0, 0.5), (1.0, 3.0, 0.7))],
        lambda r: any(x["n_updates"] > 0 and "heap_out_of_order" in x["events"] for x in r["results"]))
    # rule 8: every neighbour of the start is within the ball of robot 1's start line: the list empties
    add("rule8_list_empties", dict(radius=1.0), [(0.5, 0.5, 0.0), (1.0, 1.0, 0.0)], [((1.0, 1.0, 0.5), (3.0, 3.0, 0.5)), ((1.0, 1.0, 0.75), (3.0, 1.0, 0.5))],
        lambda r: r["results"][0]["status"] == -1 and r["results"][0]["pops"] == 1)
    # rule 9: start and goal in one cell: the path is the goal's cell centre alone
    add("rule9_same_cell", {}, [(0.5, 0.5, 0.0), far[0]], [((1.0625, 1.03125, 0.3), (1.125, 1.2, 0.45)), far[1]],
        lambda r: r["results"][0]["path"] == [(1.125, 1.125, 0.375)])
    # a cable line in the plane of swept triangles: base, start and the line all at z = 0.125, the height of the first layer of centres
    add("coplanar_line", dict(radius=0.0), [(0.5, 0.5, 0.125), (3.0, 0.25, 0.125)], [((1.125, 1.125, 0.125), (3.125, 3.125, 0.2)), ((0.25, 3.0, 0.125), (3.5, 3.5, 0.125))],
        _any("coplanar"))
    # a vertical line through robot 0's base touches every swept triangle at a vertex; one through the middle of base -> start, at an edge
    add("touch_vertex", dict(radius=0.0), [(0.5, 0.5, 0.25), (0.5, 0.5, -1.0)], [((1.125, 1.125, 0.375), (2.125, 2.125, 0.5)), ((0.5, 0.5, 1.0), (3.5, 3.5, 0.125))],
        _any("touch_vertex"))
    add("touch_edge", dict(radius=0.0), [(0.125, 0.125, 0.125), (0.625, 0.625, -1.0)], [((1.125, 1.125, 0.375), (2.125, 2.125, 0.5)), ((0.625, 0.625, 1.0), (3.5, 3.5, 0.125))],
        _any("touch_edge"))
    # a vertical line at exactly the radius from a column of centres
    add("line_at_radius", dict(radius=0.25), [(0.5, 0.5, 0.0), (1.625, 1.375, -1.0)], [((1.125, 1.125, 0.375), (2.125, 2.125, 0.5)), ((1.625, 1.375, 2.0), (3.5, 3.5, 0.125))],
        _any("ball_tangent"))
    # base, start and a neighbour's centre on one line
    add("collinear_triangle", {}, [(0.125, 0.125, 0.125), far[0]], [((0.375, 0.375, 0.125), (2.125, 2.125, 0.2)), far[1]],
        lambda r: r["results"][0]["n_degenerate"] > 0 and r["results"][0]["flags"] & ref.FLAG_DEGEN)
    # a short cable line wholly inside the ball of a neighbour
    add("ball_only", dict(radius=0.5), [(0.5, 0.5, 0.0), (1.5, 1.375, 0.375)], [((1.125, 1.125, 0.375), (2.125, 2.125, 0.5)), ((1.5, 1.5, 0.375), (3.5, 3.5, 0.125))],
        lambda r: r["results"][0]["n_ball_only"] > 0)
    # one run whose robots reach, spend the budget, and empty their list (robot 3's goal lies below its cell's centre: the goal cell is
    # "above the goal height" and never generated, a quirk of the reference that is kept)
    add("mixed_outcomes", dict(radius=0.5, max_pops=12), [(0.5, 0.5, 0.0), (1.0, 1.0, 0.0), (3.5, 0.5, 0.0), (3.5, 3.5, 0.0)],
        [((1.0, 1.0, 0.5), (1.5, 1.5, 0.5)), ((1.0, 1.0, 0.75), (1.0, 1.5, 0.7)), ((3.0, 0.5, 0.625), (3.0, 1.0, 0.625)), ((3.0, 3.5, 0.625), (0.5, 3.5, 0.5))],
        lambda r: {x["status"] for x in r["results"]} == {-1, 0, 1})
    # a long path against a short path_cap
    add("path_cap", dict(path_cap=4), [(0.5, 0.5, 0.0), far[0]], [((1.0, 1.0, 0.5), (3.0, 3.0, 0.7)), far[1]],
        lambda r: r["results"][0]["flags"] & ref.FLAG_PATH and r["results"][0]["n_path"] == 4)
    return D


@functools.lru_cache(maxsize=None)
def family():
    """FAMILY_RUNS seeded runs: 2 to 4 robots, two resolutions (0.25 dyadic, 0.2 not), coordinates on a 1/16 lattice or free
    doubles, budgets that some searches meet and some do not (seed FAMILY_SEED)."""
    rng = np.random.default_rng(FAMILY_SEED)
    F = []
    for k in range(FAMILY_RUNS):
        n = 2 + k % 3
        res = 0.25 if k % 2 == 0 else 0.2
        size = 16 * res
        c = cfg(resolution=res, x_max=size, y_max=size, z_max=4 * res, n_robots=n, radius=float(rng.choice([0.0, 0.0625, 0.125, 0.25])), max_pops=int(rng.choice([8, 300, 300])),
                max_nodes=int(rng.choice([64, 512])), path_cap=24)
        lattice = k % 4 < 2
        pt = (lambda hi_z: tuple(np.round(rng.uniform(0.25, size - 0.25, 2) * 16) / 16) + (float(np.round(rng.uniform(0.1, hi_z) * 16) / 16),)) if lattice else \
             (lambda hi_z: tuple(rng.uniform(0.25, size - 0.25, 2)) + (float(rng.uniform(0.1, hi_z)),))
        bases = [pt(0.1)[:2] + (0.0,) for _ in range(n)]
        sg = [(pt(4 * res), pt(4 * res)) for _ in range(n)]
        # (a goal below its cell's centre cannot be reached — that centre is "above the goal height": seven goals in eight are lifted to
        # the upper half of their cell)
        sg = [(s, g if rng.random() < 0.125 else g[:2] + (float((int(g[2] / res) + 0.5 + 0.4375 * rng.random()) * res) if not lattice else (int(g[2] / res) + 0.75) * res,))
              for s, g in sg]
        F.append(dict(name="family_%02d" % k, cfg=c, bases=[tuple(float(v) for v in b) for b in bases],
                      sg=[tuple(tuple(float(v) for v in p) for p in s) for s in sg], event=lambda r: True))
    return F


def all_cases():
    return directed() + family()


# ---- wide worlds: past four robots, past 512 nodes, one robot, the benchmark's own shape ------------------------------------------------
# Kept out of all_cases(): test_worlds_are_small holds for everything above.  Bounds of their own (tests/test_mtlp_cpu.py,
# test_wide_worlds_are_bounded): n_robots <= 64, max_nodes <= 8192, and min(max_pops, pool) * n_robots * max(1, n_robots - 1) <=
# WIDE_WORK — a search pops every node at most once, so min(max_pops, pool) bounds its pops, and the restatement's work per pop is
# the 26 x (N - 1) block; lattice64 is 2 * 64 * 63 = 8 064.
WIDE_WORK = 8192
LATTICE_SEED = {16: 5, 64: 5}
WIDE_NAMES = ["bench5_0", "bench5_1", "bench5_2", "lattice16", "lattice64", "one_robot_budget", "one_robot_pool", "one_robot_default_pool", "one_robot_reached"]


def _benchmark_script():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("mtlp_benchmark", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "mtlp_benchmark.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def _tuples(a):
    return [tuple(float(v) for v in p) for p in a]


def _bench5():
    """the first three runs of seed 0 of scripts/mtlp_benchmark.py, by its own functions; budgets at which some searches reach and
    some do not"""
    import math
    from neptune_amd import mtlp
    B = _benchmark_script()
    assert B.N == 5
    c = dict(resolution=B.RES, x_min=B.BOUNDS[0], x_max=B.BOUNDS[1], y_min=B.BOUNDS[2], y_max=B.BOUNDS[3], z_min=B.BOUNDS[4], z_max=B.BOUNDS[5], radius=B.RADIUS, bias=1.1,
             n_robots=5, max_nodes=2048, max_pops=48, path_cap=64)
    bases = mtlp.circle_bases(5)
    rng = np.random.default_rng(0)
    pos = np.array([[-10.0 * math.cos(2 * math.pi / 5 * i), -10.0 * math.sin(2 * math.pi / 5 * i), B.HEIGHT] for i in range(5)])
    out = []
    for r in range(3):
        goals = B.goals_random(rng, bases, pos)
        sg = np.stack([pos, goals], axis=1).astype(np.float32).astype(np.float64)
        out.append(dict(name="bench5_%d" % r, cfg=c, bases=_tuples(bases), sg=[tuple(_tuples(p)) for p in sg], event=lambda r_: True))
        pos = goals
    return out


def _lattice(n, max_pops):
    """n robots in the 4 x 4 x 1 world on a 1/16 lattice: up to n - 1 cable lines per search, n * n graph entries"""
    rng = np.random.default_rng(LATTICE_SEED[n])
    xy = lambda: tuple(float(v) / 16.0 for v in rng.integers(4, 61, 2))      # noqa: E731
    bases = [xy() + (0.0,) for _ in range(n)]
    sg = [(xy() + (float(rng.integers(1, 16)) / 16.0,), xy() + (0.6875,)) for _ in range(n)]
    return dict(name="lattice%d" % n, cfg=cfg(n_robots=n, max_nodes=256, max_pops=max_pops), bases=bases, sg=sg, event=lambda r: True)


def _wide_event(cases):
    """over the three benchmark runs together: a search reaches, one ends on the budget, one takes an in-place update"""
    def event(_):
        res = [x for c in cases for x in reference(c)["results"]]
        return any(x["status"] == 1 for x in res) and any(x["status"] == 0 for x in res) and any(x["n_updates"] > 0 for x in res)
    return event


def _is(status, pops, nodes, updates=None):
    return lambda r: (r["results"][0]["status"], r["results"][0]["pops"], r["results"][0]["nodes_used"]) == (status, pops, nodes) and \
        (updates is None or r["results"][0]["n_updates"] == updates) and r["lines"] == [[]]


@functools.lru_cache(maxsize=None)
def wide():
    D = _bench5()
    for c in D:
        c["event"] = _wide_event(list(D))
    l16, l64 = _lattice(16, 6), _lattice(64, 2)
    l16["event"] = lambda r: {x["status"] for x in r["results"]} == {-1, 0, 1} and {len(ln) for ln in r["lines"]} >= {0, 15}      # (a robot with no line among 16)
    l64["event"] = lambda r: "cross_none" in r["branches"].values() and len(r["lines"][0]) == 63 and len(r["lines"][63]) > 0
    D += [l16, l64]
    # one robot: no cable line, an empty dense block.  The goal lies below its cell's centre, which is then "above the goal height"
    # and never generated: the search runs until the budget, the pool and then the list, or the default pool ends it
    one = lambda name, c, goal, event: D.append(dict(name="one_robot_" + name, cfg=cfg(n_robots=1, **c), bases=[(0.5, 0.5, 0.0)], sg=[((1.0, 1.0, 0.5), goal)], event=event))      # noqa: E731
    one("budget", dict(max_nodes=8192, max_pops=3000), (3.0, 3.0, 0.55), _is(0, 3000, 4327, 2566))
    one("pool", dict(max_nodes=3000, max_pops=20000), (3.0, 3.0, 0.55), _is(-1, 3000, 3000))
    one("default_pool", dict(max_nodes=0, max_pops=20000), (3.0, 3.0, 0.55), _is(-1, 1024, 1024))
    one("reached", {}, (3.0, 3.0, 0.6875), lambda r: r["results"][0]["status"] == 1 and r["results"][0]["path"][0] == (1.0, 1.0, 0.5) and r["results"][0]["path"][-1] == (3.125, 3.125, 0.625))
    assert [c["name"] for c in D] == WIDE_NAMES
    return D


def wide_case(name):
    return wide()[WIDE_NAMES.index(name)]


def shifted(case, dx):
    """the case moved by dx along x"""
    mv = lambda p: (p[0] + dx, p[1], p[2])      # noqa: E731
    return dict(case, name="%s+%g" % (case["name"], dx), bases=[mv(b) for b in case["bases"]], sg=[(mv(s), mv(g)) for s, g in case["sg"]])


def wide_counts():
    """what the wide worlds exercise, on the restatement alone"""
    res = [x for c in wide() for x in reference(c)["results"]]
    br = sorted({b for c in wide() for b in reference(c)["branches"].values()})
    return dict(searches=len(res), reached=sum(x["status"] == 1 for x in res), budget=sum(x["status"] == 0 for x in res), empty=sum(x["status"] == -1 for x in res),
                updates=sum(x["n_updates"] > 0 for x in res), max_updates=max(x["n_updates"] for x in res), branches=br)


_REF = {}


def reference(case):
    if case["name"] not in _REF:
        _REF[case["name"]] = ref.solve(case["cfg"], case["bases"], case["sg"])
    return _REF[case["name"]]


def make_handle(cfgd):
    from neptune_amd import mtlp
    return mtlp.Mtlp(mtlp.make_cfg(**cfgd))


def groups(cases):
    """cases that share a configuration, in order: [(cfg, [case, ...])]"""
    out = []
    for c in cases:
        for g in out:
            if g[0] == c["cfg"]:
                g[1].append(c); break
        else:
            out.append((c["cfg"], [c]))
    return out


def pack(cases):
    return np.array([c["bases"] for c in cases], dtype=np.float64), np.array([c["sg"] for c in cases], dtype=np.float64)


def expected(cfgd, cases):
    """the restatement's answers in the layout of Mtlp.solve"""
    from neptune_amd import abi
    n, r = cfgd["n_robots"], len(cases)
    out = dict(graph=np.zeros((r, n, n), dtype=np.int32), run_status=np.zeros(r, dtype=np.int32), result=np.zeros((r, n), dtype=abi.MTLP_RESULT_DTYPE),
               path=np.zeros((r, n, cfgd["path_cap"], 3), dtype=np.float64))
    for k, c in enumerate(cases):
        ans = reference(c)
        out["graph"][k] = ans["graph"]; out["run_status"][k] = ans["run_status"]
        for i, x in enumerate(ans["results"]):
            for f in out["result"].dtype.names:
                out["result"][k, i][f] = x[f]
            if x["path"]:
                out["path"][k, i, :len(x["path"])] = np.array(x["path"])
    return out


def same_bytes(a, b):
    """None, or the first output array that differs"""
    for key in ("graph", "run_status", "result", "path"):
        if a[key].tobytes() != b[key].tobytes():
            return key
    return None


def family_counts():
    res = [x for c in family() for x in reference(c)["results"]]
    return dict(searches=len(res), reached=sum(x["status"] == 1 for x in res), budget=sum(x["status"] == 0 for x in res),
                empty=sum(x["status"] == -1 for x in res), updates=sum(x["n_updates"] > 0 for x in res))


# ---- near-degenerate inputs of the three predicates (records of 16 doubles, nep_mtlp_predicates_*) -------------------------------------
PRED_SEED = 5
PRED_N = 10000


def _ulp_move(x, k):
    """k units in the last place; below 2^-8, where an ulp is finer than the domain's lattice, k steps of 2^-60"""
    if abs(x) < 2.0 ** -8:
        return x + k * 2.0 ** -60
    for _ in range(abs(k)):
        x = float(np.nextafter(x, np.inf if k > 0 else -np.inf))
    return x


@functools.lru_cache(maxsize=None)
def predicate_records():
    """(which [n], records [n][16]): the query is put exactly on the primitive — by a dyadic combination of dyadic points, so that
    the point itself is exact — and then one coordinate moves by 0, +-1 or +-2 ulp."""
    rng = np.random.default_rng(PRED_SEED)
    which = np.zeros(PRED_N, dtype=np.int32); rec = np.zeros((PRED_N, 16), dtype=np.float64)
    dy = lambda n: rng.integers(-64, 65, n) / 8.0      # noqa: E731
    for k in range(PRED_N):
        w = k % 3
        which[k] = w
        move = int(rng.integers(-2, 3)); coord = int(rng.integers(0, 3 if w != 1 else 2))
        if w == 0:      # a segment end on the triangle's plane, inside, on an edge or on a vertex (weights of quarters)
            a, b, c = dy(3), dy(3), dy(3)
            wa, wb = rng.integers(0, 5), rng.integers(0, 5)
            wa, wb = (wa, wb) if wa + wb <= 4 else (4 - wa, 4 - wb)
            q = (wa * a + wb * b + (4 - wa - wb) * c) / 4.0
            p = dy(3) if k % 2 else (q + (b - a) * rng.integers(-2, 3) / 2.0)      # ... or a whole segment in the plane
            q = q.copy(); q[coord] = _ulp_move(q[coord], move)
            rec[k, :15] = np.concatenate([p, q, a, b, c])
        elif w == 1:      # a segment end on the other segment, or on its line beyond an end
            u, v = dy(3), dy(3)
            t = rng.integers(-2, 7) / 4.0
            q = u + (v - u) * t
            p = dy(3)
            q = q.copy(); q[coord] = _ulp_move(q[coord], move)
            rec[k, :12] = np.concatenate([p, q, u, v])
        else:      # a segment tangent to the ball, or ending on the sphere: Pythagorean offsets of a dyadic radius
            c = dy(3); r = float(rng.choice([0.625, 1.25, 3.25]))
            tr = {0.625: (0.375, 0.5), 1.25: (0.75, 1.0), 3.25: (1.25, 3.0)}[r]
            foot = c + np.array([tr[0], tr[1], 0.0])      # at distance r exactly
            d = np.array([-tr[1], tr[0], float(rng.integers(-3, 4)) * 0.0]) * float(rng.integers(1, 4))      # perpendicular to the radius
            p, q = (foot - d, foot + d) if k % 2 else (foot, foot + np.array([tr[0], tr[1], 0.0]) * float(rng.integers(0, 3)))
            p = p.copy(); p[coord] = _ulp_move(p[coord], move)
            rec[k, :10] = np.concatenate([c, p, q, [r * r]])
    return which, rec


def predicate_truth(w, q):
    """the verdict of record q under predicate w, in Fractions"""
    P = lambda i: ref.F3(q[i:i + 3])      # noqa: E731
    if w == 0:
        return int(ref.seg_tri(P(0), P(3), P(6), P(9), P(12)))
    if w == 1:
        flat = lambda i: (Fr(float(q[i])), Fr(float(q[i + 1])), Fr(0))      # noqa: E731
        return int(ref.seg_seg(flat(0), flat(3), flat(6), flat(9)))
    hit, inside = ref.ball_seg(P(0), Fr(float(q[9])), P(3), P(6))
    return int(hit) | (2 if inside else 0)


# ---- the same three predicates over the whole stated domain -----------------------------------------------------------------------------
WIDE_PRED_SEED = 11
WIDE_PRED_N = 2000      # per predicate, before the directed ball records
N_LATTICES = 5
# Pythagorean (radius, offset, offset), scaled by BALL_SCALES
BALL_TRIPLES = ((Fr(5, 8), Fr(3, 8), Fr(1, 2)), (Fr(5, 4), Fr(3, 4), Fr(1)), (Fr(13, 4), Fr(5, 4), Fr(3)))
BALL_SCALES = (Fr(1), Fr(4096), Fr(16384), Fr(1, 2 ** 20))


def _lattice_value(rng, kind):
    """one coordinate, as a Fraction, from lattice `kind`"""
    if kind == 0:
        return Fr(int(rng.integers(-64, 65)), 8)
    if kind == 1:
        return Fr(4 * int(rng.integers(-25000, 25001)))
    if kind == 2:
        return Fr(int(rng.integers(-2 ** 20, 2 ** 20 + 1)), 2 ** 58)
    if kind == 3:
        return Fr(4 * int(rng.integers(-25000, 25001))) + Fr(int(rng.integers(-8, 9)), 2 ** 34)
    return Fr(int(rng.integers(-4, 5)), 2 ** 58)


def _exact_doubles(values):
    """the values as doubles, or None when one does not convert exactly or leaves the domain"""
    out = [float(v) for v in values]
    return out if all(Fr(x) == v and ref.in_domain(x) for x, v in zip(out, values)) else None


def ball_quantities(c, r2, p, q):
    """the five quantities whose signs ball_seg takes (ball_sign_exact's `which` 0 to 4), in Fractions"""
    A, Aq, L, t = ref.dot(ref.sub(c, p), ref.sub(c, p)), ref.dot(ref.sub(c, q), ref.sub(c, q)), ref.dot(ref.sub(q, p), ref.sub(q, p)), ref.dot(ref.sub(c, p), ref.sub(q, p))
    return (A - r2, Aq - r2, t, t - L, A * L - t * t - r2 * L)


@functools.lru_cache(maxsize=None)
def predicate_records_wide():
    """(which [n], records [n][16], kinds [n][3]): predicate_records' construction — the query exactly on the primitive, then one
    coordinate moved by 0, +-1, +-2 steps — with every axis of a record on one of five lattices (kinds: the choice per axis, shared by
    all points of the record, so that dyadic combinations along an axis stay representable): 0: k / 8 in [-8, 8]; 1: 4 k up to 1e5;
    2: k 2^-58 up to 2^-38; 3: 4 k + m 2^-34, |m| <= 8 (large values whose low mantissa bits are set); 4: k 2^-58, |k| <= 4.  Points
    are built in Fractions; a record is kept when every value is a double of the domain exactly, before and after the move.  The
    ball's radius and offsets are Pythagorean triples times 1, 4096, 16384 or 2^-20, on two axes that rotate; its directed records
    put each of the five quantities of ball_seg at exactly zero, and segments wholly inside."""
    rng = np.random.default_rng(WIDE_PRED_SEED)
    which, rec, kinds = [], [], []
    zero = [0] * 5; inside = 0
    pt = lambda kd: tuple(_lattice_value(rng, int(k)) for k in kd)      # noqa: E731
    lin = lambda *terms: tuple(sum(w * x[k] for w, x in terms) for k in range(3))      # noqa: E731

    def keep(w, kd, values, moved, coord, move, r2=None):
        """values: the record in Fractions; coordinate `coord` of point `moved` moves by `move` steps"""
        d = _exact_doubles(values)
        if d is None:
            return False
        i = 3 * moved + coord
        d[i] = _ulp_move(d[i], move)
        if not ref.in_domain(d[i]):
            return False
        if r2 is not None:      # the radius squared is no coordinate: exact, a multiple of 2^-120, beyond 1e5 at the large scales
            if Fr(float(r2)) != r2:
                return False
            d.append(float(r2))
        which.append(w); rec.append(d + [0.0] * (16 - len(d))); kinds.append([int(k) for k in kd])
        return True

    for w in (0, 1, 2):
        n = 0
        while n < WIDE_PRED_N:
            kd = rng.integers(0, N_LATTICES, 3)
            move = int(rng.integers(-2, 3)); coord = int(rng.integers(0, 3 if w != 1 else 2))
            if w == 0:      # a segment end on the triangle's plane, inside, on an edge or on a vertex (weights of quarters)
                a, b, c = pt(kd), pt(kd), pt(kd)
                wa, wb = int(rng.integers(0, 5)), int(rng.integers(0, 5))
                wa, wb = (wa, wb) if wa + wb <= 4 else (4 - wa, 4 - wb)
                q = lin((Fr(wa, 4), a), (Fr(wb, 4), b), (Fr(4 - wa - wb, 4), c))
                p = pt(kd) if n % 2 else lin((1, q), (Fr(int(rng.integers(-2, 3)), 2), ref.sub(b, a)))      # ... or a whole segment in the plane
                n += keep(0, kd, p + q + a + b + c, 1, coord, move)
            elif w == 1:      # a segment end on the other segment, or on its line beyond an end
                u, v = pt(kd), pt(kd)
                q = lin((1, u), (Fr(int(rng.integers(-2, 7)), 4), ref.sub(v, u)))
                n += keep(1, kd, pt(kd) + q + u + v, 1, coord, move)
            else:      # a segment tangent to the ball, or ending on the sphere
                scale = BALL_SCALES[int(rng.integers(0, 4))]; r, o1, o2 = (x * scale for x in BALL_TRIPLES[int(rng.integers(0, 3))])
                ax = n % 3      # the offsets lie on axes ax and ax + 1
                e1 = tuple(Fr(int(k == ax)) for k in range(3)); e2 = tuple(Fr(int(k == (ax + 1) % 3)) for k in range(3))
                c = pt(kd)
                off = lin((o1, e1), (o2, e2)); foot = lin((1, c), (1, off))
                d = lin((int(rng.integers(1, 4)), lin((-o2, e1), (o1, e2))))      # perpendicular to the radius
                p, q = (ref.sub(foot, d), lin((1, foot), (1, d))) if n % 2 else (foot, lin((1, foot), (int(rng.integers(0, 3)), off)))
                n += keep(2, kd, c + p + q, 1, coord, move, r * r)
    # directed ball records, five kinds in turn until each has its share
    k = 0
    while min(zero) < 60 or inside < 60:
        k += 1
        kd = rng.integers(0, N_LATTICES, 3)
        scale = BALL_SCALES[int(rng.integers(0, 4))]; r, o1, o2 = (x * scale for x in BALL_TRIPLES[int(rng.integers(0, 3))])
        kind, ax, half = k % 6, k // 6 % 3, k // 18 % 2 == 1
        e1 = tuple(Fr(int(j == ax)) for j in range(3)); e2 = tuple(Fr(int(j == (ax + 1) % 3)) for j in range(3))
        c = pt(kd)
        off = lin((o1, e1), (o2, e2)); perp = lin((int(rng.integers(1, 4)), lin((-o2, e1), (o1, e2))))
        foot, far = lin((1, c), (1, off)), lin((1, c), (2, off))
        move = 0
        if kind == 0:      # p on the sphere, q beyond it
            p, q = foot, lin((1, far), (1, perp))
        elif kind == 1:      # q on the sphere
            p, q = lin((1, far), (1, perp)), foot
        elif kind == 2:      # both ends outside, the segment leaves p at right angles to p -> c: t = 0
            p, q = far, lin((1, far), (1, perp))
        elif kind == 3:      # ... reaches q at right angles to q -> c: t = |q - p|^2
            p, q = lin((1, far), (1, perp)), far
        elif kind == 4:      # tangent at the foot
            p, q = ref.sub(foot, perp), lin((1, foot), (1, perp))
        else:      # wholly inside: from the centre to the sphere's point, moved inward by one step, or to half the offset
            p, q = c, (lin((1, c), (Fr(1, 2), off)) if half else foot)
            move = 0 if half else -1      # (the offsets are positive)
        if not keep(2, kd, c + p + q, 2, ax, move, r * r):
            continue
        row = rec[-1]
        qty = ball_quantities(ref.F3(row[0:3]), Fr(row[9]), ref.F3(row[3:6]), ref.F3(row[6:9]))
        if kind < 5:
            assert qty[kind] == 0, (kind, row)
            zero[kind] += 1
        else:
            assert qty[0] < 0 and qty[1] < 0, row
            inside += 1
    assert min(zero) >= 50 and inside >= 50
    return np.array(which, dtype=np.int32), np.array(rec, dtype=np.float64), np.array(kinds, dtype=np.int32)
