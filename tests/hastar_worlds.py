"""Worlds for the homotopic grid A* tests (tests/test_hastar_cpu.py, tests/test_gpu_hastar.py): small hand-built cases, one per
rule of the reference's search, and a seeded family.  Every case is a dict

    name, cfg (nep_hastar_cfg's fields), world (inflated, uninflated, reps), start, goal, hsig0, cont0, event

and `event(r)` says, on the Python reference's result r alone (tests/hastar_ref.py), whether the thing the case is there for
happened.  Grids are at most 16 x 16 cells at resolution 0.5 with at most 3 polygons; references are computed once per process
(`reference`)."""
import math

import numpy as np

import hastar_ref as ref

DIAG = float(np.sqrt(np.float32(2.0)))      # 1.41421353816986083984375
RADIUS = 0.15                               # drone_radius: statics are inflated by 2 * RADIUS


def cfg(n=16, cable=100.0, max_pops=100000, max_nodes=0, hsig_cap=8, cont_cap=48, path_cap=48):
    return dict(resolution=0.5, x_min=0.0, x_max=0.5 * n, y_min=0.0, y_max=0.5 * n, z_min=0.0, z_max=1.0, cable_length=float(cable), bias=1.1,
                max_pops=max_pops, max_nodes=max_nodes, hsig_cap=hsig_cap, cont_cap=cont_cap, path_cap=path_cap)


def square(cx, cy, half=0.25):
    """neptune_ros.cpp:242-243's vertex order"""
    return [(cx + half, cy + half), (cx + half, cy - half), (cx - half, cy - half), (cx - half, cy + half)]


def inflate(poly, radius=RADIUS):
    """the 2 * drone_radius inflation of neptune_ros.cpp:313-343: the corners' hull, counter-clockwise from the lowest leftmost point
    (for an axis-aligned square: the square grown by 2 * radius)"""
    sd = 2 * radius
    xs = [p[0] for p in poly]
    ys = [p[1] for p in poly]
    x0, x1, y0, y1 = min(xs) - sd, max(xs) + sd, min(ys) - sd, max(ys) + sd
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def rep_of(cx, cy, theta, half=0.25):
    """a rep in the manner of neptune_ros.cpp:929-984: the two points where the line through the centre at angle theta leaves the
    square's inscribed circle, (min_vert, max_vert) = (col 0, col 1)"""
    ux, uy = math.cos(theta), math.sin(theta)
    return [(cx - half * ux, cy - half * uy), (cx + half * ux, cy + half * uy)]


def world(squares, thetas=None, extra_reps=()):
    un = [square(*s) for s in squares]
    thetas = thetas if thetas is not None else [math.pi / 2] * len(squares)
    reps = [rep_of(s[0], s[1], t) for s, t in zip(squares, thetas)] + list(extra_reps)
    return dict(uninflated=un, inflated=[inflate(q) for q in un], reps=reps)


def case(name, c, w, start, goal, event, hsig0=(), cont0=None):
    return dict(name=name, cfg=c, world=w, start=tuple(map(float, start)), goal=tuple(map(float, goal)), hsig0=list(hsig0),
                cont0=[tuple(map(float, p)) for p in (cont0 if cont0 is not None else [start])], event=event)


_REF = {}


def reference(c):
    """the Python reference's result of a case, computed once"""
    key = c["name"]
    if key not in _REF:
        _REF[key] = ref.search(c["cfg"], c["world"], c["start"], c["goal"], c["hsig0"], c["cont0"])
    return _REF[key]


def _directed():
    out = []
    empty = world([])
    one = world([(4.0, 4.0)])
    out.append(case("empty_straight", cfg(), empty, (1.25, 1.25), (5.25, 1.25), lambda r: r["status"] == 1 and r["g_cells"] == 8 * 1.0 and r["n_path"] == 9))
    out.append(case("empty_diagonal", cfg(), empty, (1.25, 1.25), (4.25, 4.25), lambda r: r["status"] == 1 and r["g_cells"] == 6 * DIAG))
    out.append(case("same_cell", cfg(), empty, (1.3, 1.3), (1.4, 1.45), lambda r: r["status"] == 1 and r["n_path"] == 1 and r["pops"] == 1 and r["path"][0] == (1.3, 1.3)))
    # one obstacle in the way; the rep's ray leaves it upwards, so passing above adds an entry and passing below adds none
    above = case("obstacle_above", cfg(), one, (1.25, 4.75), (6.75, 4.75), lambda r: r["status"] == 1 and len(r["hsig"]) == 1)
    out.append(above)
    out.append(case("obstacle_below", cfg(), one, (1.25, 3.25), (6.75, 3.25), lambda r: r["status"] == 1 and r["hsig"] != reference(above)["hsig"]))
    # the same passage with the opposite entry already in the signature: the path cancels it
    sign = reference(above)["hsig"][0][1] if reference(above)["hsig"] else 1
    out.append(case("cancel", cfg(), one, (1.25, 4.75), (6.75, 4.75), lambda r: r["status"] == 1 and len(r["hsig"]) < 1, hsig0=[(1, -sign)]))
    # three obstacles and the inadmissible bias: an open node is reached again more cheaply
    three = world([(3.0, 3.25), (4.5, 4.75), (3.25, 5.5)], [0.3, 2.0, 4.0])
    out.append(case("inplace_update", cfg(), three, (0.75, 2.25), (6.75, 6.25), lambda r: r["status"] == 1 and r["n_updates"] > 0))
    # the cable, in cells against metres: 3 m to go on a 4 m cable is 6 cells + whatever the tether already counts
    out.append(case("cable_lives", cfg(cable=4.0), one, (1.25, 1.25), (4.25, 1.25),
                    lambda r: r["status"] == 1 and r["n_length_checks"] > 0 and r["n_cable_pruned"] == 0))
    out.append(case("cable_prunes", cfg(cable=3.7), one, (2.25, 4.25), (5.75, 4.25), lambda r: r["status"] == 1 and r["n_cable_pruned"] > 0, cont0=[(2.25, 4.25)]))
    out.append(case("cable_too_short", cfg(cable=2.0), one, (1.25, 1.25), (4.25, 1.25), lambda r: r["status"] == -1 and r["n_cable_pruned"] > 0))
    out.append(case("goal_in_polygon", cfg(n=12), world([(4.0, 4.0)], []), (1.25, 1.25), (4.1, 4.1), lambda r: r["status"] == -1 and r["pops"] > 100))
    out.append(case("pop_budget", cfg(max_pops=5), one, (1.25, 4.25), (6.75, 4.25), lambda r: r["status"] == 0 and r["pops"] == 5))
    out.append(case("node_pool", cfg(max_nodes=12), one, (1.25, 4.25), (6.75, 4.25), lambda r: r["nodes_used"] == 12 and r["pops"] >= 2))
    # 34 reps with 2 polygons: the last ones stand in the path, so ids beyond 31 enter the signature and power_int wraps to 0
    far = [rep_of(20.0 + k, 20.0, 1.0) for k in range(30)]
    wrap = world([(2.0, 6.0), (6.0, 6.0)], None, far + [rep_of(3.0, 0.0, math.pi / 2), rep_of(5.0, 0.0, math.pi / 2)])
    out.append(case("power_int_wraps", cfg(hsig_cap=8), wrap, (1.25, 2.25), (6.75, 2.25),
                    lambda r: r["status"] == 1 and len(wrap["reps"]) == 34 and any(i >= 32 for i, _ in r["hsig"])))
    # the caps
    out.append(case("cap_hsig", cfg(hsig_cap=1), wrap, (1.25, 2.25), (6.75, 2.25), lambda r: r["flags"] & ref.FLAG_HSIG))
    out.append(case("cap_cont", cfg(cont_cap=5), empty, (1.25, 1.25), (5.25, 1.25), lambda r: r["flags"] & ref.FLAG_CONT))
    out.append(case("cap_path", cfg(path_cap=4), empty, (1.25, 1.25), (5.25, 1.25), lambda r: r["status"] == 1 and r["flags"] & ref.FLAG_PATH and r["n_path"] == 4))
    zig = [(0.25 + 0.25 * k, 0.25 + (0.2 if k % 2 else 0.0)) for k in range(31)]
    out.append(case("cap_pool", cfg(cable=3.0, max_nodes=4, cont_cap=32), one, zig[-1], (7.25, 0.25), lambda r: r["flags"] & ref.FLAG_POOL, cont0=zig))
    return out


_DIRECTED = None


def directed():
    global _DIRECTED
    if _DIRECTED is None:
        _DIRECTED = _directed()
    return _DIRECTED


# ---- the seeded family ------------------------------------------------------------------------------------------------------------
N_FAMILY = 48

EVENTS = {
    "reached": lambda c, r: r["status"] == 1,
    "open_list_empty": lambda c, r: r["status"] == -1,
    "budget": lambda c, r: r["status"] == 0,
    "signature": lambda c, r: len(r["hsig"]) > 0,
    "cancelled": lambda c, r: r["status"] == 1 and len(r["hsig"]) < len(c["hsig0"]),
    "inplace_update": lambda c, r: r["n_updates"] > 0,
    "cable_lives": lambda c, r: r["status"] == 1 and r["n_length_checks"] > 0 and r["n_cable_pruned"] == 0,
    "cable_prunes": lambda c, r: r["n_cable_pruned"] > 0,
    "node_pool": lambda c, r: r["nodes_used"] == c["cfg"]["max_nodes"],
    "power_int_wraps": lambda c, r: any(i >= 32 for i, _ in r["hsig"]),
    "cap_hsig": lambda c, r: bool(r["flags"] & ref.FLAG_HSIG),
    "cap_cont": lambda c, r: bool(r["flags"] & ref.FLAG_CONT),
    "cap_path": lambda c, r: bool(r["flags"] & ref.FLAG_PATH),
    "cap_pool": lambda c, r: bool(r["flags"] & ref.FLAG_POOL),
    "same_cell": lambda c, r: r["status"] == 1 and r["n_path"] == 1,
    "goal_in_polygon": lambda c, r: r["status"] == -1 and any(abs(c["goal"][0] - q[0][0] - 0.55) < 0.55 and abs(c["goal"][1] - q[0][1] - 0.55) < 0.55
                                                               for q in c["world"]["inflated"]),
    "shortened_terminal": lambda c, r: r["status"] == 1 and 1 < len(r["cont"]) < r["n_path"],
}


def _family():
    rng = np.random.RandomState(20261020)
    out = []
    for k in range(N_FAMILY):
        n = int(rng.randint(12, 17))
        side = 0.5 * n
        n_poly = int(rng.randint(1, 4))
        squares = []
        while len(squares) < n_poly:
            cx, cy = rng.uniform(1.5, side - 1.5, 2)
            if all(math.hypot(cx - s[0], cy - s[1]) > 1.6 for s in squares):
                squares.append((float(cx), float(cy)))
        thetas = [float(t) for t in rng.uniform(0.0, 2 * math.pi, n_poly)]
        kind = k % 8
        extra = []
        if kind == 5:      # 34 reps: far ones, and two whose rays stand across the grid
            extra = [rep_of(30.0 + j, 30.0, 1.0) for j in range(32 - n_poly)] + [rep_of(side / 3, -1.0, math.pi / 2), rep_of(2 * side / 3, -1.0, math.pi / 2)]
        w = world(squares, thetas, extra)

        def free(p):
            return all(abs(p[0] - s[0]) > 1.0 or abs(p[1] - s[1]) > 1.0 for s in squares)
        while True:
            start = tuple(float(v) for v in rng.uniform(0.3, side - 0.3, 2))
            goal = tuple(float(v) for v in rng.uniform(0.3, side - 0.3, 2))
            if free(start) and free(goal) and (kind == 7 or math.hypot(start[0] - goal[0], start[1] - goal[1]) > 0.45 * side):
                break
        if k % 16 == 8:      # a goal inside the first inflated polygon
            goal = (squares[0][0] + 0.1, squares[0][1] - 0.1)
        dist = math.hypot(start[0] - goal[0], start[1] - goal[1])
        c = cfg(n=n)
        hsig0, cont0 = [], [start]
        if kind in (1, 2):      # a cable around the straight distance: both outcomes
            c["cable_length"] = float(dist * rng.uniform(0.8, 1.5))
        elif kind == 3:      # tight budgets
            c["max_pops"] = int(rng.randint(3, 12)) if k % 16 == 3 else 100000
            c["max_nodes"] = 0 if k % 16 == 3 else int(rng.randint(8, 30))
        elif kind == 4:      # an initial signature the path may cancel, and a tether that already has a bend
            c["cable_length"] = float(dist * rng.uniform(1.5, 2.5))
            first = ref.search(c, w, start, goal, [], [start])["hsig"]      # what the path adds first, the other way round
            hsig0 = [(first[0][0], -first[0][1])] if first else [(1, int(rng.choice([-1, 1])))]
            base = (float(np.clip(start[0] - 1.0, 0.1, side)), float(np.clip(start[1] + 1.0, 0.1, side - 0.1)))
            cont0 = [base, start]
        elif kind == 5:
            c["hsig_cap"] = 8 if k % 16 == 5 else 1
        elif kind == 6:      # small lists
            c["cont_cap"] = int(rng.randint(4, 9)) if k % 16 == 6 else 48
            c["path_cap"] = 48 if k % 16 == 6 else int(rng.randint(2, 6))
        elif kind == 7:      # a short hop on a short cable with a long tether behind it, in a small pool
            goal = (start[0] + float(rng.uniform(-0.2, 0.2)), start[1] + float(rng.uniform(-0.2, 0.2))) if k % 16 == 7 else goal
            if k % 16 == 15:
                cont0 = [(start[0] + 0.1 * j, start[1] + (0.15 if j % 2 else 0.0)) for j in range(30, 0, -1)] + [start]
                c.update(cable_length=3.0, max_nodes=4, cont_cap=32)
        out.append(case("family_%02d" % k, c, w, start, goal, None, hsig0, cont0))
    return out


_FAMILY = None


def family():
    global _FAMILY
    if _FAMILY is None:
        _FAMILY = _family()
    return _FAMILY


def family_counts():
    counts = {name: 0 for name in EVENTS}
    for c in family():
        r = reference(c)
        for name, ev in EVENTS.items():
            counts[name] += bool(ev(c, r))
    return counts


def all_cases():
    return directed() + family()


# ---- cases through the library -----------------------------------------------------------------------------------------------------
def cfg_key(c):
    return tuple(sorted(c["cfg"].items()))


def groups(cases):
    """cases that share a configuration share a handle: [(cfg, [case, ...])], each case a scene of its own"""
    by = {}
    for c in cases:
        by.setdefault(cfg_key(c), []).append(c)
    return [(g[0]["cfg"], g) for g in by.values()]


def make_handle(cfg_dict, worlds):
    from neptune_amd import hastar
    ha = hastar.HomotopicAstar(hastar.make_cfg(**cfg_dict), len(worlds))
    for s, w in enumerate(worlds):
        ha.set_statics(s, w["uninflated"], w["reps"], inflated=w["inflated"])
    return ha


def pack_inputs(ha, cases):
    n = len(cases)
    st = np.zeros(n, dtype=ha.dtype)
    for k, c in enumerate(cases):
        st["n_hsig"][k] = len(c["hsig0"])
        for e, (i, s) in enumerate(c["hsig0"]):
            st["hsig_id"][k, e] = i
            st["hsig_sign"][k, e] = s
        st["n_cont"][k] = len(c["cont0"])
        st["cont"][k, :len(c["cont0"])] = np.array(c["cont0"]).reshape(-1, 2)
    start = np.array([c["start"] for c in cases], dtype=np.float64)
    goal = np.array([c["goal"] for c in cases], dtype=np.float64)
    return start, goal, st


def expected(ha, cases, refs=None):
    """the Python reference's results in the library's arrays: (results, paths, states)"""
    from neptune_amd import abi
    n = len(cases)
    res = np.zeros(n, dtype=abi.HASTAR_RESULT_DTYPE)
    path = np.zeros((n, ha.cfg.path_cap, 2), dtype=np.float64)
    st = np.zeros(n, dtype=ha.dtype)
    for k, c in enumerate(cases):
        r = refs[k] if refs is not None else reference(c)
        for f in ("status", "n_path", "nodes_used", "pops", "n_updates", "n_length_checks", "n_cable_pruned", "flags", "g_cells", "length_m"):
            res[f][k] = r[f]
        if r["path"]:
            path[k, :len(r["path"])] = np.array(r["path"])
        st["n_hsig"][k] = len(r["hsig"])
        for e, (i, s) in enumerate(r["hsig"]):
            st["hsig_id"][k, e] = i
            st["hsig_sign"][k, e] = s
        st["n_cont"][k] = len(r["cont"])
        if r["cont"]:
            st["cont"][k, :len(r["cont"])] = np.array(r["cont"]).reshape(-1, 2)
    return res, path, st


def same_bytes(got, want):
    """(results, paths, states) against (results, paths, states), byte for byte; returns the first difference as text, or None"""
    names = ("results", "paths", "states")
    for name, g, w in zip(names, got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.dtype != w.dtype or g.shape != w.shape:
            return "%s: %s %s against %s %s" % (name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            for k in range(len(g)):
                if g[k].tobytes() != w[k].tobytes():
                    return "%s[%d]: got %r\nwant %r" % (name, k, g[k] if name != "paths" else g[k][:12], w[k] if name != "paths" else w[k][:12])
    return None
