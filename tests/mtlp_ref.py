"""A Python restatement of the reference's MTLP comparator, written from neptune/src/solveMultiLinearPath.cpp and
solveMultiLinearPath.hpp: the order graph (:31-98), the cable lines of each robot (:169-194, with the order of the robots
0 .. N-1 because the ordering loop never runs), AstarGraphSearch / AstarGetSucc (:523-680) and getPath (:682-707).

The CGAL tests (cgal_utils.cpp:199-258, intersectSphereSegment) are do_intersect on an exact-predicates kernel: the verdict of the
closed point sets.  Here they are evaluated in fractions.Fraction on the doubles' exact values, by explicit constructions (the
point where a segment meets a plane, the parameter interval a triangle's edges leave of a coplanar segment, the parameters at which
two lines meet) — not by the orientation signs the library uses.  A triangle with collinear points is the closed hull of its points;
the sphere is read as the ball.  The heap is libstdc++'s, as tests/hastar_ref.py restates it."""
from fractions import Fraction as Fr

import numpy as np

from hastar_ref import Heap

FLAG_PATH, FLAG_STATE, FLAG_DEGEN = 1, 2, 4
Z3 = (0, 0, 0)
COST = [0.0] + [float(np.sqrt(np.float32(n))) for n in (1, 2, 3)]      # offsetIndex.cast<float>().lpNorm<2>(), widened


def F3(p):
    return (Fr(float(p[0])), Fr(float(p[1])), Fr(float(p[2])))


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def point_on_seg(x, u, v):
    d, xu = sub(v, u), sub(x, u)
    return cross(xu, d) == Z3 and 0 <= dot(xu, d) <= dot(d, d)


def seg_seg(p, q, u, v):
    """closed segments of R3 (either may be a point)"""
    dq, du, pu = sub(q, p), sub(v, u), sub(u, p)
    w = cross(dq, du)
    if w != Z3:      # two lines that are not parallel: they meet when coplanar, at p + s dq = u + t du
        if dot(pu, w) != 0:
            return False
        ww = dot(w, w)
        s, t = dot(cross(pu, du), w) / ww, dot(cross(pu, dq), w) / ww
        return 0 <= s <= 1 and 0 <= t <= 1
    if dq == Z3 and du == Z3:
        return p == u
    if dq == Z3:
        return point_on_seg(p, u, v)
    if du == Z3:
        return point_on_seg(u, p, q)
    if cross(pu, dq) != Z3:      # parallel, apart
        return False
    dd = dot(dq, dq)
    a, b = dot(pu, dq) / dd, dot(sub(v, p), dq) / dd
    return max(a, b) >= 0 and min(a, b) <= 1


def seg_tri(p, q, a, b, c, ev=None):
    """closed segment p q against the closed hull of a, b, c (Fractions)"""
    n = cross(sub(b, a), sub(c, a))
    if n == Z3:
        d = sub(b, a) if b != a else sub(c, a)
        if d == Z3:
            u = v = a
        else:
            u = min((a, b, c), key=lambda x: dot(sub(x, a), d)); v = max((a, b, c), key=lambda x: dot(sub(x, a), d))
        return seg_seg(p, q, u, v)
    sp, sq = dot(n, sub(p, a)), dot(n, sub(q, a))
    if sp * sq > 0:
        return False
    edges = ((a, b), (b, c), (c, a))
    inward = [cross(n, sub(e1, e0)) for e0, e1 in edges]
    if sp == 0 and sq == 0:      # in the plane: what the three edges leave of the parameter interval [0, 1]
        if ev is not None:
            ev.add("coplanar")
        lo, hi, d = Fr(0), Fr(1), sub(q, p)
        for (e0, _), m in zip(edges, inward):
            f0, fd = dot(m, sub(p, e0)), dot(m, d)
            if fd == 0:
                if f0 < 0:
                    return False
            elif fd > 0:
                lo = max(lo, -f0 / fd)
            else:
                hi = min(hi, -f0 / fd)
        return lo <= hi
    t = sp / (sp - sq)
    d = sub(q, p)
    x = (p[0] + t * d[0], p[1] + t * d[1], p[2] + t * d[2])
    f = [dot(m, sub(x, e0)) for (e0, _), m in zip(edges, inward)]
    if min(f) < 0:
        return False
    if ev is not None:
        if x in (a, b, c):
            ev.add("touch_vertex")
        elif min(f) == 0:
            ev.add("touch_edge")
        if t == 0 or t == 1:
            ev.add("touch_end")
    return True


def tri_tri(A, B):
    return any(seg_tri(A[k], A[(k + 1) % 3], *B) for k in range(3)) or any(seg_tri(B[k], B[(k + 1) % 3], *A) for k in range(3))


def seg_seg_2d(p, q, u, v):
    flat = lambda x: (x[0], x[1], Fr(0))      # noqa: E731
    return seg_seg(flat(p), flat(q), flat(u), flat(v))


def ball_seg(c, r2, p, q, ev=None):
    """(meets the closed ball, lies wholly inside the open ball)"""
    dp, dq = dot(sub(p, c), sub(p, c)), dot(sub(q, c), sub(q, c))
    d, pc = sub(q, p), sub(c, p)
    t = Fr(0) if d == Z3 else min(Fr(1), max(Fr(0), dot(pc, d) / dot(d, d)))
    x = (p[0] + t * d[0], p[1] + t * d[1], p[2] + t * d[2])
    d2 = dot(sub(x, c), sub(x, c))
    if ev is not None and d2 == r2:
        ev.add("ball_tangent")
    return d2 <= r2, dp < r2 and dq < r2


def in_domain(x):
    x = float(x)
    return np.isfinite(x) and abs(x) <= 1e5 and (Fr(x) * 2**60).denominator == 1


def graph_visit(bases, sg, i, j):
    """what the visit (i, j) sets, as a set of (row, col), and the branch it took"""
    A = (F3(bases[i]), F3(sg[i][0]), F3(sg[i][1])); B = (F3(bases[j]), F3(sg[j][0]), F3(sg[j][1]))
    if not tri_tri(A, B):
        return {(i, j), (j, i)}, "apart"
    baseline = seg_seg_2d(A[1], A[2], B[1], B[2])
    sA, eA = seg_tri(A[0], A[1], *B), seg_tri(A[0], A[2], *B)
    sB, eB = seg_tri(B[0], B[1], *A), seg_tri(B[0], B[2], *A)
    if not baseline:
        if sA and eA or sB and eB:
            return set(), "type1"
        elif sA and sB or eB and eA:
            return set(), "type2"
        elif sA and eB:
            return {(i, j)}, "type3_a_first"
        elif sB and eA:
            return {(j, i)}, "type3_b_first"
        return set(), "no_type"
    if eA:
        return {(j, i)}, "cross_end_a"
    elif eB:
        return {(i, j)}, "cross_end_b"
    elif sA:
        return {(i, j)}, "cross_start_a"
    elif sB:
        return {(j, i)}, "cross_start_b"
    return set(), "cross_none"


def order_graph(bases, sg):
    n = len(bases)
    g = np.eye(n, dtype=np.int32)
    branches = {}
    for i in range(n):
        for j in range(n):
            ones, br = graph_visit(bases, sg, i, j)
            branches[(i, j)] = br
            for (a, b) in ones:
                g[a, b] = 1
    return g, branches


def cable_lines(bases, sg, graph, i):
    lines = []
    for j in range(len(bases)):
        if j == i:
            continue
        if j < i:      # order_of_j < i, and the order is the index
            if graph[j, i] == 1:
                continue
            lines.append((bases[j], sg[j][1]))
        else:
            lines.append((bases[j], sg[j][0]))
    return lines


class Node:
    __slots__ = ("idx", "g", "f", "came", "closed", "coord")


def c_int(v):
    return int(v)


def search(cfg, base, start, goal, lines):
    """cfg: a dict of nep_mtlp_cfg's fields.  Returns a dict of nep_mtlp_result's fields, `path` and `events`."""
    res_, inv = cfg["resolution"], 1.0 / cfg["resolution"]
    lo = (cfg["x_min"], cfg["y_min"], cfg["z_min"]); hi = (cfg["x_max"], cfg["y_max"], cfg["z_max"])
    gl = [int((hi[k] - lo[k]) * inv) for k in range(3)]
    pool = cfg["max_nodes"] if cfg["max_nodes"] > 0 else gl[0] * gl[1] * gl[2]
    r2 = Fr(cfg["radius"] * cfg["radius"])
    ev = set()
    to_idx = lambda pt: tuple(min(max(c_int((pt[k] - lo[k]) * inv), 0), gl[k] - 1) for k in range(3))      # noqa: E731
    centre = lambda idx: tuple((float(idx[k]) + 0.5) * res_ + lo[k] for k in range(3))      # noqa: E731
    s_idx, g_idx = to_idx(start), to_idx(goal)
    goal_height = goal[2]
    heu = lambda idx: float(np.sqrt(float(sum((idx[k] - g_idx[k]) ** 2 for k in range(3)))))      # noqa: E731
    Fb, Fl = F3(base), [(F3(a), F3(b)) for a, b in lines]
    out = dict(status=-1, n_path=0, nodes_used=0, pops=0, n_updates=0, flags=0, n_degenerate=0, n_ball_only=0, g_cells=0.0, path=[], events=ev)
    s = Node(); s.idx = s_idx; s.g = 0.0; s.f = cfg["bias"] * heu(s_idx); s.came = None; s.closed = False; s.coord = tuple(float(v) for v in start)
    table = {s_idx: s}
    heap = Heap(); heap.push(s)
    used = 1
    terminal = None
    while True:
        if not heap.c:
            out["status"] = -1; break
        if out["pops"] >= cfg["max_pops"]:
            out["status"] = 0; break
        cur = heap.pop(); out["pops"] += 1
        cur.closed = True
        if cur.idx == g_idx:
            out["status"] = 1; terminal = cur; cur.coord = centre(g_idx); break
        Fc = F3(cur.coord)
        full = False
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                for k in (-1, 0, 1):
                    if i == 0 and j == 0 and k == 0:
                        continue
                    nidx = (cur.idx[0] + i, cur.idx[1] + j, cur.idx[2] + k)
                    pk1 = centre(nidx)
                    if pk1[2] > goal_height:
                        ev.add("above_goal"); continue
                    Fn = F3(pk1)
                    if cross(sub(Fn, Fb), sub(Fc, Fb)) == Z3:
                        out["n_degenerate"] += 1
                    blocked = False
                    for (la, lb) in Fl:      # every line is evaluated (the counters are over the whole block); the verdict is the OR
                        hit, inside = ball_seg(Fn, r2, lb, la, ev)
                        out["n_ball_only"] += int(inside)
                        if seg_tri(la, lb, Fb, Fn, Fc, ev) or hit:
                            blocked = True
                    if blocked:
                        ev.add("blocked"); continue
                    if full:      # the reference has returned; the counters above are over the whole block of an expansion
                        continue
                    if any(nidx[d] < 0 or nidx[d] >= gl[d] for d in range(3)):
                        ev.add("offgrid")
                    nd = table.get(nidx)
                    cost = COST[abs(i) + abs(j) + abs(k)]
                    if nd is None:
                        if used >= pool:
                            ev.add("pool_full"); full = True; continue      # `return`
                        nd = Node(); used += 1
                        nd.idx = nidx; nd.g = cost + cur.g; nd.f = nd.g + cfg["bias"] * heu(nidx); nd.came = cur; nd.closed = False; nd.coord = pk1
                        heap.push(nd); table[nidx] = nd
                    elif not nd.closed:
                        g = cost + cur.g
                        if nd.g > g:
                            nd.g = g; nd.f = g + cfg["bias"] * heu(nidx); nd.came = cur
                            out["n_updates"] += 1
                            c = heap.c
                            if any(Heap.comp(c[(h - 1) // 2], c[h]) for h in range(1, len(c))):
                                ev.add("heap_out_of_order")
    out["nodes_used"] = used
    if out["n_degenerate"]:
        out["flags"] |= FLAG_DEGEN
    if terminal is not None:
        path = []
        n = terminal
        while n is not None:
            path.append(n.coord); n = n.came
        path.reverse()
        if len(path) > cfg["path_cap"]:
            out["flags"] |= FLAG_PATH; path = path[:cfg["path_cap"]]
        out["path"] = path; out["n_path"] = len(path); out["g_cells"] = terminal.g
    return out


def solve(cfg, bases, sg):
    """one run: dict(graph, run_status, results [N], branches, lines)"""
    n = len(bases)
    if not all(in_domain(v) for v in np.asarray(bases, dtype=np.float64).ravel()) or not all(in_domain(v) for v in np.asarray(sg, dtype=np.float64).ravel()):
        bad = dict(status=-1, n_path=0, nodes_used=0, pops=0, n_updates=0, flags=FLAG_STATE, n_degenerate=0, n_ball_only=0, g_cells=0.0, path=[], events=set())
        return dict(graph=np.zeros((n, n), dtype=np.int32), run_status=-2, results=[dict(bad) for _ in range(n)], branches={}, lines=[[] for _ in range(n)])
    bases = [tuple(float(v) for v in b) for b in bases]
    sg = [(tuple(float(v) for v in p[0]), tuple(float(v) for v in p[1])) for p in sg]
    graph, branches = order_graph(bases, sg)
    lines = [cable_lines(bases, sg, graph, i) for i in range(n)]
    results = [search(cfg, bases[i], sg[i][0], sg[i][1], lines[i]) for i in range(n)]
    return dict(graph=graph, run_status=1, results=results, branches=branches, lines=lines)
