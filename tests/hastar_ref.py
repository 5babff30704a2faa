"""A Python restatement of the reference's AstarPathFinder (neptune/src/Astar_searcher.cpp) with eu::updateHSig_orig,
eu::updateContPts_orig and eu::tetherLength_orig (neptune/src/entangle_utils.cpp), written from the reference's source: plain
Python floats, numpy.float32 for the one float norm, oracle.gjk_collision for gjk::collision, std::vector as a Python list, the node
table as a dict on (ix, iy, iz), std::priority_queue as a list under libstdc++'s push_heap / pop_heap.  The independent side of
every comparison in tests/test_hastar_cpu.py; it shares no code with neptune_amd/csrc/hastar_common.h.

What is this build's and not the reference's (include/neptune_hastar.h) is restated from that header: the budget of pops in place
of the 30 s limit, iz starting at 0, the capacities (a child over hsig_cap / cont_cap / the pool is dropped and flagged, a path
over path_cap truncated), and the counters."""
import math

import numpy as np

from oracle import oracle

FLAG_HSIG, FLAG_CONT, FLAG_PATH, FLAG_POOL, FLAG_STATE = 1, 2, 4, 8, 16
M32 = 0xFFFFFFFF


class Node:
    __slots__ = ("id", "coord", "index", "g", "f", "came_from", "hsig", "cont", "length_used")


def gjk(V1, V2):
    return oracle.gjk_collision(np.array(V1, dtype=np.float64), np.array(V2, dtype=np.float64))


def vector_wedge2(a, b, c):
    """entangle_utils.cpp:16-27 (both overloads compute the same products)"""
    ab = (b[0] - a[0], b[1] - a[1])
    ac = (c[0] - a[0], c[1] - a[1])
    return ab[0] * ac[1] - ac[0] * ab[1], ab, ac


def update_hsig(hsig, pk, pk1, reps):
    """updateHSig_orig (:1279-1354) on a list of (id, sign) tuples, in place"""
    to_add = []
    for i, rep in enumerate(reps):
        pbi, pik = rep[0], rep[1]      # col(0), col(1)
        c1, pik_pk, pbi_pk = vector_wedge2(pk, pik, pbi)
        c2 = (pik[0] - pk1[0]) * (pbi[1] - pk1[1]) - (pbi[0] - pk1[0]) * (pik[1] - pk1[1])
        if c1 * c2 < 0:
            if abs(pik_pk[1] * pbi_pk[1]) > abs(pik_pk[0] * pbi_pk[0]):
                a = pik_pk[1] / pbi_pk[1]
            else:
                a = pik_pk[0] / pbi_pk[0]
            if a < 0:
                pass
            elif a < 1:
                to_add.append((i + 1, 1 if c1 < 0 else -1))
    have = True
    while have:
        have = False
        for i in range(len(to_add)):
            # the j loop examines the list's last entry only: it breaks after its first pass (:1341)
            j = len(hsig) - 1
            if j >= 0 and hsig[j][0] == to_add[i][0] and hsig[j][1] != to_add[i][1]:
                del to_add[i]
                del hsig[j]
                have = True
                break
    hsig.extend(to_add)


def update_cont_pts(cont, uninflated):
    """updateContPts_orig (:1356-1401): returns the new list"""
    interval = 0.2
    new = [cont[0]]
    cur = cont[0]
    prev = cur
    for i in range(len(cont) - 1):
        A, B = cont[i], cont[i + 1]
        norm = math.sqrt((A[0] - B[0]) * (A[0] - B[0]) + (A[1] - B[1]) * (A[1] - B[1]))
        ratio = int(math.floor(norm / interval))
        for j in range(1, ratio + 1):
            s = float(j) * interval
            pt = (A[0] + s * (B[0] - A[0]) / norm, A[1] + s * (B[1] - A[1]) / norm)
            for poly in uninflated:
                if gjk(poly, [cur, pt]):
                    cur = prev
                    new.append(cur)
                    break
            prev = pt
        for poly in uninflated:
            if gjk(poly, [cur, B]):
                cur = prev
                new.append(cur)
                break
        prev = B
    new.append(cont[-1])
    return new


def tether_length(cont):
    length = 0.0
    for i in range(len(cont) - 1):
        dx, dy = cont[i + 1][0] - cont[i][0], cont[i + 1][1] - cont[i][1]
        length += math.sqrt(dx * dx + dy * dy)
    return length


def power_int(base, exponent):
    """Astar_searcher.cpp:184-199 in unsigned 32-bit arithmetic"""
    if exponent == 0:
        return 1
    if base < 2:
        return base
    result, term = 1, base
    while True:
        if exponent % 2 != 0:
            result = (result * term) & M32
        exponent //= 2
        if exponent == 0:
            break
        term = (term * term) & M32
    return result


def get_iz(hsig):
    iz = 0
    for i, (idx, sign) in enumerate(hsig):
        iz = (iz + (i + 1) * power_int(2, idx) + sign) & M32
    return iz


class Heap:
    """std::priority_queue over libstdc++'s heap (bits/stl_heap.h), comp = CompareCost"""

    def __init__(self):
        self.c = []

    @staticmethod
    def comp(left, right):
        if abs(left.f - right.f) < 1e-5:
            return left.f - left.g > right.f - right.g
        return left.f > right.f

    def _push_heap(self, hole, top, value):
        c = self.c
        parent = (hole - 1) // 2
        while hole > top and self.comp(c[parent], value):
            c[hole] = c[parent]
            hole = parent
            parent = (hole - 1) // 2
        c[hole] = value

    def push(self, value):
        self.c.append(value)
        self._push_heap(len(self.c) - 1, 0, value)

    def pop(self):
        c = self.c
        top = c[0]
        if len(c) > 1:
            value = c[-1]
            c[-1] = c[0]
            length = len(c) - 1
            hole = second = 0
            while second < (length - 1) // 2:
                second = 2 * (second + 1)
                if self.comp(c[second], c[second - 1]):
                    second -= 1
                c[hole] = c[second]
                hole = second
            if length % 2 == 0 and second == (length - 2) // 2:
                second = 2 * (second + 1)
                c[hole] = c[second - 1]
                hole = second - 1
            self._push_heap(hole, 0, value)
        c.pop()
        return top


def c_int(v):
    return int(v)      # truncation toward zero, as a C cast of a double in range


def search(cfg, world, start, goal, hsig0, cont0):
    """cfg: a dict of nep_hastar_cfg's fields; world: dict(inflated, uninflated, reps); hsig0 a list of (id, sign); cont0 a list of
    points.  Returns a dict: status, counters, flags, g_cells, length_m, path, hsig, cont (the terminal state)."""
    res = cfg["resolution"]
    inv = 1.0 / res
    xl, yl = cfg["x_min"], cfg["y_min"]
    GLX = c_int((cfg["x_max"] - xl) * inv)
    GLY = c_int((cfg["y_max"] - yl) * inv)
    GLZ = c_int((cfg["z_max"] - cfg["z_min"]) * inv)
    pool_nodes = cfg["max_nodes"] if cfg["max_nodes"] > 0 else GLX * GLY * GLZ
    pool_pts = max(8 * pool_nodes, cfg["cont_cap"])
    cable, bias = cfg["cable_length"], cfg["bias"]
    inflated, uninflated, reps = world["inflated"], world["uninflated"], world["reps"]
    out = dict(status=-1, n_path=0, nodes_used=0, pops=0, n_updates=0, n_length_checks=0, n_cable_pruned=0, flags=0, g_cells=0.0,
               length_m=0.0, path=[], hsig=list(hsig0), cont=list(cont0))
    pts = [tuple(start), tuple(goal)] + [tuple(p) for p in cont0]
    if len(hsig0) > cfg["hsig_cap"] or len(cont0) < 1 or len(cont0) > cfg["cont_cap"] or not all(abs(v) <= 100000.0 for p in pts for v in p):
        out["flags"] |= FLAG_STATE
        out["hsig"], out["cont"] = [], []
        return out

    def coord2idx(pt):
        return (min(max(c_int((pt[0] - xl) * inv), 0), GLX - 1), min(max(c_int((pt[1] - yl) * inv), 0), GLY - 1))

    def idx2coord(idx):
        return ((float(idx[0]) + 0.5) * res + xl, (float(idx[1]) + 0.5) * res + yl)

    def occupied(idx):
        if idx[0] < 0 or idx[0] >= GLX or idx[1] < 0 or idx[1] >= GLY:
            return True
        c = idx2coord(idx)
        r = 0.05
        cps = [(c[0] + r, c[1] + r), (c[0] + r, c[1] - r), (c[0] - r, c[1] + r), (c[0] - r, c[1] - r)]
        for poly in inflated:
            if gjk(poly, cps):
                return True
        return False

    start_idx, end_idx = coord2idx(start), coord2idx(goal)

    def heu(idx):
        dx, dy = float(idx[0]) - float(end_idx[0]), float(idx[1]) - float(end_idx[1])
        h = math.sqrt(dx * dx + dy * dy)
        h *= 1.01
        return h

    nodes_used = 1
    pool_used = len(cont0)
    s = Node()
    s.index, s.g, s.f, s.id, s.coord = start_idx, 0.0, bias * heu(start_idx), 1, (float(start[0]), float(start[1]))
    s.hsig, s.cont, s.length_used, s.came_from = list(hsig0), list(cont0), tether_length(cont0), None
    heap = Heap()
    heap.push(s)
    table = {(start_idx[0], start_idx[1], 0): s}
    terminal = None
    while True:
        if not heap.c:
            out["status"] = -1
            break
        if out["pops"] >= cfg["max_pops"]:
            out["status"] = 0
            break
        cur = heap.pop()
        out["pops"] += 1
        cur.id = -1
        if cur.index == end_idx:
            out["status"] = 1
            terminal = cur
            break
        ended = False
        for i in (-1, 0, 1):
            if ended:
                break
            for j in (-1, 0, 1):
                if i == 0 and j == 0:
                    continue
                nidx = (cur.index[0] + i, cur.index[1] + j)
                offset_cost = float(np.sqrt(np.float32(i) * np.float32(i) + np.float32(j) * np.float32(j), dtype=np.float32))
                if occupied(nidx):
                    continue
                hsig = list(cur.hsig)
                pk1 = idx2coord(nidx)
                update_hsig(hsig, cur.coord, pk1, reps)
                if len(hsig) > cfg["hsig_cap"]:
                    out["flags"] |= FLAG_HSIG
                    continue
                cont = list(cur.cont)
                cont.append(pk1)
                if len(cont) > cfg["cont_cap"]:
                    out["flags"] |= FLAG_CONT
                    continue
                length_used = cur.length_used + offset_cost
                shortened = False
                if length_used > cable:
                    out["n_length_checks"] += 1
                    cont = update_cont_pts(cont, uninflated)
                    room = pool_pts - pool_used
                    if len(cont) > min(room, cfg["cont_cap"]):
                        out["flags"] |= FLAG_POOL if room < cfg["cont_cap"] else FLAG_CONT
                        continue
                    length_used = tether_length(cont)
                    if length_used > cable:
                        out["n_cable_pruned"] += 1
                        continue
                    shortened = True
                iz = get_iz(hsig)
                nd = table.get((nidx[0], nidx[1], iz))
                if nd is None:
                    if nodes_used >= pool_nodes:
                        ended = True
                        break
                    nodes_used += 1
                    nd = Node()
                    nd.id, nd.index = 1, nidx
                    nd.g = offset_cost + cur.g
                    nd.f = nd.g + bias * heu(nidx)
                    nd.came_from, nd.coord, nd.hsig, nd.cont, nd.length_used = cur, pk1, hsig, cont, length_used
                    heap.push(nd)
                    table[(nidx[0], nidx[1], iz)] = nd
                    if shortened:
                        pool_used += len(cont)
                elif nd.id == 1:
                    new_g = offset_cost + cur.g
                    if nd.g > new_g:
                        nd.g = new_g
                        nd.f = new_g + bias * heu(nd.index)
                        nd.came_from, nd.hsig, nd.cont, nd.length_used = cur, hsig, cont, length_used
                        out["n_updates"] += 1
                        if shortened:
                            pool_used += len(cont)
    out["nodes_used"] = nodes_used
    if terminal is not None:
        chain = []
        g = terminal
        while g.came_from is not None:
            chain.append(g)
            g = g.came_from
        chain.append(g)
        path = [n.coord for n in reversed(chain)]
        if len(path) > cfg["path_cap"]:
            out["flags"] |= FLAG_PATH
            path = path[:cfg["path_cap"]]
        out["path"] = path
        out["n_path"] = len(path)
        out["length_m"] = tether_length(path)
        out["g_cells"] = terminal.g
        out["hsig"], out["cont"] = list(terminal.hsig), list(terminal.cont)
    return out
