"""TEST INFRASTRUCTURE ONLY — KinodynamicSearch::run (kinodynamic_search.cpp:1629-1827) restated in Python, without and with
enable_entangle_check.  Nothing under neptune_amd/ imports this module, and it shares no code with the kernel it checks
(frontend_astar_ent_kernel).

With ent=None it is orc_frontend_astar (oracle/neptune_oracle.c) rule for rule: tests/test_astar_ent_ref_cpu.py holds it to
that byte for byte, which pins the search mechanics below — fe_child, libstdc++'s heap arithmetic, the voxel table, the update
toggle, the closest-so-far node.  With ent (the dict helpers.ent_inputs makes) every child additionally runs
entanglesWithOtherAgents as oracle/entangle_oracle.py states it, piece by piece (the pieces are pinned by tests/test_oracle_entangle.py),
and the rules of the module docstring of the kernel's header apply: the costs' penalties, the (ix, iy, iz) voxel, the base squares,
the valid end point, the case block.

Stated deviation (the same three numbers as the device's fixed record, so that a flagged search still compares): a child whose
list would outgrow NEP_FE_ENT_CAP entries, whose sampled step would add more than 32 crossings or whose bend points would exceed
NEP_MAX_BEND is dropped and sets ent_overflow; it is not counted in n_entangled."""
import math

import numpy as np

from neptune_amd import abi
from oracle import entangle_oracle as eo
from oracle import oracle

MAX_NODES = 20000                 # node_num_max_ (kinodynamic_search.hpp:345)
ADD_CAP = 32                      # new crossings of one sampled step
GOAL, BUDGET, EMPTY, NO_SOLUTION = 1, 0, 2, 3
PAD_POOL = 16                     # nep_fe_result._pad bit 4


class _Node:
    __slots__ = ("prev", "state", "index", "g", "h", "end", "cx", "cy", "vx", "vy", "iz", "ent")


class _Add(list):
    """the crossings of one sampled step with the device's capacity: a push beyond ADD_CAP entries is refused and remembered"""
    overflow = False

    def append(self, x):
        if len(self) < ADD_CAP:
            list.append(self, x)
        else:
            self.overflow = True


def _cround(x):
    """C's round(): half away from zero"""
    r = math.floor(abs(x))
    if abs(x) - r >= 0.5:
        r += 1
    return int(-r if x < 0 else r)


def _child(p, fe, pb_own, pe, first, jx, jy, goal):
    """fe_child of oracle/neptune_oracle.c (the child tests of both expandAndAddToQueue overloads, :1045-1160, :1240-1340)
    -> (end[6], cx, cy, dist, vx, vy) or None"""
    tau = p.T_span
    j_min, j_max, v_max, v_min, a_max, a_min = -fe.j_max, fe.j_max, p.v_max, -p.v_max, p.a_max, -p.a_max
    delta = (j_max - j_min) / (fe.num_samples - 1)
    ji = (j_min + jx * delta, j_min + jy * delta)
    e = [0.0] * 6
    for ax in range(2):
        q, v, a, j = pe[ax], pe[2 + ax], pe[4 + ax], ji[ax]
        e[ax] = ((q + v * tau) + ((a * tau) * tau) / 2) + (((j * tau) * tau) * tau) / 6
        e[2 + ax] = (v + a * tau) + ((j * tau) * tau) / 2
        e[4 + ax] = a + j * tau
    n2 = 0.0
    for i in range(6):
        n2 += (e[i] - pe[i]) * (e[i] - pe[i])
    if n2 < 0.00001 * 0.00001:
        return None
    if e[5] > a_max or e[5] < a_min or e[4] > a_max or e[4] < a_min:
        return None
    cx = [ji[0] / 6, pe[4] / 2, pe[2], pe[0]]
    cy = [ji[1] / 6, pe[5] / 2, pe[3], pe[1]]
    Qx = oracle.pos_ctrl_pts(cx, tau); Qy = oracle.pos_ctrl_pts(cy, tau)
    for i in range(4):
        if Qx[i] < p.x_min or Qx[i] > p.x_max or Qy[i] < p.y_min or Qy[i] > p.y_max:
            return None
        if (Qx[i] - pb_own[0]) * (Qx[i] - pb_own[0]) + (Qy[i] - pb_own[1]) * (Qy[i] - pb_own[1]) > fe.cable_length * fe.cable_length:
            return None
    if not first:
        Vx = oracle.vel_ctrl_pts(cx, tau); Vy = oracle.vel_ctrl_pts(cy, tau)
        for i in range(3):
            if Vx[i] < v_min or Vx[i] > v_max or Vy[i] < v_min or Vy[i] > v_max:
                return None
    for ax in range(2):
        a, v = e[4 + ax], e[2 + ax]
        if a > 0 and v - ((0.5 * a) * a) / j_min > v_max:
            return None
        elif a < 0 and v - ((0.5 * a) * a) / j_max < v_min:
            return None
    dist = math.sqrt((e[0] - goal[0]) * (e[0] - goal[0]) + (e[1] - goal[1]) * (e[1] - goal[1]))
    return e, cx, cy, dist, _cround(e[0] / fe.voxel_size), _cround(e[1] / fe.voxel_size)


def _initial_z(p0, v0, a0, z_final, T, n, v_max, a_max):
    """Neptune::getInitialZPwp as fe_initial_z of oracle/neptune_oracle.c states it -> [n][4]"""
    if n < 3:
        return [[0.0, 0.0, 0.0, p0] for _ in range(n)]
    v0 = -v_max if v0 < -v_max else (v_max if v0 > v_max else v0)
    a0 = -a_max if a0 < -a_max else (a_max if a0 > a_max else a0)
    q = [0.0] * (n + 3); v = [0.0] * (n + 2)
    q[0] = p0
    q[1] = p0 + T * v0 / 3
    q[2] = (3 * 3 * q[1] - 2 * T * (-a0 * T + v0) - 3 * (q[1] + (-2 * T) * v0)) / 6
    q[n] = z_final
    inc = (z_final - q[2]) / (n - 2)
    for i in range(3, n):
        q[i] = q[i - 1] + inc
    for i in range(3, n + 1):
        v[i - 1] = (q[i] - q[i - 1]) / T
        if v[i - 1] > v_max:
            q[i] = q[i - 1] + v_max * T; v[i - 1] = v_max
        elif v[i - 1] < -v_max:
            q[i] = q[i - 1] - v_max * T; v[i - 1] = -v_max
    for i in range(2, n):
        a_i = (v[i] - v[i - 1]) / T
        if a_i > a_max:
            v[i] = v[i - 1] + a_max * T
        elif a_i < -a_max:
            v[i] = v[i - 1] - a_max * T
        q[i + 1] = q[i] + v[i] * T
    q[n + 1] = q[n]; q[n + 2] = q[n]
    co = []
    for i in range(n):
        s = q[i:i + 4]
        c0 = (((1.0 / 6.0) * s[0] + (4.0 / 6.0) * s[1]) + (1.0 / 6.0) * s[2]) + (0.0 / 6.0) * s[3]
        c1 = (((-3.0 / 6.0) * s[0] + (0.0 / 6.0) * s[1]) + (3.0 / 6.0) * s[2]) + (0.0 / 6.0) * s[3]
        c2 = (((3.0 / 6.0) * s[0] + (-6.0 / 6.0) * s[1]) + (3.0 / 6.0) * s[2]) + (0.0 / 6.0) * s[3]
        c3 = (((-1.0 / 6.0) * s[0] + (3.0 / 6.0) * s[1]) + (-3.0 / 6.0) * s[2]) + (1.0 / 6.0) * s[3]
        co.append([(1 / (T * T * T)) * c3, (1 / (T * T)) * c2, (1 / T) * c1, 1.0 * c0])
    return co


# ---- the entangle state of a node --------------------------------------------------------------------------------------------
def state_of(rec, n_ids):
    """eo.EntState from one FE_ENT_STATE_DTYPE record (None: empty); n_ids = num_agents + statics"""
    st = eo.EntState(n_ids)
    if rec is None:
        return st
    na, nb = int(rec["n_alpha"]), int(rec["n_bend"])
    for i in range(na):
        t = (int(rec["id"][i]), int(rec["cs"][i]))
        st.alphas.append(t); st.betas.append(float(rec["beta"][i])); st.active[t[0] - 1] += 1
    st.bend = [int(rec["bend"][i]) for i in range(nb)]
    return st


def _copy(st):
    c = eo.EntState(0)
    c.alphas = list(st.alphas); c.betas = list(st.betas); c.bend = list(st.bend); c.active = list(st.active)
    return c


def _entangles(su, st, cx, cy, end, index):
    """entanglesWithOtherAgents (kinodynamic_search.cpp:707-895) on st, from the pieces of oracle/entangle_oracle.py in the order of
    its entangles_with_other_agents, with the three capacities between them -> (0 fine / 1 entangled / 2 capacity, arc length)"""
    base = su.pb[su.id - 1]
    S = len(su.static_rep)
    pk = (cx[3], cy[3]); pk1 = pk
    arc = 0.0
    old = list(st.active)
    for j in range(1, su.ns + 1):
        add = _Add()
        if j < su.ns:
            t = su.T * j / su.ns
            tt = (t * t * t, t * t, t, 1.0)
            pk1 = (((cx[0] * tt[0] + cx[1] * tt[1]) + cx[2] * tt[2]) + cx[3] * tt[3], ((cy[0] * tt[0] + cy[1] * tt[1]) + cy[2] * tt[2]) + cy[3] * tt[3])
        else:
            pk1 = (end[0], end[1])
        arc += eo._norm(pk1, pk)
        for i in range(su.N):
            if i == su.id - 1 or not su.present[i]:
                continue
            if index > su.num_pol:
                pik = su.sampled[i][su.num_pol - 1][su.ns]; pik1 = pik
            else:
                pik = su.sampled[i][index - 1][j - 1]; pik1 = su.sampled[i][index - 1][j]
            eo.hsig_to_add_agent(add, pk, pk1, pik, pik1, base, su.bendpts[i], i + 1)
        eo.hsig_to_add_static(add, pk, pk1, su.static_rep, su.N)
        if add.overflow:
            return 2, arc
        if len(st.alphas) + len(add) > su.N + S:
            return 1, arc
        eo.add_alpha_beta_to_list(add, st, pk, su.pb, base, su.static_rep, su.N, su.bendpts)
        if len(st.alphas) > abi.NEP_FE_ENT_CAP:
            return 2, arc
        for i in range(su.N):
            if old[i] < 2 and st.active[i] >= 2:
                return 1, arc
            elif old[i] >= 2 and st.active[i] > old[i]:
                return 1, arc
        eo.update_bend_pts(st, pk1, su.pb, base, su.static_rep, su.N)
        if len(st.bend) > abi.NEP_MAX_BEND:
            return 2, arc
        old = list(st.active)
        pk = pk1
    if eo.tether_length(st, su.pb, base, pk1, su.static_rep, su.static_longest, su.N) > su.cable:
        return 1, arc
    return 0, arc


def _iz(st):
    """getIz (:2006-2014) with power_int (:2016-2031) in 32-bit unsigned arithmetic"""
    M = 0xFFFFFFFF
    iz = 0
    for i, (idv, cs) in enumerate(st.alphas):
        base, ex = idv & M, cs & M
        if ex == 0:
            r = 1
        elif base < 2:
            r = base
        else:
            r, term = 1, base
            while True:
                if ex % 2:
                    r = (r * term) & M
                ex //= 2
                if ex == 0:
                    break
                term = (term * term) & M
        iz = (iz + (i + 1) * r) & M
    return iz


def _case_row(st, N):
    row = [0] * N
    for j in range(N):
        if st.active[j] != 1:
            continue
        for a in st.alphas:
            if a[0] == j + 1:
                row[j] = a[1]
    return row


# ---- the search ----------------------------------------------------------------------------------------------------------------
def astar(p, fe, agent, start, hulls, statics, max_pops, order=None, max_nodes=MAX_NODES, ent=None, init=None):
    """agent: 1-based id; start: one FE_START_DTYPE record; hulls: (hull_xy [N][num_pol][16][2], hull_nv [N][num_pol]) of
    oracle.hulls_of_scene; ent: helpers.ent_inputs(...) or None (entangle check off); init: the state at A, one FE_ENT_STATE_DTYPE
    record (None: ent["init"], else empty).
    -> (guess record, result dict, case block [NEP_MAX_POL][N] int32, coverage counters dict)"""
    hull_xy, hull_nv = hulls
    N, D, ns = p.num_agents, p.num_pol, fe.num_samples
    own = agent - 1
    pb = np.asarray(p.pb, dtype=np.float64).reshape(N, 2)
    pb_own = (float(pb[own][0]), float(pb[own][1]))
    goal = (float(start["goal"][0]), float(start["goal"][1]))
    root = [float(start["pos"][0]), float(start["pos"][1]), float(start["vel"][0]), float(start["vel"][1]), float(start["accel"][0]), float(start["accel"][1])]
    bias = fe.bias
    su = None
    if ent is not None:
        S = len(np.asarray(ent["reps"]).reshape(-1, 2, 2))
        reps = [[tuple(map(float, r[0])), tuple(map(float, r[1]))] for r in np.asarray(ent["reps"], dtype=np.float64).reshape(-1, 2, 2)]
        longest = np.asarray(ent["longest"], dtype=np.float64).reshape(-1, 2).tolist()
        sampled = [[[tuple(map(float, q)) for q in row] for row in ag] for ag in np.asarray(ent["sampled"], dtype=np.float64)]
        bendpts = [[tuple(map(float, ent["bend_xy"][j][k])) for k in range(int(ent["bend_n"][j]))] for j in range(N)]
        su = eo.Setup(N, agent, D, int(ent["num_samples"]), p.T_span, fe.cable_length, [tuple(map(float, q)) for q in pb], reps, longest, sampled,
                      [int(x) for x in ent["present"]], bendpts)
        root_state = state_of(init if init is not None else ent.get("init"), N + S)
    cnt = dict(updates=0, iz_shared=0, invalid_end_pops=0, max_list=0, max_bend=0, n_entangled=0)

    goal_occupied = 0
    G = [[goal[0] + 0.5, goal[1] + 0.5], [goal[0] + 0.5, goal[1] - 0.5], [goal[0] - 0.5, goal[1] + 0.5], [goal[0] - 0.5, goal[1] - 0.5]]
    for j in range(N):
        if j == own or goal_occupied:
            continue
        nv = int(hull_nv[j][D - 1])
        if nv > 0 and oracle.gjk_collision(hull_xy[j][D - 1][:nv], G):
            goal_occupied = 1

    pool, heap, table, xy_iz = [], [], {}, {}
    st_ = dict(ran_trigger=0, capped=0, n_entangled=0, overflow=0)
    cap = min(int(max_nodes), MAX_NODES)

    def cost(n):
        return pool[n].g + bias * pool[n].h

    def comp(l, r):                                 # CompareCost(left, right) (kinodynamic_search.hpp:163-179)
        cl, cr = cost(l), cost(r)
        if abs(cl - cr) < 1e-5:
            return pool[l].h > pool[r].h
        return cl > cr

    def push_heap(hole, value):                     # std::__push_heap(first, hole, 0, value)
        parent = (hole - 1) // 2
        while hole > 0 and comp(heap[parent], value):
            heap[hole] = heap[parent]; hole = parent; parent = (hole - 1) // 2
        heap[hole] = value

    def pop():                                      # top(); pop(): std::pop_heap + pop_back
        top = heap[0]
        ln = len(heap) - 1
        value = heap[ln]
        heap[ln] = top
        hole = second = 0
        while second < (ln - 1) // 2:               # std::__adjust_heap(first, 0, len, value)
            second = 2 * (second + 1)
            if comp(heap[second], heap[second - 1]):
                second -= 1
            heap[hole] = heap[second]; hole = second
        if (ln & 1) == 0 and second == (ln - 2) // 2:
            second = 2 * (second + 1); heap[hole] = heap[second - 1]; hole = second - 1
        if ln > 0:
            push_heap(hole, value)
        heap.pop()
        return top

    def expand(cur):
        par = None if cur < 0 else pool[cur]
        pe = root if par is None else par.end
        pindex = 0 if par is None else par.index
        for q in range(ns * ns):
            if len(pool) >= cap - 1:                # "run out of memory" (:1061-1065), at the pool when that is smaller
                if cap < MAX_NODES:
                    st_["capped"] = 1
                return
            comb = int(order[q]) if order is not None else q
            ch = _child(p, fe, pb_own, pe, par is None, comb // ns, comb % ns, goal)
            if ch is None:
                continue
            e, cx, cy, dist, vx, vy = ch
            nb = _Node()
            nb.index = pindex + 1; nb.prev = cur; nb.end = e; nb.cx = cx; nb.cy = cy; nb.vx = vx; nb.vy = vy; nb.iz = 0; nb.ent = None
            if su is None:
                arc = math.sqrt((e[0] - pe[0]) * (e[0] - pe[0]) + (e[1] - pe[1]) * (e[1] - pe[1]))
                nb.h = dist                         # getH (:401-405)
            else:
                nb.ent = _copy(root_state if par is None else par.ent)
                rc, arc = _entangles(su, nb.ent, cx, cy, (e[0], e[1]), nb.index)
                if rc == 1:
                    st_["n_entangled"] += 1
                    continue
                if rc == 2:
                    st_["overflow"] = 1
                    continue
                nb.h = (dist + 0.3 * float(len(nb.ent.alphas))) + 1.0 * float(len(nb.ent.bend))     # (:1177-1182)
                nb.iz = _iz(nb.ent)
                cnt["max_list"] = max(cnt["max_list"], len(nb.ent.alphas)); cnt["max_bend"] = max(cnt["max_bend"], len(nb.ent.bend))
            nb.g = (0.0 if par is None else par.g) + arc
            key = (vx, vy, nb.iz)
            if par is not None:
                f = table.get(key, -1)
                if f >= 0:
                    o = pool[f]
                    if o.state == 1 and o.index == nb.index:
                        if nb.g + bias * nb.h < o.g + bias * o.h and st_["ran_trigger"] % 2 == 0:
                            # the open node updated in place (:1190-1203); its entangle state stays (:1204 is commented out)
                            o.prev = cur; o.g = nb.g; o.h = nb.h; o.end = e; o.cx = cx; o.cy = cy
                            cnt["updates"] += 1
                        st_["ran_trigger"] += 1
                    continue
            nb.state = 1
            pool.append(nb)
            heap.append(len(pool) - 1); push_heap(len(heap) - 1, len(pool) - 1)
            table.setdefault(key, len(pool) - 1)    # unordered_map::insert keeps the first
            if su is not None:
                seen = xy_iz.setdefault((vx, vy), set())
                if seen and nb.iz not in seen:
                    cnt["iz_shared"] += 1
                seen.add(nb.iz)

    def collides(nd):                               # collidesWithObstacles2dSolve (:1514-1553), then collidesWithBases2d (:1583-1628)
        Qx = oracle.pos_ctrl_pts(nd.cx, p.T_span); Qy = oracle.pos_ctrl_pts(nd.cy, p.T_span)
        Q = [[Qx[i], Qy[i]] for i in range(4)]
        idx = min(nd.index, D)
        for j in range(N):
            if j == own:
                continue
            nv = int(hull_nv[j][idx - 1])
            if nv > 0 and oracle.gjk_collision(hull_xy[j][idx - 1][:nv], Q):
                return True
        for s in statics:
            if len(s) > 0 and oracle.gjk_collision(s, Q):
                return True
        if su is not None:
            radius, safe = 0.7, (p.T_span * p.v_max) * 2
            for j in range(N):
                if j == own:
                    continue
                bx, by = float(pb[j][0]), float(pb[j][1])
                if math.sqrt((Q[0][0] - bx) * (Q[0][0] - bx) + (Q[0][1] - by) * (Q[0][1] - by)) > safe:
                    continue
                if oracle.gjk_collision([[bx + radius, by + radius], [bx + radius, by - radius], [bx - radius, by - radius], [bx - radius, by + radius]], Q):
                    return True
        return False

    expand(-1)
    status, cur, closest, pops = EMPTY, -1, -1, 0
    smallest = 1.7976931348623157e308
    while heap:
        if pops >= max_pops:
            status = BUDGET
            break
        cur = pop(); pops += 1
        nd = pool[cur]
        nd.state = -1
        dist = math.sqrt((nd.end[0] - goal[0]) * (nd.end[0] - goal[0]) + (nd.end[1] - goal[1]) * (nd.end[1] - goal[1]))
        dfi = math.sqrt((nd.end[0] - root[0]) * (nd.end[0] - root[0]) + (nd.end[1] - root[1]) * (nd.end[1] - root[1]))
        if collides(nd):
            continue
        valid = su is None or all(nd.ent.active[i] <= 1 for i in range(N))      # (:1693-1700)
        if not valid:
            cnt["invalid_end_pops"] += 1
        dti = (dist * dist if goal_occupied else dfi) * float(nd.index)
        if valid and dti < smallest:
            smallest = dti; closest = cur
        if valid and dist < fe.goal_size:
            status = GOAL
            break
        expand(cur)

    best = cur if status == GOAL else closest       # use_not_reaching_soln
    if best < 0:
        status = NO_SOLUTION
    g = np.zeros(1, dtype=abi.GUESS_DTYPE)[0]
    g["t_start"] = start["t_start"]
    case = np.zeros((abi.NEP_MAX_POL, N), dtype=np.int32)
    K = depth = 0
    cst = dtg = 0.0
    if best >= 0:
        b = pool[best]
        depth = b.index; K = min(depth, D); cst = cost(best)
        dtg = math.sqrt((b.end[0] - goal[0]) * (b.end[0] - goal[0]) + (b.end[1] - goal[1]) * (b.end[1] - goal[1]))
        path = {}
        k = best
        while k >= 0:                               # recoverPwpOut (:521-553): the path's nodes of index <= num_pol
            path[pool[k].index] = pool[k]
            k = pool[k].prev
        co = np.zeros((3, abi.NEP_MAX_POL, 4))
        for d in range(1, K + 1):
            co[0, d - 1] = path[d].cx; co[1, d - 1] = path[d].cy
        Kg = K
        if fe.pad_hold and K < D:                   # (as nep_batch_frontend: segments beyond the plan hold the returned node's end point)
            co[0, K:D, 3] = b.end[0]; co[1, K:D, 3] = b.end[1]
            Kg = D
        cz = _initial_z(float(start["pos"][2]), float(start["vel"][2]), float(start["accel"][2]), float(start["goal"][2]), p.T_span, D, p.v_max, p.a_max)
        for d in range(Kg):
            co[2, d] = cz[d]
        if su is not None:                          # state at the START of segment i (held segments: the returned node's)
            for i in range(Kg):
                dd = min(i, K)
                case[i] = _case_row(root_state if dd == 0 else path[dd].ent, N)
        K = Kg
        g["coeff"] = co
    g["K"] = K
    res = dict(status=status, K=K, depth=depth, n_children=pops, n_feasible=len(pool), n_collision_free=0, goal_occupied=goal_occupied,
               _pad=PAD_POOL if st_["capped"] else 0, cost=cst, dist_to_goal=dtg, n_entangled=st_["n_entangled"], ent_overflow=st_["overflow"])
    cnt["n_entangled"] = st_["n_entangled"]
    return g, res, case, cnt
