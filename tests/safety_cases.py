"""Cases and references of the safety pass beyond one staging round (test_safety_cases_cpu.py, test_gpu_safety_sizes.py):
record sets of 5 .. 261 agents whose conflict matrices are neither empty nor symmetric, the header's resolution rule in plain
numpy, and degenerate inputs of gjk::collision on a 1/8 grid with an exact integer verdict.  No GPU here: everything is the
oracle's or numpy's.

perturbed() takes the round's clock t_start on top of (par, prev, seed): the three flags go to agents that have conflicts in both
directions ON THAT CLOCK, so `fresh` depends on it.  A seed with which the roles cannot be filled raises ValueError (the seeds
of CONFIGS are ones with which they can): a change of param_sets.make_scene shows up as that error, and the cure is another seed.
The oracle's N * N pairwise pass takes seconds at N = 261, and a configuration needs it several times over (three scenes, both
matrices, both accept vectors): its calls release the interpreter lock, so config() runs them in threads (_in_threads)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import param_sets as PS

TILE_N = 29                      # the scene that is tiled beyond 70 agents
CLOCKS = (0.0, 1.5, 3.0)         # scene k of a handle starts its round CLOCKS[k] intervals after its records do

# key -> (parameter set, N, stacked, seed): what each size reaches is in test_safety_cases_cpu.py's docstring
CONFIGS = {
    "default-5": ("default", 5, False, 14),
    "default-6": ("default", 6, False, 14),
    "default-13": ("default", 13, False, 14),
    "default-37": ("default", 37, False, 15),
    "pol5-26": ("pol5", 26, False, 15),
    "pol6-70": ("pol6", 70, False, 16),
    "default-261": ("default", 261, False, 17),
    "default-261-stacked": ("default", 261, True, 18),
}
MASKED = ("default-37", "pol6-70", "default-261-stacked")


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def fleet_records(name, N, seed, stacked=False):
    """-> (par, prev [N] records, statics = []).  Up to 70 agents the committed records of param_sets.make_scene(name, N, 0, seed);
    beyond that copies of a 29-agent scene (make_scene's rejection sampling is quadratic in N), copy k moved by (k % 3, k // 3) * 4
    world widths — or not moved at all (stacked): every copy then flies through its original, a dense conflict matrix."""
    par = PS.params(name, N, 0)
    if N <= 70:
        return par, PS.make_scene(name, N, 0, seed)["committed"].copy(), []
    base = PS.make_scene(name, TILE_N, 0, seed)
    width = base["par"].x_max - base["par"].x_min
    prev = np.concatenate([base["committed"]] * (-(-N // TILE_N)))[:N].copy()
    for a in range(N):
        k = a // TILE_N
        if not stacked:
            for ax, cell in enumerate((k % 3, k // 3)):
                prev[a]["pwp"]["coeff"][ax, :, 3] += cell * 4.0 * width
                prev[a]["pos"][ax] += cell * 4.0 * width
        prev[a]["id"] = a + 1
        prev[a]["bend"][0] = par.pb[a]
    return par, prev, []


def pair_hits(oracle, par, mine, other, t_start):
    """the oracle's pairwise test: `mine`'s trajectory against the interval hulls of `other` on the grid of t_start (the entry
    [0][1] of its matrix of the two records; `mine` enters as a non-agent, so the opposite entry costs nothing)"""
    two = np.zeros(2, dtype=mine.dtype)
    two[0] = mine; two[1] = other
    two[0]["is_agent"] = 0
    return bool(oracle.safety_resolve(two, t_start, par.T_span, par.drone_radius)[0][0, 1])


def row_and_column(oracle, par, recs, a, t_start):
    """row a and column a of the oracle's matrix of `recs`, by the pairwise test"""
    N = len(recs)
    row = np.zeros(N, dtype=np.uint8); col = np.zeros(N, dtype=np.uint8)
    for j in range(N):
        if j != a:
            row[j] = pair_hits(oracle, par, recs[a], recs[j], t_start)
            col[j] = pair_hits(oracle, par, recs[j], recs[a], t_start)
    return row, col


FLAGS = ("valid", "is_agent", "n_seg")


def set_flag(recs, a, flag):
    if flag == "n_seg":
        recs[a]["pwp"]["n_seg"] -= 2
    else:
        recs[a][flag] = 0


def perturbed_parts(par, prev, seed, t_start=0.0):
    """perturbed() with what it went through: (fresh, unflagged, {flag: agent})"""
    oracle = _oracle()
    rng = np.random.default_rng(seed)
    N = len(prev)
    unflagged = prev.copy()
    chosen = [int(a) for a in rng.choice(N, size=max(4, N // 3 + 2), replace=False)]
    stay = [j for j in range(N) if j not in chosen]
    short, probe = chosen[0], chosen[1]
    # one pair whose conflict depends on the round's clock: `timed` flies its segments 100 m apart from one another (the check takes
    # segment by segment: a jump between two of them is nothing to it) and `probe` flies next to it, segment by segment, but for the
    # last one.  On the records' own clock they meet in every interval; on a later clock the hull of interval i holds later segments
    # (the last one from the records' end on, which is why the probe's last segment is elsewhere) and they do not meet at all.
    timed = int(rng.choice(stay))
    for s_ in range(int(prev[timed]["pwp"]["n_seg"])):
        unflagged[timed]["pwp"]["coeff"][1, s_, 3] += 100.0 * s_
    for a in chosen:
        src = timed if a == probe else int(rng.choice(stay))       # (an agent that keeps its place: the neighbour is still there)
        r = rng.uniform(0.2, 0.6) if a in chosen[:4] else rng.uniform(0.2, 2.2)       # (the first four have roles: they must meet)
        th = rng.uniform(0.0, 2.0 * np.pi)
        unflagged[a]["pwp"] = unflagged[src]["pwp"]
        unflagged[a]["pwp"]["coeff"][0, :, 3] += r * np.cos(th)
        unflagged[a]["pwp"]["coeff"][1, :, 3] += r * np.sin(th)
    # the agent that will be two segments short meets its neighbour in its last two segments only, so that the shorter record
    # loses the conflict
    n = int(unflagged[short]["pwp"]["n_seg"])
    unflagged[short]["pwp"]["coeff"][0, :n - 2, 3] += 1000.0
    unflagged[probe]["pwp"]["coeff"][0, int(unflagged[probe]["pwp"]["n_seg"]) - 1, 3] += 1000.0
    unflagged["pos"] += 0.01                                       # new != previous in every record
    where = {}
    for a in [a for a in chosen if a != probe]:                    # (rows and columns by the pairwise test: the whole matrix is not needed)
        row, col = row_and_column(oracle, par, unflagged, a, t_start)
        if not (row.any() and col.any()):
            continue
        if a == short:
            trial = unflagged.copy(); set_flag(trial, a, "n_seg")
            row1, col1 = row_and_column(oracle, par, trial, a, t_start)
            if (row1 != row).any() or (col1 != col).any():
                where["n_seg"] = a
        elif "valid" not in where:
            where["valid"] = a
        elif "is_agent" not in where:
            where["is_agent"] = a
        if len(where) == 3 or "n_seg" not in where:                # (the short one is tried first: without it the seed is no use)
            break
    if len(where) < 3:
        raise ValueError("flags %s only: another seed" % sorted(where))
    fresh = unflagged.copy()
    for flag, a in where.items():
        set_flag(fresh, a, flag)
    return fresh, unflagged, where


def perturbed(par, prev, seed, t_start=0.0):
    """-> fresh: about a third of the agents fly the trajectory of an agent that keeps its own, moved by 0.2 .. 2.2 m (either end
    of the range: mutual and one-directional conflicts with the 1.2 m inflation), one pair meets on the records' own clock only,
    then one record is invalid, one is no agent and one is two segments short — each an agent with conflicts in both directions
    (at the round's clock t_start), so that every flag changes the answer"""
    return perturbed_parts(par, prev, seed, t_start)[0]


def resolve(C, Cp, mask, ent=None):
    """the header's rule: inactive agents accepted first; active ones in id order, turned down by a conflict (either direction) with
    any accepted agent, by check_prev (Cp[a, j] for any j) or by the entangle verdict"""
    N = len(mask)
    acc = (mask == 0).copy()
    for a in range(N):
        if mask[a] == 0:
            continue
        bad = bool(ent is not None and ent[a])
        if Cp is not None:
            bad |= bool(np.any(np.delete(Cp[a], a)))
        for j in range(N):
            if j != a and acc[j] and (C[a, j] or C[j, a]):
                bad = True
        acc[a] = not bad
    return acc.astype(np.int32)


def conflicts_prev(oracle, par, prev, fresh, t_start, rows=None):
    """Cp[a, j] = fresh[a] hits the hulls of prev[j] (a != j): what orc_safety_resolve_prev tests row by row, entry by entry
    (rows: only these, the others stay 0)"""
    N = len(fresh)
    Cp = np.zeros((N, N), dtype=np.uint8)
    # pair_hits without its per-call set-up (N * N calls: the interpreter's share is what the threads cannot overlap)
    fn = oracle.lib().orc_safety_resolve
    two = np.zeros(2, dtype=fresh.dtype); conf = np.zeros((2, 2), dtype=np.uint8); acc = np.zeros(2, dtype=np.int32)
    p_two, p_conf, p_acc = two.ctypes.data, conf.ctypes.data, acc.ctypes.data
    for a in (range(N) if rows is None else rows):
        two[0] = fresh[a]; two[0]["is_agent"] = 0
        for j in range(N):
            if a != j:
                two[1] = prev[j]
                fn(2, p_two, t_start, par.T_span, par.drone_radius, p_conf, p_acc)
                Cp[a, j] = conf[0, 1]
    return Cp


def _scene(args):
    key, k = args
    name, N, stacked, seed = CONFIGS[key]
    par, prev, _ = fleet_records(name, N, seed + 100 * k, stacked)
    t_start = CLOCKS[k] * par.T_span
    fresh, unflagged, where = perturbed_parts(par, prev, seed + 100 * k, t_start)
    return dict(par=par, prev=prev, fresh=fresh, unflagged=unflagged, where=where, t_start=t_start)


def _in_threads(jobs):
    """[(f, args)] -> results; the oracle's calls release the interpreter lock, so these run side by side"""
    with ThreadPoolExecutor(max_workers=min(12, len(jobs))) as ex:
        return [f.result() for f in [ex.submit(fn, *a) for fn, a in jobs]]


def matrices(oracle, par, prev, judged, t_start, accepts=True):
    """jobs for _in_threads and what to make of their results: the oracle's C and Cp of `judged` against `prev` (and its accept flags
    without and with the previous-record check) -> (jobs, finish(results) -> dict)"""
    N = len(judged)
    halves = [range(0, N // 2), range(N // 2, N)]
    jobs = [(conflicts_prev, (oracle, par, prev, judged, t_start, h)) for h in halves]
    jobs.append((oracle.safety_resolve, (judged, t_start, par.T_span, par.drone_radius)))
    if accepts:
        jobs.append((oracle.safety_resolve_prev, (prev, judged, t_start, par.T_span, par.drone_radius)))

    def finish(res):
        out = dict(Cp=res[0] | res[1], C=res[2][0], accept=res[2][1])
        if accepts:
            assert np.array_equal(res[3][0], out["C"])
            out["accept_prev"] = res[3][1]
        return out
    return jobs, finish


@functools.lru_cache(maxsize=None)
def config(key):
    """the three scenes of a configuration (seeds 100 apart, clocks CLOCKS) with the oracle's answers, worked out once per process
    -> list of dicts(par, prev, fresh, unflagged, where, t_start, C, accept, Cp, accept_prev)"""
    oracle = _oracle()
    scs = _in_threads([(_scene, ((key, k),)) for k in range(len(CLOCKS))])
    parts = [matrices(oracle, sc["par"], sc["prev"], sc["fresh"], sc["t_start"]) for sc in scs]
    res = _in_threads([j for jobs, _ in parts for j in jobs])
    for sc, (jobs, finish) in zip(scs, parts):
        sc.update(finish(res[:len(jobs)])); res = res[len(jobs):]
    return scs


def masks(N, seed=7):
    """all active, a random half, the first 40 agents inactive (accepted-first bits in the row words 0 and 1) -> [3][N] int32"""
    rng = np.random.default_rng(seed)
    half = (rng.random(N) < 0.5).astype(np.int32)
    head = np.ones(N, np.int32); head[:40] = 0
    return np.stack([np.ones(N, np.int32), half, head])


@functools.lru_cache(maxsize=None)
def masked_config(key):
    """config(key)'s scenes under masks(N)[k]: the records the header defines (the previous record where inactive) and the
    oracle's matrices of them -> list of dicts(mask, judged, C, Cp)"""
    oracle = _oracle()
    scs = config(key)
    ms = masks(len(scs[0]["prev"]))
    out, parts = [], []
    for sc, m in zip(scs, ms):
        judged = sc["prev"].copy(); judged[m == 1] = sc["fresh"][m == 1]
        out.append(dict(mask=m, judged=judged))
        if m.all():
            out[-1].update(C=sc["C"], Cp=sc["Cp"])
            parts.append(([], lambda res: {}))
        else:
            parts.append(matrices(oracle, sc["par"], sc["prev"], judged, sc["t_start"], accepts=False))
    res = _in_threads([j for jobs, _ in parts for j in jobs])
    for o, (jobs, finish) in zip(out, parts):
        o.update(finish(res[:len(jobs)])); res = res[len(jobs):]
        o.pop("accept", None)
    return out


# ---- gjk::collision on degenerate inputs ---------------------------------------------------------------------------------------
GRID = 8                 # coordinates are integers / GRID within +-8: sums, differences and products of the algorithm are exact in fp64
LIM = 8 * GRID
FAMILIES = ("random", "shared", "point_or_segment", "concentric", "boxes", "small_hull")


def _hull_int(pts):
    """convex hull (ccw, collinear points dropped) of integer points"""
    P = sorted(set(map(tuple, pts)))
    if len(P) <= 2:
        return np.array(P, dtype=np.int64)

    def chain(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h
    lo = chain(P); up = chain(P[::-1])
    return np.array(lo[:-1] + up[:-1], dtype=np.int64)


def exact_verdicts(A, B):
    """A [n][2], B [m][2] integers -> (the convex hulls intersect, their Minkowski difference holds the origin in its interior),
    by int64 cross and dot products of the differences a_i - b_j: the hulls intersect iff no open half-plane through the origin
    holds every difference, and the origin is interior iff no closed one does"""
    D = (A[:, None, :] - B[None, :, :]).reshape(-1, 2).astype(np.int64)
    nz = D[(D != 0).any(axis=1)]
    if len(nz) == 0:
        return True, False                       # one common point
    cr = nz[:, None, 0] * nz[None, :, 1] - nz[:, None, 1] * nz[None, :, 0]
    dt = nz[:, None, 0] * nz[None, :, 0] + nz[:, None, 1] * nz[None, :, 1]
    # a closed half-plane holds all: some difference has every other on one side of its line
    closed = bool(((cr >= 0).all(axis=1) | (cr <= 0).all(axis=1)).any())
    # an open one: in addition none at the origin and none opposite to that difference
    ok = ~((cr == 0) & (dt < 0)).any(axis=1)
    opened = len(nz) == len(D) and bool(((((cr >= 0).all(axis=1)) | ((cr <= 0).all(axis=1))) & ok).any())
    return (not opened), (not closed)


def _inside(P):
    return np.abs(P).max() <= LIM


def gjk_grid_cases(seed=0):
    """About 6 000 (polygon, four points) pairs on the 1/8 grid -> (polys, quads [n][4][2], verdict [n], decisive [n]):
    verdict = the sets intersect, decisive = the exact test gives the same answer for "the interiors overlap" (a touching pair
    otherwise: what gjk::collision returns there is the algorithm's business)."""
    return _gjk_cases(seed)[:4]


def gjk_grid_families(seed=0):
    """the family (index into FAMILIES) of every case of gjk_grid_cases(seed)"""
    return _gjk_cases(seed)[4]


@functools.lru_cache(maxsize=None)
def _gjk_cases(seed):
    rng = np.random.default_rng(seed)
    cases = []                                   # (family, A int [n][2], B int [4][2])

    def cloud(n, c, s):
        return np.clip(c + rng.integers(-s, s + 1, size=(n, 2)), -LIM, LIM)

    def quad_near(A):
        return cloud(4, A[rng.integers(len(A))] + rng.integers(-20, 21, size=2), int(rng.integers(1, 17)))

    for _ in range(2000):                        # a hull of 1 .. 16 vertices against a quad
        A = cloud(int(rng.integers(1, 17)), rng.integers(-40, 41, size=2), int(rng.integers(1, 25)))
        cases.append((0, A, quad_near(A)))
    while len(cases) < 3200:                     # a quad that shares a vertex or an edge with the hull, the rest of it mostly outside
        A = _hull_int(cloud(int(rng.integers(3, 17)), rng.integers(-30, 31, size=2), int(rng.integers(2, 25))))
        if len(A) < 3:
            continue
        i = int(rng.integers(len(A))); v, nxt, prv = A[i], A[(i + 1) % len(A)], A[i - 1]
        edge = rng.random() < 0.5
        e1, e0 = nxt - v, v - prv
        nrm = np.array([e1[1], -e1[0]]) if edge else np.array([e1[1] + e0[1], -e1[0] - e0[0]])      # outward (ccw hull)
        B = [v, nxt] if edge else [v]
        while len(B) < 4:
            x = cloud(1, v, int(rng.integers(1, 25)))[0]
            if (x - v) @ nrm < 0 and rng.random() < 0.7:
                x = 2 * v - x                    # mirrored to the outer side of the supporting line
            if _inside(x):
                B.append(x)
        B = np.array(B)[rng.permutation(4)]
        cases.append((1, A, B))
    for k in range(800):                         # a quad that is one point, or two points doubled
        A = _hull_int(cloud(int(rng.integers(1, 17)), rng.integers(-30, 31, size=2), int(rng.integers(1, 25))))
        pick = [A[rng.integers(len(A))], (A[0] + A[-1]) // 2, cloud(1, A[0], 12)[0], cloud(1, A.mean(axis=0).astype(np.int64), 3)[0]]
        p = pick[int(rng.integers(4))]
        q = p if k % 2 == 0 else pick[int(rng.integers(4))]
        B = np.array([[p, p, q, q], [p, q, p, q], [p, q, q, p]][int(rng.integers(3))])
        cases.append((2, A, B))
    sq = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]]); dm = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]])
    for _ in range(400):                         # concentric square and diamond: the centroids are equal, the start direction is (1, 0)
        c = rng.integers(-30, 31, size=2); a, b = int(rng.integers(0, 25)), int(rng.integers(0, 25))
        A, B = c + a * sq, c + b * dm
        if rng.random() < 0.5:
            A, B = B, A
        cases.append((3, np.roll(A, int(rng.integers(4)), axis=0), np.roll(B, int(rng.integers(4)), axis=0)))
    for k in range(600):                         # equal boxes side by side, one grid step apart, touching, one step into each other
        w, h = int(rng.integers(1, 17)), int(rng.integers(1, 17)); c = rng.integers(-24, 25, size=2)
        gap = (-1, 0, 1)[k % 3]
        A = c + np.array([[0, 0], [w, 0], [w, h], [0, h]])
        off = np.array([w + gap, int(rng.integers(-h, h + 1)) if k % 2 else 0])
        if (k // 6) % 2:
            A = A[:, ::-1]; off = off[::-1]                       # one above the other
        cases.append((4, np.roll(A, int(rng.integers(4)), axis=0), np.roll(A + off, int(rng.integers(4)), axis=0)))
    for k in range(1000):                        # hulls of one, two or three vertices
        A = cloud(1 + k % 3, rng.integers(-30, 31, size=2), int(rng.integers(1, 17)))
        B = cloud(4, A[0] + rng.integers(-6, 7, size=2), int(rng.integers(1, 13)))
        cases.append((5, A, B))
    assert all(_inside(A) and _inside(B) and len(B) == 4 for _, A, B in cases)
    ex = [exact_verdicts(A, B) for _, A, B in cases]
    polys = [A.astype(np.float64) / GRID for _, A, _ in cases]
    quads = np.array([B for _, _, B in cases], dtype=np.float64) / GRID
    verdict = np.array([e[0] for e in ex]); decisive = np.array([e[0] == e[1] for e in ex])
    return polys, quads, verdict, decisive, np.array([f for f, _, _ in cases])
