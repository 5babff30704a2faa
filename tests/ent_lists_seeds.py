"""Seeds for the tests of the list form of the tracked tether state (nep_ent_lists): lists of more than NEP_FE_ENT_CAP crossings at
small sizes come from a host pre-walk.  Every agent of a tether_crossing_scene(20, 8, seed) random-walks (normal steps, sigma 0.6 m,
clipped to the world) through nep_ent_track_step; the others' tethers are published from their states move by move.  Where the pre-walk ends and
where the scene's records start are different places: nothing in the tracking reads that.

A pre-walked state is KEPT as a seed when its walk never raised NEP_ENT_TRACK_CAP under cap = CAP (so it is the exact state), it has
at most 5 bend points, and its list is long (>= 48 entries) or short (<= 30); the other slots start empty."""
import ctypes as C
import functools

import numpy as np

from neptune_amd import abi, entangle, scene
from neptune_amd._lib import lib

CAP = 112
MOVES = 4000
SIGMA = 0.6
SCENE_SEEDS = (61, 62)
LONG, SHORT, MAX_BEND = 48, 30, 5


def reps_of(sc):
    return scene.static_reps(sc["statics"]) if len(sc["statics"]) else (np.zeros((0, 2, 2)), np.zeros((0, 2)))


@functools.lru_cache(maxsize=None)
def prewalk(n, m, seed, moves=MOVES, cap=CAP):
    """-> (states [N] entangle.State of capacity cap, flags [N]: the OR of every move's NEP_ENT_TRACK_* bits)"""
    sc = scene.tether_crossing_scene(n, m, seed)
    p = sc["par"]
    N = p.num_agents
    reps, longs = reps_of(sc)
    rng = np.random.default_rng(1000 + seed)
    chk = [entangle.EntangleCheck(N, a + 1, p.num_pol, 3, p.T_span, p.tether_length, p.pb, reps, longs) for a in range(N)]
    states = [entangle.State(N + len(reps), cap=cap) for _ in range(N)]
    pos = np.ascontiguousarray(np.asarray(sc["starts"], dtype=np.float64)[:, :2])
    new = pos.copy()
    present = np.ones(N, dtype=np.int32)
    pb = np.ascontiguousarray(p.pb, dtype=np.float64).reshape(N, 2)
    # every agent publishes the bend points of its state (base first); the lists of the previous move are the previous check's
    off, off_prev = np.arange(N + 1, dtype=np.int32), np.arange(N + 1, dtype=np.int32)
    xy, xy_prev = np.zeros((N * abi.NEP_MAX_BEND, 2)), np.zeros((N * abi.NEP_MAX_BEND, 2))
    xy[:N] = pb; xy_prev[:N] = pb
    tin = abi.nep_ent_track_inputs(abi.dptr(pos), abi.dptr(new), abi.iptr(present), abi.iptr(off), abi.dptr(xy), abi.iptr(off_prev), abi.dptr(xy_prev))
    lo, hi = np.array([p.x_min, p.y_min]), np.array([p.x_max, p.y_max])
    flags = np.zeros(N, dtype=np.int32)
    step = lib().nep_ent_track_step
    for _ in range(moves):
        new[...] = np.clip(pos + rng.normal(scale=SIGMA, size=(N, 2)), lo, hi)
        for a in range(N):
            rc = step(C.byref(chk[a].cfg), C.byref(tin), C.byref(states[a].c), abi.dptr(pos[a]), abi.dptr(new[a]))
            assert rc >= 0, rc
            flags[a] |= rc
        pos[...] = new
        off_prev[...] = off; xy_prev[...] = xy
        k = 0
        for a in range(N):
            st = states[a]
            off[a] = k
            xy[k] = pb[a]; k += 1
            for j in range(st.c.n_bend):
                i, c = st.alphas[st.bend_idx[j]]
                xy[k] = pb[i - 1] if i <= N else reps[i - N - 1][c]; k += 1
        off[N] = k
    return states, flags


def kept(states, flags):
    """per agent: 'long', 'short' or None (not a seed: the slot starts empty)"""
    out = []
    for st, fl in zip(states, flags):
        n, b = st.c.n_alpha, st.c.n_bend
        ok = not (fl & abi.NEP_ENT_TRACK_CAP) and b <= MAX_BEND
        out.append("long" if ok and n >= LONG else "short" if ok and n <= SHORT else None)
    return out


def copy_state(st, cap):
    out = entangle.State(st.c.n_active, cap=cap)
    n, b = st.c.n_alpha, st.c.n_bend
    assert n <= cap and b <= cap
    out.alphas[:n] = st.alphas[:n]; out.betas[:n] = st.betas[:n]; out.bend_idx[:b] = st.bend_idx[:b]; out.active[:] = st.active
    out.c.n_alpha, out.c.n_bend = n, b
    return out


def seeded_scenes(n=20, m=8, seeds=SCENE_SEEDS, cap=CAP, short_only=False):
    """-> (scenes, host states [S][N] of capacity cap: the kept seeds, the others empty; kinds [S][N])"""
    scenes, states, kinds = [], [], []
    for seed in seeds:
        sc = scene.tether_crossing_scene(n, m, seed)
        st, fl = prewalk(n, m, seed)
        kd = kept(st, fl)
        if short_only:
            kd = [k if k == "short" else None for k in kd]
        n_act = sc["par"].num_agents + len(reps_of(sc)[0])
        scenes.append(sc); kinds.append(kd)
        states.append([copy_state(s, cap) if k else entangle.State(n_act, cap=cap) for s, k in zip(st, kd)])
    return scenes, states, kinds


def to_lists(states, cap):
    """host states [S][N] -> abi.EntLists"""
    flat = [st for row in states for st in row]
    out = abi.EntLists(len(flat), cap)
    for i, st in enumerate(flat):
        out.set_state(i, st)
    return out


def assert_lists_equal(lists, slot, st, where):
    """slot `slot` of an abi.EntLists against a host state, byte for byte, zeros beyond the counts"""
    al, be_, bi, _ = st.as_lists()
    n, b = len(al), len(bi)
    assert int(lists.n_alpha[slot]) == n and int(lists.n_bend[slot]) == b, (where, int(lists.n_alpha[slot]), n, int(lists.n_bend[slot]), b)
    assert [(int(i), int(c)) for i, c in zip(lists.id[slot, :n], lists.cs[slot, :n])] == al, where
    assert np.array_equal(lists.beta[slot, :n].view(np.int64), np.array(be_, dtype=np.float64).view(np.int64)), where
    assert [int(x) for x in lists.bend[slot, :b]] == bi, where
    assert not lists.id[slot, n:].any() and not lists.cs[slot, n:].any() and not lists.beta[slot, n:].view(np.int64).any() and not lists.bend[slot, b:].any(), where
