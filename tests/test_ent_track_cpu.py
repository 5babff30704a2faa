"""CPU: one tracking update of a tether's entangle state (nep_ent_track_step, include/neptune_entangle.h) against an independent
Python restatement of NeptuneRos::updateEntStateStaticObs (reference neptune_ros.cpp:800-850) — with the nine-argument
eu::entangleHSigToAddAgentInd (entangle_utils.cpp:820-1127) restated below and the other pieces from oracle/entangle_oracle.py —
and, where nothing changes bend count and nothing stops the search, against nep_ent_propagate_segment.  ABI checks of
nep_batch_track_ent that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import entangle_oracle as eo

from neptune_amd import _lib, abi, entangle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


# ---- the nine-argument form, line by line (entangle_utils.cpp:820-1127); True where the reference exits the process ----
def hsig9(add, pk, pk1, pik, pik1, pb, bend, bend_prev, agent_id):
    n, q = len(bend), len(bend_prev)
    if n == q:
        eo.hsig_to_add_agent(add, pk, pk1, pik, pik1, pb, bend, agent_id)
        return False
    base_addition = abort = False
    if n == 0 or q == 0:
        return False
    if n < q:
        for i in range(n):
            last = i == n - 1
            c1p = None
            if not last:
                c1, u, v = eo.wedge2(pk, bend[i + 1], bend[i])
                c2 = eo.wedge(pk1, bend[i + 1], bend[i])
            else:
                c1, u, v = eo.wedge2(pk, pik, bend_prev[-1])
                c2 = eo.wedge(pk1, pik1, bend[i])
                c1p, up, vp = eo.wedge2(pk, bend_prev[-1], bend_prev[-2])
            if last:
                f1 = eo.wedge(pb, pik, bend_prev[-1])
                f2, ub, vb = eo.wedge2(pb, pik1, bend[i])
                if f1 * f2 < 0:
                    a = eo._ratio(ub, vb)
                    if a < 0:
                        pass
                    elif a < 1:
                        add.append((agent_id, 1))
                    base_addition = True
                if i == 0 and eo.wedge(pb, bend_prev[-1], bend_prev[-2]) * f2 < 0:
                    a = eo._ratio(ub, vb)
                    if not (a < 0) and not (a < 1):
                        add.append((agent_id, 0)); abort = True
                    base_addition = True
            added = False
            if c1 * c2 < 0:
                a = eo._ratio(u, v)
                if a < 0:
                    add.append((agent_id, i + 2)); added = True
                elif a < 1 and last:
                    add.append((agent_id, 1))
            if last and c1p * c2 < 0:
                a = eo._ratio(up, vp)
                if a < 0 and not added:
                    add.append((agent_id, i + 2))
                elif a < 1:
                    pass
                elif i == 0:
                    add.append((agent_id, 0)); abort = True
    else:
        for i in range(n):
            last = i == n - 1
            if last:
                c1 = eo.wedge(pk, pik, bend_prev[-1]); c2, u, v = eo.wedge2(pk1, pik1, bend[i])
            elif i == n - 2:
                c1 = eo.wedge(pk, pik, bend_prev[-1]); c2, u, v = eo.wedge2(pk1, bend[i + 1], bend[i])
            else:
                c1, u, v = eo.wedge2(pk, bend[i + 1], bend[i]); c2 = eo.wedge(pk1, bend[i + 1], bend[i])
            if last:
                f1 = eo.wedge(pb, pik, bend_prev[-1]); f2, ub, vb = eo.wedge2(pb, pik1, bend[i])
                if f1 * f2 < 0:
                    a = eo._ratio(ub, vb)
                    if a < 0:
                        pass
                    elif a < 1:
                        add.append((agent_id, 1))
                    base_addition = True
            if i == 0 and n == 2:
                f1 = eo.wedge(pb, pik, bend_prev[-1]); f2, ub, vb = eo.wedge2(pb, bend[i + 1], bend[i])
                if f1 * f2 < 0:
                    a = eo._ratio(ub, vb)
                    if not (a < 0) and not (a < 1):
                        add.append((agent_id, 0)); abort = True
                    base_addition = True
            if c1 * c2 < 0:
                a = eo._ratio(u, v)
                if a < 0:
                    add.append((agent_id, i + 2))
                elif a < 1 and last:
                    add.append((agent_id, 1))
                elif a >= 1 and i == 0:
                    add.append((agent_id, 0)); abort = True
    if base_addition and len(add) >= 2 and add[-1] == add[-2]:
        del add[-2:]
    return abort


def track_ref(st, pk, pk1, pik, pik1, present, bend, bend_prev, pb, me, reps, longest, N, cable, cap):
    """updateEntStateStaticObs without its rate limit, with the library's capacities (state kept, flag 8)"""
    import copy
    add, abort = [], False
    for i in range(N):
        if i == me - 1 or not present[i] or len(bend[i]) == 0:
            continue
        abort |= hsig9(add, pk, pk1, tuple(pik[i]), tuple(pik1[i]), pb[me - 1], bend[i], bend_prev[i], i + 1)
    eo.hsig_to_add_static(add, pk, pk1, reps, N)
    if len(add) > abi.NEP_ENT_TRACK_ADD_CAP:
        return abi.NEP_ENT_TRACK_CAP
    before = copy.deepcopy(st)
    eo.add_alpha_beta_to_list(add, st, pk, pb, pb[me - 1], reps, N, bend)
    eo.update_bend_pts(st, pk1, pb, pb[me - 1], reps, N)
    if len(st.alphas) > cap or len(st.bend) > 7:
        st.__dict__.update(before.__dict__)
        return abi.NEP_ENT_TRACK_CAP
    fl = abi.NEP_ENT_TRACK_ABORT if abort else 0
    if any(st.active[i] > 2 for i in range(N)):
        fl |= abi.NEP_ENT_TRACK_ENTANGLED
    if any(st.active[i] >= 2 for i in range(N)):
        fl |= abi.NEP_ENT_TRACK_TWO_CASES
    if eo.tether_length(st, pb, pb[me - 1], pk1, reps, longest, N) > cable:
        fl |= abi.NEP_ENT_TRACK_TOO_LONG
    return fl


def _world(rng, N, S):
    pb = [tuple(p) for p in rng.uniform(-4, 4, size=(N, 2))]
    reps = [[tuple(rng.uniform(-4, 4, 2)), tuple(rng.uniform(-4, 4, 2))] for _ in range(S)]
    longest = [[float(x) for x in rng.uniform(0.1, 1.0, 2)] for _ in range(S)]
    return pb, reps, longest


def _bends(rng, pb, reps, j):
    k = int(rng.integers(0, 4))
    pts = [pb[j]] + [reps[int(rng.integers(len(reps)))][int(rng.integers(2))] for _ in range(k)] if reps else [pb[j]]
    return pts


@pytest.mark.parametrize("seed", range(12))
def test_track_step_equals_the_restatement(seed):
    rng = np.random.default_rng(seed)
    N, S, me = int(rng.integers(3, 7)), int(rng.integers(0, 5)), 1
    pb, reps, longest = _world(rng, N, S)
    cable = float(rng.uniform(8, 30))
    chk = entangle.EntangleCheck(N, me, 1, 1, 1.0, cable, np.array(pb), np.array(reps).reshape(S, 2, 2) if S else (),
                                 np.array(longest).reshape(S, 2) if S else ())
    st_c = chk.new_state()
    st_p = eo.EntState(N + S)
    cap = st_c.c.cap
    bend = [_bends(rng, pb, reps, j) for j in range(N)]
    pos = rng.uniform(-4, 4, size=(N, 2))
    present = (rng.uniform(size=N) > 0.15).astype(np.int32)
    seen = set()
    for step in range(120):
        prev = bend
        if rng.uniform() < 0.25:                        # somebody's trajectory message brings a new bend-point list
            bend = list(bend)
            j = int(rng.integers(N))
            if len(bend[j]) > 1 and rng.uniform() < 0.5:
                bend[j] = bend[j][:-1]
            elif S:
                bend[j] = bend[j] + [reps[int(rng.integers(S))][int(rng.integers(2))]]
        nxt = pos + rng.normal(scale=1.2, size=(N, 2))
        pk, pk1 = tuple(pos[me - 1]), tuple(nxt[me - 1])
        f_c = chk.track_step(st_c, pk, pk1, pos, nxt, present, [np.array(b) for b in bend], [np.array(b) for b in prev])
        f_p = track_ref(st_p, pk, pk1, pos, nxt, present, bend, prev, pb, me, reps, longest, N, cable, cap)
        a, b_, bi, act = st_c.as_lists()
        assert f_c == f_p, (seed, step)
        assert a == [tuple(x) for x in st_p.alphas] and bi == st_p.bend and act == st_p.active, (seed, step)
        assert np.array_equal(np.array(b_, dtype=np.float64), np.array(st_p.betas, dtype=np.float64)), (seed, step)
        seen.update(c for _, c in st_p.alphas)
        seen.add(("bends", len(st_p.bend)))
        pos = nxt
    assert seen, seed


def test_track_step_covers_release_creation_and_base_cases():
    """the random walks above visit every kind of crossing: over a base (case 0), beyond an agent (1), between bend points (>= 2),
    tethers that gained and lost bend points, and own bend points made and released"""
    kinds, bends_made, cancelled = set(), 0, 0
    for seed in range(12):
        rng = np.random.default_rng(seed)
        N, S, me = int(rng.integers(3, 7)), int(rng.integers(0, 5)), 1
        pb, reps, longest = _world(rng, N, S)
        cable = float(rng.uniform(8, 30))
        st = eo.EntState(N + S)
        bend = [_bends(rng, pb, reps, j) for j in range(N)]
        pos = rng.uniform(-4, 4, size=(N, 2))
        present = (rng.uniform(size=N) > 0.15).astype(np.int32)
        for _ in range(120):
            prev = bend
            if rng.uniform() < 0.25:
                bend = list(bend)
                j = int(rng.integers(N))
                if len(bend[j]) > 1 and rng.uniform() < 0.5:
                    bend[j] = bend[j][:-1]
                elif S:
                    bend[j] = bend[j] + [reps[int(rng.integers(S))][int(rng.integers(2))]]
            nxt = pos + rng.normal(scale=1.2, size=(N, 2))
            n0, b0 = len(st.alphas), len(st.bend)
            track_ref(st, tuple(pos[me - 1]), tuple(nxt[me - 1]), pos, nxt, present, bend, prev, pb, me, reps, longest, N, cable, 10 ** 6)
            kinds.update(min(c, 2) for _, c in st.alphas)
            bends_made += len(st.bend) > b0
            cancelled += len(st.alphas) < n0
            pos = nxt
    assert kinds == {0, 1, 2} and bends_made > 0 and cancelled > 0


@pytest.mark.parametrize("seed", range(8))
def test_chained_steps_equal_propagate_segment(seed):
    """one interval's samples chained through nep_ent_track_step == nep_ent_propagate_segment, where no bend count changes and the
    search's function does not return true"""
    rng = np.random.default_rng(100 + seed)
    N, S, ns, num_pol, T = 5, 3, 3, 4, 0.5
    pb, reps, longest = _world(rng, N, S)
    reps_a, long_a = np.array(reps).reshape(S, 2, 2), np.array(longest).reshape(S, 2)
    bend = [np.array(_bends(rng, pb, reps, j)) for j in range(N)]
    compared = 0
    for me in range(1, N + 1):
        chk = entangle.EntangleCheck(N, me, num_pol, ns, T, 1e9, np.array(pb), reps_a, long_a)
        sampled = rng.uniform(-4, 4, size=(N, 1, 1, 2)) + rng.normal(scale=0.4, size=(N, num_pol, ns + 1, 2))
        present = np.ones(N, dtype=np.int32)
        chk.set_inputs(sampled, present, bend)
        st_s, st_t = chk.new_state(), chk.new_state()
        p0 = rng.uniform(-4, 4, 2)
        for index in range(1, num_pol + 1):
            cx = [float(rng.normal()), float(rng.normal()), float(rng.normal(scale=2)), float(p0[0])]
            cy = [float(rng.normal()), float(rng.normal()), float(rng.normal(scale=2)), float(p0[1])]
            end = p0 + rng.normal(scale=1.0, size=2)
            hit, _ = chk.propagate_segment(st_s, cx, cy, end, index)
            if hit:
                break
            pk = (cx[3], cy[3])
            for j in range(1, ns + 1):
                if j < ns:
                    t = T * j / ns
                    t3, t2 = t * t * t, t * t
                    pk1 = (((cx[0] * t3 + cx[1] * t2) + cx[2] * t) + cx[3] * 1.0, ((cy[0] * t3 + cy[1] * t2) + cy[2] * t) + cy[3] * 1.0)
                else:
                    pk1 = (float(end[0]), float(end[1]))
                chk.track_step(st_t, pk, pk1, sampled[:, index - 1, j - 1], sampled[:, index - 1, j], present, bend, bend)
                pk = pk1
            assert st_t.as_lists() == st_s.as_lists(), (seed, me, index)
            compared += 1 + len(st_s.as_lists()[0])
            p0 = end
    assert compared > 0


def test_track_step_arguments(L):
    chk = entangle.EntangleCheck(2, 1, 1, 1, 1.0, 10.0, np.zeros((2, 2)))
    st = chk.new_state()
    z = np.zeros(2); zi = np.zeros(3, dtype=np.int32); pr = np.ones(2, dtype=np.int32)
    ok = abi.nep_ent_track_inputs(abi.dptr(z), abi.dptr(z), abi.iptr(pr), abi.iptr(zi), None, abi.iptr(zi), None)
    p = np.zeros(2)
    assert L.nep_ent_track_step(C.byref(chk.cfg), C.byref(ok), C.byref(st.c), abi.dptr(p), abi.dptr(p)) == 0
    assert L.nep_ent_track_step(None, C.byref(ok), C.byref(st.c), abi.dptr(p), abi.dptr(p)) == -1
    assert L.nep_ent_track_step(C.byref(chk.cfg), None, C.byref(st.c), abi.dptr(p), abi.dptr(p)) == -1
    assert L.nep_ent_track_step(C.byref(chk.cfg), C.byref(ok), C.byref(st.c), None, abi.dptr(p)) == -1
    bad = abi.nep_ent_track_inputs(abi.dptr(z), abi.dptr(z), abi.iptr(pr), abi.iptr(zi), None, None, None)
    assert L.nep_ent_track_step(C.byref(chk.cfg), C.byref(bad), C.byref(st.c), abi.dptr(p), abi.dptr(p)) == -1
    short = abi.nep_ent_state(0, 0, 4, 1, abi.iptr(np.zeros(8, dtype=np.int32)), abi.dptr(np.zeros(4)), abi.iptr(np.zeros(4, dtype=np.int32)),
                              abi.iptr(np.zeros(1, dtype=np.int32)))
    assert L.nep_ent_track_step(C.byref(chk.cfg), C.byref(ok), C.byref(short), abi.dptr(p), abi.dptr(p)) == -1      # n_active < N + S


def test_batch_track_ent_abi(L):
    assert "nep_batch_track_ent" in _lib.FE_EXPORTS and "nep_ent_track_step" in _lib.ENT_EXPORTS
    hdr = open(os.path.join(ROOT, "include", "neptune_frontend.h")).read()
    assert re.search(r"^int nep_batch_track_ent\(nep_batch_t\* h, const nep_traj_rec\* d_prev, nep_traj_rec\* d_records, const nep_guess\* d_guess,",
                     hdr, re.M)
    assert len(L.nep_batch_track_ent.argtypes) == 10
    assert L.nep_batch_track_ent(None, None, None, None, 1, 3, 1.0, None, None, None) == -1      # NEP_E_ARG
    # struct sizes: the new input record, and no existing record changed
    assert L.nep_abi_sizeof(15) == C.sizeof(abi.nep_ent_track_inputs) == 56
    assert [L.nep_abi_sizeof(k) for k in range(15)] == [1680, 1872, 56, 48, 152, 784, 896, 48, 24, 56, 120, 64, 104, 56, 456]
    assert L.nep_abi_sizeof(16) == -1
    ent_h = open(os.path.join(ROOT, "include", "neptune_entangle.h")).read()
    for name, v in (("NEP_ENT_TRACK_ENTANGLED", 1), ("NEP_ENT_TRACK_TWO_CASES", 2), ("NEP_ENT_TRACK_TOO_LONG", 4), ("NEP_ENT_TRACK_CAP", 8),
                    ("NEP_ENT_TRACK_ABORT", 16), ("NEP_ENT_TRACK_ADD_CAP", 32)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, v), ent_h, re.M) and getattr(abi, name) == v
