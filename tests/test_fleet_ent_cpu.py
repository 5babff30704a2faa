"""CPU: nep_ent_predict_a (include/neptune_entangle.h), Neptune::PredictAlphasBetas for one agent — the state forwarded to point A
in one move, into a copy.  On the random walks of tests/test_ent_track_cpu.py it equals nep_ent_track_step on a copy with the
previous bend lists equal to the current ones, leaves its input untouched, and equals that module's Python restatement with the
eight-argument form forced even where a bend count "changed".  ABI checks of the fleet's tether calls that need no GPU."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import entangle_oracle as eo

from neptune_amd import _lib, abi, entangle
from test_ent_track_cpu import _bends, _world, track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _snapshot(st):
    return (st.c.n_alpha, st.c.n_bend, st.c.cap, st.c.n_active, st.alphas.tobytes(), st.betas.tobytes(), st.bend_idx.tobytes(), st.active.tobytes())


def _walk(seed):
    """test_track_step_equals_the_restatement's walk: (chk, per step: pk, pk1, pos, nxt, present, bend, prev), world"""
    rng = np.random.default_rng(seed)
    N, S, me = int(rng.integers(3, 7)), int(rng.integers(0, 5)), 1
    pb, reps, longest = _world(rng, N, S)
    cable = float(rng.uniform(8, 30))
    chk = entangle.EntangleCheck(N, me, 1, 1, 1.0, cable, np.array(pb), np.array(reps).reshape(S, 2, 2) if S else (),
                                 np.array(longest).reshape(S, 2) if S else ())
    bend = [_bends(rng, pb, reps, j) for j in range(N)]
    pos = rng.uniform(-4, 4, size=(N, 2))
    present = (rng.uniform(size=N) > 0.15).astype(np.int32)
    steps = []
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
        steps.append((tuple(pos[me - 1]), tuple(nxt[me - 1]), pos, nxt, present, bend, prev))
        pos = nxt
    return chk, steps, dict(N=N, S=S, me=me, pb=pb, reps=reps, longest=longest, cable=cable)


@pytest.mark.parametrize("seed", range(12))
def test_predict_a_is_one_track_step_on_a_copy(seed):
    """at every step of the walk (the walk itself advances with the tracking update, bend counts changing and all): the prediction
    of that move == nep_ent_track_step on a copy with prev = cur == the restatement with prev = cur; the input is not touched"""
    chk, steps, w = _walk(seed)
    N, S, me = w["N"], w["S"], w["me"]
    st_c = chk.new_state()
    st_p = eo.EntState(N + S)
    cap = st_c.c.cap
    changed = 0
    for k, (pk, pk1, pos, nxt, present, bend, prev) in enumerate(steps):
        cur = [np.array(b) for b in bend]
        before = _snapshot(st_c)
        out, f_a = chk.predict_a(st_c, pk, pk1, pos, nxt, present, cur)
        assert _snapshot(st_c) == before, (seed, k)                       # *in untouched
        # nep_ent_track_step on a copy, previous lists = current lists
        cp = chk.new_state()
        cp.alphas[:] = st_c.alphas; cp.betas[:] = st_c.betas; cp.bend_idx[:] = st_c.bend_idx; cp.active[:] = st_c.active
        cp.c.n_alpha, cp.c.n_bend = st_c.c.n_alpha, st_c.c.n_bend
        f_t = chk.track_step(cp, pk, pk1, pos, nxt, present, cur, cur)
        assert f_a == f_t, (seed, k)
        assert out.as_lists() == cp.as_lists(), (seed, k)
        assert np.array_equal(out.betas[:out.c.n_alpha].view(np.int64), cp.betas[:cp.c.n_alpha].view(np.int64)), (seed, k)
        # the restatement with the eight-argument form forced: bend_prev = bend even where the walk's count changed
        ref = copy.deepcopy(st_p)
        f_p = track_ref(ref, pk, pk1, pos, nxt, present, bend, bend, w["pb"], me, w["reps"], w["longest"], N, w["cable"], cap)
        a, b_, bi, act = out.as_lists()
        assert f_a == f_p, (seed, k)
        assert a == [tuple(x) for x in ref.alphas] and bi == ref.bend and act == ref.active, (seed, k)
        assert np.array_equal(np.array(b_, dtype=np.float64), np.array(ref.betas, dtype=np.float64)), (seed, k)
        if f_a & abi.NEP_ENT_TRACK_CAP:
            assert out.as_lists() == st_c.as_lists(), (seed, k)            # *out equals *in
        changed += any(len(x) != len(y) for x, y in zip(bend, prev))
        # the walk goes on with the tracking update proper (nine-argument form where a count changed)
        chk.track_step(st_c, pk, pk1, pos, nxt, present, cur, [np.array(b) for b in prev])
        track_ref(st_p, pk, pk1, pos, nxt, present, bend, prev, w["pb"], me, w["reps"], w["longest"], N, w["cable"], cap)
        assert st_c.as_lists()[0] == [tuple(x) for x in st_p.alphas], (seed, k)
    assert changed > 0 or w["S"] == 0, seed      # (a world without statics has base-only tethers: no list can change)


def test_the_walks_cross_bases_tethers_and_bend_points():
    """the predictions above see every kind of crossing: over a base (case 0), beyond an agent (1), between bend points (>= 2)"""
    kinds = set()
    for seed in range(12):
        chk, steps, w = _walk(seed)
        st = chk.new_state()
        for pk, pk1, pos, nxt, present, bend, prev in steps:
            cur = [np.array(b) for b in bend]
            n0 = st.c.n_alpha
            out, _ = chk.predict_a(st, pk, pk1, pos, nxt, present, cur)
            if out.c.n_alpha > n0:
                kinds.update(min(c, 2) for i, c in out.as_lists()[0][n0:] if i <= w["N"])
            chk.track_step(st, pk, pk1, pos, nxt, present, cur, [np.array(b) for b in prev])
    assert kinds == {0, 1, 2}, kinds


def test_predict_a_capacity_leaves_out_equal_in():
    """a list capacity of one entry: the first move that needs a second one returns NEP_ENT_TRACK_CAP alone and *out == *in"""
    hit = 0
    for seed in range(12):
        chk, steps, w = _walk(seed)
        st = entangle.State(chk.n_active, cap=1)
        for pk, pk1, pos, nxt, present, bend, prev in steps:
            cur = [np.array(b) for b in bend]
            out, fl = chk.predict_a(st, pk, pk1, pos, nxt, present, cur)
            if fl & abi.NEP_ENT_TRACK_CAP:
                assert fl == abi.NEP_ENT_TRACK_CAP and out.as_lists() == st.as_lists(), seed
                hit += 1
            chk.track_step(st, pk, pk1, pos, nxt, present, cur, cur)
    assert hit > 0


def test_predict_a_arguments(L):
    chk = entangle.EntangleCheck(2, 1, 1, 1, 1.0, 10.0, np.zeros((2, 2)))
    st, out = chk.new_state(), chk.new_state()
    z = np.zeros(4); zi = np.zeros(3, dtype=np.int32); pr = np.ones(2, dtype=np.int32); p = np.zeros(2)
    args = lambda cfg=C.byref(chk.cfg), a=C.byref(st.c), o=C.byref(out.c), pk=abi.dptr(p): (cfg, abi.dptr(z), abi.dptr(z), abi.iptr(pr), abi.iptr(zi), None, a, pk, abi.dptr(p), o)      # noqa: E731
    assert L.nep_ent_predict_a(*args()) == 0
    assert L.nep_ent_predict_a(*args(cfg=None)) == -1
    assert L.nep_ent_predict_a(*args(a=None)) == -1
    assert L.nep_ent_predict_a(*args(o=None)) == -1
    assert L.nep_ent_predict_a(*args(o=C.byref(st.c))) == -1                # in place: that is nep_ent_track_step
    assert L.nep_ent_predict_a(*args(pk=None)) == -1


def test_fleet_ent_abi(L):
    assert "nep_ent_predict_a" in _lib.ENT_EXPORTS
    for name in ("nep_batch_fleet_init_ent", "nep_batch_fleet_predict_ent", "nep_batch_fleet_track_ent", "nep_batch_fleet_ent_state"):
        assert name in _lib.FLEET_EXPORTS and getattr(L, name)
    hdr = open(os.path.join(ROOT, "include", "neptune_fleet.h")).read()
    assert re.search(r"^int nep_batch_fleet_init_ent\(nep_batch_t\* h, double cable_length, const nep_fe_ent_state\* d_ent0, void\* stream\);", hdr, re.M)
    assert re.search(r"^int nep_batch_fleet_track_ent\(nep_batch_t\* h, const nep_traj_rec\* d_records, int32_t\* d_flags, void\* stream\);", hdr, re.M)
    assert re.search(r"^int nep_batch_fleet_select\(nep_batch_t\* h, nep_fe_start\* d_start, nep_traj_rec\* d_records, int32_t\* d_active,", hdr, re.M)
    # no new struct in the ABI
    assert [L.nep_abi_sizeof(k) for k in range(15)] == [1680, 1872, 56, 48, 152, 784, 896, 48, 24, 56, 120, 64, 104, 56, 456]
    assert L.nep_abi_sizeof(18) == 80 and L.nep_abi_sizeof(19) == -1
