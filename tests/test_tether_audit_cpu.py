"""CPU: the tether audit's host form (include/neptune_entangle.h: nep_ent_tether_length, nep_tether_audit,
nep_ent_track_step_audit) on the random walks of tests/test_ent_track_cpu.py — the length against oracle/entangle_oracle.py, the
audited step against the plain one, the record against the Python accumulator of tests/tether_audit_ref.py byte for byte, dropped
moves under a small capacity, and the ABI."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import entangle_oracle as eo

import tether_audit_ref as ref
from neptune_amd import _lib, abi, audit, entangle
from test_ent_track_cpu import _bends, _world, hsig9, track_ref

# test_ent_track_cpu's walks take seeds 0..11; of those only 0, 4, 5, 6 and 9 make a bend point (the others meet no static the right
# way).  Seeds 7, 8, 10, 11 are replaced by 12..15, which do: 9 of the 12 walks below add crossings and make a bend point
# (test_walks_cross_and_bend checks it); 1, 2, 3 stay as the walks without one.
SEEDS = (0, 1, 2, 3, 4, 5, 6, 9, 12, 13, 14, 15)
MOVES = 120
REC = abi.TETHER_AUDIT_DTYPE
T0, DT = 3.25, 0.0625      # (binary fractions: t0 + q * dt is exact, so a stretch that starts later gives the same times bit for bit)


@pytest.fixture(scope="module", autouse=True)
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _n_add(pk, pk1, pik, pik1, present, bend, bend_prev, pb, me, reps, N):
    """the step list's length before the merge, by the restatement: what track_ref collects before it looks at a capacity"""
    add = []
    for i in range(N):
        if i == me - 1 or not present[i] or len(bend[i]) == 0:
            continue
        hsig9(add, pk, pk1, tuple(pik[i]), tuple(pik1[i]), pb[me - 1], bend[i], bend_prev[i], i + 1)
    eo.hsig_to_add_static(add, pk, pk1, reps, N)
    return len(add)


def _walk(seed, cap=None, moves=MOVES):
    """test_track_step_equals_the_restatement's walk of `seed`, yielded move by move: (pk, pk1, pos, nxt, present, bend, prev) and
    the world it happens in"""
    rng = np.random.default_rng(seed)
    N, S, me = int(rng.integers(3, 7)), int(rng.integers(0, 5)), 1
    pb, reps, longest = _world(rng, N, S)
    cable = float(rng.uniform(8, 30))
    world = dict(N=N, S=S, me=me, pb=pb, reps=reps, longest=longest, cable=cable)
    bend = [_bends(rng, pb, reps, j) for j in range(N)]
    pos = rng.uniform(-4, 4, size=(N, 2))
    present = (rng.uniform(size=N) > 0.15).astype(np.int32)
    steps = []
    for _ in range(moves):
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
    return world, steps


def _check(world):
    N, S = world["N"], world["S"]
    return entangle.EntangleCheck(N, world["me"], 1, 1, 1.0, world["cable"], np.array(world["pb"]), np.array(world["reps"]).reshape(S, 2, 2) if S else (),
                                  np.array(world["longest"]).reshape(S, 2) if S else ())


def _state_bytes(st):
    return (st.c.n_alpha, st.c.n_bend, st.alphas.tobytes(), st.betas.tobytes(), st.bend_idx.tobytes(), st.active.tobytes())


@functools.lru_cache(maxsize=None)
def _flown(seed, cap=None):
    """the walk of `seed` through nep_ent_track_step_audit (state capacity `cap`, default the wrapper's) next to the plain step, the
    oracle restatement and the Python accumulator.  -> dict of what the tests compare"""
    world, steps = _walk(seed)
    N, S, me = world["N"], world["S"], world["me"]
    chk = _check(world)
    mk = (lambda: entangle.State(N + S, cap=cap)) if cap is not None else chk.new_state
    st_a, st_p = mk(), mk()
    st_o = eo.EntState(N + S)
    rec = audit.new_tether_audit(1)
    want = ref.fresh()
    t0, dt = T0, DT
    out = dict(world=world, len_err=0.0, too_long_ok=True, same_ret=True, same_state=True, drops=[], flags=[], lens=[], recs=[])
    for q, (pk, pk1, pos, nxt, present, bend, prev) in enumerate(steps, 1):
        b_now, b_prev = [np.array(b) for b in bend], [np.array(b) for b in prev]
        before = _state_bytes(st_a)
        counters0 = rec.copy()
        t = t0 + float(q) * dt
        f_a = chk.track_step(st_a, pk, pk1, pos, nxt, present, b_now, b_prev, audit=rec, t=t)
        f_p = chk.track_step(st_p, pk, pk1, pos, nxt, present, b_now, b_prev)
        out["same_ret"] &= f_a == f_p
        out["same_state"] &= _state_bytes(st_a) == _state_bytes(st_p)
        n_add = _n_add(pk, pk1, pos, nxt, present, bend, prev, world["pb"], me, world["reps"], N)
        f_o = track_ref(st_o, pk, pk1, pos, nxt, present, bend, prev, world["pb"], me, world["reps"], world["longest"], N, world["cable"], st_a.c.cap)
        assert f_o == f_a, (seed, q)
        length = chk.tether_length(st_a, pk1)
        want_len = eo.tether_length(st_o, world["pb"], world["pb"][me - 1], pk1, world["reps"], world["longest"], N)
        out["len_err"] = max(out["len_err"], abs(length - want_len))
        if not f_a & abi.NEP_ENT_TRACK_CAP:
            out["too_long_ok"] &= (length > world["cable"]) == bool(f_a & abi.NEP_ENT_TRACK_TOO_LONG)
        else:
            out["drops"].append(dict(kept=_state_bytes(st_a) == before, last_len=float(rec["last_len"][0]), length=length,
                                     still=all(rec[f][0] == counters0[f][0] for f in ("n_too_long", "n_entangled", "n_two_cases", "n_abort")),
                                     counted=int(rec["n_dropped"][0]) == int(counters0["n_dropped"][0]) + 1))
        a_, _, bi, act = st_a.as_lists()
        ref.tick(want, length, t, f_a, min(n_add, abi.NEP_ENT_TRACK_ADD_CAP), len(a_), len(bi), act, N)
        out["flags"].append(f_a); out["lens"].append(length); out["recs"].append(rec.copy())
    out["rec"], out["want"], out["steps"] = rec, want, steps
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_length_equals_the_oracle(seed):
    """after every move nep_ent_tether_length of the C state == the oracle's tether_length of the restated state within 1e-12 m (at most
    9 terms, each one rounded square root, lengths under 100 m: about 1e-13 of rounding, tenfold margin), and on every move that is
    not dropped (len > cable) is exactly the TOO_LONG bit"""
    r = _flown(seed)
    print("seed", seed, "largest |len - oracle|", r["len_err"], "longest", max(r["lens"]))
    assert max(r["lens"]) < 100.0
    assert r["len_err"] <= 1e-12
    assert r["too_long_ok"]


@pytest.mark.parametrize("seed", SEEDS)
def test_audited_step_equals_plain_step_and_the_accumulator(seed):
    r = _flown(seed)
    assert r["same_ret"] and r["same_state"]
    assert r["rec"].tobytes() == r["want"].tobytes(), (seed, r["rec"], r["want"])
    assert int(r["rec"]["n_ticks"][0]) == MOVES and float(r["rec"]["last_len"][0]) == r["lens"][-1]
    assert float(r["rec"]["max_len"][0]) == max(r["lens"])
    assert int(r["rec"]["tick_max_len"][0]) == 1 + int(np.argmax(r["lens"]))      # (ties go to the earlier tick: argmax's rule too)


def test_walks_cross_and_bend():
    """the walks exercise the audit: crossings added and a bend point made on at least 8 of the 12 seeds; somewhere a tether is
    too long, entangled and wound twice round one agent"""
    recs = [_flown(seed)["rec"][0] for seed in SEEDS]
    busy = sum(1 for r in recs if r["crossings_added"] > 0 and r["max_bend"] >= 1)
    print("crossings_added", [int(r["crossings_added"]) for r in recs], "max_bend", [int(r["max_bend"]) for r in recs],
          "max_wind", [int(r["max_wind"]) for r in recs], "n_too_long", [int(r["n_too_long"]) for r in recs])
    assert busy >= 8, busy
    assert any(r["n_too_long"] > 0 for r in recs) and any(r["n_entangled"] > 0 and r["entangled_partner"] >= 1 for r in recs)
    assert any(r["max_wind"] >= 2 and r["wind_partner"] >= 1 for r in recs)


@pytest.mark.parametrize("seed", SEEDS[:4])
def test_two_stretches_equal_one(seed):
    """two chained stretches into one record (each with its own t0, the ticks' times continuing) == one long stretch"""
    r = _flown(seed)
    world, steps = r["world"], r["steps"]
    chk = _check(world)
    st = chk.new_state()
    rec = audit.new_tether_audit(1)
    cut = 47
    moves = [(pk, pk1, pos, nxt, present, [np.array(b) for b in bend], [np.array(b) for b in prev]) for pk, pk1, pos, nxt, present, bend, prev in steps]
    _, f1 = audit.tether_audit_records(chk, st, moves[:cut], T0, DT, rec)
    assert rec.tobytes() == r["recs"][cut - 1].tobytes() and f1 == r["flags"][:cut]
    _, f2 = audit.tether_audit_records(chk, st, moves[cut:], T0 + cut * DT, DT, rec)      # (tick q of it is the flight's tick cut + q)
    assert rec.tobytes() == r["rec"].tobytes() and f2 == r["flags"][cut:]


def test_dropped_ticks_under_a_small_capacity():
    """state->cap = 4 on walks that outgrow it: the dropped moves are counted, keep the state, report the kept state's length and
    advance no other flag counter"""
    dropped = 0
    for seed in SEEDS:
        r = _flown(seed, 4)
        assert r["same_ret"] and r["same_state"]
        assert r["rec"].tobytes() == r["want"].tobytes(), seed
        assert int(r["rec"]["n_dropped"][0]) == len(r["drops"]) == sum(1 for f in r["flags"] if f & abi.NEP_ENT_TRACK_CAP)
        assert int(r["rec"]["max_alpha"][0]) <= 4
        for d in r["drops"]:
            assert d["kept"] and d["still"] and d["counted"] and d["last_len"] == d["length"], (seed, d)
        dropped += len(r["drops"])
    print("dropped moves over the 12 walks at cap 4:", dropped)
    assert dropped > 0


def test_abi(L):
    assert L.nep_abi_sizeof(37) == C.sizeof(abi.nep_tether_audit) == REC.itemsize == 120
    assert L.nep_abi_sizeof(38) == -1
    for name in ("nep_ent_tether_length", "nep_tether_audit_init", "nep_ent_track_step_audit"):
        assert name in _lib.ENT_EXPORTS and getattr(L, name)
    assert "nep_batch_set_tether_audit" in _lib.FE_EXPORTS and L.nep_batch_set_tether_audit
    fresh = audit.new_tether_audit(3)
    assert fresh.tobytes() == ref.fresh(3).tobytes()
    assert (fresh["max_len"] == -np.inf).all()
    for f in REC.names:
        if f != "max_len":
            assert (fresh[f] == 0).all(), f
    assert L.nep_tether_audit_init(None, 1) == -1 and L.nep_tether_audit_init(fresh.ctypes.data_as(C.c_void_p), -1) == -1
    assert L.nep_tether_audit_init(fresh.ctypes.data_as(C.c_void_p), 0) == 0
    # NULL arguments: NEP_E_ARG
    chk = entangle.EntangleCheck(2, 1, 1, 1, 1.0, 10.0, np.zeros((2, 2)))
    st = chk.new_state()
    z = np.zeros(2); zi = np.zeros(3, dtype=np.int32); pr = np.ones(2, dtype=np.int32); p = np.zeros(2)
    ok = abi.nep_ent_track_inputs(abi.dptr(z), abi.dptr(z), abi.iptr(pr), abi.iptr(zi), None, abi.iptr(zi), None)
    rec = audit.new_tether_audit(1); vp = rec.ctypes.data_as(C.c_void_p)
    assert L.nep_ent_track_step_audit(C.byref(chk.cfg), C.byref(ok), C.byref(st.c), abi.dptr(p), abi.dptr(p), 0.5, vp) == 0
    assert rec["n_ticks"][0] == 1 and rec["max_len"][0] == 0.0 and rec["t_max_len"][0] == 0.5
    seen = rec.copy()
    assert L.nep_ent_track_step_audit(None, C.byref(ok), C.byref(st.c), abi.dptr(p), abi.dptr(p), 0.5, vp) == -1
    assert L.nep_ent_track_step_audit(C.byref(chk.cfg), None, C.byref(st.c), abi.dptr(p), abi.dptr(p), 0.5, vp) == -1
    assert L.nep_ent_track_step_audit(C.byref(chk.cfg), C.byref(ok), None, abi.dptr(p), abi.dptr(p), 0.5, vp) == -1
    assert L.nep_ent_track_step_audit(C.byref(chk.cfg), C.byref(ok), C.byref(st.c), None, abi.dptr(p), 0.5, vp) == -1
    assert L.nep_ent_track_step_audit(C.byref(chk.cfg), C.byref(ok), C.byref(st.c), abi.dptr(p), abi.dptr(p), 0.5, None) == -1
    assert rec.tobytes() == seen.tobytes()      # (a refused call audits nothing)
    out = C.c_double(-1.0)
    p1 = np.array([3.0, 4.0])
    assert L.nep_ent_tether_length(C.byref(chk.cfg), C.byref(st.c), abi.dptr(p1), C.byref(out)) == 0 and out.value == 5.0
    assert L.nep_ent_tether_length(None, C.byref(st.c), abi.dptr(p1), C.byref(out)) == -1
    assert L.nep_ent_tether_length(C.byref(chk.cfg), None, abi.dptr(p1), C.byref(out)) == -1
    assert L.nep_ent_tether_length(C.byref(chk.cfg), C.byref(st.c), None, C.byref(out)) == -1
    assert L.nep_ent_tether_length(C.byref(chk.cfg), C.byref(st.c), abi.dptr(p1), None) == -1
    assert L.nep_batch_set_tether_audit(None, None, 0.0) == -1


def test_loops_refuse_the_audit_without_tethers():
    from neptune_amd.loop import DeviceFleetLoop, check_tether_audit
    with pytest.raises(ValueError):
        check_tether_audit(True, False)
    assert check_tether_audit(True, True) is True and check_tether_audit(False, False) is False
    assert "tether_audit" in DeviceFleetLoop._MUST_MATCH


def test_summary():
    """summarize_tethers on the walks' records taken as one scene: the least slack is the longest tether's, with its agent and time"""
    recs = np.concatenate([_flown(seed)["rec"] for seed in SEEDS[:6]] + [audit.new_tether_audit(1)])      # (the last agent never flew)
    s = audit.summarize_tethers(recs, 20.0, 1)[0]
    i = int(np.argmax(recs["max_len"]))
    assert s["min_slack"] == dict(value=float(20.0 - recs["max_len"][i]), agent=i + 1, t=float(recs["t_max_len"][i]), tick=int(recs["tick_max_len"][i]))
    assert s["max_alpha"] == int(recs["max_alpha"].max()) and s["max_bend"] == int(recs["max_bend"].max())
    w = int(np.argmax(recs["max_wind"]))
    assert s["max_wind"]["value"] == int(recs["max_wind"][w]) and s["max_wind"]["agent"] == w + 1 and s["max_wind"]["partner"] == int(recs["wind_partner"][w])
    assert s["n_too_long"] == int(recs["n_too_long"].sum()) and s["n_dropped"] == 0 and s["n_ticks"] == MOVES
    assert abs(s["mean_len"] - recs["sum_len"][:6].sum() / (6 * MOVES)) < 1e-12
    two = audit.summarize_tethers(np.concatenate([recs[:3], recs[3:6]]), 20.0, 2)
    assert len(two) == 2 and two[1]["min_slack"]["agent"] == 1 + int(np.argmax(recs["max_len"][3:6]))
    assert audit.summarize_tethers(audit.new_tether_audit(2), 20.0, 1)[0]["min_slack"] is None
    assert len(audit.format_tether_summary(two, cap=28)) == 5 and "cap 28" in audit.format_tether_summary(two, cap=28)[3]


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/tether_audit_host_check.cpp: walks, dropped moves and the edges as a stand-alone executable built from
    entangle_host.cpp alone under the address and undefined-behaviour sanitizers"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "tether_audit_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "tether_audit_host_check.cpp"),
                           os.path.join(root, "neptune_amd", "csrc", "entangle_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tether_audit_host_check ok" in out.stdout
