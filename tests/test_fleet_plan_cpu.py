"""CPU: the device form of the committed plan (include/neptune_fleet.h) as far as it can be checked without a GPU — the ABI, the
loud failure without a device, and that moving nep_plan_select_a / nep_plan_splice / nep_pwp_compose_exact onto the arithmetic
shared with the kernels (neptune_amd/csrc/plan_common.h) changed no bit of what they return: a seeded random sequence of resets,
splices, pops, selections and compositions against a restatement in Python floats (IEEE doubles, one rounding per operation,
the order of plan_common.h's expressions), compared exactly."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from neptune_amd import _lib, abi, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_fleet_abi(L):
    assert L.nep_abi_sizeof(18) == C.sizeof(abi.nep_fleet_cfg) == 80
    assert [L.nep_abi_sizeof(k) for k in range(16)] == [1680, 1872, 56, 48, 152, 784, 896, 48, 24, 56, 120, 64, 104, 56, 456, 56]
    assert L.nep_abi_sizeof(16) == -1 and L.nep_abi_sizeof(17) == 112 and L.nep_abi_sizeof(19) == -1
    # nep_fleet_cfg starts with nep_plan_cfg's six doubles and deltaT0
    for (a, _), (b, _) in zip(abi.nep_fleet_cfg._fields_[:7], abi.nep_plan_cfg._fields_[:7]):
        assert a == b and getattr(abi.nep_fleet_cfg, a).offset == getattr(abi.nep_plan_cfg, b).offset
    hdr = open(os.path.join(ROOT, "include", "neptune_fleet.h")).read()
    declared = set(re.findall(r"^int\s+(nep_[a-z_0-9]+)\(", hdr, re.M))
    assert declared == set(_lib.FLEET_EXPORTS) and all(hasattr(L, n) for n in declared)
    for name, v in (("NEP_FLEET_SKIPPED", 0), ("NEP_FLEET_FE_NO_SOLUTION", 1), ("NEP_FLEET_QP_FAILED", 2), ("NEP_FLEET_REJECTED", 3),
                    ("NEP_FLEET_ACCEPTED", 4), ("NEP_FLEET_CAP", 5), ("NEP_FLEET_N_COUNTERS", 8), ("NEP_FLEET_FLAG_SEG", 1),
                    ("NEP_FLEET_FLAG_RING", 2), ("NEP_FLEET_FLAG_SPLICE", 4)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr) and getattr(abi, name) == v, name
    assert abi.FLEET_OUTCOMES[abi.NEP_FLEET_ACCEPTED] == "accepted" and abi.FLEET_OUTCOMES[abi.NEP_FLEET_REJECTED] == "rejected_by_safety"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input='#include "neptune_fleet.h"\n', text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_fleet_fails_loudly_without_a_gpu(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = abi.nep_fleet_cfg(0.01, 0.5, 0.065, 0.065, 0.0, 1.0, 6, 5, 5, 0, 0.2, 0.0)
    calls = [lambda: L.nep_batch_fleet_init(None, C.byref(cfg), None, None, None, None, None),
             lambda: L.nep_batch_fleet_select(None, None, None, None, None, None),
             lambda: L.nep_batch_fleet_commit(None, None, None, None, None, None, None),
             lambda: L.nep_batch_fleet_tick(None, None),
             lambda: L.nep_batch_fleet_ring_cap(None),
             lambda: L.nep_batch_fleet_plans(None, 0, 0, None, None),
             lambda: L.nep_batch_fleet_state(None, None, None, None, None, None, None, None),
             lambda: L.nep_batch_fleet_counters(None, None, None, None)]
    for k, call in enumerate(calls):
        L.nep_batch_check(None, None)      # (leaves another message behind)
        assert call() == -3, k             # NEP_E_HIP
        assert b"no HIP device" in L.nep_last_error(), k


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _rebase(c, s):
    return [c[0], 3 * c[0] * s + c[1], (3 * c[0] * s + 2 * c[1]) * s + c[2], ((c[0] * s + c[1]) * s + c[2]) * s + c[3]]


def _append_span(times, coeff, p_times, p_coeff, t0, t1):
    """p restricted to [t0, t1] appended to (times, coeff); coeff entries are [3][4]; False beyond NEP_TRAJ_MAX_SEG intervals"""
    n = len(p_coeff)
    a = t0
    while a < t1:
        k = 0
        while k < n and p_times[k + 1] <= a:
            k += 1
        if len(coeff) >= abi.NEP_TRAJ_MAX_SEG:
            return False
        if k >= n:
            b = t1
            T = p_times[n] - p_times[n - 1]
            coeff.append([[0.0, 0.0, 0.0, _rebase(p_coeff[n - 1][ax], T)[3]] for ax in range(3)])
        else:
            b = p_times[k + 1] if p_times[k + 1] < t1 else t1
            d = a - p_times[k]
            s = d if d > 0 else 0.0
            coeff.append([_rebase(p_coeff[k][ax], d if d < 0 else s) for ax in range(3)])
        times.append(b)
        a = b
    return True


def _compose_exact(t, p1, p2):
    (t1s, c1), (t2s, c2) = p1, p2
    times, coeff = [t], []
    if t < t2s[0]:
        if not _append_span(times, coeff, t1s, c1, t, t2s[0]):
            return None
        for i in range(len(c2)):
            if len(coeff) >= abi.NEP_TRAJ_MAX_SEG:
                return None
            times.append(t2s[i + 1]); coeff.append([list(c2[i][ax]) for ax in range(3)])
    elif not _append_span(times, coeff, t2s, c2, t, t2s[-1] if t2s[-1] > t else t + 1.0):
        return None
    return times, coeff


def _to_pwp(tc):
    times, coeff = tc
    return plan.make_pwp(np.array(times), np.array(coeff).transpose(1, 0, 2))


def _random_pwp(rng, t0, n):
    times = [t0]
    for _ in range(n):
        times.append(times[-1] + float(rng.uniform(0.05, 0.6)))
    return times, [[[float(v) for v in rng.normal(size=4)] for _ in range(3)] for _ in range(n)]


class _Plan:
    """nep_plan_* in Python floats"""

    def __init__(self, dc, T_span, lo, hi, runtime_opt, deltaT0):
        self.dc, self.T, self.lo, self.hi, self.ro, self.deltaT, self.q = dc, T_span, lo, hi, runtime_opt, deltaT0, []

    def select_a(self, pos, t_now):
        size = len(self.q)
        ilo, ihi = int(self.lo / self.dc), int(self.hi / self.dc)
        self.deltaT = ilo if self.deltaT < ilo else (ihi if self.deltaT > ihi else self.deltaT)
        fi = size - self.deltaT
        k_end = fi if fi > 0 else 0
        if float(size) < math.ceil(self.T / self.dc):
            k_end = 0
        k = size - 1 - k_end
        A = list(self.q[k])
        if fi < 0:
            A[3:9] = [0.0] * 6
        h = self.q[0]
        dx, dy, dz = h[0] - pos[0], h[1] - pos[1], h[2] - pos[2]
        far = math.sqrt(dx * dx + dy * dy + dz * dz) > 1.0
        if far:
            A[0:3] = list(pos)
        rs = k * self.dc - self.ro if k_end != 0 else self.hi
        slo, shi = self.lo - self.ro, self.hi - self.ro
        rs = slo if rs < slo else (shi if rs > shi else rs)
        return dict(A=A, k_index=k, k_index_end=k_end, runtime_search=rs, t_start=k * self.dc + t_now, short=float(size) < math.ceil(self.T / self.dc),
                    fi=fi, far=far)

    def splice(self, k_end, states):
        keep = len(self.q) - 1 - k_end
        if keep < 0:
            return False
        self.q = self.q[:keep] + [list(s) for s in states]
        return True

    def next_goal(self):
        g = self.q[0]
        if len(self.q) > 1:
            self.q = self.q[1:]
            return g, False
        return g, True


@pytest.mark.parametrize("cfg", [(0.1, 0.5, 0.65, 0.65, 0.0, 6), (0.01, 0.5, 0.03, 0.9, 0.01, 75), (0.05, 0.5, 0.4, 0.2, 0.1, 3)])
def test_plan_calls_are_unchanged_by_the_shared_header(L, cfg):
    dc, T, lo, hi, ro, d0 = cfg
    rng = np.random.default_rng(20 + d0)
    host = plan.CommittedPlan(dc, T, lo, hi, ro, 1.0, deltaT0=d0)
    ref = _Plan(dc, T, lo, hi, ro, d0)
    seen = set()
    t = 0.0
    k_end = 0
    s0 = rng.normal(size=12)
    host.reset(s0); ref.q = [list(s0)]
    for step in range(600):
        op = rng.integers(0, 10)
        if op == 0:
            s0 = rng.normal(size=12) * 3
            host.reset(s0); ref.q = [list(map(float, s0))]
        elif op <= 3:
            n = int(rng.integers(0, 60))
            st = rng.normal(size=(n, 12)) * 2
            if step % 7 == 0:
                k_end = len(ref.q) + int(rng.integers(0, 3))      # "Already published the point A"
            ok = ref.splice(k_end, st.tolist())
            if ok and len(ref.q) == 0:      # (an empty plan answers NEP_E_STATE to everything: keep one state)
                ref.q = [list(map(float, s0))]; host.reset(s0)
                continue
            if ok:
                host.splice(k_end, st)
            else:
                seen.add("splice_state")
                with pytest.raises(plan.PlanError) as e:
                    host.splice(k_end, st)
                assert e.value.code == -2
        elif op <= 6:
            for _ in range(int(rng.integers(1, 12))):
                g, last = host.next_goal(); gr, lr = ref.next_goal()
                assert g.tobytes() == np.array(gr).tobytes() and last == lr
                t += dc
        else:
            head = np.array(ref.q[0][:3])
            pos = head + (rng.normal(size=3) * 5 if rng.integers(0, 3) == 0 else rng.normal(size=3) * 0.1)
            pa = host.select_a(pos, t); r = ref.select_a([float(v) for v in pos], t)
            assert np.array([pa.A[i] for i in range(12)]).tobytes() == np.array(r["A"], dtype=np.float64).tobytes(), step
            assert (pa.k_index, pa.k_index_end) == (r["k_index"], r["k_index_end"])
            assert np.float64(pa.runtime_search).tobytes() == np.float64(r["runtime_search"]).tobytes()
            assert np.float64(pa.t_start).tobytes() == np.float64(r["t_start"]).tobytes()
            assert host.deltaT == ref.deltaT
            k_end = r["k_index_end"]
            seen |= {"short" if r["short"] else "long", "fi<0" if r["fi"] < 0 else "fi>=0", "far" if r["far"] else "near",
                     "k_end>0" if k_end > 0 else "k_end=0"}
        assert len(host) == len(ref.q)
        assert host.to_array().tobytes() == np.array(ref.q, dtype=np.float64).reshape(-1, 12).tobytes(), step
    want = {"short", "long", "fi<0", "fi>=0", "far", "near", "splice_state"} | ({"k_end>0"} if lo <= hi else set())
    assert want <= seen, want - seen
    host.close()


def test_compose_exact_is_unchanged_by_the_shared_header(L):
    rng = np.random.default_rng(7)
    seen = set()
    for trial in range(400):
        n1, n2 = int(rng.integers(1, 17)), int(rng.integers(1, 9))
        p1 = _random_pwp(rng, float(rng.uniform(-1, 1)), n1)
        kind = trial % 5
        if kind == 0:      # the usual: t inside p1, p2 starts later inside p1
            t = float(rng.uniform(p1[0][0], p1[0][-1])); t2 = float(rng.uniform(t, p1[0][-1] + 0.2))
        elif kind == 1:    # the new trajectory has already started
            t2 = float(rng.uniform(p1[0][0], p1[0][-1])); t = t2 + float(rng.uniform(0, 1.5))
        elif kind == 2:    # t beyond p1's last knot, p2 later still: the end point is held
            t = p1[0][-1] + float(rng.uniform(0, 2)); t2 = t + float(rng.uniform(0.01, 1))
        elif kind == 3:    # t before p1's first knot
            t = p1[0][0] - float(rng.uniform(0, 0.5)); t2 = float(rng.uniform(p1[0][0], p1[0][-1]))
        else:              # t exactly on knots
            t = p1[0][int(rng.integers(0, n1 + 1))]; t2 = p1[0][int(rng.integers(0, n1 + 1))]
        p2 = _random_pwp(rng, t2, n2)
        want = _compose_exact(t, p1, p2)
        a, b = _to_pwp(p1), _to_pwp(p2)
        if want is None:
            seen.add("cap")
            with pytest.raises(plan.PlanError) as e:
                plan.compose_exact(t, a, b)
            assert e.value.code == -4
            continue
        got = plan.compose_exact(t, a, b)
        assert bytes(got) == bytes(_to_pwp(want)), (trial, kind)
        seen |= {"t>=t2" if t >= p2[0][0] else "t<t2"} | ({"beyond_p1"} if t > p1[0][-1] and t < t2 else set()) | ({"past_p2"} if t >= p2[0][-1] else set())
    assert {"cap", "t>=t2", "t<t2", "beyond_p1", "past_p2"} <= seen, seen
    # a chain, as a loop composes: the result is the next round's p1
    prev = _random_pwp(rng, 0.0, 3)
    t = 0.0
    for r in range(60):
        t += 0.05 * int(rng.integers(1, 4))
        new = _random_pwp(rng, t + 0.06, int(rng.integers(1, 9)))
        want = _compose_exact(t, prev, new)
        if want is None:
            prev = new
            continue
        assert bytes(plan.compose_exact(t, _to_pwp(prev), _to_pwp(new))) == bytes(_to_pwp(want)), r
        prev = want
