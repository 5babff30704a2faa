"""CPU: the move-back rule of the fleet loops (include/neptune_fleet.h, "move-back") as far as it can be checked without a GPU —
the host form nep_moveback_step against a restatement in Python floats and ints (tests/moveback_ref.py), exactly, on seeded cases;
the two strict comparisons on exactly representable numbers; a radius of 0 and below; no t_issue; the other bits of the word; every
byte of a start record but the goal's x and y; set and release in one call; the argument checks; the ABI; both loops' argument
checks; and a stand-alone sanitizer build of the host form."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import moveback_ref as ref
from neptune_amd import _lib, abi, mission

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WB = abi.NEP_FLEET_FLAG_WAY_BACK


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _starts(n, rng=None):
    st = np.zeros(n, dtype=abi.FE_START_DTYPE)
    if rng is not None:
        st.view(np.float64)[:] = rng.uniform(-9.0, 9.0, n * abi.FE_START_DTYPE.itemsize // 8)
    return st


def _both(radius, timeout, state, pb, t_issue, t_first, t_now, flags, start):
    """the host form and the reference on copies -> (flags, start, events), after asserting that they agree exactly"""
    f, s = np.array(flags, dtype=np.int32), start.copy()
    mission.moveback_step(abi.nep_moveback_cfg(radius, timeout), state, pb, t_issue, t_first, t_now, f, s)
    rf, rg, ev = ref.step(radius, timeout, state, pb, t_issue, t_first, t_now, flags, start["goal"])
    assert f.tolist() == rf
    assert s["goal"].tobytes() == np.array(rg, dtype=np.float64).tobytes()
    return f, s, ev


def test_matches_reference_on_seeded_cases(L):
    """positions on a 1/8 grid around bases on a 1/4 grid (so that distances hit the radius exactly now and then), clocks on a 1/4
    grid (so that t_issue == t_now and age == timeout happen), random words"""
    rng = np.random.default_rng(7)
    seen = set()
    for case in range(200):
        n = int(rng.integers(1, 40))
        radius = float(rng.choice([-1.0, 0.0, 0.625, 2.5, 5.0]))
        timeout = float(rng.choice([0.0, 0.5, 1.0, 10.0]))
        pb = rng.integers(-8, 9, (n, 2)) / 4.0
        state = np.zeros((n, 12)); state[:, :2] = pb + rng.integers(-48, 49, (n, 2)) / 8.0; state[:, 2:] = rng.normal(size=(n, 10))
        t_now = float(rng.integers(0, 12)) / 4.0
        t_issue = t_now - rng.integers(0, 6, n) / 4.0
        flags = rng.integers(0, 32, n).astype(np.int32)
        start = _starts(n, rng)
        use_issue = case % 3 != 0
        f, s, ev = _both(radius, timeout, state, pb, t_issue if use_issue else None, t_now if case % 2 else 0.0, t_now, flags, start)
        for e in ev:
            seen.add(frozenset(e))
    assert {frozenset(), frozenset({"set"}), frozenset({"set", "radius"}), frozenset({"radius"}), frozenset({"timeout"})} <= seen


def test_boundaries_are_strict(L):
    state = np.zeros((1, 12)); state[0, :2] = [3.0, 4.0]
    pb = np.zeros((1, 2))
    start = _starts(1); start["goal"] = [[7.0, 8.0, 1.5]]
    up = math.nextafter(5.0, math.inf)
    f, s, _ = _both(5.0, 100.0, state, pb, [0.0], 0.0, 1.0, [WB], start)      # d == radius: on its way back still
    assert f[0] == WB and s["goal"].tolist() == [[0.0, 0.0, 1.5]]
    f, s, _ = _both(up, 100.0, state, pb, [0.0], 0.0, 1.0, [WB], start)       # the next double above: released
    assert f[0] == 0 and s["goal"].tolist() == [[7.0, 8.0, 1.5]]
    f, s, _ = _both(-1.0, 1.0, state, pb, [1.0], 0.0, 2.0, [WB], start)       # age == timeout: not released
    assert f[0] == WB
    f, s, _ = _both(-1.0, 1.0, state, pb, [1.0], 0.0, math.nextafter(2.0, math.inf), [WB], start)
    assert f[0] == 0


def test_radius_zero_and_negative_release_by_timer_only(L):
    state = np.zeros((2, 12))      # both sit ON their bases
    pb = np.zeros((2, 2))
    start = _starts(2); start["goal"] = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    for radius in (0.0, -2.0):
        f, s, ev = _both(radius, 0.5, state, pb, [0.0, 0.0], 0.0, 0.0, [0, 0], start)
        assert f.tolist() == [WB, WB] and ev == [{"set"}, {"set"}]
        f, s, ev = _both(radius, 0.5, state, pb, [0.0, 0.0], 0.0, 0.5, f, start)
        assert f.tolist() == [WB, WB]
        f, s, ev = _both(radius, 0.5, state, pb, [0.0, 0.0], 0.0, 0.75, f, start)
        assert f.tolist() == [0, 0] and ev == [{"timeout"}, {"timeout"}] and s.tobytes() == start.tobytes()


def test_t_issue_null_takes_t_first(L):
    state = np.zeros((3, 12)); state[:, 0] = 9.0
    pb = np.zeros((3, 2))
    start = _starts(3)
    f, _, _ = _both(1.0, 10.0, state, pb, None, 2.5, 2.5, [0, 0, 0], start)
    assert f.tolist() == [WB] * 3
    f, _, _ = _both(1.0, 10.0, state, pb, None, 2.5, 2.75, [0, WB, 0], start)      # nobody is set later; who is on his way stays
    assert f.tolist() == [0, WB, 0]
    f, _, _ = _both(1.0, 10.0, state, pb, None, 0.0, 12.75, [0, WB, 0], start)     # ... until the timer
    assert f.tolist() == [0, 0, 0]


def test_other_bits_and_other_bytes_kept(L):
    rng = np.random.default_rng(3)
    n = 16
    state = np.zeros((n, 12)); state[:, :2] = rng.uniform(-9, 9, (n, 2))
    pb = rng.uniform(-9, 9, (n, 2))
    start = _starts(n, rng)
    flags = (np.arange(n) % 16).astype(np.int32)      # every combination of the four sticky bits
    state0 = state.copy(); pb0 = pb.copy()
    f, s, _ = _both(0.5, 10.0, state, pb, np.zeros(n), 0.0, 0.0, flags, start)
    assert (f & 15).tolist() == flags.tolist() and (f & WB).all()
    assert state.tobytes() == state0.tobytes() and pb.tobytes() == pb0.tobytes()
    a, b = s.copy(), start.copy()
    assert (a["goal"][:, :2] == pb).all()
    a["goal"][:, :2] = 0.0; b["goal"][:, :2] = 0.0
    assert a.tobytes() == b.tobytes()      # pos, vel, accel, the goal's z, t_start: every other byte
    f2, s2, _ = _both(0.5, 10.0, state, pb, np.zeros(n), 0.0, 20.0, f, start)
    assert f2.tolist() == flags.tolist() and s2.tobytes() == start.tobytes()


def test_set_and_release_in_one_call(L):
    state = np.zeros((1, 12)); state[0, :2] = [1.0, 1.0]
    pb = np.array([[1.0, 1.5]])
    start = _starts(1); start["goal"] = [[5.0, 5.0, 1.0]]
    f, s, ev = _both(2.0, 10.0, state, pb, [3.0], 0.0, 3.0, [8], start)
    assert f[0] == 8 and ev == [{"set", "radius"}] and s.tobytes() == start.tobytes()


def test_argument_checks(L):
    cfg = abi.nep_moveback_cfg(1.0, 10.0)
    state = np.zeros((1, 12)); pb = np.zeros((1, 2)); flags = np.zeros(1, dtype=np.int32); start = _starts(1)
    state[0, 0] = 5.0
    ok = [C.byref(cfg), 1, state.ctypes.data, pb.ctypes.data, None, 0.0, 0.0, flags.ctypes.data, start.ctypes.data]
    assert L.nep_moveback_step(*ok) == 0 and flags[0] == WB
    for k in (0, 2, 3, 7, 8):
        bad = list(ok); bad[k] = None
        assert L.nep_moveback_step(*bad) == -1, k
    bad = list(ok); bad[1] = -1
    assert L.nep_moveback_step(*bad) == -1
    for radius, timeout in ((math.nan, 10.0), (math.inf, 10.0), (-math.inf, 10.0), (1.0, -0.5), (1.0, math.nan), (1.0, math.inf)):
        bad = list(ok); bad[0] = C.byref(abi.nep_moveback_cfg(radius, timeout))
        assert L.nep_moveback_step(*bad) == -1, (radius, timeout)
        with pytest.raises(ValueError):
            mission.MoveBack(radius, timeout)
    assert L.nep_moveback_step(C.byref(abi.nep_moveback_cfg(-3.0, 0.0)), *ok[1:]) == 0      # a radius <= 0 and a timeout of 0 are fine
    import torch
    want = -1 if torch.cuda.is_available() else -3      # NEP_E_ARG / NEP_E_HIP
    assert L.nep_batch_fleet_moveback(None, C.byref(cfg), None, None) == want


def test_moveback_abi(L):
    assert L.nep_abi_sizeof(27) == C.sizeof(abi.nep_moveback_cfg) == 16
    assert L.nep_abi_sizeof(26) == -1 and L.nep_abi_sizeof(28) == -1
    hdr = open(os.path.join(ROOT, "include", "neptune_fleet.h")).read()
    assert int(re.search(r"#define NEP_FLEET_FLAG_WAY_BACK (\d+)\b", hdr).group(1)) == abi.NEP_FLEET_FLAG_WAY_BACK == ref.WAY_BACK == 16
    assert abi.NEP_FLEET_FLAG_ERRORS == 15 and not abi.NEP_FLEET_FLAG_ERRORS & WB
    for name in ("nep_batch_fleet_moveback", "nep_moveback_step"):
        assert name in _lib.FLEET_EXPORTS and getattr(L, name)
    assert re.search(r"^int nep_batch_fleet_moveback\(nep_batch_t\* h, const nep_moveback_cfg\* cfg, nep_fe_start\* d_start, void\* stream\);", hdr, re.M)
    assert re.search(r"^typedef struct nep_moveback_cfg \{ double radius, timeout; \} nep_moveback_cfg;", hdr, re.M)
    assert "not built" not in re.search(r"use_moveback_.*", hdr).group(0).split(".")[0]
    m = mission.MoveBack.reference(5)
    assert (m.radius, m.timeout) == (6.33 - 0.33, 10.0) and mission.MoveBack.reference(4).radius == 6.33
    assert mission.MoveBack.reference(24).radius <= 0.0 < mission.MoveBack.reference(23).radius
    c = mission.MoveBack(2, 3).cfg()
    assert (c.radius, c.timeout) == (2.0, 3.0)


def test_loops_refuse_a_bad_moveback():
    """before anything touches a device"""
    from neptune_amd import scene
    from neptune_amd.loop import DeviceFleetLoop, FleetLoop
    sc = scene.make_scene(5, 3, seed=0)
    for bad in (5.0, "ref", (1.0, 10.0), abi.nep_moveback_cfg(1.0, 10.0)):
        with pytest.raises(TypeError):
            DeviceFleetLoop([sc], moveback=bad)
        with pytest.raises(TypeError):
            FleetLoop(sc["par"], sc["statics"], sc["starts"], sc["goals"], moveback=bad)
    with pytest.raises(ValueError):
        DeviceFleetLoop([sc], moveback=dict(radius=float("nan"), timeout=1.0))
    assert "moveback" in DeviceFleetLoop._MUST_MATCH


def test_host_form_under_sanitizers(tmp_path):
    """tests/cpp/moveback_check.cpp drives moveback_host.cpp (host code only, its own main) through seeded walks, built with
    -fsanitize=address,undefined"""
    exe = str(tmp_path / "moveback_check")
    src = [os.path.join(ROOT, "tests", "cpp", "moveback_check.cpp"), os.path.join(ROOT, "neptune_amd", "csrc", "moveback_host.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include")] + src + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "moveback_check ok" in r.stdout, (r.stdout, r.stderr)
