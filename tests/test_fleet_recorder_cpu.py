"""CPU: the fleet recorder (include/neptune_fleet.h, "recorder") as far as it can be checked without a GPU — the ABI, the header
check of nep_fleet_snapshot_describe, the section offsets against a restatement in Python, the entry points' contracts without a
device, and a stand-alone sanitizer build of the host code."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from neptune_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEP_E_ARG = -1


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_recorder_abi(L):
    # (index 24 is pinned to -1 by tests/test_ent_lists_cpu.py, as 22 is by the mission tests: the header takes the next one)
    assert L.nep_abi_sizeof(25) == C.sizeof(abi.nep_fleet_snapshot_hdr) == abi.NEP_SNAPSHOT_HDR_BYTES == 80
    assert L.nep_abi_sizeof(26) == -1 and L.nep_abi_sizeof(24) == -1 and L.nep_abi_sizeof(22) == -1
    assert L.nep_abi_sizeof(23) == C.sizeof(abi.nep_ent_lists)
    assert abi.SNAPSHOT_STAMP_DTYPE.itemsize == 16 and len(abi.SNAPSHOT_SECTIONS) == abi.NEP_SNAPSHOT_N_SECTIONS
    hdr = open(os.path.join(ROOT, "include", "neptune_fleet.h")).read()
    assert int(re.search(r"#define NEP_SNAPSHOT_MAGIC (0x[0-9a-f]+)u", hdr).group(1), 16) == abi.NEP_SNAPSHOT_MAGIC
    for name in ("NEP_SNAPSHOT_VERSION", "NEP_SNAPSHOT_HDR_BYTES", "NEP_SNAPSHOT_N_SECTIONS"):
        assert int(re.search(r"#define %s (\d+)\b" % name, hdr).group(1)) == getattr(abi, name), name
    # the enum's order is the mirror's
    enum = re.search(r"enum \{(.*?)\};", hdr, re.S).group(1)
    names = [n.strip().split(" ")[0] for n in enum.split(",")]
    assert [n[len("NEP_SNAP_"):].lower() for n in names] == list(abi.SNAPSHOT_SECTIONS)
    declared = set(re.findall(r"^(?:int|int64_t)\s+(nep_[a-z_0-9]+)\(", hdr, re.M))
    assert declared == set(_lib.FLEET_EXPORTS) | set(_lib.FLEET_SIZE_EXPORTS)
    for name in declared:
        assert hasattr(L, name), name


# ---- the layout, restated: a list of (section, bytes of one scene) from the header's fields -------------------------------------
PWP, ENT, LEG, MAX_BEND = abi.PWP_DTYPE.itemsize, abi.FE_ENT_STATE_DTYPE.itemsize, abi.MISSION_LEG_DTYPE.itemsize, abi.NEP_MAX_BEND


def sections_ref(N, ring_cap, form, cap, mode, log_cap, timers):
    ent, lists, mis = form != 0, form == 2, mode != 0
    owners = N if mode == abi.NEP_MISSION_PER_AGENT else 1
    ints = lambda on=True: 4 * N if on else 0      # noqa: E731
    return [("origin", 4), ("round", 4), ("ring", N * ring_cap * 12 * 8), ("head", ints()), ("size", ints()), ("k_end", ints()), ("state", N * 96),
            ("goal", N * 24), ("pwp", N * PWP), ("flown", ints()), ("done", ints()), ("outcome", ints()), ("sflags", ints()),
            ("period", ints(timers)), ("phase", ints(timers)), ("t_now", 8), ("counters", 4 * abi.NEP_FLEET_N_COUNTERS),
            ("ent", N * ENT if form == 1 else 0), ("l_n_alpha", ints(lists)), ("l_n_bend", ints(lists)), ("l_id", 2 * N * cap if lists else 0),
            ("l_cs", N * cap if lists else 0), ("l_beta", 8 * N * cap if lists else 0), ("l_bend", 2 * N * MAX_BEND if lists else 0), ("held", ints(lists)),
            ("pub_n", ints(ent)), ("pub_xy", 16 * N * MAX_BEND if ent else 0), ("pub_prev_n", ints(ent)), ("pub_prev_xy", 16 * N * MAX_BEND if ent else 0),
            ("ent_flags", ints(ent)), ("ent_ever", ints(ent)), ("ent_walked", ints(ent)),
            ("t_issue", 8 * N if mis else 0), ("length", 8 * N if mis else 0), ("completed", ints(mis)), ("counts", 16 * N if mis else 0),
            ("sums", 16 * N if mis else 0), ("scene_i", 16 if mis else 0), ("t_run", 8 if mis else 0), ("log", owners * log_cap * LEG if mis else 0),
            ("log_n", 4 * owners if mis else 0)]


def make_hdr(n_scenes, N, ring_cap, form=0, cap=0, mode=0, log_cap=0, timers=0, **over):
    h = abi.nep_fleet_snapshot_hdr()
    h.magic, h.version, h.hdr_bytes = abi.NEP_SNAPSHOT_MAGIC, abi.NEP_SNAPSHOT_VERSION, abi.NEP_SNAPSHOT_HDR_BYTES
    h.n_scenes, h.N, h.num_pol, h.ring_cap, h.max_states = n_scenes, N, 8, ring_cap, 48
    h.tether_form, h.tether_cap, h.mission_mode, h.log_cap, h.timers = form, cap, mode, log_cap, timers
    h.scene_bytes = sum((b + 15) // 16 * 16 for _, b in sections_ref(N, ring_cap, form, cap, mode, log_cap, timers))
    h.cfg_hash = 0x1234567890abcdef
    for k, v in over.items():
        setattr(h, k, v)
    return h


def describe(L, h, nbytes=None):
    full = abi.NEP_SNAPSHOT_HDR_BYTES + h.n_scenes * max(int(h.scene_bytes), 0)
    info = abi.nep_fleet_snapshot_info()
    buf = C.create_string_buffer(bytes(h), C.sizeof(h))      # (only the header is read)
    return L.nep_fleet_snapshot_describe(buf, full if nbytes is None else nbytes, C.byref(info)), info


CONFIGS = dict(plain=dict(n_scenes=3, N=6, ring_cap=54),
               fixed_agent=dict(n_scenes=2, N=70, ring_cap=54, form=1, cap=abi.NEP_FE_ENT_CAP, mode=abi.NEP_MISSION_PER_AGENT, log_cap=2, timers=1),
               lists_runs=dict(n_scenes=3, N=6, ring_cap=20, form=2, cap=48, mode=abi.NEP_MISSION_FLEET_RUNS, log_cap=2))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_section_offsets(L, name):
    c = CONFIGS[name]
    h = make_hdr(**c)
    rc, info = describe(L, h)
    assert rc == 0, L.nep_last_error()
    assert bytes(info.hdr) == bytes(h)
    ref = sections_ref(c["N"], c["ring_cap"], c.get("form", 0), c.get("cap", 0), c.get("mode", 0), c.get("log_cap", 0), c.get("timers", 0))
    assert [n for n, _ in ref] == list(abi.SNAPSHOT_SECTIONS)
    at = 0
    for i, (n, b) in enumerate(ref):
        assert (info.offset[i], info.bytes[i]) == (at, b), n
        assert at % 16 == 0
        at += (b + 15) // 16 * 16
    assert at == h.scene_bytes and at % 16 == 0
    present = {n for n, b in ref if b}
    assert ("ent" in present) == (c.get("form", 0) == 1) and ("l_beta" in present) == (c.get("form", 0) == 2) and ("log" in present) == (c.get("mode", 0) != 0)


def test_describe_refuses(L):
    good = make_hdr(**CONFIGS["fixed_agent"])
    assert describe(L, good)[0] == 0
    full = abi.NEP_SNAPSHOT_HDR_BYTES + good.n_scenes * good.scene_bytes
    assert describe(L, make_hdr(**CONFIGS["fixed_agent"], magic=abi.NEP_SNAPSHOT_MAGIC + 1))[0] == NEP_E_ARG
    assert describe(L, make_hdr(**CONFIGS["fixed_agent"], version=abi.NEP_SNAPSHOT_VERSION + 1))[0] == NEP_E_ARG
    assert describe(L, good, full - 1)[0] == NEP_E_ARG and describe(L, good, abi.NEP_SNAPSHOT_HDR_BYTES)[0] == NEP_E_ARG
    assert describe(L, good, abi.NEP_SNAPSHOT_HDR_BYTES - 1)[0] == NEP_E_ARG
    assert describe(L, make_hdr(**CONFIGS["fixed_agent"], scene_bytes=good.scene_bytes + 8), 1 << 40)[0] == NEP_E_ARG      # not a multiple of 16
    assert describe(L, make_hdr(**CONFIGS["fixed_agent"], scene_bytes=good.scene_bytes - 16), 1 << 40)[0] == NEP_E_ARG     # log_n would end past the block
    assert b"past" in L.nep_last_error()
    bad = make_hdr(**CONFIGS["fixed_agent"]); bad.N = 0
    assert describe(L, bad, 1 << 40)[0] == NEP_E_ARG
    bad = make_hdr(**CONFIGS["lists_runs"]); bad.tether_cap = abi.NEP_FE_ENT_CAP      # lists of the fixed record's size
    assert describe(L, bad, 1 << 40)[0] == NEP_E_ARG
    assert L.nep_fleet_snapshot_describe(None, 80, None) == NEP_E_ARG


def test_entry_points_without_a_handle(L):
    """no handle (and here no device): an error code, never a crash"""
    assert L.nep_batch_fleet_snapshot_bytes(None) < 0 and L.nep_batch_fleet_snapshot_ring_bytes(None, 4) < 0
    assert L.nep_batch_fleet_snapshot(None, None, None) < 0 and L.nep_batch_fleet_snapshot_ring(None, None, 4, None) < 0
    assert L.nep_batch_fleet_restore(None, None, 0, -1, -1) < 0


def test_host_code_under_sanitizers(tmp_path):
    """tests/cpp/recorder_check.cpp drives recorder_host.cpp (host code only, its own main) over good, broken and truncated
    headers, built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "recorder_check")
    src = [os.path.join(ROOT, "tests", "cpp", "recorder_check.cpp"), os.path.join(ROOT, "neptune_amd", "csrc", "recorder_host.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "include")] + src + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "recorder_check ok" in r.stdout, (r.stdout, r.stderr)
