"""CPU: the list form of the tracked tether state (nep_ent_lists) — its symbols and layout — and the premises of the GPU tests of
tests/test_gpu_ent_lists.py: the pre-walked seeds of tests/ent_lists_seeds.py hold lists above NEP_FE_ENT_CAP entries and short ones,
within the bend limit and exact under cap = 112."""
import ctypes as C
import os
import re

import numpy as np

import ent_lists_seeds as seeds
from neptune_amd import _lib, abi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def test_symbols_and_struct_size():
    L = _lib.lib()
    for name in ("nep_batch_track_ent_lists", "nep_batch_ent_lists_at_a"):
        assert name in _lib.FE_EXPORTS and getattr(L, name)
    for name in ("nep_batch_fleet_init_ent_lists", "nep_batch_fleet_ent_lists"):
        assert name in _lib.FLEET_EXPORTS and getattr(L, name)
    assert L.nep_abi_sizeof(23) == C.sizeof(abi.nep_ent_lists) == 56
    assert L.nep_abi_sizeof(16) == -1 and L.nep_abi_sizeof(22) == -1 and L.nep_abi_sizeof(24) == -1
    assert [L.nep_abi_sizeof(k) for k in range(16)] == [1680, 1872, 56, 48, 152, 784, 896, 48, 24, 56, 120, 64, 104, 56, 456, 56]      # nothing else moved
    fe = open(os.path.join(INCLUDE, "neptune_frontend.h")).read()
    assert int(re.search(r"#define NEP_ENT_LISTS_MAX_CAP (\d+)", fe).group(1)) == abi.NEP_ENT_LISTS_MAX_CAP == 4096
    ent = open(os.path.join(INCLUDE, "neptune_entangle.h")).read()
    assert int(re.search(r"#define NEP_ENT_TRACK_HELD (\d+)", ent).group(1)) == abi.NEP_ENT_TRACK_HELD == 32
    # the flag is a bit of its own
    assert abi.NEP_ENT_TRACK_HELD & (abi.NEP_ENT_TRACK_ENTANGLED | abi.NEP_ENT_TRACK_TWO_CASES | abi.NEP_ENT_TRACK_TOO_LONG | abi.NEP_ENT_TRACK_CAP | abi.NEP_ENT_TRACK_ABORT) == 0


def test_host_lists_mirror():
    from neptune_amd import entangle
    ls = abi.EntLists(3, 50)
    st = entangle.State(6, cap=50)
    st.alphas[:3] = [(2, 1), (5, 0), (2, 3)]; st.betas[:3] = [0.0, -1.5, 0.0]; st.bend_idx[:1] = [1]
    st.c.n_alpha, st.c.n_bend = 3, 1
    ls.set_state(1, st)
    seeds.assert_lists_equal(ls, 1, st, "mirror")
    seeds.assert_lists_equal(ls, 0, entangle.State(6, cap=50), "empty")
    assert ls.c.cap == 50 and ls.c.id[50] == 2 and ls.c.beta[51] == -1.5 and ls.c.bend[abi.NEP_MAX_BEND] == 1
    assert len(ls.tobytes()) == 3 * (4 + 4 + 50 * 11 + abi.NEP_MAX_BEND * 2)


def test_seed_conditions():
    """what the GPU tests rest on: per scene pair long (>= 48) and short (<= 30) seeds, at most 5 bend points, walked without a
    NEP_ENT_TRACK_CAP under cap = 112; every other slot empty"""
    scenes, states, kinds = seeds.seeded_scenes(cap=seeds.CAP)
    assert len(scenes) == 2 and all(sc["par"].num_agents == 20 and len(sc["statics"]) == 8 for sc in scenes)
    n_long = n_short = 0
    for s, seed in enumerate(seeds.SCENE_SEEDS):
        walked, flags = seeds.prewalk(20, 8, seed)
        for a, (st, k) in enumerate(zip(states[s], kinds[s])):
            n, b = st.c.n_alpha, st.c.n_bend
            if k is None:
                assert n == 0 and b == 0
                continue
            assert not (flags[a] & abi.NEP_ENT_TRACK_CAP) and b <= 5 and n <= seeds.CAP
            assert (n, b) == (walked[a].c.n_alpha, walked[a].c.n_bend)
            assert (k == "long" and n >= 48) or (k == "short" and n <= 30)
            n_long += k == "long"; n_short += k == "short"
            assert all(0 <= int(x) < n for x in st.bend_idx[:b])
    print("seeds: %d long, %d short" % (n_long, n_short), [[st.c.n_alpha for st in row] for row in states])
    assert n_long >= 2 and n_short >= 2
    assert all("long" in kd and "short" in kd for kd in kinds)      # (the fleet test wants held and planning slots in round 0)
    short = seeds.seeded_scenes(cap=seeds.CAP, short_only=True)[1]
    assert max(st.c.n_alpha for row in short for st in row) <= 30 and any(st.c.n_alpha > 0 for row in short for st in row)
