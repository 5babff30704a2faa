"""The best-first front end's C ABI and its Python mirror, without a GPU: the library exports the two entry points, _lib.py
declares their signatures as include/neptune_frontend.h states them, and the loops refuse what the search cannot fly."""
import ctypes as C
import os
import re

import pytest

from neptune_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_points_with_the_headers_signatures():
    L = _lib.lib()
    vp, i = C.c_void_p, C.c_int32
    assert {"nep_batch_set_fe_astar", "nep_batch_frontend_astar"} <= set(_lib.FE_EXPORTS)
    assert L.nep_batch_set_fe_astar.argtypes == [vp, i, i, C.POINTER(i), i]
    assert L.nep_batch_frontend_astar.argtypes == [vp, C.POINTER(abi.nep_fe_cfg), vp, vp, vp, vp, vp]
    with open(os.path.join(ROOT, "include", "neptune_frontend.h")) as f:
        hdr = re.sub(r"\s+", " ", f.read())
    assert "int nep_batch_set_fe_astar(nep_batch_t* h, int32_t max_pops, int32_t max_nodes, const int32_t* order, int32_t n_order);" in hdr
    assert ("int nep_batch_frontend_astar(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start, "
            "nep_guess* d_guess, nep_fe_result* d_result, void* stream);") in hdr
    assert "#define NEP_FE_ASTAR_MAX_NODES 20000" in hdr and "#define NEP_FE_ASTAR_NODE_BYTES 160" in hdr


def test_null_handle_is_an_argument_error():
    L = _lib.lib()
    assert L.nep_batch_set_fe_astar(None, 100, 0, None, 0) == -1            # NEP_E_ARG (no HIP call is made for it)
    assert L.nep_batch_frontend_astar(None, None, None, None, None, None, None) == -1


def test_loops_refuse_astar_with_tethers_and_unknown_strategies():
    from neptune_amd import loop
    assert loop.check_search("beam", 300, True) is False and loop.check_search("astar", 300, False) is True
    for search, pops, tethers in (("astar", 300, True), ("dijkstra", 300, False), ("astar", 0, False)):
        with pytest.raises(ValueError):
            loop.check_search(search, pops, tethers)
