"""The entangle-aware best-first front end's C ABI and its Python mirror, without a GPU: the library exports the entry point, _lib.py
declares its signature as include/neptune_frontend.h states it, and the loops take search="astar_ent" with tethers only."""
import ctypes as C
import os
import re

import pytest

from neptune_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_point_with_the_headers_signature():
    L = _lib.lib()
    vp = C.c_void_p
    assert "nep_batch_frontend_astar_ent" in _lib.FE_EXPORTS
    assert L.nep_batch_frontend_astar_ent.argtypes == [vp, C.POINTER(abi.nep_fe_cfg), vp, vp, vp, vp, vp, vp, vp]
    assert L.nep_batch_frontend_astar_ent.argtypes == L.nep_batch_frontend_ent.argtypes
    with open(os.path.join(ROOT, "include", "neptune_frontend.h")) as f:
        hdr = re.sub(r"\s+", " ", f.read())
    assert ("int nep_batch_frontend_astar_ent(nep_batch_t* h, const nep_fe_cfg* cfg, const nep_traj_rec* d_committed, const nep_fe_start* d_start, "
            "const nep_fe_ent_state* d_ent_init, nep_guess* d_guess, nep_fe_result* d_result, int32_t* d_case_out, void* stream);") in hdr
    assert "#define NEP_FE_ASTAR_ENT_NODE_BYTES %d" % abi.FE_ENT_STATE_DTYPE.itemsize in hdr      # (a node's state is the fixed record)


def test_null_handle_is_an_argument_error():
    L = _lib.lib()
    assert L.nep_batch_frontend_astar_ent(None, None, None, None, None, None, None, None, None) == -1      # NEP_E_ARG (no HIP call is made for it)


def test_loops_take_astar_ent_with_tethers_only():
    from neptune_amd import loop
    assert loop.check_search("astar_ent", 150, True) is True
    for search, pops, tethers in (("astar_ent", 150, False), ("astar_ent", 0, True), ("astar", 150, True)):
        with pytest.raises(ValueError):
            loop.check_search(search, pops, tethers)
    from neptune_amd.backend import BatchBackend
    assert callable(BatchBackend.frontend_astar_ent)
