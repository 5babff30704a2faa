"""CPU: the active-set entry point of the batched handle (nep_batch_set_active) is exported and bound, its status codes mirror the
headers, and no record changed size for it.  No compute calls (no GPU here)."""
import os
import re

import pytest

from neptune_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _define(header, name):
    m = re.search(r"^#define\s+%s\s+\(?(-?\d+)\)?" % name, open(os.path.join(ROOT, "include", header)).read(), re.M)
    assert m, name
    return int(m.group(1))


def test_set_active_is_exported_and_bound(L):
    assert "nep_batch_set_active" in _lib.EXPORTS
    assert hasattr(L, "nep_batch_set_active")
    assert L.nep_batch_set_active.argtypes is not None and len(L.nep_batch_set_active.argtypes) == 2
    hdr = open(os.path.join(ROOT, "include", "neptune_backend.h")).read()
    assert re.search(r"^int nep_batch_set_active\(nep_batch_t\* h, const int32_t\* d_active\);", hdr, re.M)


def test_skipped_status_codes_match_the_headers():
    assert abi.NEP_SKIPPED == _define("neptune_backend.h", "NEP_SKIPPED") == 3
    assert abi.NEP_FE_SKIPPED == _define("neptune_frontend.h", "NEP_FE_SKIPPED") == 4
    # distinct from every other status of the same field
    assert abi.NEP_SKIPPED not in (abi.NEP_OK, abi.NEP_RELAXED, abi.NEP_FAILED)
    assert abi.NEP_FE_SKIPPED not in [_define("neptune_frontend.h", n) for n in
                                      ("NEP_FE_GOAL_REACHED", "NEP_FE_DEPTH_REACHED", "NEP_FE_EMPTY", "NEP_FE_NO_SOLUTION")]


def test_set_active_refuses_a_null_handle(L):
    assert L.nep_batch_set_active(None, None) == -1        # NEP_E_ARG


def test_record_sizes_are_unchanged(L):
    # nep_abi_sizeof(0..13) before the active set was added: the feature adds no field to any record
    assert [L.nep_abi_sizeof(k) for k in range(14)] == [1680, 1872, 56, 48, 152, 784, 896, 48, 24, 56, 120, 64, 104, 56]
