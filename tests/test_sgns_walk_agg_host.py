"""Walk aggregation, the parts that need no GPU: the predicate's edges (dw_sgns_walk_agg_active)
and the bad-size refusals of the new size / predicate entry points (no pointer is touched, no
launch happens)."""
import ctypes
import os

import pytest

from shallow_encoders import _native


@pytest.fixture
def lib():
    lib = _native.load()
    yield lib
    lib.dw_sgns_set_walk_agg({'0': 0, '1': 1}.get(os.environ.get('DW_SGNS_WALK_AGG', ''), -1))


def test_predicate_edges(lib):
    act = lib.dw_sgns_walk_agg_active
    assert lib.dw_sgns_set_walk_agg(-1) == _native.DW_OK
    # the flagship window (C3) and C2's: on
    assert act(8192, 80, 5, 5, 128) == 1
    assert act(64, 10, 2, 5, 128) == 1
    # L = 2R + 1: one centre per walk, 2R(L-2R) = 2R < 2L: auto keeps the per-term records,
    # mode 1 aggregates (only that test is skipped)
    assert act(3, 5, 2, 1, 64) == 0
    # 2R(L-2R) = 2L +- 1 cannot be met (the left side is even): the nearest pairs around the
    # threshold, R = 2: 4(L-4) >= 2L <=> L >= 8; R = 3: 6(L-6) >= 2L <=> L >= 9
    assert act(3, 7, 2, 1, 64) == 0      # 12 < 14
    assert act(3, 8, 2, 1, 64) == 1      # 16 = 16
    assert act(3, 8, 3, 1, 64) == 0      # 12 < 16
    assert act(3, 9, 3, 1, 64) == 1      # 18 = 18
    # d = 96: no 16-lane-group pass 1
    assert act(3, 12, 2, 1, 96) == 0
    assert act(3, 12, 2, 1, 192) == 0
    # T = 2R(1+K) past 64 (65 itself is odd: 64 on, 66 off)
    assert act(3, 12, 2, 15, 64) == 1    # T = 64
    assert act(3, 12, 3, 10, 64) == 0    # T = 66
    # the LDS fit: (L-2R) * 512 + (L-2R) * 8R + 4L bytes <= 64 KB at d >= 128
    assert act(3, 127, 5, 1, 128) == 1   # 117 centres: 65,092 B
    assert act(3, 128, 5, 1, 128) == 0   # 118 centres: 65,648 B
    assert act(0, 80, 5, 5, 128) == 0    # no walks
    assert lib.dw_sgns_set_walk_agg(1) == _native.DW_OK
    assert act(3, 5, 2, 1, 64) == 1 and act(3, 7, 2, 1, 64) == 1
    assert act(3, 12, 2, 1, 96) == 0 and act(3, 12, 3, 10, 64) == 0
    assert lib.dw_sgns_set_walk_agg(0) == _native.DW_OK
    assert act(8192, 80, 5, 5, 128) == 0


def test_bad_sizes_are_refused_before_any_pointer(lib):
    act, size = lib.dw_sgns_walk_agg_active, lib.dw_sgns_walks_workspace_bytes
    for bad in ((-1, 80, 5, 5, 128), (1, 10, 5, 5, 128), (1, 80, 0, 5, 128), (1, 80, 5, -1, 128),
                (1, 80, 5, 5, 0)):
        assert act(*bad) == _native.DW_E_INVALID_ARG
        assert b'dw_sgns_walk_agg_active: bad sizes' in lib.dw_last_error_string()
    nbytes = ctypes.c_size_t(7)
    for bad in ((-1, 80, 5, 5, 100, 128), (1, 10, 5, 5, 100, 128), (1, 80, 0, 5, 100, 128),
                (1, 80, 5, -1, 100, 128), (1, 80, 5, 5, 0, 128), (1, 80, 5, 5, 100, 0)):
        assert size(*bad, ctypes.byref(nbytes)) == _native.DW_E_INVALID_ARG
        assert b'dw_sgns_walks_workspace_bytes: bad sizes' in lib.dw_last_error_string()
    assert size(1, 80, 5, 5, 100, 128, None) == _native.DW_E_INVALID_ARG
    assert b'bytes is null' in lib.dw_last_error_string()
    assert size(1 << 40, 80, 5, 5, 100, 128, ctypes.byref(nbytes)) == _native.DW_E_INVALID_ARG
    assert b'too many records' in lib.dw_last_error_string()
    assert nbytes.value == 7
    assert lib.dw_sgns_set_walk_agg(2) == _native.DW_E_INVALID_ARG
    assert lib.dw_sgns_set_walk_agg(-2) == _native.DW_E_INVALID_ARG
