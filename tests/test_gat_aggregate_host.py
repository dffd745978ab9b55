"""Fused GAT aggregation, host side (no GPU): the exported symbols, the return-code ladders of gespmm_gat_softmax_stats_f32 and
gespmm_gat_aggregate_f32 — the checks run before any device work, so NULL or made-up device pointers are enough — and the route table
of gespmm_gat_aggregate_route."""
import ctypes
import os

import pytest

from test_heads_host import EALIGN, EINVAL, ERANGE, ROUTE_F

NEW = ("gespmm_gat_softmax_stats_f32", "gespmm_gat_aggregate_f32", "gespmm_gat_aggregate_route")
OK = 0x1000  # a made-up address: the checks look at the number only and return before anything could read it
BIG = (1 << 31) - 4096  # one past the largest count of 32-bit word positions


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_and_version(L):
    for name in NEW:
        assert name in L.EXPORTS
        getattr(L.lib, name)
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


def test_stats_return_codes(L):
    f = L.lib.gespmm_gat_softmax_stats_f32
    # (rowptr, colind, el, er, stats, M, K, H, nnz, slope, stream)
    none = (None,) * 5
    ok = (_p(OK),) * 5
    assert f(*none, 4, 4, 0, 10, 0.2, None) == EINVAL        # H < 1
    assert f(*none, -1, 4, 2, 10, 0.2, None) == EINVAL       # negative sizes
    assert f(*none, 4, 4, 2, -1, 0.2, None) == EINVAL
    assert f(*none, 4, 0, 2, 10, 0.2, None) == EINVAL        # K < 1
    assert f(*none, 4, -3, 2, 10, 0.2, None) == EINVAL
    assert f(*none, 0, 4, 2, 10, 0.2, None) == EINVAL        # entries without rows
    assert f(*none, 4, 4, 2, 10, float("nan"), None) == EINVAL
    assert f(*none, 4, 4, 2, BIG, 0.2, None) == ERANGE       # nnz H words
    assert f(*none, 4, 4, 1 << 30, 10, 0.2, None) == ERANGE
    assert f(*none, BIG // 2 + 1, 4, 2, 10, 0.2, None) == ERANGE   # M H words
    assert f(*none, 4, BIG // 2 + 1, 2, 10, 0.2, None) == ERANGE   # K H words
    assert f(*none, 0, 4, 2, 0, 0.2, None) == 0              # M == 0: nothing to do, pointers not looked at
    assert f(*none, 4, 4, 2, 10, 0.2, None) == EINVAL        # NULL where needed
    for bad in range(5):
        assert f(*[None if i == bad else _p(OK) for i in range(5)], 4, 4, 2, 10, 0.2, None) == EINVAL, bad
        assert f(*[_p(OK + 2) if i == bad else _p(OK) for i in range(5)], 4, 4, 2, 10, 0.2, None) == EALIGN, bad
    assert f(*ok[:4], _p(OK + 4), 4, 4, 2, 10, 0.2, None) == EALIGN   # stats holds 8-byte pairs
    # no entries: stats alone is looked at
    assert f(*none, 4, 4, 2, 0, 0.2, None) == EINVAL
    assert f(None, None, None, None, _p(OK + 2), 4, 4, 2, 0, 0.2, None) == EALIGN


def test_aggregate_return_codes(L):
    f = L.lib.gespmm_gat_aggregate_f32
    # (ptr, ind, el, er, stats, B, C, M, K, H, F, nnz, slope, transposed, stream)
    none = (None,) * 7
    for t in (0, 1):
        assert f(*none, 4, 4, 0, 8, 10, 0.2, t, None) == EINVAL        # H < 1
        assert f(*none, -1, 4, 2, 8, 10, 0.2, t, None) == EINVAL       # negative sizes
        assert f(*none, 4, 4, 2, -8, 10, 0.2, t, None) == EINVAL
        assert f(*none, 4, 4, 2, 8, -1, 0.2, t, None) == EINVAL
        assert f(*none, 4, 0, 2, 8, 10, 0.2, t, None) == EINVAL        # K < 1
        assert f(*none, 0, 4, 2, 8, 10, 0.2, t, None) == EINVAL        # entries without rows
        assert f(*none, 4, 4, 2, 8, 10, float("inf"), t, None) == EINVAL
        assert f(*none, 4, 4, 2, 8, BIG, 0.2, t, None) == ERANGE       # nnz H words
        assert f(*none, 4, 4, 8, 1 << 27, 10, 0.2, t, None) == ERANGE  # H F beyond the width of the other entries
        assert f(*none, 4, 4, 1 << 30, 4, 10, 0.2, t, None) == ERANGE
        assert f(*none, BIG // 2 + 1, 4, 2, 8, 10, 0.2, t, None) == ERANGE
        assert f(*none, 4, 4, 2, 0, 10, 0.2, t, None) == 0             # F == 0: nothing to do
        assert f(*none, 4, 4, 2, 8, 10, 0.2, t, None) == EINVAL        # NULL where needed
        for bad in range(7):
            assert f(*[None if i == bad else _p(OK) for i in range(7)], 4, 4, 2, 8, 10, 0.2, t, None) == EINVAL, (t, bad)
            assert f(*[_p(OK + 2) if i == bad else _p(OK) for i in range(7)], 4, 4, 2, 8, 10, 0.2, t, None) == EALIGN, (t, bad)
        assert f(*[_p(OK + 4) if i == 4 else _p(OK) for i in range(7)], 4, 4, 2, 8, 10, 0.2, t, None) == EALIGN  # stats: 8 bytes
        # no entries: C alone is looked at
        assert f(*none, 4, 4, 2, 8, 0, 0.2, t, None) == EINVAL
        assert f(*none[:6], _p(OK + 2), 4, 4, 2, 8, 0, 0.2, t, None) == EALIGN
    assert f(*none, 4, 4, 2, 8, 10, 0.2, 2, None) == EINVAL            # transposed is 0 or 1
    assert f(*none, 0, 4, 2, 8, 0, 0.2, 0, None) == 0                  # M == 0: no rows, nothing to write
    assert f(*(_p(3),) * 7, 0, 4, 2, 8, 0, 0.2, 0, None) == 0
    r = L.lib.gespmm_gat_aggregate_route
    assert r(4, 4, 0, 8, 10, 0, 16, 16, None) == EINVAL
    assert r(4, 4, 2, 8, -1, 0, 16, 16, None) == EINVAL
    assert r(4, 0, 2, 8, 10, 0, 16, 16, None) == EINVAL
    assert r(4, 4, 2, 8, 10, 3, 16, 16, None) == EINVAL
    assert r(4, 4, 2, 8, 10, 0, 0, 16, None) == EINVAL
    assert r(4, 4, 8, 1 << 27, 10, 1, 16, 16, None) == ERANGE


@pytest.mark.parametrize("M,K,nnz", ((21, 301, 1060), (19717, 19717, 88651), (1 << 18, 1 << 18, 3 << 20)))
def test_route_table(L, M, K, nnz, monkeypatch):
    monkeypatch.delenv("GESPMM_GAT_AGGREGATE_ROUTE", raising=False)
    for transposed in (False, True):
        S = K if transposed else M
        for H in range(1, 9):
            for F in ROUTE_F:
                N = H * F
                for align, vmax in ((16, 4), (8, 2), (4, 1)):
                    route, (V, S_, W, rpw) = L.gat_aggregate_route(M, K, H, F, nnz, transposed, align, align)
                    assert route == 1, (transposed, H, F, align)
                    assert V in (1, 2, 4) and V <= vmax and F % V == 0, (H, F, align, V)
                    assert S_ in (1, 2) and W in (4, 8, 16, 32, 64) and 1 <= rpw <= 32 and rpw % (64 // W) == 0, (H, F, V, S_, W, rpw)
                    assert W * V * S_ >= N or W == 64, (H, F, V, S_, W)
                    if H >= 2:  # the geometry IS the multi-head product's on the same segments (which has no kernel at H = 1)
                        assert L.heads_route(S, M if transposed else K, H, F, nnz, align, align) == (1, (V, S_, W, rpw)), (transposed, H, F)
        for H in (9, 12, 33):
            assert L.gat_aggregate_route(M, K, H, 8, nnz, transposed) == (0, (0, 0, 0, 0)), H
    # the pin is read per call
    assert L.gat_aggregate_route(M, K, 8, 8, nnz)[0] == 1
    monkeypatch.setenv("GESPMM_GAT_AGGREGATE_ROUTE", "composition")
    assert os.environ["GESPMM_GAT_AGGREGATE_ROUTE"] == "composition"
    for transposed in (False, True):
        for H in (1, 4, 8):
            assert L.gat_aggregate_route(M, K, H, 8, nnz, transposed) == (0, (0, 0, 0, 0)), H
    monkeypatch.delenv("GESPMM_GAT_AGGREGATE_ROUTE")
    assert L.gat_aggregate_route(M, K, 8, 8, nnz)[0] == 1


def test_route_needs_32_bit_offsets(L, monkeypatch):
    monkeypatch.delenv("GESPMM_GAT_AGGREGATE_ROUTE", raising=False)
    assert L.gat_aggregate_route(1000, (1 << 24) - 1, 8, 8, 5000)[0] == 1
    assert L.gat_aggregate_route(1000, 1 << 24, 8, 8, 5000)[0] == 0            # K H F 4 = 2^32: B is [K, H F]
    assert L.gat_aggregate_route(1000, 1 << 24, 8, 8, 5000, True)[0] == 1      # transposed: B is [M, H F]
    assert L.gat_aggregate_route(1 << 24, 1000, 8, 8, 5000, True)[0] == 0
    # nnz H < 2^31 never decides: the softmax's ladder has refused such sizes before (32-bit word positions of its own)
    assert L.gat_aggregate_route(1 << 20, 1000, 8, 8, (1 << 28) - 513)[0] == 1
    assert L.lib.gespmm_gat_aggregate_route(1 << 20, 1000, 8, 8, (1 << 28) - 512, 0, 16, 16, None) == ERANGE
