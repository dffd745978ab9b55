"""Fused GAT aggregation on 16-bit features, host side (no GPU): the route table of gespmm_gat_aggregate_x16_route and the return-code
ladders of gespmm_gat_aggregate_x16 / _dropout_x16 — the checks run before any device work, so NULL or made-up device pointers are
enough."""
import ctypes

import pytest

from test_heads_host import EALIGN, EINVAL, ERANGE

OK = 0x1000  # a made-up address: the checks look at the number only and return before anything could read it
BIG = (1 << 31) - 4096  # one past the largest count of 32-bit word positions
PIN = "GESPMM_GAT_AGGREGATE_ROUTE"
F16, BF16 = 1, 2


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    assert (_lib.X16_F16, _lib.X16_BF16) == (F16, BF16)
    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


# (M, K, H, F, transposed, b_align, c_align, nnz, pin) -> route
ROUTES = (
    ((300, 211, 1, 64, False, 16, 16, 1553, None), 1),   # H = 1 runs the kernel
    ((300, 211, 8, 8, True, 16, 16, 1553, None), 1),
    ((300, 211, 8, 2, False, 4, 4, 1553, None), 1),      # one word per head, 4-byte operands
    ((300, 211, 4, 160, False, 8, 16, 1553, None), 1),
    ((300, 211, 4, 3, False, 16, 16, 1553, None), 0),    # odd F
    ((300, 211, 1, 1, True, 16, 16, 1553, None), 0),
    ((300, 211, 9, 8, False, 16, 16, 1553, None), 0),    # H > 8
    ((300, 211, 8, 8, False, 2, 16, 1553, None), 0),     # 2-byte aligned B
    ((300, 211, 8, 8, True, 16, 2, 1553, None), 0),      # ... C
    ((300, 211, 8, 8, False, 16, 16, 1553, "composition"), 0),
    ((300, 211, 8, 8, False, 16, 16, 1553, "kernel"), 1),  # (any other value pins nothing)
    ((1000, (1 << 25) - 1, 8, 8, False, 16, 16, 5000, None), 1),
    ((1000, 1 << 25, 8, 8, False, 16, 16, 5000, None), 0),  # K H F 2 = 2^32: B is [K, H F] of 2-byte elements
    ((1000, 1 << 25, 8, 8, True, 16, 16, 5000, None), 1),   # transposed: B is [M, H F]
    ((1 << 25, 1000, 8, 8, True, 16, 16, 5000, None), 0),
    ((300, 211, 8, 8, False, 16, 16, 0, None), 1),
)


@pytest.mark.parametrize("case,want", ROUTES)
def test_route_table(L, monkeypatch, case, want):
    M, K, H, F, transposed, b_align, c_align, nnz, pin = case
    monkeypatch.delenv(PIN, raising=False)
    if pin:
        monkeypatch.setenv(PIN, pin)
    route, (V, S, W, rpw) = L.gat_aggregate_x16_route(M, K, H, F, nnz, transposed, b_align, c_align)
    assert route == want, (route, V, S, W, rpw)
    if route == 0:
        assert (V, S, W, rpw) == (0, 0, 0, 0)
        return
    # the geometry in 32-bit words: V words per lane and strip inside one head, no wider than the operands allow
    assert V in (1, 2, 4) and (F // 2) % V == 0 and 4 * V <= min(b_align, c_align), (V, S, W)
    assert S in (1, 2) and W in (4, 8, 16, 32, 64) and 1 <= rpw <= 32 and rpw % (64 // W) == 0, (V, S, W, rpw)
    assert W * V * S >= H * F // 2 or W == 64, (V, S, W)
    if H >= 2:  # ... and IS the 16-bit multi-head product's on the same segments (which has no kernel at H = 1)
        Sg, Kb = (K, M) if transposed else (M, K)
        assert L.heads_x16_route(Sg, Kb, H, F, nnz, b_align, c_align) == (1, (V, S, W, rpw))


def test_return_codes(L):
    # (ptr, ind, el, er, stats, B, C, dtype, M, K, H, F, nnz, slope, transposed[, p, seed], stream)
    plain = lambda a, *r: L.lib.gespmm_gat_aggregate_x16(*a, *r, None)  # noqa: E731
    drop = lambda a, *r: L.lib.gespmm_gat_aggregate_dropout_x16(*a, *r, 0.5, _p(OK), None)  # noqa: E731
    none, ok = (None,) * 7, (_p(OK),) * 7
    for f in (plain, drop):
        for t in (0, 1):
            for dt in (0, 3, -1):
                assert f(ok, dt, 4, 4, 2, 8, 10, 0.2, t) == EINVAL         # unknown dtype, before anything else
            for dt in (F16, BF16):
                assert f(none, dt, 4, 4, 0, 8, 10, 0.2, t) == EINVAL       # H < 1
                assert f(none, dt, -1, 4, 2, 8, 10, 0.2, t) == EINVAL      # negative sizes
                assert f(none, dt, 4, 4, 2, -8, 10, 0.2, t) == EINVAL
                assert f(none, dt, 4, 0, 2, 8, 10, 0.2, t) == EINVAL       # K < 1
                assert f(none, dt, 4, 4, 2, 8, 10, float("inf"), t) == EINVAL
                assert f(none, dt, 4, 4, 2, 8, BIG, 0.2, t) == ERANGE      # nnz H words
                assert f(none, dt, 4, 4, 8, 1 << 27, 10, 0.2, t) == ERANGE
                assert f(none, dt, 4, 4, 2, 0, 10, 0.2, t) == 0            # F == 0: nothing to do
                assert f(none, dt, 4, 4, 2, 8, 10, 0.2, t) == EINVAL       # NULL where needed
                for bad in range(7):
                    assert f([None if i == bad else _p(OK) for i in range(7)], dt, 4, 4, 2, 8, 10, 0.2, t) == EINVAL, (t, bad)
                    assert f([_p(OK + 1) if i == bad else _p(OK) for i in range(7)], dt, 4, 4, 2, 8, 10, 0.2, t) == EALIGN, (t, bad)
                for bad in range(5):  # the fp32 operands: 4 bytes (stats: 8); B and C may sit on any 2-byte boundary
                    assert f([_p(OK + 2) if i == bad else _p(OK) for i in range(7)], dt, 4, 4, 2, 8, 10, 0.2, t) == EALIGN, (t, bad)
                assert f([_p(OK + 4) if i == 4 else _p(OK) for i in range(7)], dt, 4, 4, 2, 8, 10, 0.2, t) == EALIGN
                # no entries: C alone is looked at
                assert f(none, dt, 4, 4, 2, 8, 0, 0.2, t) == EINVAL
                assert f(none[:6] + (_p(OK + 1),), dt, 4, 4, 2, 8, 0, 0.2, t) == EALIGN
        assert f(none, BF16, 4, 4, 2, 8, 10, 0.2, 2) == EINVAL             # transposed is 0 or 1
        assert f(none, BF16, 0, 4, 2, 8, 0, 0.2, 0) == 0                   # M == 0: no rows, nothing to write
    g = L.lib.gespmm_gat_aggregate_dropout_x16
    assert g(*ok, BF16, 4, 4, 2, 8, 10, 0.2, 0, 1.0, _p(OK), None) == EINVAL     # p outside [0, 1)
    assert g(*ok, BF16, 4, 4, 2, 8, 10, 0.2, 0, float("nan"), _p(OK), None) == EINVAL
    assert g(*ok, BF16, 4, 4, 2, 8, 10, 0.2, 0, 0.5, None, None) == EINVAL       # the seed is a pointer like the others
    assert g(*ok, BF16, 4, 4, 2, 8, 10, 0.2, 0, 0.5, _p(OK + 2), None) == EALIGN
    r = L.lib.gespmm_gat_aggregate_x16_route
    assert r(4, 4, 0, 8, 10, 0, 16, 16, None) == EINVAL
    assert r(4, 4, 2, 8, 10, 3, 16, 16, None) == EINVAL
    assert r(4, 4, 2, 8, 10, 0, 0, 16, None) == EINVAL
    assert r(4, 4, 8, 1 << 27, 10, 1, 16, 16, None) == ERANGE
