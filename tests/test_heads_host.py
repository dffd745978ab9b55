"""Multi-head product, host side (no GPU): exported symbols, the argument checks of gespmm_csr_spmm_heads_f32 — which run before any
device work, so NULL (or made-up) device pointers are enough — the route table of gespmm_heads_route, and the edge order that
graphs.transpose_csr returns for the backward product."""
import ctypes

import pytest
import torch

EINVAL, EALIGN, ERANGE = -1, -2, -3
ROUTE_F = (1, 2, 3, 4, 5, 8, 13, 16, 20, 27, 32, 64, 100, 160)


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_and_version(L):
    for name in ("gespmm_csr_spmm_heads_f32", "gespmm_plan_spmm_heads_f32", "gespmm_heads_route", "gespmm_plan_heads_route"):
        assert name in L.EXPORTS
        getattr(L.lib, name)
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


def test_argument_errors_before_any_device_work(L):
    f = L.lib.gespmm_csr_spmm_heads_f32
    # (rowptr, colind, val, B, C, M, K, H, F, nnz, stream)
    assert f(None, None, None, None, None, 4, 4, 0, 8, 10, None) == EINVAL   # H < 1
    assert f(None, None, None, None, None, 4, 4, -2, 8, 10, None) == EINVAL
    assert f(None, None, None, None, None, -1, 4, 2, 8, 10, None) == EINVAL  # negative sizes
    assert f(None, None, None, None, None, 4, -1, 2, 8, 10, None) == EINVAL
    assert f(None, None, None, None, None, 4, 4, 2, -8, 10, None) == EINVAL
    assert f(None, None, None, None, None, 4, 4, 2, 8, -1, None) == EINVAL
    assert f(None, None, None, None, None, 4, 4, 2, 8, 10, None) == EINVAL   # NULL where needed
    ok = 0x1000  # made-up addresses: the checks look at the numbers only and return before anything could read them
    assert f(_p(ok), _p(ok), None, _p(ok), _p(ok), 4, 4, 2, 8, 10, None) == EINVAL   # val is needed when there are entries
    assert f(_p(ok), _p(ok), _p(ok), None, _p(ok), 4, 4, 2, 8, 10, None) == EINVAL   # ... and B
    assert f(_p(ok), _p(ok), _p(ok), _p(ok), None, 4, 4, 2, 8, 10, None) == EINVAL   # C always
    for bad in range(5):  # each pointer in turn two bytes off
        ptrs = [_p(ok + 2 if i == bad else ok) for i in range(5)]
        assert f(*ptrs, 4, 4, 2, 8, 10, None) == EALIGN, bad
    assert f(None, None, None, None, None, 4, 4, 8, 1 << 27, 10, None) == ERANGE       # H F beyond the width of the other entries
    assert f(None, None, None, None, None, 4, 4, 1 << 30, 4, 10, None) == ERANGE
    assert f(None, None, None, None, None, 4, 4, 2, 8, (1 << 31) - 4095, None) == ERANGE  # nnz beyond theirs
    # nothing to do: 0 without looking at pointers
    assert f(None, None, None, None, None, 0, 4, 2, 8, 10, None) == 0
    assert f(None, None, None, None, None, 4, 4, 2, 0, 10, None) == 0
    assert f(_p(3), _p(3), _p(3), _p(3), _p(3), 0, 4, 2, 8, 10, None) == 0
    # the plan entries refuse a NULL plan
    assert L.lib.gespmm_plan_spmm_heads_f32(None, None, None, None, 2, 8, None) == EINVAL
    assert L.lib.gespmm_plan_heads_route(None, 2, 8, 16, 16) == EINVAL
    # the route query: same size checks
    assert L.lib.gespmm_heads_route(4, 4, 0, 8, 10, 16, 16, None) == EINVAL
    assert L.lib.gespmm_heads_route(4, 4, 2, 8, -1, 16, 16, None) == EINVAL
    assert L.lib.gespmm_heads_route(4, 4, 8, 1 << 27, 10, 16, 16, None) == ERANGE


@pytest.mark.parametrize("M,K,nnz", ((21, 301, 1060), (19717, 19717, 88651), (1 << 18, 1 << 18, 3 << 20)))
def test_route_table(L, M, K, nnz):
    for H in range(2, 9):
        for F in ROUTE_F:
            N = H * F
            for align, vmax in ((16, 4), (8, 2), (4, 1)):
                route, (V, S, W, rpw) = L.heads_route(M, K, H, F, nnz, align, align)
                assert route == 1, (H, F, align)
                assert V in (1, 2, 4) and V <= vmax and F % V == 0, (H, F, align, V)
                assert S in (1, 2) and W in (4, 8, 16, 32, 64) and 1 <= rpw <= 32 and rpw % (64 // W) == 0, (H, F, V, S, W, rpw)
                # one column tile covers the width, or the width is cut into full-size tiles (then every lane is in use: W = 64)
                assert W * V * S >= N or W == 64, (H, F, V, S, W)
                if W * V * S >= N and W > 4:
                    assert (W // 2) * V * S < N, ("a narrower group would do", H, F, V, S, W)
    for H in (1, 9, 12, 16):
        assert L.heads_route(M, K, H, 8, nnz) == (0, (0, 0, 0, 0)), H


def test_route_needs_32_bit_offsets(L):
    assert L.heads_route(1000, (1 << 24) - 1, 8, 8, 5000)[0] == 1
    assert L.heads_route(1000, 1 << 24, 8, 8, 5000)[0] == 0          # K H F 4 = 2^32
    assert L.heads_route(1 << 20, 1000, 8, 8, (1 << 28) - 1)[0] == 1
    assert L.heads_route(1 << 20, 1000, 8, 8, 1 << 28)[0] == 0       # nnz H = 2^31
    assert L.heads_route(1 << 20, 1000, 4, 8, 1 << 29)[0] == 0


def test_transpose_order_is_stable_with_repeated_edges(pkg):
    from gespmm_amd import graphs

    # 5 x 4 pattern, unsorted columns, edge (1, 2) three times and (3, 0) twice
    rowptr = torch.tensor([0, 2, 6, 6, 9, 10], dtype=torch.int32)
    colind = torch.tensor([3, 0, 2, 2, 1, 2, 0, 3, 0, 2], dtype=torch.int32)
    rows = torch.repeat_interleave(torch.arange(5), torch.diff(rowptr).long())
    colptr, rowind, order = graphs.transpose_csr(rowptr, colind, K=4, return_order=True)
    assert order.dtype == torch.int64 and order.numel() == 10 and sorted(order.tolist()) == list(range(10))
    c = colind[order].long()
    assert bool((c[1:] >= c[:-1]).all())
    assert torch.equal(rowind, rows[order].to(torch.int32))
    assert colptr.tolist() == [0, 3, 4, 8, 10]
    # rows ascending inside a column, repeated edges in their CSR order
    key = c * 5 + rows[order]
    same = key[1:] == key[:-1]
    assert bool((key[1:] >= key[:-1]).all()) and int(same.sum()) == 3
    assert bool((order[1:][same] > order[:-1][same]).all())
    assert torch.equal(order, graphs.transpose_csr(rowptr, colind, K=4, return_order=True)[2])
    # the default call is what it was, with values too
    val = torch.arange(10, dtype=torch.float32)
    assert len(graphs.transpose_csr(rowptr, colind, K=4)) == 2
    cp2, ri2, v2 = graphs.transpose_csr(rowptr, colind, K=4, val=val)
    assert torch.equal(cp2, colptr) and torch.equal(ri2, rowind) and torch.equal(v2, val[order])
    assert len(graphs.transpose_csr(rowptr, colind, K=4, val=val, return_order=True)) == 4
