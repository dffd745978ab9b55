"""Fused add-softmax and the edge segment sum, host side only (no GPU): the three new symbols, their return codes before any device
work, and a numpy restatement ``lane_sum`` of the pinned summation order of grad_el / gespmm_edge_segment_sum_f32 — fp32 lane chains
from +0 over the entries lo + l + t W, the xor butterfly W/2 .. 1, W = 64 past L — held against float64 within the bound the GPU tests
use, per (segment, head), u = 2^-24:

    |sum - ref| <= u (ceil(d / W') + log2 W' + 1) sum_p |x_p|,      W' = W for d <= L, 64 beyond

A lane chain of T = ceil(d / W') terms makes T - 1 roundings, the butterfly log2 W' more; (1 + u)^(T - 1 + log2 W') - 1 stays below
u (T + log2 W' + 1) for every chain here (T <= 512). The bound is tight on purpose: one dropped term of typical size exceeds it, which
``test_bound_notices_a_dropped_term`` checks.

``lane_sum``, ``sum_bound`` and ``csc_of`` are shared with tests/test_gpu_gat_softmax.py."""
import ctypes

import numpy as np
import pytest

from helpers import edge_case_csr
from test_edge_softmax_host import WANT_L, _butterfly, _lane_view, hub_degrees, rowptr_of, want_W

EINVAL, EALIGN, ERANGE = -1, -2, -3
MAX_NNZ = 0x7FFFFFFF - 4096
NEW = ("gespmm_gat_softmax_f32", "gespmm_gat_softmax_backward_f32", "gespmm_edge_segment_sum_f32")
F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24


# ----------------------------------------------------------------------------------- the pinned order, restated lane by lane in fp32

def lane_sum(ptr, x, W, L=WANT_L, order=None):
    """out[s, h] = sum of x[order[p], h] over p in [ptr[s], ptr[s + 1]) the way the kernel adds: lane l of W (64 for a segment of more
    than L entries) adds its entries lo + l + t W in entry order, plain fp32 adds from +0 (a position past the end adds +0), then the
    xor butterfly. Empty segments are +0."""
    x = np.asarray(x, dtype=F32)
    x2 = x.reshape(x.shape[0], -1)
    S = len(ptr) - 1
    out = np.zeros((S, x2.shape[1]), dtype=F32)
    for s in range(S):
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        if hi <= lo:
            continue
        w = W if hi - lo <= L else 64
        v = x2[lo:hi] if order is None else x2[np.asarray(order[lo:hi], dtype=np.int64)]
        vl = _lane_view(v, w, 0.0)
        acc = np.zeros(vl.shape[1:], dtype=F32)
        for t in range(vl.shape[0]):
            acc = (acc + vl[t]).astype(F32)
        out[s] = _butterfly(acc, w, lambda a, b: (a + b).astype(F32))[0]
    return out if x.ndim == 2 else out[:, 0]


def sum_bound(ptr, x, W, L=WANT_L, order=None):
    """-> (ref, bound): the float64 sum per (segment, head) and u (ceil(d / W') + log2 W' + 1) sum |x_p|."""
    x2 = np.asarray(x, dtype=F32).astype(F64)
    x2 = x2.reshape(x2.shape[0], -1)
    if order is not None:
        x2 = x2[np.asarray(order, dtype=np.int64)]
    S = len(ptr) - 1
    ref = np.zeros((S, x2.shape[1]), dtype=F64)
    bound = np.zeros_like(ref)
    for s in range(S):
        lo, hi = int(ptr[s]), int(ptr[s + 1])
        d = hi - lo
        if d <= 0:
            continue
        w = W if d <= L else 64
        ref[s] = x2[lo:hi].sum(axis=0)
        bound[s] = U24 * (-(-d // w) + int(np.log2(w)) + 1) * np.abs(x2[lo:hi]).sum(axis=0)
    return ref, bound


def csc_of(rowptr, colind, K):
    """(colptr, order) of a CSR pattern on the host: CSC position i holds CSR entry order[i], rows ascending inside a column (stable) —
    what graphs.transpose_csr(.., return_order=True) answers."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    M = rowptr.size - 1
    rows = np.repeat(np.arange(M), np.diff(rowptr))
    order = np.argsort(np.asarray(colind, dtype=np.int64) * M + rows, kind="stable")
    colptr = np.zeros(K + 1, dtype=np.int32)
    colptr[1:] = np.cumsum(np.bincount(colind, minlength=K))
    return colptr, order.astype(np.int32)


def worst_sum_ratio(got, ref, bound):
    """max |got - ref| / bound where the bound is positive; where it is zero (empty segments, all-zero terms) got must equal ref."""
    got = np.asarray(got, dtype=F64).reshape(ref.shape)
    err = np.abs(got - ref)
    zero = bound == 0
    assert np.all(err[zero] == 0), "a sum of no terms (or of zeros) must be exact"
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# --------------------------------------------------------------------------------------------------------------------- tests

def test_symbols_version_and_names(pkg):
    import os
    import re

    import gespmm_amd
    from gespmm_amd import _lib, softmax

    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "gespmm.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(_lib.lib, name) is not None, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.lib.gespmm_version().decode().startswith("gespmm 0.5 ")
    assert "GATSoftmaxFunction" in gespmm_amd.__all__ and gespmm_amd.GATSoftmaxFunction is gespmm_amd.op.GATSoftmaxFunction
    for name in ("gat_edge_softmax", "gat_edge_softmax_backward", "edge_segment_sum"):
        assert callable(getattr(softmax, name)), name
    conv = gespmm_amd.GATConv(4, 2, heads=2)
    assert conv.fused_score is False and gespmm_amd.GATConv(4, 2, heads=2, fused_score=True).fused_score is True


def test_return_codes_need_no_gpu(pkg):
    """Sizes that make no sense, range, nnz == 0, NULL, alignment — in that order, all before any device work."""
    from gespmm_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    half = ctypes.c_void_p(p.value + 2)
    made_up = ctypes.c_void_p(0x1000)
    nan, inf = float("nan"), float("inf")

    def fwd(rp, ci, el, er, o, M, K, H, nnz, slope=1.0):
        return lib.gespmm_gat_softmax_f32(rp, ci, el, er, o, M, K, H, nnz, slope, None)

    def bwd(rp, ci, a, g, el, er, gs, gel, M, K, H, nnz, slope=1.0):
        return lib.gespmm_gat_softmax_backward_f32(rp, ci, a, g, el, er, gs, gel, M, K, H, nnz, slope, None)

    def seg(ptr, order, x, o, S, H, nnz):
        return lib.gespmm_edge_segment_sum_f32(ptr, order, x, o, S, H, nnz, None)

    # sizes that make no sense — whatever the pointers are, and before sizes that are too large
    for M, K, H, nnz, slope in ((4, 5, 0, 8, 1.0), (4, 5, -1, 8, 1.0), (-1, 5, 2, 8, 1.0), (4, 5, 2, -8, 1.0), (4, 5, 2, 8, nan),
                                (4, 5, 2, 8, inf), (4, 5, 2, 8, -inf), (0, 5, 2, 8, 1.0), (4, 0, 2, 8, 1.0), (4, -3, 2, 8, 0.2),
                                (4, 0, 2, 0, 1.0), (1 << 31, 0, 2, 8, 1.0), (4, 0, 2, MAX_NNZ + 1, 1.0), (1 << 31, 5, 2, 8, nan)):
        assert fwd(p, p, p, p, p, M, K, H, nnz, slope) == EINVAL, (M, K, H, nnz, slope)
        assert fwd(None, half, None, None, half, M, K, H, nnz, slope) == EINVAL
        assert bwd(p, p, p, p, p, p, p, p, M, K, H, nnz, slope) == EINVAL, (M, K, H, nnz, slope)
        assert bwd(None, half, None, None, None, None, half, None, M, K, H, nnz, slope) == EINVAL
    for S, H, nnz in ((4, 0, 8), (4, -1, 8), (-1, 2, 8), (4, 2, -8), (0, 2, 8), (4, 0, MAX_NNZ + 1)):
        assert seg(p, p, p, p, S, H, nnz) == EINVAL and seg(None, half, None, half, S, H, nnz) == EINVAL, (S, H, nnz)
    # range: the softmax's own limits, and the words of the dense operands — M H, K H, S H
    for M, K, H, nnz in ((1 << 31, 5, 2, 8), (MAX_NNZ + 1, 5, 1, 8), (4, 5, 1, MAX_NNZ + 1), (4, 5, 2, MAX_NNZ // 2 + 1), (4, 5, 1 << 31, 1),
                         (4, 5, 3, 1 << 40), (MAX_NNZ // 2 + 1, 5, 2, 8), (4, MAX_NNZ // 2 + 1, 2, 8), (4, 1 << 40, 1, 8),
                         (4, MAX_NNZ + 1, 1, 0)):
        assert fwd(None, p, p, p, p, M, K, H, nnz) == ERANGE, (M, K, H, nnz)
        assert bwd(None, p, p, p, p, p, p, p, M, K, H, nnz, 0.2) == ERANGE, (M, K, H, nnz)
    for S, H, nnz in ((1 << 31, 2, 8), (MAX_NNZ + 1, 1, 8), (4, 1, MAX_NNZ + 1), (4, 2, MAX_NNZ // 2 + 1), (4, 1 << 31, 1),
                      (MAX_NNZ // 2 + 1, 2, 8), (MAX_NNZ // 3 + 1, 3, 0)):
        assert seg(None, p, p, p, S, H, nnz) == ERANGE, (S, H, nnz)
    # at the limits the sizes pass: the NULL is seen
    assert fwd(None, p, p, p, p, MAX_NNZ // 2, MAX_NNZ // 2, 2, MAX_NNZ // 2) == EINVAL
    assert bwd(None, p, p, p, p, p, p, p, MAX_NNZ, MAX_NNZ, 1, 8, 0.2) == EINVAL
    assert seg(None, p, p, p, MAX_NNZ // 2, 2, 8) == EINVAL
    # no entries: the forward answers 0 without looking at pointers; the backward and the segment sum still owe their dense result its
    # zeros, so they look at that one pointer (and at nothing else) — unless there is no row either
    assert fwd(half, made_up, None, half, None, 4, 5, 3, 0) == 0 and fwd(None, None, None, None, None, 0, 1, 3, 0) == 0
    assert bwd(None, None, None, None, None, None, None, None, 0, 1, 1, 0) == 0 and seg(None, None, None, None, 0, 2, 0) == 0
    assert bwd(half, half, None, None, half, None, None, None, 4, 5, 3, 0, 0.2) == EINVAL
    assert bwd(half, half, None, None, half, None, None, half, 4, 5, 3, 0, 0.2) == EALIGN
    assert seg(half, half, None, None, 4, 3, 0) == EINVAL and seg(half, half, None, half, 4, 3, 0) == EALIGN
    # NULL, then alignment
    for bad in range(5):
        args = [p] * 5
        args[bad] = None
        assert fwd(*args, 4, 5, 3, 8) == EINVAL, bad
        args[bad] = half
        assert fwd(*args, 4, 5, 3, 8, 0.2) == EALIGN, bad
        args[(bad + 1) % 5] = None  # NULL is reported before a misaligned pointer
        assert fwd(*args, 4, 5, 3, 8) == EINVAL, bad
    for slope in (1.0, 0.2):
        # (rowptr, colind, alpha, grad_alpha, el, er, grad_score, grad_el): colind, el, er count only with a slope
        needed = (0, 2, 3, 6, 7) if slope == 1.0 else tuple(range(8))
        for bad in needed:
            args = [p] * 8
            args[bad] = None
            assert bwd(*args, 4, 5, 3, 8, slope) == EINVAL, (slope, bad)
            args[bad] = half
            assert bwd(*args, 4, 5, 3, 8, slope) == EALIGN, (slope, bad)
            args[needed[(needed.index(bad) + 1) % len(needed)]] = None
            assert bwd(*args, 4, 5, 3, 8, slope) == EINVAL, (slope, bad)
    for bad in (0, 2, 3):  # (ptr, order, x, out): order may be NULL, but not misaligned
        args = [p] * 4
        args[bad] = None
        assert seg(*args, 4, 3, 8) == EINVAL, bad
        args[bad] = half
        assert seg(*args, 4, 3, 8) == EALIGN, bad
    assert seg(p, half, p, p, 4, 3, 8) == EALIGN
    assert seg(None, half, p, p, 4, 3, 8) == EINVAL


def _values(oracle, nnz, H, seed):
    return (F32(4.0) * oracle.hash_val(nnz * H, seed=seed)).reshape(nnz, H)


def test_lane_sum_within_bound_edge_cases(oracle):
    """The edge-case pattern at its own W = 16, and its transpose (301 columns, W = 4) through the CSC order."""
    G = edge_case_csr()
    rp, nnz = G["rowptr"], G["nnz"]
    assert want_W(G["M"], nnz) == 16 and want_W(G["K"], nnz) == 4
    colptr, order = csc_of(rp, G["colind"], G["K"])
    assert int(colptr[-1]) == nnz and np.array_equal(np.sort(order), np.arange(nnz))
    assert np.array_equal(np.diff(colptr), np.bincount(G["colind"], minlength=G["K"])) and (np.diff(colptr) == 0).any()
    worst = 0.0
    for H in (1, 3, 8):
        x = _values(oracle, nnz, H, seed=41 + H)
        ref, bound = sum_bound(rp, x, 16)
        got = lane_sum(rp, x, 16)
        assert np.all(got[np.diff(rp) == 0] == 0) and not np.signbit(got[np.diff(rp) == 0]).any()
        worst = max(worst, worst_sum_ratio(got, ref, bound))
        ref, bound = sum_bound(colptr, x, 4, order=order)
        got = lane_sum(colptr, x, 4, order=order)
        assert np.all(got[np.diff(colptr) == 0] == 0)
        worst = max(worst, worst_sum_ratio(got, ref, bound))
        # the column sums are the sums over the entries with that column, whatever the order inside a column
        want = np.zeros((G["K"], H), dtype=F64)
        np.add.at(want, G["colind"], x.astype(F64))
        assert np.allclose(ref, want, rtol=0, atol=1e-9)
    print("worst error / bound %.3f" % worst)
    assert worst <= 1.0


def test_lane_sum_within_bound_long_rows(oracle):
    """Rows of L - 1, L, L + 1 and 3 L + 7 entries at W = 16 (11 rows) and W = 4: 64 lanes past L."""
    rp = rowptr_of(hub_degrees(WANT_L))
    nnz = int(rp[-1])
    assert want_W(rp.size - 1, nnz) == 16
    worst = 0.0
    for W, H in ((16, 1), (16, 3), (4, 2)):
        x = _values(oracle, nnz, H, seed=51 + H)
        ref, bound = sum_bound(rp, x, W)
        worst = max(worst, worst_sum_ratio(lane_sum(rp, x, W), ref, bound))
        one = lane_sum(rp, x[:, 0].copy(), W)
        assert one.shape == (rp.size - 1,) and np.array_equal(one.view(np.uint32), lane_sum(rp, x, W)[:, 0].view(np.uint32))
    print("worst error / bound %.3f" % worst)
    assert worst <= 1.0


def test_bound_notices_a_dropped_term(oracle):
    """The bound is tight enough to be a test: leave out one term of typical size (at least the mean |x| of its segment) from every
    segment of two or more entries and the sum leaves the bound."""
    G = edge_case_csr()
    rp, nnz = G["rowptr"], G["nnz"]
    x = _values(oracle, nnz, 1, seed=61)
    ref, bound = sum_bound(rp, x, 16)
    for s in range(G["M"]):
        lo, hi = int(rp[s]), int(rp[s + 1])
        if hi - lo < 2:
            continue
        k = lo + int(np.argmax(np.abs(x[lo:hi, 0])))
        y = x.copy()
        y[k] = 0
        got = lane_sum(rp, y, 16)
        assert abs(float(got[s, 0]) - ref[s, 0]) > bound[s, 0], s


def test_lane_order_is_the_documented_one():
    """Where the order shows: 2^24 + 1 + 1 keeps the ones only if they meet each other before they meet 2^24."""
    big = 2.0 ** 24
    rp = rowptr_of([4, 0, 8])
    x = np.array([big, 1, 0, 1, 1, 2, 3, 4, 5, 6, 7, 8], dtype=F32)
    got = lane_sum(rp, x, 4)  # lanes 0 .. 3 hold 2^24, 1, 0, 1; the butterfly adds lanes (0, 2) and (1, 3), then the two halves
    assert got[0] == F32(big + 2) and got[1] == 0 and not np.signbit(got[1]) and got[2] == 36
    swapped = np.array([0, 1, 3, 2] + list(range(4, 12)))
    assert lane_sum(rp, x, 4, order=swapped)[0] == F32(big)  # lanes hold 2^24, 1, 1, 0: each 1 meets 2^24 alone and is rounded away
    x1 = np.array([big, 0, 0, 0, 1, 0, 0, 0, 1], dtype=F32)  # entries 0, 4, 8: one lane's chain at W = 4
    assert lane_sum(rowptr_of([9]), x1, 4)[0] == F32(big)
    with pytest.raises(IndexError):
        lane_sum(rowptr_of([2]), np.ones(2, dtype=F32), 4, order=np.array([0, 2]))
