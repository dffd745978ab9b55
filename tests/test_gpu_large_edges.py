"""Every edge-sized op once on ONE pattern past 2^26 edges — where 32-bit position arithmetic and grid sizes start to matter and
where no other test goes (the largest pattern elsewhere has 4.5 M edges).

The pattern is tests/band.py's band, M = 2^20 + 16 rows of d = 64 entries: nnz = 2^26 + 1024. Its CSC arrays and the CSR -> CSC edge
order are closed forms, built with elementwise ops, one cumsum and two repeat_interleave — no gather or scatter by an edge-sized
index — and then verified through what a transpose is (band.verify_csc). Weights and features are small integers of the edge / node
number, so every fp32 sum is exact and a result must EQUAL an int64 reference that involves no index array (test_gpu_fullsize.py's
idiom). References are evaluated on a fixed list of windows of 4096 consecutive rows / columns — the first, the last, the ones holding
position nnz - 2^26 in CSR and in CSC order, and fourteen spread evenly — and every word of every window is compared.

What this pins: on torch 2.10.0+rocm7.0, ``x[order]`` and ``torch.index_select`` with 16-byte rows (fp32
[nnz, 4], bf16 [nnz, 8]) and more than 2^26 index rows leave rows ``nnz - 2^26 ..`` of their result unwritten; ``graphs.take_edges``
gathers in pieces below that size. With ``take_edges`` replaced by plain indexing, test_take_edges_every_row_past_2_26[4-float32]
and [8-bfloat16] fail from row 1024 = nnz - 2^26 on, and all cases of test_multi_head_spmm_function / test_multi_head_sddmm_function
fail in grad_feat / grad_k at column 77, the column that holds CSC position 1024.

Section f runs the edge-sized ops again at H = 17 — arrays of 1.14e9 words, between 2^30 and 2^31 — and take_edges at 64-byte rows.

The max reducer runs in both directions and both widths of element (section d): the forward, the op that PRODUCES positions past 2^26,
in fp32 and bf16, and the backward on a closed-form argmax in fp32 and bf16.

On the MI355X the module takes about 9.3 s for 54 tests (8.4 s for 51 before the three max-reducer cases were added; the fixture 1 s, no
test above 1.3 s) and peaks at 19.3 GiB of device memory (section f: four arrays of 4.5 GB; 7.8 GB without it)."""
import numpy as np
import pytest
import torch

import band

pytestmark = pytest.mark.gpu

M_BIG, D = (1 << 20) + 16, 64
M_CONTROL = (1 << 20) - 16
DEV = "cuda"


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _poison(shape, dtype=torch.float32):
    """For results an op allocates itself: the caching allocator hands the block just freed to the next request of the same size, so
    the op's result starts as NaN and a word nobody writes does not compare equal."""
    block = _nan(shape, dtype)
    del block


class Band:
    def __init__(self, M, d):
        self.M, self.d = M, d
        self.nnz, self.K = band.sizes(M, d)
        self.rowptr, self.colind = band.csr(M, d, DEV)
        self.colptr, self.rowind, self.order64 = band.csc(M, d, DEV)
        band.verify_csc(M, d, self.colptr, self.order64)
        self.order32 = self.order64.to(torch.int32)
        self.wrap = self.nnz - (1 << 26)  # the first position a 2^32-thread wrap leaves unwritten (negative: none)
        marked_rows, marked_cols = (), ()
        if self.wrap >= 0:
            marked_rows = (self.wrap // d,)
            marked_cols = (int(torch.searchsorted(self.colptr.long(), torch.tensor([self.wrap], device=DEV), right=True)) - 1,)
        self.row_windows = [(s, min(s + band.WINDOW, M)) for s in band.window_starts(M, marked_rows)]
        self.col_windows = [(s, min(s + band.WINDOW, self.K)) for s in band.window_starts(self.K, marked_cols)]

    def weights(self, H, dtype=torch.float32, fn=band.w_of):
        return band.edge_values(torch.arange(self.nnz, device=DEV), H, dtype, fn)

    def weights_csc(self, H, dtype=torch.float32, fn=band.w_of):
        """the same weights in CSC order, as a closed form of csc_order: no gather"""
        return band.edge_values(self.order64, H, dtype, fn)


@pytest.fixture(scope="module")
def big(pkg):
    g = Band(M_BIG, D)
    assert g.nnz == (1 << 26) + 1024 and g.wrap == 1024
    assert len(g.row_windows) >= 14 and len(g.col_windows) >= 14
    assert g.row_windows[0][0] == 0 and g.row_windows[-1][1] == g.M and g.col_windows[0][0] == 0 and g.col_windows[-1][1] == g.K
    yield g
    del g
    torch.cuda.empty_cache()


def _as_result(ref, dtype):
    """The int64 reference as the kernel must return it: exact in fp32; ONE rounding of the exact fp32 sum for a 16-bit result."""
    return ref.to(torch.float32).to(dtype)


def _check_windows(what, got, windows, ref_fn, scale=1, dtype=None):
    """Every word of every window of ``got`` (segments along dim 0, ``scale`` entries of dim 0 per segment) against ref_fn(s0, s1)."""
    dtype = got.dtype if dtype is None else dtype
    for s0, s1 in windows:
        want = _as_result(ref_fn(s0, s1), dtype)
        part = got[s0 * scale:s1 * scale]
        assert part.shape == want.shape, (what, part.shape, want.shape)
        diff = band.first_difference(part, want)
        if diff is not None:
            idx, g, w = diff
            pytest.fail("%s: window [%d, %d): first difference at (segment %d%s) = %r, expected %r" % (
                what, s0, s1, s0 + idx[0] // scale, "".join(", %d" % i for i in ((idx[0] % scale,) if scale > 1 else ()) + idx[1:]), g, w))


def _check_rows(what, got, want, wrap):
    """Every row of two edge arrays; names the first differing row (and where the 2^32-thread wrap would begin)."""
    bits = {4: torch.int32, 2: torch.int16}[got.element_size()]
    ne = got.view(bits) != want.view(bits)
    bad = ne if ne.dim() == 1 else ne.any(1)
    n = int(bad.sum())
    if n:
        first = int(torch.nonzero(bad)[0])
        pytest.fail("%s: %d of %d rows differ, the first is row %d (nnz - 2^26 = %d): got %s, expected %s" % (
            what, n, bad.numel(), first, wrap, got[first].flatten().tolist(), want[first].flatten().tolist()))


# ---- a. the gather --------------------------------------------------------------------------------------------------------------------

def _take_edges_case(g, H, dtype):
    from gespmm_amd import graphs

    shape = (g.nnz,) if H == 0 else (g.nnz, H)
    for order in (g.order64, g.order32):
        w = g.weights(max(H, 1), dtype).reshape(shape)
        _poison(shape, dtype)
        got = graphs.take_edges(w, order)
        del w  # (the closed form of the result is built after the input is gone: the peak stays at two arrays)
        assert got.is_contiguous() and got.dtype == dtype and got.shape == shape
        _check_rows("take_edges(w[%d, %d] %s, %s order)" % (g.nnz, H, dtype, order.dtype), got, g.weights_csc(max(H, 1), dtype).reshape(shape),
                    g.wrap)
        del got


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("float32", "bfloat16"))
@pytest.mark.parametrize("H", (1, 2, 4, 8))
def test_take_edges_every_row_past_2_26(big, H, dtype):
    _take_edges_case(big, H, dtype)


def test_take_edges_one_dimensional_past_2_26(big):
    _take_edges_case(big, 0, torch.float32)


def test_take_edges_control_below_2_26(pkg):
    """The one control: the same at M = 2^20 - 16 (nnz = 2^26 - 1024), below the size at which plain indexing goes wrong."""
    g = Band(M_CONTROL, D)
    assert g.nnz == (1 << 26) - 1024
    for H in (1, 2, 4, 8):
        for dtype in (torch.float32, torch.bfloat16):
            _take_edges_case(g, H, dtype)


# ---- b. the multi-head products on closed-form weights (no gather anywhere) -----------------------------------------------------------

@pytest.mark.parametrize("x16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("F", (2, 16))
@pytest.mark.parametrize("H", (2, 4, 8))
def test_heads_products_on_csc_and_csr_arrays(big, H, F, x16):
    from gespmm_amd import _lib, spmm

    g = big
    dtype = torch.bfloat16 if x16 else torch.float32
    route = _lib.heads_x16_route if x16 else _lib.heads_route
    fn = spmm.csr_spmm_heads_x16 if x16 else spmm.csr_spmm_heads
    # A^T: the CSC arrays, the weights in CSC order, a dense operand of M rows
    assert route(g.K, g.M, H, F, g.nnz)[0] == 1, "the heads kernel must answer"
    w = g.weights_csc(H)
    dense = band.node_values(g.M, H, F, DEV, dtype, band.k_of)
    out = fn(g.colptr, g.rowind, w, dense, out=_nan((g.K, H, F), dtype))
    _check_windows("heads product on the CSC arrays H=%d F=%d %s" % (H, F, dtype), out, g.col_windows,
                   lambda c0, c1: band.ref_csc_product(g.M, g.d, c0, c1, H, F, DEV, dense_fn=band.k_of))
    del w, dense, out
    # A: the CSR arrays
    assert route(g.M, g.K, H, F, g.nnz)[0] == 1, "the heads kernel must answer"
    w = g.weights(H)
    dense = band.node_values(g.K, H, F, DEV, dtype)
    out = fn(g.rowptr, g.colind, w, dense, out=_nan((g.M, H, F), dtype))
    _check_windows("heads product on the CSR arrays H=%d F=%d %s" % (H, F, dtype), out, g.row_windows,
                   lambda r0, r1: band.ref_csr_product(g.M, g.d, r0, r1, H, F, DEV))


# ---- c. what users call: the autograd functions, forward and backward ------------------------------------------------------------------

@pytest.mark.parametrize("heads_sddmm", (False, True), ids=("per-head-sddmm", "heads-sddmm"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("float32", "bfloat16"))
def test_multi_head_spmm_function(big, dtype, heads_sddmm):
    import gespmm_amd

    g, H, F = big, 4, 8
    feat = band.node_values(g.K, H, F, DEV, dtype).requires_grad_(True)
    weight = g.weights(H).requires_grad_(True)
    grad_out = band.node_values(g.M, H, F, DEV, dtype, band.k_of)
    _poison((g.M, H, F), dtype)
    out = gespmm_amd.MultiHeadSPMMFunction.apply(g.rowptr, g.colind, g.colptr, g.rowind, g.order64, feat, weight, None, heads_sddmm)
    _poison((g.nnz, H))
    out.backward(grad_out)
    assert out.dtype == dtype and feat.grad.dtype == dtype and weight.grad.dtype == torch.float32
    _check_windows("MultiHeadSPMMFunction forward %s" % dtype, out.detach(), g.row_windows,
                   lambda r0, r1: band.ref_csr_product(g.M, g.d, r0, r1, H, F, DEV))
    _check_windows("MultiHeadSPMMFunction grad_feat %s" % dtype, feat.grad, g.col_windows,
                   lambda c0, c1: band.ref_csc_product(g.M, g.d, c0, c1, H, F, DEV, dense_fn=band.k_of))
    _check_windows("MultiHeadSPMMFunction grad_weight %s" % dtype, weight.grad, g.row_windows,
                   lambda r0, r1: band.ref_csr_scores(g.M, g.d, r0, r1, H, F, DEV, q_fn=band.k_of, k_fn=band.b_of), scale=g.d)


@pytest.mark.parametrize("order_dtype", (torch.int64, torch.int32), ids=("int64-order", "int32-order"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("float32", "bfloat16"))
def test_multi_head_sddmm_function(big, dtype, order_dtype):
    import gespmm_amd

    g, H, F = big, 4, 8
    q = band.node_values(g.M, H, F, DEV, dtype).requires_grad_(True)
    k = band.node_values(g.K, H, F, DEV, dtype, band.k_of).requires_grad_(True)
    grad_s = g.weights(H)
    order = g.order64 if order_dtype == torch.int64 else g.order32
    _poison((g.nnz, H))
    s = gespmm_amd.MultiHeadSDDMMFunction.apply(g.rowptr, g.colind, g.colptr, g.rowind, order, q, k)
    _poison((g.nnz, H))
    s.backward(grad_s)
    assert s.dtype == torch.float32 and q.grad.dtype == dtype and k.grad.dtype == dtype
    _check_windows("MultiHeadSDDMMFunction forward %s" % dtype, s.detach(), g.row_windows,
                   lambda r0, r1: band.ref_csr_scores(g.M, g.d, r0, r1, H, F, DEV), scale=g.d)
    _check_windows("MultiHeadSDDMMFunction grad_q %s" % dtype, q.grad, g.row_windows,
                   lambda r0, r1: band.ref_csr_product(g.M, g.d, r0, r1, H, F, DEV, dense_fn=band.k_of))
    _check_windows("MultiHeadSDDMMFunction grad_k %s" % dtype, k.grad, g.col_windows,
                   lambda c0, c1: band.ref_csc_product(g.M, g.d, c0, c1, H, F, DEV, dense_fn=band.b_of))


# ---- d. the other ops that take the CSC arrays or an order: integer inputs, exact ------------------------------------------------------

@pytest.mark.parametrize("x16", (False, True), ids=("f32", "bf16"))
def test_sddmm_heads_csr_and_coo(big, x16):
    _sddmm_heads_case(big, 4, 8, x16, big.row_windows)


def _sddmm_heads_case(g, H, F, x16, row_windows):
    from gespmm_amd import _lib, sddmm

    dtype = torch.bfloat16 if x16 else torch.float32
    assert _lib.describe_sddmm_heads(True, g.M, g.nnz, H, F, x16=x16)["route"] == "kernel"
    assert _lib.describe_sddmm_heads(False, g.M, g.nnz, H, F, x16=x16)["route"] == "kernel"
    q = band.node_values(g.M, H, F, DEV, dtype)
    k = band.node_values(g.K, H, F, DEV, dtype, band.k_of)
    csr_fn, coo_fn = (sddmm.csr_sddmm_heads_x16, sddmm.coo_sddmm_heads_x16) if x16 else (sddmm.csr_sddmm_heads, sddmm.coo_sddmm_heads)

    def ref(r0, r1):
        return band.ref_csr_scores(g.M, g.d, r0, r1, H, F, DEV)

    s = csr_fn(g.rowptr, g.colind, q, k, out=_nan((g.nnz, H)))
    _check_windows("csr_sddmm_heads %s" % dtype, s, row_windows, ref, scale=g.d)
    rows = torch.div(torch.arange(g.nnz, device=DEV, dtype=torch.int32), g.d, rounding_mode="floor")
    s2 = coo_fn(rows, g.colind, q, k, out=_nan((g.nnz, H)))
    _check_windows("coo_sddmm_heads %s" % dtype, s2, row_windows, ref, scale=g.d)
    assert torch.equal(s, s2), "the two forms agree in every word"
    del s, s2
    # the COO form on the CSC order of the same edges: (rowind, column of the position) — the score array in CSC order
    cols = torch.repeat_interleave(torch.arange(g.K, device=DEV, dtype=torch.int32), (g.colptr[1:] - g.colptr[:-1]).long(),
                                   output_size=g.nnz)
    s3 = coo_fn(g.rowind, cols, q, k, out=_nan((g.nnz, H)))
    # position i holds CSR entry order[i] = r d + j: its score is <q(r), k(r + o_j)> — elementwise on order, every row
    r = torch.div(g.order64, g.d, rounding_mode="floor")
    c = r + band.offset_of(g.order64 % g.d)
    want = torch.zeros((g.nnz, H), dtype=torch.float32, device=DEV)
    for h in range(H):
        acc = torch.zeros(g.nnz, dtype=torch.int64, device=DEV)
        for f in range(F):
            acc += band.b_of(r, h, f) * band.k_of(c, h, f)
        want[:, h] = acc
    _check_rows("coo_sddmm_heads in CSC order %s" % dtype, s3, want, g.wrap)


def test_edge_segment_sum_over_columns(big):
    _edge_segment_sum_case(big, 4, big.row_windows, big.col_windows)


def _edge_segment_sum_case(g, H, row_windows, col_windows):
    from gespmm_amd import softmax

    x = g.weights(H)
    out = softmax.edge_segment_sum(g.colptr, x, order=g.order32, out=_nan((g.K, H)))
    one = lambda r, h, f: 1  # noqa: E731
    _check_windows("edge_segment_sum(colptr, w, order)", out.view(g.K, H, 1), col_windows,
                   lambda c0, c1: band.ref_csc_product(g.M, g.d, c0, c1, H, 1, DEV, dense_fn=one))
    x1 = x[:, 0].contiguous()
    out1 = softmax.edge_segment_sum(g.colptr, x1, order=g.order32, out=_nan((g.K,)))
    _check_windows("edge_segment_sum(colptr, w[nnz], order)", out1.view(g.K, 1, 1), col_windows,
                   lambda c0, c1: band.ref_csc_product(g.M, g.d, c0, c1, 1, 1, DEV, dense_fn=one))
    # rows: no order, segments are the CSR rows
    outr = softmax.edge_segment_sum(g.rowptr, x, out=_nan((g.M, H)))
    _check_windows("edge_segment_sum(rowptr, w)", outr.view(g.M, H, 1), row_windows,
                   lambda r0, r1: band.ref_csr_product(g.M, g.d, r0, r1, H, 1, DEV, dense_fn=one))


def test_gat_aggregate_with_dyadic_alpha(big):
    """er = 0 makes the d = 64 scores of a row equal, so alpha = exp(0) / 64 = 2^-6 in every entry whatever el holds: the statistics
    are exact (m = leaky_relu(el), s = 64) and the aggregation is an integer sum scaled by a power of two — exact in fp32."""
    from gespmm_amd import _lib, softmax, spmm

    g, H, F, slope = big, 4, 8, 0.25
    el = band.node_values(g.M, H, 1, DEV, fn=band.b_of).view(g.M, H).contiguous() * 0.5
    er = torch.zeros((g.K, H), device=DEV)
    stats = softmax.gat_softmax_stats(g.rowptr, g.colind, el, er, negative_slope=slope, out=_nan((g.M, H, 2)))
    assert torch.equal(stats[:, :, 0], torch.where(el > 0, el, el * slope)) and bool((stats[:, :, 1] == 64.0).all())
    one = lambda e, h: 1  # noqa: E731
    assert _lib.gat_aggregate_route(g.M, g.K, H, F, g.nnz, transposed=True)[0] == 1
    grad_out = band.node_values(g.M, H, F, DEV, fn=band.k_of)
    out_t = spmm.gat_aggregate(g.colptr, g.rowind, el, er, stats, grad_out, negative_slope=slope, transposed=True,
                               out=_nan((g.K, H, F)))
    _check_windows("gat_aggregate(transposed=True)", out_t * 64.0, g.col_windows,
                   lambda c0, c1: band.ref_csc_product(g.M, g.d, c0, c1, H, F, DEV, dense_fn=band.k_of, weight_fn=one))
    assert _lib.gat_aggregate_route(g.M, g.K, H, F, g.nnz, transposed=False)[0] == 1
    feat = band.node_values(g.K, H, F, DEV)
    out = spmm.gat_aggregate(g.rowptr, g.colind, el, er, stats, feat, negative_slope=slope, out=_nan((g.M, H, F)))
    _check_windows("gat_aggregate", out * 64.0, g.row_windows,
                   lambda r0, r1: band.ref_csr_product(g.M, g.d, r0, r1, H, F, DEV, weight_fn=one))


MAX_DTYPES, MAX_IDS = (torch.float32, torch.bfloat16), ("float32", "bfloat16")


@pytest.mark.parametrize("dtype", MAX_DTYPES, ids=MAX_IDS)
def test_max_backward_on_a_closed_form_argmax(big, dtype):
    """arg[r, n] = r d + ((r + n) mod d): row r's word n was won by its entry j = (r + n) mod d. Column k then receives grad_out[r, n]
    from every row r = k - o_j with (r + n) mod d == j. bfloat16: grad_out narrowed (integers in -3 .. 3) through
    csr_spmm_max_backward_x16; a sum is an integer of at most 64 x 3 in magnitude, exact in bf16; the reference is the same int64 form."""
    from gespmm_amd import spmm

    g, N = big, 4
    r = torch.arange(g.M, device=DEV, dtype=torch.int64).view(-1, 1)
    n = torch.arange(N, device=DEV, dtype=torch.int64).view(1, -1)
    arg = (r * g.d + (r + n) % g.d).to(torch.int32)
    grad_fn = lambda r, n: (r + 3 * n) % 7 - 3  # noqa: E731
    grad_out = grad_fn(r, n).to(torch.float32)
    if dtype == torch.float32:
        out = spmm.csr_spmm_max_backward(g.colptr, g.rowind, g.order32, arg, grad_out, g.K, out=_nan((g.K, N)))
    else:
        out = spmm.csr_spmm_max_backward_x16(g.colptr, g.rowind, g.order32, arg, grad_out.to(dtype), g.K, out=_nan((g.K, N), dtype))
    assert out.dtype == dtype and g.d * 3 <= 256

    def ref(c0, c1):
        c = torch.arange(c0, c1, device=DEV, dtype=torch.int64).view(-1, 1, 1)
        j = torch.arange(g.d, device=DEV, dtype=torch.int64).view(1, -1, 1)
        nn = n.view(1, 1, -1)
        rr = c - band.offset_of(j)
        hit = (rr >= 0) & (rr < g.M) & ((rr + nn) % g.d == j)
        return (hit.to(torch.int64) * grad_fn(rr, nn)).sum(1)

    _check_windows("csr_spmm_max_backward %s" % dtype, out, g.col_windows, ref)


@pytest.mark.parametrize("dtype", MAX_DTYPES, ids=MAX_IDS)
def test_max_arg_forward_past_2_26(big, dtype):
    """The forward is the op that PRODUCES positions past 2^26: N = 4, B = band.node_values (integers in -3 .. 3, exact in bf16:
    tests/test_large_edges_host.py), every row window against the closed form — the largest of the row's d = 64 band entries and
    arg = r d + the first j that reaches it (seven values over 64 entries: ties in every word, the first-position rule decides)."""
    from gespmm_amd import spmm

    g, N = big, 4
    B = band.node_values(g.K, 1, N, DEV, dtype).view(g.K, N)
    out, arg = _nan((g.M, N), dtype), torch.full((g.M, N), -7, dtype=torch.int32, device=DEV)
    fn = spmm.csr_spmm_max_arg if dtype == torch.float32 else spmm.csr_spmm_max_arg_x16
    got = fn(g.rowptr, g.colind, B, out=out, arg=arg)
    assert got[0] is out and got[1] is arg and out.dtype == dtype
    _all_written(out=out)
    assert int(arg.min()) >= 0 and int(arg.max()) > (1 << 26)
    assert any(s0 * g.d <= g.wrap < s1 * g.d for s0, s1 in g.row_windows), "the window holding position nnz - 2^26 is compared"
    j = torch.arange(g.d, device=DEV, dtype=torch.int64).view(1, -1, 1)
    f = torch.arange(N, device=DEV, dtype=torch.int64).view(1, 1, -1)
    for r0, r1 in g.row_windows:
        r = torch.arange(r0, r1, device=DEV, dtype=torch.int64).view(-1, 1, 1)
        vals = band.b_of(r + band.offset_of(j), 0, f)
        top = vals.max(1, keepdim=True).values
        first = torch.where(vals == top, j, g.d).min(1).values
        assert torch.equal(out[r0:r1].float(), top.view(-1, N).to(torch.float32)), "max, rows %d .. %d" % (r0, r1)
        assert torch.equal(arg[r0:r1].long(), r.view(-1, 1) * g.d + first), "arg, rows %d .. %d" % (r0, r1)


def test_transpose_csr_with_values(big):
    """The library's own transpose (argsort, bincount, take_edges) against the closed-form CSC arrays, in every entry."""
    from gespmm_amd import graphs

    g, H = big, 4
    w = g.weights(H)
    colptr, rowind, w_csc, order = graphs.transpose_csr(g.rowptr, g.colind, g.K, val=w, return_order=True)
    assert torch.equal(colptr, g.colptr)
    _check_rows("transpose_csr rowind", rowind, g.rowind, g.wrap)
    assert order.dtype == torch.int64 and torch.equal(order, g.order64)
    del colptr, rowind, order, w
    _check_rows("transpose_csr values", w_csc, g.weights_csc(H), g.wrap)


# ---- e. the float ops: random fp32 inputs, the float64 references and tolerances of their own GPU tests, on sub-patterns -----------------
# A sub-pattern is FLOAT_ROWS consecutive rows with ALL their entries, columns rebased to the first one they touch: row-wise results
# (softmax, scores, row gradients) are compared on every row of it, column-wise results (grad_er, grad_xr, grad_k, grad_v) on the
# columns ALL of whose entries lie in these rows. One sub-pattern per window of the fixed list (the first rows of the window; the
# LAST rows of the last one, so the final edges are in), every one asserted. The host references run in numpy: 4096-row windows
# would cost them seconds per test, 512 rows keep the same positions at a tenth of that.

FLOAT_ROWS = 512
DROPOUT_SEED = (0x12345678, 0x9ABCDEF0)


class Sub:
    def __init__(self, g, r0, r1):
        from test_dot_attention_host import transpose

        n, last = r1 - r0, band.offset_of(g.d - 1)
        self.r0, self.r1, self.e0, self.e1 = r0, r1, r0 * g.d, r1 * g.d
        self.c0, self.c1 = r0, min(r1 + last, g.K)  # the columns these rows touch
        self.M, self.K, self.nnz = n, self.c1 - self.c0, n * g.d
        self.rowptr = (np.arange(n + 1) * g.d).astype(np.int32)
        self.colind = (g.colind[self.e0:self.e1].cpu().numpy() - self.c0).astype(np.int32)
        self.rows = np.repeat(np.arange(n, dtype=np.int32), g.d)
        self.degs = np.full(n, g.d)
        self.colptr, self.rowind, self.order = transpose(self.rowptr, self.colind, self.K)
        # global columns whose rows c - o_j all lie in [r0, r1): from r0 + o_last (from 0 at the top) to r1 (to K at the bottom)
        self.f0, self.f1 = (0 if r0 == 0 else r0 + last), (g.K if r1 == g.M else r1)
        assert self.f1 - self.f0 >= n - last
        self.full = slice(self.f0 - self.c0, self.f1 - self.c0)  # ... in the sub-pattern's numbering
        want = np.diff(g.colptr[self.f0:self.f1 + 1].cpu().numpy())
        assert np.array_equal(np.diff(self.colptr)[self.full], want), "these columns are complete in the sub-pattern"
        self.P = {"M": self.M, "K": self.K, "nnz": self.nnz, "rowptr": self.rowptr, "colind": self.colind, "colptr": self.colptr,
                  "rowind": self.rowind, "order": self.order, "rows": self.rows, "degs": self.degs}

    def edges(self, t):
        return t[self.e0:self.e1].cpu().numpy()

    def row_nodes(self, t):
        return t[self.r0:self.r1].cpu().numpy()

    def col_nodes(self, t):
        return t[self.c0:self.c1].cpu().numpy()

    def full_cols(self, t):
        return t[self.f0:self.f1].cpu().numpy()

    def full_ptr(self):
        """(ptr, order) of the complete columns alone: segments over the sub-pattern's CSR entries"""
        p = self.colptr[self.full.start:self.full.stop + 1].astype(np.int64)
        return (p - p[0]), self.order[p[0]:p[-1]]


@pytest.fixture(scope="module")
def subs(big):
    out = [Sub(big, s0, s0 + FLOAT_ROWS) if s1 < big.M else Sub(big, big.M - FLOAT_ROWS, big.M) for s0, s1 in big.row_windows]
    assert out[0].r0 == 0 and out[0].e0 <= big.wrap < out[0].e1 and out[-1].e1 == big.nnz and out[-1].f1 == big.K and len(out) >= 14
    return out


def _rand(gen, shape, lo, hi):
    return torch.rand(shape, generator=gen, device=DEV) * (hi - lo) + lo


def _gen(seed):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return gen


def _all_written(**results):
    for name, t in results.items():
        assert not bool(torch.isnan(t).any()), "a word of %s was not written" % name


@pytest.mark.parametrize("slope", (None, 0.2))
def test_edge_softmax_forward_and_backward(big, subs, slope):
    _edge_softmax_case(big, subs, 4, slope)


def _edge_softmax_case(g, subs, H, slope):
    from gespmm_amd import softmax
    from test_edge_softmax_host import ref_backward, ref_forward, worst_ratio

    gen = _gen(11)
    score, grad = _rand(gen, (g.nnz, H), -16, 16), _rand(gen, (g.nnz, H), -2, 2)
    alpha = softmax.edge_softmax(g.rowptr, score, out=_nan((g.nnz, H)), negative_slope=slope)
    gs = softmax.edge_softmax_backward(g.rowptr, alpha, grad, score=score if slope is not None else None, negative_slope=slope,
                                       out=_nan((g.nnz, H)))
    _all_written(alpha=alpha, grad_score=gs)
    worst = [0.0, 0.0]
    for s in subs:
        sh, ah = s.edges(score), s.edges(alpha)
        a, tol = ref_forward(s.rowptr, sh, slope)
        gref, gtol = ref_backward(s.rowptr, ah, s.edges(grad), sh, slope)
        rf, rb = worst_ratio(ah, a, tol), worst_ratio(s.edges(gs), gref, gtol)
        worst = [max(worst[0], rf), max(worst[1], rb)]
        assert rf <= 1.0 and rb <= 1.0, ("rows %d .. %d" % (s.r0, s.r1), slope, rf, rb)
    print("edge_softmax H=%d slope=%s: worst error / tolerance forward %.3f backward %.3f" % (H, slope, *worst))


def test_gat_softmax_forward_and_backward(big, subs):
    _gat_softmax_case(big, subs, 4)


def _gat_softmax_case(g, subs, H):
    from gespmm_amd import _lib, softmax
    from test_edge_softmax_host import WANT_L, ref_backward, ref_forward, worst_ratio
    from test_gat_softmax_host import lane_sum, sum_bound, worst_sum_ratio

    slope, gen = 0.2, _gen(12)
    assert g.d <= WANT_L
    W_row, W_col = (_lib.describe_edge_softmax(n, g.nnz, H)["W"] for n in (g.M, g.K))
    el, er, grad = _rand(gen, (g.M, H), -16, 16), _rand(gen, (g.K, H), -16, 16), _rand(gen, (g.nnz, H), -2, 2)
    alpha = softmax.gat_edge_softmax(g.rowptr, g.colind, el, er, negative_slope=slope, out=_nan((g.nnz, H)))
    stats = softmax.gat_softmax_stats(g.rowptr, g.colind, el, er, negative_slope=slope, out=_nan((g.M, H, 2)))
    _poison((g.nnz, H))
    gs, gel = softmax.gat_edge_softmax_backward(g.rowptr, g.colind, alpha, grad, el=el, er=er, negative_slope=slope)
    ger = softmax.edge_segment_sum(g.colptr, gs, order=g.order32, out=_nan((g.K, H)))
    _all_written(alpha=alpha, grad_score=gs, grad_el=gel, grad_er=ger, stats=stats)
    worst = {}
    for s in subs:
        sh = s.row_nodes(el)[s.rows] + s.col_nodes(er)[s.colind]  # fl(el + er): one fp32 add, the contract's score
        assert sh.dtype == np.float32
        # the statistics: m the row's largest leaky score on its bits, s = sum exp(x - m) >= 1 whose quotient IS alpha's
        lk = np.where(sh >= 0, sh, sh * np.float32(slope)).astype(np.float32).reshape(s.M, g.d, H)
        st = s.row_nodes(stats)
        assert np.array_equal(st[..., 0].view(np.uint32), lk.max(1).view(np.uint32)) and bool((st[..., 1] >= 1.0).all()), "stats rows %d .." % s.r0
        ah, gsh = s.edges(alpha), s.edges(gs)
        a, tol = ref_forward(s.rowptr, sh, slope)
        gref, gtol = ref_backward(s.rowptr, ah, s.edges(grad), sh, slope)
        r = {"alpha": worst_ratio(ah, a, tol), "grad_score": worst_ratio(gsh, gref, gtol)}
        ptr_c, order_c = s.full_ptr()
        for name, got, ptr, W, order in (("grad_el", s.row_nodes(gel), s.rowptr, W_row, None), ("grad_er", s.full_cols(ger), ptr_c, W_col, order_c)):
            want = lane_sum(ptr, gsh, W, order=order)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s rows %d .. %d: not the pinned order's bits" % (name, s.r0, s.r1)
            ref, bound = sum_bound(ptr, gsh, W, order=order)
            r[name] = worst_sum_ratio(got, ref, bound)
        assert max(r.values()) <= 1.0, ("rows %d .. %d" % (s.r0, s.r1), r)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print("gat softmax H=%d: worst error / tolerance %s" % (H, worst))


def test_gatv2_score_forward_and_both_backward_passes(big, subs):
    _gatv2_case(big, subs, 4, 8)


def _gatv2_case(g, subs, H, F):
    from gespmm_amd import sddmm
    from test_gatv2_host import restate_backward, restate_score, worst_ratio

    slope, gen = 0.2, _gen(13)
    xl, xr = _rand(gen, (g.M, H, F), -1, 1), _rand(gen, (g.K, H, F), -1, 1)
    att, gsc = _rand(gen, (H, F), -2, 2), _rand(gen, (g.nnz, H), -2, 2)
    score = sddmm.gatv2_score(g.rowptr, g.colind, xl, xr, att, negative_slope=slope, out=_nan((g.nnz, H)))
    gxl, part = sddmm.gatv2_score_backward(g.rowptr, g.colind, gsc, xl, xr, att, negative_slope=slope, want_att_part=True,
                                           out=(_nan((g.M, H, F)), _nan((g.M, H, F))))
    gxr = sddmm.gatv2_score_backward(g.colptr, g.rowind, gsc, xr, xl, att, negative_slope=slope, order=g.order32, out=_nan((g.K, H, F)))
    _all_written(score=score, grad_xl=gxl, att_part=part, grad_xr=gxr)
    att_h, worst = att.cpu().numpy(), {}
    for s in subs:
        xl_h, xr_h, gs_h = s.row_nodes(xl), s.col_nodes(xr), s.edges(gsc)
        ref, terms = restate_score(s.rowptr, s.colind, xl_h, xr_h, att_h, slope)
        row = restate_backward(s.rowptr, s.colind, gs_h, xl_h, xr_h, att_h, slope)
        col = restate_backward(s.colptr, s.rowind, gs_h, xr_h, xl_h, att_h, slope, order=s.order)
        r = {"score": worst_ratio(s.edges(score), ref, terms, "score"), "grad_xl": worst_ratio(s.row_nodes(gxl), row[0], row[2], "grad_xl"),
             "att_part": worst_ratio(s.row_nodes(part), row[1], row[3], "att_part"),
             "grad_xr": worst_ratio(s.full_cols(gxr), col[0][s.full], col[2][s.full], "grad_xr")}
        assert max(r.values()) <= 1.0, ("rows %d .. %d" % (s.r0, s.r1), r)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print("gatv2 H=%d F=%d: worst error / bound %s" % (H, F, worst))


def test_dot_attention_three_launches(big, subs):
    from gespmm_amd import attention
    from test_dot_attention_host import ratio, ref_backward, ref_forward

    g, H, F, gen = big, 4, 8, _gen(14)
    q, k, v = _rand(gen, (g.M, H, F), -1, 1), _rand(gen, (g.K, H, F), -1, 1), _rand(gen, (g.K, H, F), -1, 1)
    go = _rand(gen, (g.M, H, F), 0.5, 1)
    scale = float(np.float32(1.0 / np.sqrt(F)))
    out, gq, gk, gv = _nan((g.M, H, F)), _nan((g.M, H, F)), _nan((g.K, H, F)), _nan((g.K, H, F))
    stats, delta = _nan((g.M, H, 2)), _nan((g.M, H))
    attention.dot_attention(g.rowptr, g.colind, q, k, v, scale=scale, out=out, stats=stats)
    attention.dot_attention_backward_q(g.rowptr, g.colind, q, k, v, stats, out, go, scale=scale, results=(delta, gq))
    attention.dot_attention_backward_kv(g.colptr, g.rowind, q, k, v, stats, delta, go, scale=scale, results=(gk, gv))
    _all_written(out=out, stats=stats, delta=delta, grad_q=gq, grad_k=gk, grad_v=gv)
    worst = {}
    for s in subs:
        x = {"q": s.row_nodes(q), "k": s.col_nodes(k), "v": s.col_nodes(v), "go": s.row_nodes(go), "scale": scale}
        st, o, dl = s.row_nodes(stats), s.row_nodes(out), s.row_nodes(delta)
        f = ref_forward(s.P, x)
        b = ref_backward(s.P, x, st, o, None)
        bc = ref_backward(s.P, x, st, o, dl)
        r = {"out": ratio(o, f["out"], f["tol_out"]), "m": ratio(st[..., 0], f["m"], f["tol_m"]), "l": ratio(st[..., 1], f["l"], f["tol_l"]),
             "delta": ratio(dl, b["delta"], b["tol_delta"]), "grad_q": ratio(s.row_nodes(gq), b["grad_q"], b["tol_grad_q"]),
             "grad_k": ratio(s.full_cols(gk), bc["grad_k"][s.full], bc["tol_grad_k"][s.full]),
             "grad_v": ratio(s.full_cols(gv), bc["grad_v"][s.full], bc["tol_grad_v"][s.full])}
        assert max(r.values()) <= 1.0, ("rows %d .. %d" % (s.r0, s.r1), r)
        worst = {k_: max(v_, worst.get(k_, 0.0)) for k_, v_ in r.items()}
    print("dot attention: worst error / tolerance %s" % worst)


def test_edge_dropout_mask(big, subs):
    _edge_dropout_case(big, subs, 4)


def _edge_dropout_case(g, subs, H):
    from gespmm_amd import _lib, softmax
    from test_edge_dropout_host import restate

    p, gen = 0.3, _gen(15)
    x = _rand(gen, (g.nnz, H), -2, 2)
    seed = torch.from_numpy(np.array(DROPOUT_SEED, dtype=np.uint32).view(np.int32)).to(DEV)
    y = softmax.edge_dropout(g.rowptr, g.colind, x, p, seed, out=_nan((g.nnz, H)))
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    # everywhere: a word is +0 or its input scaled, and the kept share is 1 - p
    dropped = y.view(torch.int32) == 0
    assert bool((dropped | (y == x * float(scale))).all())
    assert abs(float(dropped.float().mean()) - p) < 1e-3
    del dropped
    threshold = np.uint32(_lib.edge_dropout_threshold(p))
    assert subs[-1].nnz >= 4096 and subs[-1].e1 == g.nnz, "the last 4096 edges are in"
    for s in subs:
        bits = restate(DROPOUT_SEED[0], DROPOUT_SEED[1], (s.rows.astype(np.uint64) + s.r0)[:, None],
                       (s.colind.astype(np.uint64) + s.c0)[:, None], np.arange(H, dtype=np.uint64)[None, :])
        keep = bits >= threshold
        assert 0 < keep.sum() < keep.size
        want = np.where(keep, s.edges(x) * scale, np.float32(0.0)).astype(np.float32)
        got = s.edges(y)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "rows %d .. %d: %d words differ from the restated mask" % (
            s.r0, s.r1, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


# ---- f. the same edge-sized arrays past 2^30 WORDS: H = 17 on the same pattern is 1.14e9 words, 4.5 GB an array -------------------------
# Every kernel above forms the word position e H + h of an [nnz, H] array in 32 bits; at H = 4 and 8 it stays below 2^30, so a position
# that is turned into a 32-bit BYTE offset somewhere has never wrapped. The windows gain the one that holds edge floor(2^30 / H) — word
# 2^30 lies inside its row of the array — in CSR order and, for the column-wise results, in CSC order. References, sub-patterns and
# tolerances are those of the H = 4 cases.

H_WIDE = 17


class Wide:
    """The windows and sub-patterns of ``big`` with the mark of an H-wide edge array added."""

    def __init__(self, g, H):
        self.H, self.edge = H, (1 << 30) // H
        assert self.edge < g.nnz and (1 << 30) < g.nnz * H <= (1 << 31) - 1 - 4096
        col = int(torch.searchsorted(g.colptr.long(), torch.tensor([self.edge], device=DEV), right=True)) - 1
        self.row_windows = [(s, min(s + band.WINDOW, g.M)) for s in band.window_starts(g.M, (g.wrap // g.d, self.edge // g.d))]
        self.col_windows = [(s, min(s + band.WINDOW, g.K)) for s in band.window_starts(g.K, (col, self.edge // g.d))]
        assert any(s0 * g.d <= self.edge < s1 * g.d for s0, s1 in self.row_windows)
        self.subs = []
        for s0, s1 in self.row_windows:
            r0 = g.M - FLOAT_ROWS if s1 == g.M else (self.edge // g.d - FLOAT_ROWS // 2 if s0 <= self.edge // g.d < s1 and s0 > 0 else s0)
            self.subs.append(Sub(g, r0, r0 + FLOAT_ROWS))
        assert self.subs[0].r0 == 0 and self.subs[-1].e1 == g.nnz and any(s.e0 <= self.edge < s.e1 for s in self.subs)


@pytest.fixture(scope="module")
def wide(big):
    return Wide(big, H_WIDE)


@pytest.mark.parametrize("slope", (None, 0.2))
def test_edge_softmax_past_2_30_words(big, wide, slope):
    _edge_softmax_case(big, wide.subs, H_WIDE, slope)


def test_gat_softmax_with_stats_past_2_30_words(big, wide):
    _gat_softmax_case(big, wide.subs, H_WIDE)


def test_edge_dropout_mask_past_2_30_words(big, wide):
    _edge_dropout_case(big, wide.subs, H_WIDE)


def test_edge_segment_sum_past_2_30_words(big, wide):
    _edge_segment_sum_case(big, H_WIDE, wide.row_windows, wide.col_windows)


def test_gatv2_score_past_2_30_words(big, wide):
    _gatv2_case(big, wide.subs, H_WIDE, 2)


@pytest.mark.parametrize("x16", (False, True), ids=("f32", "bf16"))
def test_sddmm_heads_past_2_30_words(big, wide, x16):
    _sddmm_heads_case(big, H_WIDE, 2, x16, wide.row_windows)


def test_take_edges_64_byte_rows_past_2_30_words(big):
    """H = 16: 64-byte rows, the widest the HIP gather serves, 2^30 + 16384 words."""
    assert big.nnz * 16 == (1 << 30) + 16384
    _take_edges_case(big, 16, torch.float32)
