"""Host checks behind test_gpu_large_edges.py: the band pattern's closed forms (tests/band.py) against a numpy stable-argsort
transpose and a dense float64 product at a size where both are cheap, and ``graphs.take_edges`` — the chunked gather every permuted
edge array goes through — against plain indexing on CPU tensors, bit for bit, with the chunk forced down to 1, 7 and len - 1."""
import numpy as np
import pytest
import torch

import band

M_SMALL = 1000


def _numpy_transpose(M, d):
    rowptr, colind = (t.numpy() for t in band.csr(M, d))
    nnz, K = band.sizes(M, d)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(rowptr.astype(np.int64)))
    order = np.argsort(colind.astype(np.int64) * M + rows, kind="stable")
    colptr = np.zeros(K + 1, dtype=np.int64)
    colptr[1:] = np.cumsum(np.bincount(colind, minlength=K))
    return rowptr, colind, rows, colptr, rows[order], order


@pytest.mark.parametrize("d", (1, 7, 64))
def test_band_closed_forms_equal_a_numpy_transpose(d):
    M = M_SMALL
    nnz, K = band.sizes(M, d)
    rowptr, colind, rows, colptr_np, rowind_np, order_np = _numpy_transpose(M, d)
    assert nnz == M * d == colind.size and rowptr[-1] == nnz and K == colind.max() + 1
    o = np.array([band.offset_of(j) for j in range(d)])
    assert np.all(np.diff(o) > 0), "offsets strictly increasing"
    assert np.array_equal(colind, (np.arange(M)[:, None] + o[None, :]).reshape(-1))
    colptr, rowind, order = band.csc(M, d)
    assert colptr.dtype == torch.int32 and rowind.dtype == torch.int32 and order.dtype == torch.int64
    assert np.array_equal(band.in_degree(M, d).numpy(), np.diff(colptr_np))
    assert np.array_equal(colptr.numpy(), colptr_np)
    assert np.array_equal(rowind.numpy(), rowind_np)
    assert np.array_equal(order.numpy(), order_np)
    band.verify_csc(M, d, colptr, order)


def test_verify_csc_rejects_a_wrong_order():
    M, d = M_SMALL, 7
    colptr, _, order = band.csc(M, d)
    swapped = order.clone()
    swapped[[100, 101]] = order[[101, 100]]
    with pytest.raises(AssertionError):
        band.verify_csc(M, d, colptr, swapped)
    repeated = order.clone()
    repeated[500] = order[499]
    with pytest.raises(AssertionError):
        band.verify_csc(M, d, colptr, repeated)
    shifted = colptr.clone()
    shifted[10] += 1
    with pytest.raises(AssertionError):
        band.verify_csc(M, d, shifted, order)


@pytest.mark.parametrize("d", (1, 7, 64))
def test_reference_formulas_equal_a_dense_float64_product(d):
    M, H, F = M_SMALL, 3, 5
    nnz, K = band.sizes(M, d)
    _, colind, rows, colptr_np, rowind_np, order_np = _numpy_transpose(M, d)
    w = band.edge_values(torch.arange(nnz), H, dtype=torch.float64).numpy()
    assert w.min() == -2 and w.max() == 2
    w_csc = band.edge_values(torch.from_numpy(order_np), H, dtype=torch.float64).numpy()
    assert np.array_equal(w_csc, w[order_np]), "the closed-form permuted weights are the gathered ones"
    bK = band.node_values(K, H, F, dtype=torch.float64).numpy()
    kK = band.node_values(K, H, F, dtype=torch.float64, fn=band.k_of).numpy()
    kM = kK[:M]
    assert bK.min() == -3 and bK.max() == 3 and kK.min() == -2 and kK.max() == 2
    A = np.zeros((H, M, K))
    for h in range(H):
        A[h, rows, colind] = w[:, h]
    fwd = np.einsum("hmk,khf->mhf", A, bK)
    bwd = np.einsum("hmk,mhf->khf", A, kM)
    got_fwd = band.ref_csr_product(M, d, 0, M, H, F).numpy()
    got_bwd = band.ref_csc_product(M, d, 0, K, H, F, dense_fn=band.k_of).numpy()
    assert np.array_equal(got_fwd, fwd.astype(np.int64)) and np.array_equal(fwd, np.rint(fwd))
    assert np.array_equal(got_bwd, bwd.astype(np.int64))
    # a window in the middle is the slice of the whole
    assert np.array_equal(band.ref_csc_product(M, d, 300, 417, H, F, dense_fn=band.k_of).numpy(), got_bwd[300:417])
    assert np.array_equal(band.ref_csr_product(M, d, 300, 417, H, F).numpy(), got_fwd[300:417])
    scores = np.einsum("ehf,ehf->eh", bK[:M][rows], kK[colind])
    assert np.array_equal(band.ref_csr_scores(M, d, 0, M, H, F).numpy(), scores.astype(np.int64))
    assert np.array_equal(band.ref_csr_scores(M, d, 300, 417, H, F).numpy(), scores[300 * d:417 * d].astype(np.int64))
    # every partial sum of the GPU tests' shapes (d = 64, F <= 16) stays far below 2^24: fp32 sums are exact
    assert 64 * 2 * 3 < (1 << 24) and 16 * 3 * 2 < (1 << 24)


def test_window_starts_cover_first_last_and_marked():
    n = (1 << 20) + 16
    starts = band.window_starts(n, marked=(16, 700000))
    assert starts[0] == 0 and starts[-1] == n - band.WINDOW and len(starts) >= 14
    assert any(s <= 700000 < s + band.WINDOW for s in starts) and any(s <= 16 < s + band.WINDOW for s in starts)
    assert starts == sorted(set(starts))
    gaps = np.diff(starts)
    assert gaps.max() <= n // 12
    assert band.window_starts(100, marked=(50,)) == [0]


def test_first_difference_names_the_element():
    a = torch.arange(24.0).reshape(2, 3, 4)
    assert band.first_difference(a, a.clone()) is None
    b = a.clone()
    b[1, 2, 1] = -1.0
    b[1, 2, 3] = float("nan")
    assert band.first_difference(b, a) == ((1, 2, 1), -1.0, 21.0)
    c = a.clone()
    c[0, 0, 0] = float("nan")
    assert band.first_difference(c, c)[0] == (0, 0, 0)


def test_the_max_reducer_operands_past_2_26_are_exact_in_bf16_and_tied():
    """test_gpu_large_edges.test_max_arg_forward_past_2_26 / test_max_backward_on_a_closed_form_argmax[bfloat16]: band.node_values at
    H = 1, N = 4 and the closed-form grad_out narrow to bf16 without a change (integers in -3 .. 3), a backward sum is an integer of at
    most 64 x 3 <= 2^8 in magnitude (exact in bf16's 8 significant bits), and the closed-form forward agrees with the reducer's
    restatement on a small band with ties in every word — the first-position rule decides them."""
    from max_arg_ref import max_arg_forward, tied_words

    d, M, N = 64, 300, 4
    K = band.sizes(M, d)[1]
    wide = band.node_values(K, 1, N)
    assert torch.equal(band.node_values(K, 1, N, dtype=torch.bfloat16).float(), wide) and int(wide.abs().max()) == 3
    r, n = torch.arange(M).view(-1, 1), torch.arange(N).view(1, -1)
    grad = ((r + 3 * n) % 7 - 3).to(torch.float32)
    assert torch.equal(grad.to(torch.bfloat16).float(), grad) and d * 3 <= (1 << 8)
    rowptr, colind = (t.numpy() for t in band.csr(M, d))
    B = wide.view(K, N).numpy()
    C, arg = max_arg_forward(rowptr, colind, B, -10000.0)
    j, f = torch.arange(d).view(1, -1, 1), torch.arange(N).view(1, 1, -1)
    vals = band.b_of(r.view(-1, 1, 1) + band.offset_of(j), 0, f)
    top = vals.max(1, keepdim=True).values
    first = torch.where(vals == top, j, d).min(1).values
    assert np.array_equal(C, top.view(-1, N).numpy().astype(np.float32)) and np.array_equal(arg, (r * d + first).numpy().astype(np.int32))
    assert tied_words(rowptr, colind, B, C, arg).all()


# ---- graphs.take_edges ----------------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _payloads(n, H, dtype):
    """n rows of distinct finite values with -0.0, infinities and NaNs of different payloads among them."""
    g = torch.Generator().manual_seed(n * 31 + H)
    x = torch.randn((n, H) if H else (n,), generator=g).to(dtype)
    flat = x.view(-1)
    flat[0] = -0.0
    flat[1] = float("inf")
    flat[2] = float("-inf")
    raw = _bits(x).view(-1)
    if dtype == torch.float32:
        raw[3], raw[4], raw[5] = 0x7FC00001, 0x7F800123, -4194304 + 77  # quiet, signalling, negative NaN payloads
    elif dtype in (torch.bfloat16, torch.float16):
        raw[3], raw[4] = (0x7FC1, 0x7F83) if dtype == torch.bfloat16 else (0x7E01, 0x7C03)
    else:
        raw[3], raw[4] = 0x7FF8000000000001, 0x7FF0000000000123
    assert torch.isnan(flat[3]) and torch.isnan(flat[4])
    return x


@pytest.mark.parametrize("index_dtype", (torch.int32, torch.int64))
@pytest.mark.parametrize("H", (0, 1, 4, 5))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16, torch.float64))
def test_take_edges_is_bit_equal_to_plain_indexing(pkg, dtype, H, index_dtype):
    from gespmm_amd import graphs

    n = 53
    x = _payloads(n, H, dtype)
    order = torch.randperm(n, generator=torch.Generator().manual_seed(7)).to(index_dtype)
    want = _bits(x[order.long()])
    for chunk in (1, 7, n - 1, n, 1 << 24):
        got = graphs.take_edges(x, order, chunk_rows=chunk)
        assert got.is_contiguous() and got.dtype == dtype and got.shape == x.shape
        assert torch.equal(_bits(got), want), (chunk,)
    assert torch.equal(_bits(graphs.take_edges(x, order)), want), "default chunk"
    assert torch.equal(_bits(x), _bits(_payloads(n, H, dtype))), "the input is left alone"


@pytest.mark.parametrize("chunk", (1, 7, 52))
def test_take_edges_non_contiguous_and_other_layouts(pkg, chunk):
    from gespmm_amd import graphs

    n = 53
    order = torch.randperm(n, generator=torch.Generator().manual_seed(9))
    wide = _payloads(n, 12, torch.float32)
    for x in (wide[:, 2:10:2], _payloads(12, n, torch.float32).t(), _payloads(2 * n, 4, torch.float32)[::2], wide.view(n, 3, 4)[:, :, 1:3]):
        assert not x.is_contiguous()
        got = graphs.take_edges(x, order, chunk_rows=chunk)
        assert got.is_contiguous() and torch.equal(_bits(got), _bits(x[order]))
    ints = torch.arange(n, dtype=torch.int64) * 3
    assert torch.equal(graphs.take_edges(ints, order.to(torch.int32), chunk_rows=chunk), ints[order])
    # an order with repeats is a gather all the same
    rep = torch.randint(0, n, (n,), generator=torch.Generator().manual_seed(3))
    assert torch.equal(_bits(graphs.take_edges(wide, rep, chunk_rows=chunk)), _bits(wide[rep]))


def test_take_edges_empty_and_errors(pkg):
    from gespmm_amd import graphs

    for shape in ((0,), (0, 4), (0, 2, 3)):
        for index_dtype in (torch.int32, torch.int64):
            got = graphs.take_edges(torch.empty(shape), torch.empty(0, dtype=index_dtype), chunk_rows=1)
            assert got.shape == shape and got.dtype == torch.float32
    x = torch.arange(40.0).reshape(10, 4)
    order = torch.arange(10)
    with pytest.raises(ValueError):
        graphs.take_edges(x, order[:9])
    with pytest.raises(ValueError):
        graphs.take_edges(x, torch.arange(11))
    with pytest.raises(ValueError):
        graphs.take_edges(x, order.view(2, 5))
    with pytest.raises(ValueError):
        graphs.take_edges(x, order, chunk_rows=0)
    with pytest.raises(TypeError):
        graphs.take_edges(x, order.float())
    for bad in (10, -1, 1 << 40):
        o = order.clone()
        o[6] = bad
        for chunk in (1, 7, 9, 1 << 24):
            with pytest.raises(IndexError):
                graphs.take_edges(x, o, chunk_rows=chunk)
    o32 = order.to(torch.int32)
    o32[0] = 10
    with pytest.raises(IndexError):
        graphs.take_edges(x, o32)


def test_take_edges_under_autograd(pkg):
    """What the call sites need: detached tensors and no-grad mode take the preallocated path; a tensor that requires grad keeps a
    gradient (pieces concatenated), equal to plain indexing's."""
    from gespmm_amd import graphs

    order = torch.randperm(20, generator=torch.Generator().manual_seed(1))
    x = torch.randn(20, 4, generator=torch.Generator().manual_seed(2), requires_grad=True)
    y = graphs.take_edges(x, order, chunk_rows=7)
    assert y.requires_grad and torch.equal(y, x[order])
    g = torch.randn(20, 4, generator=torch.Generator().manual_seed(3))
    (gx,) = torch.autograd.grad(y, x, g)
    (gx_ref,) = torch.autograd.grad(x[order], x, g)
    assert torch.equal(gx, gx_ref)
    with torch.no_grad():
        assert not graphs.take_edges(x, order, chunk_rows=7).requires_grad
    assert not graphs.take_edges(x.detach(), order, chunk_rows=7).requires_grad


def test_transpose_csr_values_go_through_take_edges(pkg):
    from gespmm_amd import graphs

    M, d = 200, 7
    rowptr, colind = band.csr(M, d)
    nnz, K = band.sizes(M, d)
    w = band.edge_values(torch.arange(nnz), 4)
    colptr, rowind, w_csc, order = graphs.transpose_csr(rowptr, colind, K, val=w, return_order=True)
    want_ptr, want_ind, want_order = band.csc(M, d)
    assert torch.equal(colptr, want_ptr) and torch.equal(rowind, want_ind) and torch.equal(order, want_order)
    assert w_csc.is_contiguous() and torch.equal(w_csc, band.edge_values(want_order, 4))
