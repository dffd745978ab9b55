"""A band pattern whose CSR arrays, CSC arrays, CSR -> CSC edge order, edge weights, node features AND products are closed forms
(plain module beside helpers.py; shared by test_large_edges_host.py and test_gpu_large_edges.py).

Row r of an M-row pattern holds the d columns r + o_j, o_j = 3 j + (j^2 mod 3) = 0, 4, 7, 9, 13, 16, .. (strictly increasing), so
nnz = M d and K = M + o_{d-1}. Column c holds the rows c - o_j, for DESCENDING j (ascending rows) with 0 <= c - o_j < M; the valid j
of a column are a contiguous range because o is increasing, which makes every CSC array elementwise arithmetic on the column number:
nothing here gathers or scatters by an edge-sized index, so the pattern can be built past 2^26 edges without trusting the indexing
it is there to test. Weights and features are small integers of the edge / node number, so every fp32 sum is exact and the product
of a window of rows or columns is an int64 broadcast with no index array at all."""
import torch

WINDOW = 4096


def offset_of(j):
    """o_j, elementwise (tensor or int)."""
    return 3 * j + (j * j) % 3


def sizes(M, d):
    """(nnz, K)"""
    return M * d, M + offset_of(d - 1)


def _count_le(c, d):
    """Number of j in [0, d) with o_j <= c, elementwise on an integer tensor (c may be negative): o_{3m..3m+2} = 9m, 9m+4, 9m+7."""
    q = torch.div(c, 9, rounding_mode="floor")
    rem = c - 9 * q
    return (3 * q + 1 + (rem >= 4).to(c.dtype) + (rem >= 7).to(c.dtype)).clamp_(0, d)


def in_degree(M, d, device="cpu"):
    """int64[K]: entries of every column (at least one each when M > o_{d-1})."""
    c = torch.arange(sizes(M, d)[1], device=device, dtype=torch.int64)
    return _count_le(c, d) - _count_le(c - M, d)


def csr(M, d, device="cpu"):
    """(rowptr int32[M+1], colind int32[nnz])"""
    rowptr = (torch.arange(M + 1, device=device, dtype=torch.int64) * d).to(torch.int32)
    o = offset_of(torch.arange(d, device=device, dtype=torch.int32))
    colind = (torch.arange(M, device=device, dtype=torch.int32).unsqueeze(1) + o.unsqueeze(0)).reshape(-1)
    return rowptr, colind


def csc(M, d, device="cpu"):
    """(colptr int32[K+1], rowind int32[nnz], csc_order int64[nnz]): CSC position i holds CSR entry csc_order[i] = (c - o_j) d + j.
    Elementwise ops, one cumsum over K and two repeat_interleave by the in-degrees."""
    nnz, K = sizes(M, d)
    deg = in_degree(M, d, device)
    colptr = torch.zeros(K + 1, dtype=torch.int64, device=device)
    colptr[1:] = torch.cumsum(deg, 0)
    col = torch.repeat_interleave(torch.arange(K, device=device, dtype=torch.int64), deg, output_size=nnz)
    j = torch.repeat_interleave(colptr[:-1], deg, output_size=nnz)  # the start of the position's column ...
    j = torch.arange(nnz, device=device, dtype=torch.int64).sub_(j)  # ... the position's rank t inside it ...
    j = _count_le(col, d).sub_(1).sub_(j)  # ... and j = (largest j with o_j <= c) - t
    row = col.sub_(offset_of(j))
    del col
    rowind = row.to(torch.int32)
    order = row.mul_(d).add_(j)
    return colptr.to(torch.int32), rowind, order


def verify_csc(M, d, colptr, order):
    """Independent check of ``csc``'s result through what a transpose IS: the (column, row) pairs decoded from csc_order are strictly
    increasing in lexicographic order (so csc_order is a permutation, columns ascend and rows ascend inside a column), the positions
    where the column changes are colptr's segment starts, and the entries sum to nnz (nnz - 1) / 2. Shifted views only."""
    nnz, K = sizes(M, d)
    assert M > offset_of(d - 1), "every column needs an entry for the segment check"
    assert order.dtype == torch.int64 and order.numel() == nnz and colptr.numel() == K + 1
    assert int(order.min()) >= 0 and int(order.max()) < nnz
    assert int(order.sum()) == nnz * (nnz - 1) // 2
    j = order % d
    col = torch.div(order, d, rounding_mode="floor")  # the row for now
    key = (col + offset_of(j)).mul_(M).add_(col)  # column * M + row
    del j, col
    assert bool((key[1:] > key[:-1]).all()), "(column, row) not strictly increasing"
    col = torch.div(key, M, rounding_mode="floor")
    del key
    assert int(col[0]) == 0 and int(col[-1]) == K - 1
    starts = torch.nonzero(col[1:] != col[:-1]).flatten().add_(1)
    assert starts.numel() == K - 1, "a column is missing"
    assert torch.equal(starts, colptr[1:-1].to(torch.int64)), "column changes are not at colptr"
    assert int(colptr[0]) == 0 and int(colptr[-1]) == nnz


# ---- closed-form operands: small integers of the edge / node number ----------------------------------------------------------------

def w_of(e, h):
    """weight of CSR entry e, head h: ((7 e + 3 h) mod 5) - 2, in [-2, 2]"""
    return (7 * e + 3 * h) % 5 - 2


def b_of(r, h, f):
    """feature f of head h of node r: ((r + 5 h + 11 f) mod 7) - 3, in [-3, 3]"""
    return (r + 5 * h + 11 * f) % 7 - 3


def k_of(r, h, f):
    """a second node array, ((3 r + h + 2 f) mod 5) - 2, in [-2, 2]"""
    return (3 * r + h + 2 * f) % 5 - 2


def edge_values(e, H, dtype=torch.float32, fn=w_of):
    """[len(e), H] of ``dtype``: fn(e[i], h), head by head (no [nnz, H] integer temporary). ``e`` = arange(nnz) gives the weights in CSR
    order, ``e`` = csc_order the same weights in CSC order — elementwise, with no gather. The entries of ``e`` are
    entry numbers below len(e) (an arange or a permutation of it)."""
    out = torch.empty((e.numel(), H), dtype=dtype, device=e.device)
    if e.numel() and 7 * e.numel() + 3 * H < (1 << 31):
        e = e.to(torch.int32)  # entry numbers below len(e): the arithmetic fits, at half the temporaries
    for h in range(H):
        out[:, h] = fn(e, h)
    return out


def node_values(R, H, F, device="cpu", dtype=torch.float32, fn=b_of):
    """[R, H, F] of ``dtype``: fn(r, h, f)"""
    r = torch.arange(R, device=device, dtype=torch.int32).view(R, 1, 1)
    h = torch.arange(H, device=device, dtype=torch.int32).view(1, H, 1)
    f = torch.arange(F, device=device, dtype=torch.int32).view(1, 1, F)
    return fn(r, h, f).to(dtype)


def _hf(H, F, device):
    return (torch.arange(H, device=device, dtype=torch.int64).view(1, 1, H, 1),
            torch.arange(F, device=device, dtype=torch.int64).view(1, 1, 1, F))


def ref_csr_product(M, d, r0, r1, H, F, device="cpu", dense_fn=b_of, weight_fn=w_of):
    """int64[r1 - r0, H, F]: rows r0 .. r1 of out[r, h, f] = sum_j w(r d + j, h) * dense(r + o_j, h, f) — the multi-head product on the
    CSR arrays with the closed-form weights and a closed-form dense operand of K rows."""
    r = torch.arange(r0, r1, device=device, dtype=torch.int64).view(-1, 1, 1, 1)
    j = torch.arange(d, device=device, dtype=torch.int64).view(1, d, 1, 1)
    h, f = _hf(H, F, device)
    return (weight_fn(r * d + j, h) * dense_fn(r + offset_of(j), h, f)).sum(1)


def ref_csc_product(M, d, c0, c1, H, F, device="cpu", dense_fn=b_of, weight_fn=w_of):
    """int64[c1 - c0, H, F]: columns c0 .. c1 of out[c, h, f] = sum_j valid * w((c - o_j) d + j, h) * dense(c - o_j, h, f) — the product
    on the CSC arrays (A^T) with the same weights in CSC order and a dense operand of M rows."""
    c = torch.arange(c0, c1, device=device, dtype=torch.int64).view(-1, 1, 1, 1)
    j = torch.arange(d, device=device, dtype=torch.int64).view(1, d, 1, 1)
    h, f = _hf(H, F, device)
    r = c - offset_of(j)
    valid = ((r >= 0) & (r < M)).to(torch.int64)
    return (valid * weight_fn(r * d + j, h) * dense_fn(r, h, f)).sum(1)


def ref_csr_scores(M, d, r0, r1, H, F, device="cpu", q_fn=b_of, k_fn=k_of):
    """int64[(r1 - r0) d, H]: the CSR entries of rows r0 .. r1 of s[e, h] = sum_f q(row(e), h, f) * k(col(e), h, f)."""
    r = torch.arange(r0, r1, device=device, dtype=torch.int64).view(-1, 1, 1, 1)
    j = torch.arange(d, device=device, dtype=torch.int64).view(1, d, 1, 1)
    h, f = _hf(H, F, device)
    return (q_fn(r, h, f) * k_fn(r + offset_of(j), h, f)).sum(3).reshape(-1, H)


def window_starts(n_segments, marked=(), spread=14, window=WINDOW):
    """The fixed list of window starts over ``n_segments`` rows (or columns): ``spread`` windows from the first to the last, evenly
    spaced, and one centred on every marked segment. Sorted, without repeats; a window is [s, min(s + window, n_segments))."""
    last = max(n_segments - window, 0)
    starts = {(last * i) // (spread - 1) for i in range(spread)}
    starts.update(min(max(int(s) - window // 2, 0), last) for s in marked)
    return sorted(starts)


def first_difference(got, want):
    """None when the two tensors of one shape are equal in every word, else the index tuple of the first differing element with both
    values (NaN differs from everything, itself included)."""
    ne = torch.nonzero((got != want).reshape(-1))
    if ne.numel() == 0:
        return None
    flat = int(ne[0])
    idx = []
    for n in reversed(got.shape):
        idx.append(flat % n)
        flat //= n
    idx = tuple(reversed(idx))
    return idx, got[idx].item(), want[idx].item()
