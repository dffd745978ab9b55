"""The attention ops on NODE-sized operands past 2 GB, past 4 GB and at the largest sizes their entries accept.

test_gpu_large_edges.py goes past 2^26 edges; its dense operands stay below 2 GB. Here the pattern is thin — tests/band.py's band
at d = 8, K = M + 22 — and the dense operands are wide: (H, F) = (8, 64), rows of 2048 bytes whose boundaries fall on the powers of
two, and (3, 100), rows of 1200 bytes, so that bytes 2^31 and 2^32 fall INSIDE a row. tests/large_operands.py derives every size;
tests/test_large_operands_host.py checks, without a device, that the windows compared here hold the rows with byte 2^31, byte 2^32
and the last word of every operand, that "below" and "at" lie on the two sides of each route switch, and that every comparison used
here rejects a reference gathered through a byte offset displaced by 2^31 or 2^32.

a. The kernels that form ``uint32_t`` byte offsets into the gathered operand (spmm_heads_kernel.h, gat_aggregate.hip,
   spmm_max_arg.hip) run with the largest gathered operand below 2^32 bytes — route 1 asserted from the host-only route function —
   and one row more: route 0 and the same exact results through the composition; the max reducer has no composition and must
   raise GESPMM_ERANGE. Both walks: over rows (the gathered operand has K rows) and over columns (M rows).
b. The kernels that form ``int`` word positions (sddmm_heads.h and sddmm_edge.h use size_t and run beside them; gatv2_score.hip,
   dot_attention.hip, gat_backward.hip) run in regime A, 5.4 GB an array, and in regime B, the largest M and K the entry accepts —
   found here by calling the entry with null pointers: K is taken, K + 1 answers GESPMM_ERANGE. The last window of regime B ends
   with the last node: its words are the highest positions these kernels may ever form.
c. The two files that landed after that audit and form the same ``int`` positions behind the same checks: the fused GATv2 attention
   (gatv2_attention.hip; regimes A and B at p = 0 and 0.25, and once with every dense operand 4 bytes off a 16-byte boundary: the
   V = 1 kernels) and the GATv2 score on fp16 / bf16 operands (gatv2_score_x16.hip), whose limit counts ELEMENTS — regime A has byte
   2^31 inside every 16-bit operand, regime B ends them just below byte 2^32 — with the fp32 kernels on the exact widening as the
   oracle over the WHOLE arrays, bit for bit.

Sum-type ops get small integers of the word position (lo.b_at, lo.k_at: a value differs from every alias 2^31 or 2^32 bytes away)
and must EQUAL an int64 closed form on every word of every window; float ops get seeded random values and the float64 references
and tolerances of their own tests, on 512-row sub-patterns of the marked, first and last windows (test_gpu_large_edges.py section
e). Every result goes into a NaN-prefilled tensor and must hold no NaN anywhere. Dense operands are filled in row chunks (integer
temporaries of 256 MB) or in place. No tolerance is new.

Section a also runs the max reducer's 16-bit entries (spmm_max_arg_kernel.h) at the same limit, which counts the 4-byte words of
``arg``: the backward reads grad_out at ``(off + 4 c) >> 1`` with the top bit of the ``uint32_t`` sum set in the upper half of the rows.

On the MI355X the module takes 86 s for 89 tests (84 s for 83 before the six 16-bit max-reducer cases; the slowest 6.2 s; single
times move by seconds with the allocation and release of tens of GB, the kernels take milliseconds) and peaks at 65.6 GiB of device
memory (dot attention in regime B: eight arrays of 8 GB). The slowest new case, test_max_arg_x16_below_the_4gb_limit, took 0.05 s
in the module's run and 1.24 s ([8x64-fp16]) in a run of the max-reducer cases alone; its peak is below the fp32 case's (the two
largest arrays halve)."""
import numpy as np
import pytest
import torch

import band
import large_operands as lo
from test_gpu_large_edges import DEV, DROPOUT_SEED, FLOAT_ROWS, Band, Sub, _check_windows, _gen, _nan, _poison

pytestmark = pytest.mark.gpu

D = lo.D
ERANGE, EINVAL = -3, -1
SIDES = ("below", "at")
WALKS = ("rows", "cols")
REGIMES = ("A", "B")
WIDTH_IDS = ["%dx%d" % w for w in lo.WIDTHS]


@pytest.fixture(autouse=True)
def _release():
    yield
    _BANDS.clear()
    torch.cuda.empty_cache()


_BANDS = {}


def _band(M):
    """The band of M rows, verified (band.verify_csc inside Band), with the windows of the case."""
    if M not in _BANDS:
        _BANDS.clear()
        torch.cuda.empty_cache()
        _BANDS[M] = Band(M, D)
    g = _BANDS[M]
    assert g.K == M + lo.LAST and g.nnz == M * D
    return g


def _need(gib):
    free = torch.cuda.mem_get_info()[0]
    if free < gib * (1 << 30):
        pytest.skip("needs %d GiB of free device memory, %.1f are free" % (gib, free / (1 << 30)))


def _nodes(R, H, F, dtype=torch.float32, fn=None):
    """[R, H, F] of fn(r, h, f) (default: lo.b_at(H, F)) in row chunks: integer temporaries of at most 256 MB each."""
    fn = lo.b_at(H, F) if fn is None else fn
    out = torch.empty((R, H, F), dtype=dtype, device=DEV)
    itype = torch.int32 if R * H * F < (1 << 31) else torch.int64  # (the functions form the word position)
    step = max(1, (1 << (26 if itype == torch.int32 else 25)) // (H * F))
    h = torch.arange(H, device=DEV, dtype=itype).view(1, H, 1)
    f = torch.arange(F, device=DEV, dtype=itype).view(1, 1, F)
    for r0 in range(0, R, step):
        r1 = min(r0 + step, R)
        out[r0:r1] = fn(torch.arange(r0, r1, device=DEV, dtype=itype).view(-1, 1, 1), h, f)
    return out


def _uniform(gen, shape, lo_, hi):
    """Seeded uniform values drawn in place: no temporary."""
    return torch.empty(shape, dtype=torch.float32, device=DEV).uniform_(lo_, hi, generator=gen)


def _written(**results):
    """No NaN in any word, windows or not; 2^28 words at a time."""
    for name, t in results.items():
        flat = t.reshape(-1)
        for a in range(0, flat.numel(), 1 << 28):
            assert not bool(torch.isnan(flat[a:a + (1 << 28)]).any()), "a word of %s was not written" % name


def _windows(g, N, elem=4, spread=14):
    rw, cw = lo.case_windows(g.M, g.K, N, elem, spread)
    assert rw[0][0] == 0 and rw[-1][1] == g.M and cw[0][0] == 0 and cw[-1][1] == g.K
    return rw, cw


def _subs(g, rw):
    """FLOAT_ROWS-row sub-patterns of the row windows: the marked row of a window in its middle, the last rows of the last window."""
    assert lo.FLOAT_ROWS == FLOAT_ROWS
    out = [Sub(g, *lo.sub_rows(w, g.M)) for w in rw]
    assert out[0].r0 == 0 and out[-1].r1 == g.M and out[-1].f1 == g.K
    return out


one = lambda e, h: 1  # noqa: E731


# ---- a. the kernels with uint32 byte offsets, on both sides of the 4 GB switch ---------------------------------------------------------

def _heads_case(H, F, side, walk, dtype, fn, route):
    N, elem = H * F, (4 if dtype == torch.float32 else 2)
    M, K = lo.sizes_a(N, side, walk, elem)
    _need(24)
    g = _band(M)
    rw, cw = _windows(g, N, elem)
    gathered = K if walk == "rows" else M
    assert (gathered * N * elem < (1 << 32)) == (side == "below")
    what = "H=%d F=%d %s %s %s" % (H, F, dtype, side, walk)
    if walk == "rows":
        assert route(M, K, H, F, g.nnz)[0] == (1 if side == "below" else 0), what
        dense = _nodes(K, H, F, dtype)
        out = fn(g.rowptr, g.colind, g.weights(H, fn=lo.w_nz), dense, out=_nan((M, H, F), dtype))
        ref = lambda r0, r1: band.ref_csr_product(M, D, r0, r1, H, F, DEV, dense_fn=lo.b_at(H, F), weight_fn=lo.w_nz)  # noqa: E731
        _check_windows("heads product, rows, " + what, out, rw, ref)
        _written(out=out)
        # order=: the weights stored back to front and read through the reversing order
        back = (g.nnz - 1) - torch.arange(g.nnz, device=DEV, dtype=torch.int32)
        out = fn(g.rowptr, g.colind, band.edge_values(back, H, fn=lo.w_nz), dense, out=_nan((M, H, F), dtype), order=back)
        _check_windows("heads product, rows, order=, " + what, out, rw, ref)
        _written(out=out)
    else:
        assert route(K, M, H, F, g.nnz)[0] == (1 if side == "below" else 0), what
        dense = _nodes(M, H, F, dtype, lo.k_at(H, F))
        ref = lambda c0, c1: band.ref_csc_product(M, D, c0, c1, H, F, DEV, dense_fn=lo.k_at(H, F), weight_fn=lo.w_nz)  # noqa: E731
        out = fn(g.colptr, g.rowind, g.weights_csc(H, fn=lo.w_nz), dense, out=_nan((K, H, F), dtype))
        _check_windows("heads product, columns, " + what, out, cw, ref)
        _written(out=out)
        # order=: the weights in CSR order read through the CSR -> CSC edge order
        out = fn(g.colptr, g.rowind, g.weights(H, fn=lo.w_nz), dense, out=_nan((K, H, F), dtype), order=g.order32)
        _check_windows("heads product, columns, order=, " + what, out, cw, ref)
        _written(out=out)


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_heads_product_across_the_4gb_switch(pkg, H, F, side, walk):
    from gespmm_amd import _lib, spmm

    _heads_case(H, F, side, walk, torch.float32, spmm.csr_spmm_heads, _lib.heads_route)


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16), ids=("bf16", "fp16"))
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_heads_product_x16_across_the_4gb_switch(pkg, H, F, dtype, side, walk):
    from gespmm_amd import _lib, spmm

    _heads_case(H, F, side, walk, dtype, spmm.csr_spmm_heads_x16, _lib.heads_x16_route)


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_gat_aggregate_across_the_4gb_switch(pkg, H, F, side, walk):
    """er = 0 makes the 8 scores of a row equal: alpha = exp(0) / 8 = 2^-3 in every entry, the statistics are exact (m =
    leaky_relu(el), s = 8) and the aggregation is an integer sum scaled by a power of two (test_gpu_large_edges.py's idiom)."""
    from gespmm_amd import _lib, softmax, spmm

    N, slope = H * F, 0.25
    M, K = lo.sizes_a(N, side, walk)
    _need(24)
    g = _band(M)
    rw, cw = _windows(g, N)
    transposed = walk == "cols"
    assert _lib.gat_aggregate_route(M, K, H, F, g.nnz, transposed=transposed)[0] == (1 if side == "below" else 0)
    el = _nodes(M, H, 1, fn=band.b_of).view(M, H).contiguous() * 0.5
    er = torch.zeros((K, H), device=DEV)
    stats = softmax.gat_softmax_stats(g.rowptr, g.colind, el, er, negative_slope=slope, out=_nan((M, H, 2)))
    assert torch.equal(stats[:, :, 0], torch.where(el > 0, el, el * slope)) and bool((stats[:, :, 1] == float(D)).all())
    if transposed:
        dense = _nodes(M, H, F, fn=lo.k_at(H, F))
        out = spmm.gat_aggregate(g.colptr, g.rowind, el, er, stats, dense, negative_slope=slope, transposed=True, out=_nan((K, H, F)))
        _written(out=out)
        _check_windows("gat_aggregate(transposed=True) %s" % side, out.mul_(float(D)), cw,
                       lambda c0, c1: band.ref_csc_product(M, D, c0, c1, H, F, DEV, dense_fn=lo.k_at(H, F), weight_fn=one))
    else:
        dense = _nodes(K, H, F)
        out = spmm.gat_aggregate(g.rowptr, g.colind, el, er, stats, dense, negative_slope=slope, out=_nan((M, H, F)))
        _written(out=out)
        _check_windows("gat_aggregate %s" % side, out.mul_(float(D)), rw,
                       lambda r0, r1: band.ref_csr_product(M, D, r0, r1, H, F, DEV, dense_fn=lo.b_at(H, F), weight_fn=one))


def _arg_and_grad(M, N):
    """arg[r, n] = r d + ((r + n) mod d), grad_out[r, n] = ((r + 3 n) mod 7) - 3, in row chunks."""
    arg = torch.empty((M, N), dtype=torch.int32, device=DEV)
    grad = torch.empty((M, N), dtype=torch.float32, device=DEV)
    n = torch.arange(N, device=DEV, dtype=torch.int32).view(1, -1)
    step = max(1, (1 << 26) // N)
    for r0 in range(0, M, step):
        r = torch.arange(r0, min(r0 + step, M), device=DEV, dtype=torch.int32).view(-1, 1)
        arg[r0:r0 + step] = r * D + (r + n) % D
        grad[r0:r0 + step] = (r + 3 * n) % 7 - 3
    return arg, grad


@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_max_arg_below_the_4gb_limit(pkg, H, F):
    """Forward: out[r, n] = max_j b(r + o_j, n) and arg the CSR position of the FIRST entry that reaches it. Backward on a closed-form
    argmax (test_gpu_large_edges.py): column k receives grad_out[r, n] from every row r = k - o_j with (r + n) mod d == j."""
    from gespmm_amd import _lib, spmm

    N = H * F
    M, K = lo.sizes_a(N, "below", "rows")
    _need(24)
    g = _band(M)
    rw, cw = _windows(g, N)
    assert _lib.max_arg_route(M, g.nnz, N) is not None and _lib.max_arg_route(K, g.nnz, N) is not None
    dense = _nodes(K, H, F).view(K, N)
    out, arg = spmm.csr_spmm_max_arg(g.rowptr, g.colind, dense, out=_nan((M, N)), arg=torch.full((M, N), -7, dtype=torch.int32, device=DEV))
    _written(out=out)
    assert int(arg.min()) >= 0
    j = torch.arange(D, device=DEV, dtype=torch.int64).view(1, D, 1, 1)
    hh, ff = band._hf(H, F, DEV)
    for r0, r1 in rw:
        r = torch.arange(r0, r1, device=DEV, dtype=torch.int64).view(-1, 1, 1, 1)
        vals = lo.b_at(H, F)(r + band.offset_of(j), hh, ff)
        top = vals.max(1, keepdim=True).values
        first = torch.where(vals == top, j, D).min(1).values
        assert torch.equal(out[r0:r1], top.reshape(r1 - r0, N).to(torch.float32)), "max, rows %d .. %d" % (r0, r1)
        assert torch.equal(arg[r0:r1].long(), (r.view(-1, 1, 1) * D + first).reshape(r1 - r0, N)), "arg, rows %d .. %d" % (r0, r1)
    del dense, out, arg, vals, top, first
    arg, grad_out = _arg_and_grad(M, N)
    grad = spmm.csr_spmm_max_backward(g.colptr, g.rowind, g.order32, arg, grad_out, K, out=_nan((K, N)))
    _written(grad=grad)
    nn = torch.arange(N, device=DEV, dtype=torch.int64).view(1, 1, -1)

    def ref(c0, c1):
        c = torch.arange(c0, c1, device=DEV, dtype=torch.int64).view(-1, 1, 1)
        jj = torch.arange(D, device=DEV, dtype=torch.int64).view(1, -1, 1)
        rr = c - band.offset_of(jj)
        hit = (rr >= 0) & (rr < M) & ((rr + nn) % D == jj)
        return (hit.to(torch.int64) * ((rr + 3 * nn) % 7 - 3)).sum(1)

    _check_windows("csr_spmm_max_backward", grad, cw, ref)


@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_max_arg_refuses_the_first_size_past_the_limit(pkg, H, F):
    """One row more of the gathered operand: there is no composition, both calls raise GespmmError with GESPMM_ERANGE and write nothing."""
    from gespmm_amd import _lib, spmm

    N = H * F
    M, K = lo.sizes_a(N, "at", "rows")
    assert K * N * 4 >= (1 << 32) > (K - 1) * N * 4
    _need(16)
    g = _band(M)
    dense, out = torch.empty((K, N), device=DEV), _nan((M, N))
    arg = torch.full((M, N), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.GespmmError) as e:
        spmm.csr_spmm_max_arg(g.rowptr, g.colind, dense, out=out, arg=arg)
    assert e.value.code == ERANGE and "gespmm_csr_spmm_max_arg_f32" in str(e.value)
    assert bool(torch.isnan(out[-4096:]).all()) and bool((arg[-4096:] == -7).all())
    grad = _nan((K, N))
    with pytest.raises(_lib.GespmmError) as e:
        spmm.csr_spmm_max_backward(g.colptr, g.rowind, g.order32, arg, out, K, out=grad)
    assert e.value.code == ERANGE and "gespmm_csr_spmm_max_backward_f32" in str(e.value)
    assert bool(torch.isnan(grad[-4096:]).all())


X16_DTYPES, X16_IDS = (torch.bfloat16, torch.float16), ("bf16", "fp16")


@pytest.mark.parametrize("dtype", X16_DTYPES, ids=X16_IDS)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_max_arg_x16_below_the_4gb_limit(pkg, H, F, dtype):
    """The 16-bit entries at the largest size ``max_arg_sizes`` accepts. The limit counts the 4-byte ``arg`` words: arg ends just below
    byte 2^32 and the 16-bit B, out, grad_out and grad_B just below byte 2^31. The backward stages the arg row's byte offset r N 4 as
    ``uint32_t`` and reads grad_out at ``(off + 4 c) >> 1``: above row 2^31 / (4 N) the sum has its top bit set, and a signed shift, a
    31-bit mask or an ``int`` temporary in that expression is wrong only there — those rows, and the last, lie inside the windows
    (tests/test_large_operands_host.py). The closed forms are test_max_arg_below_the_4gb_limit's (lo.ref_max_forward,
    lo.ref_max_backward); every value is an integer of at most 8 x 3 in magnitude, exact in both types."""
    from gespmm_amd import _lib, spmm

    N = H * F
    M, K = lo.sizes_a(N, "below", "rows")
    assert K * N * 4 < (1 << 32) <= (K + 1) * N * 4 and K * N * 2 < (1 << 31)
    _need(24)
    g = _band(M)
    rw, cw = _windows(g, N)
    assert _lib.max_arg_route_x16(M, g.nnz, N) is not None and _lib.max_arg_route_x16(K, g.nnz, N) is not None
    dense = _nodes(K, H, F, dtype).view(K, N)
    out, arg = spmm.csr_spmm_max_arg_x16(g.rowptr, g.colind, dense, out=_nan((M, N), dtype),
                                         arg=torch.full((M, N), -7, dtype=torch.int32, device=DEV))
    assert out.dtype == dtype
    _written(out=out)
    assert int(arg.min()) >= 0
    for r0, r1 in rw:
        top, first = lo.ref_max_forward(r0, r1, H, F, DEV)
        assert torch.equal(out[r0:r1].float(), top.to(torch.float32)), "max, rows %d .. %d" % (r0, r1)
        assert torch.equal(arg[r0:r1].long(), first), "arg, rows %d .. %d" % (r0, r1)
    del dense, out, arg, top, first
    arg, grad_out = _arg_and_grad(M, N)
    tail, nn = torch.arange(M - 64, M, device=DEV).view(-1, 1), torch.arange(N, device=DEV).view(1, -1)
    assert torch.equal(arg[-64:].long(), lo.max_arg_at(tail, nn)) and torch.equal(grad_out[-64:].long(), lo.max_grad_at(tail, nn))
    grad_out = grad_out.to(dtype)
    grad = spmm.csr_spmm_max_backward_x16(g.colptr, g.rowind, g.order32, arg, grad_out, K, out=_nan((K, N), dtype))
    assert grad.dtype == dtype
    _written(grad=grad)
    _check_windows("csr_spmm_max_backward_x16", grad, cw, lambda c0, c1: lo.ref_max_backward(M, c0, c1, N, DEV))


@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_max_arg_x16_refuses_the_first_size_past_the_limit(pkg, H, F):
    """One row more: both 16-bit entries raise GespmmError with GESPMM_ERANGE, with real arrays, and write nothing (bf16)."""
    from gespmm_amd import _lib, spmm

    N, dtype = H * F, torch.bfloat16
    M, K = lo.sizes_a(N, "at", "rows")
    assert K * N * 4 >= (1 << 32) > (K - 1) * N * 4
    _need(24)
    g = _band(M)
    dense, out = torch.empty((K, N), dtype=dtype, device=DEV), _nan((M, N), dtype)
    arg = torch.full((M, N), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.GespmmError) as e:
        spmm.csr_spmm_max_arg_x16(g.rowptr, g.colind, dense, out=out, arg=arg)
    assert e.value.code == ERANGE and "gespmm_csr_spmm_max_arg_x16" in str(e.value)
    assert bool(torch.isnan(out[-4096:]).all()) and bool((arg[-4096:] == -7).all())
    grad = _nan((K, N), dtype)
    with pytest.raises(_lib.GespmmError) as e:
        spmm.csr_spmm_max_backward_x16(g.colptr, g.rowind, g.order32, arg, out, K, out=grad)
    assert e.value.code == ERANGE and "gespmm_csr_spmm_max_backward_x16" in str(e.value)
    assert bool(torch.isnan(grad[-4096:]).all())


# ---- b. the kernels with int word positions: regime A (5.4 GB an array) and regime B (the largest the entry accepts) -------------------

def _accepted(call, N):
    """Regime B's K from the entry itself: with null pointers a call answers GESPMM_EINVAL once its sizes are accepted and
    GESPMM_ERANGE when one is too large. K is taken, K + 1 (a K-side operand of one row more) is refused."""
    K = lo.regime_rows(N, "B")
    assert call(K - lo.LAST, K) == EINVAL, "the largest K must be accepted"
    assert call(K - lo.LAST, K + 1) == ERANGE, "one row more must be refused"
    return K


def _sizes_b(N, regime, call=None):
    M, K = lo.sizes_b(N, regime)
    if regime == "B" and call is not None:
        assert _accepted(call, N) == K
    assert K * N <= lo.MAX_WORDS and (K * N > (1 << 30)) and (regime == "A" or (K + 1) * N > lo.MAX_WORDS)
    return M, K


@pytest.mark.parametrize("x16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_sddmm_heads_csr_and_coo(pkg, H, F, regime, x16):
    """size_t arithmetic (sddmm_heads.h): the entries have no limit on M H F; the sizes are those of the kernels beside them."""
    from gespmm_amd import _lib, sddmm

    N = H * F
    M, K = _sizes_b(N, regime)
    _need(40)
    g = _band(M)
    rw, _ = _windows(g, N, 2 if x16 else 4)
    dtype = torch.bfloat16 if x16 else torch.float32
    assert _lib.describe_sddmm_heads(True, M, g.nnz, H, F, x16=x16)["route"] == "kernel"
    assert _lib.describe_sddmm_heads(False, M, g.nnz, H, F, x16=x16)["route"] == "kernel"
    q, k = _nodes(M, H, F, dtype), _nodes(K, H, F, dtype, lo.k_at(H, F))
    csr_fn, coo_fn = (sddmm.csr_sddmm_heads_x16, sddmm.coo_sddmm_heads_x16) if x16 else (sddmm.csr_sddmm_heads, sddmm.coo_sddmm_heads)
    ref = lambda r0, r1: band.ref_csr_scores(M, D, r0, r1, H, F, DEV, q_fn=lo.b_at(H, F), k_fn=lo.k_at(H, F))  # noqa: E731
    s = csr_fn(g.rowptr, g.colind, q, k, out=_nan((g.nnz, H)))
    _check_windows("csr_sddmm_heads %s regime %s" % (dtype, regime), s, rw, ref, scale=D)
    rows = torch.div(torch.arange(g.nnz, device=DEV, dtype=torch.int32), D, rounding_mode="floor")
    s2 = coo_fn(rows, g.colind, q, k, out=_nan((g.nnz, H)))
    _written(csr=s, coo=s2)
    assert torch.equal(s, s2), "the two forms agree in every word"


@pytest.mark.parametrize("regime", REGIMES)
def test_plain_sddmm_at_width_512(pkg, regime):
    from gespmm_amd import sddmm

    N = 512
    M, K = _sizes_b(N, regime)
    _need(40)
    g = _band(M)
    rw, _ = _windows(g, N)
    d1, d2 = _nodes(M, 1, N).view(M, N), _nodes(K, 1, N, fn=lo.k_at(1, N)).view(K, N)
    _poison((g.nnz,))
    s = sddmm.csr_sddmm(g.rowptr, g.colind, d1, d2)
    _written(s=s)
    _check_windows("csr_sddmm N=512 regime %s" % regime, s.view(-1, 1), rw, lambda r0, r1: band.ref_csr_scores(M, D, r0, r1, 1, N, DEV, q_fn=lo.b_at(1, N), k_fn=lo.k_at(1, N)), scale=D)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_gatv2_score_forward_and_both_backward_passes(pkg, H, F, regime):
    from gespmm_amd import _lib, sddmm
    from test_gatv2_host import restate_backward, restate_score, worst_ratio

    N, slope, gen = H * F, 0.2, _gen(23)
    lib = _lib.lib
    M, K = _sizes_b(N, regime, lambda m, k: lib.gespmm_gatv2_score_f32(*[None] * 6, m, k, H, F, m * D, slope, None))
    if regime == "B":  # the column pass: S = K segments, T = M rows
        assert lib.gespmm_gatv2_score_backward_f32(*[None] * 9, K, M, H, F, M * D, slope, None) == EINVAL
        assert lib.gespmm_gatv2_score_backward_f32(*[None] * 9, K + 1, M, H, F, M * D, slope, None) == ERANGE
    _need(64)
    g = _band(M)
    rw, _ = _windows(g, N, spread=2)
    subs = _subs(g, rw)
    xl, xr = _uniform(gen, (M, H, F), -1, 1), _uniform(gen, (K, H, F), -1, 1)
    att, gsc = _uniform(gen, (H, F), -2, 2), _uniform(gen, (g.nnz, H), -2, 2)
    score = sddmm.gatv2_score(g.rowptr, g.colind, xl, xr, att, negative_slope=slope, out=_nan((g.nnz, H)))
    gxl, part = sddmm.gatv2_score_backward(g.rowptr, g.colind, gsc, xl, xr, att, negative_slope=slope, want_att_part=True,
                                           out=(_nan((M, H, F)), _nan((M, H, F))))
    gxr = sddmm.gatv2_score_backward(g.colptr, g.rowind, gsc, xr, xl, att, negative_slope=slope, order=g.order32, out=_nan((K, H, F)))
    _written(score=score, grad_xl=gxl, att_part=part, grad_xr=gxr)
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
    print("gatv2 H=%d F=%d regime %s: worst error / bound %s" % (H, F, regime, worst))


def _keep(s, H, p, transposed=False):
    """The dropout decisions of a sub-pattern's entries, from their GLOBAL (row, column)."""
    from test_dot_attention_host import keep_mask

    P = {"rows": s.rows.astype(np.int64) + s.r0, "colind": s.colind.astype(np.int64) + s.c0}
    return keep_mask(P, H, p, transposed)


def _seed():
    return torch.from_numpy(np.array(DROPOUT_SEED, dtype=np.uint32).view(np.int32)).to(DEV)


@pytest.mark.parametrize("p", (0.0, 0.25))
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_dot_attention_three_launches(pkg, H, F, regime, p):
    from gespmm_amd import _lib, attention
    from test_dot_attention_host import ratio, ref_backward, ref_forward

    N, gen = H * F, _gen(24)
    lib = _lib.lib
    M, K = _sizes_b(N, regime, lambda m, k: lib.gespmm_dot_attention_f32(*[None] * 7, m, k, H, F, m * D, 0.5, None))
    if regime == "B":
        for f, n in ((lib.gespmm_dot_attention_backward_q_f32, 10), (lib.gespmm_dot_attention_backward_kv_f32, 10)):
            assert f(*[None] * n, M, K, H, F, M * D, 0.5, None) == EINVAL and f(*[None] * n, M, K + 1, H, F, M * D, 0.5, None) == ERANGE
    _need(96)
    g = _band(M)
    rw, _ = _windows(g, N, spread=2)
    subs = _subs(g, rw)
    assert _lib.describe_dot_attention(M, K, H, F, g.nnz)["V"] == 4
    q, k, v = _uniform(gen, (M, H, F), -1, 1), _uniform(gen, (K, H, F), -1, 1), _uniform(gen, (K, H, F), -1, 1)
    go = _uniform(gen, (M, H, F), 0.5, 1)
    scale = float(np.float32(1.0 / np.sqrt(F)))
    drop = (p, _seed()) if p else None
    out, gq, gk, gv = _nan((M, H, F)), _nan((M, H, F)), _nan((K, H, F)), _nan((K, H, F))
    stats, delta = _nan((M, H, 2)), _nan((M, H))
    attention.dot_attention(g.rowptr, g.colind, q, k, v, scale=scale, dropout=drop, out=out, stats=stats)
    attention.dot_attention_backward_q(g.rowptr, g.colind, q, k, v, stats, out, go, scale=scale, dropout=drop, results=(delta, gq))
    attention.dot_attention_backward_kv(g.colptr, g.rowind, q, k, v, stats, delta, go, scale=scale, dropout=drop, results=(gk, gv))
    _written(out=out, stats=stats, delta=delta, grad_q=gq, grad_k=gk, grad_v=gv)
    worst = {}
    for s in subs:
        x = {"q": s.row_nodes(q), "k": s.col_nodes(k), "v": s.col_nodes(v), "go": s.row_nodes(go), "scale": scale}
        keep, ks = _keep(s, H, p) if p else (None, None)
        st, o, dl = s.row_nodes(stats), s.row_nodes(out), s.row_nodes(delta)
        f = ref_forward(s.P, x, keep, ks)
        b = ref_backward(s.P, x, st, o, None, keep, ks)
        bc = ref_backward(s.P, x, st, o, dl, keep, ks)
        r = {"out": ratio(o, f["out"], f["tol_out"]), "m": ratio(st[..., 0], f["m"], f["tol_m"]), "l": ratio(st[..., 1], f["l"], f["tol_l"]),
             "delta": ratio(dl, b["delta"], b["tol_delta"]), "grad_q": ratio(s.row_nodes(gq), b["grad_q"], b["tol_grad_q"]),
             "grad_k": ratio(s.full_cols(gk), bc["grad_k"][s.full], bc["tol_grad_k"][s.full]),
             "grad_v": ratio(s.full_cols(gv), bc["grad_v"][s.full], bc["tol_grad_v"][s.full])}
        assert max(r.values()) <= 1.0, ("rows %d .. %d" % (s.r0, s.r1), r)
        worst = {k_: max(v_, worst.get(k_, 0.0)) for k_, v_ in r.items()}
    print("dot attention H=%d F=%d regime %s p=%g: worst error / tolerance %s" % (H, F, regime, p, worst))


@pytest.mark.parametrize("p", (0.0, 0.25))
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_gat_backward_el_and_er(pkg, H, F, regime, p):
    from attention_refs import bound_ratio, gat_backward_float64
    from gespmm_amd import _lib, softmax

    N, slope, gen = H * F, 0.2, _gen(25)
    lib = _lib.lib
    M, K = _sizes_b(N, regime, lambda m, k: lib.gespmm_gat_backward_el_f32(*[None] * 9, m, k, H, F, m * D, slope, None))
    if regime == "B":
        assert lib.gespmm_gat_backward_er_f32(*[None] * 9, M, K, H, F, M * D, slope, None) == EINVAL
        assert lib.gespmm_gat_backward_er_f32(*[None] * 9, M, K + 1, H, F, M * D, slope, None) == ERANGE
    _need(48)
    g = _band(M)
    rw, _ = _windows(g, N, spread=2)
    subs = _subs(g, rw)
    el, er = _uniform(gen, (M, H), -2, 2), _uniform(gen, (K, H), -2, 2)
    gout, feat = _uniform(gen, (M, H, F), -1, 1), _uniform(gen, (K, H, F), -1, 1)
    drop = (p, _seed()) if p else None
    stats = softmax.gat_softmax_stats(g.rowptr, g.colind, el, er, negative_slope=slope, out=_nan((M, H, 2)))
    delta, gel = softmax.gat_backward_el(g.rowptr, g.colind, el, er, stats, gout, feat, negative_slope=slope, out=(_nan((M, H)), _nan((M, H))),
                                         dropout=drop)
    ger = softmax.gat_backward_er(g.colptr, g.rowind, el, er, stats, delta, gout, feat, negative_slope=slope, out=_nan((K, H)), dropout=drop)
    _written(stats=stats, delta=delta, grad_el=gel, grad_er=ger)
    worst = [0.0, 0.0]
    for s in subs:
        keep, ks = _keep(s, H, p) if p else (None, None)
        ref_el, ref_er, sc_el, sc_er = gat_backward_float64(s.rows, s.colind, s.M, s.K, s.row_nodes(el), s.col_nodes(er), s.row_nodes(gout),
                                                            s.col_nodes(feat), slope, keep, ks)
        re_, ok_el = bound_ratio(s.row_nodes(gel), ref_el, sc_el)
        rr_, ok_er = bound_ratio(s.full_cols(ger), ref_er[s.full], sc_er[s.full])
        assert ok_el and ok_er, ("rows %d .. %d" % (s.r0, s.r1), re_, rr_)
        worst = [max(worst[0], re_), max(worst[1], rr_)]
    print("gat backward H=%d F=%d regime %s p=%g: worst error / bound grad_el %.3f grad_er %.3f" % (H, F, regime, p, *worst))


# ---- c. the fused GATv2 attention (gatv2_attention.hip) and the 16-bit GATv2 score (gatv2_score_x16.hip): int positions, as section b ----

def _off(shape, offset, gen=None, lo_=0.0, hi=1.0):
    """A contiguous fp32 tensor carved from ONE allocation, its first byte ``offset`` bytes past a 16-byte boundary (0: the allocation
    itself) — seeded uniform values drawn in place, or NaN (test_gpu_gatv2_attention._carved at node size)."""
    n = int(np.prod(shape))
    buf = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[offset // 4:offset // 4 + n].view(shape)
    assert t.data_ptr() % 16 == offset and t.is_contiguous()
    return t.uniform_(lo_, hi, generator=gen) if gen is not None else t.fill_(float("nan"))


def _gatv2_attention_case(H, F, regime, p, offset):
    from gespmm_amd import _lib, attention, sddmm
    from test_dot_attention_host import ratio
    from test_gatv2_attention_host import ref_backward, ref_forward

    N, slope, gen = H * F, 0.2, _gen(26)
    lib = _lib.lib
    M, K = _sizes_b(N, regime, lambda m, k: lib.gespmm_gatv2_attention_f32(*[None] * 7, m, k, H, F, m * D, slope, None))
    if regime == "B":
        for f, n in ((lib.gespmm_gatv2_attention_backward_row_f32, 11), (lib.gespmm_gatv2_attention_backward_col_f32, 9)):
            assert f(*[None] * n, M, K, H, F, M * D, slope, None) == EINVAL and f(*[None] * n, M, K + 1, H, F, M * D, slope, None) == ERANGE
    _need(88)  # seven node arrays of 8 GB in regime B, the score array of the stats check, the band
    g = _band(M)
    rw, _ = _windows(g, N, spread=2)
    subs = _subs(g, rw)
    align, geo = (16, {"V": 4}) if offset == 0 else (4, {"V": 1})
    assert _lib.describe_gatv2_attention(M, K, H, F, g.nnz, align, align, align) == dict(geo, W=8 if F == 64 else 16, supported=True)
    xl, xr = _off((M, H, F), offset, gen, -1, 1), _off((K, H, F), offset, gen, -1, 1)
    go = _off((M, H, F), offset, gen, 0.5, 1)
    att = _off((H, F), offset, gen, -2, 2).mul_(min(1.0, 8.0 / F))
    drop = (p, _seed()) if p else None
    out, gxl, part, gxr = _off((M, H, F), offset), _off((M, H, F), offset), _off((M, H, F), offset), _off((K, H, F), offset)
    stats, delta = _nan((M, H, 2)), _off((M, H), offset)
    attention.gatv2_attention(g.rowptr, g.colind, xl, xr, att, negative_slope=slope, dropout=drop, out=out, stats=stats)
    attention.gatv2_attention_backward_row(g.rowptr, g.colind, xl, xr, att, stats, out, go, negative_slope=slope, dropout=drop,
                                           results=(delta, gxl, part))
    attention.gatv2_attention_backward_col(g.colptr, g.rowind, xl, xr, att, stats, delta, go, negative_slope=slope, dropout=drop, result=gxr)
    _written(out=out, stats=stats, delta=delta, grad_xl=gxl, att_part=part, grad_xr=gxr)
    score = sddmm.gatv2_score(g.rowptr, g.colind, xl, xr, att, negative_slope=slope, out=_nan((g.nnz, H)))  # the same operands: one (V, W)
    att_h, worst = att.cpu().numpy(), {}
    for s in subs:
        x = {"xl": s.row_nodes(xl), "xr": s.col_nodes(xr), "att": att_h, "go": s.row_nodes(go)}
        keep, ks = _keep(s, H, p) if p else (None, None)
        st, o, dl = s.row_nodes(stats), s.row_nodes(out), s.row_nodes(delta)
        top = s.edges(score).reshape(s.M, D, H).max(1)
        assert st[..., 0].tobytes() == top.tobytes(), "rows %d .. %d: m is not the row maximum of gatv2_score, bit for bit" % (s.r0, s.r1)
        f = ref_forward(s.P, x, slope, keep, ks)
        b = ref_backward(s.P, x, slope, st, o, None, keep, ks)
        bc = ref_backward(s.P, x, slope, st, o, dl, keep, ks)
        r = {"out": ratio(o, f["out"], f["tol_out"]), "m": ratio(st[..., 0], f["m"], f["tol_m"]), "l": ratio(st[..., 1], f["l"], f["tol_l"]),
             "delta": ratio(dl, b["delta"], b["tol_delta"]), "grad_xl": ratio(s.row_nodes(gxl), b["grad_xl"], b["tol_grad_xl"]),
             "att_part": ratio(s.row_nodes(part), b["att_part"], b["tol_att_part"]),
             "grad_xr": ratio(s.full_cols(gxr), bc["grad_xr"][s.full], bc["tol_grad_xr"][s.full])}
        assert max(r.values()) <= 1.0, ("rows %d .. %d" % (s.r0, s.r1), r)
        worst = {k_: max(v_, worst.get(k_, 0.0)) for k_, v_ in r.items()}
    print("gatv2 attention H=%d F=%d regime %s p=%g offset %d: worst error / tolerance %s" % (H, F, regime, p, offset, worst))


@pytest.mark.parametrize("p", (0.0, 0.25))
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_gatv2_attention_three_launches(pkg, H, F, regime, p):
    """gatv2_attention and its two backward passes: float64 with the tolerances of test_gatv2_attention_host.py on the sub-patterns,
    m of the stats on the bits of the row maximum of sddmm.gatv2_score run on the whole operands."""
    _gatv2_attention_case(H, F, regime, p, 0)


def test_gatv2_attention_three_launches_four_bytes_off(pkg):
    """(3, 100) at the largest sizes with every dense operand and result 4 bytes off a 16-byte boundary: the V = 1 kernels."""
    _gatv2_attention_case(3, 100, "B", 0.0, 4)


def _bits_equal(a, b, what):
    """Two whole arrays on bits, 2^28 elements at a time (no temporary of the arrays' size)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    x, y = a.reshape(-1).view(view), b.reshape(-1).view(view)
    for i in range(0, x.numel(), 1 << 28):
        bad = int((x[i:i + (1 << 28)] != y[i:i + (1 << 28)]).sum())
        assert bad == 0, "%s: %d elements differ among the elements %d .. %d" % (what, bad, i, min(i + (1 << 28), x.numel()))


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16), ids=("bf16", "fp16"))
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("H,F", lo.WIDTHS, ids=WIDTH_IDS)
def test_gatv2_score_x16_forward_and_both_backward_passes(pkg, H, F, regime, dtype):
    """The limit counts ELEMENTS: regime A has more than 2^30 of them in every 16-bit operand (byte 2^31 inside), regime B ends just
    below byte 2^32, and the fp32 att_part is 5.4 / 8 GB. The oracle is the fp32 backward on the exact widening over the WHOLE arrays:
    att_part on its bits, grad_x on the bits of its result narrowed once; the score on the fp32 kernel's bits where both describe
    calls answer one (V, W), and inside the float64 bound on the sub-patterns."""
    from gespmm_amd import _lib, sddmm
    from test_gatv2_host import restate_score, worst_ratio

    N, slope, gen = H * F, 0.2, _gen(27)
    lib, code = _lib.lib, (_lib.X16_BF16 if dtype == torch.bfloat16 else _lib.X16_F16)
    M, K = _sizes_b(N, regime, lambda m, k: lib.gespmm_gatv2_score_x16(*[None] * 6, code, m, k, H, F, m * D, slope, None))
    if regime == "B":  # the column pass: S = K segments, T = M rows
        assert lib.gespmm_gatv2_score_backward_x16(*[None] * 9, code, K, M, H, F, M * D, slope, None) == EINVAL
        assert lib.gespmm_gatv2_score_backward_x16(*[None] * 9, code, K + 1, M, H, F, M * D, slope, None) == ERANGE
        assert (1 << 32) - 2 * N - 8192 <= K * N * 2 < (1 << 32), "the 16-bit K-side operands end just below byte 2^32"
    assert M * N > (1 << 30), "byte 2^31 lies inside every 16-bit operand"
    _need(72)
    g = _band(M)
    rw, _ = _windows(g, N, 2, spread=2)
    subs = _subs(g, rw)
    xl, xr = _uniform(gen, (M, H, F), -1, 1).to(dtype), _uniform(gen, (K, H, F), -1, 1).to(dtype)
    att, gsc = _uniform(gen, (H, F), -2, 2), _uniform(gen, (g.nnz, H), -2, 2)
    score = sddmm.gatv2_score_x16(g.rowptr, g.colind, xl, xr, att, negative_slope=slope, out=_nan((g.nnz, H)))
    gxl, part = sddmm.gatv2_score_backward_x16(g.rowptr, g.colind, gsc, xl, xr, att, negative_slope=slope, want_att_part=True,
                                               out=(_nan((M, H, F), dtype), _nan((M, H, F))))
    gxr = sddmm.gatv2_score_backward_x16(g.colptr, g.rowind, gsc, xr, xl, att, negative_slope=slope, order=g.order32, out=_nan((K, H, F), dtype))
    _written(score=score, grad_xl=gxl, att_part=part, grad_xr=gxr)
    # ---- the score inside the float64 bound on the sub-patterns
    att_h, worst = att.cpu().numpy(), 0.0
    for s in subs:
        xl_h, xr_h = xl[s.r0:s.r1].float().cpu().numpy(), xr[s.c0:s.c1].float().cpu().numpy()
        ref, terms = restate_score(s.rowptr, s.colind, xl_h, xr_h, att_h, slope)
        r = worst_ratio(s.edges(score), ref, terms, "score")
        assert r <= 1.0, ("rows %d .. %d" % (s.r0, s.r1), r)
        worst = max(worst, r)
    print("gatv2 x16 H=%d F=%d regime %s %s: score worst error / bound %.4g" % (H, F, regime, dtype, worst))
    # ---- the fp32 kernels on the exact widening, whole arrays
    wl, wr = xl.float(), xr.float()
    # On 16-byte aligned operands the two kernels do NOT share a lane order at these widths — (8, 64): (V, W) = (8, 4) on 16-bit operands,
    # (4, 8) on fp32; (3, 100): (4, 8) and (4, 16) — so the score above has the float64 bound alone. With att 4 bytes off a 16-byte
    # boundary (a tensor of H F floats: nothing node-sized is copied) both resolve to V = 1 at one W, asserted from the two describe
    # calls, and the 16-bit score of the whole pattern must have the fp32 kernel's bits.
    d16, d32 = _lib.describe_gatv2_score(M, g.nnz, H, F, x16=True), _lib.describe_gatv2_score(M, g.nnz, H, F)
    assert (d16["V"], d16["W"]) == {(8, 64): (8, 4), (3, 100): (4, 8)}[(H, F)] and (d32["V"], d32["W"]) == (4, 8 if F == 64 else 16)
    d16, d32 = _lib.describe_gatv2_score(M, g.nnz, H, F, 16, 16, 4, x16=True), _lib.describe_gatv2_score(M, g.nnz, H, F, 16, 16, 4)
    assert (d16["V"], d16["W"]) == (d32["V"], d32["W"]) == (1, 8 if F == 64 else 16), (d16, d32)
    att4 = _off((H, F), 4).copy_(att)
    _bits_equal(sddmm.gatv2_score_x16(g.rowptr, g.colind, xl, xr, att4, negative_slope=slope, out=score.fill_(float("nan"))),
                sddmm.gatv2_score(g.rowptr, g.colind, wl, wr, att4, negative_slope=slope, out=_nan((g.nnz, H))),
                "score against the fp32 kernel at (V, W) = (1, %d)" % d16["W"])
    _written(score=score)
    del score
    gxl32, part32 = sddmm.gatv2_score_backward(g.rowptr, g.colind, gsc, wl, wr, att, negative_slope=slope, want_att_part=True)
    _bits_equal(part, part32, "att_part against the fp32 backward on the widened operands")
    del part, part32
    _bits_equal(gxl, gxl32.to(dtype), "grad_xl against the fp32 backward's result, narrowed once")
    del gxl, gxl32
    gxr32 = sddmm.gatv2_score_backward(g.colptr, g.rowind, gsc, wr, wl, att, negative_slope=slope, order=g.order32)
    _bits_equal(gxr, gxr32.to(dtype), "grad_xr against the fp32 backward's result, narrowed once")
