"""The max reducer with argmax (spmm.csr_spmm_max_arg) and its gradient (spmm.csr_spmm_max_backward) on the device, bit for bit against
the host restatement of the two chains (tests/max_arg_ref.py).

The graph (301 rows over 257 nodes) holds what the walk can trip over: empty rows (the first and the last among them), rows of one
entry, one row each of 63, 64, 65, 130 and 700 entries (below, at and beyond one and two LDS tiles, and beyond a wavefront's whole range),
repeated (row, column) entries, unsorted columns, and a row count no rows-per-wavefront divides. Operands: (i) integers in -2 .. 2 (ties
everywhere: the first-position rule is witnessed), (ii) random floats with planted +0, -0, NaN and values below empty_value,
(iii) graphs.reference_B. CASES names every (width, operand offset) pair run; test_every_built_instantiation_is_reached proves through
_lib.max_arg_route that together they reach every (V, S, W) the launch table builds — (4, 2, 64) needs >= 2^17 segments and is reached
by the block-diagonal repetition of the same graph, whose expected result is the small one's, repeated."""
import functools

import numpy as np
import pytest
import torch

from max_arg_ref import max_arg_forward, max_backward, tied_words, transpose

pytestmark = pytest.mark.gpu

M0, K0 = 301, 257
EMPTIES = (-10000.0, 0.0, float("-inf"))
# the issue's widths, and 8 and 16 for the two lane groups between 4 and 32 lanes per row
WIDTHS = (1, 3, 4, 8, 16, 20, 47, 64, 128, 130, 256, 260, 602)
# (N, offset in floats of B / out / arg inside their allocations): 1 -> 4-byte aligned, 2 -> 8-byte aligned
CASES = tuple((N, 0) for N in WIDTHS) + ((128, 1), (128, 2), (130, 2), (260, 1), (602, 2))
BUILT = {(1, 1, 4), (1, 1, 8), (1, 1, 16), (1, 1, 32), (1, 1, 64), (4, 1, 32), (4, 1, 64), (4, 2, 64), (2, 1, 64), (2, 2, 64), (1, 2, 64)}
BIG_N, BIG_REPS = 260, 511  # 511 x 257 = 131327 >= 2^17 nodes, 511 x 301 rows


@functools.lru_cache(maxsize=None)
def graph(dedup=False):
    rng = np.random.default_rng(20260)
    deg = rng.integers(0, 13, size=M0)
    deg[[0, 5, 6, 100, M0 - 1]] = 0
    deg[[1, 2, 50, M0 - 2]] = 1
    for r, d in ((10, 63), (11, 64), (12, 65), (40, 130), (200, 700)):
        deg[r] = d
    rows = [rng.integers(0, K0, size=d) for d in deg]
    rows[20] = np.array([7, 7, 3, 7, 3])          # repeated (row, column) entries in a short row
    rows[21] = np.array([K0 - 1, 0, K0 - 1])
    if dedup:
        rows = [r[np.sort(np.unique(r, return_index=True)[1])] for r in rows]
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    colind = np.concatenate(rows).astype(np.int32)
    if not dedup:
        assert len(rows[200]) == 700 and any(len(np.unique(r)) < len(r) for r in rows)
    colptr, rowind, order = transpose(rowptr, colind, K0)
    return dict(rowptr=rowptr, colind=colind, colptr=colptr, rowind=rowind, order=order, nnz=len(colind))


@functools.lru_cache(maxsize=None)
def operand(kind, N, empty_value=-10000.0):
    rng = np.random.default_rng(1000 * N + len(kind))
    if kind == "ints":
        return rng.integers(-2, 3, size=(K0, N)).astype(np.float32)
    if kind == "floats":
        B = rng.standard_normal((K0, N)).astype(np.float32)
        low = np.float32(-20000.0) if np.isfinite(empty_value) and empty_value < 0 else np.float32(-1.5)
        for value, share in ((np.float32(0.0), 0.04), (np.float32(-0.0), 0.04), (np.float32("nan"), 0.04), (low, 0.04)):
            B[rng.random((K0, N)) < share] = value
        return B
    from gespmm_amd import graphs

    return graphs.reference_B(K0, N, seed=3).numpy()


@functools.lru_cache(maxsize=None)
def forward_ref(kind, N, empty_value):
    g = graph()
    return max_arg_forward(g["rowptr"], g["colind"], operand(kind, N, empty_value), empty_value)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _view(n_rows, N, off, dtype, fill):
    """A contiguous [n_rows, N] view that starts `off` elements into its allocation."""
    buf = torch.full((n_rows * N + off,), fill, dtype=dtype, device="cuda")
    return buf[off:].view(n_rows, N)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _gdev():
    g = graph()
    return {k: _dev(v) for k, v in g.items() if k != "nnz"}


def test_every_built_instantiation_is_reached(pkg):
    from gespmm_amd import _lib

    g = graph()
    reached_fwd, reached_bwd = set(), set()
    for N, off in CASES:
        align = {0: 16, 1: 4, 2: 8}[off]
        reached_fwd.add(_lib.max_arg_route(M0, g["nnz"], N, align, align))
        reached_bwd.add(_lib.max_arg_route(K0, g["nnz"], N, align, align))
    reached_fwd.add(_lib.max_arg_route(M0 * BIG_REPS, g["nnz"] * BIG_REPS, BIG_N))
    reached_bwd.add(_lib.max_arg_route(K0 * BIG_REPS, g["nnz"] * BIG_REPS, BIG_N))
    assert reached_fwd == BUILT and reached_bwd == BUILT, (BUILT - reached_fwd, BUILT - reached_bwd)


def test_the_integer_operand_witnesses_the_first_position_rule():
    g = graph()
    for N in (4, 64, 130):
        B = operand("ints", N)
        C, arg = forward_ref("ints", N, -10000.0)
        tied = tied_words(g["rowptr"], g["colind"], B, C, arg)
        assert tied.mean() >= 0.25, (N, tied.mean())


@pytest.mark.parametrize("N,off", CASES)
def test_forward_and_backward_equal_the_restatement(pkg, N, off):
    from gespmm_amd import _lib, spmm

    g, d = graph(), _gdev()
    align = {0: 16, 1: 4, 2: 8}[off]
    rng = np.random.default_rng(N + off)
    grad_h = rng.standard_normal((M0, N)).astype(np.float32)
    grad = _view(M0, N, off, torch.float32, 0.0)
    grad.copy_(_dev(grad_h))
    for kind in ("ints", "floats", "reference"):
        for empty in EMPTIES:
            B_h = operand(kind, N, empty)
            want_C, want_arg = forward_ref(kind, N, empty)
            B = _view(K0, N, off, torch.float32, 0.0)
            B.copy_(_dev(B_h))
            out = _view(M0, N, off, torch.float32, float("nan"))
            arg = _view(M0, N, off, torch.int32, -7)
            assert B.data_ptr() % 16 == (4 * off) % 16 and out.data_ptr() % 16 == (4 * off) % 16 and arg.data_ptr() % 16 == (4 * off) % 16
            got = spmm.csr_spmm_max_arg(d["rowptr"], d["colind"], B, empty_value=empty, out=out, arg=arg)
            assert got[0] is out and got[1] is arg
            assert np.array_equal(arg.cpu().numpy(), want_arg), (N, off, kind, empty, _lib.max_arg_route(M0, g["nnz"], N, align, align))
            assert np.array_equal(_bits(out), want_C.view(np.uint32)), (N, off, kind, empty)
            if empty != EMPTIES[0] and kind != "floats":
                continue  # the gradient once per arg array of (i) - (iii), and for every empty_value on (ii)
            want_grad = max_backward(g["colptr"], g["rowind"], g["order"], want_arg, grad_h, K0)
            gB = _view(K0, N, off, torch.float32, float("nan"))
            assert spmm.csr_spmm_max_backward(d["colptr"], d["rowind"], d["order"], arg, grad, K0, out=gB) is gB
            assert np.array_equal(_bits(gB), want_grad.view(np.uint32)), (N, off, kind, empty)
            again = spmm.csr_spmm_max_backward(d["colptr"], d["rowind"], d["order"], arg, grad, K0)
            assert np.array_equal(_bits(again), _bits(gB)), "two runs differ"
            unchosen = np.setdiff1d(np.arange(K0), g["colind"][want_arg[want_arg >= 0]])
            if unchosen.size:
                assert not _bits(gB)[unchosen].any(), "a node no row chose is not +0"
            terms = grad_h[want_arg >= 0].astype(np.float64)
            assert abs(gB.double().sum().item() - terms.sum()) <= 1e-4 * np.abs(terms).sum(), (N, off, kind, empty)


def test_c_has_the_bits_of_csr_spmm_max_where_no_zeros_compete(pkg):
    from gespmm_amd import spmm

    d = _gdev()
    for N in (20, 64, 128, 260):
        B_h = operand("reference", N)
        C, _ = forward_ref("reference", N, -10000.0)
        zero_max = (C == 0)
        if zero_max.any():  # a maximum of zero must come from zeros of one sign: reference_B holds +0 only
            assert not np.signbit(B_h[B_h == 0]).any()
        B = _dev(B_h)
        out, _ = spmm.csr_spmm_max_arg(d["rowptr"], d["colind"], B)
        assert np.array_equal(_bits(out), _bits(spmm.csr_spmm_max(d["rowptr"], d["colind"], B))), N


def test_no_entries_and_no_rows(pkg):
    from gespmm_amd import spmm

    rowptr = torch.zeros(M0 + 1, dtype=torch.int32, device="cuda")
    none = torch.empty(0, dtype=torch.int32, device="cuda")
    for N in (3, 130):
        B = torch.randn(K0, N, device="cuda")
        out, arg = spmm.csr_spmm_max_arg(rowptr, none, B, empty_value=-3.5)
        assert (out == -3.5).all().item() and (arg == -1).all().item() and out.shape == (M0, N) and arg.dtype == torch.int32
        colptr = torch.zeros(K0 + 1, dtype=torch.int32, device="cuda")
        gB = torch.full((K0, N), float("nan"), device="cuda")
        spmm.csr_spmm_max_backward(colptr, none, none, arg, torch.randn(M0, N, device="cuda"), K0, out=gB)
        assert not _bits(gB).any()
    out, arg = spmm.csr_spmm_max_arg(torch.zeros(1, dtype=torch.int32, device="cuda"), none, torch.randn(K0, 8, device="cuda"))
    assert out.shape == (0, 8) and arg.shape == (0, 8)


def test_gradient_equals_an_index_add_composition(pkg):
    """(ii) on the graph without its repeated entries — a repeated entry that holds the maximum IS a tie — and without zeros in play:
    no output word has two equal candidates (asserted), so the gradient is that of the max as a function, here a float64 index_add_ of
    grad_out at colind[arg]."""
    from gespmm_amd import spmm

    g = graph(dedup=True)
    d = {k: _dev(v) for k, v in g.items() if k != "nnz"}
    for N in (20, 130):
        rng = np.random.default_rng(7 + N)
        B_h = rng.standard_normal((K0, N)).astype(np.float32)
        B_h[rng.random((K0, N)) < 0.04] = np.float32("nan")
        B_h[rng.random((K0, N)) < 0.04] = np.float32(-20000.0)
        C, arg_h = max_arg_forward(g["rowptr"], g["colind"], B_h, -10000.0)
        assert not tied_words(g["rowptr"], g["colind"], B_h, C, arg_h).any()
        grad = torch.randn(M0, N, device="cuda")
        out, arg = spmm.csr_spmm_max_arg(d["rowptr"], d["colind"], _dev(B_h))
        assert np.array_equal(arg.cpu().numpy(), arg_h)
        gB = spmm.csr_spmm_max_backward(d["colptr"], d["rowind"], d["order"], arg, grad, K0)
        won = arg >= 0
        node = d["colind"].long()[arg.long().clamp(min=0)]
        flat = (node * N + torch.arange(N, device="cuda")).masked_select(won)
        terms = grad.double().masked_select(won)
        ref = torch.zeros(K0 * N, dtype=torch.float64, device="cuda").index_add_(0, flat, terms)
        bound = torch.zeros(K0 * N, dtype=torch.float64, device="cuda").index_add_(0, flat, terms.abs())
        assert ((gB.double().view(-1) - ref).abs() <= 1e-4 * bound).all().item(), N


def test_the_repeated_graph_reaches_two_strips_of_four(pkg):
    """511 copies of the graph on the diagonal: >= 2^17 rows and nodes, the (4, 2, 64) instantiation in both directions. Everything is
    built on the device from the small arrays; the expected result is the small one's, repeated, positions shifted per copy."""
    from gespmm_amd import _lib, spmm

    g, d, R, N = graph(), _gdev(), BIG_REPS, BIG_N
    nnz = g["nnz"]
    assert _lib.max_arg_route(M0 * R, nnz * R, N) == (4, 2, 64) and _lib.max_arg_route(K0 * R, nnz * R, N) == (4, 2, 64)
    rep = torch.arange(R, device="cuda", dtype=torch.int32)

    def ptr(p):
        return torch.cat([(p[:-1].view(1, -1) + rep.view(-1, 1) * nnz).reshape(-1), torch.tensor([nnz * R], dtype=torch.int32, device="cuda")])

    def shifted(x, step):
        return (x.view(1, -1) + rep.view(-1, 1) * step).reshape(-1).contiguous()

    rowptr, colptr = ptr(d["rowptr"]), ptr(d["colptr"])
    colind, rowind, order = shifted(d["colind"], K0), shifted(d["rowind"], M0), shifted(d["order"], nnz)
    B_h = operand("ints", N)
    want_C, want_arg = forward_ref("ints", N, -10000.0)
    grad_h = np.random.default_rng(5).standard_normal((M0, N)).astype(np.float32)
    want_grad = max_backward(g["colptr"], g["rowind"], g["order"], want_arg, grad_h, K0)
    out, arg = spmm.csr_spmm_max_arg(rowptr, colind, _dev(B_h).repeat(R, 1))
    assert torch.equal(out.view(R, M0, N).view(torch.int32), _dev(want_C).view(torch.int32).expand(R, M0, N))
    wa = _dev(want_arg)
    want_big = torch.where(wa >= 0, wa.view(1, M0, N) + (rep * nnz).view(R, 1, 1), wa.view(1, M0, N).expand(R, M0, N))
    assert torch.equal(arg.view(R, M0, N), want_big)
    gB = spmm.csr_spmm_max_backward(colptr, rowind, order, arg, _dev(grad_h).repeat(R, 1), K0 * R)
    assert torch.equal(gB.view(R, K0, N).view(torch.int32), _dev(want_grad).view(torch.int32).expand(R, K0, N))


def test_python_errors_raise_before_any_launch(pkg):
    from gespmm_amd import spmm

    d = _gdev()
    N = 8
    B = torch.randn(K0, N, device="cuda")
    grad = torch.randn(M0, N, device="cuda")
    arg = torch.zeros(M0, N, dtype=torch.int32, device="cuda")
    fwd = lambda **kw: spmm.csr_spmm_max_arg(d["rowptr"], d["colind"], kw.pop("B", B), **kw)  # noqa: E731
    bwd = lambda **kw: spmm.csr_spmm_max_backward(d["colptr"], d["rowind"], kw.pop("order", d["order"]), kw.pop("arg", arg),  # noqa: E731
                                                  kw.pop("grad", grad), kw.pop("K", K0), **kw)
    for bad in (B.half(), B.bfloat16(), B.double()):
        with pytest.raises(TypeError):
            fwd(B=bad)
        with pytest.raises(TypeError):
            bwd(grad=grad.to(bad.dtype))
    with pytest.raises(TypeError):
        fwd(arg=torch.zeros(M0, N, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        bwd(order=d["order"].long())
    with pytest.raises(TypeError):
        bwd(arg=arg.long())
    for bad in (B[0], B.view(K0, N, 1)):  # rank
        with pytest.raises(ValueError):
            fwd(B=bad)
    with pytest.raises(ValueError):
        bwd(grad=grad[0])
    with pytest.raises(ValueError):  # non-contiguous
        fwd(B=torch.randn(N, K0, device="cuda").t())
    with pytest.raises(ValueError):
        bwd(grad=torch.randn(N, M0, device="cuda").t())
    with pytest.raises(ValueError):
        fwd(out=torch.empty(M0, 2 * N, device="cuda")[:, :N])
    for shape in ((M0, N + 1), (M0 + 1, N)):  # mismatched arg / out shapes
        with pytest.raises(ValueError):
            fwd(arg=torch.zeros(shape, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError):
            fwd(out=torch.zeros(shape, device="cuda"))
        with pytest.raises(ValueError):
            bwd(arg=torch.zeros(shape, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        bwd(K=K0 + 1)
    with pytest.raises(ValueError):
        bwd(order=d["order"][:-1])
    with pytest.raises(ValueError):
        bwd(out=torch.zeros(K0 + 1, N, device="cuda"))
    with pytest.raises(ValueError):
        fwd(empty_value=float("nan"))
    with pytest.raises(ValueError):  # a result on top of an input
        big = torch.randn(max(M0, K0), N, device="cuda")
        spmm.csr_spmm_max_arg(d["rowptr"], d["colind"], big[:K0], out=big[:M0])


def test_forward_and_backward_replay_from_a_graph(pkg):
    """Both kernels allocate nothing and never synchronise: captured once, replayed with new contents at the same addresses."""
    from gespmm_amd import spmm

    g, d, N = graph(), _gdev(), 64
    feat = _dev(operand("floats", N))
    grad = torch.randn(M0, N, device="cuda")
    out = torch.empty(M0, N, device="cuda")
    arg = torch.empty(M0, N, dtype=torch.int32, device="cuda")
    gB = torch.empty(K0, N, device="cuda")

    def step():
        spmm.csr_spmm_max_arg(d["rowptr"], d["colind"], feat, out=out, arg=arg)
        spmm.csr_spmm_max_backward(d["colptr"], d["rowind"], d["order"], arg, grad, K0, out=gB)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        step()
    for seed in (2, 3):
        feat.copy_(torch.randn(K0, N, generator=torch.Generator().manual_seed(seed)).cuda())
        for t in (out, gB):
            t.fill_(float("nan"))
        arg.fill_(-5)
        cg.replay()
        torch.cuda.synchronize()
        e_out, e_arg = spmm.csr_spmm_max_arg(d["rowptr"], d["colind"], feat)
        e_gB = spmm.csr_spmm_max_backward(d["colptr"], d["rowind"], d["order"], e_arg, grad, K0)
        assert torch.equal(arg, e_arg) and np.array_equal(_bits(out), _bits(e_out)) and np.array_equal(_bits(gB), _bits(e_gB)), seed
        want_C, want_arg = max_arg_forward(g["rowptr"], g["colind"], feat.cpu().numpy(), -10000.0)
        assert np.array_equal(arg.cpu().numpy(), want_arg) and np.array_equal(_bits(out), want_C.view(np.uint32))
