"""The max reducer with argmax and its gradient on fp16 / bf16 operands (spmm.csr_spmm_max_arg_x16 / csr_spmm_max_backward_x16) on the
device, bit for bit against the oracle: a max rounds nothing, so the forward is the fp32 restatement (tests/max_arg_ref.py) on the
exactly widened operand, narrowed once, with an identical arg; the backward is the fp32 add chain on the widened grad_out, narrowed once.
No tolerance anywhere.

Graph and operand kinds are those of tests/test_gpu_max_arg.py (301 rows over 257 nodes: empty rows, rows of 1, 63, 64, 65, 130 and 700
entries, repeated entries), the operands narrowed to the dtype. X16_CASES names every (width, offset of the 16-bit arrays in ELEMENTS,
offset of arg in words) run: 0 / 1 / 2 / 4 elements are 16- / 2- / 4- / 8-byte aligned 16-bit arrays, 0 / 1 / 2 words a 16- / 4- / 8-byte
aligned arg; test_every_built_instantiation_is_reached proves through _lib.max_arg_route_x16 that together they reach every (V, S, W)
built, in both directions."""
import functools

import numpy as np
import pytest
import torch

from max_arg_ref import max_arg_forward, max_backward, tied_words
from test_gpu_max_arg import BIG_N, BIG_REPS, BUILT, EMPTIES, K0, M0, WIDTHS, graph, operand

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
X16_ALIGN = {0: 16, 1: 2, 2: 4, 4: 8}  # offset of B / out / grad in elements -> the alignment of their first element
ARG_ALIGN = {0: 16, 1: 4, 2: 8}        # offset of arg in words
# every effective alignment min(2 * x16, arg): 16 from (0, 0) and (4, 0), 8 from (2, 0), (0, 2) and (4, 2), 4 from (1, 0) and (0, 1)
OFFSETS = ((1, 0), (2, 0), (4, 0), (0, 1), (0, 2), (4, 2))
X16_CASES = (tuple((N, 0, 0) for N in WIDTHS) + tuple((N, xo, ao) for N in (128, 130, 260, 602) for xo, ao in OFFSETS)
             + ((3, 1, 1), (47, 1, 0), (256, 4, 0), (256, 2, 2)))
PAD = 8  # elements kept behind every view: what a store past the last row would hit


def _name(dt):
    return "f16" if dt == torch.float16 else "bf16"


def narrow(a, dt):
    """fp32 host array -> (16-bit torch tensor on the host: one rounding to nearest even; its exact fp32 widening as numpy)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt)
    return t, t.float().numpy()


@functools.lru_cache(maxsize=None)
def operand16(kind, N, empty_value, dt):
    return narrow(operand(kind, N, empty_value), dt)


@functools.lru_cache(maxsize=None)
def forward_ref(kind, N, empty_value, dt):
    """(C fp32 of the widened operand, its narrowing as a 16-bit tensor, arg)"""
    g = graph()
    C, arg = max_arg_forward(g["rowptr"], g["colind"], operand16(kind, N, empty_value, dt)[1], empty_value)
    return C, narrow(C, dt)[0], arg


@functools.lru_cache(maxsize=None)
def grad16(N, dt):
    return narrow(np.random.default_rng(77 + N).standard_normal((M0, N)), dt)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _view(n_rows, N, off, dtype, fill):
    """(allocation, contiguous [n_rows, N] view of it that starts `off` elements in and ends PAD elements before its end)"""
    buf = torch.full((off + n_rows * N + PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[off:off + n_rows * N].view(n_rows, N)


def _margins_untouched(buf, off, n, fill):
    m = torch.cat([buf[:off], buf[off + n:]])
    return bool((m == fill).all().item()) if fill == fill else bool(torch.isnan(m).all().item())


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gdev():
    g = graph()
    return {k: _dev(v) for k, v in g.items() if k != "nnz"}


def test_every_built_instantiation_is_reached(pkg):
    from gespmm_amd import _lib

    g = graph()
    reached_fwd, reached_bwd, effective = set(), set(), set()
    for N, xo, ao in X16_CASES:
        reached_fwd.add(_lib.max_arg_route_x16(M0, g["nnz"], N, X16_ALIGN[xo], ARG_ALIGN[ao]))
        reached_bwd.add(_lib.max_arg_route_x16(K0, g["nnz"], N, X16_ALIGN[xo], ARG_ALIGN[ao]))
        effective.add((min(2 * X16_ALIGN[xo], ARG_ALIGN[ao], 16), X16_ALIGN[xo], ARG_ALIGN[ao]))
    reached_fwd.add(_lib.max_arg_route_x16(M0 * BIG_REPS, g["nnz"] * BIG_REPS, BIG_N))
    reached_bwd.add(_lib.max_arg_route_x16(K0 * BIG_REPS, g["nnz"] * BIG_REPS, BIG_N))
    assert reached_fwd == BUILT and reached_bwd == BUILT, (BUILT - reached_fwd, BUILT - reached_bwd)
    assert {e[0] for e in effective} == {4, 8, 16} and {e[1] for e in effective} == {2, 4, 8, 16} and {e[2] for e in effective} == {4, 8, 16}
    # V = 4 on 16-bit arrays that are only 8-byte aligned, and V narrowed by either side alone
    assert _lib.max_arg_route_x16(M0, g["nnz"], 128, 8, 16)[0] == 4 and _lib.max_arg_route_x16(M0, g["nnz"], 128, 4, 16)[0] == 2
    assert _lib.max_arg_route_x16(M0, g["nnz"], 128, 16, 8)[0] == 2 and _lib.max_arg_route_x16(M0, g["nnz"], 128, 16, 4)[0] == 1


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_the_integer_operand_witnesses_the_first_position_rule(dt):
    """A condition on the inputs, not a measurement: integers in -2 .. 2 are exact in both types, so the narrowed operand has the ties
    of the fp32 one — at least a quarter of the output words have a later entry equal to the winner."""
    g = graph()
    for N in (4, 64, 130):
        B16, Bw = operand16("ints", N, -10000.0, dt)
        assert np.array_equal(Bw, operand("ints", N))
        C, _, arg = forward_ref("ints", N, -10000.0, dt)
        tied = tied_words(g["rowptr"], g["colind"], Bw, C, arg)
        assert tied.mean() >= 0.25, (N, tied.mean())


@pytest.mark.parametrize("N,xo,ao", X16_CASES)
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_forward_and_backward_bits(pkg, dt, N, xo, ao):
    from gespmm_amd import _lib, spmm

    g, d = graph(), _gdev()
    route = _lib.max_arg_route_x16(M0, g["nnz"], N, X16_ALIGN[xo], ARG_ALIGN[ao])
    grad_t, grad_w = grad16(N, dt)
    _, grad = _view(M0, N, xo, dt, 0.0)
    grad.copy_(grad_t.cuda())
    for kind in ("ints", "floats", "reference"):
        for empty in EMPTIES:
            B_t, _ = operand16(kind, N, empty, dt)
            _, want_C16, want_arg = forward_ref(kind, N, empty, dt)
            _, B = _view(K0, N, xo, dt, 0.0)
            B.copy_(B_t.cuda())
            obuf, out = _view(M0, N, xo, dt, float("nan"))
            abuf, arg = _view(M0, N, ao, torch.int32, -7)
            for t in (B, out, grad):
                assert t.data_ptr() % 16 == (2 * xo) % 16
            assert arg.data_ptr() % 16 == (4 * ao) % 16
            got = spmm.csr_spmm_max_arg_x16(d["rowptr"], d["colind"], B, empty_value=empty, out=out, arg=arg)
            assert got[0] is out and got[1] is arg
            where = (_name(dt), N, xo, ao, kind, empty, route)
            assert np.array_equal(arg.cpu().numpy(), want_arg), where
            assert np.array_equal(_bits(out), _bits(want_C16)), where
            assert _margins_untouched(obuf, xo, M0 * N, float("nan")) and _margins_untouched(abuf, ao, M0 * N, -7), where
            out2, arg2 = spmm.csr_spmm_max_arg_x16(d["rowptr"], d["colind"], B, empty_value=empty)
            assert torch.equal(arg2, arg) and np.array_equal(_bits(out2), _bits(out)), "two runs differ"
            if empty != EMPTIES[0] and kind != "floats":
                continue  # the gradient once per arg array of the three kinds, and for every empty_value on the floats
            want_grad = narrow(max_backward(g["colptr"], g["rowind"], g["order"], want_arg, grad_w, K0), dt)[0]
            gbuf, gB = _view(K0, N, xo, dt, float("nan"))
            assert spmm.csr_spmm_max_backward_x16(d["colptr"], d["rowind"], d["order"], arg, grad, K0, out=gB) is gB
            assert np.array_equal(_bits(gB), _bits(want_grad)), where
            assert _margins_untouched(gbuf, xo, K0 * N, float("nan")), where
            again = spmm.csr_spmm_max_backward_x16(d["colptr"], d["rowind"], d["order"], arg, grad, K0)
            assert np.array_equal(_bits(again), _bits(gB)), "two runs differ"
            unchosen = np.setdiff1d(np.arange(K0), g["colind"][want_arg[want_arg >= 0]])
            if unchosen.size:
                assert not _bits(gB)[unchosen].any(), "a node no row chose is not +0"


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_an_empty_value_the_type_cannot_hold(pkg, dt):
    """-10000 is no bf16 value: it is compared exactly (a bf16 -9984 wins over it, -10048 does not) and narrowed only where a row keeps it."""
    from gespmm_amd import spmm

    rowptr = torch.tensor([0, 1, 2, 2], dtype=torch.int32, device="cuda")
    colind = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    B = torch.tensor([[-9984.0] * 3, [-10048.0] * 3], device="cuda").to(dt)
    assert B.float()[0, 0].item() == -9984.0 and B.float()[1, 0].item() == -10048.0  # both are fp16 and bf16 values
    out, arg = spmm.csr_spmm_max_arg_x16(rowptr, colind, B, empty_value=-10000.0)
    kept = torch.tensor(-10000.0).to(dt)
    assert arg.tolist() == [[0] * 3, [-1] * 3, [-1] * 3]
    assert out[0].float().tolist() == [-9984.0] * 3 and (out[1:].view(torch.int16) == kept.view(torch.int16)).all().item()
    assert kept.float().item() == (-10000.0 if dt == torch.float16 else -9984.0)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_degenerate_sizes(pkg, dt):
    from gespmm_amd import spmm

    rowptr = torch.zeros(M0 + 1, dtype=torch.int32, device="cuda")
    none = torch.empty(0, dtype=torch.int32, device="cuda")
    for N in (3, 130):
        B = torch.randn(K0, N, device="cuda").to(dt)
        out, arg = spmm.csr_spmm_max_arg_x16(rowptr, none, B, empty_value=-3.5)
        assert out.dtype == dt and (out == -3.5).all().item() and (arg == -1).all().item() and out.shape == (M0, N) and arg.dtype == torch.int32
        colptr = torch.zeros(K0 + 1, dtype=torch.int32, device="cuda")
        gB = torch.full((K0, N), float("nan"), device="cuda", dtype=dt)
        spmm.csr_spmm_max_backward_x16(colptr, none, none, arg, torch.randn(M0, N, device="cuda").to(dt), K0, out=gB)
        assert not _bits(gB).any()
    out, arg = spmm.csr_spmm_max_arg_x16(torch.zeros(1, dtype=torch.int32, device="cuda"), none, torch.randn(K0, 8, device="cuda").to(dt))
    assert out.shape == (0, 8) and arg.shape == (0, 8) and out.dtype == dt
    d = _gdev()
    out, arg = spmm.csr_spmm_max_arg_x16(d["rowptr"], d["colind"], torch.empty(K0, 0, device="cuda", dtype=dt))
    assert out.shape == (M0, 0) and arg.shape == (M0, 0)
    gB = spmm.csr_spmm_max_backward_x16(d["colptr"], d["rowind"], d["order"], arg, torch.empty(M0, 0, device="cuda", dtype=dt), K0)
    assert gB.shape == (K0, 0) and gB.dtype == dt


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_the_repeated_graph_reaches_two_strips_of_four(pkg, dt):
    """511 copies of the graph on the diagonal: the (4, 2, 64) instantiation in both directions, as in tests/test_gpu_max_arg.py."""
    from gespmm_amd import _lib, spmm

    g, d, R, N = graph(), _gdev(), BIG_REPS, BIG_N
    nnz = g["nnz"]
    assert _lib.max_arg_route_x16(M0 * R, nnz * R, N) == (4, 2, 64) and _lib.max_arg_route_x16(K0 * R, nnz * R, N) == (4, 2, 64)
    rep = torch.arange(R, device="cuda", dtype=torch.int32)

    def ptr(p):
        return torch.cat([(p[:-1].view(1, -1) + rep.view(-1, 1) * nnz).reshape(-1), torch.tensor([nnz * R], dtype=torch.int32, device="cuda")])

    def shifted(x, step):
        return (x.view(1, -1) + rep.view(-1, 1) * step).reshape(-1).contiguous()

    rowptr, colptr = ptr(d["rowptr"]), ptr(d["colptr"])
    colind, rowind, order = shifted(d["colind"], K0), shifted(d["rowind"], M0), shifted(d["order"], nnz)
    B_t, _ = operand16("ints", N, -10000.0, dt)
    _, want_C16, want_arg = forward_ref("ints", N, -10000.0, dt)
    grad_t, grad_w = grad16(N, dt)
    want_grad = narrow(max_backward(g["colptr"], g["rowind"], g["order"], want_arg, grad_w, K0), dt)[0]
    out, arg = spmm.csr_spmm_max_arg_x16(rowptr, colind, B_t.cuda().repeat(R, 1))
    assert torch.equal(out.view(R, M0, N).view(torch.int16), want_C16.cuda().view(torch.int16).expand(R, M0, N))
    wa = _dev(want_arg)
    want_big = torch.where(wa >= 0, wa.view(1, M0, N) + (rep * nnz).view(R, 1, 1), wa.view(1, M0, N).expand(R, M0, N))
    assert torch.equal(arg.view(R, M0, N), want_big)
    gB = spmm.csr_spmm_max_backward_x16(colptr, rowind, order, arg, grad_t.cuda().repeat(R, 1), K0 * R)
    assert torch.equal(gB.view(R, K0, N).view(torch.int16), want_grad.cuda().view(torch.int16).expand(R, K0, N))


def test_python_errors_raise_before_any_launch(pkg):
    from gespmm_amd import spmm

    d = _gdev()
    N = 8
    B = torch.randn(K0, N, device="cuda").bfloat16()
    grad = torch.randn(M0, N, device="cuda").bfloat16()
    arg = torch.zeros(M0, N, dtype=torch.int32, device="cuda")
    fwd = lambda **kw: spmm.csr_spmm_max_arg_x16(d["rowptr"], d["colind"], kw.pop("B", B), **kw)  # noqa: E731
    bwd = lambda **kw: spmm.csr_spmm_max_backward_x16(d["colptr"], d["rowind"], kw.pop("order", d["order"]), kw.pop("arg", arg),  # noqa: E731
                                                      kw.pop("grad", grad), kw.pop("K", K0), **kw)
    for bad in (B.float(), B.double()):  # fp32 belongs to the fp32 functions
        with pytest.raises(TypeError):
            fwd(B=bad)
        with pytest.raises(TypeError):
            bwd(grad=grad.to(bad.dtype))
    for other in (torch.float16, torch.float32):  # mixed dtypes
        with pytest.raises(TypeError):
            fwd(out=torch.empty(M0, N, device="cuda", dtype=other))
        with pytest.raises(TypeError):
            bwd(out=torch.empty(K0, N, device="cuda", dtype=other))
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
        fwd(B=torch.randn(N, K0, device="cuda").bfloat16().t())
    with pytest.raises(ValueError):
        bwd(grad=torch.randn(N, M0, device="cuda").bfloat16().t())
    with pytest.raises(ValueError):
        fwd(out=torch.empty(M0, 2 * N, device="cuda", dtype=torch.bfloat16)[:, :N])
    for shape in ((M0, N + 1), (M0 + 1, N)):  # mismatched arg / out shapes
        with pytest.raises(ValueError):
            fwd(arg=torch.zeros(shape, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError):
            fwd(out=torch.zeros(shape, device="cuda", dtype=torch.bfloat16))
        with pytest.raises(ValueError):
            bwd(arg=torch.zeros(shape, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        bwd(K=K0 + 1)
    with pytest.raises(ValueError):
        bwd(order=d["order"][:-1])
    with pytest.raises(ValueError):
        bwd(out=torch.zeros(K0 + 1, N, device="cuda", dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        fwd(empty_value=float("nan"))
    big = torch.randn(max(M0, K0), N, device="cuda").bfloat16()
    with pytest.raises(ValueError):  # a result on top of an input
        spmm.csr_spmm_max_arg_x16(d["rowptr"], d["colind"], big[:K0], out=big[:M0])
    with pytest.raises(ValueError):
        spmm.csr_spmm_max_backward_x16(d["colptr"], d["rowind"], d["order"], arg, big[:M0], K0, out=big[:K0])
    # the fp32 functions keep refusing 16-bit tensors
    with pytest.raises(TypeError):
        spmm.csr_spmm_max_arg(d["rowptr"], d["colind"], B)
    with pytest.raises(TypeError):
        spmm.csr_spmm_max_backward(d["colptr"], d["rowind"], d["order"], arg, grad, K0)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_forward_and_backward_replay_from_a_graph(pkg, dt):
    """Both kernels allocate nothing and never synchronise: captured once on one stream, replayed with new contents at the same addresses."""
    from gespmm_amd import spmm

    g, d, N = graph(), _gdev(), 64
    feat = operand16("floats", N, -10000.0, dt)[0].cuda()
    grad = grad16(N, dt)[0].cuda()
    out = torch.empty(M0, N, device="cuda", dtype=dt)
    arg = torch.empty(M0, N, dtype=torch.int32, device="cuda")
    gB = torch.empty(K0, N, device="cuda", dtype=dt)

    def step():
        spmm.csr_spmm_max_arg_x16(d["rowptr"], d["colind"], feat, out=out, arg=arg)
        spmm.csr_spmm_max_backward_x16(d["colptr"], d["rowind"], d["order"], arg, grad, K0, out=gB)

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
        feat.copy_(torch.randn(K0, N, generator=torch.Generator().manual_seed(seed)).to(dt).cuda())
        for t in (out, gB):
            t.fill_(float("nan"))
        arg.fill_(-5)
        cg.replay()
        torch.cuda.synchronize()
        want_C, want_arg = max_arg_forward(g["rowptr"], g["colind"], feat.float().cpu().numpy(), -10000.0)
        want_grad = max_backward(g["colptr"], g["rowind"], g["order"], want_arg, grad.float().cpu().numpy(), K0)
        assert np.array_equal(arg.cpu().numpy(), want_arg), seed
        assert np.array_equal(_bits(out), _bits(narrow(want_C, dt)[0])) and np.array_equal(_bits(gB), _bits(narrow(want_grad, dt)[0])), seed
