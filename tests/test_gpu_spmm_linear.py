"""The fused aggregate-and-linear on fp16 / bf16 features (spmm.csr_spmm_linear, SpmmLinearFunction, SAGEConv(fused_linear=True)) on
the device. Graph: test_gpu_max_arg.graph() (301 rows over 257 nodes; empty rows, rows of 1 / 63 / 64 / 65 / 130 / 700 entries), cut to
its first M rows.

Bound of the dense-weight tests, per element, against a float64 restatement whose H is the 16-bit product the library already has:
    |out - ref| <= r u16 S' + (1 + u16) (n + 1) 2^-23 S + 2^-25
u16 = 2^-8 (bf16) / 2^-11 (fp16); S the same expression on absolute values; n the fp32 terms of an element; r = 1 and S' = |ref| for
ONE rounding at the store (products of two 16-bit numbers are exact in fp32; 2^-23 per addition covers a matrix unit that chops its
partial sums; 2^-25 is half of fp16's smallest subnormal). Where a path rounds intermediate 16-bit arrays too (the layer comparison,
the backward's g' and G) each of them moves an element by at most u16 S, so r counts the roundings and S' = S."""
import numpy as np
import pytest
import torch

from test_gpu_max_arg import K0, graph

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16), ids=("fp16", "bf16"))
U16 = {torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8, torch.float32: 0.0}  # (an fp32 result: the fp32 terms alone)
PAD, FILL = 64, 7.0  # guard margin of `out`, in elements (128 bytes: the view stays 16-byte aligned)


def _csr(M):
    g = graph()
    rp = g["rowptr"][:M + 1]
    return torch.from_numpy(rp.copy()).cuda(), torch.from_numpy(g["colind"][:rp[-1]].copy()).cuda()


def _randn(*shape, dtype, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


def _inv_deg(rp):
    deg = torch.diff(rp).float()
    return torch.where(deg > 0, 1 / deg, torch.zeros_like(deg))


def _guarded(M, N_out, dtype):
    buf = torch.full((M * N_out + 2 * PAD,), FILL, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + M * N_out].view(M, N_out)


def _h(spmm, rp, ci, val, X, scale):
    """H as the library's 16-bit product returns it today."""
    if scale is not None:
        return spmm.csr_spmm_fused(rp, ci, val, X.float(), row_scale=scale).to(X.dtype)
    return spmm.csr_spmm_no_edge_value(rp, ci, X) if val is None else spmm.csr_spmm(rp, ci, val, X)


def _within(got, terms, bias, n, dtype, roundings=1, what=""):
    """terms: [(a, b)] or [(a, b, |a| summed in absolute values)] with the element sum_k a[r, k] b[n, k]; bias fp32 or None."""
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    ref = sum(d(t[0]) @ d(t[1]).t() for t in terms)
    S = sum(d(t[-1] if len(t) == 3 else t[0]).abs() @ d(t[1]).abs().t() for t in terms)
    if bias is not None:
        ref, S = ref + d(bias), S + d(bias).abs()
    u = U16[dtype]
    bound = u * (ref.abs() if roundings == 1 else roundings * S) + (1 + u) * (n + 1) * 2.0**-23 * S + 2.0**-25
    err = (d(got) - ref).abs()
    worst = (err / bound).max().item() if err.numel() else 0.0
    print("%s max |err| / bound = %.3f" % (what, worst))
    assert (err <= bound).all(), (what, worst)


@DTYPES
@pytest.mark.parametrize("K,N_out", ((8, 1), (24, 47), (64, 32), (128, 128), (256, 256), (136, 33)))
@pytest.mark.parametrize("M", (1, 64, 65, 301))
def test_exact_weights_give_the_bits_of_the_16_bit_product(pkg, M, K, N_out, dtype):
    from gespmm_amd import _lib, spmm

    rp, ci = _csr(M)
    nnz = ci.numel()
    assert _lib.spmm_linear_route_x16(M, K0, K, N_out, nnz, 16) == 1
    X = _randn(K0, K, dtype=dtype, seed=K)
    val = torch.rand(nnz, generator=torch.Generator().manual_seed(5)).cuda() + 0.5
    cols = (torch.arange(N_out) + 3) % K
    Wn = torch.zeros(N_out, K, dtype=dtype)
    Wn[torch.arange(N_out), cols] = 1  # a selection that is not symmetric: a transposed or mis-laid fragment cannot pass
    Wn = Wn.cuda()
    for values, scale in ((None, None), (val, None), (None, _inv_deg(rp))):
        want = _h(spmm, rp, ci, values, X, scale)[:, cols.cuda()].contiguous()
        buf, out = _guarded(M, N_out, dtype)
        got = spmm.csr_spmm_linear(rp, ci, values, X, Wn, row_scale=scale, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (values is not None, scale is not None)
        assert (buf[:PAD] == FILL).all() and (buf[-PAD:] == FILL).all()


@DTYPES
@pytest.mark.parametrize("K,N_out,absent", ((24, 47, "root"), (128, 128, "bias"), (256, 256, "unweighted")))
def test_dense_weights_root_and_bias_within_the_float64_bound(pkg, K, N_out, absent, dtype):
    from gespmm_amd import _lib, spmm

    M = 301
    rp, ci = _csr(M)
    assert _lib.spmm_linear_route_x16(M, K0, K, N_out, ci.numel(), 16) == 1
    X, Wn, Xr, Wr = (_randn(*s, dtype=dtype, seed=i) for i, s in enumerate(((K0, K), (N_out, K), (M, K), (N_out, K))))
    bias = None if absent == "bias" else torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda()
    val = torch.rand(ci.numel(), generator=torch.Generator().manual_seed(5)).cuda() + 0.5 if absent == "unweighted" else None
    if absent == "root":
        Xr = Wr = None
    scale = _inv_deg(rp)
    got = spmm.csr_spmm_linear(rp, ci, val, X, Wn, row_scale=scale, root=Xr, root_weight=Wr, bias=bias)
    terms = [(_h(spmm, rp, ci, val, X, scale), Wn)] + ([(Xr, Wr)] if Xr is not None else [])
    _within(got, terms, bias, 2 * ((K + 15) // 16 * 16) + 1, dtype, what="K=%d N_out=%d" % (K, N_out))


@DTYPES
@pytest.mark.parametrize("K,N_out,offset", ((12, 32, 0), (264, 32, 0), (64, 257, 0), (64, 32, 1)))
def test_composition_route(pkg, K, N_out, offset, dtype):
    from gespmm_amd import _lib, spmm

    M = 301
    rp, ci = _csr(M)
    X = _randn(K0 * K + offset, dtype=dtype, seed=1)[offset:].view(K0, K)
    Wn, Xr, Wr = (_randn(*s, dtype=dtype, seed=i) for i, s in enumerate(((N_out, K), (M, K), (N_out, K)), 2))
    bias, scale = torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda(), _inv_deg(rp)
    assert _lib.spmm_linear_route_x16(M, K0, K, N_out, ci.numel(), 2 if offset else 16) == 0
    got = spmm.csr_spmm_linear(rp, ci, None, X, Wn, row_scale=scale, root=Xr, root_weight=Wr, bias=bias)
    _within(got, [(_h(spmm, rp, ci, None, X, scale), Wn), (Xr, Wr)], bias, 2 * ((K + 15) // 16 * 16) + 1, dtype, what="composition K=%d" % K)
    out = torch.full((M, N_out), FILL, dtype=dtype, device="cuda")
    rc = _lib.csr_spmm_linear_x16(rp.data_ptr(), ci.data_ptr(), None, scale.data_ptr(), X.data_ptr(), Wn.data_ptr(), Xr.data_ptr(), Wr.data_ptr(),
                                  bias.data_ptr(), out.data_ptr(), spmm._X16[dtype], M, K0, K, N_out, ci.numel(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == (-1 if offset else _lib.ERR_UNSUPPORTED) and (out == FILL).all()


def _square():
    from gespmm_amd import graphs

    rp, ci = _csr(K0)  # the first 257 rows over 257 nodes: square, with empty rows and the rows of 63 / 64 / 65 / 130 / 700 entries
    return (rp, ci) + tuple(graphs.transpose_csr(rp, ci))


@DTYPES
@pytest.mark.parametrize("valued", (False, True), ids=("unweighted", "valued"))
def test_function_gradients_against_the_float64_composition(pkg, dtype, valued):
    from gespmm_amd import SpmmLinearFunction, graphs, spmm

    M, K, N_out = K0, 64, 47
    rp, ci = _csr(M)
    cp, ri, order = graphs.transpose_csr(rp, ci, return_order=True)
    v_csr = torch.rand(ci.numel(), generator=torch.Generator().manual_seed(5)).cuda() + 0.5 if valued else None
    v_csc = v_csr[order] if valued else None
    x, Wn, Xr, Wr, go = (_randn(*s, dtype=dtype, seed=i) for i, s in enumerate(((M, K), (N_out, K), (M, K), (N_out, K), (M, N_out))))
    bias, scale = torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda(), _inv_deg(rp)
    if valued:  # grad_weight needs A^T as much as grad_x does: refused in the forward, whatever x asks for
        with pytest.raises(RuntimeError, match="values_csc"):
            SpmmLinearFunction.apply(rp, ci, cp, ri, x, Wn.clone().requires_grad_(True), scale, Xr, Wr, bias, v_csr, None)
    leaves = [t.requires_grad_(True) for t in (x, Wn, Xr, Wr, bias)]
    out = SpmmLinearFunction.apply(rp, ci, cp, ri, x, Wn, scale, Xr, Wr, bias, v_csr, v_csc)
    _within(out, [(_h(spmm, rp, ci, v_csr, x.detach(), scale), Wn), (Xr, Wr)], bias, 2 * K + 1, dtype, what="forward")
    gx, gw, gr, grw, gb = torch.autograd.grad(out, leaves, go)
    # G = A^T g' in float64 from the CSR arrays (independent of the CSC arrays handed to the op), g' = narrow(row_scale * grad_out) as
    # torch makes it. The op rounds G and the gradient: two roundings, each within u16 S; fp32 terms: the GEMM's and the longest column's
    rows = torch.repeat_interleave(torch.arange(M), torch.diff(rp).cpu().long())
    A = torch.zeros(M, M, dtype=torch.float64).index_put_((rows, ci.cpu().long()), torch.ones(ci.numel(), dtype=torch.float64) if v_csr is None
                                                           else v_csr.double().cpu(), accumulate=True)
    g = (go.float() * scale.unsqueeze(1)).to(dtype).double().cpu()
    G, Gabs, col = A.t() @ g, A.t() @ g.abs(), int(torch.diff(cp).max())
    _within(gx, [(G, Wn.t(), Gabs)], None, N_out + col, dtype, roundings=2, what="grad_x")
    _within(gw, [(G.t(), x.t(), Gabs.t())], None, M + col, dtype, roundings=2, what="grad_weight")
    _within(gr, [(go, Wr.t())], None, N_out, dtype, what="grad_root")
    _within(grw, [(go.t(), Xr.t())], None, M, dtype, what="grad_root_weight")
    _within(gb.unsqueeze(0), [(torch.ones(1, M), go.t())], None, M, torch.float32, what="grad_bias")


def test_sage_layer_fused_against_unfused(pkg):
    from gespmm_amd import SAGEConv

    M, K, N_out, dt = K0, 64, 47, torch.bfloat16
    rp, ci, cp, ri = _square()
    torch.manual_seed(3)
    fused, plain = (SAGEConv(K, N_out, "mean", fused_linear=f).cuda().to(dt) for f in (True, False))
    fused.load_state_dict(plain.state_dict())
    x, go = _randn(M, K, dtype=dt, seed=1), _randn(M, N_out, dtype=dt, seed=2)
    outs = [m(x, rp, ci, cp, ri) for m in (fused, plain)]
    grads = [dict(zip(("ws", "bs", "wn", "bn"), torch.autograd.grad(o, [m.fc_self.weight, m.fc_self.bias, m.fc_neigh.weight, m.fc_neigh.bias], go)))
             for o, m in zip(outs, (fused, plain))]
    # float64 absolute-value sums; each path's error is (its 16-bit roundings) u16 S + its fp32 terms: fused rounds H and out (forward),
    # g', G and the gradient (backward); unfused rounds H, both linears and their sum (forward), H and the gradient (backward)
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    deg = torch.diff(rp).double().cpu()
    A = torch.zeros(M, M, dtype=torch.float64)
    A.index_put_((torch.repeat_interleave(torch.arange(M), torch.diff(rp).cpu().long()), ci.cpu().long()), torch.ones(ci.numel(), dtype=torch.float64), accumulate=True)
    Habs = (A @ d(x).abs()) / deg.clamp(min=1).unsqueeze(1)
    p = plain
    S_out = Habs @ d(p.fc_neigh.weight).abs().t() + d(x).abs() @ d(p.fc_self.weight).abs().t() + d(p.fc_neigh.bias).abs() + d(p.fc_self.bias).abs()
    S = {"out": S_out, "ws": d(go).abs().t() @ d(x).abs(), "wn": d(go).abs().t() @ Habs, "bs": d(go).abs().sum(0), "bn": d(go).abs().sum(0)}
    u, n = U16[dt], M + int(deg.max()) + 2 * K + 2
    for key, (r_fused, r_plain) in {"out": (2, 4), "ws": (1, 1), "wn": (3, 2), "bs": (1, 1), "bn": (1, 1)}.items():
        a, b = (outs if key == "out" else [g[key] for g in grads])
        bound = (r_fused + r_plain) * u * S[key] + 2 * (1 + u) * (n + 1) * 2.0**-23 * S[key] + 2.0**-24
        err = (d(a) - d(b)).abs()
        print("%s max |fused - unfused| / bound = %.3f" % (key, (err / bound).max().item()))
        assert (err <= bound).all(), key
    with pytest.raises(TypeError, match="fp16 / bf16"):
        SAGEConv(K, N_out, "mean", fused_linear=True).cuda()(x.float(), rp, ci, cp, ri)
    for agg in ("gcn", "pool"):
        with pytest.raises(ValueError, match="mean"):
            SAGEConv(K, N_out, agg, fused_linear=True)


def test_fused_layer_allocates_nothing_of_nnz_elements(pkg):
    from gespmm_amd import SAGEConv, graphs

    M, K, N_out, dt = K0, 64, 47, torch.bfloat16
    cols = torch.randint(0, M, (M, 40), generator=torch.Generator().manual_seed(4), dtype=torch.int32).cuda()
    rp, ci = (torch.arange(M + 1, dtype=torch.int32) * 40).cuda(), cols.reshape(-1).contiguous()
    cp, ri = graphs.transpose_csr(rp, ci)
    nnz = ci.numel()
    assert 4 * nnz > M * K * 2  # an [nnz] fp32 array is larger than the [M, K] aggregate
    layer, x = SAGEConv(K, N_out, "mean", fused_linear=True).cuda().to(dt), _randn(M, K, dtype=dt, seed=1)
    with torch.no_grad():
        layer(x, rp, ci, cp, ri)  # (warm: the library's own one-time state)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = layer(x, rp, ci, cp, ri)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - (torch.cuda.memory_allocated() - base)
    print("peak above inputs and output: %d bytes, 4 nnz = %d" % (extra, 4 * nnz))
    assert out.shape == (M, N_out) and extra < 4 * nnz
