"""The relational aggregate-and-linear on fp16 / bf16 features (spmm.csr_spmm_relational_linear, RelationalLinearFunction, RGCNConv) on
the device. Graph: test_gpu_max_arg.graph() cut to its first M rows; the entry at CSR position e goes to relation e % (R - 1) when its
row is < 64 and to e % R otherwise (R = 1: everything to relation 0), so relation R - 1 has an empty first block when M > 64 and is
entirely empty when M <= 64. The stacked CSR comes from graphs.coo_to_csr, which keeps the CSR order inside a row.

Bounds: those of test_gpu_spmm_linear.py (its docstring), |out - ref| <= r u16 S' + (1 + u16) (n + 1) 2^-23 S + 2^-25, with
n = (R + 1) K_pad + 1 fp32 terms for the R relations and the root term; where H is not the library's own 16-bit product but float64
(the fp32 composition, the gradients) n also counts the longest chain of the sparse sum and its scale."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_max_arg import K0, graph
from test_gpu_spmm_linear import DTYPES, FILL, PAD, U16, _guarded, _h, _inv_deg, _randn, _within

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _stacked(M, R):
    from gespmm_amd import graphs

    g = graph()
    rp = g["rowptr"][:M + 1]
    ci = g["colind"][:rp[-1]]
    e, row = np.arange(len(ci)), np.repeat(np.arange(M), np.diff(rp))
    rel = np.where(row < 64, e % max(R - 1, 1), e % R)
    srp, sci, _ = graphs.coo_to_csr(R * M, K0, rel * M + row, ci)
    return torch.from_numpy(srp).cuda(), torch.from_numpy(sci.copy()).cuda()


def _val(nnz):
    return torch.rand(nnz, generator=torch.Generator().manual_seed(5)).cuda() + 0.5


def _dense(srp, sci, val, R, M):
    """[R, M, K0] float64 on the host from the stacked CSR arrays alone."""
    rows = torch.repeat_interleave(torch.arange(R * M), torch.diff(srp).cpu().long())
    v = torch.ones(sci.numel(), dtype=torch.float64) if val is None else val.double().cpu()
    return torch.zeros(R * M, K0, dtype=torch.float64).index_put_((rows, sci.cpu().long()), v, accumulate=True).view(R, M, K0)


@DTYPES
@pytest.mark.parametrize("R", (1, 3))
@pytest.mark.parametrize("K,N_out", ((8, 1), (24, 47), (128, 128), (256, 256), (136, 33)))
@pytest.mark.parametrize("M", (1, 64, 65, 301))
def test_selection_weights_give_the_bits_of_the_stacked_product(pkg, M, K, N_out, R, dtype):
    from gespmm_amd import _lib, spmm

    srp, sci = _stacked(M, R)
    nnz = sci.numel()
    assert _lib.spmm_relational_route_x16(R, M, K0, K, N_out, nnz, 16) == 1
    X, val = _randn(K0, K, dtype=dtype, seed=K), _val(nnz)
    ns = torch.arange(N_out)
    cols, rels = (ns + 3) % K, ns % R  # one live relation per output column, a selection that is not symmetric
    W = torch.zeros(R, N_out, K, dtype=dtype)
    W[rels, ns, cols] = 1
    W = W.cuda()
    for values, scale in ((None, None), (val, None), (None, _inv_deg(srp))):
        want = _h(spmm, srp, sci, values, X, scale).view(R, M, K)[rels.cuda(), :, cols.cuda()].t().contiguous()
        buf, out = _guarded(M, N_out, dtype)
        got = spmm.csr_spmm_relational_linear(srp, sci, values, X, W, row_scale=scale, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (values is not None, scale is not None)
        assert (buf[:PAD] == FILL).all() and (buf[-PAD:] == FILL).all()
    if R == 1:  # one relation IS the fused aggregate-and-linear: dense weights, root and bias, bit for bit
        Wn, Xr, Wr = (_randn(*s, dtype=dtype, seed=i) for i, s in enumerate(((N_out, K), (M, K), (N_out, K)), 2))
        bias, scale = torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda(), _inv_deg(srp)
        got = spmm.csr_spmm_relational_linear(srp, sci, val, X, Wn.unsqueeze(0), row_scale=scale, root=Xr, root_weight=Wr, bias=bias)
        want = spmm.csr_spmm_linear(srp, sci, val, X, Wn, row_scale=scale, root=Xr, root_weight=Wr, bias=bias)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@DTYPES
@pytest.mark.parametrize("K,N_out,absent", ((24, 47, "root"), (128, 128, "bias"), (256, 256, "unweighted")))
@pytest.mark.parametrize("R", (3, 5))
def test_dense_weights_root_and_bias_within_the_float64_bound(pkg, R, K, N_out, absent, dtype):
    from gespmm_amd import _lib, spmm

    M = 301
    srp, sci = _stacked(M, R)
    assert _lib.spmm_relational_route_x16(R, M, K0, K, N_out, sci.numel(), 16) == 1
    X, W, Xr, Wr = (_randn(*s, dtype=dtype, seed=i) for i, s in enumerate(((K0, K), (R, N_out, K), (M, K), (N_out, K))))
    bias = None if absent == "bias" else torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda()
    val = _val(sci.numel()) if absent == "unweighted" else None
    if absent == "root":
        Xr = Wr = None
    scale = _inv_deg(srp)
    got = spmm.csr_spmm_relational_linear(srp, sci, val, X, W, row_scale=scale, root=Xr, root_weight=Wr, bias=bias)
    H = _h(spmm, srp, sci, val, X, scale).view(R, M, K)
    terms = [(H[r], W[r]) for r in range(R)] + ([(Xr, Wr)] if Xr is not None else [])
    _within(got, terms, bias, (R + 1) * ((K + 15) // 16 * 16) + 1, dtype, what="R=%d K=%d N_out=%d" % (R, K, N_out))


@pytest.mark.parametrize("K,N_out,offset,dtype", ((12, 32, 0, torch.bfloat16), (264, 32, 0, torch.float16), (64, 257, 0, torch.bfloat16),
                                                 (64, 32, 1, torch.float16), (64, 32, 1, torch.bfloat16), (64, 32, 0, torch.float32)))
def test_composition_route_and_refusals(pkg, K, N_out, offset, dtype):
    from gespmm_amd import _lib, spmm

    R, M = 3, 301
    srp, sci = _stacked(M, R)
    X = _randn(K0 * K + offset, dtype=dtype, seed=1)[offset:].view(K0, K)
    W, Xr, Wr = (_randn(*s, dtype=dtype, seed=i) for i, s in enumerate(((R, N_out, K), (M, K), (N_out, K)), 2))
    bias, scale = torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda(), _inv_deg(srp)
    got = spmm.csr_spmm_relational_linear(srp, sci, None, X, W, row_scale=scale, root=Xr, root_weight=Wr, bias=bias)
    n = (R + 1) * ((K + 15) // 16 * 16) + 1
    if dtype == torch.float32:  # H in float64: the chain of the longest row and its scale count too
        A = _dense(srp, sci, None, R, M) * scale.double().cpu().view(R, M, 1)
        terms = [(A[r] @ X.double().cpu(), W[r], A[r] @ X.double().cpu().abs()) for r in range(R)] + [(Xr, Wr)]
        _within(got, terms, bias, n + int(torch.diff(srp).max()) + 1, dtype, what="fp32 composition")
        return
    assert _lib.spmm_relational_route_x16(R, M, K0, K, N_out, sci.numel(), 2 if offset else 16) == 0
    H = _h(spmm, srp, sci, None, X, scale).view(R, M, K)
    _within(got, [(H[r], W[r]) for r in range(R)] + [(Xr, Wr)], bias, n, dtype, what="composition K=%d" % K)
    out = torch.full((M, N_out), FILL, dtype=dtype, device="cuda")
    rc = _lib.csr_spmm_relational_x16(srp.data_ptr(), sci.data_ptr(), None, scale.data_ptr(), X.data_ptr(), W.data_ptr(), Xr.data_ptr(),
                                      Wr.data_ptr(), bias.data_ptr(), out.data_ptr(), spmm._X16[dtype], R, M, K0, K, N_out, sci.numel(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == (-1 if offset else _lib.ERR_UNSUPPORTED) and (out == FILL).all()


@DTYPES
@pytest.mark.parametrize("valued", (False, True), ids=("unweighted", "valued"))
def test_function_gradients_against_float64_dense_relations(pkg, dtype, valued):
    from gespmm_amd import RelationalLinearFunction, graphs

    R, M, K, N_out = 3, K0, 64, 47
    srp, sci = _stacked(M, R)
    cp, ri, order = graphs.transpose_stacked_csr(srp, sci, R, K0, return_order=True)
    v_csr = _val(sci.numel()) if valued else None
    v_csc = v_csr[order] if valued else None
    x, W, Xr, Wr, go = (_randn(*s, dtype=dtype, seed=i) for i, s in enumerate(((M, K), (R, N_out, K), (M, K), (N_out, K), (M, N_out))))
    bias, scale = torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda(), _inv_deg(srp)
    if valued:
        with pytest.raises(RuntimeError, match="values_csc"):
            RelationalLinearFunction.apply(srp, sci, cp, ri, x, W.clone().requires_grad_(True), scale, Xr, Wr, bias, v_csr, None)
    leaves = [t.requires_grad_(True) for t in (x, W, Xr, Wr, bias)]
    out = RelationalLinearFunction.apply(srp, sci, cp, ri, x, W, scale, Xr, Wr, bias, v_csr, v_csc)
    gx, gw, gr, grw, gb = torch.autograd.grad(out, leaves, go)
    # float64 per-relation matrices from the CSR arrays alone (independent of the CSC arrays handed to the op). The op rounds an
    # aggregate (A_r^T g'_r, H_r) and the gradient: two roundings, each within u16 S; fp32 terms: the GEMM's, the longest chain, the scale
    A = _dense(srp, sci, v_csr, R, M) * scale.double().cpu().view(R, M, 1)
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    col, row = int(torch.diff(cp).max()), int(torch.diff(srp).max())
    _within(gx, [(A[r].t() @ d(go), W[r].t(), A[r].t() @ d(go).abs()) for r in range(R)], None, R * 48 + col + 2, dtype, roundings=2, what="grad_x")
    for r in range(R):
        _within(gw[r].t(), [((A[r] @ d(x)).t(), go.t(), (A[r] @ d(x).abs()).t())], None, M + row + 2, dtype, roundings=2, what="grad_weight[%d]" % r)
    _within(gr, [(go, Wr.t())], None, N_out, dtype, what="grad_root")
    _within(grw, [(go.t(), Xr.t())], None, M, dtype, what="grad_root_weight")
    _within(gb.unsqueeze(0), [(torch.ones(1, M), go.t())], None, M, torch.float32, what="grad_bias")


@pytest.mark.parametrize("num_bases,norm,self_loop", ((2, "right", True), (None, None, False)))
def test_rgcn_layer_bf16_against_fp32_on_widened_parameters(pkg, num_bases, norm, self_loop):
    from gespmm_amd import RGCNConv, graphs

    R, M, K, N_out, dt = 3, K0, 64, 47, torch.bfloat16
    srp, sci = _stacked(M, R)
    cp, ri = graphs.transpose_stacked_csr(srp, sci, R, K0)
    torch.manual_seed(3)
    low = RGCNConv(K, N_out, R, num_bases=num_bases, norm=norm, self_loop=self_loop).cuda().to(dt)
    wide = RGCNConv(K, N_out, R, num_bases=num_bases, norm=norm, self_loop=self_loop).cuda()
    wide.load_state_dict({k: v.float() for k, v in low.state_dict().items()})
    x, go = _randn(M, K, dtype=dt, seed=1), _randn(M, N_out, dtype=dt, seed=2)
    names = [k for k, _ in low.named_parameters()]
    outs = [m(x.to(m.weight.dtype), srp, sci, cp, ri) for m in (low, wide)]
    assert outs[0].dtype == dt and outs[1].dtype == torch.float32
    grads = [dict(zip(names, torch.autograd.grad(o, list(m.parameters()), go.to(o.dtype)))) for o, m in zip(outs, (low, wide))]
    # float64 absolute-value sums S per compared tensor. The bf16 path rounds W_r (bases only), H_r and out in the forward; H_r, grad_W
    # and (bases only) the gradient of coeff / V in the backward; root and bias gradients once. The fp32 path has fp32 terms alone.
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    A = _dense(srp, sci, None, R, M)
    if norm == "right":
        A = A * _inv_deg(srp).double().cpu().view(R, M, 1)
    Habs, V = A @ d(x).abs(), d(wide.weight).abs()
    Wabs = V if num_bases is None else (d(wide.coeff).abs() @ V.view(num_bases, -1)).view(R, N_out, K)
    S_gw = d(go).abs().t() @ Habs  # [R, N_out, K]
    b = 1 if num_bases else 0
    S = {"out": (2 + b, (Habs @ Wabs.transpose(1, 2)).sum(0) + (d(x).abs() @ d(wide.loop_weight).abs().t() if self_loop else 0) + d(wide.bias).abs()),
         "weight": (2 + b, S_gw if num_bases is None else (d(wide.coeff).abs().t() @ S_gw.view(R, -1)).view(V.shape)),
         "bias": (1, d(go).abs().sum(0))}
    if num_bases:
        S["coeff"] = (3, S_gw.view(R, -1) @ V.view(num_bases, -1).t())
    if self_loop:
        S["loop_weight"] = (1, d(go).abs().t() @ d(x).abs())
    u, n = U16[dt], M + int(torch.diff(srp).max()) + (R + 1) * K + 2
    for key, (r, s) in S.items():
        a, c = outs if key == "out" else (g[key] for g in grads)
        bound = r * u * s + 2 * (1 + u) * (n + 1) * 2.0**-23 * s + 2.0**-24
        err = (d(a) - d(c)).abs()
        print("%s max |bf16 - fp32| / bound = %.3f" % (key, (err / bound).max().item()))
        assert (err <= bound).all(), key


def test_rgcn_forward_allocates_no_per_relation_array(pkg):
    from gespmm_amd import RGCNConv, graphs

    R, M, K, N_out, dt = 3, K0, 64, 47, torch.bfloat16
    cols = torch.randint(0, M, (M * 40,), generator=torch.Generator().manual_seed(4)).numpy()
    row = np.repeat(np.arange(M), 40)
    srp, sci, _ = graphs.coo_to_csr(R * M, M, (np.arange(M * 40) % R) * M + row, cols)
    srp, sci = torch.from_numpy(srp).cuda(), torch.from_numpy(sci.copy()).cuda()
    cp, ri = graphs.transpose_stacked_csr(srp, sci, R, M)
    layer, x = RGCNConv(K, N_out, R).cuda().to(dt), _randn(M, K, dtype=dt, seed=1)
    with torch.no_grad():
        layer(x, srp, sci, cp, ri)  # (warm: the library's own one-time state)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = layer(x, srp, sci, cp, ri)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - (torch.cuda.memory_allocated() - base)
    print("peak above inputs and output: %d bytes, R M K 2 = %d" % (extra, R * M * K * 2))
    assert out.shape == (M, N_out) and extra < R * M * K * 2
