"""The fused relational weight gradient on fp16 / bf16 features (spmm.csr_spmm_relational_weight_grad, RelationalLinearFunction and
RGCNConv with fused_weight_grad=True) on the device. Graphs, helpers and bounds are those of test_gpu_spmm_relational.py and
test_gpu_spmm_linear.py (their docstrings): |got - ref| <= r u16 S' + (1 + u16) (n + 1) 2^-23 S + 2^-25, where n counts the M rows of
the matrix unit's sum and the C + 1 terms of the chunk sum when H is the library's own 16-bit product."""
import numpy as np
import pytest
import torch

from test_gpu_max_arg import K0
from test_gpu_spmm_linear import DTYPES, FILL, PAD, U16, _h, _inv_deg, _randn, _within
from test_gpu_spmm_relational import _dense, _stacked, _val

pytestmark = pytest.mark.gpu


@DTYPES
@pytest.mark.parametrize("R", (1, 3))
@pytest.mark.parametrize("K,N_out", ((8, 1), (24, 47), (64, 32), (128, 128), (256, 256), (136, 33)))
@pytest.mark.parametrize("M", (1, 64, 65, 301))
def test_one_hot_grad_out_gives_the_bits_of_the_stacked_product(pkg, M, K, N_out, R, dtype):
    from gespmm_amd import _lib, spmm

    srp, sci = _stacked(M, R)
    nnz, blocks = sci.numel(), (M + 63) // 64
    X, val = _randn(K0, K, dtype=dtype, seed=K), _val(nnz)
    ns = torch.arange(N_out)
    sigma = (7 * ns + M - 1) % M  # column n of grad_out is row sigma(n) of the identity: every sum has ONE non-zero term
    go = torch.zeros(M, N_out, dtype=dtype)
    go[sigma, ns] = 1
    go, sigma = go.cuda(), sigma.cuda()
    for values, scale in ((None, None), (val, None), (None, _inv_deg(srp))):
        H = _h(spmm, srp, sci, values, X, scale).view(R, M, K)
        want = H[:, sigma, :].contiguous()
        if R > 1 and M <= 64:  # _stacked: relation R - 1 has no entry at all
            assert not H[R - 1].any()
        for chunks in (1, 2, None):
            if chunks is not None and chunks > blocks:
                continue
            C = _lib.spmm_relational_wgrad_chunks(R, M, K, N_out) if chunks is None else chunks
            assert _lib.spmm_relational_wgrad_route_x16(R, M, K0, K, N_out, nnz, C, 16) == 1
            buf = torch.full((R * N_out * K + 2 * PAD,), FILL, dtype=dtype, device="cuda")
            out = buf[PAD:PAD + R * N_out * K].view(R, N_out, K)
            ws = torch.full((C, R, N_out, K), float("nan"), device="cuda")
            got = spmm.csr_spmm_relational_weight_grad(srp, sci, values, X, go, R, row_scale=scale, chunks=chunks, workspace=ws, out=out)
            assert got.data_ptr() == out.data_ptr()
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (values is not None, scale is not None, chunks)
            assert (buf[:PAD] == FILL).all() and (buf[-PAD:] == FILL).all()
            again = spmm.csr_spmm_relational_weight_grad(srp, sci, values, X, go, R, row_scale=scale, chunks=chunks)
            assert torch.equal(again.view(torch.int16), got.view(torch.int16))


@DTYPES
@pytest.mark.parametrize("K,N_out,valued", ((24, 47, False), (128, 128, False), (256, 256, True)))
@pytest.mark.parametrize("R", (3, 5))
def test_dense_grad_out_within_the_float64_bound(pkg, R, K, N_out, valued, dtype):
    from gespmm_amd import _lib, spmm

    M = 301
    srp, sci = _stacked(M, R)
    X, go = _randn(K0, K, dtype=dtype, seed=1), _randn(M, N_out, dtype=dtype, seed=2)
    val, scale = (_val(sci.numel()) if valued else None), _inv_deg(srp)
    H = _h(spmm, srp, sci, val, X, scale).view(R, M, K)
    for chunks in (None, 5):
        C = _lib.spmm_relational_wgrad_chunks(R, M, K, N_out) if chunks is None else chunks
        assert _lib.spmm_relational_wgrad_route_x16(R, M, K0, K, N_out, sci.numel(), C, 16) == 1
        got = spmm.csr_spmm_relational_weight_grad(srp, sci, val, X, go, R, row_scale=scale, chunks=chunks)
        for r in range(R):
            _within(got[r], [(go.t(), H[r].t())], None, M + C + 1, dtype, what="R=%d r=%d K=%d N_out=%d C=%d" % (R, r, K, N_out, C))


@pytest.mark.parametrize("K,N_out,offset,dtype", ((12, 32, 0, torch.bfloat16), (264, 32, 0, torch.float16), (64, 257, 0, torch.bfloat16),
                                                 (64, 32, 1, torch.float16), (64, 32, 1, torch.bfloat16), (64, 32, 0, torch.float32)))
def test_composition_route_and_refusals(pkg, K, N_out, offset, dtype):
    from gespmm_amd import _lib, spmm

    R, M = 3, 301
    srp, sci = _stacked(M, R)
    X = _randn(K0 * K + offset, dtype=dtype, seed=1)[offset:].view(K0, K)
    go, scale = _randn(M, N_out, dtype=dtype, seed=2), _inv_deg(srp)
    got = spmm.csr_spmm_relational_weight_grad(srp, sci, None, X, go, R, row_scale=scale)
    assert got.shape == (R, N_out, K) and got.dtype == dtype
    if dtype == torch.float32:  # H in float64: the chain of the longest row and its scale count too
        A = _dense(srp, sci, None, R, M) * scale.double().cpu().view(R, M, 1)
        Xd = X.double().cpu()
        for r in range(R):
            _within(got[r].t(), [((A[r] @ Xd).t(), go.t(), (A[r] @ Xd.abs()).t())], None, M + int(torch.diff(srp).max()) + 2, dtype, what="fp32")
        return
    C = _lib.spmm_relational_wgrad_chunks(R, M, K, N_out)
    assert _lib.spmm_relational_wgrad_route_x16(R, M, K0, K, N_out, sci.numel(), C, 2 if offset else 16) == 0
    H = _h(spmm, srp, sci, None, X, scale).view(R, M, K)
    for r in range(R):
        _within(got[r], [(go.t(), H[r].t())], None, M + 1, dtype, roundings=2, what="composition K=%d r=%d" % (K, r))
    out = torch.full((R, N_out, K), FILL, dtype=dtype, device="cuda")
    ws = torch.empty(C * R * N_out * K, device="cuda")
    rc = _lib.csr_spmm_relational_wgrad_x16(srp.data_ptr(), sci.data_ptr(), None, scale.data_ptr(), X.data_ptr(), go.data_ptr(), ws.data_ptr(),
                                            out.data_ptr(), spmm._X16[dtype], R, M, K0, K, N_out, sci.numel(), C,
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == (-1 if offset else _lib.ERR_UNSUPPORTED) and (out == FILL).all()


@DTYPES
@pytest.mark.parametrize("valued", (False, True), ids=("unweighted", "valued"))
def test_function_weight_gradient_against_float64_dense_relations(pkg, dtype, valued):
    from gespmm_amd import RelationalLinearFunction, graphs

    R, M, K, N_out = 3, K0, 64, 47
    srp, sci = _stacked(M, R)
    cp, ri, order = graphs.transpose_stacked_csr(srp, sci, R, K0, return_order=True)
    v_csr = _val(sci.numel()) if valued else None
    v_csc = v_csr[order] if valued else None
    x, W, Xr, Wr, go = (_randn(*s, dtype=dtype, seed=i) for i, s in enumerate(((M, K), (R, N_out, K), (M, K), (N_out, K), (M, N_out))))
    bias, scale = torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda(), _inv_deg(srp)
    out = RelationalLinearFunction.apply(srp, sci, cp, ri, x, W.requires_grad_(True), scale, Xr, Wr, bias, v_csr, v_csc, True, True)
    gw, = torch.autograd.grad(out, [W], go)
    A = _dense(srp, sci, v_csr, R, M) * scale.double().cpu().view(R, M, 1)
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    row = int(torch.diff(srp).max())
    for r in range(R):  # the call of the existing gradient test
        _within(gw[r].t(), [((A[r] @ d(x)).t(), go.t(), (A[r] @ d(x).abs()).t())], None, M + row + 2, dtype, roundings=2, what="grad_weight[%d]" % r)


@pytest.mark.parametrize("num_bases,norm,self_loop", ((2, "right", True), (None, None, False)))
def test_rgcn_layer_with_the_flag_against_the_layer_without(pkg, num_bases, norm, self_loop):
    from gespmm_amd import RGCNConv, graphs

    R, M, K, N_out, dt = 3, K0, 64, 47, torch.bfloat16
    srp, sci = _stacked(M, R)
    cp, ri = graphs.transpose_stacked_csr(srp, sci, R, K0)
    torch.manual_seed(3)
    on = RGCNConv(K, N_out, R, num_bases=num_bases, norm=norm, self_loop=self_loop, fused_weight_grad=True).cuda().to(dt)
    off = RGCNConv(K, N_out, R, num_bases=num_bases, norm=norm, self_loop=self_loop).cuda().to(dt)
    off.load_state_dict(on.state_dict())
    x, go = _randn(M, K, dtype=dt, seed=1), _randn(M, N_out, dtype=dt, seed=2)
    names = [k for k, _ in on.named_parameters()]
    outs = [m(x, srp, sci, cp, ri) for m in (on, off)]
    assert torch.equal(outs[0], outs[1])
    grads = [dict(zip(names, torch.autograd.grad(o, list(m.parameters()), go))) for o, m in zip(outs, (on, off))]
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in names if k not in ("weight", "coeff"))
    # the bound of the existing layer test (its S, u and n) with one more rounding counted: the two sides differ in how grad_W is summed
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    A = _dense(srp, sci, None, R, M)
    if norm == "right":
        A = A * _inv_deg(srp).double().cpu().view(R, M, 1)
    V = d(on.weight).abs()
    S_gw = d(go).abs().t() @ (A @ d(x).abs())  # [R, N_out, K]
    S = {"weight": (4 if num_bases else 3, S_gw if num_bases is None else (d(on.coeff).abs().t() @ S_gw.view(R, -1)).view(V.shape))}
    if num_bases:
        S["coeff"] = (4, S_gw.view(R, -1) @ V.view(num_bases, -1).t())
    u, n = U16[dt], M + int(torch.diff(srp).max()) + (R + 1) * K + 2
    for key, (r, s) in S.items():
        bound = r * u * s + 2 * (1 + u) * (n + 1) * 2.0**-23 * s + 2.0**-24
        err = (d(grads[0][key]) - d(grads[1][key])).abs()
        print("%s max |flag - no flag| / bound = %.3f" % (key, (err / bound).max().item()))
        assert (err <= bound).all(), key


def test_rgcn_backward_allocates_no_per_relation_array(pkg):
    # norm=None, no root term, no bias: the other transients of the backward (index arrays of grad_x's norm path) stay out of the figure
    from gespmm_amd import RGCNConv, graphs

    R, M, K, N_out, dt = 3, K0, 64, 47, torch.bfloat16
    cols = torch.randint(0, M, (M * 40,), generator=torch.Generator().manual_seed(4)).numpy()
    row = np.repeat(np.arange(M), 40)
    srp, sci, _ = graphs.coo_to_csr(R * M, M, (np.arange(M * 40) % R) * M + row, cols)
    srp, sci = torch.from_numpy(srp).cuda(), torch.from_numpy(sci.copy()).cuda()
    cp, ri = graphs.transpose_stacked_csr(srp, sci, R, M)
    x, go = _randn(M, K, dtype=dt, seed=1), _randn(M, N_out, dtype=dt, seed=2)
    extra = {}
    for flag in (True, False):
        layer = RGCNConv(K, N_out, R, norm=None, self_loop=False, bias=False, fused_weight_grad=flag).cuda().to(dt)
        for _ in range(2):  # (the first pass warms the library's own one-time state)
            out = layer(x, srp, sci, cp, ri)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            grads = torch.autograd.grad(out, list(layer.parameters()), go)
            torch.cuda.synchronize()
            extra[flag] = torch.cuda.max_memory_allocated() - base - max(torch.cuda.memory_allocated() - base, 0)
        del out, grads
    print("backward's peak above inputs and gradients: %d bytes with the flag, %d without, R M K 2 = %d" % (extra[True], extra[False], R * M * K * 2))
    assert extra[True] < R * M * K * 2 <= extra[False]
