"""The relational aggregate-and-linear on fp32 features (gespmm_csr_spmm_relational_f32 through spmm.csr_spmm_relational_linear,
RelationalLinearFunction, RGCNConv) on the device. Graph and stacking: test_gpu_spmm_relational.py's.

Bound: |out - ref| <= (n + 1) 2^-23 S + 2^-25 per element (test_gpu_spmm_linear._within with u16 = 0), S on absolute values in float64.
With H the library's own fp32 product, n = 2 (R + 1) K_pad + 2: one rounding per product and per addition of the relations' and the
root's K_pad terms, plus the bias. Where H is float64 n also counts the longest chain, its scale and the rounded per-entry weight."""
import numpy as np
import pytest
import torch

from test_gpu_max_arg import K0
from test_gpu_spmm_linear import FILL, PAD, _guarded, _h, _inv_deg, _randn, _within
from test_gpu_spmm_relational import _dense, _stacked, _val

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.mark.parametrize("R", (1, 3))
@pytest.mark.parametrize("K,N_out", ((4, 1), (20, 47), (128, 128), (256, 256), (132, 33)))
@pytest.mark.parametrize("M", (1, 65, 301))
def test_selection_weights_give_the_bits_of_the_stacked_fp32_product(pkg, M, K, N_out, R):
    from gespmm_amd import _lib, spmm

    srp, sci = _stacked(M, R)
    nnz = sci.numel()
    assert _lib.spmm_relational_route_f32(R, M, K0, K, N_out, nnz, 16) == 1
    X, val = _randn(K0, K, dtype=F32, seed=K), _val(nnz)
    ns = torch.arange(N_out)
    cols, rels = (ns + 3) % K, ns % R  # one live (relation, k) per output column, a selection that is not symmetric
    W = torch.zeros(R, N_out, K)
    W[rels, ns, cols] = 1
    W = W.cuda()
    for values, scale in ((None, None), (val, None), (None, _inv_deg(srp))):
        want = _h(spmm, srp, sci, values, X, scale).view(R, M, K)[rels.cuda(), :, cols.cuda()].t().contiguous()
        buf, out = _guarded(M, N_out, F32)
        got = spmm.csr_spmm_relational_linear(srp, sci, values, X, W, row_scale=scale, out=out)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (values is not None, scale is not None)
        assert (buf[:PAD] == FILL).all() and (buf[-PAD:] == FILL).all()


@pytest.mark.parametrize("K,N_out,absent", ((24, 47, "root"), (128, 128, "bias"), (256, 256, "unweighted")))
@pytest.mark.parametrize("R", (3, 5))
def test_dense_weights_root_and_bias_within_the_float64_bound(pkg, R, K, N_out, absent):
    from gespmm_amd import _lib, spmm

    M = 301
    srp, sci = _stacked(M, R)
    assert _lib.spmm_relational_route_f32(R, M, K0, K, N_out, sci.numel(), 16) == 1
    X, W, Xr, Wr = (_randn(*s, dtype=F32, seed=i) for i, s in enumerate(((K0, K), (R, N_out, K), (M, K), (N_out, K))))
    bias = None if absent == "bias" else torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda()
    val = _val(sci.numel()) if absent == "unweighted" else None
    if absent == "root":
        Xr = Wr = None
    scale = _inv_deg(srp)
    got = spmm.csr_spmm_relational_linear(srp, sci, val, X, W, row_scale=scale, root=Xr, root_weight=Wr, bias=bias)
    H = _h(spmm, srp, sci, val, X, scale).view(R, M, K)
    terms = [(H[r], W[r]) for r in range(R)] + ([(Xr, Wr)] if Xr is not None else [])
    _within(got, terms, bias, 2 * (R + 1) * ((K + 7) // 8 * 8) + 2, F32, what="R=%d K=%d N_out=%d" % (R, K, N_out))


@pytest.mark.parametrize("K,N_out,offset", ((6, 32, 0), (260, 32, 0), (64, 257, 0), (64, 32, 1)))
def test_refusals_compose_and_the_c_entry_launches_nothing(pkg, K, N_out, offset):
    from gespmm_amd import _lib, spmm

    R, M = 3, 301
    srp, sci = _stacked(M, R)
    X = _randn(K0 * K + offset, dtype=F32, seed=1)[offset:].view(K0, K)
    W, Xr, Wr = (_randn(*s, dtype=F32, seed=i) for i, s in enumerate(((R, N_out, K), (M, K), (N_out, K)), 2))
    bias, scale = torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda(), _inv_deg(srp)
    assert _lib.spmm_relational_route_f32(R, M, K0, K, N_out, sci.numel(), 4 if offset else 16) == 0
    got = spmm.csr_spmm_relational_linear(srp, sci, None, X, W, row_scale=scale, root=Xr, root_weight=Wr, bias=bias)
    A = _dense(srp, sci, None, R, M) * scale.double().cpu().view(R, M, 1)  # H in float64: the longest row's chain and its scale count too
    terms = [(A[r] @ X.double().cpu(), W[r], A[r] @ X.double().cpu().abs()) for r in range(R)] + [(Xr, Wr)]
    _within(got, terms, bias, (R + 1) * ((K + 15) // 16 * 16) + 1 + int(torch.diff(srp).max()) + 1, F32, what="fp32 composition K=%d" % K)
    out = torch.full((M, N_out), FILL, device="cuda")
    rc = _lib.csr_spmm_relational_f32(srp.data_ptr(), sci.data_ptr(), None, scale.data_ptr(), X.data_ptr(), W.data_ptr(), Xr.data_ptr(),
                                      Wr.data_ptr(), bias.data_ptr(), out.data_ptr(), R, M, K0, K, N_out, sci.numel(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == (-2 if offset else _lib.ERR_UNSUPPORTED) and (out == FILL).all()


@pytest.mark.parametrize("valued", (False, True), ids=("unweighted", "valued"))
def test_function_gradients_against_float64_dense_relations(pkg, valued):
    from gespmm_amd import RelationalLinearFunction, _lib, graphs

    R, M, K, N_out = 3, K0, 64, 48
    srp, sci = _stacked(M, R)
    cp, ri, order = graphs.transpose_stacked_csr(srp, sci, R, K0, return_order=True)
    assert _lib.spmm_relational_route_f32(R, K0, M, N_out, K, sci.numel(), 16) == 1  # grad_x: the op on the stacked CSC, K = N_out
    v_csr = _val(sci.numel()) if valued else None
    v_csc = v_csr[order] if valued else None
    x, W, Xr, Wr, go = (_randn(*s, dtype=F32, seed=i) for i, s in enumerate(((M, K), (R, N_out, K), (M, K), (N_out, K), (M, N_out))))
    bias, scale = torch.randn(N_out, generator=torch.Generator().manual_seed(9)).cuda(), _inv_deg(srp)
    leaves = [t.requires_grad_(True) for t in (x, W, Xr, Wr, bias)]
    out = RelationalLinearFunction.apply(srp, sci, cp, ri, x, W, scale, Xr, Wr, bias, v_csr, v_csc)
    (gx,) = torch.autograd.grad(out, leaves[:1], go)
    A = _dense(srp, sci, v_csr, R, M) * scale.double().cpu().view(R, M, 1)
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    n = 2 * R * N_out + int(torch.diff(cp).max()) + 3
    _within(gx, [(A[r].t() @ d(go), W[r].t(), A[r].t() @ d(go).abs()) for r in range(R)], None, n, F32, what="grad_x")


def test_rgcn_fp32_forward_allocates_no_per_relation_array(pkg):
    from gespmm_amd import RGCNConv, graphs

    R, M, K, N_out = 3, K0, 64, 47
    cols = torch.randint(0, M, (M * 40,), generator=torch.Generator().manual_seed(4)).numpy()
    row = np.repeat(np.arange(M), 40)
    srp, sci, _ = graphs.coo_to_csr(R * M, M, (np.arange(M * 40) % R) * M + row, cols)
    srp, sci = torch.from_numpy(srp).cuda(), torch.from_numpy(sci.copy()).cuda()
    cp, ri = graphs.transpose_stacked_csr(srp, sci, R, M)
    layer, x = RGCNConv(K, N_out, R).cuda(), _randn(M, K, dtype=F32, seed=1)
    with torch.no_grad():
        layer(x, srp, sci, cp, ri)  # (warm: the library's own one-time state)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = layer(x, srp, sci, cp, ri)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base - (torch.cuda.memory_allocated() - base)
    assert out.shape == (M, N_out) and extra < R * M * K * 4
