"""FusedGCNFunction and GCNConv(fused=True): the scalings and the bias inside the product, with the output bits of the unfused chain."""
import numpy as np
import pytest
import torch

from helpers import bits

pytestmark = pytest.mark.gpu


def _graph_from_edges(ei, n_v):
    """The operands gcn_custom.py builds (self loops added, both index orders, random edge weights in both orders)."""
    from gespmm_amd import graphs

    loops = np.stack([np.arange(n_v), np.arange(n_v)]).astype(np.int64)
    e = np.unique(np.concatenate([ei.astype(np.int64), loops], axis=1), axis=1)
    order = np.lexsort((e[0], e[1]))  # by destination, then source: CSR of the aggregating side
    dst, src = e[1][order], e[0][order]
    rowptr = np.zeros(n_v + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(np.bincount(dst, minlength=n_v))
    g = {"n_v": n_v, "rowptr": torch.from_numpy(rowptr).cuda(), "colind": torch.from_numpy(src.astype(np.int32)).cuda()}
    w = torch.from_numpy(np.random.RandomState(3).uniform(0.1, 1.0, src.size).astype(np.float32)).cuda()
    colptr, rowind, w_csc = graphs.transpose_csr(g["rowptr"], g["colind"], K=n_v, val=w)
    g.update(colptr=colptr, rowind=rowind, value_csr=w, value_csc=w_csc)
    return g


@pytest.fixture(scope="module")
def graph():
    rng = np.random.RandomState(0)
    n_v, n_e = 300, 2400
    src, dst = rng.randint(0, n_v, n_e), rng.randint(0, n_v, n_e)
    keep = src != dst
    return _graph_from_edges(np.stack([src[keep], dst[keep]]), n_v)


@pytest.fixture(scope="module")
def pubmed(bundled):
    g = bundled["pubmed"]
    rows = np.repeat(np.arange(g["M"]), np.diff(g["rowptr"]))
    return _graph_from_edges(np.stack([g["colind"].astype(np.int64), rows]), g["M"])


def _same_bits(a, b):
    return np.array_equal(bits(a.detach().cpu().numpy()), bits(b.detach().cpu().numpy()))


def _args(g, weighted):
    a = (g["rowptr"], g["colind"], g["colptr"], g["rowind"])
    return a, ((g["value_csr"], g["value_csc"]) if weighted else (None, None))


@pytest.mark.parametrize("weighted", (False, True))
def test_function_forward_and_feat_gradient_have_the_unfused_bits(pkg, graph, weighted):
    from gespmm_amd import FusedGCNFunction, SPMMFunction

    g = graph
    idx, (w_csr, w_csc) = _args(g, weighted)
    torch.manual_seed(0)
    n = g["n_v"]
    out_scale = torch.rand(n, 1, device="cuda") + 0.5
    in_scale = -(torch.rand(n, 1, device="cuda") + 0.5)
    bias = torch.randn(24, device="cuda").requires_grad_(True)
    h0 = torch.randn(n, 24, device="cuda")
    gout = torch.randn(n, 24, device="cuda")
    # unfused chain on SPMMFunction (no GEMM in between: no rocBLAS ordering enters)
    hu = h0.clone().requires_grad_(True)
    bu = bias.detach().clone().requires_grad_(True)
    yu = SPMMFunction.apply(*idx, hu * out_scale, w_csr, w_csc) * in_scale + bu
    (yu * gout).sum().backward()
    hf = h0.clone().requires_grad_(True)
    yf = FusedGCNFunction.apply(*idx, hf, out_scale, in_scale, bias, w_csr, w_csc)
    (yf * gout).sum().backward()
    assert _same_bits(yf, yu)
    assert _same_bits(hf.grad, hu.grad)
    assert torch.allclose(bias.grad, bu.grad, rtol=1e-5, atol=1e-5)  # (a column sum: the reduction order is torch's, twice)
    assert out_scale.grad is None and in_scale.grad is None
    # every vector optional
    y2 = FusedGCNFunction.apply(*idx, h0, None, in_scale, None, w_csr, w_csc)
    assert _same_bits(y2, SPMMFunction.apply(*idx, h0, w_csr, w_csc) * in_scale)
    y3 = FusedGCNFunction.apply(*idx, h0, None, None, None, w_csr, w_csc)
    assert _same_bits(y3, SPMMFunction.apply(*idx, h0, w_csr, w_csc))


def test_function_keeps_the_error_behaviour(pkg, graph):
    from gespmm_amd import FusedGCNFunction

    g = graph
    idx, (w_csr, w_csc) = _args(g, True)
    x = torch.randn(g["n_v"], 8, device="cuda", requires_grad=True)
    s = torch.rand(g["n_v"], device="cuda") + 0.5
    y = FusedGCNFunction.apply(*idx, x, s, s, None, w_csr)  # no CSC weights
    with pytest.raises(RuntimeError, match="edge values in both"):
        y.sum().backward()
    # edge weights are constants, index tensors get no gradient
    ew = w_csr.clone().requires_grad_(True)
    x2 = torch.randn(g["n_v"], 8, device="cuda", requires_grad=True)
    FusedGCNFunction.apply(*idx, x2, s, s, None, ew, w_csc).sum().backward()
    assert ew.grad is None and x2.grad is not None
    with pytest.raises(RuntimeError):  # no CPU path, as everywhere
        FusedGCNFunction.apply(*(t.cpu() for t in idx), x.detach().cpu(), None, None, None)


@pytest.mark.parametrize("cached", (False, True))
@pytest.mark.parametrize("weighted", (False, True))
def test_gcnconv_fused_against_unfused(pkg, graph, weighted, cached):
    from gespmm_amd import GCNConv

    g = graph
    idx, w = _args(g, weighted)
    torch.manual_seed(0)
    ref = GCNConv(40, 16, cached=cached).cuda()
    fus = GCNConv(40, 16, cached=cached, fused=True).cuda()
    assert GCNConv(40, 16).fused is False  # off by default
    with torch.no_grad():
        ref.bias.uniform_(-0.1, 0.1)
        fus.weight.copy_(ref.weight)
        fus.bias.copy_(ref.bias)
    x0 = torch.randn(g["n_v"], 40, device="cuda")
    xr, xf = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    extra = w if weighted else ()
    yr, yf = ref(xr, *idx, *extra), fus(xf, *idx, *extra)
    assert _same_bits(yf, yr)
    yr.pow(2).sum().backward()
    yf.pow(2).sum().backward()
    # the tolerances of test_gpu_op.py::test_gcnconv_matches_dense_restatement
    assert torch.allclose(xf.grad.double(), xr.grad.double(), atol=2e-3)
    assert torch.allclose(fus.weight.grad.double(), ref.weight.grad.double(), atol=2e-3)
    assert torch.allclose(fus.bias.grad.double(), ref.bias.grad.double(), atol=2e-3)
    # a second forward (cached plans and scalings in use)
    assert _same_bits(fus(x0, *idx, *extra), ref(x0, *idx, *extra))
    # no normalisation: the bias alone is fused
    for kw in (dict(normalize=False),):
        a, b = GCNConv(40, 16, cached=cached, **kw).cuda(), GCNConv(40, 16, cached=cached, fused=True, **kw).cuda()
        with torch.no_grad():
            b.weight.copy_(a.weight)
        assert _same_bits(b(x0, *idx, *extra), a(x0, *idx, *extra)), kw


def test_two_layer_gcn_on_pubmed_same_losses(pkg, pubmed):
    import torch.nn.functional as F

    from gespmm_amd import GCNConv

    g = pubmed
    idx, w = _args(g, True)
    torch.manual_seed(1)
    x = torch.rand(g["n_v"], 50, device="cuda")
    ylab = torch.randint(0, 3, (g["n_v"],), device="cuda")
    losses = {}
    for fused in (False, True):
        torch.manual_seed(2)
        c1, c2 = GCNConv(50, 128, cached=True, fused=fused).cuda(), GCNConv(128, 3, cached=True, fused=fused).cuda()
        opt = torch.optim.SGD(list(c1.parameters()) + list(c2.parameters()), lr=0.05)
        seq = []
        for _ in range(5):
            opt.zero_grad()
            loss = F.nll_loss(F.log_softmax(c2(F.relu(c1(x, *idx, *w)), *idx, *w), dim=1), ylab)
            loss.backward()
            opt.step()
            seq.append(loss.detach().clone())
        losses[fused] = torch.stack(seq).cpu().numpy()
    assert np.array_equal(bits(losses[True]), bits(losses[False])), (losses[True], losses[False])
