"""GATConv(fused_aggregate=True) on the GPU: output and all five gradients bit-equal to GATConv(fused_score=True) with copied
parameters — on the random square graph of tests/test_gpu_gat_fused.py, on the edge-case pattern made square (its 21 rows padded with
empty ones to its 301 columns: long rows, swept rows, empty rows) and on cora — no tensor with nnz rows saved between forward and
backward, and two training steps of the example model with --fused-aggregate's settings."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, edge_case_csr
from test_gpu_gat import _dev, _rand, _random_graph

pytestmark = pytest.mark.gpu


def _square_edge():
    g = edge_case_csr()
    n = g["K"]
    assert g["M"] < n
    rowptr = np.concatenate((g["rowptr"], np.full(n - g["M"], g["nnz"], dtype=np.int32))).astype(np.int32)
    return n, rowptr, g["colind"]


def _cora():
    from gespmm_amd import graphs

    g = graphs.load_mtx_as_csr(os.path.join(ROOT, "tests", "golden", "cora.mtx"))
    assert g["M"] == g["K"]
    return g["M"], g["rowptr"], g["colind"]


def _graph(name):
    from gespmm_amd import graphs

    if name == "random":
        rowptr, colind, _ = _random_graph(300)
        n = 300
    else:
        n, rowptr, colind = _square_edge() if name == "edge" else _cora()
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    return n, int(colind.size), (rp, ci, colptr, rowind, order.to(torch.int32))


def _layers(n_in, F, heads, concat):
    import gespmm_amd

    torch.manual_seed(7 + heads)
    score = gespmm_amd.GATConv(n_in, F, heads=heads, concat=concat, negative_slope=0.2, fused_score=True).cuda()
    aggregate = gespmm_amd.GATConv(n_in, F, heads=heads, concat=concat, negative_slope=0.2, fused_aggregate=True).cuda()
    with torch.no_grad():
        score.bias.copy_(_rand(score.bias.shape, 5))
    aggregate.load_state_dict(score.state_dict())
    assert aggregate.fused_aggregate and aggregate.fused_score and score.fused_score and not score.fused_aggregate
    return score, aggregate


def _bits_equal(a, b):
    return a.shape == b.shape and int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum()) == 0


@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("heads", (1, 4))
@pytest.mark.parametrize("name", ("random", "edge", "cora"))
def test_fused_aggregate_has_the_bits_of_fused_score(pkg, name, heads, concat):
    n, nnz, a = _graph(name)
    n_in, F = 24, 6
    score, aggregate = _layers(n_in, F, heads, concat)
    x0 = _rand((n, n_in), 6) * 4
    gout = _rand((n, heads * F if concat else F), 8)
    got = {}
    for key, layer in (("score", score), ("aggregate", aggregate)):
        x = x0.clone().requires_grad_(True)
        out = layer(x, *a)
        out.backward(gout)
        got[key] = [out.detach(), x.grad] + [p.grad for p in (layer.weight, layer.att_dst, layer.att_src, layer.bias)]
    for what, u, v in zip(("out", "grad_x", "grad_weight", "grad_att_dst", "grad_att_src", "grad_bias"), got["score"], got["aggregate"]):
        assert u is not None and v is not None and bool(torch.isfinite(u).all()), what
        assert float(u.abs().max()) > 0 or what not in ("out", "grad_x"), what
        assert _bits_equal(u, v), (name, heads, concat, what, float((u - v).abs().max()))


def test_nothing_with_nnz_rows_is_saved(pkg):
    """Shapes packed by autograd during the forward: fused_score saves alpha [nnz, H] (so the check sees what it looks for),
    fused_aggregate nothing whose leading dimension is nnz."""
    n, nnz, a = _graph("random")
    assert nnz != n
    score, aggregate = _layers(24, 6, 4, True)
    x0 = _rand((n, 24), 6)
    packed = {}
    for key, layer in (("score", score), ("aggregate", aggregate)):
        shapes = []

        def pack(t, shapes=shapes):
            shapes.append(tuple(t.shape))
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = layer(x0.clone().requires_grad_(True), *a)
        out.sum().backward()
        packed[key] = shapes
    assert any(s and s[0] == nnz for s in packed["score"]), packed["score"]
    assert packed["aggregate"] and not any(s and s[0] == nnz for s in packed["aggregate"]), packed["aggregate"]
    assert (n, 4, 2) in packed["aggregate"], "the statistics: two words per (node, head)"


def test_two_training_steps_on_cora_fused_aggregate(pkg):
    """The example's model as --fused-aggregate builds it on cora, dropout off: the loss is finite and goes down, and it is the loss
    of the --fused-score model to the last bit."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    device = torch.device("cuda")
    edge_index, n_v, n_feat, n_cls = ex.load_edges("cora", device)
    g = ex.gat_graph(edge_index, n_v, device, int32_order=True)
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n_v, n_feat, generator=gen)
    x = (x / x.sum(1, keepdim=True)).to(device)
    y = torch.randint(0, n_cls, (n_v,), generator=gen).to(device)
    train_idx = torch.randperm(n_v, generator=gen)[:20 * n_cls].to(device)
    runs = {}
    for key, kw in (("aggregate", {"fused_aggregate": True}), ("score", {"fused_score": True})):
        torch.manual_seed(0)
        model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, **kw).to(device)
        assert model.conv1.fused_aggregate == (key == "aggregate") and model.conv1.heads == 8 and model.conv2.heads == 1
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)
        model.train()

        def loss_now():
            return torch.nn.functional.nll_loss(model(x, g).index_select(0, train_idx), y[train_idx])

        losses = []
        for _ in range(2):
            opt.zero_grad()
            loss = loss_now()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        with torch.no_grad():
            losses.append(float(loss_now()))  # what the second step did
        runs[key] = losses
    print("losses", runs)
    losses = runs["aggregate"]
    assert all(np.isfinite(losses)) and losses[1] < losses[0] and losses[2] < losses[1], losses
    assert runs["aggregate"] == runs["score"], runs
