"""GATConv(fused_score=True) on the GPU: the same output bits as the default layer, every gradient against the float64 torch
restatement of tests/test_gpu_gat.py within its margin (|got - ref| <= 1e-4 * max|ref| per tensor), and two training steps of the
example model with --fused-score's settings."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT
from test_gpu_gat import _dev, _gat_float64, _rand, _random_graph

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("heads", (1, 4))
def test_fused_gatconv_against_default_and_float64(pkg, heads, concat):
    import gespmm_amd
    from gespmm_amd import graphs

    n, n_in, F = 300, 24, 6
    rowptr, colind, rows_h = _random_graph(n)
    assert 1900 <= colind.size <= 2100 and np.diff(rowptr).min() >= 1
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    torch.manual_seed(7 + heads)
    plain = gespmm_amd.GATConv(n_in, F, heads=heads, concat=concat, negative_slope=0.2).cuda()
    fused = gespmm_amd.GATConv(n_in, F, heads=heads, concat=concat, negative_slope=0.2, fused_score=True).cuda()
    with torch.no_grad():
        plain.bias.copy_(_rand(plain.bias.shape, 5))
    fused.load_state_dict(plain.state_dict())
    assert fused.fused_score and not plain.fused_score
    x0 = _rand((n, n_in), 6) * 4
    gout = _rand((n, heads * F if concat else F), 8)
    want = plain(x0, rp, ci, colptr, rowind, order)
    x = x0.clone().requires_grad_(True)
    for od in (order, order.to(torch.int32)):  # the int64 order of transpose_csr, and the int32 one the kernels take as it is
        out = fused(x, rp, ci, colptr, rowind, od)
        assert int((out.detach().view(torch.int32) != want.detach().view(torch.int32)).sum()) == 0, "fused_score changes the output bits"
    out.backward(gout)
    params = [fused.weight, fused.att_dst, fused.att_src, fused.bias]
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    x64 = x0.double().requires_grad_(True)
    ref = _gat_float64(x64, *p64, _dev(rows_h).long(), ci.long(), n, heads, F, concat, float(np.float32(0.2)))
    ref.backward(gout.double())
    pairs = [("grad_x", x.grad, x64.grad)]
    pairs += [("grad_" + name, p.grad, q.grad) for name, p, q in zip(("weight", "att_dst", "att_src", "bias"), params, p64)]
    for name, got, ref_g in pairs:
        assert got is not None and got.shape == ref_g.shape, name
        err, scale = (got.double() - ref_g).abs().max().item(), ref_g.abs().max().item()
        print("%s: max err %.3e, max |ref| %.3e" % (name, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, (name, err, scale)


def test_two_training_steps_on_cora_fused(pkg):
    """The example's model as --fused-score builds it (fused layers, an int32 edge order made once) on cora, dropout off: the loss is
    finite and goes down."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    device = torch.device("cuda")
    edge_index, n_v, n_feat, n_cls = ex.load_edges("cora", device)
    g = ex.gat_graph(edge_index, n_v, device, int32_order=True)
    assert g["csc_order"].dtype == torch.int32
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n_v, n_feat, generator=gen)
    x = (x / x.sum(1, keepdim=True)).to(device)
    y = torch.randint(0, n_cls, (n_v,), generator=gen).to(device)
    train_idx = torch.randperm(n_v, generator=gen)[:20 * n_cls].to(device)
    torch.manual_seed(0)
    model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, fused_score=True).to(device)
    assert model.conv1.fused_score and model.conv2.fused_score and model.conv1.heads == 8 and model.conv2.heads == 1
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
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[1] < losses[0] and losses[2] < losses[1], losses
