"""SpmmMaxFunction and SAGEConv (mean / gcn / pool) against a dense float64 restatement in torch: the output and the gradients of x and
of every parameter, within the margin of the attention-layer tests — |got - ref| <= 1e-4 * max|ref| per compared tensor. The max is
differentiable as a function only where one candidate holds it: the inputs are checked on the CPU to have no ties (zeros after the
relu of the pool aggregator aside: they never win against empty_value = 0 and pass no gradient through the relu either way)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT
from max_arg_ref import max_arg_forward, tied_words

pytestmark = pytest.mark.gpu

N_V = 203


def _graph():
    """A square pattern on 203 nodes without repeated entries: rows of 0 .. 9 entries, the first, the last and a few others empty."""
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 10, size=N_V)
    deg[[0, 17, 18, N_V - 1]] = 0
    rows = [np.sort(rng.choice(N_V, size=d, replace=False)) for d in deg]
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    colind = np.concatenate(rows).astype(np.int32)
    return rowptr, colind


def _device_graph(rowptr, colind):
    from gespmm_amd import graphs

    rp, ci = torch.from_numpy(rowptr).cuda(), torch.from_numpy(colind).cuda()
    cp, ri, order = graphs.transpose_csr(rp, ci, K=N_V, return_order=True)
    return rp, ci, cp, ri, order.to(torch.int32)


def _dense(rowptr, colind):
    A = torch.zeros(N_V, N_V, dtype=torch.float64)
    rows = np.repeat(np.arange(N_V), np.diff(rowptr))
    A[torch.from_numpy(rows), torch.from_numpy(colind).long()] = 1.0
    return A.cuda()


def _close(name, got, ref):
    err = (got.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert scale > 0 and err <= 1e-4 * scale, (name, err, scale)


def _dense_max(A, m, empty):
    """max over the neighbours of each row, `empty` where nothing exceeds it — float64, differentiable through amax"""
    cand = torch.where(A.unsqueeze(2) > 0, m.unsqueeze(0), torch.full((), float("-inf"), dtype=m.dtype, device=m.device))
    return torch.clamp(cand.amax(1), min=empty)


def test_spmm_max_function(pkg):
    from gespmm_amd import SpmmMaxFunction

    rowptr, colind = _graph()
    g, A = _device_graph(rowptr, colind), _dense(rowptr, colind)
    x_h = np.random.default_rng(3).standard_normal((N_V, 24)).astype(np.float32)
    C, arg = max_arg_forward(rowptr, colind, x_h, -10000.0)
    assert not tied_words(rowptr, colind, x_h, C, arg).any()
    x = torch.from_numpy(x_h).cuda().requires_grad_(True)
    out = SpmmMaxFunction.apply(*g, x)
    w = torch.randn(N_V, 24, device="cuda")
    (out * w).sum().backward()
    xr = torch.from_numpy(x_h).double().cuda().requires_grad_(True)
    ref = _dense_max(A, xr, -10000.0)
    (ref * w.double()).sum().backward()
    assert torch.equal(out.detach().double(), ref.detach())  # a max rounds nothing
    assert (out[0] == -10000.0).all().item() and (out[-1] == -10000.0).all().item()
    _close("grad_x", x.grad, xr.grad)
    # saves arg and nothing of feat's size in floats; once differentiable
    out2 = SpmmMaxFunction.apply(*g, x)
    saved = out2.grad_fn.saved_tensors
    assert [t.dtype for t in saved if t.dim() == 2] == [torch.int32] and not any(t.dtype == torch.float32 for t in saved)
    (gx,) = torch.autograd.grad(out2.sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


@pytest.mark.parametrize("aggregator", ("mean", "gcn", "pool"))
def test_sage_conv_against_dense_float64(pkg, aggregator):
    from gespmm_amd import SAGEConv

    torch.manual_seed(5)
    rowptr, colind = _graph()
    g, A = _device_graph(rowptr, colind), _dense(rowptr, colind)
    conv = SAGEConv(12, 7, aggregator, activation=torch.relu).cuda()
    x_h = torch.randn(N_V, 12)
    if aggregator == "pool":  # no two neighbours of a row hold the same POSITIVE pooled value
        m_h = torch.relu(x_h @ conv.fc_pool.weight.detach().cpu().t() + conv.fc_pool.bias.detach().cpu()).numpy()
        C, arg = max_arg_forward(rowptr, colind, m_h, 0.0)
        assert (arg >= 0).any() and not tied_words(rowptr, colind, m_h, C, arg).any()
    x = x_h.cuda().requires_grad_(True)
    out = conv(x, *g)
    w = torch.randn(N_V, 7, device="cuda")
    (out * w).sum().backward()

    P = {n: p.detach().double().requires_grad_(True) for n, p in conv.named_parameters()}
    xr = x_h.double().cuda().requires_grad_(True)
    lin = lambda name, t: t @ P[name + ".weight"].t() + P[name + ".bias"]  # noqa: E731
    deg = A.sum(1, keepdim=True)
    if aggregator == "mean":
        ref = lin("fc_self", xr) + lin("fc_neigh", (A @ xr) / deg.clamp(min=1))
    elif aggregator == "gcn":
        ref = lin("fc_neigh", (A @ xr + xr) / (deg + 1))
    else:
        ref = lin("fc_self", xr) + lin("fc_neigh", _dense_max(A, torch.relu(lin("fc_pool", xr)), 0.0))
    ref = torch.relu(ref)
    (ref * w.double()).sum().backward()
    _close("out", out.detach(), ref.detach())
    _close("grad_x", x.grad, xr.grad)
    for n, p in conv.named_parameters():
        _close(n, p.grad, P[n].grad)
    assert sorted(n.split(".")[0] for n, _ in conv.named_parameters() if n.endswith("weight")) == {
        "mean": ["fc_neigh", "fc_self"], "gcn": ["fc_neigh"], "pool": ["fc_neigh", "fc_pool", "fc_self"]}[aggregator]


def test_sage_conv_options(pkg):
    from gespmm_amd import SAGEConv

    with pytest.raises(ValueError):
        SAGEConv(4, 4, "lstm")
    with pytest.raises(ValueError):
        SAGEConv(4, 4, "sum")
    rowptr, colind = _graph()
    g = _device_graph(rowptr, colind)
    x = torch.randn(N_V, 6, device="cuda")
    with pytest.raises(ValueError):
        SAGEConv(6, 3, "pool").cuda()(x, *g[:4])  # pool needs csc_order
    assert SAGEConv(6, 3, "mean").cuda()(x, *g[:4]).shape == (N_V, 3)
    with pytest.raises(ValueError):
        SAGEConv(6, 3, "mean").cuda()(x[:-1], *g)
    for aggregator in ("mean", "pool"):
        conv = SAGEConv(6, 3, aggregator, feat_drop=0.5, bias=False, norm=torch.nn.LayerNorm(3).cuda()).cuda()
        assert conv.fc_self.bias is None and conv.fc_neigh.bias is None
        conv.eval()  # feat_drop is off in eval(): two calls agree bit for bit, and equal feat_drop = 0
        a, b = conv(x, *g), conv(x, *g)
        assert torch.equal(a, b)
        plain = SAGEConv(6, 3, aggregator, feat_drop=0.0, bias=False, norm=conv.norm).cuda()
        plain.load_state_dict(conv.state_dict())
        assert torch.equal(plain(x, *g), a)
        conv.train()  # ... and on in train(): the generator decides, the same seed the same mask
        torch.manual_seed(1)
        c = conv(x, *g)
        torch.manual_seed(1)
        d = conv(x, *g)
        torch.manual_seed(2)
        e = conv(x, *g)
        assert torch.equal(c, d) and not torch.equal(c, e) and not torch.equal(c, a)


@pytest.mark.parametrize("aggregator", ("pool", "mean"))
def test_the_example_trains(pkg, aggregator):
    """examples/sage_custom.py in a child process: ten epochs on cora, dropout 0, a fixed seed — it exits 0 and the loss is finite and
    lower at the end than after the first epoch."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "sage_custom.py"), "--dataset", "cora", "--aggregator-type", aggregator,
           "--n-epochs", "10", "--dropout", "0", "--seed", "0"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    losses = [float(x) for x in re.findall(r"^Epoch \d+ \| Loss ([-+.\deinfa]+)$", run.stdout, flags=re.M)]
    assert len(losses) == 10, run.stdout[-2000:]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert "Test Accuracy" in run.stdout
