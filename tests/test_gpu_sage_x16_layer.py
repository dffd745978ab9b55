"""SpmmMaxFunction and SAGEConv (mean / gcn / pool) on fp16 / bf16 features, bit for bit: the function against the dense float64 maximum
(a max rounds nothing) and against the narrowed gradient of the fp32 function on the widened inputs; the layer against its documented
steps written with the ops (forward) and with the autograd functions (gradients); the fp32 layer against the fp32 functions composed by
hand, unchanged. No tolerance anywhere. The graph is the one of tests/test_gpu_sage_layer.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import ROOT
from test_gpu_sage_layer import N_V, _dense, _dense_max, _device_graph, _graph

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)


def _name(dt):
    return "f16" if dt == torch.float16 else "bf16"


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.detach().contiguous().view(view), b.detach().contiguous().view(view))


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_spmm_max_function_on_16_bit_features(pkg, dt):
    from gespmm_amd import SpmmMaxFunction

    rowptr, colind = _graph()
    g, A = _device_graph(rowptr, colind), _dense(rowptr, colind)
    x16 = torch.from_numpy(np.random.default_rng(3).standard_normal((N_V, 24)).astype(np.float32)).to(dt).cuda()
    w16 = torch.randn(N_V, 24, generator=torch.Generator().manual_seed(4)).to(dt).cuda()
    x = x16.clone().requires_grad_(True)
    empty = -8192.0  # (a value both types hold: rows without a winner store it as it is)
    out = SpmmMaxFunction.apply(*g, x, empty)
    assert out.dtype == dt
    out.backward(w16)
    # the forward: exactly the dense float64 maximum
    ref = _dense_max(A, x16.double(), empty)
    assert torch.equal(out.detach().double(), ref)
    assert (out[0] == empty).all().item() and (out[-1] == empty).all().item() and not (out == empty).all().item()
    # the gradient: narrow(the fp32 function's gradient on the widened inputs)
    xw = x16.float().requires_grad_(True)
    SpmmMaxFunction.apply(*g, xw, empty).backward(w16.float())
    assert x.grad.dtype == dt and _same_bits(x.grad, xw.grad.to(dt))
    assert x.grad.float().abs().sum().item() > 0
    # saves arg and nothing floating-point
    out2 = SpmmMaxFunction.apply(*g, x)
    saved = out2.grad_fn.saved_tensors
    assert [t.dtype for t in saved if t.dim() == 2] == [torch.int32] and not any(t.is_floating_point() for t in saved)


def _steps_with_ops(aggregator, P, x, g, dt):
    """SAGEConv's documented steps on 16-bit features, written with the ops and torch's linears (forward only)."""
    from gespmm_amd import spmm

    rp, ci, cp, ri, order = g
    lin = lambda name, t: F.linear(t, P[name + ".weight"], P.get(name + ".bias"))  # noqa: E731
    degree = torch.diff(rp).to(torch.float32)
    if aggregator == "pool":
        h_neigh, _ = spmm.csr_spmm_max_arg_x16(rp, ci, torch.relu(lin("fc_pool", x)).contiguous(), empty_value=0.0)
        return lin("fc_self", x) + lin("fc_neigh", h_neigh)
    if aggregator == "gcn":
        h_sum = spmm.csr_spmm_no_edge_value(rp, ci, x)
        return lin("fc_neigh", (h_sum + x) * (1 / (degree + 1)).to(dt).unsqueeze(1))
    inv_deg = torch.where(degree > 0, 1 / degree, torch.zeros_like(degree))
    w_csr = torch.repeat_interleave(inv_deg, torch.diff(rp), output_size=ci.numel())
    assert w_csr.dtype == torch.float32
    return lin("fc_self", x) + lin("fc_neigh", spmm.csr_spmm(rp, ci, w_csr, x))


def _steps_with_functions(aggregator, P, x, g, dt):
    """The same steps written with the autograd functions: what the gradients are compared with."""
    from gespmm_amd import SPMMFunction, SpmmMaxFunction

    rp, ci, cp, ri, order = g
    lin = lambda name, t: F.linear(t, P[name + ".weight"], P.get(name + ".bias"))  # noqa: E731
    degree = torch.diff(rp).to(torch.float32)
    if aggregator == "pool":
        return lin("fc_self", x) + lin("fc_neigh", SpmmMaxFunction.apply(rp, ci, cp, ri, order, torch.relu(lin("fc_pool", x)), 0.0))
    if aggregator == "gcn":
        h_sum = SPMMFunction.apply(rp, ci, cp, ri, x)
        return lin("fc_neigh", (h_sum + x) * (1 / (degree + 1)).to(dt).unsqueeze(1))
    inv_deg = torch.where(degree > 0, 1 / degree, torch.zeros_like(degree))
    w_csr = torch.repeat_interleave(inv_deg, torch.diff(rp), output_size=ci.numel())
    w_csc = inv_deg.index_select(0, ri)
    return lin("fc_self", x) + lin("fc_neigh", SPMMFunction.apply(rp, ci, cp, ri, x, w_csr, w_csc))


@pytest.mark.parametrize("aggregator", ("mean", "gcn", "pool"))
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_sage_conv_16_bit_equals_its_documented_steps(pkg, dt, aggregator):
    from gespmm_amd import SAGEConv

    torch.manual_seed(5)
    rowptr, colind = _graph()
    g = _device_graph(rowptr, colind)
    conv = SAGEConv(12, 7, aggregator).cuda().to(dt)
    assert all(p.dtype == dt for p in conv.parameters())
    x16 = torch.randn(N_V, 12).to(dt).cuda()
    w16 = torch.randn(N_V, 7).to(dt).cuda()
    x = x16.clone().requires_grad_(True)
    out = conv(x, *g)
    assert out.dtype == dt and out.shape == (N_V, 7) and torch.isfinite(out.float()).all().item()
    out.backward(w16)

    P = {n: p.detach().clone().requires_grad_(True) for n, p in conv.named_parameters()}
    with torch.no_grad():
        assert _same_bits(out, _steps_with_ops(aggregator, P, x16, g, dt)), "forward differs from the steps written with the ops"
    xr = x16.clone().requires_grad_(True)
    ref = _steps_with_functions(aggregator, P, xr, g, dt)
    assert _same_bits(out, ref)
    ref.backward(w16)
    assert x.grad.dtype == dt and _same_bits(x.grad, xr.grad) and x.grad.float().abs().sum().item() > 0
    for n, p in conv.named_parameters():
        assert p.grad is not None and p.grad.dtype == dt and _same_bits(p.grad, P[n].grad), n
    if aggregator == "mean":  # the valued product: rows without entries aggregate 0, the others the mean within one rounding of it
        A = _dense(rowptr, colind)
        deg = A.sum(1, keepdim=True)
        from gespmm_amd import spmm

        degree = torch.diff(g[0]).to(torch.float32)
        inv_deg = torch.where(degree > 0, 1 / degree, torch.zeros_like(degree))
        h_neigh = spmm.csr_spmm(g[0], g[1], torch.repeat_interleave(inv_deg, torch.diff(g[0]), output_size=g[1].numel()), x16)
        mean64 = (A @ x16.double()) / deg.clamp(min=1)
        # one rounding to the type (half an ulp: 2^-11 / 2^-8 of the value), plus the fp32 chain and weights (2^-20 of the mean of
        # |x|, far below it), plus fp16's subnormal spacing: twice the first, of the mean of |x|, bounds them all
        eps = 2.0 ** (-10 if dt == torch.float16 else -7)
        bound = eps * (A @ x16.double().abs()) / deg.clamp(min=1) + 2.0 ** -24
        assert ((h_neigh.double() - mean64).abs() <= bound).all().item()
        assert (h_neigh[deg.view(-1) == 0] == 0).all().item()


def test_sage_conv_pool_under_autocast_aggregates_bf16(pkg, monkeypatch):
    from gespmm_amd import SAGEConv, spmm

    rowptr, colind = _graph()
    g = _device_graph(rowptr, colind)
    seen = []
    real = spmm.csr_spmm_max_arg_x16

    def spy(rowptr, colind, dense, **kw):
        seen.append(dense.dtype)
        return real(rowptr, colind, dense, **kw)

    monkeypatch.setattr(spmm, "csr_spmm_max_arg_x16", spy)
    torch.manual_seed(6)
    for aggregator in ("pool", "mean", "gcn"):
        conv = SAGEConv(12, 7, aggregator).cuda()
        x = torch.randn(N_V, 12, device="cuda", requires_grad=True)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            out = conv(x, *g)
        out.float().sum().backward()
        assert torch.isfinite(out.float()).all().item() and x.grad is not None and x.grad.dtype == torch.float32
        assert all(p.grad is not None and p.dtype == torch.float32 for p in conv.parameters())
        assert seen == [torch.bfloat16], (aggregator, seen)  # pool alone aggregates what a linear produced: the fp32 x of mean / gcn stays fp32


@pytest.mark.parametrize("aggregator", ("mean", "gcn", "pool"))
def test_fp32_sage_conv_is_unchanged(pkg, aggregator):
    """The fp32 layer is the fp32 functions composed as before: the fused product with row_scale = 1 / deg, the plain sum divided by
    deg + 1, the fp32 max with empty_value = 0 — bit for bit, forward and gradients."""
    from gespmm_amd import FusedGCNFunction, SAGEConv, SPMMFunction, SpmmMaxFunction

    torch.manual_seed(5)
    rowptr, colind = _graph()
    g = _device_graph(rowptr, colind)
    rp, ci, cp, ri, order = g
    conv = SAGEConv(12, 7, aggregator).cuda()
    x0 = torch.randn(N_V, 12, device="cuda")
    w = torch.randn(N_V, 7, device="cuda")
    x = x0.clone().requires_grad_(True)
    out = conv(x, *g)
    out.backward(w)
    P = {n: p.detach().clone().requires_grad_(True) for n, p in conv.named_parameters()}
    lin = lambda name, t: F.linear(t, P[name + ".weight"], P[name + ".bias"])  # noqa: E731
    xr = x0.clone().requires_grad_(True)
    degree = torch.diff(rp).to(torch.float32)
    if aggregator == "mean":
        inv_deg = torch.where(degree > 0, 1 / degree, torch.zeros_like(degree))
        ref = lin("fc_self", xr) + lin("fc_neigh", FusedGCNFunction.apply(rp, ci, cp, ri, xr, None, inv_deg, None))
    elif aggregator == "gcn":
        ref = lin("fc_neigh", (SPMMFunction.apply(rp, ci, cp, ri, xr.contiguous()) + xr) / (degree + 1).unsqueeze(1))
    else:
        ref = lin("fc_self", xr) + lin("fc_neigh", SpmmMaxFunction.apply(rp, ci, cp, ri, order, torch.relu(lin("fc_pool", xr)), 0.0))
    ref.backward(w)
    assert out.dtype == torch.float32 and _same_bits(out, ref) and _same_bits(x.grad, xr.grad)
    for n, p in conv.named_parameters():
        assert _same_bits(p.grad, P[n].grad), n


@pytest.mark.parametrize("capture", (False, True), ids=("eager", "graph-capture"))
@pytest.mark.parametrize("aggregator", ("pool", "mean"))
def test_the_example_trains_in_bf16(pkg, aggregator, capture):
    """examples/sage_custom.py --dtype bf16 in a child process: ten epochs on cora, dropout 0, a fixed seed — it exits 0 and the loss is
    finite and lower at the end than after the first epoch."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "sage_custom.py"), "--dataset", "cora", "--aggregator-type", aggregator,
           "--n-epochs", "10", "--dropout", "0", "--seed", "0", "--dtype", "bf16"] + (["--graph-capture"] if capture else [])
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    losses = [float(x) for x in re.findall(r"^Epoch \d+ \| Loss ([-+.\deinfa]+)$", run.stdout, flags=re.M)]
    assert len(losses) == 10, run.stdout[-2000:]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert "Test Accuracy" in run.stdout
