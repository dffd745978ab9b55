"""GATAggregateFunction(fused_backward=True) and GATConv(fused_backward=True) on the GPU: the forward and the feature gradient are the
default's bit for bit (the same launches), the gradients of the two score terms are inside the project's bound of a float64
restatement — as are the default's, in the same test — the backward allocates nothing of size nnz H (measured, with the default as
the witness that the measure sees such arrays), and two training steps of the example model follow the --fused-aggregate model's."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from attention_refs import gat_backward_float64
from helpers import ROOT
from test_gpu_gat import _dev, _gat_float64, _rand, _random_graph
from test_gpu_gat_aggregate_layer import _bits_equal, _cora, _square_edge

pytestmark = pytest.mark.gpu


def _graph(name):
    """-> (n, host dict for gat_backward_float64, the five device index tensors GATConv.forward takes)"""
    from gespmm_amd import graphs

    if name == "random":
        rowptr, colind, _ = _random_graph(300)
        n = 300
    else:
        n, rowptr, colind = _square_edge() if name == "edge" else _cora()
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    host = {"M": n, "K": n, "nnz": int(colind.size), "colind": np.asarray(colind),
            "rows_h": np.repeat(np.arange(n, dtype=np.int32), np.diff(rowptr))}
    return n, host, (rp, ci, colptr, rowind, order.to(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the function

@pytest.mark.parametrize("slope", (None, 0.2))
@pytest.mark.parametrize("heads", (1, 4))
@pytest.mark.parametrize("name", ("random", "edge"))
def test_function_fused_backward_against_the_default(pkg, name, heads, slope):
    import gespmm_amd

    n, host, a = _graph(name)
    H, F = heads, 6
    el0, er0, feat0 = _rand((n, H), 1) * 8, _rand((n, H), 2) * 8, _rand((n, H, F), 3)
    gout = _rand((n, H, F), 4)
    got = {}
    for fused in (False, True):
        el, er, feat = (t.clone().requires_grad_(True) for t in (el0, er0, feat0))
        out = gespmm_amd.GATAggregateFunction.apply(*a, el, er, feat, slope, fused)
        out.backward(gout)
        got[fused] = (out.detach(), feat.grad, el.grad, er.grad)
        assert el.grad.shape == (n, H) and er.grad.shape == (n, H)
    assert _bits_equal(got[True][0], got[False][0]), "forward"
    assert _bits_equal(got[True][1], got[False][1]), "grad_feat: the same launch"
    ref_el, ref_er, sc_el, sc_er = gat_backward_float64(host["rows_h"], host["colind"], n, n, el0.cpu().numpy(), er0.cpu().numpy(),
                                                        gout.cpu().numpy(), feat0.cpu().numpy(), slope)
    for fused in (True, False):
        for what, g, ref, scale in (("grad_el", got[fused][2], ref_el, sc_el), ("grad_er", got[fused][3], ref_er, sc_er)):
            bound = 1e-4 * np.maximum(np.abs(ref), scale)
            err = np.abs(g.cpu().numpy().astype(np.float64) - ref)
            worst = float((err / np.where(bound > 0, bound, 1.0)).max())
            print("%s H=%d slope=%s fused_backward=%s %s: worst error / bound %.4f" % (name, H, slope, fused, what, worst))
            assert np.all(err <= bound), (name, H, slope, fused, what, worst)
    # each gradient only when asked for; the second launch only for er
    el, er, feat = el0.clone().requires_grad_(True), er0.clone(), feat0.clone()
    gespmm_amd.GATAggregateFunction.apply(*a, el, er, feat, slope, True).backward(gout)
    assert _bits_equal(el.grad, got[True][2]) and er.grad is None and feat.grad is None
    el, er, feat = el0.clone(), er0.clone().requires_grad_(True), feat0.clone()
    gespmm_amd.GATAggregateFunction.apply(*a, el, er, feat, slope, True).backward(gout)
    assert _bits_equal(er.grad, got[True][3]) and el.grad is None


# --------------------------------------------------------------------------------------------------------------------- the layer

@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("name", ("random", "cora"))
def test_gatconv_fused_backward_against_float64(pkg, name, concat):
    import gespmm_amd

    n, host, a = _graph(name)
    n_in, F, heads = 24, 6, 4
    torch.manual_seed(7 + heads)
    layers = {"aggregate": gespmm_amd.GATConv(n_in, F, heads=heads, concat=concat, negative_slope=0.2, fused_aggregate=True).cuda(),
              "backward": gespmm_amd.GATConv(n_in, F, heads=heads, concat=concat, negative_slope=0.2, fused_backward=True).cuda()}
    with torch.no_grad():
        layers["aggregate"].bias.copy_(_rand(layers["aggregate"].bias.shape, 5))
    layers["backward"].load_state_dict(layers["aggregate"].state_dict())
    fb = layers["backward"]
    assert fb.fused_backward and fb.fused_aggregate and fb.fused_score and not layers["aggregate"].fused_backward
    x0 = _rand((n, n_in), 6) * 4
    gout = _rand((n, heads * F if concat else F), 8)
    got = {}
    for key, layer in layers.items():
        x = x0.clone().requires_grad_(True)
        out = layer(x, *a)
        out.backward(gout)
        got[key] = [out.detach(), x.grad] + [p.grad for p in (layer.weight, layer.att_dst, layer.att_src, layer.bias)]
    assert _bits_equal(got["backward"][0], got["aggregate"][0]), "the forward is the same two launches"
    params = [fb.weight, fb.att_dst, fb.att_src, fb.bias]
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    x64 = x0.double().requires_grad_(True)
    ref = _gat_float64(x64, *p64, _dev(host["rows_h"]).long(), a[1].long(), n, heads, F, concat, float(np.float32(0.2)))
    ref.backward(gout.double())
    refs = [ref.detach(), x64.grad] + [q.grad for q in p64]
    for key in ("backward", "aggregate"):
        for what, g, want in zip(("out", "grad_x", "grad_weight", "grad_att_dst", "grad_att_src", "grad_bias"), got[key], refs):
            assert g is not None and g.shape == want.shape, what
            err, scale = (g.double() - want).abs().max().item(), want.abs().max().item()
            print("%s concat=%s %s %s: max err %.3e, max |ref| %.3e" % (name, concat, key, what, err, scale))
            assert scale > 0 and err <= 1e-4 * scale, (name, concat, key, what, err, scale)


# ---------------------------------------------------------------------------------------------------------------------- memory

def _regular_graph(n, deg, seed):
    """n rows of exactly `deg` distinct, sorted columns."""
    rng = np.random.RandomState(seed)
    cols = np.sort(np.argsort(rng.rand(n, n), axis=1)[:, :deg], axis=1).astype(np.int32)
    return np.arange(n + 1, dtype=np.int32) * deg, cols.reshape(-1)


def test_backward_allocates_nothing_edge_sized(pkg):
    """M = K = 2048, 64 entries per row, H = F = 8: one [nnz, H] array is 4 MiB, everything node-sized the backward makes (grad_feat
    512 KiB, delta, grad_el, grad_er 64 KiB each) under 2 MiB. The peak of backward() above what was allocated before it is below
    ONE such array with fused_backward=True — and at least three with the default, so the measure sees what it is meant to see."""
    import gespmm_amd
    from gespmm_amd import graphs

    n, deg, H, F = 2048, 64, 8, 8
    rowptr, colind = _regular_graph(n, deg, 9)
    nnz = n * deg
    edge_bytes = nnz * H * 4
    assert nnz == 131072 and edge_bytes == 4 << 20
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    a = (rp, ci, colptr, rowind, order.to(torch.int32))
    el0, er0, feat0, gout = _rand((n, H), 1) * 8, _rand((n, H), 2) * 8, _rand((n, H, F), 3), _rand((n, H, F), 4)
    assert gout.is_contiguous()
    peaks = {}
    for fused in (True, False):
        el, er, feat = (t.clone().requires_grad_(True) for t in (el0, er0, feat0))
        shapes = []

        def pack(t, shapes=shapes):
            shapes.append(tuple(t.shape))
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = gespmm_amd.GATAggregateFunction.apply(*a, el, er, feat, 0.2, fused)
        assert shapes and not any(s and s[0] == nnz for s in shapes), shapes
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out.backward(gout)
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - before
        assert el.grad is not None and er.grad is not None and feat.grad is not None
        del out, el, er, feat
    print("peak of backward above the allocation before it: fused %d bytes, default %d bytes, one [nnz, H] array %d bytes" % (
        peaks[True], peaks[False], edge_bytes))
    assert peaks[True] < edge_bytes, peaks
    assert peaks[False] >= 3 * edge_bytes, peaks


# -------------------------------------------------------------------------------------------------------------------- training

def test_two_training_steps_on_cora_fused_backward(pkg):
    """The example's model as --fused-backward builds it on cora, dropout off: the losses are finite, go down, and are within 1e-4
    relative of the --fused-aggregate model's."""
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
    for key, kw in (("backward", {"fused_backward": True}), ("aggregate", {"fused_aggregate": True})):
        torch.manual_seed(0)
        model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, **kw).to(device)
        assert model.conv1.fused_backward == (key == "backward") and model.conv1.fused_aggregate and model.conv2.heads == 1
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
    losses = runs["backward"]
    assert all(np.isfinite(losses)) and losses[1] < losses[0] and losses[2] < losses[1], losses
    for u, v in zip(runs["backward"], runs["aggregate"]):
        assert abs(u - v) <= 1e-4 * abs(v), runs
