"""GATConv(dropout=p) on the GPU: dropout on the attention coefficients in all four paths of the layer. Under one ``attn_seed`` the
outputs of the default, fused_score, fused_aggregate and fused_backward paths are bit-equal and all gradients are inside the
project's bound of a float64 layer that applies the numpy restatement of the mask; ``eval()`` and ``dropout=0`` are today's layer; the
drawn seed follows torch's generator; the fused backward still allocates nothing of size nnz H; and the example model trains."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT
from test_edge_dropout_host import restate
from test_gpu_gat import _dev, _rand
from test_gpu_gat_aggregate_layer import _bits_equal
from test_gpu_gat_backward_layer import _graph, _regular_graph

pytestmark = pytest.mark.gpu

P = 0.6
PAIR = (0x12345678, 0x9ABCDEF0)
PATHS = (("default", {}), ("score", {"fused_score": True}), ("aggregate", {"fused_aggregate": True}), ("backward", {"fused_backward": True}))
NAMES = ("out", "grad_x", "grad_weight", "grad_att_dst", "grad_att_src", "grad_bias")


def _seed(pair=PAIR):
    return _dev(np.array(pair, dtype=np.uint32).view(np.int32))


def _layers(n_in, F, heads, concat, dropout=P):
    import gespmm_amd

    torch.manual_seed(7 + heads)
    layers = {key: gespmm_amd.GATConv(n_in, F, heads=heads, concat=concat, negative_slope=0.2, dropout=dropout, **kw).cuda()
              for key, kw in PATHS}
    with torch.no_grad():
        layers["default"].bias.copy_(_rand(layers["default"].bias.shape, 5))
    for key in ("score", "aggregate", "backward"):
        layers[key].load_state_dict(layers["default"].state_dict())
    return layers


def _run(layer, x0, a, gout, **kw):
    for p in layer.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    out = layer(x, *a, **kw)
    out.backward(gout)
    return [out.detach(), x.grad] + [p.grad for p in (layer.weight, layer.att_dst, layer.att_src, layer.bias)]


def _gat_float64_dropout(x, W, att_dst, att_src, bias, rows, cols, n, H, F, concat, slope, d):
    """tests/test_gpu_gat.py's float64 layer with alpha multiplied by d [nnz, H] (0 or 1 / (1 - p)) after the normalisation."""
    xw = (x @ W).view(n, H, F)
    el, er = (xw * att_dst).sum(-1), (xw * att_src).sum(-1)
    e = torch.nn.functional.leaky_relu(el[rows] + er[cols], slope)
    top = torch.full((n, H), -float("inf"), dtype=e.dtype, device=e.device).scatter_reduce(0, rows[:, None].expand(-1, H), e.detach(), "amax")
    t = torch.exp(e - top[rows])
    alpha = t / torch.zeros((n, H), dtype=e.dtype, device=e.device).index_add_(0, rows, t)[rows]
    out = torch.zeros((n, H, F), dtype=e.dtype, device=e.device).index_add_(0, rows, (alpha * d).unsqueeze(-1) * xw[cols])
    out = out.reshape(n, H * F) if concat else out.mean(dim=1)
    return out + bias


@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("heads", (1, 4))
@pytest.mark.parametrize("name", ("random", "cora"))
def test_four_paths_one_mask(pkg, name, heads, concat):
    from gespmm_amd import _lib

    n, host, a = _graph(name)
    n_in, F = 24, 6
    layers = _layers(n_in, F, heads, concat)
    x0 = _rand((n, n_in), 6) * 4
    gout = _rand((n, heads * F if concat else F), 8)
    seed = _seed()
    got = {key: _run(layer.train(), x0, a, gout, attn_seed=seed) for key, layer in layers.items()}
    for key in ("score", "aggregate", "backward"):
        assert _bits_equal(got[key][0], got["default"][0]), (key, "output")
    for what, u, v in zip(NAMES, got["aggregate"], got["score"]):
        assert u is not None and _bits_equal(u, v), ("fused_aggregate vs fused_score", what)
    # float64 with the numpy mask
    keep = restate(PAIR[0], PAIR[1], host["rows_h"].astype(np.uint64)[:, None], host["colind"].astype(np.uint64)[:, None],
                   np.arange(heads, dtype=np.uint64)[None, :]) >= np.uint32(_lib.edge_dropout_threshold(P))
    assert 0.3 < keep.mean() < 0.5
    d = _dev(np.where(keep, float(np.float32(1.0) / (np.float32(1.0) - np.float32(P))), 0.0))
    ref_layer = layers["default"]
    p64 = [p.detach().double().requires_grad_(True) for p in (ref_layer.weight, ref_layer.att_dst, ref_layer.att_src, ref_layer.bias)]
    x64 = x0.double().requires_grad_(True)
    ref = _gat_float64_dropout(x64, *p64, _dev(host["rows_h"]).long(), a[1].long(), n, heads, F, concat, float(np.float32(0.2)), d)
    ref.backward(gout.double())
    refs = [ref.detach(), x64.grad] + [q.grad for q in p64]
    for key in got:
        for what, g, want in zip(NAMES, got[key], refs):
            assert g is not None and g.shape == want.shape, (key, what)
            err, scale = (g.double() - want).abs().max().item(), want.abs().max().item()
            print("%s heads=%d concat=%s %s %s: max err %.3e, max |ref| %.3e" % (name, heads, concat, key, what, err, scale))
            assert scale > 0 and err <= 1e-4 * scale, (name, heads, concat, key, what, err, scale)
    # the mask is on: the output differs from the layer without dropout
    plain = _run(layers["aggregate"].eval(), x0, a, gout)
    assert not _bits_equal(plain[0], got["aggregate"][0])


@pytest.mark.parametrize("key,kw", PATHS)
def test_eval_and_dropout_zero_are_todays_layer(pkg, key, kw):
    """No dropout entry point is reached: they are made to raise, and the results have the bits of a layer built without the argument."""
    import gespmm_amd
    from gespmm_amd import _lib

    n, host, a = _graph("random")
    n_in, F, heads = 24, 6, 4
    torch.manual_seed(11)
    today = gespmm_amd.GATConv(n_in, F, heads=heads, negative_slope=0.2, **kw).cuda()
    x0, gout = _rand((n, n_in), 6) * 4, _rand((n, heads * F), 8)
    want = _run(today, x0, a, gout)

    class Refuse:
        def __init__(self, real):
            self.real = real

        def __getattr__(self, name):
            if "dropout" in name:
                raise AssertionError("%s was called" % name)
            return getattr(self.real, name)

    from gespmm_amd import softmax, spmm

    real = _lib.lib
    try:
        softmax.lib = spmm.lib = Refuse(real)
        for dropout, mode in ((P, "eval"), (0.0, "train")):
            layer = gespmm_amd.GATConv(n_in, F, heads=heads, negative_slope=0.2, dropout=dropout, **kw).cuda()
            layer.load_state_dict(today.state_dict())
            getattr(layer, mode)()
            for extra in ({}, {"attn_seed": _seed()}):
                got = _run(layer, x0, a, gout, **extra)
                for what, u, v in zip(NAMES, got, want):
                    assert _bits_equal(u, v), (key, dropout, mode, what)
        with pytest.raises(AssertionError):  # the witness: in training mode with p > 0 the refused entry points ARE what is called
            layer = gespmm_amd.GATConv(n_in, F, heads=heads, negative_slope=0.2, dropout=P, **kw).cuda().train()
            _run(layer, x0, a, gout)
    finally:
        softmax.lib = spmm.lib = real


@pytest.mark.parametrize("key,kw", (PATHS[0], PATHS[3]))
def test_drawn_seed_follows_torchs_generator(pkg, key, kw):
    import gespmm_amd

    n, host, a = _graph("random")
    torch.manual_seed(3)
    layer = gespmm_amd.GATConv(24, 6, heads=4, negative_slope=0.2, dropout=P, **kw).cuda().train()
    x = _rand((n, 24), 6) * 4
    with torch.no_grad():
        torch.manual_seed(100)
        first, second = layer(x, *a), layer(x, *a)
        torch.manual_seed(100)
        again = layer(x, *a)
    assert _bits_equal(first, again), "the same torch.manual_seed gives the same mask"
    assert not _bits_equal(first, second), "two consecutive forwards draw two seeds"


def test_fused_backward_with_dropout_allocates_nothing_edge_sized(pkg):
    """tests/test_gpu_gat_backward_layer.py's measure with dropout on: M = K = 2048, 64 entries per row, H = F = 8, one [nnz, H] array
    is 4 MiB. No saved tensor has nnz rows (the seed's two words are the only addition) and the backward's peak stays under one such
    array; the default backward, as the witness, shows at least three."""
    import gespmm_amd
    from gespmm_amd import graphs

    n, deg, H, F = 2048, 64, 8, 8
    rowptr, colind = _regular_graph(n, deg, 9)
    nnz = n * deg
    edge_bytes = nnz * H * 4
    assert edge_bytes == 4 << 20
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    a = (rp, ci, colptr, rowind, order.to(torch.int32))
    el0, er0, feat0, gout = _rand((n, H), 1) * 8, _rand((n, H), 2) * 8, _rand((n, H, F), 3), _rand((n, H, F), 4)
    seed = _seed()
    peaks, grads = {}, {}
    for fused in (True, False):
        el, er, feat = (t.clone().requires_grad_(True) for t in (el0, er0, feat0))
        shapes = []

        def pack(t, shapes=shapes):
            shapes.append(tuple(t.shape))
            return t

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = gespmm_amd.GATAggregateFunction.apply(*a, el, er, feat, 0.2, fused, P, seed)
        assert (2,) in shapes and not any(s and s[0] == nnz for s in shapes), shapes
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out.backward(gout)
        torch.cuda.synchronize()
        peaks[fused] = torch.cuda.max_memory_allocated() - before
        grads[fused] = (out.detach(), feat.grad, el.grad, er.grad)
        del out, el, er, feat
    print("peak of backward above the allocation before it: fused %d bytes, default %d bytes, one [nnz, H] array %d bytes" % (
        peaks[True], peaks[False], edge_bytes))
    assert peaks[True] < edge_bytes, peaks
    assert peaks[False] >= 3 * edge_bytes, peaks
    assert _bits_equal(grads[True][0], grads[False][0]) and _bits_equal(grads[True][1], grads[False][1])
    for u, v in zip(grads[True][2:], grads[False][2:]):
        assert float((u - v).abs().max()) <= 1e-4 * float(v.abs().max())


def test_two_training_steps_on_cora_with_attention_dropout(pkg):
    """The example's model as --fused-backward --attn-dropout 0.6 builds it on cora, feature dropout off: finite losses, equal to the
    --fused-aggregate model's to the digits the example prints."""
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
        model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, attn_dropout=P, **kw).to(device)
        assert model.conv1.dropout == model.conv2.dropout == P and model.conv1.fused_backward == (key == "backward")
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)
        model.train()
        losses = []
        for _ in range(2):
            opt.zero_grad()
            loss = torch.nn.functional.nll_loss(model(x, g).index_select(0, train_idx), y[train_idx])
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        runs[key] = losses
    print("losses", runs)
    assert all(np.isfinite(v) for r in runs.values() for v in r), runs
    assert ["%.4f" % v for v in runs["backward"]] == ["%.4f" % v for v in runs["aggregate"]], runs
