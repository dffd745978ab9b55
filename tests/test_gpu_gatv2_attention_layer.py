"""The fused GATv2 attention above the kernels, on the GPU: op.GATv2AttentionFunction against torch autograd in float64 through a per-edge
restatement, op.GATv2Conv(fused=True) against GATv2Conv(fused=False) with the same parameters, dropout with one seed in both paths, the
memory a fused step needs — nothing of nnz H words — and two training steps of examples/gat_custom.py's model with --v2
--fused-attention, eager and replayed from a captured graph."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT
from test_gpu_dot_attention_layer import _close
from test_gpu_gat import _dev, _rand
from test_gpu_gat_aggregate_layer import _bits_equal
from test_gpu_gat_backward_layer import _graph, _regular_graph

pytestmark = pytest.mark.gpu

SLOPE = 0.2


def _attention_float64(xl, xr, att, rows, cols, n, slope, keep=None):
    """The only way torch has: per-edge [nnz, H, F] sums, softmax by scatter, per-edge products — float64."""
    H = xl.shape[1]
    s = (torch.nn.functional.leaky_relu(xl[rows] + xr[cols], slope) * att).sum(-1)
    top = torch.full((n, H), -float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, rows[:, None].expand(-1, H), s.detach(), "amax")
    t = torch.exp(s - top[rows])  # (softmax does not depend on the shift: no gradient through it)
    alpha = t / torch.zeros((n, H), dtype=s.dtype, device=s.device).index_add_(0, rows, t)[rows]
    if keep is not None:
        alpha = alpha * keep
    return torch.zeros((n, H, xl.shape[2]), dtype=s.dtype, device=s.device).index_add_(0, rows, alpha.unsqueeze(-1) * xr[cols])


# ------------------------------------------------------------------------------------------------------------------ the function

@pytest.mark.parametrize("heads", (1, 4))
@pytest.mark.parametrize("name", ("random", "edge", "cora"))
def test_function_against_torch_autograd_in_float64(pkg, name, heads):
    import gespmm_amd

    n, host, a = _graph(name)
    rp, ci, cp, ri, _ = a
    H, F = heads, 6
    xl0, xr0, att0, gout = _rand((n, H, F), 1) * 2, _rand((n, H, F), 2) * 2, _rand((H, F), 3) * 2, _rand((n, H, F), 4)
    rows, cols = _dev(host["rows_h"]).long(), ci.long()
    assert not bool(((xl0[rows] + xr0[cols]) == 0).any())  # (where torch's derivative of the leaky ReLU differs from the contract's)
    xl, xr, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
    out = gespmm_amd.GATv2AttentionFunction.apply(rp, ci, cp, ri, xl, xr, att, SLOPE, 0.0, None)
    out.backward(gout)
    x64 = [t.double().requires_grad_(True) for t in (xl0, xr0, att0)]
    ref = _attention_float64(*x64, rows, cols, n, float(np.float32(SLOPE)))
    ref.backward(gout.double())
    for what, got, want in (("out", out.detach(), ref.detach()), ("grad_xl", xl.grad, x64[0].grad), ("grad_xr", xr.grad, x64[1].grad),
                            ("grad_att", att.grad, x64[2].grad)):
        _close("%s H=%d %s" % (name, H, what), got, want)
    # saved: xl, xr, att, out, stats — nothing of nnz words; each pass only when asked for: the row pass for any of the three (att_part
    # only for att), the column pass for xr alone
    shapes, calls = [], []

    def pack(t):
        shapes.append(tuple(t.shape))
        return t

    real_row, real_col = gespmm_amd.attention.gatv2_attention_backward_row, gespmm_amd.attention.gatv2_attention_backward_col
    gespmm_amd.attention.gatv2_attention_backward_row = lambda *x, **kw: (calls.append(("row", bool(kw["want_att_part"]))), real_row(*x, **kw))[1]
    gespmm_amd.attention.gatv2_attention_backward_col = lambda *x, **kw: (calls.append(("col",)), real_col(*x, **kw))[1]
    try:
        for need, want_calls in (((True, False, False), [("row", False)]), ((False, True, False), [("row", False), ("col",)]),
                                 ((False, False, True), [("row", True)]), ((True, True, True), [("row", True), ("col",)])):
            del calls[:], shapes[:]
            ts = [t.clone().requires_grad_(r) for t, r in zip((xl0, xr0, att0), need)]
            with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
                o = gespmm_amd.GATv2AttentionFunction.apply(rp, ci, cp, ri, *ts, SLOPE, 0.0, None)
            o.backward(gout)
            assert calls == want_calls, (need, calls)
            assert sorted(shapes) == sorted([(n, H, F)] * 3 + [(H, F), (n, H, 2)]), shapes
            for t, r, g in zip(ts, need, (xl.grad, xr.grad, att.grad)):
                assert (t.grad is not None) == r and (not r or _bits_equal(t.grad, g))
    finally:
        gespmm_amd.attention.gatv2_attention_backward_row, gespmm_amd.attention.gatv2_attention_backward_col = real_row, real_col


def test_function_with_one_tensor_for_both_terms(pkg):
    """xl is xr (shared weights): autograd adds the two gradients — against the float64 model that does the same."""
    import gespmm_amd

    n, host, a = _graph("random")
    rp, ci, cp, ri, _ = a
    H, F = 4, 6
    x0, att0, gout = _rand((n, H, F), 1) * 2, _rand((H, F), 3) * 2, _rand((n, H, F), 4)
    rows, cols = _dev(host["rows_h"]).long(), ci.long()
    assert not bool(((x0[rows] + x0[cols]) == 0).any())
    x, att = x0.clone().requires_grad_(True), att0.clone().requires_grad_(True)
    out = gespmm_amd.GATv2AttentionFunction.apply(rp, ci, cp, ri, x, x, att, SLOPE)
    out.backward(gout)
    x64, att64 = x0.double().requires_grad_(True), att0.double().requires_grad_(True)
    ref = _attention_float64(x64, x64, att64, rows, cols, n, float(np.float32(SLOPE)))
    ref.backward(gout.double())
    for what, got, want in (("out", out.detach(), ref.detach()), ("grad_x", x.grad, x64.grad), ("grad_att", att.grad, att64.grad)):
        _close("shared " + what, got, want)


# --------------------------------------------------------------------------------------------------------------------- the layer

@pytest.mark.parametrize("share", (False, True))
@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("name", ("random", "cora"))
def test_gatv2conv_fused_against_the_composition(pkg, name, concat, share):
    import gespmm_amd

    n, host, a = _graph(name)
    n_in, F, heads = 24, 6, 4
    torch.manual_seed(11)
    fused = gespmm_amd.GATv2Conv(n_in, F, heads=heads, concat=concat, share_weights=share, fused=True).cuda()
    comp = gespmm_amd.GATv2Conv(n_in, F, heads=heads, concat=concat, share_weights=share).cuda()
    with torch.no_grad():
        fused.bias.copy_(_rand(fused.bias.shape, 5))
    comp.load_state_dict(fused.state_dict())
    assert fused.fused and not comp.fused
    x0 = _rand((n, n_in), 6) * 4
    gout = _rand((n, heads * F if concat else F), 8)
    res = {}
    for key, conv in (("fused", fused), ("composition", comp)):
        x = x0.clone().requires_grad_(True)
        # the fused layer does not read csc_order
        out = conv(x, *a) if key == "composition" else conv(x, *a[:4], None)
        out.backward(gout)
        res[key] = dict([("out", out.detach()), ("grad_x", x.grad)] + [("grad_" + k, v.grad) for k, v in conv.named_parameters()])
    assert sorted(res["fused"]) == sorted(res["composition"]) and len(res["fused"]) == (5 if share else 6)
    for what, got in res["fused"].items():
        _close("%s concat=%s share=%s %s" % (name, concat, share, what), got, res["composition"][what].double())


def test_attention_dropout_one_seed_in_both_paths_and_eval(pkg):
    """train(), dropout 0.6, one attn_seed: the fused layer and the composition agree under the layer tests' rule, so they apply the
    same mask (another seed's output is far outside it); a second forward has the bits of the first. eval() ignores dropout: the bits
    of the dropout-free fused layer."""
    import gespmm_amd

    n, _, a = _graph("random")
    p, H, F = 0.6, 4, 6
    seed = torch.tensor([0x12345678, -0x65432110], dtype=torch.int32, device="cuda")
    torch.manual_seed(3)
    layers = {key: gespmm_amd.GATv2Conv(24, F, heads=H, dropout=p, fused=key == "fused").cuda() for key in ("fused", "composition")}
    layers["composition"].load_state_dict(layers["fused"].state_dict())
    plain = gespmm_amd.GATv2Conv(24, F, heads=H, fused=True).cuda()
    plain.load_state_dict(layers["fused"].state_dict())
    x0 = _rand((n, 24), 6) * 4
    gout = _rand((n, H * F), 8)
    want_plain = plain(x0, *a).detach()
    res = {}
    for key, conv in layers.items():
        conv.train()
        x = x0.clone().requires_grad_(True)
        out = conv(x, *a, attn_seed=seed)
        out.backward(gout)
        res[key] = dict([("out", out.detach()), ("grad_x", x.grad)] + [("grad_" + k, v.grad.clone()) for k, v in conv.named_parameters()])
        assert _bits_equal(conv(x0, *a, attn_seed=seed).detach(), out.detach()) and not _bits_equal(out.detach(), want_plain)
    for what, got in res["fused"].items():
        _close("dropout %s" % what, got, res["composition"][what].double())
    other = layers["fused"](x0, *a, attn_seed=seed + 1).detach()
    scale = float(res["composition"]["out"].abs().max())
    assert float((other - res["composition"]["out"]).abs().max()) > 100 * 1e-4 * scale  # another mask is nowhere near
    for conv in layers.values():
        conv.eval()
    assert _bits_equal(layers["fused"](x0, *a, attn_seed=seed).detach(), want_plain)
    assert _bits_equal(layers["fused"](x0, *a).detach(), want_plain)


def test_fused_layer_raises_for_16_bit_features(pkg):
    import gespmm_amd

    n, _, a = _graph("random")
    for dt in (torch.float16, torch.bfloat16):
        conv = gespmm_amd.GATv2Conv(24, 6, heads=4, fused=True).cuda().to(dt)
        with pytest.raises(TypeError, match="gatv2_attention"):
            conv(_rand((n, 24), 6).to(dt), *a)


# ---------------------------------------------------------------------------------------------------------------------- memory

def test_fused_step_allocates_nothing_of_size_nnz_h(pkg):
    """M = K = 2048, 64 entries per row, H = F = 8: ONE [nnz, H] array is 4 MiB, a node-sized [n, H, F] array 512 KiB. The bound is
    derived, not measured: forward plus backward of the fused function allocate out (512 KiB), stats (128 KiB), delta (64 KiB), grad_xl,
    att_part and grad_xr (512 KiB each) and grad_att (256 bytes) — about 2.2 MiB, below ONE [nnz, H] array — while the composition
    holds the score, alpha and their gradients: several. No tensor the fused function saves has nnz H elements."""
    import gespmm_amd
    from gespmm_amd import graphs

    n, deg, H, F = 2048, 64, 8, 8
    rowptr, colind = _regular_graph(n, deg, 9)
    nnz = n * deg
    big = nnz * H * 4
    assert nnz == 131072 and big == 4 << 20 and n * H * F * 4 * 8 <= big
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    order = order.to(torch.int32)
    xl0, xr0, att0, gout = _rand((n, H, F), 1), _rand((n, H, F), 2), _rand((H, F), 3), _rand((n, H, F), 4)
    peaks, grads = {}, {}
    for key in ("fused", "composition"):
        xl, xr, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
        shapes = []

        def pack(t, shapes=shapes):
            shapes.append(tuple(t.shape))
            return t

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            if key == "fused":
                out = gespmm_amd.GATv2AttentionFunction.apply(rp, ci, colptr, rowind, xl, xr, att, SLOPE, 0.0, None)
            else:
                score = gespmm_amd.GATv2ScoreFunction.apply(rp, ci, colptr, rowind, order, xl, xr, att, SLOPE)
                alpha = gespmm_amd.EdgeSoftmaxFunction.apply(rp, score, None)
                out = gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, xr, alpha, None, True)
        out.backward(gout)
        torch.cuda.synchronize()
        peaks[key] = torch.cuda.max_memory_allocated() - before
        grads[key] = (out.detach(), xr.grad, att.grad)
        if key == "fused":
            assert shapes and not any(int(np.prod(s)) >= nnz * H for s in shapes), shapes
        else:
            assert any(int(np.prod(s)) == nnz * H for s in shapes), shapes
        del out, xl, xr, att
    print("peak of forward + backward above the allocation before it: fused %d bytes, composition %d bytes, one [nnz, H] array %d bytes"
          % (peaks["fused"], peaks["composition"], big))
    assert peaks["fused"] < big, peaks
    assert peaks["composition"] > 2 * big, peaks
    for g, w in zip(grads["fused"], grads["composition"]):
        assert float((g - w).abs().max()) <= 1e-4 * float(w.abs().max())


# -------------------------------------------------------------------------------------------------------------------- training

def test_two_training_steps_on_cora_eager_and_captured(pkg):
    """The example's model with --v2 --fused-attention on cora, dropout off: the losses are finite and go down, and steps replayed from a
    captured graph (the example's --graph-capture: a capturable Adam, three warm-up steps on a side stream) give the eager losses."""
    import gespmm_amd

    spec = importlib.util.spec_from_file_location("gat_example_fused_v2", os.path.join(ROOT, "examples", "gat_custom.py"))
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
    y_train = y[train_idx]
    with pytest.raises(ValueError):
        ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, fused_attention=True)  # GATv2Conv's path: it needs v2=True
    runs = {}
    for key in ("eager", "captured"):
        torch.manual_seed(0)
        model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, v2=True, fused_attention=True).to(device)
        assert isinstance(model.conv1, gespmm_amd.GATv2Conv) and model.conv1.fused and model.conv2.fused
        assert model.conv1.heads == 8 and model.conv1.out_channels == 8 and model.conv2.heads == 1
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4, capturable=True)
        model.train()

        def train_step():
            opt.zero_grad(set_to_none=False)
            loss = torch.nn.functional.nll_loss(model(x, g).index_select(0, train_idx), y_train)
            loss.backward()
            opt.step()
            return loss

        losses = []
        if key == "eager":
            for _ in range(5):
                losses.append(float(train_step().detach()))
        else:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(3):
                    losses.append(float(train_step().detach()))
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_loss = train_step()
            for _ in range(2):
                graph.replay()
                losses.append(float(static_loss.detach()))
        runs[key] = losses
    print("losses", runs)
    for losses in runs.values():
        assert all(np.isfinite(losses)) and losses[1] < losses[0] and losses[2] < losses[1] and losses[4] < losses[2], runs
    assert runs["captured"] == runs["eager"], runs
