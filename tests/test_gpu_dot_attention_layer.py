"""The fused dot-product attention above the kernels, on the GPU: op.DotAttentionFunction against torch autograd in float64 through a
per-edge restatement, op.TransformerConv fused against its composition and both against a float64 model, dropout with one seed in both
paths, the memory a fused step needs — nothing of nnz H words — and two training steps of examples/transformer_custom.py's model, eager
and replayed from a captured graph."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT
from test_gpu_gat import _dev, _rand
from test_gpu_gat_aggregate_layer import _bits_equal
from test_gpu_gat_backward_layer import _graph, _regular_graph

pytestmark = pytest.mark.gpu


def _attention_float64(q, k, v, rows, cols, n, scale, keep=None):
    """The only way torch has: per-edge scores, softmax by scatter, per-edge products — [nnz, H, F] arrays, float64."""
    H = q.shape[1]
    s = (q[rows] * k[cols]).sum(-1) * scale
    top = torch.full((n, H), -float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, rows[:, None].expand(-1, H), s.detach(), "amax")
    t = torch.exp(s - top[rows])  # (softmax does not depend on the shift: no gradient through it)
    alpha = t / torch.zeros((n, H), dtype=s.dtype, device=s.device).index_add_(0, rows, t)[rows]
    if keep is not None:
        alpha = alpha * keep
    return torch.zeros((n, H, q.shape[2]), dtype=s.dtype, device=s.device).index_add_(0, rows, alpha.unsqueeze(-1) * v[cols])


def _close(what, got, want, rel=1e-4, scale=None):
    """max |got - want| <= rel * max |want| — fp32 sums of at most a few hundred terms of one sign pattern against float64. `scale`:
    what stands in for max |want| where want is zero in exact arithmetic."""
    assert got is not None and got.shape == want.shape, what
    err = (got.double() - want).abs().max().item()
    scale = want.abs().max().item() if scale is None else scale
    print("%s: max err %.3e, max |ref| %.3e" % (what, err, scale))
    assert scale > 0 and err <= rel * scale, (what, err, scale)


# ------------------------------------------------------------------------------------------------------------------ the function

@pytest.mark.parametrize("heads", (1, 4))
@pytest.mark.parametrize("name", ("random", "edge", "cora"))
def test_function_against_torch_autograd_in_float64(pkg, name, heads):
    import gespmm_amd

    n, host, a = _graph(name)
    rp, ci, cp, ri, _ = a
    H, F = heads, 6
    q0, k0, v0, gout = _rand((n, H, F), 1) * 4, _rand((n, H, F), 2) * 4, _rand((n, H, F), 3), _rand((n, H, F), 4)
    rows, cols = _dev(host["rows_h"]).long(), ci.long()
    scale = 1.0 / np.sqrt(F)
    q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
    out = gespmm_amd.DotAttentionFunction.apply(q, k, v, rp, ci, cp, ri, None, 0.0, None)
    out.backward(gout)
    x64 = [t.double().requires_grad_(True) for t in (q0, k0, v0)]
    ref = _attention_float64(*x64, rows, cols, n, float(np.float32(scale)))
    ref.backward(gout.double())
    for what, got, want in (("out", out.detach(), ref.detach()), ("grad_q", q.grad, x64[0].grad), ("grad_k", k.grad, x64[1].grad),
                            ("grad_v", v.grad, x64[2].grad)):
        _close("%s H=%d %s" % (name, H, what), got, want)
    # saved: q, k, v, out, stats — nothing of nnz words; the column pass only when k or v asks for it
    shapes = []

    def pack(t):
        shapes.append(tuple(t.shape))
        return t

    calls = []
    real_q, real_kv = gespmm_amd.attention.dot_attention_backward_q, gespmm_amd.attention.dot_attention_backward_kv
    gespmm_amd.attention.dot_attention_backward_q = lambda *x, **kw: (calls.append("q"), real_q(*x, **kw))[1]
    gespmm_amd.attention.dot_attention_backward_kv = lambda *x, **kw: (calls.append("kv"), real_kv(*x, **kw))[1]
    try:
        for need, want_calls in (((True, False, False), ["q"]), ((False, True, False), ["q", "kv"]), ((False, False, True), ["q", "kv"]),
                                 ((True, True, True), ["q", "kv"])):
            del calls[:], shapes[:]
            ts = [t.clone().requires_grad_(r) for t, r in zip((q0, k0, v0), need)]
            with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
                o = gespmm_amd.DotAttentionFunction.apply(*ts, rp, ci, cp, ri, scale, 0.0, None)
            o.backward(gout)
            assert calls == want_calls, (need, calls)
            assert sorted(shapes) == sorted([(n, H, F)] * 4 + [(n, H, 2)]), shapes
            for t, r, g in zip(ts, need, (q.grad, k.grad, v.grad)):
                assert (t.grad is not None) == r and (not r or _bits_equal(t.grad, g))
    finally:
        gespmm_amd.attention.dot_attention_backward_q, gespmm_amd.attention.dot_attention_backward_kv = real_q, real_kv


# --------------------------------------------------------------------------------------------------------------------- the layer

def _transformer_float64(conv, x, rows, cols, n, keep=None):
    H, F = conv.heads, conv.out_channels
    p = {k: v.detach().double().requires_grad_(True) for k, v in conv.named_parameters()}

    def lin(name, t):
        y = t @ p[name + ".weight"].t()
        return y + p[name + ".bias"] if name + ".bias" in p else y

    q, k, v = (lin(m, x).view(n, H, F) for m in ("lin_query", "lin_key", "lin_value"))
    out = _attention_float64(q, k, v, rows, cols, n, float(np.float32(1.0 / np.sqrt(F))), keep)
    out = out.reshape(n, H * F) if conv.concat else out.mean(dim=1)
    if conv.root_weight:
        x_r = lin("lin_skip", x)
        if conv.beta:
            b = torch.sigmoid(torch.cat([out, x_r, out - x_r], dim=-1) @ p["lin_beta.weight"].t())
            out = b * x_r + (1 - b) * out
        else:
            out = out + x_r
    return out, p


@pytest.mark.parametrize("concat,beta,root", ((True, False, True), (True, True, True), (True, False, False), (False, False, True),
                                              (False, True, True), (False, False, False)))
@pytest.mark.parametrize("name", ("random", "cora"))
def test_transformerconv_fused_composition_float64(pkg, name, concat, beta, root):
    import gespmm_amd

    n, host, a = _graph(name)
    n_in, F, heads = 24, 6, 4
    torch.manual_seed(11)
    fused = gespmm_amd.TransformerConv(n_in, F, heads=heads, concat=concat, beta=beta, root_weight=root, fused=True).cuda()
    comp = gespmm_amd.TransformerConv(n_in, F, heads=heads, concat=concat, beta=beta, root_weight=root, fused=False).cuda()
    comp.load_state_dict(fused.state_dict())
    x0 = _rand((n, n_in), 6) * 8
    gout = _rand((n, heads * F if concat else F), 8)
    x64 = x0.double().requires_grad_(True)
    ref, p64 = _transformer_float64(fused, x64, _dev(host["rows_h"]).long(), a[1].long(), n)
    ref.backward(gout.double())
    outs = {}
    for key, conv in (("fused", fused), ("composition", comp)):
        x = x0.clone().requires_grad_(True)
        out = conv(x, *a)
        out.backward(gout)
        outs[key] = out.detach()
        pairs = [("out", out.detach(), ref.detach()), ("grad_x", x.grad, x64.grad)]
        pairs += [("grad_" + k, v.grad, p64[k].grad) for k, v in conv.named_parameters()]
        for what, got, want in pairs:
            # a bias on k moves every score of a row by the same <q, b>: the softmax does not see it, its gradient is zero in exact
            # arithmetic (1e-15 in float64) and rounding noise in fp32 — held to the scale of the query bias's gradient, the same sum
            scale = p64["lin_query.bias"].grad.abs().max().item() if what == "grad_lin_key.bias" else None
            _close("%s concat=%s beta=%s root=%s %s %s" % (name, concat, beta, root, key, what), got, want, scale=scale)
    _close("fused against the composition", outs["fused"], outs["composition"].double())


def test_attention_dropout_one_seed_in_both_paths_and_eval(pkg):
    """Training mode, dropout 0.4, one attn_seed: the fused layer and the composition apply the same mask — both are held to the float64
    model with that mask — a second forward has the bits of the first, another seed has not; eval() ignores dropout: the bits of a
    dropout-free layer, and no dropout launch."""
    import gespmm_amd
    from gespmm_amd import _lib, softmax

    n, host, a = _graph("random")
    p, H, F = 0.4, 4, 6
    seed = torch.tensor([0x12345678, -0x65432110], dtype=torch.int32, device="cuda")
    torch.manual_seed(3)
    layers = {key: gespmm_amd.TransformerConv(24, F, heads=H, dropout=p, fused=key == "fused", attn_seed=seed).cuda()
              for key in ("fused", "composition")}
    layers["composition"].load_state_dict(layers["fused"].state_dict())
    plain = gespmm_amd.TransformerConv(24, F, heads=H, fused=True).cuda()
    plain.load_state_dict(layers["fused"].state_dict())
    s = seed.cpu().numpy().view(np.uint32)
    bits = softmax.restate_edge_dropout_bits(s[0], s[1], host["rows_h"][:, None], host["colind"][:, None], np.arange(H)[None, :])
    keep = _dev((bits >= np.uint32(_lib.edge_dropout_threshold(p))).astype(np.float64)) * float(np.float32(1) / (np.float32(1) - np.float32(p)))
    x0 = _rand((n, 24), 6) * 8
    gout = _rand((n, H * F), 8)
    x64 = x0.double().requires_grad_(True)
    ref, _ = _transformer_float64(layers["fused"], x64, _dev(host["rows_h"]).long(), a[1].long(), n, keep)
    ref.backward(gout.double())
    want_plain = plain(x0, *a).detach()
    for key, conv in layers.items():
        conv.train()
        x = x0.clone().requires_grad_(True)
        out = conv(x, *a)
        out.backward(gout)
        _close(key + " out", out.detach(), ref.detach())
        _close(key + " grad_x", x.grad, x64.grad)
        assert _bits_equal(conv(x0, *a).detach(), out.detach()) and not _bits_equal(out.detach(), want_plain)
        conv.attn_seed = seed + 1
        assert not _bits_equal(conv(x0, *a).detach(), out.detach())
        conv.attn_seed = seed
    calls = []
    real = softmax.edge_dropout
    softmax.edge_dropout = lambda *x, **kw: (calls.append(1), real(*x, **kw))[1]
    try:
        for conv in layers.values():
            conv.eval()
        assert _bits_equal(layers["fused"](x0, *a).detach(), want_plain)
        comp_plain = gespmm_amd.TransformerConv(24, F, heads=H, fused=False).cuda()
        comp_plain.load_state_dict(layers["fused"].state_dict())
        assert _bits_equal(layers["composition"](x0, *a).detach(), comp_plain(x0, *a).detach())
        assert not calls, "eval() must not launch the dropout"
    finally:
        softmax.edge_dropout = real


# ---------------------------------------------------------------------------------------------------------------------- memory

def test_fused_step_allocates_nothing_of_size_nnz_h(pkg):
    """M = K = 2048, 64 entries per row, H = F = 8: ONE [nnz, H] array is 4 MiB, a node-sized [n, H, F] array 512 KiB. The bound is
    derived, not measured: forward plus backward of the fused function allocate out (512 KiB), stats (128 KiB), delta (64 KiB) and the
    three gradients (512 KiB each) — about 2.2 MiB, below ONE [nnz, H] array — while the composition holds the score, alpha, their
    gradients and alpha in CSC order: several. No tensor the fused function saves has nnz H elements."""
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
    q0, k0, v0, gout = _rand((n, H, F), 1), _rand((n, H, F), 2), _rand((n, H, F), 3), _rand((n, H, F), 4)
    scale = 1.0 / np.sqrt(F)
    peaks, grads = {}, {}
    for key in ("fused", "composition"):
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        shapes = []

        def pack(t, shapes=shapes):
            shapes.append(tuple(t.shape))
            return t

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            if key == "fused":
                out = gespmm_amd.DotAttentionFunction.apply(q, k, v, rp, ci, colptr, rowind, scale, 0.0, None)
            else:
                score = gespmm_amd.MultiHeadSDDMMFunction.apply(rp, ci, colptr, rowind, order, q, k) * scale
                alpha = gespmm_amd.EdgeSoftmaxFunction.apply(rp, score, None)
                out = gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, v, alpha, None, True)
        out.backward(gout)
        torch.cuda.synchronize()
        peaks[key] = torch.cuda.max_memory_allocated() - before
        grads[key] = (out.detach(), q.grad, k.grad, v.grad)
        if key == "fused":
            assert shapes and not any(int(np.prod(s)) >= nnz * H for s in shapes), shapes
        else:
            assert any(int(np.prod(s)) == nnz * H for s in shapes), shapes
        del out, q, k, v
    print("peak of forward + backward above the allocation before it: fused %d bytes, composition %d bytes, one [nnz, H] array %d bytes"
          % (peaks["fused"], peaks["composition"], big))
    assert peaks["fused"] < big, peaks
    assert peaks["composition"] > 2 * big, peaks
    for g, w in zip(grads["fused"], grads["composition"]):
        assert float((g - w).abs().max()) <= 1e-4 * float(w.abs().max())


# -------------------------------------------------------------------------------------------------------------------- training

def test_two_training_steps_on_cora_eager_and_captured(pkg):
    """The example's model with --fused on cora, dropout off: the losses are finite and go down, and steps replayed from a captured
    graph (the example's --graph-capture: a capturable Adam, three warm-up steps on a side stream) give the eager losses, bit for bit."""
    import gespmm_amd

    spec = importlib.util.spec_from_file_location("transformer_example", os.path.join(ROOT, "examples", "transformer_custom.py"))
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
    runs = {}
    for key in ("eager", "captured"):
        torch.manual_seed(0)
        model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, fused=True).to(device)
        assert isinstance(model.conv1, gespmm_amd.TransformerConv) and model.conv1.fused and model.conv2.fused
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
