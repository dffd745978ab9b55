"""GATv2 on the GPU above the kernels: op.GATv2ScoreFunction against torch's own composition in float64, op.GATv2Conv against a float64
restatement of the layer, the memory the score's forward and backward need — nothing of size [nnz, H, F] — and two training steps of
examples/gat_custom.py's model with --v2, eager and replayed from a captured graph."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT
from test_gatv2_host import restate_backward, restate_score
from test_gpu_gat import _dev, _rand
from test_gpu_gat_aggregate_layer import _bits_equal
from test_gpu_gat_backward_layer import _graph, _regular_graph

pytestmark = pytest.mark.gpu


def _composition(xl, xr, att, rows, cols, slope):
    """The only way torch has: the [nnz, H, F] sum, materialised."""
    t = xl[rows] + xr[cols]
    return ((t if slope is None else torch.nn.functional.leaky_relu(t, slope)) * att).sum(-1)


# ------------------------------------------------------------------------------------------------------------------ the function

@pytest.mark.parametrize("slope", (None, 0.2))
@pytest.mark.parametrize("heads", (1, 4))
@pytest.mark.parametrize("name", ("random", "edge"))
def test_function_against_torch_autograd_in_float64(pkg, name, heads, slope):
    """score and the three gradients inside 1e-4 max(|ref|, sum |terms|) of torch.autograd through the float64 composition; the terms
    come from the numpy restatement (for grad_att: summed over the nodes). No t is exactly zero, where torch's derivative of the leaky
    ReLU (slope) differs from ours (1)."""
    import gespmm_amd

    n, host, a = _graph(name)
    H, F = heads, 6
    xl0, xr0, att0, gs = _rand((n, H, F), 1) * 2, _rand((n, H, F), 2) * 2, _rand((H, F), 3) * 4, _rand((host["nnz"], H), 4)
    rows, cols = _dev(host["rows_h"]).long(), a[1].long()
    assert not bool(((xl0[rows] + xr0[cols]) == 0).any())
    xl, xr, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
    score = gespmm_amd.GATv2ScoreFunction.apply(*a, xl, xr, att, slope)
    score.backward(gs)
    x64 = [t.double().requires_grad_(True) for t in (xl0, xr0, att0)]
    slope32 = None if slope is None else float(np.float32(slope))
    ref = _composition(*x64, rows, cols, slope32)
    ref.backward(gs.double())
    rowptr, colptr, rowind, order = (t.cpu().numpy() for t in (a[0], a[2], a[3], a[4]))
    h = [t.cpu().numpy() for t in (xl0, xr0, att0, gs)]
    _, terms = restate_score(rowptr, host["colind"], h[0], h[1], h[2], slope32)
    _, _, tx, ta = restate_backward(rowptr, host["colind"], h[3], h[0], h[1], h[2], slope32)
    _, _, tr, _ = restate_backward(colptr, rowind, h[3], h[1], h[0], h[2], slope32, order=order)
    for what, got, want, tm in (("score", score.detach(), ref.detach(), terms), ("grad_xl", xl.grad, x64[0].grad, tx),
                                ("grad_xr", xr.grad, x64[1].grad, tr), ("grad_att", att.grad, x64[2].grad, ta.sum(0))):
        assert got is not None and got.shape == want.shape, what
        want = want.cpu().numpy()
        bound = 1e-4 * np.maximum(np.abs(want), tm)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        worst = float((err / np.where(bound > 0, bound, 1.0)).max())
        print("%s H=%d slope=%s %s: worst error / bound %.4g" % (name, H, slope, what, worst))
        assert np.all(err <= bound), (name, H, slope, what, worst)
    # each pass only when asked for: the row pass for xl or att, the column pass for xr
    calls = []
    real = gespmm_amd.sddmm.gatv2_score_backward

    def counted(*args, **kw):
        calls.append((kw.get("order") is not None, bool(kw.get("want_att_part"))))
        return real(*args, **kw)

    gespmm_amd.sddmm.gatv2_score_backward = counted
    try:
        for need, want_calls in (((True, False, False), [(False, False)]), ((False, True, False), [(True, False)]),
                                 ((False, False, True), [(False, True)]), ((True, True, True), [(False, True), (True, False)])):
            del calls[:]
            ts = [t.clone().requires_grad_(r) for t, r in zip((xl0, xr0, att0), need)]
            gespmm_amd.GATv2ScoreFunction.apply(*a, *ts, slope).backward(gs)
            assert calls == want_calls, (need, calls)
            for t, r, g in zip(ts, need, (xl.grad, xr.grad, att.grad)):
                assert (t.grad is not None) == r and (not r or _bits_equal(t.grad, g))
    finally:
        gespmm_amd.sddmm.gatv2_score_backward = real


# --------------------------------------------------------------------------------------------------------------------- the layer

def _gatv2_float64(x, w_dst, w_src, att, bias, rows, cols, n, H, F, concat, slope):
    xl, xr = (x @ w_dst).view(n, H, F), (x @ w_src).view(n, H, F)
    e = (torch.nn.functional.leaky_relu(xl[rows] + xr[cols], slope) * att).sum(-1)
    top = torch.full((n, H), -float("inf"), dtype=e.dtype, device=e.device).scatter_reduce(0, rows[:, None].expand(-1, H), e.detach(), "amax")
    t = torch.exp(e - top[rows])  # (softmax does not depend on the shift: no gradient through it)
    alpha = t / torch.zeros((n, H), dtype=e.dtype, device=e.device).index_add_(0, rows, t)[rows]
    out = torch.zeros((n, H, F), dtype=e.dtype, device=e.device).index_add_(0, rows, alpha.unsqueeze(-1) * xr[cols])
    out = out.reshape(n, H * F) if concat else out.mean(dim=1)
    return out + bias


@pytest.mark.parametrize("share", (False, True))
@pytest.mark.parametrize("concat", (True, False))
@pytest.mark.parametrize("name", ("random", "cora"))
def test_gatv2conv_against_float64(pkg, name, concat, share):
    import gespmm_amd

    n, host, a = _graph(name)
    n_in, F, heads = 24, 6, 4
    torch.manual_seed(11)
    conv = gespmm_amd.GATv2Conv(n_in, F, heads=heads, concat=concat, negative_slope=0.2, share_weights=share).cuda()
    with torch.no_grad():
        conv.bias.copy_(_rand(conv.bias.shape, 5))  # (zeros by default: give its gradient a forward to agree with)
    assert conv.att.shape == (1, heads, F) and conv.bias.shape == ((heads * F,) if concat else (F,))
    assert (conv.weight_dst is conv.weight_src) == share and conv.weight_src.shape == (n_in, heads * F)
    x = (_rand((n, n_in), 6) * 4).requires_grad_(True)
    gout = _rand((n, heads * F if concat else F), 8)
    out = conv(x, *a)
    out.backward(gout)
    names = ("weight_src", "att", "bias") + (() if share else ("weight_dst",))
    p64 = {k: getattr(conv, k).detach().double().requires_grad_(True) for k in names}
    x64 = x.detach().double().requires_grad_(True)
    ref = _gatv2_float64(x64, p64["weight_src" if share else "weight_dst"], p64["weight_src"], p64["att"], p64["bias"],
                         _dev(host["rows_h"]).long(), a[1].long(), n, heads, F, concat, float(np.float32(0.2)))
    ref.backward(gout.double())
    pairs = [("out", out.detach(), ref.detach()), ("grad_x", x.grad, x64.grad)]
    pairs += [("grad_" + k, getattr(conv, k).grad, p64[k].grad) for k in names]
    for what, got, want in pairs:
        assert got is not None and got.shape == want.shape, what
        err, scale = (got.double() - want).abs().max().item(), want.abs().max().item()
        print("%s concat=%s share=%s %s: max err %.3e, max |ref| %.3e" % (name, concat, share, what, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, (name, concat, share, what, err, scale)


def test_attention_dropout_and_eval(pkg):
    """dropout=0.6 with a fixed attn_seed: two training forwards have equal bits (and differ from the undropped layer); eval() makes
    exactly the launches of dropout=0 — no dropout call — and gives its bits."""
    import gespmm_amd

    n, _, a = _graph("random")
    torch.manual_seed(3)
    drop = gespmm_amd.GATv2Conv(24, 6, heads=4, dropout=0.6).cuda()
    plain = gespmm_amd.GATv2Conv(24, 6, heads=4).cuda()
    plain.load_state_dict(drop.state_dict())
    x = _rand((n, 24), 6) * 4
    seed = torch.tensor([0x12345678, -0x65432110], dtype=torch.int32, device="cuda")
    calls = []
    real = gespmm_amd.softmax.edge_dropout

    def counted(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    gespmm_amd.softmax.edge_dropout = counted
    try:
        drop.train()
        first, second = drop(x, *a, attn_seed=seed).detach(), drop(x, *a, attn_seed=seed).detach()
        assert len(calls) == 2 and _bits_equal(first, second)
        other = drop(x, *a, attn_seed=seed + 1).detach()
        want = plain(x, *a).detach()
        assert not _bits_equal(first, want) and not _bits_equal(first, other)
        xg = x.clone().requires_grad_(True)
        drop(xg, *a, attn_seed=seed).sum().backward()  # the op is its own adjoint: one more call
        assert len(calls) == 5 and bool(torch.isfinite(xg.grad).all())
        del calls[:]
        drop.eval()
        assert _bits_equal(drop(x, *a, attn_seed=seed).detach(), want) and _bits_equal(drop(x, *a).detach(), want)
        plain.train()
        assert _bits_equal(plain(x, *a, attn_seed=seed).detach(), want)
        assert not calls, "eval() or dropout == 0 must not launch the dropout"
    finally:
        gespmm_amd.softmax.edge_dropout = real


# ---------------------------------------------------------------------------------------------------------------------- memory

def test_score_allocates_nothing_of_size_nnz_h_f(pkg):
    """M = K = 2048, 64 entries per row, H = F = 8: ONE [nnz, H, F] array is 32 MiB. The bound is derived, not measured — the op holds
    the 4 MiB score, its 4 MiB gradient (the caller's) and node-sized tensors (512 KiB each: contiguous copies none, grad_xl, att_part,
    grad_xr) — so the peak of forward plus backward above what was allocated before is below ONE such array, while torch's composition
    on the same inputs needs several. No saved tensor has nnz H F elements."""
    import gespmm_amd
    from gespmm_amd import graphs

    n, deg, H, F = 2048, 64, 8, 8
    rowptr, colind = _regular_graph(n, deg, 9)
    nnz = n * deg
    big = nnz * H * F * 4
    assert nnz == 131072 and big == 32 << 20
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    a = (rp, ci, colptr, rowind, order.to(torch.int32))
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), deg)
    cols = ci.long()
    xl0, xr0, att0, gs = _rand((n, H, F), 1), _rand((n, H, F), 2), _rand((H, F), 3), _rand((nnz, H), 4)
    print("exact zeros among the %d sums t: %d" % (nnz * H * F, int(((xl0[rows] + xr0[cols]) == 0).sum())))
    peaks, grads = {}, {}
    for key in ("op", "torch"):
        xl, xr, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
        shapes = []

        def pack(t, shapes=shapes):
            shapes.append(tuple(t.shape))
            return t

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            if key == "op":
                score = gespmm_amd.GATv2ScoreFunction.apply(*a, xl, xr, att, 0.2)
            else:
                score = _composition(xl, xr, att, rows, cols, 0.2)
        score.backward(gs)
        torch.cuda.synchronize()
        peaks[key] = torch.cuda.max_memory_allocated() - before
        grads[key] = (score.detach(), xl.grad, xr.grad, att.grad)
        if key == "op":
            assert shapes and not any(int(np.prod(s)) >= nnz * H * F for s in shapes), shapes
        else:
            assert any(int(np.prod(s)) == nnz * H * F for s in shapes), shapes
        del score, xl, xr, att
    print("peak of forward + backward above the allocation before it: op %d bytes, torch composition %d bytes, one [nnz, H, F] array %d "
          "bytes" % (peaks["op"], peaks["torch"], big))
    assert peaks["op"] < big, peaks
    assert peaks["torch"] > big, peaks
    # the same numbers, to fp32 rounding of sums of up to 64 x 8 terms: the score and grad_att — among 8 M sums t some are exactly
    # zero, where torch's derivative of the leaky ReLU differs from ours, so grad_xl and grad_xr are left to the tests above
    for g, w in ((grads["op"][0], grads["torch"][0]), (grads["op"][3], grads["torch"][3])):
        assert float((g - w).abs().max()) <= 1e-3 * float(w.abs().max())


# -------------------------------------------------------------------------------------------------------------------- training

def test_two_training_steps_on_cora_v2_eager_and_captured(pkg):
    """The example's model as --v2 builds it on cora, dropout off: the losses are finite and go down, and a step replayed from a
    captured graph (the example's --graph-capture: a capturable Adam, three warm-up steps on a side stream) gives the eager losses."""
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
    y_train = y[train_idx]
    with pytest.raises(ValueError):
        ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, v2=True, fused_score=True)
    runs = {}
    for key in ("eager", "captured"):
        torch.manual_seed(0)
        model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, v2=True).to(device)
        import gespmm_amd

        assert isinstance(model.conv1, gespmm_amd.GATv2Conv) and isinstance(model.conv2, gespmm_amd.GATv2Conv)
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
