"""GATv2 on 16-bit features above the kernels: GATv2ScoreFunction on fp16 / bf16 node terms is WIRING — forward and every gradient are
bit-equal to the direct ``sddmm.gatv2_score_x16`` / ``gatv2_score_backward_x16`` calls it is documented to make (the ops themselves are
pinned in tests/test_gpu_gatv2_x16.py) — GATv2Conv as a ``.half()`` / ``.bfloat16()`` layer is bit-equal to the hand composition of its
documented steps, in eval and in training, and runs the 16-bit score under autocast; one numeric check against float64; and training
steps of examples/gat_custom.py's model with --v2 in bf16, eager and replayed from a captured graph."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT
from test_gpu_attention_x16_layers import DTYPES, IDS, _bits_equal, _rand, square  # noqa: F401  (square: the fixture)

pytestmark = pytest.mark.gpu

H, F = 4, 8


# ------------------------------------------------------------------------------------------------------------------ the function

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("slope", (None, 0.2))
def test_function_is_the_direct_op_calls(pkg, square, dtype, slope):
    import gespmm_amd
    from gespmm_amd import sddmm

    G = square
    gen = torch.Generator(device="cuda").manual_seed(21)
    xl = _rand(gen, G["n"], H, F).to(dtype).requires_grad_(True)
    xr = _rand(gen, G["n"], H, F).to(dtype).requires_grad_(True)
    att = (4 * _rand(gen, H, F)).requires_grad_(True)
    gs = _rand(gen, G["nnz"], H)
    score = gespmm_amd.GATv2ScoreFunction.apply(*G["args"], xl, xr, att, slope)
    assert score.dtype == torch.float32 and score.shape == (G["nnz"], H)
    a, b, w = xl.detach(), xr.detach(), att.detach()
    _bits_equal(score.detach(), sddmm.gatv2_score_x16(G["rp"], G["ci"], a, b, w, negative_slope=slope), "forward")
    score.backward(gs)
    assert xl.grad.dtype == dtype and xr.grad.dtype == dtype and att.grad.dtype == torch.float32
    gxl, part = sddmm.gatv2_score_backward_x16(G["rp"], G["ci"], gs, a, b, w, negative_slope=slope, want_att_part=True)
    gxr = sddmm.gatv2_score_backward_x16(G["colptr"], G["rowind"], gs, b, a, w, negative_slope=slope, order=G["order32"])
    assert part.dtype == torch.float32
    _bits_equal(xl.grad, gxl, "grad_xl")
    _bits_equal(xr.grad, gxr, "grad_xr")
    _bits_equal(att.grad, part.sum(0), "grad_att")
    # xl is xr (shared weights): autograd adds the two gradients, in the operands' dtype
    x = b.clone().requires_grad_(True)
    gespmm_amd.GATv2ScoreFunction.apply(*G["args"], x, x, w, slope).backward(gs)
    one = sddmm.gatv2_score_backward_x16(G["rp"], G["ci"], gs, b, b, w, negative_slope=slope)
    two = sddmm.gatv2_score_backward_x16(G["colptr"], G["rowind"], gs, b, b, w, negative_slope=slope, order=G["order32"])
    assert x.grad.dtype == dtype
    _bits_equal(x.grad, one + two, "xl is xr")
    # att must be fp32; the node terms one 16-bit type
    with pytest.raises(TypeError):
        gespmm_amd.GATv2ScoreFunction.apply(*G["args"], a, b, w.to(dtype), slope)
    with pytest.raises(TypeError):
        gespmm_amd.GATv2ScoreFunction.apply(*G["args"], a, b.float(), w, slope)
    with pytest.raises(TypeError):
        gespmm_amd.GATv2ScoreFunction.apply(*G["args"], a.half(), b.bfloat16(), w, slope)


# --------------------------------------------------------------------------------------------------------------------- the layer

def _forward_by_hand(layer, x, G, p=0.0, seed=None):
    """The documented steps of a 16-bit GATv2Conv on the ops themselves."""
    from gespmm_amd import sddmm, softmax, spmm

    n = x.shape[0]
    xr = (x @ layer.weight_src).view(n, H, F)
    xl = xr if layer.share_weights else (x @ layer.weight_dst).view(n, H, F)
    assert xl.dtype == x.dtype and xr.dtype == x.dtype
    score = sddmm.gatv2_score_x16(G["rp"], G["ci"], xl.contiguous(), xr.contiguous(), layer.att.view(H, F).float(),
                                  negative_slope=layer.negative_slope)
    alpha = softmax.edge_softmax(G["rp"], score)
    if seed is not None:
        alpha = softmax.edge_dropout(G["rp"], G["ci"], alpha, p, seed)
    assert score.dtype == torch.float32 and alpha.dtype == torch.float32
    out = spmm.csr_spmm_heads_x16(G["rp"], G["ci"], alpha, xr.contiguous())
    return out.reshape(n, H * F) + layer.bias


def _step_by_hand(layer, x, G, p=0.0, seed=None):
    """The same steps as autograd functions, on the layer's own parameters -> the output (gradients arrive by backward)."""
    import gespmm_amd

    n = x.shape[0]
    xr = (x @ layer.weight_src).view(n, H, F)
    xl = xr if layer.share_weights else (x @ layer.weight_dst).view(n, H, F)
    score = gespmm_amd.GATv2ScoreFunction.apply(*G["args"], xl, xr, layer.att.view(H, F).float(), layer.negative_slope)
    alpha = gespmm_amd.EdgeSoftmaxFunction.apply(G["rp"], score, None)
    if seed is not None:
        alpha = gespmm_amd.EdgeDropoutFunction.apply(G["rp"], G["ci"], alpha, p, seed)
    out = gespmm_amd.MultiHeadSPMMFunction.apply(*G["args"], xr, alpha, None, True)
    return out.reshape(n, H * F) + layer.bias


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("share", (False, True))
def test_gatv2conv_16_bit_is_its_documented_steps(pkg, square, dtype, share):
    """eval, and training with dropout=0.5 under a fixed attn_seed: the output is bit-equal to the steps on the ops themselves, and the
    gradients of x, both weights, att and bias are bit-equal to those of the same steps written with the autograd functions."""
    import gespmm_amd

    G = square
    torch.manual_seed(31)
    layer = gespmm_amd.GATv2Conv(12, F, heads=H, dropout=0.5, share_weights=share).cuda().to(dtype)
    with torch.no_grad():
        layer.bias.copy_(torch.rand_like(layer.bias) - 0.5)
    twin = copy.deepcopy(layer)
    x0 = (torch.rand(G["n"], 12, device="cuda") - 0.5).to(dtype)
    go = (torch.rand(G["n"], H * F, device="cuda") - 0.5).to(dtype)
    seed = torch.tensor([0x12345678, -0x65432110], dtype=torch.int32, device="cuda")
    names = [n for n, _ in layer.named_parameters()]
    assert sorted(names) == sorted(["weight_src", "att", "bias"] + ([] if share else ["weight_dst"]))
    outs = {}
    for mode in ("eval", "train"):
        layer.train(mode == "train")
        twin.train(mode == "train")
        p, s = (0.5, seed) if mode == "train" else (0.0, None)
        layer.zero_grad()
        twin.zero_grad()
        x, xt = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        out = layer(x, *G["args"], attn_seed=seed)
        assert out.dtype == dtype and out.shape == (G["n"], H * F)
        with torch.no_grad():
            _bits_equal(out.detach(), _forward_by_hand(layer, x0, G, p, s), mode + " output")
        out.backward(go)
        _step_by_hand(twin, xt, G, p, s).backward(go)
        _bits_equal(x.grad, xt.grad, mode + " grad_x")
        for name in names:
            g, gt = getattr(layer, name).grad, getattr(twin, name).grad
            assert g is not None and g.dtype == dtype and g.shape == getattr(layer, name).shape, name
            assert bool(torch.isfinite(g).all()) and bool((g != 0).any()), name
            _bits_equal(g, gt, "%s grad_%s" % (mode, name))
        outs[mode] = out.detach()
    assert not torch.equal(outs["eval"], outs["train"]), "dropout changed nothing"
    layer.eval()
    _bits_equal(layer(x0, *G["args"]).detach(), outs["eval"], "eval without a seed")


def test_gatv2conv_autocast_runs_the_16_bit_score(pkg, square, monkeypatch):
    """fp32 parameters under torch.autocast(bfloat16): x @ W comes out bf16, so the score op that runs is the _x16 one — once forward,
    and both gradient passes on the _x16 backward — with an fp32 att; the fp32 ops are not called."""
    import gespmm_amd
    from gespmm_amd import sddmm

    G = square
    torch.manual_seed(32)
    layer = gespmm_amd.GATv2Conv(12, F, heads=H).cuda()
    x = torch.rand(G["n"], 12, device="cuda") - 0.5
    calls = []

    def spy(name):
        real = getattr(sddmm, name)

        def f(*args, **kw):
            r = real(*args, **kw)
            node, att = (args[2], args[4]) if name.startswith("gatv2_score") and "backward" not in name else (args[3], args[5])
            calls.append((name, node.dtype, att.dtype, (r[0] if isinstance(r, tuple) else r).dtype))
            return r

        monkeypatch.setattr(sddmm, name, f)

    for name in ("gatv2_score", "gatv2_score_x16", "gatv2_score_backward", "gatv2_score_backward_x16"):
        spy(name)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(x, *G["args"])
    bf, f32 = torch.bfloat16, torch.float32
    assert calls == [("gatv2_score_x16", bf, f32, f32)], calls
    out.float().square().sum().backward()
    assert calls[1:] == [("gatv2_score_backward_x16", bf, f32, bf)] * 2, calls
    for name, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == f32 and bool(torch.isfinite(p.grad).all()), name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_layer_still_raises(pkg, square, dtype):
    import gespmm_amd

    G = square
    x = (torch.rand(G["n"], 12, device="cuda") - 0.5).to(dtype)
    fused = gespmm_amd.GATv2Conv(12, F, heads=H, fused=True).cuda().to(dtype)
    with pytest.raises(TypeError, match="gatv2_attention"):
        fused(x, *G["args"])
    fused.float()(x.float(), *G["args"])  # fp32 still runs


# ------------------------------------------------------------------------------------------------------- numbers, once

@pytest.mark.parametrize("dtype,u", ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)), ids=IDS)
def test_layer_against_float64(pkg, square, dtype, u):
    """|got - ref| <= u |ref| + 1e-4 max(|ref|, scale) for the layer's output and for grad_x, against a float64 torch composition on the
    widened parameters; scale is the sum of the magnitudes of the terms of the sum that is rounded (alpha xr for the output,
    grad_score m for grad_x). The bound has room for ONE 16-bit rounding of an fp32 sum, which is what the kernels of this layer do;
    the layer is therefore set up so that torch's dense steps add none of their own. in_channels = 2 H F with W_dst = [I; 0] and
    W_src = [0; B]: xl = x[:, :HF] exactly (a sum of one term and zeros), xr = x[:, HF:] B as torch rounds it — the composition takes
    that product from torch, widened, since its rounding belongs to torch's matmul — and the gradient of the first H F columns of x
    is grad_xl alone: grad_xl I^T is exact and the other term, grad_xr [0; B]^T, is exactly zero there. bias is zero (its add is
    exact) and grad_out is representable in the dtype, within +-32 so that no gradient of a long row falls below fp16's normal range."""
    import gespmm_amd

    G, n = square, square["n"]
    slope = 0.2
    torch.manual_seed(33)
    layer = gespmm_amd.GATv2Conv(2 * H * F, F, heads=H, negative_slope=slope).cuda()
    with torch.no_grad():
        B = layer.weight_src[H * F:].clone()
        layer.weight_dst.zero_()
        layer.weight_dst[:H * F] = torch.eye(H * F, device="cuda")
        layer.weight_src.zero_()
        layer.weight_src[H * F:] = B
    layer = layer.to(dtype)
    x = (2 * (torch.rand(n, 2 * H * F, device="cuda") - 0.5)).to(dtype).requires_grad_(True)
    go = (64 * (torch.rand(n, H * F, device="cuda") - 0.5)).to(dtype)
    out = layer(x, *G["args"])
    out.backward(go)
    with torch.no_grad():
        xr16 = (x @ layer.weight_src).view(n, H, F)
        assert torch.equal((x @ layer.weight_dst), x[:, :H * F]), "xl is not x[:, :HF] exactly"
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.diff(G["rp"]).long())
    cols = G["ci"].long()
    xl = x.detach()[:, :H * F].double().view(n, H, F).requires_grad_(True)
    xr = xr16.double().requires_grad_(True)
    att = layer.att.detach().double().view(H, F)
    t = xl[rows] + xr[cols]  # (t == 0 takes the branch t >= 0 here as in the kernels)
    score = (att * torch.where(t >= 0, t, t * float(np.float32(slope)))).sum(-1)
    score.retain_grad()
    top = torch.full((n, H), -float("inf"), dtype=torch.float64, device="cuda").scatter_reduce(0, rows[:, None].expand(-1, H),
                                                                                              score.detach(), "amax")
    e = torch.exp(score - top[rows])
    alpha = e / torch.zeros((n, H), dtype=torch.float64, device="cuda").index_add_(0, rows, e)[rows]
    terms = alpha.unsqueeze(-1) * xr[cols]
    ref = torch.zeros((n, H, F), dtype=torch.float64, device="cuda").index_add_(0, rows, terms)
    ref.backward(go.double().view(n, H, F))
    scale_out = torch.zeros_like(ref).index_add_(0, rows, terms.detach().abs())
    m = torch.where(t.detach() >= 0, att.expand_as(t), (att.float() * float(np.float32(slope))).double().expand_as(t))
    scale_gx = torch.zeros_like(ref).index_add_(0, rows, (score.grad.unsqueeze(-1) * m).abs())
    for what, got, want, scale in (("output", out.detach().view(n, H, F), ref.detach(), scale_out),
                                   ("grad_x", x.grad[:, :H * F].view(n, H, F), xl.grad, scale_gx)):
        # fp16 below its normal range rounds to a multiple of 2^-24, not to u |ref|: the sums are kept large enough for the second term
        # (an empty row has no terms: scale 0, and both sides exactly +0)
        assert float(scale[scale > 0].min()) * 1e-4 > 2.0 ** -25, (what, float(scale[scale > 0].min()))
        err = (got.double() - want).abs()
        bound = u * want.abs() + 1e-4 * torch.maximum(want.abs(), scale)
        worst = float((err / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
        print("GATv2Conv %s %s: worst error / bound = %.3g" % (dtype, what, worst))
        assert bool((want != 0).any()) and bool((err <= bound).all()), (what, worst)


# -------------------------------------------------------------------------------------------------------------------- training

def test_layer_step_replayed_from_a_captured_graph(pkg, square):
    """Forward and backward of a bf16 GATv2Conv (H = 4, F = 8: every step of the layer has a kernel) captured once: a replay gives the
    eager output and the eager gradients, bit for bit — nothing in the 16-bit score or its two gradient passes allocates or waits."""
    import gespmm_amd

    G, dtype = square, torch.bfloat16
    torch.manual_seed(41)
    layer = gespmm_amd.GATv2Conv(12, F, heads=H).cuda().to(dtype)
    x = (torch.rand(G["n"], 12, device="cuda") - 0.5).to(dtype).requires_grad_(True)
    go = (torch.rand(G["n"], H * F, device="cuda") - 0.5).to(dtype)
    args = (G["rp"], G["ci"], G["colptr"], G["rowind"], G["order32"])
    params = [x] + list(layer.parameters())

    def step():
        for p in params:
            p.grad = None
        out = layer(x, *args)
        grads = torch.autograd.grad(out, params, go)
        return (out.detach(),) + grads

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for t in static:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, static):
        _bits_equal(b, a, "replay")


def _example_on_cora():
    spec = importlib.util.spec_from_file_location("gat_example_v2_x16", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    device = torch.device("cuda")
    edge_index, n_v, n_feat, n_cls = ex.load_edges("cora", device)
    g = ex.gat_graph(edge_index, n_v, device, int32_order=True)
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n_v, n_feat, generator=gen)
    x = (x / x.sum(1, keepdim=True)).to(device).to(torch.bfloat16)
    y = torch.randint(0, n_cls, (n_v,), generator=gen).to(device)
    train_idx = torch.randperm(n_v, generator=gen)[:20 * n_cls].to(device)
    return ex, g, x, y[train_idx], train_idx, n_feat, n_cls


def _example_step(ex, g, x, y_train, train_idx, n_feat, n_cls):
    """The example's model as ``--v2 --dtype bf16`` builds it, dropout off, with a capturable Adam -> the training step."""
    import gespmm_amd

    torch.manual_seed(0)
    model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, v2=True).to(x.device).to(torch.bfloat16)
    assert isinstance(model.conv1, gespmm_amd.GATv2Conv) and model.conv1.att.dtype == torch.bfloat16 and not model.conv1.fused
    opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4, capturable=True)
    model.train()

    def train_step():
        opt.zero_grad(set_to_none=False)
        out = model(x, g)
        assert out.dtype == torch.bfloat16
        loss = torch.nn.functional.nll_loss(out.index_select(0, train_idx).float(), y_train)  # the mean of 140 terms in fp32
        loss.backward()
        opt.step()
        return loss

    return train_step


def test_training_steps_on_cora_v2_bf16_eager(pkg):
    """The example's model as ``--v2 --dtype bf16`` builds it on cora: the losses of the training steps are finite and the second is
    below the first."""
    train_step = _example_step(*_example_on_cora())
    losses = [float(train_step().detach()) for _ in range(5)]
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[1] < losses[0], losses


def test_training_steps_on_cora_v2_bf16_captured(pkg):
    """The same steps replayed from a captured graph (the example's --graph-capture: three warm-up steps on a side stream) give the
    eager losses. The model's SECOND layer is ``GATv2Conv(heads=1)`` on 7 classes, where the 16-bit multi-head product has no kernel
    (it needs 2 <= H <= 8 and an even F) and the op's own composition allocates, which a capturing stream refuses: there
    ``MultiHeadSPMMFunction`` composes widen / fp32 product / narrow on torch's allocations — the same bits, hence the same losses."""
    data = _example_on_cora()
    eager_step = _example_step(*data)
    eager = [float(eager_step().detach()) for _ in range(5)]
    train_step = _example_step(*data)
    losses = []
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
    print("losses", {"eager": eager, "captured": losses})
    assert all(np.isfinite(losses)) and losses[1] < losses[0], losses
    assert losses == eager, (losses, eager)
