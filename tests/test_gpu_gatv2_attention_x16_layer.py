"""The fused GATv2 attention on 16-bit features above the kernels: GATv2AttentionFunction on fp16 / bf16 node terms is WIRING — forward
and every gradient are bit-equal to the direct ``attention.gatv2_attention_x16`` / ``_backward_row_x16`` / ``_backward_col_x16`` calls
(pinned in tests/test_gpu_gatv2_attention_x16.py) — GATv2Conv(fused=True, fused_x16=True) as a ``.half()`` / ``.bfloat16()`` layer is
bit-equal to its documented steps, in eval and in training with dropout, and runs the 16-bit ops under autocast; one check against
float64 per dtype, next to the ``fused=False`` 16-bit layer on the same inputs; the memory of a step; the example's model in bf16."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import ROOT
from test_gpu_gat_backward_layer import _regular_graph

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
IDS = ("fp16", "bf16")
H, F = 4, 8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    bad = int((got.contiguous().view(view) != want.contiguous().view(view)).sum())
    assert bad == 0, "%s: %d of %d elements differ" % (what, bad, got.numel())


def _rand(gen, *shape):
    return torch.rand(*shape, device="cuda", generator=gen) - 0.5


@pytest.fixture(scope="module")
def square():
    """A square graph of 300 nodes: every row has its self-loop (no empty row) and 0, 1, 2, 4, 8, 37 or 70 more entries — rows longer
    than a lane group and no multiple of four among them — columns unsorted, repeats allowed; both index orders."""
    from gespmm_amd import graphs

    n = 300
    rng = np.random.RandomState(5)
    degs = rng.choice((0, 1, 2, 4, 8, 37, 70), size=n, p=(0.1, 0.2, 0.2, 0.2, 0.15, 0.1, 0.05))
    cols = [np.concatenate(([r], rng.randint(0, n, size=d))) for r, d in enumerate(degs)]
    for c in cols:
        rng.shuffle(c)
    rowptr = np.concatenate(([0], np.cumsum([c.size for c in cols]))).astype(np.int32)
    colind = np.concatenate(cols).astype(np.int32)
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    return {"n": n, "nnz": int(colind.size), "rp": rp, "ci": ci, "colptr": colptr, "rowind": rowind, "order32": order.to(torch.int32),
            "args": (rp, ci, colptr, rowind, order.to(torch.int32)), "fargs": (rp, ci, colptr, rowind)}


SEED = (0x12345678, -0x65432110)


def _seed():
    return torch.tensor(SEED, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------------ the function

def _count_launches(monkeypatch):
    from gespmm_amd import attention

    calls = []
    for name in ("gatv2_attention", "gatv2_attention_backward_row", "gatv2_attention_backward_col", "gatv2_attention_x16",
                 "gatv2_attention_backward_row_x16", "gatv2_attention_backward_col_x16"):
        real = getattr(attention, name)

        def f(*args, _real=real, _name=name, **kw):
            calls.append((_name, args[2].dtype, args[4].dtype))
            return _real(*args, **kw)

        monkeypatch.setattr(attention, name, f)
    return calls


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("slope,p", ((None, 0.0), (0.2, 0.0), (0.2, 0.5)))
def test_function_is_the_direct_op_calls(pkg, square, monkeypatch, dtype, slope, p):
    import gespmm_amd
    from gespmm_amd import attention

    G = square
    direct = {n: getattr(attention, n) for n in ("gatv2_attention_x16", "gatv2_attention_backward_row_x16", "gatv2_attention_backward_col_x16")}
    calls = _count_launches(monkeypatch)
    gen = torch.Generator(device="cuda").manual_seed(21)
    xl = _rand(gen, G["n"], H, F).to(dtype).requires_grad_(True)
    xr = _rand(gen, G["n"], H, F).to(dtype).requires_grad_(True)
    att = (4 * _rand(gen, H, F)).requires_grad_(True)
    go = _rand(gen, G["n"], H, F).to(dtype)
    seed = _seed() if p else None
    drop = (p, seed) if p else None
    out = gespmm_amd.GATv2AttentionFunction.apply(*G["fargs"], xl, xr, att, slope, p, seed)
    assert out.dtype == dtype and out.shape == (G["n"], H, F)
    assert calls == [("gatv2_attention_x16", dtype, torch.float32)]
    a, b, w = xl.detach(), xr.detach(), att.detach()
    want_out, stats = direct["gatv2_attention_x16"](G["rp"], G["ci"], a, b, w, negative_slope=slope, dropout=drop)
    assert stats.dtype == torch.float32
    _bits_equal(out.detach(), want_out, "forward")
    del calls[:]
    out.backward(go)
    assert [c[0] for c in calls] == ["gatv2_attention_backward_row_x16", "gatv2_attention_backward_col_x16"], calls  # two launches
    assert xl.grad.dtype == dtype and xr.grad.dtype == dtype and att.grad.dtype == torch.float32
    delta, gxl, part = direct["gatv2_attention_backward_row_x16"](G["rp"], G["ci"], a, b, w, stats, want_out, go, negative_slope=slope,
                                                                  dropout=drop)
    gxr = direct["gatv2_attention_backward_col_x16"](G["colptr"], G["rowind"], a, b, w, stats, delta, go, negative_slope=slope, dropout=drop)
    assert delta.dtype == torch.float32 and part.dtype == torch.float32 and gxl.dtype == dtype and gxr.dtype == dtype
    _bits_equal(xl.grad, gxl, "grad_xl")
    _bits_equal(xr.grad, gxr, "grad_xr")
    _bits_equal(att.grad, part.sum(0), "grad_att")
    # xl is xr (shared weights): autograd adds the two gradients, in the operands' dtype
    x = b.clone().requires_grad_(True)
    gespmm_amd.GATv2AttentionFunction.apply(*G["fargs"], x, x, w, slope, p, seed).backward(go)
    o1, s1 = direct["gatv2_attention_x16"](G["rp"], G["ci"], b, b, w, negative_slope=slope, dropout=drop)
    d1, one = direct["gatv2_attention_backward_row_x16"](G["rp"], G["ci"], b, b, w, s1, o1, go, negative_slope=slope, dropout=drop,
                                                         want_att_part=False)
    two = direct["gatv2_attention_backward_col_x16"](G["colptr"], G["rowind"], b, b, w, s1, d1, go, negative_slope=slope, dropout=drop)
    assert x.grad.dtype == dtype
    _bits_equal(x.grad, one + two, "xl is xr")
    # only att requires grad: the row pass alone
    w2 = w.clone().requires_grad_(True)
    del calls[:]
    gespmm_amd.GATv2AttentionFunction.apply(*G["fargs"], a, b, w2, slope, p, seed).backward(go)
    assert [c[0] for c in calls] == ["gatv2_attention_x16", "gatv2_attention_backward_row_x16"], calls
    _bits_equal(w2.grad, part.sum(0), "grad_att alone")
    # att must be fp32; the node terms one 16-bit type
    with pytest.raises(TypeError):
        gespmm_amd.GATv2AttentionFunction.apply(*G["fargs"], a, b, w.to(dtype), slope)
    with pytest.raises(TypeError):
        gespmm_amd.GATv2AttentionFunction.apply(*G["fargs"], a, b.float(), w, slope)
    with pytest.raises(TypeError):
        gespmm_amd.GATv2AttentionFunction.apply(*G["fargs"], a.half(), b.bfloat16(), w, slope)


# --------------------------------------------------------------------------------------------------------------------- the layer

def _terms(layer, x):
    n = x.shape[0]
    xr = (x @ layer.weight_src).view(n, H, F)
    xl = xr if layer.share_weights else (x @ layer.weight_dst).view(n, H, F)
    return xl, xr


def _forward_by_hand(layer, x, G, p=0.0, seed=None):
    """The documented steps of a 16-bit GATv2Conv(fused=True, fused_x16=True) on the ops themselves."""
    from gespmm_amd import attention

    xl, xr = _terms(layer, x)
    assert xl.dtype == x.dtype and xr.dtype == x.dtype
    out, _ = attention.gatv2_attention_x16(G["rp"], G["ci"], xl.contiguous(), xr.contiguous(), layer.att.view(H, F).float(),
                                           negative_slope=layer.negative_slope, dropout=(p, seed) if seed is not None else None)
    return out.reshape(x.shape[0], H * F) + layer.bias


def _step_by_hand(layer, x, G, p=0.0, seed=None):
    """The same steps as the autograd function, on the layer's own parameters -> the output (gradients arrive by backward)."""
    import gespmm_amd

    xl, xr = _terms(layer, x)
    out = gespmm_amd.GATv2AttentionFunction.apply(*G["fargs"], xl, xr, layer.att.view(H, F).float(), layer.negative_slope, p, seed)
    return out.reshape(x.shape[0], H * F) + layer.bias


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("share", (False, True))
def test_fused_x16_layer_is_its_documented_steps(pkg, square, dtype, share):
    """eval, and training with dropout=0.5 under a fixed attn_seed: the output is bit-equal to the steps on the ops themselves, and the
    gradients of x, both weights, att and bias are bit-equal to those of the same steps written with the autograd function."""
    import gespmm_amd

    G = square
    torch.manual_seed(31)
    layer = gespmm_amd.GATv2Conv(12, F, heads=H, dropout=0.5, share_weights=share, fused=True, fused_x16=True).cuda().to(dtype)
    with torch.no_grad():
        layer.bias.copy_(torch.rand_like(layer.bias) - 0.5)
    twin = copy.deepcopy(layer)
    x0 = (torch.rand(G["n"], 12, device="cuda") - 0.5).to(dtype)
    go = (torch.rand(G["n"], H * F, device="cuda") - 0.5).to(dtype)
    seed = _seed()
    names = [n for n, _ in layer.named_parameters()]
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
    # fp32 features with both keywords set: exactly what fused=True runs
    f32, plain = copy.deepcopy(layer).float().eval(), gespmm_amd.GATv2Conv(12, F, heads=H, share_weights=share, fused=True).cuda().eval()
    plain.load_state_dict(f32.state_dict())
    _bits_equal(f32(x0.float(), *G["args"]).detach(), plain(x0.float(), *G["args"]).detach(), "fp32 features")


def test_fused_x16_layer_under_autocast(pkg, square, monkeypatch):
    """fp32 parameters under torch.autocast(bfloat16): x @ W comes out bf16, so the three launches are the _x16 ones, with an fp32 att."""
    import gespmm_amd

    G = square
    torch.manual_seed(32)
    layer = gespmm_amd.GATv2Conv(12, F, heads=H, fused=True, fused_x16=True).cuda()
    x = torch.rand(G["n"], 12, device="cuda") - 0.5
    calls = _count_launches(monkeypatch)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(x, *G["args"])
    bf, f32 = torch.bfloat16, torch.float32
    assert calls == [("gatv2_attention_x16", bf, f32)], calls  # (out is fp32: the bias add promotes the op's bf16 result)
    out.float().square().sum().backward()
    assert calls[1:] == [("gatv2_attention_backward_row_x16", bf, f32), ("gatv2_attention_backward_col_x16", bf, f32)], calls
    for name, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == f32 and bool(torch.isfinite(p.grad).all()), name
    # without the keyword the refusal stands
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(TypeError, match="gatv2_attention"):
        gespmm_amd.GATv2Conv(12, F, heads=H, fused=True).cuda()(x, *G["args"])


# ------------------------------------------------------------------------------------------------------- numbers, once

@pytest.mark.parametrize("dtype,u", ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)), ids=IDS)
def test_layer_against_float64(pkg, square, dtype, u):
    """The layer's output and the gradients of x, both weights, att and bias against a float64 torch composition on the widened
    parameters. A tensor passes if it meets EITHER bound:
      1. |got - ref| <= u |ref| + 1e-4 max(|ref|, scale) elementwise — the rule of tests/test_gpu_gatv2_x16_layer.py, with its set-up
         (in_channels = 2 H F, W_dst = [I; 0], W_src = [0; B], zero bias, xr taken from torch's matmul and widened, grad_out within
         +-32) and its scales: the summed magnitudes of alpha xr for the output and of grad_score m for grad_x[:, :HF]; 0 for the
         tensors that rule was never written for (their sums go through torch's 16-bit matmuls).
      2. max |got - ref| / max |ref| <= 2 x the same figure of the ``fused=False`` 16-bit layer on the same inputs and seed, measured
         here. Two, because the fused path feeds one more once-rounded node array (out, through delta) into every gradient, while the
         unfused path keeps its edge arrays fp32.
    Both figures are printed per tensor."""
    import gespmm_amd

    G, n = square, square["n"]
    slope = 0.2
    torch.manual_seed(33)
    base = gespmm_amd.GATv2Conv(2 * H * F, F, heads=H, negative_slope=slope).cuda()
    with torch.no_grad():
        B = base.weight_src[H * F:].clone()
        base.weight_dst.zero_()
        base.weight_dst[:H * F] = torch.eye(H * F, device="cuda")
        base.weight_src.zero_()
        base.weight_src[H * F:] = B
    base = base.to(dtype)
    fused = gespmm_amd.GATv2Conv(2 * H * F, F, heads=H, negative_slope=slope, fused=True, fused_x16=True).cuda().to(dtype)
    fused.load_state_dict(base.state_dict())
    x0 = (2 * (torch.rand(n, 2 * H * F, device="cuda") - 0.5)).to(dtype)
    go = (64 * (torch.rand(n, H * F, device="cuda") - 0.5)).to(dtype)
    names = ("weight_dst", "weight_src", "att", "bias")
    got = {}
    for key, layer in (("fused", fused), ("unfused", base)):
        x = x0.clone().requires_grad_(True)
        out = layer(x, *G["args"])
        out.backward(go)
        got[key] = dict({"output": out.detach(), "grad_x": x.grad}, **{"grad_" + nm: getattr(layer, nm).grad for nm in names})
    with torch.no_grad():
        xr16 = (x0 @ base.weight_src).view(n, H, F)
        assert torch.equal((x0 @ base.weight_dst), x0[:, :H * F]), "xl is not x[:, :HF] exactly"
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.diff(G["rp"]).long())
    cols = G["ci"].long()
    x64 = x0.double().requires_grad_(True)
    P = {nm: getattr(base, nm).detach().double().requires_grad_(True) for nm in names}
    xl = (x64 @ P["weight_dst"]).view(n, H, F)  # (exact: one term and zeros)
    xr = (x64 @ P["weight_src"]).view(n, H, F)
    xr = xr + (xr16.double() - xr).detach()     # the VALUE of torch's 16-bit matmul, widened — its rounding belongs to torch
    xl.retain_grad()
    att = P["att"].view(H, F)
    t = xl[rows] + xr[cols]  # (t == 0 takes the branch t >= 0 here as in the kernels)
    score = (att * torch.where(t >= 0, t, t * float(np.float32(slope)))).sum(-1)
    score.retain_grad()
    top = torch.full((n, H), -float("inf"), dtype=torch.float64, device="cuda").scatter_reduce(0, rows[:, None].expand(-1, H),
                                                                                              score.detach(), "amax")
    e = torch.exp(score - top[rows])
    alpha = e / torch.zeros((n, H), dtype=torch.float64, device="cuda").index_add_(0, rows, e)[rows]
    terms = alpha.unsqueeze(-1) * xr[cols]
    agg = torch.zeros((n, H, F), dtype=torch.float64, device="cuda").index_add_(0, rows, terms)
    ref_out = agg.reshape(n, H * F) + P["bias"]
    ref_out.backward(go.double())
    ref = dict({"output": ref_out.detach(), "grad_x": x64.grad}, **{"grad_" + nm: P[nm].grad for nm in names})
    scale_out = torch.zeros_like(agg).index_add_(0, rows, terms.detach().abs()).reshape(n, H * F)
    m = torch.where(t.detach() >= 0, att.detach().expand_as(t), (att.detach().float() * float(np.float32(slope))).double().expand_as(t))
    scale_gx = torch.zeros_like(agg).index_add_(0, rows, (score.grad.unsqueeze(-1) * m).abs()).reshape(n, H * F)
    scales = {"output": scale_out, "grad_x": torch.cat((scale_gx, torch.zeros_like(scale_gx)), 1)}
    failed = []
    for name, want in ref.items():
        f, w = got["fused"][name].double().view_as(want), got["unfused"][name].double().view_as(want)
        top_ref = float(want.abs().max())
        assert top_ref > 0, name
        err_f, err_u = float((f - want).abs().max()) / top_ref, float((w - want).abs().max()) / top_ref
        scale = scales.get(name, torch.zeros_like(want))
        bound = u * want.abs() + 1e-4 * torch.maximum(want.abs(), scale)
        worst = float(((f - want).abs() / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
        rule1, rule2 = bool(((f - want).abs() <= bound).all()), err_f <= 2 * err_u
        print("GATv2Conv fused_x16 %s %s: max error / max |ref| fused %.3g, fused=False %.3g (ratio %.3g); worst error / rule-1 bound %.3g"
              % (dtype, name, err_f, err_u, err_f / err_u if err_u else float("inf"), worst))
        if not (rule1 or rule2):
            failed.append((name, err_f, err_u, worst))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------------ memory

def test_bf16_fused_step_peaks_below_fp32_fused_and_bf16_unfused(pkg):
    """n = 2048, 64 entries per row, H = F = 8: one [nnz, H] fp32 array is 4 MiB, a node-sized [n, H, F] array 512 KiB in fp32 and
    256 KiB in bf16. Forward plus backward of the bf16 fused function allocate out, grad_xl and grad_xr (256 KiB each), att_part (512
    KiB), stats (128 KiB), delta (64 KiB): about 1.5 MiB where the fp32 one allocates about 2.2 MiB."""
    import gespmm_amd
    from gespmm_amd import graphs

    n, deg, H_, F_ = 2048, 64, 8, 8
    rowptr, colind = _regular_graph(n, deg, 9)
    nnz = n * deg
    big = nnz * H_ * 4
    assert big == 4 << 20
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    order = order.to(torch.int32)
    gen = torch.Generator(device="cuda").manual_seed(1)
    xl0, xr0, att0, go0 = _rand(gen, n, H_, F_), _rand(gen, n, H_, F_), _rand(gen, H_, F_), _rand(gen, n, H_, F_)
    peaks = {}
    for key, dt, fused in (("bf16 fused", torch.bfloat16, True), ("fp32 fused", torch.float32, True), ("bf16 unfused", torch.bfloat16, False)):
        xl, xr = (t.to(dt).clone().requires_grad_(True) for t in (xl0, xr0))  # (leaves: .to(float32) alone would hand back xl0 itself)
        att, gout = att0.clone().requires_grad_(True), go0.to(dt)
        shapes = []

        def pack(t, shapes=shapes):
            shapes.append(tuple(t.shape))
            return t

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            if fused:
                out = gespmm_amd.GATv2AttentionFunction.apply(rp, ci, colptr, rowind, xl, xr, att, 0.2, 0.0, None)
            else:
                score = gespmm_amd.GATv2ScoreFunction.apply(rp, ci, colptr, rowind, order, xl, xr, att, 0.2)
                alpha = gespmm_amd.EdgeSoftmaxFunction.apply(rp, score, None)
                out = gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, xr, alpha, None, True)
        assert out.dtype == dt
        out.backward(gout)
        torch.cuda.synchronize()
        peaks[key] = torch.cuda.max_memory_allocated() - before
        assert xl.grad.dtype == dt and xr.grad.dtype == dt and att.grad.dtype == torch.float32
        if fused:
            assert shapes and not any(int(np.prod(s)) >= nnz * H_ for s in shapes), shapes
        del out, xl, xr, att
    print("peak of forward + backward above the allocation before it, bytes: %s; one [nnz, H] fp32 array %d" % (peaks, big))
    assert peaks["bf16 fused"] < peaks["fp32 fused"], peaks
    assert peaks["bf16 fused"] < peaks["bf16 unfused"], peaks
    assert peaks["bf16 fused"] < big, peaks


# -------------------------------------------------------------------------------------------------------------------- training

def test_layer_step_replayed_from_a_captured_graph(pkg, square):
    """Forward and backward of a bf16 GATv2Conv(fused=True, fused_x16=True) with dropout captured once: a replay gives the eager output
    and the eager gradients, bit for bit — nothing in the three launches allocates behind torch's back or waits."""
    import gespmm_amd

    G, dtype = square, torch.bfloat16
    torch.manual_seed(41)
    layer = gespmm_amd.GATv2Conv(12, F, heads=H, dropout=0.3, fused=True, fused_x16=True).cuda().to(dtype).train()
    x = (torch.rand(G["n"], 12, device="cuda") - 0.5).to(dtype).requires_grad_(True)
    go = (torch.rand(G["n"], H * F, device="cuda") - 0.5).to(dtype)
    seed = _seed()
    params = [x] + list(layer.parameters())

    def step():
        out = layer(x, *G["args"], attn_seed=seed)
        return (out.detach(),) + torch.autograd.grad(out, params, go)

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
    spec = importlib.util.spec_from_file_location("gat_example_v2_fused_x16", os.path.join(ROOT, "examples", "gat_custom.py"))
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
    """The example's model as ``--v2 --fused-attention --dtype bf16`` builds it, dropout off, with a capturable Adam -> the step."""
    import gespmm_amd

    torch.manual_seed(0)
    model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, v2=True, fused_attention=True).to(x.device).to(torch.bfloat16)
    for conv in (model.conv1, model.conv2):
        assert isinstance(conv, gespmm_amd.GATv2Conv) and conv.att.dtype == torch.bfloat16 and conv.fused and conv.fused_x16
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


def test_training_steps_on_cora_bf16_eager_and_captured(pkg):
    """The example's model with --v2 --fused-attention in bf16 on cora: the losses are finite and go down, eager and replayed from a
    captured graph (the example's --graph-capture: three warm-up steps on a side stream)."""
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
    for run in (eager, losses):
        assert all(np.isfinite(run)) and run[1] < run[0] and run[-1] < run[0], run
