"""The fused dot-product attention on 16-bit features above the kernels: DotAttentionFunction on fp16 / bf16 q, k and v is WIRING —
forward and every gradient are bit-equal to the direct ``attention.dot_attention_x16`` / ``_backward_q_x16`` / ``_backward_kv_x16``
calls (pinned in tests/test_gpu_dot_attention_x16.py) — TransformerConv(fused=True, fused_x16=True) runs as a ``.half()`` /
``.bfloat16()`` layer and under autocast in every setting of concat / beta / root_weight; dropout drops the entries the ``fused=False``
16-bit layer drops under one seed; one check against float64 per dtype, next to the ``fused=False`` 16-bit layer on the same inputs and
seed; the memory of a training step; the example's model in bf16, eager and captured."""
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
SEED = (0x12345678, -0x65432110)
SETTINGS = ((True, False, True), (True, True, True), (True, False, False), (False, False, True), (False, True, True), (False, False, False))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    bad = int((got.contiguous().view(view) != want.contiguous().view(view)).sum())
    assert bad == 0, "%s: %d of %d elements differ" % (what, bad, got.numel())


def _rand(gen, *shape):
    return torch.rand(*shape, device="cuda", generator=gen) - 0.5


def _seed():
    return torch.tensor(SEED, dtype=torch.int32, device="cuda")


def _square_of(rowptr, colind, n):
    from gespmm_amd import graphs

    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rowptr))
    return {"n": n, "nnz": int(colind.size), "rp": rp, "ci": ci, "colptr": colptr, "rowind": rowind, "rows_h": rows, "cols_h": colind,
            "args": (rp, ci, colptr, rowind, order.to(torch.int32)), "fargs": (rp, ci, colptr, rowind)}


@pytest.fixture(scope="module")
def square():
    """A square graph of 300 nodes: every row has its self-loop (no empty row) and 0, 1, 2, 4, 8, 37 or 70 more entries — rows longer
    than a lane group and no multiple of four among them — columns unsorted, repeats allowed; both index orders."""
    n = 300
    rng = np.random.RandomState(5)
    degs = rng.choice((0, 1, 2, 4, 8, 37, 70), size=n, p=(0.1, 0.2, 0.2, 0.2, 0.15, 0.1, 0.05))
    cols = [np.concatenate(([r], rng.randint(0, n, size=d))) for r, d in enumerate(degs)]
    for c in cols:
        rng.shuffle(c)
    rowptr = np.concatenate(([0], np.cumsum([c.size for c in cols]))).astype(np.int32)
    return _square_of(rowptr, np.concatenate(cols).astype(np.int32), n)


# ------------------------------------------------------------------------------------------------------------------ the function

def _count_launches(monkeypatch):
    from gespmm_amd import attention

    calls = []
    for name in ("dot_attention", "dot_attention_backward_q", "dot_attention_backward_kv", "dot_attention_x16",
                 "dot_attention_backward_q_x16", "dot_attention_backward_kv_x16"):
        real = getattr(attention, name)

        def f(*args, _real=real, _name=name, **kw):
            calls.append((_name, args[2].dtype))
            return _real(*args, **kw)

        monkeypatch.setattr(attention, name, f)
    return calls


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("p", (0.0, 0.5))
def test_function_is_the_direct_op_calls(pkg, square, monkeypatch, dtype, p):
    import gespmm_amd
    from gespmm_amd import attention

    G = square
    direct = {n: getattr(attention, n) for n in ("dot_attention_x16", "dot_attention_backward_q_x16", "dot_attention_backward_kv_x16")}
    calls = _count_launches(monkeypatch)
    gen = torch.Generator(device="cuda").manual_seed(21)
    q, k, v = ((4 * _rand(gen, G["n"], H, F)).to(dtype).requires_grad_(True) for _ in range(3))
    go = _rand(gen, G["n"], H, F).to(dtype)
    seed = _seed() if p else None
    drop = (p, seed) if p else None
    out = gespmm_amd.DotAttentionFunction.apply(q, k, v, *G["fargs"], None, p, seed)
    assert out.dtype == dtype and out.shape == (G["n"], H, F)
    assert calls == [("dot_attention_x16", dtype)]
    a, b, c = q.detach(), k.detach(), v.detach()
    want_out, stats = direct["dot_attention_x16"](G["rp"], G["ci"], a, b, c, dropout=drop)
    assert stats.dtype == torch.float32
    _bits_equal(out.detach(), want_out, "forward")
    del calls[:]
    out.backward(go)
    assert [c_[0] for c_ in calls] == ["dot_attention_backward_q_x16", "dot_attention_backward_kv_x16"], calls  # two launches
    delta, gq = direct["dot_attention_backward_q_x16"](G["rp"], G["ci"], a, b, c, stats, want_out, go, dropout=drop)
    gk, gv = direct["dot_attention_backward_kv_x16"](G["colptr"], G["rowind"], a, b, c, stats, delta, go, dropout=drop)
    assert delta.dtype == torch.float32
    for name, t, want in (("grad_q", q.grad, gq), ("grad_k", k.grad, gk), ("grad_v", v.grad, gv)):
        assert t.dtype == dtype and bool((t != 0).any()), name
        _bits_equal(t, want, name)
    # only q requires grad: the row pass alone
    q2 = a.clone().requires_grad_(True)
    del calls[:]
    gespmm_amd.DotAttentionFunction.apply(q2, b, c, *G["fargs"], None, p, seed).backward(go)
    assert [c_[0] for c_ in calls] == ["dot_attention_x16", "dot_attention_backward_q_x16"], calls
    _bits_equal(q2.grad, gq, "grad_q alone")
    # q, k and v of one 16-bit type
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    for mixed in ((a.float(), b, c), (a, b.float(), c), (a, b, c.to(other))):
        with pytest.raises(TypeError):
            gespmm_amd.DotAttentionFunction.apply(*mixed, *G["fargs"])


# --------------------------------------------------------------------------------------------------------------------- the layer

@pytest.mark.parametrize("concat,beta,root", SETTINGS)
@pytest.mark.parametrize("mode", ("fp16", "bf16", "autocast"))
def test_layer_runs_as_a_16_bit_module_and_under_autocast(pkg, square, monkeypatch, mode, concat, beta, root):
    """TransformerConv(12, 8, heads=4, fused=True, fused_x16=True) as .half(), as .bfloat16() and with fp32 parameters under
    torch.autocast(bfloat16): the three launches are the _x16 ones, the output has the features' dtype and the layer's shape, every
    parameter gradient is finite and in the parameter's dtype."""
    import gespmm_amd

    G = square
    torch.manual_seed(31)
    layer = gespmm_amd.TransformerConv(12, F, heads=H, concat=concat, beta=beta, root_weight=root, fused=True, fused_x16=True).cuda()
    x = torch.rand(G["n"], 12, device="cuda") - 0.5
    calls = _count_launches(monkeypatch)
    if mode == "autocast":
        dtype, pdtype = torch.bfloat16, torch.float32
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = layer(x, *G["args"])
    else:
        dtype = pdtype = torch.float16 if mode == "fp16" else torch.bfloat16
        layer = layer.to(dtype)
        out = layer(x.to(dtype), *G["args"])
    assert calls == [("dot_attention_x16", dtype)], calls
    assert out.dtype == dtype and out.shape == (G["n"], H * F if concat else F)
    assert bool(torch.isfinite(out).all())
    out.float().square().sum().backward()
    assert calls[1:] == [("dot_attention_backward_q_x16", dtype), ("dot_attention_backward_kv_x16", dtype)], calls
    for name, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == pdtype and bool(torch.isfinite(p.grad).all()), name
    assert bool((layer.lin_value.weight.grad != 0).any()) and bool((layer.lin_query.weight.grad != 0).any())


def test_without_the_keyword_the_refusal_stands_and_fp32_is_unchanged(pkg, square):
    import gespmm_amd

    G = square
    torch.manual_seed(32)
    both = gespmm_amd.TransformerConv(12, F, heads=H, fused=True, fused_x16=True).cuda().eval()
    plain = gespmm_amd.TransformerConv(12, F, heads=H, fused=True).cuda().eval()
    plain.load_state_dict(both.state_dict())
    x = torch.rand(G["n"], 12, device="cuda") - 0.5
    _bits_equal(both(x, *G["args"]).detach(), plain(x, *G["args"]).detach(), "fp32 features")  # exactly what fused=True runs
    with torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(TypeError, match="dot_attention"):
        plain(x, *G["args"])
    with pytest.raises(TypeError, match="dot_attention"):
        plain.bfloat16()(x.bfloat16(), *G["args"])


# ---------------------------------------------------------------------------------------------------------------------- dropout

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dropout_drops_the_entries_the_unfused_layer_drops(pkg, dtype):
    """One entry per row (row r attends to ONE random column), no skip term, heads concatenated: out[r, h, :] is keep(r, c, h) *
    v[c, h, :] / (1 - p) — the softmax of one entry is 1 — so a (row, head) slice is all zeros exactly where the entry is dropped and
    has no zero where it is kept (v has no zero: asserted). Under one attn_seed the fused 16-bit layer and the ``fused=False`` 16-bit
    layer show the same zero pattern, which is the restated mask's."""
    import gespmm_amd
    from gespmm_amd import _lib, softmax

    n, p = 257, 0.4
    rng = np.random.RandomState(11)
    G = _square_of(np.arange(n + 1, dtype=np.int32), rng.randint(0, n, size=n).astype(np.int32), n)
    seed = _seed()
    torch.manual_seed(34)
    kw = dict(heads=H, dropout=p, root_weight=False, attn_seed=seed)
    fused = gespmm_amd.TransformerConv(12, F, fused=True, fused_x16=True, **kw).cuda().to(dtype).train()
    comp = gespmm_amd.TransformerConv(12, F, fused=False, **kw).cuda().to(dtype).train()
    comp.load_state_dict(fused.state_dict())
    x = (torch.rand(n, 12, device="cuda") + 0.5).to(dtype)
    with torch.no_grad():
        v = fused.lin_value(x).view(n, H, F)
        assert bool((v != 0).all())
        zeros = {key: (layer(x, *G["args"]).view(n, H, F) == 0) for key, layer in (("fused", fused), ("unfused", comp))}
    s = np.array(SEED, dtype=np.int32).view(np.uint32)
    bits = softmax.restate_edge_dropout_bits(s[0], s[1], G["rows_h"][:, None], G["cols_h"][:, None], np.arange(H)[None, :])
    dropped = _dev(bits < np.uint32(_lib.edge_dropout_threshold(p)))  # [n, H]: entry e is row e's only one
    assert 0 < int(dropped.sum()) < n * H
    for key, z in zeros.items():
        assert bool((z.all(-1) == dropped).all()), key + ": a dropped entry shows, or a kept one does not"
        assert bool((z.any(-1) == dropped).all()), key + ": a kept entry has a zero word"
    assert bool((zeros["fused"] == zeros["unfused"]).all())


# ------------------------------------------------------------------------------------------------------- numbers, once

def _attention_float64(q, k, v, rows, cols, n, scale, keep):
    s = (q[rows] * k[cols]).sum(-1) * scale
    top = torch.full((n, H), -float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, rows[:, None].expand(-1, H), s.detach(), "amax")
    t = torch.exp(s - top[rows])
    alpha = t / torch.zeros((n, H), dtype=s.dtype, device=s.device).index_add_(0, rows, t)[rows]
    terms = (alpha * keep).unsqueeze(-1) * v[cols]
    out = torch.zeros((n, H, F), dtype=s.dtype, device=s.device).index_add_(0, rows, terms)
    return out, torch.zeros_like(out).index_add_(0, rows, terms.detach().abs())


@pytest.mark.parametrize("dtype,u", ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)), ids=IDS)
def test_layer_against_float64(pkg, square, dtype, u):
    """The layer's output and the gradients of x and of the three weights against a float64 model on the widened parameters, training
    mode with dropout 0.25 under one seed (the mask restated). q, k and v of the model take the VALUE of torch's 16-bit linears,
    widened — their rounding belongs to torch — and pass gradients through the float64 linears. No skip term and no bias (the gradient
    of a key bias is zero in exact arithmetic), heads concatenated: the output is the attention's. A tensor passes if it meets EITHER
      1. |got - ref| <= u |ref| + 1e-4 max(|ref|, scale) elementwise, the project's rule for a once-rounded fp32 sum; scale is the
         summed magnitudes of alpha keep v for the output and 0 for the gradients (their sums go through torch's 16-bit matmuls); or
      2. max |got - ref| / max |ref| <= 2 x the same figure of the ``fused=False`` 16-bit layer on the same inputs and seed, measured
         here. Two, because the fused path feeds one more once-rounded node array (out, through delta) into every gradient, while the
         unfused path keeps its edge arrays fp32.
    Both figures are printed per tensor."""
    import gespmm_amd
    from gespmm_amd import _lib, softmax

    G, n, p = square, square["n"], 0.25
    seed = _seed()
    torch.manual_seed(33)
    kw = dict(heads=H, dropout=p, bias=False, root_weight=False, attn_seed=seed)
    fused = gespmm_amd.TransformerConv(12, F, fused=True, fused_x16=True, **kw).cuda().to(dtype).train()
    base = gespmm_amd.TransformerConv(12, F, fused=False, **kw).cuda().to(dtype).train()
    base.load_state_dict(fused.state_dict())
    x0 = (2 * (torch.rand(n, 12, device="cuda") - 0.5)).to(dtype)
    go = (64 * (torch.rand(n, H * F, device="cuda") - 0.5)).to(dtype)
    names = ("lin_query.weight", "lin_key.weight", "lin_value.weight")
    got = {}
    for key, layer in (("fused", fused), ("unfused", base)):
        x = x0.clone().requires_grad_(True)
        out = layer(x, *G["args"])
        out.backward(go)
        params = dict(layer.named_parameters())
        got[key] = dict({"output": out.detach(), "grad_x": x.grad}, **{"grad_" + nm: params[nm].grad for nm in names})
    s = np.array(SEED, dtype=np.int32).view(np.uint32)
    bits = softmax.restate_edge_dropout_bits(s[0], s[1], G["rows_h"][:, None], G["cols_h"][:, None], np.arange(H)[None, :])
    keep = _dev((bits >= np.uint32(_lib.edge_dropout_threshold(p))).astype(np.float64)) * float(np.float32(1) / (np.float32(1) - np.float32(p)))
    rows, cols = _dev(G["rows_h"]).long(), G["ci"].long()
    x64 = x0.double().requires_grad_(True)
    P = {nm: dict(fused.named_parameters())[nm].detach().double().requires_grad_(True) for nm in names}
    qkv = []
    with torch.no_grad():
        x16 = {m: getattr(fused, m)(x0) for m in ("lin_query", "lin_key", "lin_value")}
    for m in ("lin_query", "lin_key", "lin_value"):
        t = x64 @ P[m + ".weight"].t()
        qkv.append((t + (x16[m].double() - t).detach()).view(n, H, F))  # the value of torch's 16-bit linear, the float64 gradient
    ref_out, scale_out = _attention_float64(*qkv, rows, cols, n, float(np.float32(1.0 / np.sqrt(F))), keep)
    ref_out = ref_out.reshape(n, H * F)
    ref_out.backward(go.double())
    ref = dict({"output": ref_out.detach(), "grad_x": x64.grad}, **{"grad_" + nm: P[nm].grad for nm in names})
    scales = {"output": scale_out.reshape(n, H * F)}
    failed = []
    for name, want in ref.items():
        f, w = got["fused"][name].double().view_as(want), got["unfused"][name].double().view_as(want)
        top_ref = float(want.abs().max())
        assert top_ref > 0 and bool(torch.isfinite(f).all()), name
        err_f, err_u = float((f - want).abs().max()) / top_ref, float((w - want).abs().max()) / top_ref
        scale = scales.get(name, torch.zeros_like(want))
        bound = u * want.abs() + 1e-4 * torch.maximum(want.abs(), scale)
        worst = float(((f - want).abs() / torch.where(bound > 0, bound, torch.ones_like(bound))).max())
        rule1, rule2 = bool(((f - want).abs() <= bound).all()), err_f <= 2 * err_u
        print("TransformerConv fused_x16 %s %s: max error / max |ref| fused %.3g, fused=False %.3g (ratio %.3g); worst error / rule-1 "
              "bound %.3g" % (dtype, name, err_f, err_u, err_f / err_u if err_u else float("inf"), worst))
        if not (rule1 or rule2):
            failed.append((name, err_f, err_u, worst))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------------ memory

def test_fused_bf16_training_step_allocates_nothing_of_size_nnz_h(pkg):
    """n = 2048, 256 entries per row, H = F = 8, 16 input channels: the smallest array of nnz H elements, a 16-bit one, is 8 MiB and an
    fp32 one 16 MiB; a node-sized [n, H, F] bf16 array is 256 KiB. The bound is derived, not measured: forward plus backward of the
    layer allocate q, k, v, out, the skip term and the output (6 node arrays), stats (1/2), delta (1/4), grad_q, grad_k, grad_v (3),
    four [n, 16] gradients of x and their sums (under 2) and four small weight gradients — under 12 node arrays; the bound is 16,
    4 MiB: half the smallest edge array. One step runs before the measurement, so that what torch's matmuls keep is counted before."""
    import gespmm_amd

    n, deg, H_, F_, n_in = 2048, 256, 8, 8, 16
    rowptr, colind = _regular_graph(n, deg, 9)
    G = _square_of(rowptr, colind, n)
    nnz = n * deg
    node = n * H_ * F_ * 2
    bound = 16 * node
    assert nnz * H_ * 2 == 8 << 20 and bound == 4 << 20 and nnz * H_ * 4 > nnz * H_ * 2 > bound
    torch.manual_seed(35)
    layer = gespmm_amd.TransformerConv(n_in, F_, heads=H_, dropout=0.25, fused=True, fused_x16=True, attn_seed=_seed()).cuda().bfloat16().train()
    x = (torch.rand(n, n_in, device="cuda") - 0.5).bfloat16().requires_grad_(True)
    go = (torch.rand(n, H_ * F_, device="cuda") - 0.5).bfloat16()
    shapes = []

    def pack(t):
        shapes.append(tuple(t.shape))
        return t

    def step():
        layer.zero_grad(set_to_none=True)
        x.grad = None
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = layer(x, *G["args"])
        out.backward(go)
        return out.dtype

    step()
    del shapes[:]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    assert step() == torch.bfloat16
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak of a training step above the allocation before it: %d bytes; bound %d; one 16-bit [nnz, H] array %d" % (peak, bound, nnz * H_ * 2))
    assert shapes and not any(int(np.prod(s_)) >= nnz * H_ for s_ in shapes), shapes
    assert peak < bound, (peak, bound)
    for name, p in layer.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


# -------------------------------------------------------------------------------------------------------------------- training

def test_training_steps_on_cora_bf16_eager_and_captured(pkg):
    """The example's model as ``--fused --dtype bf16`` builds it on cora, dropout off: the losses are finite and go down, eager and
    replayed from a captured graph (the example's --graph-capture: a capturable Adam, three warm-up steps on a side stream)."""
    import gespmm_amd

    spec = importlib.util.spec_from_file_location("transformer_example_x16", os.path.join(ROOT, "examples", "transformer_custom.py"))
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
    y_train = y[train_idx]
    runs = {}
    for key in ("eager", "captured"):
        torch.manual_seed(0)
        model = ex.Net(n_feat, n_cls, 8, 8, dropout=0.0, fused=True).to(device).to(torch.bfloat16)
        for conv in (model.conv1, model.conv2):
            assert isinstance(conv, gespmm_amd.TransformerConv) and conv.fused and conv.fused_x16 and conv.lin_key.weight.dtype == torch.bfloat16
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
        assert all(np.isfinite(losses)) and losses[1] < losses[0] and losses[-1] < losses[0], runs
