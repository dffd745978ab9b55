"""16-bit attention: MultiHeadSPMMFunction / MultiHeadSDDMMFunction on fp16 / bf16 node tensors, and GATConv / TransformerConv as
``.half()`` / ``.bfloat16()`` layers and under autocast. The functions are WIRING: forward and every gradient are bit-equal to the direct
op call they are documented to make (the ops themselves are pinned in test_gpu_heads_x16.py / test_gpu_sddmm_heads_x16.py); the layers
are bit-equal to the hand composition of their documented steps. One numeric check against float64 closes the file."""
import numpy as np
import pytest
import torch

from helpers import edge_case_csr

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
IDS = ("fp16", "bf16")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    bad = int((got.contiguous().view(view) != want.contiguous().view(view)).sum())
    assert bad == 0, "%s: %d of %d elements differ" % (what, bad, got.numel())


@pytest.fixture(scope="module")
def square():
    """The edge-case pattern made square: columns folded onto the 21 rows (repeated columns stay), both index orders."""
    from gespmm_amd import graphs

    g = edge_case_csr()
    n = g["M"]
    rp, ci = _dev(g["rowptr"]), _dev((g["colind"] % n).astype(np.int32))
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    return {"n": n, "nnz": g["nnz"], "rp": rp, "ci": ci, "colptr": colptr, "rowind": rowind, "order": order,
            "order32": order.to(torch.int32), "args": (rp, ci, colptr, rowind, order)}


def _rand(gen, *shape):
    return torch.rand(*shape, device="cuda", generator=gen) - 0.5


# ------------------------------------------------------------------------------------------------------------ the two functions

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads_sddmm", (True, False))
def test_multi_head_spmm_function(pkg, square, dtype, heads_sddmm):
    import gespmm_amd
    from gespmm_amd import sddmm, spmm

    G, H, F = square, 4, 8
    gen = torch.Generator(device="cuda").manual_seed(3)
    feat = _rand(gen, G["n"], H, F).to(dtype).requires_grad_(True)
    weight = _rand(gen, G["nnz"], H).requires_grad_(True)
    out = gespmm_amd.MultiHeadSPMMFunction.apply(*G["args"], feat, weight, None, heads_sddmm)
    assert out.dtype == dtype and out.shape == (G["n"], H, F)
    _bits_equal(out.detach(), spmm.csr_spmm_heads_x16(G["rp"], G["ci"], weight.detach(), feat.detach()), "forward")
    go = _rand(gen, G["n"], H, F).to(dtype)
    out.backward(go)
    assert feat.grad.dtype == dtype and weight.grad.dtype == torch.float32
    _bits_equal(feat.grad, spmm.csr_spmm_heads_x16(G["colptr"], G["rowind"], weight.detach()[G["order"]].contiguous(), go), "grad_feat")
    if heads_sddmm:
        want = sddmm.csr_sddmm_heads_x16(G["rp"], G["ci"], go, feat.detach())
    else:
        want = torch.stack([sddmm.csr_sddmm(G["rp"], G["ci"], go[:, h, :].contiguous(), feat.detach()[:, h, :].contiguous())
                            for h in range(H)], dim=1)
    _bits_equal(weight.grad, want, "grad_weight")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_multi_head_sddmm_function(pkg, square, dtype):
    import gespmm_amd
    from gespmm_amd import sddmm, spmm

    G, H, F = square, 4, 8
    gen = torch.Generator(device="cuda").manual_seed(4)
    q = _rand(gen, G["n"], H, F).to(dtype).requires_grad_(True)
    k = _rand(gen, G["n"], H, F).to(dtype).requires_grad_(True)
    s = gespmm_amd.MultiHeadSDDMMFunction.apply(*G["args"], q, k)
    assert s.dtype == torch.float32 and s.shape == (G["nnz"], H)
    _bits_equal(s.detach(), sddmm.csr_sddmm_heads_x16(G["rp"], G["ci"], q.detach(), k.detach()), "forward")
    gs = _rand(gen, G["nnz"], H)
    s.backward(gs)
    assert q.grad.dtype == dtype and k.grad.dtype == dtype
    _bits_equal(q.grad, spmm.csr_spmm_heads_x16(G["rp"], G["ci"], gs, k.detach()), "grad_q")
    _bits_equal(k.grad, spmm.csr_spmm_heads_x16(G["colptr"], G["rowind"], gs[G["order"]].contiguous(), q.detach()), "grad_k")


def test_plans_and_mixed_dtypes_raise(pkg, square):
    import gespmm_amd
    from gespmm_amd import spmm

    G, H, F = square, 4, 8
    gen = torch.Generator(device="cuda").manual_seed(5)
    feat, weight = _rand(gen, G["n"], H, F), _rand(gen, G["nnz"], H)
    plans = (spmm.SpmmPlan(G["rp"], G["ci"], G["n"], H * F), spmm.SpmmPlan(G["colptr"], G["rowind"], G["n"], H * F))
    gespmm_amd.MultiHeadSPMMFunction.apply(*G["args"], feat, weight, plans)  # fp32 keeps its plans
    for dtype in DTYPES:
        with pytest.raises(TypeError):
            gespmm_amd.MultiHeadSPMMFunction.apply(*G["args"], feat.to(dtype), weight, plans)
        with pytest.raises(TypeError):
            gespmm_amd.MultiHeadSDDMMFunction.apply(*G["args"], feat.to(dtype), feat.to(dtype), plans)
        with pytest.raises(TypeError):  # edge weights stay fp32
            gespmm_amd.MultiHeadSPMMFunction.apply(*G["args"], feat.to(dtype), weight.to(dtype))
        with pytest.raises(TypeError):  # q and k of one dtype
            gespmm_amd.MultiHeadSDDMMFunction.apply(*G["args"], feat.to(dtype), feat)
    with pytest.raises(TypeError):
        gespmm_amd.MultiHeadSDDMMFunction.apply(*G["args"], feat.half(), feat.bfloat16())


# ------------------------------------------------------------------------------------------------------------------- GATConv

def _gat_by_hand(layer, x, G, fused_score):
    """The documented steps of a 16-bit GATConv on the ops themselves."""
    from gespmm_amd import sddmm, softmax, spmm

    n, H, F = x.shape[0], layer.heads, layer.out_channels
    xw = (x @ layer.weight).view(n, H, F)
    assert xw.dtype == x.dtype
    el = (xw * layer.att_dst).sum(-1).float()
    er = (xw * layer.att_src).sum(-1).float()
    if fused_score:
        alpha = softmax.gat_edge_softmax(G["rp"], G["ci"], el, er, negative_slope=layer.negative_slope)
    else:
        q = torch.stack((el, torch.ones_like(el)), dim=-1)
        k = torch.stack((torch.ones_like(er), er), dim=-1)
        score = sddmm.csr_sddmm_heads(G["rp"], G["ci"], q, k)
        alpha = softmax.edge_softmax(G["rp"], score, negative_slope=layer.negative_slope)
    assert alpha.dtype == torch.float32
    out = spmm.csr_spmm_heads_x16(G["rp"], G["ci"], alpha, xw.contiguous())
    return out.reshape(n, H * F) + layer.bias


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fused_score", (False, True))
def test_gatconv_16_bit(pkg, square, dtype, fused_score):
    import gespmm_amd

    G = square
    torch.manual_seed(7)
    layer = gespmm_amd.GATConv(12, 8, heads=4, fused_score=fused_score).cuda().to(dtype)
    with torch.no_grad():
        layer.bias.copy_(torch.rand_like(layer.bias) - 0.5)
    x = (torch.rand(G["n"], 12, device="cuda") - 0.5).to(dtype)
    order = G["order32"] if fused_score else G["order"]
    out = layer(x, G["rp"], G["ci"], G["colptr"], G["rowind"], order)
    assert out.dtype == dtype and out.shape == (G["n"], 32)
    with torch.no_grad():
        _bits_equal(out.detach(), _gat_by_hand(layer, x, G, fused_score), "output")
    out.float().square().sum().backward()
    for name, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == dtype and p.grad.shape == p.shape, name
        assert bool(torch.isfinite(p.grad).all()), name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gatconv_fused_aggregate_is_fp32_only(pkg, square, dtype):
    import gespmm_amd

    G = square
    x = (torch.rand(G["n"], 12, device="cuda") - 0.5).to(dtype)
    for kw in ({"fused_aggregate": True}, {"fused_backward": True}):
        layer = gespmm_amd.GATConv(12, 8, heads=4, **kw).cuda().to(dtype)
        with pytest.raises(TypeError, match="gat_aggregate"):
            layer(x, G["rp"], G["ci"], G["colptr"], G["rowind"], G["order32"])
        layer.float()(x.float(), G["rp"], G["ci"], G["colptr"], G["rowind"], G["order32"])  # fp32 still runs


@pytest.mark.parametrize("fused_score", (False, True))
def test_gatconv_autocast(pkg, square, monkeypatch, fused_score):
    """fp32 parameters under torch.autocast(bfloat16): x @ W comes out bf16, so the aggregation is the 16-bit product."""
    import gespmm_amd
    from gespmm_amd import spmm

    G = square
    torch.manual_seed(8)
    layer = gespmm_amd.GATConv(12, 8, heads=4, fused_score=fused_score).cuda()
    x = torch.rand(G["n"], 12, device="cuda") - 0.5
    calls = []
    real = spmm.csr_spmm_heads_x16

    def spy(rowptr, colind, values, dense, out=None):
        r = real(rowptr, colind, values, dense, out=out)
        calls.append((values.dtype, dense.dtype, r.dtype))
        return r

    monkeypatch.setattr(spmm, "csr_spmm_heads_x16", spy)
    order = G["order32"] if fused_score else G["order"]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(x, G["rp"], G["ci"], G["colptr"], G["rowind"], order)
    assert calls == [(torch.float32, torch.bfloat16, torch.bfloat16)], calls
    out.float().square().sum().backward()
    assert len(calls) == 2 and calls[1] == (torch.float32, torch.bfloat16, torch.bfloat16), calls  # grad_feat: the 16-bit product again
    for name, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name


# ----------------------------------------------------------------------------------------------------------- TransformerConv

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_transformerconv_16_bit(pkg, square, dtype):
    import math

    import gespmm_amd
    from gespmm_amd import sddmm, softmax, spmm

    G, H, F = square, 4, 8
    torch.manual_seed(9)
    layer = gespmm_amd.TransformerConv(12, F, heads=H, fused=False).cuda().to(dtype)
    x = (torch.rand(G["n"], 12, device="cuda") - 0.5).to(dtype)
    out = layer(x, G["rp"], G["ci"], G["colptr"], G["rowind"], G["order"])
    assert out.dtype == dtype and out.shape == (G["n"], H * F)
    with torch.no_grad():
        n = G["n"]
        q, k, v = (lin(x).view(n, H, F) for lin in (layer.lin_query, layer.lin_key, layer.lin_value))
        score = sddmm.csr_sddmm_heads_x16(G["rp"], G["ci"], q.contiguous(), k.contiguous()) * (1.0 / math.sqrt(F))
        alpha = softmax.edge_softmax(G["rp"], score)
        assert score.dtype == torch.float32 and alpha.dtype == torch.float32
        want = spmm.csr_spmm_heads_x16(G["rp"], G["ci"], alpha, v.contiguous()).reshape(n, H * F) + layer.lin_skip(x)
        _bits_equal(out.detach(), want, "output")
    out.float().square().sum().backward()
    for name, p in layer.named_parameters():
        assert p.grad is not None and p.grad.dtype == dtype and bool(torch.isfinite(p.grad).all()), name
    fused = gespmm_amd.TransformerConv(12, F, heads=H, fused=True).cuda().to(dtype)
    with pytest.raises(TypeError, match="dot_attention"):
        fused(x, G["rp"], G["ci"], G["colptr"], G["rowind"])
    fused.float()(x.float(), G["rp"], G["ci"], G["colptr"], G["rowind"])  # fp32 still runs


# ------------------------------------------------------------------------------------------------------- numbers, once

@pytest.mark.parametrize("dtype,u", ((torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)), ids=IDS)
def test_product_and_grad_feat_against_float64(pkg, square, dtype, u):
    """|got - ref| <= u |ref| + 1e-4 max(|ref|, sum |a b|) against the float64 product of the widened operands: one rounding (u) of an
    fp32 sum that itself meets the project's rule for fp32 sums. |val|, |B| <= 1: no fp16 sum of 200 terms leaves the normal range."""
    import gespmm_amd

    G, H, F = square, 4, 8
    gen = torch.Generator(device="cuda").manual_seed(12)
    feat = (2 * _rand(gen, G["n"], H, F)).to(dtype).requires_grad_(True)
    weight = 2 * _rand(gen, G["nnz"], H)
    go = (2 * _rand(gen, G["n"], H, F)).to(dtype)
    out = gespmm_amd.MultiHeadSPMMFunction.apply(*G["args"], feat, weight)
    out.backward(go)
    rows = torch.repeat_interleave(torch.arange(G["n"], device="cuda"), torch.diff(G["rp"]).long())
    cols = G["ci"].long()
    w = weight.double()[:, :, None]

    def check(got, src, dst_index, src_index, what):
        terms = w * src.detach().double()[src_index]                     # [nnz, H, F]
        ref = torch.zeros(G["n"], H, F, dtype=torch.float64, device="cuda").index_add_(0, dst_index, terms)
        scale = torch.zeros_like(ref).index_add_(0, dst_index, terms.abs())
        err = (got.detach().double() - ref).abs()
        bound = u * ref.abs() + 1e-4 * torch.maximum(ref.abs(), scale)
        assert bool((err <= bound).all()), (what, float((err - bound).max()))

    check(out, feat, rows, cols, "forward")
    check(feat.grad, go, cols, rows, "grad_feat")
