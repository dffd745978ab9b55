"""GATConv(fused_aggregate / fused_backward, fused_x16=True) on fp16 / bf16 features: the layer against the existing 16-bit
GATConv(fused_score=True) bit for bit, GATAggregateFunction's fused backward against float64, its memory, autocast and the flag's rules."""
import numpy as np
import pytest
import torch

from attention_refs import gat_backward_float64
from test_gpu_gat import _dev, _rand, _random_graph
from test_gpu_gat_backward_layer import _regular_graph

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
IDS = ("fp16", "bf16")


def _same(got, want, what):
    assert got is not None and got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype)
    view = torch.int32 if got.dtype == torch.float32 else torch.int16
    bad = int((got.contiguous().view(view) != want.contiguous().view(view)).sum())
    assert bad == 0, "%s: %d of %d elements differ" % (what, bad, got.numel())


@pytest.fixture(scope="module")
def square(pkg):
    """About 200 nodes, every self-loop -> (n, rows and columns on the host, the five index tensors GATConv.forward takes)."""
    from gespmm_amd import graphs

    n = 203
    rowptr, colind, rows = _random_graph(n, edges=1200, seed=6)
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    return n, rows, colind, (rp, ci, colptr, rowind, order.to(torch.int32))


@pytest.mark.parametrize("dropout", (0.0, 0.5), ids=("plain", "dropout"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads,F", ((4, 8), (1, 16)))
def test_fused_aggregate_has_the_bits_of_the_16_bit_fused_score_layer(square, heads, F, dtype, dropout):
    import gespmm_amd

    n, _, _, a = square
    n_in = 24
    torch.manual_seed(3 + heads)
    score = gespmm_amd.GATConv(n_in, F, heads=heads, fused_score=True, dropout=dropout).cuda()
    fused = gespmm_amd.GATConv(n_in, F, heads=heads, fused_aggregate=True, fused_x16=True, dropout=dropout).cuda()
    with torch.no_grad():
        score.bias.copy_(_rand(score.bias.shape, 5))
    fused.load_state_dict(score.state_dict())
    score, fused = score.to(dtype), fused.to(dtype)
    x0, gout = (_rand((n, n_in), 6) * 4).to(dtype), _rand((n, heads * F), 8).to(dtype)
    seed = torch.tensor([17, -4], dtype=torch.int32, device="cuda") if dropout else None
    got = {}
    for key, layer in (("score", score), ("fused", fused)):
        x = x0.clone().requires_grad_(True)
        out = layer(x, *a, attn_seed=seed)
        assert out.dtype == dtype
        out.backward(gout)
        got[key] = [out.detach(), x.grad] + [p.grad for p in (layer.weight, layer.att_dst, layer.att_src, layer.bias)]
    for what, g, want in zip(("out", "grad_x", "grad_weight", "grad_att_dst", "grad_att_src", "grad_bias"), got["fused"], got["score"]):
        _same(g, want, (what, heads, F, dropout))
    if dropout:
        fused.eval()
        assert not torch.equal(fused(x0, *a), got["fused"][0]), "the mask must show in training mode"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H,F", ((4, 8), (1, 16)))
def test_function_fused_backward_on_16_bit_features(square, H, F, dtype):
    import gespmm_amd

    n, rows, cols, a = square
    el0, er0 = _rand((n, H), 1) * 4, _rand((n, H), 2) * 4
    feat0, gout = (_rand((n, H, F), 3) * 2).to(dtype), (_rand((n, H, F), 4) * 2).to(dtype)
    got = {}
    for fused in (False, True):
        el, er, feat = (t.clone().requires_grad_(True) for t in (el0, er0, feat0))
        out = gespmm_amd.GATAggregateFunction.apply(*a, el, er, feat, 0.2, fused)
        out.backward(gout)
        got[fused] = (out.detach(), feat.grad, el.grad, er.grad)
        assert out.dtype == dtype and feat.grad.dtype == dtype and el.grad.dtype == torch.float32 and er.grad.dtype == torch.float32
    _same(got[True][0], got[False][0], "forward")
    _same(got[True][1], got[False][1], "grad_feat: the same launch")
    ref_el, ref_er, sc_el, sc_er = gat_backward_float64(rows, cols, n, n, el0.cpu().numpy(), er0.cpu().numpy(), gout.float().cpu().numpy(),
                                                        feat0.float().cpu().numpy(), 0.2)
    for what, g, ref, scale in (("grad_el", got[True][2], ref_el, sc_el), ("grad_er", got[True][3], ref_er, sc_er)):
        bound = 1e-4 * np.maximum(np.abs(ref), scale)
        err = np.abs(g.cpu().numpy().astype(np.float64) - ref)
        worst = float((err / np.where(bound > 0, bound, 1.0)).max())
        print("H=%d F=%d %s %s: worst error / bound %.4f" % (H, F, dtype, what, worst))
        assert np.all(err <= bound), (H, F, what, worst)
    with pytest.raises(TypeError):  # el, er stay fp32
        gespmm_amd.GATAggregateFunction.apply(*a, el0.to(dtype), er0, feat0, 0.2, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_backward_allocates_nothing_edge_sized(pkg, dtype):
    """M = K = 2048, 64 entries per row, H = F = 8: one [nnz, H] fp32 array is 4 MiB. What the backward allocates is node-sized: the two
    widened operands (n H F fp32 each), grad_feat (n H F, 16-bit) and delta, grad_el, grad_er (n H fp32 each) — 1.44 MiB, plus the
    allocator's rounding of each block to 512 bytes."""
    import gespmm_amd
    from gespmm_amd import graphs

    n, deg, H, F = 2048, 64, 8, 8
    rowptr, colind = _regular_graph(n, deg, 9)
    edge_bytes = n * deg * H * 4
    cap = 2 * n * H * F * 4 + n * H * F * 2 + 3 * n * H * 4 + 6 * 512
    assert edge_bytes == 4 << 20 and 2 * cap < edge_bytes
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    el, er = (_rand((n, H), s).requires_grad_(True) for s in (1, 2))
    feat, gout = _rand((n, H, F), 3).to(dtype).requires_grad_(True), _rand((n, H, F), 4).to(dtype)
    out = gespmm_amd.GATAggregateFunction.apply(rp, ci, colptr, rowind, order.to(torch.int32), el, er, feat, 0.2, True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out.backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak of backward above the allocation before it: %d bytes, cap %d, one [nnz, H] array %d" % (peak, cap, edge_bytes))
    assert el.grad is not None and er.grad is not None and feat.grad.dtype == dtype
    assert peak <= cap, (peak, cap)


def test_autocast_and_the_rules_of_the_flag(square, monkeypatch):
    import gespmm_amd
    from gespmm_amd import spmm

    n, _, _, a = square
    torch.manual_seed(11)
    layer = gespmm_amd.GATConv(24, 8, heads=4, fused_backward=True, fused_x16=True, dropout=0.5).cuda()
    x = _rand((n, 24), 6).requires_grad_(True)
    calls, real = [], spmm.gat_aggregate_x16

    def spy(ptr, ind, el, er, stats, dense, **kw):
        r = real(ptr, ind, el, er, stats, dense, **kw)
        calls.append((el.dtype, dense.dtype, r.dtype, bool(kw.get("transposed")), kw.get("dropout") is not None))
        return r

    monkeypatch.setattr(spmm, "gat_aggregate_x16", spy)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(x, *a)
    # x @ W comes out bf16: the aggregation is the 16-bit one (the bias add, outside the autocast lists, promotes its result)
    assert calls == [(torch.float32, torch.bfloat16, torch.bfloat16, False, True)] and out.dtype == torch.float32, (calls, out.dtype)
    out.float().sum().backward()
    assert calls[1:] == [(torch.float32, torch.bfloat16, torch.bfloat16, True, True)], calls  # grad_feat: transposed, the same mask
    monkeypatch.undo()
    for p in (x, layer.weight, layer.att_dst, layer.att_src, layer.bias):
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all())
    assert bool((layer.att_dst.grad != 0).any()) and bool((layer.weight.grad != 0).any())
    # fp32 features ignore the flag: the bits of the layer without it
    plain = gespmm_amd.GATConv(24, 8, heads=4, fused_backward=True).cuda()
    plain.load_state_dict(layer.state_dict())
    _same(layer.eval()(x.detach(), *a), plain.eval()(x.detach(), *a), "fp32 features")
    with pytest.raises(ValueError, match="fused_x16"):
        gespmm_amd.GATConv(24, 8, heads=4, fused_x16=True)
    with pytest.raises(ValueError, match="fused_x16"):
        gespmm_amd.GATConv(24, 8, heads=4, fused_score=True, fused_x16=True)
    with pytest.raises(TypeError, match="gat_aggregate"):
        gespmm_amd.GATConv(24, 8, heads=4, fused_aggregate=True).cuda().bfloat16()(x.detach().bfloat16(), *a)
