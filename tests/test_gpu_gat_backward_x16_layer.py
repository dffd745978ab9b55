"""GATAggregateFunction(fused_backward=True) on fp16 / bf16 features: grad_el and grad_er come from the 16-bit forms of the two backward
kernels — the bits of the fp32 ops on the widened tensors — and the backward no longer makes an fp32 copy of grad_out or feat."""
import pytest
import torch

from test_gpu_gat import _dev, _rand
from test_gpu_gat_backward_layer import _regular_graph
from test_gpu_gat_x16_layer import DTYPES, IDS, _same, square  # noqa: F401  (square: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H,F", ((4, 8), (2, 32)))  # the lane form, the group form
def test_gradients_through_the_function(square, H, F, dtype):  # noqa: F811
    import gespmm_amd
    from gespmm_amd import softmax

    n, _, _, a = square
    rp, ci, cp, ri, _ = a
    el0, er0 = _rand((n, H), 1) * 4, _rand((n, H), 2) * 4
    feat0, gout = (_rand((n, H, F), 3) * 2).to(dtype), (_rand((n, H, F), 4) * 2).to(dtype)
    got = {}
    for fused in (False, True):
        el, er, feat = (t.clone().requires_grad_(True) for t in (el0, er0, feat0))
        gespmm_amd.GATAggregateFunction.apply(*a, el, er, feat, 0.2, fused).backward(gout)
        got[fused] = (feat.grad, el.grad, er.grad)
    _same(got[True][0], got[False][0], "grad_feat: untouched")
    stats = softmax.gat_softmax_stats(rp, ci, el0, er0, negative_slope=0.2)
    delta, want_el = softmax.gat_backward_el(rp, ci, el0, er0, stats, gout.float(), feat0.float(), negative_slope=0.2)
    want_er = softmax.gat_backward_er(cp, ri, el0, er0, stats, delta, gout.float(), feat0.float(), negative_slope=0.2)
    delta16, el16 = softmax.gat_backward_el_x16(rp, ci, el0, er0, stats, gout, feat0, negative_slope=0.2)
    er16 = softmax.gat_backward_er_x16(cp, ri, el0, er0, stats, delta16, gout, feat0, negative_slope=0.2)
    for what, g, op16, want in (("grad_el", got[True][1], el16, want_el), ("grad_er", got[True][2], er16, want_er)):
        _same(g, want, what + ": the fp32 op on widened tensors")
        _same(op16, want, what + ": the 16-bit op")


def test_backward_makes_no_fp32_copy_of_a_node_tensor(pkg):
    """M = K = 4096, 8 entries per row, H = 4, F = 64 in bf16, only el and er asking for gradients: one widened operand is 4 K H F bytes
    = 4 MiB, what the backward makes (delta, grad_el, grad_er: 64 KiB each) far less. The peak of backward() above what was allocated
    before it stays below ONE widened operand; the widening composition made two."""
    import gespmm_amd
    from gespmm_amd import graphs

    n, deg, H, F = 4096, 8, 4, 64
    rowptr, colind = _regular_graph(n, deg, 9)
    rp, ci = _dev(rowptr), _dev(colind)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, n, return_order=True)
    el, er = (_rand((n, H), s).requires_grad_(True) for s in (1, 2))
    feat, gout = _rand((n, H, F), 3).bfloat16(), _rand((n, H, F), 4).bfloat16()
    out = gespmm_amd.GATAggregateFunction.apply(rp, ci, colptr, rowind, order.to(torch.int32), el, er, feat, 0.2, True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out.backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("backward peak above entry: %d bytes; one widened operand: %d" % (peak, 4 * n * H * F))
    assert el.grad is not None and er.grad is not None
    assert peak < 4 * n * H * F, peak
