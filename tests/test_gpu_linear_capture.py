"""One captured training step (forward and backward) of the layers on the aggregate-and-linear kernels, after test_gpu_graph_capture.py:
RGCNConv in bf16 with fused_weight_grad=True, RGCNConv in fp32 and SAGEConv(fused_linear=True). One stream, no environment. The graph
is replayed twice with new values written in place into the input; outputs and gradients must have the bits of an eager step."""
import pytest
import torch

from test_gpu_graph_capture import _capture
from test_gpu_spmm_relational import _stacked
from test_gpu_max_arg import K0

pytestmark = pytest.mark.gpu


def _layer(kind):
    from gespmm_amd import RGCNConv, SAGEConv, graphs

    R, M, K, N_out = 3, K0, 64, 48
    torch.manual_seed(11)
    if kind == "sage":
        srp, sci = _stacked(M, 1)
        cp, ri = graphs.transpose_csr(srp, sci)
        return SAGEConv(K, N_out, "mean", fused_linear=True).cuda().to(torch.bfloat16), torch.bfloat16, (srp, sci, cp, ri)
    srp, sci = _stacked(M, R)
    cp, ri = graphs.transpose_stacked_csr(srp, sci, R, K0)
    if kind == "rgcn-bf16":
        return RGCNConv(K, N_out, R, fused_weight_grad=True).cuda().to(torch.bfloat16), torch.bfloat16, (srp, sci, cp, ri)
    return RGCNConv(K, N_out, R).cuda(), torch.float32, (srp, sci, cp, ri)


@pytest.mark.parametrize("kind", ("rgcn-bf16", "rgcn-fp32", "sage"))
def test_a_captured_step_replays_with_the_eager_bits(pkg, kind):
    layer, dtype, arrays = _layer(kind)
    M, K, N_out = K0, 64, 48
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=gen).to(dtype).cuda().requires_grad_(True)
    go = torch.randn(M, N_out, generator=gen).to(dtype).cuda()
    params = list(layer.parameters())

    def step():
        out = layer(x, *arrays)
        return (out,) + torch.autograd.grad(out, [x] + params, go)

    graph, captured = _capture(step)
    for seed in (2, 3):
        with torch.no_grad():
            x.copy_(torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).to(dtype))  # new contents, same address
        for t in captured:
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().clone() for t in captured]
        eager = step()
        torch.cuda.synchronize()
        assert len(got) == len(eager) == 2 + len(params)
        for name, a, b in zip(["out", "grad_x"] + [n for n, _ in layer.named_parameters()], got, eager):
            assert not torch.isnan(a).any(), (kind, seed, name)
            assert torch.equal(a, b.detach()), (kind, seed, name)
