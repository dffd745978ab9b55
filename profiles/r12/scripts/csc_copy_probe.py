"""One-off: on products-sbm at H = 4, is the CSC-ordered copy alpha[csc_order] (torch advanced indexing) what it should be?"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gat_softmax_timing import load_graph  # noqa: E402
from gespmm_amd import graphs, softmax, spmm  # noqa: E402

dev = torch.device("cuda")
rp, ci, K = load_graph("products-sbm", dev)
M, nnz = rp.numel() - 1, ci.numel()
colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
for H in (4, 8):
    gen = torch.Generator(device=dev).manual_seed(1)
    el = (torch.rand(M, H, device=dev, generator=gen) - 0.5) * 4
    er = (torch.rand(K, H, device=dev, generator=gen) - 0.5) * 4
    alpha = softmax.gat_edge_softmax(rp, ci, el, er, negative_slope=0.2)
    a1 = alpha[order].contiguous()
    a2 = torch.stack([alpha[:, h].contiguous()[order] for h in range(H)], dim=1).contiguous()
    a3 = torch.index_select(alpha, 0, order)
    bad12 = (a1.view(torch.int32) != a2.view(torch.int32))
    print("H=%d nnz=%d: alpha[order] vs per-head gather: %d words differ (first bad entry %s); index_select vs per-head: %d" % (
        H, nnz, int(bad12.sum()), int(bad12.any(dim=1).nonzero()[0]) if bool(bad12.any()) else None,
        int((a3.view(torch.int32) != a2.view(torch.int32)).sum())), flush=True)
    if H == 4:
        F = 16
        gout = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
        stats = softmax.gat_softmax_stats(rp, ci, el, er, negative_slope=0.2)
        mine = spmm.gat_aggregate(colptr, rowind, el, er, stats, gout, negative_slope=0.2, transposed=True)
        for name, a in (("alpha[order]", a1), ("per-head gather", a2)):
            got = spmm.csr_spmm_heads(colptr, rowind, a, gout)
            print("   csr_spmm_heads on %s vs gat_aggregate(transposed): %d words differ" % (
                name, int((got.view(torch.int32) != mine.view(torch.int32)).sum())), flush=True)
    del alpha, a1, a2, a3
