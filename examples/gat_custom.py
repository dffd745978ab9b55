#!/usr/bin/env python3
"""GAT training on the custom ops: two ``GATConv`` layers — 8 heads x 8 features, then 1 head — the model of Velickovic et al.
(2018) for the citation graphs. Every sparse step is a kernel of this library: the additive scores (multi-head SDDMM), the softmax over
each node's edges (edge softmax, leaky ReLU fused in), the aggregation (multi-head SpMM), and their backwards.

    python examples/gat_custom.py                                  # pubmed
    python examples/gat_custom.py --dataset cora --epochs 50
    python examples/gat_custom.py --graph-capture                  # replay each step from a HIP graph (one stream)
    python examples/gat_custom.py --fused-score                    # el + er added inside the softmax kernel: no score array
    python examples/gat_custom.py --fused-aggregate                # ... and the weights computed inside the aggregation: no alpha array
    python examples/gat_custom.py --fused-backward                 # ... and no [nnz, H] array in the backward either
    python examples/gat_custom.py --fused-backward --attn-dropout 0.6   # the paper's dropout on the attention coefficients: a mask recomputed
                                                                   # from a seed wherever an entry is seen, never stored
    python examples/gat_custom.py --seed 0 --fused-aggregate       # seeded parameters and dropout: the losses of --seed 0 --fused-score
    python examples/gat_custom.py --v2                             # two ``GATv2Conv`` layers (Brody et al.): the non-linearity inside the
                                                                   # score's sum, one kernel, nothing of size nnz x H x F
    python examples/gat_custom.py --v2 --fused-attention           # ``GATv2Conv(fused=True)``: score, softmax, dropout and aggregation in
                                                                   # one kernel, the backward in two: no [nnz, H] array in a step
    python examples/gat_custom.py --dtype bf16                     # a .bfloat16() model on bf16 features (or fp16): the aggregation is the
                                                                   # 16-bit multi-head product, everything edge-sized stays fp32
    python examples/gat_custom.py --v2 --dtype bf16                # ``GATv2Conv`` as a 16-bit model: the edge score and its two gradient
                                                                   # passes read bf16 (or fp16) node terms, att and the score stay fp32
    python examples/gat_custom.py --v2 --fused-attention --dtype bf16   # ``GATv2Conv(fused=True, fused_x16=True)``: the fused attention on
                                                                   # bf16 (or fp16) node terms: no [nnz, H] array AND half the node bytes

Data handling is that of examples/gcn_custom.py (same bundled adjacency, same synthetic features / labels / masks, so accuracy is
chance level by construction); the point of the script is that the loss goes down and what an epoch costs.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gespmm_amd  # noqa: E402,F401
from gcn_custom import load_edges, proc  # noqa: E402
from gespmm_amd import GATConv, GATv2Conv, graphs  # noqa: E402


def gat_graph(edge_index, n_v, device, int32_order=False):
    """The self-looped graph in both index orders, plus the edge order between them (what ``GATConv.forward`` takes).
    ``int32_order``: the order as int32, converted here once — what ``GATConv(fused_score=True)`` hands its kernels as it is."""
    g = proc(edge_index, n_v, device)
    rowptr, colind = g["rowptr"], g["colind"]
    colptr, rowind, order = graphs.transpose_csr(rowptr, colind, n_v, return_order=True)
    if int32_order:
        order = order.to(torch.int32)
    return {"rowptr": rowptr, "colind": colind, "colptr": colptr, "rowind": rowind, "csc_order": order}


class Net(torch.nn.Module):
    def __init__(self, n_in, n_out, n_hidden=8, heads=8, dropout=0.6, fused_score=False, fused_aggregate=False, fused_backward=False,
                 attn_dropout=0.0, v2=False, fused_attention=False):
        super().__init__()
        if fused_attention and not v2:
            raise ValueError("fused_attention is GATv2Conv(fused=True): it needs v2=True")
        if v2:
            if fused_score or fused_aggregate or fused_backward:
                raise ValueError("fused_score, fused_aggregate and fused_backward are GATConv's: GATv2Conv has fused_attention")
            # (fused_x16: a 16-bit model runs the fused attention on 16-bit node terms; an fp32 one runs what fused=True runs)
            fused = dict(fused=fused_attention, fused_x16=fused_attention)
            self.conv1 = GATv2Conv(n_in, n_hidden, heads=heads, concat=True, dropout=attn_dropout, **fused)
            self.conv2 = GATv2Conv(n_hidden * heads, n_out, heads=1, concat=False, dropout=attn_dropout, **fused)
        else:
            fused = dict(fused_score=fused_score, fused_aggregate=fused_aggregate, fused_backward=fused_backward, dropout=attn_dropout)
            self.conv1 = GATConv(n_in, n_hidden, heads=heads, concat=True, **fused)
            self.conv2 = GATConv(n_hidden * heads, n_out, heads=1, concat=False, **fused)
        self.dropout = dropout

    def forward(self, x, g):
        a = (g["rowptr"], g["colind"], g["colptr"], g["rowind"], g["csc_order"])
        x = F.dropout(x, p=self.dropout, training=self.training)
        x = F.elu(self.conv1(x, *a))
        x = F.dropout(x, p=self.dropout, training=self.training)
        return F.log_softmax(self.conv2(x, *a), dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-hidden", type=int, default=8, help="features per head of the first layer")
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--dataset", default="pubmed")
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--dropout", type=float, default=0.6, help="dropout on the features in front of each layer")
    ap.add_argument("--attn-dropout", type=float, default=0.0,
                    help="GATConv(dropout=P) in both layers: dropout on the attention coefficients (the paper: 0.6)")
    ap.add_argument("--graph-capture", action="store_true", help="capture one training step in a HIP graph")
    ap.add_argument("--fused-score", action="store_true", help="GATConv(fused_score=True): score and softmax in one kernel")
    ap.add_argument("--fused-aggregate", action="store_true",
                    help="GATConv(fused_aggregate=True): softmax and aggregation in one kernel, no [nnz, H] array saved")
    ap.add_argument("--fused-backward", action="store_true",
                    help="GATConv(fused_backward=True): the fused aggregation, and its backward for the attention terms in two "
                         "launches with no [nnz, H] array")
    ap.add_argument("--v2", action="store_true",
                    help="GATv2Conv in both layers (the score's non-linearity inside its sum); not together with --fused-score, "
                         "--fused-aggregate or --fused-backward")
    ap.add_argument("--fused-attention", action="store_true",
                    help="with --v2: GATv2Conv(fused=True), the whole attention in one kernel and its backward in two, no [nnz, H] array")
    ap.add_argument("--seed", type=int, default=None,
                    help="torch.manual_seed before the model is made (parameters and dropout masks): two runs, or two fused settings, "
                         "then print the same losses")
    ap.add_argument("--dtype", choices=("fp32", "bf16", "fp16"), default="fp32",
                    help="cast the model and the features (bf16 / fp16: GATConv on the 16-bit multi-head product, with --v2 GATv2Conv "
                         "on the 16-bit edge score too, with --v2 --fused-attention the fused attention on 16-bit node terms; not "
                         "with --fused-aggregate or --fused-backward, which are fp32 only)")
    args = ap.parse_args()
    if args.dtype != "fp32" and (args.fused_aggregate or args.fused_backward or (args.fused_attention and not args.v2)):
        ap.error("--dtype %s: --fused-aggregate and --fused-backward run fp32-only kernels; use the default path, --fused-score, --v2 "
                 "or --v2 --fused-attention" % args.dtype)
    if args.v2 and (args.fused_score or args.fused_aggregate or args.fused_backward):
        ap.error("--fused-score, --fused-aggregate and --fused-backward are GATConv's: --v2 has --fused-attention")
    if args.fused_attention and not args.v2:
        ap.error("--fused-attention is GATv2Conv(fused=True): it needs --v2")
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device (the ops have no CPU path)")
    device = torch.device("cuda")

    edge_index, n_v, n_feat, n_cls = load_edges(args.dataset, device)
    g = gat_graph(edge_index, n_v, device, int32_order=args.fused_score or args.fused_aggregate or args.fused_backward)
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n_v, n_feat, generator=gen)
    x = (x / x.sum(1, keepdim=True)).to(device)
    y = torch.randint(0, n_cls, (n_v,), generator=gen).to(device)
    perm = torch.randperm(n_v, generator=gen)
    masks = {}
    for name, (a, b) in (("train", (0, 20 * n_cls)), ("val", (20 * n_cls, 20 * n_cls + 500)),
                         ("test", (20 * n_cls + 500, 20 * n_cls + 1500))):
        m = torch.zeros(n_v, dtype=torch.bool)
        m[perm[a:b]] = True
        masks[name] = m.to(device)

    if args.seed is not None:
        torch.manual_seed(args.seed)
    model = Net(n_feat, n_cls, args.n_hidden, args.heads, args.dropout, fused_score=args.fused_score,
                fused_aggregate=args.fused_aggregate, fused_backward=args.fused_backward, attn_dropout=args.attn_dropout, v2=args.v2,
                fused_attention=args.fused_attention).to(device)
    if args.dtype != "fp32":
        dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
        model = model.to(dtype)
        x = x.to(dtype)
    # (fp16 parameters: Adam's default eps, 1e-8, is zero in fp16 and a parameter whose gradient is zero would be updated by 0 / 0)
    adam = {"eps": 1e-4} if args.dtype == "fp16" else {}
    optimizer = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4, capturable=args.graph_capture, **adam)
    train_idx = masks["train"].nonzero().squeeze(1)
    y_train = y[train_idx]

    def train_step():
        optimizer.zero_grad(set_to_none=False)
        out = model(x, g)
        loss = F.nll_loss(out.index_select(0, train_idx), y_train)
        loss.backward()
        optimizer.step()
        return loss

    @torch.no_grad()
    def test():
        model.eval()
        logits, accs = model(x, g), []
        for m in masks.values():
            pred = logits[m].max(1)[1]
            accs.append(pred.eq(y[m]).sum().item() / m.sum().item())
        model.train()
        return accs

    model.train()
    graph = None
    if args.graph_capture:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                train_step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = train_step()
    else:
        for _ in range(3):
            train_step()

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    best_val = test_acc = 0.0
    for epoch in range(1, args.epochs + 1):
        if graph is not None:
            graph.replay()
            loss = static_loss
        else:
            loss = train_step()
        if epoch % 50 == 0 or epoch == args.epochs:
            tr, va, te = test()
            if va > best_val:
                best_val, test_acc = va, te
            print("Epoch: {:03d}, Loss: {:.4f}, Train: {:.4f}, Val: {:.4f}, Test: {:.4f}".format(
                epoch, float(loss), tr, best_val, test_acc))
    e1.record()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print("dataset=%s n=%d nnz(+I)=%d heads=%d hidden=%d graph_capture=%s fused_score=%s fused_aggregate=%s fused_backward=%s%s" %
          (args.dataset, n_v, g["colind"].numel(), args.heads, args.n_hidden, args.graph_capture, args.fused_score, args.fused_aggregate,
           args.fused_backward, (" attn_dropout=%g" % args.attn_dropout if args.attn_dropout else "") + (" v2=True" if args.v2 else "") + (" fused_attention=True" if args.fused_attention else "") +
           (" dtype=%s" % args.dtype if args.dtype != "fp32" else "")))
    print("epochs=%d  gpu %.3f ms/epoch  wall %.3f ms/epoch" %
          (args.epochs, e0.elapsed_time(e1) / args.epochs, wall * 1e3 / args.epochs))


if __name__ == "__main__":
    main()
