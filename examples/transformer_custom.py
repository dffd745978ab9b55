#!/usr/bin/env python3
"""Graph transformer training on the custom ops: two ``TransformerConv`` layers — 8 heads x 8 features, then 1 head — scaled dot-product
attention over each node's edges with a skip connection (Shi et al., UniMP; PyG's ``TransformerConv``). Every sparse step is a kernel of
this library.

    python examples/transformer_custom.py                          # pubmed; the composition: multi-head SDDMM, edge softmax, multi-head SpMM
    python examples/transformer_custom.py --dataset cora --epochs 50
    python examples/transformer_custom.py --fused                  # ONE kernel forward, two backward: no [nnz, H] array in either direction
    python examples/transformer_custom.py --fused --attn-dropout 0.3    # dropout on the attention coefficients: a mask recomputed from a
                                                                   # seed wherever an entry is seen, never stored
    python examples/transformer_custom.py --fused --graph-capture  # replay each step from a HIP graph (one stream)
    python examples/transformer_custom.py --beta                   # the gated skip connection
    python examples/transformer_custom.py --seed 0 --fused         # seeded parameters and dropout: the losses of --seed 0 to rounding
    python examples/transformer_custom.py --dtype bf16             # a .bfloat16() model on bf16 features (or fp16): 16-bit SDDMM and
                                                                   # aggregation, everything edge-sized stays fp32
    python examples/transformer_custom.py --fused --dtype bf16     # ``TransformerConv(fused=True, fused_x16=True)``: the fused attention on
                                                                   # bf16 (or fp16) q, k, v: no [nnz, H] array AND half the node bytes

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
from gat_custom import gat_graph  # noqa: E402
from gcn_custom import load_edges  # noqa: E402,F401
from gespmm_amd import TransformerConv  # noqa: E402


class Net(torch.nn.Module):
    def __init__(self, n_in, n_out, n_hidden=8, heads=8, dropout=0.6, fused=False, attn_dropout=0.0, beta=False):
        super().__init__()
        # (fused_x16: a 16-bit model runs the fused attention on 16-bit q, k and v; an fp32 one runs what fused=True runs)
        kw = dict(fused=fused, fused_x16=fused, dropout=attn_dropout, beta=beta)
        self.conv1 = TransformerConv(n_in, n_hidden, heads=heads, concat=True, **kw)
        self.conv2 = TransformerConv(n_hidden * heads, n_out, heads=1, concat=False, **kw)
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
                    help="TransformerConv(dropout=P) in both layers: dropout on the attention coefficients")
    ap.add_argument("--graph-capture", action="store_true", help="capture one training step in a HIP graph")
    ap.add_argument("--fused", action="store_true",
                    help="TransformerConv(fused=True): the attention in one kernel, its backward in two, no [nnz, H] array")
    ap.add_argument("--beta", action="store_true", help="TransformerConv(beta=True): the gated skip connection")
    ap.add_argument("--seed", type=int, default=None,
                    help="torch.manual_seed before the model is made (parameters and dropout masks)")
    ap.add_argument("--dtype", choices=("fp32", "bf16", "fp16"), default="fp32",
                    help="cast the model and the features (bf16 / fp16: TransformerConv on the 16-bit SDDMM and multi-head product, with "
                         "--fused the fused attention on 16-bit q, k and v)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device (the ops have no CPU path)")
    device = torch.device("cuda")

    edge_index, n_v, n_feat, n_cls = load_edges(args.dataset, device)
    g = gat_graph(edge_index, n_v, device, int32_order=True)
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
    model = Net(n_feat, n_cls, args.n_hidden, args.heads, args.dropout, fused=args.fused, attn_dropout=args.attn_dropout,
                beta=args.beta).to(device)
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
    print("dataset=%s n=%d nnz(+I)=%d heads=%d hidden=%d graph_capture=%s fused=%s beta=%s%s" %
          (args.dataset, n_v, g["colind"].numel(), args.heads, args.n_hidden, args.graph_capture, args.fused, args.beta,
           (" attn_dropout=%g" % args.attn_dropout if args.attn_dropout else "") + (" dtype=%s" % args.dtype if args.dtype != "fp32" else "")))
    print("epochs=%d  gpu %.3f ms/epoch  wall %.3f ms/epoch" %
          (args.epochs, e0.elapsed_time(e1) / args.epochs, wall * 1e3 / args.epochs))


if __name__ == "__main__":
    main()
