#!/usr/bin/env python3
"""Entity classification with a two-layer relational graph convolution (Schlichtkrull et al., 2018) on ``gespmm_amd.RGCNConv``.

    python examples/rgcn_custom.py --dataset pubmed --num-rels 4
    python examples/rgcn_custom.py --dataset cora --num-rels 16 --num-bases 4 --dtype bf16    # each layer ONE relational kernel
    python examples/rgcn_custom.py --dtype bf16 --graph-capture                               # replay each step from a HIP graph
    python examples/rgcn_custom.py --dtype bf16 --fused-weight-grad                           # the weights' gradient without the [R M, K] aggregates

The data path is examples/gcn_custom.py's (the bundled adjacency matrices or the synthetic stand-ins, random features). Every edge
gets one of ``--num-rels`` types by a seeded rule (``--skew``: half of the relations share 5 % of the edges). The labels are those of
a fixed, randomly initialised one-layer fp32 RGCN on the same typed graph (seed 12345), so a model that uses the edge types can learn
them and the test accuracy means something; ``--dtype`` sets the type of the model and the features (the loss stays fp32) and
``--composition`` keeps the 16-bit layers off the kernel (``RGCNConv(fused=False)``).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gespmm_amd  # noqa: E402,F401
from gcn_custom import load_edges  # noqa: E402
from gespmm_amd import RGCNConv, graphs  # noqa: E402


def edge_types(n_edges, num_rels, skew, seed, device):
    """One relation per edge, seeded: uniform, or skewed so that the upper half of the relations holds 5 % of the edges."""
    gen = torch.Generator().manual_seed(seed)
    if not skew or num_rels < 2:
        return torch.randint(0, num_rels, (n_edges,), generator=gen).to(device)
    half = num_rels // 2
    p = torch.cat([torch.full((num_rels - half,), 0.95 / (num_rels - half)), torch.full((half,), 0.05 / half)])
    return torch.multinomial(p, n_edges, replacement=True, generator=gen).to(device)


def stacked_graph(row, col, etype, num_rels, n_v):
    """Stacked CSR (relation r's row i is row r * n_v + i; a row aggregates over its in-neighbours) and stacked CSC, on the device."""
    key = etype.to(torch.int64) * n_v + row.to(torch.int64)
    order = torch.argsort(key, stable=True)
    rowptr = torch.zeros(num_rels * n_v + 1, dtype=torch.int64, device=row.device)
    rowptr[1:] = torch.cumsum(torch.bincount(key, minlength=num_rels * n_v), 0)
    rowptr, colind = rowptr.to(torch.int32), col[order].to(torch.int32).contiguous()
    return (rowptr, colind) + tuple(graphs.transpose_stacked_csr(rowptr, colind, num_rels, n_v))


class RGCN(torch.nn.Module):
    def __init__(self, g, in_feats, n_hidden, n_classes, num_rels, num_bases, fused=True, fused_weight_grad=False):
        super().__init__()
        self.g = g
        self.conv1 = RGCNConv(in_feats, n_hidden, num_rels, num_bases=num_bases, activation=F.relu, fused=fused, fused_weight_grad=fused_weight_grad)
        self.conv2 = RGCNConv(n_hidden, n_classes, num_rels, num_bases=num_bases, fused=fused, fused_weight_grad=fused_weight_grad)

    def forward(self, features):
        return self.conv2(self.conv1(features, *self.g), *self.g)


def main():
    ap = argparse.ArgumentParser(description="RGCN")
    ap.add_argument("--dataset", default="pubmed")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--n-epochs", type=int, default=100)
    ap.add_argument("--n-hidden", type=int, default=64)
    ap.add_argument("--weight-decay", type=float, default=5e-4)
    ap.add_argument("--num-rels", type=int, default=4)
    ap.add_argument("--num-bases", type=int, default=None)
    ap.add_argument("--skew", action="store_true", help="half of the relations hold 5 %% of the edges")
    ap.add_argument("--dtype", choices=("fp32", "fp16", "bf16"), default="fp32")
    ap.add_argument("--composition", action="store_true", help="16-bit layers compose the product and the matmul instead of the kernel")
    ap.add_argument("--fused-weight-grad", action="store_true", help="16-bit layers take the weights' gradient from the fused kernel")
    ap.add_argument("--graph-capture", action="store_true", help="capture one training step in a HIP graph")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    print(args)
    if args.gpu < 0 or not torch.cuda.is_available():
        raise SystemExit("needs a HIP device (the op has no CPU path)")
    torch.cuda.set_device(args.gpu)
    device = torch.device("cuda", args.gpu)

    edge_index, n_v, n_feat, n_cls = load_edges(args.dataset, device)
    edge_index = torch.as_tensor(edge_index).to(device).long()
    n_feat = (min(n_feat, 256) + 7) // 8 * 8  # (random features anyway: a width the kernel serves)
    keep = edge_index[0] != edge_index[1]
    src, dst = edge_index[0][keep], edge_index[1][keep]
    etype = edge_types(src.numel(), args.num_rels, args.skew, 4242, device)
    g = stacked_graph(dst, src, etype, args.num_rels, n_v)
    gen = torch.Generator().manual_seed(4242)
    features = (torch.rand(n_v, n_feat, generator=gen) - 0.5).to(device)
    torch.manual_seed(12345)
    with torch.no_grad():
        teacher = RGCNConv(n_feat, n_cls, args.num_rels, bias=False).to(device)
        labels = teacher(features, *g).max(1)[1]
    torch.manual_seed(args.seed)
    perm = torch.randperm(n_v, generator=torch.Generator().manual_seed(args.seed))
    n_train = n_v // 2
    idx = {"train": perm[:n_train].to(device), "test": perm[n_train:n_train + 1000].to(device)}
    print("nodes %d  edges %d  relations %d (entries per stacked row %.2f)  classes %d  train %d  test %d"
          % (n_v, g[1].numel(), args.num_rels, g[1].numel() / (args.num_rels * n_v), n_cls, n_train, idx["test"].numel()))

    model = RGCN(g, n_feat, args.n_hidden, n_cls, args.num_rels, args.num_bases, fused=not args.composition,
                 fused_weight_grad=args.fused_weight_grad).to(device)
    if args.dtype != "fp32":
        dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
        model, features = model.to(dtype), features.to(dtype)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, capturable=args.graph_capture)
    y_train = labels[idx["train"]]

    def train_step():
        optimizer.zero_grad(set_to_none=False)
        loss = F.cross_entropy(model(features).index_select(0, idx["train"]).float(), y_train)
        loss.backward()
        optimizer.step()
        return loss

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

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for epoch in range(args.n_epochs):
        if epoch == 3:
            e0.record()
        if graph is not None:
            graph.replay()
            loss = static_loss
        else:
            loss = train_step()
        if epoch % 10 == 0 or epoch == args.n_epochs - 1:
            print("Epoch {:05d} | Loss {:.4f}".format(epoch, float(loss)))
    e1.record()
    torch.cuda.synchronize()
    if args.n_epochs > 3:
        print("gpu %.3f ms/epoch over %d epochs (dtype=%s, composition=%s, fused_weight_grad=%s, graph_capture=%s)"
              % (e0.elapsed_time(e1) / (args.n_epochs - 3), args.n_epochs - 3, args.dtype, args.composition, args.fused_weight_grad, args.graph_capture))
    with torch.no_grad():
        pred = model(features).index_select(0, idx["test"]).max(1)[1]
    print("Test Accuracy {:.4f} (seed {}, {})".format(pred.eq(labels[idx["test"]]).float().mean().item(), args.seed, args.dtype))


if __name__ == "__main__":
    main()
