#!/usr/bin/env python3
"""GraphSAGE training on the custom op — the model and training loop of the reference's dgl-custom/benchmark/sage/sage_dgl.py on
``gespmm_amd.SAGEConv`` (aggregators mean / gcn / pool; no DGL).

    python examples/sage_custom.py --dataset cora --aggregator-type pool
    python examples/sage_custom.py --dataset pubmed --aggregator-type mean --n-hidden 64
    python examples/sage_custom.py --aggregator-type pool --graph-capture      # replay each step from a HIP graph
    python examples/sage_custom.py --aggregator-type pool --dtype bf16         # a .bfloat16() model on 16-bit features

The command-line options are the reference script's (sage_dgl.py:182-201; ``--dataset`` is what ``register_data_args`` adds), plus
``--graph-capture``, ``--seed`` and ``--dtype`` (fp16 / bf16: model and features in that type, the loss in fp32). Differences forced by the environment are those of examples/gcn_custom.py, whose data path this
script uses: the bundled adjacency matrices or the synthetic stand-ins, random features, labels and masks — accuracy is chance level by
construction, the point is the step time and that the loss falls. As in the reference, self loops are removed (sage_dgl.py:101) and the
profiler table is replaced by HIP-event timing of the epoch loop.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gespmm_amd  # noqa: E402,F401
from gcn_custom import load_edges, proc  # noqa: E402
from gespmm_amd import SAGEConv, graphs  # noqa: E402


class GraphSAGE(torch.nn.Module):
    """sage_dgl.py:21-48: an input layer, n_layers - 1 hidden layers, an output layer without activation."""

    def __init__(self, g, in_feats, n_hidden, n_classes, n_layers, activation, dropout, aggregator_type):
        super().__init__()
        self.g = g
        dims = [in_feats] + [n_hidden] * n_layers + [n_classes]
        self.layers = torch.nn.ModuleList(
            [SAGEConv(dims[i], dims[i + 1], aggregator_type, feat_drop=dropout, activation=activation if i + 2 < len(dims) else None)
             for i in range(len(dims) - 1)])

    def forward(self, features):
        h = features
        for layer in self.layers:
            h = layer(h, *self.g)
        return h


def build_graph(edge_index, n_v, device):
    """Destination-major CSR (a row aggregates over its in-neighbours), its CSC arrays and the CSC -> CSR entry order, without self
    loops and without repeated edges."""
    keep = edge_index[0] != edge_index[1]
    g = proc(edge_index[:, keep], n_v, device, add_self_loop=False)
    rowptr, colind = g["rowptr"], g["colind"]
    colptr, rowind, order = graphs.transpose_csr(rowptr, colind, K=n_v, return_order=True)
    return rowptr, colind, colptr, rowind, order.to(torch.int32)


def main():
    ap = argparse.ArgumentParser(description="GraphSAGE")
    ap.add_argument("--dataset", default="cora")
    ap.add_argument("--dropout", type=float, default=0.5, help="dropout probability")
    ap.add_argument("--gpu", type=int, default=0, help="gpu")
    ap.add_argument("--lr", type=float, default=1e-2, help="learning rate")
    ap.add_argument("--n-epochs", type=int, default=200, help="number of training epochs")
    ap.add_argument("--n-hidden", type=int, default=16, help="number of hidden units")
    ap.add_argument("--n-layers", type=int, default=1, help="number of hidden layers")
    ap.add_argument("--weight-decay", type=float, default=5e-4, help="Weight for L2 loss")
    ap.add_argument("--aggregator-type", type=str, default="gcn", help="Aggregator type: mean/gcn/pool")
    ap.add_argument("--graph-capture", action="store_true", help="capture one training step in a HIP graph")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", choices=("fp32", "fp16", "bf16"), default="fp32", help="type of the model and the features (the loss stays fp32)")
    args = ap.parse_args()
    print(args)
    if args.gpu < 0 or not torch.cuda.is_available():
        raise SystemExit("needs a HIP device (the op has no CPU path)")
    torch.cuda.set_device(args.gpu)
    device = torch.device("cuda", args.gpu)
    torch.manual_seed(args.seed)

    edge_index, n_v, n_feat, n_cls = load_edges(args.dataset, device)
    g = build_graph(edge_index, n_v, device)
    n_edges = g[1].numel()
    gen = torch.Generator().manual_seed(args.seed)
    features = torch.rand(n_v, n_feat, generator=gen)
    features = (features / features.sum(1, keepdim=True)).to(device)
    labels = torch.randint(0, n_cls, (n_v,), generator=gen).to(device)
    perm = torch.randperm(n_v, generator=gen)
    idx = {name: perm[a:b].to(device) for name, (a, b) in (("train", (0, 20 * n_cls)), ("val", (20 * n_cls, 20 * n_cls + 500)),
                                                            ("test", (20 * n_cls + 500, 20 * n_cls + 1500)))}
    print("----Data statistics------\n  #Edges %d\n  #Classes %d\n  #Train samples %d\n  #Val samples %d\n  #Test samples %d"
          % (n_edges, n_cls, idx["train"].numel(), idx["val"].numel(), idx["test"].numel()))

    model = GraphSAGE(g, n_feat, args.n_hidden, n_cls, args.n_layers, F.relu, args.dropout, args.aggregator_type).to(device)
    if args.dtype != "fp32":
        dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
        model, features = model.to(dtype), features.to(dtype)
    loss_fcn = torch.nn.CrossEntropyLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, capturable=args.graph_capture)
    y_train = labels[idx["train"]]

    def train_step():
        optimizer.zero_grad(set_to_none=False)
        logits = model(features)
        loss = loss_fcn(logits.index_select(0, idx["train"]).float(), y_train)
        loss.backward()
        optimizer.step()
        return loss

    @torch.no_grad()
    def evaluate(which):
        model.eval()
        pred = model(features).index_select(0, idx[which]).max(1)[1]
        model.train()
        return pred.eq(labels[idx[which]]).sum().item() / idx[which].numel()

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

    dur = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for epoch in range(args.n_epochs):
        if epoch == 3:
            torch.cuda.synchronize()
            e0.record()
        t0 = time.time()
        if graph is not None:
            graph.replay()
            loss = static_loss
        else:
            loss = train_step()
        loss_value = float(loss)  # (synchronises: the reference reads loss.item() only at the end; the event time below excludes nothing)
        if epoch >= 3:
            dur.append(time.time() - t0)
        print("Epoch {:05d} | Loss {:.4f}".format(epoch, loss_value))
    e1.record()
    torch.cuda.synchronize()
    if dur:
        mean = sum(dur) / len(dur)
        print("Epoch {:05d} | Total Time(s) {:.4f} | Loss {:.4f} | Accuracy {:.4f} | ETputs(KTEPS) {:.2f}".format(
            args.n_epochs - 1, mean, loss_value, evaluate("val"), n_edges / mean / 1000))
        print("gpu %.3f ms/epoch over %d epochs (aggregator=%s, graph_capture=%s)"
              % (e0.elapsed_time(e1) / len(dur), len(dur), args.aggregator_type, args.graph_capture))
    print()
    print("Test Accuracy {:.4f}".format(evaluate("test")))


if __name__ == "__main__":
    main()
