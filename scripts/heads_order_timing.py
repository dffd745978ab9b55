"""Timing of the backward step of the multi-head attention layers — the multi-head product on the CSC arrays with its [nnz, H] weights in
CSR edge order — three ways IN THE SAME RUN, of ``graphs.take_edges`` alone against a plain copy, and of one training step of
examples/gat_custom.py's model with the backward of this commit and with the parent's.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures; every column is
measured three times per run, the columns of a case taking turns (round 1 of every column, then round 2, ...), so that a drift of the
machine lands on all of them.

Columns, per graph, (H, F) and dtype of the features (fp32, bf16) — all three give the same bits, checked before anything is timed:
  (a) the parent's backward step: the chunked ``index_select`` gather of the weights (``parent_take_edges`` below, a copy of the code
      this commit replaced) + the product
  (b) the HIP gather + the product: ``csr_spmm_heads(..., order=)`` under GESPMM_HEADS_ORDER_ROUTE=composition (read per call)
  (c) the ordered kernel: ``csr_spmm_heads(..., order=)``
  take     ``graphs.take_edges`` (the HIP gather) and ``parent_take_edges`` on [nnz, 1 / 2 / 4 / 8] fp32 and [nnz, 8] bf16 against
           ``out.copy_(x)`` of the same array; with --big also [2^26 + 1024, 4] fp32
  step     examples/gat_custom.py's two-layer model (8 heads x 8, then 1 head), one training step: median time over --steps steps and the
           peak of torch's allocator over them, fp32 and bf16, with this commit's backward and with the parent's (``order=`` switched
           off and ``take_edges`` replaced by ``parent_take_edges`` for that measurement: the parent's code path, not a checkout of it)
Each run appends a `#run` line per case; from the third run of the script on, the spread of a reference column's medians ACROSS the runs
is the margin: (c) is judged against (a) with (a)'s spread and against (b) with (b)'s, (b) against (a) with (a)'s.

  python scripts/heads_order_timing.py [--graphs a,b] [--launches 200] [--steps 60] [--step-datasets a,b] [--int32-order] [--big]
                                       [--out profiles/r19/heads_order/timing.log]      (--graphs , : the training step alone)
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from gespmm_amd import _lib, graphs, op, spmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed")  # (products-sbm where memory and time allow: --graphs com-amazon-sbm,pubmed,products-sbm)
SHAPES = ((4, 16), (8, 8), (8, 32), (8, 64))
COLUMNS = ("parent", "gather", "ordered")
PIN = ("GESPMM_HEADS_ORDER_ROUTE", "composition")


def parent_take_edges(x, order, chunk_rows=1 << 24):
    """What graphs.take_edges did before it had a HIP gather: index_select in pieces of at most 2^24 index rows into one result."""
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    for a in range(0, order.numel(), chunk_rows):
        torch.index_select(x, 0, order[a:a + chunk_rows], out=out[a:a + chunk_rows])
    return out


def median_us(fn, launches, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def load_csc(name, dev):
    """The CSC arrays of the graph and the int32 CSC-position -> CSR-position order: what a backward runs on."""
    if name == "pubmed":
        g = graphs.load_mtx_as_csr(os.path.join(ROOT, "tests", "golden", "pubmed.mtx"))
        rp, ci, M, K = torch.from_numpy(g["rowptr"]).to(dev), torch.from_numpy(g["colind"]).to(dev), g["M"], g["K"]
    else:
        g = graphs.synthetic_graph(name, seed=42, device=dev)
        rp, ci, M, K = g["rowptr"], g["colind"], g["M"], g["K"]
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    return colptr, rowind, order.to(torch.int32).contiguous(), order, K, M  # (the CSC product is K x M)


class pinned:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ[PIN[0]] = PIN[1]

    def __exit__(self, *exc):
        os.environ.pop(PIN[0], None)


def take_turns(fns, columns, launches, pins=()):
    res = {c: [] for c in columns}
    for _ in range(3):
        for c in columns:
            with pinned(c in pins):
                res[c].append(median_us(fns[c], launches))
    return res


def measure(colptr, rowind, order, order64, rows, cols, H, F, dtype, launches):
    dev = colptr.device
    nnz = rowind.numel()
    gen = torch.Generator(device=dev).manual_seed(1)
    val = torch.rand(nnz, H, device=dev, generator=gen) - 0.5
    D = (torch.rand(cols, H, F, device=dev, generator=gen) - 0.5).to(dtype)
    out = torch.empty(rows, H, F, device=dev, dtype=dtype)
    heads = spmm.csr_spmm_heads if dtype == torch.float32 else spmm.csr_spmm_heads_x16
    route = (_lib.heads_route if dtype == torch.float32 else _lib.heads_x16_route)(rows, cols, H, F, nnz)
    fns = {
        "parent": lambda: heads(colptr, rowind, parent_take_edges(val, order64), D, out=out),
        "gather": lambda: heads(colptr, rowind, val, D, out=out, order=order),
        "ordered": lambda: heads(colptr, rowind, val, D, out=out, order=order),
    }
    os.environ.pop(PIN[0], None)
    raw = torch.int32 if dtype == torch.float32 else torch.int16
    a = fns["parent"]().clone().view(raw)
    c = fns["ordered"]().clone().view(raw)
    with pinned(True):
        b = fns["gather"]().clone().view(raw)
    res = {"route": route, "bits_equal": torch.equal(a, b) and torch.equal(a, c)}
    res.update(take_turns(fns, COLUMNS, launches, pins=("gather",)))
    del val, D, out
    torch.cuda.empty_cache()
    return res


def measure_take(n, tail, dtype, order, order64, launches):
    dev = order.device
    gen = torch.Generator(device=dev).manual_seed(2)
    x = (torch.rand((n,) + tail, device=dev, generator=gen) - 0.5).to(dtype)
    out = torch.empty_like(x)
    fns = {"copy": lambda: out.copy_(x), "hip": lambda: graphs.take_edges(x, order), "hip64": lambda: graphs.take_edges(x, order64),
           "parent": lambda: parent_take_edges(x, order64)}
    ok = torch.equal(fns["hip"]().view(torch.int16), fns["parent"]().view(torch.int16)) and \
        torch.equal(fns["hip64"]().view(torch.int16), fns["parent"]().view(torch.int16))
    res = take_turns(fns, ("copy", "hip", "hip64", "parent"), launches)
    res["bits_equal"] = ok
    del x, out
    torch.cuda.empty_cache()
    return res


def training_step(name, dtype, parent, steps, int32_order=False):
    """(median ms of one training step, peak MiB of torch's allocator over the timed steps, last loss) of examples/gat_custom.py's model;
    parent: the backward takes the parent's path (no order=, the chunked index_select)."""
    import torch.nn.functional as F

    from gat_custom import Net, gat_graph
    from gcn_custom import load_edges

    saved = (op._csc_heads_order, graphs.take_edges)
    if parent:
        op._csc_heads_order = lambda *a, **k: None
        graphs.take_edges = parent_take_edges
    try:
        dev = torch.device("cuda")
        edge_index, n_v, n_feat, n_cls = load_edges(name, dev)
        g = gat_graph(edge_index, n_v, dev, int32_order=int32_order)
        gen = torch.Generator().manual_seed(0)
        x = torch.rand(n_v, n_feat, generator=gen)
        x = (x / x.sum(1, keepdim=True)).to(dev)
        y = torch.randint(0, n_cls, (n_v,), generator=gen).to(dev)
        train_idx = torch.randperm(n_v, generator=gen)[:20 * n_cls].to(dev)
        torch.manual_seed(0)
        model = Net(n_feat, n_cls, 8, 8, 0.6, fused_score=False).to(dev)
        if dtype != torch.float32:
            model, x = model.to(dtype), x.to(dtype)
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)
        y_train = y[train_idx]
        model.train()

        def step():
            opt.zero_grad(set_to_none=False)
            loss = F.nll_loss(model(x, g).index_select(0, train_idx), y_train)
            loss.backward()
            opt.step()
            return loss

        for _ in range(5):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for a, b in ev:
            a.record()
            loss = step()
            b.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)), "the loss is not finite"
        peak = torch.cuda.max_memory_allocated() / 2.0 ** 20
        del model, opt, g, x
        torch.cuda.empty_cache()
        return statistics.median(a.elapsed_time(b) for a, b in ev), peak, float(loss)
    finally:
        op._csc_heads_order, graphs.take_edges = saved


def earlier_runs(path):
    """{key: {column: [median of each earlier run]}} from the `#run` lines of the log."""
    runs = {}
    if os.path.exists(path):
        for line in open(path):
            if line.startswith("#run "):
                _, key, *cols = line.split()
                d = runs.setdefault(key, {})
                for kv in cols:
                    k, v = kv.split("=")
                    d.setdefault(k, []).append(float(v))
    return runs


def verdict(mine, base):
    """mine against base over >= 3 runs: the spread of base's medians across the runs is the margin."""
    margin = max(base) - min(base)
    return margin, "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=60, help="timed training steps per setting (0: skip the training step)")
    ap.add_argument("--step-datasets", default="pubmed", help="datasets of examples/gcn_custom.py's load_edges for the training step")
    ap.add_argument("--int32-order", action="store_true", help="the training step hands the layers an int32 csc_order (no conversion per forward)")
    ap.add_argument("--big", action="store_true", help="take_edges at [2^26 + 1024, 4] fp32 too (3 GiB of device memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "heads_order", "timing.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device (nothing here is a measurement without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    med = statistics.median
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        def judge(key, m, pairs):
            log("#run %s %s" % (key, " ".join("%s=%.1f" % (k, med(v)) for k, v in m.items() if isinstance(v, list))))
            r = before.get(key, {})
            for mine_k, base_k in pairs:
                base = r.get(base_k, []) + [med(m[base_k])]
                mine = r.get(mine_k, []) + [med(m[mine_k])]
                if len(base) >= 3:
                    margin, v = verdict(mine, base)
                    log("   over %d runs: %s %s, margin = spread %.1f; %s %s: %s beyond the margin" % (
                        len(base), base_k, " ".join("%.1f" % x for x in base), margin, mine_k, " ".join("%.1f" % x for x in mine), v))

        log("# %s launches=%d device=%s (us; three medians each, columns taking turns)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, torch.cuda.get_device_name(0)))
        fmt = lambda v: "%s (median %.1f)" % (" ".join("%.1f" % x for x in v), med(v))  # noqa: E731
        for name in [n for n in args.graphs.split(",") if n]:
            colptr, rowind, order, order64, rows, cols = load_csc(name, dev)
            nnz = rowind.numel()
            for H, F in SHAPES:
                for dtype in (torch.float32, torch.bfloat16):
                    dn = str(dtype).replace("torch.", "")
                    m = measure(colptr, rowind, order, order64, rows, cols, H, F, dtype, args.launches)
                    a = med(m["parent"])
                    log("%-15s H=%d F=%d %s rows=%d nnz=%d route=%d V,S,W,rpw=%s bits_equal=%s" % (
                        name, H, F, dn, rows, nnz, m["route"][0], m["route"][1], m["bits_equal"]))
                    log("   (a) index_select + product   %s" % fmt(m["parent"]))
                    log("   (b) HIP gather + product     %s   x%.2f of (a)" % (fmt(m["gather"]), a / med(m["gather"])))
                    log("   (c) ordered kernel           %s   x%.2f of (a)  x%.2f of (b)" % (
                        fmt(m["ordered"]), a / med(m["ordered"]), med(m["gather"]) / med(m["ordered"])))
                    judge("%s/H%d/F%d/%s" % (name, H, F, dn), m, (("ordered", "parent"), ("ordered", "gather"), ("gather", "parent")))
            takes = [(nnz, (h,), torch.float32) for h in (1, 2, 4, 8)] + [(nnz, (8,), torch.bfloat16)]
            for n, tail, dtype in takes:
                m = measure_take(n, tail, dtype, order, order64, args.launches)
                dn = str(dtype).replace("torch.", "")
                log("%-15s take_edges [%d, %d] %s bits_equal=%s: copy %s | HIP gather, int32 order %s | int64 order %s | index_select %s" % (
                    name, n, tail[0], dn, m["bits_equal"], fmt(m["copy"]), fmt(m["hip"]), fmt(m["hip64"]), fmt(m["parent"])))
                judge("%s/take/%d/%s" % (name, tail[0], dn), m, (("hip", "parent"), ("hip64", "parent"), ("hip", "copy")))
            del colptr, rowind, order, order64
            torch.cuda.empty_cache()
        if args.big:
            n = (1 << 26) + 1024
            order64 = torch.randperm(n, device=dev)
            m = measure_take(n, (4,), torch.float32, order64.to(torch.int32), order64, max(args.launches // 4, 20))
            log("%-15s take_edges [%d, 4] float32 bits_equal=%s: copy %s | HIP gather, int32 order %s | int64 order %s | index_select %s" % (
                "randperm", n, m["bits_equal"], fmt(m["copy"]), fmt(m["hip"]), fmt(m["hip64"]), fmt(m["parent"])))
            judge("randperm/take/4/float32", m, (("hip", "parent"), ("hip64", "parent"), ("hip", "copy")))
            del order64
            torch.cuda.empty_cache()
        if args.steps > 0:
            for name in [n for n in args.step_datasets.split(",") if n]:
                rows_ = []
                for _ in range(2):  # the settings take turns, twice
                    for dtype in (torch.float32, torch.bfloat16):
                        for parent in (True, False):
                            rows_.append((dtype, parent) + training_step(name, dtype, parent, args.steps, args.int32_order))
                for dtype, parent, ms, peak, loss in rows_:
                    log("step %-8s dtype=%-8s csc_order=%s backward=%-6s %.3f ms/step  peak %.1f MiB  last loss %.4f" % (
                        name, str(dtype).replace("torch.", ""), "int32" if args.int32_order else "int64", "parent" if parent else "order=", ms,
                        peak, loss))


if __name__ == "__main__":
    main()
