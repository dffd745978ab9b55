"""Timing of the fused GAT aggregation on 16-bit features (gespmm_gat_aggregate_x16) against its fp32 form and against the 16-bit
composition GATConv runs without it, IN THE SAME RUN, and a two-layer training step with its peak memory.

One process per run. A kernel figure is the median of `--launches` per-launch event pairs after a warm-up; every column is measured
`--rounds` times, the columns alternating inside a round, and the row reports the median of its rounds with their spread (max - min):
a difference smaller than the two spreads together is "not different".

Kernels, per graph and (H, F), bf16, slope 0.2, everything into preallocated results, the statistics ready (all three columns need them
or their equal):
  forward     (x16)  spmm.gat_aggregate_x16                                          one launch, no [nnz, H] array
              (a)    spmm.gat_aggregate on the fp32 features                         the fp32 form: twice the node bytes
              (b)    softmax.gat_edge_softmax + spmm.csr_spmm_heads_x16              the 16-bit composition: alpha written and read back
  transposed  (x16)  spmm.gat_aggregate_x16(colptr, rowind, .., transposed=True)
              (a)    spmm.gat_aggregate(.., transposed=True)
              (b)    spmm.csr_spmm_heads_x16(colptr, rowind, alpha, grad_out, order=csc_order)   (alpha ready: the forward saved it)
(x16) is checked against narrow((a)) bit for bit before anything is timed.

Step: examples/gat_custom.py's Net (64 inputs -> 8 heads x 8 -> 16 classes, dropout off), forward + backward, median of `--steps` event
pairs, and the peak allocated above the graph and the features, for bf16 fused_aggregate / fused_backward (fused_x16), their fp32 forms
and the bf16 fused_score layer.

  python scripts/gat_aggregate_x16_timing.py [--graphs com-amazon-sbm,pubmed] [--cases 1x64,4x16,8x8,8x32] [--step-graphs ..,products-sbm]
"""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from edge_softmax_timing import median_us  # noqa: E402
from gat_softmax_timing import SLOPE, load_graph  # noqa: E402
from gespmm_amd import _lib, graphs, softmax, spmm  # noqa: E402

DT = torch.bfloat16


def rounds_of(columns, rounds, launches):
    """{name: [median of each round]} with the columns alternating inside a round."""
    got = {k: [] for k, _ in columns}
    for _ in range(rounds):
        for k, fn in columns:
            got[k].append(median_us(fn, launches))
    return got


def fmt(v):
    return "%.1f (spread %.1f)" % (statistics.median(v), max(v) - min(v))


def verdict(mine, base):
    m, b = statistics.median(mine), statistics.median(base)
    margin = (max(mine) - min(mine)) + (max(base) - min(base))
    return "FASTER x%.2f" % (b / m) if m < b - margin else ("SLOWER x%.2f" % (m / b) if m > b + margin else "not different")


def kernels(rp, ci, csc, K, H, F, rounds, launches, log, name):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    el = (torch.rand(M, H, device=dev, generator=gen) - 0.5) * 4
    er = (torch.rand(K, H, device=dev, generator=gen) - 0.5) * 4
    feat = (torch.rand(K, H, F, device=dev, generator=gen) - 0.5).to(DT)
    gout = (torch.rand(M, H, F, device=dev, generator=gen) - 0.5).to(DT)
    feat32, gout32 = feat.float(), gout.float()
    stats = softmax.gat_softmax_stats(rp, ci, el, er, negative_slope=SLOPE)
    alpha = torch.empty(nnz, H, device=dev)
    out16, out32, outb = torch.empty(M, H, F, device=dev, dtype=DT), torch.empty(M, H, F, device=dev), torch.empty(M, H, F, device=dev, dtype=DT)
    gf16, gf32, gfb = torch.empty(K, H, F, device=dev, dtype=DT), torch.empty(K, H, F, device=dev), torch.empty(K, H, F, device=dev, dtype=DT)

    def fwd_b():
        softmax.gat_edge_softmax(rp, ci, el, er, negative_slope=SLOPE, out=alpha)
        spmm.csr_spmm_heads_x16(rp, ci, alpha, feat, out=outb)

    fwd = (("x16", lambda: spmm.gat_aggregate_x16(rp, ci, el, er, stats, feat, negative_slope=SLOPE, out=out16)),
           ("fp32", lambda: spmm.gat_aggregate(rp, ci, el, er, stats, feat32, negative_slope=SLOPE, out=out32)),
           ("composition", fwd_b))
    bwd = (("x16", lambda: spmm.gat_aggregate_x16(colptr, rowind, el, er, stats, gout, negative_slope=SLOPE, transposed=True, out=gf16)),
           ("fp32", lambda: spmm.gat_aggregate(colptr, rowind, el, er, stats, gout32, negative_slope=SLOPE, transposed=True, out=gf32)),
           ("composition", lambda: spmm.csr_spmm_heads_x16(colptr, rowind, alpha, gout, out=gfb, order=order)))
    for _, fn in fwd + bwd:
        fn()
    same = lambda x, y: bool((x.view(torch.int16) == y.view(torch.int16)).all())  # noqa: E731
    if not (same(out16, out32.to(DT)) and same(gf16, gf32.to(DT))):
        raise SystemExit("%s H=%d F=%d: the 16-bit result is not narrow(fp32 result): nothing timed is worth recording" % (name, H, F))
    log("%-15s H=%d F=%d M=%d nnz=%d route fwd %s transposed %s (fp32: %s) same bits as narrow(fp32)=True composition same bits fwd=%s T=%s" % (
        name, H, F, M, nnz, _lib.gat_aggregate_x16_route(M, K, H, F, nnz), _lib.gat_aggregate_x16_route(M, K, H, F, nnz, True),
        _lib.gat_aggregate_route(M, K, H, F, nnz), same(out16, outb), same(gf16, gfb)))
    for direction, columns in (("fwd", fwd), ("T", bwd)):
        r = rounds_of(columns, rounds, launches)
        log("   %-3s  x16 %s   fp32 %s   composition %s   -> against fp32: %s, against the composition: %s" % (
            direction, fmt(r["x16"]), fmt(r["fp32"]), fmt(r["composition"]), verdict(r["x16"], r["fp32"]), verdict(r["x16"], r["composition"])))
        log("#run %s %dx%d %s %s" % (name, H, F, direction, " ".join("%s=%s" % (k, ",".join("%.1f" % x for x in v)) for k, v in r.items())))


def steps(name, dev, n_steps, rounds, log):
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x32 = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    variants = (("bf16 fused_aggregate", DT, {"fused_aggregate": True}), ("bf16 fused_backward", DT, {"fused_backward": True}),
                ("fp32 fused_aggregate", None, {"fused_aggregate": True}), ("fp32 fused_backward", None, {"fused_backward": True}),
                ("bf16 fused_score", DT, {"fused_score": True}))
    models = {}
    for key, dt, kw in variants:
        torch.manual_seed(0)
        m = ex.Net(64, 16, 8, 8, dropout=0.0, **kw).to(dev)
        models[key] = (m.to(dt) if dt else m, x32.to(dt) if dt else x32)

    def step(key):
        m, x = models[key]
        loss = torch.nn.functional.nll_loss(m(x, g).float(), y)
        loss.backward()
        m.zero_grad(set_to_none=True)
        return loss

    peak, times = {}, {k: [] for k in models}
    for key in models:
        for _ in range(2):  # the second step is the one measured (pools and code objects exist)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            loss = step(key)
            torch.cuda.synchronize()
            peak[key] = (torch.cuda.max_memory_allocated() - base, float(loss.detach()))
            del loss
    for _ in range(rounds):
        for key in models:
            times[key].append(median_us(lambda: step(key), n_steps, warmup=2))
    log("#step %s nodes=%d nnz=%d (self-loops not added) two-layer GAT 64 -> 8 x 8 -> 16, forward + backward, us per step (median of %d, %d "
        "rounds) and peak allocated above the graph, the features and the parameters" % (name, K, ci.numel(), n_steps, rounds))
    for key in models:
        log("   %-22s step %s   peak %.1f MB   loss %.6f" % (key, fmt(times[key]), peak[key][0] / 2 ** 20, peak[key][1]))
    for mine, base in (("bf16 fused_aggregate", "fp32 fused_aggregate"), ("bf16 fused_backward", "fp32 fused_backward"),
                       ("bf16 fused_aggregate", "bf16 fused_score"), ("bf16 fused_backward", "bf16 fused_score")):
        log("   %s against %s: %s" % (mine, base, verdict(times[mine], times[base])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="com-amazon-sbm,pubmed")
    ap.add_argument("--cases", default="1x64,4x16,8x8,8x32")
    ap.add_argument("--step-graphs", default="com-amazon-sbm,pubmed,products-sbm")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "gat_aggregate_x16", "timing.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this script measures on the GPU: no HIP device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d rounds=%d steps=%d slope=%s dtype=bf16 device=%s (us)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, args.rounds, args.steps, SLOPE, torch.cuda.get_device_name(0)))
        for name in [n for n in args.graphs.split(",") if n]:
            rp, ci, K = load_graph(name, dev)
            csc = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (csc[0], csc[1], csc[2].to(torch.int32))
            for case in args.cases.split(","):
                H, F = (int(v) for v in case.split("x"))
                kernels(rp, ci, csc, K, H, F, args.rounds, args.launches, log, name)
            del rp, ci, csc
            torch.cuda.empty_cache()
        for name in [n for n in args.step_graphs.split(",") if n]:
            steps(name, dev, args.steps, args.rounds, log)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
