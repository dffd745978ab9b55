"""Timing of the fused GAT aggregation (gespmm_gat_softmax_stats_f32 + gespmm_gat_aggregate_f32) against the composition GATConv runs
without it, IN THE SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures.

Columns, per graph and (H, F), everything into preallocated results where the call takes one; slope 0.2:
  forward   (a)  softmax.gat_softmax_stats + spmm.gat_aggregate                     (two launches, no [nnz, H] array)
            (b)  softmax.gat_edge_softmax + spmm.csr_spmm_heads                     (today: alpha written and read back)
            (c)  spmm.csr_spmm_heads alone on a ready alpha                         (the floor: what the gathers of B cost)
  backward of the features
            (a)  spmm.gat_aggregate(colptr, rowind, .., grad_out, transposed=True)  (one launch)
            (b)  alpha[csc_order].contiguous() + spmm.csr_spmm_heads on the CSC arrays
(a) is checked against (b) bit for bit before anything is timed. Each run appends a `#run` line per case; from the third run of the
script on, the spread of (b)'s medians ACROSS the runs is the margin (a) is judged against.

  python scripts/gat_aggregate_timing.py [--graphs a,b] [--cases 1x64,4x16,8x8,8x32] [--launches 200] [--out profiles/r12/gat_aggregate/timing.log]
  python scripts/gat_aggregate_timing.py --memory [--graphs products-sbm]     peak device memory of one forward + backward step of the
                                                                               example's two-layer GAT, fused_score and fused_aggregate
"""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from edge_softmax_timing import median_us  # noqa: E402
from gat_softmax_timing import GRAPHS, SLOPE, load_graph  # noqa: E402
from gespmm_amd import _lib, graphs, softmax, spmm  # noqa: E402

CASES = "1x64,4x16,8x8,8x32"


def earlier_runs(path):
    """{(graph, "HxF", direction): {column: [median of each earlier run]}} from the `#run` lines of the log."""
    runs = {}
    if os.path.exists(path):
        for line in open(path):
            if line.startswith("#run "):
                _, name, case, direction, *cols = line.split()
                d = runs.setdefault((name, case, direction), {})
                for kv in cols:
                    k, v = kv.split("=")
                    d.setdefault(k, []).append(float(v))
    return runs


def measure(rp, ci, csc, K, H, F, launches):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind, order64 = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    el = (torch.rand(M, H, device=dev, generator=gen) - 0.5) * 4
    er = (torch.rand(K, H, device=dev, generator=gen) - 0.5) * 4
    feat = torch.rand(K, H, F, device=dev, generator=gen) - 0.5
    gout = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    stats = torch.empty(M, H, 2, device=dev)
    alpha = torch.empty(nnz, H, device=dev)
    out_a, out_b = torch.empty(M, H, F, device=dev), torch.empty(M, H, F, device=dev)
    gf_a, gf_b = torch.empty(K, H, F, device=dev), torch.empty(K, H, F, device=dev)

    def fwd_a():
        softmax.gat_softmax_stats(rp, ci, el, er, negative_slope=SLOPE, out=stats)
        spmm.gat_aggregate(rp, ci, el, er, stats, feat, negative_slope=SLOPE, out=out_a)

    def fwd_b():
        softmax.gat_edge_softmax(rp, ci, el, er, negative_slope=SLOPE, out=alpha)
        spmm.csr_spmm_heads(rp, ci, alpha, feat, out=out_b)

    def fwd_c():
        spmm.csr_spmm_heads(rp, ci, alpha, feat, out=out_b)

    def bwd_a():
        spmm.gat_aggregate(colptr, rowind, el, er, stats, gout, negative_slope=SLOPE, transposed=True, out=gf_a)

    def bwd_b():
        spmm.csr_spmm_heads(colptr, rowind, alpha[order64].contiguous(), gout, out=gf_b)

    same = lambda x, y: bool((x.view(torch.int32) == y.view(torch.int32)).all())  # noqa: E731

    def against_float64(transposed, got_a, got_b):
        """Where (a) and (b) differ, float64 decides: feature 0 of every head, sum over the entries of alpha (the fp32 weights both are
        specified on) times the dense word in float64, bound 1e-4 max(|ref|, sum |w b|) -> (worst error / bound of (a), of (b))."""
        rows = torch.repeat_interleave(torch.arange(M, device=dev), torch.diff(rp).long())
        cols = ci.long()
        src, dst, n, dense = (rows, cols, K, gout) if transposed else (cols, rows, M, feat)
        terms = alpha.double() * dense[:, :, 0][src].double()
        del rows, cols, src
        ref = torch.zeros(n, H, dtype=torch.float64, device=dev).index_add_(0, dst, terms)
        mag = torch.zeros(n, H, dtype=torch.float64, device=dev).index_add_(0, dst, terms.abs())
        del terms
        bound = 1e-4 * torch.maximum(ref.abs(), mag)
        worst = lambda got: float(((got[:, :, 0].double() - ref).abs() / bound.clamp_min(1e-300)).max())  # noqa: E731
        return worst(got_a), worst(got_b)

    fwd_a(), fwd_b(), bwd_a(), bwd_b()
    res = {"M": M, "nnz": nnz, "route": _lib.gat_aggregate_route(M, K, H, F, nnz), "route_t": _lib.gat_aggregate_route(M, K, H, F, nnz, True),
           "heads_route": _lib.heads_route(M, K, H, F, nnz), "fwd_same_bits": same(out_a, out_b), "bwd_same_bits": same(gf_a, gf_b)}
    for direction, transposed, got_a, got_b in (("fwd", False, out_a, out_b), ("bwd", True, gf_a, gf_b)):
        if not res[direction + "_same_bits"]:
            bad = (got_a.view(torch.int32) != got_b.view(torch.int32))
            res[direction + "_differ"] = (int(bad.sum()), int(bad.any(dim=2).any(dim=1).sum()), int(bad.any(dim=2).any(dim=0).sum()))
            res[direction + "_f64"] = against_float64(transposed, got_a, got_b)
    for key, fn in (("fwd_a", fwd_a), ("fwd_b", fwd_b), ("fwd_c", fwd_c), ("bwd_a", bwd_a), ("bwd_b", bwd_b)):
        res[key] = median_us(fn, launches)
    return res


def peak_memory(name, dev):
    """Peak allocated device memory of one forward + backward step of examples/gat_custom.py's Net (8 heads x 8, then 1 head; 64 input
    features, 16 classes, dropout off) in both fused settings, the graph and the features excluded (allocated before the reset)."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    out = {}
    for key, kw in (("fused_score", {"fused_score": True}), ("fused_aggregate", {"fused_aggregate": True})):
        torch.manual_seed(0)
        model = ex.Net(64, 16, 8, 8, dropout=0.0, **kw).to(dev)
        for _ in range(2):  # the second step is the one measured (pools and code objects exist)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            loss = torch.nn.functional.nll_loss(model(x, g), y)
            loss.backward()
            torch.cuda.synchronize()
            out[key] = (torch.cuda.max_memory_allocated() - base, float(loss.detach()))
            model.zero_grad(set_to_none=True)
            del loss
        del model
    return ci.numel(), K, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "gat_aggregate", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if args.memory:
            for name in (args.graphs.split(",") if args.graphs != ",".join(GRAPHS) else ["products-sbm"]):
                nnz, n, peaks = peak_memory(name, dev)
                log("#memory %s nodes=%d nnz=%d (self-loops not added) two-layer GAT 64 -> 8 x 8 -> 16, one forward + backward, peak allocated "
                    "above the graph and the features (torch.cuda.max_memory_allocated): %s" % (
                        name, n, nnz, "  ".join("%s %.1f MB (loss %.6f)" % (k, v[0] / 2 ** 20, v[1]) for k, v in peaks.items())))
            return
        log("# %s launches=%d slope=%s device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, SLOPE, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            csc = graphs.transpose_csr(rp, ci, K, return_order=True)
            for case in args.cases.split(","):
                H, F = (int(v) for v in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches)
                log("%-15s H=%d F=%d M=%d nnz=%d route fwd %s transposed %s (csr_spmm_heads: %s) fwd_same_bits=%s bwd_same_bits=%s" % (
                    name, H, F, m["M"], m["nnz"], m["route"], m["route_t"], m["heads_route"], m["fwd_same_bits"], m["bwd_same_bits"]))
                for direction in ("fwd", "bwd"):
                    if not m[direction + "_same_bits"]:
                        # float64 decides which of the two is off: (a) must be inside the bound; where (b) is not, the row says so
                        # ("composition_ok=False") and (b)'s time is reported as measured, as gat_softmax_timing.py does
                        ra, rb = m[direction + "_f64"]
                        log("   %s: (a) and (b) differ in %d words of %d segments and %d heads; against float64 (feature 0, bound 1e-4 max(|ref|, "
                            "sum |w b|)) worst error / bound: (a) %.3g (b) %.3g -> composition_ok=%s" % ((direction,) + m[direction + "_differ"] + (
                                ra, rb, rb <= 1.0)))
                        if ra > 1.0 or rb <= 1.0:
                            raise SystemExit("fused and composition disagree and float64 does not side with the fused one: nothing timed is worth recording")
                log("   fwd  (a) stats + aggregate %.1f   (b) softmax + heads product %.1f   (c) heads product alone %.1f   (b)/(a) x%.2f   (a)/(c) x%.2f" % (
                    m["fwd_a"], m["fwd_b"], m["fwd_c"], m["fwd_b"] / m["fwd_a"], m["fwd_a"] / m["fwd_c"]))
                log("   bwd  (a) aggregate(transposed) %.1f   (b) alpha[csc_order] + heads product %.1f   (b)/(a) x%.2f" % (
                    m["bwd_a"], m["bwd_b"], m["bwd_b"] / m["bwd_a"]))
                log("#run %s %s fwd fused=%.1f composition=%.1f floor=%.1f" % (name, case, m["fwd_a"], m["fwd_b"], m["fwd_c"]))
                log("#run %s %s bwd fused=%.1f composition=%.1f" % (name, case, m["bwd_a"], m["bwd_b"]))
                for direction in ("fwd", "bwd"):
                    r = before.get((name, case, direction), {})
                    base, mine = r.get("composition", []) + [m[direction + "_b"]], r.get("fused", []) + [m[direction + "_a"]]
                    if len(base) >= 3:
                        margin = max(base) - min(base)
                        verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                        log("   %s over %d runs: (b) %s, margin = spread %.1f; (a) %s: %s than (b) beyond the margin" % (
                            direction, len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
