"""Timing of the fused GAT backward for el / er (gespmm_gat_backward_el_f32 + gespmm_gat_backward_er_f32) against the four steps
GATAggregateFunction runs without it, IN THE SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures.

Columns, per graph and (H, F), everything into preallocated results where the call takes one; slope 0.2:
  (a)  softmax.gat_backward_el + softmax.gat_backward_er                                 (two launches, nothing of size nnz H)
  (b)  softmax.gat_edge_softmax + sddmm.csr_sddmm_heads + softmax.gat_edge_softmax_backward + softmax.edge_segment_sum(colptr, order)
       (today: alpha, grad_alpha and grad_score written and read back; the last two calls allocate their results, as in the layer)
(a) is checked against (b) before anything is timed: bit for bit, and where they differ (the dot product's summation order) both
against float64 on a sample of the rows. Each run appends a `#run` line per case; from the third run of the script on, the spread of
(b)'s medians ACROSS the runs is the margin (a) is judged against.

  python scripts/gat_backward_timing.py [--graphs a,b] [--cases 1x64,4x16,8x8,8x32] [--launches 200] [--out profiles/r13/gat_backward/timing.log]
  python scripts/gat_backward_timing.py --memory [--graphs products-sbm]      peak device memory of one forward + backward step of the
                                                                               example's two-layer GAT, fused_aggregate and fused_backward
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
from gat_aggregate_timing import CASES, earlier_runs  # noqa: E402
from gat_softmax_timing import GRAPHS, SLOPE, load_graph  # noqa: E402
from gespmm_amd import graphs, sddmm, softmax  # noqa: E402

SAMPLE = 4096  # rows whose entries the float64 check walks


def measure(rp, ci, csc, K, H, F, launches):
    dev = rp.device
    M = rp.numel() - 1
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    el = (torch.rand(M, H, device=dev, generator=gen) - 0.5) * 4
    er = (torch.rand(K, H, device=dev, generator=gen) - 0.5) * 4
    feat = torch.rand(K, H, F, device=dev, generator=gen) - 0.5
    gout = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    stats = softmax.gat_softmax_stats(rp, ci, el, er, negative_slope=SLOPE)
    delta, gel_a, ger_a = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev), torch.empty(K, H, device=dev)
    alpha = torch.empty(ci.numel(), H, device=dev)
    ga = torch.empty(ci.numel(), H, device=dev)
    ger_b = torch.empty(K, H, device=dev)
    kept = {}

    def a():
        softmax.gat_backward_el(rp, ci, el, er, stats, gout, feat, negative_slope=SLOPE, out=(delta, gel_a))
        softmax.gat_backward_er(colptr, rowind, el, er, stats, delta, gout, feat, negative_slope=SLOPE, out=ger_a)

    def b():
        softmax.gat_edge_softmax(rp, ci, el, er, negative_slope=SLOPE, out=alpha)
        sddmm.csr_sddmm_heads(rp, ci, gout, feat, out=ga)
        gs, kept["gel"] = softmax.gat_edge_softmax_backward(rp, ci, alpha, ga, el=el, er=er, negative_slope=SLOPE)
        softmax.edge_segment_sum(colptr, gs, order=order, out=ger_b)

    a(), b()
    gel_b = kept["gel"]
    same = lambda x, y: bool((x.view(torch.int32) == y.view(torch.int32)).all())  # noqa: E731
    res = {"M": M, "nnz": ci.numel(), "el_same_bits": same(gel_a, gel_b), "er_same_bits": same(ger_a, ger_b)}
    # float64 on the first SAMPLE rows (grad_el: the whole sum of a row is inside the sample), bound 1e-4 max(|ref|, scale)
    n = min(SAMPLE, M)
    e = int(rp[n])
    rows = torch.repeat_interleave(torch.arange(n, device=dev), torch.diff(rp[:n + 1]).long())
    cols = ci[:e].long()
    x = (el[rows] + er[cols]).double()
    x = torch.where(x >= 0, x, x * float(torch.tensor(SLOPE, dtype=torch.float32)))
    top = torch.full((n, H), -float("inf"), dtype=torch.float64, device=dev).scatter_reduce(0, rows[:, None].expand(-1, H), x, "amax")
    t = torch.exp(x - top[rows])
    w = t / torch.zeros(n, H, dtype=torch.float64, device=dev).index_add_(0, rows, t)[rows]
    terms = gout[:n][rows].double() * feat[cols].double()
    g, gabs = terms.sum(-1), terms.abs().sum(-1)
    dot = torch.zeros(n, H, dtype=torch.float64, device=dev).index_add_(0, rows, w * g)
    dabs = torch.zeros(n, H, dtype=torch.float64, device=dev).index_add_(0, rows, w * gabs)
    gs64 = w * (g - dot[rows]) * torch.where(el[rows] + er[cols] >= 0, 1.0, float(torch.tensor(SLOPE, dtype=torch.float32)))
    ref = torch.zeros(n, H, dtype=torch.float64, device=dev).index_add_(0, rows, gs64)
    scale = torch.zeros(n, H, dtype=torch.float64, device=dev).index_add_(0, rows, w * (gabs + dabs[rows]))
    bound = 1e-4 * torch.maximum(ref.abs(), scale)
    worst = lambda got: float(((got[:n].double() - ref).abs() / bound.clamp_min(1e-300)).max())  # noqa: E731
    res["f64"] = (worst(gel_a), worst(gel_b))
    del rows, cols, x, t, w, terms, g, gabs, gs64
    diff = lambda u, v: float((u.double() - v.double()).abs().max() / v.double().abs().max().clamp_min(1e-300))  # noqa: E731
    res["rel"] = (diff(gel_a, gel_b), diff(ger_a, ger_b))
    kept.clear()
    del gel_b
    res["a"], res["b"] = median_us(a, launches), median_us(b, launches)
    kept.clear()
    return res


def peak_memory(name, dev):
    """Peak allocated device memory of one forward + backward step of examples/gat_custom.py's Net (8 heads x 8, then 1 head; 64 input
    features, 16 classes, dropout off) with fused_aggregate and with fused_backward, the graph and the features excluded (allocated
    before the reset)."""
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
    for key, kw in (("fused_aggregate", {"fused_aggregate": True}), ("fused_backward", {"fused_backward": True})):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "gat_backward", "timing.log"))
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
                    "above the graph and the features (torch.cuda.max_memory_allocated): %s; one [nnz, 8] fp32 array is %.1f MB" % (
                        name, n, nnz, "  ".join("%s %.1f MB (loss %.6f)" % (k, v[0] / 2 ** 20, v[1]) for k, v in peaks.items()),
                        nnz * 8 * 4 / 2 ** 20))
            return
        log("# %s launches=%d slope=%s device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, SLOPE, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (colptr, rowind, order.to(torch.int32))
            del order
            for case in args.cases.split(","):
                H, F = (int(v) for v in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches)
                log("%-15s H=%d F=%d M=%d nnz=%d grad_el_same_bits=%s grad_er_same_bits=%s max |a - b| / max |b|: grad_el %.2e grad_er %.2e; "
                    "grad_el of the first %d rows against float64, worst error / bound (1e-4 max(|ref|, scale)): (a) %.3g (b) %.3g" % (
                        name, H, F, m["M"], m["nnz"], m["el_same_bits"], m["er_same_bits"], m["rel"][0], m["rel"][1], min(SAMPLE, m["M"]),
                        m["f64"][0], m["f64"][1]))
                if m["f64"][0] > 1.0 or m["rel"][0] > 1e-3 or m["rel"][1] > 1e-3:
                    raise SystemExit("the fused backward is outside its bound: nothing timed is worth recording")
                log("   (a) backward_el + backward_er %.1f   (b) softmax + sddmm + softmax backward + segment sum %.1f   (b)/(a) x%.2f" % (
                    m["a"], m["b"], m["b"] / m["a"]))
                log("#run %s %s bwd fused=%.1f composition=%.1f" % (name, case, m["a"], m["b"]))
                r = before.get((name, case, "bwd"), {})
                base, mine = r.get("composition", []) + [m["b"]], r.get("fused", []) + [m["a"]]
                if len(base) >= 3:
                    margin = max(base) - min(base)
                    verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                    log("   over %d runs: (b) %s, margin = spread %.1f; (a) %s: %s than (b) beyond the margin" % (
                        len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
