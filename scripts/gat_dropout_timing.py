"""Timing of dropout on the attention coefficients (the *_dropout_f32 entry points; mask recomputed from a seed, never stored)
against the entry points without it, IN THE SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures.

Per graph and (H, F), everything into preallocated results, slope 0.2, p = 0.6:
  (a)  each dropout launch against its base entry point — what the mask costs:
         fwd   spmm.gat_aggregate(dropout=)                    vs  spmm.gat_aggregate
         bwdT  spmm.gat_aggregate(transposed=True, dropout=)   vs  spmm.gat_aggregate(transposed=True)
         el    softmax.gat_backward_el(dropout=)               vs  softmax.gat_backward_el
         er    softmax.gat_backward_er(dropout=)               vs  softmax.gat_backward_er
  (b)  the fused aggregate with dropout against the composition softmax.gat_edge_softmax + softmax.edge_dropout (in place) +
       spmm.csr_spmm_heads (alpha written and read back twice)
The dropout aggregate is checked against (b)'s composition bit for bit before anything is timed. Each run appends a `#run` line per
case and direction; from the third run of the script on, the spread of the base column's medians ACROSS the runs is the margin the
dropout column is judged against. Within a pair the dropout form is timed first; `--base-first` turns that round, and the runs of a
record alternate, so that an effect of the order shows as a disagreement between runs instead of a difference between columns.

  python scripts/gat_dropout_timing.py [--graphs a,b] [--cases 1x64,4x16,8x8,8x32] [--launches 200] [--out profiles/r14/gat_dropout/timing.log]
  python scripts/gat_dropout_timing.py --memory [--graphs products-sbm]    peak device memory of one forward + backward step of the example's
                                                                           two-layer GAT with fused_backward, attention dropout off and on
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
from gespmm_amd import graphs, softmax, spmm  # noqa: E402

P = 0.6
PAIRS = (("fwd", "aggregate forward"), ("bwdT", "aggregate transposed"), ("el", "backward_el"), ("er", "backward_er"))


def measure(rp, ci, csc, K, H, F, launches, base_first=False):
    dev = rp.device
    M = rp.numel() - 1
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    el = (torch.rand(M, H, device=dev, generator=gen) - 0.5) * 4
    er = (torch.rand(K, H, device=dev, generator=gen) - 0.5) * 4
    feat = torch.rand(K, H, F, device=dev, generator=gen) - 0.5
    gout = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    seed = torch.randint(-(2 ** 31), 2 ** 31, (2,), dtype=torch.int32, device=dev, generator=gen)
    stats = softmax.gat_softmax_stats(rp, ci, el, er, negative_slope=SLOPE)
    out, out_t = torch.empty(M, H, F, device=dev), torch.empty(K, H, F, device=dev)
    delta, gel, ger = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev), torch.empty(K, H, device=dev)
    alpha = torch.empty(ci.numel(), H, device=dev)
    comp = torch.empty(M, H, F, device=dev)
    kw = dict(negative_slope=SLOPE)

    def calls(drop):
        return {"fwd": lambda: spmm.gat_aggregate(rp, ci, el, er, stats, feat, out=out, dropout=drop, **kw),
                "bwdT": lambda: spmm.gat_aggregate(colptr, rowind, el, er, stats, gout, transposed=True, out=out_t, dropout=drop, **kw),
                "el": lambda: softmax.gat_backward_el(rp, ci, el, er, stats, gout, feat, out=(delta, gel), dropout=drop, **kw),
                "er": lambda: softmax.gat_backward_er(colptr, rowind, el, er, stats, delta, gout, feat, out=ger, dropout=drop, **kw)}

    def composition():
        softmax.gat_edge_softmax(rp, ci, el, er, negative_slope=SLOPE, out=alpha)
        softmax.edge_dropout(rp, ci, alpha, P, seed, out=alpha)
        spmm.csr_spmm_heads(rp, ci, alpha, feat, out=comp)

    base, drop = calls(None), calls((P, seed))
    drop["el"]()  # (delta for the column pass)
    drop["fwd"](), composition()
    res = {"M": M, "nnz": ci.numel(), "same_bits": bool((out.view(torch.int32) == comp.view(torch.int32)).all()),
           "kept": float((alpha != 0).float().mean())}
    for key, _ in PAIRS:  # (which of the two is timed first alternates between runs: --base-first)
        if base_first:
            b = median_us(base[key], launches)
            res[key] = (median_us(drop[key], launches), b)
        else:
            res[key] = (median_us(drop[key], launches), median_us(base[key], launches))
    res["composition"] = median_us(composition, launches)
    return res


def peak_memory(name, dev):
    """Peak allocated device memory of one forward + backward step of examples/gat_custom.py's Net (8 heads x 8, then 1 head; 64 input
    features, 16 classes, feature dropout off) with fused_backward, attention dropout 0 and 0.6, the graph and the features excluded."""
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
    for key, p in (("fused_backward", 0.0), ("fused_backward+attn_dropout_0.6", P)):
        torch.manual_seed(0)
        model = ex.Net(64, 16, 8, 8, dropout=0.0, fused_backward=True, attn_dropout=p).to(dev)
        model.train()
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
    ap.add_argument("--base-first", action="store_true", help="(a): time the base entry point before its dropout form (default: after)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "gat_dropout", "timing.log"))
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
        log("# %s launches=%d slope=%s p=%s device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, SLOPE, P, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (colptr, rowind, order.to(torch.int32))
            del order
            for case in args.cases.split(","):
                H, F = (int(v) for v in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches, args.base_first)
                log("%-15s H=%d F=%d M=%d nnz=%d kept %.4f of the weights; aggregate(dropout) == csr_spmm_heads(edge_dropout(softmax)) bit for bit: %s" % (
                    name, H, F, m["M"], m["nnz"], m["kept"], m["same_bits"]))
                if not m["same_bits"]:
                    raise SystemExit("the fused aggregate with dropout differs from its composition: nothing timed is worth recording")
                for key, what in PAIRS:
                    d, b = m[key]
                    log("   (a) %-21s dropout %.1f   base %.1f   dropout / base x%.3f" % (what, d, b, d / b))
                    log("#run %s %s %s dropout=%.1f base=%.1f" % (name, case, key, d, b))
                    r = before.get((name, case, key), {})
                    bs, ds = r.get("base", []) + [b], r.get("dropout", []) + [d]
                    if len(bs) >= 3:
                        margin = max(bs) - min(bs)
                        verdict = "FASTER" if max(ds) < min(bs) - margin else ("SLOWER" if min(ds) > max(bs) + margin else "not different")
                        log("       over %d runs: base %s, margin = spread %.1f; dropout %s: %s than base beyond the margin" % (
                            len(bs), " ".join("%.1f" % v for v in bs), margin, " ".join("%.1f" % v for v in ds), verdict))
                d, c = m["fwd"][0], m["composition"]
                log("   (b) aggregate(dropout) %.1f   softmax + edge_dropout + csr_spmm_heads %.1f   composition / fused x%.2f" % (d, c, c / d))
                log("#run %s %s comp fused=%.1f composition=%.1f" % (name, case, d, c))
                r = before.get((name, case, "comp"), {})
                cs, fs = r.get("composition", []) + [c], r.get("fused", []) + [d]
                if len(cs) >= 3:
                    margin = max(cs) - min(cs)
                    verdict = "FASTER" if max(fs) < min(cs) - margin else ("SLOWER" if min(fs) > max(cs) + margin else "not different")
                    log("       over %d runs: composition %s, margin = spread %.1f; fused %s: %s than the composition beyond the margin" % (
                        len(cs), " ".join("%.1f" % v for v in cs), margin, " ".join("%.1f" % v for v in fs), verdict))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
