"""Timing of the fused GATv2 attention (gespmm_gatv2_attention_f32 + its two backward launches) against the composition it replaces — the
default ``GATv2Conv`` path of this same tree — IN THE SAME PROCESS, the forms alternating.

Every figure is the median of per-launch event pairs after a warm-up, as bench.py measures (--launches of them; where one launch
takes more than 5 ms, a quarter as many). Each form is measured --repeats times (default 3), the forms taking turns inside every
repeat; the run-to-run MARGIN is the largest spread among the repeated medians of the SAME form, and a form is called faster or slower
only where all its medians lie beyond all of the other's by more than that margin.

Forms, per graph and (H, F); negative_slope 0.2, no dropout (the dropout forms are NOT RUN by this script):
  (a)  the three launches on preallocated results: attention.gatv2_attention (out, stats); gatv2_attention_backward_row (delta, grad_xl,
       att_part); gatv2_attention_backward_col (grad_xr) — nothing of size nnz
  (a') the same through autograd: GATv2AttentionFunction forward, and torch.autograd.grad for xl, xr and att (allocations and
       att_part.sum(0) included) — what GATv2Conv(fused=True) runs
  (b)  the composition through autograd: GATv2ScoreFunction -> EdgeSoftmaxFunction -> MultiHeadSPMMFunction(heads_sddmm=True) and
       torch.autograd.grad for xl, xr and att — what GATv2Conv(fused=False) runs: score, softmax, product, and their backward
(a') and (b) are compared; (a) shows what the launches alone take. Before anything is timed the results of (a) and (b) are compared
(1e-4 of the largest value, the layer tests' rule); outside it the run ends. (b) is not run where its [nnz, H] arrays would pass
--b-limit-gb (six counted: score, alpha, their gradients, two in CSC order); the size it would need is printed instead.

  python scripts/gatv2_attention_timing.py [--graphs com-amazon-sbm,pubmed] [--cases 1x64,4x16,8x8,8x32] [--launches 200] [--repeats 3]
                                           [--out profiles/r20/gatv2_attention/timing.log]
  python scripts/gatv2_attention_timing.py --step [--graphs pubmed,com-amazon-sbm,products-sbm] [--cases 8x8]
        time and peak device memory of one training step of examples/gat_custom.py's two-layer model with --v2, with and without
        --fused-attention; a graph whose composition step would not fit the device's free memory is named as not run for (b)
"""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dot_attention_timing import timed  # noqa: E402
from gat_softmax_timing import load_graph  # noqa: E402
import gespmm_amd  # noqa: E402
from gespmm_amd import attention, graphs  # noqa: E402

GRAPHS = "com-amazon-sbm,pubmed"
CASES = "1x64,4x16,8x8,8x32"
SLOPE = 0.2
FORMS = ("a_fwd", "a_row", "a_col", "f_fwd", "f_bwd", "b_fwd", "b_bwd")


def measure(rp, ci, csc, K, H, F, launches, repeats, b_limit):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    xl = (torch.rand(M, H, F, device=dev, generator=gen) - 0.5) * 2
    xr = (torch.rand(K, H, F, device=dev, generator=gen) - 0.5) * 2
    att = (torch.rand(H, F, device=dev, generator=gen) - 0.5) * 2
    go = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    out, stats, delta = torch.empty(M, H, F, device=dev), torch.empty(M, H, 2, device=dev), torch.empty(M, H, device=dev)
    gxl, part, gxr = torch.empty(M, H, F, device=dev), torch.empty(M, H, F, device=dev), torch.empty(K, H, F, device=dev)
    leaves = [t.clone().requires_grad_(True) for t in (xl, xr, att)]
    kept = {}

    def a_fwd():
        attention.gatv2_attention(rp, ci, xl, xr, att, negative_slope=SLOPE, out=out, stats=stats)

    def a_row():
        attention.gatv2_attention_backward_row(rp, ci, xl, xr, att, stats, out, go, negative_slope=SLOPE, results=(delta, gxl, part))

    def a_col():
        attention.gatv2_attention_backward_col(colptr, rowind, xl, xr, att, stats, delta, go, negative_slope=SLOPE, result=gxr)

    def f_fwd():
        kept["f"] = gespmm_amd.GATv2AttentionFunction.apply(rp, ci, colptr, rowind, *leaves, SLOPE, 0.0, None)

    def f_bwd():
        kept["fg"] = torch.autograd.grad(kept["f"], leaves, go, retain_graph=True)

    def b_fwd():
        score = gespmm_amd.GATv2ScoreFunction.apply(rp, ci, colptr, rowind, order, *leaves, SLOPE)
        alpha = gespmm_amd.EdgeSoftmaxFunction.apply(rp, score, None)
        kept["b"] = gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, leaves[1], alpha, None, True)

    def b_bwd():
        kept["bg"] = torch.autograd.grad(kept["b"], leaves, go, retain_graph=True)

    fns = {"a_fwd": a_fwd, "a_row": a_row, "a_col": a_col, "f_fwd": f_fwd, "f_bwd": f_bwd, "b_fwd": b_fwd, "b_bwd": b_bwd}
    res = {"M": M, "nnz": nnz, "b_bytes": 6 * nnz * H * 4, "runs": {k: [] for k in FORMS}}
    with_b = res["b_bytes"] <= b_limit
    forms = [k for k in FORMS if with_b or not k.startswith("b_")]
    for k in forms:
        fns[k]()
    if with_b:
        rel = []
        for got, want in ((out, kept["b"]), (gxl, kept["bg"][0]), (gxr, kept["bg"][1]), (part.sum(0), kept["bg"][2]), (kept["f"], kept["b"])):
            rel.append(float((got.detach() - want.detach()).abs().max()) / max(float(want.detach().abs().max()), 1e-30))
        res["rel"] = rel
    for _ in range(repeats):  # the forms take turns inside every repeat
        for k in forms:
            res["runs"][k].append(timed(fns[k], launches))
    kept.clear()
    return res


def verdict(mine, other, margin):
    if max(mine) < min(other) - margin:
        return "faster"
    if min(mine) > max(other) + margin:
        return "SLOWER"
    return "not different"


def training_step(name, dev, launches, H, F):
    """Median time and peak allocated memory (above the graph and the features) of one training step — forward, loss, backward, Adam —
    of examples/gat_custom.py's Net with v2=True (64 input features, H heads x F, then 1 head, 16 classes; dropout off)."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    nnz = ci.numel()
    out = {}
    for key in ("fused", "composition"):
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info()[0]
        need = 8 * nnz * H * 4 + 8 * nnz * 4  # the first layer's [nnz, H] arrays and the second's [nnz, 1] ones, with slack
        if key == "composition" and need > 0.8 * free:
            out[key] = None
            continue
        torch.manual_seed(0)
        model = ex.Net(64, 16, F, H, dropout=0.0, v2=True, fused_attention=(key == "fused")).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.nll_loss(model(x, g), y)
            loss.backward()
            opt.step()
            return loss

        step()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss = float(step().detach())
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        out[key] = (timed(step, launches), peak, loss)
        del model, opt
        torch.cuda.empty_cache()
    return nnz, K, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=GRAPHS)
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--b-limit-gb", type=float, default=64.0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "gatv2_attention", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if args.step:
            for name in args.graphs.split(","):
                for case in args.cases.split(","):
                    H, F = (int(w) for w in case.split("x"))
                    nnz, n, res = training_step(name, dev, min(args.launches, 50), H, F)
                    log("#step %s nodes=%d nnz=%d (self-loops not added) two-layer GATv2 model 64 -> %d x %d -> 16, one training step, median us "
                        "and peak allocated above the graph and the features: %s; one [nnz, %d] fp32 array is %.1f MB" % (
                            name, n, nnz, H, F,
                            "  ".join("%s %.1f us %.1f MB (loss %.6f)" % ((k,) + (w[0], w[1] / 2 ** 20, w[2])) if w else
                                      "%s NOT RUN: its edge arrays would not fit the device's free memory" % k for k, w in res.items()),
                            H, nnz * H * 4 / 2 ** 20))
            return
        log("# %s launches=%d repeats=%d device=%s (us; median of per-launch event pairs; forms alternating in one process)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, args.repeats, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (colptr, rowind, order.to(torch.int32))
            log("%s M=%d nnz=%d largest row %d largest column %d" % (name, rp.numel() - 1, ci.numel(), int(torch.diff(rp).max()),
                                                                     int(torch.diff(colptr).max())))
            for case in args.cases.split(","):
                H, F = (int(w) for w in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches, args.repeats, args.b_limit_gb * 2 ** 30)
                torch.cuda.empty_cache()
                head = "%-15s H=%d F=%d" % (name, H, F)
                runs = m["runs"]

                def show(k):
                    return " ".join("%.1f" % w for w in runs[k])

                log("%s (a) launches alone: forward %s   row pass %s   column pass %s" % (head, show("a_fwd"), show("a_row"), show("a_col")))
                if not runs["b_fwd"]:
                    log("   (a') forward %s   backward %s   (b) NOT RUN: its [nnz, H] arrays would take %.1f GB (one is %.1f GB)" % (
                        show("f_fwd"), show("f_bwd"), m["b_bytes"] / 2 ** 30, m["b_bytes"] / 6 / 2 ** 30))
                    continue
                log("   max |(a) - (b)| / max |(b)|: out %.2e grad_xl %.2e grad_xr %.2e grad_att %.2e; (a') out %.2e" % tuple(m["rel"]))
                if max(m["rel"]) > 1e-4:
                    raise SystemExit("the fused results are outside the layer tests' rule: nothing timed is worth recording")
                for d, what in (("fwd", "forward"), ("bwd", "backward")):
                    mine, base = runs["f_" + d], runs["b_" + d]
                    margin = max(max(mine) - min(mine), max(base) - min(base))
                    med_a, med_b = sorted(mine)[len(mine) // 2], sorted(base)[len(base) // 2]
                    log("   %-8s (a') %s   (b) composition %s   margin (largest spread of one form) %.1f   (b)/(a') x%.2f: (a') is %s" % (
                        what, show("f_" + d), show("b_" + d), margin, med_b / med_a, verdict(mine, base, margin)))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
