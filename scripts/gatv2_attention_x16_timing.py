"""Timing of the fused GATv2 attention on bf16 node terms (gespmm_gatv2_attention_x16 and its two backward passes) against the fp32 fused
entry points IN THE SAME RUN, on the same values: the fp32 operands are the bf16 ones, widened.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures. The two forms
take turns, pass by pass.

Columns, per graph and (H, F); slope 0.2; results into preallocated tensors:
  x16   attention.gatv2_attention_x16 (forward), gatv2_attention_backward_row_x16 with att_part (row pass), _backward_col_x16 (column pass)
  f32   attention.gatv2_attention / _backward_row / _backward_col on xl.float(), xr.float(), grad_out.float(); the row pass is fed the
        widened 16-bit out, the column pass that delta
Before anything is timed the bf16 results are checked against the fp32 ones where both describe calls answer the same (V, W): stats,
delta and att_part bit for bit, out, grad_xl and grad_xr against the fp32 results narrowed by torch bit for bit. Each run appends a
`#run` line per case and pass; from the third run of the script on, the spread of the fp32 medians ACROSS the runs is the margin the
bf16 ones are judged against.

  python scripts/gatv2_attention_x16_timing.py [--graphs com-amazon-sbm,pubmed] [--cases 1x64,4x16,8x8,8x32] [--launches 200]
                                               [--out profiles/r22/gatv2_attention_x16/timing.log]
  python scripts/gatv2_attention_x16_timing.py --step [--graphs com-amazon-sbm,pubmed,products-sbm]
        time and peak device memory of one training step of examples/gat_custom.py's two-layer --v2 model: --fused-attention in fp32,
        --fused-attention as a .bfloat16() model on bf16 features, and the bf16 model with fused=False
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
from gat_softmax_timing import SLOPE, load_graph  # noqa: E402
from gespmm_amd import _lib, attention, graphs  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed")
STEP_GRAPHS = ("com-amazon-sbm", "pubmed", "products-sbm")
PASSES = (("fwd", "forward"), ("row", "row pass (delta, grad_xl, att_part)"), ("col", "column pass (grad_xr)"))


def _bits_equal(a, b):
    view = torch.int16 if a.element_size() == 2 else torch.int32
    return a.dtype == b.dtype and bool((a.contiguous().view(view) == b.contiguous().view(view)).all())


def measure(rp, ci, csc, K, H, F, launches):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    bf = torch.bfloat16
    xl = ((torch.rand(M, H, F, device=dev, generator=gen) - 0.5) * 2).to(bf)
    xr = ((torch.rand(K, H, F, device=dev, generator=gen) - 0.5) * 2).to(bf)
    att = (torch.rand(H, F, device=dev, generator=gen) - 0.5) * 2
    go = (torch.rand(M, H, F, device=dev, generator=gen) - 0.5).to(bf)
    ops = {"x16": (xl, xr, go, bf, attention.gatv2_attention_x16, attention.gatv2_attention_backward_row_x16,
                   attention.gatv2_attention_backward_col_x16),
           "f32": (xl.float(), xr.float(), go.float(), torch.float32, attention.gatv2_attention, attention.gatv2_attention_backward_row,
                   attention.gatv2_attention_backward_col)}
    fns, outs = {}, {}
    for key in ("x16", "f32"):  # (x16 first: the fp32 row pass reads its out, widened)
        a, b, g, dt, fwd, row, col = ops[key]
        out, gxl, gxr = (torch.empty(s, device=dev, dtype=dt) for s in ((M, H, F), (M, H, F), (K, H, F)))
        stats, delta, part = torch.empty(M, H, 2, device=dev), torch.empty(M, H, device=dev), torch.empty(M, H, F, device=dev)
        outs[key] = {"out": out, "stats": stats, "delta": delta, "grad_xl": gxl, "att_part": part, "grad_xr": gxr}
        fed = out  # the row pass's `out`
        if key == "f32":
            fed = torch.empty_like(out)
        fns[key] = {
            "fwd": lambda a=a, b=b, fwd=fwd, out=out, stats=stats: fwd(rp, ci, a, b, att, negative_slope=SLOPE, out=out, stats=stats),
            "row": lambda a=a, b=b, g=g, row=row, fed=fed, stats=stats, delta=delta, gxl=gxl, part=part:
                row(rp, ci, a, b, att, stats, fed, g, negative_slope=SLOPE, results=(delta, gxl, part)),
            "col": lambda a=a, b=b, g=g, col=col, stats=stats, delta=delta, gxr=gxr:
                col(colptr, rowind, a, b, att, stats, delta, g, negative_slope=SLOPE, result=gxr),
        }
        fns[key]["fwd"]()
        if key == "f32":
            fed.copy_(outs["x16"]["out"].float())
        fns[key]["row"]()
        fns[key]["col"]()
    torch.cuda.synchronize()
    d16, d32 = _lib.describe_gatv2_attention(M, K, H, F, nnz, x16=True), _lib.describe_gatv2_attention(M, K, H, F, nnz)
    same = (d16["V"], d16["W"]) == (d32["V"], d32["W"])
    o16, o32 = outs["x16"], outs["f32"]
    ok = same and all(_bits_equal(o16[k], o32[k]) for k in ("stats", "delta", "att_part")) and \
        all(_bits_equal(o16[k], o32[k].to(bf)) for k in ("out", "grad_xl", "grad_xr"))
    res = {"M": M, "nnz": nnz, "ok": ok, "same": same, "d16": d16, "d32": d32}
    if ok:
        for d, _ in PASSES:  # the two columns alternate, pass by pass
            for key in ("x16", "f32"):
                res[key + "_" + d] = median_us(fns[key][d], launches)
    return res


def training_step(name, dev, launches):
    """Median time and peak allocated memory (above the graph and the features) of one training step — forward, loss, backward, Adam —
    of examples/gat_custom.py's Net with --v2 (64 input features, 8 heads x 8, then 1 head, 16 classes; dropout off): the fused
    attention in fp32, the fused attention as a .bfloat16() model on bf16 features, and the bf16 model with fused=False."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x32 = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    nnz = ci.numel()
    free = torch.cuda.mem_get_info()[0]
    out = {}
    for key, dt, fused in (("fp32 fused", torch.float32, True), ("bf16 fused", torch.bfloat16, True), ("bf16 fused=False", torch.bfloat16, False)):
        if not fused and 16 * nnz * 8 * 4 > free:  # (the composition holds several [nnz, 8] fp32 arrays per layer and direction)
            out[key] = None
            continue
        torch.manual_seed(0)
        model = ex.Net(64, 16, 8, 8, dropout=0.0, v2=True, fused_attention=fused).to(dev).to(dt)
        x = x32.to(dt)
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.nll_loss(model(x, g).float(), y)
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
        out[key] = (median_us(step, launches, warmup=3), peak, loss)
        del model, opt, x
        torch.cuda.empty_cache()
    return nnz, K, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=None)
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "gatv2_attention_x16", "timing.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a time taken anywhere else says nothing")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    names = args.graphs.split(",") if args.graphs else (STEP_GRAPHS if args.step else GRAPHS)
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if args.step:
            for name in names:
                nnz, n, res = training_step(name, dev, min(args.launches, 50))
                log("#step %s nodes=%d nnz=%d (self-loops not added) two-layer --v2 model 64 -> 8 x 8 -> 16, one training step, median us and "
                    "peak allocated above the graph and the features: %s; one [nnz, 8] fp32 array is %.1f MB" % (
                        name, n, nnz, "  ".join("%s %.1f us %.1f MB (loss %.6f)" % (k, v[0], v[1] / 2 ** 20, v[2]) if v else
                                                "%s NOT RUN (its edge arrays would not fit the free memory)" % k for k, v in res.items()),
                        nnz * 8 * 4 / 2 ** 20))
            return
        log("# %s launches=%d slope=%s device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, SLOPE, torch.cuda.get_device_name(0)))
        for name in names:
            rp, ci, K = load_graph(name, dev)
            csc = graphs.transpose_csr(rp, ci, K)
            for case in args.cases.split(","):
                H, F = (int(v) for v in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches)
                torch.cuda.empty_cache()
                log("%-15s H=%d F=%d M=%d nnz=%d x16 V=%d W=%d, f32 V=%d W=%d%s" % (
                    name, H, F, m["M"], m["nnz"], m["d16"]["V"], m["d16"]["W"], m["d32"]["V"], m["d32"]["W"],
                    " (same V, W: stats, delta, att_part bit-equal; out, grad_xl, grad_xr the fp32 ones narrowed once)" if m["ok"] else ""))
                if not m["ok"]:
                    raise SystemExit("the 16-bit results are not the fp32 ones rounded once: nothing timed is worth recording")
                for d, what in PASSES:
                    t16, t32 = m["x16_" + d], m["f32_" + d]
                    log("   %-36s x16 %.1f   f32 %.1f   f32 / x16 x%.2f" % (what, t16, t32, t32 / t16))
                    log("#run %s %s %s x16=%.1f f32=%.1f" % (name, case, d, t16, t32))
                    r = before.get((name, case, d), {})
                    base, mine = r.get("f32", []) + [t32], r.get("x16", []) + [t16]
                    if len(base) >= 3:
                        margin = max(base) - min(base)
                        verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                        log("   over %d runs: f32 %s, margin = spread %.1f; x16 %s: %s than f32 beyond the margin" % (
                            len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
