"""Timing of the GATv2 edge score on bf16 node operands (gespmm_gatv2_score_x16 + gespmm_gatv2_score_backward_x16) against the fp32
entry points IN THE SAME RUN, on the same values: the fp32 operands are the bf16 ones, widened.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures.

Columns, per graph and (H, F); slope 0.2; results into preallocated tensors:
  x16   sddmm.gatv2_score_x16 (forward), sddmm.gatv2_score_backward_x16 with att_part (row pass) and through csc_order (column pass)
  f32   sddmm.gatv2_score / sddmm.gatv2_score_backward on xl.float(), xr.float()
Before anything is timed the bf16 results are checked against the fp32 ones: att_part bit for bit, grad_xl and grad_xr against the
fp32 gradients narrowed by torch bit for bit, the score bit for bit where both resolve to the same (V, W) and to 1e-5 of the largest
value elsewhere (two fp32 summation orders). Each run appends a `#run` line per case and pass; from the third run of the script on,
the spread of the fp32 medians ACROSS the runs is the margin the bf16 ones are judged against.

  python scripts/gatv2_x16_timing.py [--graphs com-amazon-sbm,pubmed] [--cases 1x64,4x16,8x8,8x32] [--launches 200]
                                     [--out profiles/r21/gatv2_x16/timing.log]
  python scripts/gatv2_x16_timing.py --step      time and peak device memory of one training step of the example's two-layer --v2
                                                 model in fp32 and as a .bfloat16() model on bf16 features
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
from gespmm_amd import _lib, graphs, sddmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed")
PASSES = (("fwd", "forward"), ("row", "row pass (grad_xl, att_part)"), ("col", "column pass (grad_xr)"))


def _bits_equal(a, b):
    view = torch.int16 if a.element_size() == 2 else torch.int32
    return a.dtype == b.dtype and bool((a.contiguous().view(view) == b.contiguous().view(view)).all())


def measure(rp, ci, csc, K, H, F, launches):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    xl = (torch.rand(M, H, F, device=dev, generator=gen) - 0.5).bfloat16()
    xr = (torch.rand(K, H, F, device=dev, generator=gen) - 0.5).bfloat16()
    att = (torch.rand(H, F, device=dev, generator=gen) - 0.5) * 2
    gs = torch.rand(nnz, H, device=dev, generator=gen) - 0.5
    ops = {"x16": (xl, xr, sddmm.gatv2_score_x16, sddmm.gatv2_score_backward_x16, torch.bfloat16),
           "f32": (xl.float(), xr.float(), sddmm.gatv2_score, sddmm.gatv2_score_backward, torch.float32)}
    fns, outs = {}, {}
    for key, (a, b, fwd, bwd, dt) in ops.items():
        score, part = torch.empty(nnz, H, device=dev), torch.empty(M, H, F, device=dev)
        gxl, gxr = torch.empty(M, H, F, device=dev, dtype=dt), torch.empty(K, H, F, device=dev, dtype=dt)
        outs[key] = (score, gxl, part, gxr)
        fns[key] = {
            "fwd": lambda a=a, b=b, fwd=fwd, score=score: fwd(rp, ci, a, b, att, negative_slope=SLOPE, out=score),
            "row": lambda a=a, b=b, bwd=bwd, gxl=gxl, part=part: bwd(rp, ci, gs, a, b, att, negative_slope=SLOPE, want_att_part=True,
                                                                     out=(gxl, part)),
            "col": lambda a=a, b=b, bwd=bwd, gxr=gxr: bwd(colptr, rowind, gs, b, a, att, negative_slope=SLOPE, order=order, out=gxr),
        }
        for f in fns[key].values():
            f()
    torch.cuda.synchronize()
    d16, d32 = _lib.describe_gatv2_score(M, nnz, H, F, x16=True), _lib.describe_gatv2_score(M, nnz, H, F)
    same = (d16["V"], d16["W"]) == (d32["V"], d32["W"])
    s16, s32 = outs["x16"][0], outs["f32"][0]
    rel = float((s16 - s32).abs().max() / s32.abs().max().clamp_min(1e-30))
    ok = (_bits_equal(s16, s32) if same else rel <= 1e-5) and _bits_equal(outs["x16"][2], outs["f32"][2]) and \
        _bits_equal(outs["x16"][1], outs["f32"][1].bfloat16()) and _bits_equal(outs["x16"][3], outs["f32"][3].bfloat16())
    res = {"M": M, "nnz": nnz, "ok": ok, "rel": rel, "same": same, "d16": d16, "d32": d32}
    if ok:
        for d, _ in PASSES:  # the two columns alternate, pass by pass
            for key in ("x16", "f32"):
                res[key + "_" + d] = median_us(fns[key][d], launches)
    return res


def training_step(name, dev, launches):
    """Median time and peak allocated memory (above the graph and the features) of one training step — forward, loss, backward, Adam —
    of examples/gat_custom.py's Net with --v2 (64 input features, 8 heads x 8, then 1 head, 16 classes; dropout off), in fp32 and as a
    .bfloat16() model on bf16 features."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x32 = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    out = {}
    for key, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        torch.manual_seed(0)
        model = ex.Net(64, 16, 8, 8, dropout=0.0, v2=True).to(dev).to(dt)
        x = x32.to(dt)
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
        out[key] = (median_us(step, launches, warmup=3), peak, loss)
        del model, opt, x
        torch.cuda.empty_cache()
    return ci.numel(), K, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "gatv2_x16", "timing.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a time taken anywhere else says nothing")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if args.step:
            for name in args.graphs.split(","):
                nnz, n, res = training_step(name, dev, min(args.launches, 50))
                log("#step %s nodes=%d nnz=%d (self-loops not added) two-layer --v2 model 64 -> 8 x 8 -> 16, one training step, median us and "
                    "peak allocated above the graph and the features: %s; one [nnz, 8] fp32 array is %.1f MB" % (
                        name, n, nnz, "  ".join("%s %.1f us %.1f MB (loss %.6f)" % (k, v[0], v[1] / 2 ** 20, v[2]) for k, v in res.items()),
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
                torch.cuda.empty_cache()
                log("%-15s H=%d F=%d M=%d nnz=%d forward x16 V=%d W=%d epw=%d, f32 V=%d W=%d epw=%d; max |score x16 - f32| / max |f32| %.2e%s" % (
                    name, H, F, m["M"], m["nnz"], m["d16"]["V"], m["d16"]["W"], m["d16"]["epw"], m["d32"]["V"], m["d32"]["W"], m["d32"]["epw"],
                    m["rel"], " (same V, W: bit-equal)" if m["same"] else ""))
                if not m["ok"]:
                    raise SystemExit("the 16-bit results are not the fp32 ones rounded once: nothing timed is worth recording")
                for d, what in PASSES:
                    t16, t32 = m["x16_" + d], m["f32_" + d]
                    log("   %-30s x16 %.1f   f32 %.1f   f32 / x16 x%.2f" % (what, t16, t32, t32 / t16))
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
