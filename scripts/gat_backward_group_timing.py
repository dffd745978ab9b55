"""Timing of the two forms of the fused GAT backward for el / er (gat_backward.hip: one lane per dot; gat_backward_group.hip: a lane
group per dot, the multi-head SDDMM's order) and of the four-step composition, IN THE SAME PROCESS.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures. Slope 0.2.
Columns, per graph and (H, F), everything into preallocated results where the call takes one:
  (a)  gat_backward_el + gat_backward_er under GESPMM_GAT_BACKWARD_FORM=lane
  (b)  the same two calls under GESPMM_GAT_BACKWARD_FORM=group (an ineligible shape, F = 8, runs the lane form again: a null row)
  (c)  gat_edge_softmax + csr_sddmm_heads + gat_edge_softmax_backward + edge_segment_sum(colptr, order)
Before anything is timed (b) is checked against (c) bit for bit where the form is `group` — its contract on any operands — and (a)
against (c) within 1e-3 of the largest value. Each run appends a `#run` line per case; from the third run of the script on, (b) is
judged against (a) as DESIGN 3.18 judges: all runs of one outside all runs of the other by more than the spread of (a)'s runs.

  python scripts/gat_backward_group_timing.py [--graphs a,b] [--cases 1x64,4x16,8x8,8x32,1x128] [--launches 200] [--tag U4] [--out LOG]
  python scripts/gat_backward_group_timing.py --step [--graphs products-sbm]   one training step of examples/gat_custom.py's two-layer GAT
        with fused_backward, 8 x 8 (lane form) and 2 x 64 (wide heads), unpinned / lane / group: time of a step and peak memory

--tag names the build in the `#run` key (the sweep of the steps in flight rebuilds the library with -DGESPMM_GB_GROUP_U=2)."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from edge_softmax_timing import median_us  # noqa: E402
from gat_aggregate_timing import earlier_runs  # noqa: E402
from gat_softmax_timing import SLOPE, load_graph  # noqa: E402
from gespmm_amd import _lib, graphs, sddmm, softmax  # noqa: E402

PIN = "GESPMM_GAT_BACKWARD_FORM"
CASES = "1x64,4x16,8x8,8x32,1x128"


def measure(rp, ci, csc, K, H, F, launches):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    el = (torch.rand(M, H, device=dev, generator=gen) - 0.5) * 4
    er = (torch.rand(K, H, device=dev, generator=gen) - 0.5) * 4
    feat = torch.rand(K, H, F, device=dev, generator=gen) - 0.5
    gout = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    stats = softmax.gat_softmax_stats(rp, ci, el, er, negative_slope=SLOPE)
    out = {pin: (torch.empty(M, H, device=dev), torch.empty(M, H, device=dev), torch.empty(K, H, device=dev)) for pin in ("lane", "group")}
    alpha, ga, ger_c = torch.empty(nnz, H, device=dev), torch.empty(nnz, H, device=dev), torch.empty(K, H, device=dev)
    kept = {}

    def fused(pin):
        delta, gel, ger = out[pin]

        def run():
            softmax.gat_backward_el(rp, ci, el, er, stats, gout, feat, negative_slope=SLOPE, out=(delta, gel))
            softmax.gat_backward_er(colptr, rowind, el, er, stats, delta, gout, feat, negative_slope=SLOPE, out=ger)
        return run

    def composition():
        softmax.gat_edge_softmax(rp, ci, el, er, negative_slope=SLOPE, out=alpha)
        sddmm.csr_sddmm_heads(rp, ci, gout, feat, out=ga)
        gs, kept["gel"] = softmax.gat_edge_softmax_backward(rp, ci, alpha, ga, el=el, er=er, negative_slope=SLOPE)
        softmax.edge_segment_sum(colptr, gs, order=order, out=ger_c)

    res = {"M": M, "nnz": nnz}
    composition()
    same = lambda x, y: bool((x.view(torch.int32) == y.view(torch.int32)).all())  # noqa: E731
    rel = lambda u, v: float((u.double() - v.double()).abs().max() / v.double().abs().max().clamp_min(1e-300))  # noqa: E731
    for pin in ("lane", "group"):
        os.environ[PIN] = pin
        res["form_" + pin] = _lib.describe_gat_backward(M, K, H, F, nnz)["form"]
        fused(pin)()
        _, gel, ger = out[pin]
        res["bits_" + pin] = (same(gel, kept["gel"]), same(ger, ger_c))
        res["rel_" + pin] = (rel(gel, kept["gel"]), rel(ger, ger_c))
        if max(res["rel_" + pin]) > 1e-3 or (res["form_" + pin] == "group" and not all(res["bits_" + pin])):
            raise SystemExit("%s form, H=%d F=%d: outside its contract (%r, %r): nothing timed is worth recording" % (
                pin, H, F, res["bits_" + pin], res["rel_" + pin]))
    for pin in ("lane", "group"):
        os.environ[PIN] = pin
        res[pin] = median_us(fused(pin), launches)
    del os.environ[PIN]
    res["composition"] = median_us(composition, launches)
    kept.clear()
    return res


def training_step(name, dev, log):
    """A forward + backward step of the example's Net (64 input features, 16 classes, dropout off) with fused_backward: wall time of a
    step (median of 10 after 3, host-synchronised) and peak allocated memory above the graph and the features."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    for hidden, heads in ((8, 8), (64, 2)):
        for pin in (None, "lane", "group"):
            os.environ.pop(PIN, None)
            if pin:
                os.environ[PIN] = pin
            torch.manual_seed(0)
            model = ex.Net(64, 16, hidden, heads, dropout=0.0, fused_backward=True).to(dev)
            times, peak, loss = [], 0, None
            for i in range(13):
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                loss = torch.nn.functional.nll_loss(model(x, g), y)
                loss.backward()
                torch.cuda.synchronize()
                if i >= 3:
                    times.append(time.perf_counter() - t0)
                    peak = max(peak, torch.cuda.max_memory_allocated() - base)
                model.zero_grad(set_to_none=True)
            log("#step %s nnz=%d hidden=%d heads=%d form=%s step %.2f ms (median of 10) peak %.1f MB loss %.6f" % (
                name, ci.numel(), hidden, heads, pin or "default", statistics.median(times) * 1e3, peak / 2 ** 20, float(loss.detach())))
            del model, loss
            torch.cuda.empty_cache()
    os.environ.pop(PIN, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="com-amazon-sbm,pubmed")
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--tag", default="U4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "gat_backward_group", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# graphs=%s cases=%s tag=%s%s launches=%d slope=%s device=%s (us; median of per-launch event pairs)" % (
            args.graphs, args.cases, args.tag, " step" if args.step else "", args.launches, SLOPE, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            if args.step:
                training_step(name, dev, log)
                continue
            rp, ci, K = load_graph(name, dev)
            colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (colptr, rowind, order.to(torch.int32))
            del order
            for case in args.cases.split(","):
                H, F = (int(v) for v in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches)
                log("%-15s H=%d F=%d M=%d nnz=%d (b) runs form=%s; grad_el / grad_er same bits as (c): (a) %s (b) %s; max |x - c| / max |c|: "
                    "(a) %.1e %.1e (b) %.1e %.1e" % ((name, H, F, m["M"], m["nnz"], m["form_group"], m["bits_lane"], m["bits_group"])
                                                     + m["rel_lane"] + m["rel_group"]))
                log("   (a) lane %.1f   (b) group %.1f   (c) composition %.1f   (a)/(b) x%.2f   (c)/(b) x%.2f" % (
                    m["lane"], m["group"], m["composition"], m["lane"] / m["group"], m["composition"] / m["group"]))
                key = "bwd" + args.tag
                log("#run %s %s %s lane=%.1f group=%.1f composition=%.1f" % (name, case, key, m["lane"], m["group"], m["composition"]))
                r = before.get((name, case, key), {})
                lane, group = r.get("lane", []) + [m["lane"]], r.get("group", []) + [m["group"]]
                if len(lane) >= 3:
                    margin = max(lane) - min(lane)
                    verdict = "FASTER" if max(group) < min(lane) - margin else ("SLOWER" if min(group) > max(lane) + margin else "not different")
                    log("   over %d runs: (a) %s, margin = spread %.1f; (b) %s: %s than (a) beyond the margin" % (
                        len(lane), " ".join("%.1f" % v for v in lane), margin, " ".join("%.1f" % v for v in group), verdict))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
