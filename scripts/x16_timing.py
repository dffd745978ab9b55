"""Timing of the 16-bit product (gespmm_csr_spmm_x16 / gespmm_plan_spmm_x16, bf16) against the fp32 product IN THE SAME RUN.

One process; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures; every column is
measured three times per run.

Columns, per graph and width:
  fp32 plain call | fp32 through an AUTO plan | bf16 plain call | bf16 plan, 16-bit kernel | bf16 plan, composition (widen, fp32 route, narrow)
The two pinned bf16 plan columns set GESPMM_X16_ROUTE around their launches (the library reads it per call); a third shows what the
policy chooses. Each run appends a `#run` line per case; from the third run of the script on, the spread of the fp32 plain call's
medians ACROSS the runs is the margin the bf16 plain call is judged against.
Also printed: the algorithmic bytes 4 (M + 1) + 8 nnz + 2 (K + M) N of the bf16 product and the fraction of 8 TB/s they amount to.

  python scripts/x16_timing.py [--graphs a,b] [--launches 200] [--out profiles/r07/x16/timing.log]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gespmm_amd import _lib, graphs, spmm  # noqa: E402

CASES = [("com-amazon-sbm", 128), ("com-amazon-like", 128), ("pubmed", 128), ("products-sbm", 128), ("com-amazon-sbm", 32), ("com-amazon-sbm", 64),
         ("com-amazon-sbm", 256)]


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


def load_csr(name, dev):
    if name == "pubmed":
        g = graphs.load_mtx_as_csr(os.path.join(ROOT, "tests", "golden", "pubmed.mtx"))
        return torch.from_numpy(g["rowptr"]).to(dev), torch.from_numpy(g["colind"]).to(dev), g["M"], g["K"]
    g = graphs.synthetic_graph(name, seed=42, device=dev)
    return g["rowptr"], g["colind"], g["M"], g["K"]


def measure(name, N, launches):
    """{column: [three medians]} plus the facts of the case. The two pinned plan columns set GESPMM_X16_ROUTE around their launches
    (the library reads it per call)."""
    dev = torch.device("cuda")
    rp, ci, M, K = load_csr(name, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    B = torch.rand(K, N, device=dev, generator=gen) - 0.5
    B16 = B.to(torch.bfloat16)
    out = torch.empty(M, N, device=dev)
    out16 = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    plan = spmm.SpmmPlan(rp, ci, K, N)
    fns = {
        "fp32_plain": lambda: spmm.csr_spmm_no_edge_value(rp, ci, B, out=out),
        "fp32_plan": lambda: plan.run(None, B, out),
        "bf16_plain": lambda: spmm.csr_spmm_no_edge_value(rp, ci, B16, out=out16),
        "bf16_plan_kernel": lambda: plan.run(None, B16, out16),
        "bf16_plan_composition": lambda: plan.run(None, B16, out16),
        "bf16_plan": lambda: plan.run(None, B16, out16),
    }
    pins = {"bf16_plan_kernel": "kernel", "bf16_plan_composition": "composition"}
    want = spmm.csr_spmm_no_edge_value(rp, ci, B16.float()).to(torch.bfloat16).view(torch.int16)
    res = {"M": M, "K": K, "nnz": ci.numel(), "describe": plan.describe().split("|")[-1].strip()[:100], "bits_equal": True, "route": {}}
    for c in COLUMNS:
        os.environ.pop("GESPMM_X16_ROUTE", None)
        if c in pins:
            os.environ["GESPMM_X16_ROUTE"] = pins[c]
        if c.startswith("bf16"):
            res["bits_equal"] = res["bits_equal"] and torch.equal(fns[c]().view(torch.int16), want)
        if c.startswith("bf16_plan"):
            res["route"][c] = plan.x16_route(N)
        elif c == "bf16_plain":
            res["route"][c] = _lib.lib.gespmm_x16_route(M, K, N, ci.numel(), _lib.VARIANT_AUTO, 16, 16)
        res[c] = [median_us(fns[c], launches) for _ in range(3)]
    os.environ.pop("GESPMM_X16_ROUTE", None)
    del plan
    torch.cuda.empty_cache()
    return res


COLUMNS = ("fp32_plain", "fp32_plan", "bf16_plain", "bf16_plan_kernel", "bf16_plan_composition", "bf16_plan")


def earlier_runs(path):
    """{(graph, N): {column: [median of each earlier run]}} from the `#run` lines of the log."""
    runs = {}
    if os.path.exists(path):
        for line in open(path):
            if line.startswith("#run "):
                _, name, n, *cols = line.split()
                d = runs.setdefault((name, int(n)), {})
                for kv in cols:
                    k, v = kv.split("=")
                    d.setdefault(k, []).append(float(v))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="com-amazon-sbm,com-amazon-like,pubmed,products-sbm")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "x16", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    med = statistics.median
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d device=%s (us; three medians each; bf16 = torch.bfloat16)" % (" ".join(sys.argv[1:]) or "(defaults)", args.launches,
                                                                                           torch.cuda.get_device_name(0)))
        fmt = lambda v: "%s (median %.1f)" % (" ".join("%.1f" % x for x in v), med(v))  # noqa: E731
        for name, N in CASES:
            if name not in args.graphs.split(","):
                continue
            m = measure(name, N, args.launches)
            algo = 4 * (m["M"] + 1) + 8 * m["nnz"] + 2 * (m["K"] + m["M"]) * N
            log("%-15s N=%d M=%d nnz=%d bits_equal=%s | fp32 plan: %s" % (name, N, m["M"], m["nnz"], m["bits_equal"], m["describe"]))
            log("   fp32 plain call            %s" % fmt(m["fp32_plain"]))
            log("   fp32 AUTO plan             %s" % fmt(m["fp32_plan"]))
            log("   bf16 plain call            %s   (route %d)   x%.2f of the fp32 plain call" % (fmt(m["bf16_plain"]), m["route"]["bf16_plain"],
                                                                                                 med(m["fp32_plain"]) / med(m["bf16_plain"])))
            log("   bf16 plan, 16-bit kernel   %s   (route %d)" % (fmt(m["bf16_plan_kernel"]), m["route"]["bf16_plan_kernel"]))
            log("   bf16 plan, composition     %s   (route %d)" % (fmt(m["bf16_plan_composition"]), m["route"]["bf16_plan_composition"]))
            log("   bf16 plan, policy's choice %s   (route %d)   x%.2f of the fp32 plan" % (fmt(m["bf16_plan"]), m["route"]["bf16_plan"],
                                                                                          med(m["fp32_plan"]) / med(m["bf16_plan"])))
            best = min(med(m["bf16_plain"]), med(m["bf16_plan"]))
            log("   algorithmic bytes (bf16) %.1f MB; best bf16 column moves them at %.2f TB/s = %.0f %% of 8 TB/s" % (
                algo / 1e6, algo / best / 1e6, 100 * algo / best / 1e6 / 8))
            log("#run %s %d %s" % (name, N, " ".join("%s=%.1f" % (c, med(m[c])) for c in COLUMNS)))
            # acceptance across RUNS of the script: the spread of the fp32 plain call's medians over the runs so far is the margin
            r = before.get((name, N), {})
            fp = r.get("fp32_plain", []) + [med(m["fp32_plain"])]
            bf = r.get("bf16_plain", []) + [med(m["bf16_plain"])]
            if len(fp) >= 3:
                margin = max(fp) - min(fp)
                verdict = "FASTER" if max(bf) < min(fp) - margin else ("SLOWER" if min(bf) > max(fp) + margin else "not different")
                log("   over %d runs: fp32 plain %s, margin = spread %.1f; bf16 plain %s: %s beyond the margin" % (
                    len(fp), " ".join("%.1f" % v for v in fp), margin, " ".join("%.1f" % v for v in bf), verdict))


if __name__ == "__main__":
    main()
