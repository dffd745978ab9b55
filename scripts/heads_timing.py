"""Timing of the multi-head product (gespmm_csr_spmm_heads_f32 / gespmm_plan_spmm_heads_f32) against what a caller can do without it,
IN THE SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures; every column is
measured three times per run.

Columns, per graph and (H, F):
  (a)  csr_spmm_heads, stateless            (a') ... through a clustered plan (per-call weight permutation included)
  (b)  H strict-order csr_spmm calls on contiguous per-head slices made BEFOREHAND (the slicing is not charged): the baseline
  (c)  csr_spmm_heads with the composition forced (GESPMM_HEADS_ROUTE=composition, read per call)
  (d)  the plain valued product at N = H F with one weight per edge: the floor (same B rows gathered, 4 (H - 1) bytes per edge less)
Bit equality of (a), (a') and (c) is checked. Each run appends a `#run` line per case; from the third run of the script on, the spread of
(b)'s medians ACROSS the runs is the margin (a) is judged against.

  python scripts/heads_timing.py [--graphs a,b] [--launches 200] [--out profiles/r08/heads/timing.log]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gespmm_amd import _lib, graphs, spmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed")
SHAPES = ((8, 8), (8, 16), (4, 32), (8, 64))
COLUMNS = ("heads", "heads_plan", "per_head_calls", "composition", "plain_floor")


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


def measure(rp, ci, M, K, H, F, launches):
    dev = rp.device
    nnz, N = ci.numel(), H * F
    gen = torch.Generator(device=dev).manual_seed(1)
    val = torch.rand(nnz, H, device=dev, generator=gen) - 0.5
    B = torch.rand(K, N, device=dev, generator=gen) - 0.5
    out = torch.empty(M, N, device=dev)
    strict = {"flags": _lib.FLAG_STRICT_ORDER}
    vals = [val[:, h].contiguous() for h in range(H)]
    Bs = [B[:, h * F:(h + 1) * F].contiguous() for h in range(H)]
    outs = [torch.empty(M, F, device=dev) for _ in range(H)]
    plan = spmm.SpmmPlan(rp, ci, K, N, reorder=True)

    def per_head():
        for h in range(H):
            spmm.csr_spmm(rp, ci, vals[h], Bs[h], cfg=strict, out=outs[h])

    fns = {
        "heads": lambda: spmm.csr_spmm_heads(rp, ci, val, B, out=out),
        "heads_plan": lambda: plan.run_heads(val, B, out),
        "per_head_calls": per_head,
        "composition": lambda: spmm.csr_spmm_heads(rp, ci, val, B, out=out),
        "plain_floor": lambda: spmm.csr_spmm(rp, ci, vals[0], B, cfg=strict, out=out),
    }
    per_head()
    want = torch.cat(outs, dim=1).view(torch.int32)
    res = {"route": _lib.heads_route(M, K, H, F, nnz), "plan_route": plan.heads_route(H, F), "clustered": plan.clustered, "bits_equal": True}
    for c in COLUMNS:
        os.environ.pop("GESPMM_HEADS_ROUTE", None)
        if c == "composition":
            os.environ["GESPMM_HEADS_ROUTE"] = "composition"
        if c in ("heads", "heads_plan", "composition"):
            res["bits_equal"] = res["bits_equal"] and torch.equal(fns[c]().view(torch.int32), want)
        res[c] = [median_us(fns[c], launches) for _ in range(3)]
    os.environ.pop("GESPMM_HEADS_ROUTE", None)
    del plan
    torch.cuda.empty_cache()
    return res


def earlier_runs(path):
    """{(graph, H, F): {column: [median of each earlier run]}} from the `#run` lines of the log."""
    runs = {}
    if os.path.exists(path):
        for line in open(path):
            if line.startswith("#run "):
                _, name, h, f, *cols = line.split()
                d = runs.setdefault((name, int(h), int(f)), {})
                for kv in cols:
                    k, v = kv.split("=")
                    d.setdefault(k, []).append(float(v))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "heads", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    med = statistics.median
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d device=%s (us; three medians each)" % (" ".join(sys.argv[1:]) or "(defaults)", args.launches,
                                                                    torch.cuda.get_device_name(0)))
        fmt = lambda v: "%s (median %.1f)" % (" ".join("%.1f" % x for x in v), med(v))  # noqa: E731
        for name in args.graphs.split(","):
            rp, ci, M, K = load_csr(name, dev)
            for H, F in SHAPES:
                m = measure(rp, ci, M, K, H, F, args.launches)
                b = med(m["per_head_calls"])
                log("%-15s H=%d F=%d N=%d M=%d nnz=%d route=%d V,S,W,rpw=%s plan: route=%d clustered=%s bits_equal=%s" % (
                    name, H, F, H * F, M, ci.numel(), m["route"][0], m["route"][1], m["plan_route"], m["clustered"], m["bits_equal"]))
                log("   (a)  csr_spmm_heads               %s   x%.2f of (b)" % (fmt(m["heads"]), b / med(m["heads"])))
                log("   (a') ... through a clustered plan %s   x%.2f of (b)" % (fmt(m["heads_plan"]), b / med(m["heads_plan"])))
                log("   (b)  H strict csr_spmm calls      %s" % fmt(m["per_head_calls"]))
                log("   (c)  forced composition           %s" % fmt(m["composition"]))
                log("   (d)  plain product at N = H F     %s" % fmt(m["plain_floor"]))
                log("#run %s %d %d %s" % (name, H, F, " ".join("%s=%.1f" % (c, med(m[c])) for c in COLUMNS)))
                r = before.get((name, H, F), {})
                base = r.get("per_head_calls", []) + [b]
                mine = r.get("heads", []) + [med(m["heads"])]
                if len(base) >= 3:
                    margin = max(base) - min(base)
                    verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                    log("   over %d runs: (b) %s, margin = spread %.1f; (a) %s: %s beyond the margin" % (
                        len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict))


if __name__ == "__main__":
    main()
