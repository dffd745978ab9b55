"""Timing of the multi-head SDDMM (gespmm_sddmm_csr_heads_f32 / gespmm_plan_sddmm_heads_f32) against what a caller can do without it,
IN THE SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures; every column is
measured three times per run.

Columns, per graph and (H, F):
  (a)  csr_sddmm_heads, stateless           (a') ... through a clustered plan
  (b)  H csr_sddmm calls on contiguous per-head slices made BEFOREHAND (the slicing is not charged): the baseline
  (b') what MultiHeadSPMMFunction.backward does by default: 2 H slicings, H calls and the stack, all charged
  (c)  csr_sddmm_heads with the composition forced (GESPMM_SDDMM_HEADS_ROUTE=composition, read per call)
  (d)  csr_sddmm at width H F: the floor (the same rows gathered, 1 / H of the results written)
  (k)  dense patterns only (mean degree >= 64, where csr_sddmm walks rows): csr_sddmm_heads pinned to the kernel
       (GESPMM_SDDMM_HEADS_ROUTE=kernel). The route rule takes the kernel there since this comparison was first run, so (a) and (k)
       are now the same launch; (k) and (c) stay so that the comparison can be repeated.
Bit equality of (a), (a'), (c) and (k) with (b) is checked. Each run appends a `#run` line per case; from the third run of the script on,
the spread of (b)'s medians ACROSS the runs is the margin (a) is judged against — and, on the dense pattern, (k) against (c).

  python scripts/sddmm_heads_timing.py [--graphs a,b] [--launches 200] [--out profiles/r09/sddmm_heads/timing.log]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gespmm_amd import _lib, graphs, sddmm, spmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed", "dense-standin", "dense-uniform")
SHAPES = ((8, 8), (8, 16), (4, 32), (8, 64))
COLUMNS = ("heads", "heads_plan", "per_head_calls", "backward_today", "composition", "wide_floor", "kernel_pinned")
PIN = "GESPMM_SDDMM_HEADS_ROUTE"


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
    if name == "dense-standin":  # reddit-shaped (mean degree >= 64, skewed) at a size that runs in seconds: 20 000 rows, mean degree ~100
        rng = np.random.RandomState(42)
        M = 20000
        degs = np.minimum(8000, (rng.pareto(1.5, size=M) * 40 + 20).astype(np.int64))
        rowptr = np.zeros(M + 1, dtype=np.int32)
        rowptr[1:] = np.cumsum(degs)
        assert rowptr[-1] // M >= 64
        colind = rng.randint(0, M, size=int(rowptr[-1])).astype(np.int32)
        return torch.from_numpy(rowptr).to(dev), torch.from_numpy(colind).to(dev), M, M
    if name == "dense-uniform":  # no hubs, every row 70 .. 90 entries, and tall enough for the cache-blocked form of csr_sddmm at F = 64
        rng = np.random.RandomState(43)
        M = 76000
        rowptr = np.zeros(M + 1, dtype=np.int32)
        rowptr[1:] = np.cumsum(rng.randint(70, 91, size=M))
        colind = rng.randint(0, M, size=int(rowptr[-1])).astype(np.int32)
        return torch.from_numpy(rowptr).to(dev), torch.from_numpy(colind).to(dev), M, M
    g = graphs.synthetic_graph(name, seed=42, device=dev)
    return g["rowptr"], g["colind"], g["M"], g["K"]


def measure(rp, ci, M, K, H, F, launches):
    dev = rp.device
    nnz = ci.numel()
    gen = torch.Generator(device=dev).manual_seed(1)
    D1 = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    D2 = torch.rand(K, H, F, device=dev, generator=gen) - 0.5
    out = torch.empty(nnz, H, device=dev)
    s1 = [D1[:, h, :].contiguous() for h in range(H)]
    s2 = [D2[:, h, :].contiguous() for h in range(H)]
    W1, W2 = D1.view(M, H * F), D2.view(K, H * F)
    plan = spmm.SpmmPlan(rp, ci, K, H * F, reorder=True)
    desc = _lib.describe_sddmm_heads(True, M, nnz, H, F)
    one = _lib.describe_sddmm(True, M, nnz, F)
    desc["per_head_form"] = one["form"]
    dense = one["form"] in ("row-walk", "blocked")

    def per_head():
        return [sddmm.csr_sddmm(rp, ci, s1[h], s2[h]) for h in range(H)]

    def backward_today():
        return torch.stack([sddmm.csr_sddmm(rp, ci, D1[:, h, :].contiguous(), D2[:, h, :].contiguous()) for h in range(H)], dim=1)

    heads = lambda: sddmm.csr_sddmm_heads(rp, ci, D1, D2, out=out)  # noqa: E731
    fns = {
        "heads": heads,
        "heads_plan": lambda: sddmm.csr_sddmm_heads(rp, ci, D1, D2, out=out, plan=plan),
        "per_head_calls": per_head,
        "backward_today": backward_today,
        "composition": heads,
        "wide_floor": lambda: sddmm.csr_sddmm(rp, ci, W1, W2),
        "kernel_pinned": heads,
    }
    want = torch.stack(per_head(), dim=1).view(torch.int32)
    res = {"describe": desc, "plan_route": plan.sddmm_heads_route(H, F), "clustered": plan.clustered, "bits_equal": True, "dense": dense}
    for c in COLUMNS:
        os.environ.pop(PIN, None)
        if c == "kernel_pinned" and not dense:
            continue
        if c in ("composition", "kernel_pinned"):
            os.environ[PIN] = "composition" if c == "composition" else "kernel"
        if c in ("heads", "heads_plan", "composition", "kernel_pinned"):
            res["bits_equal"] = res["bits_equal"] and torch.equal(fns[c]().view(torch.int32), want)
        res[c] = [median_us(fns[c], launches) for _ in range(3)]
    os.environ.pop(PIN, None)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "sddmm_heads", "timing.log"))
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

        def verdict(mine, base, margin):
            return "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")

        for name in args.graphs.split(","):
            rp, ci, M, K = load_csr(name, dev)
            for H, F in SHAPES:
                m = measure(rp, ci, M, K, H, F, args.launches)
                b = med(m["per_head_calls"])
                log("%-15s H=%d F=%d M=%d nnz=%d %s plan: route=%d clustered=%s bits_equal=%s" % (
                    name, H, F, M, ci.numel(), " ".join("%s=%s" % kv for kv in m["describe"].items()), m["plan_route"], m["clustered"],
                    m["bits_equal"]))
                log("   (a)  csr_sddmm_heads                %s   x%.2f of (b)" % (fmt(m["heads"]), b / med(m["heads"])))
                log("   (a') ... through a clustered plan   %s   x%.2f of (b)" % (fmt(m["heads_plan"]), b / med(m["heads_plan"])))
                log("   (b)  H csr_sddmm calls, pre-sliced  %s" % fmt(m["per_head_calls"]))
                log("   (b') slices + calls + stack         %s   (a) is x%.2f of it" % (fmt(m["backward_today"]), med(m["backward_today"]) / med(m["heads"])))
                log("   (c)  forced composition             %s" % fmt(m["composition"]))
                log("   (d)  csr_sddmm at width H F         %s" % fmt(m["wide_floor"]))
                if m["dense"]:
                    log("   (k)  pinned to the kernel           %s   x%.2f of (c)" % (fmt(m["kernel_pinned"]), med(m["composition"]) / med(m["kernel_pinned"])))
                log("#run %s %d %d %s" % (name, H, F, " ".join("%s=%.1f" % (c, med(m[c])) for c in COLUMNS if c in m)))
                r = before.get((name, H, F), {})
                base = r.get("per_head_calls", []) + [b]
                if len(base) >= 3:
                    margin = max(base) - min(base)
                    mine = r.get("heads", []) + [med(m["heads"])]
                    log("   over %d runs: (b) %s, margin = spread %.1f; (a) %s: %s than (b) beyond the margin" % (
                        len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict(mine, base, margin)))
                    if m["dense"]:
                        comp = r.get("composition", []) + [med(m["composition"])]
                        pinned = r.get("kernel_pinned", []) + [med(m["kernel_pinned"])]
                        log("   ... (k) %s against (c) %s: the kernel is %s than the composition beyond the margin" % (
                            " ".join("%.1f" % v for v in pinned), " ".join("%.1f" % v for v in comp), verdict(pinned, comp, margin)))


if __name__ == "__main__":
    main()
