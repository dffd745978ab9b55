"""Timing of the 16-bit SDDMM (gespmm_sddmm_{coo,csr}_x16 / gespmm_plan_sddmm_x16, bf16 operands, fp32 out) against the fp32 SDDMM
IN THE SAME RUN.

One process; every figure is the median of per-launch event pairs after a warm-up, as bench.py measures; every column is measured
three times per run.

Columns, per graph and width, for fp32 and for bf16 operands:
  plain COO call | plain CSR call | CSR call through an AUTO plan
with what gespmm_describe_sddmm[_x16] says each launches and the plan's route. The bf16 columns are checked against each other bit
for bit before they are timed (COO == CSR == plan), and against float64 within the suite's tolerance.
Also printed: the bytes an edge gathers, 2 * N * element size + 12, times nnz, for both types.

  python scripts/sddmm_x16_timing.py [--graphs a,b] [--launches 100] [--out profiles/r08/sddmm_x16/timing.log]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gespmm_amd import _lib, graphs, sddmm, spmm  # noqa: E402

# (graph, scale, launches divisor): reddit-like at a quarter of its rows and edges keeps reddit's mean degree (492)
GRAPHS = {"com-amazon-sbm": (1.0, 1), "pubmed": (1.0, 1), "reddit-like": (0.25, 4)}
WIDTHS = (64, 128, 256)
COLUMNS = ("coo", "csr", "plan")


def median_us(fn, launches, warmup=10):
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


def load_csr(name, scale, dev):
    if name == "pubmed":
        g = graphs.load_mtx_as_csr(os.path.join(ROOT, "tests", "golden", "pubmed.mtx"))
        return torch.from_numpy(g["rowptr"]).to(dev), torch.from_numpy(g["colind"]).to(dev), g["M"], g["K"]
    g = graphs.synthetic_graph(name, seed=42, device=dev, scale=scale)
    return g["rowptr"], g["colind"], g["M"], g["K"]


def describe(csr, M, nnz, N, x16):
    d = _lib.describe_sddmm(csr, M, nnz, N, x16=x16)
    return " ".join("%s=%s" % kv for kv in d.items())


def within_float64_tolerance(out, ri, ci, D1, D2, edges=200000):
    pick = torch.randint(0, out.numel(), (min(edges, out.numel()),), device=out.device, generator=torch.Generator(device=out.device).manual_seed(3))
    p = D1[ri[pick].long()].double() * D2[ci[pick].long()].double()
    ref, scale = p.sum(1), p.abs().sum(1)
    return bool(((out[pick].double() - ref).abs() <= 1e-4 * torch.maximum(ref.abs(), scale)).all())


def measure(rp, ci, ri, M, K, N, launches):
    dev = rp.device
    gen = torch.Generator(device=dev).manual_seed(1)
    D1 = torch.rand(M, N, device=dev, generator=gen) - 0.5
    D2 = torch.rand(K, N, device=dev, generator=gen) - 0.5
    H1, H2 = D1.to(torch.bfloat16), D2.to(torch.bfloat16)
    plan = spmm.SpmmPlan(rp, ci, K, N)
    res = {"route": _lib.lib.gespmm_plan_sddmm_route(plan._handle, N)}
    for tag, A, B in (("fp32", D1, D2), ("bf16", H1, H2)):
        fns = {"coo": lambda: sddmm.coo_sddmm(ri, ci, A, B), "csr": lambda: sddmm.csr_sddmm(rp, ci, A, B),
               "plan": lambda: sddmm.csr_sddmm(rp, ci, A, B, plan=plan)}
        outs = [fns[c]() for c in COLUMNS]
        res[tag + "_bits_equal"] = all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
        res[tag + "_f64_ok"] = within_float64_tolerance(outs[1], ri, ci, A, B)
        del outs
        for c in COLUMNS:
            res[tag + "_" + c] = [median_us(fns[c], launches) for _ in range(3)]
    del plan
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "sddmm_x16", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    med = statistics.median
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d device=%s (us; three medians each; bf16 = torch.bfloat16 operands, fp32 out)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, torch.cuda.get_device_name(0)))
        fmt = lambda v: "%s (median %.1f)" % (" ".join("%.1f" % x for x in v), med(v))  # noqa: E731
        for name in args.graphs.split(","):
            scale, div = GRAPHS[name]
            rp, ci, M, K = load_csr(name, scale, dev)
            nnz = ci.numel()
            ri = torch.repeat_interleave(torch.arange(M, device=dev, dtype=torch.int32), (rp[1:] - rp[:-1]).long())
            for N in WIDTHS:
                m = measure(rp, ci, ri, M, K, N, max(10, args.launches // div))
                log("%-15s scale=%.2f N=%d M=%d nnz=%d mean degree %d | plan route %d | bf16: COO == CSR == plan bits %s, float64 tolerance %s" % (
                    name, scale, N, M, nnz, nnz // max(M, 1), m["route"], m["bf16_bits_equal"], m["bf16_f64_ok"]))
                log("   fp32 launches: coo [%s]  csr [%s]" % (describe(False, M, nnz, N, False), describe(True, M, nnz, N, False)))
                log("   bf16 launches: coo [%s]  csr [%s]" % (describe(False, M, nnz, N, True), describe(True, M, nnz, N, True)))
                for c, label in (("coo", "plain COO call"), ("csr", "plain CSR call"), ("plan", "CSR call, AUTO plan")):
                    a, b = m["fp32_" + c], m["bf16_" + c]
                    log("   %-20s fp32 %s | bf16 %s | fp32 / bf16 = x%.2f%s" % (label, fmt(a), fmt(b), med(a) / med(b),
                                                                               "   <-- bf16 SLOWER" if med(b) > med(a) else ""))
                log("   gathered bytes: fp32 %.1f MB, bf16 %.1f MB" % (nnz * (8 * N + 12) / 1e6, nnz * (4 * N + 12) / 1e6))
                log("#run %s %d %s" % (name, N, " ".join("%s_%s=%.1f" % (t, c, med(m[t + "_" + c])) for t in ("fp32", "bf16") for c in COLUMNS)))
            del rp, ci, ri
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
