"""Timing of the relational aggregate-and-linear on fp32 features (spmm.csr_spmm_relational_linear on fp32 tensors: one kernel on
v_mfma_f32_32x32x2_f32) against the composition it replaces (the same call with fused=False: the fp32 product on the stacked CSR, the
regrouping copy and one matmul), IN THE SAME RUN. Nothing is claimed in advance: the fusion saves the write and read of the [R M, K]
fp32 aggregates and the regrouping copy, and pays with the fp32 rate of the matrix unit, an eighth of the 16-bit one.

One process per run; the candidates ALTERNATE (scripts/sage_x16_timing.py), the figure is the median of per-launch event pairs. Per
graph, R and (K, N_out): the op (row_scale = 1 / entries of the stacked row, root = x, bias) against fused=False, and the forward's peak
memory above inputs and output for both. Results are compared before anything is timed (elementwise within 2^-12 |x| + 2^-10, a sanity
check: the tests hold the bounds). Each run appends `#run` lines; from the third run on, the spread of the composition's medians ACROSS
runs is the margin the op is judged against (FASTER / SLOWER / not different).

  python scripts/spmm_relational_f32_timing.py [--graphs pubmed,com-amazon-sbm] [--rels 4,16] [--shapes 128x128,64x48,256x256]
                                               [--launches 200] [--out profiles/r30/spmm_relational_f32/timing.log]
"""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from gat_aggregate_timing import earlier_runs  # noqa: E402
from gat_softmax_timing import load_graph  # noqa: E402
from sage_x16_timing import alternating_medians_us  # noqa: E402
from spmm_relational_timing import peak_mib  # noqa: E402
import gespmm_amd  # noqa: E402,F401
from gespmm_amd import _lib, spmm  # noqa: E402


def ops(g, R, Kn, K, N_out, launches):
    rp, ci = g[0], g[1]
    dev = rp.device
    M, nnz = (rp.numel() - 1) // R, ci.numel()
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(Kn, K, device=dev, generator=gen) - 0.5
    W = torch.rand(R, N_out, K, device=dev, generator=gen) - 0.5
    W0 = torch.rand(N_out, K, device=dev, generator=gen) - 0.5
    bias = torch.rand(N_out, device=dev, generator=gen) - 0.5
    deg = torch.diff(rp).float()
    inv = torch.where(deg > 0, 1 / deg, torch.zeros_like(deg))
    out = torch.empty(M, N_out, device=dev)
    assert _lib.spmm_relational_route_f32(R, M, Kn, K, N_out, nnz, 16) == 1, "the kernel does not serve this shape: nothing to time"
    fns = {"op": lambda: spmm.csr_spmm_relational_linear(rp, ci, None, x, W, row_scale=inv, root=x, root_weight=W0, bias=bias, out=out),
           "comp": lambda: spmm.csr_spmm_relational_linear(rp, ci, None, x, W, row_scale=inv, root=x, root_weight=W0, bias=bias, out=out, fused=False)}
    got, want = fns["op"]().clone(), fns["comp"]()
    res = alternating_medians_us(fns, launches)
    res["agree"] = ((got - want).abs() / (2.0**-12 * want.abs() + 2.0**-10)).max().item()
    res["op_mib"], res["comp_mib"] = peak_mib(fns["op"]), peak_mib(fns["comp"])  # (out is preallocated: the peak is the transient alone)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="pubmed,com-amazon-sbm")
    ap.add_argument("--rels", default="4,16")
    ap.add_argument("--shapes", default="128x128,64x48,256x256")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30", "spmm_relational_f32", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    spec = importlib.util.spec_from_file_location("rgcn_example", os.path.join(ROOT, "examples", "rgcn_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d device=%s (us; fp32; median of per-launch event pairs, the candidates alternating)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, Kn = load_graph(name, dev)
            M = rp.numel() - 1
            row = torch.repeat_interleave(torch.arange(M, device=dev), torch.diff(rp).long())
            for R in (int(v) for v in args.rels.split(",")):
                g = ex.stacked_graph(row, ci.long(), ex.edge_types(ci.numel(), R, False, 7, dev), R, M)
                tag = "%s/R=%d" % (name, R)
                log("%s M=%d nnz=%d entries per stacked row %.2f, empty stacked rows %.0f %%" % (
                    tag, M, ci.numel(), ci.numel() / (R * M), 100.0 * (torch.diff(g[0]) == 0).float().mean().item()))
                for shape in args.shapes.split(","):
                    K, N_out = (int(v) for v in shape.split("x"))
                    m = ops(g, R, Kn, K, N_out, args.launches)
                    torch.cuda.empty_cache()
                    if not m["agree"] <= 1.0:
                        raise SystemExit("a result is wrong (%.3f): nothing timed is worth recording" % m["agree"])
                    log("   K=%d N_out=%d  op %.1f (peak %.1f MiB)   composition %.1f (peak %.1f MiB)   x%.2f" % (
                        K, N_out, m["op"], m["op_mib"], m["comp"], m["comp_mib"], m["op"] / m["comp"]))
                    log("#run %s %s ops op=%.1f comp=%.1f" % (tag, shape, m["op"], m["comp"]))
                    r = before.get((tag, shape, "ops"), {})
                    base_all, mine_all = r.get("comp", []) + [m["comp"]], r.get("op", []) + [m["op"]]
                    if len(base_all) >= 3:
                        margin = max(base_all) - min(base_all)
                        verdict = "FASTER" if max(mine_all) < min(base_all) - margin else ("SLOWER" if min(mine_all) > max(base_all) + margin else "not different")
                        log("      over %d runs: comp %s, margin = spread %.1f; op %s: %s beyond the margin" % (
                            len(base_all), " ".join("%.1f" % v for v in base_all), margin, " ".join("%.1f" % v for v in mine_all), verdict))
                del g
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
