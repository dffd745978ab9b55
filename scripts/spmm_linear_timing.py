"""Timing of the fused aggregate-and-linear (spmm.csr_spmm_linear, one kernel) against the compositions it replaces, on bf16 features,
IN THE SAME RUN. Nothing is claimed in advance: the fusion saves the write and read of the [M, K] aggregate and two launches, and pays
with 2-byte stores and a matrix unit fed from one LDS tile per 64 rows.

One process per run. The candidates ALTERNATE (scripts/sage_x16_timing.py: rounds of per-launch event pairs after a warm-up of all, the
figure is the median over all rounds). Per graph and (K, N_out):
  (a)  op        csr_spmm_linear(row_scale = 1 / deg)                           against   the 16-bit product (widen, fused fp32, narrow: what
                                                                                         row_scale costs today) + torch linear
  (b)  op, unweighted, no row_scale                                             against   csr_spmm_no_edge_value + torch linear
  (c)  SAGE-mean forward: csr_spmm_linear(row_scale, root = x, summed bias)     against   today's layer: the two [nnz] weight arrays, the
                                                                                         valued 16-bit product, two linears and an add
  (d)  a two-layer training step of examples/sage_custom.py's model (128 -> K -> 16, dropout off) with and without fused_linear, with
       the peak memory of a step; once per distinct K (N_out plays no part in it), --launches steps per candidate like (a) - (c)
Results are compared before anything is timed (the op against (a)'s composition, elementwise within 2^-6 |x| + 2^-5, a sanity check: the
tests hold the bounds). Each run appends `#run` lines; from the third run on, the spread of the composition's medians ACROSS runs is the
margin the op is judged against (FASTER / SLOWER / not different).

  python scripts/spmm_linear_timing.py [--graphs com-amazon-sbm,pubmed,products-sbm] [--shapes 128x128,256x256,64x47,128x16] [--launches 200]
                                       [--out profiles/r27/spmm_linear/timing.log]
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
import gespmm_amd  # noqa: E402,F401
from gespmm_amd import _lib, graphs, spmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed", "products-sbm")
SHAPES = ("128x128", "256x256", "64x47", "128x16")
F = torch.nn.functional


def ops(rp, ci, csc, Kn, K, N_out, launches):
    dev, dt = rp.device, torch.bfloat16
    M, nnz = rp.numel() - 1, ci.numel()
    gen = torch.Generator(device=dev).manual_seed(1)
    x = (torch.rand(Kn, K, device=dev, generator=gen) - 0.5).to(dt)
    Wn, Wr = ((torch.rand(N_out, K, device=dev, generator=gen) - 0.5).to(dt) for _ in range(2))
    b_self, b_neigh = ((torch.rand(N_out, device=dev, generator=gen) - 0.5).to(dt) for _ in range(2))
    deg = torch.diff(rp).float()
    inv = torch.where(deg > 0, 1 / deg, torch.zeros_like(deg))
    bsum = b_self.float() + b_neigh.float()
    out = torch.empty(M, N_out, device=dev, dtype=dt)
    assert _lib.spmm_linear_route_x16(M, Kn, K, N_out, nnz, 16) == 1, "the kernel does not serve this shape: nothing to time"

    def sage_today():
        w_csr = torch.repeat_interleave(inv, torch.diff(rp), output_size=nnz)
        inv.index_select(0, csc[1])  # (the CSC copy the layer makes for its backward)
        return F.linear(x, Wr, b_self) + F.linear(spmm.csr_spmm(rp, ci, w_csr, x), Wn, b_neigh)

    fns = {"a_op": lambda: spmm.csr_spmm_linear(rp, ci, None, x, Wn, row_scale=inv, out=out),
           "a_comp": lambda: F.linear(spmm.csr_spmm_fused(rp, ci, None, x.float(), row_scale=inv).to(dt), Wn),
           "b_op": lambda: spmm.csr_spmm_linear(rp, ci, None, x, Wn, out=out),
           "b_comp": lambda: F.linear(spmm.csr_spmm_no_edge_value(rp, ci, x), Wn),
           "c_op": lambda: spmm.csr_spmm_linear(rp, ci, None, x, Wn, row_scale=inv, root=x, root_weight=Wr, bias=bsum, out=out),
           "c_comp": sage_today}
    worst = 0.0
    for k in "abc":
        got, want = fns[k + "_op"]().float().clone(), fns[k + "_comp"]().float()
        worst = max(worst, ((got - want).abs() / (2.0**-6 * want.abs() + 2.0**-5)).max().item())
    res = alternating_medians_us(fns, launches)
    res["agree"] = worst
    return res


def training_steps(g, K, launches):
    spec = importlib.util.spec_from_file_location("sage_example", os.path.join(ROOT, "examples", "sage_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    dev, n = g[0].device, g[0].numel() - 1
    x = torch.rand(n, 128, device=dev).bfloat16()
    y = torch.randint(0, 16, (n,), device=dev)
    fns, kept, peak = {}, {}, {}
    for tag, flag in (("plain", False), ("fused", True)):
        torch.manual_seed(0)
        model = ex.GraphSAGE(g, 128, K, 16, 1, torch.relu, 0.0, "mean", flag).to(dev).bfloat16()
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=5e-4)

        def step(model=model, opt=opt, tag=tag):
            opt.zero_grad(set_to_none=True)
            kept[tag] = F.cross_entropy(model(x).float(), y)
            kept[tag].backward()
            opt.step()

        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        peak[tag] = (torch.cuda.max_memory_allocated() - base) / 2.0**20
        fns[tag] = step
    us = alternating_medians_us(fns, launches, warmup=3)
    return {tag: (us[tag], peak[tag], float(kept[tag])) for tag in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "spmm_linear", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        def judge(key, candidate, yardstick, mine, base):
            r = before.get(key, {})
            base_all, mine_all = r.get(yardstick, []) + [base], r.get(candidate, []) + [mine]
            if len(base_all) >= 3:
                margin = max(base_all) - min(base_all)
                verdict = "FASTER" if max(mine_all) < min(base_all) - margin else ("SLOWER" if min(mine_all) > max(base_all) + margin else "not different")
                log("      over %d runs: %s %s, margin = spread %.1f; %s %s: %s beyond the margin" % (
                    len(base_all), yardstick, " ".join("%.1f" % v for v in base_all), margin, candidate, " ".join("%.1f" % v for v in mine_all), verdict))

        log("# %s launches=%d device=%s (us; bf16; median of per-launch event pairs, the candidates alternating)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, Kn = load_graph(name, dev)
            colptr, rowind = graphs.transpose_csr(rp, ci, Kn)
            M, nnz = rp.numel() - 1, ci.numel()
            stepped = set()
            for shape in args.shapes.split(","):
                K, N_out = (int(v) for v in shape.split("x"))
                m = ops(rp, ci, (colptr, rowind), Kn, K, N_out, args.launches)
                torch.cuda.empty_cache()
                log("%-15s K=%d N_out=%d M=%d nnz=%d; op against composition, worst |diff| / (2^-6 |x| + 2^-5) = %.3f" % (name, K, N_out, M, nnz, m["agree"]))
                if not m["agree"] <= 1.0:
                    raise SystemExit("a result is wrong: nothing timed is worth recording")
                for k, what in (("a", "op, row_scale       "), ("b", "op, plain           "), ("c", "SAGE-mean forward   ")):
                    log("   (%s) %s fused %.1f   composition %.1f   x%.2f" % (k, what, m[k + "_op"], m[k + "_comp"], m[k + "_op"] / m[k + "_comp"]))
                log("#run %s %s ops %s" % (name, shape, " ".join("%s=%.1f" % (k, m[k]) for k in sorted(m) if k != "agree")))
                for k in "abc":
                    judge((name, shape, "ops"), k + "_op", k + "_comp", m[k + "_op"], m[k + "_comp"])
                if M == Kn and K not in stepped:  # (the step's model depends on K alone: 128x128 and 128x16 share it, timed once)
                    stepped.add(K)
                    s = training_steps((rp, ci, colptr, rowind, None), K, args.launches)
                    torch.cuda.empty_cache()
                    log("   (d) training step 128 -> %d -> 16, mean, %d steps each: fused %.1f (peak %.1f MiB, loss %.4f)   plain %.1f (peak %.1f MiB, loss %.4f)   x%.2f" % (
                        (K, args.launches) + s["fused"] + s["plain"] + (s["fused"][0] / s["plain"][0],)))
                    log("#run %s K=%d step fused=%.1f plain=%.1f" % (name, K, s["fused"][0], s["plain"][0]))
                    judge((name, "K=%d" % K, "step"), "fused", "plain", s["fused"][0], s["plain"][0])
            del rp, ci, colptr, rowind
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
