"""Timing of the fused relational weight gradient (spmm.csr_spmm_relational_weight_grad, two kernels) against the composed backward it
replaces — ``stacked_aggregate`` into an [R M, K] array, then one batched matmul — on bf16 features, IN THE SAME RUN. Nothing is claimed
in advance: the kernels save the write and read of the aggregates, and pay with one gather pass per K-slab, a grad_out tile re-read per
(relation, K-slab), 2-byte transposed LDS writes and an fp32 workspace of chunks R N_out K elements.

One process per run. The candidates ALTERNATE (scripts/sage_x16_timing.py). Per graph, typing, R and (K, N_out):
  (a)  op (row_scale = 1 / entries of the stacked row, chunks as the library picks them)   against   the same call with fused=False, with
       the peak memory of each call
  (c)  a two-layer training step of examples/rgcn_custom.py's model (K -> K -> 16) with RGCNConv(fused_weight_grad=True) against the
       layer without the flag (both with the forward's and grad_x's kernel), once per distinct K, with the peak memory of a step
Results are compared before anything is timed (a sanity check: the tests hold the bounds). Each run appends `#run` lines; from the third
run on, the spread of the composition's medians ACROSS runs is the margin the op is judged against (FASTER / SLOWER / not different).

  python scripts/spmm_relational_wgrad_timing.py [--graphs com-amazon-sbm,pubmed,products-sbm] [--rels 4,16] [--shapes 128x128,64x47,256x256]
                                                 [--launches 200] [--out profiles/r29/spmm_relational_wgrad/timing.log]
"""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from gat_aggregate_timing import earlier_runs  # noqa: E402
from gat_softmax_timing import load_graph  # noqa: E402
from sage_x16_timing import alternating_medians_us  # noqa: E402
from spmm_relational_timing import GRAPHS, peak_mib  # noqa: E402
import gespmm_amd  # noqa: E402,F401
from gespmm_amd import _lib, spmm  # noqa: E402

F = torch.nn.functional


def ops(g, R, Kn, K, N_out, launches):
    rp, ci = g[0], g[1]
    dev, dt = rp.device, torch.bfloat16
    M, nnz = (rp.numel() - 1) // R, ci.numel()
    gen = torch.Generator(device=dev).manual_seed(1)
    x = (torch.rand(Kn, K, device=dev, generator=gen) - 0.5).to(dt)
    go = (torch.rand(M, N_out, device=dev, generator=gen) - 0.5).to(dt)
    deg = torch.diff(rp).float()
    inv = torch.where(deg > 0, 1 / deg, torch.zeros_like(deg))
    C = _lib.spmm_relational_wgrad_chunks(R, M, K, N_out)
    assert _lib.spmm_relational_wgrad_route_x16(R, M, Kn, K, N_out, nnz, C, 16) == 1, "the kernel does not serve this shape: nothing to time"
    out = torch.empty(R, N_out, K, device=dev, dtype=dt)
    fns = {"op": lambda: spmm.csr_spmm_relational_weight_grad(rp, ci, None, x, go, R, row_scale=inv, out=out),
           "comp": lambda: spmm.csr_spmm_relational_weight_grad(rp, ci, None, x, go, R, row_scale=inv, out=out, fused=False)}
    got, want = fns["op"]().float().clone(), fns["comp"]().float()
    res = alternating_medians_us(fns, launches)
    res["agree"] = ((got - want).abs() / (2.0**-6 * want.abs() + 2.0**-5 * (1 + want.abs().max()))).max().item()
    res["op_mib"], res["comp_mib"], res["C"] = peak_mib(fns["op"]), peak_mib(fns["comp"]), C
    return res


def training_steps(ex, g, R, n, K, launches):
    dev = g[0].device
    x = (torch.rand(n, K, device=dev) - 0.5).bfloat16()
    y = torch.randint(0, 16, (n,), device=dev)
    fns, kept, peak = {}, {}, {}
    for tag, flag in (("comp", False), ("fused", True)):
        torch.manual_seed(0)
        model = ex.RGCN(g, K, K, 16, R, None, fused=True, fused_weight_grad=flag).to(dev).bfloat16()
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=5e-4)

        def step(model=model, opt=opt, tag=tag):
            opt.zero_grad(set_to_none=True)
            kept[tag] = F.cross_entropy(model(x).float(), y)
            kept[tag].backward()
            opt.step()

        peak[tag] = peak_mib(step)
        fns[tag] = step
    us = alternating_medians_us(fns, launches, warmup=3)
    return {tag: (us[tag], peak[tag], float(kept[tag])) for tag in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--rels", default="4,16")
    ap.add_argument("--shapes", default="128x128,64x47,256x256")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29", "spmm_relational_wgrad", "timing.log"))
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
            M = rp.numel() - 1
            row = torch.repeat_interleave(torch.arange(M, device=dev), torch.diff(rp).long())
            for typing in ("uniform", "skewed"):
                for R in (int(v) for v in args.rels.split(",")):
                    g = ex.stacked_graph(row, ci.long(), ex.edge_types(ci.numel(), R, typing == "skewed", 7, dev), R, M)
                    tag = "%s/%s/R=%d" % (name, typing, R)
                    log("%s M=%d nnz=%d entries per stacked row %.2f" % (tag, M, ci.numel(), ci.numel() / (R * M)))
                    stepped = set()
                    for shape in args.shapes.split(","):
                        K, N_out = (int(v) for v in shape.split("x"))
                        m = ops(g, R, Kn, K, N_out, args.launches)
                        torch.cuda.empty_cache()
                        if not m["agree"] <= 1.0:
                            raise SystemExit("a result is wrong (%.3f): nothing timed is worth recording" % m["agree"])
                        log("   (a) K=%d N_out=%d chunks=%d  op %.1f (peak %.1f MiB)   composition %.1f (peak %.1f MiB)   x%.2f" % (
                            K, N_out, m["C"], m["op"], m["op_mib"], m["comp"], m["comp_mib"], m["op"] / m["comp"]))
                        log("#run %s %s ops op=%.1f comp=%.1f" % (tag, shape, m["op"], m["comp"]))
                        judge((tag, shape, "ops"), "op", "comp", m["op"], m["comp"])
                        if M == Kn and K not in stepped:
                            stepped.add(K)
                            s = training_steps(ex, g, R, M, K, args.launches)
                            torch.cuda.empty_cache()
                            log("   (c) training step %d -> %d -> 16, %d steps each: fused %.1f (peak %.1f MiB, loss %.4f)   composition %.1f (peak %.1f MiB, loss %.4f)   x%.2f" % (
                                (K, K, args.launches) + s["fused"] + s["comp"] + (s["fused"][0] / s["comp"][0],)))
                            log("#run %s K=%d step fused=%.1f comp=%.1f" % (tag, K, s["fused"][0], s["comp"][0]))
                            judge((tag, "K=%d" % K, "step"), "fused", "comp", s["fused"][0], s["comp"][0])
                    del g
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
