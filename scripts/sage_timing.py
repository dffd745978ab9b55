"""Timing of the max reducer with argmax, of its gradient, and of a GraphSAGE training step, each against its yardstick IN THE SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures.

Per graph and width N:
  (a)  spmm.csr_spmm_max_arg against spmm.csr_spmm_max on the same operands: the price of carrying the position
  (b)  spmm.csr_spmm_max_backward against the unweighted spmm.csr_spmm_no_edge_value on the CSC arrays (strict order): the same gather
       volume, the yardstick for the walk
  (c)  the backward against the torch composition: index_add_ of grad_out at colind[arg] (atomics: not bit-reproducible)
  (d)  one training step of examples/sage_custom.py's model (one hidden layer of N units, dropout off) with the pool aggregator against
       the mean aggregator, with the loss after the timed steps
Results are checked before anything is timed: C against csr_spmm_max bit for bit (random operands hold no zeros), the backward against
the composition within 1e-4 of the sum of magnitudes per word. Each run appends `#run` lines; from the third run of the script on, the
spread of a yardstick's medians ACROSS the runs is the margin its candidate is judged against.

  python scripts/sage_timing.py [--graphs com-amazon-sbm,pubmed] [--widths 16,64,128] [--launches 200] [--out profiles/r16/sage/timing.log]
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

from edge_softmax_timing import median_us  # noqa: E402
from gat_aggregate_timing import earlier_runs  # noqa: E402
from gat_softmax_timing import load_graph  # noqa: E402
import gespmm_amd  # noqa: E402,F401
from gespmm_amd import _lib, graphs, spmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed")
WIDTHS = (16, 64, 128)


def kernels(rp, ci, csc, K, N, launches):
    dev = rp.device
    M = rp.numel() - 1
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    B = torch.rand(K, N, device=dev, generator=gen) - 0.5
    grad = torch.rand(M, N, device=dev, generator=gen) - 0.5
    out, arg = torch.empty(M, N, device=dev), torch.empty(M, N, dtype=torch.int32, device=dev)
    gB, gS = torch.empty(K, N, device=dev), torch.empty(K, N, device=dev)
    strict = {"flags": _lib.FLAG_STRICT_ORDER}
    kept = {}

    def fwd_arg():
        spmm.csr_spmm_max_arg(rp, ci, B, out=out, arg=arg)

    def fwd_max():
        kept["c"] = spmm.csr_spmm_max(rp, ci, B)

    def bwd():
        spmm.csr_spmm_max_backward(colptr, rowind, order, arg, grad, K, out=gB)

    def bwd_sum():
        spmm.csr_spmm_no_edge_value(colptr, rowind, grad, cfg=strict, out=gS)

    cols = torch.arange(N, device=dev)
    ci64 = ci.long()

    def bwd_torch():
        won = arg >= 0
        flat = (ci64[arg.long().clamp(min=0)] * N + cols).masked_select(won)
        kept["g"] = torch.zeros(K * N, device=dev).index_add_(0, flat, grad.masked_select(won)).view(K, N)

    fwd_arg(), fwd_max(), bwd(), bwd_torch()
    res = {"bits": bool(torch.equal(out.view(torch.int32), kept["c"].view(torch.int32)))}
    won = arg >= 0
    flat = (ci64[arg.long().clamp(min=0)] * N + cols).masked_select(won)
    mag = torch.zeros(K * N, dtype=torch.float64, device=dev).index_add_(0, flat, grad.double().masked_select(won).abs())
    ref = torch.zeros(K * N, dtype=torch.float64, device=dev).index_add_(0, flat, grad.double().masked_select(won))
    res["bwd_ok"] = bool(((gB.double().view(-1) - ref).abs() <= 1e-4 * mag).all())
    res["chosen"] = float(won.double().mean())
    del won, flat, mag, ref
    for key, fn in (("max_arg", fwd_arg), ("max", fwd_max), ("backward", bwd), ("sum_csc", bwd_sum), ("torch", bwd_torch)):
        res[key] = median_us(fn, launches)
    kept.clear()
    return res


def training_steps(name, dev, hidden, launches):
    spec = importlib.util.spec_from_file_location("sage_example", os.path.join(ROOT, "examples", "sage_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = (rp, ci, colptr, rowind, order.to(torch.int32))
    x = torch.rand(K, 100, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    out = {}
    for agg in ("pool", "mean"):
        torch.manual_seed(0)
        model = ex.GraphSAGE(g, 100, hidden, 16, 1, torch.relu, 0.0, agg).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=5e-4)
        kept = {}

        def step():
            opt.zero_grad(set_to_none=True)
            kept["loss"] = torch.nn.functional.cross_entropy(model(x), y)
            kept["loss"].backward()
            opt.step()

        step()
        first = float(kept["loss"])
        us = median_us(step, launches, warmup=3)
        out[agg] = (us, first, float(kept["loss"]))
        del model, opt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--widths", default=",".join(str(n) for n in WIDTHS))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "sage", "timing.log"))
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

        log("# %s launches=%d device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (colptr, rowind, order.to(torch.int32))
            del order
            M, nnz = rp.numel() - 1, ci.numel()
            for N in (int(v) for v in args.widths.split(",")):
                m = kernels(rp, ci, csc, K, N, args.launches)
                torch.cuda.empty_cache()
                log("%-15s N=%d M=%d nnz=%d geometry forward %s backward %s; C == csr_spmm_max bit for bit: %s; backward within 1e-4 sum|terms| "
                    "of the float64 composition: %s; %.1f %% of the output words have a winner" % (
                        name, N, M, nnz, _lib.max_arg_route(M, nnz, N), _lib.max_arg_route(K, nnz, N), m["bits"], m["bwd_ok"], 100 * m["chosen"]))
                if not (m["bits"] and m["bwd_ok"]):
                    raise SystemExit("a result is wrong: nothing timed is worth recording")
                log("   (a) forward   max_arg %.1f   csr_spmm_max %.1f   x%.2f" % (m["max_arg"], m["max"], m["max_arg"] / m["max"]))
                log("   (b) backward  walk %.1f   unweighted sum on the CSC arrays %.1f   x%.2f" % (m["backward"], m["sum_csc"], m["backward"] / m["sum_csc"]))
                log("   (c) backward  walk %.1f   torch index_add_ at colind[arg] %.1f   x%.2f" % (m["backward"], m["torch"], m["backward"] / m["torch"]))
                log("#run %s %d kernels max_arg=%.1f max=%.1f backward=%.1f sum_csc=%.1f torch=%.1f" % (
                    name, N, m["max_arg"], m["max"], m["backward"], m["sum_csc"], m["torch"]))
                key = (name, str(N), "kernels")
                judge(key, "max_arg", "max", m["max_arg"], m["max"])
                judge(key, "backward", "sum_csc", m["backward"], m["sum_csc"])
                judge(key, "backward", "torch", m["backward"], m["torch"])
                steps = training_steps(name, dev, N, min(args.launches, 50))
                torch.cuda.empty_cache()
                log("   (d) training step, 100 -> %d -> 16, dropout off: pool %.1f (loss %.4f -> %.4f)   mean %.1f (loss %.4f -> %.4f)   x%.2f" % (
                    (N,) + steps["pool"] + steps["mean"] + (steps["pool"][0] / steps["mean"][0],)))
                log("#run %s %d step pool=%.1f mean=%.1f" % (name, N, steps["pool"][0], steps["mean"][0]))
                judge((name, str(N), "step"), "pool", "mean", steps["pool"][0], steps["mean"][0])
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
