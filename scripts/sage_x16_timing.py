"""Timing of the max reducer with argmax, of its gradient and of a GraphSAGE training step on bf16 features, each against the fp32 form
on the same graph IN THE SAME RUN. Nothing is claimed in advance: the forward gathers half the bytes of B but writes the same 4-byte arg,
and the backward's traffic is almost all arg gathers, which do not shrink.

One process per run. The two forms ALTERNATE: the launches of a figure are taken in rounds — fp32, bf16, fp32, bf16, ... — of per-launch
event pairs after a warm-up of both, and the figure is the median over all rounds, so a drift of the machine falls on both alike.

Per graph and width N:
  (a)  spmm.csr_spmm_max_arg_x16 (bf16) against spmm.csr_spmm_max_arg (fp32) on the same operand, narrowed
  (b)  spmm.csr_spmm_max_backward_x16 against spmm.csr_spmm_max_backward on the same arg and the narrowed grad_out
  (c)  one training step of examples/sage_custom.py's model (one hidden layer of N units, dropout off), a .bfloat16() model on bf16
       features against the fp32 model, for the pool and for the mean aggregator, with the loss after the timed steps
Results are checked before anything is timed: arg identical, C and grad_B bit for bit narrow(fp32 result on the widened operand). Each
run appends `#run` lines; from the third run of the script on, the spread of the fp32 medians ACROSS the runs is the margin bf16 is
judged against (FASTER / SLOWER / not different), as scripts/sage_timing.py does.

  python scripts/sage_x16_timing.py [--graphs com-amazon-sbm,pubmed] [--widths 16,64,128] [--launches 200] [--out profiles/r24/sage_x16/timing.log]
"""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from gat_aggregate_timing import earlier_runs  # noqa: E402
from gat_softmax_timing import load_graph  # noqa: E402
import gespmm_amd  # noqa: E402,F401
from gespmm_amd import _lib, graphs, spmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed")
WIDTHS = (16, 64, 128)
ROUNDS = 4


def alternating_medians_us(fns, launches, warmup=20):
    """{name: median us} of per-launch event pairs, the functions taken in turn in ROUNDS rounds of launches / ROUNDS pairs each."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    per_round = max(1, launches // ROUNDS)
    ev = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            for _ in range(per_round):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3 for k, pairs in ev.items()}


def kernels(rp, ci, csc, K, N, launches):
    dev = rp.device
    M = rp.numel() - 1
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    B16 = (torch.rand(K, N, device=dev, generator=gen) - 0.5).bfloat16()
    g16 = (torch.rand(M, N, device=dev, generator=gen) - 0.5).bfloat16()
    B32, g32 = B16.float(), g16.float()  # the same values: the two forms pick the same winners
    out32, arg32 = torch.empty(M, N, device=dev), torch.empty(M, N, dtype=torch.int32, device=dev)
    out16, arg16 = torch.empty(M, N, device=dev, dtype=torch.bfloat16), torch.empty(M, N, dtype=torch.int32, device=dev)
    gB32, gB16 = torch.empty(K, N, device=dev), torch.empty(K, N, device=dev, dtype=torch.bfloat16)

    fns_fwd = {"fwd_fp32": lambda: spmm.csr_spmm_max_arg(rp, ci, B32, out=out32, arg=arg32),
               "fwd_bf16": lambda: spmm.csr_spmm_max_arg_x16(rp, ci, B16, out=out16, arg=arg16)}
    fns_bwd = {"bwd_fp32": lambda: spmm.csr_spmm_max_backward(colptr, rowind, order, arg32, g32, K, out=gB32),
               "bwd_bf16": lambda: spmm.csr_spmm_max_backward_x16(colptr, rowind, order, arg16, g16, K, out=gB16)}
    for fn in list(fns_fwd.values()) + list(fns_bwd.values()):
        fn()
    res = {"arg": bool(torch.equal(arg16, arg32)),
           "bits": bool(torch.equal(out16.view(torch.int16), out32.bfloat16().view(torch.int16))),
           "bwd_bits": bool(torch.equal(gB16.view(torch.int16), gB32.bfloat16().view(torch.int16)))}
    res.update(alternating_medians_us(fns_fwd, launches))
    res.update(alternating_medians_us(fns_bwd, launches))
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
        fns, kept, first = {}, {}, {}
        for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            torch.manual_seed(0)
            model = ex.GraphSAGE(g, 100, hidden, 16, 1, torch.relu, 0.0, agg).to(dev).to(dt)
            opt = torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=5e-4)
            xs = x.to(dt)

            def step(model=model, opt=opt, xs=xs, tag=tag):
                opt.zero_grad(set_to_none=True)
                kept[tag] = torch.nn.functional.cross_entropy(model(xs).float(), y)
                kept[tag].backward()
                opt.step()

            step()
            first[tag] = float(kept[tag])
            fns[tag] = step
        us = alternating_medians_us(fns, launches, warmup=3)
        out[agg] = {tag: (us[tag], first[tag], float(kept[tag])) for tag in fns}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--widths", default=",".join(str(n) for n in WIDTHS))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "sage_x16", "timing.log"))
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

        log("# %s launches=%d rounds=%d device=%s (us; median of per-launch event pairs, fp32 and bf16 alternating)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, ROUNDS, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (colptr, rowind, order.to(torch.int32))
            del order
            M, nnz = rp.numel() - 1, ci.numel()
            for N in (int(v) for v in args.widths.split(",")):
                m = kernels(rp, ci, csc, K, N, args.launches)
                torch.cuda.empty_cache()
                log("%-15s N=%d M=%d nnz=%d geometry (elements) forward fp32 %s bf16 %s, backward fp32 %s bf16 %s; arg identical: %s; C == "
                    "narrow(fp32 C) bit for bit: %s; grad_B == narrow(fp32 grad_B) bit for bit: %s" % (
                        name, N, M, nnz, _lib.max_arg_route(M, nnz, N), _lib.max_arg_route_x16(M, nnz, N), _lib.max_arg_route(K, nnz, N),
                        _lib.max_arg_route_x16(K, nnz, N), m["arg"], m["bits"], m["bwd_bits"]))
                if not (m["arg"] and m["bits"] and m["bwd_bits"]):
                    raise SystemExit("a result is wrong: nothing timed is worth recording")
                log("   (a) forward   bf16 %.1f   fp32 %.1f   x%.2f" % (m["fwd_bf16"], m["fwd_fp32"], m["fwd_bf16"] / m["fwd_fp32"]))
                log("   (b) backward  bf16 %.1f   fp32 %.1f   x%.2f" % (m["bwd_bf16"], m["bwd_fp32"], m["bwd_bf16"] / m["bwd_fp32"]))
                log("#run %s %d kernels fwd_bf16=%.1f fwd_fp32=%.1f bwd_bf16=%.1f bwd_fp32=%.1f" % (
                    name, N, m["fwd_bf16"], m["fwd_fp32"], m["bwd_bf16"], m["bwd_fp32"]))
                key = (name, str(N), "kernels")
                judge(key, "fwd_bf16", "fwd_fp32", m["fwd_bf16"], m["fwd_fp32"])
                judge(key, "bwd_bf16", "bwd_fp32", m["bwd_bf16"], m["bwd_fp32"])
                steps = training_steps(name, dev, N, min(args.launches, 48))
                torch.cuda.empty_cache()
                for agg in ("pool", "mean"):
                    s = steps[agg]
                    log("   (c) training step, 100 -> %d -> 16, dropout off, %s: bf16 %.1f (loss %.4f -> %.4f)   fp32 %.1f (loss %.4f -> %.4f)   x%.2f" % (
                        (N, agg) + s["bf16"] + s["fp32"] + (s["bf16"][0] / s["fp32"][0],)))
                log("#run %s %d step pool_bf16=%.1f pool_fp32=%.1f mean_bf16=%.1f mean_fp32=%.1f" % (
                    name, N, steps["pool"]["bf16"][0], steps["pool"]["fp32"][0], steps["mean"]["bf16"][0], steps["mean"]["fp32"][0]))
                for agg in ("pool", "mean"):
                    judge((name, str(N), "step"), agg + "_bf16", agg + "_fp32", steps[agg]["bf16"][0], steps[agg]["fp32"][0])
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
