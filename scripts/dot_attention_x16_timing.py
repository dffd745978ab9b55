"""Timing of the fused dot-product attention on bf16 q, k and v (gespmm_dot_attention_x16 and its two backward passes) against the fp32
fused entry points IN THE SAME RUN, on the same values: the fp32 operands are the bf16 ones, widened.

One process; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures. The two forms take
turns, pass by pass, and every pass is measured in `--rounds` rounds (default 3): the spread of the fp32 medians ACROSS the rounds is
the margin the bf16 ones are judged against — FASTER / SLOWER only when every bf16 median lies beyond every fp32 one by more than it.

Columns, per graph and (H, F); scale 1 / sqrt(F); results into preallocated tensors:
  x16   attention.dot_attention_x16 (forward), dot_attention_backward_q_x16 (row pass), dot_attention_backward_kv_x16 (column pass)
  f32   attention.dot_attention / _backward_q / _backward_kv on q.float(), k.float(), v.float(), grad_out.float(); the row pass is fed
        the widened 16-bit out, the column pass that delta
Before anything is timed the bf16 results are checked against the fp32 ones where both describe calls answer the same (V, W): stats
and delta bit for bit, out, grad_q, grad_k and grad_v against the fp32 results narrowed by torch bit for bit.

  python scripts/dot_attention_x16_timing.py [--graphs com-amazon-sbm,pubmed] [--cases 1x64,4x16,8x8,8x32] [--launches 200] [--rounds 3]
                                             [--out profiles/r23/dot_attention_x16/timing.log]
  python scripts/dot_attention_x16_timing.py --step [--graphs com-amazon-sbm,pubmed]
        time and peak device memory of one training step of examples/transformer_custom.py's two-layer model: --fused in fp32, --fused
        as a .bfloat16() model on bf16 features, and the bf16 model with fused=False — the step's time in `--rounds` rounds, judged
        against the spread of the fp32 fused medians (bf16 fused against fp32 fused) and of the bf16 fused=False medians
"""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from edge_softmax_timing import median_us  # noqa: E402
from gat_aggregate_timing import CASES  # noqa: E402
from gat_softmax_timing import load_graph  # noqa: E402
from gespmm_amd import _lib, attention, graphs  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed")
PASSES = (("fwd", "forward"), ("row", "row pass (delta, grad_q)"), ("col", "column pass (grad_k, grad_v)"))


def _bits_equal(a, b):
    view = torch.int16 if a.element_size() == 2 else torch.int32
    return a.dtype == b.dtype and bool((a.contiguous().view(view) == b.contiguous().view(view)).all())


def verdict(mine, base):
    """`mine` against `base` (medians of the rounds, us): beyond the spread of `base` or not."""
    margin = max(base) - min(base)
    if max(mine) < min(base) - margin:
        return margin, "faster"
    if min(mine) > max(base) + margin:
        return margin, "SLOWER"
    return margin, "not different"


def measure(rp, ci, csc, K, H, F, launches, rounds):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    bf = torch.bfloat16
    q = ((torch.rand(M, H, F, device=dev, generator=gen) - 0.5) * 2).to(bf)
    k = ((torch.rand(K, H, F, device=dev, generator=gen) - 0.5) * 2).to(bf)
    v = ((torch.rand(K, H, F, device=dev, generator=gen) - 0.5) * 2).to(bf)
    go = (torch.rand(M, H, F, device=dev, generator=gen) - 0.5).to(bf)
    ops = {"x16": (q, k, v, go, bf, attention.dot_attention_x16, attention.dot_attention_backward_q_x16,
                   attention.dot_attention_backward_kv_x16),
           "f32": (q.float(), k.float(), v.float(), go.float(), torch.float32, attention.dot_attention, attention.dot_attention_backward_q,
                   attention.dot_attention_backward_kv)}
    fns, outs = {}, {}
    for key in ("x16", "f32"):  # (x16 first: the fp32 row pass reads its out, widened)
        a, b, c, g, dt, fwd, row, col = ops[key]
        out, gq, gk, gv = (torch.empty(s, device=dev, dtype=dt) for s in ((M, H, F), (M, H, F), (K, H, F), (K, H, F)))
        stats, delta = torch.empty(M, H, 2, device=dev), torch.empty(M, H, device=dev)
        outs[key] = {"out": out, "stats": stats, "delta": delta, "grad_q": gq, "grad_k": gk, "grad_v": gv}
        fed = out  # the row pass's `out`
        if key == "f32":
            fed = torch.empty_like(out)
        fns[key] = {
            "fwd": lambda a=a, b=b, c=c, fwd=fwd, out=out, stats=stats: fwd(rp, ci, a, b, c, out=out, stats=stats),
            "row": lambda a=a, b=b, c=c, g=g, row=row, fed=fed, stats=stats, delta=delta, gq=gq:
                row(rp, ci, a, b, c, stats, fed, g, results=(delta, gq)),
            "col": lambda a=a, b=b, c=c, g=g, col=col, stats=stats, delta=delta, gk=gk, gv=gv:
                col(colptr, rowind, a, b, c, stats, delta, g, results=(gk, gv)),
        }
        fns[key]["fwd"]()
        if key == "f32":
            fed.copy_(outs["x16"]["out"].float())
        fns[key]["row"]()
        fns[key]["col"]()
    torch.cuda.synchronize()
    d16, d32 = _lib.describe_dot_attention(M, K, H, F, nnz, x16=True), _lib.describe_dot_attention(M, K, H, F, nnz)
    same = (d16["V"], d16["W"]) == (d32["V"], d32["W"])
    o16, o32 = outs["x16"], outs["f32"]
    ok = same and all(_bits_equal(o16[n], o32[n]) for n in ("stats", "delta")) and \
        all(_bits_equal(o16[n], o32[n].to(bf)) for n in ("out", "grad_q", "grad_k", "grad_v"))
    res = {"M": M, "nnz": nnz, "ok": ok, "same": same, "d16": d16, "d32": d32}
    if ok:
        for key in ("x16", "f32"):
            for d, _ in PASSES:
                res[key + "_" + d] = []
        for _ in range(rounds):
            for d, _ in PASSES:  # the two columns alternate, pass by pass
                for key in ("x16", "f32"):
                    res[key + "_" + d].append(median_us(fns[key][d], launches))
    return res


def training_step(name, dev, launches, rounds):
    """Median time and peak allocated memory (above the graph and the features) of one training step — forward, loss, backward, Adam —
    of examples/transformer_custom.py's Net (64 input features, 8 heads x 8, then 1 head, 16 classes; dropout off): the fused attention
    in fp32, the fused attention as a .bfloat16() model on bf16 features, and the bf16 model with fused=False."""
    spec = importlib.util.spec_from_file_location("transformer_example", os.path.join(ROOT, "examples", "transformer_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x32 = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    nnz = ci.numel()
    steps, out = {}, {}
    for key, dt, fused in (("fp32 fused", torch.float32, True), ("bf16 fused", torch.bfloat16, True), ("bf16 fused=False", torch.bfloat16, False)):
        torch.manual_seed(0)
        model = ex.Net(64, 16, 8, 8, dropout=0.0, fused=fused).to(dev).to(dt)
        x = x32.to(dt)
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)

        def step(model=model, opt=opt, x=x):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.nll_loss(model(x, g).float(), y)
            loss.backward()
            opt.step()
            return loss

        step()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss = float(step().detach())
        torch.cuda.synchronize()
        steps[key] = step
        out[key] = {"peak": torch.cuda.max_memory_allocated() - base, "loss": loss, "us": []}
    for _ in range(rounds):  # the three models take turns
        for key, step in steps.items():
            out[key]["us"].append(median_us(step, launches, warmup=3))
    return nnz, K, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "dot_attention_x16", "timing.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: a time taken anywhere else says nothing")
    if args.rounds < 2:
        raise SystemExit("--rounds must be at least 2: the margin is the spread across the rounds")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda")
    names = args.graphs.split(",")
    fmt = lambda vs: " ".join("%.1f" % t for t in vs)  # noqa: E731
    mid = lambda vs: sorted(vs)[len(vs) // 2]  # noqa: E731
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if args.step:
            for name in names:
                nnz, n, res = training_step(name, dev, min(args.launches, 50), args.rounds)
                log("#step %s nodes=%d nnz=%d (self-loops not added) two-layer model 64 -> 8 x 8 -> 16, one training step, median us of each "
                    "round and peak allocated above the graph and the features; one [nnz, 8] fp32 array is %.1f MB" % (
                        name, n, nnz, nnz * 8 * 4 / 2 ** 20))
                for key, r in res.items():
                    log("   %-17s %s us   peak %.1f MB   (loss %.6f)" % (key, fmt(r["us"]), r["peak"] / 2 ** 20, r["loss"]))
                mine = res["bf16 fused"]["us"]
                for other in ("fp32 fused", "bf16 fused=False"):
                    base = res[other]["us"]
                    margin, word = verdict(mine, base)
                    log("   bf16 fused against %s: x%.2f (%s / bf16 fused), margin = spread of %s %.1f us: %s beyond the margin; peak x%.2f" % (
                        other, mid(base) / mid(mine), other, other, margin, word, res[other]["peak"] / res["bf16 fused"]["peak"]))
            return
        log("# %s launches=%d rounds=%d device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, args.rounds, torch.cuda.get_device_name(0)))
        for name in names:
            rp, ci, K = load_graph(name, dev)
            csc = graphs.transpose_csr(rp, ci, K)
            for case in args.cases.split(","):
                H, F = (int(t) for t in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches, args.rounds)
                torch.cuda.empty_cache()
                log("%-15s H=%d F=%d M=%d nnz=%d x16 V=%d W=%d, f32 V=%d W=%d%s" % (
                    name, H, F, m["M"], m["nnz"], m["d16"]["V"], m["d16"]["W"], m["d32"]["V"], m["d32"]["W"],
                    " (same V, W: stats, delta bit-equal; out, grad_q, grad_k, grad_v the fp32 ones narrowed once)" if m["ok"] else ""))
                if not m["ok"]:
                    raise SystemExit("the 16-bit results are not the fp32 ones rounded once: nothing timed is worth recording")
                for d, what in PASSES:
                    t16, t32 = m["x16_" + d], m["f32_" + d]
                    margin, word = verdict(t16, t32)
                    log("   %-30s x16 %s   f32 %s   f32 / x16 x%.2f   margin = spread of f32 %.1f: x16 %s than f32 beyond the margin" % (
                        what, fmt(t16), fmt(t32), mid(t32) / mid(t16), margin, word))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
