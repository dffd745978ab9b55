"""Timing of the fused dot-product attention (gespmm_dot_attention_f32 + its two backward launches) against the composition of the
library's own ops, IN THE SAME RUN.

One process per run; every figure is the median of per-launch event pairs after a warm-up, as bench.py measures (--launches of them;
where one launch takes more than 5 ms, a quarter as many).

Columns, per graph and (H, F); scale 1 / sqrt(F):
  (a)  forward: attention.dot_attention into preallocated out and stats; backward: dot_attention_backward_q (delta, grad_q), then
       dot_attention_backward_kv (grad_k, grad_v) — three launches, nothing of size nnz
  (b)  forward: sddmm.csr_sddmm_heads -> * scale -> softmax.edge_softmax -> spmm.csr_spmm_heads; backward: csr_sddmm_heads(grad_out, v),
       csr_spmm_heads on the CSC arrays with alpha[csc_order] (grad_v), edge_softmax_backward -> * scale, csr_spmm_heads (grad_q),
       csr_spmm_heads on the CSC arrays with grad_score[csc_order] (grad_k) — what TransformerConv(fused=False) launches
(a) and (b) are both checked against float64 on 65 sampled rows and 65 sampled columns (the last ones included) before anything is
timed (1e-3 of the largest sampled value); (a) outside that ends the run, (b) outside it is said in the log and its time recorded for
scale only. (b) is not run where its
[nnz, H] arrays would pass --b-limit-gb (six of them counted: score, alpha, their gradients, alpha and grad_score in CSC order); the
size it would need is printed instead. Each run appends a `#run` line per case; from the third run of the script on, the spread of (b)'s
medians ACROSS the runs is the margin (a) is judged against.

  python scripts/dot_attention_timing.py [--graphs a,b] [--cases 1x64,4x16,8x8,8x32,4x64] [--launches 200] [--out profiles/r17/dot_attention/timing.log]
  python scripts/dot_attention_timing.py --step [--graphs pubmed,com-amazon-sbm]     time and peak device memory of one training step of
                                                                                      examples/transformer_custom.py's two-layer model,
                                                                                      --fused and the composition
"""
import argparse
import importlib.util
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from edge_softmax_timing import median_us  # noqa: E402
from gat_aggregate_timing import earlier_runs  # noqa: E402
from gat_softmax_timing import GRAPHS, load_graph  # noqa: E402
import gespmm_amd  # noqa: E402,F401
from gespmm_amd import attention, graphs, sddmm, softmax, spmm  # noqa: E402

CASES = "1x64,4x16,8x8,8x32,4x64"


def timed(fn, launches):
    """median_us with a quarter of the launches where a launch takes more than 5 ms."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    slow = a.elapsed_time(b) > 5.0
    return median_us(fn, max(10, launches // 4) if slow else launches, warmup=3 if slow else 20)


def sampled_errors(rp, ci, colptr, rowind, q, k, v, go, stats, delta, scale, results, samples=64):
    """max |x - float64| / max |float64| over sampled segments for x = (out, grad_q, grad_k, grad_v); the float64 backward reads the
    fused forward's stats and delta (both paths normalise by the same row sums to rounding)."""
    out, gq, gk, gv = results
    sc = float(torch.tensor(scale, dtype=torch.float32))
    err, top = [0.0] * 4, [1e-30] * 4

    def note(i, x, ref):
        err[i] = max(err[i], float((x.double() - ref).abs().max()))
        top[i] = max(top[i], float(ref.abs().max()))

    M, K = rp.numel() - 1, colptr.numel() - 1
    for r in sorted(set(torch.linspace(0, M - 1, samples).long().tolist() + [M - 1])):
        c = ci[int(rp[r]):int(rp[r + 1])].long()
        if c.numel() == 0:
            continue
        a = torch.softmax((q[r].double() * k[c].double()).sum(-1) * sc, dim=0)
        o = (a.unsqueeze(-1) * v[c].double()).sum(0)
        g = (go[r].double() * v[c].double()).sum(-1)
        ds = a * (g - (go[r].double() * o).sum(-1))
        note(0, out[r], o)
        note(1, gq[r], sc * (ds.unsqueeze(-1) * k[c].double()).sum(0))
    for c in sorted(set(torch.linspace(0, K - 1, samples).long().tolist() + [K - 1])):
        r = rowind[int(colptr[c]):int(colptr[c + 1])].long()
        if r.numel() == 0:
            continue
        a = torch.exp((q[r].double() * k[c].double()).sum(-1) * sc - stats[r, :, 0].double()) / stats[r, :, 1].double()
        ds = a * ((go[r].double() * v[c].double()).sum(-1) - delta[r].double())
        note(2, gk[c], sc * (ds.unsqueeze(-1) * q[r].double()).sum(0))
        note(3, gv[c], (a.unsqueeze(-1) * go[r].double()).sum(0))
    return [e / t for e, t in zip(err, top)]


def measure(rp, ci, csc, K, H, F, launches, b_limit):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind, order = csc
    scale = 1.0 / math.sqrt(F)
    gen = torch.Generator(device=dev).manual_seed(1)
    q = (torch.rand(M, H, F, device=dev, generator=gen) - 0.5) * 2
    k = (torch.rand(K, H, F, device=dev, generator=gen) - 0.5) * 2
    v = torch.rand(K, H, F, device=dev, generator=gen) - 0.5
    go = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    out, stats, delta = torch.empty(M, H, F, device=dev), torch.empty(M, H, 2, device=dev), torch.empty(M, H, device=dev)
    gq, gk, gv = torch.empty(M, H, F, device=dev), torch.empty(K, H, F, device=dev), torch.empty(K, H, F, device=dev)

    def a_fwd():
        attention.dot_attention(rp, ci, q, k, v, scale=scale, out=out, stats=stats)

    def a_bq():
        attention.dot_attention_backward_q(rp, ci, q, k, v, stats, out, go, scale=scale, results=(delta, gq))

    def a_bkv():
        attention.dot_attention_backward_kv(colptr, rowind, q, k, v, stats, delta, go, scale=scale, results=(gk, gv))

    a_fwd(), a_bq(), a_bkv()
    res = {"M": M, "nnz": nnz, "b_bytes": 6 * nnz * H * 4}
    res["a_fwd"], res["a_bq"], res["a_bkv"] = timed(a_fwd, launches), timed(a_bq, launches), timed(a_bkv, launches)
    res["a_bwd"] = res["a_bq"] + res["a_bkv"]
    if res["b_bytes"] > b_limit:
        return res
    kept = {}

    def b_fwd():
        kept["alpha"] = softmax.edge_softmax(rp, sddmm.csr_sddmm_heads(rp, ci, q, k) * scale)
        kept["out"] = spmm.csr_spmm_heads(rp, ci, kept["alpha"], v)

    def b_bwd():
        alpha = kept["alpha"]
        ga = sddmm.csr_sddmm_heads(rp, ci, go, v)
        kept["gv"] = spmm.csr_spmm_heads(colptr, rowind, graphs.take_edges(alpha, order), go)
        gs = softmax.edge_softmax_backward(rp, alpha, ga) * scale
        kept["gq"] = spmm.csr_spmm_heads(rp, ci, gs, k)
        kept["gk"] = spmm.csr_spmm_heads(colptr, rowind, graphs.take_edges(gs, order), q)

    b_fwd(), b_bwd()
    res["rel"] = sampled_errors(rp, ci, colptr, rowind, q, k, v, go, stats, delta, scale, (out, gq, gk, gv))
    res["rel_b"] = sampled_errors(rp, ci, colptr, rowind, q, k, v, go, stats, delta, scale, (kept["out"], kept["gq"], kept["gk"], kept["gv"]))
    res["b_fwd"], res["b_bwd"] = timed(b_fwd, launches), timed(b_bwd, launches)
    kept.clear()
    return res


def training_step(name, dev, launches, H, F):
    """Median time and peak allocated memory (above the graph and the features) of one training step — forward, loss, backward, Adam —
    of examples/transformer_custom.py's Net (64 input features, H heads x F, then 1 head, 16 classes; dropout off)."""
    spec = importlib.util.spec_from_file_location("transformer_example", os.path.join(ROOT, "examples", "transformer_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    out = {}
    for key in ("fused", "composition"):
        torch.manual_seed(0)
        model = ex.Net(64, 16, F, H, dropout=0.0, fused=(key == "fused")).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.nll_loss(model(x, g), y)
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
        peak = torch.cuda.max_memory_allocated() - base
        out[key] = (timed(step, launches), peak, loss)
        del model, opt
        torch.cuda.empty_cache()
    return ci.numel(), K, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--b-limit-gb", type=float, default=64.0)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "dot_attention", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if args.step:
            for name in args.graphs.split(","):
                for case in args.cases.split(","):
                    H, F = (int(w) for w in case.split("x"))
                    nnz, n, res = training_step(name, dev, min(args.launches, 50), H, F)
                    log("#step %s nodes=%d nnz=%d (self-loops not added) two-layer model 64 -> %d x %d -> 16, one training step, median us and peak "
                        "allocated above the graph and the features: %s; one [nnz, %d] fp32 array is %.1f MB" % (
                            name, n, nnz, H, F, "  ".join("%s %.1f us %.1f MB (loss %.6f)" % (k, w[0], w[1] / 2 ** 20, w[2])
                                                         for k, w in res.items()), H, nnz * H * 4 / 2 ** 20))
            return
        log("# %s launches=%d device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (colptr, rowind, order)
            log("%s M=%d nnz=%d largest row %d largest column %d" % (name, rp.numel() - 1, ci.numel(), int(torch.diff(rp).max()),
                                                                     int(torch.diff(colptr).max())))
            for case in args.cases.split(","):
                H, F = (int(w) for w in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches, args.b_limit_gb * 2 ** 30)
                torch.cuda.empty_cache()
                head = "%-15s H=%d F=%d" % (name, H, F)
                fused = "(a) forward %.1f  backward %.1f (row pass %.1f + column pass %.1f)" % (m["a_fwd"], m["a_bwd"], m["a_bq"], m["a_bkv"])
                if "b_fwd" not in m:
                    log("%s %s   (b) not run: its [nnz, H] arrays would take %.1f GB (one is %.1f GB)" % (
                        head, fused, m["b_bytes"] / 2 ** 30, m["b_bytes"] / 6 / 2 ** 30))
                    log("#run %s %s fwd fused=%.1f" % (name, case, m["a_fwd"]))
                    log("#run %s %s bwd fused=%.1f" % (name, case, m["a_bwd"]))
                    continue
                log("%s sampled max |x - float64| / max |float64|: (a) out %.2e grad_q %.2e grad_k %.2e grad_v %.2e   (b) %.2e %.2e %.2e %.2e"
                    % ((head,) + tuple(m["rel"]) + tuple(m["rel_b"])))
                if max(m["rel"]) > 1e-3:
                    raise SystemExit("the op is outside its bound: nothing timed is worth recording")
                if max(m["rel_b"]) > 1e-3:
                    log("   (b) is OUTSIDE the bound on this case: its results are wrong, its times are recorded for scale only")
                log("   " + fused)
                for d, what in (("fwd", "forward"), ("bwd", "backward")):
                    ta, tb = m["a_" + d], m["b_" + d]
                    log("   %-8s (a) %.1f   (b) composition %.1f   (b)/(a) x%.2f" % (what, ta, tb, tb / ta))
                    log("#run %s %s %s fused=%.1f composition=%.1f" % (name, case, d, ta, tb))
                    r = before.get((name, case, d), {})
                    base, mine = r.get("composition", []) + [tb], r.get("fused", []) + [ta]
                    if len(base) >= 3:
                        margin = max(base) - min(base)
                        verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                        log("   over %d runs: (b) %s, margin = spread %.1f; (a) %s: %s than (b) beyond the margin" % (
                            len(base), " ".join("%.1f" % w for w in base), margin, " ".join("%.1f" % w for w in mine), verdict))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
