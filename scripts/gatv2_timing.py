"""Timing of the GATv2 edge score (gespmm_gatv2_score_f32 + gespmm_gatv2_score_backward_f32) against the only way torch has, IN THE
SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures.

Columns, per graph and (H, F); slope 0.2:
  (a)  forward: sddmm.gatv2_score into a preallocated score; backward: the row pass (grad_xl, att_part) + the column pass (grad_xr) +
       att_part.sum(0) — three launches and one torch reduction, nothing larger than [nnz, H]
  (b)  forward: ((xl[rows] + xr[cols]).leaky_relu() * att).sum(-1); backward: torch.autograd through it (the [nnz, H, F] arrays)
(a) is checked against (b) before anything is timed (1e-3 of the largest value: two fp32 summation orders; for the check the leaky
ReLU is a select on t >= 0, so that its derivative at an exact zero of t is the op's). (b) is not run where its
[nnz, H, F] arrays would pass --b-limit-gb (five of them counted: the sum, the leaky ReLU's result, the product and two gradients);
the size it would need is printed instead. Each run appends a `#run` line per case; from the third run of the script on, the spread of
(b)'s medians ACROSS the runs is the margin (a) is judged against.

  python scripts/gatv2_timing.py [--graphs a,b] [--cases 1x64,4x16,8x8,8x32] [--launches 200] [--out profiles/r15/gatv2/timing.log]
  python scripts/gatv2_timing.py --step [--graphs pubmed,com-amazon-sbm]      time and peak device memory of one training step of the
                                                                               example's two-layer model: --v2, a v2 layer on the torch
                                                                               composition, and GATConv (default path) for scale
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
from gat_aggregate_timing import CASES, earlier_runs  # noqa: E402
from gat_softmax_timing import GRAPHS, SLOPE, load_graph  # noqa: E402
import gespmm_amd  # noqa: E402
from gespmm_amd import graphs, sddmm  # noqa: E402


def composition(xl, xr, att, rows, cols):
    return (torch.nn.functional.leaky_relu(xl[rows] + xr[cols], SLOPE) * att).sum(-1)


def measure(rp, ci, csc, K, H, F, launches, b_limit):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind, order = csc
    gen = torch.Generator(device=dev).manual_seed(1)
    xl = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    xr = torch.rand(K, H, F, device=dev, generator=gen) - 0.5
    att = (torch.rand(H, F, device=dev, generator=gen) - 0.5) * 2
    gs = torch.rand(nnz, H, device=dev, generator=gen) - 0.5
    score = torch.empty(nnz, H, device=dev)
    gxl, part, gxr = torch.empty(M, H, F, device=dev), torch.empty(M, H, F, device=dev), torch.empty(K, H, F, device=dev)
    kept = {}

    def a_fwd():
        sddmm.gatv2_score(rp, ci, xl, xr, att, negative_slope=SLOPE, out=score)

    def a_bwd():
        sddmm.gatv2_score_backward(rp, ci, gs, xl, xr, att, negative_slope=SLOPE, want_att_part=True, out=(gxl, part))
        sddmm.gatv2_score_backward(colptr, rowind, gs, xr, xl, att, negative_slope=SLOPE, order=order, out=gxr)
        kept["gatt"] = part.sum(0)

    a_fwd(), a_bwd()
    res = {"M": M, "nnz": nnz, "b_bytes": 5 * nnz * H * F * 4}
    res["a_fwd"], res["a_bwd"] = median_us(a_fwd, launches), median_us(a_bwd, launches)
    if res["b_bytes"] > b_limit:
        return res
    rows = torch.repeat_interleave(torch.arange(M, device=dev), torch.diff(rp).long())
    cols = ci.long()
    leaves = [t.clone().requires_grad_(True) for t in (xl, xr, att)]

    def b_fwd():
        kept["s"] = composition(*leaves, rows, cols)

    def b_bwd():
        kept["g"] = torch.autograd.grad(kept["s"], leaves, gs, retain_graph=True)

    # the check: the same composition with the leaky ReLU as a select on t >= 0, whose derivative at an exact zero of t is ours (1) and
    # not leaky_relu's (the slope) — among millions of sums of two fp32 words some are exactly zero
    t = leaves[0][rows] + leaves[1][cols]
    s = (torch.where(t >= 0, t, t * SLOPE) * leaves[2]).sum(-1)
    g = torch.autograd.grad(s, leaves, gs)
    rel = lambda u, v: float((u - v).abs().max() / v.abs().max().clamp_min(1e-30))  # noqa: E731
    res["rel"] = [rel(score, s.detach()), rel(gxl, g[0]), rel(gxr, g[1]), rel(kept["gatt"], g[2])]
    res["zeros"] = int((t == 0).sum())
    del t, s, g
    b_fwd(), b_bwd()
    res["b_fwd"] = median_us(b_fwd, launches)
    res["b_bwd"] = median_us(b_bwd, launches)
    kept.clear()
    return res


class TorchV2Conv(gespmm_amd.GATv2Conv):
    """GATv2Conv with the score as torch computes it; every other step is the layer's."""

    def forward(self, x, rowptr, colind, colptr, rowind, csc_order, attn_seed=None):
        n, H, F = x.shape[0], self.heads, self.out_channels
        xr = (x @ self.weight_src).view(n, H, F)
        xl = xr if self.share_weights else (x @ self.weight_dst).view(n, H, F)
        rows = torch.repeat_interleave(torch.arange(n, device=x.device), torch.diff(rowptr).long())
        score = (torch.nn.functional.leaky_relu(xl[rows] + xr[colind.long()], self.negative_slope) * self.att).sum(-1)
        alpha = gespmm_amd.EdgeSoftmaxFunction.apply(rowptr, score, None)
        out = gespmm_amd.MultiHeadSPMMFunction.apply(rowptr, colind, colptr, rowind, csc_order, xr, alpha, None, True)
        out = out.reshape(n, H * F) if self.concat else out.mean(dim=1)
        return out if self.bias is None else out + self.bias


def training_step(name, dev, launches):
    """Median time and peak allocated memory (above the graph and the features) of one training step — forward, loss, backward, Adam —
    of examples/gat_custom.py's Net (64 input features, 8 heads x 8, then 1 head, 16 classes; dropout off)."""
    spec = importlib.util.spec_from_file_location("gat_example", os.path.join(ROOT, "examples", "gat_custom.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rp, ci, K = load_graph(name, dev)
    colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
    g = {"rowptr": rp, "colind": ci, "colptr": colptr, "rowind": rowind, "csc_order": order.to(torch.int32)}
    del order
    x = torch.rand(K, 64, device=dev)
    y = torch.randint(0, 16, (K,), device=dev)
    out = {}
    for key in ("v2", "v2-torch-score", "gat"):
        torch.manual_seed(0)
        model = ex.Net(64, 16, 8, 8, dropout=0.0, v2=(key != "gat")).to(dev)
        if key == "v2-torch-score":
            model.conv1.__class__ = TorchV2Conv
            model.conv2.__class__ = TorchV2Conv
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
        out[key] = (median_us(step, launches, warmup=3), peak, loss)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "gatv2", "timing.log"))
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
            for name in (args.graphs.split(",") if args.graphs != ",".join(GRAPHS) else ["pubmed", "com-amazon-sbm"]):
                nnz, n, res = training_step(name, dev, min(args.launches, 50))
                log("#step %s nodes=%d nnz=%d (self-loops not added) two-layer model 64 -> 8 x 8 -> 16, one training step, median us and peak "
                    "allocated above the graph and the features: %s; one [nnz, 8, 8] fp32 array is %.1f MB, one [nnz, 8] array %.1f MB" % (
                        name, n, nnz, "  ".join("%s %.1f us %.1f MB (loss %.6f)" % (k, v[0], v[1] / 2 ** 20, v[2]) for k, v in res.items()),
                        nnz * 64 * 4 / 2 ** 20, nnz * 8 * 4 / 2 ** 20))
            return
        log("# %s launches=%d slope=%s device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, SLOPE, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            colptr, rowind, order = graphs.transpose_csr(rp, ci, K, return_order=True)
            csc = (colptr, rowind, order.to(torch.int32))
            del order
            for case in args.cases.split(","):
                H, F = (int(v) for v in case.split("x"))
                m = measure(rp, ci, csc, K, H, F, args.launches, args.b_limit_gb * 2 ** 30)
                torch.cuda.empty_cache()
                head = "%-15s H=%d F=%d M=%d nnz=%d" % (name, H, F, m["M"], m["nnz"])
                if "b_fwd" not in m:
                    log("%s (a) forward %.1f  backward (2 launches + sum) %.1f   (b) not run: its [nnz, H, F] arrays would take %.1f GB "
                        "(one is %.1f GB)" % (head, m["a_fwd"], m["a_bwd"], m["b_bytes"] / 2 ** 30, m["b_bytes"] / 5 / 2 ** 30))
                    log("#run %s %s fwd fused=%.1f" % (name, case, m["a_fwd"]))
                    log("#run %s %s bwd fused=%.1f" % (name, case, m["a_bwd"]))
                    continue
                log("%s max |a - b| / max |b|: score %.2e grad_xl %.2e grad_xr %.2e grad_att %.2e (%d exact zeros among the sums t)" % (
                    (head,) + tuple(m["rel"]) + (m["zeros"],)))
                if max(m["rel"]) > 1e-3:
                    raise SystemExit("the op is outside its bound: nothing timed is worth recording")
                for d, what in (("fwd", "forward"), ("bwd", "backward")):
                    ta, tb = m["a_" + d], m["b_" + d]
                    log("   %-8s (a) %.1f   (b) torch composition %.1f   (b)/(a) x%.2f" % (what, ta, tb, tb / ta))
                    log("#run %s %s %s fused=%.1f composition=%.1f" % (name, case, d, ta, tb))
                    r = before.get((name, case, d), {})
                    base, mine = r.get("composition", []) + [tb], r.get("fused", []) + [ta]
                    if len(base) >= 3:
                        margin = max(base) - min(base)
                        verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                        log("   over %d runs: (b) %s, margin = spread %.1f; (a) %s: %s than (b) beyond the margin" % (
                            len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict))
            del rp, ci, csc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
