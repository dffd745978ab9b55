"""Timing of the fused add-softmax (gespmm_gat_softmax_f32 / gespmm_gat_softmax_backward_f32 / gespmm_edge_segment_sum_f32) against the
composition GATConv runs without it, IN THE SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures.

Columns, per graph, H and direction (fwd / bwd), everything into preallocated results where the call takes one:
  (a)  fused — forward: softmax.gat_edge_softmax (one launch); backward: softmax.gat_edge_softmax_backward, then
       softmax.edge_segment_sum on (colptr, csc_order) — grad_score, grad_el, grad_er (two launches)
  (b)  today's composition — forward: the two stacks q = (el, 1), k = (1, er), sddmm.csr_sddmm_heads at F = 2, softmax.edge_softmax;
       backward: softmax.edge_softmax_backward, spmm.csr_spmm_heads at F = 2 on the CSR arrays (grad_q), the grad_score[csc_order]
       copy, spmm.csr_spmm_heads at F = 2 on the CSC arrays (grad_k): the baseline
  (c)  gespmm_baseline_copy_f32 over nnz H words, one read and one write: the floor
A leaky slope of 0.2 is on in both (the GAT layer's setting: the backward reads the score's sign). (a) is checked against (b) before
anything is timed: alpha and grad_score bit for bit; grad_el / grad_er inside the bound of their pinned order against a float64 sum
of the same grad_score, and inside the any-order bound of two fp32 sums against (b)'s (``sums_ok``; where (b)'s own sums are outside
what fp32 rounding of the float64 sum explains, the row says ``composition_sums_ok=False`` and its time is reported as measured). Each run appends a `#run` line per case;
from the third run of the script on, the spread of (b)'s medians ACROSS the runs is the margin (a) is judged against.

  python scripts/gat_softmax_timing.py [--graphs a,b] [--heads 1,4,8] [--launches 200] [--out profiles/r11/gat_softmax/timing.log]
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from edge_softmax_timing import earlier_runs, median_us  # noqa: E402
from gespmm_amd import _lib, graphs, sddmm, softmax, spmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed", "products-sbm")
COLUMNS = ("fused", "composition", "copy")
SLOPE = 0.2


def load_graph(name, dev):
    if name == "pubmed":
        g = graphs.load_mtx_as_csr(os.path.join(ROOT, "tests", "golden", "pubmed.mtx"))
        return torch.from_numpy(g["rowptr"]).to(dev), torch.from_numpy(g["colind"]).to(dev), g["K"]
    g = graphs.synthetic_graph(name, seed=42, device=dev)
    return g["rowptr"], g["colind"], g["K"]


def sums_ok(ptr, seg_of_entry, x, fused, comp, shape):
    """The two fp32 segment sums of x against the float64 one -> (ok, (b) ok, text). (a) must be inside the bound of its pinned order,
    2^-24 (ceil(d / W') + log2 W' + 1) sum |x| (tests/test_gat_softmax_host.py), and (a) and (b) must not differ by more than two fp32
    sums of d terms in any order can, 2 x 2^-24 (d + 8) sum |x|; the text carries the worst ratio of each, and of (b) against float64."""
    S, H = fused.shape
    ref = torch.zeros(S, H, dtype=torch.float64, device=x.device).index_add_(0, seg_of_entry, x.double())
    mag = torch.zeros(S, H, dtype=torch.float64, device=x.device).index_add_(0, seg_of_entry, x.double().abs())
    d = torch.diff(ptr).double()
    w = torch.where(d > shape["L"], 64.0, float(shape["W"]))
    pinned = 2.0 ** -24 * (torch.ceil(d / w) + torch.log2(w) + 1)[:, None] * mag
    any_order = 2.0 ** -24 * (d + 8)[:, None] * mag

    def worst(err, bound):
        live = bound > 0
        exact = bool((err[~live] == 0).all())  # (no terms, or zeros only: nothing to round)
        return (float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0) if exact else float("inf")

    ra = worst((fused.double() - ref).abs(), pinned)
    rb = worst((comp.double() - ref).abs(), any_order)
    rab = worst((fused.double() - comp.double()).abs(), 2 * any_order)
    # (a) answers for itself and for its distance to (b) — unless (b) is itself outside what fp32 rounding explains: then the row says so
    # ("composition_sums_ok=False") and (b)'s time is reported as measured, as edge_softmax_timing.py does with torch_fp32_ok
    return ra <= 1.0 and (rab <= 1.0 or rb > 1.0), rb <= 1.0, "(a)/pinned %.3g (b)/any-order %.3g |(a)-(b)|/2 any-order %.3g" % (ra, rb, rab)


def measure(rp, ci, K, H, launches):
    dev = rp.device
    M, nnz = rp.numel() - 1, ci.numel()
    colptr, rowind, order64 = graphs.transpose_csr(rp, ci, K, return_order=True)
    order = order64.to(torch.int32)
    gen = torch.Generator(device=dev).manual_seed(1)
    el = (torch.rand(M, H, device=dev, generator=gen) - 0.5) * 4
    er = (torch.rand(K, H, device=dev, generator=gen) - 0.5) * 4
    galpha = torch.rand(nnz, H, device=dev, generator=gen) - 0.5
    alpha, alpha_b, grad_b, scratch = (torch.empty(nnz, H, device=dev) for _ in range(4))
    grad_er = torch.empty(K, H, device=dev)
    state = {}

    def fused_fwd():
        softmax.gat_edge_softmax(rp, ci, el, er, negative_slope=SLOPE, out=alpha)

    def comp_fwd():
        q = torch.stack((el, torch.ones_like(el)), dim=-1)
        k = torch.stack((torch.ones_like(er), er), dim=-1)
        state["q"], state["k"] = q, k
        state["score"] = sddmm.csr_sddmm_heads(rp, ci, q, k)
        softmax.edge_softmax(rp, state["score"], out=alpha_b, negative_slope=SLOPE)

    def fused_bwd():
        gs, gel = softmax.gat_edge_softmax_backward(rp, ci, alpha, galpha, el=el, er=er, negative_slope=SLOPE)
        softmax.edge_segment_sum(colptr, gs, order=order, out=grad_er)
        return gs, gel, grad_er

    def comp_bwd():
        gs = softmax.edge_softmax_backward(rp, alpha_b, galpha, score=state["score"], negative_slope=SLOPE, out=grad_b)
        gq = spmm.csr_spmm_heads(rp, ci, gs, state["k"])
        gk = spmm.csr_spmm_heads(colptr, rowind, gs[order64].contiguous(), state["q"])
        return gs, gq[..., 0], gk[..., 1]

    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    src, dst = ctypes.c_void_p(galpha.data_ptr()), ctypes.c_void_p(scratch.data_ptr())

    def copy():
        _lib.check(_lib.lib.gespmm_baseline_copy_f32(src, dst, nnz * H, stream()), "gespmm_baseline_copy_f32")

    res = {"describe": _lib.describe_edge_softmax(M, nnz, H), "describe_csc": _lib.describe_edge_softmax(K, nnz, H), "M": M, "nnz": nnz,
           "max_degree": int(torch.diff(rp).max()), "max_in_degree": int(torch.diff(colptr).max())}
    fused_fwd()
    comp_fwd()
    same = lambda x, y: bool((x.view(torch.int32) == y.view(torch.int32)).all())  # noqa: E731
    fa, fb = fused_bwd(), comp_bwd()
    res["alpha_same_bits"] = same(alpha, alpha_b)
    res["grad_score_same_bits"] = same(fa[0], fb[0])
    rows64 = torch.repeat_interleave(torch.arange(M, device=dev), torch.diff(rp).long())
    res["grad_el_ok"], bel, res["grad_el_text"] = sums_ok(rp, rows64, fa[0], fa[1], fb[1], res["describe"])
    del rows64
    res["grad_er_ok"], ber, res["grad_er_text"] = sums_ok(colptr, ci.long(), fa[0], fa[2], fb[2], res["describe_csc"])
    res["composition_sums_ok"] = bel and ber
    del fa, fb
    fns = {"fwd": {"fused": fused_fwd, "composition": comp_fwd, "copy": copy},
           "bwd": {"fused": fused_bwd, "composition": comp_bwd, "copy": copy}}
    for direction in ("fwd", "bwd"):
        for c in COLUMNS:
            res[(direction, c)] = median_us(fns[direction][c], launches)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--heads", default="1,4,8")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "gat_softmax", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d slope=%s device=%s (us; median of per-launch event pairs)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, SLOPE, torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp, ci, K = load_graph(name, dev)
            for H in (int(h) for h in args.heads.split(",")):
                m = measure(rp, ci, K, H, args.launches)
                log("%-15s H=%d M=%d nnz=%d max_degree=%d max_in_degree=%d rows %s columns %s alpha_same_bits=%s grad_score_same_bits=%s "
                    "grad_el_ok=%s grad_er_ok=%s composition_sums_ok=%s" % (
                        name, H, m["M"], m["nnz"], m["max_degree"], m["max_in_degree"],
                        " ".join("%s=%s" % kv for kv in m["describe"].items()), " ".join("%s=%s" % kv for kv in m["describe_csc"].items()),
                        m["alpha_same_bits"], m["grad_score_same_bits"], m["grad_el_ok"], m["grad_er_ok"], m["composition_sums_ok"]))
                log("   sums, worst error / bound: grad_el %s; grad_er %s" % (m["grad_el_text"], m["grad_er_text"]))
                if not (m["alpha_same_bits"] and m["grad_score_same_bits"] and m["grad_el_ok"] and m["grad_er_ok"]):
                    raise SystemExit("fused and composition disagree: nothing timed is worth recording")
                for direction in ("fwd", "bwd"):
                    a, b, c = (m[(direction, col)] for col in COLUMNS)
                    log("   %s  (a) fused %.1f   (b) composition %.1f   (c) copy floor %.1f   (b)/(a) x%.2f   (a)/(c) x%.2f" % (
                        direction, a, b, c, b / a, a / c))
                    log("#run %s %d %s fused=%.1f composition=%.1f copy=%.1f" % (name, H, direction, a, b, c))
                    r = before.get((name, H, direction), {})
                    base, mine = r.get("composition", []) + [b], r.get("fused", []) + [a]
                    if len(base) >= 3:
                        margin = max(base) - min(base)
                        verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                        log("   over %d runs: (b) %s, margin = spread %.1f; (a) %s: %s than (b) beyond the margin" % (
                            len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict))
            del rp, ci
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
