"""Timing of the edge softmax (gespmm_edge_softmax_f32 / gespmm_edge_softmax_backward_f32) against what a caller can do without it,
IN THE SAME RUN.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures.

Columns, per graph, H and direction (fwd / bwd):
  (a)  the op: softmax.edge_softmax / softmax.edge_softmax_backward into a preallocated result
  (b)  a torch composition on the same arrays — forward: segment_reduce max, repeat_interleave, sub, exp, segment_reduce sum,
       repeat_interleave, div; backward: mul, segment_reduce sum, repeat_interleave, sub, mul — with the degrees made BEFOREHAND and not
       charged: the baseline
  (c)  gespmm_baseline_copy_f32 over the same nnz H words, one read and one write: the floor
(a) is checked against (b)'s formula in float64 before anything is timed, and so is (b) itself ("torch_fp32_ok": on products-sbm at H = 4
the fp32 composition returns inf in places — the op does not). Each run appends a `#run` line per case; from the third run of the script
on, the spread of (b)'s medians ACROSS the runs is the margin (a) is judged against.

  python scripts/edge_softmax_timing.py [--graphs a,b] [--heads 1,4,8] [--launches 200] [--out profiles/r10/edge_softmax/timing.log]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gespmm_amd import _lib, graphs, softmax  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed", "products-sbm")
COLUMNS = ("op", "torch", "copy")


def median_us(fn, launches, warmup=20):
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


def load_rowptr(name, dev):
    if name == "pubmed":
        g = graphs.load_mtx_as_csr(os.path.join(ROOT, "tests", "golden", "pubmed.mtx"))
        return torch.from_numpy(g["rowptr"]).to(dev)
    return graphs.synthetic_graph(name, seed=42, device=dev)["rowptr"]


def measure(rp, H, launches):
    dev = rp.device
    M, nnz = rp.numel() - 1, int(rp[-1])
    deg = torch.diff(rp).long()
    gen = torch.Generator(device=dev).manual_seed(1)
    score = (torch.rand(nnz, H, device=dev, generator=gen) - 0.5) * 8
    galpha = torch.rand(nnz, H, device=dev, generator=gen) - 0.5
    alpha, grad, scratch = torch.empty_like(score), torch.empty_like(score), torch.empty_like(score)

    def torch_fwd(score=score):
        m = torch.segment_reduce(score, "max", lengths=deg, axis=0)
        t = torch.exp(score - torch.repeat_interleave(m, deg, dim=0, output_size=nnz))
        s = torch.segment_reduce(t, "sum", lengths=deg, axis=0)
        return t / torch.repeat_interleave(s, deg, dim=0, output_size=nnz)

    def torch_bwd(alpha=alpha, galpha=galpha):
        dot = torch.segment_reduce(alpha * galpha, "sum", lengths=deg, axis=0)
        return alpha * (galpha - torch.repeat_interleave(dot, deg, dim=0, output_size=nnz))

    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    src, dst = ctypes.c_void_p(score.data_ptr()), ctypes.c_void_p(scratch.data_ptr())

    def copy():
        _lib.check(_lib.lib.gespmm_baseline_copy_f32(src, dst, nnz * H, stream()), "gespmm_baseline_copy_f32")

    fns = {
        "fwd": {"op": lambda: softmax.edge_softmax(rp, score, out=alpha), "torch": torch_fwd, "copy": copy},
        "bwd": {"op": lambda: softmax.edge_softmax_backward(rp, alpha, galpha, out=grad), "torch": torch_bwd, "copy": copy},
    }
    res = {"describe": _lib.describe_edge_softmax(M, nnz, H), "M": M, "nnz": nnz, "max_degree": int(deg.max())}
    fns["fwd"]["op"]()
    fns["bwd"]["op"]()
    ref_a = torch_fwd(score.double())
    ref_g = torch_bwd(alpha.double(), galpha.double())
    res["close"] = bool(torch.allclose(alpha.double(), ref_a, rtol=1e-4, atol=1e-30)) and bool(torch.allclose(grad.double(), ref_g, rtol=1e-3, atol=1e-6))
    res["torch_ok"] = bool(torch.allclose(torch_fwd().double(), ref_a, rtol=1e-4, atol=1e-30)) and \
        bool(torch.allclose(torch_bwd().double(), ref_g, rtol=1e-3, atol=1e-6))
    del ref_a, ref_g
    for direction in ("fwd", "bwd"):
        for c in COLUMNS:
            res[(direction, c)] = median_us(fns[direction][c], launches)
    return res


def earlier_runs(path):
    """{(graph, H, direction): {column: [median of each earlier run]}} from the `#run` lines of the log."""
    runs = {}
    if os.path.exists(path):
        for line in open(path):
            if line.startswith("#run "):
                _, name, h, direction, *cols = line.split()
                d = runs.setdefault((name, int(h), direction), {})
                for kv in cols:
                    k, v = kv.split("=")
                    d.setdefault(k, []).append(float(v))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--heads", default="1,4,8")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "edge_softmax", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d device=%s (us; median of per-launch event pairs)" % (" ".join(sys.argv[1:]) or "(defaults)", args.launches,
                                                                                   torch.cuda.get_device_name(0)))
        for name in args.graphs.split(","):
            rp = load_rowptr(name, dev)
            for H in (int(h) for h in args.heads.split(",")):
                m = measure(rp, H, args.launches)
                log("%-15s H=%d M=%d nnz=%d max_degree=%d %s op_close_to_float64=%s torch_fp32_ok=%s" % (
                    name, H, m["M"], m["nnz"], m["max_degree"], " ".join("%s=%s" % kv for kv in m["describe"].items()), m["close"],
                    m["torch_ok"]))
                for direction in ("fwd", "bwd"):
                    a, b, c = (m[(direction, col)] for col in COLUMNS)
                    log("   %s  (a) op %.1f   (b) torch composition %.1f   (c) copy floor %.1f   (b)/(a) x%.2f   (a)/(c) x%.2f" % (
                        direction, a, b, c, b / a, a / c))
                    log("#run %s %d %s op=%.1f torch=%.1f copy=%.1f" % (name, H, direction, a, b, c))
                    r = before.get((name, H, direction), {})
                    base, mine = r.get("torch", []) + [b], r.get("op", []) + [a]
                    if len(base) >= 3:
                        margin = max(base) - min(base)
                        verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                        log("   over %d runs: (b) %s, margin = spread %.1f; (a) %s: %s than (b) beyond the margin" % (
                            len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict))
            del rp
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
