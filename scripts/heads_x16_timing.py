"""Timing of the 16-bit multi-head ops (gespmm_csr_spmm_heads_x16, gespmm_sddmm_csr_heads_x16) against the fp32 entries and against
their own composition routes, IN THE SAME RUN, and of a two-layer GAT training step in bf16 against fp32.

One process per run; every figure is the median of >= 200 per-launch event pairs after a warm-up, as bench.py measures; every column is
measured three times per run, the columns of a case taking turns (round 1 of every column, then round 2, ...), so that a drift of the
machine lands on all of them.

Columns, per graph and (H, F) — the operands of the 16-bit columns are bf16:
  product  (a) csr_spmm_heads_x16, the kernel route       (b) the same call with GESPMM_HEADS_X16_ROUTE=composition (read per call)
           (c) csr_spmm_heads on the fp32 operand: what a caller ran before
  SDDMM    (a) csr_sddmm_heads_x16, the kernel route      (b) the same call with GESPMM_SDDMM_HEADS_ROUTE=composition
           (c) csr_sddmm_heads on the fp32 operands
Bit equality of (a) and (b), and of (a) with narrow((c)) for the product, is checked before anything is timed.
  step     examples/gat_custom.py's two-layer model (8 heads x 8, then 1 head), one training step: median time over --steps steps and the
           peak of torch's allocator over them, for --dtype fp32 and bf16, default path and --fused-score.
Each run appends a `#run` line per case; from the third run of the script on, the spread of (c)'s medians ACROSS the runs is the margin
(a) is judged against.

  python scripts/heads_x16_timing.py [--graphs a,b] [--launches 200] [--steps 60] [--out profiles/r18/heads_x16/timing.log]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from gespmm_amd import _lib, graphs, sddmm, spmm  # noqa: E402

GRAPHS = ("com-amazon-sbm", "pubmed")
SHAPES = ((4, 16), (8, 8), (8, 32), (8, 64))
PRODUCT = ("x16_kernel", "x16_composition", "f32")
SDDMM = ("sd_x16_kernel", "sd_x16_composition", "sd_f32")
PINS = {"x16_composition": ("GESPMM_HEADS_X16_ROUTE", "composition"), "sd_x16_composition": ("GESPMM_SDDMM_HEADS_ROUTE", "composition")}


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


def load_csr(name, dev):
    if name == "pubmed":
        g = graphs.load_mtx_as_csr(os.path.join(ROOT, "tests", "golden", "pubmed.mtx"))
        return torch.from_numpy(g["rowptr"]).to(dev), torch.from_numpy(g["colind"]).to(dev), g["M"], g["K"]
    g = graphs.synthetic_graph(name, seed=42, device=dev)
    return g["rowptr"], g["colind"], g["M"], g["K"]


class pinned:
    """The route pin of a column, set around its calls only (the library reads it per call)."""

    def __init__(self, column):
        self.pin = PINS.get(column)

    def __enter__(self):
        if self.pin:
            os.environ[self.pin[0]] = self.pin[1]

    def __exit__(self, *exc):
        if self.pin:
            os.environ.pop(self.pin[0], None)


def take_turns(fns, columns, launches):
    res = {c: [] for c in columns}
    for _ in range(3):
        for c in columns:
            with pinned(c):
                res[c].append(median_us(fns[c], launches))
    return res


def measure(rp, ci, M, K, H, F, launches):
    dev = rp.device
    nnz = ci.numel()
    gen = torch.Generator(device=dev).manual_seed(1)
    val = torch.rand(nnz, H, device=dev, generator=gen) - 0.5
    B = torch.rand(K, H, F, device=dev, generator=gen) - 0.5
    D1 = torch.rand(M, H, F, device=dev, generator=gen) - 0.5
    B16, D116 = B.bfloat16(), D1.bfloat16()
    out16 = torch.empty(M, H, F, device=dev, dtype=torch.bfloat16)
    out32 = torch.empty(M, H, F, device=dev)
    s16, s32 = torch.empty(nnz, H, device=dev), torch.empty(nnz, H, device=dev)
    fns = {
        "x16_kernel": lambda: spmm.csr_spmm_heads_x16(rp, ci, val, B16, out=out16),
        "x16_composition": lambda: spmm.csr_spmm_heads_x16(rp, ci, val, B16, out=out16),
        "f32": lambda: spmm.csr_spmm_heads(rp, ci, val, B, out=out32),
        "sd_x16_kernel": lambda: sddmm.csr_sddmm_heads_x16(rp, ci, D116, B16, out=s16),
        "sd_x16_composition": lambda: sddmm.csr_sddmm_heads_x16(rp, ci, D116, B16, out=s16),
        "sd_f32": lambda: sddmm.csr_sddmm_heads(rp, ci, D1, B, out=s32),
    }
    for k in ("GESPMM_HEADS_X16_ROUTE", "GESPMM_SDDMM_HEADS_ROUTE", "GESPMM_HEADS_ROUTE"):
        os.environ.pop(k, None)
    res = {"route": _lib.heads_x16_route(M, K, H, F, nnz), "sd": _lib.describe_sddmm_heads(True, M, nnz, H, F, x16=True)}
    a = fns["x16_kernel"]().clone()
    with pinned("x16_composition"):
        res["route_pinned"] = _lib.heads_x16_route(M, K, H, F, nnz)[0]
        b = fns["x16_composition"]().clone()
    res["bits_equal"] = torch.equal(a.view(torch.int16), b.view(torch.int16)) and \
        torch.equal(a.view(torch.int16), spmm.csr_spmm_heads(rp, ci, val, B16.float()).bfloat16().view(torch.int16))
    sa = fns["sd_x16_kernel"]().clone()
    with pinned("sd_x16_composition"):
        res["sd_pinned"] = _lib.describe_sddmm_heads(True, M, nnz, H, F, x16=True)["route"]
        sb = fns["sd_x16_composition"]().clone()
    res["sd_bits_equal"] = torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    res.update(take_turns(fns, PRODUCT, launches))
    res.update(take_turns(fns, SDDMM, launches))
    torch.cuda.empty_cache()
    return res


def training_step(name, dtype, fused_score, steps):
    """(median ms of one training step, peak MiB of torch's allocator over the timed steps) of examples/gat_custom.py's model."""
    import torch.nn.functional as F

    from gat_custom import Net, gat_graph
    from gcn_custom import load_edges

    dev = torch.device("cuda")
    edge_index, n_v, n_feat, n_cls = load_edges(name, dev)
    g = gat_graph(edge_index, n_v, dev, int32_order=fused_score)
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n_v, n_feat, generator=gen)
    x = (x / x.sum(1, keepdim=True)).to(dev)
    y = torch.randint(0, n_cls, (n_v,), generator=gen).to(dev)
    train_idx = torch.randperm(n_v, generator=gen)[:20 * n_cls].to(dev)
    torch.manual_seed(0)
    model = Net(n_feat, n_cls, 8, 8, 0.6, fused_score=fused_score).to(dev)
    if dtype != torch.float32:
        model, x = model.to(dtype), x.to(dtype)
    opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=5e-4)
    y_train = y[train_idx]
    model.train()

    def step():
        opt.zero_grad(set_to_none=False)
        loss = F.nll_loss(model(x, g).index_select(0, train_idx), y_train)
        loss.backward()
        opt.step()
        return loss

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        loss = step()
        b.record()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)), "the loss is not finite"
    peak = torch.cuda.max_memory_allocated() / 2.0 ** 20
    del model, opt, g, x
    torch.cuda.empty_cache()
    return statistics.median(a.elapsed_time(b) for a, b in ev), peak, float(loss)


def earlier_runs(path):
    """{(graph, H, F): {column: [median of each earlier run]}} from the `#run` lines of the log."""
    runs = {}
    if os.path.exists(path):
        for line in open(path):
            if line.startswith("#run "):
                _, name, h, f, *cols = line.split()
                d = runs.setdefault((name, int(h), int(f)), {})
                for kv in cols:
                    k, v = kv.split("=")
                    d.setdefault(k, []).append(float(v))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default=",".join(GRAPHS))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=60, help="timed training steps per setting (0: skip the training step)")
    ap.add_argument("--step-datasets", default="pubmed", help="datasets of examples/gcn_custom.py's load_edges for the training step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "heads_x16", "timing.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device (nothing here is a measurement without one)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    before = earlier_runs(args.out)
    med = statistics.median
    dev = torch.device("cuda")
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d device=%s (us; three medians each, columns taking turns)" % (
            " ".join(sys.argv[1:]) or "(defaults)", args.launches, torch.cuda.get_device_name(0)))
        fmt = lambda v: "%s (median %.1f)" % (" ".join("%.1f" % x for x in v), med(v))  # noqa: E731
        for name in [n for n in args.graphs.split(",") if n]:
            rp, ci, M, K = load_csr(name, dev)
            for H, F in SHAPES:
                m = measure(rp, ci, M, K, H, F, args.launches)
                c, sc = med(m["f32"]), med(m["sd_f32"])
                log("%-15s H=%d F=%d M=%d nnz=%d product: route=%d V,S,W,rpw=%s pinned route=%d bits_equal=%s | sddmm: %s pinned %s bits_equal=%s" % (
                    name, H, F, M, ci.numel(), m["route"][0], m["route"][1], m["route_pinned"], m["bits_equal"],
                    " ".join("%s=%s" % kv for kv in m["sd"].items()), m["sd_pinned"], m["sd_bits_equal"]))
                log("   product (a) bf16, kernel route       %s   x%.2f of (c)" % (fmt(m["x16_kernel"]), c / med(m["x16_kernel"])))
                log("           (b) bf16, composition route  %s   x%.2f of (c)" % (fmt(m["x16_composition"]), c / med(m["x16_composition"])))
                log("           (c) fp32 entry               %s" % fmt(m["f32"]))
                log("   sddmm   (a) bf16, kernel route       %s   x%.2f of (c)" % (fmt(m["sd_x16_kernel"]), sc / med(m["sd_x16_kernel"])))
                log("           (b) bf16, composition route  %s   x%.2f of (c)" % (fmt(m["sd_x16_composition"]), sc / med(m["sd_x16_composition"])))
                log("           (c) fp32 entry               %s" % fmt(m["sd_f32"]))
                log("#run %s %d %d %s" % (name, H, F, " ".join("%s=%.1f" % (k, med(m[k])) for k in PRODUCT + SDDMM)))
                r = before.get((name, H, F), {})
                for mine_k, base_k, what in (("x16_kernel", "f32", "product"), ("sd_x16_kernel", "sd_f32", "sddmm")):
                    base = r.get(base_k, []) + [med(m[base_k])]
                    mine = r.get(mine_k, []) + [med(m[mine_k])]
                    if len(base) >= 3:
                        margin = max(base) - min(base)
                        verdict = "FASTER" if max(mine) < min(base) - margin else ("SLOWER" if min(mine) > max(base) + margin else "not different")
                        log("   %s over %d runs: (c) %s, margin = spread %.1f; (a) %s: %s beyond the margin" % (
                            what, len(base), " ".join("%.1f" % v for v in base), margin, " ".join("%.1f" % v for v in mine), verdict))
            del rp, ci
            torch.cuda.empty_cache()
        if args.steps > 0:
            for name in [n for n in args.step_datasets.split(",") if n]:
                for fused_score in (False, True):
                    rows = []
                    for _ in range(2):  # the two dtypes take turns, twice
                        for dtype in (torch.float32, torch.bfloat16):
                            rows.append((dtype,) + training_step(name, dtype, fused_score, args.steps))
                    for dtype, ms, peak, loss in rows:
                        log("step %-8s fused_score=%-5s dtype=%-8s %.3f ms/step  peak %.1f MiB  last loss %.4f" % (
                            name, fused_score, str(dtype).replace("torch.", ""), ms, peak, loss))


if __name__ == "__main__":
    main()
