"""Timing of the fused product (gespmm_plan_spmm_fused_f32 / GCNConv(fused=True)) against the unfused path IN THE SAME RUN.

One process; every figure is the median of >= 200 launches between device events after a warm-up, as bench.py measures; every
comparison is repeated three times and the margin is the spread (max - min) of the unfused medians.

  1. product level, N = 128, default SpmmPlan, on com-amazon-sbm, products-sbm, reddit-sbm and pubmed:
       fused call with all three vectors  |  unfused composition (torch mul, the plan's product, torch mul, torch add)  |  bare product
  2. epoch level: the two-layer GCN of examples/gcn_custom.py (hidden 128, cached=True, weighted) on com-amazon-sbm and pubmed,
     fused off against on.

  python scripts/fused_timing.py [--graphs a,b] [--launches 200] [--out profiles/r07/fused/timing.log]
  python scripts/fused_timing.py --route-audit      # product level only, under whatever GESPMM_FUSED_ROUTE says (run once per setting)
"""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gespmm_amd import graphs, spmm  # noqa: E402


def _example():
    spec = importlib.util.spec_from_file_location("gcn_custom_example", os.path.join(ROOT, "examples", "gcn_custom.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def product_level(name, N, launches, log):
    dev = torch.device("cuda")
    rp, ci, M, K = load_csr(name, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    B = torch.rand(K, N, device=dev, generator=gen) - 0.5
    cs = torch.rand(K, device=dev, generator=gen) + 0.5
    rs = torch.rand(M, device=dev, generator=gen) + 0.5
    bias = torch.rand(N, device=dev, generator=gen) - 0.5
    plan = spmm.SpmmPlan(rp, ci, K, N)
    out = torch.empty(M, N, device=dev)
    route = plan.fused_route(N)

    def fused():
        return plan.run_fused(None, B, cs, rs, bias, out)

    def unfused():
        return plan.run(None, B * cs.unsqueeze(1)) * rs.unsqueeze(1) + bias

    def bare():
        return plan.run(None, B, out)

    same = torch.equal(fused().view(torch.int32), unfused().view(torch.int32))
    reps = []
    for _ in range(3):
        reps.append((median_us(unfused, launches), median_us(fused, launches), median_us(bare, launches)))
    un = [r[0] for r in reps]
    fu = [r[1] for r in reps]
    ba = [r[2] for r in reps]
    margin = max(un) - min(un)
    log("product %-15s N=%d M=%d nnz=%d fused_route=%d env=%s bits_equal=%s | %s" % (name, N, M, ci.numel(), route,
        os.environ.get("GESPMM_FUSED_ROUTE", "-"), same, plan.describe().split("|")[-1].strip()[:90]))
    log("   unfused composition us: %s  (median %.1f, margin = spread %.1f)" % (" ".join("%.1f" % v for v in un), statistics.median(un), margin))
    log("   fused call          us: %s  (median %.1f)  -> x%.2f, %s beyond the margin" % (
        " ".join("%.1f" % v for v in fu), statistics.median(fu), statistics.median(un) / statistics.median(fu),
        "FASTER" if max(fu) < min(un) - margin else ("slower" if min(fu) > max(un) + margin else "not")))
    log("   bare unfused product us: %s  (median %.1f)  fused / bare = %.2f" % (" ".join("%.1f" % v for v in ba), statistics.median(ba),
                                                                               statistics.median(fu) / statistics.median(ba)))
    del plan
    torch.cuda.empty_cache()


def epoch_level(name, launches, log):
    import torch.nn.functional as F

    ex = _example()
    dev = torch.device("cuda")
    edge_index, n_v, n_feat, n_cls = ex.load_edges(name, dev)
    g = ex.proc(edge_index, n_v, dev)
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n_v, n_feat, generator=gen)
    x = (x / x.sum(1, keepdim=True)).to(dev)
    y = torch.randint(0, n_cls, (n_v,), generator=gen).to(dev)
    idx = torch.randperm(n_v, generator=gen)[: 20 * n_cls].to(dev)
    steps = {}
    for fused in (False, True):
        torch.manual_seed(0)
        model = ex.Net(n_feat, 128, n_cls, 2, True, cached=True, fused=fused).to(dev)
        opt = torch.optim.Adam([dict(params=model.reg_params, weight_decay=5e-4), dict(params=model.non_reg_params, weight_decay=0)], lr=0.01)

        def step(model=model, opt=opt):
            opt.zero_grad(set_to_none=False)
            loss = F.nll_loss(model(x, g).index_select(0, idx), y[idx])
            loss.backward()
            opt.step()

        steps[fused] = step
    reps = [(median_us(steps[False], launches, warmup=10) / 1e3, median_us(steps[True], launches, warmup=10) / 1e3) for _ in range(3)]
    off = [r[0] for r in reps]
    on = [r[1] for r in reps]
    margin = max(off) - min(off)
    log("epoch   %-15s hidden=128 cached=True weighted: fused off ms %s | on ms %s | margin %.3f -> x%.3f, %s" % (
        name, " ".join("%.3f" % v for v in off), " ".join("%.3f" % v for v in on), margin, statistics.median(off) / statistics.median(on),
        "slower beyond the margin" if min(on) > max(off) + margin else "not slower beyond the margin"))
    if name == "com-amazon-sbm":
        log("        (the round-6 review measured 4.81 ms for this epoch and estimated <= 4.3 ms with the fusion: an estimate, not a bar)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="com-amazon-sbm,products-sbm,reddit-sbm,pubmed")
    ap.add_argument("--epoch-graphs", default="com-amazon-sbm,pubmed")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--route-audit", action="store_true", help="product level only (GESPMM_FUSED_ROUTE decides the route)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "fused", "timing.log"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        def log(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        log("# %s launches=%d device=%s" % (" ".join(sys.argv[1:]) or "(defaults)", args.launches, torch.cuda.get_device_name(0)))
        for name in [n for n in args.graphs.split(",") if n]:
            product_level(name, args.width, args.launches, log)
        if not args.route_audit:
            for name in [n for n in args.epoch_graphs.split(",") if n]:
                epoch_level(name, args.launches, log)


if __name__ == "__main__":
    main()
