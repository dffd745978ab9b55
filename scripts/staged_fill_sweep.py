"""Fill window sweep on one graph: plans with GESPMM_STAGED_FILL = each window, timed alternately.
python scripts/staged_fill_sweep.py GRAPH N windows(comma) [kernel] [rounds]   (GRAPH: a stand-in of gespmm_amd/graphs.py, planted:STAND-IN = the stand-in relabelled in its planted order, or holdout:NAME = $GESPMM_HOLDOUT_DIR/NAME.npz of scripts/holdout_graphs.py)"""
import os, statistics, sys, time
import torch
sys.path.insert(0, ".")
sys.path.insert(0, "scripts")
import gespmm_amd
from gespmm_amd import graphs, spmm

name = sys.argv[1]
N = int(sys.argv[2])
windows = [int(x) for x in sys.argv[3].split(",")]
kern = sys.argv[4] if len(sys.argv) > 4 else "auto"
rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 7

if name.startswith("holdout:"):
    import numpy as np
    z = np.load(os.path.join(os.environ.get("GESPMM_HOLDOUT_DIR", "profiles/r05/holdout"), name.split(":", 1)[1] + ".npz"))
    n = int(z["n"])
    u = torch.from_numpy(np.concatenate([z["lo"], z["hi"]]).astype(np.int64)).cuda()
    v = torch.from_numpy(np.concatenate([z["hi"], z["lo"]]).astype(np.int64)).cuda()
    key = torch.unique(u * n + v)
    u, v = key // n, key % n
    rpt = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rpt[1:] = torch.cumsum(torch.bincount(u, minlength=n), 0)
    g = {"rowptr": rpt.to(torch.int32), "colind": v.to(torch.int32), "M": n, "K": n, "nnz": int(v.numel())}
elif name.startswith("planted:"):  # the stand-in ARRIVING in its planted order (the plan keeps the caller's order)
    g = graphs.synthetic_graph(name.split(":", 1)[1], seed=42, device="cuda")
    g["rowptr"], g["colind"] = graphs.relabel_by_order(g["rowptr"], g["colind"], torch.argsort(g["truth"]))
else:
    g = graphs.synthetic_graph(name, seed=42, device="cuda")
rp, ci, M, K, nnz = g["rowptr"], g["colind"], g["M"], g["K"], g["nnz"]
torch.manual_seed(1)
val = torch.rand(nnz, device="cuda") - 0.5
B = torch.rand(K, N, device="cuda") - 0.5
C = torch.empty(M, N, device="cuda")
plans = {}
for rep in range(2):  # (second creation: warm analysis)
    for w in windows:
        os.environ["GESPMM_STAGED_FILL"] = str(w)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = spmm.SpmmPlan(rp, ci, K, N, values=val, kernel=kern)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        plans[w] = (p, ms)
ref = None
for w in windows:
    p, ms = plans[w]
    spmm.csr_spmm(rp, ci, val, B, out=C, plan=p)
    if ref is None:
        ref = C.clone()
    same = bool(torch.equal(C.view(torch.int32), ref.view(torch.int32)))
    d = p.describe()
    print("rows_env=%s %s N=%d w=%d plan_ms=%.2f bits=%s | %s" % (os.environ.get("GESPMM_STAGED_ROWS", "-"), name, N, w, ms, same,
          d.split("kernel=")[1][:150] if "kernel=" in d else d[:150]), flush=True)
reps = 100
res = {w: [] for w in windows}
for r in range(rounds):
    for w in windows:
        p = plans[w][0]
        for _ in range(5):
            spmm.csr_spmm(rp, ci, val, B, out=C, plan=p)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            spmm.csr_spmm(rp, ci, val, B, out=C, plan=p)
        b.record()
        torch.cuda.synchronize()
        res[w].append(a.elapsed_time(b) * 1e3 / reps)
for w in windows:
    v = res[w]
    print("RESULT rows_env=%s %s N=%d kernel=%s w=%d us/launch min=%.2f med=%.2f max=%.2f" % (
        os.environ.get("GESPMM_STAGED_ROWS", "-"), name, N, kern, w, min(v), statistics.median(v), max(v)), flush=True)
