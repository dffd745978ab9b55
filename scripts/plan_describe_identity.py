#!/usr/bin/env python3
"""describe() and a checksum of C for a fixed, seeded set of plans (the bundled graphs and two synthetic ones; device and host analysis;
AUTO and each explicit kernel; N in 16 32 64 128 130 256; valued and not; the max reducer; before and after tune), timing fields masked.
For comparing two builds of the library — e.g. a refactor against a checkout of its parent built beside it: run once per tree and
compare the two files byte for byte.    python scripts/plan_describe_identity.py <tree root> <out file>"""
import hashlib
import os
import re
import sys

root, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
import numpy as np
import torch

import gespmm_amd
from gespmm_amd import graphs, spmm

assert os.path.abspath(gespmm_amd.__file__).startswith(root), gespmm_amd.__file__
MASK = [(r"analysis=[0-9.]+s", "analysis=#s"), (r"tables=[0-9.]+s", "tables=#s"), (r"clustering [0-9.]+s", "clustering #s"),
        (r"tuned\[us: [^\]]*\]", "tuned[us: #]")]


def mask(d):
    for a, b in MASK:
        d = re.sub(a, b, d)
    return d


def digest(t):
    return hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()[:16]


dev = "cuda"
gs = {}
for name in ("cora", "citeseer", "pubmed"):
    g = graphs.load_mtx_as_csr(os.path.join(root, "tests", "golden", name + ".mtx"))
    gs[name] = (torch.from_numpy(g["rowptr"]).to(dev), torch.from_numpy(g["colind"]).to(dev), g["K"])
for name in ("com-amazon-sbm", "com-amazon-like"):
    g = graphs.synthetic_graph(name, seed=42, device=dev)
    gs[name] = (g["rowptr"], g["colind"], g["M"])
lines = []
for name, (rp, ci, K) in gs.items():
    nnz = ci.numel()
    big = nnz > 1000000
    gen = torch.Generator(device="cpu").manual_seed(7)
    val = (torch.rand(nnz, generator=gen) - 0.5).to(dev)
    for N in (16, 32, 64, 128, 130, 256):
        gen = torch.Generator(device="cpu").manual_seed(N)
        B = ((torch.randint(0, 100, (K, N), generator=gen, dtype=torch.int32) - 50).float() / 100).to(dev)
        for analysis in ("device", "host"):
            if big and analysis == "host" and N not in (32, 128):
                continue
            for kernel in ("auto", "stream", "seg-stream", "staged", "records", "staged-slabs"):
                if big and kernel in ("stream", "seg-stream") and N not in (32, 128):
                    continue
                for reorder in (("auto", True) if kernel == "auto" else (True,)):
                    for valued in (True, False):
                        tag = "%s N=%d %s %s reorder=%s valued=%d" % (name, N, analysis, kernel, reorder, valued)
                        try:
                            plan = spmm.SpmmPlan(rp, ci, K, N, values=val if valued else None, reorder=reorder, kernel=kernel, analysis=analysis)
                        except Exception as ex:  # an option the width does not admit: recorded as such
                            lines.append("%s | create: %s" % (tag, type(ex).__name__))
                            continue
                        C = plan.run(val if valued else None, B)
                        lines.append("%s | %s | C=%s" % (tag, mask(plan.describe()), digest(C)))
                        if not valued:
                            Cm = plan.run(None, B, reduce_max=-10000.0)
                            lines.append("%s | max C=%s" % (tag, digest(Cm)))
                        if kernel == "auto":
                            Ct = plan.tune(B, reps=2)
                            d = plan.describe()
                            winner = ""
                            if "tuned[us: " in d:  # (which candidates were measured — the times themselves are masked)
                                winner = " measured=" + ",".join("1" if float(x.split("=")[1]) > 0 else "0" for x in d.split("tuned[us: ")[1].split("]")[0].split())
                            C2 = plan.run(val if valued else None, B)
                            lines.append("%s | after tune: C=%s again=%s%s" % (tag, digest(Ct), digest(C2), winner))
                        del plan
torch.cuda.synchronize()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote %d lines to %s" % (len(lines), out_path))
