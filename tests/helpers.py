"""Shared helpers for the test-suite (plain module: tests/ is on sys.path)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def edge_case_csr(seed=0):
    """Hand-shaped CSR the reference never tests (SURVEY.md §8 c3 iii): empty rows, rows
    of exactly 1/63/64/65/127/128/129/200 entries, an empty tail, M not a multiple of
    any block size, rectangular (K != M), unsorted columns and repeated columns."""
    rng = np.random.RandomState(seed)
    K = 301
    degs = [0, 1, 63, 64, 65, 0, 0, 127, 128, 129, 200, 2, 3, 0, 5, 31, 32, 33, 7, 0, 0]
    rowptr = np.zeros(len(degs) + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    colind = rng.randint(0, K, size=int(rowptr[-1])).astype(np.int32)  # unsorted, with repeats
    return {"M": len(degs), "K": K, "nnz": int(rowptr[-1]), "rowptr": rowptr, "colind": colind}


def sampled_rows_equal_oracle(oracle, rowptr, colind, val, B, C, nrows=512, seed=0):
    """`nrows` sampled rows of C = A @ B (device tensors) against the oracle's device-arithmetic chain on the extracted
    sub-matrix, bit for bit. Only the B rows those CSR rows touch travel to the host."""
    import torch

    M = rowptr.numel() - 1
    rng = np.random.RandomState(seed)
    rows = np.sort(rng.choice(M, min(nrows, M), replace=False))
    rph = rowptr.cpu().numpy()
    sub_ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    sub_ptr[1:] = np.cumsum(rph[rows + 1] - rph[rows])
    sel = torch.from_numpy(np.concatenate([np.arange(rph[r], rph[r + 1]) for r in rows]).astype(np.int64)).to(colind.device)
    cih = colind[sel].cpu().numpy()
    vh = val[sel].cpu().numpy() if val is not None else None
    cols_u, inv = np.unique(cih, return_inverse=True)
    Bsub = B[torch.from_numpy(cols_u.astype(np.int64)).to(B.device)].cpu().numpy()
    ref = oracle.spmm(sub_ptr, inv.astype(np.int32), vh, Bsub, "fma" if vh is not None else "golden")
    got = C[torch.from_numpy(rows).to(C.device)].cpu().numpy()
    return bool(np.array_equal(bits(got), bits(ref)))


# ---- the stateless entry points and their never-planned reference (tests/test_gpu_auto_plan*.py, scripts/auto_plan_soak.py) ----------
# Every helper runs on torch's CURRENT stream: callers pick the stream with `with torch.cuda.stream(s)`.

def cptr(t):
    import ctypes

    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def cur_stream():
    import ctypes

    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan_like_product(rp, B):
    import torch

    return torch.full((rp.numel() - 1, B.shape[1]), float("nan"), device=B.device)


def plain_product(_lib, rp, ci, val, B, out=None):
    """The reference product: the _cfg entry point is never planned."""
    import ctypes

    M, (K, N) = rp.numel() - 1, B.shape
    C = nan_like_product(rp, B) if out is None else out
    cfg = _lib.LaunchCfg(0, 0, 0, 0, 0, 0)
    _lib.check(_lib.lib.gespmm_csr_spmm_f32_cfg(cptr(rp), cptr(ci), cptr(val), cptr(B), cptr(C), M, K, N, ci.numel(), -1, ctypes.byref(cfg),
                                                cur_stream()), "gespmm_csr_spmm_f32_cfg")
    return C


def auto_call(_lib, rp, ci, val, B, out=None, op="sum"):
    """One stateless call (the entry points gespmm_set_auto_plan serves): op = "sum" (gespmm_csr_spmm_f32, valued or not), "max"
    (gespmm_csr_spmm_max_f32, -10000 for empty rows) or "dgl" (gespmm_dgl_csrmm_sum_f32). C is prefilled with NaN: a row nobody
    writes does not compare equal."""
    M, (K, N) = rp.numel() - 1, B.shape
    C = nan_like_product(rp, B) if out is None else out
    if op == "sum":
        rc = _lib.lib.gespmm_csr_spmm_f32(cptr(rp), cptr(ci), cptr(val), cptr(B), cptr(C), M, K, N, ci.numel(), -1, cur_stream())
    elif op == "max":
        rc = _lib.lib.gespmm_csr_spmm_max_f32(cptr(rp), cptr(ci), cptr(B), cptr(C), M, K, N, ci.numel(), -10000.0, -1, cur_stream())
    elif op == "dgl":
        rc = _lib.lib.gespmm_dgl_csrmm_sum_f32(M, N, cptr(rp), cptr(ci), cptr(B), cptr(C), cur_stream())
    else:
        raise ValueError(op)
    _lib.check(rc, "auto_call " + op)
    return C


def mismatches(got, want):
    """Number of differing 32-bit words, as a device scalar (stream-ordered, no synchronisation)."""
    import torch

    return (got.view(torch.int32) != want.view(torch.int32)).sum()


def stats_delta(after, before):
    return {k: after[k] - before[k] for k in after if k != "cached_plans"}


def sleep_cycles_per_ms():
    """Clock rate of torch.cuda._sleep (a bounded spin on the device), measured with a pair of events."""
    import torch

    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(2_000_000)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None or ms < best else best
    return 2_000_000 / max(best, 1e-3)


def gate(cycles_per_ms, ms):
    """Holds the current stream back for about `ms` milliseconds without any host wait; returns the event recorded at its end."""
    import torch

    torch.cuda._sleep(max(1, int(cycles_per_ms * ms)))
    ev = torch.cuda.Event()
    ev.record()
    return ev


def auto_plan_soak(_lib, g, seed, steps, cycles_per_ms, N=128, k=2, ops=("sum_v", "sum", "max", "dgl")):
    """Seeded random stateless calls on two streams against the auto-plan cache. Operations: a call (valued / unweighted sum, max
    reducer, DGL sum), a weight flip in place, a switch of the value pointer, an in-place pattern edit (the columns of two entries in
    different rows swap; a second edit swaps them back), a new dense operand, a short gate, now and then a synchronisation of the device.

    Ordering: a mutation of the shared arrays on stream X follows X.wait_stream(Y), and Y's next operation waits on X — the state each
    call sees is then the host's sequence. The expected products of every state are made first with the switch off. Each call's
    mismatch count goes into a device tensor on the call's own stream; nothing synchronises per call.

    Returns (failures, stats delta, number of calls); failures = [(step, stream, op, state, mismatching words)]."""
    import torch

    rng = np.random.RandomState(seed)
    rp, ci, K, nnz = g["rowptr"], g["colind"], g["K"], g["nnz"]
    rph = rp.cpu().numpy()
    # the pattern edit: two non-empty rows, two entries with different columns
    while True:
        r1, r2 = (int(x) for x in rng.randint(0, rph.size - 1, size=2))
        if r1 != r2 and rph[r1 + 1] > rph[r1] and rph[r2 + 1] > rph[r2]:
            p1, p2 = int(rng.randint(rph[r1], rph[r1 + 1])), int(rng.randint(rph[r2], rph[r2 + 1]))
            c1, c2 = int(ci[p1]), int(ci[p2])
            if c1 != c2:
                break
    ci_orig = ci.clone()
    idx = torch.tensor([p1, p2], dtype=torch.int64, device=ci.device)
    pat_cols = [torch.tensor([c1, c2], dtype=torch.int32, device=ci.device), torch.tensor([c2, c1], dtype=torch.int32, device=ci.device)]
    W = [torch.from_numpy((rng.rand(nnz).astype(np.float32) - 0.5) * float(s)).to(ci.device) for s in (1.0, -3.0, 0.25)]
    Bs = [torch.from_numpy(rng.rand(K, N).astype(np.float32) - 0.5).to(ci.device) for _ in range(2)]
    _lib.set_auto_plan(0)
    torch.cuda.synchronize()
    want = {}
    for pat in (0, 1):
        ci.index_copy_(0, idx, pat_cols[pat])
        for b in range(2):
            for w in range(3):
                if "sum_v" in ops:
                    want[("sum_v", pat, w, b)] = plain_product(_lib, rp, ci, W[w], Bs[b])
            for op in ops:
                if op != "sum_v":
                    want[(op, pat, 0, b)] = auto_call(_lib, rp, ci, None, Bs[b], op=("sum" if op == "sum" else op))
    ci.index_copy_(0, idx, pat_cols[0])
    torch.cuda.synchronize()
    bufs = [W[0].clone(), W[1].clone()]
    state = {"pat": 0, "w": [0, 1], "cur": 0, "b": 0}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    owes = [False, False]  # owes[s]: stream s must wait on the other before its next operation
    counts = torch.zeros(steps, dtype=torch.int64, device=ci.device)
    log = []
    before = _lib.auto_plan_stats()
    _lib.set_auto_plan(k)
    ncalls = 0
    for step in range(steps):
        s = int(rng.randint(2))
        S, O = streams[s], streams[1 - s]
        with torch.cuda.stream(S):
            if owes[s]:
                S.wait_stream(O)
                owes[s] = False
            u = rng.rand()
            if u < 0.55:
                op = ops[int(rng.randint(len(ops)))]
                w = state["w"][state["cur"]] if op == "sum_v" else 0
                key = (op, state["pat"], w, state["b"])
                out = nan_like_product(rp, Bs[state["b"]])
                auto_call(_lib, rp, ci, bufs[state["cur"]] if op == "sum_v" else None, Bs[state["b"]], out=out,
                          op=("sum" if op in ("sum", "sum_v") else op))
                counts[step] = mismatches(out, want[key])
                log.append((step, s, op, key))
                ncalls += 1
                del out
            elif u < 0.80:
                kind = "flip" if u < 0.68 else ("pattern" if u < 0.74 else "pointer")
                S.wait_stream(O)  # a mutation of the shared arrays: after everything the other stream has queued ...
                owes[1 - s] = True  # ... and before anything it queues next
                if kind == "flip":
                    w = int(rng.randint(3))
                    bufs[state["cur"]].copy_(W[w])
                    state["w"][state["cur"]] = w
                elif kind == "pattern":
                    state["pat"] ^= 1
                    ci.index_copy_(0, idx, pat_cols[state["pat"]])
                else:
                    state["cur"] ^= 1
                log.append((step, s, kind, None))
            elif u < 0.88:
                state["b"] ^= 1
                log.append((step, s, "new B", None))
            elif u < 0.98:
                torch.cuda._sleep(max(1, int(cycles_per_ms * float(rng.uniform(0.05, 3.0)))))
                log.append((step, s, "gate", None))
            else:
                torch.cuda.synchronize()
                log.append((step, s, "sync", None))
    torch.cuda.synchronize()
    delta = stats_delta(_lib.auto_plan_stats(), before)
    _lib.set_auto_plan(0)
    ci.copy_(ci_orig)
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    failures = [(st, s, op, key, int(c[st])) for (st, s, op, key) in log if key is not None and c[st] != 0]
    return failures, delta, ncalls
