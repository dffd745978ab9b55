"""SDDMM: every launch form, vector width, lane count and window size, each ASSERTED through gespmm_describe_sddmm, and every
result compared (a) bit for bit with the lane-order oracle at the described (V, W) — oracle.sddmm_lanes: W lane-strided fmaf
chains, then an xor butterfly — and (b) with float64 accumulation of the same products within 1e-4 * max(|ref|, sum|d1 d2|).
`out` is prefilled with NaN wherever the entry point takes an output buffer, so an edge nobody writes fails both checks."""
import ctypes
import re

import numpy as np
import pytest
import torch

from helpers import bits, cptr, cur_stream, edge_case_csr
from test_gpu_fuzz import random_csr

pytestmark = pytest.mark.gpu

SWEEP = (0, 1, 2, 3, 4, 8, 12, 16, 17, 31, 32, 33, 64, 65, 255, 256, 257, 258, 260, 511, 512, 513, 514, 516, 602, 1024, 1433, 2048)
# (V, W) at 16-byte aligned operands, by hand: V = widest of 4, 2, 1 dividing N; W = smallest power of two in 4..64 with 8 W >= N
VW = {0: (4, 4), 1: (1, 4), 2: (2, 4), 3: (1, 4), 4: (4, 4), 8: (4, 4), 12: (4, 4), 16: (4, 4), 17: (1, 4), 31: (1, 4), 32: (4, 4),
      33: (1, 8), 64: (4, 8), 65: (1, 16), 128: (4, 16), 130: (2, 32), 255: (1, 32), 256: (4, 32), 257: (1, 64), 258: (2, 64),
      260: (4, 64), 511: (1, 64), 512: (4, 64), 513: (1, 64), 514: (2, 64), 516: (4, 64), 602: (2, 64), 1024: (4, 64),
      1433: (1, 64), 2048: (4, 64)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _align(t):
    a = t.data_ptr()
    return 16 if a % 16 == 0 else (8 if a % 8 == 0 else 4)


def _shifted(t, k):
    """Same values, storage moved by k floats off a 16-byte boundary (k = 0: as allocated)."""
    if k == 0:
        return t
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _rand(rows, N, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.rand((rows, N), device="cuda", generator=g) - 0.5


def _rows_of(rowptr):
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int32), np.diff(rowptr))


def _pattern(degs, K, rng, mixed_order=False):
    degs = np.asarray(degs, dtype=np.int64)
    rowptr = np.zeros(degs.size + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    nnz = int(rowptr[-1])
    colind = rng.randint(0, K, size=nnz).astype(np.int32)
    if mixed_order:  # rows 0 mod 3 ascending, the others as drawn (unsorted, repeats), in one sort
        rows = _rows_of(rowptr).astype(np.int64)
        key = np.where(rows % 3 == 0, colind.astype(np.int64), np.arange(nnz, dtype=np.int64) - rowptr[rows])
        colind = colind[np.lexsort((key, rows))]
    return {"M": int(degs.size), "K": int(K), "nnz": nnz, "rowptr": rowptr, "colind": colind, "rows": _rows_of(rowptr)}


def _on_device(G):
    return _dev(G["rowptr"]), _dev(G["colind"]), _dev(G["rows"])


def _run(_lib, csr, idx0, ci, D1, D2):
    """The C entry point on torch's current stream, out prefilled with NaN."""
    nnz, N = ci.numel(), D1.shape[1]
    out = torch.full((nnz,), float("nan"), device="cuda")
    if csr:
        rc = _lib.lib.gespmm_sddmm_csr_f32(cptr(idx0), cptr(ci), cptr(D1), cptr(D2), cptr(out), D1.shape[0], nnz, N, cur_stream())
    else:
        rc = _lib.lib.gespmm_sddmm_coo_f32(cptr(idx0), cptr(ci), cptr(D1), cptr(D2), cptr(out), nnz, N, cur_stream())
    _lib.check(rc, "gespmm_sddmm_%s_f32" % ("csr" if csr else "coo"))
    return out


def _expect(_lib, csr, M, nnz, D1, D2, form, capturing=False, **want):
    """What the library says this call launches; it must be what the case was built to reach."""
    d = _lib.describe_sddmm(csr, M, nnz, D1.shape[1], _align(D1), _align(D2), capturing)
    assert d["form"] == form, (d, form, want)
    for k, v in want.items():
        assert d[k] == v, (d, form, want)
    return d


def _sharp(oracle, out, ri, ci, D1, D2, V, W, edges=None, what=""):
    """Bit for bit against the lane-order oracle: all edges, or the edges listed (only the operand rows they touch travel)."""
    if edges is None:
        ref = oracle.sddmm_lanes(V, W, ri.cpu().numpy(), ci.cpu().numpy(), D1.cpu().numpy(), D2.cpu().numpy())
        got = out.cpu().numpy()
    else:
        e = _dev(np.asarray(edges, dtype=np.int64))
        ru, rinv = torch.unique(ri[e], return_inverse=True)
        cu, cinv = torch.unique(ci[e], return_inverse=True)
        ref = oracle.sddmm_lanes(V, W, rinv.cpu().numpy(), cinv.cpu().numpy(), D1[ru.long()].cpu().numpy(), D2[cu.long()].cpu().numpy())
        got = out[e].cpu().numpy()
    bad = np.flatnonzero(bits(got) != bits(ref))
    assert bad.size == 0, "%s V=%d W=%d N=%d: %d of %d edges differ from the lane oracle, first %d: %r vs %r" % (
        what, V, W, D1.shape[1], bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]])


def _f64(out, ri, ci, D1, D2, what=""):
    """All edges against float64 accumulation on the device, in chunks: |out - ref| <= 1e-4 * max(|ref|, sum |d1 d2|)."""
    nnz, N = out.numel(), D1.shape[1]
    step = max(1, (1 << 24) // max(N, 1))
    nbad = torch.zeros((), dtype=torch.int64, device="cuda")
    for s in range(0, nnz, step):
        p = D1[ri[s:s + step].long()].double() * D2[ci[s:s + step].long()].double()
        ref, scale = p.sum(1), p.abs().sum(1)
        ok = (out[s:s + step].double() - ref).abs() <= 1e-4 * torch.maximum(ref.abs(), scale)  # (NaN compares false)
        nbad += (~ok).sum()
    assert int(nbad) == 0, "%s N=%d: %d of %d edges outside the float64 tolerance" % (what, N, int(nbad), nnz)


def _sample(G, rng, extra=20000):
    """Designated rows — first and last non-empty row, hub rows, the rows on both sides of every empty run — in full, plus
    `extra` seeded random edges."""
    degs = np.diff(G["rowptr"])
    ne = np.flatnonzero(degs > 0)
    empty = degs == 0
    left = np.concatenate(([True], empty[:-1]))
    right = np.concatenate((empty[1:], [True]))
    pick = (degs > 0) & (left | right | (degs >= 257))
    pick[ne[0]] = pick[ne[-1]] = True
    rows = np.flatnonzero(pick)
    e = np.concatenate([np.arange(G["rowptr"][r], G["rowptr"][r + 1]) for r in rows] + [rng.randint(0, G["nnz"], size=extra)])
    return np.unique(e)


def _check_all(oracle, G, out, dev, D1, D2, V, W, rng, what):
    rp, ci, ri = dev
    _f64(out, ri, ci, D1, D2, what)
    _sharp(oracle, out, ri, ci, D1, D2, V, W, None if G["nnz"] <= 2000000 else _sample(G, rng), what)


# ---------------------------------------------------------------------------------------------------------------- 1. widths

@pytest.mark.parametrize("which", ("edge", "random"))
def test_width_sweep_coo_and_csr(pkg, oracle, which):
    """All three V, W from 4 to 64, and the three regimes of the edge loop: one slice per row (N <= W V), slices in registers
    (N <= 512 at V = 4), the plain loop (beyond: 513, 514, 516, 602, 1024, 1433, 2048). N = 0 writes zeros."""
    from gespmm_amd import _lib, sddmm

    rng = np.random.RandomState(11)
    if which == "edge":
        G = edge_case_csr(2)
        G["rows"] = _rows_of(G["rowptr"])
    else:
        G = _pattern(rng.randint(0, 34, size=3000), 2500, rng)
        assert 45000 < G["nnz"] < 55000
    dev = _on_device(G)
    rp, ci, ri = dev
    for N in SWEEP:
        V, W = VW[N]
        D1, D2 = _rand(G["M"], N, 2 * N + 1), _rand(G["K"], N, 2 * N + 2)
        _expect(_lib, False, 0, G["nnz"], D1, D2, "coo-edge", V=V, W=W, epw=4 * 64 // W)
        _expect(_lib, True, G["M"], G["nnz"], D1, D2, "csr-edge", V=V, W=W, epw=max(16, 4 * 64 // W))
        o_coo = _run(_lib, False, ri, ci, D1, D2)
        o_csr = _run(_lib, True, rp, ci, D1, D2)
        assert torch.equal(o_coo.view(torch.int32), o_csr.view(torch.int32)), (which, N)
        _check_all(oracle, G, o_csr, dev, D1, D2, V, W, rng, "%s csr" % which)
        if N == 0:
            assert int((o_coo != 0).sum()) == 0
            assert int((sddmm.csr_sddmm(rp, ci, D1, D2) != 0).sum()) == 0 and int((sddmm.coo_sddmm(ri, ci, D1, D2) != 0).sum()) == 0


# ------------------------------------------------------------------------------------------------------------- 2. alignment

@pytest.mark.parametrize("N", (128, 512, 1024))
def test_operand_alignment_picks_the_vector_width(pkg, oracle, N):
    """N % 4 == 0 but D1, D2 or both start one or two floats off a 16-byte boundary: V drops to 1 or 2 and with it the order of
    the sum — the bits are the lane oracle's at THAT V."""
    from gespmm_amd import _lib

    rng = np.random.RandomState(12)
    G = _pattern(rng.randint(0, 34, size=3000), 2500, rng)
    dev = _on_device(G)
    rp, ci, ri = dev
    A1, A2 = _rand(G["M"], N, 31), _rand(G["K"], N, 32)
    W = VW[N][1]
    seen = set()
    for s1, s2 in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 2), (1, 2), (3, 2)):
        D1, D2 = _shifted(A1, s1), _shifted(A2, s2)
        V = 1 if (s1 % 2 or s2 % 2) else (2 if (s1 or s2) else 4)
        for csr in (False, True):
            _expect(_lib, csr, G["M"], G["nnz"], D1, D2, "csr-edge" if csr else "coo-edge", V=V, W=W)
            out = _run(_lib, csr, rp if csr else ri, ci, D1, D2)
            _check_all(oracle, G, out, dev, D1, D2, V, W, rng, "shift %d/%d %s" % (s1, s2, "csr" if csr else "coo"))
        seen.add((V, bits(out.cpu().numpy()).tobytes()))
    assert len({v for v, _ in seen}) == 3 and len(seen) == 3, "one result per V, three different ones"


# ----------------------------------------------------------------------------------------------------------- 3. CSR windows

def _window_pattern(target, epw, start_run, tail_run, seed):
    """Mean degree < 64. Empty runs of 1, epw - 1, epw, epw + 1, 300 and 5000 rows between short rows (so one wavefront's edges
    span them), one more at the start and at the tail; rows of 1; hubs of 257, 5000 (and 70 000 where the size allows); row
    boundaries at 0, +1 and -1 modulo 256 edges (every epw divides 256); nnz not a multiple of epw."""
    rng = np.random.RandomState(seed)
    degs = [np.zeros(start_run, dtype=np.int64)]
    total = [0]

    def add(a):
        a = np.asarray(a, dtype=np.int64)
        degs.append(a)
        total[0] += int(a.sum())

    def filler(n):
        add(rng.randint(1, 48, size=max(1, n // 24)))

    hubs = [257, 5000] + ([70000] if target >= 1000000 else [])
    body = target - sum(hubs)
    for i, run in enumerate((1, epw - 1, epw, epw + 1, 300, 5000)):
        filler(body // 8)
        add([1, 2, 1])
        degs.append(np.zeros(run, dtype=np.int64))
        add([1, 1, 3, 1])
        if i < len(hubs):
            filler(body // 16)
            add([hubs[i]])
    for rem in (0, 1, 255):  # the next row starts exactly on / one past / one before a multiple of 256 edges
        filler(body // 16)
        add([(rem - total[0]) % 256 + 256])
        add([1, 5, 1])
    filler(max(24, target - total[0]))
    if total[0] % 256 == 0:
        add([1])
    degs.append(np.zeros(tail_run, dtype=np.int64))
    G = _pattern(np.concatenate(degs), 60000, rng)
    assert G["nnz"] // G["M"] < 64 and G["nnz"] % epw != 0
    return G


@pytest.mark.parametrize("target,lo,hi", ((50000, 0, 1 << 20), (1300000, 1 << 20, 1 << 22), (4500000, 1 << 22, 1 << 31)))
def test_csr_row_pointer_windows(pkg, oracle, target, lo, hi):
    """The CSR edge-parallel kernel at 16..64, 64 and 256 edges per wavefront: the LDS window of row pointers, its search, the
    fallback for more than epw empty rows inside one wavefront's edges, the padding past rowptr[M]. CSR == COO == lane oracle."""
    from gespmm_amd import _lib

    for k, N in enumerate((3, 128, 602)):
        V, W = VW[N]
        epw = 256 if lo >= (1 << 22) else 64 if lo >= (1 << 20) else max(16, 4 * 64 // W)
        start_run, tail_run = ((epw + 1, 1), (epw, 5000), (5000, epw - 1))[k]
        G = _window_pattern(target, epw, start_run, tail_run, seed=100 + k)
        assert lo <= G["nnz"] < hi, G["nnz"]
        # the pattern reaches the fallback: some wavefront's edges span more than epw + 1 row pointers
        e_lo = np.arange(0, G["nnz"], epw)
        r0 = np.searchsorted(G["rowptr"], e_lo, side="right") - 1
        r1 = np.searchsorted(G["rowptr"], np.minimum(e_lo + epw, G["nnz"]) - 1, side="right") - 1
        assert np.any(r1 - r0 >= epw + 1) and np.any(r1 == r0), "no wavefront spans an empty run / lies inside one row"
        if k == 0:
            assert np.any(r0 + epw + 1 > G["M"]), "no window reaches past rowptr[M]"
        rng = np.random.RandomState(200 + k)
        dev = _on_device(G)
        rp, ci, ri = dev
        D1, D2 = _rand(G["M"], N, 41 + k), _rand(G["K"], N, 51 + k)
        _expect(_lib, True, G["M"], G["nnz"], D1, D2, "csr-edge", V=V, W=W, epw=epw)
        _expect(_lib, False, 0, G["nnz"], D1, D2, "coo-edge", V=V, W=W, epw=4 * 64 // W)
        o_csr = _run(_lib, True, rp, ci, D1, D2)
        o_coo = _run(_lib, False, ri, ci, D1, D2)
        assert torch.equal(o_csr.view(torch.int32), o_coo.view(torch.int32)), (target, N)
        _check_all(oracle, G, o_csr, dev, D1, D2, V, W, rng, "windows %d" % target)
        del D1, D2, o_csr, o_coo


# -------------------------------------------------------------------------------------------------------------- 4. row walk

@pytest.mark.parametrize("N", (65, 128, 130, 513, 514, 1024))
def test_row_walk(pkg, oracle, N):
    """Mean degree >= 64 and one slab: a row per wavefront. Rows of 0, 1, 63, 64, 65, 129 entries (the 64-column staging
    step and its neighbours) and a 5000-entry hub; slices in registers (65, 128, 130) and the plain loop (513, 514, 1024);
    V = 1 (65, 513), 2 (130, 514) and 4."""
    from gespmm_amd import _lib

    rng = np.random.RandomState(13)
    degs = np.concatenate(([0, 1, 63, 64, 65, 129, 0, 0, 5000, 1], rng.randint(64, 131, size=300), [0, 129, 0]))
    G = _pattern(degs, 777, rng, mixed_order=True)
    dev = _on_device(G)
    rp, ci, ri = dev
    V, W = VW[N]
    D1, D2 = _rand(G["M"], N, 61), _rand(G["K"], N, 62)
    _expect(_lib, True, G["M"], G["nnz"], D1, D2, "row-walk", V=V, W=W)
    out = _run(_lib, True, rp, ci, D1, D2)
    _check_all(oracle, G, out, dev, D1, D2, V, W, rng, "row-walk")
    assert torch.equal(out.view(torch.int32), _run(_lib, False, ri, ci, D1, D2).view(torch.int32))


# --------------------------------------------------------------------------------------------------------------- 5. blocked

def _dense_pattern(M, avg, K, seed):
    rng = np.random.RandomState(seed)
    degs = rng.randint(avg - 6, avg + 7, size=M)
    degs[::997] = 0
    degs[7] = 5000
    degs[M - 2] = 1
    G = _pattern(degs, K, rng, mixed_order=True)
    assert G["nnz"] // M >= 64
    return G


# N, M, mean degree, K / M, nslab, slab_rows = max(64, 6 MiB / 4N): V = 4 (256; 1024 = plain loop), V = 2 (514), V = 1 (65, 513);
# 4 slabs and >= 8; square, K = 3 M (columns past M: the clamped last slab) and K = M / 3 (the late slabs stay empty)
BLOCKED = ((256, 20000, 70, 1, 4, 6144), (1024, 6000, 70, 3, 4, 1536), (1024, 12000, 70, 1, 8, 1536), (514, 10000, 70, 1 / 3, 4, 3060),
           (514, 22000, 70, 1, 8, 3060), (65, 80000, 80, 1, 4, 24197), (513, 15000, 70, 3, 5, 3066), (513, 24000, 70, 1 / 3, 8, 3066))


@pytest.mark.parametrize("N,M,avg,kf,nslab,slab_rows", BLOCKED)
def test_cache_blocked_form(pkg, oracle, N, M, avg, kf, nslab, slab_rows):
    from gespmm_amd import _lib

    G = _dense_pattern(M, avg, int(M * kf), seed=N + M)
    if kf > 1:
        assert (G["colind"] >= M).mean() > 0.5
    rng = np.random.RandomState(14)
    dev = _on_device(G)
    rp, ci, ri = dev
    V, W = VW[N]
    D1, D2 = _rand(G["M"], N, 71), _rand(G["K"], N, 72)
    _expect(_lib, True, M, G["nnz"], D1, D2, "blocked", V=V, W=W, nslab=nslab, slab_rows=slab_rows)
    out = _run(_lib, True, rp, ci, D1, D2)
    _check_all(oracle, G, out, dev, D1, D2, V, W, rng, "blocked nslab=%d K=%d" % (nslab, G["K"]))
    assert torch.equal(out.view(torch.int32), _run(_lib, False, ri, ci, D1, D2).view(torch.int32))


# --------------------------------------------------------------------------------------------------------------- 6. capture

def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up on the side stream (code objects, a plan's buffers)
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_captured_call_skips_the_blocked_form(pkg, oracle):
    """The blocked form allocates, so a capturing stream gets the row walk: same bits. Replays see new operand contents."""
    from gespmm_amd import _lib, sddmm

    N, M = 1024, 6000
    G = _dense_pattern(M, 70, M, seed=5)
    dev = _on_device(G)
    rp, ci, ri = dev
    D1, D2 = _rand(M, N, 81), _rand(M, N, 82)
    _expect(_lib, True, M, G["nnz"], D1, D2, "blocked", V=4, W=64, nslab=4)
    _expect(_lib, True, M, G["nnz"], D1, D2, "row-walk", capturing=True, V=4, W=64)
    graph, out = _capture(lambda: sddmm.csr_sddmm(rp, ci, D1, D2))
    for seed in (83, 85):
        D1.copy_(_rand(M, N, seed))
        D2.copy_(_rand(M, N, seed + 1))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(_lib, True, rp, ci, D1, D2)  # blocked
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)), seed
        _f64(out, ri, ci, D1, D2, "captured")
        _sharp(oracle, out, ri, ci, D1, D2, 4, 64, what="captured")


def test_captured_call_through_a_plan(pkg, oracle):
    """A plan on the clustered edge order (route 2) whose buffers the warm-up built: the capture holds two kernels."""
    from gespmm_amd import _lib, graphs, sddmm, spmm

    g = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda")
    rp, ci, M, K, N = g["rowptr"], g["colind"], g["M"], g["K"], 128
    ri = _dev(_rows_of(rp.cpu().numpy()))
    plan = spmm.SpmmPlan(rp, ci, K, N, reorder=True)
    assert _lib.lib.gespmm_plan_sddmm_route(plan._handle, N) == 2, plan.describe()
    D1, D2 = _rand(M, N, 91), _rand(K, N, 92)
    _expect(_lib, False, 0, g["nnz"], D1, D2, "coo-edge", V=4, W=16, epw=16)
    graph, out = _capture(lambda: sddmm.csr_sddmm(rp, ci, D1, D2, plan=plan))
    for seed in (93, 95):
        D1.copy_(_rand(M, N, seed))
        D2.copy_(_rand(K, N, seed + 1))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _f64(out, ri, ci, D1, D2, "captured plan")
        _sharp(oracle, out, ri, ci, D1, D2, 4, 16, what="captured plan")


# ----------------------------------------------------------------------------------------------------------- 7. plan routes

def test_plan_routes(pkg, oracle, bundled):
    """gespmm_plan_sddmm_f32 on its three routes — 0 the CSR call, 1 COO on row ids expanded once, 2 the clustered edge order
    and a scatter — each asserted through gespmm_plan_sddmm_route, each called twice with different operands (the second call
    reuses the plan's row ids / temporaries), against the lane oracle."""
    from gespmm_amd import _lib, graphs, spmm

    rng = np.random.RandomState(15)
    sbm = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda")
    dense = _pattern(rng.randint(28, 50, size=4000), 4000, rng)
    assert dense["nnz"] // dense["M"] >= 32
    pub = bundled["pubmed"]
    cases = (("pubmed", _dev(pub["rowptr"]), _dev(pub["colind"]), pub["M"], pub["K"], True),
             ("com-amazon-sbm", sbm["rowptr"], sbm["colind"], sbm["M"], sbm["K"], True),
             ("dense", _dev(dense["rowptr"]), _dev(dense["colind"]), dense["M"], dense["K"], False))
    routes = set()
    for name, rp, ci, M, K, reorder in cases:
        rph = rp.cpu().numpy()
        nnz = int(rph[-1])
        ri = _dev(_rows_of(rph))
        for N in (3, 64, 128, 602):
            plan = spmm.SpmmPlan(rp, ci, K, N, reorder=reorder)
            route = _lib.lib.gespmm_plan_sddmm_route(plan._handle, N)
            # the documented rule on the facts the plan itself reports: clustered order, modelled hits >= 0.40 and N >= 64 -> 2;
            # else mean degree < 32 -> 1, else 0. One route per (graph, N); describe prints the hits with three decimals.
            desc = plan.describe()
            hits = float(re.search(r"l2_model=[-0-9.]+->([-0-9.]+)", desc).group(1))
            clustered = " levels=" in desc
            short = 1 if nnz // M < 32 else 0
            want = 2 if (clustered and hits >= 0.40 and N >= 64) else short
            print("plan route: %s N=%d route=%d (hits %.3f, clustered %d)" % (name, N, route, hits, clustered))
            if abs(hits - 0.40) > 0.0006:
                assert route == want, (name, N, route, desc)
            assert route == {"dense": 0, "com-amazon-sbm": 1 if N < 64 else route, "pubmed": 1 if N < 64 else route}[name], (name, N, route, desc)
            routes.add(route)
            V, W = VW[N]
            for call in range(2):
                D1, D2 = _rand(M, N, 7 * N + call), _rand(K, N, 7 * N + 3 + call)
                if route == 0:
                    _expect(_lib, True, M, nnz, D1, D2, "csr-edge", V=V, W=W)
                else:
                    _expect(_lib, False, 0, nnz, D1, D2, "coo-edge", V=V, W=W)
                out = torch.full((nnz,), float("nan"), device="cuda")
                _lib.check(_lib.lib.gespmm_plan_sddmm_f32(plan._handle, cptr(D1), cptr(D2), cptr(out), N, cur_stream()), "gespmm_plan_sddmm_f32")
                _f64(out, ri, ci, D1, D2, "%s route %d call %d" % (name, route, call))
                _sharp(oracle, out, ri, ci, D1, D2, V, W, what="%s route %d call %d" % (name, route, call))
            # the checks of the stateless entry points, on every route: an operand off a float boundary is refused
            odd = ctypes.c_void_p(D1.data_ptr() + 2)
            assert _lib.lib.gespmm_plan_sddmm_f32(plan._handle, odd, cptr(D2), cptr(out), N, cur_stream()) == -2
            assert _lib.lib.gespmm_plan_sddmm_f32(plan._handle, cptr(D1), cptr(D2), None, N, cur_stream()) == -1
            assert _lib.lib.gespmm_plan_sddmm_f32(plan._handle, cptr(D1), cptr(D2), cptr(out), 1 << 30, cur_stream()) == -3
            if name == "com-amazon-sbm" and N == 128:
                assert route == 2, plan.describe()  # (communities of ~1000 rows: the clustered walk — profiles/r03/sddmm_audit.log)
            del plan
    assert routes == {0, 1, 2}


# ------------------------------------------------------------------------------------------------------------------ 8. fuzz

def _long_empty_runs(rng):
    M = int(rng.choice([70, 300, 1000, 2500]))
    degs = np.zeros(M, dtype=np.int64)
    k = int(rng.randint(1, 12))
    at = rng.randint(0, M, size=k)
    degs[at] = rng.choice([1, 1, 2, 5, 17, 64, 300], size=k)
    K = int(rng.choice([1, 64, 1000]))
    return _pattern(degs, K, rng)


def test_seeded_fuzz(pkg, oracle):
    from gespmm_amd import _lib

    rng = np.random.RandomState(20261017)
    forms = set()
    launched = 0
    for case in range(400):  # (about one in six patterns is empty: > 300 cases launch)
        if rng.rand() < 0.3:
            G, law = _long_empty_runs(rng), "empty-runs"
        else:
            G, law = random_csr(rng)
            G["rows"] = _rows_of(G["rowptr"])
        N = int(rng.choice(SWEEP))
        csr = bool(rng.rand() < 0.5)
        s1, s2 = (int(x) for x in rng.choice([0, 0, 0, 1, 2, 3], size=2))
        D1 = _shifted(_dev(oracle.hash_B(G["M"], N, seed=case)), s1 if N else 0)
        D2 = _shifted(_dev((rng.rand(G["K"], N).astype(np.float32) - np.float32(0.5)) * np.float32(3)), s2 if N else 0)
        rp, ci, ri = _on_device(G)
        d = _lib.describe_sddmm(csr, G["M"], G["nnz"], N, _align(D1), _align(D2))
        if G["nnz"] == 0:
            assert d["form"] == "none"
            assert _run(_lib, csr, rp if csr else ri, ci, D1, D2).numel() == 0
            continue
        assert d["form"] in (("csr-edge", "row-walk") if csr else ("coo-edge",)), (case, law, d)
        amax = 4 if (s1 % 2 or s2 % 2) and N else 8 if (s1 or s2) and N else 16
        assert d["V"] == max(v for v in (1, 2, 4) if N % v == 0 and amax % (4 * v) == 0) and d["W"] == VW.get(N, (0, d["W"]))[1], (case, d)
        forms.add((d["form"], d["V"], d["W"]))
        out = _run(_lib, csr, rp if csr else ri, ci, D1, D2)
        launched += 1
        _f64(out, ri, ci, D1, D2, "fuzz %d %s" % (case, law))
        _sharp(oracle, out, ri, ci, D1, D2, d["V"], d["W"], what="fuzz %d %s %s" % (case, law, d))
    assert launched >= 300, launched
    assert {f for f, _, _ in forms} == {"coo-edge", "csr-edge", "row-walk"} and len(forms) >= 25, sorted(forms)


# -------------------------------------------------------------------------------------------------------------- 9. autograd

def test_edge_weight_gradient_at_a_first_layer_width(pkg, oracle, bundled):
    """SPMMFunction's edge-weight gradient at hidden 602 (reddit's feature width: N > 512, the plain loop, V = 2) on pubmed:
    grad_w[e] = <grad_out[row(e)], feat[col(e)]>, against float64 and the lane oracle."""
    import gespmm_amd
    from gespmm_amd import _lib, graphs

    G = bundled["pubmed"]
    rp, ci = _dev(G["rowptr"]), _dev(G["colind"])
    ri = _dev(_rows_of(G["rowptr"]))
    colptr, rowind = graphs.transpose_csr(rp, ci)
    w = _rand(1, G["nnz"], 101).reshape(-1)
    _, _, w_csc = graphs.transpose_csr(rp, ci, val=w)
    x = _rand(G["K"], 602, 102).requires_grad_(True)
    go = _rand(G["M"], 602, 103)
    ww = w.clone().requires_grad_(True)
    y = gespmm_amd.SPMMFunction.apply(rp, ci, colptr, rowind, x, ww, w_csc, True)
    y.backward(go)
    assert ww.grad is not None and ww.grad.shape == (G["nnz"],)
    xd = x.detach()
    d = _expect(_lib, True, G["M"], G["nnz"], go, xd, "csr-edge", V=2, W=64, epw=16)
    _f64(ww.grad, ri, ci, go, xd, "autograd")
    _sharp(oracle, ww.grad, ri, ci, go, xd, d["V"], d["W"], what="autograd")
