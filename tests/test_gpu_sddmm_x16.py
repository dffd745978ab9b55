"""16-bit SDDMM (fp16 / bf16 D1 and D2, fp32 out) on the GPU: every launch form, V = 1 / 2 / 4 / 8, W = 4 .. 64 and the three
regimes of the edge loop, each ASSERTED through gespmm_describe_sddmm_x16, and every result compared (a) bit for bit with the
lane-order oracle (oracle_sddmm_lanes, the C function: it takes V = 8) at the described (V, W) on the operands widened to fp32, and
(b) with float64 accumulation of the same products within 1e-4 * max(|ref|, sum |d1 d2|). `out` is prefilled with NaN wherever the
entry point takes an output buffer, so an edge nobody writes fails both checks. Shapes are the smallest that reach each path."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import bits, cptr, cur_stream, edge_case_csr
from test_gpu_sddmm_forms import _capture, _dense_pattern, _dev, _f64, _on_device, _pattern, _rows_of, _sample, _window_pattern
from test_sddmm_x16_host import VW16, _lanes

pytestmark = pytest.mark.gpu

F16, BF16 = 1, 2
DT = {F16: torch.float16, BF16: torch.bfloat16}
CODE = {torch.float16: F16, torch.bfloat16: BF16}
SWEEP = (0, 1, 2, 3, 4, 8, 12, 16, 32, 33, 36, 40, 64, 65, 72, 128, 130, 255, 256, 258, 260, 511, 512, 513, 514, 602, 1024, 1026, 1028,
         1032, 2048)


def _align(t):
    a = t.data_ptr()
    return 16 if a % 16 == 0 else 8 if a % 8 == 0 else 4 if a % 4 == 0 else 2


def _shifted(t, k):
    """Same values, storage moved by k ELEMENTS (2 k bytes) off a 16-byte boundary (k = 0: as allocated)."""
    if k == 0:
        return t
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _rand(rows, N, seed, dt):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.rand((rows, N), device="cuda", generator=g) - 0.5).to(DT[dt])


def _run(_lib, csr, idx0, ci, D1, D2):
    """The C entry point on torch's current stream, out prefilled with NaN."""
    nnz, N, dt = ci.numel(), D1.shape[1], CODE[D1.dtype]
    assert D2.dtype == D1.dtype
    out = torch.full((nnz,), float("nan"), device="cuda")
    if csr:
        rc = _lib.lib.gespmm_sddmm_csr_x16(cptr(idx0), cptr(ci), cptr(D1), cptr(D2), cptr(out), dt, D1.shape[0], nnz, N, cur_stream())
    else:
        rc = _lib.lib.gespmm_sddmm_coo_x16(cptr(idx0), cptr(ci), cptr(D1), cptr(D2), cptr(out), dt, nnz, N, cur_stream())
    _lib.check(rc, "gespmm_sddmm_%s_x16" % ("csr" if csr else "coo"))
    return out


def _expect(_lib, csr, M, nnz, D1, D2, form, capturing=False, **want):
    """What the library says this call launches; it must be what the case was built to reach."""
    d = _lib.describe_sddmm(csr, M, nnz, D1.shape[1], _align(D1), _align(D2), capturing, x16=True)
    assert d["form"] == form, (d, form, want)
    for k, v in want.items():
        assert d[k] == v, (d, form, want)
    return d


def _sharp(oracle, out, ri, ci, D1, D2, V, W, edges=None, what=""):
    """Bit for bit against the lane-order oracle on the widened operands: all edges, or the edges listed."""
    if edges is None:
        ref = _lanes(oracle, V, W, ri.cpu().numpy(), ci.cpu().numpy(), D1.float().cpu().numpy(), D2.float().cpu().numpy())
        got = out.cpu().numpy()
    else:
        e = _dev(np.asarray(edges, dtype=np.int64))
        ru, rinv = torch.unique(ri[e], return_inverse=True)
        cu, cinv = torch.unique(ci[e], return_inverse=True)
        ref = _lanes(oracle, V, W, rinv.cpu().numpy(), cinv.cpu().numpy(), D1[ru.long()].float().cpu().numpy(),
                     D2[cu.long()].float().cpu().numpy())
        got = out[e].cpu().numpy()
    bad = np.flatnonzero(bits(got) != bits(ref))
    assert bad.size == 0, "%s V=%d W=%d N=%d %s: %d of %d edges differ from the lane oracle, first %d: %r vs %r" % (
        what, V, W, D1.shape[1], D1.dtype, bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]])


def _check_all(oracle, G, out, dev, D1, D2, V, W, rng, what):
    rp, ci, ri = dev
    _f64(out, ri, ci, D1, D2, what)
    _sharp(oracle, out, ri, ci, D1, D2, V, W, None if G["nnz"] <= 2000000 else _sample(G, rng), what)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 1. widths

@pytest.mark.parametrize("dt", (F16, BF16))
@pytest.mark.parametrize("which", ("edge", "random"))
def test_width_sweep_coo_and_csr(pkg, oracle, which, dt):
    """V = 1, 2, 4, 8, W from 4 to 64, and the three regimes of the edge loop for each V: one slice per row (N <= W V), slices
    in registers (N <= W V IT), the plain loop (513, 602, 1026, 1028, 1032, 2048). N = 0 writes zeros."""
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
    seen = set()
    for N in SWEEP:
        V, W = VW16[N]
        seen.add((V, W))
        D1, D2 = _rand(G["M"], N, 2 * N + 1, dt), _rand(G["K"], N, 2 * N + 2, dt)
        _expect(_lib, False, 0, G["nnz"], D1, D2, "coo-edge", V=V, W=W, epw=4 * 64 // W)
        _expect(_lib, True, G["M"], G["nnz"], D1, D2, "csr-edge", V=V, W=W, epw=max(16, 4 * 64 // W))
        o_coo = _run(_lib, False, ri, ci, D1, D2)
        o_csr = _run(_lib, True, rp, ci, D1, D2)
        assert _same(o_coo, o_csr), (which, N)
        _check_all(oracle, G, o_csr, dev, D1, D2, V, W, rng, "%s csr" % which)
        if N == 0:
            assert int((o_coo != 0).sum()) == 0
            assert int((sddmm.csr_sddmm(rp, ci, D1, D2) != 0).sum()) == 0 and int((sddmm.coo_sddmm(ri, ci, D1, D2) != 0).sum()) == 0
    assert {v for v, _ in seen} == {1, 2, 4, 8} and {w for _, w in seen} == {4, 8, 16, 32, 64}
    for V in (1, 2, 4, 8):  # every V in the plain loop, and below it
        assert (V, 64) in seen and any(v == V and w < 64 for v, w in seen)


# ------------------------------------------------------------------------------------------------------------- 2. alignment

@pytest.mark.parametrize("dt", (F16, BF16))
@pytest.mark.parametrize("N", (128, 1024))
def test_operand_alignment_picks_the_vector_width(pkg, oracle, N, dt):
    """N % 8 == 0 but D1, D2 or both start 1, 2 or 4 elements (or 3, 6) off a 16-byte boundary: V drops to 1, 2 or 4 and with it the
    order of the sum — the bits are the lane oracle's at THAT V: four results."""
    from gespmm_amd import _lib

    rng = np.random.RandomState(12)
    G = _pattern(rng.randint(0, 20, size=1500), 1200, rng)
    dev = _on_device(G)
    rp, ci, ri = dev
    A1, A2 = _rand(G["M"], N, 31, dt), _rand(G["K"], N, 32, dt)
    seen = set()
    for s1, s2 in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 2), (4, 0), (0, 4), (4, 4), (2, 4), (1, 4), (3, 2), (6, 4), (4, 7)):
        D1, D2 = _shifted(A1, s1), _shifted(A2, s2)
        amin = min(16 if s == 0 else 8 if s % 4 == 0 else 4 if s % 2 == 0 else 2 for s in (s1, s2))
        assert amin == min(_align(D1), _align(D2))
        V = amin // 2
        W = 64 if N == 1024 else (16 if V == 1 else 8)
        for csr in (False, True):
            _expect(_lib, csr, G["M"], G["nnz"], D1, D2, "csr-edge" if csr else "coo-edge", V=V, W=W)
            out = _run(_lib, csr, rp if csr else ri, ci, D1, D2)
            _check_all(oracle, G, out, dev, D1, D2, V, W, rng, "shift %d/%d %s" % (s1, s2, "csr" if csr else "coo"))
        seen.add((V, bits(out.cpu().numpy()).tobytes()))
    assert {v for v, _ in seen} == {1, 2, 4, 8} and len(seen) == 4, "one result per V, four different ones"


# ----------------------------------------------------------------------------------------------------------- 3. CSR windows

@pytest.mark.parametrize("target,lo,hi", ((50000, 0, 1 << 20), (1300000, 1 << 20, 1 << 22), (4500000, 1 << 22, 1 << 31)))
def test_csr_row_pointer_windows(pkg, oracle, target, lo, hi):
    """The CSR edge-parallel kernel's LDS window of row pointers at N = 16 (V = 8, W = 4: 64 edges per wavefront below 2^22 edges,
    256 from there), and below 2^20 edges also at N = 256 (W = 16: 16 edges per wavefront) and N = 72 (W = 8: 32): its search, the
    fallback for more than epw empty rows inside one wavefront's edges, the padding past rowptr[M]. CSR == COO == lane oracle."""
    from gespmm_amd import _lib

    for k, N in enumerate((16, 256, 72) if lo == 0 else (16,)):
        V, W = VW16[N]
        epw = 256 if lo >= (1 << 22) else 64 if lo >= (1 << 20) else max(16, 4 * 64 // W)
        start_run, tail_run = ((epw + 1, 1), (epw, 5000), (5000, epw - 1))[k]
        G = _window_pattern(target, epw, start_run, tail_run, seed=100 + k)
        assert lo <= G["nnz"] < hi, G["nnz"]
        e_lo = np.arange(0, G["nnz"], epw)
        r0 = np.searchsorted(G["rowptr"], e_lo, side="right") - 1
        r1 = np.searchsorted(G["rowptr"], np.minimum(e_lo + epw, G["nnz"]) - 1, side="right") - 1
        assert np.any(r1 - r0 >= epw + 1) and np.any(r1 == r0), "no wavefront spans an empty run / lies inside one row"
        if k == 0:
            assert np.any(r0 + epw + 1 > G["M"]), "no window reaches past rowptr[M]"
        rng = np.random.RandomState(200 + k)
        dev = _on_device(G)
        rp, ci, ri = dev
        D1, D2 = _rand(G["M"], N, 41 + k, BF16), _rand(G["K"], N, 51 + k, BF16)
        _expect(_lib, True, G["M"], G["nnz"], D1, D2, "csr-edge", V=V, W=W, epw=epw)
        _expect(_lib, False, 0, G["nnz"], D1, D2, "coo-edge", V=V, W=W, epw=4 * 64 // W)
        o_csr = _run(_lib, True, rp, ci, D1, D2)
        o_coo = _run(_lib, False, ri, ci, D1, D2)
        assert _same(o_csr, o_coo), (target, N)
        _check_all(oracle, G, o_csr, dev, D1, D2, V, W, rng, "windows %d" % target)
        del D1, D2, o_csr, o_coo


# -------------------------------------------------------------------------------------------------------------- 4. row walk

@pytest.mark.parametrize("N", (72, 128, 130, 513, 1032))
def test_row_walk(pkg, oracle, N):
    """Mean degree >= 64 and one slab: a row per wavefront. ~600 rows of degree ~70, rows of 0, 1, 63, 64, 65, 129 entries (the
    64-column staging step and its neighbours) and a 5000-entry hub; slices in registers (72, 128, 130) and the plain loop (513,
    1032); V = 8, 2 and 1; both dtypes."""
    from gespmm_amd import _lib

    rng = np.random.RandomState(13)
    degs = np.concatenate(([0, 1, 63, 64, 65, 129, 0, 0, 5000, 1], rng.randint(64, 77, size=600), [0, 129, 0]))
    G = _pattern(degs, 777, rng, mixed_order=True)
    dev = _on_device(G)
    rp, ci, ri = dev
    V, W = VW16[N]
    for dt in (F16, BF16):
        D1, D2 = _rand(G["M"], N, 61 + dt, dt), _rand(G["K"], N, 62 + dt, dt)
        _expect(_lib, True, G["M"], G["nnz"], D1, D2, "row-walk", V=V, W=W)
        out = _run(_lib, True, rp, ci, D1, D2)
        _check_all(oracle, G, out, dev, D1, D2, V, W, rng, "row-walk")
        assert _same(out, _run(_lib, False, ri, ci, D1, D2))


# --------------------------------------------------------------------------------------------------------------- 5. blocked

# N, M, mean degree, K / M, nslab, slab_rows = max(64, 6 MiB / 2N), dtype: V = 8 in the plain loop (1024) and in registers (256), V = 1
# (513); 4 slabs and 8; square, K = 3 M (columns past M: the clamped last slab) and K = M / 3 (the late slabs stay empty)
BLOCKED = ((1024, 9300, 70, 1, 4, 3072, BF16), (1024, 9300, 70, 3, 4, 3072, F16), (1024, 9300, 70, 1 / 3, 4, 3072, BF16),
           (1024, 22000, 70, 1, 8, 3072, F16), (513, 19000, 70, 1, 4, 6132, BF16), (513, 19000, 70, 3, 4, 6132, F16),
           (256, 37000, 70, 1, 4, 12288, F16))


@pytest.mark.parametrize("N,M,avg,kf,nslab,slab_rows,dt", BLOCKED)
def test_cache_blocked_form(pkg, oracle, N, M, avg, kf, nslab, slab_rows, dt):
    from gespmm_amd import _lib

    G = _dense_pattern(M, avg, int(M * kf), seed=N + M)
    if kf > 1:
        assert (G["colind"] >= M).mean() > 0.5
    rng = np.random.RandomState(14)
    dev = _on_device(G)
    rp, ci, ri = dev
    V, W = VW16[N]
    D1, D2 = _rand(G["M"], N, 71, dt), _rand(G["K"], N, 72, dt)
    _expect(_lib, True, M, G["nnz"], D1, D2, "blocked", V=V, W=W, nslab=nslab, slab_rows=slab_rows)
    out = _run(_lib, True, rp, ci, D1, D2)
    _check_all(oracle, G, out, dev, D1, D2, V, W, rng, "blocked nslab=%d K=%d" % (nslab, G["K"]))
    assert _same(out, _run(_lib, False, ri, ci, D1, D2))


# --------------------------------------------------------------------------------------------------------------- 6. capture

def test_captured_call_skips_the_blocked_form(pkg, oracle):
    """The blocked form allocates, so a capturing stream gets the row walk: same bits. Replays see new operand contents."""
    from gespmm_amd import _lib, sddmm

    N, M = 1024, 9300
    G = _dense_pattern(M, 70, M, seed=5)
    dev = _on_device(G)
    rp, ci, ri = dev
    D1, D2 = _rand(M, N, 81, BF16), _rand(M, N, 82, BF16)
    _expect(_lib, True, M, G["nnz"], D1, D2, "blocked", V=8, W=64, nslab=4)
    _expect(_lib, True, M, G["nnz"], D1, D2, "row-walk", capturing=True, V=8, W=64)
    graph, out = _capture(lambda: sddmm.csr_sddmm(rp, ci, D1, D2))
    assert out.dtype == torch.float32
    for seed in (83, 85):
        D1.copy_(_rand(M, N, seed, BF16))
        D2.copy_(_rand(M, N, seed + 1, BF16))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = _run(_lib, True, rp, ci, D1, D2)  # blocked
        assert _same(out, eager), seed
        _f64(out, ri, ci, D1, D2, "captured")
        _sharp(oracle, out, ri, ci, D1, D2, 8, 64, what="captured")


def test_captured_call_through_a_plan(pkg, oracle):
    """A plan on the clustered edge order (route 2) whose buffers the warm-up built: the capture holds two kernels."""
    from gespmm_amd import _lib, graphs, sddmm, spmm

    g = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda")
    rp, ci, M, K, N = g["rowptr"], g["colind"], g["M"], g["K"], 128
    ri = _dev(_rows_of(rp.cpu().numpy()))
    plan = spmm.SpmmPlan(rp, ci, K, N, reorder=True)
    assert _lib.lib.gespmm_plan_sddmm_route(plan._handle, N) == 2, plan.describe()
    D1, D2 = _rand(M, N, 91, F16), _rand(K, N, 92, F16)
    _expect(_lib, False, 0, g["nnz"], D1, D2, "coo-edge", V=8, W=8, epw=32)
    graph, out = _capture(lambda: sddmm.csr_sddmm(rp, ci, D1, D2, plan=plan))
    for seed in (93, 95):
        D1.copy_(_rand(M, N, seed, F16))
        D2.copy_(_rand(K, N, seed + 1, F16))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _f64(out, ri, ci, D1, D2, "captured plan")
        _sharp(oracle, out, ri, ci, D1, D2, 8, 8, what="captured plan")


# ----------------------------------------------------------------------------------------------------------- 7. plan routes

def test_plan_routes(pkg, oracle, bundled):
    """gespmm_plan_sddmm_x16 on its three routes — 0 the CSR call, 1 COO on row ids expanded once, 2 the clustered edge order and
    a scatter — each asserted through gespmm_plan_sddmm_route (the rule is the fp32 call's: tests/test_gpu_sddmm_forms.py), each
    called twice with different operands, bit-equal to the stateless 16-bit call and to the lane oracle."""
    from gespmm_amd import _lib, graphs, spmm

    rng = np.random.RandomState(15)
    sbm = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda")
    dense = _pattern(rng.randint(28, 50, size=4000), 4000, rng)
    pub = bundled["pubmed"]
    cases = (("pubmed", _dev(pub["rowptr"]), _dev(pub["colind"]), pub["M"], pub["K"], True),
             ("com-amazon-sbm", sbm["rowptr"], sbm["colind"], sbm["M"], sbm["K"], True),
             ("dense", _dev(dense["rowptr"]), _dev(dense["colind"]), dense["M"], dense["K"], False))
    routes = set()
    f = _lib.lib.gespmm_plan_sddmm_x16
    for name, rp, ci, M, K, reorder in cases:
        rph = rp.cpu().numpy()
        nnz = int(rph[-1])
        ri = _dev(_rows_of(rph))
        for N in (3, 64, 128):
            dt = BF16 if N != 64 else F16
            plan = spmm.SpmmPlan(rp, ci, K, N, reorder=reorder)
            route = _lib.lib.gespmm_plan_sddmm_route(plan._handle, N)
            assert route == {"dense": 0, "com-amazon-sbm": 1 if N < 64 else route, "pubmed": 1 if N < 64 else route}[name], (name, N, route)
            if name == "com-amazon-sbm" and N == 128:
                assert route == 2, plan.describe()
            routes.add(route)
            V, W = VW16[N]
            for call in range(2):
                D1, D2 = _rand(M, N, 7 * N + call, dt), _rand(K, N, 7 * N + 3 + call, dt)
                if route == 0:
                    _expect(_lib, True, M, nnz, D1, D2, "csr-edge", V=V, W=W)
                else:
                    _expect(_lib, False, 0, nnz, D1, D2, "coo-edge", V=V, W=W)
                out = torch.full((nnz,), float("nan"), device="cuda")
                _lib.check(f(plan._handle, cptr(D1), cptr(D2), cptr(out), dt, N, cur_stream()), "gespmm_plan_sddmm_x16")
                assert _same(out, _run(_lib, True, rp, ci, D1, D2)), (name, N, route, call)
                _f64(out, ri, ci, D1, D2, "%s route %d call %d" % (name, route, call))
                _sharp(oracle, out, ri, ci, D1, D2, V, W, what="%s route %d call %d" % (name, route, call))
            # the checks of the stateless entry points, on every route
            odd = ctypes.c_void_p(D1.data_ptr() + 1)
            assert f(plan._handle, odd, cptr(D2), cptr(out), dt, N, cur_stream()) == -2
            assert f(plan._handle, cptr(D1), odd, cptr(out), dt, N, cur_stream()) == -2
            assert f(plan._handle, cptr(D1), cptr(D2), ctypes.c_void_p(out.data_ptr() + 2), dt, N, cur_stream()) == -2
            assert f(plan._handle, cptr(D1), cptr(D2), None, dt, N, cur_stream()) == -1
            assert f(plan._handle, cptr(D1), cptr(D2), cptr(out), 0, N, cur_stream()) == -1
            assert f(plan._handle, cptr(D1), cptr(D2), cptr(out), 3, N, cur_stream()) == -1
            assert f(plan._handle, cptr(D1), cptr(D2), cptr(out), dt, 1 << 30, cur_stream()) == -3
            del plan
    assert routes == {0, 1, 2}


# -------------------------------------------------------------------------------------------------------- 8. special values

def _special_operands(G, N, dt):
    """Host tensors of the 16-bit type. A third of all elements are specials: subnormals of both signs, +-0, the largest finite
    number, the smallest normal one. Three rows with edges are set apart: row A holds one +inf (against a column of ones: its edges
    are +inf), row B +inf and -inf (NaN), row S nothing but the smallest subnormal (times finite numbers: flushed, its sums would be 0)."""
    tdt = DT[dt]
    fi = torch.finfo(tdt)
    sub = [1, 2, 3, 0x3FF if dt == F16 else 0x7F, 0x8001, 0x8000 | (0x200 if dt == F16 else 0x40)]  # bit patterns
    specials = torch.cat((torch.tensor(sub, dtype=torch.int32).to(torch.int16).view(tdt),
                          torch.tensor([0.0, -0.0, fi.max, -fi.max, fi.tiny, -fi.tiny, 1.0], dtype=torch.float32).to(tdt)))
    r = np.random.RandomState(1600 + N + dt)
    out = []
    for rows in (G["M"], G["K"]):
        D = torch.from_numpy(r.rand(rows, N).astype(np.float32) - np.float32(0.5)).to(tdt)
        pick = torch.from_numpy(r.randint(0, specials.numel(), size=(rows, N)))
        mask = torch.from_numpy(r.rand(rows, N) < 0.33)
        out.append(torch.where(mask, specials[pick], D))
    D1, D2 = out
    rowA, rowB, rowS = np.flatnonzero(np.diff(G["rowptr"]) > 0)[[0, 3, 6]]
    D2[:, 0] = 1.0
    D2[:, 1] = 1.0
    for row in (rowA, rowB):
        # small ordinary numbers but for the inf (small: against the largest bf16 number their products must stay finite)
        D1[row] = torch.from_numpy((r.rand(N).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -20)).to(tdt)
        D1[row, 0] = float("inf")
    D1[rowB, 1] = float("-inf")
    D1[rowS] = specials[0]
    return D1, D2, (int(rowA), int(rowB), int(rowS))


@pytest.mark.parametrize("dt", (F16, BF16))
def test_special_values(pkg, oracle, dt):
    """Subnormals of the 16-bit type, +-0, its largest finite number, infs: widening is exact, so every edge has the lane oracle's
    bits — +-inf and sums that are subnormal in fp32 included. Where the oracle's sum is a NaN (inf - inf,
    inf * 0) the kernel's must be a NaN; which NaN is not compared: the host's default NaN has the sign bit set, the GPU's has not,
    and include/gespmm.h pins no payload."""
    from gespmm_amd import _lib

    rng = np.random.RandomState(16)
    G = _pattern(rng.randint(0, 12, size=400), 300, rng)
    dev = _on_device(G)
    rp, ci, ri = dev
    rih = G["rows"]
    for N in (8, 33, 130, 1032):  # V = 8 one slice, V = 1 in registers, V = 2, V = 8 in the plain loop
        V, W = VW16[N]
        H1, H2, (rowA, rowB, rowS) = _special_operands(G, N, dt)
        D1, D2 = H1.cuda(), H2.cuda()
        _expect(_lib, True, G["M"], G["nnz"], D1, D2, "csr-edge", V=V, W=W)
        out = _run(_lib, True, rp, ci, D1, D2)
        assert _same(out, _run(_lib, False, ri, ci, D1, D2))
        ref = _lanes(oracle, V, W, rih, G["colind"], H1.float().numpy(), H2.float().numpy())
        got = out.cpu().numpy()
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), (N, int(np.isnan(got).sum()), int(nan.sum()))
        bad = np.flatnonzero((bits(got) != bits(ref)) & ~nan)
        assert bad.size == 0, "N=%d: %d edges differ from the lane oracle, first %d: %r vs %r" % (N, bad.size, bad[0], got[bad[0]], ref[bad[0]])
        fin = torch.from_numpy(np.isfinite(ref)).cuda()
        _f64(out[fin], ri[fin], ci[fin], D1, D2, "special values")
        # the cases are there: row A's edges are +inf, row B's NaN, row S's sums come from subnormal elements alone
        assert np.all(np.isposinf(ref[rih == rowA])) and np.all(nan[rih == rowB]) and (rih == rowA).any() and (rih == rowB).any()
        s = ref[rih == rowS]
        assert s.size > 0 and np.all(np.isfinite(s)) and np.any(s != 0), (N, s)  # (sums of subnormal * finite: nothing was flushed)


# ------------------------------------------------------------------------------------------------------------------ 9. fuzz

def _empty_runs(rng):
    M = int(rng.choice([1, 70, 150, 300]))
    degs = np.zeros(M, dtype=np.int64)
    k = int(rng.randint(1, 12))
    at = rng.randint(0, M, size=k)
    degs[at] = rng.choice([1, 1, 2, 5, 17, 64, 300], size=k)
    return _pattern(degs, int(rng.choice([1, 64, 300])), rng)


def test_seeded_fuzz(pkg, oracle):
    """~100 seeded cases: M, K <= 300, N <= 300, random empty runs, random dtype, random operand shifts (in elements)."""
    from gespmm_amd import _lib

    rng = np.random.RandomState(20261018)
    forms = set()
    launched = 0
    for case in range(110):
        if rng.rand() < 0.5:
            G, law = _empty_runs(rng), "empty-runs"
        else:
            M, K = int(rng.randint(1, 301)), int(rng.randint(1, 301))
            G, law = _pattern(rng.randint(0, int(rng.choice([3, 20, 140, 260])), size=M) * (rng.rand(M) < 0.7), K, rng, mixed_order=True), "random"
        N = int(rng.choice([int(rng.randint(0, 301)), int(rng.choice([8, 16, 24, 64, 72, 128, 136, 256, 264, 296]))]))
        dt = int(rng.choice([F16, BF16]))
        csr = bool(rng.rand() < 0.5)
        s1, s2 = (int(x) for x in rng.choice([0, 0, 0, 1, 2, 3, 4, 6], size=2))
        D1 = _shifted(_rand(G["M"], N, 1000 + case, dt) * 3, s1 if N else 0)
        D2 = _shifted(_rand(G["K"], N, 2000 + case, dt) * 2, s2 if N else 0)
        rp, ci, ri = _on_device(G)
        d = _lib.describe_sddmm(csr, G["M"], G["nnz"], N, _align(D1), _align(D2), x16=True)
        if G["nnz"] == 0:
            assert d["form"] == "none"
            assert _run(_lib, csr, rp if csr else ri, ci, D1, D2).numel() == 0
            continue
        assert d["form"] in (("csr-edge", "row-walk") if csr else ("coo-edge",)), (case, law, d)
        amin = min(_align(D1), _align(D2)) if N else 16
        V = max(v for v in (1, 2, 4, 8) if N % v == 0 and amin % (2 * v) == 0)
        per_lane = V * {8: 2, 4: 4, 2: 8, 1: 8}[V]
        W = min([w for w in (4, 8, 16, 32, 64) if w * per_lane >= N] or [64])
        assert (d["V"], d["W"]) == (V, W), (case, N, amin, d)
        forms.add((d["form"], d["V"], d["W"]))
        out = _run(_lib, csr, rp if csr else ri, ci, D1, D2)
        launched += 1
        _f64(out, ri, ci, D1, D2, "fuzz %d %s" % (case, law))
        _sharp(oracle, out, ri, ci, D1, D2, V, W, what="fuzz %d %s %s" % (case, law, d))
    assert launched >= 80, launched
    assert {f for f, _, _ in forms} == {"coo-edge", "csr-edge", "row-walk"} and {v for _, v, _ in forms} == {1, 2, 4, 8}, sorted(forms)


# -------------------------------------------------------------------------------------------------------- 10. Python surface

@pytest.mark.parametrize("path", ("pybind", "ctypes"))
def test_python_surface(pkg, oracle, bundled, monkeypatch, path):
    """sddmm.coo_sddmm / csr_sddmm (with and without plan=) on bf16 and fp16: fp32 out with the oracle's bits; the edge-weight
    gradient of a bf16 model on pubmed at N = 16 against float64; mixed dtypes and fp64 raise TypeError; SPMMFunction(..., True)
    on bf16 still raises TypeError."""
    import gespmm_amd
    from gespmm_amd import graphs, sddmm, spmm

    if path == "ctypes":
        monkeypatch.setattr(sddmm, "_ext", None)
    else:
        assert sddmm._ext is not None
    G = bundled["pubmed"]
    rp, ci = _dev(G["rowptr"]), _dev(G["colind"])
    ri = _dev(_rows_of(G["rowptr"]))
    N = 16
    V, W = VW16[N]
    plan = spmm.SpmmPlan(rp, ci, G["K"], N, reorder=True)
    for dt in (BF16, F16):
        go, feat = _rand(G["M"], N, 103 + dt, dt), _rand(G["K"], N, 102 + dt, dt)  # grad_out, features: grad_w[e] = <go[row e], feat[col e]>
        for name, gw in (("csr", sddmm.csr_sddmm(rp, ci, go, feat)), ("coo", sddmm.coo_sddmm(ri, ci, go, feat)),
                         ("plan", sddmm.csr_sddmm(rp, ci, go, feat, plan=plan))):
            assert gw.dtype == torch.float32 and gw.shape == (G["nnz"],), name
            _f64(gw, ri, ci, go, feat, "python %s" % name)
            _sharp(oracle, gw, ri, ci, go, feat, V, W, what="python %s %s" % (path, name))
        # feeds the product's values as it is
        y = spmm.csr_spmm(rp, ci, gw, feat)
        assert y.dtype == feat.dtype and y.shape == (G["M"], N)
    bf, hf = _rand(G["M"], N, 1, BF16), _rand(G["K"], N, 2, F16)
    for D1, D2 in ((bf, hf), (bf, hf.float()), (bf.float(), hf), (bf.double(), hf.double()), (bf, hf.to(torch.bfloat16).double())):
        for call in (lambda: sddmm.csr_sddmm(rp, ci, D1, D2), lambda: sddmm.coo_sddmm(ri, ci, D1, D2),
                     lambda: sddmm.csr_sddmm(rp, ci, D1, D2, plan=plan)):
            with pytest.raises(TypeError):
                call()
    colptr, rowind = graphs.transpose_csr(rp, ci)
    w = torch.rand(G["nnz"], device="cuda")
    _, _, w_csc = graphs.transpose_csr(rp, ci, val=w)
    with pytest.raises(TypeError, match="csr_sddmm"):
        gespmm_amd.SPMMFunction.apply(rp, ci, colptr, rowind, feat.to(torch.bfloat16).requires_grad_(True), w.requires_grad_(True), w_csc, True)
