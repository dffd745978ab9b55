"""Multi-head SDDMM on the GPU: out[e, h] = <D1[row(e), h, :], D2[col(e), h, :]> (sddmm.csr_sddmm_heads / coo_sddmm_heads).

Every result is written into a NaN-prefilled tensor carved out of a buffer with 64 guard words after it (they must still be NaN
afterwards), every route and launch shape is ASSERTED through gespmm_describe_sddmm_heads, and comparisons are on bit patterns: head h
against the lane-order oracle (oracle.sddmm_lanes) at the described (V, W) on the head's slices."""
import numpy as np
import pytest
import torch

from helpers import bits, edge_case_csr
from test_gpu_sddmm_forms import _capture, _pattern, _rows_of

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
GRID = ((2, 1), (3, 1), (8, 1), (2, 2), (2, 3), (3, 5), (4, 4), (8, 8), (5, 13), (3, 20), (7, 6), (8, 16), (4, 32), (7, 27), (2, 64),
        (6, 100), (4, 160), (2, 600), (2, 513), (9, 4), (16, 8), (1, 128))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _align(t):
    a = t.data_ptr()
    return 16 if a % 16 == 0 else (8 if a % 8 == 0 else 4)


def _vw(F, align=16):
    """(V, W) by hand: V the widest of 4, 2, 1 that divides F and whose 4 V bytes divide the addresses; a lane covers 8 floats (2
    dwordx4, 4 dwordx2, 8 dwords), W the smallest power of two in 4 .. 64 with 8 W >= F."""
    V = max(v for v in (1, 2, 4) if F % v == 0 and align % (4 * v) == 0)
    W = 4
    while W < 64 and 8 * W < F:
        W *= 2
    return V, W


def _rand(rows, H, F, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.rand((rows, H, F), device="cuda", generator=g) - 0.5


def _carve(t, off):
    """Same values, storage `off` bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0 and off % 4 == 0
    v = buf[off // 4:off // 4 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _out(nnz, H):
    buf = torch.full((nnz * H + GUARD,), NAN, device="cuda")
    return buf, buf[:nnz * H].view(nnz, H)


def _guard_ok(buf, what=""):
    assert bool(torch.isnan(buf[-GUARD:]).all()), "guard words after out were written: %s" % (what,)


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    assert bad == 0, "%s: %d of %d words differ" % (what, bad, got.numel())


def _csr(sddmm, G, D1, D2, plan=None):
    buf, out = _out(G["nnz"], D1.shape[1])
    r = sddmm.csr_sddmm_heads(G["rp"], G["ci"], D1, D2, out=out, plan=plan)
    assert r is out
    _guard_ok(buf, "csr")
    return out


def _coo(sddmm, G, D1, D2):
    buf, out = _out(G["nnz"], D1.shape[1])
    sddmm.coo_sddmm_heads(G["ri"], G["ci"], D1, D2, out=out)
    _guard_ok(buf, "coo")
    return out


def _up(G):
    G = dict(G)
    if "rows" not in G:
        G["rows"] = _rows_of(G["rowptr"])
    G["rp"], G["ci"], G["ri"] = _dev(G["rowptr"]), _dev(G["colind"]), _dev(G["rows"])
    return G


def _oracle_heads(oracle, V, W, rows, cols, D1, D2):
    """[len(rows), H]: the lane oracle on every head's slices (host arrays)."""
    return np.stack([oracle.sddmm_lanes(V, W, rows, cols, D1[:, h, :], D2[:, h, :]) for h in range(D1.shape[1])], axis=1)


def _sharp(oracle, out, G, D1, D2, V, W, edges=None, what=""):
    if edges is None:
        ref = _oracle_heads(oracle, V, W, G["rows"], G["colind"], D1.cpu().numpy(), D2.cpu().numpy())
        got = out.cpu().numpy()
    else:
        e = np.asarray(edges, dtype=np.int64)
        ru, rinv = np.unique(G["rows"][e], return_inverse=True)
        cu, cinv = np.unique(G["colind"][e], return_inverse=True)
        ref = _oracle_heads(oracle, V, W, rinv.astype(np.int32), cinv.astype(np.int32), D1[_dev(ru.astype(np.int64))].cpu().numpy(),
                            D2[_dev(cu.astype(np.int64))].cpu().numpy())
        got = out[_dev(e)].cpu().numpy()
    bad = np.argwhere(bits(got) != bits(ref))
    assert bad.shape[0] == 0, "%s V=%d W=%d: %d of %d words differ from the lane oracle, first (edge, head) %r: %r vs %r" % (
        what, V, W, bad.shape[0], got.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


def _f64(out, G, D1, D2, what=""):
    """Every (edge, head) against float64 accumulation on the device: |out - ref| <= 1e-4 * max(|ref|, sum |d1 d2|)."""
    nnz, (H, F) = out.shape[0], D1.shape[1:]
    step = max(1, (1 << 23) // (H * F))
    nbad = torch.zeros((), dtype=torch.int64, device="cuda")
    for s in range(0, nnz, step):
        p = D1[G["ri"][s:s + step].long()].double() * D2[G["ci"][s:s + step].long()].double()
        ref, scale = p.sum(-1), p.abs().sum(-1)
        ok = (out[s:s + step].double() - ref).abs() <= 1e-4 * torch.maximum(ref.abs(), scale)  # (NaN compares false)
        nbad += (~ok).sum()
    assert int(nbad) == 0, "%s: %d of %d results outside the float64 tolerance" % (what, int(nbad), nnz * H)


def _want_epw(csr, nnz, H, W):
    G, pairs = 64 // W, nnz * H
    per_wave = G * 4 if not csr else 256 if pairs >= 256 * 16384 else 64 if pairs >= 64 * 16384 else max(G * 4, 16)
    return min(256, max(1, per_wave // H))


def _expect_kernel(_lib, G, csr, D1, D2, V, W, capturing=False):
    H, F = D1.shape[1:]
    d = _lib.describe_sddmm_heads(csr, G["M"], G["nnz"], H, F, _align(D1), _align(D2), capturing)
    want = {"route": "kernel", "form": "csr-edge" if csr else "coo-edge", "V": V, "W": W, "epw": _want_epw(csr, G["nnz"], H, W)}
    assert d == want, (d, want)
    return d


@pytest.fixture(autouse=True)
def _no_pin(monkeypatch):
    monkeypatch.delenv("GESPMM_SDDMM_HEADS_ROUTE", raising=False)


@pytest.fixture(scope="module")
def edge():
    return _up(edge_case_csr())


# ------------------------------------------------------------------------------------------------------------------- 1. grid

@pytest.mark.parametrize("H,F", GRID)
def test_grid_equals_oracle(pkg, oracle, edge, H, F):
    """All three width branches at V = 4 and V = 1 (and V = 2), H that divides nothing, H above 8; H = 1 is the single-head call."""
    from gespmm_amd import _lib, sddmm

    G = edge
    assert G["M"] == 21 and G["K"] == 301 and G["nnz"] // G["M"] < 64
    V, W = _vw(F)
    D1, D2 = _rand(G["M"], H, F, 10 * H + F), _rand(G["K"], H, F, 10 * H + F + 1)
    assert _align(D1) == 16 and _align(D2) == 16
    if H == 1:
        assert _lib.describe_sddmm_heads(True, G["M"], G["nnz"], H, F) == dict(_lib.describe_sddmm(True, G["M"], G["nnz"], F), route="plain")
        assert _lib.describe_sddmm_heads(False, 0, G["nnz"], H, F)["route"] == "plain"
    else:
        _expect_kernel(_lib, G, True, D1, D2, V, W)
        _expect_kernel(_lib, G, False, D1, D2, V, W)
    o_csr = _csr(sddmm, G, D1, D2)
    o_coo = _coo(sddmm, G, D1, D2)
    _same(o_csr, o_coo, ("csr vs coo", H, F))
    _sharp(oracle, o_csr, G, D1, D2, V, W, what="grid H=%d F=%d" % (H, F))
    _f64(o_csr, G, D1, D2, "grid H=%d F=%d" % (H, F))


@pytest.mark.parametrize("H,F", ((3, 5), (8, 8), (4, 32), (2, 600)))
def test_equals_per_head_calls(pkg, edge, H, F):
    """On torch-allocated (16-byte aligned) operands: the bits of sddmm.csr_sddmm on the contiguous per-head copies."""
    from gespmm_amd import sddmm

    G = edge
    D1, D2 = _rand(G["M"], H, F, 71 + H), _rand(G["K"], H, F, 72 + F)
    want = torch.stack([sddmm.csr_sddmm(G["rp"], G["ci"], D1[:, h, :].contiguous(), D2[:, h, :].contiguous()) for h in range(H)], dim=1)
    _same(_csr(sddmm, G, D1, D2), want, (H, F))
    _same(_coo(sddmm, G, D1, D2), want, (H, F))


def test_zero_width_and_no_edges(pkg, edge):
    from gespmm_amd import sddmm

    G = edge
    out = _csr(sddmm, G, torch.empty(G["M"], 3, 0, device="cuda"), torch.empty(G["K"], 3, 0, device="cuda"))
    assert out.shape == (G["nnz"], 3) and int((out.view(torch.int32) != 0).sum()) == 0
    rp0 = torch.zeros(8, dtype=torch.int32, device="cuda")
    ci0 = torch.empty(0, dtype=torch.int32, device="cuda")
    assert sddmm.csr_sddmm_heads(rp0, ci0, _rand(7, 3, 5, 1), _rand(4, 3, 5, 2)).shape == (0, 3)
    assert sddmm.coo_sddmm_heads(ci0, ci0, _rand(7, 3, 5, 1), _rand(4, 3, 5, 2)).shape == (0, 3)


# -------------------------------------------------------------------------------------------------------------- 2. alignment

@pytest.mark.parametrize("route", ("kernel", "composition"))
@pytest.mark.parametrize("H,F", ((4, 8), (3, 20), (2, 64)))
def test_alignment(pkg, oracle, edge, monkeypatch, route, H, F):
    """D1 and D2 start 8 or 4 bytes past a 16-byte boundary, independently: V drops as described and the bits are the oracle's at the
    described (V, W) — on the kernel and on the forced composition, whose temporaries take the caller's alignment class."""
    from gespmm_amd import _lib, sddmm

    G = edge
    if route == "composition":
        monkeypatch.setenv("GESPMM_SDDMM_HEADS_ROUTE", "composition")
    A1, A2 = _rand(G["M"], H, F, 31), _rand(G["K"], H, F, 32)
    seen = set()
    for o1, o2 in ((0, 0), (8, 0), (0, 8), (8, 8), (4, 0), (0, 4), (4, 8), (8, 4), (4, 4), (12, 8)):
        D1, D2 = (_carve(A1, o1) if o1 else A1), (_carve(A2, o2) if o2 else A2)
        a = min(_align(D1), _align(D2))
        assert (_align(D1), _align(D2)) == tuple(16 if o == 0 else 8 if o == 8 else 4 for o in (o1, o2))
        V, W = _vw(F, a)
        assert V == {16: 4, 8: 2, 4: 1}[a]
        d = _lib.describe_sddmm_heads(True, G["M"], G["nnz"], H, F, _align(D1), _align(D2))
        if route == "kernel":
            assert d == {"route": "kernel", "form": "csr-edge", "V": V, "W": W, "epw": _want_epw(True, G["nnz"], H, W)}, d
        else:
            assert d == {"route": "composition", "V": V, "W": W}, d
        out = _csr(sddmm, G, D1, D2)
        _sharp(oracle, out, G, D1, D2, V, W, what="%s offsets %d/%d" % (route, o1, o2))
        if route == "kernel":
            _same(_coo(sddmm, G, D1, D2), out, ("coo", o1, o2))
        seen.add((V, bits(out.cpu().numpy()).tobytes()))
    assert len({v for v, _ in seen}) == 3 and len(seen) == 3, "one result per V, three different ones"


# -------------------------------------------------------------------------------------------------------- 3. rows and tails

def test_row_window_overflow(pkg, oracle):
    """Two runs of 300 empty rows between short rows — more than epw + 1 row pointers inside one wavefront's edges, so the LDS window
    overflows into the whole-array search — and a tail of empty rows."""
    from gespmm_amd import _lib, sddmm

    H, F = 3, 5
    rng = np.random.RandomState(5)
    degs = np.concatenate(([2, 1, 3], np.zeros(300), [1, 2, 1, 4], np.zeros(300), [3, 1, 1, 2, 5], rng.randint(0, 4, size=40), np.zeros(10)))
    G = _up(_pattern(degs, 97, rng))
    V, W = _vw(F)
    D1, D2 = _rand(G["M"], H, F, 41), _rand(G["K"], H, F, 42)
    epw = _expect_kernel(_lib, G, True, D1, D2, V, W)["epw"]
    e_lo = np.arange(0, G["nnz"], epw)
    r0 = np.searchsorted(G["rowptr"], e_lo, side="right") - 1
    r1 = np.searchsorted(G["rowptr"], np.minimum(e_lo + epw, G["nnz"]) - 1, side="right") - 1
    assert np.any(r1 - r0 >= epw + 1), "no wavefront spans more than epw + 1 row pointers"
    assert np.any(r0 + epw + 1 > G["M"]), "no window reaches past rowptr[M]"
    out = _csr(sddmm, G, D1, D2)
    _sharp(oracle, out, G, D1, D2, V, W, what="row window")
    _same(_coo(sddmm, G, D1, D2), out, "coo")


@pytest.mark.parametrize("H,F", ((3, 5), (7, 6)))
def test_short_rows_and_pair_tails(pkg, oracle, H, F):
    """M = 5000, degrees 0 .. 3: many rows per wavefront; nnz H is no multiple of 4, hence of no G * UE — the last step of the last
    wavefront holds pairs past the end."""
    from gespmm_amd import _lib, sddmm

    rng = np.random.RandomState(6)
    degs = rng.randint(0, 4, size=5000)
    degs[-1] += (1 - int(degs.sum())) % 4  # nnz = 1 mod 4, H odd
    G = _up(_pattern(degs, 3000, rng))
    assert (G["nnz"] * H) % 4 != 0 and G["M"] == 5000 and degs.max() <= 6
    V, W = _vw(F)
    D1, D2 = _rand(G["M"], H, F, 51), _rand(G["K"], H, F, 52)
    _expect_kernel(_lib, G, True, D1, D2, V, W)
    _expect_kernel(_lib, G, False, D1, D2, V, W)
    out = _csr(sddmm, G, D1, D2)
    _sharp(oracle, out, G, D1, D2, V, W, what="short rows")
    _same(_coo(sddmm, G, D1, D2), out, "coo")


# pair-count tiers of the carried-over thresholds (pairs per wavefront 256 from 2^22 pairs, 64 from 2^20, else max(4 * 64 / W, 16)), at
# the smallest edge counts that reach them, and both ends of the range: epw = 1 (H >= pairs per wavefront) and 128 (H = 2)
# (F = 40: 8 lanes per pair, so the tier below 2^20 pairs has 32 pairs per wavefront and differs from the 64 above it)
EPW = ((890, 16, 160, 1), (1000, 8, 64, 4), (1000, 3, 5, 21), (131072, 8, 40, 8), (524288, 8, 4, 32), (2097152, 2, 4, 128))


@pytest.mark.parametrize("nnz,H,F,epw", EPW)
def test_every_window_size(pkg, oracle, nnz, H, F, epw):
    from gespmm_amd import _lib, sddmm

    rng = np.random.RandomState(nnz % 1000 + H)
    degs = rng.randint(0, 33, size=nnz // 8 + 8)  # mean degree 16
    cut = int(np.searchsorted(np.cumsum(degs), nnz))
    degs = degs[:cut + 1]
    degs[-1] -= int(degs.sum()) - nnz
    G = _up(_pattern(degs, max(500, min(20000, 2000000 // (H * F))), rng))
    assert G["nnz"] == nnz and nnz // G["M"] < 64
    V, W = _vw(F)
    D1, D2 = _rand(G["M"], H, F, 61), _rand(G["K"], H, F, 62)
    assert _expect_kernel(_lib, G, True, D1, D2, V, W)["epw"] == epw
    if nnz >= 131072:  # the threshold itself: one edge less is the tier below
        below = _lib.describe_sddmm_heads(True, G["M"], nnz - 1, H, F)["epw"]
        assert below == _want_epw(True, nnz - 1, H, W) and below < epw
    out = _csr(sddmm, G, D1, D2)
    _f64(out, G, D1, D2, "epw=%d" % epw)
    edges = np.unique(np.concatenate((rng.randint(0, nnz, size=500), np.arange(6), np.arange(nnz - 6, nnz))))
    assert edges.size <= 512
    _sharp(oracle, out, G, D1, D2, V, W, edges=edges, what="epw=%d" % epw)
    _same(_coo(sddmm, G, D1, D2), out, "coo")


# ------------------------------------------------------------------------------------------------------------ 4. composition

@pytest.fixture(scope="module")
def dense():
    rng = np.random.RandomState(7)
    return _up(_pattern(np.full(48, 80), 301, rng))


@pytest.mark.parametrize("H,F", ((3, 5), (4, 8), (9, 4)))
def test_composition(pkg, oracle, dense, monkeypatch, H, F):
    """Mean degree 80, where gespmm_sddmm_csr_f32 walks rows. The rule takes the heads kernel there as well (measured faster: DESIGN
    3.14), so the per-head composition — what a CSR call past the pair limit runs — is reached through the pin: same bits either way."""
    from gespmm_amd import _lib, sddmm

    G = dense
    V, W = _vw(F)
    D1, D2 = _rand(G["M"], H, F, 81), _rand(G["K"], H, F, 82)
    assert _lib.describe_sddmm(True, G["M"], G["nnz"], F)["form"] == "row-walk"
    _expect_kernel(_lib, G, True, D1, D2, V, W)
    by_kernel = _csr(sddmm, G, D1, D2)
    monkeypatch.setenv("GESPMM_SDDMM_HEADS_ROUTE", "composition")
    assert _lib.describe_sddmm_heads(True, G["M"], G["nnz"], H, F) == {"route": "composition", "V": V, "W": W}
    out = _csr(sddmm, G, D1, D2)
    _sharp(oracle, out, G, D1, D2, V, W, what="composition")
    _same(by_kernel, out, "kernel on the dense pattern")
    _same(_coo(sddmm, G, D1, D2), out, "coo kernel")


def test_capture_takes_the_kernel(pkg, oracle, dense, monkeypatch):
    """The composition allocates, so a capturing stream gets the kernel even where the composition is pinned: same bits. Replays see new
    operand contents."""
    from gespmm_amd import _lib, sddmm

    G, H, F = dense, 4, 8
    V, W = _vw(F)
    D1, D2 = _rand(G["M"], H, F, 85), _rand(G["K"], H, F, 86)
    monkeypatch.setenv("GESPMM_SDDMM_HEADS_ROUTE", "composition")
    assert _lib.describe_sddmm_heads(True, G["M"], G["nnz"], H, F)["route"] == "composition"
    _expect_kernel(_lib, G, True, D1, D2, V, W, capturing=True)
    buf, out = _out(G["nnz"], H)
    graph, _ = _capture(lambda: sddmm.csr_sddmm_heads(G["rp"], G["ci"], D1, D2, out=out))
    for seed in (87, 89):
        D1.copy_(_rand(G["M"], H, F, seed))
        D2.copy_(_rand(G["K"], H, F, seed + 1))
        buf.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        _guard_ok(buf, "replay")
        _same(out, _csr(sddmm, G, D1, D2), "replay vs eager composition")
        _sharp(oracle, out, G, D1, D2, V, W, what="captured")


def test_one_head_is_the_single_head_call(pkg, dense, edge):
    from gespmm_amd import sddmm

    for G in (dense, edge):
        D1, D2 = _rand(G["M"], 1, 24, 91), _rand(G["K"], 1, 24, 92)
        want = sddmm.csr_sddmm(G["rp"], G["ci"], D1[:, 0, :], D2[:, 0, :]).view(-1, 1)
        _same(_csr(sddmm, G, D1, D2), want, "csr H=1")
        _same(_coo(sddmm, G, D1, D2), want, "coo H=1")


# ------------------------------------------------------------------------------------------------------------------ 5. plans

def test_plan_routes(pkg, oracle, dense, bundled):
    """gespmm_plan_sddmm_heads_f32 on its three routes, each ASSERTED (a route nobody reaches fails the test), each with the bits of the
    stateless call; the route-2 temporary grows with H; a plan of another pattern raises."""
    from gespmm_amd import graphs, sddmm, spmm

    pub = _up(bundled["pubmed"])
    cases = [("dense", dense, False, 4, 8), ("pubmed", pub, False, 4, 16), ("pubmed", pub, True, 4, 16)]
    reached = {}
    for name, G, reorder, H, F in cases:
        plan = spmm.SpmmPlan(G["rp"], G["ci"], G["K"], H * F, reorder=reorder)
        reached[(name, reorder)] = (plan.sddmm_heads_route(H, F), plan, G)
    if reached[("pubmed", True)][0] != 2:  # a graph whose clustered order is modelled to hit L2 (tests/test_gpu_sddmm_forms.py: route 2 at 128)
        sbm = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda")
        G = {"M": sbm["M"], "K": sbm["K"], "nnz": sbm["nnz"], "rp": sbm["rowptr"], "ci": sbm["colind"]}
        plan = spmm.SpmmPlan(G["rp"], G["ci"], G["K"], 128, reorder=True)
        reached[("com-amazon-sbm", True)] = (plan.sddmm_heads_route(8, 16), plan, G)
    print("plan routes:", {k: v[0] for k, v in reached.items()})
    assert reached[("dense", False)][0] == 0 and reached[("pubmed", False)][0] == 1, {k: v[0] for k, v in reached.items()}
    assert {v[0] for v in reached.values()} == {0, 1, 2}, {k: v[0] for k, v in reached.items()}
    for (name, reorder), (route, plan, G) in reached.items():
        for H, F in ((4, 16), (8, 16), (2, 64)):  # H·F = 64 or 128 throughout, so a plan's route holds; H grows, then shrinks
            if plan.sddmm_heads_route(H, F) != route:
                continue
            D1, D2 = _rand(G["M"], H, F, 101 + H), _rand(G["K"], H, F, 102 + H)
            want = sddmm.csr_sddmm_heads(G["rp"], G["ci"], D1, D2)
            for call in range(2):
                _same(_csr(sddmm, G, D1, D2, plan=plan), want, (name, reorder, route, H, F, call))
    other = spmm.SpmmPlan(dense["rp"], dense["ci"], dense["K"], 32, reorder=False)
    with pytest.raises(ValueError):
        sddmm.csr_sddmm_heads(pub["rp"], pub["ci"], _rand(pub["M"], 2, 4, 1), _rand(pub["K"], 2, 4, 2), plan=other)


# --------------------------------------------------------------------------------------------------------------- 6. autograd

def test_autograd_score(pkg, bundled, monkeypatch):
    """MultiHeadSDDMMFunction on pubmed, (H, F) = (4, 16): forward = csr_sddmm_heads; grad_q and grad_k are the two csr_spmm_heads calls
    written out, and within the float64 rule of the dense formula; no product runs for an input that needs no gradient."""
    import gespmm_amd
    from gespmm_amd import graphs, sddmm, spmm

    G = _up(bundled["pubmed"])
    H, F = 4, 16
    rp, ci = G["rp"], G["ci"]
    colptr, rowind, order = graphs.transpose_csr(rp, ci, G["K"], return_order=True)
    q = _rand(G["M"], H, F, 111).requires_grad_(True)
    k = _rand(G["K"], H, F, 112).requires_grad_(True)
    gs = (torch.rand(G["nnz"], H, device="cuda", generator=torch.Generator(device="cuda").manual_seed(113)) - 0.5)
    s = gespmm_amd.MultiHeadSDDMMFunction.apply(rp, ci, colptr, rowind, order, q, k)
    _same(s.detach(), sddmm.csr_sddmm_heads(rp, ci, q.detach(), k.detach()), "forward")
    s.backward(gs)
    _same(q.grad, spmm.csr_spmm_heads(rp, ci, gs, k.detach()), "grad_q")
    _same(k.grad, spmm.csr_spmm_heads(colptr, rowind, gs[order].contiguous(), q.detach()), "grad_k")
    # dense formula in float64: grad_q[r] = sum_e gs[e] k[col(e)], grad_k[c] = sum_e gs[e] q[row(e)]; |err| <= 1e-4 max(|ref|, sum |terms|)
    ri, cl = G["ri"].long(), ci.long()
    for got, dst, src, n in ((q.grad, ri, k.detach()[cl], G["M"]), (k.grad, cl, q.detach()[ri], G["K"])):
        terms = gs.double().unsqueeze(-1) * src.double()
        ref = torch.zeros(n, H, F, dtype=torch.float64, device="cuda").index_add_(0, dst, terms)
        scale = torch.zeros(n, H, F, dtype=torch.float64, device="cuda").index_add_(0, dst, terms.abs())
        err = (got.double() - ref).abs()
        bound = 1e-4 * torch.maximum(ref.abs(), scale)
        print("max err %.3e" % err.max().item())
        assert bool((err <= bound).all())
    calls = []
    real = spmm.csr_spmm_heads
    monkeypatch.setattr(spmm, "csr_spmm_heads", lambda *a, **kw: (calls.append(a[0].data_ptr()), real(*a, **kw))[1])
    q2, k2 = q.detach().clone().requires_grad_(True), k.detach().clone()
    gespmm_amd.MultiHeadSDDMMFunction.apply(rp, ci, colptr, rowind, order, q2, k2).backward(gs)
    assert calls == [rp.data_ptr()] and k2.grad is None
    _same(q2.grad, q.grad, "grad_q alone")
    del calls[:]
    q3, k3 = q.detach().clone(), k.detach().clone().requires_grad_(True)
    gespmm_amd.MultiHeadSDDMMFunction.apply(rp, ci, colptr, rowind, order, q3, k3).backward(gs)
    assert calls == [colptr.data_ptr()] and q3.grad is None
    _same(k3.grad, k.grad, "grad_k alone")


def test_autograd_edge_weight_gradient_in_one_call(pkg, bundled, monkeypatch):
    """MultiHeadSPMMFunction(..., heads_sddmm=True): grad_weight has the bits of the default path and sddmm.csr_sddmm never runs."""
    import gespmm_amd
    from gespmm_amd import graphs, sddmm, spmm

    G = _up(bundled["pubmed"])
    H, F = 4, 16
    rp, ci = G["rp"], G["ci"]
    colptr, rowind, order = graphs.transpose_csr(rp, ci, G["K"], return_order=True)
    feat, weight = _rand(G["K"], H, F, 121), _rand(G["nnz"], 1, H, 122).view(G["nnz"], H)
    grad_out = _rand(G["M"], H, F, 123)
    grads = {}
    calls = []
    real = sddmm.csr_sddmm
    monkeypatch.setattr(sddmm, "csr_sddmm", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    for setting, plans in ((False, None), (True, None), (True, "plans")):
        if plans:
            plans = (spmm.SpmmPlan(rp, ci, G["K"], H * F, reorder=True), spmm.SpmmPlan(colptr, rowind, G["M"], H * F, reorder=True))
        f, w = feat.clone().requires_grad_(True), weight.clone().requires_grad_(True)
        del calls[:]
        gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, f, w, plans, setting).backward(grad_out)
        assert len(calls) == (0 if setting else H), (setting, calls)
        grads[(setting, plans is not None)] = (f.grad, w.grad)
    for key in ((True, False), (True, True)):
        _same(grads[key][1], grads[(False, False)][1], ("grad_weight", key))
        _same(grads[key][0], grads[(False, False)][0], ("grad_feat", key))


# ----------------------------------------------------------------------------------------------------------------- 7. errors

def test_python_errors_raise_without_launching(pkg, edge):
    from gespmm_amd import sddmm, spmm

    G = edge
    D1, D2 = _rand(G["M"], 4, 8, 1), _rand(G["K"], 4, 8, 2)
    csr = lambda a, b, **kw: sddmm.csr_sddmm_heads(G["rp"], G["ci"], a, b, **kw)  # noqa: E731
    coo = lambda a, b: sddmm.coo_sddmm_heads(G["ri"], G["ci"], a, b)  # noqa: E731
    for f in (csr, coo):
        with pytest.raises(ValueError):
            f(D1.view(G["M"], 32), D2.view(G["K"], 32))  # rank 2: H comes from the shape
        with pytest.raises(ValueError):
            f(D1, D2.view(G["K"], 32))
        for dt in (torch.float16, torch.bfloat16, torch.float64):
            with pytest.raises(TypeError):
                f(D1.to(dt), D2.to(dt))
        with pytest.raises(TypeError):
            f(D1, D2.half())
        with pytest.raises(TypeError):
            f(D1.double(), D2)
        with pytest.raises(ValueError):
            f(D1, _rand(G["K"], 2, 16, 3))  # H mismatch
        with pytest.raises(ValueError):
            f(D1, _rand(G["K"], 4, 4, 3))   # F mismatch
        with pytest.raises(ValueError):
            f(_rand(G["M"], 4, 16, 3)[:, :, ::2], D2)  # non-contiguous
        with pytest.raises(RuntimeError):
            f(D1.cpu(), D2)
        with pytest.raises(RuntimeError):
            f(D1, D2.cpu())
    with pytest.raises(RuntimeError):
        sddmm.csr_sddmm_heads(G["rp"].cpu(), G["ci"], D1, D2)
    with pytest.raises(TypeError):
        sddmm.csr_sddmm_heads(G["rp"].long(), G["ci"], D1, D2)
    with pytest.raises(ValueError):
        csr(D1[:-1].contiguous(), D2)  # rowptr must have D1.size(0) + 1 entries
    with pytest.raises(ValueError):
        sddmm.coo_sddmm_heads(G["ri"][:-1].contiguous(), G["ci"], D1, D2)
    for bad in (torch.empty(G["nnz"], 3, device="cuda"), torch.empty(G["nnz"] + 1, 4, device="cuda"), torch.empty(G["nnz"] * 4, device="cuda"),
                torch.empty(G["nnz"], 8, device="cuda")[:, ::2]):
        with pytest.raises(ValueError):
            csr(D1, D2, out=bad)
    with pytest.raises(TypeError):
        csr(D1, D2, out=torch.empty(G["nnz"], 4, device="cuda", dtype=torch.float64))
    plan = spmm.SpmmPlan(G["rp"], G["ci"], G["K"], 32, reorder=False)
    with pytest.raises(ValueError):
        sddmm.csr_sddmm_heads(G["rp"].clone(), G["ci"], D1, D2, plan=plan)
