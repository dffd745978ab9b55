"""Fused GAT aggregation on the GPU (softmax.gat_softmax_stats, spmm.gat_aggregate): attention output without an alpha array.

The composition it replaces is the oracle for every bit — ``csr_spmm_heads`` on the ``alpha`` of ``gat_edge_softmax``, on the CSR
arrays and, with ``alpha[csc_order]``, on the CSC arrays — and a float64 restatement on the host (softmax, then product) checks BOTH
inside the project's bound 1e-4 max(|ref|, sum |w b|). Patterns, their asserted lane widths and the terms are those of
tests/test_gpu_gat_softmax.py; every result is written into a NaN-prefilled tensor with guard words behind it."""
import os
import re

import numpy as np
import pytest
import torch

from attention_refs import gat_aggregate_float64
from helpers import ROOT
from test_gat_softmax_host import csc_of
from test_gpu_edge_softmax import NAN, _dev, _guard_ok, _out, _same
from test_gpu_gat_softmax import PATTERNS, SLOPES, _terms, patterns  # noqa: F401  (patterns: the module's fixture, W asserted there)
from test_gpu_heads import _carve, _short_rows
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

HEADS = (1, 3, 8, 33)
KERNEL_HF = ((1, 8), (1, 64), (2, 1), (2, 2), (3, 5), (4, 2), (4, 4), (8, 8), (5, 13), (8, 16), (4, 32), (7, 27), (8, 64))
COMPOSED_HF = ((9, 4), (33, 2))
PIN = "GESPMM_GAT_AGGREGATE_ROUTE"


@pytest.fixture(scope="module")
def graphs_(patterns):  # noqa: F811
    """The patterns with their CSC arrays (csc_of on the host) on the device, and a cache of what several tests need of a
    (pattern, H, slope): the terms, alpha by gat_edge_softmax, its CSC-ordered copy and the statistics — computed once, never edited."""
    out = {}
    for name in PATTERNS:
        G = dict(patterns[name])
        # (mean8 is 64 x 64, but as little symmetric as the others: rows and columns are scored by different terms)
        assert G["M"] != G["K"] or name == "mean8", "swapped roles of the two indices must show"
        colptr_h, order_h = csc_of(G["rowptr"], G["colind"], G["K"])
        rows_h = np.repeat(np.arange(G["M"], dtype=np.int32), np.diff(G["rowptr"]))
        G["rows_h"], G["colptr_h"], G["order_h"] = rows_h, colptr_h, order_h
        G["cp"], G["ri"], G["order"] = _dev(colptr_h), _dev(rows_h[order_h]), _dev(order_h).long()
        G["cache"] = {}
        out[name] = G
    return out


def _stats(G, el, er, slope):
    from gespmm_amd import softmax

    buf, out = _out((G["M"], el.shape[1], 2))
    assert softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=slope, out=out) is out
    _guard_ok(buf, "stats")
    assert not bool(torch.isnan(out).any()), "every word of stats must be written"
    return out


def _case(G, H, slope):
    """-> dict(el, er, alpha, alpha_csc, stats) of (pattern, H, slope), shared by the tests."""
    from gespmm_amd import softmax

    key = (H, slope)
    if key not in G["cache"]:
        el, er, _ = _terms(G, H, 2000 + 7 * H + G["nnz"] % 13)
        alpha = softmax.gat_edge_softmax(G["rp"], G["ci"], el, er, negative_slope=slope)
        G["cache"][key] = {"el": el, "er": er, "alpha": alpha, "alpha_csc": alpha[G["order"]].contiguous(),
                           "stats": _stats(G, el, er, slope)}
    return G["cache"][key]


def _feat(rows, H, F, seed):
    rng = np.random.RandomState(seed)
    return _dev((rng.rand(rows, H, F) - 0.5).astype(np.float32))  # within +-0.5


def _aggregate(G, c, dense, slope, transposed, align=16):
    """gat_aggregate into a NaN-prefilled, guarded tensor whose address `align` divides."""
    from gespmm_amd import spmm

    S = G["K"] if transposed else G["M"]
    buf, out = _out((S,) + tuple(dense.shape[1:]))
    if align != 16:
        out = _carve(out, align)
        out.fill_(NAN)
    ptr, ind = (G["cp"], G["ri"]) if transposed else (G["rp"], G["ci"])
    r = spmm.gat_aggregate(ptr, ind, c["el"], c["er"], c["stats"], dense, negative_slope=slope, transposed=transposed, out=out)
    assert r is out
    if align == 16:
        _guard_ok(buf, "aggregate")
    return out


def _composition(G, c, dense, transposed):
    from gespmm_amd import spmm

    if transposed:
        return spmm.csr_spmm_heads(G["cp"], G["ri"], c["alpha_csc"], dense)
    return spmm.csr_spmm_heads(G["rp"], G["ci"], c["alpha"], dense)


def _route(G, H, F, transposed, align=16):
    from gespmm_amd import _lib

    return _lib.gat_aggregate_route(G["M"], G["K"], H, F, G["nnz"], transposed, align, align)


# ------------------------------------------------------------------------------------------------------------------- 1. stats

@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", HEADS)
def test_stats(pkg, graphs_, H, slope):
    seen_empty = False
    for name in PATTERNS:
        G = graphs_[name]
        c = _case(G, H, slope)
        st = c["stats"]
        x = c["el"][G["rows"]] + c["er"][G["ci"].long()]  # fl(el + er), one fp32 add
        if slope is not None:
            x = torch.where(x >= 0, x, x * slope)
        top = torch.full((G["M"], H), -float("inf"), device="cuda").scatter_reduce(0, G["rows"][:, None].expand(-1, H), x, "amax")
        deg = torch.diff(G["rp"]).long()
        empty, one = deg == 0, deg == 1
        assert bool(one.any()) and bool((deg > 1).any()), name
        seen_empty = seen_empty or bool(empty.any())
        top[empty] = 0.0
        _same(st[:, :, 0], top, "%s H=%d slope=%s: m is the row maximum of leaky(fl(el + er))" % (name, H, slope))
        s = st[:, :, 1]
        assert bool((st[empty].view(torch.int32) == 0).all()), "empty rows are (+0, +0)"
        assert bool((s[one] == 1.0).all()), "a row of one entry sums exp(0)"
        d = deg[~empty].float()[:, None]
        assert bool((s[~empty] >= 1.0).all()) and bool((s[~empty] <= d * (1 + 2.0 ** -20)).all()), (name, H, slope)
    assert seen_empty, "no pattern had an empty row"


# ----------------------------------------------------------------------------------------------------- 2. forward, 3. transposed

@pytest.mark.parametrize("transposed", (False, True))
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,F", KERNEL_HF + COMPOSED_HF)
def test_equals_the_composition(pkg, graphs_, H, F, slope, transposed, monkeypatch):
    monkeypatch.delenv(PIN, raising=False)
    for name in PATTERNS:
        G = graphs_[name]
        c = _case(G, H, slope)
        assert _route(G, H, F, transposed)[0] == (1 if (H, F) in KERNEL_HF else 0), (name, H, F)
        dense = _feat(G["M"] if transposed else G["K"], H, F, 300 + H * F)
        want = _composition(G, c, dense, transposed)
        _same(_aggregate(G, c, dense, slope, transposed), want, (name, H, F, slope, transposed))
        if (H, F) == (5, 13):  # rank 2 in, rank 2 out, the same numbers
            out2 = _aggregate(G, c, dense.view(dense.shape[0], H * F), slope, transposed)
            assert out2.dim() == 2
            _same(out2.view(want.shape), want, "rank 2")


@pytest.mark.parametrize("transposed", (False, True))
def test_pinned_composition(pkg, graphs_, transposed, monkeypatch):
    monkeypatch.delenv(PIN, raising=False)
    H, F = 8, 8
    for name in PATTERNS:
        G = graphs_[name]
        c = _case(G, H, 0.2)
        dense = _feat(G["M"] if transposed else G["K"], H, F, 17)
        want = _composition(G, c, dense, transposed)
        assert _route(G, H, F, transposed)[0] == 1
        monkeypatch.setenv(PIN, "composition")
        assert _route(G, H, F, transposed)[0] == 0
        _same(_aggregate(G, c, dense, 0.2, transposed), want, (name, "pinned"))
        monkeypatch.delenv(PIN)


def _launch_table():
    """The (V, S, W) of gat_aggregate.hip's launch table, read from the table itself; each exists forward and transposed."""
    text = open(os.path.join(ROOT, "gespmm_amd", "csrc", "gat_aggregate.hip")).read()
    body = text[text.index("#define GESPMM_GAT("):text.index("#undef GESPMM_GAT")]
    return {(int(v), int(s), int(w)) for v, s, w in re.findall(r"^\s*GESPMM_GAT\((\d), (\d), (\d+)\)", body, flags=re.M)}


def test_every_instantiation_of_the_launch_table_runs(pkg, graphs_, monkeypatch):
    """The storage-order cases of tests/test_gpu_heads.py. Forward on a pattern; transposed on the SAME arrays read as the CSC arrays
    of the transposed matrix (colptr' = rowptr, rowind' = colind, M' = K, K' = M), which has the same segments and so the same
    geometry: both kernels of every (V, S, W) run."""
    from gespmm_amd import _lib, graphs, softmax, spmm

    monkeypatch.delenv(PIN, raising=False)
    table = _launch_table()
    assert len(table) == 11, sorted(table)
    edge = graphs_["edge"]
    big = _short_rows(1 << 17, 500, seed=3)
    for g in (edge, big):
        # the transposed matrix in CSR order, and where each of ITS entries sits in the arrays above (its CSC order)
        g["t_rp"], g["t_ci"], order = graphs.transpose_csr(g["rp"], g["ci"], g["K"], return_order=True)
        g["t_inv"] = torch.empty_like(order)
        g["t_inv"][order] = torch.arange(order.numel(), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(11)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=gen) - 0.5  # noqa: E731
    cases = [(edge, H, F, 16) for H, F in ((2, 2), (8, 1), (8, 2), (8, 4), (4, 16), (8, 16), (8, 32), (3, 24))]
    cases += [(edge, 8, 16, 8), (edge, 8, 32, 8), (edge, 8, 16, 4), (edge, 5, 13, 16), (big, 8, 40, 16)]
    reached = {False: set(), True: set()}
    for g, H, F, align in cases:
        M, K, nnz = g["M"], g["K"], g["nnz"]
        B3 = rand(K, H, F)
        Bc = _carve(B3, align)
        # ---- forward
        route, (V, S, W, rpw) = _lib.gat_aggregate_route(M, K, H, F, nnz, False, align, align)
        assert route == 1, (H, F, align)
        el, er = rand(M, H) * 32, rand(K, H) * 32
        stats = softmax.gat_softmax_stats(g["rp"], g["ci"], el, er, negative_slope=0.2)
        alpha = softmax.gat_edge_softmax(g["rp"], g["ci"], el, er, negative_slope=0.2)
        out = _carve(torch.full((M, H, F), NAN, device="cuda"), align)
        spmm.gat_aggregate(g["rp"], g["ci"], el, er, stats, Bc, negative_slope=0.2, out=out)
        _same(out, spmm.csr_spmm_heads(g["rp"], g["ci"], alpha, B3), ("forward", H, F, align, V, S, W))
        reached[False].add((V, S, W))
        # ---- transposed: the matrix is the transpose (K rows, M columns); el_t scores ITS rows
        route, (V, S, W, rpw) = _lib.gat_aggregate_route(K, M, H, F, nnz, True, align, align)
        assert route == 1, (H, F, align)
        el_t, er_t = rand(K, H) * 32, rand(M, H) * 32
        stats_t = softmax.gat_softmax_stats(g["t_rp"], g["t_ci"], el_t, er_t, negative_slope=0.2)
        alpha_t = softmax.gat_edge_softmax(g["t_rp"], g["t_ci"], el_t, er_t, negative_slope=0.2)
        out = _carve(torch.full((M, H, F), NAN, device="cuda"), align)
        spmm.gat_aggregate(g["rp"], g["ci"], el_t, er_t, stats_t, Bc, negative_slope=0.2, transposed=True, out=out)
        _same(out, spmm.csr_spmm_heads(g["rp"], g["ci"], alpha_t[g["t_inv"]].contiguous(), B3), ("transposed", H, F, align, V, S, W))
        reached[True].add((V, S, W))
    assert reached[False] == table and reached[True] == table, (sorted(reached[False]), sorted(reached[True]), sorted(table))


# ---------------------------------------------------------------------------------------------------------- 4. independent check

@pytest.mark.parametrize("transposed", (False, True))
@pytest.mark.parametrize("H,F", ((4, 2), (8, 8), (1, 64)))
def test_against_float64(pkg, graphs_, H, F, transposed, monkeypatch):
    """The new kernel AND the composition it is compared with elsewhere, each inside 1e-4 max(|ref|, sum |w b|) of float64."""
    monkeypatch.delenv(PIN, raising=False)
    for name in ("edge", "padded"):
        G = graphs_[name]
        for slope in SLOPES:
            c = _case(G, H, slope)
            dense = _feat(G["M"] if transposed else G["K"], H, F, 900 + H + F)
            ref, mag = gat_aggregate_float64(G["rows_h"], G["colind"], G["M"], G["K"], c["el"].cpu().numpy(), c["er"].cpu().numpy(),
                                             dense.cpu().numpy(), slope, transposed)
            bound = 1e-4 * np.maximum(np.abs(ref), mag)
            assert _route(G, H, F, transposed)[0] == 1
            for what, got in (("kernel", _aggregate(G, c, dense, slope, transposed)), ("composition", _composition(G, c, dense, transposed))):
                err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                worst = float((err / np.where(bound > 0, bound, 1.0)).max())
                print("%s %s H=%d F=%d slope=%s transposed=%s: worst error / bound %.4f" % (name, what, H, F, slope, transposed, worst))
                assert np.all(err <= bound), (name, what, H, F, slope, transposed, worst)


# ------------------------------------------------------------------------------------------------------------------ 5. bad inputs

@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_bad_el_poisons_what_it_poisons_in_the_composition(pkg, graphs_, bad, monkeypatch):
    from gespmm_amd import softmax

    monkeypatch.delenv(PIN, raising=False)
    H, F = 8, 8
    for name, row in (("edge", 3), ("short", 4)):  # a swept row at W = 16, a hub row at W = 4
        G = graphs_[name]
        el, er, _ = _terms(G, H, 77)
        el[row, 2] = bad
        for slope in SLOPES:
            c = {"el": el, "er": er, "alpha": softmax.gat_edge_softmax(G["rp"], G["ci"], el, er, negative_slope=slope),
                 "stats": _stats_unchecked(G, el, er, slope)}
            c["alpha_csc"] = c["alpha"][G["order"]].contiguous()
            assert bool(torch.isnan(c["alpha"]).any())
            for transposed in (False, True):
                dense = _feat(G["M"] if transposed else G["K"], H, F, 5)
                got, want = _aggregate(G, c, dense, slope, transposed), _composition(G, c, dense, transposed)
                nan_g, nan_w = torch.isnan(got), torch.isnan(want)
                assert bool(nan_w.any()) and not bool(nan_w.all()) and torch.equal(nan_g, nan_w), (name, slope, transposed)
                _same(torch.where(nan_g, torch.zeros_like(got), got), torch.where(nan_w, torch.zeros_like(want), want),
                      (name, slope, transposed))


def _stats_unchecked(G, el, er, slope):
    """The statistics of terms that hold a NaN: no NaN check on the result."""
    from gespmm_amd import softmax

    buf, out = _out((G["M"], el.shape[1], 2))
    softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=slope, out=out)
    _guard_ok(buf, "stats")
    return out


# ---------------------------------------------------------------------------------------------------------------------- 6. capture

def test_capture_equals_eager(pkg, graphs_, monkeypatch):
    """stats + aggregate, forward and transposed, captured together (a linear capture); replays see operands edited in place."""
    from gespmm_amd import softmax, spmm

    monkeypatch.delenv(PIN, raising=False)
    G, H, F = graphs_["edge"], 8, 8
    el, er, _ = _terms(G, H, 31)
    feat, gout = _feat(G["K"], H, F, 1), _feat(G["M"], H, F, 2)
    buf_s, stats = _out((G["M"], H, 2))
    buf_o, out = _out((G["M"], H, F))
    buf_t, out_t = _out((G["K"], H, F))

    def step():
        softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2, out=stats)
        spmm.gat_aggregate(G["rp"], G["ci"], el, er, stats, feat, negative_slope=0.2, out=out)
        spmm.gat_aggregate(G["cp"], G["ri"], el, er, stats, gout, negative_slope=0.2, transposed=True, out=out_t)

    graph, _ = _capture(step)
    for seed in (33, 35):
        el2, er2, _ = _terms(G, H, seed)
        el.copy_(el2)
        er.copy_(er2)
        for b in (buf_s, buf_o, buf_t):
            b.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for b in (buf_s, buf_o, buf_t):
            _guard_ok(b, "replay")
        c = {"el": el, "er": er, "stats": _stats(G, el, er, 0.2)}
        _same(stats, c["stats"], "replayed stats vs eager")
        _same(out, _aggregate(G, c, feat, 0.2, False), "replayed forward vs eager")
        _same(out_t, _aggregate(G, c, gout, 0.2, True), "replayed transposed vs eager")


# ------------------------------------------------------------------------------------------------------------------- 7. no entries

def test_no_entries(pkg):
    from gespmm_amd import softmax, spmm

    M, K, H, F = 7, 5, 3, 4
    rp0, cp0 = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    i0 = torch.empty(0, dtype=torch.int32, device="cuda")
    el, er = torch.ones(M, H, device="cuda"), torch.ones(K, H, device="cuda")
    buf, stats = _out((M, H, 2))
    softmax.gat_softmax_stats(rp0, i0, el, er, negative_slope=0.2, out=stats)
    _guard_ok(buf)
    assert bool((stats.view(torch.int32) == 0).all())
    for transposed, ptr, S, Kb in ((False, rp0, M, K), (True, cp0, K, M)):
        buf, out = _out((S, H, F))
        spmm.gat_aggregate(ptr, i0, el, er, stats, torch.ones(Kb, H, F, device="cuda"), negative_slope=0.2, transposed=transposed, out=out)
        _guard_ok(buf)
        assert bool((out.view(torch.int32) == 0).all()), transposed


# ---------------------------------------------------------------------------------------------------------------- 8. Python errors

def test_python_errors_raise_without_launching(pkg, graphs_):
    from gespmm_amd import softmax, spmm

    G, H, F = graphs_["edge"], 4, 2
    rp, ci, cp, ri, M, K = G["rp"], G["ci"], G["cp"], G["ri"], G["M"], G["K"]
    c = _case(G, H, 0.2)
    el, er, st = c["el"], c["er"], c["stats"]
    feat, gout = _feat(K, H, F, 1), _feat(M, H, F, 2)
    stats = lambda *a, **kw: softmax.gat_softmax_stats(*a, **kw)  # noqa: E731
    agg = lambda *a, **kw: spmm.gat_aggregate(*a, **kw)  # noqa: E731
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        for call in (lambda: stats(rp, ci, el.to(dt), er), lambda: stats(rp, ci, el, er.to(dt)),
                     lambda: stats(rp, ci, el, er, out=torch.empty(M, H, 2, device="cuda", dtype=dt)),
                     lambda: agg(rp, ci, el.to(dt), er, st, feat), lambda: agg(rp, ci, el, er, st.to(dt), feat),
                     lambda: agg(rp, ci, el, er, st, feat.to(dt)),
                     lambda: agg(rp, ci, el, er, st, feat, out=torch.empty(M, H, F, device="cuda", dtype=dt))):
            with pytest.raises(TypeError):
                call()
    for call in (lambda: stats(rp.long(), ci, el, er), lambda: stats(rp, ci.long(), el, er), lambda: agg(rp.long(), ci, el, er, st, feat),
                 lambda: agg(rp, ci.long(), el, er, st, feat), lambda: agg(rp, ci, el, er, st, feat.cpu().numpy())):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: stats(rp, ci, el[:-1], er), lambda: stats(rp, ci, el, er[:, :-1].contiguous()),
                 lambda: stats(rp, ci, el.cpu(), er), lambda: stats(rp.cpu(), ci, el, er), lambda: stats(rp, ci.cpu(), el, er),
                 lambda: stats(rp, ci, el, er, out=torch.empty(M, H, device="cuda")),
                 lambda: stats(rp, ci, el, er, out=torch.empty(M, H, 2)),
                 lambda: stats(rp, ci, el, er, out=torch.empty(M, H, 4, device="cuda")[:, :, ::2]),
                 lambda: stats(rp, ci, el, er, negative_slope=float("nan")),
                 lambda: agg(cp, ri, el, er, st, feat),                       # colptr without transposed=True: K + 1 entries
                 lambda: agg(rp, ci, el, er, st, gout, transposed=True),      # ... and the reverse
                 lambda: agg(rp, ci, el, er, st, gout),                       # dense with M rows, K wanted
                 lambda: agg(rp, ci, el, er, st[:-1], feat), lambda: agg(rp, ci, el, er, st.view(M, 2 * H), feat),
                 lambda: agg(rp, ci, el, er, st, feat.view(K, F, H)),         # H is not dense's second dimension
                 lambda: agg(rp, ci, el, er, st, feat.view(-1)),
                 lambda: agg(rp, ci, el, er, st, torch.empty(K, H, 2 * F, device="cuda")[:, :, ::2]),
                 lambda: agg(rp, ci, el, er, st.cpu(), feat), lambda: agg(rp, ci, el, er, st, feat.cpu()),
                 lambda: agg(rp, ci.cpu(), el, er, st, feat),
                 lambda: agg(rp, ci, el, er, st, feat, out=torch.empty(M + 1, H, F, device="cuda")),
                 lambda: agg(rp, ci, el, er, st, feat, out=torch.empty(M, H, F)),
                 lambda: agg(rp, ci, el, er, st, feat, out=feat.view(-1)[:M * H * F].view(M, H, F))):     # out overlaps dense
        with pytest.raises(ValueError):
            call()
    # nothing was launched: the cached operands are what they were
    _same(st, _stats(G, el, er, 0.2), "stats untouched")
