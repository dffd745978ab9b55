"""Dropout on the attention coefficients on the GPU: ``softmax.edge_dropout`` and the ``dropout=(p, seed)`` forms of
``spmm.gat_aggregate``, ``softmax.gat_backward_el`` and ``softmax.gat_backward_er``.

The mask is a pure function of (seed, row, column, head), so a numpy restatement of it on the host pattern is the oracle for every
decision, and the compositions with ``edge_dropout`` in them are the oracle for every bit of the fused forms: ``csr_spmm_heads`` on
``edge_dropout(gat_edge_softmax(..))`` for the aggregation in both walks, and ``gat_edge_softmax`` -> ``csr_sddmm_heads`` ->
``edge_dropout`` -> ``gat_edge_softmax_backward`` -> ``edge_segment_sum`` for the backward wherever the dot is exact. Patterns, terms
and helpers are those of tests/test_gpu_gat_backward.py (the five patterns and the transpose of ``short``: the register regime, the
sweep regime and the hub branch, in rows and in columns); every result goes into a NaN-prefilled tensor with guard words behind it."""
import numpy as np
import pytest
import torch

from attention_refs import gat_backward_float64
from test_edge_dropout_host import restate
from test_gpu_edge_softmax import NAN, _dev, _guard_ok, _out, _same
from test_gpu_gat_aggregate import PIN
from test_gpu_gat_backward import ALL, _case, _ints, _reals, graphs_  # noqa: F401  (graphs_: the module's fixture)
from test_gpu_gat_softmax import SLOPES, _terms, patterns  # noqa: F401  (patterns: the fixture graphs_ is built on)
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

SEEDS = ((0x12345678, 0x9ABCDEF0), (0xFFFFFFFF, 7))
PS = (0.5, 0.6)
HF = ((1, 1), (1, 64), (3, 5), (4, 16), (8, 8), (7, 27))


def _seed(pair):
    return _dev(np.array(pair, dtype=np.uint32).view(np.int32))


def _keep(G, pair, p, H):
    """The numpy mask of the pattern -> bool[nnz, H] in CSR order."""
    from gespmm_amd import _lib

    bits = restate(pair[0], pair[1], G["rows_h"].astype(np.uint64)[:, None], G["colind"].astype(np.uint64)[:, None],
                   np.arange(H, dtype=np.uint64)[None, :])
    return bits >= np.uint32(_lib.edge_dropout_threshold(p))


def _scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def _dropped(G, x, p, pair, out=None):
    from gespmm_amd import softmax

    buf = None
    if out is None:
        buf, out = _out(tuple(x.shape))
    r = softmax.edge_dropout(G["rp"], G["ci"], x, p, _seed(pair), out=out)
    assert r is out
    if buf is not None:
        _guard_ok(buf, "edge_dropout")
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. edge_dropout

@pytest.mark.parametrize("pair", SEEDS)
@pytest.mark.parametrize("p", PS)
def test_edge_dropout_equals_the_restatement(pkg, graphs_, p, pair):
    for name in ALL:
        G = graphs_[name]
        for H in (1, 3, 8):
            x = _dev(((np.random.RandomState(H).rand(G["nnz"], H) - 0.5) * 4).astype(np.float32))
            keep = _keep(G, pair, p, H)
            assert 0 < keep.sum() < keep.size
            want = np.where(keep, x.cpu().numpy() * _scale(p), np.float32(0.0)).astype(np.float32)
            got = _dropped(G, x, p, pair)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (name, H)
            y = x.clone()
            assert _dropped(G, y, p, pair, out=y) is y  # in place
            _same(y, got, "%s H=%d: in place" % (name, H))
        x1 = _dev(np.random.RandomState(9).rand(G["nnz"]).astype(np.float32))  # one-dimensional: H = 1
        _same(_dropped(G, x1, p, pair).view(-1, 1), _dropped(G, x1.view(-1, 1).contiguous(), p, pair), name + ": rank 1")


def test_edge_dropout_selects_and_p_zero_is_the_identity(pkg, graphs_):
    G, H, pair, p = graphs_["edge"], 4, SEEDS[0], 0.6
    keep = _keep(G, pair, p, H)
    x = torch.ones(G["nnz"], H, device="cuda")
    for bad in (float("nan"), float("inf"), -float("inf")):
        xb = torch.full_like(x, bad)
        got = _dropped(G, xb, p, pair).cpu().numpy()
        assert np.all(got[~keep].view(np.uint32) == 0), "a dropped %r is +0" % bad
        want_kept = (np.float32(bad) * _scale(p)).astype(np.float32)
        assert np.array_equal(got[keep].view(np.uint32), np.full(int(keep.sum()), want_kept, dtype=np.float32).view(np.uint32)) or (
            np.isnan(want_kept) and np.all(np.isnan(got[keep])))
    xr = _dev(((np.random.RandomState(1).rand(G["nnz"], H) - 0.5) * 4).astype(np.float32))
    xr[0, 0], xr[1, 1], xr[2, 2] = float("nan"), float("inf"), -0.0
    for pair0 in SEEDS:
        _same(_dropped(G, xr, 0.0, pair0), xr, "p = 0 returns x's bits")


# ------------------------------------------------------------------------------------------------------------------ 2. aggregation

def _aggregate(G, c, dense, slope, transposed, drop):
    from gespmm_amd import spmm

    S = G["K"] if transposed else G["M"]
    buf, out = _out((S,) + tuple(dense.shape[1:]))
    ptr, ind = (G["cp"], G["ri"]) if transposed else (G["rp"], G["ci"])
    r = spmm.gat_aggregate(ptr, ind, c["el"], c["er"], c["stats"], dense, negative_slope=slope, transposed=transposed, out=out, dropout=drop)
    assert r is out
    _guard_ok(buf, "gat_aggregate")
    return out


def _alpha_dropped(G, c, slope, p, pair):
    from gespmm_amd import softmax

    alpha = softmax.gat_edge_softmax(G["rp"], G["ci"], c["el"], c["er"], negative_slope=slope)
    return _dropped(G, alpha, p, pair)


def _aggregate_composition(G, alpha_d, dense, transposed):
    from gespmm_amd import spmm

    if transposed:
        return spmm.csr_spmm_heads(G["cp"], G["ri"], alpha_d[G["order"].long()].contiguous(), dense)
    return spmm.csr_spmm_heads(G["rp"], G["ci"], alpha_d, dense)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,F", HF + ((9, 2),))
def test_aggregate_equals_the_composition(pkg, graphs_, H, F, slope, monkeypatch):
    from gespmm_amd import _lib

    monkeypatch.delenv(PIN, raising=False)
    for i, name in enumerate(ALL):
        G = graphs_[name]
        c = _case(G, H, slope)
        p, pair = PS[i % 2], SEEDS[(i // 2) % 2]
        alpha_d = _alpha_dropped(G, c, slope, p, pair)
        for transposed in (False, True):
            assert _lib.gat_aggregate_route(G["M"], G["K"], H, F, G["nnz"], transposed, 16, 16)[0] == (0 if H == 9 else 1)
            dense = _reals(G["M"] if transposed else G["K"], H, F, 300 + H * F)
            want = _aggregate_composition(G, alpha_d, dense, transposed)
            got = _aggregate(G, c, dense, slope, transposed, (p, _seed(pair)))
            _same(got, want, (name, H, F, slope, transposed, p))
            if H == 8:  # the pinned composition route applies the same expression to its temporary
                monkeypatch.setenv(PIN, "composition")
                _same(_aggregate(G, c, dense, slope, transposed, (p, _seed(pair))), want, (name, "pinned", transposed))
                monkeypatch.delenv(PIN)
            base = _aggregate(G, c, dense, slope, transposed, None)
            _same(_aggregate(G, c, dense, slope, transposed, (0.0, _seed(pair))), base, (name, H, F, "p = 0 is the base call"))
            assert not bool(torch.equal(got, base)) or G["nnz"] == 0


def test_a_row_whose_entries_are_all_dropped_is_zero(pkg, graphs_, monkeypatch):
    """The seed is searched with the restatement so that some non-empty row of ``edge`` loses every entry of a head at p = 0.6."""
    monkeypatch.delenv(PIN, raising=False)
    G, H, F, p = graphs_["edge"], 4, 16, 0.6
    deg = np.diff(G["rowptr"])
    found = None
    for s1 in range(200):
        keep = _keep(G, (s1, 5), p, H)
        kept = np.zeros((G["M"], H), dtype=np.int64)
        np.add.at(kept, G["rows_h"], keep)
        hit = np.argwhere((kept == 0) & (deg[:, None] > 0))
        if hit.size:
            found = ((s1, 5), hit)
            break
    assert found is not None, "no seed below 200 drops a whole row: the search, not the kernel, needs another pattern"
    pair, hit = found
    c = _case(G, H, 0.2)
    out = _aggregate(G, c, torch.ones(G["K"], H, F, device="cuda"), 0.2, False, (p, _seed(pair))).cpu().numpy()
    for r, h in hit:
        assert np.all(out[r, h].view(np.uint32) == 0), (r, h)
    assert np.count_nonzero(out) > 0


def test_both_walks_see_the_same_mask(pkg, graphs_, monkeypatch):
    """el = er = 0 makes every weight of row r 1 / deg(r) > 0. The transposed aggregate of a one-hot grad_out (row r) is then non-zero
    in exactly the columns whose entry (r, c) the forward kept, and the forward on one-hot features of column c in exactly the rows."""
    from gespmm_amd import softmax

    monkeypatch.delenv(PIN, raising=False)
    G, H, p, pair = graphs_["short"], 3, 0.6, SEEDS[0]
    M, K = G["M"], G["K"]
    el, er = torch.zeros(M, H, device="cuda"), torch.zeros(K, H, device="cuda")
    c = {"el": el, "er": er, "stats": softmax.gat_softmax_stats(G["rp"], G["ci"], el, er)}
    keep = _keep(G, pair, p, H)
    kept = np.zeros((M, K, H), dtype=bool)  # (duplicate (r, c) entries share their decision: `or` loses nothing)
    np.logical_or.at(kept, (G["rows_h"], G["colind"]), keep)
    rows = [int(r) for r in np.argsort(-np.diff(G["rowptr"]))[:3]] + [0, 1]
    for r in rows:
        gout = torch.zeros(M, H, 1, device="cuda")
        gout[r] = 1.0
        back = _aggregate(G, c, gout, None, True, (p, _seed(pair))).cpu().numpy()[:, :, 0]  # [K, H]
        assert np.array_equal(back != 0, kept[r]), r
    for col in (0, 7, K - 1):
        feat = torch.zeros(K, H, 1, device="cuda")
        feat[col] = 1.0
        fwd = _aggregate(G, c, feat, None, False, (p, _seed(pair))).cpu().numpy()[:, :, 0]  # [M, H]
        assert np.array_equal(fwd != 0, kept[:, col]), col


# --------------------------------------------------------------------------------------------------------------------- 3. backward

def _fused(G, c, gout, feat, slope, drop):
    from gespmm_amd import softmax

    H = c["el"].shape[1]
    (bd, delta), (bl, gel), (br, ger) = _out((G["M"], H)), _out((G["M"], H)), _out((G["K"], H))
    softmax.gat_backward_el(G["rp"], G["ci"], c["el"], c["er"], c["stats"], gout, feat, negative_slope=slope, out=(delta, gel), dropout=drop)
    softmax.gat_backward_er(G["cp"], G["ri"], c["el"], c["er"], c["stats"], delta, gout, feat, negative_slope=slope, out=ger, dropout=drop)
    for buf, what in zip((bd, bl, br), ("delta", "grad_el", "grad_er")):
        _guard_ok(buf, what)
    return delta, gel, ger


def _composition(G, c, gout, feat, slope, p, pair):
    """The five steps -> (alpha, g', grad_el, grad_er)."""
    from gespmm_amd import sddmm, softmax

    leaky = slope is not None
    alpha = softmax.gat_edge_softmax(G["rp"], G["ci"], c["el"], c["er"], negative_slope=slope)
    g = _dropped(G, sddmm.csr_sddmm_heads(G["rp"], G["ci"], gout, feat), p, pair)
    gs, gel = softmax.gat_edge_softmax_backward(G["rp"], G["ci"], alpha, g, el=c["el"] if leaky else None, er=c["er"] if leaky else None,
                                                negative_slope=slope)
    return alpha, g, gel, softmax.edge_segment_sum(G["cp"], gs, order=G["order"])


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,F", HF + ((33, 2),))
def test_backward_equals_the_composition_where_the_dot_is_exact(pkg, graphs_, H, F, slope):
    from test_gpu_gat_backward import _check_delta_where_exact

    p = 0.6  # s = 1 / (1 - 0.6f) is inexact: g' = fl(g s) is one rounding in the kernel and in edge_dropout
    compared = 0
    for i, name in enumerate(ALL):
        G = graphs_[name]
        c = _case(G, H, slope)
        pair = SEEDS[i % 2]
        gout, feat = _ints(G["M"], H, F, 100 + H * F), _ints(G["K"], H, F, 200 + H * F)
        delta, gel, ger = _fused(G, c, gout, feat, slope, (p, _seed(pair)))
        alpha, g, want_el, want_er = _composition(G, c, gout, feat, slope, p, pair)
        what = "%s H=%d F=%d slope=%s" % (name, H, F, slope)
        assert not bool(torch.isnan(torch.cat((delta.view(-1), gel.view(-1), ger.view(-1)))).any()), what + ": every word must be written"
        _same(gel, want_el, what + ": grad_el")
        _same(ger, want_er, what + ": grad_er")
        compared += _check_delta_where_exact(G, delta, alpha, g, what)
        base = _fused(G, c, gout, feat, slope, None)
        for w, u, v in zip(("delta", "grad_el", "grad_er"), _fused(G, c, gout, feat, slope, (0.0, _seed(pair))), base):
            _same(u, v, what + ": p = 0 is the base call, " + w)
    assert compared > 0, "no (row, head) pair had exact products: delta was compared nowhere"


@pytest.mark.parametrize("H,F", ((4, 2), (8, 8), (1, 64), (3, 5)))
def test_backward_against_float64(pkg, graphs_, H, F):
    """The new kernels AND the composition, each inside 1e-4 max(|ref|, scale) of float64 with the numpy mask."""
    worst_all = 0.0
    for name in ("edge", "padded", "short_t"):
        G = graphs_[name]
        for slope in SLOPES:
            for p, pair in zip(PS, SEEDS):
                c = _case(G, H, slope)
                gout, feat = _reals(G["M"], H, F, 900 + H + F), _reals(G["K"], H, F, 901 + H + F)
                ref_el, ref_er, sc_el, sc_er = gat_backward_float64(G["rows_h"], G["colind"], G["M"], G["K"], c["el"].cpu().numpy(),
                                                                    c["er"].cpu().numpy(), gout.cpu().numpy(), feat.cpu().numpy(), slope,
                                                                    _keep(G, pair, p, H), _scale(p))
                _, gel, ger = _fused(G, c, gout, feat, slope, (p, _seed(pair)))
                _, _, cel, cer = _composition(G, c, gout, feat, slope, p, pair)
                for what, got, ref, scale in (("kernel grad_el", gel, ref_el, sc_el), ("kernel grad_er", ger, ref_er, sc_er),
                                              ("composition grad_el", cel, ref_el, sc_el), ("composition grad_er", cer, ref_er, sc_er)):
                    bound = 1e-4 * np.maximum(np.abs(ref), scale)
                    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
                    worst_all = max(worst_all, worst)
                    assert np.all(err <= bound), (name, what, H, F, slope, p, worst)
    print("H=%d F=%d: worst error / bound %.4f" % (H, F, worst_all))


# ---------------------------------------------------------------------------------------------------------------------- 4. capture

def test_capture_equals_eager_and_the_seed_is_read_at_replay(pkg, graphs_, monkeypatch):
    """stats, the aggregate in both walks and both backward launches captured together; a replay after ``seed.copy_(other)`` has the
    eager bits of ``other``: the seed is device memory the kernels load, not a value baked into the launch."""
    from gespmm_amd import softmax, spmm

    monkeypatch.delenv(PIN, raising=False)
    G, H, F, p = graphs_["edge"], 8, 8, 0.6
    el, er, _ = _terms(G, H, 31)
    feat, gout = _reals(G["K"], H, F, 1), _reals(G["M"], H, F, 2)
    seed = _seed(SEEDS[0])
    shapes = {"stats": (G["M"], H, 2), "out": (G["M"], H, F), "out_t": (G["K"], H, F), "delta": (G["M"], H), "gel": (G["M"], H),
              "ger": (G["K"], H)}
    bufs = {k: _out(s) for k, s in shapes.items()}
    t = {k: v[1] for k, v in bufs.items()}

    def step():
        softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2, out=t["stats"])
        spmm.gat_aggregate(G["rp"], G["ci"], el, er, t["stats"], feat, negative_slope=0.2, out=t["out"], dropout=(p, seed))
        spmm.gat_aggregate(G["cp"], G["ri"], el, er, t["stats"], gout, negative_slope=0.2, transposed=True, out=t["out_t"], dropout=(p, seed))
        softmax.gat_backward_el(G["rp"], G["ci"], el, er, t["stats"], gout, feat, negative_slope=0.2, out=(t["delta"], t["gel"]),
                                dropout=(p, seed))
        softmax.gat_backward_er(G["cp"], G["ri"], el, er, t["stats"], t["delta"], gout, feat, negative_slope=0.2, out=t["ger"],
                                dropout=(p, seed))

    graph, _ = _capture(step)
    seen = []
    for pair in (SEEDS[0], SEEDS[1]):
        seed.copy_(_seed(pair))
        for b, _t in bufs.values():
            b.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for k, (b, _t) in bufs.items():
            _guard_ok(b, "replay " + k)
        c = {"el": el, "er": er, "stats": softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2)}
        drop = (p, _seed(pair))
        want = {"out": _aggregate(G, c, feat, 0.2, False, drop), "out_t": _aggregate(G, c, gout, 0.2, True, drop)}
        want["delta"], want["gel"], want["ger"] = _fused(G, c, gout, feat, 0.2, drop)
        for k, v in want.items():
            _same(t[k], v, "replayed %s vs eager, seed %r" % (k, pair))
        seen.append(t["out"].clone())
    assert not torch.equal(seen[0], seen[1]), "the two seeds must give different masks"


# ------------------------------------------------------------------------------------------------- 5. repeatability, no entries, errors

def test_two_calls_give_the_same_bits(pkg, graphs_, monkeypatch):
    monkeypatch.delenv(PIN, raising=False)
    for name in ("hubs", "short_t"):
        G = graphs_[name]
        c = _case(G, 8, 0.2)
        gout, feat = _reals(G["M"], 8, 16, 3), _reals(G["K"], 8, 16, 4)
        drop = (0.6, _seed(SEEDS[1]))
        first = _fused(G, c, gout, feat, 0.2, drop) + (_aggregate(G, c, feat, 0.2, False, drop), _aggregate(G, c, gout, 0.2, True, drop))
        again = _fused(G, c, gout, feat, 0.2, drop) + (_aggregate(G, c, feat, 0.2, False, drop), _aggregate(G, c, gout, 0.2, True, drop))
        for what, u, v in zip(("delta", "grad_el", "grad_er", "out", "out_t"), again, first):
            _same(u, v, "%s: second run, %s" % (name, what))


def test_no_entries(pkg):
    from gespmm_amd import softmax

    M, K, H, F = 7, 5, 3, 4
    rp0, cp0 = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    i0 = torch.empty(0, dtype=torch.int32, device="cuda")
    G = {"rp": rp0, "ci": i0, "cp": cp0, "ri": i0, "M": M, "K": K}
    c = {"el": torch.ones(M, H, device="cuda"), "er": torch.ones(K, H, device="cuda"), "stats": torch.zeros(M, H, 2, device="cuda")}
    drop = (0.6, _seed(SEEDS[0]))
    gout, feat = torch.ones(M, H, F, device="cuda"), torch.ones(K, H, F, device="cuda")
    for out in _fused(G, c, gout, feat, 0.2, drop) + (_aggregate(G, c, feat, 0.2, False, drop), _aggregate(G, c, gout, 0.2, True, drop)):
        assert bool((out.view(torch.int32) == 0).all())
    assert softmax.edge_dropout(rp0, i0, torch.empty(0, H, device="cuda"), 0.6, drop[1]).shape == (0, H)


def test_python_errors_raise_without_launching(pkg, graphs_):
    from gespmm_amd import softmax, spmm

    G, H, F = graphs_["edge"], 4, 2
    rp, ci, cp, ri, M, K, nnz = G["rp"], G["ci"], G["cp"], G["ri"], G["M"], G["K"], G["nnz"]
    c = _case(G, H, 0.2)
    el, er, st = c["el"], c["er"], c["stats"]
    gout, feat = _reals(M, H, F, 1), _reals(K, H, F, 2)
    seed = _seed(SEEDS[0])
    x = _reals(nnz, H, 1, 5).view(nnz, H).contiguous()
    y = _dropped(G, x, 0.6, SEEDS[0])
    out = _aggregate(G, c, feat, 0.2, False, (0.6, seed))
    delta, gel, ger = _fused(G, c, gout, feat, 0.2, (0.6, seed))
    before = [t.clone() for t in (y, out, delta, gel, ger)]
    calls = {
        "drop": lambda p, s: softmax.edge_dropout(rp, ci, x, p, s, out=y),
        "agg": lambda p, s: spmm.gat_aggregate(rp, ci, el, er, st, feat, negative_slope=0.2, out=out, dropout=(p, s)),
        "el": lambda p, s: softmax.gat_backward_el(rp, ci, el, er, st, gout, feat, negative_slope=0.2, out=(delta, gel), dropout=(p, s)),
        "er": lambda p, s: softmax.gat_backward_er(cp, ri, el, er, st, delta, gout, feat, negative_slope=0.2, out=ger, dropout=(p, s)),
    }
    for name, call in calls.items():
        for s in (seed.long(), seed.float(), seed.cpu().numpy(), None):
            with pytest.raises(TypeError):
                call(0.6, s)
        with pytest.raises(TypeError):
            call(torch.tensor(0.6, device="cuda"), seed)
        for s in (seed.cpu(), torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(2, 1, dtype=torch.int32, device="cuda"),
                  torch.zeros(4, dtype=torch.int32, device="cuda")[::2]):
            with pytest.raises(ValueError):
                call(0.6, s)
        for p in (-0.1, 1.0, float("nan")):
            with pytest.raises(ValueError):
                call(p, seed)
    with pytest.raises(ValueError):
        softmax.edge_dropout(rp, ci[:-1].contiguous(), x, 0.6, seed)
    with pytest.raises(ValueError):
        softmax.edge_dropout(rp, ci, x, 0.6, seed, out=torch.empty(nnz, H + 1, device="cuda"))
    with pytest.raises(TypeError):
        softmax.edge_dropout(rp, ci, x.double(), 0.6, seed)
    torch.cuda.synchronize()
    for t, b in zip((y, out, delta, gel, ger), before):
        _same(t, b, "untouched")
