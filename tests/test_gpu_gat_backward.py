"""Fused GAT backward for el / er on the GPU (softmax.gat_backward_el / gat_backward_er): grad_el and grad_er with no edge array.

The composition it replaces — ``gat_edge_softmax``, ``csr_sddmm_heads``, ``gat_edge_softmax_backward``, ``edge_segment_sum(colptr, ..,
order)`` — is the oracle for every bit wherever the dot product g is exact (integer-valued operands, or F = 1), and a float64
restatement on the host checks BOTH inside the project's bound on random real operands. Patterns, their asserted lane widths and the
terms are those of tests/test_gpu_gat_softmax.py, plus the transpose of its ``short`` pattern, whose COLUMNS reach the three regimes;
every result is written into a NaN-prefilled tensor with guard words behind it."""
import numpy as np
import pytest
import torch

from attention_refs import gat_backward_float64
from test_edge_softmax_host import IT, WANT_L, want_W
from test_gat_softmax_host import csc_of
from test_gpu_edge_softmax import NAN, _dev, _guard_ok, _out, _same
from test_gpu_gat_softmax import PATTERNS, SLOPES, _pattern, _terms, patterns  # noqa: F401  (patterns: the module's fixture, W asserted there)
from test_gpu_heads import _carve
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

HF = ((1, 1), (1, 8), (1, 64), (2, 2), (3, 5), (4, 16), (8, 8), (7, 27), (8, 64), (33, 2))
ALL = PATTERNS + ("short_t",)


def _regimes(ptr, W):
    """Which of the three regimes the segments of ``ptr`` ask for at lane width W, from the degrees alone."""
    d = np.diff(ptr)
    return {"register": bool(((d > 0) & (d <= IT * W)).any()), "sweep": bool(((d > IT * W) & (d <= WANT_L)).any()),
            "hub": bool((d > WANT_L).any())}


@pytest.fixture(scope="module")
def graphs_(patterns):  # noqa: F811
    """The five patterns and the transpose of ``short`` with their CSC arrays (csc_of on the host) on the device, and a cache of what
    several tests need of a (pattern, H, slope): the terms and the statistics — computed once, never edited."""
    from gespmm_amd import _lib

    out = {}
    for name in ALL:
        if name == "short_t":  # K = 50 rows of ~200 entries; 3007 columns: 0 .. 3 entries, L - 1, L, and one of L + 1
            S = _pattern("short")
            colptr_h, order_h = csc_of(S["rowptr"], S["colind"], S["K"])
            rows_h = np.repeat(np.arange(S["M"], dtype=np.int32), np.diff(S["rowptr"]))
            G = {"rowptr": colptr_h, "colind": rows_h[order_h], "M": S["K"], "K": S["M"], "nnz": S["nnz"]}
            G["W"] = want_W(G["M"], G["nnz"])
            assert _lib.describe_edge_softmax(G["M"], G["nnz"], 8) == {"W": G["W"], "L": WANT_L}
            G["rp"], G["ci"] = _dev(G["rowptr"]), _dev(G["colind"])
            G["rows"] = torch.repeat_interleave(torch.arange(G["M"], device="cuda"), torch.diff(G["rp"]).long())
        else:
            G = dict(patterns[name])
        assert G["M"] != G["K"] or name == "mean8", "swapped roles of the two indices must show"
        colptr_h, order_h = csc_of(G["rowptr"], G["colind"], G["K"])
        rows_h = np.repeat(np.arange(G["M"], dtype=np.int32), np.diff(G["rowptr"]))
        G["rows_h"], G["colptr_h"], G["order_h"] = rows_h, colptr_h, order_h
        G["cp"], G["ri"], G["order"] = _dev(colptr_h), _dev(rows_h[order_h]), _dev(order_h)
        G["Wc"] = want_W(G["K"], G["nnz"])
        assert _lib.describe_edge_softmax(G["K"], G["nnz"], 8) == {"W": G["Wc"], "L": WANT_L}, name
        G["cache"] = {}
        out[name] = G
    # every regime of the kernel is reached by rows (first pass) and by columns (second pass)
    rows = [_regimes(out[n]["rowptr"], out[n]["W"]) for n in ALL]
    cols = [_regimes(out[n]["colptr_h"], out[n]["Wc"]) for n in ALL]
    for regime in ("register", "sweep", "hub"):
        assert any(r[regime] for r in rows), "no row in the %s regime" % regime
        assert any(c[regime] for c in cols), "no column in the %s regime" % regime
    assert _regimes(out["short_t"]["colptr_h"], out["short_t"]["Wc"]) == {"register": True, "sweep": True, "hub": True}
    return out


def _case(G, H, slope):
    from gespmm_amd import softmax

    key = (H, slope)
    if key not in G["cache"]:
        el, er, _ = _terms(G, H, 3000 + 7 * H + G["nnz"] % 13)
        G["cache"][key] = {"el": el, "er": er, "stats": softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=slope)}
    return G["cache"][key]


def _ints(rows, H, F, seed):
    """Integer values in [-4, 4]: every partial sum of a dot product of them is exact in fp32, in any order."""
    rng = np.random.RandomState(seed)
    return _dev(rng.randint(-4, 5, size=(rows, H, F)).astype(np.float32))


def _reals(rows, H, F, seed):
    rng = np.random.RandomState(seed)
    return _dev((rng.rand(rows, H, F) - 0.5).astype(np.float32))  # within +-0.5


def _fused(G, c, gout, feat, slope, align=16, need_er=True):
    """Both launches into NaN-prefilled, guarded tensors whose addresses `align` divides -> (delta, grad_el, grad_er)."""
    from gespmm_amd import softmax

    H = c["el"].shape[1]
    bufs, outs = [], []
    for rows in (G["M"], G["M"], G["K"]):
        buf, out = _out((rows, H))
        if align != 16:
            out = _carve(out, align)
            out.fill_(NAN)
        bufs.append(buf)
        outs.append(out)
    delta, gel, ger = outs
    r = softmax.gat_backward_el(G["rp"], G["ci"], c["el"], c["er"], c["stats"], gout, feat, negative_slope=slope, out=(delta, gel))
    assert r[0] is delta and r[1] is gel
    r = softmax.gat_backward_er(G["cp"], G["ri"], c["el"], c["er"], c["stats"], delta, gout, feat, negative_slope=slope, out=ger)
    assert r is ger
    if align == 16:
        for buf, what in zip(bufs, ("delta", "grad_el", "grad_er")):
            _guard_ok(buf, what)
    return delta, gel, ger


def _composition(G, c, slope, grad_alpha=None, gout=None, feat=None):
    """Today's four steps -> (alpha, grad_alpha, grad_el, grad_er)."""
    from gespmm_amd import sddmm, softmax

    leaky = slope is not None
    alpha = softmax.gat_edge_softmax(G["rp"], G["ci"], c["el"], c["er"], negative_slope=slope)
    if grad_alpha is None:
        grad_alpha = sddmm.csr_sddmm_heads(G["rp"], G["ci"], gout, feat)
    gs, gel = softmax.gat_edge_softmax_backward(G["rp"], G["ci"], alpha, grad_alpha, el=c["el"] if leaky else None,
                                                er=c["er"] if leaky else None, negative_slope=slope)
    ger = softmax.edge_segment_sum(G["cp"], gs, order=G["order"])
    return alpha, grad_alpha, gel, ger


def _check_delta_where_exact(G, delta, alpha, grad_alpha, what):
    """delta is the fmaf chain of alpha * grad_alpha; edge_segment_sum adds the ROUNDED products in the same order. The two agree
    bit for bit in the (row, head) pairs all of whose products are exact, and those are compared. -> pairs compared"""
    from gespmm_amd import softmax

    prod = alpha * grad_alpha
    exact = (prod.double() == alpha.double() * grad_alpha.double()).to(torch.float32)
    all_exact = softmax.edge_segment_sum(G["rp"], 1.0 - exact) == 0  # (sums of zeros and ones)
    want = softmax.edge_segment_sum(G["rp"], prod)
    bad = int(((delta.view(torch.int32) != want.view(torch.int32)) & all_exact).sum())
    assert bad == 0, "%s: delta differs in %d pairs whose products are exact" % (what, bad)
    return int(all_exact.sum())


# --------------------------------------------------------------------------------------------------- 1. the bits of the composition

@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,F", HF)
def test_equals_the_composition_where_the_dot_is_exact(pkg, graphs_, H, F, slope):
    compared = 0
    for name in ALL:
        G = graphs_[name]
        c = _case(G, H, slope)
        gout, feat = _ints(G["M"], H, F, 100 + H * F), _ints(G["K"], H, F, 200 + H * F)
        delta, gel, ger = _fused(G, c, gout, feat, slope)
        alpha, ga, want_el, want_er = _composition(G, c, slope, gout=gout, feat=feat)
        what = "%s H=%d F=%d slope=%s" % (name, H, F, slope)
        assert not bool(torch.isnan(torch.cat((delta.view(-1), gel.view(-1), ger.view(-1)))).any()), what + ": every word must be written"
        _same(gel, want_el, what + ": grad_el")
        _same(ger, want_er, what + ": grad_er")
        compared += _check_delta_where_exact(G, delta, alpha, ga, what)
        empty_r, empty_c = np.diff(G["rowptr"]) == 0, np.diff(G["colptr_h"]) == 0
        assert np.all(delta.cpu().numpy()[empty_r].view(np.uint32) == 0) and np.all(gel.cpu().numpy()[empty_r].view(np.uint32) == 0)
        assert np.all(ger.cpu().numpy()[empty_c].view(np.uint32) == 0), what + ": empty columns are +0"
    assert compared > 0, "no (row, head) pair had exact products: delta was compared nowhere"


# ------------------------------------------------------------------------------------------------------------------ 2. the g chain

@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", (1, 3, 8))
def test_one_rounded_product_at_width_one(pkg, graphs_, H, slope):
    """F = 1, random real operands: g is fl(grad_out * feat), which torch computes with the same single rounding."""
    for name in ALL:
        G = graphs_[name]
        c = _case(G, H, slope)
        gout, feat = _reals(G["M"], H, 1, 11) * 8, _reals(G["K"], H, 1, 12) * 8
        ga = (gout[G["rows"]] * feat[G["ci"].long()]).view(G["nnz"], H)
        delta, gel, ger = _fused(G, c, gout, feat, slope)
        alpha, _, want_el, want_er = _composition(G, c, slope, grad_alpha=ga.contiguous())
        what = "%s H=%d slope=%s" % (name, H, slope)
        _same(gel, want_el, what + ": grad_el")
        _same(ger, want_er, what + ": grad_er")
        _check_delta_where_exact(G, delta, alpha, ga, what)


# ------------------------------------------------------------------------------------------------------------------ 3. accuracy

@pytest.mark.parametrize("H,F", ((4, 2), (8, 8), (1, 64), (3, 5)))
def test_against_float64(pkg, graphs_, H, F):
    """The new kernels AND the composition, each inside 1e-4 max(|ref|, scale) of float64."""
    for name in ("edge", "padded", "short_t"):
        G = graphs_[name]
        for slope in SLOPES:
            c = _case(G, H, slope)
            gout, feat = _reals(G["M"], H, F, 900 + H + F), _reals(G["K"], H, F, 901 + H + F)
            ref_el, ref_er, sc_el, sc_er = gat_backward_float64(G["rows_h"], G["colind"], G["M"], G["K"], c["el"].cpu().numpy(),
                                                                c["er"].cpu().numpy(), gout.cpu().numpy(), feat.cpu().numpy(), slope)
            _, gel, ger = _fused(G, c, gout, feat, slope)
            _, _, cel, cer = _composition(G, c, slope, gout=gout, feat=feat)
            for what, got, ref, scale in (("kernel grad_el", gel, ref_el, sc_el), ("kernel grad_er", ger, ref_er, sc_er),
                                          ("composition grad_el", cel, ref_el, sc_el), ("composition grad_er", cer, ref_er, sc_er)):
                bound = 1e-4 * np.maximum(np.abs(ref), scale)
                err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                worst = float((err / np.where(bound > 0, bound, 1.0)).max())
                print("%s %s H=%d F=%d slope=%s: worst error / bound %.4f" % (name, what, H, F, slope, worst))
                assert np.all(err <= bound), (name, what, H, F, slope, worst)


# -------------------------------------------------------------------------------------------------- 4. misalignment and odd widths

@pytest.mark.parametrize("F", (5, 8, 27))
def test_alignment_changes_no_bit(pkg, graphs_, F):
    H = 3
    for name in ("edge", "short_t"):
        G = graphs_[name]
        c = _case(G, H, 0.2)
        gout, feat = _reals(G["M"], H, F, 41), _reals(G["K"], H, F, 42)
        want = _fused(G, c, gout, feat, 0.2)
        for align in (8, 4):
            got = _fused(G, c, _carve(gout, align), _carve(feat, align), 0.2, align=align)
            for what, u, v in zip(("delta", "grad_el", "grad_er"), got, want):
                _same(u, v, "%s F=%d align=%d: %s" % (name, F, align, what))
        for a_out, a_feat in ((16, 8), (4, 16)):  # one operand off the boundary is enough for the narrow loads
            got = _fused(G, c, _carve(gout, a_out), _carve(feat, a_feat), 0.2)
            for what, u, v in zip(("delta", "grad_el", "grad_er"), got, want):
                _same(u, v, "%s F=%d align=(%d, %d): %s" % (name, F, a_out, a_feat, what))


# ------------------------------------------------------------------------------------------------------------------- 5. bad inputs

@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_bad_el_poisons_what_it_poisons_in_the_composition(pkg, graphs_, bad):
    from gespmm_amd import softmax

    H, F = 8, 8
    for name, row in (("edge", 3), ("short", 4)):  # a swept row at W = 16, a hub row at W = 4
        G = graphs_[name]
        el, er, _ = _terms(G, H, 77)
        el[row, 2] = bad
        gout, feat = _ints(G["M"], H, F, 5), _ints(G["K"], H, F, 6)
        for slope in SLOPES:
            c = {"el": el, "er": er, "stats": softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=slope)}
            _, gel, ger = _fused(G, c, gout, feat, slope)
            _, _, want_el, want_er = _composition(G, c, slope, gout=gout, feat=feat)
            for what, got, want in (("grad_el", gel, want_el), ("grad_er", ger, want_er)):
                nan_g, nan_w = torch.isnan(got), torch.isnan(want)
                assert bool(nan_w.any()) and not bool(nan_w.all()) and torch.equal(nan_g, nan_w), (name, slope, what)
                _same(torch.where(nan_g, torch.zeros_like(got), got), torch.where(nan_w, torch.zeros_like(want), want), (name, slope, what))


# ---------------------------------------------------------------------------------------------------------------------- 6. capture

def test_capture_equals_eager(pkg, graphs_):
    """Both launches captured together on a side stream; replays see operands edited in place and give the eager bits."""
    from gespmm_amd import softmax

    G, H, F = graphs_["edge"], 8, 8
    el, er, _ = _terms(G, H, 31)
    gout, feat = _reals(G["M"], H, F, 1), _reals(G["K"], H, F, 2)
    buf_s, stats = _out((G["M"], H, 2))
    buf_d, delta = _out((G["M"], H))
    buf_l, gel = _out((G["M"], H))
    buf_r, ger = _out((G["K"], H))

    def step():
        softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2, out=stats)
        softmax.gat_backward_el(G["rp"], G["ci"], el, er, stats, gout, feat, negative_slope=0.2, out=(delta, gel))
        softmax.gat_backward_er(G["cp"], G["ri"], el, er, stats, delta, gout, feat, negative_slope=0.2, out=ger)

    graph, _ = _capture(step)
    for seed in (33, 35):
        el2, er2, _ = _terms(G, H, seed)
        el.copy_(el2)
        er.copy_(er2)
        gout.copy_(_reals(G["M"], H, F, seed))
        for b in (buf_s, buf_d, buf_l, buf_r):
            b.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for b in (buf_s, buf_d, buf_l, buf_r):
            _guard_ok(b, "replay")
        c = {"el": el, "er": er, "stats": softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2)}
        want = _fused(G, c, gout, feat, 0.2)
        for what, u, v in zip(("delta", "grad_el", "grad_er"), (delta, gel, ger), want):
            _same(u, v, "replayed %s vs eager" % what)


# ------------------------------------------------------------------------------------------------- 7. no entries, 8. repeatability

def test_no_entries(pkg):
    from gespmm_amd import softmax

    M, K, H, F = 7, 5, 3, 4
    rp0, cp0 = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    i0 = torch.empty(0, dtype=torch.int32, device="cuda")
    G = {"rp": rp0, "ci": i0, "cp": cp0, "ri": i0, "M": M, "K": K}
    c = {"el": torch.ones(M, H, device="cuda"), "er": torch.ones(K, H, device="cuda"), "stats": torch.zeros(M, H, 2, device="cuda")}
    for out in _fused(G, c, torch.ones(M, H, F, device="cuda"), torch.ones(K, H, F, device="cuda"), 0.2):
        assert bool((out.view(torch.int32) == 0).all())


def test_two_calls_give_the_same_bits(pkg, graphs_):
    for name in ("hubs", "short_t"):
        G = graphs_[name]
        c = _case(G, 8, 0.2)
        gout, feat = _reals(G["M"], 8, 16, 3), _reals(G["K"], 8, 16, 4)
        first = _fused(G, c, gout, feat, 0.2)
        for what, u, v in zip(("delta", "grad_el", "grad_er"), _fused(G, c, gout, feat, 0.2), first):
            _same(u, v, "%s: second run, %s" % (name, what))


def test_python_errors_raise_without_launching(pkg, graphs_):
    from gespmm_amd import softmax

    G, H, F = graphs_["edge"], 4, 2
    rp, ci, cp, ri, M, K, nnz = G["rp"], G["ci"], G["cp"], G["ri"], G["M"], G["K"], G["nnz"]
    c = _case(G, H, 0.2)
    el, er, st = c["el"], c["er"], c["stats"]
    gout, feat = _reals(M, H, F, 1), _reals(K, H, F, 2)
    delta, gel, ger = _fused(G, c, gout, feat, 0.2)
    before = [t.clone() for t in (delta, gel, ger)]
    bel = lambda *a, **kw: softmax.gat_backward_el(*a, **kw)  # noqa: E731
    ber = lambda *a, **kw: softmax.gat_backward_er(*a, **kw)  # noqa: E731
    new = lambda *shape, **kw: torch.empty(*shape, device="cuda", **kw)  # noqa: E731
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        for call in (lambda: bel(rp, ci, el.to(dt), er, st, gout, feat), lambda: bel(rp, ci, el, er.to(dt), st, gout, feat),
                     lambda: bel(rp, ci, el, er, st.to(dt), gout, feat), lambda: bel(rp, ci, el, er, st, gout.to(dt), feat),
                     lambda: bel(rp, ci, el, er, st, gout, feat.to(dt)),
                     lambda: bel(rp, ci, el, er, st, gout, feat, out=(new(M, H, dtype=dt), gel)),
                     lambda: bel(rp, ci, el, er, st, gout, feat, out=(delta, new(M, H, dtype=dt))),
                     lambda: ber(cp, ri, el.to(dt), er, st, delta, gout, feat), lambda: ber(cp, ri, el, er, st, delta.to(dt), gout, feat),
                     lambda: ber(cp, ri, el, er, st, delta, gout, feat.to(dt)),
                     lambda: ber(cp, ri, el, er, st, delta, gout, feat, out=new(K, H, dtype=dt))):
            with pytest.raises(TypeError):
                call()
    for call in (lambda: bel(rp.long(), ci, el, er, st, gout, feat), lambda: bel(rp, ci.long(), el, er, st, gout, feat),
                 lambda: ber(cp.long(), ri, el, er, st, delta, gout, feat), lambda: ber(cp, ri.long(), el, er, st, delta, gout, feat),
                 lambda: bel(rp, ci, el, er, st, gout, feat, out=delta), lambda: bel(rp, ci, el, er, st, gout.cpu().numpy(), feat)):
        with pytest.raises(TypeError):
            call()
    misaligned = torch.zeros(M * H * 2 + 1, device="cuda")[1:].view(M, H, 2)
    assert misaligned.data_ptr() % 8 == 4
    for call in (lambda: bel(rp, ci, el[:-1], er, st, gout, feat), lambda: bel(rp, ci, el, er[:, :-1].contiguous(), st, gout, feat),
                 lambda: bel(cp, ri, el, er, st, gout, feat),                    # colptr where rowptr is wanted: K + 1 entries
                 lambda: bel(rp, ci, el, er, st[:-1], gout, feat), lambda: bel(rp, ci, el, er, st.view(M, 2 * H), gout, feat),
                 lambda: bel(rp, ci, el, er, misaligned, gout, feat),            # stats holds 8-byte pairs
                 lambda: bel(rp, ci, el, er, new(M, H, 4)[:, :, ::2], gout, feat),
                 lambda: bel(rp, ci, el, er, st, feat, gout),                    # the two dense operands swapped: M and K rows
                 lambda: bel(rp, ci, el, er, st, gout.view(M, F, H), feat),      # H is not the second dimension
                 lambda: bel(rp, ci, el, er, st, gout, _reals(K, H, F + 1, 3)),  # the widths differ
                 lambda: bel(rp, ci, el, er, st, gout.view(M, H * F), feat.view(K, H * F)),
                 lambda: bel(rp, ci, el, er, st, new(M, H, 2 * F)[:, :, ::2], feat),
                 lambda: bel(rp, ci, el, er, st.cpu(), gout, feat), lambda: bel(rp, ci, el, er, st, gout.cpu(), feat),
                 lambda: bel(rp, ci, el, er, st, gout, feat.cpu()), lambda: bel(rp, ci.cpu(), el, er, st, gout, feat),
                 lambda: bel(rp.cpu(), ci, el, er, st, gout, feat), lambda: bel(rp, ci, el.cpu(), er, st, gout, feat),
                 lambda: bel(rp, ci, el, er, st, gout, feat, negative_slope=float("nan")),
                 lambda: bel(rp, ci, el, er, st, gout, feat, out=(new(M + 1, H), gel)),
                 lambda: bel(rp, ci, el, er, st, gout, feat, out=(delta, torch.empty(M, H))),
                 lambda: bel(rp, ci, el, er, st, gout, feat, out=(delta, new(M, 2 * H)[:, ::2])),
                 lambda: ber(rp, ci, el, er, st, delta, gout, feat),             # rowptr where colptr is wanted
                 lambda: ber(cp, ri, el, er, st, delta[:-1], gout, feat), lambda: ber(cp, ri, el, er, st, delta.cpu(), gout, feat),
                 lambda: ber(cp, ri, el, er, misaligned, delta, gout, feat), lambda: ber(cp, ri, el, er, st, delta, feat, gout),
                 lambda: ber(cp, ri, el, er, st, delta, gout, _reals(K, H, F + 1, 3)),
                 lambda: ber(cp, ri.cpu(), el, er, st, delta, gout, feat),
                 lambda: ber(cp, ri, el, er, st, delta, gout, feat, negative_slope=float("inf")),
                 lambda: ber(cp, ri, el, er, st, delta, gout, feat, out=new(K + 1, H)),
                 lambda: ber(cp, ri, el, er, st, delta, gout, feat, out=torch.empty(K, H))):
        with pytest.raises(ValueError):
            call()
    # nothing was launched: the results of the call before are what they were
    for t, b in zip((delta, gel, ger), before):
        _same(t, b, "untouched")
