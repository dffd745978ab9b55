"""The GATv2 edge score on the GPU (sddmm.gatv2_score / gatv2_score_backward): both kernels against the numpy / float64 restatement of
tests/test_gatv2_host.py on the five patterns of tests/test_gpu_gat_softmax.py plus the transpose of its ``short`` pattern — empty
rows, hub rows and hub columns — at every (V, W) the forward resolver answers (ASSERTED through gespmm_describe_gatv2_score) and every
vector / strip case of the backward. Results go through ``out=`` into NaN-prefilled tensors with 64 guard words behind them.

What the bit tests see and what they do not: on integer-valued operands every product and every partial sum is a multiple of 2^-2
below 2^22, so EVERY summation order gives the same fp32 word — these tests pin the values, the addressing, the clamping and the
stores, not the order. The chain orders (forward: one fmaf chain per lane over j = l V + i + t W V, then the xor butterfly; backward:
one fmaf chain per output word in segment order) are pinned by csrc/gatv2_score.h, as DESIGN 3.18 does for the fused backward; the
real-operand tests hold them to 1e-4 max(|ref|, sum |terms|) only."""
import numpy as np
import pytest
import torch

from attention_refs import gatv2_float64
from test_edge_softmax_host import WANT_L
from test_gat_softmax_host import csc_of
from test_gatv2_host import worst_ratio
from test_gpu_edge_softmax import NAN, _dev, _guard_ok, _out, _same
from test_gpu_gat_softmax import PATTERNS, _pattern
from test_gpu_heads import _carve
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

ALL = PATTERNS + ("short_t",)
SLOPES = (None, 0.25)
# (H, F) -> (V, W) of the forward on 16-byte aligned operands. Forward: every V in {1, 2, 4} at every W in {4 .. 64}, one vector per
# lane (F <= W V) and several, past resolve_sddmm's per-lane share at W = 64 ((1, 1028): 5 vectors, (2, 130): 3 at V = 2).
# Backward (V, W, strips) at N = H F: V = 1 at W = 4 (1, 1), 8 (2, 3), 16 (3, 5), 32 (1, 27), 64 in 2 strips, the last partial (33, 2),
# 5 strips (2, 130); V = 4 at W = 4 (1, 8), 8 (4, 8), 16 (8, 8), 32 (1, 128), 64 (8, 32), 2 strips (1, 512), 5 with a partial one (1, 1028).
HF = {(1, 1): (1, 4), (3, 5): (1, 4), (8, 8): (4, 4), (4, 16): (4, 4), (1, 64): (4, 8), (2, 130): (2, 32), (33, 2): (2, 4), (8, 32): (4, 4),
      (1, 33): (1, 8), (1, 65): (1, 16), (1, 129): (1, 32), (1, 257): (1, 64), (2, 34): (2, 8), (1, 66): (2, 16), (1, 258): (2, 64),
      (1, 128): (4, 16), (1, 256): (4, 32), (1, 512): (4, 64), (1, 1028): (4, 64), (2, 3): (1, 4), (1, 27): (1, 4), (1, 8): (4, 4),
      (4, 8): (4, 4)}
BWD = {(1, 1): (1, 4, 1), (2, 3): (1, 8, 1), (3, 5): (1, 16, 1), (1, 27): (1, 32, 1), (33, 2): (1, 64, 2), (2, 130): (1, 64, 5),
       (1, 8): (4, 4, 1), (4, 8): (4, 8, 1), (8, 8): (4, 16, 1), (1, 128): (4, 32, 1), (8, 32): (4, 64, 1), (1, 512): (4, 64, 2),
       (1, 1028): (4, 64, 5)}
REAL_HF = ((3, 5), (8, 8), (2, 130), (33, 2), (8, 32), (1, 257), (1, 1028))
RATIOS = {}


def _bwd_shape(H, F, vec4=None):
    """(V, W, strips) of the backward launch for 16-byte aligned operands: the rule of csrc/gatv2_score.hip, restated."""
    V = 4 if (F % 4 == 0 if vec4 is None else vec4) else 1
    need, W = H * F // V, 4
    while W < 64 and W < need:
        W *= 2
    return V, W, -(-H * F // (W * V))


@pytest.fixture(scope="module")
def graphs_(pkg):
    """The six patterns with their CSC arrays on the device, and a cache of operands and float64 references per (H, F, slope, kind):
    computed once, never edited."""
    from gespmm_amd import _lib

    out = {}
    for name in ALL:
        if name == "short_t":  # K = 50 rows of ~200 entries; 3007 columns: 0 .. 3 entries, L - 1, L, and one of L + 1
            S = _pattern("short")
            colptr_h, order_h = csc_of(S["rowptr"], S["colind"], S["K"])
            rows_h = np.repeat(np.arange(S["M"], dtype=np.int32), np.diff(S["rowptr"]))
            G = {"rowptr": colptr_h, "colind": rows_h[order_h], "M": S["K"], "K": S["M"], "nnz": S["nnz"]}
        else:
            G = dict(_pattern(name))
        colptr_h, order_h = csc_of(G["rowptr"], G["colind"], G["K"])
        rows_h = np.repeat(np.arange(G["M"], dtype=np.int32), np.diff(G["rowptr"]))
        G["rows_h"], G["colptr_h"], G["order_h"], G["rowind_h"] = rows_h, colptr_h, order_h, rows_h[order_h]
        G["rp"], G["ci"] = _dev(G["rowptr"]), _dev(G["colind"])
        G["cp"], G["ri"], G["order"] = _dev(colptr_h), _dev(G["rowind_h"]), _dev(order_h)
        G["cache"] = {}
        out[name] = G
    # the forward's launch shape for every (H, F), and the backward's table against its restated rule
    for (H, F), vw in HF.items():
        for G in out.values():
            d = _lib.describe_gatv2_score(G["M"], G["nnz"], H, F)
            assert (d["V"], d["W"]) == vw, ((H, F), d)
    assert {v for v in HF.values()} == {(V, W) for V in (1, 2, 4) for W in (4, 8, 16, 32, 64)}, "every (V, W) of the forward"
    for hf, want in BWD.items():
        assert hf in HF and _bwd_shape(*hf) == want, (hf, _bwd_shape(*hf))
    assert {w[:2] for w in BWD.values()} == {(V, W) for V in (1, 4) for W in (4, 8, 16, 32, 64)}, "every (V, W) of the backward"
    # empty rows and columns; the backward has ONE path for every segment length — a lane group walks the whole segment W entries at a
    # time — and it is reached at its longest, a hub segment past the softmax's long-row threshold, by rows AND by columns; segments that
    # are no multiple of any W and wavefronts whose groups have different lengths are everywhere
    rdeg = np.concatenate([np.diff(G["rowptr"]) for G in out.values()])
    cdeg = np.concatenate([np.diff(G["colptr_h"]) for G in out.values()])
    for deg in (rdeg, cdeg):
        assert (deg == 0).any() and (deg == 1).any() and deg.max() > WANT_L and (deg % 64 != 0).any()
    assert np.diff(out["hubs"]["rowptr"]).max() == 6151 and np.diff(out["short_t"]["colptr_h"]).max() == WANT_L + 1
    return out


def _ints(shape, lo, hi, seed):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float32)


def _operands(G, H, F, kind):
    """Host operands: 'int' — xl, xr in [-4, 4], att and grad_score in [-2, 2], all integers; 'real' — uniform in +-1 (att, grad_score: +-2)."""
    key = (H, F, kind)
    if key not in G["cache"]:
        seed = 100 * H + F + G["nnz"] % 17
        if kind == "int":
            o = {"xl": _ints((G["M"], H, F), -4, 4, seed), "xr": _ints((G["K"], H, F), -4, 4, seed + 1), "att": _ints((H, F), -2, 2, seed + 2),
                 "gs": _ints((G["nnz"], H), -2, 2, seed + 3)}
        else:
            rng = np.random.RandomState(seed)
            o = {"xl": (2 * rng.rand(G["M"], H, F) - 1).astype(np.float32), "xr": (2 * rng.rand(G["K"], H, F) - 1).astype(np.float32),
                 "att": (4 * rng.rand(H, F) - 2).astype(np.float32), "gs": (4 * rng.rand(G["nnz"], H) - 2).astype(np.float32)}
        o["dev"] = {k: _dev(v) for k, v in o.items()}
        G["cache"][key] = o
    return G["cache"][key]


def _run(G, d, slope, H, F):
    """The three launches into guarded, NaN-prefilled tensors -> (score, grad_xl, att_part, grad_xr)."""
    from gespmm_amd import sddmm

    bs, score = _out((G["nnz"], H))
    assert sddmm.gatv2_score(G["rp"], G["ci"], d["xl"], d["xr"], d["att"], negative_slope=slope, out=score) is score
    bl, gxl = _out((G["M"], H, F))
    ba, part = _out((G["M"], H, F))
    r = sddmm.gatv2_score_backward(G["rp"], G["ci"], d["gs"], d["xl"], d["xr"], d["att"], negative_slope=slope, want_att_part=True,
                                   out=(gxl, part))
    assert r[0] is gxl and r[1] is part
    br, gxr = _out((G["K"], H, F))
    assert sddmm.gatv2_score_backward(G["cp"], G["ri"], d["gs"], d["xr"], d["xl"], d["att"], negative_slope=slope, order=G["order"],
                                      out=gxr) is gxr
    for buf, what in ((bs, "score"), (bl, "grad_xl"), (ba, "att_part"), (br, "grad_xr")):
        _guard_ok(buf, what)
    return score, gxl, part, gxr


def _f32(a):
    return _dev(np.asarray(a).astype(np.float32))


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,F", sorted(HF))
@pytest.mark.parametrize("name", ALL)
def test_bits_on_exact_operands(pkg, graphs_, name, H, F, slope):
    """Integer operands, slope 1 or 2^-2: score, grad_xl, att_part and grad_xr equal the float64 restatement cast to fp32, bit for bit;
    every word written (no NaN left), guards intact, empty segments exactly +0. The ranges are checked against the longest segment
    first: every product is a multiple of 2^-2 and every sum of magnitudes stays below 2^22."""
    G = graphs_[name]
    o = _operands(G, H, F, "int")
    longest = max(np.diff(G["rowptr"]).max(), np.diff(G["colptr_h"]).max())
    assert 2 * 8 * F < 2 ** 22 and 2 * 8 * longest < 2 ** 22 and 2 * 2 * longest < 2 ** 22
    (score, terms), row, col = gatv2_float64(G, o, slope)
    assert max(terms.max(), row[2].max(), row[3].max(), col[2].max()) < 2 ** 22
    for ref in (score, row[0], row[1], col[0]):
        assert np.array_equal(ref * 4, np.round(ref * 4))
    got = _run(G, o["dev"], slope, H, F)
    for g, ref, what in zip(got, (score, row[0], row[1], col[0]), ("score", "grad_xl", "att_part", "grad_xr")):
        _same(g, _f32(ref).view(g.shape), "%s %s (%d, %d) slope %s" % (what, name, H, F, slope))
    empty_r, empty_c = _dev(np.diff(G["rowptr"]) == 0), _dev(np.diff(G["colptr_h"]) == 0)
    for g, e in ((got[1], empty_r), (got[2], empty_r), (got[3], empty_c)):
        assert bool((g[e].view(torch.int32) == 0).all()), "an empty segment is +0"


def test_width_one_is_one_rounded_product(pkg, graphs_):
    """F = 1 with real operands: score = att * leaky(xl[rows] + xr[cols]), one rounded product — torch's bits."""
    for name in ("edge", "short_t"):
        G = graphs_[name]
        for H in (1, 3):
            d = _operands(G, H, 1, "real")["dev"]
            for slope in (None, 0.2):
                score = _run(G, d, slope, H, 1)[0]
                t = d["xl"][torch.from_numpy(G["rows_h"]).cuda().long(), :, 0] + d["xr"][G["ci"].long(), :, 0]
                lk = t if slope is None else torch.where(t >= 0, t, t * slope)
                _same(score, d["att"][:, 0] * lk, "F = 1 %s H = %d slope %s" % (name, H, slope))


@pytest.mark.parametrize("H,F", REAL_HF)
@pytest.mark.parametrize("name", ("edge", "hubs", "short_t"))
def test_real_operands_against_float64(pkg, graphs_, name, H, F):
    """Rule c4: every result inside 1e-4 max(|ref|, sum |terms|) of the float64 restatement (terms: att leaky for the score,
    grad_score m for grad_x, grad_score leaky for att_part). The worst ratio of error to bound is printed."""
    G = graphs_[name]
    o = _operands(G, H, F, "real")
    for slope in (None, 0.2):
        (score, terms), row, col = gatv2_float64(G, o, slope)
        got = [g.cpu().numpy() for g in _run(G, o["dev"], slope, H, F)]
        for g, ref, tm, what in zip(got, (score, row[0], row[1], col[0]), (terms, row[2], row[3], col[2]),
                                    ("score", "grad_xl", "att_part", "grad_xr")):
            r = worst_ratio(g, ref, tm, what)
            RATIOS[what] = max(RATIOS.get(what, 0.0), r)
            print("gatv2 %s %s (%d, %d) slope %s: worst error / bound = %.3g" % (what, name, H, F, slope, r))
            assert r <= 1.0, (what, name, H, F, slope, r)


@pytest.mark.parametrize("F", (5, 8, 27))
def test_alignment_changes_no_bit(pkg, graphs_, F):
    """Operands and results carved at 4- and 8-byte alignment: the bits of the aligned call on integer operands (the forward's V drops
    with the least aligned of xl, xr and att — asserted; the backward drops to 4-byte loads)."""
    from gespmm_amd import _lib, sddmm

    H = 3
    for name in ("edge", "short_t"):
        G = graphs_[name]
        d = _operands(G, H, F, "int")["dev"]
        want = _run(G, d, 0.25, H, F)
        for align in (4, 8):
            for who in ("all", "att", "xl", "xr"):
                c = {k: (_carve(v, align) if who in ("all", k) else v) for k, v in d.items()}
                al = {k: (align if who in ("all", k) else 16) for k in ("xl", "xr", "att")}
                V = _lib.describe_gatv2_score(G["M"], G["nnz"], H, F, al["xl"], al["xr"], al["att"])["V"]
                assert V == (1 if F % 2 else min(4, align // 4)), (F, align, who, V)
                score = _carve(torch.full((G["nnz"], H), NAN, device="cuda"), align)
                sddmm.gatv2_score(G["rp"], G["ci"], c["xl"], c["xr"], c["att"], negative_slope=0.25, out=score)
                _same(score, want[0], "score F = %d align %d %s" % (F, align, who))
                gxl, part = (_carve(torch.full((G["M"], H, F), NAN, device="cuda"), align) for _ in range(2))
                sddmm.gatv2_score_backward(G["rp"], G["ci"], c["gs"], c["xl"], c["xr"], c["att"], negative_slope=0.25, want_att_part=True,
                                           out=(gxl, part))
                gxr = _carve(torch.full((G["K"], H, F), NAN, device="cuda"), align)
                sddmm.gatv2_score_backward(G["cp"], G["ri"], c["gs"], c["xr"], c["xl"], c["att"], negative_slope=0.25, order=G["order"], out=gxr)
                for g, w, what in ((gxl, want[1], "grad_xl"), (part, want[2], "att_part"), (gxr, want[3], "grad_xr")):
                    _same(g, w, "%s F = %d align %d %s" % (what, F, align, who))


@pytest.mark.parametrize("bad", (NAN, float("inf")))
def test_a_bad_word_poisons_what_the_restatement_says(pkg, graphs_, bad):
    """One NaN or +inf word in xl: NaN exactly where the float64 restatement has NaN, its bits everywhere else (integer operands; an
    infinite result has the restatement's sign)."""
    G, H, F = graphs_["edge"], 3, 8
    o = dict(_operands(G, H, F, "int"))
    row = int(np.argmax(np.diff(G["rowptr"])))
    o["xl"] = o["xl"].copy()
    o["xl"][row, 1, 5] = bad
    d = dict(o["dev"], xl=_dev(o["xl"]))
    for slope in SLOPES:
        (score, _), rowp, colp = gatv2_float64(G, o, slope)
        got = _run(G, d, slope, H, F)
        for g, ref, what in zip(got, (score, rowp[0], rowp[1], colp[0]), ("score", "grad_xl", "att_part", "grad_xr")):
            g = g.cpu().numpy().reshape(ref.shape)
            assert np.array_equal(np.isnan(g), np.isnan(ref)), what
            ok = ~np.isnan(ref)
            assert np.array_equal(g[ok].view(np.uint32), ref[ok].astype(np.float32).view(np.uint32)), what
        assert np.isnan(score).any() or np.isinf(score).any()


def test_capture_equals_eager_and_two_calls_agree(pkg, graphs_):
    """All three launches replayed from a captured graph give the eager bits (no allocation, no host synchronisation in any of them),
    and a second eager call gives the bits of the first."""
    from gespmm_amd import sddmm

    for name, (H, F) in (("hubs", (8, 8)), ("short_t", (2, 130))):
        G = graphs_[name]
        d = _operands(G, H, F, "real")["dev"]
        eager = _run(G, d, 0.2, H, F)
        again = _run(G, d, 0.2, H, F)
        for a, b in zip(eager, again):
            _same(a, b, "two calls " + name)
        score, gxr = torch.full((G["nnz"], H), NAN, device="cuda"), torch.full((G["K"], H, F), NAN, device="cuda")
        gxl, part = torch.full((G["M"], H, F), NAN, device="cuda"), torch.full((G["M"], H, F), NAN, device="cuda")

        def step():
            sddmm.gatv2_score(G["rp"], G["ci"], d["xl"], d["xr"], d["att"], negative_slope=0.2, out=score)
            sddmm.gatv2_score_backward(G["rp"], G["ci"], d["gs"], d["xl"], d["xr"], d["att"], negative_slope=0.2, want_att_part=True,
                                       out=(gxl, part))
            sddmm.gatv2_score_backward(G["cp"], G["ri"], d["gs"], d["xr"], d["xl"], d["att"], negative_slope=0.2, order=G["order"], out=gxr)

        graph, _ = _capture(step)
        for t in (score, gxl, part, gxr):
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for a, b, what in zip(eager, (score, gxl, part, gxr), ("score", "grad_xl", "att_part", "grad_xr")):
            _same(b, a, "replay %s %s" % (what, name))


def test_no_entries_and_no_width(pkg):
    from gespmm_amd import sddmm

    M, K, H, F = 5, 4, 3, 8
    rp0, ci0 = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    cp0 = torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    xl, xr, att = torch.ones(M, H, F, device="cuda"), torch.ones(K, H, F, device="cuda"), torch.ones(H, F, device="cuda")
    assert tuple(sddmm.gatv2_score(rp0, ci0, xl, xr, att).shape) == (0, H)
    buf, gxl = _out((M, H, F))
    bufa, part = _out((M, H, F))
    sddmm.gatv2_score_backward(rp0, ci0, torch.zeros(0, H, device="cuda"), xl, xr, att, want_att_part=True, out=(gxl, part))
    bufr, gxr = _out((K, H, F))
    sddmm.gatv2_score_backward(cp0, ci0, torch.zeros(0, H, device="cuda"), xr, xl, att, order=ci0, out=gxr)
    for b, t in ((buf, gxl), (bufa, part), (bufr, gxr)):
        _guard_ok(b)
        assert bool((t.view(torch.int32) == 0).all()), "no entries: every word +0"
    # F == 0: a score of zeros, gradients of no words
    rp = torch.tensor([0, 2, 2, 3, 3, 3], dtype=torch.int32, device="cuda")
    ci = torch.tensor([1, 0, 3], dtype=torch.int32, device="cuda")
    bs, score = _out((3, H))
    sddmm.gatv2_score(rp, ci, xl[:, :, :0].contiguous(), xr[:, :, :0].contiguous(), att[:, :0].contiguous(), out=score)
    _guard_ok(bs)
    assert bool((score.view(torch.int32) == 0).all())
    g0 = sddmm.gatv2_score_backward(rp, ci, torch.ones(3, H, device="cuda"), xl[:, :, :0].contiguous(), xr[:, :, :0].contiguous(),
                                    att[:, :0].contiguous(), want_att_part=True)
    assert tuple(g0[0].shape) == (M, H, 0) and tuple(g0[1].shape) == (M, H, 0)
    torch.cuda.synchronize()


def test_python_errors_raise_without_launching(pkg, graphs_):
    """What only device tensors reach: mixed devices, a host ``out``, shapes after the device operands are known. The outputs keep
    their NaN prefill: nothing was launched."""
    from gespmm_amd import sddmm

    G, H, F = graphs_["edge"], 3, 8
    d = _operands(G, H, F, "int")["dev"]
    buf, score = _out((G["nnz"], H))
    bufx, gx = _out((G["M"], H, F))
    for kw in ({"xr": d["xr"].cpu()}, {"att": d["att"].cpu()}, {"ci": G["ci"].cpu()}, {"rp": G["rp"].cpu()}, {"out": score.cpu()},
               {"out": score[:-1]}, {"out": score.t()}, {"att": d["att"][:, :-1].contiguous()}, {"xr": d["xr"][:, :-1].contiguous()},
               {"rp": G["rp"][:-1]}, {"slope": float("nan")}):
        a = dict(rp=G["rp"], ci=G["ci"], xl=d["xl"], xr=d["xr"], att=d["att"], out=score, slope=0.2)
        a.update(kw)
        with pytest.raises(ValueError):
            sddmm.gatv2_score(a["rp"], a["ci"], a["xl"], a["xr"], a["att"], negative_slope=a["slope"], out=a["out"])
    for kw in ({"xr": d["xr"].double()}, {"att": d["att"].half()}, {"ci": G["ci"].long()}, {"out": score.double()}):
        a = dict(rp=G["rp"], ci=G["ci"], xl=d["xl"], xr=d["xr"], att=d["att"], out=score)
        a.update(kw)
        with pytest.raises(TypeError):
            sddmm.gatv2_score(a["rp"], a["ci"], a["xl"], a["xr"], a["att"], out=a["out"])
    for kw in ({"gs": d["gs"].cpu()}, {"gs": d["gs"][:-1]}, {"order": G["order"].cpu()}, {"order": G["order"][:-1]}, {"out": gx.cpu()},
               {"out": gx[:-1]}, {"out": (gx, gx)}, {"xr": d["xr"][:, :, :-1].contiguous()}):
        a = dict(gs=d["gs"], xr=d["xr"], order=None, out=gx)
        a.update(kw)
        with pytest.raises(ValueError):
            sddmm.gatv2_score_backward(G["rp"], G["ci"], a["gs"], d["xl"], a["xr"], d["att"], order=a["order"], out=a["out"])
    for kw in ({"gs": d["gs"].double()}, {"order": G["order"].long()}, {"out": gx.half()}):
        a = dict(gs=d["gs"], order=None, out=gx)
        a.update(kw)
        with pytest.raises(TypeError):
            sddmm.gatv2_score_backward(G["rp"], G["ci"], a["gs"], d["xl"], d["xr"], d["att"], order=a["order"], out=a["out"])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool(torch.isnan(bufx).all()), "a rejected call wrote to its out"
