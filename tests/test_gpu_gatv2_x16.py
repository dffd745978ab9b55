"""The GATv2 edge score on fp16 / bf16 node operands on the GPU (sddmm.gatv2_score_x16 / gatv2_score_backward_x16): the forward against
the float64 restatement of tests/test_gatv2_host.py on the WIDENED operands — bit for bit on small integers, inside the project's bound on
real operands, and bit-equal to the fp32 kernel wherever both resolve to the same (V, W) — and the backward against the fp32 kernel on
the widened operands, bit for bit: att_part as it is, grad_x rounded once. Patterns and shapes: tests/gatv2_x16_cases.py (a few hundred
rows; every V of the forward, asserted through gespmm_describe_gatv2_score_x16). Results go through ``out=`` into NaN-prefilled
tensors with guard elements behind them."""
import numpy as np
import pytest
import torch

from attention_refs import gatv2_float64
from gatv2_x16_cases import DTYPES, EXACT_SLOPES, SHAPES, SLOPES, check_patterns, edge_pattern, gaps_pattern, operands
from test_gatv2_host import worst_ratio
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
RESULTS = ("score", "grad_xl", "att_part", "grad_xr")


def _dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def _guarded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), NAN, dtype=dtype, device="cuda")
    return buf, buf[:n].view(*shape)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = int((_bits(got) != _bits(want)).sum())
    assert bad == 0, "%s: %d of %d elements differ" % (what, bad, got.numel())


def _carve(t, off):
    """Same values, storage ``off`` bytes past a 16-byte boundary: the address's alignment is the largest power of two in ``off``."""
    es = t.element_size()
    assert off % es == 0 and 0 < off < 16
    buf = torch.full((t.numel() + 16,), NAN, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off // es:off // es + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off and v.is_contiguous()
    return v


@pytest.fixture(scope="module")
def pats(pkg):
    from gespmm_amd import _lib

    out = {"gaps": gaps_pattern(), "edge": edge_pattern()}
    check_patterns(out)
    for G in out.values():
        G["rp"], G["ci"] = _dev(G["rowptr"]), _dev(G["colind"])
        G["cp"], G["ri"], G["order"] = _dev(G["colptr_h"]), _dev(G["rowind_h"]), _dev(G["order_h"])
        G["cache"] = {}
        for (H, F), V in SHAPES.items():
            assert _lib.describe_gatv2_score(G["M"], G["nnz"], H, F, x16=True)["V"] == V, (H, F)
    return out


def _case(G, H, F, kind, dt):
    """Operands of one case on the host and on the device, made once and never edited."""
    key = (H, F, kind, dt)
    if key not in G["cache"]:
        o = operands(G, H, F, kind, dt)
        o["dev"] = {k: _dev(o[k]) for k in ("xl", "xr", "att", "gs")}
        o["dev_wide"] = {k: _dev(v) for k, v in o["wide"].items()}
        G["cache"][key] = o
    return G["cache"][key]


def _run(G, d, slope, H, F):
    """The three launches into guarded, NaN-prefilled tensors -> (score f32, grad_xl 16-bit, att_part f32, grad_xr 16-bit)."""
    from gespmm_amd import sddmm

    dt = d["xl"].dtype
    bs, score = _guarded((G["nnz"], H))
    assert sddmm.gatv2_score_x16(G["rp"], G["ci"], d["xl"], d["xr"], d["att"], negative_slope=slope, out=score) is score
    bl, gxl = _guarded((G["M"], H, F), dt)
    ba, part = _guarded((G["M"], H, F))
    r = sddmm.gatv2_score_backward_x16(G["rp"], G["ci"], d["gs"], d["xl"], d["xr"], d["att"], negative_slope=slope, want_att_part=True,
                                       out=(gxl, part))
    assert r[0] is gxl and r[1] is part
    br, gxr = _guarded((G["K"], H, F), dt)
    assert sddmm.gatv2_score_backward_x16(G["cp"], G["ri"], d["gs"], d["xr"], d["xl"], d["att"], negative_slope=slope, order=G["order"],
                                          out=gxr) is gxr
    for buf, what in zip((bs, bl, ba, br), RESULTS):
        assert bool(torch.isnan(buf[-GUARD:]).all()), "guard elements after %s were written" % what
    return score, gxl, part, gxr


def _run_f32(G, w, slope):
    """The fp32 entry points on the widened operands -> (score, grad_xl, att_part, grad_xr), all fp32."""
    from gespmm_amd import sddmm

    score = sddmm.gatv2_score(G["rp"], G["ci"], w["xl"], w["xr"], w["att"], negative_slope=slope)
    gxl, part = sddmm.gatv2_score_backward(G["rp"], G["ci"], w["gs"], w["xl"], w["xr"], w["att"], negative_slope=slope, want_att_part=True)
    gxr = sddmm.gatv2_score_backward(G["cp"], G["ri"], w["gs"], w["xr"], w["xl"], w["att"], negative_slope=slope, order=G["order"])
    return score, gxl, part, gxr


def _f32(a):
    return _dev(np.asarray(a).astype(np.float32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,F", sorted(SHAPES))
def test_forward_bits_on_exact_operands(pkg, pats, H, F, dt):
    """Small integers both 16-bit types hold, slope 1 or 2^-2: every sum is exact in fp32 (multiples of 2^-2 below 2^22), so the score
    equals the float64 restatement bit for bit whatever (V, W); every word written, guards intact."""
    assert 2 * 8 * F < 2 ** 22
    for name, G in pats.items():
        o = _case(G, H, F, "int", dt)
        for slope in EXACT_SLOPES:
            (ref, terms), _, _ = gatv2_float64(G, o["wide"], slope)
            assert terms.max() < 2 ** 22 and np.array_equal(ref * 4, np.round(ref * 4))
            from gespmm_amd import sddmm

            buf, score = _guarded((G["nnz"], H))
            sddmm.gatv2_score_x16(G["rp"], G["ci"], o["dev"]["xl"], o["dev"]["xr"], o["dev"]["att"], negative_slope=slope, out=score)
            assert bool(torch.isnan(buf[-GUARD:]).all())
            _same(score, _f32(ref), "score %s (%d, %d) %s slope %s" % (name, H, F, dt, slope))


def _same_geometry(L, G, H, F):
    a, b = L.describe_gatv2_score(G["M"], G["nnz"], H, F, x16=True), L.describe_gatv2_score(G["M"], G["nnz"], H, F)
    return (a["V"], a["W"]) == (b["V"], b["W"])


def test_some_shape_shares_its_geometry_with_fp32(pkg, pats):
    """Read from the two describe calls, not assumed: at least one tested shape resolves to the same (V, W) on fp32 and on 16-bit
    operands — the bit comparison of the next test is not vacuous. (4, 4) is expected to be one."""
    from gespmm_amd import _lib

    G = pats["gaps"]
    shared = [hf for hf in SHAPES if _same_geometry(_lib, G, *hf)]
    assert shared and (4, 4) in shared, shared


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,F", sorted(SHAPES))
def test_forward_real_operands(pkg, pats, H, F, dt):
    """The project's bound: |score - ref| <= 1e-4 max(|ref|, sum |att leaky|) against the float64 restatement of the widened operands;
    and where fp32 and 16-bit resolve to the same (V, W), the bits of sddmm.gatv2_score on the widened operands."""
    from gespmm_amd import _lib, sddmm

    G = pats["gaps"]
    o = _case(G, H, F, "real", dt)
    d, w = o["dev"], o["dev_wide"]
    for slope in SLOPES:
        ref, terms = gatv2_float64(G, o["wide"], slope)[0]
        buf, score = _guarded((G["nnz"], H))
        sddmm.gatv2_score_x16(G["rp"], G["ci"], d["xl"], d["xr"], d["att"], negative_slope=slope, out=score)
        r = worst_ratio(score.cpu().numpy(), ref, terms, "score")
        print("gatv2 x16 score (%d, %d) %s slope %s: worst error / bound = %.3g" % (H, F, dt, slope, r))
        assert r <= 1.0, (H, F, dt, slope, r)
        if _same_geometry(_lib, G, H, F):
            _same(score, sddmm.gatv2_score(G["rp"], G["ci"], w["xl"], w["xr"], w["att"], negative_slope=slope),
                  "score against the fp32 kernel (%d, %d) %s slope %s" % (H, F, dt, slope))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,F", sorted(SHAPES))
def test_backward_is_the_fp32_chain_rounded_once(pkg, pats, H, F, dt):
    """Row pass (with att_part) and column pass (through csc_order) on real operands: grad_x is the fp32 kernel's grad_x on the widened
    operands narrowed by torch (to nearest even), att_part that kernel's att_part, bit for bit — the chains are one per output word in
    segment order, whatever either kernel's geometry. The inputs witness the rounding: some word of the fp32 reference is rounded
    AWAY from zero by the narrowing, which truncation would not do."""
    G = pats["gaps"]
    o = _case(G, H, F, "real", dt)
    for slope in SLOPES:
        got = _run(G, o["dev"], slope, H, F)
        want = _run_f32(G, o["dev_wide"], slope)
        what = "(%d, %d) %s slope %s" % (H, F, dt, slope)
        assert got[1].dtype == dt and got[3].dtype == dt and got[2].dtype == torch.float32
        away = 0
        for i in (1, 3):
            narrowed = want[i].to(dt)
            away += int((narrowed.float().abs() > want[i].abs()).sum())
            _same(got[i], narrowed, RESULTS[i] + " " + what)
        assert away > 0, "no word of the fp32 gradients rounds away from zero: truncation would pass " + what
        _same(got[2], want[2], "att_part " + what)
        empty = _dev(np.diff(G["rowptr"]) == 0)
        assert bool((_bits(got[1][empty]) == 0).all()) and bool((_bits(got[2][empty]) == 0).all()), "an empty segment is +0"
        assert bool((_bits(got[3][_dev(np.diff(G["colptr_h"]) == 0)]) == 0).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,F", ((3, 8), (2, 6)))
def test_alignment_changes_no_bit(pkg, pats, H, F, dt):
    """xl, xr and the 16-bit results carved 2, 4 and 8 bytes past a 16-byte boundary, att and att_part 4 and 8: the forward's V drops
    as described (asserted) and the backward takes narrower vectors; on exact operands every result keeps the bits of the aligned
    call."""
    from gespmm_amd import _lib, sddmm

    G = pats["edge"]
    d = _case(G, H, F, "int", dt)["dev"]
    want = _run(G, d, 0.25, H, F)
    top = 8 if F % 8 == 0 else 2
    cases = [(who, off) for who in ("xl", "xr", "x") for off in (2, 4, 8)] + [("att", 4), ("att", 8), ("all", 4), ("all", 8)]
    for who, off in cases:
        al = {k: (off if who in (k, "all") or (who == "x" and k != "att") else 16) for k in ("xl", "xr", "att")}
        V = _lib.describe_gatv2_score(G["M"], G["nnz"], H, F, al["xl"], al["xr"], al["att"], x16=True)["V"]
        by_x = min(al["xl"], al["xr"]) // 2
        by_att = 8 if al["att"] >= 16 else al["att"] // 4
        assert V == min(top, by_x, by_att), (F, who, off, V)
        c = {k: (_carve(d[k], al[k]) if al[k] != 16 else d[k]) for k in ("xl", "xr", "att")}
        x_off, f_off = min(al["xl"], al["xr"]), al["att"]
        score = torch.full((G["nnz"], H), NAN, device="cuda")
        sddmm.gatv2_score_x16(G["rp"], G["ci"], c["xl"], c["xr"], c["att"], negative_slope=0.25, out=score)
        gxl = torch.full((G["M"], H, F), NAN, dtype=dt, device="cuda")
        part = torch.full((G["M"], H, F), NAN, device="cuda")
        gxr = torch.full((G["K"], H, F), NAN, dtype=dt, device="cuda")
        if x_off != 16:
            gxl, gxr = _carve(gxl, x_off), _carve(gxr, x_off)
        if f_off != 16:
            part = _carve(part, f_off)
        sddmm.gatv2_score_backward_x16(G["rp"], G["ci"], d["gs"], c["xl"], c["xr"], c["att"], negative_slope=0.25, want_att_part=True,
                                       out=(gxl, part))
        sddmm.gatv2_score_backward_x16(G["cp"], G["ri"], d["gs"], c["xr"], c["xl"], c["att"], negative_slope=0.25, order=G["order"],
                                       out=gxr)
        for g, w, what in zip((score, gxl, part, gxr), want, RESULTS):
            _same(g, w, "%s F = %d %s at %d bytes" % (what, F, who, off))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("bad", (NAN, float("inf")))
def test_a_bad_element_poisons_what_the_restatement_says(pkg, pats, bad, dt):
    """One NaN or +inf element in xl: NaN exactly where the float64 restatement has NaN, the reference's bits everywhere else (integer
    operands; the 16-bit gradients are the restatement narrowed once)."""
    G, H, F = pats["edge"], 8, 8
    o = _case(G, H, F, "int", dt)
    row = int(np.argmax(np.diff(G["rowptr"])))
    xl = o["xl"].clone()
    xl[row, 1, 5] = bad
    wide = dict(o["wide"], xl=xl.float().numpy())
    d = dict(o["dev"], xl=_dev(xl))
    for slope in EXACT_SLOPES:
        (score, _), rowp, colp = gatv2_float64(G, wide, slope)
        got = _run(G, d, slope, H, F)
        for g, ref, what in zip(got, (score, rowp[0], rowp[1], colp[0]), RESULTS):
            want = torch.from_numpy(np.asarray(ref).astype(np.float32)).to(g.dtype).view(g.shape)
            g = g.cpu()
            assert torch.equal(torch.isnan(g), torch.isnan(want)), what
            ok = ~torch.isnan(want)
            assert torch.equal(_bits(g)[ok], _bits(want)[ok]), what
        assert np.isnan(score).any() or np.isinf(score).any()


@pytest.mark.parametrize("dt", DTYPES)
def test_capture_equals_eager_and_two_calls_agree(pkg, pats, dt):
    """All three launches replayed from a captured graph give the eager bits (no allocation, no host synchronisation in any of them),
    and a second eager call gives the bits of the first."""
    from gespmm_amd import sddmm

    G = pats["gaps"]
    for H, F in ((8, 8), (2, 130)):
        d = _case(G, H, F, "real", dt)["dev"]
        eager = _run(G, d, 0.2, H, F)
        for a, b, what in zip(eager, _run(G, d, 0.2, H, F), RESULTS):
            _same(a, b, "two calls " + what)
        score, part = torch.full((G["nnz"], H), NAN, device="cuda"), torch.full((G["M"], H, F), NAN, device="cuda")
        gxl, gxr = torch.full((G["M"], H, F), NAN, dtype=dt, device="cuda"), torch.full((G["K"], H, F), NAN, dtype=dt, device="cuda")

        def step():
            sddmm.gatv2_score_x16(G["rp"], G["ci"], d["xl"], d["xr"], d["att"], negative_slope=0.2, out=score)
            sddmm.gatv2_score_backward_x16(G["rp"], G["ci"], d["gs"], d["xl"], d["xr"], d["att"], negative_slope=0.2, want_att_part=True,
                                           out=(gxl, part))
            sddmm.gatv2_score_backward_x16(G["cp"], G["ri"], d["gs"], d["xr"], d["xl"], d["att"], negative_slope=0.2, order=G["order"],
                                           out=gxr)

        graph, _ = _capture(step)
        for t in (score, gxl, part, gxr):
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for a, b, what in zip(eager, (score, gxl, part, gxr), RESULTS):
            _same(b, a, "replay %s (%d, %d)" % (what, H, F))


@pytest.mark.parametrize("dt", DTYPES)
def test_no_entries_and_no_width(pkg, dt):
    from gespmm_amd import sddmm

    M, K, H, F = 5, 4, 3, 8
    rp0, ci0 = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    cp0 = torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    xl, xr = torch.ones(M, H, F, dtype=dt, device="cuda"), torch.ones(K, H, F, dtype=dt, device="cuda")
    att = torch.ones(H, F, device="cuda")
    s0 = sddmm.gatv2_score_x16(rp0, ci0, xl, xr, att)
    assert tuple(s0.shape) == (0, H) and s0.dtype == torch.float32
    buf, gxl = _guarded((M, H, F), dt)
    bufa, part = _guarded((M, H, F))
    sddmm.gatv2_score_backward_x16(rp0, ci0, torch.zeros(0, H, device="cuda"), xl, xr, att, want_att_part=True, out=(gxl, part))
    bufr, gxr = _guarded((K, H, F), dt)
    sddmm.gatv2_score_backward_x16(cp0, ci0, torch.zeros(0, H, device="cuda"), xr, xl, att, order=ci0, out=gxr)
    for b, t in ((buf, gxl), (bufa, part), (bufr, gxr)):
        assert bool(torch.isnan(b[-GUARD:]).all())
        assert bool((_bits(t) == 0).all()), "no entries: every element +0"
    fresh = sddmm.gatv2_score_backward_x16(rp0, ci0, torch.zeros(0, H, device="cuda"), xl, xr, att, want_att_part=True)
    assert fresh[0].dtype == dt and fresh[1].dtype == torch.float32 and tuple(fresh[0].shape) == (M, H, F)
    # F == 0: a score of zeros, gradients of no elements
    rp = torch.tensor([0, 2, 2, 3, 3, 3], dtype=torch.int32, device="cuda")
    ci = torch.tensor([1, 0, 3], dtype=torch.int32, device="cuda")
    bs, score = _guarded((3, H))
    sddmm.gatv2_score_x16(rp, ci, xl[:, :, :0].contiguous(), xr[:, :, :0].contiguous(), att[:, :0].contiguous(), out=score)
    assert bool(torch.isnan(bs[-GUARD:]).all()) and bool((_bits(score) == 0).all())
    g0 = sddmm.gatv2_score_backward_x16(rp, ci, torch.ones(3, H, device="cuda"), xl[:, :, :0].contiguous(), xr[:, :, :0].contiguous(),
                                        att[:, :0].contiguous(), want_att_part=True)
    assert tuple(g0[0].shape) == (M, H, 0) and g0[0].dtype == dt and tuple(g0[1].shape) == (M, H, 0) and g0[1].dtype == torch.float32
    torch.cuda.synchronize()
