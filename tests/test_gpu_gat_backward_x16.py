"""The fused GAT backward on fp16 / bf16 grad_out and feat (softmax.gat_backward_el_x16 / gat_backward_er_x16), both forms: delta, grad_el
and grad_er have the BITS of the fp32 entry points on the widened operands wherever both take the same form (and W_d). Patterns, terms
and helpers are those of tests/test_gpu_gat_backward.py (every regime reached by rows and by columns is asserted by its fixture); every
result lands in a NaN-prefilled, guarded tensor."""
import numpy as np
import pytest
import torch

from attention_refs import gat_backward_float64
from test_gpu_edge_dropout import SEEDS, _seed
from test_gpu_edge_dropout import _fused as _fused_drop
from test_gpu_edge_softmax import NAN, _guard_ok, _out, _same
from test_gpu_gat_backward import ALL, _case, _fused, _reals, graphs_  # noqa: F401
from test_gpu_gat_softmax import SLOPES, _terms, patterns  # noqa: F401  (patterns: the fixture graphs_ is built on)
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

PIN = "GESPMM_GAT_BACKWARD_FORM"
DTYPES = (torch.float16, torch.bfloat16)
LANE = ((8, 8, 8), (4, 12, 4), (3, 6, 2), (2, 7, 1), (1, 1, 1))            # (H, F, V of the 16-bit loads)
GROUP = ((4, 16, 4), (3, 20, 4), (1, 64, 8), (2, 128, 16), (1, 512, 64))   # (H, F, W_d); the last with two vectors per lane
NAMES = ("delta", "grad_el", "grad_er")


def _describe(G, H, F, aligns=(16, 16), x16=True):
    from gespmm_amd import _lib

    d = [_lib.describe_gat_backward(G["M"], G["K"], H, F, G["nnz"], transposed=t, aligns=aligns, x16=x16) for t in (False, True)]
    assert (d[0]["form"], d[0]["V"], d[0]["Wd"]) == (d[1]["form"], d[1]["V"], d[1]["Wd"])
    return d[0]["form"], d[0]["V"], d[0]["Wd"]


def _fused_x16(G, c, gout, feat, slope, drop=None):
    """Both 16-bit launches into NaN-prefilled, guarded tensors -> (delta, grad_el, grad_er)."""
    from gespmm_amd import softmax

    H = c["el"].shape[1]
    (bd, delta), (bl, gel), (br, ger) = _out((G["M"], H)), _out((G["M"], H)), _out((G["K"], H))
    r = softmax.gat_backward_el_x16(G["rp"], G["ci"], c["el"], c["er"], c["stats"], gout, feat, negative_slope=slope, out=(delta, gel),
                                    dropout=drop)
    assert r[0] is delta and r[1] is gel
    assert softmax.gat_backward_er_x16(G["cp"], G["ri"], c["el"], c["er"], c["stats"], delta, gout, feat, negative_slope=slope, out=ger,
                                       dropout=drop) is ger
    for buf, what in zip((bd, bl, br), NAMES):
        _guard_ok(buf, what)
    return delta, gel, ger


def _operands(G, H, F, dtype, seed):
    return _reals(G["M"], H, F, seed).to(dtype), _reals(G["K"], H, F, seed + 1).to(dtype)


def _carve16(t, off):
    """Same values, storage `off` bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[off // 2:off // 2 + t.numel()].view(t.shape)
    v.copy_(t)
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == off
    return v


def _check_bits(G, got, want, what):
    for name, u, v in zip(NAMES, got, want):
        assert not bool(torch.isnan(u).any()), "%s: every word of %s must be written" % (what, name)
        _same(u, v, "%s: %s" % (what, name))
    empty_r, empty_c = np.diff(G["rowptr"]) == 0, np.diff(G["colptr_h"]) == 0
    assert np.all(got[0].cpu().numpy()[empty_r].view(np.uint32) == 0) and np.all(got[1].cpu().numpy()[empty_r].view(np.uint32) == 0), what
    assert np.all(got[2].cpu().numpy()[empty_c].view(np.uint32) == 0), what + ": empty columns are +0"


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,F,geo,form", [c + ("lane",) for c in LANE] + [c + ("group",) for c in GROUP],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_bits_of_the_fp32_entries_on_widened_operands(pkg, graphs_, dtype, H, F, geo, form, slope):
    for name in ALL:
        G = graphs_[name]
        f16, v16, wd16 = _describe(G, H, F)
        f32, _, wd32 = _describe(G, H, F, x16=False)
        assert (f16, f32, wd16, wd32) == (form, form, geo if form == "group" else 1, geo if form == "group" else 1), (name, f16, f32)
        assert v16 == (4 if form == "group" else geo), (name, v16)
        c = _case(G, H, slope)
        gout, feat = _operands(G, H, F, dtype, 300 + H * F)
        want = _fused(G, c, gout.float(), feat.float(), slope)
        _check_bits(G, _fused_x16(G, c, gout, feat, slope), want, "%s H=%d F=%d slope=%s" % (name, H, F, slope))


@pytest.mark.parametrize("H,F,form", ((4, 16, "group"), (1, 64, "group"), (8, 8, "lane")))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_dropout_forms(pkg, graphs_, dtype, H, F, form):
    p = 0.25
    for i, name in enumerate(ALL):
        G = graphs_[name]
        assert _describe(G, H, F)[0] == _describe(G, H, F, x16=False)[0] == form
        for slope in SLOPES:
            c = _case(G, H, slope)
            gout, feat = _operands(G, H, F, dtype, 500 + H * F)
            for pair in SEEDS:
                drop = (p, _seed(pair))
                want = _fused_drop(G, c, gout.float(), feat.float(), slope, drop)
                _check_bits(G, _fused_x16(G, c, gout, feat, slope, drop), want, "%s H=%d F=%d slope=%s seed=%s" % (name, H, F, slope, pair))


@pytest.mark.parametrize("H,F", ((8, 32), (1, 128)))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_against_float64(pkg, graphs_, dtype, H, F):
    """Inside 1e-4 max(|ref|, scale) of float64 on the widened operands: test_gpu_gat_backward_group.test_against_float64's bound."""
    for name in ("edge", "padded", "short_t"):
        G = graphs_[name]
        for slope in SLOPES:
            c = _case(G, H, slope)
            gout, feat = _operands(G, H, F, dtype, 900 + H + F)
            ref_el, ref_er, sc_el, sc_er = gat_backward_float64(G["rows_h"], G["colind"], G["M"], G["K"], c["el"].cpu().numpy(),
                                                                c["er"].cpu().numpy(), gout.float().cpu().numpy(),
                                                                feat.float().cpu().numpy(), slope)
            _, gel, ger = _fused_x16(G, c, gout, feat, slope)
            for what, got, ref, scale in (("grad_el", gel, ref_el, sc_el), ("grad_er", ger, ref_er, sc_er)):
                bound = 1e-4 * np.maximum(np.abs(ref), scale)
                err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                worst = float((err / np.where(bound > 0, bound, 1.0)).max())
                print("%s %s %s H=%d F=%d slope=%s: worst error / bound %.4f" % (name, what, dtype, H, F, slope, worst))
                assert np.all(err <= bound), (name, what, H, F, slope, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_alignment(pkg, graphs_, monkeypatch, dtype):
    """Operands 2, 4 and 8 bytes off a 16-byte boundary: lane (V = 1, 2) even under the group pin, group at 8; the bits of aligned copies
    run in the same form."""
    H, F = 3, 32
    for name in ("edge", "short_t"):
        G = graphs_[name]
        c = _case(G, H, 0.2)
        gout, feat = _operands(G, H, F, dtype, 41)
        want = {}
        for pin in ("lane", "group"):
            monkeypatch.setenv(PIN, pin)
            assert _describe(G, H, F) == ((pin, 8, 1) if pin == "lane" else (pin, 4, 4))
            want[pin] = _fused_x16(G, c, gout, feat, 0.2)
        for off, form, V in ((2, "lane", 1), (4, "lane", 2), (8, "group", 4)):
            assert _describe(G, H, F, aligns=(off, off)) == (form, V, 4 if form == "group" else 1)  # (still under the group pin)
            for a, b in ((_carve16(gout, off), _carve16(feat, off)), (gout, _carve16(feat, off))):
                for what, u, v in zip(NAMES, _fused_x16(G, c, a, b, 0.2), want[form]):
                    _same(u, v, "%s %d bytes off: %s" % (name, off, what))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_no_entries(pkg, dtype):
    M, K, H, F = 7, 5, 3, 4
    i0 = torch.empty(0, dtype=torch.int32, device="cuda")
    G = {"rp": torch.zeros(M + 1, dtype=torch.int32, device="cuda"), "ci": i0, "cp": torch.zeros(K + 1, dtype=torch.int32, device="cuda"),
         "ri": i0, "M": M, "K": K}
    c = {"el": torch.ones(M, H, device="cuda"), "er": torch.ones(K, H, device="cuda"), "stats": torch.zeros(M, H, 2, device="cuda")}
    for out in _fused_x16(G, c, torch.ones(M, H, F, device="cuda", dtype=dtype), torch.ones(K, H, F, device="cuda", dtype=dtype), 0.2):
        assert bool((out.view(torch.int32) == 0).all())


@pytest.mark.parametrize("H,F,form", ((8, 8, "lane"), (4, 32, "group")))
@pytest.mark.parametrize("dtype", DTYPES, ids=("f16", "bf16"))
def test_capture_equals_eager(pkg, graphs_, dtype, H, F, form):
    """Both launches captured together; replays see operands edited in place and give the eager bits."""
    from gespmm_amd import softmax

    G = graphs_["edge"]
    assert _describe(G, H, F)[0] == form
    el, er, _ = _terms(G, H, 31)
    gout, feat = _operands(G, H, F, dtype, 1)
    stats = softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2)
    (buf_d, delta), (buf_l, gel), (buf_r, ger) = _out((G["M"], H)), _out((G["M"], H)), _out((G["K"], H))

    def step():
        softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2, out=stats)
        softmax.gat_backward_el_x16(G["rp"], G["ci"], el, er, stats, gout, feat, negative_slope=0.2, out=(delta, gel))
        softmax.gat_backward_er_x16(G["cp"], G["ri"], el, er, stats, delta, gout, feat, negative_slope=0.2, out=ger)

    graph, _ = _capture(step)
    for seed in (33, 35):
        el.copy_(_terms(G, H, seed)[0])
        gout.copy_(_reals(G["M"], H, F, seed).to(dtype))
        for b in (buf_d, buf_l, buf_r):
            b.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for b in (buf_d, buf_l, buf_r):
            _guard_ok(b, "replay")
        want = _fused_x16(G, {"el": el, "er": er, "stats": stats}, gout, feat, 0.2)
        for what, u, v in zip(NAMES, (delta, gel, ger), want):
            _same(u, v, "replayed %s vs eager" % what)
