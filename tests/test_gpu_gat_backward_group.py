"""The group form of the fused GAT backward on the GPU (gat_backward_group.hip, reached through GESPMM_GAT_BACKWARD_FORM=group): its dot
has the multi-head SDDMM's order, so grad_el and grad_er have the bits of the four-step composition on ANY operands — random reals
here, where the lane form's ascending chain differs. Patterns, terms and helpers are those of tests/test_gpu_gat_backward.py (every
regime reached by rows and by columns is asserted by its fixture); every result lands in a NaN-prefilled, guarded tensor.

One case of the issue is changed, because it contradicts the issue's own form rule: F = 20 is eligible (F % 4 == 0, 16 <= F <= 512), so
under the group pin it does NOT keep the lane form's bits. It is tested here for the stronger property instead (the composition's bits,
with one full and one partial vector per lane), and F = 12 stands in as the ineligible multiple of four."""
import numpy as np
import pytest
import torch

from attention_refs import gat_backward_float64
from test_gpu_edge_dropout import SEEDS, _seed
from test_gpu_edge_dropout import _composition as _composition_drop
from test_gpu_edge_dropout import _fused as _fused_drop
from test_gpu_edge_softmax import NAN, _guard_ok, _out, _same
from test_gpu_gat_backward import ALL, _case, _check_delta_where_exact, _composition, _fused, _ints, _reals, graphs_  # noqa: F401
from test_gpu_gat_softmax import SLOPES, _terms, patterns  # noqa: F401  (patterns: the fixture graphs_ is built on)
from test_gpu_heads import _carve
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

PIN = "GESPMM_GAT_BACKWARD_FORM"
# W_d = 4 with one, with one and a part, and with two vectors per lane; W_d = 8, 16, 64; W_d below and above the segment width
HF = ((1, 16), (4, 16), (3, 20), (3, 32), (1, 64), (2, 128), (1, 512))


def _form(G, H, F, aligns=(16, 16)):
    from gespmm_amd import _lib

    forms = {_lib.describe_gat_backward(G["M"], G["K"], H, F, G["nnz"], transposed=t, aligns=aligns)["form"] for t in (False, True)}
    assert len(forms) == 1, forms
    return forms.pop()


def _check_composition(G, got, want, what):
    delta, gel, ger = got
    alpha, ga, want_el, want_er = want
    assert not bool(torch.isnan(torch.cat((delta.view(-1), gel.view(-1), ger.view(-1)))).any()), what + ": every word must be written"
    _same(gel, want_el, what + ": grad_el")
    _same(ger, want_er, what + ": grad_er")
    empty_r, empty_c = np.diff(G["rowptr"]) == 0, np.diff(G["colptr_h"]) == 0
    assert np.all(delta.cpu().numpy()[empty_r].view(np.uint32) == 0) and np.all(gel.cpu().numpy()[empty_r].view(np.uint32) == 0), what
    assert np.all(ger.cpu().numpy()[empty_c].view(np.uint32) == 0), what + ": empty columns are +0"
    return _check_delta_where_exact(G, delta, alpha, ga, what)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,F", HF)
def test_composition_bits_on_real_operands(pkg, graphs_, monkeypatch, H, F, slope):
    monkeypatch.setenv(PIN, "group")
    for name in ALL:
        G = graphs_[name]
        assert _form(G, H, F) == "group"
        c = _case(G, H, slope)
        gout, feat = _reals(G["M"], H, F, 300 + H * F), _reals(G["K"], H, F, 400 + H * F)
        got = _fused(G, c, gout, feat, slope)
        _check_composition(G, got, _composition(G, c, slope, gout=gout, feat=feat), "%s H=%d F=%d slope=%s" % (name, H, F, slope))


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H,F", ((4, 16), (1, 64)))
def test_dropout_forms(pkg, graphs_, monkeypatch, H, F, slope):
    monkeypatch.setenv(PIN, "group")
    p = 0.25
    for i, name in enumerate(ALL):
        G = graphs_[name]
        assert _form(G, H, F) == "group"
        c = _case(G, H, slope)
        gout, feat = _reals(G["M"], H, F, 500 + H * F), _reals(G["K"], H, F, 600 + H * F)
        got = _fused_drop(G, c, gout, feat, slope, (p, _seed(SEEDS[i % 2])))
        want = _composition_drop(G, c, gout, feat, slope, p, SEEDS[i % 2])
        _check_composition(G, got, want, "%s H=%d F=%d slope=%s p=%s" % (name, H, F, slope, p))


@pytest.mark.parametrize("H,F", ((8, 32), (1, 128)))
def test_against_float64(pkg, graphs_, monkeypatch, H, F):
    monkeypatch.setenv(PIN, "group")
    for name in ("edge", "padded", "short_t"):
        G = graphs_[name]
        assert _form(G, H, F) == "group"
        for slope in SLOPES:
            c = _case(G, H, slope)
            gout, feat = _reals(G["M"], H, F, 900 + H + F), _reals(G["K"], H, F, 901 + H + F)
            ref_el, ref_er, sc_el, sc_er = gat_backward_float64(G["rows_h"], G["colind"], G["M"], G["K"], c["el"].cpu().numpy(),
                                                                c["er"].cpu().numpy(), gout.cpu().numpy(), feat.cpu().numpy(), slope)
            _, gel, ger = _fused(G, c, gout, feat, slope)
            for what, got, ref, scale in (("grad_el", gel, ref_el, sc_el), ("grad_er", ger, ref_er, sc_er)):
                bound = 1e-4 * np.maximum(np.abs(ref), scale)
                err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
                worst = float((err / np.where(bound > 0, bound, 1.0)).max())
                print("%s %s H=%d F=%d slope=%s: worst error / bound %.4f" % (name, what, H, F, slope, worst))
                assert np.all(err <= bound), (name, what, H, F, slope, worst)


@pytest.mark.parametrize("H,F", ((4, 16), (8, 64)))
def test_two_forms_one_answer_on_exact_operands(pkg, graphs_, monkeypatch, H, F):
    for name in ALL:
        G = graphs_[name]
        c = _case(G, H, 0.2)
        gout, feat = _ints(G["M"], H, F, 100 + H * F), _ints(G["K"], H, F, 200 + H * F)
        got = {}
        for pin in ("lane", "group"):
            monkeypatch.setenv(PIN, pin)
            assert _form(G, H, F) == pin
            got[pin] = _fused(G, c, gout, feat, 0.2)
        for what, u, v in zip(("delta", "grad_el", "grad_er"), got["group"], got["lane"]):
            _same(u, v, "%s H=%d F=%d: %s" % (name, H, F, what))


@pytest.mark.parametrize("H,F,align", ((1, 64, 8), (3, 12, 16)))
def test_ineligible_calls_keep_the_lane_form_under_the_group_pin(pkg, graphs_, monkeypatch, H, F, align):
    for name in ("edge", "short_t"):
        G = graphs_[name]
        c = _case(G, H, 0.2)
        gout, feat = _reals(G["M"], H, F, 41), _reals(G["K"], H, F, 42)
        if align != 16:
            feat = _carve(feat, align)
        got = {}
        for pin in ("lane", "group"):
            monkeypatch.setenv(PIN, pin)
            assert _form(G, H, F, aligns=(16, align)) == "lane"
            got[pin] = _fused(G, c, gout, feat, 0.2)
        for what, u, v in zip(("delta", "grad_el", "grad_er"), got["group"], got["lane"]):
            _same(u, v, "%s H=%d F=%d: %s" % (name, H, F, what))


def test_capture_equals_eager(pkg, graphs_, monkeypatch):
    """Both launches captured together under the pin; replays see operands edited in place and give the eager bits."""
    from gespmm_amd import softmax

    monkeypatch.setenv(PIN, "group")
    G, H, F = graphs_["edge"], 4, 32
    assert _form(G, H, F) == "group"
    el, er, _ = _terms(G, H, 31)
    gout, feat = _reals(G["M"], H, F, 1), _reals(G["K"], H, F, 2)
    stats = softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2)
    (buf_d, delta), (buf_l, gel), (buf_r, ger) = _out((G["M"], H)), _out((G["M"], H)), _out((G["K"], H))

    def step():
        softmax.gat_softmax_stats(G["rp"], G["ci"], el, er, negative_slope=0.2, out=stats)
        softmax.gat_backward_el(G["rp"], G["ci"], el, er, stats, gout, feat, negative_slope=0.2, out=(delta, gel))
        softmax.gat_backward_er(G["cp"], G["ri"], el, er, stats, delta, gout, feat, negative_slope=0.2, out=ger)

    graph, _ = _capture(step)
    for seed in (33, 35):
        el.copy_(_terms(G, H, seed)[0])
        gout.copy_(_reals(G["M"], H, F, seed))
        for b in (buf_d, buf_l, buf_r):
            b.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for b in (buf_d, buf_l, buf_r):
            _guard_ok(b, "replay")
        want = _fused(G, {"el": el, "er": er, "stats": stats}, gout, feat, 0.2)
        for what, u, v in zip(("delta", "grad_el", "grad_er"), (delta, gel, ger), want):
            _same(u, v, "replayed %s vs eager" % what)


def test_layer_function_has_the_unfused_bits(pkg, monkeypatch):
    """GATAggregateFunction(fused_backward=True) under the group pin: every gradient bit-equal to fused_backward=False."""
    import gespmm_amd
    from test_gpu_gat import _rand
    from test_gpu_gat_aggregate_layer import _bits_equal
    from test_gpu_gat_backward_layer import _graph

    monkeypatch.setenv(PIN, "group")
    n, host, a = _graph("edge")
    H, F = 4, 16
    from gespmm_amd import _lib

    assert _lib.describe_gat_backward(n, n, H, F, host["nnz"])["form"] == "group"
    el0, er0, feat0, gout = _rand((n, H), 1) * 8, _rand((n, H), 2) * 8, _rand((n, H, F), 3), _rand((n, H, F), 4)
    got = {}
    for fused in (False, True):
        el, er, feat = (t.clone().requires_grad_(True) for t in (el0, er0, feat0))
        out = gespmm_amd.GATAggregateFunction.apply(*a, el, er, feat, 0.2, fused)
        out.backward(gout)
        got[fused] = (out.detach(), feat.grad, el.grad, er.grad)
    for what, u, v in zip(("forward", "grad_feat", "grad_el", "grad_er"), got[True], got[False]):
        assert _bits_equal(u, v), what
