"""Fused add-softmax on the GPU (softmax.gat_edge_softmax / gat_edge_softmax_backward / edge_segment_sum, op.GATSoftmaxFunction).

The existing GPU ops are the oracle for every bit: the forward must equal ``edge_softmax`` on the score the width-2 ``csr_sddmm_heads``
writes, grad_score ``edge_softmax_backward`` on fl(el + er), grad_el ``edge_segment_sum`` on the stored grad_score — and the sums the
numpy ``lane_sum`` of tests/test_gat_softmax_host.py on the device's own terms, inside that file's bound of float64. Results that take
``out=`` are written into NaN-prefilled tensors with 64 guard words behind them; the backward goes through the C entry the same way.
The launch shape is ASSERTED through gespmm_describe_edge_softmax for every pattern."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import edge_case_csr
from test_edge_softmax_host import IT, WANT_L, hub_degrees, ref_forward, rowptr_of, worst_ratio
from test_gat_softmax_host import csc_of, lane_sum, sum_bound, worst_sum_ratio
from test_gpu_edge_softmax import NAN, _dev, _guard_ok, _out, _padded_hubs, _pattern_with_mean, _same
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

HEADS = (1, 3, 8, 33)
SLOPES = (None, 0.2)


def _short_hubs(L):
    """Rows of L - 1, L and L + 1 entries in front of 3000 rows of 0 .. 3: the mean degree stays below 4, so W = 4 — L - 1 and L are
    swept by four lanes, L + 1 takes the wavefront-per-pair branch of the W = 4 kernel."""
    rng = np.random.RandomState(5)
    return rowptr_of([0, 1, L - 1, L, L + 1, 0, 5] + list(rng.randint(0, 4, size=3000)))


def _pattern(name):
    """-> dict(rowptr, colind, M, K, nnz, W): the host arrays of one test pattern and the W its launch must report."""
    if name == "edge":
        G = dict(edge_case_csr())
        G["W"] = 16
        return G
    rowptr, K, W = {"hubs": (rowptr_of(hub_degrees(WANT_L)), 50, 16), "padded": (_padded_hubs(WANT_L), 50, 8),
                    "short": (_short_hubs(WANT_L), 50, 4), "mean8": (_pattern_with_mean(8, 8), 64, 8)}[name]
    nnz = int(rowptr[-1])
    colind = np.random.RandomState(len(name)).randint(0, K, size=nnz).astype(np.int32)
    return {"rowptr": rowptr, "colind": colind, "M": rowptr.size - 1, "K": K, "nnz": nnz, "W": W}


PATTERNS = ("edge", "hubs", "padded", "short", "mean8")


@pytest.fixture(scope="module")
def patterns(pkg):
    from gespmm_amd import _lib

    out = {}
    for name in PATTERNS:
        G = _pattern(name)
        for H in HEADS:
            assert _lib.describe_edge_softmax(G["M"], G["nnz"], H) == {"W": G["W"], "L": WANT_L}, (name, H)
        G["rp"], G["ci"] = _dev(G["rowptr"]), _dev(G["colind"])
        G["rows"] = torch.repeat_interleave(torch.arange(G["M"], device="cuda"), torch.diff(G["rp"]).long())
        out[name] = G
    degs = np.diff(out["edge"]["rowptr"])
    assert out["edge"]["M"] == 21 and out["edge"]["K"] == 301 and out["edge"]["nnz"] == 890
    assert (degs == IT * 16).any() and (degs == IT * 16 + 1).any(), "rows on both sides of the register / sweep boundary"
    assert np.diff(out["short"]["rowptr"]).max() == WANT_L + 1 and np.diff(out["mean8"]["rowptr"]).max() > IT * 8
    return out


def _terms(G, H, seed):
    """el [M, H], er [K, H] within +-16, grad_alpha [nnz, H] within +-2: device tensors from a seeded host generator."""
    rng = np.random.RandomState(seed)
    el = ((rng.rand(G["M"], H) - 0.5) * 32).astype(np.float32)
    er = ((rng.rand(G["K"], H) - 0.5) * 32).astype(np.float32)
    g = ((rng.rand(G["nnz"], H) - 0.5) * 4).astype(np.float32)
    return _dev(el), _dev(er), _dev(g)


def _score(G, el, er):
    """fl(el[row] + er[col]) by torch: one fp32 add per word."""
    return el[G["rows"]] + er[G["ci"].long()]


def _fused_fwd(G, el, er, slope):
    from gespmm_amd import softmax

    buf, out = _out((G["nnz"], el.shape[1]))
    r = softmax.gat_edge_softmax(G["rp"], G["ci"], el, er, negative_slope=slope, out=out)
    assert r is out
    _guard_ok(buf, "fused forward")
    return out


def _fused_bwd(G, alpha, g, el, er, slope):
    """The backward through the C entry into NaN-prefilled, guarded buffers -> (grad_score, grad_el)."""
    from gespmm_amd import _lib

    H = alpha.shape[1]
    buf_s, gs = _out((G["nnz"], H))
    buf_e, gel = _out((G["M"], H))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    leaky = slope is not None
    rc = _lib.lib.gespmm_gat_softmax_backward_f32(ptr(G["rp"]), ptr(G["ci"]) if leaky else None, ptr(alpha), ptr(g), ptr(el) if leaky else None,
                                                  ptr(er) if leaky else None, ptr(gs), ptr(gel), G["M"], G["K"], H, G["nnz"],
                                                  1.0 if slope is None else slope, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    _guard_ok(buf_s, "grad_score")
    _guard_ok(buf_e, "grad_el")
    assert not bool(torch.isnan(gel).any()), "every word of grad_el must be written"
    return gs, gel


def _seg(ptr, x, order=None):
    from gespmm_amd import softmax

    S = ptr.numel() - 1
    buf, out = _out((S, x.shape[1]) if x.dim() == 2 else (S,))
    r = softmax.edge_segment_sum(ptr, x, order=order, out=out)
    assert r is out
    _guard_ok(buf, "segment sum")
    assert not bool(torch.isnan(out).any()), "every word of out must be written"
    return out


def _check_sum(got, ptr_h, x_h, W, order_h, what):
    """Device sums: the bits of lane_sum on the same terms, inside the bound of float64, empty segments exactly +0."""
    got_h = got.cpu().numpy()
    want = lane_sum(ptr_h, x_h, W, order=order_h)
    assert np.array_equal(got_h.view(np.uint32), want.view(np.uint32)), "%s: %d words differ from the pinned order" % (
        what, int((got_h.view(np.uint32) != want.view(np.uint32)).sum()))
    ref, bound = sum_bound(ptr_h, x_h, W, order=order_h)
    r = worst_sum_ratio(got_h, ref, bound)
    empty = np.diff(ptr_h) == 0
    assert np.all(got_h[empty].view(np.uint32) == 0), "%s: empty segments must be +0" % what
    assert r <= 1.0, (what, r)
    return r


# ------------------------------------------------------------------------------------------------------ 1. forward and backward

@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", HEADS)
def test_forward_and_backward(pkg, patterns, H, slope):
    from gespmm_amd import sddmm, softmax

    for name in PATTERNS:
        G = patterns[name]
        what = "%s H=%d slope=%s" % (name, H, slope)
        el, er, g = _terms(G, H, 1000 + 7 * H + len(name))
        # ---- forward: the bits of the composition it replaces
        q = torch.stack((el, torch.ones_like(el)), dim=-1)
        k = torch.stack((torch.ones_like(er), er), dim=-1)
        score = sddmm.csr_sddmm_heads(G["rp"], G["ci"], q, k)
        _same(score, _score(G, el, er), what + ": the width-2 SDDMM is fl(el + er)")
        want = softmax.edge_softmax(G["rp"], score, negative_slope=slope)
        alpha = _fused_fwd(G, el, er, slope)
        _same(alpha, want, what + ": fused forward vs sddmm + edge_softmax")
        a64, tol = ref_forward(G["rowptr"], score.cpu().numpy(), slope)
        ah = alpha.cpu().numpy()
        rf = worst_ratio(ah, a64, tol)
        one = (np.diff(G["rowptr"]) == 1).nonzero()[0]
        assert one.size >= 1 and np.all(ah[G["rowptr"][one]] == 1.0), "a single-entry row must be exactly 1"
        # ---- backward: grad_score of the existing kernel on the score array, grad_el its row sums in the pinned order
        gs, gel = _fused_bwd(G, alpha, g, el, er, slope)
        _same(gs, softmax.edge_softmax_backward(G["rp"], alpha, g, score=score if slope is not None else None, negative_slope=slope),
              what + ": grad_score")
        _same(gel, _seg(G["rp"], gs), what + ": grad_el vs edge_segment_sum(rowptr, grad_score)")
        rs = _check_sum(gel, G["rowptr"], gs.cpu().numpy(), G["W"], None, what + ": grad_el")
        print("%s: forward error / tolerance %.3f, grad_el error / bound %.3f" % (what, rf, rs))
        assert rf <= 1.0
        # the Python wrapper is the same call
        gs2, gel2 = softmax.gat_edge_softmax_backward(G["rp"], G["ci"], alpha, g, el=el if slope is not None else None,
                                                      er=er if slope is not None else None, negative_slope=slope)
        _same(gs2, gs, what + ": wrapper grad_score")
        _same(gel2, gel, what + ": wrapper grad_el")


def test_no_entries(pkg):
    from gespmm_amd import softmax

    rp0 = torch.zeros(8, dtype=torch.int32, device="cuda")
    ci0 = torch.empty(0, dtype=torch.int32, device="cuda")
    el, er = torch.ones(7, 3, device="cuda"), torch.ones(5, 3, device="cuda")
    e = torch.empty(0, 3, device="cuda")
    assert softmax.gat_edge_softmax(rp0, ci0, el, er, negative_slope=0.2).shape == (0, 3)
    gs, gel = softmax.gat_edge_softmax_backward(rp0, ci0, e, e, el=el, er=er, negative_slope=0.2)
    assert gs.shape == (0, 3) and gel.shape == (7, 3) and bool((gel.view(torch.int32) == 0).all())
    out = _seg(rp0, e)
    assert out.shape == (7, 3) and bool((out.view(torch.int32) == 0).all())


# ------------------------------------------------------------------------------------------------------------ 2. segment sum

@pytest.mark.parametrize("H", HEADS)
def test_segment_sum(pkg, patterns, H):
    """On the CSC arrays of the edge-case pattern through csc_order (S = 301: W = 4), and through a random permutation on the row
    pointers of every pattern; head h is the H = 1 call; two runs give the same bits."""
    from gespmm_amd import _lib, graphs

    G = patterns["edge"]
    colptr, _, order64 = graphs.transpose_csr(G["rp"], G["ci"], G["K"], return_order=True)
    order = order64.to(torch.int32)
    colptr_h, order_h = csc_of(G["rowptr"], G["colind"], G["K"])
    assert np.array_equal(colptr.cpu().numpy(), colptr_h) and np.array_equal(order.cpu().numpy(), order_h)
    assert _lib.describe_edge_softmax(G["K"], G["nnz"], H) == {"W": 4, "L": WANT_L}
    rng = np.random.RandomState(70 + H)
    x_h = ((rng.rand(G["nnz"], H) - 0.5) * 8).astype(np.float32)
    x = _dev(x_h)
    got = _seg(colptr, x, order)
    assert got.shape == (301, H)
    r = _check_sum(got, colptr_h, x_h, 4, order_h, "csc H=%d" % H)
    _same(_seg(colptr, x, order), got, "second run")
    for h in range(H):
        xh = x[:, h].contiguous()
        _same(_seg(colptr, xh, order), got[:, h], "head %d of %d is the H = 1 call" % (h, H))
        _same(_seg(colptr, xh.view(-1, 1), order).view(-1), got[:, h], "f32[nnz] is f32[nnz, 1]")
    for name in PATTERNS:
        P = patterns[name]
        perm_h = np.random.RandomState(80 + len(name)).permutation(P["nnz"]).astype(np.int32)
        y_h = ((np.random.RandomState(81 + H).rand(P["nnz"], H) - 0.5) * 8).astype(np.float32)
        y, perm = _dev(y_h), _dev(perm_h)
        got = _seg(P["rp"], y, perm)
        r = max(r, _check_sum(got, P["rowptr"], y_h, P["W"], perm_h, "%s H=%d permuted" % (name, H)))
        _same(_seg(P["rp"], y, perm), got, "second run, " + name)
        _same(_seg(P["rp"], y[perm.long()].contiguous()), got, "order is the permuted copy, " + name)
    print("H=%d: worst error / bound %.3f" % (H, r))


# ------------------------------------------------------------------------------------------------------------------- 3. capture

def test_capture_equals_eager(pkg, patterns):
    """Forward, backward and segment sum captured together; replays see operands edited in place and give the eager bits."""
    from gespmm_amd import graphs, softmax

    G, H = patterns["short"], 3
    colptr, _, order64 = graphs.transpose_csr(G["rp"], G["ci"], G["K"], return_order=True)
    order = order64.to(torch.int32)
    el, er, g = _terms(G, H, 31)
    buf_a, alpha = _out((G["nnz"], H))
    buf_r, ger = _out((G["K"], H))

    def step():
        softmax.gat_edge_softmax(G["rp"], G["ci"], el, er, negative_slope=0.2, out=alpha)
        gs, gel = softmax.gat_edge_softmax_backward(G["rp"], G["ci"], alpha, g, el=el, er=er, negative_slope=0.2)
        softmax.edge_segment_sum(colptr, gs, order=order, out=ger)
        return gs, gel

    graph, (gs, gel) = _capture(step)
    for seed in (33, 35):
        el2, er2, g2 = _terms(G, H, seed)
        el.copy_(el2)
        er.copy_(er2)
        g.copy_(g2)
        buf_a.fill_(NAN)
        buf_r.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        _guard_ok(buf_a, "replay")
        _guard_ok(buf_r, "replay")
        want_a = _fused_fwd(G, el, er, 0.2)
        _same(alpha, want_a, "replayed forward vs eager")
        want_gs, want_gel = _fused_bwd(G, want_a, g, el, er, 0.2)
        _same(gs, want_gs, "replayed grad_score vs eager")
        _same(gel, want_gel, "replayed grad_el vs eager")
        _same(ger, _seg(colptr, want_gs, order), "replayed grad_er vs eager")


# ------------------------------------------------------------------------------------------------------------ 4. special values

@pytest.mark.parametrize("bad", (float("nan"), float("inf")))
def test_bad_el_poisons_its_own_pairs_only(pkg, patterns, bad):
    """A NaN or +inf in el[r, h] makes the entries of (row r, head h) NaN and nothing else — in a register row, a swept row and a hub row."""
    for name, rows in (("edge", (3, 10)), ("short", (3, 4))):  # degrees 64 and 200 at W = 16; L and L + 1 at W = 4
        G, H = patterns[name], 3
        el, er, _ = _terms(G, H, 41)
        want_nan = np.zeros((G["nnz"], H), dtype=bool)
        for i, r in enumerate(rows):
            el[r, i] = bad
            want_nan[int(G["rowptr"][r]):int(G["rowptr"][r + 1]), i] = True
        assert want_nan.any()
        for slope in SLOPES:
            out = _fused_fwd(G, el, er, slope).cpu().numpy()
            assert np.array_equal(np.isnan(out), want_nan), (name, slope)


# -------------------------------------------------------------------------------------------------------------------- 5. errors

def test_python_errors_raise_without_launching(pkg, patterns):
    from gespmm_amd import softmax

    G, H = patterns["edge"], 4
    rp, ci, nnz, M, K = G["rp"], G["ci"], G["nnz"], G["M"], G["K"]
    el, er, g = _terms(G, H, 51)
    a = torch.rand(nnz, H, device="cuda")
    fwd = lambda *args, **kw: softmax.gat_edge_softmax(*args, **kw)  # noqa: E731
    bwd = lambda *args, **kw: softmax.gat_edge_softmax_backward(*args, **kw)  # noqa: E731
    seg = lambda *args, **kw: softmax.edge_segment_sum(*args, **kw)  # noqa: E731
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError):
            fwd(rp, ci, el.to(dt), er)
        with pytest.raises(TypeError):
            fwd(rp, ci, el, er.to(dt))
        with pytest.raises(TypeError):
            fwd(rp, ci, el, er, out=torch.empty(nnz, H, device="cuda", dtype=dt))
        with pytest.raises(TypeError):
            bwd(rp, ci, a.to(dt), g)
        with pytest.raises(TypeError):
            bwd(rp, ci, a, g.to(dt))
        with pytest.raises(TypeError):
            bwd(rp, ci, a, g, el=el.to(dt), er=er, negative_slope=0.2)
        with pytest.raises(TypeError):
            seg(rp, a.to(dt))
        with pytest.raises(TypeError):
            seg(rp, a, out=torch.empty(M, H, device="cuda", dtype=dt))
    for call in (lambda: fwd(rp.long(), ci, el, er), lambda: fwd(rp, ci.long(), el, er), lambda: bwd(rp, ci.long(), a, g),
                 lambda: seg(rp.long(), a), lambda: seg(rp, a, order=torch.arange(nnz, device="cuda")),  # an int64 order
                 lambda: seg(rp, a, order=np.arange(nnz, dtype=np.int32)), lambda: fwd(rp, ci, el.cpu().numpy(), er)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: fwd(rp, ci, el[:-1], er),                      # el must have M rows
                 lambda: fwd(rp, ci, el, er[:, :-1].contiguous()),      # the heads of el and er differ
                 lambda: fwd(rp, ci, el.view(-1), er.view(-1)),         # rank
                 lambda: fwd(rp, ci, torch.empty(M, 2 * H, device="cuda")[:, ::2], er),  # contiguity
                 lambda: fwd(rp, ci, el.cpu(), er), lambda: fwd(rp, ci, el, er.cpu()), lambda: fwd(rp.cpu(), ci, el, er),
                 lambda: fwd(rp, ci.cpu(), el, er),
                 lambda: fwd(rp, ci, el, er, out=torch.empty(nnz + 1, H, device="cuda")),
                 lambda: fwd(rp, ci, el, er, out=torch.empty(nnz, H)),
                 lambda: fwd(rp, ci, el, er, negative_slope=float("nan")),
                 lambda: bwd(rp, ci, a, g[:-1]), lambda: bwd(rp, ci, a, g.cpu()), lambda: bwd(rp, ci[:-1], a, g),
                 lambda: bwd(rp, ci, a.view(-1), g.view(-1)),
                 lambda: bwd(rp, ci, a, g, negative_slope=0.2),         # a slope needs el and er
                 lambda: bwd(rp, ci, a, g, el=el, negative_slope=0.2),
                 lambda: bwd(rp, ci, a, g, el=el[:-1], er=er, negative_slope=0.2),
                 lambda: bwd(rp, ci, a, g, el=el, er=er[:, :-1].contiguous(), negative_slope=0.2),
                 lambda: seg(rp, a, order=torch.arange(nnz - 1, device="cuda", dtype=torch.int32)),
                 lambda: seg(rp, a, order=torch.arange(nnz, dtype=torch.int32)),
                 lambda: seg(rp, a.cpu()), lambda: seg(rp.cpu(), a), lambda: seg(rp, a.view(nnz, 2, 2)),
                 lambda: seg(rp, a, out=torch.empty(M + 1, H, device="cuda")), lambda: seg(rp, a, out=torch.empty(M, H))):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------------------------ 6. autograd

@pytest.mark.parametrize("slope", SLOPES)
def test_autograd_function(pkg, patterns, slope):
    """GATSoftmaxFunction against torch autograd through a float64 per-row restatement: alpha within ref_forward's tolerance, grad_el and
    grad_er within 1e-4 max|ref| (the project's margin for sums of this size, tests/test_gpu_gat.py; grad_el without a slope is zero
    and borrows grad_er's scale, see below)."""
    import gespmm_amd
    from gespmm_amd import graphs

    G, H = patterns["edge"], 3
    rowptr = G["rowptr"]
    colptr, _, order64 = graphs.transpose_csr(G["rp"], G["ci"], G["K"], return_order=True)
    el0, er0, g = _terms(G, H, 61)
    results = []
    for order in (order64, order64.to(torch.int32)):
        el, er = el0.clone().requires_grad_(True), er0.clone().requires_grad_(True)
        alpha = gespmm_amd.GATSoftmaxFunction.apply(G["rp"], G["ci"], colptr, order, el, er, slope)
        _same(alpha.detach(), _fused_fwd(G, el0, er0, slope), "forward")
        saved = alpha.grad_fn.saved_tensors
        assert len(saved) == (1 if slope is None else 3), "alpha alone without a slope; alpha, el, er with one"
        assert sum(t.numel() == G["nnz"] * H for t in saved) == 1, "nothing of size nnz H besides alpha is saved"
        alpha.backward(g)
        assert el.grad.shape == (G["M"], H) and er.grad.shape == (G["K"], H)
        results.append((alpha.detach(), el.grad, er.grad))
    _same(results[0][1], results[1][1], "grad_el: int64 and int32 csc_order")
    _same(results[0][2], results[1][2], "grad_er: int64 and int32 csc_order")
    alpha, grad_el, grad_er = results[0]
    el64, er64 = el0.double().requires_grad_(True), er0.double().requires_grad_(True)
    s64 = el64[G["rows"]] + er64[G["ci"].long()]
    x64 = s64 if slope is None else torch.nn.functional.leaky_relu(s64, float(np.float32(slope)))
    parts = [torch.softmax(x64[int(rowptr[r]):int(rowptr[r + 1])], dim=0) for r in range(G["M"]) if rowptr[r + 1] > rowptr[r]]
    a64 = torch.cat(parts, dim=0)
    a64.backward(g.double())
    a_ref, tol = ref_forward(rowptr, _score(G, el0, er0).cpu().numpy(), slope)  # (the contract's score is the ROUNDED sum fl(el + er))
    assert worst_ratio(alpha.cpu().numpy(), a_ref, tol) <= 1.0
    assert np.abs(a_ref - a64.detach().cpu().numpy()).max() <= 1e-4, "the two float64 restatements describe the same softmax"
    for name, got, want in (("grad_el", grad_el, el64.grad), ("grad_er", grad_er, er64.grad)):
        err, scale = (got.double() - want).abs().max().item(), want.abs().max().item()
        if name == "grad_el" and slope is None:
            # A softmax does not notice a shift of its row, so without a leaky ReLU the gradient for el is ZERO: the float64 reference is
            # rounding noise (1e-16) and no scale for a margin. The same margin is taken from the sibling sums of the same grad_score
            # terms, the column sums grad_er; the tight check of these row sums is test_forward_and_backward's, against lane_sum.
            assert scale <= 1e-12, scale
            scale = er64.grad.abs().max().item()
        print("%s slope=%s: max err %.3e, max |ref| %.3e" % (name, slope, err, scale))
        assert scale > 0 and err <= 1e-4 * scale, (name, err, scale)
    # each gradient only when asked for
    el, er = el0.clone().requires_grad_(True), er0.clone()
    gespmm_amd.GATSoftmaxFunction.apply(G["rp"], G["ci"], colptr, order64, el, er, slope).backward(g)
    _same(el.grad, grad_el, "grad_el alone")
    el, er = el0.clone(), er0.clone().requires_grad_(True)
    gespmm_amd.GATSoftmaxFunction.apply(G["rp"], G["ci"], colptr, order64, el, er, slope).backward(g)
    assert el.grad is None
    _same(er.grad, grad_er, "grad_er alone")
