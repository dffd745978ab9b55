"""Edge softmax on the GPU (softmax.edge_softmax / edge_softmax_backward, op.EdgeSoftmaxFunction).

Every result is written into a NaN-prefilled tensor carved out of a buffer with 64 guard words after it (they must still be NaN
afterwards, and no NaN may be left where the float64 reference has a number: a skipped element shows). Forward is held against
float64 on the same fp32 inputs, backward against float64 on the device's own alpha, both within the derived tolerances of
tests/test_edge_softmax_host.py (u = 2^-24):

    forward    |out - a_e|   <= a_e 2^-23 (2 |z_e| + 2 zbar + d + 8) + 2^-120
    backward   |grad - ref|  <= 2^-23 (d + 4) a_e (|g_e| + sum_p |a_p g_p|) k + 2^-120

The launch shape is ASSERTED through gespmm_describe_edge_softmax wherever a test depends on it."""
import numpy as np
import pytest
import torch

from helpers import edge_case_csr
from test_edge_softmax_host import IT, WANT_L, hub_degrees, ref_backward, ref_forward, rowptr_of, want_W, worst_ratio
from test_gpu_sddmm_forms import _capture

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), NAN, device="cuda")
    return buf, buf[:n].view(*shape)


def _guard_ok(buf, what=""):
    assert bool(torch.isnan(buf[-GUARD:]).all()), "guard words after out were written: %s" % (what,)


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    assert bad == 0, "%s: %d of %d words differ" % (what, bad, got.numel())


def _fwd(rp, score, slope=None):
    from gespmm_amd import softmax

    buf, out = _out(score.shape)
    r = softmax.edge_softmax(rp, score, out=out, negative_slope=slope)
    assert r is out
    _guard_ok(buf, "forward")
    return out


def _bwd(rp, alpha, grad, score=None, slope=None):
    from gespmm_amd import softmax

    buf, out = _out(alpha.shape)
    r = softmax.edge_softmax_backward(rp, alpha, grad, score=score, negative_slope=slope, out=out)
    assert r is out
    _guard_ok(buf, "backward")
    return out


def _scores(oracle, nnz, H, scale, seed):
    return (np.float32(scale) * oracle.hash_val(nnz * H, seed=seed)).reshape(nnz, H)


def _check_both(oracle, rowptr, H, slope, seed, what):
    """Forward and backward of one (pattern, H, slope) within tolerance; returns the device's alpha (host array)."""
    nnz = int(rowptr[-1])
    rp = _dev(rowptr)
    s = _scores(oracle, nnz, H, 32.0, seed)
    g = _scores(oracle, nnz, H, 4.0, seed + 1)
    sd, gd = _dev(s), _dev(g)
    alpha = _fwd(rp, sd, slope)
    a, tol = ref_forward(rowptr, s, slope)
    ah = alpha.cpu().numpy()
    rf = worst_ratio(ah, a, tol)
    grad = _bwd(rp, alpha, gd, sd if slope is not None else None, slope)
    gref, gtol = ref_backward(rowptr, ah, g, s, slope)
    rb = worst_ratio(grad.cpu().numpy(), gref, gtol)
    print("%s H=%d slope=%s: worst error / tolerance forward %.3f backward %.3f" % (what, H, slope, rf, rb))
    assert rf <= 1.0 and rb <= 1.0, (what, H, slope, rf, rb)
    return ah


@pytest.fixture(scope="module")
def edge():
    return edge_case_csr()


def _padded_hubs(L):
    """The hub degrees in front of 3000 rows of 0 .. 3 entries: the mean degree — and with it W — stays small, so the rows past L take
    the wavefront-per-pair branch of a W < 64 kernel."""
    rng = np.random.RandomState(3)
    return rowptr_of(hub_degrees(L) + list(rng.randint(0, 4, size=3000)))


# ------------------------------------------------------------------------------------------------------------------- 1. grid

@pytest.mark.parametrize("slope", (None, 0.2))
@pytest.mark.parametrize("H", (1, 2, 3, 5, 8, 16, 33))
def test_grid(pkg, oracle, edge, H, slope):
    from gespmm_amd import _lib

    G = edge
    assert G["M"] == 21 and G["nnz"] == 890
    d = _lib.describe_edge_softmax(G["M"], G["nnz"], H)
    assert d == {"W": 16, "L": WANT_L}, d
    degs = np.diff(G["rowptr"])
    assert (degs == IT * d["W"]).any() and (degs == IT * d["W"] + 1).any(), "rows on both sides of the register / sweep boundary"
    ah = _check_both(oracle, G["rowptr"], H, slope, 100 + H, "grid")
    one = (np.diff(G["rowptr"]) == 1).nonzero()[0]
    assert one.size >= 1 and np.all(ah[G["rowptr"][one]] == 1.0), "a single-entry row must be exactly 1"


def test_one_dimensional_score(pkg, oracle, edge):
    """f32[nnz] is the H = 1 call: same bits, same shape back."""
    G = edge
    rp = _dev(G["rowptr"])
    s = _dev(_scores(oracle, G["nnz"], 1, 32.0, 7))
    a2 = _fwd(rp, s, 0.2)
    a1 = _fwd(rp, s.view(-1), 0.2)
    assert a1.shape == (G["nnz"],)
    _same(a1.view(-1, 1), a2, "1-d forward")
    g = _dev(_scores(oracle, G["nnz"], 1, 4.0, 8))
    _same(_bwd(rp, a1, g.view(-1), s.view(-1), 0.2).view(-1, 1), _bwd(rp, a2, g, s, 0.2), "1-d backward")


def test_no_entries(pkg):
    from gespmm_amd import softmax

    rp0 = torch.zeros(8, dtype=torch.int32, device="cuda")
    for shape in ((0,), (0, 3)):
        e = torch.empty(shape, device="cuda")
        assert softmax.edge_softmax(rp0, e).shape == shape and softmax.edge_softmax_backward(rp0, e, e).shape == shape


# ------------------------------------------------------------------------------------------------------------------ 2. every W

def _pattern_with_mean(mean, W):
    """M = 64 rows, nnz = 64 * mean: empty rows, one row longer than IT * W (the sweep regime), the rest short (the register regime)."""
    rng = np.random.RandomState(mean)
    degs = rng.randint(1, max(2, 2 * mean - 1), size=64)
    degs[[5, 17, 63]] = 0
    degs[40] = IT * W + 3
    k = 0
    while degs.sum() != 64 * mean:  # land on the entry count that fixes W, without touching the chosen rows
        r = k % 64
        k += 1
        if r in (5, 17, 40, 63):
            continue
        if degs.sum() < 64 * mean:
            degs[r] += 1
        elif degs[r] > 1:
            degs[r] -= 1
    return rowptr_of(list(degs))


@pytest.mark.parametrize("mean,W", ((3, 4), (7, 8), (12, 16), (24, 16), (50, 16), (100, 16)))
def test_every_W(pkg, oracle, mean, W):
    from gespmm_amd import _lib

    rowptr = _pattern_with_mean(mean, W)
    degs = np.diff(rowptr)
    nnz = int(rowptr[-1])
    assert nnz == 64 * mean <= 6400 and want_W(64, nnz) == W
    assert (degs == 0).sum() >= 3 and degs.max() > IT * W and (degs[degs > 0] <= IT * W).sum() >= 8 and degs.max() <= WANT_L
    for H, slope in ((3, None), (8, 0.2)):
        assert _lib.describe_edge_softmax(64, nnz, H) == {"W": W, "L": WANT_L}
        _check_both(oracle, rowptr, H, slope, 200 + mean, "W=%d" % W)


# ------------------------------------------------------------------------------------------------------------------ 3. hub rows

@pytest.mark.parametrize("H", (1, 3))
def test_hub_rows(pkg, oracle, H):
    """Rows of L - 1, L, L + 1 and 3 L + 7 entries: the last two take the wavefront-per-pair branch, L - 1 and L are swept by one lane
    group. On their own (11 rows: W = 16) and in front of many short rows (W = 8)."""
    from gespmm_amd import _lib

    L = _lib.describe_edge_softmax(11, 12000, H)["L"]
    assert L == WANT_L
    rowptr = rowptr_of(hub_degrees(L))
    assert _lib.describe_edge_softmax(11, int(rowptr[-1]), H)["W"] == 16
    _check_both(oracle, rowptr, H, 0.2 if H == 3 else None, 300 + H, "hubs")
    rowptr = _padded_hubs(L)
    d = _lib.describe_edge_softmax(rowptr.size - 1, int(rowptr[-1]), H)
    assert d == {"W": 8, "L": L}, d
    _check_both(oracle, rowptr, H, 0.2 if H == 1 else None, 310 + H, "hubs among short rows")


# ------------------------------------------------------------------------------------------------- 4. identity and determinism

@pytest.mark.parametrize("H", (2, 5, 8))
def test_head_is_the_single_head_call(pkg, oracle, edge, H):
    """Column h of the multi-head result has the bits of the call on score[:, h].contiguous(); two runs are equal. On the edge-case
    pattern (W = 16, both regimes) and on hub rows among short rows (W = 8 and the wavefront-per-pair branch)."""
    for rowptr in (edge["rowptr"], _padded_hubs(WANT_L)):
        nnz = int(rowptr[-1])
        rp = _dev(rowptr)
        s, g = _dev(_scores(oracle, nnz, H, 32.0, 41)), _dev(_scores(oracle, nnz, H, 4.0, 42))
        alpha = _fwd(rp, s, 0.2)
        grad = _bwd(rp, alpha, g, s, 0.2)
        _same(_fwd(rp, s, 0.2), alpha, "second run")
        _same(_bwd(rp, alpha, g, s, 0.2), grad, "second run, backward")
        for h in range(H):
            sh, gh = s[:, h].contiguous(), g[:, h].contiguous()
            ah = _fwd(rp, sh, 0.2)
            _same(ah, alpha[:, h], "forward head %d of %d" % (h, H))
            _same(_bwd(rp, ah, gh, sh, 0.2), grad[:, h], "backward head %d of %d" % (h, H))


def test_capture_equals_eager(pkg, oracle):
    """Forward and backward captured together on one stream; replays see operands edited in place and give the eager bits."""
    from gespmm_amd import softmax

    rowptr = _padded_hubs(WANT_L)
    nnz, H = int(rowptr[-1]), 3
    rp = _dev(rowptr)
    s, g = _dev(_scores(oracle, nnz, H, 32.0, 51)), _dev(_scores(oracle, nnz, H, 4.0, 52))
    buf_a, alpha = _out((nnz, H))
    buf_g, grad = _out((nnz, H))

    def step():
        softmax.edge_softmax(rp, s, out=alpha, negative_slope=0.2)
        softmax.edge_softmax_backward(rp, alpha, g, score=s, negative_slope=0.2, out=grad)

    graph, _ = _capture(step)
    for seed in (53, 55):
        s.copy_(_dev(_scores(oracle, nnz, H, 32.0, seed)))
        g.copy_(_dev(_scores(oracle, nnz, H, 4.0, seed + 1)))
        buf_a.fill_(NAN)
        buf_g.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        _guard_ok(buf_a, "replay")
        _guard_ok(buf_g, "replay")
        want_a = _fwd(rp, s, 0.2)
        _same(alpha, want_a, "replayed forward vs eager")
        _same(grad, _bwd(rp, want_a, g, s, 0.2), "replayed backward vs eager")


# -------------------------------------------------------------------------------------------------------------- 5. special values

def test_special_values(pkg):
    """Rows of 1 .. 70 entries (W = 16: the rows past 64 entries are swept, the others sit in registers), H = 3; every planted value
    sits in its own row, the rows around it must not notice."""
    degs = list(range(1, 71))
    rowptr = rowptr_of(degs)
    nnz, H = int(rowptr[-1]), 3
    rng = np.random.RandomState(9)
    s = (rng.rand(nnz, H).astype(np.float32) - np.float32(0.5)) * np.float32(8)
    lo = lambda d: int(rowptr[d - 1])  # noqa: E731  (first entry of the row of d entries)
    s[lo(10) + 3, 0] = -np.inf                      # one -inf among finite scores
    s[lo(20):lo(21), 1] = -np.inf                   # a (row, head) of -inf only
    s[lo(30) + 7, 2] = np.nan
    s[lo(66) + 65, 0] = np.inf
    s[lo(40):lo(41), 1] = -80.0                     # one score of 80 among -80s
    s[lo(40) + 11, 1] = 80.0
    s[lo(50):lo(51), 2] = 1.25                      # an all-equal row
    s[lo(69):lo(70), 0] = -3.0e38                   # equal and huge: x - max is 0, not inf - inf
    rp = _dev(rowptr)
    out = _fwd(rp, _dev(s)).cpu().numpy()
    a, tol = ref_forward(rowptr, s)
    want_nan = np.zeros((nnz, H), dtype=bool)
    want_nan[lo(20):lo(21), 1] = True
    want_nan[lo(30):lo(31), 2] = True
    want_nan[lo(66):lo(67), 0] = True
    assert np.array_equal(np.isnan(a), want_nan), "the float64 reference disagrees with the test's own NaN map"
    assert np.array_equal(np.isnan(out), want_nan), "NaN must fill exactly the poisoned (row, head) pairs"
    assert worst_ratio(out, a, tol) <= 1.0
    z = out[lo(10) + 3, 0]
    assert z == 0.0 and not np.signbit(z), "-inf must give exactly +0.0"
    hot = out[lo(40):lo(41), 1]
    assert hot[11] == 1.0 and np.all(np.delete(hot, 11) <= 2.0 ** -120) and np.all(np.delete(hot, 11) >= 0.0)
    assert np.all(np.abs(out[lo(50):lo(51), 2].astype(np.float64) - 1 / 50) <= tol[lo(50):lo(51), 2])
    assert out[0, 0] == 1.0 and out[0, 1] == 1.0 and out[0, 2] == 1.0
    # with a leaky ReLU in front: -inf stays -inf, NaN stays NaN (slope > 0), the map does not move
    out2 = _fwd(rp, _dev(s), 0.2).cpu().numpy()
    a2, tol2 = ref_forward(rowptr, s, 0.2)
    assert np.array_equal(np.isnan(out2), want_nan) and worst_ratio(out2, a2, tol2) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ 6. alignment

def _carve(t, off):
    """Same values, storage `off` bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0 and off % 4 == 0
    v = buf[off // 4:off // 4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off
    return v


def test_alignment(pkg, oracle, edge):
    """score, out and rowptr 4 bytes past a 16-byte boundary: the bits of the aligned call (nothing in the kernel is vectorised on an
    alignment assumption)."""
    from gespmm_amd import softmax

    G, H = edge, 5
    rp = _dev(G["rowptr"])
    s, g = _dev(_scores(oracle, G["nnz"], H, 32.0, 61)), _dev(_scores(oracle, G["nnz"], H, 4.0, 62))
    alpha = _fwd(rp, s, 0.2)
    grad = _bwd(rp, alpha, g, s, 0.2)
    rp4, s4, g4 = _carve(rp, 4), _carve(s, 4), _carve(g, 4)
    buf = torch.full((G["nnz"] * H + 1 + GUARD,), NAN, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out4 = buf[1:1 + G["nnz"] * H].view(G["nnz"], H)
    softmax.edge_softmax(rp4, s4, out=out4, negative_slope=0.2)
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-GUARD:]).all())
    _same(out4, alpha, "forward, carved")
    a4 = _carve(alpha, 4)
    buf.fill_(NAN)
    softmax.edge_softmax_backward(rp4, a4, g4, score=s4, negative_slope=0.2, out=out4)
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-GUARD:]).all())
    _same(out4, grad, "backward, carved")


# --------------------------------------------------------------------------------------------------------------------- 7. pubmed

def test_pubmed(pkg, oracle, bundled):
    from gespmm_amd import _lib

    G, H = bundled["pubmed"], 8
    rowptr = G["rowptr"]
    d = _lib.describe_edge_softmax(G["M"], G["nnz"], H)
    assert d == {"W": want_W(G["M"], G["nnz"]), "L": WANT_L} and d["W"] == 8
    assert np.diff(rowptr).max() > IT * d["W"], "pubmed has rows for the sweep regime"
    _check_both(oracle, rowptr, H, 0.2, 71, "pubmed")


# ---------------------------------------------------------------------------------------------------------------- 8. errors

def test_python_errors_raise_without_launching(pkg, oracle, edge):
    from gespmm_amd import softmax

    G, H = edge, 4
    nnz = G["nnz"]
    rp = _dev(G["rowptr"])
    s = _dev(_scores(oracle, nnz, H, 32.0, 81))
    fwd = lambda score, **kw: softmax.edge_softmax(rp, score, **kw)  # noqa: E731
    bwd = lambda a, g, **kw: softmax.edge_softmax_backward(rp, a, g, **kw)  # noqa: E731
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError):
            fwd(s.to(dt))
        with pytest.raises(TypeError):
            bwd(s.to(dt), s.to(dt))
        with pytest.raises(TypeError):
            bwd(s, s.to(dt))
        with pytest.raises(TypeError):
            bwd(s, s, score=s.to(dt), negative_slope=0.2)
        with pytest.raises(TypeError):
            fwd(s, out=torch.empty(nnz, H, device="cuda", dtype=dt))
    with pytest.raises(TypeError):
        softmax.edge_softmax(rp.long(), s)
    with pytest.raises(TypeError):
        fwd(s.cpu().numpy())
    for bad in (s.view(nnz, 2, 2), s.view(nnz, H, 1), torch.empty(nnz, 2 * H, device="cuda")[:, ::2], torch.empty(nnz, 0, device="cuda"),
                s.cpu()):
        with pytest.raises(ValueError):  # rank, contiguity, no heads, device
            fwd(bad)
        with pytest.raises(ValueError):
            bwd(bad, bad)
    for other in (torch.empty(nnz, H + 1, device="cuda"), torch.empty(nnz + 1, H, device="cuda"), torch.empty(nnz * H, device="cuda"),
                  torch.empty(nnz, H)):
        with pytest.raises(ValueError):  # shape or device mismatch between edge arrays
            fwd(s, out=other)
        with pytest.raises(ValueError):
            bwd(s, other)
        with pytest.raises(ValueError):
            bwd(s, s, score=other, negative_slope=0.2)
        with pytest.raises(ValueError):
            bwd(s, s, out=other)
    with pytest.raises(ValueError):
        softmax.edge_softmax(rp.cpu(), s)
    with pytest.raises(ValueError):
        softmax.edge_softmax(rp.view(-1, 2)[:, 0], s)
    with pytest.raises(ValueError):
        bwd(s, s, negative_slope=0.2)  # a slope needs the forward's input
    for slope in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            fwd(s, negative_slope=slope)


# ---------------------------------------------------------------------------------------------------------------- 9. autograd

@pytest.mark.parametrize("slope", (None, 0.2))
def test_autograd_function(pkg, oracle, edge, slope):
    """EdgeSoftmaxFunction against torch autograd through a float64 per-row restatement. The gradient's tolerance is the backward's own
    (float64 on the device's alpha) plus what the forward's tolerance on alpha can move it by:
    |g_e - dot| tol_f(e) + a_e sum_p tol_f(p) |g_p|, times the leaky factor."""
    import gespmm_amd

    G, H = edge, 3
    rowptr, nnz = G["rowptr"], G["nnz"]
    rp = _dev(rowptr)
    s_h, g_h = _scores(oracle, nnz, H, 32.0, 91), _scores(oracle, nnz, H, 4.0, 92)
    s = _dev(s_h).requires_grad_(True)
    alpha = gespmm_amd.EdgeSoftmaxFunction.apply(rp, s, slope)
    _same(alpha.detach(), _fwd(rp, s.detach(), slope), "forward")
    alpha.backward(_dev(g_h))
    assert rp.grad is None and s.grad.shape == (nnz, H)
    s64 = torch.from_numpy(s_h).double().requires_grad_(True)
    x64 = s64 if slope is None else torch.nn.functional.leaky_relu(s64, float(np.float32(slope)))
    parts = [torch.softmax(x64[int(rowptr[r]):int(rowptr[r + 1])], dim=0) for r in range(G["M"]) if rowptr[r + 1] > rowptr[r]]
    a64 = torch.cat(parts, dim=0)
    a64.backward(torch.from_numpy(g_h).double())
    ref = s64.grad.numpy()
    a, tol_f = ref_forward(rowptr, s_h, slope)
    _, tol_b = ref_backward(rowptr, a, g_h, s_h, slope)
    starts = rowptr[:-1][np.diff(rowptr) > 0]
    seg = np.repeat(np.arange(starts.size), np.diff(rowptr)[np.diff(rowptr) > 0])
    g64 = g_h.astype(np.float64)
    dot = np.add.reduceat(a * g64, starts, axis=0)[seg]
    k = np.ones_like(a) if slope is None else np.where(s_h >= 0, 1.0, float(np.float32(slope)))
    moved = (np.abs(g64 - dot) * tol_f + a * np.add.reduceat(tol_f * np.abs(g64), starts, axis=0)[seg]) * k
    r = worst_ratio(s.grad.cpu().numpy(), ref, tol_b + moved)
    print("autograd slope=%s: worst error / tolerance %.3f" % (slope, r))
    assert r <= 1.0
    # nothing is launched for a score that needs no gradient, and score is saved only with a slope
    s2 = _dev(s_h).requires_grad_(True)
    out = gespmm_amd.EdgeSoftmaxFunction.apply(rp, s2, slope)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == (1 if slope is None else 2)
