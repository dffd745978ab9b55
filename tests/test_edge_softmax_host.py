"""Edge softmax, host side only (no GPU): the new symbols, the return codes of the three entry points before any device work, what
gespmm_describe_edge_softmax reports (resolve_edge_softmax, the function the launch itself runs) against the documented W / L rule
restated here, and a numpy restatement of the kernel's contract — fp32 lane chains, the xor butterfly, an fp32 exponential — held
against the float64 reference within the tolerances the GPU tests use, so that the tolerances themselves are under test here.

The float64 references and tolerance formulas (``ref_forward``, ``ref_backward``) and the restatement (``lanes_forward``,
``lanes_backward``) are shared with tests/test_gpu_edge_softmax.py."""
import ctypes

import numpy as np
import pytest

from helpers import edge_case_csr

EINVAL, EALIGN, ERANGE = -1, -2, -3
MAX_NNZ = 0x7FFFFFFF - 4096
NEW = ("gespmm_edge_softmax_f32", "gespmm_edge_softmax_backward_f32", "gespmm_describe_edge_softmax")
IT = 4  # entries a lane keeps in registers (select.h: kEdgeSoftmaxIT): rows of more than IT * W entries are swept
F32, F64 = np.float32, np.float64
U23, FLOOR = 2.0 ** -23, 2.0 ** -120


# ------------------------------------------------------------------------------------------------- the documented rule, by hand

def want_W(M, nnz):
    """Smallest power of two >= ceil(nnz / M), clamped to [4, 16] (the starting rule went to 64; the timing on products-sbm, mean degree
    50.5, put the upper end at 16: DESIGN 3.15)."""
    mean = -(-nnz // M)
    W = 4
    while W < 16 and W < mean:
        W *= 2
    return W


WANT_L = 2048


# ------------------------------------------------------------------------------------- float64 references and their tolerances

def _segments(rowptr):
    """(degree per row, start of every non-empty row, index of its non-empty row per entry, degree per entry)"""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    d = np.diff(rowptr)
    ne = d > 0
    starts = rowptr[:-1][ne]
    seg = np.repeat(np.arange(int(ne.sum())), d[ne])
    return d, starts, seg, np.repeat(d[ne], d[ne]).astype(F64)


def _slope64(slope):
    return None if slope is None else float(F32(slope))  # the value the kernel is handed


def ref_forward(rowptr, score, slope=None):
    """float64 softmax per (row, head) of the fp32 ``score`` [nnz, H] -> (a, tol):
    tol = a * 2^-23 * (2 |z_e| + 2 zbar + d + 8) + 2^-120,  z = x - max, zbar = sum_p a_p |z_p|.
    a is NaN exactly where float64 softmax of the row is (a NaN or +inf entry, a row of -inf only)."""
    s = np.asarray(score, dtype=F32).astype(F64)
    nnz = s.shape[0]
    s = s.reshape(nnz, -1)
    _, starts, seg, dd = _segments(rowptr)
    assert seg.shape[0] == nnz, "rowptr[M] must be nnz"
    k = _slope64(slope)
    with np.errstate(invalid="ignore", over="ignore"):
        x = s if k is None else np.where(s >= 0, s, s * k)
        m = np.maximum.reduceat(x, starts, axis=0)[seg]  # (np.maximum propagates NaN)
        z = x - m
        t = np.exp(z)
        a = t / np.add.reduceat(t, starts, axis=0)[seg]
        az = np.where(a > 0, a * np.abs(z), 0.0)
        zbar = np.add.reduceat(az, starts, axis=0)[seg]
        absz = np.where(a > 0, np.abs(z), 0.0)
        tol = a * U23 * (2 * absz + 2 * zbar + dd[:, None] + 8) + FLOOR
    return a, tol


def ref_backward(rowptr, alpha, grad_alpha, score=None, slope=None):
    """float64 on the device's own alpha -> (grad, tol): tol = 2^-23 (d + 4) a_e (|g_e| + sum_p |a_p g_p|) k + 2^-120."""
    a = np.asarray(alpha, dtype=F32).astype(F64)
    nnz = a.shape[0]
    a = a.reshape(nnz, -1)
    g = np.asarray(grad_alpha, dtype=F32).astype(F64).reshape(nnz, -1)
    _, starts, seg, dd = _segments(rowptr)
    k = np.ones_like(a)
    if slope is not None:
        k = np.where(np.asarray(score, dtype=F32).reshape(nnz, -1) >= 0, 1.0, _slope64(slope))
    dot = np.add.reduceat(a * g, starts, axis=0)[seg]
    scale = np.add.reduceat(np.abs(a * g), starts, axis=0)[seg]
    grad = a * (g - dot) * k
    tol = U23 * (dd[:, None] + 4) * np.abs(a) * (np.abs(g) + scale) * np.abs(k) + FLOOR
    return grad, tol


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over the entries where the reference is a number; NaN must sit exactly where the reference has it."""
    got = np.asarray(got, dtype=F64).reshape(ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN in %d places, the float64 reference has %d" % (int(np.isnan(got).sum()), int(nan.sum()))
    if nan.all():
        return 0.0
    return float((np.abs(got - ref)[~nan] / tol[~nan]).max())


# ----------------------------------------------------------------------------------- the contract, restated lane by lane in fp32

def _exp32(z, kind):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if kind == "exp":
            return np.exp(z.astype(F32))
        return np.exp2((F32(1.4426950408889634) * z.astype(F32)).astype(F32))  # exp2(fl(x log2 e)), the device's choice


def _butterfly(v, W, op):
    lane = np.arange(W)
    m = W >> 1
    while m > 0:
        v = op(v, v[lane ^ m])
        m >>= 1
    return v


def _leaky32(s, slope):
    if slope is None:
        return s
    with np.errstate(invalid="ignore"):
        return np.where(s >= 0, s, (F32(slope) * s).astype(F32)).astype(F32)


def _lane_view(v, W, fill):
    """[d, H] -> [T, W, H]: entry l + t W at [t, l], positions past the row's end hold ``fill``."""
    d, H = v.shape
    T = -(-d // W)
    pad = np.full((T * W, H), fill, dtype=F32)
    pad[:d] = v
    return pad.reshape(T, W, H)


def lanes_forward(rowptr, score, W, L=WANT_L, slope=None, exp="exp2"):
    score = np.asarray(score, dtype=F32)
    nnz = score.shape[0]
    s2 = score.reshape(nnz, -1)
    out = np.full_like(s2, np.nan)
    for r in range(len(rowptr) - 1):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        if hi <= lo:
            continue
        w = W if hi - lo <= L else 64
        x = _leaky32(s2[lo:hi], slope)
        xl = _lane_view(x, w, -np.inf)
        m = xl[0]
        for t in range(1, xl.shape[0]):
            m = np.fmax(m, xl[t])
        m = _butterfly(m, w, np.fmax)[0]  # (fmax: a NaN entry is ignored here and poisons the sum below instead)
        with np.errstate(invalid="ignore"):
            z = (x - m).astype(F32)
        t32 = _exp32(z, exp)
        tl = _lane_view(t32, w, 0.0)
        acc = np.zeros(tl.shape[1:], dtype=F32)
        for t in range(tl.shape[0]):
            acc = (acc + tl[t]).astype(F32)
        total = _butterfly(acc, w, lambda a, b: (a + b).astype(F32))[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[lo:hi] = (t32 / total).astype(F32)
    return out.reshape(score.shape)


def lanes_backward(rowptr, alpha, grad_alpha, W, L=WANT_L, score=None, slope=None):
    alpha = np.asarray(alpha, dtype=F32)
    nnz = alpha.shape[0]
    a2, g2 = alpha.reshape(nnz, -1), np.asarray(grad_alpha, dtype=F32).reshape(nnz, -1)
    out = np.full_like(a2, np.nan)
    for r in range(len(rowptr) - 1):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        if hi <= lo:
            continue
        w = W if hi - lo <= L else 64
        al, gl = _lane_view(a2[lo:hi], w, 0.0), _lane_view(g2[lo:hi], w, 0.0)
        acc = np.zeros(al.shape[1:], dtype=F32)
        for t in range(al.shape[0]):  # fmaf: the product of two fp32 numbers is exact in float64
            acc = (al[t].astype(F64) * gl[t].astype(F64) + acc.astype(F64)).astype(F32)
        dot = _butterfly(acc, w, lambda a, b: (a + b).astype(F32))[0]
        grad = (a2[lo:hi] * (g2[lo:hi] - dot).astype(F32)).astype(F32)
        if slope is not None:
            f = np.where(np.asarray(score, dtype=F32).reshape(nnz, -1)[lo:hi] >= 0, F32(1), F32(slope)).astype(F32)
            grad = (grad * f).astype(F32)
        out[lo:hi] = grad
    return out.reshape(alpha.shape)


def hub_degrees(L):
    return [0, 1, 2, 3, L - 1, L, L + 1, 0, 3 * L + 7, 5, 0]


def rowptr_of(degs):
    rp = np.zeros(len(degs) + 1, dtype=np.int32)
    rp[1:] = np.cumsum(degs)
    return rp


# --------------------------------------------------------------------------------------------------------------------- tests

def test_symbols_version_and_names(pkg):
    import os
    import re

    import gespmm_amd
    from gespmm_amd import _lib

    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "gespmm.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(_lib.lib, name) is not None, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.lib.gespmm_version().decode().startswith("gespmm 0.5 ")
    for name in ("softmax", "EdgeSoftmaxFunction", "GATConv"):
        assert name in gespmm_amd.__all__ and hasattr(gespmm_amd, name), name
    assert gespmm_amd.EdgeSoftmaxFunction is gespmm_amd.op.EdgeSoftmaxFunction and gespmm_amd.GATConv is gespmm_amd.op.GATConv
    assert callable(gespmm_amd.softmax.edge_softmax) and callable(gespmm_amd.softmax.edge_softmax_backward)
    assert callable(_lib.describe_edge_softmax)


def test_return_codes_need_no_gpu(pkg):
    """Sizes that make no sense, range, nnz == 0, NULL, alignment — in that order, all before any device work."""
    from gespmm_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    half = ctypes.c_void_p(p.value + 2)
    made_up = ctypes.c_void_p(0x1000)
    nan, inf = float("nan"), float("inf")

    def fwd(rp, s, o, M, H, nnz, slope=1.0):
        return lib.gespmm_edge_softmax_f32(rp, s, o, M, H, nnz, slope, None)

    def bwd(rp, a, g, s, o, M, H, nnz, slope=1.0):
        return lib.gespmm_edge_softmax_backward_f32(rp, a, g, s, o, M, H, nnz, slope, None)

    # sizes that make no sense — whatever the pointers are, and before sizes that are too large
    for M, H, nnz, slope in ((4, 0, 8, 1.0), (4, -1, 8, 1.0), (-1, 2, 8, 1.0), (4, 2, -8, 1.0), (4, 2, 8, nan), (4, 2, 8, inf), (4, 2, 8, -inf),
                             (0, 2, 8, 1.0), (4, 0, MAX_NNZ + 1, 1.0), (1 << 31, 2, 8, nan)):
        assert fwd(p, p, p, M, H, nnz, slope) == EINVAL, (M, H, nnz, slope)
        assert fwd(None, half, None, M, H, nnz, slope) == EINVAL
        assert bwd(p, p, p, p, p, M, H, nnz, slope) == EINVAL, (M, H, nnz, slope)
        assert bwd(None, half, None, None, half, M, H, nnz, slope) == EINVAL
    # range: M, nnz, and the word count nnz H (no composition route)
    for M, H, nnz in ((1 << 31, 2, 8), (MAX_NNZ + 1, 1, 8), (4, 1, MAX_NNZ + 1), (4, 2, MAX_NNZ // 2 + 1), (4, 1 << 31, 1), (4, 1 << 40, 0),
                      (4, 3, 1 << 40)):
        assert fwd(None, p, p, M, H, nnz) == ERANGE and bwd(None, p, p, None, p, M, H, nnz, 0.2) == ERANGE, (M, H, nnz)
    assert fwd(None, p, p, 4, 2, MAX_NNZ // 2) == EINVAL  # at the limit the sizes pass: the NULL is seen
    assert fwd(None, p, p, MAX_NNZ, 1, 8) == EINVAL
    # no entries: 0 without looking at pointers
    assert fwd(half, made_up, None, 4, 3, 0) == 0 and fwd(None, None, None, 0, 3, 0) == 0
    assert bwd(half, None, made_up, half, None, 4, 3, 0, 0.2) == 0 and bwd(None, None, None, None, None, 0, 1, 0) == 0
    # NULL, then alignment
    for bad in range(3):
        args = [p] * 3
        args[bad] = None
        assert fwd(*args, 4, 3, 8) == EINVAL, bad
        args[bad] = half
        assert fwd(*args, 4, 3, 8) == EALIGN, bad
        args = [made_up] * 3
        args[bad] = ctypes.c_void_p(0x1002)
        assert fwd(*args, 4, 3, 8, 0.2) == EALIGN, bad
        args[(bad + 1) % 3] = None  # NULL is reported before a misaligned pointer
        assert fwd(*args, 4, 3, 8, 0.2) == EINVAL, bad
    for slope in (1.0, 0.2):
        needed = (0, 1, 2, 4) if slope == 1.0 else (0, 1, 2, 3, 4)
        for bad in needed:
            args = [p] * 5
            args[bad] = None
            assert bwd(*args, 4, 3, 8, slope) == EINVAL, (slope, bad)
            args[bad] = half
            assert bwd(*args, 4, 3, 8, slope) == EALIGN, (slope, bad)
            args[(bad + 1) % 5 if (bad + 1) % 5 in needed else 0] = None
            assert bwd(*args, 4, 3, 8, slope) == EINVAL, (slope, bad)


def test_describe_table(pkg):
    from gespmm_amd import _lib

    seen = set()
    for M, nnz in ((1000, 2500), (1000, 5000), (1000, 12000), (1000, 30000), (1000, 60000), (1000, 200000), (21, 890)):
        answers = set()
        for H in (1, 3, 8, 33):
            d = _lib.describe_edge_softmax(M, nnz, H)
            assert d == {"W": want_W(M, nnz), "L": WANT_L}, (M, nnz, H, d)
            answers.add(tuple(sorted(d.items())))
            seen.add(d["W"])
        assert len(answers) == 1, "W or L depends on H"
    assert seen == {4, 8, 16}
    assert [want_W(1000, n) for n in (2500, 5000, 12000, 30000, 60000, 200000)] == [4, 8, 16, 16, 16, 16] and want_W(21, 890) == 16
    # the power-of-two boundaries: mean degree exactly W stays at W, one entry more doubles it — up to 16
    for W in (4, 8, 16, 32):
        assert _lib.describe_edge_softmax(1000, 1000 * W, 2)["W"] == min(W, 16)
        assert _lib.describe_edge_softmax(1000, 1000 * W + 1, 2)["W"] == min(2 * W, 16)
    assert _lib.describe_edge_softmax(1000, 1, 2)["W"] == 4


def test_describe_arguments(pkg):
    from gespmm_amd import _lib

    f = _lib.lib.gespmm_describe_edge_softmax
    buf = ctypes.create_string_buffer(64)
    # f(M, nnz, H, out, capacity)
    assert f(10, 20, 2, None, 64) == EINVAL and f(10, 20, 2, buf, 0) == EINVAL and f(10, 20, 2, buf, -1) == EINVAL
    for M, nnz, H in ((-1, 20, 2), (10, -1, 2), (10, 20, 0), (10, 20, -3), (0, 20, 2)):
        assert f(M, nnz, H, buf, 64) == EINVAL, (M, nnz, H)
    for M, nnz, H in ((1 << 31, 20, 2), (10, MAX_NNZ + 1, 1), (10, MAX_NNZ // 2 + 1, 2), (10, 20, 1 << 31)):
        assert f(M, nnz, H, buf, 64) == ERANGE, (M, nnz, H)
    want = b"W=8 long_rows>2048"
    assert f(1000, 5000, 8, buf, 64) == len(want) and buf.value == want
    assert f(10, MAX_NNZ // 2, 2, buf, 64) == len(b"W=16 long_rows>2048") and buf.value == b"W=16 long_rows>2048"
    small = ctypes.create_string_buffer(8)
    assert f(1000, 5000, 8, small, 8) == 7 and small.value == b"W=8 lon"  # truncated, NUL-terminated
    assert f(1000, 0, 8, buf, 64) == len(b"form=none") and buf.value == b"form=none"
    assert _lib.describe_edge_softmax(1000, 0, 8) == {"form": "none"} and _lib.describe_edge_softmax(0, 0, 1) == {"form": "none"}
    with pytest.raises(_lib.GespmmError):
        _lib.describe_edge_softmax(10, 20, 0)


def _scores(oracle, nnz, H, scale, seed):
    return (F32(scale) * oracle.hash_val(nnz * H, seed=seed)).reshape(nnz, H)


@pytest.mark.parametrize("exp", ("exp", "exp2"))
@pytest.mark.parametrize("slope", (None, 0.2))
def test_restatement_within_tolerance_edge_cases(oracle, exp, slope):
    """The edge-case pattern (degrees 0 .. 200) at the W the rule gives it, at a smaller W, where rows span many lane steps, and at the
    whole wavefront of a hub row; scores within +-16 and +-100."""
    G = edge_case_csr()
    rp, nnz = G["rowptr"], G["nnz"]
    assert want_W(G["M"], nnz) == 16
    worst_f = worst_b = 0.0
    for W in (4, 16, 64):
        for H, scale in ((1, 32.0), (3, 32.0), (8, 200.0)):
            s = _scores(oracle, nnz, H, scale, seed=11 + H)
            a, tol = ref_forward(rp, s, slope)
            got = lanes_forward(rp, s, W, slope=slope, exp=exp)
            worst_f = max(worst_f, worst_ratio(got, a, tol))
            g = _scores(oracle, nnz, H, 4.0, seed=23 + H)
            gref, gtol = ref_backward(rp, got, g, s, slope)
            worst_b = max(worst_b, worst_ratio(lanes_backward(rp, got, g, W, score=s, slope=slope), gref, gtol))
            one = (np.diff(rp) == 1).nonzero()[0]
            assert np.all(got[rp[one]] == 1.0), "a single-entry row must be exactly 1"
    print("worst error / tolerance: forward %.3f backward %.3f" % (worst_f, worst_b))
    assert worst_f <= 1.0 and worst_b <= 1.0


@pytest.mark.parametrize("exp", ("exp", "exp2"))
def test_restatement_within_tolerance_long_rows(oracle, exp):
    """The hub pattern of the GPU test: rows of L - 1, L, L + 1 and 3 L + 7 entries — the longest summation chains the tolerance's
    d term has to cover — folded by 4 lanes up to L and by 64 beyond."""
    rp = rowptr_of(hub_degrees(WANT_L))
    nnz = int(rp[-1])
    worst_f = worst_b = 0.0
    for H, scale, slope in ((1, 32.0, None), (3, 32.0, 0.2)):
        s = _scores(oracle, nnz, H, scale, seed=31 + H)
        a, tol = ref_forward(rp, s, slope)
        got = lanes_forward(rp, s, 4, slope=slope, exp=exp)
        worst_f = max(worst_f, worst_ratio(got, a, tol))
        g = _scores(oracle, nnz, H, 4.0, seed=37 + H)
        gref, gtol = ref_backward(rp, got, g, s, slope)
        worst_b = max(worst_b, worst_ratio(lanes_backward(rp, got, g, 4, score=s, slope=slope), gref, gtol))
    print("worst error / tolerance: forward %.3f backward %.3f" % (worst_f, worst_b))
    assert worst_f <= 1.0 and worst_b <= 1.0


def test_restatement_special_values():
    """What the GPU test asks of the device, asked of the restatement: -inf -> +0, an all -inf row -> NaN, NaN / +inf poison their own
    (row, head) only, and the float64 reference has NaN in the same places."""
    rp = rowptr_of([3, 5, 1, 4, 70])
    nnz, H = int(rp[-1]), 2
    s = np.linspace(-3, 3, nnz * H, dtype=F32).reshape(nnz, H)
    s[1, 0] = -np.inf           # row 0 head 0: one -inf among finite scores
    s[3:8, 1] = -np.inf         # row 1 head 1: -inf only
    s[9, 0] = np.nan            # row 3 head 0
    s[20, 1] = np.inf           # row 4 head 1
    for exp in ("exp", "exp2"):
        got = lanes_forward(rp, s, 4, exp=exp)
        a, tol = ref_forward(rp, s)
        assert worst_ratio(got, a, tol) <= 1.0
        assert got[1, 0] == 0.0 and not np.signbit(got[1, 0])
        assert np.isnan(got[3:8, 1]).all() and not np.isnan(got[3:8, 0]).any()
        assert np.isnan(got[9:13, 0]).all() and not np.isnan(got[9:13, 1]).any()
        assert np.isnan(got[13:, 1]).all() and not np.isnan(got[13:, 0]).any()
        assert got[8, 0] == 1.0 and got[8, 1] == 1.0
