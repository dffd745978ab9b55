"""Dropout on the attention coefficients, host side (no GPU): the exported symbols, the mask's C++ definition against its known
answers and a numpy restatement, the threshold, the return-code ladders of the four entry points — the checks run before any device
work, so NULL or made-up device pointers are enough — the Python wrappers' argument checks, and the statistics of the restatement:
that the bits behave as independent coin flips over rows, columns, heads, the transposed entry and neighbouring seeds."""
import ctypes

import numpy as np
import pytest
import torch

from test_heads_host import EALIGN, EINVAL, ERANGE

NEW = ("gespmm_edge_dropout_f32", "gespmm_gat_aggregate_dropout_f32", "gespmm_gat_backward_el_dropout_f32",
       "gespmm_gat_backward_er_dropout_f32", "gespmm_edge_dropout_bits", "gespmm_edge_dropout_threshold")
OK = 0x1000  # a made-up address: the checks look at the number only and return before anything could read it
BIG = (1 << 31) - 4096  # one past the largest count of 32-bit word positions
SEED = (0x12345678, 0x9ABCDEF0)
KNOWN = (((0, 0, 0), 0xFFB6CD07), ((1, 5, 1), 0xF2651A06), ((2, 2, 7), 0x8CEE38F8), ((511, 300, 3), 0x75F57072))
BAD_P = (-0.1, 1.0, float("nan"))


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


def restate(s0, s1, r, c, h):
    """The issue's expression, written out here independently of the package's own restatement (which is held to this one below)."""
    def mix(x):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        return x ^ (x >> np.uint32(16))

    with np.errstate(over="ignore"):
        s0, s1, r, c, h = (np.asarray(v, dtype=np.uint64).astype(np.uint32) for v in (s0, s1, r, c, h))
        return mix(mix(mix(r ^ s0) ^ c) ^ (h * np.uint32(0x9E3779B9)) ^ s1)


def test_symbols_and_version(L):
    for name in NEW:
        assert name in L.EXPORTS
        getattr(L.lib, name)
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


def test_known_answers(L):
    from gespmm_amd import softmax

    for (r, c, h), want in KNOWN:
        assert L.edge_dropout_bits(SEED[0], SEED[1], r, c, h) == want, (r, c, h)
        assert int(restate(SEED[0], SEED[1], r, c, h)) == want, (r, c, h)
        assert int(softmax.restate_edge_dropout_bits(SEED[0], SEED[1], r, c, h)) == want, (r, c, h)


def test_bits_equal_the_numpy_restatement(L):
    from gespmm_amd import softmax

    rng = np.random.RandomState(5)
    n = 10000
    s0 = rng.randint(0, 1 << 32, size=n, dtype=np.uint64)
    s1 = rng.randint(0, 1 << 32, size=n, dtype=np.uint64)
    r = rng.randint(0, 1 << 31, size=n, dtype=np.uint64)
    c = rng.randint(0, 1 << 31, size=n, dtype=np.uint64)
    h = rng.randint(0, 64, size=n, dtype=np.uint64)
    # the corners: the largest indices and the two extreme seeds, alone and together
    r[:4], c[:4] = (1 << 31) - 1, ((1 << 31) - 1, 0, (1 << 31) - 1, 0)
    c[4:8] = (1 << 31) - 1
    s0[:16:2], s1[:16:4] = 0, 0
    s0[1:16:2], s1[2:16:4] = 0xFFFFFFFF, 0xFFFFFFFF
    s0[16:20], s1[16:20] = (0, 0, 0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF, 0, 0xFFFFFFFF)
    want = restate(s0, s1, r, c, h)
    assert np.array_equal(softmax.restate_edge_dropout_bits(s0, s1, r, c, h), want)
    got = np.array([L.edge_dropout_bits(int(a), int(b), int(i), int(j), int(k)) for a, b, i, j, k in zip(s0, s1, r, c, h)], dtype=np.uint32)
    assert np.array_equal(got, want), "the C++ definition differs from the restatement at %d of %d points" % (int((got != want).sum()), n)


def test_threshold(L):
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    for p in (0.0, 0.5, 0.6, below_one):
        want = min(int(np.floor(float(np.float32(p)) * 2.0 ** 32)), 2 ** 32 - 1)
        assert L.edge_dropout_threshold(p) == want, p
    assert L.edge_dropout_threshold(0.0) == 0 and L.edge_dropout_threshold(0.5) == 1 << 31
    assert L.edge_dropout_threshold(0.6) == 2576980480  # (float)0.6 = 0.60000002384185791015625
    assert L.edge_dropout_threshold(below_one) == 2 ** 32 - 256


# ------------------------------------------------------------------------------------------------------------- the error ladders

def test_edge_dropout_return_codes(L):
    """(rowptr, colind, x, y | M, K, H, nnz, p | seed, stream): the softmax's ladder with p in the slope's place, then the pointers."""
    f = L.lib.gespmm_edge_dropout_f32
    none = (None,) * 4
    assert f(*none, 4, 4, 0, 10, 0.5, None, None) == EINVAL        # H < 1
    assert f(*none, -1, 4, 2, 10, 0.5, None, None) == EINVAL
    assert f(*none, 4, 4, 2, -1, 0.5, None, None) == EINVAL
    assert f(*none, 4, 0, 2, 10, 0.5, None, None) == EINVAL        # K < 1
    assert f(*none, 0, 4, 2, 10, 0.5, None, None) == EINVAL        # entries without rows
    for p in BAD_P:
        assert f(*(_p(OK),) * 4, 4, 4, 2, 10, p, _p(OK), None) == EINVAL, p
        assert f(*none, 4, 4, 2, BIG, p, None, None) == EINVAL, p  # with what makes no sense: before what is too large
        assert f(*none, 4, 4, 2, 0, p, None, None) == EINVAL, p    # ... and before the early return of no entries
    assert f(*none, 4, 4, 2, BIG, 0.5, None, None) == ERANGE       # nnz H words
    assert f(*none, 4, 4, 2, 0, 0.5, None, None) == 0              # no entries: nothing to do, pointers not looked at
    assert f(*(_p(3),) * 4, 4, 4, 2, 0, 0.0, _p(3), None) == 0
    assert f(*none, 4, 4, 2, 10, 0.5, None, None) == EINVAL        # NULL where needed
    ptrs = lambda bad, v: [v if i == bad else _p(OK) for i in range(5)]  # noqa: E731  (the fifth: the seed)
    for bad in range(5):
        a = ptrs(bad, None)
        assert f(*a[:4], 4, 4, 2, 10, 0.5, a[4], None) == EINVAL, bad
        a = ptrs(bad, _p(OK + 2))
        assert f(*a[:4], 4, 4, 2, 10, 0.5, a[4], None) == EALIGN, bad
    assert f(None, *(_p(OK + 2),) * 3, 4, 4, 2, 10, 0.5, _p(OK + 2), None) == EINVAL  # NULL before alignment


def test_aggregate_dropout_return_codes(L):
    """gespmm_gat_aggregate_f32's ladder: (ptr, ind, el, er, stats, B, C | M, K, H, F, nnz, slope, transposed | p, seed, stream)."""
    f = L.lib.gespmm_gat_aggregate_dropout_f32
    base = L.lib.gespmm_gat_aggregate_f32
    none = (None,) * 7
    for t in (0, 1):
        assert f(*none, 4, 4, 0, 8, 10, 0.2, t, 0.5, None, None) == EINVAL       # H < 1
        assert f(*none, 4, 4, 2, -8, 10, 0.2, t, 0.5, None, None) == EINVAL
        assert f(*none, 4, 4, 2, 8, 10, float("nan"), t, 0.5, None, None) == EINVAL
        for p in BAD_P:
            assert f(*(_p(OK),) * 7, 4, 4, 2, 8, 10, 0.2, t, p, _p(OK), None) == EINVAL, p
            assert f(*none, 4, 4, 2, 8, BIG, 0.2, t, p, None, None) == EINVAL, p   # joins the bad slope: before what is too large
            assert f(*none, 4, 4, 2, 8, 0, 0.2, t, p, None, None) == EINVAL, p
        assert f(*none, 4, 4, 2, 8, BIG, 0.2, t, 0.5, None, None) == ERANGE
        assert f(*none, 4, 4, 8, 1 << 27, 10, 0.2, t, 0.5, None, None) == ERANGE
        assert f(*none, 4, 4, 2, 8, 10, 0.2, t, 0.5, None, None) == EINVAL       # NULL where needed
        for bad in range(8):  # the eighth: the seed
            a = [None if i == bad else _p(OK) for i in range(8)]
            assert f(*a[:7], 4, 4, 2, 8, 10, 0.2, t, 0.5, a[7], None) == EINVAL, bad
            a = [_p(OK + 2) if i == bad else _p(OK) for i in range(8)]
            assert f(*a[:7], 4, 4, 2, 8, 10, 0.2, t, 0.5, a[7], None) == EALIGN, bad
        a = [_p(OK + 4) if i == 4 else _p(OK) for i in range(7)]
        assert f(*a, 4, 4, 2, 8, 10, 0.2, t, 0.5, _p(OK), None) == EALIGN          # stats: 8-byte pairs
        # no entries: C and the seed alone are looked at (C is zero-filled, on a device)
        assert f(*none, 4, 4, 2, 8, 0, 0.2, t, 0.5, None, None) == EINVAL
        c_only = [None] * 6 + [_p(OK)]
        assert f(*c_only, 4, 4, 2, 8, 0, 0.2, t, 0.5, None, None) == EINVAL        # the seed is still asked for
        assert f(*c_only, 4, 4, 2, 8, 0, 0.2, t, 0.5, _p(OK + 2), None) == EALIGN
        assert f(*([None] * 6 + [_p(OK + 2)]), 4, 4, 2, 8, 0, 0.2, t, 0.5, _p(OK), None) == EALIGN
        # F == 0: nothing to write, as in the base entry
        assert f(*none, 4, 4, 2, 0, 10, 0.2, t, 0.5, None, None) == base(*none, 4, 4, 2, 0, 10, 0.2, t, None) == 0
    assert f(*none, 4, 4, 2, 8, 10, 0.2, 2, 0.5, None, None) == EINVAL           # transposed is 0 or 1


@pytest.mark.parametrize("which", ("el", "er"))
def test_backward_dropout_return_codes(L, which):
    """The ladder of tests/test_gat_backward_host.py with (p, seed) behind the slope: nine pointers, results at 7 and 8 (el) or 8 (er)."""
    f = getattr(L.lib, "gespmm_gat_backward_%s_dropout_f32" % which)
    results = (7, 8) if which == "el" else (8,)
    none = (None,) * 9
    assert f(*none, 4, 4, 0, 8, 10, 0.2, 0.5, None, None) == EINVAL
    assert f(*none, -1, 4, 2, 8, 10, 0.2, 0.5, None, None) == EINVAL
    assert f(*none, 4, 0, 2, 8, 10, 0.2, 0.5, None, None) == EINVAL
    assert f(*none, 4, 4, 2, 8, 10, float("inf"), 0.5, None, None) == EINVAL
    for p in BAD_P:
        assert f(*(_p(OK),) * 9, 4, 4, 2, 8, 10, 0.2, p, _p(OK), None) == EINVAL, p
        assert f(*none, 4, 4, 2, 8, BIG, 0.2, p, None, None) == EINVAL, p            # joins the bad slope: before what is too large
        assert f(*none, BIG // 16 + 1, 4, 2, 8, 10, 0.2, p, None, None) == EINVAL, p
        assert f(*none, 4, 4, 2, 8, 0, 0.2, p, None, None) == EINVAL, p
    assert f(*none, 4, 4, 2, 8, BIG, 0.2, 0.5, None, None) == ERANGE
    assert f(*none, BIG // 16 + 1, 4, 2, 8, 10, 0.2, 0.5, None, None) == ERANGE      # M H F words: grad_out
    assert f(*none, 4, BIG // 16 + 1, 2, 8, 10, 0.2, 0.5, None, None) == ERANGE
    assert f(*none, 4, 4, 2, 8, 10, 0.2, 0.5, None, None) == EINVAL                  # NULL where needed
    for bad in range(10):  # the tenth: the seed
        a = [None if i == bad else _p(OK) for i in range(10)]
        assert f(*a[:9], 4, 4, 2, 8, 10, 0.2, 0.5, a[9], None) == EINVAL, bad
        a = [_p(OK + 2) if i == bad else _p(OK) for i in range(10)]
        assert f(*a[:9], 4, 4, 2, 8, 10, 0.2, 0.5, a[9], None) == EALIGN, bad
    a = [_p(OK + 4) if i == 4 else _p(OK) for i in range(9)]
    assert f(*a, 4, 4, 2, 8, 10, 0.2, 0.5, _p(OK), None) == EALIGN                   # stats: 8-byte pairs
    assert f(None, *(_p(OK + 2),) * 8, 4, 4, 2, 8, 10, 0.2, 0.5, _p(OK + 2), None) == EINVAL  # NULL before alignment
    # no entries, or rows of no width: the results and the seed alone are looked at
    for F, nnz in ((8, 0), (0, 10)):
        assert f(*none, 4, 4, 2, F, nnz, 0.2, 0.5, None, None) == EINVAL
        args = [None] * 9
        for j in results:
            args[j] = _p(OK)
        assert f(*args, 4, 4, 2, F, nnz, 0.2, 0.5, None, None) == EINVAL             # the seed is still asked for
        assert f(*args, 4, 4, 2, F, nnz, 0.2, 0.5, _p(OK + 2), None) == EALIGN
        for i in results:
            bad = list(args)
            bad[i] = _p(OK + 2)
            assert f(*bad, 4, 4, 2, F, nnz, 0.2, 0.5, _p(OK), None) == EALIGN, (F, nnz, i)
    if which == "el":
        assert f(*none, 0, 4, 2, 8, 0, 0.2, 0.5, None, None) == 0                    # M == 0: nothing to write
        assert f(*(_p(3),) * 9, 0, 4, 2, 8, 0, 0.2, 0.0, _p(3), None) == 0


# ------------------------------------------------------------------------------------------------------------- the Python wrappers

def _operands(M=6, K=5, H=3, F=4, nnz=9):
    rp = torch.zeros(M + 1, dtype=torch.int32)
    rp[1:] = nnz
    cp = torch.zeros(K + 1, dtype=torch.int32)
    cp[1:] = nnz
    ind = torch.zeros(nnz, dtype=torch.int32)
    return {"rp": rp, "cp": cp, "ci": ind, "ri": ind.clone(), "el": torch.zeros(M, H), "er": torch.zeros(K, H), "stats": torch.ones(M, H, 2),
            "delta": torch.zeros(M, H), "gout": torch.zeros(M, H, F), "feat": torch.zeros(K, H, F), "x": torch.zeros(nnz, H),
            "seed": torch.zeros(2, dtype=torch.int32), "p": 0.5}


def test_python_wrappers_raise_before_any_launch(pkg):
    """TypeError for dtypes and non-tensors, ValueError for shapes, contiguity, devices and p. Every operand here lives on the host, so
    a call that got past its checks would raise the device ValueError — which the well-formed call at the end does."""
    from gespmm_amd import softmax, spmm

    o = _operands()

    def drop(**kw):
        a = dict(o, **kw)
        return softmax.edge_dropout(a["rp"], a["ci"], a["x"], a["p"], a["seed"], out=a.get("out"))

    def agg(**kw):
        a = dict(o, **kw)
        return spmm.gat_aggregate(a["rp"], a["ci"], a["el"], a["er"], a["stats"], a["feat"], negative_slope=0.2, dropout=(a["p"], a["seed"]))

    def el(**kw):
        a = dict(o, **kw)
        return softmax.gat_backward_el(a["rp"], a["ci"], a["el"], a["er"], a["stats"], a["gout"], a["feat"], negative_slope=0.2,
                                       dropout=(a["p"], a["seed"]))

    def er(**kw):
        a = dict(o, **kw)
        return softmax.gat_backward_er(a["cp"], a["ri"], a["el"], a["er"], a["stats"], a["delta"], a["gout"], a["feat"], negative_slope=0.2,
                                       dropout=(a["p"], a["seed"]))

    for call in (drop, agg, el, er):
        for seed in (o["seed"].long(), o["seed"].float(), o["seed"].to(torch.int16), [0, 0], (1, 2), None, 7):
            with pytest.raises(TypeError):
                call(seed=seed)
        with pytest.raises(TypeError):
            call(p=torch.tensor(0.5))
        with pytest.raises(TypeError):
            call(p="0.5")
        for seed in (torch.zeros(3, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)[::2],
                     torch.zeros((), dtype=torch.int32)):
            with pytest.raises(ValueError):
                call(seed=seed)
        for p in BAD_P + (1.5, float("inf")):
            with pytest.raises(ValueError):
                call(p=p)
        with pytest.raises(ValueError):
            call()  # well formed, but on the host: the device check is the last one standing
    for pair in (0.5, (0.5,), (0.5, o["seed"], 1), o["seed"]):  # no pair (p, seed)
        with pytest.raises(TypeError):
            spmm.gat_aggregate(o["rp"], o["ci"], o["el"], o["er"], o["stats"], o["feat"], dropout=pair)
        with pytest.raises(TypeError):
            softmax.gat_backward_el(o["rp"], o["ci"], o["el"], o["er"], o["stats"], o["gout"], o["feat"], dropout=pair)
        with pytest.raises(TypeError):
            softmax.gat_backward_er(o["cp"], o["ri"], o["el"], o["er"], o["stats"], o["delta"], o["gout"], o["feat"], dropout=pair)
    for dt in (torch.float16, torch.bfloat16, torch.float64, torch.int32):
        with pytest.raises(TypeError):
            drop(x=o["x"].to(dt))
    for name in ("rp", "ci"):
        with pytest.raises(TypeError):
            drop(**{name: o[name].long()})
    with pytest.raises(TypeError):
        drop(x=o["x"].numpy())
    for bad in ({"x": torch.zeros(9, 6)[:, ::2]}, {"x": torch.zeros(9, 3, 1)}, {"rp": o["rp"][::2]}, {"ci": o["ci"][:-1]},
                {"out": torch.zeros(9, 4)}):
        with pytest.raises(ValueError):
            drop(**bad)


def test_layer_and_function_arguments(pkg):
    from gespmm_amd import GATConv

    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            GATConv(4, 4, dropout=p)
    assert GATConv(4, 4).dropout == 0.0 and GATConv(4, 4, dropout=0.6, fused_backward=True).dropout == 0.6


# ---------------------------------------------------------------------------------------------------- statistics of the restatement

STAT_SEEDS = ((0, 0), (1, 0), (0, 1), SEED, (0xFFFFFFFF, 0xFFFFFFFF))
N_RC, N_H = 512, 8


def _mask(s0, s1, T):
    r = np.arange(N_RC, dtype=np.uint64)[:, None, None]
    c = np.arange(N_RC, dtype=np.uint64)[None, :, None]
    h = np.arange(N_H, dtype=np.uint64)[None, None, :]
    return restate(s0 & 0xFFFFFFFF, s1 & 0xFFFFFFFF, r, c, h) >= np.uint32(T)


def _corr_z(a, b, q):
    """Normalised correlation of two keep masks with keep probability q, as a z-score: sum of (a - q)(b - q) / (q (1 - q) sqrt(n))."""
    a, b = a.astype(np.float64) - q, b.astype(np.float64) - q
    return float((a * b).sum() / (q * (1.0 - q) * np.sqrt(a.size)))


@pytest.mark.parametrize("p", (0.1, 0.5, 0.6, 0.9))
def test_statistics_of_the_restatement(L, p):
    """Kept counts (whole grid, each row, each head) and correlations (neighbour in c, r, h; the transposed entry; the masks of seeds
    s0 + 1 and s1 + 1) as z-scores, every one below 5 in magnitude. About 10^4 scores over the four p: the expression's own worst on
    exactly these inputs is 3.94, what independent bits give; 5 is a condition that keeps a broken mix from passing."""
    T = L.edge_dropout_threshold(p)
    q = 1.0 - T / 2.0 ** 32  # the keep probability the threshold realises
    worst = 0.0
    for s0, s1 in STAT_SEEDS:
        m = _mask(s0, s1, T)
        sd = lambda n: np.sqrt(n * q * (1.0 - q))  # noqa: E731
        off = ~np.eye(N_RC, dtype=bool)[:, :, None].repeat(N_H, axis=2)  # (r, r) is its own transpose: the diagonal is left out
        scores = {"count": np.array([(m.sum() - m.size * q) / sd(m.size)]),
                  "count per row": (m.sum(axis=(1, 2)) - N_RC * N_H * q) / sd(N_RC * N_H),
                  "count per head": (m.sum(axis=(0, 1)) - N_RC * N_RC * q) / sd(N_RC * N_RC),
                  "next c": np.array([_corr_z(m[:, :-1], m[:, 1:], q)]),
                  "next r": np.array([_corr_z(m[:-1], m[1:], q)]),
                  "next h": np.array([_corr_z(m[:, :, :-1], m[:, :, 1:], q)]),
                  "transposed entry": np.array([_corr_z(m[off], m.transpose(1, 0, 2)[off], q)]),
                  "seed s0 + 1": np.array([_corr_z(m, _mask(s0 + 1, s1, T), q)]),
                  "seed s1 + 1": np.array([_corr_z(m, _mask(s0, s1 + 1, T), q)])}
        for what, z in scores.items():
            big = float(np.abs(z).max())
            worst = max(worst, big)
            assert big < 5.0, "p=%g seed=(%#x, %#x) %s: |z| = %.2f" % (p, s0, s1, what, big)
    print("p=%g: worst |z| %.2f" % (p, worst))
