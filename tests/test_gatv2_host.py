"""GATv2 edge score, host side (no GPU): the exported symbols, the return-code ladders of gespmm_gatv2_score_f32 and
gespmm_gatv2_score_backward_f32 — the checks run before any device work, so NULL or made-up device pointers are enough, and every
call here keeps at least one pointer bad so that nothing could be launched — the forward's launch shape through
gespmm_describe_gatv2_score, the Python wrappers' argument checks (host tensors reach every one of them but the last), and the
numpy / float64 restatement of forward and backward that tests/test_gpu_gatv2_score.py holds the kernels to."""
import ctypes

import numpy as np
import pytest
import torch

from test_heads_host import EALIGN, EINVAL, ERANGE

NEW = ("gespmm_gatv2_score_f32", "gespmm_gatv2_score_backward_f32", "gespmm_describe_gatv2_score")
OK = 0x1000  # a made-up address: the checks look at the number only and return before anything could read it
BIG = (1 << 31) - 4096  # one past the largest count of 32-bit word positions
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------- the restatement

def restate_score(rowptr, colind, xl, xr, att, negative_slope=None):
    """sddmm.gatv2_score in float64 on host arrays -> (score f64[nnz, H], terms f64[nnz, H]), terms = sum_f |att leaky|: what the
    bound 1e-4 max(|ref|, terms) is made of. The branch is ``t >= 0`` on the fp32 sum, whose sign is that of the exact sum."""
    slope = 1.0 if negative_slope is None else float(negative_slope)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    cols = np.asarray(colind)
    nnz, (H, F) = cols.size, att.shape
    score, terms = np.zeros((nnz, H)), np.zeros((nnz, H))
    fc = max(1, (1 << 22) // max(1, nnz * H))  # columns per chunk: the [nnz, H, fc] temporaries stay small
    with np.errstate(invalid="ignore", over="ignore"):
        for f0 in range(0, F, fc):
            a, b = xl[:, :, f0:f0 + fc], xr[:, :, f0:f0 + fc]
            pos = (a.astype(F32)[rows] + b.astype(F32)[cols]) >= 0
            t = a.astype(F64)[rows] + b.astype(F64)[cols]
            prod = att[None, :, f0:f0 + fc].astype(F64) * np.where(pos, t, t * slope)
            score += prod.sum(-1)
            terms += np.abs(prod).sum(-1)
    return score, terms


def restate_backward(ptr, ind, grad_score, x_seg, x_ind, att, negative_slope=None, order=None):
    """sddmm.gatv2_score_backward in float64 on host arrays -> (grad_x, att_part, terms_x, terms_a), all f64[S, H, F]; the terms are
    the sums of |grad_score m| and |grad_score leaky|. m on the negative side is fl(att slope), the fp32 product the contract names.
    An empty segment is exactly +0."""
    slope = 1.0 if negative_slope is None else float(negative_slope)
    ptr = np.asarray(ptr, dtype=np.int64)
    S, d = ptr.size - 1, np.diff(ptr)
    seg = np.repeat(np.arange(S), d)
    ind = np.asarray(ind)
    nnz, (H, F) = ind.size, att.shape
    q = np.arange(nnz) if order is None else np.asarray(order)
    g = grad_score.astype(F64)[q][:, :, None]
    nonempty = d > 0
    starts = ptr[:-1][nonempty]  # entries of a segment are consecutive: one reduceat per chunk
    out = [np.zeros((S, H, F)) for _ in range(4)]
    fc = max(1, (1 << 22) // max(1, nnz * H))
    with np.errstate(invalid="ignore", over="ignore"):
        for f0 in range(0, F, fc):
            a, b = x_seg[:, :, f0:f0 + fc], x_ind[:, :, f0:f0 + fc]
            pos = (a.astype(F32)[seg] + b.astype(F32)[ind]) >= 0
            t = a.astype(F64)[seg] + b.astype(F64)[ind]
            w = att[None, :, f0:f0 + fc].astype(F32)
            gx = g * np.where(pos, w.astype(F64), (w * F32(slope)).astype(F64))
            ga = g * np.where(pos, t, t * slope)
            if starts.size:
                for o, v in zip(out, (gx, ga, np.abs(gx), np.abs(ga))):
                    o[nonempty, :, f0:f0 + fc] = np.add.reduceat(v, starts, axis=0) + 0.0  # (a chain from +0 never ends in -0)
    return tuple(out)


def worst_ratio(got, ref, terms, what=""):
    """max |got - ref| / (1e-4 max(|ref|, terms)) where the bound is positive; where it is zero got must equal ref."""
    got = np.asarray(got, dtype=F64).reshape(ref.shape)
    bound = 1e-4 * np.maximum(np.abs(ref), terms)
    err = np.abs(got - ref)
    zero = bound == 0
    assert np.all(err[zero] == 0), "%s: a sum of no terms (or of zeros) must be exact" % what
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# --------------------------------------------------------------------------------------------------------------------- tests

@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_and_version(L, pkg):
    for name in NEW:
        assert name in L.EXPORTS
        getattr(L.lib, name)
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")
    for name in ("GATv2ScoreFunction", "GATv2Conv"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert callable(pkg.sddmm.gatv2_score) and callable(pkg.sddmm.gatv2_score_backward) and callable(L.describe_gatv2_score)


def test_forward_return_codes(L):
    """(rowptr, colind, xl, xr, att, score | M, K, H, F, nnz, slope, stream): sizes that make no sense, sizes too large, nnz == 0,
    F == 0, then the pointers (NULL, alignment) — in that order."""
    f = L.lib.gespmm_gatv2_score_f32
    none = (None,) * 6
    assert f(*none, 4, 4, 0, 8, 10, 0.2, None) == EINVAL        # H < 1
    assert f(*none, -1, 4, 2, 8, 10, 0.2, None) == EINVAL       # negative sizes
    assert f(*none, 4, -4, 2, 8, 0, 0.2, None) == EINVAL
    assert f(*none, 4, 4, 2, -8, 10, 0.2, None) == EINVAL
    assert f(*none, 4, 4, 2, 8, -1, 0.2, None) == EINVAL
    assert f(*none, 4, 0, 2, 8, 10, 0.2, None) == EINVAL        # K < 1 with entries
    assert f(*none, 0, 4, 2, 8, 10, 0.2, None) == EINVAL        # entries without rows
    assert f(*none, 4, 4, 2, 8, 10, float("inf"), None) == EINVAL
    assert f(*none, 4, 4, 2, 8, 10, float("nan"), None) == EINVAL
    assert f(*none, 4, 4, 0, 8, BIG, 0.2, None) == EINVAL       # what makes no sense before what is too large
    assert f(*none, 4, 4, 2, 8, BIG, float("nan"), None) == EINVAL
    assert f(*none, 4, 4, 1, 8, BIG, 0.2, None) == ERANGE       # nnz
    assert f(*none, 4, 4, 2, 8, BIG // 2 + 1, 0.2, None) == ERANGE    # nnz H words
    assert f(*none, BIG, 4, 1, 1, 10, 0.2, None) == ERANGE      # M
    assert f(*none, BIG // 16 + 1, 4, 2, 8, 10, 0.2, None) == ERANGE  # M H F words
    assert f(*none, 4, BIG // 16 + 1, 2, 8, 10, 0.2, None) == ERANGE  # K H F words
    assert f(*none, 4, 4, 1 << 30, 4, 10, 0.2, None) == ERANGE
    assert f(*none, 4, 4, 8, 1 << 30, 10, 0.2, None) == ERANGE
    assert f(*none, BIG, 4, 1, 1, 0, 0.2, None) == ERANGE       # too large comes before "no entries"
    assert f(*none, (BIG - 1) // 16, (BIG - 1) // 16, 2, 8, 10, 0.2, None) == EINVAL  # the largest that fit: on to the pointers
    # no entries: success without a pointer being looked at
    assert f(*none, 4, 4, 2, 8, 0, 0.2, None) == 0
    assert f(*(_p(3),) * 6, 4, 4, 2, 8, 0, 0.2, None) == 0
    assert f(*none, 0, 0, 2, 8, 0, 0.2, None) == 0
    # rows of no width: score alone is looked at (and zero-filled, on a device)
    assert f(*none, 4, 4, 2, 0, 10, 0.2, None) == EINVAL
    assert f(*(None,) * 5, _p(OK + 2), 4, 4, 2, 0, 10, 0.2, None) == EALIGN
    assert f(*(_p(3),) * 5, _p(OK + 2), 4, 4, 2, 0, 10, 0.2, None) == EALIGN
    # the pointers
    assert f(*none, 4, 4, 2, 8, 10, 0.2, None) == EINVAL
    for bad in range(6):
        assert f(*[None if i == bad else _p(OK) for i in range(6)], 4, 4, 2, 8, 10, 0.2, None) == EINVAL, bad
        assert f(*[_p(OK + 2) if i == bad else _p(OK) for i in range(6)], 4, 4, 2, 8, 10, 0.2, None) == EALIGN, bad
    assert f(*[None if i == 0 else _p(OK + 2) for i in range(6)], 4, 4, 2, 8, 10, 0.2, None) == EINVAL  # NULL before alignment


def test_backward_return_codes(L):
    """(ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part | S, T, H, F, nnz, slope, stream); order (2) and att_part (8)
    may be NULL. nnz == 0 or F == 0 looks at the results alone."""
    f = L.lib.gespmm_gatv2_score_backward_f32
    none = (None,) * 9
    optional = (2, 8)
    assert f(*none, 4, 4, 0, 8, 10, 0.2, None) == EINVAL
    assert f(*none, -1, 4, 2, 8, 10, 0.2, None) == EINVAL
    assert f(*none, 4, -1, 2, 8, 0, 0.2, None) == EINVAL
    assert f(*none, 4, 4, 2, -8, 10, 0.2, None) == EINVAL
    assert f(*none, 4, 4, 2, 8, -1, 0.2, None) == EINVAL
    assert f(*none, 4, 0, 2, 8, 10, 0.2, None) == EINVAL
    assert f(*none, 0, 4, 2, 8, 10, 0.2, None) == EINVAL
    assert f(*none, 4, 4, 2, 8, 10, float("-inf"), None) == EINVAL
    assert f(*none, 4, 4, 2, 8, 10, float("nan"), None) == EINVAL
    assert f(*none, 4, 4, 0, 8, BIG, 0.2, None) == EINVAL
    assert f(*none, 4, 4, 1, 8, BIG, 0.2, None) == ERANGE
    assert f(*none, 4, 4, 2, 8, BIG // 2 + 1, 0.2, None) == ERANGE
    assert f(*none, BIG, 4, 1, 1, 10, 0.2, None) == ERANGE
    assert f(*none, BIG // 16 + 1, 4, 2, 8, 10, 0.2, None) == ERANGE
    assert f(*none, 4, BIG // 16 + 1, 2, 8, 10, 0.2, None) == ERANGE
    assert f(*none, BIG // 16 + 1, 4, 2, 8, 0, 0.2, None) == ERANGE   # too large comes before "no entries"
    assert f(*none, (BIG - 1) // 16, (BIG - 1) // 16, 2, 8, 10, 0.2, None) == EINVAL
    # no entries, or rows of no width: the results alone are looked at (and zero-filled, on a device)
    for F, nnz in ((8, 0), (0, 10)):
        assert f(*none, 4, 4, 2, F, nnz, 0.2, None) == EINVAL                                            # grad_x is needed
        assert f(*(None,) * 7, _p(OK + 2), None, 4, 4, 2, F, nnz, 0.2, None) == EALIGN
        assert f(*(None,) * 7, _p(OK), _p(OK + 2), 4, 4, 2, F, nnz, 0.2, None) == EALIGN                   # att_part, where given
        assert f(*(_p(3),) * 7, None, _p(OK), 4, 4, 2, F, nnz, 0.2, None) == EINVAL
    assert f(*(None,) * 7, _p(OK), None, 0, 0, 2, 8, 0, 0.2, None) == 0      # nothing to write
    assert f(*(None,) * 7, _p(OK), _p(OK), 4, 4, 2, 0, 10, 0.2, None) == 0   # F == 0: results of no words
    # the pointers
    assert f(*none, 4, 4, 2, 8, 10, 0.2, None) == EINVAL
    for bad in range(9):
        if bad not in optional:
            assert f(*[None if i == bad else _p(OK) for i in range(9)], 4, 4, 2, 8, 10, 0.2, None) == EINVAL, bad
        assert f(*[_p(OK + 2) if i == bad else _p(OK) for i in range(9)], 4, 4, 2, 8, 10, 0.2, None) == EALIGN, bad
    assert f(*[None if i == 0 else _p(OK + 2) for i in range(9)], 4, 4, 2, 8, 10, 0.2, None) == EINVAL  # NULL before alignment
    assert f(*[None if i in optional else _p(OK + 2) for i in range(9)], 4, 4, 2, 8, 10, 0.2, None) == EALIGN


# (F, xl_align, xr_align, att_align) -> (V, W): resolve_sddmm's width and alignment rule at width F on THREE addresses
SHAPES = (
    ((1, 16, 16, 16), (1, 4)), ((5, 16, 16, 16), (1, 4)), ((27, 16, 16, 16), (1, 4)), ((33, 16, 16, 16), (1, 8)),      # F odd
    ((65, 16, 16, 16), (1, 16)), ((129, 16, 16, 16), (1, 32)), ((257, 16, 16, 16), (1, 64)), ((1025, 16, 16, 16), (1, 64)),
    ((2, 16, 16, 16), (2, 4)), ((6, 16, 16, 16), (2, 4)), ((34, 16, 16, 16), (2, 8)), ((66, 16, 16, 16), (2, 16)),     # F = 2 mod 4
    ((130, 16, 16, 16), (2, 32)), ((258, 16, 16, 16), (2, 64)),
    ((8, 16, 16, 16), (4, 4)), ((16, 16, 16, 16), (4, 4)), ((32, 16, 16, 16), (4, 4)), ((40, 16, 16, 16), (4, 8)),     # F = 0 mod 4
    ((64, 16, 16, 16), (4, 8)), ((128, 16, 16, 16), (4, 16)), ((256, 16, 16, 16), (4, 32)), ((512, 16, 16, 16), (4, 64)),
    ((1028, 16, 16, 16), (4, 64)),
    ((8, 8, 16, 16), (2, 4)), ((8, 16, 8, 16), (2, 4)), ((8, 4, 16, 16), (1, 4)), ((8, 16, 4, 16), (1, 4)),            # carved xl / xr
    ((8, 16, 16, 8), (2, 4)), ((8, 16, 16, 4), (1, 4)), ((8, 8, 8, 4), (1, 4)), ((64, 16, 16, 8), (2, 8)),             # att less aligned
    ((64, 16, 16, 4), (1, 8)), ((6, 16, 16, 4), (1, 4)), ((6, 8, 8, 8), (2, 4)), ((5, 4, 8, 4), (1, 4)),
    ((8, 32, 64, 256), (4, 4)),                                                                                          # 16 is as good as more
)


@pytest.mark.parametrize("shape,want", SHAPES)
def test_describe(L, shape, want):
    F, a1, a2, a3 = shape
    for M, nnz, H in ((100, 1000, 8), (100000, 5000000, 1)):
        d = L.describe_gatv2_score(M, nnz, H, F, a1, a2, a3)
        assert (d["V"], d["W"]) == want, (shape, d)
        assert F % d["V"] == 0 and min(a1, a2, a3, 16) % (4 * d["V"]) == 0 and 1 <= d["epw"] <= 256


def test_describe_edges(L):
    assert L.describe_gatv2_score(10, 0, 2, 8) == {"form": "none"}
    assert L.describe_gatv2_score(10, 5, 2, 0) == {"route": "zeros"}
    # entries per wavefront: the pair thresholds of the multi-head SDDMM's CSR kernel (carried over), in whole entries
    assert L.describe_gatv2_score(1000, 10000, 8, 8)["epw"] == 8       # 64 pairs (G * 4) / 8 heads
    assert L.describe_gatv2_score(1000, 64 * 16384 // 8, 8, 8)["epw"] == 8
    assert L.describe_gatv2_score(1000, 256 * 16384 // 8, 8, 8)["epw"] == 32
    assert L.describe_gatv2_score(1000, 256 * 16384, 1, 8)["epw"] == 256
    assert L.describe_gatv2_score(1000, 10000, 300, 8)["epw"] == 1
    for bad in ((10, 5, 0, 8), (10, -1, 2, 8), (0, 5, 2, 8), (10, 5, 2, -1)):
        with pytest.raises(L.GespmmError) as e:
            L.describe_gatv2_score(*bad)
        assert e.value.code == EINVAL
    with pytest.raises(L.GespmmError) as e:
        L.describe_gatv2_score(10, BIG, 1, 8)
    assert e.value.code == ERANGE
    for al in ((2, 16, 16), (16, 12, 16), (16, 16, 0)):
        with pytest.raises(L.GespmmError) as e:
            L.describe_gatv2_score(10, 5, 2, 8, *al)
        assert e.value.code == EINVAL


def _operands(M=6, K=5, H=3, F=4, nnz=9):
    rp = torch.zeros(M + 1, dtype=torch.int32)
    rp[1:] = nnz
    ind = torch.zeros(nnz, dtype=torch.int32)
    return {"rp": rp, "ci": ind, "xl": torch.zeros(M, H, F), "xr": torch.zeros(K, H, F), "att": torch.zeros(H, F),
            "gs": torch.zeros(nnz, H), "order": torch.arange(nnz, dtype=torch.int32)}


def test_python_wrappers_raise_before_any_launch(pkg):
    """TypeError for the dtype of EVERY operand first, then ValueError for shapes, contiguity and devices. Every operand here lives on
    the host, so a call that got past its checks raises the device ValueError — which the well-formed call at the end does."""
    from gespmm_amd import sddmm

    o = _operands()
    M, K, H, F, nnz = 6, 5, 3, 4, 9

    def fwd(**kw):
        a = dict(o, **kw)
        return sddmm.gatv2_score(a["rp"], a["ci"], a["xl"], a["xr"], a["att"], negative_slope=a.get("slope", 0.2), out=a.get("out"))

    def bwd(**kw):
        a = dict(o, **kw)
        return sddmm.gatv2_score_backward(a["rp"], a["ci"], a["gs"], a["xl"], a["xr"], a["att"], negative_slope=a.get("slope", 0.2),
                                          order=a.get("order_"), want_att_part=a.get("want", False), out=a.get("out"))

    for call in (fwd, bwd):
        outs = {"out": torch.zeros(nnz, H) if call is fwd else torch.zeros(M, H, F)}
        floats = dict({k: o[k] for k in ("xl", "xr", "att") + (("gs",) if call is bwd else ())}, **outs)
        for name, t in floats.items():
            for dt in (torch.float16, torch.bfloat16, torch.float64, torch.int32):
                with pytest.raises(TypeError):
                    call(**{name: t.to(dt)})
            if name != "out":
                with pytest.raises(TypeError):
                    call(**{name: t.numpy()})
                with pytest.raises(TypeError):
                    call(**{name: None})
        ints = {"rp": o["rp"], "ci": o["ci"]}
        if call is bwd:
            ints["order_"] = o["order"]
        for name, t in ints.items():
            with pytest.raises(TypeError):
                call(**{name: t.long()})
            with pytest.raises(TypeError):
                call(**{name: t.tolist()})
        # a bad dtype wins over a bad shape of an EARLIER operand: dtypes of every operand come first
        with pytest.raises(TypeError):
            call(rp=o["rp"][:-1], att=o["att"].double())
        with pytest.raises(TypeError):
            call(xl=o["xl"].view(-1), **{"out": outs["out"].half()})
        for bad in ({"rp": o["rp"].view(1, -1)}, {"rp": o["rp"][:-1]}, {"rp": torch.zeros(2 * (M + 1), dtype=torch.int32)[::2]},
                    {"ci": o["ci"].view(1, -1)}, {"ci": torch.zeros(2 * nnz, dtype=torch.int32)[::2]},
                    {"xl": o["xl"].view(M, -1)}, {"xr": o["xr"].view(K, -1)}, {"xl": torch.zeros(M, 0, F), "xr": torch.zeros(K, 0, F)},
                    {"xr": torch.zeros(K, H, F + 1)}, {"xr": torch.zeros(K, H + 1, F)}, {"att": torch.zeros(1, H, F)},
                    {"att": torch.zeros(H, F + 1)}, {"att": torch.zeros(F, H).t()}, {"xl": torch.zeros(M, H, 2 * F)[:, :, ::2]},
                    {"out": outs["out"][:-1]}, {"out": outs["out"].unsqueeze(0)}, {"slope": float("nan")}, {"slope": float("inf")}):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(ValueError):
            call()  # well formed, but on the host: the device check is the last one standing
        with pytest.raises(ValueError):
            call(**outs)
    for bad in ({"gs": o["gs"][:-1]}, {"gs": o["gs"].view(-1)}, {"order_": o["order"][:-1]}, {"order_": o["order"].view(1, -1)},
                {"out": (torch.zeros(M, H, F), torch.zeros(M, H, F))},                      # a pair without want_att_part
                {"want": True, "out": (torch.zeros(M, H, F), torch.zeros(M, H, F + 1))}):
        with pytest.raises(ValueError):
            bwd(**bad)
    with pytest.raises(TypeError):
        bwd(want=True, out=(torch.zeros(M, H, F), torch.zeros(M, H, F).double()))
    with pytest.raises(ValueError):
        bwd(want=True, out=(torch.zeros(M, H, F), torch.zeros(M, H, F)))  # well formed, on the host


def test_layer_arguments(pkg):
    with pytest.raises(ValueError):
        pkg.GATv2Conv(4, 3, heads=0)
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            pkg.GATv2Conv(4, 3, dropout=p)
    shared, own = pkg.GATv2Conv(4, 3, heads=2, share_weights=True), pkg.GATv2Conv(4, 3, heads=2, concat=False, bias=False)
    assert shared.weight_dst is shared.weight_src and len(list(shared.parameters())) == 3  # one matrix, att, bias
    assert own.weight_dst is not own.weight_src and len(list(own.parameters())) == 3 and own.bias is None
    assert tuple(own.att.shape) == (1, 2, 3) and tuple(shared.bias.shape) == (6,)
    with pytest.raises(ValueError):  # not square
        own(torch.zeros(5, 4), torch.zeros(7, dtype=torch.int32), None, torch.zeros(6, dtype=torch.int32), None, None)


def test_restatement_on_a_hand_made_case():
    """Two rows, one head, F = 2, slope 0.5: every number worked by hand."""
    rowptr, colind = np.array([0, 2, 2, 3]), np.array([1, 0, 1])
    xl = np.array([[[1.0, -3.0]], [[9.0, 9.0]], [[-1.0, 0.0]]], dtype=F32)
    xr = np.array([[[0.0, 1.0]], [[2.0, -1.0]]], dtype=F32)
    att = np.array([[2.0, 4.0]], dtype=F32)
    score, terms = restate_score(rowptr, colind, xl, xr, att, 0.5)
    # entry 0: t = (3, -4) -> leaky (3, -2) -> 6 - 8; entry 1: t = (1, -2) -> (1, -1) -> 2 - 4; entry 2: t = (1, -1) -> (1, -.5) -> 2 - 2
    assert score.tolist() == [[-2.0], [-2.0], [0.0]] and terms.tolist() == [[14.0], [6.0], [4.0]]
    gs = np.array([[1.0], [10.0], [100.0]], dtype=F32)
    gx, ga, tx, ta = restate_backward(rowptr, colind, gs, xl, xr, att, 0.5)
    assert gx.tolist() == [[[22.0, 22.0]], [[0.0, 0.0]], [[200.0, 200.0]]]   # m = (2, 4 * .5) on every entry
    assert ga.tolist() == [[[13.0, -12.0]], [[0.0, 0.0]], [[100.0, -50.0]]]
    assert np.array_equal(tx, np.abs(gx)) and ta.tolist() == [[[13.0, 12.0]], [[0.0, 0.0]], [[100.0, 50.0]]]
    # the column pass: CSC arrays and the order between them
    colptr, rowind, order = np.array([0, 1, 3]), np.array([0, 0, 2]), np.array([1, 0, 2])
    gr = restate_backward(colptr, rowind, gs, xr, xl, att, 0.5, order=order)[0]
    assert gr.tolist() == [[[20.0, 20.0]], [[202.0, 202.0]]]
    # no slope: m = att everywhere, leaky = t
    assert restate_score(rowptr, colind, xl, xr, att)[0].tolist() == [[-10.0], [-6.0], [-2.0]]
    assert worst_ratio(np.array([[-2.0], [-2.0], [0.0]]), score, terms) == 0.0
