"""The fused GATv2 attention on fp16 / bf16 node terms, everything that needs no GPU: the seven symbols, both return-code ladders on
fabricated addresses, the describe table against a restated rule and against the fp32 describe call at twice the alignment, the
wrappers' error order, the function and the layer on host tensors — and the condition on the GPU test's inputs: with the fp32
restatement of test_gatv2_attention_host on the widened operands, more than half of the words of every 16-bit result are NOT
representable in the 16-bit type, so that a store that truncates, or stores another chain, is seen by a bit comparison."""
import ctypes

import numpy as np
import pytest
import torch

from test_dot_attention_host import keep_mask, pattern
from test_gatv2_attention_host import BIG, OK, UNSUPPORTED, geometry, inputs, restate_backward_col, restate_backward_row, restate_forward
from test_heads_host import EALIGN, EINVAL, ERANGE

F32 = np.float32
NEW = ("gespmm_gatv2_attention_x16", "gespmm_gatv2_attention_dropout_x16", "gespmm_gatv2_attention_backward_row_x16",
       "gespmm_gatv2_attention_backward_row_dropout_x16", "gespmm_gatv2_attention_backward_col_x16",
       "gespmm_gatv2_attention_backward_col_dropout_x16", "gespmm_describe_gatv2_attention_x16")
DTYPES = (torch.float16, torch.bfloat16)
IDS = ("fp16", "bf16")
CODE = {torch.float16: 1, torch.bfloat16: 2}
# the cases of the GPU test's bit comparison (F = 30: V = 2 on W = 4 lanes, the one width here with FOUR vectors per lane; F = 100: the
# one with W = 16)
FS16 = (1, 3, 6, 8, 20, 30, 64, 100, 130, 512)
HS16 = (1, 3)
SLOPES = (0.2, None)


def geometry_x16(F, x_align=16, att_align=16):
    """(V, W) of the 16-bit kernels, the rule restated: V the widest of 4 / 2 / 1 that divides F, whose 2 V bytes divide the 16-bit
    operands' alignment and whose 4 V bytes divide att's; W the smallest power of two in 4 .. 64 with 8 W >= F."""
    V = 4
    while V > 1 and (F % V != 0 or x_align % (2 * V) != 0 or att_align % (4 * V) != 0):
        V //= 2
    W = 4
    while W < 64 and 8 * W < F:
        W *= 2
    return V, W


def rounded(a, dtype):
    """fp32 array -> the same array rounded to `dtype` (to nearest even) and widened again: fp32 values the 16-bit type holds."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def inputs_x16(name, H, F, dtype):
    """The operands of test_gatv2_attention_host.inputs with the node terms rounded to `dtype` (as widened fp32 arrays); att stays fp32."""
    x = inputs(name, H, F)
    return {"xl": rounded(x["xl"], dtype), "xr": rounded(x["xr"], dtype), "go": rounded(x["go"], dtype), "att": x["att"]}


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_and_names(L, pkg):
    header = open(pkg.__file__.replace("gespmm_amd/__init__.py", "include/gespmm.h")).read()
    for name in NEW:
        assert name in L.EXPORTS
        getattr(L.lib, name)
        assert "int %s(" % name in header, name
    for name in ("gatv2_attention_x16", "gatv2_attention_backward_row_x16", "gatv2_attention_backward_col_x16"):
        assert callable(getattr(pkg.attention, name))
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


# (entry point, number of pointers, positions of the 16-bit pointers, positions of the results, position of stats, a pointer that may be NULL)
ENTRIES = (("gespmm_gatv2_attention_x16", 7, (2, 3, 5), (5, 6), 6, None),
           ("gespmm_gatv2_attention_backward_row_x16", 11, (2, 3, 6, 7, 9), (8, 9, 10), 5, 10),
           ("gespmm_gatv2_attention_backward_col_x16", 9, (2, 3, 7, 8), (8,), 5, None))


@pytest.mark.parametrize("name,np_,halves,results,stats_at,optional", ENTRIES)
@pytest.mark.parametrize("drop", (False, True))
def test_return_codes(L, name, np_, halves, results, stats_at, optional, drop):
    """(pointers | dtype, M, K, H, F, nnz, slope[, p, seed], stream), in the pinned order: a dtype that is neither code FIRST, then the
    fp32 ladder — sizes that make no sense, sizes too large (in element positions), the slice no kernel serves, nnz == 0 / F == 0 (the
    results and the seed alone), NULL, alignment: 2 bytes for a 16-bit pointer, 4 for att, delta and att_part, 8 for stats."""
    f0 = getattr(L.lib, name.replace("_x16", "_dropout_x16") if drop else name)

    def f(ptrs, M, K, H, F, nnz, slope, p=0.25, seed=_p(OK), dtype=2):
        tail = (p, seed, None) if drop else (None,)
        return f0(*ptrs, dtype, M, K, H, F, nnz, slope, *tail)

    none = (None,) * np_
    ok = [_p(OK)] * np_
    col = name.endswith("col_x16")
    for dtype in (0, 3, -1, 4):  # a bad dtype first: before sizes that make no sense, too large or not served, before the pointers
        assert f(ok, 4, 4, 2, 8, 10, 0.2, dtype=dtype) == EINVAL
        assert f(none, 4, 4, 2, 8, BIG, 0.2, dtype=dtype) == EINVAL
        assert f(none, 4, 4, 2, 513, 10, 0.2, dtype=dtype) == EINVAL
        assert f([_p(OK + 1)] * np_, 4, 4, 2, 8, 10, 0.2, dtype=dtype) == EINVAL
    for dtype in (1, 2):
        assert f(none, 4, 4, 0, 8, 10, 0.2, dtype=dtype) == EINVAL        # H < 1
        assert f(none, -1, 4, 2, 8, 10, 0.2, dtype=dtype) == EINVAL       # negative sizes
        assert f(none, 4, 4, 2, 8, 10, float("nan"), dtype=dtype) == EINVAL
        assert f(none, 4, 0, 2, 8, 10, 0.2, dtype=dtype) == EINVAL        # K < 1 with entries
        assert f(none, 4, 4, 0, 8, BIG, 0.2, dtype=dtype) == EINVAL       # what makes no sense before what is too large
        if drop:
            assert f(none, 4, 4, 2, 8, BIG, 0.2, p=1.0, dtype=dtype) == EINVAL
        assert f(none, 4, 4, 1, 8, BIG, 0.2, dtype=dtype) == ERANGE       # nnz
        assert f(none, 4, 4, 2, 8, BIG // 2 + 1, 0.2, dtype=dtype) == ERANGE    # nnz H
        assert f(none, BIG // 16 + 1, 4, 2, 8, 10, 0.2, dtype=dtype) == ERANGE  # M H F ELEMENT positions
        assert f(none, 4, BIG // 16 + 1, 2, 8, 10, 0.2, dtype=dtype) == ERANGE  # K H F
        assert f(none, BIG // 2 + 1, 4, 1, 1, 10, 0.2, dtype=dtype) == ERANGE   # the 2 M H words of stats
        assert f(none, BIG // 1024 + 1, 4, 2, 513, 10, 0.2, dtype=dtype) == ERANGE  # before "not served"
        assert f(none, 4, 4, 2, 513, 10, 0.2, dtype=dtype) == UNSUPPORTED
        assert f(none, 4, 4, 2, 513, 0, 0.2, dtype=dtype) == UNSUPPORTED  # before "no entries"
        assert f(ok, 4, 4, 2, 513, 10, 0.2, dtype=dtype) == UNSUPPORTED   # nothing is launched
        assert f(none, 4, 4, 2, 512, 10, 0.2, dtype=dtype) == EINVAL      # the widest slice served: on to the pointers
    # no entries, or rows of no width: the results (and the seed) alone are looked at
    for F, nnz in ((8, 0), (0, 10)):
        assert f(none, 4, 4, 2, F, nnz, 0.2) == (0 if F == 0 and col else EINVAL)
        for bad in results:
            if F == 0 and (col or bad not in (stats_at, 8)):
                continue  # (results of no elements: stats and delta are what is written)
            off = 1 if bad in halves else 2
            ptrs = [_p(OK + off) if i == bad else (_p(OK) if i in results else None) for i in range(np_)]
            assert f(ptrs, 4, 4, 2, F, nnz, 0.2) == EALIGN, (F, nnz, bad)
        if drop:
            assert f(none, 4, 4, 2, F, nnz, 0.2, seed=None) == EINVAL
    assert f(none, 0, 0, 2, 8, 0, 0.2) == 0              # nothing to write
    # the pointers
    assert f(none, 4, 4, 2, 8, 10, 0.2) == EINVAL
    for bad in range(np_):
        if bad != optional:
            assert f([None if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EINVAL, bad
        if bad in halves:  # a 16-bit operand at an odd address (an even one is valid and would launch: not tried here)
            assert f([_p(OK + 1) if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EALIGN, bad
        else:
            assert f([_p(OK + 2) if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EALIGN, bad
    assert f([_p(OK + 4) if i == stats_at else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EALIGN  # stats: 8 bytes
    assert f([None if i == 0 else _p(OK + 1) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EINVAL  # NULL before alignment
    if optional is not None:  # att_part may be NULL: the other checks still run
        assert f([None if i in (optional, 0) else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EINVAL
        assert f([None if i == optional else (_p(OK + 1) if i == 2 else _p(OK)) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EALIGN
    if drop:
        assert f(ok, 4, 4, 2, 8, 10, 0.2, seed=None) == EINVAL
        assert f(ok, 4, 4, 2, 8, 10, 0.2, seed=_p(OK + 2)) == EALIGN


@pytest.mark.parametrize("F", (1, 3, 6, 8, 20, 64, 100, 130, 512))
def test_describe_against_the_rule_and_the_fp32_call(L, F):
    for xa in (2, 4, 8, 16):
        for aa in (4, 8, 16):
            V, W = geometry_x16(F, xa, aa)
            got = L.describe_gatv2_attention(71, 53, 3, F, 1000, xa, xa, aa, x16=True)
            assert got == {"V": V, "W": W, "supported": True}, (F, xa, aa, got)
            assert V in (1, 2, 4) and F % V == 0 and 2 * V <= xa and 4 * V <= aa and 8 * W >= F and (W == 4 or 4 * W < F)
            # a 16-bit operand b bytes off a 16-byte boundary is an fp32 operand 2 b bytes off
            assert got == L.describe_gatv2_attention(71, 53, 3, F, 1000, min(2 * xa, 16), min(2 * xa, 16), aa)
        assert (V, W) == geometry(F, min(2 * xa, 16))  # (aa = 16: the fp32 rule at twice the alignment)
    # the least aligned 16-bit operand decides, whichever it is; more than 16 bytes is as good as 16
    assert L.describe_gatv2_attention(71, 53, 3, F, 1000, 2, 16, 16, x16=True) == L.describe_gatv2_attention(71, 53, 3, F, 1000, 16, 2, 16, x16=True)
    assert L.describe_gatv2_attention(71, 53, 3, F, 1000, 256, 64, 32, x16=True) == L.describe_gatv2_attention(71, 53, 3, F, 1000, x16=True)


def test_describe_edges(L):
    d = lambda *a, **k: L.describe_gatv2_attention(*a, x16=True, **k)  # noqa: E731
    assert d(10, 10, 2, 8, 0) == {"form": "none", "supported": True}
    assert d(10, 10, 2, 0, 5) == {"route": "zeros", "supported": True}
    assert d(10, 10, 2, 513, 5) == {"route": "unsupported", "supported": False}
    assert d(10, 10, 1, 512, 5) == {"V": 4, "W": 64, "supported": True}  # no V = 8
    assert d(10, 10, 1, 8, 5) == {"V": 4, "W": 4, "supported": True}
    for bad, code in (((10, 10, 0, 8, 5), EINVAL), ((BIG, 10, 1, 1, 5), ERANGE), ((10, 10, 2, 8, BIG), ERANGE)):
        with pytest.raises(L.GespmmError) as e:
            d(*bad)
        assert e.value.code == code, bad
    for al in ((1, 16, 16), (16, 12, 16), (16, 16, 2), (16, 16, 0)):
        with pytest.raises(L.GespmmError) as e:
            d(10, 10, 2, 8, 5, *al)
        assert e.value.code == EINVAL
    buf = ctypes.create_string_buffer(4)
    assert L.lib.gespmm_describe_gatv2_attention_x16(10, 10, 2, 64, 5, 16, 16, 16, buf, 4) == 3 and buf.value == b"V=4"
    assert L.lib.gespmm_describe_gatv2_attention_x16(10, 10, 2, 64, 5, 16, 16, 16, None, 4) == EINVAL


def _operands(dt, M=6, K=5, H=3, F=4, nnz=9):
    rp = torch.zeros(M + 1, dtype=torch.int32)
    rp[1:] = nnz
    cp = torch.zeros(K + 1, dtype=torch.int32)
    cp[1:] = nnz
    ind = torch.zeros(nnz, dtype=torch.int32)
    z = lambda *s: torch.zeros(*s, dtype=dt)  # noqa: E731
    return {"rp": rp, "cp": cp, "ind": ind, "xl": z(M, H, F), "xr": z(K, H, F), "att": torch.zeros(H, F), "stats": torch.zeros(M, H, 2),
            "out": z(M, H, F), "go": z(M, H, F), "delta": torch.zeros(M, H)}


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_python_wrappers_raise_before_any_launch(pkg, dt):
    """TypeError for the dtype of EVERY operand first — mixed fp16 / bf16, fp32 node terms, a 16-bit att, stats or delta — then
    ValueError for shapes, contiguity and devices. Every operand lives on the host: a call past its checks raises the device ValueError."""
    att = pkg.attention
    o = _operands(dt)
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    M, K, H, F = 6, 5, 3, 4

    def fwd(**kw):
        a = dict(o, **kw)
        return att.gatv2_attention_x16(a["rp"], a["ind"], a["xl"], a["xr"], a["att"], negative_slope=a.get("slope", 0.2),
                                       dropout=a.get("dropout"), out=a.get("out_"), stats=a.get("stats_"))

    def brow(**kw):
        a = dict(o, **kw)
        return att.gatv2_attention_backward_row_x16(a["rp"], a["ind"], a["xl"], a["xr"], a["att"], a["stats"], a["out"], a["go"],
                                                    negative_slope=a.get("slope", 0.2), dropout=a.get("dropout"),
                                                    want_att_part=a.get("want", True), results=a.get("results"))

    def bcol(**kw):
        a = dict(o, **kw)
        return att.gatv2_attention_backward_col_x16(a["cp"], a["ind"], a["xl"], a["xr"], a["att"], a["stats"], a["delta"], a["go"],
                                                    negative_slope=a.get("slope", 0.2), dropout=a.get("dropout"), result=a.get("result"))

    for call, halves, floats, ptr in ((fwd, ("xl", "xr"), ("att",), "rp"), (brow, ("xl", "xr", "out", "go"), ("att", "stats"), "rp"),
                                      (bcol, ("xl", "xr", "go"), ("att", "stats", "delta"), "cp")):
        for name in halves:
            for bad in (other, torch.float32, torch.float64, torch.int16):  # mixed 16-bit dtypes, fp32 node terms
                with pytest.raises(TypeError):
                    call(**{name: o[name].to(bad)})
            with pytest.raises(TypeError):
                call(**{name: None})
        for name in floats:
            for bad in (dt, other, torch.float64):  # a 16-bit att, stats or delta
                with pytest.raises(TypeError):
                    call(**{name: o[name].to(bad)})
        for name in (ptr, "ind"):
            with pytest.raises(TypeError):
                call(**{name: o[name].long()})
        # a bad dtype wins over a bad shape of an EARLIER operand
        with pytest.raises(TypeError):
            call(**{ptr: o[ptr][:-1], "att": o["att"].to(dt)})
        with pytest.raises(TypeError):
            call(**{"xl": o["xl"].view(M, -1), "xr": o["xr"].float()})
        for bad in ({ptr: o[ptr][:-1]}, {"xl": o["xl"].view(M, -1)}, {"xr": torch.zeros(K, H, F + 1, dtype=dt)},
                    {"att": torch.zeros(H, F + 1)}, {"xl": torch.zeros(M, H, 2 * F, dtype=dt)[:, :, ::2]}, {"slope": float("nan")},
                    {"dropout": (1.0, torch.zeros(2, dtype=torch.int32))}):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(ValueError, match="device"):
            call()  # well formed, but on the host: the device check is the last one standing
    for bad in ({"out_": torch.zeros(M, H, F)}, {"out_": torch.zeros(M, H, F, dtype=other)}, {"stats_": torch.zeros(M, H, 2, dtype=dt)}):
        with pytest.raises(TypeError):
            fwd(**bad)
    three = (torch.zeros(M, H), torch.zeros(M, H, F, dtype=dt), torch.zeros(M, H, F))
    for call, bad in ((brow, {"results": (three[0].to(dt), three[1], three[2])}), (brow, {"results": (three[0], three[1].float(), three[2])}),
                      (brow, {"results": (three[0], three[1], three[2].to(dt))}), (brow, {"results": three[:2]}),
                      (bcol, {"result": torch.zeros(K, H, F)}), (bcol, {"result": torch.zeros(K, H, F, dtype=other)})):
        with pytest.raises(TypeError):
            call(**bad)
    for call, bad in ((brow, {"results": three}), (brow, {"want": False, "results": three[:2]}),
                      (bcol, {"result": torch.zeros(K, H, F, dtype=dt)})):
        with pytest.raises(ValueError, match="device"):
            call(**bad)
    # the fp32 names keep refusing 16-bit tensors
    f32 = _operands(torch.float32)
    with pytest.raises(TypeError):
        att.gatv2_attention(o["rp"], o["ind"], o["xl"], o["xr"], o["att"])
    with pytest.raises(TypeError):
        att.gatv2_attention_backward_row(o["rp"], o["ind"], f32["xl"], f32["xr"], o["att"], o["stats"], o["out"], f32["go"])
    with pytest.raises(TypeError):
        att.gatv2_attention_backward_col(o["cp"], o["ind"], f32["xl"], f32["xr"], o["att"], o["stats"], o["delta"], o["go"])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_function_and_layer_on_host_tensors(pkg, dt):
    """GATv2AttentionFunction on 16-bit tensors reaches the 16-bit op's device ValueError, not a TypeError (att must be fp32: that one
    stays a TypeError). GATv2Conv(fused=True) on 16-bit features keeps its TypeError; with fused_x16=True it gets past it; fused_x16
    alone is a ValueError at construction; fp32 features with both set take the fp32 op."""
    n, H, F = 5, 2, 3
    rp = torch.arange(n + 1, dtype=torch.int32)
    ind = torch.arange(n, dtype=torch.int32)
    xl, xr = torch.ones(n, H, F, dtype=dt), torch.ones(n, H, F, dtype=dt)
    with pytest.raises(ValueError, match="device"):
        pkg.GATv2AttentionFunction.apply(rp, ind, rp, ind, xl, xr, torch.ones(H, F), 0.2)
    with pytest.raises(ValueError, match="device"):
        pkg.GATv2AttentionFunction.apply(rp, ind, rp, ind, xl, xl, torch.ones(H, F), None)
    with pytest.raises(TypeError):
        pkg.GATv2AttentionFunction.apply(rp, ind, rp, ind, xl, xr, torch.ones(H, F, dtype=dt), 0.2)
    with pytest.raises(TypeError):
        pkg.GATv2AttentionFunction.apply(rp, ind, rp, ind, xl, xr.float(), torch.ones(H, F), 0.2)
    x = torch.ones(n, 4, dtype=dt)
    with pytest.raises(TypeError, match="gatv2_attention"):
        pkg.GATv2Conv(4, F, heads=H, fused=True).to(dt)(x, rp, ind, rp, ind, None)
    for kw in ({}, {"share_weights": True}, {"concat": False, "bias": False}):
        layer = pkg.GATv2Conv(4, F, heads=H, fused=True, fused_x16=True, **kw).to(dt)
        assert layer.fused and layer.fused_x16 and layer.att.dtype == dt
        with pytest.raises(ValueError, match="device"):
            layer(x, rp, ind, rp, ind, None)
        with pytest.raises(ValueError, match="device"):  # fp32 features: what fused=True runs
            layer.float()(x.float(), rp, ind, rp, ind, None)
    with pytest.raises(ValueError, match="fused=True"):
        pkg.GATv2Conv(4, F, heads=H, fused_x16=True)
    with pytest.raises(ValueError, match="fused=True"):
        pkg.GATv2Conv(4, F, heads=H, fused=False, fused_x16=True)
    assert not pkg.GATv2Conv(4, F).fused_x16 and not pkg.GATv2Conv(4, F, fused=True).fused_x16


# ------------------------------------------------------------------------------- the condition on the GPU test's inputs

def restate_x16(P, x, slope, V, W, dtype, p=None):
    """The six results as the 16-bit kernels define them, by the fp32 restatement on the widened operands: -> (unrounded fp32 results,
    the same with out, grad_xl and grad_xr rounded once). The row pass is fed the ROUNDED out, the column pass that delta. p: the
    dropout rate, the mask ``keep_mask``'s as in ``restate_all``."""
    keep = keep_t = ks = None
    if p is not None:
        keep, ks = keep_mask(P, x["xl"].shape[1], p)
        keep_t, _ = keep_mask(P, x["xl"].shape[1], p, transposed=True)
    out, stats = restate_forward(P, x, slope, V, W, keep=keep, ks=ks)
    out16 = rounded(out, dtype)
    delta, grad_xl, att_part = restate_backward_row(P, x, stats, out16, slope, V, W, keep=keep, ks=ks)
    grad_xr = restate_backward_col(P, x, stats, delta, slope, V, W, keep_t=keep_t, ks=ks)
    raw = {"out": out, "stats": stats, "delta": delta, "grad_xl": grad_xl, "att_part": att_part, "grad_xr": grad_xr}
    return raw, dict(raw, out=out16, grad_xl=rounded(grad_xl, dtype), grad_xr=rounded(grad_xr, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", HS16)
@pytest.mark.parametrize("F", tuple(F for F in FS16 if F >= 8))
def test_inputs_witness_the_rounding(F, H, slope, dtype):
    """On the random pattern, at every F >= 8 of the GPU test: more than half of the words of out, grad_xl and grad_xr — computed by
    the fp32 restatement on the widened 16-bit operands — change when they are rounded to the 16-bit type. The GPU test asserts the
    same of the fp32 entry points' results before it compares bits, so a 16-bit store that truncates (or stores an operand, or one
    chain of grad_xr) cannot agree with the narrowed oracle."""
    P, x = pattern("random"), inputs_x16("random", H, F, dtype)
    V, W = geometry_x16(F)
    raw, narrowed = restate_x16(P, x, slope, V, W, dtype)
    for key in ("out", "grad_xl", "grad_xr"):
        frac = float((raw[key] != narrowed[key]).mean())
        print("random F=%d H=%d slope=%s %s %s: %.3f of the words change under the rounding" % (F, H, slope, dtype, key, frac))
        assert frac > 0.5, (key, frac)
    # ... and truncation is not the rounding: some word rounds up
    trunc_mask = 0xFFFF0000 if dtype == torch.bfloat16 else None
    if trunc_mask is not None:
        t = (raw["out"].view(np.uint32) & np.uint32(trunc_mask)).view(F32)
        assert (t != narrowed["out"]).any()
