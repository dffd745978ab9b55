"""The fused dot-product attention on fp16 / bf16 q, k and v, everything that needs no GPU: the seven symbols, both return-code ladders
on fabricated addresses, the describe table against a restated rule and against the fp32 describe call at twice the alignment, the
wrappers' error order, the function and the layer on host tensors — and the condition on the GPU test's inputs: with the fp32
restatement of test_dot_attention_host on the widened operands, more than half of the words of every 16-bit result are NOT
representable in the 16-bit type, so that a store that truncates, or stores another chain, is seen by a bit comparison."""
import ctypes

import numpy as np
import pytest
import torch

from test_dot_attention_host import (BIG, OK, UNSUPPORTED, geometry, inputs, keep_mask, pattern, restate_backward_kv, restate_backward_q,
                                     restate_forward)
from test_heads_host import EALIGN, EINVAL, ERANGE

F32 = np.float32
NEW = ("gespmm_dot_attention_x16", "gespmm_dot_attention_dropout_x16", "gespmm_dot_attention_backward_q_x16",
       "gespmm_dot_attention_backward_q_dropout_x16", "gespmm_dot_attention_backward_kv_x16",
       "gespmm_dot_attention_backward_kv_dropout_x16", "gespmm_describe_dot_attention_x16")
DTYPES = (torch.float16, torch.bfloat16)
IDS = ("fp16", "bf16")
CODE = {torch.float16: 1, torch.bfloat16: 2}
# the cases of the GPU test's bit comparison (F = 30: V = 2 on W = 4 lanes, the one width here with FOUR vectors per lane; F = 100: the
# one with W = 16)
FS16 = (1, 3, 6, 8, 20, 30, 64, 100, 130, 512)
HS16 = (1, 3)
PATTERNS = ("hand", "random")


def geometry_x16(F, align=16):
    """(V, W) of the 16-bit kernels, the rule restated: V the widest of 4 / 2 / 1 that divides F and whose 2 V bytes divide the 16-bit
    operands' alignment; W the smallest power of two in 4 .. 64 with 8 W >= F."""
    V = 4
    while V > 1 and (F % V != 0 or align % (2 * V) != 0):
        V //= 2
    W = 4
    while W < 64 and 8 * W < F:
        W *= 2
    return V, W


def rounded(a, dtype):
    """fp32 array -> the same array rounded to `dtype` (to nearest even) and widened again: fp32 values the 16-bit type holds."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def inputs_x16(name, H, F, dtype):
    """The operands of test_dot_attention_host.inputs with q, k, v and grad_out rounded to `dtype` (as widened fp32 arrays)."""
    x = inputs(name, H, F)
    return {"q": rounded(x["q"], dtype), "k": rounded(x["k"], dtype), "v": rounded(x["v"], dtype), "go": rounded(x["go"], dtype),
            "scale": x["scale"]}


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
    for name in ("dot_attention_x16", "dot_attention_backward_q_x16", "dot_attention_backward_kv_x16"):
        assert callable(getattr(pkg.attention, name))
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


# (entry point, number of pointers, positions of the 16-bit pointers, positions of the results, position of stats)
ENTRIES = (("gespmm_dot_attention_x16", 7, (2, 3, 4, 5), (5, 6), 6),
           ("gespmm_dot_attention_backward_q_x16", 10, (2, 3, 4, 6, 7, 9), (8, 9), 5),
           ("gespmm_dot_attention_backward_kv_x16", 10, (2, 3, 4, 7, 8, 9), (8, 9), 5))


@pytest.mark.parametrize("name,np_,halves,results,stats_at", ENTRIES)
@pytest.mark.parametrize("drop", (False, True))
def test_return_codes(L, name, np_, halves, results, stats_at, drop):
    """(pointers | dtype, M, K, H, F, nnz, scale[, p, seed], stream), in the pinned order: a dtype that is neither code FIRST, then the
    fp32 ladder of the dot entries — sizes that make no sense, sizes too large (in element positions), the slice no kernel serves,
    nnz == 0 / F == 0 (the results and the seed alone), NULL, alignment: 2 bytes for a 16-bit pointer, 4 for delta and the seed, 8 for
    stats."""
    f0 = getattr(L.lib, name.replace("_x16", "_dropout_x16") if drop else name)

    def f(ptrs, M, K, H, F, nnz, scale, p=0.25, seed=_p(OK), dtype=2):
        tail = (p, seed, None) if drop else (None,)
        return f0(*ptrs, dtype, M, K, H, F, nnz, scale, *tail)

    none = (None,) * np_
    ok = [_p(OK)] * np_
    kv = name.endswith("kv_x16")
    for dtype in (0, 3, -1, 4):  # a bad dtype first: before sizes that make no sense, too large or not served, before the pointers
        assert f(ok, 4, 4, 2, 8, 10, 0.5, dtype=dtype) == EINVAL
        assert f(none, 4, 4, 2, 8, BIG, 0.5, dtype=dtype) == EINVAL
        assert f(none, 4, 4, 2, 513, 10, 0.5, dtype=dtype) == EINVAL
        assert f([_p(OK + 1)] * np_, 4, 4, 2, 8, 10, 0.5, dtype=dtype) == EINVAL
    for dtype in (1, 2):
        assert f(none, 4, 4, 0, 8, 10, 0.5, dtype=dtype) == EINVAL        # H < 1
        assert f(none, -1, 4, 2, 8, 10, 0.5, dtype=dtype) == EINVAL       # negative sizes
        assert f(none, 4, -4, 2, 8, 0, 0.5, dtype=dtype) == EINVAL
        assert f(none, 4, 4, 2, -8, 10, 0.5, dtype=dtype) == EINVAL
        assert f(none, 4, 4, 2, 8, -1, 0.5, dtype=dtype) == EINVAL
        assert f(none, 4, 0, 2, 8, 10, 0.5, dtype=dtype) == EINVAL        # K < 1 with entries
        assert f(none, 0, 4, 2, 8, 10, 0.5, dtype=dtype) == EINVAL        # entries without rows
        assert f(none, 4, 4, 2, 8, 10, float("inf"), dtype=dtype) == EINVAL
        assert f(none, 4, 4, 2, 8, 10, float("nan"), dtype=dtype) == EINVAL
        assert f(none, 4, 4, 0, 8, BIG, 0.5, dtype=dtype) == EINVAL       # what makes no sense before what is too large
        assert f(none, 4, 4, 2, 513, 10, float("nan"), dtype=dtype) == EINVAL  # ... and before what is not served
        if drop:
            for p in (-0.1, 1.0, float("nan")):
                assert f(none, 4, 4, 2, 8, 10, 0.5, p=p, dtype=dtype) == EINVAL
                assert f(none, 4, 4, 2, 8, BIG, 0.5, p=p, dtype=dtype) == EINVAL
        assert f(none, 4, 4, 1, 8, BIG, 0.5, dtype=dtype) == ERANGE       # nnz
        assert f(none, 4, 4, 2, 8, BIG // 2 + 1, 0.5, dtype=dtype) == ERANGE    # nnz H
        assert f(none, BIG, 4, 1, 1, 10, 0.5, dtype=dtype) == ERANGE      # M
        assert f(none, BIG // 16 + 1, 4, 2, 8, 10, 0.5, dtype=dtype) == ERANGE  # M H F ELEMENT positions
        assert f(none, 4, BIG // 16 + 1, 2, 8, 10, 0.5, dtype=dtype) == ERANGE  # K H F
        assert f(none, BIG // 2 + 1, 4, 1, 1, 10, 0.5, dtype=dtype) == ERANGE   # the 2 M H words of stats
        assert f(none, BIG, 4, 1, 1, 0, 0.5, dtype=dtype) == ERANGE       # too large comes before "no entries"
        assert f(none, BIG // 1024 + 1, 4, 2, 513, 10, 0.5, dtype=dtype) == ERANGE  # ... and before "not served"
        assert f(none, 4, 4, 2, 513, 10, 0.5, dtype=dtype) == UNSUPPORTED
        assert f(none, 4, 4, 2, 513, 0, 0.5, dtype=dtype) == UNSUPPORTED  # before "no entries"
        assert f(ok, 4, 4, 2, 4096, 10, 0.5, dtype=dtype) == UNSUPPORTED  # nothing is launched
        assert f(none, 4, 4, 2, 512, 10, 0.5, dtype=dtype) == EINVAL      # the widest slice served: on to the pointers
    # no entries, or rows of no width: the results (and the seed) alone are looked at
    for F, nnz in ((8, 0), (0, 10)):
        assert f(none, 4, 4, 2, F, nnz, 0.5) == (0 if F == 0 and kv else EINVAL)
        for bad in results:
            if F == 0 and (kv or bad not in (stats_at, 8)):
                continue  # (results of no elements: stats and delta are what is written)
            off = 1 if bad in halves else 2
            ptrs = [_p(OK + off) if i == bad else (_p(OK) if i in results else None) for i in range(np_)]
            assert f(ptrs, 4, 4, 2, F, nnz, 0.5) == EALIGN, (F, nnz, bad)
        if drop:
            assert f(none, 4, 4, 2, F, nnz, 0.5, seed=None) == EINVAL
            assert f(none, 0, 0, 2, F, 0, 0.5, seed=_p(OK + 2)) == EALIGN
    assert f(none, 0, 0, 2, 8, 0, 0.5) == 0              # nothing to write
    # the pointers
    assert f(none, 4, 4, 2, 8, 10, 0.5) == EINVAL
    for bad in range(np_):
        assert f([None if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.5) == EINVAL, bad
        # a 16-bit operand at an odd address (an even one is valid and would launch: not tried here); 2 bytes off for the others
        off = 1 if bad in halves else 2
        assert f([_p(OK + off) if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.5) == EALIGN, bad
    assert f([_p(OK + 4) if i == stats_at else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.5) == EALIGN  # stats: 8 bytes
    assert f([None if i == 0 else _p(OK + 1) for i in range(np_)], 4, 4, 2, 8, 10, 0.5) == EINVAL  # NULL before alignment
    if drop:
        assert f(ok, 4, 4, 2, 8, 10, 0.5, seed=None) == EINVAL
        assert f(ok, 4, 4, 2, 8, 10, 0.5, seed=_p(OK + 2)) == EALIGN


@pytest.mark.parametrize("F", (1, 3, 6, 8, 20, 64, 100, 130, 512))
def test_describe_against_the_rule_and_the_fp32_call(L, F):
    for a in (2, 4, 8, 16):
        V, W = geometry_x16(F, a)
        got = L.describe_dot_attention(71, 53, 3, F, 1000, a, a, a, x16=True)
        assert got == {"V": V, "W": W}, (F, a, got)
        assert V in (1, 2, 4) and F % V == 0 and 2 * V <= a and 8 * W >= F and (W == 4 or 4 * W < F)
        # a 16-bit operand b bytes off a 16-byte boundary is an fp32 operand 2 b bytes off
        twice = min(2 * a, 16)
        assert got == L.describe_dot_attention(71, 53, 3, F, 1000, twice, twice, twice)
        assert (V, W) == geometry(F, twice)
        # the least aligned 16-bit operand decides, whichever it is
        for al in ((a, 16, 16), (16, a, 16), (16, 16, a)):
            assert L.describe_dot_attention(71, 53, 3, F, 1000, *al, x16=True) == got, al
    # more than 16 bytes is as good as 16
    assert L.describe_dot_attention(71, 53, 3, F, 1000, 256, 64, 32, x16=True) == L.describe_dot_attention(71, 53, 3, F, 1000, x16=True)


def test_describe_edges(L):
    d = lambda *a, **k: L.describe_dot_attention(*a, x16=True, **k)  # noqa: E731
    assert d(10, 10, 2, 8, 0) == {"form": "none"}
    assert d(0, 0, 2, 8, 0) == {"form": "none"}
    assert d(10, 10, 2, 0, 5) == {"route": "zeros"}
    assert d(10, 10, 2, 513, 5) == {"route": "unsupported"}
    assert d(10, 10, 2, 513, 0) == {"route": "unsupported"}  # the entry points' order
    assert d(10, 10, 1, 512, 5) == {"V": 4, "W": 64}  # no V = 8
    assert d(10, 10, 1, 8, 5) == {"V": 4, "W": 4}
    for bad, code in (((10, 10, 0, 8, 5), EINVAL), ((-1, 10, 2, 8, 5), EINVAL), ((BIG, 10, 1, 1, 5), ERANGE), ((10, 10, 2, 8, BIG), ERANGE)):
        with pytest.raises(L.GespmmError) as e:
            d(*bad)
        assert e.value.code == code, bad
    for al in ((1, 16, 16), (16, 12, 16), (16, 16, 0)):
        with pytest.raises(L.GespmmError) as e:
            d(10, 10, 2, 8, 5, *al)
        assert e.value.code == EINVAL
    buf = ctypes.create_string_buffer(4)
    assert L.lib.gespmm_describe_dot_attention_x16(10, 10, 2, 64, 5, 16, 16, 16, buf, 4) == 3 and buf.value == b"V=4"
    assert L.lib.gespmm_describe_dot_attention_x16(10, 10, 2, 64, 5, 16, 16, 16, None, 4) == EINVAL


def _operands(dt, M=6, K=5, H=3, F=4, nnz=9):
    rp = torch.zeros(M + 1, dtype=torch.int32)
    rp[1:] = nnz
    cp = torch.zeros(K + 1, dtype=torch.int32)
    cp[1:] = nnz
    ind = torch.zeros(nnz, dtype=torch.int32)
    z = lambda *s: torch.zeros(*s, dtype=dt)  # noqa: E731
    return {"rp": rp, "cp": cp, "ind": ind, "q": z(M, H, F), "k": z(K, H, F), "v": z(K, H, F), "stats": torch.zeros(M, H, 2),
            "out": z(M, H, F), "go": z(M, H, F), "delta": torch.zeros(M, H)}


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_python_wrappers_raise_before_any_launch(pkg, dt):
    """TypeError for the dtype of EVERY operand first — mixed fp16 / bf16, fp32 node terms, a 16-bit stats or delta — then ValueError
    for shapes, contiguity and devices. Every operand lives on the host: a call past its checks raises the device ValueError."""
    att = pkg.attention
    o = _operands(dt)
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    M, K, H, F, nnz = 6, 5, 3, 4, 9

    def fwd(**kw):
        a = dict(o, **kw)
        return att.dot_attention_x16(a["rp"], a["ind"], a["q"], a["k"], a["v"], scale=a.get("scale"), dropout=a.get("dropout"),
                                     out=a.get("out_"), stats=a.get("stats_"))

    def bq(**kw):
        a = dict(o, **kw)
        return att.dot_attention_backward_q_x16(a["rp"], a["ind"], a["q"], a["k"], a["v"], a["stats"], a["out"], a["go"],
                                                scale=a.get("scale"), dropout=a.get("dropout"), results=a.get("results"))

    def bkv(**kw):
        a = dict(o, **kw)
        return att.dot_attention_backward_kv_x16(a["cp"], a["ind"], a["q"], a["k"], a["v"], a["stats"], a["delta"], a["go"],
                                                 scale=a.get("scale"), dropout=a.get("dropout"), results=a.get("results"))

    seed = torch.zeros(2, dtype=torch.int32)
    for call, halves, floats, ptr in ((fwd, ("q", "k", "v"), (), "rp"), (bq, ("q", "k", "v", "out", "go"), ("stats",), "rp"),
                                      (bkv, ("q", "k", "v", "go"), ("stats", "delta"), "cp")):
        for name in halves:
            for bad in (other, torch.float32, torch.float64, torch.int16):  # mixed 16-bit dtypes, fp32 node terms
                with pytest.raises(TypeError):
                    call(**{name: o[name].to(bad)})
            with pytest.raises(TypeError):
                call(**{name: None})
        for name in floats:
            for bad in (dt, other, torch.float64):  # a 16-bit stats or delta
                with pytest.raises(TypeError):
                    call(**{name: o[name].to(bad)})
            with pytest.raises(TypeError):
                call(**{name: None})
        for name in (ptr, "ind"):
            with pytest.raises(TypeError):
                call(**{name: o[name].long()})
        # a bad dtype wins over a bad shape of an EARLIER operand
        with pytest.raises(TypeError):
            call(**{ptr: o[ptr][:-1], "v": o["v"].float()})
        with pytest.raises(TypeError):
            call(**{"q": o["q"].view(M, -1), "k": o["k"].to(other)})
        for bad in ({"dropout": 0.5}, {"dropout": (0.5, seed.long())}, {"scale": torch.tensor(1.0)}, {"scale": "1"}):
            with pytest.raises(TypeError):
                call(**bad)
        for bad in ({ptr: o[ptr][:-1]}, {"ind": o["ind"].view(1, -1)}, {"q": o["q"].view(M, -1)}, {"k": torch.zeros(K, H, F + 1, dtype=dt)},
                    {"v": torch.zeros(K + 1, H, F, dtype=dt)}, {"q": torch.zeros(M, H, 2 * F, dtype=dt)[:, :, ::2]}, {"scale": float("nan")},
                    {"dropout": (1.0, seed)}):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(ValueError, match="device"):
            call()  # well formed, but on the host: the device check is the last one standing
    for bad in ({"out_": torch.zeros(M, H, F)}, {"out_": torch.zeros(M, H, F, dtype=other)}, {"stats_": torch.zeros(M, H, 2, dtype=dt)}):
        with pytest.raises(TypeError):
            fwd(**bad)
    zq, zk = torch.zeros(M, H, F, dtype=dt), torch.zeros(K, H, F, dtype=dt)
    for call, bad in ((bq, {"results": (torch.zeros(M, H, dtype=dt), zq)}), (bq, {"results": (torch.zeros(M, H), zq.float())}),
                      (bq, {"results": (torch.zeros(M, H), zq.to(other))}), (bq, {"results": (torch.zeros(M, H),)}),
                      (bkv, {"results": (zk.float(), zk)}), (bkv, {"results": (zk, zk.to(other))}), (bkv, {"results": zk})):
        with pytest.raises(TypeError):
            call(**bad)
    for call, bad in ((bq, {"results": (torch.zeros(M, H), zq)}), (bkv, {"results": (zk, zk.clone())})):
        with pytest.raises(ValueError, match="device"):
            call(**bad)
    for call, bad in ((bq, {"results": (torch.zeros(M, H, 1), zq)}), (bkv, {"results": (zk, zq)}), (bq, {"stats": torch.zeros(M, H)}),
                      (bkv, {"delta": torch.zeros(M, H, 1)})):
        with pytest.raises(ValueError):
            call(**bad)
    # the fp32 names keep refusing 16-bit tensors
    f32 = _operands(torch.float32)
    with pytest.raises(TypeError):
        att.dot_attention(o["rp"], o["ind"], o["q"], o["k"], o["v"])
    with pytest.raises(TypeError):
        att.dot_attention_backward_q(o["rp"], o["ind"], f32["q"], f32["k"], f32["v"], o["stats"], o["out"], f32["go"])
    with pytest.raises(TypeError):
        att.dot_attention_backward_kv(o["cp"], o["ind"], f32["q"], f32["k"], f32["v"], o["stats"], o["delta"], o["go"])


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_function_and_layer_on_host_tensors(pkg, dt):
    """DotAttentionFunction on 16-bit tensors reaches the 16-bit op's device ValueError, not a TypeError (mixed dtypes stay a
    TypeError). TransformerConv(fused=True) on 16-bit features keeps its TypeError; with fused_x16=True it gets past it; fused_x16
    alone is a ValueError at construction; fp32 features with both set take the fp32 op."""
    n, H, F = 5, 2, 3
    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    rp = torch.arange(n + 1, dtype=torch.int32)
    ind = torch.arange(n, dtype=torch.int32)
    q, k, v = (torch.ones(n, H, F, dtype=dt) for _ in range(3))
    with pytest.raises(ValueError, match="device"):
        pkg.DotAttentionFunction.apply(q, k, v, rp, ind, rp, ind)
    with pytest.raises(ValueError, match="device"):
        pkg.DotAttentionFunction.apply(q, k, v, rp, ind, rp, ind, 0.5, 0.25, torch.zeros(2, dtype=torch.int32))
    for mixed in ((q.float(), k, v), (q, k.float(), v), (q, k, v.float()), (q, k.to(other), v), (q.to(other), k, v)):
        with pytest.raises(TypeError):
            pkg.DotAttentionFunction.apply(*mixed, rp, ind, rp, ind)
    x = torch.ones(n, 4, dtype=dt)
    with pytest.raises(TypeError, match="dot_attention"):
        pkg.TransformerConv(4, F, heads=H, fused=True).to(dt)(x, rp, ind, rp, ind, None)
    for kw in ({}, {"concat": False, "bias": False}, {"beta": True}, {"root_weight": False}):
        layer = pkg.TransformerConv(4, F, heads=H, fused=True, fused_x16=True, **kw).to(dt)
        assert layer.fused and layer.fused_x16 and layer.lin_key.weight.dtype == dt
        with pytest.raises(ValueError, match="device"):
            layer(x, rp, ind, rp, ind, None)
        with pytest.raises(ValueError, match="device"):  # fp32 features: what fused=True runs
            layer.float()(x.float(), rp, ind, rp, ind, None)
    with pytest.raises(ValueError, match="fused=True"):
        pkg.TransformerConv(4, F, heads=H, fused_x16=True)
    with pytest.raises(ValueError, match="fused=True"):
        pkg.TransformerConv(4, F, heads=H, fused=False, fused_x16=True)
    assert not pkg.TransformerConv(4, F).fused_x16 and not pkg.TransformerConv(4, F, fused=True).fused_x16


# ------------------------------------------------------------------------------- the condition on the GPU test's inputs

def restate_x16(P, x, V, W, dtype, p=None):
    """The six results as the 16-bit kernels define them, by the fp32 restatement on the widened operands: -> (unrounded fp32 results,
    the same with out, grad_q, grad_k and grad_v rounded once). The row pass is fed the ROUNDED out, the column pass that delta. p: the
    dropout rate, the mask ``keep_mask``'s as in ``restate_all``."""
    keep = keep_t = ks = None
    if p is not None:
        keep, ks = keep_mask(P, x["q"].shape[1], p)
        keep_t, _ = keep_mask(P, x["q"].shape[1], p, transposed=True)
    out, stats = restate_forward(P, x, V, W, keep=keep, ks=ks)
    out16 = rounded(out, dtype)
    delta, grad_q = restate_backward_q(P, x, stats, out16, V, W, keep=keep, ks=ks)
    grad_k, grad_v = restate_backward_kv(P, x, stats, delta, V, W, keep_t=keep_t, ks=ks)
    raw = {"out": out, "stats": stats, "delta": delta, "grad_q": grad_q, "grad_k": grad_k, "grad_v": grad_v}
    return raw, dict(raw, out=out16, grad_q=rounded(grad_q, dtype), grad_k=rounded(grad_k, dtype), grad_v=rounded(grad_v, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H", HS16)
@pytest.mark.parametrize("F", FS16)
@pytest.mark.parametrize("name", PATTERNS)
def test_inputs_witness_the_rounding(name, F, H, dtype):
    """At every case of the GPU test's bit comparison: more than half of the words of out, grad_q, grad_k and grad_v — computed by the
    fp32 restatement on the widened 16-bit operands — are not representable in the 16-bit type, and all are finite. A 16-bit store that
    truncates (or stores an operand, or an unscaled chain) cannot then agree with the narrowed oracle. The smallest share is that of
    out and grad_q (about 0.81): rows of degree 0 and 1, whose out is 0 or a copy of v."""
    P, x = pattern(name), inputs_x16(name, H, F, dtype)
    V, W = geometry_x16(F)
    raw, narrowed = restate_x16(P, x, V, W, dtype)
    for key in ("out", "grad_q", "grad_k", "grad_v"):
        assert np.isfinite(raw[key]).all() and np.isfinite(narrowed[key]).all(), key
        frac = float((raw[key] != narrowed[key]).mean())
        print("%s F=%d H=%d %s %s: %.3f of the words change under the rounding" % (name, F, H, dtype, key, frac))
        assert frac > 0.5, (key, frac)
    if dtype == torch.bfloat16:  # ... and truncation is not the rounding: some word rounds up
        t = (raw["out"].view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
        assert (t != narrowed["out"]).any()
