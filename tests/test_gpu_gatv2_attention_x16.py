"""The fused GATv2 attention on fp16 / bf16 node terms on the GPU. The 16-bit kernels keep the lane positions, chains and orders of the
fp32 kernels at the same (V, W), so the oracle is the fp32 entry points on the WIDENED operands and every comparison is of bits:
stats, delta and att_part equal the fp32 results (the row pass fed widen(out16), the column pass that delta), out, grad_xl and grad_xr
equal them narrowed once (``.to(dtype)``: to nearest even). Inputs: the patterns of test_dot_attention_host and the operands of
test_gatv2_attention_host rounded to the dtype, which test_gatv2_attention_x16_host shows to witness the rounding."""
import functools

import numpy as np
import pytest
import torch

from test_dot_attention_host import SEED, pattern
from test_gatv2_attention_host import geometry
from test_gatv2_attention_x16_host import DTYPES, FS16, HS16, IDS, SLOPES, geometry_x16, inputs_x16

pytestmark = pytest.mark.gpu

KEYS = ("out", "stats", "delta", "grad_xl", "att_part", "grad_xr")
NARROW = ("out", "grad_xl", "grad_xr")  # the 16-bit results; the others are fp32 in both
NAN = float("nan")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _carved(shape, offset, dtype, fill=None):
    """A contiguous device tensor of `dtype` whose first byte lies `offset` bytes past a 16-byte boundary (torch allocates on 256)."""
    n, size = int(np.prod(shape)), torch.empty(0, dtype=dtype).element_size()
    assert offset % size == 0
    buf = torch.empty(n + 16 // size, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset // size: offset // size + n].view(shape)
    assert t.data_ptr() % 16 == offset % 16 and t.is_contiguous()
    if fill is not None:
        t.copy_(fill) if isinstance(fill, torch.Tensor) else t.fill_(fill)
    return t


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and int((_bits(a) != _bits(b)).sum()) == 0


@functools.lru_cache(maxsize=None)
def _graph(name):
    P = pattern(name)
    return {k: _dev(P[k]) for k in ("rowptr", "colind", "colptr", "rowind")}


def _seed():
    return _dev(np.array(SEED, dtype=np.uint32).view(np.int32))


def _run16(P, x, dtype, slope, g, p=None, offset=0, att_offset=0, want=True):
    """The three 16-bit launches on NaN-prefilled results -> dict of device tensors. offset: every 16-bit operand and result is carved
    `offset` bytes off a 16-byte boundary; att_offset: att and att_part."""
    from gespmm_amd import attention

    xl, xr, go = (_carved(x[n].shape, offset, dtype, _dev(x[n]).to(dtype)) for n in ("xl", "xr", "go"))
    att = _carved(x["att"].shape, att_offset, torch.float32, _dev(x["att"]))
    M, H, F = x["xl"].shape
    K = x["xr"].shape[0]
    out, gxl, gxr = (_carved(s, offset, dtype, NAN) for s in ((M, H, F), (M, H, F), (K, H, F)))
    part = _carved((M, H, F), att_offset, torch.float32, NAN)
    stats, delta = torch.full((M, H, 2), NAN, device="cuda"), torch.full((M, H), NAN, device="cuda")
    drop = None if p is None else (p, _seed())
    attention.gatv2_attention_x16(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope, dropout=drop, out=out, stats=stats)
    attention.gatv2_attention_backward_row_x16(g["rowptr"], g["colind"], xl, xr, att, stats, out, go, negative_slope=slope, dropout=drop,
                                               want_att_part=want, results=(delta, gxl, part) if want else (delta, gxl))
    attention.gatv2_attention_backward_col_x16(g["colptr"], g["rowind"], xl, xr, att, stats, delta, go, negative_slope=slope, dropout=drop,
                                               result=gxr)
    return {"out": out, "stats": stats, "delta": delta, "grad_xl": gxl, "att_part": part, "grad_xr": gxr}


def _oracle(P, x, dtype, slope, g, p=None, offset=0, att_offset=0):
    """The fp32 entry points on the widened operands, carved `offset` bytes off (att and att_part: att_offset): the row pass is fed
    widen(out narrowed once), the column pass that delta. -> (the fp32 results, the same with the 16-bit ones narrowed once)."""
    from gespmm_amd import attention

    f32 = torch.float32
    xl, xr, go = (_carved(x[n].shape, offset, f32, _dev(x[n])) for n in ("xl", "xr", "go"))
    att = _carved(x["att"].shape, att_offset, f32, _dev(x["att"]))
    M, H, F = x["xl"].shape
    K = x["xr"].shape[0]
    out, gxl, gxr = (_carved(s, offset, f32, NAN) for s in ((M, H, F), (M, H, F), (K, H, F)))
    part = _carved((M, H, F), att_offset, f32, NAN)
    stats, delta = torch.full((M, H, 2), NAN, device="cuda"), torch.full((M, H), NAN, device="cuda")
    drop = None if p is None else (p, _seed())
    attention.gatv2_attention(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope, dropout=drop, out=out, stats=stats)
    stored = _carved((M, H, F), offset, f32, out.to(dtype).float())  # what the 16-bit forward stores, widened
    attention.gatv2_attention_backward_row(g["rowptr"], g["colind"], xl, xr, att, stats, stored, go, negative_slope=slope, dropout=drop,
                                           results=(delta, gxl, part))
    attention.gatv2_attention_backward_col(g["colptr"], g["rowind"], xl, xr, att, stats, delta, go, negative_slope=slope, dropout=drop,
                                           result=gxr)
    raw = {"out": out, "stats": stats, "delta": delta, "grad_xl": gxl, "att_part": part, "grad_xr": gxr}
    return raw, {k: (t.to(dtype) if k in NARROW else t) for k, t in raw.items()}


def _assert_bits(got, want, what):
    for key in KEYS:
        assert not bool(torch.isnan(got[key]).any()), "%s: a word of %s was not written" % (what, key)
        assert _bits_equal(got[key], want[key]), "%s: %s differs from the fp32 entry point%s in %d words" % (
            what, key, " narrowed once" if key in NARROW else "", int((_bits(got[key]) != _bits(want[key])).sum()))


@functools.lru_cache(maxsize=None)
def _case(name, H, F, slope, di):
    """One case of the bit comparison, computed once: (16-bit results, unrounded fp32 oracle, narrowed oracle)."""
    dtype = DTYPES[di]
    P, x, g = pattern(name), inputs_x16(name, H, F, dtype), _graph(name)
    got = _run16(P, x, dtype, slope, g)
    raw, want = _oracle(P, x, dtype, slope, g)
    return got, raw, want


# ------------------------------------------------------------------------------------------------- 1. bits of the fp32 entries

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", HS16)
@pytest.mark.parametrize("F", FS16)
def test_bits_of_the_fp32_entry_points(pkg, F, H, slope, di):
    """V = 1 / 2 / 4, every W from 4 to 64, one to four vectors per lane, a masked last vector (F = 130)."""
    from gespmm_amd import _lib

    V, W = geometry_x16(F)
    assert (V, W) == geometry(F)
    d16 = _lib.describe_gatv2_attention(71, 53, H, F, 100, x16=True)
    assert d16 == _lib.describe_gatv2_attention(71, 53, H, F, 100) == {"V": V, "W": W, "supported": True}
    for name in ("hand", "random"):
        got, _, want = _case(name, H, F, slope, di)
        _assert_bits(got, want, "%s F=%d H=%d slope=%s %s" % (name, F, H, slope, IDS[di]))


def test_the_cases_reach_every_geometry():
    seen = {geometry_x16(F) for F in FS16}
    assert {v for v, _ in seen} == {1, 2, 4} and {w for _, w in seen} == {4, 8, 16, 32, 64}
    assert {-(-F // (geometry_x16(F)[0] * geometry_x16(F)[1])) for F in FS16} >= {1, 2, 3, 4}  # vectors per lane
    assert 130 % (2 * 32) != 0  # the last vector of F = 130 is masked in all lanes but one


# ------------------------------------------------------------------------------------------------- 2. the rounding is witnessed

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", HS16)
@pytest.mark.parametrize("F", tuple(F for F in FS16 if F >= 8))
def test_the_rounding_is_witnessed(pkg, F, H, slope, di):
    """More than half of the words of each 16-bit result differ from the fp32 oracle's unrounded word: a store that truncates, or that
    stores the wrong chain, is seen by test 1. (A condition on the inputs, checked on the CPU in test_gatv2_attention_x16_host.)"""
    got, raw, _ = _case("random", H, F, slope, di)
    for key in NARROW:
        frac = float((got[key].float() != raw[key]).float().mean())
        print("random F=%d H=%d slope=%s %s %s: %.3f of the words differ from the unrounded fp32 word" % (F, H, slope, IDS[di], key, frac))
        assert frac > 0.5, (key, frac)


# ------------------------------------------------------------------------------------------------- 3. exact corners

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("F", (3, 8, 20))
def test_exact_corners(pkg, F, di):
    """A single-entry row has out == xr[col] bit for bit and stats == (s, 1), s the bits of sddmm.gatv2_score on the widened operands; an
    empty row is +0 in every word of every row result."""
    from gespmm_amd import sddmm

    H, slope, dtype = 3, 0.2, DTYPES[di]
    P, x, g = pattern("hand"), inputs_x16("hand", H, F, dtype), _graph("hand")
    got, _, _ = _case("hand", H, F, slope, di)
    score = sddmm.gatv2_score(g["rowptr"], g["colind"], _dev(x["xl"]), _dev(x["xr"]), _dev(x["att"]), negative_slope=slope)
    one, none = np.nonzero(P["degs"] == 1)[0], np.nonzero(P["degs"] == 0)[0]
    assert one.size and none.size
    first = torch.from_numpy(P["rowptr"][one].astype(np.int64)).cuda()
    cols = torch.from_numpy(P["colind"][P["rowptr"][one]].astype(np.int64)).cuda()
    rows = torch.from_numpy(one).cuda()
    assert _bits_equal(got["out"][rows], _dev(x["xr"]).to(dtype)[cols])
    assert _bits_equal(got["stats"][rows, :, 0], score[first])
    assert bool((got["stats"][rows, :, 1] == 1.0).all())
    empty = torch.from_numpy(none).cuda()
    for key in ("out", "stats", "delta", "grad_xl", "att_part"):
        assert int((_bits(got[key][empty]) != 0).sum()) == 0, key


# ------------------------------------------------------------------------------------------------- 4. carved operands

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("offset,att_offset,V", ((2, 0, 1), (4, 0, 2), (8, 0, 4), (0, 4, 1)))
def test_carved_operands(pkg, offset, att_offset, V, di):
    """All 16-bit operands and results 2, 4 and 8 bytes off a 16-byte boundary at F = 8: V = 1, 2, 4, each with the bits of the fp32
    oracle carved 4, 8 and 16 bytes off; att (and att_part) 4 bytes off forces V = 1."""
    from gespmm_amd import _lib

    H, F, slope, dtype = 3, 8, 0.2, DTYPES[di]
    a16 = offset if offset else 16
    aatt = att_offset if att_offset else 16
    d16 = _lib.describe_gatv2_attention(71, 53, H, F, 100, a16, a16, aatt, x16=True)
    a32 = min(2 * a16, 16, aatt)
    assert d16 == {"V": V, "W": 4, "supported": True} == _lib.describe_gatv2_attention(71, 53, H, F, 100, a32, a32, a32)
    for name in ("hand", "random"):
        P, x, g = pattern(name), inputs_x16(name, H, F, dtype), _graph(name)
        got = _run16(P, x, dtype, slope, g, offset=offset, att_offset=att_offset)
        _, want = _oracle(P, x, dtype, slope, g, offset=(2 * offset) % 16, att_offset=att_offset)
        _assert_bits(got, want, "%s offset=%d att_offset=%d %s" % (name, offset, att_offset, IDS[di]))


# ------------------------------------------------------------------------------------------------- 5. dropout

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("p", (0.3, 0.6))
@pytest.mark.parametrize("F", (8, 20))
def test_dropout_bits_of_the_fp32_entry_points(pkg, F, p, di):
    H, slope, dtype = 3, 0.2, DTYPES[di]
    for name in ("hand", "random"):
        P, x, g = pattern(name), inputs_x16(name, H, F, dtype), _graph(name)
        got = _run16(P, x, dtype, slope, g, p=p)
        _, want = _oracle(P, x, dtype, slope, g, p=p)
        _assert_bits(got, want, "%s F=%d p=%g %s" % (name, F, p, IDS[di]))
        plain, _, _ = _case(name, H, F, slope, di)
        assert not _bits_equal(got["out"], plain["out"])  # the mask did something


# ------------------------------------------------------------------------------------------------- 6. NaN and infinity

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
def test_nan_and_infinity(pkg, di):
    """One NaN and one +inf element planted in xr: NaN positions equal the fp32 oracle's, every other word is bit-equal."""
    H, F, slope, dtype = 3, 8, 0.2, DTYPES[di]
    P, g = pattern("hand"), _graph("hand")
    x = {k: v.copy() for k, v in inputs_x16("hand", H, F, dtype).items()}
    c = np.unique(P["colind"])
    x["xr"][c[1], 0, 1] = np.nan
    x["xr"][c[-2], 2, 5] = np.inf
    got = _run16(P, x, dtype, slope, g)
    _, want = _oracle(P, x, dtype, slope, g)
    for key in KEYS:
        a, b = got[key], want[key]
        na, nb = torch.isnan(a), torch.isnan(b)
        assert bool((na == nb).all()), key
        assert int(((_bits(a) != _bits(b)) & ~na).sum()) == 0, key
    assert bool(torch.isnan(got["out"]).any()) and bool(torch.isnan(got["grad_xr"]).any())
    assert not bool(torch.isnan(got["out"]).all())


# ------------------------------------------------------------------------------------------------- 7. repeatability

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
def test_second_run_and_many_heads(pkg, di):
    dtype = DTYPES[di]
    P, x, g = pattern("random"), inputs_x16("random", 3, 20, dtype), _graph("random")
    first, _, _ = _case("random", 3, 20, 0.2, di)
    again = _run16(P, x, dtype, 0.2, g)
    for key in KEYS:
        assert _bits_equal(first[key], again[key]), "second run: " + key
    # H = 33 at F = 4: more heads than a wavefront has lane groups
    got, _, want = _case("hand", 33, 4, 0.2, di)
    _assert_bits(got, want, "hand F=4 H=33 %s" % IDS[di])


@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("p", (None, 0.3))
def test_eager_equals_captured(pkg, p, di):
    """One stream, no parallel branches: the three launches captured, replayed twice."""
    from gespmm_amd import attention

    H, F, slope, dtype = 3, 20, 0.2, DTYPES[di]
    P, x, g = pattern("hand"), inputs_x16("hand", H, F, dtype), _graph("hand")
    eager = _run16(P, x, dtype, slope, g, p=p)
    xl, xr, go = (_dev(x[n]).to(dtype) for n in ("xl", "xr", "go"))
    att = _dev(x["att"])
    drop = None if p is None else (p, _seed())
    M = xl.shape[0]
    res = {"out": torch.empty_like(xl), "stats": torch.empty(M, H, 2, device="cuda"), "delta": torch.empty(M, H, device="cuda"),
           "grad_xl": torch.empty_like(xl), "att_part": torch.empty(M, H, F, device="cuda"), "grad_xr": torch.empty_like(xr)}

    def launches():
        attention.gatv2_attention_x16(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope, dropout=drop, out=res["out"],
                                      stats=res["stats"])
        attention.gatv2_attention_backward_row_x16(g["rowptr"], g["colind"], xl, xr, att, res["stats"], res["out"], go, negative_slope=slope,
                                                   dropout=drop, results=(res["delta"], res["grad_xl"], res["att_part"]))
        attention.gatv2_attention_backward_col_x16(g["colptr"], g["rowind"], xl, xr, att, res["stats"], res["delta"], go,
                                                   negative_slope=slope, dropout=drop, result=res["grad_xr"])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launches()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    for _ in range(2):
        for t in res.values():
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for key in KEYS:
            assert _bits_equal(res[key], eager[key]), key


# ------------------------------------------------------------------------------------------------- 8. rejected sizes

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
def test_a_slice_of_513_elements_raises_and_launches_nothing(pkg, di):
    from gespmm_amd import _lib, attention

    dtype, code = DTYPES[di], di + 1
    P, g = pattern("random"), _graph("random")
    H, F = 1, 513
    M, K = P["M"], P["K"]
    h = lambda *s: torch.ones(*s, dtype=dtype, device="cuda")  # noqa: E731
    hn = lambda *s: torch.full(s, NAN, dtype=dtype, device="cuda")  # noqa: E731
    fn = lambda *s: torch.full(s, NAN, device="cuda")  # noqa: E731
    xl, xr, att = h(M, H, F), h(K, H, F), torch.ones(H, F, device="cuda")
    out, stats, delta, gxl, part, gxr = hn(M, H, F), fn(M, H, 2), fn(M, H), hn(M, H, F), fn(M, H, F), hn(K, H, F)
    calls = (lambda: attention.gatv2_attention_x16(g["rowptr"], g["colind"], xl, xr, att, out=out, stats=stats),
             lambda: attention.gatv2_attention_backward_row_x16(g["rowptr"], g["colind"], xl, xr, att, stats, out, xl, results=(delta, gxl, part)),
             lambda: attention.gatv2_attention_backward_col_x16(g["colptr"], g["rowind"], xl, xr, att, stats, delta, xl, result=gxr))
    for call in calls:
        with pytest.raises(_lib.GespmmError) as e:
            call()
        assert e.value.code == -7 and "512" in str(e.value)
    ptr = [t.data_ptr() for t in (g["rowptr"], g["colind"], xl, xr, att)]
    rcs = (_lib.lib.gespmm_gatv2_attention_x16(*ptr, out.data_ptr(), stats.data_ptr(), code, M, K, H, F, P["nnz"], 0.2, None),
           _lib.lib.gespmm_gatv2_attention_backward_row_x16(*ptr, stats.data_ptr(), out.data_ptr(), xl.data_ptr(), delta.data_ptr(),
                                                            gxl.data_ptr(), part.data_ptr(), code, M, K, H, F, P["nnz"], 0.2, None),
           _lib.lib.gespmm_gatv2_attention_backward_col_x16(g["colptr"].data_ptr(), g["rowind"].data_ptr(), *ptr[2:], stats.data_ptr(),
                                                            delta.data_ptr(), xl.data_ptr(), gxr.data_ptr(), code, M, K, H, F, P["nnz"], 0.2,
                                                            None))
    torch.cuda.synchronize()
    assert rcs == (-7, -7, -7)
    for t in (out, stats, delta, gxl, part, gxr):
        assert bool(torch.isnan(t).all())


@pytest.mark.parametrize("di", (0, 1), ids=IDS)
def test_no_entries_zero_fills(pkg, di):
    from gespmm_amd import attention

    dtype = DTYPES[di]
    M, K, H, F = 5, 4, 2, 8
    rowptr, colptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    ind = torch.zeros(0, dtype=torch.int32, device="cuda")
    xl, xr = torch.ones(M, H, F, dtype=dtype, device="cuda"), torch.ones(K, H, F, dtype=dtype, device="cuda")
    att = torch.ones(H, F, device="cuda")
    out, gxl, gxr = (torch.full(s, NAN, dtype=dtype, device="cuda") for s in ((M, H, F), (M, H, F), (K, H, F)))
    stats, delta, part = (torch.full(s, NAN, device="cuda") for s in ((M, H, 2), (M, H), (M, H, F)))
    for drop in (None, (0.5, _seed())):
        for t in (out, stats, delta, gxl, part, gxr):
            t.fill_(NAN)
        attention.gatv2_attention_x16(rowptr, ind, xl, xr, att, dropout=drop, out=out, stats=stats)
        attention.gatv2_attention_backward_row_x16(rowptr, ind, xl, xr, att, stats, out, xl, dropout=drop, results=(delta, gxl, part))
        attention.gatv2_attention_backward_col_x16(colptr, ind, xl, xr, att, stats, delta, xl, dropout=drop, result=gxr)
        for t in (out, stats, delta, gxl, part, gxr):
            assert int((_bits(t) != 0).sum()) == 0  # +0 in every word
