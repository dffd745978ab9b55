"""The fused dot-product attention on fp16 / bf16 q, k and v on the GPU. The 16-bit kernels keep the lane positions, chains and orders
of the fp32 kernels at the same (V, W), so the oracle is the fp32 entry points on the WIDENED operands and every comparison is of bits,
on NaN-prefilled results: stats and delta equal the fp32 results (the row pass fed widen(out16), the column pass that delta), out,
grad_q, grad_k and grad_v equal them narrowed once (``.to(dtype)``: to nearest even). Inputs: the patterns and operands of
test_dot_attention_host rounded to the dtype, which test_dot_attention_x16_host shows to witness the rounding. One check against
float64 holds the results to the derived tolerances of test_dot_attention_host plus the one rounding of a 16-bit store."""
import functools

import numpy as np
import pytest
import torch

from attention_refs import tol16
from test_dot_attention_host import FS, HS, SEED, _chain_case, geometry, pattern, ratio, ref_backward, ref_forward, transpose
from test_dot_attention_x16_host import DTYPES, FS16, HS16, IDS, PATTERNS, geometry_x16, inputs_x16, rounded
from test_gpu_dot_attention import CHAINS

pytestmark = pytest.mark.gpu

KEYS = ("out", "stats", "delta", "grad_q", "grad_k", "grad_v")
NARROW = ("out", "grad_q", "grad_k", "grad_v")  # the 16-bit results; stats and delta are fp32 in both
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


def _graph_of(P):
    return {k: _dev(P[k]) for k in ("rowptr", "colind", "colptr", "rowind")}


@functools.lru_cache(maxsize=None)
def _graph(name):
    return _graph_of(pattern(name))


def _seed():
    return _dev(np.array(SEED, dtype=np.uint32).view(np.int32))


def _run16(x, dtype, g, p=None, offset=0):
    """The three 16-bit launches on NaN-prefilled results -> dict of device tensors. offset: every 16-bit operand and result is carved
    `offset` bytes off a 16-byte boundary."""
    from gespmm_amd import attention

    q, k, v, go = (_carved(x[n].shape, offset, dtype, _dev(x[n]).to(dtype)) for n in ("q", "k", "v", "go"))
    M, H, F = x["q"].shape
    K = x["k"].shape[0]
    out, gq, gk, gv = (_carved(s, offset, dtype, NAN) for s in ((M, H, F), (M, H, F), (K, H, F), (K, H, F)))
    stats, delta = torch.full((M, H, 2), NAN, device="cuda"), torch.full((M, H), NAN, device="cuda")
    drop = None if p is None else (p, _seed())
    attention.dot_attention_x16(g["rowptr"], g["colind"], q, k, v, scale=x["scale"], dropout=drop, out=out, stats=stats)
    attention.dot_attention_backward_q_x16(g["rowptr"], g["colind"], q, k, v, stats, out, go, scale=x["scale"], dropout=drop,
                                           results=(delta, gq))
    attention.dot_attention_backward_kv_x16(g["colptr"], g["rowind"], q, k, v, stats, delta, go, scale=x["scale"], dropout=drop,
                                            results=(gk, gv))
    return {"out": out, "stats": stats, "delta": delta, "grad_q": gq, "grad_k": gk, "grad_v": gv}


def _oracle(x, dtype, g, p=None, offset=0):
    """The fp32 entry points on the widened operands, carved `offset` bytes off: the row pass is fed widen(out narrowed once), the
    column pass that delta. -> (the fp32 results, the same with the 16-bit ones narrowed once)."""
    from gespmm_amd import attention

    f32 = torch.float32
    q, k, v, go = (_carved(x[n].shape, offset, f32, _dev(x[n])) for n in ("q", "k", "v", "go"))
    M, H, F = x["q"].shape
    K = x["k"].shape[0]
    out, gq, gk, gv = (_carved(s, offset, f32, NAN) for s in ((M, H, F), (M, H, F), (K, H, F), (K, H, F)))
    stats, delta = torch.full((M, H, 2), NAN, device="cuda"), torch.full((M, H), NAN, device="cuda")
    drop = None if p is None else (p, _seed())
    attention.dot_attention(g["rowptr"], g["colind"], q, k, v, scale=x["scale"], dropout=drop, out=out, stats=stats)
    stored = _carved((M, H, F), offset, f32, out.to(dtype).float())  # what the 16-bit forward stores, widened
    attention.dot_attention_backward_q(g["rowptr"], g["colind"], q, k, v, stats, stored, go, scale=x["scale"], dropout=drop,
                                       results=(delta, gq))
    attention.dot_attention_backward_kv(g["colptr"], g["rowind"], q, k, v, stats, delta, go, scale=x["scale"], dropout=drop,
                                        results=(gk, gv))
    raw = {"out": out, "stats": stats, "delta": delta, "grad_q": gq, "grad_k": gk, "grad_v": gv}
    return raw, {k_: (t.to(dtype) if k_ in NARROW else t) for k_, t in raw.items()}


def _assert_bits(got, want, what):
    for key in KEYS:
        assert not bool(torch.isnan(got[key]).any()), "%s: a word of %s was not written" % (what, key)
        assert _bits_equal(got[key], want[key]), "%s: %s differs from the fp32 entry point%s in %d words" % (
            what, key, " narrowed once" if key in NARROW else "", int((_bits(got[key]) != _bits(want[key])).sum()))


@functools.lru_cache(maxsize=None)
def _case(name, H, F, di):
    """One case of the bit comparison, computed once: (16-bit results, unrounded fp32 oracle, narrowed oracle)."""
    dtype = DTYPES[di]
    x, g = inputs_x16(name, H, F, dtype), _graph(name)
    got = _run16(x, dtype, g)
    raw, want = _oracle(x, dtype, g)
    return got, raw, want


# ------------------------------------------------------------------------------------------------- 1. bits of the fp32 entries

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("H", HS16)
@pytest.mark.parametrize("F", FS16)
def test_bits_of_the_fp32_entry_points(pkg, F, H, di):
    """V = 1 / 2 / 4, every W from 4 to 64, one to four vectors per lane, a masked last vector (F = 130)."""
    from gespmm_amd import _lib

    V, W = geometry_x16(F)
    assert (V, W) == geometry(F)
    assert _lib.describe_dot_attention(71, 53, H, F, 100, x16=True) == _lib.describe_dot_attention(71, 53, H, F, 100) == {"V": V, "W": W}
    for name in PATTERNS:
        got, raw, want = _case(name, H, F, di)
        _assert_bits(got, want, "%s F=%d H=%d %s" % (name, F, H, IDS[di]))
        for key in NARROW:  # the rounding is witnessed (a condition on the inputs: test_dot_attention_x16_host)
            assert float((got[key].float() != raw[key]).float().mean()) > 0.5, (name, key)
        P = pattern(name)
        empty = torch.from_numpy(np.nonzero(P["degs"] == 0)[0]).cuda()
        assert empty.numel()
        for key in ("out", "stats", "delta", "grad_q"):  # an empty row writes +0 to every word
            assert int((_bits(got[key][empty]) != 0).sum()) == 0, key


def test_the_cases_reach_every_geometry():
    seen = {geometry_x16(F) for F in FS16}
    assert {v for v, _ in seen} == {1, 2, 4} and {w for _, w in seen} == {4, 8, 16, 32, 64}
    assert {-(-F // (geometry_x16(F)[0] * geometry_x16(F)[1])) for F in FS16} >= {1, 2, 3, 4}  # vectors per lane
    assert 130 % (2 * 32) != 0  # the last vector of F = 130 is masked in all lanes but one


# ------------------------------------------------------------------------------------------------- 2. off the boundary

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("offset", (2, 4, 8))
@pytest.mark.parametrize("F", (8, 20, 100, 512))
def test_operands_off_a_16_byte_boundary(pkg, F, offset, di):
    """All 16-bit operands and results 2, 4 and 8 bytes off a 16-byte boundary: V = 1, 2, 4, each with the bits of the fp32 entries
    carved at twice the offset (4, 8 and 16 bytes off)."""
    from gespmm_amd import _lib

    H, dtype = 3, DTYPES[di]
    V = offset // 2
    d16 = _lib.describe_dot_attention(71, 53, H, F, 100, offset, offset, offset, x16=True)
    a32 = min(2 * offset, 16)
    assert d16 == {"V": V, "W": geometry_x16(F)[1]} == _lib.describe_dot_attention(71, 53, H, F, 100, a32, a32, a32)
    x, g = inputs_x16("hand", H, F, dtype), _graph("hand")
    got = _run16(x, dtype, g, offset=offset)
    _, want = _oracle(x, dtype, g, offset=(2 * offset) % 16)
    _assert_bits(got, want, "hand F=%d offset=%d %s" % (F, offset, IDS[di]))


# ------------------------------------------------------------------------------------------------- 3. dropout

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("p", (0.25, 0.6))
@pytest.mark.parametrize("F,H", ((3, 3), (32, 4), (100, 1)))
def test_dropout_bits_of_the_fp32_entry_points(pkg, F, H, p, di):
    dtype = DTYPES[di]
    for name in PATTERNS:
        x, g = inputs_x16(name, H, F, dtype), _graph(name)
        got = _run16(x, dtype, g, p=p)
        _, want = _oracle(x, dtype, g, p=p)
        _assert_bits(got, want, "%s F=%d H=%d p=%g %s" % (name, F, H, p, IDS[di]))
        plain = _run16(x, dtype, g)
        assert not _bits_equal(got["out"], plain["out"])  # the mask did something


# ------------------------------------------------------------------------------------------------- 4. against float64

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("name", PATTERNS)
def test_three_launches_against_float64(pkg, name, F, H, di):
    """On the rounded inputs: stats and delta within check_all's derived tolerances; each 16-bit result within that tolerance plus
    u16 |ref| for the one rounding at its store (u16 = 2^-11 for fp16, 2^-8 for bf16; fp16: plus 2^-25, half its smallest subnormal).
    As in the fp32 test, the backward references read the device's own stats, out and delta. Nothing here is measured."""
    dtype = DTYPES[di]
    P, x, g = pattern(name), inputs_x16(name, H, F, dtype), _graph(name)
    h = {k_: t.float().cpu().numpy() for k_, t in _run16(x, dtype, g).items()}
    for key, a in h.items():
        assert not np.isnan(a).any(), "%s: a word of %s was not written" % (name, key)
    f = ref_forward(P, x)
    b = ref_backward(P, x, h["stats"], h["out"], None)
    bc = ref_backward(P, x, h["stats"], h["out"], h["delta"])

    r = {"out": ratio(h["out"], f["out"], tol16(f["out"], f["tol_out"], dtype)), "m": ratio(h["stats"][..., 0], f["m"], f["tol_m"]),
         "l": ratio(h["stats"][..., 1], f["l"], f["tol_l"]), "delta": ratio(h["delta"], b["delta"], b["tol_delta"]),
         "grad_q": ratio(h["grad_q"], b["grad_q"], tol16(b["grad_q"], b["tol_grad_q"], dtype)),
         "grad_k": ratio(h["grad_k"], bc["grad_k"], tol16(bc["grad_k"], bc["tol_grad_k"], dtype)),
         "grad_v": ratio(h["grad_v"], bc["grad_v"], tol16(bc["grad_v"], bc["tol_grad_v"], dtype))}
    print("gpu %s F=%d H=%d %s worst error / tolerance: %s" % (name, F, H, IDS[di], "  ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r


# ------------------------------------------------------------------------------------------------- 5. corner cases

@pytest.mark.parametrize("name", sorted(CHAINS))
def test_online_softmax_corner_cases(pkg, name):
    """The chain cases of test_gpu_dot_attention (a single entry, 40 ascending scores, 40 descending ones, scores of +-80) rounded to
    bf16: every result finite and bit-equal to the fp32 entry points on the widened operands; the rows around the chain are +0."""
    dtype = torch.bfloat16
    P, x = _chain_case(CHAINS[name])
    P = dict(P)
    P["colptr"], P["rowind"], P["order"] = transpose(P["rowptr"], P["colind"], P["K"])
    go = np.random.RandomState(5).uniform(0.5, 1.0, size=x["q"].shape).astype(np.float32)
    x = {"q": rounded(x["q"], dtype), "k": rounded(x["k"], dtype), "v": rounded(x["v"], dtype), "go": rounded(go, dtype), "scale": x["scale"]}
    g = _graph_of(P)
    got = _run16(x, dtype, g)
    _, want = _oracle(x, dtype, g)
    for key in KEYS:
        assert bool(torch.isfinite(got[key].float()).all()), key
    _assert_bits(got, want, "chain %s" % name)
    for key in ("out", "stats", "delta", "grad_q"):
        assert int((_bits(got[key][[0, 2]]) != 0).sum()) == 0, key
    if name == "single":
        assert _bits_equal(got["out"][1], _dev(x["v"]).to(dtype)[0]) and float(got["stats"][1, 0, 1]) == 1.0
        assert float(got["stats"][1, 0, 0]) == float(x["k"][0, 0, 0])


@pytest.mark.parametrize("di", (0, 1), ids=IDS)
def test_no_entries_zero_fills(pkg, di):
    from gespmm_amd import attention

    dtype = DTYPES[di]
    M, K, H, F = 5, 4, 2, 8
    rowptr, colptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    ind = torch.zeros(0, dtype=torch.int32, device="cuda")
    q, k, v = (torch.ones(n, H, F, dtype=dtype, device="cuda") for n in (M, K, K))
    out, gq, gk, gv = (torch.full(s, NAN, dtype=dtype, device="cuda") for s in ((M, H, F), (M, H, F), (K, H, F), (K, H, F)))
    stats, delta = torch.full((M, H, 2), NAN, device="cuda"), torch.full((M, H), NAN, device="cuda")
    for drop in (None, (0.5, _seed())):
        for t in (out, stats, delta, gq, gk, gv):
            t.fill_(NAN)
        attention.dot_attention_x16(rowptr, ind, q, k, v, dropout=drop, out=out, stats=stats)
        attention.dot_attention_backward_q_x16(rowptr, ind, q, k, v, stats, out, q, dropout=drop, results=(delta, gq))
        attention.dot_attention_backward_kv_x16(colptr, ind, q, k, v, stats, delta, q, dropout=drop, results=(gk, gv))
        for t in (out, stats, delta, gq, gk, gv):
            assert int((_bits(t) != 0).sum()) == 0  # +0 in every word


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
    q, k, v = h(M, H, F), h(K, H, F), h(K, H, F)
    out, stats, delta, gq, gk, gv = hn(M, H, F), fn(M, H, 2), fn(M, H), hn(M, H, F), hn(K, H, F), hn(K, H, F)
    calls = (lambda: attention.dot_attention_x16(g["rowptr"], g["colind"], q, k, v, out=out, stats=stats),
             lambda: attention.dot_attention_backward_q_x16(g["rowptr"], g["colind"], q, k, v, stats, out, q, results=(delta, gq)),
             lambda: attention.dot_attention_backward_kv_x16(g["colptr"], g["rowind"], q, k, v, stats, delta, q, results=(gk, gv)))
    for call in calls:
        with pytest.raises(attention.DotAttentionUnsupported) as e:
            call()
        assert e.value.code == -7 and "512" in str(e.value)
    ptr = [t.data_ptr() for t in (q, k, v)]
    rcs = (_lib.lib.gespmm_dot_attention_x16(g["rowptr"].data_ptr(), g["colind"].data_ptr(), *ptr, out.data_ptr(), stats.data_ptr(), code,
                                             M, K, H, F, P["nnz"], 1.0, None),
           _lib.lib.gespmm_dot_attention_backward_q_x16(g["rowptr"].data_ptr(), g["colind"].data_ptr(), *ptr, stats.data_ptr(),
                                                        out.data_ptr(), q.data_ptr(), delta.data_ptr(), gq.data_ptr(), code, M, K, H, F,
                                                        P["nnz"], 1.0, None),
           _lib.lib.gespmm_dot_attention_backward_kv_x16(g["colptr"].data_ptr(), g["rowind"].data_ptr(), *ptr, stats.data_ptr(),
                                                         delta.data_ptr(), q.data_ptr(), gk.data_ptr(), gv.data_ptr(), code, M, K, H, F,
                                                         P["nnz"], 1.0, None))
    torch.cuda.synchronize()
    assert rcs == (-7, -7, -7)
    for t in (out, stats, delta, gq, gk, gv):
        assert bool(torch.isnan(t).all())


# ------------------------------------------------------------------------------------------------- 6. graph capture

@pytest.mark.parametrize("di", (0, 1), ids=IDS)
@pytest.mark.parametrize("p", (None, 0.25))
def test_eager_equals_captured(pkg, p, di):
    """One stream, no parallel branches: the three launches captured, replayed twice."""
    from gespmm_amd import attention

    H, F, dtype = 4, 32, DTYPES[di]
    x, g = inputs_x16("hand", H, F, dtype), _graph("hand")
    eager = _run16(x, dtype, g, p=p)
    q, k, v, go = (_dev(x[n]).to(dtype) for n in ("q", "k", "v", "go"))
    drop = None if p is None else (p, _seed())
    M = q.shape[0]
    res = {"out": torch.empty_like(q), "stats": torch.empty(M, H, 2, device="cuda"), "delta": torch.empty(M, H, device="cuda"),
           "grad_q": torch.empty_like(q), "grad_k": torch.empty_like(k), "grad_v": torch.empty_like(k)}

    def launches():
        attention.dot_attention_x16(g["rowptr"], g["colind"], q, k, v, scale=x["scale"], dropout=drop, out=res["out"], stats=res["stats"])
        attention.dot_attention_backward_q_x16(g["rowptr"], g["colind"], q, k, v, res["stats"], res["out"], go, scale=x["scale"],
                                               dropout=drop, results=(res["delta"], res["grad_q"]))
        attention.dot_attention_backward_kv_x16(g["colptr"], g["rowind"], q, k, v, res["stats"], res["delta"], go, scale=x["scale"],
                                                dropout=drop, results=(res["grad_k"], res["grad_v"]))

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
