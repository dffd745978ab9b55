"""The fused dot-product attention on the GPU: the forward and the two backward launches against float64 within the tolerances derived
in test_dot_attention_host.py (imported unchanged, with the inputs that test shows to witness every entry), every word written, heads
and runs and captures bit for bit, dropout against the composition with softmax.edge_dropout in it, F = 513 and nnz == 0."""
import numpy as np
import pytest
import torch

from test_dot_attention_host import (F32, F64, FS, HS, SEED, _chain_case, check_all, geometry, inputs, keep_mask, pattern, ratio, ref_forward,
                                     seg_sum, transpose)

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _carved(shape, offset, fill=None):
    """A contiguous f32 device tensor whose first byte lies `offset` bytes past a 16-byte boundary (torch allocates on 256)."""
    n = int(np.prod(shape))
    buf = torch.empty(n + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset // 4: offset // 4 + n].view(shape)
    assert t.data_ptr() % 16 == offset % 16 and t.is_contiguous()
    if fill is not None:
        t.copy_(fill) if isinstance(fill, torch.Tensor) else t.fill_(fill)
    return t


def _bits_equal(a, b):
    return a.shape == b.shape and int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum()) == 0


def _graph(P):
    return {k: _dev(P[k]) for k in ("rowptr", "colind", "colptr", "rowind")}


def _seed():
    return _dev(np.array(SEED, dtype=np.uint32).view(np.int32))


def _run(P, x, p=None, offset=0, g=None):
    """The three launches on NaN-prefilled results -> dict of device tensors. offset: every dense operand and result (but stats, which
    needs 8 bytes) is carved `offset` bytes off a 16-byte boundary."""
    from gespmm_amd import attention

    g = g or _graph(P)
    q, k, v, go = (_carved(x[n].shape, offset, _dev(x[n])) for n in ("q", "k", "v", "go"))
    M, H, F = x["q"].shape
    K = x["k"].shape[0]
    nan = float("nan")
    out, gq, gk, gv = (_carved(s, offset, nan) for s in ((M, H, F), (M, H, F), (K, H, F), (K, H, F)))
    stats, delta = torch.full((M, H, 2), nan, device="cuda"), torch.full((M, H), nan, device="cuda")
    drop = None if p is None else (p, _seed())
    attention.dot_attention(g["rowptr"], g["colind"], q, k, v, scale=x["scale"], dropout=drop, out=out, stats=stats)
    attention.dot_attention_backward_q(g["rowptr"], g["colind"], q, k, v, stats, out, go, scale=x["scale"], dropout=drop, results=(delta, gq))
    attention.dot_attention_backward_kv(g["colptr"], g["rowind"], q, k, v, stats, delta, go, scale=x["scale"], dropout=drop, results=(gk, gv))
    return {"out": out, "stats": stats, "delta": delta, "grad_q": gq, "grad_k": gk, "grad_v": gv}


def _host(got):
    return {k: t.cpu().numpy() for k, t in got.items()}


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("F", FS)
def test_three_launches_against_float64(pkg, F, H):
    from gespmm_amd import _lib

    assert _lib.describe_dot_attention(71, 53, H, F, 100) == dict(zip("VW", geometry(F)))
    for name in ("hand", "random"):
        P, x = pattern(name), inputs(name, H, F)
        got = _run(P, x)
        h = _host(got)
        for key, a in h.items():
            assert not np.isnan(a).any(), "%s: a word of %s was not written" % (name, key)
        r = check_all(P, x, h, what="gpu %s F=%d H=%d" % (name, F, H))
        assert max(r.values()) <= 1.0, r
        # exact: a single-entry row is its neighbour's v, (m, l) = (s, 1); an empty row is +0 in every word
        one, none = np.nonzero(P["degs"] == 1)[0], np.nonzero(P["degs"] == 0)[0]
        assert one.size and none.size
        assert h["out"][one].tobytes() == x["v"][P["colind"][P["rowptr"][one]]].tobytes()
        assert np.all(h["stats"][one, :, 1] == 1.0)
        for key in ("out", "stats", "delta", "grad_q"):
            assert not h[key][none].any() and not np.signbit(h[key][none]).any(), key
        again = _run(P, x)
        for key in got:
            assert _bits_equal(got[key], again[key]), "second run: " + key


@pytest.mark.parametrize("H", (8, 33))
@pytest.mark.parametrize("F", (3, 32))
def test_many_heads_against_float64(pkg, F, H):
    """Head counts past the kernels' own tests (the other ops go up to 33) on the "hand" pattern, with the inputs of ``inputs()``: the
    witness condition for these (H, F) is asserted in tests/test_attention_fuzz_host.py."""
    from gespmm_amd import _lib

    assert _lib.describe_dot_attention(71, 53, H, F, 100) == dict(zip("VW", geometry(F)))
    P, x = pattern("hand"), inputs("hand", H, F)
    got = _run(P, x)
    h = _host(got)
    for key, a in h.items():
        assert not np.isnan(a).any(), "a word of %s was not written" % key
    r = check_all(P, x, h, what="gpu hand F=%d H=%d" % (F, H))
    assert max(r.values()) <= 1.0, r
    one, none = np.nonzero(P["degs"] == 1)[0], np.nonzero(P["degs"] == 0)[0]
    assert h["out"][one].tobytes() == x["v"][P["colind"][P["rowptr"][one]]].tobytes() and np.all(h["stats"][one, :, 1] == 1.0)
    for key in ("out", "stats", "delta", "grad_q"):
        assert not h[key][none].any() and not np.signbit(h[key][none]).any(), key
    again = _run(P, x)
    for key in got:
        assert _bits_equal(got[key], again[key]), "second run: " + key


_UP = np.linspace(-3, 3, 40)
CHAINS = {"single": [0.37], "ascending": _UP, "descending": _UP[::-1], "far": [-80.0, 80.0, -79.0, 0.0, 79.5, -80.0]}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_online_softmax_corner_cases_on_the_kernel(pkg, name):
    """``_chain_case`` of the host module on the kernels, held to what test_special_shapes_exact asserts of the restatement: a single
    entry (out and stats exact, the rows around it +0), 40 ascending scores (a rescale at every entry), 40 descending ones (none), and
    scores of +-80 where t underflows — and both backward launches on each, against ``ref_backward``."""
    P, x = _chain_case(CHAINS[name])
    P = dict(P)
    P["colptr"], P["rowind"], P["order"] = transpose(P["rowptr"], P["colind"], P["K"])
    x = dict(x, go=np.random.RandomState(5).uniform(0.5, 1.0, size=x["q"].shape).astype(F32))
    h = _host(_run(P, x))
    for key, a in h.items():
        assert np.isfinite(a).all(), "%s: a word of %s was not written, or is not finite" % (name, key)
    out, stats = h["out"], h["stats"]
    f = ref_forward(P, x)
    if name == "single":
        assert out[1].tobytes() == x["v"][0].tobytes() and stats[1, 0, 0] == F32(0.37) and stats[1, 0, 1] == 1.0
        assert not out[[0, 2]].any() and not stats[[0, 2]].any() and not np.signbit(out[[0, 2]]).any() and not np.signbit(stats[[0, 2]]).any()
    elif name == "far":
        assert stats[1, 0, 0] == F32(80.0)
        assert ratio(out, f["out"], f["tol_out"]) <= 1.0
    else:
        assert stats[1, 0, 0] == F32(3.0)
        assert ratio(out, f["out"], f["tol_out"]) <= 1.0 and ratio(stats[..., 1], f["l"], f["tol_l"]) <= 1.0
    r = check_all(P, x, h, what="gpu chain %s" % name)
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("F", (3, 8, 64, 100))
def test_a_head_is_the_single_head_call_on_its_slices(pkg, F):
    H = 3
    P, x = pattern("hand"), inputs("hand", H, F)
    g = _graph(P)
    got = _run(P, x, g=g)
    for hd in range(H):
        xs = {n: np.ascontiguousarray(x[n][:, hd:hd + 1]) for n in ("q", "k", "v", "go")}
        xs["scale"] = x["scale"]
        single = _run(P, xs, g=g)
        for key in got:
            assert _bits_equal(got[key][:, hd:hd + 1].contiguous(), single[key]), (F, hd, key)


@pytest.mark.parametrize("F,offset", ((8, 4), (8, 8), (20, 8), (20, 12), (100, 4), (512, 8), (512, 4)))
def test_operands_off_a_16_byte_boundary(pkg, F, offset):
    """4 (and 12) bytes off: V = 1; 8 bytes off: V = 2 — the same tolerances."""
    from gespmm_amd import _lib

    H = 3
    align = 4 if offset % 8 else 8
    V, W = geometry(F, align)
    assert V == (1 if align == 4 else 2) and _lib.describe_dot_attention(71, 53, H, F, 100, align, align, align) == {"V": V, "W": W}
    P, x = pattern("hand"), inputs("hand", H, F)
    h = _host(_run(P, x, offset=offset))
    for key, a in h.items():
        assert not np.isnan(a).any(), key
    r = check_all(P, x, h, what="gpu hand F=%d H=%d offset=%d (V=%d)" % (F, H, offset, V))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("p", (None, 0.25))
def test_eager_equals_captured(pkg, p):
    from gespmm_amd import attention

    H, F = 4, 32
    P, x = pattern("hand"), inputs("hand", H, F)
    g = _graph(P)
    eager = _run(P, x, p=p, g=g)
    q, k, v, go = (_dev(x[n]) for n in ("q", "k", "v", "go"))
    drop = None if p is None else (p, _seed())
    res = {"out": torch.empty_like(q), "stats": torch.empty(q.shape[0], H, 2, device="cuda"), "delta": torch.empty(q.shape[0], H, device="cuda"),
           "grad_q": torch.empty_like(q), "grad_k": torch.empty_like(k), "grad_v": torch.empty_like(k)}

    def launches():
        attention.dot_attention(g["rowptr"], g["colind"], q, k, v, scale=x["scale"], dropout=drop, out=res["out"], stats=res["stats"])
        attention.dot_attention_backward_q(g["rowptr"], g["colind"], q, k, v, res["stats"], res["out"], go, scale=x["scale"], dropout=drop,
                                           results=(res["delta"], res["grad_q"]))
        attention.dot_attention_backward_kv(g["colptr"], g["rowind"], q, k, v, res["stats"], res["delta"], go, scale=x["scale"],
                                            dropout=drop, results=(res["grad_k"], res["grad_v"]))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launches()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    for t in res.values():
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for key in res:
        assert _bits_equal(res[key], eager[key]), key


@pytest.mark.parametrize("p", (0.25, 0.6))
@pytest.mark.parametrize("F,H", ((3, 3), (32, 4), (100, 1)))
def test_dropout_against_float64_and_the_composition(pkg, F, H, p):
    """Fixed seed. The three launches against float64 with the restated mask; the forward against the composition
    csr_sddmm_heads -> * scale -> edge_softmax -> edge_dropout -> csr_spmm_heads, which applies the same mask: both are within the
    forward's tolerance of float64 (the composition's chains are no longer than the fused ones and its exp is the same instruction),
    so within the sum of the two of each other. A row whose entries are all dropped is exactly +0."""
    from gespmm_amd import sddmm, softmax, spmm

    P, x = pattern("hand"), inputs("hand", H, F)
    g = _graph(P)
    keep, ks = keep_mask(P, H, p)
    got = _run(P, x, p=p, g=g)
    h = _host(got)
    r = check_all(P, x, h, keep, ks, what="gpu hand F=%d H=%d p=%g" % (F, H, p))
    assert max(r.values()) <= 1.0, r
    dead = (seg_sum(keep.astype(F64), P["rowptr"]) == 0) & (P["degs"] > 0)[:, None]
    assert dead.any() and not h["out"][dead].any() and not np.signbit(h["out"][dead]).any()
    q, k, v = (_dev(x[n]) for n in ("q", "k", "v"))
    score = sddmm.csr_sddmm_heads(g["rowptr"], g["colind"], q, k) * x["scale"]
    alpha = softmax.edge_dropout(g["rowptr"], g["colind"], softmax.edge_softmax(g["rowptr"], score), p, _seed())
    assert np.array_equal(alpha.cpu().numpy() != 0, keep & (alpha.cpu().numpy() != 0)) and int((alpha != 0).sum()) > 0  # the same mask
    comp = spmm.csr_spmm_heads(g["rowptr"], g["colind"], alpha, v).cpu().numpy()
    f = ref_forward(P, x, keep, ks)
    both = ratio(h["out"], comp.astype(F64), 2 * f["tol_out"])
    print("fused against the composition, worst difference / summed tolerances: %.3g; composition against float64: %.3g"
          % (both, ratio(comp, f["out"], f["tol_out"])))
    assert both <= 1.0


def test_a_slice_of_513_floats_raises_and_launches_nothing(pkg):
    from gespmm_amd import _lib, attention

    P = pattern("random")
    g = _graph(P)
    H, F = 1, 513
    q, k, v = torch.ones(P["M"], H, F, device="cuda"), torch.ones(P["K"], H, F, device="cuda"), torch.ones(P["K"], H, F, device="cuda")
    out, stats = torch.full((P["M"], H, F), float("nan"), device="cuda"), torch.full((P["M"], H, 2), float("nan"), device="cuda")
    delta = torch.full((P["M"], H), float("nan"), device="cuda")
    calls = (lambda: attention.dot_attention(g["rowptr"], g["colind"], q, k, v, out=out, stats=stats),
             lambda: attention.dot_attention_backward_q(g["rowptr"], g["colind"], q, k, v, stats, out, q, results=(delta, out)),
             lambda: attention.dot_attention_backward_kv(g["colptr"], g["rowind"], q, k, v, stats, delta, q, results=(k.clone(), v.clone())))
    for call in calls:
        with pytest.raises(_lib.GespmmError) as e:
            call()
        assert e.value.code == -7 and "512" in str(e.value)
    rc = _lib.lib.gespmm_dot_attention_f32(g["rowptr"].data_ptr(), g["colind"].data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                                           out.data_ptr(), stats.data_ptr(), P["M"], P["K"], H, F, P["nnz"], 1.0, None)
    torch.cuda.synchronize()
    assert rc == -7 and bool(torch.isnan(out).all()) and bool(torch.isnan(stats).all()) and bool(torch.isnan(delta).all())


def test_no_entries_zero_fills(pkg):
    from gespmm_amd import attention

    M, K, H, F = 5, 4, 2, 8
    rowptr, colptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    ind = torch.zeros(0, dtype=torch.int32, device="cuda")
    q, k, v = torch.ones(M, H, F, device="cuda"), torch.ones(K, H, F, device="cuda"), torch.ones(K, H, F, device="cuda")
    nan = float("nan")
    out, stats = torch.full((M, H, F), nan, device="cuda"), torch.full((M, H, 2), nan, device="cuda")
    delta, gq = torch.full((M, H), nan, device="cuda"), torch.full((M, H, F), nan, device="cuda")
    gk, gv = torch.full((K, H, F), nan, device="cuda"), torch.full((K, H, F), nan, device="cuda")
    for drop in (None, (0.5, _seed())):
        for t in (out, stats, delta, gq, gk, gv):
            t.fill_(nan)
        attention.dot_attention(rowptr, ind, q, k, v, dropout=drop, out=out, stats=stats)
        attention.dot_attention_backward_q(rowptr, ind, q, k, v, stats, out, q, dropout=drop, results=(delta, gq))
        attention.dot_attention_backward_kv(colptr, ind, q, k, v, stats, delta, q, dropout=drop, results=(gk, gv))
        for t in (out, stats, delta, gq, gk, gv):
            assert int((t.view(torch.int32) != 0).sum()) == 0  # +0 in every word
