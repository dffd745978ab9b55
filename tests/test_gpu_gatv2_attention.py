"""The fused GATv2 attention on the GPU: the forward and the two backward launches against float64 within the tolerances derived in
test_gatv2_attention_host.py (imported unchanged, with the inputs that test shows to witness every entry), every word written, the
score's bits against sddmm.gatv2_score, heads and runs and captures bit for bit, dropout against the restated mask, F = 513."""
import numpy as np
import pytest
import torch

from test_dot_attention_host import SEED, keep_mask, pattern, ratio, seg_sum, transpose
from test_gatv2_attention_host import F32, F64, FS, HS, chain_case, check_all, geometry, inputs, ref_forward

pytestmark = pytest.mark.gpu

KEYS = ("out", "stats", "delta", "grad_xl", "att_part", "grad_xr")


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


def _run(P, x, slope, p=None, offset=0, g=None, want=True):
    """The three launches on NaN-prefilled results -> dict of device tensors. offset: every dense operand and result (but stats, which
    needs 8 bytes) is carved `offset` bytes off a 16-byte boundary."""
    from gespmm_amd import attention

    g = g or _graph(P)
    xl, xr, att, go = (_carved(x[n].shape, offset, _dev(x[n])) for n in ("xl", "xr", "att", "go"))
    M, H, F = x["xl"].shape
    K = x["xr"].shape[0]
    nan = float("nan")
    out, gxl, part, gxr = (_carved(s, offset, nan) for s in ((M, H, F), (M, H, F), (M, H, F), (K, H, F)))
    stats, delta = torch.full((M, H, 2), nan, device="cuda"), torch.full((M, H), nan, device="cuda")
    drop = None if p is None else (p, _seed())
    attention.gatv2_attention(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope, dropout=drop, out=out, stats=stats)
    attention.gatv2_attention_backward_row(g["rowptr"], g["colind"], xl, xr, att, stats, out, go, negative_slope=slope, dropout=drop,
                                           want_att_part=want, results=(delta, gxl, part) if want else (delta, gxl))
    attention.gatv2_attention_backward_col(g["colptr"], g["rowind"], xl, xr, att, stats, delta, go, negative_slope=slope, dropout=drop,
                                           result=gxr)
    return {"out": out, "stats": stats, "delta": delta, "grad_xl": gxl, "att_part": part, "grad_xr": gxr}


def _host(got):
    return {k: t.cpu().numpy() for k, t in got.items()}


def _exact_checks(P, x, slope, h, g):
    """What holds bit for bit: the maximum of the fused scores is the maximum of sddmm.gatv2_score's, a single-entry row is its
    neighbour's xr with (m, l) = (s, 1), an empty row is +0 in every word of every row result."""
    from gespmm_amd import sddmm

    score = sddmm.gatv2_score(g["rowptr"], g["colind"], _dev(x["xl"]), _dev(x["xr"]), _dev(x["att"]), negative_slope=slope).cpu().numpy()
    m = np.zeros(h["stats"].shape[:2], F32)
    some = np.nonzero(P["degs"] > 0)[0]
    m[some] = np.maximum.reduceat(score, P["rowptr"][some], axis=0)
    assert h["stats"][..., 0].tobytes() == m.tobytes(), "stats[..., 0] is not the row maximum of gatv2_score, bit for bit"
    one, none = np.nonzero(P["degs"] == 1)[0], np.nonzero(P["degs"] == 0)[0]
    assert one.size and none.size
    assert h["out"][one].tobytes() == x["xr"][P["colind"][P["rowptr"][one]]].tobytes()
    assert np.all(h["stats"][one, :, 1] == 1.0)
    for key in ("out", "stats", "delta", "grad_xl", "att_part"):
        assert not h[key][none].any() and not np.signbit(h[key][none]).any(), key


@pytest.mark.parametrize("slope", (0.2, None))
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("F", FS)
def test_three_launches_against_float64(pkg, F, H, slope):
    from gespmm_amd import _lib

    V, W = geometry(F)
    assert _lib.describe_gatv2_attention(71, 53, H, F, 100) == {"V": V, "W": W, "supported": True}
    for name in ("hand", "random"):
        P, x = pattern(name), inputs(name, H, F)
        g = _graph(P)
        got = _run(P, x, slope, g=g)
        h = _host(got)
        for key, a in h.items():
            assert not np.isnan(a).any(), "%s: a word of %s was not written" % (name, key)
        r = check_all(P, x, slope, h, what="gpu %s F=%d H=%d slope=%s" % (name, F, H, slope))
        assert max(r.values()) <= 1.0, r
        _exact_checks(P, x, slope, h, g)
        again = _run(P, x, slope, g=g)
        for key in got:
            assert _bits_equal(got[key], again[key]), "second run: " + key


def test_many_heads_against_float64(pkg):
    """H = 33, F = 3: more heads than a wavefront has lane groups, a slice that is no multiple of a vector."""
    H, F, slope = 33, 3, 0.2
    P, x = pattern("hand"), inputs("hand", H, F)
    g = _graph(P)
    h = _host(_run(P, x, slope, g=g))
    for key, a in h.items():
        assert not np.isnan(a).any(), "a word of %s was not written" % key
    r = check_all(P, x, slope, h, what="gpu hand F=%d H=%d" % (F, H))
    assert max(r.values()) <= 1.0, r
    _exact_checks(P, x, slope, h, g)


def test_empty_columns_are_plus_zero(pkg):
    """Three columns no entry names (the last ones): every word of their grad_xr is +0, and the other results do not notice them."""
    H, F, slope = 3, 8, 0.2
    P, x = pattern("random"), inputs("random", H, F)
    P2 = dict(P, K=P["K"] + 3, colptr=np.concatenate((P["colptr"], np.full(3, P["nnz"], dtype=np.int32))))
    x2 = dict(x, xr=np.concatenate((x["xr"], np.ones((3, H, F), F32))))
    got, wide = _run(P, x, slope), _run(P2, x2, slope)
    tail = wide["grad_xr"][P["K"]:]
    assert int((tail.view(torch.int32) != 0).sum()) == 0
    for key in KEYS:
        assert _bits_equal(got[key], wide[key][:P["K"]] if key == "grad_xr" else wide[key]), key


_UP = np.linspace(-3, 3, 40)
CHAINS = {"single": [0.37], "ascending": _UP, "descending": _UP[::-1], "far": [-80.0, 80.0, -79.0, 0.0, 79.5, -80.0]}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_online_softmax_corner_cases_on_the_kernel(pkg, name):
    """``chain_case`` of the host module — the scores chosen through att and xr — on the kernels, held to what test_special_shapes_exact
    asserts of the restatement: a single entry (out and stats exact, the rows around it +0), 40 ascending scores (a rescale at every
    entry), 40 descending ones (none), and scores of +-80 where t underflows — and both backward launches on each."""
    P, x = chain_case(CHAINS[name])
    P = dict(P)
    P["colptr"], P["rowind"], P["order"] = transpose(P["rowptr"], P["colind"], P["K"])
    h = _host(_run(P, x, None))
    for key, a in h.items():
        assert np.isfinite(a).all(), "%s: a word of %s was not written, or is not finite" % (name, key)
    out, stats = h["out"], h["stats"]
    f = ref_forward(P, x, None)
    if name == "single":
        assert out[1].tobytes() == x["xr"][0].tobytes() and stats[1, 0, 0] == F32(0.37) and stats[1, 0, 1] == 1.0
        assert not out[[0, 2]].any() and not stats[[0, 2]].any() and not np.signbit(out[[0, 2]]).any() and not np.signbit(stats[[0, 2]]).any()
    elif name == "far":
        assert stats[1, 0, 0] == F32(80.0)
        assert ratio(out, f["out"], f["tol_out"]) <= 1.0
    else:
        assert stats[1, 0, 0] == F32(3.0)
        assert ratio(out, f["out"], f["tol_out"]) <= 1.0 and ratio(stats[..., 1], f["l"], f["tol_l"]) <= 1.0
    r = check_all(P, x, None, h, what="gpu chain %s" % name)
    assert max(r.values()) <= 1.0, r


def test_a_head_is_the_single_head_call_on_its_slices(pkg):
    H, F, slope = 4, 8, 0.2
    P, x = pattern("hand"), inputs("hand", H, F)
    g = _graph(P)
    got = _run(P, x, slope, g=g)
    for hd in range(H):
        xs = {n: np.ascontiguousarray(x[n][:, hd:hd + 1]) for n in ("xl", "xr", "go")}
        xs["att"] = np.ascontiguousarray(x["att"][hd:hd + 1])
        single = _run(P, xs, slope, g=g)
        for key in got:
            assert _bits_equal(got[key][:, hd:hd + 1].contiguous(), single[key]), (hd, key)


@pytest.mark.parametrize("F,offset", ((8, 4), (8, 8), (20, 8), (100, 4), (512, 8)))
def test_operands_off_a_16_byte_boundary(pkg, F, offset):
    """4 bytes off: V = 1; 8 bytes off: V = 2 — the same tolerances, and describe answers the V that ran (the restatement at that V
    is held to the same tolerances on the CPU)."""
    from gespmm_amd import _lib

    H, slope = 3, 0.2
    align = 4 if offset % 8 else 8
    V, W = geometry(F, align)
    assert V == (1 if align == 4 else 2)
    assert _lib.describe_gatv2_attention(71, 53, H, F, 100, align, align, align) == {"V": V, "W": W, "supported": True}
    P, x = pattern("hand"), inputs("hand", H, F)
    h = _host(_run(P, x, slope, offset=offset))
    for key, a in h.items():
        assert not np.isnan(a).any(), key
    r = check_all(P, x, slope, h, what="gpu hand F=%d H=%d offset=%d (V=%d)" % (F, H, offset, V))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("p", (None, 0.3))
def test_eager_equals_captured(pkg, p):
    from gespmm_amd import attention

    H, F, slope = 4, 32, 0.2
    P, x = pattern("hand"), inputs("hand", H, F)
    g = _graph(P)
    eager = _run(P, x, slope, p=p, g=g)
    xl, xr, att, go = (_dev(x[n]) for n in ("xl", "xr", "att", "go"))
    drop = None if p is None else (p, _seed())
    res = {"out": torch.empty_like(xl), "stats": torch.empty(xl.shape[0], H, 2, device="cuda"), "delta": torch.empty(xl.shape[0], H, device="cuda"),
           "grad_xl": torch.empty_like(xl), "att_part": torch.empty_like(xl), "grad_xr": torch.empty_like(xr)}

    def launches():
        attention.gatv2_attention(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope, dropout=drop, out=res["out"], stats=res["stats"])
        attention.gatv2_attention_backward_row(g["rowptr"], g["colind"], xl, xr, att, res["stats"], res["out"], go, negative_slope=slope,
                                               dropout=drop, results=(res["delta"], res["grad_xl"], res["att_part"]))
        attention.gatv2_attention_backward_col(g["colptr"], g["rowind"], xl, xr, att, res["stats"], res["delta"], go, negative_slope=slope,
                                               dropout=drop, result=res["grad_xr"])

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


@pytest.mark.parametrize("p", (0.3, 0.6))
@pytest.mark.parametrize("F,H", ((3, 3), (32, 4), (100, 1)))
def test_dropout_against_float64(pkg, F, H, p):
    """Fixed seed: the three launches against float64 with the mask of softmax.restate_edge_dropout_bits (``keep_mask``). A row whose
    entries are all dropped is exactly +0."""
    slope = 0.2
    P, x = pattern("hand"), inputs("hand", H, F)
    keep, ks = keep_mask(P, H, p)
    h = _host(_run(P, x, slope, p=p))
    for key, a in h.items():
        assert not np.isnan(a).any(), key
    r = check_all(P, x, slope, h, keep, ks, what="gpu hand F=%d H=%d p=%g" % (F, H, p))
    assert max(r.values()) <= 1.0, r
    dead = (seg_sum(keep.astype(F64), P["rowptr"]) == 0) & (P["degs"] > 0)[:, None]
    assert dead.any() and not h["out"][dead].any() and not np.signbit(h["out"][dead]).any()


@pytest.mark.parametrize("p", (None, 0.3))
def test_without_att_part_nothing_of_its_size_is_written(pkg, p):
    """want_att_part=False: delta and grad_xl have the bits of the call that asks for it, and the buffer a call WITH it writes stays as
    it was poisoned."""
    H, F, slope = 3, 20, 0.2
    P, x = pattern("hand"), inputs("hand", H, F)
    g = _graph(P)
    full = _run(P, x, slope, p=p, g=g)
    bare = _run(P, x, slope, p=p, g=g, want=False)
    assert bool(torch.isnan(bare["att_part"]).all()) and not bool(torch.isnan(full["att_part"]).any())
    for key in ("out", "stats", "delta", "grad_xl", "grad_xr"):
        assert _bits_equal(full[key], bare[key]), key


def test_a_slice_of_513_floats_raises_and_launches_nothing(pkg):
    from gespmm_amd import _lib, attention

    P = pattern("random")
    g = _graph(P)
    H, F = 1, 513
    nan = float("nan")
    xl, xr, att = torch.ones(P["M"], H, F, device="cuda"), torch.ones(P["K"], H, F, device="cuda"), torch.ones(H, F, device="cuda")
    out, stats = torch.full((P["M"], H, F), nan, device="cuda"), torch.full((P["M"], H, 2), nan, device="cuda")
    delta = torch.full((P["M"], H), nan, device="cuda")
    gxl, part = torch.full((P["M"], H, F), nan, device="cuda"), torch.full((P["M"], H, F), nan, device="cuda")
    gxr = torch.full((P["K"], H, F), nan, device="cuda")
    calls = (lambda: attention.gatv2_attention(g["rowptr"], g["colind"], xl, xr, att, out=out, stats=stats),
             lambda: attention.gatv2_attention_backward_row(g["rowptr"], g["colind"], xl, xr, att, stats, out, xl, results=(delta, gxl, part)),
             lambda: attention.gatv2_attention_backward_col(g["colptr"], g["rowind"], xl, xr, att, stats, delta, xl, result=gxr))
    for call in calls:
        with pytest.raises(_lib.GespmmError) as e:
            call()
        assert e.value.code == -7 and "512" in str(e.value)
    ptr = [t.data_ptr() for t in (g["rowptr"], g["colind"], xl, xr, att)]
    rcs = (_lib.lib.gespmm_gatv2_attention_f32(*ptr, out.data_ptr(), stats.data_ptr(), P["M"], P["K"], H, F, P["nnz"], 0.2, None),
           _lib.lib.gespmm_gatv2_attention_backward_row_f32(*ptr, stats.data_ptr(), out.data_ptr(), xl.data_ptr(), delta.data_ptr(),
                                                            gxl.data_ptr(), part.data_ptr(), P["M"], P["K"], H, F, P["nnz"], 0.2, None),
           _lib.lib.gespmm_gatv2_attention_backward_col_f32(g["colptr"].data_ptr(), g["rowind"].data_ptr(), *ptr[2:], stats.data_ptr(),
                                                            delta.data_ptr(), xl.data_ptr(), gxr.data_ptr(), P["M"], P["K"], H, F, P["nnz"],
                                                            0.2, None))
    torch.cuda.synchronize()
    assert rcs == (-7, -7, -7)
    for t in (out, stats, delta, gxl, part, gxr):
        assert bool(torch.isnan(t).all())


def test_no_entries_zero_fills(pkg):
    from gespmm_amd import attention

    M, K, H, F = 5, 4, 2, 8
    rowptr, colptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda"), torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    ind = torch.zeros(0, dtype=torch.int32, device="cuda")
    xl, xr, att = torch.ones(M, H, F, device="cuda"), torch.ones(K, H, F, device="cuda"), torch.ones(H, F, device="cuda")
    nan = float("nan")
    out, stats = torch.full((M, H, F), nan, device="cuda"), torch.full((M, H, 2), nan, device="cuda")
    delta, gxl, part = torch.full((M, H), nan, device="cuda"), torch.full((M, H, F), nan, device="cuda"), torch.full((M, H, F), nan, device="cuda")
    gxr = torch.full((K, H, F), nan, device="cuda")
    for drop in (None, (0.5, _seed())):
        for t in (out, stats, delta, gxl, part, gxr):
            t.fill_(nan)
        attention.gatv2_attention(rowptr, ind, xl, xr, att, dropout=drop, out=out, stats=stats)
        attention.gatv2_attention_backward_row(rowptr, ind, xl, xr, att, stats, out, xl, dropout=drop, results=(delta, gxl, part))
        attention.gatv2_attention_backward_col(colptr, ind, xl, xr, att, stats, delta, xl, dropout=drop, result=gxr)
        for t in (out, stats, delta, gxl, part, gxr):
            assert int((t.view(torch.int32) != 0).sum()) == 0  # +0 in every word
