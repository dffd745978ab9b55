"""Fused GAT aggregation on 16-bit features (spmm.gat_aggregate_x16): fp16 / bf16 B and C, fp32 el, er, stats and weights.

Two references for every result. (a) A float64 restatement on the host (softmax, then product, on the widened features): every word
inside the project's bound 1e-4 max(|ref|, sum |w b|) plus the one rounding of the store. (b) The fp32 entry on the widened features,
narrowed by torch: the same BITS — one fp32 chain per element in strict entry order, rounded once. Results are written into tensors
prefilled with NaN: an element nobody writes shows."""
import numpy as np
import pytest
import torch

from attention_refs import gat_aggregate_float64, tol16
from test_gpu_heads_x16 import DTYPES, GRID, _carve, _nan, _same, _short_rows

pytestmark = pytest.mark.gpu

IDS = ("fp16", "bf16")
SLOPES = (None, 0.2)
H1 = ((1, 2), (1, 8), (1, 64))
PIN = "GESPMM_GAT_AGGREGATE_ROUTE"
# the launch table of gat_aggregate_x16.hip (launch_gat_aggregate's), as (V, S, W)
TABLE = {(1, 1, 4), (1, 1, 8), (1, 1, 16), (1, 1, 32), (1, 1, 64), (4, 1, 32), (4, 1, 64), (4, 2, 64), (2, 1, 64), (2, 2, 64), (1, 2, 64)}


def _terms(M, K, H, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(M, H, device="cuda", generator=gen) * 4 - 2), (torch.rand(K, H, device="cuda", generator=gen) * 4 - 2)


def _feat(rows, H, F, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(rows, H, F, device="cuda", generator=gen) * 2 - 1).to(dtype)


@pytest.fixture(scope="module")
def G(pkg):
    """Bipartite, 300 x 211: runs of empty rows (the first rows, the rows around multiples of 32 and 64, the last rows), rows of one
    entry, a row of 150 entries (three tiles), one of 700, a duplicate (row, column) pair — with its CSC arrays."""
    from gespmm_amd import graphs

    rng = np.random.RandomState(20261)
    M, K = 300, 211
    deg = rng.randint(0, 7, M)
    deg[rng.rand(M) < 0.15] = 1
    for a, b in ((0, 9), (30, 34), (60, 66), (127, 131), (255, 258), (290, 300)):
        deg[a:b] = 0
    deg[20], deg[100], deg[150] = 150, 700, 2
    rowptr = np.zeros(M + 1, np.int32)
    rowptr[1:] = np.cumsum(deg)
    colind = rng.randint(0, K, rowptr[-1]).astype(np.int32)
    colind[rowptr[150]:rowptr[150] + 2] = 17  # the duplicate pair (150, 17)
    g = {"M": M, "K": K, "nnz": int(rowptr[-1]), "rows_h": np.repeat(np.arange(M, dtype=np.int32), deg), "cols_h": colind, "dup": int(rowptr[150])}
    g["rp"], g["ci"] = torch.from_numpy(rowptr).cuda(), torch.from_numpy(colind).cuda()
    g["cp"], g["ri"] = graphs.transpose_csr(g["rp"], g["ci"], K)
    assert (np.diff(rowptr) == 1).any() and g["cp"].dtype == torch.int32
    return g


def _stats(g, el, er, slope):
    from gespmm_amd import softmax

    return softmax.gat_softmax_stats(g["rp"], g["ci"], el, er, negative_slope=slope)


def _run(g, el, er, st, dense, slope, transposed, dropout=None, out=None):
    """gat_aggregate_x16 into a NaN-prefilled tensor, and reference (b): the fp32 entry on the widened features, narrowed by torch."""
    from gespmm_amd import spmm

    ptr, ind = (g["cp"], g["ri"]) if transposed else (g["rp"], g["ci"])
    S = (g["cp"] if transposed else g["rp"]).numel() - 1
    out = _nan(dense.dtype, S, *dense.shape[1:]) if out is None else out
    assert spmm.gat_aggregate_x16(ptr, ind, el, er, st, dense, negative_slope=slope, transposed=transposed, out=out, dropout=dropout) is out
    want = spmm.gat_aggregate(ptr, ind, el, er, st, dense.float(), negative_slope=slope, transposed=transposed, dropout=dropout).to(dense.dtype)
    return out, want


def _inside_float64(g, el, er, dense, slope, transposed, got, what, keep=None, s=None):
    """Reference (a), printed before it is asserted."""
    ref, mag = gat_aggregate_float64(g["rows_h"], g["cols_h"], g["M"], g["K"], el.cpu().numpy(), er.cpu().numpy(),
                                     dense.float().cpu().numpy(), slope, transposed, keep, s)
    tol = tol16(ref, 1e-4 * np.maximum(np.abs(ref), mag), dense.dtype)
    err = np.abs(got.float().cpu().numpy().astype(np.float64) - ref)
    worst = float((err / np.where(tol > 0, tol, 1.0)).max())
    print("%s worst error / tolerance: %.3g" % (what, worst))
    assert np.all(err <= tol), (what, worst)  # (a NaN is outside)


# ------------------------------------------------------------------------------------------------------------------------ 1. grid

@pytest.mark.parametrize("transposed", (False, True), ids=("fwd", "T"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H,F", GRID + H1)
def test_grid(G, monkeypatch, H, F, dtype, transposed):
    from gespmm_amd import _lib

    monkeypatch.delenv(PIN, raising=False)
    route, (V, S, W, rpw) = _lib.gat_aggregate_x16_route(G["M"], G["K"], H, F, G["nnz"], transposed)
    assert route == 1 and (F // 2) % V == 0 and (V, S, W) in TABLE, (route, V, S, W)
    el, er = _terms(G["M"], G["K"], H, 100 + H)
    dense = _feat(G["M"] if transposed else G["K"], H, F, dtype, 7 * H + F)
    for slope in SLOPES:
        st = _stats(G, el, er, slope)
        out, want = _run(G, el, er, st, dense, slope, transposed)
        _inside_float64(G, el, er, dense, slope, transposed, out, (H, F, slope, transposed, V, S, W))
        _same(out, want, ("fp32 entry", H, F, slope, transposed, V, S, W))
    # rank 2 in, rank 2 out, the same numbers
    out2, _ = _run(G, el, er, st, dense.view(dense.shape[0], H * F), slope, transposed)
    _same(out2.view(out.shape), out, "rank 2")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_geometry_of_the_launch_table_runs(G, monkeypatch, dtype):
    """The grid's geometries at 16-byte operands, the two-word ones at 8-byte operands, and two strips of four words (what the selector
    picks for 256 < H F / 2 <= 384 words from 2^17 segments on): each matches the fp32 entry, and the set reached is the launch table."""
    from gespmm_amd import _lib, graphs, spmm

    monkeypatch.delenv(PIN, raising=False)
    reached = {_lib.gat_aggregate_x16_route(G["M"], G["K"], H, F, G["nnz"], t)[1][:3] for H, F in GRID + H1 for t in (False, True)}
    big = _short_rows(1 << 17, 500, seed=3)
    big["cp"], big["ri"] = graphs.transpose_csr(big["rp"], big["ci"], 500)
    for g, H, F, align, transposed in ((G, 8, 32, 8, False), (G, 8, 32, 8, True), (G, 4, 160, 8, False), (G, 4, 160, 8, True),
                                       (big, 5, 104, 16, False), (big, 5, 104, 16, True)):
        M, K = g["rp"].numel() - 1, g["cp"].numel() - 1
        route, (V, S, W, rpw) = _lib.gat_aggregate_x16_route(M, K, H, F, g["ci"].numel(), transposed, align, align)
        assert route == 1 and (F // 2) % V == 0 and 4 * V <= align, (H, F, align, V, S, W)
        el, er = _terms(M, K, H, 5)
        dense = _carve(_feat(M if transposed else K, H, F, dtype, 6), align)
        out = _carve(_nan(dtype, K if transposed else M, H, F), align)
        got, want = _run(g, el, er, _stats(g, el, er, 0.2), dense, 0.2, transposed, out=out)
        _same(got, want, (H, F, align, transposed, V, S, W))
        reached.add((V, S, W))
    assert reached == TABLE, (sorted(reached), sorted(TABLE))


# --------------------------------------------------------------------------------------------------------------------- 2. dropout

@pytest.mark.parametrize("transposed", (False, True), ids=("fwd", "T"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H,F", ((8, 8), (4, 32), (1, 64)))
def test_dropout(G, monkeypatch, H, F, dtype, transposed):
    from gespmm_amd import _lib, softmax

    monkeypatch.delenv(PIN, raising=False)
    p, seed_h = 0.5, np.array([123456789, -987654321], dtype=np.int32)
    seed = torch.from_numpy(seed_h).cuda()
    assert _lib.gat_aggregate_x16_route(G["M"], G["K"], H, F, G["nnz"], transposed)[0] == 1
    bits = softmax.restate_edge_dropout_bits(seed_h[0], seed_h[1], G["rows_h"][:, None], G["cols_h"][:, None], np.arange(H)[None, :])
    keep = bits >= _lib.edge_dropout_threshold(p)
    assert keep.any() and not keep.all() and np.array_equal(keep[G["dup"]], keep[G["dup"] + 1]), "the duplicate pair shares its decision"
    el, er = _terms(G["M"], G["K"], H, 200 + H)
    dense = _feat(G["M"] if transposed else G["K"], H, F, dtype, 9 * H + F)
    st = _stats(G, el, er, 0.2)
    out, want = _run(G, el, er, st, dense, 0.2, transposed, dropout=(p, seed))
    _inside_float64(G, el, er, dense, 0.2, transposed, out, ("dropout", H, F, transposed), keep, 1.0 / (1.0 - p))
    _same(out, want, ("fp32 dropout entry", H, F, transposed))
    assert not torch.equal(out, _run(G, el, er, st, dense, 0.2, transposed)[0]), "the mask must show"


# ----------------------------------------------------------------------------------------------------------- 3. composition route

@pytest.mark.parametrize("transposed", (False, True), ids=("fwd", "T"))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_composition_route(G, monkeypatch, dtype, transposed):
    from gespmm_amd import _lib, spmm

    monkeypatch.delenv(PIN, raising=False)
    route = lambda H, F, a=16: _lib.gat_aggregate_x16_route(G["M"], G["K"], H, F, G["nnz"], transposed, a, 16)[0]  # noqa: E731
    rows = G["M"] if transposed else G["K"]
    # odd F
    el, er = _terms(G["M"], G["K"], 4, 31)
    st = _stats(G, el, er, 0.2)
    assert route(4, 3) == 0
    _same(*_run(G, el, er, st, _feat(rows, 4, 3, dtype, 32), 0.2, transposed), "odd F")
    # a 2-byte aligned operand
    assert route(4, 8, 2) == 0 and route(4, 8) == 1
    _same(*_run(G, el, er, st, _carve(_feat(rows, 4, 8, dtype, 33), 2), 0.2, transposed), "2-byte aligned dense")
    # the pin, with and without dropout
    el, er = _terms(G["M"], G["K"], 8, 34)
    st, dense = _stats(G, el, er, None), _feat(rows, 8, 8, dtype, 35)
    seed = torch.tensor([5, 6], dtype=torch.int32, device="cuda")
    kernel = [_run(G, el, er, st, dense, None, transposed, dropout=d)[0] for d in (None, (0.5, seed))]
    monkeypatch.setenv(PIN, "composition")
    assert route(8, 8) == 0
    for k, d in zip(kernel, (None, (0.5, seed))):
        out, want = _run(G, el, er, st, dense, None, transposed, dropout=d)
        _same(out, want, ("pinned", d is not None))
        _same(out, k, ("pinned vs kernel", d is not None))
    # ... which allocates: refused on a capturing stream, nothing launched
    ptr, ind = (G["cp"], G["ri"]) if transposed else (G["rp"], G["ci"])
    out = torch.full_like(k, 5.0)
    caught = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        try:
            spmm.gat_aggregate_x16(ptr, ind, el, er, st, dense, transposed=transposed, out=out)
        except _lib.GespmmError as e:
            caught.append(e)
    assert len(caught) == 1 and caught[0].code == 900, caught  # hipErrorStreamCaptureUnsupported
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


# ----------------------------------------------------------------------------------------------------- 4. capture, special cases

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_capture_with_dropout_equals_eager(G, monkeypatch, dtype):
    from gespmm_amd import spmm

    monkeypatch.delenv(PIN, raising=False)
    H, F = 8, 8
    el, er = _terms(G["M"], G["K"], H, 41)
    st = _stats(G, el, er, 0.2)
    feat, gout = _feat(G["K"], H, F, dtype, 42), _feat(G["M"], H, F, dtype, 43)
    seed = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    out, out_t = _nan(dtype, G["M"], H, F), _nan(dtype, G["K"], H, F)

    def step():
        spmm.gat_aggregate_x16(G["rp"], G["ci"], el, er, st, feat, negative_slope=0.2, out=out, dropout=(0.5, seed))
        spmm.gat_aggregate_x16(G["cp"], G["ri"], el, er, st, gout, negative_slope=0.2, transposed=True, out=out_t, dropout=(0.5, seed))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the side stream (code objects)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for words in ((7, 8), (-9, 10), (11, 12)):
        seed.copy_(torch.tensor(words, dtype=torch.int32))
        out.fill_(float("nan"))
        out_t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _same(out, _run(G, el, er, st, feat, 0.2, False, dropout=(0.5, seed))[0], ("replay", words))
        _same(out_t, _run(G, el, er, st, gout, 0.2, True, dropout=(0.5, seed))[0], ("replay, transposed", words))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_entries_gives_zero_bits(pkg, monkeypatch, dtype):
    from gespmm_amd import spmm

    monkeypatch.delenv(PIN, raising=False)
    M, K, H = 7, 5, 3
    i0 = torch.empty(0, dtype=torch.int32, device="cuda")
    el, er, st = torch.ones(M, H, device="cuda"), torch.ones(K, H, device="cuda"), torch.zeros(M, H, 2, device="cuda")
    for F in (4, 3):  # route 1, route 0
        for transposed, S, Kb in ((False, M, K), (True, K, M)):
            out = _nan(dtype, S, H, F)
            spmm.gat_aggregate_x16(torch.zeros(S + 1, dtype=torch.int32, device="cuda"), i0, el, er, st,
                                   torch.ones(Kb, H, F, dtype=dtype, device="cuda"), transposed=transposed, out=out)
            assert bool((out.view(torch.int16) == 0).all()), (F, transposed)


def test_fp16_overflow_stores_inf(pkg, monkeypatch):
    """A softmax's weights sum to one, so a row's sum passes the largest fp16 value only through dropout's scale: a row of one entry has
    weight exactly 1, p = 0.5 doubles a kept one, and 2 * 40000 = 80000 > 65504 must be stored as inf, not as 65504."""
    from gespmm_amd import spmm

    monkeypatch.delenv(PIN, raising=False)
    M = K = 64
    rp = torch.arange(M + 1, dtype=torch.int32, device="cuda")
    ci = torch.arange(M, dtype=torch.int32, device="cuda")
    el, er = torch.zeros(M, 1, device="cuda"), torch.zeros(K, 1, device="cuda")
    st = _stats({"rp": rp, "ci": ci}, el, er, None)
    dense = torch.full((K, 1, 2), 40000.0, dtype=torch.float16, device="cuda")
    dense[:, :, 1] = -40000.0
    seed = torch.tensor([3, 4], dtype=torch.int32, device="cuda")
    out = spmm.gat_aggregate_x16(rp, ci, el, er, st, dense, dropout=(0.5, seed), out=_nan(torch.float16, M, 1, 2))
    kept = out[:, 0, 0] != 0
    assert bool(kept.any()) and not bool(kept.all())
    assert bool(torch.isposinf(out[kept][:, 0, 0]).all()) and bool(torch.isneginf(out[kept][:, 0, 1]).all()), out[kept][:2]
    assert bool((out[~kept].view(torch.int16) == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 5. Python errors

def test_python_errors_raise_before_any_launch(G):
    from gespmm_amd import spmm

    H, F = 4, 8
    el, er = _terms(G["M"], G["K"], H, 51)
    st = _stats(G, el, er, 0.2)
    feat = _feat(G["K"], H, F, torch.bfloat16, 52)
    agg = lambda *a, **kw: spmm.gat_aggregate_x16(G["rp"], G["ci"], *a, **kw)  # noqa: E731
    with pytest.raises(TypeError, match="gat_aggregate"):
        agg(el, er, st, feat.float())
    for call in (lambda: agg(el, er, st, feat, out=torch.empty(G["M"], H, F, dtype=torch.float16, device="cuda")),
                 lambda: agg(el, er, st, feat, out=torch.empty(G["M"], H, F, device="cuda")),
                 lambda: agg(el.bfloat16(), er, st, feat),
                 lambda: spmm.gat_aggregate_x16(G["rp"].long(), G["ci"], el, er, st, feat)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(TypeError):  # the fp32 op keeps refusing 16-bit operands
        spmm.gat_aggregate(G["rp"], G["ci"], el, er, st, feat)
