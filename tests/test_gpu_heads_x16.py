"""Multi-head product on 16-bit features (gespmm_csr_spmm_heads_x16): fp16 / bf16 B and C, fp32 weights. The contract is exact — C has
the bits of narrow(gespmm_csr_spmm_heads_f32(val, widen(B))): one fp32 fma chain per output element in strict CSR order, rounded once at
the store — so every comparison is on bit patterns. Results are written into arrays prefilled with NaN: an element nobody writes shows."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, edge_case_csr

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
GRID = ((2, 2), (3, 2), (8, 2), (2, 4), (3, 10), (4, 8), (8, 8), (5, 26), (8, 16), (4, 32), (7, 54), (8, 32), (8, 64), (4, 160))
COMPOSED = ((1, 128), (9, 4), (4, 3), (8, 1), (16, 8))
PIN = "GESPMM_HEADS_X16_ROUTE"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(dtype, *shape):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype and got.dtype in DTYPES, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (got.contiguous().view(torch.int16) != want.contiguous().view(torch.int16)).nonzero()
    assert bad.numel() == 0, (what, int(bad.shape[0]), bad[:4].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


def _carve(t, align):
    """A copy of the 16-bit tensor `t` whose address `align` (16, 8, 4, 2) divides and 2 * align (below 16) does not."""
    skip = {16: 0, 8: 4, 4: 2, 2: 1}[align]
    buf = torch.full((t.numel() + 16,), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[skip:skip + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % align == 0 and (align == 16 or v.data_ptr() % (2 * align) != 0)
    return v


@pytest.fixture(scope="module")
def edge(oracle):
    """The edge-case pattern with ONE fp32 dense operand of the widest width (a case takes its leading H F columns, rounded to its
    dtype) and one weight array of the most heads."""
    g = edge_case_csr()
    g["B_h"] = oracle.hash_B(g["K"], 640, seed=1)
    g["val_h"] = oracle.hash_val(g["nnz"] * 16).reshape(g["nnz"], 16)
    g["rp"], g["ci"] = _dev(g["rowptr"]), _dev(g["colind"])
    return g


def _edge_case(g, H, F, dtype):
    """-> (weights on the host, weights, the 16-bit operand [K, H F])"""
    val_h = np.ascontiguousarray(g["val_h"][:, :H])
    return val_h, _dev(val_h), _dev(g["B_h"][:, :H * F]).to(dtype)


def _oracle_heads(oracle, g, val_h, B16, H, F):
    """narrow([M, H F] from the CPU restatement: each head an ordinary valued product of its WIDENED slices), narrowed by torch."""
    B_h = B16.float().cpu().numpy()
    ref = np.concatenate([oracle.spmm(g["rowptr"], g["colind"], np.ascontiguousarray(val_h[:, h]),
                                      np.ascontiguousarray(B_h[:, h * F:(h + 1) * F]), "fma") for h in range(H)], axis=1)
    return torch.from_numpy(ref).to(B16.dtype).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp16", "bf16"))
@pytest.mark.parametrize("H,F", GRID)
def test_grid_equals_oracle(pkg, oracle, edge, monkeypatch, H, F, dtype):
    from gespmm_amd import _lib, spmm

    monkeypatch.delenv(PIN, raising=False)
    g = edge
    val_h, val, B = _edge_case(g, H, F, dtype)
    route, (V, S, W, rpw) = _lib.heads_x16_route(g["M"], g["K"], H, F, g["nnz"])
    assert route == 1 and (F // 2) % V == 0, (route, V, S, W)
    out = _nan(dtype, g["M"], H * F)
    assert spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, B, out=out) is out
    _same(out, _oracle_heads(oracle, g, val_h, B, H, F), ("oracle", H, F, V, S, W))
    _same(out, spmm.csr_spmm_heads(g["rp"], g["ci"], val, B.float()).to(dtype), ("fp32 entry", H, F, V, S, W))
    # rank 3 in, rank 3 out, the same numbers
    out3 = spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, B.view(g["K"], H, F))
    assert out3.shape == (g["M"], H, F) and out3.dtype == dtype
    _same(out3.view(g["M"], H * F), out, "rank 3")
    # the pinned composition: the same bits
    monkeypatch.setenv(PIN, "composition")
    assert _lib.heads_x16_route(g["M"], g["K"], H, F, g["nnz"])[0] == 0
    _same(spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, B, out=_nan(dtype, g["M"], H * F)), out, ("pinned composition", H, F))


def _launch_table():
    """The instantiations of spmm_heads_x16.hip as {(V, S, W)}, read from the launch table itself."""
    text = open(os.path.join(ROOT, "gespmm_amd", "csrc", "spmm_heads_x16.hip")).read()
    body = text[text.index("static hipError_t launch_heads_x16_geometry"):text.index("#undef GESPMM_HEADS_X16")]
    return {(int(v), int(s_), int(w)) for v, s_, w in re.findall(r"^\s*GESPMM_HEADS_X16\((\d), (\d), (\d+)\)", body, flags=re.M)}


def _short_rows(M, K, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    deg = torch.randint(0, 4, (M,), device="cuda", generator=gen)
    rowptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    nnz = int(rowptr[-1])
    colind = torch.randint(0, K, (nnz,), device="cuda", generator=gen).to(torch.int32)
    return {"M": M, "K": K, "nnz": nnz, "rp": rowptr, "ci": colind}


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp16", "bf16"))
def test_every_instantiation_of_the_launch_table_runs(pkg, edge, monkeypatch, dtype):
    """H is a runtime argument of the kernels, so an instantiation is (V, S, W) and the element type: each is launched at least once,
    matches the fp32 entry on the widened operand, and the set reached IS the launch table of spmm_heads_x16.hip."""
    from gespmm_amd import _lib, spmm

    monkeypatch.delenv(PIN, raising=False)
    table = _launch_table()
    assert len(table) == 11, sorted(table)
    gen = torch.Generator(device="cuda").manual_seed(11)
    e = {"M": edge["M"], "K": edge["K"], "nnz": edge["nnz"], "rp": edge["rp"], "ci": edge["ci"]}
    short = _short_rows(2000, 500, seed=4)
    # two strips of four words are what the selector picks for 256 < H F / 2 <= 384 words from 2^17 rows on
    big = _short_rows(1 << 17, 500, seed=3)
    cases = [(e, H, F, 16) for H, F in ((2, 2), (2, 6), (2, 10), (2, 18), (2, 34), (2, 66), (2, 68), (2, 132), (2, 72), (2, 136))]
    cases += [(e, 8, 16, 8), (e, 8, 32, 8), (e, 8, 16, 4), (e, 8, 32, 4), (e, 5, 26, 4)]
    cases += [(short, H, F, 16) for H, F in ((2, 2), (8, 2), (8, 4), (4, 8), (8, 8), (8, 32))]
    cases += [(big, 5, 104, 16)]
    reached = set()
    for g, H, F, align in cases:
        route, (V, S, W, rpw) = _lib.heads_x16_route(g["M"], g["K"], H, F, g["nnz"], align, align)
        assert route == 1 and (F // 2) % V == 0 and 4 * V <= align, (H, F, align, V, S, W)
        val = torch.rand(g["nnz"], H, device="cuda", generator=gen) - 0.5
        B = _carve((torch.rand(g["K"], H * F, device="cuda", generator=gen) - 0.5).to(dtype), align)
        out = _carve(_nan(dtype, g["M"], H * F), align)
        spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, B, out=out)
        _same(out, spmm.csr_spmm_heads(g["rp"], g["ci"], val, B.float()).to(dtype), (H, F, align, V, S, W))
        reached.add((V, S, W))
    assert reached == table, (sorted(reached), sorted(table))


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp16", "bf16"))
def test_composition_route(pkg, oracle, edge, monkeypatch, dtype):
    """What the rule sends to the composition — H = 1, H > 8, odd F, operands that are only 2-byte aligned: the same bits."""
    from gespmm_amd import _lib, spmm

    monkeypatch.delenv(PIN, raising=False)
    g = edge
    for H, F in COMPOSED:
        val_h, val, B = _edge_case(g, H, F, dtype)
        assert _lib.heads_x16_route(g["M"], g["K"], H, F, g["nnz"])[0] == 0, (H, F)
        out = spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, B, out=_nan(dtype, g["M"], H * F))
        _same(out, _oracle_heads(oracle, g, val_h, B, H, F), ("oracle", H, F))
        _same(out, spmm.csr_spmm_heads(g["rp"], g["ci"], val, B.float()).to(dtype), ("fp32 entry", H, F))
    # 2-byte carved operands of a shape the kernel serves: B alone, C alone, both
    H, F = 4, 8
    val_h, val, B = _edge_case(g, H, F, dtype)
    want = _oracle_heads(oracle, g, val_h, B, H, F)
    for b_align, c_align in ((2, 16), (16, 2), (2, 2)):
        Bc, out = _carve(B, b_align), _carve(_nan(dtype, g["M"], H * F), c_align)
        assert _lib.heads_x16_route(g["M"], g["K"], H, F, g["nnz"], b_align, c_align)[0] == 0
        spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, Bc, out=out)
        _same(out, want, ("carved", b_align, c_align))


def _special_case(dtype):
    """Rows whose sums pin the rounding and the special values. Every row of B holds ONE value in all its columns, both heads of an
    entry carry ONE weight: -> (rowptr, colind, val[nnz, 2], B[K, 4], expected[M] as exactly representable floats / inf / nan)."""
    f16 = dtype == torch.float16
    u = 2.0 ** -10 if f16 else 2.0 ** -7          # the unit in the last place at 1
    big = 60000.0 if f16 else (2.0 - 2.0 ** -7) * 2.0 ** 127  # near the largest finite number (bf16: the largest)
    push = 60000.0 if f16 else 2.0 ** 119         # ... and what takes the sum past it at the store (bf16: exactly half a unit: a tie)
    tiny = 2.0 ** -24                             # the smallest fp16 subnormal (a normal bf16 number)
    bvals = [1.0, u / 2, u, -0.0, float("inf"), float("nan"), big, push, tiny, 0.0, -1.0]
    ONE, HALF, U, NZ, INF, NAN, BIG, PUSH, TINY, Z, M1 = range(len(bvals))
    rows = [
        ([(ONE, 1.0), (HALF, 1.0)], 1.0),                       # a tie at the store: to even (down)
        ([(ONE, 1.0), (U, 1.0), (HALF, 1.0)], 1.0 + 2 * u),     # a tie at the store: to even (up)
        ([(ONE, 1.0), (HALF, 1.0), (HALF, 1.0)], 1.0 + u),      # exact in fp32; a sum held in 16 bits would stay 1
        ([(HALF, 0.5), (ONE, 1.0), (HALF, 0.5)], 1.0),          # 1 + u / 2 in fp32: one rounding, a tie, to even
        ([(TINY, 1.0)], tiny),                                  # fp16: a subnormal in, the same subnormal out
        ([(TINY, 1024.0)], tiny * 1024.0),                      # fp16: widened exactly (2^-24 -> 2^-14)
        ([(TINY, 0.5)], 0.0),                                   # fp16: half the smallest subnormal: a tie, to even = +0
        ([(NZ, 1.0)], 0.0),                                     # fmaf(1, -0, +0) = +0
        ([(Z, -1.0), (NZ, 1.0)], 0.0),
        ([], 0.0),                                              # no entries: +0
        ([(INF, 1.0)], float("inf")),
        ([(INF, -2.0), (ONE, 1.0)], float("-inf")),
        ([(INF, 0.0)], float("nan")),
        ([(INF, 1.0), (INF, -1.0)], float("nan")),
        ([(NAN, 1.0), (ONE, 1.0)], float("nan")),
        ([(BIG, 1.0), (PUSH, 1.0)], float("inf")),              # finite in fp32, overflows at the store
        ([(BIG, -1.0), (PUSH, -1.0)], float("-inf")),
        ([(BIG, 1.0), (PUSH, 1.0), (PUSH, -1.0)], big),         # ... and the sum itself never was infinite
        ([(M1, 1.0), (HALF, 1.0)], -1.0 + u / 2),               # below 1 the spacing halves: exact
    ]
    if not f16:  # 2^-24 is a normal bf16 number: the three subnormal rows are plain products
        rows[6] = ([(TINY, 0.5)], tiny / 2)
    rowptr = np.zeros(len(rows) + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(r[0]) for r in rows])
    colind = np.array([c for r in rows for c, _ in r[0]], dtype=np.int32)
    w = np.array([x for r in rows for _, x in r[0]], dtype=np.float32)
    val = np.stack([w, w], axis=1)
    B = torch.tensor(bvals, dtype=torch.float64).to(dtype)[:, None].expand(len(bvals), 4).contiguous()
    assert torch.equal(B[:, 0].double().nan_to_num(7.0), torch.tensor(bvals, dtype=torch.float64).nan_to_num(7.0)), "not representable"
    want = torch.tensor([r[1] for r in rows], dtype=torch.float64)
    want16 = want.to(dtype)
    assert torch.equal(want16.double().nan_to_num(7.0), want.nan_to_num(7.0)), "an expected value is not representable"
    return _dev(rowptr), _dev(colind), _dev(val), B.cuda(), want16.cuda()


@pytest.mark.parametrize("route", ("kernel", "composition"))
@pytest.mark.parametrize("dtype", DTYPES, ids=("fp16", "bf16"))
def test_rounding_and_special_values(pkg, monkeypatch, dtype, route):
    from gespmm_amd import _lib, spmm

    monkeypatch.setenv(PIN, route)
    rp, ci, val, B, want = _special_case(dtype)
    M, K = rp.numel() - 1, B.shape[0]
    assert _lib.heads_x16_route(M, K, 2, 2, ci.numel())[0] == (1 if route == "kernel" else 0)
    out = spmm.csr_spmm_heads_x16(rp, ci, val, B, out=_nan(dtype, M, 4))
    nan = torch.isnan(want)
    for col in range(4):
        got = out[:, col]
        assert torch.equal(torch.isnan(got), nan), (col, got.tolist(), want.tolist())
        ok = got.view(torch.int16)[~nan] == want.view(torch.int16)[~nan]  # bit patterns: the sign of a zero counts
        assert bool(ok.all()), (col, (~ok).nonzero().flatten().tolist(), got[~nan].tolist(), want[~nan].tolist())
    # ... and the fp32 entry's result, narrowed by torch: NaN where it is NaN (the library keeps the sign and payload of the fp32 NaN,
    # torch stores its canonical one), the same bits everywhere else
    ref = spmm.csr_spmm_heads(rp, ci, val, B.float()).to(dtype)
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    keep = ~torch.isnan(ref)
    assert torch.equal(out.view(torch.int16)[keep], ref.view(torch.int16)[keep])


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp16", "bf16"))
@pytest.mark.parametrize("H,F", ((2, 2), (8, 8), (4, 32), (9, 4), (4, 3)))
def test_matrix_without_entries_gives_zero_bits(pkg, monkeypatch, H, F, dtype):
    from gespmm_amd import _lib, spmm

    monkeypatch.delenv(PIN, raising=False)
    M, K = 37, 11
    rp = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    ci = torch.empty(0, dtype=torch.int32, device="cuda")
    val = torch.empty(0, H, device="cuda")
    B = torch.rand(K, H, F, device="cuda").to(dtype)
    assert val.data_ptr() == 0 and _lib.heads_x16_route(M, K, H, F, 0)[0] == (1 if (H <= 8 and F % 2 == 0) else 0)
    out = spmm.csr_spmm_heads_x16(rp, ci, val, B, out=_nan(dtype, M, H, F))
    assert bool((out.view(torch.int16) == 0).all())
    monkeypatch.setenv(PIN, "composition")
    out = spmm.csr_spmm_heads_x16(rp, ci, val, B, out=_nan(dtype, M, H, F))
    assert bool((out.view(torch.int16) == 0).all())


def _warm_on_side_stream(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_capture(pkg, edge, monkeypatch):
    from gespmm_amd import _lib, spmm

    monkeypatch.delenv(PIN, raising=False)
    g, H, F, dtype = edge, 8, 8, torch.bfloat16
    _, val, B0 = _edge_case(g, H, F, dtype)
    assert _lib.heads_x16_route(g["M"], g["K"], H, F, g["nnz"])[0] == 1
    B = B0.clone()
    out = _nan(dtype, g["M"], H * F)
    fn = lambda: spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, B, out=out)  # noqa: E731
    _warm_on_side_stream(fn)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    B.copy_(torch.flip(B0, dims=(0,)))  # new contents, same address
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _same(out, spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, B.clone()), "replay")
    # the composition would have to allocate: refused while capturing, nothing launched
    _, val3, B3 = _edge_case(g, 4, 3, dtype)
    out3 = torch.full((g["M"], 12), 5.0, dtype=dtype, device="cuda")
    tick = torch.zeros(8, device="cuda")
    _warm_on_side_stream(lambda: spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val3, B3))
    caught = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick.add_(1.0)
        try:
            spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val3, B3, out=out3)
        except _lib.GespmmError as e:
            caught.append(e)
    assert len(caught) == 1 and caught[0].code == 900, caught  # hipErrorStreamCaptureUnsupported
    graph.replay()
    torch.cuda.synchronize()
    assert bool((out3 == 5.0).all())


def test_python_errors_raise_before_any_launch(pkg, edge):
    from gespmm_amd import spmm

    g, H, F = edge, 4, 8
    _, val, B = _edge_case(g, H, F, torch.bfloat16)
    rp, ci = g["rp"], g["ci"]
    out = torch.full((g["M"], H * F), 5.0, dtype=torch.bfloat16, device="cuda")
    f = spmm.csr_spmm_heads_x16
    for bad in (lambda: f(rp, ci, val, B.float(), out=out),                 # fp32 features: the other name
                lambda: f(rp, ci, val, B.double(), out=out),
                lambda: f(rp, ci, val.to(torch.bfloat16), B, out=out),      # edge weights stay fp32
                lambda: f(rp, ci, val.double(), B, out=out),
                lambda: f(rp.long(), ci, val, B, out=out),
                lambda: f(rp, ci.long(), val, B, out=out),
                lambda: f(rp, ci, val, B, out=out.half()),                  # mixed 16-bit dtypes
                lambda: f(rp, ci, val, B, out=out.float()),
                lambda: f(rp, ci, val, None, out=out)):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: f(rp, ci, val, B.t(), out=out),                     # not contiguous
                lambda: f(rp, ci, val.t(), B, out=out),
                lambda: f(rp, ci, val[:-1], B, out=out),                    # nnz
                lambda: f(rp, ci, val[:, :3].contiguous(), B, out=out),     # 32 columns do not hold 3 heads
                lambda: f(rp, ci, val, B.view(g["K"], 2, 16), out=out),     # rank 3 with another H
                lambda: f(rp, ci, val, B.view(-1), out=out),
                lambda: f(rp, ci, val, B, out=out[:-1]),
                lambda: f(rp, ci, val, B, out=out.view(g["M"], H, F)),      # rank of out follows dense
                lambda: f(rp[:0], ci, val, B, out=out)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    # the fp32 names keep refusing 16-bit tensors
    with pytest.raises(TypeError):
        spmm.csr_spmm_heads(rp, ci, val, B)
