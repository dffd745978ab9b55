"""The multi-head product with its weights read through an edge order (``csr_spmm_heads(..., order=)``: gespmm_csr_spmm_heads_order_f32 /
_x16 / gespmm_plan_spmm_heads_order_f32) and the HIP gather behind ``graphs.take_edges`` (gespmm_edge_gather). The contract is exact: the
ordered call has the bits of the unordered call on the torch-gathered weights, on every route. Every comparison is on bit patterns, and
results are written into arrays prefilled with NaN: an element a kernel skips shows."""
import re

import numpy as np
import pytest
import torch

from helpers import bits, edge_case_csr

pytestmark = pytest.mark.gpu

# the grid of tests/test_gpu_heads.py
GRID = ((2, 1), (3, 1), (8, 1), (2, 2), (2, 3), (3, 5), (4, 4), (8, 8), (5, 13), (3, 20), (7, 6), (8, 16), (8, 22), (4, 32), (7, 27),
        (2, 64), (6, 100), (8, 64), (4, 160))
X16 = (torch.bfloat16, torch.float16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _raw(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (_raw(got) != _raw(want)).nonzero()
    assert bad.numel() == 0, (what, int(bad.shape[0]), bad[:4].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


def _carve(t, align):
    """A copy of `t` whose address `align` (16, 8, 4) divides and 2 * align (for 8, 4) does not."""
    skip = {16: 0, 8: 8 // t.element_size(), 4: 4 // t.element_size()}[align]
    buf = torch.full((t.numel() + 16,), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[skip:skip + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % align == 0 and (align == 16 or v.data_ptr() % (2 * align) != 0)
    return v


def _orders(nnz, seed):
    """A seeded random permutation and an order with repeated entries (so some rows of val are never read), both int32."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    perm = torch.randperm(nnz, device="cuda", generator=gen).to(torch.int32)
    rep = torch.randint(0, max(nnz // 3, 1), (nnz,), device="cuda", generator=gen).to(torch.int32)
    return (("perm", perm), ("repeated", rep))


def _heads(dense):
    from gespmm_amd import spmm

    return spmm.csr_spmm_heads if dense.dtype == torch.float32 else spmm.csr_spmm_heads_x16


@pytest.fixture(scope="module")
def edge(oracle):
    """The edge-case pattern — rows of 0 / 1 / 63 / 64 / 65 / 127 / 128 / 129 / 200 entries: tiles end inside, at and just past row
    ends — with ONE dense operand of the widest width (a case takes its leading H F columns) and the two orders."""
    g = edge_case_csr()
    g["B_h"] = oracle.hash_B(g["K"], 640, seed=1)
    g["rp"], g["ci"] = _dev(g["rowptr"]), _dev(g["colind"])
    g["orders"] = _orders(g["nnz"], seed=21)
    return g


def _edge_case(oracle, g, H, F):
    val_h = oracle.hash_val(g["nnz"] * H).reshape(g["nnz"], H)
    B_h = np.ascontiguousarray(g["B_h"][:, :H * F])
    return val_h, B_h, _dev(val_h), _dev(B_h)


@pytest.mark.parametrize("H,F", GRID)
def test_grid_equals_gathered_weights_and_oracle(pkg, oracle, edge, H, F):
    from gespmm_amd import _lib, spmm

    g = edge
    val_h, B_h, val, B = _edge_case(oracle, g, H, F)
    assert _lib.heads_route(g["M"], g["K"], H, F, g["nnz"])[0] == 1
    for name, order in g["orders"]:
        out = _nan(g["M"], H * F)
        assert spmm.csr_spmm_heads(g["rp"], g["ci"], val, B, out=out, order=order) is out
        _same(out, spmm.csr_spmm_heads(g["rp"], g["ci"], val[order.long()].contiguous(), B), (name, H, F))
        vo_h = np.ascontiguousarray(val_h[order.cpu().numpy()])
        ref = np.concatenate([oracle.spmm(g["rowptr"], g["colind"], np.ascontiguousarray(vo_h[:, h]),
                                          np.ascontiguousarray(B_h[:, h * F:(h + 1) * F]), "fma") for h in range(H)], axis=1)
        assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), (name, H, F)
        # rank 3 in, rank 3 out, the same numbers
        out3 = spmm.csr_spmm_heads(g["rp"], g["ci"], val, B.view(g["K"], H, F), order=order)
        assert out3.shape == (g["M"], H, F)
        _same(out3.view(g["M"], H * F), out, ("rank 3", name))
        # the order handed over with the weights, as one argument
        _same(spmm.csr_spmm_heads(g["rp"], g["ci"], spmm.OrderedValues(val, order), B), out, ("OrderedValues", name))
    with pytest.raises(ValueError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], spmm.OrderedValues(val, order), B, order=order)


def _short_rows(M, K, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    deg = torch.randint(0, 4, (M,), device="cuda", generator=gen)
    rowptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    nnz = int(rowptr[-1])
    colind = torch.randint(0, K, (nnz,), device="cuda", generator=gen).to(torch.int32)
    return {"M": M, "K": K, "nnz": nnz, "rp": rowptr, "ci": colind}


def test_every_ordered_instantiation_runs(pkg, edge):
    """An instantiation is (V, S, W) per element type: the storage-order cases of tests/test_gpu_heads.py reach the 11 geometries of
    the table; val is carved at 16 / 8 / 4 bytes so that every weight-load width runs (H = 2, 3, 4, 8 are all among the cases)."""
    from gespmm_amd import _lib

    gen = torch.Generator(device="cuda").manual_seed(11)
    big = _short_rows(1 << 17, 500, seed=3)
    big["orders"] = _orders(big["nnz"], seed=22)
    cases = [(edge, H, F, 16) for H, F in ((2, 2), (8, 1), (8, 2), (8, 4), (4, 16), (8, 16), (8, 32), (3, 24))]
    cases += [(edge, 8, 16, 8), (edge, 8, 32, 8), (edge, 8, 16, 4), (edge, 5, 13, 16), (big, 8, 40, 16)]
    assert {c[1] for c in cases} >= {2, 3, 4, 8}
    reached = {0: set(), torch.bfloat16: set(), torch.float16: set()}
    for g, H, F, align in cases:
        route, (V, S, W, rpw) = _lib.heads_route(g["M"], g["K"], H, F, g["nnz"], align, align)
        assert route == 1, (H, F, align)
        val = torch.rand(g["nnz"], H, device="cuda", generator=gen) - 0.5
        B3 = torch.rand(g["K"], H, F, device="cuda", generator=gen) - 0.5
        order = g["orders"][0][1]
        gathered = val[order.long()].contiguous()
        Bc = _carve(B3, align)
        want = _heads(Bc)(g["rp"], g["ci"], gathered, Bc, out=_carve(_nan(g["M"], H, F), align))
        for val_align in (16, 8, 4):
            out = _carve(_nan(g["M"], H, F), align)
            _heads(Bc)(g["rp"], g["ci"], _carve(val, val_align), Bc, out=out, order=order)
            _same(out, want, ("fp32", H, F, align, val_align, V, S, W))
        reached[0].add((V, S, W))
        # ... and the 16-bit forms where the width in words has a kernel: the geometry is the one of F / 2 words
        if F % 2 == 0 and align >= 8:
            for dt in X16:
                route, (V, S, W, rpw) = _lib.heads_x16_route(g["M"], g["K"], H, F, g["nnz"], align, align)
                assert route == 1
                Bx = _carve(B3.to(dt), align)
                want = _heads(Bx)(g["rp"], g["ci"], gathered, Bx, out=_carve(_nan(g["M"], H, F, dtype=dt), align))
                for val_align in (16, 4):
                    out = _carve(_nan(g["M"], H, F, dtype=dt), align)
                    _heads(Bx)(g["rp"], g["ci"], _carve(val, val_align), Bx, out=out, order=order)
                    _same(out, want, (dt, H, F, align, val_align, V, S, W))
                reached[dt].add((V, S, W))
    table = {(1, 1, 4), (1, 1, 8), (1, 1, 16), (1, 1, 32), (1, 1, 64), (4, 1, 32), (4, 1, 64), (4, 2, 64), (2, 1, 64), (2, 2, 64), (1, 2, 64)}
    assert reached[0] == table, (sorted(reached[0]), sorted(table))
    for dt in X16:  # (the same cases at half the width in words: a part of the table)
        assert reached[dt] and reached[dt] <= table, (dt, sorted(reached[dt]))


@pytest.mark.parametrize("degs", ([0, 1, 63, 64, 65, 0, 0, 127, 128, 129, 200, 2, 3, 0, 5, 31, 32, 33, 7, 0, 0], [5, 0, 200], [64, 64, 128],
                                  [3] * 40 + [330]), ids=("edge", "last-range-over-two-tiles", "nnz-multiple-of-64", "many-then-long"))
def test_guard_words(pkg, degs):
    """No entry past a wavefront's range is used, and no read can fault: ``order`` is a view whose buffer goes on with nnz .. nnz + 127,
    ``val`` a view whose buffer goes on with 128 rows of NaN. A kernel that stages — and uses — an entry past its range picks up an index
    past nnz and with it NaN; every address such an index could produce is inside the buffers."""
    M, K = len(degs), 50
    rowptr = torch.zeros(M + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.tensor(degs), 0).to(torch.int32)
    nnz = int(rowptr[-1])
    assert (nnz % 64 == 0) == (degs == [64, 64, 128])
    gen = torch.Generator(device="cuda").manual_seed(7)
    rp = rowptr.cuda()
    ci = torch.randint(0, K, (nnz,), device="cuda", generator=gen).to(torch.int32)
    obuf = torch.cat([torch.randperm(nnz, device="cuda", generator=gen), torch.arange(nnz, nnz + 128, device="cuda")]).to(torch.int32)
    order = obuf[:nnz]
    for H, F in ((2, 8), (3, 8), (4, 8), (8, 8), (8, 32)):
        vbuf = _nan(nnz + 128, H)
        vbuf[:nnz] = torch.rand(nnz, H, device="cuda", generator=gen) - 0.5
        val = vbuf[:nnz]
        assert val.is_contiguous() and order.is_contiguous()
        for dt in (torch.float32,) + X16:
            B = (torch.rand(K, H, F, device="cuda", generator=gen) - 0.5).to(dt)
            out = _nan(M, H, F, dtype=dt)
            _heads(B)(rp, ci, val, B, out=out, order=order)
            want = _heads(B)(rp, ci, val[order.long()].contiguous(), B)
            assert not bool(torch.isnan(want.float()).any())
            _same(out, want, (degs[-1], H, F, dt))
        assert bool((torch.isnan(vbuf[nnz:])).all()) and bool((obuf[nnz:] >= nnz).all())


@pytest.mark.parametrize("dt", X16, ids=("bf16", "fp16"))
def test_x16(pkg, oracle, edge, dt):
    from gespmm_amd import _lib, spmm

    g = edge
    for H, F in GRID + ((1, 128), (9, 4), (12, 3)):
        _, _, val, B32 = _edge_case(oracle, g, H, F)
        B = B32.to(dt)
        route = _lib.heads_x16_route(g["M"], g["K"], H, F, g["nnz"])[0]
        assert route == (1 if (F % 2 == 0 and 2 <= H <= 8) else 0), (H, F)  # odd F, H = 1, H = 9, H = 12: compositions
        for name, order in g["orders"]:
            out = _nan(g["M"], H * F, dtype=dt)
            spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val, B, out=out, order=order)
            _same(out, spmm.csr_spmm_heads_x16(g["rp"], g["ci"], val[order.long()].contiguous(), B), (dt, name, H, F, route))


@pytest.mark.parametrize("H,F", ((1, 128), (9, 4), (12, 3), (16, 8)))
def test_fp32_compositions(pkg, oracle, edge, H, F):
    from gespmm_amd import _lib, spmm

    g = edge
    _, _, val, B = _edge_case(oracle, g, H, F)
    assert _lib.heads_route(g["M"], g["K"], H, F, g["nnz"])[0] == 0
    for name, order in g["orders"]:
        out = _nan(g["M"], H * F)
        spmm.csr_spmm_heads(g["rp"], g["ci"], val, B, out=out, order=order)
        _same(out, spmm.csr_spmm_heads(g["rp"], g["ci"], val[order.long()].contiguous(), B), (name, H, F))


def test_route_pin(pkg, oracle, edge, monkeypatch):
    from gespmm_amd import spmm

    g = edge
    for H, F in ((2, 2), (4, 8), (8, 16), (3, 5)):
        _, _, val, B = _edge_case(oracle, g, H, F)
        order = g["orders"][0][1]
        for dense in (B, B.to(torch.bfloat16)):
            monkeypatch.delenv("GESPMM_HEADS_ORDER_ROUTE", raising=False)
            kernel = _heads(dense)(g["rp"], g["ci"], val, dense, out=_nan(g["M"], H * F, dtype=dense.dtype), order=order)
            monkeypatch.setenv("GESPMM_HEADS_ORDER_ROUTE", "composition")
            pinned = _heads(dense)(g["rp"], g["ci"], val, dense, out=_nan(g["M"], H * F, dtype=dense.dtype), order=order)
            _same(pinned, kernel, (H, F, dense.dtype))
            _same(pinned, _heads(dense)(g["rp"], g["ci"], val[order.long()].contiguous(), dense), (H, F, dense.dtype, "gathered"))


@pytest.mark.parametrize("H,F", ((2, 2), (8, 8), (9, 4)))
def test_matrix_without_entries_gives_zeros(pkg, H, F):
    """nnz == 0: the empty edge arrays — the order among them — reach the library as NULL pointers; C comes back as all +0."""
    from gespmm_amd import _lib, spmm

    M, K = 37, 11
    rp = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    ci = torch.empty(0, dtype=torch.int32, device="cuda")
    order = torch.empty(0, dtype=torch.int32, device="cuda")
    val = torch.empty(0, H, device="cuda")
    assert val.data_ptr() == 0 and order.data_ptr() == 0
    for dt in (torch.float32, torch.bfloat16):
        B = torch.rand(K, H, F, device="cuda").to(dt)
        _same(_heads(B)(rp, ci, val, B, out=_nan(M, H, F, dtype=dt), order=order), torch.zeros(M, H, F, device="cuda", dtype=dt), (H, F, dt))
    # a non-NULL order with no entries: the ladder lets it through, nothing reads it
    from helpers import cptr, cur_stream

    spare = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = _nan(M, H * F)
    rc = _lib.lib.gespmm_csr_spmm_heads_order_f32(cptr(rp), None, cptr(spare), None, None, cptr(out), M, K, H, F, 0, cur_stream())
    assert rc == 0
    _same(out, torch.zeros(M, H * F, device="cuda"), "NULL edge arrays")


@pytest.mark.parametrize("reorder", (False, True), ids=("storage-order", "clustered"))
def test_plans(pkg, bundled, reorder):
    from gespmm_amd import spmm

    g = bundled["cora"]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    gen = torch.Generator(device="cuda").manual_seed(13)
    plan = spmm.SpmmPlan(rp, ci, g["K"], 64, reorder=reorder)
    assert plan.clustered == reorder, plan.describe()
    for H, F in ((4, 8), (8, 8), (3, 5), (9, 4)):
        val = torch.rand(g["nnz"], H, device="cuda", generator=gen) - 0.5
        B = torch.rand(g["K"], H, F, device="cuda", generator=gen) - 0.5
        for name, order in _orders(g["nnz"], seed=H):
            want = spmm.csr_spmm_heads(rp, ci, val, B, order=order)
            _same(want, spmm.csr_spmm_heads(rp, ci, val[order.long()].contiguous(), B), ("no plan", name, H, F))
            _same(plan.run_heads(val, B, _nan(g["M"], H, F), order=order), want, ("run_heads", reorder, name, H, F))
            _same(spmm.csr_spmm_heads(rp, ci, val, B, plan=plan, order=order), want, ("plan=", reorder, name, H, F))
            assert re.search(r"heads H=%d F=%d route=%d " % (H, F, 1 if H <= 8 else 0), plan.describe()), plan.describe()
        _same(plan.run_heads(val, B), spmm.csr_spmm_heads(rp, ci, val, B), ("the plan without an order afterwards", H, F))


def _warm_on_side_stream(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_capture(pkg, edge, oracle):
    from gespmm_amd import _lib, spmm

    g, H, F = edge, 8, 8
    _, _, val0, B = _edge_case(oracle, g, H, F)
    (_, order0), (_, order1) = g["orders"]
    val, order = val0.clone(), order0.clone()
    for dense in (B, B.to(torch.bfloat16)):
        out = _nan(g["M"], H * F, dtype=dense.dtype)
        fn = lambda: _heads(dense)(g["rp"], g["ci"], val, dense, out=out, order=order)  # noqa: E731
        _warm_on_side_stream(fn)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # the kernel route allocates nothing
            fn()
        val.copy_(torch.flip(val0, dims=(0,)))  # new contents, same addresses
        order.copy_(order1)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _same(out, _heads(dense)(g["rp"], g["ci"], val[order.long()].contiguous(), dense), ("replay", dense.dtype))
        val.copy_(val0)
        order.copy_(order0)
    # the composition would have to allocate: refused while capturing, nothing launched
    val9 = torch.rand(g["nnz"], 9, device="cuda")
    B9 = torch.rand(g["K"], 9 * 4, device="cuda")
    out9 = torch.full((g["M"], 36), 5.0, device="cuda")
    tick = torch.zeros(8, device="cuda")
    _warm_on_side_stream(lambda: spmm.csr_spmm_heads(g["rp"], g["ci"], val9, B9, order=order0))
    caught = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick.add_(1.0)
        try:
            spmm.csr_spmm_heads(g["rp"], g["ci"], val9, B9, out=out9, order=order0)
        except _lib.GespmmError as e:
            caught.append(e)
    assert len(caught) == 1 and caught[0].code == 900, caught  # hipErrorStreamCaptureUnsupported
    graph.replay()
    torch.cuda.synchronize()
    assert bool((out9 == 5.0).all())


def test_python_errors_raise_without_launching(pkg, edge):
    from gespmm_amd import spmm

    g = edge
    val = torch.rand(g["nnz"], 4, device="cuda")
    order = g["orders"][0][1]
    for B in (torch.rand(g["K"], 4, 8, device="cuda"), torch.rand(g["K"], 4, 8, device="cuda").bfloat16()):
        out = torch.full((g["M"], 4, 8), 5.0, device="cuda", dtype=B.dtype)
        with pytest.raises(TypeError, match="convert it once"):
            _heads(B)(g["rp"], g["ci"], val, B, out=out, order=order.long())
        with pytest.raises(ValueError):
            _heads(B)(g["rp"], g["ci"], val, B, out=out, order=order[:-1].contiguous())
        with pytest.raises(ValueError):
            _heads(B)(g["rp"], g["ci"], val, B, out=out, order=order.cpu())
        with pytest.raises(ValueError):
            _heads(B)(g["rp"], g["ci"], val, B, out=out, order=torch.cat([order, order])[::2])
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())


@pytest.mark.parametrize("dt", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_autograd_reads_the_weights_through_the_order(pkg, bundled, monkeypatch, dt):
    """Both autograd functions on cora at H = 4, F = 8: the gradients are those computed with ``weight[order].contiguous()``, and the
    backward makes no permuted copy — ``graphs.take_edges`` is not called where the ordered kernel exists, and is for one head."""
    import gespmm_amd
    from gespmm_amd import _lib, graphs

    g = bundled["cora"]
    H, F = 4, 8
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    colptr, rowind, order = graphs.transpose_csr(rp, ci, g["K"], return_order=True)
    assert order.dtype == torch.int64
    route = (_lib.heads_route if dt == torch.float32 else _lib.heads_x16_route)(g["K"], g["M"], H, F, g["nnz"])[0]
    assert route == 1
    calls = []
    real = graphs.take_edges
    monkeypatch.setattr(graphs, "take_edges", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    gen = torch.Generator(device="cuda").manual_seed(3)

    def rand(*shape, dtype=torch.float32):
        return (torch.rand(*shape, device="cuda", generator=gen) - 0.5).to(dtype)

    for csc_order in (order, order.to(torch.int32)):
        feat = rand(g["K"], H, F, dtype=dt).requires_grad_(True)
        weight = rand(g["nnz"], H).requires_grad_(True)
        grad_out = rand(g["M"], H, F, dtype=dt)
        out = gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, csc_order, feat, weight, None, True)
        out.backward(grad_out)
        _same(feat.grad, _heads(grad_out)(colptr, rowind, weight.detach()[order].contiguous(), grad_out), ("grad_feat", dt))
        assert weight.grad is not None and weight.grad.shape == (g["nnz"], H)

        q, k = rand(g["M"], H, F, dtype=dt).requires_grad_(True), rand(g["K"], H, F, dtype=dt).requires_grad_(True)
        grad_s = rand(g["nnz"], H)
        s = gespmm_amd.MultiHeadSDDMMFunction.apply(rp, ci, colptr, rowind, csc_order, q, k)
        s.backward(grad_s)
        _same(k.grad, _heads(q)(colptr, rowind, grad_s[order].contiguous(), q.detach()), ("grad_k", dt))
        _same(q.grad, _heads(k)(rp, ci, grad_s, k.detach()), ("grad_q", dt))
        assert calls == [], len(calls)

    # one head has no ordered kernel: the backward gathers, as it always did, and gives the same bits
    feat = rand(g["K"], 1, F, dtype=dt).requires_grad_(True)
    weight = rand(g["nnz"], 1)
    grad_out = rand(g["M"], 1, F, dtype=dt)
    gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, feat, weight).backward(grad_out)
    assert len(calls) > 0
    _same(feat.grad, _heads(grad_out)(colptr, rowind, weight[order].contiguous(), grad_out), ("grad_feat, one head", dt))


TAKE = [((), torch.float32), ((1,), torch.float32), ((2,), torch.float32), ((3,), torch.float32), ((4,), torch.float32), ((8,), torch.float32),
        ((16,), torch.float32), ((2,), torch.bfloat16), ((8,), torch.bfloat16), ((), torch.int32),
        ((), torch.bfloat16), ((17,), torch.float32), ((2, 2), torch.float16)]  # ... and 2-byte and 68-byte rows: the index_select route


@pytest.mark.parametrize("n", (0, 1, 1000, (1 << 16) + 3))
def test_take_edges_on_the_device(pkg, n):
    from gespmm_amd import graphs

    gen = torch.Generator(device="cuda").manual_seed(n)
    for odt in (torch.int32, torch.int64):
        order = torch.randint(0, max(n, 1), (n,), device="cuda", generator=gen).to(odt)
        for tail, dt in TAKE:
            x = torch.randint(-(1 << 15), 1 << 15, (n,) + tail, device="cuda", generator=gen).to(dt)
            got = graphs.take_edges(x, order)
            assert got.is_contiguous() and got.data_ptr() != x.data_ptr() or n == 0
            _same(got, x[order.long()], (n, odt, tail, dt))
            if n > 1:  # a view 4 bytes into a buffer: the word-by-word form of the gather where rows are 16 bytes
                step = 4 // x.element_size()
                buf = torch.zeros(x.numel() + step, dtype=dt, device="cuda")
                view = buf[step:].view(x.shape)
                view.copy_(x)
                _same(graphs.take_edges(view, order), got, ("offset view", n, odt, tail, dt))
    # what stays on the index_select route gives the same bits: a non-contiguous x, and x that requires grad
    if n:
        x = torch.rand(n, 8, device="cuda", generator=gen)
        order = torch.randperm(n, device="cuda", generator=gen)
        _same(graphs.take_edges(x[:, ::2], order), x[:, ::2][order].contiguous(), "non-contiguous")
        xg = x.clone().requires_grad_(True)
        y = graphs.take_edges(xg, order)
        assert y.requires_grad
        _same(y.detach(), x[order], "requires_grad")


def test_take_edges_out_of_range_index_shows(pkg):
    """The gather never uses an index outside [0, n) as an address: that row of the result is all-ones words, every other row is right."""
    from gespmm_amd import graphs

    n = 1000
    gen = torch.Generator(device="cuda").manual_seed(5)
    for odt, bad in ((torch.int32, n), (torch.int32, -1), (torch.int64, n + 12345), (torch.int64, -(1 << 40)), (torch.int64, 1 << 33)):
        order = torch.randperm(n, device="cuda", generator=gen).to(odt)
        good = order.clone()
        order[137] = bad
        for tail, dt in (((4,), torch.float32), ((3,), torch.float32), ((8,), torch.bfloat16), ((), torch.int32)):
            x = torch.randint(0, 1 << 15, (n,) + tail, device="cuda", generator=gen).to(dt)
            got = graphs.take_edges(x, order)
            want = x[good.long()].contiguous()
            _raw(want)[137] = -1
            _same(got, want, (odt, bad, tail, dt))
            assert dt == torch.int32 or bool(torch.isnan(got[137].float()).all())
