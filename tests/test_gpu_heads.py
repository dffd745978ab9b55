"""Multi-head product (gespmm_csr_spmm_heads_f32 / gespmm_plan_spmm_heads_f32): H weights per edge, one fp32 fma chain per output element in
strict CSR order. The contract is exact — head h has the bits of the valued product of its slices (oracle.spmm(..., "fma"), and
spmm.csr_spmm with GESPMM_FLAG_STRICT_ORDER) — so every comparison is on bit patterns unless it says otherwise. Results are written into
arrays prefilled with NaN: an element the kernel skips shows."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, bits, edge_case_csr, sampled_rows_equal_oracle

pytestmark = pytest.mark.gpu

GRID = ((2, 1), (3, 1), (8, 1), (2, 2), (2, 3), (3, 5), (4, 4), (8, 8), (5, 13), (3, 20), (7, 6), (8, 16), (8, 22), (4, 32), (7, 27),
        (2, 64), (6, 100), (8, 64), (4, 160))
COMPOSED = ((1, 128), (9, 4), (12, 3), (16, 8))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape)
    bad = (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).nonzero()
    assert bad.numel() == 0, (what, int(bad.shape[0]), bad[:4].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


def _strict():
    from gespmm_amd import _lib

    return {"flags": _lib.FLAG_STRICT_ORDER}


def _per_head_calls(rp, ci, val, B3):
    """What a caller can do without the op: H strict-order products on contiguous slices, stacked to [M, H, F]."""
    from gespmm_amd import spmm

    H = val.shape[1]
    return torch.stack([spmm.csr_spmm(rp, ci, val[:, h].contiguous(), B3[:, h, :].contiguous(), cfg=_strict()) for h in range(H)], dim=1)


def _oracle_heads(oracle, g, val_h, B_h, H, F):
    """[M, H F] from the CPU restatement: each head an ordinary valued product of its slices."""
    return np.concatenate([oracle.spmm(g["rowptr"], g["colind"], np.ascontiguousarray(val_h[:, h]),
                                       np.ascontiguousarray(B_h[:, h * F:(h + 1) * F]), "fma") for h in range(H)], axis=1)


@pytest.fixture(scope="module")
def edge(oracle):
    """The edge-case pattern with ONE dense operand of the widest width: a case takes its leading H F columns."""
    g = edge_case_csr()
    g["B_h"] = oracle.hash_B(g["K"], 640, seed=1)
    g["rp"], g["ci"] = _dev(g["rowptr"]), _dev(g["colind"])
    return g


def _edge_case(oracle, g, H, F):
    val_h = oracle.hash_val(g["nnz"] * H).reshape(g["nnz"], H)
    B_h = np.ascontiguousarray(g["B_h"][:, :H * F])
    return val_h, B_h, _dev(val_h), _dev(B_h)


@pytest.mark.parametrize("H,F", GRID)
def test_grid_equals_oracle(pkg, oracle, edge, H, F):
    from gespmm_amd import _lib, spmm

    g = edge
    val_h, B_h, val, B = _edge_case(oracle, g, H, F)
    route, (V, S, W, rpw) = _lib.heads_route(g["M"], g["K"], H, F, g["nnz"])
    assert route == 1 and F % V == 0, (route, V, S, W)
    out = _nan(g["M"], H * F)
    assert spmm.csr_spmm_heads(g["rp"], g["ci"], val, B, out=out) is out
    ref = _oracle_heads(oracle, g, val_h, B_h, H, F)
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), (H, F, V, S, W)
    # rank 3 in, rank 3 out, the same numbers
    out3 = spmm.csr_spmm_heads(g["rp"], g["ci"], val, B.view(g["K"], H, F))
    assert out3.shape == (g["M"], H, F)
    _same(out3.view(g["M"], H * F), out, "rank 3")


def _launch_table():
    """The instantiations of spmm_heads.hip as {(V, S, W, plan_only)}, read from the launch table itself."""
    text = open(os.path.join(ROOT, "gespmm_amd", "csrc", "spmm_heads.hip")).read()
    body = text[text.index("static hipError_t launch_heads_geometry"):text.index("#undef GESPMM_HEADS")]
    common, planned = body.split("if constexpr (PLANNED)")
    table = set()
    for part, plan_only in ((common, False), (planned, True)):
        for v, s_, w in re.findall(r"^\s*GESPMM_HEADS\((\d), (\d), (\d+)\)", part, flags=re.M):
            table.add((int(v), int(s_), int(w), plan_only))
    return table


def _carve(t, align):
    """A copy of `t` whose address `align` (16, 8, 4) divides and 2 * align (for 8, 4) does not."""
    skip = {16: 0, 8: 2, 4: 1}[align]
    buf = torch.full((t.numel() + 16,), float("nan"), dtype=t.dtype, device=t.device)
    v = buf[skip:skip + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % align == 0 and (align == 16 or v.data_ptr() % (2 * align) != 0)
    return v


def _short_rows(M, K, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    deg = torch.randint(0, 4, (M,), device="cuda", generator=gen)
    rowptr = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    nnz = int(rowptr[-1])
    colind = torch.randint(0, K, (nnz,), device="cuda", generator=gen).to(torch.int32)
    return {"M": M, "K": K, "nnz": nnz, "rp": rowptr, "ci": colind, "gen": gen}


def test_every_instantiation_of_the_launch_table_runs(pkg, edge):
    """H is a runtime argument of the kernels, so an instantiation is (V, S, W) and plan mode: each is launched at least once (with
    several H), matches the per-head calls, and the set reached IS the launch table of spmm_heads.hip."""
    from gespmm_amd import _lib, spmm

    table = _launch_table()
    assert len(table) == 14 and sum(not t[3] for t in table) == 11, sorted(table)
    gen = torch.Generator(device="cuda").manual_seed(11)

    def operands(g, H, F):
        return (torch.rand(g["nnz"], H, device="cuda", generator=gen) - 0.5, torch.rand(g["K"], H, F, device="cuda", generator=gen) - 0.5)

    # ---- storage order: two strips of four floats are what the selector picks for 256 < N <= 384 from 2^17 rows on
    big = _short_rows(1 << 17, 500, seed=3)
    reached = set()
    cases = [(edge, H, F, 16) for H, F in ((2, 2), (8, 1), (8, 2), (8, 4), (4, 16), (8, 16), (8, 32), (3, 24))]
    cases += [(edge, 8, 16, 8), (edge, 8, 32, 8), (edge, 8, 16, 4), (edge, 5, 13, 16), (big, 8, 40, 16)]
    for g, H, F, align in cases:
        route, (V, S, W, rpw) = _lib.heads_route(g["M"], g["K"], H, F, g["nnz"], align, align)
        assert route == 1, (H, F, align)
        val, B3 = operands(g, H, F)
        Bc, out = _carve(B3, align), _carve(_nan(g["M"], H, F), align)
        spmm.csr_spmm_heads(g["rp"], g["ci"], val, Bc, out=out)
        _same(out, _per_head_calls(g["rp"], g["ci"], val, B3), ("storage", H, F, align, V, S, W))
        reached.add((V, S, W, False))
    assert reached == {t for t in table if not t[3]}, (sorted(reached), sorted(t for t in table if not t[3]))

    # ---- a clustered plan's task table: explicit variants stand in for what only large matrices select (four floats per lane at narrow
    # widths: plan_policy.cpp narrow_vec4); the geometry is what plan.describe() says RAN
    g = _short_rows(2000, 500, seed=4)
    planned, plans = set(), {}
    cases = [(1, H, F, 16) for H, F in ((2, 2), (8, 1), (8, 2), (8, 4), (8, 8))]                # V=1 W=4..64
    cases += [(3, H, F, 16) for H, F in ((4, 4), (8, 4), (8, 8), (8, 16), (8, 32))]             # V=4 W=4, 8, 16 (plans only), 32, 64
    cases += [(4, 8, 64, 16), (-1, 8, 16, 8), (-1, 8, 32, 8), (-1, 8, 16, 4)]                   # (4,2,64) (2,1,64) (2,2,64) (1,2,64)
    for variant, H, F, align in cases:
        if variant not in plans:
            plans[variant] = spmm.SpmmPlan(g["rp"], g["ci"], g["K"], 64, variant=variant, reorder=True, kernel="stream")
            assert plans[variant].clustered
        plan = plans[variant]
        val, B3 = operands(g, H, F)
        Bc, out = _carve(B3, align), _carve(_nan(g["M"], H, F), align)
        assert plan.heads_route(H, F, align, align) == 1, (variant, H, F, align, plan.describe())
        plan.run_heads(val, Bc, out)
        m = re.search(r"heads H=%d F=%d route=1 \(heads kernel, task table V=(\d) S=(\d) W=(\d+)\)" % (H, F), plan.describe())
        assert m, plan.describe()
        _same(out, _per_head_calls(g["rp"], g["ci"], val, B3), ("plan", variant, H, F, align))
        planned.add(tuple(int(x) for x in m.groups()))
    assert planned == {t[:3] for t in table}, (sorted(planned), sorted({t[:3] for t in table}))


@pytest.mark.parametrize("H,F", ((8, 8), (3, 5)))
def test_head_identity(pkg, edge, H, F):
    """val[p, h] = h + 1 and B = 1: every element of head h is deg(r) (h + 1), exactly — a lane that took another head's weight shows."""
    from gespmm_amd import spmm

    g = edge
    val = (torch.arange(H, dtype=torch.float32, device="cuda") + 1).repeat(g["nnz"], 1)
    out = _nan(g["M"], H, F)
    spmm.csr_spmm_heads(g["rp"], g["ci"], val, torch.ones(g["K"], H, F, device="cuda"), out=out)
    deg = torch.diff(g["rp"]).float()
    want = (deg[:, None, None] * (torch.arange(H, device="cuda").float() + 1)[None, :, None]).expand(g["M"], H, F)
    _same(out, want.contiguous(), (H, F))


@pytest.mark.parametrize("shape,H,F", (("long", 8, 8), ("long", 3, 5), ("short", 8, 4)))
def test_long_and_short_rows(pkg, oracle, shape, H, F):
    from gespmm_amd import _lib, spmm

    rng = np.random.RandomState(5)
    if shape == "long":  # one row of 1000 entries: sixteen weight tiles, the last one partial
        M, K = 1, 50
        degs = np.array([1000])
    else:  # 1000 rows of 0..3 entries: many rows per tile, tiles cut inside rows
        M, K = 1000, 50
        degs = rng.randint(0, 4, size=M)
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    g = {"M": M, "K": K, "nnz": int(rowptr[-1]), "rowptr": rowptr, "colind": rng.randint(0, K, size=int(rowptr[-1])).astype(np.int32)}
    val_h = oracle.hash_val(g["nnz"] * H).reshape(g["nnz"], H)
    B_h = oracle.hash_B(K, H * F, seed=2)
    assert _lib.heads_route(M, K, H, F, g["nnz"])[0] == 1
    out = _nan(M, H * F)
    spmm.csr_spmm_heads(_dev(rowptr), _dev(g["colind"]), _dev(val_h), _dev(B_h), out=out)
    assert np.array_equal(bits(out.cpu().numpy()), bits(_oracle_heads(oracle, g, val_h, B_h, H, F))), (shape, H, F)


@pytest.mark.parametrize("H,F", COMPOSED)
def test_composition(pkg, oracle, edge, H, F):
    from gespmm_amd import _lib, spmm

    g = edge
    val_h, B_h, val, B = _edge_case(oracle, g, H, F)
    assert _lib.heads_route(g["M"], g["K"], H, F, g["nnz"]) == (0, (0, 0, 0, 0))
    out = _nan(g["M"], H * F)
    spmm.csr_spmm_heads(g["rp"], g["ci"], val, B, out=out)
    assert np.array_equal(bits(out.cpu().numpy()), bits(_oracle_heads(oracle, g, val_h, B_h, H, F))), (H, F)


@pytest.mark.parametrize("H,F", ((8, 8), (4, 32)))
def test_alignment(pkg, oracle, edge, H, F):
    from gespmm_amd import _lib, spmm

    g = edge
    _, _, val, B = _edge_case(oracle, g, H, F)
    want = spmm.csr_spmm_heads(g["rp"], g["ci"], val, B, out=_nan(g["M"], H * F))
    V16 = _lib.heads_route(g["M"], g["K"], H, F, g["nnz"], 16, 16)[1][0]
    for align in (8, 4):
        route, (V, S, W, rpw) = _lib.heads_route(g["M"], g["K"], H, F, g["nnz"], align, align)
        assert route == 1 and V <= align // 4 and V <= V16, (align, V, V16)
        if V16 == 4:
            assert V < V16, (align, V)
        Bc, vc, out = _carve(B, align), _carve(val, align), _carve(_nan(g["M"], H * F), align)
        spmm.csr_spmm_heads(g["rp"], g["ci"], vc, Bc, out=out)
        _same(out, want, (H, F, align))


@pytest.mark.parametrize("H,F", ((8, 8), (4, 32)))
def test_pubmed(pkg, oracle, bundled, H, F):
    from gespmm_amd import _lib, spmm

    g = bundled["pubmed"]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    gen = torch.Generator(device="cuda").manual_seed(9)
    val = torch.rand(g["nnz"], H, device="cuda", generator=gen) - 0.5
    B3 = torch.rand(g["K"], H, F, device="cuda", generator=gen) - 0.5
    assert _lib.heads_route(g["M"], g["K"], H, F, g["nnz"])[0] == 1
    out = _nan(g["M"], H, F)
    spmm.csr_spmm_heads(rp, ci, val, B3, out=out)
    for h in range(H):
        assert sampled_rows_equal_oracle(oracle, rp, ci, val[:, h].contiguous(), B3[:, h, :].contiguous(), out[:, h, :].contiguous(),
                                         nrows=512, seed=h), (H, F, h)
    _same(out, _per_head_calls(rp, ci, val, B3), (H, F))


@pytest.fixture(scope="module")
def amazon():
    from gespmm_amd import graphs

    g = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda", scale=0.25)
    gen = torch.Generator(device="cuda").manual_seed(5)
    g["val"] = torch.rand(g["colind"].numel(), 16, device="cuda", generator=gen) - 0.5
    g["val2"] = torch.rand(g["colind"].numel(), 16, device="cuda", generator=gen) + 0.5
    g["B"] = torch.rand(g["K"], 64, device="cuda", generator=gen) - 0.5
    g["w1"] = torch.rand(g["colind"].numel(), device="cuda", generator=gen) - 0.5
    return g


@pytest.mark.parametrize("kernel,reorder", (("stream", True), ("auto", True), ("auto", False)))
def test_plans(pkg, oracle, amazon, kernel, reorder):
    from gespmm_amd import spmm

    g = amazon
    rp, ci, K, M = g["rowptr"], g["colind"], g["K"], g["M"]
    plan = spmm.SpmmPlan(rp, ci, K, 64, values=g["w1"], reorder=reorder, kernel=kernel)
    assert plan.clustered == bool(reorder), plan.describe()
    scalar_before = spmm.csr_spmm(rp, ci, g["w1"], g["B"], plan=plan).clone()
    for H, F in ((8, 8), (4, 16), (3, 5), (9, 4)):
        val = g["val"][:, :H].contiguous()
        B = g["B"][:, :H * F].contiguous()
        assert plan.heads_route(H, F) == (1 if H <= 8 else 0), (H, F, plan.describe())
        want = spmm.csr_spmm_heads(rp, ci, val, B, out=_nan(M, H * F))
        got = spmm.csr_spmm_heads(rp, ci, val, B, out=_nan(M, H * F), plan=plan)
        assert "heads H=%d F=%d route=%d " % (H, F, 1 if H <= 8 else 0) in plan.describe(), plan.describe()
        _same(got, want, (kernel, reorder, H, F))
        for h in (0, H - 1):
            assert sampled_rows_equal_oracle(oracle, rp, ci, val[:, h].contiguous(), B[:, h * F:(h + 1) * F].contiguous(),
                                             got[:, h * F:(h + 1) * F].contiguous(), nrows=256, seed=h), (kernel, H, F, h)
    # the weights are an argument of every call: another tensor, then the same tensor edited in place
    H, F = 8, 8
    B = g["B"]
    val2 = g["val2"][:, :H].contiguous()
    _same(plan.run_heads(val2, B, _nan(M, 64)), spmm.csr_spmm_heads(rp, ci, val2, B), "new weights")
    val2.mul_(-1.5)
    _same(plan.run_heads(val2, B, _nan(M, 64)), spmm.csr_spmm_heads(rp, ci, val2, B), "weights edited in place")
    # ... and the plan's own values are not touched by any of it
    _same(spmm.csr_spmm(rp, ci, g["w1"], B, plan=plan), scalar_before, "the plan's scalar product")


@pytest.mark.parametrize("H,F", ((2, 2), (8, 8), (4, 32), (9, 4)))
def test_matrix_without_entries_gives_zeros(pkg, H, F):
    """M > 0, nnz == 0 (an edgeless graph or mini-batch): the empty weight tensor reaches the library as a NULL pointer, and C — prefilled
    with NaN — comes back as all +0, stateless and through a plan, on the kernel route and on the composition."""
    from gespmm_amd import _lib, spmm

    M, K = 37, 11
    rp = torch.zeros(M + 1, dtype=torch.int32, device="cuda")
    ci = torch.empty(0, dtype=torch.int32, device="cuda")
    val = torch.empty(0, H, device="cuda")
    B = torch.rand(K, H, F, device="cuda")
    assert val.data_ptr() == 0 and _lib.heads_route(M, K, H, F, 0)[0] == (1 if H <= 8 else 0)
    zero = torch.zeros(M, H, F, device="cuda")
    _same(spmm.csr_spmm_heads(rp, ci, val, B, out=_nan(M, H, F)), zero, "stateless")
    for reorder in (True, False):
        plan = spmm.SpmmPlan(rp, ci, K, H * F, reorder=reorder)
        _same(plan.run_heads(val, B, _nan(M, H, F)), zero, ("plan", reorder, plan.describe()))


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
    _, _, val, B0 = _edge_case(oracle, g, H, F)
    assert _lib.heads_route(g["M"], g["K"], H, F, g["nnz"])[0] == 1
    B = B0.clone()
    out = _nan(g["M"], H * F)
    fn = lambda: spmm.csr_spmm_heads(g["rp"], g["ci"], val, B, out=out)  # noqa: E731
    _warm_on_side_stream(fn)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    B.copy_(torch.flip(B0, dims=(0,)))  # new contents, same address
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _same(out, spmm.csr_spmm_heads(g["rp"], g["ci"], val, B.clone()), "replay")
    # a composition would have to allocate: refused while capturing, nothing launched
    val9 = torch.rand(g["nnz"], 9, device="cuda")
    B9 = torch.rand(g["K"], 9 * 4, device="cuda")
    out9 = torch.full((g["M"], 36), 5.0, device="cuda")
    tick = torch.zeros(8, device="cuda")
    _warm_on_side_stream(lambda: spmm.csr_spmm_heads(g["rp"], g["ci"], val9, B9))
    caught = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick.add_(1.0)
        try:
            spmm.csr_spmm_heads(g["rp"], g["ci"], val9, B9, out=out9)
        except _lib.GespmmError as e:
            caught.append(e)
    assert len(caught) == 1 and caught[0].code == 900, caught  # hipErrorStreamCaptureUnsupported
    graph.replay()
    torch.cuda.synchronize()
    assert bool((out9 == 5.0).all())


def test_autograd(pkg, bundled, monkeypatch):
    import gespmm_amd
    from gespmm_amd import graphs, sddmm, spmm

    g = bundled["cora"]
    H, F = 4, 8
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    colptr, rowind, order = graphs.transpose_csr(rp, ci, g["K"], return_order=True)
    gen = torch.Generator(device="cuda").manual_seed(3)
    feat = (torch.rand(g["K"], H, F, device="cuda", generator=gen) - 0.5).requires_grad_(True)
    weight = (torch.rand(g["nnz"], H, device="cuda", generator=gen) - 0.5).requires_grad_(True)
    grad_out = torch.rand(g["M"], H, F, device="cuda", generator=gen) - 0.5
    calls = []
    real = sddmm.csr_sddmm
    monkeypatch.setattr(sddmm, "csr_sddmm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    out = gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, feat, weight)
    _same(out.detach(), spmm.csr_spmm_heads(rp, ci, weight.detach(), feat.detach()), "forward")
    out.backward(grad_out)
    assert len(calls) == H
    _same(feat.grad, spmm.csr_spmm_heads(colptr, rowind, weight.detach()[order].contiguous(), grad_out), "grad_feat")
    # grad_weight[e, h] = <grad_out[row(e), h, :], feat[col(e), h, :]> in float64, within the project's SDDMM rule
    rows = torch.repeat_interleave(torch.arange(g["M"], device="cuda"), torch.diff(rp).long())
    d1, d2 = grad_out[rows].double(), feat.detach()[ci.long()].double()
    ref = (d1 * d2).sum(-1)
    bound = 1e-4 * torch.maximum(ref.abs(), (d1 * d2).abs().sum(-1))
    err = (weight.grad.double() - ref).abs()
    print("grad_weight: max err %.3e, smallest bound %.3e" % (err.max().item(), bound.min().item()))
    assert weight.grad.shape == (g["nnz"], H) and bool((err <= bound).all())

    # weights that need no gradient: no SDDMM runs
    del calls[:]
    feat2 = feat.detach().clone().requires_grad_(True)
    w2 = weight.detach().clone()
    out2 = gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, feat2, w2)
    out2.backward(grad_out)
    assert calls == [] and w2.grad is None
    _same(feat2.grad, feat.grad, "grad_feat without grad_weight")

    # plans=(forward, backward): the CSR and the CSC pattern, storage order and clustered — the same bits everywhere
    for reorder in (False, True):
        plans = (spmm.SpmmPlan(rp, ci, g["K"], H * F, reorder=reorder), spmm.SpmmPlan(colptr, rowind, g["M"], H * F, reorder=reorder))
        feat3 = feat.detach().clone().requires_grad_(True)
        w3 = weight.detach().clone().requires_grad_(True)
        out3 = gespmm_amd.MultiHeadSPMMFunction.apply(rp, ci, colptr, rowind, order, feat3, w3, plans)
        _same(out3.detach(), out.detach(), ("forward through a plan", reorder))
        out3.backward(grad_out)
        assert "heads H=%d F=%d route=1" % (H, F) in plans[0].describe() and "heads H=%d F=%d route=1" % (H, F) in plans[1].describe()
        _same(feat3.grad, feat.grad, ("grad_feat through plans[1]", reorder))
        _same(w3.grad, weight.grad, ("grad_weight", reorder))


def test_python_errors_raise_without_launching(pkg, edge):
    from gespmm_amd import spmm

    g = edge
    nnz, K = g["nnz"], g["K"]
    val = torch.rand(nnz, 4, device="cuda")
    B = torch.rand(K, 4, 8, device="cuda")
    with pytest.raises(TypeError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], val.double(), B)
    with pytest.raises(TypeError):
        spmm.csr_spmm_heads(g["rp"], g["ci"].long(), val, B)
    for dt in (torch.float16, torch.bfloat16):  # 16-bit operands have no multi-head entry
        with pytest.raises(TypeError):
            spmm.csr_spmm_heads(g["rp"], g["ci"], val, B.to(dt))
    with pytest.raises(ValueError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], torch.rand(nnz, 8, device="cuda")[:, ::2], B)   # non-contiguous values
    with pytest.raises(ValueError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], val, torch.rand(K, 4, 16, device="cuda")[:, :, ::2])  # non-contiguous dense
    with pytest.raises(ValueError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], val[:-1].contiguous(), B)                       # values.shape[0] != nnz
    with pytest.raises(ValueError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], val, torch.rand(K, 30, device="cuda"))          # N not divisible by H
    with pytest.raises(ValueError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], val, torch.rand(K, 2, 16, device="cuda"))       # rank 3 with another H
    with pytest.raises(ValueError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], val.view(-1), B)                                # one weight per edge is csr_spmm's
    with pytest.raises(ValueError):
        spmm.csr_spmm_heads(g["rp"], g["ci"], val, B, out=torch.empty(g["M"], 32, device="cuda"))  # out of the other rank
