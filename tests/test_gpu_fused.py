"""The fused product C = ((A (col_scale . B)) . row_scale) + bias: the same bits as the unfused composition, on every route.

Each product is checked by integer compare of the fp32 bits (-0.0 != +0.0), two ways:
  1. against the GPU composition through the UNFUSED API — torch mul, spmm.csr_spmm[_no_edge_value] with the same plan or plain call,
     torch mul / add;
  2. where the unfused product is itself pinned to the oracle, against the CPU composition — float32 numpy B * col_scale[:, None], the
     oracle's SpMM, float32 numpy scale and add.
The only exception is a case with infinite scales (zero-degree rows: 0 * inf = NaN): NaN positions are compared, and the bits elsewhere.
Storage-order plans and clustered plans with an explicit streaming kernel must take the FUSED kernel (fused_route 1 or 2): the composition
alone cannot pass this file."""
import itertools

import numpy as np
import pytest
import torch

from helpers import bits, edge_case_csr

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 16, 32, 47, 64, 100, 128, 256)
SUBSETS = tuple(itertools.product((False, True), repeat=3))  # (col_scale, row_scale, bias) present


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _vectors(M, K, N, seed, special=True):
    """Scales with negative and denormal entries, a bias with -0.0 entries (host float32)."""
    rng = np.random.RandomState(seed)
    cs = rng.uniform(-2.0, 2.0, K).astype(np.float32)
    rs = rng.uniform(-2.0, 2.0, M).astype(np.float32)
    bias = rng.uniform(-1.0, 1.0, N).astype(np.float32)
    if special:
        cs[::7] = np.float32(1e-40)   # denormal
        cs[3::11] = np.float32(-3e-39)
        rs[::5] = np.float32(-1e-41)
        rs[1::9] = np.float32(0.0)
        bias[::2] = np.float32(-0.0)
    return cs, rs, bias


def _pick(subset, cs, rs, bias):
    return (cs if subset[0] else None, rs if subset[1] else None, bias if subset[2] else None)


def _unfused_gpu(spmm, rp, ci, val, B, cs, rs, bias, plan=None):
    h = B if cs is None else (B * cs.unsqueeze(1)).contiguous()
    out = spmm.csr_spmm(rp, ci, val, h, plan=plan) if val is not None else spmm.csr_spmm_no_edge_value(rp, ci, h, plan=plan)
    if rs is not None:
        out = out * rs.unsqueeze(1)
    if bias is not None:
        out = out + bias
    return out


def _unfused_cpu(oracle, g, val_h, B_h, cs, rs, bias):
    with np.errstate(all="ignore"):
        h = B_h if cs is None else (B_h * cs[:, None]).astype(np.float32)
        out = oracle.spmm(g["rowptr"], g["colind"], val_h, np.ascontiguousarray(h), "fma" if val_h is not None else "golden")
        if rs is not None:
            out = (out * rs[:, None]).astype(np.float32)
        if bias is not None:
            out = (out + bias[None, :]).astype(np.float32)
    return out


def _assert_same_bits(got, want, what, nan_positions_only=False):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape, what
    if nan_positions_only:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), what
        assert np.array_equal(bits(got)[~gn], bits(want)[~wn]), what
    else:
        bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
        assert bad.size == 0, (what, "first mismatch at", int(bad[0]), float(got.ravel()[bad[0]]), float(want.ravel()[bad[0]]), "of", bad.size)


def _small_community(M=6000, nnz=60000, seed=5):
    from gespmm_amd import graphs

    rowptr, colind, _ = graphs.community_csr(M, nnz, n_comm=300, n_groups=12, intra_deg=6, seed=seed)
    return {"M": M, "K": M, "nnz": nnz, "rowptr": rowptr.numpy().astype(np.int32), "colind": colind.numpy().astype(np.int32)}


@pytest.fixture(scope="module")
def matrices(bundled):
    return {"edge": edge_case_csr(seed=2), "pubmed": bundled["pubmed"], "community": _small_community()}


@pytest.mark.parametrize("valued", (True, False))
@pytest.mark.parametrize("name", ("edge", "pubmed", "community"))
def test_plain_call_every_width_and_every_subset(pkg, oracle, matrices, name, valued):
    from gespmm_amd import spmm

    g = matrices[name]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    val_h = oracle.hash_val(g["nnz"], seed=7) if valued else None
    val = _dev(val_h) if valued else None
    for N in WIDTHS:
        B_h = oracle.hash_B(g["K"], N, seed=N + 1)
        B = _dev(B_h)
        vh = _vectors(g["M"], g["K"], N, seed=N)
        vd = tuple(_dev(v) for v in vh)
        for subset in SUBSETS:
            cs, rs, bias = _pick(subset, *vd)
            got = spmm.csr_spmm_fused(rp, ci, val, B, col_scale=cs, row_scale=rs, bias=bias)
            _assert_same_bits(got, _unfused_gpu(spmm, rp, ci, val, B, cs, rs, bias), (name, valued, N, subset, "gpu composition"))
            if subset in ((True, True, True), (False, False, False), (True, False, False), (False, True, True)):
                _assert_same_bits(got, _unfused_cpu(oracle, g, val_h, B_h, *_pick(subset, *vh)), (name, valued, N, subset, "cpu composition"))
        # scales as columns ([K, 1] / [M, 1]: how GCNConv keeps them)
        got = spmm.csr_spmm_fused(rp, ci, val, B, col_scale=vd[0].unsqueeze(1), row_scale=vd[1].unsqueeze(1), bias=vd[2])
        _assert_same_bits(got, _unfused_gpu(spmm, rp, ci, val, B, *vd), (name, valued, N, "column-shaped scales"))


@pytest.mark.parametrize("N", (16, 64, 100, 128, 256))
def test_operands_offset_by_four_bytes(pkg, oracle, matrices, N):
    """B, C and the bias one float past a 16-byte boundary: the kernels fall back to narrower vectors, the bits stay."""
    from gespmm_amd import spmm

    g = matrices["pubmed"]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    val_h = oracle.hash_val(g["nnz"], seed=3)
    val = _dev(val_h)
    B_h = oracle.hash_B(g["K"], N, seed=N)
    cs_h, rs_h, bias_h = _vectors(g["M"], g["K"], N, seed=9)
    Bbuf = torch.empty(g["K"] * N + 1, device="cuda")
    B = Bbuf[1:].view(g["K"], N)
    B.copy_(_dev(B_h))
    Cbuf = torch.full((g["M"] * N + 1,), float("nan"), device="cuda")
    C = Cbuf[1:].view(g["M"], N)
    bbuf = torch.empty(N + 1, device="cuda")
    bias = bbuf[1:]
    bias.copy_(_dev(bias_h))
    assert B.data_ptr() % 16 == 4 and C.data_ptr() % 16 == 4 and bias.data_ptr() % 16 == 4
    cs, rs = _dev(cs_h), _dev(rs_h)
    want = _unfused_cpu(oracle, g, val_h, B_h, cs_h, rs_h, bias_h)
    spmm.csr_spmm_fused(rp, ci, val, B, col_scale=cs, row_scale=rs, bias=bias, out=C)
    _assert_same_bits(C, want, (N, "plain, offset"))
    _assert_same_bits(C, _unfused_gpu(spmm, rp, ci, val, B, cs, rs, bias), (N, "plain, offset, gpu composition"))
    for reorder in (False, True):
        plan = spmm.SpmmPlan(rp, ci, g["K"], N, values=val, reorder=reorder, kernel="stream")
        C.fill_(float("nan"))
        spmm.csr_spmm_fused(rp, ci, val, B, col_scale=cs, row_scale=rs, bias=bias, out=C, plan=plan)
        _assert_same_bits(C, want, (N, reorder, "plan, offset"))


def test_infinite_scales_of_zero_degree_rows(pkg, oracle, matrices):
    """GCN's 1 / sqrt(degree) on a matrix with empty rows and unused columns: 0 * inf = NaN, as in the unfused chain."""
    from gespmm_amd import spmm

    g = matrices["edge"]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    with np.errstate(divide="ignore"):
        rs_h = (1.0 / np.sqrt(np.diff(g["rowptr"]).astype(np.float32))).astype(np.float32)
        cs_h = (1.0 / np.sqrt(np.bincount(g["colind"], minlength=g["K"]).astype(np.float32))).astype(np.float32)
    assert np.isinf(rs_h).any()
    for N in (32, 128):
        B_h = oracle.hash_B(g["K"], N, seed=N)
        bias_h = _vectors(g["M"], g["K"], N, seed=1)[2]
        B, cs, rs, bias = _dev(B_h), _dev(cs_h), _dev(rs_h), _dev(bias_h)
        for plan in (None, spmm.SpmmPlan(rp, ci, g["K"], N, reorder=True, kernel="stream")):
            got = spmm.csr_spmm_fused(rp, ci, None, B, col_scale=cs, row_scale=rs, bias=bias, plan=plan)
            assert torch.isnan(got).any()
            _assert_same_bits(got, _unfused_gpu(spmm, rp, ci, None, B, cs, rs, bias, plan=plan), (N, plan is not None, "gpu"), nan_positions_only=True)
            _assert_same_bits(got, _unfused_cpu(oracle, g, None, B_h, cs_h, rs_h, bias_h), (N, plan is not None, "cpu"), nan_positions_only=True)


def _dense_community(rng, M, K, comm=150, deg_in=120, deg_out=40):
    """Rows in shuffled communities with ascending columns (what the column-slab tables ask for)."""
    rows = []
    ncomm = (M + comm - 1) // comm
    cols_of = [rng.choice(K, size=min(K, 6 * comm), replace=False) for _ in range(ncomm)]
    shuffle = rng.permutation(M)
    for i in range(M):
        a = rng.choice(cols_of[shuffle[i] // comm], size=rng.randint(1, 2 * deg_in))
        b = rng.randint(0, K, size=rng.randint(0, 2 * deg_out + 1))
        rows.append(np.sort(np.concatenate([a, b]).astype(np.int32), kind="stable"))
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    return {"M": M, "K": K, "nnz": int(rowptr[-1]), "rowptr": rowptr, "colind": np.concatenate(rows).astype(np.int32)}


PLAN_CASES = [(reorder, kernel) for reorder in (False, True) for kernel in ("auto", "stream", "seg-stream", "staged", "records", "staged-slabs")]


@pytest.mark.parametrize("reorder,kernel", PLAN_CASES)
def test_plans_every_kernel_choice(pkg, oracle, matrices, reorder, kernel):
    from gespmm_amd import spmm

    if kernel == "staged-slabs":
        g = _dense_community(np.random.RandomState(4), 1500, 2000)
    else:
        g = matrices["pubmed"]
    N = 32 if kernel == "records" else 128
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    val_h = oracle.hash_val(g["nnz"], seed=11)
    val = _dev(val_h)
    plan = spmm.SpmmPlan(rp, ci, g["K"], N, values=val, reorder=reorder, kernel=kernel)
    if reorder and kernel in ("staged", "records", "staged-slabs"):
        tag = {"staged": "kernel=staged-rows", "records": "kernel=padded-records", "staged-slabs": "kernel=staged-slabs"}[kernel]
        assert tag in plan.describe(), plan.describe()
    for width in (N, 64 if N == 128 else 47):
        B_h = oracle.hash_B(g["K"], width, seed=width)
        B = _dev(B_h)
        vh = _vectors(g["M"], g["K"], width, seed=width + 1)
        vd = tuple(_dev(v) for v in vh)
        # the route condition: both operands far below 4 GB, no long rows, not dense enough for cache blocking
        assert width * max(g["M"], g["K"]) * 4 < (1 << 32)
        route = plan.fused_route(width)
        assert route in (0, 1, 2)
        if not reorder or kernel in ("stream", "seg-stream"):
            assert route in (1, 2), (reorder, kernel, width, plan.describe())
        assert plan.fused_route(width, col_scale=False, row_scale=False, bias=False) == 0  # (no vector: the plain plan call)
        for use_val in (val, None):
            for subset in SUBSETS:
                cs, rs, bias = _pick(subset, *vd)
                got = spmm.csr_spmm_fused(rp, ci, use_val, B, col_scale=cs, row_scale=rs, bias=bias, plan=plan)
                what = (reorder, kernel, width, use_val is not None, subset)
                _assert_same_bits(got, _unfused_gpu(spmm, rp, ci, use_val, B, cs, rs, bias, plan=plan), what + ("gpu composition",))
                if subset == (True, True, True):
                    _assert_same_bits(got, _unfused_cpu(oracle, g, val_h if use_val is not None else None, B_h, *vh), what + ("cpu composition",))
                if subset == (False, False, False):
                    plain = spmm.csr_spmm(rp, ci, val, B, plan=plan) if use_val is not None else spmm.csr_spmm_no_edge_value(rp, ci, B, plan=plan)
                    _assert_same_bits(got, plain, what + ("empty subset == the plan call",))


def test_long_row_pass_and_64_bit_offsets_take_the_composition(pkg, oracle):
    from gespmm_amd import _lib, spmm

    rng = np.random.RandomState(8)
    M, K, N = 3000, 3000, 128
    degs = rng.randint(0, 12, M)
    degs[17] = 2600  # one hub row beyond the long-row threshold (2048 entries)
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    colind = rng.randint(0, K, int(rowptr[-1])).astype(np.int32)
    g = {"M": M, "K": K, "nnz": int(rowptr[-1]), "rowptr": rowptr, "colind": colind}
    rp, ci = _dev(rowptr), _dev(colind)
    val_h = oracle.hash_val(g["nnz"], seed=2)
    val = _dev(val_h)
    B_h = oracle.hash_B(K, N, seed=4)
    B = _dev(B_h)
    vh = _vectors(M, K, N, seed=6)
    cs, rs, bias = (_dev(v) for v in vh)
    for reorder in (False, True):
        plan = spmm.SpmmPlan(rp, ci, K, N, values=val, reorder=reorder, kernel="stream", flags=_lib.FLAG_SPLIT_LONG_ROWS)
        assert plan.fused_route(N) == 0, plan.describe()
        got = spmm.csr_spmm_fused(rp, ci, val, B, col_scale=cs, row_scale=rs, bias=bias, plan=plan)
        _assert_same_bits(got, _unfused_gpu(spmm, rp, ci, val, B, cs, rs, bias, plan=plan), (reorder, "long-row pass"))
        # the second call reuses the plan's scratch
        got2 = spmm.csr_spmm_fused(rp, ci, val, B, col_scale=cs, row_scale=rs, bias=bias, plan=plan)
        assert torch.equal(got.view(torch.int32), got2.view(torch.int32))
        plan64 = spmm.SpmmPlan(rp, ci, K, N, values=val, reorder=reorder, kernel="stream", flags=_lib.FLAG_FORCE_IDX64)
        assert plan64.fused_route(N) == 0, plan64.describe()
        got = spmm.csr_spmm_fused(rp, ci, val, B, col_scale=cs, row_scale=rs, bias=bias, plan=plan64)
        _assert_same_bits(got, _unfused_gpu(spmm, rp, ci, val, B, cs, rs, bias, plan=plan64), (reorder, "64-bit offsets, gpu"))
        _assert_same_bits(got, _unfused_cpu(oracle, g, val_h, B_h, *vh), (reorder, "64-bit offsets, cpu"))


def test_fused_plan_call_replays_from_a_graph(pkg, oracle, matrices):
    from gespmm_amd import spmm

    g = matrices["pubmed"]
    N = 128
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    val_h = oracle.hash_val(g["nnz"], seed=7)
    val = _dev(val_h)
    cs_h, rs_h, bias_h = _vectors(g["M"], g["K"], N, seed=3)
    cs, rs, bias = _dev(cs_h), _dev(rs_h), _dev(bias_h)
    B = _dev(oracle.hash_B(g["K"], N, seed=1))
    C = torch.empty((g["M"], N), device="cuda")
    from gespmm_amd import _lib

    # the fused kernel on two kinds of plan, and the composition (64-bit offsets) on scratch the warm-up calls made
    for kernel, flags, want_route in (("stream", 0, (1, 2)), ("staged", 0, (0, 1, 2)), ("stream", _lib.FLAG_FORCE_IDX64, (0,))):
        plan = spmm.SpmmPlan(rp, ci, g["K"], N, values=val, reorder=True, kernel=kernel, flags=flags)
        assert plan.fused_route(N) in want_route, plan.describe()
        fn = lambda: spmm.csr_spmm_fused(rp, ci, val, B, col_scale=cs, row_scale=rs, bias=bias, out=C, plan=plan)  # noqa: E731
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # warm-up on the side stream (code objects, the plan's scratch)
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        for seed in (2, 3):
            B_h = oracle.hash_B(g["K"], N, seed=seed)
            B.copy_(_dev(B_h))  # new contents, same address
            C.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            _assert_same_bits(C, _unfused_cpu(oracle, g, val_h, B_h, cs_h, rs_h, bias_h), (kernel, flags, seed))


def test_max_reducer_with_a_vector_is_an_error(pkg, oracle, matrices):
    from gespmm_amd import _lib, spmm

    g = matrices["edge"]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    B = _dev(oracle.hash_B(g["K"], 32, seed=1))
    cs, rs, bias = (_dev(v) for v in _vectors(g["M"], g["K"], 32, seed=1))
    plan = spmm.SpmmPlan(rp, ci, g["K"], 32, reorder=False)
    for kw in (dict(col_scale=cs), dict(row_scale=rs), dict(bias=bias)):
        for p in (None, plan):
            with pytest.raises(_lib.GespmmError) as e:
                spmm.csr_spmm_fused(rp, ci, None, B, plan=p, reduce_max=-10000.0, **kw)
            assert e.value.code == -1
    # without a vector it is the max reducer
    got = spmm.csr_spmm_fused(rp, ci, None, B, reduce_max=-10000.0)
    assert torch.equal(got, spmm.csr_spmm_max(rp, ci, B, -10000.0))
