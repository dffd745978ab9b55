"""16-bit dense operands (fp16 / bf16 B and C, fp32 sum, ONE rounding at the store) — gespmm_csr_spmm_x16 / gespmm_plan_spmm_x16.

The contract (include/gespmm.h): C16 == narrow(fp32 product of widen(B16)), bit for bit, wherever the fp32 route is a strict chain; where
the fp32 route re-associates (long-row pass) the 16-bit call re-associates identically. `widen` / `narrow` on the host are torch's
``.float()`` / ``.to(dtype)``. Every test compares bits (NaN by isnan)."""
import numpy as np
import pytest
import torch

from helpers import edge_case_csr

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
KERNEL_WIDTHS = (2, 6, 8, 16, 24, 32, 40, 64, 72, 128, 136, 256, 264, 520)
COMPOSED_WIDTHS = (1, 3, 41, 47)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w), what
    a = torch.where(nan_g, torch.zeros_like(got), got).view(torch.int16)
    b = torch.where(nan_w, torch.zeros_like(want), want).view(torch.int16)
    bad = (a != b).nonzero()
    assert bad.numel() == 0, (what, bad[:4].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


def _route(_lib, M, K, N, nnz, b_align=16, c_align=16, variant=-1):
    return _lib.lib.gespmm_x16_route(M, K, N, nnz, variant, b_align, c_align)


def _call(spmm, rp, ci, val, B, **kw):
    return spmm.csr_spmm(rp, ci, val, B, **kw) if val is not None else spmm.csr_spmm_no_edge_value(rp, ci, B, **kw)


@pytest.fixture(scope="module")
def edge(oracle):
    """The edge-case graph with ONE fp32 B of the widest width (narrower tests take its leading columns) and its values."""
    g = edge_case_csr()
    g["val_h"] = oracle.hash_val(g["nnz"], seed=7)
    g["B_h"] = oracle.hash_B(g["K"], max(KERNEL_WIDTHS), seed=1)
    g["rp"], g["ci"], g["val"] = _dev(g["rowptr"]), _dev(g["colind"]), _dev(g["val_h"])
    return g


@pytest.mark.parametrize("dt", ("f16", "bf16"))
@pytest.mark.parametrize("valued", (True, False))
def test_width_sweep_bits_equal_oracle_and_fp32_call(pkg, oracle, edge, dt, valued):
    import ctypes

    from gespmm_amd import _lib, spmm

    g, dtype = edge, DT[dt]
    val, val_h = (g["val"], g["val_h"]) if valued else (None, None)
    reached = set()
    buf = ctypes.create_string_buffer(300)
    for N in KERNEL_WIDTHS + COMPOSED_WIDTHS:
        B16 = _dev(g["B_h"][:, :N]).to(dtype)
        want_route = 0 if N in COMPOSED_WIDTHS else 1
        assert _route(_lib, g["M"], g["K"], N, g["nnz"]) == want_route, N
        got = _call(spmm, g["rp"], g["ci"], val, B16)
        assert got.dtype == dtype
        ref = oracle.spmm(g["rowptr"], g["colind"], val_h, B16.float().cpu().numpy(), "fma" if valued else "golden")
        _same_bits(got, torch.from_numpy(ref).to(dtype).cuda(), (dt, valued, N, "oracle"))
        _same_bits(got, _call(spmm, g["rp"], g["ci"], val, B16.float()).to(dtype), (dt, valued, N, "fp32 call"))
        if want_route:
            _lib.lib.gespmm_describe_launch(g["M"], g["K"], N // 2, g["nnz"], -1, None, buf, 300)
            d = dict(kv.split("=") for kv in buf.value.decode().split() if "=" in kv)
            assert d["kernel"] == "batch-stream", buf.value
            reached.add((int(d["V"]), int(d["S"]), int(d["W"])))
    # the batch-stream geometries the selector reaches on this graph with 16-byte operands; the WHOLE launch table (two strips, narrower
    # vectors, segmented, plan-only) is covered and asserted by test_every_instantiation_of_the_launch_table_runs
    assert reached == {(1, 1, 4), (1, 1, 8), (1, 1, 16), (1, 1, 32), (1, 1, 64), (4, 1, 32), (4, 1, 64)}, reached


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_alignment_and_neighbours(pkg, edge, dt):
    """B and C carved at 16-, 8-, 4- and 2-byte offsets: the route follows the alignment, the bits do not, and a narrowing store never
    spills past its matrix."""
    from gespmm_amd import _lib, spmm

    g, dtype = edge, DT[dt]
    for N in (128, 24, 264):
        B_full = _dev(g["B_h"][:, :N]).to(dtype)
        want = spmm.csr_spmm(g["rp"], g["ci"], g["val"], B_full.float()).to(dtype)
        for align, skip in ((16, 8), (8, 4), (4, 2), (2, 1)):  # elements skipped from a 256-byte aligned base
            bbuf = torch.zeros(g["K"] * N + 64, dtype=dtype, device="cuda")
            cbuf = torch.full((g["M"] * N + 64,), 123.0, dtype=dtype, device="cuda")
            B = bbuf[skip:skip + g["K"] * N].view(g["K"], N)
            C = cbuf[skip:skip + g["M"] * N].view(g["M"], N)
            B.copy_(B_full)
            assert B.data_ptr() % align == 0 and B.data_ptr() % (2 * align) != 0
            assert _route(_lib, g["M"], g["K"], N, g["nnz"], align, align) == (0 if align == 2 else 1), (N, align)
            got = spmm.csr_spmm(g["rp"], g["ci"], g["val"], B, out=C)
            assert got.data_ptr() == C.data_ptr()
            _same_bits(C, want, (dt, N, align))
            assert bool((cbuf[:skip] == 123.0).all()) and bool((cbuf[skip + g["M"] * N:] == 123.0).all()), (dt, N, align)


def _special_cases(dt):
    """(B values of the row's entries, edge values or None, expected result or None = whatever narrow(fp32 chain) gives)."""
    inf, nan = float("inf"), float("nan")
    if dt == "bf16":
        big = float(torch.tensor(0x7F7F, dtype=torch.int16).view(torch.bfloat16).float())  # largest finite bf16
        return [
            ([1.0, 2.0 ** -8], None, 1.0),                                  # exact tie -> even (down)
            ([1.0 + 2.0 ** -7, 2.0 ** -8], None, 1.0 + 2.0 ** -6),          # exact tie -> even (up)
            ([1.0, 2.0 ** -8, 2.0 ** -20], None, 1.0 + 2.0 ** -7),          # just above the tie
            ([big, 2.0 ** 119], [1.0, 1.0], inf),                           # fp32 sum is finite, above bf16's largest: overflow at the store
            ([big, big], [2.0, 2.0], inf),                                  # overflow in fp32 already
            ([2.0 ** -130, 2.0 ** -133], None, 9 * 2.0 ** -133),            # subnormal inputs, subnormal result
            ([2.0 ** -130, 2.0 ** -133], [0.5, 0.5], 4 * 2.0 ** -133),      # 4.5 units: tie -> even, rounded not flushed
            ([2.0 ** -126, -(2.0 ** -133)], None, None),                    # normal minus subnormal
        ]
    return [
        ([1.0, 2.0 ** -11], None, 1.0),
        ([1.0 + 2.0 ** -10, 2.0 ** -11], None, 1.0 + 2.0 ** -9),
        ([1.0, 2.0 ** -11, 2.0 ** -20], None, 1.0 + 2.0 ** -10),
        ([65504.0, 65504.0], None, inf),                                    # overflow at the store
        ([65504.0, 15.0], None, 65504.0),                                   # below the tie to infinity
        ([65504.0, 16.0], None, inf),                                       # the tie itself rounds to even = infinity
        ([2.0 ** -24, 2.0 ** -24], None, 2.0 ** -23),                       # subnormal inputs, subnormal result
        ([3 * 2.0 ** -24], [0.5], 2 * 2.0 ** -24),                          # 1.5 units: tie -> even
        ([2.0 ** -14, -(2.0 ** -24)], None, None),
    ]


@pytest.mark.parametrize("dt", ("f16", "bf16"))
@pytest.mark.parametrize("N", (8, 3))  # the kernel route and the composition
def test_rounding_and_special_values(pkg, dt, N):
    from gespmm_amd import _lib, spmm

    dtype = DT[dt]
    inf, nan = float("inf"), float("nan")
    cases = _special_cases(dt) + [
        ([-0.0], None, None), ([], None, 0.0), ([-0.0, -0.0], None, None), ([-0.0], [1.0], None),
        ([inf, 1.0], None, inf), ([-inf, 1.0], None, -inf), ([inf, -inf], None, nan), ([nan, 1.0], None, nan), ([1.0, nan, 2.0], [1.0, 0.0, 1.0], nan),
    ]
    for valued in (False, True):
        rows = [c for c in cases if valued or c[1] is None]
        bvals, rowptr, colind, vals = [], [0], [], []
        for b, v, _ in rows:
            for j, x in enumerate(b):
                colind.append(len(bvals))
                bvals.append(x)
                vals.append(1.0 if v is None else v[j])
            rowptr.append(len(colind))
        K, M = len(bvals), len(rows)
        B32 = torch.tensor(bvals, dtype=torch.float32).unsqueeze(1).repeat(1, N)
        B16 = B32.to(dtype).cuda()
        assert torch.equal(torch.nan_to_num(B16.float().cpu(), nan=7.0), torch.nan_to_num(B32, nan=7.0)), "every input must be exact in the 16-bit type"
        rp, ci = _dev(np.array(rowptr, dtype=np.int32)), _dev(np.array(colind, dtype=np.int32))
        val = _dev(np.array(vals, dtype=np.float32)) if valued else None
        assert _route(_lib, M, K, N, len(colind)) == (1 if N % 2 == 0 else 0)
        got = _call(spmm, rp, ci, val, B16)
        _same_bits(got, _call(spmm, rp, ci, val, B16.float()).to(dtype), (dt, N, valued, "fp32 call"))
        for r, (b, v, want) in enumerate(rows):
            if want is None:
                continue
            w = torch.full((N,), want, dtype=torch.float32).to(dtype).cuda()
            _same_bits(got[r], w, (dt, N, valued, r, b))
        empty = [r for r, c in enumerate(rows) if not c[0]][0]
        assert bool((got[empty].view(torch.int16) == 0).all()), "an empty row is +0"


@pytest.fixture(scope="module")
def amazon():
    from gespmm_amd import graphs

    g = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda", scale=0.25)
    gen = torch.Generator(device="cuda").manual_seed(5)
    g["val"] = torch.rand(g["colind"].numel(), device="cuda", generator=gen) - 0.5
    g["val2"] = torch.rand(g["colind"].numel(), device="cuda", generator=gen) + 0.5
    g["B"] = torch.rand(g["K"], 128, device="cuda", generator=gen) - 0.5
    return g


@pytest.mark.parametrize("kernel", ("stream", "seg-stream", "auto", "staged"))
def test_plans(pkg, amazon, kernel, monkeypatch):
    from gespmm_amd import spmm

    g = amazon
    rp, ci, K = g["rowptr"], g["colind"], g["K"]
    plan = spmm.SpmmPlan(rp, ci, K, 128, values=g["val"], reorder=True, kernel=kernel)
    assert plan.clustered, plan.describe()
    # (at this quarter size "auto" routes to the batch-stream kernel — only the full-size graph gets staged rows from the policy,
    # test_gpu_plan.py — so the table plan is asked for by name)
    if kernel == "staged":  # the fp32 route at the plan's width is the staged-rows kernel: the composition below wraps THAT kernel
        assert "kernel=staged-rows" in plan.describe(), plan.describe()
    routes = set()
    for N in (128, 64, 32, 33):  # the plan's width, two others, and one only the composition serves
        for dt, dtype in DT.items():  # both element types on the same plan, one after the other
            B16 = g["B"][:, :N].contiguous().to(dtype)
            route = plan.x16_route(N)
            routes.add(route)
            assert route == 0 if N % 2 else route in (0, 1, 2), (N, route)
            if kernel in ("stream", "seg-stream") and N % 2 == 0:
                assert route == (2 if kernel == "seg-stream" else 1), (kernel, N, plan.describe())
            got = spmm.csr_spmm(rp, ci, g["val"], B16, plan=plan)
            assert got.dtype == dtype
            assert "x16 %s N=%d route=%d " % (dt, N, route) in plan.describe(), plan.describe()
            _same_bits(got, spmm.csr_spmm(rp, ci, g["val"], B16.float()).to(dtype), (kernel, N, dt))
    # both executions at the plan's own width, pinned (GESPMM_X16_ROUTE is read per call): the 16-bit kernel on the task tables, and
    # widen -> the plan's fp32 route (staged rows for kernel="staged") -> narrow on the plan's temporaries
    B16 = g["B"].to(torch.bfloat16)
    want = spmm.csr_spmm(rp, ci, g["val"], B16.float()).to(torch.bfloat16)
    for pin in ("kernel", "composition"):
        monkeypatch.setenv("GESPMM_X16_ROUTE", pin)
        route = plan.x16_route(128)
        assert (route == 0) == (pin == "composition"), (pin, route)
        got = spmm.csr_spmm(rp, ci, g["val"], B16, plan=plan)
        assert "x16 bf16 N=128 route=%d " % route in plan.describe(), plan.describe()
        _same_bits(got, want, (kernel, "pinned", pin))
    monkeypatch.delenv("GESPMM_X16_ROUTE")
    # new values reach the 16-bit launch through the plan's own bookkeeping (_sync_inputs -> gespmm_plan_set_values)
    got = spmm.csr_spmm(rp, ci, g["val2"], B16, plan=plan)
    _same_bits(got, spmm.csr_spmm(rp, ci, g["val2"], B16.float()).to(torch.bfloat16), (kernel, "new values"))
    # unweighted through the same plan
    got = spmm.csr_spmm_no_edge_value(rp, ci, B16, plan=plan)
    _same_bits(got, spmm.csr_spmm_no_edge_value(rp, ci, B16.float()).to(torch.bfloat16), (kernel, "unweighted"))


def _launch_table():
    """The instantiations of spmm_x16.h as {(V, S, W, segmented, plan_only)}, read from the launch table itself."""
    import os
    import re

    from helpers import ROOT

    text = open(os.path.join(ROOT, "gespmm_amd", "csrc", "spmm_x16.h")).read()
    body = text[text.index("static hipError_t launch_x16_geometry"):text.index("#undef GESPMM_X16_STREAM")]
    common, planned = body.split("if constexpr (PLANNED)")
    table = set()
    for part, plan_only in ((common, False), (planned, True)):
        for kind, v, s_, w in re.findall(r"^\s*GESPMM_X16_(STREAM|SEG)\((\d), (\d), (\d+)\)", part, flags=re.M):
            table.add((int(v), int(s_), int(w), kind == "SEG", plan_only))
    return table


def _short_row_graph(M=2000, K=500, seed=3):
    """Mean degree ~4 with empty rows over a B that fits the L2s: the shape select.cpp gives the segmented-stream kernel at W >= 32."""
    rng = np.random.RandomState(seed)
    degs = rng.randint(0, 9, size=M)
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    return {"M": M, "K": K, "nnz": int(rowptr[-1]), "rowptr": rowptr, "colind": rng.randint(0, K, size=int(rowptr[-1])).astype(np.int32)}


def _carve(t, align):
    """A copy of 2-D `t` whose address `align` (16, 8, 4) divides and 2 * align (for 8, 4) does not."""
    skip = {16: 0, 8: 4, 4: 2}[align]
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[skip:skip + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def test_every_instantiation_of_the_launch_table_runs(pkg, edge):
    """Every kernel spmm_x16.h builds is launched at least once and gives the contract's bits: (V, S, W, segmented) of each launch comes
    from gespmm_describe_launch at the byte-equivalent width (storage order) or from plan.describe() (task tables), and the set
    reached must BE the launch table. Explicit variants stand in for shapes only huge matrices select on their own (two strips of four
    words: M >= 2^17); alignment selects the narrower vectors."""
    import ctypes

    from gespmm_amd import _lib, spmm

    table = _launch_table()
    assert len(table) == 23 and sum(not t[4] for t in table) == 17, sorted(table)
    dtype = torch.bfloat16
    buf = ctypes.create_string_buffer(300)
    dense, short = edge, _short_row_graph()
    short["rp"], short["ci"] = _dev(short["rowptr"]), _dev(short["colind"])
    short["val"] = torch.rand(short["nnz"], device="cuda") - 0.5
    Bcache = {}

    def operand(g, N):
        key = (g["K"], N)
        if key not in Bcache:
            Bcache[key] = (torch.rand(g["K"], N, device="cuda") - 0.5).to(dtype)
        return Bcache[key]

    def stateless_geometry(g, N, variant, align):
        cfg = _lib.LaunchCfg()
        _lib.lib.gespmm_describe_launch(g["M"], g["K"], N // 2, g["nnz"], variant, None, buf, 300)
        d = dict(kv.split("=") for kv in buf.value.decode().split() if "=" in kv)
        if int(d["V"]) > align // 4:  # what the operands' alignment leaves of the vector
            cfg.vec = align // 4
            _lib.lib.gespmm_describe_launch(g["M"], g["K"], N // 2, g["nnz"], variant, ctypes.byref(cfg), buf, 300)
            d = dict(kv.split("=") for kv in buf.value.decode().split() if "=" in kv)
        assert d["kernel"] in ("batch-stream", "segmented-stream"), buf.value
        return int(d["V"]), int(d["S"]), int(d["W"]), d["kernel"] == "segmented-stream"

    # ---- storage order: (graph, N, variant, alignment)
    reached = set()
    cases = [(dense, N, -1, 16) for N in (8, 16, 32, 64, 128, 136, 264)]                # batch V=1 W=4..64, V=4 W=32, 64
    cases += [(dense, 528, 4, 16), (dense, 256, -1, 8), (dense, 264, -1, 8), (dense, 264, -1, 4)]  # (4,2,64) (2,1,64) (2,2,64) (1,2,64)
    cases += [(short, N, -1, 16) for N in (64, 128, 256, 520)]                          # segmented V=1 W=32, 64, V=4 W=32, 64
    cases += [(short, 528, 4, 16), (short, 256, -1, 8)]                                 # segmented (4,2,64) (2,1,64)
    for g, N, variant, align in cases:
        B, val = _carve(operand(g, N), align), g["val"]
        assert _route(_lib, g["M"], g["K"], N, g["nnz"], align, align, variant) in (1, 2), (N, variant, align)
        geo = stateless_geometry(g, N, variant, align)
        assert (_route(_lib, g["M"], g["K"], N, g["nnz"], align, align, variant) == 2) == geo[3]
        out = _carve(torch.zeros(g["M"], N, dtype=dtype, device="cuda"), align)
        spmm.csr_spmm(g["rp"], g["ci"], val, B, variant=variant, out=out)
        _same_bits(out, spmm.csr_spmm(g["rp"], g["ci"], val, B.float()).to(dtype), ("storage", N, variant, align, geo))
        reached.add(geo + (False,))
    assert reached == {t for t in table if not t[4]}, (sorted(reached), sorted(t for t in table if not t[4]))

    # ---- a clustered plan's task tables: (kernel, variant, N, alignment); the geometry is what plan.describe() says RAN
    import re

    g = short
    planned = set()
    plans = {}
    cases = [("stream", 1, N, 16) for N in (8, 16, 32, 64, 128)]                         # V=1 W=4..64
    cases += [("stream", 3, N, 16) for N in (32, 64, 128, 256, 512)]                     # V=4 W=4, 8, 16 (plans only), 32, 64
    cases += [("stream", 4, 528, 16), ("stream", -1, 256, 8), ("stream", -1, 264, 8), ("stream", -1, 264, 4)]
    cases += [("seg-stream", 1, N, 16) for N in (8, 16, 32, 64, 128)]                    # V=1 W=4, 8, 16 (plans only), 32, 64
    cases += [("seg-stream", 3, 256, 16), ("seg-stream", 3, 512, 16), ("seg-stream", 4, 528, 16), ("seg-stream", -1, 256, 8)]
    for kernel, variant, N, align in cases:
        if (kernel, variant) not in plans:
            plans[(kernel, variant)] = spmm.SpmmPlan(g["rp"], g["ci"], g["K"], 128, variant=variant, values=g["val"], reorder=True, kernel=kernel)
            assert plans[(kernel, variant)].clustered
        plan = plans[(kernel, variant)]
        B = _carve(operand(g, N), align)
        out = _carve(torch.zeros(g["M"], N, dtype=dtype, device="cuda"), align)
        assert plan.x16_route(N, align, align) == (2 if kernel == "seg-stream" else 1), (kernel, variant, N, align, plan.describe())
        plan.run(g["val"], B, out)
        m = re.search(r"x16 bf16 N=%d route=(\d) \(16-bit (batch|segmented)-stream V=(\d) S=(\d) W=(\d+)\)" % N, plan.describe())
        assert m, plan.describe()
        assert (m.group(2) == "segmented") == (kernel == "seg-stream") == (m.group(1) == "2")
        _same_bits(out, spmm.csr_spmm(g["rp"], g["ci"], g["val"], B.float()).to(dtype), ("plan", kernel, variant, N, align))
        planned.add((int(m.group(3)), int(m.group(4)), int(m.group(5)), kernel == "seg-stream"))
    assert planned == {t[:4] for t in table}, (sorted(planned), sorted({t[:4] for t in table}))


def test_storage_order_plan_and_python_errors(pkg, oracle, bundled):
    from gespmm_amd import spmm

    g = bundled["pubmed"]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    val = _dev(oracle.hash_val(g["nnz"], seed=7))
    B16 = _dev(oracle.hash_B(g["K"], 128, seed=1)).to(torch.float16)
    plan = spmm.SpmmPlan(rp, ci, g["K"], 128, values=val, reorder=False)
    assert plan.x16_route(128) in (1, 2) and plan.x16_route(41) == 0
    _same_bits(spmm.csr_spmm(rp, ci, val, B16, plan=plan), spmm.csr_spmm(rp, ci, val, B16.float()).to(torch.float16), "storage order")
    with pytest.raises(ValueError):
        spmm.csr_spmm(rp, ci, val, B16, cfg={"vec": 1})
    with pytest.raises(TypeError):
        spmm.csr_spmm(rp, ci, val, B16, out=torch.empty(g["M"], 128, device="cuda"))
    with pytest.raises(TypeError):
        spmm.csr_spmm(rp, ci, val.half(), B16)
    for bad in (lambda: spmm.csr_spmm_fused(rp, ci, val, B16, bias=torch.zeros(128, device="cuda")), lambda: spmm.csr_spmm_max(rp, ci, B16),
                lambda: plan.tune(B16), lambda: plan.run(None, B16, reduce_max=-1.0), lambda: spmm.csr_spmm(rp, ci, val, B16.double())):
        with pytest.raises(TypeError):
            bad()


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_long_row_pass_reassociates_identically(pkg, oracle, dt):
    from test_gpu_spmm import _skewed_csr

    from gespmm_amd import _lib, spmm

    G, long_rows = _skewed_csr()
    dtype, N = DT[dt], 128
    rp, ci = _dev(G["rowptr"]), _dev(G["colind"])
    val_h = oracle.hash_val(G["nnz"], seed=11)
    val = _dev(val_h)
    B16 = _dev(oracle.hash_B(G["K"], N, seed=N)).to(dtype)
    plan = spmm.SpmmPlan(rp, ci, G["K"], N, values=val, flags=_lib.FLAG_SPLIT_LONG_ROWS)
    assert plan.x16_route(N) == 0, plan.describe()
    got = spmm.csr_spmm(rp, ci, val, B16, plan=plan)
    _same_bits(got, spmm.csr_spmm(rp, ci, val, B16.float(), plan=plan).to(dtype), "the fp32 route of the same plan")
    # c4's rule plus the rounding of the store: 1e-4 sum |a b| + half a unit in the last place of the 16-bit type at the result
    Bh = B16.float().cpu().numpy().astype(np.float64)
    ref = np.zeros((G["M"], N))
    scale = np.zeros((G["M"], N))
    for r in long_rows:
        lo, hi = G["rowptr"][r], G["rowptr"][r + 1]
        a = val_h[lo:hi].astype(np.float64)[:, None]
        rows = Bh[G["colind"][lo:hi]]
        ref[r] = (a * rows).sum(0)
        scale[r] = np.abs(a * rows).sum(0)
    p = 8 if dt == "bf16" else 11  # significand bits
    g64 = got.float().cpu().numpy().astype(np.float64)[long_rows]
    mag = np.maximum(np.abs(ref[long_rows]), np.abs(g64))
    half_ulp = 2.0 ** (np.floor(np.log2(np.maximum(mag, 2.0 ** -126))) - p)
    err = np.abs(g64 - ref[long_rows])
    assert np.all(err <= 1e-4 * scale[long_rows] + half_ulp), float((err - 1e-4 * scale[long_rows] - half_ulp).max())


def _warm_on_side_stream(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_capture(pkg, oracle, bundled):
    from gespmm_amd import _lib, spmm

    g = bundled["pubmed"]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    val = _dev(oracle.hash_val(g["nnz"], seed=7))
    plan = spmm.SpmmPlan(rp, ci, g["K"], 41, values=val, reorder=True, kernel="stream")
    assert plan.x16_route(41) == 0
    # the kernel route without a plan, and a plan's composition whose temporaries the warm-up made: both capture and replay
    for N, p in ((128, None), (41, plan)):
        B = torch.zeros(g["K"], N, dtype=torch.bfloat16, device="cuda")
        C = torch.zeros(g["M"], N, dtype=torch.bfloat16, device="cuda")
        assert p is not None or _route(_lib, g["M"], g["K"], N, g["nnz"]) in (1, 2)
        fn = lambda: spmm.csr_spmm(rp, ci, val, B, out=C, plan=p)  # noqa: E731
        _warm_on_side_stream(fn)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        for seed in (2, 3):
            B.copy_(_dev(oracle.hash_B(g["K"], N, seed=seed)).to(torch.bfloat16))  # new contents, same address
            C.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            _same_bits(C, spmm.csr_spmm(rp, ci, val, B.float()).to(torch.bfloat16), (N, seed))
    # the stateless composition would have to allocate: refused under capture, nothing launched
    B = _dev(oracle.hash_B(g["K"], 41, seed=1)).to(torch.bfloat16)
    C = torch.full((g["M"], 41), 5.0, dtype=torch.bfloat16, device="cuda")
    tick = torch.zeros(8, device="cuda")
    _warm_on_side_stream(lambda: spmm.csr_spmm(rp, ci, val, B))
    caught = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tick.add_(1.0)
        try:
            spmm.csr_spmm(rp, ci, val, B, out=C)
        except _lib.GespmmError as e:
            caught.append(e)
    assert len(caught) == 1 and caught[0].code == 900, caught  # hipErrorStreamCaptureUnsupported
    graph.replay()
    torch.cuda.synchronize()
    assert bool((C == 5.0).all())


def test_autograd_and_gcnconv(pkg, oracle, bundled):
    import gespmm_amd
    from gespmm_amd import graphs, spmm

    g = bundled["pubmed"]
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    colptr, rowind = graphs.transpose_csr(rp, ci)
    w_csr = _dev(oracle.hash_val(g["nnz"], seed=7))
    w_csc = spmm.csr2csc(rp, ci, torch.empty_like(colptr), torch.empty_like(rowind), w_csr)
    bf = torch.bfloat16
    x0 = _dev(oracle.hash_B(g["K"], 16, seed=4)).to(bf)
    go = _dev(oracle.hash_B(g["M"], 16, seed=5)).to(bf)
    for w1, w2 in ((None, None), (w_csr, w_csc)):
        x = x0.clone().requires_grad_(True)
        y = gespmm_amd.SPMMFunction.apply(rp, ci, colptr, rowind, x, w1, w2)
        y.backward(go)
        assert y.dtype == bf and x.grad.dtype == bf
        _same_bits(y.detach(), _call(spmm, rp, ci, w1, x0.float()).to(bf), "forward")
        _same_bits(x.grad, _call(spmm, colptr, rowind, w2, go.float()).to(bf), "backward")
    with pytest.raises(TypeError):
        gespmm_amd.SPMMFunction.apply(rp, ci, colptr, rowind, x0.clone().requires_grad_(True), w_csr, w_csc, True)
    torch.manual_seed(0)
    conv = gespmm_amd.GCNConv(16, 8).cuda().to(bf)
    with torch.no_grad():
        conv.bias.copy_(torch.linspace(-1, 1, 8))
    x = x0.clone().requires_grad_(True)
    y = conv(x, rp, ci, colptr, rowind)
    assert y.dtype == bf
    with torch.no_grad():
        s_in = (1 / torch.sqrt(torch.diff(rp).float())).unsqueeze(1).to(bf)
        s_out = (1 / torch.sqrt(torch.diff(colptr).float())).unsqueeze(1).to(bf)
        h = (x0 @ conv.weight) * s_out
        want = spmm.csr_spmm_no_edge_value(rp, ci, h.float()).to(bf) * s_in + conv.bias
    _same_bits(y.detach(), want, "GCNConv forward")
    y.float().square().sum().backward()
    assert x.grad is not None and x.grad.dtype == bf and conv.weight.grad.dtype == bf
    fused = gespmm_amd.GCNConv(16, 8, fused=True).cuda().to(bf)
    with pytest.raises(TypeError):
        fused(x0, rp, ci, colptr, rowind)


FUZZ_SEED, FUZZ_CASES, FUZZ_MIN_KERNEL = 2025, 200, 120  # (seed 2025: 141 of the 200 cases take a kernel route)


def _fuzz_cases():
    rng = np.random.RandomState(FUZZ_SEED)
    for i in range(FUZZ_CASES):
        M, K = int(rng.randint(1, 301)), int(rng.randint(1, 301))
        N = int(rng.randint(1, 301))
        if rng.rand() < 0.8:
            N += N % 2  # most users' widths are even
        mix = rng.choice([0, 0, 1, 2, 5, 17, 64, 130], size=M)
        degs = np.minimum(rng.poisson(mix), 4 * K)
        rowptr = np.zeros(M + 1, dtype=np.int32)
        rowptr[1:] = np.cumsum(degs)
        colind = rng.randint(0, K, size=int(rowptr[-1])).astype(np.int32)
        skip_b, skip_c = (int(rng.choice([0, 0, 0, 8, 4, 2, 1])) for _ in range(2))
        yield dict(i=i, M=M, K=K, N=N, rowptr=rowptr, colind=colind, nnz=int(rowptr[-1]), dt=("f16", "bf16")[int(rng.randint(2))],
                   valued=bool(rng.randint(2)), skip_b=skip_b, skip_c=skip_c, seed=int(rng.randint(1 << 30)))


def _align_of(skip):
    return {0: 16, 8: 16, 4: 8, 2: 4, 1: 2}[skip]


def test_fuzz(pkg):
    from gespmm_amd import _lib, spmm

    kernel_routes = 0
    for c in _fuzz_cases():
        dtype = DT[c["dt"]]
        M, K, N = c["M"], c["K"], c["N"]
        route = _route(_lib, M, K, N, c["nnz"], _align_of(c["skip_b"]), _align_of(c["skip_c"]))
        kernel_routes += route != 0
        gen = torch.Generator(device="cuda").manual_seed(c["seed"])
        rp, ci = _dev(c["rowptr"]), _dev(c["colind"])
        val = (torch.rand(c["nnz"], device="cuda", generator=gen) - 0.5) if c["valued"] else None
        bbuf = torch.zeros(K * N + 16, dtype=dtype, device="cuda")
        cbuf = torch.full((M * N + 16,), 3.0, dtype=dtype, device="cuda")
        B = bbuf[c["skip_b"]:c["skip_b"] + K * N].view(K, N)
        C = cbuf[c["skip_c"]:c["skip_c"] + M * N].view(M, N)
        B.copy_((torch.rand(K, N, device="cuda", generator=gen) - 0.5) * 8)
        _call(spmm, rp, ci, val, B, out=C)
        _same_bits(C, _call(spmm, rp, ci, val, B.float()).to(dtype), {k: c[k] for k in ("i", "M", "K", "N", "dt", "valued", "skip_b", "skip_c")})
        assert bool((cbuf[:c["skip_c"]] == 3.0).all()) and bool((cbuf[c["skip_c"] + M * N:] == 3.0).all()), c["i"]
    assert kernel_routes >= FUZZ_MIN_KERNEL, kernel_routes
