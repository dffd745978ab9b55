"""The sum / max products and their plans at the 32-bit offset switches: 2 GB (bit 31 of a byte offset), 4 GB (the offset's width) and
8 GB (the two-halves form of the tuned staged kernel) — DESIGN.md §4.3.

Every kernel of the table below forms a 32-bit byte offset that is added to a scalar base. Each case runs ONE kernel at the largest
size it is offered (``below``) or one row more (``at``: the plan must name another kernel and still be right), on the patterns of
tests/large_products.py: ``both`` (B and C at the size), ``tall`` (only C: B has 4099 rows) and ``wide`` (only B: C has 4096 rows).

  kernel (file)                                  widths here          offered while
  tuned staged      spmm_staged.hip              128, 256, 512, 1024  max(M, K) N 4 < 0xFFFF0000; 512 / 1024: < 0x1FFFF0000 (two halves)
  lane-group staged spmm_staged_narrow.hip       64                   < 0xFFFF0000
  general staged    spmm_staged_gen.hip          602, 100 (sum, max)  < 0xFFFF0000
  padded records    spmm_records.hip             64, 48               max(M, K) N 4 < 2^32
  streaming         spmm_stream.h                512, 300             idx32 while K N 4 < 2^32, idx64 from there
  fused streaming   spmm_fused.hip               512                  route 1 / 2 while idx32, the composition (route 0) from there
  16-bit streaming  spmm_x16.hip                 512, 1024            route 1 / 2 while K N 2 < 2^32, the composition from there
  long-row pass     spmm_kernels.hip             512                  a hub row of 4096 entries; offsets as the streaming launch's
  plan SDDMM        sddmm_edge.h, plan.cpp       512                  routes 0 / 1 / 2 on both sides (size_t arithmetic: no switch)

B is large_operands.b_at — a function of the WORD position, so no displacement by 2^29, 2^30 or 2^31 words is invisible — the weights
are large_operands.w_nz (no zeros). Every result goes into a NaN-prefilled tensor; afterwards no word of the WHOLE result is NaN (a
wrongly addressed C row leaves its own row unwritten), the windows of large_products.Pattern.windows (4096 rows around the rows holding
byte 2^31, byte 2^32 and the last byte, the first and the last window) EQUAL the int64 closed form, and the whole result has the bits
of an independent path: the plain call with 64-bit offsets, the four separate passes of the fused product, widen / fp32 / narrow of
the 16-bit one. tests/test_large_products_host.py shows without a device that each of these comparisons rejects a B offset or a C
row displaced by 2^31 or 2^32 bytes, that the windows hold the marked rows, and that ``below`` / ``at`` lie on the two sides of every
switch. Every case asserts from plan.describe(), plan.fused_route(), plan.x16_route() or the launch description that the kernel it
is named after ran. No tolerance: every sum is an exact small integer.

On the MI355X the module takes 77 s for 104 cases and peaks at 24.4 GiB of device memory; plan creation takes 0.01 - 0.09 s at 4 - 22 M
rows and a product milliseconds, so a case takes 0.02 - 0.9 s unless an allocation of its operands waits: measured alone, allocating
three 8 GB tensors takes 0.001 s in fourteen of sixteen rounds and 3.7 / 5.2 s in the other two (which cases wait changes from run to
run; DESIGN.md has the table)."""
import ctypes

import pytest
import torch

import band
import large_operands as lo
import large_products as lp
import test_gpu_large_operands as glo
from large_products import (GENERAL, K300, K512, NARROW, R64, R100, R128, R256, R512, R512P, R1024, R1024P, REC48, REC64, RECORD, TUNED, X512,
                            X1024)
from test_gpu_large_edges import DEV, _check_windows, _nan, _poison

pytestmark = pytest.mark.gpu

D = lp.D
STAGED, RECORDS = "kernel=staged-rows", "kernel=padded-records"


def test_the_row_counts_are_those_of_the_issue():
    assert (R128, R256, R512, R512P, R1024, R1024P) == (8_388_479, 4_194_239, 2_097_119, 4_194_271, 1_048_559, 2_097_135)
    assert (R64, R100, REC64, REC48) == (16_776_959, 10_737_254, 16_777_215, 22_369_621)
    assert (K512, K300, X512, X1024) == (2_097_151, 3_579_139, 4_194_303, 2_097_151)


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _launch(M, K, N, nnz, variant=-1, flags=0):
    """What the plain call launches (gespmm_describe_launch: host only)."""
    from gespmm_amd import _lib

    buf = ctypes.create_string_buffer(256)
    cfg = _lib.LaunchCfg(0, 0, 0, 0, 0, flags)
    assert _lib.lib.gespmm_describe_launch(M, K, N, nnz, variant, ctypes.byref(cfg), buf, 256) > 0
    return buf.value.decode()


def _inputs(kind, R, N, elem=4, arrays=3):
    """Pattern, CSR arrays and weights; skips only where the device has less free memory than the case holds: B and ``arrays`` - 1
    results (or copies) of the larger of the two shapes, the edge arrays and the plan's copies of them."""
    p = lp.Pattern(kind, R, D).set_marks(N, elem)
    need = (p.K + (arrays - 1) * max(p.M, p.K)) * N * 4 + 10 * 12 * p.nnz + (4 << 30)
    glo._need(-(-need // (1 << 30)))
    rp, ci = p.csr(DEV)
    assert int(ci.min()) >= 0 and int(ci.max()) == p.K - 1  # the last row of B is gathered
    return p, rp, ci, p.values(DEV)


def _dense(p, N, dtype=torch.float32):
    """[K, N] of large_operands.b_at(1, N), in row chunks (integer temporaries of at most 256 MB)."""
    return glo._nodes(p.K, 1, N, dtype).view(p.K, N)


def _same_bits(what, a, b):
    """The WHOLE of two results, bit for bit, 2^28 words at a time."""
    view = {4: torch.int32, 2: torch.int16}[a.element_size()]
    fa, fb = a.view(view).reshape(-1), b.view(view).reshape(-1)
    assert fa.numel() == fb.numel()
    for s in range(0, fa.numel(), 1 << 28):
        assert torch.equal(fa[s:s + (1 << 28)], fb[s:s + (1 << 28)]), "%s: words %d .. differ from the independent path" % (what, s)


def _check_sum(what, p, N, out, weighted=True):
    glo._written(out=out)
    _check_windows(what, out, p.windows(N), lambda r0, r1: p.ref_sum(r0, r1, N, DEV, weighted=weighted))


def _both_sides(p, N, elem=4):
    """Host-side facts of the case: which operands are past byte 2^31 / 2^32, and that the pattern reaches both sides."""
    rb = N * elem
    far = p.far(torch.arange(p.M, device=DEV, dtype=torch.int64))
    for byte in lo.BYTES:
        row = byte // rb
        if row < p.K - 1:  # B reaches past this byte: far columns, and band columns, on both sides of it and in the row holding it
            assert bool((far < row).any()) and bool((far > row).any()), (byte, "far columns on one side only")
            if p.kind != "tall":
                lo_band, hi_band = int(p.col(0, 0)), int(p.col(p.M - 1, D - 1))
                assert lo_band < row < hi_band, (byte, "band columns on one side only")
    assert bool((far == p.K - 1).any()), "no far column in the last row of B"
    assert int(p.far(p.M - 2)) == p.K - 1 or p.kind == "wide"


# ---- the table kernels through their plans -------------------------------------------------------------------------------------------

def _staged_fraction(desc):
    return float(desc.split("staged_entries=")[1].split()[0])


def _crossings_inside_a_block(perm, row, rows):
    """Adjacent positions i, i + 1 of the plan's row order that belong to ONE block of ``rows`` positions and hold C rows on the two
    sides of ``row``."""
    up = perm >= row
    at = torch.nonzero(up[1:] != up[:-1]).flatten() + 1
    return int((at % rows != 0).sum())


def _plan_case(kernel, tag, N, R, kind, reorder, served=True, idx=None, reducers=("sum",)):
    from gespmm_amd import _lib, spmm

    p, rp, ci, val = _inputs(kind, R, N)
    _both_sides(p, N)
    what = "%s N=%d R=%d %s reorder=%s" % (kernel, N, R, kind, reorder)
    B = _dense(p, N)
    plan = spmm.SpmmPlan(rp, ci, p.K, N, values=val, reorder=reorder, kernel=kernel)
    desc = plan.describe()
    assert (tag in desc) == served, (what, desc)
    assert idx in desc and {"idx32": "idx64", "idx64": "idx32"}[idx] not in desc, (what, desc)  # the streaming launch behind the plan
    if served and tag == STAGED:
        # both staged (LDS) and memory-gathered entries; the tall pattern, whose 4099 columns every block shares, may stage them all
        f = _staged_fraction(desc)
        assert 0.0 < f < 1.0 or (kind == "tall" and f == 1.0), (what, desc)
    paged = tag == STAGED and served and max(p.M, p.K) * N * 4 >= lp.TABLE_BOUND
    if paged and kind == "tall" and reorder is True:
        # the tall pattern puts C rows on both sides of row 2^32 / row bytes inside ONE block (rows r and r + 4099 share their band)
        blocks = int(desc.split("blocks=")[1].split()[0])
        rows = -(-p.M // blocks)
        assert -(-p.M // rows) == blocks, (what, desc)  # blocks of ``rows`` consecutive positions of the row order
        inside = _crossings_inside_a_block(plan.order(), (1 << 32) // (N * 4), rows)
        assert inside > 0, (what, inside, desc)
    if "sum" in reducers:
        out = spmm.csr_spmm(rp, ci, val, B, plan=plan, out=_nan((p.M, N)))
        _check_sum(what, p, N, out)
        launch = _launch(p.M, p.K, N, p.nnz, flags=_lib.FLAG_FORCE_IDX64)
        assert "idx64" in launch, launch
        plain = spmm.csr_spmm(rp, ci, val, B, cfg={"flags": _lib.FLAG_FORCE_IDX64}, out=_nan((p.M, N)))
        glo._written(plain=plain)
        _same_bits(what, out, plain)
        del plain
        out.fill_(float("nan"))
        spmm.csr_spmm_no_edge_value(rp, ci, B, plan=plan, out=out)  # the same plan without values
        _check_sum(what + " unweighted", p, N, out, weighted=False)
        del out
    del plan
    if "max" in reducers:
        plan = spmm.SpmmPlan(rp, ci, p.K, N, reorder=reorder, kernel=kernel)  # (the max reducer takes plans without values)
        assert (tag in plan.describe()) == served, (what, plan.describe())
        out = _nan((p.M, N))
        # (no entry point answers which kernel a max launch took. What plan_route asks of it beyond the tables that describe() names:
        #  the plan's own width, 16-byte operands — asserted here — and tables of this width's block shape, which they have by construction)
        assert B.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and B.shape[1] == N
        plan.run(None, B, out=out, reduce_max=lp.EMPTY)
        glo._written(out=out)
        _check_windows(what + " max", out, p.windows(N), lambda r0, r1: p.ref_max(r0, r1, N, DEV))
        assert float(out.min()) >= -3.0 and float(out.max()) <= 3.0, "the empty value among the maxima"
        plain = spmm.csr_spmm_max(rp, ci, B, lp.EMPTY)
        _same_bits(what + " max", out, plain)


def _ids(cases):
    return ["%d-%d-%s-%s" % (c[0], c[1], c[2], "clustered" if c[3] else "storage") for c in cases]


@pytest.mark.parametrize("N,R,kind,reorder,served,idx", TUNED, ids=_ids(TUNED))
def test_tuned_staged_kernel(pkg, N, R, kind, reorder, served, idx):
    assert pkg._lib.plan_policy(R, R, 5 * R, N, 5, kernel=pkg._lib.PLAN_KERNEL_STAGED, reorder=pkg._lib.PLAN_REORDER)["build_staged"] == int(served)
    _plan_case("staged", STAGED, N, R, kind, reorder, served, idx)


@pytest.mark.parametrize("N,R,kind,reorder,served,idx", NARROW, ids=_ids(NARROW))
def test_lane_group_staged_kernel(pkg, N, R, kind, reorder, served, idx):
    _plan_case("staged", STAGED, N, R, kind, reorder, served, idx)


@pytest.mark.parametrize("reducer", ("sum", "max"))
@pytest.mark.parametrize("N,R,kind,reorder,served,idx", GENERAL, ids=_ids(GENERAL))
def test_general_staged_kernel(pkg, N, R, kind, reorder, served, idx, reducer):
    """N = 602: rows of 2408 bytes, bytes 2^31 and 2^32 fall inside a row. The max reducer's reference is the exact maximum; the
    empty value (-10000) must not occur."""
    _plan_case("staged", STAGED, N, R, kind, reorder, served, idx, reducers=(reducer,))


@pytest.mark.parametrize("N,R,kind,reorder,served,idx", RECORD, ids=_ids(RECORD))
def test_padded_record_kernel(pkg, N, R, kind, reorder, served, idx):
    assert D + 1 <= 1024  # kRecordMaxRow
    _plan_case("records", RECORDS, N, R, kind, reorder, served, idx)


# ---- the streaming kernels, plain and planned -----------------------------------------------------------------------------------------

VARIANTS = (-1, 1, 2, 4)


@pytest.mark.parametrize("side", ("below", "at"))
@pytest.mark.parametrize("N,K", ((512, K512), (300, K300)), ids=("512", "300"))
def test_streaming_kernels_plain(pkg, N, K, side):
    """idx32 with every offset past the middle of B at bit 31 set, and idx64 one row later; every variant, and the launch flags that
    pick another streaming kernel."""
    from gespmm_amd import _lib, spmm

    K = K + (side == "at")
    word = "idx32" if side == "below" else "idx64"
    p, rp, ci, val = _inputs("both", K, N)
    _both_sides(p, N)
    assert (p.K * N * 4 < (1 << 32)) == (side == "below")
    B = _dense(p, N)
    want = spmm.csr_spmm(rp, ci, val, B, cfg={"flags": _lib.FLAG_FORCE_IDX64}, out=_nan((p.M, N)))
    _check_sum("plain idx64 N=%d K=%d" % (N, K), p, N, want)
    out = _nan((p.M, N))
    seg = _lib.FLAG_SEG_STREAM | _lib.FLAG_STRICT_ORDER  # (the segmented kernel has no long-row pass: taken in strict order only)
    launches = [(v, 0, "batch-stream") for v in VARIANTS] + [(v, seg, "segmented-stream") for v in VARIANTS] + \
        [(-1, _lib.FLAG_BATCH_STREAM, "batch-stream"), (-1, _lib.FLAG_SLAB_BLOCKED, "slab-blocked"), (-1, _lib.FLAG_SPLIT_LONG_ROWS, "batch-stream")]
    for variant, flags, name in launches:
        desc = _launch(p.M, p.K, N, p.nnz, variant, flags)
        assert desc.split(" long_rows")[0].endswith(word) and ("kernel=" + name) in desc, desc
        what = "plain N=%d K=%d variant=%d flags=%#x" % (N, K, variant, flags)
        out.fill_(float("nan"))
        spmm.csr_spmm(rp, ci, val, B, variant=variant, cfg={"flags": flags}, out=out)
        glo._written(out=out)
        _same_bits(what, out, want)
    out.fill_(float("nan"))
    spmm.csr_spmm_no_edge_value(rp, ci, B, cfg={"flags": 0}, out=out)
    _check_sum("plain unweighted N=%d K=%d" % (N, K), p, N, out, weighted=False)


@pytest.mark.parametrize("side", ("below", "at"))
@pytest.mark.parametrize("kernel,reorder", (("stream", True), ("seg-stream", True), ("stream", False)),
                         ids=("stream", "seg-stream", "stream-storage"))
def test_streaming_kernels_planned(pkg, kernel, reorder, side):
    from gespmm_amd import _lib, spmm

    N, K = 512, K512 + (side == "at")
    word = "idx32" if side == "below" else "idx64"
    name = "kernel=segmented-stream" if kernel == "seg-stream" else "kernel=batch-stream"
    p, rp, ci, val = _inputs("both", K, N)
    B = _dense(p, N)
    want = spmm.csr_spmm(rp, ci, val, B, cfg={"flags": _lib.FLAG_FORCE_IDX64}, out=_nan((p.M, N)))
    _check_sum("plain idx64 N=%d K=%d" % (N, K), p, N, want)
    out = _nan((p.M, N))
    for variant in VARIANTS:
        plan = spmm.SpmmPlan(rp, ci, p.K, N, variant=variant, values=val, reorder=reorder, kernel=kernel)
        desc = plan.describe()
        assert name in desc and desc.split(" long_rows")[0].endswith(word) and plan.clustered == reorder, desc
        what = "plan %s N=%d K=%d variant=%d" % (kernel, N, K, variant)
        out.fill_(float("nan"))
        spmm.csr_spmm(rp, ci, val, B, variant=variant, plan=plan, out=out)
        glo._written(out=out)
        _same_bits(what, out, want)
        if variant == -1:
            out.fill_(float("nan"))
            spmm.csr_spmm_no_edge_value(rp, ci, B, plan=plan, out=out)
            _check_sum(what + " unweighted", p, N, out, weighted=False)
        del plan


# ---- the long-row pass: one hub row of 4096 entries ------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", ("below", "at"))
def test_long_row_pass_on_a_hub_row(pkg, side):
    """large_products.HubPattern: ``both`` plus one row of 4096 entries whose columns stride over all of B and end in the rows holding byte
    2^31, byte 2^32 and the last. The plain call's long-row pass (on by itself at this size, and by FLAG_SPLIT_LONG_ROWS), the stream
    plan's and the hub pass of a staged plan each take that row: chunked partial sums, then one sum per element into the (permuted) C
    row. Exact integers, so the re-association changes no bit: closed form, no NaN, and the bits of the strict-order idx64 call."""
    from gespmm_amd import _lib, spmm

    N, K = 512, K512 + (side == "at")
    word = "idx32" if side == "below" else "idx64"
    p = lp.HubPattern(K, D, N)
    glo._need(24)
    rp, ci = p.csr(DEV)
    val = p.values(DEV)
    assert int(ci.max()) == p.K - 1 and int(rp[-1] - rp[-2]) == lp.HUB > 2048 and p.max_abs_sum() < (1 << 24)
    assert (p.K * N * 4 < (1 << 32)) == (side == "below")
    B = _dense(p, N)
    strict = _lib.FLAG_FORCE_IDX64 | _lib.FLAG_STRICT_ORDER
    assert "long_rows" not in _launch(p.M, p.K, N, p.nnz, flags=strict)
    want = spmm.csr_spmm(rp, ci, val, B, cfg={"flags": strict}, out=_nan((p.M, N)))
    _check_sum("strict idx64 with a hub row, K=%d" % K, p, N, want)
    out = _nan((p.M, N))
    for flags in (0, _lib.FLAG_SPLIT_LONG_ROWS):
        desc = _launch(p.M, p.K, N, p.nnz, flags=flags)
        assert "long_rows>2048" in desc and desc.split(" long_rows")[0].endswith(word), desc  # the pass is on, and the hub row is long
        out.fill_(float("nan"))
        spmm.csr_spmm(rp, ci, val, B, cfg={"flags": flags}, out=out)
        _check_sum("plain with a hub row, flags=%#x K=%d" % (flags, K), p, N, out)
        _same_bits("plain with a hub row, flags=%#x" % flags, out, want)
    out.fill_(float("nan"))
    spmm.csr_spmm_no_edge_value(rp, ci, B, cfg={"flags": 0}, out=out)
    _check_sum("plain unweighted with a hub row, K=%d" % K, p, N, out, weighted=False)
    for kernel, reorder, tag in (("stream", True, "long_rows>2048"), ("stream", False, "long_rows>2048"), ("staged", True, "hub_rows=1")):
        plan = spmm.SpmmPlan(rp, ci, p.K, N, values=val, reorder=reorder, kernel=kernel)
        desc = plan.describe()
        assert "max_degree=%d" % lp.HUB in desc and tag in desc and word in desc, desc
        assert (STAGED in desc) == (kernel == "staged"), desc
        what = "plan %s reorder=%s with a hub row, K=%d" % (kernel, reorder, K)
        out.fill_(float("nan"))
        spmm.csr_spmm(rp, ci, val, B, plan=plan, out=out)
        _check_sum(what, p, N, out)
        _same_bits(what, out, want)
        out.fill_(float("nan"))
        spmm.csr_spmm_no_edge_value(rp, ci, B, plan=plan, out=out)
        _check_sum(what + " unweighted", p, N, out, weighted=False)
        del plan


# ---- the fused product -----------------------------------------------------------------------------------------------------------------

def _cs(c):
    return c % 2 + 1          # column scale in {1, 2}


def _rs(r):
    return r % 3 - 1 + 3 * (r % 3 == 1)  # row scale in {-1, 3, 1}: no zero


def _bias(n):
    return n % 5 - 2


@pytest.mark.parametrize("side", ("below", "at"))
@pytest.mark.parametrize("kernel", (None, "stream", "seg-stream"), ids=("plain", "stream", "seg-stream"))
def test_fused_product(pkg, kernel, side):
    """((A (cs * B)) * rs) + bias with integer vectors: exact, so the fused kernel (route 1 / 2 below the switch), the composition
    (route 0 at it) and the four separate passes on 64-bit offsets have the same bits — and the windows equal the closed form."""
    from gespmm_amd import _lib, spmm

    N, K = 512, K512 + (side == "at")
    p, rp, ci, val = _inputs("both", K, N, arrays=4)
    B = _dense(p, N)
    i64 = lambda n: torch.arange(n, device=DEV, dtype=torch.int64)  # noqa: E731
    cs, rs, bias = _cs(i64(p.K)).float(), _rs(i64(p.M)).float(), _bias(i64(N)).float()
    assert bool((rs != 0).all())
    plan = None
    if kernel is not None:
        plan = spmm.SpmmPlan(rp, ci, p.K, N, values=val, reorder=True, kernel=kernel)
        want_route = 0 if side == "at" else (2 if kernel == "seg-stream" else 1)
        assert plan.fused_route(N) == want_route, plan.describe()
    else:
        assert _launch(p.M, p.K, N, p.nnz).split(" long_rows")[0].endswith("idx32" if side == "below" else "idx64")
    out = spmm.csr_spmm_fused(rp, ci, val, B, cs, rs, bias, out=_nan((p.M, N)), plan=plan)
    glo._written(out=out)

    def ref(r0, r1):
        b = lo.b_at(1, N)
        s = p.ref_sum(r0, r1, N, DEV, dense_fn=lambda c, h, n: _cs(c) * b(c, h, n))
        return s * _rs(i64(p.M)[r0:r1]).view(-1, 1) + _bias(i64(N)).view(1, -1)

    _check_windows("fused %s %s" % (kernel, side), out, p.windows(N), ref)
    scaled = B * cs.view(-1, 1)
    del B
    sep = spmm.csr_spmm(rp, ci, val, scaled, cfg={"flags": _lib.FLAG_FORCE_IDX64}, out=_nan((p.M, N)))
    del scaled
    sep.mul_(rs.view(-1, 1)).add_(bias.view(1, -1))
    _same_bits("fused %s %s vs four passes" % (kernel, side), out, sep)


# ---- 16-bit operands -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", ("below", "at"))
@pytest.mark.parametrize("kernel", (None, "stream", "seg-stream"), ids=("plain", "stream", "seg-stream"))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16), ids=("bf16", "fp16"))
@pytest.mark.parametrize("N,K", ((512, X512), (1024, X1024)), ids=("512", "1024"))
def test_x16_product(pkg, N, K, dtype, kernel, side):
    """K N 2 < 2^32: the 16-bit kernel (route 1 / 2); one row more: widen, the fp32 route (idx64, on an 8 GB scratch), narrow. Every
    sum is an integer of magnitude <= 45 — exact in bf16 (<= 256) and fp16."""
    from gespmm_amd import _lib, spmm

    K = K + (side == "at")
    p, rp, ci, val = _inputs("both", K, N, elem=2, arrays=5)
    assert p.max_abs_sum() <= 256
    assert (p.K * N * 2 < (1 << 32)) == (side == "below")
    B = _dense(p, N, dtype)
    code = {torch.float16: 1, torch.bfloat16: 2}[dtype]
    plan = None
    if kernel is not None:
        plan = spmm.SpmmPlan(rp, ci, p.K, N, values=val, reorder=True, kernel=kernel)
        want_route = 0 if side == "at" else (2 if kernel == "seg-stream" else 1)
        assert plan.x16_route(N) == want_route, plan.describe()
    else:
        # (the plain call at 2^23 entries and more has a long-row pass, which the 16-bit kernel lacks: the composition on both sides —
        #  only a plan, whose launches are in strict order, reaches the 16-bit kernel at these sizes)
        assert _lib.lib.gespmm_x16_route(p.M, p.K, N, p.nnz, -1, 16, 16) == 0
    # the composition's fp32 product on the widened scratch: 64-bit offsets (K N 4 is 8 GB)
    assert _launch(p.M, p.K, N, p.nnz).split(" long_rows")[0].endswith("idx64")
    assert plan is None or ("idx64" in plan.describe() and "idx32" not in plan.describe()), plan.describe()
    out = spmm.csr_spmm(rp, ci, val, B, plan=plan, out=_nan((p.M, N), dtype))
    if plan is not None:
        tag = "x16 %s N=%d route=%d " % ("f16" if code == 1 else "bf16", N, want_route)
        assert tag in plan.describe(), plan.describe()
    glo._written(out=out)
    _check_windows("x16 %s %s %s" % (dtype, kernel, side), out, p.windows(N, 2), lambda r0, r1: p.ref_sum(r0, r1, N, DEV))
    del plan
    wide = B.float()
    del B
    sep = spmm.csr_spmm(rp, ci, val, wide, cfg={"flags": _lib.FLAG_FORCE_IDX64}, out=_nan((p.M, N)))
    del wide
    _same_bits("x16 vs widen / fp32 / narrow", out, sep.to(dtype))


# ---- the multi-head product through a plan (what §4.2 left out) -------------------------------------------------------------------------

@pytest.mark.parametrize("reorder", (True, False), ids=("clustered", "storage"))
@pytest.mark.parametrize("side", glo.SIDES)
def test_heads_product_through_a_plan_across_the_4gb_switch(pkg, side, reorder):
    """SpmmPlan.run_heads, plain and with order=, at (H, F) = (8, 64): the sizes, windows and int64 closed forms of
    test_gpu_large_operands.py's section a; route 1 below the switch, the per-head composition at it."""
    from gespmm_amd import _lib, spmm

    H, F = 8, 64
    plans = {}

    def through_plan(rowptr, colind, values, dense, out=None, order=None):
        if not plans:
            plans[0] = spmm.SpmmPlan(rowptr, colind, dense.shape[0], H * F, reorder=reorder, kernel="stream")
            assert plans[0].heads_route(H, F) == (1 if side == "below" else 0), plans[0].describe()
        got = plans[0].run_heads(values, dense, out=out, order=order)
        assert "heads H=%d F=%d route=%d " % (H, F, 1 if side == "below" else 0) in plans[0].describe(), plans[0].describe()
        return got

    try:
        glo._heads_case(H, F, side, "rows", torch.float32, through_plan, _lib.heads_route)
    finally:
        plans.clear()
        glo._BANDS.clear()


# ---- SDDMM through a plan, its three routes (what §4.2 left out) --------------------------------------------------------------------------

SDDMM_ROUTES = ((0, 32, False), (1, 8, False), (2, 8, True))  # route, entries of a band row, reorder


@pytest.mark.parametrize("route,d,reorder", SDDMM_ROUTES, ids=("csr", "coo-row-ids", "clustered-scatter"))
@pytest.mark.parametrize("side", glo.SIDES)
def test_plan_sddmm_through_its_three_routes(pkg, side, route, d, reorder):
    """gespmm_plan_sddmm_f32 at N = 8 x 64 = 512 with D2 of large_operands.sizes_a "below" / "at" rows (2^32 bytes less one row, and one
    more): route 0 the CSR call (rows of 32 entries), 1 the COO form on row ids the plan expands once (storage order, 8 entries), 2 the
    clustered edge order and a scatter into the caller's (8 entries) — each asserted from gespmm_plan_sddmm_route. Integer operands of
    the word position; the entries of every window equal the int64 closed form, and the whole result has the stateless call's bits."""
    from gespmm_amd import _lib, sddmm, spmm

    N = 512
    K = lo.switch_rows(N) + (side == "at")
    M = K - band.offset_of(d - 1)
    if d == lo.D:
        assert (M, K) == lo.sizes_a(N, side, "rows")
    assert (K * N * 4 < (1 << 32)) == (side == "below")
    glo._need(24)
    rp, ci = band.csr(M, d, DEV)
    nnz = M * d
    rw, _ = lo.case_windows(M, K, N, 4, spread=6)
    assert rw[0][0] == 0 and rw[-1][1] == M
    d1, d2 = glo._nodes(M, 1, N).view(M, N), glo._nodes(K, 1, N, fn=lo.k_at(1, N)).view(K, N)
    plan = spmm.SpmmPlan(rp, ci, K, N, reorder=reorder)
    assert _lib.lib.gespmm_plan_sddmm_route(plan._handle, N) == route, plan.describe()
    assert plan.clustered == reorder, plan.describe()
    ref = lambda r0, r1: band.ref_csr_scores(M, d, r0, r1, 1, N, DEV, q_fn=lo.b_at(1, N), k_fn=lo.k_at(1, N))  # noqa: E731
    for call in range(2):  # (the second call reuses the plan's row ids / edge map)
        _poison((nnz,))
        s = sddmm.csr_sddmm(rp, ci, d1, d2, plan=plan)
        glo._written(s=s)
        _check_windows("plan sddmm route %d %s call %d" % (route, side, call), s.view(-1, 1), rw, ref, scale=d)
    _poison((nnz,))
    plain = sddmm.csr_sddmm(rp, ci, d1, d2)
    _same_bits("plan sddmm route %d vs the stateless call" % route, s, plain)
