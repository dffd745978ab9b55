"""Host checks behind test_gpu_large_products.py (no device).

* Sizes and routes: every row count of the GPU cases is the last one its kernel is offered (R = floor((bound - 1) / row bytes)) or
  one more, as the host-only entry points answer — ``_lib.plan_policy`` (build_staged / build_records), the idx32 / idx64 word of
  the launch description — on BOTH sides of every switch.
* The reference itself: on a small instance of each pattern the closed form equals a dense float64 product and ``oracle.spmm``.
* Each comparison can fail: for every marked window of every case the reference is recomputed through a B byte offset displaced by
  2^31 and by 2^32 (modulo 2^32: ``large_operands.displaced``), through a C row displaced the same way (row r keeps NaN) and, for the
  two-halves form of the tuned staged kernel, through the wrong half (B -+ 4 GB; C rows stored 4 GB too high or too low:
  ``large_products.wrong_half_c``). The equality check rejects the B cases, the NaN check alone rejects the C cases. A displacement is asked of a case where it lands INSIDE the operand (one
  that leaves it is a fault, not a wrong value).
* Windows: the marked rows lie inside the compared windows, and the far columns of the window rows reach every half of B and its last
  row."""
import ctypes

import numpy as np
import pytest
import torch

import band
import large_operands as lo
import large_products as lp

D = lp.D
PLAN_CASES = [("staged",) + c for c in lp.TUNED + lp.NARROW + lp.GENERAL] + [("records",) + c for c in lp.RECORD]
STREAM_CASES = [(512, lp.K512, 4), (300, lp.K300, 4), (512, lp.X512, 2), (1024, lp.X1024, 2)]
# (kind, R, N, elem) of every GPU case that is offered its kernel, once each
SHAPES = sorted({(c[3], c[2], c[1], 4) for c in PLAN_CASES if c[5]} | {("both", K, N, e) for N, K, e in STREAM_CASES}
                | {("both", K + 1, N, e) for N, K, e in STREAM_CASES})
SHAPE_IDS = ["%s-%d-%d-%d" % s for s in SHAPES]
HALF = 128  # rows on each side of a marked row that the rejection tests recompute (a part of the marked row's 4096-row window)


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _launch(L, M, K, N, nnz, variant=-1, flags=0):
    buf = ctypes.create_string_buffer(256)
    cfg = L.LaunchCfg(0, 0, 0, 0, 0, flags)
    assert L.lib.gespmm_describe_launch(M, K, N, nnz, variant, ctypes.byref(cfg), buf, 256) > 0
    return buf.value.decode()


def _idx(desc):
    return desc.split(" long_rows")[0].split()[-1]


# ---- sizes and routes ------------------------------------------------------------------------------------------------------------------

def test_the_row_counts():
    assert (lp.R128, lp.R256, lp.R512, lp.R512P, lp.R1024, lp.R1024P) == (8_388_479, 4_194_239, 2_097_119, 4_194_271, 1_048_559, 2_097_135)
    assert (lp.R64, lp.R602, lp.R100) == (16_776_959, (0xFFFF0000 - 1) // 2408, 10_737_254)
    assert (lp.REC64, lp.REC48) == (16_777_215, 22_369_621)
    assert (lp.K512, lp.K300, lp.X512, lp.X1024) == (2_097_151, (2 ** 32 - 1) // 1200, 4_194_303, 2_097_151)
    for bound, N, R in ((lp.TABLE_BOUND, 128, lp.R128), (lp.TABLE_BOUND_PAGED, 512, lp.R512P), (lp.BYTE_BOUND, 48, lp.REC48)):
        assert R * N * 4 < bound <= (R + 1) * N * 4


@pytest.mark.parametrize("kernel,bound,N", [("staged", lp.TABLE_BOUND, 128), ("staged", lp.TABLE_BOUND, 256), ("staged", lp.TABLE_BOUND_PAGED, 512),
                                            ("staged", lp.TABLE_BOUND_PAGED, 1024), ("staged", lp.TABLE_BOUND, 64), ("staged", lp.TABLE_BOUND, 602),
                                            ("staged", lp.TABLE_BOUND, 100), ("records", lp.BYTE_BOUND, 64), ("records", lp.BYTE_BOUND, 48)])
def test_a_table_kernel_is_offered_up_to_its_bound_and_not_one_row_further(L, kernel, bound, N):
    """At R = floor((bound - 1) / row bytes) rows the tables are built, at R + 1 they are not — whichever of M and K is the larger, for a
    forced clustered plan (records: and for one in storage order)."""
    R = lp.last_row_below(bound, N)
    kern = {"staged": L.PLAN_KERNEL_STAGED, "records": L.PLAN_KERNEL_RECORDS}[kernel]
    field = {"staged": "build_staged", "records": "build_records"}[kernel]
    # (a storage-order plan with a forced staged kernel becomes an identity-order copy at creation: the policy is asked as for a clustered one)
    for reorder in (L.PLAN_REORDER,) + ((L.PLAN_NO_REORDER,) if kernel == "records" else ()):
        for M, K in ((R, R), (R, lp.K_TALL), (lp.M_WIDE, R), (R - 9, R)):
            assert L.plan_policy(M, K, 5 * M, N, 5, kernel=kern, reorder=reorder)[field] == 1, (M, K, reorder)
        for M, K in ((R + 1, R + 1), (R + 1, lp.K_TALL), (lp.M_WIDE, R + 1), (R - 8, R + 1)):
            assert L.plan_policy(M, K, 5 * M, N, 5, kernel=kern, reorder=reorder)[field] == 0, (M, K, reorder)
    if kernel == "records":  # rows stay at or below kRecordMaxRow
        assert L.plan_policy(R, R, 5 * R, N, 1024, kernel=kern, reorder=L.PLAN_REORDER)[field] == 1
        assert L.plan_policy(R, R, 5 * R, N, 1025, kernel=kern, reorder=L.PLAN_REORDER)[field] == 0


@pytest.mark.parametrize("kernel,N,R,kind,reorder,served,idx", PLAN_CASES)
def test_every_plan_case_lies_on_its_side_of_the_switch(L, kernel, N, R, kind, reorder, served, idx):
    p = lp.Pattern(kind, R, D)
    assert max(p.M, p.K) == R and p.nnz < (1 << 31)
    kern = {"staged": L.PLAN_KERNEL_STAGED, "records": L.PLAN_KERNEL_RECORDS}[kernel]
    ans = L.plan_policy(p.M, p.K, p.nnz, N, D + 1, kernel=kern, reorder=L.PLAN_REORDER if reorder or kernel == "staged" else L.PLAN_NO_REORDER)
    assert ans["build_staged" if kernel == "staged" else "build_records"] == int(served)
    bound = lp.BYTE_BOUND if kernel == "records" else (lp.TABLE_BOUND_PAGED if N in (512, 1024) else lp.TABLE_BOUND)
    assert (R * N * 4 < bound) == served
    if not served:
        assert (R - 1) * N * 4 < bound, "one row past the last size offered, no more"
    assert _idx(_launch(L, p.M, p.K, N, p.nnz)) == idx  # what the plan falls back to (and the max reducer / other widths take)
    assert (p.K * N * 4 >= (1 << 32)) == (idx == "idx64")


@pytest.mark.parametrize("N,K,elem", STREAM_CASES)
def test_the_streaming_kernels_switch_to_64_bit_offsets_at_4gb(L, N, K, elem):
    """fp32: K N 4; 16-bit operands: the geometry is that of half the width in 32-bit words, so K N 2."""
    Nw = N * elem // 4
    for variant in (-1, 1, 2, 4):
        for flags in (0, L.FLAG_STRICT_ORDER, L.FLAG_SEG_STREAM | L.FLAG_STRICT_ORDER, L.FLAG_BATCH_STREAM, L.FLAG_SLAB_BLOCKED, L.FLAG_SPLIT_LONG_ROWS):
            assert _idx(_launch(L, K - 9, K, Nw, 5 * (K - 9), variant, flags)) == "idx32", (variant, flags)
            assert _idx(_launch(L, K - 8, K + 1, Nw, 5 * (K - 8), variant, flags)) == "idx64", (variant, flags)
    assert K * N * elem < (1 << 32) <= (K + 1) * N * elem
    assert _idx(_launch(L, K - 9, K, Nw, 5 * (K - 9), -1, L.FLAG_FORCE_IDX64)) == "idx64"  # the independent path of the GPU cases
    if elem == 2:  # the plain 16-bit call at these sizes: the long-row pass of 2^23 entries and more has no 16-bit kernel
        assert L.lib.gespmm_x16_route(K - 9, K, N, 5 * (K - 9), -1, 16, 16) == 0
        assert L.lib.gespmm_x16_route(100000, 100009, N, 500000, -1, 16, 16) in (1, 2)


# ---- the reference itself ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,R", (("both", 5009), ("tall", 5000), ("wide", 20000)))
@pytest.mark.parametrize("N", (16, 100))
def test_closed_form_equals_a_dense_product_and_the_oracle(oracle, kind, R, N):
    p = lp.Pattern(kind, R, 6).set_marks(N)
    rp, ci = p.csr()
    val = p.values()
    assert rp.numel() == p.M + 1 and int(rp[-1]) == p.nnz and int(ci.min()) >= 0 and int(ci.max()) == p.K - 1
    assert torch.equal(ci.view(p.M, p.w).to(torch.int64), p.cols(0, p.M))
    assert all(int(ci[r * p.w + j]) == p.col(r, j) for r in (0, 1, 127, 128, p.M - 1) for j in range(p.w))  # the scalar form
    B = band.node_values(p.K, 1, N, dtype=torch.float64, fn=lo.b_at(1, N)).view(p.K, N)
    A = torch.zeros((p.M, p.K), dtype=torch.float64)
    rows = torch.arange(p.M).repeat_interleave(p.w)
    A.index_put_((rows, ci.long()), val.double(), accumulate=True)
    ref = p.ref_sum(0, p.M, N)
    assert int(ref.abs().max()) <= p.max_abs_sum()
    assert torch.equal(A @ B, ref.double())
    got = oracle.spmm(rp.numpy(), ci.numpy(), val.numpy(), B.float().numpy(), "fma")
    assert np.array_equal(got, ref.float().numpy())
    ones = torch.zeros((p.M, p.K), dtype=torch.float64)
    ones.index_put_((rows, ci.long()), torch.ones(p.nnz, dtype=torch.float64), accumulate=True)
    assert torch.equal(ones @ B, p.ref_sum(0, p.M, N, weighted=False).double())
    mx = p.ref_max(0, p.M, N)
    assert np.array_equal(oracle.spmm_max(rp.numpy(), ci.numpy(), B.float().numpy(), lp.EMPTY), mx.float().numpy())
    assert int(mx.min()) >= -3 and lp.EMPTY < -3


# ---- windows ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,R,N,elem", SHAPES, ids=SHAPE_IDS)
def test_windows_hold_the_marked_rows_and_reach_every_half(kind, R, N, elem):
    p = lp.Pattern(kind, R, D).set_marks(N, elem)
    wins = p.windows(N, elem)
    assert wins[0][0] == 0 and wins[-1][1] == p.M and all(0 <= a < b <= p.M and b - a <= band.WINDOW for a, b in wins)
    for m in lo.marked(p.M, N, elem):  # C's rows with byte 2^31, byte 2^32 and its last
        assert lo.holds(wins, m), m
    if kind == "both":  # the rows whose band gathers B's marked rows
        for m in lo.marked(p.K, N, elem):
            for j in range(D):
                r = m - band.offset_of(j)
                assert not (0 <= r < p.M) or lo.holds(wins, r), (m, j)
    halves, last = lp.far_reach(p, wins, N, elem)
    want = [0] + [i + 1 for i, b in enumerate(lo.BYTES) if p.K * N * elem > b + N * elem]
    assert halves == want and last, (halves, want, last)
    if kind == "wide":  # every marked row of B, and the row before it, is some window row's far column
        far = set(p.far(torch.arange(p.M, dtype=torch.int64)).tolist())
        assert all(m in far and max(m - 1, 0) in far for m in p.marks_wide)


# ---- each comparison can fail -------------------------------------------------------------------------------------------------------------

def _near(p, m):
    return max(m - HALF, 0), min(m + HALF, p.M)


def _b_marked_windows(p, N, elem):
    """Row ranges inside the compared windows around every marked row (of C, and — both — of the rows that gather B's marked rows)."""
    marks = list(lo.marked(p.M, N, elem))
    if p.kind == "both":
        marks += [min(m, p.M - 1) for m in lo.marked(p.K, N, elem)]
    out = sorted({_near(p, m) for m in marks})
    wins = p.windows(N, elem)
    assert all(any(a <= r0 and r1 <= b for a, b in wins) for r0, r1 in out)
    return out


def _wrong_half(fn, N, rows):
    """B read from the other 4 GB half: word w -+ 2^30 where that lies inside the operand."""
    def at(r, h, f):
        w = r * N + f
        alias = torch.where(w >= (1 << 30), w - (1 << 30), w + (1 << 30))
        return lo.value_at_word(fn, torch.where(alias < rows * N, alias, w), 1, N)

    return at


@pytest.mark.parametrize("kind,R,N,elem", SHAPES, ids=SHAPE_IDS)
def test_a_displaced_b_offset_is_rejected_in_every_marked_window(kind, R, N, elem):
    p = lp.Pattern(kind, R, D).set_marks(N, elem)
    b = lo.b_at(1, N)
    asked = 0
    for shift in lo.BYTES:
        if p.K * N * elem <= shift:
            continue  # no word of B has its alias inside B: the displaced load leaves the operand
        fn = lo.displaced(b, 1, N, shift, p.K, elem)
        last = False
        for r0, r1 in _b_marked_windows(p, N, elem):
            if bool((p._gathered(r0, r1, N, "cpu", fn) == p._gathered(r0, r1, N, "cpu", b)).all()):
                continue  # (B ends a few bytes past the shift: these rows gather no word that has an alias)
            for weighted in (True, False):
                got = p.ref_sum(r0, r1, N, dense_fn=fn, weighted=weighted)
                wrong = int((got != p.ref_sum(r0, r1, N, weighted=weighted)).sum())
                assert wrong > 0, (shift, r0, r1, weighted)
            assert bool((p.ref_max(r0, r1, N, dense_fn=fn) != p.ref_max(r0, r1, N)).any()), (shift, r0, r1, "max")
            asked += 1
            last = r1 == p.M
        assert last, (shift, "the window with the last row gathers the last row of B, which has an alias")
    assert asked > 0 or p.K * N * elem <= lo.BYTES[0]
    if p.K * N * elem > (1 << 32):  # the two-halves form (and every 64-bit path): the wrong half
        fn = _wrong_half(b, N, p.K)
        last = False
        for r0, r1 in _b_marked_windows(p, N, elem):
            if bool((p._gathered(r0, r1, N, "cpu", fn) == p._gathered(r0, r1, N, "cpu", b)).all()):
                continue
            assert bool((p.ref_sum(r0, r1, N, dense_fn=fn) != p.ref_sum(r0, r1, N)).any()), (r0, r1)
            last = r1 == p.M
        assert last


@pytest.mark.parametrize("kind,R,N,elem", SHAPES, ids=SHAPE_IDS)
def test_a_displaced_c_row_is_rejected_by_the_nan_check_alone(kind, R, N, elem):
    """Row r's sums land in the alias row, row r keeps its NaN: around every marked row of C some row stays unwritten."""
    p = lp.Pattern(kind, R, D).set_marks(N, elem)
    size = p.M * N * elem
    for shift in lo.BYTES:
        if size <= shift:
            continue
        for m in lo.marked(p.M, N, elem):
            r0, r1 = _near(p, m)
            ref = p.ref_sum(r0, r1, N)
            moved = lp.displaced_c(ref, r0, N, shift, p.M, elem)
            if (m + 1) * N * elem > shift:  # the marked row holds byte ``shift`` or lies past it: the rows behind it move down, inside C
                assert bool(torch.isnan(moved).any()), (shift, m)


@pytest.mark.parametrize("kind,R,N,elem", [c for c in SHAPES if c[0] != "wide" and (c[1] - 9) * c[2] * c[3] > (1 << 32)],
                         ids=[i for c, i in zip(SHAPES, SHAPE_IDS) if c[0] != "wide" and (c[1] - 9) * c[2] * c[3] > (1 << 32)])
def test_a_c_row_stored_into_the_wrong_half_is_rejected_by_the_nan_check_alone(kind, R, N, elem):
    """C past 4 GB (the two-halves form, and every 64-bit path): a block that stores its rows with the other base — rows below row
    2^32 / row bytes at r + 2^32 / row bytes, rows past it 4 GB lower — leaves the rows it should have written NaN, around EVERY marked row."""
    p = lp.Pattern(kind, R, D).set_marks(N, elem)
    page = (1 << 32) // (N * elem)
    assert p.M * N * elem > (1 << 32)
    for m in lo.marked(p.M, N, elem):
        r0, r1 = _near(p, m)
        ref = p.ref_sum(r0, r1, N)
        assert not bool(torch.isnan(ref.double()).any())
        moved = lp.wrong_half_c(ref, r0, N, p.M, elem)
        assert bool(torch.isnan(moved).any()), m
        rows = torch.arange(r0, r1)
        lands = torch.where(rows >= page, rows - page, rows + page) < p.M
        assert torch.equal(torch.isnan(moved).all(1), lands) and bool(lands[m - r0]), m  # the marked row itself is among the moved


@pytest.mark.parametrize("R,N", ((20000, 16), (9000, 100)))
def test_hub_pattern_closed_form_equals_a_dense_product_and_the_oracle(oracle, R, N):
    p = lp.HubPattern(R, D, N)
    rp, ci = p.csr()
    val = p.values()
    assert p.M == p.rows + 1 and int(rp[-1]) == p.nnz == p.rows * (D + 1) + lp.HUB and int(rp[-1] - rp[-2]) == lp.HUB > 2048
    assert int(ci.min()) >= 0 and int(ci.max()) == p.K - 1 and val.numel() == p.nnz
    hub = ci[p.rows * p.w:].long()
    assert all(m in hub.tolist() for m in lo.marked(p.K, N)) and int(hub[0]) == 0 and int(hub[:lp.HUB - len(p.tail)].max()) > p.K // 2
    B = band.node_values(p.K, 1, N, dtype=torch.float64, fn=lo.b_at(1, N)).view(p.K, N)
    rows = torch.repeat_interleave(torch.arange(p.M), (rp[1:] - rp[:-1]).long())
    for weighted in (True, False):
        A = torch.zeros((p.M, p.K), dtype=torch.float64)
        A.index_put_((rows, ci.long()), val.double() if weighted else torch.ones(p.nnz, dtype=torch.float64), accumulate=True)
        ref = p.ref_sum(0, p.M, N, weighted=weighted)
        assert ref.shape == (p.M, N) and int(ref.abs().max()) <= p.max_abs_sum() < (1 << 24)
        assert torch.equal(A @ B, ref.double())
    got = oracle.spmm(rp.numpy(), ci.numpy(), val.numpy(), B.float().numpy(), "fma")
    assert np.array_equal(got, p.ref_sum(0, p.M, N).float().numpy())
    wins = p.windows(N)
    assert wins[-1][1] == p.M, "the hub row lies in the last window"
    # a displaced B offset shows in the hub row's sum (small instance: B below 2 GB, so the displacement is scaled to its size)
    for K, Nw in ((lp.K512, 512), (lp.K512 + 1, 512)):
        big = lp.HubPattern(K, D, Nw)
        strided = big.hub_cols()[:lp.HUB - len(big.tail)]
        assert int(strided.max()) * Nw * 4 > 0xF0000000 and bool((strided * Nw * 4 < (1 << 31)).any())  # over all of B, bit 31 clear and set
        for shift in lo.BYTES:
            if big.K * Nw * 4 <= shift:
                continue
            fn = lo.displaced(lo.b_at(1, Nw), 1, Nw, shift, big.K)
            assert bool((big._hub(Nw, "cpu", fn, True, "sum") != big._hub(Nw, "cpu", lo.b_at(1, Nw), True, "sum")).any()), (K, shift)


def test_a_hub_row_turns_the_long_row_pass_of_a_plan_on(L):
    """The plan's streaming launch is in strict order (0x100) until the matrix has a row past 2048 entries: then the long-row pass (0x200)."""
    p = lp.HubPattern(lp.K512, D, 512)
    for kern in (L.PLAN_KERNEL_STREAM, L.PLAN_KERNEL_STAGED):
        assert L.plan_policy(p.M, p.K, p.nnz, 512, D + 1, kernel=kern, reorder=L.PLAN_REORDER)["launch_flags"] == L.FLAG_STRICT_ORDER
        assert L.plan_policy(p.M, p.K, p.nnz, 512, lp.HUB, kernel=kern, reorder=L.PLAN_REORDER)["launch_flags"] == L.FLAG_SPLIT_LONG_ROWS
    for K, word in ((lp.K512, "idx32"), (lp.K512 + 1, "idx64")):
        p = lp.HubPattern(K, D, 512)
        desc = _launch(L, p.M, p.K, 512, p.nnz)
        assert "long_rows>2048" in desc and _idx(desc) == word and lp.HUB > 2048
