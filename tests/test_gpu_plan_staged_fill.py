"""The fill pass of the staging tables (csrc/plan_device.hip: k_stage_select): slots of a block that the >= 2-use rule leaves
free go to columns the block uses ONCE whose own row lies in the block or within `w` blocks of it in the plan's order — nearest blocks
first, ties in column order. Only WHERE a B row comes from changes (LDS instead of a gather), so every product keeps the bits of the
oracle's `fma` chain and of the same plan built without the pass; the tables themselves are held to a numpy restatement of the rule.

GESPMM_STAGED_FILL (read when a plan is created) sets the window: 0 = no fill, unset = the policy's window."""
import re

import numpy as np
import pytest
import torch

from helpers import bits, edge_case_csr

pytestmark = pytest.mark.gpu

HUB = 2048  # longer rows leave the staged kernel (spmm_kernels.h: kStagedMaxRow)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _plan(monkeypatch, window, rp, ci, K, N, **kw):
    from gespmm_amd import spmm

    if window is None:
        monkeypatch.delenv("GESPMM_STAGED_FILL", raising=False)
    else:
        monkeypatch.setenv("GESPMM_STAGED_FILL", str(window))
    kw.setdefault("kernel", "staged")
    plan = spmm.SpmmPlan(rp, ci, K, N, **kw)
    monkeypatch.delenv("GESPMM_STAGED_FILL", raising=False)
    return plan


def _field(d, name):
    return d.split(name + "=")[1].split()[0]


def _untimed(d):
    """describe() without its stopwatch readings (tables=0.0012s, clustering 0.0013s ...): everything that is decided, nothing that is
    measured."""
    return re.sub(r"\b\d+\.\d+s\b", "<t>s", d)


def _tables(pkg, plan):
    """(staging lists [blocks, slots], rows per block, the window the tables were built with)"""
    lib = pkg._lib.lib
    info = np.zeros(4, dtype=np.int32)
    n = lib.gespmm_plan_debug_staging(plan._handle, info.ctypes.data, None, 0)
    assert n > 0 and n == int(info[0]) * int(info[1]), (n, info)
    hot = np.empty(n, dtype=np.int32)
    assert lib.gespmm_plan_debug_staging(plan._handle, info.ctypes.data, hot.ctypes.data, n) == n
    return hot.reshape(int(info[0]), int(info[1])), int(info[2]), int(info[3])


def _model(rowptr, colind, perm, R, H, w):
    """The rule, restated: per block of R rows of the matrix in `perm` order (rows beyond HUB entries empty) the staging list and the
    number of entries staged by the >= 2 rule / by the fill pass."""
    M = rowptr.size - 1
    rank = np.empty(M, dtype=np.int64)
    rank[perm] = np.arange(M)
    deg = np.diff(rowptr)
    lists, staged, filled, facts = [], 0, 0, []
    for b0 in range(0, M, R):
        b1 = min(b0 + R, M)
        rows = [r for r in perm[b0:b1] if deg[r] <= HUB]
        cols = np.concatenate([colind[rowptr[r]:rowptr[r + 1]] for r in rows]) if rows else np.zeros(0, dtype=np.int32)
        keys, cnt = np.unique(cols, return_counts=True)  # (column order)
        lenc = np.minimum(cnt, 255)
        multi = lenc >= 2
        hot = []
        if multi.sum() <= H:
            hot = list(keys[multi])
            staged += int(cnt[multi].sum())
            nfree = H - len(hot)
            once = keys[cnt == 1]
            cand, dist = [], []
            if w > 0 and nfree > 0 and once.size:
                rk = rank[once]
                d = np.where(rk < b0, (b0 - 1 - rk) // R + 1, np.where(rk >= b1, (rk - b1) // R + 1, 0))
                near = d <= w
                cand, dist = once[near], d[near]
            taken = 0
            if len(cand):
                fd, nlt = 0, 0
                while fd <= w and nlt + int((dist == fd).sum()) <= nfree:
                    nlt += int((dist == fd).sum())
                    fd += 1
                first = list(cand[dist < fd])
                second = list(cand[dist == fd][:nfree - nlt]) if fd <= w else []
                hot += first + second
                taken = len(first) + len(second)
                filled += taken
            facts.append({"multi": int(multi.sum()), "free": nfree, "cand": len(cand), "filled": taken,
                          "clipped_lo": b0 - w * R < 0, "clipped_hi": b1 + w * R > M})
        else:
            # more runs than slots: everything longer than t is staged, runs of length exactly t fill the rest, ties in column order
            t = next(L for L in range(255, 1, -1) if (lenc >= L).sum() > H)
            gt = lenc > t
            eq = keys[lenc == t][:H - int(gt.sum())]
            hot = list(keys[gt]) + list(eq)
            staged += int(cnt[gt].sum()) + int(cnt[np.isin(keys, eq)].sum())
            facts.append({"multi": int(multi.sum()), "free": 0, "cand": 0, "filled": 0, "clipped_lo": False, "clipped_hi": False})
        lists.append(np.array(hot + [-1] * (H - len(hot)), dtype=np.int32))
    return np.stack(lists), staged, filled, facts


def _check_products(oracle, plan, plan_off, rowptr, colind, rp, ci, K, N, seed):
    """valued, unweighted, new values on the same plan: the oracle's bits, and the bits of the plan without the fill pass."""
    from gespmm_amd import spmm

    nnz = colind.size
    B_h = oracle.hash_B(K, N, seed=seed + N)
    B = _dev(B_h)
    for vseed in (7, None, 8):  # (None: unweighted; the plans were created with the values of seed 7)
        if vseed is None:
            got = spmm.csr_spmm_no_edge_value(rp, ci, B, plan=plan).cpu().numpy()
            off = spmm.csr_spmm_no_edge_value(rp, ci, B, plan=plan_off).cpu().numpy()
            want = oracle.spmm(rowptr, colind, None, B_h, "golden")
        else:
            val_h = oracle.hash_val(nnz, seed=vseed)
            val = _dev(val_h)
            got = spmm.csr_spmm(rp, ci, val, B, plan=plan).cpu().numpy()
            off = spmm.csr_spmm(rp, ci, val, B, plan=plan_off).cpu().numpy()
            want = oracle.spmm(rowptr, colind, val_h, B_h, "fma")
        assert np.array_equal(bits(got), bits(want)), (N, vseed)
        assert np.array_equal(bits(got), bits(off)), (N, vseed, "fill on / off")


@pytest.fixture(scope="module")
def amazon(pkg):
    from gespmm_amd import graphs

    g = graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cpu", scale=0.02)  # ~6.7 k rows, ~37 k entries
    rowptr, colind = g["rowptr"].numpy(), g["colind"].numpy()
    return {"g": g, "rowptr": rowptr, "colind": colind, "rp": _dev(rowptr), "ci": _dev(colind), "K": g["K"]}


@pytest.mark.parametrize("N", (128, 256, 100, 32))  # tuned 128- / 256-column tiles, the general kernel, the lane-group kernel
def test_community_graph_bits_tables_and_counts(pkg, oracle, monkeypatch, amazon, N):
    a = amazon
    val = _dev(oracle.hash_val(a["colind"].size, seed=7))
    plan = _plan(monkeypatch, None, a["rp"], a["ci"], a["K"], N, values=val, reorder=True)
    plan_off = _plan(monkeypatch, 0, a["rp"], a["ci"], a["K"], N, values=val, reorder=True)
    d, d_off = plan.describe(), plan_off.describe()
    assert "kernel=staged-rows" in d and "kernel=staged-rows" in d_off, (d, d_off)
    print(d)
    assert float(_field(d, "filled_entries")) > 0.0, d
    assert _field(d_off, "filled_entries") == "0.000", d_off
    assert _field(d, "staged_entries") == _field(d_off, "staged_entries"), (d, d_off)
    # two builds of the same plan: the same description and the same tables
    plan2 = _plan(monkeypatch, None, a["rp"], a["ci"], a["K"], N, values=val, reorder=True)
    assert _untimed(plan2.describe()) == _untimed(d)
    hot, R, w = _tables(pkg, plan)
    assert np.array_equal(hot, _tables(pkg, plan2)[0])
    # the tables against the rule restated in numpy: with the policy's window, and none
    assert w > 0
    perm = plan.order().numpy().astype(np.int64)
    want, staged, filled, _ = _model(a["rowptr"], a["colind"], perm, R, hot.shape[1], w)
    assert np.array_equal(hot, want)
    nnz = a["colind"].size
    assert _field(d, "staged_entries") == "%.3f" % (staged / nnz) and _field(d, "filled_entries") == "%.3f" % (filled / nnz), (d, staged, filled)
    hot_off, R_off, w_off = _tables(pkg, plan_off)
    assert (R_off, w_off) == (R, 0) and np.array_equal(hot_off, _model(a["rowptr"], a["colind"], perm, R, hot.shape[1], 0)[0])
    _check_products(oracle, plan, plan_off, a["rowptr"], a["colind"], a["rp"], a["ci"], a["K"], N, seed=1)


def _three_kinds_of_block(R, H):
    """Five blocks of R rows in the identity order (the last one ragged). Block 1: more than H columns used twice — nothing to fill.
    Block 2: a few shared columns and several single-use columns per row whose own rows lie 0, 1, 2 and 3+ blocks away — more near ones
    than free slots. Blocks 0 and 4: near columns whose window reaches past the first / last row of the matrix."""
    rng = np.random.RandomState(11)
    M = 4 * R + R // 2 + 3
    rows = [[] for _ in range(M)]
    for i in range(R // 2):  # block 1: pairs of rows share 3 columns: 3 * R / 2 >= H + 8 distinct columns, two uses each
        shared = [300 + 3 * i + j for j in range(3)]
        rows[R + 2 * i] += shared
        rows[R + 2 * i + 1] += shared + [int(rng.randint(R, 2 * R))]  # (a near single-use column: must stay a gather)
    assert 3 * (R // 2) > H
    for r in range(2 * R, 3 * R):  # block 2
        rows[r] += [2 * R + (r % 5), 2 * R + 5 + (r % 3)]  # 8 columns used again and again
        rows[r] += [int(c) for c in rng.randint(0, M, size=3)]  # spread over every block: distance 0, 1, 2 and beyond
    for r in list(range(0, R)) + list(range(4 * R, M)):  # blocks 0 and 4: columns from the three blocks at their end of the matrix
        lo, hi = (0, 3 * R) if r < R else (2 * R, M)
        rows[r] += [int(c) for c in rng.randint(lo, hi, size=2)] + [int(rng.randint(0, M))]
    for r in range(3 * R, 4 * R):  # block 3: short rows, one empty now and then
        rows[r] += [int(c) for c in rng.randint(2 * R, M, size=r % 3)]
    degs = np.array([len(x) for x in rows])
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    colind = np.array([c for x in rows for c in x], dtype=np.int32)
    return rowptr, colind, M


@pytest.mark.parametrize("window", (1, 2, 4))
def test_hand_made_blocks_full_overflowing_and_clipped(pkg, oracle, monkeypatch, window):
    N, R, H = 128, 112, 160  # (mean degree <= 24 at 128-column tiles: 112 rows per block, 160 slots)
    rowptr, colind, M = _three_kinds_of_block(R, H)
    rp, ci = _dev(rowptr), _dev(colind)
    val = _dev(oracle.hash_val(colind.size, seed=7))
    plan = _plan(monkeypatch, window, rp, ci, M, N, values=val, reorder=False)
    plan_off = _plan(monkeypatch, 0, rp, ci, M, N, values=val, reorder=False)
    assert "order=storage" in plan.describe() and "kernel=staged-rows" in plan.describe(), plan.describe()
    hot, R_plan, w_plan = _tables(pkg, plan)
    assert (R_plan, hot.shape[1], w_plan) == (R, H, window)
    want, staged, filled, facts = _model(rowptr, colind, np.arange(M), R, H, window)
    # the matrix is what its docstring says
    assert facts[1]["multi"] > H and facts[1]["filled"] == 0
    assert facts[2]["cand"] > facts[2]["free"] > 0 and facts[2]["filled"] == facts[2]["free"]
    assert facts[0]["clipped_lo"] and facts[0]["filled"] > 0 and facts[4]["clipped_hi"] and facts[4]["filled"] > 0
    for b in range(hot.shape[0]):
        assert np.array_equal(hot[b], want[b]), (b, facts[b])
    d = plan.describe()
    assert _field(d, "staged_entries") == "%.3f" % (staged / colind.size) and _field(d, "filled_entries") == "%.3f" % (filled / colind.size), d
    assert np.array_equal(_tables(pkg, plan_off)[0], _model(rowptr, colind, np.arange(M), R, H, 0)[0])
    _check_products(oracle, plan, plan_off, rowptr, colind, rp, ci, M, N, seed=2)


@pytest.mark.parametrize("N", (128, 256))
def test_rectangular_matrix_is_not_filled(pkg, oracle, monkeypatch, N):
    g = edge_case_csr(seed=4)  # K != M: a column has no home row
    rp, ci = _dev(g["rowptr"]), _dev(g["colind"])
    val = _dev(oracle.hash_val(g["nnz"], seed=7))
    plans = [_plan(monkeypatch, w, rp, ci, g["K"], N, values=val, reorder=True) for w in (None, 4, 0)]
    for p in plans:
        assert "kernel=staged-rows" in p.describe() and _field(p.describe(), "filled_entries") == "0.000", p.describe()
        assert _tables(pkg, p)[2] == 0
    assert np.array_equal(_tables(pkg, plans[0])[0], _tables(pkg, plans[2])[0])
    assert np.array_equal(_tables(pkg, plans[1])[0], _tables(pkg, plans[2])[0])
    _check_products(oracle, plans[0], plans[2], g["rowptr"], g["colind"], rp, ci, g["K"], N, seed=3)


@pytest.mark.parametrize("reorder", (True, False))
def test_hub_row_among_community_rows_strict_order(pkg, oracle, monkeypatch, reorder):
    """One row beyond 2048 entries is split off; the fill works on what is left. Rows of a band: row r uses columns r - 40 .. r + 40."""
    rng = np.random.RandomState(5)
    M = K = 3000
    degs = rng.randint(2, 9, size=M)
    degs[1234] = 2500
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    rows = np.repeat(np.arange(M), degs)
    colind = np.clip(rows + rng.randint(-40, 41, size=rows.size), 0, K - 1).astype(np.int32)
    hub = slice(rowptr[1234], rowptr[1235])
    colind[hub] = rng.randint(0, K, size=2500)
    rp, ci = _dev(rowptr), _dev(colind)
    val = _dev(oracle.hash_val(colind.size, seed=7))
    N = 128
    plan = _plan(monkeypatch, None, rp, ci, K, N, values=val, reorder=reorder, flags=0x100)  # GESPMM_FLAG_STRICT_ORDER
    plan_off = _plan(monkeypatch, 0, rp, ci, K, N, values=val, reorder=reorder, flags=0x100)
    d = plan.describe()
    assert "kernel=staged-rows" in d and "hub_rows=1" in d, d
    hot, R, w = _tables(pkg, plan)
    assert w > 0
    perm = plan.order().numpy().astype(np.int64)
    want, _, filled, _ = _model(rowptr, colind, perm, R, hot.shape[1], w)
    assert np.array_equal(hot, want)
    if not reorder:  # (the band IS the order: every single-use column is near)
        assert filled > 0 and float(_field(d, "filled_entries")) > 0.0, d
    _check_products(oracle, plan, plan_off, rowptr, colind, rp, ci, K, N, seed=4)


def test_identity_order_plan_uses_the_row_numbers(pkg, oracle, monkeypatch, amazon):
    """A graph that arrives in its community order, the plan told to keep it: rank[i] = i."""
    from gespmm_amd import graphs

    g = amazon["g"]
    order = torch.argsort(g["truth"].long(), stable=True)
    rp_t, ci_t = graphs.relabel_by_order(g["rowptr"], g["colind"], order)
    rowptr, colind = rp_t.numpy(), ci_t.numpy()
    rp, ci = _dev(rowptr), _dev(colind)
    K, N = g["K"], 128
    val = _dev(oracle.hash_val(colind.size, seed=7))
    plan = _plan(monkeypatch, None, rp, ci, K, N, values=val, reorder=False)
    plan_off = _plan(monkeypatch, 0, rp, ci, K, N, values=val, reorder=False)
    d = plan.describe()
    assert "order=storage" in d and "kernel=staged-rows" in d and float(_field(d, "filled_entries")) > 0.0, d
    assert _field(d, "staged_entries") == _field(plan_off.describe(), "staged_entries")
    hot, R, w = _tables(pkg, plan)
    assert w > 0
    want, _, filled, _ = _model(rowptr, colind, np.arange(K), R, hot.shape[1], w)
    assert filled > 0 and np.array_equal(hot, want)
    _check_products(oracle, plan, plan_off, rowptr, colind, rp, ci, K, N, seed=5)
