"""The aggregate-and-linear kernels where their 32-bit element positions are largest: large_linear.py's cases (one array past 2^32 bytes
or at the entry's limit of 2^31 - 4097 elements, or R M past 2^26 stacked rows; test_large_linear_host.py derives the sizes). Closed-form
integer operands, so every comparison is exact: the windows round the marked rows against an int64 reference made on the HOST from the
closed forms alone, then the whole result against the same closed forms on the device, in slices. The route function must answer 1
before every launch. A case skips itself only when the device has too little free memory, never on a device of 64 GB or more."""
import time

import pytest
import torch

import band
import large_linear as ll

pytestmark = pytest.mark.gpu

TD = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
SLICE = 1 << 18
CASES = ll.cases()


def _fill(fn, rows, K, dtype):
    out = torch.empty((rows, K), dtype=dtype, device="cuda")
    for r0 in range(0, rows, SLICE):
        r1 = min(r0 + SLICE, rows)
        out[r0:r1] = ll.dense(fn, r0, r1, K, "cuda")
    return out


def _operands(c):
    R, M, K, N_out, d = (c[k] for k in ("R", "M", "K", "N_out", "d"))
    dtype = TD[c["dt"]]
    rp = (torch.arange(R * M + 1, device="cuda", dtype=torch.int64) * d).to(torch.int32)
    ci = band.csr(M, d, "cuda")[1].repeat(R)
    val = ll.value_at(torch.arange(c["nnz"], device="cuda", dtype=torch.int32)).float() if c["valued"] else None
    scale = (ll.scale2_at(torch.arange(R * M, device="cuda", dtype=torch.int32)).float() / 2) if c["scaled"] else None
    return rp, ci, val, scale, _fill(ll.x_at, c["Kn"], K, dtype)


def _need_memory(c):
    free, total = torch.cuda.mem_get_info()
    need = ll.memory_needed(c)
    if free < need:
        assert total < 64 << 30, "a device of %d GB must run every case (%d GB free, %d GB needed)" % (total >> 30, free >> 30, need >> 30)
        pytest.skip("needs %d GB of device memory, %d GB free" % (need >> 30, free >> 30))


def _equal2(got, want2):
    """Every word of ``got`` is half the int64 ``want2`` (NaN equals nothing)."""
    return bool((got.double() * 2 == want2.to(got.device).double()).all())


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n]["op"] != "wgrad"])
def test_forward(pkg, name):
    from gespmm_amd import spmm

    c = CASES[name]
    _need_memory(c)
    t0 = time.perf_counter()
    R, M, K, N_out = (c[k] for k in ("R", "M", "K", "N_out"))
    dtype = TD[c["dt"]]
    rp, ci, val, scale, X = _operands(c)
    W = ll.weights(R, N_out, K, device="cuda").to(dtype)
    root = _fill(ll.root_at, M, K, dtype) if c["root"] else None
    rw = ll.weights(1, N_out, K, terms=2, device="cuda")[0].to(dtype) if c["root"] else None
    bias = ll.bias_at(torch.arange(N_out, device="cuda")).float()
    out = torch.full((M, N_out), float("nan"), dtype=dtype, device="cuda")
    assert ll.route(c) == 1 and spmm.x16_align(X, W, root, rw, out) == 16
    if c["op"] == "linear":
        got = spmm.csr_spmm_linear(rp, ci, val, X, W[0], row_scale=scale, root=root, root_weight=rw, bias=bias, out=out)
    else:
        got = spmm.csr_spmm_relational_linear(rp, ci, val, X, W, row_scale=scale, root=root, root_weight=rw, bias=bias, out=out)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for mark in ll.marked_rows(c):  # the windows round the marked rows: int64 closed forms on the host
        i0 = min(max(mark - 2048, 0), max(M - band.WINDOW, 0))
        i1 = min(i0 + band.WINDOW, M)
        diff = band.first_difference(got[i0:i1].double().cpu() * 2, ll.ref_forward2(c, i0, i1).double())
        assert diff is None, (name, "window of row %d" % mark, diff)
    bad = 0
    for i0 in range(0, M, SLICE):  # the whole result, on the device
        i1 = min(i0 + SLICE, M)
        bad += int((got[i0:i1].double() * 2 != ll.ref_forward2(c, i0, i1, "cuda").double()).sum())
    assert bad == 0, (name, "%d words of the whole result differ" % bad)
    torch.cuda.synchronize()
    print("%s: M=%d Kn=%d K=%d N_out=%d R=%d nnz=%d: operands and launch %.1f s, checks %.1f s"
          % (name, M, c["Kn"], K, N_out, R, c["nnz"], t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n]["op"] == "wgrad"])
def test_weight_gradient(pkg, name):
    from gespmm_amd import _lib, spmm

    c = CASES[name]
    _need_memory(c)
    t0 = time.perf_counter()
    R, M, K, N_out = (c[k] for k in ("R", "M", "K", "N_out"))
    dtype = TD[c["dt"]]
    rp, ci, val, scale, X = _operands(c)
    go = torch.zeros((M, N_out), dtype=dtype, device="cuda")
    for i in ll.grad_rows(c):
        go[i] = ll.grad_at(i, torch.arange(N_out, device="cuda")).to(dtype)
    want2 = ll.ref_wgrad2(c)
    blocks = (M + 63) // 64
    for chunks in (None, 1, blocks if R * N_out * K * blocks <= ll.LIM else 7):
        C = _lib.spmm_relational_wgrad_chunks(R, M, K, N_out) if chunks is None else chunks
        out = torch.full((R, N_out, K), float("nan"), dtype=dtype, device="cuda")
        ws = torch.full((C * R * N_out * K,), float("nan"), device="cuda")
        assert ll.route(c, chunks=C) == 1 and spmm.x16_align(X, go, out, ws) == 16
        got = spmm.csr_spmm_relational_weight_grad(rp, ci, val, X, go, R, row_scale=scale, chunks=chunks, workspace=ws, out=out)
        assert _equal2(got, want2), (name, chunks, band.first_difference(got.double().cpu() * 2, want2.double()))
    torch.cuda.synchronize()
    print("%s: M=%d Kn=%d K=%d N_out=%d R=%d nnz=%d: %.1f s" % (name, M, c["Kn"], K, N_out, R, c["nnz"], time.perf_counter() - t0))
