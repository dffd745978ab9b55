"""SDDMM, host side only (no GPU): the routing decision gespmm_describe_sddmm reports (the function launch_sddmm itself runs,
csrc/select.cpp: resolve_sddmm) against answers written out by hand from the documented rules; the lane-order oracle against
the float64 oracle; and the return codes the entry points give before any pointer is touched."""
import ctypes

import numpy as np
import pytest

EINVAL, EALIGN, ERANGE = -1, -2, -3
MAX_NNZ = 0x7FFFFFFF - 4096  # include/gespmm.h: the kernels count edges in 32 bits, a wavefront's span past the end included
WIDTHS = (0, 1, 3, 4, 16, 17, 41, 256, 257, 512, 513, 602, 1433)
VW = [(V, W) for V in (1, 2, 4) for W in (4, 8, 16, 32, 64)]  # every pair the router can answer


def _d(_lib, csr, M, nnz, N, a1=16, a2=16, cap=False):
    r = _lib.describe_sddmm(csr, M, nnz, N, a1, a2, cap)
    return " ".join("%s=%s" % kv for kv in r.items())


def test_router_vector_width_and_lanes(pkg):
    """V: the widest of 4, 2, 1 that divides N and whose 4 V bytes divide both addresses. W: the smallest power of two in 4..64
    with 8 W >= N (a lane covers 2 x 4, 4 x 2 or 8 x 1 floats). COO form: 4 edges per lane group, 64 / W groups."""
    from gespmm_amd import _lib

    want = {0: (4, 4), 1: (1, 4), 2: (2, 4), 3: (1, 4), 4: (4, 4), 8: (4, 4), 12: (4, 4), 16: (4, 4), 17: (1, 4), 31: (1, 4), 32: (4, 4),
            33: (1, 8), 64: (4, 8), 65: (1, 16), 128: (4, 16), 129: (1, 32), 130: (2, 32), 255: (1, 32), 256: (4, 32), 257: (1, 64),
            258: (2, 64), 260: (4, 64), 511: (1, 64), 512: (4, 64), 513: (1, 64), 514: (2, 64), 516: (4, 64), 602: (2, 64),
            1024: (4, 64), 1433: (1, 64), 2048: (4, 64), 3703: (1, 64)}
    for N, (V, W) in want.items():
        assert _d(_lib, False, 0, 1000, N) == "form=coo-edge V=%d W=%d epw=%d" % (V, W, 4 * 64 // W), N
    # alignment: N % 4 == 0, addresses on 16 / 8 / 4 bytes (the narrower operand decides); W does not move (8 W >= N whatever V)
    for a1, a2, V in ((16, 16, 4), (8, 16, 2), (16, 8, 2), (8, 8, 2), (4, 16, 1), (16, 4, 1), (4, 8, 1), (4, 4, 1), (32, 64, 4), (64, 8, 2)):
        assert _d(_lib, False, 0, 1000, 128, a1, a2) == "form=coo-edge V=%d W=16 epw=16" % V, (a1, a2)
        assert _d(_lib, True, 1000, 5000, 1024, a1, a2) == "form=csr-edge V=%d W=64 epw=16" % V, (a1, a2)
    assert _d(_lib, False, 0, 1000, 130, 4, 16) == "form=coo-edge V=1 W=32 epw=8"  # N % 4 != 0 and one float of alignment
    assert _d(_lib, False, 0, 0, 128) == "form=none"
    assert _d(_lib, True, 10, 0, 128) == "form=none"


def test_router_csr_edge_window_sizes(pkg):
    """CSR edge-parallel form (mean degree < 64): 256 edges per wavefront from 2^22 edges, 64 from 2^20, below that what the
    COO form takes (4 x 64 / W) but at least 16."""
    from gespmm_amd import _lib

    M = 1000000
    for nnz, N, epw in ((1048575, 128, 16), (1048576, 128, 64), (4194303, 128, 64), (4194304, 128, 256),
                        (1048575, 16, 64), (1048575, 64, 32), (1048575, 602, 16), (1048576, 602, 64), (4194304, 3, 256),
                        (50000, 3, 64), (50000, 33, 32), (50000, 65, 16), (50000, 1433, 16)):
        got = _lib.describe_sddmm(True, M, nnz, N)
        assert (got["form"], got["epw"]) == ("csr-edge", epw), (nnz, N, got)
    assert _d(_lib, True, 0, 5000, 128) == "form=csr-edge V=4 W=16 epw=16"  # M = 0 is not a mean degree


def test_router_row_walk_and_blocked_thresholds(pkg):
    """Row-walking from mean degree 64 (integer division nnz / M). Cache-blocked on top of that when N * 4 >= 256, the slab
    count ceil(M / slab_rows), slab_rows = max(64, 6 MiB / (4 N)), lies in 4..4096, a row gathers >= 4608 bytes per slab
    (mean degree * 4 N >= 4608 * nslab), and the stream is not capturing."""
    from gespmm_amd import _lib

    # mean degree 63 / 64 (one slab: M far below 12288 rows of 512 bytes)
    assert _d(_lib, True, 1000, 63999, 128) == "form=csr-edge V=4 W=16 epw=16"
    assert _d(_lib, True, 1000, 64000, 128) == "form=row-walk V=4 W=16"
    # nslab 3 / 4: N = 128 -> slab_rows = 6291456 / 512 = 12288; 3 * 12288 = 36864
    assert _d(_lib, True, 36864, 64 * 36864, 128) == "form=row-walk V=4 W=16"
    assert _d(_lib, True, 36865, 64 * 36865, 128) == "form=blocked V=4 W=16 nslab=4 slab_rows=12288"
    # nslab 4096 / 4097: N = 24576 -> slab_rows = 6291456 / 98304 = 64 (the floor); 4096 * 64 = 262144 rows;
    # 192 * 98304 = 18874368 = 4608 * 4096, so degree 192 passes the bytes-per-slab gate exactly
    assert _d(_lib, True, 262144, 192 * 262144, 24576) == "form=blocked V=4 W=64 nslab=4096 slab_rows=64"
    assert _d(_lib, True, 262145, 192 * 262145, 24576) == "form=row-walk V=4 W=64"
    assert _d(_lib, True, 262144, 192 * 262144 - 1, 24576) == "form=row-walk V=4 W=64"  # degree 191: one side of the gate
    # N * 4 at 252 / 256, M = 100000, degree 128: N = 63 -> 24966 rows a slab, 5 slabs, 128 * 252 >= 4608 * 5, but rows too short
    assert _d(_lib, True, 100000, 12800000, 63) == "form=row-walk V=1 W=8"
    assert _d(_lib, True, 100000, 12800000, 64) == "form=blocked V=4 W=8 nslab=5 slab_rows=24576"
    # the bytes-per-slab gate, both sides: N = 64, M = 80000 -> 4 slabs, 256 * degree >= 18432 <=> degree >= 72
    assert _d(_lib, True, 80000, 71 * 80000, 64) == "form=row-walk V=4 W=8"
    assert _d(_lib, True, 80000, 72 * 80000 - 1, 64) == "form=row-walk V=4 W=8"
    assert _d(_lib, True, 80000, 72 * 80000, 64) == "form=blocked V=4 W=8 nslab=4 slab_rows=24576"
    # capturing on / off (the blocked form allocates), and V follows the alignment in every form
    assert _d(_lib, True, 15000, 64 * 15000, 513) == "form=blocked V=1 W=64 nslab=5 slab_rows=3066"
    assert _d(_lib, True, 15000, 64 * 15000, 513, cap=True) == "form=row-walk V=1 W=64"
    assert _d(_lib, True, 36865, 64 * 36865, 128, cap=True) == "form=row-walk V=4 W=16"
    assert _d(_lib, True, 36865, 64 * 36865, 128, 8, 16) == "form=blocked V=2 W=16 nslab=4 slab_rows=12288"
    assert _d(_lib, True, 36865, 64 * 36865, 128, 16, 4, cap=True) == "form=row-walk V=1 W=16"
    assert _d(_lib, True, 1000, 63999, 128, cap=True) == "form=csr-edge V=4 W=16 epw=16"  # capture changes nothing else
    # the COO form never looks at M or the degree
    assert _d(_lib, False, 36865, 64 * 36865, 128) == "form=coo-edge V=4 W=16 epw=16"
    # N = 0: zeros are written by the narrowest edge-parallel launch (or the row walk)
    assert _d(_lib, True, 1000, 5000, 0) == "form=csr-edge V=4 W=4 epw=64"
    assert _d(_lib, True, 1000, 64000, 0) == "form=row-walk V=4 W=4"


def test_describe_sddmm_arguments(pkg):
    from gespmm_amd import _lib

    f = _lib.lib.gespmm_describe_sddmm
    buf = ctypes.create_string_buffer(64)
    assert f(1, 10, 20, 8, 16, 16, 0, None, 64) == EINVAL
    assert f(1, 10, 20, 8, 16, 16, 0, buf, 0) == EINVAL
    assert f(1, -1, 20, 8, 16, 16, 0, buf, 64) == EINVAL
    assert f(1, 10, -1, 8, 16, 16, 0, buf, 64) == EINVAL
    assert f(1, 10, 20, -8, 16, 16, 0, buf, 64) == EINVAL
    assert f(1, 10, 20, 8, 2, 16, 0, buf, 64) == EINVAL   # floats are 4-byte aligned at least
    assert f(1, 10, 20, 8, 16, 12, 0, buf, 64) == EINVAL  # not a power of two
    assert f(1, 10, MAX_NNZ + 1, 8, 16, 16, 0, buf, 64) == ERANGE
    small = ctypes.create_string_buffer(8)
    assert f(0, 0, 20, 8, 16, 16, 0, small, 8) == 7 and small.value == b"form=co"  # truncated, NUL-terminated


def test_sddmm_return_codes_need_no_gpu(pkg):
    """Range and alignment are checked before any pointer is touched. nnz: the kernels form (block * 4 + wave) * per_wave and
    that plus per_wave (<= 256) in 32 bits for every wavefront of the last workgroup, so the entry points take 2^31 - 1 - 4096
    edges at the most (the margin the SpMM entry points keep) and answer GESPMM_ERANGE beyond."""
    from gespmm_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 2)
    coo, csr, plan = lib.gespmm_sddmm_coo_f32, lib.gespmm_sddmm_csr_f32, lib.gespmm_plan_sddmm_f32
    # the largest accepted nnz passes the range check (and stops at the null pointer behind it); one more does not
    assert coo(None, p, p, p, p, MAX_NNZ, 4, None) == EINVAL
    assert csr(None, p, p, p, p, 16, MAX_NNZ, 4, None) == EINVAL
    for nnz in (MAX_NNZ + 1, 0x7FFFFFFF - 256, 0x7FFFFFFF, 1 << 31, 1 << 40):
        assert coo(None, p, p, p, p, nnz, 4, None) == ERANGE, nnz
        assert csr(None, p, p, p, p, 16, nnz, 4, None) == ERANGE, nnz
        assert coo(p, p, p, p, p, nnz, 4, None) == ERANGE, nnz
    assert coo(p, p, p, p, p, 8, 1 << 30, None) == ERANGE and csr(p, p, p, p, p, 1 << 31, 8, 4, None) == ERANGE
    assert coo(p, p, p, p, p, -1, 4, None) == EINVAL and csr(p, p, p, p, p, 4, 8, -4, None) == EINVAL
    for bad in range(5):
        args = [p] * 5
        args[bad] = odd
        assert coo(*args, 8, 4, None) == EALIGN and csr(*args, 4, 8, 4, None) == EALIGN, bad
    assert coo(p, p, None, p, p, 8, 4, None) == EINVAL and csr(p, p, p, None, p, 4, 8, 4, None) == EINVAL
    assert coo(p, p, p, p, None, 8, 0, None) == EINVAL  # N == 0 still writes nnz zeros: out is needed, D1 / D2 are not
    assert coo(odd, odd, odd, odd, odd, 0, 4, None) == 0 and csr(None, None, None, None, None, 4, 0, 4, None) == 0
    # the plan entry point without a plan (its range and alignment checks need one: tests/test_gpu_sddmm_forms.py::test_plan_routes)
    assert plan(None, p, p, p, -1, None) == EINVAL
    assert plan(None, p, p, p, 1 << 30, None) == EINVAL
    assert plan(None, p, p, p, 4, None) == EINVAL
    assert lib.gespmm_plan_sddmm_route(None, 128) == EINVAL


def _int_operands(rng, rows, cols, N):
    # small integers: every product and every partial sum is an integer below 2^24 — exact in any order
    return (rng.randint(-8, 9, size=(rows, N)).astype(np.float32), rng.randint(-8, 9, size=(cols, N)).astype(np.float32))


@pytest.mark.parametrize("N", WIDTHS)
def test_lane_oracle_against_float64(oracle, N):
    rng = np.random.RandomState(1000 + N)
    M, K, nnz = 37, 53, 400
    rows = rng.randint(0, M, size=nnz).astype(np.int32)
    cols = rng.randint(0, K, size=nnz).astype(np.int32)
    D1 = (rng.rand(M, N).astype(np.float32) - np.float32(0.5)) * np.float32(4)
    D2 = oracle.hash_B(K, N, seed=N + 3)
    ref, scale = oracle.sddmm(rows, cols, D1, D2, csr=False)
    I1, I2 = _int_operands(rng, M, K, N)
    iref, _ = oracle.sddmm(rows, cols, I1, I2, csr=False)
    for V, W in VW:
        got = oracle.sddmm_lanes(V, W, rows, cols, D1, D2)
        assert got.shape == (nnz,)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 1e-4 * np.maximum(np.abs(ref), scale)), (V, W, N)
        exact = oracle.sddmm_lanes(V, W, rows, cols, I1, I2)
        assert np.array_equal(exact, iref), (V, W, N)  # (integers: exact whether or not one slice covers the row, W V >= N included)


def test_lane_oracle_is_the_stated_order(oracle):
    """The order itself, on inputs where it shows: one large element and many small ones that a different chain or tree
    would absorb differently. Expected values are built here with numpy float32 steps, element by element."""
    f = np.float32
    x = np.array([[2 ** 24, 3, 1, 1, 1, 1, 1, 1]], dtype=np.float32)  # (2^24 + 1 and 2^24 + 3 are ties: to 2^24 and 2^24 + 4)
    y = np.ones((1, 8), dtype=np.float32)  # products are exact: fmaf(a, 1, acc) = fl(a + acc)

    def chain(idx):
        acc = f(0)
        for j in idx:
            acc = f(acc + x[0, j])
        return acc

    def tree4(p):
        return f(f(p[0] + p[2]) + f(p[1] + p[3]))  # masks 2, then 1, as lane 0 sees them

    # V = 1, W = 4: lane l takes x[l], x[l + 4]
    assert oracle.sddmm_lanes(1, 4, [0], [0], x, y)[0] == tree4([chain((l, l + 4)) for l in range(4)]) == f(2 ** 24 + 8)
    # V = 2, W = 4: lane l takes x[2l], x[2l + 1] in one chain
    assert oracle.sddmm_lanes(2, 4, [0], [0], x, y)[0] == tree4([chain((2 * l, 2 * l + 1)) for l in range(4)]) == f(2 ** 24 + 10)
    # V = 4, W = 4: lanes 0 and 1 take four elements each, lanes 2 and 3 nothing
    assert oracle.sddmm_lanes(4, 4, [0], [0], x, y)[0] == tree4([chain(range(0, 4)), chain(range(4, 8)), f(0), f(0)]) == f(2 ** 24 + 8)
    assert chain(range(8)) == f(2 ** 24 + 4)  # (what one sequential float32 chain gives)
    # W = 8 at V = 1: one element per lane, three butterfly levels (masks 4, 2, 1)
    q = [f(x[0, l] + x[0, l ^ 4]) for l in range(8)]
    q = [f(q[l] + q[l ^ 2]) for l in range(8)]
    assert oracle.sddmm_lanes(1, 8, [0], [0], x, y)[0] == f(q[0] + q[1])
    # the multiply is fused: -1 + (1 + 2^-12)^2 keeps its 2^-24 term only if the product is not rounded first
    a = np.array([[1.0, 1 + 2.0 ** -12]], dtype=np.float32)
    b = np.array([[-1.0, 1 + 2.0 ** -12]], dtype=np.float32)
    assert oracle.sddmm_lanes(2, 4, [0], [0], a, b)[0] == f(2.0 ** -11 + 2.0 ** -24)  # one chain: fma(a1, b1, -1)
    assert oracle.sddmm_lanes(1, 4, [0], [0], a, b)[0] == f(2.0 ** -11)  # two lanes: fl(a1 b1) = 1 + 2^-11 (a tie), then the add
    with pytest.raises(ValueError):
        oracle.sddmm_lanes(3, 4, [0], [0], a, b)
