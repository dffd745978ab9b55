"""16-bit SDDMM, host side only (no GPU): what gespmm_describe_sddmm_x16 reports (resolve_sddmm at element size 2, the function
launch_sddmm_x16 itself runs) against answers written out by hand from the documented rules; the V = 8 lane order of the oracle's
C function against a numpy restatement, float64 and one hand-computed vector; the return codes of the new entry points before any
pointer is touched."""
import ctypes

import numpy as np
import pytest

EINVAL, EALIGN, ERANGE = -1, -2, -3
MAX_NNZ = 0x7FFFFFFF - 4096
F16, BF16 = 1, 2

# (V, W) at 16-byte aligned operands, by hand. V: widest of 8, 4, 2, 1 dividing N. A lane covers V * IT elements, IT = 2 / 4 / 8 / 8 for
# V = 8 / 4 / 2 / 1, i.e. 16, 16, 16, 8 elements; W = smallest power of two in 4..64 with W * that >= N.
VW16 = {0: (8, 4), 1: (1, 4), 2: (2, 4), 3: (1, 4), 4: (4, 4), 8: (8, 4), 12: (4, 4), 16: (8, 4), 24: (8, 4), 32: (8, 4), 33: (1, 8),
        36: (4, 4), 40: (8, 4), 64: (8, 4), 65: (1, 16), 72: (8, 8), 128: (8, 8), 130: (2, 16), 255: (1, 32), 256: (8, 16),
        258: (2, 32), 260: (4, 32), 511: (1, 64), 512: (8, 32), 513: (1, 64), 514: (2, 64), 602: (2, 64), 1024: (8, 64),
        1026: (2, 64), 1028: (4, 64), 1032: (8, 64), 2048: (8, 64)}


def _d(_lib, csr, M, nnz, N, a1=16, a2=16, cap=False, x16=True):
    r = _lib.describe_sddmm(csr, M, nnz, N, a1, a2, cap, x16=x16)
    return " ".join("%s=%s" % kv for kv in r.items())


def test_router_vector_width_and_lanes_x16(pkg):
    from gespmm_amd import _lib

    for N, (V, W) in VW16.items():
        assert _d(_lib, False, 0, 1000, N) == "form=coo-edge V=%d W=%d epw=%d" % (V, W, 4 * 64 // W), N
    # alignment, either operand: 2 V bytes must divide both addresses. N = 128: 16 elements per lane at V = 8, 4, 2 (W = 8), 8 at V = 1
    # (W = 16); N = 1024: W = 64 whatever V.
    for a1, a2, V in ((16, 16, 8), (8, 16, 4), (16, 8, 4), (8, 8, 4), (4, 16, 2), (16, 4, 2), (4, 8, 2), (4, 4, 2), (2, 16, 1), (16, 2, 1),
                      (2, 8, 1), (4, 2, 1), (2, 2, 1), (32, 64, 8), (64, 8, 4), (256, 2, 1)):
        assert _d(_lib, False, 0, 1000, 128, a1, a2) == "form=coo-edge V=%d W=%d epw=%d" % (V, 16 if V == 1 else 8, 16 if V == 1 else 32), (a1, a2)
        assert _d(_lib, True, 1000, 5000, 1024, a1, a2) == "form=csr-edge V=%d W=64 epw=16" % V, (a1, a2)
    assert _d(_lib, False, 0, 1000, 130, 2, 16) == "form=coo-edge V=1 W=32 epw=8"  # N % 4 != 0 and one element of alignment
    assert _d(_lib, False, 0, 1000, 36, 16, 4) == "form=coo-edge V=2 W=4 epw=64"
    assert _d(_lib, False, 0, 0, 128) == "form=none"
    assert _d(_lib, True, 10, 0, 128) == "form=none"


def test_router_csr_edge_window_sizes_x16(pkg):
    """epw keeps its rule: 256 from 2^22 edges, 64 from 2^20, below that the COO form's 4 x 64 / W but at least 16."""
    from gespmm_amd import _lib

    M = 1000000
    for nnz, N, epw in ((1048575, 128, 32), (1048576, 128, 64), (4194303, 128, 64), (4194304, 128, 256), (1048575, 16, 64),
                        (1048575, 256, 16), (1048575, 602, 16), (1048576, 602, 64), (4194304, 3, 256), (50000, 3, 64), (50000, 33, 32),
                        (50000, 65, 16), (50000, 1032, 16)):
        got = _lib.describe_sddmm(True, M, nnz, N, x16=True)
        assert (got["form"], got["epw"]) == ("csr-edge", epw), (nnz, N, got)
    assert _d(_lib, True, 0, 5000, 128) == "form=csr-edge V=8 W=8 epw=32"  # M = 0 is not a mean degree


def test_router_row_walk_and_blocked_thresholds_x16(pkg):
    """Row-walking from mean degree 64. Cache-blocked on top when 2 N >= 256, nslab = ceil(M / slab_rows) with
    slab_rows = max(64, 6 MiB / 2N) lies in 4..4096, mean degree * 2N >= 4608 * nslab, and the stream is not capturing."""
    from gespmm_amd import _lib

    assert _d(_lib, True, 1000, 63999, 128) == "form=csr-edge V=8 W=8 epw=32"
    assert _d(_lib, True, 1000, 64000, 128) == "form=row-walk V=8 W=8"
    # N = 128: 256 bytes a row, slab_rows = 6291456 / 256 = 24576; 3 * 24576 = 73728; 4 slabs need degree * 256 >= 18432 <=> degree >= 72
    assert _d(_lib, True, 73728, 72 * 73728, 128) == "form=row-walk V=8 W=8"
    assert _d(_lib, True, 73729, 72 * 73729, 128) == "form=blocked V=8 W=8 nslab=4 slab_rows=24576"
    assert _d(_lib, True, 73729, 72 * 73729 - 1, 128) == "form=row-walk V=8 W=8"  # degree 71
    assert _d(_lib, True, 73729, 64 * 73729, 128) == "form=row-walk V=8 W=8"
    # 2 N at 254 / 256 bytes, M = 100000 (5 slabs of 24576 at N = 128), degree 128
    assert _d(_lib, True, 100000, 12800000, 127) == "form=row-walk V=1 W=16"
    assert _d(_lib, True, 100000, 12800000, 128) == "form=blocked V=8 W=8 nslab=5 slab_rows=24576"
    # nslab 4096 / 4097: N = 49152 -> 98304 bytes a row, slab_rows = 64 (the floor); 192 * 98304 = 4608 * 4096 exactly
    assert _d(_lib, True, 262144, 192 * 262144, 49152) == "form=blocked V=8 W=64 nslab=4096 slab_rows=64"
    assert _d(_lib, True, 262145, 192 * 262145, 49152) == "form=row-walk V=8 W=64"
    assert _d(_lib, True, 262144, 192 * 262144 - 1, 49152) == "form=row-walk V=8 W=64"
    # the shapes the GPU tests use: N = 1024 -> slab_rows = 6291456 / 2048 = 3072; N = 513 -> 6291456 / 1026 = 6132
    assert _d(_lib, True, 9300, 70 * 9300, 1024) == "form=blocked V=8 W=64 nslab=4 slab_rows=3072"
    assert _d(_lib, True, 22000, 70 * 22000, 1024) == "form=blocked V=8 W=64 nslab=8 slab_rows=3072"
    assert _d(_lib, True, 19000, 70 * 19000, 513) == "form=blocked V=1 W=64 nslab=4 slab_rows=6132"
    # capturing on / off, and V follows the alignment in every form
    assert _d(_lib, True, 9300, 70 * 9300, 1024, cap=True) == "form=row-walk V=8 W=64"
    assert _d(_lib, True, 9300, 70 * 9300, 1024, 8, 16) == "form=blocked V=4 W=64 nslab=4 slab_rows=3072"
    assert _d(_lib, True, 9300, 70 * 9300, 1024, 16, 2, cap=True) == "form=row-walk V=1 W=64"
    assert _d(_lib, True, 1000, 63999, 128, cap=True) == "form=csr-edge V=8 W=8 epw=32"
    assert _d(_lib, False, 73729, 72 * 73729, 128) == "form=coo-edge V=8 W=8 epw=32"  # the COO form never looks at M
    assert _d(_lib, True, 1000, 5000, 0) == "form=csr-edge V=8 W=4 epw=64"
    assert _d(_lib, True, 1000, 64000, 0) == "form=row-walk V=8 W=4"


def test_fp32_describe_is_what_it_was(pkg):
    """The element-size argument at 4 bytes reproduces the fp32 answers (tests/test_sddmm_host.py holds the full table)."""
    from gespmm_amd import _lib

    assert _d(_lib, False, 0, 1000, 128, x16=False) == "form=coo-edge V=4 W=16 epw=16"
    assert _d(_lib, False, 0, 1000, 130, x16=False) == "form=coo-edge V=2 W=32 epw=8"
    assert _d(_lib, False, 0, 1000, 0, x16=False) == "form=coo-edge V=4 W=4 epw=64"
    assert _d(_lib, True, 36865, 64 * 36865, 128, x16=False) == "form=blocked V=4 W=16 nslab=4 slab_rows=12288"
    assert _d(_lib, True, 15000, 64 * 15000, 513, x16=False) == "form=blocked V=1 W=64 nslab=5 slab_rows=3066"
    assert _d(_lib, True, 100000, 12800000, 63, x16=False) == "form=row-walk V=1 W=8"
    assert _d(_lib, True, 1000, 63999, 128, 8, 16, x16=False) == "form=csr-edge V=2 W=16 epw=16"
    assert _lib.describe_sddmm(True, 1000, 5000, 1024) == _lib.describe_sddmm(True, 1000, 5000, 1024, x16=False)
    with pytest.raises(_lib.GespmmError):
        _lib.describe_sddmm(True, 1000, 5000, 128, 2, 16)  # fp32 operands are 4-byte aligned at least


def test_describe_sddmm_x16_arguments(pkg):
    from gespmm_amd import _lib

    f = _lib.lib.gespmm_describe_sddmm_x16
    buf = ctypes.create_string_buffer(64)
    assert f(1, 10, 20, 8, 16, 16, 0, None, 64) == EINVAL
    assert f(1, 10, 20, 8, 16, 16, 0, buf, 0) == EINVAL
    assert f(1, -1, 20, 8, 16, 16, 0, buf, 64) == EINVAL
    assert f(1, 10, -1, 8, 16, 16, 0, buf, 64) == EINVAL
    assert f(1, 10, 20, -8, 16, 16, 0, buf, 64) == EINVAL
    assert f(1, 10, 20, 8, 1, 16, 0, buf, 64) == EINVAL   # 16-bit elements are 2-byte aligned at least
    assert f(1, 10, 20, 8, 16, 0, 0, buf, 64) == EINVAL
    assert f(1, 10, 20, 8, 16, 12, 0, buf, 64) == EINVAL  # not a power of two
    assert f(1, 10, 20, 8, 2, 2, 0, buf, 64) == len(b"form=csr-edge V=1 W=4 epw=64") and buf.value == b"form=csr-edge V=1 W=4 epw=64"
    assert f(1, 10, MAX_NNZ + 1, 8, 16, 16, 0, buf, 64) == ERANGE
    assert f(1, 1 << 31, 20, 8, 16, 16, 0, buf, 64) == ERANGE
    small = ctypes.create_string_buffer(8)
    assert f(0, 0, 20, 8, 16, 16, 0, small, 8) == 7 and small.value == b"form=co"  # truncated, NUL-terminated


def test_sddmm_x16_return_codes_need_no_gpu(pkg):
    """The checks of the fp32 entry points in their order — sizes and dtype, range, nnz == 0, null pointers, alignment (D1 / D2 on
    2 bytes, the index arrays and out on 4) — all before any device work."""
    from gespmm_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    half = ctypes.c_void_p(p.value + 2)
    odd = ctypes.c_void_p(p.value + 1)
    coo, csr, plan = lib.gespmm_sddmm_coo_x16, lib.gespmm_sddmm_csr_x16, lib.gespmm_plan_sddmm_x16
    for dt in (F16, BF16):
        assert coo(None, p, p, p, p, dt, MAX_NNZ, 4, None) == EINVAL
        assert csr(None, p, p, p, p, dt, 16, MAX_NNZ, 4, None) == EINVAL
        for nnz in (MAX_NNZ + 1, 0x7FFFFFFF, 1 << 31, 1 << 40):
            assert coo(None, p, p, p, p, dt, nnz, 4, None) == ERANGE, nnz
            assert csr(None, p, p, p, p, dt, 16, nnz, 4, None) == ERANGE, nnz
            assert coo(p, p, p, p, p, dt, nnz, 4, None) == ERANGE, nnz
        assert coo(p, p, p, p, p, dt, 8, 1 << 30, None) == ERANGE and csr(p, p, p, p, p, dt, 1 << 31, 8, 4, None) == ERANGE
        assert coo(p, p, p, p, p, dt, -1, 4, None) == EINVAL and csr(p, p, p, p, p, dt, 4, 8, -4, None) == EINVAL
        for bad in range(5):
            args = [p] * 5
            args[bad] = odd  # one byte off: no operand is aligned
            assert coo(*args, dt, 8, 4, None) == EALIGN and csr(*args, dt, 4, 8, 4, None) == EALIGN, bad
        for bad in (0, 1, 4):  # two bytes off: fine for D1 and D2 (checked on the GPU), not for the index arrays and out
            args = [p] * 5
            args[bad] = half
            assert coo(*args, dt, 8, 4, None) == EALIGN and csr(*args, dt, 4, 8, 4, None) == EALIGN, bad
        assert coo(p, p, None, p, p, dt, 8, 4, None) == EINVAL and csr(p, p, p, None, p, dt, 4, 8, 4, None) == EINVAL
        assert coo(p, p, p, p, None, dt, 8, 0, None) == EINVAL  # N == 0 still writes nnz zeros: out is needed, D1 / D2 are not
        assert coo(odd, odd, odd, odd, odd, dt, 0, 4, None) == 0 and csr(None, None, None, None, None, dt, 4, 0, 4, None) == 0
        # the plan entry point without a plan
        assert plan(None, p, p, p, dt, -1, None) == EINVAL
        assert plan(None, p, p, p, dt, 1 << 30, None) == EINVAL
        assert plan(None, p, p, p, dt, 4, None) == EINVAL
    for dt in (0, 3, -1, 4):  # 0 is fp32 elsewhere in the library: not here
        assert coo(p, p, p, p, p, dt, 8, 4, None) == EINVAL and csr(p, p, p, p, p, dt, 4, 8, 4, None) == EINVAL, dt
        assert coo(p, p, p, p, p, dt, 0, 4, None) == EINVAL and coo(p, p, p, p, p, dt, MAX_NNZ + 1, 4, None) == EINVAL, dt
        assert plan(None, p, p, p, dt, 4, None) == EINVAL


# ------------------------------------------------------------------------------------------------------------- the V = 8 order

def _operands(rng, rows, N, dtype):
    """Values of the 16-bit type, as float32 (the widening is exact)."""
    a = (rng.rand(rows, N).astype(np.float32) - np.float32(0.5)) * np.float32(4)
    if dtype == F16:
        return a.astype(np.float16).astype(np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)  # bf16 by truncation: representable is all that matters


def _lanes(oracle, V, W, rows, cols, D1, D2):
    """oracle_sddmm_lanes itself: the C function takes any V (the Python wrapper admits 1, 2, 4 only)."""
    rows, cols = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    D1, D2 = np.ascontiguousarray(D1, dtype=np.float32), np.ascontiguousarray(D2, dtype=np.float32)
    out = np.full(max(cols.shape[0], 1), np.nan, dtype=np.float32)
    oracle.lib.oracle_sddmm_lanes(int(V), int(W), cols.shape[0], D1.shape[1], rows.ctypes.data, cols.ctypes.data, D1.ctypes.data,
                                  D2.ctypes.data, out.ctypes.data)
    return out[:cols.shape[0]]


def _numpy_lanes(V, W, rows, cols, D1, D2):
    """The formula in numpy float32 steps. The product of two fp16 or two bf16 numbers has at most 22 significant bits: exact in
    fp32, so fmaf(x, y, acc) is fl(acc + x y)."""
    N = D1.shape[1]
    p = D1[rows].astype(np.float32) * D2[cols].astype(np.float32)
    assert np.array_equal(p.astype(np.float64), D1[rows].astype(np.float64) * D2[cols].astype(np.float64))
    part = np.zeros((len(cols), W), dtype=np.float32)
    for l in range(W):
        for j0 in range(l * V, N, W * V):
            for j in range(j0, min(j0 + V, N)):
                part[:, l] = part[:, l] + p[:, j]
    m = W // 2
    while m >= 1:
        part = part + part[:, np.arange(W) ^ m]
        m //= 2
    return part[:, 0]


@pytest.mark.parametrize("dtype", (F16, BF16))
@pytest.mark.parametrize("N,V,W", ((128, 8, 8), (64, 8, 4), (41, 1, 8), (130, 2, 16), (1032, 8, 64), (36, 4, 4), (256, 8, 16), (8, 8, 4)))
def test_lane_oracle_at_sixteen_bit_geometry(oracle, dtype, N, V, W):
    rng = np.random.RandomState(3000 + N + dtype)
    M, K, nnz = 37, 53, 400
    rows = rng.randint(0, M, size=nnz).astype(np.int32)
    cols = rng.randint(0, K, size=nnz).astype(np.int32)
    D1, D2 = _operands(rng, M, N, dtype), _operands(rng, K, N, dtype)
    got = _lanes(oracle, V, W, rows, cols, D1, D2)
    assert np.array_equal(got.view(np.uint32), _numpy_lanes(V, W, rows, cols, D1, D2).view(np.uint32)), (N, V, W)
    ref, scale = oracle.sddmm(rows, cols, D1, D2, csr=False)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 1e-4 * np.maximum(np.abs(ref), scale)), (N, V, W)
    if V <= 4:  # the wrapper and the direct call are the same function
        assert np.array_equal(got.view(np.uint32), oracle.sddmm_lanes(V, W, rows, cols, D1, D2).view(np.uint32))
    # small integers: exact in any order
    I1 = rng.randint(-8, 9, size=(M, N)).astype(np.float32)
    I2 = rng.randint(-8, 9, size=(K, N)).astype(np.float32)
    assert np.array_equal(_lanes(oracle, V, W, rows, cols, I1, I2), oracle.sddmm(rows, cols, I1, I2, csr=False)[0])


def test_v8_order_by_hand(oracle):
    """One large element and small ones a different chain would absorb differently; every value is a bf16 number. V = 8, W = 4 on 16
    elements: lane 0 runs ONE chain over elements 0..7, lane 1 over 8..15, lanes 2 and 3 hold 0; then masks 2, 1."""
    f = np.float32
    x = np.array([[2 ** 24, 3] + [1] * 14], dtype=np.float32)
    y = np.ones((1, 16), dtype=np.float32)

    def chain(idx):
        acc = f(0)
        for j in idx:
            acc = f(acc + x[0, j])
        return acc

    def tree4(p):
        return f(f(p[0] + p[2]) + f(p[1] + p[3]))

    # lane 0: 2^24 + 3 is a tie -> 2^24 + 4; every further + 1 is a tie that goes back to 2^24 + 4. lane 1: 8.
    assert chain(range(8)) == f(2 ** 24 + 4) and chain(range(8, 16)) == f(8)
    assert _lanes(oracle, 8, 4, [0], [0], x, y)[0] == tree4([chain(range(0, 8)), chain(range(8, 16)), f(0), f(0)]) == f(2 ** 24 + 12)
    # the fp32 call's V = 4 on the same numbers: four chains of four, lanes 1..3 hold 4 each -> another result
    assert _lanes(oracle, 4, 4, [0], [0], x, y)[0] == tree4([chain(range(4 * l, 4 * l + 4)) for l in range(4)]) == f(2 ** 24 + 16)
    # V = 8, W = 8 on 128 elements: lane l takes [8l, 8l + 8) and [64 + 8l, 64 + 8l + 8) in one chain
    rng = np.random.RandomState(5)
    a, b = _operands(rng, 1, 128, BF16), _operands(rng, 1, 128, BF16)
    part = []
    for l in range(8):
        acc = f(0)
        for j in list(range(8 * l, 8 * l + 8)) + list(range(64 + 8 * l, 64 + 8 * l + 8)):
            acc = f(acc + f(a[0, j] * b[0, j]))
        part.append(acc)
    for m in (4, 2, 1):
        part = [f(part[l] + part[l ^ m]) for l in range(8)]
    assert _lanes(oracle, 8, 8, [0], [0], a, b)[0] == part[0]
