"""16-bit dense operands (fp16 / bf16), host side only: the four symbols exist, bad arguments come back as GESPMM_E* codes before any device
work, gespmm_x16_route answers a hand-written table, and the header's integer formula for the bf16 rounding is torch's ``.to(torch.bfloat16)``
(this pins the CONTRACT to torch; tests/test_gpu_x16.py pins the kernels to the contract)."""
import ctypes
import subprocess

import numpy as np
import torch

EINVAL, EALIGN = -1, -2
F16, BF16 = 1, 2
X16 = ("gespmm_csr_spmm_x16", "gespmm_plan_spmm_x16", "gespmm_x16_route", "gespmm_plan_x16_route")


def test_the_four_symbols_exist(pkg):
    from gespmm_amd import _lib

    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in X16:
        assert name in _lib.EXPORTS
        assert (" T %s\n" % name) in nm, name
        getattr(_lib.lib, name)
    assert (_lib.X16_F16, _lib.X16_BF16) == (F16, BF16)


def _stateless(_lib, rowptr=0x1000, colind=0x2000, val=None, B=0x3000, C=0x4000, dtype=BF16, M=4, K=4, N=8, nnz=5, variant=-1):
    p = lambda v: ctypes.c_void_p(v) if v is not None else None  # noqa: E731  (addresses are never dereferenced: the checks come first)
    return _lib.lib.gespmm_csr_spmm_x16(p(rowptr), p(colind), p(val), p(B), p(C), dtype, M, K, N, nnz, variant, None)


def test_bad_arguments_are_refused_without_a_device(pkg):
    from gespmm_amd import _lib

    for dtype in (0, 3, -1):
        assert _stateless(_lib, dtype=dtype) == EINVAL
    assert _stateless(_lib, B=None) == EINVAL
    assert _stateless(_lib, C=None) == EINVAL
    assert _stateless(_lib, rowptr=None) == EINVAL
    assert _stateless(_lib, colind=None) == EINVAL
    assert _stateless(_lib, M=-1) == EINVAL
    assert _stateless(_lib, N=-3) == EINVAL
    assert _stateless(_lib, K=-1) == EINVAL
    assert _stateless(_lib, nnz=-2) == EINVAL
    assert _stateless(_lib, variant=17) == EINVAL
    for name in ("B", "C"):
        assert _stateless(_lib, **{name: 0x5001}) == EALIGN, name  # 2-byte alignment is what 16-bit operands need ...
    assert _stateless(_lib, val=0x5002) == EALIGN  # ... and the fp32 values 4
    assert _stateless(_lib, rowptr=0x1002) == EALIGN
    # nothing to do: legal whatever the pointers are
    assert _stateless(_lib, M=0, B=None, C=None, rowptr=None, colind=None) == 0
    assert _stateless(_lib, N=0, B=None, C=None, rowptr=None, colind=None) == 0
    # the plan entry points
    lib = _lib.lib
    assert lib.gespmm_plan_spmm_x16(None, ctypes.c_void_p(0x3000), ctypes.c_void_p(0x4000), BF16, 8, None) == EINVAL
    assert lib.gespmm_plan_x16_route(None, 128, 16, 16) == EINVAL
    assert lib.gespmm_x16_route(-1, 4, 8, 5, -1, 16, 16) == EINVAL
    assert lib.gespmm_x16_route(4, 4, 8, 5, 17, 16, 16) == EINVAL


def test_route_table(pkg):
    """0 composition, 1 the 16-bit batch-stream kernel, 2 the 16-bit segmented-stream kernel."""
    from gespmm_amd import _lib

    route = _lib.lib.gespmm_x16_route
    M = K = 100000
    nnz = 5 * M
    for N in (1, 3, 41):  # odd widths: a row is not a whole number of words
        assert route(M, K, N, nnz, -1, 16, 16) == 0, N
    assert route(M, K, 128, nnz, -1, 16, 16) == 1
    assert route(M, K, 128, nnz, -1, 4, 4) == 1
    assert route(M, K, 128, nnz, -1, 16, 4) == 1
    assert route(M, K, 128, nnz, -1, 2, 16) == 0  # B only 2-byte aligned
    assert route(M, K, 128, nnz, -1, 16, 2) == 0  # C only 2-byte aligned
    # reddit-sized (mean degree 492): the fp32 route is cache-blocked, at the byte-equivalent width too
    buf = ctypes.create_string_buffer(300)
    for N in (128, 256):
        _lib.lib.gespmm_describe_launch(232965, 232965, N, 114615892, -1, None, buf, 300)
        assert b"slab-blocked" in buf.value, buf.value
        assert route(232965, 232965, N, 114615892, -1, 16, 16) == 0, N
    # K N 2 >= 2^32: 64-bit offsets
    assert (1 << 24) * 128 * 2 >= 1 << 32
    assert route(1 << 20, 1 << 24, 128, 1 << 22, -1, 16, 16) == 0
    assert route(1 << 20, (1 << 24) - 1024, 128, 1 << 22, -1, 16, 16) in (1, 2)  # just below
    # short rows (mean degree 3, 2^17 rows): the segmented-stream kernel
    assert route(1 << 17, 1 << 17, 128, 3 << 17, -1, 16, 16) == 2
    # the naive and the parallel-reduction variants have no 16-bit form
    assert route(M, K, 128, nnz, 0, 16, 16) == 0
    assert route(M, K, 16, 64 * M, 5, 16, 16) == 0


def _narrow_bf16_formula(u):
    """gespmm.h: narrow of a non-NaN with fp32 bits u is (u + 0x7fff + ((u >> 16) & 1)) >> 16."""
    u = u.astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def test_bf16_rounding_formula_is_torchs():
    rng = np.random.RandomState(16)
    u = rng.randint(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF,  # 1, ties both ways, neighbours
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F800000, 0xFF800000,  # largest finite -> inf, bf16 max, +-inf
                        0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x00800000, 0x807FFFFF],  # subnormals
                       dtype=np.uint32)
    u = np.concatenate([u, special])
    f = torch.from_numpy(u.view(np.int32)).view(torch.float32)
    finite_or_inf = ~torch.isnan(f)
    want = f.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = _narrow_bf16_formula(u)
    keep = finite_or_inf.numpy()
    assert keep.sum() > (1 << 20) - (1 << 14)
    assert np.array_equal(got[keep], want[keep])
    # NaN stays NaN (payload not pinned)
    assert torch.isnan(f[~finite_or_inf].to(torch.bfloat16)).all()
