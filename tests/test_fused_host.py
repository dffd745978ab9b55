"""The fused product's C entry points, host side only: the symbols exist, the version is at least the 0.4 they came with (0.5 since the SDDMM describe call), and bad arguments come back as
GESPMM_E* codes before any device work (so these run on a machine without a GPU)."""
import ctypes
import subprocess

EINVAL, EALIGN = -1, -2
FUSED = ("gespmm_csr_spmm_fused_f32", "gespmm_plan_spmm_fused_f32", "gespmm_plan_fused_route")


def test_the_three_symbols_exist(pkg):
    from gespmm_amd import _lib

    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in FUSED:
        assert name in _lib.EXPORTS
        assert (" T %s\n" % name) in nm, name
        getattr(_lib.lib, name)


def test_version_is_0_5(pkg):
    from gespmm_amd import _lib

    assert _lib.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


def _stateless(_lib, rowptr=0x1000, colind=0x2000, val=None, B=0x3000, cs=None, rs=None, bias=None, C=0x4000, M=4, K=4, N=8, nnz=5, variant=-1):
    p = lambda v: ctypes.c_void_p(v) if v is not None else None  # noqa: E731  (addresses are never dereferenced: the checks come first)
    return _lib.lib.gespmm_csr_spmm_fused_f32(p(rowptr), p(colind), p(val), p(B), p(cs), p(rs), p(bias), p(C), M, K, N, nnz, variant, None)


def test_bad_arguments_are_refused_without_a_device(pkg):
    from gespmm_amd import _lib

    assert _stateless(_lib, B=None, cs=0x5000) == EINVAL
    assert _stateless(_lib, C=None, rs=0x5000) == EINVAL
    assert _stateless(_lib, rowptr=None, bias=0x5000) == EINVAL
    assert _stateless(_lib, M=-1, cs=0x5000) == EINVAL
    assert _stateless(_lib, N=-3, cs=0x5000) == EINVAL
    assert _stateless(_lib, K=-1, cs=0x5000) == EINVAL
    assert _stateless(_lib, nnz=-2, cs=0x5000) == EINVAL
    assert _stateless(_lib, variant=17, cs=0x5000) == EINVAL
    for name in ("B", "C", "cs", "rs", "bias", "val"):
        assert _stateless(_lib, **{name: 0x5002}) == EALIGN, name
    # nothing to do: legal whatever the pointers are
    assert _stateless(_lib, M=0, B=None, C=None, rowptr=None, colind=None) == 0
    # the plan entry points
    lib = _lib.lib
    assert lib.gespmm_plan_spmm_fused_f32(None, ctypes.c_void_p(0x3000), None, None, None, ctypes.c_void_p(0x4000), 8, None) == EINVAL
    assert lib.gespmm_plan_fused_route(None, 128, 1, 1, 1) == EINVAL
