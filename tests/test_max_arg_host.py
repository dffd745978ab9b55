"""The max reducer with argmax and its gradient, host side only: exported symbols, both return-code ladders through ctypes with
fabricated addresses (every call returns from the checks: nothing is dereferenced, no device is needed), the lane-geometry table of
gespmm_max_arg_route, and the host restatement (tests/max_arg_ref.py) on a hand-written case."""
import ctypes

import numpy as np
import pytest

from max_arg_ref import max_arg_forward, max_backward, tied_words, transpose

EINVAL, EALIGN, ERANGE = -1, -2, -3
I31 = 0x7FFFFFFF
MAX_M, MAX_K, MAX_N, MAX_NNZ = I31 - 64, I31, I31 // 4, I31 - 4096
NAN = float("nan")

FWD = dict(Prowptr=0x1000, Pcolind=0x2000, PB=0x4000, PC=0x5000, Parg=0x6000, M=4, K=4, N=8, nnz=5, empty_value=-10000.0)
BWD = dict(Pcolptr=0x1000, Prowind=0x2000, Porder=0x3000, Parg=0x4000, Pgrad_out=0x5000, Pgrad_B=0x6000, M=4, K=4, N=8, nnz=5)
ENTRIES = {"gespmm_csr_spmm_max_arg_f32": FWD, "gespmm_csr_spmm_max_backward_f32": BWD}


def _call(name, **override):
    from gespmm_amd import _lib

    args = dict(ENTRIES[name])
    for k in override:
        assert k in args, (name, k)
    args.update(override)
    values = [(ctypes.c_void_p(v) if v is not None else None) if k.startswith("P") else v for k, v in args.items()]
    return getattr(_lib.lib, name)(*values, None)


def _nulls(name):
    return {k: None for k in ENTRIES[name] if k.startswith("P")}


def test_symbols_and_version(pkg):
    from gespmm_amd import _lib

    for name in ("gespmm_csr_spmm_max_arg_f32", "gespmm_csr_spmm_max_backward_f32", "gespmm_max_arg_route"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib, name)
    assert _lib.lib.gespmm_version().decode().startswith("gespmm 0.5 ")
    import gespmm_amd

    assert hasattr(gespmm_amd, "SAGEConv") and hasattr(gespmm_amd, "SpmmMaxFunction")
    assert callable(gespmm_amd.spmm.csr_spmm_max_arg) and callable(gespmm_amd.spmm.csr_spmm_max_backward)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_size_rungs(pkg, name):
    for bad in (dict(M=-1), dict(K=-1), dict(N=-1), dict(nnz=-1), dict(M=-(1 << 40))):
        assert _call(name, **bad) == EINVAL, bad
    for past in (dict(M=MAX_M + 1), dict(K=MAX_K + 1), dict(N=MAX_N + 1), dict(nnz=MAX_NNZ + 1), dict(M=1 << 40)):
        assert _call(name, **past) == ERANGE, past
    # what makes no sense is reported before what does not fit
    assert _call(name, M=-1, K=MAX_K + 1) == EINVAL
    # the kernels' 32-bit byte offsets, for the gathered operand and for the result alike: no allocation, no second route
    assert _call(name, K=1 << 20, N=1 << 10) == ERANGE
    assert _call(name, M=1 << 20, N=1 << 10) == ERANGE
    assert _call(name, M=1 << 22, K=1, N=256) == ERANGE
    # one word below the limit the sizes pass: the NULL is what is reported
    result = "PC" if name.endswith("arg_f32") else "Pgrad_B"
    assert _call(name, K=(1 << 20) - 1, N=1 << 10, **{result: None}) == EINVAL
    assert _call(name, M=(1 << 20) - 1, N=1 << 10, **{result: None}) == EINVAL


def test_forward_ladder(pkg):
    name = "gespmm_csr_spmm_max_arg_f32"
    # a NaN empty_value is senseless: before ERANGE, before "nothing to do"
    assert _call(name, empty_value=NAN) == EINVAL
    assert _call(name, empty_value=NAN, K=MAX_K + 1) == EINVAL
    assert _call(name, empty_value=NAN, M=0, **_nulls(name)) == EINVAL
    # nothing to do: legal whatever the pointers are
    assert _call(name, M=0, **_nulls(name)) == 0
    assert _call(name, N=0, **_nulls(name)) == 0
    # required pointers
    for p in ("Prowptr", "Pcolind", "PB", "PC", "Parg"):
        assert _call(name, **{p: None}) == EINVAL, p
    # NULL before alignment; 4 bytes is all that is asked of an address
    assert _call(name, PC=None, PB=0x4002) == EINVAL
    for p in ("Prowptr", "Pcolind", "PB", "PC", "Parg"):
        assert _call(name, **{p: FWD[p] + 2}) == EALIGN, p
    # nnz == 0: colind and B may be NULL (the misaligned result is what is reported, which comes after the NULL check)
    assert _call(name, nnz=0, Pcolind=None, PB=None, Parg=0x6002) == EALIGN
    assert _call(name, nnz=0, Pcolind=None, PB=None, PC=None) == EINVAL
    # overlap: C or arg inside B (B is K N 4 = 128 bytes), B inside C, C on arg — after alignment
    assert _call(name, PC=0x4000 + 4) == EINVAL
    assert _call(name, Parg=0x4000 + 124) == EINVAL
    assert _call(name, PB=0x5000 + 64) == EINVAL
    assert _call(name, Parg=0x5000 + 8) == EINVAL
    assert _call(name, PC=0x4002) == EALIGN


def test_backward_ladder(pkg):
    name = "gespmm_csr_spmm_max_backward_f32"
    # nothing to do is decided on the TRANSPOSED sizes: no column or no width
    assert _call(name, K=0, **_nulls(name)) == 0
    assert _call(name, N=0, **_nulls(name)) == 0
    assert _call(name, M=0, Pgrad_B=None) == EINVAL  # (no rows: grad_B is still written, +0)
    for p in ("Pcolptr", "Prowind", "Porder", "Parg", "Pgrad_out", "Pgrad_B"):
        assert _call(name, **{p: None}) == EINVAL, p
    assert _call(name, Pgrad_B=None, Parg=0x4002) == EINVAL
    for p in ("Pcolptr", "Prowind", "Porder", "Parg", "Pgrad_out", "Pgrad_B"):
        assert _call(name, **{p: BWD[p] + 2}) == EALIGN, p
    assert _call(name, nnz=0, Prowind=None, Porder=None, Parg=None, Pgrad_out=None, Pgrad_B=0x6002) == EALIGN
    assert _call(name, nnz=0, Prowind=None, Porder=None, Parg=None, Pgrad_out=None, Pgrad_B=None) == EINVAL
    # overlap: grad_B on grad_out or on arg (each M N 4 = 128 bytes)
    assert _call(name, Pgrad_B=0x5000 + 4) == EINVAL
    assert _call(name, Pgrad_B=0x4000 + 124) == EINVAL
    assert _call(name, Pgrad_out=0x6000 + 64) == EINVAL


# (V, S, W) by width and by the alignment of the dense operands, for a graph of 300 rows: one lane per column up to N = 64 (W the power of
# two that covers N, at least 4); beyond, the widest vector N and the alignment allow, two strips where that vector is narrower than 4.
ROUTES = {
    1: ((1, 1, 4),) * 3, 3: ((1, 1, 4),) * 3, 4: ((1, 1, 4),) * 3, 20: ((1, 1, 32),) * 3, 47: ((1, 1, 64),) * 3, 64: ((1, 1, 64),) * 3,
    128: ((1, 2, 64), (2, 1, 64), (4, 1, 32)),
    130: ((1, 2, 64), (2, 2, 64), (2, 2, 64)),
    256: ((1, 2, 64), (2, 2, 64), (4, 1, 64)),
    260: ((1, 2, 64), (2, 2, 64), (4, 1, 64)),
    602: ((1, 2, 64), (2, 2, 64), (2, 2, 64)),
}


def test_route_table(pkg):
    from gespmm_amd import _lib

    for N, want in ROUTES.items():
        for align, geo in zip((4, 8, 16), want):
            assert _lib.max_arg_route(300, 2500, N, align, align) == geo, (N, align)
            assert _lib.max_arg_route(300, 2500, N, align, 16) == geo and _lib.max_arg_route(300, 2500, N, 16, align) == geo, (N, align)
    assert _lib.max_arg_route(300, 2500, 8) == (1, 1, 8) and _lib.max_arg_route(300, 2500, 16) == (1, 1, 16)
    # two strips of four floats: one 512-column tile just above 256 columns, on graphs large enough to fill the chip with one tile
    assert _lib.max_arg_route(1 << 17, 1 << 19, 260) == (4, 2, 64)
    assert _lib.max_arg_route(1 << 17, 1 << 19, 260, 8, 16) == (2, 2, 64)
    assert _lib.max_arg_route(0, 0, 64) is None and _lib.max_arg_route(300, 2500, 0) is None
    for bad in ((-1, 0, 4, 16, 16), (4, -1, 4, 16, 16), (4, 4, -1, 16, 16), (4, 4, 4, 2, 16), (4, 4, 4, 16, 12)):
        with pytest.raises(_lib.GespmmError) as e:
            _lib.max_arg_route(*bad)
        assert e.value.code == EINVAL, bad
    with pytest.raises(_lib.GespmmError) as e:
        _lib.max_arg_route(MAX_M + 1, 4, 4)
    assert e.value.code == ERANGE


def test_restatement_on_a_hand_written_case():
    """Six rows over five nodes, three columns; column 0 carries the case, columns 1 and 2 vary it."""
    nz, pz = np.float32(-0.0), np.float32(0.0)
    B = np.array([[1.0, pz, -20000.0],   # node 0
                  [3.0, nz, -30000.0],   # node 1
                  [3.0, pz, NAN],        # node 2
                  [nz, 5.0, -10000.0],   # node 3
                  [pz, NAN, NAN]],       # node 4
                 dtype=np.float32)
    rows = [[0, 1, 2, 1],   # first of equal values: 3.0 at position 1, again at 2 and 3
            [3, 4],         # -0 then +0: -0 wins and keeps its sign
            [4, 3],         # +0 then -0: +0 stays; column 1: NaN first, then 5.0; column 2: NaN, then -10000 (== empty) -> nothing wins
            [0, 1],         # column 2: all below empty_value
            [],             # an empty row
            [2, 2]]         # a repeated (row, column) entry: the first position
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    colind = np.array([c for r in rows for c in r], dtype=np.int32)
    C, arg = max_arg_forward(rowptr, colind, B, -10000.0)
    E = np.float32(-10000.0)
    want_C = np.array([[3.0, pz, E], [nz, 5.0, E], [pz, 5.0, E], [3.0, pz, E], [E, E, E], [3.0, pz, E]], dtype=np.float32)
    want_arg = np.array([[1, 0, -1], [4, 4, -1], [6, 7, -1], [9, 8, -1], [-1, -1, -1], [10, 10, -1]], dtype=np.int32)
    assert np.array_equal(arg, want_arg), arg
    assert np.array_equal(C.view(np.uint32), want_C.view(np.uint32)), C  # bits: the sign of the winning zero
    assert np.signbit(C[1, 0]) and not np.signbit(C[2, 0]) and not np.signbit(C[0, 1])
    tied = tied_words(rowptr, colind, B, C, arg)
    assert tied[0, 0] and tied[1, 0] and tied[5, 0] and not tied[3, 0] and not tied[4, 0]
    # with empty_value = 0 nothing <= 0 wins: both zeros lose
    C0, arg0 = max_arg_forward(rowptr, colind, B, 0.0)
    assert arg0[1, 0] == -1 and C0[1, 0] == 0 and not np.signbit(C0[1, 0])

    # the gradient: every word of grad_out goes to the node of the position arg names, in CSC order
    colptr, rowind, order = transpose(rowptr, colind, 5)
    assert np.array_equal(colind[order], np.repeat(np.arange(5), np.diff(colptr)))
    grad_out = (np.arange(18, dtype=np.float32).reshape(6, 3) + 1) / 8
    grad_B = max_backward(colptr, rowind, order, arg, grad_out, 5)
    want = np.zeros((5, 3), dtype=np.float32)
    for r in range(6):
        for c in range(3):
            if arg[r, c] >= 0:
                want[colind[arg[r, c]], c] += grad_out[r, c]
    assert np.array_equal(grad_B, want)  # (multiples of 1/8: every order of these adds is exact)
    assert grad_B[:, 2].tolist() == [0.0] * 5 and not np.signbit(grad_B).any()
    assert np.isclose(grad_B.sum(dtype=np.float64), grad_out[arg >= 0].sum(dtype=np.float64))
