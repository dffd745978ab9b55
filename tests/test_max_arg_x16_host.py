"""The 16-bit max reducer with argmax and its gradient, host side only: exported symbols, both return-code ladders through ctypes with
fabricated addresses (a refused call returns from the checks; the accepted ones are made where no device is visible: nothing is
dereferenced, no device is needed), the lane-geometry table of
gespmm_max_arg_route_x16 against the fp32 table at the effective alignment, and the oracle — the fp32 restatement on the exactly
widened operand, narrowed once — on the hand-written case of tests/test_max_arg_host.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from max_arg_ref import max_arg_forward, max_backward, transpose
from test_max_arg_host import ROUTES

EINVAL, EALIGN, ERANGE = -1, -2, -3
I31 = 0x7FFFFFFF
MAX_M, MAX_K, MAX_N, MAX_NNZ = I31 - 64, I31, I31 // 4, I31 - 4096
NAN = float("nan")
F16, BF16 = 1, 2

# B is K N 2 = 64 bytes, C and grad_out M N 2 = 64 bytes, arg M N 4 = 128 bytes
FWD = dict(Prowptr=0x1000, Pcolind=0x2000, PB=0x4000, PC=0x5000, Parg=0x6000, M=4, K=4, N=8, nnz=5, empty_value=-10000.0, dtype=BF16)
BWD = dict(Pcolptr=0x1000, Prowind=0x2000, Porder=0x3000, Parg=0x4000, Pgrad_out=0x5000, Pgrad_B=0x6000, M=4, K=4, N=8, nnz=5, dtype=F16)
ENTRIES = {"gespmm_csr_spmm_max_arg_x16": FWD, "gespmm_csr_spmm_max_backward_x16": BWD}


def _call(name, **override):
    from gespmm_amd import _lib

    args = dict(ENTRIES[name])
    for k in override:
        assert k in args, (name, k)
    args.update(override)
    values = [(ctypes.c_void_p(v) if v is not None else None) if k.startswith("P") else v for k, v in args.items()]
    return getattr(_lib.lib, name)(*values, None)


# A call that passes every check goes on to launch its kernel — with these fabricated addresses. Such calls are made in a child process
# that sees NO device (it checks that itself before the first call, and makes none otherwise): the launch then fails in the runtime
# with a positive HIP code and nothing is dereferenced anywhere. The ladder's own codes are negative, so "accepted" is `rc >= 0`.
_CHILD = r"""
import ctypes, json, sys
lib_path, calls = sys.argv[1], json.loads(sys.argv[2])
lib = ctypes.CDLL(lib_path)
hip = ctypes.CDLL("libamdhip64.so")
n = ctypes.c_int(-1)
rc = hip.hipGetDeviceCount(ctypes.byref(n))
if rc == 0 and n.value > 0:
    print("a device is visible: no call is made")
    sys.exit(3)
out = []
for name, args in calls:
    values = []
    for k, v in args:
        if k.startswith("P"):
            values.append(ctypes.c_void_p(v))
        elif k == "empty_value":
            values.append(ctypes.c_float(v))
        elif k == "dtype":
            values.append(ctypes.c_int(v))
        else:
            values.append(ctypes.c_int64(v))
    f = getattr(lib, name)
    f.restype = ctypes.c_int
    out.append(f(*values, ctypes.c_void_p(None)))
print(json.dumps(out))
"""


def _accepted(calls):
    """Return codes of [(name, override)] calls that are expected to pass every check, made where no device is visible."""
    from gespmm_amd import _lib

    payload = []
    for name, override in calls:
        args = dict(ENTRIES[name])
        for k in override:
            assert k in args, (name, k)
        args.update(override)
        payload.append((name, list(args.items())))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, "-c", _CHILD, _lib.LIB_PATH, json.dumps(payload)], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    return json.loads(run.stdout.strip().splitlines()[-1])


def _nulls(name):
    return {k: None for k in ENTRIES[name] if k.startswith("P")}


def test_symbols_and_version(pkg):
    from gespmm_amd import _lib

    for name in ("gespmm_csr_spmm_max_arg_x16", "gespmm_csr_spmm_max_backward_x16", "gespmm_max_arg_route_x16"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib, name)
    assert _lib.lib.gespmm_version().decode().startswith("gespmm 0.5 ")
    import gespmm_amd

    assert callable(gespmm_amd.spmm.csr_spmm_max_arg_x16) and callable(gespmm_amd.spmm.csr_spmm_max_backward_x16)
    assert callable(_lib.max_arg_route_x16)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_dtype_and_size_rungs(pkg, name):
    for dtype in (0, 3):
        assert _call(name, dtype=dtype) == EINVAL, dtype
        assert _call(name, dtype=dtype, M=0, **_nulls(name)) == EINVAL, dtype
    for dtype in (F16, BF16):
        assert _call(name, dtype=dtype, N=0, **_nulls(name)) == 0, dtype
    for bad in (dict(M=-1), dict(K=-1), dict(N=-1), dict(nnz=-1), dict(M=-(1 << 40))):
        assert _call(name, **bad) == EINVAL, bad
    for past in (dict(M=MAX_M + 1), dict(K=MAX_K + 1), dict(N=MAX_N + 1), dict(nnz=MAX_NNZ + 1), dict(M=1 << 40)):
        assert _call(name, **past) == ERANGE, past
    assert _call(name, M=-1, K=MAX_K + 1) == EINVAL
    # the limits are the fp32 entries', unchanged: arg is the 4-byte array that sets them, in both directions
    assert _call(name, K=1 << 20, N=1 << 10) == ERANGE
    assert _call(name, M=1 << 20, N=1 << 10) == ERANGE
    assert _call(name, M=1 << 22, K=1, N=256) == ERANGE
    result = "PC" if name.endswith("arg_x16") else "Pgrad_B"
    assert _call(name, K=(1 << 20) - 1, N=1 << 10, **{result: None}) == EINVAL
    assert _call(name, M=(1 << 20) - 1, N=1 << 10, **{result: None}) == EINVAL


def test_forward_ladder(pkg):
    name = "gespmm_csr_spmm_max_arg_x16"
    assert _call(name, empty_value=NAN) == EINVAL
    assert _call(name, empty_value=NAN, K=MAX_K + 1) == EINVAL
    assert _call(name, empty_value=NAN, M=0, **_nulls(name)) == EINVAL
    assert _call(name, M=0, **_nulls(name)) == 0
    assert _call(name, N=0, **_nulls(name)) == 0
    for p in ("Prowptr", "Pcolind", "PB", "PC", "Parg"):
        assert _call(name, **{p: None}) == EINVAL, p
    # NULL before alignment
    assert _call(name, PC=None, PB=0x4001) == EINVAL
    # an odd address of a 16-bit array is misaligned, + 2 is not; index arrays and arg need 4
    for p in ("PB", "PC"):
        assert _call(name, **{p: FWD[p] + 1}) == EALIGN, p
        assert _call(name, Parg=0x5000 + 8, **{p: FWD[p] + 1}) == EALIGN, p  # (alignment before overlap)
        assert _call(name, Parg=0x5000 + 8, **{p: FWD[p] + 2}) == EINVAL, p  # + 2 is aligned: the overlap is what is reported
    for p in ("Prowptr", "Pcolind", "Parg"):
        assert _call(name, **{p: FWD[p] + 2}) == EALIGN, p
    assert _call(name, nnz=0, Pcolind=None, PB=None, Parg=0x6002) == EALIGN
    assert _call(name, nnz=0, Pcolind=None, PB=None, PC=0x5001) == EALIGN
    assert _call(name, nnz=0, Pcolind=None, PB=None, PC=None) == EINVAL
    # overlap, sized in 2-byte elements: B is 64 bytes, C 64, arg 128
    assert _call(name, PC=0x4000 + 4) == EINVAL
    assert _call(name, PC=0x4000 + 62) == EINVAL
    assert _call(name, Parg=0x4000 + 60) == EINVAL
    assert _call(name, PB=0x5000 + 32) == EINVAL
    assert _call(name, Parg=0x5000 + 8) == EINVAL
    assert _call(name, PC=0x6000 + 124) == EINVAL  # inside arg's M N 4 bytes
    assert _call(name, PC=0x4001) == EALIGN
    # accepted: a 2-byte aligned 16-bit array; C or arg just past the K N 2 bytes of B, B just past the M N 2 bytes of C, C just past
    # the M N 4 bytes of arg (in 4-byte elements the first three would overlap)
    accepted = [dict(PB=0x4002), dict(PC=0x5002), dict(PC=0x4000 + 64), dict(Parg=0x4000 + 64), dict(PB=0x5000 + 64), dict(PC=0x6000 + 128),
                dict(dtype=F16)]
    codes = _accepted([(name, o) for o in accepted])
    assert all(rc >= 0 for rc in codes), list(zip(accepted, codes))


def test_backward_ladder(pkg):
    name = "gespmm_csr_spmm_max_backward_x16"
    assert _call(name, K=0, **_nulls(name)) == 0
    assert _call(name, N=0, **_nulls(name)) == 0
    assert _call(name, M=0, Pgrad_B=None) == EINVAL
    for p in ("Pcolptr", "Prowind", "Porder", "Parg", "Pgrad_out", "Pgrad_B"):
        assert _call(name, **{p: None}) == EINVAL, p
    assert _call(name, Pgrad_B=None, Parg=0x4002) == EINVAL
    for p in ("Pgrad_out", "Pgrad_B"):
        assert _call(name, **{p: BWD[p] + 1}) == EALIGN, p
    for p in ("Pcolptr", "Prowind", "Porder", "Parg"):
        assert _call(name, **{p: BWD[p] + 2}) == EALIGN, p
    assert _call(name, nnz=0, Prowind=None, Porder=None, Parg=None, Pgrad_out=None, Pgrad_B=0x6001) == EALIGN
    assert _call(name, nnz=0, Prowind=None, Porder=None, Parg=None, Pgrad_out=None, Pgrad_B=None) == EINVAL
    # overlap: grad_B (K N 2 = 64 bytes) on grad_out (64 bytes) or on arg (128 bytes)
    assert _call(name, Pgrad_B=0x5000 + 4) == EINVAL
    assert _call(name, Pgrad_B=0x5000 + 62) == EINVAL
    assert _call(name, Pgrad_B=0x4000 + 124) == EINVAL
    assert _call(name, Pgrad_out=0x6000 + 32) == EINVAL
    accepted = [dict(Pgrad_out=0x5002), dict(Pgrad_B=0x6002), dict(Pgrad_B=0x5000 + 64), dict(Pgrad_B=0x4000 + 128), dict(Pgrad_out=0x6000 + 64),
                dict(dtype=BF16)]
    codes = _accepted([(name, o) for o in accepted])
    assert all(rc >= 0 for rc in codes), list(zip(accepted, codes))


def test_route_table_is_the_fp32_one_at_the_effective_alignment(pkg):
    from gespmm_amd import _lib

    assert sorted(ROUTES) == [1, 3, 4, 20, 47, 64, 128, 130, 256, 260, 602]
    for N, want in ROUTES.items():
        for i, (x16_align, arg_align) in enumerate(((2, 4), (4, 8), (8, 16))):
            geo = _lib.max_arg_route_x16(300, 2500, N, x16_align, arg_align)
            assert geo == want[i], (N, x16_align, arg_align)
            assert geo == _lib.max_arg_route(300, 2500, N, 2 * x16_align, arg_align), (N, x16_align)
            # wider than needed on one side changes nothing; 16-byte aligned 16-bit arrays count as 8 (V = 8 is not built)
            assert _lib.max_arg_route_x16(300, 2500, N, 16, arg_align) == geo and _lib.max_arg_route_x16(300, 2500, N, x16_align, 16) == geo
        # narrowing either alignment alone narrows V
        for x16_align, arg_align, j in ((2, 16, 0), (8, 4, 0), (4, 16, 1), (8, 8, 1), (16, 16, 2)):
            assert _lib.max_arg_route_x16(300, 2500, N, x16_align, arg_align) == want[j], (N, x16_align, arg_align)
    assert _lib.max_arg_route_x16(300, 2500, 128, 8, 16)[0] == 4 and _lib.max_arg_route_x16(300, 2500, 128, 4, 16)[0] == 2
    assert _lib.max_arg_route_x16(300, 2500, 128, 8, 8)[0] == 2 and _lib.max_arg_route_x16(300, 2500, 128, 2, 16)[0] == 1
    assert _lib.max_arg_route_x16(1 << 17, 1 << 19, 260) == (4, 2, 64)
    assert _lib.max_arg_route_x16(1 << 17, 1 << 19, 260, 4, 16) == (2, 2, 64)
    assert _lib.max_arg_route_x16(0, 0, 64) is None and _lib.max_arg_route_x16(300, 2500, 0) is None
    for bad in ((-1, 0, 4, 16, 16), (4, -1, 4, 16, 16), (4, 4, -1, 16, 16), (4, 4, 4, 1, 16), (4, 4, 4, 16, 2), (4, 4, 4, 6, 16), (4, 4, 4, 16, 12)):
        with pytest.raises(_lib.GespmmError) as e:
            _lib.max_arg_route_x16(*bad)
        assert e.value.code == EINVAL, bad
    with pytest.raises(_lib.GespmmError) as e:
        _lib.max_arg_route_x16(MAX_M + 1, 4, 4)
    assert e.value.code == ERANGE


def _narrow(a, dt):
    """fp32 host array -> (its 16-bit rounding, to nearest even, as a torch tensor; that tensor's exact fp32 widening as numpy)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt)
    return t, t.float().numpy()


@pytest.mark.parametrize("dt", (torch.float16, torch.bfloat16))
def test_oracle_on_the_hand_written_case(dt):
    """The case of test_restatement_on_a_hand_written_case. Every finite value of it but -10000 in bf16 is a 16-bit value (-20000 and
    -30000 are fp16 values: multiples of 16 below 2^15), so narrowing B changes nothing the chains see."""
    nz, pz = np.float32(-0.0), np.float32(0.0)
    B = np.array([[1.0, pz, -20000.0], [3.0, nz, -30000.0], [3.0, pz, NAN], [nz, 5.0, -10000.0], [pz, NAN, NAN]], dtype=np.float32)
    rows = [[0, 1, 2, 1], [3, 4], [4, 3], [0, 1], [], [2, 2]]
    rowptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    colind = np.array([c for r in rows for c in r], dtype=np.int32)
    B16, Bw = _narrow(B, dt)
    want_arg = np.array([[1, 0, -1], [4, 4, -1], [6, 7, -1], [9, 8, -1], [-1, -1, -1], [10, 10, -1]], dtype=np.int32)
    if dt == torch.float16:
        ok = ~np.isnan(B)
        assert np.array_equal(np.isnan(Bw), ~ok) and np.array_equal(Bw[ok].view(np.uint32), B[ok].view(np.uint32))  # lossless
    else:
        # bf16 has 8 significant bits: -10000 -> -9984, -20000 -> -19968, -30000 -> -29952; node 3's -9984 now BEATS empty_value = -10000
        assert Bw[3, 2] == -9984.0 and Bw[0, 2] == -19968.0 and Bw[1, 2] == -29952.0
        want_arg[1, 2], want_arg[2, 2] = 4, 7  # rows 1 and 2 hold node 3 at positions 4 and 7
    C, arg = max_arg_forward(rowptr, colind, Bw, -10000.0)
    assert np.array_equal(arg, want_arg), arg
    C16, Cw = _narrow(C, dt)
    E = np.float32(-10000.0)
    kept = C != E
    assert np.array_equal(Cw[kept].view(np.uint32), C[kept].view(np.uint32))  # a max rounds nothing: the winners are 16-bit values
    assert np.signbit(Cw[1, 0]) and not np.signbit(Cw[2, 0])                   # the sign of the winning zero survives
    empty_bits = int(C16.view(torch.int16)[4, 0].item()) & 0xFFFF
    if dt == torch.float16:
        assert empty_bits == 0xF0E2 and Cw[4, 0] == -10000.0  # fp16 holds -10000: 1.220703125 x 2^13
    else:
        # fp32 -10000 = 0xC61C4000: the discarded half 0x4000 is below the tie, so narrow(-10000) = 0xC61C = -9984
        assert empty_bits == 0xC61C and Cw[4, 0] == -9984.0
    # compared exactly, narrowed only at the store: a bf16 -9984 wins over the fp32 empty_value, while -10000 itself could not
    assert (arg[4] == -1).all() and (C[4] == E).all()

    colptr, rowind, order = transpose(rowptr, colind, 5)
    g16, gw = _narrow((np.arange(18, dtype=np.float32).reshape(6, 3) + 1) / 8, dt)
    grad_B = max_backward(colptr, rowind, order, arg, gw, 5)
    _, gBw = _narrow(grad_B, dt)
    assert np.array_equal(gBw, grad_B)  # multiples of 1/8 below 8: sums and their narrowing are exact in both types
    assert np.isclose(grad_B.sum(dtype=np.float64), gw[arg >= 0].sum(dtype=np.float64))
