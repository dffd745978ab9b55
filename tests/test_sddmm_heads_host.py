"""Multi-head SDDMM, host side only (no GPU): the new symbols, the return codes of the entry points before any device work, what
gespmm_describe_sddmm_heads reports (resolve_sddmm_heads, the function the launch itself runs) against the documented rules restated
here, and the lane oracle per head against float64."""
import ctypes

import numpy as np
import pytest

EINVAL, EALIGN, ERANGE = -1, -2, -3
MAX_NNZ = 0x7FFFFFFF - 4096
NEW = ("gespmm_sddmm_coo_heads_f32", "gespmm_sddmm_csr_heads_f32", "gespmm_plan_sddmm_heads_f32", "gespmm_describe_sddmm_heads",
       "gespmm_plan_sddmm_heads_route")

HS = tuple(range(1, 10)) + (16,)
FS = (1, 2, 3, 4, 5, 8, 13, 16, 20, 27, 32, 64, 100, 160, 600)
# (M, nnz): short rows; a size whose pair counts nnz H cross both window thresholds (2^20, 2^22) within H = 1 .. 16; mean degree 64 (every
# pair count past 2^22)
SIZES = ((1000, 5000), (300000, 600000), (40000, 2560000))


def test_symbols_and_version(pkg):
    from gespmm_amd import _lib

    for name in NEW:
        assert name in _lib.EXPORTS and getattr(_lib.lib, name) is not None, name
    assert _lib.lib.gespmm_version().decode().startswith("gespmm 0.5 ")
    import gespmm_amd

    assert gespmm_amd.MultiHeadSDDMMFunction is gespmm_amd.op.MultiHeadSDDMMFunction and "MultiHeadSDDMMFunction" in gespmm_amd.__all__
    assert callable(gespmm_amd.sddmm.coo_sddmm_heads) and callable(gespmm_amd.sddmm.csr_sddmm_heads)


def test_return_codes_need_no_gpu(pkg):
    """Negative sizes / H < 1, range, nnz == 0, NULL, alignment — in that order, all before any device work."""
    from gespmm_amd import _lib

    lib = _lib.lib
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    half = ctypes.c_void_p(p.value + 2)
    made_up = ctypes.c_void_p(0x1000)
    coo, csr, plan = lib.gespmm_sddmm_coo_heads_f32, lib.gespmm_sddmm_csr_heads_f32, lib.gespmm_plan_sddmm_heads_f32
    # coo(rowind, colind, D1, D2, out, H, F, nnz, stream) / csr(rowptr, colind, D1, D2, out, M, H, F, nnz, stream)
    for H, F, nnz in ((0, 4, 8), (-1, 4, 8), (2, -4, 8), (2, 4, -8)):
        assert coo(p, p, p, p, p, H, F, nnz, None) == EINVAL, (H, F, nnz)
        assert csr(p, p, p, p, p, 4, H, F, nnz, None) == EINVAL, (H, F, nnz)
        assert coo(None, half, None, p, p, H, F, nnz, None) == EINVAL
    assert csr(p, p, p, p, p, -1, 2, 4, 8, None) == EINVAL
    assert coo(p, p, p, p, p, 0, 4, MAX_NNZ + 1, None) == EINVAL  # sizes that make no sense come before sizes that are too large
    # range: nnz, M, H, the width H F; in COO form the pair count nnz H as well (no composition there)
    for nnz in (MAX_NNZ + 1, 0x7FFFFFFF, 1 << 31, 1 << 40):
        assert coo(None, p, p, p, p, 2, 4, nnz, None) == ERANGE and csr(None, p, p, p, p, 16, 2, 4, nnz, None) == ERANGE, nnz
    assert csr(p, p, p, p, p, 1 << 31, 2, 4, 8, None) == ERANGE
    assert coo(p, p, p, p, p, 1 << 29, 1, 8, None) == ERANGE and csr(p, p, p, p, p, 4, 1 << 29, 1, 8, None) == ERANGE
    assert coo(p, p, p, p, p, 2, 1 << 28, 8, None) == ERANGE and csr(p, p, p, p, p, 4, 1 << 14, 1 << 15, 8, None) == ERANGE
    assert coo(p, p, p, p, p, 8, (1 << 26) - 1, 0, None) == 0  # H F = 2^29 - 8: the widest row the other entries take
    assert coo(p, p, p, p, p, 2, 4, MAX_NNZ // 2 + 1, None) == ERANGE and coo(None, p, p, p, p, 2, 4, MAX_NNZ // 2, None) == EINVAL
    assert csr(None, p, p, p, p, 16, 2, 4, MAX_NNZ // 2 + 1, None) == EINVAL  # CSR form: past the pair limit is the composition's
    # no edges: 0 without looking at pointers
    assert coo(half, half, made_up, None, half, 3, 5, 0, None) == 0 and csr(None, None, None, None, None, 4, 3, 5, 0, None) == 0
    assert csr(None, None, None, None, None, 0, 3, 5, 0, None) == 0
    # NULL, then alignment
    for bad in range(5):
        args = [p] * 5
        args[bad] = None
        assert coo(*args, 3, 5, 8, None) == EINVAL and csr(*args, 4, 3, 5, 8, None) == EINVAL, bad
        args[bad] = half
        assert coo(*args, 3, 5, 8, None) == EALIGN and csr(*args, 4, 3, 5, 8, None) == EALIGN, bad
        args = [made_up] * 5
        args[bad] = ctypes.c_void_p(0x1002)
        assert coo(*args, 3, 5, 8, None) == EALIGN and csr(*args, 4, 3, 5, 8, None) == EALIGN, bad
        other = (bad + 1) % 5
        args[other] = None  # NULL is reported before a misaligned pointer
        assert coo(*args, 3, 5, 8, None) == EINVAL and csr(*args, 4, 3, 5, 8, None) == EINVAL, bad
    # F == 0 writes zeros: out and the index arrays are needed, D1 / D2 are not
    assert coo(p, p, None, None, None, 3, 0, 8, None) == EINVAL and csr(p, p, None, None, half, 4, 3, 0, 8, None) == EALIGN
    # the plan entries without a plan
    assert plan(None, p, p, p, 3, 5, None) == EINVAL
    assert lib.gespmm_plan_sddmm_heads_route(None, 3, 5) == EINVAL


def test_describe_arguments(pkg):
    from gespmm_amd import _lib

    f = _lib.lib.gespmm_describe_sddmm_heads
    buf = ctypes.create_string_buffer(96)
    # f(csr, M, nnz, H, F, d1_align, d2_align, capturing, out, capacity)
    assert f(1, 10, 20, 2, 8, 16, 16, 0, None, 96) == EINVAL and f(1, 10, 20, 2, 8, 16, 16, 0, buf, 0) == EINVAL
    for M, nnz, H, F in ((-1, 20, 2, 8), (10, -1, 2, 8), (10, 20, 0, 8), (10, 20, 2, -8)):
        assert f(1, M, nnz, H, F, 16, 16, 0, buf, 96) == EINVAL
    assert f(1, 10, 20, 2, 8, 2, 16, 0, buf, 96) == EINVAL and f(1, 10, 20, 2, 8, 16, 12, 0, buf, 96) == EINVAL
    assert f(1, 10, MAX_NNZ + 1, 2, 8, 16, 16, 0, buf, 96) == ERANGE and f(1, 1 << 31, 20, 2, 8, 16, 16, 0, buf, 96) == ERANGE
    assert f(1, 10, 20, 1 << 20, 1 << 10, 16, 16, 0, buf, 96) == ERANGE
    assert f(0, 0, MAX_NNZ // 2 + 1, 2, 8, 16, 16, 0, buf, 96) == ERANGE
    want = b"route=kernel form=csr-edge V=4 W=4 epw=32"
    assert f(1, 10, 20, 2, 8, 64, 32, 0, buf, 96) == len(want) and buf.value == want
    small = ctypes.create_string_buffer(8)
    assert f(1, 10, 20, 2, 8, 16, 16, 0, small, 8) == 7 and small.value == b"route=k"  # truncated, NUL-terminated
    assert _lib.describe_sddmm_heads(True, 10, 0, 2, 8) == {"form": "none"} and _lib.describe_sddmm_heads(False, 0, 0, 2, 8) == {"form": "none"}
    assert _lib.describe_sddmm_heads(True, 10, 20, 2, 0) == {"route": "zeros"}
    with pytest.raises(_lib.GespmmError):
        _lib.describe_sddmm_heads(True, 10, 20, 0, 8)


def _want_epw(csr, nnz, H, W):
    """The carried-over fp32 thresholds on the pair count, in whole edges."""
    G, pairs = 64 // W, nnz * H
    per_wave = G * 4 if not csr else 256 if pairs >= 256 * 16384 else 64 if pairs >= 64 * 16384 else max(G * 4, 16)
    return min(256, max(1, per_wave // H))


def test_describe_table(pkg, monkeypatch):
    from gespmm_amd import _lib

    monkeypatch.delenv("GESPMM_SDDMM_HEADS_ROUTE", raising=False)
    seen = set()
    for M, nnz in SIZES:
        for H in HS:
            for F in FS:
                for a1, a2 in ((16, 16), (8, 16), (16, 4), (4, 8), (8, 8), (4, 4)):
                    for csr in (False, True):
                        for cap in (False, True):
                            d = _lib.describe_sddmm_heads(csr, M, nnz, H, F, a1, a2, cap)
                            one = _lib.describe_sddmm(csr, M, nnz, F, a1, a2, cap)
                            what = (csr, M, nnz, H, F, a1, a2, cap, d)
                            assert (d["V"], d["W"]) == (one["V"], one["W"]) and F % d["V"] == 0, what
                            assert d["V"] == max(v for v in (1, 2, 4) if F % v == 0 and min(a1, a2) % (4 * v) == 0), what
                            if H == 1:
                                assert d == dict(one, route="plain"), what
                                continue
                            # the rule after the measurement: the kernel wherever it can run — COO and CSR, capturing or
                            # not, also at mean degree >= 64 where the single-head call walks rows (`one` is row-walk / blocked there)
                            assert d["route"] == "kernel" and set(d) == {"route", "form", "V", "W", "epw"}, what
                            assert d["form"] == ("csr-edge" if csr else "coo-edge") and 1 <= d["epw"] <= 256, what
                            assert d["epw"] == _want_epw(csr, nnz, H, d["W"]), what
                            if csr and nnz // M >= 64:
                                assert one["form"] in ("row-walk", "blocked"), what
                            seen.add(d["epw"])
    assert {1, 2, 4, 8, 16, 32, 64, 128}.issubset(seen), sorted(seen)


def test_describe_pair_limit_and_pin(pkg, monkeypatch):
    from gespmm_amd import _lib

    monkeypatch.delenv("GESPMM_SDDMM_HEADS_ROUTE", raising=False)
    M, H, F = 1 << 24, 8, 8
    at, past = MAX_NNZ // H, MAX_NNZ // H + 1
    assert _lib.describe_sddmm_heads(True, M, at, H, F) == {"route": "kernel", "form": "csr-edge", "V": 4, "W": 4, "epw": 32}
    for cap in (False, True):  # past the limit the kernel cannot run, capturing or not
        assert _lib.describe_sddmm_heads(True, M, past, H, F, capturing=cap) == {"route": "composition", "V": 4, "W": 4}
    assert _lib.describe_sddmm_heads(False, 0, at, H, F)["route"] == "kernel"
    with pytest.raises(_lib.GespmmError):
        _lib.describe_sddmm_heads(False, 0, past, H, F)
    # the pin: read on every call; "kernel" only where the kernel can run, "composition" in CSR form off a capturing stream
    assert _lib.describe_sddmm_heads(True, 1000, 64000, 3, 5)["route"] == "kernel"  # mean degree 64, no pin
    monkeypatch.setenv("GESPMM_SDDMM_HEADS_ROUTE", "composition")
    assert _lib.describe_sddmm_heads(True, 1000, 5000, 3, 5) == {"route": "composition", "V": 1, "W": 4}
    assert _lib.describe_sddmm_heads(True, 1000, 64000, 3, 5) == {"route": "composition", "V": 1, "W": 4}
    assert _lib.describe_sddmm_heads(True, 1000, 5000, 3, 5, capturing=True)["route"] == "kernel"
    assert _lib.describe_sddmm_heads(False, 0, 5000, 3, 5)["route"] == "kernel"
    assert _lib.describe_sddmm_heads(True, 1000, 5000, 1, 5)["route"] == "plain"
    monkeypatch.setenv("GESPMM_SDDMM_HEADS_ROUTE", "kernel")
    assert _lib.describe_sddmm_heads(True, 1000, 64000, 3, 5) == {"route": "kernel", "form": "csr-edge", "V": 1, "W": 4, "epw": 21}
    assert _lib.describe_sddmm_heads(True, M, past, H, F)["route"] == "composition"
    assert _lib.describe_sddmm_heads(True, 1000, 64000, 1, 5)["route"] == "plain"
    monkeypatch.setenv("GESPMM_SDDMM_HEADS_ROUTE", "something else")
    assert _lib.describe_sddmm_heads(True, 1000, 64000, 3, 5)["route"] == "kernel"
    assert _lib.describe_sddmm_heads(True, M, past, H, F)["route"] == "composition"


@pytest.mark.parametrize("H,F,V,W", ((3, 5, 1, 4), (8, 8, 4, 4), (2, 64, 4, 8), (7, 6, 2, 4), (2, 600, 4, 64), (5, 13, 1, 4)))
def test_lane_oracle_per_head_against_float64(oracle, H, F, V, W):
    """What the GPU tests compare with: oracle.sddmm_lanes on the head slices, within 1e-4 * max(|ref|, sum |d1 d2|) of float64."""
    rng = np.random.RandomState(100 * H + F)
    M, K, nnz = 29, 41, 300
    rows = rng.randint(0, M, size=nnz).astype(np.int32)
    cols = rng.randint(0, K, size=nnz).astype(np.int32)
    D1 = (rng.rand(M, H, F).astype(np.float32) - np.float32(0.5)) * np.float32(4)
    D2 = (rng.rand(K, H, F).astype(np.float32) - np.float32(0.5)) * np.float32(4)
    for h in range(H):
        got = oracle.sddmm_lanes(V, W, rows, cols, D1[:, h, :], D2[:, h, :])
        p = D1[rows, h, :].astype(np.float64) * D2[cols, h, :].astype(np.float64)
        ref, scale = p.sum(1), np.abs(p).sum(1)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= 1e-4 * np.maximum(np.abs(ref), scale)), (H, F, h)
    # small integers: exact in any order, so every head equals the plain sum
    I1 = rng.randint(-8, 9, size=(M, H, F)).astype(np.float32)
    I2 = rng.randint(-8, 9, size=(K, H, F)).astype(np.float32)
    for h in range(H):
        assert np.array_equal(oracle.sddmm_lanes(V, W, rows, cols, I1[:, h, :], I2[:, h, :]), (I1[rows, h, :] * I2[cols, h, :]).sum(1))
