"""The 16-bit multi-head entries, host side only: the symbols, the return-code ladders (fabricated addresses that the checks never
dereference: every call returns before any device work), the route table of gespmm_heads_x16_route and what
gespmm_describe_sddmm_heads_x16 answers. No device is needed."""
import ctypes
import os

import pytest

EINVAL, EALIGN, ERANGE = -1, -2, -3
I31 = 0x7FFFFFFF

SYMBOLS = ("gespmm_csr_spmm_heads_x16", "gespmm_heads_x16_route", "gespmm_sddmm_coo_heads_x16", "gespmm_sddmm_csr_heads_x16",
           "gespmm_describe_sddmm_heads_x16", "gespmm_describe_sddmm_heads")

# the (H, F) grid of tests/test_gpu_heads_x16.py on the edge-case pattern (M = 21, K = 301, nnz = 1206)
GRID = ((2, 2), (3, 2), (8, 2), (2, 4), (3, 10), (4, 8), (8, 8), (5, 26), (8, 16), (4, 32), (7, 54), (8, 32), (8, 64), (4, 160))
EDGE = dict(M=21, K=301, nnz=1206)

A = dict
ENTRIES = {
    "gespmm_csr_spmm_heads_x16": A(Prowptr=0x1000, Pcolind=0x2000, Pval=0x3000, PB=0x4000, PC=0x5000, dtype=2, M=4, K=4, H=2, F=8, nnz=5),
    "gespmm_sddmm_coo_heads_x16": A(Prowind=0x1000, Pcolind=0x2000, PD1=0x3000, PD2=0x4000, Pout=0x5000, dtype=1, H=2, F=8, nnz=5),
    "gespmm_sddmm_csr_heads_x16": A(Prowptr=0x1000, Pcolind=0x2000, PD1=0x3000, PD2=0x4000, Pout=0x5000, dtype=1, M=4, H=2, F=8, nnz=5),
}


def _call(name, **override):
    from gespmm_amd import _lib

    args = dict(ENTRIES[name])
    for k in override:
        assert k in args, (name, k)
    args.update(override)
    values = [(ctypes.c_void_p(v) if v is not None else None) if k.startswith("P") else v for k, v in args.items()]
    return getattr(_lib.lib, name)(*values, None)


def _all_null(name):
    return {k: None for k in ENTRIES[name] if k.startswith("P")}


def test_symbols_and_version(pkg):
    from gespmm_amd import _lib

    for name in SYMBOLS:
        assert name in _lib.EXPORTS or name == "gespmm_describe_sddmm_heads", name
        assert getattr(_lib.lib, name) is not None
    assert _lib.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


def test_product_ladder(pkg):
    name = "gespmm_csr_spmm_heads_x16"
    # the dtype is looked at first: even with sizes that make no sense or are out of range
    for dt in (0, 3, -1):
        assert _call(name, dtype=dt) == EINVAL
        assert _call(name, dtype=dt, M=I31) == EINVAL
    for dt in (1, 2):
        for bad in (A(H=0), A(H=-1), A(M=-1), A(K=-1), A(F=-1), A(nnz=-1)):
            assert _call(name, dtype=dt, **bad) == EINVAL, bad
        # what the fp32 entry does not take either: rows, entries, the width H F
        for bad in (A(M=I31), A(nnz=I31), A(F=I31), A(H=1 << 20, F=1 << 20), A(H=I31)):
            assert _call(name, dtype=dt, **bad) == ERANGE, bad
        assert _call(name, dtype=dt, M=-1, K=I31 + 5) == EINVAL  # what makes no sense comes before what is too large
        # nothing to do: pointers are not looked at
        assert _call(name, dtype=dt, M=0, **_all_null(name)) == 0
        assert _call(name, dtype=dt, F=0, **_all_null(name)) == 0
        assert _call(name, dtype=dt, M=0, PB=0x4001, Pval=0x3002) == 0
        for k in ("Prowptr", "Pcolind", "Pval", "PB", "PC"):
            assert _call(name, dtype=dt, **{k: None}) == EINVAL, k
        assert _call(name, dtype=dt, PB=None, PC=0x5001) == EINVAL  # NULL before alignment
        # 16-bit arrays need 2-byte alignment, the fp32 and int32 ones 4
        assert _call(name, dtype=dt, PB=0x4001) == EALIGN
        assert _call(name, dtype=dt, PC=0x5001) == EALIGN
        assert _call(name, dtype=dt, Pval=0x3002) == EALIGN
        assert _call(name, dtype=dt, Prowptr=0x1002) == EALIGN
        assert _call(name, dtype=dt, Pcolind=0x2002) == EALIGN


@pytest.mark.parametrize("name", ("gespmm_sddmm_coo_heads_x16", "gespmm_sddmm_csr_heads_x16"))
def test_sddmm_ladder(pkg, name):
    csr = "csr" in name
    for dt in (0, 3):
        assert _call(name, dtype=dt) == EINVAL
        assert _call(name, dtype=dt, nnz=0) == EINVAL  # the dtype comes first
    for bad in (A(H=0), A(H=-3), A(F=-1), A(nnz=-1)) + ((A(M=-1),) if csr else ()):
        assert _call(name, **bad) == EINVAL, bad
    for bad in (A(nnz=I31), A(F=I31), A(H=1 << 20, F=1 << 20)) + ((A(M=I31),) if csr else (A(nnz=1 << 29, H=8),)):
        assert _call(name, **bad) == ERANGE, bad
    assert _call(name, nnz=0, **_all_null(name)) == 0
    if csr:
        assert _call(name, M=0, nnz=0, **_all_null(name)) == 0
    for k in ENTRIES[name]:
        if k.startswith("P"):
            assert _call(name, **{k: None}) == EINVAL, k
    assert _call(name, PD1=0x3001) == EALIGN
    assert _call(name, PD2=0x4001) == EALIGN
    assert _call(name, Pout=0x5002) == EALIGN
    assert _call(name, Pcolind=0x2002) == EALIGN
    # F == 0 looks at neither operand; a 2-byte aligned operand is legal
    assert _call(name, PD1=0x3002, PD2=0x4002, nnz=0) == 0


def test_route_table(pkg, monkeypatch):
    from gespmm_amd import _lib

    monkeypatch.delenv("GESPMM_HEADS_X16_ROUTE", raising=False)
    M, K, nnz = EDGE["M"], EDGE["K"], EDGE["nnz"]
    for H, F in GRID:
        for align in (16, 8, 4):
            route, (V, S, W, rpw) = _lib.heads_x16_route(M, K, H, F, nnz, align, align)
            assert route == 1 and V in (1, 2, 4) and (F // 2) % V == 0 and 4 * V <= align, (H, F, align, V, S, W)
            assert S in (1, 2) and W in (4, 8, 16, 32, 64) and rpw >= 1
    for H, F, ba, ca in ((1, 128, 16, 16), (9, 4, 16, 16), (16, 8, 16, 16), (4, 3, 16, 16), (8, 1, 16, 16), (5, 27, 16, 16),
                         (4, 8, 2, 16), (4, 8, 16, 2), (8, 64, 2, 2)):
        assert _lib.heads_x16_route(M, K, H, F, nnz, ba, ca) == (0, (0, 0, 0, 0)), (H, F, ba, ca)
    # 64-bit offsets: K H F 2 bytes from 2^32, or nnz H from 2^31
    assert _lib.heads_x16_route(1000, 1 << 22, 8, 64, 5000)[0] == 0
    assert _lib.heads_x16_route(1000, (1 << 22) - 1, 8, 64, 5000)[0] == 1
    assert _lib.heads_x16_route(1000, 1000, 8, 64, 1 << 28)[0] == 0
    # the checks of the entry
    for bad in (dict(H=0), dict(M=-1), dict(F=-1)):
        args = dict(M=M, K=K, H=4, F=8, nnz=nnz)
        args.update(bad)
        with pytest.raises(_lib.GespmmError):
            _lib.heads_x16_route(**args)
    # the pin, read per call; the fp32 entry's pin is another variable
    monkeypatch.setenv("GESPMM_HEADS_ROUTE", "composition")
    assert _lib.heads_x16_route(M, K, 4, 8, nnz)[0] == 1
    monkeypatch.delenv("GESPMM_HEADS_ROUTE")
    monkeypatch.setenv("GESPMM_HEADS_X16_ROUTE", "composition")
    for H, F in GRID:
        assert _lib.heads_x16_route(M, K, H, F, nnz) == (0, (0, 0, 0, 0))
    assert _lib.heads_route(M, K, 4, 8, nnz)[0] == 1
    monkeypatch.setenv("GESPMM_HEADS_X16_ROUTE", "kernel")
    assert _lib.heads_x16_route(M, K, 4, 8, nnz)[0] == 1


def test_route_geometries_are_in_the_launch_table(pkg, monkeypatch):
    """Whatever the route query answers for the grid has an instantiation in spmm_heads_x16.hip."""
    import re

    from gespmm_amd import _lib
    from helpers import ROOT

    monkeypatch.delenv("GESPMM_HEADS_X16_ROUTE", raising=False)
    text = open(os.path.join(ROOT, "gespmm_amd", "csrc", "spmm_heads_x16.hip")).read()
    body = text[text.index("static hipError_t launch_heads_x16_geometry"):text.index("#undef GESPMM_HEADS_X16")]
    table = {(int(v), int(s), int(w)) for v, s, w in re.findall(r"^\s*GESPMM_HEADS_X16\((\d), (\d), (\d+)\)", body, flags=re.M)}
    assert len(table) == 11
    for H, F in GRID:
        for align in (16, 8, 4):
            _, (V, S, W, _) = _lib.heads_x16_route(EDGE["M"], EDGE["K"], H, F, EDGE["nnz"], align, align)
            assert (V, S, W) in table, (H, F, align, V, S, W)


def test_describe_sddmm_heads_x16(pkg, monkeypatch):
    from gespmm_amd import _lib

    monkeypatch.delenv("GESPMM_SDDMM_HEADS_ROUTE", raising=False)
    for csr in (True, False):
        for H, F in ((2, 2), (8, 2), (3, 5), (4, 8), (8, 8), (7, 6), (8, 16), (4, 32), (2, 64), (6, 100)):
            for align in (16, 8, 4, 2):
                d = _lib.describe_sddmm_heads(csr, 21, 1206, H, F, align, align, x16=True)
                assert d["route"] == "kernel" and d["form"] == ("csr-edge" if csr else "coo-edge"), d
                assert 1 <= d["V"] <= 8 and F % d["V"] == 0 and 2 * d["V"] <= align and 1 <= d["epw"] <= 256, (H, F, align, d)
                # V and W are the single-head 16-bit call's at width F
                s = _lib.describe_sddmm(csr, 21, 1206, F, align, align, x16=True)
                assert (d["V"], d["W"]) == (s["V"], s["W"]), (d, s)
            # widest vector where everything allows it
            d = _lib.describe_sddmm_heads(csr, 21, 1206, H, F, 16, 16, x16=True)
            assert d["V"] == max(v for v in (1, 2, 4, 8) if F % v == 0)
    # the composition where the fp32 rule answers it: CSR past the pair limit, and the pin (CSR, not capturing)
    big = (I31 - 4096) // 2
    for x16 in (False, True):
        assert _lib.describe_sddmm_heads(True, 1 << 20, big, 4, 8, x16=x16)["route"] == "composition"
        assert _lib.describe_sddmm_heads(True, 1 << 20, big, 2, 8, x16=x16)["route"] == "kernel"
        assert _lib.describe_sddmm_heads(True, 21, 1206, 1, 8, x16=x16)["route"] == "plain"
        assert _lib.describe_sddmm_heads(True, 21, 1206, 4, 0, x16=x16)["route"] == "zeros"
        assert _lib.describe_sddmm_heads(True, 21, 0, 4, 8, x16=x16) == {"form": "none"}
    monkeypatch.setenv("GESPMM_SDDMM_HEADS_ROUTE", "composition")
    for x16 in (False, True):
        assert _lib.describe_sddmm_heads(True, 21, 1206, 4, 8, x16=x16)["route"] == "composition"
        assert _lib.describe_sddmm_heads(True, 21, 1206, 4, 8, capturing=True, x16=x16)["route"] == "kernel"
        assert _lib.describe_sddmm_heads(False, 21, 1206, 4, 8, x16=x16)["route"] == "kernel"
    d = _lib.describe_sddmm_heads(True, 21, 1206, 4, 8, x16=True)
    assert d["V"] == 8 and _lib.describe_sddmm_heads(True, 21, 1206, 4, 8)["V"] == 4
    # alignments: 2 bytes are legal at 16 bits only
    with pytest.raises(_lib.GespmmError):
        _lib.describe_sddmm_heads(True, 21, 1206, 4, 8, 2, 2)
    with pytest.raises(_lib.GespmmError):
        _lib.describe_sddmm_heads(True, 21, 1206, 4, 8, 1, 2, x16=True)
