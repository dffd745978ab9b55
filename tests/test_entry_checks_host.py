"""The argument checks of every stateless entry point of include/gespmm.h that validates arguments, host side only: a hand-written table of
return codes. Every call in it returns from the checks — the addresses are fabricated and never dereferenced, no device is needed — and the
order of the checks is part of what is pinned: GESPMM_EINVAL for sizes that make no sense, then GESPMM_ERANGE for sizes past the 32-bit
limits, then 0 where nothing is left to do (pointers may be NULL), then GESPMM_EINVAL for a required pointer that is NULL, then GESPMM_EALIGN."""
import ctypes

import pytest

EINVAL, EALIGN, ERANGE = -1, -2, -3
I31 = 0x7FFFFFFF
MAX_M, MAX_K, MAX_N, MAX_NNZ = I31 - 64, I31, I31 // 4, I31 - 4096  # the CSR x dense products
SDDMM_MAX_M, SDDMM_MAX_NNZ = I31 - 1, I31 - 4096                     # the SDDMM family
SOFTMAX_MAX_M = I31 - 4096
NAN, INF = float("nan"), float("inf")

# name -> the arguments in call order with values every check accepts (the stream, always NULL, is appended). Names that start with a
# capital P are pointers: an int is a fabricated address, None is NULL.
A = dict  # noqa: E731
SPMM = A(Prowptr=0x1000, Pcolind=0x2000, Pval=0x3000, PB=0x4000, PC=0x5000, M=4, K=4, N=8, nnz=5, variant=-1)
ENTRIES = {
    "gespmm_csr_spmm_f32": SPMM,
    "gespmm_csr_spmm_f32_cfg": A(SPMM, cfg=None),
    "gespmm_csr_spmm_f32_ws": A(SPMM, cfg=None, Pworkspace=None, workspace_bytes=0),
    "gespmm_csr_spmm_max_f32": A(Prowptr=0x1000, Pcolind=0x2000, PB=0x4000, PC=0x5000, M=4, K=4, N=8, nnz=5, empty_value=0.0, variant=-1),
    "gespmm_csr_spmm_fused_f32": A(Prowptr=0x1000, Pcolind=0x2000, Pval=0x3000, PB=0x4000, Pcol_scale=0x6000, Prow_scale=0x7000, Pbias=0x8000,
                                   PC=0x5000, M=4, K=4, N=8, nnz=5, variant=-1),
    "gespmm_csr_spmm_x16": A(Prowptr=0x1000, Pcolind=0x2000, Pval=0x3000, PB=0x4000, PC=0x5000, dtype=2, M=4, K=4, N=8, nnz=5, variant=-1),
    "gespmm_csr_spmm_heads_f32": A(Prowptr=0x1000, Pcolind=0x2000, Pval=0x3000, PB=0x4000, PC=0x5000, M=4, K=4, H=2, F=8, nnz=5),
    "gespmm_sddmm_coo_f32": A(Prowind=0x1000, Pcolind=0x2000, PD1=0x3000, PD2=0x4000, Pout=0x5000, nnz=5, N=8),
    "gespmm_sddmm_csr_f32": A(Prowptr=0x1000, Pcolind=0x2000, PD1=0x3000, PD2=0x4000, Pout=0x5000, M=4, nnz=5, N=8),
    "gespmm_sddmm_coo_x16": A(Prowind=0x1000, Pcolind=0x2000, PD1=0x3000, PD2=0x4000, Pout=0x5000, dtype=1, nnz=5, N=8),
    "gespmm_sddmm_csr_x16": A(Prowptr=0x1000, Pcolind=0x2000, PD1=0x3000, PD2=0x4000, Pout=0x5000, dtype=1, M=4, nnz=5, N=8),
    "gespmm_sddmm_coo_heads_f32": A(Prowind=0x1000, Pcolind=0x2000, PD1=0x3000, PD2=0x4000, Pout=0x5000, H=2, F=8, nnz=5),
    "gespmm_sddmm_csr_heads_f32": A(Prowptr=0x1000, Pcolind=0x2000, PD1=0x3000, PD2=0x4000, Pout=0x5000, M=4, H=2, F=8, nnz=5),
    "gespmm_edge_softmax_f32": A(Prowptr=0x1000, Pscore=0x2000, Pout=0x3000, M=4, H=2, nnz=5, slope=0.2),
    "gespmm_edge_softmax_backward_f32": A(Prowptr=0x1000, Palpha=0x2000, Pgrad_alpha=0x3000, Pscore=0x4000, Pgrad_score=0x5000, M=4, H=2, nnz=5,
                                          slope=0.2),
    "gespmm_csr2csc_f32": A(Prowptr=0x1000, Pcolind=0x2000, Pcsr_val=0x3000, Pcolptr=0x4000, Prowind=0x5000, Pcsc_val=0x6000, M=4, K=4, nnz=5,
                            Pworkspace=0x7000),
    "gespmm_baseline_atomic_scatter_f32": A(Prowptr=0x1000, Pcolind=0x2000, Pin=0x3000, Pout=0x4000, M=4, K=4, N=8, nnz=5),
    "gespmm_baseline_copy_f32": A(Psrc=0x1000, Pdst=0x2000, n=5),
}


def _cfg(**kw):
    from gespmm_amd import _lib

    return _lib.LaunchCfg(**kw)


def _call(name, **override):
    from gespmm_amd import _lib

    args = dict(ENTRIES[name])
    for k in override:
        assert k in args, (name, k)
    args.update(override)
    values = []
    for k, v in args.items():
        if k == "cfg":
            values.append(ctypes.byref(v) if v is not None else None)
        elif k.startswith("P"):
            values.append(ctypes.c_void_p(v) if v is not None else None)
        else:
            values.append(v)
    return getattr(_lib.lib, name)(*values, None)


def _all_null(name):
    return {k: None for k in ENTRIES[name] if k.startswith("P")}


# ---- the CSR x dense products that share (M, K, N, nnz): fp32, cfg, ws, max, fused, x16
PRODUCTS = ("gespmm_csr_spmm_f32", "gespmm_csr_spmm_f32_cfg", "gespmm_csr_spmm_f32_ws", "gespmm_csr_spmm_max_f32", "gespmm_csr_spmm_fused_f32",
            "gespmm_csr_spmm_x16")


@pytest.mark.parametrize("name", PRODUCTS)
def test_products_sizes(pkg, name):
    for bad in (A(M=-1), A(K=-1), A(N=-1), A(nnz=-2), A(M=-(1 << 40))):
        assert _call(name, **bad) == EINVAL, bad
    for past in (A(M=MAX_M + 1), A(K=MAX_K + 1), A(N=MAX_N + 1), A(nnz=MAX_NNZ + 1), A(M=1 << 40)):
        assert _call(name, **past) == ERANGE, past
    # at the limit the size checks pass: the NULL is what is reported
    for at in (A(M=MAX_M), A(K=MAX_K), A(N=MAX_N), A(nnz=MAX_NNZ)):
        assert _call(name, PC=None, **at) == EINVAL, at
    # nothing to do: legal whatever the pointers are, at the other sizes' limits too
    null = _all_null(name)
    assert _call(name, M=0, **null) == 0
    assert _call(name, N=0, **null) == 0
    assert _call(name, M=0, K=MAX_K, N=MAX_N, nnz=MAX_NNZ, **null) == 0
    # precedence: a size that makes no sense before one that is too large, both before nothing-to-do, all before the pointers
    assert _call(name, M=-1, N=MAX_N + 1) == EINVAL
    assert _call(name, M=0, K=MAX_K + 1, **null) == ERANGE
    assert _call(name, N=0, nnz=-2, **null) == EINVAL
    assert _call(name, M=-1, PB=0x4002) == EINVAL
    assert _call(name, K=-1, PC=0x5001, Prowptr=None) == EINVAL
    assert _call(name, nnz=MAX_NNZ + 1, PC=None) == ERANGE
    assert _call(name, N=MAX_N + 1, Prowptr=None, PB=0x4001) == ERANGE


@pytest.mark.parametrize("name", PRODUCTS)
def test_products_pointers(pkg, name):
    for ptr in ("Prowptr", "Pcolind", "PB", "PC"):
        assert _call(name, **{ptr: None}) == EINVAL, ptr
    # no entries: colind and B are not looked at, rowptr and C still are
    assert _call(name, nnz=0, Pcolind=None, PB=None, PC=None) == EINVAL
    assert _call(name, nnz=0, Pcolind=None, PB=None, Prowptr=None) == EINVAL
    # NULL before alignment
    assert _call(name, PC=None, PB=0x4001) == EINVAL
    assert _call(name, Pcolind=None, Prowptr=0x1002) == EINVAL
    elem = {p: 4 for p in ENTRIES[name] if p.startswith("P") and p != "Pworkspace"}
    if name == "gespmm_csr_spmm_x16":
        elem["PB"] = elem["PC"] = 2
    for ptr, size in elem.items():
        assert _call(name, **{ptr: ENTRIES[name][ptr] + size // 2}) == EALIGN, ptr
        assert _call(name, **{ptr: ENTRIES[name][ptr] + size + size // 2}) == EALIGN, ptr
    # alignment before the variant
    assert _call(name, variant=17, PB=0x4001) == EALIGN
    for variant in (-2, 6, 17):
        assert _call(name, variant=variant) == EINVAL, variant


def test_products_particulars(pkg):
    # fp32 / cfg / ws / max: nothing-to-do comes before the variant is looked at; fused and x16 look at the variant first
    null = A(Prowptr=None, Pcolind=None, PB=None, PC=None)
    for name in ("gespmm_csr_spmm_f32", "gespmm_csr_spmm_f32_cfg", "gespmm_csr_spmm_f32_ws", "gespmm_csr_spmm_max_f32"):
        assert _call(name, M=0, variant=17, **null) == 0, name
    for name in ("gespmm_csr_spmm_fused_f32", "gespmm_csr_spmm_x16"):
        assert _call(name, M=0, variant=17, **null) == EINVAL, name
    # cfg: the launch knobs that make no sense (after the pointers, after nothing-to-do)
    for name in ("gespmm_csr_spmm_f32_cfg", "gespmm_csr_spmm_f32_ws"):
        for bad in (_cfg(rows_per_wave=-1), _cfg(rows_per_wave=33), _cfg(slab_rows=-1)):
            assert _call(name, cfg=bad) == EINVAL
            assert _call(name, cfg=bad, PB=0x4002) == EALIGN
            assert _call(name, cfg=bad, N=0) == 0
    # ws: the workspace arguments come first of all
    ws = "gespmm_csr_spmm_f32_ws"
    assert _call(ws, workspace_bytes=-1) == EINVAL
    assert _call(ws, workspace_bytes=256, Pworkspace=None) == EINVAL
    assert _call(ws, workspace_bytes=-1, M=MAX_M + 1) == EINVAL
    assert _call(ws, workspace_bytes=256, Pworkspace=None, M=0, **null) == EINVAL
    assert _call(ws, workspace_bytes=256, Pworkspace=0x9000, M=MAX_M + 1) == ERANGE
    # max: no values, and neither the naive nor the parallel-reduction variant
    mx = "gespmm_csr_spmm_max_f32"
    assert _call(mx, variant=0) == EINVAL
    assert _call(mx, variant=5) == EINVAL
    assert _call(mx, variant=0, M=0, **null) == 0
    # fused: the three vectors may be NULL, not misaligned — checked with the other pointers, before the variant and before nothing-to-do
    fu = "gespmm_csr_spmm_fused_f32"
    assert _call(fu, Pcol_scale=None, Prow_scale=None, Pbias=None, PC=None) == EINVAL
    assert _call(fu, Pbias=0x8002, variant=17) == EALIGN
    assert _call(fu, Pbias=0x8002, PC=None) == EINVAL
    assert _call(fu, Pbias=0x8002, N=MAX_N + 1) == ERANGE
    # x16: the element type first of all
    x16 = "gespmm_csr_spmm_x16"
    for dtype in (0, 3, -1):
        assert _call(x16, dtype=dtype) == EINVAL, dtype
        assert _call(x16, dtype=dtype, M=MAX_M + 1) == EINVAL
        assert _call(x16, dtype=dtype, M=0) == EINVAL
    assert _call(x16, dtype=1, PB=0x4001) == EALIGN
    assert _call(x16, dtype=1, Pval=0x3002) == EALIGN


# ---- the multi-head product
def test_heads(pkg):
    name = "gespmm_csr_spmm_heads_f32"
    for bad in (A(H=0), A(H=-1), A(M=-1), A(K=-1), A(F=-1), A(nnz=-1)):
        assert _call(name, **bad) == EINVAL, bad
    for past in (A(M=MAX_M + 1), A(K=MAX_K + 1), A(H=MAX_N + 1), A(H=2, F=MAX_N // 2 + 1), A(H=1, F=MAX_N + 1), A(nnz=MAX_NNZ + 1)):
        assert _call(name, **past) == ERANGE, past
    for at in (A(M=MAX_M), A(K=MAX_K), A(H=MAX_N, F=1), A(H=2, F=MAX_N // 2), A(H=1, F=MAX_N), A(nnz=MAX_NNZ)):
        assert _call(name, PC=None, **at) == EINVAL, at
    null = _all_null(name)
    assert _call(name, M=0, **null) == 0
    assert _call(name, F=0, **null) == 0
    assert _call(name, F=0, H=0, **null) == EINVAL
    assert _call(name, M=0, K=MAX_K + 1, **null) == ERANGE
    for ptr in ("Prowptr", "Pcolind", "Pval", "PB", "PC"):
        assert _call(name, **{ptr: None}) == EINVAL, ptr
        assert _call(name, **{ptr: ENTRIES[name][ptr] + 2}) == EALIGN, ptr
    assert _call(name, nnz=0, Pcolind=None, Pval=None, PB=None, PC=None) == EINVAL
    # precedence
    assert _call(name, H=0, M=MAX_M + 1) == EINVAL
    assert _call(name, M=-1, PB=0x4002) == EINVAL
    assert _call(name, nnz=MAX_NNZ + 1, Pval=None) == ERANGE
    assert _call(name, Pval=None, PB=0x4002) == EINVAL


# ---- the six SDDMM entries
SDDMM = ("gespmm_sddmm_coo_f32", "gespmm_sddmm_csr_f32", "gespmm_sddmm_coo_x16", "gespmm_sddmm_csr_x16", "gespmm_sddmm_coo_heads_f32",
         "gespmm_sddmm_csr_heads_f32")


@pytest.mark.parametrize("name", SDDMM)
def test_sddmm(pkg, name):
    csr, x16, heads = "_csr_" in name, name.endswith("x16"), "heads" in name
    width = "F" if heads else "N"
    rows = "Prowptr" if csr else "Prowind"
    for bad in (A(nnz=-1), {width: -1}) + ((A(M=-1),) if csr else ()) + ((A(H=0), A(H=-2)) if heads else ()) + \
            ((A(dtype=0), A(dtype=3)) if x16 else ()):
        assert _call(name, **bad) == EINVAL, bad
    past = [A(nnz=SDDMM_MAX_NNZ + 1), {width: MAX_N + 1}] + ([A(M=SDDMM_MAX_M + 1)] if csr else [])
    at = [{width: MAX_N, "H": 1} if heads else {width: MAX_N}] + ([A(M=SDDMM_MAX_M)] if csr else [])
    if heads:
        past += [A(H=MAX_N + 1), A(H=2, F=MAX_N // 2 + 1)]
        at += [A(H=MAX_N, F=1, nnz=1), A(H=2, F=MAX_N // 2)]  # (nnz = 1: the COO form bounds nnz H too)
        if csr:  # pairs past the kernel's limit: the CSR form has the composition
            at += [A(nnz=SDDMM_MAX_NNZ, H=1), A(nnz=SDDMM_MAX_NNZ // 2 + 1, H=2)]
        else:    # ... the COO form has not
            past += [A(nnz=SDDMM_MAX_NNZ // 2 + 1, H=2)]
            at += [A(nnz=SDDMM_MAX_NNZ, H=1), A(nnz=SDDMM_MAX_NNZ // 2, H=2)]
    else:
        at += [A(nnz=SDDMM_MAX_NNZ)]
    for p in past:
        assert _call(name, **p) == ERANGE, p
    for a in at:
        assert _call(name, Pout=None, **a) == EINVAL, a
    # no edges: nothing to do
    null = _all_null(name)
    assert _call(name, nnz=0, **null) == 0
    assert _call(name, nnz=0, **{width: MAX_N + 1}, **null) == ERANGE
    assert _call(name, nnz=0, **{width: -1}, **null) == EINVAL
    if x16:
        assert _call(name, nnz=0, dtype=0, **null) == EINVAL
    for ptr in (rows, "Pcolind", "PD1", "PD2", "Pout"):
        assert _call(name, **{ptr: None}) == EINVAL, ptr
        size = 2 if x16 and ptr in ("PD1", "PD2") else 4
        assert _call(name, **{ptr: ENTRIES[name][ptr] + size // 2}) == EALIGN, ptr
    # width 0: D1 and D2 are not looked at, the rest is
    assert _call(name, PD1=None, PD2=None, Pout=None, **{width: 0}) == EINVAL
    # precedence
    assert _call(name, nnz=-1, PD1=0x3001) == EINVAL
    assert _call(name, nnz=-1, **{width: MAX_N + 1}) == EINVAL
    assert _call(name, nnz=SDDMM_MAX_NNZ + 1, Pcolind=None) == ERANGE
    assert _call(name, PD2=None, PD1=0x3001) == EINVAL


# ---- the edge softmax pair
@pytest.mark.parametrize("name", ("gespmm_edge_softmax_f32", "gespmm_edge_softmax_backward_f32"))
def test_edge_softmax(pkg, name):
    for bad in (A(M=-1), A(H=0), A(H=-1), A(nnz=-1), A(slope=NAN), A(slope=INF), A(slope=-INF), A(M=0, nnz=1)):
        assert _call(name, **bad) == EINVAL, bad
    for past in (A(M=SOFTMAX_MAX_M + 1), A(H=SDDMM_MAX_NNZ + 1, nnz=0), A(H=1, nnz=SDDMM_MAX_NNZ + 1), A(H=2, nnz=SDDMM_MAX_NNZ // 2 + 1)):
        assert _call(name, **past) == ERANGE, past
    for at in (A(M=SOFTMAX_MAX_M), A(H=SDDMM_MAX_NNZ, nnz=1), A(H=1, nnz=SDDMM_MAX_NNZ), A(H=2, nnz=SDDMM_MAX_NNZ // 2)):
        assert _call(name, Prowptr=None, **at) == EINVAL, at
    null = _all_null(name)
    assert _call(name, nnz=0, **null) == 0
    assert _call(name, nnz=0, M=0, **null) == 0
    assert _call(name, nnz=0, M=SOFTMAX_MAX_M + 1, **null) == ERANGE
    assert _call(name, nnz=0, slope=NAN, **null) == EINVAL
    for ptr in ENTRIES[name]:
        if ptr.startswith("P"):
            assert _call(name, **{ptr: None}) == EINVAL, ptr
            assert _call(name, **{ptr: ENTRIES[name][ptr] + 2}) == EALIGN, ptr
    # precedence
    assert _call(name, slope=NAN, M=SOFTMAX_MAX_M + 1) == EINVAL
    assert _call(name, H=0, Prowptr=0x1002) == EINVAL
    assert _call(name, M=SOFTMAX_MAX_M + 1, Prowptr=None) == ERANGE
    result = "Pout" if "Pout" in ENTRIES[name] else "Pgrad_score"
    assert _call(name, Prowptr=None, **{result: ENTRIES[name][result] + 2}) == EINVAL


def test_edge_softmax_backward_score_only_when_leaky(pkg):
    name = "gespmm_edge_softmax_backward_f32"
    # slope == 1: the score is neither required nor looked at — the other pointers still are
    assert _call(name, slope=1.0, Pscore=None, Palpha=None) == EINVAL
    assert _call(name, slope=1.0, Pscore=0x4002, Pgrad_score=None) == EINVAL
    assert _call(name, slope=1.0, Pscore=0x4002, Pgrad_alpha=0x3002) == EALIGN


# ---- csr2csc and the two baselines
def test_csr2csc(pkg):
    name = "gespmm_csr2csc_f32"
    for bad in (A(M=-1), A(K=-1), A(nnz=-1)):
        assert _call(name, **bad) == EINVAL, bad
    for past in (A(M=I31), A(K=I31), A(nnz=I31 + 1)):
        assert _call(name, **past) == ERANGE, past
    for at in (A(M=I31 - 1), A(K=I31 - 1), A(nnz=I31)):
        assert _call(name, Pcolptr=None, **at) == EINVAL, at
    for ptr in ("Prowptr", "Pcolptr", "Pcolind", "Prowind", "Pworkspace", "Pcsr_val", "Pcsc_val"):
        assert _call(name, **{ptr: None}) == EINVAL, ptr
    assert _call(name, nnz=0, Pcolind=None, Prowind=None, Pworkspace=None, Prowptr=None) == EINVAL
    assert _call(name, M=-1, K=I31) == EINVAL
    assert _call(name, M=I31, Prowptr=None) == ERANGE


def test_baselines(pkg):
    name = "gespmm_baseline_atomic_scatter_f32"
    for bad in (A(M=-1), A(K=-1), A(N=-1), A(nnz=-1)):
        assert _call(name, **bad) == EINVAL, bad
    for past in (A(M=I31), A(K=I31 + 1), A(N=MAX_N + 1), A(nnz=I31 + 1)):
        assert _call(name, **past) == ERANGE, past
    for at in (A(M=I31 - 1), A(K=I31), A(N=MAX_N), A(nnz=I31)):
        assert _call(name, Pout=None, **at) == EINVAL, at
    null = _all_null(name)
    assert _call(name, K=0, **null) == 0
    assert _call(name, N=0, **null) == 0
    assert _call(name, N=0, M=I31, **null) == ERANGE
    for ptr in ("Prowptr", "Pcolind", "Pin", "Pout"):
        assert _call(name, **{ptr: None}) == EINVAL, ptr
    assert _call(name, nnz=0, Prowptr=None, Pcolind=None, Pin=None, Pout=None) == EINVAL
    assert _call(name, M=-1, N=MAX_N + 1) == EINVAL
    assert _call(name, nnz=I31 + 1, Pout=None) == ERANGE
    name = "gespmm_baseline_copy_f32"
    assert _call(name, n=-1) == EINVAL
    assert _call(name, n=0, Psrc=None, Pdst=None) == 0
    for ptr in ("Psrc", "Pdst"):
        assert _call(name, **{ptr: None}) == EINVAL, ptr
        assert _call(name, **{ptr: ENTRIES[name][ptr] + 2}) == EALIGN, ptr
    assert _call(name, n=-1, Psrc=0x1002) == EINVAL
    assert _call(name, Psrc=None, Pdst=0x2002) == EINVAL
