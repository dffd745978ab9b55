"""The multi-head product through an edge order and the edge gather, host side only: the symbols, the return-code ladders (fabricated
addresses that the checks never dereference: every call returns before any device work), what the Python wrappers refuse before a launch,
``graphs.take_edges`` on CPU tensors (unchanged by the gather route), and the launch tables the new translation unit must leave alone.
No device is needed."""
import ctypes
import os
import re

import pytest
import torch

EINVAL, EALIGN, ERANGE = -1, -2, -3
I31 = 0x7FFFFFFF

SYMBOLS = ("gespmm_csr_spmm_heads_order_f32", "gespmm_csr_spmm_heads_order_x16", "gespmm_plan_spmm_heads_order_f32", "gespmm_edge_gather")

A = dict
ENTRIES = {
    "gespmm_csr_spmm_heads_order_f32": A(Prowptr=0x1000, Pcolind=0x2000, Porder=0x6000, Pval=0x3000, PB=0x4000, PC=0x5000, M=4, K=4, H=2, F=8,
                                         nnz=5),
    "gespmm_csr_spmm_heads_order_x16": A(Prowptr=0x1000, Pcolind=0x2000, Porder=0x6000, Pval=0x3000, PB=0x4000, PC=0x5000, dtype=2, M=4, K=4,
                                         H=2, F=8, nnz=5),
    "gespmm_edge_gather": A(Px=0x1000, Porder=0x2000, is64=0, Pout=0x3000, n=5, row_bytes=16),
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
        assert name in _lib.EXPORTS, name
        assert getattr(_lib.lib, name) is not None
    assert _lib.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


@pytest.mark.parametrize("name", ("gespmm_csr_spmm_heads_order_f32", "gespmm_csr_spmm_heads_order_x16"))
def test_product_ladder(pkg, name):
    x16 = name.endswith("x16")
    if x16:
        for dt in (0, 3, -1):  # the dtype is looked at first, as by the unordered entry
            assert _call(name, dtype=dt) == EINVAL
            assert _call(name, dtype=dt, M=I31) == EINVAL
    for bad in (A(H=0), A(H=-1), A(M=-1), A(K=-1), A(F=-1), A(nnz=-1)):
        assert _call(name, **bad) == EINVAL, bad
    for bad in (A(M=I31), A(nnz=I31), A(F=I31), A(H=1 << 20, F=1 << 20), A(H=I31)):
        assert _call(name, **bad) == ERANGE, bad
    assert _call(name, M=-1, K=I31 + 5) == EINVAL  # what makes no sense comes before what is too large
    # nothing to do: pointers are not looked at
    assert _call(name, M=0, **_all_null(name)) == 0
    assert _call(name, F=0, **_all_null(name)) == 0
    assert _call(name, M=0, PB=0x4001, Pval=0x3002, Porder=0x6001) == 0
    for k in ("Prowptr", "Pcolind", "Pval", "PB", "PC"):
        assert _call(name, **{k: None}) == EINVAL, k
    assert _call(name, PB=None, Porder=0x6002) == EINVAL  # NULL before alignment
    assert _call(name, Porder=0x6002) == EALIGN
    assert _call(name, Porder=0x6001) == EALIGN
    assert _call(name, Pval=0x3002) == EALIGN
    assert _call(name, Prowptr=0x1002) == EALIGN
    assert _call(name, Pcolind=0x2002) == EALIGN
    assert _call(name, PC=0x5001) == EALIGN
    assert _call(name, PB=0x4001) == EALIGN
    if not x16:
        assert _call(name, PB=0x4002) == EALIGN and _call(name, PC=0x5002) == EALIGN
    # order == NULL is the unordered entry: its ladder, nothing of the order's
    for bad, rc in ((A(H=0), EINVAL), (A(M=I31), ERANGE), (A(Pval=None), EINVAL), (A(Pval=0x3002), EALIGN)):
        assert _call(name, Porder=None, **bad) == rc, bad
    assert _call(name, Porder=None, M=0, **{k: None for k in _all_null(name) if k != "Porder"}) == 0


def test_plan_entry_without_a_plan(pkg):
    from gespmm_amd import _lib

    f = _lib.lib.gespmm_plan_spmm_heads_order_f32
    p = ctypes.c_void_p
    assert f(None, p(0x6000), p(0x3000), p(0x4000), p(0x5000), 2, 8, None) == EINVAL
    assert f(None, None, p(0x3000), p(0x4000), p(0x5000), 2, 8, None) == EINVAL  # (the unordered plan entry's answer)


def test_gather_ladder(pkg):
    name = "gespmm_edge_gather"
    for rb in (0, -4, 1, 2, 3, 6, 18, 63, 65, 68, 128, 1 << 20):
        assert _call(name, row_bytes=rb) == EINVAL, rb
        assert _call(name, row_bytes=rb, n=0) == EINVAL, rb
    for bad in (A(n=-1), A(is64=2), A(is64=-1)):
        assert _call(name, **bad) == EINVAL, bad
    assert _call(name, n=I31) == ERANGE
    assert _call(name, n=-1, row_bytes=68) == EINVAL
    assert _call(name, n=0, **_all_null(name)) == 0  # nothing to do: pointers are not looked at
    assert _call(name, n=0, Px=0x1001) == 0
    for k in ("Px", "Porder", "Pout"):
        assert _call(name, **{k: None}) == EINVAL, k
    assert _call(name, Px=None, Pout=0x3002) == EINVAL  # NULL before alignment
    for rb in range(4, 68, 4):
        assert _call(name, row_bytes=rb, Px=0x1002) == EALIGN, rb
    assert _call(name, Pout=0x3001) == EALIGN
    assert _call(name, Porder=0x2002) == EALIGN
    assert _call(name, Porder=0x2004, is64=1) == EALIGN  # an int64 order needs 8 bytes


def test_python_errors_raise_without_launching(pkg):
    """``order=`` is validated by one function before either wrapper touches the library: it needs no device to be asked."""
    from gespmm_amd import spmm

    dev = torch.device("cpu")
    nnz = 12
    good = torch.arange(nnz, dtype=torch.int32)
    spmm._need_order(good, nnz, dev)
    with pytest.raises(TypeError, match="convert it once"):
        spmm._need_order(good.long(), nnz, dev)
    for bad in (good.float(), good.to(torch.int16), list(range(nnz))):
        with pytest.raises(TypeError):
            spmm._need_order(bad, nnz, dev)
    for bad in (good[:-1], torch.arange(nnz + 1, dtype=torch.int32), good.view(3, 4), torch.arange(2 * nnz, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError):
            spmm._need_order(bad, nnz, dev)
    with pytest.raises(ValueError, match="must live on"):  # wrong device: a CPU order for tensors of a GPU
        spmm._need_order(good, nnz, torch.device("cuda", 0))
    # the wrappers ask it (and everything else) before the library: nothing here is a device tensor, so nothing can have been launched
    rp = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        spmm.csr_spmm_heads(rp, good, torch.zeros(nnz, 2), torch.zeros(2, 2, 4), order=good)
    import inspect

    for fn in (spmm.csr_spmm_heads, spmm.csr_spmm_heads_x16, spmm.SpmmPlan.run_heads):
        assert inspect.signature(fn).parameters["order"].default is None, fn


def test_take_edges_on_cpu_tensors_is_unchanged(pkg):
    from gespmm_amd import graphs

    gen = torch.Generator().manual_seed(1)
    n = 1000
    for odt in (torch.int32, torch.int64):
        order = torch.randperm(n, generator=gen).to(odt)
        rep = torch.randint(0, n, (n,), generator=gen).to(odt)
        for x in (torch.rand(n, generator=gen), torch.rand(n, 4, generator=gen), torch.rand(n, 3, 5, generator=gen).to(torch.bfloat16),
                  torch.randint(0, 99, (n, 2), generator=gen).to(torch.int32), torch.rand(n, 8, generator=gen)[:, ::2],
                  torch.rand(n, 17, generator=gen)):
            for o in (order, rep):
                got = graphs.take_edges(x, o)
                want = x[o.long()]
                assert got.is_contiguous() and got.dtype == x.dtype and got.shape == want.shape
                assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))
                assert torch.equal(graphs.take_edges(x, o, chunk_rows=7).view(torch.uint8), got.view(torch.uint8))
    assert graphs.take_edges(torch.empty(0, 4), torch.empty(0, dtype=torch.int64)).shape == (0, 4)
    x = torch.rand(10, 4, generator=gen)
    for bad in (torch.arange(10).index_fill(0, torch.tensor([3]), 10), torch.arange(10).index_fill(0, torch.tensor([0]), -1)):
        with pytest.raises(IndexError):
            graphs.take_edges(x, bad)
    with pytest.raises(ValueError):
        graphs.take_edges(x, torch.arange(9))
    with pytest.raises(TypeError):
        graphs.take_edges(x, torch.arange(10).to(torch.int16))
    with pytest.raises(ValueError):
        graphs.take_edges(x, torch.arange(10), chunk_rows=0)
    # grad mode: differentiable when x requires grad, a plain copy otherwise
    order = torch.randperm(10, generator=gen)
    xg = x.clone().requires_grad_(True)
    y = graphs.take_edges(xg, order, chunk_rows=3)
    assert y.requires_grad and torch.equal(y.detach(), x[order])
    y.sum().backward()
    assert torch.equal(xg.grad, torch.ones_like(x))
    with torch.no_grad():
        assert not graphs.take_edges(xg, order).requires_grad
    assert not graphs.take_edges(xg.detach(), order).requires_grad


def test_launch_tables_of_the_unordered_kernels_read_as_before(pkg):
    """The ordered kernels live in a translation unit of their own: the two tables the other tests read keep their 14 and 11 entries, the
    new table names the 11 stateless geometries, and the table macro of spmm_heads.hip appears in no other file."""
    from helpers import ROOT

    csrc = os.path.join(ROOT, "gespmm_amd", "csrc")
    text = open(os.path.join(csrc, "spmm_heads.hip")).read()
    body = text[text.index("static hipError_t launch_heads_geometry"):text.index("#undef GESPMM_HEADS")]
    common, planned = body.split("if constexpr (PLANNED)")
    f32 = [re.findall(r"^\s*GESPMM_HEADS\((\d), (\d), (\d+)\)", part, flags=re.M) for part in (common, planned)]
    assert len(f32[0]) == 11 and len(f32[1]) == 3 and len(set(f32[0]) | set(f32[1])) == 14
    text = open(os.path.join(csrc, "spmm_heads_x16.hip")).read()
    body = text[text.index("static hipError_t launch_heads_x16_geometry"):text.index("#undef GESPMM_HEADS_X16")]
    x16 = re.findall(r"^\s*GESPMM_HEADS_X16\((\d), (\d), (\d+)\)", body, flags=re.M)
    assert len(x16) == 11 and set(x16) == set(f32[0])
    text = open(os.path.join(csrc, "spmm_heads_order.hip")).read()
    body = text[text.index("static hipError_t launch_ordered_geometry"):text.index("#undef GESPMM_ORDERED")]
    ordered = re.findall(r"^\s*GESPMM_ORDERED\((\d), (\d), (\d+)\)", body, flags=re.M)
    assert len(ordered) == 11 and set(ordered) == set(f32[0])
    for fn in os.listdir(csrc):
        if fn not in ("spmm_heads.hip", "spmm_heads_x16.hip"):
            assert "GESPMM_HEADS(" not in open(os.path.join(csrc, fn), errors="replace").read(), fn
