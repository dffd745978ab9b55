"""Fused GAT backward for el / er, host side (no GPU): the exported symbols, the return-code ladders of gespmm_gat_backward_el_f32 and
gespmm_gat_backward_er_f32 — the checks run before any device work, so NULL or made-up device pointers are enough — and the Python
wrappers' argument checks, which raise before anything is launched (CPU tensors are enough to reach every one of them but the last)."""
import ctypes

import pytest
import torch

from test_heads_host import EALIGN, EINVAL, ERANGE

NEW = ("gespmm_gat_backward_el_f32", "gespmm_gat_backward_er_f32")
OK = 0x1000  # a made-up address: the checks look at the number only and return before anything could read it
BIG = (1 << 31) - 4096  # one past the largest count of 32-bit word positions
STATS = 4  # position of stats among the nine pointers of both calls


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_and_version(L):
    for name in NEW:
        assert name in L.EXPORTS
        getattr(L.lib, name)
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")


@pytest.mark.parametrize("which", ("el", "er"))
def test_return_codes(L, which):
    """The ladder of gespmm_gat_aggregate_f32: sizes that make no sense, sizes too large, then the pointers (NULL, alignment).
    el: (rowptr, colind, el, er, stats, grad_out, feat, delta, grad_el | M, K, H, F, nnz, slope, stream), results at 7 and 8;
    er: (colptr, rowind, el, er, stats, delta, grad_out, feat, grad_er | ...), result at 8."""
    f = getattr(L.lib, "gespmm_gat_backward_%s_f32" % which)
    results = (7, 8) if which == "el" else (8,)
    none = (None,) * 9
    assert f(*none, 4, 4, 0, 8, 10, 0.2, None) == EINVAL        # H < 1
    assert f(*none, -1, 4, 2, 8, 10, 0.2, None) == EINVAL       # negative sizes
    assert f(*none, 4, 4, 2, -8, 10, 0.2, None) == EINVAL
    assert f(*none, 4, 4, 2, 8, -1, 0.2, None) == EINVAL
    assert f(*none, 4, 0, 2, 8, 10, 0.2, None) == EINVAL        # K < 1
    assert f(*none, 0, 4, 2, 8, 10, 0.2, None) == EINVAL        # entries without rows
    assert f(*none, 4, 4, 2, 8, 10, float("inf"), None) == EINVAL
    assert f(*none, 4, 4, 2, 8, 10, float("nan"), None) == EINVAL
    assert f(*none, 4, 4, 2, 8, BIG, 0.2, None) == ERANGE       # nnz H words
    assert f(*none, 4, 4, 8, 1 << 27, 10, 0.2, None) == ERANGE  # H F beyond the width of the other entries
    assert f(*none, 4, 4, 1 << 30, 4, 10, 0.2, None) == ERANGE
    assert f(*none, BIG // 2 + 1, 4, 2, 8, 10, 0.2, None) == ERANGE   # M H words
    assert f(*none, 4, BIG // 2 + 1, 2, 8, 10, 0.2, None) == ERANGE   # K H words
    assert f(*none, BIG // 16 + 1, 4, 2, 8, 10, 0.2, None) == ERANGE  # M H F words: grad_out
    assert f(*none, 4, BIG // 16 + 1, 2, 8, 10, 0.2, None) == ERANGE  # K H F words: feat
    assert f(*none, (BIG - 1) // 16, (BIG - 1) // 16, 2, 8, 10, 0.2, None) == EINVAL  # the largest that fit: on to the pointers
    assert f(*none, 4, 4, 2, 8, 10, 0.2, None) == EINVAL        # NULL where needed
    for bad in range(9):
        assert f(*[None if i == bad else _p(OK) for i in range(9)], 4, 4, 2, 8, 10, 0.2, None) == EINVAL, bad
        assert f(*[_p(OK + 2) if i == bad else _p(OK) for i in range(9)], 4, 4, 2, 8, 10, 0.2, None) == EALIGN, bad
    assert f(*[_p(OK + 4) if i == STATS else _p(OK) for i in range(9)], 4, 4, 2, 8, 10, 0.2, None) == EALIGN  # stats: 8-byte pairs
    assert f(*[None if i == 0 else _p(OK + 2) for i in range(9)], 4, 4, 2, 8, 10, 0.2, None) == EINVAL  # NULL before alignment
    # no entries, or rows of no width: the results alone are looked at (and zero-filled, on a device)
    for F, nnz in ((8, 0), (0, 10)):
        assert f(*none, 4, 4, 2, F, nnz, 0.2, None) == EINVAL
        for i in results:
            args = [None] * 9
            for j in results:
                args[j] = _p(OK)
            args[i] = _p(OK + 2)
            assert f(*args, 4, 4, 2, F, nnz, 0.2, None) == EALIGN, (F, nnz, i)
    if which == "el":
        assert f(*none, 0, 4, 2, 8, 0, 0.2, None) == 0              # M == 0: nothing to write, pointers not looked at
        assert f(*(_p(3),) * 9, 0, 4, 2, 8, 0, 0.2, None) == 0


def test_no_entries_returns_success_without_a_device_pointer_being_read(L):
    """nnz == 0 with no rows at all (M == 0): the row pass has nothing to write and returns success whatever the pointers are."""
    assert L.lib.gespmm_gat_backward_el_f32(*(None,) * 9, 0, 7, 3, 4, 0, 0.2, None) == 0


def _operands(M=6, K=5, H=3, F=4, nnz=9):
    rp = torch.zeros(M + 1, dtype=torch.int32)
    rp[1:] = nnz
    cp = torch.zeros(K + 1, dtype=torch.int32)
    cp[1:] = nnz
    ind = torch.zeros(nnz, dtype=torch.int32)
    return {"rp": rp, "cp": cp, "ci": ind, "ri": ind.clone(), "el": torch.zeros(M, H), "er": torch.zeros(K, H), "stats": torch.ones(M, H, 2),
            "delta": torch.zeros(M, H), "gout": torch.zeros(M, H, F), "feat": torch.zeros(K, H, F)}


def test_python_wrappers_raise_before_any_launch(pkg):
    """TypeError for dtypes and non-tensors, ValueError for shapes, contiguity and devices. Every operand here lives on the host, so a
    call that got past its checks would raise the device ValueError — which the well-formed call at the end does."""
    from gespmm_amd import softmax

    o = _operands()
    M, K, H, F = 6, 5, 3, 4

    def el(**kw):
        a = dict(o, **kw)
        return softmax.gat_backward_el(a["rp"], a["ci"], a["el"], a["er"], a["stats"], a["gout"], a["feat"], negative_slope=a.get("slope", 0.2),
                                       out=a.get("out"))

    def er(**kw):
        a = dict(o, **kw)
        return softmax.gat_backward_er(a["cp"], a["ri"], a["el"], a["er"], a["stats"], a["delta"], a["gout"], a["feat"],
                                       negative_slope=a.get("slope", 0.2), out=a.get("out"))

    for call in (el, er):
        floats = ("el", "er", "stats", "gout", "feat") + (("delta",) if call is er else ())
        for name in floats:
            for dt in (torch.float16, torch.bfloat16, torch.float64, torch.int32):
                with pytest.raises(TypeError):
                    call(**{name: o[name].to(dt)})
            with pytest.raises(TypeError):
                call(**{name: o[name].numpy()})
        for name in (("rp", "ci") if call is el else ("cp", "ri")):
            with pytest.raises(TypeError):
                call(**{name: o[name].long()})
            with pytest.raises(TypeError):
                call(**{name: o[name].tolist()})
        # shapes of what is looked at before the first device check
        for bad in ({"rp": o["rp"].view(1, -1), "cp": o["cp"].view(1, -1)}, {"rp": o["rp"][::2], "cp": o["cp"][::2]},
                    {"el": o["el"].view(-1), "er": o["er"].view(-1)}, {"el": torch.zeros(M, 2 * H)[:, ::2], "er": torch.zeros(K, 2 * H)[:, ::2]},
                    {"el": o["el"][:-1], "er": o["er"][:-1]}, {"slope": float("nan")}, {"slope": float("inf")}):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(ValueError):
            call()  # well formed, but on the host: the device check is the last one standing
    # what only device tensors reach in the order of the checks — the other shapes, the stats' alignment, mixed devices — is covered on
    # the GPU (tests/test_gpu_gat_backward.py)
