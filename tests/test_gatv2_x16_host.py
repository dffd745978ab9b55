"""GATv2 edge score on 16-bit node operands, host side (no GPU): the exported symbols, the return-code ladders of
gespmm_gatv2_score_x16 and gespmm_gatv2_score_backward_x16 (made-up addresses: every call keeps at least one pointer bad, or sizes
that end the call before a pointer is read), the forward's launch shape through gespmm_describe_gatv2_score_x16, the Python wrappers'
argument checks on host tensors, the layer's dtype dispatch, and a check that the comparison tests/test_gpu_gatv2_x16.py makes can
fail."""
import ctypes

import numpy as np
import pytest
import torch

from gatv2_x16_cases import DTYPES, SHAPES, check_patterns, edge_pattern, gaps_pattern, operands
from test_gatv2_host import BIG, OK, restate_score
from test_heads_host import EALIGN, EINVAL, ERANGE

NEW = ("gespmm_gatv2_score_x16", "gespmm_gatv2_score_backward_x16", "gespmm_describe_gatv2_score_x16")
F16, BF16 = 1, 2  # GESPMM_X16_F16, GESPMM_X16_BF16


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_and_version(L, pkg):
    for name in NEW:
        assert name in L.EXPORTS
        getattr(L.lib, name)
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")
    assert callable(pkg.sddmm.gatv2_score_x16) and callable(pkg.sddmm.gatv2_score_backward_x16)


def test_forward_return_codes(L):
    """(rowptr, colind, xl, xr, att, score | dtype, M, K, H, F, nnz, slope, stream): the dtype code, then the fp32 ladder — sizes that
    make no sense, sizes too large, nnz == 0, F == 0, the pointers (NULL, then alignment: 2 bytes for xl and xr, 4 for the rest)."""
    f = L.lib.gespmm_gatv2_score_x16
    none = (None,) * 6
    for bad in (0, 3, -1, 4):
        assert f(*none, bad, 4, 4, 2, 8, 0, 0.2, None) == EINVAL          # a bad dtype code, even where nothing would be launched
        assert f(*(_p(OK),) * 6, bad, 4, 4, 2, 8, 10, 0.2, None) == EINVAL
    for dt in (F16, BF16):
        assert f(*none, dt, 4, 4, 0, 8, 10, 0.2, None) == EINVAL          # H < 1
        assert f(*none, dt, -1, 4, 2, 8, 10, 0.2, None) == EINVAL
        assert f(*none, dt, 4, 4, 2, -8, 10, 0.2, None) == EINVAL
        assert f(*none, dt, 4, 0, 2, 8, 10, 0.2, None) == EINVAL          # K < 1 with entries
        assert f(*none, dt, 4, 4, 2, 8, 10, float("inf"), None) == EINVAL
        assert f(*none, dt, 4, 4, 2, 8, 10, float("nan"), None) == EINVAL
        assert f(*none, dt, 4, 4, 2, 8, BIG, float("nan"), None) == EINVAL  # what makes no sense before what is too large
        assert f(*none, dt, 4, 4, 1, 8, BIG, 0.2, None) == ERANGE           # nnz one past kSddmmMaxNnz
        assert f(*none, dt, 4, 4, 2, 8, BIG // 2 + 1, 0.2, None) == ERANGE  # nnz H
        assert f(*none, dt, BIG, 4, 1, 1, 10, 0.2, None) == ERANGE          # M
        assert f(*none, dt, BIG // 16 + 1, 4, 2, 8, 10, 0.2, None) == ERANGE  # M H F ELEMENTS (not bytes: the fp32 limit)
        assert f(*none, dt, 4, BIG // 16 + 1, 2, 8, 10, 0.2, None) == ERANGE  # K H F
        assert f(*none, dt, (BIG - 1) // 16, (BIG - 1) // 16, 2, 8, 10, 0.2, None) == EINVAL  # the largest that fit: on to the pointers
        assert f(*none, dt, BIG, 4, 1, 1, 0, 0.2, None) == ERANGE           # too large comes before "no entries"
        # no entries: success without a pointer being looked at
        assert f(*none, dt, 4, 4, 2, 8, 0, 0.2, None) == 0
        assert f(*(_p(3),) * 6, dt, 4, 4, 2, 8, 0, 0.2, None) == 0
        # rows of no width: score alone is looked at
        assert f(*none, dt, 4, 4, 2, 0, 10, 0.2, None) == EINVAL
        assert f(*(_p(3),) * 5, _p(OK + 2), dt, 4, 4, 2, 0, 10, 0.2, None) == EALIGN
        # the pointers
        assert f(*none, dt, 4, 4, 2, 8, 10, 0.2, None) == EINVAL
        for bad in range(6):
            assert f(*[None if i == bad else _p(OK) for i in range(6)], dt, 4, 4, 2, 8, 10, 0.2, None) == EINVAL, bad
            assert f(*[_p(OK + 1) if i == bad else _p(OK) for i in range(6)], dt, 4, 4, 2, 8, 10, 0.2, None) == EALIGN, bad  # odd
            if bad not in (2, 3):  # 2-byte aligned is misaligned for everything but xl and xr
                assert f(*[_p(OK + 2) if i == bad else _p(OK) for i in range(6)], dt, 4, 4, 2, 8, 10, 0.2, None) == EALIGN, bad
        assert f(_p(OK), _p(OK), _p(OK), _p(OK), _p(OK + 2), None, dt, 4, 4, 2, 8, 10, 0.2, None) == EINVAL  # NULL before alignment
        assert f(_p(OK), _p(OK), _p(OK), _p(OK), _p(OK + 2), _p(OK), dt, 4, 4, 2, 8, 10, 0.2, None) == EALIGN  # a 2-byte aligned att
        assert f(_p(OK), _p(OK), _p(OK + 1), _p(OK), _p(OK), _p(OK), dt, 4, 4, 2, 8, 10, 0.2, None) == EALIGN  # an odd xl
        assert f(_p(OK), _p(OK), _p(OK), _p(OK + 3), _p(OK), _p(OK), dt, 4, 4, 2, 8, 10, 0.2, None) == EALIGN  # an odd xr


def test_backward_return_codes(L):
    """(ptr, ind, order, grad_score, x_seg, x_ind, att, grad_x, att_part | dtype, S, T, H, F, nnz, slope, stream); order (2) and
    att_part (8) may be NULL; x_seg (4), x_ind (5) and grad_x (7) are 16-bit. nnz == 0 or F == 0 looks at the results alone."""
    f = L.lib.gespmm_gatv2_score_backward_x16
    none = (None,) * 9
    optional, half = (2, 8), (4, 5, 7)
    for bad in (0, 3, -2):
        assert f(*none, bad, 4, 4, 2, 8, 0, 0.2, None) == EINVAL
        assert f(*(_p(OK),) * 9, bad, 4, 4, 2, 8, 10, 0.2, None) == EINVAL
    for dt in (F16, BF16):
        assert f(*none, dt, 4, 4, 0, 8, 10, 0.2, None) == EINVAL
        assert f(*none, dt, -1, 4, 2, 8, 10, 0.2, None) == EINVAL
        assert f(*none, dt, 4, 0, 2, 8, 10, 0.2, None) == EINVAL
        assert f(*none, dt, 4, 4, 2, 8, 10, float("-inf"), None) == EINVAL
        assert f(*none, dt, 4, 4, 2, 8, 10, float("nan"), None) == EINVAL
        assert f(*none, dt, 4, 4, 1, 8, BIG, 0.2, None) == ERANGE
        assert f(*none, dt, 4, 4, 2, 8, BIG // 2 + 1, 0.2, None) == ERANGE
        assert f(*none, dt, BIG, 4, 1, 1, 10, 0.2, None) == ERANGE
        assert f(*none, dt, BIG // 16 + 1, 4, 2, 8, 10, 0.2, None) == ERANGE
        assert f(*none, dt, 4, BIG // 16 + 1, 2, 8, 10, 0.2, None) == ERANGE
        assert f(*none, dt, BIG // 16 + 1, 4, 2, 8, 0, 0.2, None) == ERANGE   # too large comes before "no entries"
        assert f(*none, dt, (BIG - 1) // 16, (BIG - 1) // 16, 2, 8, 10, 0.2, None) == EINVAL
        for F, nnz in ((8, 0), (0, 10)):
            assert f(*none, dt, 4, 4, 2, F, nnz, 0.2, None) == EINVAL                                   # grad_x is needed
            assert f(*(None,) * 7, _p(OK + 1), None, dt, 4, 4, 2, F, nnz, 0.2, None) == EALIGN           # an odd grad_x
            assert f(*(None,) * 7, _p(OK), _p(OK + 2), dt, 4, 4, 2, F, nnz, 0.2, None) == EALIGN         # att_part, where given
            assert f(*(_p(3),) * 7, None, _p(OK), dt, 4, 4, 2, F, nnz, 0.2, None) == EINVAL
        assert f(*(None,) * 7, _p(OK + 2), None, dt, 0, 0, 2, 8, 0, 0.2, None) == 0      # nothing to write; 2-byte aligned is enough
        assert f(*(None,) * 7, _p(OK + 2), _p(OK), dt, 4, 4, 2, 0, 10, 0.2, None) == 0   # F == 0: results of no elements
        assert f(*none, dt, 4, 4, 2, 8, 10, 0.2, None) == EINVAL
        for bad in range(9):
            if bad not in optional:
                assert f(*[None if i == bad else _p(OK) for i in range(9)], dt, 4, 4, 2, 8, 10, 0.2, None) == EINVAL, bad
            assert f(*[_p(OK + 1) if i == bad else _p(OK) for i in range(9)], dt, 4, 4, 2, 8, 10, 0.2, None) == EALIGN, bad
            if bad not in half:  # 2-byte aligned is misaligned for everything that is not 16-bit: att among them
                assert f(*[_p(OK + 2) if i == bad else _p(OK) for i in range(9)], dt, 4, 4, 2, 8, 10, 0.2, None) == EALIGN, bad
        # 2-byte aligned 16-bit operands pass the alignment check: the call goes on to the NULL it still has
        assert f(None, _p(OK), None, _p(OK), _p(OK + 2), _p(OK + 2), _p(OK), _p(OK + 2), None, dt, 4, 4, 2, 8, 10, 0.2, None) == EINVAL
        assert f(*[None if i == 0 else _p(OK + 1) for i in range(9)], dt, 4, 4, 2, 8, 10, 0.2, None) == EINVAL  # NULL before alignment


def test_describe_table(L):
    """V by F and by alignment; W and epw as gespmm_describe_sddmm_heads_x16 answers them at width F."""
    d = lambda F, *al: L.describe_gatv2_score(314, 1345, 2, F, *al, x16=True)  # noqa: E731
    for F, V in ((8, 8), (16, 8), (24, 8), (12, 4), (4, 4), (6, 2), (130, 2), (5, 1), (1, 1), (520, 8)):
        assert d(F)["V"] == V, (F, d(F))
    # the xl (and xr) address at 2, 4, 8, 16 bytes: 2 V bytes divide it
    for al, V in ((2, 1), (4, 2), (8, 4), (16, 8), (64, 8)):
        assert d(8, al, 16, 16)["V"] == V and d(8, 16, al, 16)["V"] == V, al
        assert d(12, al, 16, 16)["V"] == min(V, 4)
    # the att address at 4, 8, 16 bytes: min(4 V, 16) bytes divide it — V = 4 and V = 8 both need 16
    for al, V in ((4, 1), (8, 2), (16, 8), (32, 8)):
        assert d(8, 16, 16, al)["V"] == V, al
    assert d(4, 16, 16, 8)["V"] == 2 and d(4, 16, 16, 16)["V"] == 4 and d(6, 8, 4, 8)["V"] == 2 and d(6, 2, 4, 8)["V"] == 1
    # W and epw: the multi-head SDDMM's rule at element size 2
    for (H, F), V in SHAPES.items():
        for G in (edge_pattern(), gaps_pattern()):
            mine = L.describe_gatv2_score(G["M"], G["nnz"], H, F, x16=True)
            assert mine["V"] == V, ((H, F), mine)
            if H >= 2:
                heads = L.describe_sddmm_heads(True, G["M"], G["nnz"], H, F, x16=True)
                assert (mine["V"], mine["W"], mine["epw"]) == (heads["V"], heads["W"], heads["epw"]), ((H, F), mine, heads)
    got = {hf: L.describe_gatv2_score(314, 1345, hf[0], hf[1], x16=True) for hf in SHAPES}
    assert got[(1, 520)]["W"] == 64 and got[(2, 130)]["W"] == 16 and got[(2, 24)]["W"] == 4
    assert {g["epw"] for g in got.values()} <= {64, 32, 21, 16, 8}, got   # the moduli gaps_pattern's nnz is one past
    # (4, 4): the same (V, W) with and without x16 — where the GPU test expects the fp32 kernel's bits
    assert [got[(4, 4)][k] for k in "VW"] == [L.describe_gatv2_score(314, 1345, 4, 4)[k] for k in "VW"] == [4, 4]
    assert L.describe_gatv2_score(10, 0, 2, 8, x16=True) == {"form": "none"}
    assert L.describe_gatv2_score(10, 5, 2, 0, x16=True) == {"route": "zeros"}
    for bad, code in (((10, 5, 0, 8), EINVAL), ((10, -1, 2, 8), EINVAL), ((10, BIG, 1, 8), ERANGE)):
        with pytest.raises(L.GespmmError) as e:
            L.describe_gatv2_score(*bad, x16=True)
        assert e.value.code == code
    for al in ((1, 16, 16), (16, 12, 16), (16, 16, 2), (16, 16, 0)):
        with pytest.raises(L.GespmmError) as e:
            L.describe_gatv2_score(10, 5, 2, 8, *al, x16=True)
        assert e.value.code == EINVAL
    assert L.describe_gatv2_score(10, 5, 2, 8, 2, 2, 4, x16=True)["V"] == 1
    with pytest.raises(L.GespmmError):   # the fp32 describe keeps its floor of 4 bytes
        L.describe_gatv2_score(10, 5, 2, 8, 2, 16, 16)


def _operands(dt, M=6, K=5, H=3, F=4, nnz=9):
    rp = torch.zeros(M + 1, dtype=torch.int32)
    rp[1:] = nnz
    return {"rp": rp, "ci": torch.zeros(nnz, dtype=torch.int32), "xl": torch.zeros(M, H, F, dtype=dt), "xr": torch.zeros(K, H, F, dtype=dt),
            "att": torch.zeros(H, F), "gs": torch.zeros(nnz, H), "order": torch.arange(nnz, dtype=torch.int32)}


@pytest.mark.parametrize("dt", DTYPES)
def test_python_wrappers_raise_before_any_launch(pkg, dt):
    """TypeError for the dtype of EVERY operand first, then ValueError for shapes, contiguity and devices. Every operand lives on the
    host, so a call that got past its checks raises the device ValueError — which the well-formed calls at the end do."""
    from gespmm_amd import sddmm

    other = torch.bfloat16 if dt == torch.float16 else torch.float16
    o = _operands(dt)
    M, K, H, F, nnz = 6, 5, 3, 4, 9

    def fwd(**kw):
        a = dict(o, **kw)
        return sddmm.gatv2_score_x16(a["rp"], a["ci"], a["xl"], a["xr"], a["att"], negative_slope=a.get("slope", 0.2), out=a.get("out"))

    def bwd(**kw):
        a = dict(o, **kw)
        return sddmm.gatv2_score_backward_x16(a["rp"], a["ci"], a["gs"], a["xl"], a["xr"], a["att"], negative_slope=a.get("slope", 0.2),
                                              order=a.get("order_"), want_att_part=a.get("want", False), out=a.get("out"))

    for call in (fwd, bwd):
        out = torch.zeros(nnz, H) if call is fwd else torch.zeros(M, H, F, dtype=dt)
        # node operands: fp32, fp64 and the OTHER 16-bit type are TypeErrors (mixed fp16 / bf16 among them)
        for name in ("xl", "xr"):
            for bad in (torch.float32, torch.float64, other, torch.int32):
                with pytest.raises(TypeError):
                    call(**{name: o[name].to(bad)})
            with pytest.raises(TypeError):
                call(**{name: None})
            with pytest.raises(TypeError):
                call(**{name: o[name].float().numpy()})
        with pytest.raises(TypeError):
            call(xl=o["xl"].to(other), xr=o["xr"].float())
        # att (and grad_score) stay fp32: a 16-bit one is a TypeError
        for name in ("att",) + (("gs",) if call is bwd else ()):
            for bad in (dt, other, torch.float64):
                with pytest.raises(TypeError):
                    call(**{name: o[name].to(bad)})
            with pytest.raises(TypeError):
                call(**{name: None})
        for bad in ((torch.float16, torch.bfloat16, torch.float64) if call is fwd else (torch.float32, other, torch.float64)):
            with pytest.raises(TypeError):
                call(out=out.to(bad))
        for name in ("rp", "ci") + (("order_",) if call is bwd else ()):
            t = o["order"] if name == "order_" else o[name]
            with pytest.raises(TypeError):
                call(**{name: t.long()})
        # a bad dtype wins over a bad shape of an EARLIER operand: dtypes of every operand come first
        with pytest.raises(TypeError):
            call(rp=o["rp"][:-1], att=o["att"].to(dt))
        with pytest.raises(TypeError):
            call(xl=o["xl"].view(-1), xr=o["xr"].float())
        with pytest.raises(TypeError):
            call(rp=o["rp"].view(1, -1), xl=o["xl"].float(), xr=o["xr"].float())
        for bad in ({"rp": o["rp"][:-1]}, {"ci": o["ci"].view(1, -1)}, {"xl": o["xl"].view(M, -1)},
                    {"xr": torch.zeros(K, H, F + 1, dtype=dt)}, {"att": torch.zeros(1, H, F)}, {"att": torch.zeros(F, H).t()},
                    {"xl": torch.zeros(M, H, 2 * F, dtype=dt)[:, :, ::2]}, {"out": out[:-1]}, {"slope": float("nan")}):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(ValueError, match="device"):
            call()  # well formed, but on the host: the device check is the last one standing
        with pytest.raises(ValueError, match="device"):
            call(out=out)
    with pytest.raises(TypeError):   # att_part stays fp32
        bwd(want=True, out=(torch.zeros(M, H, F, dtype=dt), torch.zeros(M, H, F, dtype=dt)))
    with pytest.raises(ValueError):
        bwd(out=(torch.zeros(M, H, F, dtype=dt), torch.zeros(M, H, F)))  # a pair without want_att_part
    with pytest.raises(ValueError, match="device"):
        bwd(want=True, out=(torch.zeros(M, H, F, dtype=dt), torch.zeros(M, H, F)), order_=o["order"])
    # the fp32 names keep raising TypeError on 16-bit tensors
    with pytest.raises(TypeError):
        sddmm.gatv2_score(o["rp"], o["ci"], o["xl"], o["xr"], o["att"])
    with pytest.raises(TypeError):
        sddmm.gatv2_score_backward(o["rp"], o["ci"], o["gs"], o["xl"], o["xr"], o["att"])


@pytest.mark.parametrize("dt", DTYPES)
def test_layer_gets_past_the_dtype_checks(pkg, dt):
    """GATv2Conv(...).to(dt), fused=False, on host tensors: the 16-bit score op is reached and raises the device ValueError — no
    TypeError about fp32-only kernels; shared weights take the same road. fused=True keeps its TypeError."""
    n = 5
    rp = torch.arange(n + 1, dtype=torch.int32)
    ind = torch.arange(n, dtype=torch.int32)
    x = torch.ones(n, 4, dtype=dt)
    for kw in ({}, {"share_weights": True}, {"concat": False, "bias": False}):
        layer = pkg.GATv2Conv(4, 3, heads=2, **kw).to(dt)
        assert layer.att.dtype == dt
        with pytest.raises(ValueError, match="device"):
            layer(x, rp, ind, rp, ind, ind)
    with pytest.raises(TypeError, match="gatv2_attention"):
        pkg.GATv2Conv(4, 3, heads=2, fused=True).to(dt)(x, rp, ind, rp, ind, None)
    # the function on its own: att must be fp32
    with pytest.raises(TypeError):
        pkg.GATv2ScoreFunction.apply(rp, ind, rp, ind, ind, torch.ones(n, 2, 3, dtype=dt), torch.ones(n, 2, 3, dtype=dt),
                                     torch.ones(2, 3, dtype=dt), 0.2)


def test_the_comparison_can_fail():
    """The GPU test holds the score to 1e-4 max(|ref|, terms) of the float64 restatement on the WIDENED operands. A kernel that widened
    with the wrong type's rule must fall outside: the fp16 operands of every tested shape, their bits re-read as bf16, give a
    restatement that differs from the right one by more than that bound."""
    pats = {"gaps": gaps_pattern(), "edge": edge_pattern()}
    check_patterns(pats)
    G = pats["gaps"]
    for H, F in SHAPES:
        o = operands(G, H, F, "real", torch.float16)
        w = o["wide"]
        ref, terms = restate_score(G["rowptr"], G["colind"], w["xl"], w["xr"], w["att"], 0.2)
        as_bf16 = [t.view(torch.bfloat16).float().numpy() for t in (o["xl"], o["xr"])]
        assert all(np.isfinite(a).all() for a in as_bf16)
        wrong, _ = restate_score(G["rowptr"], G["colind"], as_bf16[0], as_bf16[1], w["att"], 0.2)
        bound = 1e-4 * np.maximum(np.abs(ref), terms)
        assert (bound > 0).all()
        ratio = np.abs(wrong - ref) / bound
        assert ratio.max() > 1.0 and np.median(ratio) > 1.0, ((H, F), ratio.max())
