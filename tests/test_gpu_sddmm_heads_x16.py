"""Multi-head SDDMM on 16-bit operands (sddmm.csr_sddmm_heads_x16 / coo_sddmm_heads_x16): D1 and D2 fp16 or bf16, out fp32 [nnz, H].

The contract is exact: head h has the bits of the 16-bit single-head call (sddmm.csr_sddmm) on the contiguous copies of its slices
whenever both run at the same (V, W) — which gespmm_describe_sddmm_heads_x16 and gespmm_describe_sddmm_x16 are ASSERTED to report, the
copies being placed at the alignment of the operands. Every result is written into a NaN-prefilled tensor with guard words after it."""
import numpy as np
import pytest
import torch

from helpers import edge_case_csr

pytestmark = pytest.mark.gpu

DTYPES = (torch.float16, torch.bfloat16)
GRID = ((2, 2), (8, 2), (3, 5), (4, 8), (8, 8), (7, 6), (8, 16), (4, 32), (2, 64), (6, 100))
GUARD = 64
PIN = "GESPMM_SDDMM_HEADS_ROUTE"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _align(t):
    a = t.data_ptr()
    return next(p for p in (16, 8, 4, 2) if a % p == 0)


def _rand(rows, H, F, seed, dtype):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.rand((rows, H, F), device="cuda", generator=g) - 0.5).to(dtype)


def _carve(t, off):
    """Same values, storage `off` bytes (even) past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0 and off % 2 == 0 and off < 16
    v = buf[off // 2:off // 2 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _run(f, idx, G, D1, D2):
    nnz, H = G["nnz"], D1.shape[1]
    buf = torch.full((nnz * H + GUARD,), float("nan"), device="cuda")
    out = buf[:nnz * H].view(nnz, H)
    assert f(idx, G["ci"], D1, D2, out=out) is out
    assert bool(torch.isnan(buf[-GUARD:]).all()), "guard words after out were written"
    assert not bool(torch.isnan(out).any()), "an (edge, head) pair was not written"
    return out


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape)
    bad = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
    assert bad == 0, "%s: %d of %d words differ" % (what, bad, got.numel())


def _per_head(_lib, sddmm, G, D1, D2, V, W):
    """The 16-bit single-head call on contiguous copies of every head's slices, placed at the operands' alignment; its described
    (V, W) is asserted to be the multi-head call's."""
    H, F = D1.shape[1:]
    a1, a2 = _align(D1), _align(D2)
    d = _lib.describe_sddmm(True, G["M"], G["nnz"], F, a1, a2, x16=True)
    assert (d["V"], d["W"]) == (V, W), (d, V, W)
    cols = []
    for h in range(H):
        s1, s2 = _carve(D1[:, h, :], a1 % 16), _carve(D2[:, h, :], a2 % 16)
        assert _align(s1) == a1 and _align(s2) == a2
        cols.append(sddmm.csr_sddmm(G["rp"], G["ci"], s1, s2))
    return torch.stack(cols, dim=1)


def _f64(out, G, D1, D2, what=""):
    """Every (edge, head) against float64 accumulation of the widened operands: |out - ref| <= 1e-4 * max(|ref|, sum |d1 d2|)."""
    p = D1[G["ri"].long()].double() * D2[G["ci"].long()].double()
    ref, scale = p.sum(-1), p.abs().sum(-1)
    ok = (out.double() - ref).abs() <= 1e-4 * torch.maximum(ref.abs(), scale)  # (NaN compares false)
    assert bool(ok.all()), "%s: %d of %d results outside the float64 tolerance" % (what, int((~ok).sum()), out.numel())


@pytest.fixture(autouse=True)
def _no_pin(monkeypatch):
    monkeypatch.delenv(PIN, raising=False)


@pytest.fixture(scope="module")
def edge():
    G = edge_case_csr()
    G["rows"] = np.repeat(np.arange(G["M"], dtype=np.int32), np.diff(G["rowptr"]))
    G["rp"], G["ci"], G["ri"] = _dev(G["rowptr"]), _dev(G["colind"]), _dev(G["rows"])
    return G


def _vw(F, align=16):
    """(V, W) by hand at element size 2: V the widest of 8, 4, 2, 1 that divides F and whose 2 V bytes divide the addresses; a lane
    covers min(16 / V, 8) vectors, W the smallest power of two in 4 .. 64 whose lanes cover F."""
    V = max(v for v in (1, 2, 4, 8) if F % v == 0 and align % (2 * v) == 0)
    W = 4
    while W < 64 and W * V * min(16 // V, 8) < F:
        W *= 2
    return V, W


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp16", "bf16"))
@pytest.mark.parametrize("H,F", GRID)
def test_grid(pkg, edge, H, F, dtype):
    from gespmm_amd import _lib, sddmm

    G = edge
    V, W = _vw(F)
    D1, D2 = _rand(G["M"], H, F, 10 * H + F, dtype), _rand(G["K"], H, F, 10 * H + F + 1, dtype)
    assert _align(D1) == 16 and _align(D2) == 16
    for csr in (True, False):
        d = _lib.describe_sddmm_heads(csr, G["M"], G["nnz"], H, F, 16, 16, x16=True)
        assert (d["route"], d["form"], d["V"], d["W"]) == ("kernel", "csr-edge" if csr else "coo-edge", V, W), (d, V, W)
    o_csr = _run(sddmm.csr_sddmm_heads_x16, G["rp"], G, D1, D2)
    o_coo = _run(sddmm.coo_sddmm_heads_x16, G["ri"], G, D1, D2)
    _same(o_coo, o_csr, ("coo vs csr", H, F))
    _same(o_csr, _per_head(_lib, sddmm, G, D1, D2, V, W), ("per-head calls", H, F, V, W))
    _f64(o_csr, G, D1, D2, "grid H=%d F=%d" % (H, F))


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp16", "bf16"))
@pytest.mark.parametrize("off1,off2", ((8, 0), (0, 8), (4, 4), (12, 8), (2, 0), (0, 6), (2, 10)))
def test_carved_operands(pkg, edge, off1, off2, dtype):
    """Operands 8, 4 and 2 bytes past a 16-byte boundary: V follows the less aligned one, the bits follow V."""
    from gespmm_amd import _lib, sddmm

    G = edge
    for H, F in ((4, 8), (3, 24), (7, 6)):
        D1, D2 = _carve(_rand(G["M"], H, F, 3 + H, dtype), off1), _carve(_rand(G["K"], H, F, 4 + F, dtype), off2)
        a = min(_align(D1), _align(D2))
        assert a == min(16 if off1 == 0 else off1 & -off1, 16 if off2 == 0 else off2 & -off2)
        V, W = _vw(F, a)
        for csr in (True, False):
            d = _lib.describe_sddmm_heads(csr, G["M"], G["nnz"], H, F, _align(D1), _align(D2), x16=True)
            assert (d["route"], d["V"], d["W"]) == ("kernel", V, W), (d, V, W)
        o_csr = _run(sddmm.csr_sddmm_heads_x16, G["rp"], G, D1, D2)
        _same(_run(sddmm.coo_sddmm_heads_x16, G["ri"], G, D1, D2), o_csr, ("coo vs csr", H, F, off1, off2))
        _same(o_csr, _per_head(_lib, sddmm, G, D1, D2, V, W), ("per-head calls", H, F, off1, off2, V, W))
        _f64(o_csr, G, D1, D2, "carved H=%d F=%d" % (H, F))


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp16", "bf16"))
def test_composition_route(pkg, edge, monkeypatch, dtype):
    """Pinned (CSR form, not capturing): per head, 16-bit slices, the single-head 16-bit launch, a scatter — the kernel's bits, at every
    alignment class. H = 1 is the single-head call itself ("plain")."""
    from gespmm_amd import _lib, sddmm

    G = edge
    for H, F, off in ((4, 8, 0), (3, 5, 0), (6, 100, 0), (4, 8, 8), (4, 8, 4), (4, 8, 2), (7, 6, 2)):
        D1, D2 = _carve(_rand(G["M"], H, F, 21 + H, dtype), off), _carve(_rand(G["K"], H, F, 22 + F, dtype), off)
        assert _lib.describe_sddmm_heads(True, G["M"], G["nnz"], H, F, _align(D1), _align(D2), x16=True)["route"] == "kernel"
        want = _run(sddmm.csr_sddmm_heads_x16, G["rp"], G, D1, D2)
        monkeypatch.setenv(PIN, "composition")
        d = _lib.describe_sddmm_heads(True, G["M"], G["nnz"], H, F, _align(D1), _align(D2), x16=True)
        assert d["route"] == "composition" and (d["V"], d["W"]) == _vw(F, _align(D1)), d
        _same(_run(sddmm.csr_sddmm_heads_x16, G["rp"], G, D1, D2), want, ("composition", H, F, off))
        # the COO form has no composition: the pin is ignored there
        assert _lib.describe_sddmm_heads(False, G["M"], G["nnz"], H, F, _align(D1), _align(D2), x16=True)["route"] == "kernel"
        _same(_run(sddmm.coo_sddmm_heads_x16, G["ri"], G, D1, D2), want, ("coo under the pin", H, F, off))
        monkeypatch.delenv(PIN)
    D1, D2 = _rand(G["M"], 1, 40, 5, dtype), _rand(G["K"], 1, 40, 6, dtype)
    assert _lib.describe_sddmm_heads(True, G["M"], G["nnz"], 1, 40, x16=True)["route"] == "plain"
    want = sddmm.csr_sddmm(G["rp"], G["ci"], D1[:, 0, :].contiguous(), D2[:, 0, :].contiguous())[:, None]
    _same(_run(sddmm.csr_sddmm_heads_x16, G["rp"], G, D1, D2), want, "H = 1 csr")
    _same(_run(sddmm.coo_sddmm_heads_x16, G["ri"], G, D1, D2), want, "H = 1 coo")


def test_zero_width_and_no_edges(pkg, edge):
    from gespmm_amd import sddmm

    G, dt = edge, torch.bfloat16
    out = torch.full((G["nnz"], 3), float("nan"), device="cuda")
    sddmm.csr_sddmm_heads_x16(G["rp"], G["ci"], torch.empty(G["M"], 3, 0, device="cuda", dtype=dt), torch.empty(G["K"], 3, 0, device="cuda", dtype=dt),
                              out=out)
    assert int((out.view(torch.int32) != 0).sum()) == 0
    rp0 = torch.zeros(8, dtype=torch.int32, device="cuda")
    ci0 = torch.empty(0, dtype=torch.int32, device="cuda")
    assert sddmm.csr_sddmm_heads_x16(rp0, ci0, _rand(7, 3, 6, 1, dt), _rand(4, 3, 6, 2, dt)).shape == (0, 3)
    assert sddmm.coo_sddmm_heads_x16(ci0, ci0, _rand(7, 3, 6, 1, dt), _rand(4, 3, 6, 2, dt)).shape == (0, 3)


def test_python_errors_raise_before_any_launch(pkg, edge):
    from gespmm_amd import sddmm

    G, H, F, dt = edge, 4, 8, torch.float16
    D1, D2 = _rand(G["M"], H, F, 1, dt), _rand(G["K"], H, F, 2, dt)
    out = torch.full((G["nnz"], H), 5.0, device="cuda")
    for f, idx in ((sddmm.csr_sddmm_heads_x16, G["rp"]), (sddmm.coo_sddmm_heads_x16, G["ri"])):
        for bad in (lambda: f(idx, G["ci"], D1.float(), D2.float(), out=out),      # fp32 operands: the other names
                    lambda: f(idx, G["ci"], D1, D2.to(torch.bfloat16), out=out),   # mixed 16-bit dtypes
                    lambda: f(idx, G["ci"], D1, D2.float(), out=out),
                    lambda: f(idx.long(), G["ci"], D1, D2, out=out),
                    lambda: f(idx, G["ci"], D1, D2, out=out.half()),               # the result is fp32
                    lambda: f(idx, G["ci"], None, D2, out=out)):
            with pytest.raises(TypeError):
                bad()
        for bad in (lambda: f(idx, G["ci"], D1.view(G["M"], H * F), D2.view(G["K"], H * F), out=out),  # rank 2
                    lambda: f(idx, G["ci"], D1.transpose(1, 2), D2.transpose(1, 2), out=out),          # not contiguous
                    lambda: f(idx, G["ci"], D1, D2[:, :3].contiguous(), out=out),                      # heads differ
                    lambda: f(idx, G["ci"], D1, D2, out=out[:-1]),
                    lambda: f(idx[:-1], G["ci"], D1, D2, out=out)):
            with pytest.raises(ValueError):
                bad()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    # the fp32 names keep refusing 16-bit tensors
    with pytest.raises(TypeError):
        sddmm.csr_sddmm_heads(G["rp"], G["ci"], D1, D2)
