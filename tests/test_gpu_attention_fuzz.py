"""A seeded sweep of the attention ops over graphs, head counts, widths, operand offsets, slopes and dropout rates nobody hand-picked:
whatever launch geometry the resolvers choose, every op must write every word of its result and nothing behind it, give +0 for empty
rows and columns, stay inside ITS OWN tolerance of the float64 reference (tests/attention_refs.py: the rules are those of the op's
own tests, none is new), repeat its bits, and keep the bit equalities its documentation promises on both sides of every route pin.

The graphs come from ``test_gpu_fuzz.random_csr`` (imported), redrawn until they lie inside the small set of sizes that still crosses
every threshold — M in {1, 2, 7, 63, 64, 65, 300}, K in {1, 5, 64, 333}, hubs of 2049 and 4097 entries (the first sizes past the
long-row threshold of 2048, and two wavefront sweeps) — plus two laws of this file: "lone hub" (one hub row, every other row empty) and
"mean" (a mean degree that lands the softmax's W on 4, 8 or 16, with rows of IT W and IT W + 1 entries: both sides of the register /
sweep boundary). A case holds at most 2^22 words nnz H F; an (H, F) over the cap is redrawn. tests/test_attention_fuzz_host.py asserts,
without a GPU, that the case lists below reach the launch parameters of every family's tables and that every comparison can fail."""
import functools

import numpy as np
import pytest
import torch

import attention_refs as refs
from test_dot_attention_host import SEED, keep_mask
from test_edge_softmax_host import IT, want_W
from test_gpu_fuzz import random_csr

pytestmark = pytest.mark.gpu

MS, KS = (1, 2, 7, 63, 64, 65, 300), (1, 5, 64, 333)
HUBS = (2049, 4097)
HS = (1, 2, 3, 8, 9, 33)
FS = (1, 2, 3, 5, 8, 27, 32, 64, 100, 130, 512)
OFFSETS = (0, 4, 8)
SLOPES = (None, 0.2)
PS = (0.0, 0.25, 0.6)
CAP = 1 << 22
N_CASES = 24
FAMILIES = ("heads", "sddmm", "softmax", "aggregate", "gatv2", "dropout", "dot", "max_arg", "gatv2_attention", "gatv2_x16",
            "gatv2_attention_x16", "dot_x16", "max_arg_x16")
# one seed per family, chosen on the CPU so that the reach conditions of tests/test_attention_fuzz_host.py hold
FAMILY_SEEDS = {"heads": 20261227, "sddmm": 20262022, "softmax": 20263020, "aggregate": 20264032, "gatv2": 20265021,
                "dropout": 20266023, "dot": 20267022, "max_arg": 20268022,
                "gatv2_attention": 20269000, "gatv2_x16": 20270024,
                "gatv2_attention_x16": 20271023, "dot_x16": 20272031, "max_arg_x16": 20273002}
GUARD = 64
NAN = float("nan")
WORST = {}


# ------------------------------------------------------------------------------------------------------------------- the generator

def _pattern(rng, M, K, degs):
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    colind = rng.randint(0, K, size=int(rowptr[-1])).astype(np.int32)
    if rng.rand() < 0.5:
        for r in range(M):
            colind[rowptr[r]:rowptr[r + 1]].sort()
    return {"M": M, "K": K, "nnz": int(rowptr[-1]), "rowptr": rowptr, "colind": colind}


def draw_graph(rng):
    """-> (G, law): a pattern of ``random_csr`` inside the set of sizes, or one of the two laws of this file, with its CSC arrays and
    ``order`` (CSC position i holds CSR entry order[i]) from ``graphs.transpose_csr``."""
    from gespmm_amd import graphs

    u = rng.randint(0, 10)
    if u < 6:
        while True:
            G, law = random_csr(rng)
            if G["M"] in MS and G["K"] in KS and (law != "hub" or int(np.diff(G["rowptr"]).max()) in HUBS):
                break
        G, law = dict(G), str(law)
    else:
        M, K = int(rng.choice(MS)), int(rng.choice(KS))
        if u < 8:
            law = "lone hub"
            degs = np.zeros(M, dtype=np.int64)
            degs[rng.randint(0, M)] = int(rng.choice(HUBS))
        else:
            law = "mean"
            W = int(rng.choice((4, 8, 16)))
            mean = {4: 3, 8: 7, 16: 12}[W]
            degs = rng.randint(0, 2 * mean, size=M)
            if M >= 7:  # rows on both sides of the register / sweep boundary of this W, and an empty one
                at = rng.choice(M, size=3, replace=False)
                degs[at[0]], degs[at[1]], degs[at[2]] = IT * W, IT * W + 1, 0
        G = _pattern(rng, M, K, degs)
    rp, ci = torch.from_numpy(G["rowptr"]), torch.from_numpy(G["colind"])
    colptr, rowind, order = graphs.transpose_csr(rp, ci, G["K"], return_order=True)
    G["colptr"], G["rowind"], G["order"] = colptr.numpy(), rowind.numpy(), order.numpy().astype(np.int32)
    G["degs"] = np.diff(G["rowptr"])
    G["rows"] = refs.rows_of(G["rowptr"])
    return G, law


def draw_case(rng, index=0):
    G, law = draw_graph(rng)
    while True:
        H, F = int(rng.choice(HS)), int(rng.choice(FS))
        if G["nnz"] * H * F <= CAP:
            break
    return {"G": G, "law": law, "H": H, "F": F, "offset": int(rng.choice(OFFSETS)), "slope": SLOPES[int(rng.randint(2))],
            "p": PS[int(rng.randint(3))], "index": index, "seed": int(rng.randint(1 << 30))}


def family_cases(family, n=N_CASES, seed=None):
    rng = np.random.RandomState(FAMILY_SEEDS[family] if seed is None else seed)
    return [draw_case(rng, i) for i in range(n)]


def what(family, c):
    G = c["G"]
    return "%s case %d (seed %d): %s M=%d K=%d nnz=%d H=%d F=%d offset=%d slope=%s p=%s" % (
        family, c["index"], FAMILY_SEEDS[family], c["law"], G["M"], G["K"], G["nnz"], c["H"], c["F"], c["offset"], c["slope"], c["p"])


def align_of(offset):
    return {0: 16, 4: 4, 8: 8}[offset]


# -------------------------------------------------------------------------------------------------------------- operands (host)

def uniform(rng, shape, scale=1.0):
    """fp32, uniform in +-scale / 2"""
    return ((rng.rand(*shape) - 0.5) * scale).astype(np.float32)


def away_from_zero(rng, shape, signs=True):
    """fp32 magnitudes in [0.5, 1), a random sign per word: no word is close to zero (test_dot_attention_host.inputs)."""
    x = rng.uniform(0.5, 1.0, size=shape)
    return (x * rng.choice((-1.0, 1.0), size=shape) if signs else x).astype(np.float32)


def dot_inputs(c):
    """q, k, v, grad_out of a case in the manner of test_dot_attention_host.inputs: scores wide on short rows, narrow on hubs and at
    large F, v with one sign and one amplitude per (column, head)."""
    G, H, F = c["G"], c["H"], c["F"]
    rng = np.random.RandomState(c["seed"])
    q, k, go = away_from_zero(rng, (G["M"], H, F)), away_from_zero(rng, (G["K"], H, F)), away_from_zero(rng, (G["M"], H, F), False)
    amp = np.stack([(0.5 + rng.permutation(G["K"]) / G["K"]) * rng.choice((-1.0, 1.0), size=G["K"]) for _ in range(H)], 1)
    v = (away_from_zero(rng, (G["K"], H, F), False) * amp[:, :, None]).astype(np.float32)
    base = np.where(G["degs"] <= 9, 2.0, np.where(G["degs"] <= 65, 0.8, 0.5)) * min(1.0, 32.0 / F)
    return {"q": (q * base[:, None, None]).astype(np.float32), "k": k, "v": v, "go": go, "scale": float(np.float32(1.0 / np.sqrt(F)))}


def gat_inputs(c):
    """el, er within +-16 (tests/test_gpu_gat_softmax.py), features and grad_out away from zero."""
    G, H, F = c["G"], c["H"], c["F"]
    rng = np.random.RandomState(c["seed"])
    return {"el": uniform(rng, (G["M"], H), 32), "er": uniform(rng, (G["K"], H), 32), "feat": away_from_zero(rng, (G["K"], H, F)) / 2,
            "gout": away_from_zero(rng, (G["M"], H, F)) / 2}


def gatv2_inputs(c):
    """uniform in +-1 (att, grad_score: +-2), as tests/test_gpu_gatv2_score.py draws its real operands"""
    G, H, F = c["G"], c["H"], c["F"]
    rng = np.random.RandomState(c["seed"])
    return {"xl": uniform(rng, (G["M"], H, F), 2), "xr": uniform(rng, (G["K"], H, F), 2), "att": uniform(rng, (H, F), 4),
            "gs": uniform(rng, (G["nnz"], H), 4)}


def gatv2_attention_inputs(c):
    """xl, xr, grad_out uniform in +-1, att uniform in +-2 narrowed by min(1, 8 / F) (a score of F terms stays of the order of one, as
    test_gatv2_attention_host.draw_inputs keeps it); no fl(xl + xr) of an entry is exactly 0 (the branch t >= 0 has no tie)."""
    G, H, F = c["G"], c["H"], c["F"]
    rng = np.random.RandomState(c["seed"])
    x = {"xl": uniform(rng, (G["M"], H, F), 2), "xr": uniform(rng, (G["K"], H, F), 2),
         "att": (uniform(rng, (H, F), 4) * np.float32(min(1.0, 8.0 / F))).astype(np.float32), "go": uniform(rng, (G["M"], H, F), 2)}
    t = (x["xl"][G["rows"]] + x["xr"][G["colind"]]).astype(np.float32)
    assert not (t == 0).any() and np.isfinite(t).all(), "a sum fl(xl + xr) is exactly 0"
    return x


def keep_of(G, H, p):
    """(bool[nnz, H] in CSR order, the kept entries' scale) of the seed pair the dropout tests use"""
    return keep_mask({"rows": G["rows"], "colind": G["colind"]}, H, p)


# ------------------------------------------------------------------------------------------------------------- device helpers

def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _place(t, offset):
    """The values of ``t`` in storage that starts ``offset`` bytes past a 16-byte boundary."""
    skip = offset // t.element_size()
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[skip:skip + t.numel()].view(t.shape)
    v.copy_(t)
    return v


class Out:
    """A result tensor prefilled with NaN (int32: -7) ``offset`` bytes past a 16-byte boundary, guard words before and behind it."""

    def __init__(self, shape, offset=0, dtype=torch.float32):
        n = int(np.prod(shape))
        self.fill = -7 if dtype == torch.int32 else NAN
        self.buf = torch.full((n + 16 + GUARD,), self.fill, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.skip, self.n = offset // self.buf.element_size(), n
        self.t = self.buf[self.skip:self.skip + n].view(*shape)

    def _untouched(self, x):
        return bool((x == self.fill).all()) if self.fill == -7 else bool(torch.isnan(x).all())

    def check(self, msg, written=True):
        assert self._untouched(self.buf[:self.skip]) and self._untouched(self.buf[self.skip + self.n:]), msg + ": guard words were written"
        if written:
            left = int((self.t == self.fill).sum()) if self.fill == -7 else int(torch.isnan(self.t).sum())
            assert left == 0, "%s: %d words were not written" % (msg, left)
        return self.t

    def refill(self):
        self.buf.fill_(self.fill)


def _same(got, want, msg):
    assert got.shape == want.shape and got.dtype == want.dtype, (msg, got.shape, want.shape, got.dtype, want.dtype)
    view = {2: torch.int16, 4: torch.int32}[got.element_size()]
    bad = int((got.contiguous().view(view) != want.contiguous().view(view)).sum())
    assert bad == 0, "%s: %d of %d words differ" % (msg, bad, got.numel())


def _plus_zero(t, mask, msg):
    if mask.any():
        words = t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]).cpu().numpy()[mask]
        assert not words.any(), msg + ": an empty segment is not +0"


def _bound(family, got, ref, scale, msg):
    worst, ok = refs.bound_ratio(got.float().cpu().numpy(), ref, scale)
    WORST[family] = max(WORST.get(family, 0.0), worst)
    assert ok, "%s: worst error / bound %.4g" % (msg, worst)


def _ratio(family, r, msg):
    WORST[family] = max(WORST.get(family, 0.0), r)
    assert r <= 1.0, "%s: worst error / tolerance %.4g" % (msg, r)


def _graph(G):
    return {k: _dev(G[k]) for k in ("rowptr", "colind", "colptr", "rowind", "order", "rows")}


def _seed():
    return _dev(np.array(SEED, dtype=np.uint32).view(np.int32))


def _report(family):
    print("%s: %d cases, worst error / tolerance %.4g" % (family, N_CASES, WORST.get(family, 0.0)))


# ------------------------------------------------------------------------------------------------------------------ 1. heads product

def test_heads_product(pkg, monkeypatch):
    """csr_spmm_heads fp32, with order=, and on bf16 / fp16 features: float64 inside 1e-4 max(|ref|, sum |w b|), the bits of the
    per-head strict-order csr_spmm, of the unordered call on gathered weights, of widen / fp32 entry / narrow; pins on both sides."""
    from gespmm_amd import _lib, spmm

    for pin in ("GESPMM_HEADS_ROUTE", "GESPMM_HEADS_ORDER_ROUTE", "GESPMM_HEADS_X16_ROUTE"):
        monkeypatch.delenv(pin, raising=False)
    for c in family_cases("heads"):
        G, H, F, off, msg = c["G"], c["H"], c["F"], c["offset"], what("heads", c)
        g = _graph(G)
        rng = np.random.RandomState(c["seed"])
        val_h, B_h = uniform(rng, (G["nnz"], H)), uniform(rng, (G["K"], H, F))
        val, B = _place(_dev(val_h), off), _place(_dev(B_h), off)
        perm = _dev(rng.permutation(G["nnz"]).astype(np.int32))
        empty = G["degs"] == 0

        def run(values, dense, order=None, f=spmm.csr_spmm_heads):
            o = Out((G["M"], H, F), off, dense.dtype)
            assert f(g["rowptr"], g["colind"], values, dense, out=o.t, order=order) is o.t
            return o.check(msg)

        out = run(val, B)
        _plus_zero(out, empty, msg)
        ref, mag = refs.heads_float64(G["rows"], G["colind"], G["M"], val_h, B_h)
        _bound("heads", out, ref, mag, msg)
        _same(run(val, B), out, msg + ": second run")
        per_head = torch.stack([spmm.csr_spmm(g["rowptr"], g["colind"], val[:, h].contiguous(), B[:, h, :].contiguous(),
                                              cfg={"flags": _lib.FLAG_STRICT_ORDER}) for h in range(H)], dim=1)
        _same(out, per_head, msg + ": per-head csr_spmm in strict order")
        monkeypatch.setenv("GESPMM_HEADS_ROUTE", "composition")
        _same(run(val, B), out, msg + ": pinned composition")
        monkeypatch.delenv("GESPMM_HEADS_ROUTE")
        # ---- weights through an edge order
        gathered = run(val[perm.long()].contiguous(), B)
        _same(run(val, B, perm), gathered, msg + ": order= vs gathered weights")
        monkeypatch.setenv("GESPMM_HEADS_ORDER_ROUTE", "composition")
        _same(run(val, B, perm), gathered, msg + ": order=, pinned composition")
        monkeypatch.delenv("GESPMM_HEADS_ORDER_ROUTE")
        # ---- 16-bit features: widen, fp32 entry, narrow
        for dtype in (torch.bfloat16, torch.float16):
            B16 = _place(_dev(B_h).to(dtype), off)
            want = spmm.csr_spmm_heads(g["rowptr"], g["colind"], val, B16.float()).to(dtype)
            o16 = run(val, B16, f=spmm.csr_spmm_heads_x16)
            _plus_zero(o16, empty, msg)
            _same(o16, want, "%s: %s vs narrow(fp32(widen))" % (msg, dtype))
            _same(run(val, B16, f=spmm.csr_spmm_heads_x16), o16, msg + ": x16 second run")
            monkeypatch.setenv("GESPMM_HEADS_X16_ROUTE", "composition")
            _same(run(val, B16, f=spmm.csr_spmm_heads_x16), o16, msg + ": x16 pinned composition")
            monkeypatch.delenv("GESPMM_HEADS_X16_ROUTE")
            want_o = spmm.csr_spmm_heads(g["rowptr"], g["colind"], val[perm.long()].contiguous(), B16.float()).to(dtype)
            _same(run(val, B16, perm, f=spmm.csr_spmm_heads_x16), want_o, "%s: %s order=" % (msg, dtype))
    _report("heads")


# ------------------------------------------------------------------------------------------------------------------- 2. heads SDDMM

def sddmm_pinned_shapes(_lib, monkeypatch, G, H, F, align, x16):
    """What the CSR entry reports under each pin (host only), and whether both sides sum in one order: the same V and W."""
    PIN = "GESPMM_SDDMM_HEADS_ROUTE"
    shapes = {}
    for pin in ("kernel", "composition"):
        monkeypatch.setenv(PIN, pin)
        shapes[pin] = _lib.describe_sddmm_heads(True, G["M"], G["nnz"], H, F, align, align, x16=x16)
    monkeypatch.delenv(PIN)
    shapes["same_order"] = all(k in shapes["kernel"] and shapes["kernel"][k] == shapes["composition"].get(k) for k in ("V", "W"))
    return shapes


def test_heads_sddmm(pkg, monkeypatch):
    """csr / coo_sddmm_heads, fp32 and 16-bit operands: float64 inside 1e-4 max(|ref|, sum |d1 d2|), CSR and COO the same bits, the
    kernel the bits of its pinned per-head composition wherever both report the same (V, W)."""
    from gespmm_amd import _lib, sddmm

    PIN = "GESPMM_SDDMM_HEADS_ROUTE"
    monkeypatch.delenv(PIN, raising=False)
    pinned = 0
    for c in family_cases("sddmm"):
        G, H, F, off, msg = c["G"], c["H"], c["F"], c["offset"], what("sddmm", c)
        g = _graph(G)
        rng = np.random.RandomState(c["seed"])
        D1_h, D2_h = away_from_zero(rng, (G["M"], H, F)), away_from_zero(rng, (G["K"], H, F))
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            x16 = dtype != torch.float32
            D1, D2 = _place(_dev(D1_h).to(dtype), off), _place(_dev(D2_h).to(dtype), off)
            f_csr, f_coo = (sddmm.csr_sddmm_heads_x16, sddmm.coo_sddmm_heads_x16) if x16 else (sddmm.csr_sddmm_heads, sddmm.coo_sddmm_heads)

            def run(f, idx):
                o = Out((G["nnz"], H), off)
                assert f(idx, g["colind"], D1, D2, out=o.t) is o.t
                return o.check("%s %s" % (msg, dtype))

            out = run(f_csr, g["rowptr"])
            ref, mag = refs.sddmm_float64(G["rows"], G["colind"], D1.float().cpu().numpy(), D2.float().cpu().numpy())
            _bound("sddmm", out, ref, mag, "%s %s" % (msg, dtype))
            _same(run(f_coo, g["rows"]), out, "%s %s: coo vs csr" % (msg, dtype))
            _same(run(f_csr, g["rowptr"]), out, "%s %s: second run" % (msg, dtype))
            if G["nnz"] == 0:
                continue
            shapes = sddmm_pinned_shapes(_lib, monkeypatch, G, H, F, align_of(off), x16)
            if shapes["same_order"]:
                monkeypatch.setenv(PIN, "kernel")
                by_kernel = run(f_csr, g["rowptr"])
                monkeypatch.setenv(PIN, "composition")
                _same(run(f_csr, g["rowptr"]), by_kernel, "%s %s: kernel vs pinned composition" % (msg, dtype))
                monkeypatch.delenv(PIN)
                _same(out, by_kernel, "%s %s: unpinned vs pinned kernel" % (msg, dtype))
                pinned += shapes["kernel"]["route"] != shapes["composition"]["route"]
    assert pinned > 0, "no case ran the kernel AND its composition at one (V, W)"
    _report("sddmm")


# --------------------------------------------------------------------------------------------------- 3. softmax, GAT softmax, sums

def test_softmax_family(pkg):
    """edge_softmax and its backward inside the derived tolerances; gat_edge_softmax the bits of edge_softmax on the width-2 SDDMM
    score; gat_softmax_stats' m the row maximum (bits) and its sum inside [1, d], exactly 1 on a row of one entry (what
    test_gpu_gat_aggregate.py::test_stats asserts; that the sum is the one the softmax divides by is test_gat_aggregate_and_backward's
    bit comparison with csr_spmm_heads on alpha); the segment sums the bits of the pinned lane order."""
    from gespmm_amd import sddmm, softmax
    from test_gpu_gat_softmax import _check_sum

    for c in family_cases("softmax"):
        G, H, off, slope, msg = c["G"], c["H"], c["offset"], c["slope"], what("softmax", c)
        g = _graph(G)
        nnz = G["nnz"]
        rng = np.random.RandomState(c["seed"])
        s_h, ga_h = uniform(rng, (nnz, H), 64), uniform(rng, (nnz, H), 8)
        el_h, er_h = uniform(rng, (G["M"], H), 32), uniform(rng, (G["K"], H), 32)
        s, ga, el, er = (_place(_dev(x), off) for x in (s_h, ga_h, el_h, er_h))

        def fwd():
            o = Out((nnz, H), off)
            assert softmax.edge_softmax(g["rowptr"], s, out=o.t, negative_slope=slope) is o.t
            return o.check(msg + ": forward")

        def bwd(alpha):
            o = Out((nnz, H), off)
            softmax.edge_softmax_backward(g["rowptr"], alpha, ga, score=s if slope is not None else None, negative_slope=slope, out=o.t)
            return o.check(msg + ": backward")

        alpha = fwd()
        a64, tol = refs.softmax_ref_forward(G["rowptr"], s_h, slope) if nnz else (None, None)
        _ratio("softmax", refs.softmax_worst_ratio(alpha.cpu().numpy(), a64, tol) if nnz else 0.0, msg + ": forward")
        one = G["rowptr"][:-1][G["degs"] == 1]
        assert np.all(alpha.cpu().numpy()[one] == 1.0), msg + ": a single-entry row must be exactly 1"
        grad = bwd(alpha)
        if nnz:
            g64, gtol = refs.softmax_ref_backward(G["rowptr"], alpha.cpu().numpy(), ga_h, s_h, slope)
            _ratio("softmax", refs.softmax_worst_ratio(grad.cpu().numpy(), g64, gtol), msg + ": backward")
        _same(fwd(), alpha, msg + ": forward, second run")
        _same(bwd(alpha), grad, msg + ": backward, second run")
        # ---- the fused add-softmax: the bits of the composition it replaces
        q = torch.stack((el, torch.ones_like(el)), dim=-1)
        k = torch.stack((torch.ones_like(er), er), dim=-1)
        score = sddmm.csr_sddmm_heads(g["rowptr"], g["colind"], q, k)
        _same(score, el[g["rows"].long()] + er[g["colind"].long()], msg + ": the width-2 SDDMM is fl(el + er)")
        o = Out((nnz, H), off)
        softmax.gat_edge_softmax(g["rowptr"], g["colind"], el, er, negative_slope=slope, out=o.t)
        fused = o.check(msg + ": gat_edge_softmax")
        _same(fused, softmax.edge_softmax(g["rowptr"], score, negative_slope=slope), msg + ": gat_edge_softmax vs sddmm + edge_softmax")
        gs, gel = softmax.gat_edge_softmax_backward(g["rowptr"], g["colind"], fused, ga, el=el if slope is not None else None,
                                                    er=er if slope is not None else None, negative_slope=slope)
        _same(gs, softmax.edge_softmax_backward(g["rowptr"], fused, ga, score=score if slope is not None else None, negative_slope=slope),
              msg + ": fused grad_score")
        # ---- statistics
        st = Out((G["M"], H, 2), 8 if off == 8 else 0)
        softmax.gat_softmax_stats(g["rowptr"], g["colind"], el, er, negative_slope=slope, out=st.t)
        stats = st.check(msg + ": stats")
        x = score if slope is None else torch.where(score >= 0, score, score * slope)
        top = torch.full((G["M"], H), -float("inf"), device="cuda")
        if nnz:
            top = top.scatter_reduce(0, g["rows"].long()[:, None].expand(-1, H), x, "amax")
        empty = _dev(G["degs"] == 0)
        top[empty] = 0.0
        _same(stats[:, :, 0].contiguous(), top, msg + ": m is the row maximum of leaky(fl(el + er))")
        _plus_zero(stats, G["degs"] == 0, msg + ": stats")
        d = _dev(G["degs"].astype(np.float32))[:, None]
        den = stats[:, :, 1]
        assert bool((den[~empty] >= 1.0).all()) and bool((den <= d * (1 + 2.0 ** -20)).all()), msg + ": 1 <= s <= d"
        assert bool((den[_dev(G["degs"] == 1)] == 1.0).all()), msg + ": a row of one entry sums exp(0)"
        # ---- segment sums: rows of grad_score (grad_el), columns through csc_order (grad_er)
        W_r, W_c = want_W(G["M"], nnz), want_W(G["K"], nnz)
        sr = Out((G["M"], H), off)
        softmax.edge_segment_sum(g["rowptr"], gs, out=sr.t)
        _same(sr.check(msg + ": row sums"), gel, msg + ": grad_el vs edge_segment_sum(rowptr, grad_score)")
        sums = lambda *a: _check_sum(*a) if nnz else 0.0  # noqa: E731  (the numpy lane order has no form for an array of no rows)
        r1 = sums(sr.t, G["rowptr"], gs.cpu().numpy(), W_r, None, msg + ": row sums")
        sc = Out((G["K"], H), off)
        softmax.edge_segment_sum(g["colptr"], gs, order=g["order"], out=sc.t)
        r2 = sums(sc.check(msg + ": column sums"), G["colptr"], gs.cpu().numpy(), W_c, G["order"], msg + ": column sums")
        _plus_zero(sr.t, G["degs"] == 0, msg + ": row sums")
        _plus_zero(sc.t, np.diff(G["colptr"]) == 0, msg + ": column sums")
        WORST["softmax sums"] = max(WORST.get("softmax sums", 0.0), r1, r2)
    _report("softmax")
    _report("softmax sums")


# ------------------------------------------------------------------------------------------------- 4. GAT aggregate and backward

def _gat_case(c):
    from gespmm_amd import softmax

    G, H, off = c["G"], c["H"], c["offset"]
    g = _graph(G)
    x = gat_inputs(c)
    d = {k: _place(_dev(v), off) for k, v in x.items()}
    st = Out((G["M"], H, 2), 8 if off == 8 else 0)
    softmax.gat_softmax_stats(g["rowptr"], g["colind"], d["el"], d["er"], negative_slope=c["slope"], out=st.t)
    d["stats"] = st.check("stats")
    d["alpha"] = softmax.gat_edge_softmax(g["rowptr"], g["colind"], d["el"], d["er"], negative_slope=c["slope"])
    return g, x, d


def _aggregate_and_backward(family, c, p, monkeypatch):
    """One case of the fused aggregation (both walks) and of the two backward launches, dropout rate p (0: no dropout argument)."""
    from gespmm_amd import sddmm, softmax, spmm

    PIN = "GESPMM_GAT_AGGREGATE_ROUTE"
    monkeypatch.delenv(PIN, raising=False)
    G, H, F, off, slope, msg = c["G"], c["H"], c["F"], c["offset"], c["slope"], what(family, c)
    g, x, d = _gat_case(c)
    keep = ks = drop = None
    alpha = d["alpha"]
    if p:
        keep, ks = keep_of(G, H, p)
        drop = (p, _seed())
        alpha = softmax.edge_dropout(g["rowptr"], g["colind"], alpha, p, drop[1])
    alpha_csc = alpha[g["order"].long()].contiguous()
    empty_r, empty_c = G["degs"] == 0, np.diff(G["colptr"]) == 0

    def aggregate(transposed):
        o = Out((G["K"] if transposed else G["M"], H, F), off)
        ptr, ind = (g["colptr"], g["rowind"]) if transposed else (g["rowptr"], g["colind"])
        r = spmm.gat_aggregate(ptr, ind, d["el"], d["er"], d["stats"], d["gout"] if transposed else d["feat"], negative_slope=slope,
                               transposed=transposed, out=o.t, dropout=drop)
        assert r is o.t
        return o.check("%s: aggregate transposed=%s" % (msg, transposed))

    for transposed in (False, True):
        m2 = "%s: aggregate transposed=%s" % (msg, transposed)
        out = aggregate(transposed)
        _plus_zero(out, empty_c if transposed else empty_r, m2)
        ref, mag = refs.gat_aggregate_float64(G["rows"], G["colind"], G["M"], G["K"], x["el"], x["er"], x["gout"] if transposed else x["feat"],
                                              slope, transposed, keep, ks)
        _bound(family, out, ref, mag, m2)
        want = spmm.csr_spmm_heads(g["colptr"], g["rowind"], alpha_csc, d["gout"]) if transposed else \
            spmm.csr_spmm_heads(g["rowptr"], g["colind"], alpha, d["feat"])
        _same(out, want, m2 + " vs csr_spmm_heads on alpha")
        monkeypatch.setenv(PIN, "composition")
        _same(aggregate(transposed), out, m2 + ", pinned composition")
        monkeypatch.delenv(PIN)
        _same(aggregate(transposed), out, m2 + ", second run")

    def backward():
        outs = [Out((G["M"], H), off), Out((G["M"], H), off), Out((G["K"], H), off)]
        delta, gel, ger = (o.t for o in outs)
        softmax.gat_backward_el(g["rowptr"], g["colind"], d["el"], d["er"], d["stats"], d["gout"], d["feat"], negative_slope=slope,
                                out=(delta, gel), dropout=drop)
        softmax.gat_backward_er(g["colptr"], g["rowind"], d["el"], d["er"], d["stats"], delta, d["gout"], d["feat"], negative_slope=slope,
                                out=ger, dropout=drop)
        return [o.check("%s: %s" % (msg, n)) for o, n in zip(outs, ("delta", "grad_el", "grad_er"))]

    delta, gel, ger = backward()
    _plus_zero(delta, empty_r, msg + ": delta")
    _plus_zero(gel, empty_r, msg + ": grad_el")
    _plus_zero(ger, empty_c, msg + ": grad_er")
    ref_el, ref_er, sc_el, sc_er = refs.gat_backward_float64(G["rows"], G["colind"], G["M"], G["K"], x["el"], x["er"], x["gout"], x["feat"],
                                                             slope, keep, ks)
    _bound(family, gel, ref_el, sc_el, msg + ": grad_el")
    _bound(family, ger, ref_er, sc_er, msg + ": grad_er")
    for u, v, n in zip(backward(), (delta, gel, ger), ("delta", "grad_el", "grad_er")):
        _same(u, v, "%s: %s, second run" % (msg, n))
    # the composition the two launches replace, held to the same bound (its bits are the kernels' only where the dot is exact)
    ga = sddmm.csr_sddmm_heads(g["rowptr"], g["colind"], d["gout"], d["feat"])
    if p:
        ga = softmax.edge_dropout(g["rowptr"], g["colind"], ga, p, drop[1])
    gs, cel = softmax.gat_edge_softmax_backward(g["rowptr"], g["colind"], d["alpha"], ga, el=d["el"] if slope is not None else None,
                                                er=d["er"] if slope is not None else None, negative_slope=slope)
    _bound(family, cel, ref_el, sc_el, msg + ": composition grad_el")
    _bound(family, softmax.edge_segment_sum(g["colptr"], gs, order=g["order"]), ref_er, sc_er, msg + ": composition grad_er")


def test_gat_aggregate_and_backward(pkg, monkeypatch):
    """gat_aggregate in both walks the bits of csr_spmm_heads on alpha (alpha[csc_order]) on both sides of its pin, it and
    gat_backward_el / _er inside 1e-4 max(|ref|, scale) of float64. Every other case runs with its drawn dropout rate."""
    for c in family_cases("aggregate"):
        _aggregate_and_backward("aggregate", c, c["p"] if c["index"] % 2 else 0.0, monkeypatch)
    _report("aggregate")


# ------------------------------------------------------------------------------------------------------------------------ 5. GATv2

def test_gatv2_score_and_backward(pkg):
    """gatv2_score and both passes of its backward inside 1e-4 max(|ref|, sum |terms|) of the float64 restatement."""
    from gespmm_amd import sddmm

    for c in family_cases("gatv2"):
        G, H, F, off, slope, msg = c["G"], c["H"], c["F"], c["offset"], c["slope"], what("gatv2", c)
        g = _graph(G)
        o = gatv2_inputs(c)
        d = {k: _place(_dev(v), off) for k, v in o.items()}
        host = {"rowptr": G["rowptr"], "colind": G["colind"], "colptr_h": G["colptr"], "rowind_h": G["rowind"], "order_h": G["order"]}
        (score, terms), row, col = refs.gatv2_float64(host, o, slope)

        def run():
            outs = [Out((G["nnz"], H), off), Out((G["M"], H, F), off), Out((G["M"], H, F), off), Out((G["K"], H, F), off)]
            sddmm.gatv2_score(g["rowptr"], g["colind"], d["xl"], d["xr"], d["att"], negative_slope=slope, out=outs[0].t)
            sddmm.gatv2_score_backward(g["rowptr"], g["colind"], d["gs"], d["xl"], d["xr"], d["att"], negative_slope=slope, want_att_part=True,
                                       out=(outs[1].t, outs[2].t))
            sddmm.gatv2_score_backward(g["colptr"], g["rowind"], d["gs"], d["xr"], d["xl"], d["att"], negative_slope=slope, order=g["order"],
                                       out=outs[3].t)
            return [x.check("%s: %s" % (msg, n)) for x, n in zip(outs, ("score", "grad_xl", "att_part", "grad_xr"))]

        got = run()
        for t, ref, tm, n in zip(got, (score, row[0], row[1], col[0]), (terms, row[2], row[3], col[2]), ("score", "grad_xl", "att_part", "grad_xr")):
            _ratio("gatv2", refs.gatv2_worst_ratio(t.cpu().numpy(), ref, tm, n), "%s: %s" % (msg, n))
        _plus_zero(got[1], G["degs"] == 0, msg + ": grad_xl")
        _plus_zero(got[2], G["degs"] == 0, msg + ": att_part")
        _plus_zero(got[3], np.diff(G["colptr"]) == 0, msg + ": grad_xr")
        for u, v, n in zip(run(), got, ("score", "grad_xl", "att_part", "grad_xr")):
            _same(u, v, "%s: %s, second run" % (msg, n))
    _report("gatv2")


# ----------------------------------------------------------------------------------------------------------------- 6. edge dropout

def test_edge_dropout(pkg, monkeypatch):
    """edge_dropout the bits of the numpy mask (p = 0: the bits of x), in place too; the fused forms with the drawn rate (never 0 here)
    against the compositions with edge_dropout in them and float64 with the restated mask."""
    from gespmm_amd import softmax

    for c in family_cases("dropout"):
        G, H, off, msg = c["G"], c["H"], c["offset"], what("dropout", c)
        g = _graph(G)
        rng = np.random.RandomState(c["seed"])
        x_h = uniform(rng, (G["nnz"], H), 4)
        x = _place(_dev(x_h), off)
        for p in PS:
            keep, ks = keep_of(G, H, p)
            want = np.where(keep, x_h * ks, np.float32(0.0)).astype(np.float32) if p else x_h
            o = Out((G["nnz"], H), off)
            assert softmax.edge_dropout(g["rowptr"], g["colind"], x, p, _seed(), out=o.t) is o.t
            got = o.check("%s: p=%g" % (msg, p))
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), "%s: p=%g differs from the restated mask" % (msg, p)
            y = _place(x, off)
            softmax.edge_dropout(g["rowptr"], g["colind"], y, p, _seed(), out=y)
            _same(y, got, "%s: p=%g in place" % (msg, p))
        _aggregate_and_backward("dropout", c, c["p"] or 0.25, monkeypatch)
    _report("dropout")


# --------------------------------------------------------------------------------------------------------------- 7. dot attention

def _dot_run(g, x, offset, drop, small=None, stored=None):
    """The three launches, every dense operand and result ``offset`` bytes off a 16-byte boundary; small: the offsets of (stats, delta)
    where they are not the family's own (8 or 0, ``offset``); stored: a 16-bit type — the row pass is fed out rounded once to it."""
    from gespmm_amd import attention

    q, k, v, go = (_place(_dev(x[n]), offset) for n in ("q", "k", "v", "go"))
    M, H, F = x["q"].shape
    K = x["k"].shape[0]
    at_stats, at_delta = small or (8 if offset == 8 else 0, offset)
    o = {"out": Out((M, H, F), offset), "stats": Out((M, H, 2), at_stats), "delta": Out((M, H), at_delta),
         "grad_q": Out((M, H, F), offset), "grad_k": Out((K, H, F), offset), "grad_v": Out((K, H, F), offset)}
    attention.dot_attention(g["rowptr"], g["colind"], q, k, v, scale=x["scale"], dropout=drop, out=o["out"].t, stats=o["stats"].t)
    fed = o["out"].t if stored is None else _place(o["out"].t.to(stored).float(), offset)
    attention.dot_attention_backward_q(g["rowptr"], g["colind"], q, k, v, o["stats"].t, fed, go, scale=x["scale"], dropout=drop,
                                       results=(o["delta"].t, o["grad_q"].t))
    attention.dot_attention_backward_kv(g["colptr"], g["rowind"], q, k, v, o["stats"].t, o["delta"].t, go, scale=x["scale"], dropout=drop,
                                        results=(o["grad_k"].t, o["grad_v"].t))
    return o


def test_dot_attention(pkg):
    """The three launches inside the derived tolerances of test_dot_attention_host.py, with and without dropout; a head the bits of
    the single-head call on its slices."""
    for c in family_cases("dot"):
        G, H, F, off, p, msg = c["G"], c["H"], c["F"], c["offset"], c["p"], what("dot", c)
        g = _graph(G)
        x = dot_inputs(c)
        keep = ks = drop = None
        if p:
            (keep, ks), drop = keep_of(G, H, p), (p, _seed())
        o = _dot_run(g, x, off, drop)
        got = {n: v.check("%s: %s" % (msg, n)) for n, v in o.items()}
        h = {n: t.cpu().numpy() for n, t in got.items()}
        r = refs.dot_check_all(G, x, h, keep, ks, what=msg)
        _ratio("dot", max(r.values()), "%s: %r" % (msg, r))
        empty_r, empty_c = G["degs"] == 0, np.diff(G["colptr"]) == 0
        for n in ("out", "stats", "delta", "grad_q"):
            _plus_zero(got[n], empty_r, "%s: %s" % (msg, n))
        for n in ("grad_k", "grad_v"):
            _plus_zero(got[n], empty_c, "%s: %s" % (msg, n))
        if not p:
            one = np.nonzero(G["degs"] == 1)[0]
            assert h["out"][one].tobytes() == x["v"][G["colind"][G["rowptr"][one]]].tobytes(), msg + ": a single-entry row is its neighbour's v"
            assert np.all(h["stats"][one, :, 1] == 1.0), msg
        again = _dot_run(g, x, off, drop)
        for n in got:
            _same(again[n].t, got[n], "%s: %s, second run" % (msg, n))
        for hd in sorted({0, H - 1}) if H > 1 and not p else ():  # (with dropout the single-head call would draw head 0's mask)
            xs = {n: np.ascontiguousarray(x[n][:, hd:hd + 1]) for n in ("q", "k", "v", "go")}
            xs["scale"] = x["scale"]
            single = _dot_run(g, xs, off, None)
            for n in got:
                _same(got[n][:, hd:hd + 1].contiguous(), single[n].t, "%s: head %d of %s is the single-head call" % (msg, hd, n))
    _report("dot")


# ------------------------------------------------------------------------------------------------------------------ 8. max reducer

def test_max_arg_and_backward(pkg):
    """csr_spmm_max_arg and its backward, bit for bit against the host restatement of the two chains (width N = H F), on integers (ties
    everywhere) and on floats with planted zeros of both signs and NaN; C the bits of csr_spmm_max on an operand that holds +0 only."""
    from gespmm_amd import spmm

    for c in family_cases("max_arg"):
        G, N, off, msg = c["G"], c["H"] * c["F"], c["offset"], what("max_arg", c)
        g = _graph(G)
        rng = np.random.RandomState(c["seed"])
        grad_h = rng.standard_normal((G["M"], N)).astype(np.float32)
        grad = _place(_dev(grad_h), off)
        for kind in ("ints", "floats", "positive"):
            if kind == "ints":
                B_h = rng.randint(-2, 3, size=(G["K"], N)).astype(np.float32)
            elif kind == "floats":
                B_h = rng.standard_normal((G["K"], N)).astype(np.float32)
                for value in (0.0, -0.0, np.nan, -20000.0):
                    B_h[rng.rand(G["K"], N) < 0.04] = np.float32(value)
            else:
                B_h = np.abs(rng.standard_normal((G["K"], N))).astype(np.float32)
            want_C, want_arg = refs.max_arg_forward(G["rowptr"], G["colind"], B_h, -10000.0)
            B = _place(_dev(B_h), off)

            def forward():
                oc, oa = Out((G["M"], N), off), Out((G["M"], N), off, torch.int32)
                spmm.csr_spmm_max_arg(g["rowptr"], g["colind"], B, out=oc.t, arg=oa.t)
                return oc.check("%s %s: C" % (msg, kind)), oa.check("%s %s: arg" % (msg, kind))

            C, arg = forward()
            assert np.array_equal(arg.cpu().numpy(), want_arg), "%s %s: arg" % (msg, kind)
            assert np.array_equal(C.cpu().numpy().view(np.uint32), want_C.view(np.uint32)), "%s %s: C" % (msg, kind)
            C2, arg2 = forward()
            _same(C2, C, "%s %s: C, second run" % (msg, kind))
            _same(arg2, arg, "%s %s: arg, second run" % (msg, kind))
            if kind == "positive":
                _same(C, spmm.csr_spmm_max(g["rowptr"], g["colind"], _dev(B_h)), "%s: C vs csr_spmm_max" % msg)

            def backward():
                ob = Out((G["K"], N), off)
                spmm.csr_spmm_max_backward(g["colptr"], g["rowind"], g["order"], arg, grad, G["K"], out=ob.t)
                return ob.check("%s %s: grad_B" % (msg, kind))

            gB = backward()
            want_g = refs.max_backward(G["colptr"], G["rowind"], G["order"], want_arg, grad_h, G["K"])
            assert np.array_equal(gB.cpu().numpy().view(np.uint32), want_g.view(np.uint32)), "%s %s: grad_B" % (msg, kind)
            _same(backward(), gB, "%s %s: grad_B, second run" % (msg, kind))
    print("max_arg: %d cases, every comparison on bits" % N_CASES)


# ------------------------------------------------------------------------------------------------------- 9. fused GATv2 attention

RESULTS_V2 = ("out", "stats", "delta", "grad_xl", "att_part", "grad_xr")


def _gatv2_attention_run(g, x, offset, slope, drop, want=True, small=None, stored=None):
    """The three launches, every dense operand and result ``offset`` bytes off a 16-byte boundary (stats: 8 or 0) -> (results, placed
    operands). want=False: the row pass without att_part; its buffer stays as it was poisoned. small: the offsets of (stats, delta)
    where they are not the family's own; stored: a 16-bit type — the row pass is fed out rounded once to it."""
    from gespmm_amd import attention

    xl, xr, att, go = (_place(_dev(x[n]), offset) for n in ("xl", "xr", "att", "go"))
    M, H, F = x["xl"].shape
    K = x["xr"].shape[0]
    at_stats, at_delta = small or (8 if offset == 8 else 0, offset)
    o = {"out": Out((M, H, F), offset), "stats": Out((M, H, 2), at_stats), "delta": Out((M, H), at_delta),
         "grad_xl": Out((M, H, F), offset), "att_part": Out((M, H, F), offset), "grad_xr": Out((K, H, F), offset)}
    attention.gatv2_attention(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope, dropout=drop, out=o["out"].t, stats=o["stats"].t)
    row = (o["delta"].t, o["grad_xl"].t, o["att_part"].t)
    fed = o["out"].t if stored is None else _place(o["out"].t.to(stored).float(), offset)
    attention.gatv2_attention_backward_row(g["rowptr"], g["colind"], xl, xr, att, o["stats"].t, fed, go, negative_slope=slope,
                                           dropout=drop, want_att_part=want, results=row if want else row[:2])
    attention.gatv2_attention_backward_col(g["colptr"], g["rowind"], xl, xr, att, o["stats"].t, o["delta"].t, go, negative_slope=slope,
                                           dropout=drop, result=o["grad_xr"].t)
    return o, (xl, xr, att)


def test_gatv2_attention(pkg):
    """gatv2_attention and its two backward passes inside the derived tolerances of test_gatv2_attention_host.py, with and without
    dropout; m of the stats the bits of the row maximum of sddmm.gatv2_score at the same alignment; a single-entry row its neighbour's
    xr; a head the bits of the single-head call on its slices; the row pass without att_part the bits of the one with it."""
    from gespmm_amd import sddmm

    for c in family_cases("gatv2_attention"):
        G, H, F, off, slope, p, msg = c["G"], c["H"], c["F"], c["offset"], c["slope"], c["p"], what("gatv2_attention", c)
        g = _graph(G)
        x = gatv2_attention_inputs(c)
        keep = ks = drop = None
        if p:
            (keep, ks), drop = keep_of(G, H, p), (p, _seed())
        o, (xl, xr, att) = _gatv2_attention_run(g, x, off, slope, drop)
        got = {n: v.check("%s: %s" % (msg, n)) for n, v in o.items()}
        h = {n: t.cpu().numpy() for n, t in got.items()}
        r = refs.gatv2_attention_check_all(G, x, slope, h, keep, ks, what=msg)
        _ratio("gatv2_attention", max(r.values()), "%s: %r" % (msg, r))
        empty_r, empty_c = G["degs"] == 0, np.diff(G["colptr"]) == 0
        for n in ("out", "stats", "delta", "grad_xl", "att_part"):
            _plus_zero(got[n], empty_r, "%s: %s" % (msg, n))
        _plus_zero(got["grad_xr"], empty_c, msg + ": grad_xr")
        # ---- m: the row maximum of the score kernel's bits, on the very operands (one alignment: one (V, W), one lane order)
        score = sddmm.gatv2_score(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope)
        top = torch.full((G["M"], H), -float("inf"), device="cuda")
        if G["nnz"]:
            top = top.scatter_reduce(0, g["rows"].long()[:, None].expand(-1, H), score, "amax")
        top[_dev(empty_r)] = 0.0
        _same(got["stats"][:, :, 0].contiguous(), top, msg + ": m is the row maximum of gatv2_score")
        if not p:
            one = np.nonzero(G["degs"] == 1)[0]
            assert h["out"][one].tobytes() == x["xr"][G["colind"][G["rowptr"][one]]].tobytes(), msg + ": a single-entry row is its neighbour's xr"
            assert np.all(h["stats"][one, :, 1] == 1.0), msg + ": a single-entry row has l = 1"
        again, _ = _gatv2_attention_run(g, x, off, slope, drop)
        for n in got:
            _same(again[n].check("%s: %s, second run" % (msg, n)), got[n], "%s: %s, second run" % (msg, n))
        for hd in sorted({0, H - 1}) if H > 1 and not p else ():  # (with dropout the single-head call would draw head 0's mask)
            xs = {n: np.ascontiguousarray(x[n][:, hd:hd + 1]) for n in ("xl", "xr", "go")}
            xs["att"] = np.ascontiguousarray(x["att"][hd:hd + 1])
            single, _ = _gatv2_attention_run(g, xs, off, slope, None)
            for n in got:
                _same(got[n][:, hd:hd + 1].contiguous(), single[n].t, "%s: head %d of %s is the single-head call" % (msg, hd, n))
        if c["index"] % 2:
            bare, _ = _gatv2_attention_run(g, x, off, slope, drop, want=False)
            for n in ("delta", "grad_xl"):
                _same(bare[n].check("%s: %s without att_part" % (msg, n)), got[n], "%s: %s without att_part" % (msg, n))
            assert bare["att_part"]._untouched(bare["att_part"].buf), msg + ": want_att_part=False wrote into the poisoned buffer"
    _report("gatv2_attention")


# ----------------------------------------------------------------------------------------------- 10. GATv2 score on 16-bit operands

def x16_aligns(offset, extra=0):
    """(alignment of the 16-bit operands, alignment of the fp32 ones) in bytes: both ``offset`` bytes off a 16-byte boundary, the 16-bit
    ones ``extra`` (0 or 2) bytes further."""
    return (2 if extra else align_of(offset)), align_of(offset)


def test_gatv2_x16(pkg):
    """gatv2_score_x16 inside 1e-4 max(|ref|, sum |terms|) of the float64 restatement on the widened operands and on the bits of
    sddmm.gatv2_score wherever both describe calls answer one (V, W); both passes of gatv2_score_backward_x16 on the bits of the fp32
    backward on the widened operands (grad_x narrowed once), again with the 16-bit operands 2 bytes further off (V = 1)."""
    from gatv2_x16_cases import narrow
    from gespmm_amd import _lib, sddmm

    shared = 0
    for c in family_cases("gatv2_x16"):
        G, H, F, off, slope = c["G"], c["H"], c["F"], c["offset"], c["slope"]
        g = _graph(G)
        o = gatv2_inputs(c)
        att, gs = _place(_dev(o["att"]), off), _place(_dev(o["gs"]), off)
        empty_r, empty_c = G["degs"] == 0, np.diff(G["colptr"]) == 0
        for dtype in (torch.bfloat16, torch.float16):
            msg = "%s %s" % (what("gatv2_x16", c), dtype)
            (xl16, xl_w), (xr16, xr_w) = narrow(o["xl"], dtype), narrow(o["xr"], dtype)
            ref, terms = refs.gatv2_restate_score(G["rowptr"], G["colind"], xl_w, xr_w, o["att"], slope)
            # ---- the fp32 kernels on the exact widening, operands at the same offset
            wl, wr = _place(_dev(xl_w), off), _place(_dev(xr_w), off)
            score32 = sddmm.gatv2_score(g["rowptr"], g["colind"], wl, wr, att, negative_slope=slope)
            gxl32, part32 = sddmm.gatv2_score_backward(g["rowptr"], g["colind"], gs, wl, wr, att, negative_slope=slope, want_att_part=True)
            gxr32 = sddmm.gatv2_score_backward(g["colptr"], g["rowind"], gs, wr, wl, att, negative_slope=slope, order=g["order"])
            want = (gxl32.to(dtype), part32, gxr32.to(dtype))
            for extra in (0, 2):
                m2 = "%s, 16-bit operands %d bytes off" % (msg, off + extra)
                xl, xr = _place(xl16.cuda(), off + extra), _place(xr16.cuda(), off + extra)
                assert xl.data_ptr() % 16 == off + extra and att.data_ptr() % 16 == off

                def run():
                    outs = [Out((G["nnz"], H), off), Out((G["M"], H, F), off + extra, dtype), Out((G["M"], H, F), off),
                            Out((G["K"], H, F), off + extra, dtype)]
                    sddmm.gatv2_score_x16(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope, out=outs[0].t)
                    sddmm.gatv2_score_backward_x16(g["rowptr"], g["colind"], gs, xl, xr, att, negative_slope=slope, want_att_part=True,
                                                   out=(outs[1].t, outs[2].t))
                    sddmm.gatv2_score_backward_x16(g["colptr"], g["rowind"], gs, xr, xl, att, negative_slope=slope, order=g["order"],
                                                   out=outs[3].t)
                    return [t.check("%s: %s" % (m2, n)) for t, n in zip(outs, ("score", "grad_xl", "att_part", "grad_xr"))]

                score, gxl, part, gxr = run()
                _ratio("gatv2_x16", refs.gatv2_worst_ratio(score.cpu().numpy(), ref, terms, "score"), m2 + ": score")
                if G["nnz"]:
                    xa, fa = x16_aligns(off, extra)
                    d16 = _lib.describe_gatv2_score(G["M"], G["nnz"], H, F, xa, xa, fa, x16=True)
                    d32 = _lib.describe_gatv2_score(G["M"], G["nnz"], H, F, fa, fa, fa)
                    if (d16["V"], d16["W"]) == (d32["V"], d32["W"]):
                        _same(score, score32, m2 + ": score against the fp32 kernel at one (V, W)")
                        shared += not extra
                for t, w, n in zip((gxl, part, gxr), want, ("grad_xl", "att_part", "grad_xr")):
                    _same(t, w, "%s: %s against the fp32 backward on the widened operands" % (m2, n))
                _plus_zero(gxl, empty_r, m2 + ": grad_xl")
                _plus_zero(part, empty_r, m2 + ": att_part")
                _plus_zero(gxr, empty_c, m2 + ": grad_xr")
                if not extra:
                    for u, v, n in zip(run(), (score, gxl, part, gxr), ("score", "grad_xl", "att_part", "grad_xr")):
                        _same(u, v, "%s: %s, second run" % (m2, n))
    assert shared > 0, "no case compared the 16-bit score with the fp32 kernel's bits"
    _report("gatv2_x16")


# ------------------------------------------------------------------- 11, 12. the fused GATv2 and dot-product attention on 16-bit operands

X16_DTYPES = (torch.bfloat16, torch.float16)
X16_IDS = ("bf16", "fp16")
RESULTS_DOT = ("out", "stats", "delta", "grad_q", "grad_k", "grad_v")
NARROW_V2, NARROW_DOT = ("out", "grad_xl", "grad_xr"), ("out", "grad_q", "grad_k", "grad_v")  # the 16-bit results; the others are fp32


def x16_offsets(offset, extra=0):
    """(offset of the 16-bit operands and results, offset of the fp32 oracle's tensors — and of the 16-bit run's fp32 att and att_part)
    in bytes past a 16-byte boundary: a 16-bit operand b bytes off is an fp32 operand 2 b bytes off."""
    return offset + extra, (2 * (offset + extra)) % 16


def align_at(offset):
    """The alignment in bytes, capped at 16, of an address ``offset`` bytes past a 16-byte boundary."""
    return 16 if offset % 16 == 0 else offset & -offset


def gatv2_attention_x16_inputs(c, dtype):
    """``gatv2_attention_inputs`` with xl, xr and grad_out rounded to ``dtype`` AFTER the call (widened fp32 arrays; att stays fp32): the
    fp32 family's assertion that no fl(xl + xr) is exactly 0 stays where it is, on the unrounded draw, and cannot be asked of the rounded
    operands — sums of 16-bit values cancel exactly in hundreds of words a case. A sum of two 16-bit values is zero in fp32 exactly when
    it is zero exactly, and the kernels (``!(t >= 0.0f)``) and the float64 reference (``t >= 0``) both take the non-negative branch
    there: a tie is a legitimate input, and only finiteness is asserted."""
    x = gatv2_attention_inputs(c)
    x = dict(x, **{n: refs.rounded(x[n], dtype) for n in ("xl", "xr", "go")})
    assert all(np.isfinite(x[n]).all() for n in ("xl", "xr", "go", "att"))
    return x


def dot_x16_inputs(c, dtype):
    """``dot_inputs`` with q, k, v and grad_out rounded to ``dtype`` (widened fp32 arrays); the fp32 scale is untouched."""
    x = dot_inputs(c)
    x = dict(x, **{n: refs.rounded(x[n], dtype) for n in ("q", "k", "v", "go")})
    assert all(np.isfinite(x[n]).all() for n in ("q", "k", "v", "go"))
    return x


def _gatv2_attention_x16_run(g, x, dtype, at16, at32, small, slope, drop, want=True):
    """The three 16-bit launches: xl, xr, grad_out, out, grad_xl and grad_xr ``at16`` bytes off a 16-byte boundary, att and att_part
    ``at32``, (stats, delta) at ``small`` -> results. want=False: the row pass without att_part; its buffer stays as it was poisoned."""
    from gespmm_amd import attention

    xl, xr, go = (_place(_dev(x[n]).to(dtype), at16) for n in ("xl", "xr", "go"))
    att = _place(_dev(x["att"]), at32)
    M, H, F = x["xl"].shape
    K = x["xr"].shape[0]
    o = {"out": Out((M, H, F), at16, dtype), "stats": Out((M, H, 2), small[0]), "delta": Out((M, H), small[1]),
         "grad_xl": Out((M, H, F), at16, dtype), "att_part": Out((M, H, F), at32), "grad_xr": Out((K, H, F), at16, dtype)}
    for t in (xl, xr, go, o["out"].t, o["grad_xl"].t, o["grad_xr"].t):
        assert t.data_ptr() % 16 == at16
    assert att.data_ptr() % 16 == at32 == o["att_part"].t.data_ptr() % 16
    assert o["stats"].t.data_ptr() % 16 == small[0] and o["delta"].t.data_ptr() % 16 == small[1]
    attention.gatv2_attention_x16(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope, dropout=drop, out=o["out"].t, stats=o["stats"].t)
    row = (o["delta"].t, o["grad_xl"].t, o["att_part"].t)
    attention.gatv2_attention_backward_row_x16(g["rowptr"], g["colind"], xl, xr, att, o["stats"].t, o["out"].t, go, negative_slope=slope,
                                               dropout=drop, want_att_part=want, results=row if want else row[:2])
    attention.gatv2_attention_backward_col_x16(g["colptr"], g["rowind"], xl, xr, att, o["stats"].t, o["delta"].t, go, negative_slope=slope,
                                               dropout=drop, result=o["grad_xr"].t)
    return o


def _dot_x16_run(g, x, dtype, at16, small, drop):
    """The three 16-bit launches: q, k, v, grad_out, out, grad_q, grad_k and grad_v ``at16`` bytes off a 16-byte boundary, (stats, delta)
    at ``small`` -> results."""
    from gespmm_amd import attention

    q, k, v, go = (_place(_dev(x[n]).to(dtype), at16) for n in ("q", "k", "v", "go"))
    M, H, F = x["q"].shape
    K = x["k"].shape[0]
    o = {"out": Out((M, H, F), at16, dtype), "stats": Out((M, H, 2), small[0]), "delta": Out((M, H), small[1]),
         "grad_q": Out((M, H, F), at16, dtype), "grad_k": Out((K, H, F), at16, dtype), "grad_v": Out((K, H, F), at16, dtype)}
    for t in (q, k, v, go, o["out"].t, o["grad_q"].t, o["grad_k"].t, o["grad_v"].t):
        assert t.data_ptr() % 16 == at16
    assert o["stats"].t.data_ptr() % 16 == small[0] and o["delta"].t.data_ptr() % 16 == small[1]
    attention.dot_attention_x16(g["rowptr"], g["colind"], q, k, v, scale=x["scale"], dropout=drop, out=o["out"].t, stats=o["stats"].t)
    attention.dot_attention_backward_q_x16(g["rowptr"], g["colind"], q, k, v, o["stats"].t, o["out"].t, go, scale=x["scale"], dropout=drop,
                                           results=(o["delta"].t, o["grad_q"].t))
    attention.dot_attention_backward_kv_x16(g["colptr"], g["rowind"], q, k, v, o["stats"].t, o["delta"].t, go, scale=x["scale"], dropout=drop,
                                            results=(o["grad_k"].t, o["grad_v"].t))
    return o


def _x16_common(family, c, dtype, names, narrow, column, run, oracle, describe, single, check64, neighbour, extra_checks=None):
    """What the two 16-bit attention families share, per case: two passes — the 16-bit operands and results ``c["offset"]`` bytes off a
    16-byte boundary, then 2 bytes further (V = 1) — each written and guarded, +0 on empty rows (``column``: on empty columns), on the
    bits of the fp32 entry points on the widened operands carved at twice the offset (the 16-bit results narrowed once), at one (V, W)
    by both describe calls (a mismatch fails: nothing is skipped); stats at 8 bytes off where the case's offset is 8, delta at the
    case's offset, in both runs; on the first pass inside the derived tolerances of float64 plus the one rounding of a 16-bit store,
    the same bits in a second run, and, without dropout, a single-entry row its neighbour's value and heads 0 and H - 1 the bits of
    the single-head call."""
    G, H, off, p = c["G"], c["H"], c["offset"], c["p"]
    g = _graph(G)
    keep = ks = drop = None
    if p:
        (keep, ks), drop = keep_of(G, H, p), (p, _seed())
    small = (8 if off == 8 else 0, off)
    empty_r, empty_c = G["degs"] == 0, np.diff(G["colptr"]) == 0
    for extra in (0, 2):
        at16, at32 = x16_offsets(off, extra)
        msg = "%s %s, 16-bit operands %d bytes off" % (what(family, c), dtype, at16)
        o = run(g, at16, at32, small, drop)
        got = {n: o[n].check("%s: %s" % (msg, n)) for n in names}
        for n in names:
            _plus_zero(got[n], empty_c if n in column else empty_r, "%s: %s" % (msg, n))
        # ---- the bits of the fp32 entry points on the widened operands
        want, placed = oracle(g, at32, small, drop)
        if G["nnz"]:
            d16, d32 = describe(align_at(at16), align_at(at32), True), describe(align_at(at32), align_at(at32), False)
            assert {k: d16[k] for k in ("V", "W")} == {k: d32[k] for k in ("V", "W")}, "%s: %r on 16-bit, %r on fp32" % (msg, d16, d32)
            assert extra == 0 or d16["V"] == 1, (msg, d16)
        for n in names:
            w = want[n].check("%s: fp32 %s" % (msg, n))
            _same(got[n], w.to(dtype) if n in narrow else w, "%s: %s against the fp32 entry point%s" % (msg, n, " narrowed once" if n in narrow else ""))
        if extra_checks is not None:
            extra_checks(g, at16, at32, small, drop, got, placed, msg)
        if extra:
            continue
        # ---- float64, the derived tolerances plus the one rounding of a 16-bit store
        h = {n: t.float().cpu().numpy() for n, t in got.items()}
        r = check64(h, keep, ks, msg)
        _ratio("%s %s" % (family, X16_IDS[X16_DTYPES.index(dtype)]), max(r.values()), "%s: %r" % (msg, r))
        if not p:
            one = np.nonzero(G["degs"] == 1)[0]
            assert _bits16(got["out"][_dev(one).long()]) == _bits16(_dev(neighbour[G["colind"][G["rowptr"][one]]]).to(dtype)), \
                msg + ": a single-entry row is its neighbour's value"
            assert np.all(h["stats"][one, :, 1] == 1.0), msg + ": a single-entry row has l = 1"
        again = run(g, at16, at32, small, drop)
        for n in names:
            _same(again[n].check("%s: %s, second run" % (msg, n)), got[n], "%s: %s, second run" % (msg, n))
        for hd in sorted({0, H - 1}) if H > 1 and not p else ():  # (with dropout the single-head call would draw head 0's mask)
            alone = single(hd)(g, at16, at32, small, None)
            for n in names:
                _same(got[n][:, hd:hd + 1].contiguous(), alone[n].check("%s: head %d of %s alone" % (msg, hd, n)),
                      "%s: head %d of %s is the single-head call" % (msg, hd, n))


def _bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().tobytes()


@pytest.mark.parametrize("dtype", X16_DTYPES, ids=X16_IDS)
def test_gatv2_attention_x16(pkg, dtype):
    """gatv2_attention_x16 and its two backward passes on bf16 / fp16 node terms (``_x16_common``): att and att_part (fp32) at the fp32
    oracle's offset, so that both describe calls answer one V; m of the stats the bits of the row maximum of sddmm.gatv2_score on the
    widened operands at the oracle's offset; on every odd case the row pass without att_part the bits of the one with it, the poisoned
    buffer untouched. Exact zeros of fl(xl + xr) are in the inputs (``gatv2_attention_x16_inputs``)."""
    from gespmm_amd import _lib, sddmm

    family = "gatv2_attention_x16"
    for c in family_cases(family):
        G, H, F, slope = c["G"], c["H"], c["F"], c["slope"]
        x = gatv2_attention_x16_inputs(c, dtype)

        def head(hd):
            xs = {n: np.ascontiguousarray(x[n][:, hd:hd + 1]) for n in ("xl", "xr", "go")}
            xs["att"] = np.ascontiguousarray(x["att"][hd:hd + 1])
            return lambda g, at16, at32, small, drop: _gatv2_attention_x16_run(g, xs, dtype, at16, at32, small, slope, drop)

        def extras(g, at16, at32, small, drop, got, placed, msg):
            xl, xr, att = placed
            score = sddmm.gatv2_score(g["rowptr"], g["colind"], xl, xr, att, negative_slope=slope)
            top = torch.full((G["M"], H), -float("inf"), device="cuda")
            if G["nnz"]:
                top = top.scatter_reduce(0, g["rows"].long()[:, None].expand(-1, H), score, "amax")
            top[_dev(G["degs"] == 0)] = 0.0
            _same(got["stats"][:, :, 0].contiguous(), top, msg + ": m is the row maximum of gatv2_score on the widened operands")
            if c["index"] % 2:
                bare = _gatv2_attention_x16_run(g, x, dtype, at16, at32, small, slope, drop, want=False)
                for n in ("delta", "grad_xl"):
                    _same(bare[n].check("%s: %s without att_part" % (msg, n)), got[n], "%s: %s without att_part" % (msg, n))
                assert bare["att_part"]._untouched(bare["att_part"].buf), msg + ": want_att_part=False wrote into the poisoned buffer"

        _x16_common(
            family, c, dtype, RESULTS_V2, NARROW_V2, ("grad_xr",),
            run=lambda g, at16, at32, small, drop: _gatv2_attention_x16_run(g, x, dtype, at16, at32, small, slope, drop),
            oracle=lambda g, at32, small, drop: _gatv2_attention_run(g, x, at32, slope, drop, small=small, stored=dtype),
            describe=lambda xa, fa, x16: _lib.describe_gatv2_attention(G["M"], G["K"], H, F, G["nnz"], xa, xa, fa, x16=x16),
            single=head,
            check64=lambda h, keep, ks, msg: refs.gatv2_attention_x16_check_all(G, x, slope, h, dtype, keep, ks, what=msg),
            neighbour=x["xr"], extra_checks=extras)
    _report("%s %s" % (family, X16_IDS[X16_DTYPES.index(dtype)]))


@pytest.mark.parametrize("dtype", X16_DTYPES, ids=X16_IDS)
def test_dot_attention_x16(pkg, dtype):
    """dot_attention_x16 and its two backward passes on bf16 / fp16 q, k and v (``_x16_common``)."""
    from gespmm_amd import _lib

    family = "dot_x16"
    for c in family_cases(family):
        G, H, F = c["G"], c["H"], c["F"]
        x = dot_x16_inputs(c, dtype)

        def head(hd):
            xs = {n: np.ascontiguousarray(x[n][:, hd:hd + 1]) for n in ("q", "k", "v", "go")}
            xs["scale"] = x["scale"]
            return lambda g, at16, at32, small, drop: _dot_x16_run(g, xs, dtype, at16, small, drop)

        _x16_common(
            family, c, dtype, RESULTS_DOT, NARROW_DOT, ("grad_k", "grad_v"),
            run=lambda g, at16, at32, small, drop: _dot_x16_run(g, x, dtype, at16, small, drop),
            oracle=lambda g, at32, small, drop: (_dot_run(g, x, at32, drop, small=small, stored=dtype), None),
            describe=lambda xa, fa, x16: _lib.describe_dot_attention(G["M"], G["K"], H, F, G["nnz"], xa, xa, xa, x16=x16),
            single=head,
            check64=lambda h, keep, ks, msg: refs.dot_x16_check_all(G, x, h, dtype, keep, ks, what=msg),
            neighbour=x["v"])
    _report("%s %s" % (family, X16_IDS[X16_DTYPES.index(dtype)]))


# ------------------------------------------------------------------------------------------ 13. the max reducer on 16-bit operands

MAX_ARG_KINDS = ("ints", "floats", "positive")
MAX_ARG_EMPTIES = (-10000.0, 0.0, float("-inf"))


def narrow_bits(a, dtype):
    """fp32 host array -> the bits (int16) of its ONE rounding to ``dtype``, to nearest even."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).view(torch.int16).numpy()


def max_arg_x16_inputs(c, dtype):
    """-> (grad_out, {kind: B}, empty_value): the draws of ``test_max_arg_and_backward`` in its order — grad_out seeded normals, B
    integers in -2 .. 2, normals with planted +0, -0, NaN and -20000, and |normals| — rounded once to ``dtype`` and widened again
    (``refs.rounded``): the fp32 values of what the device holds, so the reference sees bf16's -19968 where -20000 was planted.
    ``empty_value`` is one of -10000, 0 and -inf by the case's seed. bf16 alone: after every other draw, -9984 and -10048 are planted
    in the floats (4 % of the words each) — the two bf16 neighbours of -10000, which is no bf16 value; no draw holds either by itself,
    and without them nothing in the family tells a compare against -10000 as given from one against its rounding, -9984."""
    G, N = c["G"], c["H"] * c["F"]
    rng = np.random.RandomState(c["seed"])
    grad = rng.standard_normal((G["M"], N)).astype(np.float32)
    B = {"ints": rng.randint(-2, 3, size=(G["K"], N)).astype(np.float32)}
    B["floats"] = rng.standard_normal((G["K"], N)).astype(np.float32)
    for value in (0.0, -0.0, np.nan, -20000.0):
        B["floats"][rng.rand(G["K"], N) < 0.04] = np.float32(value)
    B["positive"] = np.abs(rng.standard_normal((G["K"], N))).astype(np.float32)
    if dtype == torch.bfloat16:
        for value in (-9984.0, -10048.0):
            B["floats"][rng.rand(G["K"], N) < 0.04] = np.float32(value)
    return refs.rounded(grad, dtype), {k: refs.rounded(v, dtype) for k, v in B.items()}, MAX_ARG_EMPTIES[c["seed"] % 3]


@functools.lru_cache(maxsize=None)
def max_arg_x16_cases():
    return tuple(family_cases("max_arg_x16"))


@functools.lru_cache(maxsize=None)
def max_arg_x16_expected(index, dtype):
    """The expected results of case ``index`` in ``dtype``, computed once and shared by the device test and the host tests (nobody
    writes into them): {"empty", "grad" (widened fp32), kind: {"B" (widened fp32), "arg", "C" (fp32, of the widened operand), "out_bits"
    (C narrowed once), "grad_B" (fp32 chain on the widened grad_out), "grad_B_bits" (narrowed once)}}."""
    c = max_arg_x16_cases()[index]
    G = c["G"]
    grad, B, empty = max_arg_x16_inputs(c, dtype)
    want = {"empty": empty, "grad": grad}
    for kind in MAX_ARG_KINDS:
        C, arg = refs.max_arg_forward(G["rowptr"], G["colind"], B[kind], empty)
        gB = refs.max_backward(G["colptr"], G["rowind"], G["order"], arg, grad, G["K"])
        want[kind] = {"B": B[kind], "arg": arg, "C": C, "out_bits": narrow_bits(C, dtype), "grad_B": gB, "grad_B_bits": narrow_bits(gB, dtype)}
    return want


def _host_bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


@pytest.mark.parametrize("dtype", X16_DTYPES, ids=X16_IDS)
def test_max_arg_x16(pkg, dtype):
    """csr_spmm_max_arg_x16 and csr_spmm_max_backward_x16 (width N = H F), every comparison on bits: arg the restatement's on the
    exact widening of the 16-bit operand, out its C narrowed once, grad_B the fp32 add chain on the widened grad_out narrowed once
    (``max_arg_x16_expected``). Two passes: B, out, grad_out and grad_B at the case's offset in bytes, then 2 bytes further, where the
    route function must answer V = 1 (neighbouring lanes store the two halves of a dword); arg at the fp32 oracle's offset, twice the
    16-bit one modulo 16. Operands of ``test_max_arg_and_backward`` narrowed once; empty_value -10000 (no bf16 value: compared as given,
    narrowed only where a row keeps it), 0 or -inf by the case's seed. On |normals| the fp32 entry on the widened operand, on the GPU,
    gives the same arg and, narrowed, the same out. First pass: a second run repeats the bits. On the MI355X: 0.43 s (bf16) and
    0.38 s (fp16) in the module's own run, where the other 16-bit families take 0.66 - 0.72 s; no mismatch."""
    from gespmm_amd import _lib, spmm

    for c in max_arg_x16_cases():
        G, N, off = c["G"], c["H"] * c["F"], c["offset"]
        g = _graph(G)
        want = max_arg_x16_expected(c["index"], dtype)
        empty = want["empty"]
        empty_bits = narrow_bits(np.full(1, empty, dtype=np.float32), dtype)[0]
        empty_r = G["degs"] == 0
        for extra in (0, 2):
            at16, at32 = x16_offsets(off, extra)
            msg = "%s %s empty_value=%s, 16-bit arrays %d bytes off, arg %d" % (what("max_arg_x16", c), dtype, empty, at16, at32)
            for S in (G["M"], G["K"]):
                route = _lib.max_arg_route_x16(S, G["nnz"], N, align_at(at16), align_at(at32))
                assert route is not None and (extra == 0 or route[0] == 1), (msg, route)
            grad = _place(_dev(want["grad"]).to(dtype), at16)
            for kind in MAX_ARG_KINDS:
                w, m2 = want[kind], "%s %s" % (msg, kind)
                B = _place(_dev(w["B"]).to(dtype), at16)
                assert B.data_ptr() % 16 == at16 == grad.data_ptr() % 16

                def forward():
                    oc, oa = Out((G["M"], N), at16, dtype), Out((G["M"], N), at32, torch.int32)
                    assert oc.t.data_ptr() % 16 == at16 and oa.t.data_ptr() % 16 == at32
                    r = spmm.csr_spmm_max_arg_x16(g["rowptr"], g["colind"], B, empty_value=empty, out=oc.t, arg=oa.t)
                    assert r[0] is oc.t and r[1] is oa.t
                    return oc.check(m2 + ": out"), oa.check(m2 + ": arg")

                out, arg = forward()
                assert out.dtype == dtype and np.array_equal(arg.cpu().numpy(), w["arg"]), m2 + ": arg"
                assert np.array_equal(_host_bits16(out), w["out_bits"]), m2 + ": out"
                if empty_r.any():
                    assert bool((arg.cpu().numpy()[empty_r] == -1).all()) and bool((_host_bits16(out)[empty_r] == empty_bits).all()), \
                        m2 + ": an empty row is not (narrow(empty_value), -1)"
                if kind == "positive":
                    C32, arg32 = spmm.csr_spmm_max_arg(g["rowptr"], g["colind"], _place(_dev(w["B"]), at32), empty_value=empty)
                    _same(arg32, arg, m2 + ": arg against the fp32 entry on the widened operand")
                    _same(C32.to(dtype), out, m2 + ": out against the fp32 entry's C narrowed once")

                def backward():
                    ob = Out((G["K"], N), at16, dtype)
                    assert ob.t.data_ptr() % 16 == at16
                    assert spmm.csr_spmm_max_backward_x16(g["colptr"], g["rowind"], g["order"], arg, grad, G["K"], out=ob.t) is ob.t
                    return ob.check(m2 + ": grad_B")

                gB = backward()
                assert gB.dtype == dtype and np.array_equal(_host_bits16(gB), w["grad_B_bits"]), m2 + ": grad_B"
                chosen = np.zeros(G["K"], dtype=bool)
                chosen[G["colind"][w["arg"][w["arg"] >= 0]]] = True
                _plus_zero(gB, ~chosen, m2 + ": grad_B of a node no row chose")
                if not extra:
                    out2, arg2 = forward()
                    _same(out2, out, m2 + ": out, second run")
                    _same(arg2, arg, m2 + ": arg, second run")
                    _same(backward(), gB, m2 + ": grad_B, second run")
    print("max_arg_x16 %s: %d cases, two passes, every comparison on bits" % (X16_IDS[X16_DTYPES.index(dtype)], N_CASES))
