"""The seeded sweep of the aggregate-and-linear family on the device: linear_cases.py's fixed case lists (test_linear_fuzz_host.py shows
that they reach every template instance of spmm_linear.hip, spmm_relational.hip, spmm_relational_wgrad.hip and
spmm_relational_f32.hip) on every dtype of the op, valued and unweighted.

Every case asserts: the route function's answer (1 served, 0 unserved); every word of the NaN-prefilled result written; the 64-element
guards round the result and round every operand view untouched; exact equality with the int64 reference on the exact-eligible rows
(linear_cases' docstring) and test_gpu_spmm_linear._within — H the library's own product on the stacked arrays, n as the existing
docstrings derive it — on the others; the same bits from a second call and from a call on a non-default stream.

Not tested: non-finite WEIGHTS. A (block, relation) pair without entries is skipped, so an Inf in W[r] meets no 0 there while the
composition multiplies it by the zero aggregate: 0 x Inf differs between the two by design."""
import time

import numpy as np
import pytest
import torch

import linear_cases as lc
from test_gpu_spmm_linear import _h, _within

pytestmark = pytest.mark.gpu

TD = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
PAD = 64
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _running_time():
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\ntest_gpu_linear_fuzz.py: %.1f s" % (time.perf_counter() - t0))


def _params(op):
    return [pytest.param(c, dt, id="%s-%s" % (lc.case_id(c), dt)) for c in lc.cases(op) for dt in lc.DTYPES[op]]


class Placed:
    """A dense operand as a view at ``off`` bytes (plus the 64-element guard) into a NaN-filled buffer."""

    def __init__(self, a, dtype, off, shape=None):
        shape = tuple(a.shape) if shape is None else shape
        n = int(np.prod(shape))
        es = torch.empty(0, dtype=dtype).element_size()
        assert off % es == 0
        self.start, self.n = PAD + off // es, n
        self.buf = torch.full((n + 2 * PAD + 16,), NAN, dtype=dtype, device="cuda")
        self.view = self.buf[self.start:self.start + n].view(shape)
        if a is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.start]).all()) and bool(torch.isnan(self.buf[self.start + self.n:]).all())


def _f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).float().cuda()


class Device:
    """The operands of a case on the device, in ``dtype``."""

    def __init__(self, case, dt):
        self.case, self.dt, self.dtype = case, dt, TD[dt]
        off = case["offsets"]
        self.rp, self.ci = torch.from_numpy(case["rowptr"]).cuda(), torch.from_numpy(case["colind"]).cuda()
        self.val, self.scale = _f32(case["values"]), _f32(case["row_scale"])
        self.X = Placed(case["X"], self.dtype, off["X"])
        self.placed = [self.X]
        if case["op"] == "wgrad":
            self.go = Placed(case["grad_out"], self.dtype, off["grad_out"])
            self.placed.append(self.go)
        else:
            self.W = Placed(case["W"], self.dtype, off["W"])
            self.placed.append(self.W)
            self.root = self.rw = None
            if case["root"] is not None:
                self.root, self.rw = Placed(case["root"], self.dtype, off["root"]), Placed(case["root_weight"], self.dtype, off["root_weight"])
                self.placed += [self.root, self.rw]
            self.bias = _f32(case["bias"])

    def align(self, *more):
        from gespmm_amd import spmm

        al = spmm.x16_align(*([p.view for p in self.placed[(0 if self.case["nnz"] else 1):]] + list(more)))
        return max(al, 4) if self.dt == "fp32" else al

    def result(self, shape):
        return Placed(None, self.dtype, self.case["offsets"]["out"], shape)

    def H(self, valued):
        from gespmm_amd import spmm

        c = self.case
        return _h(spmm, self.rp, self.ci, self.val if valued else None, self.X.view, self.scale).view(c["R"], c["M"], c["K"])

    def forward(self, valued, out=None):
        from gespmm_amd import spmm

        v, x, w = (self.val if valued else None), self.X.view, self.W.view
        root, rw = (None, None) if self.root is None else (self.root.view, self.rw.view)
        if self.case["op"] == "linear":
            return spmm.csr_spmm_linear(self.rp, self.ci, v, x, w[0], row_scale=self.scale, root=root, root_weight=rw, bias=self.bias, out=out)
        return spmm.csr_spmm_relational_linear(self.rp, self.ci, v, x, w, row_scale=self.scale, root=root, root_weight=rw, bias=self.bias, out=out)

    def wgrad(self, valued, chunks, out=None, workspace=None):
        from gespmm_amd import spmm

        return spmm.csr_spmm_relational_weight_grad(self.rp, self.ci, self.val if valued else None, self.X.view, self.go.view, self.case["R"],
                                                    row_scale=self.scale, chunks=chunks, out=out, workspace=workspace)

    def route(self, out, chunks=None):
        from gespmm_amd import _lib

        c = self.case
        args = (c["R"], c["M"], c["Kn"], c["K"], c["N_out"], c["nnz"])
        if c["op"] == "linear":
            return _lib.spmm_linear_route_x16(*args[1:], self.align(out))
        if c["op"] == "rel":
            return _lib.spmm_relational_route_x16(*args, self.align(out))
        if c["op"] == "f32":
            return _lib.spmm_relational_route_f32(*args, self.align(out))
        return _lib.spmm_relational_wgrad_route_x16(*args, chunks, self.align(out))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _on_side_stream(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = fn()
    s.synchronize()
    return out


def _kpad(case, dt):
    return (case["K"] + 7) // 8 * 8 if dt == "fp32" else (case["K"] + 15) // 16 * 16


def _check_forward(dev, valued, got):
    case, dt = dev.case, dev.dt
    ref, eligible, _, _ = lc.forward_ref(case, valued)
    elig = eligible(dt)
    g = got.double().cpu().numpy()

    def bounded(mask):
        rows = torch.from_numpy(np.flatnonzero(mask[:, 0])).cuda()
        H = dev.H(valued)
        terms = [(H[r][rows], dev.W.view[r]) for r in range(case["R"])] + ([(dev.root.view[rows], dev.rw.view)] if dev.root is not None else [])
        n = (case["R"] + 1) * _kpad(case, dt)
        _within(got[rows], terms, dev.bias, 2 * n + 2 if dt == "fp32" else n + 1, dev.dtype, what="%s rows off the exact mode: %d" % (lc.case_id(case), rows.numel()))
        return True

    assert lc.agrees(case, g, ref, lc.broadcast_rows(elig, ref.shape), bounded), (lc.case_id(case), dt, valued)
    return elig


def _forward_case(case, dt):
    dev = Device(case, dt)
    M, N_out = case["M"], case["N_out"]
    for valued in (False, True):
        res = dev.result((M, N_out))
        assert dev.route(res.view) == (1 if case["unserved"] is None else 0)
        got = dev.forward(valued, out=res.view)
        assert got.data_ptr() == res.view.data_ptr()
        assert not torch.isnan(got).any(), "a word of the result was not written"
        assert res.guards_intact() and all(p.guards_intact() for p in dev.placed)
        _check_forward(dev, valued, got)
        again = dev.forward(valued)
        assert torch.equal(_bits(again), _bits(got)), "a second call gives other bits"
        side = _on_side_stream(lambda: dev.forward(valued))
        assert torch.equal(_bits(side), _bits(got)), "a call on a non-default stream gives other bits"
    return dev, got


@pytest.mark.parametrize("case,dt", _params("linear"))
def test_linear(pkg, case, dt):
    from gespmm_amd import spmm

    dev, got = _forward_case(case, dt)
    if case["unserved"] is None:  # R = 1 of the relational kernel IS this op, bit for bit (its documented promise)
        root, rw = (None, None) if dev.root is None else (dev.root.view, dev.rw.view)
        rel = spmm.csr_spmm_relational_linear(dev.rp, dev.ci, dev.val, dev.X.view, dev.W.view, row_scale=dev.scale, root=root, root_weight=rw,
                                              bias=dev.bias)
        assert torch.equal(_bits(rel), _bits(got))


@pytest.mark.parametrize("case,dt", _params("rel"))
def test_relational(pkg, case, dt):
    _forward_case(case, dt)


@pytest.mark.parametrize("case,dt", _params("f32"))
def test_relational_f32(pkg, case, dt):
    _forward_case(case, dt)


def _check_wgrad(dev, valued, got, C, roundings=1, known=None):
    case, dt = dev.case, dev.dt
    ref, eligible, _, _ = lc.wgrad_ref(case, valued) if known is None else known
    elig = eligible(dt)

    def bounded(mask):
        H = dev.H(valued)
        for r in range(case["R"]):
            rows = torch.from_numpy(np.flatnonzero(mask[r].any(axis=1))).cuda()
            if rows.numel():
                _within(got[r][rows], [(dev.go.view.t()[rows], H[r].t())], None, case["M"] + C + 1, dev.dtype, roundings=roundings,
                        what="%s r=%d rows off the exact mode: %d" % (lc.case_id(case), r, rows.numel()))
        return True

    assert lc.agrees(case, got.double().cpu().numpy(), ref, elig, bounded), (lc.case_id(case), dt, valued, C)
    return torch.from_numpy(elig).cuda()


@pytest.mark.parametrize("case,dt", _params("wgrad"))
def test_weight_gradient(pkg, case, dt):
    from gespmm_amd import _lib

    dev = Device(case, dt)
    R, M, K, N_out = case["R"], case["M"], case["K"], case["N_out"]
    for valued in (False, True):
        results, known = [], lc.wgrad_ref(case, valued)
        for chunks in lc.chunk_list(R, M, K, N_out):
            C = _lib.spmm_relational_wgrad_chunks(R, M, K, N_out) if chunks is None else chunks
            assert C == (lc.wgrad_chunks(R, M, K, N_out) if chunks is None else chunks)
            res = dev.result((R, N_out, K))
            ws = torch.full((C, R, N_out, K), NAN, device="cuda")
            assert dev.route(res.view, C) == (1 if case["unserved"] is None else 0)
            got = dev.wgrad(valued, chunks, out=res.view, workspace=ws)
            assert got.data_ptr() == res.view.data_ptr()
            assert not torch.isnan(got).any(), "a word of the result was not written"
            assert res.guards_intact() and all(p.guards_intact() for p in dev.placed)
            elig = _check_wgrad(dev, valued, got, C, roundings=1 if case["unserved"] is None else 2, known=known)
            results.append(got.clone())
            again = dev.wgrad(valued, chunks)
            assert torch.equal(_bits(again), _bits(got)), "a second call gives other bits"
            side = _on_side_stream(lambda: dev.wgrad(valued, chunks))
            assert torch.equal(_bits(side), _bits(got)), "a call on a non-default stream gives other bits"
        for other in results[1:]:  # any forced chunk count: the same exact-eligible elements
            assert torch.equal(other[elig], results[0][elig])


# ---- NaN in rows of X: unread rows stay out, a named row reaches exactly the reference's rows -----------------------------------------

def _nan_case(op):
    """The served case with named and unnamed rows of X that has more than one relation, by preference a uniform one of several blocks."""
    ok = [c for c in lc.cases(op) if c["unserved"] is None and c["R"] >= 2 - (op == "linear") and 0 < np.unique(c["colind"]).size < c["Kn"]]
    return max(ok, key=lambda c: (c["law"] == "uniform", c["M"] > 64, c["K"]))


@pytest.mark.parametrize("op,dt", [(op, dt) for op in lc.OPS for dt in lc.DTYPES[op]])
def test_nan_in_rows_of_x(pkg, op, dt):
    """Rows of X that no entry names hold NaN: the result is finite. Then one named row j holds NaN too: the result is NaN exactly where the float64 reference is — output row i when some
    relation's row i names j (0 x NaN is NaN for every output column), every element of grad_W[r] when relation r names j. Weights stay
    finite: see the module docstring."""
    case = _nan_case(op)
    dev = Device(case, dt)
    named = np.unique(case["colind"])
    unnamed = np.setdiff1d(np.arange(case["Kn"]), named)
    dev.X.view[torch.from_numpy(unnamed).cuda()] = NAN
    run = (lambda: dev.wgrad(True, None)) if op == "wgrad" else (lambda: dev.forward(True))
    assert torch.isfinite(run()).all()
    cols, counts = np.unique(case["colind"], return_counts=True)
    j = int(cols[np.argmin(counts)])  # the named row with the fewest entries: some rows (relations) stay finite
    dev.X.view[j] = NAN
    rows = np.repeat(np.arange(case["R"] * case["M"]), np.diff(case["rowptr"]))[case["colind"] == j]
    got = torch.isnan(run()).cpu().numpy()
    if op == "wgrad":
        want = np.zeros(got.shape, dtype=bool)
        want[np.unique(rows // case["M"])] = True
    else:
        want = np.zeros(got.shape, dtype=bool)
        want[np.unique(rows % case["M"])] = True
    assert 0 < want.sum() < want.size or case["R"] == 1
    assert np.array_equal(got, want)
    assert torch.isfinite(run()[torch.from_numpy(~want).cuda()]).all()


# ---- the autograd functions on rectangular graphs --------------------------------------------------------------------------------------

def _gradient_cases(op):
    picked = [c for c in lc.cases(op) if c["unserved"] is None and c["Kn"] != c["M"] and c["nnz"]][:6]
    return [pytest.param(c, dt, id="%s-%s" % (lc.case_id(c), dt)) for c in picked for dt in lc.DTYPES[op]]


def _grad_out(case):
    rng = np.random.RandomState(case["index"] + 7)
    return lc._sparse_columns(rng, case["N_out"], case["M"], 4, (case["N_out"], case["M"])).T.copy()


def _transposed(case, go, valued, linear):
    """grad_x as a forward case on the stacked CSC: dense = grad_out, weight = W^T and per-entry weights row_scale x value (the relational
    backward), or dense = narrow(row_scale * grad_out) and the values alone (SpmmLinearFunction's)."""
    cp, ri, order = lc.stacked_csc(case)
    R, M, Kn = case["R"], case["M"], case["Kn"]
    w = case["values"][order] if valued else np.ones(order.shape[0])
    scale = case["row_scale"]
    X = go
    if scale is not None and linear:
        X = go * scale[:, None]
    elif scale is not None:
        rel = np.repeat(np.arange(R * Kn) // Kn, np.diff(cp))
        w = w * scale[rel * M + ri]
    t = {"op": "rel", "R": R, "M": Kn, "Kn": M, "K": case["N_out"], "N_out": case["K"], "rowptr": cp, "colind": ri, "values": w, "row_scale": None,
         "X": X, "W": case["W"].transpose(0, 2, 1).copy(), "root": None, "bias": None, "grid": 0.5, "nnz": case["nnz"]}
    return t, cp, ri, order


def _check_grad_x(case, t, gx, dt, n):
    ref, eligible, H, _ = lc.forward_ref(t, True)
    elig = eligible(dt)
    _, Habs = lc.aggregates(t, True)

    def bounded(mask):
        rows = np.flatnonzero(mask[:, 0])
        terms = [(torch.from_numpy(H[r][rows]), torch.from_numpy(t["W"][r]), torch.from_numpy(Habs[r][rows])) for r in range(t["R"])]
        _within(gx[torch.from_numpy(rows).cuda()], terms, None, n, TD[dt], roundings=2, what="grad_x rows off the exact mode: %d" % rows.size)
        return True

    assert lc.agrees(t, gx.double().cpu().numpy(), ref, lc.broadcast_rows(elig, ref.shape), bounded), (lc.case_id(case), dt)


@pytest.mark.parametrize("case,dt", _gradient_cases("rel") + _gradient_cases("f32"))
def test_relational_function_gradients_on_rectangular_graphs(pkg, case, dt):
    from gespmm_amd import RelationalLinearFunction

    dev = Device(case, dt)
    go_h = _grad_out(case)
    go = torch.from_numpy(go_h).to(dev.dtype).cuda()
    R, M, Kn, K, N_out = (case[k] for k in ("R", "M", "Kn", "K", "N_out"))
    for valued in (False, True):
        t, cp, ri, order = _transposed(case, go_h, valued, linear=False)
        cpd, rid = torch.from_numpy(cp).cuda(), torch.from_numpy(ri).cuda()
        v_csr = dev.val if valued else None
        v_csc = dev.val[torch.from_numpy(order).cuda()] if valued else None
        leaves = [p.clone().requires_grad_(True) for p in (dev.X.view, dev.W.view)]
        extra = [] if dev.root is None else [dev.root.view.clone().requires_grad_(True), dev.rw.view.clone().requires_grad_(True)]
        root, rw = extra if extra else (None, None)
        bias = None if dev.bias is None else dev.bias.clone().requires_grad_(True)
        out = RelationalLinearFunction.apply(dev.rp, dev.ci, cpd, rid, leaves[0], leaves[1], dev.scale, root, rw, bias, v_csr, v_csc, True,
                                             dt != "fp32")
        _check_forward(dev, valued, out.detach())
        grads = torch.autograd.grad(out, leaves + extra + ([bias] if bias is not None else []), go)
        col = int(np.diff(cp).max())
        npad = (N_out + 15) // 16 * 16
        _check_grad_x(case, t, grads[0], dt, 2 * R * N_out + col + 3 if dt == "fp32" else R * npad + col + 2)
        wcase = dict(case, grad_out=go_h)
        wdev = Device(dict(wcase, op="wgrad", offsets={"X": 0, "grad_out": 0, "out": 0}), dt)
        if dt == "fp32":  # composed: H the library's fp32 product, a rounding per product and per addition
            H = wdev.H(valued)
            for r in range(R):
                _within(grads[1][r], [(go.t(), H[r].t())], None, 2 * M + 2, dev.dtype, what="grad_weight[%d]" % r)
        else:
            from gespmm_amd import _lib

            _check_wgrad(wdev, valued, grads[1], _lib.spmm_relational_wgrad_chunks(R, M, K, N_out))
        if extra:
            _within(grads[2], [(go, rw.detach().t())], None, N_out, dev.dtype, what="grad_root")
            _within(grads[3], [(go.t(), root.detach().t())], None, M, dev.dtype, what="grad_root_weight")
        if bias is not None:
            _within(grads[-1].unsqueeze(0), [(torch.ones(1, M), go.t())], None, M, torch.float32, what="grad_bias")


@pytest.mark.parametrize("case,dt", _gradient_cases("linear"))
def test_linear_function_gradients_on_rectangular_graphs(pkg, case, dt):
    from gespmm_amd import SpmmLinearFunction

    dev = Device(case, dt)
    go_h = _grad_out(case)
    go = torch.from_numpy(go_h).to(dev.dtype).cuda()
    M, Kn, K, N_out = (case[k] for k in ("M", "Kn", "K", "N_out"))
    for valued in (False, True):
        t, cp, ri, order = _transposed(case, go_h, valued, linear=True)
        cpd, rid = torch.from_numpy(cp).cuda(), torch.from_numpy(ri).cuda()
        v_csr = dev.val if valued else None
        v_csc = dev.val[torch.from_numpy(order).cuda()] if valued else None
        x, w = dev.X.view.clone().requires_grad_(True), dev.W.view[0].clone().requires_grad_(True)
        root, rw = (None, None) if dev.root is None else (dev.root.view, dev.rw.view)
        out = SpmmLinearFunction.apply(dev.rp, dev.ci, cpd, rid, x, w, dev.scale, root, rw, dev.bias, v_csr, v_csc)
        _check_forward(dev, valued, out.detach())
        gx, gw = torch.autograd.grad(out, [x, w], go)
        col = int(np.diff(cp).max())
        _check_grad_x(case, t, gx, dt, N_out + col)
        G, Gabs = lc.aggregates(t, True)  # [1, Kn, N_out] float64: A^T g' and its absolute-value sums
        _within(gw, [(torch.from_numpy(G[0]).t(), x.detach().t(), torch.from_numpy(Gabs[0]).t())], None, Kn + col, dev.dtype, roundings=2,
                what="grad_weight")
