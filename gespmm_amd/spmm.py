"""Mirror of the reference's pybind11 module ``spmm`` (pytorch-custom/spmm.cpp:96-101):

    csr_spmm(rowptr, colind, values, dense)        -> f32[M, N]   spmm.cpp:24-43
    csr_spmm_no_edge_value(rowptr, colind, dense)  -> f32[M, N]   spmm.cpp:45-60
    csr2csc(rowptr, colind, colptr, rowind, csr_data) -> f32[nnz] spmm.cpp:70-93

Same names, argument order and meaning. Where the reference only ``assert``s its
inputs (compiled out under NDEBUG) these functions raise. Outputs are allocated with
``torch.empty`` on ``dense.device`` like spmm_kernel.cu:183,434; kernels run on the
CURRENT torch stream (the reference uses the legacy default stream). Calls go through
the pybind11 extension `_gespmm_torch` (csrc/torch_binding.cpp) when it is built and
through the ctypes binding of the same C ABI otherwise or when tuning knobs are used;
both validate identically and neither has a CPU path. Extra keyword
arguments (``variant``, ``cfg``) expose the C ABI's tuning knobs and default to the
library's choice.

16-bit operands: ``csr_spmm``, ``csr_spmm_no_edge_value`` and ``SpmmPlan.run`` also take ``dense`` of ``torch.float16`` /
``torch.bfloat16`` and return that dtype (gespmm_csr_spmm_x16 / gespmm_plan_spmm_x16: the sum is fp32 and is rounded once, so the result
has the bits of ``op(dense.float()).to(dense.dtype)``). ``values`` stay fp32, ``out=`` must have the dtype of ``dense``, ``cfg=`` needs
fp32. ``csr_spmm_fused``, ``csr_spmm_max`` / ``reduce_max=`` and ``SpmmPlan.tune`` are fp32 only. The SDDMM ops (``sddmm.py``) take fp16 / bf16
operands too and return fp32: ``sddmm.csr_sddmm(rowptr, colind, grad_out, feat)`` is the edge-weight gradient of a 16-bit model.
"""
import ctypes

import torch

from . import _lib
from ._ext import ext as _ext
from ._lib import LaunchCfg, check, lib


def _need(t, name, dtype, ndim):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.device.type != "cuda":
        raise RuntimeError("%s must be a HIP (cuda) device tensor; gespmm_amd has no CPU path" % name)
    if t.dtype != dtype:
        raise TypeError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != ndim:
        raise ValueError("%s must be %d-dimensional" % (name, ndim))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


_X16 = {torch.float16: _lib.X16_F16, torch.bfloat16: _lib.X16_BF16}


def _need_dense(t, name="dense"):
    """``dense`` of the products: fp32, or fp16 / bf16 (the 16-bit entry points). Returns the GESPMM_X16_* code, 0 for fp32."""
    if isinstance(t, torch.Tensor) and t.dtype in _X16:
        _need(t, name, t.dtype, 2)
        return _X16[t.dtype]
    _need(t, name, torch.float32, 2)
    return 0


def _same_device(*ts):
    dev = ts[0].device
    for t in ts[1:]:
        if t.device != dev:
            raise RuntimeError("all tensors must live on the same device")
    return dev


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _on_device:
    """`with torch.cuda.device(dev)` only when dev is not already current (the context
    manager costs ~3 us per op call; the common case needs nothing)."""

    __slots__ = ("ctx",)

    def __init__(self, dev):
        self.ctx = None if dev.index is None or dev.index == torch.cuda.current_device() else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


def _make_cfg(cfg):
    if cfg is None:
        return None
    if isinstance(cfg, LaunchCfg):
        return cfg
    return LaunchCfg(int(cfg.get("vec", 0)), int(cfg.get("strips", 0)), int(cfg.get("group", 0)),
                     int(cfg.get("rows_per_wave", 0)), int(cfg.get("slab_rows", 0)), int(cfg.get("flags", 0)))


class SpmmPlan:
    """The analysis stage for ONE sparse matrix at one feature width (``gespmm_plan_*`` of the C ABI — what the
    vendor libraries call preprocess; the reference has none). Creating a plan analyses the matrix once, on the
    device (``analysis="host"`` keeps the round-2 host form: same order, ~20x slower), and keeps what every later
    launch reuses: the long-row decision from the longest row it
    saw, the split points of the cache-blocked path (dense graphs), and — for sparse graphs whose B exceeds the
    L2s — a row-CLUSTERED copy of the matrix with an nnz-balanced task table, so rows that share neighbours run
    next to each other and find the shared B rows in L2 (and, at N = 128 / 256 where blocks of 96 / 64 clustered rows
    reuse their B rows, the tables of the staged-rows kernel: those rows are read from LDS; made for THIS width
    only). Only the processing order changes: the result has the same bits as the plain call.
    ``kernel``: "auto" | "stream" | "seg-stream" | "staged" | "records" | "staged-slabs" (dense clustered matrices, N = 128).

        plan = SpmmPlan(rowptr, colind, K, N, values=val)      # reorder="auto" | True | False
        out = csr_spmm(rowptr, colind, val, dense, plan=plan)

    The plan keeps references to ``rowptr`` / ``colind`` (and the values it last saw) and notices in-place edits
    through the tensors' version counters: new VALUES are re-permuted automatically, a changed PATTERN raises —
    make a new plan. One plan serves one stream at a time.

    ``expected_launches`` (0 = 200, the reference's protocols): with ``reorder="auto"`` the analysis is weighed against the
    products that will use it — a matrix whose estimated gain x launches does not pay for the estimated analysis time keeps
    its storage order and costs one validation pass (``describe()`` says so).
    """

    def __init__(self, rowptr, colind, K, N, variant=_lib.VARIANT_AUTO, values=None, reorder="auto", task_entries=0,
                 threads=0, flags=0, row_floor=0, kernel="auto", analysis="device", expected_launches=0):
        _need(rowptr, "rowptr", torch.int32, 1)
        _need(colind, "colind", torch.int32, 1)
        if values is not None:
            _need(values, "values", torch.float32, 1)
            if values.numel() != colind.numel():
                raise ValueError("values and colind must have the same length")
        dev = _same_device(rowptr, colind) if values is None else _same_device(rowptr, colind, values)
        self.shape = (rowptr.numel() - 1, int(K), int(N), colind.numel(), int(variant))
        self._rowptr, self._colind = rowptr, colind  # strong references: the plan may point at them
        self._pattern_version = (rowptr._version, colind._version)
        self._values = values
        self._values_version = values._version if values is not None else None
        self.device = dev
        mode = {"auto": _lib.PLAN_REORDER_AUTO, True: _lib.PLAN_REORDER, False: _lib.PLAN_NO_REORDER}[reorder]
        kern = {"auto": _lib.PLAN_KERNEL_AUTO, "stream": _lib.PLAN_KERNEL_STREAM, "seg-stream": _lib.PLAN_KERNEL_SEG_STREAM,
                "staged": _lib.PLAN_KERNEL_STAGED, "records": _lib.PLAN_KERNEL_RECORDS, "staged-slabs": _lib.PLAN_KERNEL_STAGED_SLABS}[kernel]
        where = {"device": _lib.PLAN_ANALYSIS_DEVICE, "host": _lib.PLAN_ANALYSIS_HOST}[analysis]
        opt = _lib.PlanOptions(mode, int(task_entries), int(row_floor), int(threads), int(flags), kern, where, int(expected_launches))
        self._handle = ctypes.c_void_p()
        M, K_, N_, nnz, var = self.shape
        with _on_device(dev):
            _lib.ensure_init(dev.index if dev.index is not None else torch.cuda.current_device(), _stream(dev), shape=(M, K_, nnz, N_),
                             expected_launches=expected_launches, forced=(reorder is True))
            rc = lib.gespmm_plan_create_v2(ctypes.byref(self._handle), _ptr(rowptr), _ptr(colind),
                                           _ptr(values) if values is not None else None, M, K_, nnz, N_, var,
                                           ctypes.byref(opt), ctypes.sizeof(opt), _stream(dev))
        check(rc, "gespmm_plan_create_v2")

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value and lib is not None:  # (module globals are gone at interpreter shutdown)
            lib.gespmm_plan_destroy(h)
            self._handle = ctypes.c_void_p()

    def tune(self, dense, out=None, reps=3):
        """Kernel choice by measurement (gespmm_plan_tune): the plan's candidate kernels run ``reps`` times each on ``dense`` and the
        fastest is kept; returns the product (same bits whichever wins). ``dense`` must have the plan's width. fp32 only."""
        _need(dense, "dense", torch.float32, 2)
        M, K, N, _, _ = self.shape
        if tuple(dense.shape) != (K, N):
            raise ValueError("tune() needs dense of shape (K, N) = (%d, %d)" % (K, N))
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=self.device)
        with _on_device(self.device):
            check(lib.gespmm_plan_tune(self._handle, _ptr(dense), _ptr(out), N, int(reps), _stream(self.device)), "gespmm_plan_tune")
        return out

    def describe(self):
        buf = ctypes.create_string_buffer(1400)
        n = lib.gespmm_plan_describe(self._handle, buf, 1400)
        if n < 0:
            check(int(n), "gespmm_plan_describe")
        return buf.value.decode()

    @property
    def clustered(self):
        return self.describe().startswith("order=clustered")

    def order(self):
        """perm[i] = row processed at position i (torch int32 on the CPU)."""
        perm = torch.empty(self.shape[0], dtype=torch.int32)
        rc = lib.gespmm_plan_get_order(self._handle, ctypes.c_void_p(perm.data_ptr()))
        if rc < 0:
            check(rc, "gespmm_plan_get_order")
        return perm

    def _sync_inputs(self, rowptr, colind, values, dense, variant):
        if int(variant) != self.shape[4]:
            raise ValueError("SpmmPlan was made for a different matrix or variant")
        self._check_pattern(rowptr, colind, dense.shape[0])
        if values is None:
            if self._values is not None:
                with _on_device(self.device):
                    check(lib.gespmm_plan_set_values(self._handle, None, _stream(self.device)), "gespmm_plan_set_values")
                self._values, self._values_version = None, None
        elif self._values is None or values.data_ptr() != self._values.data_ptr() or \
                values._version != self._values_version:
            with _on_device(self.device):
                check(lib.gespmm_plan_set_values(self._handle, _ptr(values), _stream(self.device)), "gespmm_plan_set_values")
            self._values, self._values_version = values, values._version

    def run(self, values, dense, out=None, reduce_max=None):
        """``dense`` may be fp16 / bf16 (the result has its dtype; sum reducer only: ``reduce_max`` needs fp32)."""
        x16 = _need_dense(dense) if reduce_max is None else _need(dense, "dense", torch.float32, 2)
        M, K, _, _, _ = self.shape
        N = dense.shape[1]
        if _ext is not None and reduce_max is None and hasattr(_ext, "plan_spmm"):
            return _ext.plan_spmm(self._handle.value, dense, out, M)  # pybind11 path: ~5 us per call instead of ~12
        if out is None:
            out = torch.empty((M, N), dtype=dense.dtype, device=self.device)
        elif x16:
            _need(out, "out", dense.dtype, 2)
            if tuple(out.shape) != (M, N) or out.device != self.device:
                raise ValueError("out must be [M, N] of the dtype of dense on the same device")
        if x16:
            with _on_device(self.device):
                rc = lib.gespmm_plan_spmm_x16(self._handle, _ptr(dense), _ptr(out), x16, N, _stream(self.device))
            check(rc, "gespmm_plan_spmm_x16")
            return out
        with _on_device(self.device):
            if reduce_max is None:
                rc = lib.gespmm_plan_spmm_f32(self._handle, _ptr(dense), _ptr(out), N, _stream(self.device))
            else:
                rc = lib.gespmm_plan_spmm_max_f32(self._handle, _ptr(dense), _ptr(out), N, float(reduce_max),
                                                  _stream(self.device))
        check(rc, "gespmm_plan_spmm_f32")
        return out

    def run_fused(self, values, dense, col_scale, row_scale, bias, out=None, reduce_max=None):
        """The fused product through the plan (gespmm_plan_spmm_fused_f32): ``((A @ (col_scale * dense)) * row_scale) + bias`` with the
        bits of the four separate passes; each vector may be None. ``values`` is what ``run`` takes (the plan already holds them)."""
        _need(dense, "dense", torch.float32, 2)
        M, K, _, _, _ = self.shape
        N = dense.shape[1]
        col_scale, row_scale, bias = _fused_vectors(dense, M, col_scale, row_scale, bias)
        if reduce_max is not None:
            if col_scale is not None or row_scale is not None or bias is not None:
                raise _lib.GespmmError(-1, "gespmm_plan_spmm_fused_f32 (the fused product supports the sum reducer only)")
            return self.run(values, dense, out, reduce_max=reduce_max)
        if _ext is not None and hasattr(_ext, "plan_spmm_fused"):
            return _ext.plan_spmm_fused(self._handle.value, dense, col_scale, row_scale, bias, out, M)
        if out is None:
            out = torch.empty((M, N), dtype=torch.float32, device=self.device)
        with _on_device(self.device):
            rc = lib.gespmm_plan_spmm_fused_f32(self._handle, _ptr(dense), _optr(col_scale), _optr(row_scale), _optr(bias), _ptr(out), N,
                                                _stream(self.device))
        check(rc, "gespmm_plan_spmm_fused_f32")
        return out

    def x16_route(self, N=None, b_align=16, c_align=16):
        """What ``run`` does with fp16 / bf16 operands at width N (default: the plan's) whose addresses ``b_align`` / ``c_align`` divide
        (gespmm_plan_x16_route, host only): 0 widen + the fp32 route + narrow, 1 / 2 the 16-bit batch- / segmented-stream kernel."""
        rc = lib.gespmm_plan_x16_route(self._handle, int(self.shape[2] if N is None else N), int(b_align), int(c_align))
        if rc < 0:
            check(rc, "gespmm_plan_x16_route")
        return rc

    def _check_pattern(self, rowptr, colind, K):
        """The plan was made for exactly these index tensors, unmodified since."""
        M, K_, _, nnz, _ = self.shape
        if (rowptr.numel() - 1, int(K), colind.numel()) != (M, K_, nnz) or rowptr.data_ptr() != self._rowptr.data_ptr() or \
                colind.data_ptr() != self._colind.data_ptr():
            raise ValueError("SpmmPlan was made for a different matrix or variant")
        if (self._rowptr._version, self._colind._version) != self._pattern_version:
            raise ValueError("rowptr/colind were modified in place after the plan was made: create a new SpmmPlan")

    def run_heads(self, values, dense, out=None, order=None):
        """The multi-head product through the plan (gespmm_plan_spmm_heads_f32; see ``csr_spmm_heads``): ``values`` f32[nnz, H] in the
        caller's edge order — an argument of every call, the plan caches nothing of them and its own values stay what they are — and
        ``dense`` f32[K, H, F] or f32[K, H * F]. Same bits as the call without a plan. A clustered plan copies the weights into its own
        edge order on every call, which on a large graph with narrow heads costs more than clustering gains (com-amazon-sbm, H F <= 128:
        1.1-1.4x the time of the call without a plan) — there, call ``csr_spmm_heads`` without ``plan=``.
        ``order=`` (int32[nnz]): the weights of entry e are ``values[order[e]]``; a clustered plan composes it into that copy."""
        return csr_spmm_heads(self._rowptr, self._colind, values, dense, out=out, plan=self, order=order)

    def heads_route(self, H, F, b_align=16, c_align=16):
        """What ``run_heads`` does at H heads of F columns with operands whose addresses ``b_align`` / ``c_align`` divide
        (gespmm_plan_heads_route, host only): 1 the heads kernel, 0 the per-head composition."""
        rc = lib.gespmm_plan_heads_route(self._handle, int(H), int(F), int(b_align), int(c_align))
        if rc < 0:
            check(rc, "gespmm_plan_heads_route")
        return rc

    def sddmm_heads_route(self, H, F):
        """Which way ``sddmm.csr_sddmm_heads(..., plan=self)`` goes at H heads of F columns (gespmm_plan_sddmm_heads_route, host only):
        0 the stateless CSR call, 1 the heads kernel in COO form on row ids the plan expands once, 2 the plan's clustered edge order and
        a scatter into the caller's."""
        rc = lib.gespmm_plan_sddmm_heads_route(self._handle, int(H), int(F))
        if rc < 0:
            check(rc, "gespmm_plan_sddmm_heads_route")
        return rc

    def fused_route(self, N=None, col_scale=True, row_scale=True, bias=True):
        """What ``run_fused`` does at width N (default: the plan's) with these vectors present (gespmm_plan_fused_route, host only):
        0 the composition around the unfused launch, 1 the fused batch-stream kernel, 2 the fused segmented-stream kernel."""
        rc = lib.gespmm_plan_fused_route(self._handle, int(self.shape[2] if N is None else N), int(bool(col_scale)), int(bool(row_scale)),
                                         int(bool(bias)))
        if rc < 0:
            check(rc, "gespmm_plan_fused_route")
        return rc


def _optr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _fused_vectors(dense, M, col_scale, row_scale, bias):
    """The three optional vectors of the fused product as contiguous 1-D tensors: scales are accepted as [n] or [n, 1] (GCNConv keeps
    them as columns), bias as [N]."""
    K, N = dense.shape

    def one(t, name, n, column_ok):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor or None" % name)
        if column_ok and t.dim() == 2 and t.shape[1] == 1:
            t = t.reshape(-1)
        _need(t, name, torch.float32, 1)
        if t.numel() != n:
            raise ValueError("%s must have %d entries, got %d" % (name, n, t.numel()))
        if t.device != dense.device:
            raise RuntimeError("all tensors must live on the same device")
        return t

    return one(col_scale, "col_scale", K, True), one(row_scale, "row_scale", M, True), one(bias, "bias", N, False)


def csr_spmm_fused(rowptr, colind, values, dense, col_scale=None, row_scale=None, bias=None, out=None, plan=None,
                   variant=_lib.VARIANT_AUTO, reduce_max=None):
    """``C = ((A @ (col_scale[:, None] * dense)) * row_scale[:, None]) + bias`` in ONE product (gespmm_csr_spmm_fused_f32 /
    gespmm_plan_spmm_fused_f32) — the normalisation of a graph convolution without its three elementwise passes. ``values`` None: A == 1.
    fp32 only. Every vector is optional; the result has the bits of torch ``mul``, ``csr_spmm``, ``mul``, ``add`` as separate steps (with no
    vector at all the call IS the plain product). Sum reducer only: ``reduce_max`` together with a vector raises GESPMM_EINVAL."""
    _need(rowptr, "rowptr", torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    _need(dense, "dense", torch.float32, 2)
    if values is not None:
        _need(values, "values", torch.float32, 1)
        if values.numel() != colind.numel():
            raise ValueError("values and colind must have the same length")
        dev = _same_device(dense, rowptr, colind, values)
    else:
        dev = _same_device(dense, rowptr, colind)
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have M+1 >= 1 entries")
    M = rowptr.numel() - 1
    K, N = dense.shape
    if out is not None:
        _need(out, "out", torch.float32, 2)
        if tuple(out.shape) != (M, N) or out.device != dev:
            raise ValueError("out must be f32[M, N] on the same device")
    if plan is not None:
        plan._sync_inputs(rowptr, colind, values, dense, variant)
        return plan.run_fused(values, dense, col_scale, row_scale, bias, out, reduce_max=reduce_max)
    col_scale, row_scale, bias = _fused_vectors(dense, M, col_scale, row_scale, bias)
    if reduce_max is not None:
        if col_scale is not None or row_scale is not None or bias is not None:
            raise _lib.GespmmError(-1, "gespmm_csr_spmm_fused_f32 (the fused product supports the sum reducer only)")
        if values is not None:
            raise _lib.GespmmError(-1, "gespmm_csr_spmm_max_f32 (the max reducer is unweighted)")
        return csr_spmm_max(rowptr, colind, dense, float(reduce_max), variant)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    with _on_device(dev):
        rc = lib.gespmm_csr_spmm_fused_f32(_ptr(rowptr), _ptr(colind), _optr(values), _ptr(dense), _optr(col_scale), _optr(row_scale),
                                           _optr(bias), _ptr(out), M, K, N, colind.numel(), int(variant), _stream(dev))
    check(rc, "gespmm_csr_spmm_fused_f32")
    return out


def _heads_args(rowptr, colind, values, dense, out):
    """Validation of the multi-head product: (H, F, the result array — of the rank of ``dense``, contiguous, so the library's [M, H F])."""
    _need(rowptr, "rowptr", torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    _need(values, "values", torch.float32, 2)
    if not isinstance(dense, torch.Tensor):
        raise TypeError("dense must be a torch.Tensor")
    if dense.dim() not in (2, 3):
        raise ValueError("dense must be [K, H, F] or [K, H * F]")
    _need(dense, "dense", torch.float32, dense.dim())  # (16-bit operands have no multi-head entry: TypeError)
    dev = _same_device(dense, rowptr, colind, values)
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have M+1 >= 1 entries")
    M = rowptr.numel() - 1
    nnz, H = values.shape
    if nnz != colind.numel():
        raise ValueError("values must be [nnz, H] with nnz = %d rows, got %d" % (colind.numel(), nnz))
    if H < 1:
        raise ValueError("values must have at least one head")
    N = dense.shape[1] * dense.shape[2] if dense.dim() == 3 else dense.shape[1]
    if (dense.dim() == 3 and dense.shape[1] != H) or N % H != 0:
        raise ValueError("dense of shape %s does not hold H = %d heads" % (tuple(dense.shape), H))
    F = N // H
    shape = (M, H, F) if dense.dim() == 3 else (M, N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        _need(out, "out", torch.float32, len(shape))
        if tuple(out.shape) != shape or out.device != dev:
            raise ValueError("out must be f32%s on the same device" % (list(shape),))
    return H, F, out


class OrderedValues:
    """``values`` of the multi-head products read through an edge order, as ONE argument: ``csr_spmm_heads(rowptr, colind,
    OrderedValues(values, order), dense)`` is ``csr_spmm_heads(rowptr, colind, values, dense, order=order)`` — for callers that hand the
    weights on positionally (the autograd functions of ``op.py`` do: whatever wraps the product sees one call of its usual shape)."""

    __slots__ = ("values", "order")

    def __init__(self, values, order):
        self.values, self.order = values, order

    dtype = property(lambda self: self.values.dtype)
    shape = property(lambda self: self.values.shape)
    device = property(lambda self: self.values.device)


def _split_ordered(values, order):
    if isinstance(values, OrderedValues):
        if order is not None:
            raise ValueError("order= given twice: values is already an OrderedValues")
        return values.values, values.order
    return values, order


def _need_order(order, nnz, dev):
    """``order=`` of the multi-head products: int32[nnz], contiguous, on ``dev``. Raises before any launch."""
    if not isinstance(order, torch.Tensor):
        raise TypeError("order must be a torch.Tensor")
    if order.dtype == torch.int64:
        raise TypeError("order must have dtype torch.int32, got torch.int64: convert it once (order.to(torch.int32)), not per call")
    if order.dtype != torch.int32:
        raise TypeError("order must have dtype torch.int32, got %s" % order.dtype)
    if order.dim() != 1 or order.numel() != nnz:
        raise ValueError("order must be int32[nnz] with nnz = %d entries, got shape %s" % (nnz, tuple(order.shape)))
    if order.device != dev:
        raise ValueError("order must live on %s like the other tensors, got %s" % (dev, order.device))
    if not order.is_contiguous():
        raise ValueError("order must be contiguous")


def csr_spmm_heads(rowptr, colind, values, dense, out=None, plan=None, order=None):
    """Multi-head product (attention aggregation): ``out[r, h, :] = sum_e values[e, h] * dense[col(e), h, :]`` over the entries e of row
    r (gespmm_csr_spmm_heads_f32 / gespmm_plan_spmm_heads_f32). ``values`` f32[nnz, H]; ``dense`` f32[K, H, F] or f32[K, H * F], the
    result has the matching rank. One fp32 fma chain per output element in strict CSR order, so head h has the bits of
    ``csr_spmm(rowptr, colind, values[:, h].contiguous(), dense[:, h, :].contiguous(), cfg={"flags": FLAG_STRICT_ORDER})``.
    One kernel for 2 <= H <= 8 (``_lib.heads_route``), a per-head composition otherwise. fp32 only (TypeError otherwise): fp16 / bf16
    features go through ``csr_spmm_heads_x16``.

    ``order=`` (int32[nnz], contiguous, same device; entries in [0, nnz), not checked): the weights of entry e are ``values[order[e]]``
    — the bits of ``csr_spmm_heads(rowptr, colind, graphs.take_edges(values, order), dense)`` with no permuted copy
    (gespmm_csr_spmm_heads_order_f32 / gespmm_plan_spmm_heads_order_f32): one kernel wherever ``_lib.heads_route`` answers 1, allocating
    nothing; elsewhere a HIP gather into a stream-ordered temporary and the call above (not on a capturing stream). An int64 order
    raises TypeError — convert it once. ``values=OrderedValues(values, order)`` is the same call."""
    values, order = _split_ordered(values, order)
    H, F, out = _heads_args(rowptr, colind, values, dense, out)
    dev = dense.device
    M, K = rowptr.numel() - 1, dense.shape[0]
    if order is not None:
        _need_order(order, colind.numel(), dev)
    with _on_device(dev):
        if plan is not None:
            plan._check_pattern(rowptr, colind, K)
            if order is None:
                name = "gespmm_plan_spmm_heads_f32"
                rc = lib.gespmm_plan_spmm_heads_f32(plan._handle, _ptr(values), _ptr(dense), _ptr(out), H, F, _stream(dev))
            else:
                name = "gespmm_plan_spmm_heads_order_f32"
                rc = lib.gespmm_plan_spmm_heads_order_f32(plan._handle, _ptr(order), _ptr(values), _ptr(dense), _ptr(out), H, F, _stream(dev))
        elif order is None:
            name = "gespmm_csr_spmm_heads_f32"
            rc = lib.gespmm_csr_spmm_heads_f32(_ptr(rowptr), _ptr(colind), _ptr(values), _ptr(dense), _ptr(out), M, K, H, F, colind.numel(),
                                               _stream(dev))
        else:
            name = "gespmm_csr_spmm_heads_order_f32"
            rc = lib.gespmm_csr_spmm_heads_order_f32(_ptr(rowptr), _ptr(colind), _ptr(order), _ptr(values), _ptr(dense), _ptr(out), M, K, H, F,
                                                     colind.numel(), _stream(dev))
    check(rc, name)
    return out


def csr_spmm_heads_x16(rowptr, colind, values, dense, out=None, order=None):
    """The multi-head product on 16-bit features (gespmm_csr_spmm_heads_x16): ``values`` f32[nnz, H] — edge-sized arrays stay fp32 —
    ``dense`` fp16 or bf16, [K, H, F] or [K, H * F]; the result has the dtype and rank of ``dense``. Each output element is one fp32 fma
    chain in strict CSR order, rounded once at the store: the bits of ``csr_spmm_heads(rowptr, colind, values, dense.float()).to(dense.dtype)``.
    One kernel for 2 <= H <= 8, even F and 4-byte aligned operands (``_lib.heads_x16_route``), the composition widen / fp32 / narrow
    otherwise (not on a capturing stream). No plan form. ``order=``: as for ``csr_spmm_heads`` (gespmm_csr_spmm_heads_order_x16; one
    kernel wherever ``_lib.heads_x16_route`` answers 1)."""
    values, order = _split_ordered(values, order)
    _need(rowptr, "rowptr", torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    _need(values, "values", torch.float32, 2)
    if not isinstance(dense, torch.Tensor):
        raise TypeError("dense must be a torch.Tensor")
    if dense.dtype not in _X16:
        raise TypeError("dense must have dtype torch.float16 or torch.bfloat16, got %s (fp32: csr_spmm_heads)" % dense.dtype)
    if dense.dim() not in (2, 3):
        raise ValueError("dense must be [K, H, F] or [K, H * F]")
    _need(dense, "dense", dense.dtype, dense.dim())
    dev = _same_device(dense, rowptr, colind, values)
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have M+1 >= 1 entries")
    M, K = rowptr.numel() - 1, dense.shape[0]
    nnz, H = values.shape
    if nnz != colind.numel():
        raise ValueError("values must be [nnz, H] with nnz = %d rows, got %d" % (colind.numel(), nnz))
    if H < 1:
        raise ValueError("values must have at least one head")
    N = dense.shape[1] * dense.shape[2] if dense.dim() == 3 else dense.shape[1]
    if (dense.dim() == 3 and dense.shape[1] != H) or N % H != 0:
        raise ValueError("dense of shape %s does not hold H = %d heads" % (tuple(dense.shape), H))
    F = N // H
    shape = (M, H, F) if dense.dim() == 3 else (M, N)
    if out is None:
        out = torch.empty(shape, dtype=dense.dtype, device=dev)
    else:
        _need(out, "out", dense.dtype, len(shape))
        if tuple(out.shape) != shape or out.device != dev:
            raise ValueError("out must be %s%s on the same device" % (dense.dtype, list(shape)))
    if order is not None:
        _need_order(order, nnz, dev)
    with _on_device(dev):
        if order is None:
            name = "gespmm_csr_spmm_heads_x16"
            rc = lib.gespmm_csr_spmm_heads_x16(_ptr(rowptr), _ptr(colind), _ptr(values), _ptr(dense), _ptr(out), _X16[dense.dtype], M, K, H, F,
                                               nnz, _stream(dev))
        else:
            name = "gespmm_csr_spmm_heads_order_x16"
            rc = lib.gespmm_csr_spmm_heads_order_x16(_ptr(rowptr), _ptr(colind), _ptr(order), _ptr(values), _ptr(dense), _ptr(out),
                                                     _X16[dense.dtype], M, K, H, F, nnz, _stream(dev))
    check(rc, name)
    return out


def _overlaps(a, b):
    """Do the byte ranges of two contiguous tensors intersect?"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a.numel() > 0 and b.numel() > 0 and a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def gat_aggregate(ptr, ind, el, er, stats, dense, negative_slope=None, transposed=False, out=None, dropout=None):
    """GAT aggregation with no attention array (gespmm_gat_aggregate_f32): ``csr_spmm_heads`` with the weight of an entry computed
    inside the kernel, ``exp(leaky_relu(el[r, h] + er[c, h]) - stats[r, h, 0]) / stats[r, h, 1]`` for the entry's row r and column c —
    the bits of ``softmax.gat_edge_softmax`` when ``stats = softmax.gat_softmax_stats(rowptr, colind, el, er, negative_slope)``.

        transposed=False  (ptr, ind) = (rowptr, colind), dense f32[K, H, F] -> f32[M, H, F]: csr_spmm_heads(rowptr, colind, alpha, dense)
        transposed=True   (ptr, ind) = (colptr, rowind), dense f32[M, H, F] -> f32[K, H, F]: csr_spmm_heads(colptr, rowind,
                          alpha[csc_order], dense) — the feature gradient, without alpha and without its permuted copy

    bit for bit. ``el`` f32[M, H], ``er`` f32[K, H], ``stats`` f32[M, H, 2] are the same tensors in both modes. ``dense`` may be
    rank 2 ([rows, H * F]); the result has its rank. One kernel for H <= 8 (``_lib.gat_aggregate_route``), else the weights go through
    a pooled temporary. ``out`` must not overlap an input. fp32 only.

    ``dropout=(p, seed)`` (gespmm_gat_aggregate_dropout_f32): the weight becomes ``softmax.edge_dropout``'s value of it — kept and
    scaled by 1 / (1 - p), or +0 — recomputed inside the kernel from ``seed`` (int32[2] on the device) and the entry's (row, column,
    head), which are the same in both modes: the bits of ``csr_spmm_heads`` on ``edge_dropout(gat_edge_softmax(..))``. ``stats`` stay
    those of the softmax without dropout."""
    from . import softmax as _sm  # (softmax imports this module)

    slope = _sm._slope(negative_slope)
    _sm._dropout_typed(dropout)
    _sm._node_array(el, "el")
    _sm._node_array(er, "er", like=el)
    dev = el.device
    M, K, H = el.shape[0], er.shape[0], el.shape[1]
    S, Kb = (K, M) if transposed else (M, K)
    if _sm._checked_rowptr(ptr, dev) != S:
        raise ValueError("ptr must have %d + 1 entries (%s)" % (S, "colptr: transposed" if transposed else "rowptr"))
    _sm._index_vector(ind, "ind", dev)
    _sm._stats_array(stats, "stats", M, H, dev)
    if not isinstance(dense, torch.Tensor):
        raise TypeError("dense must be a torch.Tensor")
    if dense.dtype != torch.float32:
        raise TypeError("dense must have dtype torch.float32, got %s" % dense.dtype)
    if dense.dim() not in (2, 3) or dense.shape[0] != Kb:
        raise ValueError("dense must be [%d, H, F] or [%d, H * F]" % (Kb, Kb))
    N = dense.shape[1] * dense.shape[2] if dense.dim() == 3 else dense.shape[1]
    if (dense.dim() == 3 and dense.shape[1] != H) or N % H != 0:
        raise ValueError("dense of shape %s does not hold H = %d heads" % (tuple(dense.shape), H))
    if not dense.is_contiguous() or dense.device != dev:
        raise ValueError("dense must be contiguous on %s, as the other operands" % (dev,))
    F = N // H
    shape = (S, H, F) if dense.dim() == 3 else (S, N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch.Tensor")
        if out.dtype != torch.float32:
            raise TypeError("out must have dtype torch.float32, got %s" % out.dtype)
        if tuple(out.shape) != shape or out.device != dev or not out.is_contiguous():
            raise ValueError("out must be contiguous f32%s on %s" % (list(shape), dev))
        if any(_overlaps(out, t) for t in (el, er, stats, dense)):
            raise ValueError("out must not overlap an input")
    if dropout is not None:
        p, seed = _sm._dropout(dropout, dev)
        with _on_device(dev):
            rc = lib.gespmm_gat_aggregate_dropout_f32(_ptr(ptr), _ptr(ind), _ptr(el), _ptr(er), _ptr(stats), _ptr(dense), _ptr(out), M, K,
                                                      H, F, ind.numel(), slope, 1 if transposed else 0, p, _ptr(seed), _stream(dev))
        check(rc, "gespmm_gat_aggregate_dropout_f32")
        return out
    with _on_device(dev):
        rc = lib.gespmm_gat_aggregate_f32(_ptr(ptr), _ptr(ind), _ptr(el), _ptr(er), _ptr(stats), _ptr(dense), _ptr(out), M, K, H, F,
                                          ind.numel(), slope, 1 if transposed else 0, _stream(dev))
    check(rc, "gespmm_gat_aggregate_f32")
    return out


def _spmm(rowptr, colind, values, dense, variant, cfg, out, plan=None):
    _need(rowptr, "rowptr", torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    x16 = _need_dense(dense)
    if values is not None:
        _need(values, "values", torch.float32, 1)
        if values.numel() != colind.numel():
            raise ValueError("values and colind must have the same length")
        dev = _same_device(dense, rowptr, colind, values)
    else:
        dev = _same_device(dense, rowptr, colind)
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have M+1 >= 1 entries")
    M = rowptr.numel() - 1
    K, N = dense.shape
    nnz = colind.numel()
    if x16 and cfg is not None:
        raise ValueError("cfg (launch knobs) needs a torch.float32 dense: the 16-bit kernels are built without them")
    if out is None:
        out = torch.empty((M, N), dtype=dense.dtype, device=dev)
    else:
        _need(out, "out", dense.dtype, 2)
        if tuple(out.shape) != (M, N) or out.device != dev:
            raise ValueError("out must be [M, N] of the dtype of dense on the same device")
    c = _make_cfg(cfg)
    if plan is not None:
        if c is not None:
            raise ValueError("a plan fixes the launch configuration: pass either cfg or plan")
        plan._sync_inputs(rowptr, colind, values, dense, variant)
        return plan.run(values, dense, out)
    if x16:
        with _on_device(dev):
            rc = lib.gespmm_csr_spmm_x16(_ptr(rowptr), _ptr(colind), _ptr(values) if values is not None else None, _ptr(dense), _ptr(out),
                                         x16, M, K, N, nnz, int(variant), _stream(dev))
        check(rc, "gespmm_csr_spmm_x16")
        return out
    cref = ctypes.byref(c) if c is not None else None
    # scratch for the cache-blocked / long-row paths from torch's allocator (see torch_binding.cpp)
    ws_bytes = lib.gespmm_csr_spmm_workspace_bytes(M, K, N, nnz, int(variant), cref)
    if ws_bytes < 0:
        check(int(ws_bytes), "gespmm_csr_spmm_workspace_bytes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes > 0 else None
    with _on_device(dev):
        rc = lib.gespmm_csr_spmm_f32_ws(_ptr(rowptr), _ptr(colind), _ptr(values) if values is not None else None,
                                        _ptr(dense), _ptr(out), M, K, N, nnz, int(variant), cref,
                                        _ptr(ws) if ws is not None else None, ws_bytes, _stream(dev))
    check(rc, "gespmm_csr_spmm_f32")
    return out


def csr_spmm(rowptr, colind, values, dense, variant=_lib.VARIANT_AUTO, cfg=None, out=None, plan=None):
    """C = A @ dense with A = CSR(rowptr, colind, values). Mirrors spmm.cpp:24-43. ``dense`` may be fp16 / bf16 (see the module text)."""
    if values is None:
        raise TypeError("csr_spmm needs edge values; use csr_spmm_no_edge_value for A == 1")
    if _ext is not None and cfg is None and out is None and plan is None:
        return _ext.csr_spmm(rowptr, colind, values, dense, int(variant))
    return _spmm(rowptr, colind, values, dense, variant, cfg, out, plan)


def csr_spmm_no_edge_value(rowptr, colind, dense, variant=_lib.VARIANT_AUTO, cfg=None, out=None, plan=None):
    """C = A @ dense with A == 1 on its pattern. Mirrors spmm.cpp:45-60. ``dense`` may be fp16 / bf16 (see the module text)."""
    if _ext is not None and cfg is None and out is None and plan is None:
        return _ext.csr_spmm_no_edge_value(rowptr, colind, dense, int(variant))
    return _spmm(rowptr, colind, None, dense, variant, cfg, out, plan)


def csr_spmm_max(rowptr, colind, dense, empty_value=-10000.0, variant=_lib.VARIANT_AUTO):
    """C[r, :] = max over neighbours of dense[col, :] (DGL max reducer,
    binary_reduce_max.cu:182-207; rows without neighbours give ``empty_value``, the
    reference's hard-coded -10000). fp32 only."""
    if _ext is not None:
        return _ext.csr_spmm_max(rowptr, colind, dense, float(empty_value), int(variant))
    _need(rowptr, "rowptr", torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    _need(dense, "dense", torch.float32, 2)
    dev = _same_device(dense, rowptr, colind)
    M = rowptr.numel() - 1
    K, N = dense.shape
    out = torch.empty((M, N), dtype=torch.float32, device=dev)
    with _on_device(dev):
        rc = lib.gespmm_csr_spmm_max_f32(_ptr(rowptr), _ptr(colind), _ptr(dense), _ptr(out), M, K, N,
                                         colind.numel(), float(empty_value), int(variant), _stream(dev))
    check(rc, "gespmm_csr_spmm_max_f32")
    return out


def _result(t, name, dtype, shape, dev, inputs):
    """A caller's result tensor: contiguous ``dtype`` of ``shape`` on ``dev`` that overlaps no input."""
    _need(t, name, dtype, len(shape))
    if tuple(t.shape) != tuple(shape) or t.device != dev:
        raise ValueError("%s must be %s%s on %s" % (name, dtype, list(shape), dev))
    if any(_overlaps(t, x) for x in inputs):
        raise ValueError("%s must not overlap an input" % name)
    return t


def csr_spmm_max_arg(rowptr, colind, dense, empty_value=-10000.0, out=None, arg=None):
    """``csr_spmm_max`` that also says which neighbour won (gespmm_csr_spmm_max_arg_f32): returns ``(out, arg)``, f32[M, N] and
    int32[M, N]. Per output word ONE chain over the row's entries in CSR order, ``if dense[colind[p], c] > acc: acc, a = that, p`` from
    ``(empty_value, -1)``: ``arg`` is a CSR POSITION (not a column id), the first of equal values wins (+0 == -0), NaN and values
    ``<= empty_value`` never win. ``out`` has the bits of ``csr_spmm_max`` wherever no zeros of both signs compete for a maximum.
    fp32 tensors only (fp16 / bf16: ``csr_spmm_max_arg_x16``); ``out=`` / ``arg=`` reuse the caller's tensors."""
    _need(rowptr, "rowptr", torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    _need(dense, "dense", torch.float32, 2)
    dev = _same_device(dense, rowptr, colind)
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have M+1 >= 1 entries")
    empty_value = float(empty_value)
    if empty_value != empty_value:
        raise ValueError("empty_value must not be NaN")
    M = rowptr.numel() - 1
    K, N = dense.shape
    out = torch.empty((M, N), dtype=torch.float32, device=dev) if out is None else _result(out, "out", torch.float32, (M, N), dev, (dense,))
    arg = torch.empty((M, N), dtype=torch.int32, device=dev) if arg is None else _result(arg, "arg", torch.int32, (M, N), dev, (dense, out))
    with _on_device(dev):
        rc = lib.gespmm_csr_spmm_max_arg_f32(_ptr(rowptr), _ptr(colind), _ptr(dense), _ptr(out), _ptr(arg), M, K, N, colind.numel(),
                                             empty_value, _stream(dev))
    check(rc, "gespmm_csr_spmm_max_arg_f32")
    return out, arg


def csr_spmm_max_backward(colptr, rowind, order, arg, grad_out, K, out=None):
    """The gradient of ``csr_spmm_max_arg`` for ``dense`` (gespmm_csr_spmm_max_backward_f32): f32[K, N] with
    ``out[k, c] = sum of grad_out[r, c] over the entries (r, k) whose position arg[r, c] names`` — per word one fp32 add chain from +0 in
    CSC order, no atomics: bit-reproducible. ``(colptr, rowind)`` are the CSC arrays of the pattern and ``order`` (int32) maps a CSC
    position to its CSR position: ``graphs.transpose_csr(..., return_order=True)``, cast to int32. Nodes no row chose get +0."""
    _need(colptr, "colptr", torch.int32, 1)
    _need(rowind, "rowind", torch.int32, 1)
    _need(order, "order", torch.int32, 1)
    _need(grad_out, "grad_out", torch.float32, 2)
    _need(arg, "arg", torch.int32, 2)
    dev = _same_device(grad_out, colptr, rowind, order, arg)
    K = int(K)
    if colptr.numel() != K + 1:
        raise ValueError("colptr must have K + 1 = %d entries" % (K + 1))
    if order.numel() != rowind.numel():
        raise ValueError("order and rowind must have the same length")
    if tuple(arg.shape) != tuple(grad_out.shape):
        raise ValueError("arg must have the shape of grad_out, %s" % (list(grad_out.shape),))
    M, N = grad_out.shape
    out = torch.empty((K, N), dtype=torch.float32, device=dev) if out is None else _result(out, "out", torch.float32, (K, N), dev, (grad_out, arg))
    with _on_device(dev):
        rc = lib.gespmm_csr_spmm_max_backward_f32(_ptr(colptr), _ptr(rowind), _ptr(order), _ptr(arg), _ptr(grad_out), _ptr(out), M, K, N,
                                                  rowind.numel(), _stream(dev))
    check(rc, "gespmm_csr_spmm_max_backward_f32")
    return out


def _need_x16(t, name, sibling):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype not in _X16:
        raise TypeError("%s must have dtype torch.float16 or torch.bfloat16, got %s (fp32: %s)" % (name, t.dtype, sibling))
    _need(t, name, t.dtype, 2)


def csr_spmm_max_arg_x16(rowptr, colind, dense, empty_value=-10000.0, out=None, arg=None):
    """``csr_spmm_max_arg`` on 16-bit features (gespmm_csr_spmm_max_arg_x16): ``dense`` fp16 or bf16 [K, N]; returns ``(out, arg)``, ``out``
    in the dtype of ``dense`` and ``arg`` int32. A max rounds nothing: the chain runs in fp32 on the exactly widened elements, from
    ``empty_value`` as given, and ``out`` is narrowed once at the store — ``arg`` is that of ``csr_spmm_max_arg(.., dense.float(), ..)``
    and ``out`` has the bits of its result cast to the dtype (an ``empty_value`` the dtype cannot hold, -10000 in bf16, is rounded only
    where a row without a winner stores it). Any N and any 2-byte aligned tensor is served by one kernel; no allocation when ``out=`` and
    ``arg=`` are given."""
    _need(rowptr, "rowptr", torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    _need_x16(dense, "dense", "csr_spmm_max_arg")
    dev = _same_device(dense, rowptr, colind)
    if rowptr.numel() < 1:
        raise ValueError("rowptr must have M+1 >= 1 entries")
    empty_value = float(empty_value)
    if empty_value != empty_value:
        raise ValueError("empty_value must not be NaN")
    M = rowptr.numel() - 1
    K, N = dense.shape
    out = torch.empty((M, N), dtype=dense.dtype, device=dev) if out is None else _result(out, "out", dense.dtype, (M, N), dev, (dense,))
    arg = torch.empty((M, N), dtype=torch.int32, device=dev) if arg is None else _result(arg, "arg", torch.int32, (M, N), dev, (dense, out))
    with _on_device(dev):
        rc = lib.gespmm_csr_spmm_max_arg_x16(_ptr(rowptr), _ptr(colind), _ptr(dense), _ptr(out), _ptr(arg), M, K, N, colind.numel(),
                                             empty_value, _X16[dense.dtype], _stream(dev))
    check(rc, "gespmm_csr_spmm_max_arg_x16")
    return out, arg


def csr_spmm_max_backward_x16(colptr, rowind, order, arg, grad_out, K, out=None):
    """``csr_spmm_max_backward`` on a 16-bit ``grad_out`` (gespmm_csr_spmm_max_backward_x16): fp16 or bf16 [K, N] in its dtype. Per word
    one fp32 add chain from +0 in CSC order over the widened elements, rounded once at the store: the bits of
    ``csr_spmm_max_backward(.., grad_out.float(), K).to(grad_out.dtype)``. ``arg`` stays int32."""
    _need(colptr, "colptr", torch.int32, 1)
    _need(rowind, "rowind", torch.int32, 1)
    _need(order, "order", torch.int32, 1)
    _need_x16(grad_out, "grad_out", "csr_spmm_max_backward")
    _need(arg, "arg", torch.int32, 2)
    dev = _same_device(grad_out, colptr, rowind, order, arg)
    K = int(K)
    if colptr.numel() != K + 1:
        raise ValueError("colptr must have K + 1 = %d entries" % (K + 1))
    if order.numel() != rowind.numel():
        raise ValueError("order and rowind must have the same length")
    if tuple(arg.shape) != tuple(grad_out.shape):
        raise ValueError("arg must have the shape of grad_out, %s" % (list(grad_out.shape),))
    M, N = grad_out.shape
    out = torch.empty((K, N), dtype=grad_out.dtype, device=dev) if out is None else _result(out, "out", grad_out.dtype, (K, N), dev, (grad_out, arg))
    with _on_device(dev):
        rc = lib.gespmm_csr_spmm_max_backward_x16(_ptr(colptr), _ptr(rowind), _ptr(order), _ptr(arg), _ptr(grad_out), _ptr(out), M, K, N,
                                                  rowind.numel(), _X16[grad_out.dtype], _stream(dev))
    check(rc, "gespmm_csr_spmm_max_backward_x16")
    return out


def csr2csc(rowptr, colind, colptr, rowind, csr_data):
    """Fill ``colptr`` / ``rowind`` in place with the CSC form of CSR(rowptr, colind)
    and return the values in CSC order. Mirrors spmm.cpp:70-93 (whose CUDA
    implementation is unusable as shipped: spmm_kernel.cu:386 uses an uninitialised
    cuSPARSE handle). The number of columns is ``colptr.numel() - 1``."""
    if _ext is not None:
        return _ext.csr2csc(rowptr, colind, colptr, rowind, csr_data)
    _need(rowptr, "rowptr", torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    _need(colptr, "colptr", torch.int32, 1)
    _need(rowind, "rowind", torch.int32, 1)
    _need(csr_data, "csr_data", torch.float32, 1)
    dev = _same_device(rowptr, colind, colptr, rowind, csr_data)
    M = rowptr.numel() - 1
    K = colptr.numel() - 1
    nnz = colind.numel()
    if rowind.numel() != nnz or csr_data.numel() != nnz:
        raise ValueError("rowind and csr_data must have nnz entries")
    out = torch.empty((nnz,), dtype=torch.float32, device=dev)
    with _on_device(dev):
        ws_bytes = lib.gespmm_csr2csc_workspace_bytes(M, K, nnz)
        if ws_bytes < 0:
            check(int(ws_bytes), "gespmm_csr2csc_workspace_bytes")
        ws = torch.empty((max(int(ws_bytes), 1),), dtype=torch.uint8, device=dev)
        rc = lib.gespmm_csr2csc_f32(_ptr(rowptr), _ptr(colind), _ptr(csr_data), _ptr(colptr), _ptr(rowind),
                                    _ptr(out), M, K, nnz, _ptr(ws), _stream(dev))
    check(rc, "gespmm_csr2csc_f32")
    return out


def baseline_copy(src, out=None):
    """dst[i] = src[i] through the library's streaming-copy yardstick (gespmm_baseline_copy_f32) — NOT a product path:
    bench.py times it beside the product to price `ceiling_frac` with the read + write rate of the box."""
    _need(src, "src", torch.float32, src.dim())
    if out is None:
        out = torch.empty_like(src)
    _need(out, "out", torch.float32, src.dim())
    if out.numel() != src.numel():
        raise ValueError("out must have as many elements as src")
    dev = _same_device(src, out)
    with _on_device(dev):
        rc = lib.gespmm_baseline_copy_f32(_ptr(src), _ptr(out), src.numel(), _stream(dev))
    check(rc, "gespmm_baseline_copy_f32")
    return out


def select_variant(M, nnz, N):
    """The variant VARIANT_AUTO resolves to for this shape (host-only)."""
    return lib.gespmm_select_variant(int(M), int(nnz), int(N))
