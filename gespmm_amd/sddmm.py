"""Mirror of the reference's pybind11 module ``sddmm`` (pytorch-custom/sddmm.cpp:21-67):

    coo_sddmm(rowind, colind, D1, D2) -> f32[nnz]     sddmm.cpp:21-40
    csr_sddmm(rowptr, colind, D1, D2) -> f32[nnz]     sddmm.cpp:42-60

out[e] = <D1[row(e), :], D2[col(e), :]> in pattern order (sddmm.cu:7-424). As in the
reference the feature width is D1.size(1) and, for the CSR form, M = D1.size(0).

16-bit operands (extension): D1 and D2 may both be ``torch.float16`` or both ``torch.bfloat16`` (gespmm_sddmm_{coo,csr}_x16,
gespmm_plan_sddmm_x16: 16-bit kernels at every width and alignment, nothing is widened in memory). The result stays
``torch.float32[nnz]`` — edge values are fp32 everywhere in this package, so it feeds ``spmm.csr_spmm``'s ``values`` as it is — and
``csr_sddmm(rowptr, colind, grad_out, feat)`` is the edge-weight gradient of a ``.half()`` / ``.bfloat16()`` / autocast model, which
``SPMMFunction(need_edge_grad=True)`` does not compute. Mixed dtypes raise TypeError.

Multi-head form (extension; gespmm_sddmm_{coo,csr}_heads_f32, gespmm_plan_sddmm_heads_f32):

    coo_sddmm_heads(rowind, colind, D1, D2)                      -> f32[nnz, H]
    csr_sddmm_heads(rowptr, colind, D1, D2, out=None, plan=None) -> f32[nnz, H]

D1 f32[M, H, F], D2 f32[K, H, F]: out[e, h] = <D1[row(e), h, :], D2[col(e), h, :]> — the attention score of a dot-product attention
layer, or the edge-weight gradient of ``spmm.csr_spmm_heads`` — in ONE kernel that finds the row and column of an edge once for all
heads. Head h has the bits of ``csr_sddmm`` on ``D1[:, h, :].contiguous()`` and ``D2[:, h, :].contiguous()``. These two are fp32 only
(16-bit operands raise TypeError); fp16 / bf16 operands have names of their own (gespmm_sddmm_{coo,csr}_heads_x16):

    coo_sddmm_heads_x16(rowind, colind, D1, D2, out=None) -> f32[nnz, H]
    csr_sddmm_heads_x16(rowptr, colind, D1, D2, out=None) -> f32[nnz, H]

D1 and D2 both ``torch.float16`` or both ``torch.bfloat16``; head h has the bits of the 16-bit ``csr_sddmm`` on the contiguous slices.

GATv2 edge score (extension; gespmm_gatv2_score_f32, gespmm_gatv2_score_backward_f32):

    gatv2_score(rowptr, colind, xl, xr, att, negative_slope=0.2, out=None)                         -> f32[nnz, H]
    gatv2_score_backward(ptr, ind, grad_score, x_seg, x_ind, att, negative_slope=0.2, order=None,
                         want_att_part=False, out=None)                                            -> grad_x f32[S, H, F] (, att_part)

score[p, h] = sum_f att[h, f] leaky_relu(xl[row(p), h, f] + xr[col(p), h, f]) — the non-linearity inside the sum, so the score is no
dot product of a row term and a column term — in ONE kernel, and its gradients in one kernel that serves both node terms; nothing of
size nnz * H * F exists in either direction. CSR form only. These two are fp32 only (16-bit operands raise TypeError); fp16 / bf16 node
terms have names of their own (gespmm_gatv2_score_x16, gespmm_gatv2_score_backward_x16):

    gatv2_score_x16(rowptr, colind, xl, xr, att, negative_slope=0.2, out=None)                     -> f32[nnz, H]
    gatv2_score_backward_x16(ptr, ind, grad_score, x_seg, x_ind, att, negative_slope=0.2, order=None,
                             want_att_part=False, out=None)                                        -> grad_x 16-bit [S, H, F] (, att_part f32)

xl / xr (x_seg / x_ind) both ``torch.float16`` or both ``torch.bfloat16``; ``att``, ``grad_score``, the score and ``att_part`` stay fp32.
The arithmetic is that of the fp32 pair on the exactly widened elements; ``grad_x`` is rounded once, to nearest even.
"""
import torch

from ._ext import ext as _ext
from ._lib import check, lib
from .spmm import _need, _need_dense, _on_device, _ptr, _same_device, _stream


def _checked(idx0, name0, colind, D1, D2):
    """-> (device, GESPMM_X16_* code of the operands or 0 for fp32)"""
    _need(idx0, name0, torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    x16 = _need_dense(D1, "D1")
    _need(D2, "D2", D1.dtype, 2)
    if D1.shape[1] != D2.shape[1]:
        raise ValueError("D1 and D2 must have the same number of columns")
    return _same_device(D1, D2, idx0, colind), x16


def coo_sddmm(rowind, colind, D1, D2):
    if _ext is not None:
        return _ext.coo_sddmm(rowind, colind, D1, D2)
    dev, x16 = _checked(rowind, "rowind", colind, D1, D2)
    nnz = rowind.numel()
    if colind.numel() != nnz:
        raise ValueError("rowind and colind must have the same length")
    out = torch.empty((nnz,), dtype=torch.float32, device=dev)
    with _on_device(dev):
        if x16:
            rc = lib.gespmm_sddmm_coo_x16(_ptr(rowind), _ptr(colind), _ptr(D1), _ptr(D2), _ptr(out), x16, nnz, D1.shape[1], _stream(dev))
        else:
            rc = lib.gespmm_sddmm_coo_f32(_ptr(rowind), _ptr(colind), _ptr(D1), _ptr(D2), _ptr(out), nnz,
                                          D1.shape[1], _stream(dev))
    check(rc, "gespmm_sddmm_coo_x16" if x16 else "gespmm_sddmm_coo_f32")
    return out


def csr_sddmm(rowptr, colind, D1, D2, plan=None):
    """``plan``: a ``spmm.SpmmPlan`` of the same pattern — a clustered plan walks the edges in its own order (rows of D2
    shared by neighbouring rows come from L2) and returns the same bits in the caller's edge order."""
    if plan is not None:
        dev, x16 = _checked(rowptr, "rowptr", colind, D1, D2)
        if (rowptr.data_ptr(), colind.data_ptr()) != (plan._rowptr.data_ptr(), plan._colind.data_ptr()) or \
                (rowptr._version, colind._version) != plan._pattern_version:
            raise ValueError("the plan was made for a different (or since modified) pattern")
        if D1.shape[0] != rowptr.numel() - 1:
            raise ValueError("rowptr must have D1.size(0)+1 entries")
        if _ext is not None and hasattr(_ext, "plan_sddmm"):
            return _ext.plan_sddmm(plan._handle.value, D1, D2, colind.numel())
        out = torch.empty((colind.numel(),), dtype=torch.float32, device=dev)
        with _on_device(dev):
            if x16:
                rc = lib.gespmm_plan_sddmm_x16(plan._handle, _ptr(D1), _ptr(D2), _ptr(out), x16, D1.shape[1], _stream(dev))
            else:
                rc = lib.gespmm_plan_sddmm_f32(plan._handle, _ptr(D1), _ptr(D2), _ptr(out), D1.shape[1], _stream(dev))
        check(rc, "gespmm_plan_sddmm_x16" if x16 else "gespmm_plan_sddmm_f32")
        return out
    if _ext is not None:
        return _ext.csr_sddmm(rowptr, colind, D1, D2)
    dev, x16 = _checked(rowptr, "rowptr", colind, D1, D2)
    M = D1.shape[0]
    if rowptr.numel() != M + 1:
        raise ValueError("rowptr must have D1.size(0)+1 entries")
    nnz = colind.numel()
    out = torch.empty((nnz,), dtype=torch.float32, device=dev)
    with _on_device(dev):
        if x16:
            rc = lib.gespmm_sddmm_csr_x16(_ptr(rowptr), _ptr(colind), _ptr(D1), _ptr(D2), _ptr(out), x16, M, nnz, D1.shape[1], _stream(dev))
        else:
            rc = lib.gespmm_sddmm_csr_f32(_ptr(rowptr), _ptr(colind), _ptr(D1), _ptr(D2), _ptr(out), M, nnz,
                                          D1.shape[1], _stream(dev))
    check(rc, "gespmm_sddmm_csr_x16" if x16 else "gespmm_sddmm_csr_f32")
    return out


def _checked_heads(idx0, name0, colind, D1, D2):
    """-> (device, H, F) of the multi-head forms: rank-3 fp32 operands (H comes from the shape), same H and F on both sides."""
    _need(idx0, name0, torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    for t, name in ((D1, "D1"), (D2, "D2")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dim() != 3:
            raise ValueError("%s must be [rows, H, F]" % name)
        _need(t, name, torch.float32, 3)  # (16-bit operands have no multi-head entry: TypeError)
    if D1.shape[1:] != D2.shape[1:]:
        raise ValueError("D1 %s and D2 %s must have the same heads and columns" % (tuple(D1.shape), tuple(D2.shape)))
    if D1.shape[1] < 1:
        raise ValueError("D1 and D2 must have at least one head")
    return _same_device(D1, D2, idx0, colind), D1.shape[1], D1.shape[2]


def _heads_out(out, nnz, H, dev):
    if out is None:
        return torch.empty((nnz, H), dtype=torch.float32, device=dev)
    _need(out, "out", torch.float32, 2)
    if tuple(out.shape) != (nnz, H) or out.device != dev:
        raise ValueError("out must be f32[%d, %d] on the same device" % (nnz, H))
    return out


def coo_sddmm_heads(rowind, colind, D1, D2, out=None):
    """``out[e, h] = <D1[rowind[e], h, :], D2[colind[e], h, :]>`` (gespmm_sddmm_coo_heads_f32); see ``csr_sddmm_heads``."""
    dev, H, F = _checked_heads(rowind, "rowind", colind, D1, D2)
    nnz = rowind.numel()
    if colind.numel() != nnz:
        raise ValueError("rowind and colind must have the same length")
    out = _heads_out(out, nnz, H, dev)
    with _on_device(dev):
        rc = lib.gespmm_sddmm_coo_heads_f32(_ptr(rowind), _ptr(colind), _ptr(D1), _ptr(D2), _ptr(out), H, F, nnz, _stream(dev))
    check(rc, "gespmm_sddmm_coo_heads_f32")
    return out


def csr_sddmm_heads(rowptr, colind, D1, D2, out=None, plan=None):
    """Multi-head SDDMM: ``out[e, h] = <D1[row(e), h, :], D2[col(e), h, :]>`` for every edge e of the CSR pattern, D1 f32[M, H, F], D2
    f32[K, H, F], result f32[nnz, H] (gespmm_sddmm_csr_heads_f32 / gespmm_plan_sddmm_heads_f32). Head h has the bits of
    ``csr_sddmm(rowptr, colind, D1[:, h, :].contiguous(), D2[:, h, :].contiguous())``. One kernel for H >= 2 while nnz * H stays
    below 2^31 - 4096, a per-head composition beyond (``_lib.describe_sddmm_heads``). ``plan``: a
    ``spmm.SpmmPlan`` of the same pattern, as in ``csr_sddmm`` (``plan.sddmm_heads_route(H, F)``): same bits."""
    dev, H, F = _checked_heads(rowptr, "rowptr", colind, D1, D2)
    M, nnz = D1.shape[0], colind.numel()
    if rowptr.numel() != M + 1:
        raise ValueError("rowptr must have D1.size(0)+1 entries")
    if plan is not None and ((rowptr.data_ptr(), colind.data_ptr()) != (plan._rowptr.data_ptr(), plan._colind.data_ptr()) or
                             (rowptr._version, colind._version) != plan._pattern_version):
        raise ValueError("the plan was made for a different (or since modified) pattern")
    out = _heads_out(out, nnz, H, dev)
    with _on_device(dev):
        if plan is not None:
            rc = lib.gespmm_plan_sddmm_heads_f32(plan._handle, _ptr(D1), _ptr(D2), _ptr(out), H, F, _stream(dev))
        else:
            rc = lib.gespmm_sddmm_csr_heads_f32(_ptr(rowptr), _ptr(colind), _ptr(D1), _ptr(D2), _ptr(out), M, H, F, nnz, _stream(dev))
    check(rc, "gespmm_plan_sddmm_heads_f32" if plan is not None else "gespmm_sddmm_csr_heads_f32")
    return out


def _checked_heads_x16(idx0, name0, colind, D1, D2):
    """-> (device, H, F, GESPMM_X16_* code): rank-3 operands, both fp16 or both bf16, same H and F on both sides."""
    from .spmm import _X16

    _need(idx0, name0, torch.int32, 1)
    _need(colind, "colind", torch.int32, 1)
    for t, name in ((D1, "D1"), (D2, "D2")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    if D1.dtype not in _X16:
        raise TypeError("D1 must have dtype torch.float16 or torch.bfloat16, got %s (fp32: the functions without _x16)" % D1.dtype)
    for t, name in ((D1, "D1"), (D2, "D2")):
        if t.dim() != 3:
            raise ValueError("%s must be [rows, H, F]" % name)
        _need(t, name, D1.dtype, 3)  # (mixed 16-bit dtypes: TypeError)
    if D1.shape[1:] != D2.shape[1:]:
        raise ValueError("D1 %s and D2 %s must have the same heads and columns" % (tuple(D1.shape), tuple(D2.shape)))
    if D1.shape[1] < 1:
        raise ValueError("D1 and D2 must have at least one head")
    return _same_device(D1, D2, idx0, colind), D1.shape[1], D1.shape[2], _X16[D1.dtype]


def coo_sddmm_heads_x16(rowind, colind, D1, D2, out=None):
    """``coo_sddmm_heads`` on fp16 / bf16 operands (gespmm_sddmm_coo_heads_x16): the result stays f32[nnz, H]; see ``csr_sddmm_heads_x16``."""
    dev, H, F, x16 = _checked_heads_x16(rowind, "rowind", colind, D1, D2)
    nnz = rowind.numel()
    if colind.numel() != nnz:
        raise ValueError("rowind and colind must have the same length")
    out = _heads_out(out, nnz, H, dev)
    with _on_device(dev):
        rc = lib.gespmm_sddmm_coo_heads_x16(_ptr(rowind), _ptr(colind), _ptr(D1), _ptr(D2), _ptr(out), x16, H, F, nnz, _stream(dev))
    check(rc, "gespmm_sddmm_coo_heads_x16")
    return out


def csr_sddmm_heads_x16(rowptr, colind, D1, D2, out=None):
    """Multi-head SDDMM on 16-bit operands (gespmm_sddmm_csr_heads_x16): D1 [M, H, F] and D2 [K, H, F] both fp16 or both bf16, result
    f32[nnz, H] — the fp32 score of a 16-bit dot-product attention layer, or the fp32 edge-weight gradient of ``spmm.csr_spmm_heads_x16``.
    Every element is widened exactly at its FMA; head h has the bits of ``csr_sddmm(rowptr, colind, D1[:, h, :].contiguous(),
    D2[:, h, :].contiguous())`` (``_lib.describe_sddmm_heads(..., x16=True)``). No plan form."""
    dev, H, F, x16 = _checked_heads_x16(rowptr, "rowptr", colind, D1, D2)
    M, nnz = D1.shape[0], colind.numel()
    if rowptr.numel() != M + 1:
        raise ValueError("rowptr must have D1.size(0)+1 entries")
    out = _heads_out(out, nnz, H, dev)
    with _on_device(dev):
        rc = lib.gespmm_sddmm_csr_heads_x16(_ptr(rowptr), _ptr(colind), _ptr(D1), _ptr(D2), _ptr(out), x16, M, H, F, nnz, _stream(dev))
    check(rc, "gespmm_sddmm_csr_heads_x16")
    return out


# ---- GATv2 edge score (extension; gespmm_gatv2_score_f32 / gespmm_gatv2_score_backward_f32)

def _gatv2_typed(int_ops, float_ops):
    """TypeError for every operand that is no tensor of its dtype — before any shape is looked at (``None`` passes)."""
    for dtype, ops in ((torch.int32, int_ops), (torch.float32, float_ops)):
        for name, t in ops:
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch.Tensor" % name)
            if t.dtype != dtype:  # (16-bit and fp64 operands have no entry point: TypeError)
                raise TypeError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))


def _gatv2_slope(negative_slope):
    if negative_slope is None:
        return 1.0
    s = float(negative_slope)
    if s != s or s in (float("inf"), float("-inf")):
        raise ValueError("negative_slope must be finite, got %r" % (negative_slope,))
    return s


def _gatv2_shaped(named, dev):
    """ValueError for what is not contiguous or not on ``dev`` (shapes were checked by the caller)."""
    for name, t in named:
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        if t.device != dev:
            raise ValueError("%s must live on %s, as the other operands" % (name, dev))
    if dev.type != "cuda":
        raise ValueError("the operands must be HIP (cuda) device tensors; gespmm_amd has no CPU path")


def gatv2_score(rowptr, colind, xl, xr, att, negative_slope=0.2, out=None):
    """The GATv2 attention score (Brody et al.) on the entries of a CSR pattern, H heads in ONE launch (gespmm_gatv2_score_f32):

        score[p, h] = sum_f att[h, f] * leaky_relu(xl[row(p), h, f] + xr[colind[p], h, f], negative_slope)

    ``xl`` f32[M, H, F] is the aggregating node's term, ``xr`` f32[K, H, F] the neighbour's, ``att`` f32[H, F]; the result is f32[nnz, H]
    in CSR entry order — what ``softmax.edge_softmax`` reads. Nothing of size nnz * H * F exists. ``negative_slope=None``: no leaky
    ReLU. ``out``: an f32[nnz, H] tensor to write into. The summation order is pinned by ``_lib.describe_gatv2_score`` (include/gespmm.h).
    ``colind`` within [0, K) and ``rowptr[M] == nnz`` are preconditions. fp32 only: other dtypes raise TypeError."""
    _gatv2_typed((("rowptr", rowptr), ("colind", colind)), (("xl", xl), ("xr", xr), ("att", att), ("out", out)))
    for name, t in (("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att)):
        if t is None:
            raise TypeError("%s must be a torch.Tensor" % name)
    slope = _gatv2_slope(negative_slope)
    if xl.dim() != 3 or xr.dim() != 3 or xl.shape[1] < 1:
        raise ValueError("xl and xr must be [rows, H, F] with at least one head")
    M, H, F = xl.shape
    K = xr.shape[0]
    if tuple(xr.shape[1:]) != (H, F):
        raise ValueError("xl %s and xr %s must have the same heads and columns" % (tuple(xl.shape), tuple(xr.shape)))
    if tuple(att.shape) != (H, F):
        raise ValueError("att must be f32[%d, %d], got %s" % (H, F, tuple(att.shape)))
    if rowptr.dim() != 1 or rowptr.numel() != M + 1:
        raise ValueError("rowptr must be a vector of xl.size(0) + 1 entries")
    if colind.dim() != 1:
        raise ValueError("colind must be a vector")
    nnz = colind.numel()
    if out is not None and tuple(out.shape) != (nnz, H):
        raise ValueError("out must be f32[%d, %d]" % (nnz, H))
    dev = xl.device
    _gatv2_shaped((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att), ("out", out)), dev)
    if out is None:
        out = torch.empty((nnz, H), dtype=torch.float32, device=dev)
    with _on_device(dev):
        rc = lib.gespmm_gatv2_score_f32(_ptr(rowptr), _ptr(colind), _ptr(xl), _ptr(xr), _ptr(att), _ptr(out), M, K, H, F, nnz, slope,
                                        _stream(dev))
    check(rc, "gespmm_gatv2_score_f32")
    return out


def gatv2_score_backward(ptr, ind, grad_score, x_seg, x_ind, att, negative_slope=0.2, order=None, want_att_part=False, out=None):
    """The gradient of ``gatv2_score`` for one node term, over the segments ``(ptr, ind)`` describe (gespmm_gatv2_score_backward_f32):

        grad_x[s, h, f]   = sum over the entries p of segment s of grad_score[q, h] * (t >= 0 ? att[h, f] : att[h, f] * negative_slope)
        att_part[s, h, f] = sum over the entries p of segment s of grad_score[q, h] * leaky_relu(t, negative_slope)

    with ``t = x_seg[s, h, f] + x_ind[ind[p], h, f]`` and ``q = order[p]`` (``p`` without ``order``). Row pass — ``(rowptr, colind, grad_score,
    xl, xr, att, want_att_part=True)`` — returns ``(grad_xl, att_part)``, and ``att_part.sum(0)`` is the gradient of ``att``; column pass
    — ``(colptr, rowind, grad_score, xr, xl, att, order=csc_order)`` — returns ``grad_xr``. One fp32 chain per output word in segment
    order, whatever the lane geometry; every word is written (+0 for an empty segment). ``order`` is int32. ``out``: the f32[S, H, F]
    tensor for grad_x, or the pair ``(grad_x, att_part)`` with ``want_att_part``. Nothing of size nnz * H * F exists."""
    out_x, out_a = out if isinstance(out, (tuple, list)) and len(out) == 2 else (out, None)
    _gatv2_typed((("ptr", ptr), ("ind", ind), ("order", order)),
                 (("grad_score", grad_score), ("x_seg", x_seg), ("x_ind", x_ind), ("att", att), ("out", out_x), ("out[1]", out_a)))
    for name, t in (("ptr", ptr), ("ind", ind), ("grad_score", grad_score), ("x_seg", x_seg), ("x_ind", x_ind), ("att", att)):
        if t is None:
            raise TypeError("%s must be a torch.Tensor" % name)
    slope = _gatv2_slope(negative_slope)
    if x_seg.dim() != 3 or x_ind.dim() != 3 or x_seg.shape[1] < 1:
        raise ValueError("x_seg and x_ind must be [rows, H, F] with at least one head")
    S, H, F = x_seg.shape
    T = x_ind.shape[0]
    if tuple(x_ind.shape[1:]) != (H, F):
        raise ValueError("x_seg %s and x_ind %s must have the same heads and columns" % (tuple(x_seg.shape), tuple(x_ind.shape)))
    if tuple(att.shape) != (H, F):
        raise ValueError("att must be f32[%d, %d], got %s" % (H, F, tuple(att.shape)))
    if ptr.dim() != 1 or ptr.numel() != S + 1:
        raise ValueError("ptr must be a vector of x_seg.size(0) + 1 entries")
    if ind.dim() != 1:
        raise ValueError("ind must be a vector")
    nnz = ind.numel()
    if tuple(grad_score.shape) != (nnz, H):
        raise ValueError("grad_score must be f32[%d, %d], got %s" % (nnz, H, tuple(grad_score.shape)))
    if order is not None and tuple(order.shape) != (nnz,):
        raise ValueError("order must be a vector of %d entries" % nnz)
    if out_a is not None and not want_att_part:
        raise ValueError("out is a pair only with want_att_part")
    for name, t in (("out", out_x), ("out[1]", out_a)):
        if t is not None and tuple(t.shape) != (S, H, F):
            raise ValueError("%s must be f32[%d, %d, %d]" % (name, S, H, F))
    dev = x_seg.device
    _gatv2_shaped((("ptr", ptr), ("ind", ind), ("order", order), ("grad_score", grad_score), ("x_seg", x_seg), ("x_ind", x_ind),
                   ("att", att), ("out", out_x), ("out[1]", out_a)), dev)
    if out_x is None:
        out_x = torch.empty((S, H, F), dtype=torch.float32, device=dev)
    if want_att_part and out_a is None:
        out_a = torch.empty((S, H, F), dtype=torch.float32, device=dev)
    if out_x.numel() == 0:  # (results of no words have no address to hand over)
        return (out_x, out_a) if want_att_part else out_x
    with _on_device(dev):
        rc = lib.gespmm_gatv2_score_backward_f32(_ptr(ptr), _ptr(ind), _ptr(order) if order is not None else None, _ptr(grad_score),
                                                 _ptr(x_seg), _ptr(x_ind), _ptr(att), _ptr(out_x), _ptr(out_a) if want_att_part else None,
                                                 S, T, H, F, nnz, slope, _stream(dev))
    check(rc, "gespmm_gatv2_score_backward_f32")
    return (out_x, out_a) if want_att_part else out_x


# ---- ... on fp16 / bf16 node operands (gespmm_gatv2_score_x16 / gespmm_gatv2_score_backward_x16)

def _gatv2_typed_x16(int_ops, node_ops, float_ops):
    """``_gatv2_typed`` with a third class: the node operands, all ``torch.float16`` or all ``torch.bfloat16`` -> the GESPMM_X16_* code.
    The first of them names the type (``None`` passes, but not there)."""
    from .spmm import _X16

    _gatv2_typed(int_ops, float_ops)
    first_name, first = node_ops[0]
    if not isinstance(first, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % first_name)
    if first.dtype not in _X16:
        raise TypeError("%s must have dtype torch.float16 or torch.bfloat16, got %s (fp32: the functions without _x16)" %
                        (first_name, first.dtype))
    for name, t in node_ops[1:]:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != first.dtype:  # (mixed 16-bit dtypes and fp32 node operands: TypeError)
            raise TypeError("%s must have dtype %s, as %s, got %s" % (name, first.dtype, first_name, t.dtype))
    return _X16[first.dtype]


def gatv2_score_x16(rowptr, colind, xl, xr, att, negative_slope=0.2, out=None):
    """``gatv2_score`` on 16-bit node terms (gespmm_gatv2_score_x16): ``xl`` [M, H, F] and ``xr`` [K, H, F] both ``torch.float16`` or both
    ``torch.bfloat16``, ``att`` f32[H, F], result f32[nnz, H] — everything edge-sized stays fp32. Every element is widened exactly at its
    use and the arithmetic is ``gatv2_score``'s: where ``_lib.describe_gatv2_score`` answers the same (V, W) with and without ``x16=True``
    the result has the bits of ``gatv2_score`` on ``xl.float(), xr.float()``. A 16-bit ``att`` or ``out``, fp32 node terms and mixed 16-bit
    dtypes raise TypeError."""
    x16 = _gatv2_typed_x16((("rowptr", rowptr), ("colind", colind)), (("xl", xl), ("xr", xr)), (("att", att), ("out", out)))
    for name, t in (("rowptr", rowptr), ("colind", colind), ("xr", xr), ("att", att)):
        if t is None:
            raise TypeError("%s must be a torch.Tensor" % name)
    slope = _gatv2_slope(negative_slope)
    if xl.dim() != 3 or xr.dim() != 3 or xl.shape[1] < 1:
        raise ValueError("xl and xr must be [rows, H, F] with at least one head")
    M, H, F = xl.shape
    K = xr.shape[0]
    if tuple(xr.shape[1:]) != (H, F):
        raise ValueError("xl %s and xr %s must have the same heads and columns" % (tuple(xl.shape), tuple(xr.shape)))
    if tuple(att.shape) != (H, F):
        raise ValueError("att must be f32[%d, %d], got %s" % (H, F, tuple(att.shape)))
    if rowptr.dim() != 1 or rowptr.numel() != M + 1:
        raise ValueError("rowptr must be a vector of xl.size(0) + 1 entries")
    if colind.dim() != 1:
        raise ValueError("colind must be a vector")
    nnz = colind.numel()
    if out is not None and tuple(out.shape) != (nnz, H):
        raise ValueError("out must be f32[%d, %d]" % (nnz, H))
    dev = xl.device
    _gatv2_shaped((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att), ("out", out)), dev)
    if out is None:
        out = torch.empty((nnz, H), dtype=torch.float32, device=dev)
    with _on_device(dev):
        rc = lib.gespmm_gatv2_score_x16(_ptr(rowptr), _ptr(colind), _ptr(xl), _ptr(xr), _ptr(att), _ptr(out), x16, M, K, H, F, nnz, slope,
                                        _stream(dev))
    check(rc, "gespmm_gatv2_score_x16")
    return out


def gatv2_score_backward_x16(ptr, ind, grad_score, x_seg, x_ind, att, negative_slope=0.2, order=None, want_att_part=False, out=None):
    """``gatv2_score_backward`` on 16-bit node terms (gespmm_gatv2_score_backward_x16): ``x_seg`` [S, H, F] and ``x_ind`` [T, H, F] both
    ``torch.float16`` or both ``torch.bfloat16``, ``grad_score`` f32[nnz, H] and ``att`` f32[H, F]. ``grad_x`` comes back in the operands'
    dtype — the fp32 chain of ``gatv2_score_backward`` on the widened operands, rounded ONCE to nearest even — and ``att_part`` (with
    ``want_att_part``) stays f32[S, H, F] with that call's bits. ``out``: the 16-bit [S, H, F] tensor for grad_x, or the pair ``(grad_x,
    att_part)``. A 16-bit ``att`` or ``grad_score``, fp32 node terms and mixed 16-bit dtypes raise TypeError."""
    out_x, out_a = out if isinstance(out, (tuple, list)) and len(out) == 2 else (out, None)
    x16 = _gatv2_typed_x16((("ptr", ptr), ("ind", ind), ("order", order)), (("x_seg", x_seg), ("x_ind", x_ind), ("out", out_x)),
                           (("grad_score", grad_score), ("att", att), ("out[1]", out_a)))
    for name, t in (("ptr", ptr), ("ind", ind), ("grad_score", grad_score), ("x_ind", x_ind), ("att", att)):
        if t is None:
            raise TypeError("%s must be a torch.Tensor" % name)
    slope = _gatv2_slope(negative_slope)
    if x_seg.dim() != 3 or x_ind.dim() != 3 or x_seg.shape[1] < 1:
        raise ValueError("x_seg and x_ind must be [rows, H, F] with at least one head")
    S, H, F = x_seg.shape
    T = x_ind.shape[0]
    if tuple(x_ind.shape[1:]) != (H, F):
        raise ValueError("x_seg %s and x_ind %s must have the same heads and columns" % (tuple(x_seg.shape), tuple(x_ind.shape)))
    if tuple(att.shape) != (H, F):
        raise ValueError("att must be f32[%d, %d], got %s" % (H, F, tuple(att.shape)))
    if ptr.dim() != 1 or ptr.numel() != S + 1:
        raise ValueError("ptr must be a vector of x_seg.size(0) + 1 entries")
    if ind.dim() != 1:
        raise ValueError("ind must be a vector")
    nnz = ind.numel()
    if tuple(grad_score.shape) != (nnz, H):
        raise ValueError("grad_score must be f32[%d, %d], got %s" % (nnz, H, tuple(grad_score.shape)))
    if order is not None and tuple(order.shape) != (nnz,):
        raise ValueError("order must be a vector of %d entries" % nnz)
    if out_a is not None and not want_att_part:
        raise ValueError("out is a pair only with want_att_part")
    for name, t in (("out", out_x), ("out[1]", out_a)):
        if t is not None and tuple(t.shape) != (S, H, F):
            raise ValueError("%s must be [%d, %d, %d]" % (name, S, H, F))
    dev = x_seg.device
    _gatv2_shaped((("ptr", ptr), ("ind", ind), ("order", order), ("grad_score", grad_score), ("x_seg", x_seg), ("x_ind", x_ind),
                   ("att", att), ("out", out_x), ("out[1]", out_a)), dev)
    if out_x is None:
        out_x = torch.empty((S, H, F), dtype=x_seg.dtype, device=dev)
    if want_att_part and out_a is None:
        out_a = torch.empty((S, H, F), dtype=torch.float32, device=dev)
    if out_x.numel() == 0:  # (results of no words have no address to hand over)
        return (out_x, out_a) if want_att_part else out_x
    with _on_device(dev):
        rc = lib.gespmm_gatv2_score_backward_x16(_ptr(ptr), _ptr(ind), _ptr(order) if order is not None else None, _ptr(grad_score),
                                                 _ptr(x_seg), _ptr(x_ind), _ptr(att), _ptr(out_x), _ptr(out_a) if want_att_part else None,
                                                 x16, S, T, H, F, nnz, slope, _stream(dev))
    check(rc, "gespmm_gatv2_score_backward_x16")
    return (out_x, out_a) if want_att_part else out_x

