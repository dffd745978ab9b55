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
heads. Head h has the bits of ``csr_sddmm`` on ``D1[:, h, :].contiguous()`` and ``D2[:, h, :].contiguous()``. fp32 only: 16-bit
operands raise TypeError.
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
