"""Fused scaled dot-product attention over the entries of a sparsity pattern (extension: no reference counterpart; the attention of
PyG's TransformerConv, of graph transformers and UniMP), forward and backward, with nothing of size nnz but the index arrays.

    dot_attention(rowptr, colind, q, k, v, scale=None, dropout=None, out=None, stats=None)                  -> (out f32[M, H, F], stats f32[M, H, 2])
    dot_attention_backward_q(rowptr, colind, q, k, v, stats, out, grad_out, scale=None, dropout=None, results=None)       -> (delta f32[M, H], grad_q f32[M, H, F])
    dot_attention_backward_kv(colptr, rowind, q, k, v, stats, delta, grad_out, scale=None, dropout=None, results=None)    -> (grad_k, grad_v) f32[K, H, F]

``q`` f32[M, H, F] is the aggregating node's term (the row of an entry), ``k`` and ``v`` f32[K, H, F] the neighbour's (the column). For
entry p of row r with column c and head h

    s_p = scale * <q[r, h, :], k[c, h, :]>      a_p = exp(s_p - m) / l,  stats[r, h] = (m, l) = (max_p s_p, sum_p exp(s_p - m))
    out[r, h, :] = sum_p a_p v[c, h, :]

``scale`` defaults to ``1 / sqrt(F)``. The forward is one sweep with an online softmax; the backward is a walk over the rows
(``delta = <grad_out, out>`` and ``grad_q``) and a walk over the columns on the CSC arrays of ``graphs.transpose_csr`` (``grad_k``,
``grad_v``; no ``csc_order``), both recomputing ``s_p`` and ``a_p`` with the same bits. ``dropout=(p, seed)`` puts ``softmax.edge_dropout``'s
mask on ``a_p``: the decision of an entry is a function of ``(seed, row, column, head)``, recomputed wherever it is needed. Lane geometry
and summation orders: include/gespmm.h and ``_lib.describe_dot_attention``. A head slice wider than 512 floats has no kernel: the calls
raise a ``GespmmError`` that says so. fp32 only: other dtypes raise TypeError. All calls go through ctypes."""
import math

import torch

from ._lib import DOT_ATTENTION_MAX_F, ERR_UNSUPPORTED, GespmmError, check, lib
from .softmax import _dropout, _dropout_typed
from .spmm import _on_device, _ptr, _stream


class DotAttentionUnsupported(GespmmError):
    """F > 512: no kernel serves the shape and nothing was launched."""

    def __init__(self, F, where):
        RuntimeError.__init__(self, "%s: a head slice of F = %d floats has no kernel; the fused dot-product attention serves F <= %d "
                                    "(code %d)" % (where, F, DOT_ATTENTION_MAX_F, ERR_UNSUPPORTED))
        self.code = ERR_UNSUPPORTED


def _typed(int_ops, float_ops):
    """TypeError for every operand that is no tensor of its dtype — before any shape is looked at (``None`` passes)."""
    for dtype, ops in ((torch.int32, int_ops), (torch.float32, float_ops)):
        for name, t in ops:
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch.Tensor" % name)
            if t.dtype != dtype:
                raise TypeError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))


def _required(named):
    for name, t in named:
        if t is None:
            raise TypeError("%s must be a torch.Tensor" % name)


def _scale(scale, F):
    if scale is None:
        return 1.0 / math.sqrt(F) if F > 0 else 1.0
    if isinstance(scale, torch.Tensor) or not isinstance(scale, (int, float)):
        raise TypeError("scale must be a Python number")
    s = float(scale)
    if s != s or s in (float("inf"), float("-inf")):
        raise ValueError("scale must be finite, got %r" % (scale,))
    return s


def _placed(named, dev):
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


def _shapes(ptr, ptr_name, ind, ind_name, q, k, v, segments_are_rows):
    """(M, K, H, F, nnz) of a call whose segments are the rows of q (forward, q-pass) or of k (k/v-pass)."""
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or q.shape[1] < 1:
        raise ValueError("q, k and v must be [rows, H, F] with at least one head")
    M, H, F = q.shape
    K = k.shape[0]
    if tuple(k.shape[1:]) != (H, F) or tuple(v.shape) != tuple(k.shape):
        raise ValueError("q %s, k %s and v %s must have the same heads and columns, k and v the same rows" %
                         (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    S = M if segments_are_rows else K
    if ptr.dim() != 1 or ptr.numel() != S + 1:
        raise ValueError("%s must be a vector of %d + 1 entries" % (ptr_name, S))
    if ind.dim() != 1:
        raise ValueError("%s must be a vector" % ind_name)
    return M, K, H, F, ind.numel()


def _shaped(t, name, shape):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be f32%s, got %s" % (name, list(shape), tuple(t.shape)))


def _pair(results):
    if results is None:
        return None, None
    if not isinstance(results, (tuple, list)) or len(results) != 2 or any(t is None for t in results):
        raise TypeError("results must be a pair of tensors")
    return results


def _served(F, where):
    if F > DOT_ATTENTION_MAX_F:
        raise DotAttentionUnsupported(F, where)


def dot_attention(rowptr, colind, q, k, v, scale=None, dropout=None, out=None, stats=None):
    """``out[r, h, :] = sum_p softmax_row(scale <q[r, h], k[c_p, h]>)_p v[c_p, h, :]`` over the entries of CSR row r, H heads in ONE
    launch (gespmm_dot_attention_f32): no score, no alpha, nothing of size nnz. Returns ``(out, stats)``; ``stats[r, h] = (m, l)`` is
    what the backward needs. Every word is written, an empty row +0. ``dropout=(p, seed)``: dropout on the coefficients after the
    normalisation (gespmm_dot_attention_dropout_f32). ``out`` / ``stats``: tensors to write into. ``colind`` within [0, K) and
    ``rowptr[M] == nnz`` are preconditions."""
    _typed((("rowptr", rowptr), ("colind", colind)), (("q", q), ("k", k), ("v", v), ("out", out), ("stats", stats)))
    _required((("rowptr", rowptr), ("colind", colind), ("q", q), ("k", k), ("v", v)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _shapes(rowptr, "rowptr", colind, "colind", q, k, v, True)
    sc = _scale(scale, F)
    _shaped(out, "out", (M, H, F))
    _shaped(stats, "stats", (M, H, 2))
    dev = q.device
    _placed((("rowptr", rowptr), ("colind", colind), ("q", q), ("k", k), ("v", v), ("out", out), ("stats", stats)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _served(F, "gespmm_dot_attention_f32")
    if out is None:
        out = torch.empty((M, H, F), dtype=torch.float32, device=dev)
    if stats is None:
        stats = torch.empty((M, H, 2), dtype=torch.float32, device=dev)
    if M == 0:  # (results of no words have no address to hand over)
        return out, stats
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_dot_attention_dropout_f32(_ptr(rowptr), _ptr(colind), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(stats), M, K, H,
                                                      F, nnz, sc, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_dot_attention_f32(_ptr(rowptr), _ptr(colind), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(stats), M, K, H, F, nnz,
                                              sc, _stream(dev))
    check(rc, "gespmm_dot_attention_dropout_f32" if dropout is not None else "gespmm_dot_attention_f32")
    return out, stats


def dot_attention_backward_q(rowptr, colind, q, k, v, stats, out, grad_out, scale=None, dropout=None, results=None):
    """The row pass of ``dot_attention``'s backward (gespmm_dot_attention_backward_q_f32): ``delta[r, h] = <grad_out[r, h], out[r, h]>``
    and ``grad_q[r, h, :] = scale * sum_p a_p (<grad_out[r, h], v[c_p, h]> - delta[r, h]) k[c_p, h, :]``. ``stats`` and ``out`` are the
    forward's results; ``dropout`` the forward's pair. Returns ``(delta, grad_q)``; every word is written. ``results``: a pair of tensors
    ``(delta, grad_q)`` to write into."""
    delta, grad_q = _pair(results)
    _typed((("rowptr", rowptr), ("colind", colind)),
           (("q", q), ("k", k), ("v", v), ("stats", stats), ("out", out), ("grad_out", grad_out), ("results[0]", delta),
            ("results[1]", grad_q)))
    _required((("rowptr", rowptr), ("colind", colind), ("q", q), ("k", k), ("v", v), ("stats", stats), ("out", out), ("grad_out", grad_out)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _shapes(rowptr, "rowptr", colind, "colind", q, k, v, True)
    sc = _scale(scale, F)
    _shaped(stats, "stats", (M, H, 2))
    _shaped(out, "out", (M, H, F))
    _shaped(grad_out, "grad_out", (M, H, F))
    _shaped(delta, "results[0]", (M, H))
    _shaped(grad_q, "results[1]", (M, H, F))
    dev = q.device
    _placed((("rowptr", rowptr), ("colind", colind), ("q", q), ("k", k), ("v", v), ("stats", stats), ("out", out), ("grad_out", grad_out),
             ("results[0]", delta), ("results[1]", grad_q)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _served(F, "gespmm_dot_attention_backward_q_f32")
    if delta is None:
        delta = torch.empty((M, H), dtype=torch.float32, device=dev)
        grad_q = torch.empty((M, H, F), dtype=torch.float32, device=dev)
    if M == 0:
        return delta, grad_q
    args = (_ptr(rowptr), _ptr(colind), _ptr(q), _ptr(k), _ptr(v), _ptr(stats), _ptr(out), _ptr(grad_out), _ptr(delta), _ptr(grad_q), M, K, H,
            F, nnz, sc)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_dot_attention_backward_q_dropout_f32(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_dot_attention_backward_q_f32(*args, _stream(dev))
    check(rc, "gespmm_dot_attention_backward_q_dropout_f32" if dropout is not None else "gespmm_dot_attention_backward_q_f32")
    return delta, grad_q


def dot_attention_backward_kv(colptr, rowind, q, k, v, stats, delta, grad_out, scale=None, dropout=None, results=None):
    """The column pass of ``dot_attention``'s backward (gespmm_dot_attention_backward_kv_f32) on the CSC arrays of the pattern
    (``graphs.transpose_csr``; no ``csc_order``): ``grad_k[c, h, :] = scale * sum over column c of ds_p q[r_p, h, :]`` and ``grad_v[c, h, :]
    = sum over column c of a_p grad_out[r_p, h, :]``, with ``ds_p`` and ``a_p`` the bits of the row pass. ``delta`` is the row pass's.
    Returns ``(grad_k, grad_v)``; every word is written, an empty column +0. ``results``: a pair ``(grad_k, grad_v)`` to write into."""
    grad_k, grad_v = _pair(results)
    _typed((("colptr", colptr), ("rowind", rowind)),
           (("q", q), ("k", k), ("v", v), ("stats", stats), ("delta", delta), ("grad_out", grad_out), ("results[0]", grad_k),
            ("results[1]", grad_v)))
    _required((("colptr", colptr), ("rowind", rowind), ("q", q), ("k", k), ("v", v), ("stats", stats), ("delta", delta),
               ("grad_out", grad_out)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _shapes(colptr, "colptr", rowind, "rowind", q, k, v, False)
    sc = _scale(scale, F)
    _shaped(stats, "stats", (M, H, 2))
    _shaped(delta, "delta", (M, H))
    _shaped(grad_out, "grad_out", (M, H, F))
    _shaped(grad_k, "results[0]", (K, H, F))
    _shaped(grad_v, "results[1]", (K, H, F))
    dev = q.device
    _placed((("colptr", colptr), ("rowind", rowind), ("q", q), ("k", k), ("v", v), ("stats", stats), ("delta", delta),
             ("grad_out", grad_out), ("results[0]", grad_k), ("results[1]", grad_v)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _served(F, "gespmm_dot_attention_backward_kv_f32")
    if grad_k is None:
        grad_k = torch.empty((K, H, F), dtype=torch.float32, device=dev)
        grad_v = torch.empty((K, H, F), dtype=torch.float32, device=dev)
    if K == 0:
        return grad_k, grad_v
    args = (_ptr(colptr), _ptr(rowind), _ptr(q), _ptr(k), _ptr(v), _ptr(stats), _ptr(delta), _ptr(grad_out), _ptr(grad_k), _ptr(grad_v), M, K,
            H, F, nnz, sc)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_dot_attention_backward_kv_dropout_f32(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_dot_attention_backward_kv_f32(*args, _stream(dev))
    check(rc, "gespmm_dot_attention_backward_kv_dropout_f32" if dropout is not None else "gespmm_dot_attention_backward_kv_f32")
    return grad_k, grad_v
