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
raise a ``GespmmError`` that says so. These three names are fp32 only: other dtypes raise TypeError. All calls go through ctypes. On
fp16 / bf16 q, k and v (``stats`` and ``delta`` stay fp32; fp32 sums, every 16-bit result rounded once at its store):

    dot_attention_x16(rowptr, colind, q, k, v, scale=None, dropout=None, out=None, stats=None)               -> (out x16[M, H, F], stats f32[M, H, 2])
    dot_attention_backward_q_x16(rowptr, colind, q, k, v, stats, out, grad_out, scale=None, dropout=None, results=None)    -> (delta f32[M, H], grad_q x16[M, H, F])
    dot_attention_backward_kv_x16(colptr, rowind, q, k, v, stats, delta, grad_out, scale=None, dropout=None, results=None) -> (grad_k, grad_v) x16[K, H, F]

Where ``_lib.describe_dot_attention`` answers the same (V, W) with and without ``x16=True``, ``stats`` and ``delta`` have the bits of the
fp32 calls on the widened operands and ``out``, ``grad_q``, ``grad_k``, ``grad_v`` are theirs narrowed once.

Fused GATv2 attention (Brody et al.) — score, softmax and aggregation in one sweep, the same contract otherwise:

    gatv2_attention(rowptr, colind, xl, xr, att, negative_slope=None, dropout=None, out=None, stats=None)        -> (out f32[M, H, F], stats f32[M, H, 2])
    gatv2_attention_backward_row(rowptr, colind, xl, xr, att, stats, out, grad_out, negative_slope=None, dropout=None,
                                 want_att_part=True, results=None)                                               -> (delta, grad_xl[, att_part])
    gatv2_attention_backward_col(colptr, rowind, xl, xr, att, stats, delta, grad_out, negative_slope=None, dropout=None,
                                 result=None)                                                                    -> grad_xr f32[K, H, F]

``xl`` f32[M, H, F] is the aggregating node's term, ``xr`` f32[K, H, F] the neighbour's — the score's operand AND the aggregated value, so
one gathered row per entry serves the forward — ``att`` f32[H, F]:

    s_p = sum_f att[h, f] leaky_relu(xl[r, h, f] + xr[c, h, f])      a_p = exp(s_p - m) / l      out[r, h, :] = sum_p a_p xr[c, h, :]

``s_p`` has the bits of ``sddmm.gatv2_score`` on equally aligned operands (``_lib.describe_gatv2_attention``). ``negative_slope=None``: no
leaky ReLU. F <= 512. These three names are fp32 only; on fp16 / bf16 node terms (``att``, ``stats``, ``delta`` and ``att_part`` stay fp32):

    gatv2_attention_x16(rowptr, colind, xl, xr, att, negative_slope=None, dropout=None, out=None, stats=None)    -> (out x16[M, H, F], stats f32[M, H, 2])
    gatv2_attention_backward_row_x16(rowptr, colind, xl, xr, att, stats, out, grad_out, negative_slope=None, dropout=None,
                                     want_att_part=True, results=None)                                           -> (delta f32, grad_xl x16[, att_part f32])
    gatv2_attention_backward_col_x16(colptr, rowind, xl, xr, att, stats, delta, grad_out, negative_slope=None, dropout=None,
                                     result=None)                                                                -> grad_xr x16[K, H, F]

Every 16-bit element is widened exactly at its use, the arithmetic and the lane geometry are the fp32 kernels' and every 16-bit result is
rounded once at its store: where ``_lib.describe_gatv2_attention`` answers the same (V, W) with and without ``x16=True``, ``stats``,
``delta`` and ``att_part`` have the bits of the fp32 calls on the widened operands and ``out``, ``grad_xl``, ``grad_xr`` are theirs
narrowed once."""
import math

import torch

from ._lib import DOT_ATTENTION_MAX_F, ERR_UNSUPPORTED, GATV2_ATTENTION_MAX_F, GespmmError, check, lib
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


# ---- fused GATv2 attention

class Gatv2AttentionUnsupported(GespmmError):
    """F > 512: no kernel serves the shape and nothing was launched."""

    def __init__(self, F, where):
        RuntimeError.__init__(self, "%s: a head slice of F = %d floats has no kernel; the fused GATv2 attention (gatv2_attention) "
                                    "serves F <= %d (code %d)" % (where, F, GATV2_ATTENTION_MAX_F, ERR_UNSUPPORTED))
        self.code = ERR_UNSUPPORTED


def _slope(negative_slope):
    if negative_slope is None:
        return 1.0
    if isinstance(negative_slope, torch.Tensor) or not isinstance(negative_slope, (int, float)):
        raise TypeError("negative_slope must be a Python number or None")
    s = float(negative_slope)
    if s != s or s in (float("inf"), float("-inf")):
        raise ValueError("negative_slope must be finite, got %r" % (negative_slope,))
    return s


def _gatv2_shapes(ptr, ptr_name, ind, ind_name, xl, xr, att, segments_are_rows):
    """(M, K, H, F, nnz) of a call whose segments are the rows of xl (forward, row pass) or of xr (column pass)."""
    if xl.dim() != 3 or xr.dim() != 3 or xl.shape[1] < 1:
        raise ValueError("xl and xr must be [rows, H, F] with at least one head")
    M, H, F = xl.shape
    K = xr.shape[0]
    if tuple(xr.shape[1:]) != (H, F) or tuple(att.shape) != (H, F):
        raise ValueError("xl %s, xr %s and att %s must have the same heads and columns: att is [H, F]" %
                         (tuple(xl.shape), tuple(xr.shape), tuple(att.shape)))
    S = M if segments_are_rows else K
    if ptr.dim() != 1 or ptr.numel() != S + 1:
        raise ValueError("%s must be a vector of %d + 1 entries" % (ptr_name, S))
    if ind.dim() != 1:
        raise ValueError("%s must be a vector" % ind_name)
    return M, K, H, F, ind.numel()


def _gatv2_served(F, where):
    if F > GATV2_ATTENTION_MAX_F:
        raise Gatv2AttentionUnsupported(F, where)


def gatv2_attention(rowptr, colind, xl, xr, att, negative_slope=None, dropout=None, out=None, stats=None):
    """``out[r, h, :] = sum_p softmax_row(sum_f att[h, f] leaky_relu(xl[r, h, f] + xr[c_p, h, f]))_p xr[c_p, h, :]`` over the entries of CSR
    row r, H heads in ONE launch (gespmm_gatv2_attention_f32): no score, no alpha, nothing of size nnz, one gathered row per entry.
    Returns ``(out, stats)``; ``stats[r, h] = (m, l)`` is what the backward needs. Every word is written, an empty row +0.
    ``dropout=(p, seed)``: dropout on the coefficients after the normalisation (gespmm_gatv2_attention_dropout_f32). ``out`` / ``stats``:
    tensors to write into. ``colind`` within [0, K) and ``rowptr[M] == nnz`` are preconditions."""
    _typed((("rowptr", rowptr), ("colind", colind)), (("xl", xl), ("xr", xr), ("att", att), ("out", out), ("stats", stats)))
    _required((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _gatv2_shapes(rowptr, "rowptr", colind, "colind", xl, xr, att, True)
    slope = _slope(negative_slope)
    _shaped(out, "out", (M, H, F))
    _shaped(stats, "stats", (M, H, 2))
    dev = xl.device
    _placed((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att), ("out", out), ("stats", stats)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _gatv2_served(F, "gespmm_gatv2_attention_f32")
    if out is None:
        out = torch.empty((M, H, F), dtype=torch.float32, device=dev)
    if stats is None:
        stats = torch.empty((M, H, 2), dtype=torch.float32, device=dev)
    if M == 0:  # (results of no words have no address to hand over)
        return out, stats
    args = (_ptr(rowptr), _ptr(colind), _ptr(xl), _ptr(xr), _ptr(att), _ptr(out), _ptr(stats), M, K, H, F, nnz, slope)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_gatv2_attention_dropout_f32(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_gatv2_attention_f32(*args, _stream(dev))
    check(rc, "gespmm_gatv2_attention_dropout_f32" if dropout is not None else "gespmm_gatv2_attention_f32")
    return out, stats


def gatv2_attention_backward_row(rowptr, colind, xl, xr, att, stats, out, grad_out, negative_slope=None, dropout=None, want_att_part=True,
                                 results=None):
    """The row pass of ``gatv2_attention``'s backward (gespmm_gatv2_attention_backward_row_f32): ``delta[r, h] = <grad_out[r, h], out[r, h]>``,
    ``grad_xl[r, h, f] = sum_p ds_p (t_pf >= 0 ? att[h, f] : att[h, f] negative_slope)`` and, with ``want_att_part``, ``att_part[r, h, f] =
    sum_p ds_p leaky_relu(t_pf)`` — ``att_part.sum(0)`` is the gradient of ``att`` — where ``ds_p = a_p (<grad_out[r, h], xr[c_p, h]> -
    delta[r, h])``. ``stats`` and ``out`` are the forward's results; ``dropout`` the forward's pair. Returns ``(delta, grad_xl, att_part)``,
    or ``(delta, grad_xl)`` with ``want_att_part=False`` (nothing of att_part's size is then written); every word is written.
    ``results``: a tuple of tensors of that form to write into."""
    want = bool(want_att_part)
    n_res = 3 if want else 2
    if results is None:
        res = (None,) * n_res
    elif not isinstance(results, (tuple, list)) or len(results) != n_res or any(t is None for t in results):
        raise TypeError("results must be a tuple of %d tensors" % n_res)
    else:
        res = tuple(results)
    delta, grad_xl = res[0], res[1]
    att_part = res[2] if want else None
    _typed((("rowptr", rowptr), ("colind", colind)),
           (("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("out", out), ("grad_out", grad_out), ("results[0]", delta),
            ("results[1]", grad_xl), ("results[2]", att_part)))
    _required((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("out", out),
               ("grad_out", grad_out)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _gatv2_shapes(rowptr, "rowptr", colind, "colind", xl, xr, att, True)
    slope = _slope(negative_slope)
    _shaped(stats, "stats", (M, H, 2))
    _shaped(out, "out", (M, H, F))
    _shaped(grad_out, "grad_out", (M, H, F))
    _shaped(delta, "results[0]", (M, H))
    _shaped(grad_xl, "results[1]", (M, H, F))
    _shaped(att_part, "results[2]", (M, H, F))
    dev = xl.device
    _placed((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("out", out),
             ("grad_out", grad_out), ("results[0]", delta), ("results[1]", grad_xl), ("results[2]", att_part)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _gatv2_served(F, "gespmm_gatv2_attention_backward_row_f32")
    if delta is None:
        delta = torch.empty((M, H), dtype=torch.float32, device=dev)
        grad_xl = torch.empty((M, H, F), dtype=torch.float32, device=dev)
        if want:
            att_part = torch.empty((M, H, F), dtype=torch.float32, device=dev)
    ret = (delta, grad_xl, att_part) if want else (delta, grad_xl)
    if M == 0:
        return ret
    args = (_ptr(rowptr), _ptr(colind), _ptr(xl), _ptr(xr), _ptr(att), _ptr(stats), _ptr(out), _ptr(grad_out), _ptr(delta), _ptr(grad_xl),
            _ptr(att_part) if want else None, M, K, H, F, nnz, slope)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_gatv2_attention_backward_row_dropout_f32(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_gatv2_attention_backward_row_f32(*args, _stream(dev))
    check(rc, "gespmm_gatv2_attention_backward_row_dropout_f32" if dropout is not None else "gespmm_gatv2_attention_backward_row_f32")
    return ret


def gatv2_attention_backward_col(colptr, rowind, xl, xr, att, stats, delta, grad_out, negative_slope=None, dropout=None, result=None):
    """The column pass of ``gatv2_attention``'s backward (gespmm_gatv2_attention_backward_col_f32) on the CSC arrays of the pattern
    (``graphs.transpose_csr``; no ``csc_order``): ``grad_xr[c, h, f] = sum over column c of ds_p (t_pf >= 0 ? att[h, f] : att[h, f]
    negative_slope) + sum over column c of a_p grad_out[r_p, h, f]`` — the score's term and the aggregation's, two chains added once —
    with ``ds_p`` and ``a_p`` the bits of the row pass. ``delta`` is the row pass's. Returns ``grad_xr``; every word is written, an
    empty column +0. ``result``: a tensor to write into."""
    _typed((("colptr", colptr), ("rowind", rowind)),
           (("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("delta", delta), ("grad_out", grad_out), ("result", result)))
    _required((("colptr", colptr), ("rowind", rowind), ("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("delta", delta),
               ("grad_out", grad_out)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _gatv2_shapes(colptr, "colptr", rowind, "rowind", xl, xr, att, False)
    slope = _slope(negative_slope)
    _shaped(stats, "stats", (M, H, 2))
    _shaped(delta, "delta", (M, H))
    _shaped(grad_out, "grad_out", (M, H, F))
    _shaped(result, "result", (K, H, F))
    dev = xl.device
    _placed((("colptr", colptr), ("rowind", rowind), ("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("delta", delta),
             ("grad_out", grad_out), ("result", result)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _gatv2_served(F, "gespmm_gatv2_attention_backward_col_f32")
    grad_xr = result if result is not None else torch.empty((K, H, F), dtype=torch.float32, device=dev)
    if K == 0:
        return grad_xr
    args = (_ptr(colptr), _ptr(rowind), _ptr(xl), _ptr(xr), _ptr(att), _ptr(stats), _ptr(delta), _ptr(grad_out), _ptr(grad_xr), M, K, H, F,
            nnz, slope)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_gatv2_attention_backward_col_dropout_f32(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_gatv2_attention_backward_col_f32(*args, _stream(dev))
    check(rc, "gespmm_gatv2_attention_backward_col_dropout_f32" if dropout is not None else "gespmm_gatv2_attention_backward_col_f32")
    return grad_xr


# ---- ... on fp16 / bf16 node terms (gespmm_gatv2_attention_x16 and its backward)

def _typed_x16(int_ops, node_ops, float_ops):
    """``_typed`` with a third class: the node operands and 16-bit results, all ``torch.float16`` or all ``torch.bfloat16`` -> the
    GESPMM_X16_* code. The first of them names the type (``None`` passes, but not there)."""
    from .spmm import _X16

    _typed(int_ops, float_ops)
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
        if t.dtype != first.dtype:  # (mixed 16-bit dtypes and fp32 node terms: TypeError)
            raise TypeError("%s must have dtype %s, as %s, got %s" % (name, first.dtype, first_name, t.dtype))
    return _X16[first.dtype]


def gatv2_attention_x16(rowptr, colind, xl, xr, att, negative_slope=None, dropout=None, out=None, stats=None):
    """``gatv2_attention`` on 16-bit node terms (gespmm_gatv2_attention_x16 / _dropout_x16): ``xl`` [M, H, F] and ``xr`` [K, H, F] both
    ``torch.float16`` or both ``torch.bfloat16``, ``att`` f32[H, F]. Returns ``(out, stats)``: ``out`` [M, H, F] in the node terms' dtype,
    rounded once at the store; ``stats`` f32[M, H, 2]. Every element is widened exactly at its use and the arithmetic is
    ``gatv2_attention``'s: where ``_lib.describe_gatv2_attention`` answers the same (V, W) with and without ``x16=True``, ``stats`` has the
    bits of ``gatv2_attention`` on ``xl.float(), xr.float()`` and ``out`` is that call's ``out`` narrowed once. A 16-bit ``att`` or
    ``stats``, fp32 node terms and mixed 16-bit dtypes raise TypeError."""
    x16 = _typed_x16((("rowptr", rowptr), ("colind", colind)), (("xl", xl), ("xr", xr), ("out", out)), (("att", att), ("stats", stats)))
    _required((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _gatv2_shapes(rowptr, "rowptr", colind, "colind", xl, xr, att, True)
    slope = _slope(negative_slope)
    _shaped(out, "out", (M, H, F))
    _shaped(stats, "stats", (M, H, 2))
    dev = xl.device
    _placed((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att), ("out", out), ("stats", stats)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _gatv2_served(F, "gespmm_gatv2_attention_x16")
    if out is None:
        out = torch.empty((M, H, F), dtype=xl.dtype, device=dev)
    if stats is None:
        stats = torch.empty((M, H, 2), dtype=torch.float32, device=dev)
    if M == 0:  # (results of no words have no address to hand over)
        return out, stats
    args = (_ptr(rowptr), _ptr(colind), _ptr(xl), _ptr(xr), _ptr(att), _ptr(out), _ptr(stats), x16, M, K, H, F, nnz, slope)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_gatv2_attention_dropout_x16(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_gatv2_attention_x16(*args, _stream(dev))
    check(rc, "gespmm_gatv2_attention_dropout_x16" if dropout is not None else "gespmm_gatv2_attention_x16")
    return out, stats


def gatv2_attention_backward_row_x16(rowptr, colind, xl, xr, att, stats, out, grad_out, negative_slope=None, dropout=None,
                                     want_att_part=True, results=None):
    """``gatv2_attention_backward_row`` on 16-bit node terms (gespmm_gatv2_attention_backward_row_x16 / _dropout_x16): ``xl``, ``xr``,
    ``out``, ``grad_out`` and the result ``grad_xl`` in one 16-bit dtype; ``att``, ``stats`` and the results ``delta`` f32[M, H] and
    ``att_part`` f32[M, H, F] stay fp32. ``delta`` is taken of the STORED 16-bit ``out``; ``grad_xl`` is rounded once at the store.
    Returns ``(delta, grad_xl, att_part)``, or ``(delta, grad_xl)`` with ``want_att_part=False``. On equal (V, W) ``delta`` and
    ``att_part`` have the bits of ``gatv2_attention_backward_row`` on the widened operands, ``grad_xl`` is its ``grad_xl`` narrowed once."""
    want = bool(want_att_part)
    n_res = 3 if want else 2
    if results is None:
        res = (None,) * n_res
    elif not isinstance(results, (tuple, list)) or len(results) != n_res or any(t is None for t in results):
        raise TypeError("results must be a tuple of %d tensors" % n_res)
    else:
        res = tuple(results)
    delta, grad_xl = res[0], res[1]
    att_part = res[2] if want else None
    x16 = _typed_x16((("rowptr", rowptr), ("colind", colind)),
                     (("xl", xl), ("xr", xr), ("out", out), ("grad_out", grad_out), ("results[1]", grad_xl)),
                     (("att", att), ("stats", stats), ("results[0]", delta), ("results[2]", att_part)))
    _required((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("out", out),
               ("grad_out", grad_out)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _gatv2_shapes(rowptr, "rowptr", colind, "colind", xl, xr, att, True)
    slope = _slope(negative_slope)
    _shaped(stats, "stats", (M, H, 2))
    _shaped(out, "out", (M, H, F))
    _shaped(grad_out, "grad_out", (M, H, F))
    _shaped(delta, "results[0]", (M, H))
    _shaped(grad_xl, "results[1]", (M, H, F))
    _shaped(att_part, "results[2]", (M, H, F))
    dev = xl.device
    _placed((("rowptr", rowptr), ("colind", colind), ("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("out", out),
             ("grad_out", grad_out), ("results[0]", delta), ("results[1]", grad_xl), ("results[2]", att_part)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _gatv2_served(F, "gespmm_gatv2_attention_backward_row_x16")
    if delta is None:
        delta = torch.empty((M, H), dtype=torch.float32, device=dev)
        grad_xl = torch.empty((M, H, F), dtype=xl.dtype, device=dev)
        if want:
            att_part = torch.empty((M, H, F), dtype=torch.float32, device=dev)
    ret = (delta, grad_xl, att_part) if want else (delta, grad_xl)
    if M == 0:
        return ret
    args = (_ptr(rowptr), _ptr(colind), _ptr(xl), _ptr(xr), _ptr(att), _ptr(stats), _ptr(out), _ptr(grad_out), _ptr(delta), _ptr(grad_xl),
            _ptr(att_part) if want else None, x16, M, K, H, F, nnz, slope)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_gatv2_attention_backward_row_dropout_x16(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_gatv2_attention_backward_row_x16(*args, _stream(dev))
    check(rc, "gespmm_gatv2_attention_backward_row_dropout_x16" if dropout is not None else "gespmm_gatv2_attention_backward_row_x16")
    return ret


def gatv2_attention_backward_col_x16(colptr, rowind, xl, xr, att, stats, delta, grad_out, negative_slope=None, dropout=None, result=None):
    """``gatv2_attention_backward_col`` on 16-bit node terms (gespmm_gatv2_attention_backward_col_x16 / _dropout_x16): ``xl``, ``xr``,
    ``grad_out`` and the result ``grad_xr`` [K, H, F] in one 16-bit dtype; ``att``, ``stats`` and ``delta`` (the row pass's) stay fp32.
    The two fp32 chains of a word are added once and that sum is rounded once, at the store: on equal (V, W) ``grad_xr`` is
    ``gatv2_attention_backward_col`` on the widened operands, narrowed once. ``result``: a tensor to write into."""
    x16 = _typed_x16((("colptr", colptr), ("rowind", rowind)), (("xl", xl), ("xr", xr), ("grad_out", grad_out), ("result", result)),
                     (("att", att), ("stats", stats), ("delta", delta)))
    _required((("colptr", colptr), ("rowind", rowind), ("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("delta", delta),
               ("grad_out", grad_out)))
    _dropout_typed(dropout)
    M, K, H, F, nnz = _gatv2_shapes(colptr, "colptr", rowind, "rowind", xl, xr, att, False)
    slope = _slope(negative_slope)
    _shaped(stats, "stats", (M, H, 2))
    _shaped(delta, "delta", (M, H))
    _shaped(grad_out, "grad_out", (M, H, F))
    _shaped(result, "result", (K, H, F))
    dev = xl.device
    _placed((("colptr", colptr), ("rowind", rowind), ("xl", xl), ("xr", xr), ("att", att), ("stats", stats), ("delta", delta),
             ("grad_out", grad_out), ("result", result)), dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
    _gatv2_served(F, "gespmm_gatv2_attention_backward_col_x16")
    grad_xr = result if result is not None else torch.empty((K, H, F), dtype=xl.dtype, device=dev)
    if K == 0:
        return grad_xr
    args = (_ptr(colptr), _ptr(rowind), _ptr(xl), _ptr(xr), _ptr(att), _ptr(stats), _ptr(delta), _ptr(grad_out), _ptr(grad_xr), x16, M, K, H,
            F, nnz, slope)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_gatv2_attention_backward_col_dropout_x16(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_gatv2_attention_backward_col_x16(*args, _stream(dev))
    check(rc, "gespmm_gatv2_attention_backward_col_dropout_x16" if dropout is not None else "gespmm_gatv2_attention_backward_col_x16")
    return grad_xr


# ---- the fused dot-product attention on fp16 / bf16 q, k and v (gespmm_dot_attention_x16 and its backward)

def dot_attention_x16(rowptr, colind, q, k, v, scale=None, dropout=None, out=None, stats=None):
    """``dot_attention`` on 16-bit node terms (gespmm_dot_attention_x16 / _dropout_x16): ``q`` [M, H, F], ``k`` and ``v`` [K, H, F] all
    ``torch.float16`` or all ``torch.bfloat16``. Returns ``(out, stats)``: ``out`` [M, H, F] in the terms' dtype, fp32 sums rounded once
    at the store; ``stats`` f32[M, H, 2]. Every element is widened exactly at its use and the arithmetic is ``dot_attention``'s: where
    ``_lib.describe_dot_attention`` answers the same (V, W) with and without ``x16=True``, ``stats`` has the bits of ``dot_attention`` on
    ``q.float(), k.float(), v.float()`` and ``out`` is that call's ``out`` narrowed once. A 16-bit ``stats``, fp32 node terms and mixed
    16-bit dtypes raise TypeError."""
    x16 = _typed_x16((("rowptr", rowptr), ("colind", colind)), (("q", q), ("k", k), ("v", v), ("out", out)), (("stats", stats),))
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
    _served(F, "gespmm_dot_attention_x16")
    if out is None:
        out = torch.empty((M, H, F), dtype=q.dtype, device=dev)
    if stats is None:
        stats = torch.empty((M, H, 2), dtype=torch.float32, device=dev)
    if M == 0:  # (results of no words have no address to hand over)
        return out, stats
    args = (_ptr(rowptr), _ptr(colind), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(stats), x16, M, K, H, F, nnz, sc)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_dot_attention_dropout_x16(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_dot_attention_x16(*args, _stream(dev))
    check(rc, "gespmm_dot_attention_dropout_x16" if dropout is not None else "gespmm_dot_attention_x16")
    return out, stats


def dot_attention_backward_q_x16(rowptr, colind, q, k, v, stats, out, grad_out, scale=None, dropout=None, results=None):
    """``dot_attention_backward_q`` on 16-bit node terms (gespmm_dot_attention_backward_q_x16 / _dropout_x16): ``q``, ``k``, ``v``,
    ``out``, ``grad_out`` and the result ``grad_q`` in one 16-bit dtype; ``stats`` and the result ``delta`` f32[M, H] stay fp32.
    ``delta`` is taken of the STORED 16-bit ``out``; ``grad_q`` is ``fl32(scale * chain)`` rounded once at the store. Returns
    ``(delta, grad_q)``. On equal (V, W) ``delta`` has the bits of ``dot_attention_backward_q`` on the widened operands and ``grad_q`` is
    its ``grad_q`` narrowed once. ``results``: a pair ``(delta, grad_q)`` to write into."""
    delta, grad_q = _pair(results)
    x16 = _typed_x16((("rowptr", rowptr), ("colind", colind)),
                     (("q", q), ("k", k), ("v", v), ("out", out), ("grad_out", grad_out), ("results[1]", grad_q)),
                     (("stats", stats), ("results[0]", delta)))
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
    _served(F, "gespmm_dot_attention_backward_q_x16")
    if delta is None:
        delta = torch.empty((M, H), dtype=torch.float32, device=dev)
        grad_q = torch.empty((M, H, F), dtype=q.dtype, device=dev)
    if M == 0:
        return delta, grad_q
    args = (_ptr(rowptr), _ptr(colind), _ptr(q), _ptr(k), _ptr(v), _ptr(stats), _ptr(out), _ptr(grad_out), _ptr(delta), _ptr(grad_q), x16, M,
            K, H, F, nnz, sc)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_dot_attention_backward_q_dropout_x16(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_dot_attention_backward_q_x16(*args, _stream(dev))
    check(rc, "gespmm_dot_attention_backward_q_dropout_x16" if dropout is not None else "gespmm_dot_attention_backward_q_x16")
    return delta, grad_q


def dot_attention_backward_kv_x16(colptr, rowind, q, k, v, stats, delta, grad_out, scale=None, dropout=None, results=None):
    """``dot_attention_backward_kv`` on 16-bit node terms (gespmm_dot_attention_backward_kv_x16 / _dropout_x16): ``q``, ``k``, ``v``,
    ``grad_out`` and the results ``grad_k``, ``grad_v`` [K, H, F] in one 16-bit dtype; ``stats`` and ``delta`` (the row pass's) stay
    fp32. ``grad_k`` is ``fl32(scale * chain)`` and ``grad_v`` its chain, each rounded once at the store: on equal (V, W) they are
    ``dot_attention_backward_kv``'s on the widened operands, narrowed once. ``results``: a pair ``(grad_k, grad_v)`` to write into."""
    grad_k, grad_v = _pair(results)
    x16 = _typed_x16((("colptr", colptr), ("rowind", rowind)),
                     (("q", q), ("k", k), ("v", v), ("grad_out", grad_out), ("results[0]", grad_k), ("results[1]", grad_v)),
                     (("stats", stats), ("delta", delta)))
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
    _served(F, "gespmm_dot_attention_backward_kv_x16")
    if grad_k is None:
        grad_k = torch.empty((K, H, F), dtype=q.dtype, device=dev)
        grad_v = torch.empty((K, H, F), dtype=q.dtype, device=dev)
    if K == 0:
        return grad_k, grad_v
    args = (_ptr(colptr), _ptr(rowind), _ptr(q), _ptr(k), _ptr(v), _ptr(stats), _ptr(delta), _ptr(grad_out), _ptr(grad_k), _ptr(grad_v), x16,
            M, K, H, F, nnz, sc)
    with _on_device(dev):
        if dropout is not None:
            rc = lib.gespmm_dot_attention_backward_kv_dropout_x16(*args, p, _ptr(seed), _stream(dev))
        else:
            rc = lib.gespmm_dot_attention_backward_kv_x16(*args, _stream(dev))
    check(rc, "gespmm_dot_attention_backward_kv_dropout_x16" if dropout is not None else "gespmm_dot_attention_backward_kv_x16")
    return grad_k, grad_v
