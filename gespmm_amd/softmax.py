"""Edge softmax: softmax over the entries of each CSR row, per head (extension; gespmm_edge_softmax_f32 /
gespmm_edge_softmax_backward_f32 — the reference has no counterpart).

    edge_softmax(rowptr, score, out=None, negative_slope=None)                                    -> f32, the shape of score
    edge_softmax_backward(rowptr, alpha, grad_alpha, score=None, negative_slope=None, out=None)   -> f32, the shape of alpha

``score`` is f32[nnz] or f32[nnz, H] in CSR edge order — what ``sddmm.csr_sddmm`` / ``sddmm.csr_sddmm_heads`` return and what
``spmm.csr_spmm`` / ``spmm.csr_spmm_heads`` take as edge weights. For row r with entries [lo, hi) and head h

    x = leaky_relu(score[lo:hi, h], negative_slope)          (negative_slope=None: no leaky ReLU)
    out[lo:hi, h] = exp(x - max(x)) / sum(exp(x - max(x)))

in ONE kernel on the row pointers as they are: no expanded row ids, no ``segment_reduce`` / ``repeat_interleave`` passes over an
[nnz, H] array. Empty rows write nothing. Head h has the bits of the single-head call on ``score[:, h].contiguous()``; the bits do not
depend on H, on stream capture or on the run (``_lib.describe_edge_softmax``). ``rowptr[M] == score.shape[0]`` is a precondition, as
everywhere in this package; ``out`` must not overlap an input. fp32 only: 16-bit and fp64 tensors raise TypeError. Both calls go
through ctypes."""
import torch

from ._lib import check, lib
from .spmm import _on_device, _ptr, _stream


def _slope(negative_slope):
    if negative_slope is None:
        return 1.0
    s = float(negative_slope)
    if s != s or s in (float("inf"), float("-inf")):
        raise ValueError("negative_slope must be finite, got %r" % (negative_slope,))
    return s


def _edge_array(t, name, like=None):
    """fp32, contiguous, [nnz] or [nnz, H] on a HIP device; the shape and device of ``like`` when that is given."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != torch.float32:  # (16-bit and fp64 edge arrays have no entry point: TypeError)
        raise TypeError("%s must have dtype torch.float32, got %s" % (name, t.dtype))
    if t.dim() not in (1, 2):
        raise ValueError("%s must be [nnz] or [nnz, H]" % name)
    if t.dim() == 2 and t.shape[1] < 1:
        raise ValueError("%s must have at least one head" % name)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if t.device.type != "cuda":
        raise ValueError("%s must be a HIP (cuda) device tensor; gespmm_amd has no CPU path" % name)
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError("%s must be f32%s on %s, as the other edge arrays" % (name, list(like.shape), like.device))


def _checked(rowptr, first, name):
    """-> (device, M, H, nnz)"""
    if not isinstance(rowptr, torch.Tensor):
        raise TypeError("rowptr must be a torch.Tensor")
    if rowptr.dtype != torch.int32:
        raise TypeError("rowptr must have dtype torch.int32, got %s" % rowptr.dtype)
    if rowptr.dim() != 1 or rowptr.numel() < 1 or not rowptr.is_contiguous():
        raise ValueError("rowptr must be a contiguous vector of M + 1 entries")
    _edge_array(first, name)
    if rowptr.device != first.device:
        raise ValueError("rowptr and %s must live on the same device" % name)
    return first.device, rowptr.numel() - 1, (first.shape[1] if first.dim() == 2 else 1), first.shape[0]


def edge_softmax(rowptr, score, out=None, negative_slope=None):
    """Softmax of ``score`` (f32[nnz] or f32[nnz, H]) over the entries of each row of the CSR pattern ``rowptr`` describes, per head, with
    an optional leaky ReLU in front (gespmm_edge_softmax_f32). ``out``: a tensor like ``score`` to write into (entries of no row — there
    are none when ``rowptr[M] == nnz`` — and nothing else are left untouched)."""
    slope = _slope(negative_slope)
    dev, M, H, nnz = _checked(rowptr, score, "score")
    if out is None:
        out = torch.empty_like(score)
    else:
        _edge_array(out, "out", like=score)
    with _on_device(dev):
        rc = lib.gespmm_edge_softmax_f32(_ptr(rowptr), _ptr(score), _ptr(out), M, H, nnz, slope, _stream(dev))
    check(rc, "gespmm_edge_softmax_f32")
    return out


def edge_softmax_backward(rowptr, alpha, grad_alpha, score=None, negative_slope=None, out=None):
    """Gradient of ``edge_softmax`` with respect to ``score``: ``alpha * (grad_alpha - sum_row(alpha * grad_alpha))``, times the leaky
    ReLU's factor (gespmm_edge_softmax_backward_f32). ``alpha`` is the forward's result; ``score`` — the forward's input, read for its
    sign — is needed exactly when ``negative_slope`` is given."""
    slope = _slope(negative_slope)
    dev, M, H, nnz = _checked(rowptr, alpha, "alpha")
    _edge_array(grad_alpha, "grad_alpha", like=alpha)
    if slope != 1.0:
        if score is None:
            raise ValueError("negative_slope needs score (the forward's input)")
        _edge_array(score, "score", like=alpha)
    else:
        score = None
    if out is None:
        out = torch.empty_like(alpha)
    else:
        _edge_array(out, "out", like=alpha)
    with _on_device(dev):
        rc = lib.gespmm_edge_softmax_backward_f32(_ptr(rowptr), _ptr(alpha), _ptr(grad_alpha), _ptr(score) if score is not None else None,
                                                  _ptr(out), M, H, nnz, slope, _stream(dev))
    check(rc, "gespmm_edge_softmax_backward_f32")
    return out
