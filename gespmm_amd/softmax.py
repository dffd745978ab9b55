"""Edge softmax: softmax over the entries of each CSR row, per head (extension; gespmm_edge_softmax_f32 /
gespmm_edge_softmax_backward_f32 — the reference has no counterpart).

    edge_softmax(rowptr, score, out=None, negative_slope=None)                                    -> f32, the shape of score
    edge_softmax_backward(rowptr, alpha, grad_alpha, score=None, negative_slope=None, out=None)   -> f32, the shape of alpha
    gat_edge_softmax(rowptr, colind, el, er, negative_slope=None, out=None)                       -> f32[nnz, H]
    gat_edge_softmax_backward(rowptr, colind, alpha, grad_alpha, el=None, er=None, negative_slope=None) -> (grad_score, grad_el)
    edge_segment_sum(ptr, x, order=None, out=None)                                                -> f32[S, H] (or f32[S])
    gat_softmax_stats(rowptr, colind, el, er, negative_slope=None, out=None)                      -> f32[M, H, 2]
    gat_backward_el(rowptr, colind, el, er, stats, grad_out, feat, negative_slope=None, out=None, dropout=None) -> (delta f32[M, H], grad_el f32[M, H])
    gat_backward_er(colptr, rowind, el, er, stats, delta, grad_out, feat, negative_slope=None, out=None, dropout=None) -> grad_er f32[K, H]
    edge_dropout(rowptr, colind, x, p, seed, out=None)                                            -> f32[nnz, H] (or f32[nnz])

``score`` is f32[nnz] or f32[nnz, H] in CSR edge order — what ``sddmm.csr_sddmm`` / ``sddmm.csr_sddmm_heads`` return and what
``spmm.csr_spmm`` / ``spmm.csr_spmm_heads`` take as edge weights. For row r with entries [lo, hi) and head h

    x = leaky_relu(score[lo:hi, h], negative_slope)          (negative_slope=None: no leaky ReLU)
    out[lo:hi, h] = exp(x - max(x)) / sum(exp(x - max(x)))

in ONE kernel on the row pointers as they are: no expanded row ids, no ``segment_reduce`` / ``repeat_interleave`` passes over an
[nnz, H] array. Empty rows write nothing. Head h has the bits of the single-head call on ``score[:, h].contiguous()``; the bits do not
depend on H, on stream capture or on the run (``_lib.describe_edge_softmax``). ``rowptr[M] == score.shape[0]`` is a precondition, as
everywhere in this package; ``out`` must not overlap an input. fp32 only: 16-bit and fp64 tensors raise TypeError.

``gat_edge_softmax`` is the same softmax on the additive score of a graph attention layer, ``score[e, h] = el[row(e), h] +
er[colind[e], h]``, computed inside the kernel: no ``[nnz, H]`` score exists, and the result has the bits of ``edge_softmax`` on the
score ``sddmm.csr_sddmm_heads`` writes for ``q = (el, 1), k = (1, er)``. Its backward returns ``grad_score`` and, from the same launch,
``grad_el = sum_row(grad_score)``; ``edge_segment_sum`` on the CSC arrays (``ptr=colptr, order=csc_order``) gives ``grad_er`` without a
permuted copy. The sums have a pinned order (include/gespmm.h), the one ``edge_segment_sum(rowptr, grad_score)`` reproduces.
``gat_softmax_stats`` returns what that softmax divides by — per (row, head) the maximum and the sum, with its bits — for
``spmm.gat_aggregate``, which computes the weights inside the aggregation and needs no ``[nnz, H]`` array at all.
``gat_backward_el`` / ``gat_backward_er`` are that aggregation's backward for ``el`` and ``er``: two launches that compute the weight,
the dot product ``<grad_out[row], feat[col]>`` and the softmax's backward per entry from node-sized words, over the rows and over the
columns, and sum them in the pinned order — no ``[nnz, H]`` array there either.
``edge_dropout`` is dropout on the attention coefficients with a mask that is never stored: whether entry (row, column) keeps head h is
a pure function of ``(seed, row, column, h)`` (``restate_edge_dropout_bits``; include/gespmm.h), so the fused aggregation and both
passes of the fused backward recompute it (``dropout=(p, seed)``) and nothing edge-sized is saved for it. ``seed`` is an int32[2]
DEVICE tensor: no host synchronisation, and a seed drawn or overwritten on the device between two replays of a captured graph
changes the mask. Two entries with the same (row, column) — a multigraph — share their decision.
All calls go through ctypes."""
import torch

from ._lib import check, lib
from .spmm import _on_device, _ptr, _stream


def _dropout_typed(dropout):
    """TypeError for what is no pair (p, seed) with an int32 seed tensor (``None`` passes: no dropout)."""
    if dropout is None:
        return
    if not isinstance(dropout, (tuple, list)) or len(dropout) != 2:
        raise TypeError("dropout must be a pair (p, seed)")
    p, seed = dropout
    if not isinstance(seed, torch.Tensor):
        raise TypeError("seed must be a torch.Tensor")
    if seed.dtype != torch.int32:
        raise TypeError("seed must have dtype torch.int32, got %s" % seed.dtype)
    if isinstance(p, torch.Tensor) or not isinstance(p, (int, float)):
        raise TypeError("the dropout probability must be a Python number (the seed, not p, is what lives on the device)")


def _dropout(dropout, dev):
    """``(p, seed)`` -> (float p in [0, 1), the int32[2] seed tensor on ``dev``)."""
    _dropout_typed(dropout)
    p, seed = dropout
    p = float(p)
    if not (0.0 <= p < 1.0):  # (NaN included)
        raise ValueError("the dropout probability must be in [0, 1), got %r" % (p,))
    if tuple(seed.shape) != (2,) or not seed.is_contiguous():
        raise ValueError("seed must be a contiguous int32[2] tensor")
    if seed.device != dev:
        raise ValueError("seed must live on %s, as the other operands" % (dev,))
    return p, seed


def restate_edge_dropout_bits(s0, s1, r, c, h):
    """The mask's bits in numpy (uint32 arrays or scalars, broadcast) — the restatement the tests hold the kernels and
    ``gespmm_edge_dropout_bits`` to. An entry keeps its value when ``bits >= _lib.edge_dropout_threshold(p)``."""
    import numpy as np

    def mix(x):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        return x ^ (x >> np.uint32(16))

    with np.errstate(over="ignore"):
        s0, s1, r, c, h = (np.asarray(v).astype(np.uint32) for v in (s0, s1, r, c, h))
        return mix(mix(mix(r ^ s0) ^ c) ^ (h * np.uint32(0x9E3779B9)) ^ s1)


def edge_dropout(rowptr, colind, x, p, seed, out=None):
    """``out[e, h] = keep(row(e), colind[e], h) ? x[e, h] / (1 - p) : +0`` on an edge array of the CSR pattern (gespmm_edge_dropout_f32):
    one launch, no workspace, capturable. ``x`` f32[nnz] or f32[nnz, H]; ``seed`` int32[2] on the device; ``out`` may be ``x``. The
    drop is a select — a dropped NaN or inf becomes +0 — and ``p == 0`` returns the bits of ``x``. The op is its own adjoint: the
    backward is the same call on the gradient."""
    _typed(torch.int32, rowptr=rowptr, colind=colind)
    _typed(torch.float32, x=x)
    _dropout_typed((p, seed))
    dev, M, H, nnz = _checked(rowptr, x, "x")
    _index_vector(colind, "colind", dev, nnz)
    p, seed = _dropout((p, seed), dev)
    if out is None:
        out = torch.empty_like(x)
    else:
        _edge_array(out, "out", like=x)
    with _on_device(dev):
        # (K: the entry point checks it for sense only; no kernel addresses by it)
        rc = lib.gespmm_edge_dropout_f32(_ptr(rowptr), _ptr(colind), _ptr(x), _ptr(out), M, 1, H, nnz, p, _ptr(seed), _stream(dev))
    check(rc, "gespmm_edge_dropout_f32")
    return out


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


def _index_vector(t, name, dev, n=None):
    """int32, contiguous, one-dimensional, on ``dev`` (``n`` entries when given)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != torch.int32:
        raise TypeError("%s must have dtype torch.int32, got %s" % (name, t.dtype))
    if t.dim() != 1 or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError("%s must be a contiguous vector%s" % (name, "" if n is None else " of %d entries" % n))
    if t.device != dev:
        raise ValueError("%s must live on %s, as the other operands" % (name, dev))


def _node_array(t, name, like=None, rows=None):
    """fp32, contiguous, [rows, H] on a HIP device; the head count and device of ``like`` when that is given."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s must have dtype torch.float32, got %s" % (name, t.dtype))
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError("%s must be [rows, H] with at least one head" % name)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if t.device.type != "cuda":
        raise ValueError("%s must be a HIP (cuda) device tensor; gespmm_amd has no CPU path" % name)
    if rows is not None and t.shape[0] != rows:
        raise ValueError("%s must have %d rows, got %d" % (name, rows, t.shape[0]))
    if like is not None and (t.shape[1] != like.shape[1] or t.device != like.device):
        raise ValueError("%s must have %d heads on %s, as the other operands" % (name, like.shape[1], like.device))


def _checked_rowptr(rowptr, dev=None):
    if not isinstance(rowptr, torch.Tensor):
        raise TypeError("rowptr must be a torch.Tensor")
    if rowptr.dtype != torch.int32:
        raise TypeError("rowptr must have dtype torch.int32, got %s" % rowptr.dtype)
    if rowptr.dim() != 1 or rowptr.numel() < 1 or not rowptr.is_contiguous():
        raise ValueError("rowptr must be a contiguous vector of M + 1 entries")
    if dev is not None and rowptr.device != dev:
        raise ValueError("rowptr must live on %s, as the other operands" % (dev,))
    return rowptr.numel() - 1


def gat_edge_softmax(rowptr, colind, el, er, negative_slope=None, out=None):
    """``edge_softmax(rowptr, el[row] + er[colind], negative_slope)`` with the score never written (gespmm_gat_softmax_f32): ``el``
    f32[M, H] scores the row of an entry, ``er`` f32[K, H] its column; ``colind`` int32[nnz] within [0, K) (a precondition). One launch
    that writes ``out`` f32[nnz, H] only; the bits are those of ``edge_softmax`` on the score array of the width-2 ``csr_sddmm_heads``."""
    slope = _slope(negative_slope)
    M = _checked_rowptr(rowptr)
    _node_array(el, "el", rows=M)
    _node_array(er, "er", like=el)
    dev = el.device
    _checked_rowptr(rowptr, dev)
    _index_vector(colind, "colind", dev)
    nnz, H, K = colind.numel(), el.shape[1], er.shape[0]
    if out is None:
        out = torch.empty(nnz, H, dtype=torch.float32, device=dev)
    else:
        _edge_array(out, "out")
        if out.shape != (nnz, H) or out.device != dev:
            raise ValueError("out must be f32[%d, %d] on %s" % (nnz, H, dev))
    with _on_device(dev):
        rc = lib.gespmm_gat_softmax_f32(_ptr(rowptr), _ptr(colind), _ptr(el), _ptr(er), _ptr(out), M, K, H, nnz, slope, _stream(dev))
    check(rc, "gespmm_gat_softmax_f32")
    return out


def _gat_terms(rowptr, colind, el, er):
    """The shared checks of the calls on (rowptr, colind, el, er) -> (device, M, K, H, nnz)."""
    M = _checked_rowptr(rowptr)
    _node_array(el, "el", rows=M)
    _node_array(er, "er", like=el)
    dev = el.device
    _checked_rowptr(rowptr, dev)
    _index_vector(colind, "colind", dev)
    return dev, M, er.shape[0], el.shape[1], colind.numel()


def _stats_array(t, name, M, H, dev):
    """fp32, contiguous, [M, H, 2] on ``dev``, 8-byte aligned (the kernels move a pair as one 8-byte word)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s must have dtype torch.float32, got %s" % (name, t.dtype))
    if tuple(t.shape) != (M, H, 2) or t.device != dev:
        raise ValueError("%s must be f32[%d, %d, 2] on %s" % (name, M, H, dev))
    if not t.is_contiguous() or t.data_ptr() % 8 != 0:
        raise ValueError("%s must be contiguous and 8-byte aligned" % name)


def gat_softmax_stats(rowptr, colind, el, er, negative_slope=None, out=None):
    """The row statistics of ``gat_edge_softmax`` -> f32[M, H, 2] (gespmm_gat_softmax_stats_f32): ``[r, h, 0]`` the maximum m of
    ``leaky_relu(el[r, h] + er[colind, h])`` over the row's entries, ``[r, h, 1]`` the sum s of ``exp(x - m)``, with exactly the bits
    ``gat_edge_softmax`` divides by (the same kernel without its last pass), so ``alpha[e, h] == exp(x - m) / s`` bit for bit. Every
    word is written; an empty row gives (+0, +0). Node-sized: what ``spmm.gat_aggregate`` needs in place of ``alpha``."""
    slope = _slope(negative_slope)
    dev, M, K, H, nnz = _gat_terms(rowptr, colind, el, er)
    if out is None:
        out = torch.empty(M, H, 2, dtype=torch.float32, device=dev)
    else:
        _stats_array(out, "out", M, H, dev)
    with _on_device(dev):
        rc = lib.gespmm_gat_softmax_stats_f32(_ptr(rowptr), _ptr(colind), _ptr(el), _ptr(er), _ptr(out), M, K, H, nnz, slope, _stream(dev))
    check(rc, "gespmm_gat_softmax_stats_f32")
    return out


def gat_edge_softmax_backward(rowptr, colind, alpha, grad_alpha, el=None, er=None, negative_slope=None):
    """Backward of ``gat_edge_softmax`` in one launch (gespmm_gat_softmax_backward_f32) -> ``(grad_score, grad_el)``: ``grad_score``
    f32[nnz, H] is ``edge_softmax_backward`` with the sign of ``el[row] + er[colind]`` in place of a score array, ``grad_el`` f32[M, H]
    its row sums (empty rows +0). ``el`` and ``er`` are needed exactly when ``negative_slope`` is given. ``grad_er`` is
    ``edge_segment_sum(colptr, grad_score, order=csc_order)``."""
    slope = _slope(negative_slope)
    M = _checked_rowptr(rowptr)
    _edge_array(alpha, "alpha")
    if alpha.dim() != 2:
        raise ValueError("alpha must be [nnz, H]")
    _edge_array(grad_alpha, "grad_alpha", like=alpha)
    dev = alpha.device
    _checked_rowptr(rowptr, dev)
    nnz, H = alpha.shape
    _index_vector(colind, "colind", dev, nnz)
    K = 1
    if slope != 1.0:
        if el is None or er is None:
            raise ValueError("negative_slope needs el and er (the forward's inputs)")
        _node_array(el, "el", like=alpha, rows=M)
        _node_array(er, "er", like=alpha)
        K = er.shape[0]
    else:
        el = er = None
    grad_score = torch.empty_like(alpha)
    grad_el = torch.empty(M, H, dtype=torch.float32, device=dev)
    with _on_device(dev):
        rc = lib.gespmm_gat_softmax_backward_f32(_ptr(rowptr), _ptr(colind), _ptr(alpha), _ptr(grad_alpha),
                                                 _ptr(el) if el is not None else None, _ptr(er) if er is not None else None,
                                                 _ptr(grad_score), _ptr(grad_el), M, K, H, nnz, slope, _stream(dev))
    check(rc, "gespmm_gat_softmax_backward_f32")
    return grad_score, grad_el


def edge_segment_sum(ptr, x, order=None, out=None):
    """``out[s, h] = sum of x[order[p], h] over p in [ptr[s], ptr[s + 1])`` (``order=None``: ``x[p, h]``) in one launch, in the pinned
    order of the edge softmax (gespmm_edge_segment_sum_f32). ``x`` f32[nnz] or f32[nnz, H]; ``order`` int32[nnz] within [0, nnz) — an
    int64 order raises TypeError, convert it once; ``out`` f32[S, H] (f32[S] for a one-dimensional ``x``), every word written, empty
    segments +0. With ``ptr=colptr, order=csc_order`` it sums an edge array over the columns of the pattern."""
    dev, S, H, nnz = _checked(ptr, x, "x")
    if order is not None:
        _index_vector(order, "order", dev, nnz)
    shape = (S, H) if x.dim() == 2 else (S,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch.Tensor")
        if out.dtype != torch.float32:
            raise TypeError("out must have dtype torch.float32, got %s" % out.dtype)
        if out.shape != shape or out.device != dev or not out.is_contiguous():
            raise ValueError("out must be contiguous f32%s on %s" % (list(shape), dev))
    with _on_device(dev):
        rc = lib.gespmm_edge_segment_sum_f32(_ptr(ptr), _ptr(order) if order is not None else None, _ptr(x), _ptr(out), S, H, nnz,
                                             _stream(dev))
    check(rc, "gespmm_edge_segment_sum_f32")
    return out


def _head_rows(t, name, rows, H, dev, F=None):
    """fp32, contiguous, [rows, H, F] on ``dev`` (F >= 1; the given F when there is one) -> F"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s must have dtype torch.float32, got %s" % (name, t.dtype))
    if t.dim() != 3 or t.shape[0] != rows or t.shape[1] != H or t.shape[2] < 1 or (F is not None and t.shape[2] != F):
        raise ValueError("%s must be f32[%d, %d, %s], got %s" % (name, rows, H, "F" if F is None else F, list(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if t.device != dev:
        raise ValueError("%s must live on %s, as the other operands" % (name, dev))
    return t.shape[2]


def _node_result(t, name, rows, H, dev):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s must have dtype torch.float32, got %s" % (name, t.dtype))
    if tuple(t.shape) != (rows, H) or t.device != dev or not t.is_contiguous():
        raise ValueError("%s must be contiguous f32[%d, %d] on %s" % (name, rows, H, dev))


def _typed(dtype, **operands):
    """TypeError for what is no tensor of ``dtype`` — for every operand before any of them is looked at more closely."""
    for name, t in operands.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != dtype:
            raise TypeError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))


def gat_backward_el(rowptr, colind, el, er, stats, grad_out, feat, negative_slope=None, out=None, dropout=None):
    """Backward of ``spmm.gat_aggregate`` for ``el`` with no edge array (gespmm_gat_backward_el_f32) -> ``(delta, grad_el)``, both
    f32[M, H]: per entry the weight (``stats = gat_softmax_stats(..)``: the bits of alpha), ``g = <grad_out[row], feat[col]>`` (one
    fmaf chain over ascending f) and ``gs = w (g - delta) * leaky'``, with ``delta = sum_row(w g)`` and ``grad_el = sum_row(gs)`` in
    the pinned order of ``gat_edge_softmax_backward``. ``grad_out`` f32[M, H, F], ``feat`` f32[K, H, F]. ``delta`` is what
    ``gat_backward_er`` needs. ``out``: a pair of tensors ``(delta, grad_el)`` to write into; every word is written, empty rows +0.
    ``dropout=(p, seed)``: the backward of ``spmm.gat_aggregate(.., dropout=(p, seed))`` (gespmm_gat_backward_el_dropout_f32): ``g``
    becomes ``edge_dropout``'s value of it, recomputed from the seed; ``w`` stays the undropped weight."""
    slope = _slope(negative_slope)
    _typed(torch.int32, rowptr=rowptr, colind=colind)
    _typed(torch.float32, el=el, er=er, stats=stats, grad_out=grad_out, feat=feat)
    _dropout_typed(dropout)
    dev, M, K, H, nnz = _gat_terms(rowptr, colind, el, er)
    _stats_array(stats, "stats", M, H, dev)
    F = _head_rows(grad_out, "grad_out", M, H, dev)
    _head_rows(feat, "feat", K, H, dev, F)
    if out is None:
        delta = torch.empty(M, H, dtype=torch.float32, device=dev)
        grad_el = torch.empty(M, H, dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out must be a pair of tensors (delta, grad_el)")
        delta, grad_el = out
        _node_result(delta, "out[0]", M, H, dev)
        _node_result(grad_el, "out[1]", M, H, dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
        with _on_device(dev):
            rc = lib.gespmm_gat_backward_el_dropout_f32(_ptr(rowptr), _ptr(colind), _ptr(el), _ptr(er), _ptr(stats), _ptr(grad_out),
                                                        _ptr(feat), _ptr(delta), _ptr(grad_el), M, K, H, F, nnz, slope, p, _ptr(seed),
                                                        _stream(dev))
        check(rc, "gespmm_gat_backward_el_dropout_f32")
        return delta, grad_el
    with _on_device(dev):
        rc = lib.gespmm_gat_backward_el_f32(_ptr(rowptr), _ptr(colind), _ptr(el), _ptr(er), _ptr(stats), _ptr(grad_out), _ptr(feat),
                                            _ptr(delta), _ptr(grad_el), M, K, H, F, nnz, slope, _stream(dev))
    check(rc, "gespmm_gat_backward_el_f32")
    return delta, grad_el


def gat_backward_er(colptr, rowind, el, er, stats, delta, grad_out, feat, negative_slope=None, out=None, dropout=None):
    """Backward of ``spmm.gat_aggregate`` for ``er`` with no edge array (gespmm_gat_backward_er_f32) -> ``grad_er`` f32[K, H]: the same
    per-entry ``gs`` as ``gat_backward_el``, recomputed with the same bits from ``delta`` (that call's first result), summed over the
    entries of each column in the pinned order of ``edge_segment_sum(colptr, .., order=csc_order)``. ``colptr, rowind`` are the CSC
    arrays (``graphs.transpose_csr``); no ``csc_order`` is needed. Every word is written, empty columns +0. ``dropout=(p, seed)``: as in
    ``gat_backward_el`` (gespmm_gat_backward_er_dropout_f32) — the walk over the columns recomputes the decisions of the walk over rows."""
    slope = _slope(negative_slope)
    _typed(torch.int32, colptr=colptr, rowind=rowind)
    _typed(torch.float32, el=el, er=er, stats=stats, delta=delta, grad_out=grad_out, feat=feat)
    _dropout_typed(dropout)
    K = _checked_rowptr(colptr)
    _node_array(er, "er", rows=K)
    _node_array(el, "el", like=er)
    dev = er.device
    _checked_rowptr(colptr, dev)
    _index_vector(rowind, "rowind", dev)
    M, H, nnz = el.shape[0], er.shape[1], rowind.numel()
    _stats_array(stats, "stats", M, H, dev)
    _node_result(delta, "delta", M, H, dev)
    F = _head_rows(grad_out, "grad_out", M, H, dev)
    _head_rows(feat, "feat", K, H, dev, F)
    if out is None:
        out = torch.empty(K, H, dtype=torch.float32, device=dev)
    else:
        _node_result(out, "out", K, H, dev)
    if dropout is not None:
        p, seed = _dropout(dropout, dev)
        with _on_device(dev):
            rc = lib.gespmm_gat_backward_er_dropout_f32(_ptr(colptr), _ptr(rowind), _ptr(el), _ptr(er), _ptr(stats), _ptr(delta),
                                                        _ptr(grad_out), _ptr(feat), _ptr(out), M, K, H, F, nnz, slope, p, _ptr(seed),
                                                        _stream(dev))
        check(rc, "gespmm_gat_backward_er_dropout_f32")
        return out
    with _on_device(dev):
        rc = lib.gespmm_gat_backward_er_f32(_ptr(colptr), _ptr(rowind), _ptr(el), _ptr(er), _ptr(stats), _ptr(delta), _ptr(grad_out),
                                            _ptr(feat), _ptr(out), M, K, H, F, nnz, slope, _stream(dev))
    check(rc, "gespmm_gat_backward_er_f32")
    return out
