"""SPMMFunction and GCNConv — mirror of the reference's pytorch-custom/op.py.

    SPMMFunction.apply(rowptr, colind, colptr, rowind, feat,
                       edge_weight_csr=None, edge_weight_csc=None)        op.py:8-36
    GCNConv(in_channels, out_channels, improved=False, cached=False,
            bias=True, normalize=True).forward(x, rowptr, colind, colptr, rowind,
            edge_weight_csr=None, edge_weight_csc=None)                   op.py:77-152

Semantics kept from the reference:
  * forward picks the unweighted kernel iff ``edge_weight_csr is None`` (op.py:11-14);
  * backward is the same SpMM on the caller-supplied CSC arrays, i.e.
    grad_feat = A^T @ grad_out (op.py:20-36); index tensors get no gradient;
  * giving ``edge_weight_csr`` without ``edge_weight_csc`` raises RuntimeError in
    backward (op.py:22-27);
  * edge weights are treated as constants (op.py:30-31 prints
    "[I] Treat edge weight as no_grad." — printed once per process here, not once
    per backward call).
Two optional extensions (off by default, so default behaviour is the reference's):
``need_edge_grad=True`` as an 8th argument returns d loss / d edge_weight_csr via
SDDMM, grad_w[e] = <grad_out[row(e), :], feat[col(e), :]> — the "SpMM fwd + SDDMM
bwd" pairing BASELINE.json's config 4 names; ``plans=(forward, backward)`` as a 9th
argument passes ``spmm.SpmmPlan`` objects (scratch kept across calls on a static graph).

GCNConv computes  D_in^-1/2 · A · (D_out^-1/2 ⊙ (X W)) + b  with degrees taken from
the rowptr / colptr differences (op.py:103-109, 128-147). ``glorot`` / ``zeros`` are
re-implemented (the reference imports them from torch_geometric, op.py:75).
With ``cached=True`` — which already promises a static graph for the cached normalisation — GCNConv
also keeps one SpmmPlan per direction (the analysis stage: sparse graphs are row-clustered once and launched from a
task table, dense graphs keep the split points of the cache-blocked path; results keep their bits).
``GCNConv(..., cached=True, tune_plans=True)`` (extension, off by default) additionally lets each plan pick its kernel by MEASUREMENT on the
first forward's operands (``SpmmPlan.tune``: a few extra launches once per direction; not under stream capture — run one eager step first).
``GCNConv(..., fused=True)`` (extension, off by default) runs the two scalings and the bias INSIDE the product
(``FusedGCNFunction`` on ``spmm.csr_spmm_fused``): three elementwise passes over an M x N matrix less in forward, two less in
backward, and the same output bits. It works with ``cached=True`` (plans) and without.
16-bit features (extension): ``SPMMFunction`` takes ``feat`` of ``torch.float16`` / ``torch.bfloat16`` (a ``.half()`` / ``.bfloat16()``
model, or ``torch.autocast``) and runs forward and backward on the 16-bit product (``spmm.csr_spmm`` with a 16-bit ``dense``: fp32 sum,
one rounding; ``grad_out`` arrives in the forward's dtype); edge weights stay fp32. GCNConv casts its two scaling vectors to the dtype
of ``x @ W`` so that the product stays 16-bit. fp32 only, with a TypeError otherwise: ``need_edge_grad=True``, ``fused=True``
and ``tune_plans=True``. The edge-weight gradient of a 16-bit model is one call away all the same:
``sddmm.csr_sddmm(rowptr, colind, grad_out, feat)`` takes fp16 / bf16 tensors as they are and returns the fp32 gradient.
Attention layers (extension): ``MultiHeadSPMMFunction`` is the aggregation with one weight per edge and head, ``MultiHeadSDDMMFunction``
the dot-product score s[e, h] = <q[row(e), h, :], k[col(e), h, :]>; each has the other as its backward (``spmm.csr_spmm_heads``,
``sddmm.csr_sddmm_heads``). ``MultiHeadSPMMFunction(..., heads_sddmm=True)`` computes the edge-weight gradient in one multi-head SDDMM
instead of one ``sddmm.csr_sddmm`` per head on copies (the default, kept as it was): same bits.
16-bit attention (extension): both functions take fp16 / bf16 node tensors (``feat``; ``q`` and ``k``) and run forward and backward on
``spmm.csr_spmm_heads_x16`` / ``sddmm.csr_sddmm_heads_x16``; everything edge-sized — scores, weights, their gradients — stays fp32.
``GATConv`` (default and ``fused_score=True`` paths) and ``TransformerConv(fused=False)`` therefore work as ``.half()`` / ``.bfloat16()``
models and under ``torch.autocast``, and so does ``GATv2Conv(fused=False)``, whose score runs on 16-bit node terms too
(``GATv2ScoreFunction`` on ``sddmm.gatv2_score_x16`` / ``gatv2_score_backward_x16``); the fused aggregation / backward,
``GATv2Conv(fused=True)`` and ``TransformerConv(fused=True)`` are fp32 only.
``EdgeSoftmaxFunction`` is the step between the two — softmax over the entries of each row, per head, with the leaky ReLU of a GAT
fused in (``softmax.edge_softmax`` and its backward kernel) — and ``GATConv`` the graph attention layer composed from the three.
``GATSoftmaxFunction`` is the first two in one: the softmax of el[row] + er[col] with no score array (``GATConv(fused_score=True)``).
``EdgeDropoutFunction`` is dropout on alpha with a mask recomputed from (seed, row, column, head), never stored (``GATConv(dropout=p)``).
``GATAggregateFunction`` is all three in one: no score and no attention array, nothing of size nnz x H saved (``GATConv(fused_aggregate=True)``).
GraphSAGE (extension): ``SpmmMaxFunction`` is the max over neighbours with a gradient — the forward saves the winning CSR position of
every output word (``spmm.csr_spmm_max_arg``), the backward adds ``grad_out`` where that position sits (``spmm.csr_spmm_max_backward``) —
and ``SAGEConv`` DGL's layer of that name with the ``mean``, ``gcn`` and ``pool`` aggregators. Both take fp16 / bf16 features
(``spmm.csr_spmm_max_arg_x16`` / ``csr_spmm_max_backward_x16``; ``mean`` as the valued 16-bit product with fp32 weights 1 / deg).
Graph transformers (extension): ``DotAttentionFunction`` is scaled dot-product attention over the edges in three fused launches
(``attention.dot_attention`` and its two backward passes: no score, no alpha, nothing of size nnz saved), ``TransformerConv`` PyG's layer
of that name on it (``fused=True``) or on the composition of the functions above (the default) — and on fp16 / bf16 q, k and v
(``attention.dot_attention_x16`` and its two backward passes), behind ``TransformerConv(fused=True, fused_x16=True)``.
``GATv2AttentionFunction`` is the same for GATv2 — score, softmax, dropout and aggregation in one launch on one gathered row per entry
(``attention.gatv2_attention`` and its two backward passes), behind ``GATv2Conv(fused=True)`` — and on fp16 / bf16 node terms
(``attention.gatv2_attention_x16`` and its two backward passes), behind ``GATv2Conv(fused=True, fused_x16=True)``.
The reference's ``normalize=False`` branch raises TypeError (``rowptr.shape(0)``,
op.py:133-134); here it does what the branch evidently intends: no scaling.
"""
import math

import torch
from torch.autograd.function import once_differentiable
from torch.nn import Parameter

from . import attention as _attention
from . import graphs as _graphs
from . import sddmm as _sddmm
from . import softmax as _softmax
from . import _lib
from . import spmm as _spmm

_warned_no_grad = False


def _csc_heads_order(csc_order, rows, cols, H, F, nnz, x16, plan):
    """The int32 edge order a multi-head backward hands to its product on the CSC arrays (``csr_spmm_heads(..., order=)``: the weights
    read through the order, no permuted copy), or None where that product has no ordered kernel — H = 1, H > 8, odd F in 16 bits —
    and the backward does ``graphs.take_edges`` plus the plain call. ``rows`` x ``cols``: the CSC product's shape (K x M). A plan
    always takes the order. An int64 ``csc_order`` is converted once, here, in the forward."""
    if plan is None and (_lib.heads_x16_route if x16 else _lib.heads_route)(rows, cols, H, F, nnz)[0] != 1:
        return None
    return (csc_order if csc_order.dtype == torch.int32 else csc_order.to(torch.int32)).contiguous()


def _csc_heads_product(ctx, colptr, rowind, csc_order, weight, dense):
    """grad = A(weight)^T @ dense on the CSC arrays, ``weight`` f32[nnz, H] in CSR edge order: read through the order (``order=``, handed
    over as ``spmm.OrderedValues`` in the place of the weights) where the forward found the ordered kernel, gathered otherwise."""
    values = _spmm.OrderedValues(weight, ctx.order) if ctx.order is not None else _graphs.take_edges(weight, csc_order)
    if ctx.x16:
        return _heads_x16_product(colptr, rowind, values, dense)
    return _spmm.csr_spmm_heads(colptr, rowind, values, dense, plan=ctx.bwd_plan)


def _heads_x16_product(rowptr, colind, values, dense):
    """``spmm.csr_spmm_heads_x16`` for the autograd functions. Where that op has no kernel (``_lib.heads_x16_route`` answers 0: H = 1,
    H > 8, odd F) it composes widen / fp32 product / narrow through a stream-ordered temporary, which it refuses on a capturing stream.
    There — and only there — the same composition is made of torch's allocations, which a capture may hold:
    ``csr_spmm_heads(rowptr, colind, values, dense.float()).to(dense.dtype)``, the bits the op documents."""
    if isinstance(values, torch.Tensor) and dense.is_cuda and torch.cuda.is_current_stream_capturing():
        M, K, (nnz, H) = rowptr.numel() - 1, dense.shape[0], values.shape
        F = math.prod(dense.shape[1:]) // max(H, 1)
        if _lib.heads_x16_route(M, K, H, F, nnz)[0] != 1:
            return _spmm.csr_spmm_heads(rowptr, colind, values, dense.float()).to(dense.dtype)
    return _spmm.csr_spmm_heads_x16(rowptr, colind, values, dense)


def _is_x16(t):
    return isinstance(t, torch.Tensor) and t.dtype in (torch.float16, torch.bfloat16)


class SPMMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rowptr, colind, colptr, rowind, feat, edge_weight_csr=None, edge_weight_csc=None,
                need_edge_grad=False, plans=None):
        fwd_plan, ctx.bwd_plan = plans if plans is not None else (None, None)
        ctx.fwd_plan = fwd_plan
        if need_edge_grad and feat.dtype != torch.float32:
            raise TypeError("need_edge_grad=True needs torch.float32 feat, got %s: on 16-bit tensors sddmm.csr_sddmm(rowptr, colind, grad_out, feat) "
                            "computes the (fp32) edge-weight gradient" % feat.dtype)
        if edge_weight_csr is None:
            out = _spmm.csr_spmm_no_edge_value(rowptr, colind, feat, plan=fwd_plan)
        else:
            out = _spmm.csr_spmm(rowptr, colind, edge_weight_csr, feat, plan=fwd_plan)
        ctx.backward_csc = (colptr, rowind, feat, edge_weight_csr, edge_weight_csc)
        ctx.forward_csr = (rowptr, colind)
        ctx.need_edge_grad = bool(need_edge_grad)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        global _warned_no_grad
        colptr, rowind, feat, edge_weight_csr, edge_weight_csc = ctx.backward_csc
        grad_out = grad_out.contiguous()
        grad_edge_weight = None
        if edge_weight_csr is not None:
            if edge_weight_csc is None:
                raise RuntimeError(
                    "Backward of SPMM require edge values in both src-first and dst-first order, "
                    "and do not support gradients for edge values. Call with SPMMFunction.apply("
                    "rowptr, colind, colptr, rowind, in_feat, edge_value_row_first, edge_value_col_first")
            grad_feat = _spmm.csr_spmm(colptr, rowind, edge_weight_csc, grad_out, plan=ctx.bwd_plan)
            if ctx.need_edge_grad:
                rowptr, colind = ctx.forward_csr
                grad_edge_weight = _sddmm.csr_sddmm(rowptr, colind, grad_out, feat.detach().contiguous(), plan=ctx.fwd_plan)
            elif not _warned_no_grad:
                print("[I] Treat edge weight as no_grad.")
                _warned_no_grad = True
        else:
            grad_feat = _spmm.csr_spmm_no_edge_value(colptr, rowind, grad_out, plan=ctx.bwd_plan)
        return None, None, None, None, grad_feat, grad_edge_weight, None, None, None


class FusedGCNFunction(torch.autograd.Function):
    """out = ((A @ (out_scale * feat)) * in_scale) + bias as ONE product (``spmm.csr_spmm_fused``), and its backward
    grad_feat = (A^T @ (in_scale * grad_out)) * out_scale as one product on the CSC arrays; grad_bias = grad_out.sum(0).

        FusedGCNFunction.apply(rowptr, colind, colptr, rowind, feat, out_scale, in_scale, bias,
                               edge_weight_csr=None, edge_weight_csc=None, plans=None)

    ``out_scale`` ([K] or [K, 1]: scales the rows of ``feat``), ``in_scale`` ([M] or [M, 1]: scales the rows of the result) and ``bias``
    ([N]) may each be None. The rules are SPMMFunction's: ``edge_weight_csc`` is required in backward when the product is weighted,
    index tensors and the two scales get no gradient, edge weights are treated as constants. Forward and the gradient with respect
    to ``feat`` have the bits of the unfused chain (mul, SPMMFunction, mul, add)."""

    @staticmethod
    def forward(ctx, rowptr, colind, colptr, rowind, feat, out_scale, in_scale, bias, edge_weight_csr=None, edge_weight_csc=None,
                plans=None):
        fwd_plan, ctx.bwd_plan = plans if plans is not None else (None, None)
        out = _spmm.csr_spmm_fused(rowptr, colind, edge_weight_csr, feat.contiguous(), col_scale=out_scale, row_scale=in_scale,
                                   bias=bias, plan=fwd_plan)
        ctx.backward_csc = (colptr, rowind, out_scale, in_scale, edge_weight_csr, edge_weight_csc)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        global _warned_no_grad
        colptr, rowind, out_scale, in_scale, edge_weight_csr, edge_weight_csc = ctx.backward_csc
        grad_out = grad_out.contiguous()
        if edge_weight_csr is not None:
            if edge_weight_csc is None:
                raise RuntimeError(
                    "Backward of SPMM require edge values in both src-first and dst-first order, "
                    "and do not support gradients for edge values. Call with SPMMFunction.apply("
                    "rowptr, colind, colptr, rowind, in_feat, edge_value_row_first, edge_value_col_first")
            if not _warned_no_grad:
                print("[I] Treat edge weight as no_grad.")
                _warned_no_grad = True
        grad_feat = None
        if ctx.needs_input_grad[4]:
            grad_feat = _spmm.csr_spmm_fused(colptr, rowind, edge_weight_csc, grad_out, col_scale=in_scale, row_scale=out_scale,
                                             plan=ctx.bwd_plan)
        grad_bias = grad_out.sum(0) if (ctx.has_bias and ctx.needs_input_grad[7]) else None
        return None, None, None, None, grad_feat, None, None, grad_bias, None, None, None


class MultiHeadSPMMFunction(torch.autograd.Function):
    """out[r, h, :] = sum_e weight[e, h] * feat[col(e), h, :] — the aggregation of a multi-head attention layer
    (``spmm.csr_spmm_heads``) with gradients for the features and, when asked for, the edge weights.

        MultiHeadSPMMFunction.apply(rowptr, colind, colptr, rowind, csc_order, feat, weight, plans=None, heads_sddmm=False)

    ``feat`` f32[K, H, F], ``weight`` f32[nnz, H] in CSR edge order; ``colptr, rowind, csc_order`` =
    ``graphs.transpose_csr(rowptr, colind, K, return_order=True)``; ``plans=(forward, backward)`` are ``spmm.SpmmPlan`` objects of the
    CSR and the CSC pattern. Backward: grad_feat is the same product on the CSC arrays with the weights read through ``csc_order``
    (``csr_spmm_heads(colptr, rowind, weight, grad_out, order=)``: no permuted copy of ``weight``; an int64 ``csc_order`` is converted to
    int32 once per forward — pass an int32 one) wherever the ordered kernel exists — ``_lib.heads_route`` answers 1 for the CSC
    product, or a plan is given — and with ``graphs.take_edges(weight, csc_order)`` elsewhere (H = 1, H > 8); the same bits either way;
    grad_weight[e, h] = <grad_out[row(e), h, :], feat[col(e), h, :]> is computed only when ``weight`` requires grad — by default as one
    ``sddmm.csr_sddmm`` per head on contiguous copies, with ``heads_sddmm=True`` as ONE ``sddmm.csr_sddmm_heads(rowptr, colind, grad_out,
    feat, plan=forward plan)`` on the tensors as they are (no copies, one launch). The two settings give the same bits on
    torch-allocated tensors (16-byte aligned: the per-head copies and the head slices take the same vector width).
    Index tensors get no gradient.

    16-bit ``feat`` (fp16 / bf16) with fp32 ``weight``: the output has ``feat``'s dtype (``spmm.csr_spmm_heads_x16``: fp32 sums, one
    rounding), grad_feat is ``csr_spmm_heads_x16`` on the CSC arrays with ``order=`` (``take_edges`` where ``_lib.heads_x16_route`` is 0: odd F
    too), grad_weight stays fp32 —
    ``sddmm.csr_sddmm_heads_x16(rowptr, colind, grad_out, feat)`` with ``heads_sddmm=True``, the 16-bit ``sddmm.csr_sddmm`` per head
    otherwise. ``plans=`` with 16-bit tensors raises TypeError (the 16-bit multi-head ops have no plan form). On a capturing stream,
    where ``_lib.heads_x16_route`` is 0 (H = 1, H > 8, odd F: the op's own composition allocates and is refused there), forward and
    grad_feat are ``csr_spmm_heads(..., feat.float()).to(feat.dtype)`` on torch's allocations — the same bits, so a 16-bit layer with one
    head replays from a captured graph."""

    @staticmethod
    def forward(ctx, rowptr, colind, colptr, rowind, csc_order, feat, weight, plans=None, heads_sddmm=False):
        fwd_plan, ctx.bwd_plan = plans if plans is not None else (None, None)
        ctx.fwd_plan = fwd_plan
        ctx.heads_sddmm = bool(heads_sddmm)
        ctx.x16 = _is_x16(feat)
        if ctx.x16 and plans is not None:
            raise TypeError("plans= needs torch.float32 feat, got %s: spmm.csr_spmm_heads_x16 has no plan form" % feat.dtype)
        feat_c, weight_c = feat.contiguous(), weight.contiguous()
        if ctx.x16:
            out = _heads_x16_product(rowptr, colind, weight_c, feat_c)
        else:
            out = _spmm.csr_spmm_heads(rowptr, colind, weight_c, feat_c, plan=fwd_plan)
        ctx.graph = (rowptr, colind, colptr, rowind, csc_order)
        ctx.order = None
        if ctx.needs_input_grad[5]:
            ctx.order = _csc_heads_order(csc_order, colptr.numel() - 1, rowptr.numel() - 1, weight_c.shape[1],
                                         math.prod(feat_c.shape[1:]) // max(weight_c.shape[1], 1), colind.numel(), ctx.x16, ctx.bwd_plan)
        ctx.save_for_backward(feat_c, weight_c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rowptr, colind, colptr, rowind, csc_order = ctx.graph
        feat, weight = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        grad_feat = grad_weight = None
        if ctx.needs_input_grad[5]:
            grad_feat = _csc_heads_product(ctx, colptr, rowind, csc_order, weight, grad_out)
        if ctx.needs_input_grad[6]:
            if ctx.heads_sddmm and ctx.x16:
                grad_weight = _sddmm.csr_sddmm_heads_x16(rowptr, colind, grad_out, feat)
            elif ctx.heads_sddmm:
                grad_weight = _sddmm.csr_sddmm_heads(rowptr, colind, grad_out, feat, plan=ctx.fwd_plan)
            else:
                H = weight.shape[1]
                grad_weight = torch.stack([_sddmm.csr_sddmm(rowptr, colind, grad_out[:, h, :].contiguous(), feat[:, h, :].contiguous())
                                           for h in range(H)], dim=1)
        return None, None, None, None, None, grad_feat, grad_weight, None, None


class MultiHeadSDDMMFunction(torch.autograd.Function):
    """s[e, h] = <q[row(e), h, :], k[col(e), h, :]> — the scores of a dot-product attention layer on the edges of a graph
    (``sddmm.csr_sddmm_heads``), with gradients for both operands.

        MultiHeadSDDMMFunction.apply(rowptr, colind, colptr, rowind, csc_order, q, k, plans=None) -> f32[nnz, H]

    ``q`` f32[M, H, F], ``k`` f32[K, H, F]; ``colptr, rowind, csc_order`` = ``graphs.transpose_csr(rowptr, colind, K,
    return_order=True)``; ``plans=(forward, backward)`` are ``spmm.SpmmPlan`` objects of the CSR and the CSC pattern. Backward is two
    multi-head products (``spmm.csr_spmm_heads``), each computed only for an input that requires grad:
    grad_q = A(grad_s) @ k on the CSR arrays, grad_k = A(grad_s)^T @ q on the CSC arrays with ``grad_s`` read through ``csc_order``
    (``order=``: no permuted copy; int64 is converted to int32 once per forward) where the ordered kernel exists or a plan is given, with
    ``graphs.take_edges(grad_s, csc_order)`` elsewhere (H = 1, H > 8, odd F in 16 bits) — the same bits.
    Index tensors get no gradient.

    16-bit ``q`` and ``k`` (both fp16 or both bf16): the score stays fp32 (``sddmm.csr_sddmm_heads_x16``), grad_q / grad_k are
    ``spmm.csr_spmm_heads_x16`` products with the fp32 ``grad_s`` and come back in the operands' dtype. ``plans=`` raises TypeError."""

    @staticmethod
    def forward(ctx, rowptr, colind, colptr, rowind, csc_order, q, k, plans=None):
        fwd_plan, ctx.bwd_plan = plans if plans is not None else (None, None)
        ctx.fwd_plan = fwd_plan
        ctx.x16 = _is_x16(q) or _is_x16(k)
        if ctx.x16 and plans is not None:
            raise TypeError("plans= needs torch.float32 q and k, got %s: sddmm.csr_sddmm_heads_x16 has no plan form" % q.dtype)
        q_c, k_c = q.contiguous(), k.contiguous()
        if ctx.x16:
            out = _sddmm.csr_sddmm_heads_x16(rowptr, colind, q_c, k_c)
        else:
            out = _sddmm.csr_sddmm_heads(rowptr, colind, q_c, k_c, plan=fwd_plan)
        ctx.graph = (rowptr, colind, colptr, rowind, csc_order)
        ctx.order = None
        if ctx.needs_input_grad[6]:
            ctx.order = _csc_heads_order(csc_order, colptr.numel() - 1, rowptr.numel() - 1, out.shape[1],
                                         math.prod(q_c.shape[1:]) // max(out.shape[1], 1), colind.numel(), ctx.x16, ctx.bwd_plan)
        ctx.save_for_backward(q_c, k_c)
        return out

    @staticmethod
    def backward(ctx, grad_s):
        rowptr, colind, colptr, rowind, csc_order = ctx.graph
        q, k = ctx.saved_tensors
        grad_s = grad_s.contiguous()
        grad_q = grad_k = None
        if ctx.x16:
            if ctx.needs_input_grad[5]:
                grad_q = _spmm.csr_spmm_heads_x16(rowptr, colind, grad_s, k)
            if ctx.needs_input_grad[6]:
                grad_k = _csc_heads_product(ctx, colptr, rowind, csc_order, grad_s, q)
            return None, None, None, None, None, grad_q, grad_k, None
        if ctx.needs_input_grad[5]:
            grad_q = _spmm.csr_spmm_heads(rowptr, colind, grad_s, k, plan=ctx.fwd_plan)
        if ctx.needs_input_grad[6]:
            grad_k = _csc_heads_product(ctx, colptr, rowind, csc_order, grad_s, q)
        return None, None, None, None, None, grad_q, grad_k, None


class EdgeSoftmaxFunction(torch.autograd.Function):
    """alpha[e, h] = softmax over the entries e of each CSR row of leaky_relu(score[e, h], negative_slope) — the attention weights of
    a graph attention layer (``softmax.edge_softmax``), with the gradient for ``score`` (``softmax.edge_softmax_backward``).

        EdgeSoftmaxFunction.apply(rowptr, score, negative_slope=None) -> f32, the shape of score

    ``score`` f32[nnz] or f32[nnz, H] in CSR edge order; ``negative_slope=None``: no leaky ReLU. Backward needs ``alpha`` alone — and
    the sign of ``score`` when a slope is given, so ``score`` is saved only then. ``rowptr`` gets no gradient."""

    @staticmethod
    def forward(ctx, rowptr, score, negative_slope=None):
        score_c = score.contiguous()
        alpha = _softmax.edge_softmax(rowptr, score_c, negative_slope=negative_slope)
        ctx.rowptr, ctx.negative_slope = rowptr, negative_slope
        if negative_slope is None:
            ctx.save_for_backward(alpha)
        else:
            ctx.save_for_backward(alpha, score_c)
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha):
        alpha = ctx.saved_tensors[0]
        score = ctx.saved_tensors[1] if ctx.negative_slope is not None else None
        grad_score = None
        if ctx.needs_input_grad[1]:
            grad_score = _softmax.edge_softmax_backward(ctx.rowptr, alpha, grad_alpha.contiguous(), score=score,
                                                        negative_slope=ctx.negative_slope)
        return None, grad_score, None


class EdgeDropoutFunction(torch.autograd.Function):
    """y[e, h] = keep(row(e), col(e), h) ? x[e, h] / (1 - p) : 0 — dropout on the attention coefficients of a CSR pattern with a mask
    that is a pure function of ``(seed, row, column, head)`` and is never stored (``softmax.edge_dropout``).

        EdgeDropoutFunction.apply(rowptr, colind, x, p, seed) -> f32, the shape of x

    ``x`` f32[nnz] or f32[nnz, H] in CSR edge order; ``p`` a Python number in [0, 1); ``seed`` an int32[2] device tensor. The op is
    its own adjoint: the backward is the same call on the gradient with the same seed, so the two seed words are all it saves —
    nothing edge-sized. The seed is read when the backward runs: do not overwrite it between a forward and its backward. Two entries
    with the same (row, column) share their decision."""

    @staticmethod
    def forward(ctx, rowptr, colind, x, p, seed):
        y = _softmax.edge_dropout(rowptr, colind, x.contiguous(), p, seed)
        ctx.graph, ctx.p = (rowptr, colind), float(p)
        ctx.save_for_backward(seed)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        rowptr, colind = ctx.graph
        (seed,) = ctx.saved_tensors
        grad_x = None
        if ctx.needs_input_grad[2]:
            grad_x = _softmax.edge_dropout(rowptr, colind, grad_y.contiguous(), ctx.p, seed)
        return None, None, grad_x, None, None


class GATSoftmaxFunction(torch.autograd.Function):
    """alpha[e, h] = softmax over the entries e of each CSR row of leaky_relu(el[row(e), h] + er[col(e), h], negative_slope) — the
    attention weights of a graph attention layer straight from the two per-node terms (``softmax.gat_edge_softmax``): no score array is
    written, saved or read.

        GATSoftmaxFunction.apply(rowptr, colind, colptr, csc_order, el, er, negative_slope=None) -> f32[nnz, H]

    ``el`` f32[M, H], ``er`` f32[K, H]; ``colptr, _, csc_order = graphs.transpose_csr(rowptr, colind, K, return_order=True)``. The
    bits of ``alpha`` are those of ``EdgeSoftmaxFunction`` on the score of ``MultiHeadSDDMMFunction`` with q = (el, 1), k = (1, er).
    Saved: ``alpha``, and ``el``, ``er`` when a slope is given (their sum's sign) — nothing else of size nnz H. Backward is two
    launches: ``softmax.gat_edge_softmax_backward`` (grad_score, and grad_el as its row sums), then ``softmax.edge_segment_sum`` on
    ``(colptr, csc_order)`` for grad_er, only when ``er`` requires grad. An int64 ``csc_order`` is converted to int32 once per forward
    and kept for the backward; pass an int32 one to convert it once per graph. Index tensors get no gradient."""

    @staticmethod
    def forward(ctx, rowptr, colind, colptr, csc_order, el, er, negative_slope=None):
        el_c, er_c = el.contiguous(), er.contiguous()
        alpha = _softmax.gat_edge_softmax(rowptr, colind, el_c, er_c, negative_slope=negative_slope)
        order = csc_order if csc_order.dtype == torch.int32 else csc_order.to(torch.int32)
        ctx.graph = (rowptr, colind, colptr, order.contiguous())
        ctx.negative_slope = negative_slope
        if negative_slope is None:
            ctx.save_for_backward(alpha)
        else:
            ctx.save_for_backward(alpha, el_c, er_c)
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha):
        rowptr, colind, colptr, order = ctx.graph
        alpha = ctx.saved_tensors[0]
        el, er = ctx.saved_tensors[1:] if ctx.negative_slope is not None else (None, None)
        grad_el = grad_er = None
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[5]:
            grad_score, grad_el = _softmax.gat_edge_softmax_backward(rowptr, colind, alpha, grad_alpha.contiguous(), el=el, er=er,
                                                                     negative_slope=ctx.negative_slope)
            if ctx.needs_input_grad[5]:
                grad_er = _softmax.edge_segment_sum(colptr, grad_score, order=order)
            if not ctx.needs_input_grad[4]:
                grad_el = None
        return None, None, None, None, grad_el, grad_er, None


class GATAggregateFunction(torch.autograd.Function):
    """out[r, h, :] = sum_e alpha[e, h] feat[col(e), h, :] with alpha = softmax over each row's entries of
    leaky_relu(el[row(e), h] + er[col(e), h], negative_slope) — the softmax AND the aggregation of a graph attention layer with no
    attention array (``softmax.gat_softmax_stats`` + ``spmm.gat_aggregate``): the weights are computed inside the product's kernel
    from el, er and two words per (row, head).

        GATAggregateFunction.apply(rowptr, colind, colptr, rowind, csc_order, el, er, feat, negative_slope=None,
                                   fused_backward=False, dropout_p=0.0, seed=None) -> f32[M, H, F]

    ``el`` f32[M, H], ``er`` f32[K, H], ``feat`` f32[K, H, F]; ``colptr, rowind, csc_order = graphs.transpose_csr(rowptr, colind, K,
    return_order=True)``. The output has the bits of ``MultiHeadSPMMFunction`` on ``GATSoftmaxFunction``'s alpha. Saved: ``el``,
    ``er``, ``feat`` and the statistics — node-sized tensors only. Backward, each part only when asked for: grad_feat is
    ``spmm.gat_aggregate(colptr, rowind, .., grad_out, transposed=True)`` (no alpha, no ``alpha[csc_order]`` copy); for grad_el /
    grad_er alpha is recomputed (``softmax.gat_edge_softmax``: the forward's bits) and the steps are those of the two functions
    above — ``sddmm.csr_sddmm_heads`` for grad_alpha, ``softmax.gat_edge_softmax_backward``, ``softmax.edge_segment_sum`` on
    ``(colptr, csc_order)`` — so every gradient has their bits; alpha and grad_alpha live only inside the backward. An int64
    ``csc_order`` is converted to int32 in every forward; pass an int32 one. Index tensors get no gradient.

    ``fused_backward=True``: grad_el / grad_er are ``softmax.gat_backward_el`` and ``softmax.gat_backward_er`` — two launches that
    recompute weight, dot product and softmax backward per entry from node-sized words; the backward allocates nothing of size
    nnz H either (``csc_order`` is not looked at). The second launch is made only when ``er`` requires grad. grad_feat is the same
    launch; grad_el / grad_er differ from the default's by the rounding of the dot product's summation order.

    ``dropout_p > 0`` with ``seed`` (int32[2] on the device): dropout on alpha, as ``EdgeDropoutFunction`` between the two functions
    above would apply it, with the mask recomputed wherever an entry is seen — in the aggregation, in its transposed form for
    grad_feat and in both backward passes (``dropout=(p, seed)`` of those calls; the default backward applies ``softmax.edge_dropout``
    to its transient grad_alpha). The two seed words are the only thing saved on top; with ``dropout_p == 0`` the launches are exactly
    those above."""

    @staticmethod
    def forward(ctx, rowptr, colind, colptr, rowind, csc_order, el, er, feat, negative_slope=None, fused_backward=False, dropout_p=0.0,
                seed=None):
        el_c, er_c, feat_c = el.contiguous(), er.contiguous(), feat.contiguous()
        dropout_p = float(dropout_p)
        if dropout_p != 0.0 and seed is None:
            raise ValueError("dropout_p needs a seed (an int32[2] device tensor)")
        ctx.dropout_p = dropout_p
        drop = (dropout_p, seed) if dropout_p != 0.0 else None
        stats = _softmax.gat_softmax_stats(rowptr, colind, el_c, er_c, negative_slope=negative_slope)
        out = _spmm.gat_aggregate(rowptr, colind, el_c, er_c, stats, feat_c, negative_slope=negative_slope, dropout=drop)
        order = None
        if not fused_backward:
            order = (csc_order if csc_order.dtype == torch.int32 else csc_order.to(torch.int32)).contiguous()
        ctx.graph = (rowptr, colind, colptr, rowind, order)
        ctx.negative_slope, ctx.fused_backward = negative_slope, bool(fused_backward)
        if drop is None:
            ctx.save_for_backward(el_c, er_c, feat_c, stats)
        else:
            ctx.save_for_backward(el_c, er_c, feat_c, stats, seed)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        rowptr, colind, colptr, rowind, order = ctx.graph
        el, er, feat, stats = ctx.saved_tensors[:4]
        drop = (ctx.dropout_p, ctx.saved_tensors[4]) if ctx.dropout_p != 0.0 else None
        slope = ctx.negative_slope
        grad_out = grad_out.contiguous()
        grad_el = grad_er = grad_feat = None
        if ctx.fused_backward and (ctx.needs_input_grad[5] or ctx.needs_input_grad[6]):  # node-sized tensors only
            delta, grad_el = _softmax.gat_backward_el(rowptr, colind, el, er, stats, grad_out, feat, negative_slope=slope, dropout=drop)
            if ctx.needs_input_grad[6]:
                grad_er = _softmax.gat_backward_er(colptr, rowind, el, er, stats, delta, grad_out, feat, negative_slope=slope,
                                                   dropout=drop)
            if not ctx.needs_input_grad[5]:
                grad_el = None
        elif ctx.needs_input_grad[5] or ctx.needs_input_grad[6]:  # (first: its three edge-sized temporaries are gone before grad_feat exists)
            alpha = _softmax.gat_edge_softmax(rowptr, colind, el, er, negative_slope=slope)
            grad_alpha = _sddmm.csr_sddmm_heads(rowptr, colind, grad_out, feat)
            if drop is not None:  # the gradient of the undropped alpha, in place
                _softmax.edge_dropout(rowptr, colind, grad_alpha, drop[0], drop[1], out=grad_alpha)
            grad_score, grad_el = _softmax.gat_edge_softmax_backward(rowptr, colind, alpha, grad_alpha, el=el if slope is not None else None,
                                                                     er=er if slope is not None else None, negative_slope=slope)
            del alpha, grad_alpha
            if ctx.needs_input_grad[6]:
                grad_er = _softmax.edge_segment_sum(colptr, grad_score, order=order)
            del grad_score
            if not ctx.needs_input_grad[5]:
                grad_el = None
        if ctx.needs_input_grad[7]:
            grad_feat = _spmm.gat_aggregate(colptr, rowind, el, er, stats, grad_out, negative_slope=slope, transposed=True, dropout=drop)
        return None, None, None, None, None, grad_el, grad_er, grad_feat, None, None, None, None


def glorot(tensor):
    """torch_geometric.nn.inits.glorot: U(-a, a), a = sqrt(6 / (fan_in + fan_out))."""
    if tensor is not None:
        stdv = math.sqrt(6.0 / (tensor.size(-2) + tensor.size(-1)))
        tensor.data.uniform_(-stdv, stdv)


def zeros(tensor):
    if tensor is not None:
        tensor.data.fill_(0)


class GCNConv(torch.nn.Module):
    """Graph convolution  out = D_in^-1/2 · A · (D_out^-1/2 ⊙ (x W)) + b  on the custom op.

    Constructor and ``forward`` signatures are the reference's (op.py:77-152). Degrees
    come from the pointer differences of the two index orders (``rowptr`` -> in-degree
    of the aggregating side, ``colptr`` -> out-degree of the source side); with
    ``cached=True`` the two scaling vectors are computed once and reused.
    """

    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, normalize=True,
                 **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.normalize = improved, cached, normalize
        self.tune_plans = bool(kwargs.pop("tune_plans", False))
        self.fused = bool(kwargs.pop("fused", False))  # extension: scalings and bias inside the product (FusedGCNFunction)
        # extension: products each cached plan is expected to serve (0 = 200: the reference trains 200 epochs, gcn_custom.py:134, one
        # forward and one backward product per layer and epoch) — the plans weigh their analysis against it (SpmmPlan)
        self.expected_launches = int(kwargs.pop("expected_launches", 0))
        self.weight = Parameter(torch.empty(in_channels, out_channels))
        self.bias = Parameter(torch.empty(out_channels)) if bias else None
        if not bias:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        zeros(self.bias)
        self.cached_result = None
        self.cached_num_edges = None
        self.cached_plans = None

    @staticmethod
    def _inv_sqrt_degree(indptr):
        degree = torch.diff(indptr).to(torch.float32)
        return (1 / torch.sqrt(degree)).unsqueeze(1)  # zero-degree rows give inf, as in the reference

    # names kept from the reference (op.py:103-109); both are the same pointer-difference rule
    in_deg_sqrt = _inv_sqrt_degree
    out_deg_sqrt = _inv_sqrt_degree

    def _scalings(self, x, rowptr, colptr):
        if self.cached and self.cached_result is not None:
            return self.cached_result
        if self.normalize:
            scal = (self._inv_sqrt_degree(rowptr), self._inv_sqrt_degree(colptr))
        else:  # the reference's branch here raises TypeError (rowptr.shape(0)); intent: no scaling
            scal = (torch.ones(rowptr.numel() - 1, 1, dtype=x.dtype, device=x.device),
                    torch.ones(colptr.numel() - 1, 1, dtype=x.dtype, device=x.device))
        self.cached_result = scal
        return scal

    def forward(self, x, rowptr, colind, colptr, rowind, edge_weight_csr=None, edge_weight_csc=None):
        h = x @ self.weight
        in_scale, out_scale = self._scalings(h, rowptr, colptr)
        if h.dtype in (torch.float16, torch.bfloat16):  # 16-bit features: keep `h * out_scale` (and with it the product) in that dtype
            if self.fused:
                raise TypeError("GCNConv(fused=True) needs torch.float32 features (the fused product is fp32 only), got %s" % h.dtype)
            in_scale, out_scale = in_scale.to(h.dtype), out_scale.to(h.dtype)
        if self.normalize and not self.fused:
            h = h * out_scale
        plans = None
        if self.cached:  # `cached` is the caller's promise of a static graph: keep the SpMM scratch as well
            # Keyed on the addresses only. That is safe: the plans hold strong references to the index tensors they were
            # made from, so those addresses cannot be recycled for another graph while the plans are alive, and SpmmPlan
            # itself notices in-place edits of the pattern through the tensors' version counters (and raises). The analysis
            # runs on the device and is weighed against the launches it serves (round 5): a com-Amazon-sized graph with communities
            # is clustered (~7 ms per direction), pubmed keeps its storage order (one validation pass, ~0.1 ms).
            key = (rowptr.data_ptr(), colind.data_ptr(), colptr.data_ptr(), rowind.data_ptr(), h.shape[1])
            if self.cached_plans is None or self.cached_plans[0] != key:
                n = rowptr.numel() - 1
                self.cached_plans = (key, (_spmm.SpmmPlan(rowptr, colind, colptr.numel() - 1, h.shape[1],
                                                          expected_launches=self.expected_launches),
                                           _spmm.SpmmPlan(colptr, rowind, n, h.shape[1], expected_launches=self.expected_launches)))
                if self.tune_plans and not torch.cuda.is_current_stream_capturing():
                    with torch.no_grad():  # kernel choice by measurement, once per direction (same bits whichever wins)
                        fwd, bwd = self.cached_plans[1]
                        if edge_weight_csr is not None:
                            fwd._sync_inputs(rowptr, colind, edge_weight_csr, h.detach(), fwd.shape[4])
                        out0 = fwd.tune((h.detach() * out_scale).contiguous() if (self.fused and self.normalize) else h.detach().contiguous())
                        if edge_weight_csc is not None:
                            bwd._sync_inputs(colptr, rowind, edge_weight_csc, out0, bwd.shape[4])
                        bwd.tune(out0)
            plans = self.cached_plans[1]
        if self.fused:
            return FusedGCNFunction.apply(rowptr, colind, colptr, rowind, h, out_scale if self.normalize else None,
                                          in_scale if self.normalize else None, self.bias, edge_weight_csr, edge_weight_csc, plans)
        h = SPMMFunction.apply(rowptr, colind, colptr, rowind, h, edge_weight_csr, edge_weight_csc, False, plans)
        if self.normalize:
            h = h * in_scale
        return h if self.bias is None else h + self.bias

    def __repr__(self):
        return "%s(%d, %d)" % (type(self).__name__, self.in_channels, self.out_channels)


class GATConv(torch.nn.Module):
    """Graph attention layer (Velickovic et al., 2018) on the library's ops, H heads in every call:

        xw = (x W).view(K, H, F),  el = <xw, att_dst>,  er = <xw, att_src>                                     (dense, torch)
        score[e, h] = el[row(e), h] + er[col(e), h]                ``MultiHeadSDDMMFunction`` on q = (el, 1), k = (1, er)
        alpha = softmax over each row's entries of leaky_relu(score, negative_slope)      ``EdgeSoftmaxFunction``
        out[r, h, :] = sum_e alpha[e, h] xw[col(e), h, :]          ``MultiHeadSPMMFunction(..., heads_sddmm=True)``

    then heads concatenated (``concat=True``: [M, H F]) or averaged ([M, F]), plus bias. No torch index op touches an edge array: the
    additive score is a width-2 dot product whose pinned chain is fmaf(1, er, fmaf(el, 1, 0)) = fl(el + er) (or el + er across two lanes),
    and its backward hands grad_el and grad_er back as component 0 of grad_q and component 1 of grad_k.

        GATConv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, bias=True, fused_score=False,
                fused_aggregate=False, fused_backward=False, dropout=0.0)
        forward(x, rowptr, colind, colptr, rowind, csc_order, attn_seed=None)

    ``fused_score=True``: the score and the softmax are ONE ``GATSoftmaxFunction`` — el + er is added inside the softmax kernel, no
    score, q or k tensor exists, and the backward sums grad_score over rows and columns in two launches. Same output bits. Pass an
    int32 ``csc_order`` then (an int64 one is converted in every forward).

    ``fused_aggregate=True`` (implies the fused score): the softmax AND the aggregation are ONE ``GATAggregateFunction`` — alpha is
    never an array. The forward keeps two words per (node, head) instead of ``[nnz, H]``, the feature gradient is one product on the
    CSC arrays with no ``alpha[csc_order]`` copy, and only the backward for ``att_dst`` / ``att_src`` recomputes alpha, transiently.
    Output and all gradients have the bits of ``fused_score=True``. Off by default.

    ``fused_backward=True`` (implies the fused aggregation): that backward recomputes nothing edge-sized either — the gradients for
    ``att_dst`` / ``att_src`` come from ``softmax.gat_backward_el`` / ``gat_backward_er``, so a layer allocates no ``[nnz, H]`` array
    forward or backward. Same output bits; the two gradients agree to rounding. Off by default.

    ``dropout=p`` (0 <= p < 1): dropout on the attention coefficients, as in the paper (p = 0.6 on the citation graphs), in training
    mode and in all four paths — ``EdgeDropoutFunction`` on alpha where alpha exists, ``dropout=`` of the fused calls where it does
    not. The mask is a pure function of ``(seed, row, column, head)`` and is never stored, so the fused paths still allocate nothing of
    size ``[nnz, H]``. Each training forward draws the two seed words from torch's device generator (``torch.manual_seed`` fixes the
    mask; a draw inside a captured region is fresh at every replay) unless ``attn_seed``, an int32[2] device tensor, is given. Outputs
    of the four paths are bit-equal under one seed. Two entries with the same (row, column) — a multigraph — share their decision.
    In ``eval()`` mode or with ``dropout == 0`` the layer makes exactly the launches it makes without the argument.

    The graph is square (row r and column r are the same node; add self-loops so that no row is empty);
    ``colptr, rowind, csc_order = graphs.transpose_csr(rowptr, colind, K, return_order=True)``.

    16-bit features (a ``.half()`` / ``.bfloat16()`` layer, or ``torch.autocast``), default and ``fused_score=True`` paths: ``xw`` stays
    16-bit, ``el`` and ``er`` — node-sized — are computed by torch from it and widened (``.float()``), score, softmax and dropout are the
    unchanged fp32 ops, the aggregation is the 16-bit product (``MultiHeadSPMMFunction`` on ``spmm.csr_spmm_heads_x16``: fp32 sums, one
    rounding) and the bias add is torch's. ``fused_aggregate`` / ``fused_backward`` are fp32 only: 16-bit features raise TypeError."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, bias=True, fused_score=False,
                 fused_aggregate=False, fused_backward=False, dropout=0.0):
        super().__init__()
        self.dropout = float(dropout)
        if not (0.0 <= self.dropout < 1.0):
            raise ValueError("dropout must be in [0, 1), got %r" % (dropout,))
        self.fused_backward = bool(fused_backward)
        self.fused_aggregate = bool(fused_aggregate) or self.fused_backward
        self.fused_score = bool(fused_score) or self.fused_aggregate
        if heads < 1:
            raise ValueError("heads must be at least 1")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, int(heads)
        self.concat, self.negative_slope = bool(concat), negative_slope
        self.weight = Parameter(torch.empty(in_channels, self.heads * out_channels))
        self.att_dst = Parameter(torch.empty(1, self.heads, out_channels))  # scores the aggregating node (the row of an edge)
        self.att_src = Parameter(torch.empty(1, self.heads, out_channels))  # scores the neighbour (the column of an edge)
        self.bias = Parameter(torch.empty(self.heads * out_channels if self.concat else out_channels)) if bias else None
        if not bias:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        glorot(self.att_dst)
        glorot(self.att_src)
        zeros(self.bias)

    def forward(self, x, rowptr, colind, colptr, rowind, csc_order, attn_seed=None):
        n, H, F = x.shape[0], self.heads, self.out_channels
        p, seed = 0.0, None
        if self.training and self.dropout > 0.0:
            p = self.dropout
            seed = attn_seed
            if seed is None:  # two 32-bit words from the device generator: no host synchronisation
                seed = torch.randint(-(2 ** 31), 2 ** 31, (2,), dtype=torch.int32, device=x.device)
        if rowptr.numel() != n + 1 or colptr.numel() != n + 1:
            raise ValueError("GATConv needs a square graph: rowptr and colptr must have x.size(0) + 1 entries")
        xw = (x @ self.weight).view(n, H, F)
        if self.fused_aggregate and _is_x16(xw):
            raise TypeError("GATConv(fused_aggregate=True / fused_backward=True) needs torch.float32 features, got %s: "
                            "spmm.gat_aggregate (GATAggregateFunction) is fp32 only" % xw.dtype)
        el = (xw * self.att_dst).sum(-1).float()  # (node-sized; fp32 features: the same tensor)
        er = (xw * self.att_src).sum(-1).float()
        if self.fused_aggregate:
            if seed is None:
                out = GATAggregateFunction.apply(rowptr, colind, colptr, rowind, csc_order, el, er, xw, self.negative_slope,
                                                 self.fused_backward)
            else:
                out = GATAggregateFunction.apply(rowptr, colind, colptr, rowind, csc_order, el, er, xw, self.negative_slope,
                                                 self.fused_backward, p, seed)
            out = out.reshape(n, H * F) if self.concat else out.mean(dim=1)
            return out if self.bias is None else out + self.bias
        if self.fused_score:
            alpha = GATSoftmaxFunction.apply(rowptr, colind, colptr, csc_order, el, er, self.negative_slope)
        else:
            q = torch.stack((el, torch.ones_like(el)), dim=-1)  # [n, H, 2]
            k = torch.stack((torch.ones_like(er), er), dim=-1)
            score = MultiHeadSDDMMFunction.apply(rowptr, colind, colptr, rowind, csc_order, q, k)
            alpha = EdgeSoftmaxFunction.apply(rowptr, score, self.negative_slope)
        if seed is not None:
            alpha = EdgeDropoutFunction.apply(rowptr, colind, alpha, p, seed)
        out = MultiHeadSPMMFunction.apply(rowptr, colind, colptr, rowind, csc_order, xw, alpha, None, True)
        out = out.reshape(n, H * F) if self.concat else out.mean(dim=1)
        return out if self.bias is None else out + self.bias

    def __repr__(self):
        return "%s(%d, %d, heads=%d)" % (type(self).__name__, self.in_channels, self.out_channels, self.heads)


class GATv2ScoreFunction(torch.autograd.Function):
    """score[e, h] = sum_f att[h, f] leaky_relu(xl[row(e), h, f] + xr[col(e), h, f], negative_slope) — the attention score of GATv2
    (Brody et al.) on the entries of a CSR pattern (``sddmm.gatv2_score``), with gradients for all three operands.

        GATv2ScoreFunction.apply(rowptr, colind, colptr, rowind, csc_order, xl, xr, att, negative_slope) -> f32[nnz, H]

    ``xl`` f32[M, H, F] (the aggregating node), ``xr`` f32[K, H, F] (the neighbour), ``att`` f32[H, F]; ``colptr, rowind, csc_order =
    graphs.transpose_csr(rowptr, colind, K, return_order=True)``; ``negative_slope=None``: no leaky ReLU. Forward: one launch. Backward:
    the row pass of ``sddmm.gatv2_score_backward`` when ``xl`` or ``att`` needs a gradient (grad_att is the sum over nodes of its second,
    node-sized result), the column pass on the CSC arrays when ``xr`` does. Saved: the three operands — no saved or allocated tensor
    has nnz * H * F words. An int64 ``csc_order`` is converted to int32 in every forward; pass an int32 one. Index tensors get no
    gradient.

    16-bit ``xl`` and ``xr`` (both ``torch.float16`` or both ``torch.bfloat16``; ``att`` must be fp32): the same three launches through
    ``sddmm.gatv2_score_x16`` / ``sddmm.gatv2_score_backward_x16``. The score stays f32[nnz, H], the 16-bit operands are what is saved,
    ``grad_xl`` / ``grad_xr`` come back in their dtype (fp32 chains, one rounding) and ``grad_att`` as fp32 (``att_part.sum(0)``)."""

    @staticmethod
    def forward(ctx, rowptr, colind, colptr, rowind, csc_order, xl, xr, att, negative_slope=None):
        xl_c, xr_c, att_c = xl.contiguous(), xr.contiguous(), att.contiguous()
        ctx.x16 = _is_x16(xl) or _is_x16(xr)
        score_op = _sddmm.gatv2_score_x16 if ctx.x16 else _sddmm.gatv2_score
        score = score_op(rowptr, colind, xl_c, xr_c, att_c, negative_slope=negative_slope)
        order = (csc_order if csc_order.dtype == torch.int32 else csc_order.to(torch.int32)).contiguous()
        ctx.graph = (rowptr, colind, colptr, rowind, order)
        ctx.negative_slope = negative_slope
        ctx.save_for_backward(xl_c, xr_c, att_c)
        return score

    @staticmethod
    def backward(ctx, grad_score):
        rowptr, colind, colptr, rowind, order = ctx.graph
        xl, xr, att = ctx.saved_tensors
        slope = ctx.negative_slope
        grad_score = grad_score.contiguous()
        backward_op = _sddmm.gatv2_score_backward_x16 if ctx.x16 else _sddmm.gatv2_score_backward
        grad_xl = grad_xr = grad_att = None
        if ctx.needs_input_grad[5] or ctx.needs_input_grad[7]:
            want_att = bool(ctx.needs_input_grad[7])
            res = backward_op(rowptr, colind, grad_score, xl, xr, att, negative_slope=slope, want_att_part=want_att)
            grad_xl, att_part = res if want_att else (res, None)
            if want_att:
                grad_att = att_part.sum(0)
                del att_part
            if not ctx.needs_input_grad[5]:
                grad_xl = None
        if ctx.needs_input_grad[6]:
            grad_xr = backward_op(colptr, rowind, grad_score, xr, xl, att, negative_slope=slope, order=order)
        return None, None, None, None, None, grad_xl, grad_xr, grad_att, None


class GATv2AttentionFunction(torch.autograd.Function):
    """out[r, h, :] = sum_e softmax_row(sum_f att[h, f] leaky_relu(xl[r, h, f] + xr[col(e), h, f]))_e xr[col(e), h, :] — the whole attention
    of GATv2 (score, softmax, dropout, aggregation) over the edges of a graph in ONE launch (``attention.gatv2_attention``), with
    gradients for xl, xr and att in two more (``attention.gatv2_attention_backward_row`` over the rows,
    ``attention.gatv2_attention_backward_col`` over the columns).

        GATv2AttentionFunction.apply(rowptr, colind, colptr, rowind, xl, xr, att, negative_slope=None, dropout_p=0.0, seed=None) -> f32[M, H, F]

    ``xl`` f32[M, H, F] (the aggregating node), ``xr`` f32[K, H, F] (the neighbour: scored AND aggregated), ``att`` f32[H, F]; ``colptr,
    rowind = graphs.transpose_csr(rowptr, colind, K)`` — no ``csc_order``; ``negative_slope=None``: no leaky ReLU. No score and no
    attention array exists in either direction: the function saves ``xl, xr, att, out`` and the [M, H, 2] softmax statistics (and the
    two seed words), nothing of size nnz. ``dropout_p > 0`` with ``seed`` (int32[2] on the device): dropout on the coefficients with
    ``EdgeDropoutFunction``'s mask, recomputed in all three launches; the seed is read when the backward runs. The row pass runs when
    any of the three needs a gradient (``att``'s is the sum over nodes of a node-sized result asked for only then), the column pass
    only when ``xr`` does. ``xl is xr`` (shared weights) works: autograd adds the two gradients. F <= 512. Index tensors get no
    gradient.

    16-bit ``xl`` and ``xr`` (both ``torch.float16`` or both ``torch.bfloat16``; ``att`` must be fp32): the same three launches through
    ``attention.gatv2_attention_x16`` / ``gatv2_attention_backward_row_x16`` / ``gatv2_attention_backward_col_x16``. Saved: the 16-bit
    ``xl, xr, out`` and the fp32 ``att, stats``. ``out``, ``grad_xl`` and ``grad_xr`` come in the features' dtype (fp32 sums, one
    rounding each), ``grad_att`` as fp32 (``att_part.sum(0)``)."""

    @staticmethod
    def forward(ctx, rowptr, colind, colptr, rowind, xl, xr, att, negative_slope=None, dropout_p=0.0, seed=None):
        dropout_p = float(dropout_p)
        if dropout_p != 0.0 and seed is None:
            raise ValueError("dropout_p needs a seed (an int32[2] device tensor)")
        drop = (dropout_p, seed) if dropout_p != 0.0 else None
        xl_c, xr_c, att_c = xl.contiguous(), xr.contiguous(), att.contiguous()
        ctx.x16 = _is_x16(xl) or _is_x16(xr)
        forward_op = _attention.gatv2_attention_x16 if ctx.x16 else _attention.gatv2_attention
        out, stats = forward_op(rowptr, colind, xl_c, xr_c, att_c, negative_slope=negative_slope, dropout=drop)
        ctx.graph = (rowptr, colind, colptr, rowind)
        ctx.negative_slope, ctx.dropout_p = negative_slope, dropout_p
        if drop is None:
            ctx.save_for_backward(xl_c, xr_c, att_c, out, stats)
        else:
            ctx.save_for_backward(xl_c, xr_c, att_c, out, stats, seed)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        rowptr, colind, colptr, rowind = ctx.graph
        xl, xr, att, out, stats = ctx.saved_tensors[:5]
        drop = (ctx.dropout_p, ctx.saved_tensors[5]) if ctx.dropout_p != 0.0 else None
        slope = ctx.negative_slope
        row_op = _attention.gatv2_attention_backward_row_x16 if ctx.x16 else _attention.gatv2_attention_backward_row
        col_op = _attention.gatv2_attention_backward_col_x16 if ctx.x16 else _attention.gatv2_attention_backward_col
        grad_xl = grad_xr = grad_att = None
        if any(ctx.needs_input_grad[4:7]):
            grad_out = grad_out.contiguous()
            want_att = bool(ctx.needs_input_grad[6])
            res = row_op(rowptr, colind, xl, xr, att, stats, out, grad_out, negative_slope=slope, dropout=drop, want_att_part=want_att)
            delta, grad_xl = res[0], res[1]
            if want_att:
                grad_att = res[2].sum(0)
            del res
            if not ctx.needs_input_grad[4]:
                grad_xl = None
            if ctx.needs_input_grad[5]:
                grad_xr = col_op(colptr, rowind, xl, xr, att, stats, delta, grad_out, negative_slope=slope, dropout=drop)
        return None, None, None, None, grad_xl, grad_xr, grad_att, None, None, None


class GATv2Conv(torch.nn.Module):
    """GATv2 layer (Brody et al., "How attentive are graph attention networks?") on the library's ops, H heads in every call:

        xl = (x W_dst).view(n, H, F),  xr = (x W_src).view(n, H, F)                                        (dense, torch)
        score[e, h] = sum_f att[h, f] leaky_relu(xl[row(e), h, f] + xr[col(e), h, f])     ``GATv2ScoreFunction``: nothing of size nnz H F
        alpha = softmax over each row's entries of score                                  ``EdgeSoftmaxFunction`` (no second leaky ReLU)
        out[r, h, :] = sum_e alpha[e, h] xr[col(e), h, :]                                 ``MultiHeadSPMMFunction(..., heads_sddmm=True)``

    then heads concatenated (``concat=True``: [n, H F]) or averaged ([n, F]), plus bias.

        GATv2Conv(in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, bias=True, share_weights=False, dropout=0.0,
                  fused=False, fused_x16=False)
        forward(x, rowptr, colind, colptr, rowind, csc_order, attn_seed=None)

    ``share_weights=True``: one matrix for both terms (W_dst is W_src). ``dropout=p`` (0 <= p < 1): ``EdgeDropoutFunction`` on alpha in
    training mode, the seed handled exactly as in ``GATConv`` (two words from torch's device generator unless ``attn_seed``, an int32[2]
    device tensor, is given); in ``eval()`` mode or with ``dropout == 0`` the layer makes exactly the launches it makes without it.
    With ``fused=False`` (the default) the ``[nnz, H]`` score and alpha arrays exist, with their gradients, and alpha is read through
    ``csc_order`` in the backward.

    ``fused=True`` runs ``GATv2AttentionFunction`` instead: score, softmax, dropout and aggregation are ONE launch on one gathered row
    per entry, the backward two more, and a training step allocates nothing of size ``[nnz, H]`` in either direction. It serves
    ``out_channels <= 512`` (ValueError at construction beyond), does not read ``csc_order``, and applies the mask of ``fused=False``
    under one ``attn_seed``; outputs and gradients of the two settings agree to rounding. Off by default.

    The graph is square (row r and column r are the same node; add self-loops so that no row is empty);
    ``colptr, rowind, csc_order = graphs.transpose_csr(rowptr, colind, K, return_order=True)``.

    16-bit features (a ``.half()`` / ``.bfloat16()`` layer, or ``torch.autocast``) with ``fused=False``: ``xl`` and ``xr`` stay 16-bit,
    ``att`` is passed as ``self.att.view(H, F).float()`` (autograd rounds its gradient back into the parameter's dtype), the score is
    ``GATv2ScoreFunction`` on ``sddmm.gatv2_score_x16`` (fp32 result; both gradient passes on ``sddmm.gatv2_score_backward_x16``),
    softmax and dropout are the unchanged fp32 ops, the aggregation is the 16-bit product (``MultiHeadSPMMFunction`` on
    ``spmm.csr_spmm_heads_x16``: fp32 sums, one rounding) and the bias add is torch's. ``share_weights=True`` works as in fp32.
    ``fused=True`` alone refuses 16-bit features with a TypeError.

    ``fused=True, fused_x16=True``: 16-bit features run ``GATv2AttentionFunction`` on the 16-bit terms (``attention.gatv2_attention_x16``
    and its two backward passes: fp32 sums, one rounding per 16-bit result, nothing of size ``[nnz, H]``), with ``att`` passed as
    ``self.att.view(H, F).float()`` as in the unfused 16-bit path; fp32 features run exactly what ``fused=True`` runs. The keyword exists
    because the refusal of ``fused=True`` on 16-bit features is pinned by committed tests; it is to be folded into ``fused=True`` when
    those tests may change. ``fused_x16=True`` without ``fused=True`` is a ValueError."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, bias=True, share_weights=False, dropout=0.0,
                 fused=False, fused_x16=False):
        super().__init__()
        if fused_x16 and not fused:
            raise ValueError("fused_x16=True selects the 16-bit form of the fused attention: it needs fused=True")
        self.fused_x16 = bool(fused_x16)
        if fused and out_channels > _attention.GATV2_ATTENTION_MAX_F:
            raise ValueError("fused=True serves out_channels <= %d (a head slice is held in registers), got %d" %
                             (_attention.GATV2_ATTENTION_MAX_F, out_channels))
        self.fused = bool(fused)
        self.dropout = float(dropout)
        if not (0.0 <= self.dropout < 1.0):
            raise ValueError("dropout must be in [0, 1), got %r" % (dropout,))
        if heads < 1:
            raise ValueError("heads must be at least 1")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, int(heads)
        self.concat, self.negative_slope, self.share_weights = bool(concat), negative_slope, bool(share_weights)
        self.weight_src = Parameter(torch.empty(in_channels, self.heads * out_channels))  # the neighbour's term (the column of an edge)
        if self.share_weights:
            self.weight_dst = self.weight_src
        else:
            self.weight_dst = Parameter(torch.empty(in_channels, self.heads * out_channels))  # the aggregating node's term (the row)
        self.att = Parameter(torch.empty(1, self.heads, out_channels))
        if bias:
            self.bias = Parameter(torch.empty(self.heads * out_channels if self.concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight_src)
        if not self.share_weights:
            glorot(self.weight_dst)
        glorot(self.att)
        zeros(self.bias)

    def forward(self, x, rowptr, colind, colptr, rowind, csc_order, attn_seed=None):
        n, H, F = x.shape[0], self.heads, self.out_channels
        p, seed = 0.0, None
        if self.training and self.dropout > 0.0:
            p = self.dropout
            seed = attn_seed
            if seed is None:  # two 32-bit words from the device generator: no host synchronisation
                seed = torch.randint(-(2 ** 31), 2 ** 31, (2,), dtype=torch.int32, device=x.device)
        if rowptr.numel() != n + 1 or colptr.numel() != n + 1:
            raise ValueError("GATv2Conv needs a square graph: rowptr and colptr must have x.size(0) + 1 entries")
        xr = (x @ self.weight_src).view(n, H, F)
        xl = xr if self.share_weights else (x @ self.weight_dst).view(n, H, F)
        if self.fused:
            att = self.att.view(H, F)
            if _is_x16(xl) or _is_x16(xr):
                if not self.fused_x16:
                    raise TypeError("GATv2Conv(fused=True) needs torch.float32 features, got %s: attention.gatv2_attention "
                                    "(GATv2AttentionFunction) is fp32 only here; fused_x16=True selects the 16-bit form" % xr.dtype)
                att = att.float()  # (autograd rounds its gradient back into the parameter's dtype)
            out = GATv2AttentionFunction.apply(rowptr, colind, colptr, rowind, xl, xr, att, self.negative_slope, p, seed)
            out = out.reshape(n, H * F) if self.concat else out.mean(dim=1)
            return out if self.bias is None else out + self.bias
        # (att as fp32 — the same tensor in an fp32 layer; in a 16-bit one autograd rounds its gradient back into the parameter's dtype)
        score = GATv2ScoreFunction.apply(rowptr, colind, colptr, rowind, csc_order, xl, xr, self.att.view(H, F).float(),
                                         self.negative_slope)
        alpha = EdgeSoftmaxFunction.apply(rowptr, score, None)
        if seed is not None:
            alpha = EdgeDropoutFunction.apply(rowptr, colind, alpha, p, seed)
        out = MultiHeadSPMMFunction.apply(rowptr, colind, colptr, rowind, csc_order, xr, alpha, None, True)
        out = out.reshape(n, H * F) if self.concat else out.mean(dim=1)
        return out if self.bias is None else out + self.bias

    def __repr__(self):
        return "%s(%d, %d, heads=%d)" % (type(self).__name__, self.in_channels, self.out_channels, self.heads)


class DotAttentionFunction(torch.autograd.Function):
    """out[r, h, :] = sum_e softmax_row(scale <q[r, h, :], k[col(e), h, :]>)_e v[col(e), h, :] — scaled dot-product attention over the
    edges of a graph in ONE launch (``attention.dot_attention``), with gradients for q, k and v in two more
    (``attention.dot_attention_backward_q`` over the rows, ``attention.dot_attention_backward_kv`` over the columns).

        DotAttentionFunction.apply(q, k, v, rowptr, colind, colptr, rowind, scale=None, dropout_p=0.0, seed=None) -> f32[M, H, F]

    ``q`` f32[M, H, F], ``k`` and ``v`` f32[K, H, F]; ``colptr, rowind = graphs.transpose_csr(rowptr, colind, K)`` — no ``csc_order``;
    ``scale=None``: 1 / sqrt(F). No score and no attention array exists in either direction: the function saves ``q, k, v, out`` and the
    [M, H, 2] softmax statistics (and the two seed words), nothing of size nnz. ``dropout_p > 0`` with ``seed`` (int32[2] on the device):
    dropout on the coefficients with ``EdgeDropoutFunction``'s mask, recomputed in all three launches; the seed is read when the backward
    runs. F <= 512. Index tensors get no gradient. Both backward launches run whenever any of q, k, v requires grad.

    16-bit ``q``, ``k`` and ``v`` (all ``torch.float16`` or all ``torch.bfloat16``; anything mixed is a TypeError): the same three
    launches through ``attention.dot_attention_x16`` / ``dot_attention_backward_q_x16`` / ``dot_attention_backward_kv_x16``. Saved: the
    16-bit ``q, k, v, out`` and the fp32 ``stats``. ``out``, ``grad_q``, ``grad_k`` and ``grad_v`` come in the inputs' dtype (fp32 sums,
    one rounding each)."""

    @staticmethod
    def forward(ctx, q, k, v, rowptr, colind, colptr, rowind, scale=None, dropout_p=0.0, seed=None):
        dropout_p = float(dropout_p)
        if dropout_p != 0.0 and seed is None:
            raise ValueError("dropout_p needs a seed (an int32[2] device tensor)")
        drop = (dropout_p, seed) if dropout_p != 0.0 else None
        q_c, k_c, v_c = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.x16 = _is_x16(q) or _is_x16(k) or _is_x16(v)
        forward_op = _attention.dot_attention_x16 if ctx.x16 else _attention.dot_attention
        out, stats = forward_op(rowptr, colind, q_c, k_c, v_c, scale=scale, dropout=drop)
        ctx.graph = (rowptr, colind, colptr, rowind)
        ctx.scale, ctx.dropout_p = scale, dropout_p
        if drop is None:
            ctx.save_for_backward(q_c, k_c, v_c, out, stats)
        else:
            ctx.save_for_backward(q_c, k_c, v_c, out, stats, seed)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        rowptr, colind, colptr, rowind = ctx.graph
        q, k, v, out, stats = ctx.saved_tensors[:5]
        drop = (ctx.dropout_p, ctx.saved_tensors[5]) if ctx.dropout_p != 0.0 else None
        q_op = _attention.dot_attention_backward_q_x16 if ctx.x16 else _attention.dot_attention_backward_q
        kv_op = _attention.dot_attention_backward_kv_x16 if ctx.x16 else _attention.dot_attention_backward_kv
        grad_q = grad_k = grad_v = None
        if any(ctx.needs_input_grad[:3]):
            grad_out = grad_out.contiguous()
            delta, grad_q = q_op(rowptr, colind, q, k, v, stats, out, grad_out, scale=ctx.scale, dropout=drop)
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                grad_k, grad_v = kv_op(colptr, rowind, q, k, v, stats, delta, grad_out, scale=ctx.scale, dropout=drop)
        return grad_q, grad_k, grad_v, None, None, None, None, None, None, None


class TransformerConv(torch.nn.Module):
    """The graph transformer layer of Shi et al. ("Masked label prediction: unified message passing model for semi-supervised
    classification"; PyG's ``TransformerConv`` without edge features) on the library's ops, H heads in every call:

        q = lin_query(x).view(n, H, F),  k = lin_key(x).view(n, H, F),  v = lin_value(x).view(n, H, F)              (dense, torch)
        alpha[e, h] = softmax over each row's entries of <q[row(e), h, :], k[col(e), h, :]> / sqrt(F)
        out[r, h, :] = sum_e alpha[e, h] v[col(e), h, :]

    then heads concatenated (``concat=True``: [n, H F]) or averaged ([n, F]); with ``root_weight`` the skip term ``x_r = lin_skip(x)`` is
    added — or, with ``beta``, gated: ``b = sigmoid(lin_beta([out, x_r, out - x_r]))``, ``out = b x_r + (1 - b) out``.

        TransformerConv(in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, bias=True, root_weight=True, fused=False,
                        attn_seed=None, fused_x16=False)
        forward(x, rowptr, colind, colptr, rowind, csc_order)

    ``fused=False`` (the default) composes the attention from ``MultiHeadSDDMMFunction``, the scaling, ``EdgeSoftmaxFunction`` (no slope),
    ``EdgeDropoutFunction`` and ``MultiHeadSPMMFunction``: [nnz, H] score and alpha arrays in both directions, any F. ``fused=True`` runs
    ``DotAttentionFunction``: three launches per training step, nothing of size nnz allocated; it serves ``out_channels <= 512`` and raises
    at construction beyond. ``dropout=p`` (0 <= p < 1) is dropout on alpha in training mode with the mask of ``EdgeDropoutFunction``: the
    two seed words come from torch's device generator at every forward unless ``attn_seed``, an int32[2] device tensor, is given; both
    settings of ``fused`` apply the same mask under one seed. In ``eval()`` mode or with ``dropout == 0`` no mask exists. ``bias``
    switches the bias of the four linear maps, as in PyG. ``beta`` needs ``root_weight``.

    The graph is square (row r and column r are the same node); ``colptr, rowind, csc_order = graphs.transpose_csr(rowptr, colind, K,
    return_order=True)`` (``csc_order`` int32; the fused path does not read it).

    16-bit ``x`` (a ``.half()`` / ``.bfloat16()`` layer, or ``torch.autocast``) with ``fused=False``: q, k and v stay 16-bit, the score
    (``MultiHeadSDDMMFunction`` on ``sddmm.csr_sddmm_heads_x16``), the scaling, softmax and dropout are fp32, the aggregation is the 16-bit
    product. ``fused=True`` alone refuses 16-bit features with a TypeError.

    ``fused=True, fused_x16=True``: 16-bit features run ``DotAttentionFunction`` on the 16-bit q, k and v (``attention.dot_attention_x16``
    and its two backward passes: fp32 sums, one rounding per 16-bit result, nothing of size ``[nnz, H]``); fp32 features run exactly what
    ``fused=True`` runs. The keyword exists because the refusal of ``fused=True`` on 16-bit features is pinned by a committed test; it
    is to be folded into ``fused=True`` when that test may change. ``fused_x16=True`` without ``fused=True`` is a ValueError."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, bias=True, root_weight=True, fused=False,
                 attn_seed=None, fused_x16=False):
        super().__init__()
        if fused_x16 and not fused:
            raise ValueError("fused_x16=True selects the 16-bit form of the fused attention: it needs fused=True")
        self.fused_x16 = bool(fused_x16)
        self.dropout = float(dropout)
        if not (0.0 <= self.dropout < 1.0):
            raise ValueError("dropout must be in [0, 1), got %r" % (dropout,))
        if heads < 1:
            raise ValueError("heads must be at least 1")
        if in_channels < 1 or out_channels < 1:
            raise ValueError("in_channels and out_channels must be at least 1")
        if beta and not root_weight:
            raise ValueError("beta gates the skip term: it needs root_weight=True")
        if fused and out_channels > _attention.DOT_ATTENTION_MAX_F:
            raise ValueError("fused=True serves out_channels <= %d (a head slice is held in registers), got %d" %
                             (_attention.DOT_ATTENTION_MAX_F, out_channels))
        if attn_seed is not None and (not isinstance(attn_seed, torch.Tensor) or attn_seed.dtype != torch.int32 or
                                      tuple(attn_seed.shape) != (2,)):
            raise TypeError("attn_seed must be an int32[2] tensor")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, int(heads)
        self.concat, self.beta, self.root_weight, self.fused = bool(concat), bool(beta), bool(root_weight), bool(fused)
        self.attn_seed = attn_seed
        hf = self.heads * out_channels
        self.lin_key = torch.nn.Linear(in_channels, hf, bias=bias)
        self.lin_query = torch.nn.Linear(in_channels, hf, bias=bias)
        self.lin_value = torch.nn.Linear(in_channels, hf, bias=bias)
        width = hf if self.concat else out_channels
        self.lin_skip = torch.nn.Linear(in_channels, width, bias=bias) if self.root_weight else None
        self.lin_beta = torch.nn.Linear(3 * width, 1, bias=False) if self.beta else None

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):
            if lin is not None:
                lin.reset_parameters()

    def forward(self, x, rowptr, colind, colptr, rowind, csc_order=None):
        n, H, F = x.shape[0], self.heads, self.out_channels
        if rowptr.numel() != n + 1 or colptr.numel() != n + 1:
            raise ValueError("TransformerConv needs a square graph: rowptr and colptr must have x.size(0) + 1 entries")
        p, seed = 0.0, None
        if self.training and self.dropout > 0.0:
            p = self.dropout
            seed = self.attn_seed
            if seed is None:  # two 32-bit words from the device generator: no host synchronisation
                seed = torch.randint(-(2 ** 31), 2 ** 31, (2,), dtype=torch.int32, device=x.device)
        q = self.lin_query(x).view(n, H, F)
        k = self.lin_key(x).view(n, H, F)
        v = self.lin_value(x).view(n, H, F)
        scale = 1.0 / math.sqrt(F)
        if self.fused and not self.fused_x16 and (_is_x16(q) or _is_x16(k) or _is_x16(v)):
            raise TypeError("TransformerConv(fused=True) needs torch.float32 features, got %s: attention.dot_attention "
                            "(DotAttentionFunction) is fp32 only; fused=False serves fp16 / bf16" % q.dtype)
        if self.fused:
            out = DotAttentionFunction.apply(q, k, v, rowptr, colind, colptr, rowind, scale, p, seed)
        else:
            if csc_order is None:
                raise ValueError("fused=False needs csc_order (graphs.transpose_csr(..., return_order=True))")
            score = MultiHeadSDDMMFunction.apply(rowptr, colind, colptr, rowind, csc_order, q, k) * scale
            alpha = EdgeSoftmaxFunction.apply(rowptr, score, None)
            if seed is not None:
                alpha = EdgeDropoutFunction.apply(rowptr, colind, alpha, p, seed)
            out = MultiHeadSPMMFunction.apply(rowptr, colind, colptr, rowind, csc_order, v, alpha, None, True)
        out = out.reshape(n, H * F) if self.concat else out.mean(dim=1)
        if self.root_weight:
            x_r = self.lin_skip(x)
            if self.beta:
                b = torch.sigmoid(self.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)))
                out = b * x_r + (1.0 - b) * out
            else:
                out = out + x_r
        return out

    def __repr__(self):
        return "%s(%d, %d, heads=%d)" % (type(self).__name__, self.in_channels, self.out_channels, self.heads)


class SpmmMaxFunction(torch.autograd.Function):
    """out[r, :] = max over the entries of row r of feat[col, :], with a gradient (``spmm.csr_spmm_max_arg`` / ``csr_spmm_max_backward``).

        SpmmMaxFunction.apply(rowptr, colind, colptr, rowind, csc_order, feat, empty_value=-10000.0)

    The forward saves ``arg`` (int32 [M, N]: the CSR position that won each output word, -1 where none did) and nothing else — not
    ``feat``. The backward gives each word of ``grad_out`` to the ONE entry ``arg`` names: grad_feat[k, c] is the sum, in CSC order,
    of grad_out[r, c] over the rows that chose an entry of node k; words nobody chose (and rows that kept ``empty_value``) pass
    nothing on. Among equal values the first entry of the row gets the gradient. ``csc_order`` (int32) maps a CSC position to its CSR
    position, as in the GAT functions. Index tensors get no gradient; once differentiable.

    ``feat`` of ``torch.float16`` / ``torch.bfloat16`` runs on the 16-bit kernels (``spmm.csr_spmm_max_arg_x16`` /
    ``csr_spmm_max_backward_x16``): ``out`` has the dtype of ``feat`` and is the exact maximum (a max rounds nothing), the saved ``arg``
    is still the only saved array, ``grad_out`` arrives in the forward's dtype and each word of ``grad_feat`` is one fp32 add chain
    rounded once."""

    @staticmethod
    def forward(ctx, rowptr, colind, colptr, rowind, csc_order, feat, empty_value=-10000.0):
        ctx.x16 = feat.dtype in (torch.float16, torch.bfloat16)
        if ctx.x16:
            out, arg = _spmm.csr_spmm_max_arg_x16(rowptr, colind, feat.contiguous(), empty_value=empty_value)
        else:
            out, arg = _spmm.csr_spmm_max_arg(rowptr, colind, feat.contiguous(), empty_value=empty_value)
        ctx.save_for_backward(colptr, rowind, csc_order, arg)
        ctx.K = feat.shape[0]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        colptr, rowind, csc_order, arg = ctx.saved_tensors
        grad_feat = None
        if ctx.needs_input_grad[5]:
            backward = _spmm.csr_spmm_max_backward_x16 if ctx.x16 else _spmm.csr_spmm_max_backward
            grad_feat = backward(colptr, rowind, csc_order, arg, grad_out.contiguous(), ctx.K)
        return None, None, None, None, None, grad_feat, None


class SAGEConv(torch.nn.Module):
    """GraphSAGE layer (Hamilton et al., 2017) with the constructor and semantics of DGL's ``SAGEConv``, on the library's ops:

        mean   fc_self(h) + fc_neigh(D^-1 A h)                    the fused product with row_scale = 1 / deg (``FusedGCNFunction``)
        gcn    fc_neigh((A h + h) / (deg + 1))                    ``SPMMFunction``
        pool   fc_self(h) + fc_neigh(max_nbr relu(fc_pool(h)))    ``SpmmMaxFunction`` with empty_value = 0: after the relu, 0 never
                                                                  changes a non-empty row, and a row without neighbours gets DGL's 0

    with h = feat_drop(x), deg the row's entry count (rows without entries aggregate 0), then ``activation``, then ``norm``.
    ``forward(x, rowptr, colind, colptr, rowind, csc_order)`` takes the square pattern in both orders; ``csc_order`` (int32: CSC
    position -> CSR position, ``graphs.transpose_csr(..., return_order=True)``) is read by ``pool`` alone and may be None otherwise.
    ``lstm`` is not served (ValueError).

    16-bit features: the layer runs as ``.half()`` / ``.bfloat16()`` and under ``torch.autocast``; the dtype of the tensor that reaches
    the aggregation decides the path, and fp32 tensors take exactly the steps above. On fp16 / bf16:

        pool   ``SpmmMaxFunction`` on the 16-bit relu(fc_pool(h)): the exact maximum, int32 ``arg`` the only saved array
        gcn    the 16-bit ``SPMMFunction`` sum (fp32 chain, one rounding), ``+ h``, times 1 / (deg + 1) cast to the dtype
        mean   the VALUED 16-bit product with fp32 edge weights 1 / deg(row): one fp32 fma chain per word and ONE rounding (a 16-bit
               sum scaled afterwards would round twice and can overflow fp16 on hub rows). The weights are two fp32 [nnz] arrays,
               in CSR and in CSC order, made per forward by torch without a host synchronisation."""

    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0.0, bias=True, norm=None, activation=None):
        super().__init__()
        if aggregator_type not in ("mean", "gcn", "pool"):
            raise ValueError("aggregator_type must be 'mean', 'gcn' or 'pool', got %r%s"
                             % (aggregator_type, " (the lstm aggregator is not served)" if aggregator_type == "lstm" else ""))
        self.in_feats, self.out_feats, self.aggregator_type = in_feats, out_feats, aggregator_type
        self.norm, self.activation = norm, activation
        self.feat_drop = torch.nn.Dropout(feat_drop)
        if aggregator_type == "pool":
            self.fc_pool = torch.nn.Linear(in_feats, in_feats)
        if aggregator_type != "gcn":
            self.fc_self = torch.nn.Linear(in_feats, out_feats, bias=bias)
        self.fc_neigh = torch.nn.Linear(in_feats, out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        gain = torch.nn.init.calculate_gain("relu")
        for name in ("fc_pool", "fc_self", "fc_neigh"):
            fc = getattr(self, name, None)
            if fc is not None:
                torch.nn.init.xavier_uniform_(fc.weight, gain=gain)

    def forward(self, x, rowptr, colind, colptr, rowind, csc_order=None):
        n = rowptr.numel() - 1
        if x.dim() != 2 or x.shape[0] != n or colptr.numel() - 1 != n:
            raise ValueError("SAGEConv needs a square pattern and x of [%d, in_feats]" % n)
        h = self.feat_drop(x)
        degree = torch.diff(rowptr).to(torch.float32)
        x16 = h.dtype in (torch.float16, torch.bfloat16)
        if self.aggregator_type == "mean":
            inv_deg = torch.where(degree > 0, 1 / degree, torch.zeros_like(degree))
            if x16:
                w_csr = torch.repeat_interleave(inv_deg, torch.diff(rowptr), output_size=colind.numel())
                w_csc = inv_deg.index_select(0, rowind)
                h_neigh = SPMMFunction.apply(rowptr, colind, colptr, rowind, h.contiguous(), w_csr, w_csc)
            else:
                h_neigh = FusedGCNFunction.apply(rowptr, colind, colptr, rowind, h, None, inv_deg, None)
            out = self.fc_self(h) + self.fc_neigh(h_neigh)
        elif self.aggregator_type == "gcn":
            h_sum = SPMMFunction.apply(rowptr, colind, colptr, rowind, h.contiguous())
            if x16:
                out = self.fc_neigh((h_sum + h) * (1 / (degree + 1)).to(h.dtype).unsqueeze(1))
            else:
                out = self.fc_neigh((h_sum + h) / (degree + 1).unsqueeze(1))
        else:
            if csc_order is None:
                raise ValueError("the pool aggregator needs csc_order (graphs.transpose_csr(..., return_order=True), int32)")
            m = torch.relu(self.fc_pool(h))
            h_neigh = SpmmMaxFunction.apply(rowptr, colind, colptr, rowind, csc_order, m, 0.0)
            out = self.fc_self(h) + self.fc_neigh(h_neigh)
        if self.activation is not None:
            out = self.activation(out)
        if self.norm is not None:
            out = self.norm(out)
        return out

    def __repr__(self):
        return "%s(%d, %d, %s)" % (type(self).__name__, self.in_feats, self.out_feats, self.aggregator_type)
