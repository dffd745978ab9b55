"""The float64 references of the attention ops and the rules they are compared by, in one plain module (numpy only, like max_arg_ref.py):
what the GPU tests of each op and the seeded sweep of tests/test_gpu_attention_fuzz.py share.

Moved here from the GPU test files, arguments now host arrays instead of the files' device dictionaries, every expression unchanged:
``gat_aggregate_float64`` (test_gpu_gat_aggregate.py), ``gat_backward_float64`` (test_gpu_gat_backward.py and, with the dropout mask,
test_gpu_edge_dropout.py: the two were one function but for ``keep``), ``gatv2_float64`` (test_gpu_gatv2_score.py), and the rule those
files wrote inline, ``bound_ratio``: |got - ref| <= 1e-4 max(|ref|, sum |terms|). Re-exported from the host test modules that own
them: the derived tolerances of the edge softmax, of the dot-product attention and of the fused GATv2 attention (its ``check_all``,
restatement and geometry), the GATv2 restatement, the max-arg chains, and the rounding, the restated geometry and the restatement of the
two 16-bit attention families. The one rounding of a 16-bit store (``U16``, ``TINY16``, ``tol16``) moved here from
test_gpu_dot_attention_x16.py; ``dot_x16_check_all`` and ``gatv2_attention_x16_check_all`` are the fp32 ``check_all`` with ``tol16``
around the tolerance of each 16-bit result, as that file's float64 test wrote it inline."""
import numpy as np
import torch

from max_arg_ref import max_arg_forward, max_backward, tied_words  # noqa: F401
from max_arg_ref import transpose as max_arg_transpose  # noqa: F401
from test_dot_attention_host import check_all as dot_check_all  # noqa: F401
from test_dot_attention_host import ratio as dot_ratio
from test_dot_attention_host import ref_backward as dot_ref_backward
from test_dot_attention_host import ref_forward as dot_ref_forward
from test_dot_attention_x16_host import geometry_x16 as dot_x16_geometry  # noqa: F401
from test_dot_attention_x16_host import restate_x16 as dot_x16_restate  # noqa: F401
from test_dot_attention_x16_host import rounded  # noqa: F401
from test_edge_dropout_host import restate as dropout_bits  # noqa: F401
from test_edge_softmax_host import ref_backward as softmax_ref_backward  # noqa: F401
from test_edge_softmax_host import ref_forward as softmax_ref_forward  # noqa: F401
from test_edge_softmax_host import worst_ratio as softmax_worst_ratio  # noqa: F401
from test_gatv2_attention_host import check_all as gatv2_attention_check_all  # noqa: F401
from test_gatv2_attention_host import geometry as gatv2_attention_geometry  # noqa: F401
from test_gatv2_attention_host import ref_backward as gatv2_attention_ref_backward
from test_gatv2_attention_host import ref_forward as gatv2_attention_ref_forward
from test_gatv2_attention_host import restate_all as gatv2_attention_restate_all  # noqa: F401
from test_gatv2_attention_x16_host import geometry_x16 as gatv2_attention_x16_geometry  # noqa: F401
from test_gatv2_attention_x16_host import restate_x16 as gatv2_attention_x16_restate  # noqa: F401
from test_gatv2_host import restate_backward as gatv2_restate_backward
from test_gatv2_host import restate_score as gatv2_restate_score
from test_gatv2_host import worst_ratio as gatv2_worst_ratio  # noqa: F401


U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}  # the one rounding at a 16-bit store
TINY16 = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}     # half the smallest fp16 subnormal; bf16 has fp32's exponents


def tol16(ref, tol, dtype):
    """The tolerance of a result stored in a 16-bit type: the fp32 result's own ``tol`` plus the one rounding at the store."""
    return tol + U16[dtype] * np.abs(ref) + TINY16[dtype]


def dot_x16_check_all(P, x, got, dtype, keep=None, ks=None, what=""):
    """test_dot_attention_host.check_all for the results of the 16-bit launches (fp32 host arrays; x: the widened operands): stats and
    delta inside the derived tolerances, out, grad_q, grad_k and grad_v inside ``tol16`` of theirs -> the worst ratio per result."""
    f = dot_ref_forward(P, x, keep, ks)
    b = dot_ref_backward(P, x, got["stats"], got["out"], None, keep, ks)
    bc = dot_ref_backward(P, x, got["stats"], got["out"], got["delta"], keep, ks)
    r = {"out": dot_ratio(got["out"], f["out"], tol16(f["out"], f["tol_out"], dtype)), "m": dot_ratio(got["stats"][..., 0], f["m"], f["tol_m"]),
         "l": dot_ratio(got["stats"][..., 1], f["l"], f["tol_l"]), "delta": dot_ratio(got["delta"], b["delta"], b["tol_delta"]),
         "grad_q": dot_ratio(got["grad_q"], b["grad_q"], tol16(b["grad_q"], b["tol_grad_q"], dtype)),
         "grad_k": dot_ratio(got["grad_k"], bc["grad_k"], tol16(bc["grad_k"], bc["tol_grad_k"], dtype)),
         "grad_v": dot_ratio(got["grad_v"], bc["grad_v"], tol16(bc["grad_v"], bc["tol_grad_v"], dtype))}
    print("%s worst error / tolerance: %s" % (what, "  ".join("%s %.3g" % kv for kv in r.items())))
    return r


def gatv2_attention_x16_check_all(P, x, slope, got, dtype, keep=None, ks=None, what=""):
    """test_gatv2_attention_host.check_all for the results of the 16-bit launches (fp32 host arrays; x: the widened operands): stats,
    delta and att_part inside the derived tolerances, out, grad_xl and grad_xr inside ``tol16`` of theirs -> the worst ratio per result."""
    f = gatv2_attention_ref_forward(P, x, slope, keep, ks)
    b = gatv2_attention_ref_backward(P, x, slope, got["stats"], got["out"], None, keep, ks)
    bc = gatv2_attention_ref_backward(P, x, slope, got["stats"], got["out"], got["delta"], keep, ks)
    r = {"out": dot_ratio(got["out"], f["out"], tol16(f["out"], f["tol_out"], dtype)), "m": dot_ratio(got["stats"][..., 0], f["m"], f["tol_m"]),
         "l": dot_ratio(got["stats"][..., 1], f["l"], f["tol_l"]), "delta": dot_ratio(got["delta"], b["delta"], b["tol_delta"]),
         "grad_xl": dot_ratio(got["grad_xl"], b["grad_xl"], tol16(b["grad_xl"], b["tol_grad_xl"], dtype)),
         "att_part": dot_ratio(got["att_part"], b["att_part"], b["tol_att_part"]),
         "grad_xr": dot_ratio(got["grad_xr"], bc["grad_xr"], tol16(bc["grad_xr"], bc["tol_grad_xr"], dtype))}
    print("%s worst error / tolerance: %s" % (what, "  ".join("%s %.3g" % kv for kv in r.items())))
    return r


def rows_of(rowptr):
    """The row of every entry, int32[nnz]."""
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(rowptr))


def bound_ratio(got, ref, scale):
    """The project's rule |got - ref| <= 1e-4 max(|ref|, scale), scale the sum of the magnitudes of the terms -> (worst error /
    bound, every word inside). Where the bound is zero the error itself is the ratio: only an exact result passes there. A NaN in
    ``got`` is outside."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    bound = 1e-4 * np.maximum(np.abs(ref), scale)
    err = np.abs(got - ref)
    if err.size == 0:
        return 0.0, True
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    return worst, bool(np.all(err <= bound))


def gat_weights_float64(rows, cols, M, el, er, slope):
    """Softmax over every row of leaky(fl(el[row] + er[col])) in float64 -> (w f64[nnz, H], the fp32 score as float64). The score is
    the contract's rounded sum fl(el + er)."""
    s = (el[rows] + er[cols]).astype(np.float64)
    x = s if slope is None else np.where(s >= 0, s, s * float(np.float32(slope)))
    H = x.shape[1]
    top = np.full((M, H), -np.inf)
    np.maximum.at(top, rows, x)
    t = np.exp(x - top[rows])
    den = np.zeros((M, H))
    np.add.at(den, rows, t)
    return t / den[rows], s


def gat_aggregate_float64(rows, cols, M, K, el, er, dense, slope, transposed, keep=None, s=None):
    """Softmax, then product, in float64 on the host -> (ref, sum |w b|). ``keep`` (bool[nnz, H]) and ``s``: the dropout mask and the
    kept entries' scale, w' = keep ? w s : 0."""
    w, _ = gat_weights_float64(rows, cols, M, el, er, slope)
    if keep is not None:
        w = w * np.where(keep, float(s), 0.0)
    src, dst, n = (rows, cols, K) if transposed else (cols, rows, M)
    terms = w[:, :, None] * dense.astype(np.float64)[src]
    ref, mag = np.zeros((n,) + dense.shape[1:]), np.zeros((n,) + dense.shape[1:])
    np.add.at(ref, dst, terms)
    np.add.at(mag, dst, np.abs(terms))
    return ref, mag


def gat_backward_float64(rows, cols, M, K, el, er, gout, feat, slope, keep=None, s=None):
    """Softmax, dot, backward and both sums in float64 on the host -> (grad_el, grad_er, scale_el, scale_er) with
    scale = sum_p w_p (G_p + sum_q w_q G_q), G_p = sum_f |grad_out feat|; with a dropout mask g' = keep ? g s : 0."""
    w, sc = gat_weights_float64(rows, cols, M, el, er, slope)
    k = 1.0 if slope is None else float(np.float32(slope))
    H = w.shape[1]
    terms = gout.astype(np.float64)[rows] * feat.astype(np.float64)[cols]
    g, gabs = terms.sum(-1), np.abs(terms).sum(-1)
    if keep is not None:
        d = np.where(keep, float(s), 0.0)
        g, gabs = g * d, gabs * d
    dot, dabs = np.zeros((M, H)), np.zeros((M, H))
    np.add.at(dot, rows, w * g)
    np.add.at(dabs, rows, w * gabs)
    gs = w * (g - dot[rows]) * np.where(sc >= 0, 1.0, k)
    mag = w * (gabs + dabs[rows])
    gel, ger, sel, ser = np.zeros((M, H)), np.zeros((K, H)), np.zeros((M, H)), np.zeros((K, H))
    np.add.at(gel, rows, gs)
    np.add.at(sel, rows, mag)
    np.add.at(ger, cols, gs)
    np.add.at(ser, cols, mag)
    return gel, ger, sel, ser


def gatv2_float64(G, o, slope):
    """float64: (score, terms), the row pass (grad_xl, att_part, terms, terms) and the column pass (grad_xr, _, terms, _) of the host
    pattern G (rowptr, colind, colptr_h, rowind_h, order_h) and the host operands o (xl, xr, att, gs)."""
    return (gatv2_restate_score(G["rowptr"], G["colind"], o["xl"], o["xr"], o["att"], slope),
            gatv2_restate_backward(G["rowptr"], G["colind"], o["gs"], o["xl"], o["xr"], o["att"], slope),
            gatv2_restate_backward(G["colptr_h"], G["rowind_h"], o["gs"], o["xr"], o["xl"], o["att"], slope, order=G["order_h"]))


def sddmm_float64(rows, cols, D1, D2):
    """out[e, h] = <D1[row(e), h, :], D2[col(e), h, :]> in float64 -> (ref, sum |d1 d2|) (test_gpu_sddmm_heads.py's rule, on the host)."""
    p = D1.astype(np.float64)[rows] * D2.astype(np.float64)[cols]
    return p.sum(-1), np.abs(p).sum(-1)


def heads_float64(rows, cols, M, val, B):
    """C[r, h, :] = sum_p val[p, h] B[col(p), h, :] in float64 -> (ref, sum |w b|)."""
    terms = val.astype(np.float64)[:, :, None] * B.astype(np.float64)[cols]
    ref, mag = np.zeros((M,) + B.shape[1:]), np.zeros((M,) + B.shape[1:])
    np.add.at(ref, rows, terms)
    np.add.at(mag, rows, np.abs(terms))
    return ref, mag
