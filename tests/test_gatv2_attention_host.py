"""The fused GATv2 attention (gespmm_gatv2_attention_f32 and its two backward passes) without a GPU: exports, the order of the argument
checks, the describe table, the Python wrappers' errors, the layer's argument errors — and an fp32 RESTATEMENT of the three kernels'
chains in numpy, held against float64 within a derived tolerance. The GPU tests import the inputs, the restatement, the float64
references and the tolerances from here, unchanged. The pieces of the restatement (fma32, expf, lane_dot, steps, seg_sum, ratio,
pattern, keep_mask) are test_dot_attention_host's, the float64 score and its sum of magnitudes test_gatv2_host's restate_score.

The float64 references start from the contract's ROUNDED t = fl32(xl + xr): the one fp32 add is part of what is computed, not an error
(against restate_score, which adds in float64, the reference's score moves by at most u sum_f |att_f leaky(t_f)|: asserted here).

The tolerances (u = 2^-23; every fp32 operation is taken to err by at most u relative, a generous unit; d entries in the segment)
-------------------------------------------------------------------------------------------------------------------------------
This is test_dot_attention_host's derivation with v = k = xr and the score's term replaced.
score: one add, one optional multiply (the leaky slope), a chain of F fmaf and the butterfly, on T_p = sum_f |att_f leaky(t_pf)|:
    |s_p - s64_p| <= es_p = u (F + 3) T_p
forward: with z_p = s_p - m, zbar = sum_p a_p |z_p|:
    tol(out_f) = sum_p [a_p (es_p + sum_j a_j es_j) + a_p u (2 |z_p| + 2 zbar + 2 d + 8)] |xr_pf| + u (d + 2) sum_p a_p |xr_pf| + 2^-120
  (the score's error moves a_p directly and through the normaliser; exp2 of fl(z log2 e) errs by about 2 |z| u relative, once in t, once
  — averaged — in l; each of the at most d rescales of acc and l costs one rounding each (2 d), the division, the product t xr and the
  first step a handful more (8); the fmaf chain of acc itself is u (d + 2) of the sum of magnitudes. With dropout |xr| is |xr| keep s
  and one more rounding fl(t s) joins the 8.)
stats: tol(m) = max_p es_p;  tol(l) = sum_p e^{z_p} (es_p + max_j es_j + u (2 |z_p| + d + 4)).
backward, both passes — the float64 reference reads the DEVICE's (restatement's) own stats, out and delta:
    tol(delta) = u (F + 2) sum_f |go_f out_f|                                             (the dot)
    ea_p = es_p + u (2 |z_p| + 4)                                                         (relative error of a_p = exp(s_p - m) / l)
    eg_p = u (F + 3) sum_f |go_f xr_pf| keep s                                            (the dot; + 1: the dropout's rounding)
    eds_p = a_p (ea_p + 3 u) (|g_p| + |delta|) + a_p (eg_p + tol(delta))                  (ds_p = a_p (g_p - delta))
  m_pf = t_pf >= 0 ? att_f : fl(att_f slope) is the contract's own fp32 number (no error); leaky(t_pf) carries the multiply's u:
    tol(grad_xl_f)  = sum_p eds_p |m_pf| + u (d + 2) sum_p |ds_p m_pf| + 2^-120           (one fmaf chain of d steps)
    tol(att_part_f) = sum_p eds_p |leaky(t_pf)| + u (d + 3) sum_p |ds_p leaky(t_pf)| + 2^-120
  grad_xr carries TWO chains and ONE add (c1 = sum_p ds_p m_pf, c2 = sum_p a_p keep s go_pf over the column's d entries):
    tol(grad_xr_f)  = sum_p eds_p |m_pf| + u (d + 2) sum_p |ds_p m_pf|
                    + sum_p a_p keep s (ea_p + 2 u) |go_pf| + u (d + 2) sum_p a_p keep s |go_pf|
                    + u (sum_p |ds_p m_pf| + sum_p a_p keep s |go_pf|) + 2^-120           (the last line: the add at the store)
With negative_slope=None every m_pf is att_f, so grad_xl = att_f sum_p a_p (g_p - delta) is zero but for rounding (the softmax does not
see a shift of all its scores): its reference is of the tolerance's own size and no entry can show in it; the witness test asks for
grad_xl at slope 0.2 only.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_dot_attention_host import expf, fma32, keep_mask, lane_dot, pattern, ratio, seg_sum, steps
from test_gatv2_host import restate_score
from test_heads_host import EALIGN, EINVAL, ERANGE

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
FLOOR = 2.0 ** -120
UNSUPPORTED = -7
NEW = ("gespmm_gatv2_attention_f32", "gespmm_gatv2_attention_dropout_f32", "gespmm_gatv2_attention_backward_row_f32",
       "gespmm_gatv2_attention_backward_row_dropout_f32", "gespmm_gatv2_attention_backward_col_f32",
       "gespmm_gatv2_attention_backward_col_dropout_f32", "gespmm_describe_gatv2_attention")
OK = 0x1000  # a made-up address: the checks look at the number only and return before anything could read it
BIG = (1 << 31) - 4096  # one past the largest count of 32-bit word positions
FS = (1, 3, 8, 20, 32, 64, 100, 512)
HS = (1, 3, 4)
SLOPES = (0.2, None)
# (pattern, H, F) -> which draw of the inputs is used (0 where absent; a tuple: one single-head draw per head): see inputs(). Filled by
# the search at the end of this module (python tests/test_gatv2_attention_host.py), which looks for the first draw at which
# test_witness_every_entry_shows holds. F = 1 on "hand": 340, 424, 780 and 1336 are the first four single-head draws that pass.
SEEDS = {("hand", 1, 1): 340, ("hand", 3, 1): (340, 424, 780), ("hand", 4, 1): (340, 424, 780, 1336), ("hand", 3, 3): 3, ("hand", 4, 3): 13}


# ------------------------------------------------------------------------------------------------------------- inputs

@functools.lru_cache(maxsize=None)
def inputs(name, H, F):
    """The inputs of a case: draw SEEDS[(name, H, F)] of ``draw_inputs`` (0 where absent); where SEEDS holds a tuple, head h is the one
    head of draw number SEEDS[..][h] at H = 1 — the heads do not meet anywhere in the op, and at F = 1 on the "hand" pattern a draw in
    a few hundred passes the witness test for one head, which no draw of three or four heads at once did in 3000."""
    draw = SEEDS.get((name, H, F), 0)
    if isinstance(draw, tuple):
        assert len(draw) == H
        heads = [draw_inputs(name, 1, F, d) for d in draw]
        return {k: np.concatenate([x[k] for x in heads], axis=0 if k == "att" else 1) for k in heads[0]}
    return draw_inputs(name, H, F, draw)


def draw_inputs(name, H, F, number):
    """xl, xr, att, grad_out for a pattern of test_dot_attention_host, shaped so that EVERY entry shows in every result it feeds (the
    witness test):
      * magnitudes in [0.5, 1) before the scalings: no t = fl(xl + xr) is exactly 0 (asserted);
      * att with a random sign per word and an amplitude that narrows the scores at large F, where the bound on the score's error is
        large against the 1 / d share of an entry; xl with a random sign per word on rows of fewer than two entries, and placed between
        the xr words of two of the row's entries elsewhere (below);
      * xr — the score's operand AND the aggregated value — with ONE sign and ONE amplitude per (column, head): the K amplitudes of
        a head are the K steps of [0.5, 1.5) in a random order, all different; grad_out positive, so that g_p = <grad_out, xr_p> is a
        coherent sum and the g_p of a row differ from each other and from delta.
    SEEDS names, per case, the first draw at which the witness test's condition holds — a condition on the inputs, found and checked
    on the CPU."""
    P = pattern(name)
    rng = np.random.RandomState(2000 * H + F + (0 if name == "hand" else 500000) + 7919 * number)

    def draw(shape, signs=True):
        x = rng.uniform(0.5, 1.0, size=shape)
        return (x * rng.choice((-1.0, 1.0), size=shape) if signs else x).astype(F32)

    xl, go = draw((P["M"], H, F)), draw((P["M"], H, F), signs=False)
    amp = np.stack([(0.5 + rng.permutation(P["K"]) / P["K"]) * rng.choice((-1.0, 1.0), size=P["K"]) for _ in range(H)], 1)
    xr = (draw((P["K"], H, F), signs=False) * amp[:, :, None]).astype(F32)
    # the classes of test_dot_attention_host's "hand" pattern: short rows draw their columns from [0, 12), rows of 63 .. 65 entries from
    # [12, 30), hub rows from [30, 53) — so the spread of a row's scores, which only xr can move, is set through its columns' scale
    row_scale = np.where(P["degs"] <= 9, 1.0, np.where(P["degs"] <= 65, 0.4, 0.25))
    cols = np.arange(P["K"])
    col_scale = np.where(cols < 12, 1.0, np.where(cols < 30, 0.4, 0.25)) if name == "hand" else np.ones(P["K"])
    xl = (xl * (0.75 * row_scale)[:, None, None]).astype(F32)
    xr = (xr * col_scale[:, None, None]).astype(F32)
    att = (draw((H, F)) * F32(min(2.5 / np.sqrt(F), 16.0 / F))).astype(F32)
    # grad_xl sees an entry only through the SIGNS of its t: where all entries of a row agree in them, the row's grad_xl is zero but for
    # rounding (the module docstring's last paragraph). So word f of a row with d >= 2 entries is put halfway between the xr words of
    # its entries f mod d and the next one on another column: those two get t of opposite signs there, (xr_p - xr_q) / 2 and its negative.
    # At F = 1 that one word decides alone, and it also has to keep every |t| of the row away from zero (att_part's word is a sum of
    # ds_p leaky(t_p)): there it sits in the middle of the widest gap between the row's xr values.
    for r in np.nonzero(P["degs"] >= 2)[0]:
        c = P["colind"][P["rowptr"][r]:P["rowptr"][r + 1]]
        if F == 1 and np.unique(c).size >= 2:
            for h in range(H):
                v = np.unique(xr[c, h, 0])
                i = int(np.argmax(np.diff(v)))
                xl[r, h, 0] = -(v[i] + v[i + 1]) / F32(2)
            continue
        for f in range(F):
            p = f % c.size
            other = np.nonzero(c != c[p])[0]
            if other.size:
                q = other[np.searchsorted(other, p) % other.size]
                xl[r, :, f] = -(xr[c[p], :, f] + xr[c[q], :, f]) / F32(2)
    return {"xl": xl, "xr": xr, "att": att, "go": go}


def geometry(F, align=16):
    """(V, W) of the kernels at width F for operands on an `align`-byte boundary: the rule, restated."""
    V = 4
    while V > 1 and (F % V != 0 or align % (4 * V) != 0):
        V //= 2
    W = 4
    while W < 64 and 8 * W < F:
        W *= 2
    return V, W


# ------------------------------------------------------------------------------------------------------------------ the restatement

def leaky32(t, slope):
    """leaky(t) on fp32: t >= 0 ? t : fl(slope t); slope None (== 1): no multiply."""
    if slope is None or float(slope) == 1.0:
        return t
    return np.where(t >= 0, t, (F32(slope) * t).astype(F32))


def factor32(t, att, slope):
    """m = t >= 0 ? att : fl(att slope), broadcast to t's shape (att [H, F] against t [n, H, F])."""
    a = np.broadcast_to(att[None], t.shape)
    if slope is None or float(slope) == 1.0:
        return a
    return np.where(t >= 0, a, (att * F32(slope)).astype(F32)[None])


def lane_score(att, xa, xb, slope, V, W):
    """-> (s f32[n, H], t f32[n, H, F]): t = fl(xa + xb), s by the pinned chain fmaf(att_j, leaky(t_j), acc) and the butterfly."""
    t = (xa + xb).astype(F32)
    return lane_dot(np.broadcast_to(att[None], t.shape), leaky32(t, slope), V, W), t


def restate_forward(P, x, slope, V, W, mode="exp2", keep=None, ks=None, count_rescales=False):
    """-> (out f32[M, H, F], stats f32[M, H, 2]) by the forward kernel's chain; with count_rescales also the number of steps with m' > m."""
    xl, xr, att = x["xl"], x["xr"], x["att"]
    M, H, F = xl.shape
    s, _ = lane_score(att, xl[P["rows"]], xr[P["colind"]], slope, V, W)  # [nnz, H]
    m, l, acc = np.zeros((M, H), F32), np.zeros((M, H), F32), np.zeros((M, H, F), F32)
    rescales = np.zeros((M, H), dtype=np.int64)
    for t, (seg, e) in enumerate(steps(P["rowptr"])):
        sp = s[e]
        mo = sp if t == 0 else m[seg]
        mn = np.maximum(mo, sp)
        c, te = expf(mo - mn, mode), expf(sp - mn, mode)
        rescales[seg] += mn > mo
        l[seg] = fma32(l[seg], c, te)
        tv = te if keep is None else np.where(keep[e], (te * ks).astype(F32), F32(0))
        acc[seg] = fma32(tv[..., None], xr[P["colind"][e]], (acc[seg] * c[..., None]).astype(F32))
        m[seg] = mn
    some = (P["degs"] > 0)[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(some, (acc / l[..., None]).astype(F32), F32(0))
    stats = np.stack((m, l), -1)
    return (out, stats, rescales) if count_rescales else (out, stats)


def _entry_terms(P, x, stats, slope, V, W, mode, keep, ks, transposed):
    """rows, cols, t, a, a', g' of every entry by the kernels' expressions, in CSR order or (transposed) in CSC order."""
    rows, cols = (P["rows"], P["colind"]) if not transposed else (P["rowind"], np.repeat(np.arange(P["K"]), np.diff(P["colptr"])))
    s, t = lane_score(x["att"], x["xl"][rows], x["xr"][cols], slope, V, W)
    g = lane_dot(x["go"][rows], x["xr"][cols], V, W)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (expf(s - stats[rows, :, 0], mode) / stats[rows, :, 1]).astype(F32)
    av = a
    if keep is not None:
        g = np.where(keep, (g * ks).astype(F32), F32(0))
        av = np.where(keep, (a * ks).astype(F32), F32(0))
    return rows, cols, t, a, av, g


def restate_backward_row(P, x, stats, out, slope, V, W, mode="exp2", keep=None, ks=None):
    """-> (delta f32[M, H], grad_xl, att_part f32[M, H, F]) by the row pass's chains."""
    rows, cols, t, a, _, g = _entry_terms(P, x, stats, slope, V, W, mode, keep, ks, False)
    delta = lane_dot(x["go"], out, V, W)
    ds = (a * (g - delta[rows]).astype(F32)).astype(F32)
    mf, lk = factor32(t, x["att"], slope), leaky32(t, slope)
    gx, ga = np.zeros(x["xl"].shape, F32), np.zeros(x["xl"].shape, F32)
    for seg, e in steps(P["rowptr"]):
        gx[seg] = fma32(ds[e][..., None], mf[e], gx[seg])
        ga[seg] = fma32(ds[e][..., None], lk[e], ga[seg])
    return delta, gx, ga


def restate_backward_col(P, x, stats, delta, slope, V, W, mode="exp2", keep_t=None, ks=None):
    """-> grad_xr f32[K, H, F] by the column pass's two chains and their one add (keep_t: the mask in CSC order)."""
    rows, cols, t, a, av, g = _entry_terms(P, x, stats, slope, V, W, mode, keep_t, ks, True)
    ds = (a * (g - delta[rows]).astype(F32)).astype(F32)
    mf = factor32(t, x["att"], slope)
    c1, c2 = np.zeros(x["xr"].shape, F32), np.zeros(x["xr"].shape, F32)
    for seg, e in steps(P["colptr"]):
        c1[seg] = fma32(ds[e][..., None], mf[e], c1[seg])
        c2[seg] = fma32(av[e][..., None], x["go"][rows[e]], c2[seg])
    return (c1 + c2).astype(F32)


def restate_all(P, x, slope, V, W, mode="exp2", p=None):
    keep = keep_t = ks = None
    if p is not None:
        H = x["xl"].shape[1]
        keep, ks = keep_mask(P, H, p)
        keep_t, _ = keep_mask(P, H, p, transposed=True)
    out, stats = restate_forward(P, x, slope, V, W, mode, keep, ks)
    delta, grad_xl, att_part = restate_backward_row(P, x, stats, out, slope, V, W, mode, keep, ks)
    grad_xr = restate_backward_col(P, x, stats, delta, slope, V, W, mode, keep_t, ks)
    return {"out": out, "stats": stats, "delta": delta, "grad_xl": grad_xl, "att_part": att_part, "grad_xr": grad_xr}, keep, ks


# ------------------------------------------------------------------------------------------ float64 references and their tolerances

def _score64(P, x, slope):
    """From the contract's rounded t: (t f64, leaky f64, m f64, s f64[nnz, H], T = sum |att leaky| f64[nnz, H]) in CSR order."""
    rows, cols = P["rows"], P["colind"]
    t = (x["xl"][rows] + x["xr"][cols]).astype(F32).astype(F64)
    att = x["att"].astype(F64)[None]
    if slope is None or float(slope) == 1.0:
        lk, mf = t, np.broadcast_to(att, t.shape)
    else:
        lk = np.where(t >= 0, t, t * F64(F32(slope)))
        mf = np.where(t >= 0, att, (x["att"] * F32(slope)).astype(F32).astype(F64)[None])
    prod = att * lk
    return t, lk, mf, prod.sum(-1), np.abs(prod).sum(-1)


def ref_forward(P, x, slope, keep=None, ks=None):
    """float64 on the fp32 inputs -> dict(out, m, l, tol_out, tol_m, tol_l) and the per-entry pieces the other references reuse."""
    rows, cols, ptr = P["rows"], P["colind"], P["rowptr"]
    M, H, F = x["xl"].shape
    d = P["degs"].astype(F64)[:, None]
    _, _, _, s, T = _score64(P, x, slope)
    es = U * (F + 3) * T
    m = np.full((M, H), -np.inf)
    np.maximum.at(m, rows, s)
    m[P["degs"] == 0] = 0.0
    z = s - m[rows]
    ez = np.exp(z)
    l = seg_sum(ez, ptr)
    a = ez / np.where(l > 0, l, 1.0)[rows]
    w = a if keep is None else a * keep * F64(ks)  # the coefficient that multiplies xr
    vv = x["xr"].astype(F64)[cols]
    out = seg_sum(w[..., None] * vv, ptr)
    zbar = seg_sum(a * np.abs(z), ptr)
    esbar = seg_sum(a * es, ptr)
    per = w * (es + esbar[rows]) + w * U * (2 * np.abs(z) + 2 * zbar[rows] + 2 * d[rows] + 8 + (0 if keep is None else 1))
    tol_out = seg_sum(per[..., None] * np.abs(vv), ptr) + U * (d[..., None] + 2) * seg_sum(w[..., None] * np.abs(vv), ptr) + FLOOR
    es_max = np.zeros((M, H))
    np.maximum.at(es_max, rows, es)
    tol_l = seg_sum(ez * (es + es_max[rows] + U * (2 * np.abs(z) + d[rows] + 4)), ptr) + FLOOR
    return {"out": out, "m": m, "l": l, "tol_out": tol_out, "tol_m": es_max + FLOOR, "tol_l": tol_l, "a": a, "w": w, "s": s, "es": es}


def ref_backward(P, x, slope, stats, out, delta=None, keep=None, ks=None):
    """float64 on the fp32 inputs AND on the given (device's, restatement's) stats and out — and delta, for the column pass; without it
    the float64 delta of `out` — -> dict(delta, grad_xl, att_part, grad_xr and their tol_*, and the per-entry contributions)."""
    rows, cols, ptr = P["rows"], P["colind"], P["rowptr"]
    M, H, F = x["xl"].shape
    xr, go = x["xr"].astype(F64), x["go"].astype(F64)
    st = stats.astype(F64)
    kf = F64(1.0) if keep is None else keep * F64(ks)
    t, lk, mf, s, T = _score64(P, x, slope)
    es = U * (F + 3) * T
    z = s - st[rows, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.exp(z) / st[rows, :, 1]
    g = (go[rows] * xr[cols]).sum(-1) * kf
    eg = U * (F + 3) * (np.abs(go[rows]) * np.abs(xr[cols])).sum(-1) * kf
    delta64 = (go * out.astype(F64)).sum(-1)
    tol_delta = U * (F + 2) * (np.abs(go) * np.abs(out.astype(F64))).sum(-1) + FLOOR
    dl = delta64 if delta is None else delta.astype(F64)
    ds = a * (g - dl[rows])
    ea = es + U * (2 * np.abs(z) + 4)
    eds = a * (ea + 3 * U) * (np.abs(g) + np.abs(dl[rows])) + a * (eg + tol_delta[rows])
    dr = P["degs"].astype(F64)[:, None, None]
    dc = np.diff(P["colptr"]).astype(F64)[:, None, None]
    o = P["order"]  # CSC order: the column pass sums a column's entries
    cx = ds[..., None] * mf
    ca = ds[..., None] * lk
    c1 = cx
    c2 = (a * kf)[..., None] * go[rows]
    mag1, mag2 = seg_sum(np.abs(c1)[o], P["colptr"]), seg_sum(np.abs(c2)[o], P["colptr"])
    return {"delta": delta64, "tol_delta": tol_delta,
            "grad_xl": seg_sum(cx, ptr),
            "tol_grad_xl": seg_sum(eds[..., None] * np.abs(mf), ptr) + U * (dr + 2) * seg_sum(np.abs(cx), ptr) + FLOOR,
            "att_part": seg_sum(ca, ptr),
            "tol_att_part": seg_sum(eds[..., None] * np.abs(lk), ptr) + U * (dr + 3) * seg_sum(np.abs(ca), ptr) + FLOOR,
            "grad_xr": seg_sum((c1 + c2)[o], P["colptr"]),
            "tol_grad_xr": seg_sum((eds[..., None] * np.abs(mf))[o], P["colptr"]) + U * (dc + 2) * mag1
            + seg_sum(((a * kf * (ea + 2 * U))[..., None] * np.abs(go[rows]))[o], P["colptr"]) + U * (dc + 2) * mag2
            + U * (mag1 + mag2) + FLOOR,
            "contrib_xr": c1 + c2, "a": a, "g": g, "ds": ds, "mf": mf, "lk": lk}


def check_all(P, x, slope, got, keep=None, ks=None, what="", att_part=True):
    """The results of the three launches (a dict with out, stats, delta, grad_xl, att_part, grad_xr) against float64: -> the worst ratio
    per result, printed. The backward's reference reads got's own stats, out and delta."""
    f = ref_forward(P, x, slope, keep, ks)
    b = ref_backward(P, x, slope, got["stats"], got["out"], None, keep, ks)
    bc = ref_backward(P, x, slope, got["stats"], got["out"], got["delta"], keep, ks)
    r = {"out": ratio(got["out"], f["out"], f["tol_out"]), "m": ratio(got["stats"][..., 0], f["m"], f["tol_m"]),
         "l": ratio(got["stats"][..., 1], f["l"], f["tol_l"]), "delta": ratio(got["delta"], b["delta"], b["tol_delta"]),
         "grad_xl": ratio(got["grad_xl"], b["grad_xl"], b["tol_grad_xl"]),
         "grad_xr": ratio(got["grad_xr"], bc["grad_xr"], bc["tol_grad_xr"])}
    if att_part:
        r["att_part"] = ratio(got["att_part"], b["att_part"], b["tol_att_part"])
    print("%s worst error / tolerance: %s" % (what, "  ".join("%s %.3g" % kv for kv in r.items())))
    return r


# --------------------------------------------------------------------------------------------------------------------- tests

@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_and_version(L, pkg):
    for name in NEW:
        assert name in L.EXPORTS
        getattr(L.lib, name)
    assert L.lib.gespmm_version().decode().startswith("gespmm 0.5 ")
    for name in ("attention", "GATv2AttentionFunction", "GATv2Conv"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("gatv2_attention", "gatv2_attention_backward_row", "gatv2_attention_backward_col"):
        assert callable(getattr(pkg.attention, name))
    assert callable(L.describe_gatv2_attention) and L.GATV2_ATTENTION_MAX_F == 512


# (entry point, number of pointers, positions of the results, position of stats, position of a pointer that may be NULL)
ENTRIES = (("gespmm_gatv2_attention_f32", 7, (5, 6), 6, None), ("gespmm_gatv2_attention_backward_row_f32", 11, (8, 9, 10), 5, 10),
           ("gespmm_gatv2_attention_backward_col_f32", 9, (8,), 5, None))


@pytest.mark.parametrize("name,np_,results,stats_at,optional", ENTRIES)
@pytest.mark.parametrize("drop", (False, True))
def test_return_codes(L, name, np_, results, stats_at, optional, drop):
    """(pointers | M, K, H, F, nnz, slope[, p, seed], stream): sizes that make no sense (a bad slope and a bad p with them), sizes too
    large, the slice no kernel serves, nnz == 0 / F == 0 (the results and the seed alone), then the pointers: NULL, alignment."""
    f0 = getattr(L.lib, name.replace("_f32", "_dropout_f32") if drop else name)

    def f(ptrs, M, K, H, F, nnz, slope, p=0.25, seed=_p(OK)):
        tail = (p, seed, None) if drop else (None,)
        return f0(*ptrs, M, K, H, F, nnz, slope, *tail)

    none = (None,) * np_
    col = name.endswith("col_f32")
    assert f(none, 4, 4, 0, 8, 10, 0.2) == EINVAL        # H < 1
    assert f(none, -1, 4, 2, 8, 10, 0.2) == EINVAL       # negative sizes
    assert f(none, 4, -4, 2, 8, 0, 0.2) == EINVAL
    assert f(none, 4, 4, 2, -8, 10, 0.2) == EINVAL
    assert f(none, 4, 4, 2, 8, -1, 0.2) == EINVAL
    assert f(none, 4, 0, 2, 8, 10, 0.2) == EINVAL        # K < 1 with entries
    assert f(none, 0, 4, 2, 8, 10, 0.2) == EINVAL        # entries without rows
    assert f(none, 4, 4, 2, 8, 10, float("inf")) == EINVAL
    assert f(none, 4, 4, 2, 8, 10, float("nan")) == EINVAL
    assert f(none, 4, 4, 0, 8, BIG, 0.2) == EINVAL       # what makes no sense before what is too large
    assert f(none, 4, 4, 2, 513, 10, float("nan")) == EINVAL  # ... and before what is not served
    if drop:
        for p in (-0.1, 1.0, float("nan")):
            assert f(none, 4, 4, 2, 8, 10, 0.2, p=p) == EINVAL
            assert f(none, 4, 4, 2, 8, BIG, 0.2, p=p) == EINVAL
    assert f(none, 4, 4, 1, 8, BIG, 0.2) == ERANGE       # nnz
    assert f(none, 4, 4, 2, 8, BIG // 2 + 1, 0.2) == ERANGE    # nnz H
    assert f(none, BIG, 4, 1, 1, 10, 0.2) == ERANGE      # M
    assert f(none, BIG // 16 + 1, 4, 2, 8, 10, 0.2) == ERANGE  # M H F words
    assert f(none, 4, BIG // 16 + 1, 2, 8, 10, 0.2) == ERANGE  # K H F words
    assert f(none, BIG // 2 + 1, 4, 1, 1, 10, 0.2) == ERANGE   # the 2 M H words of stats
    assert f(none, BIG, 4, 1, 1, 0, 0.2) == ERANGE       # too large comes before "no entries"
    assert f(none, BIG // 1024 + 1, 4, 2, 513, 10, 0.2) == ERANGE  # ... and before "not served"
    assert f(none, 4, 4, 2, 513, 10, 0.2) == UNSUPPORTED
    assert f(none, 4, 4, 2, 513, 0, 0.2) == UNSUPPORTED  # before "no entries"
    assert f(tuple(_p(OK) for _ in none), 4, 4, 2, 4096, 10, 0.2) == UNSUPPORTED  # nothing is launched
    assert f(none, 4, 4, 2, 512, 10, 0.2) == EINVAL      # the widest slice served: on to the pointers
    assert f(none, 4, 4, 2, 512, 10, 1.0) == EINVAL      # slope == 1 (no multiply) is a slope like any other
    # no entries, or rows of no width: the results (and the seed) alone are looked at, and zero-filled on a device
    for F, nnz in ((8, 0), (0, 10)):
        assert f(none, 4, 4, 2, F, nnz, 0.2) == (0 if F == 0 and col else EINVAL)
        for bad in results:
            if F == 0 and (col or bad not in (stats_at, 8)):
                continue  # (results of no words: stats and delta are what is written)
            ptrs = [_p(OK + 2) if i == bad else (_p(OK) if i in results else None) for i in range(np_)]
            assert f(ptrs, 4, 4, 2, F, nnz, 0.2) == EALIGN, (F, nnz, bad)
        if drop:
            assert f(none, 4, 4, 2, F, nnz, 0.2, seed=None) == EINVAL
            assert f(none, 0, 0, 2, F, 0, 0.2, seed=_p(OK + 2)) == EALIGN
    assert f(none, 0, 0, 2, 8, 0, 0.2) == 0              # nothing to write
    # the pointers
    assert f(none, 4, 4, 2, 8, 10, 0.2) == EINVAL
    for bad in range(np_):
        if bad != optional:
            assert f([None if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EINVAL, bad
        assert f([_p(OK + 2) if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EALIGN, bad
    assert f([_p(OK + 4) if i == stats_at else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EALIGN  # stats: 8 bytes
    assert f([None if i == 0 else _p(OK + 2) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EINVAL  # NULL before alignment
    if optional is not None:  # att_part may be NULL: the other checks still run
        assert f([None if i in (optional, 0) else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EINVAL
        assert f([None if i == optional else (_p(OK + 2) if i == 2 else _p(OK)) for i in range(np_)], 4, 4, 2, 8, 10, 0.2) == EALIGN
    if drop:
        assert f([_p(OK)] * np_, 4, 4, 2, 8, 10, 0.2, seed=None) == EINVAL
        assert f([_p(OK)] * np_, 4, 4, 2, 8, 10, 0.2, seed=_p(OK + 2)) == EALIGN


@pytest.mark.parametrize("F", FS + (33, 513))
def test_describe(L, F):
    for align in (16, 8, 4):
        got = L.describe_gatv2_attention(71, 53, 3, F, 1000, align, align, align)
        if F > 512:
            assert got == {"route": "unsupported", "supported": False}
            continue
        V, W = geometry(F, align)
        assert got == {"V": V, "W": W, "supported": True}, (F, align, got)
        assert F % V == 0 and (4 * V) <= align and 8 * W >= F and (W == 4 or 4 * W < F)
        # the rule is the one the score kernel and the dot-product attention answer: the bits of s_p depend on it
        score = L.describe_gatv2_score(71, 1000, 3, F, align, align, align)
        assert (score["V"], score["W"]) == (V, W) and L.describe_dot_attention(71, 53, 3, F, 1000, align, align, align) == {"V": V, "W": W}
    # the least aligned operand decides, whichever it is; more than 16 bytes is as good as 16
    want = geometry(F, 4) if F <= 512 else None
    for al in ((4, 16, 16), (16, 4, 16), (16, 16, 4)):
        got = L.describe_gatv2_attention(71, 53, 3, F, 1000, *al)
        assert got == ({"V": want[0], "W": want[1], "supported": True} if want else {"route": "unsupported", "supported": False})
    assert L.describe_gatv2_attention(71, 53, 3, F, 1000, 256, 64, 32) == L.describe_gatv2_attention(71, 53, 3, F, 1000)


def test_describe_edges(L):
    assert L.describe_gatv2_attention(10, 10, 2, 8, 0) == {"form": "none", "supported": True}
    assert L.describe_gatv2_attention(0, 0, 2, 8, 0) == {"form": "none", "supported": True}
    assert L.describe_gatv2_attention(10, 10, 2, 0, 5) == {"route": "zeros", "supported": True}
    assert L.describe_gatv2_attention(10, 10, 2, 513, 0) == {"route": "unsupported", "supported": False}  # the entry points' order
    assert L.describe_gatv2_attention(10, 10, 1, 512, 5) == {"V": 4, "W": 64, "supported": True}
    buf = ctypes.create_string_buffer(4)
    assert L.lib.gespmm_describe_gatv2_attention(10, 10, 2, 64, 5, 16, 16, 16, buf, 4) == 3 and buf.value == b"V=4"
    assert L.lib.gespmm_describe_gatv2_attention(10, 10, 2, 64, 5, 16, 16, 16, None, 4) == EINVAL
    for bad, code in (((10, 10, 0, 8, 5), EINVAL), ((-1, 10, 2, 8, 5), EINVAL), ((0, 10, 2, 8, 5), EINVAL), ((10, 0, 2, 8, 5), EINVAL),
                      ((BIG, 10, 1, 1, 5), ERANGE), ((10, 10, 2, 8, BIG), ERANGE)):
        with pytest.raises(L.GespmmError) as e:
            L.describe_gatv2_attention(*bad)
        assert e.value.code == code, bad
    for al in ((2, 16, 16), (16, 12, 16), (16, 16, 0)):
        with pytest.raises(L.GespmmError) as e:
            L.describe_gatv2_attention(10, 10, 2, 8, 5, *al)
        assert e.value.code == EINVAL


def _operands(M=6, K=5, H=3, F=4, nnz=9):
    rp = torch.zeros(M + 1, dtype=torch.int32)
    rp[1:] = nnz
    cp = torch.zeros(K + 1, dtype=torch.int32)
    cp[1:] = nnz
    ind = torch.zeros(nnz, dtype=torch.int32)
    return {"rp": rp, "cp": cp, "ind": ind, "xl": torch.zeros(M, H, F), "xr": torch.zeros(K, H, F), "att": torch.zeros(H, F),
            "stats": torch.zeros(M, H, 2), "out": torch.zeros(M, H, F), "go": torch.zeros(M, H, F), "delta": torch.zeros(M, H)}


def test_python_wrappers_raise_before_any_launch(pkg):
    """TypeError for the dtype of EVERY operand first — a 16-bit tensor in any slot included — then ValueError for shapes, contiguity
    and devices. Every operand here lives on the host, so a call that got past its checks raises the device ValueError — which the
    well-formed call at the end does."""
    att = pkg.attention
    o = _operands()
    M, K, H, F, nnz = 6, 5, 3, 4, 9

    def fwd(**kw):
        a = dict(o, **kw)
        return att.gatv2_attention(a["rp"], a["ind"], a["xl"], a["xr"], a["att"], negative_slope=a.get("slope", 0.2),
                                   dropout=a.get("dropout"), out=a.get("out_"), stats=a.get("stats_"))

    def brow(**kw):
        a = dict(o, **kw)
        return att.gatv2_attention_backward_row(a["rp"], a["ind"], a["xl"], a["xr"], a["att"], a["stats"], a["out"], a["go"],
                                                negative_slope=a.get("slope", 0.2), dropout=a.get("dropout"),
                                                want_att_part=a.get("want", True), results=a.get("results"))

    def bcol(**kw):
        a = dict(o, **kw)
        return att.gatv2_attention_backward_col(a["cp"], a["ind"], a["xl"], a["xr"], a["att"], a["stats"], a["delta"], a["go"],
                                                negative_slope=a.get("slope", 0.2), dropout=a.get("dropout"), result=a.get("result"))

    seed = torch.zeros(2, dtype=torch.int32)
    for call, floats, ptr in ((fwd, ("xl", "xr", "att"), "rp"), (brow, ("xl", "xr", "att", "stats", "out", "go"), "rp"),
                              (bcol, ("xl", "xr", "att", "stats", "delta", "go"), "cp")):
        for name in floats:
            for dt in (torch.float16, torch.bfloat16, torch.float64, torch.int32):
                with pytest.raises(TypeError):
                    call(**{name: o[name].to(dt)})
            with pytest.raises(TypeError):
                call(**{name: o[name].numpy()})
            with pytest.raises(TypeError):
                call(**{name: None})
        for name in (ptr, "ind"):
            with pytest.raises(TypeError):
                call(**{name: o[name].long()})
            with pytest.raises(TypeError):
                call(**{name: o[name].tolist()})
        # a bad dtype wins over a bad shape of an EARLIER operand
        with pytest.raises(TypeError):
            call(**{ptr: o[ptr][:-1], "att": o["att"].double()})
        with pytest.raises(TypeError):
            call(**{"xl": o["xl"].view(M, -1), "xr": o["xr"].half()})
        for bad in ({"dropout": 0.5}, {"dropout": (0.5, seed.long())}, {"dropout": (0.5, [1, 2])}, {"dropout": (torch.tensor(0.5), seed)},
                    {"slope": torch.tensor(0.2)}, {"slope": "0.2"}):
            with pytest.raises(TypeError):
                call(**bad)
        for bad in ({ptr: o[ptr].view(1, -1)}, {ptr: o[ptr][:-1]}, {"ind": o["ind"].view(1, -1)},
                    {"ind": torch.zeros(2 * nnz, dtype=torch.int32)[::2]}, {"xl": o["xl"].view(M, -1)}, {"xr": o["xr"].view(K, -1)},
                    {"xl": torch.zeros(M, 0, F), "xr": torch.zeros(K, 0, F), "att": torch.zeros(0, F)}, {"xr": torch.zeros(K, H, F + 1)},
                    {"xr": torch.zeros(K, H + 1, F)}, {"att": torch.zeros(1, H, F)}, {"att": torch.zeros(H, F + 1)},
                    {"att": torch.zeros(F, H).t()}, {"xl": torch.zeros(M, H, 2 * F)[:, :, ::2]},
                    {"slope": float("nan")}, {"slope": float("inf")}, {"dropout": (1.0, seed)}, {"dropout": (-0.5, seed)},
                    {"dropout": (float("nan"), seed)}, {"dropout": (0.5, torch.zeros(3, dtype=torch.int32))}):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(ValueError):
            call()  # well formed, but on the host: the device check is the last one standing
        with pytest.raises(ValueError):
            call(slope=None)
    for bad in ({"out_": torch.zeros(M, H, F + 1)}, {"stats_": torch.zeros(M, H)}, {"stats_": torch.zeros(M, H, 2)}):
        with pytest.raises(ValueError):
            fwd(**bad)
    for bad in ({"out_": torch.zeros(M, H, F).double()}, {"out_": torch.zeros(M, H, F).half()}, {"stats_": torch.zeros(M, H, 2).bfloat16()}):
        with pytest.raises(TypeError):
            fwd(**bad)
    three = (torch.zeros(M, H), torch.zeros(M, H, F), torch.zeros(M, H, F))
    for call, bad in ((brow, {"stats": torch.zeros(M, H)}), (brow, {"out": torch.zeros(M, H, F + 1)}), (brow, {"go": torch.zeros(M + 1, H, F)}),
                      (brow, {"results": (three[0], three[1], torch.zeros(M, H, F + 1))}), (brow, {"results": (three[1], three[1], three[2])}),
                      (brow, {"results": three}), (brow, {"want": False, "results": three[:2]}),
                      (bcol, {"delta": torch.zeros(M, H, 1)}), (bcol, {"go": torch.zeros(K, H, F)}), (bcol, {"cp": o["rp"]}),
                      (bcol, {"result": torch.zeros(M, H, F)}), (bcol, {"result": torch.zeros(K, H, F)})):
        with pytest.raises(ValueError):
            call(**bad)
    for call, bad in ((brow, {"results": three[:2]}), (brow, {"want": False, "results": three}), (brow, {"results": three[0]}),
                      (brow, {"results": (three[0], three[1], three[2].half())}), (bcol, {"result": torch.zeros(K, H, F).half()}),
                      (bcol, {"result": [1.0]})):
        with pytest.raises(TypeError):
            call(**bad)


def test_python_wrappers_name_the_limit(pkg):
    e = pkg.attention.Gatv2AttentionUnsupported(513, "gespmm_gatv2_attention_f32")
    assert isinstance(e, pkg._lib.GespmmError) and e.code == UNSUPPORTED and "512" in str(e) and "513" in str(e)
    assert "gatv2_attention" in str(e)


def test_layer_arguments(pkg):
    G = pkg.GATv2Conv
    with pytest.raises(ValueError):
        G(4, 3, heads=0, fused=True)
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            G(4, 3, dropout=p, fused=True)
    with pytest.raises(ValueError):
        G(4, 513, fused=True)
    assert not G(4, 513).fused and not G(4, 513, fused=False).fused   # the composition serves any F, and is the default
    fused = G(4, 512, fused=True)
    assert fused.fused and sorted(n for n, _ in fused.named_parameters()) == sorted(n for n, _ in G(4, 512).named_parameters())
    shared = G(4, 3, heads=2, share_weights=True, fused=True)
    assert shared.weight_dst is shared.weight_src and len(list(shared.parameters())) == 3
    with pytest.raises(ValueError):  # not square
        shared(torch.zeros(5, 4), torch.zeros(7, dtype=torch.int32), None, torch.zeros(6, dtype=torch.int32), None, None)
    # 16-bit features: a TypeError at the call that names the op — before anything is launched (host tensors)
    n = 5
    rp = torch.arange(n + 1, dtype=torch.int32)
    ind = torch.arange(n, dtype=torch.int32)
    for dt in (torch.float16, torch.bfloat16):
        layer = G(4, 3, heads=2, fused=True).to(dt)
        with pytest.raises(TypeError, match="gatv2_attention"):
            layer(torch.zeros(n, 4, dtype=dt), rp, ind, rp, ind, None)


# ------------------------------------------------------------------------------------------- the restatement against float64

def test_inputs_have_no_zero_sum_and_both_signs():
    for name in ("hand", "random"):
        for H in HS:
            for F in FS:
                P, x = pattern(name), inputs(name, H, F)
                t = (x["xl"][P["rows"]] + x["xr"][P["colind"]]).astype(F32)
                assert not (t == 0).any() and np.isfinite(t).all()
                if F >= 8:
                    assert (t > 0).any() and (t < 0).any()


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("F,H", ((1, 1), (3, 3), (8, 4), (100, 3)))
def test_reference_score_against_the_score_restatement(F, H, slope):
    """The float64 score on the rounded t against test_gatv2_host's restate_score (float64 on the exact sum): apart by at most the one
    add's rounding, u T — and the two sums of magnitudes agree to that as well."""
    for name in ("hand", "random"):
        P, x = pattern(name), inputs(name, H, F)
        score, terms = restate_score(P["rowptr"], P["colind"], x["xl"], x["xr"], x["att"], slope)
        _, _, _, s, T = _score64(P, x, slope)
        assert np.all(np.abs(s - score) <= U * terms) and np.all(np.abs(T - terms) <= U * terms)


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("F", FS)
def test_restatement_within_the_derived_tolerance(F, H, slope):
    """Both forms of exp, V as an aligned call has it, on the GPU tests' inputs: worst error / tolerance <= 1 in every result."""
    for name in ("hand", "random"):
        P, x = pattern(name), inputs(name, H, F)
        V, W = geometry(F)
        for mode in ("exp2", "exp"):
            got, _, _ = restate_all(P, x, slope, V, W, mode)
            r = check_all(P, x, slope, got, what="%s F=%d H=%d slope=%s %s" % (name, F, H, slope, mode))
            assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("F,align", ((8, 4), (8, 8), (20, 8), (100, 4), (512, 8)))
def test_restatement_at_other_vector_widths(F, align):
    P, x = pattern("hand"), inputs("hand", 3, F)
    V, W = geometry(F, align)
    got, _, _ = restate_all(P, x, 0.2, V, W)
    r = check_all(P, x, 0.2, got, what="hand F=%d H=3 V=%d" % (F, V))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("p", (0.3, 0.6))
@pytest.mark.parametrize("F,H", ((3, 3), (32, 4), (100, 1)))
def test_restatement_with_dropout(F, H, p):
    P, x = pattern("hand"), inputs("hand", H, F)
    V, W = geometry(F)
    got, keep, ks = restate_all(P, x, 0.2, V, W, p=p)
    r = check_all(P, x, 0.2, got, keep, ks, what="hand F=%d H=%d p=%g" % (F, H, p))
    assert max(r.values()) <= 1.0, r
    kept = seg_sum(keep.astype(F64), P["rowptr"])
    dead = (kept == 0) & (P["degs"] > 0)[:, None]
    assert dead.any() and np.all(got["out"][dead] == 0) and not np.signbit(got["out"][dead]).any()  # all dropped: exactly +0
    assert 0.5 * (1 - p) < keep.mean() < min(1.0, 1.5 * (1 - p))


def test_grad_xl_without_a_slope_is_rounding_alone():
    """negative_slope=None: every m_pf is att_f and sum_p a_p (g_p - delta) = 0, so grad_xl is zero but for rounding — the reference on
    the float64 forward's own stats is below the tolerance everywhere."""
    P, x = pattern("hand"), inputs("hand", 3, 8)
    f = ref_forward(P, x, None)
    b = ref_backward(P, x, None, np.stack((f["m"], f["l"]), -1), f["out"])
    assert np.all(np.abs(b["grad_xl"]) <= b["tol_grad_xl"])


def witness_ratios(P, x, slope):
    """Per result: the least, over the entries (of rows with d >= 2 for the row results) and the heads, of (largest change of a word by
    skipping the entry / that word's tolerance) — float64, closed form (the docstring of test_witness_every_entry_shows)."""
    f = ref_forward(P, x, slope)
    stats64 = np.stack((f["m"], f["l"]), -1)
    b = ref_backward(P, x, slope, stats64, f["out"])
    rows, cols = P["rows"], P["colind"]
    xr, go = x["xr"].astype(F64), x["go"].astype(F64)
    multi = (P["degs"] >= 2)[rows]
    a = f["a"][..., None]
    one = np.where(multi[:, None, None], 1.0 - a, 1.0)
    out_s = (f["out"][rows] - a * xr[cols]) / one
    worst = {}
    worst["out"] = (np.abs(out_s - f["out"][rows]) / f["tol_out"][rows]).max(-1)[multi].min()
    delta_s = (go[rows] * out_s).sum(-1)[..., None]
    for key, fac in (("grad_xl", b["mf"]), ("att_part", b["lk"])):
        if key == "grad_xl" and (slope is None or float(slope) == 1.0):
            continue  # zero but for rounding: test_grad_xl_without_a_slope_is_rounding_alone
        A = seg_sum((f["a"] * b["g"])[..., None] * fac, P["rowptr"])
        B = seg_sum(a * fac, P["rowptr"])
        skipped = ((A[rows] - a * b["g"][..., None] * fac) - delta_s * (B[rows] - a * fac)) / one
        worst[key] = (np.abs(skipped - b[key][rows]) / b["tol_" + key][rows]).max(-1)[multi].min()
    worst["grad_xr"] = (np.abs(b["contrib_xr"]) / b["tol_grad_xr"][cols]).max(-1).min()
    return {k_: float(v_) for k_, v_ in worst.items()}


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("F", FS)
def test_witness_every_entry_shows(F, H, slope):
    """On the very inputs the GPU tests use, the float64 reference alone: a walk that skips ANY single entry lands outside the tolerance
    of every result the entry feeds. For a skipped entry j of a row with d >= 2, in closed form (a'_p = a_p / (1 - a_j)):
        out'     = (out - a_j xr_j) / (1 - a_j)
        grad_xl' = [(A - a_j g_j m_j) - delta' (B - a_j m_j)] / (1 - a_j),   A = sum a_p g_p m_p, B = sum a_p m_p, delta' = <go, out'>
        att_part' the same with leaky(t_p) in m_p's place,
    and grad_xr, at the entry's column, loses that entry's contribution ds_j m_j + a_j go (every entry: a single-entry row has a = 1).
    The entry of a single-entry row has ds_p = 0 by construction: nothing can show it in grad_xl or att_part, which is why their
    condition is about rows with d >= 2. The restatement itself stays within 0.25 of the tolerance on these inputs (asserted here), so
    a restatement with the skip is further than the tolerance from the float64 result wherever the float64 results with and without
    the skip differ by more than 1.25 tolerances — in at least one word of the segment's slice, for every head."""
    for name in ("hand", "random"):
        P, x = pattern(name), inputs(name, H, F)
        V, W = geometry(F)
        got, _, _ = restate_all(P, x, slope, V, W)
        assert max(check_all(P, x, slope, got, what="%s F=%d H=%d slope=%s" % (name, F, H, slope)).values()) <= 0.25
        worst = witness_ratios(P, x, slope)
        print("%s F=%d H=%d slope=%s least (change by a skipped entry / tolerance): %s" %
              (name, F, H, slope, "  ".join("%s %.3g" % kv for kv in worst.items())))
        assert min(worst.values()) > 1.25, worst


# ------------------------------------------------------------------------------------------------------------ special shapes

def chain_case(scores, F=4):
    """One row whose entry p has exactly the score scores[p], by the choice of att and xr: att = (1, 0, ..), xl = 0, xr[p] =
    (scores[p], ..) and no slope, so t = xr, leaky(t) = t and s_p = 1 * scores[p] + 0 * .. exactly. (A zero att word and a zero xl row
    are fine here: nothing is asked of a witness.)"""
    d = len(scores)
    rng = np.random.RandomState(3)
    rowptr, colind = np.array([0, 0, d, d], dtype=np.int32), np.arange(d, dtype=np.int32)
    P = {"M": 3, "K": d, "nnz": d, "rowptr": rowptr, "colind": colind, "rows": np.full(d, 1, dtype=np.int32), "degs": np.array([0, d, 0])}
    att = np.zeros((1, F), F32)
    att[0, 0] = 1
    xr = rng.uniform(0.5, 1, size=(d, 1, F)).astype(F32)
    xr[:, 0, 0] = np.asarray(scores, dtype=F32)
    return P, {"xl": np.zeros((3, 1, F), F32), "xr": xr, "att": att, "go": rng.uniform(0.5, 1, size=(3, 1, F)).astype(F32)}


def test_special_shapes_exact():
    V, W = 4, 4
    # a single entry: out == xr[c] bit for bit, stats == (s, 1); the rows around it are empty: +0 everywhere
    P, x = chain_case([0.37])
    out, stats = restate_forward(P, x, None, V, W)
    assert out[1].tobytes() == x["xr"][0].tobytes() and stats[1, 0, 0] == F32(0.37) and stats[1, 0, 1] == 1.0
    assert not out[[0, 2]].any() and not stats[[0, 2]].any() and not np.signbit(out[[0, 2]]).any() and not np.signbit(stats[[0, 2]]).any()
    # ascending scores: a rescale at every entry after the first; descending: none — both inside the tolerance
    up = np.linspace(-3, 3, 40)
    for scores, want in ((up, 39), (up[::-1], 0)):
        P, x = chain_case(scores)
        for mode in ("exp2", "exp"):
            out, stats, n = restate_forward(P, x, None, V, W, mode, count_rescales=True)
            assert int(n[1, 0]) == want
            f = ref_forward(P, x, None)
            assert ratio(out, f["out"], f["tol_out"]) <= 1.0 and ratio(stats[..., 1], f["l"], f["tol_l"]) <= 1.0
            assert stats[1, 0, 0] == F32(3.0)
    # scores over +-80: t underflows to 0 for most entries and nothing is NaN
    P, x = chain_case([-80.0, 80.0, -79.0, 0.0, 79.5, -80.0])
    for mode in ("exp2", "exp"):
        out, stats = restate_forward(P, x, None, V, W, mode)
        assert np.isfinite(out).all() and np.isfinite(stats).all() and stats[1, 0, 0] == F32(80.0)
        f = ref_forward(P, x, None)
        assert ratio(out, f["out"], f["tol_out"]) <= 1.0


def test_restatement_on_a_hand_made_case():
    """One row, two entries, one head, F = 2, slope 0.5, every number worked by hand: t = (3, -4) and (1, -2), leaky (3, -2) and (1, -1),
    att (2, 4): s = (-2, -2), so a = (1/2, 1/2), out = (xr_1 + xr_0) / 2 = (1, 0). go = (1, 1): g = (1, 1) = delta, ds = 0."""
    P = {"M": 1, "K": 2, "nnz": 2, "rowptr": np.array([0, 2], dtype=np.int32), "colind": np.array([1, 0], dtype=np.int32),
         "rows": np.zeros(2, dtype=np.int32), "degs": np.array([2]), "colptr": np.array([0, 1, 2], dtype=np.int32),
         "rowind": np.zeros(2, dtype=np.int32), "order": np.array([1, 0])}
    x = {"xl": np.array([[[1.0, -3.0]]], F32), "xr": np.array([[[0.0, 1.0]], [[2.0, -1.0]]], F32), "att": np.array([[2.0, 4.0]], F32),
         "go": np.array([[[1.0, 1.0]]], F32)}
    got, _, _ = restate_all(P, x, 0.5, 1, 4)
    assert got["out"].tolist() == [[[1.0, 0.0]]] and got["stats"].tolist() == [[[-2.0, 2.0]]] and got["delta"].tolist() == [[1.0]]
    assert got["grad_xl"].tolist() == [[[0.0, 0.0]]] and got["att_part"].tolist() == [[[0.0, 0.0]]]
    assert got["grad_xr"].tolist() == [[[0.5, 0.5]], [[0.5, 0.5]]]   # ds = 0: the aggregation's chain alone, a_p go
    f = ref_forward(P, x, 0.5)
    assert f["out"].tolist() == [[[1.0, 0.0]]] and f["s"].tolist() == [[-2.0], [-2.0]]


if __name__ == "__main__":  # the search that fills SEEDS: python tests/test_gatv2_attention_host.py [F ..] — per case the first draw
    import sys  # at which the inputs have no zero sum and the witness condition holds for both slopes

    found = {}
    for F_ in [int(a) for a in sys.argv[1:]] or FS:
        for name_ in ("hand", "random"):
            for H_ in HS:
                for draw_ in range(3000):  # (where none passes: collect passing draws at H = 1 and name one per head)
                    P_, x_ = pattern(name_), draw_inputs(name_, H_, F_, draw_)
                    t_ = (x_["xl"][P_["rows"]] + x_["xr"][P_["colind"]]).astype(F32)
                    if not (t_ == 0).any() and all(min(witness_ratios(P_, x_, s_).values()) > 1.25 for s_ in SLOPES):
                        break
                else:
                    draw_ = -1
                if draw_:
                    found[(name_, H_, F_)] = draw_
                print(name_, H_, F_, draw_, flush=True)
    print(found)
