"""The fused dot-product attention (gespmm_dot_attention_f32 and its two backward passes) without a GPU: exports, the order of the
argument checks, the describe table, the Python wrappers' errors, the layer's argument errors — and an fp32 RESTATEMENT of the three
kernels' chains in numpy, held against float64 within a derived tolerance. The GPU tests import the inputs, the restatement, the
float64 references and the tolerances from here, unchanged.

The tolerances (u = 2^-23; every fp32 operation is taken to err by at most u relative, a generous unit; d entries in the segment)
-------------------------------------------------------------------------------------------------------------------------------
dot: a chain of F fmaf, a butterfly and the multiplication by scale: |s_p - s64_p| <= es_p = u (F + 2) scale sum_f |q_f k_pf|.
forward: with z_p = s_p - m, zbar = sum_p a_p |z_p|:
    tol(out_f) = sum_p [a_p (es_p + sum_j a_j es_j) + a_p u (2 |z_p| + 2 zbar + 2 d + 8)] |v_pf| + u (d + 2) sum_p a_p |v_pf| + 2^-120
  origin of the terms: the score's error moves a_p by a_p es_p directly and by a_p sum_j a_j es_j through the normaliser; exp2 of
  fl(z log2 e) errs by about 2 |z| u relative (once in t, once — averaged — in l); each of the at most d rescales of acc and l costs
  one rounding each (2 d), the division, the product t v and the first step a handful more (8); the fmaf chain of acc itself is
  u (d + 2) of the sum of magnitudes. With dropout |v| is |v| keep s and one more rounding fl(t s) joins the 8.
stats: m is one of the s_p: tol(m) = max_p es_p. l = sum_p exp(s_p - m): tol(l) = sum_p e^{z_p} (es_p + max_j es_j + u (2 |z_p| + d + 4)).
backward, both passes — the float64 reference reads the DEVICE's (restatement's) own stats, out and delta, so what the forward's
tolerance can move is not in the comparison (the layer tests, which compare against a float64 forward, use the project's 1e-4 bar):
    tol(delta) = u (F + 2) sum_f |go_f out_f|                                             (the dot)
    ea_p = es_p + u (2 |z_p| + 4)                                                         (relative error of a_p = exp(s_p - m) / l)
    eg_p = u (F + 3) sum_f |go_f v_pf| keep s                                             (the dot; + 1: the dropout's rounding)
    eds_p = a_p (ea_p + 3 u) (|g_p| + |delta|) + a_p (eg_p + tol(delta))                  (ds_p = a_p (g_p - delta))
    tol(grad_q_f) = scale [sum_p eds_p |k_pf| + u (d + F + 4) sum_p |ds_p k_pf|] + 2^-120 (chain, final scaling)
    tol(grad_k_f) = scale [sum_p eds_p |q_pf| + u (d + F + 4) sum_p |ds_p q_pf|] + 2^-120
    tol(grad_v_f) = sum_p a_p keep s (ea_p + 2 u) |go_pf| + u (d + F + 4) sum_p a_p keep s |go_pf| + 2^-120
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_heads_host import EALIGN, EINVAL, ERANGE

F32, F64 = np.float32, np.float64
U = 2.0 ** -23
FLOOR = 2.0 ** -120
UNSUPPORTED = -7
NEW = ("gespmm_dot_attention_f32", "gespmm_dot_attention_dropout_f32", "gespmm_dot_attention_backward_q_f32",
       "gespmm_dot_attention_backward_q_dropout_f32", "gespmm_dot_attention_backward_kv_f32",
       "gespmm_dot_attention_backward_kv_dropout_f32", "gespmm_describe_dot_attention")
OK = 0x1000  # a made-up address: the checks look at the number only and return before anything could read it
BIG = (1 << 31) - 4096  # one past the largest count of 32-bit word positions
FS = (1, 3, 8, 20, 32, 64, 100, 512)
HS = (1, 3, 4)
SEED = (0x12345678, 0x9ABCDEF0)
# (pattern, H, F) -> which draw of the inputs is used (0 where absent): see inputs()
SEEDS = {("hand", 1, 1): 3, ("hand", 3, 1): 15, ("hand", 4, 1): 51, ("hand", 3, 3): 1, ("hand", 1, 20): 1, ("hand", 3, 20): 3,
         ("hand", 3, 32): 5, ("hand", 4, 32): 8, ("hand", 4, 64): 3, ("hand", 1, 100): 1, ("hand", 1, 512): 1, ("hand", 3, 512): 7,
         ("hand", 4, 512): 14, ("random", 3, 8): 2, ("random", 1, 20): 2, ("random", 3, 20): 1, ("random", 4, 20): 8, ("random", 1, 32): 11,
         ("random", 3, 32): 36, ("random", 4, 32): 18, ("random", 1, 64): 1, ("random", 3, 64): 3, ("random", 4, 64): 11,
         ("random", 1, 100): 1, ("random", 3, 100): 3, ("random", 4, 100): 1, ("random", 3, 512): 5, ("random", 4, 512): 33,
         # the head counts past HS that tests/test_gpu_dot_attention.py::test_many_heads_against_float64 runs
         ("hand", 8, 32): 37, ("hand", 33, 3): 5, ("hand", 33, 32): 1080}


# ------------------------------------------------------------------------------------------------------------- patterns and inputs

def transpose(rowptr, colind, K):
    """-> (colptr, rowind, order): the CSC arrays of the pattern, entries of a column in CSR order (a stable sort)."""
    order = np.argsort(colind, kind="stable").astype(np.int64)
    rows = np.repeat(np.arange(rowptr.size - 1, dtype=np.int32), np.diff(rowptr))
    colptr = np.zeros(K + 1, dtype=np.int32)
    colptr[1:] = np.cumsum(np.bincount(colind, minlength=K))
    return colptr, rows[order].astype(np.int32), order


@functools.lru_cache(maxsize=None)
def pattern(name):
    """"hand": M = 71, K = 53, row degrees {0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 300} repeated, first and last row empty, columns unsorted
    with repeats. Rows of up to 9 entries draw their columns from [0, 12), rows of 63 .. 65 from [12, 30), hub rows from [30, 53): a
    column's gradient then sums entries of comparable weight, and the 1 / 300 share of a hub entry is not asked to show against the
    error bound of a single-entry row's share in the same word (the witness test). "random": M = 300, K = 211, degrees 0 .. 9 — more
    than one workgroup at every W."""
    rng = np.random.RandomState(7 if name == "hand" else 8)
    if name == "hand":
        cycle = (0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 300)
        M, K = 71, 53
        degs = np.array([cycle[i % 12] for i in range(M)])
        degs[-1] = 0
    else:
        M, K = 300, 211
        degs = rng.randint(0, 10, size=M)
    rowptr = np.zeros(M + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    rows = np.repeat(np.arange(M, dtype=np.int32), degs)
    colind = rng.randint(0, K, size=int(rowptr[-1])).astype(np.int32)
    if name == "hand":
        dr = degs[rows]
        lo, hi = np.where(dr <= 9, 0, np.where(dr <= 65, 12, 30)), np.where(dr <= 9, 12, np.where(dr <= 65, 30, K))
        colind = (lo + colind % (hi - lo)).astype(np.int32)
    colptr, rowind, order = transpose(rowptr, colind, K)
    return {"M": M, "K": K, "nnz": int(rowptr[-1]), "rowptr": rowptr, "colind": colind, "colptr": colptr, "rowind": rowind, "order": order,
            "rows": rows, "degs": degs}


@functools.lru_cache(maxsize=None)
def inputs(name, H, F):
    """q, k, v, grad_out for a pattern, shaped so that EVERY entry shows in every result it feeds (the witness test) although the
    bounds on the dots' errors grow like F and a hub entry's share is 1 / 300:
      * magnitudes in [0.5, 1): no word is close to zero;
      * q and k with a random sign per word, q scaled per row: scores spread wide on short rows (about +-4), narrow on hub rows and at
        large F, where the bound on the score's error is large against the 1 / d share of an entry;
      * v with ONE sign and ONE amplitude per (column, head) — the K amplitudes of a head are the K steps of [0.5, 1.5) in a random
        order, all different — and grad_out positive, so that g_p = <grad_out, v_p> is a coherent sum — of the order of its error
        bound's sum of magnitudes, not sqrt(F) below it — and the g_p of a row differ from each other and from delta by about as much.
    A result of few words can still hide an entry by coincidence (at F = 1 a row's out may fall on one of its v): SEEDS names, per case,
    the first seed at which the witness test's condition holds — a condition on the inputs, found and checked on the CPU."""
    P = pattern(name)
    rng = np.random.RandomState(1000 * H + F + (0 if name == "hand" else 500000) + 7919 * SEEDS.get((name, H, F), 0))

    def draw(shape, signs=True):
        x = rng.uniform(0.5, 1.0, size=shape)
        return (x * rng.choice((-1.0, 1.0), size=shape) if signs else x).astype(F32)

    q, k, go = draw((P["M"], H, F)), draw((P["K"], H, F)), draw((P["M"], H, F), signs=False)
    amp = np.stack([(0.5 + rng.permutation(P["K"]) / P["K"]) * rng.choice((-1.0, 1.0), size=P["K"]) for _ in range(H)], 1)
    v = (draw((P["K"], H, F), signs=False) * amp[:, :, None]).astype(F32)
    base = np.where(P["degs"] <= 9, 2.0, np.where(P["degs"] <= 65, 0.8, 0.5)) * min(1.0, 32.0 / F)
    q = (q * base[:, None, None]).astype(F32)
    return {"q": q, "k": k, "v": v, "go": go, "scale": float(F32(1.0 / np.sqrt(F)))}


def geometry(F, align=16):
    """(V, W) of the kernels at width F for operands on an `align`-byte boundary: the rule, restated."""
    V = 4
    while V > 1 and (F % V != 0 or align % (4 * V) != 0):
        V //= 2
    W = 4
    while W < 64 and 8 * W < F:
        W *= 2
    return V, W


def keep_mask(P, H, p, transposed=False):
    """[nnz, H] bool, in CSR order (or in CSC order): the kernels' decision for every entry and head, and the kept entry's scale."""
    from gespmm_amd import _lib, softmax

    rows, cols = (P["rows"], P["colind"]) if not transposed else (P["rowind"], np.repeat(np.arange(P["K"]), np.diff(P["colptr"])))
    bits = softmax.restate_edge_dropout_bits(SEED[0], SEED[1], rows[:, None], cols[:, None], np.arange(H)[None, :])
    return bits >= np.uint32(_lib.edge_dropout_threshold(p)), F32(1.0) / (F32(1.0) - F32(p))


# ------------------------------------------------------------------------------------------------------------------ the restatement

def fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 numbers is exact in float64; the sum is rounded to float64, then to fp32 (a double
    rounding that differs from fmaf in rare ties: the restatement is held to a tolerance, not to bits)."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def expf(x, mode):
    """__expf as exp2(fl(x log2 e)) ("exp2") or as a correctly rounded exp ("exp"): the two forms the device's fast exp may take."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(under="ignore", over="ignore"):
        if mode == "exp2":
            return np.exp2((x * F32(1.4426950408889634)).astype(F32)).astype(F32)
        return np.exp(x).astype(F32)


def lane_dot(x, y, V, W):
    """The pinned dot of two fp32 arrays [..., F]: lane l runs one fmaf chain from +0 over j = l V + i + t W V, then the xor butterfly."""
    F = x.shape[-1]
    nT = -(-F // (W * V))
    pad = nT * W * V - F
    if pad:
        z = np.zeros(x.shape[:-1] + (pad,), dtype=F32)
        x, y = np.concatenate((x, z), -1), np.concatenate((y, z), -1)
    x, y = x.reshape(x.shape[:-1] + (nT, W, V)), y.reshape(y.shape[:-1] + (nT, W, V))
    acc = np.zeros(x.shape[:-3] + (W,), dtype=F32)
    for t in range(nT):
        for i in range(V):
            acc = fma32(x[..., t, :, i], y[..., t, :, i], acc)
    m = W // 2
    lanes = np.arange(W)
    while m:
        acc = (acc + acc[..., lanes ^ m]).astype(F32)
        m //= 2
    return acc[..., 0]


def steps(ptr):
    """For t = 0, 1, ..: (segments with more than t entries, the position of their t-th entry) — a chain per segment, all segments at once."""
    d = np.diff(ptr)
    for t in range(int(d.max()) if d.size else 0):
        seg = np.nonzero(d > t)[0]
        yield seg, ptr[seg] + t


def restate_forward(P, x, V, W, mode="exp2", keep=None, ks=None, count_rescales=False):
    """-> (out f32[M, H, F], stats f32[M, H, 2]) by the forward kernel's chain; with count_rescales also the number of steps with m' > m."""
    q, k, v, scale = x["q"], x["k"], x["v"], F32(x["scale"])
    M, H, F = q.shape
    s = (scale * lane_dot(q[P["rows"]], k[P["colind"]], V, W)).astype(F32)  # [nnz, H]
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
        acc[seg] = fma32(tv[..., None], v[P["colind"][e]], (acc[seg] * c[..., None]).astype(F32))
        m[seg] = mn
    some = (P["degs"] > 0)[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(some, (acc / l[..., None]).astype(F32), F32(0))
    stats = np.stack((m, l), -1)
    return (out, stats, rescales) if count_rescales else (out, stats)


def _entry_terms(P, x, stats, V, W, mode, keep, ks, transposed, skip=None):
    """s, a, g' and ds of every entry by the kernels' expressions, in CSR order or (transposed) in CSC order."""
    rows, cols = (P["rows"], P["colind"]) if not transposed else (P["rowind"], np.repeat(np.arange(P["K"]), np.diff(P["colptr"])))
    scale = F32(x["scale"])
    s = (scale * lane_dot(x["q"][rows], x["k"][cols], V, W)).astype(F32)
    g = lane_dot(x["go"][rows], x["v"][cols], V, W)
    a = (expf(s - stats[rows, :, 0], mode) / stats[rows, :, 1]).astype(F32)
    av = a
    if keep is not None:
        g = np.where(keep, (g * ks).astype(F32), F32(0))
        av = np.where(keep, (a * ks).astype(F32), F32(0))
    return rows, cols, a, av, g


def restate_backward_q(P, x, stats, out, V, W, mode="exp2", keep=None, ks=None):
    """-> (delta f32[M, H], grad_q f32[M, H, F]) by the row pass's chain."""
    rows, cols, a, _, g = _entry_terms(P, x, stats, V, W, mode, keep, ks, False)
    delta = lane_dot(x["go"], out, V, W)
    ds = (a * (g - delta[rows]).astype(F32)).astype(F32)
    acc = np.zeros(x["q"].shape, F32)
    for seg, e in steps(P["rowptr"]):
        acc[seg] = fma32(ds[e][..., None], x["k"][cols[e]], acc[seg])
    return delta, (F32(x["scale"]) * acc).astype(F32)


def restate_backward_kv(P, x, stats, delta, V, W, mode="exp2", keep_t=None, ks=None):
    """-> (grad_k, grad_v) f32[K, H, F] by the column pass's chain (keep_t: the mask in CSC order)."""
    rows, cols, a, av, g = _entry_terms(P, x, stats, V, W, mode, keep_t, ks, True)
    ds = (a * (g - delta[rows]).astype(F32)).astype(F32)
    gk, gv = np.zeros(x["k"].shape, F32), np.zeros(x["k"].shape, F32)
    for seg, e in steps(P["colptr"]):
        gk[seg] = fma32(ds[e][..., None], x["q"][rows[e]], gk[seg])
        gv[seg] = fma32(av[e][..., None], x["go"][rows[e]], gv[seg])
    return (F32(x["scale"]) * gk).astype(F32), gv


# ------------------------------------------------------------------------------------------ float64 references and their tolerances

def seg_sum(x, ptr):
    """sum of x's rows over each segment -> [segments, ...] (float64; an empty segment gives 0)."""
    out = np.zeros((ptr.size - 1,) + x.shape[1:], dtype=F64)
    ne = np.nonzero(np.diff(ptr) > 0)[0]
    if ne.size:
        out[ne] = np.add.reduceat(x, ptr[ne], axis=0)
    return out


def ref_forward(P, x, keep=None, ks=None):
    """float64 on the fp32 inputs -> dict(out, m, l, tol_out, tol_m, tol_l) and the per-entry pieces the other references reuse."""
    rows, cols, ptr = P["rows"], P["colind"], P["rowptr"]
    q, k, v = (x[n].astype(F64) for n in ("q", "k", "v"))
    scale = F64(F32(x["scale"]))
    M, H, F = q.shape
    d = P["degs"].astype(F64)[:, None]
    s = scale * (q[rows] * k[cols]).sum(-1)
    es = U * (F + 2) * scale * (np.abs(q[rows]) * np.abs(k[cols])).sum(-1)
    m = np.full((M, H), -np.inf)
    np.maximum.at(m, rows, s)
    m[P["degs"] == 0] = 0.0
    z = s - m[rows]
    ez = np.exp(z)
    l = seg_sum(ez, ptr)
    a = ez / np.where(l > 0, l, 1.0)[rows]
    w = a if keep is None else a * keep * F64(ks)  # the coefficient that multiplies v
    vv = v[cols]
    out = seg_sum(w[..., None] * vv, ptr)
    zbar = seg_sum(a * np.abs(z), ptr)
    esbar = seg_sum(a * es, ptr)
    per = w * (es + esbar[rows]) + w * U * (2 * np.abs(z) + 2 * zbar[rows] + 2 * d[rows] + 8 + (0 if keep is None else 1))
    tol_out = seg_sum(per[..., None] * np.abs(vv), ptr) + U * (d[..., None] + 2) * seg_sum(w[..., None] * np.abs(vv), ptr) + FLOOR
    es_max = np.zeros((M, H))
    np.maximum.at(es_max, rows, es)
    tol_l = seg_sum(ez * (es + es_max[rows] + U * (2 * np.abs(z) + d[rows] + 4)), ptr) + FLOOR
    return {"out": out, "m": m, "l": l, "tol_out": tol_out, "tol_m": es_max + FLOOR, "tol_l": tol_l, "a": a, "w": w, "s": s, "es": es}


def ref_backward(P, x, stats, out, delta=None, keep=None, ks=None):
    """float64 on the fp32 inputs AND on the given (device's, restatement's) stats and out — and delta, for the column pass; without it
    the float64 delta of `out` — -> dict(delta, grad_q, grad_k, grad_v and their tol_*, and the per-entry contributions)."""
    rows, cols, ptr = P["rows"], P["colind"], P["rowptr"]
    q, k, v, go = (x[n].astype(F64) for n in ("q", "k", "v", "go"))
    scale = F64(F32(x["scale"]))
    M, H, F = q.shape
    st = stats.astype(F64)
    kf = F64(1.0) if keep is None else keep * F64(ks)
    s = scale * (q[rows] * k[cols]).sum(-1)
    es = U * (F + 2) * scale * (np.abs(q[rows]) * np.abs(k[cols])).sum(-1)
    z = s - st[rows, :, 0]
    a = np.exp(z) / st[rows, :, 1]
    g = (go[rows] * v[cols]).sum(-1) * kf
    eg = U * (F + 3) * (np.abs(go[rows]) * np.abs(v[cols])).sum(-1) * kf
    delta64 = (go * out.astype(F64)).sum(-1)
    tol_delta = U * (F + 2) * (np.abs(go) * np.abs(out.astype(F64))).sum(-1) + FLOOR
    dl = delta64 if delta is None else delta.astype(F64)
    ds = a * (g - dl[rows])
    ea = es + U * (2 * np.abs(z) + 4)
    eds = a * (ea + 3 * U) * (np.abs(g) + np.abs(dl[rows])) + a * (eg + tol_delta[rows])
    dr = P["degs"].astype(F64)[:, None, None]
    dc = np.diff(P["colptr"]).astype(F64)[:, None, None]
    o = P["order"]  # CSC order: the column pass sums a column's entries
    ck = scale * ds[..., None] * q[rows]
    cv = (a * kf)[..., None] * go[rows]
    res = {"delta": delta64, "tol_delta": tol_delta,
           "grad_q": scale * seg_sum(ds[..., None] * k[cols], ptr),
           "tol_grad_q": scale * (seg_sum(eds[..., None] * np.abs(k[cols]), ptr) + U * (dr + F + 4) * seg_sum(np.abs(ds[..., None] * k[cols]), ptr))
           + FLOOR,
           "grad_k": seg_sum(ck[o], P["colptr"]),
           "tol_grad_k": scale * seg_sum((eds[..., None] * np.abs(q[rows]))[o], P["colptr"]) + U * (dc + F + 4) * seg_sum(np.abs(ck)[o], P["colptr"])
           + FLOOR,
           "grad_v": seg_sum(cv[o], P["colptr"]),
           "tol_grad_v": seg_sum(((a * kf * (ea + 2 * U))[..., None] * np.abs(go[rows]))[o], P["colptr"])
           + U * (dc + F + 4) * seg_sum(np.abs(cv)[o], P["colptr"]) + FLOOR,
           "contrib_k": ck, "contrib_v": cv, "a": a, "g": g, "ds": ds}
    return res


def ratio(got, ref, tol):
    """worst |got - ref| / tol; a NaN in got counts as infinite."""
    err = np.abs(np.asarray(got, dtype=F64).reshape(ref.shape) - ref)
    if err.size == 0:
        return 0.0
    if np.isnan(err).any():
        return float("inf")
    return float((err / tol).max())


def check_all(P, x, got, keep=None, ks=None, what=""):
    """The five results of the three launches (a dict with out, stats, delta, grad_q, grad_k, grad_v) against float64: -> the worst
    ratio per result, printed. The backward's reference reads got's own stats, out and delta."""
    keep_csr = keep
    f = ref_forward(P, x, keep_csr, ks)
    b = ref_backward(P, x, got["stats"], got["out"], None, keep_csr, ks)
    bc = ref_backward(P, x, got["stats"], got["out"], got["delta"], keep_csr, ks)
    r = {"out": ratio(got["out"], f["out"], f["tol_out"]), "m": ratio(got["stats"][..., 0], f["m"], f["tol_m"]),
         "l": ratio(got["stats"][..., 1], f["l"], f["tol_l"]), "delta": ratio(got["delta"], b["delta"], b["tol_delta"]),
         "grad_q": ratio(got["grad_q"], b["grad_q"], b["tol_grad_q"]), "grad_k": ratio(got["grad_k"], bc["grad_k"], bc["tol_grad_k"]),
         "grad_v": ratio(got["grad_v"], bc["grad_v"], bc["tol_grad_v"])}
    print("%s worst error / tolerance: %s" % (what, "  ".join("%s %.3g" % kv for kv in r.items())))
    return r


def restate_all(P, x, V, W, mode="exp2", p=None):
    keep = keep_t = ks = None
    if p is not None:
        H = x["q"].shape[1]
        keep, ks = keep_mask(P, H, p)
        keep_t, _ = keep_mask(P, H, p, transposed=True)
    out, stats = restate_forward(P, x, V, W, mode, keep, ks)
    delta, grad_q = restate_backward_q(P, x, stats, out, V, W, mode, keep, ks)
    grad_k, grad_v = restate_backward_kv(P, x, stats, delta, V, W, mode, keep_t, ks)
    return {"out": out, "stats": stats, "delta": delta, "grad_q": grad_q, "grad_k": grad_k, "grad_v": grad_v}, keep, ks


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
    for name in ("attention", "DotAttentionFunction", "TransformerConv"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("dot_attention", "dot_attention_backward_q", "dot_attention_backward_kv"):
        assert callable(getattr(pkg.attention, name))
    assert callable(L.describe_dot_attention)
    assert b"512" in L.lib.gespmm_error_string(UNSUPPORTED)


# (entry point, its dropout form, number of pointers, positions of the results, position of stats)
ENTRIES = (("gespmm_dot_attention_f32", 7, (5, 6), 6), ("gespmm_dot_attention_backward_q_f32", 10, (8, 9), 5),
           ("gespmm_dot_attention_backward_kv_f32", 10, (8, 9), 5))


@pytest.mark.parametrize("name,np_,results,stats_at", ENTRIES)
@pytest.mark.parametrize("drop", (False, True))
def test_return_codes(L, name, np_, results, stats_at, drop):
    """(pointers | M, K, H, F, nnz, scale[, p, seed], stream): sizes that make no sense (a bad scale and a bad p with them), sizes too
    large, the slice no kernel serves, nnz == 0 / F == 0 (the results and the seed alone), then the pointers: NULL, alignment."""
    f0 = getattr(L.lib, name.replace("_f32", "_dropout_f32") if drop else name)

    def f(ptrs, M, K, H, F, nnz, scale, p=0.25, seed=_p(OK)):
        tail = (p, seed, None) if drop else (None,)
        return f0(*ptrs, M, K, H, F, nnz, scale, *tail)

    none = (None,) * np_
    assert f(none, 4, 4, 0, 8, 10, 0.5) == EINVAL        # H < 1
    assert f(none, -1, 4, 2, 8, 10, 0.5) == EINVAL       # negative sizes
    assert f(none, 4, -4, 2, 8, 0, 0.5) == EINVAL
    assert f(none, 4, 4, 2, -8, 10, 0.5) == EINVAL
    assert f(none, 4, 4, 2, 8, -1, 0.5) == EINVAL
    assert f(none, 4, 0, 2, 8, 10, 0.5) == EINVAL        # K < 1 with entries
    assert f(none, 0, 4, 2, 8, 10, 0.5) == EINVAL        # entries without rows
    assert f(none, 4, 4, 2, 8, 10, float("inf")) == EINVAL
    assert f(none, 4, 4, 2, 8, 10, float("nan")) == EINVAL
    assert f(none, 4, 4, 0, 8, BIG, 0.5) == EINVAL       # what makes no sense before what is too large
    assert f(none, 4, 4, 2, 513, 10, float("nan")) == EINVAL  # ... and before what is not served
    if drop:
        for p in (-0.1, 1.0, float("nan")):
            assert f(none, 4, 4, 2, 8, 10, 0.5, p=p) == EINVAL
            assert f(none, 4, 4, 2, 8, BIG, 0.5, p=p) == EINVAL
    assert f(none, 4, 4, 1, 8, BIG, 0.5) == ERANGE       # nnz
    assert f(none, 4, 4, 2, 8, BIG // 2 + 1, 0.5) == ERANGE    # nnz H
    assert f(none, BIG, 4, 1, 1, 10, 0.5) == ERANGE      # M
    assert f(none, BIG // 16 + 1, 4, 2, 8, 10, 0.5) == ERANGE  # M H F words
    assert f(none, 4, BIG // 16 + 1, 2, 8, 10, 0.5) == ERANGE  # K H F words
    assert f(none, BIG // 2 + 1, 4, 1, 1, 10, 0.5) == ERANGE   # the 2 M H words of stats
    assert f(none, BIG, 4, 1, 1, 0, 0.5) == ERANGE       # too large comes before "no entries"
    assert f(none, BIG // 1024 + 1, 4, 2, 513, 10, 0.5) == ERANGE  # ... and before "not served"
    assert f(none, 4, 4, 2, 513, 10, 0.5) == UNSUPPORTED
    assert f(none, 4, 4, 2, 513, 0, 0.5) == UNSUPPORTED  # before "no entries"
    assert f(tuple(_p(OK) for _ in none), 4, 4, 2, 4096, 10, 0.5) == UNSUPPORTED  # nothing is launched
    assert f(none, 4, 4, 2, 512, 10, 0.5) == EINVAL      # the widest slice served: on to the pointers
    # no entries, or rows of no width: the results (and the seed) alone are looked at, and zero-filled on a device
    for F, nnz in ((8, 0), (0, 10)):
        assert f(none, 4, 4, 2, F, nnz, 0.5) == (0 if F == 0 and name.endswith("kv_f32") else EINVAL)
        for bad in results:
            if F == 0 and name.endswith("kv_f32"):
                continue  # (grad_k and grad_v have no words)
            if F == 0 and bad != stats_at and bad != 8:
                continue  # (out / grad_q have no words: stats and delta are what is written)
            ptrs = [_p(OK + 2) if i == bad else (_p(OK) if i in results else None) for i in range(np_)]
            assert f(ptrs, 4, 4, 2, F, nnz, 0.5) == EALIGN, (F, nnz, bad)
        if drop:
            assert f(none, 4, 4, 2, F, nnz, 0.5, seed=None) == EINVAL
            assert f(none, 0, 0, 2, F, 0, 0.5, seed=_p(OK + 2)) == EALIGN
    assert f(none, 0, 0, 2, 8, 0, 0.5) == 0              # nothing to write
    # the pointers
    assert f(none, 4, 4, 2, 8, 10, 0.5) == EINVAL
    for bad in range(np_):
        assert f([None if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.5) == EINVAL, bad
        assert f([_p(OK + 2) if i == bad else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.5) == EALIGN, bad
    assert f([_p(OK + 4) if i == stats_at else _p(OK) for i in range(np_)], 4, 4, 2, 8, 10, 0.5) == EALIGN  # stats: 8 bytes
    assert f([None if i == 0 else _p(OK + 2) for i in range(np_)], 4, 4, 2, 8, 10, 0.5) == EINVAL  # NULL before alignment
    if drop:
        assert f([_p(OK)] * np_, 4, 4, 2, 8, 10, 0.5, seed=None) == EINVAL
        assert f([_p(OK)] * np_, 4, 4, 2, 8, 10, 0.5, seed=_p(OK + 2)) == EALIGN


@pytest.mark.parametrize("F", (1, 3, 8, 20, 32, 33, 64, 100, 512, 513))
def test_describe(L, F):
    for align in (16, 8, 4):
        got = L.describe_dot_attention(71, 53, 3, F, 1000, align, align, align)
        if F > 512:
            assert got == {"route": "unsupported"}
            continue
        V, W = geometry(F, align)
        assert got == {"V": V, "W": W}, (F, align, got)
        assert F % V == 0 and (4 * V) <= align and 8 * W >= F and (W == 4 or 4 * W < F)
    # the least aligned operand decides, whichever it is; more than 16 bytes is as good as 16
    want = geometry(F, 4) if F <= 512 else None
    for al in ((4, 16, 16), (16, 4, 16), (16, 16, 4)):
        got = L.describe_dot_attention(71, 53, 3, F, 1000, *al)
        assert got == ({"V": want[0], "W": want[1]} if want else {"route": "unsupported"})
    assert L.describe_dot_attention(71, 53, 3, F, 1000, 256, 64, 32) == L.describe_dot_attention(71, 53, 3, F, 1000)


def test_describe_edges(L):
    assert L.describe_dot_attention(10, 10, 2, 8, 0) == {"form": "none"}
    assert L.describe_dot_attention(0, 0, 2, 8, 0) == {"form": "none"}
    assert L.describe_dot_attention(10, 10, 2, 0, 5) == {"route": "zeros"}
    assert L.describe_dot_attention(10, 10, 2, 513, 0) == {"route": "unsupported"}  # the entry points' order
    assert L.describe_dot_attention(10, 10, 1, 512, 5) == {"V": 4, "W": 64}
    buf = ctypes.create_string_buffer(4)
    assert L.lib.gespmm_describe_dot_attention(10, 10, 2, 64, 5, 16, 16, 16, buf, 4) == 3 and buf.value == b"V=4"
    assert L.lib.gespmm_describe_dot_attention(10, 10, 2, 64, 5, 16, 16, 16, None, 4) == EINVAL
    for bad, code in (((10, 10, 0, 8, 5), EINVAL), ((-1, 10, 2, 8, 5), EINVAL), ((0, 10, 2, 8, 5), EINVAL), ((10, 0, 2, 8, 5), EINVAL),
                      ((BIG, 10, 1, 1, 5), ERANGE), ((10, 10, 2, 8, BIG), ERANGE)):
        with pytest.raises(L.GespmmError) as e:
            L.describe_dot_attention(*bad)
        assert e.value.code == code, bad
    for al in ((2, 16, 16), (16, 12, 16), (16, 16, 0)):
        with pytest.raises(L.GespmmError) as e:
            L.describe_dot_attention(10, 10, 2, 8, 5, *al)
        assert e.value.code == EINVAL


def _operands(M=6, K=5, H=3, F=4, nnz=9):
    rp = torch.zeros(M + 1, dtype=torch.int32)
    rp[1:] = nnz
    cp = torch.zeros(K + 1, dtype=torch.int32)
    cp[1:] = nnz
    ind = torch.zeros(nnz, dtype=torch.int32)
    return {"rp": rp, "cp": cp, "ind": ind, "q": torch.zeros(M, H, F), "k": torch.zeros(K, H, F), "v": torch.zeros(K, H, F),
            "stats": torch.zeros(M, H, 2), "out": torch.zeros(M, H, F), "go": torch.zeros(M, H, F), "delta": torch.zeros(M, H)}


def test_python_wrappers_raise_before_any_launch(pkg):
    """TypeError for the dtype of EVERY operand first, then ValueError for shapes, contiguity and devices. Every operand here lives on
    the host, so a call that got past its checks raises the device ValueError — which the well-formed call at the end does."""
    att = pkg.attention
    o = _operands()
    M, K, H, F, nnz = 6, 5, 3, 4, 9

    def fwd(**kw):
        a = dict(o, **kw)
        return att.dot_attention(a["rp"], a["ind"], a["q"], a["k"], a["v"], scale=a.get("scale"), dropout=a.get("dropout"),
                                 out=a.get("out_"), stats=a.get("stats_"))

    def bq(**kw):
        a = dict(o, **kw)
        return att.dot_attention_backward_q(a["rp"], a["ind"], a["q"], a["k"], a["v"], a["stats"], a["out"], a["go"], scale=a.get("scale"),
                                            dropout=a.get("dropout"))

    def bkv(**kw):
        a = dict(o, **kw)
        return att.dot_attention_backward_kv(a["cp"], a["ind"], a["q"], a["k"], a["v"], a["stats"], a["delta"], a["go"],
                                             scale=a.get("scale"), dropout=a.get("dropout"))

    seed = torch.zeros(2, dtype=torch.int32)
    for call, floats, ptr in ((fwd, ("q", "k", "v"), "rp"), (bq, ("q", "k", "v", "stats", "out", "go"), "rp"),
                              (bkv, ("q", "k", "v", "stats", "delta", "go"), "cp")):
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
            call(**{ptr: o[ptr][:-1], "v": o["v"].double()})
        for bad in ({"dropout": 0.5}, {"dropout": (0.5, seed.long())}, {"dropout": (0.5, [1, 2])}, {"dropout": (torch.tensor(0.5), seed)},
                    {"scale": torch.tensor(1.0)}, {"scale": "1"}):
            with pytest.raises(TypeError):
                call(**bad)
        for bad in ({ptr: o[ptr].view(1, -1)}, {ptr: o[ptr][:-1]}, {"ind": o["ind"].view(1, -1)},
                    {"ind": torch.zeros(2 * nnz, dtype=torch.int32)[::2]}, {"q": o["q"].view(M, -1)}, {"k": o["k"].view(K, -1)},
                    {"q": torch.zeros(M, 0, F), "k": torch.zeros(K, 0, F), "v": torch.zeros(K, 0, F)}, {"k": torch.zeros(K, H, F + 1)},
                    {"v": torch.zeros(K, H + 1, F)}, {"v": torch.zeros(K + 1, H, F)}, {"q": torch.zeros(M, H, 2 * F)[:, :, ::2]},
                    {"scale": float("nan")}, {"scale": float("inf")}, {"dropout": (1.0, seed)}, {"dropout": (-0.5, seed)},
                    {"dropout": (float("nan"), seed)}, {"dropout": (0.5, torch.zeros(3, dtype=torch.int32))}):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(ValueError):
            call()  # well formed, but on the host: the device check is the last one standing
    for bad in ({"out_": torch.zeros(M, H, F + 1)}, {"stats_": torch.zeros(M, H)}, {"stats_": torch.zeros(M, H, 2)}):
        with pytest.raises(ValueError):
            fwd(**bad)
    with pytest.raises(TypeError):
        fwd(out_=torch.zeros(M, H, F).double())
    for call, bad in ((bq, {"stats": torch.zeros(M, H)}), (bq, {"out": torch.zeros(M, H, F + 1)}), (bq, {"go": torch.zeros(M + 1, H, F)}),
                      (bkv, {"delta": torch.zeros(M, H, 1)}), (bkv, {"go": torch.zeros(K, H, F)}), (bkv, {"cp": o["rp"]})):
        with pytest.raises(ValueError):
            call(**bad)


def test_python_wrappers_name_the_limit(pkg):
    """F = 513: a GespmmError that names the limit, raised only once the operands are known to be well formed and on a device — so on
    the host the device check comes first; the error's class and message are checked directly."""
    e = pkg.attention.DotAttentionUnsupported(513, "gespmm_dot_attention_f32")
    assert isinstance(e, pkg._lib.GespmmError) and e.code == UNSUPPORTED and "512" in str(e) and "513" in str(e)
    with pytest.raises(pkg._lib.GespmmError) as err:
        pkg._lib.check(UNSUPPORTED, "gespmm_dot_attention_f32")
    assert "512" in str(err.value)


def test_layer_arguments(pkg):
    T = pkg.TransformerConv
    with pytest.raises(ValueError):
        T(4, 3, heads=0)
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            T(4, 3, dropout=p)
    with pytest.raises(ValueError):
        T(4, 3, beta=True, root_weight=False)
    with pytest.raises(ValueError):
        T(4, 513, fused=True)
    with pytest.raises(TypeError):
        T(4, 3, dropout=0.5, attn_seed=torch.zeros(2, dtype=torch.int64))
    T(4, 513, fused=False)   # the composition serves any F
    T(4, 512, fused=True)
    full = T(4, 3, heads=2, beta=True)
    names = sorted(n for n, _ in full.named_parameters())
    assert names == ["lin_beta.weight", "lin_key.bias", "lin_key.weight", "lin_query.bias", "lin_query.weight", "lin_skip.bias",
                     "lin_skip.weight", "lin_value.bias", "lin_value.weight"]
    assert tuple(full.lin_beta.weight.shape) == (1, 18) and tuple(full.lin_skip.weight.shape) == (6, 4)
    mean = T(4, 3, heads=2, concat=False, beta=True, bias=False)
    assert tuple(mean.lin_beta.weight.shape) == (1, 9) and tuple(mean.lin_skip.weight.shape) == (3, 4) and mean.lin_key.bias is None
    bare = T(4, 3, heads=2, root_weight=False)
    assert bare.lin_skip is None and bare.lin_beta is None and not bare.fused
    with pytest.raises(ValueError):  # not square
        bare(torch.zeros(5, 4), torch.zeros(7, dtype=torch.int32), None, torch.zeros(6, dtype=torch.int32), None, None)


# ------------------------------------------------------------------------------------------- the restatement against float64

@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("F", FS)
def test_restatement_within_the_derived_tolerance(F, H):
    """Both forms of exp, V as an aligned call has it, on the GPU tests' inputs: worst error / tolerance <= 1 in every result."""
    for name in ("hand", "random"):
        P, x = pattern(name), inputs(name, H, F)
        V, W = geometry(F)
        for mode in ("exp2", "exp"):
            got, _, _ = restate_all(P, x, V, W, mode)
            r = check_all(P, x, got, what="%s F=%d H=%d %s" % (name, F, H, mode))
            assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("F,align", ((8, 4), (8, 8), (20, 8), (100, 4), (512, 8)))
def test_restatement_at_other_vector_widths(F, align):
    P, x = pattern("hand"), inputs("hand", 3, F)
    V, W = geometry(F, align)
    got, _, _ = restate_all(P, x, V, W)
    r = check_all(P, x, got, what="hand F=%d H=3 V=%d" % (F, V))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("p", (0.25, 0.6))
@pytest.mark.parametrize("F,H", ((3, 3), (32, 4), (100, 1)))
def test_restatement_with_dropout(F, H, p):
    P, x = pattern("hand"), inputs("hand", H, F)
    V, W = geometry(F)
    got, keep, ks = restate_all(P, x, V, W, p=p)
    r = check_all(P, x, got, keep, ks, what="hand F=%d H=%d p=%g" % (F, H, p))
    assert max(r.values()) <= 1.0, r
    kept = seg_sum(keep.astype(F64), P["rowptr"])
    dead = (kept == 0) & (P["degs"] > 0)[:, None]
    assert dead.any() and np.all(got["out"][dead] == 0) and not np.signbit(got["out"][dead]).any()  # all dropped: exactly +0
    assert 0.5 * (1 - p) < keep.mean() < min(1.0, 1.5 * (1 - p))


def witness_ratios(P, x):
    """Per result: the least, over the entries of rows with d >= 2 and the heads, of (largest change of a word by skipping the entry /
    that word's tolerance) — float64, closed form (the docstring of test_witness_every_entry_shows)."""
    f = ref_forward(P, x)
    stats64 = np.stack((f["m"], f["l"]), -1)
    b = ref_backward(P, x, stats64, f["out"])
    rows, cols = P["rows"], P["colind"]
    k, v, go = (x[n].astype(F64) for n in ("k", "v", "go"))
    scale = F64(F32(x["scale"]))
    multi = (P["degs"] >= 2)[rows]
    a = f["a"][..., None]
    one = np.where(multi[:, None, None], 1.0 - a, 1.0)
    out_s = (f["out"][rows] - a * v[cols]) / one
    worst = {}
    worst["out"] = (np.abs(out_s - f["out"][rows]) / f["tol_out"][rows]).max(-1)[multi].min()
    A = seg_sum((f["a"] * b["g"])[..., None] * k[cols], P["rowptr"])
    B = seg_sum(a * k[cols], P["rowptr"])
    delta_s = (go[rows] * out_s).sum(-1)[..., None]
    gq_s = scale * ((A[rows] - a * b["g"][..., None] * k[cols]) - delta_s * (B[rows] - a * k[cols])) / one
    worst["grad_q"] = (np.abs(gq_s - b["grad_q"][rows]) / b["tol_grad_q"][rows]).max(-1)[multi].min()
    worst["grad_k"] = (np.abs(b["contrib_k"]) / b["tol_grad_k"][cols]).max(-1)[multi].min()
    worst["grad_v"] = (np.abs(b["contrib_v"]) / b["tol_grad_v"][cols]).max(-1)[multi].min()
    return {k_: float(v_) for k_, v_ in worst.items()}


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("F", FS)
def test_witness_every_entry_shows(F, H):
    """On the very inputs the GPU tests use: a walk that skips ANY single entry of a segment with d >= 2 lands outside the tolerance.
    For a skipped entry j of a row, in float64 and closed form (a'_p = a_p / (1 - a_j)):
        out'    = (out - a_j v_j) / (1 - a_j)
        grad_q' = scale [(A - a_j g_j k_j) - delta' (B - a_j k_j)] / (1 - a_j),   A = sum a_p g_p k_p, B = sum a_p k_p, delta' = <go, out'>
    and grad_k and grad_v, at the entry's column, lose that entry's contribution (the entry of a single-entry row has ds_p = 0 by
    construction: nothing can show it in grad_k, which is why the condition is about rows with d >= 2). The restatement itself stays within 0.25 of
    the tolerance on these inputs (asserted here), so a restatement with the skip is further than the tolerance from the float64
    result wherever the float64 results with and without the skip differ by more than 1.25 tolerances — in at least one word of the
    segment's slice, for every head."""
    for name in ("hand", "random"):
        P, x = pattern(name), inputs(name, H, F)
        V, W = geometry(F)
        got, _, _ = restate_all(P, x, V, W)
        assert max(check_all(P, x, got, what="%s F=%d H=%d" % (name, F, H)).values()) <= 0.25
        worst = witness_ratios(P, x)
        print("%s F=%d H=%d least (change by a skipped entry / tolerance): %s" % (name, F, H, "  ".join("%s %.3g" % kv for kv in worst.items())))
        assert min(worst.values()) > 1.25, worst


# ------------------------------------------------------------------------------------------------------------ special shapes

def _chain_case(scores, F=4):
    """One row whose entry p has exactly the score scores[p]: q = (1, 0, ..), k[p] = (scores[p], ..), scale 1."""
    d = len(scores)
    rng = np.random.RandomState(3)
    P = {"M": 3, "K": d, "nnz": d, "rowptr": np.array([0, 0, d, d], dtype=np.int32), "colind": np.arange(d, dtype=np.int32),
         "rows": np.full(d, 1, dtype=np.int32), "degs": np.array([0, d, 0])}
    q = np.zeros((3, 1, F), F32)
    q[:, 0, 0] = 1
    k = rng.uniform(-1, 1, size=(d, 1, F)).astype(F32)
    k[:, 0, 0] = np.asarray(scores, dtype=F32)
    return P, {"q": q, "k": k, "v": rng.uniform(0.5, 1, size=(d, 1, F)).astype(F32), "scale": 1.0}


def test_special_shapes_exact():
    V, W = 4, 4
    # a single entry: out == v[c] bit for bit, stats == (s, 1); the rows around it are empty: +0 everywhere
    P, x = _chain_case([0.37])
    out, stats = restate_forward(P, x, V, W)
    assert out[1].tobytes() == x["v"][0].tobytes() and stats[1, 0, 0] == F32(0.37) and stats[1, 0, 1] == 1.0
    assert not out[[0, 2]].any() and not stats[[0, 2]].any() and not np.signbit(out[[0, 2]]).any() and not np.signbit(stats[[0, 2]]).any()
    # ascending scores: a rescale at every entry after the first; descending: none — both inside the tolerance
    up = np.linspace(-3, 3, 40)
    for scores, want in ((up, 39), (up[::-1], 0)):
        P, x = _chain_case(scores)
        for mode in ("exp2", "exp"):
            out, stats, n = restate_forward(P, x, V, W, mode, count_rescales=True)
            assert int(n[1, 0]) == want
            f = ref_forward(P, x)
            assert ratio(out, f["out"], f["tol_out"]) <= 1.0 and ratio(stats[..., 1], f["l"], f["tol_l"]) <= 1.0
            assert stats[1, 0, 0] == F32(3.0)
    # scores over +-80: t underflows to 0 for most entries and nothing is NaN
    P, x = _chain_case([-80.0, 80.0, -79.0, 0.0, 79.5, -80.0])
    for mode in ("exp2", "exp"):
        out, stats = restate_forward(P, x, V, W, mode)
        assert np.isfinite(out).all() and np.isfinite(stats).all() and stats[1, 0, 0] == F32(80.0)
        f = ref_forward(P, x)
        assert ratio(out, f["out"], f["tol_out"]) <= 1.0
        assert expf(F32(-160.0), mode) == 0.0


def test_lane_dot_is_the_pinned_order():
    """F = 5, V = 1, W = 4: lane 0 owns j = 0 and 4, lanes 1 .. 3 one word each; the butterfly adds (0 + 2) + (1 + 3). Exact integers."""
    x = np.array([1, 2, 3, 4, 5], dtype=F32)
    y = np.array([1, 10, 100, 1000, 10000], dtype=F32)
    assert lane_dot(x, y, 1, 4) == F32(54321)
    big = np.array([2.0 ** 24, 1.0, -2.0 ** 24, 1.0], dtype=F32)
    ones = np.ones(4, F32)
    assert lane_dot(big, ones, 1, 4) == F32(2.0)   # lanes (0 + 2) + (1 + 3): a left-to-right chain would give 1
    assert lane_dot(big, ones, 4, 4) == F32(1.0)   # V = 4: ONE lane runs the chain ((2^24 + 1) - 2^24) + 1
