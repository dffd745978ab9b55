"""Seeded cases, integer data and exact references of the aggregate-and-linear family (plain module beside helpers.py; shared by
test_linear_fuzz_host.py, which checks all of it without a device, and test_gpu_linear_fuzz.py):

    linear   spmm.csr_spmm_linear                  fp16 / bf16     spmm_linear.hip
    rel      spmm.csr_spmm_relational_linear       fp16 / bf16     spmm_relational.hip
    f32      spmm.csr_spmm_relational_linear       fp32            spmm_relational_f32.hip
    wgrad    spmm.csr_spmm_relational_weight_grad  fp16 / bf16     spmm_relational_wgrad.hip

A case is a shape, a stacked CSR and integer operands; the tests run it on every dtype of its op, valued and unweighted. The widths of
case i are NOT drawn: its lane geometry is i modulo the op's geometry list and its accumulator count NS follows the next digit of i, so
a case list reaches every template instance by construction (``reach`` restates the four launch_*_geometry functions); K and N_out then
cycle through the values of that class. Sizes, degrees, relation law, operand switches and data come from the seeded generator.

Exact mode. X, root, W, grad_out in {-1, 0, 1} (W, grad_out: at most four non-zeros per output column; root_weight: two), edge values
in {1, 2}, row_scale in {0.5, 1, 2}, bias in -3 .. 3. Every H_r element and every output element is then a multiple of g = 1/2 (g = 1
without row_scale). An output row is exact-eligible when, counted in units of g, the absolute-value sum of every element of its H_r
rows (before and after the scale) and of every element of the row itself is at most LIMIT = 256 (bf16) / 2048 (fp16) / 2^24 (fp32): an
integer of that size has a significand of 8 / 11 / 24 bits, so every partial sum in any order and every 16-bit rounding is exact and the
kernel must return the reference's value, word for word. (Counting in units of g is stricter than counting in units of 1: 255.5 is below
256 and is not a bf16 number.) For the weight gradient eligibility is per element of grad_W, and asks the same of every H_r row that the
element's column of grad_out names. Everything else goes by test_gpu_spmm_linear._within with the n its docstrings derive."""
import numpy as np

MS = (1, 2, 63, 64, 65, 128, 129, 300)
KNS = (1, 5, 64, 333)
RS = (1, 2, 3, 7, 17)
LAWS = ("uniform", "one empty relation", "live only in the last block", "block with no entry", "only relation R-1 live", "nnz = 0")
HUB = 2049
BLOCK = 64
K16 = (8, 16, 24, 32, 40, 64, 72, 120, 128, 136, 248, 256)
K32 = (4, 12, 16, 20, 28, 32, 36, 60, 64, 68, 124, 128, 132, 252, 256)
NOUTS = (1, 31, 32, 33, 34, 36, 47, 64, 65, 96, 97, 128, 129, 160, 161, 255, 256)
LIMIT = {"bf16": 256, "fp16": 2048, "fp32": 1 << 24}
DTYPES = {"linear": ("fp16", "bf16"), "rel": ("fp16", "bf16"), "f32": ("fp32",), "wgrad": ("fp16", "bf16")}
OPS = tuple(DTYPES)
SEEDS = {"linear": 20261101, "rel": 20261102, "f32": 20261103, "wgrad": 20261104}
N_CASES = 24
UNSERVED = ("K", "N_out", "offset")
OPERANDS = {"linear": ("X", "W", "root", "root_weight", "out"), "rel": ("X", "W", "root", "root_weight", "out"),
            "f32": ("X", "W", "root", "root_weight", "out"), "wgrad": ("X", "grad_out", "out")}


# ---- the launch rules, restated (spmm_linear.hip, spmm_relational.hip, spmm_relational_wgrad.hip, spmm_relational_f32.hip) ----------

def lanes_x16(K):
    """(W, words per lane) of launch_linear_geometry / launch_relational_geometry."""
    Kw = K // 2
    for bound, geo in ((64, (64, 2)), (32, (64, 1)), (16, (32, 1)), (8, (16, 1)), (4, (8, 1))):
        if Kw > bound:
            return geo
    return (4, 1)


def lanes_wgrad(K):
    """W of launch_wgrad_geometry: by the words of the widest 64-column slab."""
    Sw = min(K, 64) // 2
    return 32 if Sw > 16 else 16 if Sw > 8 else 8 if Sw > 4 else 4


def lanes_f32(K):
    """W of launch_relational_f32_geometry: by the float4 vectors of a row."""
    Kv = K // 4
    return 64 if Kv > 32 else 32 if Kv > 16 else 16 if Kv > 8 else 8 if Kv > 4 else 4


def ns_of(N_out):
    return 2 if N_out > 128 else 1


def stage_width(N_out):
    """V of wg_stage_grad_out."""
    return 8 if N_out % 8 == 0 else 4 if N_out % 4 == 0 else 2 if N_out % 2 == 0 else 1


def slab_widths(K):
    """SW of every 64-column slab of the weight gradient; SW > 32 is its ``two``."""
    return [min(64, K - k0) for k0 in range(0, K, 64)]


def wgrad_chunks(R, M, K, N_out):
    """spmm_relational_wgrad_chunks (spmm_relational_wgrad.h), restated."""
    if 0 in (R, M, K, N_out):
        return 0
    slabs = (K + 63) // 64
    C = min((1024 + R * slabs - 1) // (R * slabs), (M + 63) // 64, M // (4 * N_out))
    return max(C, 1)


def chunk_list(R, M, K, N_out):
    """The chunk counts a weight-gradient case runs: 1, ceil(M / 64), the default and one value in between (None: the default)."""
    blocks = (M + 63) // 64
    return [None] + sorted({1, blocks, (1 + blocks) // 2})


def f32_pad(K):
    """(the zero-pad rule ``4 l == K && K < K_pad`` fires, its lane is the last of the group: l == W - 1)"""
    on = K % 8 == 4
    return on, on and K // 4 == lanes_f32(K) - 1


def served(op, K, N_out):
    if op == "f32":
        return K % 4 == 0 and 4 <= K <= 256 and 1 <= N_out <= 256
    return K % 8 == 0 and 8 <= K <= 256 and 1 <= N_out <= 256


def reach(op, case, valued, dtype):
    """The template instance (as a tuple) that ``case`` launches on ``dtype``, valued or not."""
    K, N = case["K"], case["N_out"]
    if op == "linear":
        return (dtype, valued) + lanes_x16(K)
    if op == "rel":
        return (dtype, valued) + lanes_x16(K) + (ns_of(N),)
    if op == "wgrad":
        return (dtype, valued, lanes_wgrad(K), ns_of(N))
    return (valued, lanes_f32(K), ns_of(N))


GEOMETRIES = {  # the K values of every lane geometry, in the order the cases cycle through
    "linear": ((8,), (16,), (24, 32), (40, 64), (72, 120, 128), (136, 248, 256)),
    "rel": ((8,), (16,), (24, 32), (40, 64), (72, 120, 128), (136, 248, 256)),
    "wgrad": ((8,), (16,), (24, 32), (40, 64, 72, 120), (128, 136), (248, 256)),  # the last three are all W = 32
    "f32": ((4, 12, 16), (20, 28, 32), (36, 60, 64), (68, 124, 128), (132, 252, 256)),
}
NOUT_BY_NS = {1: tuple(n for n in NOUTS if n <= 128), 2: tuple(n for n in NOUTS if n > 128)}


# ---- graphs --------------------------------------------------------------------------------------------------------------------------

def _degrees(rng, rows, W, mean):
    """Degrees of ``rows`` stacked rows: a few per row around ``mean``, with rows on both sides of the walk's edges (0, 1, W, W + 1, 8, 9)."""
    degs = rng.randint(0, 2 * mean + 1, size=rows)
    edges = (0, 1, W, W + 1, 8, 9)
    at = rng.choice(rows, size=min(rows, len(edges)), replace=False)
    for a, d in zip(at, rng.permutation(edges)):
        degs[a] = d
    return degs.astype(np.int64)


def _apply_law(rng, degs, law, R, M):
    """Zero the (relation, row) degrees the law empties; make every (block, relation) pair it keeps hold an entry."""
    d = degs.reshape(R, M).copy()
    blocks = (M + BLOCK - 1) // BLOCK
    live = np.ones((R, blocks), dtype=bool)
    if law == "one empty relation":
        live[rng.randint(R)] = False
    elif law == "live only in the last block":
        live[rng.randint(R), :blocks - 1] = False
    elif law == "block with no entry":
        live[:, rng.randint(blocks)] = False
    elif law == "only relation R-1 live":
        live[:R - 1] = False
    elif law == "nnz = 0":
        live[:] = False
    for r in range(R):
        for b in range(blocks):
            rows = slice(b * BLOCK, min((b + 1) * BLOCK, M))
            if not live[r, b]:
                d[r, rows] = 0
            elif not d[r, rows].any():
                d[r, rng.randint(rows.start, rows.stop)] = 1
    return d.reshape(-1), live


def stacked_csr(degs, cols, R, M, Kn):
    """The stacked CSR of (relation, row, column) triples through graphs.coo_to_csr, as the ops' docstrings build it."""
    from gespmm_amd import graphs

    rows = np.repeat(np.arange(R * M), degs)
    rp, ci, _ = graphs.coo_to_csr(R * M, Kn, rows, cols)
    return np.ascontiguousarray(rp), np.ascontiguousarray(ci)


def stacked_csc(case):
    """(colptr, rowind, order) of graphs.transpose_stacked_csr(..., return_order=True), as numpy arrays."""
    import torch

    from gespmm_amd import graphs

    cp, ri, order = graphs.transpose_stacked_csr(torch.from_numpy(case["rowptr"]), torch.from_numpy(case["colind"]), case["R"], case["Kn"],
                                                 return_order=True)
    return cp.numpy(), ri.numpy(), order.numpy()


# ---- cases ---------------------------------------------------------------------------------------------------------------------------

def _sparse_columns(rng, cols, span, count, shape):
    """[cols, span] in {-1, 0, 1} with at most ``count`` non-zeros per row of the result (an output column)."""
    t = np.zeros((cols, span), dtype=np.float64)
    pos = rng.randint(0, span, size=(cols, count))
    t[np.arange(cols)[:, None], pos] = rng.choice([-1.0, 1.0], size=(cols, count))
    return t.reshape(shape)


def draw_case(op, index, rng, unserved=None):
    geos = GEOMETRIES[op]
    ks = geos[index % len(geos)]
    K = ks[(index // len(geos)) % len(ks)]
    ns = 1 + (index // len(geos)) % 2
    nouts = NOUT_BY_NS[ns]
    N_out = nouts[(index // (2 * len(geos)) * len(geos) + index % len(geos)) % len(nouts)]
    # the law walks through every geometry: index + index // 6 where the geometry list has six entries too, plain index beside five
    law = LAWS[(index + (index // len(LAWS) if len(geos) == len(LAWS) else 0)) % len(LAWS)] if unserved is None else "uniform"
    M, Kn = int(rng.choice(MS)), int(rng.choice(KNS))
    R = 1 if op == "linear" else int(rng.choice(RS))
    if law in ("one empty relation", "only relation R-1 live") and R == 1 and op != "linear":
        R = int(rng.choice(RS[1:]))
    if law in ("live only in the last block", "block with no entry") and M <= BLOCK:
        M = int(rng.choice([m for m in MS if m > BLOCK]))
    if unserved == "K":
        K += 1 if op == "f32" else 2
    if unserved == "N_out":
        N_out = 257
    W = lanes_f32(K) if op == "f32" else lanes_wgrad(K) if op == "wgrad" else lanes_x16(K)[0]
    mean = int(rng.choice((1, 3, 6)))
    degs, live = _apply_law(rng, _degrees(rng, R * M, W, mean), law, R, M)
    if unserved is None and index % 5 == 2 and degs.any():  # one hub of 2049 entries, in a row the law left live
        degs[rng.choice(np.flatnonzero(degs))] = HUB
    cols = rng.randint(0, Kn, size=int(degs.sum()))
    rowptr, colind = stacked_csr(degs, cols, R, M, Kn)
    nnz = int(colind.shape[0])
    case = {"op": op, "index": index, "law": law, "unserved": unserved, "M": M, "Kn": Kn, "K": K, "N_out": N_out, "R": R, "nnz": nnz,
            "rowptr": rowptr, "colind": colind, "live": live,
            "values": rng.randint(1, 3, size=nnz).astype(np.float64),
            "row_scale": rng.choice([0.5, 1.0, 2.0], size=R * M) if rng.randint(3) else None,
            "X": rng.randint(-1, 2, size=(Kn, K)).astype(np.float64),
            "offsets": {name: 16 * int(rng.randint(2)) for name in OPERANDS[op]}}
    if unserved == "offset":
        case["offsets"]["X"] = 4 if op == "f32" else 2
    if op == "wgrad":
        case["grad_out"] = _sparse_columns(rng, N_out, M, 4, (N_out, M)).T.copy()
    else:
        case["W"] = _sparse_columns(rng, N_out, R * K, 4, (N_out, R, K)).transpose(1, 0, 2).copy()
        has_root = bool(rng.randint(4))
        case["root"] = rng.randint(-1, 2, size=(M, K)).astype(np.float64) if has_root else None
        case["root_weight"] = _sparse_columns(rng, N_out, K, 2, (N_out, K)) if has_root else None
        case["bias"] = rng.randint(-3, 4, size=N_out).astype(np.float64) if rng.randint(4) else None
    return case


_CACHE = {}


def cases(op):
    """The op's fixed case list: N_CASES served cases and two of every unserved variant."""
    if op not in _CACHE:
        rng = np.random.RandomState(SEEDS[op])
        n = N_CASES + (1 if op == "f32" else 0)  # 25 = 5 geometries x 5
        out = [draw_case(op, i, rng) for i in range(n)]
        out += [draw_case(op, i, rng, unserved=u) for u in UNSERVED for i in (1, 9)]
        _CACHE[op] = out
    return _CACHE[op]


def case_id(case):
    tag = case["law"] if case["unserved"] is None else "unserved " + case["unserved"]
    return "%s%d-M%d-Kn%d-K%d-N%d-R%d-%s" % (case["op"], case["index"], case["M"], case["Kn"], case["K"], case["N_out"], case["R"],
                                             tag.replace(" ", "_"))


# ---- exact references ----------------------------------------------------------------------------------------------------------------

def dense_relations(case, valued, drop=None):
    """(A, |A|) as float64 [R M, Kn] from the stacked CSR arrays alone (small integers: exact). ``drop``: leave out that CSR entry."""
    rp, ci = case["rowptr"], case["colind"]
    rows = np.repeat(np.arange(rp.shape[0] - 1), np.diff(rp))
    v = case["values"].copy() if valued else np.ones(ci.shape[0])
    if drop is not None:
        v[drop] = 0.0
    A = np.zeros((rp.shape[0] - 1, case["Kn"]))
    np.add.at(A, (rows, ci), v)
    return A


def aggregates(case, valued, drop=None):
    """(H, Habs): [R, M, K] float64, the exact aggregate with its scale, and the larger of the absolute-value sums before and after it."""
    A = dense_relations(case, valued, drop)
    H, Habs = A @ case["X"], A @ np.abs(case["X"])
    if case["row_scale"] is not None:
        s = case["row_scale"][:, None]
        H, Habs = H * s, np.maximum(Habs, Habs * s)
    shape = (case["R"], case["M"], case["K"])
    return H.reshape(shape), Habs.reshape(shape)


def grid(case):
    return case.get("grid", 0.5 if case["row_scale"] is not None else 1.0)


def forward_ref(case, valued, drop=None, weight=None, root_rows=None):
    """(ref [M, N_out] float64, eligible-row test by dtype name -> bool [M], H, the absolute-value sums S [M, N_out]). ``weight``: in
    place of the case's W; ``root_rows``: bool [M], the rows that keep their root term (None: all)."""
    H, Habs = aggregates(case, valued, drop)
    W = case["W"] if weight is None else weight
    R, M, K = H.shape
    side = lambda t: t.transpose(1, 0, 2).reshape(t.shape[1], R * K)  # noqa: E731  (the relations side by side: [., R K])
    ref = side(H) @ side(W).T
    S = side(Habs) @ np.abs(side(W)).T
    if case["root"] is not None:
        term = case["root"] @ case["root_weight"].T
        ref = ref + (term if root_rows is None else term * root_rows[:, None])
        S = S + np.abs(case["root"]) @ np.abs(case["root_weight"]).T
    if case["bias"] is not None:
        ref, S = ref + case["bias"], S + np.abs(case["bias"])
    g = grid(case)
    worst = np.maximum(Habs.max(axis=(0, 2)), S.max(axis=1)) / g

    def eligible(dtype):
        return worst <= LIMIT[dtype]

    return ref, eligible, H, S


def wgrad_ref(case, valued, drop=None):
    """(ref [R, N_out, K] float64, eligible-element test by dtype name -> bool [R, N_out, K], H, S)."""
    H, Habs = aggregates(case, valued, drop)
    go = case["grad_out"]
    ref = np.matmul(go.T[None], H)
    S = np.matmul(np.abs(go).T[None], Habs)
    g = grid(case)
    named = (np.abs(go)[None, :, :] * Habs.max(axis=2)[:, :, None]).max(axis=1)  # [R, N_out]: the largest H_r row a column names

    def eligible(dtype):
        return (S / g <= LIMIT[dtype]) & (named[:, :, None] / g <= LIMIT[dtype])

    return ref, eligible, H, S


def as_int64(ref, case):
    """The reference in units of the case's grid as int64 — it IS an integer there, which is what makes the comparison exact."""
    scaled = ref / grid(case)
    out = np.rint(scaled).astype(np.int64)
    assert np.array_equal(out.astype(np.float64), scaled), "the reference left its grid"
    return out


def reference(case, valued, **mutation):
    return wgrad_ref(case, valued, **mutation) if case["op"] == "wgrad" else forward_ref(case, valued, **mutation)


def agrees(case, got, ref, eligible, bounded=None):
    """The comparison of the tests: ``got`` (float64 array of the result's shape) equals ``ref`` wherever ``eligible``; everything else is
    handed to ``bounded(mask)`` (None: nothing else is checked here). The reference is an int64 in units of the grid."""
    want = as_int64(ref, case)[eligible].astype(np.float64) * grid(case)
    ok = bool(np.array_equal(got[eligible], want))  # (a NaN equals nothing)
    if bounded is not None and not eligible.all():
        ok = bounded(~eligible) and ok
    return ok


def broadcast_rows(elig, shape):
    return np.broadcast_to(elig[:, None], shape) if elig.ndim == 1 else elig


# ---- mutations of the reference: what a subtly wrong kernel would return --------------------------------------------------------------

def skipped_blocks(case):
    """bool [M]: rows of the blocks in which some relation has no entry (the kernel skips that (block, relation) pair)."""
    skip = ~case["live"].all(axis=0)
    return np.repeat(skip, BLOCK)[:case["M"]]


def mutants(case, valued):
    """{name: mutated reference} — the mutations that apply to this case (``test_linear_fuzz_host.py`` rejects each on some case)."""
    op, out = case["op"], {}
    ref = reference(case, valued)[0]
    if case["nnz"]:
        out["dropping one CSR entry"] = reference(case, valued, drop=case["nnz"] // 2)[0]
    if min(ref.shape[-2:]) >= 32:
        t = ref.copy()
        t[..., :32, :32] = np.swapaxes(ref[..., :32, :32], -1, -2)
        out["transposing a 32 x 32 fragment"] = t
    half = 4 if op == "f32" else 8
    if case["K"] % (2 * half) == 0:
        perm = np.arange(case["K"]) ^ half
        if op == "wgrad":
            out["exchanging the two k-halves"] = ref[:, :, perm]
        else:
            out["exchanging the two k-halves"] = forward_ref(case, valued, weight=case["W"][:, :, perm])[0]
    if case["R"] >= 2:
        if op == "wgrad":
            out["swapping two relations' weights"] = ref[[1, 0] + list(range(2, case["R"]))]
        else:
            out["swapping two relations' weights"] = forward_ref(case, valued, weight=case["W"][[1, 0] + list(range(2, case["R"]))])[0]
    if op != "wgrad" and case["root"] is not None:
        out["dropping the skipped relation's root term"] = forward_ref(case, valued, root_rows=~skipped_blocks(case))[0]
    return out
