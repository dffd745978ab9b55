"""Host checks behind test_gpu_large_operands.py and the H = 17 cases of test_gpu_large_edges.py (no device).

* Sizes: every case's (M, K) from tests/large_operands.py; "below" and "at" lie on the two sides of each route switch, as the
  host-only route functions and the entries themselves (called with null pointers) answer; regime B is the largest size the
  entries accept and one row more is refused.
* Windows: the compared windows — and, for the float ops, the 512-row sub-patterns inside them — hold the rows with byte 2^31, byte
  2^32 and the last word of every operand of every case.
* Each comparison can fail: for every marked window the reference is recomputed with the gathered operand read through a byte
  offset displaced by 2^32 and by 2^31 (modulo 2^32; at 1200-byte rows the alias lies inside another row, at another head and
  feature) and the case's comparator must reject it — exact equality for the integer ops, the op's own tolerance for the float ops
  (there the alias holds another draw of the random values). This is a requirement on the INPUTS: a value and its aliases differ.
* Section c of the GPU module (the fused GATv2 attention; the GATv2 score on 16-bit operands, limits counted in elements): the sizes
  on both sides of the limit through the same null-pointer calls, the windows marked at element size 2, byte 2^31 inside and byte
  2^32 just outside every 16-bit operand, and the float comparators against a reference read through a displaced position, here
  with node values that are a function of the GLOBAL word position (another value at every alias, as in an array of random values).
* The band at d = 8 against a numpy transpose."""
import numpy as np
import pytest
import torch

import band
import large_operands as lo
from test_large_edges_host import _numpy_transpose

EINVAL, ERANGE = -1, -3
D = lo.D
CASES_A = [(H, F, elem, side, walk) for H, F in lo.WIDTHS for elem in (4, 2) for side in ("below", "at") for walk in ("rows", "cols")]
CASES_B = [(H, F, regime) for H, F in lo.WIDTHS for regime in ("A", "B")]


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


# ---- sizes and routes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,F,elem,side,walk", CASES_A)
def test_below_and_at_lie_on_the_two_sides_of_the_switch(L, H, F, elem, side, walk):
    N = H * F
    M, K = lo.sizes_a(N, side, walk, elem)
    assert K == M + lo.LAST == band.sizes(M, D)[1]
    nnz, below = M * D, side == "below"
    gathered = K if walk == "rows" else M
    assert (gathered * N * elem < (1 << 32)) == below and ((gathered + 1) * N * elem >= (1 << 32)) and (gathered - 1) * N * elem < (1 << 32)
    S, T = (M, K) if walk == "rows" else (K, M)  # segments, rows of the gathered operand
    if elem == 2:
        assert L.heads_x16_route(S, T, H, F, nnz)[0] == (1 if below else 0)
        assert L.heads_route(S, T, H, F, nnz)[0] == 0 or not below or N * T * 4 < (1 << 32)
        return
    assert L.heads_route(S, T, H, F, nnz)[0] == (1 if below else 0)
    assert L.gat_aggregate_route(M, K, H, F, nnz, transposed=walk == "cols")[0] == (1 if below else 0)
    if walk == "rows":  # the max reducer: no composition
        f, b = L.lib.gespmm_csr_spmm_max_arg_f32, L.lib.gespmm_csr_spmm_max_backward_f32
        assert f(*[None] * 5, M, K, N, nnz, -1e4, None) == (EINVAL if below else ERANGE)
        assert b(*[None] * 6, M, K, N, nnz, None) == (EINVAL if below else ERANGE)
        assert L.max_arg_route(M, nnz, N) is not None
        # ... and its 16-bit entries: the limit is the same one, counted in the 4-byte words of arg
        for code in (L.X16_BF16, L.X16_F16):
            assert L.lib.gespmm_csr_spmm_max_arg_x16(*[None] * 5, M, K, N, nnz, -1e4, code, None) == (EINVAL if below else ERANGE)
            assert L.lib.gespmm_csr_spmm_max_backward_x16(*[None] * 6, M, K, N, nnz, code, None) == (EINVAL if below else ERANGE)
        assert L.max_arg_route_x16(M, nnz, N) is not None and L.max_arg_route_x16(K, nnz, N) is not None


def _entries(L, H, F, slope=0.2):
    """name -> f(M, K): the return code of the entry on null pointers"""
    lib = L.lib
    return {
        "gatv2_score": lambda m, k: lib.gespmm_gatv2_score_f32(*[None] * 6, m, k, H, F, m * D, slope, None),
        "gatv2_backward_rows": lambda m, k: lib.gespmm_gatv2_score_backward_f32(*[None] * 9, m, k, H, F, m * D, slope, None),
        "gatv2_backward_cols": lambda m, k: lib.gespmm_gatv2_score_backward_f32(*[None] * 9, k, m, H, F, m * D, slope, None),
        "dot_attention": lambda m, k: lib.gespmm_dot_attention_f32(*[None] * 7, m, k, H, F, m * D, 0.5, None),
        "dot_attention_backward_q": lambda m, k: lib.gespmm_dot_attention_backward_q_f32(*[None] * 10, m, k, H, F, m * D, 0.5, None),
        "dot_attention_backward_kv": lambda m, k: lib.gespmm_dot_attention_backward_kv_f32(*[None] * 10, m, k, H, F, m * D, 0.5, None),
        "gat_backward_el": lambda m, k: lib.gespmm_gat_backward_el_f32(*[None] * 9, m, k, H, F, m * D, slope, None),
        "gat_backward_er": lambda m, k: lib.gespmm_gat_backward_er_f32(*[None] * 9, m, k, H, F, m * D, slope, None),
        "gatv2_attention": lambda m, k: lib.gespmm_gatv2_attention_f32(*[None] * 7, m, k, H, F, m * D, slope, None),
        "gatv2_attention_backward_row": lambda m, k: lib.gespmm_gatv2_attention_backward_row_f32(*[None] * 11, m, k, H, F, m * D, slope, None),
        "gatv2_attention_backward_col": lambda m, k: lib.gespmm_gatv2_attention_backward_col_f32(*[None] * 9, m, k, H, F, m * D, slope, None),
        # the 16-bit GATv2 score: the same limits, counted in ELEMENTS (the operands are half the bytes)
        "gatv2_score_bf16": lambda m, k: lib.gespmm_gatv2_score_x16(*[None] * 6, L.X16_BF16, m, k, H, F, m * D, slope, None),
        "gatv2_score_fp16": lambda m, k: lib.gespmm_gatv2_score_x16(*[None] * 6, L.X16_F16, m, k, H, F, m * D, slope, None),
        "gatv2_backward_rows_bf16": lambda m, k: lib.gespmm_gatv2_score_backward_x16(*[None] * 9, L.X16_BF16, m, k, H, F, m * D, slope, None),
        "gatv2_backward_cols_fp16": lambda m, k: lib.gespmm_gatv2_score_backward_x16(*[None] * 9, L.X16_F16, k, m, H, F, m * D, slope, None),
    }


@pytest.mark.parametrize("H,F,regime", CASES_B)
def test_regimes_of_the_word_position_kernels(L, H, F, regime):
    N = H * F
    M, K = lo.sizes_b(N, regime)
    assert K == M + lo.LAST and K * N > (1 << 30), "word 2^30 (byte 2^32) lies inside every K-side operand"
    assert M * N > (1 << 30) and K * N <= lo.MAX_WORDS
    if regime == "A":
        assert abs(M * N - lo.REGIME_A_ROWS_512 * 512) < N and 5.3e9 < M * N * 4 < 5.5e9
    for name, f in _entries(L, H, F).items():
        assert f(M, K) == EINVAL, (name, "sizes accepted: on to the pointers")
        if regime == "B":
            assert f(M, K + 1) == ERANGE, (name, "one row more of the K-side operands")
            assert f(K + 1 - lo.LAST, K + 1) == ERANGE, (name, "the band of one row more")
    # the routes of the GPU cases: one kernel each (H = 3 takes the ordinary routes too)
    nnz = M * D
    assert L.describe_dot_attention(M, K, H, F, nnz) == {"V": 4, "W": 8 if F == 64 else 16}
    assert L.describe_gatv2_score(M, nnz, H, F)["V"] == 4
    W = 8 if F == 64 else 16
    assert L.describe_gatv2_attention(M, K, H, F, nnz) == {"V": 4, "W": W, "supported": True}
    assert L.describe_gatv2_attention(M, K, H, F, nnz, 4, 4, 4) == {"V": 1, "W": W, "supported": True}  # every operand 4 bytes off
    # the 16-bit score: no lane order shared with fp32 on aligned operands at these widths; one (V, W) = (1, W) with att 4 bytes off
    x16 = L.describe_gatv2_score(M, nnz, H, F, x16=True)
    assert (x16["V"], x16["W"]) == ((8, 4) if F == 64 else (4, 8))
    off = [L.describe_gatv2_score(M, nnz, H, F, 16, 16, 4, x16=x) for x in (True, False)]
    assert [(d["V"], d["W"]) for d in off] == [(1, W), (1, W)]
    for csr in (True, False):
        for x16 in (False, True):
            assert L.describe_sddmm_heads(csr, M, nnz, H, F, x16=x16)["route"] == "kernel"
    if N == 512:
        assert L.describe_sddmm(True, M, nnz, N)["form"] == "csr-edge"


# ---- windows ------------------------------------------------------------------------------------------------------------------------

def _check_marks(M, K, N, elem, float_ops):
    rw, cw = lo.case_windows(M, K, N, elem)
    assert rw[0][0] == 0 and rw[-1][1] == M and cw[0][0] == 0 and cw[-1][1] == K and len(rw) >= 14 and len(cw) >= 14
    rb = N * elem
    few = lo.case_windows(M, K, N, elem, spread=2)[0]  # the float ops: the marked windows, the first and the last
    assert set(few) <= set(rw) and few[0][0] == 0 and few[-1][1] == M
    subs = [lo.sub_rows(w, M) for w in few]
    assert subs[0] == (0, lo.FLOAT_ROWS) and subs[-1] == (M - lo.FLOAT_ROWS, M)
    for rows, side in ((M, "M"), (K, "K")):
        marks = lo.marked(rows, N, elem)
        assert marks[-1] == rows - 1
        for b in lo.BYTES:
            if b < rows * rb:
                r = b // rb
                assert r in marks and r * rb <= b < (r + 1) * rb
                if rb == 1200:
                    assert r * rb < b, "the byte falls inside the row, not on its boundary"
        for m in marks:
            # an M-side row is compared in the row windows (its own result words) and gathered by the columns m .. m + 22;
            # a K-side row is compared in the column windows and gathered by the rows m - 22 .. m
            assert lo.holds(cw, m) and lo.holds(rw, min(m, M - 1)), (side, m)
            if float_ops:  # ... and the sub-pattern's rows r0 .. r1 hold it or gather it, and its complete columns hold it
                hit = [(r0, r1) for r0, r1 in subs if r0 <= min(m, M - 1) < r1]
                assert hit, (side, m)
                r0, r1 = hit[0]
                if side == "K" and m < K - 1:
                    f0, f1 = (0 if r0 == 0 else r0 + lo.LAST), (K if r1 == M else r1)
                    assert f0 <= m < f1, "a complete column of the sub-pattern"
    return rw, cw


@pytest.mark.parametrize("H,F,elem,side,walk", CASES_A)
def test_windows_hold_the_marked_rows_section_a(H, F, elem, side, walk):
    N = H * F
    M, K = lo.sizes_a(N, side, walk, elem)
    _check_marks(M, K, N, elem, False)
    if side == "below":  # the row straddling byte 2^31 of the gathered operand, and its last rows
        gathered = K if walk == "rows" else M
        assert (1 << 31) // (N * elem) in lo.marked(gathered, N, elem) and gathered - 1 in lo.marked(gathered, N, elem)


@pytest.mark.parametrize("H,F,regime", CASES_B)
def test_windows_hold_the_marked_rows_section_b(H, F, regime):
    N = H * F
    M, K = lo.sizes_b(N, regime)
    _check_marks(M, K, N, 4, True)
    assert {(1 << 29) // N, (1 << 30) // N} <= set(lo.marked(M, N)) and {(1 << 29) // N, (1 << 30) // N} <= set(lo.marked(K, N))
    _check_marks(M, K, N, 2, False)  # the bf16 SDDMM: byte 2^32 is word 2^31 of a 16-bit array


def test_windows_of_the_h17_edge_arrays():
    """test_gpu_large_edges.py at H = 17: the [nnz, 17] arrays lie between 2^30 and 2^31 words and the window of the added mark holds
    edge floor(2^30 / 17); take_edges at H = 16 has 2^30 + 16384 words in 64-byte rows."""
    M, d = (1 << 20) + 16, 64
    nnz = M * d
    assert (1 << 30) < nnz * 17 <= lo.MAX_WORDS and nnz * 16 == (1 << 30) + 16384
    e = (1 << 30) // 17
    starts = band.window_starts(M, (1024 // d, e // d))
    assert any(s <= e // d < s + band.WINDOW for s in starts)
    assert e * 17 <= (1 << 30) < (e + 1) * 17, "word 2^30 lies inside this edge's row of the array"


# ---- each comparison can fail: the reference through a displaced byte offset ---------------------------------------------------------

def _slices(M, K, N, elem, rows_of_operand, shift):
    """32-row slices of the marked windows at and after the rows whose aliases lie inside the operand"""
    rb = N * elem
    out = []
    for m in lo.marked(rows_of_operand, N, elem):
        if m * rb >= shift or (m + 1) * rb > shift:
            out.append(m)
    return out


def _gathered_rows(H, F, elem, side, walk):
    M, K = lo.sizes_a(H * F, side, walk, elem)
    return K if walk == "rows" else M


# (a displacement of 2^32 bytes has an alias inside the operand only past the switch: the "at" cases)
CASES_A_SHIFTED = [c + (shift,) for c in CASES_A for shift in lo.BYTES if _gathered_rows(*c) * c[0] * c[1] * c[2] > shift]


@pytest.mark.parametrize("H,F,elem,side,walk,shift", CASES_A_SHIFTED)
def test_integer_references_reject_a_displaced_gather_section_a(H, F, elem, side, walk, shift):
    """The heads product (fp32 and x16 element sizes), the fused aggregation (the same sum with unit weights) and the max reducer."""
    N = H * F
    M, K = lo.sizes_a(N, side, walk, elem)
    gathered = K if walk == "rows" else M
    assert gathered * N * elem > shift
    fn = lo.b_at(H, F) if walk == "rows" else lo.k_at(H, F)
    wrong = lo.displaced(fn, H, F, shift, gathered, elem)
    one = lambda e, h: 1  # noqa: E731
    for m in _slices(M, K, N, elem, gathered, shift):
        for weight_fn in (lo.w_nz, one):
            if walk == "rows":  # rows m - 22 .. m gather row m of the K-side operand
                r1 = min(m + 1, M)
                r0 = max(r1 - 32, 0)
                good = band.ref_csr_product(M, D, r0, r1, H, F, dense_fn=fn, weight_fn=weight_fn)
                bad = band.ref_csr_product(M, D, r0, r1, H, F, dense_fn=wrong, weight_fn=weight_fn)
            else:  # columns m .. m + 22 gather row m of the M-side operand
                c0 = m
                good = band.ref_csc_product(M, D, c0, c0 + 32, H, F, dense_fn=fn, weight_fn=weight_fn)
                bad = band.ref_csc_product(M, D, c0, c0 + 32, H, F, dense_fn=wrong, weight_fn=weight_fn)
            assert band.first_difference(good.to(torch.float32), bad.to(torch.float32)) is not None, (m, weight_fn)
        if walk == "rows" and elem == 4:  # the max: the values, or the first position that reaches them
            r1 = min(m + 1, M)
            r = torch.arange(max(r1 - 32, 0), r1).view(-1, 1, 1, 1)
            j = torch.arange(D).view(1, D, 1, 1)
            hh, ff = band._hf(H, F, "cpu")
            tops = []
            for f_ in (fn, wrong):
                vals = f_(r + band.offset_of(j), hh, ff)
                top = vals.max(1, keepdim=True).values
                tops.append((top, torch.where(vals == top, j, D).min(1).values))
            assert not (torch.equal(tops[0][0], tops[1][0]) and torch.equal(tops[0][1], tops[1][1])), m


@pytest.mark.parametrize("shift", lo.BYTES)
@pytest.mark.parametrize("x16", (False, True))
@pytest.mark.parametrize("H,F,regime", CASES_B + [(1, 512, "A"), (1, 512, "B")])
def test_integer_references_reject_a_displaced_gather_sddmm(H, F, regime, x16, shift):
    """The multi-head SDDMM and (H = 1, F = 512) the plain one: either operand read through the displaced offset."""
    N, elem = H * F, 2 if x16 else 4
    M, K = lo.sizes_b(N, regime)
    for side in ("q", "k"):
        rows = M if side == "q" else K
        if rows * N * elem <= shift:
            continue
        fns = {"q_fn": lo.b_at(H, F), "k_fn": lo.k_at(H, F)}
        wrong = lo.displaced(fns[side + "_fn"], H, F, shift, rows, elem)
        for m in _slices(M, K, N, elem, rows, shift):
            r1 = min(m + 1, M)
            r0 = max(r1 - 32, 0)
            good = band.ref_csr_scores(M, D, r0, r1, H, F, **fns)
            bad = band.ref_csr_scores(M, D, r0, r1, H, F, **dict(fns, **{side + "_fn": wrong}))
            assert band.first_difference(good.to(torch.float32), bad.to(torch.float32)) is not None, (side, m)


def test_the_closed_forms_differ_at_their_aliases():
    """What the rejections above rest on: lo.b_at and lo.k_at are functions of the word position modulo 7 and 5, and no displacement
    by 2^31 or 2^32 bytes — 2^29, 2^30 words, 2^30, 2^31 16-bit elements — is a multiple of either: EVERY word differs from its alias,
    at 2048-byte and at 1200-byte rows. band.b_of / band.k_of would do at 2048-byte rows (2^21 = 1, 2^20 = 4 mod 7; 3 2^21 = 1,
    3 2^20 = 3 mod 5); at 1200-byte rows a linear form of (r, h, f) can keep its value over whole bands of aliases."""
    assert [(1 << e) % 7 for e in (29, 30, 31)] == [4, 1, 2] and [(1 << e) % 5 for e in (29, 30, 31)] == [2, 4, 3]
    assert (1 << 21) % 7 == 1 and (1 << 20) % 7 == 4 and (3 << 21) % 5 == 1 and (3 << 20) % 5 == 3
    for H, F in lo.WIDTHS:
        N = H * F
        h, f = torch.arange(H).view(1, H, 1), torch.arange(F).view(1, 1, F)
        for elem in (4, 2):
            rows = lo.regime_rows(N, "B") * 4 // elem
            r = torch.arange(rows - 64, rows).view(-1, 1, 1)
            for fn in (lo.b_at(H, F), lo.k_at(H, F)):
                for shift in lo.BYTES:
                    assert bool((fn(r, h, f) != lo.displaced(fn, H, F, shift, rows, elem)(r, h, f)).all())


# ---- the float ops: a gathered row that holds another draw must fall outside the op's own tolerance ----------------------------------

def _float_case(H, F):
    """A 512-row sub-pattern's shape at small size: the band at d = 8 on 64 rows, random operands, and the same operands with ONE
    gathered row (K side: row 40; M side: row 30) holding another draw — what a displaced offset reads in an array of random values."""
    from test_dot_attention_host import transpose

    M = 64
    rowptr, colind = (t.numpy() for t in band.csr(M, D))
    K = M + lo.LAST
    colptr, rowind, order = transpose(rowptr, colind, K)
    rows = np.repeat(np.arange(M, dtype=np.int32), D)
    P = {"M": M, "K": K, "nnz": M * D, "rowptr": rowptr, "colind": colind, "colptr": colptr, "rowind": rowind, "order": order, "rows": rows,
         "degs": np.full(M, D)}
    rng = np.random.RandomState(100 * H + F)
    u = lambda shape, a, b: rng.uniform(a, b, size=shape).astype(np.float32)  # noqa: E731
    x = {"xm": u((M, H, F), -1, 1), "xk": u((K, H, F), -1, 1), "vk": u((K, H, F), -1, 1), "go": u((M, H, F), 0.5, 1), "att": u((H, F), -2, 2),
         "gs": u((M * D, H), -2, 2), "el": u((M, H), -2, 2), "er": u((K, H), -2, 2)}
    other = {k: v.copy() for k, v in x.items()}
    for name, row in (("xk", 40), ("vk", 40), ("xm", 30), ("go", 30)):
        other[name][row] = u(x[name][row].shape, *((0.5, 1) if name == "go" else (-1, 1)))
    return P, x, other


@pytest.mark.parametrize("H,F", lo.WIDTHS)
def test_float_comparators_reject_a_displaced_gather(H, F):
    from attention_refs import bound_ratio, gat_backward_float64
    from test_dot_attention_host import ratio, ref_backward, ref_forward
    from test_gatv2_host import restate_backward, restate_score, worst_ratio

    P, x, o = _float_case(H, F)
    f32 = lambda a: np.asarray(a).astype(np.float32)  # noqa: E731  (the result a correct kernel returns: the reference, rounded)
    slope = 0.2
    # GATv2: the score and the row pass gather xr (K side), the column pass gathers xl (M side)
    got = restate_score(P["rowptr"], P["colind"], x["xm"], x["xk"], x["att"], slope)
    bad = restate_score(P["rowptr"], P["colind"], x["xm"], o["xk"], x["att"], slope)
    assert worst_ratio(f32(got[0]), got[0], got[1], "score") <= 1.0 < worst_ratio(f32(got[0]), bad[0], bad[1], "score")
    got = restate_backward(P["rowptr"], P["colind"], x["gs"], x["xm"], x["xk"], x["att"], slope)
    bad = restate_backward(P["rowptr"], P["colind"], x["gs"], x["xm"], o["xk"], x["att"], slope)
    for i, name in ((0, "grad_xl"), (1, "att_part")):
        assert worst_ratio(f32(got[i]), got[i], got[i + 2], name) <= 1.0 < worst_ratio(f32(got[i]), bad[i], bad[i + 2], name)
    got = restate_backward(P["colptr"], P["rowind"], x["gs"], x["xk"], x["xm"], x["att"], slope, order=P["order"])
    bad = restate_backward(P["colptr"], P["rowind"], x["gs"], x["xk"], o["xm"], x["att"], slope, order=P["order"])
    assert worst_ratio(f32(got[0]), got[0], got[2], "grad_xr") <= 1.0 < worst_ratio(f32(got[0]), bad[0], bad[2], "grad_xr")
    # dot attention: forward and row pass gather k and v, the column pass gathers q and grad_out
    scale = float(np.float32(1.0 / np.sqrt(F)))
    xs = {"q": x["xm"], "k": x["xk"], "v": x["vk"], "go": x["go"], "scale": scale}
    f = ref_forward(P, xs)
    stats, out = f32(np.stack([f["m"], f["l"]], -1)), f32(f["out"])
    b = ref_backward(P, xs, stats, out)
    delta = f32(b["delta"])
    for name, other in (("k", o["xk"]), ("v", o["vk"]), ("q", o["xm"]), ("go", o["go"])):
        xo = dict(xs, **{name: other})
        fo = ref_forward(P, xo)
        bo = ref_backward(P, xo, stats, out, delta)
        r = {"out": ratio(out, fo["out"], fo["tol_out"]), "grad_q": ratio(f32(b["grad_q"]), bo["grad_q"], bo["tol_grad_q"]),
             "grad_k": ratio(f32(b["grad_k"]), bo["grad_k"], bo["tol_grad_k"]), "grad_v": ratio(f32(b["grad_v"]), bo["grad_v"], bo["tol_grad_v"])}
        seen = {"k": ("out", "grad_q"), "v": ("out", "grad_q"), "q": ("grad_k",), "go": ("grad_k", "grad_v")}[name]
        assert all(r[s] > 1.0 for s in seen), (name, r)
    r = {"out": ratio(out, f["out"], f["tol_out"]), "grad_q": ratio(f32(b["grad_q"]), b["grad_q"], b["tol_grad_q"]),
         "grad_k": ratio(f32(b["grad_k"]), b["grad_k"], b["tol_grad_k"]), "grad_v": ratio(f32(b["grad_v"]), b["grad_v"], b["tol_grad_v"])}
    assert max(r.values()) <= 1.0, r
    # the fused GAT backward: grad_el gathers feat (K side); grad_er gathers grad_out (M side)
    for p_keep in (None, 0.25):
        keep = ks = None
        if p_keep:
            keep, ks = np.random.RandomState(5).uniform(size=(P["nnz"], H)) >= p_keep, np.float32(1.0) / (np.float32(1.0) - np.float32(p_keep))
        args = (P["rows"], P["colind"], P["M"], P["K"], x["el"], x["er"])
        gel, ger, sel, ser = gat_backward_float64(*args, x["go"], x["vk"], slope, keep, ks)
        assert bound_ratio(f32(gel), gel, sel)[1] and bound_ratio(f32(ger), ger, ser)[1]
        bel, _, bsel, _ = gat_backward_float64(*args, x["go"], o["vk"], slope, keep, ks)
        _, ber, _, bser = gat_backward_float64(*args, o["go"], x["vk"], slope, keep, ks)
        assert not bound_ratio(f32(gel), bel, bsel)[1] and not bound_ratio(f32(ger), ber, bser)[1]


# ---- the fused GATv2 attention and the 16-bit GATv2 score (section c of the GPU module) ------------------------------------------------

@pytest.mark.parametrize("H,F,regime", CASES_B)
def test_windows_and_bytes_of_the_16_bit_gatv2_score(H, F, regime):
    """The limit counts elements: regime A's row counts put byte 2^31 (element 2^30) inside every 16-bit operand; regime B ends the
    K-side operands within one row and the limit's margin (4096 elements) of byte 2^32, and nothing the entries accept reaches it. The
    sub-patterns the score is compared on hold the rows with byte 2^31 and the last row of both sides (windows marked at elem = 2); the
    fused attention's fp32 operands are the sizes test_windows_hold_the_marked_rows_section_b already checks at elem = 4."""
    N = H * F
    M, K = lo.sizes_b(N, regime)
    _check_marks(M, K, N, 2, True)
    for rows in (M, K):
        assert rows * N > (1 << 30) and (1 << 31) // (2 * N) in lo.marked(rows, N, 2), "byte 2^31 lies inside the operand, its row is marked"
        assert rows * N * 2 < (1 << 32) and lo.marked(rows, N, 2)[-1] == rows - 1
    if regime == "B":
        assert (1 << 32) - 2 * N - 8192 <= K * N * 2 < (1 << 32) <= (K + 1) * N * 2 + 8192
    assert M * N * 4 > (1 << 32), "att_part (fp32, M rows) holds byte 2^32: compared whole on the device"


def _hashed(lo_, hi, salt, H, F):
    """A node-value function of the WORD position with values spread over [lo_, hi): what an array of seeded random values is to a
    displaced offset — another value at every alias (float64 torch tensor)."""
    def at(r, h, f):
        w = torch.as_tensor(r * (H * F) + h * F + f, dtype=torch.int64)
        return ((w * 1103515245 + salt) % (1 << 31)).to(torch.float64) / float(1 << 31) * (hi - lo_) + lo_

    return at


def _rows_of(fn, r0, r1, H, F):
    r = torch.arange(r0, r1, dtype=torch.int64).view(-1, 1, 1)
    return fn(r, torch.arange(H, dtype=torch.int64).view(1, H, 1), torch.arange(F, dtype=torch.int64).view(1, 1, F)).numpy().astype(np.float32)


def _band_pattern(n):
    """The band at d = 8 on n rows as a host pattern (the shape of a GPU sub-pattern)."""
    from test_dot_attention_host import transpose

    rowptr, colind = (t.numpy() for t in band.csr(n, D))
    K = n + lo.LAST
    colptr, rowind, order = transpose(rowptr, colind, K)
    return {"M": n, "K": K, "nnz": n * D, "rowptr": rowptr, "colind": colind, "colptr": colptr, "rowind": rowind, "order": order,
            "rows": np.repeat(np.arange(n, dtype=np.int32), D), "degs": np.full(n, D)}


def _displaced_cases(elem):
    """(H, F, regime, shift, side, first row): 64 rows of the pattern right behind the marked row of the operand of ``side`` — every word
    there has its alias, ``shift`` bytes back, inside the operand."""
    out = []
    for H, F, regime in CASES_B:
        N = H * F
        M, K = lo.sizes_b(N, regime)
        for shift in lo.BYTES:
            for side, rows in (("M", M), ("K", K)):
                if shift < rows * N * elem:
                    r0 = shift // (N * elem) + 1
                    assert r0 + 64 + lo.LAST <= rows
                    out.append((H, F, regime, shift, side, r0))
    return out


def test_no_alias_2_32_bytes_away_inside_a_16_bit_operand():
    """A displacement by 2^31 ELEMENTS (a position's sign, or a 32-bit byte offset formed from it) leaves every 16-bit operand the
    entries accept: a fault, not a wrong value. What a value comparison has to reject at element size 2 is 2^30 elements."""
    assert {c[3] for c in _displaced_cases(2)} == {1 << 31} and {c[3] for c in _displaced_cases(4)} == set(lo.BYTES)


@pytest.mark.parametrize("H,F,regime,shift,side,r0", _displaced_cases(4))
def test_gatv2_attention_comparators_reject_a_displaced_gather(H, F, regime, shift, side, r0):
    """Displaced by 2^29 and 2^30 WORDS (2^31, 2^32 bytes of an fp32 operand; 2^31 words lie outside every accepted one): the float64
    reference recomputed with the gathered operand read through the displaced position must put the correct result outside the
    tolerances of test_gatv2_attention_host.py — xr (K side) for the forward and the row pass, xl and grad_out (M side) for the
    column pass."""
    from test_dot_attention_host import ratio
    from test_gatv2_attention_host import ref_backward, ref_forward

    N, slope = H * F, 0.2
    M, K = lo.sizes_b(N, regime)
    P = _band_pattern(64)
    fns = {"xl": _hashed(-1, 1, 11, H, F), "xr": _hashed(-1, 1, 23, H, F), "go": _hashed(0.5, 1, 37, H, F)}
    spans = {"xl": (r0, r0 + 64, M), "xr": (r0, r0 + 64 + lo.LAST, K), "go": (r0, r0 + 64, M)}
    x = {k: _rows_of(fns[k], *spans[k][:2], H, F) for k in fns}
    x["att"] = (np.random.RandomState(N).uniform(-2, 2, size=(H, F)) * min(1.0, 8.0 / F)).astype(np.float32)
    f32 = lambda a: np.asarray(a).astype(np.float32)  # noqa: E731
    f = ref_forward(P, x, slope)
    stats, out = f32(np.stack([f["m"], f["l"]], -1)), f32(f["out"])
    b = ref_backward(P, x, slope, stats, out)
    delta = f32(b["delta"])
    bc = ref_backward(P, x, slope, stats, out, delta)
    good = {"out": ratio(out, f["out"], f["tol_out"]), "grad_xl": ratio(f32(b["grad_xl"]), b["grad_xl"], b["tol_grad_xl"]),
            "att_part": ratio(f32(b["att_part"]), b["att_part"], b["tol_att_part"]),
            "grad_xr": ratio(f32(bc["grad_xr"]), bc["grad_xr"], bc["tol_grad_xr"])}
    assert max(good.values()) <= 1.0, good
    for name in ("xr",) if side == "K" else ("xl", "go"):
        wrong = lo.displaced(fns[name], H, F, shift, spans[name][2], 4)
        xo = dict(x, **{name: _rows_of(wrong, *spans[name][:2], H, F)})
        assert not np.array_equal(xo[name], x[name])
        fo = ref_forward(P, xo, slope)
        bo = ref_backward(P, xo, slope, stats, out, delta)
        r = {"out": ratio(out, fo["out"], fo["tol_out"]), "grad_xl": ratio(f32(b["grad_xl"]), bo["grad_xl"], bo["tol_grad_xl"]),
             "att_part": ratio(f32(b["att_part"]), bo["att_part"], bo["tol_att_part"]),
             "grad_xr": ratio(f32(bc["grad_xr"]), bo["grad_xr"], bo["tol_grad_xr"])}
        seen = {"xr": ("out", "grad_xl", "att_part"), "xl": ("grad_xr",), "go": ("grad_xr",)}[name]
        assert all(r[s] > 1.0 for s in seen), (name, r)


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16))
@pytest.mark.parametrize("H,F,regime,shift,side,r0", _displaced_cases(2))
def test_gatv2_x16_comparators_reject_a_displaced_gather(H, F, regime, shift, side, r0, dtype):
    """Displaced by 2^30 ELEMENTS (2^31 bytes at element size 2): the score's float64 bound must reject the restatement on the displaced
    operand, and the oracle of the backward — compared on bits on the device — must differ from it in att_part and in the narrowed
    grad_x (xr, K side, for the score and the row pass; xl, M side, for the column pass)."""
    from gatv2_x16_cases import narrow
    from test_gatv2_host import restate_backward, restate_score, worst_ratio

    N, slope = H * F, 0.2
    M, K = lo.sizes_b(N, regime)
    P = _band_pattern(64)
    fns = {"xl": _hashed(-1, 1, 11, H, F), "xr": _hashed(-1, 1, 23, H, F)}
    spans = {"xl": (r0, r0 + 64, M), "xr": (r0, r0 + 64 + lo.LAST, K)}
    wide = lambda fn, k: narrow(_rows_of(fn, *spans[k][:2], H, F), dtype)[1]  # noqa: E731  (the 16-bit values, widened exactly)
    rng = np.random.RandomState(N)
    x = {"xl": wide(fns["xl"], "xl"), "xr": wide(fns["xr"], "xr"), "att": rng.uniform(-2, 2, size=(H, F)).astype(np.float32),
         "gs": rng.uniform(-2, 2, size=(P["nnz"], H)).astype(np.float32)}
    name = "xr" if side == "K" else "xl"
    xo = dict(x, **{name: wide(lo.displaced(fns[name], H, F, shift, spans[name][2], 2), name)})
    narrowed = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32)).to(dtype).view(torch.int16).numpy()  # noqa: E731
    if side == "K":
        ref, terms = restate_score(P["rowptr"], P["colind"], x["xl"], x["xr"], x["att"], slope)
        bad, bad_terms = restate_score(P["rowptr"], P["colind"], xo["xl"], xo["xr"], x["att"], slope)
        got32 = ref.astype(np.float32)
        assert worst_ratio(got32, ref, terms, "score") <= 1.0 < worst_ratio(got32, bad, bad_terms, "score")
        got = restate_backward(P["rowptr"], P["colind"], x["gs"], x["xl"], x["xr"], x["att"], slope)
        other = restate_backward(P["rowptr"], P["colind"], x["gs"], xo["xl"], xo["xr"], x["att"], slope)
        assert not np.array_equal(got[1].astype(np.float32), other[1].astype(np.float32)), "att_part"
    else:
        got = restate_backward(P["colptr"], P["rowind"], x["gs"], x["xr"], x["xl"], x["att"], slope, order=P["order"])
        other = restate_backward(P["colptr"], P["rowind"], x["gs"], xo["xr"], xo["xl"], x["att"], slope, order=P["order"])
    assert not np.array_equal(narrowed(got[0]), narrowed(other[0])), "grad_x"


# ---- the 16-bit max reducer at the 4 GB limit (section a of the GPU module) -------------------------------------------------------------

def _x16_max_sizes(H, F):
    N = H * F
    M, K = lo.sizes_a(N, "below", "rows")
    assert K * N * 4 < (1 << 32) <= (K + 1) * N * 4 and (1 << 30) < M * N * 2 < K * N * 2 < (1 << 31)
    return N, M, K


@pytest.mark.parametrize("H,F", lo.WIDTHS)
def test_windows_of_the_16_bit_max_reducer(H, F):
    """The windows of test_max_arg_x16_below_the_4gb_limit are marked at elem = 4, the size of an ``arg`` word: the row with byte 2^31
    of arg is the row with byte 2^30 of every 16-bit array — from it on ``off + 4 c`` has its top bit set — and it, and the last row of
    every operand, lie inside a row window and a column window."""
    N, M, K = _x16_max_sizes(H, F)
    rw, cw = _check_marks(M, K, N, 4, False)
    r = (1 << 31) // (N * 4)
    assert r == (1 << 30) // (N * 2) and r * N * 2 <= (1 << 30) < (r + 1) * N * 2 and r * N * 4 <= (1 << 31) < (r + 1) * N * 4
    for rows in (M, K):
        assert r in lo.marked(rows, N, 4) and rows - 1 in lo.marked(rows, N, 4) and r < rows - 1
    assert lo.holds(rw, r) and lo.holds(cw, r) and lo.holds(rw, M - 1) and lo.holds(cw, M - 1) and lo.holds(cw, K - 1)
    assert ((M - 1) * N * 4 + 4 * (N - 1)) >> 31 == 1 and (M - 1) * N * 4 + 4 * (N - 1) <= (1 << 32) - 16, "the largest staged sum: top bit set"
    assert ((r - 1) * N * 4) >> 31 == 0


def _marks_with_an_alias(rows, N, shift_words):
    """The marked rows (elem = 4: the windows' marks) of a [rows, N] array that hold a word whose alias ``shift_words`` back lies inside"""
    return [m for m in lo.marked(rows, N, 4) if (m + 1) * N > shift_words]


@pytest.mark.parametrize("H,F", lo.WIDTHS)
def test_16_bit_max_references_reject_a_displaced_gather(H, F):
    """What a lost top bit of ``(off + 4 c)`` reads: grad_out 2^30 bytes back (elem = 2), arg 2^31 bytes back (elem = 4) — 2^29 words
    either way; and for the forward a B row 2^30 bytes back. Around every marked row whose alias lies inside the array, the closed-form
    reference through the displaced offset must differ from the true one: the comparisons of the GPU test are exact equalities."""
    N, M, K = _x16_max_sizes(H, F)
    shift = 1 << 29  # words of arg, elements of a 16-bit array
    assert shift % 7 != 0 and (1 << 30) % 7 != 0, "b_at and max_grad_at are residues modulo 7"
    # ---- forward: B (K rows, 16-bit) gathered 2^30 bytes back
    fn = lo.b_at(H, F)
    wrong = lo.displaced(fn, H, F, 1 << 30, K, 2)
    marks = _marks_with_an_alias(K, N, shift)
    assert (1 << 30) // (N * 2) in marks and K - 1 in marks
    for m in marks:
        r1 = min(m + 1, M)
        good, bad = (lo.ref_max_forward(max(r1 - 32, 0), r1, H, F, dense_fn=f_) for f_ in (fn, wrong))
        assert not (torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1])), ("forward", m)
        assert not torch.equal(good[0], bad[0]), ("forward: the values alone", m)
    # ---- backward: grad_out (M rows, 16-bit) 2^30 bytes back, arg (M rows, 4-byte) 2^31 bytes back
    grad_back = lo.displaced(lambda r, h, f: lo.max_grad_at(r, f), 1, N, 1 << 30, M, 2)
    arg_back = lo.displaced(lambda r, h, f: lo.max_arg_at(r, f), 1, N, 1 << 31, M, 4)
    marks = _marks_with_an_alias(M, N, shift)
    assert (1 << 31) // (N * 4) in marks and M - 1 in marks
    for m in marks:
        c0, c1 = m, min(m + 32, K)
        good = lo.ref_max_backward(M, c0, c1, N)
        assert int(good.abs().sum()) > 0 and int(good.abs().max()) <= D * 3
        bad_grad = lo.ref_max_backward(M, c0, c1, N, grad_fn=lambda r, n: grad_back(r, 0, n))
        bad_arg = lo.ref_max_backward(M, c0, c1, N, arg_fn=lambda r, n: arg_back(r, 0, n))
        for dtype in (torch.bfloat16, torch.float16):
            narrow = lambda t: t.to(torch.float32).to(dtype)  # noqa: E731  (what _check_windows compares with)
            assert band.first_difference(narrow(good), narrow(bad_grad)) is not None, ("grad_out", m, dtype)
            assert band.first_difference(narrow(good), narrow(bad_arg)) is not None, ("arg", m, dtype)


def test_the_closed_forms_of_the_max_reducer_are_the_fp32_tests():
    """lo.ref_max_forward / lo.ref_max_backward against the reducer's restatement (max_arg_ref.py) on a small band with the same
    operands: the closed forms the 16-bit GPU test compares with are the chains' results."""
    from max_arg_ref import max_arg_forward, max_backward, transpose

    M, H, F = 200, 3, 5
    N, K = H * F, M + lo.LAST
    rowptr, colind = (t.numpy() for t in band.csr(M, D))
    r, h, f = torch.arange(K).view(-1, 1, 1), torch.arange(H).view(1, H, 1), torch.arange(F).view(1, 1, F)
    B = lo.b_at(H, F)(r, h, f).reshape(K, N).numpy().astype(np.float32)
    C, arg = max_arg_forward(rowptr, colind, B, -10000.0)
    top, first = lo.ref_max_forward(0, M, H, F)
    assert np.array_equal(C, top.numpy().astype(np.float32)) and np.array_equal(arg, first.numpy().astype(np.int32))
    rr, nn = torch.arange(M).view(-1, 1), torch.arange(N).view(1, -1)
    arg2, grad = lo.max_arg_at(rr, nn).numpy().astype(np.int32), lo.max_grad_at(rr, nn).numpy().astype(np.float32)
    colptr, rowind, order = transpose(rowptr, colind, K)
    want = max_backward(colptr, rowind, order, arg2, grad, K)
    assert np.array_equal(want, lo.ref_max_backward(M, 0, K, N).numpy().astype(np.float32))


# ---- the band at d = 8 ----------------------------------------------------------------------------------------------------------------

def test_band_at_d8_equals_a_numpy_transpose():
    M = 1000
    nnz, K = band.sizes(M, D)
    assert K == M + 22 and [band.offset_of(j) for j in range(D)] == [0, 4, 7, 9, 13, 16, 18, 22]
    rowptr, colind, rows, colptr_np, rowind_np, order_np = _numpy_transpose(M, D)
    assert nnz == colind.size and K == colind.max() + 1
    colptr, rowind, order = band.csc(M, D)
    assert np.array_equal(colptr.numpy(), colptr_np) and np.array_equal(rowind.numpy(), rowind_np) and np.array_equal(order.numpy(), order_np)
    band.verify_csc(M, D, colptr, order)
    # the products of the GPU cases stay exact: |sum| <= 8 * 2 * 3 (heads with w_nz: 8 * 3 * 3, also in bf16 / fp16: integers below 2^8) and 512 * 3 * 2 (SDDMM)
    assert D * 3 * 3 < (1 << 8) and 512 * 3 * 2 < (1 << 24)
