"""Sizes, marked rows, windows and closed-form aliases of the node-sized cases of test_gpu_large_operands.py (plain module beside
band.py; shared with test_large_operands_host.py, which derives and checks all of it without a device).

The pattern is band.py's band at d = 8: row r holds the columns r + {0, 4, 7, 9, 13, 16, 18, 22}, K = M + 22. A case fixes the width
(H, F), the element size of the dense operands and ONE of the two row counts — the other follows from K = M + 22:

  section a (the kernels with ``uint32_t`` byte offsets): the GATHERED operand has R rows (``below``: the largest R with
      R * row_bytes < 2^32) or R + 1 (``at``: the first size the kernel is not offered). Walking rows, the gathered operand has K
      rows; walking columns (the CSC arrays, transposed=True) it has M rows — M plays K's part.
  section b (the kernels with ``int`` word positions): regime A, 2^21 + 2^19 + 16 rows at H F = 512 and as many words at H F = 300
      (5.4 GB an array); regime B, K = floor(kSddmmMaxNnz / (H F)), the largest the entries accept (8.0 GB an array).

Marked rows of an operand: the rows holding byte 2^31 and byte 2^32 (word 2^29 and word 2^30 of an fp32 array) and its last row.
Windows: band.window_starts over the pattern's rows and over its columns, one centred on every marked row of EITHER side (a row
window around r gathers the K-side rows r .. r + 22 and a column window around c the M-side rows c - 22 .. c), plus the first and
the last."""
import torch

import band

D = 8
LAST = band.offset_of(D - 1)  # 22
WIDTHS = ((8, 64), (3, 100))
MAX_WORDS = (1 << 31) - 1 - 4096  # kSddmmMaxNnz (csrc/spmm_kernels.h): the largest count of 32-bit word positions an entry accepts
BYTES = (1 << 31, 1 << 32)
REGIME_A_ROWS_512 = (1 << 21) + (1 << 19) + 16
ERANGE = -3


def w_nz(e, h):
    """band.w_of without its zeros (0 becomes 3): a weight in {-2, -1, 1, 2, 3} of CSR entry e, head h. With it EVERY gathered word
    shows in the product — a wrapped offset may touch one entry of one row only, and a zero weight would hide it."""
    v = (7 * e + 3 * h) % 5 - 2
    return v + 3 * (v == 0)


def b_at(H, F):
    """A node-value function of the WORD position: ((r H F + h F + f) mod 7) - 3. A linear form of (r, h, f) like band.b_of keeps its
    value across whole bands of aliases when the row is 1200 bytes (the alias of a word lies in another row at another head); this
    one differs from its alias in EVERY word, whatever the width: 2^29, 2^30 and 2^31 are 4, 1 and 2 modulo 7."""
    return lambda r, h, f: (r * (H * F) + h * F + f) % 7 - 3


def k_at(H, F):
    """The second node array, ((r H F + h F + f) mod 5) - 2: 2^29, 2^30 and 2^31 are 2, 4 and 3 modulo 5."""
    return lambda r, h, f: (r * (H * F) + h * F + f) % 5 - 2


def row_bytes(N, elem=4):
    return N * elem


def switch_rows(N, elem=4):
    """Largest R with R * row_bytes < 2^32: the gathered operand the byte-offset kernels still take."""
    return ((1 << 32) - 1) // row_bytes(N, elem)


def sizes_a(N, side, walk, elem=4):
    """(M, K) of a section-a case: ``walk`` "rows" (the gathered operand has K rows) or "cols" (M rows)."""
    R = switch_rows(N, elem) + (1 if side == "at" else 0)
    return (R - LAST, R) if walk == "rows" else (R, R + LAST)


def regime_rows(N, regime):
    """K of a section-b case; M = K - 22."""
    if regime == "A":
        return -(-REGIME_A_ROWS_512 * 512 // N) + LAST
    return MAX_WORDS // N


def sizes_b(N, regime):
    K = regime_rows(N, regime)
    return K - LAST, K


def marked(rows, N, elem=4):
    """Rows of a [rows, N] operand that hold byte 2^31 / byte 2^32 (where it is that large), and its last row."""
    rb = row_bytes(N, elem)
    return sorted({b // rb for b in BYTES if b < rows * rb} | {rows - 1})


def windows(n, marks, spread=14):
    """band.window_starts over n segments, one window centred on every mark (clamped into [0, n))."""
    return [(s, min(s + band.WINDOW, n)) for s in band.window_starts(n, [min(max(m, 0), n - 1) for m in marks], spread=spread)]


def case_windows(M, K, N, elem=4, spread=14):
    """(row windows, column windows) of a case: every marked row of the M-side and of the K-side operands in both lists, the first
    window and the last, and ``spread`` - 2 evenly spaced between them — 14 for the integer ops, whose references cost nothing; 2 for
    the float ops, whose float64 references run on the host (one 512-row sub-pattern per window)."""
    marks = marked(M, N, elem) + marked(K, N, elem)
    return windows(M, marks, spread), windows(K, marks, spread)


# ---- the max reducer on the band: closed forms of both directions, by window (the 16-bit tests and their host checks) -----------------

def max_arg_at(r, n):
    """arg[r, n] = r d + ((r + n) mod d): word n of row r was won by the row's entry j = (r + n) mod d (test_gpu_large_edges.py)."""
    return r * D + (r + n) % D


def max_grad_at(r, n):
    """grad_out[r, n] = ((r + 3 n) mod 7) - 3, an integer in -3 .. 3: exact in fp32, bf16 and fp16."""
    return (r + 3 * n) % 7 - 3


def ref_max_forward(r0, r1, H, F, device="cpu", dense_fn=None):
    """(int64[r1 - r0, H F] max, int64[r1 - r0, H F] arg) of rows r0 .. r1: the largest of dense(r + o_j, h, f) over the d band entries
    and the CSR position r d + j of the FIRST entry that reaches it."""
    dense_fn = b_at(H, F) if dense_fn is None else dense_fn
    r = torch.arange(r0, r1, device=device, dtype=torch.int64).view(-1, 1, 1, 1)
    j = torch.arange(D, device=device, dtype=torch.int64).view(1, D, 1, 1)
    hh, ff = band._hf(H, F, device)
    vals = dense_fn(r + band.offset_of(j), hh, ff)
    top = vals.max(1, keepdim=True).values
    first = torch.where(vals == top, j, D).min(1).values
    return top.reshape(r1 - r0, H * F), (r.view(-1, 1, 1) * D + first).reshape(r1 - r0, H * F)


def ref_max_backward(M, c0, c1, N, device="cpu", grad_fn=max_grad_at, arg_fn=max_arg_at):
    """int64[c1 - c0, N]: columns c0 .. c1 of grad_B — column c receives grad(r, n) from every row r = c - o_j of the band whose
    arg(r, n) names that entry's CSR position r d + j."""
    c = torch.arange(c0, c1, device=device, dtype=torch.int64).view(-1, 1, 1)
    j = torch.arange(D, device=device, dtype=torch.int64).view(1, -1, 1)
    n = torch.arange(N, device=device, dtype=torch.int64).view(1, 1, -1)
    r = c - band.offset_of(j)
    inside = (r >= 0) & (r < M)
    r = r.clamp(0, M - 1)  # (rows outside the band contribute nothing; clamped so that the closed forms see a row that exists)
    hit = inside & (arg_fn(r, n) == r * D + j)
    return (hit.to(torch.int64) * grad_fn(r, n)).sum(1)


FLOAT_ROWS = 512  # rows of a float op's sub-pattern (test_gpu_large_edges.py)


def sub_rows(win, M):
    """The FLOAT_ROWS rows of a row window that the float ops are compared on: the first rows of the first window, the last rows of the
    last one (the last node is in), the MIDDLE of every other — a window is centred on its mark."""
    s0, s1 = win
    if s0 == 0:
        return 0, FLOAT_ROWS
    if s1 == M:
        return M - FLOAT_ROWS, M
    r0 = s0 + (s1 - s0 - FLOAT_ROWS) // 2
    return r0, r0 + FLOAT_ROWS


def holds(wins, seg):
    return any(s0 <= seg < s1 for s0, s1 in wins)


# ---- what a wrapped offset would read: the closed-form node arrays by WORD position -----------------------------------------------

def value_at_word(fn, w, H, F):
    """fn(r, h, f) of the word at position w of an [R, H, F] array (tensor or int)."""
    N = H * F
    r = w // N
    n = w - r * N
    return fn(r, n // F, n % F)


def displaced(fn, H, F, shift_bytes, rows, elem=4):
    """A node-value function that reads what a byte offset displaced by ``shift_bytes`` modulo 2^32 holds: word position
    (w elem - shift_bytes) mod 2^32 / elem of the same array, where that lies inside its ``rows`` rows; the true word elsewhere (a
    wrap that leaves the array is a fault, not a wrong value). At N = 512 this is row r -+ 2^21 (2^20); at N = 300 the alias falls
    inside another row at another (h, f)."""
    N = H * F
    span = (1 << 32) // elem

    def at(r, h, f):
        w = r * N + h * F + f
        alias = (w - shift_bytes // elem) % span
        if isinstance(alias, torch.Tensor):
            return value_at_word(fn, torch.where(alias < rows * N, alias, w), H, F)
        return value_at_word(fn, alias if alias < rows * N else w, H, F)

    return at
