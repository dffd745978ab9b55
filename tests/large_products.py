"""Patterns, sizes, marked rows and closed-form references of the sum / max products at the 32-bit offset switches (DESIGN.md §4.3;
plain module beside band.py and large_operands.py; shared by test_large_products_host.py, which derives and checks all of it without
a device, and test_gpu_large_products.py).

A pattern has M rows of d + 1 entries: the d BAND columns base(r) + o_j (band.offset_of) and, last, one FAR column far(r). Every array is
elementwise arithmetic on the row number — nothing gathers or scatters by an index, so the pattern can be built at 22 M rows without
trusting the indexing it is there to test. Three kinds:

  both   base(r) = r, K = M + o_{d-1}: band.py's band; far(r) = (r P + c0) mod K, P an odd prime, c0 such that that of the last row but one is K - 1.
         B and C are both at the size under test. The band is what a block of rows shares (staged in LDS / padded records), the far column is gathered from memory.
  tall   the same rows with every column folded into a small K (mod K): B stays a few MB, only the C addressing is at its limit.
  wide   M = 4096 rows in groups of 128: a group's band starts at (r div 128) J + (r mod 128), the groups J rows apart from the first
         row of B to its last; far(r) walks the MARKED rows of B (the rows holding byte 2^31 and byte 2^32, the last row) and the row
         before each. C stays a few MB, only the B addressing is at its limit.

Dense operand: large_operands.b_at(1, N), a function of the WORD position ((w mod 7) - 3), weights large_operands.w_nz (no zeros) of
the entry number e = r (d + 1) + j. Every fp32 sum is an exact small integer: |sum| <= 9 (d + 1)."""
import torch

import band
import large_operands as lo

D = 4              # band entries of a row in the GPU cases; with the far column a row end every 5 records
P_FAR = 1_000_003  # an odd prime: r -> r P mod K visits rows of B far from the band, on both sides of every power-of-two byte
GROUP = 128        # rows of a group of the wide pattern (a block of the staged kernels holds 64 .. 128 rows)
M_WIDE = 4096
K_TALL = 4099      # rows of B of a tall pattern (prime: the folded band wraps at no power of two)
TABLE_BOUND = 0xFFFF0000        # staged_serves / staged_narrow_serves / staged_gen_serves: max(M, K) N 4 below it
TABLE_BOUND_PAGED = 0x1FFFF0000  # staged_serves at N = 512 / 1024: two 4 GB halves
BYTE_BOUND = 1 << 32            # records_serves, and the idx32 / idx64 switch of the streaming kernels (K N elem)
EMPTY = -10000.0                # the max reducer's value of an empty row: never among the maxima (|b| <= 3)


def last_row_below(bound, N, elem=4):
    """R = floor((bound - 1) / row bytes): the largest row count with R * row bytes < bound."""
    return (bound - 1) // (N * elem)


class Pattern:
    def __init__(self, kind, R, d):
        """``R``: the row count of the operand(s) under test — K (= the larger of M and K) for ``both``, M for ``tall``, K for ``wide``."""
        assert kind in ("both", "tall", "wide")
        self.kind, self.d, self.R = kind, d, R
        last = band.offset_of(d - 1)
        if kind == "both":
            self.M, self.K = R - last, R
        elif kind == "tall":
            self.M, self.K = R, K_TALL
        else:
            self.M, self.K = M_WIDE, R
            self.jump = (R - GROUP - last) // (M_WIDE // GROUP - 1)
            assert self.jump > GROUP + last
        self.c0 = (self.K - 1 - (self.M - 2) * P_FAR) % self.K  # the far column of the last row but one is the LAST row of B (the last row's band ends there)
        self.w = d + 1                # entries of a row
        self.nnz = self.M * self.w

    # -- elementwise on an int64 tensor (or an int) of row numbers
    def base(self, r):
        if self.kind == "wide":
            return (r // GROUP) * self.jump + r % GROUP
        return r

    def far(self, r, marks=None):
        if self.kind == "wide":
            marks = self.marks_wide if marks is None else marks
            n = len(marks)
            i, odd = r % n, (r // n) % 2
            if isinstance(r, torch.Tensor):
                m = torch.tensor(marks, dtype=torch.int64, device=r.device)[i]
                return (m - odd).clamp_(min=0)
            return max(marks[i] - odd, 0)
        return (r * P_FAR + self.c0) % self.K

    def col(self, r, j):
        """Column of entry j (0 .. d: d is the far one) of row r."""
        if j == self.d:
            return self.far(r)
        c = self.base(r) + band.offset_of(j)
        return c % self.K if self.kind == "tall" else c

    def set_marks(self, N, elem=4):
        """The wide pattern's far columns walk B's marked rows at this width."""
        self.marks_wide = lo.marked(self.K, N, elem)
        return self

    def cols(self, r0, r1, device="cpu"):
        """int64[r1 - r0, d + 1]"""
        r = torch.arange(r0, r1, device=device, dtype=torch.int64)
        return torch.stack([self.col(r, j) for j in range(self.w)], 1)

    def csr(self, device="cpu", chunk=1 << 22):
        """(rowptr int32[M + 1], colind int32[nnz]), in row chunks."""
        assert self.nnz < (1 << 31)
        rowptr = (torch.arange(self.M + 1, device=device, dtype=torch.int64) * self.w).to(torch.int32)
        colind = torch.empty(self.nnz, dtype=torch.int32, device=device)
        for r0 in range(0, self.M, chunk):
            r1 = min(r0 + chunk, self.M)
            colind[r0 * self.w:r1 * self.w] = self.cols(r0, r1, device).reshape(-1)
        return rowptr, colind

    def values(self, device="cpu", dtype=torch.float32):
        return band.edge_values(torch.arange(self.nnz, device=device), 1, dtype, lo.w_nz).view(-1)

    # -- references on rows r0 .. r1, int64[r1 - r0, N]
    def _gathered(self, r0, r1, N, device, dense_fn):
        c = self.cols(r0, r1, device).view(r1 - r0, self.w, 1)
        n = torch.arange(N, device=device, dtype=torch.int64).view(1, 1, N)
        return dense_fn(c, 0, n)

    def ref_sum(self, r0, r1, N, device="cpu", dense_fn=None, weighted=True):
        dense_fn = lo.b_at(1, N) if dense_fn is None else dense_fn
        b = self._gathered(r0, r1, N, device, dense_fn)
        if not weighted:
            return b.sum(1)
        r = torch.arange(r0, r1, device=device, dtype=torch.int64).view(-1, 1, 1)
        j = torch.arange(self.w, device=device, dtype=torch.int64).view(1, self.w, 1)
        return (lo.w_nz(r * self.w + j, 0) * b).sum(1)

    def ref_max(self, r0, r1, N, device="cpu", dense_fn=None):
        dense_fn = lo.b_at(1, N) if dense_fn is None else dense_fn
        return self._gathered(r0, r1, N, device, dense_fn).max(1).values

    def max_abs_sum(self):
        return 9 * self.w  # |w| <= 3, |b| <= 3

    # -- what the test compares
    def marked_rows(self, N, elem=4):
        """Rows of C whose result a wrong address would spoil: C's own marked rows, and — wide — nothing more (every row gathers a
        marked row of B)."""
        return lo.marked(self.M, N, elem)

    def windows(self, N, elem=4, spread=6):
        """Row windows of 4096 rows: the first, the last, ``spread`` - 2 between them and one centred on every marked row of C; for
        ``both`` also on the rows whose BAND reaches B's marked rows (row m - o_j gathers row m)."""
        marks = list(self.marked_rows(N, elem))
        if self.kind == "both":
            marks += lo.marked(self.K, N, elem)
        return lo.windows(self.M, marks, spread)


HUB = 4096  # entries of the hub row: more than the 2048 at which the long-row pass (and a staged plan's hub pass) takes a row over


class HubPattern(Pattern):
    """``both`` with ONE more row at the end, row M - 1, of HUB entries: the columns j J (J = K div HUB: ascending, from the first row
    of B towards its last) and, in its last entries, B's marked rows — the rows holding byte 2^31 and byte 2^32 and the last row — and
    the row before each. The other rows, their entry numbers and their weights are those of ``both``; the hub's entries follow them."""

    def __init__(self, R, d, N, elem=4):
        Pattern.__init__(self, "both", R, d)
        self.rows = self.M          # the rows of d + 1 entries
        self.M = self.rows + 1
        self.c0 = (self.K - 1 - (self.rows - 2) * P_FAR) % self.K
        self.nnz = self.rows * self.w + HUB
        self.set_marks(N, elem)
        self.tail = sorted({max(m - i, 0) for m in self.marks_wide for i in (0, 1)})
        self.stride = self.K // HUB
        assert self.stride >= 1 and len(self.tail) < HUB

    def hub_cols(self, device="cpu"):
        j = torch.arange(HUB, device=device, dtype=torch.int64)
        c = j * self.stride
        c[HUB - len(self.tail):] = torch.tensor(self.tail, dtype=torch.int64, device=device)
        return c

    def csr(self, device="cpu", chunk=1 << 22):
        assert self.nnz < (1 << 31)
        rowptr = torch.empty(self.M + 1, dtype=torch.int32, device=device)
        rowptr[:self.M] = (torch.arange(self.M, device=device, dtype=torch.int64) * self.w).to(torch.int32)
        rowptr[self.M] = self.nnz
        colind = torch.empty(self.nnz, dtype=torch.int32, device=device)
        for r0 in range(0, self.rows, chunk):
            r1 = min(r0 + chunk, self.rows)
            colind[r0 * self.w:r1 * self.w] = self.cols(r0, r1, device).reshape(-1)
        colind[self.rows * self.w:] = self.hub_cols(device).to(torch.int32)
        return rowptr, colind

    def _hub(self, N, device, dense_fn, weighted, reduce):
        c = self.hub_cols(device).view(HUB, 1)
        n = torch.arange(N, device=device, dtype=torch.int64).view(1, N)
        b = dense_fn(c, 0, n)
        if reduce == "max":
            return b.max(0).values.view(1, N)
        if weighted:
            b = b * lo.w_nz(self.rows * self.w + torch.arange(HUB, device=device, dtype=torch.int64), 0).view(HUB, 1)
        return b.sum(0).view(1, N)

    def ref_sum(self, r0, r1, N, device="cpu", dense_fn=None, weighted=True):
        dense_fn = lo.b_at(1, N) if dense_fn is None else dense_fn
        parts = [Pattern.ref_sum(self, r0, min(r1, self.rows), N, device, dense_fn, weighted)] if r0 < self.rows else []
        if r1 == self.M:
            parts.append(self._hub(N, device, dense_fn, weighted, "sum"))
        return torch.cat(parts, 0)

    def max_abs_sum(self):
        return 9 * HUB


def far_reach(p, wins, N, elem=4):
    """For the rows of ``wins``: the set of halves of B (split at byte 2^31 and, where B is that large, byte 2^32) that their far
    columns reach, as a sorted list of 0 / 1 / 2, and whether the last row of B is among them."""
    rb = N * elem
    seen, last = set(), False
    for s0, s1 in wins:
        f = p.far(torch.arange(s0, s1, dtype=torch.int64))
        byte = f * rb
        seen |= set(torch.unique((byte >= (1 << 31)).to(torch.int64) + (byte >= (1 << 32)).to(torch.int64)).tolist())
        last = last or bool((f == p.K - 1).any())
    return sorted(seen), last


def displaced_c(ref, r0, N, shift_bytes, rows, elem=4):
    """What a window [r0, r0 + len(ref)) of a NaN-prefilled C holds when every C row of the window is stored at its byte offset
    displaced by ``shift_bytes`` modulo 2^32 (where that still lies inside C's ``rows`` rows; a store that leaves C is a fault, not a wrong
    value): the displaced rows keep NaN. float64, so NaN can be told from a sum."""
    out = ref.to(torch.float64).clone()
    r = torch.arange(r0, r0 + ref.shape[0], dtype=torch.int64)
    alias = ((r * N * elem - shift_bytes) % (1 << 32)) // (N * elem)
    moved = (alias < rows) & (alias != r)
    out[moved] = float("nan")
    return out


def wrong_half_c(ref, r0, N, rows, elem=4):
    """The window of a NaN-prefilled C when every row is stored into the OTHER 4 GB half — row r below row 2^32 / row bytes lands at
    r + 2^32 / row bytes, a row at or past it at r - 2^32 / row bytes — where that lies inside C's ``rows`` rows: those rows keep NaN."""
    out = ref.to(torch.float64).clone()
    page = (1 << 32) // (N * elem)
    r = torch.arange(r0, r0 + ref.shape[0], dtype=torch.int64)
    other = torch.where(r >= page, r - page, r + page)
    out[other < rows] = float("nan")
    return out


# ---- the sizes and the cases of test_gpu_large_products.py (shared with test_large_products_host.py) ------------------------------------

R128 = last_row_below(TABLE_BOUND, 128)
R256 = last_row_below(TABLE_BOUND, 256)
R512, R512P = last_row_below(TABLE_BOUND, 512), last_row_below(TABLE_BOUND_PAGED, 512)
R1024, R1024P = last_row_below(TABLE_BOUND, 1024), last_row_below(TABLE_BOUND_PAGED, 1024)
R64 = last_row_below(TABLE_BOUND, 64)
R602, R100 = last_row_below(TABLE_BOUND, 602), last_row_below(TABLE_BOUND, 100)
REC64, REC48 = last_row_below(BYTE_BOUND, 64), last_row_below(BYTE_BOUND, 48)
K512, K300 = last_row_below(BYTE_BOUND, 512), last_row_below(BYTE_BOUND, 300)
X512, X1024 = last_row_below(BYTE_BOUND, 512, 2), last_row_below(BYTE_BOUND, 1024, 2)

# N, R, kind, reorder, served (the kernel is offered), idx word of the streaming launch behind the plan
TUNED = [
    # N, R, kind, reorder, served, idx word of the fallback launch
    (128, R128, "both", True, True, "idx32"),
    (128, R128, "tall", True, True, "idx32"),
    (128, R128, "wide", True, True, "idx32"),
    (128, R128, "both", False, True, "idx32"),
    (128, R128 + 1, "both", True, False, "idx32"),
    (256, R256, "both", True, True, "idx32"),
    (256, R256, "tall", True, True, "idx32"),
    (256, R256, "wide", True, True, "idx32"),
    (256, R256, "tall", False, True, "idx32"),
    (256, R256 + 1, "both", True, False, "idx32"),
    (512, R512, "both", True, True, "idx32"),       # unpaged, bit 31 set past row 2^20
    (512, R512, "tall", True, True, "idx32"),
    (512, R512, "wide", True, True, "idx32"),
    (512, R512 + 1, "both", True, True, "idx32"),   # paged just above it; every code still in the lower half
    (512, R512P, "both", True, True, "idx64"),      # paged, 8 GB
    (512, R512P, "tall", True, True, "idx32"),
    (512, R512P, "wide", True, True, "idx64"),
    (512, R512P, "both", False, True, "idx64"),
    (512, R512P + 1, "both", True, False, "idx64"),
    (1024, R1024, "both", True, True, "idx32"),
    (1024, R1024, "tall", True, True, "idx32"),
    (1024, R1024, "wide", True, True, "idx32"),
    (1024, R1024 + 1, "both", True, True, "idx32"),
    (1024, R1024P, "both", True, True, "idx64"),
    (1024, R1024P, "tall", True, True, "idx32"),
    (1024, R1024P, "wide", True, True, "idx64"),
    (1024, R1024P, "tall", False, True, "idx32"),
    (1024, R1024P + 1, "both", True, False, "idx64"),
]


NARROW = [
    (64, R64, "both", True, True, "idx32"),
    (64, R64, "tall", True, True, "idx32"),
    (64, R64, "both", False, True, "idx32"),
    (64, R64 + 1, "both", True, False, "idx32"),
]


GENERAL = [
    (602, R602, "both", True, True, "idx32"),
    (602, R602, "tall", False, True, "idx32"),
    (602, R602 + 1, "both", True, False, "idx32"),
    (100, R100, "both", True, True, "idx32"),
    (100, R100, "both", False, True, "idx32"),
    (100, R100 + 1, "both", True, False, "idx32"),
]


RECORD = [
    (64, REC64, "both", True, True, "idx32"),
    (64, REC64, "tall", True, True, "idx32"),
    (64, REC64, "both", False, True, "idx32"),
    (64, REC64 + 1, "both", True, False, "idx64"),
    (48, REC48, "both", True, True, "idx32"),
    (48, REC48, "tall", False, True, "idx32"),
    (48, REC48 + 1, "both", True, False, "idx64"),
]
