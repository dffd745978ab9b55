"""Sizes, marked rows, closed-form operands and references of test_gpu_linear_large.py (plain module beside band.py and
large_operands.py; test_large_linear_host.py derives and checks all of it without a device).

Pattern: band.py's band, d entries per row (row i holds the columns i + o_j, Kn = M + o_{d-1}), the same band in every relation of the
stacked CSR. A case sizes ONE array just past 2^32 bytes, or up to the entry's limit of 2^31 - 4097 elements, and keeps every other
size at its minimum. (Every dense array of these entries is held to 2^31 - 4097 ELEMENTS, so a 16-bit array ends 8194 bytes short of
2^32: the 16-bit cases sit at the limit and cross byte 2^31; only fp32 arrays cross byte 2^32.) Operands are integers of the element's position, so every sum is exact in the case's type (linear_cases.py's
exact mode: at most |H| <= 2 d and four non-zero weights per output column, far below 256) and a window of output rows is an int64
broadcast of closed forms, with no index array:

    X[c, k]      = ((c K + k) mod 7) mod 3 - 1          in {-1, 0, 1}; 2^31 and 2^32 are 2 and 4 modulo 7: an offset that wraps reads
                                                        another residue in most words
    root[i, k]   = ((3 i K + k) mod 5) mod 3 - 1
    value of CSR entry e       1 + e mod 2              row_scale of stacked row s      (0.5, 1, 2)[s mod 3]
    W[r, n, k]   = +-1 where k = (5 n + 3 r + 7 t) mod K for t = 0 .. 3 (sign by t + n), 0 elsewhere; root_weight the same with t < 2
    bias[n]      = n mod 7 - 3
    grad_out[i, n] (weight gradient) = +-1 in the marked rows of grad_out, the first row and the row before the last, 0 elsewhere

Marked rows of an array: large_operands.marked — the rows holding byte 2^31 and byte 2^32, and the last row."""
import torch

import band
import large_operands as lo

LIM = lo.MAX_WORDS  # 2^31 - 4097: the largest count of 32-bit element positions an entry accepts
ES = {"bf16": 2, "fp16": 2, "fp32": 4}


def _past(row_elems, elem):
    """The first row count with a row that holds byte 2^32."""
    return (1 << 32) // (row_elems * elem) + 1


def _case(name, op, dt, R, M, K, N_out, d, root=False, valued=False, scaled=False, array=None):
    Kn = M + band.offset_of(d - 1)
    return {"name": name, "op": op, "dt": dt, "R": R, "M": M, "Kn": Kn, "K": K, "N_out": N_out, "d": d, "nnz": R * M * d, "root": root,
            "valued": valued, "scaled": scaled, "array": array}


def cases():
    """name -> case. ``array``: (rows, row elements) of the array the case is about."""
    last = band.offset_of(7)
    out = [
        _case("x16 gathered X at the entry's limit", "rel", "bf16", 1, LIM // 256 - last, 256, 8, 8, valued=True, array=("X", 256)),
        _case("x16 root X at the entry's limit", "linear", "fp16", 1, LIM // 256 - last, 256, 8, 8, root=True, scaled=True, array=("root", 256)),
        _case("f32 gathered X and root X past 2^32 bytes", "f32", "fp32", 1, _past(256, 4), 256, 8, 8, root=True, scaled=True, array=("root", 256)),
        _case("f32 gathered X at the entry's limit", "f32", "fp32", 1, LIM // 256 - last, 256, 8, 8, valued=True, array=("X", 256)),
        _case("f32 out past 2^32 bytes", "f32", "fp32", 1, _past(256, 4), 4, 256, 8, scaled=True, array=("out", 256)),
        _case("wgrad grad_out at the entry's limit", "wgrad", "bf16", 1, LIM // 256, 8, 256, 8, valued=True, array=("grad_out", 256)),
        _case("x16 R M large, M K small", "rel", "fp16", 17, 1 << 22, 8, 8, 2, root=True, scaled=True, array=("row_scale", 1)),
        _case("wgrad R M large, M K small", "wgrad", "bf16", 17, 1 << 22, 8, 8, 2, scaled=True, array=("row_scale", 1)),
    ]
    return {c["name"]: c for c in out}


def array_rows(c):
    name = c["array"][0]
    return {"X": c["Kn"], "out": c["M"], "root": c["M"], "grad_out": c["M"], "row_scale": c["R"] * c["M"]}[name]


def marked_rows(c):
    """The output rows (0 <= i < M) whose windows a case compares: the rows that touch a marked row of the case's array, and the last."""
    name, width = c["array"]
    elem = 4 if name == "row_scale" else ES[c["dt"]]
    marks = lo.marked(array_rows(c), width, elem)
    if name == "row_scale":
        marks = [m % c["M"] for m in marks]
    return sorted({min(max(m, 0), c["M"] - 1) for m in marks} | {c["M"] - 1})


def memory_needed(c):
    """Bytes of the operands, the result and the sliced reference's transients (an upper estimate)."""
    es = ES[c["dt"]]
    dense = c["Kn"] * c["K"] * es + c["M"] * c["N_out"] * es + (c["M"] * c["K"] * es if c["root"] else 0)
    return int(1.5 * (dense + c["nnz"] * 8 + c["R"] * c["M"] * 8)) + (2 << 30)


def route(c, chunks=None):
    from gespmm_amd import _lib

    args = (c["R"], c["M"], c["Kn"], c["K"], c["N_out"], c["nnz"])
    if c["op"] == "linear":
        return _lib.spmm_linear_route_x16(*args[1:], 16)
    if c["op"] == "rel":
        return _lib.spmm_relational_route_x16(*args, 16)
    if c["op"] == "f32":
        return _lib.spmm_relational_route_f32(*args, 16)
    return _lib.spmm_relational_wgrad_route_x16(*args, _lib.spmm_relational_wgrad_chunks(c["R"], c["M"], c["K"], c["N_out"]) if chunks is None
                                                else chunks, 16)


# ---- closed forms (int64 tensors on any device) ----------------------------------------------------------------------------------------

def x_at(c, k, K):
    return ((c * K + k) % 7) % 3 - 1


def root_at(i, k, K):
    return ((3 * i * K + k) % 5) % 3 - 1


def value_at(e):
    return 1 + e % 2


def scale2_at(s):
    """TWICE the row_scale of stacked row s: 1, 2 or 4."""
    return 1 << (s % 3)


def weights(R, N_out, K, terms=4, device="cpu"):
    """int64 [R, N_out, K]"""
    W = torch.zeros(R, N_out, K, dtype=torch.int64, device=device)
    r = torch.arange(R, device=device).view(R, 1).expand(R, N_out)
    n = torch.arange(N_out, device=device).view(1, N_out).expand(R, N_out)
    for t in range(terms):
        W[r, n, (5 * n + 3 * r + 7 * t) % K] = 1 - 2 * ((t + n) % 2)
    return W


def bias_at(n):
    return n % 7 - 3


def grad_rows(c):
    """The rows of grad_out that hold non-zeros (+-1 in every column): its marked rows, the first row and the row before the last — at
    most five, so an element of grad_W is a sum of five H_r rows and stays exact in bf16."""
    return sorted(set(lo.marked(c["M"], c["N_out"], ES[c["dt"]])) | {0, max(c["M"] - 2, 0)})


def grad_at(i, n):
    return 1 - 2 * ((i + n) % 2)


def dense(fn, r0, r1, K, device="cpu"):
    """int64 [r1 - r0, K] of fn(row, k, K)"""
    i = torch.arange(r0, r1, device=device, dtype=torch.int64).view(-1, 1)
    k = torch.arange(K, device=device, dtype=torch.int64).view(1, -1)
    return fn(i, k, K)


def ref_aggregate2(c, r, i0, i1, device="cpu"):
    """int64 [i1 - i0, K]: TWICE rows i0 .. i1 of H_r (the factor keeps row_scale = 0.5 an integer). The closed form of X is evaluated
    once for rows i0 .. i1 + o_{d-1}; entry j of every row is a shifted slice of it."""
    d, K, M, n = c["d"], c["K"], c["M"], i1 - i0
    X = dense(x_at, i0, i1 + band.offset_of(d - 1), K, device)
    i = torch.arange(i0, i1, device=device, dtype=torch.int64).view(-1, 1)
    H = torch.zeros(n, K, dtype=torch.int64, device=device)
    for j in range(d):
        o = band.offset_of(j)
        H += X[o:o + n] * (value_at((r * M + i) * d + j) if c["valued"] else 1)
    return H * (scale2_at(r * M + i) if c["scaled"] else 2)


def ref_forward2(c, i0, i1, device="cpu"):
    """int64 [i1 - i0, N_out]: TWICE rows i0 .. i1 of the forward's result."""
    W = weights(c["R"], c["N_out"], c["K"], device=device).double()  # (float64 products of small integers: exact, and a GEMM)
    out = sum(ref_aggregate2(c, r, i0, i1, device).double() @ W[r].t() for r in range(c["R"]))
    if c["root"]:
        out = out + 2 * dense(root_at, i0, i1, c["K"], device).double() @ weights(1, c["N_out"], c["K"], terms=2, device=device)[0].double().t()
    n = torch.arange(c["N_out"], device=device, dtype=torch.int64)
    return out.to(torch.int64) + 2 * bias_at(n)


def ref_wgrad2(c, device="cpu"):
    """int64 [R, N_out, K]: TWICE grad_W — only the rows of ``grad_rows`` contribute."""
    n = torch.arange(c["N_out"], device=device, dtype=torch.int64).view(-1, 1)
    out = torch.zeros(c["R"], c["N_out"], c["K"], dtype=torch.int64, device=device)
    for r in range(c["R"]):
        for i in grad_rows(c):
            out[r] += grad_at(i, n) * ref_aggregate2(c, r, i, i + 1, device)
    return out
