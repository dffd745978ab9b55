"""Host restatement of the two chains of include/gespmm.h: the max reducer with argmax and its gradient. numpy, float32, the comparisons
exactly as the header writes them; a row is vectorised over its columns (every column runs the same chain), never over its entries."""
import numpy as np


def max_arg_forward(rowptr, colind, B, empty_value):
    """acc = empty; a = -1; for p ascending: b = B[colind[p], c]; if (b > acc) { acc = b; a = p; }  ->  (C f32[M, N], arg int32[M, N])"""
    B = np.asarray(B, dtype=np.float32)
    M, N = len(rowptr) - 1, B.shape[1]
    C = np.full((M, N), np.float32(empty_value), dtype=np.float32)
    arg = np.full((M, N), -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for r in range(M):
            acc, a = C[r], arg[r]  # views
            for p in range(int(rowptr[r]), int(rowptr[r + 1])):
                b = B[colind[p]]
                win = b > acc  # false for NaN and for equal values (+0 == -0): the first one stays, with its bits
                acc[win] = b[win]
                a[win] = p
    return C, arg


def max_backward(colptr, rowind, order, arg, grad_out, K):
    """g = +0; for q ascending: r = rowind[q]; if (arg[r, c] == order[q]) g = g + grad_out[r, c]  ->  grad_B f32[K, N]"""
    grad_out = np.asarray(grad_out, dtype=np.float32)
    N = grad_out.shape[1]
    grad_B = np.zeros((K, N), dtype=np.float32)
    for k in range(K):
        g = grad_B[k]
        for q in range(int(colptr[k]), int(colptr[k + 1])):
            r = rowind[q]
            hit = arg[r] == order[q]
            g[hit] = g[hit] + grad_out[r][hit]  # plain fp32 add
    return grad_B


def transpose(rowptr, colind, K):
    """(colptr, rowind, order) of a CSR pattern, rows ascending inside a column and repeated entries in CSR order: CSC position q is
    CSR entry order[q] — what graphs.transpose_csr(..., return_order=True) gives, as int32 numpy arrays."""
    rowptr, colind = np.asarray(rowptr), np.asarray(colind)
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(rowptr))
    order = np.argsort(colind, kind="stable").astype(np.int32)
    colptr = np.zeros(K + 1, dtype=np.int32)
    colptr[1:] = np.cumsum(np.bincount(colind, minlength=K))
    return colptr, rows[order].astype(np.int32), order


def tied_words(rowptr, colind, B, C, arg):
    """bool[M, N]: the output word has a winner AND a later entry of the row holds an equal value (the first-position rule decided)."""
    M, N = C.shape
    tied = np.zeros((M, N), dtype=bool)
    for r in range(M):
        lo, hi = int(rowptr[r]), int(rowptr[r + 1])
        if hi - lo >= 2:
            vals = B[colind[lo:hi]]
            tied[r] = (arg[r] >= 0) & ((vals == C[r]).sum(0) >= 2)
    return tied
