"""Patterns, shapes and operands of the 16-bit GATv2 score tests (plain module: tests/test_gatv2_x16_host.py builds the same host
arrays tests/test_gpu_gatv2_x16.py sends to the device). Everything is seeded and a few hundred rows at most."""
import numpy as np
import torch

from helpers import edge_case_csr
from test_gat_softmax_host import csc_of

DTYPES = (torch.float16, torch.bfloat16)
# (H, F) -> the forward's V on 16-byte aligned operands: V = 1 (odd F), 2, 4, 8, several vectors per slice (2, 24), several trips at
# V = 2 (2, 130: W = 16, 32 elements a trip) and two trips at V = 8, W = 64 (1, 520: 512 elements a trip).
SHAPES = {(1, 1): 1, (3, 5): 1, (2, 6): 2, (4, 4): 4, (8, 8): 8, (2, 24): 8, (2, 130): 2, (1, 520): 8}
SLOPES = (None, 0.25, 0.2)
EXACT_SLOPES = (None, 0.25)  # slope 1 or 2^-2: every product of small integers stays exact


def _finish(G):
    colptr, order = csc_of(G["rowptr"], G["colind"], G["K"])
    rows = np.repeat(np.arange(G["M"], dtype=np.int32), np.diff(G["rowptr"]))
    G.update(rows_h=rows, colptr_h=colptr, order_h=order, rowind_h=rows[order])
    return G


def gaps_pattern():
    """314 rows, 97 columns, 1345 entries. Row 0 has 3 entries, rows 1 .. 300 are empty — more than 256 consecutive empty rows inside
    the window of the wavefront that owns entry 0, whatever its epw — row 301 has 300 entries (longer than 4 W for every W up to 64),
    and nnz = 1345 = 1 mod 64, 32, 21, 16 and 8: one entry past a wavefront's epw for every epw the tested shapes resolve to. Columns
    90 .. 96 are never named (empty segments of the column pass), column 7 is named 400 times (a segment longer than 4 W there),
    and repeated columns inside a row are everywhere."""
    degs = [3] + [0] * 300 + [300, 0, 1, 65, 129, 200, 7, 33, 64, 63, 2, 0, 478]
    rowptr = np.zeros(len(degs) + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(degs)
    nnz = int(rowptr[-1])
    rng = np.random.RandomState(11)
    colind = rng.randint(0, 90, size=nnz).astype(np.int32)
    colind[rng.permutation(nnz)[:400]] = 7
    return _finish({"rowptr": rowptr, "colind": colind, "M": len(degs), "K": 97, "nnz": nnz})


def edge_pattern():
    """helpers.edge_case_csr: 21 rows of 0 .. 200 entries, 301 columns (many never named), unsorted and repeated columns."""
    return _finish(dict(edge_case_csr()))


def check_patterns(pats):
    """What the patterns are there for, asserted."""
    G = pats["gaps"]
    d, c = np.diff(G["rowptr"]), np.diff(G["colptr_h"])
    assert G["M"] == 314 and G["nnz"] == 1345 and all(G["nnz"] % e == 1 for e in (64, 32, 21, 16, 8))
    assert d[0] > 0 and (d[1:301] == 0).all() and d[301] > 4 * 64 and (c == 0).any() and c.max() > 4 * 64
    assert any(np.unique(G["colind"][a:b]).size < b - a for a, b in zip(G["rowptr"][:-1], G["rowptr"][1:]))
    E = pats["edge"]
    assert (np.diff(E["rowptr"]) == 0).any() and (np.diff(E["colptr_h"]) == 0).any()


def narrow(a, dt):
    """fp32 host array -> (16-bit torch tensor on the host, its exact fp32 widening as a numpy array)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt)
    return t, t.float().numpy()


def operands(G, H, F, kind, dt):
    """Host operands of one case -> dict: 16-bit tensors ``xl``, ``xr``; fp32 arrays ``att``, ``gs``; and ``wide``, the dict of fp32
    numpy arrays (xl, xr widened exactly) the float64 restatement and the fp32 entry points take. 'int': xl, xr in [-4, 4], att and
    grad_score in [-2, 2], all integers — both 16-bit types hold them; 'real': uniform in +-1 (att, grad_score: +-2), rounded to dt."""
    seed = 1000 + 100 * H + F + G["nnz"] % 17
    rng = np.random.RandomState(seed)
    if kind == "int":
        xl, xr = rng.randint(-4, 5, size=(G["M"], H, F)), rng.randint(-4, 5, size=(G["K"], H, F))
        att, gs = rng.randint(-2, 3, size=(H, F)), rng.randint(-2, 3, size=(G["nnz"], H))
    else:
        xl, xr = 2 * rng.rand(G["M"], H, F) - 1, 2 * rng.rand(G["K"], H, F) - 1
        att, gs = 4 * rng.rand(H, F) - 2, 4 * rng.rand(G["nnz"], H) - 2
    xl16, xlw = narrow(xl, dt)
    xr16, xrw = narrow(xr, dt)
    att, gs = att.astype(np.float32), gs.astype(np.float32)
    if kind == "int":
        assert np.array_equal(xlw, xl) and np.array_equal(xrw, xr)
    return {"xl": xl16, "xr": xr16, "att": att, "gs": gs, "wide": {"xl": xlw, "xr": xrw, "att": att, "gs": gs}}
