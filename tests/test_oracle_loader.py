"""The oracle loader against the reference's own recorded facts (the pin), hand-made
edge cases, and the reference's mmio.hpp parser (built from the reference checkout; its answers
are recorded in tests/golden/ref_lines.json for machines without it: tests/ref_lines.py)."""
import glob
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN

GRAPHS = ("cora", "citeseer", "pubmed")


@pytest.mark.parametrize("g", GRAPHS)
def test_bundled_matches_reference_loader_facts(oracle, known_answers, g):
    """M / nnz / first / last / max-degree as the unmodified reference loader produced
    them — and sortedness, no self-loops, no duplicates."""
    coo = oracle.read_mtx(os.path.join(GOLDEN, g + ".mtx"))
    f = known_answers["survey"][g]
    assert coo["rc"] == 0
    assert coo["nrows"] == f["M"] and coo["ncols"] == f["M"]
    assert coo["nnz"] == f["nnz"]
    assert [int(coo["row"][0]), int(coo["col"][0])] == f["first"]
    assert [int(coo["row"][-1]), int(coo["col"][-1])] == f["last"]
    assert int(np.bincount(coo["row"]).max()) == f["max_degree"]
    key = coo["row"].astype(np.int64) * coo["ncols"] + coo["col"]
    assert np.all(np.diff(key) > 0), "sorted by (row, col) with no duplicates"
    assert not np.any(coo["row"] == coo["col"]), "symmetric expansion drops self-loops"
    # symmetric pattern
    tkey = np.sort(coo["col"].astype(np.int64) * coo["ncols"] + coo["row"])
    assert np.array_equal(tkey, key)


@pytest.mark.parametrize("g", GRAPHS)
def test_bundled_nnz_matches_reference_spreadsheet(oracle, known_answers, g):
    """matrix_id_info.xlsx records time and GFLOP/s of the reference run on this file;
    time*throughput = 2*nnz*N/1e6 gives the nnz the reference loader fed its kernels."""
    coo = oracle.read_mtx(os.path.join(GOLDEN, g + ".mtx"))
    implied = known_answers["xlsx"][g]["implied_nnz"]
    assert abs(implied - coo["nnz"]) < 1.0, (implied, coo["nnz"])


def test_handmade_cases(oracle):
    with open(os.path.join(GOLDEN, "mtx_expected.json")) as f:
        expected = json.load(f)
    assert expected
    for name, exp in expected.items():
        got = oracle.read_mtx(os.path.join(GOLDEN, "mtx", name))
        if exp["rc"] == "format":
            assert got["rc"] in (2, 3), name
            continue
        assert got["rc"] == 0, name
        assert got["nrows"] == exp["nrows"] and got["ncols"] == exp["ncols"], name
        assert got["row"].tolist() == exp["row"], name
        assert got["col"].tolist() == exp["col"], name
        assert np.allclose(got["val"], np.array(exp["val"], dtype=np.float32), rtol=0, atol=0), name


def test_missing_file(oracle, tmp_path):
    assert oracle.read_mtx(tmp_path / "nope.mtx")["rc"] == 1


def test_header_agrees_with_reference_mmio(oracle):
    """oracle/_ref/mmio_probe is the reference's util/mmio.hpp compiled where it lies (or what it answered: tests/ref_lines.py)."""
    from ref_lines import REF

    files = sorted(glob.glob(os.path.join(GOLDEN, "*.mtx")) + glob.glob(os.path.join(GOLDEN, "mtx", "*.mtx")))
    checked = 0
    for path in files:
        ref = REF.mmio_probe(path)
        got = oracle.read_mtx(path)
        if ref["banner_rc"] != 0:
            assert got["rc"] != 0, path
            continue
        if ref["typecode"][2] == "C":  # complex: the reference parses the header, we reject the file
            assert got["rc"] != 0
            continue
        assert got["rc"] == 0, path
        assert (got["nrows"], got["ncols"]) == (ref["M"], ref["N"]), path
        checked += 1
    assert checked >= 8


def test_coo_to_csr_restated_loop(oracle):
    rng = np.random.RandomState(3)
    nrows, nnz = 37, 500
    row = rng.randint(0, nrows, nnz).astype(np.int32)
    col = rng.randint(0, 50, nnz).astype(np.int32)
    val = rng.rand(nnz).astype(np.float32)
    indptr, indices, data = oracle.coo_to_csr(nrows, row, col, val)
    assert indptr[0] == 0 and indptr[-1] == nnz
    assert np.array_equal(np.diff(indptr), np.bincount(row, minlength=nrows))
    for r in range(nrows):  # input order kept inside a row
        sel = np.nonzero(row == r)[0]
        assert np.array_equal(indices[indptr[r]:indptr[r + 1]], col[sel])
        assert np.array_equal(data[indptr[r]:indptr[r + 1]], val[sel])
    _, _, ones = oracle.coo_to_csr(nrows, row, col, None)
    assert np.all(ones == 1.0)  # spmm_test.cu:574
