"""THE PIN: oracle/gespmm_oracle.c and the product's host code against the REFERENCE'S OWN
LINES, compiled from the reference checkout by oracle/make_ref.sh (util/util.hpp:57-333 + mmio.hpp;
spmm_test.cu:558-581 COO->CSR, :592-594 B init, :596-604 CPU golden loop). Bit for bit.

The lines answer through tests/ref_lines.py: live from oracle/_ref/ where it was built, else from
what they returned on these inputs (tests/golden/ref_lines.json) — the pin holds on every machine.
The inputs of each comparison are the oracle's own arrays, each first checked equal to the reference's.
"""
import glob
import os

import numpy as np
import pytest

from helpers import GOLDEN, bits, edge_case_csr
from ref_lines import REF, fp

GRAPHS = ("cora", "citeseer", "pubmed")
WIDTHS = (3, 32, 128, 512)


def _fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "mtx", "*.mtx")))


@pytest.fixture(scope="module")
def ref_bundled(oracle):
    """The reference's answers on the bundled graphs, and the oracle's arrays that equal them (the inputs downstream)."""
    out = {}
    for g in GRAPHS:
        path = os.path.join(GOLDEN, g + ".mtx")
        coo = REF.read_mtx(path)
        assert coo["rc"] == 0 and coo["tuples"] == coo["nvals"]
        mine = oracle.read_mtx(path)
        assert (fp(mine["row"]), fp(mine["col"])) == (coo["row"], coo["col"])
        csr = REF.coo_to_csr(coo["nrows"], coo["ncols"], mine["row"], mine["col"])
        indptr, indices, data = oracle.coo_to_csr(coo["nrows"], mine["row"], mine["col"])
        assert (fp(indptr), fp(indices), fp(data)) == (csr["indptr"], csr["indices"], csr["data"])
        out[g] = dict(coo=coo, csr=csr, indptr=indptr, indices=indices, data=data)
    return out


@pytest.mark.parametrize("g", GRAPHS)
def test_loader_and_coo_to_csr_equal_the_reference_on_bundled_graphs(oracle, pkg, ref_bundled, g):
    from gespmm_amd import graphs

    path = os.path.join(GOLDEN, g + ".mtx")
    ref = ref_bundled[g]
    for name, got in (("oracle", oracle.read_mtx(path)), ("product", graphs.read_mtx(path))):
        assert (got["nrows"], got["ncols"], got["nnz"]) == (ref["coo"]["nrows"], ref["coo"]["ncols"],
                                                             ref["coo"]["nvals"]), name
        assert fp(got["row"]) == ref["coo"]["row"], name
        assert fp(got["col"]) == ref["coo"]["col"], name
        assert fp(got["val"]) == ref["coo"]["val"], name  # float32 bits
    coo, csr = oracle.read_mtx(path), ref["csr"]
    ip, ix, d = oracle.coo_to_csr(coo["nrows"], coo["row"], coo["col"])
    assert fp(ip) == csr["indptr"] and fp(ix) == csr["indices"] and fp(d) == csr["data"]
    ip, ix, d = graphs.coo_to_csr(coo["nrows"], coo["ncols"], coo["row"], coo["col"])
    assert fp(ip) == csr["indptr"] and fp(ix) == csr["indices"]
    assert csr["data"] == fp(np.ones(coo["nnz"], dtype=np.float32))  # spmm_test.cu:574


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("g", GRAPHS)
def test_golden_loop_and_B_init_equal_the_reference(oracle, ref_bundled, g, N):
    ref = ref_bundled[g]
    K = ref["coo"]["ncols"]
    B = oracle.fill_B_rand(1, K, N)
    assert fp(B) == REF.fill_B(1, N, K)
    want = REF.golden(ref["indptr"], ref["indices"], ref["data"], B)
    got = oracle.spmm(ref["indptr"], ref["indices"], None, B, mode="golden")
    assert fp(got) == want
    # the OpenMP form used as the all-cores CPU baseline has the same loop body
    assert fp(oracle.spmm(ref["indptr"], ref["indices"], None, B, mode="omp")) == want
    # valued (A_data is a parameter of the reference's loop; the driver sets it to 1)
    val = oracle.hash_val(ref["indices"].shape[0], seed=7)
    want = REF.golden(ref["indptr"], ref["indices"], val, B)
    got = oracle.spmm(ref["indptr"], ref["indices"], val, B, mode="golden")
    assert fp(got) == want


@pytest.mark.parametrize("N", (1, 3, 41, 64, 100, 128))
def test_golden_loop_on_edge_shapes(oracle, N):
    g = edge_case_csr(seed=3)
    B = oracle.hash_B(g["K"], N, seed=5)
    val = oracle.hash_val(g["nnz"], seed=11)
    for v in (np.ones(g["nnz"], dtype=np.float32), val):
        want = REF.golden(g["rowptr"], g["colind"], v, B)
        got = oracle.spmm(g["rowptr"], g["colind"], v, B, mode="golden")
        assert fp(got) == want


def test_handmade_files_against_the_reference_loader(oracle, pkg):
    """Every tests/golden/mtx fixture through the reference's readMtx (as a process).
    Two deliberate deviations, both asserted here so they stay visible:
      * complex files: the reference reads NOTHING and returns 0 with nvals = the header's
        count and empty vectors (util.hpp:315-320) — spmm_test would then index empty vectors;
        oracle and product reject the file instead;
      * symmetric files with entries removed by compaction: the reference moves row/col but not
        val (util.hpp:268-277), leaving values misaligned; oracle and product keep each value
        with its entry. spmm_test overwrites the values with 1 (spmm_test.cu:574) either way."""
    from gespmm_amd import graphs

    seen = set()
    for path in _fixture_files():
        name = os.path.basename(path)
        ref = REF.read_mtx(path)
        mine = oracle.read_mtx(path)
        if ref["rc"] != 0:  # exit(1): bad banner / size line
            assert mine["rc"] != 0, name
            seen.add("exit")
            continue
        if ref["tuples"] == 0 and ref["nvals"] > 0 and mine["rc"] != 0:
            assert "complex" in name
            seen.add("complex")
            continue
        assert mine["rc"] == 0, name
        n = mine["nnz"]
        # short files: the reference keeps nvals from the header and returns what it read
        assert ref["tuples"] == n, name
        assert (mine["nrows"], mine["ncols"]) == (ref["nrows"], ref["ncols"]), name
        assert fp(mine["row"]) == ref["row"] and fp(mine["col"]) == ref["col"], name
        prod = graphs.read_mtx(path)
        assert fp(prod["row"]) == ref["row"] and fp(prod["col"]) == ref["col"], name
        if fp(mine["val"]) == ref["val"]:
            seen.add("vals-equal")
        else:
            assert "symmetric" in name, name  # the compaction quirk only
            assert sorted(mine["val"].tolist()) != [] and np.array_equal(bits(prod["val"]), bits(mine["val"]))
            seen.add("quirk")
    assert {"exit", "complex", "vals-equal", "quirk"} <= seen


def _write_random_mtx(path, rng, M, K, n, field, symmetric):
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate %s %s\n%% seeded random fixture\n%d %d %d\n"
                % (field, "symmetric" if symmetric else "general", M, K, n))
        for _ in range(n):
            r = rng.randint(1, M + 1)
            c = rng.randint(1, (r if symmetric else K) + 1)  # lower triangle incl. diagonal; repeats happen
            if field == "pattern":
                f.write("%d %d\n" % (r, c))
            elif field == "integer":
                f.write("%d %d %d\n" % (r, c, rng.randint(-9, 10)))
            else:
                f.write("%d %d %.3f\n" % (r, c, rng.uniform(-2, 2)))


@pytest.mark.parametrize("seed", range(6))
def test_random_files_against_the_reference_loader(oracle, pkg, tmp_path, seed):
    """Seeded random coordinate files — duplicates, self loops, empty rows, rectangular — through
    readMtx + the COO->CSR lines of the reference vs oracle and product."""
    from gespmm_amd import graphs

    rng = np.random.RandomState(100 + seed)
    symmetric = seed % 2 == 0
    field = ("pattern", "integer", "real")[seed % 3]
    M = int(rng.randint(5, 400))
    K = M if symmetric else int(rng.randint(5, 400))
    n = int(rng.randint(1, 6 * M))
    path = str(tmp_path / ("r%d.mtx" % seed))
    _write_random_mtx(path, rng, M, K, n, field, symmetric)
    ref = REF.read_mtx(path)
    assert ref["rc"] == 0
    for got in (oracle.read_mtx(path), graphs.read_mtx(path)):
        assert got["nnz"] == ref["nvals"] == ref["tuples"]
        # general files: the reference's sort leaves the order among equal (row, col) unspecified
        # (util.hpp:57-73 compares row and col only) — rows/cols are still determined
        assert fp(got["row"]) == ref["row"] and fp(got["col"]) == ref["col"]
    mine = oracle.read_mtx(path)
    row, col = mine["row"], mine["col"]  # == the reference's (above)
    rcsr = REF.coo_to_csr(ref["nrows"], ref["ncols"], row, col)
    oip, oix, _ = oracle.coo_to_csr(ref["nrows"], row, col)
    pip_, pix, _ = graphs.coo_to_csr(ref["nrows"], ref["ncols"], row, col)
    assert fp(oip) == rcsr["indptr"] and fp(oix) == rcsr["indices"]
    assert fp(pip_) == rcsr["indptr"] and fp(pix) == rcsr["indices"]
    B = oracle.fill_B_rand(seed + 1, K, 7)
    assert fp(B) == REF.fill_B(seed + 1, 7, K)
    ones = np.ones(oix.shape[0], dtype=np.float32)
    assert fp(oracle.spmm(oip, oix, None, B, mode="golden")) == REF.golden(oip, oix, ones, B)


def test_committed_vectors_are_the_reference_lines_output(oracle, ref_bundled):
    """tests/golden/spmm_checksums.json: the `unweighted_golden` / `valued_golden` columns are
    outputs of the reference's own loader + COO->CSR + golden loop (tests/golden/make_golden.py).
    Re-derive them here from oracle/_ref, and check the oracle reproduces them — so the committed
    vectors pin the oracle wherever the reference checkout is not available."""
    import json

    with open(os.path.join(GOLDEN, "spmm_checksums.json")) as f:
        chk = json.load(f)["graphs"]
    for g in GRAPHS:
        ref = ref_bundled[g]
        val = oracle.hash_val(ref["indices"].shape[0], seed=7)
        for N in ("3", "41", "128"):
            B = oracle.hash_B(ref["coo"]["ncols"], int(N), seed=1)
            for mode, v in (("unweighted_golden", ref["data"]), ("valued_golden", val)):
                exp = chk[g][N][mode]
                C = oracle.spmm(ref["indptr"], ref["indices"], v, B, mode="golden")
                assert fp(C) == REF.golden(ref["indptr"], ref["indices"], v, B), (g, N, mode)  # the reference's C, bit for bit
                assert int(np.bitwise_xor.reduce(bits(C).ravel())) == exp["xor"], (g, N, mode)
                assert float(C.astype(np.float64).sum()) == exp["sum"]
                for r, c, b in exp["samples"]:
                    assert int(bits(C[r, c:c + 1])[0]) == b
