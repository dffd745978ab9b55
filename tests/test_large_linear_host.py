"""large_linear.py without a device: every case's array is JUST past its switch (or at the entry's limit), its route answers 1, the
first size past every entry's limit answers ERANGE (-3), the marked rows are where the bytes are, and the closed-form references agree
with a dense float64 product on a small instance of every case."""
import numpy as np
import pytest
import torch

import band
import large_linear as ll

CASES = ll.cases()
NAMES = pytest.mark.parametrize("name", sorted(CASES))


@NAMES
def test_sizes_cross_their_switch_and_are_served(pkg, name):
    c = CASES[name]
    arr, width = c["array"]
    rows = ll.array_rows(c)
    elem = 4 if arr == "row_scale" else ll.ES[c["dt"]]
    if "limit" in name:
        assert rows * width <= ll.LIM and rows * width * elem > 1 << 31
        assert (c["Kn"] + 1) * c["K"] > ll.LIM or (c["M"] + 1) * c["N_out"] > ll.LIM  # one more row is refused
    elif arr == "row_scale":
        assert c["R"] * c["M"] * elem > 1 << 28 and c["M"] * c["K"] * ll.ES[c["dt"]] <= 1 << 26  # R M large, M K small
        assert (c["R"] - 1) * c["M"] + c["M"] - 1 > 1 << 26
    else:
        assert (rows - 1) * width * elem <= 1 << 32 < rows * width * elem  # the last row holds byte 2^32
    assert ll.route(c) == 1
    marks = ll.marked_rows(c)
    assert marks[-1] == c["M"] - 1 and all(0 <= m < c["M"] for m in marks)
    if arr != "row_scale":
        assert min((1 << 31) // (width * elem), c["M"] - 1) in marks
        assert len(marks) == (3 if rows * width * elem > 1 << 32 and (1 << 32) // (width * elem) < c["M"] - 1 else 2)
    assert ll.memory_needed(c) < 48 << 30


@pytest.mark.parametrize("op", ("linear", "rel", "f32", "wgrad"))
def test_the_first_size_past_an_entrys_limit_is_refused(pkg, op):
    from gespmm_amd import _lib

    K = 4 if op == "f32" else 8
    fits = dict(R=1, M=64, Kn=ll.LIM // K, K=K, N_out=8, nnz=8, d=1, op=op)
    assert ll.route(fits, chunks=1) == 1
    for grow in (dict(Kn=ll.LIM // K + 1), dict(M=ll.LIM // K + 1), dict(M=ll.LIM // 256 + 1, N_out=256), dict(nnz=ll.LIM + 1)):
        with pytest.raises(_lib.GespmmError) as info:
            ll.route(dict(fits, **grow), chunks=1)
        assert info.value.code == -3, grow
    if op != "linear":
        with pytest.raises(_lib.GespmmError) as info:
            ll.route(dict(fits, R=17, M=ll.LIM // (17 * K) + 1), chunks=1)
        assert info.value.code == -3


@NAMES
def test_closed_forms_against_a_dense_product(pkg, name):
    c = dict(CASES[name])
    c["M"] = 200
    c["Kn"] = c["M"] + band.offset_of(c["d"] - 1)
    R, M, Kn, K, N_out, d = (c[k] for k in ("R", "M", "Kn", "K", "N_out", "d"))
    rp, ci = band.csr(M, d)
    A = np.zeros((R, M, Kn))
    e = np.arange(R * M * d)
    vals = ll.value_at(e) if c["valued"] else np.ones(R * M * d)
    np.add.at(A, (e // (M * d), (e // d) % M, np.tile(ci.numpy(), R)), vals)
    X = ll.dense(ll.x_at, 0, Kn, K).double().numpy()
    H = A @ X
    if c["scaled"]:
        H = H * (ll.scale2_at(np.arange(R * M)).reshape(R, M, 1) / 2.0)
    W = ll.weights(R, N_out, K).double().numpy()
    assert (np.abs(W).sum(axis=(0, 2)) <= 4 * R).all() and set(np.unique(W)) <= {-1.0, 0.0, 1.0} and set(np.unique(X)) == {-1.0, 0.0, 1.0}
    if c["op"] == "wgrad":
        go = np.zeros((M, N_out))
        for i in ll.grad_rows(c):
            go[i] = ll.grad_at(i, np.arange(N_out))
        want = np.einsum("mn,rmk->rnk", go, H)
        assert np.array_equal(ll.ref_wgrad2(c).double().numpy(), 2 * want)
        assert np.abs(2 * want).max() <= 256
        return
    want = np.einsum("rmk,rnk->mn", H, W) + ll.bias_at(np.arange(N_out))
    if c["root"]:
        want = want + ll.dense(ll.root_at, 0, M, K).double().numpy() @ ll.weights(1, N_out, K, terms=2)[0].double().numpy().T
    got = torch.cat([ll.ref_forward2(c, 0, 77), ll.ref_forward2(c, 77, M)]).double().numpy()
    assert np.array_equal(got, 2 * want)
    assert np.abs(got).max() <= (256 if c["dt"] == "bf16" else 2048)
