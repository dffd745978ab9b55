"""linear_cases.py without a device: the generator is deterministic, the fixed case lists reach every template instance of the four
kernel files, every relation law and every unserved variant occurs for every op, at least 3/4 of all output rows (elements, for the
weight gradient) are exact-eligible on every dtype, and the comparison rejects every mutation of the reference on some case."""
import numpy as np
import pytest

import linear_cases as lc

OPS = pytest.mark.parametrize("op", lc.OPS)


def _served(op):
    return [c for c in lc.cases(op) if c["unserved"] is None]


@OPS
def test_the_generator_is_deterministic(pkg, op):
    a = lc.cases(op)
    rng = np.random.RandomState(lc.SEEDS[op])
    b = [lc.draw_case(op, i, rng) for i in range(len(_served(op)))]
    assert len(set(lc.case_id(c) for c in a)) == len(a)
    for x, y in zip(a, b):
        assert lc.case_id(x) == lc.case_id(y)
        for key in x:
            if isinstance(x[key], np.ndarray):
                assert np.array_equal(x[key], y[key]), key
            else:
                assert x[key] == y[key], key


def test_the_launch_rules_agree_with_the_library(pkg):
    from gespmm_amd import _lib

    for R, M, K, N_out in ((1, 1, 8, 1), (3, 301, 64, 32), (17, 300, 256, 256), (7, 129, 72, 34), (2, 4096, 8, 1), (5, 100000, 136, 47)):
        assert lc.wgrad_chunks(R, M, K, N_out) == _lib.spmm_relational_wgrad_chunks(R, M, K, N_out)
    for op, route in (("linear", lambda K, N: _lib.spmm_linear_route_x16(65, 5, K, N, 9, 16)),
                      ("rel", lambda K, N: _lib.spmm_relational_route_x16(3, 65, 5, K, N, 9, 16)),
                      ("f32", lambda K, N: _lib.spmm_relational_route_f32(3, 65, 5, K, N, 9, 16)),
                      ("wgrad", lambda K, N: _lib.spmm_relational_wgrad_route_x16(3, 65, 5, K, N, 9, 1, 16))):
        for K in sorted(set(lc.K16 + lc.K32 + (10, 5, 258, 260, 264))):
            for N_out in (1, 256, 257):
                assert route(K, N_out) == int(lc.served(op, K, N_out)), (op, K, N_out)


@OPS
def test_the_case_list_reaches_every_template_instance(pkg, op):
    served = _served(op)
    assert all(lc.served(op, c["K"], c["N_out"]) for c in served)
    got = {lc.reach(op, c, valued, dt) for c in served for valued in (False, True) for dt in lc.DTYPES[op]}
    both = (False, True)
    if op == "linear":
        want = {(dt, v) + geo for dt in lc.DTYPES[op] for v in both for geo in ((4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2))}
        assert len(want) == 24
    elif op == "rel":
        want = {(dt, v) + geo + (ns,) for dt in lc.DTYPES[op] for v in both for geo in ((4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2))
                for ns in (1, 2)}
        assert len(want) == 48
    elif op == "wgrad":
        want = {(dt, v, W, ns) for dt in lc.DTYPES[op] for v in both for W in (4, 8, 16, 32) for ns in (1, 2)}
        assert len(want) == 32
        assert {lc.stage_width(c["N_out"]) for c in served} == {8, 4, 2, 1}
        two = {sw > 32 for c in served for sw in lc.slab_widths(c["K"])}
        assert two == {False, True} and any(len({sw > 32 for sw in lc.slab_widths(c["K"])}) == 2 for c in served)
        for c in served:
            blocks = (c["M"] + 63) // 64
            cl = lc.chunk_list(c["R"], c["M"], c["K"], c["N_out"])
            assert cl[0] is None and 1 in cl and blocks in cl and all(1 <= x <= blocks for x in cl[1:])
        assert any(len(lc.chunk_list(c["R"], c["M"], c["K"], c["N_out"])) == 4 for c in served)  # one value in between
    else:
        want = {(v, W, ns) for v in both for W in (4, 8, 16, 32, 64) for ns in (1, 2)}
        assert len(want) == 20
        pads = {lc.f32_pad(c["K"]) for c in served}
        assert pads == {(False, False), (True, False), (True, True)}
        assert {c["K"] for c in served if lc.f32_pad(c["K"])[1]} == {12, 28, 60, 124, 252}
    assert got == want, sorted(want - got)
    ks = lc.K32 if op == "f32" else lc.K16
    assert {c["K"] for c in served} == set(ks) and {c["N_out"] for c in served} == set(lc.NOUTS)
    print("\n".join("%-60s %s" % (lc.case_id(c), sorted({lc.reach(op, c, v, lc.DTYPES[op][0])[1:] for v in both})) for c in served))


@OPS
def test_every_law_switch_and_unserved_variant_occurs(pkg, op):
    from gespmm_amd import _lib

    all_cases = lc.cases(op)
    served = _served(op)
    assert {c["law"] for c in served} == set(lc.LAWS)
    assert {u: sum(c["unserved"] == u for c in all_cases) for u in lc.UNSERVED} == {u: 2 for u in lc.UNSERVED}
    assert {c["row_scale"] is None for c in served} == {False, True}
    for name in lc.OPERANDS[op]:
        assert {c["offsets"][name] for c in served} == {0, 16}, name
    if op != "wgrad":
        assert {c["root"] is None for c in served} == {False, True} and {c["bias"] is None for c in served} == {False, True}
    assert {c["M"] for c in all_cases} <= set(lc.MS) and {c["Kn"] for c in all_cases} <= set(lc.KNS) and {c["R"] for c in all_cases} <= set(lc.RS)
    assert len({c["M"] for c in all_cases}) >= 6 and len({c["Kn"] for c in all_cases}) == 4
    if op != "linear":
        assert {c["R"] for c in all_cases} == set(lc.RS)
    assert any(c["nnz"] == 0 for c in served) and any(int(np.diff(c["rowptr"]).max()) == lc.HUB for c in served if c["nnz"])
    for c in served:  # the law holds on the arrays: a (block, relation) pair has an entry exactly where it is live
        rp = c["rowptr"]
        for r in range(c["R"]):
            for b in range(c["live"].shape[1]):
                lo, hi = r * c["M"] + b * 64, r * c["M"] + min((b + 1) * 64, c["M"])
                assert (rp[hi] > rp[lo]) == bool(c["live"][r, b]), (lc.case_id(c), r, b)
    for c in all_cases:
        al = min([16] + [o for o in c["offsets"].values() if o % 16])
        al = max(al, 4) if op == "f32" else al
        args = (c["R"], c["M"], c["Kn"], c["K"], c["N_out"], c["nnz"])
        route = {"linear": lambda: _lib.spmm_linear_route_x16(*args[1:], al), "rel": lambda: _lib.spmm_relational_route_x16(*args, al),
                 "f32": lambda: _lib.spmm_relational_route_f32(*args, al),
                 "wgrad": lambda: _lib.spmm_relational_wgrad_route_x16(*args, lc.wgrad_chunks(c["R"], c["M"], c["K"], c["N_out"]), al)}[op]()
        assert route == (1 if c["unserved"] is None else 0), lc.case_id(c)


@OPS
def test_three_quarters_of_all_rows_are_exact_eligible(pkg, op):
    for dt in lc.DTYPES[op]:
        for valued in (False, True):
            elig = total = 0
            for c in lc.cases(op):
                ref, eligible, _, _ = lc.reference(c, valued)
                lc.as_int64(ref, c)  # the reference is an integer of its grid
                e = eligible(dt)
                elig, total = elig + int(e.sum()), total + e.size
            print("%s %s valued=%s: %d of %d exact-eligible (%.4f)" % (op, dt, valued, elig, total, elig / total))
            assert 4 * elig >= 3 * total


@OPS
def test_the_comparison_rejects_every_mutation(pkg, op):
    rejected, names = {}, set()
    for c in _served(op):
        for valued in (False, True):
            ref, eligible, _, _ = lc.reference(c, valued)
            e = lc.broadcast_rows(eligible(lc.DTYPES[op][-1]), ref.shape)
            assert lc.agrees(c, ref.copy(), ref, e)
            for name, mutant in lc.mutants(c, valued).items():
                names.add(name)
                if not lc.agrees(c, mutant, ref, e):
                    rejected[name] = rejected.get(name, 0) + 1
    want = {"swapping two relations' weights", "transposing a 32 x 32 fragment", "exchanging the two k-halves", "dropping one CSR entry"}
    if op != "wgrad":
        want.add("dropping the skipped relation's root term")
    if op == "linear":
        want.discard("swapping two relations' weights")  # one relation
    print(op, rejected)
    assert want <= names and all(rejected.get(n, 0) >= 1 for n in want), rejected
