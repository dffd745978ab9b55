"""The auto-plan cache (csrc/auto_plan.cpp) where its callers really are: in-place changes that are ordered on the stream but
not waited for by the host, and several streams on one graph.

The contract (include/gespmm.h): every call returns the plain call's bits for the operands as they are at that point in stream order. The
ground truth of every call is the never-planned _cfg entry point on the same operands (itself checked against the oracle on sampled rows
for each state used). Outputs are prefilled with NaN and compared as bits. Streams are held back by torch.cuda._sleep — a bounded spin
on the device, never a host-released wait — and every test checks that its gate held, so a test cannot pass by finding the stream idle.
The statistics prove which path of the cache each call under test took."""
import numpy as np
import pytest
import torch

from helpers import (auto_call, gate, mismatches, nan_like_product, plain_product, sampled_rows_equal_oracle, sleep_cycles_per_ms,
                     stats_delta)

pytestmark = pytest.mark.gpu

GATE_MS = 50.0


@pytest.fixture(scope="module")
def sbm(pkg):
    from gespmm_amd import graphs

    return graphs.synthetic_graph("com-amazon-sbm", seed=42, device="cuda")


@pytest.fixture(scope="module")
def cpms(pkg):
    return sleep_cycles_per_ms()


@pytest.fixture()
def auto(pkg):
    from gespmm_amd import _lib

    _lib.set_auto_plan(0)
    yield _lib
    torch.cuda.synchronize()
    _lib.set_auto_plan(0)


def _eq(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _weights(oracle, nnz, seeds):
    return [torch.from_numpy(oracle.hash_val(nnz, seed=s)).cuda() for s in seeds]


def _pinned_plain(_lib, oracle, rp, ci, val, B):
    """The plain product, and that it is the oracle's on sampled rows."""
    C = plain_product(_lib, rp, ci, val, B)
    assert sampled_rows_equal_oracle(oracle, rp, ci, val, B, C, nrows=256), "the plain product differs from the oracle"
    return C


def test_value_flips_in_one_buffer_without_host_sync(auto, oracle, sbm, cpms):
    """Advisor finding 1: the plan is refreshed with the values of the moment while the host believes it holds the values of an earlier
    check's record. Traced: V2 (check fails, plain kernel), one host sync, gate, V1 (a refresh is due), gate, V2 — the last call must
    not run the plan with V1's values. (N = 128: at N = 32 the cost rule keeps this graph's storage order, so nothing is cached to race
    on; test_gpu_auto_plan.py::test_narrow_width_through_the_record_kernel allows for that.)"""
    _lib = auto
    N = 128
    rp, ci, K, nnz = sbm["rowptr"], sbm["colind"], sbm["K"], sbm["nnz"]
    V = _weights(oracle, nnz, (11, 12, 13))
    B = torch.from_numpy(oracle.hash_B(K, N, seed=14)).cuda()
    want = [_pinned_plain(_lib, oracle, rp, ci, v, B) for v in V]
    assert not _eq(want[0], want[1]) and not _eq(want[1], want[2])
    val = V[0].clone()
    torch.cuda.synchronize()
    st0 = _lib.auto_plan_stats()
    _lib.set_auto_plan(2)
    for _ in range(3):
        assert _eq(auto_call(_lib, rp, ci, val, B), want[0])
    d = stats_delta(_lib.auto_plan_stats(), st0)
    assert d["plans_created"] == 1 and d["calls_async"] == 1, ("the third call was not served asynchronously", d)

    outs = [nan_like_product(rp, B) for _ in range(3)]
    torch.cuda.synchronize()
    s_c1 = _lib.auto_plan_stats()
    val.copy_(V[1])
    auto_call(_lib, rp, ci, val, B, out=outs[0])  # c1: its check fails on the device, the plain kernel runs
    s_c2 = _lib.auto_plan_stats()
    assert s_c2["calls_async"] - s_c1["calls_async"] == 1, stats_delta(s_c2, s_c1)
    torch.cuda.synchronize()  # c1's record lands
    g1 = gate(cpms, GATE_MS)
    val.copy_(V[0])
    auto_call(_lib, rp, ci, val, B, out=outs[1])  # c2: the host reads c1's value mismatch
    s_c3 = _lib.auto_plan_stats()
    g2 = gate(cpms, GATE_MS)
    val.copy_(V[1])
    auto_call(_lib, rp, ci, val, B, out=outs[2])  # c3: the call under test
    s_end = _lib.auto_plan_stats()
    c2_async = s_c3["calls_async"] - s_c2["calls_async"] == 1
    held2, held1 = not g2.query(), not g1.query()
    assert held2, "precondition not met: the gate in front of c3 had finished before c3 was queued (gate too short?)"
    if c2_async:  # c2 queued its check behind gate 1: that check's record must not have landed before c3 read the records
        assert held1, "precondition not met: gate 1 had finished before c3 was queued (gate too short?)"
    assert s_end["calls_async"] - s_c3["calls_async"] == 1, ("c3 did not take the asynchronous path", stats_delta(s_end, s_c3))
    d = stats_delta(s_c3, s_c2)  # c2 acted on c1's record: re-permuted from it, or took a fingerprint of its own
    assert d["values_refreshed"] + d["fingerprints"] >= 1, d
    torch.cuda.synchronize()
    for i, j in enumerate((1, 0, 1)):
        assert _eq(outs[i], want[j]), f"call c{i + 1}: not the plain product of the weights current in stream order (V{j + 1})"

    # seeded flips among the three weight sets in the one buffer, random gates, no host synchronisation
    rng = np.random.RandomState(N)
    flips = 30
    counts = torch.zeros(flips, dtype=torch.int64, device="cuda")
    expect = []
    s0 = _lib.auto_plan_stats()
    for i in range(flips):
        j = int(rng.randint(3))
        val.copy_(V[j])
        if rng.rand() < 0.6:
            torch.cuda._sleep(max(1, int(cpms * float(rng.uniform(0.5, 20.0)))))
        out = auto_call(_lib, rp, ci, val, B)
        counts[i] = mismatches(out, want[j])
        expect.append(j)
    torch.cuda.synchronize()
    d = stats_delta(_lib.auto_plan_stats(), s0)
    assert d["calls_planned"] == flips and d["calls_async"] > 0 and d["values_refreshed"] > 0, d
    bad = [(i, expect[i], int(c)) for i, c in enumerate(counts.cpu().numpy()) if c]
    assert not bad, f"(flip, weight set, mismatching words): {bad}"


def test_two_streams_two_weight_buffers_one_graph(auto, oracle, sbm, cpms):
    """Advisor finding 2: stream A's planned call is queued behind other work; a call on stream B with other weights (another buffer, same
    arrays) goes through meanwhile. A's product must still be A's."""
    _lib = auto
    rp, ci, K, nnz = sbm["rowptr"], sbm["colind"], sbm["K"], sbm["nnz"]
    WA, WB = _weights(oracle, nnz, (21, 22))
    BA = torch.from_numpy(oracle.hash_B(K, 128, seed=23)).cuda()
    BB = torch.from_numpy(oracle.hash_B(K, 128, seed=24)).cuda()
    want_a = _pinned_plain(_lib, oracle, rp, ci, WA, BA)
    want_b = _pinned_plain(_lib, oracle, rp, ci, WB, BB)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    _lib.set_auto_plan(2)
    for s, w, b, ref in ((sa, WA, BA, want_a), (sb, WB, BB, want_b), (sa, WA, BA, want_a), (sa, WA, BA, want_a)):
        with torch.cuda.stream(s):  # the key warmed on both streams; A's last calls leave the cache with A's weights
            for _ in range(2):
                out = auto_call(_lib, rp, ci, w, b)
                s.synchronize()
                assert _eq(out, ref)
    with torch.cuda.stream(sa):
        out_a = nan_like_product(rp, BA)
    with torch.cuda.stream(sb):
        out_b = nan_like_product(rp, BB)
    torch.cuda.synchronize()
    s0 = _lib.auto_plan_stats()
    with torch.cuda.stream(sa):
        ga = gate(cpms, GATE_MS)
        auto_call(_lib, rp, ci, WA, BA, out=out_a)
    s1 = _lib.auto_plan_stats()
    with torch.cuda.stream(sb):
        auto_call(_lib, rp, ci, WB, BB, out=out_b)
        eb = torch.cuda.Event()
        eb.record()
    eb.synchronize()
    held = not ga.query()
    torch.cuda.synchronize()
    assert s1["calls_async"] - s0["calls_async"] == 1, ("A's call was not asynchronous", stats_delta(s1, s0))
    assert held, "precondition not met: stream A's gate ended before stream B's call finished (gate too short, or one hardware queue)"
    assert _eq(out_b, want_b), "stream B's product"
    assert _eq(out_a, want_a), "stream A's product was computed with stream B's weights"


def _overlapping(Bs, wants, cpms, call, gated_from):
    """Both streams wait on one gate event, then 16 interleaved calls each, no host sync; returns (bits ok per call, gate held).
    `gated_from` receives the cache's statistics as they were just before the gated calls."""
    from gespmm_amd._lib import auto_plan_stats

    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s, b in zip(streams, Bs):  # the key warmed on both streams; the allocator's blocks for 16 outputs per stream exist
        with torch.cuda.stream(s):
            keep = [call(b) for _ in range(16)]
            del keep
    torch.cuda.synchronize()
    gated_from.update(auto_plan_stats())
    outs = {0: [], 1: []}
    with torch.cuda.stream(torch.cuda.Stream()):
        g = gate(cpms, GATE_MS)
    for s in streams:
        s.wait_event(g)
    for i in range(16):
        for j, s in enumerate(streams):
            with torch.cuda.stream(s):
                outs[j].append(call(Bs[j]))
    held = not g.query()
    torch.cuda.synchronize()
    ok = [[_eq(o, wants[j]) for o in outs[j]] for j in (0, 1)]
    return ok, held, streams


def test_two_streams_same_arrays_overlapping_checks(auto, oracle, sbm, cpms):
    """Advisor finding 2 (its second half): two streams, the same arrays, their device-side checks in flight together. Nothing changes,
    so no plan may be dropped, and the key must go on being served through a plan afterwards."""
    _lib = auto
    rp, ci, K, nnz = sbm["rowptr"], sbm["colind"], sbm["K"], sbm["nnz"]
    (val,) = _weights(oracle, nnz, (31,))
    Bs = [torch.from_numpy(oracle.hash_B(K, 128, seed=s)).cuda() for s in (32, 33)]
    wants = [_pinned_plain(_lib, oracle, rp, ci, val, b) for b in Bs]
    _lib.set_auto_plan(2)

    def call(b):
        out = nan_like_product(rp, b)
        return auto_call(_lib, rp, ci, val, b, out=out)

    s_gate = {}
    ok, held, streams = _overlapping(Bs, wants, cpms, call, s_gate)
    s1 = _lib.auto_plan_stats()
    assert held, "precondition not met: the gate had finished before the 32 calls were queued"
    bad = [(j, i) for j in (0, 1) for i, good in enumerate(ok[j]) if not good]
    assert not bad, f"(stream, call) not the plain product: {bad}"
    d = stats_delta(s1, s_gate)
    assert d["calls_async"] >= 16, ("the overlapping calls were not served through the device-side check", d)
    assert d["invalidated"] == 0, ("a plan was dropped although the arrays never changed", d)
    # ... and the key is served through a plan again, without a stale check state
    s2 = _lib.auto_plan_stats()
    with torch.cuda.stream(streams[0]):
        for _ in range(8):
            out = call(Bs[0])
            streams[0].synchronize()
            assert _eq(out, wants[0])
    d = stats_delta(_lib.auto_plan_stats(), s2)
    assert d["calls_async"] >= 7 and d["invalidated"] == 0, d


def test_two_torch_streams_through_the_op(auto, oracle, sbm, cpms):
    """The same through spmm.csr_spmm (the op GCNConv uses) on two torch.cuda.Streams: two micro-batches sharing an adjacency."""
    _lib = auto
    from gespmm_amd import spmm

    rp, ci, K, nnz = sbm["rowptr"], sbm["colind"], sbm["K"], sbm["nnz"]
    (val,) = _weights(oracle, nnz, (41,))
    Bs = [torch.from_numpy(oracle.hash_B(K, 128, seed=s)).cuda() for s in (42, 43)]
    wants = [_pinned_plain(_lib, oracle, rp, ci, val, b) for b in Bs]
    _lib.set_auto_plan(2)
    s0 = {}
    ok, held, streams = _overlapping(Bs, wants, cpms, lambda b: spmm.csr_spmm(rp, ci, val, b), s0)
    s1 = _lib.auto_plan_stats()
    assert held, "precondition not met: the gate had finished before the 32 calls were queued"
    bad = [(j, i) for j in (0, 1) for i, good in enumerate(ok[j]) if not good]
    assert not bad, f"(stream, call) not the plain product: {bad}"
    d = stats_delta(s1, s0)
    assert d["calls_async"] >= 16 and d["invalidated"] == 0, d


def test_operand_alignment_changes_under_a_cached_plan(auto, oracle, sbm):
    """A plan made with 16-byte-aligned B / C, then called with 4-byte-aligned views: it cannot use its staged or record tables; the
    cache launches its streaming form behind the guard, or falls back to the synchronous path. The bits hold either way, C is fully
    written, and an aligned call afterwards gives the plain bits again."""
    _lib = auto
    rp, ci, K, nnz, M = sbm["rowptr"], sbm["colind"], sbm["K"], sbm["nnz"], sbm["M"]
    (val,) = _weights(oracle, nnz, (51,))
    N = 128
    Bbuf = torch.from_numpy(oracle.hash_B(K * N + 1, 1, seed=52).reshape(-1)).cuda()
    B_al = Bbuf[: K * N].view(K, N)
    B_un = Bbuf[1:].view(K, N)
    assert B_al.data_ptr() % 16 == 0 and B_un.data_ptr() % 16 == 4
    want_al = _pinned_plain(_lib, oracle, rp, ci, val, B_al)
    want_un = _pinned_plain(_lib, oracle, rp, ci, val, B_un)

    def out_view(aligned):
        buf = torch.full((M * N + 1,), float("nan"), device="cuda")
        return buf[: M * N].view(M, N) if aligned else buf[1:].view(M, N)

    _lib.set_auto_plan(2)
    for _ in range(3):
        assert _eq(auto_call(_lib, rp, ci, val, B_al, out=out_view(True)), want_al)
    paths = []
    for aligned in (False, True, False, True, True):
        C = out_view(aligned)
        s0 = _lib.auto_plan_stats()
        auto_call(_lib, rp, ci, val, B_al if aligned else B_un, out=C)
        torch.cuda.synchronize()
        d = stats_delta(_lib.auto_plan_stats(), s0)
        assert d["calls_planned"] == 1 and d["calls_async"] + d["fingerprints"] == 1, d
        paths.append(("aligned" if aligned else "4-byte", "async" if d["calls_async"] else "synchronous"))
        assert _eq(C, want_al if aligned else want_un), paths
    if paths[0][1] == "async":  # the streaming form behind the guard: the entry stays in the asynchronous mode for every alignment
        assert all(p[1] == "async" for p in paths), paths


def test_reduced_soak_of_the_auto_plan_cache(auto, sbm, cpms):
    """~300 seeded random steps on two streams: calls through every entry the cache serves, weight flips, value-pointer switches,
    in-place pattern edits, new dense operands, gates — against the products of the same states with the switch off."""
    from helpers import auto_plan_soak

    failures, d, ncalls = auto_plan_soak(auto, sbm, seed=7, steps=300, cycles_per_ms=cpms)
    assert ncalls > 100 and d["calls_async"] > 0 and d["values_refreshed"] > 0 and d["fingerprints"] > 0, d
    assert not failures, f"(step, stream, op, state, mismatching words), first 10 of {len(failures)}: {failures[:10]}"
