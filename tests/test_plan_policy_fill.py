"""The fill pass of the staging tables and the policy (csrc/plan_policy.cpp: staged_fill_window) — host only, no device.
`staged_fraction` stays the share of entries staged by the >= 2-use rule, so every staged / not-staged decision the policy table of
tests/test_plan_policy.py pins is what it was; the window is a policy constant that the GESPMM_STAGED_FILL switch (read by plan creation,
not by the policy) does not move."""
import pytest

from gespmm_amd import _lib
from test_plan_policy import TABLE

STAGED_ROWS = [t for t in TABLE if "build_staged" in t[2] or "keep_staged" in t[2]]


@pytest.mark.parametrize("name,shape,expect", STAGED_ROWS, ids=[t[0] for t in STAGED_ROWS])
@pytest.mark.parametrize("switch", (None, "0", "4"))
def test_staged_decisions_are_what_they_were(monkeypatch, name, shape, expect, switch):
    if switch is None:
        monkeypatch.delenv("GESPMM_STAGED_FILL", raising=False)
    else:
        monkeypatch.setenv("GESPMM_STAGED_FILL", switch)
    M, nnz, N, maxdeg, hb, ha, sf = shape
    got = _lib.plan_policy(M, M, nnz, N, maxdeg, hb, ha, sf, expected_launches=1000000)
    for k in ("build_staged", "keep_staged"):
        if k in expect:
            assert got[k] == expect[k], (name, k, got)
    # the window: two blocks on a square matrix wherever the width is served by a staged kernel, whatever the switch says
    assert got["staged_fill_window"] == (2 if got["staged_rows"] > 0 else 0), (name, got)


def test_structureless_stand_in_stays_with_the_streaming_kernels():
    """com-amazon-like at N = 128 stages 0.21 of its entries by the >= 2 rule (tests/test_gpu_plan_staged.py); filled entries are not
    counted into that share, so AUTO drops its tables as before — and would keep them if they were (0.21 + 0.35 >= 0.55)."""
    base = (334863, 334863, 1851744, 128, 120, 0.02, 0.45)
    assert _lib.plan_policy(*base, 0.21, expected_launches=5000)["keep_staged"] == 0
    assert _lib.plan_policy(*base, 0.56, expected_launches=5000)["keep_staged"] == 1


def test_no_window_without_a_home_row_or_on_the_host():
    sq = _lib.plan_policy(334863, 334863, 1851744, 128, 120, 0.02, 0.65, 0.75)
    assert sq["staged_fill_window"] == 2
    assert _lib.plan_policy(334863, 400000, 1851744, 128, 120, 0.02, 0.65, 0.75)["staged_fill_window"] == 0  # K != M
    assert _lib.plan_policy(334863, 334863, 1851744, 128, 120, 0.02, 0.65, 0.75, analysis=_lib.PLAN_ANALYSIS_HOST)["staged_fill_window"] == 0
