"""gespmm_describe_gat_backward_x16 and the return codes of the 16-bit fused GAT backward entries, on the host: the routing table over F,
alignments and the pin, and the ladder up to the first launch (no device is touched: every call returns before one)."""
import ctypes

import pytest

from test_heads_host import EALIGN, EINVAL, ERANGE

PIN = "GESPMM_GAT_BACKWARD_FORM"
SIZES = (1000, 900, 4)  # M, K, H; nnz = 8000: W = 8


def _describe(F, aligns=(16, 16), transposed=False):
    from gespmm_amd import _lib

    d = _lib.describe_gat_backward(SIZES[0], SIZES[1], SIZES[2], F, 8000, transposed=transposed, aligns=aligns, x16=True)
    return d["form"], d["V"], d["Wd"]


# (F, aligns of (grad_out, feat), pin) -> (form, V in elements, W_d)
TABLE = (
    (1, (16, 16), None, ("lane", 1, 1)), (6, (16, 16), None, ("lane", 2, 1)), (12, (16, 16), None, ("lane", 4, 1)),
    (8, (16, 16), None, ("lane", 8, 1)), (8, (16, 8), None, ("lane", 4, 1)), (8, (4, 16), None, ("lane", 2, 1)),
    (8, (2, 16), None, ("lane", 1, 1)), (8, (16, 16), "group", ("lane", 8, 1)),             # F < 16: never eligible
    (16, (16, 16), None, ("group", 4, 4)), (20, (8, 16), None, ("group", 4, 4)), (32, (8, 8), None, ("group", 4, 4)),
    (36, (16, 16), None, ("group", 4, 8)), (64, (16, 16), None, ("group", 4, 8)), (128, (16, 16), None, ("group", 4, 16)),
    (256, (16, 16), None, ("group", 4, 32)), (512, (16, 16), None, ("group", 4, 64)),
    (516, (16, 16), "group", ("lane", 4, 1)), (520, (16, 16), None, ("lane", 8, 1)),         # past kGatBackwardGroupMaxF
    (18, (16, 16), "group", ("lane", 2, 1)),                                                 # F % 4 != 0
    (64, (16, 16), "lane", ("lane", 8, 1)), (64, (8, 16), "lane", ("lane", 4, 1)),
    (64, (4, 16), "group", ("lane", 2, 1)), (64, (16, 2), "group", ("lane", 1, 1)),          # below 8 bytes: the pin is ignored
)


@pytest.mark.parametrize("F,aligns,pin,want", TABLE)
def test_routing_table(pkg, monkeypatch, F, aligns, pin, want):
    from gespmm_amd import _lib

    monkeypatch.delenv(PIN, raising=False)
    if pin:
        monkeypatch.setenv(PIN, pin)
    for transposed in (False, True):
        assert _describe(F, aligns, transposed) == want
    if want[0] == "group":  # the answer for the widened operands: an operand b bytes off is one 2 b bytes off
        wide = _lib.describe_gat_backward(SIZES[0], SIZES[1], SIZES[2], F, 8000, aligns=tuple(min(16, 2 * a) for a in aligns))
        assert (wide["form"], wide["V"], wide["Wd"]) == want
    d = _lib.describe_gat_backward(SIZES[0], SIZES[1], SIZES[2], F, 8000, aligns=aligns, x16=True)
    e = _lib.describe_edge_softmax(SIZES[0], 8000, SIZES[2])
    assert (d["W"], d["L"], d["rpw"]) == (e["W"], e["L"], 16)
    assert _lib.describe_gat_backward(SIZES[0], SIZES[1], SIZES[2], F, 0, x16=True) == {"form": "none"}


def test_return_codes(pkg):
    from gespmm_amd import _lib

    lib, big = _lib.lib, 1 << 31
    p = lambda a: ctypes.c_void_p(a)  # noqa: E731  (never dereferenced: every call returns before a launch)
    ok, odd = p(4096), p(4098 + 1)

    def el(dtype=_lib.X16_BF16, go=ok, ft=ok, M=10, K=10, H=2, F=8, nnz=20, dropout=None, delta=ok):
        args = (ok, ok, ok, ok, ok, go, ft, dtype, delta, ok, M, K, H, F, nnz, 0.2)
        if dropout is None:
            return lib.gespmm_gat_backward_el_x16(*args, None)
        return lib.gespmm_gat_backward_el_dropout_x16(*args, dropout, ok, None)

    def er(dtype=_lib.X16_F16, go=ok, ft=ok, M=10, K=10, H=2, F=8, nnz=20):
        return lib.gespmm_gat_backward_er_x16(ok, ok, ok, ok, ok, ok, go, ft, dtype, ok, M, K, H, F, nnz, 0.2, None)

    for f in (el, er):
        assert f(dtype=0) == EINVAL and f(dtype=3) == EINVAL
        assert f(dtype=0, M=big) == EINVAL              # the dtype comes first
        assert f(H=0) == EINVAL and f(nnz=-1) == EINVAL
        assert f(M=big, nnz=big) == ERANGE              # sizes past the limit
        assert f(M=1 << 22, K=8, H=8, F=128) == ERANGE  # M H F past 32-bit word positions
        assert f(go=odd) == EALIGN and f(ft=odd) == EALIGN
        assert f(go=p(0)) == EINVAL
    assert el(dropout=1.0) == EINVAL
    assert el(M=0, nnz=0) == 0                                      # nothing to write, nothing launched
    assert el(nnz=0, delta=p(0)) == EINVAL and el(nnz=0, delta=odd) == EALIGN  # no entries: the results are still checked
