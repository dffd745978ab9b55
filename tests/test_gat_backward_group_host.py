"""The form rule of the fused GAT backward, host side (no GPU): ``gespmm_describe_gat_backward`` answers what the two entry points
route through — lane or group form, the dot geometry (V, W_d) and the segment geometry (W, L) — with and without the pin
GESPMM_GAT_BACKWARD_FORM."""
import pytest

F_MIN = 16  # the committed kGatBackwardGroupMinF (select.h); None: the group form is the default nowhere, the pin alone reaches it
SIZES = dict(M=3000, K=2500, H=3, nnz=40000)
ELIGIBLE = (16, 20, 32, 64, 128, 256, 512)


@pytest.fixture(scope="module")
def L(pkg):
    from gespmm_amd import _lib

    return _lib


def _describe(L, F, transposed=False, aligns=(16, 16), **kw):
    s = dict(SIZES, **kw)
    return L.describe_gat_backward(s["M"], s["K"], s["H"], F, s["nnz"], transposed=transposed, aligns=aligns)


def test_symbol(L):
    assert "gespmm_describe_gat_backward" in L.EXPORTS
    getattr(L.lib, "gespmm_describe_gat_backward")
    assert L.describe_gat_backward(4, 4, 2, 16, 0) == {"form": "none"}
    with pytest.raises(L.GespmmError):
        L.describe_gat_backward(4, 4, 0, 16, 10)


@pytest.mark.parametrize("pin", (None, "lane", "group"))
@pytest.mark.parametrize("F,aligns", [(F, (16, 16)) for F in (1, 5, 8, 12, 27, 516)] + [(F, a) for F in (16, 64) for a in ((8, 16), (16, 4))])
def test_ineligible_calls_take_the_lane_form_whatever_the_pin(L, monkeypatch, F, aligns, pin):
    if pin:
        monkeypatch.setenv("GESPMM_GAT_BACKWARD_FORM", pin)
    for transposed in (False, True):
        d = _describe(L, F, transposed, aligns)
        assert d["form"] == "lane" and d["Wd"] == 1 and d["V"] == (4 if F % 4 == 0 and aligns == (16, 16) else 1), (F, aligns, d)


@pytest.mark.parametrize("F,Wd", ((16, 4), (20, 4), (32, 4), (36, 8), (64, 8), (128, 16), (132, 32), (256, 32), (260, 64), (512, 64)))
def test_group_pin(L, monkeypatch, F, Wd):
    monkeypatch.setenv("GESPMM_GAT_BACKWARD_FORM", "group")
    for transposed in (False, True):
        for H, nnz in ((1, 9000), (3, 40000), (8, 400000)):  # W_s = 4, 16, 16: independent of W_d
            d = _describe(L, F, transposed, H=H, nnz=nnz)
            S = SIZES["K"] if transposed else SIZES["M"]
            assert d == dict(L.describe_edge_softmax(S, nnz, H), form="group", V=4, Wd=Wd), (F, transposed, H, nnz, d)
            if H > 1:
                assert L.describe_sddmm_heads(True, SIZES["M"], nnz, H, F)["W"] == Wd, "the multi-head SDDMM's lanes per pair at this width"
    monkeypatch.setenv("GESPMM_GAT_BACKWARD_FORM", "lane")
    assert _describe(L, F)["form"] == "lane"


def test_default_is_the_group_form_exactly_from_the_committed_threshold(L, monkeypatch):
    monkeypatch.delenv("GESPMM_GAT_BACKWARD_FORM", raising=False)
    assert F_MIN is None or F_MIN in (16, 32, 64)
    for F in ELIGIBLE:
        want = "group" if F_MIN is not None and F >= F_MIN else "lane"
        for transposed in (False, True):
            assert _describe(L, F, transposed)["form"] == want, (F, transposed)
