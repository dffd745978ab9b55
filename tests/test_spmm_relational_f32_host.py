"""The relational aggregate-and-linear on fp32 features, host side only: the route table of gespmm_spmm_relational_route_f32 on both
sides of every threshold, and the return codes of gespmm_csr_spmm_relational_f32 that come back before any launch (fabricated addresses:
nothing is dereferenced)."""
import pytest

EINVAL, EALIGN, ERANGE, UNSUPPORTED = -1, -2, -3, -7
LIM = 2**31 - 4097

ROUTE = [  # (R, M, Kn, K, N_out, nnz, align) -> route
    ((1, 301, 257, 4, 1, 2500, 16), 1), ((3, 301, 257, 256, 256, 2500, 16), 1), ((16, 301, 257, 132, 33, 0, 16), 1),
    ((0, 301, 257, 64, 32, 0, 16), 0), ((3, 301, 257, 0, 32, 2500, 16), 0), ((3, 301, 257, 2, 32, 2500, 16), 0),
    ((3, 301, 257, 6, 32, 2500, 16), 0), ((3, 301, 257, 260, 32, 2500, 16), 0), ((3, 301, 257, 64, 257, 2500, 16), 0),
    ((3, 301, 257, 64, 0, 2500, 16), 0), ((3, 0, 257, 64, 32, 0, 16), 0), ((3, 301, 257, 64, 32, 2500, 8), 0), ((3, 301, 257, 64, 32, 2500, 4), 0),
    ((4, LIM // 4 + 1, 1, 0, 1, 0, 16), ERANGE),  # R M
    ((4, LIM // 16, 1, 4, 1, 0, 16), 1), ((4, LIM // 16 + 1, 1, 4, 1, 0, 16), ERANGE),  # R M K
    ((LIM // 1024, 1, 1, 4, 256, 0, 16), 1), ((LIM // 1024 + 1, 1, 1, 4, 256, 0, 16), ERANGE),  # R N_out K
    ((1, 1, 1, 4, 1, LIM, 16), 1), ((1, 1, 1, 4, 1, LIM + 1, 16), ERANGE),
    ((-1, 1, 1, 4, 1, 0, 16), EINVAL), ((1, -1, 1, 4, 1, 0, 16), EINVAL), ((1, 1, 1, 4, 1, -1, 16), EINVAL),
    ((1, 1, 1, 4, 1, 0, 12), EINVAL), ((1, 1, 1, 4, 1, 0, 2), EINVAL),
]


@pytest.mark.parametrize("args,want", ROUTE)
def test_route_table(pkg, args, want):
    from gespmm_amd import _lib

    assert _lib.lib.gespmm_spmm_relational_route_f32(*args) == want
    if want >= 0:
        assert _lib.spmm_relational_route_f32(*args) == want
    else:
        with pytest.raises(_lib.GespmmError) as e:
            _lib.spmm_relational_route_f32(*args)
        assert e.value.code == want


BASE = dict(rowptr=0x1000, colind=0x2000, val=0x3000, row_scale=0x4000, X=0x5000, W=0x6000, X_root=0x7000, W_root=0x8000, bias=0x9000,
            out=0x20000, R=3, M=4, Kn=4, K=8, N_out=8, nnz=5)

LADDER = [
    (dict(R=-1), EINVAL), (dict(M=-1), EINVAL), (dict(nnz=-1), EINVAL), (dict(K=-8), EINVAL),
    (dict(M=LIM // 3 + 1), ERANGE), (dict(Kn=LIM + 1), ERANGE), (dict(nnz=LIM + 1), ERANGE), (dict(M=LIM // 24 + 1), ERANGE),
    (dict(R=LIM // 64 + 1, M=1), ERANGE),
    (dict(M=0, rowptr=None, out=None), 0), (dict(N_out=0, W=None), 0),
    (dict(X_root=None), EINVAL), (dict(W_root=None), EINVAL),
    (dict(rowptr=None), EINVAL), (dict(W=None), EINVAL), (dict(out=None), EINVAL), (dict(colind=None), EINVAL), (dict(X=None), EINVAL),
    (dict(rowptr=0x1002), EALIGN), (dict(bias=0x9002), EALIGN), (dict(X=0x5002), EALIGN),
    (dict(X=0x5004), EALIGN), (dict(out=0x20008), EALIGN), (dict(W_root=0x8004), EALIGN), (dict(X=0x5004, K=6), EALIGN),
    (dict(out=0x5000 + 64), EINVAL),  # inside X's Kn K 4 = 128 bytes
    (dict(out=0x6000 + 512), EINVAL),  # inside W's R N_out K 4 = 768 bytes, past its first relation
    (dict(R=0), UNSUPPORTED), (dict(K=6), UNSUPPORTED), (dict(K=260), UNSUPPORTED), (dict(N_out=257), UNSUPPORTED), (dict(K=0), UNSUPPORTED),
    (dict(bias=0x9004, row_scale=0x4004, val=0x3004, K=6), UNSUPPORTED),  # (4-byte alignment is all the fp32 vectors need)
]


@pytest.mark.parametrize("override,want", LADDER)
def test_return_codes_before_any_launch(pkg, override, want):
    from gespmm_amd import _lib

    args = dict(BASE, **override)
    assert _lib.csr_spmm_relational_f32(**args) == want
