"""The fused relational weight gradient on 16-bit features, host side only: the route table of gespmm_spmm_relational_wgrad_route_x16,
the chunk count of gespmm_spmm_relational_wgrad_chunks at its edges, and the return codes of gespmm_csr_spmm_relational_wgrad_x16 that
come back before any launch (fabricated addresses: nothing is dereferenced)."""
import pytest

EINVAL, EALIGN, ERANGE, UNSUPPORTED = -1, -2, -3, -7
LIM = 2**31 - 4097
BF16 = 2

ROUTE = [  # (R, M, Kn, K, N_out, nnz, chunks, align) -> route
    ((1, 301, 257, 8, 1, 2500, 1, 16), 1), ((3, 301, 257, 256, 256, 2500, 5, 16), 1), ((16, 301, 257, 136, 33, 0, 2, 16), 1),
    ((3, 301, 257, 64, 32, 2500, 0, 16), 0), ((3, 301, 257, 64, 32, 2500, 6, 16), 0), ((3, 64, 257, 64, 32, 2500, 2, 16), 0),  # chunks
    ((0, 301, 257, 64, 32, 0, 1, 16), 0), ((3, 0, 257, 64, 32, 0, 1, 16), 0), ((3, 301, 257, 12, 32, 2500, 1, 16), 0),
    ((3, 301, 257, 264, 32, 2500, 1, 16), 0), ((3, 301, 257, 64, 257, 2500, 1, 16), 0), ((3, 301, 257, 64, 32, 2500, 1, 8), 0),
    ((4096, 2047, 1, 256, 256, 0, 7, 16), 1), ((4096, 2047, 1, 256, 256, 0, 8, 16), 0),  # chunks R N_out K
    ((4, LIM // 32 + 1, 1, 8, 1, 0, 1, 16), ERANGE), ((-1, 1, 1, 8, 1, 0, 1, 16), EINVAL), ((1, 1, 1, 8, 1, 0, 1, 12), EINVAL),
]


@pytest.mark.parametrize("args,want", ROUTE)
def test_route_table(pkg, args, want):
    from gespmm_amd import _lib

    assert _lib.lib.gespmm_spmm_relational_wgrad_route_x16(*args) == want
    assert want < 0 or _lib.spmm_relational_wgrad_route_x16(*args) == want


CHUNKS = [  # (R, M, K, N_out) -> chunks
    ((1, 63, 64, 1), 1), ((1, 64, 8, 1), 1), ((1, 65, 8, 1), 2),  # M < 64: one block
    ((300, 10000, 256, 8), 1), ((256, 10000, 256, 8), 1), ((255, 10000, 256, 8), 2),  # R slabs > / = / < 1024
    ((16, 334863, 256, 256), 16), ((4, 334863, 64, 47), 256), ((4, 334863, 72, 47), 128),  # ceil(1024 / (R slabs))
    ((1, 6400, 8, 1), 100), ((1, 6401, 8, 1), 101),  # the cap: ceil(M / 64)
    ((3, 257, 64, 47), 1), ((1, 301, 8, 32), 2), ((1, 301, 8, 1), 5),  # a workspace below half of the aggregates: M / (4 N_out)
    ((0, 301, 64, 32), 0), ((3, 0, 64, 32), 0), ((3, 301, 0, 32), 0), ((3, 301, 64, 0), 0),
    ((-1, 301, 64, 32), EINVAL), ((3, 301, 64, -1), EINVAL), ((3, LIM // 3 + 1, 8, 1), ERANGE), ((LIM // 2048 + 1, 1, 8, 256), ERANGE),
]


@pytest.mark.parametrize("args,want", CHUNKS)
def test_chunk_count(pkg, args, want):
    from gespmm_amd import _lib

    assert _lib.lib.gespmm_spmm_relational_wgrad_chunks(*args) == want
    assert want < 0 or _lib.spmm_relational_wgrad_chunks(*args) == want


BASE = dict(rowptr=0x1000, colind=0x2000, val=0x3000, row_scale=0x4000, X=0x5000, grad_out=0x6000, partials=0x10000, grad_W=0x8000,
            dtype=BF16, R=3, M=4, Kn=4, K=8, N_out=8, nnz=5, chunks=1)

LADDER = [
    (dict(dtype=0), EINVAL), (dict(dtype=3), EINVAL), (dict(dtype=0, M=LIM + 1), EINVAL),
    (dict(R=-1), EINVAL), (dict(M=-1), EINVAL), (dict(nnz=-1), EINVAL), (dict(K=-8), EINVAL),
    (dict(M=LIM // 3 + 1), ERANGE), (dict(Kn=LIM + 1), ERANGE), (dict(nnz=LIM + 1), ERANGE), (dict(M=LIM // 24 + 1), ERANGE),
    (dict(R=LIM // 64 + 1, M=1), ERANGE),
    (dict(R=0, rowptr=None, grad_W=None, partials=None), 0), (dict(N_out=0, grad_W=None), 0), (dict(K=0, X=None), 0),
    (dict(rowptr=None), EINVAL), (dict(grad_out=None), EINVAL), (dict(partials=None), EINVAL), (dict(grad_W=None), EINVAL),
    (dict(colind=None), EINVAL), (dict(X=None), EINVAL),
    (dict(rowptr=0x1002), EALIGN), (dict(row_scale=0x4002), EALIGN), (dict(partials=0x10002), EALIGN), (dict(X=0x5001), EALIGN),
    (dict(X=0x5002), EINVAL), (dict(grad_out=0x6008), EINVAL), (dict(grad_W=0x8004), EINVAL), (dict(partials=0x10008), EINVAL),
    (dict(K=12), UNSUPPORTED), (dict(K=264), UNSUPPORTED), (dict(N_out=257), UNSUPPORTED), (dict(M=0, grad_out=None), UNSUPPORTED),
    (dict(chunks=0), UNSUPPORTED), (dict(chunks=2), UNSUPPORTED), (dict(chunks=-1), UNSUPPORTED),
    (dict(grad_W=0x5000 + 32), EINVAL),  # inside X's Kn K 2 = 64 bytes
    (dict(grad_W=0x6000 + 32), EINVAL),  # inside grad_out's M N_out 2 = 64 bytes
    (dict(partials=0x8000 + 256), EINVAL),  # inside grad_W's R N_out K 2 = 384 bytes
    (dict(partials=0x6000 - 512), EINVAL),  # its chunks R N_out K 4 = 768 bytes reach into grad_out
]


@pytest.mark.parametrize("override,want", LADDER)
def test_return_codes_before_any_launch(pkg, override, want):
    from gespmm_amd import _lib

    args = dict(BASE, **override)
    assert _lib.csr_spmm_relational_wgrad_x16(**args) == want
