"""The split-K MFMA fp32 GEMM behind the TGN memory path (include/tgnx.h tgnx_gemm_f32) against a
plain torch fp32 matmul: all four transpose modes, split-K (K > 64), ragged edges, bias,
accumulate, determinism; on integer data (exact) the switch to 64x64 tiles at 512 of them, accumulate + bias
through the split-K fixup, and ldc > N.  The split workspace is NaN-filled.  (The tile configs this entry does
not reach: test_gpu_gemm_core.py.)"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _gemm(A, B, ta, tb, M, N, K, bias=None, C=None, acc=False):
    from tgnx import _lib
    dev = A.device
    if C is None:
        C = torch.zeros(M, N, device=dev)
    nb = _lib.lib().tgnx_gemm_f32_ws_bytes(M, N, K)
    assert nb % 4 == 0
    ws = torch.full((nb // 4,), float("nan"), device=dev)    # a split partial that is read must have been written
    lda, ldb = A.shape[1], B.shape[1]
    _lib.call("tgnx_gemm_f32", M, N, K, _lib.ptr(A), lda, int(ta), _lib.ptr(B), ldb, int(tb), _lib.ptr(C),
              C.stride(0), _lib.ptr(bias) if bias is not None else None, int(acc), _lib.ptr(ws), ctypes.c_size_t(nb),
              _lib.stream())
    return C


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (17, 33, 5), (64, 64, 64), (413, 400, 572), (100, 272, 1710),
                                   (3, 100, 413)])
@pytest.mark.parametrize("ta,tb", [(0, 1), (0, 0), (1, 1), (1, 0)])
def test_gemm_matches_torch(M, N, K, ta, tb):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    dev = torch.device("cuda")
    A = torch.randn((K, M) if ta else (M, K), generator=g).to(dev)
    B = torch.randn((N, K) if tb else (K, N), generator=g).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    opA = A.t() if ta else A
    opB = B.t() if tb else B
    ref = (opA.double() @ opB.double() + bias.double()).float()
    out = _gemm(A, B, ta, tb, M, N, K, bias=bias)
    torch.cuda.synchronize()
    tol = 1e-5 * (K ** 0.5) + 1e-6
    assert torch.allclose(out, ref, rtol=tol, atol=tol * 4), (out - ref).abs().max()
    out2 = _gemm(A, B, ta, tb, M, N, K, bias=bias)
    assert torch.equal(out, out2)           # fixed-order split-K reduction


def test_gemm_accumulate():
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    A, B = torch.randn(70, 130, generator=g).to(dev), torch.randn(90, 130, generator=g).to(dev)
    C0 = torch.randn(70, 90, generator=g).to(dev)
    out = _gemm(A, B, 0, 1, 70, 90, 130, C=C0.clone(), acc=True)
    ref = C0 + A @ B.t()
    assert torch.allclose(out, ref, rtol=1e-4, atol=1e-4)


def _ints(g, *shape):
    """Integers in [-3, 3] as fp32: every product and partial sum is an exact integer (9 K + 6 < 2^24), so the
    result equals an int64 matmul whatever the tile, split or wave order."""
    return torch.randint(-3, 4, shape, generator=g).float()


@pytest.mark.parametrize("M,N,K", [(32705, 3, 7), (32705, 3, 260), (32641, 3, 7), (32641, 3, 260)])
def test_gemm_exact_around_the_64x64_threshold(M, N, K):
    """512 tiles of 64x64 (M = 32705 = 511 * 64 + 1) take the 64x64 config, direct at K = 7 and split-K at
    K = 260; 511 tiles (M = 32641) the 16x16 one.  Integer data: exact."""
    from tgnx import _lib
    g = torch.Generator().manual_seed(M + K)
    dev = torch.device("cuda")
    A, B, bias = _ints(g, M, K), _ints(g, N, K), _ints(g, N)
    want = (A.long() @ B.long().t() + bias.long()).float()
    out = _gemm(A.to(dev), B.to(dev), 0, 1, M, N, K, bias=bias.to(dev))
    assert torch.equal(out.cpu(), want)
    At = A.t().contiguous()                                   # the same product from a transposed A
    out = _gemm(At.to(dev), B.to(dev), 1, 1, M, N, K, bias=bias.to(dev))
    assert torch.equal(out.cpu(), want)
    # the workspace size is accepted at exactly its own value and rejected one byte below
    lib = _lib.lib()
    nb = lib.tgnx_gemm_f32_ws_bytes(M, N, K)
    Ad, Bd = A.to(dev), B.to(dev)
    C = torch.full((M, N), -7.0, device=dev)
    ws = torch.full((nb // 4,), float("nan"), device=dev)
    rc = lib.tgnx_gemm_f32(M, N, K, _lib.ptr(Ad), K, 0, _lib.ptr(Bd), K, 1, _lib.ptr(C), N, None, 0, _lib.ptr(ws),
                           ctypes.c_size_t(nb - 1), _lib.stream())
    assert rc != 0 and b"workspace" in lib.tgnx_last_error()
    torch.cuda.synchronize()
    assert bool((C == -7.0).all())                            # rejected before any launch


@pytest.mark.parametrize("M,N", [(70, 90), (32705, 3)])
def test_gemm_accumulate_with_bias_split_k_exact(M, N):
    """accumulate + bias through the split-K fixup (K = 572 > 256), into a C whose rows are wider than N: the
    padding columns keep their sentinel."""
    K, ldc = 572, N + 5
    g = torch.Generator().manual_seed(M)
    dev = torch.device("cuda")
    A, B, bias, C0 = _ints(g, M, K), _ints(g, K, N), _ints(g, N), _ints(g, M, N)
    wide = torch.full((M, ldc), -12345.0)
    wide[:, :N] = C0
    Cd = wide.to(dev)
    out = _gemm(A.to(dev), B.to(dev), 0, 0, M, N, K, bias=bias.to(dev), C=Cd[:, :N], acc=True)
    assert out.stride(0) == ldc
    got = Cd.cpu()
    assert torch.equal(got[:, :N], (A.long() @ B.long() + bias.long() + C0.long()).float())
    assert bool((got[:, N:] == -12345.0).all())


def test_gemm_ldc_wider_than_n_direct():
    M, N, K, ldc = 33, 17, 100, 24
    g = torch.Generator().manual_seed(5)
    dev = torch.device("cuda")
    A, B = _ints(g, K, M), _ints(g, N, K)
    Cd = torch.full((M, ldc), -12345.0, device=dev)
    _gemm(A.to(dev), B.to(dev), 1, 1, M, N, K, C=Cd[:, :N])
    got = Cd.cpu()
    assert torch.equal(got[:, :N], (A.long().t() @ B.long().t()).float())
    assert bool((got[:, N:] == -12345.0).all())
