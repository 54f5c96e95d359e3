"""CSMOE_EPI_ACCUM: csmoe_dense_gemm adds round(A @ B) into C in its epilogue -- C = round(C + round(acc)) in bf16, C += acc in fp32 --
on every kernel the call can select (include/csmoe.h).  GPU cases compare with the same kernel's plain product added by torch's
`add_` (bit for bit) and with an fp64 product; the refusal of the other entry points runs on the CPU (it happens before any launch)."""
import pytest
import torch

from competesmoe_amd import _lib as L


def test_accum_refused_outside_dense_gemm():
    """csmoe_grouped_gemm / _f32w / the MXFP8 entries return CSMOE_ERR_UNSUPPORTED for EPI_ACCUM before touching any pointer."""
    lib = L.lib
    unsupported = 3
    assert lib.csmoe_grouped_gemm(None, 64, None, 0, 64, None, None, 1, 256, 64, 64, None, None, None, 64, L.EPI_ACCUM, 0, L.BF16, 0,
                                  None) == unsupported
    assert b"ACCUM" in lib.csmoe_last_error()
    assert lib.csmoe_grouped_gemm_f32w(None, 64, None, 64, None, None, None, 1, 256, 64, 64, None, None, None, 64, L.EPI_ACCUM, 0,
                                       None) == unsupported
    assert lib.csmoe_dense_gemm_mxfp8(None, 64, None, 2, None, None, 64, 2, None, 256, 64, 64, None, None, None, 64, L.EPI_ACCUM, 0,
                                      None) == unsupported
    # dense_gemm itself: ACCUM takes no bias / C2 / aux and needs ldc >= N
    assert lib.csmoe_dense_gemm(None, 64, None, 0, 64, None, 0, 64, 64, None, None, None, 32, L.EPI_ACCUM, 0, L.BF16, 0, None) == 1


def _cases():
    # (M, N, K, b_layout, kernel): kernel 0 = the library's choice (the 128x128 kernel at these sizes), 1 generic, 2 the 8-wave
    # 256x256 kernel, 4 the one-wave-per-SIMD kernel (K-contiguous weights, K a multiple of 128); M not a multiple of any tile,
    # N % 256 != 0
    return [(300, 200, 136, L.B_NK, 0), (300, 200, 136, L.B_KN, 0), (333, 72, 40, L.B_NK, 1), (333, 200, 136, L.B_KN, 1),
            (1100, 520, 512, L.B_NK, 2), (1100, 520, 392, L.B_KN, 2), (2500, 264, 256, L.B_NK, 2),
            (1100, 520, 512, L.B_NK, 4), (2500, 776, 384, L.B_NK, 4), (4096, 512, 256, L.B_NK, 0)]


def _operands(M, N, K, layout, dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, K, device="cuda", generator=g).to(dt)
    B = (torch.randn(N, K, device="cuda", generator=g) if layout == L.B_NK else torch.randn(K, N, device="cuda", generator=g)).to(dt)
    C0 = (4 * torch.randn(M, N, device="cuda", generator=g)).to(dt)
    return A, B, C0


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,layout,kernel", _cases())
@pytest.mark.parametrize("strided", [False, True])
def test_accum_bf16_bit_exact(M, N, K, layout, kernel, strided):
    from competesmoe_amd import ops
    A, B, C0 = _operands(M, N, K, layout, torch.bfloat16, M + N + K)
    P = ops.dense_gemm(A, B, layout, kernel=kernel)                      # the same kernel's rounded product
    want = C0.clone().add_(P)                                             # torch's bf16 add_: the chain the layer builds today
    if strided:                                                           # C inside a wider buffer: ldc = N + 24, 16 bytes in
        buf = torch.full((M, N + 24), 7.0, dtype=torch.bfloat16, device="cuda")
        C = buf[:, 8:8 + N]
        C.copy_(C0)
    else:
        C = C0.clone()
    out = ops.dense_gemm(A, B, layout, epilogue=L.EPI_ACCUM, out=C, kernel=kernel)
    torch.cuda.synchronize()
    assert out is C
    assert torch.equal(C, want)
    if strided:                                                           # nothing outside the view was touched
        assert bool((buf[:, :8] == 7).all()) and bool((buf[:, 8 + N:] == 7).all())
    ref = C0.double() + A.double() @ (B.double().t() if layout == L.B_NK else B.double())
    assert float((C.double() - ref).norm() / ref.norm()) < 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,layout", [(300, 200, 136, L.B_NK), (333, 72, 40, L.B_KN), (129, 65, 33, L.B_NK)])
def test_accum_fp32(M, N, K, layout):
    """fp32 operands (the generic kernel): C += acc, within fp32 rounding of torch's C0 + A @ B."""
    from competesmoe_amd import ops
    A, B, C0 = _operands(M, N, K, layout, torch.float32, 5 + M)
    C = C0.clone()
    ops.dense_gemm(A, B, layout, epilogue=L.EPI_ACCUM, out=C)
    P = ops.dense_gemm(A, B, layout)
    torch.cuda.synchronize()
    assert torch.equal(C, C0 + P)
    ref = C0.double() + A.double() @ (B.double().t() if layout == L.B_NK else B.double())
    assert float((C.double() - ref).abs().max()) < 1e-4 * float(ref.abs().max())


@pytest.mark.gpu
def test_accum_chain_equals_add_chain():
    """The competition backward's dX chain: expert 0 writes, experts 1.. add (EPI_ACCUM) -- the GEMM + add_ chain bit for bit."""
    from competesmoe_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    T, D, Fh, E = 1500, 264, 512, 4
    dh = [torch.randn(T, Fh, device="cuda", generator=g).bfloat16() for _ in range(E)]
    keys = [torch.randn(D, Fh, device="cuda", generator=g).bfloat16() for _ in range(E)]
    ref = None
    for e in range(E):
        p = ops.dense_gemm(dh[e], keys[e], L.B_NK)
        ref = p if ref is None else ref.add_(p)
    dx = ops.dense_gemm(dh[0], keys[0], L.B_NK)
    for e in range(1, E):
        ops.dense_gemm(dh[e], keys[e], L.B_NK, epilogue=L.EPI_ACCUM, out=dx)
    torch.cuda.synchronize()
    assert torch.equal(dx, ref)
