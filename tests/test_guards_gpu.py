"""GPU: both sides of every kernel-selection guard of the C ABI.

Almost every entry point picks one of two or more kernels from a predicate over alignment, leading dimensions, divisibility, the
2 GiB buffer-record limit of the tiled GEMMs or a grid limit.  The rest of the suite runs fresh contiguous (256-byte aligned)
operands, so it tests the fast side of these guards.  Here every guard gets one case just inside and one just outside it:

* a guard that CHOOSES a kernel for a valid input: both sides are compared with a plain fp64 torch reference of the operation
  (copies and permutations: exact equality);
* a guard that REFUSES: the outside case raises from L.check with the library's message and writes no output.

Where the choice is observable from the host it is pinned too: csmoe_grouped_gemm_rowdot_cols (fast GEMM and which of its tilings),
csmoe_gate_select_ok, csmoe_gate_bwd_small_ok, csmoe_dispatch_vec_ok, and the ACTGRAD_ROWSCALE dot table, which only the tiled bf16
kernels write (the generic kernel refuses it before launching: a probe of which side of the rowspace guard a launch takes).

Guard table (file:line at the time of writing -> inside / outside test):

  csrc/gemm_bf16.hip:258 gg_fast_rowspace_ok   lda % 8                test_rowspace_lda[in] / [out]
                                               A alignment            test_rowspace_misaligned_a[in] / [out]
                                               ldb % 8                test_rowspace_ldb[in] / [out]
                                               M * lda * 2 < 2^31     test_rowspace_2gib_a[in] / [out]
                                               max(N,Kd) * ldb * 2    test_rowspace_2gib_b[in] / [out]
  csrc/gemm_bf16.hip:285 gg_fast_wgrad_ok      M * max(lda,ldb) * 2   test_wgrad_2gib[in] / [out]
                                               A / B alignment        test_wgrad_misaligned[in] / [a] / [b]
  csrc/capi.hip:126 use_v2_rowspace            M, N, Kd               test_v2_rowspace_rule[*]
  csrc/capi.hip:132 use_v4_rowspace (gg4_rowspace_ok, gemm_bf16_v4.hip:279)  test_v4_k_pair_rule[*]
  csrc/capi.hip:150 use_v2_wgrad               Na, Nb, M              test_v2_wgrad_rule[*]
  csrc/gemm_generic.hip:162 row-tile limit     grid.y <= 65535        test_generic_row_tile_limit[in] / [out]
  csrc/capi.hip:186 gate_logits fast GEMM      w_gate alignment       test_dense_gemm_misaligned_b[in] / [out]
  csrc/capi.hip:370 dense_gemm fast GEMM       B alignment            test_dense_gemm_misaligned_b[in] / [out]
  csrc/router_fused.hip:171 k_gate_select_ok   E, D % 8, alignment    test_gate_select_guard[*]
  csrc/moe_kernels.hip:1631 k_gate_small_ok    E, D % n, alignment    test_gate_small_guard[*]
  csrc/capi.hip:261 dispatch vec_ok            row bytes, alignment   test_dispatch_vec_guard[*]
  csrc/moe_kernels.hip:1339 combine k2/vec/scalar                     test_combine_paths[*]
  csrc/moe_kernels.hip:1383 combine_bwd k2/vec/scalar                 test_combine_bwd_paths[*]
  csrc/moe_kernels.hip:1490 colsum bf16x8 / f32_wide / plain          test_colsum_paths[*], test_colsum_f32_wide_grid[*]
  csrc/moe_kernels.hip:1540 softplus_mean(_bwd) vec / scalar          test_softplus_paths[*]
  csrc/moe_kernels.hip:1590 pair_cosine(_bwd) vec / scalar            test_pair_cosine_paths[*]
  csrc/capi.hip:499 layernorm D <= k_layernorm_max_d, alignment       test_layernorm_guard[*]
  csrc/capi.hip:718 grouped_gemm_f32w refusals                        test_f32w_refusals[*]
  flat extents past 2^32 bytes (dispatch, combine, dispatch_rows_bwd) test_copy_families_past_4gib

fp64 bound of a bf16 GEMM with fp32 accumulation and one rounding of the output (Higham, fp32 dot products of length Kd):
  |C - C64| <= 2^-8 |C64| + Kd * 2^-23 * (|A| @ |B|)
-- half a bf16 ulp (unit roundoff 2^-8 relative, the tie case included) for the final rounding, plus Kd * u32 (u32 = 2^-24, taken
twice over for the summation error of any association order) times the sum of the magnitudes of the products.  Exact-integer data
(|sum| <= 256) makes every kernel's result exact; those cases assert equality with the fp64 product.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from competesmoe_amd import ops, _lib as L

DEV = "cuda"
BF = torch.bfloat16
GIB2 = 1 << 31


# ------------------------------------------------------------------------------------------------ operand helpers
def misaligned(shape, dtype, elems=1):
    """Contiguous tensor whose base address is elems * itemsize bytes past a 16-byte boundary."""
    n = math.prod(shape)
    buf = torch.empty(n + 64, dtype=dtype, device=DEV)
    isz = buf.element_size()
    lead = (-buf.data_ptr() % 16) // isz            # the caching allocator hands out 256-byte aligned blocks: lead is 0
    t = buf[lead + elems: lead + elems + n].view(shape)
    assert t.data_ptr() % 16 == (elems * isz) % 16 and t.is_contiguous()
    return t


def in_wider(t, pad, sentinel=-7.0):
    """(view, buffer): a row-strided view of t's values inside a [rows, cols + pad] buffer whose extra columns hold `sentinel`."""
    rows, cols = t.shape
    buf = torch.full((rows, cols + pad), sentinel, dtype=t.dtype, device=t.device)
    buf[:, :cols].copy_(t)
    return buf[:, :cols], buf


def sentinel_intact(buf, cols, sentinel=-7.0):
    return bool((buf[:, cols:] == sentinel).all())


def ints(shape, lo=-2, hi=2, seed=0, dtype=BF):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=DEV).to(dtype)


def rnd(shape, seed=0, dtype=BF, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


def gemm_bound_ok(C, A, B):
    """C = A @ B (bf16 output, fp32 accumulation) within the fp64 bound of the module docstring; A [M, Kd], B [Kd, N]."""
    ref = A.double() @ B.double()
    mag = A.double().abs() @ B.double().abs()
    Kd = A.shape[1]
    err = (C.double() - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + Kd * 2.0 ** -23 * mag + 1e-30
    return bool((err <= lim).all()), float((err - lim).max())


def takes_fast_rowspace(A, bp, ldb, N, off, E):
    """Does csmoe_grouped_gemm put this launch on a tiled bf16 kernel?  Only those fill an ACTGRAD_ROWSCALE dot table; the generic
    kernel's side of the guard refuses the table with CSMOE_ERR_UNSUPPORTED before anything is launched."""
    M = A.shape[0]
    scale = torch.ones(M, dtype=torch.float32, device=DEV)
    aux = torch.ones(M, N, dtype=A.dtype, device=DEV)
    cols = max(1, ops.rowdot_cols(M, N, A.shape[1], A.stride(0), ldb, N, A.dtype))
    dot = torch.empty(M, cols, dtype=torch.float32, device=DEV)
    try:
        ops.grouped_gemm(A, bp, L.B_NK, ldb, N, off, E, epilogue=L.EPI_ACTGRAD_ROWSCALE, act=L.ACT_RELU, aux=aux, row_scale=scale,
                         row_dot=dot)
    except L.CsmoeError as e:
        assert "generic kernel" in str(e), e
        return False
    return True


def one_expert(M):
    return torch.tensor([0, M], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ gg_fast_rowspace_ok
def _rowspace_case(A, B, ldb=None):
    """grouped_gemm of one expert, C = A @ B^T (B [N, Kd], row stride ldb) on the kernel the library picks and on the generic one."""
    M, Kd = A.shape
    N = B.shape[0]
    ldb = B.stride(0) if ldb is None else ldb
    bp = ops.ptr_array([B], DEV)
    off = one_expert(M)
    fast = takes_fast_rowspace(A, bp, ldb, N, off, 1)
    c = ops.grouped_gemm(A, bp, L.B_NK, ldb, N, off, 1)
    cg = ops.grouped_gemm(A, bp, L.B_NK, ldb, N, off, 1, force_generic=True)
    return fast, c, cg


@pytest.mark.parametrize("side", ["in", "out"])
def test_rowspace_lda(side):
    M, N, Kd = 300, 72, 64
    A0, B = rnd((M, Kd), 1), rnd((N, Kd), 2, scale=0.125)
    A, buf = in_wider(A0, 8 if side == "in" else 4)
    assert (ops.rowdot_cols(M, N, Kd, A.stride(0), Kd, N, BF) > 0) == (side == "in")
    fast, c, cg = _rowspace_case(A, B)
    assert fast == (side == "in")
    for out in (c, cg):
        ok, worst = gemm_bound_ok(out, A0, B.t())
        assert ok, worst
    assert sentinel_intact(buf, Kd)


@pytest.mark.parametrize("side", ["in", "out"])
def test_rowspace_misaligned_a(side):
    M, N, Kd = 257, 64, 136
    A0, B = rnd((M, Kd), 3), rnd((N, Kd), 4, scale=0.1)
    A = A0 if side == "in" else misaligned((M, Kd), BF)
    A.copy_(A0)
    fast, c, cg = _rowspace_case(A, B)
    assert fast == (side == "in")
    for out in (c, cg):
        ok, worst = gemm_bound_ok(out, A0, B.t())
        assert ok, worst


@pytest.mark.parametrize("side", ["in", "out"])
def test_rowspace_ldb(side):
    M, N, Kd = 200, 64, 64
    A, B0 = rnd((M, Kd), 5), rnd((N, Kd), 6, scale=0.125)
    B, buf = in_wider(B0, 8 if side == "in" else 4)
    assert (ops.rowdot_cols(M, N, Kd, Kd, B.stride(0), N, BF) > 0) == (side == "in")
    fast, c, cg = _rowspace_case(A, B)
    assert fast == (side == "in")
    for out in (c, cg):
        ok, worst = gemm_bound_ok(out, A, B0.t())
        assert ok, worst
    assert sentinel_intact(buf, Kd)


def _sample_rows(M, lda, isz):
    """First row tile, the rows on both sides of the 2^31-byte offset (when inside the operand), the last 64 rows."""
    b = GIB2 // (lda * isz)
    rows = set(range(0, 64)) | set(range(max(0, M - 64), M)) | {r for r in range(b - 64, b + 64) if 0 <= r < M}
    return torch.tensor(sorted(rows), dtype=torch.long, device=DEV)


@pytest.mark.parametrize("side", ["in", "out"])
def test_rowspace_2gib_a(side):
    """A with a huge row stride and few columns: the operand spans 2 GiB (inside: 16 KiB short of it, lda 8192, M 131071) or 4 GiB
    (outside: lda 16384, 131200 rows -- element offsets past 2^31 too, so a 32-bit row offset in the generic kernel is caught).
    Exact-integer data: both kernels must give the exact product."""
    Kd, N = 64, 64
    lda, M = (8192, 131071) if side == "in" else (16384, 131200)
    assert (M * lda * 2 < GIB2) == (side == "in")
    big = torch.empty(M, lda, dtype=BF, device=DEV)
    A = big[:, :Kd]
    A.copy_(ints((M, Kd), seed=7))
    B = ints((N, Kd), seed=8)
    assert (ops.rowdot_cols(M, N, Kd, lda, Kd, N, BF) > 0) == (side == "in")
    fast, c, cg = _rowspace_case(A, B)
    assert fast == (side == "in")
    rows = _sample_rows(M, lda, 2)
    ref = A[rows].double() @ B.double().t()
    assert torch.equal(c[rows].double(), ref)
    assert torch.equal(cg[rows].double(), ref)
    assert torch.equal(c, cg)                      # exact data: the fast and generic kernels agree everywhere
    del big, A, c, cg
    torch.cuda.empty_cache()


@pytest.mark.parametrize("side", ["in", "out"])
def test_rowspace_2gib_b(side):
    """max(N, Kd) * ldb * 2 < 2^31 for the weights: a single B [N, Kd] with a huge row stride (NK layout)."""
    M, Kd, N = 64, 8, 64
    ldb = (GIB2 // 2) // N - 8 if side == "in" else (GIB2 // 2) // N
    assert (N * ldb * 2 < GIB2) == (side == "in")
    big = torch.empty(N, ldb, dtype=BF, device=DEV)
    B = big[:, :Kd]
    B.copy_(ints((N, Kd), seed=9))
    A = ints((M, Kd), seed=10)
    fast, c, cg = _rowspace_case(A, B, ldb=ldb)
    assert fast == (side == "in")
    ref = A.double() @ B.double().t()
    assert torch.equal(c.double(), ref) and torch.equal(cg.double(), ref)
    del big, B
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ kernel-choice rules
@pytest.mark.parametrize("M,N,Kd,v2", [(2047, 256, 128, False), (2048, 256, 128, True), (2048, 248, 128, False),
                                       (2048, 256, 120, False)])
def test_v2_rowspace_rule(M, N, Kd, v2):
    """use_v2_rowspace: N >= 256, Kd >= 128, M >= 2048 -> the 256x256 tile (one dot-table column per 128 output columns), else the
    128x128 tile (one per 8).  Both sides against fp64."""
    cols = ops.rowdot_cols(M, N, Kd, Kd, Kd, N, BF)
    assert cols == ((N + 127) // 128 if v2 else N // 8)
    E = 3
    off = torch.tensor([0, M // 3, M // 3, M], dtype=torch.int32, device=DEV)      # expert 1 empty
    A = rnd((M, Kd), M + N)
    Bs = [rnd((N, Kd), 20 + e, scale=Kd ** -0.5) for e in range(E)]
    c = ops.grouped_gemm(A, ops.ptr_array(Bs, DEV), L.B_NK, Kd, N, off, E)
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        if r1 > r0:
            ok, worst = gemm_bound_ok(c[r0:r1], A[r0:r1], Bs[e].t())
            assert ok, (e, worst)


@pytest.mark.parametrize("Kd,layout", [(128, 0), (192, 0), (128, 1)])
def test_v4_k_pair_rule(Kd, layout):
    """gg4_rowspace_ok: the one-wave-per-SIMD kernel takes K-contiguous weights with an even number of 64-deep K-tiles; a request for
    it (kernel=4) on any other launch runs the 8-wave kernel.  Both against fp64 and against each other's bound."""
    M, N, E = 2048, 256, 2
    off = torch.tensor([0, 1000, M], dtype=torch.int32, device=DEV)
    A = rnd((M, Kd), Kd + layout)
    shape = (N, Kd) if layout == 0 else (Kd, N)
    Bs = [rnd(shape, 30 + e, scale=Kd ** -0.5) for e in range(E)]
    bp = ops.ptr_array(Bs, DEV)
    for kernel in (4, 2, 0):                         # CSMOE_KERNEL_V4, CSMOE_KERNEL_V2, automatic
        c = ops.grouped_gemm(A, bp, layout, Bs[0].stride(0), N, off, E, kernel=kernel)
        for e in range(E):
            r0, r1 = int(off[e]), int(off[e + 1])
            ok, worst = gemm_bound_ok(c[r0:r1], A[r0:r1], Bs[e].t() if layout == 0 else Bs[e])
            assert ok, (kernel, e, worst)


@pytest.mark.parametrize("M,Na,Nb", [(512, 256, 256), (511, 256, 256), (512, 248, 256), (512, 256, 248)])
def test_v2_wgrad_rule(M, Na, Nb):
    """use_v2_wgrad: Na >= 256, Nb >= 256, M >= 512 -> the 256-tile weight gradient, else the 128-tile one; fp32 output."""
    E = 2
    off = torch.tensor([0, M // 2, M], dtype=torch.int32, device=DEV)
    A, B = rnd((M, Na), M + Na), rnd((M, Nb), Nb)
    out = torch.full((E, Na, Nb), float("nan"), device=DEV)
    ops.grouped_wgrad(A, B, off, E, out, ops.ptr_table(out, E, Na * Nb * 4))
    for e in range(E):
        r0, r1 = int(off[e]), int(off[e + 1])
        ref = A[r0:r1].double().t() @ B[r0:r1].double()
        mag = A[r0:r1].double().abs().t() @ B[r0:r1].double().abs()
        assert ((out[e].double() - ref).abs() <= (r1 - r0) * 2.0 ** -23 * mag + 1e-30).all()


# ------------------------------------------------------------------------------------------------ gg_fast_wgrad_ok
@pytest.mark.parametrize("side", ["in", "out"])
def test_wgrad_2gib(side):
    """M * max(lda, ldb) * 2 < 2^31: A [M, 64] with a huge row stride; exact-integer data, fp32 output (sums < 2^24: exact)."""
    Na = Nb = 64
    lda, M = (8192, 131071) if side == "in" else (8192, 131200)
    assert (M * lda * 2 < GIB2) == (side == "in")
    big = torch.empty(M, lda, dtype=BF, device=DEV)
    A = big[:, :Na]
    A.copy_(ints((M, Na), -1, 1, seed=11))
    B = ints((M, Nb), -1, 1, seed=12)
    ref = A.double().t() @ B.double()
    for generic in (False, True):
        out = ops.dense_wgrad(A, B, out_dtype=torch.float32, force_generic=generic)
        assert torch.equal(out.double(), ref), generic
    del big, A
    torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ["in", "a", "b"])
def test_wgrad_misaligned(which):
    M, Na, Nb = 700, 64, 72
    A0, B0 = rnd((M, Na), 13), rnd((M, Nb), 14)
    A = misaligned((M, Na), BF) if which == "a" else A0.clone()
    B = misaligned((M, Nb), BF) if which == "b" else B0.clone()
    A.copy_(A0)
    B.copy_(B0)
    out = ops.dense_wgrad(A, B, out_dtype=torch.float32)
    ref = A0.double().t() @ B0.double()
    mag = A0.double().abs().t() @ B0.double().abs()
    assert ((out.double() - ref).abs() <= M * 2.0 ** -23 * mag + 1e-30).all()


# ------------------------------------------------------------------------------------------------ generic row-tile limit
@pytest.mark.parametrize("side", ["in", "out"])
def test_generic_row_tile_limit(side):
    """gg_generic_rowspace launches ceil(M / 64) + E row tiles in grid.y (<= 65535): M = 65534 * 64 runs, one row more is refused with
    CSMOE_ERR_UNSUPPORTED before anything is written.  fp32 (always the generic kernel), Kd = N = 8, exact-integer data."""
    M = 65534 * 64 if side == "in" else 65534 * 64 + 1
    A = ints((M, 8), seed=15, dtype=torch.float32)
    B = ints((8, 8), seed=16, dtype=torch.float32)
    out = torch.full((M, 8), -7.0, device=DEV)
    if side == "in":
        ops.dense_gemm(A, B, L.B_NK, out=out)
        assert torch.equal(out.double(), A.double() @ B.double().t())
    else:
        with pytest.raises(L.CsmoeError, match="too many row tiles"):
            ops.dense_gemm(A, B, L.B_NK, out=out)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
    del A, out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ single-B alignment
@pytest.mark.parametrize("side", ["in", "out"])
def test_dense_gemm_misaligned_b(side):
    """csmoe_dense_gemm / csmoe_gate_logits hand a host-visible B to the tiled kernel, which reads it in 16-byte pieces: a misaligned B
    must take the generic kernel (this guard was missing: only A and C were checked)."""
    M, N, Kd = 300, 64, 64
    A, B0 = rnd((M, Kd), 17), rnd((N, Kd), 18, scale=0.125)
    B = B0 if side == "in" else misaligned((N, Kd), BF)
    B.copy_(B0)
    c = ops.dense_gemm(A, B, L.B_NK)
    ok, worst = gemm_bound_ok(c, A, B0.t())
    assert ok, worst
    lg = ops.gate_logits(A, B)                       # E = 64 > 4: the GEMM path of the gate
    ok, worst = gemm_bound_ok(lg, A, B0.t())
    assert ok, worst


# ------------------------------------------------------------------------------------------------ router guards
@pytest.mark.parametrize("case", ["in", "E65", "D68", "misaligned"])
def test_gate_select_guard(case):
    """k_gate_select_ok: bf16, E <= 64, D % 8 == 0, 16-byte aligned x and w_gate.  Outside, csmoe_gate_select refuses and the
    two-launch router (gate_logits + router_select) gives the routing the one-pass router gives on the aligned copy.  Exact-integer
    data: every logits kernel gives the same exact logits."""
    T, K = 300, 2
    D = 68 if case == "D68" else 64
    E = 65 if case == "E65" else 64
    x0, wg = ints((T, D), -1, 1, seed=19), ints((E, D), -1, 1, seed=20)
    x = misaligned((T, D), BF) if case == "misaligned" else x0.clone()
    x.copy_(x0)
    assert ops.gate_select_ok(x, wg, K) == (case == "in")
    exact = (x0.double() @ wg.double().t())
    lg = ops.gate_logits(x, wg)
    assert torch.equal(lg.double(), exact)
    sm2, idx2, w2 = ops.router_select(lg, K, L.SEL_SOFTMAX, True)
    if case == "in":
        logits, sm, idx, w = ops.gate_select(x, wg, K, L.SEL_SOFTMAX, True)
        assert torch.equal(logits, lg) and torch.equal(idx, idx2) and torch.equal(w, w2) and torch.equal(sm, sm2)
    else:
        with pytest.raises(ValueError, match="gate_select"):
            ops.gate_select(x, wg, K, L.SEL_SOFTMAX, True)
        if case == "misaligned":
            _, sm, idx, w = ops.gate_select(x0, wg, K, L.SEL_SOFTMAX, True)
            assert torch.equal(idx, idx2) and torch.equal(w, w2) and torch.equal(sm, sm2)


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("case", ["in", "E5", "Dodd", "misaligned"])
def test_gate_small_guard(case, dt):
    """k_gate_small_ok: E <= 4, D a whole number of 16-byte chunks, aligned operands -> the row-pass kernels; else the GEMM.  The
    backward entries refuse outside it (csmoe_gate_bwd_small_ok tells the caller)."""
    T = 333
    n = 8 if dt == BF else 4
    D = 64 + (n // 2 if case == "Dodd" else 0)
    E = 5 if case == "E5" else 4
    x0, wg = ints((T, D), -1, 1, seed=21, dtype=dt), ints((E, D), -1, 1, seed=22, dtype=dt)
    x = misaligned((T, D), dt) if case == "misaligned" else x0.clone()
    x.copy_(x0)
    lg = ops.gate_logits(x, wg)
    assert torch.equal(lg.double(), x0.double() @ wg.double().t())
    assert ops.gate_bwd_small_ok(D, E, dt) == (case in ("in", "misaligned"))
    dl = ints((T, E), -1, 1, seed=23, dtype=dt)
    if ops.gate_bwd_small_ok(D, E, dt):
        assert torch.equal(ops.gate_bwd_dx(dl, wg).double(), dl.double() @ wg.double())
        if case == "misaligned":
            with pytest.raises(ValueError, match="gate_bwd_dw"):
                ops.gate_bwd_dw(dl, x, torch.float32)
        else:
            assert torch.equal(ops.gate_bwd_dw(dl, x, torch.float32).double(), dl.double().t() @ x0.double())
    else:
        with pytest.raises(ValueError, match="gate_bwd_dx"):
            ops.gate_bwd_dx(dl, wg)


# ------------------------------------------------------------------------------------------------ dispatch / combine
def _bins(T, K, E, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.rand(T, E, generator=g).topk(K, dim=-1).indices.int().to(DEV)
    return idx, ops.bin_tokens(idx, E)


@pytest.mark.parametrize("case,vec", [("in", 1), ("rowbytes", 0), ("misaligned", 0), ("f32", 1), ("f32_rowbytes", 0)])
def test_dispatch_vec_guard(case, vec):
    """dispatch vec_ok: rows of a whole number of 16 bytes and 16-byte aligned x / xs -> 16-byte copies; else 2-byte copies.
    Both entries, exact equality with torch indexing."""
    dt = torch.float32 if case.startswith("f32") else BF
    D = {"in": 64, "rowbytes": 68, "misaligned": 64, "f32": 64, "f32_rowbytes": 66}[case]
    T, K, E = 513, 2, 8
    idx, b = _bins(T, K, E, D)
    x0 = rnd((T, D), D, dtype=dt)
    x = misaligned((T, D), dt) if case == "misaligned" else x0.clone()
    x.copy_(x0)
    xs_probe = torch.empty(8, D, dtype=dt, device=DEV)
    assert L.lib.csmoe_dispatch_vec_ok(x.data_ptr(), xs_probe.data_ptr(), D, ops._dt(x)) == vec
    ref = x0[(b.perm // K).long()]
    assert torch.equal(ops.dispatch_rows(x, b), ref)
    assert torch.equal(ops.dispatch_tokens(x, b), ref)


def _combine_ref_seq(y, b, idx, w, T, K, dt, mode):
    """mode 0 / 2: sequential accumulation in ascending expert order, x.dtype rounding after every add (exact reference)."""
    yk = y[b.slot_of.long()].view(T, K, -1)
    order = idx.long().argsort(dim=-1, stable=True)
    ref = torch.zeros(T, y.shape[1], dtype=dt, device=DEV)
    ar = torch.arange(T, device=DEV)
    for j in range(K):
        k = order[:, j]
        prod = w[ar, k].unsqueeze(-1) * yk[ar, k].float()
        if mode == 2:
            prod = prod.to(dt).float()
        ref = (ref.float() + prod).to(dt)
    return ref


@pytest.mark.parametrize("case", ["k2", "vec", "scalar", "misaligned"])
def test_combine_paths(case):
    """combine: K = 2 and D % 512 == 0 and aligned -> the K=2 kernel; D % 8 == 0 and aligned -> the 8-wide kernel; else scalar.
    Sequential modes: exact; DOT mode: fp64 bound 2^-8 |ref| + 2^-22 sum |w y| (one rounding of an fp32 sum of K terms)."""
    T, K, E = 300, 2, 8
    D = {"k2": 512, "vec": 520, "scalar": 516, "misaligned": 512}[case]
    idx, b = _bins(T, K, E, D + 1)
    y0 = rnd((T * K, D), D)
    y = misaligned((T * K, D), BF) if case == "misaligned" else y0.clone()
    y.copy_(y0)
    w = torch.rand(T, K, generator=torch.Generator().manual_seed(D)).to(DEV)
    for mode in (0, 2):
        wm = w.to(BF).float() if mode == 2 else w
        assert torch.equal(ops.combine(y, b, idx, wm, mode, T), _combine_ref_seq(y0, b, idx, wm, T, K, BF, mode)), mode
    out = ops.combine(y, b, idx, w, L.COMBINE_DOT, T)
    yk = y0[b.slot_of.long()].view(T, K, D).double()
    ref = (w.double().unsqueeze(-1) * yk).sum(1)
    mag = (w.double().unsqueeze(-1) * yk).abs().sum(1)
    assert ((out.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -22 * mag + 1e-30).all()


@pytest.mark.parametrize("case", ["k2", "vec", "scalar", "misaligned"])
def test_combine_bwd_paths(case):
    """combine_bwd: dy = round(w * dout[t]) exact on every path; dw = <dout[t], y[slot]> within D * 2^-23 sum |dout y| of fp64."""
    T, K, E = 300, 2, 8
    D = {"k2": 512, "vec": 520, "scalar": 516, "misaligned": 512}[case]
    idx, b = _bins(T, K, E, D + 2)
    y = rnd((T * K, D), D + 3)
    d0 = rnd((T, D), D + 4)
    dout = misaligned((T, D), BF) if case == "misaligned" else d0.clone()
    dout.copy_(d0)
    w = torch.rand(T, K, generator=torch.Generator().manual_seed(D)).to(DEV)
    dy, dw = ops.combine_bwd(dout, y, b, w)
    ft = (b.perm // K).long()
    assert torch.equal(dy, (d0[ft].float() * w.flatten()[b.perm.long()].unsqueeze(-1)).to(BF))
    yk = y[b.slot_of.long()].view(T, K, D).double()
    prod = d0.double().unsqueeze(1) * yk
    assert ((dw.double() - prod.sum(-1)).abs() <= D * 2.0 ** -23 * prod.abs().sum(-1) + 1e-30).all()


# ------------------------------------------------------------------------------------------------ small reductions
@pytest.mark.parametrize("case", ["bf16x8", "bf16_N", "bf16_ldg", "bf16_misaligned"])
def test_colsum_paths(case):
    """colsum (bf16 rows): N % 8, ldg % 8 and an aligned G -> the 8-wide kernel; else the plain one.  fp32 output within
    M * 2^-23 sum |g| of fp64."""
    M = 300
    N = 204 if case == "bf16_N" else 200
    G0 = rnd((M, N), N)
    if case == "bf16_ldg":
        G, buf = in_wider(G0, 4)
    elif case == "bf16_misaligned":
        G = misaligned((M, N), BF)
        G.copy_(G0)
    else:
        G = G0
    out = ops.dense_colsum(G, torch.float32)
    ref, mag = G0.double().sum(0), G0.double().abs().sum(0)
    assert ((out.double() - ref).abs() <= M * 2.0 ** -23 * mag + 1e-30).all()
    if case == "bf16_ldg":
        assert sentinel_intact(buf, N)


@pytest.mark.parametrize("E,wide", [(256, True), (255, False)])
def test_colsum_f32_wide_grid(E, wide):
    """colsum (fp32 rows): the wide kernel needs ((N / 8 + 255) / 256) * E >= 256 blocks; N = 2048 puts the edge at E = 256."""
    N, rows = 2048, 3
    M = E * rows
    off = (torch.arange(E + 1, dtype=torch.int32) * rows).to(DEV)
    G = rnd((M, N), E, dtype=torch.float32)
    assert ((N // 8 + 255) // 256) * E >= 256 if wide else ((N // 8 + 255) // 256) * E < 256
    out = torch.full((E, N), float("nan"), device=DEV)
    ops.grouped_colsum(G, off, E, out, ops.ptr_table(out, E, N * 4))
    Gd = G.double().view(E, rows, N)
    assert ((out.double() - Gd.sum(1)).abs() <= rows * 2.0 ** -23 * Gd.abs().sum(1) + 1e-30).all()


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("case", ["vec", "Dodd", "misaligned"])
def test_softplus_paths(case, dt):
    """softplus_mean(_bwd): D a multiple of the vector width and aligned rows -> the vector kernel, else scalar.  fp32 affinities
    within 1e-5 relative of fp64 (hardware exp / log: a few fp32 ulps per term); bf16 dy within 2^-7 relative."""
    R = 300
    D = 100 if case == "Dodd" else 96
    if dt == torch.float32 and case == "Dodd":
        D = 98
    y0 = rnd((R, D), D, dtype=dt, scale=3.0)
    y = misaligned((R, D), dt) if case == "misaligned" else y0.clone()
    y.copy_(y0)
    aff = ops.softplus_mean(y, torch.float32)
    ref = torch.nn.functional.softplus(y0.double()).mean(-1)
    assert ((aff.double() - ref).abs() <= 1e-5 * ref.abs() + 1e-7).all()
    daff = torch.randn(R, generator=torch.Generator().manual_seed(1)).to(DEV)
    dy = ops.softplus_mean_bwd(y, daff)
    rdy = (daff.double() / D).unsqueeze(-1) * torch.sigmoid(y0.double())
    rel = 2.0 ** -7 if dt == BF else 1e-5
    assert ((dy.double() - rdy).abs() <= rel * rdy.abs() + 1e-12).all()


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("case", ["vec", "Dodd", "misaligned"])
def test_pair_cosine_paths(case, dt):
    """pair_cosine(_bwd): vector kernel for D % width == 0 and aligned y, else scalar.  tok_loss = sum_{i != j} cos(y_i, y_j) within
    1e-5 * K^2 of fp64; dy against the fp64 autograd of the same sum (bf16: 2^-7 relative + 1e-3 of the row's largest)."""
    T, K = 129, 3
    D = (68 if dt == BF else 66) if case == "Dodd" else 64
    y0 = rnd((T, K, D), D + K, dtype=dt, scale=1.5)
    y = misaligned((T, K, D), dt) if case == "misaligned" else y0.clone()
    y.copy_(y0)
    tok = ops.pair_cosine(y)
    yr = y0.double().requires_grad_(True)
    n = torch.nn.functional.normalize(yr, p=2, dim=-1)
    sim = (n @ n.transpose(1, 2)) * (1 - torch.eye(K, device=DEV, dtype=torch.float64))
    ref = sim.sum((1, 2))
    assert ((tok.double() - ref.detach()).abs() <= 1e-5 * K * K).all()
    gs = torch.tensor([0.37], device=DEV)
    dy = ops.pair_cosine_bwd(y, gs)
    (rdy,) = torch.autograd.grad(ref.sum() * 0.37, yr)
    lim = (2.0 ** -7 if dt == BF else 1e-5) * rdy.abs() + 1e-3 * rdy.abs().amax(-1, keepdim=True)
    assert ((dy.double() - rdy).abs() <= lim).all()


# ------------------------------------------------------------------------------------------------ layernorm
@pytest.mark.parametrize("case", ["in", "D4104", "misaligned"])
def test_layernorm_guard(case):
    """csmoe_layernorm_gate: D <= k_layernorm_max_d (4096) and 16-byte aligned operands, else refused (ValueError, nothing written)."""
    T = 64
    D = 4104 if case == "D4104" else 4096
    x0 = rnd((T, D), D)
    x = misaligned((T, D), BF) if case == "misaligned" else x0.clone()
    x.copy_(x0)
    gamma = rnd((D,), 1, scale=0.2) + 1
    beta = rnd((D,), 2, scale=0.1)
    if case == "in":
        xn, mean, rstd, _ = ops.layernorm_gate(x, gamma, beta, 1e-5)
        ref = torch.nn.functional.layer_norm(x0.double(), (D,), gamma.double(), beta.double(), 1e-5)
        assert ((xn.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-3).all()
    else:
        with pytest.raises(ValueError, match="unsupported" if case == "D4104" else "16-byte aligned"):
            ops.layernorm_gate(x, gamma, beta, 1e-5)


# ------------------------------------------------------------------------------------------------ fp32-master GEMM refusals
@pytest.mark.parametrize("case", ["in", "misaligned_a", "a_2gib"])
def test_f32w_refusals(case):
    """csmoe_grouped_gemm_f32w refuses misaligned rows and operands of 2 GiB or more (CSMOE_ERR_UNSUPPORTED, before any launch).
    The split condition that followed (Kd * N * 2 < 2^31) could never be false once Kd * ldb * 4 < 2^31 and ldb >= N had passed, and
    is gone.  Inside: exact-integer data, the exact product."""
    N, Kd, E = 256, 128, 1
    M = 131071 if case == "in" else (131072 if case == "a_2gib" else 300)
    B32 = ints((E, Kd, N), -1, 1, seed=24, dtype=torch.float32)
    off = one_expert(M)
    if case == "misaligned_a":
        A = misaligned((M, Kd), BF)
        A.copy_(ints((M, Kd), -1, 1, seed=25))
        big = None
    else:
        big = torch.empty(M, 8192, dtype=BF, device=DEV)
        A = big[:, :Kd]
        A.copy_(ints((M, Kd), -1, 1, seed=25))
    copy = torch.full((E, Kd, N), -7.0, dtype=BF, device=DEV)
    if case == "in":
        c = ops.grouped_gemm_f32w(A, B32, off, copy=copy)
        rows = _sample_rows(M, 8192, 2)
        assert torch.equal(c[rows].double(), A[rows].double() @ B32[0].double())
        assert torch.equal(copy.float(), B32)
    else:
        with pytest.raises(L.CsmoeError, match="grouped_gemm_f32w"):
            ops.grouped_gemm_f32w(A, B32, off, copy=copy)
        torch.cuda.synchronize()
        assert bool((copy == -7.0).all())
    del big, A
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ byte extents past 2^32
def test_copy_families_past_4gib():
    """dispatch, combine and dispatch_rows_bwd over T = 300000 tokens, K = 2, D = 4096 bf16: the binned rows span 4.9 GB, past 2^32
    bytes.  Sampled rows (the first, those around the 2^31 and 2^32 byte offsets, the last) exactly against torch."""
    T, K, E, D = 300000, 2, 8, 4096
    n = T * K
    idx, b = _bins(T, K, E, 99)
    x = torch.empty(T, D, dtype=BF, device=DEV)
    x.copy_(torch.arange(T, device=DEV, dtype=torch.float32).remainder(251).unsqueeze(1).to(BF))
    x[:, 1::2] = -x[:, 1::2]
    row_b = D * 2
    samp = sorted({*range(0, 8), *range(n - 8, n), *[s + d for s in (GIB2 // row_b, (2 * GIB2) // row_b) for d in range(-4, 4)]})
    ms = torch.tensor(samp, dtype=torch.long, device=DEV)
    xs = ops.dispatch_rows(x, b)
    assert torch.equal(xs[ms], x[(b.perm[ms] // K).long()])
    xs2 = ops.dispatch_tokens(x, b)
    assert torch.equal(xs2[ms], xs[ms])
    del xs2
    tsamp = torch.tensor(sorted({*range(0, 8), *range(T - 8, T), T // 2}), dtype=torch.long, device=DEV)
    w = torch.rand(T, K, generator=torch.Generator().manual_seed(5)).to(DEV)
    out = ops.combine(xs, b, idx, w, 0, T)
    sl = b.slot_of.view(T, K)[tsamp].long()
    ysl = xs[sl.flatten()].view(-1, K, D)
    ref = _combine_ref_seq(ysl.reshape(-1, D), ops.Bins(None, None, None, torch.arange(len(tsamp) * K, dtype=torch.int32, device=DEV),
                                                          len(tsamp) * K, E, K), idx[tsamp], w[tsamp], len(tsamp), K, BF, 0)
    assert torch.equal(out[tsamp], ref)
    del out
    dx = ops.dispatch_rows_bwd(xs, b, T)
    assert torch.equal(dx[tsamp], ysl.float().sum(1).to(BF))       # two bf16 terms: the fp32 sum is exact, one rounding
    del xs, dx, x
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ layout contract of the ops wrappers
def _mis_copy(t):
    m = misaligned(tuple(t.shape), t.dtype)
    m.copy_(t)
    return m


def _colslice(t):
    if t.dim() == 1:
        return in_wider(t.view(-1, 1), 1)[0].view(-1)            # stride 2
    lead, last = t.shape[:-1], t.shape[-1]
    v, _ = in_wider(t.reshape(-1, last), 8)
    return v.as_strided(t.shape, tuple(s * (last + 8) // last if i < t.dim() - 1 else 1 for i, s in enumerate(t.stride())))


def _transposed(t):
    if t.dim() == 1:
        return t
    return t.transpose(0, 1).contiguous().transpose(0, 1)


def _contract(fn, args, which, cmp):
    """fn(*args) with args[which] given as a column-sliced view, a transposed view and a misaligned contiguous copy: each gives the
    contiguous input's result (cmp) or raises ValueError."""
    ref = fn(*args)
    for name, tf in (("colslice", _colslice), ("transposed", _transposed), ("misaligned", _mis_copy)):
        a = list(args)
        a[which] = tf(args[which])
        assert torch.equal(a[which], args[which])
        if name != "misaligned" and a[which].is_contiguous():
            continue                                              # a view that happens to be dense (1-D, or a single row)
        try:
            got = fn(*a)
        except ValueError:
            continue
        cmp(got, ref, name)


def _eq(got, ref, name):
    got = got if isinstance(got, (tuple, list)) else (got,)
    ref = ref if isinstance(ref, (tuple, list)) else (ref,)
    for g_, r_ in zip(got, ref):
        if r_ is not None:
            assert torch.equal(g_, r_), name


def _close(rel):
    def cmp(got, ref, name):
        got = got if isinstance(got, (tuple, list)) else (got,)
        ref = ref if isinstance(ref, (tuple, list)) else (ref,)
        for g_, r_ in zip(got, ref):
            if r_ is not None:
                assert ((g_.double() - r_.double()).abs() <= rel * r_.double().abs() + rel * r_.double().abs().max()).all(), name
    return cmp


def test_wrapper_layout_contract():
    """Every wrapper that hands data_ptr() to the C ABI: a view that is not dense row-major gives the contiguous result or raises
    ValueError (ops._rows), never a silently wrong answer; a misaligned contiguous tensor takes a scalar kernel (same bits where the
    kernels round at the same points) or is refused."""
    T, K, E, D = 96, 2, 8, 64
    idx, b = _bins(T, K, E, 7)
    x = ints((T, D), -1, 1, seed=1)
    wg = ints((E, D), -1, 1, seed=2)
    _contract(ops.gate_logits, (x, wg), 0, _eq)
    _contract(ops.gate_logits, (x, wg), 1, _eq)
    scores = rnd((T, E), 3)
    _contract(lambda s: ops.router_select(s, K, L.SEL_SOFTMAX, True), (scores,), 0, _eq)
    sm, ix, w = ops.router_select(scores, K, L.SEL_SOFTMAX, True)
    dw = torch.randn(T, K, device=DEV)
    _contract(lambda s, d: ops.router_select_bwd(s, K, L.SEL_SOFTMAX, True, sm, ix, w, d, None), (scores, dw), 0, _eq)
    _contract(lambda s, d: ops.router_select_bwd(s, K, L.SEL_SOFTMAX, True, sm, ix, w, d, None), (scores, dw), 1, _eq)
    _contract(lambda lg, s: ops.router_aux(lg.view(2, T // 2, E), s.view(2, T // 2, E), ix.view(2, T // 2, K)), (scores, sm), 1,
              _eq)
    _contract(lambda xx: ops.dispatch_rows(xx, b), (x,), 0, _eq)
    _contract(lambda xx: ops.dispatch_tokens(xx, b), (x,), 0, _eq)
    dxs = ints((T * K, D), -2, 2, seed=4)
    add = ints((T, D), -2, 2, seed=5)
    _contract(lambda d, a: ops.dispatch_rows_bwd(d, b, T, add=a), (dxs, add), 0, _eq)
    _contract(lambda d, a: ops.dispatch_rows_bwd(d, b, T, add=a), (dxs, add), 1, _eq)
    wc = torch.rand(T, K, generator=torch.Generator().manual_seed(1)).to(DEV)
    y = rnd((T * K, D), 6)
    _contract(lambda yy, ww: ops.combine(yy, b, idx, ww, L.COMBINE_SEQ, T), (y, wc), 0, _eq)
    _contract(lambda yy, ww: ops.combine(yy, b, idx, ww, L.COMBINE_SEQ, T), (y, wc), 1, _eq)
    dout = rnd((T, D), 7)
    _contract(lambda d, yy: ops.combine_bwd(d, yy, b, wc)[0], (dout, y), 0, _eq)
    _contract(lambda d, yy: ops.combine_bwd(d, yy, b, wc), (dout, y), 1, _close(2.0 ** -20))
    _contract(lambda r: ops.scale_rows(r, wc.flatten()), (y,), 0, _eq)
    _contract(lambda a_, b_: ops.widen_sum([a_, b_]), (dout, add), 0, _eq)
    ys = rnd((T, 96), 8, scale=3.0)
    _contract(lambda yy: ops.softplus_mean(yy, torch.float32), (ys,), 0, _close(1e-6))
    da = torch.randn(T, device=DEV)
    _contract(lambda yy: ops.softplus_mean_bwd(yy, da), (ys,), 0, _close(2.0 ** -8))
    y3 = rnd((T, 3, D), 9)
    _contract(ops.pair_cosine, (y3,), 0, _close(1e-5))
    _contract(lambda yy: ops.pair_cosine_bwd(yy, torch.tensor([0.5], device=DEV)), (y3,), 0, _close(2.0 ** -7))
    g = rnd((D,), 10, scale=0.1) + 1
    _contract(lambda xx: ops.layernorm_gate(xx, g, None, 1e-5, wg)[:2], (rnd((T, D), 11),), 0, _eq)


def test_combine_refuses_a_column_slice():
    """ops.combine on a row-strided y: ValueError before anything is launched, not a combine of the wrong elements."""
    T, K, E, D = 64, 2, 4, 64
    idx, b = _bins(T, K, E, 3)
    y, _ = in_wider(rnd((T * K, D), 1), 8)
    with pytest.raises(ValueError, match="dense row-major"):
        ops.combine(y, b, idx, torch.rand(T, K, device=DEV), L.COMBINE_SEQ, T)


# ------------------------------------------------------------------------------------------------ layers on a view of a wider buffer
def _layer_run(layer, x, call):
    layer.zero_grad(set_to_none=True)
    xi = x.detach().clone() if x.is_contiguous() else x.detach()
    xi.requires_grad_(True)
    out = call(layer, xi)
    out.float().pow(2).mean().backward()
    grads = [p.grad.clone() for p in layer.parameters() if p.grad is not None]
    return out.detach().clone(), xi.grad.clone(), grads


def _same_on_view(layer, D, call, dt):
    g = torch.Generator(device=DEV).manual_seed(5)
    buf = torch.randn(2, 96, D + 24, generator=g, device=DEV).to(dt)
    view = buf[..., :D]
    assert not view.is_contiguous()
    a = _layer_run(layer, view, call)
    b = _layer_run(layer, view.contiguous(), call)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert len(a[2]) == len(b[2]) and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


@pytest.mark.parametrize("name", ["smoe", "competesmoe"])
def test_pretrain_layer_on_a_column_slice(name):
    """pretrain smoe / competesmoe forward + backward on buf[..., :D] equal the run on its contiguous copy, bit for bit."""
    import types
    import torch.nn.functional as F
    from competesmoe_amd.pretrain import get_moe
    D, E, Fh, K = 64, 8, 128, 2
    args = types.SimpleNamespace(stop_after=10, warm_up=0.0, rate_flip=1.0, max_compete_in_iter=8, balance_loss_coef=0.01,
                                 balance_loss_coef_comp=0.02, router_loss_coef=0.03, router_theta=0.5, in_topk=False, hybrid=False,
                                 tribrid=False, balance_affinity=False, is_cosine=False, is_norm_weight=False, norm_sigmoid=False,
                                 scale_weight=1.0, test_only=False)
    torch.manual_seed(11)
    layer = get_moe(name)(D, E, Fh, n_heads=K, activation=F.relu, bias=False, log_interval=None, args=args).to(DEV).train()
    layer.regularization_present = True
    if name == "competesmoe":
        layer.step_warm, layer.flip_steps = 0, 2
        layer.prob_flips_final = {0: torch.tensor([False, True], device=DEV)}
    for cur in ((0, 1) if name == "competesmoe" else (0,)):
        def call(lay, xi):
            if name == "competesmoe":
                lay.set_current_steps(cur)
            return lay(xi, id_layer=0)
        _same_on_view(layer, D, call, torch.float32)


def test_llava_moe_layer_on_a_column_slice():
    """The LLaVA `smoe` MoeLayer forward + backward on buf[..., :D] equal the run on its contiguous copy, bit for bit."""
    import types
    import torch.nn as nn
    from competesmoe_amd.moe.smoe import SMoeLayer
    D, F, E, K = 64, 128, 8, 2
    torch.manual_seed(3)
    expert = nn.Sequential(nn.Linear(D, F), nn.GELU(), nn.Linear(F, D))
    args = types.SimpleNamespace(balance_loss_coef=0.01, router_z_loss_coef=0.001)
    layer = SMoeLayer(D, D, E, K, expert, args).to(DEV).to(BF)
    _same_on_view(layer, D, lambda lay, xi: lay(xi)[0], BF)
