"""The quantised output of the tiled MXFP8 GEMM (csmoe_dense_gemm_mxfp8_q / csmoe_grouped_gemm_mxfp8_q, csrc/gemm_epilogue_q.h) and
the affinity epilogues on MXFP8 operands.

Quantised output: Cq / Cs are compared byte for byte with the two launches they replace -- the existing entry on the same operands,
then ops.quantize_mxfp8(C2) -- and C / C2 of the new launch bit for bit with the existing entry's (as int16 words, so that a NaN
compares equal to itself).  Shapes are the smallest at which the epilogue can go wrong: a thin tile with a quarter-filled column tile
and one K-tile; a full row tile + 44 rows whose second column tile holds ONE 32-column block; three column tiles and three K-tiles;
grouped: an empty expert, then one with a single row beyond a full tile.  N(0, 1) operands; input row 1 is zeroed, because 32
independent N(0, 1) products are all negative once in 2^32 blocks, so ReLU alone gives no all-zero block (scale byte 0) at these sizes:
without a bias row 1 of the output is all-zero blocks under both activations.  One case puts a NaN into one input row and an Inf
into another.  Cq / Cs carry 8 guard rows of 0xA5.

Affinity epilogues: tests/test_ops_gpu.py::test_affinity_epilogues_match_gemm_then_softplus_mean on MXFP8 operands -- y = the existing
plain fp8 dense GEMM, then the softplus_mean kernels; the bounds are those of a re-ordered fp32 row sum (2^-7 relative on bf16
affinities, 2e-6 on fp32 ones) and do not depend on the operand type; the gradient is bit-equal."""
import functools

import pytest
import torch

from competesmoe_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8

if torch.cuda.is_available():
    from competesmoe_amd import ops

DENSE = [(40, 64, 128), (300, 288, 256), (700, 544, 384)]
GROUPED = ([0, 0, 257, 300, 700], 288, 256)
ACTS = [L.ACT_RELU, L.ACT_GELU]
OUTSETS = ["q", "c2+q", "c+c2+q"]


def _bits(t):
    return t.view(torch.int16)


def _guarded(M, N):
    q = torch.full((M + GUARD, N), 0xA5, dtype=torch.uint8, device=DEV)
    s = torch.full((M + GUARD, N // 32), 0xA5, dtype=torch.uint8, device=DEV)
    return q, s


def _check_guard(q, s, M):
    assert bool((q[M:] == 0xA5).all()) and bool((s[M:] == 0xA5).all()), "guard rows written"


@functools.lru_cache(maxsize=None)
def _dense_case(M, N, Kd, act, bias, nonfinite=False):
    """Operands and the parent's two launches, computed once per case and left unchanged."""
    g = torch.Generator(device=DEV).manual_seed(M + N + Kd)
    A = torch.randn(M, Kd, device=DEV, generator=g).to(torch.bfloat16)
    A[1] = 0
    if nonfinite:
        A[3, 5] = float("nan")
        A[7, 9] = float("inf")
    B = torch.randn(N, Kd, device=DEV, generator=g).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16) if bias else None
    Aq, As = ops.quantize_mxfp8(A)
    Bq, Bs = ops.quantize_mxfp8(B)
    C, C2 = ops.dense_gemm_mxfp8(Aq, As, Bq, Bs, bias=b, epilogue=L.EPI_BIAS_ACT, act=act, want_c2=True)
    q, s = ops.quantize_mxfp8(C2)
    return Aq, As, Bq, Bs, b, C, C2, q, s


@pytest.mark.parametrize("outset", OUTSETS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,Kd", DENSE)
def test_dense_quantised_output_is_the_quantiser_on_c2(M, N, Kd, act, bias, outset):
    Aq, As, Bq, Bs, b, C, C2, q, s = _dense_case(M, N, Kd, act, bias)
    gq, gs = _guarded(M, N)
    c, c2, cq, cs = ops.dense_gemm_mxfp8_q(Aq, As, Bq, Bs, bias=b, act=act, want_c="c+" in outset, want_c2="c2" in outset,
                                           out_q=gq[:M], out_s=gs[:M])
    assert (c is None) == ("c+" not in outset) and (c2 is None) == ("c2" not in outset)
    if not bias:
        assert bool((s[1] == 0).all()), "no all-zero block in the data: the case does not test its scale byte"
    assert torch.equal(cs, s)
    assert torch.equal(cq, q)
    if c2 is not None:
        assert torch.equal(_bits(c2), _bits(C2))
    if c is not None:
        assert torch.equal(_bits(c), _bits(C))
    _check_guard(gq, gs, M)


@pytest.mark.parametrize("act", ACTS)
def test_nan_and_inf_rows_come_out_as_the_quantiser_encodes_them(act):
    M, N, Kd = 300, 288, 256
    Aq, As, Bq, Bs, b, C, C2, q, s = _dense_case(M, N, Kd, act, True, nonfinite=True)
    assert bool(torch.isnan(C[3].float()).all()), "the NaN row did not reach the output"
    assert not bool(torch.isfinite(C[7].float()).all()), "the Inf row did not reach the output"
    gq, gs = _guarded(M, N)
    c, c2, cq, cs = ops.dense_gemm_mxfp8_q(Aq, As, Bq, Bs, bias=b, act=act, want_c=True, want_c2=True, out_q=gq[:M], out_s=gs[:M])
    assert torch.equal(cs, s) and torch.equal(cq, q)
    assert torch.equal(_bits(c2), _bits(C2)) and torch.equal(_bits(c), _bits(C))
    _check_guard(gq, gs, M)


@functools.lru_cache(maxsize=None)
def _grouped_case(act, bias):
    offs, N, Kd = GROUPED
    E, M = len(offs) - 1, offs[-1]
    g = torch.Generator(device=DEV).manual_seed(M + N + Kd + E)
    A = torch.randn(M, Kd, device=DEV, generator=g).to(torch.bfloat16)
    A[1] = 0
    B = torch.randn(E, N, Kd, device=DEV, generator=g).to(torch.bfloat16)
    b = torch.randn(E, N, device=DEV, generator=g).to(torch.bfloat16) if bias else None
    bp = ops.ptr_table(b, E, N * 2) if bias else None
    offsets = torch.tensor(offs, dtype=torch.int32, device=DEV)
    Aq, As = ops.quantize_mxfp8(A)
    Bq, Bs = ops.quantize_mxfp8(B)
    C, C2 = ops.grouped_gemm_mxfp8(Aq, As, Bq, Bs, offsets, bias_ptrs=bp, epilogue=L.EPI_BIAS_ACT, act=act, want_c2=True)
    q, s = ops.quantize_mxfp8(C2)
    return Aq, As, Bq, Bs, (b, bp), offsets, C, C2, q, s


@pytest.mark.parametrize("outset", OUTSETS)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("act", ACTS)
def test_grouped_quantised_output_is_the_quantiser_on_c2(act, bias, outset):
    Aq, As, Bq, Bs, (b, bp), offsets, C, C2, q, s = _grouped_case(act, bias)
    M, N = C2.shape
    gq, gs = _guarded(M, N)
    c, c2, cq, cs = ops.grouped_gemm_mxfp8_q(Aq, As, Bq, Bs, offsets, bias_ptrs=bp, act=act, want_c="c+" in outset,
                                             want_c2="c2" in outset, out_q=gq[:M], out_s=gs[:M])
    assert torch.equal(cs, s)
    assert torch.equal(cq, q)
    if c2 is not None:
        assert torch.equal(_bits(c2), _bits(C2))
    if c is not None:
        assert torch.equal(_bits(c), _bits(C))
    _check_guard(gq, gs, M)


def test_without_cq_the_new_entry_is_the_old_launch():
    """Cq / Cs left out: csmoe_dense_gemm_mxfp8_q runs gg8f_kernel as csmoe_dense_gemm_mxfp8 does (plain and ACTGRAD here)."""
    M, N, Kd = 300, 288, 256
    Aq, As, Bq, Bs, _, C, C2, _, _ = _dense_case(M, N, Kd, L.ACT_GELU, False)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    call = lambda epi, aux: L.check(L.lib.csmoe_dense_gemm_mxfp8_q(Aq.data_ptr(), Kd, As.data_ptr(), Kd // 32, Bq.data_ptr(), Bs.data_ptr(), Kd,
                                                                    Kd // 32, None, M, N, Kd, out.data_ptr(), None, aux, N, epi, L.ACT_GELU, None,
                                                                    0, None, 0, None), "dense_gemm_mxfp8_q")
    call(L.EPI_PLAIN, None)
    assert torch.equal(_bits(out), _bits(ops.dense_gemm_mxfp8(Aq, As, Bq, Bs)))
    call(L.EPI_ACTGRAD, C.data_ptr())
    assert torch.equal(_bits(out), _bits(ops.dense_gemm_mxfp8(Aq, As, Bq, Bs, epilogue=L.EPI_ACTGRAD, act=L.ACT_GELU, aux=C)))


# ------------------------------------------------------------------------------------------------ affinity epilogues on MXFP8 operands
@pytest.mark.parametrize("T,F,Dout,bias", [(300, 512, 256, True), (64, 256, 264, True), (520, 384, 520, False)])
@pytest.mark.parametrize("rounded", [True, False])
def test_affinity_epilogues_on_mxfp8_match_gemm_then_softplus_mean(T, F, Dout, bias, rounded):
    g = torch.Generator(device=DEV).manual_seed(T + F)
    h = torch.randn(T, F, device=DEV, generator=g).to(torch.bfloat16)
    w2 = (torch.randn(Dout, F, device=DEV, generator=g) * F ** -0.5 * 2).to(torch.bfloat16)
    b2 = (torch.randn(Dout, device=DEV, generator=g) * 0.1).to(torch.bfloat16) if bias else None
    hq, hs = ops.quantize_mxfp8(h)
    wq, ws = ops.quantize_mxfp8(w2)
    y = ops.dense_gemm_mxfp8(hq, hs, wq, ws, bias=b2, epilogue=L.EPI_BIAS if bias else L.EPI_PLAIN)
    adt = torch.bfloat16 if rounded else torch.float32
    ref = ops.softplus_mean(y, adt)
    aff = torch.full((T, 3), -1.0, dtype=adt, device=DEV)
    ops.dense_gemm_affinity_mxfp8(hq, hs, wq, ws, b2, aff[:, 1], rounded=rounded)
    got = aff[:, 1]
    assert bool((aff[:, 0] == -1).all()) and bool((aff[:, 2] == -1).all())       # the neighbouring columns of the table are not touched
    tol = 2.0 ** -7 if rounded else 2e-6
    err = ((got.float() - ref.float()).abs() / ref.float().abs()).max().item()
    print(f"affinity T={T} F={F} Dout={Dout} rounded={rounded}: max relative error {err:.3e} (bound {tol:.3e})")
    assert ((got.float() - ref.float()).abs() <= tol * ref.float().abs()).all()
    if rounded:
        assert (got != ref).float().mean().item() <= 0.01            # a bf16 rounding boundary now and then
    daff = torch.randn(T, device=DEV, generator=g).to(adt)
    ref_dy = ops.softplus_mean_bwd(y, daff)
    dy = ops.dense_gemm_affinity_grad_mxfp8(hq, hs, wq, ws, b2, daff.float().contiguous(), rounded)
    assert torch.equal(dy, ref_dy)
