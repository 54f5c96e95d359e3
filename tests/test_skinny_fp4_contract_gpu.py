"""The contract of csmoe_grouped_gemm_skinny_mxfp4w (csrc/gemm_skinny_mx.hip) on exact data, bit for bit: the recipe of
tests/test_skinny_fp8_contract_gpu.py with MXFP4 weights.

A integers in [-2, 2] as e4m3 with scales 2^-2 .. 2^2, B drawn from {-1, 0, 1, 2} as e2m1 (packed two per byte) with scales
2^-1 .. 2^1, both different per row and per k-block, bf16 biases that are multiples of 2^-5 in [-2, 2].  A term is at most
2 * 4 * 2 * 2 = 32 at a granularity of 2^-3, so a sum over Kd <= 5120 terms stays below 2^18 and, with the bias, at a granularity of
2^-5: 23 bits, exact in fp32 in any order, the split over the 8 waves included.  The test asserts that on the CPU for its own data
(fp32 sums in ascending and in descending k order equal the fp64 sum) before it trusts it.  Random asymmetric data per k catches a
wrong nibble order, a wrong lane -> k map, a swapped operand role and a wrong scale byte.

Shapes: expert row counts [0, 1, 16, 17, 3, 0, 33], i.e. 11 row blocks at most, so the launch takes the 64-column slab from
ceil(N / 64) >= 24 on (256 workgroups: gemm_skinny_mx.hip's slab rule).  N in {72, 200, 1464} without and {96, 224, 1440} with the
quantised output on the 32-column slab (1464 and 1440: 23 slabs of 64, the last N before the switch), N = 1480 without and 1504
with it on the 64-column slab (24 slabs, the first after it); none is a multiple of 64, and 72 / 200 / 1464 none of 32.  Kd = 128
(one K-step: seven waves contribute zero tiles), 1152 (nine steps dealt 2, 2, 2, 2, 1, 0, 0, 0: no unrolled iteration on either
slab), 4096 on the narrow slab (four steps per wave = its unroll depth 4), 5120 on the narrow slab (five: one unrolled iteration
and a single step) and 3072 on the wide slab (three steps per wave = its unroll depth 3).  Outputs live inside buffers of M + 16
rows with padded leading dimensions, pre-filled: everything outside [0, M) x [0, N) must keep its fill.  A has exactly the rows named
(out-of-range loads are not provoked)."""
import functools
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

if torch.cuda.is_available():
    from competesmoe_amd import ops, _lib as L

from oracle import mxfp8 as MX
from tests import mxfp4_ref as R4
from tests.golden_util import rel_l2

COUNTS = [0, 1, 16, 17, 3, 0, 33]
E, M = len(COUNTS), sum(COUNTS)
OFF = torch.tensor([0] + list(itertools.accumulate(COUNTS)), dtype=torch.int32)
PLAIN_CASES = [(72, 128), (200, 128), (72, 1152), (200, 1152), (72, 4096), (72, 5120), (1464, 128), (1480, 128), (1480, 1152),
               (1480, 3072)]
QUANT_CASES = [(96, 128), (224, 128), (96, 1152), (224, 1152), (96, 4096), (1440, 128), (1504, 128), (1504, 1152)]


def _assert_exact_on_cpu(A, B, bias):
    """fp32 sums over k of dq(A)[m, k] dq(B_e)[n, k] (+ bias), accumulated one k at a time in ascending and in descending order,
    equal the fp64 sum."""
    for e in range(E):
        r0, r1 = int(OFF[e]), int(OFF[e + 1])
        if r1 == r0:
            continue
        a, b = A[r0:r1].float().t().contiguous(), B[e].float().t().contiguous()          # [Kd, rows], [Kd, N]
        fwd = torch.zeros(r1 - r0, B.shape[1])
        rev = torch.zeros(r1 - r0, B.shape[1])
        for k in range(a.shape[0]):
            fwd.addcmul_(a[k][:, None], b[k][None, :])
            rev.addcmul_(a[-1 - k][:, None], b[-1 - k][None, :])
        d = A[r0:r1] @ B[e].t()
        assert torch.equal(fwd.double(), d) and torch.equal(rev.double(), d)
        pre = fwd + bias[e].float()
        assert torch.equal(pre.double(), d + bias[e].double())
        assert float(d.abs().max()) < 2.0 ** 18


@functools.lru_cache(maxsize=None)
def _data(N, Kd):
    """The operands of one case, the fp64 product and its three epilogues (computed once, shared, never modified)."""
    g = torch.Generator().manual_seed(N * 7 + Kd)
    Aq = MX.to_e4m3_bytes(torch.randint(-2, 3, (M, Kd), generator=g).float())
    Bq = R4.pack(R4.to_e2m1_codes(torch.randint(-1, 3, (E, N, Kd), generator=g).float()))
    As = torch.randint(125, 130, (M, Kd // 32), generator=g, dtype=torch.uint8)
    Bs = torch.randint(126, 129, (E, N, Kd // 32), generator=g, dtype=torch.uint8)
    bias = (torch.randint(-64, 65, (E, N), generator=g).float() * 2.0 ** -5).bfloat16()
    B8 = R4.as_mxfp8(Bq, Bs)[0]
    assert torch.equal(MX.dequantize(B8, Bs), R4.dequantize(Bq, Bs))
    _assert_exact_on_cpu(MX.dequantize(Aq, As), R4.dequantize(Bq, Bs), bias)
    prod = MX.grouped_matmul(Aq, As, B8, Bs, OFF)
    with_bias = prod.clone()
    for e in range(E):
        with_bias[int(OFF[e]):int(OFF[e + 1])] += bias[e].double()
    ref = {"plain": prod.float().bfloat16(), "bias": with_bias.float().bfloat16()}
    ref["act"] = torch.relu(ref["bias"].float()).bfloat16()
    dev = {k: v.to(DEV) for k, v in dict(Aq=Aq, As=As, Bq=Bq, Bs=Bs, bias=bias).items()}
    return dev, ref


def _padded(rows, cols, ld, dtype, fill):
    """A [rows, cols] view at the top left of a pre-filled [rows + 16, ld] buffer; (view, buffer, copy of the untouched buffer)."""
    buf = torch.full((rows + 16, ld), fill, dtype=dtype, device=DEV)
    return buf[:rows, :cols], buf, buf.clone()


def _assert_outside_untouched(buf, before, rows, cols):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:rows, :cols] = False
    assert torch.equal(buf[mask], before[mask]), "written outside [0, M) x [0, N)"


def test_the_cases_lie_on_both_sides_of_the_slab_switch():
    nrb = min(M, M // 16 + E)                                    # the host's bound of the number of 16-row blocks
    wide = lambda N: nrb * ((N + 63) // 64) >= 256
    assert nrb == 11
    assert not wide(1464) and wide(1480) and not wide(1440) and wide(1504) and not wide(224)
    assert all(N % 64 for N, _ in PLAIN_CASES + QUANT_CASES) and all(N % 32 for N, _ in PLAIN_CASES)


@pytest.mark.parametrize("N,Kd", PLAIN_CASES + QUANT_CASES)
def test_epilogues_bit_exact_and_nothing_else_written(N, Kd):
    d, ref = _data(N, Kd)
    off = OFF.to(DEV)
    bp = ops.ptr_table(d["bias"], E, N * 2)
    ldc = N + 8
    # PLAIN
    c, cbuf, c0 = _padded(M, N, ldc, torch.bfloat16, -3.0)
    ops.grouped_gemm_skinny_mxfp4w(d["Aq"], d["As"], d["Bq"], d["Bs"], off, out=c)
    assert torch.equal(c.cpu(), ref["plain"]), float((c.cpu().float() - ref["plain"].float()).abs().max())
    _assert_outside_untouched(cbuf, c0, M, N)
    # BIAS
    c, cbuf, c0 = _padded(M, N, ldc, torch.bfloat16, -3.0)
    ops.grouped_gemm_skinny_mxfp4w(d["Aq"], d["As"], d["Bq"], d["Bs"], off, bias_ptrs=bp, epilogue=L.EPI_BIAS, out=c)
    assert torch.equal(c.cpu(), ref["bias"])
    _assert_outside_untouched(cbuf, c0, M, N)
    # BIAS_ACT (ReLU): the pre-activation and the activated output at the contract's rounding points
    c, cbuf, c0 = _padded(M, N, ldc, torch.bfloat16, -3.0)
    c2, c2buf, c20 = _padded(M, N, ldc, torch.bfloat16, -5.0)
    ops.grouped_gemm_skinny_mxfp4w(d["Aq"], d["As"], d["Bq"], d["Bs"], off, bias_ptrs=bp, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU,
                                   out=c, out2=c2)
    assert torch.equal(c.cpu(), ref["bias"]) and torch.equal(c2.cpu(), ref["act"])
    _assert_outside_untouched(cbuf, c0, M, N)
    _assert_outside_untouched(c2buf, c20, M, N)
    # only the activated output
    c2, c2buf, c20 = _padded(M, N, ldc, torch.bfloat16, -5.0)
    ops.grouped_gemm_skinny_mxfp4w(d["Aq"], d["As"], d["Bq"], d["Bs"], off, bias_ptrs=bp, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU,
                                   want_c=False, out2=c2)
    assert torch.equal(c2.cpu(), ref["act"])
    _assert_outside_untouched(c2buf, c20, M, N)


@pytest.mark.parametrize("N,Kd", QUANT_CASES)
def test_fused_quantised_output(N, Kd):
    d, ref = _data(N, Kd)
    off = OFF.to(DEV)
    bp = ops.ptr_table(d["bias"], E, N * 2)
    kw = dict(bias_ptrs=bp, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU, want_c=False)
    c2, c2buf, c20 = _padded(M, N, N + 8, torch.bfloat16, -5.0)
    q, qbuf, q0 = _padded(M, N, N + 24, torch.uint8, 0xA5)
    s, sbuf, s0 = _padded(M, N // 32, N // 32 + 3, torch.uint8, 0x5A)
    ops.grouped_gemm_skinny_mxfp4w(d["Aq"], d["As"], d["Bq"], d["Bs"], off, out2=c2, out_q=q, out_s=s, **kw)
    assert torch.equal(c2.cpu(), ref["act"])
    rq, rs = MX.quantize(c2.cpu().float())                      # of the kernel's own C2
    assert torch.equal(s.cpu(), rs) and torch.equal(q.cpu(), rq)
    for buf, before, cols in ((c2buf, c20, N), (qbuf, q0, N), (sbuf, s0, N // 32)):
        _assert_outside_untouched(buf, before, M, cols)
    # ... and byte for byte what the quantiser writes for that C2
    q_ref, s_ref = ops.quantize_mxfp8(c2.contiguous())
    assert torch.equal(q, q_ref) and torch.equal(s, s_ref)
    # without C2 (what the layer does): Cq / Cs unchanged
    q2, q2buf, q20 = _padded(M, N, N + 24, torch.uint8, 0xA5)
    s2, s2buf, s20 = _padded(M, N // 32, N // 32 + 3, torch.uint8, 0x5A)
    r = ops.grouped_gemm_skinny_mxfp4w(d["Aq"], d["As"], d["Bq"], d["Bs"], off, out_q=q2, out_s=s2, **kw)
    assert r[0] is None and r[1] is None
    assert torch.equal(q2, q) and torch.equal(s2, s)
    _assert_outside_untouched(q2buf, q20, M, N)
    _assert_outside_untouched(s2buf, s20, M, N // 32)


@pytest.mark.parametrize("N,Kd", [(72, 128), (224, 1152)])
def test_gather_equals_pregathered_rows(N, Kd):
    """src_rows / src_div = 2 over a T-row source (elements and scale rows) against the same product on the gathered rows."""
    d, _ = _data(N, Kd)
    T, K = 40, 2
    g = torch.Generator().manual_seed(N + Kd)
    src_q = MX.to_e4m3_bytes(torch.randint(-2, 3, (T, Kd), generator=g).float()).to(DEV)
    src_s = torch.randint(125, 130, (T, Kd // 32), generator=g, dtype=torch.uint8).to(DEV)
    perm = torch.randint(0, T * K, (M,), generator=g, dtype=torch.int32).to(DEV)
    rows = (perm // K).long()
    off = OFF.to(DEV)
    bp = ops.ptr_table(d["bias"], E, N * 2)
    kw = dict(bias_ptrs=bp, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU, want_c2=True)
    c_g, c2_g = ops.grouped_gemm_skinny_mxfp4w(src_q, src_s, d["Bq"], d["Bs"], off, src_rows=perm, src_div=K, **kw)
    c_p, c2_p = ops.grouped_gemm_skinny_mxfp4w(src_q[rows].contiguous(), src_s[rows].contiguous(), d["Bq"], d["Bs"], off, **kw)
    assert torch.equal(c_g, c_p) and torch.equal(c2_g, c2_p)
    assert c_g.shape == (M, N) and bool(c_g.float().abs().sum() > 0)


@pytest.mark.parametrize("N,Kd", [(224, 1152), (1504, 128)])
def test_random_data_gelu_and_run_to_run(N, Kd):
    """A ~ N(0, 1), B ~ N(0, 1) / sqrt(Kd), quantised by the library (A to MXFP8, B to MXFP4): within 2e-3 / 3e-3 relative L2 of the
    fp64 product of the dequantised operands (the bounds the fp8 kernel is held to), and two runs agree bit for bit."""
    g = torch.Generator().manual_seed(N + Kd + 1)
    A = torch.randn(M, Kd, generator=g).bfloat16()
    B = (torch.randn(E, N, Kd, generator=g) / math.sqrt(Kd)).bfloat16()
    bias = (torch.randn(E, N, generator=g) * 0.5).bfloat16()
    Aq, As = ops.quantize_mxfp8(A.to(DEV))
    Bq, Bs = ops.quantize_mxfp4(B.to(DEV))
    rq, rs = R4.quantize(B.float())
    assert torch.equal(Bq.cpu(), rq) and torch.equal(Bs.cpu(), rs)
    emu = MX.grouped_matmul(Aq.cpu(), As.cpu(), R4.as_mxfp8(rq, rs)[0], rs, OFF)
    for e in range(E):
        emu[int(OFF[e]):int(OFF[e + 1])] += bias[e].double()
    bd = bias.to(DEV)
    kw = dict(bias_ptrs=ops.ptr_table(bd, E, N * 2), epilogue=L.EPI_BIAS_ACT, act=L.ACT_GELU, want_c2=True, want_q=True)
    off = OFF.to(DEV)
    pre, act, q, s = ops.grouped_gemm_skinny_mxfp4w(Aq, As, Bq, Bs, off, **kw)
    e_pre = rel_l2(pre.cpu(), emu)
    e_act = rel_l2(act.cpu(), torch.nn.functional.gelu(pre.cpu().double()))
    print(f"N={N} Kd={Kd}: pre rel_l2 {e_pre:.3e}, act rel_l2 {e_act:.3e}")
    assert e_pre <= 2e-3, e_pre
    assert e_act <= 3e-3, e_act
    rq, rs = MX.quantize(act.cpu().float())
    assert torch.equal(q.cpu(), rq) and torch.equal(s.cpu(), rs)
    pre2, act2, q2, s2 = ops.grouped_gemm_skinny_mxfp4w(Aq, As, Bq, Bs, off, **kw)
    assert torch.equal(pre2, pre) and torch.equal(act2, act) and torch.equal(q2, q) and torch.equal(s2, s)
