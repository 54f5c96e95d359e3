"""The contract of csmoe_grouped_gemm_skinny_mxfp8 (csrc/gemm_skinny_mx.hip) on exact data, bit for bit.

Recipe of tests/test_fp8_gpu.py::test_gemm_is_exact_on_exact_data: A integers in [-2, 2] and B integers in [-1, 2] as e4m3, A scales
2^-2 .. 2^2 and B scales 2^-1 .. 2^1 that differ per row and per k-block, bf16 biases that are multiples of 2^-5 in [-2, 2].  A term
is at most 2 * 4 * 2 * 2 = 32 at a granularity of 2^-3, so a sum over Kd = 4096 terms stays below 2^17 and, with the bias, at a
granularity of 2^-5: 22 bits, exact in fp32 in any order, the split over the 8 waves included.  The test asserts that on the CPU for
its own data (ascending, descending and fp64 sums agree) before it trusts it.  Asymmetric operands and per-block scales catch a
swapped operand role, a wrong lane -> k-byte map and a wrong scale byte.

Shapes: expert row counts [0, 1, 16, 17, 3, 0, 33] (an empty expert first and in the middle, one row, exactly one 16-row block, a
block plus one, two blocks plus one); N in {72, 200} without and {96, 224} with the quantised output on the 32-column slab, N in
{3016, 3040} on the 64-column slab (the launch switches slabs at 512 workgroups), none a multiple of its slab; Kd = 128 (one K-step:
seven waves contribute zero tiles), 1152 (nine steps dealt 2, 2, 2, 2, 1, 0, 0, 0) and 4096 (four steps per wave: one unrolled iteration of three steps and a single step on
the narrow slab).  Outputs live inside buffers of M + 16 rows with padded leading dimensions, pre-filled: everything outside
[0, M) x [0, N) must keep its fill.  A has exactly the rows named (out-of-bounds loads are not provoked)."""
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
from tests.golden_util import rel_l2

COUNTS = [0, 1, 16, 17, 3, 0, 33]
E, M = len(COUNTS), sum(COUNTS)
OFF = torch.tensor([0] + list(itertools.accumulate(COUNTS)), dtype=torch.int32)
PLAIN_CASES = [(72, 128), (200, 128), (72, 1152), (200, 1152), (72, 4096), (3016, 128), (3016, 1152)]
QUANT_CASES = [(96, 128), (224, 128), (96, 1152), (224, 1152), (96, 4096), (3040, 128), (3040, 1152)]


def _assert_exact_on_cpu(A, B, bias):
    """fp32 sums over k of dq(A)[m, k] dq(B_e)[n, k] (+ bias) in ascending and in descending order equal the fp64 sum."""
    for e in range(E):
        r0, r1 = int(OFF[e]), int(OFF[e + 1])
        if r1 == r0:
            continue
        for c0 in range(0, B.shape[1], 256):
            a, b = A[r0:r1].float(), B[e, c0:c0 + 256].float()
            prod = a[:, None, :] * b[None, :, :]
            fwd, rev = prod.cumsum(-1)[..., -1], prod.flip(-1).cumsum(-1)[..., -1]
            d = A[r0:r1] @ B[e, c0:c0 + 256].t()
            assert torch.equal(fwd.double(), d) and torch.equal(rev.double(), d)
            pre = fwd + bias[e, c0:c0 + 256].float()
            assert torch.equal(pre.double(), d + bias[e, c0:c0 + 256].double())
            assert float(d.abs().max()) < 2.0 ** 17


@functools.lru_cache(maxsize=None)
def _data(N, Kd):
    """The operands of one case, the fp64 product and its three epilogues (computed once, shared, never modified)."""
    g = torch.Generator().manual_seed(N * 7 + Kd)
    Aq = MX.to_e4m3_bytes(torch.randint(-2, 3, (M, Kd), generator=g).float())
    Bq = MX.to_e4m3_bytes(torch.randint(-1, 3, (E, N, Kd), generator=g).float())
    As = torch.randint(125, 130, (M, Kd // 32), generator=g, dtype=torch.uint8)
    Bs = torch.randint(126, 129, (E, N, Kd // 32), generator=g, dtype=torch.uint8)
    bias = (torch.randint(-64, 65, (E, N), generator=g).float() * 2.0 ** -5).bfloat16()
    _assert_exact_on_cpu(MX.dequantize(Aq, As), MX.dequantize(Bq, Bs), bias)
    prod = MX.grouped_matmul(Aq, As, Bq, Bs, OFF)
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


@pytest.mark.parametrize("N,Kd", PLAIN_CASES + QUANT_CASES)
def test_epilogues_bit_exact_and_nothing_else_written(N, Kd):
    d, ref = _data(N, Kd)
    off = OFF.to(DEV)
    bp = ops.ptr_table(d["bias"], E, N * 2)
    ldc = N + 8
    # PLAIN
    c, cbuf, c0 = _padded(M, N, ldc, torch.bfloat16, -3.0)
    ops.grouped_gemm_skinny_mxfp8(d["Aq"], d["As"], d["Bq"], d["Bs"], off, out=c)
    assert torch.equal(c.cpu(), ref["plain"]), float((c.cpu().float() - ref["plain"].float()).abs().max())
    _assert_outside_untouched(cbuf, c0, M, N)
    # BIAS
    c, cbuf, c0 = _padded(M, N, ldc, torch.bfloat16, -3.0)
    ops.grouped_gemm_skinny_mxfp8(d["Aq"], d["As"], d["Bq"], d["Bs"], off, bias_ptrs=bp, epilogue=L.EPI_BIAS, out=c)
    assert torch.equal(c.cpu(), ref["bias"])
    _assert_outside_untouched(cbuf, c0, M, N)
    # BIAS_ACT (ReLU): the pre-activation and the activated output at the contract's rounding points
    c, cbuf, c0 = _padded(M, N, ldc, torch.bfloat16, -3.0)
    c2, c2buf, c20 = _padded(M, N, ldc, torch.bfloat16, -5.0)
    ops.grouped_gemm_skinny_mxfp8(d["Aq"], d["As"], d["Bq"], d["Bs"], off, bias_ptrs=bp, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU,
                                  out=c, out2=c2)
    assert torch.equal(c.cpu(), ref["bias"]) and torch.equal(c2.cpu(), ref["act"])
    _assert_outside_untouched(cbuf, c0, M, N)
    _assert_outside_untouched(c2buf, c20, M, N)
    # only the activated output
    c2, c2buf, c20 = _padded(M, N, ldc, torch.bfloat16, -5.0)
    ops.grouped_gemm_skinny_mxfp8(d["Aq"], d["As"], d["Bq"], d["Bs"], off, bias_ptrs=bp, epilogue=L.EPI_BIAS_ACT, act=L.ACT_RELU,
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
    ops.grouped_gemm_skinny_mxfp8(d["Aq"], d["As"], d["Bq"], d["Bs"], off, out2=c2, out_q=q, out_s=s, **kw)
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
    r = ops.grouped_gemm_skinny_mxfp8(d["Aq"], d["As"], d["Bq"], d["Bs"], off, out_q=q2, out_s=s2, **kw)
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
    c_g, c2_g = ops.grouped_gemm_skinny_mxfp8(src_q, src_s, d["Bq"], d["Bs"], off, src_rows=perm, src_div=K, **kw)
    c_p, c2_p = ops.grouped_gemm_skinny_mxfp8(src_q[rows].contiguous(), src_s[rows].contiguous(), d["Bq"], d["Bs"], off, **kw)
    assert torch.equal(c_g, c_p) and torch.equal(c2_g, c2_p)
    assert c_g.shape == (M, N) and bool(c_g.float().abs().sum() > 0)


@pytest.mark.parametrize("N,Kd", [(224, 1152), (3040, 128)])
def test_random_data_gelu_and_run_to_run(N, Kd):
    """A ~ N(0, 1), B ~ N(0, 1) / sqrt(Kd), quantised by the library: within 2e-3 relative L2 of the fp64 product of the dequantised
    operands (the bound tests/test_fp8_gpu.py holds the tiled kernel to), and two runs agree bit for bit."""
    g = torch.Generator().manual_seed(N + Kd + 1)
    A = torch.randn(M, Kd, generator=g).bfloat16()
    B = (torch.randn(E, N, Kd, generator=g) / math.sqrt(Kd)).bfloat16()
    bias = (torch.randn(E, N, generator=g) * 0.5).bfloat16()
    Aq, As = ops.quantize_mxfp8(A.to(DEV))
    Bq, Bs = ops.quantize_mxfp8(B.to(DEV))
    emu = MX.grouped_matmul(Aq.cpu(), As.cpu(), Bq.cpu(), Bs.cpu(), OFF)
    for e in range(E):
        emu[int(OFF[e]):int(OFF[e + 1])] += bias[e].double()
    bd = bias.to(DEV)
    kw = dict(bias_ptrs=ops.ptr_table(bd, E, N * 2), epilogue=L.EPI_BIAS_ACT, act=L.ACT_GELU, want_c2=True, want_q=True)
    off = OFF.to(DEV)
    pre, act, q, s = ops.grouped_gemm_skinny_mxfp8(Aq, As, Bq, Bs, off, **kw)
    e_pre = rel_l2(pre.cpu(), emu)
    e_act = rel_l2(act.cpu(), torch.nn.functional.gelu(pre.cpu().double()))
    print(f"N={N} Kd={Kd}: pre rel_l2 {e_pre:.3e}, act rel_l2 {e_act:.3e}")
    assert e_pre <= 2e-3, e_pre
    assert e_act <= 3e-3, e_act
    rq, rs = MX.quantize(act.cpu().float())
    assert torch.equal(q.cpu(), rq) and torch.equal(s.cpu(), rs)
    pre2, act2, q2, s2 = ops.grouped_gemm_skinny_mxfp8(Aq, As, Bq, Bs, off, **kw)
    assert torch.equal(pre2, pre) and torch.equal(act2, act) and torch.equal(q2, q) and torch.equal(s2, s)
