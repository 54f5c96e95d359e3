"""MXFP4 weights of the W4A8 decode path, the parts that need no GPU: the properties of the reference (tests/mxfp4_ref.py) that the GPU
tests compare the library with, the one fact the layer test rests on, and the host side of csmoe_grouped_gemm_skinny_mxfp4w (shape
query and refusals, decided before any pointer is read or anything is launched; as tests/test_skinny_fp8_cpu.py)."""
import torch

from competesmoe_amd import _lib as L
from oracle import mxfp8 as MX
from tests import mxfp4_ref as R4

OK, INVALID, UNSUPPORTED = 0, 1, 3
POISON = 0xDEAD0000          # a made-up, 16-byte aligned address: a call that read through it would not come back with a refusal
TIES = [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0)]      # (midpoint, the even neighbour)


# ------------------------------------------------------------------------------------------------------------ the reference
def test_pack_unpack_round_trip():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 16, (3, 5, 64), generator=g, dtype=torch.uint8)
    q = R4.pack(codes)
    assert q.shape == (3, 5, 32) and q.dtype == torch.uint8
    assert torch.equal(R4.unpack(q), codes)
    assert int(R4.pack(torch.tensor([0x3, 0xA], dtype=torch.uint8))[0]) == 0xA3       # the even element is the low nibble
    assert torch.equal(R4.from_e2m1_codes(torch.arange(16, dtype=torch.uint8)),
                       torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6]))


def test_ties_round_to_even_at_every_power_of_two():
    for p in (-20, -3, 0, 1, 9):
        for tie, even in TIES:
            for sign in (1.0, -1.0):
                x = torch.zeros(32)
                x[0] = 4.0 * 2.0 ** p                       # amax: shared exponent p, the scaled block has amax 4
                x[5] = sign * tie * 2.0 ** p
                q, s = R4.quantize(x)
                assert int(s[0]) == 127 + p
                d = R4.dequantize(q, s)
                assert float(d[5]) == sign * even * 2.0 ** p, (p, tie, sign, float(d[5]))
                assert float(d[0]) == 4.0 * 2.0 ** p
                # a hair to either side goes to the nearer neighbour
                for eps, want in ((1 + 2.0 ** -20, None), (1 - 2.0 ** -20, None)):
                    x2 = x.clone()
                    x2[5] = sign * tie * eps * 2.0 ** p
                    d2 = float(R4.dequantize(*R4.quantize(x2))[5]) / 2.0 ** p * sign
                    lo = max(v for v in R4.GRID.tolist() if v < tie)
                    hi = min(v for v in R4.GRID.tolist() if v > tie)
                    assert d2 == (hi if eps > 1 else lo)


def test_saturation_when_the_scaled_amax_lies_between_6_and_8():
    for amax in (6.5, 7.0, 7.999):
        x = torch.zeros(2, 32)
        x[0, 3], x[0, 4], x[1, 9] = amax, -amax, -amax * 2.0 ** 5
        q, s = R4.quantize(x)
        assert s.flatten().tolist() == [127, 132]               # floor(log2(amax)) - 2 = 0 and 5
        d = R4.dequantize(q, s)
        assert float(d[0, 3]) == 6.0 and float(d[0, 4]) == -6.0 and float(d[1, 9]) == -6.0 * 32


def test_all_zero_block_and_scale_clamp():
    q, s = R4.quantize(torch.zeros(64))
    assert s.tolist() == [0, 0] and not bool(q.any())
    assert not bool(R4.dequantize(q, s).any())
    x = torch.zeros(32)
    x[1] = 2.0 ** -126                                          # shared exponent -128: below the smallest scale byte
    q, s = R4.quantize(x)
    assert int(s[0]) == 0 and float(R4.dequantize(q, s)[1]) == 2.0 ** -126


def test_round_trip_error_is_at_most_half_a_grid_step():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(64, 256, generator=g) * torch.exp(torch.randn(64, 1, generator=g) * 3)
    q, s = R4.quantize(x)
    d = R4.dequantize(q, s)
    scale = torch.pow(2.0, s.double() - 127).repeat_interleave(32, dim=-1)
    a = (x.double() / scale).abs()                              # the scaled magnitudes, below 8
    assert float(a.max()) < 8.0
    step = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0)).double()
    err = (d - x.double()).abs() / scale
    inside = a <= 6
    assert bool((err[inside] <= step[inside] / 2).all())
    assert bool((d.abs() / scale)[~inside].eq(6).all())         # beyond the grid: saturated
    # the quantisation error the issue quotes for N(0, 1) data: about 11.5 % relative L2
    y = torch.randn(256, 1024, generator=g)
    rel = float((R4.dequantize(*R4.quantize(y)) - y.double()).norm() / y.double().norm())
    assert 0.09 < rel < 0.14, rel


def test_a_dequantised_mxfp4_table_survives_the_mxfp8_quantiser_exactly():
    """The layer test feeds the oracle's MXFP8 FFN the dequantised MXFP4 masters: its own quantiser must give them back unchanged
    (every e2m1 value is an e4m3 value, and the MXFP8 scale of such a block never loses a bit of it)."""
    g = torch.Generator().manual_seed(2)
    for scale in (1e-20, 1e-3, 1.0, 37.0, 1e20):
        w = torch.randn(8, 96, 128, generator=g) * scale                       # fp32 masters
        d = R4.dequantize(*R4.quantize(w))
        assert torch.equal(d.float().double(), d)                                # representable in fp32
        assert torch.equal(MX.dequantize(*MX.quantize(d.float())), d)
    wb = (torch.randn(8, 96, 128, generator=g) * 0.05).bfloat16()               # bf16 masters
    d = R4.dequantize(*R4.quantize(wb))
    assert torch.equal(MX.dequantize(*MX.quantize(d.float())), d)
    # and as_mxfp8 is the same table
    q, s = R4.quantize(wb)
    assert torch.equal(MX.dequantize(*R4.as_mxfp8(q, s)), d)


# ------------------------------------------------------------------------------------------------------------ the host side
def _ok(M=70, N=72, Kd=128, lda=None, ldas=None, ldb=None, ldbs=None, ldc=None, ldcq=None, ldcs=None, epi=L.EPI_PLAIN, quant=0):
    d = lambda v, dflt: dflt if v is None else v
    return L.lib.csmoe_grouped_gemm_skinny_mxfp4w_ok(M, N, Kd, d(lda, Kd), d(ldas, Kd // 32), d(ldb, Kd // 2), d(ldbs, Kd // 32),
                                                     d(ldc, N), d(ldcq, N), d(ldcs, N // 32), epi, quant)


def test_shape_query_both_sides_of_every_rule():
    assert _ok(Kd=128) == 1 and _ok(Kd=96) == 0 and _ok(Kd=1152) == 1 and _ok(Kd=1152 + 32) == 0
    assert _ok(N=8) == 1 and _ok(N=12) == 0
    act = dict(epi=L.EPI_BIAS_ACT, quant=1)
    assert _ok(N=32, **act) == 1 and _ok(N=40, **act) == 0
    assert _ok(N=40, epi=L.EPI_BIAS_ACT) == 1                   # ... which is fine without the quantised output
    # leading dimensions: lda / ldb (bytes of the packed row) multiples of 16, ldas / ldbs of 4, ldc of 8; ldcq of 8 with the output
    assert _ok(lda=128 + 16) == 1 and _ok(lda=128 + 8) == 0
    assert _ok(ldb=64) == 1 and _ok(ldb=64 + 16) == 1 and _ok(ldb=64 + 8) == 0
    assert _ok(ldb=48) == 0                                     # shorter than a packed row
    assert _ok(ldas=8) == 1 and _ok(ldas=6) == 0
    assert _ok(ldbs=8) == 1 and _ok(ldbs=6) == 0
    assert _ok(ldc=80) == 1 and _ok(ldc=76) == 0
    assert _ok(N=96, ldcq=104, ldcs=5, **act) == 1 and _ok(N=96, ldcq=100, **act) == 0 and _ok(N=96, ldcs=2, **act) == 0
    assert _ok(N=96, ldcq=100, ldcs=2, epi=L.EPI_BIAS_ACT) == 1     # not looked at without the quantised output
    assert _ok(lda=64) == 0 and _ok(ldc=64) == 0                    # shorter than a row
    # the 2 GiB panel rule: M * lda and N * ldb bytes (a packed row is Kd / 2 bytes: twice the rows of the fp8 kernel)
    assert _ok(M=1 << 18, Kd=4096) == 1 and _ok(M=1 << 19, Kd=4096) == 0
    assert _ok(N=(1 << 19) - 8, Kd=8192) == 1 and _ok(N=1 << 19, Kd=8192) == 0
    # epilogues: the forward ones of the fp8 layer; the quantised output goes with BIAS_ACT
    for epi in (L.EPI_PLAIN, L.EPI_BIAS, L.EPI_BIAS_ACT):
        assert _ok(epi=epi) == 1
    for epi in (L.EPI_ACTGRAD, L.EPI_ROUND_BIAS32_ACT, L.EPI_SOFTPLUS_ROWSUM, L.EPI_ACTGRAD_ROWSCALE, L.EPI_ACCUM):
        assert _ok(epi=epi) == 0
    assert _ok(N=96, epi=L.EPI_BIAS, quant=1) == 0 and _ok(N=96, epi=L.EPI_PLAIN, quant=1) == 0


def _entry(M=70, N=72, Kd=128, lda=None, ldas=None, ldb=None, epi=L.EPI_PLAIN, ptr=POISON, tables=POISON, src_rows=None, src_div=1,
           cq=None, cs=None, scales=None):
    d = lambda v, dflt: dflt if v is None else v
    return L.lib.csmoe_grouped_gemm_skinny_mxfp4w(ptr, d(lda, Kd), ptr if scales is None else scales, d(ldas, Kd // 32), src_rows,
                                                  src_div, tables, tables, d(ldb, Kd // 2), Kd // 32, None, tables, 7, M, N, Kd, ptr,
                                                  None, N, cq, cs, N, N // 32, epi, 0, None)


def test_refused_before_any_pointer_is_read():
    """Every operand is a poisoned address: a refusal is the only way back."""
    assert _entry(Kd=96) == UNSUPPORTED
    assert b"skinny_mxfp4w" in L.lib.csmoe_last_error()
    assert _entry(N=12) == UNSUPPORTED
    assert _entry(N=40, epi=L.EPI_BIAS_ACT, cq=POISON, cs=POISON) == UNSUPPORTED
    assert _entry(lda=128 + 8) == UNSUPPORTED
    assert _entry(ldb=64 + 8) == UNSUPPORTED
    assert _entry(ldas=6) == UNSUPPORTED
    assert _entry(M=1 << 19, Kd=4096) == UNSUPPORTED
    assert _entry(ptr=POISON + 8) == UNSUPPORTED                # operands not 16-byte aligned
    assert _entry(scales=POISON + 2) == UNSUPPORTED             # As not 4-byte aligned (scale bytes are read a word at a time)
    assert _entry(epi=L.EPI_ACTGRAD) == UNSUPPORTED
    assert b"forward epilogues" in L.lib.csmoe_last_error()
    assert _entry(epi=L.EPI_ACCUM) == UNSUPPORTED
    assert b"ACCUM" in L.lib.csmoe_last_error()


def test_invalid_arguments():
    assert _entry(tables=None) == INVALID                       # null pointer tables / offsets
    assert b"null" in L.lib.csmoe_last_error()
    assert _entry(ptr=None) == INVALID                          # null operands
    assert _entry(ldb=32) == INVALID                            # shorter than a packed row
    assert _entry(src_rows=POISON, src_div=0) == INVALID
    assert _entry(src_rows=POISON, src_div=-2) == INVALID
    assert b"src_div" in L.lib.csmoe_last_error()
    assert _entry(N=96, epi=L.EPI_BIAS, cq=POISON, cs=POISON) == INVALID        # the quantised output goes with BIAS_ACT
    assert _entry(N=96, epi=L.EPI_BIAS_ACT, cq=POISON) == INVALID               # Cq without Cs


def test_no_rows_is_ok():
    assert _entry(M=0) == OK
    assert _entry(M=0, ptr=None) == OK


def test_quantiser_refusals_come_before_any_pointer_is_read():
    q4 = L.lib.csmoe_quantize_mxfp4
    assert q4(POISON, None, 1, 40, 32, 40, L.F32, 0, POISON, POISON, None) == UNSUPPORTED      # C % 32 != 0
    assert b"quantize_mxfp4" in L.lib.csmoe_last_error()
    assert q4(POISON, None, 1, 64, 48, 64, L.F32, 1, POISON, POISON, None) == UNSUPPORTED      # transposed: R % 32 != 0
    assert q4(POISON, None, 1, 64, 32, 64, L.F32, 0, POISON + 8, POISON, None) == UNSUPPORTED  # q not 16-byte aligned
    assert q4(POISON, None, 1, 64, 32, 64, L.F32, 0, None, POISON, None) == INVALID
    assert q4(None, None, 1, 64, 32, 64, L.F32, 0, POISON, POISON, None) == INVALID
    assert q4(None, None, 1, 64, 0, 64, L.F32, 0, None, None, None) == OK                      # no rows
