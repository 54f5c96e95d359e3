"""Host side of the fp8 decode kernel (no GPU): the shape query and the refusals of csmoe_grouped_gemm_skinny_mxfp8, which are decided
before any pointer is read or anything is launched."""
from competesmoe_amd import _lib as L

OK, INVALID, UNSUPPORTED = 0, 1, 3
POISON = 0xDEAD0000          # a made-up, 16-byte aligned address: a call that read through it would not come back with a refusal


def _ok(M=70, N=72, Kd=128, lda=None, ldas=None, ldb=None, ldbs=None, ldc=None, ldcq=None, ldcs=None, epi=L.EPI_PLAIN, quant=0):
    d = lambda v, dflt: dflt if v is None else v
    return L.lib.csmoe_grouped_gemm_skinny_mxfp8_ok(M, N, Kd, d(lda, Kd), d(ldas, Kd // 32), d(ldb, Kd), d(ldbs, Kd // 32), d(ldc, N),
                                                    d(ldcq, N), d(ldcs, N // 32), epi, quant)


def test_shape_query_both_sides_of_every_rule():
    assert _ok(Kd=128) == 1 and _ok(Kd=96) == 0 and _ok(Kd=1152) == 1 and _ok(Kd=1152 + 32) == 0
    assert _ok(N=8) == 1 and _ok(N=12) == 0
    act = dict(epi=L.EPI_BIAS_ACT, quant=1)
    assert _ok(N=32, **act) == 1 and _ok(N=40, **act) == 0
    assert _ok(N=40, epi=L.EPI_BIAS_ACT) == 1                   # ... which is fine without the quantised output
    # leading dimensions: lda / ldb multiples of 16, ldas / ldbs of 4, ldc of 8; ldcq of 8 with the quantised output
    assert _ok(lda=128 + 16) == 1 and _ok(lda=128 + 8) == 0
    assert _ok(ldb=128 + 16) == 1 and _ok(ldb=128 + 8) == 0
    assert _ok(ldas=8) == 1 and _ok(ldas=6) == 0
    assert _ok(ldbs=8) == 1 and _ok(ldbs=6) == 0
    assert _ok(ldc=80) == 1 and _ok(ldc=76) == 0
    assert _ok(N=96, ldcq=104, ldcs=5, **act) == 1 and _ok(N=96, ldcq=100, **act) == 0 and _ok(N=96, ldcs=2, **act) == 0
    assert _ok(N=96, ldcq=100, ldcs=2, epi=L.EPI_BIAS_ACT) == 1     # not looked at without the quantised output
    assert _ok(lda=64) == 0 and _ok(ldc=64) == 0                    # shorter than a row
    # the 2 GiB panel rule: M * lda and N * ldb bytes
    assert _ok(M=1 << 18, Kd=4096) == 1 and _ok(M=1 << 19, Kd=4096) == 0
    assert _ok(N=(1 << 18) - 8, Kd=8192) == 1 and _ok(N=1 << 18, Kd=8192) == 0
    # epilogues: the forward ones of the fp8 layer; the quantised output goes with BIAS_ACT
    for epi in (L.EPI_PLAIN, L.EPI_BIAS, L.EPI_BIAS_ACT):
        assert _ok(epi=epi) == 1
    for epi in (L.EPI_ACTGRAD, L.EPI_ROUND_BIAS32_ACT, L.EPI_SOFTPLUS_ROWSUM, L.EPI_ACTGRAD_ROWSCALE, L.EPI_ACCUM):
        assert _ok(epi=epi) == 0
    assert _ok(N=96, epi=L.EPI_BIAS, quant=1) == 0 and _ok(N=96, epi=L.EPI_PLAIN, quant=1) == 0


def _entry(M=70, N=72, Kd=128, lda=None, ldas=None, epi=L.EPI_PLAIN, ptr=POISON, tables=POISON, src_rows=None, src_div=1, cq=None,
           cs=None, scales=None):
    d = lambda v, dflt: dflt if v is None else v
    return L.lib.csmoe_grouped_gemm_skinny_mxfp8(ptr, d(lda, Kd), ptr if scales is None else scales, d(ldas, Kd // 32), src_rows, src_div, tables, tables, Kd, Kd // 32,
                                                 None, tables, 7, M, N, Kd, ptr, None, N, cq, cs, N, N // 32, epi, 0, None)


def test_refused_before_any_pointer_is_read():
    """Every operand is a poisoned address: a refusal is the only way back."""
    assert _entry(Kd=96) == UNSUPPORTED
    assert b"skinny_mxfp8" in L.lib.csmoe_last_error()
    assert _entry(N=12) == UNSUPPORTED
    assert _entry(N=40, epi=L.EPI_BIAS_ACT, cq=POISON, cs=POISON) == UNSUPPORTED
    assert _entry(lda=128 + 8) == UNSUPPORTED
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
    assert _entry(src_rows=POISON, src_div=0) == INVALID
    assert _entry(src_rows=POISON, src_div=-2) == INVALID
    assert b"src_div" in L.lib.csmoe_last_error()
    assert _entry(N=96, epi=L.EPI_BIAS, cq=POISON, cs=POISON) == INVALID        # the quantised output goes with BIAS_ACT
    assert _entry(N=96, epi=L.EPI_BIAS_ACT, cq=POISON) == INVALID               # Cq without Cs


def test_no_rows_is_ok():
    assert _entry(M=0) == OK
    assert _entry(M=0, ptr=None) == OK
