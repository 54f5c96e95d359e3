"""Host side of the decode path (no GPU): the shape query and the refusals of csmoe_grouped_gemm_skinny, which are decided before
any pointer is read or anything is launched, and the decode_rows switch."""
import pytest

import competesmoe_amd
from competesmoe_amd import _lib as L

INVALID, UNSUPPORTED = 1, 3
EPI_SOFTPLUS_ROWSUM = L.EPI_SOFTPLUS_ROWSUM


def _ok(M, N, Kd, layout, lda=None, ldb=None, ldc=None, epi=L.EPI_PLAIN, dt=L.BF16):
    lda = Kd if lda is None else lda
    ldb = (Kd if layout == L.B_NK else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    return L.lib.csmoe_grouped_gemm_skinny_ok(M, N, Kd, lda, ldb, ldc, layout, epi, dt)


@pytest.mark.parametrize("layout", [L.B_NK, L.B_KN])
def test_shape_query(layout):
    assert _ok(70, 72, 40, layout) == 1                     # N no multiple of 16, Kd no multiple of 32
    assert _ok(70, 68, 40, layout) == 0                     # N not a multiple of 8
    assert _ok(70, 72, 44, layout) == 0                     # Kd not a multiple of 8
    assert _ok(70, 72, 40, layout, lda=44) == 0             # lda = Kd + 4: rows not 16-byte aligned
    assert _ok(70, 72, 40, layout, dt=L.F32) == 0
    for epi in (L.EPI_ACTGRAD, L.EPI_ACCUM, EPI_SOFTPLUS_ROWSUM, L.EPI_ACTGRAD_ROWSCALE):
        assert _ok(70, 72, 40, layout, epi=epi) == 0
    for epi in (L.EPI_PLAIN, L.EPI_BIAS, L.EPI_BIAS_ACT, L.EPI_ROUND_BIAS32_ACT):
        assert _ok(70, 72, 40, layout, epi=epi) == 1


def _entry(layout=L.B_NK, epi=L.EPI_PLAIN, dt=L.BF16, src_rows=None, src_div=1, N=72, Kd=40):
    """The entry with null operand pointers: a return value other than a refusal would mean a pointer had been read."""
    return L.lib.csmoe_grouped_gemm_skinny(None, Kd, src_rows, src_div, None, layout, Kd if layout == L.B_NK else N, None, None, 7, 70,
                                           N, Kd, None, None, N, epi, 0, dt, None)


@pytest.mark.parametrize("layout", [L.B_NK, L.B_KN])
def test_refused_before_any_pointer_is_read(layout):
    assert _entry(layout, dt=L.F32) == UNSUPPORTED
    assert b"bf16" in L.lib.csmoe_last_error()
    assert _entry(layout, epi=L.EPI_ACTGRAD) == UNSUPPORTED
    assert _entry(layout, epi=L.EPI_ACCUM) == UNSUPPORTED
    assert b"ACCUM" in L.lib.csmoe_last_error()
    assert _entry(layout, epi=EPI_SOFTPLUS_ROWSUM) == UNSUPPORTED
    assert b"forward epilogues" in L.lib.csmoe_last_error()


def test_invalid_arguments():
    assert _entry(layout=2) == INVALID
    assert b"layout" in L.lib.csmoe_last_error()
    # src_rows given (a made-up address: nothing reads it) with src_div <= 0
    assert _entry(src_rows=4096, src_div=0) == INVALID
    assert _entry(src_rows=4096, src_div=-2) == INVALID
    assert b"src_div" in L.lib.csmoe_last_error()
    assert _entry() == INVALID                              # valid request, null pointer tables


def test_decode_rows_switch():
    assert competesmoe_amd.decode_rows() == 0               # the default (CSMOE_DECODE_ROWS unset): off
    try:
        assert competesmoe_amd.decode_rows(32) == 32
        assert competesmoe_amd.decode_rows() == 32
        assert competesmoe_amd.decode_rows(0) == 0
        assert competesmoe_amd.decode_rows() == 0
        with pytest.raises(ValueError):
            competesmoe_amd.decode_rows(-1)
    finally:
        competesmoe_amd.decode_rows(0)
