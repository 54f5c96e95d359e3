"""ops.quantize_mxfp4 (csmoe_quantize_mxfp4) byte for byte against tests/mxfp4_ref.py: fp32 and bf16 masters, [E, R, C] with E in
{1, 3}, R in {32, 96}, C in {8, 40} transposed (blocks along R: the layout of the weight tables, C need not be a multiple of anything)
and with R and C swapped for the rows form (blocks along the contiguous dim), the tie / saturation / zero blocks of
tests/test_mxfp4_cpu.py planted in random data, and padded output buffers that keep their fill outside the result."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

if torch.cuda.is_available():
    from competesmoe_amd import ops, _lib as L

from tests import mxfp4_ref as R4

TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def _masters(E, R, C, dtype, seed):
    """[E, R, C] random masters with special blocks ALONG R (dim 1) planted in the first columns: ties at two powers of two, a block
    whose scaled amax lies in (6, 8), an all-zero block, a negative zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(E, R, C, generator=g) * torch.exp(torch.randn(E, 1, C, generator=g) * 2)
    for e in range(E):
        for j, p in enumerate((0, -7)):                          # column j of block 0: amax 4 * 2^p, all seven ties of both signs
            x[e, :32, j] = 0.0
            x[e, 0, j] = 4.0 * 2.0 ** p
            for i, t in enumerate(TIES):
                x[e, 1 + 2 * i, j] = t * 2.0 ** p
                x[e, 2 + 2 * i, j] = -t * 2.0 ** p
        x[e, :32, 2] = torch.linspace(-1, 1, 32) * 5.0
        x[e, 7, 2], x[e, 8, 2] = 7.5, -6.5                       # scaled amax 7.5: both saturate at 6
        x[e, :32, 3] = 0.0                                       # an all-zero block (scale byte 0)
        x[e, 4, 3] = -0.0
        x[e, :32, 4] = 0.0
        x[e, 5, 4] = -0.0                                        # ... and one whose only content is a negative zero
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E,R,C", list(itertools.product((1, 3), (32, 96), (8, 40))))
def test_transposed_tables_byte_for_byte(E, R, C, dtype):
    x = _masters(E, R, C, dtype, 100 * E + R + C)
    rq, rs = R4.quantize(x.float().transpose(1, 2).contiguous())          # [E, C, R/2], [E, C, R/32]
    q, s = ops.quantize_mxfp4(x.to(DEV), transpose=True)
    assert q.shape == (E, C, R // 2) and s.shape == (E, C, R // 32) and q.dtype == torch.uint8 and s.dtype == torch.uint8
    assert torch.equal(s.cpu(), rs)
    assert torch.equal(q.cpu(), rq)
    if E == 1:                                                              # the 2-D form (the shared expert's tables)
        q2, s2 = ops.quantize_mxfp4(x[0].to(DEV), transpose=True)
        assert torch.equal(q2, q[0]) and torch.equal(s2, s[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E,R,C", list(itertools.product((1, 3), (32, 96), (8, 40))))
def test_rows_form_byte_for_byte(E, R, C, dtype):
    x = _masters(E, R, C, dtype, 100 * E + R + C + 1).transpose(1, 2).contiguous()      # [E, C, R]: blocks along the last dim
    rq, rs = R4.quantize(x.float())
    q, s = ops.quantize_mxfp4(x.to(DEV))
    assert q.shape == (E, C, R // 2) and s.shape == (E, C, R // 32)
    assert torch.equal(s.cpu(), rs) and torch.equal(q.cpu(), rq)


def test_planted_blocks_are_what_they_claim():
    """The special blocks reach the kernel as intended: the ties decode to their even neighbours, the (6, 8) block saturates."""
    x = _masters(1, 32, 8, torch.float32, 7)
    q, s = ops.quantize_mxfp4(x.to(DEV), transpose=True)
    d = R4.dequantize(q.cpu(), s.cpu())[0]                                  # [C, R]
    even = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    for j, p in enumerate((0, -7)):
        assert int(s[0, j, 0]) == 127 + p
        for i, v in enumerate(even):
            assert float(d[j, 1 + 2 * i]) == v * 2.0 ** p and float(d[j, 2 + 2 * i]) == -v * 2.0 ** p
    assert float(d[2, 7]) == 6.0 and float(d[2, 8]) == -6.0 and int(s[0, 2, 0]) == 127
    assert int(s[0, 3, 0]) == 0 and int(s[0, 4, 0]) == 0
    assert int(q[0, 3, 2]) == 0x08 and int(q[0, 4, 2]) == 0x80              # the negative zeros keep their sign nibble


@pytest.mark.parametrize("transpose", [False, True])
def test_padded_output_buffers_keep_their_fill(transpose):
    E, R, C = 3, 96, 64
    x = torch.randn(E, R, C, generator=torch.Generator().manual_seed(3)).to(DEV)
    qn = E * R * C // 2
    sn = E * R * C // 32
    qbuf = torch.full((qn + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((sn + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    q_out, s_out = qbuf[128:128 + qn], sbuf[32:32 + sn]
    ptrs = ops.ptr_table(x, E, R * C * 4)
    L.check(L.lib.csmoe_quantize_mxfp4(None, ptrs.data_ptr(), E, C, R, C, L.F32, int(transpose), q_out.data_ptr(), s_out.data_ptr(),
                                       None), "quantize_mxfp4")
    torch.cuda.synchronize()
    q, s = ops.quantize_mxfp4(x, transpose=transpose)
    assert torch.equal(q_out, q.flatten()) and torch.equal(s_out, s.flatten())
    assert bool((qbuf[:128] == 0xA5).all()) and bool((qbuf[128 + qn:] == 0xA5).all())
    assert bool((sbuf[:32] == 0x5A).all()) and bool((sbuf[32 + sn:] == 0x5A).all())
