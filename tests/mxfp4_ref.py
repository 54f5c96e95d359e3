"""CPU reference for the MXFP4 weight tables of the W4A8 decode path -- test infrastructure, plain torch.

OCP Microscaling v1.0: blocks of 32 consecutive elements along the last dim share one e8m0 scale byte s worth 2^(s - 127); elements
are e2m1 (sign and magnitude, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6); shared exponent = floor(log2(amax)) - 2 (emax of e2m1), the
byte clamped to [0, 254]; an element is round-to-nearest-even of x * 2^-shared on the e2m1 grid, saturated at +-6.  A packed row of
C elements is C / 2 bytes in natural order: byte j holds element 2 j in its low nibble and element 2 j + 1 in its high nibble.

Written independently of csrc/mx_quant.h (which compares against the seven midpoints): here the grid is three uniform pieces, each
rounded by torch.round (half to even): steps of 0.5 below 2, of 1 below 4, of 2 above."""
import torch

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def to_e2m1_codes(v: torch.Tensor) -> torch.Tensor:
    """float -> e2m1 codes (uint8, 0..15: bit 3 the sign), round to nearest even, saturating at +-6."""
    a = v.abs().double()
    r = torch.where(a < 2.0, torch.round(a * 2.0) / 2.0, torch.where(a < 4.0, torch.round(a), torch.round(a / 2.0) * 2.0))
    r = r.clamp(max=6.0)
    code = torch.bucketize(r, GRID.double())                     # r is a grid value: its index
    assert torch.equal(GRID.double()[code], r)
    return (code + 8 * torch.signbit(v).long()).to(torch.uint8)


def from_e2m1_codes(c: torch.Tensor) -> torch.Tensor:
    mag = GRID[(c & 7).long()]
    return torch.where((c & 8) != 0, -mag, mag)


def pack(codes: torch.Tensor) -> torch.Tensor:
    """codes [..., C] (0..15) -> bytes [..., C / 2]: element 2 j in the low nibble of byte j."""
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).to(torch.uint8)


def unpack(q: torch.Tensor) -> torch.Tensor:
    return torch.stack((q & 15, q >> 4), dim=-1).reshape(*q.shape[:-1], q.shape[-1] * 2)


def quantize(x: torch.Tensor):
    """x [..., C] (C % 32 == 0) -> (q uint8 [..., C / 2] packed, s uint8 [..., C / 32]), blocks along the last dim."""
    shp = x.shape
    xb = x.float().reshape(*shp[:-1], shp[-1] // 32, 32)
    amax = xb.abs().amax(-1)
    be = (amax.contiguous().view(torch.int32) >> 23) & 0xFF      # floor(log2(amax)) + 127 for normal amax, 0 for zero / subnormal
    sb = (be - 2).clamp(0, 254)
    inv = torch.pow(2.0, (127 - sb).double()).float()            # 2^-(sb - 127), exact
    codes = to_e2m1_codes(xb * inv.unsqueeze(-1))
    return pack(codes.reshape(shp)), sb.to(torch.uint8)


def dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(packed q [..., C / 2], s [..., C / 32]) -> fp64 [..., C]."""
    v = from_e2m1_codes(unpack(q)).double()
    shp = v.shape
    v = v.reshape(*shp[:-1], shp[-1] // 32, 32)
    return (v * torch.pow(2.0, s.double() - 127).unsqueeze(-1)).reshape(shp)


def as_mxfp8(q: torch.Tensor, s: torch.Tensor):
    """The same table as e4m3 bytes with the same scales (every e2m1 value is an e4m3 value): oracle.mxfp8's dequantize and
    grouped_matmul then serve unchanged."""
    return from_e2m1_codes(unpack(q)).to(torch.float8_e4m3fn).view(torch.uint8), s
