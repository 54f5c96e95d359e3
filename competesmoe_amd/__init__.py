"""MI355X-native (gfx950) sparse-MoE hot path for CompeteSMoE-style training.

HIP kernels behind a C ABI (include/csmoe.h) + the reference's nn.Module / registry surface on top.
Importing this package loads `lib/libcsmoe_hip.so`; there is no CPU fallback.
"""
from . import _lib  # noqa: F401  (fails loudly when the HIP library is not built)

__all__ = ["_lib", "decode_rows", "decode_front"]


def decode_rows(n=None) -> int:
    """Decode-path switch: `n` = the largest number of routed rows (T * K) a forward-only call may have to run its expert GEMMs on
    the weight-streaming kernel (csmoe_grouped_gemm_skinny; csmoe_grouped_gemm_skinny_mxfp8 in the fp8 layers with
    `args.fp8_weight_cache`, or csmoe_grouped_gemm_skinny_mxfp4w on MXFP4 weight tables where such a layer also sets
    `args.fp4_decode_weights`) without a dispatch copy; 0 (the default, or CSMOE_DECODE_ROWS unset) switches the path off.
    Returns the value in force; `decode_rows()` only reads it."""
    from . import ops
    return ops.decode_rows(n)


def decode_front(on=None) -> bool:
    """Decode front end switch: with it on, a call in no-grad mode with at most decode_rows() routed rows, on a layer whose gate is
    the plain bf16 linear map (E <= 256), routes, bins and -- in the fp8 layers with `args.fp8_weight_cache` -- quantises its tokens
    in ONE launch (csmoe_decode_route) instead of the router, binning and quantiser launches; the expert GEMMs and the combine are
    the same launches on the same operands.  Off by default (or CSMOE_DECODE_FRONT unset); CSMOE_DECODE_FRONT=1 switches it on.
    Returns the value in force; `decode_front()` only reads it."""
    from . import ops
    return ops.decode_front(on)
