// The scale-and-convert step of the MXFP8 quantiser (OCP Microscaling: shared exponent = floor(log2(amax)) - emax_elem,
// emax(e4m3) = 8; elements = round-to-nearest-even(x * 2^-shared), saturated at +-448, NaN kept).  One copy for every kernel that
// writes MXFP8: the quantisers of fp8_quant.hip and the fused quantised output of gemm_skinny_fp8.hip, which must agree byte for byte.
#pragma once
#include "common.h"

__device__ __forceinline__ int e8m0_of_amax(float amax) {
  // biased exponent byte of 2^(floor(log2(amax)) - 8); amax == 0 (or subnormal) -> the smallest scale
  const int be = (int)((__float_as_uint(amax) >> 23) & 0xff);      // floor(log2(amax)) + 127 for normal amax
  const int s = be - 8;
  return s < 0 ? 0 : (s > 254 ? 254 : s);
}
__device__ __forceinline__ float inv_scale_of(int sbyte) {         // 2^-(sbyte - 127), exact
  const int e = 254 - sbyte;                                       // biased exponent of the reciprocal
  return e <= 0 ? __uint_as_float(0x00400000u >> (-e)) : __uint_as_float((unsigned)e << 23);
}
// saturate to +-448 but let a NaN through (fminf / fmaxf return their non-NaN operand, which would turn NaN into -448): the
// conversion below encodes it as the e4m3 NaN, so a NaN activation still poisons its output row as it does on the bf16 path
__device__ __forceinline__ float sat448(float v) { return v != v ? v : fminf(fmaxf(v, -448.f), 448.f); }
__device__ __forceinline__ unsigned pack4_e4m3(float a, float b, float c, float d) {
  a = sat448(a); b = sat448(b); c = sat448(c); d = sat448(d);
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (unsigned)w;
}
