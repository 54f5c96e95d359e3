// The scale-and-convert step of the MXFP8 quantiser (OCP Microscaling: shared exponent = floor(log2(amax)) - emax_elem,
// emax(e4m3) = 8; elements = round-to-nearest-even(x * 2^-shared), saturated at +-448, NaN kept).  One copy for every kernel that
// writes MXFP8: the quantisers of fp8_quant.hip and the fused quantised output of gemm_skinny_mx.hip, which must
// agree byte for byte.  The MXFP4 step of the weight quantiser follows it.
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

// ---- MXFP4 (weights of the W4A8 decode path, gemm_skinny_mx.hip) ------------------------------------------------------------------
// OCP e2m1 elements (sign, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6), emax(e2m1) = 2: shared exponent = floor(log2(amax)) - 2, so the
// scaled block lies in (-8, 8); elements = round-to-nearest-even(x * 2^-shared) on that grid, saturated at +-6.  Plain compares: the
// seven midpoints of the grid, a tie going to the code with the even mantissa bit (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2,
// 2.5 -> 2, 3.5 -> 4, 5 -> 4).  Non-finite values are outside the contract: +-inf saturates to +-6, a NaN fails every compare and
// becomes +-0 (its sign bit); a block that holds one takes the scale byte 253 like any amax with exponent 255.
__device__ __forceinline__ int e8m0_of_amax_fp4(float amax) {
  const int s = (int)((__float_as_uint(amax) >> 23) & 0xff) - 2;
  return s < 0 ? 0 : (s > 254 ? 254 : s);
}
__device__ __forceinline__ unsigned e2m1_of(float v) {
  const float a = fabsf(v);
  const unsigned m = (unsigned)(a > 0.25f) + (unsigned)(a >= 0.75f) + (unsigned)(a > 1.25f) + (unsigned)(a >= 1.75f) +
                     (unsigned)(a > 2.5f) + (unsigned)(a >= 3.5f) + (unsigned)(a > 5.f);
  return ((__float_as_uint(v) >> 28) & 8u) | m;
}
// eight consecutive elements -> one word: element j in bits 4 j .. 4 j + 3 (byte j / 2: the even element in the low nibble)
__device__ __forceinline__ unsigned pack8_e2m1(const float* v, float inv) {
  unsigned w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) w |= e2m1_of(v[j] * inv) << (4 * j);
  return w;
}
