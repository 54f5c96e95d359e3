// What the two MX decode kernels share (gemm_skinny_fp8.hip: MXFP8 weights; gemm_skinny_fp4.hip: MXFP4 weights) besides
// gemm_tiles.h: the argument block and the operand types.  Their epilogue is gemm_skinny_mx_epilogue.inc.
#pragma once
#include "gemm_tiles.h"
#include "mx_quant.h"
#include <algorithm>

using namespace ggt;

namespace {

constexpr int NW = 8;      // waves per workgroup (the K range of a tile is dealt to them)

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((address_space(1))) uint8_t gbyte;
typedef __attribute__((address_space(1))) i32x4 gi32x4;

// ldb counts BYTES of a weight row (Kd for e4m3, Kd / 2 for packed e2m1)
struct Skinny8Args {
  const uint8_t* A; int64_t lda; const uint8_t* AS; int64_t ldas; const int32_t* src_rows; int src_div;
  const void* const* bq_ptrs; const void* const* bs_ptrs; int64_t ldb, ldbs; const void* const* bias_ptrs;
  const int32_t* offsets; int E, M, N, Kd;
  bf16* C; bf16* C2; int64_t ldc; uint8_t* Cq; uint8_t* Cs; int64_t ldcq, ldcs; int epilogue, act;
};

}  // namespace
