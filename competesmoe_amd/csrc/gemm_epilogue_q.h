// CSMOE_EPI_BIAS_ACT epilogue of the 8-wave 256x256 MXFP8 kernel with a QUANTISED activated output (gemm_fp8.hip, gg8fq_kernel):
// next to the bf16 C = round(acc + bias) and C2 = round(act(C)) of gemm_epilogue.h's epi_run<EC_BIAS_ACT>, either of which may be
// left out, it writes C2 as MXFP8 -- Cq [M, N] e4m3 bytes and Cs [M, N/32] e8m0 scales, blocks along N: the operand orientation
// of the GEMM that reads the activations next -- byte for byte what csmoe_quantize_mxfp8(transpose = 0) gives for the bf16 C2 of
// the same launch (the ROUNDED activated value is quantised, through mx_quant.h like every MXFP8 writer).
//
// A header of its own, reached only from gg8fq_kernel: one more case in rowspace_epilogue would change the code of the
// instantiations every other launch runs (gemm_epilogue.h; EC_ACCUM was kept out the same way).
//
// Mapping (epi_run's): after the staging barrier thread t holds columns (t % 32) * 8 .. + 7 of row t / 32 + 16 i, so the four
// lanes l, l ^ 1, l ^ 2, l ^ 3 hold one 32-column block and its amax is two cross-lane steps (csmoe_dispatch_tokens_mxfp8's;
// fmaxf drops a NaN operand, so the order of the maxima does not matter and the result is quant_rows_kernel's).  N % 32 == 0 makes
// a block lie inside the matrix or outside it as a whole.  Lanes past `rows` or past the last column take part in the shuffles with
// zeros and store nothing.
#pragma once
#include "gemm_epilogue.h"
#include "mx_quant.h"

namespace ggt {

struct EpiQArgs {
  uint8_t* Cq; uint8_t* Cs;      // [M, ldcq] e4m3, [M, ldcs] e8m0
  int64_t ldcq, ldcs;
};

template <int ACT>
__device__ __forceinline__ void epi_run_q(const EpiArgs& p, const EpiQArgs& q, const f32x4 (&acc)[Lay8::NCB][Lay8::NRB], char* smem,
                                          int row0, int rows, int tc0, int wm, int wn, int lane) {
  using LAY = Lay8;
  constexpr int RSTEP = LAY::THREADS / 32, RPT = 256 / RSTEP;     // 16 rows per pass, 16 rows per thread
  bf16* stg = (bf16*)smem;
  const int g = lane >> 4, i16 = lane & 15;
  const int ec = (threadIdx.x & 31) * 8;
  const int er = threadIdx.x >> 5;
  const int ncol = tc0 + ec;
  const bool col_ok = ncol < p.NC;

  // ---- stage: accumulators (+ bf16 bias, added before the rounding as F.linear does) -> bf16 -> LDS (epi_run<EC_BIAS_ACT>)
#pragma unroll
  for (int cb = 0; cb < LAY::NCB; ++cb) {
    const int n = LAY::n(wn, cb, g);
    float b[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias && tc0 + n < p.NC) {
      const bf16x4 b4 = *(const bf16x4*)((const bf16*)p.bias + tc0 + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = (float)b4[j];
    }
#pragma unroll
    for (int rb = 0; rb < LAY::NRB; ++rb) {
      const int m = LAY::m(wm, rb, i16);
      bf16x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (bf16)(acc[cb][rb][j] + b[j]);
      *(bf16x4*)(stg + m * EPI_LD + n) = o;
    }
  }
  EPI_SYNC();

  // ---- rows: every thread walks all 16 of its rows (the staging tile holds 256), the stores are predicated
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    const int r = er + RSTEP * i;
    const bool live = col_ok && r < rows;
    const bf16x8 o0 = *(const bf16x8*)(stg + r * EPI_LD + ec);
    const int64_t o = (int64_t)(row0 + r) * p.ldc + ncol;
    if (live && p.C) *(bf16x8*)((bf16*)p.C + o) = o0;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)o0[j];
    epi_act_fwd8<ACT>(v, p.act);
    bf16x8 o1;
    float f[8];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o1[j] = (bf16)v[j];
      f[j] = live ? (float)o1[j] : 0.f;              // the quantiser sees what quantize_mxfp8 would read back from C2
      amax = fmaxf(amax, fabsf(f[j]));
    }
    if (live && p.C2) *(bf16x8*)((bf16*)p.C2 + o) = o1;
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    const int sb = e8m0_of_amax(amax);
    const float inv = inv_scale_of(sb);
    u32x2 w;
    w[0] = pack4_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
    w[1] = pack4_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
    if (live) {
      *(u32x2*)(q.Cq + (int64_t)(row0 + r) * q.ldcq + ncol) = w;
      if ((lane & 3) == 0) q.Cs[(int64_t)(row0 + r) * q.ldcs + (ncol >> 5)] = (uint8_t)sb;
    }
  }
}

// Called by all of the workgroup's threads after the K-loop's LDS traffic has drained, like rowspace_epilogue.
__device__ __forceinline__ void rowspace_epilogue_q(const EpiArgs& p, const EpiQArgs& q, const f32x4 (&acc)[Lay8::NCB][Lay8::NRB],
                                                    char* smem, int row0, int rows, int tc0, int wm, int wn, int lane) {
  if (p.act == CSMOE_ACT_GELU) epi_run_q<CSMOE_ACT_GELU>(p, q, acc, smem, row0, rows, tc0, wm, wn, lane);
  else if (p.act == CSMOE_ACT_RELU) epi_run_q<CSMOE_ACT_RELU>(p, q, acc, smem, row0, rows, tc0, wm, wn, lane);
  else epi_run_q<ACT_RT>(p, q, acc, smem, row0, rows, tc0, wm, wn, lane);
}

}  // namespace ggt
