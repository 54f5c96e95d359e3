// Row-space grouped GEMM for FEW rows (decode: T = batch size, 2..32 routed rows over up to 64 experts), bf16 in / fp32 accumulate,
// for gfx950 (MI355X).  Forward epilogues only.  The launch is bound by the bytes of the active experts' weights, so the kernel is a
// weight streamer (kernel guide, GEMM staging table, row "GEMV / M <= 16 decode weights"): every weight element is loaded once per
// 16-row block, 16 bytes per lane straight into VGPRs, several K-steps in flight per wave, and is used by one
// v_mfma_f32_16x16x32_bf16.  An expert with more rows is walked in 16-row blocks, each of which streams the weight slab again: the
// 128x128 / 256x256 kernels are the right ones from a few dozen rows per expert on (tools/decode_bench.py).
//
// Decomposition.  One workgroup of 8 waves per (16-row block of one expert, slab of 16 * NB output columns).  The 8 waves deal the
// K range among themselves in contiguous runs of 32-element K-steps (wave w: steps [w * per, (w + 1) * per)); each keeps NB fp32
// accumulator tiles.  The partial tiles meet in LDS and are summed in wave order 0..7 by the threads that run the epilogue: a fixed
// order, no atomics, bit-identical from run to run.  Splitting K inside the workgroup needs no workspace, no second launch and no
// traffic between workgroups, and gives 512 workgroups x 8 waves at the smallest case (T = 1, second GEMM, N = 4096).  Blocks of the
// grid past the last tile (the host sizes it from an upper bound of the number of row blocks: the counts stay on the device) find that
// out from the offsets and return; experts without rows own no tile.
//
// MFMA roles are swapped as in gemm_bf16.hip: the weights feed the A input (rows = output columns n), the token rows the B input
// (columns = output rows m), so lane (g = lane / 16, i = lane % 16) ends with columns n0 + 4g .. 4g + 3 of row i.
//   B_NK (weights [N, Kd], K-contiguous): lane (g, i) loads the 8 elements k0 + 8g .. + 7 of weight row n0 + i: its MFMA fragment as
//         stored.  No LDS.
//   B_KN (weights [Kd, N], N-contiguous: the pretrain stack's keys / values): the fragment is strided in memory.  A K-step's 32 k-rows
//         x slab are fetched in 16-byte pieces of one k-row, written to a wave-private LDS image [32][slab + 8] and read back with
//         ds_read_b64_tr_b16 (two 4 x 16 blocks per fragment, guide T10).  Only the owning wave touches its image: LDS executes a
//         wave's instructions in order, so no barrier is needed; every lane takes part in every transposed read (EXEC all ones: the
//         trip counts are wave-uniform).
//   Token rows: lane (g, i) loads elements k0 + 8g .. + 7 of its row straight from global memory (at most 16 rows x Kd, L2-resident
//         and shared by all column slabs).  With `src_rows` the row is A[src_rows[m] / src_div]: the gather of csmoe_dispatch_rows.
//
// Bounds (nothing outside the operands is read, nothing outside this expert's rows x [0, N) is written):
//   * lanes i >= rows of a partial block take row0's row index instead (row0 < offsets[e + 1] <= M always holds: a tile exists only
//     for a non-empty block), so src_rows[] is read at m in [row0, offsets[e + 1]) only and A at rows the caller named;
//   * weight rows n >= N (B_NK) are clamped to N - 1, column pieces past N (B_KN) to N - 8 (N % 8 == 0, N >= 8): in bounds, and the
//     columns they feed are never stored;
//   * K-steps below Kd / 32 are whole; the one partial step (Kd % 32 = 8, 16 or 24) loads a piece only where k0 + 8g < Kd (B_NK, A)
//     / its k-row < Kd (B_KN) and zero-fills the registers otherwise.  Kd % 8 == 0 makes every 8-element piece whole or absent;
//   * stores: thread (r, cg) of the epilogue writes 8 columns at n0 + 8 cg of row row0 + r only when r < rows and n0 + 8 cg < N.
//
// Epilogue = the non-gradient branch of gemm_bf16.hip's, same rounding points (include/csmoe.h), 8 columns per thread through
// act_fwd8, 16-byte stores.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 everywhere):
//   kernel <layout, NB>    VGPRs  AGPRs  SGPRs  LDS bytes / block  scratch  occupancy (waves / SIMD)
//   <B_NK, 1>                 78      0     59             10,240        0                         6
//   <B_NK, 2>                 78      0     59             18,432        0                         6
//   <B_KN, 2>                 98      0     59             20,480        0                         4
//   <B_KN, 4>                126      0     59             36,864        0                         4
//
// Replaces, for few rows: cvmm_kernel (moe_pretrain_model/layers/cvmm.py:61-168) and the per-expert nn.Linear calls of compute_moe
// (moe_model/model/moe/moe.py:196-204) with the gather of moe.py:201 / cvmm.py:114-119 folded into the first product.
#include "gemm_tiles.h"
#include <algorithm>

using namespace ggt;

namespace {

constexpr int NW = 8;      // waves per workgroup (the K range of a tile is dealt to them)
constexpr int U = 4;       // K-steps whose loads a wave issues before it waits for the first

struct SkinnyArgs {
  const bf16* A; int64_t lda; const int32_t* src_rows; int src_div;
  const void* const* b_ptrs; int64_t ldb; const void* const* bias_ptrs;
  const int32_t* offsets; int E, M, N, Kd;
  bf16* C; bf16* C2; int64_t ldc; int epilogue, act;
};

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ bf16x8 zero8() {
  const i32x4 z = {0, 0, 0, 0};
  return __builtin_bit_cast(bf16x8, z);
}

template <int LAYOUT, int NB>
__global__ void __launch_bounds__(NW * 64) skinny_kernel(SkinnyArgs p) {
  constexpr int SLAB = 16 * NB;                       // output columns per workgroup
  constexpr int LDW = SLAB + 4;                       // floats per row of a wave's partial tile
  constexpr int RED_B = NW * 16 * LDW * 4;
  constexpr int ROWB = 2 * SLAB + 16;                 // B_KN image: bytes per k-row (16-byte pad)
  constexpr int STG_B = LAYOUT == CSMOE_B_KN ? NW * 32 * ROWB : 0;
  constexpr int CPR = 2 * NB;                         // B_KN: 16-byte pieces per k-row of the slab; NB loads per lane cover 32 k-rows
  __shared__ __attribute__((aligned(16))) char smem[RED_B > STG_B ? RED_B : STG_B];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, i16 = lane & 15;

  // ---------------- tile lookup (wave-uniform) ----------------
  const int ncs = (p.N + SLAB - 1) / SLAB;
  FIND_TILE_OR_RETURN(tp, p.offsets, p.E, p.M, 16, ncs, 0, 0);
  const int e = __builtin_amdgcn_readfirstlane(tp.e);
  const int row0 = __builtin_amdgcn_readfirstlane(tp.o0 + tp.mt * 16);
  const int rows = __builtin_amdgcn_readfirstlane(min(16, tp.o1 - row0));
  const int n0 = __builtin_amdgcn_readfirstlane(tp.nt * SLAB);

  // ---------------- operand addresses ----------------
  const int mm = row0 + (i16 < rows ? i16 : 0);
  const int64_t srow = p.src_rows ? (int64_t)(p.src_rows[mm] / p.src_div) : (int64_t)mm;
  const bf16* pa = p.A + srow * p.lda + 8 * g;
  const bf16* wb = (const bf16*)p.b_ptrs[e];
  const bf16* pb[NB];
  [[maybe_unused]] int kn_kr[NB];                                      // B_KN: k-row of this lane's piece in load i
  if constexpr (LAYOUT == CSMOE_B_NK) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) pb[nb] = wb + (int64_t)min(n0 + nb * 16 + i16, p.N - 1) * p.ldb + 8 * g;
  } else {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int P = i * 64 + lane;
      kn_kr[i] = P / CPR;
      pb[i] = wb + (int64_t)kn_kr[i] * p.ldb + min(n0 + (P % CPR) * 8, p.N - 8);
    }
  }
  char* const stg = smem + wave * (32 * ROWB);        // B_KN: this wave's image
  const int tr_off = (8 * g + (i16 >> 2)) * ROWB + (i16 & 3) * 8;

  // ---------------- this wave's K-steps ----------------
  const int nst = (p.Kd + 31) >> 5, nfull = p.Kd >> 5;
  const int per = (nst + NW - 1) / NW;
  const int s0 = min(wave * per, nst), s1 = min(s0 + per, nst);
  const int f1 = min(s1, nfull);                      // [s0, f1): whole steps; step nfull (if any) is the partial one

  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragments of one K-step from the loaded pieces, and its MFMAs
  auto step = [&](const bf16x8& fa, const bf16x8 (&fb)[NB]) {
    if constexpr (LAYOUT == CSMOE_B_NK) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[nb], fa, acc[nb], 0, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < NB; ++i) *(bf16x8*)(stg + kn_kr[i] * ROWB + ((i * 64 + lane) % CPR) * 16) = fb[i];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(stg + tr_off + nb * 32));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(stg + tr_off + nb * 32 + 4 * ROWB));
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, v), fa, acc[nb], 0, 0, 0);
      }
    }
  };
  auto load = [&](int s, bf16x8& fa, bf16x8 (&fb)[NB]) {
    fa = *(const bf16x8*)(pa + s * 32);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      if constexpr (LAYOUT == CSMOE_B_NK) fb[i] = *(const bf16x8*)(pb[i] + s * 32);
      else fb[i] = *(const bf16x8*)(pb[i] + (int64_t)s * 32 * p.ldb);
    }
  };

  int s = s0;
  for (; s + U <= f1; s += U) {
    bf16x8 fa[U], fb[U][NB];
#pragma unroll
    for (int u = 0; u < U; ++u) load(s + u, fa[u], fb[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) step(fa[u], fb[u]);
  }
  for (; s < f1; ++s) {
    bf16x8 fa, fb[NB];
    load(s, fa, fb);
    step(fa, fb);
  }
  if (s0 <= nfull && nfull < s1) {                    // the partial last step: pieces past Kd are zero registers, never loads
    const int k0 = nfull * 32;
    bf16x8 fa = zero8(), fb[NB];
    if (k0 + 8 * g < p.Kd) fa = *(const bf16x8*)(pa + k0);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      fb[i] = zero8();
      if constexpr (LAYOUT == CSMOE_B_NK) {
        if (k0 + 8 * g < p.Kd) fb[i] = *(const bf16x8*)(pb[i] + k0);
      } else {
        if (k0 + kn_kr[i] < p.Kd) fb[i] = *(const bf16x8*)(pb[i] + (int64_t)k0 * p.ldb);
      }
    }
    step(fa, fb);
  }

  // ---------------- the 8 partial tiles meet in LDS (overlaying the B_KN images) ----------------
  __syncthreads();
  SKINNY_STORE_PARTIAL((float*)smem, acc);

  // ---------------- epilogue: thread (r, cg) owns 8 columns of one row ----------------
  const int r = threadIdx.x / CPR, cg = threadIdx.x % CPR;
  const int ncol = n0 + cg * 8;
  if (r >= rows || ncol >= p.N) return;
  SKINNY_SUM_PARTIALS(v, (float*)smem, r, cg);
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool post_bias = p.epilogue == CSMOE_EPI_ROUND_BIAS32_ACT;     // fp32 bias added to the ROUNDED product (cvmm + bias)
  if (p.epilogue != CSMOE_EPI_PLAIN) {
    const void* bias = p.bias_ptrs ? p.bias_ptrs[e] : nullptr;
    if (bias && post_bias) {
      const f32x4 b0 = *(const f32x4*)((const float*)bias + ncol), b1 = *(const f32x4*)((const float*)bias + ncol + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { bv[j] = b0[j]; bv[4 + j] = b1[j]; }
    } else if (bias) {
      const bf16x8 b8 = *(const bf16x8*)((const bf16*)bias + ncol);
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = (float)b8[j];
    }
  }
  const int64_t o = (int64_t)(row0 + r) * p.ldc + ncol;
  bf16x8 o0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (post_bias) { v[j] = (float)(bf16)v[j] + bv[j]; o0[j] = (bf16)v[j]; }
    else { o0[j] = (bf16)(v[j] + bv[j]); v[j] = (float)o0[j]; }
  }
  if (p.C) *(bf16x8*)(p.C + o) = o0;
  if ((p.epilogue == CSMOE_EPI_BIAS_ACT || post_bias) && p.C2) {
    act_fwd8(v, p.act);
    bf16x8 o1;
#pragma unroll
    for (int j = 0; j < 8; ++j) o1[j] = (bf16)v[j];
    *(bf16x8*)(p.C2 + o) = o1;
  }
}

}  // namespace

// the shape rule of gg_fast_rowspace_ok without the pointers (a pure host query)
bool gg_skinny_shape_ok(int64_t lda, int64_t ldb, int64_t ldc, int M, int N, int Kd) {
  if (N < 8 || Kd < 8 || N % 8 || Kd % 8 || lda % 8 || ldb % 8 || ldc % 8) return false;
  if ((int64_t)M * lda * 2 >= (int64_t)OOB) return false;
  if ((int64_t)std::max(N, Kd) * ldb * 2 >= (int64_t)OOB) return false;
  return true;
}

int gg_skinny_rowspace(const void* A, int64_t lda, const int32_t* src_rows, int src_div, const void* const* b_ptrs, int b_layout,
                       int64_t ldb, const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd, void* C,
                       void* C2, int64_t ldc, int epilogue, int act, hipStream_t st) {
  SkinnyArgs p{};
  p.A = (const bf16*)A; p.lda = lda; p.src_rows = src_rows; p.src_div = src_rows ? src_div : 1;
  p.b_ptrs = b_ptrs; p.ldb = ldb; p.bias_ptrs = bias_ptrs; p.offsets = offsets; p.E = E; p.M = M; p.N = N; p.Kd = Kd;
  p.C = (bf16*)C; p.C2 = (bf16*)C2; p.ldc = ldc; p.epilogue = epilogue; p.act = act;
  const int64_t nrb = skinny_row_blocks(M, E);
  // the wider slab (half the token-row loads per weight byte; 128-byte k-row pieces for B_KN) once it still gives two workgroups
  // per CU; the narrow one below that
  const int big = b_layout == CSMOE_B_NK ? 2 : 4;
  const bool wide = nrb * ((N + 16 * big - 1) / (16 * big)) >= 512;
  const int nb = wide ? big : big / 2;
  unsigned grid;
  const int rc = grid_1d("grouped_gemm_skinny", nrb * ((N + 16 * nb - 1) / (16 * nb)), &grid);
  if (rc || !grid) return rc;
  const dim3 gr(grid), bl(NW * 64);
  if (b_layout == CSMOE_B_NK) {
    if (nb == 2) hipLaunchKernelGGL((skinny_kernel<CSMOE_B_NK, 2>), gr, bl, 0, st, p);
    else hipLaunchKernelGGL((skinny_kernel<CSMOE_B_NK, 1>), gr, bl, 0, st, p);
  } else {
    if (nb == 4) hipLaunchKernelGGL((skinny_kernel<CSMOE_B_KN, 4>), gr, bl, 0, st, p);
    else hipLaunchKernelGGL((skinny_kernel<CSMOE_B_KN, 2>), gr, bl, 0, st, p);
  }
  CSMOE_CHECK_LAUNCH("grouped_gemm_skinny");
  return CSMOE_OK;
}
