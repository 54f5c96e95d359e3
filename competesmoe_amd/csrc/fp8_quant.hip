// MXFP8 quantisation for the block-scaled MFMA path (BASELINE config 5): OCP e4m3 elements with one e8m0 scale per 32 elements
// ALONG THE REDUCTION DIMENSION of the GEMM that will consume the tensor (OCP Microscaling spec: shared exponent =
// floor(log2(amax)) - emax_elem, emax(e4m3) = 8; elements = round-to-nearest-even(x * 2^-shared), saturated at +-448).
// The reference has no fp8: nothing upstream to cite; the oracle restates this file in torch.
//   rows:       x [R, C] -> q [R, C] u8, s [R, C/32] u8          (blocks along the contiguous dim: activations, K-contiguous weights)
//   transposed: x [R, C] -> q [C, R] u8, s [C, R/32] u8          (blocks along dim 0: the same weights for the transposed product)
// Inputs bf16 or fp32 (the pretrain stack's fp32 master weights are quantised directly: no bf16 cast pass).
// The scale-and-convert device code (e8m0_of_amax, inv_scale_of, sat448, pack4_e4m3) lives in mx_quant.h, shared with the fused
// quantised output of gemm_skinny_mx.hip.  The MXFP4 weight quantiser (csmoe_quantize_mxfp4: e2m1 elements, two per byte, the same
// e8m0 block scales with emax = 2) is the rows / transposed pair once more, at the end of the kernels.
#include "mx_quant.h"
#include <algorithm>
#include <type_traits>

namespace {

template <typename T> __device__ __forceinline__ void load32(const T* p, float (&v)[32]);
template <> __device__ __forceinline__ void load32<bf16>(const bf16* p, float (&v)[32]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const bf16x8 x = *(const bf16x8*)(p + 8 * c);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[8 * c + j] = (float)x[j];
  }
}
template <> __device__ __forceinline__ void load32<float>(const float* p, float (&v)[32]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const f32x4 x = *(const f32x4*)(p + 4 * c);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[4 * c + j] = x[j];
  }
}

// one lane per 32-element block; blocks of a row are consecutive lanes.  grid.y = matrix (expert) index
template <typename T>
__global__ void __launch_bounds__(256) quant_rows_kernel(const void* const* x_ptrs, const T* x_single, int64_t ldx, int R, int C,
                                                         uint8_t* q, uint8_t* s, int64_t q_mat, int64_t s_mat) {
  const int e = blockIdx.y;
  const T* x = x_ptrs ? (const T*)x_ptrs[e] : x_single;
  uint8_t* qe = q + (int64_t)e * q_mat;
  uint8_t* se = s + (int64_t)e * s_mat;
  const int nb = C >> 5;
  const int64_t total = (int64_t)R * nb;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / nb), b = (int)(i - (int64_t)r * nb);
    float v[32];
    load32<T>(x + (int64_t)r * ldx + b * 32, v);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(v[j]));
    const int sb = e8m0_of_amax(amax);
    const float inv = inv_scale_of(sb);
    u32x4 o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o0[j] = pack4_e4m3(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
      o1[j] = pack4_e4m3(v[16 + 4 * j] * inv, v[17 + 4 * j] * inv, v[18 + 4 * j] * inv, v[19 + 4 * j] * inv);
    }
    uint8_t* dst = qe + (int64_t)r * C + b * 32;
    *(u32x4*)dst = o0;
    *(u32x4*)(dst + 16) = o1;
    se[(int64_t)r * nb + b] = (uint8_t)sb;
  }
}

// transposed: one wave per 32-row x 64-column tile; lane = column, the 32 rows of the block sit in the lane's registers
template <typename T>
__global__ void __launch_bounds__(256) quant_cols_kernel(const void* const* x_ptrs, const T* x_single, int64_t ldx, int R, int C,
                                                         uint8_t* q, uint8_t* s, int64_t q_mat, int64_t s_mat) {
  const int e = blockIdx.y;
  const T* x = x_ptrs ? (const T*)x_ptrs[e] : x_single;
  uint8_t* qe = q + (int64_t)e * q_mat;       // [C, R]
  uint8_t* se = s + (int64_t)e * s_mat;       // [C, R/32]
  const int lane = threadIdx.x & 63;
  const int rb_n = R >> 5, cb_n = (C + 63) >> 6;
  const int64_t tiles = (int64_t)rb_n * cb_n;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * 4) {
    const int rb = (int)(t / cb_n), cb = (int)(t - (int64_t)rb * cb_n);
    const int c = cb * 64 + lane;
    if (c >= C) continue;
    float v[32];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      v[i] = (float)x[(int64_t)(rb * 32 + i) * ldx + c];
      amax = fmaxf(amax, fabsf(v[i]));
    }
    const int sb = e8m0_of_amax(amax);
    const float inv = inv_scale_of(sb);
    u32x4 o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o0[j] = pack4_e4m3(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
      o1[j] = pack4_e4m3(v[16 + 4 * j] * inv, v[17 + 4 * j] * inv, v[18 + 4 * j] * inv, v[19 + 4 * j] * inv);
    }
    uint8_t* dst = qe + (int64_t)c * R + rb * 32;
    *(u32x4*)dst = o0;
    *(u32x4*)(dst + 16) = o1;
    se[(int64_t)c * rb_n + rb] = (uint8_t)sb;
  }
}

// both orientations in ONE pass over the source (weights: the forward product needs blocks along one dim, the backward product
// along the other; reading 4-byte masters twice was the larger half of the fp8 step's quantisation time).  One 256-thread
// workgroup per 64-row x 128-column tile: 16-byte global loads (512 B per row and wave-instruction, 8 in flight per thread) into an
// fp32 LDS tile (33 KiB: four workgroups per CU), then the 256 (row, 32-column block) units and the 256 (column, 32-row block) units
// are quantised one each per thread straight from LDS -- rows by ds_read_b128 along the row, columns by ds_read_b32 down the
// column (consecutive lanes = consecutive banks) -- and every output leaves as 16-byte stores; two threads complete a 64-byte run
// of a transposed row.  6 B of HBM traffic per element with fp32 masters (4 read + 2 written).
// Tile height, same box (gpurun_out r2x / r3n): 32 rows (lone 32-byte pieces of the transposed rows, 8 workgroups per CU) 4.50 ms per
// call = 3.9 TB/s; 64 rows 4.18 ms = 4.2 TB/s; 128 rows (66 KiB of LDS, 2 workgroups per CU: too few to keep HBM busy while a
// workgroup's load and quantise phases do not overlap) 5.49 ms.
constexpr int QB_R = 64, QB_C = 128, QB_LD = QB_C + 4;       // +4 floats: rows 16 B apart in bank space (b128 row reads)

template <typename T>
__global__ void __launch_bounds__(256) quant_both_kernel(const void* const* x_ptrs, const T* x_single, int64_t ldx, int R, int C,
                                                         uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, int64_t q_mat,
                                                         int64_t s_mat, int64_t st_mat) {
  __shared__ __attribute__((aligned(16))) float tile[QB_R * QB_LD];
  const int e = blockIdx.y;
  const T* x = x_ptrs ? (const T*)x_ptrs[e] : x_single;
  uint8_t* qe = q + (int64_t)e * q_mat;         // [R, C]
  uint8_t* se = s + (int64_t)e * s_mat;         // [R, C/32]
  uint8_t* qte = qt + (int64_t)e * q_mat;       // [C, R]
  uint8_t* ste = st + (int64_t)e * st_mat;      // [C, R/32]
  const int t = threadIdx.x;
  const int rt_n = (R + QB_R - 1) / QB_R, cb_n = (C + QB_C - 1) / QB_C, nbc = C >> 5, nbr = R >> 5;
  const int64_t tiles = (int64_t)rt_n * cb_n;
  // A tile's eight 16-byte loads per thread are all issued into registers before the first LDS write (round 3: 4.2 -> 4.5 TB/s; written
  // as load-then-store per row, hipcc waited for each load in turn).  When a workgroup has more than one tile (grids beyond 16 384
  // tiles per expert) the next tile's loads are issued before the current one is quantised.
  f32x4 nxt[8];
  auto fetch = [&](int64_t ti) {
    const int rt = (int)(ti / cb_n), cb = (int)(ti - (int64_t)rt * cb_n);
    const int r0 = rt * QB_R, c0 = cb * QB_C;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = (t >> 5) + 8 * i, c = (t & 31) * 4;      // thread -> (row t / 32 + 8 i, 4 columns (t % 32) * 4)
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (c0 + c < C && r0 + r < R) {
        const T* src = x + (int64_t)(r0 + r) * ldx + c0 + c;
        if constexpr (std::is_same<T, float>::value) {
          v = *(const f32x4*)src;
        } else {
          const bf16x4 h = *(const bf16x4*)src;
          v = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        }
      }
      nxt[i] = v;
    }
  };
  if ((int64_t)blockIdx.x < tiles) fetch(blockIdx.x);
  for (int64_t ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
    const int rt = (int)(ti / cb_n), cb = (int)(ti - (int64_t)rt * cb_n);
    const int r0 = rt * QB_R, c0 = cb * QB_C;
#pragma unroll
    for (int i = 0; i < 8; ++i) *(f32x4*)(tile + ((t >> 5) + 8 * i) * QB_LD + (t & 31) * 4) = nxt[i];
    __syncthreads();
    if (ti + gridDim.x < tiles) fetch(ti + gridDim.x);
    {
      // ---- row-major output: unit (row t / 4, column block t % 4)
      const int r = t >> 2, bk = t & 3;
      if (c0 + bk * 32 < C && r0 + r < R) {
        float v[32];
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const f32x4 w4 = *(const f32x4*)(tile + r * QB_LD + bk * 32 + 4 * j);
#pragma unroll
          for (int k = 0; k < 4; ++k) { v[4 * j + k] = w4[k]; amax = fmaxf(amax, fabsf(w4[k])); }
        }
        const int sb = e8m0_of_amax(amax);
        const float inv = inv_scale_of(sb);
        u32x4 o0, o1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o0[j] = pack4_e4m3(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
          o1[j] = pack4_e4m3(v[16 + 4 * j] * inv, v[17 + 4 * j] * inv, v[18 + 4 * j] * inv, v[19 + 4 * j] * inv);
        }
        uint8_t* dst = qe + (int64_t)(r0 + r) * C + c0 + bk * 32;
        *(u32x4*)dst = o0;
        *(u32x4*)(dst + 16) = o1;
        se[(int64_t)(r0 + r) * nbc + (c0 >> 5) + bk] = (uint8_t)sb;
      }
    }
    {
      // ---- transposed output: column t % 128, row block t / 128 (two threads complete a 64-byte run of the column)
      const int c = t & 127, rbk = t >> 7;
      if (c0 + c < C && r0 + rbk * 32 < R) {
        float v[32];
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) { v[i] = tile[(rbk * 32 + i) * QB_LD + c]; amax = fmaxf(amax, fabsf(v[i])); }
        const int sb = e8m0_of_amax(amax);
        const float inv = inv_scale_of(sb);
        u32x4 o0, o1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o0[j] = pack4_e4m3(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
          o1[j] = pack4_e4m3(v[16 + 4 * j] * inv, v[17 + 4 * j] * inv, v[18 + 4 * j] * inv, v[19 + 4 * j] * inv);
        }
        uint8_t* dst = qte + (int64_t)(c0 + c) * R + r0 + rbk * 32;
        *(u32x4*)dst = o0;
        *(u32x4*)(dst + 16) = o1;
        ste[(int64_t)(c0 + c) * nbr + (r0 >> 5) + rbk] = (uint8_t)sb;
      }
    }
    __syncthreads();
  }
}

// ---- token-dim quantisation of binned rows (the operands of the MXFP8 weight gradient) ---------------------------------------
// The weight gradient reduces over the tokens, so its operands need blocks of 32 consecutive BINNED ROWS OF ONE EXPERT: expert e's
// count_e rows are laid out at padded positions poff[e] .. poff[e] + count_e, poff[e] = sum_{j<e} roundup(count_j, 128), the rest
// of the expert's range up to poff[e+1] is zero.  Blocks start at the expert's first row, so none straddles two experts, and a
// 128-byte K-tile of the GEMM belongs to one expert.

// poff[0..E] from offsets[0..E]: one workgroup, a contiguous run of experts per thread and a scan over the 256 partial sums
__global__ void __launch_bounds__(256) token_pad_offsets_kernel(const int32_t* offsets, int E, int32_t* poff) {
  __shared__ int part[256];
  const int t = threadIdx.x;
  const int per = (E + 255) / 256;
  const int e0 = min(E, t * per), e1 = min(E, e0 + per);
  int sum = 0;
  for (int e = e0; e < e1; ++e) sum += (offsets[e + 1] - offsets[e] + 127) & ~127;
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int run = part[t] - sum;                       // exclusive prefix
  for (int e = e0; e < e1; ++e) {
    poff[e] = run;
    run += (offsets[e + 1] - offsets[e] + 127) & ~127;
  }
  if (t == 255) poff[E] = part[255];
}

// One 256-thread workgroup per 64 padded rows x 128 columns (quant_both_kernel's tile and unit mapping): the padded rows map to
// binned source rows of ONE expert (its range is a multiple of 128 long), rows past the expert's count load as zeros.  Row output
// (q / s, indexed by source row) for the real rows only, when requested; transposed output (qt / st) for all 64 padded rows.
template <bool ROWS>
__global__ void __launch_bounds__(256) quant_tokens_kernel(const bf16* x, int64_t ldx, const int32_t* offsets, const int32_t* poff,
                                                           int E, int C, int64_t n_pad, uint8_t* q, uint8_t* s, uint8_t* qt,
                                                           uint8_t* st) {
  __shared__ __attribute__((aligned(16))) float tile[QB_R * QB_LD];
  __shared__ int tile_e;
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * QB_R;
  const int c0 = blockIdx.y * QB_C;
  if (r0 >= poff[E]) return;                     // past the last expert's range: not written
  for (int j = t; j < E; j += 256)
    if (poff[j] <= r0 && r0 < poff[j + 1]) tile_e = j;     // exactly one (non-empty) expert's range holds r0
  __syncthreads();
  const int e = tile_e;
  const int64_t pos = r0 - poff[e];              // position of padded row r0 inside the expert's range
  const int64_t src0 = offsets[e] + pos;         // its source row
  const int64_t nreal = (int64_t)(offsets[e + 1] - offsets[e]) - pos;   // real rows from r0 on (may be <= 0)
  const int nbc = C >> 5;
  const int64_t nbr = n_pad >> 5;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = (t >> 5) + 8 * i, c = (t & 31) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c0 + c < C && r < nreal) {
      const bf16x4 h = *(const bf16x4*)(x + (src0 + r) * ldx + c0 + c);
      v = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    }
    *(f32x4*)(tile + r * QB_LD + c) = v;
  }
  __syncthreads();
  if (ROWS) {
    // ---- row-major output of the real rows: unit (row t / 4, column block t % 4)
    const int r = t >> 2, bk = t & 3;
    if (c0 + bk * 32 < C && r < nreal) {
      float v[32];
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 w4 = *(const f32x4*)(tile + r * QB_LD + bk * 32 + 4 * j);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[4 * j + k] = w4[k]; amax = fmaxf(amax, fabsf(w4[k])); }
      }
      const int sb = e8m0_of_amax(amax);
      const float inv = inv_scale_of(sb);
      u32x4 o0, o1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o0[j] = pack4_e4m3(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
        o1[j] = pack4_e4m3(v[16 + 4 * j] * inv, v[17 + 4 * j] * inv, v[18 + 4 * j] * inv, v[19 + 4 * j] * inv);
      }
      uint8_t* dst = q + (src0 + r) * C + c0 + bk * 32;
      *(u32x4*)dst = o0;
      *(u32x4*)(dst + 16) = o1;
      s[(src0 + r) * nbc + (c0 >> 5) + bk] = (uint8_t)sb;
    }
  }
  {
    // ---- transposed output: column t % 128, padded row block t / 128 (two threads complete a 64-byte run of the column)
    const int c = t & 127, rbk = t >> 7;
    if (c0 + c < C) {
      float v[32];
      float amax = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) { v[i] = tile[(rbk * 32 + i) * QB_LD + c]; amax = fmaxf(amax, fabsf(v[i])); }
      const int sb = e8m0_of_amax(amax);
      const float inv = inv_scale_of(sb);
      u32x4 o0, o1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o0[j] = pack4_e4m3(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
        o1[j] = pack4_e4m3(v[16 + 4 * j] * inv, v[17 + 4 * j] * inv, v[18 + 4 * j] * inv, v[19 + 4 * j] * inv);
      }
      uint8_t* dst = qt + (int64_t)(c0 + c) * n_pad + r0 + rbk * 32;
      *(u32x4*)dst = o0;
      *(u32x4*)(dst + 16) = o1;
      st[(int64_t)(c0 + c) * nbr + (r0 >> 5) + rbk] = (uint8_t)sb;
    }
  }
}


// ---- gather rows into the binned row space AND quantise them, one pass (csmoe_dispatch_rows_mxfp8 / csmoe_dispatch_tokens_mxfp8) ----
// moe_kernels.hip's dispatch kernels followed by quant_rows_kernel write every gathered bf16 row and read it straight back; here the
// row is quantised from the registers that hold it for the copy.  One wave per source row, eight 16-byte loads in flight per lane (one
// 8 KiB row per pass).  A 32-element block is the 16-byte pieces of four consecutive lanes: the block amax is two cross-lane steps
// (xor 1, xor 2; fmaxf drops a NaN operand, so the order of the maxima does not matter and the result is quant_rows_kernel's), every
// lane converts its 8 values and stores 8 bytes, one lane in four stores the scale byte.  D % 32 == 0 makes the pieces of a row a
// multiple of 4, so a quad is in range or out of range as a whole.  TOKENS: the wave's row is token t, stored to its K binned rows
// slot_of[t*K + k] (read and quantised once); else destination row m takes source row perm[m] / K.  xs may be null (no bf16 copy).
#ifndef CSMOE_DQ_LOADS
#define CSMOE_DQ_LOADS 8
#endif
constexpr int DQ_LOADS = CSMOE_DQ_LOADS;      // 16-byte loads in flight per lane
template <bool TOKENS>
__global__ void __launch_bounds__(256) dispatch_quant_kernel(const bf16* x, const int32_t* index, int K, bf16* xs, uint8_t* q,
                                                             uint8_t* s, int n, int D) {
  const int lane = threadIdx.x & 63;
  const int wave_g = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nw = gridDim.x * 4;
  const int nv = D >> 3;                    // 16-byte pieces (8 bf16) per row
  const int nb = D >> 5;                    // scale bytes per row
  for (int r = wave_g; r < n; r += nw) {
    const int64_t srow = TOKENS ? r : index[r] / K;
    const bf16x8* src = (const bf16x8*)(x + srow * D);
    for (int c0 = 0; c0 < nv; c0 += 64 * DQ_LOADS) {
      bf16x8 v[DQ_LOADS];
#pragma unroll
      for (int c = 0; c < DQ_LOADS; ++c) {
        const int i = c0 + c * 64 + lane;
        if (i < nv) v[c] = src[i];
      }
      u32x2 o[DQ_LOADS];
      int sb[DQ_LOADS];
#pragma unroll
      for (int c = 0; c < DQ_LOADS; ++c) {
        const bool live = c0 + c * 64 + lane < nv;
        float f[8];
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          f[j] = live ? (float)v[c][j] : 0.f;
          amax = fmaxf(amax, fabsf(f[j]));
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
        sb[c] = e8m0_of_amax(amax);
        const float inv = inv_scale_of(sb[c]);
        o[c][0] = pack4_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
        o[c][1] = pack4_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
      }
      const int reps = TOKENS ? K : 1;
      for (int k = 0; k < reps; ++k) {
        const int64_t m = TOKENS ? index[(int64_t)r * K + k] : r;
        bf16x8* dst = xs ? (bf16x8*)(xs + m * D) : nullptr;
        u32x2* qd = (u32x2*)(q + m * D);
        uint8_t* sd = s + m * nb;
#pragma unroll
        for (int c = 0; c < DQ_LOADS; ++c) {
          const int i = c0 + c * 64 + lane;
          if (i < nv) {
            if (dst) dst[i] = v[c];
            qd[i] = o[c];
            if ((lane & 3) == 0) sd[i >> 2] = (uint8_t)sb[c];
          }
        }
      }
    }
  }
}

// ---- MXFP4 weight tables (csmoe_quantize_mxfp4): quant_rows_kernel / quant_cols_kernel with e2m1 elements, two per byte -----------
// A block's 32 elements are 16 bytes (element 2 j in the low nibble of byte j): one 16-byte store per block.  q rows are C / 2
// (rows form) or R / 2 (transposed) bytes; the scales as for MXFP8.
__device__ __forceinline__ int quant4_block(const float (&v)[32], u32x4& o) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(v[j]));
  const int sb = e8m0_of_amax_fp4(amax);
  const float inv = inv_scale_of(sb);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = pack8_e2m1(v + 8 * j, inv);
  return sb;
}

template <typename T>
__global__ void __launch_bounds__(256) quant4_rows_kernel(const void* const* x_ptrs, const T* x_single, int64_t ldx, int R, int C,
                                                          uint8_t* q, uint8_t* s, int64_t q_mat, int64_t s_mat) {
  const int e = blockIdx.y;
  const T* x = x_ptrs ? (const T*)x_ptrs[e] : x_single;
  uint8_t* qe = q + (int64_t)e * q_mat;
  uint8_t* se = s + (int64_t)e * s_mat;
  const int nb = C >> 5;
  const int64_t total = (int64_t)R * nb;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / nb), b = (int)(i - (int64_t)r * nb);
    float v[32];
    load32<T>(x + (int64_t)r * ldx + b * 32, v);
    u32x4 o;
    const int sb = quant4_block(v, o);
    *(u32x4*)(qe + ((int64_t)r * nb + b) * 16) = o;
    se[(int64_t)r * nb + b] = (uint8_t)sb;
  }
}

// transposed: one wave per 32-row x 64-column tile; lane = column, the 32 rows of the block sit in the lane's registers
template <typename T>
__global__ void __launch_bounds__(256) quant4_cols_kernel(const void* const* x_ptrs, const T* x_single, int64_t ldx, int R, int C,
                                                          uint8_t* q, uint8_t* s, int64_t q_mat, int64_t s_mat) {
  const int e = blockIdx.y;
  const T* x = x_ptrs ? (const T*)x_ptrs[e] : x_single;
  uint8_t* qe = q + (int64_t)e * q_mat;       // [C, R/2]
  uint8_t* se = s + (int64_t)e * s_mat;       // [C, R/32]
  const int lane = threadIdx.x & 63;
  const int rb_n = R >> 5, cb_n = (C + 63) >> 6;
  const int64_t tiles = (int64_t)rb_n * cb_n;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < tiles; t += (int64_t)gridDim.x * 4) {
    const int rb = (int)(t / cb_n), cb = (int)(t - (int64_t)rb * cb_n);
    const int c = cb * 64 + lane;
    if (c >= C) continue;
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = (float)x[(int64_t)(rb * 32 + i) * ldx + c];
    u32x4 o;
    const int sb = quant4_block(v, o);
    *(u32x4*)(qe + ((int64_t)c * rb_n + rb) * 16) = o;
    se[(int64_t)c * rb_n + rb] = (uint8_t)sb;
  }
}

}  // namespace

int k_quantize_mxfp4(const void* const* x_ptrs, const void* x_single, int E, int64_t ldx, int R, int C, int in_dtype, int transpose,
                     void* q, void* s, hipStream_t st) {
  if (E <= 0 || R <= 0 || C <= 0) return CSMOE_OK;
  const int64_t q_mat = (int64_t)R * C / 2;
  const int64_t s_mat = transpose ? (int64_t)C * (R / 32) : (int64_t)R * (C / 32);
  if (!transpose) {
    const int64_t total = (int64_t)R * (C / 32);
    dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 8192), (unsigned)E), block(256);
    if (in_dtype == CSMOE_BF16)
      hipLaunchKernelGGL((quant4_rows_kernel<bf16>), grid, block, 0, st, x_ptrs, (const bf16*)x_single, ldx, R, C, (uint8_t*)q, (uint8_t*)s, q_mat, s_mat);
    else
      hipLaunchKernelGGL((quant4_rows_kernel<float>), grid, block, 0, st, x_ptrs, (const float*)x_single, ldx, R, C, (uint8_t*)q, (uint8_t*)s, q_mat, s_mat);
  } else {
    const int64_t tiles = (int64_t)(R / 32) * ((C + 63) / 64);
    dim3 grid((unsigned)std::min<int64_t>((tiles + 3) / 4, 8192), (unsigned)E), block(256);
    if (in_dtype == CSMOE_BF16)
      hipLaunchKernelGGL((quant4_cols_kernel<bf16>), grid, block, 0, st, x_ptrs, (const bf16*)x_single, ldx, R, C, (uint8_t*)q, (uint8_t*)s, q_mat, s_mat);
    else
      hipLaunchKernelGGL((quant4_cols_kernel<float>), grid, block, 0, st, x_ptrs, (const float*)x_single, ldx, R, C, (uint8_t*)q, (uint8_t*)s, q_mat, s_mat);
  }
  CSMOE_CHECK_LAUNCH("quantize_mxfp4");
  return CSMOE_OK;
}

int k_quantize_mxfp8_both(const void* const* x_ptrs, const void* x_single, int E, int64_t ldx, int R, int C, int in_dtype, void* q,
                          void* s, void* qt, void* st, hipStream_t stream) {
  if (E <= 0 || R <= 0 || C <= 0) return CSMOE_OK;
  const int64_t tiles = (int64_t)((R + QB_R - 1) / QB_R) * ((C + QB_C - 1) / QB_C);
  // one tile per workgroup where the grid allows (16 384 per expert): a persistent grid walking several tiles per workgroup with
  // the next tile prefetched measured SLOWER (2 048 workgroups 4.86 ms, 65 536 4.33 ms, one per tile 3.92 ms per 128-expert table)
  dim3 grid((unsigned)std::min<int64_t>(tiles, 16384), (unsigned)E), block(256);
  const int64_t q_mat = (int64_t)R * C, s_mat = (int64_t)R * (C / 32), st_mat = (int64_t)C * (R / 32);
  if (in_dtype == CSMOE_BF16)
    hipLaunchKernelGGL((quant_both_kernel<bf16>), grid, block, 0, stream, x_ptrs, (const bf16*)x_single, ldx, R, C, (uint8_t*)q,
                       (uint8_t*)s, (uint8_t*)qt, (uint8_t*)st, q_mat, s_mat, st_mat);
  else
    hipLaunchKernelGGL((quant_both_kernel<float>), grid, block, 0, stream, x_ptrs, (const float*)x_single, ldx, R, C, (uint8_t*)q,
                       (uint8_t*)s, (uint8_t*)qt, (uint8_t*)st, q_mat, s_mat, st_mat);
  CSMOE_CHECK_LAUNCH("quantize_mxfp8_both");
  return CSMOE_OK;
}

int k_quantize_mxfp8(const void* const* x_ptrs, const void* x_single, int E, int64_t ldx, int R, int C, int in_dtype, int transpose,
                     void* q, void* s, hipStream_t st) {
  if (E <= 0 || R <= 0 || C <= 0) return CSMOE_OK;
  const int64_t q_mat = (int64_t)R * C;
  const int64_t s_mat = transpose ? (int64_t)C * (R / 32) : (int64_t)R * (C / 32);
  if (!transpose) {
    const int64_t total = (int64_t)R * (C / 32);
    dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 8192), (unsigned)E), block(256);
    if (in_dtype == CSMOE_BF16)
      hipLaunchKernelGGL((quant_rows_kernel<bf16>), grid, block, 0, st, x_ptrs, (const bf16*)x_single, ldx, R, C, (uint8_t*)q, (uint8_t*)s, q_mat, s_mat);
    else
      hipLaunchKernelGGL((quant_rows_kernel<float>), grid, block, 0, st, x_ptrs, (const float*)x_single, ldx, R, C, (uint8_t*)q, (uint8_t*)s, q_mat, s_mat);
  } else {
    const int64_t tiles = (int64_t)(R / 32) * ((C + 63) / 64);
    dim3 grid((unsigned)std::min<int64_t>((tiles + 3) / 4, 8192), (unsigned)E), block(256);
    if (in_dtype == CSMOE_BF16)
      hipLaunchKernelGGL((quant_cols_kernel<bf16>), grid, block, 0, st, x_ptrs, (const bf16*)x_single, ldx, R, C, (uint8_t*)q, (uint8_t*)s, q_mat, s_mat);
    else
      hipLaunchKernelGGL((quant_cols_kernel<float>), grid, block, 0, st, x_ptrs, (const float*)x_single, ldx, R, C, (uint8_t*)q, (uint8_t*)s, q_mat, s_mat);
  }
  CSMOE_CHECK_LAUNCH("quantize_mxfp8");
  return CSMOE_OK;
}

int k_quantize_mxfp8_tokens(const void* x, int64_t ldx, const int32_t* offsets, int E, int C, int64_t n_pad, void* poff, void* q, void* s,
                            void* qt, void* st, hipStream_t stream) {
  hipLaunchKernelGGL(token_pad_offsets_kernel, dim3(1), dim3(256), 0, stream, offsets, E, (int32_t*)poff);
  CSMOE_CHECK_LAUNCH("quantize_mxfp8_tokens (offsets)");
  if (C <= 0 || n_pad <= 0) return CSMOE_OK;
  dim3 grid((unsigned)(n_pad / QB_R), (unsigned)((C + QB_C - 1) / QB_C)), block(256);
  if (q)
    hipLaunchKernelGGL((quant_tokens_kernel<true>), grid, block, 0, stream, (const bf16*)x, ldx, offsets, (const int32_t*)poff, E, C,
                       n_pad, (uint8_t*)q, (uint8_t*)s, (uint8_t*)qt, (uint8_t*)st);
  else
    hipLaunchKernelGGL((quant_tokens_kernel<false>), grid, block, 0, stream, (const bf16*)x, ldx, offsets, (const int32_t*)poff, E, C,
                       n_pad, (uint8_t*)q, (uint8_t*)s, (uint8_t*)qt, (uint8_t*)st);
  CSMOE_CHECK_LAUNCH("quantize_mxfp8_tokens");
  return CSMOE_OK;
}

// index = perm [n] (rows form: source row perm[m] / K) or slot_of [n * K] (tokens form: n tokens); bounds are the caller's contract,
// as for k_dispatch_rows / k_dispatch_tokens
int k_dispatch_quant_mxfp8(const void* x, const int32_t* index, int K, void* xs, void* q, void* s, int n, int D, int tokens,
                           hipStream_t st) {
  if (n == 0) return CSMOE_OK;
  dim3 grid(stride_grid(n)), block(256);
  if (tokens)
    hipLaunchKernelGGL((dispatch_quant_kernel<true>), grid, block, 0, st, (const bf16*)x, index, K, (bf16*)xs, (uint8_t*)q, (uint8_t*)s,
                       n, D);
  else
    hipLaunchKernelGGL((dispatch_quant_kernel<false>), grid, block, 0, st, (const bf16*)x, index, K, (bf16*)xs, (uint8_t*)q, (uint8_t*)s,
                       n, D);
  CSMOE_CHECK_LAUNCH(tokens ? "dispatch_tokens_mxfp8" : "dispatch_rows_mxfp8");
  return CSMOE_OK;
}
