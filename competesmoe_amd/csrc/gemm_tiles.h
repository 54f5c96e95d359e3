// Shared pieces of the bf16 grouped-GEMM kernels: argument block, buffer descriptors, the two swizzled 16 KiB LDS tile
// images (KC / KM, see gemm_bf16.hip) with their LDS-DMA fill and fragment reads, and the 8-wide activation helpers.
#pragma once
#include "common.h"

namespace ggt {

constexpr unsigned OOB = 0x80000000u;       // any offset >= num_records reads as zero
constexpr int TILE_B = 16384;               // one 128x64 (KC) / 64x128 (KM) bf16 tile image

enum { KC = 0, KM = 1 };

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((ext_vector_type(4))) short s16x4;

struct FastArgs {
  // row operand ("tokens" / wgrad A): [*, ld_r]; col operand (weights / wgrad B)
  const void* R; int64_t ld_r;
  const void* Cflat; int64_t ld_c;            // wgrad col operand (flat [M, Nb])
  const void* const* c_ptrs_in;               // row-space: per-expert weight pointers
  const void* const* bias_ptrs;
  const int32_t* offsets; int E;
  int single_M; const void* single_B; const void* single_bias; void* single_C;
  int NR;      // row-space: unused;  wgrad: Na (output rows)
  int NC;      // output columns (N or Nb)
  int Kd;      // row-space reduction length
  void* C; void* C2; const void* aux; int64_t ldc;
  void* const* out_ptrs;                      // wgrad outputs
  int epilogue, act, accumulate, out_f32;
  const int32_t* xcd_order;                   // persistent wgrad: experts dealt to XCDs (csmoe_expert_order), or null
  int tile_band;                              // persistent weight gradient: row tiles per band of the tile order (gemm_bf16_v2p.hip tile_of)
  int row_part;                               // row-space v2: which row tiles of every expert (common.h part_tiles)
  int thin_loop;                              // row-space v2: tiles of <= 128 rows take the one-phase loop
};

// the fields every row-space launch of FastArgs kernels fills (gg8_rowspace, gg4_rowspace)
inline FastArgs rowspace_args(const void* A, int64_t lda, const void* const* b_ptrs, int64_t ldb, const void* const* bias_ptrs,
                              const int32_t* offsets, int E, int M, int N, int Kd, void* C, void* C2, const void* aux, int64_t ldc,
                              int epilogue, int act, const void* single_B, const void* single_bias) {
  FastArgs p{};
  p.single_M = M; p.single_B = single_B; p.single_bias = single_bias;
  p.R = A; p.ld_r = lda; p.c_ptrs_in = b_ptrs; p.ld_c = ldb; p.bias_ptrs = bias_ptrs; p.offsets = offsets; p.E = E;
  p.NC = N; p.Kd = Kd; p.C = C; p.C2 = C2; p.aux = aux; p.ldc = ldc; p.epilogue = epilogue; p.act = act;
  return p;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// ---- scaffolding of the 256 x 256 tile kernels, shared as TEXT (macros, like the gemm_loop_*.inc K-loops): these kernels are
// sensitive to what hipcc hoists and how it allocates registers, and a macro keeps each kernel's code what it was when written in
// place (tools/kernel_isa_diff.py is the check).  In scope where they are used: smem, lane, and the names they declare.
// slot(kind, parity) = (parity * 4 + kind) * 16 KiB with kind RL=0, CL=1, CH=2, RH=3
#define SLOT(kind, tile) (smem + ((((tile) & 1) * 4 + (kind)) * TILE_B))
#define WAIT_DMA(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
// barrier A closes a phase's read/issue section (reads retired, counted DMA wait taken), barrier B its MFMA section
#define PHASE_SYNC_IN()                                \
  __builtin_amdgcn_sched_barrier(0);                   \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
  __builtin_amdgcn_s_barrier();                        \
  __builtin_amdgcn_sched_barrier(0);                   \
  __builtin_amdgcn_s_setprio(1)
#define PHASE_SYNC_OUT()                               \
  __builtin_amdgcn_s_setprio(0);                       \
  __builtin_amdgcn_sched_barrier(0);                   \
  __builtin_amdgcn_s_barrier();                        \
  __builtin_amdgcn_sched_barrier(0)
// epilogue barrier: LDS traffic only.  __syncthreads() would add s_waitcnt vmcnt(0) = a wait for the pass's own global stores (and,
// in the persistent weight gradient, for the next tile's prefetch) at every pass.
#define EPI_SYNC()                                     \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
  __builtin_amdgcn_s_barrier();                        \
  asm volatile("" ::: "memory")

// Row-space tile lookup: declares TilePos tp, this workgroup's tile; a workgroup past the last tile RETURNS from the kernel.
// WHOLE / part: grouped_find_tile.
#define FIND_TILE_OR_RETURN(tp, offsets_, E_, M_, BMt, nct_, WHOLE, part)                                              \
  TilePos tp;                                                                                                          \
  {                                                                                                                    \
    const int total = grouped_total_tiles(offsets_, E_, M_, BMt, nct_, lane, part);                                    \
    if ((int)blockIdx.x >= total) return;                                                                              \
    if (!grouped_find_tile<WHOLE>(offsets_, E_, M_, BMt, nct_, xcd_remap(blockIdx.x, total), lane, tp, part)) return;  \
  }
// the 8-wave kernels' wave-uniform e (expert), row0 / rows (the tile's rows of the row operand) and tc0 (first output column) of tp.
// (gg4_kernel and the decode kernels take `rows` from the UNIFORM row0, which compiles to other code: they keep their own lines.)
#define TILE_VARS_8W(tp, BMt, BNt)                                                                                     \
  int e = tp.e, row0 = tp.o0 + tp.mt * (BMt), rows = min(BMt, tp.o1 - row0), tc0 = tp.nt * (BNt);                      \
  e = __builtin_amdgcn_readfirstlane(e);                                                                               \
  row0 = __builtin_amdgcn_readfirstlane(row0);                                                                         \
  rows = __builtin_amdgcn_readfirstlane(rows);                                                                         \
  tc0 = __builtin_amdgcn_readfirstlane(tc0)

// LDS read addressing of the 8-wave kernels' fragments for wave (wm, wn): this lane's offset in a K-contiguous block (kc_lane, for
// frag_kc) and the wave's first 16-row / 16-column block inside an R / C image (wm*4 + 0..3, wn*2 + 0..1) ...
#define FRAG_LANE_8W(wm_, wn_)                                                                                         \
  const int g = lane >> 4, i16 = lane & 15;                                                                            \
  const int kc_lane = i16 * 128 + ((g ^ (i16 >> 1)) << 4);                                                             \
  const int q = i16 >> 2, pp = i16 & 3;                                                                                \
  const int fk = q | ((g & 1) << 2);                                                                                   \
  const int r_blk0 = (wm_) * 4, c_blk0 = (wn_) * 2;                                                                    \
  (void)kc_lane; (void)r_blk0
// ... and, for the kernels with K-major images, its offsets of the N blocks from blk0_ on (km_[], for frag_km_raw).  Declared only
// where they are read: the unused arrays changed gg8c_kernel's register allocation
#define FRAG_KM_BLOCKS(km_, N, blk0_)                                                                                  \
  int km_[N];                                                                                                          \
  _Pragma("unroll") for (int b = 0; b < N; ++b) km_[b] = (8 * g + q) * 256 + ((((blk0_) + b) ^ fk) << 5) + pp * 8

// f32x4 acc[NA][NB], zeroed
#define ZERO_ACC(acc_, NA, NB)                                                                                         \
  f32x4 acc_[NA][NB];                                                                                                  \
  _Pragma("unroll") for (int a_ = 0; a_ < NA; ++a_)                                                                    \
    _Pragma("unroll") for (int b_ = 0; b_ < NB; ++b_) acc_[a_][b_] = f32x4{0.f, 0.f, 0.f, 0.f}


// Scalar (SMEM) load of 8 bytes from a wave-uniform address (the persistent weight-gradient kernels' table reads).  Written as asm because hipcc turns a plain load of the offsets /
// pointer tables into a VECTOR load once the kernel also stores to global memory, and every use of such a load costs an
// `s_waitcnt vmcnt(0)`: a wait for the prefetch DMA and for all earlier stores of the epilogue.  The tables are written before
// the launch, so the scalar cache is coherent for them.
__device__ __forceinline__ uint64_t sload_b64(const void* ptr) {
  const uint64_t a = (uint64_t)ptr;
  const uint64_t u = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                     (unsigned)__builtin_amdgcn_readfirstlane((int)a);
  uint64_t r;
  asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(u) : "memory");
  return r;
}

// ---- LDS-DMA fill of one 16 KiB tile image: NJ wave-instructions per wave (NJ * waves = 16) ----------------------
// KC: tile rows are operand rows (stride ld_bytes), 64 reduction elements per row starting at red0.
// KM: tile rows are 64 reduction rows, 128 operand columns starting at col0.
template <int KIND, int NJ>
__device__ __forceinline__ void dma_tile(__amdgpu_buffer_rsrc_t rsrc, char* lds_tile, const unsigned (&vbase)[NJ],
                                         const int (&aux)[NJ], int red0, int red_len, unsigned ld_bytes, int wave) {
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    unsigned voff;
    if (KIND == KC) {
      voff = vbase[j] + (unsigned)red0 * 2u;            // aux[j] = first reduction element of this lane's chunk
      if (red0 + aux[j] >= red_len) voff = OOB;
    } else {
      voff = vbase[j] + (unsigned)red0 * ld_bytes;      // vbase already OOB for out-of-range columns; rows past the
    }                                                   // end of the reduction fall off num_records
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)(lds_tile + (wave * NJ + j) * 1024), 16, voff, 0, 0, 0);
  }
}

// one 1 KiB piece (wave-instruction) of an image: lets a caller interleave the NJ pieces with other work
template <int KIND, int NJ>
__device__ __forceinline__ void dma_piece(__amdgpu_buffer_rsrc_t rsrc, char* lds_tile, unsigned vbase_j, int aux_j, int j,
                                          int red0, int red_len, unsigned ld_bytes, int wave) {
  unsigned voff;
  if (KIND == KC) {
    voff = vbase_j + (unsigned)red0 * 2u;
    if (red0 + aux_j >= red_len) voff = OOB;
  } else {
    voff = vbase_j + (unsigned)red0 * ld_bytes;
  }
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void*)(lds_tile + (wave * NJ + j) * 1024), 16, voff, 0, 0, 0);
}

// per-lane, loop-invariant DMA source offsets.  Image row / column i (0..127) is fetched from source row / column
//   src(i) = (i >> gshift) * gstride + (i & ((1 << gshift) - 1)) + sub
// (identity for gshift = 7).  The v2 kernel uses it to build images out of the 64-row / 32-column strips each wave reads in
// one phase.
template <int KIND, int NJ>
__device__ __forceinline__ void dma_setup(unsigned (&vbase)[NJ], int (&aux)[NJ], unsigned ld_bytes, int col0, int ncols,
                                          int gshift, int gstride, int sub, int wave, int lane) {
  const int gmask = (1 << gshift) - 1;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    int P = (wave * NJ + j) * 64 + lane;
    if (KIND == KC) {
      int r = P >> 3, pc = P & 7;
      int c = pc ^ ((r >> 1) & 7);
      int src = (r >> gshift) * gstride + (r & gmask) + sub;
      vbase[j] = (unsigned)src * ld_bytes + (unsigned)c * 16u;
      aux[j] = c * 8;
    } else {
      int k = P >> 4, pc = P & 15;
      int f = (k & 3) | (((k >> 3) & 1) << 2);
      int seg = (pc >> 1) ^ f;
      int ic = seg * 16 + (pc & 1) * 8;
      int col = col0 + (ic >> gshift) * gstride + (ic & gmask) + sub;
      vbase[j] = (col < ncols) ? ((unsigned)k * ld_bytes + (unsigned)col * 2u) : OOB;
      aux[j] = 0;
    }
  }
}

// ---- the decode kernels (gemm_skinny.hip, gemm_skinny_mx.hip): the NW waves' partial 16 x SLAB tiles (acc[NB]) meet in LDS at
// red_ (NW tiles of 16 rows x LDW floats) ...
#define SKINNY_STORE_PARTIAL(red_, acc_)                                                                               \
  {                                                                                                                    \
    float* red = (red_) + wave * (16 * LDW);                                                                           \
    _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) *(f32x4*)(red + i16 * LDW + nb * 16 + 4 * g) = acc_[nb];         \
  }                                                                                                                    \
  __syncthreads()
// ... and thread (r_, cg_) of the epilogue sums its 8 columns into float v_[8] in wave order 0..7: the one summation order of every run
#define SKINNY_SUM_PARTIALS(v_, red_, r_, cg_)                                                                         \
  float v_[8];                                                                                                         \
  {                                                                                                                    \
    const float* red = (red_) + (r_) * LDW + (cg_) * 8;                                                                \
    const f32x4 lo = *(const f32x4*)red, hi = *(const f32x4*)(red + 4);                                                \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) { v_[j] = lo[j]; v_[4 + j] = hi[j]; }                                \
    _Pragma("unroll") for (int w = 1; w < NW; ++w) {                                                                   \
      const f32x4 l2 = *(const f32x4*)(red + w * 16 * LDW), h2 = *(const f32x4*)(red + w * 16 * LDW + 4);              \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) { v_[j] += l2[j]; v_[4 + j] += h2[j]; }                            \
    }                                                                                                                  \
  }

// ---- fragment reads ------------------------------------------------------------------------------------------------
// KC: block b = 16 operand rows; returns the 8 reduction elements k = s*32 + 8*(lane>>4) .. +7 of row (lane&15)
__device__ __forceinline__ bf16x8 frag_kc(const char* tile, int lane_off, int b, int s) {
  return *(const bf16x8*)(tile + b * 2048 + (lane_off ^ (s << 6)));
}
// KM: column block cb; two transposed 4x16 reads
__device__ __forceinline__ bf16x8 frag_km(const char* tile, int addr_cb, int s) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + addr_cb + s * 8192));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + addr_cb + s * 8192 + 1024));
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

// Same fragment by inline asm, for the hand-scheduled v2 loops.  hipcc's waitcnt pass cannot tell which LDS bytes a pending
// LDS-DMA (buffer_load ... lds) will write and puts `s_waitcnt vmcnt(0)` in front of every ds_read_b64_tr_b16 builtin: that
// drained the whole prefetch queue twice per K-tile in every kernel with a K-major image (profiles/r01).  The asm form is
// invisible to that pass; the CALLER owns the ordering: the counted vmcnt + s_barrier before the slot is read, and
// `s_waitcnt lgkmcnt(0)` before the first use of the result (PHASE_SYNC_IN does both).
__device__ __forceinline__ unsigned lds_addr(const char* p) {
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const char*)p;
}
__device__ __forceinline__ bf16x8 frag_km_raw(const char* tile, int addr_cb, int s) {
  const unsigned a = lds_addr(tile) + (unsigned)addr_cb;
  i32x2 lo, hi;
  if (s == 0) {
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a) : "memory");
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(hi) : "v"(a) : "memory");
  } else {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:8192" : "=v"(lo) : "v"(a) : "memory");
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:9216" : "=v"(hi) : "v"(a) : "memory");
  }
  i32x4 v = {lo[0], lo[1], hi[0], hi[1]};
  return __builtin_bit_cast(bf16x8, v);
}

// ---- fast GELU for the bf16 epilogues -------------------------------------------------------------------------------------
// erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, far below half a bf16 ulp), one v_exp + one v_rcp: the OCML erff costs
// ~50 instructions and made the bias+GELU epilogue ~30 % of a K=4096 tile (profiles/r01).  The fp32 path (gemm_generic.hip)
// keeps the exact erff.
// Both formulas (GELU and its derivative) over 8 values as 4 pairs, written on 2-vectors so that the multiplies / adds / FMAs become packed fp32
// instructions (v_pk_mul_f32, v_pk_add_f32, v_pk_fma_f32: two elements per issue slot); v_rcp_f32 / v_exp_f32 stay per element.
// Per tile of the bias+GELU epilogue this arithmetic was ~15 us of a 134 us tile (tools/tile_stamps.py): VALU-bound, no MFMA beside it.
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x2 pk_splat(float c) { return f32x2{c, c}; }
// erf(z) for a pair; e_out = exp(-z*z)
__device__ __forceinline__ f32x2 erf_as2(f32x2 z, f32x2& e_out) {
  const f32x2 az = {fabsf(z[0]), fabsf(z[1])};
  const f32x2 d = pk_fma(pk_splat(0.3275911f), az, pk_splat(1.f));
  const f32x2 t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
  const f32x2 a2 = (az * az) * pk_splat(-1.44269504088896340736f);           // -z^2 * log2(e)
  const f32x2 e = {__builtin_amdgcn_exp2f(a2[0]), __builtin_amdgcn_exp2f(a2[1])};
  f32x2 p = pk_fma(pk_splat(1.061405429f), t, pk_splat(-1.453152027f));
  p = pk_fma(p, t, pk_splat(1.421413741f));
  p = pk_fma(p, t, pk_splat(-0.284496736f));
  p = pk_fma(p, t, pk_splat(0.254829592f));
  const f32x2 r = pk_fma(-(p * t), e, pk_splat(1.f));
  e_out = e;
  return f32x2{copysignf(r[0], z[0]), copysignf(r[1], z[1])};
}
__device__ __forceinline__ void gelu_fast8(float (&v)[8]) {
#ifdef CSMOE_EPI_NOMATH     // timing experiment (wrong results): what the GELU arithmetic of the epilogues costs
  return;
#endif
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f32x2 x = {v[2 * k], v[2 * k + 1]};
    f32x2 e;
    const f32x2 erf = erf_as2(x * pk_splat(0.70710678118654752440f), e);
    const f32x2 y = (x * pk_splat(0.5f)) * (erf + pk_splat(1.f));
    v[2 * k] = y[0]; v[2 * k + 1] = y[1];
  }
}
__device__ __forceinline__ void gelu_grad_fast8(float (&h)[8]) {
#ifdef CSMOE_EPI_NOMATH
  return;
#endif
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f32x2 x = {h[2 * k], h[2 * k + 1]};
    f32x2 e;   // exp(-x^2/2)
    const f32x2 erf = erf_as2(x * pk_splat(0.70710678118654752440f), e);
    const f32x2 cdf = pk_fma(erf, pk_splat(0.5f), pk_splat(0.5f));
    const f32x2 y = pk_fma(x * pk_splat(0.39894228040143267794f), e, cdf);
    h[2 * k] = y[0]; h[2 * k + 1] = y[1];
  }
}

// activation over 8 values, `switch` outside the element loop so each formula is emitted once
__device__ __forceinline__ void act_fwd8(float (&v)[8], int act) {
  switch (act) {
    case CSMOE_ACT_RELU:
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = act_fwd(v[j], CSMOE_ACT_RELU);
      break;
    case CSMOE_ACT_GELU:
      gelu_fast8(v);
      break;
    case CSMOE_ACT_GELU_TANH:
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = act_fwd(v[j], CSMOE_ACT_GELU_TANH);
      break;
    case CSMOE_ACT_SILU:
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = act_fwd(v[j], CSMOE_ACT_SILU);
      break;
    case CSMOE_ACT_QUICK_GELU:
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = quick_gelu_rounded<bf16>(v[j]);
      break;
    default: break;
  }
}
// h[j] <- act'(h[j])
__device__ __forceinline__ void act_bwd8(float (&h)[8], int act) {
  switch (act) {
    case CSMOE_ACT_RELU:
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = act_bwd(h[j], CSMOE_ACT_RELU);
      break;
    case CSMOE_ACT_GELU:
      gelu_grad_fast8(h);
      break;
    case CSMOE_ACT_GELU_TANH:
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = act_bwd(h[j], CSMOE_ACT_GELU_TANH);
      break;
    case CSMOE_ACT_SILU:
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = act_bwd(h[j], CSMOE_ACT_SILU);
      break;
    case CSMOE_ACT_QUICK_GELU:
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = quick_gelu_grad_rounded<bf16>(h[j]);
      break;
    default:
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = 1.f;
      break;
  }
}

}  // namespace ggt
