// Row-space grouped GEMM for FEW rows with MXFP8 operands (decode on the fp8 experts of BASELINE config 5), for gfx950 (MI355X):
// C[m, 0:N] = epilogue(sum_k dq(A)[src(m), k] dq(B_e)[n, k]), OCP e4m3 elements with one e8m0 scale per 32 elements along k, on
// v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulate, bf16 outputs.  Forward epilogues only.  gemm_skinny.hip's weight streamer
// (kernel guide, GEMM staging table, row "GEMV / M <= 16 decode weights") at half the weight bytes: every weight byte is loaded once
// per 16-row block, 16 bytes per lane straight into VGPRs, U K-steps in flight per wave (below).  The fp8 layer's forward tables are
// [N, Kd] with scales [N, Kd/32] (K-contiguous: _quantize_weight_both's forward half), which is the fragment as stored: no LDS image,
// one weight layout.  No counterpart upstream (the reference has no fp8).
//
// Decomposition (gemm_skinny.hip's).  One workgroup of 8 waves per (16-row block of one expert, slab of 16 * NB output columns).  The
// 8 waves deal the K range among themselves in contiguous runs of 128-element K-steps (wave w: steps [w * per, (w + 1) * per)), one
// MFMA per step and 16-column block; each keeps NB fp32 accumulator tiles.  The partial tiles meet in LDS and are summed in wave
// order 0..7 by the threads that run the epilogue: a fixed order, no atomics, bit-identical from run to run.  Blocks of the grid past
// the last tile (the host sizes it from an upper bound of the number of row blocks: the counts stay on the device) find that out from
// the offsets and return; experts without rows own no tile.
//
// Fragments (the instruction's own k order, gemm_fp8.hip's header, measured with tools/probes/mfma_scale_probe.hip): lane
// (i = l & 15, g = l >> 4) holds k = 16 g .. 16 g + 15 of its row in registers 0-3 and k = 64 + 16 g .. + 15 in registers 4-7 -- two
// 16-byte loads of one row per K-step -- and supplies the scale byte of block g (k = 32 g .. 32 g + 31) of that row.  A row's 4
// scale bytes of a K-step are one word, and the unrolled loop loads the words of its U steps at once: one load per row.
// MFMA roles are swapped as in the other kernels: the weights feed the A input (rows = output columns n), the token rows the B input,
// so lane (g, i) ends with columns n0 + 4 g .. + 3 of row i.  With `src_rows` the token row is src_rows[m] / src_div, for the
// elements AND the scales (quantisation is per row: quantise-then-gather is gather-then-quantise).
//
// Loads in flight.  The unrolled loop issues the loads of U K-steps -- U * (2 NB + 2) 16-byte loads and NB + 1 scale-word loads:
// 18 + 3 for the 32-column slab (U = 3), 20 + 5 for the 64-column slab (U = 2) -- and a __builtin_amdgcn_sched_barrier keeps the
// MFMAs behind all of them: left to itself hipcc sinks each load next to its MFMA and waits vmcnt(0) in every iteration, about one
// K-step in flight.  As compiled (-save-temps): the 21 / 25 loads, then counted waits vmcnt(14), 12, 8, 6, 2, 0 / vmcnt(16), 14,
// 12, 10, 6, 4, 2, 0, one MFMA behind each.  Nothing is carried over from one iteration to the next (no software pipeline): each
// ends at vmcnt(0).  U is what 128 VGPRs hold (two 8-wave workgroups per CU, asked for by the launch bounds); the weight and scale
// addresses are 32-bit offsets from the expert's wave-uniform bases to stay inside that.
//
// Bounds (nothing outside the operands is read, nothing outside this expert's rows x [0, N) is written):
//   * lanes i >= rows of a partial block take row0's row index instead (row0 < offsets[e + 1] <= M always holds: a tile exists only
//     for a non-empty block), so src_rows[] is read at m in [row0, offsets[e + 1]) only and A / As at rows the caller named;
//   * weight rows n >= N are clamped to N - 1, elements and scales alike: in bounds, and the columns they feed are never stored;
//   * Kd % 128 == 0: every K-step is whole, a lane's two 16-byte pieces end at k0 + 64 + 16 g + 16 <= Kd and its scale byte is
//     k0 / 32 + g < Kd / 32;
//   * the epilogue runs on threads (r, cg), r < 16: all of them read the LDS tile (in range) and take part in the shuffles, but only
//     those with r < rows and n0 + 8 cg < N load a bias or store: 8 columns of C / C2 / Cq at n0 + 8 cg .. + 7 < N (N % 8 == 0) of
//     row row0 + r < offsets[e + 1], and, from one thread in four, the byte Cs[row0 + r][(n0 + 8 cg) / 32] < N / 32.  With Cq the
//     host requires N % 32 == 0 and the slab is a multiple of 32 wide, so the four threads of a 32-column block are in one
//     workgroup, adjacent, in one row, and all inside or all outside [0, N).
//
// Epilogue (gemm_skinny_mx_epilogue.inc, one copy for this kernel and gemm_skinny_fp4.hip; the argument block is gemm_skinny_mx.h's)
// = the non-gradient branch of gemm_epilogue.h at the same rounding points as csmoe_grouped_gemm_mxfp8 (the product plus
// bias is rounded to bf16, the activation sees the rounded value and is rounded again), 8 columns per thread through act_fwd8,
// 16-byte stores.  Optional fused MXFP8 output (BIAS_ACT): Cq / Cs take the MX quantisation of the bf16-ROUNDED activated output,
// blocks along N, byte for byte what csmoe_quantize_mxfp8(transpose = 0) writes for C2 (the scale-and-convert code is mx_quant.h's,
// shared with that quantiser; the block amax is two shuffles among the block's four threads, as in dispatch_quant_kernel: fmaxf
// drops a NaN operand, so the order of the maxima does not matter).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 everywhere):
//   kernel <NB>   VGPRs  AGPRs  SGPRs  LDS bytes / block  scratch  occupancy (waves / SIMD)
//   <2>             107      0     74             18,432        0                         4
//   <4>             126      0     74             34,816        0                         4
// (a workgroup is 2 waves per SIMD: two workgroups are resident per CU.)
#include "gemm_skinny_mx.h"

namespace {

struct Frag8 { i32x4 lo, hi; int sc; };      // one row's 32 k-bytes of a K-step in the MFMA's k order, and its block's scale byte

__device__ __forceinline__ i32x8 join8(const Frag8& f) {
  return i32x8{f.lo[0], f.lo[1], f.lo[2], f.lo[3], f.hi[0], f.hi[1], f.hi[2], f.hi[3]};
}

template <int NB>
__global__ void __launch_bounds__(NW * 64, 4) skinny8_kernel(Skinny8Args p) {
  constexpr int SLAB = 16 * NB;                       // output columns per workgroup
  constexpr int LDW = SLAB + 4;                       // floats per row of a wave's partial tile
  constexpr int U = NB == 2 ? 3 : 2;                  // K-steps whose loads a wave issues before it waits for the first
  static_assert(NB == 2 || NB == 4, "a 32-column block of the quantised output lies inside one slab");
  __shared__ __attribute__((aligned(16))) float red_s[NW * 16 * LDW];

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
  const uint8_t* pa = p.A + srow * p.lda + 16 * g;
  const uint8_t* psa = p.AS + srow * p.ldas + g;
  const gbyte* wq = (const gbyte*)p.bq_ptrs[e];        // global address space stated: pointers read from a table are generic otherwise
  const gbyte* ws = (const gbyte*)p.bs_ptrs[e];
  // the expert's bases are wave-uniform (scalar registers); a lane keeps 32-bit offsets (N * ldb < 2 GiB: the shape rule)
  unsigned ob[NB], osb[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const unsigned wrow = (unsigned)min(n0 + nb * 16 + i16, p.N - 1);
    ob[nb] = wrow * (unsigned)p.ldb + 16 * g;
    osb[nb] = wrow * (unsigned)p.ldbs;                 // the row's scale words; the lane's byte is g
  }

  // ---------------- this wave's K-steps ----------------
  const int nst = p.Kd >> 7;
  const int per = (nst + NW - 1) / NW;
  const int s0 = min(wave * per, nst), s1 = min(s0 + per, nst);

  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // elements of one K-step (two 16-byte pieces per row); `sc`: also the scale bytes, one byte load per row
  auto load = [&](int s, Frag8& fa, Frag8 (&fb)[NB], bool sc) {
    fa.lo = *(const i32x4*)(pa + s * 128);
    fa.hi = *(const i32x4*)(pa + s * 128 + 64);
    if (sc) fa.sc = psa[s * 4];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      fb[nb].lo = *(const gi32x4*)(wq + (ob[nb] + s * 128));
      fb[nb].hi = *(const gi32x4*)(wq + (ob[nb] + s * 128 + 64));
      if (sc) fb[nb].sc = ws[osb[nb] + s * 4 + g];
    }
  };
  auto step = [&](const Frag8& fa, const Frag8 (&fb)[NB]) {
    const i32x8 ra = join8(fa);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      acc[nb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(join8(fb[nb]), ra, acc[nb], 0, 0, 0, fb[nb].sc, 0, fa.sc);
  };

  // U steps at a time.  Their 4 U scale bytes of a row are consecutive: ONE load per row (4-byte aligned: ldas % 4 == 0, 4 bytes per
  // step) instead of U byte loads, and the lane takes byte g of step u's word.  The barrier keeps every MFMA behind every load of
  // the iteration (header: loads in flight)
  typedef unsigned scale_words __attribute__((ext_vector_type(U), aligned(4)));
  typedef __attribute__((address_space(1))) scale_words gscale_words;
  int s = s0;
  for (; s + U <= s1; s += U) {
    Frag8 fa[U], fb[U][NB];
    const scale_words wa = *(const scale_words*)(psa - g + s * 4);
    scale_words wb[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) wb[nb] = *(const gscale_words*)(ws + (osb[nb] + s * 4));
#pragma unroll
    for (int u = 0; u < U; ++u) load(s + u, fa[u], fb[u], false);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      fa[u].sc = (int)((wa[u] >> (8 * g)) & 0xffu);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) fb[u][nb].sc = (int)((wb[nb][u] >> (8 * g)) & 0xffu);
      step(fa[u], fb[u]);
    }
  }
  for (; s < s1; ++s) {
    Frag8 fa, fb[NB];
    load(s, fa, fb, true);
    step(fa, fb);
  }

  // ---------------- the 8 partial tiles meet in LDS ----------------
  SKINNY_STORE_PARTIAL(red_s, acc);

  // ---------------- epilogue: thread (r, cg) owns 8 columns of one row; whole waves past the 16 rows leave ----------------
#include "gemm_skinny_mx_epilogue.inc"
}

}  // namespace

// the shape rule without the pointers (a pure host query)
bool gg_skinny8_shape_ok(int64_t lda, int64_t ldas, int64_t ldb, int64_t ldbs, int64_t ldc, int64_t ldcq, int64_t ldcs, int M, int N,
                         int Kd, int quant_out) {
  if (N < 8 || Kd < 128 || Kd % 128 || N % 8 || lda % 16 || ldb % 16 || ldas % 4 || ldbs % 4 || ldc % 8) return false;
  if (quant_out && (N % 32 || ldcq % 8)) return false;      // 8-byte stores to Cq, byte stores to Cs
  if ((int64_t)M * lda >= (int64_t)OOB) return false;
  if ((int64_t)N * ldb >= (int64_t)OOB) return false;
  return true;
}

int gg_skinny8_rowspace(const void* Aq, int64_t lda, const void* As, int64_t ldas, const int32_t* src_rows, int src_div,
                        const void* const* bq_ptrs, const void* const* bs_ptrs, int64_t ldb, int64_t ldbs,
                        const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd, void* C, void* C2,
                        int64_t ldc, void* Cq, void* Cs, int64_t ldcq, int64_t ldcs, int epilogue, int act, hipStream_t st) {
  Skinny8Args p{};
  p.A = (const uint8_t*)Aq; p.lda = lda; p.AS = (const uint8_t*)As; p.ldas = ldas;
  p.src_rows = src_rows; p.src_div = src_rows ? src_div : 1;
  p.bq_ptrs = bq_ptrs; p.bs_ptrs = bs_ptrs; p.ldb = ldb; p.ldbs = ldbs; p.bias_ptrs = bias_ptrs;
  p.offsets = offsets; p.E = E; p.M = M; p.N = N; p.Kd = Kd;
  p.C = (bf16*)C; p.C2 = (bf16*)C2; p.ldc = ldc; p.Cq = (uint8_t*)Cq; p.Cs = (uint8_t*)Cs; p.ldcq = ldcq; p.ldcs = ldcs;
  p.epilogue = epilogue; p.act = act;
  const int64_t nrb = skinny_row_blocks(M, E);
  // the 64-column slab (half the token-row loads per weight byte) once it still gives two workgroups per CU; 32 columns below that
  const bool wide = nrb * ((N + 63) / 64) >= 512;
  const int slab = wide ? 64 : 32;
  unsigned grid;
  const int rc = grid_1d("grouped_gemm_skinny_mxfp8", nrb * ((N + slab - 1) / slab), &grid);
  if (rc || !grid) return rc;
  const dim3 gr(grid), bl(NW * 64);
  if (wide) hipLaunchKernelGGL((skinny8_kernel<4>), gr, bl, 0, st, p);
  else hipLaunchKernelGGL((skinny8_kernel<2>), gr, bl, 0, st, p);
  CSMOE_CHECK_LAUNCH("grouped_gemm_skinny_mxfp8");
  return CSMOE_OK;
}
