// Row-space grouped GEMM for FEW rows with MXFP4 WEIGHTS and MXFP8 activations (W4A8 decode on the fp8 experts), for gfx950 (MI355X):
// C[m, 0:N] = epilogue(sum_k dq(A)[src(m), k] dq(B_e)[n, k]); A = OCP e4m3 token rows, B_e = OCP e2m1 weights packed two per byte,
// both with one e8m0 scale per 32 elements along k, on v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz 4: the A input is FP4; blgp 0: the
// B input is e4m3), fp32 accumulate, bf16 outputs.  Forward epilogues only.  gemm_skinny_fp8.hip's weight streamer at 0.516 of its
// weight bytes (0.5 + 1/32 per element against 1 + 1/32).  The table is [N, Kd / 2] bytes in natural k order (byte j of a row =
// element 2 j in the low nibble, 2 j + 1 in the high nibble) with scales [N, Kd / 32]: what csmoe_quantize_mxfp4(transpose != 0)
// writes for a master [Kd, N].  No counterpart upstream (the reference has no fp8 and no fp4).
//
// Decomposition, gather, epilogue: gemm_skinny_fp8.hip's, shared through gemm_skinny_mx.h (argument block), gemm_skinny_mx_epilogue.inc (epilogue with the
// fused MXFP8 output) and gemm_tiles.h (FIND_TILE_OR_RETURN, SKINNY_STORE_PARTIAL, SKINNY_SUM_PARTIALS).  One workgroup of 8 waves per
// (16-row block of one expert, slab of 16 * NB output columns); the waves deal the 128-element K-steps among themselves in
// contiguous runs, one MFMA per step and 16-column block; the partial tiles are summed in LDS in wave order 0..7: no atomics,
// bit-identical from run to run.
//
// Fragments (measured with tools/probes/mfma_scale_fp4_probe.hip on an MI355X, exact integer data; k named by the e4m3 side):
//   * FP4 side (the weights, A input): lane (i = l & 15, g = l >> 4) holds k = 32 g .. 32 g + 31 of its row in its four registers,
//     register r nibble n (bits 4 n .. 4 n + 3) = k 32 g + 8 r + n: the low nibble is the lower k, and a lane's 32 k are 16
//     consecutive bytes of the natural-order table -- ONE 16-byte load per row and K-step (64 bytes per row and step; the four lane
//     groups read them side by side).  This is NOT the e4m3 layout (two runs of 16 k, 64 apart): the two inputs of one instruction
//     disagree on which k a lane holds, and each is loaded its own way;
//   * the FP4 lane group g supplies the scale byte of block g (k = 32 g .. 32 g + 31) of its row: the scale it supplies covers
//     exactly the 32 k it holds (established by tests/test_skinny_fp4_contract_gpu.py, whose scales differ per row and per k-block
//     and which is bit-exact only with this assignment; the probe's second table prints the same question directly);
//   * e4m3 side (the token rows, B input), next to an FP4 A input: as in gemm_skinny_fp8.hip -- k = 16 g .. + 15 in registers 0-3,
//     k = 64 + 16 g .. + 15 in registers 4-7, scale byte of block g -- two 16-byte loads per row and K-step.
// A row's 4 scale bytes of a K-step are one word, and the unrolled loop loads the words of its U steps at once: one load per row.
// MFMA roles as in the other kernels: the weights feed the A input (rows = output columns n), the token rows the B input, so lane
// (g, i) ends with columns n0 + 4 g .. + 3 of row i.
//
// Loads in flight, unroll depth and slab rule, re-derived for the halved weight operand.  A K-step costs a lane 8 registers of token
// row and 4 NB of weights (fp8: 8 + 8 NB), and its loads are 2 + NB of 16 bytes (fp8: 2 + 2 NB).  Fragment registers of U steps:
//   NB = 2:  16 U   -> U = 4: 64 (fp8 kernel: 72 at U = 3);   NB = 4:  24 U   -> U = 3: 72 (fp8 kernel: 80 at U = 2)
// plus 4 NB accumulators, (NB + 1) U scale words and 2 NB row offsets: 96 / 111 before addressing, inside the 128 VGPRs that two
// 8-wave workgroups per CU allow (launch bounds); one step more (U = 5 / 4: 112 / 135) does not fit.  The unrolled loop issues
// U (2 + NB) 16-byte loads and NB + 1 scale-word loads (16 + 3 / 18 + 5) and a __builtin_amdgcn_sched_barrier keeps the MFMAs
// behind all of them, as in the fp8 kernel.  Slab: on the 32-column slab HALF of a lane's loaded bytes are token rows (L2 hits that
// still take load slots), on the 64-column slab a third, so the wide slab pays earlier than for fp8 weights; and a workgroup of the
// wide slab keeps 8 waves x 12 weight loads x 1 KiB = 96 KiB of weights in flight, three times what one CU's share of 8 TB/s needs
// at 1 us of latency (31 KiB), so ONE resident workgroup per CU already covers the latency: the 64-column slab from 256 workgroups
// on (fp8 kernel: 512), 32 columns below that, where the narrow slab's larger grid is what fills the chip.
//
// Bounds (nothing outside the operands is read, nothing outside this expert's rows x [0, N) is written):
//   * lanes i >= rows of a partial block take row0's row index instead (row0 < offsets[e + 1] <= M always holds: a tile exists only
//     for a non-empty block), so src_rows[] is read at m in [row0, offsets[e + 1]) only and A / As at rows the caller named;
//   * weight rows n >= N are clamped to N - 1, elements and scales alike: in bounds, and the columns they feed are never stored;
//   * Kd % 128 == 0: every K-step is whole.  A token lane's two 16-byte pieces end at k0 + 64 + 16 g + 16 <= Kd and its scale byte
//     is k0 / 32 + g < Kd / 32; a weight lane's bytes end at (k0 + 128) / 2 <= Kd / 2 <= ldb (below) and its scale byte is
//     k0 / 32 + g < Kd / 32 <= ldbs;
//   * the 32-bit weight offsets stay below N * ldb < 2 GiB (shape rule); the unrolled loop's scale-word load covers the 4 U scale
//     bytes of steps s .. s + U - 1 < nst: bytes [4 s, 4 (s + U)) of a row of Kd / 32 = 4 nst bytes;
//   * the epilogue (gemm_skinny_mx_epilogue.inc) stores 8 columns of C / C2 / Cq at n0 + 8 cg .. + 7 < N of row row0 + r < offsets[e + 1]
//     from threads with r < rows and n0 + 8 cg < N only, and the byte Cs[row0 + r][(n0 + 8 cg) / 32] from one thread in four.
//
// Non-finite weights do not exist in a table (e2m1 has no encodings for them; the quantiser's header says what they become); a NaN
// or an inf in a token row behaves as in the fp8 kernel.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 everywhere):
//   kernel <NB>   U  VGPRs  AGPRs  SGPRs  LDS bytes / block  scratch  occupancy (waves / SIMD)
//   <2>           4    104      0     74             18,432        0                         4
//   <4>           3    126      0     74             34,816        0                         4
// (a workgroup is 2 waves per SIMD: two workgroups are resident per CU.)  As compiled (-S): the unrolled iteration is 19 loads
// (16 of elements, 3 scale-word loads of 16 bytes) then vmcnt(13), 12, 9, 8, 5, 4, 1, 0 with one MFMA behind each on the narrow
// slab; 23 loads (18 of elements, 5 scale-word loads of 12 bytes) then vmcnt(15), 14, 13, 12, 9, 8, 7, 6, 3, 2, 1, 0 on the wide.
#include "gemm_skinny_mx.h"

namespace {

struct FragA { i32x4 lo, hi; int sc; };      // a token row's 32 k-bytes of a K-step (e4m3) in the MFMA's k order, and its scale byte
struct FragW { i32x4 q; int sc; };           // a weight row's 32 k-nibbles of a K-step (e2m1), and its scale byte

__device__ __forceinline__ i32x8 join_a(const FragA& f) {
  return i32x8{f.lo[0], f.lo[1], f.lo[2], f.lo[3], f.hi[0], f.hi[1], f.hi[2], f.hi[3]};
}
__device__ __forceinline__ i32x8 join_w(const FragW& f) {       // the instruction reads the first four registers of an FP4 operand
  return i32x8{f.q[0], f.q[1], f.q[2], f.q[3], 0, 0, 0, 0};
}

template <int NB>
__global__ void __launch_bounds__(NW * 64, 4) skinny4w_kernel(Skinny8Args p) {
  constexpr int SLAB = 16 * NB;                       // output columns per workgroup
  constexpr int LDW = SLAB + 4;                       // floats per row of a wave's partial tile
  constexpr int U = NB == 2 ? 4 : 3;                  // K-steps whose loads a wave issues before it waits for the first (header)
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
    ob[nb] = wrow * (unsigned)p.ldb + 16 * g;          // the lane's 32 k of a step are 16 consecutive bytes: k = 32 g .. 32 g + 31
    osb[nb] = wrow * (unsigned)p.ldbs;                 // the row's scale words; the lane's byte is g
  }

  // ---------------- this wave's K-steps ----------------
  const int nst = p.Kd >> 7;
  const int per = (nst + NW - 1) / NW;
  const int s0 = min(wave * per, nst), s1 = min(s0 + per, nst);

  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // elements of one K-step (token row: two 16-byte pieces; weight row: one, 64 bytes per row and step); `sc`: also the scale bytes
  auto load = [&](int s, FragA& fa, FragW (&fb)[NB], bool sc) {
    fa.lo = *(const i32x4*)(pa + s * 128);
    fa.hi = *(const i32x4*)(pa + s * 128 + 64);
    if (sc) fa.sc = psa[s * 4];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      fb[nb].q = *(const gi32x4*)(wq + (ob[nb] + s * 64));
      if (sc) fb[nb].sc = ws[osb[nb] + s * 4 + g];
    }
  };
  auto step = [&](const FragA& fa, const FragW (&fb)[NB]) {
    const i32x8 ra = join_a(fa);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      acc[nb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(join_w(fb[nb]), ra, acc[nb], /*cbsz: fp4*/ 4, /*blgp: e4m3*/ 0, 0,
                                                                 fb[nb].sc, 0, fa.sc);
  };

  // U steps at a time.  Their 4 U scale bytes of a row are consecutive: ONE load per row (4-byte aligned: ldas, ldbs % 4 == 0, 4 bytes
  // per step) instead of U byte loads, and the lane takes byte g of step u's word.  The barrier keeps every MFMA behind every load of
  // the iteration (header: loads in flight)
  typedef unsigned scale_words __attribute__((ext_vector_type(U), aligned(4)));
  typedef __attribute__((address_space(1))) scale_words gscale_words;
  int s = s0;
  for (; s + U <= s1; s += U) {
    FragA fa[U];
    FragW fb[U][NB];
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
    FragA fa;
    FragW fb[NB];
    load(s, fa, fb, true);
    step(fa, fb);
  }

  // ---------------- the 8 partial tiles meet in LDS ----------------
  SKINNY_STORE_PARTIAL(red_s, acc);

  // ---------------- epilogue: thread (r, cg) owns 8 columns of one row; whole waves past the 16 rows leave ----------------
#include "gemm_skinny_mx_epilogue.inc"
}

}  // namespace

// the shape rule without the pointers (a pure host query); ldb in bytes of a packed weight row
bool gg_skinny4w_shape_ok(int64_t lda, int64_t ldas, int64_t ldb, int64_t ldbs, int64_t ldc, int64_t ldcq, int64_t ldcs, int M, int N,
                          int Kd, int quant_out) {
  if (N < 8 || Kd < 128 || Kd % 128 || N % 8 || lda % 16 || ldb % 16 || ldas % 4 || ldbs % 4 || ldc % 8) return false;
  if (quant_out && (N % 32 || ldcq % 8)) return false;      // 8-byte stores to Cq, byte stores to Cs
  if ((int64_t)M * lda >= (int64_t)OOB) return false;
  if ((int64_t)N * ldb >= (int64_t)OOB) return false;
  return true;
}

// 1 if a launch of this shape takes the 64-column slab (header: slab rule)
static int gg_skinny4w_wide(int M, int N, int E) { return skinny_row_blocks(M, E) * ((N + 63) / 64) >= 256 ? 1 : 0; }

int gg_skinny4w_rowspace(const void* Aq, int64_t lda, const void* As, int64_t ldas, const int32_t* src_rows, int src_div,
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
  const bool wide = gg_skinny4w_wide(M, N, E) != 0;
  const int slab = wide ? 64 : 32;
  unsigned grid;
  const int rc = grid_1d("grouped_gemm_skinny_mxfp4w", nrb * ((N + slab - 1) / slab), &grid);
  if (rc || !grid) return rc;
  const dim3 gr(grid), bl(NW * 64);
  if (wide) hipLaunchKernelGGL((skinny4w_kernel<4>), gr, bl, 0, st, p);
  else hipLaunchKernelGGL((skinny4w_kernel<2>), gr, bl, 0, st, p);
  CSMOE_CHECK_LAUNCH("grouped_gemm_skinny_mxfp4w");
  return CSMOE_OK;
}
