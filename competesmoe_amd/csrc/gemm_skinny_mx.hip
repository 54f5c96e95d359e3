// Row-space grouped GEMM for FEW rows with MXFP8 token rows and MX weight tables (decode on the fp8 experts of BASELINE config 5), for
// gfx950 (MI355X): C[m, 0:N] = epilogue(sum_k dq(A)[src(m), k] dq(B_e)[n, k]), one e8m0 scale per 32 elements along k on both sides,
// on v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulate, bf16 outputs.  Forward epilogues only.  ONE kernel text for two weight
// formats (the descriptors W8 / W4 below):
//   * W8, MXFP8 weights (csmoe_grouped_gemm_skinny_mxfp8): OCP e4m3 on both inputs (cbsz 0, blgp 0).  gemm_skinny.hip's weight
//     streamer (kernel guide, GEMM staging table, row "GEMV / M <= 16 decode weights") at half the weight bytes.  The fp8 layer's
//     forward tables are [N, Kd] with scales [N, Kd/32] (K-contiguous: _quantize_weight_both's forward half), which is the fragment
//     as stored: no LDS image, one weight layout;
//   * W4, MXFP4 weights, W4A8 (csmoe_grouped_gemm_skinny_mxfp4w): A = e4m3 token rows, B_e = OCP e2m1 weights packed two per byte
//     (cbsz 4: the A input is FP4; blgp 0: the B input is e4m3): the W8 streamer at 0.516 of its weight bytes (0.5 + 1/32 per
//     element against 1 + 1/32).  The table is [N, Kd / 2] bytes in natural k order (byte j of a row = element 2 j in the low nibble,
//     2 j + 1 in the high nibble) with scales [N, Kd / 32]: what csmoe_quantize_mxfp4(transpose != 0) writes for a master [Kd, N].
// Every weight byte is loaded once per 16-row block, 16 bytes per lane straight into VGPRs, U K-steps in flight per wave (below).
// ldb counts BYTES of a weight row (Kd for e4m3, Kd / 2 for packed e2m1).  No counterpart upstream (the reference has no fp8 and no
// fp4).
//
// Decomposition (gemm_skinny.hip's; FIND_TILE_OR_RETURN, SKINNY_STORE_PARTIAL, SKINNY_SUM_PARTIALS are gemm_tiles.h's).  One
// workgroup of 8 waves per (16-row block of one expert, slab of 16 * NB output columns).  The 8 waves deal the K range among
// themselves in contiguous runs of 128-element K-steps (wave w: steps [w * per, (w + 1) * per)), one MFMA per step and 16-column
// block; each keeps NB fp32 accumulator tiles.  The partial tiles meet in LDS and are summed in wave order 0..7 by the threads that
// run the epilogue: a fixed order, no atomics, bit-identical from run to run.  Blocks of the grid past the last tile (the host sizes
// it from an upper bound of the number of row blocks: the counts stay on the device) find that out from the offsets and return;
// experts without rows own no tile.
//
// Fragments (the instruction's own k order; k named by the e4m3 side).  The two inputs of one instruction may disagree on which k a
// lane holds, and each is loaded its own way:
//   * e4m3 (the token rows, B input, next to either weight format; the W8 weights, A input: gemm_fp8.hip's header, measured with
//     tools/probes/mfma_scale_probe.hip): lane (i = l & 15, g = l >> 4) holds k = 16 g .. 16 g + 15 of its row in registers 0-3 and
//     k = 64 + 16 g .. + 15 in registers 4-7 -- two 16-byte loads of one row per K-step (128 bytes per row and step) -- and supplies
//     the scale byte of block g (k = 32 g .. 32 g + 31) of that row;
//   * e2m1 (the W4 weights, A input; measured with tools/probes/mfma_scale_fp4_probe.hip on an MI355X, exact integer data): lane
//     (i, g) holds k = 32 g .. 32 g + 31 of its row in its four registers, register r nibble n (bits 4 n .. 4 n + 3) =
//     k 32 g + 8 r + n: the low nibble is the lower k, and a lane's 32 k are 16 consecutive bytes of the natural-order table -- ONE
//     16-byte load per row and K-step (64 bytes per row and step; the four lane groups read them side by side).  This is NOT the e4m3
//     layout (two runs of 16 k, 64 apart).  Lane group g supplies the scale byte of block g (k = 32 g .. 32 g + 31) of its row: the
//     scale it supplies covers exactly the 32 k it holds (established by tests/test_skinny_fp4_contract_gpu.py, whose scales differ
//     per row and per k-block and which is bit-exact only with this assignment; the probe's second table prints the same question
//     directly).
// A row's 4 scale bytes of a K-step are one word, and the unrolled loop loads the words of its U steps at once: one load per row.
// MFMA roles are swapped as in the other kernels: the weights feed the A input (rows = output columns n), the token rows the B input,
// so lane (g, i) ends with columns n0 + 4 g .. + 3 of row i.  With `src_rows` the token row is src_rows[m] / src_div, for the
// elements AND the scales (quantisation is per row: quantise-then-gather is gather-then-quantise).
//
// Loads in flight and unroll depth U.  The unrolled loop issues the loads of U K-steps and NB + 1 scale-word loads, and a
// __builtin_amdgcn_sched_barrier keeps the MFMAs behind all of them: left to itself hipcc sinks each load next to its MFMA and waits
// vmcnt(0) in every iteration, about one K-step in flight.  Nothing is carried over from one iteration to the next (no software
// pipeline): each ends at vmcnt(0).  U is what 128 VGPRs hold (two 8-wave workgroups per CU, asked for by the launch bounds); the
// weight and scale addresses are 32-bit offsets from the expert's wave-uniform bases to stay inside that.  A K-step costs a lane 8
// registers of token row and 8 NB (W8) / 4 NB (W4) of weights, and its loads are 2 + 2 NB (W8) / 2 + NB (W4) of 16 bytes.  Fragment
// registers of U steps:
//   W8:  NB = 2:  24 U   -> U = 3: 72;    NB = 4:  40 U   -> U = 2: 80
//   W4:  NB = 2:  16 U   -> U = 4: 64;    NB = 4:  24 U   -> U = 3: 72
// plus 4 NB accumulators, (NB + 1) U scale words and 2 NB row offsets (W4: 96 / 111 before addressing; one step more, U = 5 / 4:
// 112 / 135, does not fit).  16-byte + scale-word loads of an iteration: W8 18 + 3 / 20 + 5, W4 16 + 3 / 18 + 5.
//
// Slab rule (skinny_mx_wide: the 64-column slab, NB = 4, from W::WIDE_FROM workgroups of it on; 32 columns, NB = 2, below that, where
// the narrow slab's larger grid is what fills the chip).  W8: the 64-column slab (half the token-row loads per weight byte) once it
// still gives two workgroups per CU: 512.  W4: on the 32-column slab HALF of a lane's loaded bytes are token rows (L2 hits that
// still take load slots), on the 64-column slab a third, so the wide slab pays earlier than for fp8 weights; and a workgroup of the
// wide slab keeps 8 waves x 12 weight loads x 1 KiB = 96 KiB of weights in flight, three times what one CU's share of 8 TB/s needs
// at 1 us of latency (31 KiB), so ONE resident workgroup per CU already covers the latency: 256.
//
// Bounds (nothing outside the operands is read, nothing outside this expert's rows x [0, N) is written):
//   * lanes i >= rows of a partial block take row0's row index instead (row0 < offsets[e + 1] <= M always holds: a tile exists only
//     for a non-empty block), so src_rows[] is read at m in [row0, offsets[e + 1]) only and A / As at rows the caller named;
//   * weight rows n >= N are clamped to N - 1, elements and scales alike: in bounds, and the columns they feed are never stored;
//   * Kd % 128 == 0: every K-step is whole.  An e4m3 lane's two 16-byte pieces end at k0 + 64 + 16 g + 16 <= Kd (<= ldb for W8
//     weights) and its scale byte is k0 / 32 + g < Kd / 32; a W4 weight lane's bytes end at (k0 + 128) / 2 <= Kd / 2 <= ldb and its
//     scale byte is k0 / 32 + g < Kd / 32 <= ldbs;
//   * the 32-bit weight offsets stay below N * ldb < 2 GiB (shape rule); the unrolled loop's scale-word load covers the 4 U scale
//     bytes of steps s .. s + U - 1 < nst: bytes [4 s, 4 (s + U)) of a row of Kd / 32 = 4 nst bytes;
//   * the epilogue runs on threads (r, cg), r < 16: all of them read the LDS tile (in range) and take part in the shuffles, but only
//     those with r < rows and n0 + 8 cg < N load a bias or store: 8 columns of C / C2 / Cq at n0 + 8 cg .. + 7 < N (N % 8 == 0) of
//     row row0 + r < offsets[e + 1], and, from one thread in four, the byte Cs[row0 + r][(n0 + 8 cg) / 32] < N / 32.  With Cq the
//     host requires N % 32 == 0 and the slab is a multiple of 32 wide, so the four threads of a 32-column block are in one
//     workgroup, adjacent, in one row, and all inside or all outside [0, N).
//
// Epilogue = the non-gradient branch of gemm_epilogue.h at the same rounding points as csmoe_grouped_gemm_mxfp8 (the product plus
// bias is rounded to bf16, the activation sees the rounded value and is rounded again), 8 columns per thread through act_fwd8,
// 16-byte stores.  Optional fused MXFP8 output (BIAS_ACT): Cq / Cs take the MX quantisation of the bf16-ROUNDED activated output,
// blocks along N, byte for byte what csmoe_quantize_mxfp8(transpose = 0) writes for C2 (the scale-and-convert code is mx_quant.h's,
// shared with that quantiser; the block amax is two shuffles among the block's four threads, as in dispatch_quant_kernel: fmaxf
// drops a NaN operand, so the order of the maxima does not matter).
//
// Non-finite W4 weights do not exist in a table (e2m1 has no encodings for them; the quantiser's header says what they become); a
// NaN or an inf in a token row behaves the same next to either weight format.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 everywhere):
//   kernel <W, NB>   U  VGPRs  AGPRs  SGPRs  LDS bytes / block  scratch  occupancy (waves / SIMD)
//   <W8, 2>          3    107      0     74             18,432        0                         4
//   <W8, 4>          2    126      0     74             34,816        0                         4
//   <W4, 2>          4    104      0     74             18,432        0                         4
//   <W4, 4>          3    126      0     74             34,816        0                         4
// (a workgroup is 2 waves per SIMD: two workgroups are resident per CU.)  As compiled (-save-temps / -S), the unrolled iteration:
//   <W8, 2>  21 loads, then counted waits vmcnt(14), 12, 8, 6, 2, 0, one MFMA behind each
//   <W8, 4>  25 loads, then vmcnt(16), 14, 12, 10, 6, 4, 2, 0
//   <W4, 2>  19 loads (16 of elements, 3 scale-word loads of 16 bytes), then vmcnt(13), 12, 9, 8, 5, 4, 1, 0
//   <W4, 4>  23 loads (18 of elements, 5 scale-word loads of 12 bytes), then vmcnt(15), 14, 13, 12, 9, 8, 7, 6, 3, 2, 1, 0
// The four instantiations are instruction for instruction what the two separate units of this kernel compiled to
// (tools/kernel_isa_diff.py --units).  That holds only while the weight load keeps its per-format arithmetic (`load` below): forming
// the pointer first and adding 64 to it, or routing the load through a member function of the descriptor, changes the W8 code.
#include "gemm_tiles.h"
#include "mx_quant.h"
#include <algorithm>

using namespace ggt;

namespace {

constexpr int NW = 8;      // waves per workgroup (the K range of a tile is dealt to them)

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((address_space(1))) uint8_t gbyte;
typedef __attribute__((address_space(1))) i32x4 gi32x4;

struct SkinnyMxArgs {
  const uint8_t* A; int64_t lda; const uint8_t* AS; int64_t ldas; const int32_t* src_rows; int src_div;
  const void* const* bq_ptrs; const void* const* bs_ptrs; int64_t ldb, ldbs; const void* const* bias_ptrs;
  const int32_t* offsets; int E, M, N, Kd;
  bf16* C; bf16* C2; int64_t ldc; uint8_t* Cq; uint8_t* Cs; int64_t ldcq, ldcs; int epilogue, act;
};

struct FragA { i32x4 lo, hi; int sc; };      // a token row's 32 k-bytes of a K-step (e4m3) in the MFMA's k order, and its scale byte

__device__ __forceinline__ i32x8 join_a(const FragA& f) {
  return i32x8{f.lo[0], f.lo[1], f.lo[2], f.lo[3], f.hi[0], f.hi[1], f.hi[2], f.hi[3]};
}

// The weight formats: a row's fragment of a K-step and its scale byte, the MFMA's view of it, elements per byte (common.h's
// SkinnyMxFmt names the entry of each: its tag and Kd / ldb), bytes per row and K-step, the MFMA's cbsz, the unroll depth for
// NB = 2 / 4 and the slab switch (header)
struct W8 {
  struct Frag { i32x4 lo, hi; int sc; };     // 32 k-bytes (e4m3) in the MFMA's k order
  static __device__ __forceinline__ i32x8 join(const Frag& f) {
    return i32x8{f.lo[0], f.lo[1], f.lo[2], f.lo[3], f.hi[0], f.hi[1], f.hi[2], f.hi[3]};
  }
  static constexpr int K_PER_BYTE = 1, STEP_BYTES = 128 / K_PER_BYTE, CBSZ = 0, U2 = 3, U4 = 2, WIDE_FROM = 512;
};
struct W4 {
  struct Frag { i32x4 q; int sc; };          // 32 k-nibbles (e2m1)
  static __device__ __forceinline__ i32x8 join(const Frag& f) {   // the instruction reads the first four registers of an FP4 operand
    return i32x8{f.q[0], f.q[1], f.q[2], f.q[3], 0, 0, 0, 0};
  }
  static constexpr int K_PER_BYTE = 2, STEP_BYTES = 128 / K_PER_BYTE, CBSZ = 4, U2 = 4, U4 = 3, WIDE_FROM = 256;
};

template <class W, int NB>
__global__ void __launch_bounds__(NW * 64, 4) skinny_mx_kernel(SkinnyMxArgs p) {
  using FragW = typename W::Frag;
  constexpr int SLAB = 16 * NB;                       // output columns per workgroup
  constexpr int LDW = SLAB + 4;                       // floats per row of a wave's partial tile
  constexpr int U = NB == 2 ? W::U2 : W::U4;          // K-steps whose loads a wave issues before it waits for the first (header)
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
    ob[nb] = wrow * (unsigned)p.ldb + 16 * g;          // the lane's first 16 bytes of a step (W4: its only ones, k = 32 g .. 32 g + 31)
    osb[nb] = wrow * (unsigned)p.ldbs;                 // the row's scale words; the lane's byte is g
  }

  // ---------------- this wave's K-steps ----------------
  const int nst = p.Kd >> 7;
  const int per = (nst + NW - 1) / NW;
  const int s0 = min(wave * per, nst), s1 = min(s0 + per, nst);

  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // elements of one K-step (e4m3 row: two 16-byte pieces; e2m1 row: one); `sc`: also the scale bytes, one byte load per row.  The
  // weight offsets are written out per format: this arithmetic is what reproduces the compiled code (header, last paragraph)
  auto load = [&](int s, FragA& fa, FragW (&fb)[NB], bool sc) {
    fa.lo = *(const i32x4*)(pa + s * 128);
    fa.hi = *(const i32x4*)(pa + s * 128 + 64);
    if (sc) fa.sc = psa[s * 4];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if constexpr (W::STEP_BYTES == 128) {
        fb[nb].lo = *(const gi32x4*)(wq + (ob[nb] + s * 128));
        fb[nb].hi = *(const gi32x4*)(wq + (ob[nb] + s * 128 + 64));
      } else {
        fb[nb].q = *(const gi32x4*)(wq + (ob[nb] + s * 64));
      }
      if (sc) fb[nb].sc = ws[osb[nb] + s * 4 + g];
    }
  };
  auto step = [&](const FragA& fa, const FragW (&fb)[NB]) {
    const i32x8 ra = join_a(fa);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      acc[nb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(W::join(fb[nb]), ra, acc[nb], W::CBSZ, /*blgp: e4m3*/ 0, 0,
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
  constexpr int CPR = 2 * NB;                         // epilogue threads (8 columns each) per row
  if (threadIdx.x >= 16 * CPR) return;
  const int r = threadIdx.x / CPR, cg = threadIdx.x % CPR;
  const int ncol = n0 + cg * 8;
  const bool live = r < rows && ncol < p.N;           // the others stay for the shuffles only
  SKINNY_SUM_PARTIALS(v, red_s, r, cg);
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (p.epilogue != CSMOE_EPI_PLAIN && live) {
    const void* bias = p.bias_ptrs ? p.bias_ptrs[e] : nullptr;
    if (bias) {
      const bf16x8 b8 = *(const bf16x8*)((const bf16*)bias + ncol);
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = (float)b8[j];
    }
  }
  const int64_t o = (int64_t)(row0 + r) * p.ldc + ncol;
  bf16x8 o0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { o0[j] = (bf16)(v[j] + bv[j]); v[j] = (float)o0[j]; }
  if (p.C && live) *(bf16x8*)(p.C + o) = o0;
  if (p.epilogue != CSMOE_EPI_BIAS_ACT || !(p.C2 || p.Cq)) return;
  act_fwd8(v, p.act);
  bf16x8 o1;
#pragma unroll
  for (int j = 0; j < 8; ++j) o1[j] = (bf16)v[j];
  if (p.C2 && live) *(bf16x8*)(p.C2 + o) = o1;
  if (p.Cq) {                                         // wave-uniform; every thread of the wave is still here
    float f[8];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { f[j] = (float)o1[j]; amax = fmaxf(amax, fabsf(f[j])); }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    const int sb = e8m0_of_amax(amax);
    const float inv = inv_scale_of(sb);
    u32x2 q;
    q[0] = pack4_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
    q[1] = pack4_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
    if (live) {
      *(u32x2*)(p.Cq + (int64_t)(row0 + r) * p.ldcq + ncol) = q;
      if ((cg & 3) == 0) p.Cs[(int64_t)(row0 + r) * p.ldcs + (ncol >> 5)] = (uint8_t)sb;
    }
  }
}

// true if a launch of this shape takes the 64-column slab (header: slab rule)
template <class W>
bool skinny_mx_wide(int M, int N, int E) { return skinny_row_blocks(M, E) * ((N + 63) / 64) >= W::WIDE_FROM; }

template <class W>
int skinny_mx_launch(const char* tag, const SkinnyMxArgs& p, hipStream_t st) {
  const bool wide = skinny_mx_wide<W>(p.M, p.N, p.E);
  const int slab = wide ? 64 : 32;
  unsigned grid;
  const int rc = grid_1d(tag, skinny_row_blocks(p.M, p.E) * ((p.N + slab - 1) / slab), &grid);
  if (rc || !grid) return rc;
  const dim3 gr(grid), bl(NW * 64);
  if (wide) hipLaunchKernelGGL((skinny_mx_kernel<W, 4>), gr, bl, 0, st, p);
  else hipLaunchKernelGGL((skinny_mx_kernel<W, 2>), gr, bl, 0, st, p);
  CSMOE_CHECK_LAUNCH(tag);
  return CSMOE_OK;
}

}  // namespace

// the shape rule without the pointers (a pure host query), the same for both formats; ldb in bytes of a weight row
bool gg_skinny_mx_shape_ok(int64_t lda, int64_t ldas, int64_t ldb, int64_t ldbs, int64_t ldc, int64_t ldcq, int64_t ldcs, int M, int N,
                           int Kd, int quant_out) {
  if (N < 8 || Kd < 128 || Kd % 128 || N % 8 || lda % 16 || ldb % 16 || ldas % 4 || ldbs % 4 || ldc % 8) return false;
  if (quant_out && (N % 32 || ldcq % 8)) return false;      // 8-byte stores to Cq, byte stores to Cs
  if ((int64_t)M * lda >= (int64_t)OOB) return false;
  if ((int64_t)N * ldb >= (int64_t)OOB) return false;
  return true;
}

int gg_skinny_mx_rowspace(const SkinnyMxFmt& fmt, const void* Aq, int64_t lda, const void* As, int64_t ldas, const int32_t* src_rows,
                          int src_div, const void* const* bq_ptrs, const void* const* bs_ptrs, int64_t ldb, int64_t ldbs,
                          const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd, void* C, void* C2,
                          int64_t ldc, void* Cq, void* Cs, int64_t ldcq, int64_t ldcs, int epilogue, int act, hipStream_t st) {
  SkinnyMxArgs p{};
  p.A = (const uint8_t*)Aq; p.lda = lda; p.AS = (const uint8_t*)As; p.ldas = ldas;
  p.src_rows = src_rows; p.src_div = src_rows ? src_div : 1;
  p.bq_ptrs = bq_ptrs; p.bs_ptrs = bs_ptrs; p.ldb = ldb; p.ldbs = ldbs; p.bias_ptrs = bias_ptrs;
  p.offsets = offsets; p.E = E; p.M = M; p.N = N; p.Kd = Kd;
  p.C = (bf16*)C; p.C2 = (bf16*)C2; p.ldc = ldc; p.Cq = (uint8_t*)Cq; p.Cs = (uint8_t*)Cs; p.ldcq = ldcq; p.ldcs = ldcs;
  p.epilogue = epilogue; p.act = act;
  return fmt.k_per_byte == W4::K_PER_BYTE ? skinny_mx_launch<W4>(fmt.tag, p, st) : skinny_mx_launch<W8>(fmt.tag, p, st);
}
