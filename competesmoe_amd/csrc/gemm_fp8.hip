// Grouped expert GEMM on the block-scaled fp8 matrix pipe of gfx950 (BASELINE config 5): C[m, :] = epilogue(sum_k A[m,k] B_e[n,k])
// with MXFP8 operands -- OCP e4m3 elements, one e8m0 scale per 32 elements along k -- on `v_mfma_scale_f32_16x16x128_f8f6f4`
// (2x the bf16 rate, dequantisation fused into the instruction), fp32 accumulators, bf16 outputs through the same epilogues as the
// bf16 kernel.  No counterpart upstream (the reference has no fp8).
//
// Structure = the 256x256, 8-wave, two-phase ("BAL") loop of gemm_bf16_v2.hip, byte for byte: a K-tile is 128 fp8 elements = the
// same 128-byte image rows as 64 bf16, so the LDS-DMA fill, the source-side swizzle, the four image kinds (RL / RH / CL / CH), the
// counted vmcnt discipline and the half-phase stagger carry over unchanged.  What differs:
//   * a fragment is 32 k-bytes of one row in the instruction's own k order, measured with tools/probes/mfma_scale_probe.hip: lane l
//     (row l & 15, group g = l >> 4) holds k = 16 g .. 16 g + 15 in its first four registers and k = 64 + 16 g .. + 15 in the last
//     four -- the SAME two 16-byte chunks (g, g + 4) the bf16 kernel reads for its two K = 32 steps -- and the scale of the
//     32-element block b (k = 32 b .. 32 b + 31) is taken from the lanes of group b;
//   * one K = 128 MFMA per (column block, row block) and K-tile instead of two K = 32 ones: 16 per phase at 32 cycles each;
//   * the e8m0 scales travel by LDS-DMA too (4 bytes per row and K-tile: one 256-byte wave-instruction per wave and K-tile --
//     waves 0-3 the 256 row scales, waves 4-7 the 256 column scales), are read as bytes in phase A and handed to the MFMA as
//     per-lane scale operands (lane l supplies the scale of ITS 32-element block).
#include "gemm_epilogue_q.h"
#include <algorithm>

using namespace ggt;

namespace {

constexpr int BM8 = 256, BN8 = 256;
constexpr int SC_OFF = 8 * TILE_B;                       // scale slots behind the 8 image slots: 2 x (1 KiB rows + 1 KiB columns)
constexpr int LDS8_BYTES = SC_OFF + 4096;                // 8 image slots + the scale slots behind them
static_assert(LDS8_BYTES >= EPI_LDS_BYTES, "the epilogue's staging tile overlays the operand images");

typedef __attribute__((ext_vector_type(8))) int i32x8;

struct Fp8Args {
  const uint8_t* R; int64_t ld_r;                 // A elements [M, Kd]
  const uint8_t* RS; int64_t ld_rs;               // A scales   [M, Kd/32]
  const void* const* c_ptrs; const void* const* cs_ptrs; int64_t ld_c, ld_cs;     // per-expert B [N, Kd], scales [N, Kd/32]
  const void* single_B; const void* single_BS;
  const void* const* bias_ptrs; const void* single_bias;
  const int32_t* offsets; int E; int single_M;
  int NC, Kd;
  void* C; void* C2; const void* aux; int64_t ldc;
  int epilogue, act;
};

__global__ void __launch_bounds__(512, 2) gg8f_kernel(Fp8Args p) {
#include "gemm_fp8_tile.inc"

  // ---------------- epilogue: the bf16 kernels' (gemm_epilogue.h) ----------------
  const EpiArgs ea{p.C, p.C2, p.aux, p.bias_ptrs ? p.bias_ptrs[e] : p.single_bias, p.ldc, p.epilogue, p.act, p.NC};
  rowspace_epilogue(ea, acc, smem, row0, rows, tc0, wm, wn, lane);
}

// The same tile with the quantised activated output of gemm_epilogue_q.h (CSMOE_EPI_BIAS_ACT only): a kernel of its own, so that
// gg8f_kernel's arguments, registers and code stay what they are for every launch without Cq / Cs.
struct Fp8QArgs {
  Fp8Args a;
  uint8_t* Cq; uint8_t* Cs; int64_t ldcq, ldcs;    // [M, N] e4m3, [M, N/32] e8m0
};

__global__ void __launch_bounds__(512, 2) gg8fq_kernel(Fp8QArgs pq) {
  const Fp8Args& p = pq.a;
#include "gemm_fp8_tile.inc"

  const EpiArgs ea{p.C, p.C2, nullptr, p.bias_ptrs ? p.bias_ptrs[e] : p.single_bias, p.ldc, CSMOE_EPI_BIAS_ACT, p.act, p.NC};
  const EpiQArgs eq{pq.Cq, pq.Cs, pq.ldcq, pq.ldcs};
  rowspace_epilogue_q(ea, eq, acc, smem, row0, rows, tc0, wm, wn, lane);
}

}  // namespace

int gg8f_rowspace(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* const* bq_ptrs, const void* const* bs_ptrs,
                  int64_t ldb, int64_t ldbs, const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd,
                  void* C, void* C2, const void* aux, int64_t ldc, int epilogue, int act, const void* single_B,
                  const void* single_BS, const void* single_bias, hipStream_t st) {
  Fp8Args p{};
  p.R = (const uint8_t*)Aq; p.ld_r = lda; p.RS = (const uint8_t*)As; p.ld_rs = ldas;
  p.c_ptrs = bq_ptrs; p.cs_ptrs = bs_ptrs; p.ld_c = ldb; p.ld_cs = ldbs; p.single_B = single_B; p.single_BS = single_BS;
  p.bias_ptrs = bias_ptrs; p.single_bias = single_bias; p.offsets = offsets; p.E = E; p.single_M = M;
  p.NC = N; p.Kd = Kd; p.C = C; p.C2 = C2; p.aux = aux; p.ldc = ldc; p.epilogue = epilogue; p.act = act;
  unsigned grid;
  int rc = grid_1d("grouped_gemm_mxfp8", rowspace_tiles(M, E, N, BM8, BN8), &grid);
  if (rc || !grid) return rc;
  if ((rc = set_dyn_lds<gg8f_kernel, LDS8_BYTES>())) return rc;
  hipLaunchKernelGGL(gg8f_kernel, dim3(grid), dim3(512), LDS8_BYTES, st, p);
  CSMOE_CHECK_LAUNCH("grouped_gemm_mxfp8");
  return CSMOE_OK;
}

// gg8f_rowspace with Cq [M, ldcq] / Cs [M, ldcs] next to (or instead of) C / C2: CSMOE_EPI_BIAS_ACT, N % 32 == 0 (the caller's checks)
int gg8f_rowspace_q(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* const* bq_ptrs, const void* const* bs_ptrs,
                    int64_t ldb, int64_t ldbs, const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd,
                    void* C, void* C2, int64_t ldc, void* Cq, int64_t ldcq, void* Cs, int64_t ldcs, int act, const void* single_B,
                    const void* single_BS, const void* single_bias, hipStream_t st) {
  Fp8QArgs pq{};
  Fp8Args& p = pq.a;
  p.R = (const uint8_t*)Aq; p.ld_r = lda; p.RS = (const uint8_t*)As; p.ld_rs = ldas;
  p.c_ptrs = bq_ptrs; p.cs_ptrs = bs_ptrs; p.ld_c = ldb; p.ld_cs = ldbs; p.single_B = single_B; p.single_BS = single_BS;
  p.bias_ptrs = bias_ptrs; p.single_bias = single_bias; p.offsets = offsets; p.E = E; p.single_M = M;
  p.NC = N; p.Kd = Kd; p.C = C; p.C2 = C2; p.aux = nullptr; p.ldc = ldc; p.epilogue = CSMOE_EPI_BIAS_ACT; p.act = act;
  pq.Cq = (uint8_t*)Cq; pq.Cs = (uint8_t*)Cs; pq.ldcq = ldcq; pq.ldcs = ldcs;
  unsigned grid;
  int rc = grid_1d("grouped_gemm_mxfp8_q", rowspace_tiles(M, E, N, BM8, BN8), &grid);
  if (rc || !grid) return rc;
  if ((rc = set_dyn_lds<gg8fq_kernel, LDS8_BYTES>())) return rc;
  hipLaunchKernelGGL(gg8fq_kernel, dim3(grid), dim3(512), LDS8_BYTES, st, pq);
  CSMOE_CHECK_LAUNCH("grouped_gemm_mxfp8_q");
  return CSMOE_OK;
}

// ==================================================================================================== MXFP8 weight gradient
// dW_e [Na, Nb] = sum_{k in [poff[e], poff[e+1])} At[:, k] Bt[:, k] for every expert e, both operands token-dim quantised by
// csmoe_quantize_mxfp8_tokens: At [Na, n_pad] / Bt [Nb, n_pad] e4m3, contiguous along k, scales [., n_pad/32], every expert's k range
// a multiple of 128 long and zero-padded, so that a K-tile never mixes two experts and the last one needs no masking.  An NT
// product with a K range per tile, assembled from two kernels the project already has:
//   * the K-loop, fragments, scale DMA and MFMA of gg8f_kernel above, unchanged (one text: gemm_loop_fp8.inc; the A operand takes the place of the token rows,
//     the B operand that of the weight rows; the operand and scale descriptors start at the expert's first k);
//   * the persistent tile walk of gg8w_kernel (gemm_bf16_v2p.hip): one workgroup per CU walks its XCD's contiguous chunk of the
//     expert-major tile order, or the experts dealt to its XCD (`xcd_order`), in bands of row tiles, and its store epilogue
//     (fp32: one 1-KiB row segment per store instruction; bf16: 16-byte row pieces; non-temporal; optional accumulate).
// Not carried over: gg8w's prefetch of the next tile's K-tile 0 during the epilogue (its staging tile would overlap this kernel's
// scale slots); every tile starts with its own DMA prologue.
namespace {

struct Fp8WArgs {
  const uint8_t* A; int64_t ld_a; const uint8_t* AS; int64_t ld_as;     // At [Na, *], scales [Na, */32]
  const uint8_t* B; int64_t ld_b; const uint8_t* BS; int64_t ld_bs;     // Bt [Nb, *], scales [Nb, */32]
  const int32_t* poff; int E; int NR, NC;
  void* const* out_ptrs; int64_t ldc; int accumulate, out_f32;
  const int32_t* xcd_order; int tile_band;
};

constexpr int CT8_LD = BN8 + 4;                  // fp32 staging row stride (floats): 64 rows x 1040 B
static_assert(64 * CT8_LD * 4 <= LDS8_BYTES, "the staging tile overlays the operand images");

__global__ void __launch_bounds__(512, 2) gg8wf_kernel(Fp8WArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nct = (p.NC + BN8 - 1) / BN8;
  const int nrt = (p.NR + BM8 - 1) / BM8;
  const int per_e = nrt * nct;
  const int total = per_e * p.E;
  int v_begin, v_end, v_step;
  if (p.xcd_order) {                             // experts dealt to the XCDs by row count (gg8w_kernel)
    const int x = blockIdx.x & 7, slots = (p.E + 7) >> 3;
    const int last_pos = ((slots - 1) & 1) ? 7 - x : x;
    const int n_mine = slots - 1 + (8 * (slots - 1) + last_pos < p.E ? 1 : 0);
    v_begin = blockIdx.x >> 3; v_end = n_mine * per_e; v_step = gridDim.x >> 3;
  } else if ((gridDim.x & 7) == 0) {             // one contiguous chunk of the tile order per XCD
    const int x = blockIdx.x & 7, q8 = total >> 3, r8 = total & 7;
    const int cs = (x < r8) ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8;
    v_begin = cs + (blockIdx.x >> 3); v_end = cs + q8 + (x < r8 ? 1 : 0); v_step = gridDim.x >> 3;
  } else {
    v_begin = blockIdx.x; v_end = total; v_step = gridDim.x;
  }
  const unsigned ldr_b = (unsigned)p.ld_a, ldc_b = (unsigned)p.ld_b;
  const unsigned ldrs = (unsigned)p.ld_as, ldcs = (unsigned)p.ld_bs;

  for (int v = v_begin; v < v_end; v += v_step) {
    // thread-id derived values pinned inside the iteration (gg8w_kernel: left visible, hipcc hoists them across the loop and spills)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    __builtin_assume(tid >= 0 && tid < 512);
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;

    // ---------------- tile: expert, k range, output row / column tile ----------------
    int e = v / per_e;
    const int local = v - e * per_e;
    if (p.xcd_order) e = (int)(unsigned)sload_b64(p.xcd_order + (blockIdx.x & 7) * ((p.E + 7) >> 3) + e);
    const uint64_t oo = sload_b64(p.poff + e);    // poff[e], poff[e + 1]
    const int k0 = __builtin_amdgcn_readfirstlane((int)(unsigned)oo);
    const int kd = __builtin_amdgcn_readfirstlane((int)(unsigned)(oo >> 32) - k0);
    e = __builtin_amdgcn_readfirstlane(e);
    const int band = p.tile_band;
    const int grp = local / (band * nct), rem = local - grp * band * nct;
    const int g_eff = min(band, nrt - grp * band);
    const int tr0 = __builtin_amdgcn_readfirstlane((grp * band + rem % g_eff) * BM8);
    const int tc0 = __builtin_amdgcn_readfirstlane((rem / g_eff) * BN8);
    const int rows = min(BM8, p.NR - tr0), ncols = min(BN8, p.NC - tc0);
    const int red_len = kd >> 1;                 // in the DMA helpers' 2-byte units
    const unsigned nsb = (unsigned)(kd >> 5);

    __amdgpu_buffer_rsrc_t rs_r, rs_c, rs_rs, rs_cs;
    unsigned vb_rl[2], vb_rh[2], vb_cl[2], vb_ch[2];
    int ax_r[2], ax_c[2], ax_dummy[2];
    rs_r = make_rsrc(p.A + (int64_t)tr0 * ldr_b + k0, (unsigned)rows * ldr_b);
    dma_setup<KC, 2>(vb_rl, ax_r, ldr_b, 0, 0, 7, 0, 0, wave, lane);
    dma_setup<KC, 2>(vb_rh, ax_dummy, ldr_b, 0, 0, 7, 0, 128, wave, lane);
    rs_c = make_rsrc(p.B + (int64_t)tc0 * ldc_b + k0, (unsigned)ncols * ldc_b);
    dma_setup<KC, 2>(vb_cl, ax_c, ldc_b, 0, 0, 7, 0, 0, wave, lane);
    dma_setup<KC, 2>(vb_ch, ax_dummy, ldc_b, 0, 0, 7, 0, 128, wave, lane);
    rs_rs = make_rsrc(p.AS + (int64_t)tr0 * ldrs + (k0 >> 5), (unsigned)rows * ldrs);
    rs_cs = make_rsrc(p.BS + (int64_t)tc0 * ldcs + (k0 >> 5), (unsigned)ncols * ldcs);
    const bool sc_rows = wave < 4;
    const unsigned sc_vbase = (unsigned)((wave & 3) * 64 + lane) * (sc_rows ? ldrs : ldcs);

    const int g = lane >> 4, i16 = lane & 15;
    const int sw = (i16 >> 1) & 7;
    const int f_lo = i16 * 128 + ((g ^ sw) << 4);
    const int f_hi = i16 * 128 + (((g + 4) ^ sw) << 4);
    const int r_blk0 = wm * 4, c_blk0 = wn * 2;

    ZERO_ACC(acc, 4, 8);

    const int nk = kd >> 7;
    const int rows_here = rows - wm * 64;
    const int cols_here = ncols - wn * 32;
    const bool rlo = rows_here > 0, rhi = rows_here > 128, clo = cols_here > 0, chi = cols_here > 128;

    // ---------------- K-loop: gg8f_kernel's (SLOT / ISSUE_* / FRAG / MFMA8 as defined there) ----------------
#include "gemm_loop_fp8.inc"
    // the zero-fill DMAs of the K-tiles past the end may still be writing LDS: drain before the staging tile overlays the slots
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // ---------------- epilogue: four passes of 64 rows through an fp32 tile (gg8w_kernel's) ----------------
    // pass (h, u): row blocks 4h + 2u + {0,1} of every wave -> staging row wm*32 + i*16 + (lane & 15)
    //              = tile row h*128 + wm*64 + u*32 + i*16 + (lane & 15)
    float* stg = (float*)smem;
    typedef __attribute__((address_space(1))) char gchar;
    typedef __attribute__((address_space(1))) f32x4 gf32x4;
    typedef __attribute__((address_space(1))) bf16x8 gbf16x8;
    gchar* Ce = (gchar*)(char*)sload_b64(p.out_ptrs + e);
    const int nrows = p.NR - tr0;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int h = pass >> 1, u = pass & 1;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int m = wm * 32 + i * 16 + i16;
          const int n = (cb >> 1) * 128 + wn * 32 + (cb & 1) * 16 + 4 * g;
          *(f32x4*)(stg + m * CT8_LD + n) = acc[cb][4 * h + 2 * u + i];
        }
      EPI_SYNC();
      if (p.out_f32) {
        // one store instruction = one 1-KiB row segment (64 lanes x 16 B)
        const int ec4 = lane * 4, er8 = wave;
        f32x4 rw[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) rw[j] = *(const f32x4*)(stg + (er8 + 8 * j) * CT8_LD + ec4);
        if (tc0 + ec4 < p.NC) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int r = er8 + 8 * j;
            const int trow = h * 128 + (r >> 5) * 64 + u * 32 + (r & 31);
            if (trow < nrows) {
              gf32x4* dst = (gf32x4*)(Ce + ((int64_t)(tr0 + trow) * p.ldc + tc0 + ec4) * 4);
              f32x4 a = rw[j];
              if (p.accumulate) a += dst[0];
              __builtin_nontemporal_store(a, dst);
            }
          }
        }
      } else {
        // bf16: 8 columns (one 16-byte piece) of 4 rows per thread
        const int ec = (tid & 31) * 8, er = tid >> 5;
        f32x4 lo[4], hi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          lo[j] = *(const f32x4*)(stg + (er + 16 * j) * CT8_LD + ec);
          hi[j] = *(const f32x4*)(stg + (er + 16 * j) * CT8_LD + ec + 4);
        }
        if (tc0 + ec < p.NC) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = er + 16 * j;
            const int trow = h * 128 + (r >> 5) * 64 + u * 32 + (r & 31);
            if (trow < nrows) {
              gbf16x8* dst = (gbf16x8*)(Ce + ((int64_t)(tr0 + trow) * p.ldc + tc0 + ec) * 2);
              float vv[8] = {lo[j][0], lo[j][1], lo[j][2], lo[j][3], hi[j][0], hi[j][1], hi[j][2], hi[j][3]};
              if (p.accumulate) {
                const bf16x8 old = *dst;
#pragma unroll
                for (int t = 0; t < 8; ++t) vv[t] += (float)old[t];
              }
              bf16x8 o8;
#pragma unroll
              for (int t = 0; t < 8; ++t) o8[t] = (bf16)vv[t];
              __builtin_nontemporal_store(o8, dst);
            }
          }
        }
      }
      EPI_SYNC();                                          // every thread's staging reads retired before the next pass / tile
    }
  }   // persistent tile loop
}

int fp8w_grid(int64_t tiles) {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
    if (ncu <= 0) ncu = 256;
  }
  return (int)std::min<int64_t>(tiles, ncu);
}

}  // namespace

int gg8f_wgrad(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Bq, int64_t ldb, const void* Bs, int64_t ldbs,
               const int32_t* poff, int E, int Na, int Nb, void* const* c_ptrs, int64_t ldc, int out_dtype, int accumulate,
               const int32_t* xcd_order, hipStream_t st) {
  Fp8WArgs p{};
  p.A = (const uint8_t*)Aq; p.ld_a = lda; p.AS = (const uint8_t*)As; p.ld_as = ldas;
  p.B = (const uint8_t*)Bq; p.ld_b = ldb; p.BS = (const uint8_t*)Bs; p.ld_bs = ldbs;
  p.poff = poff; p.E = E; p.NR = Na; p.NC = Nb;
  p.out_ptrs = c_ptrs; p.ldc = ldc; p.accumulate = accumulate; p.out_f32 = out_dtype == CSMOE_F32;
  p.tile_band = E > 1 ? 5 : 4;                   // gg8_wgrad's band heights
  const int64_t tiles = (int64_t)E * ((Na + BM8 - 1) / BM8) * ((Nb + BN8 - 1) / BN8);
  unsigned n_tiles;
  int rc = grid_1d("grouped_wgrad_mxfp8", tiles, &n_tiles);
  if (rc || !n_tiles) return rc;
  const int grid = fp8w_grid(tiles);
  // dealing needs whole experts per XCD and a grid that is a multiple of 8 (gg8_wgrad)
  const bool deal = xcd_order && (E % 8 == 0 || E >= 64) && grid % 8 == 0 && grid < tiles;
  p.xcd_order = deal ? xcd_order : nullptr;
  if ((rc = set_dyn_lds<gg8wf_kernel, LDS8_BYTES>())) return rc;
  hipLaunchKernelGGL(gg8wf_kernel, dim3((unsigned)grid), dim3(512), LDS8_BYTES, st, p);
  CSMOE_CHECK_LAUNCH("grouped_wgrad_mxfp8");
  return CSMOE_OK;
}
