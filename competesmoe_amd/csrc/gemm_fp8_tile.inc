// Body of the row-space MXFP8 tile kernels of gemm_fp8.hip (gg8f_kernel, gg8fq_kernel) from the tile lookup to the drained K-loop, shared as
// TEXT like the gemm_loop_*.inc K-loops (gemm_tiles.h: these kernels are sensitive to what hipcc hoists; tools/kernel_isa_diff.py is
// the check).  In scope: Fp8Args p.  Leaves acc[4][8], smem, lane, wm, wn, e, row0, rows, tc0 and the SLOT / ISSUE_* / FRAG / MFMA8
// macros (the weight-gradient kernel's K-loop uses them too) for the epilogue that follows.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  const int nct = (p.NC + BN8 - 1) / BN8;
  FIND_TILE_OR_RETURN(tp, p.offsets, p.E, p.single_M, BM8, nct, 0, 0);
  TILE_VARS_8W(tp, BM8, BN8);
  // the DMA helpers count the reduction in 2-byte units (they were written for bf16): 64 units = one 128-byte K-tile
  const int red_len = p.Kd >> 1;
  const int ncols = min(BN8, p.NC - tc0);

  const unsigned ldr_b = (unsigned)p.ld_r, ldc_b = (unsigned)p.ld_c;
  const unsigned ldrs = (unsigned)p.ld_rs, ldcs = (unsigned)p.ld_cs;
  const unsigned nsb = (unsigned)(p.Kd >> 5);          // scale bytes per row
  __amdgpu_buffer_rsrc_t rs_r, rs_c, rs_rs, rs_cs;
  unsigned vb_rl[2], vb_rh[2], vb_cl[2], vb_ch[2];
  int ax_r[2], ax_c[2], ax_dummy[2];
  rs_r = make_rsrc(p.R + (int64_t)row0 * ldr_b, (unsigned)rows * ldr_b);
  dma_setup<KC, 2>(vb_rl, ax_r, ldr_b, 0, 0, 7, 0, 0, wave, lane);
  dma_setup<KC, 2>(vb_rh, ax_dummy, ldr_b, 0, 0, 7, 0, 128, wave, lane);
  const char* wb = (const char*)(p.c_ptrs ? p.c_ptrs[e] : p.single_B);
  const char* wsb = (const char*)(p.cs_ptrs ? p.cs_ptrs[e] : p.single_BS);
  rs_c = make_rsrc(wb + (int64_t)tc0 * ldc_b, (unsigned)ncols * ldc_b);
  dma_setup<KC, 2>(vb_cl, ax_c, ldc_b, 0, 0, 7, 0, 0, wave, lane);
  dma_setup<KC, 2>(vb_ch, ax_dummy, ldc_b, 0, 0, 7, 0, 128, wave, lane);
  rs_rs = make_rsrc(p.RS + (int64_t)row0 * ldrs, (unsigned)rows * ldrs);
  rs_cs = make_rsrc(wsb + (int64_t)tc0 * ldcs, (unsigned)ncols * ldcs);
  // scale piece of this wave: waves 0-3 rows (wave * 64 + lane) of the tile, waves 4-7 columns ((wave - 4) * 64 + lane)
  const bool sc_rows = wave < 4;
  const unsigned sc_vbase = (unsigned)((wave & 3) * 64 + lane) * (sc_rows ? ldrs : ldcs);

  // ---------------- LDS read addressing ----------------
  const int g = lane >> 4, i16 = lane & 15;
  const int sw = (i16 >> 1) & 7;
  const int f_lo = i16 * 128 + ((g ^ sw) << 4);                // chunk g     of this lane's row (source-side swizzle of dma_setup)
  const int f_hi = i16 * 128 + (((g + 4) ^ sw) << 4);          // chunk g + 4
  const int r_blk0 = wm * 4, c_blk0 = wn * 2;

  ZERO_ACC(acc, 4, 8);

  const int nk = (p.Kd + 127) / 128;

#define SCSLOT(tile) (smem + SC_OFF + ((tile) & 1) * 2048)
#define ISSUE_RL(tile) dma_tile<KC, 2>(rs_r, SLOT(0, tile), vb_rl, ax_r, (tile) * 64, red_len, ldr_b, wave)
#define ISSUE_CL(tile) dma_tile<KC, 2>(rs_c, SLOT(1, tile), vb_cl, ax_c, (tile) * 64, red_len, ldc_b, wave)
#define ISSUE_CH(tile) dma_tile<KC, 2>(rs_c, SLOT(2, tile), vb_ch, ax_c, (tile) * 64, red_len, ldc_b, wave)
#define ISSUE_RH(tile) dma_tile<KC, 2>(rs_r, SLOT(3, tile), vb_rh, ax_r, (tile) * 64, red_len, ldr_b, wave)
  // 4 scale bytes (the K-tile's four 32-element blocks) of one row / column per lane
#define ISSUE_SC(tile)                                                                                              \
  do {                                                                                                              \
    unsigned vo_ = sc_vbase + (unsigned)(tile) * 4u;                                                                \
    if ((unsigned)(tile) * 4u >= nsb) vo_ = OOB;                                                                    \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(sc_rows ? rs_rs : rs_cs, (lds_void*)(SCSLOT(tile) + wave * 256), 4,    \
                                             vo_, 0, 0, 0);                                                         \
  } while (0)
#define FRAG(img, blk) ({                                                              \
    const i32x4 lo_ = *(const i32x4*)((img) + (blk) * 2048 + f_lo);                     \
    const i32x4 hi_ = *(const i32x4*)((img) + (blk) * 2048 + f_hi);                     \
    i32x8{lo_[0], lo_[1], lo_[2], lo_[3], hi_[0], hi_[1], hi_[2], hi_[3]}; })
#define MFMA8(ACC, FC, FR, SC, SR) \
  ACC = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(FC, FR, ACC, 0, 0, 0, SC, 0, SR)

  const int rows_here = rows - wm * 64;
  const int cols_here = ncols - wn * 32;
  const bool rlo = rows_here > 0, rhi = rows_here > 128, clo = cols_here > 0, chi = cols_here > 128;

#include "gemm_loop_fp8.inc"

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
