// The K-loop section of the two MXFP8 256 x 256 kernels of gemm_fp8.hip (gg8f_kernel: row-space; gg8wf_kernel: weight gradient) --
// ONE text: DMA prologue, the hooks of the thin / BAL loop (gemm_loop_thin.inc, gemm_loop_bal.inc) and the closing barrier of the
// stagger.  In scope: rows, wm, r_blk0 / c_blk0, g, i16, rlo / rhi / clo / chi, acc, nk and the macros SLOT, SCSLOT, ISSUE_*, FRAG,
// MFMA8, WAIT_DMA, PHASE_SYNC_IN / _OUT.
  if (rows <= 128) {
    // Thin tile (the remainder tile of an expert: at 128 experts x ~512 rows half of the experts end in one of a few dozen rows):
    // the one-phase loop of gemm_bf16_v2.hip -- no RH image, one barrier pair and 7 pieces per K-tile, every wave's 4 x 4 blocks
    // of C_all x R_lo in one MFMA section.
    ISSUE_CL(0); ISSUE_CH(0); ISSUE_RL(0); ISSUE_SC(0); ISSUE_CL(1); ISSUE_CH(1); ISSUE_RL(1); ISSUE_SC(1);
    WAIT_DMA(7);                                           // K-tile 0 landed
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
#define THIN_FRAG_DECL const char* sc = SCSLOT(s); i32x8 fc[4], fr[4]; int sc_c[4], sc_r[4];
#define THIN_READ_CL(cb) fc[cb] = FRAG(i_cl, c_blk0 + cb); sc_c[cb] = *(const uint8_t*)(sc + 1024 + ((c_blk0 + cb) * 16 + i16) * 4 + g);
#define THIN_READ_CH(cb) fc[2 + cb] = FRAG(i_ch, c_blk0 + cb); sc_c[2 + cb] = *(const uint8_t*)(sc + 1024 + (128 + (c_blk0 + cb) * 16 + i16) * 4 + g);
#define THIN_READ_RL(rb) fr[rb] = FRAG(i_rl, r_blk0 + rb); sc_r[rb] = *(const uint8_t*)(sc + ((r_blk0 + rb) * 16 + i16) * 4 + g);
#define THIN_KSTEPS 1
#define THIN_MFMA(ks, cb, rb) MFMA8(acc[cb][rb], fc[cb], fr[rb], sc_c[cb], sc_r[rb]);
#define THIN_ISSUE(s) ISSUE_CL(s + 2); ISSUE_CH(s + 2); ISSUE_RL(s + 2); ISSUE_SC(s + 2)
#define THIN_WAIT(s) WAIT_DMA(7)                           /* K-tile s+1 landed (s+2 stays in flight) */
#include "gemm_loop_thin.inc"
  } else {
    // issue order ... [CL,CH,RL,SC](s+1) | RH(s+1) | [CL,CH,RL,SC](s+2) | RH(s+2) ...: 7 + 2 pieces per K-tile and wave, so the
    // counted waits of the bf16 loop (8) become 9
    ISSUE_CL(0); ISSUE_CH(0); ISSUE_RL(0); ISSUE_SC(0); ISSUE_RH(0); ISSUE_CL(1); ISSUE_CH(1); ISSUE_RL(1); ISSUE_SC(1);
    WAIT_DMA(9);                                           // CL, CH, RL, SC(0) landed
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();             // row half 1 starts half a phase late
    __builtin_amdgcn_sched_barrier(0);
    // phase A also reads ALL scales of K-tile s (the RH rows' too); a K = 128 MFMA per (column block, row block) and K-tile
#define BAL_FRAG_DECL const char* sc = SCSLOT(s); i32x8 fc[4], fr[4]; int sc_c[4], sc_r[8];
#define BAL_READ_CL(cb) fc[cb] = FRAG(i_cl, c_blk0 + cb); sc_c[cb] = *(const uint8_t*)(sc + 1024 + ((c_blk0 + cb) * 16 + i16) * 4 + g);
#define BAL_READ_CH(cb) fc[2 + cb] = FRAG(i_ch, c_blk0 + cb); sc_c[2 + cb] = *(const uint8_t*)(sc + 1024 + (128 + (c_blk0 + cb) * 16 + i16) * 4 + g);
#define BAL_READ_RL(rb) fr[rb] = FRAG(i_rl, r_blk0 + rb); sc_r[rb] = *(const uint8_t*)(sc + ((r_blk0 + rb) * 16 + i16) * 4 + g);
#define BAL_READ_RH(rb) fr[rb] = FRAG(i_rh, r_blk0 + rb);
#define BAL_PHASE_A_EXTRA                                                                                                      \
  if (rhi && clo) {                                                                                                            \
    _Pragma("unroll") for (int rb = 0; rb < 4; ++rb) sc_r[4 + rb] = *(const uint8_t*)(sc + (128 + (r_blk0 + rb) * 16 + i16) * 4 + g); \
  }
#define BAL_KSTEPS 1
#define BAL_MFMA(ks, cb, rb, arb) MFMA8(acc[cb][arb], fc[cb], fr[rb], sc_c[cb], sc_r[arb]);
#define BAL_ISSUE_A(s) ISSUE_RH(s + 1)
#define BAL_ISSUE_B(s) ISSUE_CL(s + 2); ISSUE_CH(s + 2); ISSUE_RL(s + 2); ISSUE_SC(s + 2)
#define BAL_WAIT_A(s) WAIT_DMA(9)                          /* RH(s) landed */
#define BAL_WAIT_B(s) WAIT_DMA(9)                          /* CL, CH, RL, SC(s+1) landed */
#include "gemm_loop_bal.inc"
    if (wm == 0) __builtin_amdgcn_s_barrier();
  }

