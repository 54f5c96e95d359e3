// The epilogue of the two MX decode kernels (gemm_skinny_fp8.hip, gemm_skinny_fp4.hip), included INSIDE the kernel body right after
// SKINNY_STORE_PARTIAL: one copy, so the two kernels cannot drift apart at the rounding points or in what they write.  From the
// enclosing scope: NB, NW, LDW, p (Skinny8Args), red_s (the NW partial tiles of 16 rows x LDW floats), e, row0, rows, n0.  The
// contract is stated in gemm_skinny_fp8.hip's header (bounds, last bullet; epilogue paragraph).
  constexpr int CPR = 2 * NB;                         // epilogue threads (8 columns each) per row
  // thread (r, cg) owns 8 columns of one row; whole waves past the 16 rows leave
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
