// One-pass XMoE cosine router for gfx950 (moe_model/model/moe/xmoe.py:80-91, moe_pretrain_model/layers/moe/xmoe.py:143-162):
// x is read ONCE and leaves as reduced = x @ expert_sel^T (bf16, R = E / 2 columns), the cosine logits of the normalised row
// against the expert embeddings, p = softmax(logits / temperature), the top-K expert ids with the softmax over their K values and
// the per-block expert histogram of the token binning -- `inp_reduction` + `_cosine` + softmax + `_keepTopk` + the counting pass,
// which upstream (and the torch-op form of this project's layers) runs as a chain of ~15 launches.
//
// Streaming half: router_fused.hip's loop with the reduction matrix in the gate's place (a second copy, so that gate_select_kernel's
// code does not move): 4 waves x 16 rows per workgroup, A fragments from global memory straight into v_mfma_f32_16x16x32_bf16,
// expert_sel staged through LDS in 256-wide K chunks, K ascending (the bits csmoe_gate_logits gives), a ring of three x chunks per
// wave and an LDS-only barrier per chunk (that file's header says why).  R <= 32: one or two column blocks.
// Row half: 16 lanes per row, four rows per wave at once: fp32 sum of squares in a fixed tree, the row divided by
// max(norm, eps), E cosines accumulated in fp32 over ascending r against the embeddings held in LDS, rounded to bf16, then
// select_row_temp_g16 (CSMOE_SEL_TEMP_SOFTMAX_TOPK) -- the bits csmoe_router_select gives on the stored logits.
// Non-finite rows (`_make_finite`): a non-finite reduced row makes all its E logits non-finite; upstream replaces them by the smallest
// finite logit of the tensor, i.e. routes the row from E equal values.  The row is routed that way here (experts 0..K-1, weights
// 1/K) without knowing the minimum; every workgroup leaves the minimum of its finite logits and its count of such rows, and a
// one-workgroup patch launch that returns at once when the counts are all zero rewrites the stored logits of those rows.
// Second normalisation (CSMOE_COS_NORM_THETA, the perturbed-cosine router `smoe_perturbed`, moe_model/model/moe/smoe_perturbed.py:
// 102): the row is divided by ||reduced|| + theta, no clamp (`eps` carries theta); under CSMOE_COS_NORM_BF16 the norm and the sum
// are bf16 tensors, as in a bf16 module without autocast.  A template parameter: the XMoE instantiations hold none of its code.
#include "router_select.h"

namespace {

constexpr int RC_WAVES = 4;
constexpr int RC_ROWS = 16 * RC_WAVES;
constexpr int RC_RING = 3;
constexpr int RC_KCH = 256;
constexpr int RC_LD = RC_KCH + 8;
constexpr int RC_LR = 33;                                     // floats per staged row of `reduced` / of the embeddings (R <= 32, +1: banks)
// LDS after the stream (over the dead staging buffers): reduced rows, embeddings, histogram, per-wave minimum / count
constexpr int RC_OFF_EMB = RC_WAVES * 16 * RC_LR;             // in floats
constexpr int RC_OFF_HIST = RC_OFF_EMB + 64 * RC_LR;
constexpr int RC_OFF_WG = RC_OFF_HIST + 64;
constexpr int RC_TAIL_FLOATS = RC_OFF_WG + 2 * RC_WAVES;

__device__ __forceinline__ float g16_sum(float v) {
  v += dpp_ror<8>(v); v += dpp_ror<4>(v); v += dpp_ror<2>(v); v += dpp_ror<1>(v);
  return v;
}

// The row half of both kernels: `reduced` of this wave's 16 rows lies in LDS ([16][RC_LR] per wave, fp32 values of the bf16 results).
// ||reduced|| + theta of CSMOE_COS_NORM_THETA from the fp32 sum of squares; `nrm` receives the norm the autograd sees.
__device__ __forceinline__ float theta_denom(float ss, float theta, bool norm_bf16, float& nrm) {
  nrm = sqrtf(ss);
  if (!norm_bf16) return nrm + theta;
  nrm = (float)(bf16)nrm;                                      // `mat1.norm()` of a bf16 tensor: an fp32 sum rounded once
  return (float)(bf16)(nrm + theta);                           // `+ theta` on that bf16 tensor
}

template <bool K2, bool THETA>
__device__ __forceinline__ void cosine_row_half(char* smem, const float* __restrict__ emb, int T, int E, int K_rt, int flags,
                                                float temperature, float eps, bf16* __restrict__ reduced, bf16* __restrict__ logits,
                                                float* __restrict__ p, int32_t* __restrict__ idx, float* __restrict__ w,
                                                int32_t* __restrict__ block_hist, int32_t* __restrict__ work) {
  const int K = K2 ? 2 : K_rt;
  const int R = E >> 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int row0 = blockIdx.x * RC_ROWS + wave * 16;
  float* lds = (float*)smem;
  float* lrow = lds + wave * 16 * RC_LR;                       // [16][RC_LR] per wave: reduced (bf16 values), then the normalised row
  float* semb = lds + RC_OFF_EMB;                              // [E][RC_LR]
  int32_t* hist = (int32_t*)(lds + RC_OFF_HIST);               // [64]
  float* wgmin = lds + RC_OFF_WG;                              // [RC_WAVES]
  int32_t* wgcnt = (int32_t*)(lds + RC_OFF_WG + RC_WAVES);     // [RC_WAVES]
  const bool oper_bf16 = flags & CSMOE_COS_OPER_BF16;
  for (int i = tid; i < E * R; i += 64 * RC_WAVES) {
    const float v = emb[i];
    semb[(i / R) * RC_LR + (i % R)] = oper_bf16 ? (float)(bf16)v : v;
  }
  if (tid < 64) hist[tid] = 0;
  __syncthreads();

  float lmin = INFINITY;
  int nbad = 0;
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const int r = r4 * 4 + g;
    const int t = row0 + r;
    const bool live = t < T;
    const int64_t tt = live ? t : 0;
    float* mr = lrow + r * RC_LR;
    const float x0 = i16 < R ? mr[i16] : 0.f;
    const float x1 = i16 + 16 < R ? mr[i16 + 16] : 0.f;
    if (live && i16 < R) reduced[tt * R + i16] = (bf16)x0;
    if (live && i16 + 16 < R) reduced[tt * R + i16 + 16] = (bf16)x1;
    // ||reduced||: elements l and l + 16 inside the lane, then the 16-lane tree (xor 8, 4, 2, 1)
    const float ss = g16_sum(x0 * x0 + x1 * x1);
    float denom, nrm_;
    if constexpr (THETA) denom = theta_denom(ss, eps, flags & CSMOE_COS_NORM_BF16, nrm_);
    else denom = fmaxf(sqrtf(ss), eps);
    float m0 = x0 / denom, m1 = x1 / denom;
    if (oper_bf16) { m0 = (float)(bf16)m0; m1 = (float)(bf16)m1; }
    if (i16 < R) mr[i16] = m0;
    if (i16 + 16 < R) mr[i16 + 16] = m1;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    for (int rr = 0; rr < R; ++rr) {
      const float mv = mr[rr];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = fmaf(mv, semb[(i16 + 16 * j) * RC_LR + rr], c[j]);     // rows >= E: stale LDS, masked below
    }
    float badf = 0.f, rmin = INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = (float)(bf16)c[j];
      if (i16 + 16 * j < E) {
        if (!isfinite(c[j])) badf = 1.f;
        rmin = fminf(rmin, c[j]);
      }
    }
    const bool bad = g16_max(badf) != 0.f;
    float s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = i16 + 16 * j;
      s[j] = e < E ? (bad ? 0.f : c[j]) : -INFINITY;
      if (live && e < E) logits[tt * E + e] = bad ? (bf16)NAN : (bf16)c[j];
    }
    if (live && !bad) lmin = fminf(lmin, rmin);
    if (live && bad && i16 == 0) ++nbad;
    int myi[4];
    select_row_temp_g16(s, i16, E, K, flags & 3, temperature, CSMOE_BF16, live, p + tt * E, idx + tt * K, w + tt * K, myi);
    if (block_hist && live) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i16 + 16 * j < K) atomicAdd(&hist[myi[j]], 1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lmin = fminf(lmin, __shfl_xor(lmin, o, 64));
    nbad += __shfl_xor(nbad, o, 64);
  }
  if (lane == 0) { wgmin[wave] = lmin; wgcnt[wave] = nbad; }
  __syncthreads();
  if (block_hist && tid < E) block_hist[(int64_t)blockIdx.x * E + tid] = hist[tid];
  if (tid == 0) {
    float m = wgmin[0];
    int n = wgcnt[0];
#pragma unroll
    for (int v = 1; v < RC_WAVES; ++v) { m = fminf(m, wgmin[v]); n += wgcnt[v]; }
    work[2 + blockIdx.x] = n;
    work[2 + gridDim.x + blockIdx.x] = __float_as_int(m);
  }
}

// R <= 4 (E <= 8): the reduction as csmoe_gate_logits computes it for so few columns (gate_small_fwd_kernel, moe_kernels.hip) -- a wave
// per row, lane l takes the 16-byte pieces l, l + 64, ... of the row, fp32 products added in element order, then the wave
// butterfly -- so that `reduced` carries that entry's bits here too; an MFMA tile would be 3/4 empty.  A wave owns the same 16 rows
// of the same 64-row block as in the MFMA kernel (one block histogram contract), four rows in flight at a time.
template <bool K2, bool THETA>
__global__ void __launch_bounds__(64 * RC_WAVES) cosine_select_small_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wr,
                                                                            const float* __restrict__ emb, int T, int D, int E, int K_rt,
                                                                            int flags, float temperature, float eps,
                                                                            bf16* __restrict__ reduced, bf16* __restrict__ logits,
                                                                            float* __restrict__ p, int32_t* __restrict__ idx,
                                                                            float* __restrict__ w, int32_t* __restrict__ block_hist,
                                                                            int32_t* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int R = E >> 1;                                        // <= 4
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * RC_ROWS + wave * 16;
  float* lrow = (float*)smem + wave * 16 * RC_LR;
  for (int r0 = 0; r0 < 16; r0 += 4) {
    float acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[q][e] = 0.f;
    for (int d = lane * 8; d < D; d += 64 * 8) {
      bf16x8 xv[4], wv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) xv[q] = *(const bf16x8*)(x + (int64_t)min(row0 + r0 + q, T - 1) * D + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[e] = e < R ? *(const bf16x8*)(wr + (int64_t)e * D + d) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[q][e] += (float)xv[q][j] * (float)wv[e][j];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float sum = wave_sum(acc[q][e]);
        if (lane == 0 && e < R) lrow[(r0 + q) * RC_LR + e] = (float)(bf16)sum;
      }
  }
  cosine_row_half<K2, THETA>(smem, emb, T, E, K_rt, flags, temperature, eps, reduced, logits, p, idx, w, block_hist, work);
}

// work[0]: non-finite rows of the call (patch launch); work[2 + b]: count of workgroup b; work[2 + nb + b]: its finite minimum (float bits)
template <int NE, bool K2, bool THETA>
__global__ void __launch_bounds__(64 * RC_WAVES) cosine_select_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wr,
                                                                      const float* __restrict__ emb, int T, int D, int E, int K_rt,
                                                                      int flags, float temperature, float eps,
                                                                      bf16* __restrict__ reduced, bf16* __restrict__ logits,
                                                                      float* __restrict__ p, int32_t* __restrict__ idx,
                                                                      float* __restrict__ w, int32_t* __restrict__ block_hist,
                                                                      int32_t* __restrict__ work) {
  const int R = E >> 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* wbuf = (bf16*)smem;                                   // 2 x [NE*16][RC_LD]
  constexpr int WB = NE * 16 * RC_LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int row0 = blockIdx.x * RC_ROWS + wave * 16;
  const int my_row = min(row0 + i16, T - 1);                  // rows past the end re-read the last row; their results are dropped
  const bf16* xrow = x + (int64_t)my_row * D + 8 * g;

  const int s_seg = tid & 31, s_row = tid >> 5;
  constexpr int RPP = 2 * RC_WAVES;
  constexpr int NPASS = NE * 16 / RPP;
  bf16x8 wreg[NPASS];
  bf16x8 a[RC_RING][8];
  f32x4 acc[NE];
#pragma unroll
  for (int c = 0; c < NE; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nch = (D + RC_KCH - 1) / RC_KCH;
  auto load_w = [&](int ch) {
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      const int e = ps * RPP + s_row, k = ch * RC_KCH + s_seg * 8;
      wreg[ps] = (e < R && k < D) ? *(const bf16x8*)(wr + (int64_t)e * D + k) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  auto store_w = [&](int buf) {
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) *(bf16x8*)(wbuf + buf * WB + (ps * RPP + s_row) * RC_LD + s_seg * 8) = wreg[ps];
  };
  auto load_a = [&](bf16x8 (&av)[8], int ch) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int k = ch * RC_KCH + ks * 32;
      av[ks] = (k + 8 * g < D) ? *(const bf16x8*)(xrow + k) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  auto step = [&](int ch, bf16x8 (&a_use)[8], bf16x8 (&a_fill)[8]) {
    const bool more = ch + 1 < nch;
    if (more) load_w(ch + 1);
    if (ch + RC_RING - 1 < nch) load_a(a_fill, ch + RC_RING - 1);
    const bf16* wb = wbuf + (ch & 1) * WB + i16 * RC_LD + 8 * g;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
      for (int c = 0; c < NE; ++c) {
        const bf16x8 b = *(const bf16x8*)(wb + c * 16 * RC_LD + ks * 32);
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_use[ks], b, acc[c], 0, 0, 0);
      }
    }
    if (more) store_w((ch + 1) & 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // LDS-only barrier: the x chunks in flight stay in flight
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  load_w(0);
#pragma unroll
  for (int j = 0; j < RC_RING - 1; ++j)
    if (j < nch) load_a(a[j], j);
  store_w(0);
  __syncthreads();
  for (int ch = 0; ch < nch; ch += RC_RING) {
#pragma unroll
    for (int j = 0; j < RC_RING; ++j)
      if (ch + j < nch) step(ch + j, a[j], a[(j + RC_RING - 1) % RC_RING]);
  }

  // ---- row half.  Every staging read is behind the last step's barrier: the buffers are reused.
  float* lrow = (float*)smem + wave * 16 * RC_LR;
#pragma unroll
  for (int c = 0; c < NE; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) lrow[(4 * g + j) * RC_LR + c * 16 + i16] = (float)(bf16)acc[c][j];
  cosine_row_half<K2, THETA>(smem, emb, T, E, K_rt, flags, temperature, eps, reduced, logits, p, idx, w, block_hist, work);
}

// One workgroup after every cosine_select launch: sums the counts; nothing else to do when the sum is zero.
__global__ void __launch_bounds__(256) cosine_patch_kernel(bf16* __restrict__ logits, int T, int E, int nb, int32_t* __restrict__ work) {
  __shared__ int s_cnt[256];
  __shared__ float s_min[256];
  __shared__ int s_bad[RC_ROWS];
  const int tid = threadIdx.x;
  int n = 0;
  for (int b = tid; b < nb; b += 256) n += work[2 + b];
  s_cnt[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_cnt[tid] += s_cnt[tid + o];
    __syncthreads();
  }
  const int total = s_cnt[0];
  if (tid == 0) work[0] = total;
  if (total == 0) return;
  float m = INFINITY;
  for (int b = tid; b < nb; b += 256) m = fminf(m, __int_as_float(work[2 + nb + b]));
  s_min[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_min[tid] = fminf(s_min[tid], s_min[tid + o]);
    __syncthreads();
  }
  const float low = isfinite(s_min[0]) ? s_min[0] : 0.f;      // no finite logit at all: upstream raises there
  for (int b = 0; b < nb; ++b) {
    if (work[2 + b] == 0) continue;                             // uniform over the workgroup
    __syncthreads();
    if (tid < RC_ROWS) {
      const int t = b * RC_ROWS + tid;
      s_bad[tid] = t < T && !isfinite((float)logits[(int64_t)t * E]);
    }
    __syncthreads();
    for (int i = tid; i < RC_ROWS * E; i += 256) {
      const int r = i / E;
      if (s_bad[r]) logits[((int64_t)b * RC_ROWS + r) * E + (i % E)] = (bf16)low;
    }
  }
}

// ---- backward of the row half ---------------------------------------------------------------------------------------------------
// 16 lanes per row.  Lane l16 holds experts l16 + 16 j (j < 4) and reduced columns l16, l16 + 16.  Autograd of the reference's ops
// in their order: softmax over K, top-K scatter (+ d p of the losses), the fp32 softmax with its own unrounded output, the cast and
// the division by the temperature in bf16, (+ d logits of the losses, added in bf16 as the engine adds two bf16 gradients), the
// cosine product (fp32; its operand gradients rounded to bf16 under CSMOE_COS_OPER_BF16), F.normalize (the clamp blocks the norm's
// branch where the norm is below eps: d reduced = d m / eps there), rounded to bf16 at `reduced`.  Under CSMOE_COS_NORM_THETA the
// last step is the division by ||v|| + theta instead: two bf16 gradients of `reduced` (the cast and the norm) added in bf16.
// d emb[e][r] = sum_t d cos[t][e] m[t][r]: each lane keeps its 4 x 32 entries in registers over the rows its group visits (ascending),
// the 16 groups of a workgroup are added in group order through LDS, and workgroup b writes partial table b; cosine_demb_kernel
// adds the tables in ascending b.  No atomics: the same bits on every run.
constexpr int CB_GROUPS = 16;                                  // row groups per workgroup (256 threads)
constexpr int CB_MAX_PARTS = 256;

template <bool THETA>
__global__ void __launch_bounds__(256) cosine_select_bwd_kernel(const bf16* __restrict__ reduced, const float* __restrict__ emb,
                                                                const bf16* __restrict__ logits, const int32_t* __restrict__ idx,
                                                                const float* __restrict__ w, const float* __restrict__ dw,
                                                                const float* __restrict__ dp, const bf16* __restrict__ dlogits, int T,
                                                                int E, int K, int flags, float temperature, float eps,
                                                                bf16* __restrict__ d_reduced, float* __restrict__ part) {
  __shared__ float semb[64 * RC_LR];
  __shared__ float srow[CB_GROUPS][2][64];                     // per group: m (R values), d cos (E values)
  __shared__ float sred[CB_GROUPS][65];
  const int R = E >> 1;
  const int tid = threadIdx.x, grp = tid >> 4, l16 = tid & 15;
  const bool oper_bf16 = flags & CSMOE_COS_OPER_BF16, pb = flags & CSMOE_TEMP_P_BF16, wb = flags & CSMOE_TEMP_W_BF16;
  const bool norm_bf16 = THETA && (flags & CSMOE_COS_NORM_BF16);
  for (int i = tid; i < E * R; i += 256) {
    const float v = emb[i];
    semb[(i / R) * RC_LR + (i % R)] = oper_bf16 ? (float)(bf16)v : v;
  }
  __syncthreads();
  float acc[4][32];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 32; ++r) acc[j][r] = 0.f;
  float* sm_ = srow[grp][0];
  float* sd_ = srow[grp][1];
  // rows of this workgroup: a contiguous range, groups interleaved inside it; every group runs the same number of rounds
  const int per = (T + gridDim.x - 1) / gridDim.x;
  const int t_lo = blockIdx.x * per, t_hi = min(T, t_lo + per);
  for (int t0 = t_lo; t0 < t_hi; t0 += CB_GROUPS) {
    const int t = t0 + grp;
    const bool live = t < t_hi;
    const int64_t tt = live ? t : t_lo;
    // ---- d w -> d keys (softmax over K), scattered into d p
    float g[4], z[4], ex[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = l16 + 16 * j;
      g[j] = (dp && e < E) ? dp[tt * E + e] : 0.f;
      z[j] = e < E ? (float)(bf16)((float)logits[tt * E + e] / temperature) : -INFINITY;
    }
    float dot = 0.f;
    for (int k = 0; k < K; ++k) dot += (dw ? dw[tt * K + k] : 0.f) * w[tt * K + k];       // k order, the same in every lane
    for (int k = 0; k < K; ++k) {
      const float wk = w[tt * K + k];
      float dv = wk * ((dw ? dw[tt * K + k] : 0.f) - dot);
      if (wb) dv = (float)(bf16)dv;
      const int ei = idx[tt * K + k];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (l16 + 16 * j == ei) g[j] = pb ? (float)(bf16)(g[j] + dv) : g[j] + dv;
    }
    // ---- fp32 softmax of z, recomputed with select_row_g16's trees
    const float mx = g16_max(fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3])));
#pragma unroll
    for (int j = 0; j < 4; ++j) ex[j] = (l16 + 16 * j) < E ? expf(z[j] - mx) : 0.f;
    const float sum = g16_sum64(ex);
    float in4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) in4[j] = g[j] * (ex[j] / sum);
    const float inner = g16_sum64(in4);
    // ---- the normalised row.  A non-finite row had its logits ASSIGNED (`_make_finite`): no gradient reaches it
    const float x0 = l16 < R ? (float)reduced[tt * R + l16] : 0.f;
    const float x1 = l16 + 16 < R ? (float)reduced[tt * R + l16 + 16] : 0.f;
    const float ss = g16_sum(x0 * x0 + x1 * x1);
    const float nrm = sqrtf(ss);
    // The forward flags a row by its non-finite LOGITS, i.e. by a non-finite element of `reduced`; this tests the sum of squares.
    // The two differ only for a finite row whose fp32 sum of squares overflows (|v| >~ 1.8e19): the forward gives it m = 0 and
    // finite zero logits, and here it gets no gradient -- which is also what the arithmetic below yields for it (every term is
    // d / inf = 0), so the results agree.
    const bool row_ok = isfinite(ss);
    float dc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = l16 + 16 * j;
      const float dz = (float)(bf16)((ex[j] / sum) * (g[j] - inner));
      float d = (float)(bf16)(dz / temperature);
      if (dlogits && e < E) d = (float)(bf16)(d + (float)dlogits[tt * E + e]);
      dc[j] = (live && row_ok && e < E) ? d : 0.f;
      sd_[e] = dc[j];
    }
    float denom, nrm_t = nrm;                                  // nrm_t: the norm as the reference's tensor holds it (THETA)
    if constexpr (THETA) denom = theta_denom(ss, eps, norm_bf16, nrm_t);
    else denom = fmaxf(nrm, eps);
    float m0 = x0 / denom, m1 = x1 / denom;
    const float q0 = m0, q1 = m1;                              // the fp32 quotient: what the division's backward multiplies by
    if (oper_bf16) { m0 = (float)(bf16)m0; m1 = (float)(bf16)m1; }
    sm_[l16] = l16 < R ? m0 : 0.f;
    sm_[l16 + 16] = l16 + 16 < R ? m1 : 0.f;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // ---- d emb: this lane's experts x every r
#pragma unroll
    for (int r = 0; r < 32; ++r) {
      const float mv = sm_[r];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j][r] = fmaf(dc[j], mv, acc[j][r]);
    }
    // ---- d m[r] = sum_e d cos[e] emb[e][r], ascending e; this lane's r = l16, l16 + 16
    float dm0 = 0.f, dm1 = 0.f;
    for (int e = 0; e < E; ++e) {
      const float d = sd_[e];
      dm0 = fmaf(d, semb[e * RC_LR + l16], dm0);
      dm1 = fmaf(d, semb[e * RC_LR + l16 + 16], dm1);
    }
    if (l16 >= R) dm0 = 0.f;
    if (l16 + 16 >= R) dm1 = 0.f;
    if (oper_bf16) { dm0 = (float)(bf16)dm0; dm1 = (float)(bf16)dm1; }
    float dx0 = dm0 / denom, dx1 = dm1 / denom;
    if constexpr (THETA) {
      // ---- m = v.float() / (||v|| + theta): `reduced` is used twice and the engine adds two bf16 gradients.  Stream 1, the
      // `.float()` cast, is d m / den rounded to bf16.  Stream 2, the norm: d den = sum_r -(d m_r (m_r / den)), a bf16 tensor under
      // NORM_BF16 like den itself; the norm's backward d den (v / n) then runs in bf16, else in fp32 with one rounding at the
      // autocast cast; it is masked where n == 0.
      dx0 = (float)(bf16)dx0; dx1 = (float)(bf16)dx1;
      float dden = g16_sum(-(dm0 * (q0 / denom)) - dm1 * (q1 / denom));
      if (norm_bf16) dden = (float)(bf16)dden;
      if (nrm_t != 0.f) {
        float u0 = x0 / nrm_t, u1 = x1 / nrm_t;
        if (norm_bf16) { u0 = (float)(bf16)u0; u1 = (float)(bf16)u1; }
        dx0 += (float)(bf16)(dden * u0);
        dx1 += (float)(bf16)(dden * u1);
      }
    } else {
      // ---- F.normalize: m = v / clamp_min(||v||, eps)
      if (row_ok && nrm >= eps) {
        const float dd = g16_sum(dm0 * x0 + dm1 * x1);    // uniform branch inside the 16-lane group: the rotation stays inside it
        const float dden = -dd / (denom * denom);
        dx0 += dden * (x0 / nrm);
        dx1 += dden * (x1 / nrm);
      }
    }
    if (!row_ok) { dx0 = 0.f; dx1 = 0.f; }
    if (live && l16 < R) d_reduced[tt * R + l16] = (bf16)dx0;
    if (live && l16 + 16 < R) d_reduced[tt * R + l16 + 16] = (bf16)dx1;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  // ---- the 16 groups' tables, added in group order: 32 rounds of one r each (E values per group and round)
  float* out = part + (int64_t)blockIdx.x * E * R;
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) sred[grp][l16 + 16 * j] = acc[j][r];
    __syncthreads();
    if (tid < E && r < R) {
      float s = sred[0][tid];
#pragma unroll
      for (int q = 1; q < CB_GROUPS; ++q) s += sred[q][tid];
      out[tid * R + r] = s;
    }
  }
}

__global__ void __launch_bounds__(256) cosine_demb_kernel(const float* __restrict__ part, int nparts, int n, float* __restrict__ d_emb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int b = 0; b < nparts; ++b) s += part[(int64_t)b * n + i];
  d_emb[i] = s;
}

}  // namespace

bool k_cosine_select_ok(int T, int D, int E, int K, int dtype, const void* x, const void* wr) {
  return dtype == CSMOE_BF16 && E >= 2 && E <= 64 && E % 2 == 0 && K <= E && D % 8 == 0 && ((((uintptr_t)x | (uintptr_t)wr) & 15) == 0);
}

static int rc_blocks(int T) { return (T + RC_ROWS - 1) / RC_ROWS; }
int64_t k_cosine_select_work_ints(int T) { return 2 + 2 * (int64_t)rc_blocks(T); }

int k_cosine_select(const void* x, const void* wr, const float* emb, int T, int D, int E, int K, int flags, float temperature, float eps,
                    void* reduced, void* logits, float* p, int32_t* idx, float* w, int32_t* block_hist, int32_t* work, hipStream_t st) {
  const int nb = rc_blocks(T);
  if (T > 0) {
    const int ne = (E / 2 + 15) / 16;
    const dim3 grid(nb), block(64 * RC_WAVES);
    const size_t lds = std::max<size_t>((size_t)2 * ne * 16 * RC_LD * 2, (size_t)RC_TAIL_FLOATS * 4);
    const bool theta = flags & CSMOE_COS_NORM_THETA;
#define RC_LAUNCH(NE, K2, TH)                                                                                                      \
  hipLaunchKernelGGL((cosine_select_kernel<NE, K2, TH>), grid, block, lds, st, (const bf16*)x, (const bf16*)wr, emb, T, D, E, K,     \
                     flags, temperature, eps, (bf16*)reduced, (bf16*)logits, p, idx, w, block_hist, work)
#define RC_LAUNCH_SMALL(K2, TH)                                                                                                    \
  hipLaunchKernelGGL((cosine_select_small_kernel<K2, TH>), grid, block, (size_t)RC_TAIL_FLOATS * 4, st, (const bf16*)x,              \
                     (const bf16*)wr, emb, T, D, E, K, flags, temperature, eps, (bf16*)reduced, (bf16*)logits, p, idx, w, block_hist,  \
                     work)
#define RC_PICK(LAUNCH, ...)                                                                                                       \
  do {                                                                                                                             \
    if (theta) { if (K == 2) LAUNCH(__VA_ARGS__ true, true); else LAUNCH(__VA_ARGS__ false, true); }                               \
    else       { if (K == 2) LAUNCH(__VA_ARGS__ true, false); else LAUNCH(__VA_ARGS__ false, false); }                             \
  } while (0)
    if (E <= 8) RC_PICK(RC_LAUNCH_SMALL, );
    else if (ne == 1) RC_PICK(RC_LAUNCH, 1, );
    else RC_PICK(RC_LAUNCH, 2, );
#undef RC_PICK
#undef RC_LAUNCH_SMALL
#undef RC_LAUNCH
    CSMOE_CHECK_LAUNCH("cosine_select");
  }
  hipLaunchKernelGGL(cosine_patch_kernel, dim3(1), dim3(256), 0, st, (bf16*)logits, T, E, nb, work);
  CSMOE_CHECK_LAUNCH("cosine_select(patch)");
  return CSMOE_OK;
}

int k_cosine_select_bwd_parts(int T) { return std::max(1, std::min(CB_MAX_PARTS, (T + CB_GROUPS - 1) / CB_GROUPS)); }

int k_cosine_select_bwd(const void* reduced, const float* emb, const void* logits, const int32_t* idx, const float* w, const float* dw,
                        const float* dp, const void* dlogits, int T, int E, int K, int flags, float temperature, float eps,
                        void* d_reduced, float* d_emb, float* part, hipStream_t st) {
  const int nparts = k_cosine_select_bwd_parts(T);
  const int n = E * (E / 2);
  if (T > 0) {
    if (flags & CSMOE_COS_NORM_THETA)
      hipLaunchKernelGGL(cosine_select_bwd_kernel<true>, dim3(nparts), dim3(256), 0, st, (const bf16*)reduced, emb, (const bf16*)logits,
                         idx, w, dw, dp, (const bf16*)dlogits, T, E, K, flags, temperature, eps, (bf16*)d_reduced, part);
    else
      hipLaunchKernelGGL(cosine_select_bwd_kernel<false>, dim3(nparts), dim3(256), 0, st, (const bf16*)reduced, emb, (const bf16*)logits,
                         idx, w, dw, dp, (const bf16*)dlogits, T, E, K, flags, temperature, eps, (bf16*)d_reduced, part);
    CSMOE_CHECK_LAUNCH("cosine_select_bwd");
  }
  hipLaunchKernelGGL(cosine_demb_kernel, dim3((n + 255) / 256), dim3(256), 0, st, part, T > 0 ? nparts : 0, n, d_emb);
  CSMOE_CHECK_LAUNCH("cosine_select_bwd(d_emb)");
  return CSMOE_OK;
}
