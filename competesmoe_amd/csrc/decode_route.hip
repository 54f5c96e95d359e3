// Decode front end for gfx950: ONE launch that reads the T token rows of a decode call once (T * K <= 1024 routed rows) and leaves
// everything the weight-streaming expert GEMMs and the combine need -- the gate logits (bf16), their fp32 softmax, the top-K expert ids
// with their weights, the stable counting sort of those ids (counts / offsets / perm / slot_of) and, when asked, the MXFP8 form of x.
// It stands for csmoe_gate_select (or csmoe_gate_logits + csmoe_router_select where E > 64), the scan and scatter launches of
// csmoe_bin_tokens_hist and csmoe_quantize_mxfp8 over x: `self.gate(x)` + `topk_expert` + the sort in front of `compute_moe`
// (moe_model/model/moe/smoe.py:42-44, moe.py:113-132, 189-191; moe_pretrain_model/layers/moe/moe.py:121, cvmm.py:580-593).
//
//   * grid (ceil(E / 16), ceil(T / 16)): a workgroup of 4 waves owns a 16-row x 16-expert tile of the logits.  Both operands are
//     K-contiguous and go by 16-byte loads straight into the MFMA operand registers (lane l: row / expert l % 16, 8 elements at
//     k = 8 * (l / 16), the B_NK form of gemm_skinny.hip): no LDS image.  The 32-element K-steps are dealt to the waves in runs, the
//     ragged last step (D % 32 != 0) zero-filled; v_mfma_f32_16x16x32_bf16, fp32 accumulate.  The four partial tiles meet in LDS and are
//     summed in wave order, then rounded to bf16 once: no float atomics, bit-identical from run to run.  At T = 1, E = 128 that is
//     eight workgroups streaming 128 KB of the gate each instead of one streaming 1 MB.
//   * the column-block-0 workgroup of a row block holds its rows' fragments already and writes xq / xs: a 32-element MX block is the
//     four lane groups of one K-step, so the block amax is two cross-lane steps; scale and convert are mx_quant.h's (the bytes of
//     csmoe_quantize_mxfp8).
//   * selection needs a whole row and the bins need every row: the hand-offs are ARRIVAL COUNTERS inside the launch.  Each column block
//     stores its logits and adds one to its row block's counter; the workgroup whose add came last selects the 16 rows (one wave per
//     row, select_row<VPL> / select_row_temp / select_row_signorm of router_select.h: the bits of csmoe_router_select) and adds one to
//     the global counter; the last of those sorts the ids in LDS (bin_scatter_kernel's ballot ranks).  Nobody polls or sleeps: a
//     workgroup that is not last returns, so a missing arrival could give a wrong result, never a hang.  With one row block (T <= 16)
//     the ids never leave LDS and there is one hand-off; with one column block as well there is none.
//   * a hand-off is: plain stores; every storing wave s_waitcnt vmcnt(0); __syncthreads(); lane 0 agent-scope release fence, the wait
//     again, a relaxed agent-scope fetch_add from that vector lane; the last arriver an agent-scope acquire fence, the wait,
//     __syncthreads(), then plain vector loads.  The XCDs' L2s are not coherent with each other: a workgroup-scope fence would be as
//     stale as none.  "I am last" travels through the kernel's one LDS object.  The counters are zeroed by a hipMemsetAsync on the launch
//     stream in front of every launch (capturable; right on the first call and after a failed one), never by the last arriver.
#include "router_select.h"
#include "mx_quant.h"

namespace {

constexpr int DR_WAVES = 4;
constexpr int DR_EMAX = 256;       // experts (select_row<4>)
constexpr int DR_NMAX = 1024;      // routed rows T * K whose ids fit the LDS sort
constexpr int DR_LGLD = DR_EMAX + 1;

struct DrLds {                     // the kernel's ONE LDS object
  float part[DR_WAVES][16][17];    // the waves' partial logit tiles
  float lg[16][DR_LGLD];           // the row block's logits (fp32 value of the bf16 logit) for the selection
  int32_t ids[DR_NMAX];            // selected ids: of this row block, then of the whole call
  int32_t running[DR_EMAX];        // histogram -> running offsets of the sort
  int32_t wcnt[DR_WAVES][DR_EMAX];
  int32_t wtot[DR_WAVES];
  int32_t last;
};

// Arrive on *counter after this workgroup's stores; true in every thread of the workgroup whose add was the `expect`-th (the last).
// That workgroup may then read what all the others stored before they arrived, with plain vector loads.
__device__ __forceinline__ bool arrive_last(int32_t* counter, int expect, DrLds& S) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == expect - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    S.last = last;
  }
  __syncthreads();
  return S.last != 0;
}

template <int VPL>
__global__ void __launch_bounds__(64 * DR_WAVES) decode_route_kernel(const bf16* __restrict__ x, const bf16* __restrict__ wg, int T, int D,
                                                                     int E, int K, int mode, int round_sum_bf16, float sel_param,
                                                                     bf16* logits, float* softmax, int32_t* idx, float* w,
                                                                     int32_t* counts, int32_t* offsets, int32_t* perm, int32_t* slot_of,
                                                                     uint8_t* xq, uint8_t* xs, int32_t* cnt) {
  __shared__ __attribute__((aligned(16))) DrLds S;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i16 = lane & 15;
  const int cb = blockIdx.x, rb = blockIdx.y, ncb = gridDim.x, nrb = gridDim.y;
  const int row0 = rb * 16;
  const int rows = min(16, T - row0);
  // rows past T re-read the last row, experts past E the last expert: their results are dropped
  const bf16* xrow = x + (int64_t)min(row0 + i16, T - 1) * D + 8 * g;
  const bf16* wrow = wg + (int64_t)min(cb * 16 + i16, E - 1) * D + 8 * g;
  const bool quant = xq != nullptr && cb == 0;
  const bool row_live = i16 < rows;
  uint8_t* qrow = xq + (int64_t)(row0 + i16) * D + 8 * g;
  uint8_t* srow = xs + (int64_t)(row0 + i16) * (D >> 5);

  // ---- the gate product: K-steps [s0, s1) of this wave, the full ones first
  const int nfull = D >> 5, nks = (D + 31) >> 5;
  const int per = (nks + DR_WAVES - 1) / DR_WAVES;
  const int s0 = min(nks, wave * per), s1 = min(nks, s0 + per), f1 = min(s1, nfull);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  auto quant_step = [&](const bf16x8& a, int ks) {
    float f[8];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = (float)a[j];
      amax = fmaxf(amax, fabsf(f[j]));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
    const int sb = e8m0_of_amax(amax);
    const float inv = inv_scale_of(sb);
    u32x2 o;
    o[0] = pack4_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
    o[1] = pack4_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
    if (row_live) {
      *(u32x2*)(qrow + ks * 32) = o;
      if (g == 0) srow[ks] = (uint8_t)sb;
    }
  };
  int ks = s0;
  for (; ks + 8 <= f1; ks += 8) {                 // sixteen 16-byte loads in flight per lane
    bf16x8 a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a[u] = *(const bf16x8*)(xrow + (ks + u) * 32);
      b[u] = *(const bf16x8*)(wrow + (ks + u) * 32);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], b[u], acc, 0, 0, 0);
    if (quant) {
#pragma unroll
      for (int u = 0; u < 8; ++u) quant_step(a[u], ks + u);
    }
  }
  for (; ks < f1; ++ks) {
    const bf16x8 a = *(const bf16x8*)(xrow + ks * 32);
    const bf16x8 b = *(const bf16x8*)(wrow + ks * 32);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    if (quant) quant_step(a, ks);
  }
  if (ks < s1) {                                  // the ragged last step (D % 32 != 0, so no quantised output): pieces past D are zero
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool in = ks * 32 + 8 * g < D;
    const bf16x8 a = in ? *(const bf16x8*)(xrow + ks * 32) : z;
    const bf16x8 b = in ? *(const bf16x8*)(wrow + ks * 32) : z;
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }

  // ---- the four partial tiles, summed in wave order, rounded once
#pragma unroll
  for (int j = 0; j < 4; ++j) S.part[wave][4 * g + j][i16] = acc[j];
  __syncthreads();
  {
    const int r = tid >> 4, c = tid & 15;
    const float v = ((S.part[0][r][c] + S.part[1][r][c]) + S.part[2][r][c]) + S.part[3][r][c];
    const bf16 lv = (bf16)v;
    const int e = cb * 16 + c;
    if (ncb == 1) S.lg[r][c] = (float)lv;
    if (r < rows && e < E) logits[(int64_t)(row0 + r) * E + e] = lv;
  }
  if (ncb > 1) {
    // hand-off 1: the last column block of this row block to arrive selects its rows
    if (!arrive_last(cnt + 1 + rb, ncb, S)) return;
    const bf16* src = logits + (int64_t)row0 * E;                // the rows of a row block are one contiguous range
    for (int i = tid; i < rows * E; i += 64 * DR_WAVES) S.lg[i / E][i % E] = (float)src[i];
  }
  __syncthreads();

  // ---- selection: one wave per row, the routines (and so the bits) of router_select_kernel; the ids go to LDS
  for (int r = wave; r < rows; r += DR_WAVES) {
    float s[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int e = lane + 64 * v;
      s[v] = e < E ? S.lg[r][e] : -INFINITY;
    }
    const int64_t t = row0 + r;
    float* sm_row = softmax ? softmax + t * E : nullptr;
    int32_t* idx_row = S.ids + r * K;
    float* w_row = w + t * K;
    if (mode == CSMOE_SEL_TEMP_SOFTMAX_TOPK)
      select_row_temp<VPL>(s, lane, E, K, round_sum_bf16, sel_param, CSMOE_BF16, sm_row, idx_row, w_row);
    else if (mode == CSMOE_SEL_SIGMOID_NORM)
      select_row_signorm<VPL>(s, lane, E, K, round_sum_bf16, CSMOE_BF16, sm_row, idx_row, w_row);
    else
      select_row<VPL>(s, lane, E, K, mode, round_sum_bf16, sel_param, CSMOE_BF16, sm_row, idx_row, w_row);
  }
  __syncthreads();
  for (int i = tid; i < rows * K; i += 64 * DR_WAVES) idx[(int64_t)row0 * K + i] = S.ids[i];
  const int n = T * K;
  if (nrb > 1) {
    // hand-off 2: the last row block to arrive sorts the ids of the whole call
    if (!arrive_last(cnt, nrb, S)) return;
    for (int i = tid; i < n; i += 64 * DR_WAVES) S.ids[i] = idx[i];
  }

  // ---- bins: the stable counting sort of csmoe_bin_tokens over the n <= 1024 ids in LDS; ids outside [0, E) are skipped as
  // bin_hist_kernel / bin_scatter_kernel skip them, and never index the histogram
  for (int i = tid; i < E; i += 64 * DR_WAVES) S.running[i] = 0;
  for (int i = tid; i < DR_WAVES * DR_EMAX; i += 64 * DR_WAVES) (&S.wcnt[0][0])[i] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 64 * DR_WAVES) {
    const int e = S.ids[i];
    if (e >= 0 && e < E) atomicAdd(&S.running[e], 1);
  }
  __syncthreads();
  {
    const int c = tid < E ? S.running[tid] : 0;                  // E <= 256: one expert per thread
    const int inc = wave_incl_scan(c, lane);
    if (lane == 63) S.wtot[wave] = inc;
    __syncthreads();
    int excl = inc - c;
    for (int w2 = 0; w2 < wave; ++w2) excl += S.wtot[w2];
    if (tid < E) {
      counts[tid] = c;
      offsets[tid] = excl;
      S.running[tid] = excl;
    }
    if (tid == 64 * DR_WAVES - 1) offsets[E] = excl + c;
  }
  __syncthreads();
  int ebits = 0;
  while ((1 << ebits) < E) ++ebits;
  for (int base = 0; base < n; base += 64 * DR_WAVES) {
    const int j = base + tid;
    int e = j < n ? S.ids[j] : -1;
    const bool valid = e >= 0 && e < E;
    if (!valid) e = -1;
    unsigned long long mask = __ballot(valid);                   // lanes of this wave holding the same expert
    for (int b = 0; b < ebits; ++b) {
      const unsigned long long bm = __ballot((e >> b) & 1);
      mask &= ((e >> b) & 1) ? bm : ~bm;
    }
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    const int cntw = __popcll(mask);
    if (valid && rank == cntw - 1) S.wcnt[wave][e] = cntw;       // one writer per (wave, expert)
    __syncthreads();
    if (valid) {
      int pos = S.running[e] + rank;
      for (int w2 = 0; w2 < wave; ++w2) pos += S.wcnt[w2][e];
      perm[pos] = j;
      slot_of[j] = pos;
    }
    __syncthreads();
    for (int i = tid; i < E; i += 64 * DR_WAVES) {
      S.running[i] += S.wcnt[0][i] + S.wcnt[1][i] + S.wcnt[2][i] + S.wcnt[3][i];
      S.wcnt[0][i] = 0; S.wcnt[1][i] = 0; S.wcnt[2][i] = 0; S.wcnt[3][i] = 0;
    }
    __syncthreads();
  }
}

}  // namespace

bool k_decode_route_ok(int T, int D, int E, int K, int dtype, int want_quant) {
  return dtype == CSMOE_BF16 && T >= 1 && K >= 1 && K <= 64 && K <= E && E <= DR_EMAX && (int64_t)T * K <= DR_NMAX && D > 0 &&
         D % 8 == 0 && (!want_quant || D % 32 == 0);
}

// the arrival counters: [0] the call's, [1 + rb] row block rb's; a block of its own, a multiple of 16 bytes, zeroed as a whole
int64_t k_decode_route_workspace_bytes(int T) {
  const int64_t nrb = T > 0 ? ((int64_t)T + 15) / 16 : 0;
  return (4 * (1 + nrb) + 15) & ~(int64_t)15;
}

int k_decode_route(const void* x, const void* wg, int T, int D, int E, int K, int mode, int round_sum_bf16, float sel_param, void* logits,
                   float* softmax, int32_t* idx, float* w, int32_t* counts, int32_t* offsets, int32_t* perm, int32_t* slot_of, void* xq,
                   void* xs, void* workspace, hipStream_t st) {
  const dim3 grid((E + 15) / 16, (T + 15) / 16), block(64 * DR_WAVES);
  if (grid.x > 1 || grid.y > 1) {
    const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)k_decode_route_workspace_bytes(T), st);
    if (e != hipSuccess) {
      csmoe_set_error("decode_route: zeroing the arrival counters failed: %s", hipGetErrorString(e));
      return CSMOE_ERR_LAUNCH;
    }
  }
#define DR_LAUNCH(VPL)                                                                                                              \
  hipLaunchKernelGGL((decode_route_kernel<VPL>), grid, block, 0, st, (const bf16*)x, (const bf16*)wg, T, D, E, K, mode, round_sum_bf16, \
                     sel_param, (bf16*)logits, softmax, idx, w, counts, offsets, perm, slot_of, (uint8_t*)xq, (uint8_t*)xs,            \
                     (int32_t*)workspace)
  if (E <= 64) DR_LAUNCH(1);
  else if (E <= 128) DR_LAUNCH(2);
  else DR_LAUNCH(4);
#undef DR_LAUNCH
  CSMOE_CHECK_LAUNCH("decode_route");
  return CSMOE_OK;
}
