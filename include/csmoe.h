/* csmoe.h -- C ABI of the MI355X-native (gfx950) sparse-MoE hot path for CompeteSMoE.
 *
 * Drop-in boundary: the reference hides this path behind Python nn.Module classes
 * (`moe_model/model/moe/` and `moe_pretrain_model/layers/moe/`) whose only native code is the two
 * Triton kernels of `moe_pretrain_model/layers/cvmm.py`.  Every entry point below replaces a piece of
 * that path and cites it.  The host side (`competesmoe_amd/`) keeps the reference's module / registry
 * surface and calls these functions through ctypes with raw device pointers -- no torch types cross
 * this boundary.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless marked host; tensors are dense row-major;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); nothing synchronises;
 *   - `dtype` is CSMOE_F32 or CSMOE_BF16 (the activation / weight storage type; accumulation is fp32);
 *   - T tokens, D model dim, F expert hidden dim, E experts, K selected per token, n = T*K binned rows;
 *   - "binned row space": rows sorted by expert (stable counting sort), expert e owns rows
 *     [offsets[e], offsets[e+1]);
 *   - return value: 0 on success, CSMOE_ERR_* otherwise; csmoe_last_error() gives the message.
 */
#ifndef CSMOE_H
#define CSMOE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* csmoe_stream_t;

enum { CSMOE_F32 = 0, CSMOE_BF16 = 1 };
enum { CSMOE_ACT_NONE = 0, CSMOE_ACT_RELU = 1, CSMOE_ACT_GELU = 2, CSMOE_ACT_GELU_TANH = 3, CSMOE_ACT_SILU = 4,
       CSMOE_ACT_QUICK_GELU = 5 /* x * sigmoid(1.702 x): CLIP towers (clip_smoe.py CLIPMLP, hidden_act "quick_gelu") */ };
enum { CSMOE_OK = 0, CSMOE_ERR_INVALID = 1, CSMOE_ERR_LAUNCH = 2, CSMOE_ERR_UNSUPPORTED = 3 };

/* Router selection rule (what top-k runs on, how the K weights are normalised). */
enum {
  CSMOE_SEL_SOFTMAX = 0,  /* softmax(fp32) -> topk -> w/sum          moe_model/model/moe/moe.py:129-130, smoe.py:44      */
  CSMOE_SEL_RAW = 1,      /* topk on raw scores -> w/sum (competition) moe_model/model/moe/competesmoe.py:253-255          */
  CSMOE_SEL_TOPK_SOFTMAX = 2, /* topk(logits) -> softmax over the K  moe_pretrain_model/layers/moe/deepseekv2.py:140-142 */
  CSMOE_SEL_SIGMOID = 3,  /* topk(sigmoid in the scores' dtype) -> w/(fp32 sum+1e-20), fp32 quotient (under CUDA autocast `sum` is an
                             fp32-policy op)                          moe_pretrain_model/layers/moe/deepseekv3.py:147-151 */
  CSMOE_SEL_TOPK_SIGMOID = 4, /* topk(logits) -> sigmoid(v / sel_param) -> w/sum   (`norm_sigmoid` + `scale_weight`,
                                moe_pretrain_model/layers/moe/competesmoe.py:476-483)                                    */
  CSMOE_SEL_TEMP_SOFTMAX_TOPK = 5 /* p = softmax(fp32) of (score / sel_param rounded to the scores' dtype) -> topk(p) -> softmax over
                                the K values; the `softmax` output holds p.  `round_sum_bf16` is a set of CSMOE_TEMP_* flags here
                                (XMoE: moe_model/model/moe/xmoe.py:90-91, 48-51; moe_pretrain_model/layers/moe/xmoe.py:161-162) */
  ,
  CSMOE_SEL_SIGMOID_NORM = 6 /* topk(sigmoid in the scores' dtype) -> w / den, den = the fp32 K-sum in slot order, rounded to bf16
                                under `round_sum_bf16` (`.to(x.dtype)`).  No epsilon and no guard: a row whose K keys are all zero
                                divides by zero exactly as the reference does (NaN weights).  The quotient is fp32, except that bf16
                                scores WITH `round_sum_bf16` make both operands bf16 tensors and the quotient a bf16 tensor op: w then
                                holds bf16 values (the array stays fp32).  `softmax` is the fp32 softmax of the scores.
                                (MoEUT's sigmoid gate: moe_model/model/moe/smoe_sigmoidgating.py:33-42;
                                moe_pretrain_model/layers/moe/smoeut_norm.py:112-125) */
};
/* Rounding points of the cosine router (flags; the first two are SEL_TEMP_SOFTMAX_TOPK's `round_sum_bf16`). */
enum {
  CSMOE_TEMP_P_BF16 = 1,    /* p is cast to bf16 before the top-K (`.to(x.dtype)` of a bf16 module)                          */
  CSMOE_TEMP_W_BF16 = 2,    /* the softmax over the K keys is a bf16 tensor op                                                */
  CSMOE_COS_OPER_BF16 = 4,  /* the cosine product's operands are rounded to bf16 (`matmul` under bf16 autocast)              */
  CSMOE_COS_NORM_THETA = 8, /* perturbed cosine: the row is reduced / (||reduced|| + theta), no clamp; `eps` carries theta    */
  CSMOE_COS_NORM_BF16 = 16  /* with NORM_THETA: the norm and `norm + theta` are bf16 tensors (a bf16 module without autocast) */
};

/* Combine rounding rule. */
enum {
  CSMOE_COMBINE_SEQ = 0,  /* LLaVA compute_moe: experts visited in index order, accumulator rounded to the
                             activation dtype after every add (moe_model/model/moe/moe.py:204)                        */
  CSMOE_COMBINE_DOT = 1,  /* cvmm reduction_weight: one fp32 dot over K, rounded once
                             (moe_pretrain_model/layers/cvmm.py:481-483)                                              */
  CSMOE_COMBINE_SEQ_RW = 2 /* as SEQ, but the product w*y is rounded to the activation dtype before the add: the
                             competition branch hands compute_moe weights already in x.dtype
                             (moe_model/model/moe/competesmoe.py:253-255 -> moe.py:204)                               */
};

/* GEMM operand layouts for the grouped expert GEMMs. */
enum {
  CSMOE_B_NK = 0,  /* per-expert B stored [N, Kd] (nn.Linear weight: y = a @ B^T)  */
  CSMOE_B_KN = 1   /* per-expert B stored [Kd, N] (cvmm keys/values: y = a @ B)    */
};

/* Epilogues of the row-space grouped GEMM. */
enum {
  CSMOE_EPI_PLAIN = 0,     /* C = round(acc)                                                         */
  CSMOE_EPI_BIAS = 1,      /* C = round(acc + bias_e[n])                                            */
  CSMOE_EPI_BIAS_ACT = 2,  /* C = round(acc + bias_e[n]);  C2 = round(act(C))   (bias may be null; C may be null when only
                              the activated output is kept: for ReLU act'(pre) = (act(pre) > 0), so ACTGRAD takes C2 as aux) */
  CSMOE_EPI_ACTGRAD = 3,   /* C = round(round(acc) * act'(aux[m,n]))             (GELU/ReLU backward) */
  CSMOE_EPI_ROUND_BIAS32_ACT = 4 /* u = round(acc) + bias_e[n] with an FP32 bias table; C = round(u) (may be null); C2 = round(act(u)):
                              the pretrain stack's `scores = cvmm(...) + bias[sel]` under autocast -- the cvmm output is already
                              rounded to bf16, the fp32 master bias promotes the sum to fp32, the activation runs on that and the
                              next cvmm rounds once more (moe_pretrain_model/layers/moe/moe.py:400-405) */
  ,
  /* The competition pass without its [T,E,D] outputs (csmoe_dense_gemm only, bf16 fast path; `act` carries two flags: bit 0 =
   * precise expf / log1pf, bit 1 = every softplus value / the row scale's product is rounded to bf16 as x.dtype tensor ops do):
   *   SOFTPLUS_ROWSUM: y = round(acc + bias[n]) is never stored; C is an FP32 table [M, ceil(N/256)] (ldc = its row stride) that
   *                    receives sum_n softplus(y[m,n]) over each 256-column tile -- `torch.mean(F.softplus(expert(x)), dim=-1)`
   *                    (moe_model/model/moe/competesmoe.py:240-243) is the row sum of that table over D (csmoe_affinity_finish);
   *   SOFTPLUS_GRAD:   C[m,n] = round(g[m] * sigmoid(y[m,n])), g[m] = aux[m] / N (rounded to bf16 under bit 1) with aux an FP32
   *                    vector [M] = d affinity[m]: the gradient of that mean with respect to y, from a recomputed y (autograd of
   *                    the same lines). */
  CSMOE_EPI_SOFTPLUS_ROWSUM = 5,
  CSMOE_EPI_SOFTPLUS_GRAD = 6,
  /* C[m,n] = round(round(scale[m] * round(acc)) * act'(aux[m,n])) with scale an FP32 vector [M] passed in the C2 slot: the
   * backward of the pretrain stack's weighted cvmm, which multiplies by the reduction weight AFTER the product has been rounded --
   * `grad_x_full = cvmm(grad_output, ..)` (unscaled, bf16), then `reduction_weight @ grad_x_full`
   * (moe_pretrain_model/layers/cvmm.py:527-543) -- so A holds the UNSCALED upstream rows.  (csmoe_grouped_gemm)
   * Optional dot table in the bias slot (every bias_ptrs[e] the SAME FP32 table [M][csmoe_grouped_gemm_rowdot_cols(..)]): receives
   * partial sums over column groups of round(acc)[m,n] * aux[m,n]; their row sums (csmoe_affinity_finish with D = 1) are the gradient
   * of the reduction weights as the reference forms it, `grad_x_full @ x` (cvmm.py:544) -- meaningful when aux is the activated
   * input of the second product (ReLU experts). */
  CSMOE_EPI_ACTGRAD_ROWSCALE = 7,
  /* C[m,n] = round(C[m,n] + round(acc)) in bf16 (C += acc in fp32): the product is ADDED to what C holds -- bit for bit
   * `C.add_(A @ B)` of two bf16 tensors, the running sum of the competition backward's per-expert dX chain
   * (moe_pretrain_model/layers/moe/competesmoe.py:395-401 under autograd).  C is read in the epilogue (16-byte loads issued
   * before the tile is staged through LDS), each tile is owned by one workgroup: no atomics, deterministic.  csmoe_dense_gemm only,
   * on every kernel it can select (bias, C2 and aux must be null; ldc >= N); csmoe_grouped_gemm, csmoe_grouped_gemm_f32w and the
   * MXFP8 entry points return CSMOE_ERR_UNSUPPORTED for it before launching anything, so C is never half-written. */
  CSMOE_EPI_ACCUM = 8
};

int csmoe_version(void);
const char* csmoe_last_error(void);
/* Number of compute units / name of the device `stream` belongs to (host ints). */
int csmoe_device_info(int* n_cu, int* lds_bytes, char* name, int name_len);

/* ---- router ------------------------------------------------------------------------------------------
 * gate projection  logits[T,E] = x[T,D] @ w_gate[E,D]^T, rounded to `dtype`
 * replaces `self.gate(x)` (moe_model/model/moe/smoe.py:42, competesmoe.py:314) and
 * `F.linear(x, self.w_gate)` (moe_pretrain_model/layers/moe/moe.py:121). */
int csmoe_gate_logits(const void* x, const void* w_gate, void* logits, int T, int D, int E, int dtype,
                      csmoe_stream_t stream);

/* scores[T,E] (dtype) -> softmax[T,E] fp32 (of the scores), idx[T,K] int32 (descending value, ties ->
 * lowest index), w[T,K] fp32.  `round_sum_bf16` != 0 rounds the K-sum to bf16 before the division
 * (`.to(x.dtype)` on the denominator, smoe.py:44).  softmax may be null for SEL_TOPK_SOFTMAX/SIGMOID.
 * `sel_param`: the scale of SEL_TOPK_SIGMOID (args.scale_weight), the temperature of SEL_TEMP_SOFTMAX_TOPK, ignored by the other
 * rules.  SEL_SIGMOID_NORM as the reference reaches it: fp32 scores, round_sum_bf16 = 0 (fp32 modules); bf16 scores, 1 (a bf16
 * module, a bf16 stream: bf16 quotient); bf16 scores, 0 (bf16 autocast on an fp32 stream: `sum` is fp32-policy, fp32 quotient).
 * replaces topk_expert + renorm (moe_model/model/moe/moe.py:113-132; smoe.py:19-44;
 * competesmoe.py:246-255; pretrain smoe.py:123-143, deepseekv2.py:140-142, deepseekv3.py:147-151). */
int csmoe_router_select(const void* scores, int dtype, int T, int E, int K, int sel_mode, int round_sum_bf16,
                        float sel_param, float* softmax, int32_t* idx, float* w, csmoe_stream_t stream);

/* backward of csmoe_router_select: given dw[T,K] (fp32) and optional dsoftmax[T,E] (fp32, from the aux
 * losses), produce dscores[T,E] in `dtype`.  (autograd of the same reference lines.) */
int csmoe_router_select_bwd(const void* scores, int dtype, int T, int E, int K, int sel_mode, int round_sum_bf16,
                            float sel_param, const float* softmax, const int32_t* idx, const float* w, const float* dw,
                            const float* dsoftmax, void* dscores, csmoe_stream_t stream);

/* ---- binning -----------------------------------------------------------------------------------------
 * Stable counting sort of idx[n] (expert id per (token,k) slot, n = T*K) into the binned row space.
 *   counts[E], offsets[E+1]; perm[n]: flat (t*K+k) held by binned row m; slot_of[n]: binned row of flat j.
 * `workspace` must hold csmoe_bin_workspace_bytes(n, E) bytes.
 * replaces cvmm_prepare_sel2's sort (moe_pretrain_model/layers/cvmm.py:580-593) and the E `torch.where`
 * scans of compute_moe (moe_model/model/moe/moe.py:189-191). */
int64_t csmoe_bin_workspace_bytes(int n, int E);
int csmoe_bin_tokens(const int32_t* idx, int n, int E, int32_t* counts, int32_t* offsets, int32_t* perm,
                     int32_t* slot_of, void* workspace, csmoe_stream_t stream);

/* the same sort from a histogram built elsewhere (csmoe_gate_select): block_hist[nb][E] counts the ids of
 * [b*chunk, (b+1)*chunk), nb = ceil(n / chunk); block_base[nb][E] is scratch.  Same outputs as csmoe_bin_tokens. */
int csmoe_bin_tokens_hist(const int32_t* idx, int n, int E, int chunk, const int32_t* block_hist, int32_t* block_base,
                          int32_t* counts, int32_t* offsets, int32_t* perm, int32_t* slot_of, csmoe_stream_t stream);

/* ---- one-pass router -----------------------------------------------------------------------------------
 * csmoe_gate_logits + csmoe_router_select (+ the counting pass of csmoe_bin_tokens) in ONE launch that reads x once:
 *   logits[T,E] (dtype) = x[T,D] @ w_gate[E,D]^T;  softmax[T,E] fp32 (nullable), idx[T,K], w[T,K] as csmoe_router_select
 *   gives them on those logits (identical bits: same selection routine);  block_hist (nullable): [ceil(T / rows)][E] counts of
 *   the ids of each block of csmoe_gate_select_rows() token rows, i.e. chunk = rows*K for csmoe_bin_tokens_hist.
 * Shapes it takes: csmoe_gate_select_ok(...) = 1 (bf16, E <= 64, D % 8 == 0); others use the two separate entries.
 * Rules it takes: SEL_SOFTMAX .. SEL_TOPK_SIGMOID and SEL_SIGMOID_NORM (SEL_TEMP_SOFTMAX_TOPK is csmoe_cosine_select's).
 * replaces `self.gate(x)` + `topk_expert` (moe_model/model/moe/smoe.py:42-44, moe.py:113-132) and `F.linear(x, w_gate)` + top-k
 * (moe_pretrain_model/layers/moe/moe.py:121, smoe.py:30-40, deepseekv2.py:140-142). */
int csmoe_gate_select_ok(int T, int D, int E, int K, int dtype);
int csmoe_gate_select_rows(void);
int csmoe_gate_select(const void* x, const void* w_gate, int T, int D, int E, int K, int sel_mode, int round_sum_bf16,
                      float sel_param, int dtype, void* logits, float* softmax, int32_t* idx, float* w, int32_t* block_hist,
                      csmoe_stream_t stream);

/* ---- decode front end ------------------------------------------------------------------------------------
 * Route, bin and quantise the tokens of a decode call (T * K <= 1024 routed rows) in ONE launch that reads x once:
 *   logits[T,E] (bf16), softmax[T,E] fp32 (nullable), idx[T,K], w[T,K]: the meaning of csmoe_gate_select.  The logits are the fp32
 *     sum over D (v_mfma_f32_16x16x32_bf16, K dealt to four waves, partials added in wave order) rounded to bf16 once: within
 *     2^-7 * max(|ref|, 2^-6) of csmoe_gate_logits, bit-identical from run to run (no float atomics).  softmax / idx / w are the bits
 *     csmoe_router_select gives on THESE logits, for every rule 0..6 (`sel_param` / `round_sum_bf16` as there).
 *   counts[E], offsets[E+1], perm[n], slot_of[n], n = T*K: csmoe_bin_tokens of this idx (ids outside [0, E) skipped as there).
 *   xq[T,D], xs[T,D/32] uint8 (both or neither): the bytes csmoe_quantize_mxfp8 writes for x, rows orientation.
 * `workspace`: csmoe_decode_route_workspace_bytes(T) bytes, 16-byte aligned (arrival counters of the in-launch hand-offs; zeroed by
 * the call on `stream`, so the call is capturable and one buffer serves every call on that stream).
 * Shapes it takes: csmoe_decode_route_ok(...) = 1: bf16, T >= 1, T*K <= 1024, 1 <= K <= min(E, 64), E <= 256, D % 8 == 0, and
 * D % 32 == 0 with `want_quant`; x, w_gate and xq 16-byte aligned.
 * Returns CSMOE_ERR_INVALID for bad arguments (K > E, an unknown rule, xq without xs, null operands) and CSMOE_ERR_UNSUPPORTED for a
 * shape or alignment the rule rejects, both before any pointer is read and before anything is launched; T == 0 is CSMOE_OK.
 * replaces `self.gate(x)` + `topk_expert` (moe_model/model/moe/smoe.py:42-44, moe.py:113-132), the E `torch.where` scans of
 * compute_moe (moe.py:189-191), `F.linear(x, self.w_gate)` (moe_pretrain_model/layers/moe/moe.py:121) and cvmm_prepare_sel2's sort
 * (moe_pretrain_model/layers/cvmm.py:580-593); the quantised rows have no counterpart upstream (the reference has no fp8). */
int csmoe_decode_route_ok(int T, int D, int E, int K, int dtype, int want_quant);
int64_t csmoe_decode_route_workspace_bytes(int T);
int csmoe_decode_route(const void* x, const void* w_gate, int T, int D, int E, int K, int sel_mode, int round_sum_bf16,
                       float sel_param, int dtype, void* logits, float* softmax, int32_t* idx, float* w, int32_t* counts,
                       int32_t* offsets, int32_t* perm, int32_t* slot_of, void* xq, void* xs, void* workspace,
                       csmoe_stream_t stream);

/* ---- one-pass cosine router (XMoE) ----------------------------------------------------------------------
 * `inp_reduction(x)` + `_cosine` + `_make_finite` + softmax(logits / temperature) + `_keepTopk` (+ the counting pass of
 * csmoe_bin_tokens) of moe_model/model/moe/xmoe.py:80-91 / moe_pretrain_model/layers/moe/xmoe.py:143-162 in ONE launch that reads
 * x once, followed by a one-workgroup patch launch that returns at once unless a row was non-finite.  With R = E / 2:
 *   reduced[T,R] (dtype) = x[T,D] @ w_red[R,D]^T: the bits csmoe_gate_logits gives (a layer with `sel_bias` uses the separate entries);
 *   logits[T,E] (dtype)  = (reduced / max(||reduced||, eps)) @ emb[E,R]^T, fp32 over ascending r (operands rounded to bf16 first
 *                          under CSMOE_COS_OPER_BF16); `emb` is the fp32 copy of the (already renormalised) expert embeddings;
 *                          under CSMOE_COS_NORM_THETA (`smoe_perturbed`) the row is reduced / (||reduced|| + eps) instead, `eps`
 *                          carrying theta, no clamp: a zero row gives E zero logits; with CSMOE_COS_NORM_BF16 the norm and the sum
 *                          are rounded to bf16 (n = bf16(sqrt(sum v^2)), den = bf16(n + theta)), the division stays fp32;
 *   p[T,E] fp32, idx[T,K], w[T,K] = csmoe_router_select(logits, SEL_TEMP_SOFTMAX_TOPK, flags & 3, temperature): identical bits;
 *   block_hist (nullable) as csmoe_gate_select (rows per block: csmoe_gate_select_rows()).
 * A row whose logits are not finite is routed from E equal values (experts 0..K-1, weights 1/K); its stored logits become the
 * smallest finite logit of the whole tensor (what `_make_finite` assigns) in the patch launch.  `work` holds
 * csmoe_cosine_select_work_ints(T) int32: [0] = number of non-finite rows of this call (written by the patch launch), the rest
 * per-workgroup scratch.  No host synchronisation.
 * Shapes it takes: csmoe_cosine_select_ok(...) = 1 (bf16, E even, E <= 64, D % 8 == 0). */
int csmoe_cosine_select_ok(int T, int D, int E, int K, int dtype);
int64_t csmoe_cosine_select_work_ints(int T);
int csmoe_cosine_select(const void* x, const void* w_red, const float* emb, int T, int D, int E, int K,
                        int flags, float temperature, float eps, int dtype, void* reduced, void* logits, float* p, int32_t* idx,
                        float* w, int32_t* block_hist, int32_t* work, csmoe_stream_t stream);

/* backward of the row half of csmoe_cosine_select (autograd of the same reference lines, rounding where its ops round):
 * dw[T,K] fp32, dp[T,E] fp32 (nullable: the balance loss), dlogits[T,E] `dtype` (nullable: z-loss / entropy balance) ->
 * d_reduced[T,R] (dtype) and d_emb[E,R] fp32 (gradient w.r.t. `emb`; under CSMOE_COS_OPER_BF16 the caller rounds it to bf16 as the
 * reference's bf16 matmul backward does).  `part` holds csmoe_cosine_select_bwd_parts(T) * E * R fp32 partial tables summed in a
 * fixed order (a second launch): deterministic, no floating-point atomics.  `logits` are the stored (patched) ones: rows that were
 * non-finite carry E equal logits and route uniformly, exactly as the reference's.  Under CSMOE_COS_NORM_THETA d_reduced is the
 * bf16 sum of two bf16 gradients, as the engine adds them: d m / den (the `.float()` cast) and the norm's d den * (v / n), zero
 * where n == 0, computed in bf16 under CSMOE_COS_NORM_BF16 and in fp32 with one rounding otherwise. */
int csmoe_cosine_select_bwd_parts(int T);
int csmoe_cosine_select_bwd(const void* reduced, const float* emb, const void* logits, const int32_t* idx, const float* w,
                            const float* dw, const float* dp, const void* dlogits, int T, int E, int K, int flags,
                            float temperature, float eps, int dtype, void* d_reduced, float* d_emb, float* part,
                            csmoe_stream_t stream);

/* aff[m] = (sum_j partial[m, j]) / D in `aff_dtype` (bf16 or fp32): closes CSMOE_EPI_SOFTPLUS_ROWSUM; `aff` is strided
 * (element stride `aff_stride`) so that expert e's column of an affinity matrix [T, E] is written in place. */
int csmoe_affinity_finish(const float* partial, int M, int ntiles, int D, void* aff, int64_t aff_stride, int aff_dtype,
                          csmoe_stream_t stream);

/* ---- dispatch / combine ------------------------------------------------------------------------------
 * dispatch: xs[m,:] = x[perm[m] / K, :]                      (gather of x rows, moe.py:201 `x[batch_idx, token_idx]`;
 *                                                             cvmm.py:114-119 remap_offs_am) */
int csmoe_dispatch_rows(const void* x, const int32_t* perm, int K, void* xs, int n, int D, int dtype,
                        csmoe_stream_t stream);
/* token-major dispatch (same result; reads every x row from HBM once): xs[slot_of[t*K+k], :] = x[t, :] */
int csmoe_dispatch_tokens(const void* x, const int32_t* slot_of, int K, void* xs, int T, int D, int dtype,
                          csmoe_stream_t stream);
/* Kernel choice of the two dispatch entries: 1 = the 16-byte vector copy (x and xs 16-byte aligned, rows a multiple of 16 bytes),
 * 0 = the 2-byte copy.  Both copy the same bytes. */
int csmoe_dispatch_vec_ok(const void* x, const void* xs, int D, int dtype);
/* dispatch backward: dx[t,:] = round(round(sum_k dxs[slot_of[t*K+k], :]) + add[t,:])  (add may be null): the K-sum in fp32, rounded
 * once -- CVMM.backward's reduction (cvmm.py:544-545) and, for K <= 2, the LLaVA stack's autograd.
 * `idx` [T,K] != null selects what autograd does for the LLaVA stack's per-expert modules (moe.py:196-204): every expert's `x[...]`
 * is its own use of x, the engine runs their backward nodes last-created first and adds each result into the leaf's buffer in
 * x.dtype -- dx[t] = (((pre[t] + dxs[slot of the HIGHEST expert]) + ...) + dxs[slot of the lowest]) + add[t], rounded after every
 * add.  `pre` [T,D] (may be null) = a gradient stream that reached x before the experts' (the always-on expert of smoe_share /
 * deepseekv3, shard_smoe.py:53, created after the routed experts); `add` = one that arrives after them (the gate's). */
int csmoe_dispatch_rows_bwd(const void* dxs, const int32_t* slot_of, int K, const void* add, void* dx, int T, int D,
                            int dtype, const int32_t* idx, const void* pre, csmoe_stream_t stream);
/* combine: out[t,:] = sum_k w[t,k] * y[slot_of[t*K+k], :]  (+ obias[:] if non-null) with the rounding rule `mode`
 * (moe.py:204; cvmm.py:481-483).  idx gives the expert of each slot (visit order for COMBINE_SEQ).
 * `residual` [T,D] (may be null) is added last, as one more x.dtype addition: out = round(out + residual) -- the
 * `hidden_states = residual + results` of the block around the layer (siglip_smoe.py:155; relative_moe_transformer.py:161). */
int csmoe_combine(const void* y, const int32_t* slot_of, const int32_t* idx, const float* w, const void* obias,
                  const void* residual, void* out, int T, int K, int D, int dtype, int mode, csmoe_stream_t stream);
/* combine backward: dy[m,:] = round(w * dout[t,:]) in the binned row space; dw[t,k] = <dout[t,:], y[slot,:]>
 * (y may be null -> dw not written).  (autograd of moe.py:204; cvmm.py:497-499,543)
 * `round_products` != 0: dw[t,k] = round(sum_d round(dout[t,d] * y[slot,d])), every product and the sum rounded to `dtype` -- what
 * autograd returns for `weights * out_exp` when the weights are an x.dtype tensor (the competition step's affinity weights,
 * competesmoe.py:253-258 -> moe.py:204); 0: one fp32 dot product (fp32 weights: router steps, cvmm). */
int csmoe_combine_bwd(const void* dout, const void* y, const int32_t* perm, const int32_t* slot_of, const float* w,
                      void* dy, float* dw, int T, int K, int D, int dtype, int round_products, csmoe_stream_t stream);

/* ---- grouped expert GEMM -----------------------------------------------------------------------------
 * Row-space GEMM: for every expert e and binned row m in [offsets[e], offsets[e+1]):
 *     C[m, 0:N] = epilogue( A[m, 0:Kd] (x) B_e )
 * B_e = b_ptrs[e] is [N,Kd] (CSMOE_B_NK) or [Kd,N] (CSMOE_B_KN) with leading dimension ldb.
 * bias_ptrs[e] -> [N] or null; C2 / aux are [M,N] with ldc.  M = offsets[E] rows in total (upper bound `M`).
 * replaces cvmm_kernel (moe_pretrain_model/layers/cvmm.py:61-168, 354-398), the per-expert nn.Linear calls of
 * compute_moe (moe_model/model/moe/moe.py:196-204) and their grad-input (cvmm.py:519-536).
 * `kernel` (CSMOE_KERNEL_*): 0 = the library chooses (one-wave-per-SIMD 256x256 kernel for K-contiguous weights where the shape allows, else the 8-wave
 * 256x256 kernel, the 128x128 kernel for small / narrow problems, the generic kernel for fp32 and unaligned operands); 1 forces the
 * generic kernel; 2 / 4 ask for the 8-wave / one-wave-per-SIMD kernel where the shape allows (tests and A/B runs: every kernel is
 * reachable through the interface, none through hidden state).  A CSMOE_EPI_ACTGRAD_ROWSCALE launch that passes a dot table and
 * lands on a kernel that cannot fill it returns CSMOE_ERR_UNSUPPORTED instead of leaving the table unwritten; so does one whose
 * kernel would write a different table layout from the one csmoe_grouped_gemm_rowdot_cols reports for the shape (that function does
 * not take `kernel`: `kernel` = 2 / 4 below M = 2048 selects a 256x256 kernel where it reports the 128x128 kernel's N / 8 columns).
 * Both refusals come before anything is launched. */
#define CSMOE_KERNEL_AUTO 0
#define CSMOE_KERNEL_GENERIC 1
#define CSMOE_KERNEL_V2 2
#define CSMOE_KERNEL_V4 4
int csmoe_grouped_gemm(const void* A, int64_t lda, const void* const* b_ptrs, int b_layout, int64_t ldb,
                       const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd,
                       void* C, void* C2, const void* aux, int64_t ldc, int epilogue, int act, int dtype,
                       int kernel, csmoe_stream_t stream);

/* ---- few-row (decode) grouped GEMM ----------------------------------------------------------------------
 * The row-space product of csmoe_grouped_gemm for a call with FEW rows -- a model in use after training sees T = batch size tokens
 * per layer, i.e. 2 .. 32 routed rows over up to 64 experts -- where the launch is bound by the bytes of the active experts' weights:
 * 16-row tiles of one expert on v_mfma_f32_16x16x32_bf16, the weights streamed once per tile straight into registers
 * (csrc/gemm_skinny.hip).  Same semantics: for every expert e and binned row m in [offsets[e], offsets[e+1])
 *     C[m, 0:N] = epilogue( A[row(m), 0:Kd] (x) B_e ),   row(m) = src_rows ? src_rows[m] / src_div : m
 * with B_e = b_ptrs[e] [N,Kd] (CSMOE_B_NK) or [Kd,N] (CSMOE_B_KN), leading dimension ldb.  `src_rows` (int32 [M], may be null)
 * gathers on the A side: with bins.perm and K it reads the rows csmoe_dispatch_rows would have copied (`x[batch_idx, token_idx]`,
 * moe_model/model/moe/moe.py:201; cvmm.py:114-119), so a decode step has no dispatch copy.  Any M: an expert with more than 16 rows is
 * walked in 16-row blocks that each stream the weight slab again, which is why this entry is for few rows and CSMOE_KERNEL_AUTO
 * never selects it.  Forward epilogues only (PLAIN, BIAS, BIAS_ACT, ROUND_BIAS32_ACT; all six activations; C may be null when only
 * C2 is wanted), bf16 only.  Shape rule (csmoe_grouped_gemm_skinny_ok, a pure host query returning 0 / 1): N, Kd, lda, ldb, ldc
 * multiples of 8 (Kd need not be a multiple of 32, N not of 16), operands 16-byte aligned, panels under 2 GiB.
 * Returns CSMOE_ERR_INVALID for bad arguments; CSMOE_ERR_UNSUPPORTED for fp32, a backward or affinity epilogue, CSMOE_EPI_ACCUM or a
 * shape the rule rejects -- decided before any pointer is read and before anything is launched, so nothing is written; M == 0 is
 * CSMOE_OK.  K is split over the 8 waves of a workgroup and summed in wave order: no atomics, bit-identical from run to run.
 * replaces, for few rows: cvmm_kernel (moe_pretrain_model/layers/cvmm.py:61-168) and the per-expert nn.Linear calls of compute_moe
 * (moe_model/model/moe/moe.py:196-204) -- the path `generate` takes through the layer at decode time. */
int csmoe_grouped_gemm_skinny(const void* A, int64_t lda, const int32_t* src_rows, int src_div, const void* const* b_ptrs,
                              int b_layout, int64_t ldb, const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N,
                              int Kd, void* C, void* C2, int64_t ldc, int epilogue, int act, int dtype, csmoe_stream_t stream);
int csmoe_grouped_gemm_skinny_ok(int M, int N, int Kd, int64_t lda, int64_t ldb, int64_t ldc, int b_layout, int epilogue, int dtype);

/* partial sums per row written into the dot table of CSMOE_EPI_ACTGRAD_ROWSCALE for this launch shape; 0: no table (generic kernel) */
int csmoe_grouped_gemm_rowdot_cols(int M, int N, int Kd, int64_t lda, int64_t ldb, int64_t ldc, int dtype);

/* Dense (single weight matrix) form of the same kernel: C[M,N] = epilogue(A[M,Kd] (x) B), used for the gate projection and
 * the always-on shared expert (moe_model/model/moe/shard_smoe.py:53, deepseekv3.py:44; pretrain deepseekv2.py:154-165). */
int csmoe_dense_gemm(const void* A, int64_t lda, const void* B, int b_layout, int64_t ldb, const void* bias, int M, int N,
                     int Kd, void* C, void* C2, const void* aux, int64_t ldc, int epilogue, int act, int dtype,
                     int kernel, csmoe_stream_t stream);

/* Weight-gradient GEMM: for every expert e:  C_e[0:Na, 0:Nb] = sum_{m in expert e} A[m,0:Na]^T B[m,0:Nb]
 * c_ptrs[e] -> [Na, Nb] (leading dim ldc) written in `out_dtype` (CSMOE_F32 or CSMOE_BF16); empty experts get zeros.
 * Deterministic (no atomics).  `accumulate` != 0 adds into the existing C_e.
 * replaces cvmm_backward_kernel3 (cvmm.py:194-345, 421-457) and autograd's per-expert weight grads. */
int csmoe_grouped_wgrad(const void* A, int64_t lda, const void* B, int64_t ldb, const int32_t* offsets, int E, int M,
                        int Na, int Nb, void* const* c_ptrs, int64_t ldc, int dtype, int out_dtype, int accumulate,
                        int force_generic, const int32_t* xcd_order, csmoe_stream_t stream);
/* Load balance of the persistent weight-gradient kernel under skewed routing: experts dealt to the 8 XCDs by row count (rank r,
 * most rows first, goes to XCD r % 8 in snake order).  order: 8 * ceil(E / 8) + 1 int32, entry [x * ceil(E/8) + k] = k-th
 * expert of XCD x or -1.  Computed once per routing decision, passed as `xcd_order` (may be null: contiguous expert ranges). */
int csmoe_expert_order(const int32_t* offsets, int E, int32_t* order, csmoe_stream_t stream);

/* Row ranges of the E experts cut into P chunks each, out [E * P + 1]: out[e * P + j] = min(offsets[e] + roundup(count_e * j / P,
 * align), offsets[e + 1]), out[E * P] = offsets[E].  The chunks are handed to csmoe_grouped_wgrad / csmoe_grouped_colsum as
 * E * P pseudo-experts (split-K with fp32 partials) when E experts alone give too few workgroups for the chip -- the reference's
 * LLaVA configurations use 4 experts (sft.sh:19-20).  No counterpart upstream. */
int csmoe_chunk_offsets(const int32_t* offsets, int E, int P, int align, int32_t* out, csmoe_stream_t stream);

/* Dense form: C[Na,Nb] = A[M,Na]^T B[M,Nb]. */
int csmoe_dense_wgrad(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int Na, int Nb, void* C, int64_t ldc,
                      int dtype, int out_dtype, int accumulate, int force_generic, csmoe_stream_t stream);

/* Per-expert column sums (bias gradients): out_e[0:N] = sum_{m in e} G[m, 0:N]; out in `out_dtype`. */
int csmoe_grouped_colsum(const void* G, int64_t ldg, const int32_t* offsets, int E, int N, void* const* out_ptrs,
                         int dtype, int out_dtype, csmoe_stream_t stream);

int csmoe_dense_colsum(const void* G, int64_t ldg, int M, int N, void* out, int dtype, int out_dtype, csmoe_stream_t stream);

/* Router auxiliary losses of the LLaVA stack (moe.py:71-110): out2[0] = balance loss (fp32), out2[1] = z-loss (each step rounded
 * to x.dtype like the reference's tensor ops; 0 when logits == null).  softmax [B,N,E] fp32 = softmax of logits, idx [B,N,K]
 * (column 0 = top-1).  Keeps dens [B,E] (fraction of tokens whose top-1 is e) and lse [B*N] for the backward; workspace =
 * csmoe_router_aux_workspace_floats(B, N, E) floats.  Backward: dsoftmax (fp32, from d balance) and dlogits (x.dtype, from d z)
 * given the device scalars g_balance / g_z; either output may be null. */
int64_t csmoe_router_aux_workspace_floats(int B, int N, int E);
int csmoe_router_aux(const void* logits, const float* softmax, const int32_t* idx, float* lse, float* workspace, float* dens,
                     float* out2, int B, int N, int E, int K, int dtype, csmoe_stream_t stream);
int csmoe_router_aux_bwd(const float* softmax, const float* dens, const float* lse, const float* g_balance, const float* g_z,
                         float* dsoftmax, void* dlogits, int B, int N, int E, int dtype, csmoe_stream_t stream);

/* Gate backward for few experts (E <= 4, D a multiple of 8 (bf16) / 4 (fp32), 16-byte aligned rows; csmoe_gate_bwd_small_ok):
 * dx[T,D] = dlogits[T,E] @ w_gate[E,D] and the partial sums of dWg = dlogits^T @ x over csmoe_gate_bwd_dw_ranges(T, D, dtype)
 * row ranges (partial [nranges][E][D] fp32; their sum over the ranges -- csmoe_dense_colsum over [nranges, E*D] -- is dWg).
 * HBM-bound row passes replacing the MFMA GEMMs whose 128-wide tiles are empty at E = 4 (autograd of `self.gate(x)`, smoe.py:42;
 * csmoe_gate_logits switches to the matching forward kernel by itself). */
int csmoe_gate_bwd_small_ok(int D, int E, int dtype);
int csmoe_gate_bwd_dx(const void* dlogits, const void* w_gate, void* dx, int T, int D, int E, int dtype, csmoe_stream_t stream);
int csmoe_gate_bwd_dw_ranges(int T, int D, int dtype);
int csmoe_gate_bwd_dw(const void* dlogits, const void* x, float* partial, int T, int D, int E, int dtype, int nranges,
                      csmoe_stream_t stream);

/* diversity loss of the competition step (moe.py:133-171, competesmoe.py:180-218): tok_loss[t] = sum over ordered pairs
 * i != j of <y[t,i,:] / max(|y[t,i,:]|, 1e-12), y[t,j,:] / ...> (fp32), y = [T, K, D] selected expert outputs, K <= 8; the loss
 * is sum_t tok_loss[t] / (T*K*K).  Backward: dy = gscale[0] * d(sum_t tok_loss)/dy in x.dtype (gscale: device scalar). */
int csmoe_pair_cosine(const void* y, float* tok_loss, int T, int K, int D, int dtype, csmoe_stream_t stream);
int csmoe_pair_cosine_bwd(const void* y, const float* gscale, void* dy, int T, int K, int D, int dtype, csmoe_stream_t stream);

/* ---- the MoE half of a pre-LN block around the layer: out = x + MoE(LayerNorm(x))  (SURVEY.md section 8 f1;
 *      siglip_smoe.py:141-157 SiglipEncoderMoELayer.forward; relative_moe_transformer.py:153-161, preln) ----
 * LayerNorm over the last dimension with fp32 statistics (torch.nn.LayerNorm semantics): xn = (x - mean) * rstd * gamma + beta,
 * mean/rstd [T] fp32 are kept for the backward.  gamma / beta may be null.  With w_gate != null the router's gate projection is
 * computed from the rounded xn by the same call (second launch on the stream: the gate GEMM of csmoe_gate_logits reads the rows
 * the LayerNorm just wrote): logits[T,E] = xn @ w_gate^T (gate of moe.py:46 / F.linear(x, w_gate) moe.py:121).
 * D <= 4096, D % 8 == 0 (bf16) / D % 4 == 0 (fp32), 16-byte aligned operands. */
int csmoe_layernorm_gate(const void* x, const void* gamma, const void* beta, float eps, void* xn, float* mean, float* rstd,
                         int T, int D, int dtype, const void* w_gate, void* logits, int E, csmoe_stream_t stream);
/* LayerNorm backward: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dxn * gamma, xhat = (x - mean) * rstd.  With
 * dxn2 != null the gradient of xn is round(dxn + dxn2) (expert path + gate path, summed as autograd would).  With
 * add != null the residual-path gradient is added in the same pass: dx = round(dx) + add.  `partial` receives
 * csmoe_layernorm_bwd_blocks(T) rows of [2][D] fp32 (row sums of dxn * xhat and of dxn): their column sums (csmoe_dense_colsum)
 * are dgamma and dbeta -- deterministic, no atomics. */
int csmoe_layernorm_bwd(const void* dxn, const void* dxn2, const void* x, const void* gamma, const float* mean, const float* rstd,
                        const void* add, void* dx, float* partial, int T, int D, int dtype, csmoe_stream_t stream);
int csmoe_layernorm_bwd_blocks(int T);

/* ---- the same block with an fp32 residual stream around bf16 activations: the pretrain stack under bf16 autocast
 *      (relative_moe_transformer.py:153-161 inside simple_task.py:295's autocast).  There LayerNorm is an fp32 op on fp32 x with
 *      fp32 gamma / beta, its output is cast to bf16 by the gate's F.linear (moe.py:121) and by cvmm (cvmm.py:29-32), the bf16 MoE
 *      output is added to the fp32 residual in fp32 (type promotion), and in the backward autograd casts the fp32 gradient to
 *      bf16 for the MoE, casts the two bf16 gradients of xn back to fp32 and sums them.  These entries read and write the fp32
 *      stream directly (no cast passes): xn / logits / y / dy / dxn are bf16, x / residual / out / dout / dx are fp32.
 *      D <= 4096, D % 8 == 0, 16-byte aligned operands. */
int csmoe_layernorm_gate_mixed(const float* x, const float* gamma, const float* beta, float eps, void* xn, float* mean, float* rstd,
                               int T, int D, const void* w_gate, void* logits, int E, csmoe_stream_t stream);
/* dx = LayerNorm backward of (float(dxn) + float(dxn2)) [+ add], all sums in fp32 */
int csmoe_layernorm_bwd_mixed(const void* dxn, const void* dxn2, const float* x, const float* gamma, const float* mean,
                              const float* rstd, const float* add, float* dx, float* partial, int T, int D, csmoe_stream_t stream);
/* out[t] = float(round_bf16(combine of the bf16 rows y)) + residual[t]   (csmoe_combine with an fp32 residual / output) */
int csmoe_combine_mixed(const void* y, const int32_t* slot_of, const int32_t* idx, const float* w, const float* residual, float* out,
                        int T, int K, int D, int mode, csmoe_stream_t stream);
/* csmoe_combine_bwd with an fp32 upstream gradient, rounded to bf16 on load (the cast autograd would insert) */
int csmoe_combine_bwd_mixed(const float* dout, const void* y, const int32_t* slot_of, const float* w, void* dy, float* dw, int T, int K,
                            int D, csmoe_stream_t stream);
/* csmoe_dispatch_rows_bwd into the fp32 stream: dx[t,:] = float(round_bf16(sum_k dxs[slot_of[t*K+k], :])) + float(add[t,:]), the sum
 * of the two in fp32 -- what autograd leaves in an fp32 x under bf16 autocast when the experts (CVMM.backward's bf16 reduction,
 * cvmm.py:544-545) and the gate (F.linear's bf16 dx, moe.py:121) each read their own bf16 cast of x: every cast's backward widens
 * its bf16 gradient and the engine adds the fp32 streams.  dxs, add (may be null): bf16; D % 8 == 0, 16-byte aligned operands. */
int csmoe_dispatch_rows_bwd_mixed(const void* dxs, const int32_t* slot_of, int K, const void* add, float* dx, int T, int D,
                                  csmoe_stream_t stream);
/* out[i] = (float(a[i]) + float(b[i])) + float(c[i]), a / b / c bf16 (b, c may be null, in that order), n elements: the gradient an
 * fp32 x receives under bf16 autocast when several ops read it -- the gate's F.linear, the experts' cvmm, the shared expert
 * (moe.py:121, cvmm.py:29-32,445; deepseekv2.py:154-165) each cast x themselves, every cast's backward widens its bf16 stream and the
 * autograd engine adds the fp32 streams.  One pass over the streams; 16-byte aligned operands. */
int csmoe_widen_sum(const void* a, const void* b, const void* c, float* out, int64_t n, csmoe_stream_t stream);

/* ---- competition affinity ----------------------------------------------------------------------------
 * aff[r] = mean_d softplus(y[r, d])  (competesmoe.py:242; pretrain competesmoe.py:401) and its backward
 * dy[r,d] = round(daff[r] / D * sigmoid(y[r,d])) (+ dy_add if non-null).
 * `aff_dtype` == `dtype`: the LLaVA stack's x.dtype tensor ops (every softplus value rounded to dtype before the mean, the mean
 * rounded to dtype).  `aff_dtype` == CSMOE_F32 around bf16 rows: the pretrain stack under CUDA autocast, where F.softplus is an
 * fp32-policy op (simple_task.py:295 + torch's autocast table): softplus, mean and the affinities are fp32, daff is fp32 and the
 * gradient is rounded to bf16 once.  `precise` != 0 evaluates exp / log1p as torch does instead of with the hardware
 * approximations. */
int csmoe_softplus_mean(const void* y, void* aff, int R, int D, int dtype, int aff_dtype, int precise, csmoe_stream_t stream);
int csmoe_softplus_mean_bwd(const void* y, const void* daff, const void* dy_add, void* dy, int R, int D, int dtype, int aff_dtype,
                            int precise, csmoe_stream_t stream);

/* Row-space grouped GEMM with the weights read straight from FP32 MASTERS: A [M, Kd] bf16, B_e = b_ptrs[e] [Kd, N] FP32 (leading
 * dimension ldb), converted to bf16 inside the tile fill (global -> registers -> cvt -> LDS) -- what the reference's Triton kernel
 * does per tile (`a.to(tl.bfloat16)`, moe_pretrain_model/layers/cvmm.py:126-140, fp32 `keys` / `values` under bf16 autocast) instead of
 * a separate cast pass over the weights.  Bit-identical to "cast to bf16, then csmoe_grouped_gemm(CSMOE_B_KN)".  b_copy_ptrs[e]
 * (may be null) receives the bf16 copy [Kd, N] of every expert that has rows -- the operand of the step's two backward products;
 * experts without rows are not written.  Same epilogues, outputs and bias conventions as csmoe_grouped_gemm with dtype bf16.
 * N % 8 == 0, Kd % 8 == 0, 16-byte aligned rows (else CSMOE_ERR_UNSUPPORTED: cast and use csmoe_grouped_gemm). */
int csmoe_grouped_gemm_f32w(const void* A, int64_t lda, const void* const* b_ptrs, int64_t ldb, void* const* b_copy_ptrs,
                            const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd, void* C, void* C2,
                            const void* aux, int64_t ldc, int epilogue, int act, csmoe_stream_t stream);

/* ---- MXFP8 expert GEMMs (BASELINE.json config 5: shared-expert variant on the fp8 matrix pipe) -------------------------
 * The reference has no fp8 path: these entries have no upstream counterpart; the contract is the bf16 path's
 * result within the quantisation error (tests: <= 3e-2 relative to the bf16 oracle, <= 2e-3 to the oracle's own MXFP8 emulation).
 * Format: OCP e4m3 elements, one e8m0 scale (2^(s - 127)) per 32 consecutive elements ALONG THE REDUCTION dimension of the GEMM
 * that consumes the tensor; scale = 2^(floor(log2(amax)) - 8), elements round-to-nearest-even, saturated at +-448.
 *
 * csmoe_quantize_mxfp8: E matrices [R, C] (x_ptrs[e], or the single matrix x when x_ptrs == null and E == 1), leading dimension
 * ldx, dtype CSMOE_BF16 or CSMOE_F32 (fp32 master weights are quantised directly).  transpose == 0: q [E, R, C], s [E, R, C/32]
 * (blocks along C; C % 32 == 0).  transpose != 0: q [E, C, R], s [E, C, R/32] (blocks along R; R % 32 == 0) -- the operand of the
 * transposed product (dX = dY . W for a weight stored [N, K]). */
int csmoe_quantize_mxfp8(const void* x, const void* const* x_ptrs, int E, int64_t ldx, int R, int C, int dtype, int transpose,
                         void* q, void* s, csmoe_stream_t stream);
/* Gather and quantise in one pass: xs as csmoe_dispatch_rows / csmoe_dispatch_tokens write it (xs may be null: no bf16 copy), and
 * q [n, D] / s [n, D/32] byte for byte what csmoe_quantize_mxfp8 (transpose == 0) writes for xs.  Replaces the gather of
 * cvmm.py:114-119 followed by this library's own quantiser (the reference has no fp8): the gathered bf16 rows are not read back.
 * The tokens form has n = T * K destination rows.  CSMOE_BF16 only, D % 32 == 0, x / xs 16-byte aligned (else CSMOE_ERR_INVALID
 * before anything is launched); n == 0 / T == 0 is a no-op. */
int csmoe_dispatch_rows_mxfp8(const void* x, const int32_t* perm, int K, void* xs, uint8_t* q, uint8_t* s, int n, int D, int dtype,
                              csmoe_stream_t stream);
int csmoe_dispatch_tokens_mxfp8(const void* x, const int32_t* slot_of, int K, void* xs, uint8_t* q, uint8_t* s, int T, int D,
                                int dtype, csmoe_stream_t stream);
/* Both orientations in one pass over the source (weights are needed along one dim by the forward product and along the other by
 * the backward product): q [E, R, C] / s [E, R, C/32] and qt [E, C, R] / st [E, C, R/32], bit-identical to the two separate calls.
 * R % 32 == 0, C % 32 == 0, 16-byte aligned rows. */
int csmoe_quantize_mxfp8_both(const void* x, const void* const* x_ptrs, int E, int64_t ldx, int R, int C, int dtype, void* q, void* s,
                              void* qt, void* st, csmoe_stream_t stream);
/* Row-space grouped GEMM on v_mfma_scale_f32_16x16x128_f8f6f4: C[m, 0:N] = epilogue(sum_k A[m,k] B_e[n,k]) for the binned rows of
 * expert e; A [M, Kd] e4m3 (lda) with scales [M, Kd/32] (ldas); B_e = bq_ptrs[e] [N, Kd] e4m3 (ldb), scales bs_ptrs[e] [N, Kd/32]
 * (ldbs); bf16 outputs / bias / aux and the epilogues PLAIN / BIAS / BIAS_ACT / ACTGRAD of csmoe_grouped_gemm.
 * Kd % 128 == 0, N % 8 == 0, 16-byte aligned operands, lda % 16 == 0, ldas % 4 == 0 (else CSMOE_ERR_UNSUPPORTED). */
int csmoe_grouped_gemm_mxfp8(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* const* bq_ptrs,
                             const void* const* bs_ptrs, int64_t ldb, int64_t ldbs, const void* const* bias_ptrs,
                             const int32_t* offsets, int E, int M, int N, int Kd, void* C, void* C2, const void* aux, int64_t ldc,
                             int epilogue, int act, csmoe_stream_t stream);
/* Dense form (one weight matrix: the always-on shared expert). */
int csmoe_dense_gemm_mxfp8(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Bq, const void* Bs, int64_t ldb,
                           int64_t ldbs, const void* bias, int M, int N, int Kd, void* C, void* C2, const void* aux, int64_t ldc,
                           int epilogue, int act, csmoe_stream_t stream);
/* The two entries above with a quantised activated output, and on the dense entry the affinity epilogues of the competition pass
 * (the entries above keep their signatures and their refusals).  Same operands, shape rule and rounding points; in addition:
 *   - Cq [M, N] e4m3 (ldcq) and Cs [M, N/32] e8m0 (ldcs), both null or both given, CSMOE_EPI_BIAS_ACT only: the MX quantisation of
 *     the bf16-ROUNDED activated output, blocks along N -- the operand orientation of the GEMM that reads the activations next.
 *     Contract: Cq and Cs are, byte for byte, what csmoe_quantize_mxfp8 (transpose = 0) writes for the bf16 C2 of the same launch,
 *     all-zero blocks (scale byte 0), NaN and Inf included; C and C2, when given, are the bytes the entries above write.  C, C2 and
 *     Cq are each optional (one of them must be given).  Needs N % 32 == 0 (no block straddles the matrix edge), Cq 16-byte aligned
 *     and ldcq % 16 == 0, else CSMOE_ERR_UNSUPPORTED.  Without Cq the call launches what the entries above launch.
 *   - csmoe_dense_gemm_mxfp8_q also takes CSMOE_EPI_SOFTPLUS_ROWSUM (C = the FP32 table [M, ceil(N/256)], ldc its row stride; closed
 *     by csmoe_affinity_finish) and CSMOE_EPI_SOFTPLUS_GRAD (aux = FP32 d aff [M], required), with `act` = their flag bits, as
 *     csmoe_dense_gemm does on bf16 operands.
 * Returns CSMOE_ERR_INVALID for an argument combination that makes no sense (Cq without Cs, Cq with another epilogue, SOFTPLUS_GRAD
 * without aux, a leading dimension too small, null operands) and CSMOE_ERR_UNSUPPORTED for CSMOE_EPI_ACCUM or a shape / alignment
 * the rule rejects, with a message, before any pointer is read and before anything is launched; M == 0 is CSMOE_OK.
 * csmoe_gemm_mxfp8_q_ok: the shape rule as a pure host query (0 / 1; ldcq / ldcs are looked at only with quant_out; `dense`
 * admits the affinity epilogues).  No counterpart upstream (the reference has no fp8). */
int csmoe_grouped_gemm_mxfp8_q(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* const* bq_ptrs,
                               const void* const* bs_ptrs, int64_t ldb, int64_t ldbs, const void* const* bias_ptrs,
                               const int32_t* offsets, int E, int M, int N, int Kd, void* C, void* C2, const void* aux, int64_t ldc,
                               int epilogue, int act, void* Cq, int64_t ldcq, void* Cs, int64_t ldcs, csmoe_stream_t stream);
int csmoe_dense_gemm_mxfp8_q(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Bq, const void* Bs, int64_t ldb,
                             int64_t ldbs, const void* bias, int M, int N, int Kd, void* C, void* C2, const void* aux, int64_t ldc,
                             int epilogue, int act, void* Cq, int64_t ldcq, void* Cs, int64_t ldcs, csmoe_stream_t stream);
int csmoe_gemm_mxfp8_q_ok(int M, int N, int Kd, int64_t lda, int64_t ldas, int64_t ldb, int64_t ldbs, int64_t ldc, int64_t ldcq,
                          int64_t ldcs, int epilogue, int quant_out, int dense);
/* Few-row (decode) form of csmoe_grouped_gemm_mxfp8 (csrc/gemm_skinny_mx.hip): the weight streamer of csmoe_grouped_gemm_skinny
 * on MXFP8 operands, one v_mfma_scale_f32_16x16x128_f8f6f4 per 128-element K-step, the weights (half the bytes of bf16) read once
 * per 16-row block straight into registers.  For every expert e and binned row m in [offsets[e], offsets[e+1])
 *     C[m, 0:N] = epilogue( sum_k dq(A)[row(m), k] dq(B_e)[n, k] ),   row(m) = src_rows ? src_rows[m] / src_div : m
 * A = Aq [R, Kd] e4m3 (lda) with scales As [R, Kd/32] (ldas): one source row supplies its elements and its scale row, so with
 * bins.perm and K the call reads the T quantised token rows and no dispatch copy exists.  B_e = bq_ptrs[e] [N, Kd] e4m3 (ldb) with
 * scales bs_ptrs[e] [N, Kd/32] (ldbs): the one weight layout of csmoe_grouped_gemm_mxfp8; every bq_ptrs[e] 16-byte and every
 * bs_ptrs[e] 4-byte aligned (device tables: the caller's contract, the entry cannot look).  bf16 outputs and biases;
 * epilogues PLAIN, BIAS, BIAS_ACT (all six activations) at the rounding points of csmoe_grouped_gemm_mxfp8; C may be null when only
 * the activated output is wanted.
 * Fused MXFP8 output (BIAS_ACT only; Cq and Cs both null or both given): Cq [M, N] e4m3 (ldcq) and Cs [M, N/32] e8m0 (ldcs) receive
 * the MX quantisation of the bf16-ROUNDED activated output, blocks along N -- byte for byte what csmoe_quantize_mxfp8 (transpose = 0)
 * writes for C2 -- and C2 may then be null: the operand of the second product without a quantiser launch and without a bf16 write.
 * Shape rule (csmoe_grouped_gemm_skinny_mxfp8_ok, a pure host query returning 0 / 1; ldcq / ldcs are looked at only with
 * quant_out): Kd % 128 == 0, N % 8 == 0, lda % 16 == 0, ldb % 16 == 0, ldas % 4 == 0, ldbs % 4 == 0, ldc % 8 == 0; with the quantised
 * output N % 32 == 0 and ldcq % 8 == 0; Aq / C / C2 16-byte, Cq 8-byte and As 4-byte aligned (scale bytes are read a word at a time); M * lda and N * ldb under 2 GiB.
 * Returns CSMOE_ERR_INVALID for bad arguments (null tables, src_div <= 0, Cq without BIAS_ACT); CSMOE_ERR_UNSUPPORTED for a backward
 * epilogue, CSMOE_EPI_ACCUM or a shape the rule rejects -- decided before any pointer is read and before anything is launched;
 * M == 0 is CSMOE_OK.  K is split over the 8 waves of a workgroup and summed in wave order: no atomics, bit-identical from run to
 * run.  No counterpart upstream (the reference has no fp8). */
int csmoe_grouped_gemm_skinny_mxfp8(const void* Aq, int64_t lda, const void* As, int64_t ldas, const int32_t* src_rows, int src_div,
                                    const void* const* bq_ptrs, const void* const* bs_ptrs, int64_t ldb, int64_t ldbs,
                                    const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd, void* C,
                                    void* C2, int64_t ldc, void* Cq, void* Cs, int64_t ldcq, int64_t ldcs, int epilogue, int act,
                                    csmoe_stream_t stream);
int csmoe_grouped_gemm_skinny_mxfp8_ok(int M, int N, int Kd, int64_t lda, int64_t ldas, int64_t ldb, int64_t ldbs, int64_t ldc,
                                       int64_t ldcq, int64_t ldcs, int epilogue, int quant_out);

/* ---- MXFP4 weights for decode (W4A8): a weight-only 4-bit form of the two entries above ------------------------------------
 * Format (OCP Microscaling v1.0, MXFP4): blocks of 32 consecutive elements along the reduction dimension share one e8m0 scale byte
 * s worth 2^(s - 127); elements are e2m1 (sign and magnitude, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6); the shared exponent is
 * floor(log2(amax)) - 2, the byte clamped to [0, 254]; an element is round-to-nearest-even of x * 2^-shared on that grid, saturated
 * at +-6.  A row of Kd elements is Kd / 2 bytes in natural k order: byte j holds element 2 j in its low nibble and element 2 j + 1
 * in its high nibble.  Non-finite inputs are outside the contract: +-inf becomes +-6 and a NaN +-0 (its sign bit), and their block
 * takes the scale byte 253; nothing is read or written out of range because of them.
 *
 * csmoe_quantize_mxfp4: the argument list of csmoe_quantize_mxfp8.  transpose == 0: q [E, R, C/2], s [E, R, C/32] (blocks along C;
 * C % 32 == 0, 16-byte aligned rows).  transpose != 0: q [E, C, R/2], s [E, C, R/32] (blocks along R; R % 32 == 0) -- the forward
 * table of a master stored [Kd, N].  q 16-byte aligned (a block is one 16-byte store); else CSMOE_ERR_UNSUPPORTED. */
int csmoe_quantize_mxfp4(const void* x, const void* const* x_ptrs, int E, int64_t ldx, int R, int C, int dtype, int transpose,
                         void* q, void* s, csmoe_stream_t stream);
/* csmoe_grouped_gemm_skinny_mxfp8 with MXFP4 weights (csrc/gemm_skinny_mx.hip, the same kernel text): the same decomposition, gather (src_rows /
 * src_div for elements and scale rows), epilogues (PLAIN, BIAS, BIAS_ACT at the same rounding points) and optional fused MXFP8
 * output Cq / Cs (byte for byte what csmoe_quantize_mxfp8 (transpose = 0) writes for C2).  For every expert e and binned row m
 *     C[m, 0:N] = epilogue( sum_k dq(A)[row(m), k] dq(B_e)[n, k] ),   row(m) = src_rows ? src_rows[m] / src_div : m
 * A = Aq [R, Kd] e4m3 (lda) with scales As [R, Kd/32] (ldas) exactly as above: the activations stay MXFP8.  B_e = bq_ptrs[e]
 * [N, Kd/2] packed e2m1 with ldb counted in BYTES of the packed row (ldb >= Kd / 2), scales bs_ptrs[e] [N, Kd/32] (ldbs); every
 * bq_ptrs[e] 16-byte and every bs_ptrs[e] 4-byte aligned (device tables: the caller's contract).
 * Shape rule (csmoe_grouped_gemm_skinny_mxfp4w_ok): Kd % 128 == 0, N % 8 == 0, lda % 16 == 0, ldb % 16 == 0, ldas % 4 == 0,
 * ldbs % 4 == 0, ldc % 8 == 0; with the quantised output N % 32 == 0 and ldcq % 8 == 0; Aq / C / C2 16-byte, Cq 8-byte and As 4-byte
 * aligned; M * lda and N * ldb under 2 GiB.  Returns as the fp8 entry does: CSMOE_ERR_INVALID for bad arguments,
 * CSMOE_ERR_UNSUPPORTED for a backward epilogue, CSMOE_EPI_ACCUM or a shape the rule rejects -- decided before any pointer is read
 * and before anything is launched; M == 0 is CSMOE_OK.  No atomics, bit-identical from run to run. */
int csmoe_grouped_gemm_skinny_mxfp4w(const void* Aq, int64_t lda, const void* As, int64_t ldas, const int32_t* src_rows, int src_div,
                                     const void* const* bq_ptrs, const void* const* bs_ptrs, int64_t ldb, int64_t ldbs,
                                     const void* const* bias_ptrs, const int32_t* offsets, int E, int M, int N, int Kd, void* C,
                                     void* C2, int64_t ldc, void* Cq, void* Cs, int64_t ldcq, int64_t ldcs, int epilogue, int act,
                                     csmoe_stream_t stream);
int csmoe_grouped_gemm_skinny_mxfp4w_ok(int M, int N, int Kd, int64_t lda, int64_t ldas, int64_t ldb, int64_t ldbs, int64_t ldc,
                                        int64_t ldcq, int64_t ldcs, int epilogue, int quant_out);

/* ---- MXFP8 weight gradients: operands quantised along the TOKEN dimension -------------------------------------------------
 * Blocking contract.  A block is 32 consecutive BINNED rows of ONE expert.  Binned order is that of csmoe_bin_tokens (a stable
 * counting sort: ascending t * K + k inside an expert -- the order `(idx == e).nonzero()` lists).  Expert e's count_e rows
 * (count_e = offsets[e+1] - offsets[e]) occupy the padded positions poff[e] .. poff[e] + count_e - 1, with
 *     poff[e] = sum_{j<e} roundup(count_j, 128),
 * and the positions up to poff[e+1] hold zeros; blocks start at poff[e], so none mixes two experts, and every 128-element K-tile
 * of the weight-gradient GEMM belongs to one expert (no masking).  The scale rule is that of csmoe_quantize_mxfp8; an all-zero
 * padding block gets the zero-amax scale byte 0.
 *
 * csmoe_token_pad_bound: the padded length the host can size without reading the counts, roundup(n + 127 E, 128) >= poff[E].
 *
 * csmoe_quantize_mxfp8_tokens: binned rows x [n, C] bf16 (leading dim ldx, 16-byte aligned rows, C % 32 == 0) and the device
 * offsets[E+1] of the experts' row ranges ->
 *     poff [E+1] int32 (device),
 *     qt [C, n_pad] e4m3 and st [C, n_pad/32] e8m0: column c of qt is column c of x in padded token order; positions from
 *         poff[E] to n_pad are not written,
 *     optionally (q and s non-null) the row orientation q [n, C] / s [n, C/32] of rows offsets[0] .. offsets[E] - 1 in the same pass,
 *         bit-identical to csmoe_quantize_mxfp8 (transpose = 0) of those rows.
 * n_pad % 128 == 0 and n_pad >= csmoe_token_pad_bound(n, E): no host round trip, the step stays capturable. */
int64_t csmoe_token_pad_bound(int64_t n, int E);
int csmoe_quantize_mxfp8_tokens(const void* x, int64_t ldx, int n, int C, int dtype, const int32_t* offsets, int E, int64_t n_pad,
                                int32_t* poff, void* qt, void* st, void* q, void* s, csmoe_stream_t stream);
/* Weight gradient on v_mfma_scale_f32_16x16x128_f8f6f4: for every expert e
 *     C_e[0:Na, 0:Nb] = sum_{k in [poff[e], poff[e+1])} A[0:Na, k] B[0:Nb, k]
 * with A = Aq [Na, n_pad] (lda) / As [Na, n_pad / 32] (ldas) and B = Bq [Nb, n_pad] (ldb) / Bs [Nb, n_pad / 32] (ldbs) from
 * csmoe_quantize_mxfp8_tokens (poff ranges multiples of 128, inside [0, n_pad)).  E pseudo-experts may also be chunks of those
 * ranges cut at multiples of 128 (csmoe_chunk_offsets of poff with align 128: split-K with fp32 partials).  c_ptrs[e] -> [Na, Nb]
 * (leading dim ldc) in out_dtype CSMOE_F32 or CSMOE_BF16, `accumulate` != 0 adds into it, empty ranges give zeros; `xcd_order`
 * (csmoe_expert_order, or null) deals the experts to the XCDs as in csmoe_grouped_wgrad.  The dense form is E = 1.
 * Na % 8 == 0, Nb % 8 == 0, n_pad % 128 == 0, 16-byte aligned operands, lda / ldb >= n_pad, ldc % 8 == 0. */
int csmoe_grouped_wgrad_mxfp8(const void* Aq, int64_t lda, const void* As, int64_t ldas, const void* Bq, int64_t ldb, const void* Bs,
                              int64_t ldbs, const int32_t* poff, int E, int64_t n_pad, int Na, int Nb, void* const* c_ptrs, int64_t ldc,
                              int out_dtype, int accumulate, const int32_t* xcd_order, csmoe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CSMOE_H */
