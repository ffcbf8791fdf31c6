/* libavec_hip.so -- C ABI of the MI355X (gfx950) hot path for the AV Efficient Conformer.
 *
 * Drop-in boundary: the reference reaches its native code through
 * PyTorch ops emitted by `nn.Module.forward` of the classes registered in
 *   nnet/layers.py:1372-1396 (layer_dict), nnet/attentions.py:739-746 (att_dict),
 *   nnet/normalizations.py:306-316 (norm_dict), nnet/activations.py:71-82 (act_dict),
 *   nnet/blocks.py:312-314 (block_dict), nnet/losses.py:363-366 (loss_dict),
 *   nnet/optimizers.py:184-189 (optim_dict).
 * Each entry point below replaces the ATen op group one of those forwards (or its autograd
 * backward) dispatches; the reference file:line it stands in for is cited per function.
 *
 * Conventions
 *   - plain C symbols, raw device pointers, explicit sizes; no torch types.
 *   - the library never allocates, frees or retains device memory; outputs/workspaces are the
 *     caller's.  Every launch goes to the `hipStream_t` argument, asynchronously (graph-capture safe).
 *   - return 0 on success, <0 for argument errors, >0 = hipError_t; text via avec_last_error().
 *   - `dtype`: AVEC_F32 (0) = fp32 storage + fp32 MFMA (exact; parity mode),
 *              AVEC_BF16 (1) = bf16 storage + bf16 MFMA with fp32 accumulate (throughput mode).
 *     "act" below means a buffer of that dtype; `float*` buffers are fp32 in both modes
 *     (residual stream, statistics, parameters' gradients).
 */
#ifndef AVEC_HIP_H
#define AVEC_HIP_H
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
typedef struct ihipStream_t* hipStream_t;
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define AVEC_F32 0
#define AVEC_BF16 1
#define AVEC_ABI_VERSION 4      /* 2: avec_epilogue_t grew (bnb_*, res_cls0); avec_struct_size() handshake.  3: the row-resident module chains (avec_ffn_chain_*, avec_ln_gemm, avec_layernorm_*_sum) were removed.  4: avec_glu_dwconv_fwd_bn added.  (The Transformer-LM entry points and epilogue act = 3 came without a bump: no struct changed, and a binding resolves every declared symbol at load time) */
#define AVEC_STAT_REPLICAS 64   /* `stats` buffers handed to avec_gemm_nt hold this many [2N] replicas (block b adds to replica b % 64) */

int avec_version(void);
/* sizeof() of the structs that cross this boundary, as THIS library was compiled: a binding compares them with its own declarations at load time, so that a header / .so
 * pair that drifted apart fails loudly instead of reading past a shorter struct.  which: 0 avec_rows_t, 1 avec_epilogue_t, 2 avec_attn_t, 3 avec_tn_item_t,
 * 4 avec_tn_batched_t, 5 avec_ln_item_t, 6 avec_fp8_item_t, 7 avec_wgrad3x3_item_t, 8 avec_ngram_t; -1 for an unknown index. */
int avec_struct_size(int which);
const char* avec_last_error(void);
/* the kernel instance chosen by the last GEMM-family entry point called on this thread ("gemm_nt_glds_kernel<bf16,64,64,0,4,0,128>" ...): measurement aid, bench.py's roofline rows */
const char* avec_last_kernel(void);
/* Optional scratch for the two-pass column reductions (LayerNorm / BatchNorm / depthwise-conv parameter-gradient sums): a 256-byte aligned
 * device buffer (>= 64 KB; 32 MB serves every shape of the AV model) registered for the current device.  Without it those kernels fall back
 * to one float atomic per column per workgroup.  The buffer must stay alive and must not be used by two streams at once.
 * (base = NULL, bytes = 0 unregisters.) */
int avec_set_reduce_workspace(void* base, long long bytes);
/* A second workspace bound to one stream: kernels launched on `stream` use it instead of the device default, so two streams (the audio and the
 * visual branch of the AV encoder) can run reductions concurrently. */
int avec_set_reduce_workspace_stream(void* base, long long bytes, hipStream_t stream);

/* ---- row sources for the GEMM family ------------------------------------------------------ */
enum { AVEC_ROWS_PLAIN = 0, AVEC_ROWS_CONV_FWD = 1, AVEC_ROWS_CONV_BWD = 2 };
typedef struct avec_rows {
  long long ld;                 /* PLAIN: row stride (elements) */
  int rows_out, rows_in, step;  /* PLAIN: src_row = (m / rows_out) * rows_in + (m % rows_out) * step when step > 1
                                   (strided time sub-sampling: the k=1 stride-2 conv_res, nnet/blocks.py:273-277) */
  int H, W, C, KH, KW, stride, pad, OH, OW; /* CONV_*: NHWC geometry; explicit "same" zero padding of nnet/layers.py:250-261 is folded into the loader */
  int T3;                       /* reserved */
} avec_rows_t;

typedef struct avec_epilogue {
  void* out; long long ldo; int out_f32;       /* final output: act, or fp32 when out_f32 */
  void* out_pre; long long ldpre;              /* optional: value before activation (act) */
  const float* bias;                           /* [N] */
  int act;                                     /* 0 none, 1 Swish (nnet/activations.py:39-45), 2 ReLU, 3 GELU (erf form, nn.GELU(); forward only: dact has no 3) */
  float drop_p; const unsigned long long* rng; unsigned rng_stream;  /* nn.Dropout: counter-based mask, rng = {seed, step} on device */
  const void* res; long long ldres; float alpha; int res_act; /* out = res + alpha * v (res fp32, or act when res_act; residuals nnet/blocks.py:292-301) */
  const void* dact_z; long long ldz; int dact; /* backward: v *= act'(z) */
  float* colsum;                               /* += per-column sum of v  (bias gradients) */
  float* stats;                                /* += [N] sum, [N] sum of squares (BatchNorm batch statistics) */
  /* BatchNorm-BACKWARD fusion (round 3; nnet/normalizations.py:90-170): this product IS the gradient d of a BatchNorm(+ReLU) output whose input was `bnb_y`.
   * With bnb_y set the epilogue order is  v = alpha * acc + res;  v *= mask;  stats += (sum v | sum v * y);  out = v   -- the ReLU mask comes from the saved
   * activation `dact_z` (dact = 2: v where z > 0) or, with bnb_mask = 1, from the pre-activation itself (scale * y + shift > 0, bnb_ss = [scale | shift | ...]).
   * avec_bn_bwd_finalize turns the replicated (sum d, sum d*y) into (sum d, sum d*xhat); avec_bn_bwd_apply(act = 0) then needs d and y only. */
  const void* bnb_y; long long ldby; const float* bnb_ss; int bnb_mask;
  /* backward-data of a stride-2 convolution (bf16, parity-class order): `res` holds one row per pixel of class (even row, even column) only -- the gradient that a
   * 1x1 / stride-2 shortcut convolution sends to the same input (nnet/blocks.py: ResNetBlock.residual), computed as a plain product on the subsampled grid --
   * instead of a full-size, three-quarters-zero tensor.  Rejected (< 0) when the launch cannot run in parity-class order. */
  int res_cls0;
  /* ReLU mask on the RESIDUAL operand (round 6): one bit per element of `res` (bit e of byte (row * ldres + col) / 8 = column col + e, the layout avec_bn_apply_fwd_mask
   * writes): out = alpha * v + (bit ? res : 0).  The backward-data product of a ResNetBlock's first convolution adds the block-output gradient that passed the final ReLU
   * (nnet/blocks.py:88-91) -- with this the masked gradient is never written out as a tensor of its own.  bf16 residual, register-direct epilogue kernels only (an error
   * otherwise). */
  const unsigned char* res_mask;
} avec_epilogue_t;

/* C[m][n] = epi(sum_k A[m][k] W[n][k]).  Replaces aten::addmm/mm of layers.Linear.forward (nnet/layers.py:64-76),
 * the k=1 Conv1d of nnet/modules.py:374,379, aten::convolution / convolution_backward(input) of layers.Conv2d
 * (nnet/layers.py:200-324) and the Conv3d stem (nnet/layers.py:326-503). */
int avec_gemm_nt(int dtype, const void* A, const avec_rows_t* a_rows, int a_mode, int a_f32,
                 const void* W, long long ldw, long long M, int N, int K,
                 const avec_epilogue_t* ep, hipStream_t stream);

/* ---- fp8 (OCP e4m3) forward Linear products: BASELINE config 5's "fp8 GEMMs" for the FFN / QKV / output / pointwise-conv projections
 * (nnet/modules.py:257-289,341-385, nnet/attentions.py:60-110; the reference trains them under fp16 autocast, nnet/model.py:404-414).
 * Per-tensor "current" scaling: amax slots are plain device floats holding max|x|; scale = max(amax, tiny) / 448 is derived by the consumers. */
typedef struct { const float* src; void* dst; long long n; int slot; int K, Kp; int reserved; } avec_fp8_item_t;   /* fp32 master [n / K][K] -> e4m3 rows of Kp >= K bytes (zero padded, Kp % 16 == 0, K % 4 == 0), amax in amax[slot] */
/* x [M][K] (fp32 / bf16, row stride ldx) -> q [M][K] e4m3 (row stride ldq bytes); compute_amax != 0: *amax is first raised to max|x| (the caller zeroed it),
 * else *amax is taken as given.  K % 8 == 0; columns K .. roundup16(K) of q are written as zeros (ldq >= roundup16(K)). */
int avec_fp8_quantize(int src_dtype, const void* x, long long ldx, void* q, long long ldq, long long M, int K, float* amax, int compute_amax, hipStream_t stream);
/* every weight of `table` (device memory, n_items entries): amax[slot] = max|w| (caller zeroed the slots), then dst = e4m3(w / scale). */
int avec_fp8_weights_refresh(const avec_fp8_item_t* table, int n_items, int blocks_per_item, float* amax, hipStream_t stream);
/* C = epi( (sum_k A[m][k] W[n][k]) * scale_a * scale_w ), A and W e4m3 (row strides in bytes), epilogue fields as avec_gemm_nt with bf16 "act" buffers. */
int avec_gemm_nt_fp8(const void* A, long long lda, const void* W, long long ldw, long long M, int N, int K,
                     const float* amax_a, const float* amax_w, const avec_epilogue_t* ep, hipStream_t stream);


/* O[i][j] += sum_m P[m][i] Q[m][j]  (fp32 atomics, split over m).  Replaces the weight-gradient aten::mm of
 * Linear backward and convolution_backward(weight). */
int avec_gemm_tn(int dtype, const void* P, long long ldp, const void* Q, const avec_rows_t* q_rows, int q_mode, int q_f32,
                 float* O, long long ldo, long long M, int I, int J, hipStream_t stream);
/* batched form: batch = outer * nb_inner + inner; strides6 = element strides {P_outer, P_inner, Q_outer, Q_inner, O_outer, O_inner}.
 * Used for the attention backward bmm's (dK = dS^T Q, dV = P^T dO per (batch, head); dE_h = sum_b skew(dS)^T Q), nnet/attentions.py:300-315. */
/* avec_gemm_tn plus p_colsum[i] += sum_m P[m][i] (fp32, optional): the bias gradient of a Linear / 1x1 conv comes out of its weight-gradient GEMM
 * (nn.Linear backward: grad_bias = grad_output.sum(0)) */
int avec_gemm_tn_bias(int dtype, const void* P, long long ldp, const void* Q, const avec_rows_t* q_rows, int q_mode, int q_f32,
                      float* O, long long ldo, float* p_colsum, long long M, int I, int J, hipStream_t stream);
/* Grouped weight gradients: up to AVEC_TN_GROUP_MAX independent products O_k[I_k][J_k] += P_k^T Q_k (+ optional column sums of P_k = bias gradients) as ONE launch --
 * the ~10 weight-gradient products of a ConformerBlock backward (nnet/blocks.py:289-306: two FFN modules, attention projections, two pointwise convs) only feed the
 * optimizer, so the caller may queue them and submit them together; one grid over all their tiles fills the chip where each product alone is latency-bound.
 * bf16 only (avec_gemm_tn_grouped_ok tells; others go through avec_gemm_tn_bias).  No alignment requirement.  Operand rows are read in 16-byte chunks up to the next
 * multiple of 8 elements: when I (J) is not a multiple of 8 and ldp (ldq) is smaller than that multiple, the chunk runs into the next row, and behind the LAST row
 * the caller must keep 16 bytes readable (what is read there never reaches a stored result). */
#define AVEC_TN_GROUP_MAX 32
typedef struct avec_tn_item {
  const void* P; const void* Q; float* O; float* p_colsum;
  long long ldp, ldq, ldo, M;
  int I, J;
  int q_rows_out, q_rows_in, q_step;   /* strided row remap of Q as in avec_rows_t (q_step <= 1: identity) */
  int reserved;
} avec_tn_item_t;
int avec_gemm_tn_grouped_ok(int dtype, const avec_tn_item_t* item);
int avec_gemm_tn_grouped(int dtype, const avec_tn_item_t* items, int n, hipStream_t stream);
int avec_gemm_tn_batched(int dtype, const void* P, long long ldp, const void* Q, long long ldq, float* O, long long ldo, long long M, int I, int J,
                         int nb_outer, int nb_inner, const long long* strides6, hipStream_t stream);
/* (batched: as above, rows of P / Q are read in whole 16-byte chunks up to the next multiple of the vector width -- 8 bf16 / 4 fp32 elements -- of I / J, counted from the
 * batch's first column; with batches laid side by side in a row (attention heads of width 45 or 90) the last batch's last chunk of the LAST row ends up to 12 bytes behind the
 * operand: the caller keeps 16 bytes readable there) */
/* the same products STORED in the activation dtype (one workgroup per tile reduces over all M rows: no split, no atomics, no zero-filled fp32 staging):
 * dK and dV of the attention backward go straight into the Q|K|V gradient matrix */
int avec_gemm_tn_batched_store(int dtype, const void* P, long long ldp, const void* Q, long long ldq, void* O_act, long long ldo, long long M, int I, int J,
                               int nb_outer, int nb_inner, const long long* strides6, hipStream_t stream);

/* up to 3 such batched products (accumulating into fp32 `O`, or stored into `O_act` when that is set) as ONE launch: dK, dV and dE of an attention layer's
 * backward pass (nnet/attentions.py:280-323 backward) are three launches of ~5 us otherwise.  A problem that needs another kernel is launched on its own. */
typedef struct {
  const void* P; long long ldp; const void* Q; long long ldq;
  float* O; void* O_act; long long ldo;       /* exactly one of O (accumulate) / O_act (store) */
  long long M; int I, J, nb_outer, nb_inner;
  const long long* strides6;
} avec_tn_batched_t;
int avec_gemm_tn_batched_multi(int dtype, const avec_tn_batched_t* items, int n, hipStream_t stream);

/* ---- SyncBatchNorm statistic exchange by peer writes over xGMI (avec_amd/csrc/peer.hip) ----------
 * all-reduce(sum) of a short fp32 vector (the (2C+1)-float / 2C-float vectors of nnet/normalizations.py:172-249) between the GPUs of one node
 * without RCCL and without the host: every rank writes {value, epoch} granules into its slot of an exchange page in EVERY rank's buffer
 * (buffers mapped by all ranks through HIP IPC), polls its own page and adds the slots in rank order (bit-identical on all ranks).
 * pages[r] = base of this exchange site's page pair in rank r's buffer: 2 pages of world * n granules (8 bytes each), `page_stride_granules` apart;
 * epoch = this site's visit counter in the caller's device memory (zero-initialised, advanced by the kernel: graph-capturable);
 * err_flag is set to 1 if a peer did not arrive within timeout_ms (<= 0: 20 s) -- the call never hangs the GPU. */
#define AVEC_PEER_MAX_WORLD 8
int avec_peer_exchange_sum(const float* in, float* out, int n, void* const* pages, long long page_stride_granules, int rank, int world,
                           unsigned* epoch, int* err_flag, int timeout_ms, hipStream_t stream);
/* the same exchange with the producer-side work folded in (one launch instead of two per SyncBatchNorm exchange): the exchanged vector is
 *   v[i] = sum_{r < n_replicas} in[r * n_in + i] (i < n_in: the AVEC_STAT_REPLICAS statistic copies collapsed on the fly), v[n_in] = tail when has_tail (the local count);
 * with dgamma / dbeta set (backward exchange of [sum dy | sum dy * xhat], n_in = 2 C) the LOCAL sums are first added to the affine gradients, as avec_bn_affine_grads does.
 * out = [n_in + has_tail] sums over ranks. */
int avec_peer_exchange_sum_fused(const float* in, int n_replicas, int n_in, int has_tail, float tail, float* dgamma, float* dbeta, int C, float* out,
                                 void* const* pages, long long page_stride_granules, int rank, int world, unsigned* epoch, int* err_flag, int timeout_ms,
                                 hipStream_t stream);
int avec_enable_peer_access(int peer_device);
/* exchange-buffer management: uncached (fine-grained) device memory + its 64-byte HIP IPC handle; peers map it with _open.  The caller owns the pointers. */
int avec_peer_buffer_alloc(void** ptr, long long bytes, void* ipc_handle_64b);
int avec_peer_buffer_open(const void* ipc_handle_64b, void** ptr);
int avec_peer_buffer_close(void* ptr);
int avec_peer_buffer_free(void* ptr);

/* ---- normalisation / elementwise (avec_amd/csrc/norm.hip) ---------------------------------- */
/* nn.LayerNorm(eps=1e-6) forward/backward: aten::native_layer_norm(_backward) emitted by nnet/modules.py:278,302,373
 * and nnet/blocks.py:267.  x fp32 [M][D]; y act or fp32; dx optionally accumulated (residual merge). */
int avec_layernorm_fwd(int dtype, const float* x, const float* gamma, const float* beta, void* y, int y_f32,
                       float* mean, float* rstd, long long M, int D, float eps, hipStream_t stream);
int avec_layernorm_bwd(int dtype, const void* dy, int dy_f32, const float* x, const float* mean, const float* rstd, const float* gamma,
                       float* dx, const float* dres, float* dgamma, float* dbeta, long long M, int D, hipStream_t stream);
/* dx-only LayerNorm backward with a second output  prep = act(prep_alpha * dropmask(rng, rng_stream, prep_drop_p) * dx):  the gradient the module IN FRONT of this
 * LayerNorm needs at the start of its own backward (out = res + alpha * Dropout(acc + bias), nnet/blocks.py:292-301; otherwise an avec_grad_prep launch per module) */
int avec_layernorm_bwd_prep(int dtype, const void* dy, int dy_f32, const float* x, const float* mean, const float* rstd, const float* gamma,
                            float* dx, const float* dres, void* prep, float prep_alpha, float prep_drop_p, const unsigned long long* rng, unsigned rng_stream,
                            long long M, int D, hipStream_t stream);
/* Two consecutive LayerNorms in one launch (D <= 512): the one that closes a ConformerBlock (nnet/blocks.py:267,303: y1 = LN1(x), fp32) and the one that opens the
 * next block's first feed-forward module (nnet/modules.py:278: h2 = LN2(y1), act) -- rows are independent, the second reads the first's registers.
 * Backward: dy2 (act) = gradient of h2, dres2 (fp32, may be NULL) = the gradient that reaches y1 past LN2 (the residual path); writes dx2 = dres2 + LN2'(dy2)
 * (= the gradient of y1: also LN1's dy for avec_layernorm_param_grads_grouped) and dx1 = LN1'(dx2), plus the optional prepared gradient of dx1 (see _bwd_prep). */
int avec_layernorm_fwd2(int dtype, const float* x, const float* gamma1, const float* beta1, float eps1, float* y1, float* mean1, float* rstd1,
                        const float* gamma2, const float* beta2, float eps2, void* h2, float* mean2, float* rstd2, long long M, int D, hipStream_t stream);
int avec_layernorm_bwd2(int dtype, const void* dy2, const float* x2, const float* mean2, const float* rstd2, const float* gamma2, const float* dres2, float* dx2,
                        const float* x1, const float* mean1, const float* rstd1, const float* gamma1, float* dx1,
                        void* prep, float prep_alpha, float prep_drop_p, const unsigned long long* rng, unsigned rng_stream, long long M, int D, hipStream_t stream);
/* avec_layernorm_bwd with dgamma == dbeta == NULL computes dx only (one wave per row); the parameter gradients of up to AVEC_LN_GROUP_MAX such layers are
 * then produced by ONE launch: dgamma_k[c] += sum_m dy_k[m][c] * xhat_k[m][c], dbeta_k[c] += sum_m dy_k[m][c]  (native_layer_norm_backward's weight / bias terms). */
#define AVEC_LN_GROUP_MAX 40
typedef struct avec_ln_item {
  const void* dy; const float* x; const float* mean; const float* rstd; float* dgamma; float* dbeta;
  long long M; int D; int dy_f32;      /* dy: fp32 when dy_f32 (or dtype == AVEC_F32), else act */
} avec_ln_item_t;
int avec_layernorm_param_grads_grouped(int dtype, const avec_ln_item_t* items, int n, hipStream_t stream);
/* backward of out = res + alpha*Dropout(acc + bias): dacc (act) and dbias; nnet/modules.py:286-288 + nnet/blocks.py:292-301 */
int avec_grad_prep(int dtype, const float* dout, long long ld, void* dacc, float alpha, float drop_p, const unsigned long long* rng,
                   unsigned rng_stream, float* dbias, long long M, int N, hipStream_t stream);
int avec_colsum(int dtype, const void* x, long long ld, float* out, long long M, int N, hipStream_t stream);
int avec_strided_rows_add(float* dx, const float* src, int B, int T, int To, int D, int step, hipStream_t stream);
/* BatchNorm{1,2,3}d over channels-last [M][C] (aten::native_batch_norm(_backward), nnet/normalizations.py:42-170).
 * stats = n_replicas x [sum | sumsq] (the GEMM epilogue spreads its atomics over AVEC_STAT_REPLICAS copies); ss = [scale | shift | mean | rstd]; SyncBatchNorm (:172-249) = all-reduce stats/count/dstats between calls. */
int avec_bn_stats(int dtype, const void* y, float* stats, long long M, int C, hipStream_t stream);
/* SyncBatchNorm glue (normalizations.SyncBatchNorm, nnet/normalizations.py:172-249): out[2C+1] = collapsed [sum | sumsq] + local count (the vector
 * the caller all-reduces); dgamma/dbeta += the LOCAL sums of dstats before dstats is all-reduced */
int avec_bn_collapse(const float* stats, int n_replicas, float count, float* out, int C, hipStream_t stream);
int avec_bn_affine_grads(const float* dstats, float* dgamma, float* dbeta, int C, hipStream_t stream);
int avec_bn_finalize(const float* stats, int n_replicas, const float* count_ptr, float count, const float* gamma, const float* beta, float* running_mean,
                     float* running_var, long long* num_batches_tracked, float momentum, float eps, float* ss, int C, int training, hipStream_t stream);
/* dstats[c] = sum over the n_replicas copies of stats[c], dstats[C + c] = rstd[c] * (sum of stats[C + c] - mean[c] * dstats[c]):  (sum d, sum d*y) -> (sum d, sum d*xhat) */
/* measurement aid: out[slot] = 100 MHz wall clock, written by a one-wave kernel on `stream` (graph-capturable) */
int avec_stamp(unsigned long long* out, int slot, hipStream_t stream);
int avec_bn_bwd_finalize(const float* stats, int n_replicas, const float* ss, float* dstats, int C, hipStream_t stream);
int avec_bn_apply_fwd(int dtype, const void* y, const float* ss, const void* residual, int act, void* out, long long M, int C, hipStream_t stream);
int avec_bn_bwd_reduce(int dtype, const void* dout, const void* y, const void* out, const float* ss, int act, float* dstats, long long M, int C, hipStream_t stream);
int avec_bn_bwd_apply(int dtype, const void* dout, const void* y, const void* out, const float* ss, const float* gamma, const float* dstats,
                      const float* count_ptr, float count, int act, void* dy, void* dres, float* dgamma, float* dbeta, long long M, int C, hipStream_t stream);
/* ReLU mask as one bit per element (C % 8 == 0; byte k = elements 8k .. 8k+7 of the row-major matrix, bit e = out[8k + e] > 0): the forward pass of a
 * residual BatchNorm + ReLU (out = relu(y*scale + shift + residual), the end of a ResNet block, nnet/blocks.py ResNetBlock) writes it next to `out`, the
 * backward passes read M*C/8 bytes instead of the whole saved output tensor (act = ReLU implied, otherwise like avec_bn_bwd_reduce / avec_bn_bwd_apply).
 * residual_ss (optional, [scale | shift | ..] of ANOTHER BatchNorm): the residual is that layer's raw input, normalised on the fly -- the projection shortcut
 * conv1x1 + BatchNorm of a down-sampling block without a tensor of its own: out = relu(y*scale + shift + residual*rscale + rshift). */
int avec_bn_apply_fwd_mask(int dtype, const void* y, const float* ss, const void* residual, const float* residual_ss, void* out, unsigned char* mask, long long M, int C,
                           hipStream_t stream);
int avec_bn_bwd_reduce_mask(int dtype, const void* dout, const void* y, const unsigned char* mask, const float* ss, float* dstats, long long M, int C, hipStream_t stream);
int avec_bn_bwd_apply_mask(int dtype, const void* dout, const void* y, const unsigned char* mask, const float* ss, const float* gamma, const float* dstats,
                           const float* count_ptr, float count, void* dy, void* dres, float* dgamma, float* dbeta, long long M, int C, hipStream_t stream);
/* softmax of the InterCTC residual (nnet/modules.py:395-400) */
int avec_softmax_fwd(int dtype, const float* logits, void* probs, long long M, int V, hipStream_t stream);
int avec_softmax_bwd(int dtype, const void* dprobs, const float* logits, float* dlogits, const float* dadd, long long M, int V, hipStream_t stream);
int avec_cast_rows(int dtype, const float* src, long long ld_src, void* dst, long long ld_dst, long long M, int N, hipStream_t stream);
int avec_to_f32_rows(int dtype, const void* src, long long ld_src, float* dst, long long ld_dst, long long M, int N, int accum, hipStream_t stream);
/* Stand-alone activations on fp32 tensors (nnet/activations.py:39-69; on the hot path they are epilogues of the producing kernels): act 1 Swish, 2 ReLU,
 * 3 GLU over the last axis (x [rows][2C] -> out [rows][C]).  backward != 0: out = d(loss)/dx from dy (GLU: out is [rows][2C]). */
int avec_act_f32(int act, const float* x, const float* dy, float* out, long long rows, int C, int backward, hipStream_t stream);
int avec_dropout_f32(const float* x, float* y, float p, const unsigned long long* rng, unsigned rng_stream, long long n, hipStream_t stream);
/* Stand-alone layers (avec_amd/csrc/standalone.hip): layers.MaxPool3d with a (1, KH, KW) window on a channels-last tensor [frames][H][W][C] (nnet/layers.py:839-915: zero
 * padding pad0 / pad1 before / behind each spatial axis, then a valid max pool; idx = winner slot kh*KW + kw, 255 = the zero padding), and layers.Upsample(mode="nearest")
 * on rows [B][T][D] -> [B][T*P][D] (nnet/layers.py:1013-1043; backward != 0: the P-row sums).  On the hot path both run fused (stem3p.hip, patch attention). */
int avec_maxpool_hw_fwd(int dtype, const void* x, void* out, unsigned char* idx, long long frames, int H, int W, int C, int KH, int KW, int SH, int SW,
                        int pad0_h, int pad0_w, int pad1_h, int pad1_w, hipStream_t stream);
int avec_maxpool_hw_bwd(int dtype, const void* dy, const unsigned char* idx, void* dx, long long frames, int H, int W, int C, int KH, int KW, int SH, int SW,
                        int pad0_h, int pad0_w, int pad1_h, int pad1_w, hipStream_t stream);
int avec_upsample_rows(int dtype, const void* src, void* dst, long long B, int T, int D, int P, int backward, hipStream_t stream);
/* patch attention pooling (layers.AvgPool1d / Upsample, nnet/attentions.py:342-346,365-380) */
int avec_patch_pool_fwd(int dtype, const void* x, void* y, int B, int T, int D, int P, hipStream_t stream);
int avec_patch_pool_bwd(int dtype, const void* dy, void* dx, int B, int T, int D, int P, hipStream_t stream);
int avec_patch_unpool_add(int dtype, const void* o, const float* res, float* out, float drop_p, const unsigned long long* rng, unsigned rng_stream,
                          int B, int T, int D, int P, hipStream_t stream);
int avec_patch_unpool_bwd(int dtype, const float* dout, void* dob, float drop_p, const unsigned long long* rng, unsigned rng_stream,
                          int B, int T, int D, int P, hipStream_t stream);
/* layers.GlobalAvgPool2d (nnet/layers.py:1328-1342), channels-last */
int avec_avgpool_fwd(int dtype, const void* x, void* y, long long N, int HW, int C, hipStream_t stream);
int avec_avgpool_bwd(int dtype, const void* dy, void* dx, long long N, int HW, int C, hipStream_t stream);

/* ---- conformer convolution module middle (avec_amd/csrc/convmod.hip) ----------------------- */
/* nn.GLU(dim=-1) + depthwise layers.Conv1d(k, groups=C, stride, padding) (nnet/modules.py:375-376); w is tap-major [K][C].
 * pad_left = zero frames in front of the sequence (nnet/layers.py:137-156): K / 2 for "same", K - 1 for "causal" (streaming), 0 for "valid"-like use;
 * the output always has (T - 1) / stride + 1 frames, i.e. the right padding is whatever completes K - 1. */
int avec_glu_dwconv_fwd(int dtype, const void* u, const float* w, const float* bias, void* out, float* stats,
                        int B, int T, int C, int K, int stride, int pad_left, hipStream_t stream);
/* avec_glu_dwconv_fwd followed by avec_bn_finalize in training mode over the B * To output rows (local batch statistics): the finalize reads the column-reduction partials
 * directly (two launches instead of three in the conformer block's dependent chain).  stats: zeroed [2C], used only when the reduction runs on atomics. */
int avec_glu_dwconv_fwd_bn(int dtype, const void* u, const float* w, const float* bias, void* out, float* stats, int B, int T, int C, int K, int stride, int pad_left,
                           const float* gamma, const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                           float* ss, hipStream_t stream);
int avec_dwconv_glu_bwd(int dtype, const void* dc, const void* u, const float* w, void* du, float* dw, float* dbias,
                        int B, int T, int C, int K, int stride, int pad_left, hipStream_t stream);
/* avec_bn_bwd_apply (act = Swish, local batch statistics: count = B * T rows, dstats = the (sum d, sum d * xhat) of avec_bn_bwd_reduce) folded into avec_dwconv_glu_bwd's
 * staging pass (stride 1): da = gradient of the BatchNorm + Swish output, c = the BatchNorm input; dgamma / dbeta += dstats.  One launch and one tensor less in the block's chain. */
int avec_dwconv_glu_bwd_bn(int dtype, const void* da, const void* c, const float* ss, const float* gamma, const float* dstats, float count, const void* u, const float* w,
                           void* du, float* dw, float* dbias, float* dgamma, float* dbeta, int B, int T, int C, int K, int pad_left, hipStream_t stream);

/* ---- attention (avec_amd/csrc/attention.hip) ------------------------------------------------ */
typedef struct avec_attn {
  const void *q, *k, *v; long long ld;        /* act [B*T][ld]; head h = columns [h*d,(h+1)*d) */
  const void* e; long long lde;               /* act [2T-1][lde]: pos_layer(sinusoid rows p = T-1 .. -(T-1)) (nnet/embeddings.py:101-158) */
  const long long* lens; int len_div;         /* key j kept iff j < lens[b]/len_div (Mask.padding_mask, nnet/attentions.py:682-733; patch min-pool :357-362) */
  int q_full;                                 /* query rows >= q_full are fully masked (zero-padded last patch); 0 = T */
  const float* mask; long long mask_bstride;  /* optional dense (Bm,T,T) 0/1 mask (1 = keep) instead of lens */
  void* o; long long ldo; float* lse;         /* outputs: act [B*T][ldo], fp32 [B*H][T][2] = softmax row (max, sum) */
  const void* dout;                           /* backward input, act [B*T][ldo] */
  void *dq, *dk, *dv; long long lddq, ldd;    /* act gradients: dq (row stride lddq), dk / dv (row stride ldd) */
  float* de; long long ldde;                  /* fp32 [2T-1][ldde], accumulated */
  void *pbuf, *dsbuf; long long ldt;          /* backward scratch, act [B*H][T][ldt] each (probabilities, dS) */
  void* dsrel; long long ldr;                 /* optional act [H][B*T][ldr] (zero-filled): dS indexed by E row; when given, dK/dV/dE are left to avec_gemm_tn_batched */
  int B, H, T, d; float scale;
  int Tk;                                     /* keys / values per batch element, 0 = T.  Tk > T: a key/value cache (`hidden`, nnet/attentions.py:506-512) precedes the T new frames:
                                                 k, v = act [B*Tk][ld], e = act [Tk+T-1][lde] (row r <-> relative position Tk-1-r), dense mask (Bm,T,Tk); forward and the probability
                                                 pass of avec_relpos_attention_bwd (pbuf) only */
} avec_attn_t;
/* RelPos1dMultiHeadAttention.forwardQKV core (nnet/attentions.py:299-315): bmm + rel_to_abs + mask + softmax + bmm */
int avec_relpos_attention_fwd(int dtype, const avec_attn_t* args, hipStream_t stream);
int avec_relpos_attention_bwd(int dtype, const avec_attn_t* args, hipStream_t stream);

/* ---- streaming encoder (nnet.ConformerStreamSession; avec_amd/csrc/convmod.hip, attention.hip) ---------------------------------------------------------------
 * A causal Conformer stack run chunk by chunk: everything row-wise reuses the offline entry points; these two carry the depthwise convolution's left context
 * and the attention's keys / values across launches in caller-owned buffers.  The library keeps no pointers between calls; nothing here synchronises.
 * Common arguments: pos [B] int64 on the device = frames (at the stack's input rate) slot b has taken since its restart, BEFORE this chunk; reset [B] bytes
 * (NULL: none): a set slot restarts from position 0 before the chunk -- whatever its buffers hold is then older than the restart and counts as absent (no memset);
 * chunk_len [B] int64 (NULL: the whole chunk) = input-rate frames of the chunk the slot takes; div = product of the strides in front of this stage.  At this
 * stage a slot starts at p0 = pos / div and takes n = ceil(chunk_len / div) <= Tq rows; rows at or beyond n are computed from what was passed and never reach the
 * carried state.  avec_stream_advance ends a push: pos = (reset ? 0 : pos) + min(chunk_len, full), then clears the reset flags (they are consumed).
 *
 * avec_glu_dwconv_stream: GLU -> causal depthwise conv (K <= 16 taps, stride s, w tap-major [K][C], optional bias) -> y * ss[c] + ss[C + c] (eval-mode BatchNorm,
 *   the scale | shift of avec_bn_finalize) -> Swish, one launch.  u [B][Tq][2C] act -> out [B][Tq / s][C] act, output row o = chunk row o * s.  state: per slot the
 *   last K - 1 rows of u ([B][K - 1][2C] act, avec_glu_dwconv_stream_state_bytes), updated in place.  C % 4 == 0, all bases 16-byte aligned, K - 1 + Tq <= 96.
 * avec_relpos_attention_stream: the chunk's Tq queries over the band 0 <= p_i - p_j <= L:  scores = scale * q_i . (k_j + E[p_i - p_j]), E [L + 1][lde] (row delta =
 *   pos_layer(PE(delta))); q / k / v rows of the chunk with row stride ld, head h in columns [h * d, (h + 1) * d); kcache / vcache: rings of L + Tq rows of H * d channels
 *   per slot (act, avec_relpos_attention_stream_state_bytes EACH), frame p in row p mod (L + Tq); the chunk's first n rows are appended.  o [B * Tq][ldo] act.  d <= 192. */
long long avec_glu_dwconv_stream_state_bytes(int dtype, int B, int C, int K);
int avec_glu_dwconv_stream(int dtype, const void* u, const float* w, const float* bias, const float* ss, void* out, void* state, long long state_bytes,
                           const long long* pos, const unsigned char* reset, const long long* chunk_len, int div, int B, int Tq, int C, int K, int stride, hipStream_t stream);
long long avec_relpos_attention_stream_state_bytes(int dtype, int B, int H, int d, int L, int Tq);
int avec_relpos_attention_stream(int dtype, const void* q, const void* k, const void* v, long long ld, const void* e, long long lde, void* kcache, void* vcache,
                                 long long cache_bytes, const long long* pos, const unsigned char* reset, const long long* chunk_len, int div, void* o, long long ldo,
                                 int B, int H, int Tq, int d, int L, float scale, hipStream_t stream);
int avec_stream_advance(long long* pos, unsigned char* reset, const long long* chunk_len, long long full, int B, hipStream_t stream);

/* ---- streaming encoder with look-ahead (nnet.ConformerLookaheadStreamSession; avec_amd/csrc/convmod.hip, attention.hip) ---------------------------------------
 * A stack with Mask(left_context=L, right_context=R > 0) run chunk by chunk: every push runs the stack on a WINDOW of W = Tc + LAe input frames per slot, the
 * pend <= LAe frames carried from earlier pushes followed by the new chunk, n = pend + n_new of them valid.  Only c = max(0, n - LAe) frames are final (committed):
 * they reach the carried state and are emitted; the others come back, recomputed, in the next window.  A slot that ends (`last`) emits all n and commits nothing.
 * pos [B] int64 = COMMITTED input frames since the restart; reset as above; nvalid / ncommit [B] int64 = n and c at the input rate (a stage behind total stride div
 * sees ceil(nvalid / div) valid and ncommit / div committed rows of its Wq = W / div).
 *
 * avec_stream_window: X [B][W][D] fp32 = [tail[:pend] | x_new[:n_new] | zeros] (x_new [B][Tc][D], tail [B][LAe][D]; n_new NULL: Tc), nvalid = n, ncommit = c rounded
 *   down to a multiple of S (0 for a slot that ends), emit = c (n for a slot that ends).  A restarted slot has pend = 0 and is not ended; an ended slot takes no frame.
 * avec_stream_window_advance ends the push: tail <- X[c : n], pend = n - c (0 for a slot that ends), pos = (reset ? 0 : pos) + c, ended = (reset ? 0 : ended) | last,
 *   and the reset / last flags are cleared (consumed).
 * avec_glu_dwconv_stream_la: avec_glu_dwconv_stream on the Wq window rows; the new context is the last K - 1 rows of [old context | first ncommit / div rows].
 *   K - 1 + Wq <= 96.
 * avec_relpos_attention_stream_la: the Wq queries over the band -R <= p_i - p_j <= L: scores = scale * q_i . (k_j + E[p_i - p_j + R]), E [L + R + 1][lde] (row
 *   delta + R = pos_layer(PE(delta))).  Keys / values: the last L ring frames before pos / div, then the window rows below ceil(nvalid / div) (a row at or past it is
 *   left out whatever it holds); rings as avec_relpos_attention_stream's (L + Tq rows, Tq = Tc / div), only the first ncommit / div <= Tq rows are appended.  A query
 *   that keeps no key writes zeros. */
int avec_stream_window(const float* x_new, const float* tail, float* X, const long long* pend, const long long* n_new, const unsigned char* last, const unsigned char* reset,
                       const unsigned char* ended, long long* nvalid, long long* ncommit, long long* emit, int B, int Tc, int LAe, int D, int S, hipStream_t stream);
int avec_stream_window_advance(const float* X, float* tail, long long* pend, long long* pos, const long long* nvalid, const long long* ncommit, unsigned char* last,
                               unsigned char* reset, unsigned char* ended, int B, int W, int LAe, int D, hipStream_t stream);
int avec_glu_dwconv_stream_la(int dtype, const void* u, const float* w, const float* bias, const float* ss, void* out, void* state, long long state_bytes,
                              const long long* pos, const unsigned char* reset, const long long* ncommit, int div, int B, int Wq, int C, int K, int stride, hipStream_t stream);
int avec_relpos_attention_stream_la(int dtype, const void* q, const void* k, const void* v, long long ld, const void* e, long long lde, void* kcache, void* vcache,
                                    long long cache_bytes, const long long* pos, const unsigned char* reset, const long long* nvalid, const long long* ncommit, int div,
                                    void* o, long long ldo, int B, int H, int Wq, int Tq, int d, int L, int R, float scale, hipStream_t stream);

/* ---- streamed audio front-end (nnet.AudioFrontStreamSession; avec_amd/csrc/audio_stream.hip) -------------------------------------------------------------------
 * Waveform chunks -> the audio stem's rows, with the offline arithmetic (avec_mel_frames -> DFT GEMM -> avec_mel_power_log -> stem).  Mel frame f reads samples
 * [hop f - win/2, hop f + win/2), reflected at both ends of the utterance; stem frame t reads mel frames 2t - 1, 2t, 2t + 1 (frame -1 and frames past the utterance's
 * last are the convolution's zero padding).  With n samples heard, E(n) = n < hop + win/2 ? 0 : (n - hop - win/2) / (2 hop) + 1 stem frames can be computed; an
 * utterance that ends at Ta samples has Ta / (2 hop) + 1.  state (caller-owned, avec_audio_stream_state_bytes, 16-byte aligned, never cleared): per slot the samples
 * [max(0, 2 hop E(n) - hop - win/2), n) (fewer than 2 (hop + win/2) <= 768), n, and an `ended` flag.
 * Controls of a push, [B] each: n_samples int64 (NULL: W) = how many samples of wave row b ([B] rows of W samples, row stride ldw) the slot takes, clamped to 0 .. W;
 * reset bytes (NULL: none): the slot restarts (n = 0, not ended) before the samples -- whatever the state holds is older and counts as absent; last bytes (NULL:
 * none): the utterance ends with these samples (Ta = n + n_samples must exceed n_fft / 2 as offline: the caller's contract); the slot is then ended: until a reset it
 * takes no samples and yields 0 frames.  Samples at or past n_samples are never read into a valid output; every read is clamped into its buffer.
 * One push = avec_mel_frames_stream -> avec_gemm_nt (fp32 DFT, B * Fmax rows) -> avec_mel_power_log(B, Fmax) -> avec_audio_stem_stream -> avec_audio_stream_advance.
 *
 * avec_mel_frames_stream: frames [B][Fmax = 2 Tmax + 1][win] = window * samples of mel frames 2 E0 - 1 .. 2 E1 - 1 (E0 = frames before the push, E1 after, E1 - E0
 *   clamped to Tmax) in rows 0 .. 2 (E1 - E0); every other row, and a row whose mel frame does not exist, is written as zeros.  out_len[b] = E1 - E0;
 *   meta [B][2] int64 = {mel frame of row 0, number of mel frames that exist (Ta / hop + 1 when last, else 2 E1)}.  Reads the state only.
 * avec_audio_stem_stream: mel [B][n_mels][Fmax] (avec_mel_power_log on those rows) -> out [B][Tmax][C * n_mels / 2] act: Conv2d(1 -> C, 3x3, stride 2, pad 1) + bias,
 *   then y * ss[c] + ss[C + c] (eval-mode BatchNorm, the scale | shift of avec_bn_finalize), then Swish, fp32 up to the store; local row r reads local columns
 *   2r, 2r + 1, 2r + 2; columns whose mel frame (meta) is < 0 or does not exist count as zero; rows at or past out_len[b] are written as zeros.  n_mels even,
 *   n_mels / 2 a multiple of 8, out 16-byte aligned.
 * avec_audio_stream_advance: ends the push: shifts the tail (one workgroup per slot, read whole before it is written), n += n_samples, ended |= last, and clears the
 *   reset and last flags (they are consumed).  The last reader of the controls in the push. */
long long avec_audio_stream_state_bytes(int B);
int avec_mel_frames_stream(const float* wave, long long ldw, const float* window, float* frames, const void* state, long long state_bytes,
                           const long long* n_samples, const unsigned char* reset, const unsigned char* last, long long* out_len, long long* meta,
                           int B, int W, int Tmax, int n_fft, int win, int hop, hipStream_t stream);
int avec_audio_stem_stream(int dtype, const float* mel, const float* w, const float* bias, const float* ss, void* out, const long long* out_len,
                           const long long* meta, int B, int n_mels, int Tmax, int C, hipStream_t stream);
int avec_audio_stream_advance(const float* wave, long long ldw, void* state, long long state_bytes, const long long* n_samples, unsigned char* reset,
                              unsigned char* last, int B, int W, int n_fft, int win, int hop, hipStream_t stream);

/* ---- streamed visual stem (nnet.VisualFrontStreamSession; avec_amd/csrc/video_stream.hip) ----------------------------------------------------------------------
 * Video chunks -> the pooled NHWC frames of the visual stem, with the offline arithmetic: Conv3d(1 -> 64, (5,7,7), stride (1,2,2), zero pad (2,3,3)) + bias, then
 * y * ss[c] + ss[64 + c] (eval-mode BatchNorm, the scale | shift of avec_bn_finalize), ReLU, max pool 3x3 / stride 2 / pad 1 per frame.  Output frame t reads input
 * frames t - 2 .. t + 2; a frame index < 0 is zero, and so is one >= n once the utterance has ended (the offline paddings).  With n frames heard E(n) = max(0, n - 2)
 * output frames exist, n once the utterance has ended.  state (caller-owned, avec_video_stream_state_bytes, 16-byte aligned, never cleared): per slot a ring
 * [4][H][W] of the last input frames in the compute dtype (frame f in ring slot f & 3; bf16 for AVEC_BF16: the format the conv loop consumes, so a carried frame is
 * bit-identical to a fresh one), the frame counter n and an `ended` flag.
 * Controls of a push, [B] each: n_frames int64 (NULL: Tin) = how many frames of chunk row b ([B] rows of Tin frames of H x W fp32, row stride ldc floats) the slot
 * takes, clamped to 0 .. Tin; reset bytes (NULL: none): the slot restarts (n = 0, not ended) before the frames -- whatever the state holds is older and counts as
 * absent; last bytes (NULL: none): the utterance ends with these frames; the slot is then ended: until a reset it takes no frames and yields 0.  Frames at or past
 * n_frames and a state never written are not read into a valid output: a zero is sourced, never multiplied.
 * One push = avec_video_stem_stream -> avec_video_stream_advance.
 *
 * avec_video_stem_stream: with n0 = reset ? 0 : n and c = n_frames[b], slot b yields output frames E0 .. E1 - 1, E0 = max(0, n0 - 2), E1 = last ? n0 + c :
 *   max(0, n0 + c - 2) (E1 - E0 clamped to Tmax; an ended slot that was not reset yields 0).  Input frame f comes from ring slot f & 3 for n0 - 4 <= f < n0, from
 *   chunk[b][f - n0] for n0 <= f < n0 + c, from a zero page otherwise.  out is FRAME-major, [Tmax][B][PH][PW][64] in the activation dtype (PH = ceil(ceil(H/2)/2)):
 *   local frame r of slot b in row r * B + b, the NHWC activation ResNet consumes; rows at or past out_len[b] = E1 - E0 are written as zeros.  w8: the weights
 *   repacked [64][36][8] in the compute dtype, row (kd, kh) = slot 0 zero, slots 1 .. 7 = kw 0 .. 6, row 35 zero (what avec_stem3p_fwd takes).  An output element is
 *   one fixed-order reduction over (kd, kh, kw) inside one workgroup: it depends on the values of its five input frames alone, not on where they came from nor on
 *   the push.  Reads the state only.  W % 8 == 0, W >= 32, H >= 8; chunk, state, w8 and out 16-byte aligned.  AVEC_BF16: MFMA 32x32x16 bf16, fp32 accumulation.
 * avec_video_stream_advance: ends the push: the chunk's last min(c, 4) frames go into their ring slots (converted to the compute dtype), n = n0 + c, ended |= last,
 *   and the reset and last flags are cleared (they are consumed).  A launch of its own: it overwrites ring slots that workgroups of the stem launch read. */
long long avec_video_stream_state_bytes(int dtype, int B, int H, int W);
int avec_video_stem_stream(int dtype, const float* chunk, long long ldc, const void* state, long long state_bytes, const long long* n_frames,
                           const unsigned char* reset, const unsigned char* last, const void* w8, const float* bias, const float* ss, void* out,
                           long long* out_len, int B, int Tin, int Tmax, int H, int W, hipStream_t stream);
int avec_video_stream_advance(int dtype, const float* chunk, long long ldc, void* state, long long state_bytes, const long long* n_frames, unsigned char* reset,
                              unsigned char* last, int B, int Tin, int H, int W, hipStream_t stream);

/* ---- streamed audio-visual fusion input (nnet.AudioVisualStreamSession; avec_amd/csrc/av_stream.hip) -------------------------------------------------------------
 * Pairs the 80 ms rows of the audio and the visual branch across pushes and writes the operand of the fusion module's first Linear.  state (caller-owned,
 * avec_av_fuse_stream_state_bytes, 16-byte aligned, never cleared): per slot two rings of `cap` rows in the activation dtype (absolute row p of a branch in ring row
 * p mod cap, cast as avec_cast_rows casts: a carried row is bit-identical to a freshly cast one) and three int64 counters: audio rows received, video rows received,
 * pairs emitted.
 * avec_av_fuse_stream, for slot b: with reset[b] (bytes, NULL: none) the three counters count as 0 -- whatever the rings hold is older and counts as absent; the
 *   first a_len[b] rows of a [B][Ra][Da] fp32 and the first v_len[b] rows of v [B][Rv][Dv] fp32 are appended (lengths int64, clamped to 0 .. Ra / Rv; rows at or past
 *   them are never loaded); m = min(audio rows - pairs, video rows - pairs, max_emit); xc[b][i] = [audio row (pairs + i) | video row (pairs + i)] for i < m and zeros
 *   for m <= i < max_emit (xc [B][max_emit][Da + Dv] in the activation dtype); pair_len[b] = m; pairs += m; the counters are stored and reset[b] is cleared (consumed).
 *   A launch with a_len = v_len = 0 emits what an earlier one left pending.  One workgroup per slot: every read of the old state precedes a barrier, every write to it
 *   follows; an output element is a copy of one input element through one cast, no atomics.  Da % 4 == 0, Dv % 4 == 0; a, v, state and xc 16-byte aligned, the int64
 *   vectors 8-byte aligned; cap >= max_emit + 2, Ra <= cap, Rv <= cap, state_bytes exactly avec_av_fuse_stream_state_bytes: argument errors before any launch.  A
 *   slot whose pending + incoming rows exceed cap loses rows: that cannot be reported from the device and is the caller's contract. */
long long avec_av_fuse_stream_state_bytes(int dtype, int B, int Da, int Dv, int cap);
int avec_av_fuse_stream(int dtype, const float* a, const long long* a_len, const float* v, const long long* v_len, void* state, long long state_bytes,
                        unsigned char* reset, void* xc, long long* pair_len, int B, int Ra, int Rv, int Da, int Dv, int cap, int max_emit, hipStream_t stream);

/* ---- front-ends (avec_amd/csrc/frontend.hip) ------------------------------------------------ */
/* AudioPreprocessing (nnet/preprocessing.py:57-85; torchaudio Spectrogram/MelScale restated): frames -> [DFT via avec_gemm_nt fp32] -> power/mel/log */
int avec_mel_frames(const float* audio, const float* window, float* frames, int B, long long L, int n_fft, int win, int hop, hipStream_t stream);
int avec_mel_power_log(const float* spec, const float* fb, float* out, int B, int F, int n_bins, int n_mels, hipStream_t stream);
/* SpecAugment (nnet/preprocessing.py:115-130) */
int avec_specaugment(float* mel, const long long* lens, int B, int n_mels, int F, int mF, int Fparam, int mT, float pS,
                     const unsigned long long* rng, unsigned rng_stream, hipStream_t stream);
/* debugging / parity aid: out[i] = the uniform in [0, 1) that the counter-based generator of the dropout and SpecAugment kernels yields for (rng = {seed, step}, rng_stream,
 * ids[i]).  SpecAugment (avec_specaugment) draws, per frequency mask q, value = u(2q) * F and min = u(2q + 1) * (n_mels - value); per sample b and time mask q,
 * value = u(1000 + 64 b + 2q) * T_b and min = u(1000 + 64 b + 2q + 1) * (len_b - value): tests replay these draws through the oracle's mask_along_axis restatement and
 * compare the masks bit for bit. */
int avec_debug_rng_uniform(const unsigned long long* rng, unsigned rng_stream, const long long* ids, int n, float* out, hipStream_t stream);
/* audio stem Conv2d(1->C,3x3,s2,"same")+BatchNorm2d+Swish (nnet/networks.py:359-368) in (B,T',C*F') layout */
int avec_audio_stem_conv_fwd(int dtype, const float* mel, const float* w, const float* bias, void* y, float* stats, int B, int n_mels, int F, int C, hipStream_t stream);
int avec_audio_stem_act_fwd(int dtype, const void* y, const float* ss, void* a, int B, int n_mels, int F, int C, hipStream_t stream);
int avec_audio_stem_bwd(int dtype, const void* da, const void* y, const float* mel, const float* ss, const float* gamma, float* dstats,
                        const float* count_ptr, float count, int phase, float* dw, float* dbias, float* dgamma, float* dbeta,
                        int B, int n_mels, int F, int C, hipStream_t stream);
/* BatchNorm3d+ReLU+MaxPool3d((1,3,3),(1,2,2),"same") after the Conv3d stem (nnet/networks.py:459-470, nnet/layers.py:839-915) */
/* im2col of the Cin=1 (5,7,7)/(1,2,2) stem: video fp32 [clips][T][H][W] -> A act [clips*T*OH*OW][ldk] (k = (kd*7+kh)*7+kw, zero padded to ldk) */
int avec_stem_im2col(int dtype, const float* video, void* A, long long clips, int T, int H, int W, int ldk, hipStream_t stream);
/* Direct (no im2col) bf16 MFMA kernels for the same stem (avec_amd/csrc/stem3d.hip): the input band is staged once in LDS and the operands are
 * gathered from it.  w_shadow: bf16 [64][36][8] = per (kd,kh) row the 7 kw taps + a zero slot, row 35 zero (ldw = 288); y: bf16 [clips*T*OH*OW][64]; stats (optional):
 * fp32 [2*64] += (sum, sum of squares) of y per channel; dw: fp32 [64][245] +=.  avec_stem3d_supported() tells whether the frame size fits. */
int avec_stem3d_supported(long long clips, int T, int H, int W);
int avec_stem3d_fwd(const float* video, const void* w_shadow, int ldw, const float* bias, void* y, float* stats, long long clips, int T, int H, int W, hipStream_t stream);
int avec_stem3d_wgrad(const float* video, const void* dy, float* dw, long long clips, int T, int H, int W, hipStream_t stream);
/* Round 3: the same stem WITHOUT the pre-pool activation in memory (avec_amd/csrc/stem3p.hip).  BatchNorm + ReLU is monotone per channel, so the max pool is taken on the raw
 * conv output (max for gamma >= 0, min for gamma < 0) inside the convolution kernel:
 *   avec_stem3p_fwd   : video_bf16 [clips][T][H][W] (W % 8 == 0), w_shadow bf16 [64][36][8] (slot 0 of every (kd,kh) row and row 35 zero, slots 1..7 = kw 0..6), gamma = the
 *                       BatchNorm weight -> zp act [clips*T][PH][PW][64] (raw conv output of each window's winner), idx u8 (window slot kh*3+kw), stats fp32 [2*64] += (sum, sumsq) of z
 *                       (then avec_bn_finalize + avec_bn_apply_fwd(zp, ReLU) give the pooled activation);
 *   avec_stem3p_reduce: dpool <- dpool * [scale*zp+shift > 0] in place, dstats [2*64] += (sum d, sum d * xhat) over the pooled tensor;
 *   avec_stem3p_dz    : recomputes z and writes dz [clips*T*OH*OW][64] = gamma*rstd*(route(dpool) - mean(dy) - xhat*mean(dy*xhat)) (the operand of avec_stem3d_wgrad); dgamma/dbeta += dstats. */
int avec_stem3p_supported(long long clips, int T, int H, int W);
int avec_stem3p_fwd(const void* video_bf16, const void* w_shadow, const float* bias, const float* gamma, void* zp, unsigned char* idx, float* stats,
                    long long clips, int T, int H, int W, hipStream_t stream);
int avec_stem3p_reduce(void* dpool, const void* zp, const float* ss, float* dstats, long long frames, int PH, int PW, hipStream_t stream);
/* fused: dw fp32 [64][245] += the stem's weight gradient straight from the pooled gradients (z recomputed per tile, dz formed in LDS, never written) */
int avec_stem3p_wgrad_supported(long long clips, int T, int H, int W);
/* the layout the two kernels' geometry rules chose (host only; 0 when avec_stem3p_supported is 0): out int[10] = bands per frame NB, pooled rows per band pn, PH, PW,
 * OH, OW, staged row pitch in bytes, avec_stem3p_wgrad_supported, frames per weight-gradient unit, units per clip and band (both 0 where the fused kernel declines) */
int avec_stem3p_geom(long long clips, int T, int H, int W, int* out);
int avec_stem3p_wgrad(const void* video_bf16, const void* w_shadow, const float* bias, const void* dpool_masked, const unsigned char* idx, const float* ss,
                      const float* gamma, const float* dstats, const float* count_ptr, float count, float* dw, float* dgamma, float* dbeta,
                      long long clips, int T, int H, int W, hipStream_t stream);
int avec_stem3p_dz(const void* video_bf16, const void* w_shadow, const float* bias, const void* dpool_masked, const unsigned char* idx, const float* ss,
                   const float* gamma, const float* dstats, const float* count_ptr, float count, void* dz, float* dgamma, float* dbeta,
                   long long clips, int T, int H, int W, hipStream_t stream);
/* ymax (optional, act, pooled shape): the conv output under each window's winning tap -- lets avec_stem_pool_bwd_reduce_pooled compute the BatchNorm-backward sums from
 * pooled-size tensors instead of the full-resolution conv output */
int avec_stem_pool_fwd(int dtype, const void* y, const float* ss, void* out, unsigned char* idx, void* ymax, long long frames, int H, int W, int C, hipStream_t stream);
int avec_stem_pool_bwd_reduce_pooled(int dtype, const void* dpool, const unsigned char* idx, const void* ymax, const float* ss, float* dstats,
                                     long long frames, int H, int W, int C, hipStream_t stream);
int avec_stem_pool_bwd(int dtype, const void* dpool, const unsigned char* idx, const void* y, const float* ss, const float* gamma, float* dstats,
                       const float* count_ptr, float count, int phase, void* dy, float* dgamma, float* dbeta, long long frames, int H, int W, int C, hipStream_t stream);

/* ---- 3x3 / stride 1 / 64->64 channel convolution of ResNet stage 1 (avec_amd/csrc/conv3x3.hip) ------ */
/* Same contract as avec_gemm_nt with ROWS_CONV_FWD (flip = 0: x NHWC bf16, w = forward shadow [64][9][64], y NHWC bf16, stats = AVEC_STAT_REPLICAS x [sum | sumsq]
 * of the fp32 results) or ROWS_CONV_BWD (flip = 1: x = dy, w = backward shadow [Cin][9][Cout], y = dx, res = optional bf16 tensor added to dx) for layers.Conv2d
 * (nnet/layers.py:200-306) with kernel 3x3, stride 1, "same" padding, 64 input and output channels, images of at most 512 pixels whose zero-bordered slab fits
 * 72 KB of LDS ((H+2)(W+2) <= 576, even): weights stay in LDS, every input byte crosses L2 -> LDS once.  bf16 only. */
int avec_conv3x3_c64_supported(int H, int W, int Cin, int Cout, int KH, int KW, int stride);
int avec_conv3x3_c64(const void* x, const void* w, void* y, const void* res, float* stats, long long images, int H, int W, int flip, hipStream_t stream);
/* the same with a residual whose ReLU mask (one bit per element, as avec_epilogue_t.res_mask) is applied while it is added: y = conv(x) + (bit ? res : 0) */
int avec_conv3x3_c64_res_masked(const void* x, const void* w, void* y, const void* res, const unsigned char* res_mask, long long images, int H, int W, int flip, hipStream_t stream);
/* weight gradient of the same layers (what avec_gemm_tn with ROWS_CONV_FWD computes): dw fp32 [64][9][64] (row stride 576) += sum over images / pixels of
 * dy[p][co] * x[p + tap - 1][ci]; x, dy NHWC bf16.  Needs avec_conv3x3_c64_supported and H * (W + 1) <= 512. */
int avec_wgrad3x3_c64(const void* x, const void* dy, float* dw, long long images, int H, int W, hipStream_t stream);
/* the same for the wider 3x3 / stride-1 layers with Cin == Cout == C, C a multiple of 128 (ResNet stages 2..4: 128 / 256 / 512 channels, 11x11 / 6x6 / 3x3 images):
 * dw fp32 [C][9][C] (row stride 9C) += ...; supported when the per-image slabs fit (H (W+1) <= 288 rows of reduction, see csrc/conv3x3.hip) */
int avec_wgrad3x3_c128_supported(int H, int W, int Cin, int Cout, int KH, int KW, int stride);
int avec_wgrad3x3_c128(const void* x, const void* dy, float* dw, long long images, int C, int H, int W, hipStream_t stream);
/* the same for up to AVEC_WGRAD_GROUP_MAX layers in ONE launch: the 256 workgroups are shared out by work, and the final fp32 atomics (256 x 73 728 sums per launch,
 * ~30 % of a single layer's launch) are paid once for all of them.  A binding queues (x, dy, dw) of the 3x3 stride-1 layers during the backward pass (the operands must stay
 * alive and unmodified) and submits them when the ResNet's backward is through. */
#define AVEC_WGRAD_GROUP_MAX 16
typedef struct { const void* x; const void* dy; float* dw; long long images; int C, H, W, reserved; } avec_wgrad3x3_item_t;
int avec_wgrad3x3_c128_grouped(const avec_wgrad3x3_item_t* items, int n, hipStream_t stream);
int avec_wgrad3x3_c64_grouped(const avec_wgrad3x3_item_t* items, int n, hipStream_t stream);      /* the 64-channel layers (C = 64 in every item) */

/* ---- video input pipeline (avec_amd/csrc/video_input.hip) ------------------ */
/* Replaces, for a whole batch, the per-sample dataloader work of LRS.__getitem__ (nnet/datasets.py:187-196,348-356): uint8 -> float / 255, Grayscale,
 * NormalizeVideo (nnet/transforms.py:40-52), RandomCrop / CenterCrop + RandomHorizontalFlip (AV cfg:82-89), TimeMaskSecond (nnet/transforms.py:108-126),
 * align_video_to_audio (nnet/transforms.py:169-180) and CollateFn's zero padding (nnet/collate_fn.py:143-146).
 * clips: device uint8, clip b = [tv][H][W][channels] at byte offset clip_off[b];  geom: device int [B][8] = {tv, H, W, crop_y, crop_x, flip, zero frames in front, n_masks};
 * masks: device int [B][max_masks][2] = (first, one-past-last) frame of each time mask, in clip frames, in application order (null when max_masks == 0);
 * out: fp32 [B][Tout][OH][OW] (every frame outside [pad_left, pad_left + tv) is zero);  frame_ws: fp32 [2][B][Tout] scratch (only with masks).
 * lut: device fp32 [channels][256] = w_c * (u / 255) with w = (0.2989, 0.587, 0.114) for RGB clips and 1 for gray ones (made with the reference's own fp32 operations, so
 * that the device only adds the three terms, subtracts mean and divides by stdv: bit-identical pixels);  mean_frame != 0: mask k is filled with the mean of the clip as left by masks 0..k-1, else with 0. */
int avec_video_input(const unsigned char* clips, const long long* clip_off, const int* geom, const int* masks, int max_masks, int channels, const float* lut, float mean, float stdv,
                     int mean_frame, float* out, float* frame_ws, int B, int Tout, int OH, int OW, hipStream_t stream);
/* ---- test-time augmentation (avec_amd/csrc/tta.hip) ------------------------------------------ */
/* The clip batch of VisualEfficientConformerInterCTC.forward with test_augments (nnet/models_zoo.py:113-122: the clips, then test_augment(clips) for every augment,
 * each through its own encoder pass) for augments that are the horizontal flip, laid out for ONE encoder pass: x fp32 [B][rows][W] (rows = frames * height) ->
 * y fp32 [B * n][rows][W], y[b * n + k] = x[b] mirrored along W when bit k of flip_mask is set, x[b] otherwise (utterance-major: the logits of the batch are a view
 * [B][n][T'][V]).  Every input row is read once and written n times; 16-byte accesses when W % 4 == 0.  x and y 16-byte aligned, n <= 32, no flip_mask bit at or above n. */
int avec_video_tta_batch(const float* x, float* y, int B, long long rows, int W, int n, unsigned flip_mask, hipStream_t stream);

/* ---- loss / optimizer (avec_amd/csrc/loss_optim.hip) ---------------------------------------- */
/* CTCLoss.forward (nnet/losses.py:311-334): per-utterance -log p, batch mean, and d/dlogits (unscaled) */
long long avec_ctc_workspace_floats(int B, int T, int Lmax);
int avec_ctc_loss(const float* logits, const long long* in_lens, const long long* targets, const long long* tgt_lens, float* nll, float* mean_out,
                  float* grad, float* workspace, int B, int T, int V, int Lmax, int blank, int zero_infinity, hipStream_t stream);
/* the same for up to 8 heads that share the batch and the labels (ConformerInterCTC: nnet/networks.py:285-305 feeds six CTC losses), one launch; every head must
 * fit the all-LDS kernel (avec_ctc_loss_multi_fits).  Arrays of n_heads host pointers / frame counts. */
int avec_ctc_loss_multi_fits(int T, int V, int Lmax);
int avec_ctc_loss_multi(int n_heads, const float* const* logits, const long long* const* in_lens, const int* T, float* const* nll, float* const* mean_out, float* const* grad,
                        const long long* targets, const long long* tgt_lens, const float* weights, float* total, int B, int V, int Lmax, int blank, int zero_infinity, hipStream_t stream);
/* (weights: n_heads host floats, total: optional device scalar, += sum_i weights[i] * mean loss of head i -- the weighted total of nnet/model.py:275-287 out of the same launch) */
int avec_scale_by_scalar(const float* g, const float* scalar_dev, float mul, float* out, long long n, hipStream_t stream);
/* out[k] = g[k] * (*scalar_dev) * mul[k] for n_tensors <= 8 tensors in one launch (arrays of host pointers / sizes / factors): the backward of avec_ctc_loss_multi's
 * weighted total, nnet/model.py:275-287 */
int avec_scale_by_scalar_multi(int n_tensors, const float* const* g, float* const* out, const long long* numel, const float* mul, const float* scalar_dev, hipStream_t stream);
/* losses.SoftmaxCrossEntropy (nnet/losses.py:258-290; the LRW word classifier): per-row cross entropy of fp32 logits [M][V] against int64 targets,
 * rows with target == ignore_index give 0; mean_out (optional) += loss/M; grad (optional) = softmax - onehot */
int avec_softmax_ce(const float* logits, const long long* targets, long long ignore_index, float* loss, float* mean_out, float* grad, long long M, int V, hipStream_t stream);
/* length arithmetic of the strided layers (nnet/preprocessing.py:77, nnet/modules.py:127-128, nnet/networks.py:298,302): out[i] = floor((in[i] - sub) / div) + add, int64 */
int avec_len_affine(const long long* in, long long* out, int n, long long sub, long long div, long long add, hipStream_t stream);
/* CTCGreedySearchDecoder argmax (nnet/decoders.py:97-120) */
int avec_argmax_rows(const float* x, long long* out, long long M, int V, hipStream_t stream);

/* ---- CTC prefix beam search with n-gram LM fusion (CTCBeamSearchDecoder, nnet/decoders.py:175-257: ctcdecode + KenLM) ------------------------------
 * An n-gram LM as device tables (avec_amd/ngram.py builds them from an ARPA file).  Token k is the ARPA word chr(k + ngram_offset); every value is a
 * NATURAL log.  A context is a tuple of at most order-1 tokens, oldest first, where token -1 is <s>; it is packed 16 bits per token (code = token + 1,
 * 0xFFFF for <s>; token j of the tuple at bits [16j, 16j+16) of the 128-bit key {lo: tokens 0-3, hi: tokens 4-6}) and found by linear probing from
 * slot mix64(lo * 0x9E3779B97F4A7C15 ^ hi * 0xC2B2AE3D27D4EB4F) & (ctx_cap - 1), mix64 = the splitmix64 finaliser; an all-zero key is an empty slot.
 * A context entry holds its backoff and the continuations (token, ln p) of the n-grams it starts, sorted by token.  ln P(. | ctx) is built as a row:
 * the unigram row, then for each longer suffix of ctx that is in the table: + its backoff, then its continuations overwrite.  unigram[c] = -INFINITY
 * marks a token that is not an LM word: its term is exactly oov_logprob in every context. */
typedef struct avec_ngram {
  int order;                          /* 1..8 */
  int V;                              /* length of `unigram` (the vocabulary the table was built for) */
  const float* unigram;               /* [V] */
  long long ctx_cap;                  /* slots of the context table, a power of two (load <= 0.5) */
  const unsigned long long* ctx_key;  /* [ctx_cap][2] {lo, hi} */
  const float* ctx_bo;                /* [ctx_cap] */
  const int* ctx_off;                 /* [ctx_cap] first continuation */
  const int* ctx_cnt;                 /* [ctx_cap] number of continuations */
  const int* cont_tok;                /* [n_cont] */
  const float* cont_lp;               /* [n_cont] */
} avec_ngram_t;
/* bytes of the backpointer workspace avec_ctc_beam_search needs: [B][T][W] int32 */
long long avec_ctc_beam_workspace_bytes(int B, int T, int W);
/* Prefix beam search over logits [B][T][V] fp32 (lengths int64, clamped to [0, T]), blank = 0, per frame logp = log_softmax(logits * inv_tmp); one
 * workgroup per utterance, the frame loop inside the kernel.  lm = NULL decodes without an LM; otherwise an extension by c adds
 * alpha * ln P(c | last order-1 tokens of <s> prefix) + beta to the prefix's LM score.  Per utterance the W best prefixes by
 * score = ln(p_blank + p_nonblank) + LM score, best first; ties go to the lower candidate index (stays: slot i; extension (slot i, token c): W + i*V + c).
 * Outputs: tokens [B][W][T] int32 (zero past out_len), out_len [B][W] int32, score [B][W], ctc_logp [B][W] = ln(p_blank + p_nonblank); empty slots:
 * score = ctc_logp = -inf, out_len = 0.  Limits: W <= 64, V <= 1024, order <= 8.  workspace: avec_ctc_beam_workspace_bytes. */
int avec_ctc_beam_search(const float* logits, const long long* lengths, int B, int T, int V, int W, float inv_tmp, const avec_ngram_t* lm, float alpha, float beta,
                         float oov_logprob, void* workspace, long long workspace_bytes, int* tokens, int* out_len, float* score, float* ctc_logp, hipStream_t stream);
/* Streaming form of avec_ctc_beam_search: the same search, carried across launches by a caller-owned state, so logits can be decoded chunk by chunk as an
 * encoder emits them.  Pushing an utterance's frames in any split gives, bit for bit, what avec_ctc_beam_search gives on the frames pushed so far (the frame
 * loop is the same code; a launch only loads the beam at its start and stores it at its end).  The library keeps no pointers between calls.
 * state: avec_ctc_beam_state_bytes(B, W) bytes, 16-byte aligned: per utterance the W beam slots and {live beams, frames consumed}.  An utterance starts from the
 * empty prefix when reset[b] != 0 (reset: [B] bytes, NULL = none), and also when its state was not written by this entry point with the same W, LM order and
 * Tcap (zero-filled memory, for instance).  Use the same V, W, Tcap, inv_tmp, LM, alpha, beta and backpointer buffer for every push of a session.
 * logits [B][Tc][V] fp32; chunk_len [B] int64 = frames of this chunk that utterance b consumes (NULL: Tc), clamped to [0, Tc] and to Tcap - frames consumed, so
 * an utterance never holds more than Tcap frames (0 leaves it as it is; with reset it becomes the empty prefix).  backptr: avec_ctc_beam_workspace_bytes(B, Tcap, W)
 * bytes, [B][Tcap][W]; a push writes the rows of its own frames.
 * emit != 0 also writes, for the frames consumed so far, tokens [B][W][Tcap] (zero past out_len), out_len, score and ctc_logp exactly as avec_ctc_beam_search does,
 * and stable_len [B] int32 = the length of the longest common prefix of the live beams: every later hypothesis extends a live beam, so
 * tokens[b][0][0 .. stable_len[b]) is final.  The traceback walks every frame consumed so far.  emit == 0 writes no output (the five pointers may be NULL).
 * Limits as avec_ctc_beam_search: W <= 64, V <= 1024, order <= 8; Tc >= 1, Tcap >= 1. */
long long avec_ctc_beam_state_bytes(int B, int W);
int avec_ctc_beam_stream(const float* logits, const long long* chunk_len, const unsigned char* reset, int B, int Tc, int V, int W, int Tcap, float inv_tmp,
                         const avec_ngram_t* lm, float alpha, float beta, float oov_logprob, void* state, long long state_bytes, void* backptr, long long backptr_bytes,
                         int* tokens, int* out_len, float* score, float* ctc_logp, int* stable_len, int emit, hipStream_t stream);
/* Ring form of avec_ctc_beam_stream: a stream without a frame limit (window-limited prefix beam search).  The backpointer workspace holds `window` rows per
 * utterance (absolute frame t at row t % window), and per utterance the state also keeps base (the oldest frame whose row is held), ccount (tokens committed since
 * the reset), dropped and commits.  Immediately before the search consumes absolute frame t with t - base == window it runs the commit step, with h = window / 2 and
 * f = base + h - 1: (1) every live beam walks rows t-1 .. f+1 to the slot it descends from after frame f; a = that slot of beam 0, the best beam; (2) the tokens on
 * a's path through rows f .. base are appended, oldest first, to the commit log with the frame that emitted each; (3) the beams that descend from another slot are
 * dropped and the others compacted in their order, every field and their entries of row t-1 with them; (4) base = f + 1.  Scores and absolute prefix lengths are not
 * touched.  The step depends on the frame index alone, so any split of the frames into pushes gives the same bits; while t <= window nothing was committed and the
 * search is avec_ctc_beam_search's bit for bit.  t - base <= window holds after every push.
 * state: avec_ctc_beam_ring_state_bytes(B, W) bytes, 16-byte aligned; a state not written by this entry point with the same W, LM order and window (zero-filled
 * memory, a state of avec_ctc_beam_stream) and a slot with reset[b] != 0 start from the empty prefix with base = ccount = dropped = commits = 0.  backptr:
 * avec_ctc_beam_ring_workspace_bytes(B, window, W) bytes.  log: [B][log_frames] pairs of int32 (token, frame), 8-byte aligned; committed token k of an utterance
 * (counted from its reset) is entry k % log_frames.  At most one token is committed per frame and the tokens logged between two reads are those of the frames
 * between the two values of base, at most the frames pushed in between plus window: a host that reads the log whenever (frames pushed since the last read) + window
 * would pass log_frames loses nothing, and it can count pushed frames without a synchronisation.  chunk_len is clamped to [0, Tc] only.  The counters and frame
 * indices are int32.
 * emit != 0 writes the tails: tokens and frames [B][W][window] int32 (the tokens of every beam after the committed ones and the absolute frame that emitted each, zero
 * past out_len), out_len [B][W] = the tail length, score and ctc_logp as avec_ctc_beam_search, stable_len [B] = ccount + the common prefix of the live tails, and
 * info [B][4] = {base, ccount, dropped, commits}; a hypothesis is the committed tokens followed by its tail.  The traceback walks rows t-1 .. base only.
 * emit == 0 writes no output (the seven pointers may be NULL).  Limits: W <= 64, V <= 1024, order <= 8; Tc >= 1, window >= 2, log_frames >= 1. */
long long avec_ctc_beam_ring_state_bytes(int B, int W);
long long avec_ctc_beam_ring_workspace_bytes(int B, int window, int W);
int avec_ctc_beam_stream_ring(const float* logits, const long long* chunk_len, const unsigned char* reset, int B, int Tc, int V, int W, int window, int log_frames,
                              float inv_tmp, const avec_ngram_t* lm, float alpha, float beta, float oov_logprob, void* state, long long state_bytes, void* backptr,
                              long long backptr_bytes, void* log, long long log_bytes, int* tokens, int* frames, int* out_len, float* score, float* ctc_logp,
                              int* stable_len, int* info, int emit, hipStream_t stream);
/* rows[i][c] = ln P(c | ctx_i) as the beam search sees it: ctx [n][max_len] int32 tokens oldest first (-1 = <s>), ctx_len [n]; only the last order-1
 * tokens of a context are used.  Test and documentation aid for the table layout above. */
int avec_ngram_rows(const avec_ngram_t* lm, const int* ctx, const int* ctx_len, int n, int max_len, float oov_logprob, float* rows, hipStream_t stream);
/* ---- CTC forced alignment (avec_amd/csrc/ctc_align.hip): token timestamps for a GIVEN label sequence ------------------------------------------------
 * Viterbi (best-path) alignment of targets to CTC logits: argmax over paths pi with collapse(pi) == target of sum_t log_softmax(logits[t])[pi_t].
 * Inputs as avec_ctc_loss: logits [B][T][V] fp32, in_lens [B] int64 (clamped to [0, T]), targets [B][Lmax] int64, tgt_lens [B] int64 (clamped to [0, Lmax]).
 * Outputs: path [B][T] int32 = the token of every frame, blank included (-1 for t >= in_len); spans [B][Lmax][2] int32 = (first frame, last frame + 1) of the frames
 * that emit target token i (-1, -1 for i >= tgt_len; the blank frames between tokens belong to no token); score [B] = the log-probability of the best path;
 * token_logp [B][Lmax] = the sum of log_softmax over the token's own frames (0 for i >= tgt_len).
 * Infeasible utterance (in_len < tgt_len + number of adjacent equal targets, or a target inside tgt_len that equals blank or lies outside [0, V)): score = -inf,
 * path and spans all -1, token_logp 0; such a target is never used as an index and targets at or past tgt_len are never read.  tgt_len == 0 is feasible (all blank);
 * in_len == 0 == tgt_len gives score 0.  Logits without a path of finite probability (-inf / NaN) give the infeasible outputs too.
 * Tie rule over the S = 2 L + 1 extended states, recursion in fp32, delta_t[s] = max(...) + (logits[t][ext[s]] - lse[t]): the predecessor of s is s unless
 * delta[s-1] is strictly greater; s-2 (allowed when ext[s] != blank && ext[s] != ext[s-2]) only if strictly greater than the winner of those two; the end state is
 * S-1 unless delta[S-2] is strictly greater.  tier: 0 = auto (1 when avec_ctc_align_fits_lds), 1 = emissions and backpointers in LDS (an argument error when the
 * shape does not fit), 2 = in the workspace; the tiers agree bit for bit.  workspace: avec_ctc_align_workspace_bytes, 16-byte aligned, required for every tier. */
long long avec_ctc_align_workspace_bytes(int B, int T, int Lmax);
int avec_ctc_align_fits_lds(int T, int Lmax);          /* 1 when the all-LDS tier can run this shape */
int avec_ctc_align(const float* logits, const long long* in_lens, const long long* targets, const long long* tgt_lens,
                   int B, int T, int V, int Lmax, int blank, int tier /* 0 auto, 1 all-LDS, 2 workspace */,
                   void* workspace, long long workspace_bytes,
                   int* path, int* spans, float* score, float* token_logp, hipStream_t stream);
/* ---- Transformer-LM (GPT) rescoring of the beam (avec_amd/csrc/lm.hip; CTCBeamSearchDecoder's neural rescorer, nnet/decoders.py:208-242) -- inference only ----------------
 * x[n][t][:] = E[ids[n][t]][:] + P[t][:]: nn.Embedding (V x D fp32 table; an id outside [0, V) is clamped) plus the rows of SinPosEmbedding / PosEmbedding1d
 * (nnet/embeddings.py:20-62, fp32 [>= L][D]).  ids int64 [N][L]; out [N*L][D] act, or fp32 when out_f32 (the residual stream).  D % 8 == 0, 16-byte aligned tables. */
int avec_embed_pos(int dtype, const long long* ids, const float* E, const float* P, void* out, int out_f32, long long N, int L, int V, int D, hipStream_t stream);
/* MultiHeadAttention.forwardQKV core under Mask(right_context=0) (nnet/attentions.py:89-138): o = softmax(q k^T * scale + causal) v per (sequence, head) on the fused
 * projection qkv = act [N*L][ld] (q | k | v at columns 0, H*d, 2*H*d; head h = d columns from h*d), o = act [N*L][ldo].  Causality comes from the indices (no mask
 * tensor); lens (optional, int64 [N]): query rows from the first 32-row tile at or past lens[n] on are written as zeros (under a causal mask keys >= lens[n] never reach
 * a row < lens[n]).  d = 64 only (avec_causal_attention_supported), any L. */
int avec_causal_attention_supported(int d);
int avec_causal_attention(int dtype, const void* qkv, long long ld, const long long* lens, void* o, long long ldo, int N, int H, int L, int d, float scale, hipStream_t stream);
/* head Linear + log_softmax + target gather in one kernel: nll[r] = logsumexp_v(h[r] . W[v] + bias[v]) - (h[r] . W[tgt[r]] + bias[tgt[r]]) (fp32), 0 where tgt[r] is
 * outside [0, V) (-1 = ignore).  h = act [R][ldh], W = act [V][ldw] (the compute-dtype copy of the head weight), D a multiple of 64 (bf16) / 32 (fp32).  The [R][V] logits
 * are never written; rows of W at or past V are never read.  The workspace size does not depend on R or V (it is 0: the running state lives in registers and LDS). */
long long avec_lm_head_nll_workspace_bytes(long long R, int V, int D);
int avec_lm_head_nll(int dtype, const void* h, long long ldh, const void* W, long long ldw, const float* bias, const long long* tgt, float* nll, long long R, int V, int D,
                     void* workspace, long long workspace_bytes, hipStream_t stream);
/* nll [S][L] as above with row (s, t) scoring token t + 1 of hypothesis s, lens [S] int64 = tokens of the hypothesis including <sos> and <eos>:
 * out[s] = sum_{t < lens[s] - 1} nll[s][t], added in that order (nnet/decoders.py:226-231, length_pred = N + eos). */
int avec_lm_segment_sum(const float* nll, const long long* lens, long long S, int L, float* out, hipStream_t stream);
/* B utterances x K hypotheses (K = augmentations x beam), lens as above (0 = empty slot):
 * total[s] = beam_score[s] - alpha * neural[s] + beta * beta * (lens[s] - 1)  (higher is better; beta enters squared as in nnet/decoders.py:231,234; -inf for an empty slot or
 * beam_score = -inf),  best[b] (int64) = the first maximum of total[b][:]. */
int avec_lm_rescore_select(const float* neural, const long long* lens, const float* beam_score, float alpha, float beta, int B, int K, float* total, long long* best,
                           hipStream_t stream);
/* The winner among the augmentations of an utterance (CTCBeamSearchDecoder with test_time_aug, nnet/decoders.py:177-180 with the argmin of :242 / :252 over the
 * n * W slots; avec_amd/csrc/tta.hip), kept on the device together with WHICH augmentation won.  tokens [S][W][T] int32, out_len [S][W] int32, score [S][W] as
 * avec_ctc_beam_search writes them for S = B * n rows (row b * n + k = augmentation k of utterance b).  best_slot (optional, int64 [B]): the winning slot in
 * [0, n * W) (avec_lm_rescore_select's `best`), clamped into that range before use.  NULL: the augmentation whose slot-0 score is highest, scanned from augmentation
 * 0 with a strict >, so ties go to the lower index, and beam 0.  Outputs (int64): best_aug [B], best_beam [B], ids [B][T] = the winner's tokens (zero at and past
 * ids_len), ids_len [B] = its out_len clamped to [0, T] (0 when its score is -inf), and best_score [B] fp32 = its score.  An utterance whose slots are all empty
 * gives augmentation 0, beam 0, length 0, score -inf.  One launch, one workgroup per utterance. */
int avec_ctc_tta_pick(const int* tokens, const int* out_len, const float* score, const long long* best_slot, int B, int n, int W, int T, long long* best_aug,
                      long long* best_beam, long long* ids, long long* ids_len, float* best_score, hipStream_t stream);
/* optimizers.Adam.step (nnet/optimizers.py:71-75) over flat arenas; state_dev = {step, lr} */
int avec_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* state_dev, float beta1, float beta2, float eps,
                   float weight_decay, float grad_scale, int zero_grad, long long n, hipStream_t stream);
/* the same with a device-side guard: *skip_flag != 0 (the SyncBatchNorm peer exchange's error flag: a rank did not arrive and the sums of this step are NaN)
 * leaves parameters and moments untouched and only clears the gradient arena -- the step is skipped instead of poisoning the model state */
int avec_adam_step_guarded(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* state_dev, float beta1, float beta2, float eps,
                           float weight_decay, float grad_scale, int zero_grad, long long n, const int* skip_flag, hipStream_t stream);
/* Global L2 norm of a flat fp32 arena (16-byte aligned, n > 0, n % 4 == 0) and the clip factor of torch.nn.utils.clip_grad_norm_ (nnet/model.py:381-383), on the
 * device: no host synchronisation, no atomics, and the same bits from every launch on the same input.  Two launches: every workgroup of the first stores one fp64
 * partial sum of squares (each element is widened to fp64 before it is squared) into `workspace` (avec_grad_norm_workspace_bytes(n) bytes, 8-byte aligned;
 * avec_grad_norm_blocks(n) = that launch's workgroups, capped), one workgroup of the second adds them in a fixed order and writes
 *   stats[0] = norm = fp32(sqrt(sum) * grad_scale)      stats[1] = coef = min(1, max_norm / (norm + 1e-6f))  in fp32
 * max_norm <= 0, infinite or NaN: coef = 1 (the norm alone).  A norm that is not finite also gives coef = 1.
 * flag (optional, int[2]):  flag[0] = (skip_in && *skip_in != 0) || (skip_nonfinite && !isfinite(norm));  flag[1] += flag[0], the running count of skipped steps.
 * skip_in (optional): another device flag to pass on, e.g. the SyncBatchNorm peer exchange's error flag.  Argument errors are reported before any launch. */
long long avec_grad_norm_workspace_bytes(long long n);
int avec_grad_norm_blocks(long long n);
int avec_grad_norm(const float* g, long long n, float grad_scale, float max_norm, int skip_nonfinite, const int* skip_in, void* workspace, long long workspace_bytes,
                   float* stats, int* flag, hipStream_t stream);
/* avec_adam_step_guarded with the clip factor read on the device: clip_dev (optional) = avec_grad_norm's `stats`; the kernel scales the gradient by
 * fp32(grad_scale * clip_dev[1]) where it used grad_scale.  NULL: avec_adam_step_guarded, bit for bit.  skip_flag takes avec_grad_norm's `flag`. */
int avec_adam_step_clipped(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* state_dev, float beta1, float beta2, float eps,
                           float weight_decay, float grad_scale, int zero_grad, long long n, const int* skip_flag, const float* clip_dev, hipStream_t stream);
/* Weight averaging over two flat fp32 arenas of n elements (n > 0, n % 4 == 0; avg and p must not overlap), one launch, no atomics:
 *   mode 0: avg = p                         the first checkpoint (torch.optim.swa_utils.AveragedModel with n_averaged == 0, nnet/model.py:948-967)
 *   mode 1: avg = avg + wp * (p - avg)      swa_type "equal", wp = 1 / (n_averaged + 1); wa is ignored
 *   mode 2: avg = (wa * avg) + (wp * p)     swa_type "exp" (nnet/model.py:950: wa = 1 - swa_decay, wp = swa_decay) and the EMA model's update
 *                                           (nnet/model.py:403-405: param_target.mul_(tau); param_target.add_((1 - tau) * param_net), wa = tau, wp = 1 - tau)
 * Every product, difference and sum is one correctly rounded fp32 operation (never contracted into an FMA): the result equals the same lines on torch fp32 tensors. */
int avec_weight_average(float* avg, const float* p, int mode, float wa, float wp, long long n, hipStream_t stream);
/* Compute-dtype copies of the GEMM weights (master fp32 [A][Tm][C]): fwd = same order, bwd = [C][Tm][A].  table entry = 10 x int64: src_off, fwd_off|-1,
 * bwd_off|-1, A, Tm, C, first_block, n_blocks = Tm*ceil(A/64)*ceil(C/64) (one workgroup per 64x64 tile and tap), C_pad (row stride of the fwd
 * shadow when Tm==1), bwd row pitch (0: Tm*A; larger when several weights share one [C][G*A] backward matrix, e.g. Q|K|V) */
int avec_shadow_refresh(int dtype, const float* master, void* shadow, const long long* table_dev, int n_entries, long long total_blocks, hipStream_t stream);
/* partial refresh: `table_dev` points at the first of `n_entries` consecutive entries, whose blocks are [first_block, first_block + n_blocks) of the full table
 * (the weights of one sub-network right after ITS optimizer launch, while the rest of the backward pass is still running) */
int avec_shadow_refresh_range(int dtype, const float* master, void* shadow, const long long* table_dev, int n_entries, long long first_block, long long n_blocks, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* AVEC_HIP_H */
