// Transformer-LM (GPT) rescoring of the CTC beam, inference only (nnet/decoders.py:208-242, nnet/models_zoo.py:194-273 of the reference).
//
//   avec_embed_pos          x[n][t] = E[ids[n][t]] + P[t]                                   (nn.Embedding + SinPosEmbedding / PosEmbedding1d)
//   avec_causal_attention   softmax(Q K^T / sqrt(d) + causal) V on the fused Q|K|V rows      (MultiHeadAttention under Mask(right_context=0)), d = 64
//   avec_lm_head_nll        nll[r] = logsumexp_v(h[r].W[v] + b[v]) - (h[r].W[tgt] + b[tgt])  (head Linear + log_softmax + gather; the [R][V] logits never exist)
//   avec_lm_segment_sum     per-hypothesis nll sums
//   avec_lm_rescore_select  beam + LM total, first maximum per utterance
//
// Both MFMA kernels are written once for the two compute dtypes through Mma<T> (gemm_dev.h): v_mfma_f32_32x32x16_bf16, or v_mfma_f32_32x32x2_f32 (exact fp32, the
// parity mode).  Accumulator layout of either: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) for register r.
#include "gemm_dev.h"
#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------
// embedding + position: one thread per 8 consecutive channels (16-byte loads; one 16-byte store in bf16, two in fp32)
// ---------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void embed_pos_kernel(const long long* ids, const float* E, const float* P, TO* out, long long rows, int L, int V, int D) {
  const int per = D >> 3;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * per) return;
  const long long r = i / per; const int c = (int)(i - r * per) << 3;
  long long id = ids[r]; id = id < 0 ? 0 : (id >= V ? V - 1 : id);       // (an id outside the table would be a caller bug: clamped, never read out of bounds)
  float e[8], p[8];
  ld8<float>(E + id * D + c, e); ld8<float>(P + (r % L) * (long long)D + c, p);
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] += p[k];
  st8<TO>(out + r * D + c, e);
}

// ---------------------------------------------------------------------------------------------
// causal attention, d = 64.  One wave per (32 query rows, head, sequence); key tiles of 32 up to the diagonal, online softmax.
// Scores are computed transposed (S^T = K Q^T: keys in the accumulator registers, the query on the lane), so a row's max / sum is 16 in-lane operations + one exchange
// between the lane halves, and the probabilities are already an MFMA operand for O^T = V^T P^T (k order inside a step: key 8 g + 4 h + t for register 4 g + t of lane half
// h -- the V^T operand is read from LDS in that order).  Q and K fragments come straight from global memory (a lane's fragment is 16 contiguous bytes of one row); V is
// transposed through LDS.
// The reference adds -1e9 to the masked scores instead of -inf (nnet/attentions.py:121).  Under a causal mask row t always keeps key t, whose score is finite, so
// exp(-1e9 + s - max) is exactly 0 in fp32 as exp(-inf) is: the two agree to fp32 rounding and the constant is not imitated.
// ---------------------------------------------------------------------------------------------
constexpr int AD = 64, VLD = 36;      // head width; row stride (elements) of the transposed V tile: 32 keys + 4 (8- / 16-byte aligned rows for bf16 / fp32)

template <typename T> __device__ __forceinline__ T chunk_elem(const chunk16& c, int e);      // element e of a 16-byte chunk (e is a compile-time constant after unrolling)
template <> __device__ __forceinline__ float chunk_elem<float>(const chunk16& c, int e) { return __uint_as_float(c.w[e]); }
template <> __device__ __forceinline__ bf16 chunk_elem<bf16>(const chunk16& c, int e) { bf16 r; r.v = (bf16_raw)(c.w[e >> 1] >> (16 * (e & 1))); return r; }

template <typename T> struct PV;
template <> struct PV<bf16> {        // two steps of 16 keys
  __device__ static __forceinline__ void run(const bf16* vt_row, int h, const float (&p)[16], f32x16& acc) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint2 a0 = *(const uint2*)(vt_row + 16 * s + 4 * h), a1 = *(const uint2*)(vt_row + 16 * s + 8 + 4 * h);
      chunk16 a, b; a.w[0] = a0.x; a.w[1] = a0.y; a.w[2] = a1.x; a.w[3] = a1.y;
#pragma unroll
      for (int k = 0; k < 4; ++k) b.w[k] = f32x2_to_bf16x2(p[8 * s + 2 * k], p[8 * s + 2 * k + 1]);
      Mma<bf16>::run(a, b, acc);
    }
  }
};
template <> struct PV<float> {       // four groups of 4 registers = 8 keys over the two lane halves
  __device__ static __forceinline__ void run(const float* vt_row, int h, const float (&p)[16], f32x16& acc) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const chunk16 a = *(const chunk16*)(vt_row + 8 * g + 4 * h);
      chunk16 b;
#pragma unroll
      for (int k = 0; k < 4; ++k) b.w[k] = __float_as_uint(p[4 * g + k]);
      Mma<float>::run(a, b, acc);
    }
  }
};

template <typename T>
__global__ __launch_bounds__(64) void causal_attn_kernel(const T* qkv, long long ld, const long long* lens, T* o, long long ldo, int H, int L, float scale_log2e) {
  constexpr int NCH = AD * (int)sizeof(T) / 32;        // 32-byte K-steps of a 64-wide head row: 4 (bf16) / 8 (fp32)
  constexpr int EPC = 16 / (int)sizeof(T);             // elements per 16-byte chunk
  __shared__ __attribute__((aligned(16))) T vt[AD * VLD];
  const int lane = threadIdx.x, r32 = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * 32, head = blockIdx.y, n = blockIdx.z, D = H * AD;
  const long long row0 = (long long)n * L;
  int len = L;
  if (lens) { const long long t = lens[n]; len = t < 0 ? 0 : (t > L ? L : (int)t); }
  const int qi = q0 + r32;
  if (q0 >= len) {                                      // rows that are never scored: defined output, no work
    if (qi < L) {
      const float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 8; ++c) st4<T>(o + (row0 + qi) * ldo + head * AD + 32 * h + 4 * c, z);
    }
    return;
  }
  const int qrow = qi < L ? qi : L - 1;                 // (rows past the sequence repeat the last one and are not stored)
  chunk16 qf[NCH];
  {
    const T* qp = qkv + (row0 + qrow) * ld + head * AD + h * EPC;
#pragma unroll
    for (int c = 0; c < NCH; ++c) qf[c] = *(const chunk16*)(qp + c * 2 * EPC);
  }
  f32x16 oacc[2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[cb][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int kend = q0 + 32 < L ? q0 + 32 : L;           // key tiles above the diagonal are skipped
  for (int j0 = 0; j0 < kend; j0 += 32) {
    const int krow = j0 + r32 < L ? j0 + r32 : L - 1;
    const T* kp = qkv + (row0 + krow) * ld + D + head * AD + h * EPC;
    const T* vp = qkv + (row0 + krow) * ld + 2 * D + head * AD + 32 * h;
    chunk16 kf[NCH], vf[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) kf[c] = *(const chunk16*)(kp + c * 2 * EPC);
#pragma unroll
    for (int c = 0; c < NCH; ++c) vf[c] = *(const chunk16*)(vp + c * EPC);       // 32 consecutive channels of key r32
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) Mma<T>::run(kf[c], qf[c], s);
    __syncthreads();                                    // the previous tile's V^T reads are done
#pragma unroll
    for (int c = 0; c < 32; ++c) vt[(32 * h + c) * VLD + r32] = chunk_elem<T>(vf[c / EPC], c % EPC);
    float p[16], tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      p[r] = key <= qi ? s[r] * scale_log2e : -INFINITY;
      tmax = fmaxf(tmax, p[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);                    // finite from the first tile on: key 0 is visible to every query
    const float corr = exp2f(m - mn);
    float ts = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { p[r] = exp2f(p[r] - mn); ts += p[r]; }
    ts += __shfl_xor(ts, 32, 64);
    l = l * corr + ts; m = mn;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[cb][r] *= corr;
    __syncthreads();                                    // V^T of this tile is in LDS
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) PV<T>::run(vt + (32 * cb + r32) * VLD, h, p, oacc[cb]);
  }
  if (qi < L) {
    const float inv = 1.f / l;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float v[4] = {oacc[cb][4 * g] * inv, oacc[cb][4 * g + 1] * inv, oacc[cb][4 * g + 2] * inv, oacc[cb][4 * g + 3] * inv};
        st4<T>(o + (row0 + qi) * ldo + head * AD + 32 * cb + 8 * g + 4 * h, v);
      }
  }
}

// ---------------------------------------------------------------------------------------------
// fused head: a workgroup (4 waves, 2 x 2) owns 64 rows of h and walks the vocabulary in tiles of 64 columns; a wave's 32 x 32 accumulator holds W h^T (vocabulary
// entries in the registers, the row on the lane), so a lane keeps the running (max, sum) and the target logit of ITS row over the columns it sees and nothing crosses
// lanes until the end, when the 4 partial states of a row (2 column halves x 2 lane halves) are merged through LDS.  Operand tiles use the LDS image of the GEMM family
// (128 bytes of K per row + 16 of padding); the loads of step i + 1 are in flight during the MFMAs of step i.  Rows of W past V and rows of h past R are never read (the
// row index is clamped; what a clamped row contributes is masked).
// ---------------------------------------------------------------------------------------------
constexpr int HB = 64;
template <typename T>
__global__ __launch_bounds__(256) void lm_head_nll_kernel(const T* hid, long long ldh, const T* W, long long ldw, const float* bias, const long long* tgt, float* nll,
                                                          long long R, int V, int D) {
  constexpr int KE = BKB / (int)sizeof(T), EPC = 16 / (int)sizeof(T);
  __shared__ __attribute__((aligned(16))) char As[HB * LDS_ROW];
  __shared__ __attribute__((aligned(16))) char Bs[HB * LDS_ROW];
  __shared__ float red[HB][4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, h = lane >> 5;
  const long long m0 = (long long)blockIdx.x * HB;
  const int ksteps = D / KE, ntiles = (V + HB - 1) / HB, total = ksteps * ntiles;
  const int lrow = tid >> 3, lch = tid & 7;            // staging: rows lrow and lrow + 32, 16-byte chunk lch of the K-step
  const long long arow0 = (m0 + lrow < R ? m0 + lrow : R - 1) * ldh, arow1 = (m0 + lrow + 32 < R ? m0 + lrow + 32 : R - 1) * ldh;
  const long long myrow = m0 + wm * 32 + (lane & 31);
  const long long t64 = myrow < R ? tgt[myrow] : -1;
  const int mytgt = (t64 >= 0 && t64 < V) ? (int)t64 : -1;
  u32x4 pa0, pa1, pw0, pw1;        // (vector values, not structs: a struct assigned under a condition ends up in scratch)
#define LM_HEAD_ISSUE(it_) do { \
    const int n0_ = ((it_) / ksteps) * HB, k0_ = ((it_) % ksteps) * KE + lch * EPC, w0_ = n0_ + lrow, w1_ = n0_ + lrow + 32; \
    pa0 = *(const u32x4*)(hid + arow0 + k0_); pa1 = *(const u32x4*)(hid + arow1 + k0_); \
    pw0 = *(const u32x4*)(W + (long long)(w0_ < V ? w0_ : V - 1) * ldw + k0_); pw1 = *(const u32x4*)(W + (long long)(w1_ < V ? w1_ : V - 1) * ldw + k0_); } while (0)
  float m = -INFINITY, s = 0.f, tl = 0.f;
  LM_HEAD_ISSUE(0);
  int it = 0;
  for (int tile = 0; tile < ntiles; ++tile) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int ks = 0; ks < ksteps; ++ks, ++it) {
      __syncthreads();
      *(u32x4*)(As + lrow * LDS_ROW + lch * 16) = pa0; *(u32x4*)(As + (lrow + 32) * LDS_ROW + lch * 16) = pa1;
      *(u32x4*)(Bs + lrow * LDS_ROW + lch * 16) = pw0; *(u32x4*)(Bs + (lrow + 32) * LDS_ROW + lch * 16) = pw1;
      __syncthreads();
      if (it + 1 < total) LM_HEAD_ISSUE(it + 1);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const chunk16 fw = *(const chunk16*)(Bs + (wn * 32 + (lane & 31)) * LDS_ROW + h * 16 + kk * 32);
        const chunk16 fh = *(const chunk16*)(As + (wm * 32 + (lane & 31)) * LDS_ROW + h * 16 + kk * 32);
        Mma<T>::run(fw, fh, acc);
      }
    }
    // this column tile is complete: fold it into the lane's running state
    const int cbase = tile * HB + wn * 32 + 4 * h;
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int col = cbase + (r & 3) + 8 * (r >> 2);
      const float v = col < V ? acc[r] + bias[col < V ? col : 0] : -INFINITY;
      acc[r] = v;
      tl = col == mytgt ? v : tl;
      tmax = fmaxf(tmax, v);
    }
    const float mn = fmaxf(m, tmax);
    if (mn > -INFINITY) {                               // (a lane whose columns were all past V so far has nothing to add)
      float ts = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) ts += __expf(acc[r] - mn);
      s = s * __expf(m - mn) + ts; m = mn;
    }
  }
  red[wm * 32 + (lane & 31)][wn * 2 + h][0] = m; red[wm * 32 + (lane & 31)][wn * 2 + h][1] = s; red[wm * 32 + (lane & 31)][wn * 2 + h][2] = tl;
  __syncthreads();
  if (tid < HB && m0 + tid < R) {
    float M = -INFINITY, S = 0.f, TL = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) M = fmaxf(M, red[tid][q][0]);
#pragma unroll
    for (int q = 0; q < 4; ++q) { if (red[tid][q][1] > 0.f) S += red[tid][q][1] * __expf(red[tid][q][0] - M); TL += red[tid][q][2]; }
    const long long t = tgt[m0 + tid];
    nll[m0 + tid] = (t >= 0 && t < V) ? (M + logf(S)) - TL : 0.f;
  }
}

#undef LM_HEAD_ISSUE

// ---------------------------------------------------------------------------------------------
// per-hypothesis nll sums (one thread per hypothesis, fixed order), then beam + LM total and the first maximum (one wave per utterance)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lm_segment_sum_kernel(const float* nll, const long long* lens, long long S, int L, float* out) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  long long len = lens[s]; len = len < 0 ? 0 : (len > L ? L : len);
  float sum = 0.f;
  for (int t = 0; t + 1 < len; ++t) sum += nll[s * L + t];
  out[s] = sum;
}

__global__ __launch_bounds__(64) void lm_rescore_kernel(const float* neural, const long long* lens, const float* beam, float alpha, float beta2, int K, float* total,
                                                        long long* best) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float bv = -INFINITY; int bi = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const long long s = (long long)b * K + k;
    const long long len = lens[s];
    const float bs = beam[s];
    const float tot = (bs > -INFINITY && len >= 1) ? bs - alpha * neural[s] + beta2 * (float)(len - 1) : -INFINITY;       // empty slots never win
    total[s] = tot;
    if (tot > bv) { bv = tot; bi = k; }                 // (k ascends: the first maximum of this lane's slots)
  }
  for (int off = 32; off; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64); const int oi = __shfl_xor(bi, off, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) best[b] = bi == 0x7fffffff ? 0 : bi;
}

inline bool al16(const void* p) { return ((size_t)p & 15) == 0; }
}  // namespace

extern "C" int avec_embed_pos(int dtype, const long long* ids, const float* E, const float* P, void* out, int out_f32, long long N, int L, int V, int D, hipStream_t st) {
  AVEC_CHECK_ARG(dtype == AVEC_F32 || dtype == AVEC_BF16, "embed_pos: bad dtype %d", dtype);
  AVEC_CHECK_ARG(ids && E && P && out, "embed_pos: null pointer");
  AVEC_CHECK_ARG(N >= 1 && L >= 1 && V >= 1 && D >= 8 && D % 8 == 0, "embed_pos: bad dims N=%lld L=%d V=%d D=%d (D a multiple of 8)", N, L, V, D);
  AVEC_CHECK_ARG(al16(E) && al16(P) && al16(out), "embed_pos: tables and output must be 16-byte aligned");
  const long long rows = N * L, items = rows * (D / 8);
  const dim3 grid((unsigned)((items + 255) / 256));
  if (out_f32 || dtype == AVEC_F32) hipLaunchKernelGGL(embed_pos_kernel<float>, grid, dim3(256), 0, st, ids, E, P, (float*)out, rows, L, V, D);
  else hipLaunchKernelGGL(embed_pos_kernel<bf16>, grid, dim3(256), 0, st, ids, E, P, (bf16*)out, rows, L, V, D);
  AVEC_LAUNCH_CHECK(); return 0;
}

extern "C" int avec_causal_attention_supported(int d) { return d == AD; }

extern "C" int avec_causal_attention(int dtype, const void* qkv, long long ld, const long long* lens, void* o, long long ldo, int N, int H, int L, int d, float scale,
                                     hipStream_t st) {
  AVEC_CHECK_ARG(dtype == AVEC_F32 || dtype == AVEC_BF16, "causal_attention: bad dtype %d", dtype);
  AVEC_CHECK_ARG(qkv && o, "causal_attention: null pointer");
  AVEC_CHECK_ARG(d == AD, "causal_attention: head width %d is not supported (only %d)", d, AD);
  AVEC_CHECK_ARG(N >= 1 && N <= 65535 && H >= 1 && H <= 65535 && L >= 1, "causal_attention: bad dims N=%d H=%d L=%d", N, H, L);
  const int epc = dtype == AVEC_BF16 ? 8 : 4;
  AVEC_CHECK_ARG(ld >= 3ll * H * d && ldo >= (long long)H * d && ld % epc == 0 && ldo % 4 == 0 && al16(qkv) && ((size_t)o & 15) == 0,
                 "causal_attention: ld=%lld ldo=%lld: rows of Q|K|V must be 16-byte aligned and hold 3*H*d elements", ld, ldo);
  const dim3 grid((unsigned)((L + 31) / 32), (unsigned)H, (unsigned)N);
  const float sl = scale * 1.4426950408889634f;
  if (dtype == AVEC_BF16) hipLaunchKernelGGL(causal_attn_kernel<bf16>, grid, dim3(64), 0, st, (const bf16*)qkv, ld, lens, (bf16*)o, ldo, H, L, sl);
  else hipLaunchKernelGGL(causal_attn_kernel<float>, grid, dim3(64), 0, st, (const float*)qkv, ld, lens, (float*)o, ldo, H, L, sl);
  AVEC_LAUNCH_CHECK(); return 0;
}

// the running softmax state lives in registers and 3 KB of LDS: no global workspace at all, whatever R and V
extern "C" long long avec_lm_head_nll_workspace_bytes(long long R, int V, int D) { (void)R; (void)V; (void)D; return 0; }

extern "C" int avec_lm_head_nll(int dtype, const void* h, long long ldh, const void* W, long long ldw, const float* bias, const long long* tgt, float* nll, long long R, int V,
                                int D, void* workspace, long long workspace_bytes, hipStream_t st) {
  (void)workspace;
  AVEC_CHECK_ARG(dtype == AVEC_F32 || dtype == AVEC_BF16, "lm_head_nll: bad dtype %d", dtype);
  AVEC_CHECK_ARG(h && W && bias && tgt && nll, "lm_head_nll: null pointer");
  AVEC_CHECK_ARG(workspace_bytes >= avec_lm_head_nll_workspace_bytes(R, V, D), "lm_head_nll: workspace too small");
  const int ke = dtype == AVEC_BF16 ? 64 : 32, epc = dtype == AVEC_BF16 ? 8 : 4;
  AVEC_CHECK_ARG(R >= 1 && R <= 64ll * 0x7fffffff && V >= 1 && D >= ke && D % ke == 0, "lm_head_nll: bad dims R=%lld V=%d D=%d (D a multiple of %d)", R, V, D, ke);
  AVEC_CHECK_ARG(ldh >= D && ldw >= D && ldh % epc == 0 && ldw % epc == 0 && al16(h) && al16(W), "lm_head_nll: ldh=%lld ldw=%lld: rows must be 16-byte aligned", ldh, ldw);
  const dim3 grid((unsigned)((R + HB - 1) / HB));
  if (dtype == AVEC_BF16) hipLaunchKernelGGL(lm_head_nll_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)h, ldh, (const bf16*)W, ldw, bias, tgt, nll, R, V, D);
  else hipLaunchKernelGGL(lm_head_nll_kernel<float>, grid, dim3(256), 0, st, (const float*)h, ldh, (const float*)W, ldw, bias, tgt, nll, R, V, D);
  AVEC_LAUNCH_CHECK(); return 0;
}

extern "C" int avec_lm_segment_sum(const float* nll, const long long* lens, long long S, int L, float* out, hipStream_t st) {
  AVEC_CHECK_ARG(nll && lens && out && S >= 1 && L >= 1, "lm_segment_sum: bad arguments");
  hipLaunchKernelGGL(lm_segment_sum_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, nll, lens, S, L, out);
  AVEC_LAUNCH_CHECK(); return 0;
}

extern "C" int avec_lm_rescore_select(const float* neural, const long long* lens, const float* beam_score, float alpha, float beta, int B, int K, float* total, long long* best,
                                      hipStream_t st) {
  AVEC_CHECK_ARG(neural && lens && beam_score && total && best, "lm_rescore_select: null pointer");
  AVEC_CHECK_ARG(B >= 1 && K >= 1, "lm_rescore_select: bad dims B=%d K=%d", B, K);
  hipLaunchKernelGGL(lm_rescore_kernel, dim3(B), dim3(64), 0, st, neural, lens, beam_score, alpha, beta * beta, K, total, best);
  AVEC_LAUNCH_CHECK(); return 0;
}
