// Conformer convolution-module middle section (nnet/modules.py:375-376 + layers.Conv1d :82-198):
//   g = GLU(u) = u[:, :C] * sigmoid(u[:, C:]);   c[b][t'][ch] = bias[ch] + sum_k w[k][ch] * g[b][t'*s + k - (K-1)/2][ch]
// depthwise, zero "same" padding ((K-1)//2, K//2), stride s; channels-last throughout.  The depthwise
// weight lives tap-major ([K][C]) so channel vectors are contiguous.  BatchNorm batch statistics of
// the conv output are accumulated in the same pass.
#include "vec.h"
#include "avec_hip.h"

static constexpr int KMAX = 16;

template <typename T>
__device__ __forceinline__ void glu4(const T* u, long long row, int C, int col, float g[4]) {
  float a[4], b[4]; ld4<T>(u + row * 2 * C + col, a); ld4<T>(u + row * 2 * C + C + col, b);
  for (int e = 0; e < 4; ++e) g[e] = a[e] * sigmoidf_(b[e]);
}

// Workgroup = (128-channel slab, batch b, chunk of DW_TT output frames).  GLU(u) of the frames the chunk touches is computed ONCE into
// LDS (fp32, zero outside the sequence = the "same" padding), then every output frame reads its K taps from LDS.
static constexpr int DW_TT = 32;
template <typename T>
__device__ __forceinline__ void stage_glu(float* gs, const T* u, long long b, int Tn, int C, int col, int t_base, int nrows) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  // six rows per pass: all twelve loads are in flight before the first sigmoid (one load latency per pass instead of one per row)
  for (int r0 = ty; r0 < nrows; r0 += 48) {
    float a[6][4], bq[6][4];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const int r = r0 + 8 * q, t = t_base + r;
      const bool ok = r < nrows && col < C && t >= 0 && t < Tn;
      const long long row = ok ? b * Tn + t : b * Tn;          // clamped: the loads stay unconditional
      const int cc = col < C ? col : 0;
      ld4<T>(u + row * 2 * C + cc, a[q]); ld4<T>(u + row * 2 * C + C + cc, bq[q]);
      if (!ok) { a[q][0] = a[q][1] = a[q][2] = a[q][3] = 0.f; }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const int r = r0 + 8 * q;
      if (r < nrows) *(float4*)(gs + r * 128 + tx * 4) = make_float4(a[q][0] * sigmoidf_(bq[q][0]), a[q][1] * sigmoidf_(bq[q][1]), a[q][2] * sigmoidf_(bq[q][2]), a[q][3] * sigmoidf_(bq[q][3]));
    }
  }
}
template <typename T>
__global__ __launch_bounds__(256) void glu_dwconv_fwd_kernel(const T* __restrict__ u, const float* __restrict__ w, const float* __restrict__ bias, T* __restrict__ out,
                                                             float* stats, int B, int Tn, int C, int K, int stride, int To, int padl, int nchunks, ColWs ws) {
  extern __shared__ __attribute__((aligned(16))) float gs[];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; const int col = (blockIdx.x * 32 + tx) * 4;
  const int b = blockIdx.y / nchunks, to0 = (blockIdx.y - b * nchunks) * DW_TT; const int nto = min(DW_TT, To - to0);
  // the taps of this thread's four channels in registers, requested in front of the staging pass (one memory round trip for both): the tap loop used to fetch
  // w[k][col] from memory once per (row, tap) -- 60 dependent L1 / L2 round trips per thread, most of the kernel's 10 us (tools/block_trace.py)
  const bool wreg = K <= KMAX;
  float ww[KMAX][4], bb[4] = {0.f, 0.f, 0.f, 0.f};
  if (wreg && col < C) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { if (k < K) ld4<float>(w + (long long)k * C + col, ww[k]); else ww[k][0] = ww[k][1] = ww[k][2] = ww[k][3] = 0.f; }
  }
  if (col < C && bias) ld4<float>(bias + col, bb);
  stage_glu<T>(gs, u, b, Tn, C, col, to0 * stride - padl, (nto - 1) * stride + K);
  __syncthreads();
  float part[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if (col < C && wreg) {
    for (int r = ty; r < nto; r += 8) {
      float acc[4] = {bb[0], bb[1], bb[2], bb[3]};
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          const float4 g = *(const float4*)(gs + (r * stride + k) * 128 + tx * 4);
          acc[0] += ww[k][0] * g.x; acc[1] += ww[k][1] * g.y; acc[2] += ww[k][2] * g.z; acc[3] += ww[k][3] * g.w;
        }
      }
      st4<T>(out + ((long long)b * To + to0 + r) * C + col, acc);
      for (int e = 0; e < 4; ++e) { part[0][e] += acc[e]; part[1][e] += acc[e] * acc[e]; }
    }
  } else
  if (col < C) {
    for (int r = ty; r < nto; r += 8) {
      float acc[4] = {bb[0], bb[1], bb[2], bb[3]};
      for (int k = 0; k < K; ++k) {
        const float4 g = *(const float4*)(gs + (r * stride + k) * 128 + tx * 4); float ww[4]; ld4<float>(w + (long long)k * C + col, ww);
        acc[0] += ww[0] * g.x; acc[1] += ww[1] * g.y; acc[2] += ww[2] * g.z; acc[3] += ww[3] * g.w;
      }
      st4<T>(out + ((long long)b * To + to0 + r) * C + col, acc);
      for (int e = 0; e < 4; ++e) { part[0][e] += acc[e]; part[1][e] += acc[e] * acc[e]; }
    }
  }
  float* const dst[2] = {stats, stats ? stats + C : nullptr};
  if (stats) colreduce_atomic<2>(part, dst, col, C, ws);
}

// du (act [B*T][2C]) from dc (act [B*To][C])
template <typename T>
__global__ __launch_bounds__(256) void dwconv_glu_bwd_input_kernel(const T* __restrict__ dc, const T* __restrict__ u, const float* __restrict__ w, T* __restrict__ du,
                                                                   int B, int Tn, int C, int K, int stride, int To, int padl) {
  const long long n4 = (long long)B * Tn * (C / 4);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const int col = (int)(i % (C / 4)) * 4; const long long row = i / (C / 4); const int t = (int)(row % Tn); const long long b = row / Tn;
    float dg[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
      const int tt = t + padl - k; if (tt < 0) break;
      const int to = tt / stride; if (to * stride != tt || to >= To) continue;
      float d[4], ww[4]; ld4<T>(dc + (b * To + to) * C + col, d); ld4<float>(w + (long long)k * C + col, ww);
      for (int e = 0; e < 4; ++e) dg[e] += ww[e] * d[e];
    }
    float a[4], bq[4], o1[4], o2[4]; ld4<T>(u + row * 2 * C + col, a); ld4<T>(u + row * 2 * C + C + col, bq);
    for (int e = 0; e < 4; ++e) { const float s = sigmoidf_(bq[e]); o1[e] = dg[e] * s; o2[e] = dg[e] * a[e] * s * (1.f - s); }
    st4<T>(du + row * 2 * C + col, o1); st4<T>(du + row * 2 * C + C + col, o2);
  }
}

// dw[k][c] += sum dc * g(shifted);  dbias[c] += sum dc        (same tiling as the forward: GLU staged once per chunk in LDS)
template <typename T>
__global__ __launch_bounds__(256) void dwconv_bwd_weight_kernel(const T* __restrict__ dc, const T* __restrict__ u, float* dw, float* dbias,
                                                                int B, int Tn, int C, int K, int stride, int To, int padl, int nchunks, ColWs ws) {
  extern __shared__ __attribute__((aligned(16))) float gs[];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; const int col = (blockIdx.x * 32 + tx) * 4;
  const int b = blockIdx.y / nchunks, to0 = (blockIdx.y - b * nchunks) * DW_TT; const int nto = min(DW_TT, To - to0);
  stage_glu<T>(gs, u, b, Tn, C, col, to0 * stride - padl, (nto - 1) * stride + K);
  __syncthreads();
  float part[KMAX + 1][4];
#pragma unroll
  for (int k = 0; k <= KMAX; ++k) for (int e = 0; e < 4; ++e) part[k][e] = 0.f;
  if (col < C) {
    float dq[DW_TT / 8][4];                      // this thread's rows of dc, all requested before the first one is used
#pragma unroll
    for (int q = 0; q < DW_TT / 8; ++q) {
      const int r = ty + 8 * q;
      ld4<T>(dc + ((long long)b * To + to0 + (r < nto ? r : 0)) * C + col, dq[q]);
      if (r >= nto) { dq[q][0] = dq[q][1] = dq[q][2] = dq[q][3] = 0.f; }
    }
#pragma unroll
    for (int q = 0; q < DW_TT / 8; ++q) {
      const int r = ty + 8 * q;
      if (r >= nto) break;
#pragma unroll
      for (int e = 0; e < 4; ++e) part[KMAX][e] += dq[q][e];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          const float4 g = *(const float4*)(gs + (r * stride + k) * 128 + tx * 4);
          part[k][0] += dq[q][0] * g.x; part[k][1] += dq[q][1] * g.y; part[k][2] += dq[q][2] * g.z; part[k][3] += dq[q][3] * g.w;
        }
      }
    }
  }
  // reduce the 17 partial vectors over the 8 row groups of the workgroup in ONE pass (the generic colreduce_atomic walks them one at a time: 34 barriers):
  // the two row groups of a wave meet by a shuffle, the four waves through the (now dead) GLU image
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k <= KMAX; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) part[k][e] += __shfl_xor(part[k][e], 32, 64);
  if (lane < 32) {
#pragma unroll
    for (int k = 0; k <= KMAX; ++k) *(float4*)(gs + ((wv * (KMAX + 1) + k) * 32 + tx) * 4) = make_float4(part[k][0], part[k][1], part[k][2], part[k][3]);
  }
  __syncthreads();
  float* mine = ws.partial ? ws_slot(ws, blockIdx.x, blockIdx.y, gridDim.y, (KMAX + 1) * 128) : nullptr;
  for (int i = threadIdx.x; i < (KMAX + 1) * 128; i += 256) {
    const int k = i >> 7, c = i & 127;
    const float v = gs[(0 * (KMAX + 1) + k) * 128 + c] + gs[(1 * (KMAX + 1) + k) * 128 + c] + gs[(2 * (KMAX + 1) + k) * 128 + c] + gs[(3 * (KMAX + 1) + k) * 128 + c];
    if (mine) mine[i] = v;
    else {
      const int cc = blockIdx.x * 128 + c;
      float* d = k == KMAX ? dbias : (k < K ? dw + (long long)k * C : nullptr);
      if (d && cc < C) atomicAdd(d + cc, v);
    }
  }
}

// Both halves of the backward pass in ONE launch (stride 1: every conformer block but the two stage boundaries): the workgroup of the weight-gradient kernel also
// stages the dc rows its 32 frames can see (K - 1 rows of halo, fp32, zero outside the sequence) and produces du for those frames -- one launch, one pass over u and dc
// instead of two (the input-gradient kernel re-read K dc rows per element from L2).  LDS: (31 + K) x 128 floats twice.
// BatchNorm(+Swish) backward folded into the staging pass (round 6): with bnb.c set, `dc` is the gradient of the BatchNorm + Swish OUTPUT and the rows staged in LDS are
//   dc = gamma rstd (d - mean(d) - xhat mean(d xhat)),  d = da * swish'(scale c + shift)          (avec_bn_bwd_apply's arithmetic, act = Swish)
// from the reduced sums `dstats` -- the apply pass and its tensor disappear from the conformer block's chain; workgroup (0, 0) adds dgamma / dbeta.
struct DwBnb { const void* c; const float* ss; const float* gamma; const float* dstats; float inv_n; float* dgamma; float* dbeta; };
template <typename T>
__global__ __launch_bounds__(256) void dwconv_glu_bwd_fused_kernel(const T* __restrict__ dc, const T* __restrict__ u, const float* __restrict__ w, T* __restrict__ du, float* dw, float* dbias,
                                                                   int B, int Tn, int C, int K, int padl, int nchunks, ColWs ws, DwBnb bnb = DwBnb{nullptr}) {
  extern __shared__ __attribute__((aligned(16))) float gs[];
  const int NR = DW_TT - 1 + K;
  float* const ds = gs + NR * 128;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; const int col = (blockIdx.x * 32 + tx) * 4;
  const int b = blockIdx.y / nchunks, t0 = (blockIdx.y - b * nchunks) * DW_TT; const int nto = min(DW_TT, Tn - t0);
  stage_glu<T>(gs, u, b, Tn, C, col, t0 - padl, nto - 1 + K);
  {                                                            // dc rows of frames t0 + padl - (K - 1) + j, j < nto - 1 + K
    const int f0 = t0 + padl - (K - 1), nrows = nto - 1 + K, cc = col < C ? col : 0;
    float bA[4], bM1[4], bM2[4], bMu[4], bRs[4], bSc[4], bSh[4];
    if (bnb.c) {
      float g4[4], s1[4], s2[4];
      ld4<float>(bnb.ss + cc, bSc); ld4<float>(bnb.ss + C + cc, bSh); ld4<float>(bnb.ss + 2 * C + cc, bMu); ld4<float>(bnb.ss + 3 * C + cc, bRs);
      ld4<float>(bnb.gamma + cc, g4); ld4<float>(bnb.dstats + cc, s1); ld4<float>(bnb.dstats + C + cc, s2);
#pragma unroll
      for (int e = 0; e < 4; ++e) { bA[e] = g4[e] * bRs[e]; bM1[e] = s1[e] * bnb.inv_n; bM2[e] = s2[e] * bnb.inv_n; }
      if (blockIdx.y == 0 && ty == 0 && col < C && bnb.dgamma) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { atomicAdd(bnb.dgamma + col + e, s2[e]); atomicAdd(bnb.dbeta + col + e, s1[e]); }
      }
    }
    for (int r0 = ty; r0 < nrows; r0 += 48) {
      float d[6][4];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const int r = r0 + 8 * q, f = f0 + r; const bool ok = r < nrows && col < C && f >= 0 && f < Tn;
        ld4<T>(dc + ((long long)b * Tn + (ok ? f : 0)) * C + cc, d[q]);
        if (bnb.c) {
          float cv[4]; ld4<T>((const T*)bnb.c + ((long long)b * Tn + (ok ? f : 0)) * C + cc, cv);
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float dd = d[q][e] * dswishf_(cv[e] * bSc[e] + bSh[e]); d[q][e] = bA[e] * (dd - bM1[e] - (cv[e] - bMu[e]) * bRs[e] * bM2[e]); }
        }
        if (!ok) d[q][0] = d[q][1] = d[q][2] = d[q][3] = 0.f;
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) { const int r = r0 + 8 * q; if (r < nrows) *(float4*)(ds + r * 128 + tx * 4) = make_float4(d[q][0], d[q][1], d[q][2], d[q][3]); }
    }
  }
  __syncthreads();
  float part[KMAX + 1][4];
#pragma unroll
  for (int k = 0; k <= KMAX; ++k) for (int e = 0; e < 4; ++e) part[k][e] = 0.f;
  if (col < C) {
    float ww[KMAX][4];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { if (k < K) ld4<float>(w + (long long)k * C + col, ww[k]); else ww[k][0] = ww[k][1] = ww[k][2] = ww[k][3] = 0.f; }
    const int own = K - 1 - padl;                              // ds row of this chunk's frame 0
#pragma unroll
    for (int q = 0; q < DW_TT / 8; ++q) {
      const int r = ty + 8 * q;
      if (r >= nto) break;
      const long long row = (long long)b * Tn + t0 + r;
      float a[4], bq[4]; ld4<T>(u + row * 2 * C + col, a); ld4<T>(u + row * 2 * C + C + col, bq);      // (requested before the tap loop: L2 hits, the staging pass has just read them)
      const float4 dq = *(const float4*)(ds + (own + r) * 128 + tx * 4);
      part[KMAX][0] += dq.x; part[KMAX][1] += dq.y; part[KMAX][2] += dq.z; part[KMAX][3] += dq.w;
      float dg[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          const float4 g = *(const float4*)(gs + (r + k) * 128 + tx * 4);
          part[k][0] += dq.x * g.x; part[k][1] += dq.y * g.y; part[k][2] += dq.z * g.z; part[k][3] += dq.w * g.w;
          const float4 dd = *(const float4*)(ds + (r + K - 1 - k) * 128 + tx * 4);
          dg[0] += ww[k][0] * dd.x; dg[1] += ww[k][1] * dd.y; dg[2] += ww[k][2] * dd.z; dg[3] += ww[k][3] * dd.w;
        }
      }
      float o1[4], o2[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float sg = sigmoidf_(bq[e]); o1[e] = dg[e] * sg; o2[e] = dg[e] * a[e] * sg * (1.f - sg); }
      st4<T>(du + row * 2 * C + col, o1); st4<T>(du + row * 2 * C + C + col, o2);
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k <= KMAX; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) part[k][e] += __shfl_xor(part[k][e], 32, 64);
  if (lane < 32) {
#pragma unroll
    for (int k = 0; k <= KMAX; ++k) *(float4*)(gs + ((wv * (KMAX + 1) + k) * 32 + tx) * 4) = make_float4(part[k][0], part[k][1], part[k][2], part[k][3]);
  }
  __syncthreads();
  float* mine = ws.partial ? ws_slot(ws, blockIdx.x, blockIdx.y, gridDim.y, (KMAX + 1) * 128) : nullptr;
  for (int i = threadIdx.x; i < (KMAX + 1) * 128; i += 256) {
    const int k = i >> 7, c = i & 127;
    const float v = gs[(0 * (KMAX + 1) + k) * 128 + c] + gs[(1 * (KMAX + 1) + k) * 128 + c] + gs[(2 * (KMAX + 1) + k) * 128 + c] + gs[(3 * (KMAX + 1) + k) * 128 + c];
    if (mine) mine[i] = v;
    else {
      const int cc = blockIdx.x * 128 + c;
      float* d = k == KMAX ? dbias : (k < K ? dw + (long long)k * C : nullptr);
      if (d && cc < C) atomicAdd(d + cc, v);
    }
  }
}

extern "C" int avec_glu_dwconv_fwd(int dtype, const void* u, const float* w, const float* bias, void* out, float* stats,
                                   int B, int T_, int C, int K, int stride, int pad_left, hipStream_t st) {
  AVEC_CHECK_ARG(u && w && out && B > 0 && T_ > 0 && C > 0 && C % 4 == 0 && K > 0 && K <= KMAX && stride > 0 && pad_left >= 0 && pad_left < K, "glu_dwconv_fwd: bad arguments (C=%d K=%d pad_left=%d)", C, K, pad_left);
  const int To = (T_ - 1) / stride + 1;
  const int nchunks = (To + DW_TT - 1) / DW_TT;
  dim3 grid((unsigned)((C / 4 + 31) / 32), (unsigned)(B * nchunks)); const ColPlan plan = ColPlan::grid<2>(grid, C, st, stats != nullptr);
  const size_t lds = (size_t)((DW_TT - 1) * stride + K) * 128 * sizeof(float);
  AVEC_CHECK_ARG(lds <= 64 * 1024, "glu_dwconv_fwd: stride %d too large", stride);
  DISPATCH_T(dtype, hipLaunchKernelGGL(glu_dwconv_fwd_kernel<T>, grid, dim3(256), lds, st, (const T*)u, w, bias, (T*)out, stats, B, T_, C, K, stride, To, pad_left, nchunks, plan.ws));
  AVEC_LAUNCH_CHECK();
  return plan.finish({stats, stats + C}, C, st);
}
// BatchNorm finalize (norm.hip bn_finalize_kernel, training mode) reading the two-pass column-reduction partials of glu_dwconv_fwd_kernel directly: the second pass
// (ColPlan::finish) and the finalize were two ~4.8 us launches back to back in every conformer block's dependent chain (round 6).  block = 16 channels x 16 slot lanes;
// partial[(colblock * nslots + slot) * 256 + n * 128 + w], channel c = 128 colblock + w, n = 0 sum / 1 sum of squares.
__global__ __launch_bounds__(256) void bn_finalize_ws_kernel(const float* __restrict__ partial, int nslots, float count, const float* gamma, const float* beta, float* rmean, float* rvar,
                                                             long long* nbt, float momentum, float eps, float* ss, int C) {
  __shared__ float red[2][16][17];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const bool lead = rl == 0 && c < C;
  float gm = 0.f, bt = 0.f, rm = 0.f, rv = 0.f;
  if (lead) { gm = gamma[c]; bt = beta[c]; if (rmean) { rm = rmean[c]; rv = rvar[c]; } }
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const float* p = partial + (size_t)(c >> 7) * nslots * 256 + (c & 127);
    for (int r = rl; r < nslots; r += 16) { s1 += p[(size_t)r * 256]; s2 += p[(size_t)r * 256 + 128]; }
  }
  red[0][rl][cl] = s1; red[1][rl][cl] = s2;
  __syncthreads();
  if (!lead) return;
  s1 = 0.f; s2 = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) { s1 += red[0][k][cl]; s2 += red[1][k][cl]; }
  const float n = count;
  const float mean = s1 / n, var = fmaxf(s2 / n - mean * mean, 0.f);
  if (rmean && isfinite(mean) && isfinite(var)) {
    rmean[c] = (1.f - momentum) * rm + momentum * mean;
    rvar[c] = (1.f - momentum) * rv + momentum * var * (n / fmaxf(n - 1.f, 1.f));
    if (c == 0 && nbt) *nbt += 1;
  }
  const float rs = rsqrtf(var + eps);
  ss[c] = gm * rs; ss[C + c] = bt - mean * gm * rs; ss[2 * C + c] = mean; ss[3 * C + c] = rs;
}

// avec_glu_dwconv_fwd + avec_bn_finalize (training mode, local batch statistics over count = B * To rows) as TWO launches instead of three; `stats` ([2C], zeroed) is used
// only when the reduction runs on atomics (no workspace registered / few partials)
extern "C" int avec_glu_dwconv_fwd_bn(int dtype, const void* u, const float* w, const float* bias, void* out, float* stats, int B, int T_, int C, int K, int stride, int pad_left,
                                      const float* gamma, const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                                      float* ss, hipStream_t st) {
  AVEC_CHECK_ARG(u && w && out && stats && gamma && beta && ss && B > 0 && T_ > 0 && C > 0 && C % 4 == 0 && K > 0 && K <= KMAX && stride > 0 && pad_left >= 0 && pad_left < K,
                 "glu_dwconv_fwd_bn: bad arguments (C=%d K=%d pad_left=%d)", C, K, pad_left);
  const int To = (T_ - 1) / stride + 1;
  const int nchunks = (To + DW_TT - 1) / DW_TT;
  dim3 grid((unsigned)((C / 4 + 31) / 32), (unsigned)(B * nchunks)); const ColPlan plan = ColPlan::grid<2>(grid, C, st);
  const size_t lds = (size_t)((DW_TT - 1) * stride + K) * 128 * sizeof(float);
  AVEC_CHECK_ARG(lds <= 64 * 1024, "glu_dwconv_fwd_bn: stride %d too large", stride);
  DISPATCH_T(dtype, hipLaunchKernelGGL(glu_dwconv_fwd_kernel<T>, grid, dim3(256), lds, st, (const T*)u, w, bias, (T*)out, stats, B, T_, C, K, stride, To, pad_left, nchunks, plan.ws));
  AVEC_LAUNCH_CHECK();
  const float count = (float)((long long)B * To);
  if (plan.ws.partial) {
    hipLaunchKernelGGL(bn_finalize_ws_kernel, dim3((C + 15) / 16), dim3(256), 0, st, (const float*)plan.ws.partial, (int)plan.nslots, count, gamma, beta, running_mean, running_var,
                       num_batches_tracked, momentum, eps, ss, C);
    AVEC_LAUNCH_CHECK();
    return 0;
  }
  return avec_bn_finalize(stats, 1, nullptr, count, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, ss, C, 1, st);
}
// second pass of the depthwise weight gradient: partial rows are [KMAX + 1][128], taps 0..K-1 go to dw[k][C], row KMAX to dbias
static int dw_finish(const ColPlan& plan, float* dw, float* dbias, int C, int K, hipStream_t st) {
  float* dst[KMAX + 1];
  for (int k = 0; k < KMAX; ++k) dst[k] = (k < K) ? dw + (long long)k * C : nullptr;
  dst[KMAX] = dbias;
  return plan.finish(dst, C, st);
}
// avec_bn_bwd_apply (act = Swish, local batch statistics over B * T rows, dstats = the reduced (sum d, sum d xhat) of avec_bn_bwd_reduce) + avec_dwconv_glu_bwd in ONE launch
// (stride 1): da = gradient of the BatchNorm + Swish output, c = the BatchNorm input (= the depthwise convolution's output); dgamma / dbeta += dstats.
extern "C" int avec_dwconv_glu_bwd_bn(int dtype, const void* da, const void* c, const float* ss, const float* gamma, const float* dstats, float count, const void* u, const float* w,
                                      void* du, float* dw, float* dbias, float* dgamma, float* dbeta, int B, int T_, int C, int K, int pad_left, hipStream_t st) {
  AVEC_CHECK_ARG(da && c && ss && gamma && dstats && count > 0.f && u && w && du && dw && B > 0 && T_ > 0 && C > 0 && C % 4 == 0 && K > 0 && K <= KMAX && pad_left >= 0 && pad_left < K,
                 "dwconv_glu_bwd_bn: bad arguments");
  AVEC_CHECK_ARG((dgamma == nullptr) == (dbeta == nullptr), "dwconv_glu_bwd_bn: dgamma and dbeta come together (both or neither)");      // the kernel adds to both under one test
  const int nchunks = (T_ + DW_TT - 1) / DW_TT;
  dim3 grid((unsigned)((C / 4 + 31) / 32), (unsigned)(B * nchunks)); const ColPlan plan = ColPlan::grid<KMAX + 1>(grid, C, st);
  size_t l2 = (size_t)2 * (DW_TT - 1 + K) * 128 * sizeof(float);
  if (l2 < (size_t)4 * (KMAX + 1) * 128 * sizeof(float)) l2 = (size_t)4 * (KMAX + 1) * 128 * sizeof(float);
  AVEC_CHECK_ARG(l2 <= 64 * 1024, "dwconv_glu_bwd_bn: kernel size %d too large", K);
  DwBnb bnb{c, ss, gamma, dstats, 1.f / count, dgamma, dbeta};
  DISPATCH_T(dtype, hipLaunchKernelGGL(dwconv_glu_bwd_fused_kernel<T>, grid, dim3(256), l2, st, (const T*)da, (const T*)u, w, (T*)du, dw, dbias, B, T_, C, K, pad_left, nchunks, plan.ws, bnb));
  AVEC_LAUNCH_CHECK();
  return dw_finish(plan, dw, dbias, C, K, st);
}
extern "C" int avec_dwconv_glu_bwd(int dtype, const void* dc, const void* u, const float* w, void* du, float* dw, float* dbias,
                                   int B, int T_, int C, int K, int stride, int pad_left, hipStream_t st) {
  AVEC_CHECK_ARG(dc && u && w && du && dw && B > 0 && T_ > 0 && C > 0 && C % 4 == 0 && K > 0 && K <= KMAX && stride > 0 && pad_left >= 0 && pad_left < K, "dwconv_glu_bwd: bad arguments");
  const int To = (T_ - 1) / stride + 1;
  long long n4 = (long long)B * T_ * (C / 4); long long nb = (n4 + 255) / 256; if (nb > 4096) nb = 4096;
  const int nchunks = (To + DW_TT - 1) / DW_TT;
  dim3 grid((unsigned)((C / 4 + 31) / 32), (unsigned)(B * nchunks)); const ColPlan plan = ColPlan::grid<KMAX + 1>(grid, C, st);
  size_t lds = (size_t)((DW_TT - 1) * stride + K) * 128 * sizeof(float);
  if (lds < (size_t)4 * (KMAX + 1) * 128 * sizeof(float)) lds = (size_t)4 * (KMAX + 1) * 128 * sizeof(float);      // the reduction image of the weight-gradient kernel
  AVEC_CHECK_ARG(lds <= 64 * 1024, "dwconv_glu_bwd: stride %d too large", stride);
  if (stride == 1) {
    size_t l2 = (size_t)2 * (DW_TT - 1 + K) * 128 * sizeof(float); if (l2 < lds) l2 = lds;
    DISPATCH_T(dtype, hipLaunchKernelGGL(dwconv_glu_bwd_fused_kernel<T>, grid, dim3(256), l2, st, (const T*)dc, (const T*)u, w, (T*)du, dw, dbias, B, T_, C, K, pad_left, nchunks, plan.ws));
  } else
  DISPATCH_T(dtype, hipLaunchKernelGGL(dwconv_glu_bwd_input_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, (const T*)dc, (const T*)u, w, (T*)du, B, T_, C, K, stride, To, pad_left);
             hipLaunchKernelGGL(dwconv_bwd_weight_kernel<T>, grid, dim3(256), lds, st, (const T*)dc, (const T*)u, dw, dbias, B, T_, C, K, stride, To, pad_left, nchunks, plan.ws));
  AVEC_LAUNCH_CHECK();
  return dw_finish(plan, dw, dbias, C, K, st);
}

// ================================================================================================================================================================
// Streaming form (nnet.ConformerStreamSession): GLU -> causal depthwise conv (stride s) -> eval-mode BatchNorm scale / shift -> Swish of ONE chunk of Tq frames per
// utterance slot, on the concatenation [carried left context | chunk].  The carried context is the last K - 1 rows of u (pre-GLU, 2C channels, act dtype) of the
// slot: the convolution reads exactly the operands avec_glu_dwconv_fwd reads offline, taps in the same order, fp32 accumulation.
//   slot b starts at stage position p0 = reset[b] ? 0 : pos[b] / div and takes n = ceil(chunk_len[b] / div) (<= Tq) frames; a context row whose position
//   p0 - (K - 1) + r is negative is absent (a zero GLU output: the causal zero padding) whatever the buffer holds -- a reset costs no memset.
//   output row o (< To = Tq / s) is the frame at chunk position o * s = global position p0 + o * s (a multiple of s, where the offline To = (T - 1) / s + 1 puts it).
//   new context = the last K - 1 rows of [old context | first n chunk rows]; rows at or beyond n never enter it.
// Workgroup = (128-channel slab, slot): it owns the slab's columns of the slot's context rows alone.  State ordering: every read of the old context (the GLU staging
// pass and the rows that move up into the new context, kept in registers) happens BEFORE the workgroup barrier, every write of the new context AFTER it, and no
// other workgroup touches these columns of this slot: in place without a race.
// ================================================================================================================================================================
// the body of both streaming kernels: the slot starts at stage position p0, all Tq rows are convolved, the first n enter the carried context
template <typename T>
__device__ __forceinline__ void glu_dwconv_stream_body(const T* __restrict__ u, const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ ss,
                                                       T* __restrict__ out, T* state, long long p0, int n, int Tq, int C, int K, int stride, int To) {
  extern __shared__ __attribute__((aligned(16))) float gs[];         // [(K - 1) + Tq][128] GLU outputs, row r = chunk position r - (K - 1)
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; const int col = (blockIdx.x * 32 + tx) * 4; const int b = blockIdx.y;
  const int Hn = K - 1;
  const bool live = col < C; const int cc = live ? col : 0;
  float ww[KMAX][4], bb[4] = {0.f, 0.f, 0.f, 0.f}, sc[4], sh[4];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { if (k < K) ld4<float>(w + (long long)k * C + cc, ww[k]); else ww[k][0] = ww[k][1] = ww[k][2] = ww[k][3] = 0.f; }
  if (bias) ld4<float>(bias + cc, bb);
  ld4<float>(ss + cc, sc); ld4<float>(ss + C + cc, sh);
  T* const sb = state + (long long)b * Hn * 2 * C;
  const T* const ub = u + (long long)b * Tq * 2 * C;
  for (int r = ty; r < Hn + Tq; r += 8) {
    const bool ctx = r < Hn; const bool ok = live && (!ctx || p0 - Hn + r >= 0);
    const T* row = ctx ? sb + (long long)r * 2 * C : ub + (long long)(r - Hn) * 2 * C;
    float a[4], g[4]; ld4<T>(row + cc, a); ld4<T>(row + C + cc, g);
    *(float4*)(gs + r * 128 + tx * 4) = ok ? make_float4(a[0] * sigmoidf_(g[0]), a[1] * sigmoidf_(g[1]), a[2] * sigmoidf_(g[2]), a[3] * sigmoidf_(g[3])) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // new context row r = old row r + n (while that is a context row) or chunk row n - Hn + r: at most two rows per thread, read before the barrier
  float na[2][4], nb[2][4];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = ty + 8 * q;
    if (r < Hn && n > 0) {
      const int src = r + n; const T* row = src < Hn ? sb + (long long)src * 2 * C : ub + (long long)(src - Hn) * 2 * C;
      ld4<T>(row + cc, na[q]); ld4<T>(row + C + cc, nb[q]);
    }
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int r = ty + 8 * q;
    if (r < Hn && n > 0) { st4<T>(sb + (long long)r * 2 * C + col, na[q]); st4<T>(sb + (long long)r * 2 * C + C + col, nb[q]); }
  }
  for (int o = ty; o < To; o += 8) {
    float acc[4] = {bb[0], bb[1], bb[2], bb[3]};
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        const float4 g = *(const float4*)(gs + (o * stride + k) * 128 + tx * 4);
        acc[0] += ww[k][0] * g.x; acc[1] += ww[k][1] * g.y; acc[2] += ww[k][2] * g.z; acc[3] += ww[k][3] * g.w;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = swishf_(acc[e] * sc[e] + sh[e]);
    st4<T>(out + ((long long)b * To + o) * C + col, acc);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void glu_dwconv_stream_kernel(const T* __restrict__ u, const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ ss,
                                                                T* __restrict__ out, T* state, const long long* __restrict__ pos, const unsigned char* __restrict__ reset,
                                                                const long long* __restrict__ clen, int div, int Tq, int C, int K, int stride, int To) {
  const int b = blockIdx.y;
  long long p0 = (reset && reset[b]) ? 0 : pos[b] / div; if (p0 < 0) p0 = 0;
  int n = Tq;
  if (clen) { long long c = (clen[b] + div - 1) / div; n = c < 0 ? 0 : (c > Tq ? Tq : (int)c); }
  glu_dwconv_stream_body<T>(u, w, bias, ss, out, state, p0, n, Tq, C, K, stride, To);
}
// Look-ahead form (nnet.ConformerLookaheadStreamSession): a window of Wq rows per slot, all convolved; only the first c = ncommit / div are final and enter the context
// (the others come back, recomputed, in the next window).
template <typename T>
__global__ __launch_bounds__(256) void glu_dwconv_stream_la_kernel(const T* __restrict__ u, const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ ss,
                                                                   T* __restrict__ out, T* state, const long long* __restrict__ pos, const unsigned char* __restrict__ reset,
                                                                   const long long* __restrict__ ncommit, int div, int Wq, int C, int K, int stride, int To) {
  const int b = blockIdx.y;
  long long p0 = (reset && reset[b]) ? 0 : pos[b] / div; if (p0 < 0) p0 = 0;
  const long long c = ncommit[b] / div;
  glu_dwconv_stream_body<T>(u, w, bias, ss, out, state, p0, c < 0 ? 0 : (c > Wq ? Wq : (int)c), Wq, C, K, stride, To);
}

extern "C" long long avec_glu_dwconv_stream_state_bytes(int dtype, int B, int C, int K) {
  if (B <= 0 || C <= 0 || K <= 0) return 0;
  return (long long)B * (K - 1) * 2 * C * (dtype == AVEC_BF16 ? 2 : 4);
}
extern "C" int avec_glu_dwconv_stream(int dtype, const void* u, const float* w, const float* bias, const float* ss, void* out, void* state, long long state_bytes,
                                      const long long* pos, const unsigned char* reset, const long long* chunk_len, int div, int B, int Tq, int C, int K, int stride, hipStream_t st) {
  AVEC_CHECK_ARG(u && w && ss && out && pos, "glu_dwconv_stream: null pointer (u, w, ss, out and pos are required)");
  AVEC_CHECK_ARG(B > 0 && Tq > 0 && div > 0 && stride > 0 && Tq % stride == 0, "glu_dwconv_stream: bad dims B=%d Tq=%d div=%d stride=%d (Tq must be a multiple of the stride)", B, Tq, div, stride);
  AVEC_CHECK_ARG(C > 0 && C % 4 == 0, "glu_dwconv_stream: C=%d must be a positive multiple of 4 (4-channel vector accesses)", C);
  AVEC_CHECK_ARG(K > 0 && K <= KMAX, "glu_dwconv_stream: kernel size K=%d outside 1..%d", K, KMAX);
  AVEC_CHECK_ARG(K == 1 || state, "glu_dwconv_stream: null state (K=%d needs %d context rows per slot)", K, K - 1);
  AVEC_CHECK_ARG(state_bytes >= avec_glu_dwconv_stream_state_bytes(dtype, B, C, K), "glu_dwconv_stream: state of %lld bytes, %lld needed (avec_glu_dwconv_stream_state_bytes)",
                 state_bytes, avec_glu_dwconv_stream_state_bytes(dtype, B, C, K));
  // 16-byte aligned bases: with C % 4 == 0 every fp32 access is then a whole aligned 16-byte chunk and every bf16 access an aligned 8-byte one (4 channels)
  AVEC_CHECK_ARG(avec_aligned16(u) && avec_aligned16(w) && avec_aligned16(bias) && avec_aligned16(ss) && avec_aligned16(out) && avec_aligned16(state),
                 "glu_dwconv_stream: u, w, bias, ss, out and state must be 16-byte aligned");
  AVEC_CHECK_ARG((((uintptr_t)pos) & 7) == 0 && (((uintptr_t)chunk_len) & 7) == 0, "glu_dwconv_stream: pos and chunk_len must be 8-byte aligned (int64)");
  const size_t lds = (size_t)(K - 1 + Tq) * 128 * sizeof(float);
  AVEC_CHECK_ARG(lds <= 48 * 1024, "glu_dwconv_stream: chunk of %d frames too long (K - 1 + Tq <= 96)", Tq);
  dim3 grid((unsigned)((C / 4 + 31) / 32), (unsigned)B);
  DISPATCH_T(dtype, hipLaunchKernelGGL(glu_dwconv_stream_kernel<T>, grid, dim3(256), lds, st, (const T*)u, w, bias, ss, (T*)out, (T*)state, pos, reset, chunk_len, div, Tq, C, K, stride, Tq / stride));
  AVEC_LAUNCH_CHECK();
  return 0;
}
extern "C" int avec_glu_dwconv_stream_la(int dtype, const void* u, const float* w, const float* bias, const float* ss, void* out, void* state, long long state_bytes,
                                         const long long* pos, const unsigned char* reset, const long long* ncommit, int div, int B, int Wq, int C, int K, int stride, hipStream_t st) {
  AVEC_CHECK_ARG(u && w && ss && out && pos && ncommit, "glu_dwconv_stream_la: null pointer (u, w, ss, out, pos and ncommit are required)");
  AVEC_CHECK_ARG(B > 0 && Wq > 0 && div > 0 && stride > 0 && Wq % stride == 0, "glu_dwconv_stream_la: bad dims B=%d Wq=%d div=%d stride=%d (Wq must be a multiple of the stride)", B, Wq, div, stride);
  AVEC_CHECK_ARG(C > 0 && C % 4 == 0, "glu_dwconv_stream_la: C=%d must be a positive multiple of 4 (4-channel vector accesses)", C);
  AVEC_CHECK_ARG(K > 0 && K <= KMAX, "glu_dwconv_stream_la: kernel size K=%d outside 1..%d", K, KMAX);
  AVEC_CHECK_ARG(K == 1 || state, "glu_dwconv_stream_la: null state (K=%d needs %d context rows per slot)", K, K - 1);
  AVEC_CHECK_ARG(state_bytes >= avec_glu_dwconv_stream_state_bytes(dtype, B, C, K), "glu_dwconv_stream_la: state of %lld bytes, %lld needed (avec_glu_dwconv_stream_state_bytes)",
                 state_bytes, avec_glu_dwconv_stream_state_bytes(dtype, B, C, K));
  AVEC_CHECK_ARG(avec_aligned16(u) && avec_aligned16(w) && avec_aligned16(bias) && avec_aligned16(ss) && avec_aligned16(out) && avec_aligned16(state),
                 "glu_dwconv_stream_la: u, w, bias, ss, out and state must be 16-byte aligned");
  AVEC_CHECK_ARG((((uintptr_t)pos) & 7) == 0 && (((uintptr_t)ncommit) & 7) == 0, "glu_dwconv_stream_la: pos and ncommit must be 8-byte aligned (int64)");
  const size_t lds = (size_t)(K - 1 + Wq) * 128 * sizeof(float);
  AVEC_CHECK_ARG(lds <= 48 * 1024, "glu_dwconv_stream_la: window of %d frames too long (K - 1 + Wq <= 96)", Wq);
  dim3 grid((unsigned)((C / 4 + 31) / 32), (unsigned)B);
  DISPATCH_T(dtype, hipLaunchKernelGGL(glu_dwconv_stream_la_kernel<T>, grid, dim3(256), lds, st, (const T*)u, w, bias, ss, (T*)out, (T*)state, pos, reset, ncommit, div, Wq, C, K, stride, Wq / stride));
  AVEC_LAUNCH_CHECK();
  return 0;
}
// end of a push: pos[b] = (reset[b] ? 0 : pos[b]) + min(chunk_len[b], full)   (chunk_len NULL: full), then reset[b] = 0: the flags are consumed, the caller sets only
// those of the next push (no clearing copy or memset after a restart).  One launch per push whether or not a slot restarts; the last reader of pos / reset in the push.
__global__ void stream_advance_kernel(long long* pos, unsigned char* reset, const long long* clen, long long full, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  long long c = clen ? clen[b] : full; c = c < 0 ? 0 : (c > full ? full : c);
  pos[b] = ((reset && reset[b]) ? 0 : pos[b]) + c;
  if (reset) reset[b] = 0;
}
extern "C" int avec_stream_advance(long long* pos, unsigned char* reset, const long long* chunk_len, long long full, int B, hipStream_t st) {
  AVEC_CHECK_ARG(pos && B > 0 && full > 0 && (((uintptr_t)pos) & 7) == 0 && (((uintptr_t)chunk_len) & 7) == 0, "stream_advance: bad arguments (B=%d full=%lld)", B, full);
  hipLaunchKernelGGL(stream_advance_kernel, dim3((B + 63) / 64), dim3(64), 0, st, pos, reset, chunk_len, full, B);
  AVEC_LAUNCH_CHECK();
  return 0;
}

// ================================================================================================================================================================
// Window control of the look-ahead session (nnet.ConformerLookaheadStreamSession): two launches around a push.  Per slot the session carries a tail of pend <= LAe
// input frames that were heard and are not final yet, pos (committed input frames) and an `ended` flag.
//   avec_stream_window, the first launch: the window X [B][W = Tc + LAe][D] = [tail[:pend] | x_new[:n_new] | zeros], n = pend + n_new valid frames, and what the
//     stack's kernels read:  nvalid = n;  ncommit = c = max(0, n - LAe) rounded down to a multiple of S for a running slot, 0 for a slot that ends (`last`: nothing after
//     this push reads its state);  emit = c for a running slot, n for one that ends.  A restarted slot has pend = 0 and is not ended; an ended slot takes no frame.
//   avec_stream_window_advance, the last launch: tail <- X[c : n] (from X, never in place), pend = n - c (0 for a slot that ends), pos = (reset ? 0 : pos) + c,
//     ended = (reset ? 0 : ended) | last, and the reset / last flags are cleared (consumed, as avec_stream_advance does).  The copying workgroups read nvalid / ncommit
//     only, which this launch does not write; one thread per slot owns the counters and flags.
// grid (rows, B), one workgroup per row.
// ================================================================================================================================================================
__global__ __launch_bounds__(256) void stream_window_kernel(const float* __restrict__ x_new, const float* __restrict__ tail, float* __restrict__ X, const long long* __restrict__ pend,
                                                            const long long* __restrict__ n_new, const unsigned char* __restrict__ last, const unsigned char* __restrict__ reset,
                                                            const unsigned char* __restrict__ ended, long long* __restrict__ nvalid, long long* __restrict__ ncommit,
                                                            long long* __restrict__ emit, int Tc, int LAe, int D, int S) {
  const int r = blockIdx.x, b = blockIdx.y;
  const bool rs = reset && reset[b];
  long long pe = rs ? 0 : pend[b]; pe = pe < 0 ? 0 : (pe > LAe ? LAe : pe);
  long long nn = n_new ? n_new[b] : Tc; nn = nn < 0 ? 0 : (nn > Tc ? Tc : nn);
  if (!rs && ended[b]) { pe = 0; nn = 0; }
  const long long n = pe + nn;
  const float* src = r < pe ? tail + ((long long)b * LAe + r) * D : (r < n ? x_new + ((long long)b * Tc + (r - pe)) * D : nullptr);
  float* dst = X + ((long long)b * (Tc + LAe) + r) * D;
  for (int c = threadIdx.x; c < D; c += 256) dst[c] = src ? src[c] : 0.f;
  if (r == 0 && threadIdx.x == 0) {
    const bool ends = last && last[b];
    long long c = n - LAe; c = c < 0 ? 0 : c - c % S;
    nvalid[b] = n; ncommit[b] = ends ? 0 : c; emit[b] = ends ? n : c;
  }
}
extern "C" int avec_stream_window(const float* x_new, const float* tail, float* X, const long long* pend, const long long* n_new, const unsigned char* last, const unsigned char* reset,
                                  const unsigned char* ended, long long* nvalid, long long* ncommit, long long* emit, int B, int Tc, int LAe, int D, int S, hipStream_t st) {
  AVEC_CHECK_ARG(x_new && X && pend && ended && nvalid && ncommit && emit && (tail || LAe == 0),
                 "stream_window: null pointer (x_new, tail, X, pend, ended, nvalid, ncommit and emit are required)");
  AVEC_CHECK_ARG(B > 0 && Tc > 0 && LAe >= 0 && D > 0 && S > 0 && Tc % S == 0 && LAe % S == 0, "stream_window: bad dims B=%d Tc=%d LAe=%d D=%d S=%d (Tc and LAe must be multiples of S)", B, Tc, LAe, D, S);
  AVEC_CHECK_ARG(!(((uintptr_t)x_new | (uintptr_t)tail | (uintptr_t)X) & 3) && !(((uintptr_t)pend | (uintptr_t)n_new | (uintptr_t)nvalid | (uintptr_t)ncommit | (uintptr_t)emit) & 7),
                 "stream_window: misaligned pointer (x_new / tail / X: 4 bytes, the int64 vectors: 8 bytes)");
  AVEC_CHECK_ARG(X != x_new && X != tail, "stream_window: X must be a buffer of its own");
  hipLaunchKernelGGL(stream_window_kernel, dim3((unsigned)(Tc + LAe), (unsigned)B), dim3(256), 0, st, x_new, tail, X, pend, n_new, last, reset, ended, nvalid, ncommit, emit, Tc, LAe, D, S);
  AVEC_LAUNCH_CHECK();
  return 0;
}
__global__ __launch_bounds__(256) void stream_window_advance_kernel(const float* __restrict__ X, float* __restrict__ tail, long long* pend, long long* pos, const long long* __restrict__ nvalid,
                                                                    const long long* __restrict__ ncommit, unsigned char* last, unsigned char* reset, unsigned char* ended,
                                                                    int W, int LAe, int D) {
  const int r = blockIdx.x, b = blockIdx.y;
  long long n = nvalid[b], c = ncommit[b];
  n = n < 0 ? 0 : (n > W ? W : n); c = c < 0 ? 0 : (c > n ? n : c);
  if (r < LAe && c + r < n) {
    const float* src = X + ((long long)b * W + c + r) * D; float* dst = tail + ((long long)b * LAe + r) * D;
    for (int ch = threadIdx.x; ch < D; ch += 256) dst[ch] = src[ch];
  }
  if (r == 0 && threadIdx.x == 0) {
    const bool rs = reset && reset[b], ends = last && last[b];
    long long left = n - c; left = left > LAe ? LAe : left;
    pend[b] = ends ? 0 : left;
    pos[b] = (rs ? 0 : pos[b]) + c;
    ended[b] = ((rs ? 0 : ended[b]) || ends) ? 1 : 0;
    if (reset) reset[b] = 0;
    if (last) last[b] = 0;
  }
}
extern "C" int avec_stream_window_advance(const float* X, float* tail, long long* pend, long long* pos, const long long* nvalid, const long long* ncommit, unsigned char* last,
                                          unsigned char* reset, unsigned char* ended, int B, int W, int LAe, int D, hipStream_t st) {
  AVEC_CHECK_ARG(X && pend && pos && nvalid && ncommit && ended && (tail || LAe == 0), "stream_window_advance: null pointer (X, tail, pend, pos, nvalid, ncommit and ended are required)");
  AVEC_CHECK_ARG(B > 0 && LAe >= 0 && W > LAe && D > 0, "stream_window_advance: bad dims B=%d W=%d LAe=%d D=%d (W = Tc + LAe)", B, W, LAe, D);
  AVEC_CHECK_ARG(!(((uintptr_t)X | (uintptr_t)tail) & 3) && !(((uintptr_t)pend | (uintptr_t)pos | (uintptr_t)nvalid | (uintptr_t)ncommit) & 7),
                 "stream_window_advance: misaligned pointer (X / tail: 4 bytes, the int64 vectors: 8 bytes)");
  AVEC_CHECK_ARG((const float*)tail != X, "stream_window_advance: the tail must be a buffer of its own (it is read from X, not in place)");
  hipLaunchKernelGGL(stream_window_advance_kernel, dim3((unsigned)(LAe > 0 ? LAe : 1), (unsigned)B), dim3(256), 0, st, X, tail, pend, pos, nvalid, ncommit, last, reset, ended, W, LAe, D);
  AVEC_LAUNCH_CHECK();
  return 0;
}
