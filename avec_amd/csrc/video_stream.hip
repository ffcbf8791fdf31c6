// Streamed visual stem (nnet.VisualFrontStreamSession): video chunks -> the pooled NHWC frames ResNet.forward_nhwc consumes, with the offline stem's arithmetic.
//   Conv3d(1 -> 64, (5,7,7), stride (1,2,2), zero pad (2,3,3), bias) + eval-mode BatchNorm3d + ReLU + max pool 3x3 / s2 / p1 per frame.  Output frame t reads input
//   frames t-2 .. t+2: with n frames heard E(n) = max(0, n - 2) output frames exist, n once the utterance has ended.  The only coupling in time is that window, so the
//   carried state per slot is the last 4 input frames (a ring indexed by frame & 3: nothing is ever shifted), a frame counter and an `ended` flag.  The ring holds
//   frames in the format the conv loop consumes (bf16 / fp32): a carried frame is bit-identical to a fresh one, and an output frame depends on the VALUES of its five
//   input frames alone -- every output element is one fixed-order reduction in one workgroup, no atomics -- whatever push produces it.
//   Per push: avec_video_stem_stream (reads the state only; many workgroups per slot read the ring) -> avec_video_stream_advance (the launch that overwrites it).
// Workgroup = (band of pn pooled rows, local output frame r, slot b).  It stages the 5 x SH input rows of its band in LDS as rows of [8 zero px | W px | 8 zero px]
// (the layout of stem3p.hip: the 8 operand elements of output pixel ow, slot 0 = zero weight, slots 1..7 = kw 0..6, are the 8 consecutive staged pixels 2 ow - 4 ..
// 2 ow + 3), every 8-pixel chunk SOURCED from the ring, the chunk or nowhere (zeros) -- never multiplied by zero.  Reduction order k = (kd, kh, slot).  The band's
// conv rows go through bias, scale | shift and ReLU into a channel-major LDS tile in the activation dtype (rounding is monotone: it commutes with the max), then the
// pool stage (thread = channel) reads its 3x3 windows and writes NHWC.  bf16: MFMA 32x32x16, fp32 accumulation; fp32 (parity path): VALU FMAs from the same slab.
#include <type_traits>
#include "vec.h"
#include "avec_hip.h"
#include "wave_prims.h"

static constexpr int VS_C = 64;

struct VsGeom {
  int H, W, OH, OW, PH, PW;
  int NB, pn;              // bands per frame, pooled rows per band
  int SH;                  // staged input rows per frame of the window: 2 * (2 * pn) + 7
  int CPR, PP;             // 8-pixel chunks per staged row (W / 8 + 2), staged pixels per row
  int CS;                  // channel stride of the conv tile, in elements: an odd number of 32-bit words (the pool stage's 64 channels hit 64 banks)
  size_t slab_bytes, lds_bytes;
};

// state blob: [B][4][H][W] T ring | [B] int64 n (frames since the restart) | [B] int64 ended
struct VsState { char* ring; long long* n; long long* ended; };
static __host__ __device__ __forceinline__ VsState vs_state(void* base, int B, int H, int W, size_t esz) {
  VsState s; s.ring = (char*)base; s.n = (long long*)((char*)base + (size_t)B * 4 * H * W * esz); s.ended = s.n + B; return s;
}
struct VsSlot { long long n0, c, E0, E1; bool last, ended; };
// what a push does to slot b, from the state BEFORE the push and the push's controls; both launches of the push derive the same numbers
__device__ __forceinline__ VsSlot vs_slot(const VsState& st, const long long* n_frames, const unsigned char* reset, const unsigned char* last, int b, int Tin) {
  VsSlot s; const bool rs = reset && reset[b];
  s.n0 = rs ? 0 : st.n[b]; if (s.n0 < 0) s.n0 = 0;
  s.ended = !rs && st.ended[b] != 0;
  long long c = n_frames ? n_frames[b] : Tin; c = c < 0 ? 0 : (c > Tin ? Tin : c);
  s.c = s.ended ? 0 : c;
  s.last = !s.ended && last && last[b];
  s.E0 = s.n0 > 2 ? s.n0 - 2 : 0;
  const long long n1 = s.n0 + s.c;
  s.E1 = s.ended ? s.E0 : (s.last ? n1 : (n1 > 2 ? n1 - 2 : 0));
  if (s.E1 < s.E0) s.E1 = s.E0;
  return s;
}

// four consecutive pixels of one channel into the conv tile (p is a multiple of 4, CS is even for bf16: 4-byte aligned)
__device__ __forceinline__ void vs_put4(bf16* p, float v0, float v1, float v2, float v3) { ((uint32_t*)p)[0] = f32x2_to_bf16x2(v0, v1); ((uint32_t*)p)[1] = f32x2_to_bf16x2(v2, v3); }
__device__ __forceinline__ void vs_put4(float* p, float v0, float v1, float v2, float v3) { p[0] = v0; p[1] = v1; p[2] = v2; p[3] = v3; }
__device__ __forceinline__ float vs_act(float acc, float bias, float sc, float sh) { const float y = (acc + bias) * sc + sh; return y > 0.f ? y : 0.f; }

template <typename T>
__global__ __launch_bounds__(256, 2) void video_stem_stream_kernel(const float* __restrict__ chunk, long long ldc, VsState st, const long long* __restrict__ n_frames,
                                                                   const unsigned char* __restrict__ reset, const unsigned char* __restrict__ last, const T* __restrict__ w8,
                                                                   const float* __restrict__ bias, const float* __restrict__ ss, T* __restrict__ out,
                                                                   long long* __restrict__ out_len, int B, int Tin, int Tmax, VsGeom G) {
  extern __shared__ __attribute__((aligned(16))) char vs_lds[];
  T* const slab = (T*)vs_lds;                                       // [5][SH][PP]
  T* const tile = (T*)(vs_lds + G.slab_bytes);                      // [64][CS]: relu(bn(conv)) of the band's conv rows, pixel p = local conv row * OW + ow
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int band = blockIdx.x, r = blockIdx.y, b = blockIdx.z;
  VsSlot s = vs_slot(st, n_frames, reset, last, b, Tin);
  if (s.E1 > s.E0 + Tmax) s.E1 = s.E0 + Tmax;                       // (a count the caller should not have passed: frames are missing, no access out of range)
  if (band == 0 && r == 0 && tid == 0) out_len[b] = s.E1 - s.E0;
  const int ph0 = band * G.pn, pnb = min(G.pn, G.PH - ph0);
  T* const obase = out + (((long long)r * B + b) * G.PH + ph0) * (long long)G.PW * VS_C;      // frame-major: [Tmax][B][PH][PW][64]
  if (r >= s.E1 - s.E0) {                                           // (uniform over the workgroup) rows at or past out_len: zeros
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int q = tid; q < pnb * G.PW * (VS_C / 8); q += 256) st8<T>(obase + q * 8, z);
    return;
  }
  const long long t = s.E0 + r;                                     // the output frame
  const int cr0 = max(0, 2 * ph0 - 1), cr1 = min(G.OH - 1, 2 * (ph0 + pnb - 1) + 1);
  const int npx = (cr1 - cr0 + 1) * G.OW, ir0 = 2 * cr0 - 3;
  const long long HW = (long long)G.H * G.W;
  const T* const ringb = (const T*)st.ring + (long long)b * 4 * HW;
  const float* const chb = chunk + (long long)b * ldc;
  // ---- stage: chunk q = 8 pixels of staged row (kd, rr); frame f = t + kd - 2 comes from the ring (n0 - 4 <= f < n0: f >= t - 2 >= n0 - 4 always), from the chunk
  // (n0 <= f < n0 + c) or from nowhere (f < 0; f >= n0 + c, which a valid output frame reaches only in an utterance's last push: the offline paddings)
  for (int q = tid; q < 5 * G.SH * G.CPR; q += 256) {
    const int row = q / G.CPR, j = q - row * G.CPR;
    const int kd = row / G.SH, rr = row - kd * G.SH;
    const long long f = t + kd - 2; const int ih = ir0 + rr;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (j >= 1 && j <= G.CPR - 2 && ih >= 0 && ih < G.H && f >= 0) {
      const long long off = (long long)ih * G.W + (j - 1) * 8;
      if (f < s.n0) ld8<T>(ringb + (f & 3) * HW + off, v);
      else if (f < s.n0 + s.c) ld8<float>(chb + (f - s.n0) * HW + off, v);
    }
    st8<T>(slab + (long long)row * G.PP + 8 * j, v);
  }
  __syncthreads();
  // ---- conv + bias, scale | shift, ReLU -> tile
  if constexpr (std::is_same<T, bf16>::value) {
    // wave = 32 pixels x 64 channels per tile of 128 pixels, K = 36 rows (kd, kh) of 8 slots (row 35 and slot 0 carry zero weights).  acc[j][q]: channel
    // 32 j + (lane & 31), pixel (q & 3) + 8 (q >> 2) + 4 (lane >> 5) of the wave's 32
    const int g = lane >> 5, pl = lane & 31;
    chunk16 wf[18][2];
#pragma unroll
    for (int k = 0; k < 18; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j) wf[k][j] = ldg16(w8 + (long long)(32 * j + pl) * 288 + (2 * k + g) * 8);
    const int pitch = G.PP * 2;
    int rowoff[35];
#pragma unroll
    for (int k = 0; k < 35; ++k) rowoff[k] = ((k / 7) * G.SH + (k % 7)) * pitch;
    const float b0 = bias ? bias[pl] : 0.f, b1 = bias ? bias[32 + pl] : 0.f;
    const float sc0 = ss[pl], sc1 = ss[32 + pl], sh0 = ss[VS_C + pl], sh1 = ss[VS_C + 32 + pl];
    for (int t0 = 0; t0 < npx; t0 += 128) {
      const int p = t0 + 32 * wave + pl; const int pc = p < npx ? p : 0;
      const int ohl = pc / G.OW, ow = pc - ohl * G.OW;
      const char* pix = (const char*)slab + (2 * ohl) * pitch + 4 * ow + 8;
      f32x16 acc[2];
#pragma unroll
      for (int q = 0; q < 16; ++q) { acc[0][q] = 0.f; acc[1][q] = 0.f; }
#pragma unroll
      for (int k = 0; k < 18; ++k) {
        const int offA = rowoff[2 * k > 34 ? 34 : 2 * k], offB = rowoff[2 * k + 1 > 34 ? 34 : 2 * k + 1];
        const uint32_t* rp = (const uint32_t*)(pix + (g ? offB : offA));
        chunk16 fa; fa.w[0] = rp[0]; fa.w[1] = rp[1]; fa.w[2] = rp[2]; fa.w[3] = rp[3];
        acc[0] = mma16(fa, wf[k][0], acc[0]);
        acc[1] = mma16(fa, wf[k][1], acc[1]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float bb = j ? b1 : b0, sc = j ? sc1 : sc0, sh = j ? sh1 : sh0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {                               // register quad a = pixels 8 a + 4 g .. + 3 of the wave's 32 (npx is a multiple of 4)
          const int pr = t0 + 32 * wave + 8 * a + 4 * g;
          if (pr < npx)
            vs_put4(tile + (32 * j + pl) * G.CS + pr, vs_act(acc[j][4 * a], bb, sc, sh), vs_act(acc[j][4 * a + 1], bb, sc, sh), vs_act(acc[j][4 * a + 2], bb, sc, sh),
                    vs_act(acc[j][4 * a + 3], bb, sc, sh));
        }
      }
    }
  } else {
    // parity path: lane = channel, a wave takes 8 pixels at a time; the 8 staged pixels of a (pixel, row) are a broadcast LDS read
    const int c = lane;
    const float bb = bias ? bias[c] : 0.f, sc = ss[c], sh = ss[VS_C + c];
    const float* wc = (const float*)w8 + (long long)c * 288;
    for (int p0 = 8 * wave; p0 < npx; p0 += 32) {
      int poff[8]; float acc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int p = min(p0 + i, npx - 1); const int ohl = p / G.OW, ow = p - ohl * G.OW;
        poff[i] = 2 * ohl * G.PP + 2 * ow + 4; acc[i] = 0.f;
      }
#pragma unroll 1
      for (int k = 0; k < 35; ++k) {
        const int base = ((k / 7) * G.SH + (k % 7)) * G.PP;
        const float4 wa = *(const float4*)(wc + k * 8), wb = *(const float4*)(wc + k * 8 + 4);
        const float wv[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float2* px = (const float2*)((const float*)slab + base + poff[i]);
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float2 x = px[e]; acc[i] = fmaf(wv[2 * e], x.x, acc[i]); acc[i] = fmaf(wv[2 * e + 1], x.y, acc[i]); }
        }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) if (p0 + i < npx) ((float*)tile)[c * G.CS + p0 + i] = vs_act(acc[i], bb, sc, sh);
    }
  }
  __syncthreads();
  // ---- pool: thread = channel x every fourth pooled pixel of the band.  The tile holds values >= +0 and every window holds a valid pixel: 0 is the identity of this
  // max, columns and rows outside the conv output are skipped (the pool's padding never wins)
  {
    const int c = tid & 63, qg = tid >> 6;
    const T* tc = tile + c * G.CS;
    for (int i = qg; i < pnb * G.PW; i += 4) {
      const int phl = i / G.PW, pw = i - phl * G.PW;
      float best = 0.f;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int cr = 2 * (ph0 + phl) + kh - 1;
        if (cr < 0 || cr >= G.OH) continue;
        const T* rowp = tc + (cr - cr0) * G.OW;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int cc = 2 * pw + kw - 1;
          if (cc >= 0 && cc < G.OW) best = fmaxf(best, ldf<T>(rowp + cc));
        }
      }
      stf<T>(obase + (long long)i * VS_C + c, best);
    }
  }
}

// workgroup = one slot: the chunk's last min(c, 4) frames into their ring slots (the format the conv loop consumes), then the counters; every thread has read the
// controls and the counter before thread 0 overwrites them
template <typename T>
__global__ __launch_bounds__(256) void video_stream_advance_kernel(const float* __restrict__ chunk, long long ldc, VsState st, const long long* __restrict__ n_frames,
                                                                   unsigned char* reset, unsigned char* last, int Tin, int H, int W) {
  const int b = blockIdx.x;
  const VsSlot s = vs_slot(st, n_frames, reset, last, b, Tin);
  __syncthreads();
  const long long HW = (long long)H * W; const int HW8 = (int)(HW >> 3);
  const int keep = (int)(s.c < 4 ? s.c : 4);
  T* const ringb = (T*)st.ring + (long long)b * 4 * HW;
  const float* const chb = chunk + (long long)b * ldc;
  for (int q = threadIdx.x; q < keep * HW8; q += 256) {
    const int kk = q / HW8; const long long o = (long long)(q - kk * HW8) * 8;
    const long long i = s.c - 1 - kk, f = s.n0 + i;
    float v[8]; ld8<float>(chb + i * HW + o, v);
    st8<T>(ringb + (f & 3) * HW + o, v);
  }
  if (threadIdx.x == 0) {
    st.n[b] = s.n0 + s.c; st.ended[b] = (s.ended || s.last) ? 1 : 0;
    if (reset) reset[b] = 0;
    if (last) last[b] = 0;
  }
}

// ------------------------------------------------------------------------------------------------
static bool vs_geom(VsGeom& G, int dtype, int H, int W) {
  if (H < 8 || W < 32 || (W & 7) || H > 4096 || W > 4096) return false;
  const size_t esz = dtype == AVEC_BF16 ? 2 : 4;
  G.H = H; G.W = W; G.OH = (H - 1) / 2 + 1; G.OW = (W - 1) / 2 + 1; G.PH = (G.OH - 1) / 2 + 1; G.PW = (G.OW - 1) / 2 + 1;
  G.CPR = W / 8 + 2; G.PP = G.CPR * 8;
  for (int nb = 1; nb <= G.PH; ++nb) {                              // fewest bands whose workgroup fits twice into a CU's LDS; one pooled row per band may take all of it
    G.NB = nb; G.pn = (G.PH + nb - 1) / nb;
    if ((G.NB - 1) * G.pn >= G.PH) continue;                        // (an empty last band)
    G.SH = 2 * (2 * G.pn) + 7;
    const int npx = (2 * G.pn + 1) * G.OW;                          // a multiple of 4
    G.CS = dtype == AVEC_BF16 ? npx + 2 : npx + 1;
    G.slab_bytes = (size_t)5 * G.SH * G.PP * esz;                   // a multiple of 16
    G.lds_bytes = G.slab_bytes + (size_t)VS_C * G.CS * esz;
    if (G.lds_bytes <= 80 * 1024) return true;
  }
  return G.lds_bytes <= 160 * 1024;
}

extern "C" long long avec_video_stream_state_bytes(int dtype, int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (W & 7) || (dtype != AVEC_BF16 && dtype != AVEC_F32)) return 0;
  return (long long)B * (4ll * H * W * (dtype == AVEC_BF16 ? 2 : 4) + 16);
}

static int vs_check(const char* who, int dtype, const void* chunk, long long ldc, const void* state, long long state_bytes, const void* n_frames, int B, int Tin, int H, int W, VsGeom& G) {
  AVEC_CHECK_ARG(chunk && state, "%s: null pointer (chunk and state are required)", who);
  AVEC_CHECK_ARG(dtype == AVEC_BF16 || dtype == AVEC_F32, "%s: dtype %d", who, dtype);
  AVEC_CHECK_ARG(B > 0 && B < 65536 && Tin > 0 && H > 0 && W > 0, "%s: bad dims B=%d Tin=%d H=%d W=%d", who, B, Tin, H, W);
  AVEC_CHECK_ARG(vs_geom(G, dtype, H, W), "%s: frame %dx%d not supported (W %% 8 == 0, W >= 32, H >= 8: rows are staged as whole 8-pixel chunks)", who, H, W);
  AVEC_CHECK_ARG(ldc >= (long long)Tin * H * W && (ldc & 3) == 0, "%s: slot stride %lld of chunk [B][Tin=%d][%d][%d] (at least Tin H W, a multiple of 4 floats)", who, ldc, Tin, H, W);
  AVEC_CHECK_ARG(state_bytes >= avec_video_stream_state_bytes(dtype, B, H, W), "%s: state of %lld bytes, %lld needed (avec_video_stream_state_bytes)", who, state_bytes,
                 avec_video_stream_state_bytes(dtype, B, H, W));
  AVEC_CHECK_ARG(avec_aligned16(state) && avec_aligned16(chunk) && (((uintptr_t)n_frames) & 7) == 0, "%s: state and chunk must be 16-byte aligned, n_frames 8-byte aligned (int64)", who);
  return 0;
}

extern "C" int avec_video_stem_stream(int dtype, const float* chunk, long long ldc, const void* state, long long state_bytes, const long long* n_frames,
                                      const unsigned char* reset, const unsigned char* last, const void* w8, const float* bias, const float* ss, void* out,
                                      long long* out_len, int B, int Tin, int Tmax, int H, int W, hipStream_t st) {
  VsGeom G;
  if (int r = vs_check("video_stem_stream", dtype, chunk, ldc, state, state_bytes, n_frames, B, Tin, H, W, G)) return r;
  AVEC_CHECK_ARG(w8 && ss && out && out_len, "video_stem_stream: null pointer (w8, ss, out and out_len are required)");
  AVEC_CHECK_ARG(Tmax >= 1 && Tmax < 65536, "video_stem_stream: bad Tmax=%d", Tmax);
  AVEC_CHECK_ARG(avec_aligned16(w8) && avec_aligned16(out) && (((uintptr_t)out_len) & 7) == 0, "video_stem_stream: w8 and out must be 16-byte aligned, out_len 8-byte aligned (int64)");
  const VsState S = vs_state((void*)state, B, H, W, dtype == AVEC_BF16 ? 2 : 4);
  const dim3 grid((unsigned)G.NB, (unsigned)Tmax, (unsigned)B);
  if (dtype == AVEC_BF16) {
    if (int r = avec_lds_optin(video_stem_stream_kernel<bf16>, G.lds_bytes)) return r;
    avec_note_kernel("video_stem_stream_kernel<bf16>");
    hipLaunchKernelGGL(video_stem_stream_kernel<bf16>, grid, dim3(256), G.lds_bytes, st, chunk, ldc, S, n_frames, reset, last, (const bf16*)w8, bias, ss, (bf16*)out, out_len, B, Tin, Tmax, G);
  } else {
    if (int r = avec_lds_optin(video_stem_stream_kernel<float>, G.lds_bytes)) return r;
    avec_note_kernel("video_stem_stream_kernel<float>");
    hipLaunchKernelGGL(video_stem_stream_kernel<float>, grid, dim3(256), G.lds_bytes, st, chunk, ldc, S, n_frames, reset, last, (const float*)w8, bias, ss, (float*)out, out_len, B, Tin, Tmax, G);
  }
  AVEC_LAUNCH_CHECK(); return 0;
}

extern "C" int avec_video_stream_advance(int dtype, const float* chunk, long long ldc, void* state, long long state_bytes, const long long* n_frames, unsigned char* reset,
                                         unsigned char* last, int B, int Tin, int H, int W, hipStream_t st) {
  VsGeom G;
  if (int r = vs_check("video_stream_advance", dtype, chunk, ldc, state, state_bytes, n_frames, B, Tin, H, W, G)) return r;
  const VsState S = vs_state(state, B, H, W, dtype == AVEC_BF16 ? 2 : 4);
  DISPATCH_T(dtype, hipLaunchKernelGGL(video_stream_advance_kernel<T>, dim3((unsigned)B), dim3(256), 0, st, chunk, ldc, S, n_frames, reset, last, Tin, H, W));
  AVEC_LAUNCH_CHECK(); return 0;
}
