// Streamed audio front-end (nnet.AudioFrontStreamSession): waveform chunks -> the stem's (B, T', C*F') rows, with the offline path's arithmetic.
//   mel frame f reads samples [hop f - win/2, hop f + win/2) (reflected at both ends of the utterance), stem frame t reads mel frames 2t-1, 2t, 2t+1, so with n samples
//   heard E(n) = n < hop + win/2 ? 0 : (n - hop - win/2) / (2 hop) + 1 stem frames are computable before the end, and Ta / (2 hop) + 1 once the utterance ended at Ta.
//   The only carried state is the sample tail [max(0, 2 hop E(n) - hop - win/2), n): fewer than 2 (hop + win/2) samples (720 for 160 / 400).  No mel column is carried:
//   mel frame 2E - 1 is framed again from the tail.  Per push: avec_mel_frames_stream (windowed frames of mel frames 2 E0 - 1 .. 2 E1 - 1 from [tail | new samples])
//   -> the offline DFT GEMM and avec_mel_power_log on the B * Fmax rows -> avec_audio_stem_stream (conv + eval BatchNorm + Swish) -> avec_audio_stream_advance
//   (shifts the tail, advances the counters, consumes the flags).  The framing launch only READS the state: many workgroups per slot read the tail, the advance is the
//   launch that overwrites it.
#include "vec.h"
#include "avec_hip.h"

static constexpr int AF_CAP = 768;       // tail floats per slot (>= 2 (hop + win/2))

// state blob: [B][AF_CAP] fp32 tails | [B] int64 n (samples since the restart) | [B] int64 ended
struct AfState { float* tail; long long* n; long long* ended; };
static __host__ __device__ __forceinline__ AfState af_state(void* base, int B) {
  AfState s; s.tail = (float*)base; s.n = (long long*)((char*)base + (size_t)B * AF_CAP * sizeof(float)); s.ended = s.n + B; return s;
}
struct AfSlot { long long n0, c0, len0, ns, n1, E0, E1; bool last, ended; };
__device__ __forceinline__ long long af_ready(long long n, int win, int hop) { const long long a = hop + win / 2; return n < a ? 0 : (n - a) / (2 * hop) + 1; }
__device__ __forceinline__ long long af_first(long long E, int win, int hop) { const long long c = 2ll * hop * E - hop - win / 2; return c < 0 ? 0 : c; }
// what a push does to slot b, from the state BEFORE the push and the push's controls; every launch of the push derives the same numbers
__device__ __forceinline__ AfSlot af_slot(const AfState& st, const long long* n_samples, const unsigned char* reset, const unsigned char* last, int b, int W, int win, int hop) {
  AfSlot s; const bool rs = reset && reset[b];
  s.n0 = rs ? 0 : st.n[b]; if (s.n0 < 0) s.n0 = 0;
  s.ended = !rs && st.ended[b] != 0;
  long long ns = n_samples ? n_samples[b] : W; ns = ns < 0 ? 0 : (ns > W ? W : ns);
  s.ns = s.ended ? 0 : ns; s.n1 = s.n0 + s.ns;
  s.last = !s.ended && last && last[b];
  s.E0 = af_ready(s.n0, win, hop); s.c0 = af_first(s.E0, win, hop);
  s.len0 = s.n0 - s.c0; if (s.len0 > AF_CAP) s.len0 = AF_CAP;
  s.E1 = s.ended ? s.E0 : (s.last ? s.n1 / (2 * hop) + 1 : af_ready(s.n1, win, hop));
  return s;
}

// workgroup = one row (slot b, local mel column j = mel frame 2 E0 - 1 + j) of frames [B][Fmax][win]; rows the push does not produce are written as zeros
__global__ __launch_bounds__(256) void mel_frames_stream_kernel(const float* __restrict__ wave, long long ldw, const float* __restrict__ window, float* __restrict__ frames,
                                                                AfState st, const long long* __restrict__ n_samples, const unsigned char* __restrict__ reset,
                                                                const unsigned char* __restrict__ last, long long* __restrict__ out_len, long long* __restrict__ meta,
                                                                int W, int Tmax, int win, int hop) {
  const int Fmax = 2 * Tmax + 1;
  const int b = blockIdx.x / Fmax, j = blockIdx.x - b * Fmax;
  AfSlot s = af_slot(st, n_samples, reset, last, b, W, win, hop);
  if (s.E1 > s.E0 + Tmax) s.E1 = s.E0 + Tmax;                          // (a count the caller should not have passed: wrong frames, no access out of range)
  const long long m = 2 * s.E0 - 1 + j, Fv = s.last ? s.n1 / hop + 1 : 2 * s.E1;
  if (j == 0 && threadIdx.x == 0) { out_len[b] = s.E1 - s.E0; meta[2 * b] = 2 * s.E0 - 1; meta[2 * b + 1] = Fv; }
  const bool live = s.E1 > s.E0 && j <= 2 * (s.E1 - s.E0) && m >= 0 && m < Fv;
  float* row = frames + (long long)blockIdx.x * win;
  const float* tail = st.tail + (long long)b * AF_CAP; const float* wv = wave + (long long)b * ldw;
  for (int n = threadIdx.x; n < win; n += 256) {
    float v = 0.f;
    if (live) {
      long long p = m * hop + n - win / 2;
      if (p < 0) p = -p; else if (p >= s.n1) p = 2 * (s.n1 - 1) - p;   // reflect (no edge repeat); the right one only happens in an utterance's last push
      long long i = p - s.c0; if (i < 0) i = 0;
      if (i < s.len0) v = tail[i];
      else { long long k = i - s.len0; if (k > W - 1) k = W - 1; v = wv[k]; }
      v *= window[n];
    }
    row[n] = v;
  }
}

// workgroup = one slot: new tail = samples [c1, n1) of [tail | new samples], read whole into registers before any of it is written
__global__ __launch_bounds__(256) void audio_stream_advance_kernel(const float* __restrict__ wave, long long ldw, AfState st, const long long* __restrict__ n_samples,
                                                                   unsigned char* reset, unsigned char* last, int W, int win, int hop) {
  const int b = blockIdx.x;
  const AfSlot s = af_slot(st, n_samples, reset, last, b, W, win, hop);
  const bool move = !s.ended && !s.last;                               // an ended slot keeps nothing
  const long long c1 = af_first(af_ready(s.n1, win, hop), win, hop);
  long long len1 = s.n1 - c1; if (len1 > AF_CAP) len1 = AF_CAP;
  float* tail = st.tail + (long long)b * AF_CAP; const float* wv = wave + (long long)b * ldw;
  float v[AF_CAP / 256];
#pragma unroll
  for (int q = 0; q < AF_CAP / 256; ++q) {
    const int jx = threadIdx.x + 256 * q; v[q] = 0.f;
    if (move && jx < len1) {
      const long long g = c1 + jx;
      if (g < s.n0) { long long i = g - s.c0; i = i < 0 ? 0 : (i > AF_CAP - 1 ? AF_CAP - 1 : i); v[q] = tail[i]; }
      else { long long k = g - s.n0; if (k > W - 1) k = W - 1; v[q] = wv[k]; }
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < AF_CAP / 256; ++q) { const int jx = threadIdx.x + 256 * q; if (move && jx < len1) tail[jx] = v[q]; }
  if (threadIdx.x == 0) {
    st.n[b] = s.n1; st.ended[b] = (s.ended || s.last) ? 1 : 0;
    if (reset) reset[b] = 0;
    if (last) last[b] = 0;
  }
}

// workgroup = one output row (slot b, local stem frame r): the 3 mel columns it touches staged zero-padded in LDS ([NM + 2][3], the offline 8-wide kernel's
// patch), thread = 8 consecutive fo of one channel per iteration: conv + bias in the offline tap order, y * scale + shift, Swish, one 16-byte store
template <typename T>
__global__ __launch_bounds__(256) void audio_stem_stream_kernel(const float* __restrict__ mel, const float* __restrict__ w, const float* __restrict__ bias,
                                                                const float* __restrict__ ss, T* __restrict__ out, const long long* __restrict__ out_len,
                                                                const long long* __restrict__ meta, int NM, int Tmax, int C, int Fo, int patch_floats) {
  extern __shared__ __attribute__((aligned(16))) float asp_[];
  const int Fmax = 2 * Tmax + 1;
  const int b = blockIdx.x / Tmax, r = blockIdx.x - b * Tmax;
  const int J = C * Fo, F8 = Fo >> 3, chunks = C * F8;
  T* orow = out + (long long)blockIdx.x * J;
  if (r >= out_len[b]) {                                              // (uniform over the workgroup)
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int ch = threadIdx.x; ch < chunks; ch += 256) st8<T>(orow + ch * 8, z);
    return;
  }
  const long long m0 = meta[2 * b], Fv = meta[2 * b + 1];
  for (int idx = threadIdx.x; idx < patch_floats; idx += 256) {
    const int fi = idx / 3 - 1, kw = idx - (fi + 1) * 3; const int jc = 2 * r + kw; const long long m = m0 + jc;
    asp_[idx] = (fi >= 0 && fi < NM && jc < Fmax && m >= 0 && m < Fv) ? mel[((long long)b * NM + fi) * Fmax + jc] : 0.f;
  }
  __syncthreads();
  for (int ch = threadIdx.x; ch < chunks; ch += 256) {
    const int c = ch / F8, fo0 = (ch - c * F8) * 8;
    float wk[10];
#pragma unroll
    for (int q = 0; q < 9; ++q) wk[q] = w[c * 9 + q];
    wk[9] = bias ? bias[c] : 0.f;
    const float sc = ss[c], sh = ss[C + c];
    float p[52], acc[8];
    const float4* pq = (const float4*)(asp_ + 6 * fo0);               // patch rows 2 fo0 .. 2 fo0 + 16 (x 3 taps): 51 contiguous floats, 16-byte aligned
#pragma unroll
    for (int k = 0; k < 13; ++k) { const float4 t = pq[k]; p[4 * k] = t.x; p[4 * k + 1] = t.y; p[4 * k + 2] = t.z; p[4 * k + 3] = t.w; }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = wk[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) a += wk[q] * p[6 * e + q];
      acc[e] = swishf_(a * sc + sh);
    }
    st8<T>(orow + c * Fo + fo0, acc);
  }
}

extern "C" long long avec_audio_stream_state_bytes(int B) { return B <= 0 ? 0 : (long long)B * (AF_CAP * (long long)sizeof(float) + 16); }

static int af_check(const char* who, const void* wave, long long ldw, const void* state, long long state_bytes, const void* n_samples, int B, int W, int n_fft, int win, int hop) {
  AVEC_CHECK_ARG(wave && state, "%s: null pointer (wave and state are required)", who);
  AVEC_CHECK_ARG(B > 0 && W > 0 && ldw >= W, "%s: bad dims B=%d W=%d ldw=%lld", who, B, W, ldw);
  AVEC_CHECK_ARG(hop > 0 && win > 0 && win % 2 == 0 && win <= n_fft, "%s: bad framing n_fft=%d win=%d hop=%d (an even window no longer than n_fft)", who, n_fft, win, hop);
  AVEC_CHECK_ARG(2 * (hop + win / 2) <= AF_CAP, "%s: hop=%d win=%d needs a tail of %d samples per slot, the state holds %d", who, hop, win, 2 * (hop + win / 2), AF_CAP);
  AVEC_CHECK_ARG(state_bytes >= avec_audio_stream_state_bytes(B), "%s: state of %lld bytes, %lld needed (avec_audio_stream_state_bytes)", who, state_bytes, avec_audio_stream_state_bytes(B));
  AVEC_CHECK_ARG(avec_aligned16(state) && (((uintptr_t)wave) & 3) == 0 && (((uintptr_t)n_samples) & 7) == 0, "%s: state must be 16-byte aligned, n_samples 8-byte aligned (int64)", who);
  return 0;
}
extern "C" int avec_mel_frames_stream(const float* wave, long long ldw, const float* window, float* frames, const void* state, long long state_bytes,
                                      const long long* n_samples, const unsigned char* reset, const unsigned char* last, long long* out_len, long long* meta,
                                      int B, int W, int Tmax, int n_fft, int win, int hop, hipStream_t st) {
  if (int r = af_check("mel_frames_stream", wave, ldw, state, state_bytes, n_samples, B, W, n_fft, win, hop)) return r;
  AVEC_CHECK_ARG(window && frames && out_len && meta, "mel_frames_stream: null pointer (window, frames, out_len and meta are required)");
  AVEC_CHECK_ARG(Tmax > 0 && (long long)B * (2 * (long long)Tmax + 1) < (1ll << 31), "mel_frames_stream: bad Tmax=%d", Tmax);
  AVEC_CHECK_ARG((((uintptr_t)out_len) & 7) == 0 && (((uintptr_t)meta) & 7) == 0, "mel_frames_stream: out_len and meta must be 8-byte aligned (int64)");
  hipLaunchKernelGGL(mel_frames_stream_kernel, dim3((unsigned)(B * (2 * Tmax + 1))), dim3(256), 0, st, wave, ldw, window, frames, af_state((void*)state, B), n_samples, reset, last,
                     out_len, meta, W, Tmax, win, hop);
  AVEC_LAUNCH_CHECK(); return 0;
}
extern "C" int avec_audio_stream_advance(const float* wave, long long ldw, void* state, long long state_bytes, const long long* n_samples, unsigned char* reset,
                                         unsigned char* last, int B, int W, int n_fft, int win, int hop, hipStream_t st) {
  if (int r = af_check("audio_stream_advance", wave, ldw, state, state_bytes, n_samples, B, W, n_fft, win, hop)) return r;
  hipLaunchKernelGGL(audio_stream_advance_kernel, dim3((unsigned)B), dim3(256), 0, st, wave, ldw, af_state(state, B), n_samples, reset, last, W, win, hop);
  AVEC_LAUNCH_CHECK(); return 0;
}
extern "C" int avec_audio_stem_stream(int dtype, const float* mel, const float* w, const float* bias, const float* ss, void* out, const long long* out_len,
                                      const long long* meta, int B, int n_mels, int Tmax, int C, hipStream_t st) {
  AVEC_CHECK_ARG(mel && w && ss && out && out_len && meta, "audio_stem_stream: null pointer (mel, w, ss, out, out_len and meta are required)");
  AVEC_CHECK_ARG(B > 0 && Tmax > 0 && C > 0 && n_mels > 0 && (long long)B * Tmax < (1ll << 31), "audio_stem_stream: bad dims B=%d Tmax=%d C=%d n_mels=%d", B, Tmax, C, n_mels);
  AVEC_CHECK_ARG(n_mels % 2 == 0 && (n_mels / 2) % 8 == 0, "audio_stem_stream: n_mels=%d must be even with n_mels / 2 a multiple of 8 (8 output bins per 16-byte store)", n_mels);
  AVEC_CHECK_ARG(avec_aligned16(out) && (((uintptr_t)out_len) & 7) == 0 && (((uintptr_t)meta) & 7) == 0, "audio_stem_stream: out must be 16-byte aligned, out_len and meta 8-byte aligned");
  const int patch_floats = ((n_mels + 2) * 3 + 4 + 3) & ~3;
  AVEC_CHECK_ARG((size_t)patch_floats * 4 <= 48 * 1024, "audio_stem_stream: n_mels=%d too large for the LDS patch", n_mels);
  DISPATCH_T(dtype, hipLaunchKernelGGL(audio_stem_stream_kernel<T>, dim3((unsigned)(B * Tmax)), dim3(256), (size_t)patch_floats * 4, st, mel, w, bias, ss, (T*)out, out_len, meta,
                                       n_mels, Tmax, C, n_mels / 2, patch_floats));
  AVEC_LAUNCH_CHECK(); return 0;
}
