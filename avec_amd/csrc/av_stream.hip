// Streamed audio-visual fusion input (nnet.AudioVisualStreamSession): pairs the 80 ms rows of the audio and the visual branch across pushes and writes the operand of the
// fusion module's first Linear, [audio row | video row] in the activation dtype.
//   The audio front-end looks 40 samples ahead, the visual stem 2 frames: in some pushes one branch is a row ahead of the other and, at the end of an utterance, one
//   branch ends a push before the other.  Per slot the state is two rings of `cap` rows (absolute row p of a branch in ring row p mod cap, already cast: the cast is
//   cast_rows', so a carried row is bit-identical to a freshly cast one) and three int64 counters: audio rows received, video rows received, pairs emitted.
//   A restart only makes the counters count as 0 (nothing is cleared: whatever the rings hold is older than the counters and counts as absent).
// One launch per push, workgroup = one slot: phase 1 reads the old state (counters, pending ring rows) and this push's rows and writes the pairs; a barrier; phase 2
// overwrites the state (this push's rows into their ring rows, then the counters from one thread).  Every output element is a copy of one input element through one
// cast; no atomics.  Rows at or past a_len / v_len are never loaded.
#include <type_traits>
#include "vec.h"
#include "avec_hip.h"

// state blob: [B][cap][Da] T audio ring | [B][cap][Dv] T video ring | [B][3] int64 (audio rows received, video rows received, pairs emitted), padded to 16 bytes
struct AvState { char* ring_a; char* ring_v; long long* cnt; };
static __host__ __device__ __forceinline__ AvState av_state(void* base, int B, int Da, int Dv, int cap, size_t esz) {
  AvState s; s.ring_a = (char*)base; s.ring_v = s.ring_a + (size_t)B * cap * Da * esz; s.cnt = (long long*)(s.ring_v + (size_t)B * cap * Dv * esz); return s;
}

// four elements as they lie in memory (a carried row is copied, not converted again)
__device__ __forceinline__ void av_copy4(float* dst, const float* src) { *(float4*)dst = *(const float4*)src; }
__device__ __forceinline__ void av_copy4(bf16* dst, const bf16* src) { *(uint2*)dst = *(const uint2*)src; }
__device__ __forceinline__ int av_ring_row(long long p, int cap) { const int r = (int)(p % cap); return r < 0 ? r + cap : r; }

template <typename T>
__global__ __launch_bounds__(256) void av_fuse_stream_kernel(const float* __restrict__ a, const long long* __restrict__ a_len, const float* __restrict__ v,
                                                             const long long* __restrict__ v_len, AvState st, unsigned char* reset, T* __restrict__ xc,
                                                             long long* __restrict__ pair_len, int Ra, int Rv, int Da, int Dv, int cap, int max_emit) {
  const int b = blockIdx.x, tid = threadIdx.x;
  // ---- the old state and the controls, read by every thread before anything is written
  const bool rs = reset && reset[b];
  long long na = rs ? 0 : st.cnt[3 * b], nv = rs ? 0 : st.cnt[3 * b + 1], em = rs ? 0 : st.cnt[3 * b + 2];
  if (na < 0) na = 0;
  if (nv < 0) nv = 0;
  if (em < 0) em = 0;
  if (em > na) em = na;                                                // (a state never written: no pair is pending, no access out of range)
  if (em > nv) em = nv;
  long long la = a_len[b], lv = v_len[b];
  la = la < 0 ? 0 : (la > Ra ? Ra : la); lv = lv < 0 ? 0 : (lv > Rv ? Rv : lv);
  long long m = min(na + la - em, nv + lv - em);
  m = m < 0 ? 0 : (m > max_emit ? max_emit : m);
  T* const ra = (T*)st.ring_a + (long long)b * cap * Da;
  T* const rv = (T*)st.ring_v + (long long)b * cap * Dv;
  const float* const ab = a + (long long)b * Ra * Da;
  const float* const vb = v + (long long)b * Rv * Dv;
  const int Da4 = Da >> 2, W4 = (Da + Dv) >> 2, D = Da + Dv;
  // ---- phase 1: pair i = rows em + i of both branches; a row older than this push comes from its ring, a row of this push from the input through the cast
  T* const ob = xc + (long long)b * max_emit * D;
  for (int q = tid; q < max_emit * W4; q += 256) {
    const int i = q / W4, c4 = q - i * W4;
    T* const dst = ob + (long long)i * D + 4 * c4;
    if (i >= m) { const float z[4] = {0.f, 0.f, 0.f, 0.f}; st4<T>(dst, z); continue; }
    const long long p = em + i;
    const bool aud = c4 < Da4;
    const int c = 4 * (aud ? c4 : c4 - Da4), Dx = aud ? Da : Dv;
    const long long n0 = aud ? na : nv;
    if (p < n0) av_copy4(dst, (aud ? ra : rv) + (long long)av_ring_row(p, cap) * Dx + c);
    else { float x[4]; ld4<float>((aud ? ab : vb) + (p - n0) * Dx + c, x); st4<T>(dst, x); }
  }
  __syncthreads();
  // ---- phase 2: this push's rows into their ring rows (Ra, Rv <= cap: no two of them share one), then the counters
  for (int q = tid; q < (int)la * Da4; q += 256) {
    const int i = q / Da4, c = 4 * (q - i * Da4);
    float x[4]; ld4<float>(ab + (long long)i * Da + c, x); st4<T>(ra + (long long)av_ring_row(na + i, cap) * Da + c, x);
  }
  const int Dv4 = Dv >> 2;
  for (int q = tid; q < (int)lv * Dv4; q += 256) {
    const int i = q / Dv4, c = 4 * (q - i * Dv4);
    float x[4]; ld4<float>(vb + (long long)i * Dv + c, x); st4<T>(rv + (long long)av_ring_row(nv + i, cap) * Dv + c, x);
  }
  if (tid == 0) {
    st.cnt[3 * b] = na + la; st.cnt[3 * b + 1] = nv + lv; st.cnt[3 * b + 2] = em + m;
    pair_len[b] = m;
    if (reset) reset[b] = 0;
  }
}

// ------------------------------------------------------------------------------------------------
extern "C" long long avec_av_fuse_stream_state_bytes(int dtype, int B, int Da, int Dv, int cap) {
  if (B <= 0 || Da <= 0 || Dv <= 0 || cap <= 0 || (Da & 3) || (Dv & 3) || (dtype != AVEC_BF16 && dtype != AVEC_F32)) return 0;
  const long long n = (long long)B * ((long long)cap * (Da + Dv) * (dtype == AVEC_BF16 ? 2 : 4) + 24);
  return (n + 15) & ~15ll;
}

extern "C" int avec_av_fuse_stream(int dtype, const float* a, const long long* a_len, const float* v, const long long* v_len, void* state, long long state_bytes,
                                   unsigned char* reset, void* xc, long long* pair_len, int B, int Ra, int Rv, int Da, int Dv, int cap, int max_emit, hipStream_t st) {
  const char* who = "av_fuse_stream";
  AVEC_CHECK_ARG(a && a_len && v && v_len && state && xc && pair_len, "%s: null pointer (a, a_len, v, v_len, state, xc and pair_len are required)", who);
  AVEC_CHECK_ARG(dtype == AVEC_BF16 || dtype == AVEC_F32, "%s: dtype %d", who, dtype);
  AVEC_CHECK_ARG(B > 0 && B < 65536 && Ra > 0 && Rv > 0 && Da > 0 && Dv > 0 && Da <= 65536 && Dv <= 65536, "%s: bad dims B=%d Ra=%d Rv=%d Da=%d Dv=%d", who, B, Ra, Rv, Da, Dv);
  AVEC_CHECK_ARG((Da & 3) == 0 && (Dv & 3) == 0, "%s: row widths Da=%d Dv=%d must be multiples of 4 (16-byte accesses on the fp32 side)", who, Da, Dv);
  AVEC_CHECK_ARG(max_emit >= 1 && max_emit < 65536, "%s: bad max_emit=%d", who, max_emit);
  AVEC_CHECK_ARG(cap >= max_emit + 2 && cap < 65536, "%s: ring of cap=%d rows for max_emit=%d (at least max_emit + 2)", who, cap, max_emit);
  AVEC_CHECK_ARG(Ra <= cap && Rv <= cap, "%s: a push of Ra=%d / Rv=%d rows does not fit a ring of cap=%d rows", who, Ra, Rv, cap);
  AVEC_CHECK_ARG(state_bytes == avec_av_fuse_stream_state_bytes(dtype, B, Da, Dv, cap), "%s: state of %lld bytes, %lld expected (avec_av_fuse_stream_state_bytes)", who,
                 state_bytes, avec_av_fuse_stream_state_bytes(dtype, B, Da, Dv, cap));
  AVEC_CHECK_ARG(avec_aligned16(a) && avec_aligned16(v) && avec_aligned16(state) && avec_aligned16(xc), "%s: a, v, state and xc must be 16-byte aligned", who);
  AVEC_CHECK_ARG(((((uintptr_t)a_len) | ((uintptr_t)v_len) | ((uintptr_t)pair_len)) & 7) == 0, "%s: a_len, v_len and pair_len must be 8-byte aligned (int64)", who);
  const AvState S = av_state(state, B, Da, Dv, cap, dtype == AVEC_BF16 ? 2 : 4);
  DISPATCH_T(dtype, hipLaunchKernelGGL(av_fuse_stream_kernel<T>, dim3((unsigned)B), dim3(256), 0, st, a, a_len, v, v_len, S, reset, (T*)xc, pair_len, Ra, Rv, Da, Dv, cap,
                                       max_emit));
  AVEC_LAUNCH_CHECK(); return 0;
}
