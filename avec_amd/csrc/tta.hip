// Test-time augmentation (VisualEfficientConformerInterCTC(test_augments=...), CTCBeamSearchDecoder(test_time_aug=True); nnet/models_zoo.py:113-122 and
// nnet/decoders.py:177-180,242,252 in the reference): the two small kernels around the one encoder pass over (1 + A) * B clips.
//
//   video_tta_batch  x [B][rows][W] fp32 -> y [B * n][rows][W]: clip b * n + k is x[b], mirrored along W when bit k of flip_mask is set (utterance-major, so the
//                    logits of the batch are a plain view [B][n][T'][V]).  One thread per 16-byte chunk of x (W % 4 == 0: one load, n stores; a mirrored store
//                    goes to chunk W / 4 - 1 - q with its four lanes reversed), one thread per element otherwise.  Every element of y is written exactly once.
//   ctc_tta_pick     the outputs of avec_ctc_beam_search on S = B * n rows -> per utterance the winning (augmentation, beam), its tokens, length and score.
//                    One workgroup per utterance.  Without best_slot the winner is the augmentation whose slot-0 score is highest, scanned from augmentation 0
//                    with a strict >, so ties (and an utterance whose slots are all -inf) go to the lower index; with best_slot (avec_lm_rescore_select's
//                    `best`, an index into the n * W slots) it is that slot, clamped into range before it is used.  out_len is clamped to [0, T].
#include "common.h"
#include "avec_hip.h"

namespace {
constexpr int NT = 256;

template <bool VEC>
__global__ __launch_bounds__(NT) void video_tta_batch_kernel(const float* __restrict__ x, float* __restrict__ y, long long rows, int W, int n, unsigned flip_mask) {
  const int b = blockIdx.y;
  const int WQ = VEC ? W >> 2 : W;                                        // chunks (elements) per row
  const long long per = rows * WQ, i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= per) return;
  const long long r = i / WQ; const int q = (int)(i - r * WQ);
  const size_t clip = (size_t)rows * W;
  float* yr = y + (size_t)b * n * clip + (size_t)r * W;
  if constexpr (VEC) {
    const float4 v = *(const float4*)(x + (size_t)b * clip + (size_t)r * W + 4 * q);
    for (int k = 0; k < n; ++k) {
      const bool f = (flip_mask >> k) & 1u;
      *(float4*)(yr + (size_t)k * clip + 4 * (f ? WQ - 1 - q : q)) = make_float4(f ? v.w : v.x, f ? v.z : v.y, f ? v.y : v.z, f ? v.x : v.w);      // (selects on registers)
    }
  } else {
    const float v = x[(size_t)b * clip + (size_t)r * W + q];
    for (int k = 0; k < n; ++k) yr[(size_t)k * clip + (((flip_mask >> k) & 1u) ? W - 1 - q : q)] = v;
  }
}

__global__ __launch_bounds__(NT) void ctc_tta_pick_kernel(const int* __restrict__ tokens, const int* __restrict__ out_len, const float* __restrict__ score,
                                                          const long long* __restrict__ best_slot, int n, int W, int T, long long* __restrict__ best_aug,
                                                          long long* __restrict__ best_beam, long long* __restrict__ ids, long long* __restrict__ ids_len,
                                                          float* __restrict__ best_score) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int aug = 0, beam = 0;                                                  // (every thread finds the same winner: n broadcast loads)
  if (best_slot) {
    long long s = best_slot[b];
    const long long K = (long long)n * W;
    s = s < 0 ? 0 : (s >= K ? K - 1 : s);
    aug = (int)(s / W); beam = (int)(s - (long long)aug * W);
  } else {
    float best = score[(size_t)b * n * W];
    for (int k = 1; k < n; ++k) {
      const float v = score[((size_t)b * n + k) * W];
      if (v > best) { best = v; aug = k; }
    }
  }
  const size_t slot = ((size_t)b * n + aug) * W + beam;
  const float sc = score[slot];
  int len = out_len[slot];
  len = (len < 0 || !(sc > -INFINITY)) ? 0 : (len > T ? T : len);         // an empty slot has no tokens, whatever its row holds
  const int* row = tokens + slot * (size_t)T;
  for (int t = tid; t < T; t += NT) ids[(size_t)b * T + t] = t < len ? (long long)row[t] : 0ll;
  if (tid == 0) { best_aug[b] = aug; best_beam[b] = beam; ids_len[b] = len; best_score[b] = sc; }
}
}  // namespace

extern "C" int avec_video_tta_batch(const float* x, float* y, int B, long long rows, int W, int n, unsigned flip_mask, hipStream_t st) {
  AVEC_CHECK_ARG(x && y, "video_tta_batch: null pointer");
  AVEC_CHECK_ARG(B >= 1 && B <= 65535 && rows >= 1 && W >= 1 && n >= 1 && n <= 32, "video_tta_batch: bad dims B=%d rows=%lld W=%d n=%d (B in 1..65535, rows >= 1, W >= 1, n in 1..32)",
                 B, rows, W, n);
  AVEC_CHECK_ARG(n == 32 || (flip_mask >> n) == 0u, "video_tta_batch: flip_mask 0x%x has bits at or above n=%d", flip_mask, n);
  AVEC_CHECK_ARG(rows * (long long)W <= 0x7fffffffLL * 256, "video_tta_batch: rows=%lld x W=%d is more than the grid covers", rows, W);
  AVEC_CHECK_ARG((((size_t)x | (size_t)y) & 15) == 0, "video_tta_batch: x and y must be 16-byte aligned");
  if ((W & 3) == 0) {
    const long long per = rows * (W >> 2);
    hipLaunchKernelGGL(video_tta_batch_kernel<true>, dim3((unsigned)((per + NT - 1) / NT), B), dim3(NT), 0, st, x, y, rows, W, n, flip_mask);
  } else {
    const long long per = rows * W;
    hipLaunchKernelGGL(video_tta_batch_kernel<false>, dim3((unsigned)((per + NT - 1) / NT), B), dim3(NT), 0, st, x, y, rows, W, n, flip_mask);
  }
  AVEC_LAUNCH_CHECK(); return 0;
}

extern "C" int avec_ctc_tta_pick(const int* tokens, const int* out_len, const float* score, const long long* best_slot, int B, int n, int W, int T, long long* best_aug,
                                 long long* best_beam, long long* ids, long long* ids_len, float* best_score, hipStream_t st) {
  AVEC_CHECK_ARG(tokens && out_len && score && best_aug && best_beam && ids && ids_len && best_score, "ctc_tta_pick: null pointer");
  AVEC_CHECK_ARG(B >= 1 && n >= 1 && W >= 1 && T >= 1, "ctc_tta_pick: bad dims B=%d n=%d W=%d T=%d (all >= 1)", B, n, W, T);
  AVEC_CHECK_ARG((long long)B * n * W <= 0x7fffffffLL, "ctc_tta_pick: B=%d x n=%d x W=%d beyond 2^31", B, n, W);
  AVEC_CHECK_ARG((((size_t)tokens | (size_t)out_len | (size_t)score | (size_t)best_score) & 3) == 0, "ctc_tta_pick: the 32-bit buffers must be 4-byte aligned");
  AVEC_CHECK_ARG((((size_t)best_slot | (size_t)best_aug | (size_t)best_beam | (size_t)ids | (size_t)ids_len) & 7) == 0, "ctc_tta_pick: the 64-bit buffers must be 8-byte aligned");
  hipLaunchKernelGGL(ctc_tta_pick_kernel, dim3(B), dim3(NT), 0, st, tokens, out_len, score, best_slot, n, W, T, best_aug, best_beam, ids, ids_len, best_score);
  AVEC_LAUNCH_CHECK(); return 0;
}
