// CTC prefix beam search with n-gram LM fusion (CTCBeamSearchDecoder, nnet/decoders.py:175-257 of the reference: ctcdecode + KenLM).
//
// One workgroup (8 waves) decodes one utterance; the frame loop runs inside the kernel, the beam state lives in LDS and nothing returns to the host between
// frames.  Per frame:
//   every wave    log_softmax(logits[t] * inv_tmp) in registers (lane l holds tokens l, l+64, ...; every wave computes it the same way)
//   wave 0        the W "stay" candidates (blank / repeat), with the mass of extensions that re-create a prefix already in the beam merged in
//   wave w        for beams i = w, w+8, ...: the LM row ln P(. | ctx_i) (LDS), the V extension scores, and that beam's own top W of them (level 1)
//   -- barrier --
//   wave 0        the global top W among W stays + W*W level-1 survivors (level 2), ranked best first; new beam state; backpointers to the workspace
//   -- barrier --
// Level 2 over level-1 survivors is exact: an extension outside its own beam's top W has W better distinct candidates.  Candidates are ranked by a unique
// 64-bit key (order-preserving score bits << 32 | ~candidate index), so ties go to the lower index and the selection is the same on every run.  Both levels
// find the W-th largest key by a bitwise search of counts (ballot / wave sums): no sort, no atomics.
// A prefix is identified by a 64-bit rolling hash; an extension (i, c) re-creates beam j when hash(j's parent) = hash(i), len(j) = len(i) + 1 and
// last(j) = c (node ids would not do: a prefix can be dropped and created again later).
//
// Streaming (avec_ctc_beam_stream): the same kernel with MODE = STREAMING.  Everything a frame hands to the next one is the current Beams buffer, n_live and the
// backpointer rows, so a launch that loads the buffer from a caller-owned state at its start and stores it at its end can stop after any frame and go on in a
// later launch: per utterance the state is the W * BEAM_BYTES_PER_SLOT bytes of the buffer (always loaded into st0) plus a 16-byte header {n_live, frames
// consumed, tag of (W, LM order), Tcap}.  The frame body is this one loop for both, so chunked and offline searches do the same arithmetic in the same order.
//
// Ring (avec_ctc_beam_stream_ring): the third mode, a stream without a frame limit.  The backpointer workspace holds `window` rows (row t at t % window) and the
// state header grows by {base, ccount, dropped, commits}.  Immediately before the frame loop consumes absolute frame t with t - base == window, wave 0 runs the
// commit step (ring_commit below): with h = window / 2 and f = base + h - 1, every live beam walks rows t-1 .. f+1 to the slot it descends from after frame f; the
// tokens on the best beam's path through rows f .. base go to the commit log with their frames; the beams that descend from another slot are dropped, the others
// compacted in place (row t-1 with them); base = f + 1.  The step depends on the frame index alone, so any split into pushes gives the same bits, and until frame
// `window` the search is the offline one.  An emitting push walks rows t-1 .. base only and writes the tails [W][window] with their emission frames.
#include "common.h"
#include "avec_hip.h"

namespace {
typedef unsigned long long u64;
constexpr int NW = 8, NT = NW * 64, MAXV = 1024, NPL = MAXV / 64, MAXW = 64, KMAX = 7, MAXORDER = KMAX + 1;
constexpr u64 H_EMPTY = 0x6A09E667F3BCC909ull;

__host__ __device__ inline u64 mix64(u64 x) {      // splitmix64 finaliser
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
  return x;
}
__device__ __forceinline__ u64 child_hash(u64 parent, int c) { return mix64(parent ^ ((u64)(c + 1) * 0x9E3779B97F4A7C15ull)); }

__device__ __forceinline__ float lse2(float a, float b) {      // ln(e^a + e^b), exact when one side is -inf
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (n == -INFINITY) return m;
  return m + log1pf(expf(n - m));
}
// unique ranking key: larger = better; 0 = never kept (-inf or NaN score)
__device__ __forceinline__ u64 make_key(float s, unsigned idx) {
  if (!(s > -INFINITY)) return 0ull;
  unsigned u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((u64)u << 32) | (u64)(~idx);
}
__device__ __forceinline__ u64 lanemask_lt(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

// The W-th largest of the non-zero keys a wave holds (NPL per lane in registers, nk of them live), or 1 when at most W are non-zero: keep key >= result.
__device__ u64 wave_topw_threshold(const u64 (&key)[NPL], int nk, int W) {
  auto count = [&](u64 t) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < NPL; ++k)
      if (k < nk) c += __popcll(__ballot(key[k] >= t));
    return c;
  };
  if (count(1) <= W) return 1;
  u64 thr = 0;
  for (int bit = 63; bit >= 0; --bit) {
    const u64 t = thr | (1ull << bit);
    const int c = count(t);
    if (c >= W) { thr = t; if (c == W) break; }
  }
  return thr;
}
// the same over n keys in LDS (one wave)
__device__ u64 lds_topw_threshold(const u64* key, int n, int W, int lane) {
  auto count = [&](u64 t) {
    int c = 0;
    for (int j = lane; j < n; j += 64) c += key[j] >= t;
    return (int)wave_sum((float)c);
  };
  if (count(1) <= W) return 1;
  u64 thr = 0;
  for (int bit = 63; bit >= 0; --bit) {
    const u64 t = thr | (1ull << bit);
    const int c = count(t);
    if (c >= W) { thr = t; if (c == W) break; }
  }
  return thr;
}

// row[c] = ln P(c | ctx) for one context (one wave).  win[p * stride], p < clen: the last clen (<= order-1) tokens of <s> + prefix, oldest first, -1 = <s>.
__device__ void build_row(const avec_ngram_t& lm, const int* win, int stride, int clen, float oov, float* row, int V, int lane) {
  float bo = 0.f; int off = 0, cnt = 0;
  if (lane < clen && lm.ctx_cap > 0) {                 // lane s probes the suffix of length s + 1
    const int L = lane + 1;
    u64 lo = 0, hi = 0;
    for (int j = 0; j < L; ++j) {
      const int tok = win[(clen - L + j) * stride];
      const u64 code = tok < 0 ? 0xFFFFull : (u64)(tok + 1);
      if (j < 4) lo |= code << (16 * j); else hi |= code << (16 * (j - 4));
    }
    const u64 mask = (u64)lm.ctx_cap - 1;
    u64 h = mix64(lo * 0x9E3779B97F4A7C15ull ^ hi * 0xC2B2AE3D27D4EB4Full) & mask;
    for (long long probe = 0; probe < lm.ctx_cap; ++probe) {
      const u64 klo = lm.ctx_key[2 * h], khi = lm.ctx_key[2 * h + 1];
      if (klo == lo && khi == hi) { bo = lm.ctx_bo[h]; off = lm.ctx_off[h]; cnt = lm.ctx_cnt[h]; break; }
      if ((klo | khi) == 0) break;
      h = (h + 1) & mask;
    }
  }
  const float tot = wave_sum(bo);
  for (int c = lane; c < V; c += 64) {
    const float u = lm.unigram[c];
    row[c] = u == -INFINITY ? oov : u + tot;
  }
  float sfx = tot;                                      // backoffs of the suffixes longer than the current one
  for (int s = 0; s < clen; ++s) {
    const float bs = __shfl(bo, s, 64); const int os = __shfl(off, s, 64), ns = __shfl(cnt, s, 64);
    sfx -= bs;
    __builtin_amdgcn_wave_barrier();
    for (int j = lane; j < ns; j += 64) row[lm.cont_tok[os + j]] = lm.cont_lp[os + j] + sfx;
  }
  __builtin_amdgcn_wave_barrier();
}

struct Beams {          // one beam buffer in LDS, structure of arrays over W slots
  u64* hash; u64* phash; float* pb; float* pnb; float* lm; int* last; int* len; int* clen; int* ctx;   // ctx: [KMAX][W], right-aligned window
};
constexpr int BEAM_BYTES_PER_SLOT = 2 * 8 + 3 * 4 + 3 * 4 + KMAX * 4;
__device__ __forceinline__ Beams carve(unsigned char* p, int W) {
  Beams s;
  s.hash = (u64*)p; s.phash = s.hash + W; s.pb = (float*)(s.phash + W); s.pnb = s.pb + W; s.lm = s.pnb + W;
  s.last = (int*)(s.lm + W); s.len = s.last + W; s.clen = s.len + W; s.ctx = s.clen + W;
  return s;
}

__host__ __device__ inline size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }
struct Lay { size_t ck, cpnb, clm, spb, logp, rows, selk, selp, st0, st1, misc, total; };
__host__ __device__ inline Lay lay(int W, int V, bool lm) {
  Lay L; size_t o = 0; const size_t nc = (size_t)W + (size_t)W * W;
  L.ck = o; o = a16(o + nc * 8); L.cpnb = o; o = a16(o + nc * 4); L.clm = o; o = a16(o + nc * 4); L.spb = o; o = a16(o + (size_t)W * 4);
  L.logp = o; o = a16(o + (size_t)V * 4); L.rows = o; o = a16(o + (lm ? (size_t)NW * V * 4 : 0));
  L.selk = o; o = a16(o + (size_t)W * 8); L.selp = o; o = a16(o + (size_t)W * 4);
  L.st0 = o; o = a16(o + (size_t)W * BEAM_BYTES_PER_SLOT); L.st1 = o; o = a16(o + (size_t)W * BEAM_BYTES_PER_SLOT);
  L.misc = o; o += 32; L.total = o;                    // {n_live, common prefix, -, -} and the ring mode's {-, ccount, dropped, commits}
  return L;
}

struct BeamArgs {
  const float* logits; const long long* lengths; int T, V, W; float inv_tmp;
  avec_ngram_t lm; float alpha, beta, oov;
  int* bp; int* tokens; int* out_len; float* score; float* ctc_logp;
  // streaming only: lengths = frames of this chunk per utterance (null: T), T = frames per utterance in `logits`, Tcap = rows of bp and of tokens
  int Tcap, emit; const unsigned char* reset; unsigned char* state; int* stable_len;
  // ring only (Tcap = window): the commit log [B][log_frames] of (token, frame), the tails' emission frames [B][W][window], info [B][4] = {base, ccount, dropped, commits}
  int2* log; int log_frames; int* frames; int* info;
};
constexpr int STATE_TAG = 0x43544342, RING_TAG = 0x43544352;
constexpr int OFFLINE = 0, STREAMING = 1, RING = 2;
__host__ __device__ inline size_t state_stride(int W) { return a16((size_t)W * BEAM_BYTES_PER_SLOT) + 16; }
__host__ __device__ inline size_t ring_state_stride(int W) { return a16((size_t)W * BEAM_BYTES_PER_SLOT) + 32; }

// The commit step of the ring mode (wave 0, one lane per beam), run before absolute frame t is consumed when t - base == window.  rg = {-, ccount, dropped, commits}
// in LDS.  Every walk is bounded by `window` rows; rows are taken % window, slots clamped to W and log positions taken % log_frames before use.
template <bool LM>
__device__ __forceinline__ void ring_commit(const Beams& S, int* n_live, int* rg, int* bp, int2* log, int log_frames, int W, int K, int window, int base, int t, int lane) {
  const int nl = *n_live, f = base + (window >> 1) - 1;
  int anc = lane;                                      // 1. the slot beam `lane` descends from after frame f
  if (lane < nl)
    for (int r = t - 1; r > f; --r) {
      anc = bp[(size_t)(r % window) * W + anc] & 255;
      if (anc >= W) anc = 0;
    }
  const int a = __shfl(anc, 0, 64);                    // slot 0 is the best beam: the buffer is ranked best first
  const int cc = rg[1];
  int n = 0;                                           // 2. the tokens on a's path through rows f .. base: counted, then logged in forward order
  if (nl > 0) {                                        // (every lane walks the same addresses: one request per row)
    int s = a;
    for (int r = f; r >= base; --r) {
      const int code = bp[(size_t)(r % window) * W + s];
      n += (code >> 8) != 0;
      s = code & 255;
      if (s >= W) s = 0;
    }
    s = a;
    int k = n;
    for (int r = f; r >= base && k > 0; --r) {
      const int code = bp[(size_t)(r % window) * W + s];
      if (code >> 8) {
        --k;
        if (lane == 0) log[(unsigned)(cc + k) % (unsigned)log_frames] = make_int2((code >> 8) - 1, r);
      }
      s = code & 255;
      if (s >= W) s = 0;
    }
  }
  const bool keep = lane < nl && anc == a;             // 3. drop the beams of other ancestors, compact the rest in their order
  const u64 m = __ballot(keep);
  const int p = __popcll(m & lanemask_lt(lane)), ns = __popcll(m);
  int* last_row = bp + (size_t)((t - 1) % window) * W;
  u64 hs = 0, ph = 0; float pb = 0.f, pnb = 0.f, lmv = 0.f; int last = 0, len = 0, clen = 0, code = 0;
  [[maybe_unused]] int cx[KMAX];
  if (keep) {                                          // every source field into registers before any is written
    hs = S.hash[lane]; ph = S.phash[lane]; pb = S.pb[lane]; pnb = S.pnb[lane]; lmv = S.lm[lane]; last = S.last[lane]; len = S.len[lane]; clen = S.clen[lane];
    if constexpr (LM) {
#pragma unroll
      for (int q = 0; q < KMAX; ++q) cx[q] = q < K ? S.ctx[q * W + lane] : 0;
    }
    code = last_row[lane];
  }
  __builtin_amdgcn_wave_barrier();
  if (keep) {
    S.hash[p] = hs; S.phash[p] = ph; S.pb[p] = pb; S.pnb[p] = pnb; S.lm[p] = lmv; S.last[p] = last; S.len[p] = len; S.clen[p] = clen;
    if constexpr (LM) {
#pragma unroll
      for (int q = 0; q < KMAX; ++q) if (q < K) S.ctx[q * W + p] = cx[q];
    }
    last_row[p] = code;                                // later walks through row t-1 land on the survivors' new slots
  }
  if (lane == 0) { *n_live = ns; rg[1] = cc + n; rg[2] += nl - ns; rg[3] += 1; }
}

template <bool LM, int MODE>
__global__ __launch_bounds__(NT) void ctc_beam_kernel(BeamArgs a) {
  constexpr bool STREAM = MODE != OFFLINE;
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int W = a.W, V = a.V, T = a.T, K = LM ? a.lm.order - 1 : 0, nk = (V + 63) >> 6;
  const Lay L = lay(W, V, LM);
  u64* ck = (u64*)(sm + L.ck); float* cpnb = (float*)(sm + L.cpnb); float* clm = (float*)(sm + L.clm); float* spb = (float*)(sm + L.spb);
  float* logp_s = (float*)(sm + L.logp); float* rows = (float*)(sm + L.rows);
  u64* selk = (u64*)(sm + L.selk); int* selp = (int*)(sm + L.selp); int* n_live = (int*)(sm + L.misc);
  const int TO = STREAM ? a.Tcap : T;                  // rows of bp and of tokens
  const long long len_ll = (STREAM && !a.lengths) ? T : a.lengths[b];
  int len = len_ll < 0 ? 0 : (len_ll > T ? T : (int)len_ll);
  const float* lg = a.logits + (size_t)b * T * V;
  int* bp = a.bp + (size_t)b * TO * W;
  int t0 = 0;                                          // frames consumed by earlier launches
  bool fresh = true;
  [[maybe_unused]] int base = 0;                       // ring: the oldest frame whose backpointer row is held (the same value in every thread)
  [[maybe_unused]] int* rg = n_live + 4;               // ring: {-, ccount, dropped, commits}
  if constexpr (MODE == RING) {
    const int* st = (const int*)(a.state + (size_t)b * ring_state_stride(W));
    const int* hdr = st + a16((size_t)W * BEAM_BYTES_PER_SLOT) / 4;
    // as below, with a tag of its own; a header is taken only when base, the window it implies and ccount (at most one token per committed frame) are consistent
    fresh = (a.reset && a.reset[b]) || hdr[2] != (RING_TAG ^ (W | K << 8)) || hdr[3] != TO || hdr[0] < 0 || hdr[0] > W || hdr[1] < 0 || hdr[4] < 0 ||
            hdr[4] > hdr[1] || hdr[1] - hdr[4] > TO || hdr[5] < 0 || hdr[5] > hdr[4];
    if (!fresh) {
      t0 = hdr[1]; base = hdr[4];
      int* dst = (int*)(sm + L.st0);
      for (int q = tid; q < W * (BEAM_BYTES_PER_SLOT / 4); q += NT) dst[q] = st[q];
      if (tid == 0) { *n_live = hdr[0]; rg[1] = hdr[5]; rg[2] = hdr[6]; rg[3] = hdr[7]; }
    } else if (tid == 0) {
      rg[1] = 0; rg[2] = 0; rg[3] = 0;
    }
  } else if constexpr (STREAM) {
    const int* st = (const int*)(a.state + (size_t)b * state_stride(W));
    const int* hdr = st + a16((size_t)W * BEAM_BYTES_PER_SLOT) / 4;
    // a state this kernel did not write for the same W, LM order and Tcap (zeroed memory, say) starts from the empty prefix: its fields index LDS and bp
    fresh = (a.reset && a.reset[b]) || hdr[2] != (STATE_TAG ^ (W | K << 8)) || hdr[3] != TO || hdr[0] < 0 || hdr[0] > W || hdr[1] < 0 || hdr[1] > TO;
    if (!fresh) {
      t0 = hdr[1];
      int* dst = (int*)(sm + L.st0);
      for (int q = tid; q < W * (BEAM_BYTES_PER_SLOT / 4); q += NT) dst[q] = st[q];
      if (tid == 0) *n_live = hdr[0];
    }
    len = len < TO - t0 ? len : TO - t0;
  }
  if (fresh && tid == 0) {                             // the empty prefix
    const Beams s = carve(sm + L.st0, W);
    s.hash[0] = H_EMPTY; s.phash[0] = 0; s.pb[0] = 0.f; s.pnb[0] = -INFINITY; s.lm[0] = 0.f; s.last[0] = -1; s.len[0] = 0;
    s.clen[0] = K > 0 ? 1 : 0;
    if (K > 0) s.ctx[(K - 1) * W] = -1;
    *n_live = 1;
  }
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < len; ++t) {
    const Beams S = carve(sm + (cur ? L.st1 : L.st0), W), N = carve(sm + (cur ? L.st0 : L.st1), W);
    if constexpr (MODE == RING) {
      if (t0 + t - base == TO) {                       // the same in every thread: `base` is a register that every thread advances alike
        if (wv == 0) ring_commit<LM>(S, n_live, rg, bp, a.log + (size_t)b * a.log_frames, a.log_frames, W, K, TO, base, t0 + t, lane);
        base += TO >> 1;
        __syncthreads();
      }
    }
    const int nl = *n_live;
    float lp[NPL];
    {
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        const int c = lane + 64 * k;
        lp[k] = (k < nk && c < V) ? lg[(size_t)t * V + c] * a.inv_tmp : -INFINITY;
        mx = fmaxf(mx, lp[k]);
      }
      mx = wave_max(mx);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < NPL; ++k) if (k < nk) se += expf(lp[k] - mx);
      const float lse = logf(wave_sum(se));
#pragma unroll
      for (int k = 0; k < NPL; ++k) lp[k] = (lp[k] - mx) - lse;
    }
    if (wv == 0) {
#pragma unroll
      for (int k = 0; k < NPL; ++k) if (k < nk && lane + 64 * k < V) logp_s[lane + 64 * k] = lp[k];
      __builtin_amdgcn_wave_barrier();
      if (lane < nl) {                                 // stays of slot j: blank, repeat, and the extension that re-creates j
        const int j = lane, e = S.last[j];
        const float pb = S.pb[j], pnb = S.pnb[j];
        const float npb = lse2(pb, pnb) + logp_s[0];
        float npnb = e >= 0 ? pnb + logp_s[e] : -INFINITY;
        if (S.len[j] > 0) {
          const u64 ph = S.phash[j];
          for (int i = 0; i < nl; ++i)
            if (S.hash[i] == ph && S.len[i] == S.len[j] - 1) {
              npnb = lse2(npnb, (S.last[i] == e ? S.pb[i] : lse2(S.pb[i], S.pnb[i])) + logp_s[e]);
              break;
            }
        }
        ck[j] = make_key(lse2(npb, npnb) + S.lm[j], (unsigned)j);
        spb[j] = npb; cpnb[j] = npnb; clm[j] = S.lm[j];
      } else if (lane < W) {
        ck[lane] = 0;
      }
    }
    for (int i = wv; i < nl; i += NW) {                // level 1: beam i's own top W extensions
      const float pb = S.pb[i], pnb = S.pnb[i], lmi = S.lm[i], pall = lse2(pb, pnb);
      const int e = S.last[i];
      float* row = rows + (size_t)wv * V;
      if (LM) build_row(a.lm, S.ctx + (K - S.clen[i]) * W + i, W, S.clen[i], a.oov, row, V, lane);
      u64 key[NPL]; float pe[NPL], lv[NPL];
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        const int c = lane + 64 * k;
        key[k] = 0; pe[k] = -INFINITY; lv[k] = 0.f;
        if (k < nk && c < V && c != 0) {
          pe[k] = (c == e ? pb : pall) + lp[k];
          lv[k] = LM ? lmi + a.alpha * row[c] + a.beta : lmi;
          key[k] = make_key(pe[k] + lv[k], (unsigned)(W + i * V + c));
        }
      }
      const u64 hi = S.hash[i]; const int li = S.len[i];
      for (int j = 0; j < nl; ++j)                     // merged into an existing beam (its stay): not an extension candidate
        if (S.phash[j] == hi && S.len[j] == li + 1) {
          const int c = S.last[j];
#pragma unroll
          for (int k = 0; k < NPL; ++k) if (c == lane + 64 * k) key[k] = 0;
        }
      const u64 thr = wave_topw_threshold(key, nk, W);
      const int base0 = W + i * W;
      int base = 0;
#pragma unroll
      for (int k = 0; k < NPL; ++k) {
        if (k < nk) {
          const bool keep = key[k] >= thr;
          const u64 m = __ballot(keep);
          const int q = base + __popcll(m & lanemask_lt(lane));
          if (keep && q < W) { ck[base0 + q] = key[k]; cpnb[base0 + q] = pe[k]; clm[base0 + q] = lv[k]; }
          base += __popcll(m);
        }
      }
      for (int p = (base < W ? base : W) + lane; p < W; p += 64) ck[base0 + p] = 0;
    }
    __syncthreads();
    if (wv == 0) {                                     // level 2 + new beam state
      const int n = W + nl * W;
      const u64 thr = lds_topw_threshold(ck, n, W, lane);
      int ns = 0;
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const bool keep = j < n && ck[j] >= thr;
        const u64 m = __ballot(keep);
        const int p = ns + __popcll(m & lanemask_lt(lane));
        if (keep && p < W) { selk[p] = ck[j]; selp[p] = j; }
        ns += __popcll(m);
      }
      ns = ns < W ? ns : W;                            // exactly W unless fewer are live (unique keys); the clamp only guards the LDS bounds
      __builtin_amdgcn_wave_barrier();
      if (lane < ns) {
        const u64 mk = selk[lane];
        int r = 0;
        for (int m = 0; m < ns; ++m) r += selk[m] > mk;
        const int p = selp[lane];
        const unsigned idx = ~(unsigned)mk;
        int code;
        if (p < W) {                                   // stay of slot p
          N.hash[r] = S.hash[p]; N.phash[r] = S.phash[p]; N.last[r] = S.last[p]; N.len[r] = S.len[p]; N.clen[r] = S.clen[p];
          for (int q = 0; q < K; ++q) N.ctx[q * W + r] = S.ctx[q * W + p];
          N.pb[r] = spb[p];
          code = p;
        } else {                                       // extension (i, c)
          const int i = (int)((idx - (unsigned)W) / (unsigned)V), c = (int)(idx - (unsigned)W - (unsigned)(i * V));
          N.hash[r] = child_hash(S.hash[i], c); N.phash[r] = S.hash[i]; N.last[r] = c; N.len[r] = S.len[i] + 1;
          N.clen[r] = S.clen[i] + 1 < K ? S.clen[i] + 1 : K;
          for (int q = 0; q + 1 < K; ++q) N.ctx[q * W + r] = S.ctx[(q + 1) * W + i];
          if (K > 0) N.ctx[(K - 1) * W + r] = c;
          N.pb[r] = -INFINITY;
          code = i | ((c + 1) << 8);
        }
        N.pnb[r] = cpnb[p]; N.lm[r] = clm[p];
        bp[(size_t)(MODE == RING ? (t0 + t) % TO : t0 + t) * W + r] = code;
      }
      if (lane == 0) *n_live = ns;
    }
    __syncthreads();
    cur ^= 1;
  }
  const Beams S = carve(sm + (cur ? L.st1 : L.st0), W);
  const int nl = *n_live;
  const int cc = MODE == RING ? rg[1] : 0;             // ring: tokens already committed; the outputs below are the tails after them
  if constexpr (STREAM) {
    int* st = (int*)(a.state + (size_t)b * (MODE == RING ? ring_state_stride(W) : state_stride(W)));
    const int* src = (const int*)(sm + (cur ? L.st1 : L.st0));
    for (int q = tid; q < W * (BEAM_BYTES_PER_SLOT / 4); q += NT) st[q] = src[q];
    if (tid == 0) {
      int* hdr = st + a16((size_t)W * BEAM_BYTES_PER_SLOT) / 4;
      hdr[0] = nl; hdr[1] = t0 + len; hdr[2] = (MODE == RING ? RING_TAG : STATE_TAG) ^ (W | K << 8); hdr[3] = TO;
      if constexpr (MODE == RING) { hdr[4] = base; hdr[5] = cc; hdr[6] = rg[2]; hdr[7] = rg[3]; }
    }
    if (!a.emit) return;
  }
  int* tok = a.tokens + (size_t)b * W * TO;
  [[maybe_unused]] int* frm = MODE == RING ? a.frames + (size_t)b * W * TO : nullptr;
  if (tid < W) {
    const int w = tid;
    float sc = -INFINITY, cl = -INFINITY; int ol = 0;
    if (w < nl) {
      cl = lse2(S.pb[w], S.pnb[w]); sc = cl + S.lm[w]; ol = S.len[w] - cc;
      if constexpr (MODE == RING) ol = ol < 0 ? 0 : (ol > TO ? TO : ol);      // at most one token per held row
      int slot = w, pos = ol - 1;
      for (int t = t0 + len - 1; t >= base && pos >= 0; --t) {   // walk the backpointers (streaming: through every frame so far; ring: down to base)
        const int code = bp[(size_t)(MODE == RING ? t % TO : t) * W + slot];
        if (code >> 8) {
          if constexpr (MODE == RING) frm[(size_t)w * TO + pos] = t;
          tok[(size_t)w * TO + pos--] = (code >> 8) - 1;
        }
        slot = code & 255;
        if (STREAM && slot >= W) slot = 0;               // (rows a caller swapped under the state: stay inside the buffer)
      }
    }
    a.score[(size_t)b * W + w] = sc; a.ctc_logp[(size_t)b * W + w] = cl; a.out_len[(size_t)b * W + w] = ol;
  }
  for (int q = tid; q < W * TO; q += NT) {
    const int w = q / TO, k = q - w * TO;
    if (k >= (w < nl ? S.len[w] - cc : 0)) {
      tok[q] = 0;
      if constexpr (MODE == RING) frm[q] = 0;
    }
  }
  if constexpr (STREAM) {                              // the longest common prefix of the live beams: every later hypothesis extends one of them
    int* common = n_live + 1;
    if (tid == 0) {
      int m = nl > 0 ? S.len[0] : 0;
      for (int w = 1; w < nl; ++w) m = m < S.len[w] ? m : S.len[w];
      if constexpr (MODE == RING) { m -= cc; m = m < 0 ? 0 : (m > TO ? TO : m); }
      *common = m;
    }
    __syncthreads();                                   // tokens of all beams written, *common set
    const int m = *common;
    for (int k = tid; k < m; k += NT) {
      const int c = tok[k];
      bool same = true;
      for (int w = 1; w < nl; ++w) same = same && tok[(size_t)w * TO + k] == c;
      if (!same) atomicMin(common, k);
    }
    __syncthreads();
    if (tid == 0) {
      a.stable_len[b] = *common + cc;
      if constexpr (MODE == RING) { int* info = a.info + 4 * b; info[0] = base; info[1] = cc; info[2] = rg[2]; info[3] = rg[3]; }
    }
  }
}

__global__ __launch_bounds__(64) void ngram_rows_kernel(avec_ngram_t lm, const int* ctx, const int* ctx_len, int max_len, float oov, float* rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  float* row = (float*)sm;
  const int i = blockIdx.x, lane = threadIdx.x, V = lm.V, K = lm.order - 1;
  int n = ctx_len[i]; n = n < 0 ? 0 : (n > max_len ? max_len : n);
  const int clen = n < K ? n : K;
  build_row(lm, ctx + (size_t)i * max_len + (n - clen), 1, clen, oov, row, V, lane);
  for (int c = lane; c < V; c += 64) rows[(size_t)i * V + c] = row[c];
}

int check_lm(const avec_ngram_t* lm, int V) {
  AVEC_CHECK_ARG(lm->order >= 1 && lm->order <= MAXORDER, "ctc_beam: LM order %d (1..%d)", lm->order, MAXORDER);
  AVEC_CHECK_ARG(lm->V == V && lm->unigram, "ctc_beam: LM built for V=%d, decoding V=%d (or no unigram row)", lm->V, V);
  AVEC_CHECK_ARG(lm->ctx_cap >= 0 && (lm->ctx_cap & (lm->ctx_cap - 1)) == 0, "ctc_beam: ctx_cap %lld is not a power of two", lm->ctx_cap);
  AVEC_CHECK_ARG(lm->ctx_cap == 0 || (lm->ctx_key && lm->ctx_bo && lm->ctx_off && lm->ctx_cnt && lm->cont_tok && lm->cont_lp), "ctc_beam: null LM table");
  return 0;
}

template <int MODE>
int launch_beam(const BeamArgs& a, bool lm, int B, hipStream_t st) {
  const size_t bytes = lay(a.W, a.V, lm).total;
  if (lm) {
    if (int r = avec_lds_optin(ctc_beam_kernel<true, MODE>, bytes)) return r;
    hipLaunchKernelGGL((ctc_beam_kernel<true, MODE>), dim3(B), dim3(NT), bytes, st, a);
  } else {
    if (int r = avec_lds_optin(ctc_beam_kernel<false, MODE>, bytes)) return r;
    hipLaunchKernelGGL((ctc_beam_kernel<false, MODE>), dim3(B), dim3(NT), bytes, st, a);
  }
  AVEC_LAUNCH_CHECK(); return 0;
}
}  // namespace

extern "C" long long avec_ctc_beam_workspace_bytes(int B, int T, int W) { return (long long)B * T * W * 4; }

extern "C" int avec_ctc_beam_search(const float* logits, const long long* lengths, int B, int T, int V, int W, float inv_tmp, const avec_ngram_t* lm, float alpha,
                                    float beta, float oov_logprob, void* workspace, long long workspace_bytes, int* tokens, int* out_len, float* score, float* ctc_logp,
                                    hipStream_t st) {
  AVEC_CHECK_ARG(logits && lengths && tokens && out_len && score && ctc_logp && workspace, "ctc_beam_search: null pointer");
  AVEC_CHECK_ARG(B >= 1 && T >= 1 && V >= 2 && V <= MAXV && W >= 1 && W <= MAXW, "ctc_beam_search: bad dims B=%d T=%d V=%d W=%d (V <= %d, W <= %d)", B, T, V, W, MAXV, MAXW);
  AVEC_CHECK_ARG(workspace_bytes >= avec_ctc_beam_workspace_bytes(B, T, W), "ctc_beam_search: workspace of %lld bytes, need %lld", workspace_bytes,
                 avec_ctc_beam_workspace_bytes(B, T, W));
  AVEC_CHECK_ARG(inv_tmp > 0.f, "ctc_beam_search: 1/tmp must be > 0");
  BeamArgs a;
  a.logits = logits; a.lengths = lengths; a.T = T; a.V = V; a.W = W; a.inv_tmp = inv_tmp;
  a.lm = avec_ngram_t{}; a.alpha = alpha; a.beta = beta; a.oov = oov_logprob;
  a.bp = (int*)workspace; a.tokens = tokens; a.out_len = out_len; a.score = score; a.ctc_logp = ctc_logp;
  if (lm) { if (int r = check_lm(lm, V)) return r; a.lm = *lm; }
  a.Tcap = T; a.emit = 1; a.reset = nullptr; a.state = nullptr; a.stable_len = nullptr;
  a.log = nullptr; a.log_frames = 0; a.frames = nullptr; a.info = nullptr;
  return launch_beam<OFFLINE>(a, lm != nullptr, B, st);
}

extern "C" long long avec_ctc_beam_state_bytes(int B, int W) { return (long long)B * (long long)state_stride(W); }

extern "C" int avec_ctc_beam_stream(const float* logits, const long long* chunk_len, const unsigned char* reset, int B, int Tc, int V, int W, int Tcap, float inv_tmp,
                                    const avec_ngram_t* lm, float alpha, float beta, float oov_logprob, void* state, long long state_bytes, void* backptr,
                                    long long backptr_bytes, int* tokens, int* out_len, float* score, float* ctc_logp, int* stable_len, int emit, hipStream_t st) {
  AVEC_CHECK_ARG(logits && state && backptr, "ctc_beam_stream: null pointer");
  AVEC_CHECK_ARG(!emit || (tokens && out_len && score && ctc_logp && stable_len), "ctc_beam_stream: null output with emit set");
  AVEC_CHECK_ARG(B >= 1 && Tc >= 1 && Tcap >= 1 && V >= 2 && V <= MAXV && W >= 1 && W <= MAXW,
                 "ctc_beam_stream: bad dims B=%d Tc=%d Tcap=%d V=%d W=%d (Tc >= 1, Tcap >= 1, V <= %d, W <= %d)", B, Tc, Tcap, V, W, MAXV, MAXW);
  AVEC_CHECK_ARG(state_bytes >= avec_ctc_beam_state_bytes(B, W), "ctc_beam_stream: state of %lld bytes, need %lld", state_bytes, avec_ctc_beam_state_bytes(B, W));
  AVEC_CHECK_ARG(backptr_bytes >= avec_ctc_beam_workspace_bytes(B, Tcap, W), "ctc_beam_stream: backpointers of %lld bytes, need %lld", backptr_bytes,
                 avec_ctc_beam_workspace_bytes(B, Tcap, W));
  AVEC_CHECK_ARG(((size_t)state & 15) == 0, "ctc_beam_stream: the state must be 16-byte aligned");
  AVEC_CHECK_ARG(inv_tmp > 0.f, "ctc_beam_stream: 1/tmp must be > 0");
  BeamArgs a;
  a.logits = logits; a.lengths = chunk_len; a.T = Tc; a.V = V; a.W = W; a.inv_tmp = inv_tmp;
  a.lm = avec_ngram_t{}; a.alpha = alpha; a.beta = beta; a.oov = oov_logprob;
  a.bp = (int*)backptr; a.tokens = tokens; a.out_len = out_len; a.score = score; a.ctc_logp = ctc_logp;
  a.Tcap = Tcap; a.emit = emit; a.reset = reset; a.state = (unsigned char*)state; a.stable_len = stable_len;
  a.log = nullptr; a.log_frames = 0; a.frames = nullptr; a.info = nullptr;
  if (lm) { if (int r = check_lm(lm, V)) return r; a.lm = *lm; }
  return launch_beam<STREAMING>(a, lm != nullptr, B, st);
}

extern "C" long long avec_ctc_beam_ring_state_bytes(int B, int W) { return (long long)B * (long long)ring_state_stride(W); }
extern "C" long long avec_ctc_beam_ring_workspace_bytes(int B, int window, int W) { return (long long)B * window * W * 4; }

extern "C" int avec_ctc_beam_stream_ring(const float* logits, const long long* chunk_len, const unsigned char* reset, int B, int Tc, int V, int W, int window, int log_frames,
                                         float inv_tmp, const avec_ngram_t* lm, float alpha, float beta, float oov_logprob, void* state, long long state_bytes, void* backptr,
                                         long long backptr_bytes, void* log, long long log_bytes, int* tokens, int* frames, int* out_len, float* score, float* ctc_logp,
                                         int* stable_len, int* info, int emit, hipStream_t st) {
  AVEC_CHECK_ARG(logits && state && backptr && log, "ctc_beam_stream_ring: null pointer");
  AVEC_CHECK_ARG(!emit || (tokens && frames && out_len && score && ctc_logp && stable_len && info), "ctc_beam_stream_ring: null output with emit set");
  AVEC_CHECK_ARG(B >= 1 && Tc >= 1 && window >= 2 && log_frames >= 1 && V >= 2 && V <= MAXV && W >= 1 && W <= MAXW,
                 "ctc_beam_stream_ring: bad dims B=%d Tc=%d window=%d log_frames=%d V=%d W=%d (Tc >= 1, window >= 2, log_frames >= 1, V <= %d, W <= %d)", B, Tc, window,
                 log_frames, V, W, MAXV, MAXW);
  AVEC_CHECK_ARG(state_bytes >= avec_ctc_beam_ring_state_bytes(B, W), "ctc_beam_stream_ring: state of %lld bytes, need %lld", state_bytes,
                 avec_ctc_beam_ring_state_bytes(B, W));
  AVEC_CHECK_ARG(backptr_bytes >= avec_ctc_beam_ring_workspace_bytes(B, window, W), "ctc_beam_stream_ring: backpointers of %lld bytes, need %lld", backptr_bytes,
                 avec_ctc_beam_ring_workspace_bytes(B, window, W));
  AVEC_CHECK_ARG(log_bytes >= (long long)B * log_frames * 8, "ctc_beam_stream_ring: commit log of %lld bytes, need %lld", log_bytes, (long long)B * log_frames * 8);
  AVEC_CHECK_ARG(((size_t)state & 15) == 0, "ctc_beam_stream_ring: the state must be 16-byte aligned");
  AVEC_CHECK_ARG(((size_t)log & 7) == 0, "ctc_beam_stream_ring: the commit log must be 8-byte aligned");
  AVEC_CHECK_ARG(inv_tmp > 0.f, "ctc_beam_stream_ring: 1/tmp must be > 0");
  BeamArgs a;
  a.logits = logits; a.lengths = chunk_len; a.T = Tc; a.V = V; a.W = W; a.inv_tmp = inv_tmp;
  a.lm = avec_ngram_t{}; a.alpha = alpha; a.beta = beta; a.oov = oov_logprob;
  a.bp = (int*)backptr; a.tokens = tokens; a.out_len = out_len; a.score = score; a.ctc_logp = ctc_logp;
  a.Tcap = window; a.emit = emit; a.reset = reset; a.state = (unsigned char*)state; a.stable_len = stable_len;
  a.log = (int2*)log; a.log_frames = log_frames; a.frames = frames; a.info = info;
  if (lm) { if (int r = check_lm(lm, V)) return r; a.lm = *lm; }
  return launch_beam<RING>(a, lm != nullptr, B, st);
}

extern "C" int avec_ngram_rows(const avec_ngram_t* lm, const int* ctx, const int* ctx_len, int n, int max_len, float oov_logprob, float* rows, hipStream_t st) {
  AVEC_CHECK_ARG(lm && ctx && ctx_len && rows && n >= 1 && max_len >= 1, "ngram_rows: bad arguments");
  AVEC_CHECK_ARG(lm->V >= 1 && lm->V <= MAXV, "ngram_rows: V=%d (<= %d)", lm->V, MAXV);
  if (int r = check_lm(lm, lm->V)) return r;
  hipLaunchKernelGGL(ngram_rows_kernel, dim3(n), dim3(64), (size_t)lm->V * 4, st, *lm, ctx, ctx_len, max_len, oov_logprob, rows);
  AVEC_LAUNCH_CHECK(); return 0;
}
