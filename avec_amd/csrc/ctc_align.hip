// CTC forced alignment: the Viterbi (best) path of a GIVEN label sequence through the CTC trellis of logits [B][T][V], with the frame span and the log-probability
// of every target token (token / word timestamps for the decoders of nnet/decoders.py; no ATen op and no kernel of loss_optim.hip computes a best path).
//
// One workgroup of 4 waves aligns one utterance; S = 2 L + 1 extended states (blank, y1, blank, ..., yL, blank).
//   check    targets inside tgt_len are validated (not blank, inside [0, V)) before any of them is used as an index, adjacent repeats are counted:
//            in_len < L + repeats or an invalid target -> the sentinel outputs (score -inf, path / spans -1, token_logp 0) and nothing else runs
//   phase A  frame normalisers lse[t] = logsumexp(logits[t]), one frame per wave and eight frames per wave in flight; the same wave then gathers the emissions
//            E[t][s] = logits[t][ext[s]] - lse[t] of its eight frames (rows it has just read), eight independent loads per lane before the eight stores
//   phase B  delta_t[s] = max(delta_{t-1}[s], delta_{t-1}[s-1], delta_{t-1}[s-2] if allowed) + E[t][s] in fp32: state s = tid, tid + 256, ... (any Lmax), two
//            delta rows in LDS, ONE barrier per frame, a branch-free step (written with branches it waited for five LDS reads one after the other); the emissions of frame t + 1 of a thread's first two states are loaded before the work of frame t so that
//            their latency is off the chain.  The 2-bit backpointer (0 stay, 1 from s-1, 2 from s-2) of the 64 states a wave handles in one pass is packed by two
//            ballots into four 32-bit words {bit0 lo, bit0 hi, bit1 lo, bit1 hi}: BP[t][s / 64][4], one 16-byte store by lane 0
//   phase C  wave 0 walks the backpointers: per window of 32 frames the 64 lanes fetch the words of the two 64-state chunks the walk can reach (it moves down by
//            at most 2 states a frame) with ONE 16-byte load each, and the 32 steps run on v_readlane with the state in a scalar register: T / 32 dependent
//            memory round trips instead of T
//   phase D  all threads: path[t] = ext[state[t]], the span of every token (first frame, last frame + 1 of its state), token_logp = sum of E over its frames
//            in frame order, score = delta at the end state
// Tie rule (both tiers, the oracle of tests/ctc_align_oracle.py): the predecessor of s is s unless delta[s-1] is STRICTLY greater, s-2 only if strictly greater
// than the winner of those two (and only when ext[s] != blank && ext[s] != ext[s-2]); the end state is S-1 unless delta[S-2] is strictly greater.
// Tier 1 keeps E and BP in LDS (T * (2 Lmax + 1) * 4 + T * ceil((2 Lmax + 1) / 64) * 16 bytes plus the small arrays, up to 160 KB: avec_ctc_align_fits_lds);
// tier 2 keeps them in the caller's workspace (15 s clips: T = 376, Lmax = 130 is 393 KB of emissions).  The code is the same template, so the two tiers do the
// same fp32 operations in the same order and agree bit for bit.
#include "common.h"
#include "avec_hip.h"

namespace {
constexpr int NT = 256, NW = NT / 64, FR = 8, WIN = 32;
constexpr size_t LDS_MAX = 160 * 1024;

__host__ __device__ inline size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }
struct Lay { size_t ext, delta, spath, span, misc, bp, emis, total; };
__host__ __device__ inline size_t bp_bytes(int T, int Lmax) { return (size_t)T * ((2 * (size_t)Lmax + 1 + 63) / 64) * 16; }
__host__ __device__ inline size_t emis_bytes(int T, int Lmax) { return a16((size_t)T * (2 * (size_t)Lmax + 1) * 4); }
__host__ __device__ inline Lay lay(int T, int Lmax, bool all_lds) {
  const size_t S = 2 * (size_t)Lmax + 1;
  Lay L; size_t o = 0;
  L.ext = o; o = a16(o + S * 4);
  L.delta = o; o = a16(o + 2 * (S + 2) * 4);
  L.spath = o; o = a16(o + (size_t)T * 4);
  L.span = o; o = a16(o + 2 * (size_t)(Lmax > 0 ? Lmax : 1) * 4);
  L.misc = o; o += 16;
  L.bp = o; if (all_lds) o += bp_bytes(T, Lmax);
  L.emis = o; if (all_lds) o += emis_bytes(T, Lmax);
  L.total = o;
  return L;
}
inline size_t ws_per_utt(int T, int Lmax) { return bp_bytes(T, Lmax) + emis_bytes(T, Lmax); }

struct AlignArgs {
  const float* logits; const long long* in_lens; const long long* targets; const long long* tgt_lens; int T, V, Lmax, blank;
  unsigned char* ws; size_t ws_per_utt;
  int* path; int* spans; float* score; float* token_logp;
};

template <bool ALL_LDS>
__global__ __launch_bounds__(NT) void ctc_align_kernel(AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int T = a.T, V = a.V, Lmax = a.Lmax, blank = a.blank, Smax = 2 * Lmax + 1, NC = (Smax + 63) >> 6;
  const Lay Y = lay(T, Lmax, ALL_LDS);
  int* ext = (int*)(sm + Y.ext); float* delta = (float*)(sm + Y.delta);
  int* spath = (int*)(sm + Y.spath); int* span = (int*)(sm + Y.span); int* misc = (int*)(sm + Y.misc);
  unsigned* bp; float* E;
  if constexpr (ALL_LDS) { bp = (unsigned*)(sm + Y.bp); E = (float*)(sm + Y.emis); }
  else { unsigned char* w = a.ws + (size_t)b * a.ws_per_utt; bp = (unsigned*)w; E = (float*)(w + bp_bytes(T, Lmax)); }
  const long long il = a.in_lens[b], tl = a.tgt_lens[b];
  const int Tb = il < 0 ? 0 : (il > T ? T : (int)il), L = tl < 0 ? 0 : (tl > Lmax ? Lmax : (int)tl), S = 2 * L + 1;
  const float* lg = a.logits + (size_t)b * T * V;
  int* path = a.path + (size_t)b * T; int* spans = a.spans + (size_t)b * Lmax * 2; float* tlp = a.token_logp + (size_t)b * Lmax;

  auto no_alignment = [&](float sc) {
    for (int t = tid; t < T; t += NT) path[t] = -1;
    for (int i = tid; i < Lmax; i += NT) { spans[2 * i] = -1; spans[2 * i + 1] = -1; tlp[i] = 0.f; }
    if (tid == 0) a.score[b] = sc;
  };

  // ---- check: a target becomes an index only after it was found valid
  if (tid == 0) { misc[0] = 0; misc[1] = 0; }
  __syncthreads();
  {
    const long long* tg = a.targets + (size_t)b * Lmax;
    int bad = 0, rep = 0;
    for (int i = tid; i < L; i += NT) {
      const long long c = tg[i];
      if (c == blank || c < 0 || c >= V) bad = 1; else ext[2 * i + 1] = (int)c;
      if (i > 0 && c == tg[i - 1]) ++rep;
      span[2 * i] = 0; span[2 * i + 1] = 0;
    }
    for (int i = tid; i <= L; i += NT) ext[2 * i] = blank;
    if (rep) atomicAdd(misc, rep);
    if (bad) misc[1] = 1;
    __syncthreads();
    if (misc[1] || Tb < L + misc[0]) { no_alignment(-INFINITY); return; }
  }
  if (Tb == 0) { no_alignment(0.f); return; }            // (then L == 0: the empty path)

  for (int k = tid; k < 2 * (Smax + 2); k += NT) delta[k] = k == (Smax + 2) + 2 ? 0.f : -INFINITY;      // (visible after phase A's barrier)

  // ---- phase A
  for (int t0 = wv * FR; t0 < Tb; t0 += FR * NW) {
    float mx[FR], se[FR];
#pragma unroll
    for (int q = 0; q < FR; ++q) { const int t = min(t0 + q, Tb - 1); mx[q] = -INFINITY; for (int v = lane; v < V; v += 64) mx[q] = fmaxf(mx[q], lg[(size_t)t * V + v]); }
#pragma unroll
    for (int q = 0; q < FR; ++q) mx[q] = wave_max(mx[q]);
#pragma unroll
    for (int q = 0; q < FR; ++q) { const int t = min(t0 + q, Tb - 1); se[q] = 0.f; for (int v = lane; v < V; v += 64) se[q] += expf(lg[(size_t)t * V + v] - mx[q]); }
#pragma unroll
    for (int q = 0; q < FR; ++q) se[q] = wave_sum(se[q]);
    float ls[FR];
#pragma unroll
    for (int q = 0; q < FR; ++q) ls[q] = mx[q] + logf(se[q]);
    for (int s = lane; s < S; s += 64) {               // the emissions of these frames while their rows are warm: FR independent loads, then FR stores
      const int k = ext[s];
      float v[FR];
#pragma unroll
      for (int q = 0; q < FR; ++q) v[q] = lg[(size_t)min(t0 + q, Tb - 1) * V + k];
#pragma unroll
      for (int q = 0; q < FR; ++q) if (t0 + q < Tb) E[(size_t)(t0 + q) * Smax + s] = v[q] - ls[q];
    }
  }
  __syncthreads();

  // ---- phase B.  A delta row has two -inf entries in front, so that s-1 and s-2 are always there, and the row "before frame 0" is {0, -inf, ...}: every frame is
  // the same branch-free step (three LDS reads in flight together, selects); delta_0[s] = 0 + E[0][s] for s < 2 and -inf above, as the definition says
  float* const row0 = delta + 2; float* const row1 = delta + (Smax + 2) + 2;
  {
    const int sA = tid, sB = tid + NT;
    auto skip_ok = [&](int s) { return s >= 2 && s < S && ext[s] != blank && ext[s] != ext[s - 2]; };
    const bool okA = skip_ok(sA), okB = skip_ok(sB);
    float enA = sA < S ? E[sA] : 0.f, enB = sB < S ? E[sB] : 0.f;
    for (int t = 0; t < Tb; ++t) {
      const float* dp = (t & 1) ? row0 : row1; float* dn = (t & 1) ? row1 : row0;
      const float ecA = enA, ecB = enB;
      if (t + 1 < Tb) {
        if (sA < S) enA = E[(size_t)(t + 1) * Smax + sA];
        if (sB < S) enB = E[(size_t)(t + 1) * Smax + sB];
      }
      unsigned* bpt = bp + (size_t)t * NC * 4;
      auto step = [&](int c, float e, bool ok) {        // the 64 states of chunk c: one per lane
        const int s = c * 64 + lane; const bool in = s < S; const int sr = in ? s : S - 1;
        const float a = dp[sr], b1 = dp[sr - 1], c2 = dp[sr - 2];
        float best = a; int code = 0;
        if (b1 > best) { best = b1; code = 1; }
        if (ok && c2 > best) { best = c2; code = 2; }
        if (in) dn[s] = best + e; else code = 0;
        const unsigned long long m0 = __ballot(code & 1), m1 = __ballot(code & 2);
        if (lane == 0) *(uint4*)(bpt + c * 4) = make_uint4((unsigned)m0, (unsigned)(m0 >> 32), (unsigned)m1, (unsigned)(m1 >> 32));
      };
      if (wv * 64 < S) step(wv, ecA, okA);
      if ((wv + NW) * 64 < S) step(wv + NW, ecB, okB);
      for (int c = wv + 2 * NW; c * 64 < S; c += NW) { const int s = c * 64 + lane; step(c, s < S ? E[(size_t)t * Smax + s] : 0.f, skip_ok(s)); }
      __syncthreads();
    }
  }
  const float* dl = ((Tb - 1) & 1) ? row1 : row0;
  float fin = dl[S - 1]; int send = S - 1;
  if (S > 1 && dl[S - 2] > fin) { fin = dl[S - 2]; send = S - 2; }
  if (!(fin > -INFINITY)) { no_alignment(-INFINITY); return; }      // (-inf or NaN logits: no path of finite probability)

  // ---- phase C
  if (wv == 0) {
    int s = __builtin_amdgcn_readfirstlane(send);
    for (int t0 = Tb - 1; t0 >= 0; t0 -= WIN) {
      const int c = s >> 6;                              // within WIN = 32 frames the walk stays inside chunks c and c - 1
      const int tf = t0 - (lane & 31), cc = c - (lane >> 5);
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      if (tf >= 1 && cc >= 0) w = *(const uint4*)(bp + ((size_t)tf * NC + cc) * 4);
      const int nf = t0 + 1 < WIN ? t0 + 1 : WIN;
      for (int k = 0; k < nf; ++k) {
        const int t = t0 - k;
        if (lane == 0) spath[t] = s;
        if (t == 0) break;
        const int src = k + ((s >> 6) == c ? 0 : 32), bit = s & 31;
        const bool hi = (s & 32) != 0;
        const unsigned b0 = (unsigned)__builtin_amdgcn_readlane((int)(hi ? w.y : w.x), src), b1 = (unsigned)__builtin_amdgcn_readlane((int)(hi ? w.w : w.z), src);
        s -= (int)((b0 >> bit) & 1u) + 2 * (int)((b1 >> bit) & 1u);
      }
    }
  }
  __syncthreads();

  // ---- phase D
  for (int t = tid; t < T; t += NT) {
    int tok = -1;
    if (t < Tb) {
      const int st = spath[t];
      tok = ext[st];
      if (st & 1) {
        if (t == 0 || spath[t - 1] != st) span[st - 1] = t;
        if (t == Tb - 1 || spath[t + 1] != st) span[st] = t + 1;
      }
    }
    path[t] = tok;
  }
  __syncthreads();
  for (int i = tid; i < Lmax; i += NT) {
    int f0 = -1, f1 = -1; float lp = 0.f;
    if (i < L) {
      f0 = span[2 * i]; f1 = span[2 * i + 1];
      for (int t = max(f0, 0); t < min(f1, Tb); ++t) lp += E[(size_t)t * Smax + 2 * i + 1];
    }
    spans[2 * i] = f0; spans[2 * i + 1] = f1; tlp[i] = lp;
  }
  if (tid == 0) a.score[b] = fin;
}
}  // namespace

extern "C" long long avec_ctc_align_workspace_bytes(int B, int T, int Lmax) {
  if (B < 1 || T < 1 || Lmax < 0) return 0;
  return (long long)((size_t)B * ws_per_utt(T, Lmax));
}

extern "C" int avec_ctc_align_fits_lds(int T, int Lmax) { return T >= 1 && Lmax >= 0 && lay(T, Lmax, true).total <= LDS_MAX; }

extern "C" int avec_ctc_align(const float* logits, const long long* in_lens, const long long* targets, const long long* tgt_lens, int B, int T, int V, int Lmax, int blank,
                              int tier, void* workspace, long long workspace_bytes, int* path, int* spans, float* score, float* token_logp, hipStream_t st) {
  AVEC_CHECK_ARG(logits && in_lens && tgt_lens && path && score && workspace, "ctc_align: null pointer");
  AVEC_CHECK_ARG(B >= 1 && T >= 1 && V >= 1 && Lmax >= 0 && blank >= 0 && blank < V, "ctc_align: bad dims B=%d T=%d V=%d Lmax=%d blank=%d", B, T, V, Lmax, blank);
  AVEC_CHECK_ARG(Lmax == 0 || (targets && spans && token_logp), "ctc_align: null pointer");
  AVEC_CHECK_ARG((long long)T * V <= 0x7fffffffLL && (long long)T * (2 * (long long)Lmax + 1) <= 0x7fffffffLL, "ctc_align: T=%d x V=%d or T x (2 Lmax + 1) (Lmax=%d) beyond 2^31", T, V, Lmax);
  AVEC_CHECK_ARG(tier >= 0 && tier <= 2, "ctc_align: tier %d (0 auto, 1 all-LDS, 2 workspace)", tier);
  AVEC_CHECK_ARG(workspace_bytes >= avec_ctc_align_workspace_bytes(B, T, Lmax), "ctc_align: workspace of %lld bytes, need %lld", workspace_bytes,
                 avec_ctc_align_workspace_bytes(B, T, Lmax));
  AVEC_CHECK_ARG(((size_t)workspace & 15) == 0, "ctc_align: the workspace must be 16-byte aligned");
  const int fits = avec_ctc_align_fits_lds(T, Lmax);
  AVEC_CHECK_ARG(tier != 1 || fits, "ctc_align: tier 1 (all-LDS) does not fit T=%d Lmax=%d (%zu bytes of LDS, %zu at most)", T, Lmax, lay(T, Lmax, true).total, LDS_MAX);
  const size_t lds2 = lay(T, Lmax, false).total;
  AVEC_CHECK_ARG(lds2 <= LDS_MAX, "ctc_align: T=%d Lmax=%d needs %zu bytes of LDS for the state rows (%zu at most)", T, Lmax, lds2, LDS_MAX);
  AlignArgs a;
  a.logits = logits; a.in_lens = in_lens; a.targets = targets; a.tgt_lens = tgt_lens; a.T = T; a.V = V; a.Lmax = Lmax; a.blank = blank;
  a.ws = (unsigned char*)workspace; a.ws_per_utt = ws_per_utt(T, Lmax);
  a.path = path; a.spans = spans; a.score = score; a.token_logp = token_logp;
  if (tier != 2 && fits) {
    const size_t bytes = lay(T, Lmax, true).total;
    // tier 0: a device that refuses the opt-in (remembered by avec_lds_optin) runs the workspace tier instead; tier 1 reports the refusal
    const int r = tier == 1 ? avec_lds_optin(ctc_align_kernel<true>, bytes) : avec_lds_optin_quiet((const void*)ctc_align_kernel<true>, bytes);
    if (r == 0) {
      hipLaunchKernelGGL(ctc_align_kernel<true>, dim3(B), dim3(NT), bytes, st, a);
      AVEC_LAUNCH_CHECK(); return 0;
    }
    if (tier == 1) return r;
  }
  if (int r = avec_lds_optin(ctc_align_kernel<false>, lds2)) return r;
  hipLaunchKernelGGL(ctc_align_kernel<false>, dim3(B), dim3(NT), lds2, st, a);
  AVEC_LAUNCH_CHECK(); return 0;
}
