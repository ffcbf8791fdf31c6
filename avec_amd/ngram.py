"""N-gram language models for the CTC beam search (avec_amd/csrc/ctc_beam.hip): an ARPA parser, the device tables of `avec_ngram_t`
(include/avec_hip.h) built with numpy, and `NGramLM`, which holds them on the host and uploads them to a device on first use.

Token k of the acoustic model is the ARPA word chr(k + offset), as the reference names its labels (nnet/decoders.py:187).  ARPA values are log10;
the tables hold natural logs.  Lines that name a word which is neither `<s>` (first position only) nor a token word (one character, id < V) are
dropped and counted, as are n-grams that name a token which is not among the unigrams (`<unk>` and `</s>` are such words: there is no end-of-sentence
term, and an out-of-vocabulary token costs the fixed `oov_logprob` instead of `<unk>`'s probability)."""
import math
import warnings

import numpy as np

LN10 = math.log(10.0)
BOS = -1                  # <s> in a context tuple
MAX_ORDER = 8
_C1, _C2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xC2B2AE3D27D4EB4F)


def _mix64(x):
    """splitmix64 finaliser on a uint64 array (the device's mix64)"""
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def pack_contexts(ctx):
    """int [m, L] contexts (oldest first, -1 = <s>, L <= 7) -> (lo, hi) uint64 keys: code = token + 1 (0xFFFF for <s>) at bits 16 j"""
    ctx = np.asarray(ctx, dtype=np.int64).reshape(len(ctx), -1)
    codes = np.where(ctx < 0, 0xFFFF, ctx + 1).astype(np.uint64)
    lo, hi = np.zeros(len(ctx), np.uint64), np.zeros(len(ctx), np.uint64)
    for j in range(ctx.shape[1]):
        if j < 4:
            lo |= codes[:, j] << np.uint64(16 * j)
        else:
            hi |= codes[:, j] << np.uint64(16 * (j - 4))
    return lo, hi


def context_slot(lo, hi, cap):
    with np.errstate(over="ignore"):
        return (_mix64((lo * _C1) ^ (hi * _C2)) & np.uint64(cap - 1)).astype(np.int64)


class Arpa:
    """A parsed ARPA file restricted to a vocabulary: grams[n] = (tokens [m, n] int32 (-1 = <s>), log10 p [m], log10 backoff [m] (NaN = absent))"""

    def __init__(self, order, counts, grams, dropped):
        self.order, self.counts, self.grams, self.dropped = order, counts, grams, dropped

    def entries(self):
        """{token tuple: (log10 p, log10 backoff or None)}"""
        out = {}
        for n, (tok, lp, bo) in self.grams.items():
            for t, p, b in zip(tok.tolist(), lp.tolist(), bo.tolist()):
                out[tuple(t)] = (p, None if math.isnan(b) else b)
        return out

    @property
    def n_unigrams(self):
        tok = self.grams.get(1, (np.zeros((0, 1), np.int32),))[0]
        return int((tok[:, 0] >= 0).sum())


def parse_arpa(path, vocab_size, offset=100):
    """ARPA text -> Arpa: `\\data\\` counts, `\\k-grams:` sections (optional backoff column), blank lines, `\\end\\`."""
    tokmap = {chr(k + offset): k for k in range(vocab_size)}
    tokmap["<s>"] = BOS
    counts, lists, dropped, n = {}, {}, 0, 0
    with open(path, encoding="utf-8", errors="replace") as f:
        for line in f:
            if line[:1] == "\\":
                head = line.strip()
                if head == "\\data\\":
                    n = 0
                elif head == "\\end\\":
                    break
                elif head.endswith("-grams:"):
                    n = int(head[1:-7])
                    lists.setdefault(n, ([], [], []))
                continue
            f_ = [x for x in line.rstrip("\r\n").replace("\t", " ").split(" ") if x]     # ASCII separators only: token words such as
            if not f_:                                                                   # chr(133) and chr(160) are Unicode whitespace
                continue
            if n == 0:
                if f_[0] == "ngram" and "=" in line:
                    k, c = line.split("ngram", 1)[1].split("=")
                    counts[int(k)] = int(c)
                continue
            ids = [tokmap.get(w) for w in f_[1:1 + n]]
            if len(ids) < n or None in ids or BOS in ids[1:]:
                dropped += 1
                continue
            toks, lps, bos = lists[n]
            toks.append(ids)
            lps.append(float(f_[0]))
            bos.append(float(f_[1 + n]) if len(f_) > 1 + n else math.nan)
    grams = {}
    for k, (toks, lps, bos) in lists.items():
        grams[k] = (np.array(toks, dtype=np.int32).reshape(-1, k), np.array(lps, dtype=np.float64), np.array(bos, dtype=np.float64))
    order = max([k for k in counts] + [k for k in grams] + [1])
    known = np.zeros(vocab_size + 1, bool)                     # index -1 (<s>) -> the last slot, always "known"
    known[-1] = True
    if 1 in grams:
        known[grams[1][0][grams[1][0][:, 0] >= 0, 0]] = True
    for k in list(grams):
        tok, lp, bo = grams[k]
        ok = known[tok].all(axis=1)
        dropped += int((~ok).sum())
        grams[k] = (tok[ok], lp[ok], bo[ok])
    return Arpa(order, counts, grams, dropped)


class NGramLM:
    """An n-gram LM as the beam search's device tables.  Construction parses and builds on the host only; `device_struct` uploads on first use.

    usable is False when the file has no unigram that names a token: the decoder then runs without an LM."""

    def __init__(self, path, vocab_size, offset=100, oov_logprob=-1000.0):
        self.path, self.V, self.offset, self.oov_logprob = path, int(vocab_size), offset, float(oov_logprob)
        self.arpa = parse_arpa(path, self.V, offset)
        self.order, self.dropped = self.arpa.order, self.arpa.dropped
        if self.order > MAX_ORDER:
            raise ValueError("NGramLM: order %d > %d (the beam search's limit)" % (self.order, MAX_ORDER))
        self.usable = self.arpa.n_unigrams > 0
        self._build()
        self._dev = {}

    def _build(self):
        g, V, K = self.arpa.grams, self.V, self.order - 1
        uni = np.full(V, -np.inf, np.float64)
        if 1 in g:
            tok, lp, _ = g[1]
            m = tok[:, 0] >= 0
            uni[tok[m, 0]] = lp[m] * LN10
        self.unigram = uni.astype(np.float32)
        # contexts: every n-gram of order <= K (its backoff) and every prefix of an n-gram of order >= 2 (its continuations)
        keys, bo_of, conts = [], [], []
        for n in range(1, K + 1):
            if n in g and len(g[n][0]):
                lo, hi = pack_contexts(g[n][0])
                keys.append(np.stack([lo, hi], 1))
                bo_of.append((len(keys) - 1, np.nan_to_num(g[n][2], nan=0.0) * LN10))
        for n in range(2, self.order + 1):
            if n in g and len(g[n][0]):
                tok, lp, _ = g[n]
                lo, hi = pack_contexts(tok[:, :-1])
                keys.append(np.stack([lo, hi], 1))
                conts.append((len(keys) - 1, tok[:, -1].astype(np.int64), lp * LN10))
        if not keys:
            self.ctx_cap, self.n_contexts = 0, 0
            self.ctx_key = np.zeros((0, 2), np.uint64)
            self.ctx_bo, self.ctx_off, self.ctx_cnt = np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32)
            self.cont_tok, self.cont_lp = np.zeros(0, np.int32), np.zeros(0, np.float32)
            return
        sizes = [len(k) for k in keys]
        starts = np.cumsum([0] + sizes)
        uniq, inv = np.unique(np.concatenate(keys), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        nctx = len(uniq)
        bo = np.zeros(nctx, np.float64)
        for i, v in bo_of:
            bo[inv[starts[i]:starts[i + 1]]] = v
        if conts:
            cid = np.concatenate([inv[starts[i]:starts[i + 1]] for i, _, _ in conts])
            ctok = np.concatenate([t for _, t, _ in conts])
            clp = np.concatenate([p for _, _, p in conts])
            o = np.lexsort((ctok, cid))                        # by context, then token (stable: the first of duplicate lines wins)
            cid, ctok, clp = cid[o], ctok[o], clp[o]
            keep = np.ones(len(cid), bool)
            keep[1:] = (cid[1:] != cid[:-1]) | (ctok[1:] != ctok[:-1])
            cid, ctok, clp = cid[keep], ctok[keep], clp[keep]
        else:
            cid, ctok, clp = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
        cnt = np.bincount(cid, minlength=nctx)
        off = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        # open addressing, linear probing, load <= 0.5; a key that finds its home slot taken moves on by one slot per round
        cap = 2
        while cap < 2 * nctx:
            cap *= 2
        slot_of = np.full(cap, -1, np.int64)
        pos = context_slot(uniq[:, 0], uniq[:, 1], cap)
        pending = np.arange(nctx)
        while len(pending):
            p = pos[pending]
            free = np.flatnonzero(slot_of[p] < 0)
            u, first = np.unique(p[free], return_index=True)
            slot_of[u] = pending[free[first]]
            won = np.zeros(len(pending), bool)
            won[free[first]] = True
            pending = pending[~won]
            pos[pending] = (pos[pending] + 1) & (cap - 1)
        filled = slot_of >= 0
        src = slot_of[filled]
        self.ctx_cap, self.n_contexts = cap, nctx
        self.ctx_key = np.zeros((cap, 2), np.uint64)
        self.ctx_key[filled] = uniq[src]
        self.ctx_bo = np.zeros(cap, np.float32)
        self.ctx_bo[filled] = bo[src]
        self.ctx_off = np.zeros(cap, np.int32)
        self.ctx_off[filled] = off[src]
        self.ctx_cnt = np.zeros(cap, np.int32)
        self.ctx_cnt[filled] = cnt[src]
        self.cont_tok, self.cont_lp = ctok.astype(np.int32), clp.astype(np.float32)

    # ---- host mirror of the device row builder (build_row in ctc_beam.hip), fp64 over the fp32 tables ----
    def _find(self, ctx):
        if self.ctx_cap == 0:
            return None
        lo, hi = pack_contexts(np.array([ctx]))
        h = int(context_slot(lo, hi, self.ctx_cap)[0])
        for _ in range(self.ctx_cap):
            k = self.ctx_key[h]
            if k[0] == lo[0] and k[1] == hi[0]:
                return h
            if k[0] == 0 and k[1] == 0:
                return None
            h = (h + 1) & (self.ctx_cap - 1)
        return None

    def row(self, ctx):
        """ln P(. | ctx) [V] (fp64): ctx = token history oldest first, -1 = <s>; only its last order-1 tokens count"""
        K = self.order - 1
        ctx = list(ctx)[len(ctx) - min(len(ctx), K):] if K > 0 else []
        found = [self._find(ctx[len(ctx) - s:]) for s in range(1, len(ctx) + 1)]
        bos = [float(self.ctx_bo[h]) if h is not None else 0.0 for h in found]
        tot = sum(bos)
        uni = self.unigram.astype(np.float64)
        row = np.where(np.isneginf(uni), self.oov_logprob, uni + tot)
        sfx = tot
        for h, b in zip(found, bos):
            sfx -= b
            if h is not None:
                o, c = int(self.ctx_off[h]), int(self.ctx_cnt[h])
                row[self.cont_tok[o:o + c]] = self.cont_lp[o:o + c].astype(np.float64) + sfx
        return row

    # ---- device ----
    def device_struct(self, device):
        """the avec_ngram_t of this LM on `device` (tables uploaded on the first call per device and kept)"""
        import torch
        from .lib import NGram
        key = str(torch.device(device))
        if key not in self._dev:
            def up(a):
                return torch.from_numpy(np.ascontiguousarray(a)).to(device) if a.size else None
            keep = [up(self.unigram), up(self.ctx_key.view(np.int64)), up(self.ctx_bo), up(self.ctx_off), up(self.ctx_cnt), up(self.cont_tok),
                    up(self.cont_lp)]
            ptr = [t.data_ptr() if t is not None else None for t in keep]
            st = NGram(self.order, self.V, ptr[0], self.ctx_cap, ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ptr[6])
            self._dev[key] = (st, keep)
        return self._dev[key][0]


def load(path, vocab_size, offset=100, oov_logprob=-1000.0):
    """NGramLM, or None with a warning when the file is missing or has no usable unigram"""
    import os
    if not path or not os.path.exists(path):
        warnings.warn("n-gram LM %r not found: beam search without an LM" % (path,))
        return None
    lm = NGramLM(path, vocab_size, offset, oov_logprob)
    if not lm.usable:
        warnings.warn("n-gram LM %r has no unigram that names a token: beam search without an LM (alpha = beta = 0)" % (path,))
        return None
    return lm
