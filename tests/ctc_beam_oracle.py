"""fp64 reference of the CTC prefix beam search with n-gram LM fusion (avec_amd/csrc/ctc_beam.hip): a dict of prefixes, the same candidate order
(stays in slot order, then extension (i, c) at index W + i V + c; ties to the lower index), and the ARPA backoff definition read straight off a dict of
n-gram entries.  Also random ARPA writers for the tests and tools/bench_beam.py."""
import math
import random

import numpy as np

LN10 = math.log(10.0)
NEG = -math.inf


def lae(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def log_softmax64(logits, tmp=1.0):
    x = np.asarray(logits, dtype=np.float64) / tmp
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


# ---- the ARPA backoff definition over a dict {token tuple (-1 = <s>): (log10 p, log10 bo or None)} ----
def lm_logprob(entries, order, hist, c, oov=-1000.0):
    """ln P(c | hist): hist = <s> + prefix as a token tuple; standard backoff over its last order-1 tokens; a non-unigram token costs `oov`"""
    if (c,) not in entries:
        return oov
    h = tuple(hist)[len(hist) - min(len(hist), order - 1):] if order > 1 else ()

    def rec(h):
        if h + (c,) in entries:
            return entries[h + (c,)][0]
        bo = entries[h][1] if h in entries and entries[h][1] is not None else 0.0
        return bo + rec(h[1:])
    return rec(h) * LN10


class DictLM:
    """the same definition, a whole row ln P(. | hist) at a time (cached per context)"""

    def __init__(self, entries, order, V, oov=-1000.0):
        self.order, self.V, self.oov = order, V, oov
        self.cont, self.bo = {}, {}
        for k, (p, b) in entries.items():
            self.cont.setdefault(k[:-1], {})[k[-1]] = p * LN10
            if b is not None:
                self.bo[k] = b * LN10
        self.known = np.zeros(V, bool)
        for c in self.cont.get((), {}):
            if 0 <= c < V:
                self.known[c] = True
        self.cache = {}

    def _rec(self, h):
        if h in self.cache:
            return self.cache[h]
        if not h:
            row = np.zeros(self.V)
        else:
            row = self._rec(h[1:]) + self.bo.get(h, 0.0)
        for c, p in self.cont.get(h, {}).items():
            if 0 <= c < self.V:
                row[c] = p
        row = row.copy()
        self.cache[h] = row
        return row

    def row(self, hist):
        h = tuple(hist)[len(hist) - min(len(hist), self.order - 1):] if self.order > 1 else ()
        return np.where(self.known, self._rec(h), self.oov)


def beam_search(logp, length, W, lm=None, alpha=0.6, beta=1.0):
    """logp [T, V] fp64 (already log_softmax'ed).  Returns (beams, gap): beams = [(tokens, score, ctc_logp)] best first; gap = the smallest margin,
    over all frames, between the W-th kept score and the best dropped one, and at the last frame also between consecutive kept scores"""
    V = logp.shape[1]
    beams = [((), 0.0, NEG, 0.0)]           # (prefix, pb, pnb, lm)
    gap = math.inf
    for t in range(int(length)):
        lp = logp[t]
        slot = {b[0]: i for i, b in enumerate(beams)}
        stay = []
        for pre, pb, pnb, _ in beams:
            stay.append([lae(pb, pnb) + lp[0], pnb + lp[pre[-1]] if pre else NEG])
        ext_pnb, ext_lm = [], []
        for pre, pb, pnb, lms in beams:
            e = pre[-1] if pre else -1
            base = np.full(V, lae(pb, pnb))
            if e >= 0:
                base[e] = pb
            m = base + lp
            m[0] = NEG
            ext_pnb.append(m)
            ext_lm.append((lms + alpha * lm.row((-1,) + pre) + beta) if lm is not None else np.full(V, lms))
        for j, (pre, _, _, _) in enumerate(beams):
            i = slot.get(pre[:-1]) if pre else None
            if i is not None:                       # extension (i, last) re-creates beam j: its mass joins j's stay
                stay[j][1] = lae(stay[j][1], ext_pnb[i][pre[-1]])
                ext_pnb[i][pre[-1]] = NEG
        n = len(beams)
        cand_s = np.concatenate([np.array([lae(s_[0], s_[1]) + b[3] for s_, b in zip(stay, beams)])] + [m + l for m, l in zip(ext_pnb, ext_lm)])
        cand_i = np.concatenate([np.arange(n), W + (np.arange(n)[:, None] * V + np.arange(V)[None, :]).reshape(-1)])
        live = np.flatnonzero(cand_s > NEG)
        order = live[np.lexsort((cand_i[live], -cand_s[live]))]
        kept = order[:W]
        if len(order) > W:
            gap = min(gap, cand_s[kept[-1]] - cand_s[order[W]])
        nb = []
        for k in kept:
            if k < n:
                pre, _, _, lms = beams[k]
                nb.append((pre, stay[k][0], stay[k][1], lms))
            else:
                i, c = divmod(int(cand_i[k]) - W, V)
                nb.append((beams[i][0] + (c,), NEG, float(ext_pnb[i][c]), float(ext_lm[i][c])))
        beams = nb
    out = [(list(pre), lae(pb, pnb) + lms, lae(pb, pnb)) for pre, pb, pnb, lms in beams]
    for a, b in zip(out, out[1:]):
        gap = min(gap, a[1] - b[1])
    return out, gap


# ---- random inputs ----
def ctc_like_logits(B, T, V, seed, peak=6.0, noise=1.0):
    """a seeded label path with blanks, plus noise: peaked, CTC-shaped frames"""
    g = np.random.default_rng(seed)
    x = noise * g.standard_normal((B, T, V)).astype(np.float32)
    for b in range(B):
        for t in range(T):
            k = 0 if g.random() < 0.4 else int(g.integers(1, V))
            x[b, t, k] += peak
    return x


def write_random_arpa(path, V, order, n_per_order, seed, offset=100, extras=True):
    """A random (not normalised) ARPA file over token words chr(k + offset), k in 1..V-1 (most of them unigrams), with <s>, optional backoffs and,
    with extras, </s>, <unk>, a multi-character word and ids >= V.  Returns (entries for token ids, number of lines the parser must drop)."""
    rnd = random.Random(seed)
    known = [k for k in range(1, V) if rnd.random() < 0.9]
    entries, lines, dropped, lines_ctx = {}, {n: [] for n in range(1, order + 1)}, 0, {}

    def w(k):
        return "<s>" if k == -1 else chr(k + offset)

    def add(n, toks, p, bo):
        lines[n].append("%.6f\t%s%s" % (p, " ".join(w(k) for k in toks), "" if bo is None else "\t%.6f" % bo))
        entries[tuple(toks)] = (float("%.6f" % p), None if bo is None else float("%.6f" % bo))

    for k in known:
        add(1, [k], -rnd.uniform(0.5, 4.0), -rnd.uniform(0.0, 1.0) if (order > 1 and rnd.random() < 0.8) else None)
    add(1, [-1], -99.0, -rnd.uniform(0.0, 1.0) if order > 1 else None)
    if extras:
        lines[1].append("%.6f\t</s>" % -1.5)
        lines[1].append("%.6f\t<unk>\t%.6f" % (-3.0, -0.2))
        lines[1].append("%.6f\tab\t%.6f" % (-2.0, -0.1))
        lines[1].append("%.6f\t%s" % (-2.0, chr(V + offset)))
        dropped += 4
    for n in range(2, order + 1):
        seen = set()
        target = n_per_order if isinstance(n_per_order, int) else n_per_order[n]
        tries = 0
        while len(seen) < target and tries < 4 * target:
            tries += 1
            toks = [rnd.choice(known) for _ in range(n)]
            if rnd.random() < 0.3:
                toks[0] = -1
            # most higher-order n-grams extend a context that exists (so long backoff chains are exercised)
            if n > 2 and rnd.random() < 0.7:
                prev = rnd.choice(lines_ctx[n - 1]) if lines_ctx.get(n - 1) else None
                if prev is not None:
                    toks = list(prev) + [rnd.choice(known)]
            t = tuple(toks)
            if t in seen:
                continue
            seen.add(t)
            add(n, toks, -rnd.uniform(0.1, 3.0), -rnd.uniform(0.0, 1.0) if (n < order and rnd.random() < 0.7) else None)
            lines_ctx.setdefault(n, []).append(t)
        if extras:
            lines[n].append("%.6f\t%s </s>" % (-1.0, " ".join(w(known[0]) for _ in range(n - 1))))
            lines[n].append("%.6f\t%s %s" % (-1.0, " ".join(w(known[0]) for _ in range(n - 1)), chr(V + 5 + offset)))
            dropped += 2
    with open(path, "w") as f:
        f.write("\\data\\\n")
        for n in range(1, order + 1):
            f.write("ngram %d=%d\n" % (n, len(lines[n])))
        for n in range(1, order + 1):
            f.write("\n\\%d-grams:\n" % n)
            f.write("\n".join(lines[n]) + "\n")
        f.write("\n\\end\\\n")
    return entries, dropped

