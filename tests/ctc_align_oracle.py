"""fp64 reference of CTC forced alignment (avec_amd/csrc/ctc_align.hip): the Viterbi path of a given label sequence through the CTC trellis with the kernel's
tie rule, its score and its decision margin, plus a brute-force enumerator for tiny shapes and the input generators the tests and tools/bench_ctc_align.py share.

Tie rule over the S = 2 L + 1 extended states: the predecessor of s is s unless delta[s-1] is strictly greater; s-2 (allowed when ext[s] != blank and
ext[s] != ext[s-2]) only if strictly greater than the winner of those two; the end state is S-1 unless delta[S-2] is strictly greater."""
import itertools
import math

import numpy as np

NEG = -math.inf


def log_softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def collapse(path, blank=0):
    out, prev = [], None
    for t in path:
        if t != prev and t != blank:
            out.append(int(t))
        prev = t
    return out


def feasible(target, in_len, V, blank=0):
    target = list(target)
    if any(c == blank or c < 0 or c >= V for c in target):
        return False
    return in_len >= len(target) + sum(1 for i in range(1, len(target)) if target[i] == target[i - 1])


def _gap(cands):
    """best minus second best over the first axis of the finite candidates (inf where only one can be taken)"""
    c = -np.sort(-np.asarray(cands, dtype=np.float64), axis=0)
    with np.errstate(invalid="ignore"):
        return np.where(c[1] > NEG, c[0] - c[1], math.inf)


def viterbi(logp, in_len, target, blank=0):
    """logp [T, V] (log_softmax, fp64).  Returns (path, score, margin): path = the token of every frame t < in_len (None when infeasible, score -inf);
    margin = the smallest gap between the best and the second-best candidate over the decisions on the backtracked path, the end-state choice included."""
    T, V = logp.shape
    target = [int(c) for c in target]
    Tb, L = int(in_len), len(target)
    if not feasible(target, Tb, V, blank):
        return None, NEG, math.inf
    if Tb == 0:
        return [], 0.0, math.inf
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = target
    S = len(ext)
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    delta = np.full((Tb, S), NEG)
    back = np.zeros((Tb, S), dtype=np.int64)
    gaps = np.full((Tb, S), math.inf)
    delta[0, :2] = logp[0, ext[:2]]
    for t in range(1, Tb):
        a = delta[t - 1]
        b = np.concatenate([[NEG], a[:-1]])
        c = np.where(skip, np.concatenate([[NEG, NEG], a[:-2]])[:S], NEG)
        best, code = a, np.zeros(S, dtype=np.int64)
        m = b > best
        best, code = np.where(m, b, best), np.where(m, 1, code)
        m = c > best
        best, code = np.where(m, c, best), np.where(m, 2, code)
        delta[t] = best + logp[t, ext]                     # the emission is formed first, as in the kernel
        back[t], gaps[t] = code, _gap([a, b, c])
    s, score = S - 1, delta[Tb - 1, S - 1]
    ends = [score, NEG]
    if S > 1:
        ends[1] = delta[Tb - 1, S - 2]
        if delta[Tb - 1, S - 2] > score:
            s, score = S - 2, delta[Tb - 1, S - 2]
    if not score > NEG:
        return None, NEG, math.inf
    margin = float(_gap(ends))
    states = [0] * Tb
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        if t > 0:
            margin = min(margin, float(gaps[t, s]))
            s -= int(back[t, s])
    return [int(ext[k]) for k in states], float(score), float(margin)


def runs(path, blank=0):
    """[(token, first frame, last frame + 1)] of the non-blank runs of a frame path: the spans an alignment must report (a repeated token is two runs,
    separated by at least one blank frame)"""
    out, t = [], 0
    while t < len(path):
        u = t
        while u < len(path) and path[u] == path[t]:
            u += 1
        if path[t] != blank:
            out.append((int(path[t]), t, u))
        t = u
    return out


def brute_force(logp, in_len, target, blank=0):
    """max over ALL V^T frame paths that collapse to the target (T <= 6, V <= 3): (score, set of the paths that reach it)"""
    T, V = logp.shape
    Tb = int(in_len)
    assert Tb <= 6 and V <= 3
    target = [int(c) for c in target]
    best, arg = NEG, set()
    for p in itertools.product(range(V), repeat=Tb):
        if collapse(p, blank) != target:
            continue
        sc = float(sum(logp[t, k] for t, k in enumerate(p)))
        if sc > best:
            best, arg = sc, {p}
        elif sc == best:
            arg.add(p)
    return best, arg


# ---- inputs shared by the tests and tools/bench_ctc_align.py ----
def random_targets(B, Lmax, V, seed, p_repeat=0.2, lens=None):
    """targets [B, Lmax] int64 drawn from [1, V), each token repeating its left neighbour with probability p_repeat, lengths in [0, Lmax];
    the padding past tgt_len alternates -1 and V + 5 (values that must never be used as an index)"""
    g = np.random.default_rng(seed)
    tl = g.integers(0, Lmax + 1, size=B) if lens is None else np.asarray(lens)
    tg = np.empty((B, Lmax), dtype=np.int64)
    tg[:, 0::2], tg[:, 1::2] = -1, V + 5
    for b in range(B):
        for i in range(int(tl[b])):
            tg[b, i] = tg[b, i - 1] if i > 0 and g.random() < p_repeat else g.integers(1, V)
    return tg, tl.astype(np.int64)


def noise_logits(B, T, V, seed, scale=3.0):
    return (scale * np.random.default_rng(seed).standard_normal((B, T, V))).astype(np.float32)


def peaky_logits(B, T, V, seed, boost=6.0):
    """N(0, 1) with +boost on a random label per frame, half of them blank"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, T, V))
    lab = np.where(g.random((B, T)) < 0.5, 0, g.integers(1, V, size=(B, T)))
    np.add.at(x, (np.arange(B)[:, None], np.arange(T)[None, :], lab), boost)
    return x.astype(np.float32)


def aligned_logits(T, V, targets, tgt_lens, in_lens, seed, boost=6.0):
    """N(0, 1) with +boost along a random monotone alignment of each target (2 L random cut points over its in_len frames: blank, y1, blank, y2, ...).
    An utterance that is too short for its target stays plain noise."""
    g = np.random.default_rng(seed)
    B = targets.shape[0]
    x = g.standard_normal((B, T, V))
    for b in range(B):
        L, Tb = int(tgt_lens[b]), int(in_lens[b])
        if Tb < 2 * L + 1:
            continue
        # every token gets >= 1 frame and every blank gap >= 1 frame, so the labelling collapses to the target whatever its repeats
        extra = np.sort(g.integers(0, Tb - (2 * L + 1) + 1, size=2 * L))
        cuts = extra + np.arange(1, 2 * L + 1)
        lab = np.zeros(Tb, dtype=np.int64)
        for i in range(L):
            lab[cuts[2 * i]:cuts[2 * i + 1]] = targets[b, i]
        x[b, np.arange(Tb), lab] += boost
    return x.astype(np.float32)
