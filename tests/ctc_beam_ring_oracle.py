"""fp64 reference of the ring mode of the CTC prefix beam search (avec_ctc_beam_stream_ring in avec_amd/csrc/ctc_beam.hip): the frame loop of
ctc_beam_oracle.beam_search, statement for statement, plus one backpointer row per frame, (parent slot, token or None) per new beam, and the commit step.

The rule.  `base` is the oldest frame whose row is held.  Immediately before absolute frame t is consumed, when t - base == window, with h = window // 2 and
f = base + h - 1:
  1. every live beam w walks rows t-1 .. f+1 to anc[w], the slot it descends from after frame f; a = anc[0] (slot 0 is the best beam);
  2. from slot a, rows f .. base give the tokens that become final, logged oldest first with the frame of the row that emitted each;
  3. the beams with anc[w] != a are dropped, the others keep their order, and row t-1 is rewritten in that order;
  4. base = f + 1, dropped += beams dropped, commits += 1.
Nothing else changes: a prefix stays the whole token tuple (the device's absolute `len` and whole-prefix hash), scores are untouched."""
import collections
import math

import numpy as np

from ctc_beam_oracle import NEG, lae

Ring = collections.namedtuple("Ring", "beams tails committed base dropped commits gap")
Ring.__doc__ = """beams [(tokens, score, ctc_logp)] best first, whole hypotheses, as ctc_beam_oracle.beam_search; tails [(tokens, frames)] per beam: its own path through the
held rows; committed [(token, frame)]; base, dropped, commits; gap = beam_search's gap extended by score[0] - score[1] at every commit step"""


def _commit(beams, rows, base, t, window, committed):
    """the commit step before frame t -> (beams, base, beams dropped, score margin of beam 0); rows {frame: [(parent, token or None)]} is edited in place"""
    f = base + window // 2 - 1
    anc = []
    for w in range(len(beams)):
        s = w
        for r in range(t - 1, f, -1):
            s = rows[r][s][0]
        anc.append(s)
    a = anc[0]
    new, s = [], a
    for r in range(f, base - 1, -1):
        parent, tok = rows[r][s]
        if tok is not None:
            new.append((tok, r))
        s = parent
    committed.extend(reversed(new))
    keep = [w for w in range(len(beams)) if anc[w] == a]
    score = [lae(pb, pnb) + lms for _, pb, pnb, lms in beams]
    margin = score[0] - score[1] if len(beams) > 1 else math.inf
    rows[t - 1] = [rows[t - 1][w] for w in keep]
    for r in range(base, f + 1):
        del rows[r]
    return [beams[w] for w in keep], f + 1, len(beams) - len(keep), margin


def _snapshot(beams, rows, base, t, committed, dropped, commits, gap):
    out = [(list(pre), lae(pb, pnb) + lms, lae(pb, pnb)) for pre, pb, pnb, lms in beams]
    for p, q in zip(out, out[1:]):
        gap = min(gap, p[1] - q[1])
    tails = []
    for w in range(len(beams)):
        s, tk, fr = w, [], []
        for r in range(t - 1, base - 1, -1):
            parent, tok = rows[r][s]
            if tok is not None:
                tk.append(tok)
                fr.append(r)
            s = parent
        tails.append((tk[::-1], fr[::-1]))
    return Ring(out, tails, list(committed), base, dropped, commits, gap)


def beam_search_windowed(logp, length, W, window, lm=None, alpha=0.6, beta=1.0, per_frame=False):
    """logp [T, V] fp64 (already log_softmax'ed).  Returns a Ring for the `length` frames, or with per_frame the list of Rings after 0, 1, .. length frames (the
    commit that precedes frame t is not part of the result after t frames: t - base <= window in every one)."""
    if window < 2:
        raise ValueError("window %d < 2" % window)
    V = logp.shape[1]
    beams = [((), 0.0, NEG, 0.0)]           # (prefix, pb, pnb, lm)
    gap = math.inf
    rows, committed, base, dropped, commits = {}, [], 0, 0, 0
    snaps = [_snapshot(beams, rows, base, 0, committed, dropped, commits, gap)] if per_frame else None
    for t in range(int(length)):
        if t - base == window:
            beams, base, nd, margin = _commit(beams, rows, base, t, window, committed)
            dropped, commits, gap = dropped + nd, commits + 1, min(gap, margin)
        lp = logp[t]
        slot = {b[0]: i for i, b in enumerate(beams)}
        stay = []
        for pre, pb, pnb, _ in beams:
            stay.append([lae(pb, pnb) + lp[0], pnb + lp[pre[-1]] if pre else NEG])
        ext_pnb, ext_lm = [], []
        for pre, pb, pnb, lms in beams:
            e = pre[-1] if pre else -1
            m = np.full(V, lae(pb, pnb))
            if e >= 0:
                m[e] = pb
            m = m + lp
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
        nb, row = [], []
        for k in kept:
            if k < n:
                pre, _, _, lms = beams[k]
                nb.append((pre, stay[k][0], stay[k][1], lms))
                row.append((int(k), None))
            else:
                i, c = divmod(int(cand_i[k]) - W, V)
                nb.append((beams[i][0] + (c,), NEG, float(ext_pnb[i][c]), float(ext_lm[i][c])))
                row.append((i, c))
        beams, rows[t] = nb, row
        if per_frame:
            snaps.append(_snapshot(beams, rows, base, t + 1, committed, dropped, commits, gap))
    return snaps if per_frame else _snapshot(beams, rows, base, int(length), committed, dropped, commits, gap)
