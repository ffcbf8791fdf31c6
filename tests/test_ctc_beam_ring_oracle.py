"""The fp64 oracle of the ring mode (tests/ctc_beam_ring_oracle.py) against the offline oracle where the two must agree, its own invariant, and a commit worked
out by hand."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_beam_oracle as O  # noqa: E402
import ctc_beam_ring_oracle as R  # noqa: E402


def _lm(tmp_path, V, order):
    want, _ = O.write_random_arpa(str(tmp_path / ("lm%d.arpa" % order)), V=V, order=order, n_per_order=500, seed=order)
    return O.DictLM(want, order, V)


@pytest.mark.parametrize("order", [None, 3])
@pytest.mark.parametrize("window", [40, 41, 1000])
def test_window_of_the_whole_utterance_is_the_offline_search(tmp_path, order, window):
    T, V, W = 40, 32, 8
    lm = None if order is None else _lm(tmp_path, V, order)
    for seed in (1, 2):
        logp = O.log_softmax64(O.ctc_like_logits(1, T, V, seed=seed)[0], 1.5)
        beams, gap = O.beam_search(logp, T, W, lm=lm)
        r = R.beam_search_windowed(logp, T, W, window, lm=lm)
        assert r.beams == beams and r.gap == gap                     # the same arithmetic in the same order: exact
        assert (r.base, r.dropped, r.commits, r.committed) == (0, 0, 0, [])
        assert [t for t, _ in r.tails] == [b[0] for b in beams]


@pytest.mark.parametrize("window", [2, 3, 8, 16])
def test_one_beam_never_drops_and_equals_offline(window):
    T, V = 50, 32
    logp = O.log_softmax64(O.ctc_like_logits(1, T, V, seed=window)[0], 1.0)
    beams, _ = O.beam_search(logp, T, 1)
    r = R.beam_search_windowed(logp, T, 1, window)
    assert r.beams == beams and r.dropped == 0
    assert r.commits == (T - 1 - window) // (window // 2) + 1 and r.base == r.commits * (window // 2)
    assert [t for t, _ in r.committed] + r.tails[0][0] == beams[0][0]


@pytest.mark.parametrize("order", [None, 3])
@pytest.mark.parametrize("W,window", [(16, 16), (4, 8), (16, 2), (8, 5)])
def test_committed_and_tail_spell_every_live_prefix_after_every_frame(tmp_path, order, W, window):
    T, V = 70, 32
    lm = None if order is None else _lm(tmp_path, V, order)
    logp = O.log_softmax64(O.ctc_like_logits(1, T, V, seed=W + window)[0], 1.5)
    snaps = R.beam_search_windowed(logp, T, W, window, lm=lm, per_frame=True)
    assert len(snaps) == T + 1
    h = window // 2
    for t, s in enumerate(snaps):
        assert 0 <= t - s.base <= window and s.base == s.commits * h
        assert s.commits == (0 if t <= window else (t - 1 - window) // h + 1)
        ctok, cfr = [c for c, _ in s.committed], [f for _, f in s.committed]
        assert cfr == sorted(set(cfr)) and all(f < s.base for f in cfr)       # at most one token per frame, all older than base
        for (tokens, _, _), (tail, frames) in zip(s.beams, s.tails):
            assert ctok + tail == tokens
            assert frames == sorted(set(frames)) and all(s.base <= f < t for f in frames)
        if t:
            p = snaps[t - 1]
            assert s.committed[:len(p.committed)] == p.committed and s.dropped >= p.dropped     # what is final stays
    last = snaps[-1]
    assert last == R.beam_search_windowed(logp, T, W, window, lm=lm)
    assert last.commits >= 5 and (W == 1 or last.dropped > 0)


def test_six_frames_by_hand():
    """V = 3 (blank, 1, 2), W = 2, window = 4, so h = 2 and the one commit comes before frame 4 with f = 1: rows 0 and 1 become final.  Probabilities per frame:
        frame 0  [.40 .55 .05]   (1) = .55, () = .40                                  [(2) = .05 is third]      slot 0 = (1) from slot 0 with token 1, slot 1 = ()
        frame 1  [.90 .05 .05]   (1) = .55 * .95 + .40 * .05 (() extended by 1 joins it) = .5425, () = .36   [(1, 2) = .0275]   both stay in place
        frame 2  [.02 .02 .96]   (1, 2) = .5425 * .96 = .5208, (2) = .36 * .96 = .3456  [stays: about .011, .007]  slot 0 = (1, 2) from slot 0, slot 1 = (2) from slot 1
        frame 3  [.98 .01 .01]   (1, 2) = .5208 * .99 = .5156, (2) = .3421            [extensions below .006]    both stay in place
    Commit before frame 4: beam 0 walks rows 3, 2 to slot 0 after frame 1, beam 1 walks them to slot 1, so a = 0.  From slot 0, row 1 is a stay and row 0 emitted
    token 1: committed = [(1, 0)].  Beam 1, (2), descends from slot 1: dropped = 1.  base = 2, and the margin ln(.5156 / .3421) = 0.4101 joins the gap.
        frame 4  [.98 .01 .01]   (1, 2) alone is live: it stays, and (1, 2, 1) = .5156 * .01 enters as slot 1, from slot 0 with token 1
        frame 5  [.05 .90 .05]   the extension of (1, 2) by 1 re-creates (1, 2, 1), so its mass joins that beam's stay: (1, 2, 1) wins as the stay of slot 1
    so the best tail is [2, 1], emitted at frames 2 and 4 (frame 4 is where that beam's own path took the 1, not frame 5 where it gained its mass)."""
    p = np.array([[0.40, 0.55, 0.05], [0.90, 0.05, 0.05], [0.02, 0.02, 0.96], [0.98, 0.01, 0.01], [0.98, 0.01, 0.01], [0.05, 0.90, 0.05]])
    snaps = R.beam_search_windowed(np.log(p), 6, 2, 4, per_frame=True)
    assert [b[0] for b in snaps[2].beams] == [[1], []]
    s = snaps[4]
    assert [b[0] for b in s.beams] == [[1, 2], [2]] and (s.base, s.dropped, s.commits, s.committed) == (0, 0, 0, [])
    assert s.tails == [([1, 2], [0, 2]), ([2], [2])]
    assert abs(math.exp(s.beams[0][1]) - 0.5156) < 1e-4 and abs(math.exp(s.beams[1][1]) - 0.3421) < 1e-4
    s = snaps[5]
    assert (s.base, s.dropped, s.commits, s.committed) == (2, 1, 1, [(1, 0)])
    assert [b[0] for b in s.beams] == [[1, 2], [1, 2, 1]] and s.tails == [([2], [2]), ([2, 1], [2, 4])]
    assert s.gap <= math.log(0.5156 / 0.3421) + 1e-3                              # the commit margin bounds the gap from then on
    end = snaps[6]
    assert end.beams[0][0] == [1, 2, 1] and end.committed == [(1, 0)] and end.tails[0] == ([2, 1], [2, 4]) and end.dropped == 1 and end.commits == 1
    assert all([c for c, _ in end.committed] + t == b[0] for b, (t, _) in zip(end.beams, end.tails))
    off, _ = O.beam_search(np.log(p), 6, 2)                                         # the unlimited search ends on the same best hypothesis here
    assert off[0][0] == [1, 2, 1]
