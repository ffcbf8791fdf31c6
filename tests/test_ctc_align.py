"""CTC forced alignment, the parts that need no GPU: the fp64 oracle of tests/ctc_align_oracle.py against brute force over all frame paths, the word grouping of
nnet.decoders.words_from_pieces, and the argument checks of avec_ctc_align (reported before any launch)."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_align_oracle as O  # noqa: E402
from avec_amd.nnet.decoders import CTCBeamSearchDecoder, CTCGreedySearchDecoder, words_from_pieces  # noqa: E402

SP = "▁"


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_oracle_equals_brute_force_on_every_short_target(T):
    """every target of length <= 3 over {0 (blank, never alignable), 1, 2} at V = 3: the oracle's score is the maximum over all 3^T frame paths, its path is one of
    the maximisers, and it reports infeasible exactly when no frame path collapses to the target"""
    V = 3
    logp = O.log_softmax64(np.random.default_rng(100 + T).standard_normal((T, V)) * 2.0)
    n_inf = 0
    for L in range(4):
        for target in itertools.product(range(V), repeat=L):
            best, arg = O.brute_force(logp, T, target)
            path, score, margin = O.viterbi(logp, T, target)
            if best == -math.inf:
                n_inf += 1
                assert path is None and score == -math.inf, (T, target)
                assert not O.feasible(target, T, V)
                continue
            assert O.feasible(target, T, V)
            assert abs(score - best) <= 1e-12 * max(1.0, abs(best)), (T, target, score, best)
            assert tuple(path) in arg and O.collapse(path) == list(target), (T, target, path)
            assert margin >= 0.0
            if margin > 1e-9 and len(arg) == 1:
                assert tuple(path) == next(iter(arg))
    assert n_inf >= 1 + 3 + 9 + 27 - (1 + 2 + 4 + 8)          # at least every target with a blank in it


def test_oracle_tie_rule_and_margin():
    """a flat trellis ties everywhere: the rule keeps the state (stay before s-1 before s-2) and ends in the last blank, and the margin says so"""
    logp = np.full((4, 3), math.log(1.0 / 3.0))
    path, score, margin = O.viterbi(logp, 4, [1])
    assert path == [1, 0, 0, 0] and margin == 0.0 and abs(score - 4 * math.log(1.0 / 3.0)) < 1e-12
    path, _, _ = O.viterbi(logp, 4, [1, 1])
    assert path == [1, 0, 1, 0]
    assert O.viterbi(logp, 2, [1, 1])[0] is None and O.viterbi(logp, 3, [1, 1])[0] == [1, 0, 1]
    assert O.viterbi(logp, 0, []) == ([], 0.0, math.inf) and O.viterbi(logp, 0, [1])[0] is None
    assert O.runs([0, 1, 1, 0, 1, 2, 2]) == [(1, 1, 3), (1, 4, 5), (2, 5, 7)]


def test_words_from_pieces():
    # a leading marker, pieces that continue a word, a second word
    w = words_from_pieces([SP + "he", "llo", SP + "wor", "ld"], [(0, 2), (3, 4), (6, 7), (7, 9)], [-0.5, -0.25, -1.0, -2.0])
    assert w == [("hello", 0, 4, -0.75), ("world", 6, 9, -3.0)]
    # no leading marker: the first piece still begins a word
    assert words_from_pieces(["a", "b", SP + "c"], [(1, 2), (2, 3), (5, 6)], [-1.0, -1.0, -1.0]) == [("ab", 1, 3, -2.0), ("c", 5, 6, -1.0)]
    # a lone marker followed by a continuation piece is one word that starts at the marker; a lone marker with nothing after it is dropped
    assert words_from_pieces([SP, "x", SP], [(0, 1), (2, 3), (4, 5)], [-0.5, -0.5, -0.125]) == [("x", 0, 3, -1.0)]
    assert words_from_pieces([SP, SP + "y"], [(0, 1), (1, 2)], [-1.0, -2.0]) == [("y", 1, 2, -2.0)]
    assert words_from_pieces([], [], []) == []
    # seconds work as well as frames
    assert words_from_pieces([SP + "a"], [(0.04, 0.12)], [-1.0]) == [("a", 0.04, 0.12, -1.0)]


def test_decoders_expose_alignment_api():
    import nnet
    assert nnet.words_from_pieces is words_from_pieces
    for cls in (CTCGreedySearchDecoder, CTCBeamSearchDecoder):
        assert callable(cls.align) and callable(cls.decode_with_timestamps)
    from avec_amd import ops
    assert callable(ops.ctc_align)


def test_ctc_align_argument_errors_without_gpu():
    """argument errors are reported before any launch (no GPU needed): the pointers below are never dereferenced"""
    from avec_amd.lib import lib
    P = 4096                                                # a non-null, 16-byte aligned "pointer"
    B, T, V, Lmax = 2, 10, 8, 3
    need = lib.raw("avec_ctc_align_workspace_bytes")(B, T, Lmax)
    S, NC = 2 * Lmax + 1, (2 * Lmax + 1 + 63) // 64
    assert need == B * (T * NC * 16 + (T * S * 4 + 15) // 16 * 16)
    assert lib.raw("avec_ctc_align_fits_lds")(100, 40) == 1 and lib.raw("avec_ctc_align_fits_lds")(376, 130) == 0
    assert lib.raw("avec_ctc_align_fits_lds")(0, 4) == 0
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.ctc_align(None, P, P, P, B, T, V, Lmax, 0, 0, P, need, P, P, P, P, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.ctc_align(P, P, P, P, B, T, V, Lmax, 0, 0, P, need, P, None, P, P, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        lib.ctc_align(P, P, P, P, B, T, V, Lmax, 0, 0, None, need, P, P, P, P, None)
    with pytest.raises(RuntimeError, match="bad dims"):
        lib.ctc_align(P, P, P, P, B, 0, V, Lmax, 0, 0, P, need, P, P, P, P, None)
    with pytest.raises(RuntimeError, match="bad dims"):
        lib.ctc_align(P, P, P, P, B, T, V, Lmax, V, 0, P, need, P, P, P, P, None)
    with pytest.raises(RuntimeError, match="workspace of"):
        lib.ctc_align(P, P, P, P, B, T, V, Lmax, 0, 0, P, need - 1, P, P, P, P, None)
    with pytest.raises(RuntimeError, match="tier 1"):
        lib.ctc_align(P, P, P, P, 8, 376, 256, 130, 0, 1, P, lib.raw("avec_ctc_align_workspace_bytes")(8, 376, 130), P, P, P, P, None)
    with pytest.raises(RuntimeError, match="tier 3"):
        lib.ctc_align(P, P, P, P, B, T, V, Lmax, 0, 3, P, need, P, P, P, P, None)
