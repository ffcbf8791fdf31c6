"""CTC forced alignment on the device (avec_ctc_align, ops.ctc_align, the decoders' align / decode_with_timestamps) against the fp64 oracle of
tests/ctc_align_oracle.py.  Both tiers (1: emissions and backpointers in LDS, 2: in the workspace) run every case they can and must agree bit for bit.

Tolerances.  A sum x of log-probabilities is compared to its fp64 value to 1e-4 |x| + 1e-5: the device adds at most T = 376 fp32 terms in sequence (relative
error <= T * 2^-24 = 2.3e-5 of the largest partial sum) on top of emissions that carry the fp32 rounding of logit - lse (<= 2^-23 * 16 = 2e-6 each).  The exact
frame path is compared where the oracle's decision margin exceeds GAP = max(1e-4, 64 * 2^-23 * |score|): a decision compares two partial sums of magnitude <= |score|,
each within a few dozen fp32 roundings of its fp64 value."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_align_oracle as O  # noqa: E402
from avec_amd import ops  # noqa: E402
from avec_amd.lib import lib  # noqa: E402
from avec_amd.nnet.decoders import ctc_collapse  # noqa: E402

pytestmark = pytest.mark.gpu
NT = 256                                # threads of the alignment workgroup (csrc/ctc_align.hip): 2 Lmax + 1 > NT makes the strided state loop run twice
L_STRIDED = NT // 2                     # the smallest Lmax with 2 Lmax + 1 > NT


def _gap(score):
    return max(1e-4, 64 * 2.0 ** -23 * abs(score))


def _close(a, b):
    return abs(a - b) <= 1e-4 * abs(b) + 1e-5


def _ragged(B, T, lo, seed):
    lens = np.random.default_rng(seed).integers(lo, T + 1, size=B)
    lens[0] = T
    return lens.astype(np.int64)


# ---- the cases: (logits [B, T, V] fp32, in_lens, targets [B, Lmax] padded with -1 / V + 5, tgt_lens); built once, never modified ----
SHAPES = {"small": (16, 30, 32, 8), "mid": (16, 100, 256, 40), "long": (8, 376, 256, 130)}
EXACT = ["small-noise", "small-peaky", "mid-noise", "mid-peaky", "long-aligned"]          # the exact-path cases: >= 75 % of the feasible utterances above GAP


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "edges":
        return _edges()
    if name == "strided":
        return _strided()
    shape, kind = name.split("-")
    B, T, V, Lmax = SHAPES[shape]
    seed = sorted(SHAPES).index(shape) * 10 + len(kind)
    tg, tl = O.random_targets(B, Lmax, V, seed)
    il = _ragged(B, T, {"small": 12, "mid": 56, "long": 300}[shape], seed + 1)
    if kind == "noise":
        x = O.noise_logits(B, T, V, seed + 2)
    elif kind == "peaky":
        x = O.peaky_logits(B, T, V, seed + 2)
    else:
        x = O.aligned_logits(T, V, tg, tl, il, seed + 2)
    return x, il, tg, tl


def _edges():
    V, T, Lmax = 16, 12, 4
    rows = [  # (in_len, tgt_len, targets)
        (T, 3, [3, 5, 7]),                  # 0 plain
        (0, 2, [3, 5]),                     # 1 no frames, two tokens: infeasible
        (0, 0, []),                         # 2 nothing to nothing: score 0
        (1, 1, [4]),                        # 3 one frame, one token
        (1, 0, []),                         # 4 one blank frame
        (T, 0, []),                         # 5 all blank
        (4, 3, [6, 6, 2]),                  # 6 exactly L + repeats frames
        (3, 3, [6, 6, 2]),                  # 7 one frame too short: infeasible
        (T, 3, [3, 0, 5]),                  # 8 a target equal to blank: infeasible
        (T, 2, [3, V + 5]),                 # 9 a target >= V: infeasible
        (T, 2, [2 ** 40 + 3, 3]),           # 10 a target far outside (its low 32 bits would be a valid token): infeasible
        (T, 2, [3, -1]),                    # 11 a negative target: infeasible
        (T, 4, [1, 15, 15, 1]),             # 12 L = Lmax, the first and the last token of the vocabulary
        (T + 5, Lmax + 3, [9, 8, 7, 6]),    # 13 lengths beyond the tensors: clamped to T and Lmax
        (-3, 0, []),                        # 14 a negative length: clamped to 0
    ]
    B = len(rows)
    tg = np.empty((B, Lmax), dtype=np.int64)
    tg[:, 0::2], tg[:, 1::2] = -1, V + 5
    for b, (_, _, t) in enumerate(rows):
        tg[b, :len(t)] = t
    il, tl = np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.int64)
    return O.noise_logits(B, T, V, seed=77), il, tg, tl


EDGE_INFEASIBLE = [1, 7, 8, 9, 10, 11]


def _strided():
    """Lmax = 128: an utterance of 128 tokens has 257 states, one more than the workgroup has threads.  T = 140 keeps the shape inside the all-LDS tier."""
    V, T, Lmax = 64, 140, L_STRIDED
    g = np.random.default_rng(5)
    tg, tl = O.random_targets(4, Lmax, V, seed=6, lens=[Lmax, Lmax, 100, Lmax])
    tg[0] = 1 + (np.arange(Lmax) * 7) % (V - 1)                       # no adjacent repeats
    tg[0, 1::2] = 1 + (tg[0, 1::2] + 30) % (V - 1)
    assert (tg[0, 1:] != tg[0, :-1]).all()
    tg[1] = tg[0]
    tg[1, [10, 40, 41, 90, 100, 127]] = tg[1, [9, 39, 40, 89, 99, 126]]          # 6 adjacent repeats (40, 41: three equal tokens in a row)
    rep1 = int((tg[1, 1:] == tg[1, :-1]).sum())
    tg[3] = tg[0]
    il = np.array([T, Lmax + rep1, T, Lmax - 1], dtype=np.int64)      # 1: exactly L + repeats frames; 3: one frame short
    return O.noise_logits(4, T, V, seed=int(g.integers(1000))), il, tg, tl


def _clamped(name):
    x, il, tg, tl = case(name)
    return np.clip(il, 0, x.shape[1]), np.clip(tl, 0, tg.shape[1])


@functools.lru_cache(maxsize=None)
def oracle(name):
    """per utterance (path or None, score, margin) of the fp64 oracle"""
    x, _, tg, _ = case(name)
    il, tl = _clamped(name)
    return [O.viterbi(O.log_softmax64(x[b]), il[b], tg[b, :tl[b]]) for b in range(x.shape[0])]


@functools.lru_cache(maxsize=None)
def device(name, tier):
    """(path, spans, score, token_logp) as numpy arrays"""
    x, il, tg, tl = case(name)
    args = [torch.from_numpy(x).cuda(), torch.from_numpy(il).cuda(), torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda()]
    out = ops.ctc_align(*args, blank=0, tier=tier)
    return tuple(o.cpu().numpy() for o in out)


def tiers(name):
    T, Lmax = case(name)[0].shape[1], case(name)[2].shape[1]
    return (1, 2) if lib.raw("avec_ctc_align_fits_lds")(T, Lmax) else (0, 2)


def check_utterance(name, b, out, exact_counter=None):
    """every property of one utterance's outputs; counts the utterance in exact_counter = [checked, feasible] when its margin allows the exact-path check"""
    x, _, tg, _ = case(name)
    il, tl = _clamped(name)
    path, spans, score, tlp = (o[b] for o in out)
    ref_path, ref_score, margin = oracle(name)[b]
    Tb, L, Lmax = int(il[b]), int(tl[b]), tg.shape[1]
    where = (name, b)
    assert not np.isnan(score) and not np.isnan(tlp).any(), where
    if ref_path is None:
        assert score == -np.inf and (path == -1).all() and (spans == -1).all() and (tlp == 0).all(), where
        return
    assert (path[Tb:] == -1).all() and (spans[L:] == -1).all() and (tlp[L:] == 0).all(), where
    p = path[:Tb].tolist()
    assert all(0 <= k < x.shape[2] for k in p), where
    assert ctc_collapse(p, Tb, 0) == tg[b, :L].tolist(), where
    runs = O.runs(p)
    assert [r[0] for r in runs] == tg[b, :L].tolist() and spans[:L].tolist() == [[r[1], r[2]] for r in runs], where
    logp = O.log_softmax64(x[b])
    for i, (k, f0, f1) in enumerate(runs):
        want = float(logp[f0:f1, k].sum())
        assert _close(float(tlp[i]), want), (where, i, float(tlp[i]), want)
    along = float(logp[np.arange(Tb), p].sum()) if Tb else 0.0
    assert _close(float(score), along), (where, float(score), along)
    assert _close(float(score), ref_score), (where, float(score), ref_score)          # optimal whatever the ties
    if exact_counter is not None:
        exact_counter[1] += 1
        if margin > _gap(ref_score):
            exact_counter[0] += 1
            assert p == ref_path, (where, margin)


def device_nll(name):
    """-log p(target | logits) per utterance from avec_ctc_loss (inf where infeasible)"""
    x, il, tg, tl = case(name)
    B, T, V = x.shape
    Lmax = tg.shape[1]
    lg, ilc, tlc = torch.from_numpy(x).cuda(), torch.from_numpy(il).cuda(), torch.from_numpy(tl).cuda()
    tgc = torch.from_numpy(np.where((tg < 0) | (tg >= V), 1, tg)).cuda()          # (the loss kernel is not the subject here: give it clean padding)
    nll = torch.empty(B, dtype=torch.float32, device="cuda")
    mean = torch.zeros((), dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.raw("avec_ctc_workspace_floats")(B, T, max(Lmax, 1)), dtype=torch.float32, device="cuda")
    lib.ctc_loss(lg.data_ptr(), ilc.data_ptr(), tgc.data_ptr(), tlc.data_ptr(), nll.data_ptr(), mean.data_ptr(), None, ws.data_ptr(), B, T, V, Lmax, 0, 0,
                 torch.cuda.current_stream().cuda_stream)
    return nll.cpu().numpy()


@pytest.mark.parametrize("name", EXACT)
def test_properties_exact_path_and_loss_bound(name):
    """cases 1 and 2: every property on every utterance, the oracle's exact path where its margin exceeds GAP (at least 75 % of the feasible utterances), and
    score <= log p(target) of avec_ctc_loss"""
    nll = device_nll(name)
    B = case(name)[0].shape[0]
    for tier in tiers(name):
        out = device(name, tier)
        n = [0, 0]
        for b in range(B):
            check_utterance(name, b, out, n)
            if oracle(name)[b][0] is not None:
                sc = float(out[2][b])
                assert sc <= -float(nll[b]) + 1e-4 * abs(sc) + 1e-5, (name, tier, b, sc, -float(nll[b]))
        assert n[1] >= B // 2, "only %d of %d utterances of %s are feasible" % (n[1], B, name)
        assert n[0] >= 0.75 * n[1], "only %d of %d feasible utterances of %s have an oracle margin above GAP" % (n[0], n[1], name)


@pytest.mark.parametrize("name", EXACT + ["edges", "strided"])
def test_tiers_agree_bit_for_bit(name):
    a, b = (device(name, t) for t in tiers(name))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    if 1 not in tiers(name):                # the long clips do not fit the all-LDS tier: asking for it is an argument error, not a fallback
        x, il, tg, tl = case(name)
        with pytest.raises(RuntimeError, match="tier 1"):
            ops.ctc_align(torch.from_numpy(x).cuda(), torch.from_numpy(il).cuda(), torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda(), tier=1)


def test_edges_in_one_ragged_batch():
    """case 3: the sentinel outputs of the infeasible utterances, the special lengths, and the other utterances of the batch unaffected by them"""
    x, il, tg, tl = case("edges")
    B = x.shape[0]
    assert [b for b in range(B) if oracle("edges")[b][0] is None] == EDGE_INFEASIBLE
    for tier in (1, 2):
        out = device("edges", tier)
        for b in range(B):
            check_utterance("edges", b, out)
        path, spans, score, tlp = out
        assert score[2] == 0.0 and (path[2] == -1).all() and score[14] == 0.0 and (path[14] == -1).all()          # in_len == 0 == tgt_len
        assert path[4].tolist() == [0] + [-1] * 11 and (path[5] == 0).all() and (spans[5] == -1).all()            # tgt_len == 0: all blank
        assert path[3, 0] == 4 and spans[3, 0].tolist() == [0, 1]
        assert path[6, :4].tolist() == [6, 0, 6, 2] and spans[6, :3].tolist() == [[0, 1], [2, 3], [3, 4]]          # the only path of [6, 6, 2] in 4 frames
        assert ctc_collapse(path[13].tolist(), 12, 0) == [9, 8, 7, 6]
        # each feasible utterance alone gives the same bits as inside the batch
        for b in (0, 6, 12):
            one = ops.ctc_align(torch.from_numpy(x[b:b + 1]).cuda(), torch.from_numpy(il[b:b + 1]).cuda(), torch.from_numpy(tg[b:b + 1]).cuda(),
                                torch.from_numpy(tl[b:b + 1]).cuda(), tier=tier)
            for o, full in zip(one, out):
                assert o.cpu().numpy()[0].tobytes() == full[b].tobytes(), (tier, b)


def test_more_states_than_threads():
    """case 4: 2 Lmax + 1 = 257 states on 256 threads"""
    x, il, tg, tl = case("strided")
    assert 2 * tg.shape[1] + 1 == NT + 1 and int(tl[0]) == tg.shape[1]
    feas = [o[0] is not None for o in oracle("strided")]
    assert feas == [True, True, True, False]
    for tier in (1, 2):
        out = device("strided", tier)
        n = [0, 0]
        for b in range(4):
            check_utterance("strided", b, out, n)
        assert out[1][0, -1, 0] >= 0 and out[0][1, :int(il[1])].tolist() == O.viterbi(O.log_softmax64(x[1]), il[1], tg[1])[0]          # no slack: one path


@pytest.mark.parametrize("name", ["small-noise", "edges", "strided"])
def test_every_output_element_is_written(name, monkeypatch):
    """case 5: outputs allocated full of NaN bit patterns come back without one"""
    real = torch.empty

    def poisoned(*a, **k):
        t = real(*a, **k)
        if t.dtype == torch.float32:
            t.fill_(float("nan"))
        elif t.dtype == torch.int32:
            t.fill_(0x7FC00000)                     # the int32 view of a quiet NaN
        return t
    x, il, tg, tl = case(name)
    args = [torch.from_numpy(x).cuda(), torch.from_numpy(il).cuda(), torch.from_numpy(tg).cuda(), torch.from_numpy(tl).cuda()]
    for tier in (1, 2):
        monkeypatch.setattr(torch, "empty", poisoned)
        out = ops.ctc_align(*args, tier=tier)
        monkeypatch.setattr(torch, "empty", real)
        path, spans, score, tlp = (o.cpu().numpy() for o in out)
        assert not np.isnan(score).any() and not np.isnan(tlp).any()
        assert (path != 0x7FC00000).all() and (spans != 0x7FC00000).all()
        for got, want in zip((path, spans, score, tlp), device(name, tier)):
            assert got.tobytes() == want.tobytes()


def test_decoders_with_timestamps():
    """case 6: greedy and small-beam decoders return forward()'s ids plus consistent records; the greedy alignment is the argmax path"""
    import nnet
    B, T, V = 6, 40, 64
    x = O.peaky_logits(B, T, V, seed=31)
    lens = _ragged(B, T, 20, seed=32)
    lens[1] = 0
    outputs = (torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda())
    logp = O.log_softmax64(x)
    greedy = nnet.CTCGreedySearchDecoder()
    ids, recs = greedy.decode_with_timestamps(outputs)
    assert ids == greedy(outputs) and len(recs) == B
    am = ops.argmax_rows(outputs[0]).cpu().numpy()
    path = ops.ctc_align(outputs[0], outputs[1], *_pad(ids))[0].cpu().numpy()
    for b in range(B):
        n = int(lens[b])
        want = float(logp[b, :n].max(axis=1).sum())
        assert _close(recs[b]["score"], want), (b, recs[b]["score"], want)
        top2 = np.sort(logp[b, :n], axis=1)[:, -2:]
        if n == 0 or (top2[:, 1] - top2[:, 0]).min() > _gap(want):
            assert path[b, :n].tolist() == am[b, :n].tolist(), b
        _check_record(recs[b], ids[b], logp[b], n)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        beam = nnet.CTCBeamSearchDecoder(beam_size=4)
        tta = nnet.CTCBeamSearchDecoder(beam_size=4, test_time_aug=True)
    ids, recs = beam.decode_with_timestamps(outputs)
    assert ids == beam(outputs)
    for b in range(B):
        _check_record(recs[b], ids[b], logp[b], int(lens[b]))
    with pytest.raises(NotImplementedError, match="test_time_aug"):
        tta.decode_with_timestamps((outputs[0][:, None], outputs[1][:, None]))
    # align() with tensors equals align() with lists; a transcript that cannot be aligned gives an empty record with score -inf
    tok, tl = _pad(ids)
    assert beam.align(outputs, (tok, tl)) == recs
    bad = greedy.align(outputs, [[1] * (T + 1)] * B)
    assert all(r["score"] == -math.inf and r["tokens"] == [] for r in bad)


def _pad(ids):
    tl = torch.tensor([len(h) for h in ids], dtype=torch.int64)
    tok = torch.full((len(ids), max(1, int(tl.max()))), -1, dtype=torch.int64)
    for b, h in enumerate(ids):
        tok[b, :len(h)] = torch.tensor(h, dtype=torch.int64)
    return tok, tl


def _check_record(rec, ids, logp, n):
    """a record is internally consistent: its tokens are the hypothesis, spans are increasing, inside the utterance and disjoint, logps are the sums over the spans
    and never exceed the score's share, seconds are frames * 0.04"""
    assert [t[0] for t in rec["tokens"]] == list(ids)
    end = 0
    for (k, f0, f1, lp), (s0, s1) in zip(rec["tokens"], rec["token_seconds"]):
        assert end <= f0 < f1 <= n
        end = f1
        assert _close(lp, float(logp[f0:f1, k].sum()))
        assert s0 == f0 * 0.04 and s1 == f1 * 0.04
    assert sum(t[3] for t in rec["tokens"]) >= rec["score"] - 1e-4 * abs(rec["score"]) - 1e-5          # the blank frames only take probability away
    assert "words" not in rec                                                                            # no tokenizer
