"""Streaming CTC beam search on the device (avec_ctc_beam_stream, ops.ctc_beam_stream, CTCBeamSearchDecoder.stream) against the offline search
(ops.ctc_beam_search, itself pinned to the fp64 oracle by tests/test_gpu_ctc_beam.py).  Every frame does the same arithmetic in the same order whether it
arrives alone or with the whole utterance, so every comparison here is torch.equal: there is no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_beam_oracle as O  # noqa: E402
from avec_amd import ngram, ops  # noqa: E402

pytestmark = pytest.mark.gpu
TMP = 1.5
SCHEDULES = {"1": [1] * 30, "4": [4] * 8, "7": [7] * 5, "30": [30], "irregular": [3, 1, 11, 2, 13]}


def _ragged(B, T, seed):
    g = np.random.default_rng(seed)
    lens = g.integers(T // 2, T + 1, size=B)
    lens[0], lens[1 % B], lens[-1] = T, 0, 1
    return lens


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """{(order, V): NGramLM} of random ARPA files, written once"""
    d = tmp_path_factory.mktemp("arpa")
    out = {}
    for order, V in ((3, 32), (6, 32), (6, 256)):
        p = str(d / ("lm%d_%d.arpa" % (order, V)))
        O.write_random_arpa(p, V=V, order=order, n_per_order=3000, seed=order * 7 + V)
        out[(order, V)] = ngram.NGramLM(p, V)
    return out


_offline_cache = {}


def _offline(key, logits, lens, W, lm):
    """{t: the offline W-best on frames [0, t)} for every t, computed once per input and shared by the schedules (never modified)"""
    if key not in _offline_cache:
        T = logits.shape[1]
        _offline_cache[key] = {t: ops.ctc_beam_search(logits[:, :t].contiguous(), lens.clamp(max=t), W, TMP, lm) for t in range(1, T + 1)}
    return _offline_cache[key]


def _chunk(logits, off, Tc):
    """frames [off, off + Tc) of every utterance, zero-padded past the end"""
    B, T, V = logits.shape
    c = torch.zeros(B, Tc, V, device=logits.device)
    n = max(0, min(Tc, T - off))
    c[:, :n] = logits[:, off:off + n]
    return c


def _same_as_offline(st, ref, t):
    tokens, out_len, score, ctc_logp = ref
    assert torch.equal(st.tokens[..., :t], tokens) and not st.tokens[..., t:].any()
    assert torch.equal(st.out_len, out_len) and torch.equal(st.score, score) and torch.equal(st.ctc_logp, ctc_logp)


def _run(logits, lens, W, schedule, lm, ref, Tcap=None, emit_all=True):
    """push `schedule`; utterance b takes min(Tc, remaining) frames per push.  Checks every emitting push against the offline search on the frames so far."""
    B, T, V = logits.shape
    st = ops.CTCBeamStreamState(B, W, T if Tcap is None else Tcap)
    off = 0
    for i, Tc in enumerate(schedule):
        take = (lens - off).clamp(0, Tc)
        emit = emit_all or i == len(schedule) - 1
        out = ops.ctc_beam_stream(st, _chunk(logits, off, Tc), take, st.reset_flags.fill_(1) if i == 0 else None, TMP, lm, emit=emit)
        off += Tc
        assert (out is None) == (not emit)
        if emit:
            _same_as_offline(st, ref[min(off, T)], min(off, T))
    return st


@pytest.mark.parametrize("order", [None, 3, 6])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_chunked_equals_offline_after_every_push(lms, order, schedule):
    B, T, V, W = 5, 30, 32, 8
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=B + T + 3000)).cuda()
    lens = torch.from_numpy(_ragged(B, T, seed=V)).cuda()
    assert lens.tolist()[0] == T and lens.tolist()[1] == 0 and lens.tolist()[-1] == 1
    lm = None if order is None else lms[(order, V)]
    ref = _offline(("ragged", order), logits, lens, W, lm)
    _run(logits, lens, W, SCHEDULES[schedule], lm, ref)


def test_wide_vocabulary_order6_beams_over_several_waves(lms):
    B, T, V, W = 4, 40, 256, 16                            # four tokens per lane, 16 beams over the 8 waves
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=77)).cuda()
    lens = torch.from_numpy(_ragged(B, T, seed=78)).cuda()
    ref = _offline(("wide",), logits, lens, W, lms[(6, V)])
    _run(logits, lens, W, [8] * 5, lms[(6, V)], ref, Tcap=T + 3)      # a capacity that is not the utterance length


def test_beam_limit_w64():
    B, T, V, W = 2, 12, 40, 64
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=5)).cuda()
    lens = torch.tensor([T, T - 3]).cuda()
    ref = _offline(("w64",), logits, lens, W, None)
    _run(logits, lens, W, [5, 5, 5], None, ref)            # the last push holds 2 frames


def test_silent_pushes_then_one_emit(lms):
    B, T, V, W = 5, 30, 32, 8
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=B + T + 3000)).cuda()
    lens = torch.from_numpy(_ragged(B, T, seed=V)).cuda()
    lm = lms[(3, V)]
    ref = _offline(("ragged", 3), logits, lens, W, lm)
    loud = _run(logits, lens, W, SCHEDULES["irregular"], lm, ref)
    quiet = _run(logits, lens, W, SCHEDULES["irregular"], lm, ref, emit_all=False)
    for name in ("tokens", "out_len", "score", "ctc_logp", "stable_len"):
        assert torch.equal(getattr(loud, name), getattr(quiet, name)), name


def _common_prefix(tokens, out_len, score):
    """per utterance the length of the longest common prefix of the live beams (score > -inf) of an offline result"""
    out = []
    for tk, ol, sc in zip(tokens.tolist(), out_len.tolist(), score.tolist()):
        hyps = [tk[w][:ol[w]] for w in range(len(sc)) if sc[w] > float("-inf")]
        n = 0
        while n < min(len(h) for h in hyps) and all(h[n] == hyps[0][n] for h in hyps):
            n += 1
        out.append(n)
    return out


def test_stable_prefix_is_the_common_prefix_and_final():
    B, T, V, W = 5, 30, 32, 8
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=11, peak=6)).cuda()
    lens = torch.full((B,), T, dtype=torch.int64).cuda()
    ref = _offline(("stable",), logits, lens, W, None)
    st = ops.CTCBeamStreamState(B, W, T)
    stable, best = [], []
    for t in range(T):
        _, out_len, _, _, sl = ops.ctc_beam_stream(st, logits[:, t:t + 1].contiguous(), None, st.reset_flags.fill_(1) if t == 0 else None, TMP)
        tokens, rol, score, _ = ref[t + 1]
        assert sl.tolist() == _common_prefix(tokens, rol, score), t
        stable.append([st.tokens[b, 0, :n].tolist() for b, n in enumerate(sl.tolist())])
        best.append(out_len[:, 0].tolist())
    final = [st.tokens[b, 0, :n].tolist() for b, n in enumerate(st.out_len[:, 0].tolist())]
    positive = shorter = 0
    for b in range(B):
        for t in range(T):
            n = len(stable[t][b])
            assert t == 0 or n >= len(stable[t - 1][b]), (b, t)              # never decreases
            assert stable[t][b] == final[b][:n], (b, t)                      # what was called final stayed
            positive += n > 0
            shorter += n < best[t][b]
    print("stable_len > 0 at %d of %d points, shorter than the best hypothesis at %d" % (positive, B * T, shorter))      # fp64 oracle: 90 and 148 of 150
    assert positive >= B * T / 3 and shorter >= 1


def test_slots_are_independent_and_runs_repeat():
    """slot 1 ends one utterance and starts another while slot 0 goes on: each equals the offline search of its own logits; reset by index == reset by mask"""
    import nnet
    V, W, Tc = 32, 8, 4
    a = torch.from_numpy(O.ctc_like_logits(1, 20, V, seed=1)).cuda()
    x = torch.from_numpy(O.ctc_like_logits(1, 8, V, seed=2)).cuda()
    y = torch.from_numpy(O.ctc_like_logits(1, 12, V, seed=3)).cuda()
    slot1 = torch.cat([x, y], 1)
    dec = nnet.CTCBeamSearchDecoder(beam_size=W, ngram_tmp=TMP)
    full = lambda lg: ops.ctc_beam_search(lg, torch.tensor([lg.shape[1]]).cuda(), W, TMP)      # noqa: E731
    runs = []
    for reset in ([1], [False, True]):
        s = dec.stream(2, 20)
        snap = {}
        for i in range(5):
            recs = s.push(torch.cat([a[:, 4 * i:4 * i + Tc], slot1[:, 4 * i:4 * i + Tc]], 0), reset=reset if i == 2 else None)
            snap[i] = [t.clone() for t in (s.state.tokens, s.state.out_len, s.state.score, s.state.ctc_logp, s.state.stable_len)]
            assert all(r["stable_ids"] == r["partial_ids"][:len(r["stable_ids"])] for r in recs)
        runs.append(snap)
        for i, lg in ((1, x), (4, y)):                      # slot 1: utterance x after two pushes, utterance y after three more
            tokens, out_len, score, ctc_logp = full(lg)
            t = lg.shape[1]
            assert torch.equal(snap[i][0][1, :, :t], tokens[0]) and not snap[i][0][1, :, t:].any()
            assert torch.equal(snap[i][1][1], out_len[0]) and torch.equal(snap[i][2][1], score[0]) and torch.equal(snap[i][3][1], ctc_logp[0])
        tokens, out_len, score, ctc_logp = full(a)
        assert torch.equal(snap[4][0][0], tokens[0]) and torch.equal(snap[4][1][0], out_len[0]) and torch.equal(snap[4][2][0], score[0])
        assert s.finish() == [tokens[0, 0, :int(out_len[0, 0])].tolist(), full(y)[0][0, 0, :int(full(y)[1][0, 0])].tolist()]
    for i in range(5):
        for p, q in zip(runs[0][i], runs[1][i]):
            assert torch.equal(p, q), i


@pytest.mark.parametrize("neural", [False, True])
def test_decoder_stream_equals_beam_search(tmp_path, monkeypatch, neural):
    import nnet
    B, T, V, W, Tc = 6, 40, 64, 8, 7
    arpa = str(tmp_path / "lm.arpa")
    O.write_random_arpa(arpa, V=V, order=3, n_per_order=500, seed=2)
    kw = {}
    if neural:                                              # the rescorer of tests/test_gpu_lm_rescore.py
        import make_synthetic_lm_assets as A
        monkeypatch.setenv("AVEC_TEST_LM_DIR", str(tmp_path))
        cfg = A.load_config(os.path.join(ROOT, "tests", "configs", "lm_synthetic.py"))
        A.write_checkpoint(A.draw_weights(cfg.model, seed=11, head_std=3.0), str(tmp_path / "lm.ckpt"))
        kw = dict(neural_config_path=os.path.join(ROOT, "tests", "configs", "lm_synthetic.py"), neural_checkpoint="lm.ckpt", neural_alpha=0.6, neural_beta=1.0)
    dec = nnet.CTCBeamSearchDecoder(beam_size=W, ngram_path=arpa, ngram_tmp=1.2, ngram_alpha=0.6, ngram_beta=1.0, **kw)
    assert (dec.neural_rescorer is not None) == neural
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=70)).cuda()
    lens = torch.from_numpy(_ragged(B, T, seed=80)).cuda()
    want = dec.beam_search(logits, lens)
    totals = dec.last_totals.clone() if neural else None
    s = dec.stream(B, T + 2)
    for off in range(0, T, Tc):
        recs = s.push(_chunk(logits, off, Tc), (lens - off).clamp(0, Tc), fetch=off % (2 * Tc) == 0)
        if recs is not None:
            seen = lens.clamp(max=off + Tc)
            tokens, out_len, _, _ = ops.ctc_beam_search(logits[:, :off + Tc].contiguous() if off + Tc <= T else logits, seen, W, 1.2, dec.lm(V), 0.6, 1.0)
            assert [r["partial_ids"] for r in recs] == [tokens[b, 0, :int(out_len[b, 0])].tolist() for b in range(B)]
            assert all(r["stable_ids"] == r["partial_ids"][:len(r["stable_ids"])] for r in recs)
    assert s.finish() == want
    if neural:
        assert torch.equal(dec.last_totals, totals)
    # T + 2 frames of capacity, 6 pushes of 7 counted: one more frame does not fit, and nothing is launched for it
    calls = []
    stream = ops.ctc_beam_stream
    monkeypatch.setattr(ops, "ctc_beam_stream", lambda *a, **k: (calls.append(1), stream(*a, **k))[1])
    with pytest.raises(RuntimeError, match="max_frames"):
        s.push(_chunk(logits, 0, 1))
    assert not calls and s.finish() == want
    with pytest.raises(NotImplementedError, match="test_time_aug"):
        nnet.CTCBeamSearchDecoder(beam_size=W, ngram_path=arpa, test_time_aug=True).stream(B, T)
