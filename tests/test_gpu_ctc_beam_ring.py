"""Ring mode of the streaming CTC beam search on the device (avec_ctc_beam_stream_ring, ops.ctc_beam_stream_ring, CTCBeamSearchDecoder.stream(window=N)):
against the fp64 oracle of tests/ctc_beam_ring_oracle.py (scores to 1e-4 relative + 1e-5, everything else exact, utterances whose oracle gap is <= 1e-4 skipped as
in tests/test_gpu_ctc_beam.py), and torch.equal for everything that must not depend on how the stream is cut into pushes or must equal what exists."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctc_beam_oracle as O  # noqa: E402
import ctc_beam_ring_oracle as R  # noqa: E402
from avec_amd import ngram, ops  # noqa: E402
from test_gpu_ctc_beam import GAP, _close, _ragged  # noqa: E402

pytestmark = pytest.mark.gpu
TMP = 1.5
OUT = ("tokens", "frames", "out_len", "score", "ctc_logp", "stable_len", "info", "log")
# seeds picked on the CPU oracle, where they leave 7 or 8 of the 8 utterances with a gap above 1e-4 both after 57 and after 100 frames (6 are needed); seed 3100
# leaves 6 at (16, 16) without an LM and 5 with the order-6 one.  Beams dropped per utterance: 42-85 at (16, 16), 12-32 at (4, 8), 631-785 at (16, 2)
SEEDS = {(16, 16, None): 3101, (16, 16, 3): 3100, (16, 16, 6): 3101, (4, 8, None): 3100, (4, 8, 3): 3100, (4, 8, 6): 3100, (16, 2, None): 3100, (16, 2, 3): 3100,
         (16, 2, 6): 3100}


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """{order: (NGramLM, DictLM)} over V = 32 from random ARPA files, written once"""
    d = tmp_path_factory.mktemp("arpa")
    out = {None: (None, None)}
    for order in (3, 6):
        p = str(d / ("lm%d.arpa" % order))
        want, _ = O.write_random_arpa(p, V=32, order=order, n_per_order=3000, seed=order * 7 + 32)
        out[order] = (ngram.NGramLM(p, 32), O.DictLM(want, order, 32))
    return out


def _chunk(logits, off, Tc):
    """frames [off, off + Tc) of every utterance, zero-padded past the end"""
    B, T, V = logits.shape
    c = torch.zeros(B, Tc, V, device=logits.device)
    n = max(0, min(Tc, T - off))
    c[:, :n] = logits[:, off:off + n]
    return c


def _snap(st):
    return {name: getattr(st, name).clone() for name in OUT}


def _run(logits, lens, W, window, schedule, lm=None, log_frames=128, emit_all=True, st=None, first_reset=True):
    """push `schedule` (utterance b takes min(Tc, remaining) frames per push) -> (state, {frames offered so far, capped at T: a snapshot of every output and the log})"""
    B, T, V = logits.shape
    st = ops.CTCBeamRingState(B, W, window, log_frames) if st is None else st
    off, snaps = 0, {}
    for i, Tc in enumerate(schedule):
        emit = emit_all or i == len(schedule) - 1
        out = ops.ctc_beam_stream_ring(st, _chunk(logits, off, Tc), (lens - off).clamp(0, Tc), st.reset_flags.fill_(1) if i == 0 and first_reset else None, TMP, lm,
                                       emit=emit)
        off += Tc
        assert (out is None) == (not emit)
        hdr = st.header()
        assert bool(((hdr[:, 1] - hdr[:, 4] <= window) & (hdr[:, 4] >= 0)).all())          # t - base <= window after every push
        if emit:
            assert torch.equal(hdr[:, 4:], st.info)
            snaps[min(off, T)] = _snap(st)
    return st, snaps


def _same(a, b, what):
    for name in OUT:
        assert torch.equal(a[name], b[name]), (what, name)


def _committed(snap, b):
    cc, log = int(snap["info"][b, 1]), snap["log"][b].tolist()
    assert cc <= len(log)
    return [tuple(log[k]) for k in range(cc)]


# ---- against the oracle ----------------------------------------------------------------------------------------------------------------------------------
def _check_snapshot(snap, refs, W, window):
    checked = 0
    for b, r in enumerate(refs):
        if r.gap <= GAP:
            continue
        checked += 1
        assert snap["info"][b].tolist() == [r.base, len(r.committed), r.dropped, r.commits], b
        assert _committed(snap, b) == r.committed, b
        tok, frm, ol = snap["tokens"][b].tolist(), snap["frames"][b].tolist(), snap["out_len"][b].tolist()
        for w in range(W):
            if w < len(r.beams):
                tail, frames = r.tails[w]
                assert ol[w] == len(tail) and tok[w][:ol[w]] == tail and frm[w][:ol[w]] == frames, (b, w)
                assert [c for c, _ in r.committed] + tail == r.beams[w][0]
                assert _close(float(snap["score"][b, w]), r.beams[w][1]) and _close(float(snap["ctc_logp"][b, w]), r.beams[w][2]), (b, w)
            else:
                assert ol[w] == 0 and float(snap["score"][b, w]) == -np.inf
            assert not any(tok[w][ol[w]:]) and not any(frm[w][ol[w]:])
        tails = [t for t, _ in r.tails]
        n = 0
        while n < min(len(t) for t in tails) and all(t[n] == tails[0][n] for t in tails):
            n += 1
        assert int(snap["stable_len"][b]) == len(r.committed) + n, b
    return checked


@pytest.mark.parametrize("order", [None, 3, 6])
@pytest.mark.parametrize("W,window", [(16, 16), (4, 8), (16, 2)])
def test_ring_matches_oracle(lms, W, window, order):
    B, T, V = 8, 100, 32
    logits = O.ctc_like_logits(B, T, V, seed=SEEDS[(W, window, order)])
    lm, dlm = lms[order]
    ref = [R.beam_search_windowed(O.log_softmax64(logits[b], TMP), T, W, window, lm=dlm, per_frame=True) for b in range(B)]
    for r in ref:                                            # otherwise the case tests nothing
        assert r[T].dropped > 0 and r[T].commits >= 5
    _, snaps = _run(torch.from_numpy(logits).cuda(), torch.full((B,), T, dtype=torch.int64).cuda(), W, window, [57, 43], lm)
    for t in (57, T):
        checked = _check_snapshot(snaps[t], [r[t] for r in ref], W, window)
        print("W %d window %d order %s, %d frames: %d of %d utterances checked" % (W, window, order, t, checked, B))
        assert checked >= 0.75 * B, "only %d of %d utterances have an oracle gap above %g after %d frames" % (checked, B, GAP, t)


# ---- split invariance ------------------------------------------------------------------------------------------------------------------------------------
SCHEDULES = {"4": [4] * 25, "7": [7] * 15, "irregular": [3, 1, 11, 2, 13, 40, 5, 25], "100": [100]}
_frame_by_frame = {}


def _reference(key, logits, lens, W, window, lm):
    """the snapshots of the frame-by-frame schedule, one per frame count: computed once per input, shared by the schedules, never modified"""
    if key not in _frame_by_frame:
        _frame_by_frame[key] = _run(logits, lens, W, window, [1] * logits.shape[1], lm)[1]
    return _frame_by_frame[key]


def _split_case(order, lms):
    B, T, V, W, window = 5, 100, 32, 8, 16
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=B + T + 3000)).cuda()
    lens = torch.from_numpy(_ragged(B, T, seed=V)).cuda()
    assert lens.tolist()[0] == T and lens.tolist()[1] == 0 and lens.tolist()[-1] == 1
    return logits, lens, W, window, lms[order][0]


@pytest.mark.parametrize("order", [None, 6])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_any_split_gives_the_same_bits(lms, order, schedule):
    logits, lens, W, window, lm = _split_case(order, lms)
    ref = _reference(("ragged", order), logits, lens, W, window, lm)
    assert int(ref[100]["info"][0, 3]) >= 10 and int(ref[100]["info"][0, 2]) > 0 and ref[100]["info"][1].tolist() == [0, 0, 0, 0]
    _, snaps = _run(logits, lens, W, window, SCHEDULES[schedule], lm)
    assert 100 in snaps
    for t, s in snaps.items():                               # every common frame count at which both emit, the last one among them
        _same(s, ref[t], (schedule, t))
    _, quiet = _run(logits, lens, W, window, SCHEDULES[schedule], lm, emit_all=False)
    _same(quiet[100], ref[100], (schedule, "silent"))


def test_beam_limit_w64_any_split():
    B, T, V, W, window = 2, 48, 40, 64, 16
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=5)).cuda()
    lens = torch.tensor([T, T - 3]).cuda()
    ref = _reference(("w64",), logits, lens, W, window, None)
    assert int(ref[T]["info"][0, 3]) == 4 and int(ref[T]["info"][0, 2]) > 0
    for schedule in ([5] * 10, [T]):
        for t, s in _run(logits, lens, W, window, schedule)[1].items():
            _same(s, ref[t], (schedule, t))


# ---- equals what exists ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [None, 3])
def test_up_to_the_window_it_is_the_bounded_stream(lms, order):
    B, T, V, W, window = 5, 32, 32, 8, 32
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=21)).cuda()
    lens = torch.from_numpy(_ragged(B, T, seed=22)).cuda()
    lm = lms[order][0]
    ring, bounded = ops.CTCBeamRingState(B, W, window, 64), ops.CTCBeamStreamState(B, W, window)
    for i, off in enumerate(range(0, T, 4)):
        chunk, take = _chunk(logits, off, 4), (lens - off).clamp(0, 4)
        tokens, frames, out_len, score, ctc_logp, stable_len, info = ops.ctc_beam_stream_ring(ring, chunk, take, ring.reset_flags.fill_(1) if i == 0 else None, TMP, lm)
        want = ops.ctc_beam_stream(bounded, chunk, take, bounded.reset_flags.fill_(1) if i == 0 else None, TMP, lm)
        for got, ref, name in zip((tokens, out_len, score, ctc_logp, stable_len), want, ("tokens", "out_len", "score", "ctc_logp", "stable_len")):
            assert torch.equal(got, ref), (off, name)
        assert not info.any()                                # base = ccount = dropped = commits = 0: nothing was committed
        assert bool((frames < off + 4).all())


@pytest.mark.parametrize("order", [None, 3])
@pytest.mark.parametrize("window", [2, 16])
def test_one_beam_equals_the_offline_search(lms, order, window):
    B, T, V = 5, 100, 32
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=31)).cuda()
    lens = torch.from_numpy(_ragged(B, T, seed=32)).cuda()
    lm = lms[order][0]
    tokens, out_len, score, ctc_logp = ops.ctc_beam_search(logits, lens, 1, TMP, lm)
    _, snaps = _run(logits, lens, 1, window, [9] * 12, lm)
    s = snaps[T]
    assert torch.equal(s["score"], score) and torch.equal(s["ctc_logp"], ctc_logp)
    assert not s["info"][:, 2].any() and int(s["info"][0, 3]) == (T - 1 - window) // (window // 2) + 1
    for b in range(B):
        got = [c for c, _ in _committed(s, b)] + s["tokens"][b, 0, :int(s["out_len"][b, 0])].tolist()
        assert got == tokens[b, 0, :int(out_len[b, 0])].tolist(), b


# ---- stale memory ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_fill", [0, 0xFF])
def test_stale_buffers_give_the_same_results(state_fill):
    B, T, V, W, window = 3, 60, 32, 8, 8
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=41)).cuda()
    lens = torch.tensor([T, T - 7, 2]).cuda()
    _, fresh = _run(logits, lens, W, window, [6] * 10)
    st = ops.CTCBeamRingState(B, W, window, 128)
    st.state.fill_(state_fill)                               # a header this mode did not write: the empty prefix, without a reset flag
    for name in ("backptr", "log", "tokens", "frames", "out_len", "stable_len", "info"):
        getattr(st, name).view(torch.uint8).fill_(0xFF)
    st.score.fill_(float("nan"))
    st.ctc_logp.fill_(float("nan"))
    _, stale = _run(logits, lens, W, window, [6] * 10, st=st, first_reset=False)
    for t in fresh:
        for name in OUT[:-1]:
            assert torch.equal(stale[t][name], fresh[t][name]), (t, name)
        for b in range(B):
            assert _committed(stale[t], b) == _committed(fresh[t], b)
    assert int(fresh[T]["info"][0, 3]) >= 10 and int(fresh[T]["info"][0, 1]) > 0


# ---- the session -----------------------------------------------------------------------------------------------------------------------------------------
def _decoder(W, **kw):
    import warnings

    import nnet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return nnet.CTCBeamSearchDecoder(beam_size=W, ngram_tmp=TMP, **kw)


def _session_run(dec, logits, Tc, fetch_every=1, reset_at=None, **kw):
    """push logits in chunks of Tc -> (session, the records of every fetching push, the state header after every push)"""
    B, T, _ = logits.shape
    s = dec.stream(B, **kw)
    recs, hdrs = {}, []
    for i, off in enumerate(range(0, T, Tc)):
        r = s.push(logits[:, off:off + Tc].contiguous(), reset=[1] if reset_at == i else None, fetch=(i + 1) % fetch_every == 0 or off + Tc >= T)
        if r is not None:
            recs[off + Tc] = r
        hdrs.append(s.state.header().clone())
    return s, recs, hdrs


def test_unbounded_session_and_mid_stream_reset():
    B, V, W, window, Tc = 3, 32, 8, 16, 8
    T = 8 * window
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=51)).cuda()
    dec = _decoder(W)
    bounded = dec.stream(B, window)                          # the bounded session stops at its max_frames
    bounded.push(logits[:, :Tc].contiguous())
    bounded.push(logits[:, Tc:2 * Tc].contiguous())
    with pytest.raises(RuntimeError, match="max_frames = %d" % window):
        bounded.push(logits[:, 2 * Tc:3 * Tc].contiguous())
    s, recs, hdrs = _session_run(dec, logits, Tc, window=window)
    assert sorted(recs) == list(range(Tc, T + 1, Tc))
    prev = None
    for (t, rec), hdr in zip(sorted(recs.items()), hdrs):
        assert hdr[:, 1].tolist() == [t] * B and bool((hdr[:, 1] - hdr[:, 4] <= window).all())
        for b in range(B):
            r = rec[b]
            assert set(r) == {"committed_ids", "committed_frames", "n_new", "partial_ids", "partial_frames", "stable_ids", "dropped"}
            n = len(r["committed_ids"])
            assert n == int(hdr[b, 5]) and len(r["committed_frames"]) == n and len(r["partial_frames"]) == len(r["partial_ids"])
            assert r["partial_ids"][:n] == r["committed_ids"] and r["stable_ids"] == r["partial_ids"][:len(r["stable_ids"])] and len(r["stable_ids"]) >= n
            assert r["partial_frames"] == sorted(set(r["partial_frames"])) and all(f < int(hdr[b, 4]) for f in r["committed_frames"])
            assert r["dropped"] == int(hdr[b, 6])
            if prev is not None:                             # ccount, stable_len and base never decrease; what was reported as committed stays
                p = prev[0][b]
                assert r["committed_ids"][:len(p["committed_ids"])] == p["committed_ids"] and r["n_new"] == n - len(p["committed_ids"])
                assert len(r["stable_ids"]) >= len(p["stable_ids"]) and int(hdr[b, 4]) >= int(prev[1][b, 4])
                assert r["stable_ids"][:len(p["stable_ids"])] == p["stable_ids"]
            else:
                assert r["n_new"] == n
        prev = (rec, hdr)
    last = recs[T]
    assert all(sum(recs[t][b]["n_new"] for t in recs) == len(last[b]["committed_ids"]) > 0 for b in range(B))
    assert int(hdrs[-1][0, 7]) == (T - 1 - window) // (window // 2) + 1 and all(r["dropped"] > 0 for r in last)
    assert s.finish() == [r["partial_ids"] for r in last]
    # slot 1 restarts before push 7: it equals a stream of its own frames from there, the other slots equal the run without the reset
    s2, recs2, hdrs2 = _session_run(dec, logits, Tc, window=window, reset_at=7)
    assert recs2[7 * Tc] == recs[7 * Tc]
    for t in range(8 * Tc, T + 1, Tc):
        for b in (0, 2):
            assert recs2[t][b] == recs[t][b], (t, b)
    assert len(recs2[8 * Tc][1]["committed_ids"]) == 0 and int(hdrs2[7][1, 1]) == Tc and hdrs2[7][1, 4:].tolist() == [0, 0, 0, 0]
    for name in ("tokens", "frames", "out_len", "score", "ctc_logp", "stable_len", "info"):
        assert torch.equal(getattr(s2.state, name)[[0, 2]], getattr(s.state, name)[[0, 2]]), name
    s3, recs3, _ = _session_run(dec, logits[1:2, 7 * Tc:].contiguous(), Tc, window=window)
    for t in recs3:
        assert recs3[t][0] == recs2[7 * Tc + t][1], t
    assert len(recs3[T - 7 * Tc][0]["committed_ids"]) > 0


def test_silent_pushes_past_the_log_lose_nothing(monkeypatch):
    import nnet
    B, V, W, window, Tc = 3, 32, 8, 16, 8
    T = 8 * window
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=51)).cuda()
    dec = _decoder(W)
    _, loud, _ = _session_run(dec, logits, Tc, window=window)
    want = loud[T]
    assert len(want[0]["committed_ids"]) > 40                # more than the small logs below hold at once
    drains, drain = [], nnet.CTCBeamRingStreamSession._drain
    monkeypatch.setattr(nnet.CTCBeamRingStreamSession, "_drain", lambda self, extra=(): (drains.append(len(extra)), drain(self, extra))[1])
    for kw in (dict(fetch_every=1000, log_frames=40), dict(fetch_every=5, log_frames=17)):        # the session reads the log on its own, with fetch=False too
        del drains[:]
        _, recs, _ = _session_run(dec, logits, Tc, window=window, **kw)
        got = recs[T]
        assert drains.count(0) >= 2, drains                  # reads that no fetch asked for
        for b in range(B):
            assert {k: v for k, v in got[b].items() if k != "n_new"} == {k: v for k, v in want[b].items() if k != "n_new"}, b
    # one push of the whole stream, longer than the log: consumed in pieces
    s = dec.stream(B, window=window, log_frames=40)
    got = s.push(logits)
    for b in range(B):
        assert {k: v for k, v in got[b].items() if k != "n_new"} == {k: v for k, v in want[b].items() if k != "n_new"}, b
        assert got[b]["n_new"] == len(want[b]["committed_ids"])


def test_finish_goes_through_the_neural_rescorer(tmp_path, monkeypatch):
    import make_synthetic_lm_assets as A
    B, T, V, W, window, Tc = 4, 64, 64, 8, 16, 7
    arpa = str(tmp_path / "lm.arpa")
    O.write_random_arpa(arpa, V=V, order=3, n_per_order=500, seed=2)
    monkeypatch.setenv("AVEC_TEST_LM_DIR", str(tmp_path))
    cfg = A.load_config(os.path.join(ROOT, "tests", "configs", "lm_synthetic.py"))
    A.write_checkpoint(A.draw_weights(cfg.model, seed=11, head_std=3.0), str(tmp_path / "lm.ckpt"))
    dec = _decoder(W, ngram_path=arpa, ngram_alpha=0.6, ngram_beta=1.0, neural_config_path=os.path.join(ROOT, "tests", "configs", "lm_synthetic.py"),
                   neural_checkpoint="lm.ckpt", neural_alpha=0.6, neural_beta=1.0)
    assert dec.neural_rescorer is not None
    logits = torch.from_numpy(O.ctc_like_logits(B, T, V, seed=70)).cuda()
    s, recs, _ = _session_run(dec, logits, Tc, fetch_every=3, window=window)
    st, last = s.state, recs[max(recs)]
    assert all(len(r["committed_ids"]) > 0 for r in last)
    # committed ++ tail of every beam, assembled here from the state and the records
    tails, lens = st.tokens.cpu().tolist(), st.out_len.cpu().tolist()
    hyps = [[last[b]["committed_ids"] + tails[b][w][:lens[b][w]] if float(st.score[b, w]) > -np.inf else [] for w in range(W)] for b in range(B)]
    L = max(len(h) for hb in hyps for h in hb)
    tokens, out_len = torch.zeros(B, W, L, dtype=torch.int32), torch.zeros(B, W, dtype=torch.int32)
    for b in range(B):
        for w in range(W):
            tokens[b, w, :len(hyps[b][w])] = torch.tensor(hyps[b][w], dtype=torch.int32)
            out_len[b, w] = len(hyps[b][w])
    want = dec._rescore(tokens, out_len, st.score, B, 1)
    totals = dec.last_totals.clone()
    assert s.finish() == want and torch.equal(dec.last_totals, totals)
    assert all(h in hyps[b] for b, h in enumerate(want))
