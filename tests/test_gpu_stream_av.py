"""GPU (-m gpu): AudioVisualEfficientConformerEncoder.stream() -- video and waveform chunks to logits -- against the CPU oracle on each WHOLE utterance.

The model is tests/av_stream_ref.make_av_enc(): AudioVisualEfficientConformerEncoder(vocab_size=16) with both back-ends, the fusion module, the fusion stack and the head
replaced by small causal ones at width 48 (Mask(left_context=6, right_context=0), K = 15 causal, one InterCTC module per stack: v_ctc_0, a_ctc_1, f_ctc_0; video stack
stride 2, audio stack stride 4), seeded weights, running statistics that are not the identity, eval mode.  88x88 frames, B = 3 slots, Tv = 4 (R = 2 rows per push,
rings of 4 rows); utterances of T = 1 .. 11 video frames with 640 T - 160 samples on the session's schedule; slots 1 and 2 end their first utterance, are restarted and
fed a second one (slot 2 a third).  6, 5 and 10 frames end in different pushes (the video branch one push before the audio branch), 11, 1 and 3 in the same push.

f32 and bf16: the logits and the three families of InterCTC logits per utterance against the oracle composed as oracle.av_forward composes it (visual_frontend,
mel_frontend + audio_stem, conformer_interctc(context=(6, 0, 0), causal_conv=True) three times, the fusion module, the head).  The bound is measured in the test: the
offline GPU forward of the same module on the whole utterance (B = 1) is compared with the same oracle, and the streamed result may be at most 2 x that.  Lengths are
exact.  Measured on MI355X: DESIGN section 35.
"""
import functools

import pytest
import torch

from oracle import avec_oracle as O
from tests import av_stream_ref as AR
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
UTTS = [[11], [6, 5], [1, 10, 3]]
TV, R, HW = 4, 2, 88
KEYS = AR.KEYS
CTX = dict(context=(6, 0, 0), causal_conv=True)


def oracle_rows(sd, data):
    """the oracle, composed as oracle.av_forward composes it, on every utterance of data[b][utterance] = (video, wave) -> ({"logits" / InterCTC key: rows}, rows)"""
    ref = []
    for ub in data:
        row = []
        for x, w in ub:
            T = x.shape[0]
            with torch.no_grad():
                v = O.visual_frontend(sd, "m.video_encoder.front_end", x[None, None], False, {})
                v, vlen, v_inter = O.conformer_interctc(sd, "m.video_encoder.back_end", v, torch.tensor([T]), AR.V_BLOCKS[0], AR.V_BLOCKS[1], "v_ctc", [1, 1], False, {}, **CTX)
                mel, alen = O.mel_frontend(w[None], torch.tensor([w.shape[0]]))
                a, alen = O.audio_stem(sd, "m.audio_encoder", mel, alen, False, {})
                a, alen, a_inter = O.conformer_interctc(sd, "m.audio_encoder.back_end", a, alen, AR.A_BLOCKS[0], AR.A_BLOCKS[1], "a_ctc", [1, 1, 1], False, {}, **CTX)
                f = torch.cat([a, v], dim=-1)
                f = O.linear(sd, "m.fusion_module.layers.2", O.swish(O.linear(sd, "m.fusion_module.layers.0", f)))
                f, flen, f_inter = O.conformer_interctc(sd, "m.audio_visual_encoder", f, alen, AR.F_BLOCKS[0], AR.F_BLOCKS[1], "f_ctc", [1], False, {}, **CTX)
                logits = O.linear(sd, "m.head", f)
            n = -(-T // 2)
            inter = {**v_inter, **a_inter, **f_inter}
            assert int(vlen[0]) == int(alen[0]) == int(flen[0]) == n and sorted(inter) == sorted(KEYS) and all(int(inter[k][1][0]) == n for k in KEYS)
            row.append(({"logits": logits[0], **{k: inter[k][0][0] for k in KEYS}}, n))
        ref.append(row)
    return ref


@functools.lru_cache(maxsize=1)
def state_dict():
    return {"m." + k: v.detach().clone() for k, v in AR.make_av_enc().state_dict().items()}


@functools.lru_cache(maxsize=1)
def fixture():
    """(data[b][utterance] = (video [T][H][W], wave [640 T - 160]), oracle results per (slot, utterance)) -- computed once"""
    g = torch.Generator().manual_seed(7)
    data = [[(0.5 * torch.randn(T, HW, HW, generator=g), 0.1 * torch.randn(640 * T - 160, generator=g)) for T in ut] for ut in UTTS]
    return data, oracle_rows(state_dict(), data)


def gpu_enc(dtype):
    import avec_amd
    avec_amd.set_compute_dtype(dtype)
    return AR.make_av_enc().to("cuda").eval()


def pushes(ses, data):
    """per push and slot (utterance index or None, first frame, first sample, n_frames, n_samples, last_video, last_audio, restart)"""
    queue = []
    for ub in data:
        q = []
        for ui, (x, w) in enumerate(ub):
            vat = aat = 0
            for i, (nf, ns, lv, la) in enumerate(ses.schedule(x.shape[0], w.shape[0])):
                q.append((ui, vat, aat, nf, ns, lv, la, i == 0))
                vat, aat = vat + nf, aat + ns
        queue.append(q)
    n = max(len(q) for q in queue)
    return [[q[i] if i < len(q) else (None, 0, 0, 0, 0, False, False, False) for q in queue] for i in range(n)]


def inputs_of(data, row, ses):
    v = torch.full((len(row), ses.first_frames, HW, HW), float("nan"))       # frames / samples at or past the counts are never read into a valid output
    w = torch.full((len(row), ses.first_samples), float("nan"))
    for b, (ui, vat, aat, nf, ns, _, _, _) in enumerate(row):
        if ui is not None:
            v[b, :nf], w[b, :ns] = data[b][ui][0][vat:vat + nf], data[b][ui][1][aat:aat + ns]
    return v.cuda(), w.cuda()


def streamed(enc, utts=UTTS, data=None, capture=False, sync_free=False, beam=None):
    """-> per (slot, utterance) {"logits" / InterCTC key: rows}, the per-push raw outputs, the row count of every push's logits"""
    data = fixture()[0] if data is None else data
    B = len(utts)
    ses = enc.stream(B, TV)
    if capture:
        ses.capture(frame=(HW, HW))
    assert (ses.R, ses.cap, ses.first_frames, ses.first_samples) == (R, R + 2, TV + 2, 640 * TV + 40)
    got, raw, widths = [[{k: [] for k in ("logits",) + KEYS} for _ in ut] for ut in utts], [], []
    assert [[x.shape[0] for x, _ in ub] for ub in data] == [list(ut) for ut in utts]
    for pi, row in enumerate(pushes(ses, data)):
        v, w = inputs_of(data, row, ses)
        ctl = ([r[3] for r in row], [r[4] for r in row], [b for b, r in enumerate(row) if r[5]] or None, [b for b, r in enumerate(row) if r[6]] or None,
               [b for b, r in enumerate(row) if r[7]] or None)
        if sync_free and pi > 0:
            torch.cuda.set_sync_debug_mode("error")
        try:
            logits, olen, inter = ses.push(v, w, *ctl)
            if beam is not None:
                beam.push(logits.contiguous(), olen, ctl[4], fetch=False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert sorted(inter) == sorted(KEYS) and logits.dtype == torch.float32 and logits.shape[0] == B and logits.shape[2] == 16
        assert inter["f_ctc_0"][0].shape[1] == logits.shape[1] and R <= logits.shape[1] <= 2 * R
        rec = {"logits": (logits.clone(), olen.clone()), **{k: (inter[k][0].clone(), inter[k][1].clone()) for k in KEYS}}
        raw.append(rec)
        widths.append(logits.shape[1])
        assert torch.equal(olen, inter["f_ctc_0"][1])
        for b, r in enumerate(row):
            if ses._end_a[b] and ses._end_v[b]:                          # the host mirrors of an ended slot: nothing left in either ring
                assert ses._pend_a[b] == ses._pend_v[b] == 0 and ses._rows_a[b] == ses._rows_v[b], (pi, b)
            for k, (t, tl) in rec.items():
                n = int(tl[b])
                assert n <= t.shape[1]
                if r[0] is None:
                    assert n == 0, (pi, b, k, n)
                else:
                    got[b][r[0]][k].append(t[b, :n].float().cpu())
    return [[{k: torch.cat(v) for k, v in g.items()} for g in gb] for gb in got], raw, widths


def offline(enc, data=None, ref=None):
    """the offline GPU forward, one utterance at a time -> per (slot, utterance) {"logits" / InterCTC key: rows}"""
    if data is None:
        data, ref = fixture()
    out = []
    for b, ub in enumerate(data):
        row = []
        for ui, (x, w) in enumerate(ub):
            with torch.no_grad():
                y, ylen, inter = enc(x[None, None].cuda(), torch.tensor([x.shape[0]]).cuda(), w[None].cuda(), torch.tensor([w.shape[0]]).cuda())
            assert int(ylen[0]) == ref[b][ui][1] and all(int(inter[k][1][0]) == ref[b][ui][1] for k in KEYS)
            row.append({"logits": y[0].float().cpu(), **{k: inter[k][0][0].float().cpu() for k in KEYS}})
        out.append(row)
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stream_within_twice_the_offline_error(dtype):
    """measured on MI355X (max over slots and utterances): see DESIGN section 35"""
    _, ref = fixture()
    enc = gpu_enc(dtype)
    try:
        off = offline(enc)
        got, _, widths = streamed(enc)
    finally:
        import avec_amd
        avec_amd.set_compute_dtype("f32")
    assert widths == [R] * len(widths)       # (on 640 T - 160 samples no push brings R + 1 rows in both branches: test_second_fuse_launch has the utterances that do)
    compare(dtype, ref, got, off)


def compare(dtype, ref, got, off):
    bad = []
    for b, ub in enumerate(ref):
        for ui, (want, n) in enumerate(ub):
            for k in ("logits",) + KEYS:
                assert got[b][ui][k].shape == want[k].shape and want[k].shape[0] == n, (b, ui, k, got[b][ui][k].shape, want[k].shape)
                es, eo = rel_err(got[b][ui][k], want[k]), rel_err(off[b][ui][k], want[k])
                print("%s slot %d utterance %d (%d rows) %s: streamed %.3g | offline GPU %.3g" % (dtype, b, ui, n, k, es, eo))
                if not es <= 2 * eo:
                    bad.append((b, ui, k, es, eo))
    assert not bad, bad


def test_second_fuse_launch():
    """utterances whose last push brings R + 1 rows in BOTH branches (6 frames with 2600 samples in one push; 10 frames with 5160 samples in two): the first fuse launch
    emits R pairs, a second one without new rows the pair behind them, and the fusion stack is pushed twice; same oracle, same bound"""
    g = torch.Generator().manual_seed(11)
    data = [[(0.5 * torch.randn(6, HW, HW, generator=g), 0.1 * torch.randn(2600, generator=g))], [(0.5 * torch.randn(10, HW, HW, generator=g), 0.1 * torch.randn(5160, generator=g))],
            [(0.5 * torch.randn(3, HW, HW, generator=g), 0.1 * torch.randn(1760, generator=g))]]
    ref = oracle_rows(state_dict(), data)
    assert [r[0][1] for r in ref] == [3, 5, 2]
    enc = gpu_enc("f32")
    off = offline(enc, data, ref)
    got, raw, widths = streamed(enc, utts=[[6], [10], [3]], data=data)
    assert widths == [R + 1, R + 1] and [r["logits"][1].tolist() for r in raw] == [[3, 2, 2], [0, 3, 0]]
    compare("f32", ref, got, off)
    _, graph, wg = streamed(enc, utts=[[6], [10], [3]], data=data, capture=True)
    assert wg == widths
    for pi, (e, c) in enumerate(zip(raw, graph)):
        for k in e:
            assert torch.equal(e[k][0], c[k][0]) and torch.equal(e[k][1], c[k][1]), (pi, k)


def test_captured_pushes_equal_eager_pushes():
    enc = gpu_enc("f32")
    _, eager, we = streamed(enc)
    _, graph, wg = streamed(enc, capture=True)
    assert we == wg and len(eager) == len(graph) >= 3
    for pi, (e, g) in enumerate(zip(eager, graph)):
        for k in e:
            assert torch.equal(e[k][0], g[k][0]) and torch.equal(e[k][1], g[k][1]), (pi, k)


def test_restarted_slots_reproduce_fresh_sessions():
    enc = gpu_enc("f32")
    data, _ = fixture()
    run, _, _ = streamed(enc)
    fresh, _, _ = streamed(enc, utts=[[11], [5], [10]], data=[[data[0][0]], [data[1][1]], [data[2][1]]])
    for (b, ui) in ((0, 0), (1, 1), (2, 1)):
        for k in ("logits",) + KEYS:
            assert torch.equal(run[b][ui][k], fresh[b][0][k]), (b, ui, k)


def test_pushes_do_not_synchronise_or_grow():
    enc = gpu_enc("f32")
    streamed(enc, sync_free=True)                                       # restarts, branches that end in different pushes and second fuse launches under sync debug mode
    ses = enc.stream(3, TV)
    v, w = 0.5 * torch.randn(3, ses.first_frames, HW, HW, device="cuda"), 0.1 * torch.randn(3, ses.first_samples, device="cuda")
    for kw in (dict(), dict(last_video=[1], last_audio=[1]), dict(reset=[1])):       # (the first tail pushes allocate the branch sessions' second-push inputs once)
        out = ses.push(v, w, **kw)
    del out
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    widths = []
    try:
        for i in range(20):
            last = [1] if i % 10 == 4 else None
            out = ses.push(v, w, None, None, last, last, [1] if i % 10 == 5 else ([i % 3] if i % 7 == 0 else None))
            widths.append(out[0].shape[1])
            del out
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    assert widths == [R + 1 if i % 10 == 4 else R for i in range(20)]           # the pushes that end slot 1 run the second fuse launch and the second stack push
    assert ses._end_a == ses._end_v == [False] * 3 and ses._pend_a == ses._pend_v == [0] * 3 and ses._rows_a == ses._rows_v


def test_streamed_logits_feed_the_streaming_beam_search():
    """chunks -> both branches -> paired rows -> fusion stack -> logits -> beam, one chain of sessions: finish() gives what beam_search gives on the concatenated logits"""
    import nnet
    utts = [[11], [6], [1]]
    data, _ = fixture()
    enc = gpu_enc("f32")
    dec = nnet.CTCBeamSearchDecoder(beam_size=4, ngram_tmp=1.0)
    bs = dec.stream(len(utts), 64)
    got, _, widths = streamed(enc, utts=utts, data=[[data[0][0]], [data[1][0]], [data[2][0]]], beam=bs)
    n = [g[0]["logits"].shape[0] for g in got]
    assert n == [6, 3, 1]
    logits = torch.zeros(len(utts), max(n), 16)
    for b, g in enumerate(got):
        logits[b, :n[b]] = g[0]["logits"]
    assert bs.finish() == dec.beam_search(logits.cuda(), torch.tensor(n).cuda())


def test_gpu_refusals_change_nothing():
    enc = gpu_enc("f32")
    ses = enc.stream(3, TV)
    v, w = 0.5 * torch.randn(3, ses.first_frames, HW, HW, device="cuda"), 0.1 * torch.randn(3, ses.first_samples, device="cuda")
    ses.push(v, w)
    before = (list(ses._rows_a), list(ses._rows_v), list(ses.video.front._n), list(ses.audio.front._n))
    with pytest.raises(ValueError, match="off the schedule"):
        ses.push(v, w, [4, 2, 4])
    with pytest.raises(ValueError, match="off the schedule"):
        ses.push(v, w, None, [2560, 100, 2560])
    with pytest.raises(TypeError, match="host lists"):
        ses.push(v, w, torch.tensor([4, 4, 4]))
    with pytest.raises(ValueError, match="slot 1 ends its utterance with 5 audio rows and 3 video rows"):
        ses.push(v, w, [4, 0, 4], None, [1], [1])
    with pytest.raises(RuntimeError, match="training mode"):
        enc.train()
        ses.push(v, w)
    enc.eval()
    assert before == (ses._rows_a, ses._rows_v, ses.video.front._n, ses.audio.front._n)
    out = ses.push(v, w, [4, 2, 4], [2560, 2360, 2560], [1], [1])         # slot 1: 8 frames with 640 * 8 - 160 samples
    assert out[1].tolist() == [2, 2, 2] and ses._end_a == ses._end_v == [False, True, False] and ses._rows_a[1] == ses._rows_v[1] == 4
    with pytest.raises(RuntimeError, match="slot 1 has ended"):
        ses.push(v, w, [4, 4, 4])
