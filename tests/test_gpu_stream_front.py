"""GPU (-m gpu): AudioEfficientConformerEncoder.stream_front() and .stream() -- waveform chunks to features and to logits -- against the CPU oracle on each WHOLE utterance.

The model is AudioEfficientConformerEncoder(num_blocks=[1, 1, 1], interctc_blocks=[], att_type="regular") with its back_end replaced by the causal stack of
tests/test_gpu_stream_stack.py at the audio width (dims [180, 48], blocks [1, 1], InterCTC after block 1, conv stride 2, K = 15 causal, Mask(left_context=6,
right_context=0)) and head = Linear(48, 16); seeded weights, running statistics that are not the identity, eval mode.  B = 3 slots, chunks of Tc = 2, 4, 8 frames on the
session's schedule; slots 1 and 2 end their first utterance, are restarted and fed a second one.  The first utterance of slot 0 has 5160 = 40 + 320 * 16 samples, so for
every Tc its last push brings exactly 320 Tc samples and yields Tc + 1 frames: the combined session's second stack push (R = Tc / S + 1) is exercised on purpose.

f32: features, logits and InterCTC logits per utterance against oracle.mel_frontend + audio_stem + conformer_interctc(context=(6, 0, 0), causal_conv=True) + head:
rel_err < 1e-3 (the project's parity bound), lengths equal, Ta // 320 + 1 frames in all.
bf16: the offline GPU forward's error against the oracle is measured in the same test (B = 1 per utterance: a padded batch reflects at the batch's length) and the
streamed result may be at most 2 x that, as tests/test_gpu_stream_stack.py.  Measured on MI355X: DESIGN section 32.
"""
import functools

import pytest
import torch

from oracle import avec_oracle as O
from tests import stream_front_ref as FR
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
ATT = lambda cls, **kw: {"class": cls, "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=64, weight_init="default", bias_init="default", **kw)}
UTTS = [[5160], [3333, 2000], [1700, 4121]]
KEY, S = "c_ctc_0", 2


def make_enc():
    import nnet
    torch.manual_seed(1234)
    enc = nnet.AudioEfficientConformerEncoder(vocab_size=16, num_blocks=[1, 1, 1], interctc_blocks=[], att_type="regular")
    enc.back_end = nnet.ConformerInterCTC(dim_model=[180, 48], num_blocks=[1, 1], interctc_blocks=[1], vocab_size=16, loss_prefix="c_ctc",
                                          att_params=[ATT("RelPos1dMultiHeadAttention"), ATT("RelPos1dMultiHeadAttention", causal=True)],
                                          conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                          mask=nnet.Mask(left_context=6, right_context=0), conv_stride=2)
    enc.head = nnet.Linear(48, 16)
    g = torch.Generator().manual_seed(99)
    for m in enc.modules():
        if hasattr(m, "running_mean") and m.running_mean is not None:       # running statistics that are not the identity (the stem's BatchNorm2d and the stack's BatchNorm1d)
            m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape[0], generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape[0], generator=g))
    return enc.eval()


@functools.lru_cache(maxsize=1)
def fixture():
    """(waveforms data[b][utterance] [Ta], oracle results per (slot, utterance): (features, logits, InterCTC logits, frames at the stack's output)) -- computed once"""
    enc = make_enc()
    sd = {"m." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    data = [[0.1 * torch.randn(Ta, generator=g) for Ta in ut] for ut in UTTS]
    ref = []
    for ub in data:
        row = []
        for x in ub:
            with torch.no_grad():
                mel = O.mel_frontend(x[None])
                feat, flen = O.audio_stem(sd, "m", mel, torch.tensor([mel.shape[-1]]), False, {})
                y, ylen, inter = O.conformer_interctc(sd, "m.back_end", feat, flen, [1, 1], [1], "c_ctc", [1, 1], False, {}, context=(6, 0, 0), causal_conv=True)
                logits = O.linear(sd, "m.head", y)
            assert int(flen[0]) == feat.shape[1] == x.shape[0] // 320 + 1 and int(inter[KEY][1][0]) == int(ylen[0])
            row.append((feat[0], logits[0], inter[KEY][0][0], int(ylen[0])))
        ref.append(row)
    return data, ref


def gpu_enc(dtype):
    import avec_amd
    avec_amd.set_compute_dtype(dtype)
    return make_enc().to("cuda").eval()


def pushes(utts, Tc):
    """the schedule: per push and slot (utterance index or None, first sample, count, restart, last)"""
    queue = []
    for ut in utts:
        q = []
        for ui, Ta in enumerate(ut):
            at = 0
            for c in FR.schedule_sizes(Ta, Tc):
                q.append((ui, at, c, at == 0, at + c == Ta))
                at += c
        queue.append(q)
    n = max(len(q) for q in queue)
    return [[q[i] if i < len(q) else (None, 0, 0, False, False) for q in queue] for i in range(n)]


def wave_of(data, row, width):
    w = torch.full((len(row), width), float("nan"))                          # samples at or past n_samples are never read into a valid output
    for b, (ui, at, c, _, _) in enumerate(row):
        if ui is not None:
            w[b, :c] = data[b][ui][at:at + c]
    return w


def controls(row):
    return [r[2] for r in row], [b for b, r in enumerate(row) if r[4]], [b for b, r in enumerate(row) if r[3]]


def streamed_front(enc, Tc, counts="list", sync_free=False):
    """-> per (slot, utterance) the feature rows, and the per-push raw outputs"""
    data, _ = fixture()
    ses = enc.stream_front(len(UTTS), Tc)
    assert (ses.first_samples, ses.chunk_samples) == (320 * Tc + 40, 320 * Tc)
    got, raw = [[[] for _ in ut] for ut in UTTS], []
    for pi, row in enumerate(pushes(UTTS, Tc)):
        n, last, reset = controls(row)
        w = wave_of(data, row, ses.first_samples).cuda()
        ns = n if counts == "list" else torch.tensor(n, dtype=torch.int64, device="cuda")
        if sync_free and pi > 0:
            torch.cuda.set_sync_debug_mode("error")
        try:
            feat, flen = ses.push(w, ns, last or None, reset or None)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert tuple(feat.shape) == (len(UTTS), Tc + 2, 180) and feat.dtype == torch.float32
        raw.append((feat.clone(), flen.clone()))
        fl = flen.tolist()
        for b, (ui, at, c, _, fin) in enumerate(row):
            assert fl[b] == (0 if ui is None else (Tc if not fin else (at + c) // 320 + 1 - FR.ready(at))), (pi, b, fl)
            if ui is not None:
                got[b][ui].append(feat[b, :fl[b]].float().cpu())
    return [[torch.cat(g) for g in gb] for gb in got], raw


def streamed(enc, Tc, utts=UTTS, capture=False, sync_free=False, beam=None):
    """the combined session -> per (slot, utterance) (logits rows, InterCTC rows, frames), the per-push raw outputs, the R of every push"""
    data, _ = fixture()
    ses = enc.stream(len(utts), Tc)
    if capture:
        ses.capture()
    got, raw, Rs = [[[[], [], 0] for _ in ut] for ut in utts], [], []
    for pi, row in enumerate(pushes(utts, Tc)):
        n, last, reset = controls(row)
        w = wave_of(data, row, ses.first_samples).cuda()
        if sync_free and pi > 0:
            torch.cuda.set_sync_debug_mode("error")
        try:
            logits, olen, inter = ses.push(w, n, last or None, reset or None)
            if beam is not None:
                beam.push(logits.contiguous(), olen, reset or None, fetch=False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        lg, lglen = inter[KEY]
        raw.append((logits.clone(), olen.clone(), lg.clone(), lglen.clone()))
        Rs.append(logits.shape[1])
        assert logits.shape[1] == lg.shape[1] and logits.shape[1] in (Tc // S, Tc // S + 1)
        ol, ll = olen.tolist(), lglen.tolist()
        yielded = [0 if ui is None else (Tc if not fin else (at + c) // 320 + 1 - FR.ready(at)) for ui, at, c, _, fin in row]
        tail = max(0, max(yielded) - Tc)                                # (at most 1 frame behind the stack's chunk)
        assert tail <= 1 and logits.shape[1] == Tc // S + -(-tail // S), (pi, tail, logits.shape)
        for b, (ui, at, c, _, fin) in enumerate(row):
            frames = yielded[b]
            assert ol[b] == ll[b] == -(-frames // S), (pi, b, ol, ll, frames)
            if ui is not None:
                acc = got[b][ui]
                acc[0].append(logits[b, :ol[b]].float().cpu()), acc[1].append(lg[b, :ll[b]].float().cpu())
                acc[2] += ol[b]
    return [[(torch.cat(a[0]), torch.cat(a[1]), a[2]) for a in gb] for gb in got], raw, Rs


def offline(enc):
    """the offline GPU forward, one utterance at a time -> per (slot, utterance) (features, logits, InterCTC logits)"""
    from avec_amd import ops
    data, ref = fixture()
    out = []
    for b, ub in enumerate(data):
        row = []
        for ui, x in enumerate(ub):
            with torch.no_grad():
                xs, ln = x[None].cuda(), torch.tensor([x.shape[0]]).cuda()
                y, ylen, inter = enc(xs, ln)
                mel, _ = enc.audio_preprocessing(xs, ln)
                stem = enc.subsampling_module.layers[0]
                feat = ops.linear(ops.AudioStemFn.apply(mel, stem[0].weight, stem[0], stem[1], False), enc.linear.weight, enc.linear.bias)
            assert int(ylen[0]) == ref[b][ui][3]
            row.append((feat[0].float().cpu(), y[0].float().cpu(), inter[KEY][0][0].float().cpu()))
        out.append(row)
    return out


@pytest.mark.parametrize("Tc", [2, 4, 8])
def test_front_f32_matches_oracle(Tc):
    _, ref = fixture()
    got, _ = streamed_front(gpu_enc("f32"), Tc)
    for b, ub in enumerate(ref):
        for ui, (feat, _, _, _) in enumerate(ub):
            e = rel_err(got[b][ui], feat) if got[b][ui].shape == feat.shape else float("inf")
            print("front Tc=%d slot %d utterance %d: %d frames, features %.3g" % (Tc, b, ui, feat.shape[0], e))
            assert got[b][ui].shape == feat.shape and feat.shape[0] == UTTS[b][ui] // 320 + 1 and e < 1e-3, (Tc, b, ui, got[b][ui].shape, feat.shape, e)


@pytest.mark.parametrize("Tc", [2, 4, 8])
def test_stream_f32_matches_oracle(Tc):
    _, ref = fixture()
    got, _, Rs = streamed(gpu_enc("f32"), Tc)
    assert Tc // S + 1 in Rs and Tc // S in Rs, "the tail case (a last push of 320 Tc samples -> Tc + 1 frames) is part of this run"
    for b, ub in enumerate(ref):
        for ui, (_, logits, lg, n) in enumerate(ub):
            gl, gi, gn = got[b][ui]
            assert gn == n and gl.shape == logits.shape and gi.shape == lg.shape, (Tc, b, ui, gn, n, gl.shape, logits.shape)
            el, ei = rel_err(gl, logits), rel_err(gi, lg)
            print("stream Tc=%d slot %d utterance %d: %d rows, logits %.3g InterCTC %.3g" % (Tc, b, ui, n, el, ei))
            assert el < 1e-3 and ei < 1e-3, (Tc, b, ui, el, ei)


@pytest.mark.parametrize("Tc", [2, 4, 8])
def test_stream_bf16_within_twice_the_offline_error(Tc):
    """measured on MI355X (max over slots and utterances): see DESIGN section 32"""
    _, ref = fixture()
    enc = gpu_enc("bf16")
    try:
        off = offline(enc)
        front, _ = streamed_front(enc, Tc)
        got, _, _ = streamed(enc, Tc)
    finally:
        import avec_amd
        avec_amd.set_compute_dtype("f32")
    bad = []
    for b, ub in enumerate(ref):
        for ui, (feat, logits, lg, n) in enumerate(ub):
            gl, gi, gn = got[b][ui]
            assert gn == n and front[b][ui].shape == feat.shape
            ef, el, ei = rel_err(front[b][ui], feat), rel_err(gl, logits), rel_err(gi, lg)
            of, ol, oi = rel_err(off[b][ui][0], feat), rel_err(off[b][ui][1], logits), rel_err(off[b][ui][2], lg)
            print("bf16 Tc=%d slot %d utterance %d: streamed features %.3g logits %.3g InterCTC %.3g | offline GPU %.3g %.3g %.3g" % (Tc, b, ui, ef, el, ei, of, ol, oi))
            if not (ef <= 2 * of and el <= 2 * ol and ei <= 2 * oi):
                bad.append((b, ui, ef, of, el, ol, ei, oi))
    assert not bad, bad


def test_splits_agree_and_device_counts_equal_host_counts():
    enc = gpu_enc("f32")
    a, _, _ = streamed(enc, 2)
    b, _, _ = streamed(enc, 8)
    for ga, gb in zip(a, b):
        for (la, ia, na), (lb, ib, nb) in zip(ga, gb):
            assert na == nb and rel_err(la, lb) < 1e-3 and rel_err(ia, ib) < 1e-3
    fa, _ = streamed_front(enc, 2)
    fb, _ = streamed_front(enc, 8)
    for ga, gb in zip(fa, fb):
        for xa, xb in zip(ga, gb):
            assert rel_err(xa, xb) < 1e-3
    _, host = streamed_front(enc, 4)
    _, dev = streamed_front(enc, 4, counts="tensor")
    for (fh, lh), (fd, ld) in zip(host, dev):
        assert torch.equal(lh, ld) and torch.equal(fh, fd)


def test_captured_pushes_equal_eager_pushes():
    enc = gpu_enc("f32")
    _, eager, Re = streamed(enc, 4)
    _, graph, Rg = streamed(enc, 4, capture=True)
    assert Re == Rg and len(eager) == len(graph) >= 3 and 3 in Re
    for pi, (e, g) in enumerate(zip(eager, graph)):
        for te, tg in zip(e, g):
            assert torch.equal(te, tg), pi


def test_pushes_do_not_synchronise_or_grow():
    enc = gpu_enc("f32")
    streamed_front(enc, 4, sync_free=True)
    streamed(enc, 4, sync_free=True)                                   # host-list counts, restarts, ends and the second stack push under torch's sync debug mode
    for make in (enc.stream_front, enc.stream):
        ses = make(3, 4)
        w = 0.1 * torch.randn(3, ses.first_samples, device="cuda")
        for kw in (dict(), dict(last=[1]), dict(reset=[1])):            # (the first tail push allocates the second push's input once)
            out = ses.push(w, **kw)
        del out
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for i in range(50):
                out = ses.push(w, None, [1] if i % 10 == 4 else None, [1] if i % 10 == 5 else ([i % 3] if i % 7 == 0 else None))
                del out
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m0, make.__name__


def test_streamed_logits_feed_the_streaming_beam_search():
    """waveform chunk -> features -> causal stack -> logits -> beam, one chain of sessions: finish() gives what beam_search gives on the concatenated streamed logits"""
    import nnet
    utts = [[5160], [3333], [1700]]
    enc = gpu_enc("f32")
    dec = nnet.CTCBeamSearchDecoder(beam_size=4, ngram_tmp=1.0)
    bs = dec.stream(len(utts), 64)
    got, _, Rs = streamed(enc, 4, utts=utts, beam=bs)
    assert 3 in Rs
    T = max(g[0][2] for g in got)
    logits = torch.zeros(len(utts), T, 16)
    for b, g in enumerate(got):
        logits[b, :g[0][2]] = g[0][0]
    assert bs.finish() == dec.beam_search(logits.cuda(), torch.tensor([g[0][2] for g in got]).cuda())


def test_gpu_refusals_and_contract():
    enc = gpu_enc("f32")
    ses = enc.stream(3, 4)
    w = 0.1 * torch.randn(3, ses.first_samples, device="cuda")
    ses.push(w)
    with pytest.raises(ValueError, match="off the schedule"):
        ses.push(w, [1280, 640, 1280])
    with pytest.raises(TypeError, match="host lists"):
        ses.push(w, torch.tensor([1280, 1280, 1280]))
    ses.push(w, [1280, 640, 1280], last=[1])
    with pytest.raises(RuntimeError, match="slot 1 has ended"):
        ses.push(w, [1280, 1280, 1280])
    ses.push(w, [1280, 1320, 1280], reset=[1])
    with pytest.raises(ValueError, match="wave"):
        ses.push(w[:, :100])
    with pytest.raises(RuntimeError, match="training mode"):
        enc.train().stream_front(3, 4)
