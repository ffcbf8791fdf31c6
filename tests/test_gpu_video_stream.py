"""GPU (-m gpu): VisualEfficientConformerEncoder.stream_front() and .stream() -- video chunks to per-frame features and to logits -- against the CPU oracle on each WHOLE
utterance.

The model is VisualEfficientConformerEncoder(num_blocks=[1, 1], interctc_blocks=[]) with its back_end replaced by the causal stack of tests/test_gpu_stream_front.py at
the visual width (dims [256, 48], blocks [1, 1], InterCTC after block 1, conv stride 2, K = 15 causal, Mask(left_context=6, right_context=0)) and head = Linear(48, 16);
seeded weights, running statistics that are not the identity, eval mode.  88x88 frames, B = 3 slots, Tc = 4 on the session's schedule; utterances of 1 to 11 frames;
slots 1 and 2 end their first utterance, are restarted and fed a second one (slot 2 a third).  Utterances of 6, 5 and 10 frames end with a push that yields Tc + 2,
Tc + 1 and Tc + 2 frames: the combined session's second stack push (R = Tc / S + 1) is exercised on purpose; the run's last push has no such slot (R = Tc / S).

f32 and bf16: features per utterance against oracle.visual_frontend(train=False), logits and InterCTC logits against oracle.conformer_interctc(context=(6, 0, 0),
causal_conv=True) + head.  The bound is measured in the test: the offline GPU forward of the same module on the whole utterance (B = 1) is compared with the same
oracle, and the streamed result may be at most 2 x that.  Lengths are exact.  Measured on MI355X: DESIGN section 33.
"""
import functools

import pytest
import torch

from oracle import avec_oracle as O
from tests import video_stream_ref as VR
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
ATT = lambda cls, **kw: {"class": cls, "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=64, weight_init="default", bias_init="default", **kw)}
UTTS = [[11], [6, 5], [1, 10, 3]]
KEY, S, TC, HW = "c_ctc_0", 2, 4, 88


def make_enc():
    import nnet
    torch.manual_seed(1234)
    enc = nnet.VisualEfficientConformerEncoder(vocab_size=16, num_blocks=[1, 1], interctc_blocks=[])
    enc.back_end = nnet.ConformerInterCTC(dim_model=[256, 48], num_blocks=[1, 1], interctc_blocks=[1], vocab_size=16, loss_prefix="c_ctc",
                                          att_params=[ATT("RelPos1dMultiHeadAttention"), ATT("RelPos1dMultiHeadAttention", causal=True)],
                                          conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                          mask=nnet.Mask(left_context=6, right_context=0), conv_stride=2)
    enc.head = nnet.Linear(48, 16)
    g = torch.Generator().manual_seed(99)
    for m in enc.modules():
        if hasattr(m, "running_mean") and m.running_mean is not None:       # running statistics that are not the identity (the stem's BatchNorm3d, the ResNet's, the stack's)
            m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape[0], generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape[0], generator=g))
    return enc.eval()


@functools.lru_cache(maxsize=1)
def fixture():
    """(videos data[b][utterance] [T][H][W], oracle results per (slot, utterance): (features, logits, InterCTC logits, rows at the stack's output)) -- computed once"""
    enc = make_enc()
    sd = {"m." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    data = [[0.5 * torch.randn(T, HW, HW, generator=g) for T in ut] for ut in UTTS]
    ref = []
    for ub in data:
        row = []
        for x in ub:
            with torch.no_grad():
                feat = O.visual_frontend(sd, "m.front_end", x[None, None], False, {})
                flen = torch.tensor([x.shape[0]])
                y, ylen, inter = O.conformer_interctc(sd, "m.back_end", feat, flen, [1, 1], [1], "c_ctc", [1, 1], False, {}, context=(6, 0, 0), causal_conv=True)
                logits = O.linear(sd, "m.head", y)
            assert feat.shape[1] == x.shape[0] and int(inter[KEY][1][0]) == int(ylen[0]) == -(-x.shape[0] // S)
            row.append((feat[0], logits[0], inter[KEY][0][0], int(ylen[0])))
        ref.append(row)
    return data, ref


def gpu_enc(dtype):
    import avec_amd
    avec_amd.set_compute_dtype(dtype)
    return make_enc().to("cuda").eval()


def pushes(utts, Tc):
    """the schedule: per push and slot (utterance index or None, first frame, count, restart, last)"""
    queue = []
    for ut in utts:
        q = []
        for ui, T in enumerate(ut):
            at = 0
            for c in VR.schedule_sizes(T, Tc):
                q.append((ui, at, c, at == 0, at + c == T))
                at += c
        queue.append(q)
    n = max(len(q) for q in queue)
    return [[q[i] if i < len(q) else (None, 0, 0, False, False) for q in queue] for i in range(n)]


def video_of(data, row, frames):
    v = torch.full((len(row), frames, HW, HW), float("nan"))                 # frames at or past n_frames are never read into a valid output
    for b, (ui, at, c, _, _) in enumerate(row):
        if ui is not None:
            v[b, :c] = data[b][ui][at:at + c]
    return v


def controls(row):
    return [r[2] for r in row], [b for b, r in enumerate(row) if r[4]], [b for b, r in enumerate(row) if r[3]]


def yielded(r):
    ui, at, c, _, fin = r
    return 0 if ui is None else (at + c if fin else VR.ready(at + c)) - VR.ready(at)


def streamed_front(enc, Tc, utts=UTTS, data=None, counts="list", sync_free=False, capture=False):
    """-> per (slot, utterance) (feature rows, stem frames), the per-push raw outputs"""
    data = fixture()[0] if data is None else data
    ses = enc.stream_front(len(utts), Tc)
    if capture:
        ses.capture(frame=(HW, HW))
    assert (ses.first_frames, ses.chunk_frames) == (Tc + 2, Tc)
    got, raw = [[([], []) for _ in ut] for ut in utts], []
    for pi, row in enumerate(pushes(utts, Tc)):
        n, last, reset = controls(row)
        v = video_of(data, row, ses.first_frames).cuda()
        nf = n if counts == "list" else torch.tensor(n, dtype=torch.int64, device="cuda")
        if sync_free and pi > 0:
            torch.cuda.set_sync_debug_mode("error")
        try:
            feat, flen = ses.push(v[:, None] if pi % 2 else v, nf, last or None, reset or None)      # [B, 1, Tc + 2, H, W] is accepted as well
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert tuple(feat.shape) == (len(utts), Tc + 2, 256) and feat.dtype == torch.float32
        want = [yielded(r) for r in row]
        if counts == "list":          # a push with no slot beyond Tc frames runs the ResNet and the Linear on B * Tc frames, the others on B * (Tc + 2)
            assert ses.resnet_frames == len(utts) * (Tc + 2 if max(want) > Tc else Tc), (pi, ses.resnet_frames, want)
        raw.append((feat.clone(), flen.clone()))
        fl = flen.tolist()
        assert fl == want, (pi, fl, want)
        for b, (ui, _, _, _, _) in enumerate(row):
            if ui is not None:
                got[b][ui][0].append(feat[b, :fl[b]].float().cpu()), got[b][ui][1].append(ses._frames[:fl[b], b].float().cpu())
    return [[(torch.cat(g[0]), torch.cat(g[1])) for g in gb] for gb in got], raw


def streamed(enc, Tc, utts=UTTS, capture=False, sync_free=False, beam=None):
    """the combined session -> per (slot, utterance) (logits rows, InterCTC rows, rows), the per-push raw outputs, the R of every push"""
    data, _ = fixture()
    ses = enc.stream(len(utts), Tc)
    if capture:
        ses.capture(frame=(HW, HW))
    got, raw, Rs = [[[[], [], 0] for _ in ut] for ut in utts], [], []
    for pi, row in enumerate(pushes(utts, Tc)):
        n, last, reset = controls(row)
        v = video_of(data, row, ses.first_frames).cuda()
        if sync_free and pi > 0:
            torch.cuda.set_sync_debug_mode("error")
        try:
            logits, olen, inter = ses.push(v, n, last or None, reset or None)
            if beam is not None:
                beam.push(logits.contiguous(), olen, reset or None, fetch=False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        lg, lglen = inter[KEY]
        raw.append((logits.clone(), olen.clone(), lg.clone(), lglen.clone()))
        Rs.append(logits.shape[1])
        assert logits.shape[1] == lg.shape[1] and logits.shape[1] in (Tc // S, Tc // S + 1)
        tail = max(0, max(yielded(r) for r in row) - Tc)                # (at most 2 frames behind the stack's chunk)
        assert tail <= 2 and logits.shape[1] == Tc // S + -(-tail // S), (pi, tail, logits.shape)
        ol, ll = olen.tolist(), lglen.tolist()
        for b, r in enumerate(row):
            assert ol[b] == ll[b] == -(-yielded(r) // S), (pi, b, ol, ll, yielded(r))
            if r[0] is not None:
                acc = got[b][r[0]]
                acc[0].append(logits[b, :ol[b]].float().cpu()), acc[1].append(lg[b, :ll[b]].float().cpu())
                acc[2] += ol[b]
    return [[(torch.cat(a[0]), torch.cat(a[1]), a[2]) for a in gb] for gb in got], raw, Rs


def offline(enc):
    """the offline GPU forward, one utterance at a time -> per (slot, utterance) (features, logits, InterCTC logits)"""
    data, ref = fixture()
    out = []
    for b, ub in enumerate(data):
        row = []
        for ui, x in enumerate(ub):
            with torch.no_grad():
                xs, ln = x[None, None].cuda(), torch.tensor([x.shape[0]]).cuda()
                y, ylen, inter = enc(xs, ln)
                feat = enc.forward_front(xs)
            assert int(ylen[0]) == ref[b][ui][3]
            row.append((feat[0].float().cpu(), y[0].float().cpu(), inter[KEY][0][0].float().cpu()))
        out.append(row)
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stream_within_twice_the_offline_error(dtype):
    """measured on MI355X (max over slots and utterances): see DESIGN section 33"""
    _, ref = fixture()
    enc = gpu_enc(dtype)
    try:
        off = offline(enc)
        front, _ = streamed_front(enc, TC)
        got, _, Rs = streamed(enc, TC)
    finally:
        import avec_amd
        avec_amd.set_compute_dtype("f32")
    assert TC // S + 1 in Rs and TC // S in Rs, "the tail case (a last push that yields more than Tc frames) is part of this run"
    bad = []
    for b, ub in enumerate(ref):
        for ui, (feat, logits, lg, n) in enumerate(ub):
            gl, gi, gn = got[b][ui]
            assert gn == n and gl.shape == logits.shape and gi.shape == lg.shape and front[b][ui][0].shape == feat.shape, (b, ui, gn, n, gl.shape, front[b][ui][0].shape)
            ef, el, ei = rel_err(front[b][ui][0], feat), rel_err(gl, logits), rel_err(gi, lg)
            of, ol, oi = rel_err(off[b][ui][0], feat), rel_err(off[b][ui][1], logits), rel_err(off[b][ui][2], lg)
            print("%s slot %d utterance %d (%d frames): streamed features %.3g logits %.3g InterCTC %.3g | offline GPU %.3g %.3g %.3g"
                  % (dtype, b, ui, feat.shape[0], ef, el, ei, of, ol, oi))
            if not (ef <= 2 * of and el <= 2 * ol and ei <= 2 * oi):
                bad.append((b, ui, ef, of, el, ol, ei, oi))
    assert not bad, bad


def test_device_counts_equal_host_counts_and_restarts_reproduce_fresh_sessions():
    enc = gpu_enc("f32")
    data, _ = fixture()
    run, host = streamed_front(enc, TC)
    _, dev = streamed_front(enc, TC, counts="tensor")
    for (fh, lh), (fd, ld) in zip(host, dev):
        assert torch.equal(lh, ld)
        for b, n in enumerate(lh.tolist()):
            assert torch.equal(fh[b, :n], fd[b, :n])
    # a slot reset mid-run reproduces the fresh-session result for its new utterance, at the stem output bit for bit; slot 0 goes on undisturbed
    fresh, _ = streamed_front(enc, TC, utts=[[11], [5], [10]], data=[[data[0][0]], [data[1][1]], [data[2][1]]])
    for (b, ui) in ((0, 0), (1, 1), (2, 1)):
        assert torch.equal(run[b][ui][1], fresh[b][0][1]) and torch.equal(run[b][ui][0], fresh[b][0][0]), (b, ui)


def test_captured_pushes_equal_eager_pushes():
    enc = gpu_enc("f32")
    _, eager, Re = streamed(enc, TC)
    _, graph, Rg = streamed(enc, TC, capture=True)
    assert Re == Rg and len(eager) == len(graph) >= 3 and 3 in Re
    for pi, (e, g) in enumerate(zip(eager, graph)):
        for te, tg in zip(e, g):
            assert torch.equal(te, tg), pi
    _, fe = streamed_front(enc, TC)
    _, fg = streamed_front(enc, TC, capture=True)
    for pi, (e, g) in enumerate(zip(fe, fg)):
        assert torch.equal(e[0], g[0]) and torch.equal(e[1], g[1]), pi


def test_pushes_do_not_synchronise_or_grow():
    enc = gpu_enc("f32")
    streamed_front(enc, TC, sync_free=True)
    streamed(enc, TC, sync_free=True)                                  # host-list counts, restarts, ends and the second stack push under torch's sync debug mode
    for make in (enc.stream_front, enc.stream):
        ses = make(3, TC)
        v = 0.5 * torch.randn(3, ses.first_frames, HW, HW, device="cuda")
        for kw in (dict(), dict(last=[1]), dict(reset=[1])):            # (the first tail push allocates the second push's input once)
            out = ses.push(v, **kw)
        del out
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for i in range(20):
                out = ses.push(v, None, [1] if i % 10 == 4 else None, [1] if i % 10 == 5 else ([i % 3] if i % 7 == 0 else None))
                del out
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == m0, make.__name__


def test_streamed_logits_feed_the_streaming_beam_search():
    """video chunk -> per-frame features -> causal stack -> logits -> beam, one chain of sessions: finish() gives what beam_search gives on the concatenated logits"""
    import nnet
    utts = [[11], [6], [1]]
    enc = gpu_enc("f32")
    dec = nnet.CTCBeamSearchDecoder(beam_size=4, ngram_tmp=1.0)
    bs = dec.stream(len(utts), 64)
    got, _, Rs = streamed(enc, TC, utts=utts, beam=bs)
    assert 3 in Rs
    T = max(g[0][2] for g in got)
    logits = torch.zeros(len(utts), T, 16)
    for b, g in enumerate(got):
        logits[b, :g[0][2]] = g[0][0]
    assert bs.finish() == dec.beam_search(logits.cuda(), torch.tensor([g[0][2] for g in got]).cuda())


def test_gpu_refusals_and_contract():
    enc = gpu_enc("f32")
    ses = enc.stream(3, TC)
    v = 0.5 * torch.randn(3, ses.first_frames, HW, HW, device="cuda")
    ses.push(v)
    with pytest.raises(ValueError, match="off the schedule"):
        ses.push(v, [4, 2, 4])
    with pytest.raises(TypeError, match="host lists"):
        ses.push(v, torch.tensor([4, 4, 4]))
    ses.push(v, [4, 2, 4], last=[1])
    with pytest.raises(RuntimeError, match="slot 1 has ended"):
        ses.push(v, [4, 4, 4])
    ses.push(v, [4, 6, 4], reset=[1])
    with pytest.raises(ValueError, match="video"):
        ses.push(v[:, :3])
    front = enc.stream_front(3, TC).capture(frame=(HW, HW))
    with pytest.raises(ValueError, match="captured at 88x88"):
        front.push(torch.zeros(3, 6, 96, 96, device="cuda"))
    with pytest.raises(RuntimeError, match="training mode"):
        enc.train().stream_front(3, TC)
