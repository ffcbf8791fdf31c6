"""GPU (-m gpu): the streamed audio front-end at the ops level (ops.mel_frames_stream -> mel_from_frames -> audio_stem_stream -> audio_stream_advance), push by push
against the chunked fp64 reference of tests/stream_front_ref.py.

B = 3 slots receive the 15 utterance lengths of stream_front_ref.LENGTHS one after the other (every slot restarts four times mid-run, and idles as an ended slot once it
has run out), at Tc = 4 (rows of 1320 samples, Tmax = 6), on the schedule and on an uneven plan of counts (161, 1320, 0, 40, 1000, ...); shapes (n_mels 80, C 180) and
(16, 4); 0.1 * randn input (no mel power near zero); both activation dtypes.  The state blob and every output buffer are pre-filled with NaN bytes, the wave columns at or
past n_samples[b] hold NaN: every valid output must be finite, rows past out_len zero, unproduced frame rows zero, out_len exact, an ended slot yields 0.

Bounds are measured, not assumed: in the same test the offline ops.mel_spectrogram and ops.AudioStemFn (eval mode) run on each whole utterance (B = 1) and are compared
per element with the same fp64 reference; the streamed result's worst element error over the run may be at most 2 x the offline one's (identical operands: the margin
is for another GEMM tile at another M).  The maximum is taken over the whole run, not per utterance: an utterance of 257 samples has one stem row, and the maximum of
so few elements is one draw, not a bound.  Figures per utterance are printed.  Measured on MI355X: DESIGN section 32.
"""
import pytest
import torch

from tests import stream_front_ref as FR

pytestmark = pytest.mark.gpu
TC, W, TMAX = 4, 1320, 6
FMAX = 2 * TMAX + 1
UTTS = [[2600, 257, 359, 360, 680], [2599, 319, 361, 679, 800], [960, 320, 640, 681, 799]]
assert sorted(sum(UTTS, [])) == sorted(FR.LENGTHS)
UNEVEN = [161, 1320, 0, 40, 1000, 1, 159, 160, 320, 360]


def _sizes(Ta, plan, k):
    if plan == "schedule":
        return FR.schedule_sizes(Ta, TC)
    sizes, i = [], k
    while sum(sizes) < Ta:
        sizes.append(min(UNEVEN[i % len(UNEVEN)], Ta - sum(sizes)))
        i += 1
    return sizes


def _pushes(plan):
    """-> list of pushes; a push = per slot (utterance index or None, first sample, count, restart, last)"""
    queue = [[(ui, at, c, at == 0, at + c == Ta) for ui, Ta in enumerate(ut) for at, c in _offsets(_sizes(Ta, plan, 3 * b + ui))] for b, ut in enumerate(UTTS)]
    n = max(len(q) for q in queue)
    return [[q[i] if i < len(q) else (None, 0, 0, False, False) for q in queue] for i in range(n)]


def _offsets(sizes):
    at = 0
    for c in sizes:
        yield at, c
        at += c


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("plan", ["schedule", "uneven"])
@pytest.mark.parametrize("n_mels,C", [(80, 180), (16, 4)])
def test_streamed_front_kernels_against_fp64(n_mels, C, plan, dtype):
    import avec_amd
    from avec_amd import ops
    from avec_amd.nnet.preprocessing import AudioPreprocessing
    avec_amd.set_compute_dtype(dtype)
    try:
        _run(ops, AudioPreprocessing, n_mels, C, plan, dtype)
    finally:
        avec_amd.set_compute_dtype("f32")


def _run(ops, AudioPreprocessing, n_mels, C, plan, dtype):
    dev, B, Fo = "cuda", len(UTTS), n_mels // 2
    sd = {k: (v.float().double() if v.is_floating_point() else v) for k, v in FR.params(n_mels, C, 6, 17).items()}         # fp32-representable parameters
    g = torch.Generator().manual_seed(23)
    data = [[(0.1 * torch.randn(Ta, generator=g)).double() for Ta in ut] for ut in UTTS]
    pre = AudioPreprocessing(16000, FR.N_FFT, 25, 10, n_mels).to(dev)
    window, dft, fb = pre.Spectrogram.window, pre._dft_matrix(torch.device(dev)), pre.MelScale.fb
    p = "m.subsampling_module.layers.0."
    conv, bn = torch.nn.Conv2d(1, C, 3, stride=2), torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        conv.weight.copy_(sd[p + "0.weight"]), conv.bias.copy_(sd[p + "0.bias"]), bn.weight.copy_(sd[p + "1.weight"]), bn.bias.copy_(sd[p + "1.bias"])
        bn.running_mean.copy_(sd[p + "1.running_mean"]), bn.running_var.copy_(sd[p + "1.running_var"])
    conv, bn = conv.to(dev), bn.to(dev).eval()
    bst = ops.BNState(C, window)
    ops.bn_finalize(bn, bst, 1, False)
    adt = torch.float32 if dtype == "f32" else torch.bfloat16

    # offline GPU error per utterance against the fp64 offline chain (B = 1: a padded batch would reflect at the batch's length)
    off_mel, off_stem, refs = 0.0, 0.0, {}
    for b, ut in enumerate(UTTS):
        for ui, Ta in enumerate(ut):
            mel_ref, rows_ref, _ = FR.offline(sd, data[b][ui], n_mels)
            with torch.no_grad():
                mel = ops.mel_spectrogram(data[b][ui].float()[None].to(dev), window, dft, fb, FR.N_FFT, FR.WIN, FR.HOP, n_mels)
                a = ops.AudioStemFn.apply(mel, conv.weight, conv, bn, False)
            em, es = float((mel[0].double().cpu() - mel_ref).abs().max()), float((a[0].double().cpu() - rows_ref).abs().max())
            refs[(b, ui)] = (em, es)
            off_mel, off_stem = max(off_mel, em), max(off_stem, es)

    state = ops.audio_stream_state(B, dev)
    assert state.numel() == B * (768 * 4 + 16)
    state.fill_(0xFF)                                                      # NaN tails, counters of -1: the first push restarts every slot
    fs = FR.FrontStream(B, sd, n_mels)
    got_mel, got_stem, worst = 0.0, 0.0, {}
    totals = [[0] * len(ut) for ut in UTTS]
    for pi, row in enumerate(_pushes(plan)):
        wave = torch.full((B, W), float("nan"))
        chunks = []
        for b, (ui, at, c, _, _) in enumerate(row):
            chunks.append(data[b][ui][at:at + c] if ui is not None else torch.zeros(0, dtype=FR.D64))
            wave[b, :c] = chunks[b].float()
        reset = {b for b, r in enumerate(row) if r[3]} | (set(range(B)) if pi == 0 else set())
        last = {b for b, r in enumerate(row) if r[4]}
        ref = fs.push(chunks, last, reset)
        wave_d = wave.to(dev)
        ns = torch.tensor([r[2] for r in row], dtype=torch.int64, device=dev)
        rs = torch.tensor([b in reset for b in range(B)], dtype=torch.uint8, device=dev)
        ls = torch.tensor([b in last for b in range(B)], dtype=torch.uint8, device=dev)
        out = (torch.full((B * FMAX, FR.WIN), float("nan"), device=dev), torch.full((B,), -7, dtype=torch.int64, device=dev), torch.full((B, 2), -7, dtype=torch.int64, device=dev))
        kw = dict(n_fft=FR.N_FFT, win=FR.WIN, hop=FR.HOP)
        frames, out_len, meta = ops.mel_frames_stream(wave_d, window, state, ns, rs, ls, Tmax=TMAX, out=out, **kw)
        mel = ops.mel_from_frames(frames, dft, fb, B, FMAX, n_mels)
        a = ops.audio_stem_stream(mel, conv.weight, conv.bias, bst.ss, out_len, meta, C, out=torch.full((B, TMAX, C * Fo), float("nan"), dtype=adt, device=dev))
        ops.audio_stream_advance(wave_d, state, ns, rs, ls, **kw)
        assert int(rs.sum()) == 0 and int(ls.sum()) == 0, "the advance consumes the flags"
        frames, mel, a, lens = frames.view(B, FMAX, FR.WIN).cpu(), mel.double().cpu(), a.double().cpu(), out_len.tolist()
        assert torch.isfinite(frames).all() and torch.isfinite(a).all(), (pi, "NaN reached an output")
        for b, (ui, at, c, _, _) in enumerate(row):
            mel_ref, valid, rows_ref, _ = ref[b]
            k = rows_ref.shape[0]
            assert lens[b] == k, (pi, b, lens, k)
            if ui is None:
                assert k == 0, "an ended slot yields 0 frames"
            assert float(a[b, k:].abs().max()) == 0.0 if k < TMAX else True, (pi, b, "rows past out_len")
            for j in range(FMAX):
                if j < len(valid) and valid[j]:
                    assert torch.isfinite(mel[b, :, j]).all()
                    e = float((mel[b, :, j] - mel_ref[:, j]).abs().max())
                    got_mel = max(got_mel, e)
                    worst[(b, ui)] = (max(worst.get((b, ui), (0, 0))[0], e), worst.get((b, ui), (0, 0))[1])
                else:
                    assert float(frames[b, j].abs().max()) == 0.0, (pi, b, j, "a frame row the push does not produce")
            if k:
                totals[b][ui] += k
                e = float((a[b, :k] - rows_ref).abs().max())
                got_stem = max(got_stem, e)
                worst[(b, ui)] = (worst.get((b, ui), (0, 0))[0], max(worst.get((b, ui), (0, 0))[1], e))
    for b, ut in enumerate(UTTS):
        for ui, Ta in enumerate(ut):
            assert totals[b][ui] == Ta // 320 + 1, (b, ui, Ta, totals[b][ui])
            print("%s %s n_mels=%d Ta=%d: streamed mel %.3g stem %.3g | offline mel %.3g stem %.3g" % ((dtype, plan, n_mels, Ta) + worst[(b, ui)] + refs[(b, ui)]))
    print("%s %s n_mels=%d worst: streamed mel %.3g stem %.3g | offline mel %.3g stem %.3g | ratios %.2f %.2f"
          % (dtype, plan, n_mels, got_mel, got_stem, off_mel, off_stem, got_mel / off_mel, got_stem / off_stem))
    assert got_mel <= 2 * off_mel and got_stem <= 2 * off_stem, (got_mel, off_mel, got_stem, off_stem)
