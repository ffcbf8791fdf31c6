"""The streamed audio front-end without a GPU: the chunked fp64 reference of tests/stream_front_ref.py (a sample carry, a counter and an `ended` flag per slot) equals
the offline chain (oracle.mel_frontend + stem + Linear) on each whole utterance to 1e-12 for every utterance length and split tried; the schedule's identities; the
four entry points are declared and exported and the ABI version stays 4; their argument errors; the sessions' refusals and host-side contract checks."""
import random

import pytest
import torch

from tests import stream_front_ref as FR

TOL = 1e-12
N_MELS, C, D = 16, 4, 6


def _utt(Ta, seed):
    return 0.1 * torch.randn(Ta, generator=torch.Generator().manual_seed(seed), dtype=FR.D64)


@pytest.mark.parametrize("Ta", FR.LENGTHS)
def test_chunked_equals_offline(Ta):
    sd = FR.params(N_MELS, C, D, 5)
    x = _utt(Ta, 100 + Ta)
    _, rows, feat = FR.offline(sd, x, N_MELS)
    assert rows.shape[0] == Ta // 320 + 1
    plans = [("split %d" % s, FR.split_sizes(Ta, s)) for s in FR.SPLITS] + [("schedule Tc=%d" % Tc, FR.schedule_sizes(Ta, Tc)) for Tc in (2, 4, 8)] + [("whole", [Ta])]
    for name, sizes in plans:
        fs = FR.FrontStream(1, sd, N_MELS)
        got_rows, got_feat, per_push = FR.run_utterance(fs, 0, x, sizes)
        assert got_rows.shape == rows.shape and sum(per_push) == Ta // 320 + 1, (Ta, name, got_rows.shape, rows.shape)
        assert float((got_rows - rows).abs().max()) < TOL and float((got_feat - feat).abs().max()) < TOL, (Ta, name)


def test_restarted_slot_and_80_mel_shape():
    """a second utterance in a restarted slot sees nothing of the first (the carry is hidden by the counter, not cleared); the shipped 80-mel / 180-channel shape"""
    sd = FR.params(80, 180, 12, 6)
    fs = FR.FrontStream(2, sd, 80)
    for slot, Ta, Tc in [(1, 960, 2), (1, 681, 2), (0, 800, 4), (1, 257, 2)]:
        x = _utt(Ta, 7 * Ta + slot)
        got_rows, got_feat, _ = FR.run_utterance(fs, slot, x, FR.schedule_sizes(Ta, Tc))
        _, rows, feat = FR.offline(sd, x, 80)
        assert float((got_rows - rows).abs().max()) < TOL and float((got_feat - feat).abs().max()) < TOL, (slot, Ta)


def test_schedule_identities():
    """every push but the last yields exactly Tc frames; the last at most Tc + 1, and Tc + 1 exactly when it brings >= 320 Tc - 40 samples (>= 320 Tc as the only push);
    the total is Ta // 320 + 1; the carry is 400 samples under the schedule and fewer than 720 for any counts"""
    rnd = random.Random(11)
    for _ in range(20000):
        Tc, Ta = rnd.randint(2, 16), rnd.randint(257, 40000)
        sizes, n, total = FR.schedule_sizes(Ta, Tc), 0, 0
        for i, c in enumerate(sizes):
            fin = i == len(sizes) - 1
            k = ((n + c) // 320 + 1 if fin else FR.ready(n + c)) - FR.ready(n)
            if fin:
                assert k <= Tc + 1 and (k == Tc + 1) == (c >= (320 * Tc - 40 if i else 320 * Tc)), (Tc, Ta, i, c, k)
            else:
                assert k == Tc and (n + c) - FR.first_kept(FR.ready(n + c)) == 400, (Tc, Ta, i, c, k)
            n, total = n + c, total + k
        assert total == Ta // 320 + 1
    for n in range(0, 5000):
        assert n - FR.first_kept(FR.ready(n)) < 720
    # arbitrary counts up to first_samples: a push never yields more than Tc + 2 frames (the session's buffers)
    for _ in range(20000):
        Tc, n = rnd.randint(2, 16), rnd.randint(0, 20000)
        c = rnd.randint(0, 320 * Tc + 40)
        assert max((n + c) // 320 + 1, FR.ready(n + c)) - FR.ready(n) <= Tc + 2


def test_entry_points_declared_exported_and_version():
    import subprocess
    from avec_amd.lib import LIB_PATH, declared_functions, lib
    fns = declared_functions()
    names = ["avec_audio_stream_state_bytes", "avec_mel_frames_stream", "avec_audio_stem_stream", "avec_audio_stream_advance"]
    assert [len(fns[n][1]) for n in names] == [1, 18, 13, 13]
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    assert lib.raw("avec_version")() == 4
    sb = lib.raw("avec_audio_stream_state_bytes")
    assert sb(3) == 3 * (768 * 4 + 16) and sb(0) == 0 and sb(3) >= 3 * 720 * 4


def test_entry_points_validate_arguments_without_gpu():
    """each argument error is reported before any launch (no GPU needed): the addresses are fake, nothing is dereferenced before the checks pass, and they do not pass"""
    from avec_amd.lib import lib
    P, SB = 4096, 3 * (768 * 4 + 16)

    def frames(wave=P, ldw=1320, window=P, out=P, state=P, sb=SB, ns=P, out_len=P, meta=P, B=3, W=1320, Tmax=6, n_fft=512, win=400, hop=160):
        lib.mel_frames_stream(wave, ldw, window, out, state, sb, ns, None, None, out_len, meta, B, W, Tmax, n_fft, win, hop, None)
    for kw, msg in [(dict(wave=None), "null pointer"), (dict(state=None), "null pointer"), (dict(window=None), "null pointer"), (dict(meta=None), "null pointer"),
                    (dict(ldw=1000), "bad dims"), (dict(B=0), "bad dims"), (dict(win=401), "bad framing"), (dict(win=600), "bad framing"), (dict(hop=0), "bad framing"),
                    (dict(hop=200), "tail of 800 samples"), (dict(sb=SB - 1), "state of"), (dict(state=P + 8), "16-byte aligned"), (dict(ns=P + 4), "8-byte aligned"),
                    (dict(Tmax=0), "bad Tmax"), (dict(out_len=P + 4), "8-byte aligned")]:
        with pytest.raises(RuntimeError, match=msg):
            frames(**kw)

    def advance(wave=P, ldw=1320, state=P, sb=SB, ns=P, B=3, W=1320, win=400, hop=160):
        lib.audio_stream_advance(wave, ldw, state, sb, ns, None, None, B, W, 512, win, hop, None)
    for kw, msg in [(dict(wave=None), "null pointer"), (dict(sb=100), "state of"), (dict(W=0), "bad dims"), (dict(hop=300), "tail of")]:
        with pytest.raises(RuntimeError, match="audio_stream_advance.*" + msg):
            advance(**kw)

    def stem(mel=P, w=P, ss=P, out=P, out_len=P, meta=P, B=3, n_mels=80, Tmax=6, C=180, dtype=0):
        lib.audio_stem_stream(dtype, mel, w, None, ss, out, out_len, meta, B, n_mels, Tmax, C, None)
    for kw, msg in [(dict(mel=None), "null pointer"), (dict(ss=None), "null pointer"), (dict(out_len=None), "null pointer"), (dict(C=0), "bad dims"),
                    (dict(n_mels=81), "must be even"), (dict(n_mels=40), "multiple of 8"), (dict(out=P + 8, dtype=1), "16-byte aligned"), (dict(meta=P + 4), "8-byte aligned")]:
        with pytest.raises(RuntimeError, match=msg):
            stem(**kw)


def _enc(**kw):
    import nnet
    torch.manual_seed(3)
    return nnet.AudioEfficientConformerEncoder(vocab_size=16, num_blocks=[1, 1, 1], interctc_blocks=[], att_type="regular", **kw)


def test_session_refusals_and_host_contract():
    """every refusal names its cause and comes before any launch (no GPU here)"""
    enc = _enc()
    with pytest.raises(RuntimeError, match="training mode"):
        enc.train().stream_front(3, 4)
    with pytest.raises(RuntimeError, match="training mode"):
        enc.train().stream(3, 4)
    enc.eval()
    with pytest.raises(ValueError, match="chunk_frames = 1"):
        enc.stream_front(3, 1)
    enc.audio_preprocessing.normalize = True
    with pytest.raises(NotImplementedError, match="normalize=True"):
        enc.stream_front(3, 4)
    enc.audio_preprocessing.normalize = False
    bn = enc.subsampling_module.layers[0][1]
    bn.track_running_stats = False
    with pytest.raises(NotImplementedError, match="running statistics"):
        enc.stream_front(3, 4)
    bn.track_running_stats = True
    with pytest.raises(NotImplementedError, match="left_context=None"):       # the shipped back-end (Mask(), "same" padding): the stack's own refusal, unchanged
        enc.stream(3, 4)
    ses = enc.stream_front(3, 4)
    assert (ses.first_samples, ses.chunk_samples, ses.Tmax) == (1320, 1280, 6)
    assert enc.stream_front(2, 16).first_samples == 5160
    assert not any("stream" in k or "carry" in k for k in enc.state_dict())
    # the host contract of list counts, checked before anything is launched; _controls changes nothing
    assert ses._controls(None, None, None) == ([True] * 3, [False] * 3, [1320] * 3, [4] * 3)              # the first push restarts every slot
    ses._first, ses._n, ses._ended = False, [1320, 2600, 0], [False, True, False]
    assert ses._controls(None, None, None) == ([False] * 3, [False] * 3, [1280, 0, 1320], [4, 0, 4])      # defaults: the schedule's counts; an ended slot idles
    assert ses._controls([1280, 0, 300], [0], [2]) == ([False, False, True], [True, False, False], [1280, 0, 300], [5, 0, 0])
    with pytest.raises(ValueError, match=r"n_samples\[0\] = 1321 outside 0 .. 1320"):
        ses._controls([1321, 0, 0], None, None)
    with pytest.raises(ValueError, match="for 3 slots"):
        ses._controls([1, 2], None, None)
    with pytest.raises(RuntimeError, match="slot 1 has ended"):
        ses._controls([0, 5, 0], None, None)
    assert ses._controls([0, 5, 0], None, [1])[3] == [0, 0, 0]                                            # restarted: legal again
    with pytest.raises(ValueError, match="slot 2 ends after 256 samples"):
        ses._controls([0, 0, 256], [2], None)
    assert ses._controls([0, 0, 257], [2], None)[3] == [0, 0, 1]
    ses._n = [None, None, None]
    with pytest.raises(RuntimeError, match="device-tensor counts"):
        ses._controls([0, 0, 0], None, None)
