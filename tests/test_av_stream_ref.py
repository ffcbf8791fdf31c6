"""CPU: the FIFO reference of the audio-visual row pairing (tests/av_stream_ref.py), the joint schedule's identities, the two entry points of csrc/av_stream.hip
(declared, exported, argument errors before any launch) and AudioVisualStreamSession's refusals and host-side contract.  No GPU."""
import functools

import pytest
import torch

from tests import av_stream_ref as AR
from tests import stream_front_ref as SF
from tests import video_stream_ref as VR

TVS = range(2, 17, 2)
OFFSETS = (-480, -320, -161, -159, -1, 0, 159, 160, 319, 480)        # run 2: ten other sample counts per T, as offsets from 640 T - 160


def test_fifo_reference():
    g = torch.Generator().manual_seed(0)
    a, v = torch.randn(2, 3, 8, generator=g), torch.randn(2, 3, 4, generator=g)
    f = AR.FuseRef(2, 3, torch.bfloat16)
    xc, n = f.push(a, [2, 0], v, [1, 3], max_emit=1)
    assert n == [1, 0] and torch.equal(xc[0, 0], torch.cat([a[0, 0], v[0, 0]]).bfloat16()) and not xc[1].any()
    xc, n = f.push(a, [0, 0], v, [0, 0], max_emit=1)                   # nothing new: slot 0 waits for a video row, slot 1 for an audio row
    assert n == [0, 0] and not xc.any()
    xc, n = f.push(a[:, 1:], [0, 2], v[:, 2:], [1, 0], reset=(1,), max_emit=1)      # slot 1 restarts: its three pending video rows vanish
    assert n == [1, 0] and torch.equal(xc[0, 0], torch.cat([a[0, 1], v[0, 2]]).bfloat16())
    assert [len(q) for q in f.fa + f.fv] == [0, 2, 0, 0]
    with pytest.raises(AssertionError, match="overflow"):
        f.push(a, [0, 2], v, [0, 0], max_emit=1)


def test_joint_schedule_run_1():
    """Tv = 2 .. 16, T = 1 .. 400, 640 T - 160 samples: both branches total ceil(T / 2) rows, the rings drain, no branch holds more than R + 1 unpaired rows (cap =
    R + 2), the fusion stack never gets a short chunk followed by more rows, and a third of the cases end in different pushes"""
    n = differ = 0
    for Tv in TVS:
        for T in range(1, 401):
            s = AR.simulate(T, 640 * T - 160, Tv)
            assert s["total_a"] == s["total_v"] == s["pairs"] == -(-T // 2), (Tv, T, s)
            assert s["left"] == (0, 0) and s["peak"] <= s["R"] + 1 and not s["short_then_more"], (Tv, T, s)
            assert abs(s["pushes"][0] - s["pushes"][1]) <= 1
            n, differ = n + 1, differ + (s["pushes"][0] != s["pushes"][1])
            assert (s["pushes"][0] == s["pushes"][1] + 1) == (T > Tv and T % Tv in (1, 2)) or Tv == 2, (Tv, T, s)
    assert (n, differ) == (3200, 1074)


@functools.lru_cache(maxsize=None)
def _session(Tv, B=1):
    return _enc().stream(B, Tv)


@functools.lru_cache(maxsize=1)
def _enc():
    return AR.make_av_enc()


def _fresh(Tv, B=1):
    ses = _session(Tv, B)
    ses._forget()
    ses._first = ses.video.front._first = ses.audio.front._first = True
    for front in (ses.video.front, ses.audio.front):
        front._forget()
    return ses


def test_joint_schedule_run_2_and_the_session_refuses_the_rest():
    """other sample counts: where the branches' row totals agree the same properties hold and the session's host mirrors end at zero; where they differ the session
    refuses, before any launch, at the latest in the push where the second branch ends"""
    agree = differ = 0
    for T in range(1, 201):
        for d in OFFSETS:
            Ta = 640 * T - 160 + d
            if Ta <= 256:                                               # (refused by the audio front-end, offline as well: no reflection padding)
                continue
            for Tv in TVS:
                s = AR.simulate(T, Ta, Tv)
                ok = s["total_a"] == s["total_v"]
                if ok:
                    assert s["left"] == (0, 0) and s["peak"] <= s["R"] + 1 and not s["short_then_more"], (Tv, T, Ta, s)
                agree, differ = agree + ok, differ + (not ok)
                if T > 40 and T % 7:                                    # the session's host side on a sixth of the cases (all lengths up to 40)
                    continue
                ses = _fresh(Tv)
                rows = ses.schedule(T, Ta)
                if ok:
                    for row in rows:
                        AR.host_push(ses, [row])
                    assert ses._pend_a == ses._pend_v == [0] and ses._rows_a == ses._rows_v == [s["total_a"]] and ses._end_a == ses._end_v == [True]
                else:
                    with pytest.raises((ValueError, RuntimeError), match="slot 0 (ends its utterance with|would hold)"):
                        for row in rows:
                            AR.host_push(ses, [row])
    assert agree > 10000 and differ > 2000, (agree, differ)


def test_schedule_is_both_branch_schedules():
    for Tv in (2, 4, 6):
        ses = _fresh(Tv)
        assert (ses.first_frames, ses.chunk_frames, ses.first_samples, ses.chunk_samples, ses.R, ses.cap) == (Tv + 2, Tv, 640 * Tv + 40, 640 * Tv, Tv // 2, Tv // 2 + 2)
        for T in list(range(1, 40)) + [97, 400]:
            for Ta in (640 * T - 160, 640 * T, 640 * T + 333):
                rows = ses.schedule(T, Ta)
                assert rows == AR.joint_schedule(T, Ta, Tv)
                v, a = VR.schedule_sizes(T, Tv), SF.schedule_sizes(Ta, 2 * Tv)
                assert [r[0] for r in rows][:len(v)] == v and [r[1] for r in rows][:len(a)] == a
                assert [r[2] for r in rows].index(True) == len(v) - 1 and [r[3] for r in rows].index(True) == len(a) - 1
                assert sum(r[2] for r in rows) == sum(r[3] for r in rows) == 1
    with pytest.raises(ValueError, match="schedule"):
        _fresh(4).schedule(0, 100)


def test_entry_points_declared_exported_and_version():
    import subprocess
    from avec_amd.lib import LIB_PATH, declared_functions, lib
    fns = declared_functions()
    names = ["avec_av_fuse_stream_state_bytes", "avec_av_fuse_stream"]
    assert [len(fns[n][1]) for n in names] == [5, 18]
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    assert lib.raw("avec_version")() == 4
    sb = lib.raw("avec_av_fuse_stream_state_bytes")
    r16 = lambda n: (n + 15) // 16 * 16
    for dtype, esz in ((1, 2), (0, 4)):
        for B, Da, Dv, cap in ((3, 360, 360, 4), (3, 8, 4, 3), (1, 4, 4, 3), (32, 360, 360, 4), (5, 48, 48, 3)):
            assert sb(dtype, B, Da, Dv, cap) == r16(B * (cap * (Da + Dv) * esz + 24)) and sb(dtype, B, Da, Dv, cap) % 16 == 0
    assert sb(1, 0, 8, 4, 3) == 0 and sb(1, 3, 6, 4, 3) == 0 and sb(1, 3, 8, 2, 3) == 0 and sb(1, 3, 8, 4, 0) == 0 and sb(2, 3, 8, 4, 3) == 0


def test_entry_point_validates_arguments_without_gpu():
    """each argument error is reported before any HIP call (no GPU needed): the addresses are fake, nothing is dereferenced before the checks pass, and they do not pass"""
    from avec_amd.lib import lib
    P = 4096
    sb = lib.raw("avec_av_fuse_stream_state_bytes")

    def fuse(dtype=1, a=P, a_len=P, v=P, v_len=P, state=P, nbytes=None, reset=None, xc=P, pair_len=P, B=3, Ra=2, Rv=3, Da=8, Dv=4, cap=4, max_emit=2):
        lib.av_fuse_stream(dtype, a, a_len, v, v_len, state, sb(dtype, B, Da, Dv, cap) if nbytes is None else nbytes, reset, xc, pair_len, B, Ra, Rv, Da, Dv, cap, max_emit, None)
    for kw, msg in [(dict(a=None), "null pointer"), (dict(a_len=None), "null pointer"), (dict(v=None), "null pointer"), (dict(v_len=None), "null pointer"),
                    (dict(state=None), "null pointer"), (dict(xc=None), "null pointer"), (dict(pair_len=None), "null pointer"), (dict(dtype=2, nbytes=64), "dtype 2"),
                    (dict(B=0, nbytes=64), "bad dims"), (dict(Ra=0), "bad dims"), (dict(Rv=0), "bad dims"), (dict(Da=0, nbytes=64), "bad dims"),
                    (dict(Da=6, nbytes=64), "multiples of 4"), (dict(Dv=2, nbytes=64), "multiples of 4"), (dict(max_emit=0), "bad max_emit"),
                    (dict(max_emit=3), "at least max_emit \\+ 2"), (dict(cap=3), "at least max_emit \\+ 2"), (dict(Ra=5), "does not fit a ring"), (dict(Rv=5), "does not fit a ring"),
                    (dict(nbytes=sb(1, 3, 8, 4, 4) - 16), "state of"), (dict(nbytes=sb(1, 3, 8, 4, 4) + 16), "state of"), (dict(dtype=0, nbytes=sb(1, 3, 8, 4, 4)), "state of"),
                    (dict(cap=5, nbytes=sb(1, 3, 8, 4, 4)), "state of"), (dict(a=P + 8), "16-byte aligned"), (dict(v=P + 4), "16-byte aligned"),
                    (dict(state=P + 8), "16-byte aligned"), (dict(xc=P + 8), "16-byte aligned"), (dict(a_len=P + 4), "8-byte aligned"), (dict(v_len=P + 4), "8-byte aligned"),
                    (dict(pair_len=P + 4), "8-byte aligned")]:
        with pytest.raises(RuntimeError, match="av_fuse_stream.*" + msg):
            fuse(**kw)


def test_session_refusals_and_host_contract():
    """every refusal names its cause and comes before any launch (no GPU here)"""
    import nnet
    shipped = AR.make_av_enc(causal=False)
    with pytest.raises(NotImplementedError, match="left_context=None"):         # the shipped config (patch attention, Mask(), "same" padding): the stack's own refusal
        shipped.stream(3, 4)
    with pytest.raises(RuntimeError, match="training mode"):
        shipped.train().stream(3, 4)
    enc = _enc()
    assert not hasattr(nnet.AudioVisualEfficientConformerEncoder, "stream_front") and "AudioVisualStreamSession" in nnet.streaming.__all__
    with pytest.raises(RuntimeError, match="training mode"):
        enc.train().stream(3, 4)
    enc.eval()
    enc.audio_visual_encoder.train()
    with pytest.raises(RuntimeError, match="training mode"):
        enc.stream(3, 4)
    enc.eval()
    with pytest.raises(ValueError, match="chunk_frames = 3 must be a positive multiple"):      # odd chunk_frames: the video stack's own refusal
        enc.stream(3, 3)
    with pytest.raises(ValueError, match="batch_size 0"):
        enc.stream(0, 4)
    blk = enc.audio_encoder.back_end.conformer_blocks[1]
    stride, blk.stride = blk.stride, 1                                           # audio stride 2: 2 Tv / 2 rows against Tv / 2
    try:
        with pytest.raises(ValueError, match=r"video stack \(stride 2\).*audio stack \(stride 2, 8 stem frames\)"):
            enc.stream(3, 4)
    finally:
        blk.stride = stride
    ses = enc.stream(3, 4)
    assert isinstance(ses, nnet.AudioVisualStreamSession) and (ses.R, ses.cap, ses.video.S, ses.audio.S, ses.back.S, ses.back.Tc) == (2, 4, 2, 4, 1, 2)
    assert not any("stream" in k or "ring" in k for k in enc.state_dict())
    V, W = torch.zeros(3, 6, 88, 88), torch.zeros(3, ses.first_samples)
    with pytest.raises(ValueError, match="video"):
        ses.push(V[:, :5], W)
    with pytest.raises(ValueError, match="wave"):
        ses.push(V, W[:, :100])
    with pytest.raises(RuntimeError):                                            # CPU tensors: a missing GPU is an error, not a fall-back
        ses.push(V, W)
    # tensor counts and counts of the wrong number, checked before anything is launched; _plan changes nothing
    with pytest.raises(TypeError, match="host lists for n_frames"):
        ses._plan(torch.tensor([6, 6, 6]), None, None, None, None)
    with pytest.raises(TypeError, match="host lists for n_samples"):
        ses._plan(None, torch.tensor([2600, 2600, 2600]), None, None, None)
    with pytest.raises(ValueError, match="for 3 slots"):
        ses._plan([6, 6], None, None, None, None)
    with pytest.raises(ValueError, match="for 3 slots"):
        ses._plan(None, [2600], None, None, None)
    with pytest.raises(ValueError, match="off the schedule"):
        ses._plan([6, 5, 6], None, None, None, None)
    with pytest.raises(ValueError, match="off the schedule"):
        ses._plan(None, [2600, 2600, 2000], None, None, None)
    rmask, vplan, aplan, launches, mirrors = ses._plan(None, None, None, None, None)          # the first push restarts every slot, on the schedule's counts
    assert rmask == [True] * 3 and vplan[2] == [6] * 3 and aplan[2] == [2600] * 3 and launches == [[2, 2, 2]] and mirrors[0] == mirrors[1] == [0] * 3
    assert ses._first and ses._pend_a == [0] * 3 and ses.video.front._n == [0] * 3
    # utterances of 6, 5 and 11 frames side by side: 6 and 5 end in different pushes (video first), with a second fuse launch for the row behind the first R
    rows = [ses.schedule(T, 640 * T - 160) for T in (6, 5, 11)]
    idle = (0, 0, False, False)
    got = [AR.host_push(ses, [r[i] if i < len(r) else idle for r in rows]) for i in range(3)]
    assert got == [[[2, 2, 2]], [[1, 1, 2]], [[0, 0, 2]]] and ses._pend_a == ses._pend_v == [0] * 3 and ses._rows_a == ses._rows_v == [3, 3, 6]
    assert [len(r) for r in rows] == [2, 2, 3] and rows[0][0][2] and not rows[0][0][3] and rows[0][1][3]
    # the row-total mismatch at `last`: 6 frames (3 rows) with the samples of 4 frames (2 rows); refused in the push where the second branch ends, nothing changed
    ses = _fresh(4, 3)
    with pytest.raises(ValueError, match="slot 0 ends its utterance with 2 audio rows and 3 video rows"):
        AR.host_push(ses, [(6, 2400, True, True), (6, 2600, False, False), (6, 2600, False, False)])
    assert ses._first and ses._rows_a == [0] * 3
    # ring overflow: one branch goes on alone
    ses = _fresh(4, 3)
    AR.host_push(ses, [(6, 0, False, False)] * 3)
    AR.host_push(ses, [(4, 0, False, False)] * 3)
    with pytest.raises(RuntimeError, match="slot 0 would hold 0 audio and 6 video rows that are not paired yet: the rings keep 4"):
        AR.host_push(ses, [(4, 0, False, False)] * 3)
    AR.host_push(ses, [(6, 2600, False, False)] * 3, reset=[0, 1, 2])            # a restart empties the rings
    assert ses._pend_a == ses._pend_v == [0] * 3 and ses._rows_a == ses._rows_v == [2] * 3
