"""CPU: the chunked reference of the streamed visual stem (tests/video_stream_ref.py) equals the offline stem exactly, the schedule's identities, the three entry points
of csrc/video_stream.hip (declared, exported, argument errors before any launch) and the sessions' refusals and host-side contract.  No GPU."""
import random

import pytest
import torch

from tests import stem_exact_ref as SR
from tests import video_stream_ref as VR

F64 = torch.float64


def _k():
    k = SR.channel_constants()
    return SR.stem_weights(), k["bias"], k["scale"], k["shift"]


def _video(T, seed, H=16, W=16):
    return SR.ints(torch.Generator().manual_seed(seed), (T, H, W), 2)


@pytest.mark.parametrize("T", VR.LENGTHS)
def test_chunked_equals_offline(T):
    """float64 integer-valued operands: no rounding enters, torch.equal"""
    k = _k()
    v = _video(T, 100 + T)
    ref = VR.offline_stem(v, *k)
    assert ref.shape == (T, 4, 4, 64) and float((ref != 0).double().mean()) > 0.3
    plans = [VR.schedule_sizes(T, 2), VR.schedule_sizes(T, 4), VR.uneven_sizes(T), VR.uneven_sizes(T, 1)]
    for sizes in plans:
        for late in (False, True):
            got = VR.run_plan(v, sizes, k, late_last=late)
            assert got.shape == ref.shape and torch.equal(got, ref), (T, sizes, late)


def test_uneven_plan_wraps_the_ring_partially():
    assert {0, 1, 2, 3} <= set(VR.UNEVEN) and max(VR.UNEVEN) <= 4
    assert set(VR.uneven_sizes(23)) >= {0, 1, 2, 3}


def test_random_plans_equal_offline():
    k = _k()
    rnd = random.Random(5)
    for i in range(300):
        T = rnd.randint(1, 14)
        Tc = rnd.randint(1, 6)
        sizes, at = [], 0
        while at < T:
            c = min(T - at, rnd.randint(0, Tc + 2 if at == 0 else Tc))
            sizes.append(c)
            at += c
        v = _video(T, 1000 + i, 8, 16)
        assert torch.equal(VR.run_plan(v, sizes, k, late_last=rnd.random() < 0.3), VR.offline_stem(v, *k)), (T, sizes)


def test_restarted_and_idle_slots():
    """two slots: slot 1 ends, idles, is restarted mid-run; slot 0 goes on undisturbed"""
    k = _k()
    a, b1, b2 = _video(11, 1), _video(3, 2), _video(6, 3)
    s = VR.VideoFrontStream(2, 16, 16, *k)
    o = [s.push([a[0:6], b1[0:3]], last=(1,)), s.push([a[6:10], b2[0:0]]), s.push([a[10:11], b2[0:6]], last=(0, 1), reset=(1,)), s.push([a[0:0], b2[0:0]])]
    assert [x[1].shape[0] for x in o] == [3, 0, 6, 0] and [x[0].shape[0] for x in o] == [4, 4, 3, 0]
    assert torch.equal(torch.cat([x[0] for x in o]), VR.offline_stem(a, *k))
    assert torch.equal(o[0][1], VR.offline_stem(b1, *k)) and torch.equal(o[2][1], VR.offline_stem(b2, *k))


def test_schedule_identities():
    rnd = random.Random(11)
    for _ in range(20000):
        Tc, T = rnd.randint(1, 32), rnd.randint(1, 400)
        sizes = VR.schedule_sizes(T, Tc)
        y = VR.yields(sizes)
        assert sum(sizes) == T and sum(y) == T
        assert all(v == Tc for v in y[:-1]) and 0 < y[-1] <= Tc + 2, (Tc, T, sizes, y)
        assert sizes[0] == min(T, Tc + 2) and all(c == Tc for c in sizes[1:-1])
    for n in range(0, 50):
        assert VR.ready(n) == max(0, n - 2)
    # arbitrary legal counts: a push never yields more than Tc + 2 frames (the session's buffers)
    for _ in range(20000):
        Tc, n = rnd.randint(1, 16), rnd.randint(0, 500)
        c = rnd.randint(0, Tc + 2 if n == 0 else Tc)
        assert max(n + c, VR.ready(n + c)) - VR.ready(n) <= Tc + 2


def test_entry_points_declared_exported_and_version():
    import subprocess
    from avec_amd.lib import LIB_PATH, declared_functions, lib
    fns = declared_functions()
    names = ["avec_video_stream_state_bytes", "avec_video_stem_stream", "avec_video_stream_advance"]
    assert [len(fns[n][1]) for n in names] == [4, 19, 13]
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    assert lib.raw("avec_version")() == 4
    sb = lib.raw("avec_video_stream_state_bytes")
    assert sb(1, 3, 88, 88) == 3 * (4 * 88 * 88 * 2 + 16) and sb(0, 3, 88, 88) == 3 * (4 * 88 * 88 * 4 + 16)
    assert sb(1, 0, 88, 88) == 0 and sb(1, 3, 88, 84) == 0 and sb(2, 3, 88, 88) == 0
    assert sb(1, 3, 88, 88) % 16 == 0 and sb(0, 5, 9, 40) % 16 == 0


def test_entry_points_validate_arguments_without_gpu():
    """each argument error is reported before any HIP call (no GPU needed): the addresses are fake, nothing is dereferenced before the checks pass, and they do not pass"""
    from avec_amd.lib import lib
    P = 4096

    def SB(dtype, B=3, H=88, W=88):
        return B * (4 * H * W * (2 if dtype else 4) + 16)

    def stem(dtype=1, chunk=P, ldc=6 * 88 * 88, state=P, sb=None, nf=P, w8=P, ss=P, out=P, out_len=P, B=3, Tin=6, Tmax=6, H=88, W=88):
        lib.video_stem_stream(dtype, chunk, ldc, state, SB(dtype) if sb is None else sb, nf, None, None, w8, None, ss, out, out_len, B, Tin, Tmax, H, W, None)
    for kw, msg in [(dict(chunk=None), "null pointer"), (dict(state=None), "null pointer"), (dict(w8=None), "null pointer"), (dict(ss=None), "null pointer"),
                    (dict(out=None), "null pointer"), (dict(out_len=None), "null pointer"), (dict(dtype=2), "dtype 2"), (dict(B=0), "bad dims"), (dict(Tin=0), "bad dims"),
                    (dict(W=84), "frame 88x84 not supported"), (dict(W=24), "frame 88x24 not supported"), (dict(H=7), "frame 7x88 not supported"),
                    (dict(Tmax=0), "bad Tmax"), (dict(Tmax=-3), "bad Tmax"), (dict(ldc=6 * 88 * 88 - 4), "slot stride"), (dict(ldc=6 * 88 * 88 + 2), "slot stride"),
                    (dict(sb=SB(1) - 1), "state of"), (dict(dtype=0, sb=SB(1)), "state of"), (dict(state=P + 8), "16-byte aligned"), (dict(chunk=P + 4), "16-byte aligned"),
                    (dict(nf=P + 4), "8-byte aligned"), (dict(out=P + 8), "16-byte aligned"), (dict(out_len=P + 4), "8-byte aligned")]:
        with pytest.raises(RuntimeError, match="video_stem_stream.*" + msg):
            stem(**kw)

    def advance(dtype=1, chunk=P, ldc=6 * 88 * 88, state=P, sb=None, nf=P, B=3, Tin=6, H=88, W=88):
        lib.video_stream_advance(dtype, chunk, ldc, state, SB(dtype) if sb is None else sb, nf, None, None, B, Tin, H, W, None)
    for kw, msg in [(dict(chunk=None), "null pointer"), (dict(state=None), "null pointer"), (dict(sb=100), "state of"), (dict(W=90), "not supported"), (dict(B=0), "bad dims"),
                    (dict(nf=P + 4), "8-byte aligned")]:
        with pytest.raises(RuntimeError, match="video_stream_advance.*" + msg):
            advance(**kw)


ATT = lambda cls, **kw: {"class": cls, "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=64, weight_init="default", bias_init="default", **kw)}


def _enc(causal=False):
    import nnet
    torch.manual_seed(3)
    enc = nnet.VisualEfficientConformerEncoder(vocab_size=16, interctc_blocks=[], num_blocks=[1, 1])
    if causal:
        enc.back_end = nnet.ConformerInterCTC(dim_model=[256, 48], num_blocks=[1, 1], interctc_blocks=[1], vocab_size=16, loss_prefix="c_ctc",
                                              att_params=[ATT("RelPos1dMultiHeadAttention"), ATT("RelPos1dMultiHeadAttention", causal=True)],
                                              conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                              mask=nnet.Mask(left_context=6, right_context=0), conv_stride=2)
        enc.head = nnet.Linear(48, 16)
    return enc


def test_session_refusals_and_host_contract():
    """every refusal names its cause and comes before any launch (no GPU here)"""
    import nnet
    enc = _enc()
    with pytest.raises(RuntimeError, match="training mode"):
        enc.train().stream_front(3, 4)
    with pytest.raises(RuntimeError, match="training mode"):
        enc.train().stream(3, 4)
    enc.eval()
    with pytest.raises(ValueError, match="chunk_frames = 0"):
        enc.stream_front(3, 0)
    with pytest.raises(ValueError, match="batch_size 0"):
        enc.stream_front(0, 4)
    stem = enc.front_end[0].layers[0]
    stem[1].track_running_stats = False
    with pytest.raises(NotImplementedError, match="running statistics"):
        enc.stream_front(3, 4)
    stem[1].track_running_stats = True
    stride = stem[0].stride
    stem[0].stride = (1, 1, 1)
    with pytest.raises(NotImplementedError, match=r"not the \(5, 7, 7\)"):
        enc.stream_front(3, 4)
    stem[0].stride = stride
    with pytest.raises(NotImplementedError, match="left_context=None"):       # the shipped back-end (Mask(), "same" padding): the stack's own refusal, unchanged
        enc.stream(3, 4)
    causal = _enc(causal=True).eval()
    with pytest.raises(ValueError, match="chunk_frames = 3 must be a positive multiple"):
        causal.stream(3, 3)
    both = causal.stream(3, 4)
    assert isinstance(both, nnet.VisualStreamSession) and (both.first_frames, both.chunk_frames, both.S) == (6, 4, 2)
    with pytest.raises(TypeError, match="host lists"):
        both.push(torch.zeros(3, 6, 88, 88), torch.tensor([6, 6, 6]))
    with pytest.raises(ValueError, match="off the schedule"):
        both.push(torch.zeros(3, 6, 88, 88), [6, 5, 6])
    ses = enc.stream_front(3, 4)
    assert isinstance(ses, nnet.VisualFrontStreamSession) and (ses.first_frames, ses.chunk_frames, ses.Tmax) == (6, 4, 6)
    assert not any("stream" in k or "ring" in k for k in enc.state_dict())
    with pytest.raises(ValueError, match="video"):
        ses.push(torch.zeros(3, 5, 88, 88))
    # the host contract of list counts, checked before anything is launched; _controls changes nothing
    assert ses._controls(None, None, None) == ([True] * 3, [False] * 3, [6] * 3, [4] * 3)                 # the first push restarts every slot
    ses._first, ses._n, ses._ended = False, [6, 10, 0], [False, True, False]
    assert ses._controls(None, None, None) == ([False] * 3, [False] * 3, [4, 0, 6], [4, 0, 4])            # defaults: the schedule's counts; an ended slot idles
    assert ses._controls([3, 0, 2], [0], [2]) == ([False, False, True], [True, False, False], [3, 0, 2], [5, 0, 0])
    assert ses._controls([0, 0, 1], [0, 2], None)[3] == [2, 0, 1]                                         # the end announced late: the two look-ahead frames; a 1-frame utterance
    with pytest.raises(ValueError, match=r"n_frames\[0\] = 5 outside 0 .. 4"):
        ses._controls([5, 0, 0], None, None)
    with pytest.raises(ValueError, match=r"n_frames\[2\] = 7 outside 0 .. 6"):
        ses._controls([0, 0, 7], None, None)
    with pytest.raises(ValueError, match="for 3 slots"):
        ses._controls([1, 2], None, None)
    with pytest.raises(RuntimeError, match="slot 1 has ended"):
        ses._controls([0, 2, 0], None, None)
    assert ses._controls([0, 5, 0], None, [1])[3] == [0, 3, 0]                                            # restarted: legal again, at its start up to first_frames
    assert (ses._n, ses._ended) == ([6, 10, 0], [False, True, False])
    ses._n = [None, None, None]
    with pytest.raises(RuntimeError, match="device-tensor counts"):
        ses._controls([0, 0, 0], None, None)
