"""Ring mode of the streaming CTC beam search, the parts that need no GPU: the three entry points are declared and exported, the state size, the argument checks of
avec_ctc_beam_stream_ring (reported before any HIP call: the pointers below are never dereferenced) and what the decoder refuses on the host."""
import re
import warnings

import pytest

from avec_amd.lib import HEADER, declared_functions, lib

P = 4096                                                    # a non-null, 16-byte aligned "pointer"
B, Tc, V, W, WIN, LOG = 3, 4, 32, 8, 16, 64
OUTPUTS = ("tokens", "frames", "out_len", "score", "ctc_logp", "stable_len", "info")


def _call(logits=P, chunk_len=P, reset=None, B=B, Tc=Tc, V=V, W=W, window=WIN, log_frames=LOG, state=P, state_bytes=None, backptr=P, backptr_bytes=None, log=P,
          log_bytes=None, emit=1, **outs):
    sb = lib.raw("avec_ctc_beam_ring_state_bytes")(B, min(W, 64)) if state_bytes is None else state_bytes
    bb = lib.raw("avec_ctc_beam_ring_workspace_bytes")(B, max(window, 0), W) if backptr_bytes is None else backptr_bytes
    lb = B * max(log_frames, 0) * 8 if log_bytes is None else log_bytes
    o = [outs.get(name, P) for name in OUTPUTS]
    lib.ctc_beam_stream_ring(logits, chunk_len, reset, B, Tc, V, W, window, log_frames, 1.0, None, 0.0, 0.0, 0.0, state, sb, backptr, bb, log, lb, *o, emit, None)


def test_header_declares_and_library_exports_the_entry_points():
    fns = declared_functions()
    assert len(fns["avec_ctc_beam_ring_state_bytes"][1]) == 2 and len(fns["avec_ctc_beam_ring_workspace_bytes"][1]) == 3
    assert len(fns["avec_ctc_beam_stream_ring"][1]) == 29
    for name in ("avec_ctc_beam_ring_state_bytes", "avec_ctc_beam_ring_workspace_bytes", "avec_ctc_beam_stream_ring"):
        assert callable(lib.raw(name))
    assert len(fns["avec_ctc_beam_search"][1]) == 18 and len(fns["avec_ctc_beam_stream"][1]) == 24          # what existed keeps its signature
    assert int(re.search(r"#define AVEC_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 4               # no struct changed
    assert lib.raw("avec_version")() == 4


def test_state_and_workspace_bytes():
    sb, wb = lib.raw("avec_ctc_beam_ring_state_bytes"), lib.raw("avec_ctc_beam_ring_workspace_bytes")
    for w in (1, 8, 16, 64):
        one = sb(1, w)
        assert one > 0 and one % 16 == 0
        assert one >= w * 68 + 32                           # the W slots of the beam buffer plus the two headers
        assert one > lib.raw("avec_ctc_beam_state_bytes")(1, w)      # {base, ccount, dropped, commits} on top of the bounded stream's state
        assert [sb(b, w) for b in (2, 5, 32)] == [2 * one, 5 * one, 32 * one]
    assert sb(1, 64) > sb(1, 8)
    assert wb(3, 16, 8) == 3 * 16 * 8 * 4 and wb(3, 16, 8) == lib.raw("avec_ctc_beam_workspace_bytes")(3, 16, 8)      # `window` rows, whatever the stream's length


def test_argument_errors_before_any_hip_call():
    with pytest.raises(RuntimeError, match="W=65"):
        _call(W=65)
    with pytest.raises(RuntimeError, match="V=1025"):
        _call(V=1025)
    with pytest.raises(RuntimeError, match="Tc=0"):
        _call(Tc=0)
    for bad in (1, 0, -4):
        with pytest.raises(RuntimeError, match=r"window=%d .*window >= 2" % bad):
            _call(window=bad, backptr_bytes=1 << 20)
    with pytest.raises(RuntimeError, match="log_frames=0"):
        _call(log_frames=0, log_bytes=1 << 20)
    need_s, need_b = lib.raw("avec_ctc_beam_ring_state_bytes")(B, W), lib.raw("avec_ctc_beam_ring_workspace_bytes")(B, WIN, W)
    with pytest.raises(RuntimeError, match="state of %d bytes, need %d" % (need_s - 1, need_s)):
        _call(state_bytes=need_s - 1)
    with pytest.raises(RuntimeError, match="state of %d bytes, need %d" % (lib.raw("avec_ctc_beam_state_bytes")(B, W), need_s)):
        _call(state_bytes=lib.raw("avec_ctc_beam_state_bytes")(B, W))              # a bounded stream's state is too small
    with pytest.raises(RuntimeError, match="backpointers of %d bytes, need %d" % (need_b - 1, need_b)):
        _call(backptr_bytes=need_b - 1)
    with pytest.raises(RuntimeError, match="commit log of %d bytes, need %d" % (B * LOG * 8 - 1, B * LOG * 8)):
        _call(log_bytes=B * LOG * 8 - 1)
    for out in OUTPUTS:
        with pytest.raises(RuntimeError, match="null output"):
            _call(**{out: None})
    for ptr in ("logits", "state", "backptr", "log"):
        with pytest.raises(RuntimeError, match="null pointer"):
            _call(**{ptr: None})
    with pytest.raises(RuntimeError, match="state must be 16-byte aligned"):
        _call(state=P + 4)
    with pytest.raises(RuntimeError, match="commit log must be 8-byte aligned"):
        _call(log=P + 4)


def test_decoder_refuses_on_the_host():
    """window together with max_frames, window < 2, a log no longer than the window, neither limit, and test_time_aug: all before anything touches the device"""
    import nnet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tta = nnet.CTCBeamSearchDecoder(beam_size=4, test_time_aug=True)
        dec = nnet.CTCBeamSearchDecoder(beam_size=4)
    with pytest.raises(NotImplementedError, match="test_time_aug"):
        tta.stream(2, window=16)
    with pytest.raises(ValueError, match="window=16 together with max_frames=100"):
        dec.stream(2, 100, window=16)
    with pytest.raises(ValueError, match="max_frames is needed"):
        dec.stream(2)
    with pytest.raises(ValueError, match="log_frames belongs to window"):
        dec.stream(2, 100, log_frames=64)
    for bad in (1, 0, -2):
        with pytest.raises(ValueError, match="window %d" % bad):
            dec.stream(2, window=bad)
    with pytest.raises(ValueError, match="log_frames 16 for window 16"):
        dec.stream(2, window=16, log_frames=16)
    s = dec.stream(2, window=16)
    assert type(s).__name__ == "CTCBeamRingStreamSession" and (s.window, s.log_frames) == (16, 256) and s.state is None
    assert dec.stream(2, window=100).log_frames == 400
    assert type(dec.stream(2, 10)).__name__ == "CTCBeamStreamSession" and type(dec.stream(2, max_frames=10)).__name__ == "CTCBeamStreamSession"
    with pytest.raises(RuntimeError, match="nothing was pushed"):
        s.finish()
