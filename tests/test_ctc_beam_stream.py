"""Streaming CTC beam search, the parts that need no GPU: the two entry points are declared and exported, the state size, and the argument checks of
avec_ctc_beam_stream (reported before any HIP call: the pointers below are never dereferenced)."""
import re

import pytest

from avec_amd.lib import HEADER, declared_functions, lib

P = 4096                                                    # a non-null, 16-byte aligned "pointer"
B, Tc, V, W, Tcap = 3, 4, 32, 8, 20


def _call(logits=P, chunk_len=P, reset=None, B=B, Tc=Tc, V=V, W=W, Tcap=Tcap, state=P, state_bytes=None, backptr=P, backptr_bytes=None, tokens=P, out_len=P,
          score=P, ctc_logp=P, stable_len=P, emit=1):
    sb = lib.raw("avec_ctc_beam_state_bytes")(B, min(W, 64)) if state_bytes is None else state_bytes
    bb = lib.raw("avec_ctc_beam_workspace_bytes")(B, Tcap, W) if backptr_bytes is None else backptr_bytes
    lib.ctc_beam_stream(logits, chunk_len, reset, B, Tc, V, W, Tcap, 1.0, None, 0.0, 0.0, 0.0, state, sb, backptr, bb, tokens, out_len, score, ctc_logp,
                        stable_len, emit, None)


def test_header_declares_and_library_exports_the_entry_points():
    fns = declared_functions()
    assert len(fns["avec_ctc_beam_state_bytes"][1]) == 2 and len(fns["avec_ctc_beam_stream"][1]) == 24
    for name in ("avec_ctc_beam_state_bytes", "avec_ctc_beam_stream"):
        assert callable(lib.raw(name))
    assert int(re.search(r"#define AVEC_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 4        # no struct changed


def test_state_bytes_positive_and_linear_in_batch():
    sb = lib.raw("avec_ctc_beam_state_bytes")
    for w in (1, 8, 16, 64):
        one = sb(1, w)
        assert one > 0 and one % 16 == 0
        assert one >= w * 68 + 8                            # the W slots of the beam buffer plus {live beams, frames consumed}
        assert [sb(b, w) for b in (2, 5, 32)] == [2 * one, 5 * one, 32 * one]
    assert sb(1, 64) > sb(1, 8)


def test_argument_errors_before_any_hip_call():
    with pytest.raises(RuntimeError, match="W=65"):
        _call(W=65)
    with pytest.raises(RuntimeError, match="V=1025"):
        _call(V=1025)
    with pytest.raises(RuntimeError, match="Tc=0"):
        _call(Tc=0)
    with pytest.raises(RuntimeError, match="Tcap=0"):
        _call(Tcap=0, backptr_bytes=1 << 20)
    need_s, need_b = lib.raw("avec_ctc_beam_state_bytes")(B, W), lib.raw("avec_ctc_beam_workspace_bytes")(B, Tcap, W)
    with pytest.raises(RuntimeError, match="state of %d bytes, need %d" % (need_s - 1, need_s)):
        _call(state_bytes=need_s - 1)
    with pytest.raises(RuntimeError, match="backpointers of %d bytes, need %d" % (need_b - 1, need_b)):
        _call(backptr_bytes=need_b - 1)
    for out in ("tokens", "out_len", "score", "ctc_logp", "stable_len"):
        with pytest.raises(RuntimeError, match="null output"):
            _call(**{out: None})
    for ptr in ("logits", "state", "backptr"):
        with pytest.raises(RuntimeError, match="null pointer"):
            _call(**{ptr: None})
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _call(state=P + 4)


def test_decoder_stream_needs_no_gpu_to_refuse():
    """test_time_aug and a push past max_frames are refused on the host, before anything touches the device"""
    import warnings

    import torch

    import nnet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tta = nnet.CTCBeamSearchDecoder(beam_size=4, test_time_aug=True)
        dec = nnet.CTCBeamSearchDecoder(beam_size=4)
    with pytest.raises(NotImplementedError, match="test_time_aug"):
        tta.stream(2, 10)
    s = dec.stream(2, 10)
    with pytest.raises(RuntimeError, match="max_frames = 10"):
        s.push(torch.zeros(2, 11, 8))
    assert s.state is None
    with pytest.raises(RuntimeError, match="nothing was pushed"):
        s.finish()
