"""The look-ahead streaming encoder's semantics without a GPU: the chunked fp64 references of tests/stream_la_ref.py (window, ring of committed rows, carried context,
commit rule, restarts; state pre-filled with GARBAGE) equal the offline formulas on the whole utterance to 1e-12 for Tq = 1, 2, 4, 8; a toy stack pins the look-ahead
LA and its rounding LAe, and shows that committing S frames more is an error; the values of LA; argument validation of the four entry points; the session's
attributes, refusals and host-list contract."""
import pytest
import torch

from tests import rowwise_ref as RW
from tests import stream_la_ref as LR
from tests import stream_ref as SR

TOL = 1e-12
TQS = (1, 2, 4, 8)


def _close(got, ref):
    return all(g.shape == r.shape and float((g - r).abs().max()) < TOL for gb, rb in zip(got, ref) for g, r in zip(gb, rb))


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("L,R", [(0, 1), (3, 2), (6, 5), (7, 2)])
def test_attention_window_equals_offline_two_sided_band(L, R, S):
    """the stage behind total stride S sees L // S past and R // S future frames: the offline mask is the input-rate band strided [::S, ::S]"""
    H, d, Lk, Rk = 2, 5, L // S, R // S
    scale = 1.0 / d ** 0.5
    E = RW.gauss((Lk + Rk + 1, H, d), 3)
    for Tq in TQS:
        T0 = 3 * (Lk + Tq) + 2                                       # enough pushes to wrap the ring three times
        utts = [[T0, 7], [T0 // 2 + 1, T0], [2]]                      # restarts in the middle, short last chunks, a slot that runs out at once
        data = [[RW.gauss((T, 3, H, d), 100 * b + 10 * u) for u, T in enumerate(ut)] for b, ut in enumerate(utts)]
        ref = [[LR.attn_offline(x[:, 0], x[:, 1], x[:, 2], E, scale, LR.band(x.shape[0], L, R, S), Rk)[0] for x in ub] for ub in data]
        st = LR.AttnStreamLA(len(utts), H, d, Lk, Rk, Tq)
        got, win = LR.walk(utts, Tq, max(Rk, 1), 1, data, lambda X, n, c, reset: st.push(X[:, :, 0], X[:, :, 1], X[:, :, 2], E, scale, n, c, reset)[0])
        assert _close(got, ref), (L, R, S, Tq)
        assert st.pos == win.pos


@pytest.mark.parametrize("K", [15, 3])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_window_equals_offline(K, stride):
    C = 8
    utts = [[23, 9], [16, 30], [40]]
    data = [[RW.gauss((T, 2 * C), 40 + 10 * b + u) for u, T in enumerate(ut)] for b, ut in enumerate(utts)]
    w, bias = RW.gauss((K, C), 1), RW.gauss((C,), 2)
    ss = torch.stack([RW.coef(C, 2, positive=True), RW.coef(C, 3)])
    ref = [[SR.conv_offline(u, w, bias, ss, stride)[0] for u in ub] for ub in data]
    for Tq in TQS:
        for LAe in (stride, 3 * stride):
            st = SR.ConvStream(len(utts), C, K)
            got, win = LR.walk(utts, Tq * stride, LAe, stride, data, lambda X, n, c, reset: st.push(X, w, bias, ss, stride, c, reset)[0])
            assert _close(got, ref), (K, stride, Tq, LAe)
            assert st.pos == win.pos


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_toy_stack_pins_the_lookahead_and_one_stride_more_is_an_error(R):
    """attention -> stride-2 convolution -> attention at half rate: chunked with the commit rule it equals the offline toy; committing S = 2 frames more does not.
    The rule is tight in this toy for R = 1, 2, 4.  For R = 3 it is safe and one stride wide of tight: LA = 3 + 2 = 5 rounds up to LAe = 6, but rows exist only at
    even positions, the last committed one is at c - 2, and it needs input frames up to c - 2 + 5 < n already for c = n - 4; there only the equality is asserted."""
    H, d, L, K = 2, 4, 6, 5
    toy = LR.Toy(H, d, L, R, K)
    assert (toy.la, toy.lae, toy.S) == {1: (1, 2, 2), 2: (4, 4, 2), 3: (5, 6, 2), 4: (8, 8, 2)}[R]
    utts = [[40, 11], [33, 21], [18]]
    data = [[RW.gauss((T, H * d), 70 + 10 * b + u) for u, T in enumerate(ut)] for b, ut in enumerate(utts)]
    ref = [[toy.offline(x) for x in ub] for ub in data]
    for Tq in TQS:
        Tc = 2 * Tq
        got, _ = LR.walk(utts, Tc, toy.lae, 2, data, toy.session(len(utts), Tc))
        assert _close(got, ref), (R, Tq)
        if R == 3:
            continue
        bad, _ = LR.walk(utts, Tc, toy.lae, 2, data, toy.session(len(utts), Tc, extra=2), extra=2)
        assert all(g.shape == r.shape for gb, rb in zip(bad, ref) for g, r in zip(gb, rb))
        worst = max(float((g - r).abs().max()) for gb, rb in zip(bad, ref) for g, r in zip(gb, rb))
        assert worst > 1e-6, (R, Tq, worst)


def test_lookahead_values():
    assert [LR.lookahead([1, 2, 1], R)[:2] for R in (1, 2, 3)] == [(2, 2), (6, 6), (8, 8)]
    strides = [1] * 4 + [2] + [1] * 5 + [2] + [1] * 5                  # blocks [5, 6, 5], strides 2 and 2
    assert LR.lookahead(strides, 2) == (22, 24, 4)
    assert LR.lookahead(strides, 0) == (0, 0, 4)


def test_window_bookkeeping():
    """the window is the utterance's frames [pos, pos + n); pend <= LAe, commits are multiples of S and at most Tc; an ended slot takes nothing"""
    utts = [[23, 9], [5], [16, 30]]
    data = [[RW.gauss((T, 3), 10 * b + u) for u, T in enumerate(ut)] for b, ut in enumerate(utts)]
    for Tc, LAe, S in [(2, 2, 2), (4, 6, 2), (8, 2, 1), (4, 24, 4)]:
        win = LR.Window(len(utts), Tc, LAe, S, (3,))
        done = [0] * len(utts)
        for row in LR.schedule(utts, Tc):
            x = SR.chunk_of(data, [r[:4] for r in row], Tc, 3.0)
            last, reset = {b for b, r in enumerate(row) if r[4]}, {b for b, r in enumerate(row) if r[3]}
            X, n, c, emit = win.begin(x, [Tc if r[0] is None else r[2] for r in row], last, reset)       # (an ended slot is offered Tc frames and takes none)
            for b, (ui, t0, nb, rs, la) in enumerate(row):
                if rs:
                    done[b] = 0
                if ui is None:
                    assert n[b] == c[b] == emit[b] == 0
                    continue
                assert torch.equal(X[b, :n[b]], data[b][ui][done[b]:done[b] + n[b]]) and not bool(X[b, n[b]:].any())
                assert c[b] % S == 0 and c[b] <= Tc and n[b] <= Tc + LAe and (c[b] == 0 if la else c[b] == max(0, n[b] - LAe))
                assert emit[b] == (n[b] if la else c[b]) and (not la or done[b] + n[b] == utts[b][ui])
                done[b] += c[b]
            win.advance(X)
            assert all(p <= LAe for p in win.pend) and win.pos == done


def test_stream_la_entry_points_validate_arguments_without_gpu():
    """declared, exported, and each argument error is reported before any launch (no GPU needed)"""
    from avec_amd.lib import declared_functions, lib
    for name in ("avec_stream_window", "avec_stream_window_advance", "avec_glu_dwconv_stream_la", "avec_relpos_attention_stream_la"):
        assert name in declared_functions() and lib.raw(name) is not None
    assert lib.raw("avec_version")() == 4
    P = 4096                                                     # a fake, aligned address: nothing is dereferenced before the checks pass, and they do not pass

    def conv(u=P, w=P, bias=P, ss=P, out=P, state=P, state_bytes=1 << 20, pos=P, nc=P, B=3, Wq=6, C=8, K=15, stride=1, div=1):
        lib.glu_dwconv_stream_la(0, u, w, bias, ss, out, state, state_bytes, pos, None, nc, div, B, Wq, C, K, stride, None)
    for kw, msg in [(dict(u=None), "null pointer"), (dict(nc=None), "null pointer"), (dict(C=6), "multiple of 4"), (dict(K=17), "kernel size K=17"),
                    (dict(state=None), "null state"), (dict(state_bytes=3 * 14 * 16 * 4 - 1), "state of"), (dict(u=P + 4), "16-byte aligned"),
                    (dict(nc=P + 4), "8-byte aligned"), (dict(Wq=3, stride=2), "multiple of the stride"), (dict(Wq=90), "too long")]:
        with pytest.raises(RuntimeError, match="glu_dwconv_stream_la: .*" + msg):
            conv(**kw)

    def attn(q=P, k=P, v=P, e=P, kc=P, vc=2 * P, cache_bytes=1 << 20, pos=P, nv=P, nc=P, o=P, ld=48, lde=16, ldo=16, B=2, H=2, Wq=5, Tq=3, d=8, L=5, R=2, dtype=0):
        lib.relpos_attention_stream_la(dtype, q, k, v, ld, e, lde, kc, vc, cache_bytes, pos, None, nv, nc, 1, o, ldo, B, H, Wq, Tq, d, L, R, 0.35, None)
    for kw, msg in [(dict(q=None), "null pointer"), (dict(nv=None), "null pointer"), (dict(nc=None), "null pointer"), (dict(d=193), "bad dims"), (dict(R=-1), "bad dims"),
                    (dict(Wq=2), "bad dims"), (dict(ld=15), "row strides"), (dict(cache_bytes=2 * 8 * 16 * 4 - 1), "rings of"), (dict(k=P + 2), "misaligned"),
                    (dict(o=P + 1, dtype=1), "misaligned"), (dict(nc=P + 4), "misaligned"), (dict(vc=P), "two buffers")]:
        with pytest.raises(RuntimeError, match="relpos_attention_stream_la: .*" + msg):
            attn(**kw)

    def window(x=P, tail=2 * P, X=3 * P, pend=P, ended=P, nv=P, nc=P, emit=P, B=2, Tc=4, LAe=2, D=8, S=2):
        lib.stream_window(x, tail, X, pend, None, None, None, ended, nv, nc, emit, B, Tc, LAe, D, S, None)
    for kw, msg in [(dict(x=None), "null pointer"), (dict(tail=None), "null pointer"), (dict(emit=None), "null pointer"), (dict(Tc=3), "bad dims"), (dict(LAe=3), "bad dims"),
                    (dict(X=3 * P + 2), "misaligned"), (dict(pend=P + 4), "misaligned"), (dict(X=P), "buffer of its own")]:
        with pytest.raises(RuntimeError, match="stream_window: .*" + msg):
            window(**kw)

    def advance(X=3 * P, tail=2 * P, pend=P, pos=P, nv=P, nc=P, ended=P, B=2, W=6, LAe=2, D=8):
        lib.stream_window_advance(X, tail, pend, pos, nv, nc, None, None, ended, B, W, LAe, D, None)
    for kw, msg in [(dict(X=None), "null pointer"), (dict(pos=None), "null pointer"), (dict(W=2), "bad dims"), (dict(pos=P + 4), "misaligned"), (dict(tail=3 * P), "buffer of its own")]:
        with pytest.raises(RuntimeError, match="stream_window_advance: .*" + msg):
            advance(**kw)


ATT = {"class": "RelPos1dMultiHeadAttention", "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=64, weight_init="default", bias_init="default")}


def _net(mask, kernel_size=15, padding="causal"):
    import nnet
    return nnet.ConformerInterCTC(dim_model=[32, 48], num_blocks=[2, 1], interctc_blocks=[2], vocab_size=16, loss_prefix="c_ctc", att_params=ATT,
                                  conv_params={"class": "Conv1d", "params": {"padding": padding, "kernel_size": kernel_size}}, ff_ratio=4, drop_rate=0.1,
                                  mask=mask, conv_stride=2)


def test_session_attributes_and_refusals():
    import nnet
    from avec_amd.nnet.streaming import ConformerLookaheadStreamSession, ConformerStreamSession
    net = _net(nnet.Mask(left_context=6, right_context=1)).eval()
    with pytest.raises(NotImplementedError, match=r"stream: right_context=1 needs look-ahead buffering \(only right_context=0 is streamed\)"):
        net.stream(3, 4)
    ses = net.stream(3, 4, lookahead=True)
    assert type(ses) is ConformerLookaheadStreamSession and ses.lookahead == 2 and ses.window == 6 and ses.S == 2
    assert [(p["div"], p["L"], p["R"]) for p in ses.plan] == [(1, 6, 1), (1, 6, 1), (2, 3, 0)]
    for R, lae in [(2, 6), (3, 8)]:
        s2 = _net(nnet.Mask(left_context=6, right_context=R)).eval().stream(3, 8, lookahead=True)
        assert (s2.lookahead, s2.window) == (lae, 8 + lae)
    plain = _net(nnet.Mask(left_context=6, right_context=0)).eval().stream(3, 4, lookahead=True)
    assert type(plain) is ConformerStreamSession and [p["R"] for p in plain.plan] == [0, 0, 0]
    # the other refusals stay
    for make, exc, msg in [(lambda: _net(nnet.Mask(left_context=6, right_context=1), padding="same"), NotImplementedError, "padding='same'"),
                           (lambda: _net(nnet.Mask(right_context=1)), NotImplementedError, "left_context=None"),
                           (lambda: _net(nnet.Mask(left_context=6, right_context=1, mask_start=2)), NotImplementedError, "mask_start=2")]:
        with pytest.raises(exc, match=msg):
            make().eval().stream(3, 4, lookahead=True)
    with pytest.raises(RuntimeError, match="training mode"):
        _net(nnet.Mask(left_context=6, right_context=1)).train().stream(3, 4, lookahead=True)
    with pytest.raises(ValueError, match="multiple of the stack's total stride 2"):
        net.stream(3, 3, lookahead=True)
    with pytest.raises(ValueError, match=r"block 0 \(total stride 1\): the window of 78 \+ 6 frames"):          # K - 1 + Wq = 14 + 82 = 96 is the most
        _net(nnet.Mask(left_context=6, right_context=2)).eval().stream(3, 78, lookahead=True)
    assert _net(nnet.Mask(left_context=6, right_context=2)).eval().stream(3, 76, lookahead=True).window == 82


def test_host_list_contract():
    """checked on the host mirror of pend / pos / ended, before anything is launched (no GPU here)"""
    import nnet
    ses = _net(nnet.Mask(left_context=6, right_context=1)).eval().stream(3, 4, lookahead=True)
    first = ses._controls(None, None, None)
    assert first == ([True] * 3, [False] * 3, [4, 4, 4])
    ses._commit(*first)
    ses._first = False
    assert (ses._pend, ses._pos, ses._ended) == ([2, 2, 2], [2, 2, 2], [False] * 3)
    with pytest.raises(ValueError, match="slot 1 is running and takes exactly chunk_frames = 4 frames, got 2"):
        ses._controls([4, 2, 4], None, None)
    with pytest.raises(ValueError, match="outside 0 .. 4"):
        ses._controls([4, 5, 4], [1], None)
    with pytest.raises(ValueError, match="for 3 slots"):
        ses._controls([4, 4], None, None)
    c = ses._controls([4, 2, 0], [1, 2], None)                        # a slot in `last` takes any 0 .. Tc
    assert c == ([False] * 3, [False, True, True], [4, 2, 0])
    ses._commit(*c)
    assert (ses._pend, ses._pos, ses._ended) == ([2, 0, 0], [6, 2, 2], [False, True, True])
    with pytest.raises(RuntimeError, match="slot 1 has ended"):
        ses._controls([4, 4, 0], None, None)
    assert ses._controls(None, None, None)[2] == [4, 0, 0]             # an ended slot idles by default
    c = ses._controls([4, 4, 0], None, [1])                            # restarted: legal again
    ses._commit(*c)
    assert (ses._pend, ses._pos, ses._ended) == ([2, 2, 0], [10, 2, 2], [False, False, True])
    ses._commit([False] * 3, [False] * 3, None)                        # device-tensor counts: the host no longer knows
    with pytest.raises(RuntimeError, match="device-tensor counts"):
        ses._controls([4, 4, 4], None, None)
    assert ses._controls([4, 4, 4], None, [0, 1, 2])[2] == [4, 4, 4]


def test_lookahead_sinusoid_rows_are_the_offline_tables_rows():
    """the session's E input, delta = -R .. L, equals the sinusoid written out position by position"""
    from avec_amd import runtime as rt
    from avec_amd.nnet.streaming import ConformerLookaheadStreamSession
    for L, R in [(6, 1), (3, 5), (0, 2)]:
        D = 32
        pos = torch.arange(-R, L + 1, dtype=torch.float32).unsqueeze(1)
        inv = 10000 ** (2 * torch.arange(0, D // 2, dtype=torch.float32).unsqueeze(0) / D)
        pe = torch.zeros(L + R + 1, D)
        pe[:, 0::2], pe[:, 1::2] = (pos / inv).sin(), (pos / inv).cos()
        got = ConformerLookaheadStreamSession._pos_rows({"L": L, "R": R}, D, "cpu")
        assert got.shape == pe.shape and torch.equal(got, pe.to(rt.act_dtype()))
