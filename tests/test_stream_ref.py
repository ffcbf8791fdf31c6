"""The streaming encoder's semantics without a GPU: the chunked fp64 references of tests/stream_ref.py (the state the kernels keep: carried context rows, ring cache,
position counters, restarts) equal the plain offline formulas on the whole utterance to 1e-12, for every split into chunks tried; the band is the offline stack's own
(oracle.context_mask strided [::S, ::S], which pins L_k = L // S_k); argument validation of the two entry points; the session's refusals."""
import pytest
import torch

from tests import rowwise_ref as RW
from tests import stream_ref as SR

TOL = 1e-12


def _walk(utts, Tq, push, out_rows):
    """drive `push(chunk inputs, n, reset)` over the schedule and collect, per (slot, utterance), the rows it produced"""
    got = [[[] for _ in u] for u in utts]
    for row in SR.schedule(utts, Tq):
        n = [r[2] for r in row]
        reset = {b for b, r in enumerate(row) if r[3]}
        out = push(row, n, reset)
        for b, (ui, _, nb, _) in enumerate(row):
            if ui is not None:
                got[b][ui].append(out[b][:out_rows(nb)])
    return [[torch.cat(g) for g in gb] for gb in got]


@pytest.mark.parametrize("K", [15, 3])
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_chunked_equals_offline(K, stride):
    C = 8
    utts = [[23, 9], [16, 30], [40]]                 # a reset in the middle (every second utterance), short last chunks, a slot that runs out
    data = [[RW.gauss((T, 2 * C), 40 + 10 * b + u) for u, T in enumerate(ut)] for b, ut in enumerate(utts)]
    w, bias = RW.gauss((K, C), 1), RW.gauss((C,), 2)
    ss = torch.stack([RW.coef(C, 2, positive=True), RW.coef(C, 3)])
    ref = [[SR.conv_offline(u, w, bias, ss, stride)[0] for u in ub] for ub in data]
    for Tq in [stride * m for m in (1, 2, 3, 5, 8)] + [40]:
        st = SR.ConvStream(len(utts), C, K)
        got = _walk(utts, Tq, lambda row, n, reset: st.push(SR.chunk_of(data, row, Tq, 3.0), w, bias, ss, stride, n, reset)[0], lambda nb: -(-nb // stride))
        for b, ub in enumerate(ref):
            for ui, r in enumerate(ub):
                assert got[b][ui].shape == r.shape and float((got[b][ui] - r).abs().max()) < TOL, (K, stride, Tq, b, ui)


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("L", [0, 1, 6, 7])
def test_attention_chunked_equals_offline_band(L, S):
    """the stage behind total stride S sees L_k = L // S: the offline mask is the input-rate band strided [::S, ::S]"""
    H, d, Lk = 2, 5, L // S
    scale = 1.0 / d ** 0.5
    E = RW.gauss((Lk + 1, H, d), 3)
    for Tq in (1, 2, 3, 8, 33):
        cap = Lk + Tq
        T0 = max(3 * cap + 2, 33) if Tq < 33 else 33            # enough pushes to wrap the ring three times
        utts = [[T0, 7], [T0 // 2 + 1, T0]]                      # resets in the middle, short last chunks
        data = [[[RW.gauss((T, H, d), 100 * b + 10 * u + n) for n in range(3)] for u, T in enumerate(ut)] for b, ut in enumerate(utts)]
        ref = [[SR.attn_offline(q, k, v, E, scale, SR.band(q.shape[0], L, S))[0] for q, k, v in ub] for ub in data]
        st = SR.AttnStream(len(utts), H, d, Lk, Tq)
        part = lambda j: [[x[j] for x in ub] for ub in data]

        def push(row, n, reset):
            q, k, v = (SR.chunk_of(part(j), row, Tq, 2.0) for j in range(3))
            return st.push(q, k, v, E, scale, n, reset)[0]
        got = _walk(utts, Tq, push, lambda nb: nb)
        for b, ub in enumerate(ref):
            for ui, r in enumerate(ub):
                assert float((got[b][ui] - r).abs().max()) < TOL, (L, S, Tq, b, ui)


def test_band_is_the_strided_offline_mask():
    for L in (0, 1, 6, 7):
        for S in (1, 2, 4):
            m = SR.band(9, L, S)
            i, j = torch.arange(9)[:, None], torch.arange(9)[None, :]
            assert torch.equal(m, (i - j >= 0) & (i - j <= L // S)), (L, S)


def test_conv_host_model_ratio_is_the_recorded_one():
    w = SR.measure_conv_host()
    assert w <= SR.CONV_HOST_WORST and w > SR.CONV_HOST_WORST / 4, w


def test_stream_entry_points_validate_arguments_without_gpu():
    """each argument error has its own message and is reported before any launch (no GPU needed)"""
    from avec_amd.lib import lib
    sb = lib.raw("avec_glu_dwconv_stream_state_bytes")
    assert sb(0, 3, 36, 15) == 3 * 14 * 72 * 4 and sb(1, 3, 36, 15) == 3 * 14 * 72 * 2 and sb(0, 2, 8, 1) == 0
    ab = lib.raw("avec_relpos_attention_stream_state_bytes")
    assert ab(1, 2, 2, 45, 5, 3) == 2 * 8 * 90 * 2 and ab(0, 2, 2, 45, 0, 1) == 2 * 1 * 90 * 4
    P = 4096                                                     # a fake, aligned address: nothing is dereferenced before the checks pass, and they do not pass

    def conv(u=P, w=P, bias=P, ss=P, out=P, state=P, state_bytes=1 << 20, pos=P, B=3, Tq=4, C=8, K=15, stride=1, div=1):
        lib.glu_dwconv_stream(0, u, w, bias, ss, out, state, state_bytes, pos, None, None, div, B, Tq, C, K, stride, None)
    for kw, msg in [(dict(u=None), "null pointer"), (dict(pos=None), "null pointer"), (dict(C=6), "multiple of 4"), (dict(K=17), "kernel size K=17"),
                    (dict(state=None), "null state"), (dict(state_bytes=3 * 14 * 16 * 4 - 1), "state of"), (dict(u=P + 4), "16-byte aligned"),
                    (dict(state=P + 8), "16-byte aligned"), (dict(pos=P + 4), "8-byte aligned"), (dict(Tq=3, stride=2), "multiple of the stride"),
                    (dict(Tq=90), "too long")]:
        with pytest.raises(RuntimeError, match=msg):
            conv(**kw)

    def attn(q=P, k=P, v=P, e=P, kc=P, vc=2 * P, cache_bytes=1 << 20, pos=P, o=P, ld=48, lde=16, ldo=16, B=2, H=2, Tq=3, d=8, L=5, dtype=0):
        lib.relpos_attention_stream(dtype, q, k, v, ld, e, lde, kc, vc, cache_bytes, pos, None, None, 1, o, ldo, B, H, Tq, d, L, 0.35, None)
    for kw, msg in [(dict(q=None), "null pointer"), (dict(kc=None), "null pointer"), (dict(d=193), "bad dims"), (dict(L=-1), "bad dims"), (dict(ld=15), "row strides"),
                    (dict(cache_bytes=2 * 8 * 16 * 4 - 1), "rings of"), (dict(k=P + 2), "misaligned"), (dict(o=P + 1, dtype=1), "misaligned"), (dict(pos=P + 4), "misaligned"),
                    (dict(vc=P), "two buffers")]:
        with pytest.raises(RuntimeError, match=msg):
            attn(**kw)
    with pytest.raises(RuntimeError, match="stream_advance"):
        lib.stream_advance(None, None, None, 4, 2, None)


ATT = lambda cls, **kw: {"class": cls, "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=64, weight_init="default", bias_init="default", **kw)}


def _net(att=None, padding="causal", mask=None, **kw):
    import nnet
    return nnet.ConformerInterCTC(dim_model=[32, 48], num_blocks=[2, 1], interctc_blocks=[2], vocab_size=16, loss_prefix="c_ctc",
                                  att_params=att or ATT("RelPos1dMultiHeadAttention"),
                                  conv_params={"class": "Conv1d", "params": {"padding": padding, "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                  mask=mask or nnet.Mask(left_context=6, right_context=0), conv_stride=2, **kw)


def test_session_refusals_name_their_cause():
    """every unsupported stack is refused when the session is made, before any launch (no GPU here)"""
    import nnet
    grouped = {"class": "GroupedRelPosMultiHeadSelfAttention", "params": {"num_heads": 4, "group_size": 1, "attn_drop_rate": 0.0, "max_pos_encoding": 64, "causal": False}}
    for make, exc, msg in [
            (lambda: _net(att=[ATT("RelPosPatch1dMultiHeadAttention", patch_size=3), ATT("RelPos1dMultiHeadAttention")]), NotImplementedError, "patch attention"),
            (lambda: _net(att=grouped), NotImplementedError, "grouped"),
            (lambda: _net(padding="same"), NotImplementedError, "padding='same'"),
            (lambda: _net(mask=nnet.Mask(left_context=6, right_context=1)), NotImplementedError, "right_context=1"),
            (lambda: _net(mask=nnet.Mask(right_context=0)), NotImplementedError, "left_context=None"),
            (lambda: _net(mask=nnet.Mask(left_context=6, right_context=0, mask_start=2)), NotImplementedError, "mask_start=2")]:
        with pytest.raises(exc, match=msg):
            make().eval().stream(3, 4)
    with pytest.raises(RuntimeError, match="training mode"):
        _net().train().stream(3, 4)
    with pytest.raises(ValueError, match="multiple of the stack's total stride 2"):
        _net().eval().stream(3, 3)
    ses = _net(att=ATT("RelPos1dMultiHeadAttention", causal=True)).eval().stream(3, 4)
    assert [(p["div"], p["L"]) for p in ses.plan] == [(1, 6), (1, 6), (2, 3)] and ses.S == 2
    # the host-list contract: a slot that ended short must be reset before it is pushed to again (checked on the host, before the chunk is looked at)
    ses._first = False
    ses._short = [False, True, False]
    with pytest.raises(RuntimeError, match="slot 1 ended with a short chunk"):
        ses._controls([4, 4, 4], None)
    with pytest.raises(RuntimeError, match="slot 1 ended with a short chunk"):
        ses._controls(None, [0])
    assert ses._controls([4, 2, 4], [1]) == ([False, True, False], [4, 2, 4])
    assert ses._controls([4, 0, 4], None) == (None, [4, 0, 4])         # a slot that has ended may idle on chunks of 0 frames


def test_slot_mask():
    """reset / last in every accepted form -> the one bool list [B]"""
    from avec_amd.nnet.streaming import slot_mask
    assert slot_mask(None, 3) == [False, False, False]
    assert slot_mask([1], 3) == slot_mask([False, True, False], 3) == [False, True, False]
    t = torch.tensor([True, False, True])
    assert slot_mask(t, 3) == t.tolist() == [True, False, True]
    assert slot_mask(torch.tensor([2]), 3) == [False, False, True]
    assert slot_mask([0, 1, 2], 3) == [True, True, True]               # B ints are indices, not a mask
    assert slot_mask([], 3) == [False, False, False]


def test_stream_sinusoid_table_is_the_offline_tables_rows():
    """the session's E input, delta = 0 .. L: the first L + 1 rows of ops.rel_pos_table(L + 1, D) flipped equal the table written out position by position"""
    from avec_amd import ops
    from avec_amd import runtime as rt
    L, D = 6, 32
    pos = torch.arange(0, L + 1, dtype=torch.float32).unsqueeze(1)
    inv = 10000 ** (2 * torch.arange(0, D // 2, dtype=torch.float32).unsqueeze(0) / D)
    pe = torch.zeros(L + 1, D)
    pe[:, 0::2], pe[:, 1::2] = (pos / inv).sin(), (pos / inv).cos()
    pe = pe.to(rt.act_dtype())
    got = ops.rel_pos_table(L + 1, D, "cpu")[:L + 1].flip(0)
    assert got.dtype == pe.dtype and torch.equal(got, pe)
