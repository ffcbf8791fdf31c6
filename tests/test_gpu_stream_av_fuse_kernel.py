"""GPU (-m gpu): avec_av_fuse_stream (avec_amd/csrc/av_stream.hip) through ops.av_fuse_stream against the FIFO reference of tests/av_stream_ref.py, torch.equal.

Every expected row is torch.cat([a row, v row]) cast to the activation dtype (finite random values that need rounding in bf16); rows at or past pair_len are exact
zeros; pair_len is exact.  B = 3 slots, (Da, Dv) = (360, 360) and (8, 4), R = max_emit = 1 and 2 with cap = R + 2 (the rings wrap every few pushes), f32 and bf16.
The state blob starts as all-ones bytes (NaN rows, counters of -1: only the first push's reset makes it a state), the outputs and the input rows at or past the
lengths are NaN before every launch.  Plans, side by side in the three slots and shifted against each other: the row counts the joint schedule implies for utterances of
1 .. 7, 11 and 23 frames (one after the other, restarted); an uneven plan where the audio branch runs ahead until its ring is full and is drained, then the video branch;
pushes of zero rows; a slot restarted with rows still pending (they must vanish); idle slots.  After a push a launch with zero new rows follows while the reference has
a pair pending, and after every other push regardless (it must then emit nothing)."""
import pytest
import torch

from tests import av_stream_ref as AR

pytestmark = pytest.mark.gpu
B = 3
IDLE = (0, 0, False)
NAN = float("nan")


def scheduled(Ts, R):
    ev = []
    for T in Ts:
        rows = AR.branch_rows(T, 640 * T - 160, 2 * R)[0]
        ev += [(ra, rv, i == 0) for i, (ra, rv) in enumerate(rows)]
    return ev


def uneven(R):
    """audio alone until its ring holds cap rows, video until they are paired, then the other way round (at most R + 1 rows per push)"""
    cap, ev = R + 2, []
    for audio in (True, False):
        n = 0
        while n < cap:
            c = min(R + 1, cap - n)
            ev.append((c, 0, False) if audio else (0, c, False))
            n += c
        n = 0
        while n < cap:
            c = min(R + 1, cap - n)
            ev.append((0, c, False) if audio else (c, 0, False))
            n += c
    return ev


def restarted_with_rows_pending(R):
    return [(R + 1, 0, True), (0, 1, False), (1, 1, True), IDLE, (0, 0, True), (1, 0, False), (0, 1, False)]


def plan(R):
    slots = [scheduled([1, 2, 3, 4, 5, 6, 7, 11, 23], R),
             [(0, 0, True)] + uneven(R) + [IDLE] * 2 + restarted_with_rows_pending(R) + scheduled([23, 5], R),
             [(0, 0, True)] + [IDLE] * 3 + restarted_with_rows_pending(R) + scheduled([6], R) + [(0, 0, True)] + uneven(R) + uneven(R)]
    n = max(len(s) for s in slots)
    return [[s[i] if i < len(s) else IDLE for s in slots] for i in range(n)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("dims", [(360, 360), (8, 4)])
def test_fuse_stream_equals_the_fifo_reference(dims, R, dtype):
    import avec_amd
    from avec_amd import ops
    Da, Dv = dims
    cap, Rin = R + 2, R + 1
    avec_amd.set_compute_dtype(dtype)
    try:
        adt = torch.bfloat16 if dtype == "bf16" else torch.float32
        state = ops.av_fuse_stream_state(B, Da, Dv, cap, "cuda")
        assert state.numel() == (B * (cap * (Da + Dv) * state.new_empty(0, dtype=adt).element_size() + 24) + 15) // 16 * 16
        state.fill_(255)
        ref = AR.FuseRef(B, cap, adt)
        flags = torch.zeros(B, dtype=torch.uint8, device="cuda")
        zero = torch.zeros(B, dtype=torch.int64, device="cuda")
        g = torch.Generator().manual_seed(R * 1000 + Da)
        emitted, seconds, wrapped = 0, 0, [0] * B

        def launch(a, la, v, lv, reset):
            xc = torch.full((B, R, Da + Dv), NAN, dtype=adt, device="cuda")
            plen = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            if reset:
                flags.copy_(torch.tensor([b in reset for b in range(B)], dtype=torch.uint8))
            out = ops.av_fuse_stream(a.cuda(), torch.tensor(la).cuda() if la is not None else zero, v.cuda(), torch.tensor(lv).cuda() if lv is not None else zero,
                                     state, flags if reset else None, R, out=(xc, plen))
            assert out[0] is xc and out[1] is plen
            want, wlen = ref.push(a, la or [0] * B, v, lv or [0] * B, reset, R)
            assert plen.tolist() == wlen, (plen.tolist(), wlen)
            assert torch.equal(xc.cpu(), want), (la, lv, reset, wlen)
            assert not flags.any()                                       # consumed
            return sum(wlen)

        for pi, row in enumerate(plan(R)):
            a, v = torch.randn(B, Rin, Da, generator=g), torch.randn(B, Rin, Dv, generator=g)
            la, lv, reset = [r[0] for r in row], [r[1] for r in row], tuple(b for b, r in enumerate(row) if r[2])
            for b in range(B):
                a[b, la[b]:], v[b, lv[b]:] = NAN, NAN
                wrapped[b] = 0 if b in reset else wrapped[b] + la[b]
            emitted += launch(a, la, v, lv, reset)
            nothing = torch.full((B, Rin, Da), NAN), torch.full((B, Rin, Dv), NAN)
            while any(min(len(ref.fa[b]), len(ref.fv[b])) for b in range(B)):
                emitted, seconds = emitted + launch(nothing[0], None, nothing[1], None, ()), seconds + 1
            if pi % 2:
                assert launch(nothing[0], None, nothing[1], None, ()) == 0
        assert seconds >= 4 and emitted >= 40 and max(wrapped) > 2 * cap, (seconds, emitted, wrapped)
    finally:
        avec_amd.set_compute_dtype("f32")


def test_wrapper_refuses_before_any_launch():
    from avec_amd import ops
    state = ops.av_fuse_stream_state(B, 8, 4, 4, "cuda")
    a, v = torch.zeros(B, 3, 8, device="cuda"), torch.zeros(B, 3, 4, device="cuda")
    n = torch.zeros(B, dtype=torch.int64, device="cuda")
    ops.av_fuse_stream(a, n, v, n, state, None, 2)
    with pytest.raises(ValueError, match="a_len must be a contiguous int64"):
        ops.av_fuse_stream(a, n.int(), v, n, state, None, 2)
    with pytest.raises(ValueError, match="a_len and v_len are required"):
        ops.av_fuse_stream(a, None, v, n, state, None, 2)
    with pytest.raises(ValueError, match="fp32, contiguous"):
        ops.av_fuse_stream(a.double(), n, v, n, state, None, 2)
    with pytest.raises(ValueError, match="fp32, contiguous"):
        ops.av_fuse_stream(a[:, :, ::2], n, v, n, state, None, 2)
    with pytest.raises(RuntimeError, match="at least max_emit \\+ 2"):
        ops.av_fuse_stream(a, n, v, n, state, None, 3)
    with pytest.raises(RuntimeError, match="state of"):
        ops.av_fuse_stream(a, n, v, n, ops.av_fuse_stream_state(B, 8, 8, 4, "cuda"), None, 2)         # a state of another shape
    with pytest.raises(ValueError, match="out ="):
        ops.av_fuse_stream(a, n, v, n, state, None, 2, out=(torch.zeros(B, 2, 12, device="cuda", dtype=torch.float64), n))
    with pytest.raises(ValueError, match="no state"):
        ops.av_fuse_stream_state(B, 6, 4, 4, "cuda")
