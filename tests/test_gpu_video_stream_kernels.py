"""GPU (-m gpu): the streamed visual stem at the ops level (ops.video_stem_stream -> ops.video_stream_advance), push by push against the chunked float64 reference of
tests/video_stream_ref.py.  B = 3 slots, Tc = 4 (Tin = Tmax = 6), both compute dtypes.

(a) exact: the integer operands of tests/stem_exact_ref.py (video in {-2 .. 2}, weights in {-1, 0, 1} with the tap cap and the one-hot channels, integer biases,
    power-of-two scale, a shift with exact zeros at the threshold, gamma < 0 on every fifth channel): every intermediate is an exact bf16 / fp32 value, so the streamed
    output must equal the reference bit for bit.  The slots receive the utterance lengths 1 .. 7, 11, 23 one after the other, restart mid-run and idle once ended, on
    the schedule and on the uneven plan, at 88x88, 96x96 and the smallest frame the kernel accepts (8x32).  The state blob and every output buffer are pre-filled with
    NaN bytes, chunk rows at or past n_frames[b] hold NaN: every valid output finite and exact, rows past out_len zero, out_len exact, an ended slot yields 0, the flag
    vectors zero after the advance.
(b) split invariance: one 0.5 * randn utterance of 11 frames at 88x88 runs in the three slots under three plans (schedule at Tc = 4, schedule at Tc = 2, uneven); the
    concatenated outputs are torch.equal.
(c) accuracy: the same run per element against the float64 reference; in the same test the offline ops.VideoStemFn (eval mode, B = 1, the whole utterance) is compared
    with the same reference, and the streamed worst element error may be at most 2 x the offline one's (the same operands; the margin covers another rounding point and
    another summation order).  Both figures are printed.  Measured on MI355X: DESIGN section 33.
"""
import functools

import pytest
import torch

from tests import stem_exact_ref as SR
from tests import video_stream_ref as VR

pytestmark = pytest.mark.gpu
TC, TIN, TMAX, B = 4, 6, 6, 3
UTTS = [[23, 1, 4], [11, 2, 5, 3], [7, 6]]
assert sorted(sum(UTTS, [])) == sorted(VR.LENGTHS)
NAMES = ("frame", "row", "column", "channel")


def _offsets(sizes):
    at = 0
    for c in sizes:
        yield at, c
        at += c


def _pushes(plans):
    """plans[b][ui] = the counts of utterance ui of slot b -> list of pushes; a push = per slot (utterance index or None, first frame, count, restart, last)"""
    queue = []
    for b, ut in enumerate(plans):
        q = []
        for ui, sizes in enumerate(ut):
            T = sum(sizes)
            q += [(ui, at, c, at == 0, at + c == T) for at, c in _offsets(sizes)]
        queue.append(q)
    n = max(len(q) for q in queue)
    return [[q[i] if i < len(q) else (None, 0, 0, False, False) for q in queue] for i in range(n)]


def _reference(data, pushes, H, W, k):
    """the chunked float64 reference of a run: per push, per slot the frames it yields"""
    fs = VR.VideoFrontStream(B, H, W, *k)
    refs = []
    for pi, row in enumerate(pushes):
        chunks = [data[b][ui][at:at + c] if ui is not None else None for b, (ui, at, c, _, _) in enumerate(row)]
        reset = {b for b, r in enumerate(row) if r[3]} | (set(range(B)) if pi == 0 else set())
        refs.append(fs.push(chunks, {b for b, r in enumerate(row) if r[4]}, reset))
    return refs


@functools.lru_cache(maxsize=None)
def _exact_case(H, W, plan):
    """operands and reference of one (frame, plan) of (a): computed once, shared by both dtypes"""
    kc = SR.channel_constants()
    k = (SR.stem_weights(), kc["bias"], kc["scale"], kc["shift"])
    gen = SR._gen("video stream %dx%d %s" % (H, W, plan))
    data = [[SR.ints(gen, (T, H, W), 2) for T in ut] for ut in UTTS]
    plans = [[VR.schedule_sizes(T, TC) if plan == "schedule" else VR.uneven_sizes(T, 3 * b + ui) for ui, T in enumerate(ut)] for b, ut in enumerate(UTTS)]
    pushes = _pushes(plans)
    return data, pushes, _reference(data, pushes, H, W, k), k


def _stream(ops, dtype, H, W, data, pushes, w, bias, ss):
    """the GPU side of a run -> per push (frames [Tmax][B][PH][PW][64] fp32 on the host, out_len list); w [64][245], bias [64], ss = scale | shift, fp32 on the device"""
    dev = "cuda"
    adt = torch.float32 if dtype == "f32" else torch.bfloat16
    PH, PW = ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1
    state = ops.video_stream_state(B, H, W, dev)
    assert state.numel() == B * (4 * H * W * (4 if dtype == "f32" else 2) + 16)
    state.fill_(0xFF)                                                      # NaN rings, counters of -1: the first push restarts every slot
    w8 = ops.video_stem_w8(w.view(64, 1, 5, 7, 7))
    rflags, lflags = torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    out = []
    for pi, row in enumerate(pushes):
        chunk = torch.full((B, TIN, H, W), float("nan"))
        for b, (ui, at, c, _, _) in enumerate(row):
            if ui is not None:
                chunk[b, :c] = data[b][ui][at:at + c].float()
        chunk = chunk.to(dev)
        nf = torch.tensor([r[2] for r in row], dtype=torch.int64, device=dev)
        rflags.copy_(torch.tensor([1 if (r[3] or pi == 0) else 0 for r in row], dtype=torch.uint8))
        lflags.copy_(torch.tensor([1 if r[4] else 0 for r in row], dtype=torch.uint8))
        frames = torch.full((TMAX, B, PH, PW, 64), float("nan"), dtype=adt, device=dev)
        out_len = torch.full((B,), -1, dtype=torch.int64, device=dev)
        ops.video_stem_stream(chunk, state, w8, bias, ss, nf, rflags, lflags, Tmax=TMAX, out=(frames, out_len))
        ops.video_stream_advance(chunk, state, nf, rflags, lflags)
        assert int(rflags.sum()) == 0 and int(lflags.sum()) == 0, "the advance consumes the flags"
        out.append((frames.float().cpu(), out_len.tolist()))
    return out


def _with_dtype(dtype, fn):
    import avec_amd
    from avec_amd import ops
    avec_amd.set_compute_dtype(dtype)
    try:
        return fn(ops)
    finally:
        avec_amd.set_compute_dtype("f32")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("plan", ["schedule", "uneven"])
@pytest.mark.parametrize("H,W", [(88, 88), (96, 96), (8, 32)])
def test_streamed_stem_is_exact(H, W, plan, dtype):
    data, pushes, refs, k = _exact_case(H, W, plan)
    SR.check_stem_exact({"bf16_wide": [torch.cat([r for ref in refs for r in ref])]})      # a few significant bits times a power of two: exact in bf16 and fp32
    w, bias, ss = k[0].float().cuda(), k[1].float().cuda(), torch.cat([k[2], k[3]]).float().cuda()
    got = _with_dtype(dtype, lambda ops: _stream(ops, dtype, H, W, data, pushes, w, bias, ss))
    total = [[0] * len(ut) for ut in UTTS]
    for pi, (row, ref, (frames, out_len)) in enumerate(zip(pushes, refs, got)):
        for b, (ui, at, c, _, fin) in enumerate(row):
            n = ref[b].shape[0]
            assert out_len[b] == n, (pi, b, out_len, n)
            assert n == (0 if ui is None else (at + c if fin else VR.ready(at + c)) - VR.ready(at))          # an ended slot yields 0
            assert bool(torch.isfinite(frames[:n, b]).all()), (pi, b)
            SR.assert_exact(frames[:n, b], ref[b], tuple(ref[b].shape), NAMES, "push %d slot %d (%r)" % (pi, b, row[b]))
            assert bool((frames[n:, b] == 0).all()), "rows past out_len are zero (push %d slot %d)" % (pi, b)
            if ui is not None:
                total[b][ui] += n
    assert total == UTTS


RAND_T, RAND_HW = 11, 88
RAND_PLANS = [[VR.schedule_sizes(RAND_T, 4)], [VR.schedule_sizes(RAND_T, 2)], [VR.uneven_sizes(RAND_T)]]


@functools.lru_cache(maxsize=None)
def _random_operands():
    g = torch.Generator().manual_seed(31)
    video = 0.5 * torch.randn(RAND_T, RAND_HW, RAND_HW, generator=g)
    import nnet
    stem = nnet.ConvNeuralNetwork(dim_input=1, dim_layers=64, kernel_size=(5, 7, 7), strides=(1, 2, 2), norm="BatchNorm3d", act_fun="ReLU", drop_rate=0.0, dim=3).layers[0]
    conv, bn = stem[0], stem[1]
    with torch.no_grad():
        conv.weight.copy_(0.08 * torch.randn(conv.weight.shape, generator=g)), conv.bias.copy_(0.1 * torch.randn(64, generator=g))
        bn.weight.copy_((0.5 + torch.rand(64, generator=g)) * torch.where(torch.arange(64) % 5 == 0, -1.0, 1.0)), bn.bias.copy_(0.2 * torch.randn(64, generator=g))
        bn.running_mean.copy_(0.3 * torch.randn(64, generator=g)), bn.running_var.copy_(0.5 + torch.rand(64, generator=g))
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.double() - bn.running_mean.double() * scale
    ref = VR.offline_stem(video.double(), conv.weight.detach().double().view(64, 245), conv.bias.detach().double(), scale.detach(), shift.detach())
    return video, conv, bn.eval(), ref


@functools.lru_cache(maxsize=None)
def _random_run(dtype):
    """-> (per plan the concatenated streamed output, the offline ops.VideoStemFn output), fp32 on the host"""
    video, conv, bn, _ = _random_operands()

    def run(ops):
        c, b = conv.to("cuda"), bn.to("cuda").eval()
        st = ops.BNState(64, c.weight)
        ops.bn_finalize(b, st, 1, False)
        data = [[video.double()] for _ in range(B)]
        got = _stream(ops, dtype, RAND_HW, RAND_HW, data, _pushes(RAND_PLANS), c.weight.detach().view(64, 245), c.bias.detach(), st.ss)
        cat = [torch.cat([frames[:out_len[s], s] for frames, out_len in got]) for s in range(B)]
        with torch.no_grad():
            off = ops.VideoStemFn.apply(video[None].to("cuda"), c.weight, c, b, False)
        return cat, off.float().cpu()
    return _with_dtype(dtype, run)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_split_invariance(dtype):
    cat, _ = _random_run(dtype)
    assert all(c.shape == (RAND_T, 22, 22, 64) for c in cat)
    assert torch.equal(cat[0], cat[1]) and torch.equal(cat[0], cat[2])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_accuracy_within_twice_the_offline_error(dtype):
    """measured on MI355X: see DESIGN section 33"""
    _, _, _, ref = _random_operands()
    cat, off = _random_run(dtype)
    e_off = float((off.double().view(ref.shape) - ref).abs().max())
    e_str = max(float((c.double() - ref).abs().max()) for c in cat)
    print("video stem %s: worst element error streamed %.3g, offline ops.VideoStemFn %.3g (reference magnitude %.3g)" % (dtype, e_str, e_off, float(ref.abs().max())))
    assert e_str <= 2 * e_off, (dtype, e_str, e_off)
