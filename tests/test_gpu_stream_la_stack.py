"""GPU (-m gpu): ConformerInterCTC.stream(lookahead=True) -- a stack with right_context > 0 run chunk by chunk (nnet.ConformerLookaheadStreamSession) -- against the
CPU oracle on each WHOLE utterance.

The stack, slots, utterances and chunk sizes are those of tests/test_gpu_stream_stack.py (dims [32, 48], blocks [2, 1], InterCTC after block 2, conv stride 2, K = 15
causal, B = 3, utterances [40], [33, 21], [18, 30], Tc = 2, 4, 8, 40) with non-causal position tables and Mask(6, 2) (LAe = 6) or Mask(6, 1) (LAe = 2; the strided
stage is then causal: R // 2 = 0).  Every utterance's last chunk carries `last`; the rows a slot emits trail its input by LAe frames and the last push emits the rest.

Judged against O.conformer_interctc(train=False, context=(6, R, 0), causal_conv=True) per whole utterance: lengths equal, every valid row compared.
f32: rel_err < 1e-3 (the project's parity bound) and <= max(2 x the offline GPU forward's error against the same oracle, 1e-5): 2 x is the project's margin for "same
operands, other summation order"; 1e-5 sits an order under the smallest effect of a commit one row too early (1.2e-4, measured on the CPU in fp64) and an order over
fp32 noise.  bf16: at most 2 x the offline GPU error measured in the same test.  Measured ratios: DESIGN section 36.
"""
import functools

import pytest
import torch

from oracle import avec_oracle as O
from tests import stream_la_ref as LR
from tests import stream_ref as SR
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
ATT = {"class": "RelPos1dMultiHeadAttention", "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=64, weight_init="default", bias_init="default")}
UTTS = [[40], [33, 21], [18, 30]]
D0, KEY, S = 32, "c_ctc_1", 2
LAE = {2: 6, 1: 2}


def make_net(R):
    import nnet
    torch.manual_seed(4321)
    net = nnet.ConformerInterCTC(dim_model=[32, 48], num_blocks=[2, 1], interctc_blocks=[2], vocab_size=16, loss_prefix="c_ctc", att_params=ATT,
                                 conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                 mask=nnet.Mask(left_context=6, right_context=R), conv_stride=2)
    g = torch.Generator().manual_seed(99)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):              # running statistics that are not the identity
            m.running_mean.copy_(0.3 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    return net.eval()


@functools.lru_cache(maxsize=2)
def fixture(R):
    """(inputs data[b][utterance] [T][32], oracle results per (slot, utterance): (y, ylen, logits, loglen)) -- computed once per mask, never modified"""
    net = make_net(R)
    sd = {"m." + k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    data = [[torch.randn(T, D0, generator=g) for T in ut] for ut in UTTS]
    ref = []
    for ub in data:
        row = []
        for x in ub:
            with torch.no_grad():
                y, ylen, inter = O.conformer_interctc(sd, "m", x[None], torch.tensor([x.shape[0]]), [2, 1], [2], "c_ctc", [1, 1], False, {}, context=(6, R, 0), causal_conv=True)
            row.append((y[0], int(ylen[0]), inter[KEY][0][0], int(inter[KEY][1][0])))
        ref.append(row)
    return data, ref


def gpu_net(R, dtype):
    import avec_amd
    avec_amd.set_compute_dtype(dtype)
    return make_net(R).to("cuda").eval()


def streamed(net, R, Tc, capture=False, chunk_len="list", sync_free=False):
    """walk the schedule; -> per (slot, utterance) (y rows, sum of out_len, logits rows, sum of logit lengths), the per-push raw outputs (cloned), the session"""
    data, _ = fixture(R)
    B = len(UTTS)
    ses = net.stream(B, Tc, lookahead=True)
    assert ses.lookahead == LAE[R] and ses.window == Tc + LAE[R]
    if capture:
        ses.capture()
    book = LR.Window(B, Tc, ses.lookahead, S, (1,))            # the host reference of the window bookkeeping: what every push must emit
    got = [[[[], 0, [], 0] for _ in ut] for ut in UTTS]
    raw = []
    for pi, row in enumerate(LR.schedule(UTTS, Tc)):
        x = SR.chunk_of(data, [r[:4] for r in row], Tc, 0.5).cuda()
        n = [r[2] for r in row]
        reset, last = [b for b, r in enumerate(row) if r[3]], [b for b, r in enumerate(row) if r[4]]
        cl = n if chunk_len == "list" else torch.tensor(n, dtype=torch.int64, device="cuda")
        if sync_free and pi > 0:
            torch.cuda.set_sync_debug_mode("error")
        try:
            y, ylen, inter = ses.push(x, cl, last or None, reset or None)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        X, _, _, emit = book.begin(torch.zeros(B, Tc, 1, dtype=torch.float64), n, set(last), set(reset))
        book.advance(X)
        lg, lglen = inter[KEY]
        assert y.shape[:2] == lg.shape[:2] == (B, ses.window // S)
        raw.append((y.clone(), ylen.clone(), lg.clone(), lglen.clone()))
        yl, ll = ylen.tolist(), lglen.tolist()
        for b, (ui, _, _, _, _) in enumerate(row):
            assert yl[b] == ll[b] == -(-emit[b] // S), (pi, b, yl, ll, emit)
            if ui is not None:
                acc = got[b][ui]
                acc[0].append(y[b, :yl[b]].float().cpu()), acc[2].append(lg[b, :ll[b]].float().cpu())
                acc[1] += yl[b]
                acc[3] += ll[b]
        if chunk_len == "list":
            assert (ses._pend, ses._pos, ses._ended) == (book.pend, book.pos, book.ended), pi
    if chunk_len == "list":
        assert ses.pos.tolist() == ses._pos                    # the device counter is where the host mirror predicts it
    return [[(torch.cat(a[0]), a[1], torch.cat(a[2]), a[3]) for a in gb] for gb in got], raw, ses


def offline(net, R):
    """the offline GPU forward on the padded batches of first and second utterances -> per (slot, utterance) (y valid rows, logits valid rows)"""
    data, ref = fixture(R)
    out = [[None] * len(ut) for ut in UTTS]
    for ui in range(2):
        slots = [b for b, ut in enumerate(UTTS) if ui < len(ut)]
        T = max(UTTS[b][ui] for b in slots)
        x = torch.zeros(len(slots), T, D0)
        for k, b in enumerate(slots):
            x[k, :UTTS[b][ui]] = data[b][ui]
        with torch.no_grad():
            y, ylen, inter = net(x.cuda(), torch.tensor([UTTS[b][ui] for b in slots]).cuda())
        for k, b in enumerate(slots):
            n = ref[b][ui][1]
            assert int(ylen[k]) == n
            out[b][ui] = (y[k, :n].float().cpu(), inter[KEY][0][k, :n].float().cpu())
    return out


@pytest.mark.parametrize("Tc", [2, 4, 8, 40])
@pytest.mark.parametrize("R", [2, 1])
def test_lookahead_stream_f32_matches_oracle(R, Tc):
    _, ref = fixture(R)
    net = gpu_net(R, "f32")
    off = offline(net, R)
    got, _, _ = streamed(net, R, Tc)
    bad = []
    for b, ub in enumerate(ref):
        for ui, (y, ylen, lg, lglen) in enumerate(ub):
            gy, gyl, gl, gll = got[b][ui]
            assert gyl == ylen and gll == lglen and gy.shape == y.shape and gl.shape == lg.shape, (R, Tc, b, ui, gyl, ylen, gll, lglen)
            ey, el, oy, ol = rel_err(gy, y), rel_err(gl, lg), rel_err(off[b][ui][0], y), rel_err(off[b][ui][1], lg)
            print("R=%d Tc=%d slot %d utterance %d: streamed y %.3g logits %.3g | offline GPU y %.3g logits %.3g" % (R, Tc, b, ui, ey, el, oy, ol))
            if not (ey < 1e-3 and el < 1e-3 and ey <= max(2 * oy, 1e-5) and el <= max(2 * ol, 1e-5)):
                bad.append((b, ui, ey, oy, el, ol))
    assert not bad, bad


@pytest.mark.parametrize("Tc", [2, 4, 8, 40])
@pytest.mark.parametrize("R", [2, 1])
def test_lookahead_stream_bf16_within_twice_the_offline_error(R, Tc):
    _, ref = fixture(R)
    net = gpu_net(R, "bf16")
    try:
        off = offline(net, R)
        got, _, _ = streamed(net, R, Tc)
    finally:
        import avec_amd
        avec_amd.set_compute_dtype("f32")
    bad = []
    for b, ub in enumerate(ref):
        for ui, (y, ylen, lg, lglen) in enumerate(ub):
            gy, gyl, gl, gll = got[b][ui]
            assert gyl == ylen and gll == lglen and gy.shape == y.shape and gl.shape == lg.shape
            ey, el, oy, ol = rel_err(gy, y), rel_err(gl, lg), rel_err(off[b][ui][0], y), rel_err(off[b][ui][1], lg)
            print("bf16 R=%d Tc=%d slot %d utterance %d: streamed y %.3g logits %.3g | offline GPU y %.3g logits %.3g" % (R, Tc, b, ui, ey, el, oy, ol))
            if not (ey <= 2 * oy and el <= 2 * ol):
                bad.append((b, ui, ey, oy, el, ol))
    assert not bad, bad


def test_chunking_invariance_and_device_counts():
    net = gpu_net(2, "f32")
    a, _, _ = streamed(net, 2, 2)
    b, _, _ = streamed(net, 2, 8, chunk_len="tensor")
    for ga, gb in zip(a, b):
        for (ya, na, la, _), (yb, nb, lb, _) in zip(ga, gb):
            assert na == nb and rel_err(ya, yb) < 1e-3 and rel_err(la, lb) < 1e-3


def test_captured_pushes_equal_eager_pushes():
    net = gpu_net(2, "f32")
    _, eager, _ = streamed(net, 2, 4)
    _, graph, _ = streamed(net, 2, 4, capture=True)
    assert len(eager) == len(graph) >= 3
    for pi, (e, g) in enumerate(zip(eager, graph)):
        for te, tg in zip(e, g):
            assert torch.equal(te, tg), pi


def test_pushes_do_not_synchronise_or_grow():
    net = gpu_net(2, "f32")
    streamed(net, 2, 4, sync_free=True)                               # host-list counts, `last` and restarts under torch's sync debug mode
    ses = net.stream(3, 4, lookahead=True)
    x = torch.randn(3, 4, D0, device="cuda")
    out = ses.push(x)
    del out
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(50):
            out = ses.push(x, [4, 4, 4], None, [i % 3] if i % 7 == 0 else None)
            del out
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    # restarts at i = 42 (slot 0), 49 (slot 1), 35 (slot 2): 8, 1 and 15 pushes of 4 frames since, of which all but the last LAe = 6 are committed (never below 0)
    assert ses._pos == [26, 0, 54] and ses.pos.tolist() == ses._pos and ses.win.pend.tolist() == ses._pend == [6, 4, 6]


def test_host_list_contract_on_the_gpu():
    net = gpu_net(1, "f32")
    ses = net.stream(3, 4, lookahead=True)
    x = torch.randn(3, 4, D0, device="cuda")
    ses.push(x)
    with pytest.raises(ValueError, match="slot 1 is running and takes exactly"):
        ses.push(x, [4, 2, 4])
    _, ylen, _ = ses.push(x, [4, 2, 4], [1])                          # LAe = 2: slot 1 has 2 frames pending + 2 new, all 4 emitted as 2 rows; the others commit 4
    assert ylen.tolist() == [2, 2, 2]
    with pytest.raises(RuntimeError, match="slot 1 has ended"):
        ses.push(x, [4, 4, 4])
    _, ylen, _ = ses.push(x)                                          # the ended slot idles
    assert ylen.tolist() == [2, 0, 2]
    _, ylen, _ = ses.push(x, [4, 4, 4], None, [1])                    # restarted: legal again, 4 - 2 frames committed
    assert ylen.tolist() == [2, 1, 2]
    with pytest.raises(ValueError, match="chunk"):
        ses.push(x[:, :2])
