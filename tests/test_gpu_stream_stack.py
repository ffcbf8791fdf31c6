"""GPU (-m gpu): ConformerInterCTC.stream() -- a causal stack run chunk by chunk (nnet.ConformerStreamSession) -- against the CPU oracle on each WHOLE utterance.

The stack is tests/test_streaming.py's causal one with RelPos1dMultiHeadAttention in both stages: dims [32, 48], blocks [2, 1], InterCTC after block 2, conv stride 2,
K = 15 causal, Mask(left_context=6, right_context=0), seeded weights and running statistics, eval mode.  B = 3 slots, T = 40, lengths [40, 33, 18]; chunk sizes 2, 4, 8
and 40; the shorter utterances end with a short chunk, their slots are then restarted and fed a second utterance (lengths 21 and 30), judged as strictly as the first.

f32: valid rows of y, the InterCTC logits and every length against O.conformer_interctc(train=False, context=(6, 0, 0), causal_conv=True): rel_err < 1e-3 (the
project's parity bound), lengths equal; the offline GPU forward's error against the same oracle is printed beside it.
bf16: no bound taken in advance -- the offline GPU forward's bf16 error against the oracle is measured in the same test, per utterance and tensor, and the streamed
result may be at most 2 x that (the margin is for the different summation order over the same operands).
"""
import functools

import pytest
import torch

from oracle import avec_oracle as O
from tests import stream_ref as SR
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
ATT = lambda cls, **kw: {"class": cls, "params": dict(num_heads=4, attn_drop_rate=0.0, num_pos_embeddings=64, weight_init="default", bias_init="default", **kw)}
UTTS = [[40], [33, 21], [18, 30]]
D0, KEY = 32, "c_ctc_1"


def make_net():
    import nnet
    torch.manual_seed(4321)
    net = nnet.ConformerInterCTC(dim_model=[32, 48], num_blocks=[2, 1], interctc_blocks=[2], vocab_size=16, loss_prefix="c_ctc",
                                 att_params=[ATT("RelPos1dMultiHeadAttention"), ATT("RelPos1dMultiHeadAttention", causal=True)],
                                 conv_params={"class": "Conv1d", "params": {"padding": "causal", "kernel_size": 15}}, ff_ratio=4, drop_rate=0.1,
                                 mask=nnet.Mask(left_context=6, right_context=0), conv_stride=2)
    g = torch.Generator().manual_seed(99)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):              # running statistics that are not the identity
            m.running_mean.copy_(0.3 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    return net.eval()


@functools.lru_cache(maxsize=1)
def fixture():
    """(state dict on the host, inputs data[b][utterance] [T][32], oracle results per (slot, utterance): (y, ylen, logits, loglen)) -- computed once, never modified"""
    net = make_net()
    sd = {"m." + k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    data = [[torch.randn(T, D0, generator=g) for T in ut] for ut in UTTS]
    ref = []
    for ub in data:
        row = []
        for x in ub:
            with torch.no_grad():
                y, ylen, inter = O.conformer_interctc(sd, "m", x[None], torch.tensor([x.shape[0]]), [2, 1], [2], "c_ctc", [1, 1], False, {}, context=(6, 0, 0), causal_conv=True)
            row.append((y[0], int(ylen[0]), inter[KEY][0][0], int(inter[KEY][1][0])))
        ref.append(row)
    return sd, data, ref


def gpu_net(dtype):
    import avec_amd
    avec_amd.set_compute_dtype(dtype)
    return make_net().to("cuda").eval()


def streamed(net, Tc, capture=False, chunk_len="list", sync_free=False):
    """walk the schedule; -> per (slot, utterance) (y rows, sum of out_len, logits rows, sum of logit lengths), and the per-push raw outputs (cloned)"""
    _, data, _ = fixture()
    ses = net.stream(len(UTTS), Tc)
    if capture:
        ses.capture()
    got = [[[[], 0, [], 0] for _ in ut] for ut in UTTS]
    raw = []
    for pi, row in enumerate(SR.schedule(UTTS, Tc)):
        x = SR.chunk_of(data, row, Tc, 0.5).cuda()
        n = [r[2] for r in row]
        reset = [b for b, r in enumerate(row) if r[3]]
        cl = n if chunk_len == "list" else torch.tensor(n, dtype=torch.int64, device="cuda")
        if sync_free and pi > 0:
            torch.cuda.set_sync_debug_mode("error")
        try:
            y, ylen, inter = ses.push(x, cl, reset or None)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        lg, lglen = inter[KEY]
        raw.append((y.clone(), ylen.clone(), lg.clone(), lglen.clone()))
        yl, ll = ylen.tolist(), lglen.tolist()
        for b, (ui, _, nb, _) in enumerate(row):
            assert yl[b] == ll[b] == -(-nb // 2), (pi, b, yl, ll, nb)
            if ui is not None:
                acc = got[b][ui]
                acc[0].append(y[b, :yl[b]].float().cpu()), acc[2].append(lg[b, :ll[b]].float().cpu())
                acc[1] += yl[b]
                acc[3] += ll[b]
    return [[(torch.cat(a[0]), a[1], torch.cat(a[2]), a[3]) for a in gb] for gb in got], raw


def offline(net):
    """the offline GPU forward on the padded batches of first and second utterances -> per (slot, utterance) (y valid rows, logits valid rows)"""
    _, data, ref = fixture()
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
def test_stream_f32_matches_oracle(Tc):
    _, _, ref = fixture()
    net = gpu_net("f32")
    off = offline(net)
    got, _ = streamed(net, Tc)
    for b, ub in enumerate(ref):
        for ui, (y, ylen, lg, lglen) in enumerate(ub):
            gy, gyl, gl, gll = got[b][ui]
            ey, el = rel_err(gy, y), rel_err(gl, lg)
            print("Tc=%d slot %d utterance %d: streamed y %.3g logits %.3g | offline GPU y %.3g logits %.3g" % (Tc, b, ui, ey, el, rel_err(off[b][ui][0], y), rel_err(off[b][ui][1], lg)))
            assert gyl == ylen and gll == lglen and gy.shape == y.shape and gl.shape == lg.shape, (Tc, b, ui, gyl, ylen, gll, lglen)
            assert ey < 1e-3 and el < 1e-3, (Tc, b, ui, ey, el)


@pytest.mark.parametrize("Tc", [2, 4, 8, 40])
def test_stream_bf16_within_twice_the_offline_error(Tc):
    """measured on MI355X (max over slots and utterances): see DESIGN section 31"""
    _, _, ref = fixture()
    net = gpu_net("bf16")
    try:
        off = offline(net)
        got, _ = streamed(net, Tc)
    finally:
        import avec_amd
        avec_amd.set_compute_dtype("f32")
    bad = []
    for b, ub in enumerate(ref):
        for ui, (y, ylen, lg, lglen) in enumerate(ub):
            gy, gyl, gl, gll = got[b][ui]
            assert gyl == ylen and gll == lglen
            ey, el, oy, ol = rel_err(gy, y), rel_err(gl, lg), rel_err(off[b][ui][0], y), rel_err(off[b][ui][1], lg)
            print("bf16 Tc=%d slot %d utterance %d: streamed y %.3g logits %.3g | offline GPU y %.3g logits %.3g" % (Tc, b, ui, ey, el, oy, ol))
            if not (ey <= 2 * oy and el <= 2 * ol):
                bad.append((b, ui, ey, oy, el, ol))
    assert not bad, bad


def test_chunking_invariance_and_device_chunk_len():
    net = gpu_net("f32")
    a, _ = streamed(net, 2)
    b, _ = streamed(net, 8, chunk_len="tensor")
    for ga, gb in zip(a, b):
        for (ya, na, la, _), (yb, nb, lb, _) in zip(ga, gb):
            assert na == nb and rel_err(ya, yb) < 1e-3 and rel_err(la, lb) < 1e-3


def test_captured_pushes_equal_eager_pushes():
    net = gpu_net("f32")
    _, eager = streamed(net, 4)
    _, graph = streamed(net, 4, capture=True)
    assert len(eager) == len(graph) >= 3
    for pi, (e, g) in enumerate(zip(eager, graph)):
        for te, tg in zip(e, g):
            assert torch.equal(te, tg), pi


def test_pushes_do_not_synchronise_or_grow():
    net = gpu_net("f32")
    streamed(net, 4, sync_free=True)                                  # host-list chunk lengths and restarts under torch's sync debug mode
    ses = net.stream(3, 4)
    x = torch.randn(3, 4, D0, device="cuda")
    out = ses.push(x)
    del out
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(50):
            out = ses.push(x, [4, 4, 4], [i % 3] if i % 7 == 0 else None)
            del out
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == m0
    assert ses.pos.tolist() == [32, 4, 60]                            # restarts at i = 42 (slot 0), 49 (slot 1), 35 (slot 2): 8, 1 and 15 pushes of 4 frames since


def test_host_list_contract_and_gpu_refusals():
    net = gpu_net("f32")
    ses = net.stream(3, 4)
    x = torch.randn(3, 4, D0, device="cuda")
    ses.push(x, [4, 2, 4])
    with pytest.raises(RuntimeError, match="slot 1 ended with a short chunk"):
        ses.push(x, [4, 4, 4])
    ses.push(x, [4, 4, 4], [1])                                      # restarted: legal again
    with pytest.raises(ValueError, match="chunk"):
        ses.push(x[:, :2])
    with pytest.raises(RuntimeError, match="training mode"):
        net.train().stream(3, 4)
