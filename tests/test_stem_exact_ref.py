"""CPU: the references of tests/stem_exact_ref.py against torch's own conv3d, max_pool2d and autograd in float64, the tie rule by hand, and the exactness conditions of
every operand set that tests/test_gpu_stem_exact.py uses (its torch.equal means something only while these hold)."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import stem_exact_ref as S

F64 = S.F64


def _tie_free(gen, shape):
    """a random permutation of distinct integers: no two candidates of any window are equal"""
    n = 1
    for s in shape:
        n *= s
    return (torch.randperm(n, generator=gen).to(F64) - n // 2).view(shape)


@pytest.mark.parametrize("shape", [(1, 1, 7, 9), (2, 3, 8, 11), (1, 6, 9, 16)])
def test_conv_and_im2col_match_conv3d(shape):
    gen = S._gen("conv %r" % (shape,))
    B, T, H, W = shape
    video, w, k = S.ints(gen, shape, 2), S.stem_weights(), S.channel_constants()
    z, stats = S.conv(video, w, k["bias"])
    ref = Fn.conv3d(video.view(B, 1, T, H, W), w.view(64, 1, 5, 7, 7), k["bias"], stride=(1, 2, 2), padding=(2, 3, 3))
    OH, OW = S.out_size(H), S.out_size(W)
    assert tuple(ref.shape) == (B, 64, T, OH, OW)
    ref = ref.permute(0, 2, 3, 4, 1).reshape(-1, 64)
    assert torch.equal(z, ref) and torch.equal(stats[0], ref.sum(0)) and torch.equal(stats[1], (ref * ref).sum(0))
    A = S.im2col(video, 256)
    assert A.shape == (B * T * OH * OW, 256) and float(A[:, 245:].abs().sum()) == 0 and torch.equal(A[:, :245] @ w.t() + k["bias"], z)
    # the one-hot channels are shifted copies of the video: channel 2 (centre tap, +1) is the video at the even pixels
    assert torch.equal(z[:, 2].view(B, T, OH, OW) - k["bias"][2], video[:, :, ::2, ::2])


def test_weights_cover_every_tap_and_stay_bf16_integers():
    w = S.stem_weights()
    assert bool((w != 0).any(0).all()) and int((w != 0).sum(1).max()) <= S.TAP_CAP and bool(((w[:8] != 0).sum(1) == 1).all())
    assert 2 * S.TAP_CAP + 32 < 256
    w8 = S.pack_w8(w, True)
    assert float(w8[:, :, 0].abs().sum()) == 0 and float(w8[:, 35].abs().sum()) == 0 and torch.equal(w8[:, :35, 1:].reshape(64, 245), w)
    w8 = S.pack_w8(w, False)
    assert float(w8[:, :, 7].abs().sum()) == 0 and float(w8[:, 35].abs().sum()) == 0 and torch.equal(w8[:, :35, :7].reshape(64, 245), w)


@pytest.mark.parametrize("F,OH,OW", [(2, 5, 7), (1, 4, 6), (3, 7, 4)])
def test_pool_references_match_max_pool2d_on_tie_free_inputs(F, OH, OW):
    gen = S._gen("pool %d %d %d" % (F, OH, OW))
    C = 8
    z = _tie_free(gen, (F * OH * OW, C))
    k = S.channel_constants(C)
    PH, PW = S.out_size(OH), S.out_size(OW)

    def torch_pool(v):      # -> values, (h, w) of the winner
        val, ind = Fn.max_pool2d(v.view(F, OH, OW, C).permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
        return val.permute(0, 2, 3, 1), ind.permute(0, 2, 3, 1)

    def slot_to_flat(slot):
        ph, pw = torch.arange(PH).view(1, PH, 1, 1), torch.arange(PW).view(1, 1, PW, 1)
        return (2 * ph + slot // 3 - 1) * OW + 2 * pw + slot % 3 - 1

    s = torch.where(k["gamma"] < 0, -1.0, 1.0).to(F64)
    zp, idx = S.pool_raw(z, k["gamma"], F, OH, OW)
    val, ind = torch_pool(z * s)
    assert torch.equal(zp, val * s) and torch.equal(slot_to_flat(idx), ind)
    out, idx, ymax = S.pool_act(z, k["scale"], k["shift"], F, OH, OW)
    val, ind = torch_pool((z * k["scale"] + k["shift"]).clamp_min(0))
    assert torch.equal(out, val)
    live = out > 0
    assert torch.equal(idx == 255, ~live) and torch.equal(slot_to_flat(idx)[live], ind[live])
    zz = z.view(F, OH * OW, C)
    want = torch.gather(zz, 1, ind.reshape(F, -1, C)).view(F, PH, PW, C)
    assert torch.equal(ymax[live], want[live]) and float(ymax[~live].abs().sum()) == 0
    # route: autograd of max_pool2d sends each pooled gradient to its winner
    dp = S.ints(gen, (F, PH, PW, C), 3)
    zr = (z * s).clone().requires_grad_(True)
    Fn.max_pool2d(zr.view(F, OH, OW, C).permute(0, 3, 1, 2), 3, 2, 1).backward(dp.permute(0, 3, 1, 2))
    zp, idx = S.pool_raw(z, k["gamma"], F, OH, OW)
    assert torch.equal(S.route(dp, idx, OH, OW), zr.grad)


def test_tie_rule_by_hand():
    """a constant 3 x 3 frame: every candidate of every window ties.  The first one INSIDE the frame in scan order wins: window (0, 0) has its kh = 0 row and kw = 0
    column outside, so slot 4 (the centre); window (0, 1) sees columns 1, 2, outside: slot 3; (1, 0): slot 1; (1, 1): slot 0.  Negative gamma (min pool): the same."""
    z = torch.full((9, 2), 5.0, dtype=F64)
    zp, idx = S.pool_raw(z, torch.tensor([2.0, -2.0], dtype=F64), 1, 3, 3)
    assert zp.shape == (1, 2, 2, 2) and bool((zp == 5).all())
    assert idx[0, :, :, 0].tolist() == [[4, 3], [1, 0]] and idx[0, :, :, 1].tolist() == [[4, 3], [1, 0]]
    out, idx, ymax = S.pool_act(z, torch.tensor([2.0, 2.0], dtype=F64), torch.tensor([-4.0, -10.0], dtype=F64), 1, 3, 3)
    assert idx[0, :, :, 0].tolist() == [[4, 3], [1, 0]] and bool((out[..., 0] == 6).all()) and bool((ymax[..., 0] == 5).all())
    assert bool((idx[..., 1] == 255).all()) and float(out[..., 1].abs().sum()) == 0 and float(ymax[..., 1].abs().sum()) == 0      # 2 * 5 - 10 = 0 is not positive
    # one larger value later in the scan beats the earlier ties; an equal one does not
    z[8, 0] = 6.0                                                  # pixel (2, 2): the centre (slot 4) of window (1, 1) alone
    assert S.pool_raw(z, torch.tensor([2.0, -2.0], dtype=F64), 1, 3, 3)[1][0, :, :, 0].tolist() == [[4, 3], [1, 4]]
    # routing of ties: pixel (1, 1) is named by windows (0,1), (1,0) under their slots 3 and 1 only when those won
    d = torch.ones(1, 2, 2, 1, dtype=F64)
    dr = S.route(d, torch.tensor([[[[4], [3]], [[1], [0]]]]), 3, 3).view(3, 3)
    assert dr.tolist() == [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]]


def test_backward_chain_matches_autograd_on_a_tie_free_case():
    """reduce -> route -> dz -> wgrad against autograd of conv3d + batch-statistics BatchNorm + ReLU + max_pool2d in float64 (random real weights: no ties)"""
    gen = S._gen("autograd")
    B, T, H, W = 1, 2, 9, 12
    video = torch.randn(B, T, H, W, generator=gen, dtype=F64)
    w = torch.randn(64, 245, generator=gen, dtype=F64).requires_grad_(True)
    bias = torch.randn(64, generator=gen, dtype=F64)
    gamma = torch.randn(64, generator=gen, dtype=F64).requires_grad_(True)
    beta = torch.randn(64, generator=gen, dtype=F64).requires_grad_(True)
    F, OH, OW = B * T, S.out_size(H), S.out_size(W)
    PH, PW = S.out_size(OH), S.out_size(OW)
    A = S.im2col(video)
    z = A @ w.t() + bias
    mean, var = z.mean(0), z.var(0, unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    a = torch.relu((z - mean) * rstd * gamma + beta)
    out = Fn.max_pool2d(a.view(F, OH, OW, 64).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    dp = torch.randn(F, PH, PW, 64, generator=gen, dtype=F64)
    (out * dp).sum().backward()
    with torch.no_grad():
        k = dict(gamma=gamma, rstd=rstd, mean=mean, scale=gamma * rstd, shift=beta - mean * gamma * rstd)
        zp, idx = S.pool_raw(z, gamma, F, OH, OW)
        d, dstats, _ = S.reduce(dp, zp, k)
        exact, _ = S.bn_backward(S.route(d, idx, OH, OW), z, k, dstats, float(z.shape[0]))
        dW = S.wgrad(exact, A)
    assert torch.allclose(dW, w.grad, rtol=1e-9, atol=1e-9 * float(w.grad.abs().max()))
    assert torch.allclose(dstats[1], gamma.grad, rtol=1e-9, atol=1e-9) and torch.allclose(dstats[0], beta.grad, rtol=1e-9, atol=1e-9)      # dgamma += dstats1, dbeta += dstats0


def test_bf16_rounding_of_dz_is_round_to_nearest_even_once():
    k = {n: torch.tensor([v], dtype=F64) for n, v in (("gamma", 2.0), ("rstd", 4.0), ("mean", 0.0))}
    # 8 * (dr - 0 - z * 4 * 0.25) with dr = 0: -8 z.  z = 32.125 -> -257 (9 bits: a tie between -256 and -258, even mantissa wins: -256); z = 32.375 -> -259 -> -260
    z = torch.tensor([[32.125], [32.375]], dtype=F64)
    exact, dz = S.bn_backward(torch.zeros(2, 1, dtype=F64), z, k, torch.tensor([[0.0], [0.25 * 8]], dtype=F64), 8.0)
    assert exact.view(-1).tolist() == [-257.0, -259.0] and dz.view(-1).tolist() == [-256.0, -260.0]


def test_column_grain_and_units():
    t = torch.tensor([[0.5, 3.0, 0.0], [1.5, 6.0, 0.0]], dtype=F64)
    assert S.col_grain(t).tolist() == [0.5, 1.0, 2.0 ** 40]       # (3 and 6 share no power of two above 1; a column of zeros divides by anything)
    assert S.units(t[:, :2]) == 9.0
    with pytest.raises(AssertionError):
        S.check_stem_exact({"colsums": [(torch.full((1 << 12, 1), 2048.5, dtype=F64), torch.zeros(1))]})      # halves: 2^23 is the limit
    with pytest.raises(AssertionError):
        S.check_stem_exact({"rounded": [torch.tensor([1.0 + 2.0 ** -30], dtype=F64)]})
    with pytest.raises(AssertionError):
        S.check_stem_exact({"bf16_wide": [torch.tensor([257.0], dtype=F64)]})


SETS = S.all_operand_sets()


def test_operand_set_ids_are_unique():
    ids = [i for i, _ in SETS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("check", [c for _, c in SETS], ids=[i for i, _ in SETS])
def test_exactness_conditions_hold_for_every_gpu_operand_set(check):
    fig = check()
    assert fig["bf16_max"] <= 256 and max(fig["f32_max"], fig.get("col_units", 0.0), fig.get("dw_units", 0.0)) < 2 ** 24


def test_stem3p_cases_tie_often_and_reach_the_masks():
    """what the integer frames are for: most windows hold several equal candidates, both pool directions occur, and the ReLU mask is exactly zero at many winners"""
    o = S.s3p_operands("h37_two_bands")
    z = o["z"].view(o["F"], o["OH"], o["OW"], 64)
    centre = z[:, 0:2 * o["PH"] - 1:2, 0:2 * o["PW"] - 1:2][:, :o["PH"], :o["PW"]]
    tied = (o["zp"] == centre) & (o["idx"] != 4)                  # the centre equals the winner, yet an earlier candidate won
    assert float(tied.double().mean()) > 0.02
    assert sorted(set(o["idx"].reshape(-1).tolist())) == list(range(9))
    pre = o["zp"] * o["k"]["scale"] + o["k"]["shift"]
    assert float((pre == 0).double().mean()) > 0.01 and 0.2 < float((pre > 0).double().mean()) < 0.8
    assert int((o["k"]["gamma"] < 0).sum()) == 13
