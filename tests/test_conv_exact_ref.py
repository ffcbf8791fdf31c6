"""CPU: the integer references of tests/conv_exact_ref.py against torch.nn.functional.conv2d plus autograd in float64, check_exact() on every operand set that
tests/test_gpu_conv_exact.py uses (the GPU file's torch.equal is only meaningful while these preconditions hold), and the mismatch report."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_exact_ref as R

# (N, H, W, Cin, Cout, K, stride): non-square, stride 1 and 2, 3x3 and 1x1, odd-by-even at stride 2, one image
GEOMETRIES = [(2, 5, 7, 8, 16, 3, 1), (3, 7, 5, 8, 8, 3, 1), (2, 7, 12, 8, 16, 3, 2), (2, 12, 7, 16, 8, 3, 2), (1, 12, 7, 8, 8, 1, 2), (3, 4, 3, 8, 24, 1, 1), (1, 3, 3, 8, 8, 3, 2)]


@pytest.mark.parametrize("N,H,W,C,Co,K,s", GEOMETRIES)
def test_references_match_conv2d_autograd(N, H, W, C, Co, K, s):
    g = torch.Generator().manual_seed(N * 100 + H)
    x, w = R.activations(g, (N, H, W, C)), R.weights(g, (Co, K, K, C))
    OH, OW = R.out_size(H, s), R.out_size(W, s)
    dy = R.activations(g, (N, OH, OW, Co))
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=s, padding=(K - 1) // 2)
    assert tuple(y.shape[2:]) == (OH, OW)
    y.backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(R.conv_fwd(x, w, s), y.detach().permute(0, 2, 3, 1).reshape(-1, Co))
    assert torch.equal(R.conv_bwd_data(dy, R.backward_weights(w), H, W, s), xr.grad.permute(0, 2, 3, 1).reshape(-1, C))
    assert torch.equal(R.conv_wgrad(x, dy, K, s), wr.grad.permute(0, 2, 3, 1))
    v = R.conv_fwd(x, w, s)
    st = R.column_stats(v)
    assert torch.equal(st[0], v.sum(0)) and torch.equal(st[1], (v ** 2).sum(0))


def test_operand_generators_draw_the_stated_sets():
    g = torch.Generator().manual_seed(7)
    a, w, r = R.activations(g, (4000,), 1.0), R.weights(g, (4000,), 1.0), R.nonzero_ints(g, (4000,))
    assert sorted(set(a.tolist())) == [-2.0, -1.0, 0.0, 1.0, 2.0] and sorted(set(w.tolist())) == [-1.0, 0.0, 1.0] and sorted(set(r.tolist())) == [-2.0, -1.0, 1.0, 2.0]
    thin = R.activations(g, (20000,), 0.5)
    assert abs(float((thin != 0).double().mean()) - 0.4) < 0.02            # 4/5 non-zero values, half of them kept
    g2 = torch.Generator().manual_seed(7)
    assert torch.equal(R.activations(g2, (4000,), 1.0), a)                # seeded: the same operands on every machine


def test_mask_layout_and_epilogues():
    keep = torch.zeros(2, 16, dtype=torch.bool)
    keep[0, 0] = keep[0, 9] = keep[1, 7] = True
    m = R.pack_mask(keep)
    assert m.tolist() == [1, 2, 128, 0]                                   # bit e of byte k is element 8k + e
    assert torch.equal(R.unpack_mask(m, 2, 16), keep)
    acc, res = torch.full((2, 16), 3.0, dtype=R.F64), torch.full((2, 16), 2.0, dtype=R.F64)
    out = R.residual_masked(acc, res, m, 0.5)
    assert float(out[0, 0]) == 3.5 and float(out[0, 1]) == 1.5 and float(out[1, 7]) == 3.5
    # class-0 residual: only pixels with even row and even column get one
    N, H, W, C = 2, 3, 4, 8
    res0 = torch.arange(N * 2 * 2 * C, dtype=R.F64).view(-1, C) + 1
    out = R.residual_cls0(torch.zeros(N * H * W, C, dtype=R.F64), res0, N, H, W).view(N, H, W, C)
    assert torch.equal(out[:, ::2, ::2].reshape(-1, C), res0) and float(out[:, 1].abs().sum()) == 0 and float(out[:, :, 1::2].abs().sum()) == 0
    # BatchNorm-backward fusion: 0 and -0 block the gradient, with either mask source
    z = torch.tensor([[1.0, 0.0, -0.0, -1.0]], dtype=R.F64)
    assert R.relu_keep_from_activation(z).tolist() == [[True, False, False, False]]
    y = torch.tensor([[1.0, 1.0, -0.0, 2.0]], dtype=R.F64)
    keep = R.relu_keep_from_preactivation(y, torch.tensor([0.5, -0.5, 1.0, 0.5]), torch.tensor([0.0, 0.5, 0.0, -1.0]))
    assert keep.tolist() == [[True, False, False, False]]                # 0.5, exactly 0, -0, exactly 0
    v, st = R.bn_backward_fusion(torch.tensor([[4.0, 4.0, 4.0, 4.0]], dtype=R.F64), y, keep, torch.ones(1, 4, dtype=R.F64), 0.5)
    assert v.tolist() == [[3.0, 0.0, 0.0, 0.0]] and st.tolist() == [[3.0, 0.0, 0.0, 0.0], [3.0, 0.0, 0.0, 0.0]]


SETS = R.all_operand_sets()


def test_operand_set_ids_are_unique():
    ids = [i for i, _ in SETS]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("build", [b for _, b in SETS], ids=[i for i, _ in SETS])
def test_check_exact_holds_for_every_gpu_operand_set(build):
    fig = R.check_exact(build()["check"])
    assert fig["nonzero_min"] >= 0.9 and fig["bf16_max"] <= 256 and max(fig["sum_max"], fig["dw_max"], fig["f32_max"]) < 2 ** 24


def test_check_exact_refuses_what_is_not_exact():
    ok = torch.full((4, 8), 3.0, dtype=R.F64)
    R.check_exact({"bf16": [ok], "sums": [ok], "nonzero": [ok], "dw": [(ok, 0.5)], "f32": [ok]})
    with pytest.raises(AssertionError):
        R.check_exact({"bf16": [ok * 100]})                               # 300 > 256
    with pytest.raises(AssertionError):
        R.check_exact({"bf16": [ok + 126.25]})                            # 129.25 is no bf16 number
    with pytest.raises(AssertionError):
        R.check_exact({"sums": [torch.full((1 << 12, 1), 4096.0, dtype=R.F64)]})      # a column of 2^24
    with pytest.raises(AssertionError):
        R.check_exact({"sums": [torch.full((1 << 12, 1), 2048.5, dtype=R.F64)]})      # halves: 2^23 is the limit
    with pytest.raises(AssertionError):
        R.check_exact({"dw": [(torch.full((2, 2), float(1 << 24), dtype=R.F64), 0.5)]})
    with pytest.raises(AssertionError):
        R.check_exact({"nonzero": [torch.tensor([1.0, 0.0, 0.0, 1.0], dtype=R.F64)]})
    with pytest.raises(AssertionError):
        R.check_exact({"bf16": [ok]}, {"bf16_max": 512.0})                # limits only tighten


def _window_conv(x, w, swap):
    """3x3 / stride-1 forward the way a shifted-window kernel does it: pixels in one flat array, tap (kh, kw) reads the pixel (kh - 1) * W + (kw - 1) further on and a
    border test decides whether it counts.  swap: the row test compares with W instead of H -- the slip that square images cannot show"""
    N, H, W, C = x.shape
    flat = x.reshape(-1, C)
    P = flat.shape[0]
    p = torch.arange(P)
    col, row = p % W, (p // W) % H
    y = torch.zeros(P, w.shape[0], dtype=R.F64)
    for kh in range(3):
        for kw in range(3):
            rr, cc = row + kh - 1, col + kw - 1
            ok = (rr >= 0) & (rr < (W if swap else H)) & (cc >= 0) & (cc < W)
            src = (p + (kh - 1) * W + (kw - 1)).clamp(0, P - 1)
            y += (flat[src] * ok.unsqueeze(1)) @ w[:, kh, kw, :].t()
    return y


def test_swapped_height_and_width_show_only_on_non_square_images():
    """why the GPU file runs H < W and H > W everywhere: a border test that takes W for H is right on every square image and wrong on each of the non-square ones"""
    g = torch.Generator().manual_seed(11)
    w = R.weights(g, (8, 3, 3, 8), 1.0)
    for H, W, differs in [(8, 8, False), (5, 31, True), (31, 5, True), (7, 12, True), (12, 7, True)]:
        x = R.activations(g, (3, H, W, 8), 1.0)
        ref = R.conv_fwd(x, w)
        assert torch.equal(_window_conv(x, w, False), ref)
        msg = R.describe_mismatch(_window_conv(x, w, True), ref, (3, H, W, 8), R.CONV_NAMES)
        assert (msg is not None) == differs, (H, W, msg)
        if differs and H < W:      # the rows that wrongly count are the last of an image: they read the first row of the next one
            assert "(0, %d, " % (H - 1) in msg, msg


def test_planted_single_term_error_is_reported_with_its_coordinates():
    g = torch.Generator().manual_seed(3)
    N, H, W, C, Co = 3, 5, 7, 8, 16
    x, w = R.activations(g, (N, H, W, C), 1.0), R.weights(g, (Co, 3, 3, C), 1.0)
    ref = R.conv_fwd(x, w)
    assert R.describe_mismatch(ref.clone(), ref, (N, H, W, Co), R.CONV_NAMES) is None
    # drop ONE term: tap (0, 2) of input channel 5 at output pixel (image 2, row 0 -- where that tap reads the zero border -- is no error; row 3, column 6 is)
    n, oh, ow, co, ci = 2, 3, 5, 11, 5
    x[n, oh - 1, ow + 1, ci], w[co, 0, 2, ci] = 2.0, -1.0
    ref = R.conv_fwd(x, w)
    got = ref.clone().view(N, H, W, Co)
    got[n, oh, ow, co] -= x[n, oh - 1, ow + 1, ci] * w[co, 0, 2, ci]
    msg = R.describe_mismatch(got, ref, (N, H, W, Co), R.CONV_NAMES)
    want = float(ref.view(N, H, W, Co)[n, oh, ow, co])
    assert msg.startswith("1 of %d elements differ" % ref.numel()) and "(image, row, column, channel)" in msg
    assert "(2, 3, 5, 11): %r / %r" % (want, want + 2.0) in msg, msg
    with pytest.raises(AssertionError, match=r"\(2, 3, 5, 11\)"):
        R.assert_exact(got, ref, (N, H, W, Co), R.CONV_NAMES, "planted")
    # a NaN left in the output differs too, and a weight gradient reports (co, kh, kw, ci)
    dW = R.conv_wgrad(x, R.activations(g, (N, H, W, Co), 1.0))
    bad = dW.clone()
    bad[7, 2, 0, 3] = float("nan")
    msg = R.describe_mismatch(bad, dW, tuple(dW.shape), R.WGRAD_NAMES)
    assert "(co, kh, kw, ci)" in msg and "(7, 2, 0, 3): %r / nan" % float(dW[7, 2, 0, 3]) in msg, msg
