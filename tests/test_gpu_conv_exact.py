"""GPU (-m gpu): the ResNet convolution kernels -- forward, backward-data and weight gradient of the 3x3, stride-2 and 1x1 layers (csrc/conv3x3.hip, csrc/wgrad_pairs.hip,
csrc/conv_s2.hip, the conv modes of avec_gemm_nt / avec_gemm_tn) -- reproduce an integer reference EXACTLY, at every element.

tests/conv_exact_ref.py holds the operands (activations and gradients in {-2 .. 2}, weights in {-1, 0, 1}), the plain float64 references and check_exact(), which
asserts on the reference alone that a correct kernel has no choice: every product and every fp32 partial sum is an exactly representable number below 2^24 whatever the
order of summation (so the fp32 atomics of the weight gradients and of the BatchNorm statistics are deterministic too), and every bf16 result is a bf16 number.  Every
comparison below is therefore torch.equal; a failure names the differing elements as (image, row, column, channel) or (co, kh, kw, ci) with expected and got values.
Outputs are NaN-filled with a guard row behind them.  Every case asserts the kernel instance it means to reach (avec_last_kernel), so a retuned dispatch cannot
silently empty the coverage: move the case to a shape that reaches the instance again.

Geometry: every family here accepts non-square images (none rejects them), so each runs H < W and H > W; stride 2 runs odd-by-even sizes (7x12, 12x7), OW = 15 and
OW = 2 (the limits of the stride-2 kernel; OW = 16 falls to the parity-class order of the LDS-DMA kernel), the shifted-window kernel W = 31 (W = 32 falls through);
image counts leave the last tile ragged, 128-row tiles straddle image boundaries (8x8 images), and every family runs one image alone.

Not here (see the issue this file answers): the stems (tests/test_gpu_stem_exact.py has them), the fp8 products, the env-forced variants (AVEC_NO_*, AVEC_SHIFT_BM, AVEC_NT_RB: read once per process).
The BatchNorm-backward fusion has no register-direct form: epi_tr_ok() and the stride-2 kernel decline a launch that carries bnb_y, so it is tested in the staged
epilogue from every kernel that reaches it.
"""
import ctypes

import pytest
import torch

from tests import conv_exact_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
FWD, BWD = 1, 2
NAN = float("nan")
STAT_NAMES = ("sum | second moment", "channel")


def dev():
    return torch.device("cuda:0")


def _lib():
    from avec_amd import lib as L, ops, runtime as rt
    return L, ops, rt


def up(t, dtype, off=0):
    """the float64 tensor on the device as `dtype` (exact: check_exact has seen the values), `off` elements behind an aligned address, 64 spare elements behind it"""
    n = t.numel()
    buf = torch.zeros(n + off + 64, dtype=dtype, device=dev())
    buf[off:off + n].copy_(t.reshape(-1).to(dtype))
    return buf[off:off + n]


def nan_rows(rows, cols, dtype, init=None):
    """[rows + 1][cols] on the device: NaN (or `init` in the first `rows` rows), the last row is the guard"""
    buf = torch.full((rows + 1, cols), NAN, dtype=dtype, device=dev())
    if init is not None:
        buf[:rows] = init
    return buf


def assert_guard(buf, what):
    assert bool(torch.isnan(buf[-1]).all()), "%s: the guard row behind the output was written" % what


def last_kernel():
    L, _, _ = _lib()
    return L.lib.raw("avec_last_kernel")().decode()


def check_stats(st, ref, N, what):
    """the 64 replicas of [sum | second moment] summed in float64 (each replica is exact on its own)"""
    R.assert_exact(st.view(64, 2, N).double().sum(0).cpu(), ref, (2, N), STAT_NAMES, what + ": statistics")


# ---- 1, 2, 5: avec_gemm_nt conv modes ------------------------------------------------------------------------------------------------------------
def launch_nt(c, o):
    """one avec_gemm_nt call on the operands `o` of case `c`: the NaN-filled output with its guard row, the replicated statistics (or None), the kernel reached"""
    L, ops, rt = _lib()
    f32 = c["dtype"] == "f32"
    adt = torch.float32 if f32 else torch.bfloat16
    M, N, K = o["M"], o["N"], o["K"]
    keep = [up(o["a"], adt), up(o["w"], adt)]
    out = nan_rows(M, N, torch.float32 if (f32 or c["out_f32"]) else torch.bfloat16)
    ep = L.Epilogue()
    ep.out, ep.ldo, ep.out_f32, ep.alpha = out.data_ptr(), N, int(c["out_f32"]), c["alpha"]
    st = None
    if "bias" in o:
        keep.append(up(o["bias"], torch.float32)); ep.bias = keep[-1].data_ptr()
    if "stats" in o:
        st = torch.zeros(64 * 2 * N, dtype=torch.float32, device=dev()); ep.stats = st.data_ptr()
    if "res" in o:
        keep.append(up(o["res"], adt if c["res"] == "bf16" else torch.float32))
        ep.res, ep.ldres, ep.res_act, ep.res_cls0 = keep[-1].data_ptr(), N, int(c["res"] == "bf16"), int(c["res_cls0"])
    if "mask" in o:
        keep.append(up(o["mask"], torch.uint8)); ep.res_mask = keep[-1].data_ptr()
    if "y" in o:
        keep.append(up(o["y"], adt)); ep.bnb_y, ep.ldby = keep[-1].data_ptr(), N
        if "z" in o:
            keep.append(up(o["z"], adt)); ep.dact_z, ep.ldz, ep.dact, ep.bnb_mask = keep[-1].data_ptr(), N, 2, 0
        else:
            keep.append(up(o["ss"], torch.float32)); ep.bnb_ss, ep.bnb_mask = keep[-1].data_ptr(), 1
    rows = ops.rows_conv(*o["rows"])
    L.lib.gemm_nt(F32 if f32 else BF16, keep[0].data_ptr(), ctypes.byref(rows), FWD if c["mode"] == "fwd" else BWD, 0, keep[1].data_ptr(), K, M, N, K, ctypes.byref(ep), rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    return out, st, name


def run_nt(c):
    o = R.nt_operands(c)
    R.check_exact(o["check"])
    out, st, name = launch_nt(c, o)
    assert name == c["kernel"], "%s reached %s, not %s" % (c["id"], name, c["kernel"])
    R.assert_exact(out[:-1].cpu(), o["out"], o["shape"], R.CONV_NAMES, c["id"])
    assert_guard(out, c["id"])
    if st is not None:
        check_stats(st, o["stats"], o["N"], c["id"])


@pytest.mark.parametrize("c", R.NT_CASES, ids=[c["id"] for c in R.NT_CASES])
def test_conv_nt_exact(c):
    """forward / backward-data of avec_gemm_nt's conv modes with their epilogues (statistics of the fp32 results, alpha, bf16 / fp32 / bit-masked / class-0 residual,
    bias, fp32 output): bit-equal to the integer reference"""
    run_nt(c)


@pytest.mark.parametrize("c", R.BNB_CASES, ids=[c["id"] for c in R.BNB_CASES])
def test_conv_bn_backward_fusion_exact(c):
    """the BatchNorm-backward fusion of the backward-data epilogue, v = alpha * acc + res; v = mask ? v : 0; stats += (sum v, sum v * y): both mask sources (dact = 2
    with a saved activation holding planted +0 / -0; bnb_mask = 1 with scale * y + shift in halves, exactly zero at many elements -- `> 0`, not `>= 0`), the masked
    gradient and both sums bit-equal"""
    run_nt(c)


def test_one_altered_weight_is_found_at_its_pixels():
    """negative control on the unmodified kernel: ONE weight entry (co 5, tap (0, 2), ci 7) raised by 1 on the device only.  The comparison with the unaltered reference
    must fail, at output channel 5 alone and exactly at the pixels whose upper-right neighbour holds a non-zero x[.][7] -- none of them in the first row or the last
    column of an image, where that tap reads the zero border -- and the result must equal the reference of the altered weights"""
    c = R.NT_CASES[0]
    assert c["id"] == "shift_128x64_fwd_stats"
    o = R.nt_operands(c)
    w4 = o["w"].view(c["Cn"], 3, 3, c["Cs"]).clone()
    w4[5, 0, 2, 7] += 1
    out, _, _ = launch_nt(c, dict(o, w=w4.reshape(c["Cn"], -1)))
    got = out[:-1].cpu().double()
    msg = R.describe_mismatch(got, o["out"], o["shape"], R.CONV_NAMES, first=1 << 20)
    assert msg is not None
    x = o["a"]
    hit = torch.zeros(o["shape"][:3], dtype=torch.bool)
    hit[:, 1:, :-1] = x[:, :-1, 1:, 7] != 0
    want = sorted((n, r, q, 5) for n, r, q in hit.nonzero().tolist())
    found = sorted(tuple(int(t) for t in line.split("):")[0].strip(" (").split(", ")) for line in msg.splitlines()[1:])
    assert found == want and len(want) > 100
    assert torch.equal(got, R.conv_fwd(x, w4))


# ---- 3: stage-1 slab kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SLAB_CASES, ids=[c[0] for c in R.SLAB_CASES])
def test_slab_conv_exact(case):
    """avec_conv3x3_c64 (forward + statistics, flip = 1 + residual) and avec_conv3x3_c64_res_masked; more than 256 images make a workgroup loop over several"""
    L, _, rt = _lib()
    cid, imgs, H, W, flip, what = case
    assert L.lib.raw("avec_conv3x3_c64_supported")(H, W, 64, 64, 3, 3, 1)
    o = R.slab_operands(case)
    R.check_exact(o["check"])
    bf = torch.bfloat16
    x, w = up(o["a"], bf), up(o["w"], bf)
    M = imgs * H * W
    out = nan_rows(M, 64, bf)
    st = torch.zeros(64 * 128, dtype=torch.float32, device=dev()) if what == "stats" else None
    res = up(o["res"], bf) if "res" in o else None
    if what == "masked":
        mask = up(o["mask"], torch.uint8)
        L.lib.conv3x3_c64_res_masked(x.data_ptr(), w.data_ptr(), out.data_ptr(), res.data_ptr(), mask.data_ptr(), imgs, H, W, flip, rt.stream())
    else:
        L.lib.conv3x3_c64(x.data_ptr(), w.data_ptr(), out.data_ptr(), None if res is None else res.data_ptr(), None if st is None else st.data_ptr(), imgs, H, W, flip, rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == ("conv3x3_c64_kernel<true,false>" if what == "stats" else "conv3x3_c64_res_kernel" if res is not None else "conv3x3_c64_kernel<false,false>"), name
    R.assert_exact(out[:M].cpu(), o["out"], o["shape"], R.CONV_NAMES, cid)
    assert_guard(out, cid)
    if st is not None:
        check_stats(st, o["stats"], 64, cid)


# ---- 4: weight gradients -----------------------------------------------------------------------------------------------------------------------
def _wg_buffers(c, o, dtype=torch.bfloat16, off_p=0):
    Co, J = c["Co"], c["K"] * c["K"] * c["C"]
    return up(o["x"], dtype), up(o["dy"], dtype, off_p), nan_rows(Co, J, torch.float32, c["init"])


def _wg_check(c, o, dw):
    R.assert_exact(dw[:-1].cpu(), o["out"], o["shape"], R.WGRAD_NAMES, c["id"])
    assert_guard(dw, c["id"])


def _wg_items(L, cases):
    items, held = (L.WgradItem * len(cases))(), []
    for k, c in enumerate(cases):
        o = R.wgrad_operands(c)
        R.check_exact(o["check"])
        x, dy, dw = _wg_buffers(c, o)
        held.append((c, o, x, dy, dw))
        t = items[k]
        t.x, t.dy, t.dw, t.images, t.C, t.H, t.W = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), c["imgs"], c["C"], c["H"], c["W"]
    return items, held


@pytest.mark.parametrize("c", R.WG64_CASES, ids=[c["id"] for c in R.WG64_CASES])
def test_wgrad3x3_c64_exact(c):
    """avec_wgrad3x3_c64 adds the exact weight gradient to a non-zero dW"""
    L, _, rt = _lib()
    o = R.wgrad_operands(c)
    R.check_exact(o["check"])
    x, dy, dw = _wg_buffers(c, o)
    L.lib.wgrad3x3_c64(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), c["imgs"], c["H"], c["W"], rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == "wgrad3x3_c64_grouped_kernel", name
    _wg_check(c, o, dw)


def test_wgrad3x3_c64_grouped_exact():
    """one grouped launch over four 64-channel layers of different geometry and image count"""
    L, _, rt = _lib()
    items, held = _wg_items(L, R.WG64_GROUP)
    L.lib.wgrad3x3_c64_grouped(items, len(held), rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == "wgrad3x3_c64_grouped_kernel", name
    for c, o, _, _, dw in held:
        _wg_check(c, o, dw)


@pytest.mark.parametrize("c,kernel", R.WG128_CASES, ids=[c["id"] for c, _ in R.WG128_CASES])
def test_wgrad3x3_c128_exact(c, kernel):
    """avec_wgrad3x3_c128 on the pair-kernel geometries (11x11, 6x6, 3x3) and on slab-kernel ones (5x7, 7x5, 8x8, 3x4)"""
    L, _, rt = _lib()
    assert L.lib.raw("avec_wgrad3x3_c128_supported")(c["H"], c["W"], c["C"], c["C"], 3, 3, 1)
    o = R.wgrad_operands(c)
    R.check_exact(o["check"])
    x, dy, dw = _wg_buffers(c, o)
    L.lib.wgrad3x3_c128(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), c["imgs"], c["C"], c["H"], c["W"], rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == kernel, name
    _wg_check(c, o, dw)


def test_one_altered_activation_is_found_in_the_weight_gradient():
    """negative control on the unmodified pair kernel: ONE element of x (image 3, pixel (0, 10), channel 77) raised by 1 on the device only.  The unaltered reference
    must differ, in input channel 77 alone and at the four taps that reach the top-right corner pixel, and the result must equal the reference of the altered x"""
    L, _, rt = _lib()
    c, kernel = R.WG128_CASES[0]
    assert c["id"] == "wg128_11x11"
    o = R.wgrad_operands(c)
    x2 = o["x"].clone()
    x2[3, 0, 10, 77] += 1
    x, dy, dw = _wg_buffers(c, dict(o, x=x2))
    L.lib.wgrad3x3_c128(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), c["imgs"], c["C"], c["H"], c["W"], rt.stream())
    assert last_kernel() == kernel
    torch.cuda.synchronize()
    got = dw[:-1].cpu().double().view(o["shape"])
    bad = (got != o["out"]).nonzero()
    assert bad.numel() > 0 and set(bad[:, 3].tolist()) == {77} and set(map(tuple, bad[:, 1:3].tolist())) <= {(0, 1), (0, 2), (1, 1), (1, 2)}
    assert torch.equal(got, R.conv_wgrad(x2, o["dy"]) + c["init"])


def test_wgrad3x3_c128_grouped_mixed_exact():
    """one grouped call whose items go to both kernels (the pair kernel first, then the slab kernel for the rest)"""
    L, _, rt = _lib()
    items, held = _wg_items(L, R.WG128_GROUP)
    L.lib.wgrad3x3_c128_grouped(items, len(held), rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == R.WIDE, name
    for c, o, _, _, dw in held:
        _wg_check(c, o, dw)


@pytest.mark.parametrize("c,kernel,off_p,colsum", R.TN_CASES, ids=[t[0]["id"] for t in R.TN_CASES])
def test_gemm_tn_conv_exact(c, kernel, off_p, colsum):
    """avec_gemm_tn / avec_gemm_tn_bias with conv-gathered rows (3x3 stride 1 and 2, 1x1 stride 2): the transposed-read kernel, the generic one (P four bytes behind an
    aligned address) and the fp32 one; the column sums of P (bias gradient) fused and as the separate pass"""
    L, ops, rt = _lib()
    o = R.wgrad_operands(c)
    R.check_exact(o["check"])
    f32 = c["dtype"] == "f32"
    x, dy, dw = _wg_buffers(c, o, torch.float32 if f32 else torch.bfloat16, off_p)
    Co, J = c["Co"], c["K"] * c["K"] * c["C"]
    M = dy.numel() // Co
    rows = ops.rows_conv(*o["rows"])
    cs = nan_rows(1, Co, torch.float32, c["init"]) if colsum else None
    if colsum:
        L.lib.gemm_tn_bias(F32 if f32 else BF16, dy.data_ptr(), Co, x.data_ptr(), ctypes.byref(rows), FWD, 0, dw.data_ptr(), J, cs.data_ptr(), M, Co, J, rt.stream())
    else:
        L.lib.gemm_tn(F32 if f32 else BF16, dy.data_ptr(), Co, x.data_ptr(), ctypes.byref(rows), FWD, 0, dw.data_ptr(), J, M, Co, J, rt.stream())
    name = last_kernel()
    torch.cuda.synchronize()
    assert name == kernel, name
    _wg_check(c, o, dw)
    if colsum:
        R.assert_exact(cs[0].cpu(), o["colsum"], (Co,), ("co",), c["id"] + ": column sums")
        assert_guard(cs, c["id"])
