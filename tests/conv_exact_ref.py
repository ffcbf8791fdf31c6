"""Integer operands and plain references for the ResNet convolution family (3x3 / stride 1 and 2, 1x1), NHWC, in the layouts of the kernels.

Why integers: with activations and gradients in {-2 .. 2} and weights in {-1, 0, 1} every bf16 (or fp32) product is an exact small integer, every fp32 partial sum an
integer below 2^24 -- exact whatever the order of summation, so the kernels that finish with fp32 atomics (weight gradients, BatchNorm statistics) are deterministic --
and a result of magnitude <= 256 survives the bf16 store.  A kernel then has to reproduce the reference below at EVERY element, bit for bit: a dropped, doubled, misplaced
or stale term is a non-zero integer difference.

Everything here is torch on the CPU in float64 (exact for these integers; int64 matmul has no BLAS) and calls no project code.  Layouts:
  x   [N][H][W][Cin]          dy  [N][OH][OW][Cout]      (rows m = (n * OH + oh) * OW + ow of the 2-D views)
  w   [Cout][KH][KW][Cin]     forward weights
  wb  [Cin][KH][KW][Cout]     backward-data weights: wb[ci][kh][kw][co] = w[co][kh][kw][ci] (taps NOT flipped: the kernels turn the window)
  dW  [Cout][KH][KW][Cin]
"same" zero padding: pad = (K - 1) / 2, OH = (H - 1) / stride + 1.
"""
import zlib

import torch

F64 = torch.float64
TWO24 = float(1 << 24)
# the preconditions check_exact() enforces; a caller may pass tighter ones, never looser
LIMITS = {"bf16_max": 256.0, "sum_max": TWO24, "nonzero_min": 0.90}


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def draw_ints(gen, shape, amax, density=1.0):
    """integers uniform in {-amax .. amax}, each kept with probability `density` (else 0), float64"""
    v = torch.randint(-amax, amax + 1, tuple(shape), generator=gen)
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=gen) < density)
    return v.to(F64)


def activations(gen, shape, density=0.5):
    """activations / gradients: {-2 .. 2}"""
    return draw_ints(gen, shape, 2, density)


def weights(gen, shape, density=0.5):
    """weights: {-1, 0, 1}"""
    return draw_ints(gen, shape, 1, density)


def out_size(H, stride):
    return (H - 1) // stride + 1


def backward_weights(w):
    """[Cout][KH][KW][Cin] -> [Cin][KH][KW][Cout]"""
    return w.permute(3, 1, 2, 0).contiguous()


# ---- the three products --------------------------------------------------------------------------------------------------------------------
def _taps(KH, KW):
    return [(kh, kw) for kh in range(KH) for kw in range(KW)]


def _window(t, kh, kw, OH, OW, stride):
    """the pixels of a zero-bordered tensor that tap (kh, kw) pairs with the OH x OW outputs"""
    return t[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride]


def _bordered(N, H, W, C, pad, stride):
    return torch.zeros(N, H + 2 * pad + stride, W + 2 * pad + stride, C, dtype=F64)


def conv_fwd(x, w, stride=1):
    """y[m][co] = sum_{kh, kw, ci} x[n][oh * stride - pad + kh][ow * stride - pad + kw][ci] * w[co][kh][kw][ci]   ->  [N * OH * OW][Cout]"""
    N, H, W, C = x.shape
    Co, KH, KW, Ci = w.shape
    assert Ci == C and KH == KW
    pad, OH, OW = (KH - 1) // 2, out_size(H, stride), out_size(W, stride)
    xp = _bordered(N, H, W, C, pad, stride)
    xp[:, pad:pad + H, pad:pad + W] = x
    y = torch.zeros(N * OH * OW, Co, dtype=F64)
    for kh, kw in _taps(KH, KW):
        y += _window(xp, kh, kw, OH, OW, stride).reshape(-1, C) @ w[:, kh, kw, :].t()
    return y


def conv_bwd_data(dy, wb, H, W, stride=1):
    """dx[m][ci] = sum over the outputs (oh, ow) and taps with oh * stride - pad + kh = ih (same for columns) of dy[n][oh][ow][co] * wb[ci][kh][kw][co]
    -> [N * H * W][Cin]"""
    N, OH, OW, Co = dy.shape
    Ci, KH, KW, Co2 = wb.shape
    assert Co2 == Co and KH == KW and OH == out_size(H, stride) and OW == out_size(W, stride)
    pad = (KH - 1) // 2
    dxp = _bordered(N, H, W, Ci, pad, stride)
    flat = dy.reshape(-1, Co)
    for kh, kw in _taps(KH, KW):
        _window(dxp, kh, kw, OH, OW, stride).add_((flat @ wb[:, kh, kw, :].t()).view(N, OH, OW, Ci))
    return dxp[:, pad:pad + H, pad:pad + W].reshape(-1, Ci).clone()


def conv_wgrad(x, dy, K=3, stride=1):
    """dW[co][kh][kw][ci] = sum_m dy[m][co] * x[n][oh * stride - pad + kh][ow * stride - pad + kw][ci]"""
    N, H, W, C = x.shape
    _, OH, OW, Co = dy.shape
    assert OH == out_size(H, stride) and OW == out_size(W, stride)
    pad = (K - 1) // 2
    xp = _bordered(N, H, W, C, pad, stride)
    xp[:, pad:pad + H, pad:pad + W] = x
    dW = torch.zeros(Co, K, K, C, dtype=F64)
    flat = dy.reshape(-1, Co)
    for kh, kw in _taps(K, K):
        dW[:, kh, kw, :] = flat.t() @ _window(xp, kh, kw, OH, OW, stride).reshape(-1, C)
    return dW


def column_stats(v, y=None):
    """[2][C]: (sum v, sum v^2) per column, or (sum v, sum v * y) with y"""
    return torch.stack([v.sum(0), (v * (v if y is None else y)).sum(0)])


# ---- epilogues -----------------------------------------------------------------------------------------------------------------------------
def pack_mask(keep):
    """bool [M][C] (C % 8 == 0) -> the bytes avec_bn_apply_fwd_mask writes (include/avec_hip.h): byte k holds elements 8k .. 8k + 7 of the row-major matrix, bit e is
    element 8k + e"""
    assert keep.shape[-1] % 8 == 0
    bits = keep.reshape(-1, 8).to(torch.int64) << torch.arange(8)
    return bits.sum(1).to(torch.uint8)


def unpack_mask(mask, M, C):
    return ((mask.to(torch.int64).unsqueeze(1) >> torch.arange(8)) & 1).bool().reshape(-1)[:M * C].view(M, C)


def residual(acc, res, alpha=1.0):
    """out = alpha * acc + res"""
    return alpha * acc + res


def residual_masked(acc, res, mask, alpha=1.0):
    """out = alpha * acc + (bit ? res : 0), bits as pack_mask lays them out"""
    M, C = acc.shape
    return alpha * acc + res * unpack_mask(mask, M, C)


def residual_cls0(acc, res0, N, H, W, alpha=1.0):
    """out = alpha * acc + res, where res0 [N * ceil(H/2) * ceil(W/2)][C] holds one row per pixel with even row and even column (in image, row, column order) and every
    other pixel gets none (avec_epilogue_t.res_cls0)"""
    C = acc.shape[1]
    full = torch.zeros(N, H, W, C, dtype=F64)
    full[:, ::2, ::2] = res0.view(N, (H + 1) // 2, (W + 1) // 2, C)
    return alpha * acc + full.view(-1, C)


def bn_backward_fusion(acc, y, keep, res=None, alpha=1.0):
    """the BatchNorm-backward fusion of the backward-data epilogue: v = alpha * acc + res; v = keep ? v : 0; -> v, [2][C] (sum v, sum v * y)"""
    v = alpha * acc + (0 if res is None else res)
    v = torch.where(keep, v, torch.zeros_like(v))
    return v, column_stats(v, y)


def relu_keep_from_activation(z):
    """dact = 2: the gradient passes where the saved activation is > 0 (0 and -0 block it)"""
    return z > 0


def relu_keep_from_preactivation(y, scale, shift):
    """bnb_mask = 1: the gradient passes where scale * y + shift > 0"""
    return (y * scale + shift) > 0


# ---- preconditions and reports ---------------------------------------------------------------------------------------------------------------
def _bf16_exact(v):
    return bool((v.to(torch.bfloat16).to(F64) == v).all())


def _f32_exact(v):
    return bool((v.to(torch.float32).to(F64) == v).all())


def _grain(t):
    """1, 2 or 4: the terms are whole multiples of 1 / grain (integers; halves where alpha = 0.5 or a half-valued operand enters; their products).  A sum of such terms is
    exact in fp32 while grain * sum |terms| stays below 2^24"""
    for q in (1, 2, 4):
        if bool(((t * q) == (t * q).round()).all()):
            return q
    raise AssertionError("terms finer than quarters")


def check_exact(ref, limits=None):
    """Assert, on the REFERENCE alone, that a correct kernel must reproduce it bit for bit.  `ref` maps
      "bf16":    tensors the kernel stores as bf16: |v| <= 256 and exactly representable (integers, or halves up to 128)
      "f32":     tensors the kernel stores as fp32: exactly representable, |v| < 2^24
      "sums":    [M][C] tensors of terms that the kernel adds up per column in fp32 in an order of its own (v, v^2, v * y): sum_m |term| < 2^24 in every column
                 (counted in units of the terms' grain, see _grain)
      "dw":      (|terms| total, initial value) pairs of a weight gradient: sum |dy * x| + |initial| < 2^24 in every entry, so no partial sum in any order leaves the
                 exact range (this bounds |dW| + |initial| as well)
      "nonzero": reference tensors of which at least 90 % of the elements must be non-zero (equality with a mostly-zero tensor would prove little)
    each a list.  Returns the measured figures."""
    lim = dict(LIMITS)
    if limits:
        assert set(limits) <= set(LIMITS)
        assert limits.get("bf16_max", 0) <= LIMITS["bf16_max"] and limits.get("sum_max", 0) <= LIMITS["sum_max"] and limits.get("nonzero_min", 1) >= LIMITS["nonzero_min"], "limits may only tighten"
        lim.update(limits)
    fig = {"bf16_max": 0.0, "f32_max": 0.0, "sum_max": 0.0, "dw_max": 0.0, "nonzero_min": 1.0}
    for v in ref.get("bf16", []):
        fig["bf16_max"] = max(fig["bf16_max"], float(v.abs().max()))
        assert float(v.abs().max()) <= lim["bf16_max"], "bf16 result of magnitude %g > %g" % (float(v.abs().max()), lim["bf16_max"])
        assert _bf16_exact(v), "a result is not a bf16 number"
    for v in ref.get("f32", []):
        fig["f32_max"] = max(fig["f32_max"], float(v.abs().max()))
        assert float(v.abs().max()) < lim["sum_max"] and _f32_exact(v), "a result is not an exact fp32 number"
    for t in ref.get("sums", []):
        s = _grain(t) * float(t.abs().sum(0).max())
        fig["sum_max"] = max(fig["sum_max"], s)
        assert s < lim["sum_max"], "a column sums |terms| to %g >= %g" % (s, lim["sum_max"])
    for total, init in ref.get("dw", []):
        s = _grain(total + init) * float((total.abs() + (init.abs() if torch.is_tensor(init) else abs(init))).max())
        fig["dw_max"] = max(fig["dw_max"], s)
        assert s < lim["sum_max"], "a weight-gradient entry sums |terms| to %g >= %g" % (s, lim["sum_max"])
        assert _f32_exact(total + init), "initial value + gradient is not an exact fp32 number"
    for v in ref.get("nonzero", []):
        share = float((v != 0).double().mean())
        fig["nonzero_min"] = min(fig["nonzero_min"], share)
        assert share >= lim["nonzero_min"], "only %.3f of the reference is non-zero" % share
    return fig


def describe_mismatch(got, ref, shape, names, first=6):
    """None when got == ref everywhere (NaN in `got` differs), else the count of differing elements and the first few with their coordinates in `shape` (named by `names`)"""
    got, ref = got.reshape(-1).to(F64), ref.reshape(-1).to(F64)
    assert got.numel() == ref.numel(), (got.numel(), ref.numel())
    n = 1
    for s in shape:
        n *= s
    assert n == ref.numel(), (shape, ref.numel())
    bad = torch.nonzero(~(got == ref)).reshape(-1)
    if bad.numel() == 0:
        return None
    lines = ["%d of %d elements differ; (%s): expected / got" % (bad.numel(), ref.numel(), ", ".join(names))]
    for i in bad[:first].tolist():
        coord, r = [], i
        for s in reversed(shape):
            coord.append(r % s); r //= s
        lines.append("  (%s): %r / %r" % (", ".join(str(c) for c in reversed(coord)), float(ref[i]), float(got[i])))
    return "\n".join(lines)


CONV_NAMES = ("image", "row", "column", "channel")
WGRAD_NAMES = ("co", "kh", "kw", "ci")


def assert_exact(got, ref, shape, names, what=""):
    """torch.equal, with the coordinates of the first differences in the failure message"""
    g, r = got.reshape(-1).to(F64), ref.reshape(-1).to(F64)
    if not torch.equal(g, r):
        raise AssertionError("%s\n%s" % (what, describe_mismatch(g, r, shape, names)))


# ---- the operand sets of tests/test_gpu_conv_exact.py ------------------------------------------------------------------------------------------
# Plain data: which kernel instance a case means to reach, its geometry and epilogue.  tests/test_conv_exact_ref.py runs check_exact() on every one of them without a GPU.
def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def nonzero_ints(gen, shape, amax=2):
    """integers uniform in {-amax .. -1, 1 .. amax} (residuals: a structurally empty pixel of a stride-2 backward-data product still gets a non-zero reference)"""
    v = torch.randint(1, amax + 1, tuple(shape), generator=gen)
    return (v * (2 * torch.randint(0, 2, tuple(shape), generator=gen) - 1)).to(F64)


def expand_cls0(res0, N, H, W):
    C = res0.shape[1]
    full = torch.zeros(N, H, W, C, dtype=F64)
    full[:, ::2, ::2] = res0.view(N, (H + 1) // 2, (W + 1) // 2, C)
    return full.view(-1, C)


_NT_DEFAULTS = dict(k=3, stride=1, dtype="bf16", dx=0.5, dw=0.5, stats=False, bias=False, res=None, res_mask=False, res_cls0=False, alpha=1.0, out_f32=False, bnb=None)


def _nt(cid, kernel, mode, imgs, H, W, Cs, Cn, **kw):
    """mode "fwd": x [imgs][H][W][Cs] -> y [.][Cn]; "bwd": dy [imgs][OH][OW][Cs] -> dx [imgs * H * W][Cn].  res: None / "bf16" / "f32"; bnb: None / "act" / "pre" """
    assert set(kw) <= set(_NT_DEFAULTS), kw
    d = dict(_NT_DEFAULTS, id=cid, kernel=kernel, mode=mode, imgs=imgs, H=H, W=W, Cs=Cs, Cn=Cn)
    d.update(kw)
    return d


SHIFT = "conv3x3_shift_kernel<%s>"
S2F, S2B = "conv3x3_s2_fwd_kernel<256,%s>", "conv3x3_s2_bwd_kernel<256,%s>"
CLEAN = "gemm_nt_conv_lean_kernel<%s>"
GLDS = "gemm_nt_glds_kernel<%s>"

# section 1 (and 5): forward and backward-data through the conv modes of avec_gemm_nt
NT_CASES = [
    # shifted-window kernel, 3x3 / stride 1 (tile height by the host's wave-quantisation rule: 2 tiles of 128 rows -> 128, 1 or 3 -> 256; tiles of 128 rows hold two 8x8 images)
    _nt("shift_128x64_fwd_stats", SHIFT % "128,64,1", "fwd", 12, 8, 8, 32, 64, stats=True),
    _nt("shift_128x64_bwd_res_ragged", SHIFT % "128,64,2", "bwd", 13, 8, 8, 32, 64, res="bf16", alpha=0.5),
    _nt("shift_128x128_fwd_stats", SHIFT % "128,128,1", "fwd", 4, 8, 8, 32, 128, stats=True),
    _nt("shift_128x128_bwd_f32", SHIFT % "128,128,2", "bwd", 4, 8, 8, 32, 128, res="f32", out_f32=True),
    _nt("shift_256_tr_fwd_1538", SHIFT % "256,128,1,tr", "fwd", 1538, 8, 8, 32, 128, stats=True, dx=0.4, dw=0.4),
    _nt("shift_256_tr_bwd_res_ragged", SHIFT % "256,128,2,tr", "bwd", 5, 8, 8, 32, 128, res="bf16"),
    _nt("shift_256_tr_bwd_res_mask", SHIFT % "256,128,2,tr", "bwd", 12, 8, 8, 32, 128, res="bf16", res_mask=True, alpha=0.5),
    _nt("shift_256_staged_fwd_bias", SHIFT % "256,128,1", "fwd", 5, 8, 8, 32, 128, bias=True, stats=True),
    _nt("shift_256_staged_bwd_1538", SHIFT % "256,128,2", "bwd", 1538, 8, 8, 32, 128, res="f32", alpha=0.5, dx=0.4, dw=0.4),
    _nt("shift_w31_h5_fwd", SHIFT % "128,64,1", "fwd", 3, 5, 31, 32, 64, stats=True),
    _nt("shift_h31_w5_bwd", SHIFT % "128,64,2", "bwd", 3, 31, 5, 32, 64, res="bf16"),
    _nt("shift_one_image", SHIFT % "256,128,1,tr", "fwd", 1, 8, 8, 32, 128, stats=True),
    _nt("shift_7x12_bwd", SHIFT % "128,128,2", "bwd", 9, 7, 12, 32, 128, res="bf16", alpha=0.5),
    _nt("shift_12x7_fwd", SHIFT % "128,128,1", "fwd", 9, 12, 7, 32, 128, stats=True),
    # 3x3 / stride 2 over the parity classes (the register-direct epilogue only: alpha, bf16 residual, statistics)
    _nt("s2_fwd_even_128", S2F % "128,1", "fwd", 20, 12, 8, 32, 128, stride=2, stats=True),
    _nt("s2_fwd_7x12_64", S2F % "64,0", "fwd", 20, 7, 12, 32, 64, stride=2, stats=True),
    _nt("s2_fwd_12x7_128", S2F % "128,0", "fwd", 20, 12, 7, 32, 128, stride=2, alpha=0.5),
    _nt("s2_fwd_ow15", S2F % "64,1", "fwd", 7, 4, 30, 32, 64, stride=2, stats=True),
    _nt("s2_fwd_ow2", S2F % "64,0", "fwd", 30, 9, 3, 32, 64, stride=2, stats=True),
    _nt("s2_fwd_one_image", S2F % "128,0", "fwd", 1, 11, 11, 32, 128, stride=2, stats=True),
    _nt("s2_bwd_even_64", S2B % "64,1", "bwd", 20, 8, 12, 32, 64, stride=2, res="bf16", dx=1.0, dw=1.0),
    _nt("s2_bwd_12x7_128", S2B % "128,0", "bwd", 20, 12, 7, 32, 128, stride=2, alpha=0.5, dx=1.0, dw=1.0),
    _nt("s2_bwd_7x12_cls0", S2B % "64,0", "bwd", 20, 7, 12, 64, 64, stride=2, res="bf16", res_cls0=True, dx=1.0),
    _nt("s2_bwd_ow15", S2B % "64,1", "bwd", 7, 4, 30, 32, 64, stride=2, dx=1.0, dw=1.0),
    _nt("s2_bwd_ow2", S2B % "128,0", "bwd", 30, 9, 3, 32, 128, stride=2, res="bf16", dx=1.0, dw=1.0),
    _nt("s2_bwd_one_image", S2B % "64,0", "bwd", 1, 11, 11, 32, 64, stride=2, dx=1.0, dw=1.0),
    # parity-class order in the LDS-DMA kernel: OW = 16 is too wide for the stride-2 kernel
    _nt("perm2_glds_ow16", GLDS % "bf16,64,64,2,4,1,128", "bwd", 2, 30, 32, 64, 64, stride=2, dx=1.0),
    _nt("perm2_glds_ow16_cls0", GLDS % "bf16,64,64,2,4,1,128", "bwd", 2, 30, 32, 64, 64, stride=2, res="bf16", res_cls0=True, alpha=0.5, dx=1.0),
    _nt("perm2_glds_33x32_one_image", GLDS % "bf16,64,64,2,4,1,128", "bwd", 1, 33, 32, 64, 64, stride=2, res="bf16", dx=1.0),
    # 1x1 shortcut convolutions on the 128-row tiles (>= 384 tiles: 49152 rows)
    _nt("clean_fwd_128_tr_ragged", CLEAN % "128,1,tr", "fwd", 769, 8, 8, 64, 128, k=1, stats=True, dx=1.0, dw=1.0),
    _nt("clean_bwd_128_staged", CLEAN % "128,2", "bwd", 768, 8, 8, 64, 128, k=1, res="f32", alpha=0.5, dx=1.0, dw=1.0),
    _nt("clean_bwd_res_mask_tr", CLEAN % "128,2,tr", "bwd", 768, 8, 8, 64, 128, k=1, res="bf16", res_mask=True, dx=1.0, dw=1.0),
    _nt("clean_bwd_s2_7x12_tr", CLEAN % "128,2,tr", "bwd", 586, 7, 12, 64, 128, k=1, stride=2, res="bf16", dx=1.0, dw=1.0),
    _nt("clean_fwd_s2_12x7_staged_ragged", CLEAN % "64,1", "fwd", 2049, 12, 7, 64, 64, k=1, stride=2, out_f32=True, stats=True, dx=1.0, dw=1.0),
    # the general LDS-DMA conv kernel by fall-through: W = 32, the 1x1 cases below the 128-row tiles
    _nt("glds_w32_fwd", GLDS % "bf16,64,64,1,4,0,128", "fwd", 5, 6, 32, 32, 64, stats=True),
    _nt("glds_1x1_fwd_5x7", GLDS % "bf16,64,64,1,4,1,128", "fwd", 40, 5, 7, 64, 64, k=1, stats=True, dx=1.0, dw=1.0),
    _nt("glds_1x1_bwd_s2_7x12", GLDS % "bf16,64,64,2,4,1,128", "bwd", 40, 7, 12, 64, 64, k=1, stride=2, res="bf16", alpha=0.5, dx=1.0, dw=1.0),
    _nt("glds_1x1_bwd_s2_12x7_cls_order", GLDS % "bf16,64,64,2,4,1,128", "bwd", 7, 12, 7, 64, 64, k=1, stride=2, res="bf16", dx=1.0, dw=1.0),
    _nt("glds_1x1_fwd_one_image", GLDS % "bf16,64,64,1,4,1,128", "fwd", 1, 7, 5, 64, 64, k=1, stats=True, dx=1.0, dw=1.0),
    # fp32 operands, the fp32 MFMA path
    _nt("f32_3x3_fwd_5x7", GLDS % "float,64,64,1,4,1,128", "fwd", 9, 5, 7, 32, 64, dtype="f32", stats=True),
    _nt("f32_3x3_bwd_7x5", GLDS % "float,64,64,2,4,1,128", "bwd", 9, 7, 5, 32, 64, dtype="f32", res="f32", alpha=0.5),
]

# section 2: the BatchNorm-backward fusion.  epi_tr_ok() (csrc/gemm.hip) and the stride-2 kernel both decline a launch with bnb_y, so the fusion exists in the staged
# epilogue (nt_epilogue) alone; the cases below reach it from the shifted-window kernel at its three tile shapes, from the 1x1 kernel, and in parity-class order
BNB_CASES = [
    _nt("bnb_shift_128x64_act", SHIFT % "128,64,2", "bwd", 13, 8, 8, 32, 64, bnb="act", res="bf16"),
    _nt("bnb_shift_128x128_pre", SHIFT % "128,128,2", "bwd", 4, 8, 8, 32, 128, bnb="pre"),
    _nt("bnb_shift_256_pre", SHIFT % "256,128,2", "bwd", 5, 8, 8, 32, 128, bnb="pre", res="f32", alpha=0.5),
    _nt("bnb_clean_128_act", CLEAN % "128,2", "bwd", 768, 8, 8, 64, 128, k=1, bnb="act", res="bf16", dx=1.0, dw=1.0),
    _nt("bnb_perm2_glds_pre_cls0", GLDS % "bf16,64,64,2,4,1,128", "bwd", 6, 7, 12, 64, 64, stride=2, bnb="pre", res="bf16", res_cls0=True, dx=1.0),
]


def nt_operands(c):
    """operands (float64 integers / halves), references and the check_exact() input of one NT_CASES / BNB_CASES entry"""
    gen = _gen(c["id"])
    k, s, imgs, H, W, Cs, Cn = c["k"], c["stride"], c["imgs"], c["H"], c["W"], c["Cs"], c["Cn"]
    OH, OW = out_size(H, s), out_size(W, s)
    w = weights(gen, (Cn, k, k, Cs), c["dw"])
    if c["mode"] == "fwd":
        a = activations(gen, (imgs, H, W, Cs), c["dx"])
        acc, pix = conv_fwd(a, w, s), (OH, OW)
    else:
        a = activations(gen, (imgs, OH, OW, Cs), c["dx"])
        acc, pix = conv_bwd_data(a, w, H, W, s), (H, W)
    M = acc.shape[0]
    o = dict(a=a, w=w.reshape(Cn, -1), M=M, N=Cn, K=k * k * Cs, rows=(H, W, Cs, k, k, s, (k - 1) // 2, OH, OW), shape=(imgs,) + pix + (Cn,))
    chk = {"bf16": [], "f32": [], "sums": [], "nonzero": []}
    if c["bias"]:
        o["bias"] = draw_ints(gen, (Cn,), 2)
        acc = acc + o["bias"]
    full = None
    if c["res"]:
        assert not c["res_cls0"] or (c["mode"] == "bwd" and s == 2)
        o["res"] = nonzero_ints(gen, (imgs * ((H + 1) // 2) * ((W + 1) // 2) if c["res_cls0"] else M, Cn))
        full = expand_cls0(o["res"], imgs, H, W) if c["res_cls0"] else o["res"]
        if c["res_mask"]:
            o["mask"] = pack_mask(torch.rand((M, Cn), generator=gen) < 0.5)
    if c["bnb"]:
        if c["bnb"] == "act":      # saved activation: integers, with +0 and -0 planted (neither lets the gradient pass)
            y = draw_ints(gen, (M, Cn), 2)
            z = draw_ints(gen, (M, Cn), 2)
            z.view(-1)[3::7] = 0.0
            z.view(-1)[::7] = -0.0
            keep = relu_keep_from_activation(z)
            o["z"] = z
        else:                      # scale * y + shift in halves: exact in fp32, fused or not, and exactly zero at many elements (y = -0 planted as well)
            y = draw_ints(gen, (M, Cn), 4) / 2
            y.view(-1)[::11] = -0.0
            scale = nonzero_ints(gen, (Cn,), 2) / 2
            shift = draw_ints(gen, (Cn,), 2) / 2
            pre = y * scale + shift
            assert int((pre == 0).sum()) > M * Cn // 50
            keep = relu_keep_from_preactivation(y, scale, shift)
            o["ss"] = torch.cat([scale, shift])
        o["y"] = y
        out, st = bn_backward_fusion(acc, y, keep, full, c["alpha"])
        chk["sums"] += [out, out * y]
        chk["nonzero"].append(residual(acc, 0 if full is None else full, c["alpha"]))      # before the mask, which zeroes about half by design
        o["stats"] = st
    else:
        if full is None:
            out = c["alpha"] * acc
        elif c["res_mask"]:
            out = residual_masked(acc, o["res"], o["mask"], c["alpha"])
        elif c["res_cls0"]:
            out = residual_cls0(acc, o["res"], imgs, H, W, c["alpha"])
        else:
            out = residual(acc, full, c["alpha"])
        chk["nonzero"].append(residual(acc, 0 if full is None else full, c["alpha"]))      # (a masked residual leaves alpha * acc behind: judged without the mask)
        if c["stats"]:
            o["stats"] = column_stats(acc)
            chk["sums"] += [acc, acc * acc]
    if "stats" in o:
        chk["f32"].append(o["stats"])
    chk["f32" if c["out_f32"] or c["dtype"] == "f32" else "bf16"].append(out)
    o["out"], o["check"] = out, chk
    return o


# section 3: the stage-1 slab kernels (64 -> 64 channels).  (images, H, W, flip, what): what = "stats" / "res" / "masked" / None
SLAB_CASES = [
    ("slab_fwd_stats_22x22", 5, 22, 22, 0, "stats"), ("slab_fwd_stats_20x22", 2, 20, 22, 0, "stats"), ("slab_fwd_stats_300_7x5", 300, 7, 5, 0, "stats"),
    ("slab_fwd_plain_5x7", 3, 5, 7, 0, None), ("slab_fwd_one_image", 1, 22, 22, 0, "stats"),
    ("slab_bwd_res_21x22", 3, 21, 22, 1, "res"), ("slab_bwd_res_300_5x7", 300, 5, 7, 1, "res"), ("slab_bwd_res_one_image", 1, 6, 6, 1, "res"),
    ("slab_bwd_masked_22x22", 5, 22, 22, 1, "masked"), ("slab_bwd_masked_260_7x5", 260, 7, 5, 1, "masked"), ("slab_fwd_masked_20x22", 2, 20, 22, 0, "masked"),
]


def slab_operands(case):
    cid, imgs, H, W, flip, what = case
    gen = _gen(cid)
    a = activations(gen, (imgs, H, W, 64))
    w = weights(gen, (64, 3, 3, 64))
    acc = conv_bwd_data(a, w, H, W) if flip else conv_fwd(a, w)
    o = dict(a=a, w=w.reshape(64, 576), shape=(imgs, H, W, 64))
    chk = {"bf16": [], "f32": [], "sums": [], "nonzero": [acc]}
    out = acc
    if what == "stats":
        o["stats"] = column_stats(acc)
        chk["sums"] += [acc, acc * acc]
        chk["f32"].append(o["stats"])
    elif what in ("res", "masked"):
        o["res"] = nonzero_ints(gen, acc.shape)
        if what == "masked":
            o["mask"] = pack_mask(torch.rand(acc.shape, generator=gen) < 0.5)
            out = residual_masked(acc, o["res"], o["mask"])
        else:
            out = residual(acc, o["res"])
    chk["bf16"].append(out)
    o["out"], o["check"] = out, chk
    return o


# section 4: weight gradients.  (images, C, H, W, K, stride, initial dW value); dy has C channels as well unless Co says otherwise
def _wg(cid, imgs, C, H, W, K=3, stride=1, init=0.5, Co=None, dtype="bf16"):
    return dict(id=cid, imgs=imgs, C=C, H=H, W=W, K=K, stride=stride, init=init, Co=C if Co is None else Co, dtype=dtype)


WG64_CASES = [_wg("wg64_22x22", 5, 64, 22, 22), _wg("wg64_20x22", 2, 64, 20, 22, init=-3.0), _wg("wg64_21x22", 3, 64, 21, 22), _wg("wg64_one_image", 1, 64, 22, 22),
              _wg("wg64_300_7x5", 300, 64, 7, 5), _wg("wg64_5x7", 7, 64, 5, 7, init=2.0)]
WG64_GROUP = [_wg("wg64_grp_a", 5, 64, 22, 22, init=1.0), _wg("wg64_grp_b", 9, 64, 5, 7, init=-0.5), _wg("wg64_grp_c", 1, 64, 20, 22, init=0.25), _wg("wg64_grp_d", 270, 64, 7, 5)]
PAIRS, WIDE = "wgrad3x3_pairs_grouped_kernel", "wgrad3x3_wide_grouped_kernel"
WG128_CASES = [(_wg("wg128_11x11", 7, 128, 11, 11), PAIRS), (_wg("wg256_6x6", 37, 256, 6, 6, init=-0.25), PAIRS), (_wg("wg512_3x3", 9, 512, 3, 3), PAIRS),
               (_wg("wg128_one_image_11x11", 1, 128, 11, 11), PAIRS), (_wg("wg128_5x7", 4, 128, 5, 7), WIDE), (_wg("wg128_7x5", 5, 128, 7, 5, init=3.0), WIDE),
               (_wg("wg128_8x8", 3, 128, 8, 8), WIDE), (_wg("wg256_one_image_3x4", 1, 256, 3, 4), WIDE)]
# one grouped launch that mixes the pair-kernel geometries with slab-kernel ones, image counts that leave the last iteration of a workgroup partly filled
WG128_GROUP = [_wg("wg_mix_a", 6, 128, 11, 11, init=1.0), _wg("wg_mix_b", 4, 128, 5, 7, init=-2.0), _wg("wg_mix_c", 23, 512, 3, 3), _wg("wg_mix_d", 3, 256, 7, 5, init=0.25),
               _wg("wg_mix_e", 37, 256, 6, 6, init=-0.5)]
TN_TR, TN_GEN = "gemm_tn_tr_kernel<%s>", "gemm_tn_kernel<%s>"
# avec_gemm_tn / avec_gemm_tn_bias with conv-gathered rows: (case, kernel, element offset of P from an aligned address, column sums?)
TN_CASES = [
    (_wg("tn_tr_3x3_5x7", 41, 64, 5, 7), TN_TR % "64,64,1,2,1,32", 0, False),
    (_wg("tn_generic_unaligned_3x3", 11, 64, 7, 5, init=-1.0), TN_GEN % "bf16,64,64,1,0,0", 2, False),
    (_wg("tn_f32_3x3", 9, 32, 5, 7, Co=64, dtype="f32"), TN_GEN % "float,64,64,1,0,1", 0, False),
    (_wg("tn_tr_3x3_s2_7x12", 12, 64, 7, 12, stride=2), TN_TR % "64,64,1,2,1,32", 0, False),
    (_wg("tn_tr_3x3_s2_12x7", 12, 64, 12, 7, stride=2, Co=128, init=2.0), TN_TR % "64,64,1,2,1,32", 0, False),
    (_wg("tn_tr_1x1_s2_7x12", 30, 64, 7, 12, K=1, stride=2, Co=128), TN_TR % "64,64,1,2,1,32", 0, False),
    (_wg("tn_bias_tr_1x1_s2_12x7", 30, 64, 12, 7, K=1, stride=2, Co=128, init=-0.5), TN_TR % "64,64,1,2,1,32", 0, True),
    (_wg("tn_bias_separate_pass_3x3", 6, 64, 8, 8), TN_GEN % "bf16,64,64,1,0,0", 2, True),
    (_wg("tn_tr_3x3_one_image", 1, 64, 9, 11, init=1.0), TN_TR % "64,64,1,2,1,32", 0, False),
]
# dense operands (density 1) where the reduction over pixels is short (few small images): with density 0.5 too many gradient entries would be zero for check_exact
_WG_DENSE = {"tn_tr_3x3_one_image", "tn_tr_1x1_s2_7x12", "tn_bias_tr_1x1_s2_12x7", "wg256_one_image_3x4", "wg128_one_image_11x11", "wg_mix_c", "wg512_3x3", "wg128_8x8", "wg128_5x7", "wg128_7x5", "wg_mix_b", "wg_mix_d"}


def wgrad_operands(c):
    gen = _gen(c["id"])
    d = 1.0 if c["id"] in _WG_DENSE else 0.5
    OH, OW = out_size(c["H"], c["stride"]), out_size(c["W"], c["stride"])
    x = activations(gen, (c["imgs"], c["H"], c["W"], c["C"]), d)
    dy = activations(gen, (c["imgs"], OH, OW, c["Co"]), d)
    dW = conv_wgrad(x, dy, c["K"], c["stride"])
    total = conv_wgrad(x.abs(), dy.abs(), c["K"], c["stride"])
    colsum = dy.reshape(-1, c["Co"]).sum(0)
    o = dict(x=x, dy=dy, dW=dW, out=dW + c["init"], colsum=colsum + c["init"], shape=tuple(dW.shape),
             rows=(c["H"], c["W"], c["C"], c["K"], c["K"], c["stride"], (c["K"] - 1) // 2, OH, OW))
    o["check"] = {"dw": [(total, c["init"])], "sums": [dy.reshape(-1, c["Co"])], "f32": [o["out"], o["colsum"]], "nonzero": [dW]}
    return o


def all_operand_sets():
    """(id, builder) of every operand set the GPU file uses"""
    sets = [(c["id"], (lambda c=c: nt_operands(c))) for c in NT_CASES + BNB_CASES]
    sets += [(c[0], (lambda c=c: slab_operands(c))) for c in SLAB_CASES]
    wg = WG64_CASES + WG64_GROUP + [c for c, _ in WG128_CASES] + WG128_GROUP + [t[0] for t in TN_CASES]
    sets += [(c["id"], (lambda c=c: wgrad_operands(c))) for c in wg]
    return sets
