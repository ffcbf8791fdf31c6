"""Integer operands and plain float64 references for the visual stem: Conv3d(1 -> 64, (5,7,7), stride (1,2,2), pad (2,3,3)) + BatchNorm3d + ReLU + the 3x3 / stride-2 /
pad-1 window pool, in the layouts of csrc/stem3p.hip, csrc/stem3d.hip and the stem tail of csrc/frontend.hip.  Torch on the CPU only; no project code is called.

Same idea as tests/conv_exact_ref.py (whose check_exact / assert_exact / describe_mismatch are reused): operands that leave a correct kernel no choice.
  video     integers in {-2 .. 2}
  weights   {-1, 0, 1}, at most TAP_CAP non-zero taps per channel (|z| <= 2 * TAP_CAP + 32: a bf16 integer), every one of the 245 taps non-zero in some channel,
            channels 0 .. 7 ONE-HOT (a single tap +-1: z is a shifted copy of the video plus the bias, so a tap-index or padding slip names itself)
  bias      integers, non-zero, all different;  mean: integers, non-zero
  gamma, rstd, scale = gamma * rstd, 1 / n, dstats / n: signed powers of two, different per channel, none 1 or 0; gamma < 0 on every fifth channel (the min-pool ones)
  pooled gradients: integers in {-3 .. 3}
Integer frames tie all the time inside a 3x3 window: the first-candidate-wins rule is tested at almost every window.

Layouts (frames F = clips * T, rows m = (f * OH + oh) * OW + ow):
  z, dz, dr [F * OH * OW][64];  zp, idx, dp [F][PH][PW][64];  w [64][245], k = (kd * 7 + kh) * 7 + kw;  ss [4][C] = scale | shift | mean | rstd
"""
import functools
import zlib

import torch

from tests.conv_exact_ref import F64, TWO24, assert_exact, check_exact, describe_mismatch  # noqa: F401  (re-exported for the test files)

C64 = 64
KD, KH, KW = 5, 7, 7
NTAP = KD * KH * KW          # 245
TAP_CAP = 12
ONE_HOT = [(0, 0, 0), (4, 6, 6), (2, 3, 3), (0, 6, 0), (4, 0, 6), (2, 0, 3), (1, 3, 0), (3, 3, 6)]      # (kd, kh, kw) of channels 0 .. 7: corners in space and time, the centre
COUNT = 2048.0               # the `count` of the dz formula: 1 / n = 2^-11
PIX_NAMES = ("frame", "row", "column", "channel")
TAP_NAMES = ("channel", "kd", "kh", "kw")
STAT_NAMES = ("sum | second moment", "channel")


def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def ints(gen, shape, amax):
    return torch.randint(-amax, amax + 1, tuple(shape), generator=gen).to(F64)


def signs(gen, shape):
    return (2 * torch.randint(0, 2, tuple(shape), generator=gen) - 1).to(F64)


def out_size(n):
    return (n - 1) // 2 + 1


# ---- per-channel constants -------------------------------------------------------------------------------------------------------------------------
def channel_constants(C=C64):
    """gamma = +-2^odd, rstd = 2^even (non-zero exponent): scale = gamma * rstd is never 1.  shift = -scale * thr: scale * v + shift is EXACTLY zero where v == thr
    (`> 0`, not `>= 0`).  dstats / n in {+-2, +-1/2}."""
    c = torch.arange(C)
    gamma = torch.tensor([2.0, 8.0, 0.5, 0.125], dtype=F64)[c % 4] * torch.where(c % 5 == 0, -1.0, 1.0).to(F64)
    rstd = torch.tensor([4.0, 0.25, 16.0], dtype=F64)[c % 3]
    mean = ((c % 7) - 3).to(F64)
    mean[mean == 0] = 4.0
    bias = torch.where(c < C // 2, c - C // 2, c - C // 2 + 1).to(F64)                      # -C/2 .. -1, 1 .. C/2
    scale = gamma * rstd
    thr = ((c % 5) - 2).to(F64)
    shift = -scale * thr
    d0n = torch.tensor([2.0, -0.5, -2.0, 0.5], dtype=F64)[(c // 2) % 4]
    d1n = torch.tensor([0.5, 2.0, -0.5, -2.0], dtype=F64)[(c // 3) % 4]
    k = dict(gamma=gamma, rstd=rstd, mean=mean, bias=bias, scale=scale, shift=shift, thr=thr, dstats=torch.stack([d0n, d1n]) * COUNT)
    for name in ("gamma", "rstd", "scale"):
        v = k[name].abs()
        assert bool((v != 1).all() and (v != 0).all() and (torch.log2(v) == torch.log2(v).round()).all()), name
    assert bool((mean != 0).all() and (bias != 0).all()) and len(set(bias.tolist())) == C
    return k


def ss_of(k):
    return torch.stack([k["scale"], k["shift"], k["mean"], k["rstd"]])


@functools.lru_cache(maxsize=None)
def stem_weights():
    """[64][245]: see the module header"""
    gen = _gen("stem weights")
    w = torch.zeros(C64, NTAP, dtype=F64)
    for c, (kd, kh, kw) in enumerate(ONE_HOT):
        w[c, (kd * KH + kh) * KW + kw] = 1.0 if c % 2 == 0 else -1.0
    rest = C64 - len(ONE_HOT)
    for i, t in enumerate(torch.randperm(NTAP, generator=gen).tolist()):                    # every tap lives in one channel at least
        w[len(ONE_HOT) + i % rest, t] = float(signs(gen, (1,)))
    for c in range(len(ONE_HOT), C64):
        for t in torch.randperm(NTAP, generator=gen)[:TAP_CAP - 5].tolist():
            if w[c, t] == 0:
                w[c, t] = float(signs(gen, (1,)))
    assert bool(((w != 0).sum(1) <= TAP_CAP).all()) and bool((w != 0).any(0).all()), "tap cap / tap coverage"
    assert bool(((w[:len(ONE_HOT)] != 0).sum(1) == 1).all())
    return w


def pack_w8(w, zero_first):
    """[64][245] -> [64][36][8]: per (kd, kh) row the 7 kw taps and one zero slot (first: stem3p, last: stem3d), row 35 zero"""
    w8 = torch.zeros(w.shape[0], 36, 8, dtype=F64)
    w8[:, :35, 1 if zero_first else 0:8 if zero_first else 7] = w.view(w.shape[0], 35, 7)
    return w8


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------
def im2col(video, ldk=NTAP):
    """[clips][T][H][W] -> [clips * T * OH * OW][ldk]: column k = (kd * 7 + kh) * 7 + kw holds video[clip][t + kd - 2][2 oh + kh - 3][2 ow + kw - 3] (zero outside the clip
    in time and outside the frame), columns 245 .. ldk - 1 are zero"""
    B, T, H, W = video.shape
    OH, OW = out_size(H), out_size(W)
    vp = torch.zeros(B, T + 4, H + 7, W + 7, dtype=F64)
    vp[:, 2:2 + T, 3:3 + H, 3:3 + W] = video
    A = torch.zeros(B * T * OH * OW, ldk, dtype=F64)
    for kd in range(KD):
        for kh in range(KH):
            for kw in range(KW):
                A[:, (kd * KH + kh) * KW + kw] = vp[:, kd:kd + T, kh:kh + 2 * (OH - 1) + 1:2, kw:kw + 2 * (OW - 1) + 1:2].reshape(-1)
    return A


def conv(video, w, bias):
    """z [M][64] = bias + the convolution; [2][64] column sums of z and z^2"""
    z = im2col(video) @ w.t() + bias
    return z, torch.stack([z.sum(0), (z * z).sum(0)])


def _pool(v, F, OH, OW, floor, none):
    """3x3 / stride 2 / pad 1 window maximum of v [F * OH * OW][C] over the candidates INSIDE the frame, scanned kh-major; a candidate wins only when it is GREATER than
    the best so far (first one on ties), starting from `floor` with slot `none` -> best value, slot kh * 3 + kw, flat row of the winner (-1: none)"""
    C = v.shape[1]
    PH, PW = out_size(OH), out_size(OW)
    vp = torch.full((F, OH + 2, OW + 2, C), float("-inf"), dtype=F64)
    vp[:, 1:1 + OH, 1:1 + OW] = v.view(F, OH, OW, C)
    rows = torch.full((F, OH + 2, OW + 2, 1), -1, dtype=torch.int64)
    rows[:, 1:1 + OH, 1:1 + OW, 0] = torch.arange(F * OH * OW).view(F, OH, OW)
    best = torch.full((F, PH, PW, C), float(floor), dtype=F64)
    slot = torch.full((F, PH, PW, C), none, dtype=torch.int64)
    src = torch.full((F, PH, PW, C), -1, dtype=torch.int64)
    for kh in range(3):
        for kw in range(3):
            sl = (slice(None), slice(kh, kh + 2 * (PH - 1) + 1, 2), slice(kw, kw + 2 * (PW - 1) + 1, 2))
            cand = vp[sl]
            win = cand > best
            best = torch.where(win, cand, best)
            slot = torch.where(win, torch.full_like(slot, kh * 3 + kw), slot)
            src = torch.where(win, rows[sl].expand_as(src), src)
    return best, slot, src


def pool_raw(z, gamma, F, OH, OW):
    """the stem3p_fwd contract: zp = s * max_window(s * z), s = -1 where gamma < 0 else +1; idx = the winner's slot, never 255 (the centre candidate is always inside)"""
    s = torch.where(gamma < 0, -1.0, 1.0).to(F64)
    best, slot, _ = _pool(z * s, F, OH, OW, float("-inf"), 255)
    assert int(slot.max()) <= 8
    return best * s, slot


def pool_act(z, scale, shift, F, OH, OW):
    """the avec_stem_pool_fwd contract: out = max(0, max_window relu(z * scale + shift)); idx = 255 and ymax = 0 where no candidate is positive; ymax = z under the winner"""
    best, slot, src = _pool(z * scale + shift, F, OH, OW, 0.0, 255)
    C = z.shape[1]
    ymax = torch.where(src >= 0, z[src.clamp_min(0), torch.arange(C).expand_as(src)], torch.zeros_like(best))
    return best, slot, ymax


def reduce(dp, zp, k):
    """d = (zp * scale + shift > 0) ? dp : 0 (what the kernel leaves in dp's place); dstats [2][64] = (sum d, sum d * (zp - mean) * rstd); the terms of the second sum"""
    C = zp.shape[-1]
    d = torch.where(zp * k["scale"] + k["shift"] > 0, dp, torch.zeros_like(dp))
    t = d * (zp - k["mean"]) * k["rstd"]
    return d, torch.stack([d.reshape(-1, C).sum(0), t.reshape(-1, C).sum(0)]), t.reshape(-1, C)


def route(d, idx, OH, OW):
    """dr [F * OH * OW][C]: pixel (h, w) collects the pooled gradients of the up to four windows (ph, pw) whose idx names it: h = 2 ph + kh - 1, w = 2 pw + kw - 1"""
    F, PH, PW, C = d.shape
    drp = torch.zeros(F, OH + 2, OW + 2, C, dtype=F64)
    for kh in range(3):
        for kw in range(3):
            drp[:, kh:kh + 2 * (PH - 1) + 1:2, kw:kw + 2 * (PW - 1) + 1:2] += d * (idx == kh * 3 + kw)
    return drp[:, 1:1 + OH, 1:1 + OW].reshape(-1, C).clone()


def bn_backward(dr, z, k, dstats, count):
    """gamma * rstd * (dr - dstats0 / n - (z - mean) * rstd * dstats1 / n): the exact value and the same rounded ONCE to bf16 (through fp32, in which it is exact)"""
    exact = k["gamma"] * k["rstd"] * (dr - dstats[0] / count - (z - k["mean"]) * k["rstd"] * dstats[1] / count)
    return exact, exact.to(torch.float32).to(torch.bfloat16).to(F64)


def wgrad(dz, patches):
    """dW [64][245] = dz^T patches"""
    return dz.t() @ patches[:, :NTAP]


# ---- preconditions -------------------------------------------------------------------------------------------------------------------------------------
def col_grain(t):
    """per column: the largest power of two (2^-40 .. 2^40) of which every entry is a whole multiple"""
    g = torch.zeros(t.shape[1], dtype=F64)
    for e in range(-40, 41):
        q = t / 2.0 ** e
        g[(q == q.round()).all(0)] = 2.0 ** e
    assert bool((g > 0).all()), "entries finer than 2^-40"
    return g


def units(t, extra=None):
    """sum of |entries| per column in units of the column's grain (a column of terms adds up exactly in fp32, in ANY order, while this stays below 2^24);
    `extra` [C]: an initial value the sum lands on"""
    both = t if extra is None else torch.cat([t, extra.reshape(1, -1).to(F64)])
    return float((both.abs().sum(0) / col_grain(both)).max())


def check_stem_exact(chk):
    """check_exact() of tests/conv_exact_ref.py for its keys "bf16" / "f32", and, with a grain PER COLUMN (the power-of-two constants differ per channel):
      "colsums": (terms [M][C], initial [C]) pairs: every column's sum of magnitudes, initial value included, below 2^24 grains
      "rounded": exact values a kernel rounds once to bf16: each must be an fp32 number (and is then below 2^24 grains of its own)
    -> the figures"""
    fig = check_exact({k: v for k, v in chk.items() if k in ("bf16", "f32")})
    fig["col_units"] = 0.0
    for t, init in chk.get("colsums", []):
        u = units(t, init)
        fig["col_units"] = max(fig["col_units"], u)
        assert u < TWO24, "a column sums |terms| to %g grains >= 2^24" % u
    for v in chk.get("bf16_wide", []):       # bf16 numbers of any magnitude (a few significant bits times a power of two)
        assert bool((v.to(torch.bfloat16).to(F64) == v).all()), "a result is not a bf16 number"
    for v in chk.get("rounded", []):
        assert bool((v.to(torch.float32).to(F64) == v).all()), "a value to be rounded to bf16 is not an exact fp32 number"
        assert float(v.abs().max()) < 2.0 ** 100
    return fig


# ---- the operand sets of tests/test_gpu_stem_exact.py ----------------------------------------------------------------------------------------------------
# stem3p: (clips, T, H, W) and the layout avec_stem3p_geom must report: NB, pn, PH, PW, OH, OW, pitch, fused weight gradient accepted, frames per unit, units
def _p(cid, shape, NB, pn, PH, PW, OH, OW, pitch, wg, CH, NCH, note):
    return dict(id=cid, shape=shape, geom=(NB, pn, PH, PW, OH, OW, pitch, wg, CH, NCH), note=note)


S3P_CASES = [
    _p("t1_one_band_176px", (1, 1, 8, 88), 1, 2, 2, 22, 4, 44, 208, 1, 1, 1, "T = 1: every temporal neighbour outside the clip; 176 pixels = one full 128-pixel tile + a ragged one"),
    _p("w96_odd_oh_two_clips", (2, 3, 10, 96), 1, 3, 3, 24, 5, 48, 224, 1, 3, 1, "OH = 5: kh = 2 of the last pool row out of frame; PW = 24 = 4 x 6 pool threads; pitch 224: roles kernel <0>"),
    _p("h37_two_bands", (1, 2, 37, 88), 2, 5, 10, 22, 19, 44, 208, 1, 2, 1, "odd H, odd OH, NB = 2: the overlap row is recomputed and must be counted once"),
    _p("w96_ragged_last_band", (1, 2, 34, 96), 2, 5, 9, 24, 17, 48, 224, 1, 2, 1, "NB = 2, bands of 5 and 4 pooled rows"),
    _p("t14_two_units", (1, 14, 8, 88), 1, 2, 2, 22, 4, 44, 208, 1, 13, 2, "T = 14 > the 13-frame unit: frames 11, 12 fetched again at the unit boundary, the 6-slot frame ring wraps"),
    _p("h34_w88_unfused", (1, 2, 34, 88), 1, 9, 9, 22, 17, 44, 208, 0, 0, 0, "SH * CPR = 559 > 512: the fused weight gradient declines; dz + stem3d_wgrad is the fallback"),
]
S3P_ROLES_INSTANCE = {208: "<208>", 224: "<0>"}       # pitch -> instance of stem3p_wgrad_roles_kernel (avec_last_kernel reports the name without it)
DW_INIT, STAT_INIT, DG_INIT, DB_INIT = 0.5, (3.0, -2.0), -1.5, 2.5


def s3p_dw_init(k):
    """[64][245] initial value of the stem3p weight gradients: scale[c], a signed power of two per channel that is a whole multiple of the grain of that channel's dz
    (a common 0.5 would not be: gamma * rstd reaches 128, and a sum of multiples of 64 plus 0.5 is no fp32 number once it passes 2^23 * 0.5)"""
    return k["scale"].unsqueeze(1).expand(C64, NTAP).clone()


@functools.lru_cache(maxsize=None)
def s3p_operands(cid):
    c = next(c for c in S3P_CASES if c["id"] == cid)
    B, T, H, W = c["shape"]
    gen = _gen(cid)
    k, w = channel_constants(), stem_weights()
    video = ints(gen, (B, T, H, W), 2)
    F, OH, OW = B * T, out_size(H), out_size(W)
    PH, PW = out_size(OH), out_size(OW)
    A = im2col(video)
    z = A @ w.t() + k["bias"]
    stats = torch.stack([z.sum(0), (z * z).sum(0)])
    zp, idx = pool_raw(z, k["gamma"], F, OH, OW)
    dp = ints(gen, (F, PH, PW, C64), 3)
    d, dstats, xterms = reduce(dp, zp, k)
    dr = route(d, idx, OH, OW)
    zero = torch.zeros(2, C64, dtype=F64)
    o = dict(case=c, video=video, w=w, k=k, A=A, z=z, stats=stats, zp=zp, idx=idx, dp=dp, d=d, dstats=dstats, dr=dr, F=F, OH=OH, OW=OW, PH=PH, PW=PW, M=F * OH * OW)
    chk = {"bf16": [z, zp, d, video], "f32": [stats, dstats], "rounded": [], "colsums": [(z, torch.full((C64,), STAT_INIT[0])), (z * z, torch.full((C64,), STAT_INIT[1])),
                                                                                          (d.reshape(-1, C64), torch.full((C64,), STAT_INIT[0])), (xterms, torch.full((C64,), STAT_INIT[1]))]}
    for name, ds in (("route", zero), ("full", k["dstats"])):
        exact, dz = bn_backward(dr, z, k, ds, COUNT)
        dW = wgrad(dz, A)
        o["dz_" + name], o["dW_" + name] = dz, dW
        chk["rounded"].append(exact)
        # the terms of dW[c][k] are dz[m][c] * A[m][k] (A: integers), their grain the column grain of dz[.][c]; the sum lands on the initial value s3p_dw_init()[c]
        g = col_grain(torch.cat([dz, k["scale"].reshape(1, -1)]))
        tot = dz.abs().t() @ A.abs() + k["scale"].abs().unsqueeze(1)
        chk.setdefault("dw_units", []).append(float((tot / g.unsqueeze(1)).max()))
    o["check"] = chk
    return o


def check_s3p(o):
    fig = check_stem_exact(o["check"])
    fig["dw_units"] = max(o["check"]["dw_units"])
    assert fig["dw_units"] < TWO24, "a weight-gradient entry sums |terms| to %g grains >= 2^24" % fig["dw_units"]
    live = (o["A"] != 0).any(0)                  # (a tap whose frame offset leaves a short clip everywhere has a zero gradient by construction: T = 1 keeps kd = 2 alone)
    fig["dw_nonzero"] = float((o["dW_full"][:, live] != 0).double().mean())
    assert fig["dw_nonzero"] >= 0.9, "only %.3f of the weight gradient is non-zero" % fig["dw_nonzero"]
    return fig


# stem3d: (id, (clips, T, H, W), video offset in floats, note)
S3D_CASES = [
    ("s3d_smallest_7x31", (1, 1, 7, 31), 0, "the smallest supported frame; W % 4 != 0: scalar staging"),
    ("s3d_9x33_two_clips", (2, 3, 9, 33), 0, "OH = 5: half-frame bands of 3 and 2 rows"),
    ("s3d_12x32_float4", (1, 6, 12, 32), 0, "float4 staging"),
    ("s3d_12x32_unaligned", (1, 6, 12, 32), 1, "the same, video one float behind an aligned address: scalar staging again"),
]


@functools.lru_cache(maxsize=None)
def s3d_operands(cid):
    _, (B, T, H, W), off, _ = next(c for c in S3D_CASES if c[0] == cid)
    gen = _gen(cid)
    k, w = channel_constants(), stem_weights()
    video = ints(gen, (B, T, H, W), 2)
    A = im2col(video)
    z, stats = conv(video, w, k["bias"])
    dy = ints(gen, z.shape, 2)
    dW = wgrad(dy, A)
    init = torch.full((C64,), STAT_INIT[0])
    chk = {"bf16": [z, dy, video], "f32": [stats, dW + DW_INIT], "colsums": [(z, init), (z * z, init)], "rounded": []}
    tot = dy.abs().t() @ A.abs() + DW_INIT
    return dict(video=video, w=w, k=k, A=A, z=z, stats=stats, dy=dy, dW=dW, off=off, shape=(B, T, H, W), M=z.shape[0], OH=out_size(H), OW=out_size(W),
                check=chk, dw_units=float(tot.max()) * 2)


IM2COL_SHAPES = [(2, 3, 9, 33), (1, 2, 8, 88)]


def im2col_operands(shape):
    return ints(_gen("im2col %r" % (shape,)), shape, 2)


# avec_stem_pool_fwd / avec_stem_pool_bwd phase 1: (frames, H, W, C).  C = 64 takes the 8-wide apply kernel (C % 8 == 0), C = 12 the generic 4-wide one; C = 4 is the
# narrowest the forward kernel accepts
POOL_CASES = [("pool_9x11_c64", 2, 9, 11, 64), ("pool_9x11_c4", 2, 9, 11, 4), ("pool_7x13_c12", 2, 7, 13, 12)]


@functools.lru_cache(maxsize=None)
def pool_operands(cid):
    _, F, H, W, C = next(c for c in POOL_CASES if c[0] == cid)
    gen = _gen(cid)
    k = channel_constants(C)
    PH, PW = out_size(H), out_size(W)
    y = ints(gen, (F * H * W, C), 4)
    out, idx, ymax = pool_act(y, k["scale"], k["shift"], F, H, W)
    dp = ints(gen, (F, PH, PW, C), 3)
    dr = route(dp, idx, H, W)
    exact, dy_bf16 = bn_backward(dr, y, k, k["dstats"], COUNT)
    none = float((idx == 255).double().mean())
    assert 0.02 < none < 0.9, "share of windows without a positive candidate: %g" % none
    chk = {"bf16": [y, ymax, dp], "bf16_wide": [out], "f32": [exact], "rounded": [exact]}
    return dict(F=F, H=H, W=W, C=C, PH=PH, PW=PW, k=k, y=y, out=out, idx=idx, ymax=ymax, dp=dp, dy_f32=exact, dy_bf16=dy_bf16, check=chk)


# avec_stem3p_reduce alone at a size whose partials exceed 16 384 atomics (135 blocks of 32 rows x 128): the only stem3p reduction with a one-pass threshold
REDUCE_BIG = (2, 33, 65)      # frames, PH, PW: 4290 pooled pixels


@functools.lru_cache(maxsize=None)
def reduce_big_operands():
    F, PH, PW = REDUCE_BIG
    gen = _gen("reduce big")
    k = channel_constants()
    zp, dp = ints(gen, (F, PH, PW, C64), 6), ints(gen, (F, PH, PW, C64), 3)
    d, dstats, xterms = reduce(dp, zp, k)
    chk = {"bf16": [zp, dp, d], "f32": [dstats], "colsums": [(d.reshape(-1, C64), torch.full((C64,), STAT_INIT[0])), (xterms, torch.full((C64,), STAT_INIT[1]))], "rounded": []}
    return dict(zp=zp, dp=dp, d=d, dstats=dstats, k=k, check=chk)


def all_operand_sets():
    """(id, checker) of every operand set the GPU file uses; a checker returns the figures"""
    sets = [(c["id"], (lambda c=c: check_s3p(s3p_operands(c["id"])))) for c in S3P_CASES]

    def s3d(cid):
        o = s3d_operands(cid)
        fig = check_stem_exact(o["check"])
        assert o["dw_units"] < TWO24
        return fig
    sets += [(c[0], (lambda c=c: s3d(c[0]))) for c in S3D_CASES]
    sets += [(c[0], (lambda c=c: check_stem_exact(pool_operands(c[0])["check"]))) for c in POOL_CASES]
    sets += [("reduce_big", lambda: check_stem_exact(reduce_big_operands()["check"]))]
    sets += [("im2col %r" % (s,), (lambda s=s: check_stem_exact({"bf16": [im2col_operands(s)]}))) for s in IM2COL_SHAPES]
    return sets
