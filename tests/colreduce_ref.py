"""Host-side pieces of the column-reduction / fused conv-module BatchNorm kernel tests (tests/test_gpu_colreduce.py, tests/test_gpu_convmod_bn.py):
launch-geometry restatements, input generators, fp64 reference formulas, the per-column error metric and the exact-arithmetic bounds.  Pure torch on
the host -- tests/test_colreduce_ref.py exercises everything here without a GPU.

The geometry functions restate avec_amd/csrc/vec.h, convmod.hip and frontend.hip.  They are used ONLY to choose shapes (how many partial-sum slots a
shape produces, how many floats of workspace it needs); whether a launch really took the two-pass path is observed on the GPU from the workspace itself.
"""
import math

import torch

F32_EXACT = 1 << 24            # every integer of magnitude <= 2^24 is a float: integer sums below it are exact in ANY summation order
EPS32 = 2.0 ** -24             # unit round-off of fp32
DW_TT, KMAX, AS_ROWS, AS_NIT = 32, 16, 16, 4
WS_MIN_BYTES = 1 << 16         # the smallest workspace avec_set_reduce_workspace accepts


# ---- launch geometry -----------------------------------------------------------------------------------------------------------------------
def col_grid(M, C):
    """vec.h col_grid: (column blocks of 128, row slots)"""
    gx = (C // 4 + 31) // 32
    return gx, max(1, min((M + 63) // 64, max(2048 // gx, 1)))


def col8_blocks(M, C, cap=1024):
    """vec.h col8_blocks: slots of the flat 8-wide mapping (C % 8 == 0, C <= 2048)"""
    R = 256 // (C // 8)
    return min((M + R - 1) // R, cap)


def col_partial_floats(M, C, NV):
    gx, gy = col_grid(M, C)
    return gx * gy * NV * 128


def dw_grid(B, T, C, stride=1):
    """convmod.hip: (column blocks of 128, B * chunks of 32 output frames)"""
    To = (T - 1) // stride + 1
    return (C // 4 + 31) // 32, B * ((To + DW_TT - 1) // DW_TT)


def stem_dims(n_mels, F):
    return (n_mels - 1) // 2 + 1, (F - 1) // 2 + 1          # Fo, To


def stem_family(n_mels, C):
    """frontend.hip:440-512 -- which of the three audio-stem kernel families a shape runs"""
    Fo = (n_mels - 1) // 2 + 1
    if not (Fo % 8 == 0 and ((n_mels + 2) * 3 + C * 12) * 4 <= 60 * 1024):
        return "generic"
    return "8x" if C * (Fo >> 3) <= AS_NIT * 256 else "8"


def stem_blocks(B, F):
    return (B * ((F - 1) // 2 + 1) + AS_ROWS - 1) // AS_ROWS


# ---- generators (CPU generator: the same numbers on every machine) ---------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def int_tensor(shape, lo, hi, seed):
    """integers in [lo, hi] as float64"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()


def gauss(shape, seed, mean=0.0, std=1.0):
    return torch.randn(tuple(shape), generator=_gen(seed), dtype=torch.float64) * std + mean


def positive(shape, seed):
    """|N(0,1)| + 0.5: no cancellation, so one lost partial of `nslots` moves a column sum by about 1 / nslots of itself"""
    return torch.randn(tuple(shape), generator=_gen(seed), dtype=torch.float64).abs() + 0.5


def as_dtype(x64, dtype):
    """round an fp64 host tensor to the activation dtype ("f32" / "bf16") and give back (rounded tensor in that dtype, the same values in fp64)"""
    t = x64.to(torch.bfloat16 if dtype == "bf16" else torch.float32)
    return t, t.double()


# ---- the per-column metric -------------------------------------------------------------------------------------------------------------------
def col_ratio(got, ref, scale):
    """|got_c - ref_c| / scale_c for every column c, scale_c = sum_i |t_ic| of the fp64 terms of that column's sum (condition-aware: a column of
    small magnitude is judged against its own terms, not against the largest column of the tensor).  A column whose terms are all zero must be exact."""
    got, ref, scale = got.double().flatten(), ref.double().flatten(), scale.double().flatten()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    err = (got - ref).abs()
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))          # NaN (a stale workspace slot) never passes


def worst(got, ref, scale):
    return float(col_ratio(got, ref, scale).max())


def elem_ratio(got, ref, dim_rows=0):
    """per-(frame, channel) error normalised per CHANNEL: max_i |got_ic - ref_ic| / max_i |ref_ic|, one figure per channel (last dim)"""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    return (got - ref).abs().amax(0) / ref.abs().amax(0).clamp_min(1e-30)


# ---- reference formulas (fp64) -----------------------------------------------------------------------------------------------------------------
# The `*_terms` functions give the matrices whose COLUMN SUMS the kernel under test produces, in the dtype of their arguments: fp64 arguments give the
# reference (ref = terms.sum(0), scale = |terms|.sum(0)); fp32 arguments give the plain host evaluation of the same formula whose own error sets the
# tolerance (reduce()).
def reduce(terms):
    """[(ref, scale)] concatenated over the reduced quantities: column sums and column sums of magnitudes"""
    return torch.cat([t.reshape(-1, t.shape[-1]).sum(0) for t in terms]), torch.cat([t.reshape(-1, t.shape[-1]).abs().sum(0) for t in terms])


def stats_terms(x):
    return [x, x * x]


def swish(x):
    return x * torch.sigmoid(x)


def dswish(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def dswish_mag(x):
    """swish'(x) with its two terms taken by magnitude: s (1 + |x| (1 - s)).  swish' crosses zero at x = -1.278; next to the crossing its fp32 rounding error is a
    few eps of THIS, not of swish' itself"""
    s = torch.sigmoid(x)
    return s * (1 + x.abs() * (1 - s))


def d_mag(dout, y, sc, sh):
    """magnitude scale of d = dout swish'(sc y + sh): the terms of swish' by magnitude, plus the pre-activation's own rounding -- sc y + sh is a rounded fp32 sum
    of magnitude |sc y| + |sh|, and |swish''| <= 1/2 carries its error into swish'"""
    return dout.abs() * (dswish_mag(y * sc + sh) + 0.5 * ((y * sc).abs() + sh.abs()))


def bn_finalize_ref(stats, n, gamma, beta, rmean, rvar, momentum, eps, training=True):
    """avec_bn_finalize in fp64.  stats [nrep][2C]; returns ss [4][C] = scale | shift | mean | rstd and the updated running statistics"""
    gamma, beta = gamma.double(), beta.double()
    if training:
        s = stats.double().reshape(-1, stats.shape[-1]).sum(0)
        C = s.numel() // 2
        mean = s[:C] / n
        var = (s[C:] / n - mean * mean).clamp_min(0)
        if rmean is not None:
            rmean = (1 - momentum) * rmean.double() + momentum * mean
            rvar = (1 - momentum) * rvar.double() + momentum * var * (n / max(n - 1.0, 1.0))
    else:
        mean, var = rmean.double(), rvar.double()
    rs = 1 / torch.sqrt(var + eps)
    return torch.stack([gamma * rs, beta - mean * gamma * rs, mean, rs]), rmean, rvar


def bn_bwd_reduce_terms(dout, y, ss, act, out=None, mask=None):
    """terms of avec_bn_bwd_reduce(_mask): (d, d * xhat), d = dout * act'(.); ss fp64 [4][C]; act 0 none, 1 Swish, 2 ReLU (by `out` > 0, by `mask`, else by the
    recomputed pre-activation)"""
    ss = ss.to(dout.dtype)
    if mask is not None:
        d = dout * mask.to(dout.dtype)
    elif act == 2:
        d = dout * ((out > 0) if out is not None else (y * ss[0] + ss[1] > 0)).to(dout.dtype)
    elif act == 1:
        d = dout * dswish(y * ss[0] + ss[1])
    else:
        d = dout
    return [d, d * (y - ss[2]) * ss[3]]


def bn_bwd_reduce_ref(dout, y, ss, act, out=None, mask=None):
    """(reference [2C], scale [2C]); the scale of sum d xhat takes |y| + |mean| for y - mean: that difference is formed in fp32 and its rounding error does not
    shrink with it"""
    t = bn_bwd_reduce_terms(dout, y, ss, act, out, mask)
    ss = ss.to(dout.dtype)
    dm = d_mag(dout, y, ss[0], ss[1]) if act == 1 else t[0].abs()
    return reduce(t)[0], reduce([dm, dm * (y.abs() + ss[2].abs()) * ss[3].abs()])[0]


def pack_mask(m):
    """[M][C] booleans -> the bit layout of avec_bn_apply_fwd_mask: byte k = elements 8k .. 8k+7 of the row-major matrix, bit e = element 8k + e"""
    b = m.reshape(-1, 8).to(torch.int64)
    return (b * (2 ** torch.arange(8))).sum(1).to(torch.uint8)


def audio_stem_ref(mel, w, bias):
    """Conv2d(1 -> C, 3x3, stride 2, pad 1) over mel [B][n_mels][F] -> y [B][To][C * Fo] (channel-major inside a frame), and the same with every factor
    replaced by its magnitude (the scale of y's rounding error)"""
    def conv(m, ww, bb):
        o = torch.nn.functional.conv2d(m.unsqueeze(1), ww.reshape(-1, 1, 3, 3), bb, stride=2, padding=1)      # [B][C][Fo][To]
        return o.permute(0, 3, 1, 2).contiguous()                                                                                          # [B][To][C][Fo]
    return conv(mel, w, bias), conv(mel.abs(), w.abs(), bias.abs())


def audio_stem_patches(mel):
    """[B][To][Fo][9]: the 3x3 input patch of every output element (zero outside)"""
    B, NM, F = mel.shape
    Fo, To = stem_dims(NM, F)
    p = torch.nn.functional.unfold(mel.unsqueeze(1), kernel_size=3, padding=1, stride=2)        # [B][9][Fo * To]
    return p.reshape(B, 9, Fo, To).permute(0, 3, 2, 1).contiguous()


def glu_dwconv_ref(u, w, bias, stride, padl, absolute=False):
    """GLU + depthwise conv in fp64: u [B][T][2C], w tap-major [K][C] -> [B][To][C]; absolute = magnitudes of every factor (error scale)"""
    K, C = w.shape
    To = (u.shape[1] - 1) // stride + 1
    g = torch.nn.functional.glu(u, dim=-1)
    if absolute:
        g, w, bias = g.abs(), w.abs(), bias.abs()
    gp = torch.nn.functional.pad(g.transpose(1, 2), (padl, K - 1 - padl))
    return torch.nn.functional.conv1d(gp, w.t().unsqueeze(1), bias, stride=stride, groups=C)[:, :, :To].transpose(1, 2)


def convmod_ref(u, w, bias, gamma, beta, da, stride, padl, eps):
    """glu -> pad -> conv1d(groups = C) -> batch_norm(training) -> swish in fp64, gradients by autograd from `da`.  All inputs fp64 host tensors.  (BatchNorm is written
    out -- biased batch variance -- because torch refuses a single row per channel; tests/test_colreduce_ref.py checks it against torch.nn.functional.batch_norm.)"""
    u, w, bias, gamma, beta = [t.detach().clone().requires_grad_(True) for t in (u, w, bias, gamma, beta)]
    c = glu_dwconv_ref(u, w, bias, stride, padl)
    B, To, C = c.shape
    c2 = c.reshape(B * To, C)
    mean = c2.mean(0)
    var = ((c2 - mean) ** 2).mean(0)
    rs = 1 / torch.sqrt(var + eps)
    z = (c2 - mean) * rs * gamma + beta
    z.retain_grad()
    a = swish(z)
    out = {"c": c.detach(), "a": a.detach(), "mean": mean.detach(), "var": var.detach(),
           "ss": torch.stack([gamma * rs, beta - mean * gamma * rs, mean, rs]).detach(), "mag": glu_dwconv_ref(u.detach(), w.detach(), bias.detach(), stride, padl, absolute=True)}
    if da is not None:
        a.backward(da.reshape(B * To, C))
        out.update(du=u.grad, dw=w.grad, dbias=bias.grad, dgamma=gamma.grad, dbeta=beta.grad, dz=z.grad)
    return out


def convmod_bwd_ref(u, w, c, ss, gamma, da, padl):
    """the backward of the convolution-module middle from what the backward kernels are GIVEN (stride 1): u, the BatchNorm input c [B][T][C] as stored, ss [4][C] as
    finalized, da; in the dtype of the arguments.  d = da swish'(scale c + shift); dstats = (sum d, sum d xhat); dc = gamma rstd (d - s1/n - xhat s2/n);
    du, dw, dbias = depthwise-convolution + GLU backward of dc.  {name: (reference, scale)}; scales as in stem_bwd_ref (differences by their operands' magnitudes)"""
    B, T, C = c.shape
    K = w.shape[0]
    n = float(B * T)
    pre = c * ss[0] + ss[1]
    d = da * dswish(pre)
    xh = (c - ss[2]) * ss[3]
    s1, s2 = d.reshape(-1, C).sum(0), (d * xh).reshape(-1, C).sum(0)
    dc = gamma * ss[3] * (d - s1 / n - xh * s2 / n)
    dm = d_mag(da, c, ss[0], ss[1])
    xm = (c.abs() + ss[2].abs()) * ss[3].abs()
    dcm = (gamma * ss[3]).abs() * (dm + s1.abs() / n + xm * s2.abs() / n)

    def back(uu, ww, g_out, absolute):
        uu, ww = uu.detach().clone().requires_grad_(True), ww.detach().clone().requires_grad_(True)
        bb = torch.zeros(C, dtype=uu.dtype, requires_grad=True)
        g = torch.nn.functional.glu(uu, dim=-1)
        if absolute:
            g = g.abs()
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(g.transpose(1, 2), (padl, K - 1 - padl)), ww.t().unsqueeze(1), bb, groups=C).transpose(1, 2)
        y.backward(g_out)
        return uu.grad, ww.grad, bb.grad
    du, dw, dbias = back(u, w, dc, False)
    _, dwm, dbm = back(u, w.abs(), dcm, True)
    return {"dstats": (torch.cat([s1, s2]), torch.cat([dm.reshape(-1, C).sum(0), (dm * xm).reshape(-1, C).sum(0)])), "dw": (dw, dwm), "dbias": (dbias, dbm), "du": du, "dc": dc}


# ---- host fp32 emulation of the one-pass statistics (section 5 of the issue: the numerical envelope) --------------------------------------------
def onepass_var_f32(x):
    """var = s2/n - mean^2 with fp32 sums (torch fp32 `sum`), as every statistics kernel of the library computes it"""
    x = x.float()
    n = float(x.shape[0])
    mean = x.sum(0) / n
    return ((x * x).sum(0) / n - mean * mean).clamp_min(0), mean


def var_envelope(mean, var, kappa):
    """allowed relative variance error of the one-pass fp32 formula: kappa * eps_fp32 * (1 + mean^2 / var), eps_fp32 = 2^-23"""
    return kappa * 2.0 ** -23 * (1 + mean.double() ** 2 / var.double())


# ---- tolerances (see the table in tests/test_gpu_colreduce.py; tests/test_colreduce_ref.py re-measures them on the host) --------------------------------
# Per-column tolerance of the random-data cases: |got_c - ref_c| <= TOL[formula] * scale_c.  Each is 8 x the worst ratio that a plain fp32 HOST evaluation of
# the same formula (torch fp32 elementwise arithmetic and `sum` / `einsum`; not the library) reaches over the shape lists below with Gaussian and with positive
# inputs -- the margin for a different summation order.  Measured 2026-10-16 with torch 2 on the CPU (tests/test_colreduce_ref.py measure_host_fp32):
#     formula                  worst host fp32 ratio     x 8
HOST_FP32_WORST = {
    "colsum":                  2.03e-7,               # 1.6e-6   (avec_colsum, avec_grad_prep dbias)
    "bn_stats":                2.13e-7,               # 1.7e-6
    "bn_bwd_reduce":           2.24e-7,               # 1.8e-6   (act none and Swish; the mask variants share the arithmetic of act none)
    "glu_dwconv stats":        2.49e-7,               # 2.0e-6   (avec_glu_dwconv_fwd, avec_glu_dwconv_fwd_bn: mean and the sums behind the variance)
    "audio stem stats":        2.81e-7,               # 2.2e-6
    "audio stem dstats":       5.93e-8,               # 4.7e-7
    "audio stem dw":           2.80e-7,               # 2.2e-6
    "audio stem dbias":        7.29e-8,               # 5.8e-7
    "convmod dstats":          5.14e-8,               # 4.1e-7   (avec_bn_bwd_reduce, act = Swish, on the convolution module's shapes)
    "convmod dw":              1.23e-7,               # 9.8e-7   (avec_dwconv_glu_bwd_bn and the unfused chain)
    "convmod dbias":           5.41e-8,               # 4.3e-7
}
TOL = {k: 8 * v for k, v in HOST_FP32_WORST.items()}
TOL_SUM = max(TOL.values())
# One lost partial of `nslots` moves a positive-valued column sum by about 1 / nslots of itself: 4.9e-4 at the 2048 slots col_grid can reach, 200 x TOL_SUM.
assert TOL_SUM < 1.0 / (2 * 2048)
# One-pass variance envelope |var - var_ref| / var_ref <= KAPPA * eps_fp32 * (1 + mean^2 / var): the host fp32 emulation of the same formula (torch fp32 sums,
# VAR_ROWS rows, var read back through rstd) has the constants 1.56 / 1.65 / 2.91 / 3.12 at mean / std = 0 / 5 / 50 / 300 (relative variance errors 1.9e-7 / 5.1e-6 /
# 8.7e-4 / 3.4e-2); KAPPA = 4 x the worst of them.
HOST_DU_FP32_WORST = 7.04e-7     # du of the convolution-module backward, per channel max |diff| / max |ref| of the fp32 host evaluation (x 8 = 5.6e-6)
HOST_KAPPA_WORST = 3.12
KAPPA = 4 * HOST_KAPPA_WORST
EPS_F32 = 2.0 ** -23     # machine epsilon of fp32 (torch.finfo(torch.float32).eps): the `eps_fp32` of the variance envelope
VAR_ROWS, VAR_RATIOS = 6400, (0.0, 5.0, 50.0, 300.0)


def exact_or_die(scale, name, case, unit=1.0):
    """every term of an exact case is a multiple of `unit`; the sum of the terms' magnitudes bounds every partial sum of every summation order, so below
    2^24 units (less 16 for the pre-filled destination) all of them are fp32 numbers and the result does not depend on the order"""
    worst_sum = float(scale.max()) / unit + 16
    assert worst_sum < F32_EXACT, "%s %s: worst-case sum %g units of %g is not below 2^24 -- not an exact case" % (name, case, worst_sum, unit)


def data(mode, shape, seed, lo=0, hi=3):
    if mode == "exact":
        return int_tensor(shape, lo, hi, seed)
    return positive(shape, seed) if mode == "positive" else gauss(shape, seed)


def variance_case(M, C):
    """[M][C] fp64, channel c has std 1 + (c // 4) % 3 and mean / std = VAR_RATIOS[c % 4]"""
    c = torch.arange(C)
    std = 1.0 + ((c // 4) % 3).double()
    ratio = torch.tensor(VAR_RATIOS, dtype=torch.float64)[c % 4]
    return gauss((M, C), 77) * std + ratio * std


def onepass_var_via_rstd_f32(x32):
    """the host fp32 emulation of avec_bn_stats + avec_bn_finalize(eps = 0) as the tests read it back: var = 1 / rstd^2, rstd = 1 / sqrt(s2/n - mean^2) in fp32"""
    var, _ = onepass_var_f32(x32)
    rs = 1.0 / torch.sqrt(var)
    return 1.0 / rs.double() ** 2


# ---- shape lists: every structural edge of the mappings, read from vec.h / norm.hip / convmod.hip / frontend.hip ----------------------------------------
# (M, C) of the col_grid / col8 kernels.  M: 1, 7, 8, 9 (the 8 row lanes), 63, 64, 65 (one slot per 64 rows), 1234, 6400, slot counts 15 / 16 / 17 and
# 127 / 128 / 129 / 193 (col_finalize: 16 slot lanes x 8, grid.z of 128), 65 600 rows x 132 columns (col_grid caps grid.y at 2048 / grid.x = 1024 < 1025).
# C: 4, 8, 64, 124, 128, 132 (last column block partly empty), 144 (col8: 18 lanes x 14 rows, 4 idle threads), 180 (C % 8 != 0: the 4-wide path), 256, 360,
# 2048 (col8: one row per block; 16 column blocks); 8200 x 256 asks for 1025 col8 blocks and gets the cap of 1024.
SHAPES_COL = [(1, 4), (7, 8), (8, 64), (9, 124), (63, 128), (64, 132), (65, 144), (1234, 180), (6400, 256), (1234, 360), (1, 2048), (9, 2048),
              (960, 2048), (1024, 256), (1088, 132), (8128, 128), (8192, 144), (8256, 180), (12345, 128), (6400, 124), (1234, 128), (6400, 4), (1234, 8), (8200, 256)]
SHAPES_COL_CAP = [(65600, 132)]          # 1025 row slots asked for, 1024 given: exact cases only (8.7 M elements)
# (B, T, C, K, stride, causal) of the depthwise kernels: slots = B * ceil(To / 32)
SHAPES_DW = [(1, 1, 144, 3, 1, False), (1, 5, 180, 15, 1, False), (3, 31, 256, 7, 1, True), (3, 32, 360, 16, 1, False), (1, 33, 132, 15, 1, False),
             (3, 57, 144, 15, 2, False), (32, 100, 144, 15, 1, False), (32, 376, 256, 15, 1, False), (3, 376, 360, 15, 1, True), (32, 33, 180, 3, 2, False),
             (1, 300, 1024, 7, 1, False), (1, 500, 1024, 16, 1, False), (1, 520, 1024, 3, 1, True), (43, 96, 144, 15, 1, False), (127, 32, 144, 7, 1, False),
             (1, 500, 256, 15, 1, False)]
# (B, n_mels, F, C) of the audio stem: 8x family (C * Fo / 8 <= 1024), 8 family, generic (Fo % 8 != 0); one utterance of a few dozen
# frames (and of 3: one output row in the only block); STEM_BENCH is the bench shape, run in the exact mode only (46 M outputs)
SHAPES_STEM = [(1, 80, 61, 180), (1, 80, 3, 180), (2, 80, 64, 180), (1, 160, 61, 180), (3, 160, 95, 180), (1, 30, 61, 180), (3, 30, 40, 36), (1, 16, 70, 4),
               (5, 80, 1001, 64)]
STEM_BENCH = (32, 80, 400, 180)
# (F, the partials fit 64 KB): B = 1, 16 mels, C = 4 -> 8 floats of partials per block of 16 output frames
STEM_EDGE = [(2 * 16 * 2048, True), (2 * 16 * 2048 + 1, False)]


def dw_inputs(mode, shape, i):
    """u [B][T][2C], w [K][C], bias [C] in fp64.  exact: gate half zero (sigmoid = 1/2), value half in {-2, 0, 2}, taps in {-1, 0, 1}, integer bias"""
    B, T, C, K, stride, causal = shape
    if mode == "exact":
        u = torch.cat([2 * int_tensor((B, T, C), -1, 1, 401 + i), torch.zeros(B, T, C, dtype=torch.float64)], -1)
        return u, int_tensor((K, C), -1, 1, 501 + i), int_tensor((C,), -2, 2, 601 + i)
    u = torch.cat([data(mode, (B, T, C), 401 + i), gauss((B, T, C), 451 + i)], -1)
    return u, (positive((K, C), 501 + i) if mode == "positive" else gauss((K, C), 501 + i)) * 0.3, data(mode, (C,), 601 + i)


def dw_stats_ref(u, w, bias, stride, padl):
    """(conv output, reference [2C], scale [2C]) -- the scale takes every factor by its magnitude: the rounding error of c and of c^2"""
    c = glu_dwconv_ref(u, w, bias, stride, padl)
    mag = glu_dwconv_ref(u, w, bias, stride, padl, absolute=True)
    return c, reduce(stats_terms(c))[0], reduce(stats_terms(mag))[0]


def stem_inputs(mode, shape, seed):
    """fp64 inputs of the audio stem forward and backward.  exact: mel in {0, 1}, taps and bias in {-1, 0, 1}; scale = shift = 0 (swish'(0) = 1/2), da in
    {-4 .. 4} even, mean an integer, rstd in {1/2, 1}, gamma in {1, 2}, the reduced sums handed to phase 1 multiples of count = 4"""
    B, NM, F, C = shape
    Fo, To = stem_dims(NM, F)
    c = torch.arange(C)
    if mode == "exact":
        z = torch.zeros(C, dtype=torch.float64)
        return dict(mel=int_tensor((B, NM, F), 0, 1, seed), w=int_tensor((C, 9), -1, 1, seed + 1), bias=int_tensor((C,), -1, 1, seed + 2),
                    ss=torch.stack([z, z, (c % 3).double() - 1, torch.tensor([0.5, 1.0], dtype=torch.float64)[c % 2]]),
                    da=2 * int_tensor((B, To, C, Fo), -2, 2, seed + 3), gamma=torch.tensor([1.0, 2.0], dtype=torch.float64)[c % 2], count=4.0,
                    dstats=4 * int_tensor((2 * C,), -1, 1, seed + 4))
    g = gauss((5, C), seed + 5)
    count = float(B * To * Fo)
    return dict(mel=data(mode, (B, NM, F), seed), w=(positive((C, 9), seed + 1) if mode == "positive" else gauss((C, 9), seed + 1)) * 0.3, bias=data(mode, (C,), seed + 2),
                ss=torch.stack([0.5 + g[0].abs(), 0.3 * g[1], 0.2 * g[2], 0.5 + g[3].abs()]), da=data(mode, (B, To, C, Fo), seed + 3), gamma=0.5 + g[4].abs(),
                count=count, dstats=gauss((2 * C,), seed + 4) * count * 0.05)


def stem_percol(t):
    """[B][To][C][Fo] -> rows (b, to, fo) x columns = channels"""
    return t.permute(0, 1, 3, 2).reshape(-1, t.shape[2])


def stem_fwd_ref(mel, w, bias):
    """(y [B][To][C][Fo], statistics reference [2C], their scale [2C]) in the dtype of the arguments"""
    y, mag = audio_stem_ref(mel, w, bias)
    return y, reduce(stats_terms(stem_percol(y)))[0], reduce(stats_terms(stem_percol(mag)))[0]


def stem_bwd_ref(mel, y, da, ss, gamma, dstats, count):
    """audio-stem backward in the dtype of the arguments (y, da: [B][To][C][Fo]) as {name: (reference, scale)}: phase 0 dstats [2C] = (sum d, sum d xhat),
    d = da swish'(scale y + shift); phase 1 dw [C][9], dbias [C] from dy = gamma rstd (d - s1/n - xhat s2/n).  The scales sum the terms with every difference
    replaced by the sum of its operands' magnitudes (y - mean and the three-term dy are formed in fp32: their rounding errors do not shrink with them)"""
    C = y.shape[2]
    v = lambda t: t.view(1, 1, C, 1)
    dr = da * dswish(y * v(ss[0]) + v(ss[1]))
    xh = (y - v(ss[2])) * v(ss[3])
    dy = v(gamma * ss[3]) * (dr - v(dstats[:C]) / count - xh * v(dstats[C:]) / count)
    p = audio_stem_patches(mel)                                                                 # [B][To][Fo][9]
    e = lambda a, b: torch.einsum("btcf,btfq->cq", a, b)
    xm = (y.abs() + v(ss[2]).abs()) * v(ss[3]).abs()
    drm = d_mag(da, y, v(ss[0]), v(ss[1]))
    dm = v(gamma * ss[3]).abs() * (drm + v(dstats[:C]).abs() / count + xm * v(dstats[C:]).abs() / count)
    return {"dstats": (reduce([stem_percol(dr), stem_percol(dr * xh)])[0], reduce([stem_percol(drm), stem_percol(drm * xm)])[0]),
            "dw": (e(dy, p), e(dm, p.abs())), "dbias": (reduce([stem_percol(dy)])[0], reduce([stem_percol(dm)])[0])}


# (B, T, C, K, stride, causal) of the fused convolution-module tests: T = 1, T < K (the halo is longer than the sequence), the 32-frame chunk boundary +-1, several
# chunks; B in {1, 3, 32}; C in {144, 180, 256, 360}, 132 (just above 128) and 1024 (two-pass statistics with 10 / 16 / 17 slots: bn_finalize_ws_kernel's
# stride-16 loop); K in {3, 7, 15, 16 = KMAX}; "same" and causal; stride 2 (forward only) with odd T.  slots = B * ceil(To / 32); the forward goes two-pass
# above 16 384 / (2 C) slots, the backward above 16 384 / (17 C).
SHAPES_CONVMOD = [(32, 1, 144, 3, 1, False), (3, 5, 180, 15, 1, False), (1, 31, 256, 7, 1, True), (3, 32, 360, 16, 1, False), (3, 33, 132, 15, 1, True),
                  (32, 57, 144, 15, 1, False), (3, 100, 256, 15, 1, False), (32, 376, 180, 15, 1, False), (1, 376, 360, 7, 1, True), (3, 57, 144, 15, 2, False),
                  (32, 100, 256, 16, 2, True), (32, 33, 180, 3, 2, False), (1, 300, 1024, 7, 1, False), (1, 500, 1024, 16, 1, False), (1, 520, 1024, 3, 1, True)]


def convmod_inputs(mode, shape, i):
    """fp64 inputs of the fused convolution-module tests: u [B][T][2C], depthwise w [K][C] and bias, BatchNorm gamma / beta, da [B][To][C], running statistics.
    The taps are kept away from zero (0.3 (0.5 + |N|), random sign): a channel whose only live tap is ~0 has ~0 variance, and BatchNorm's backward through it is
    ill-conditioned in any fp32 evaluation -- that is a property of the input, not of a kernel; for the same reason the depthwise bias is small (0.1 N(0,1), as
    in a trained model), which keeps mean / std of the BatchNorm input at O(1) even where one tap is all a frame sees (T = 1)"""
    B, T, C, K, stride, causal = shape
    To = (T - 1) // stride + 1
    u, w, bias = dw_inputs(mode, (B, T, C, K, stride, causal), 40 + i)
    if mode != "exact":
        w = 0.3 * positive((K, C), 850 + i) * (1 if mode == "positive" else torch.sign(gauss((K, C), 860 + i)))
        bias = 0.1 * bias
    return dict(u=u, w=w, bias=bias, gamma=0.5 + gauss((C,), 800 + i).abs(), beta=gauss((C,), 810 + i), da=data(mode, (B, To, C), 820 + i),
                rmean=gauss((C,), 830 + i), rvar=positive((C,), 840 + i))
