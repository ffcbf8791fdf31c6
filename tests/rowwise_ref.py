"""Host-side pieces of the row-wise / element-wise kernel tests (tests/test_gpu_rowwise.py): fp64 references of the LayerNorm forward and dx kernels, the BatchNorm apply
passes, the InterCTC softmax, the patch-attention pool / un-pool, the stand-alone activations, the average pool and the strided casts of avec_amd/csrc/norm.hip; the
dropout hash of csrc/common.h in numpy.uint32 arithmetic; the per-element error scales, the case tables and the tolerances.  Pure torch / numpy on the host --
tests/test_rowwise_ref.py pins every reference to something independent of it, without a GPU.

Every formula below is written once, in the dtype of its arguments: fp64 arguments give the reference and its scale, fp32 arguments give the plain host fp32
evaluation whose own error sets the tolerance.  A formula returns {output name: (value, scale)}; `scale` is the same formula with every term taken by its
magnitude (a difference x - mu counts |x| + |mu|: it is formed in fp32 and its rounding error does not shrink with it), so that a small element is judged against
its own terms and not against the largest element of the tensor.

The judgement (ratio): |got - ref| <= TOL * scale + half a bf16 ulp of ref (bf16 outputs only) + 2^-126.  The last term is the flush of a subnormal fp32 result to
zero (swish(-100) = -3.7e-42 is one); the bf16 term is the exact half ulp 2^(floor(log2 |ref|) - 8) -- between 2^-9 |ref| (top of a binade) and 2^-8 |ref| (bottom):
a correctly rounded output can miss ref by that much and no more.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import colreduce_ref as C

EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126
DT = {"f32": 0, "bf16": 1}
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
as_dtype, pack_mask, gauss, int_tensor, exact_or_die = C.as_dtype, C.pack_mask, C.gauss, C.int_tensor, C.exact_or_die


def rd(x64, dtype):
    """the fp64 values of x64 once stored in `dtype` ("f32" / "bf16")"""
    return as_dtype(x64, dtype)[1]


# ---- the dropout hash of csrc/common.h ------------------------------------------------------------------------------------------------------------
U32, U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def mix32(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 in uint32 (wrapping) arithmetic; array in, array out"""
    x = np.array(x, dtype=np.uint32, ndmin=1, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def drop_key(rng, stream, p):
    """(k0, thr, scale) of a launch: rng = (seed, step) as the int64[2] device tensor holds them, stream the launch's rng_stream, p the probability as the float
    argument carries it.  thr = int(p * 65536 + 0.5) (fp32 arithmetic, capped at 65536); an element is dropped when its 16 hash bits are below thr, and the kept
    ones are scaled by 65536 / (65536 - thr) -- the reciprocal of the QUANTISED keep probability; p >= 1 drops everything with scale 0, p <= 0 is the identity.
    scale is the exact ratio (a Python float: fp64); the kernel holds it rounded to fp32."""
    if not p > 0:
        return 0, 0, 1.0
    seed, step = (int(v) & U64 for v in rng)
    s = (seed + 0x9E3779B97F4A7C15 * step) & U64
    a = int(mix32(((s & U32) + stream * 0x9E3779B9) & U32)[0])
    b = int(mix32(((s >> 32) ^ 0x85EBCA6B) & U32)[0])
    t = np.float32(np.float32(p) * np.float32(65536.0)) + np.float32(0.5)
    thr = 65536 if t >= 65536 else int(t)
    return a ^ b, thr, (0.0 if thr >= 65536 else 65536.0 / (65536 - thr))


def drop_hash(k0, pair):
    """the 32-bit hash of element pair `pair` (uint64 array): mix32(low32(pair) ^ k0 [^ high32(pair) * 0x9e3779b1 when the high word is not zero])"""
    pair = np.asarray(pair, dtype=np.uint64)
    x = (pair & np.uint64(U32)).astype(np.uint32) ^ np.uint32(k0)
    hi = (pair >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = x ^ np.where(hi != 0, hi * np.uint32(0x9E3779B1), np.uint32(0)).astype(np.uint32)
    return mix32(x)


def drop_keep(key, idx):
    """bool array: element idx survives.  Element idx takes the low (even idx) / high (odd idx) 16 bits of the hash of pair idx >> 1"""
    k0, thr, _ = key
    idx = np.asarray(idx, dtype=np.uint64)
    h = drop_hash(k0, idx >> np.uint64(1))
    v = np.where((idx & np.uint64(1)) != 0, h >> np.uint32(16), h & np.uint32(0xFFFF))
    return v.astype(np.int64) >= thr


def drop_mask(rng, stream, p, shape, index=None):
    """fp64 tensor of the factors (0 or scale) of the elements of a row-major tensor of `shape` (element index = flat position, or `index`, an int64 tensor)"""
    n = int(np.prod(shape))
    if not p > 0:
        return torch.ones(tuple(shape), dtype=torch.float64)
    key = drop_key(rng, stream, p)
    idx = np.arange(n, dtype=np.uint64) if index is None else index.reshape(-1).numpy().astype(np.uint64)
    return torch.from_numpy(drop_keep(key, idx).astype(np.float64) * key[2]).reshape(tuple(shape))


RNG = (0x1234567887654321, 77)             # {seed, step} of every GPU launch with dropout (the test's own int64[2] tensor)
RNG_STREAM = 5


# ---- elementary functions in the dtype of the argument ---------------------------------------------------------------------------------------------
LOG2E32 = torch.tensor(math.log2(math.e), dtype=torch.float32)


def exp_(x):
    """exp in fp64; in fp32 the fast intrinsic's definition exp2(fl32(x * log2(e))): the product is rounded to fp32 before the exponential, an argument error
    that grows with |x| (a model of the instruction, not taken from a GPU run)"""
    return torch.exp2(x * LOG2E32) if x.dtype == torch.float32 else torch.exp(x)


def sigmoid_(x):
    return 1 / (1 + exp_(-x))


def swish_(x):
    return x * sigmoid_(x)


def dswish_(x):
    s = sigmoid_(x)
    return s * (1 + x * (1 - s))


def sig_mag(x):
    """scale of sigmoid(x): itself plus its sensitivity to the rounded exponent argument, sigma (1 - sigma) |x|"""
    s = torch.sigmoid(x)
    return s * (1 + x.abs() * (1 - s))


def swish_mag(x):
    return x.abs() * sig_mag(x)


def dswish_mag(x):
    """scale of swish'(x) = s (1 + x (1 - s)): an error of s enters through both factors, at most (1 + |x|) times"""
    return sig_mag(x) * (1 + x.abs())


def _k(v, like):
    return torch.as_tensor(v, dtype=like.dtype)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, g, b, eps, x_mag=None):
    """y = (x - mean) / sqrt(var + eps) * g + b over the last dim, biased variance about the mean (two-pass by definition).  x_mag: the scale of x itself when x is a
    computed quantity (the second norm of layernorm_fwd2)"""
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    rs = 1 / torch.sqrt(var + _k(eps, x))
    y = d * rs * g + b
    xm = x.abs() if x_mag is None else x_mag
    mu_s = xm.mean(-1, keepdim=True)
    ax = xm + mu_s
    # var = mean(d^2): one rounding of d (|x| + |mean| units) moves d^2 by 2 |d| of it; rstd moves by rstd^3 / 2 times the variance's error
    rs_s = rs * (1 + rs * rs * (d.abs() * ax).mean(-1, keepdim=True))
    y_s = ax * (rs if x_mag is None else rs_s) * g.abs() + b.abs()
    return {"y": (y, y_s), "mean": (mu[..., 0], mu_s[..., 0]), "rstd": (rs[..., 0], rs_s[..., 0])}


def layernorm_bwd(dy, x, mu, rs, g, dres=None, mask=None, alpha=1.0, dy_mag=None):
    """dx = rstd (t - mean(t) - xhat mean(t xhat)) (+ dres), t = dy g, xhat = (x - mean) rstd, from the SAVED mean / rstd [M]; prep = alpha * mask * dx"""
    mu, rs = mu.unsqueeze(-1), rs.unsqueeze(-1)
    xh = (x - mu) * rs
    t = dy * g
    dx = rs * (t - t.mean(-1, keepdim=True) - xh * (t * xh).mean(-1, keepdim=True))
    xm = (x.abs() + mu.abs()) * rs.abs()
    tm = (dy.abs() if dy_mag is None else dy_mag) * g.abs()
    dx_s = rs.abs() * (tm + tm.mean(-1, keepdim=True) + xm * (tm * xm).mean(-1, keepdim=True))
    if dres is not None:
        dx, dx_s = dx + dres, dx_s + dres.abs()
    out = {"dx": (dx, dx_s)}
    if mask is not None:
        a = _k(alpha, x)
        out["prep"] = (a * mask * dx, a.abs() * mask * dx_s)
    return out


def layernorm_fwd2(x, g1, b1, eps1, g2, b2, eps2):
    """y1 = LN1(x), h2 = LN2(y1)"""
    a = layernorm_fwd(x, g1, b1, eps1)
    b = layernorm_fwd(a["y"][0], g2, b2, eps2, x_mag=a["y"][1])
    return {"y1": a["y"], "mean1": a["mean"], "rstd1": a["rstd"], "h2": b["y"], "mean2": b["mean"], "rstd2": b["rstd"]}


def layernorm_bwd2(dy2, x2, mu2, rs2, g2, dres2, x1, mu1, rs1, g1, mask=None, alpha=1.0):
    """the gradient of LN2(LN1(x1)) (+ a residual branch dres2 on LN1's output): dx2 w.r.t. LN2's input, dx1 w.r.t. LN1's input, prep from dx1"""
    a = layernorm_bwd(dy2, x2, mu2, rs2, g2, dres2)
    b = layernorm_bwd(a["dx"][0], x1, mu1, rs1, g1, None, mask, alpha, dy_mag=a["dx"][1])
    out = {"dx2": a["dx"], "dx1": b["dx"]}
    if mask is not None:
        out["prep"] = b["prep"]
    return out


def grad_prep(dout, mask, alpha):
    a = _k(alpha, dout)
    v = a * mask * dout
    return {"dacc": (v, v.abs())}


# ---- BatchNorm apply ------------------------------------------------------------------------------------------------------------------------------
def bn_pre(y, ss, res=None, res_ss=None):
    """(pre-activation, its scale): y scale + shift (+ res | + res rscale + rshift); ss [4][C] = scale | shift | mean | rstd"""
    pre, mag = y * ss[0] + ss[1], (y * ss[0]).abs() + ss[1].abs()
    if res is not None and res_ss is not None:
        pre, mag = pre + res * res_ss[0] + res_ss[1], mag + (res * res_ss[0]).abs() + res_ss[1].abs()
    elif res is not None:
        pre, mag = pre + res, mag + res.abs()
    return pre, mag


def bn_apply_fwd(y, ss, act, res=None, res_ss=None):
    """out = act(pre); act 0 none, 1 Swish, 2 ReLU.  The scale of swish(pre) is its own plus |swish'| (<= the magnitude form of swish') times the pre-activation's"""
    pre, mag = bn_pre(y, ss, res, res_ss)
    if act == 1:
        return {"out": (swish_(pre), swish_mag(pre) + C.dswish_mag(pre) * mag), "pre": (pre, mag)}
    if act == 2:
        return {"out": (pre.clamp_min(0), mag), "pre": (pre, mag)}
    return {"out": (pre, mag), "pre": (pre, mag)}


def bn_bwd_apply(dout, y, ss, gamma, dstats, count, act, out=None, mask=None, keep=None):
    """dy = gamma rstd (d - s1 / n - xhat s2 / n), dres = d, d = dout act'(.): act 1 Swish' of the recomputed pre-activation; act 2 by the saved out > 0, by the
    mask bits, else by the recomputed pre-activation > 0 (keep: that decision taken once, in fp64, and shared with the fp32 evaluation); dstats = (s1 | s2)"""
    Cn = y.shape[-1]
    n = _k(count, y)
    if act == 1:
        pre, pm = bn_pre(y, ss)
        d, dm = dout * dswish_(pre), dout.abs() * (dswish_mag(pre) + 0.5 * pm)
    elif act == 2:
        k = keep if keep is not None else (mask if mask is not None else ((out > 0) if out is not None else (bn_pre(y, ss)[0] > 0)))
        d = dout * k.to(dout.dtype)
        dm = d.abs()
    else:
        d, dm = dout, dout.abs()
    xh, xm = (y - ss[2]) * ss[3], (y.abs() + ss[2].abs()) * ss[3].abs()
    s1, s2 = dstats[:Cn], dstats[Cn:]
    A = gamma * ss[3]
    return {"dy": (A * (d - s1 / n - xh * s2 / n), A.abs() * (dm + s1.abs() / n + xm * s2.abs() / n)), "dres": (d, dm)}


# ---- softmax --------------------------------------------------------------------------------------------------------------------------------------
def _softmax_parts(x):
    a = x - x.amax(-1, keepdim=True)
    e = exp_(a)
    p = e / e.sum(-1, keepdim=True)
    am = torch.where(torch.isfinite(a), a.abs(), torch.zeros_like(a))
    w = 1 + am                                               # the exponent's argument is rounded: |a| roundings of e
    return p, p * (w + (p * w).sum(-1, keepdim=True))


def softmax_fwd(x):
    p, ps = _softmax_parts(x)
    return {"p": (p, ps)}


def softmax_bwd(dp, x, dadd=None):
    """dx = p (dp - sum(p dp)) (+ dadd)"""
    p, ps = _softmax_parts(x)
    g = p * (dp - (p * dp).sum(-1, keepdim=True))
    gs = ps * (dp.abs() + (ps * dp.abs()).sum(-1, keepdim=True))
    if dadd is not None:
        g, gs = g + dadd, gs + dadd.abs()
    return {"dx": (g, gs)}


# ---- stand-alone activations -----------------------------------------------------------------------------------------------------------------------
def act_fwd(act, x):
    """1 Swish, 2 ReLU, 3 GLU over the last dim ([rows][2C] -> [rows][C], a sigmoid(b))"""
    if act == 1:
        return {"out": (swish_(x), swish_mag(x))}
    if act == 2:
        return {"out": (x.clamp_min(0), x.abs())}
    a, b = x.chunk(2, -1)
    return {"out": (a * sigmoid_(b), a.abs() * sig_mag(b))}


def act_bwd(act, x, dy):
    if act == 1:
        return {"out": (dy * dswish_(x), dy.abs() * dswish_mag(x))}
    if act == 2:
        v = dy * (x > 0).to(dy.dtype)
        return {"out": (v, v.abs())}
    a, b = x.chunk(2, -1)
    s = sigmoid_(b)
    # 1 - s is formed from the rounded s: its absolute error is that of s, so the product s (1 - s) carries sig_mag(b) whole
    return {"out": (torch.cat([dy * s, dy * a * s * (1 - s)], -1), torch.cat([dy.abs() * sig_mag(b), (dy * a).abs() * sig_mag(b)], -1))}


# ---- patch pool / un-pool, average pool, strided rows ------------------------------------------------------------------------------------------------
def _pool(x, P):
    B, T, D = x.shape
    Tp = (T + P - 1) // P
    return F.pad(x, (0, 0, 0, Tp * P - T)).view(B, Tp, P, D).sum(2)


def patch_pool_fwd(x, P):
    """zero padding to a multiple of P, mean over P frames with divisor P (the short last patch included): [B][T][D] -> [B][ceil(T / P)][D]"""
    return {"y": (_pool(x, P) / P, _pool(x.abs(), P) / P)}


def patch_pool_bwd(dy, T, P):
    v = dy.repeat_interleave(P, dim=1)[:, :T] / P
    return {"dx": (v, v.abs())}


def patch_unpool_add(o, res, mask, P):
    """out = res + mask * (nearest up-sampling of o by P, sliced to T); the mask is indexed by the UN-pooled element (b T + t) D + c"""
    T = res.shape[1]
    u = o.repeat_interleave(P, dim=1)[:, :T] * mask
    return {"out": (res + u, res.abs() + u.abs())}


def patch_unpool_bwd(dout, mask, P):
    return {"dob": (_pool(dout * mask, P), _pool((dout * mask).abs(), P))}


def avgpool_fwd(x):
    return {"y": (x.mean(1), x.abs().mean(1))}


def avgpool_bwd(dy, HW):
    v = (dy / HW).unsqueeze(1).expand(-1, HW, -1)
    return {"dx": (v, v.abs())}


def strided_rows_add(dx, src, step):
    """dx[b][to * step] += src[b][to]; every other row of dx unchanged"""
    out = dx.clone()
    To = src.shape[1]
    out[:, 0:(To - 1) * step + 1:step] += src
    return out


# ---- the judgement -----------------------------------------------------------------------------------------------------------------------------------
def half_ulp_bf16(v):
    """half the spacing of the bf16 numbers around |v| (8 significant bits): 2^(floor(log2 |v|) - 8); 0 at 0"""
    v = v.double().abs()
    e = torch.floor(torch.log2(v.clamp_min(1e-300)))
    return torch.where(v > 0, torch.exp2(e - 8), torch.zeros_like(v))


def ratio(got, ref, scale, out_dtype="f32"):
    """per element: (|got - ref| - half a bf16 ulp (bf16 outputs) - 2^-126)+ / scale.  NaN or inf in `got` where the reference is finite never passes; an element
    without terms (scale 0) must be exact"""
    got, ref, scale = got.double().reshape(-1), ref.double().reshape(-1), scale.double().reshape(-1)
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    err = (got - ref).abs() - TINY32
    if out_dtype == "bf16":
        err = err - half_ulp_bf16(torch.maximum(ref.abs(), got.abs()))
    err = err.clamp_min(0)
    r = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))


def worst(got, ref, scale, out_dtype="f32"):
    return float(ratio(got, ref, scale, out_dtype).max())


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
def coef(n, k=0, positive=False):
    """a per-channel coefficient vector whose entries differ clearly in sign and magnitude from channel to channel: |v_c| = 0.4 + 0.17 ((7 c + 3 k) mod 13),
    negative where (5 c + k) mod 3 == 0.  v_c != v_(c+4), v_(c+8): an index that is off by one vector of channels shows"""
    c = torch.arange(n)
    v = 0.4 + 0.17 * ((7 * c + 3 * k) % 13).double()
    return v if positive else v * torch.where((5 * c + k) % 3 == 0, -1.0, 1.0)


def icoef(n, k=0, zero_ok=True):
    """integer coefficients in [-3, 3] varying from channel to channel; channel 0 of k = 0 is 1 (zero_ok False) resp. 0 (zero_ok True) for the planted elements"""
    c = torch.arange(n)
    if zero_ok:
        return (((5 * c + 3 * k) % 7) - 3).double() * (c > 0)
    v = ((5 * c + k) % 6).double()
    return torch.where(v < 3, v + 1, v - 6)                   # k = 0: 1 -1 -2 -3 3 2 ...


LN_M = [1, 5, 9]
LN_FWD_D = [4, 180, 252, 256, 260, 360, 512, 516, 1536, 2052]
LN_EPS = [1e-6, 1e-2]
LN_BWD_D = [4, 180, 256, 260, 512, 516, 1024, 1536]
LN_BWD_REJECT = [1540, 6]
LN2_M, LN2_D, LN2_REJECT = [1, 5], [4, 180, 256, 260, 512], 516
LNP_M, LNP_D = [1, 17, 4100], [180, 516]
DROP_P = [0.0, 0.1, 0.5, 1.0]
ALPHAS = [1.0, 0.5]
GP_M, GP_N, GP_PAD = [1, 3, 67], [4, 180, 256], [0, 8]
BN4 = [(1, 4), (65, 12), (7, 180)]
BN8 = [(1, 8), (343, 24), (31, 360), (33, 64), (3, 512)]
BN8_CAP_FWD, BN8_CAP_BWD = 8192, 3072
BN_CAP_C = 64
# C = 40: C/8 = 5 = q and neither cap is a multiple of 5, so above the cap the grid is rounded down (8190 / 3070 blocks).  Below the cap an unrounded grid covers the
# tensor in one trip and no thread ever strides, so this is the only place where the rounding decides which channels a thread meets
BN_CAP_CQ = 40


def bn_cap_rows(cap, Cn):
    """rows above a grid cap: more than 2 x cap x 256 chunks, so that a thread's second in-flight chunk AND a second trip of its loop (with a short tail) both run"""
    return -(-2 * cap * 256 * 8 // Cn) + 37


BN_CAP_M_FWD, BN_CAP_M_BWD = bn_cap_rows(BN8_CAP_FWD, BN_CAP_C), bn_cap_rows(BN8_CAP_BWD, BN_CAP_C)
BN_CAP_FWD_CASES = [(bn_cap_rows(BN8_CAP_FWD, Cn), Cn) for Cn in (BN_CAP_C, BN_CAP_CQ)]
BN_CAP_BWD_CASES = [(bn_cap_rows(BN8_CAP_BWD, Cn), Cn) for Cn in (BN_CAP_C, BN_CAP_CQ)]
SM_M, SM_V = [1, 5], [1, 2, 63, 64, 65, 256, 257]
ACT_ROWS, ACT_C = [1, 3], [1, 5, 257]
PATCH = [(2, 7, 3), (1, 8, 4), (3, 1, 3), (2, 9, 1)]
PATCH_D = [4, 180]
AVGPOOL = [(1, 1, 4), (3, 9, 12), (2, 16, 512)]
STRIDED = [(2, 7, 4, 2), (1, 5, 5, 1), (3, 9, 3, 4)]
CAST_N = [4, 180]
DROPOUT_N = [1, 2, 255, 257, (1 << 20) + 3]
EXTREMES = [30.0, -30.0, 100.0, -100.0]


def bn8_blocks(n8, Cn, cap):
    """norm.hip bn8_blocks (used ONLY to document which shapes reach which path): the grid, rounded down to a multiple of q = (C/8) / gcd(C/8, 256)"""
    c8 = Cn // 8
    q = c8 // math.gcd(c8, 256)
    nb = min((n8 + 255) // 256, cap)
    return max(nb // q * q, q), q


def ln_rows(M, D, k=0):
    """[M][D] fp64, rounded to fp32: row r is, by (r + k) mod 4, Gaussian; mean 1000 with unit variance; constant; Gaussian scaled by 1e-3"""
    x = gauss((M, D), 100 + 7 * D + M + k)
    for r in range(M):
        kind = (r + k) % 4
        if kind == 1:
            x[r] += 1000
        elif kind == 2:
            x[r] = 0.75 * (1 + r)
        elif kind == 3:
            x[r] *= 1e-3
    return rd(x, "f32")


def ln_fwd_cases():
    for i, D in enumerate(LN_FWD_D):
        for M in LN_M:
            for eps in LN_EPS:
                yield (M, D, eps), dict(x=ln_rows(M, D, i), g=rd(coef(D, 1), "f32"), b=rd(coef(D, 2), "f32"), eps=eps)


def ln_saved(x, eps):
    """the statistics a forward pass saved: fp64 definition, rounded to fp32"""
    r = layernorm_fwd(x, torch.ones(x.shape[-1], dtype=torch.float64), torch.zeros(x.shape[-1], dtype=torch.float64), eps)
    return rd(r["mean"][0], "f32"), rd(r["rstd"][0], "f32")


def ln_bwd_inputs(M, D, gdtype, with_dres, k=0):
    """rows: Gaussian, and every third one with mean 3"""
    x = gauss((M, D), 300 + D + M + k)
    x[1::3] += 3
    x = rd(x, "f32")
    mu, rs = ln_saved(x, 1e-6)
    return dict(dy=rd(gauss((M, D), 400 + D + M + k), gdtype), x=x, mu=mu, rs=rs, g=rd(coef(D, 3), "f32"),
                dres=rd(gauss((M, D), 500 + D + M + k), "f32") if with_dres else None)


def ln_bwd_cases(Ms=None, Ds=None):
    for D in (Ds or LN_BWD_D):
        for M in (Ms or LN_M):
            for gdtype in ("f32", "bf16"):
                for with_dres in (False, True):
                    yield (M, D, gdtype, with_dres), ln_bwd_inputs(M, D, gdtype, with_dres)


def ln2_inputs(M, D, gdtype, with_dres):
    """forward inputs and what the backward is given: x2 = y1 and both pairs of statistics as a forward pass in fp64 leaves them in fp32 memory"""
    x = ln_rows(M, D, 0) if M > 1 else rd(gauss((M, D), 600 + D), "f32")
    f = dict(x=x, g1=rd(coef(D, 4), "f32"), b1=rd(coef(D, 5), "f32"), eps1=1e-6, g2=rd(coef(D, 6), "f32"), b2=rd(coef(D, 7), "f32"), eps2=1e-2)
    xb = gauss((M, D), 650 + D + M)
    xb[1::3] += 3
    xb = rd(xb, "f32")
    r = layernorm_fwd2(xb, f["g1"], f["b1"], f["eps1"], f["g2"], f["b2"], f["eps2"])
    b = dict(dy2=rd(gauss((M, D), 700 + D + M), gdtype), x2=rd(r["y1"][0], "f32"), mu2=rd(r["mean2"][0], "f32"), rs2=rd(r["rstd2"][0], "f32"), g2=f["g2"],
             dres2=rd(gauss((M, D), 750 + D + M), "f32") if with_dres else None, x1=xb, mu1=rd(r["mean1"][0], "f32"), rs1=rd(r["rstd1"][0], "f32"), g1=f["g1"])
    return f, b


def bn_ss(Cn, k=0, exact=False):
    """[4][C] scale | shift | mean | rstd"""
    if exact:
        c = torch.arange(Cn)
        sh = icoef(Cn, k, True)
        sh[0] = -0.0                                           # with y = -0 and scale 1 the pre-activation is -0 itself (-0 * 1 + -0); with y = +0 it is +0
        return torch.stack([icoef(Cn, k, False), sh, ((c + k) % 3).double() - 1, torch.tensor([0.5, 1.0], dtype=torch.float64)[(c // 2 + k) % 2]])
    return rd(torch.stack([coef(Cn, k), coef(Cn, k + 1), 0.5 * coef(Cn, k + 2), coef(Cn, k + 3, positive=True)]), "f32")


def plant_pre(y, ss, dtype, res=None):
    """plants the pre-activations EXTREMES (as far as the storage dtype resolves them) into row 0 of y, channels 1..4 (mod C)"""
    Cn = y.shape[-1]
    for j, v in enumerate(EXTREMES):
        c = (1 + j) % Cn
        if j < Cn:
            y[0, c] = (v - ss[1, c] - (res[0, c] if res is not None else 0)) / ss[0, c]
    return rd(y, dtype)


def bn_fwd_inputs(M, Cn, dtype, act, with_res, k=0):
    ss = bn_ss(Cn, k)
    res = rd(gauss((M, Cn), 820 + M + Cn), dtype) if with_res else None
    y = gauss((M, Cn), 800 + M + Cn) * (2.5 if act == 1 else 1.0)           # Swish: pre-activations within about [-8, 8]
    if act == 1:
        y = (y * ss[0] + ss[1]).clamp(-8, 8).sub(ss[1]).div(ss[0]) - (0 if res is None else res / ss[0])
        y = plant_pre(y, ss, dtype, res)
    return dict(y=rd(y, dtype), ss=ss, act=act, res=res)


def bn_fwd_exact(M, Cn, with_res, seed=0, res_ss=False):
    """integers throughout: y, res in [-3, 3], scale in +-{1, 2, 3}, shift in [-3, 3] (channel 0: scale 1, shift 0): |pre| <= 3 * 3 + 3 + 3 * 3 + 3 = 24, a bf16
    number; row 0 channel 0 holds +0, row 1 (if any) -0, row 2 the smallest positive normal number (2^-126 in both dtypes)"""
    y = int_tensor((M, Cn), -3, 3, 900 + seed)
    res = int_tensor((M, Cn), -3, 3, 901 + seed) if with_res else None
    y[0, 0] = 0.0
    if res is not None:
        res[:3, 0] = 0.0
    if M > 1:
        y[1, 0] = -0.0
    if M > 2:
        y[2, 0] = TINY32
    d = dict(y=y, ss=bn_ss(Cn, 0, exact=True), act=2, res=res)
    if res_ss:
        d["res_ss"] = torch.stack([icoef(Cn, 2, False), icoef(Cn, 1, True)])
    return d


def bn_bwd_inputs(M, Cn, dtype, act, k=0):
    ss = bn_ss(Cn, k)
    y = gauss((M, Cn), 840 + M + Cn)
    if act == 1:
        y = plant_pre(y * 2, ss, dtype)
    if act == 2:                # ReLU by the recomputed pre-activation: keep it clear of zero (by 1/2 where it came within 1e-3 of its terms), so that the decision is no matter of rounding
        pre, mag = bn_pre(rd(y, dtype), ss)
        y = torch.where(pre.abs() <= 1e-3 * mag, y + 0.5 / ss[0], y)
    count = float(M)
    return dict(dout=rd(gauss((M, Cn), 860 + M + Cn), dtype), y=rd(y, dtype), ss=ss, gamma=rd(coef(Cn, k + 4), "f32"),
                dstats=rd(torch.cat([coef(Cn, k + 5), coef(Cn, k + 6)]) * count * 0.05, "f32"), count=count, act=act)


def bn_bwd_exact(M, Cn, seed=0):
    """dout, y in [-2, 2], mean in {-1, 0, 1}, rstd in {1/2, 1}, gamma in {1, 2}, dstats multiples of count = 4 in [-4, 4]: every intermediate of
    gamma rstd (d - s1/4 - (y - mean) rstd s2/4) is a multiple of 1/4 below 12 -- an fp32 AND a bf16 number; ReLU by the mask of a integer forward pass"""
    c = torch.arange(Cn)
    ss = bn_ss(Cn, 0, exact=True)
    return dict(dout=int_tensor((M, Cn), -2, 2, 950 + seed), y=int_tensor((M, Cn), -2, 2, 951 + seed), ss=ss, gamma=torch.tensor([1.0, 2.0], dtype=torch.float64)[(c // 3) % 2],
                dstats=4 * torch.cat([((c % 3) - 1).double(), (((c // 2) % 3) - 1).double()]), count=4.0, act=2)


def softmax_rows(M, V):
    """rows by r mod 5: Gaussian; one dominant logit (+40); shifted by +1e4 (r = 2) / -1e4 (r = 7, ...); all equal; one -inf entry"""
    x = gauss((M, V), 1000 + V + M) * 2
    for r in range(M):
        kind = (r + V) % 5
        if kind == 1:
            x[r, (3 * r + 1) % V] += 40
        elif kind == 2:
            x[r] += 1e4 if r % 2 == 0 else -1e4
        elif kind == 3:
            x[r] = 1.25
        elif kind == 4 and V > 1:
            x[r, (r + 2) % V] = -math.inf
    return rd(x, "f32")


def act_inputs(rows, Cn, act):
    W = 2 * Cn if act == 3 else Cn
    x = gauss((rows, W), 1100 + rows + Cn + act) * 3
    flat = x.view(-1)
    for j, v in enumerate(EXTREMES):
        if j < flat.numel():
            flat[-1 - j] = v                                    # (GLU: these land in the gate half of the last row)
    if act == 2:
        flat[0] = 0.0
        if flat.numel() > 5:
            flat[5] = -0.0
    return rd(x, "f32"), rd(gauss((rows, Cn), 1150 + rows + Cn + act), "f32")


# ---- the plain fp32 host evaluation and the tolerances ----------------------------------------------------------------------------------------------------
def to32(v):
    if torch.is_tensor(v) and v.dtype == torch.float64:
        return v.float()
    return v


def host_fp32_ratio(fn, kwargs, names=None, out_dtype="f32"):
    """worst per-element ratio of fn evaluated in fp32 (torch fp32 ops and sums) against fn in fp64 on the same (already rounded) inputs"""
    ref = fn(**kwargs)
    got = fn(**{k: to32(v) for k, v in kwargs.items()})
    return max(worst(got[n][0], ref[n][0], ref[n][1]) for n in (names or ref) if n != "pre")


def measure_host_fp32():
    """{formula: worst per-element ratio of the fp32 host evaluation over that formula's case table}"""
    out = {}

    def upd(k, v):
        out[k] = max(out.get(k, 0.0), v)
    for _, kw in ln_fwd_cases():
        upd("layernorm_fwd", host_fp32_ratio(layernorm_fwd, kw))
    for M in LN2_M:
        for D in LN2_D:
            for gd in ("f32", "bf16"):
                f, b = ln2_inputs(M, D, gd, True)
                upd("layernorm_fwd2", host_fp32_ratio(layernorm_fwd2, f))
                upd("layernorm_bwd2", host_fp32_ratio(layernorm_bwd2, dict(b, mask=torch.ones(M, D, dtype=torch.float64), alpha=0.5)))
    for _, kw in list(ln_bwd_cases()) + list(ln_bwd_cases(LNP_M[:2], LNP_D)):
        upd("layernorm_bwd", host_fp32_ratio(layernorm_bwd, dict(kw, mask=drop_mask(RNG, RNG_STREAM, 0.1, kw["x"].shape), alpha=0.5)))
    for dt in ("f32", "bf16"):
        for M, Cn in BN4 + BN8:
            for act in (0, 1, 2):
                for with_res in (False, True):
                    kw = bn_fwd_inputs(M, Cn, dt, act, with_res)
                    upd("bn_apply_fwd", host_fp32_ratio(bn_apply_fwd, kw, ["out"]))
                kw = bn_bwd_inputs(M, Cn, dt, act)
                if act == 2:
                    kw["keep"] = bn_pre(kw["y"], kw["ss"])[0] > 0
                upd("bn_bwd_apply", host_fp32_ratio(bn_bwd_apply, kw))
    for M in SM_M:
        for V in SM_V:
            x = softmax_rows(M, V)
            upd("softmax_fwd", host_fp32_ratio(softmax_fwd, dict(x=x)))
            for dt in ("f32", "bf16"):
                upd("softmax_bwd", host_fp32_ratio(softmax_bwd, dict(dp=rd(gauss((M, V), 1050 + V), dt), x=x, dadd=rd(gauss((M, V), 1060 + V), "f32"))))
    for rows in ACT_ROWS:
        for Cn in ACT_C:
            for act in (1, 3):
                x, dy = act_inputs(rows, Cn, act)
                upd("act", host_fp32_ratio(lambda x, dy, act=act: act_fwd(act, x), dict(x=x, dy=dy)))
                upd("act", host_fp32_ratio(lambda x, dy, act=act: act_bwd(act, x, dy), dict(x=x, dy=dy)))
    for dt in ("f32", "bf16"):
        for B, T, P in PATCH:
            for D in PATCH_D:
                Tp = (T + P - 1) // P
                x, o = rd(gauss((B, T, D), 1200 + T + D), dt), rd(gauss((B, Tp, D), 1210 + T + D), dt)
                res = rd(gauss((B, T, D), 1220 + T + D), "f32")
                m = drop_mask(RNG, RNG_STREAM, 0.1, (B, T, D))
                upd("patch", host_fp32_ratio(patch_pool_fwd, dict(x=x, P=P)))
                upd("patch", host_fp32_ratio(patch_pool_bwd, dict(dy=o, T=T, P=P)))
                upd("patch", host_fp32_ratio(patch_unpool_add, dict(o=o, res=res, mask=m, P=P)))
                upd("patch", host_fp32_ratio(patch_unpool_bwd, dict(dout=res, mask=m, P=P)))
        for N, HW, Cn in AVGPOOL:
            upd("avgpool", host_fp32_ratio(avgpool_fwd, dict(x=rd(gauss((N, HW, Cn), 1300 + HW), dt))))
            upd("avgpool", host_fp32_ratio(avgpool_bwd, dict(dy=rd(gauss((N, Cn), 1310 + HW), dt), HW=HW)))
    for M in GP_M:
        for N in GP_N:
            upd("grad_prep", host_fp32_ratio(grad_prep, dict(dout=rd(gauss((M, N), 1400 + M + N), "f32"), mask=drop_mask(RNG, RNG_STREAM, 0.1, (M, N)), alpha=0.5)))
    return out


# Per-element tolerance: |got - ref| <= TOL[formula] * scale (+ the bf16 and subnormal terms of ratio()).  Each is 8 x the worst ratio that the plain fp32 HOST
# evaluation of the same formula reaches over the case table above -- the project's margin for fp32 kernels: wave-shuffle summation order, FMA contraction, rsqrtf, and
# the 1-ulp v_rcp_f32 / v_exp_f32 behind the sigmoid.  Measured 2026-10-19 with torch 2 on the CPU (measure_host_fp32; tests/test_rowwise_ref.py re-measures):
#     formula              worst host fp32 ratio      x 8
HOST_FP32_WORST = {
    "layernorm_fwd":      1.62e-7,               # 1.3e-06   (y, mean, rstd)
    "layernorm_fwd2":     1.23e-7,               # 9.8e-07   (y1, h2 and both pairs of statistics)
    "layernorm_bwd":      1.86e-7,               # 1.5e-06   (dx and prep; avec_layernorm_bwd with and without dgamma, avec_layernorm_bwd_prep)
    "layernorm_bwd2":     1.07e-7,               # 8.6e-07   (dx2, dx1, prep)
    "grad_prep":          8.38e-8,               # 6.7e-07   (dacc)
    "bn_apply_fwd":       1.32e-7,               # 1.1e-06   (act none / Swish / ReLU, with and without residual; avec_bn_apply_fwd_mask shares it)
    "bn_bwd_apply":       1.99e-7,               # 1.6e-06   (dy and dres; the mask variant shares it)
    "softmax_fwd":        9.49e-8,               # 7.6e-07   
    "softmax_bwd":        5.75e-8,               # 4.6e-07   
    "act":                1.81e-7,               # 1.4e-06   (avec_act_f32: Swish and GLU, forward and backward (ReLU is exact))
    "patch":              1.57e-7,               # 1.3e-06   (pool forward / backward, un-pool add / backward)
    "avgpool":            1.32e-7,               # 1.1e-06   (forward and backward)
}
TOL = {k: 8 * v for k, v in HOST_FP32_WORST.items()}
