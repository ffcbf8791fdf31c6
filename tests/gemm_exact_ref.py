"""Integer operands, plain float64 references and the case tables of the PLAIN (non-convolution) products of csrc/gemm.hip: avec_gemm_nt in plain mode,
avec_gemm_nt_fp8 and the avec_gemm_tn family (tests/test_gpu_gemm_exact.py runs them on the GPU, tests/test_gemm_exact_ref.py checks this file without one).

The idea is that of tests/conv_exact_ref.py, whose operand generators, check_exact() and assert_exact() are used here: activations and gradients in {-2 .. 2}, weights
in {-1, 0, 1}, bias / residual / initial values in integers or halves, alpha 1 or 0.5, dropout at p = 0.5 (kept scale exactly 2).  Every product, every fp32 partial sum
in any order (split-K atomics, replicated statistics, column sums) and every bf16 result is then an exactly representable number and a kernel has to reproduce the
reference at EVERY element.  Everything here is torch on the CPU in float64 and calls no project code.

The epilogue order (nt_epilogue / plain_epilogue_tr, csrc/gemm_dev.h):
    v = acc + bias;  out_pre = v;  v = act(v);  v *= dropmask[row * N + col];  v *= act'(z);  colsum += v;  stats += (v, v * v);  out = alpha * v + res
The transcendental activations (Swish, GELU, dact = 1) cannot be bit-exact: there out_pre and the set of written elements stay exact and the activated output is judged
per element against the float64 function of the exact pre-activation (rowwise_ref.ratio, TOL below).
"""
import math
import zlib

import torch

from tests.conv_exact_ref import F64, LIMITS, activations, assert_exact, check_exact, column_stats, draw_ints, nonzero_ints, weights      # noqa: F401 (re-exported)
from tests import rowwise_ref as RW
from tests.rowwise_ref import RNG, RNG_STREAM, drop_mask

NAN = float("nan")
DROP_P = 0.5                    # thr = 32768: an element is kept when its 16 hash bits are >= 32768, the kept scale is 65536 / 32768 = 2 exactly


def _gen(cid):
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def odd_halves(gen, shape, amax=2):
    """odd multiples of 1/2 in [-(amax + 1/2), amax + 1/2]: never zero, and integer + odd half is never zero either (the bias of the short-K cases)"""
    return (2 * torch.randint(-amax - 1, amax + 1, tuple(shape), generator=gen) + 1).to(F64) / 2


def plant_zeros(z):
    """+0 and -0 at fixed places of a saved activation: the kernels pass the gradient where z > 0, not >= 0"""
    z.view(-1)[3::7] = 0.0
    z.view(-1)[::7] = -0.0
    return z


# ---- transcendental activations: float64 value and per-element scale ----------------------------------------------------------------------------
def gelu_(x):
    """0.5 x (1 + erf(x / sqrt 2)) in the dtype of x (the formula of geluf_, csrc/common.h)"""
    return 0.5 * x * (1 + torch.erf(x * torch.as_tensor(math.sqrt(0.5), dtype=x.dtype)))


def gelu_mag(x):
    """both terms of the bracket by their magnitude: for x << 0 the bracket cancels and keeps the absolute error of erf"""
    return 0.5 * x.abs() * (1 + torch.erf(x.abs() * math.sqrt(0.5)))


def act_value(act, x):
    """(value, scale) of act(x): 1 Swish, 3 GELU"""
    return (RW.swish_(x), RW.swish_mag(x)) if act == 1 else (gelu_(x), gelu_mag(x))


# Per-element tolerances of the transcendental outputs, |got - ref| <= TOL * scale (+ half a bf16 ulp for bf16 outputs, rowwise_ref.ratio).  Swish and dswish go through
# the device functions of avec_act_f32 (swishf_ / dswishf_): rowwise_ref.TOL["act"].  GELU (erff) follows the same rule, 8 x the worst ratio of the plain host fp32
# evaluation against float64, measured over the pre-activations of the GELU cases below (measure_gelu_host_fp32(); tests/test_gemm_exact_ref.py re-measures):
#     worst host fp32 ratio 3.85e-8  ->  x 8 = 3.1e-7   (measured 2026-10-21 with torch 2 on the CPU)
GELU_HOST_FP32_WORST = 3.85e-8
TOL = {"swish": RW.TOL["act"], "dswish": RW.TOL["act"], "gelu": 8 * GELU_HOST_FP32_WORST}


# ---- avec_gemm_nt, plain mode ------------------------------------------------------------------------------------------------------------------------
_NT_DEF = dict(dtype="bf16", a_f32=False, lda=None, ldw=None, off_a=0, off_w=0, step=None, bias=None, act=0, drop=False, res=None, alpha=1.0, out_f32=False,
               out_pre=False, dact=0, colsum=False, stats=False, ldo=None, ldpre=None, ldres=None, ldz=None, off_out=0, alias=False, da=1.0, dw=1.0)


def _nt(cid, kernel, M, N, K, **kw):
    """bias: None / "int" / "half" (odd halves) / "mixed" (integers and halves); res: None / "bf16" / "f32"; step: (rows_out, rows_in, step) of the strided row source; off_*: elements behind an aligned address;
    alias: `out` is the bf16 residual buffer itself; da / dw: densities of A and W"""
    assert set(kw) <= set(_NT_DEF), kw
    return dict(_NT_DEF, id=cid, kernel=kernel, M=M, N=N, K=K, **kw)


PLAIN, GLDS, GEN = "gemm_nt_plain_kernel<64,64,%s>", "gemm_nt_glds_kernel<%s,0,%s,0,128>", "gemm_nt_kernel<%s,0,%s>"
M384 = 128 * 383 + 5             # 384 row tiles of 128, the last with 5 rows
M257 = 64 * 256 + 5              # 257 row tiles of 64: with 3 column tiles more than 512 tiles (two-stage ring), and the 64 statistics replicas wrap four times

# K: one reduction tile is 64 bf16 / 32 fp32 / 128 fp8 elements; every kernel family has cases whose K wraps its ring (more tiles than stages) and cases of one tile
NT_CASES = [
    # -- lean plain kernel, four-stage ring, register-direct epilogue (N % 8 == 0, everything 16-byte aligned, no column reduction)
    _nt("plain4_tr_one_tile", PLAIN % "4,tr", 37, 40, 16, bias="int"),
    _nt("plain4_tr_bias_relu_pre_res", PLAIN % "4,tr", 300, 72, 64, bias="int", act=2, out_pre=True, res="bf16", alpha=0.5, ldo=80, ldpre=88, ldres=96),
    _nt("plain4_tr_f32_res_out", PLAIN % "4,tr", 300, 72, 64, bias="half", res="f32", alpha=0.5, out_f32=True, ldo=76, ldres=84),
    _nt("plain4_tr_out_f32_from_bf16", PLAIN % "4,tr", 101, 136, 32, out_f32=True),
    _nt("plain4_tr_dact2", PLAIN % "4,tr", 300, 72, 64, dact=2, ldz=80, res="bf16"),
    _nt("plain4_tr_alias_res", PLAIN % "4,tr", 300, 72, 64, res="bf16", alias=True, alpha=0.5, ldo=80, ldres=80),
    _nt("plain4_tr_dropout", PLAIN % "4,tr", 300, 72, 64, bias="int", drop=True, res="bf16", alpha=0.5),
    _nt("plain4_tr_ktail_180", PLAIN % "4,tr", 300, 72, 180, lda=184, ldw=188, bias="int", da=0.5),
    _nt("plain4_tr_k392", PLAIN % "4,tr", 133, 72, 392, lda=400, da=0.5, dw=0.5, res="bf16"),
    _nt("plain4_tr_operands_2_bytes_off", PLAIN % "4,tr", 300, 72, 64, off_a=1, off_w=1, lda=66, ldw=66, bias="int"),
    _nt("plain4_tr_swish_pre", PLAIN % "4,tr", 300, 72, 64, bias="half", act=1, out_pre=True),
    _nt("plain4_tr_gelu_pre", PLAIN % "4,tr", 300, 72, 64, bias="mixed", act=3, out_pre=True),
    _nt("plain4_tr_dswish", PLAIN % "4,tr", 300, 72, 64, dact=1, out_f32=True),
    # -- the same kernel with the staged epilogue: the 64-column four-row-group form (whole 4-column groups, strides % 4 == 0) and the scalar form (the rest)
    _nt("plain4_st_one_tile_n_odd", PLAIN % "4,false", 37, 39, 16, bias="int", res="bf16"),
    _nt("plain4_st_n70_everything", PLAIN % "4,false", 300, 70, 328, da=0.5, dw=0.5, lda=336, bias="int", act=2, out_pre=True, res="f32", alpha=0.5, ldo=76, ldpre=72, ldres=80),
    _nt("plain4_st_n_odd_dropout", PLAIN % "4,false", 300, 71, 64, bias="int", drop=True, res="bf16", alpha=0.5, ldo=72, ldres=72),
    _nt("plain4_st_n70_dropout_rows", PLAIN % "4,false", 300, 70, 64, bias="int", drop=True, res="f32", ldo=72, ldres=76),
    _nt("plain4_st_ldo_breaks_v4", PLAIN % "4,false", 300, 72, 64, bias="int", res="bf16", alpha=0.5, ldo=74, ldres=72),
    _nt("plain4_st_out_4_elements_off", PLAIN % "4,false", 300, 72, 64, off_out=4, bias="int", act=2, out_pre=True),
    _nt("plain4_st_dact2_ldz", PLAIN % "4,false", 300, 70, 64, dact=2, ldz=74, colsum=True),
    _nt("plain4_st_colsum", PLAIN % "4,false", 300, 72, 64, bias="int", colsum=True),
    _nt("plain4_st_stats", PLAIN % "4,false", 300, 72, 64, bias="half", stats=True),
    _nt("plain4_st_colsum_stats_wrap", PLAIN % "4,false", 64 * 130 + 7, 40, 16, bias="int", act=2, colsum=True, stats=True),      # 131 row tiles: the replicas wrap twice
    _nt("plain4_st_alias_res", PLAIN % "4,false", 300, 70, 64, res="bf16", alias=True, ldo=72, ldres=72),
    _nt("plain4_st_ktail_20", PLAIN % "4,false", 300, 70, 20, lda=24, ldw=28, bias="int"),
    _nt("plain4_st_swish_n70", PLAIN % "4,false", 300, 70, 64, bias="half", act=1, out_pre=True, ldpre=72),
    _nt("plain4_st_gelu_f32_out", PLAIN % "4,false", 300, 70, 64, bias="mixed", act=3, out_pre=True, out_f32=True),
    # -- two-stage ring: more than 512 tiles, K <= 384, no K tail
    _nt("plain2_tr_771_tiles", PLAIN % "2,tr", M257, 136, 16, bias="int", res="bf16", alpha=0.5),
    _nt("plain2_tr_k384", PLAIN % "2,tr", M257, 136, 384, da=0.25, dw=0.5, lda=392),
    _nt("plain2_st_771_tiles_n130", PLAIN % "2,false", M257, 130, 200, da=0.5, dw=0.5, bias="int", act=2, out_pre=True, res="f32", ldo=132, ldpre=136, ldres=132),
    _nt("plain2_st_stats_colsum", PLAIN % "2,false", M257, 136, 16, bias="half", colsum=True, stats=True),
    # -- LDS-DMA kernel
    _nt("glds_128x128_ragged", GLDS % ("bf16,128,128", 2), M384, 130, 200, da=0.5, dw=0.5, bias="int", res="bf16", alpha=0.5, lda=208, ldw=216),
    _nt("glds_128x128_stats_relu_pre", GLDS % ("bf16,128,128", 2), M384, 130, 16, bias="int", act=2, out_pre=True, stats=True, colsum=True, ldo=132, ldpre=136),
    _nt("glds_128x128_ktail_dropout", GLDS % ("bf16,128,128", 2), M384, 130, 12, bias="half", drop=True, lda=16, ldw=12),
    _nt("glds_128x128_n_odd_f32_out", GLDS % ("bf16,128,128", 2), M384, 129, 16, bias="int", out_f32=True, dact=2),
    _nt("glds_128x64_ktail", GLDS % ("bf16,128,64", 2), M384, 40, 140, da=0.5, dw=0.5, bias="half", res="f32", alpha=0.5, lda=144, ldw=148),
    _nt("glds_128x64_ktail_n_odd_stats", GLDS % ("bf16,128,64", 2), M384, 39, 20, bias="half", stats=True, off_a=1, lda=20),
    _nt("glds_64x64_step2", GLDS % ("bf16,64,64", 4), 187, 72, 328, da=0.5, dw=0.5, step=(25, 50, 2), bias="int", res="bf16"),
    _nt("glds_64x64_step2_n70", GLDS % ("bf16,64,64", 4), 187, 70, 32, step=(25, 50, 2), bias="int", act=2, out_pre=True, lda=40),
    _nt("glds_f32_128x128", GLDS % ("float,128,128", 2), M384, 130, 72, dtype="f32", bias="half", res="f32", alpha=0.5, lda=76, ldw=80),
    _nt("glds_f32_128x64", GLDS % ("float,128,64", 2), M384, 40, 8, dtype="f32", bias="half", stats=True),
    _nt("glds_f32_64x64", GLDS % ("float,64,64", 4), 200, 70, 168, da=0.5, dtype="f32", bias="int", act=2, out_pre=True, res="f32", ldo=72, ldpre=72, ldres=76, lda=172),
    _nt("glds_f32_64x64_one_tile", GLDS % ("float,64,64", 4), 37, 40, 16, dtype="f32", drop=True, bias="int"),
    # -- register-staged kernel: K = 8n + 2, an fp32 source, unaligned fp32 operands
    _nt("gen_k266", GEN % ("bf16,64,64", "0,0"), 300, 70, 266, da=0.5, dw=0.5, lda=268, ldw=270, bias="int", res="bf16", alpha=0.5),
    _nt("gen_k66_one_tile_dropout", GEN % ("bf16,64,64", "0,0"), 37, 40, 18, bias="int", drop=True),
    _nt("gen_step2_unaligned", GEN % ("bf16,64,64", "0,0"), 187, 72, 64, step=(25, 50, 2), off_a=2, bias="int"),
    _nt("gen_k10_128x64", GEN % ("bf16,128,64", "0,0"), M384, 40, 10, bias="half", colsum=True, lda=12),
    _nt("gen_k10_128x128", GEN % ("bf16,128,128", "0,0"), M384, 130, 138, da=0.5, dw=0.5, bias="half", res="bf16", ldw=140),
    _nt("gen_f32src_aligned", GEN % ("bf16,64,64", "1,1"), 300, 72, 200, da=0.5, a_f32=True, bias="int", act=2, out_pre=True, lda=204),
    _nt("gen_f32src_unaligned", GEN % ("bf16,64,64", "1,0"), 300, 70, 36, a_f32=True, off_a=1, bias="int", res="f32", stats=True),
    _nt("gen_f32src_128x64", GEN % ("bf16,128,64", "1,1"), M384, 40, 16, a_f32=True, bias="int", res="bf16"),
    _nt("gen_f32src_128x64_unaligned", GEN % ("bf16,128,64", "1,0"), M384, 39, 16, a_f32=True, off_a=1, bias="int"),
    _nt("gen_f32src_128x128", GEN % ("bf16,128,128", "1,1"), M384, 130, 136, da=0.5, dw=0.5, a_f32=True, bias="int", drop=True, res="bf16", alpha=0.5),
    _nt("gen_f32src_128x128_unaligned", GEN % ("bf16,128,128", "1,0"), M384, 130, 16, a_f32=True, off_w=2, bias="int", colsum=True),
    _nt("gen_f32_64x64", GEN % ("float,64,64", "0,0"), 200, 70, 100, da=0.5, dtype="f32", off_a=1, bias="int", res="f32", alpha=0.5),
    _nt("gen_f32_64x64_one_tile", GEN % ("float,64,64", "0,0"), 37, 39, 20, dtype="f32", bias="int", lda=22, ldw=21),
    _nt("gen_f32_128x64", GEN % ("float,128,64", "0,0"), M384, 40, 8, dtype="f32", off_w=1, bias="half"),
    _nt("gen_f32_128x128", GEN % ("float,128,128", "0,0"), M384, 130, 72, da=0.5, dtype="f32", off_w=1, bias="int", stats=True),
]
# the MODE 0 instances that launch_nt_mode / launch_nt_general (csrc/gemm.hip) can reach without an environment variable: every one has a case above
NT_REACHABLE = sorted(
    [PLAIN % s for s in ("2,tr", "2,false", "4,tr", "4,false")]
    + [GLDS % (t, 4 if t.endswith("64,64") else 2) for t in ("bf16,128,128", "bf16,128,64", "bf16,64,64", "float,128,128", "float,128,64", "float,64,64")]
    + [GEN % (t, f) for t in ("bf16,128,128", "bf16,128,64", "bf16,64,64") for f in ("0,0", "1,0", "1,1")]
    + [GEN % (t, "0,0") for t in ("float,128,128", "float,128,64", "float,64,64")])


def step_rows(M, step):
    """source row of every output row of the strided row source: (m / rows_out) * rows_in + (m % rows_out) * step; and the number of source rows"""
    ro, ri, st = step
    m = torch.arange(M)
    return (m // ro) * ri + (m % ro) * st, ((M - 1) // ro + 1) * ri


def nt_reference(c, a, w, o):
    """the epilogue of avec_gemm_nt on the operands in `o` (bias, keep, z, res): -> o with pre, v (None when transcendental), out, colsum, stats"""
    acc = a @ w.t()
    if "sc" in o:
        acc = acc * o["sc"]
    pre = acc + (o["bias"] if "bias" in o else 0)
    v = pre.clamp_min(0) if c["act"] == 2 else pre
    if c["drop"]:
        v = v * o["keep"]
    if c["dact"] == 2:
        v = v * (o["z"] > 0)
    res = o.get("res", 0)
    return dict(pre=pre, v=v, out=c["alpha"] * v + res)


def nt_operands(c):
    """operands, references and the check_exact() input of one NT_CASES / FP8_CASES entry"""
    gen = _gen(c["id"])
    M, N, K = c["M"], c["N"], c["K"]
    o = dict(a=activations(gen, (M, K), c["da"]), w=weights(gen, (N, K), c["dw"]))
    if c.get("amax_a"):
        o["sc"] = (c["amax_a"] / 448.0) * (c["amax_w"] / 448.0)
    if c["bias"]:
        o["bias"] = draw_ints(gen, (N,), 2) if c["bias"] == "int" else odd_halves(gen, (N,)) if c["bias"] == "half" else draw_ints(gen, (N,), 5) / 2
    if c["drop"]:
        o["keep"] = drop_mask(RNG, RNG_STREAM, DROP_P, (M, N))
    if c["dact"] == 2:
        o["z"] = plant_zeros(draw_ints(gen, (M, N), 2))
        assert bool((o["z"] > 0).any()) and bool((o["z"] < 0).any())
    elif c["dact"] == 1:
        o["z"] = draw_ints(gen, (M, N), 12) / 4               # bf16 numbers in [-3, 3]
    if c["res"]:
        o["res"] = nonzero_ints(gen, (M, N))
    o.update(nt_reference(c, o["a"], o["w"], o))
    f32_out = c["out_f32"] or c["dtype"] == "f32"
    chk = {"bf16": [], "f32": [], "sums": [], "nonzero": []}
    o["transcendental"] = "swish" if c["act"] == 1 else "gelu" if c["act"] == 3 else "dswish" if c["dact"] == 1 else None
    if o["transcendental"]:
        assert not (c["res"] or c["drop"] or c["colsum"] or c["stats"]) and c["alpha"] == 1.0
        if c["dact"] == 1:
            o["out"], o["scale"] = o["pre"] * RW.dswish_(o["z"]), o["pre"].abs() * RW.dswish_mag(o["z"])
        else:
            o["out"], o["scale"] = act_value(c["act"], o["pre"])
        chk["nonzero"].append(o["pre"])
    else:
        masked = c["act"] == 2 or c["dact"] == 2 or c["drop"]
        chk["nonzero"].append(o["pre"] if masked and not c["res"] else o["out"])
        chk["nonzero"].append(o["pre"])
        chk["f32" if f32_out else "bf16"].append(o["out"])
        if c["colsum"]:
            o["colsum"] = o["v"].sum(0) + 0.5              # the accumulated output starts at 0.5
            chk["sums"].append(o["v"]); chk["f32"].append(o["colsum"])
        if c["stats"]:
            o["stats"] = column_stats(o["v"])
            chk["sums"] += [o["v"], o["v"] * o["v"]]; chk["f32"].append(o["stats"])
    if c["out_pre"]:
        chk["f32" if c["dtype"] == "f32" else "bf16"].append(o["pre"])
    chk["sums"].append((o["a"].abs() @ o["w"].abs().t()).reshape(1, -1))          # every accumulator's sum of |products| stays below 2^24
    o["check"] = chk
    return o


# ---- avec_gemm_nt_fp8 ----------------------------------------------------------------------------------------------------------------------------------
# OCP e4m3 (bias 7, 3 mantissa bits) bytes of the integers 0 .. 16; the sign is bit 7
E4M3 = [0x00, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C, 0x4E, 0x50, 0x51, 0x52, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58]


def e4m3_bytes(v):
    """float64 integers in [-16, 16] -> uint8 e4m3 codes"""
    mag = torch.tensor(E4M3, dtype=torch.int64)[v.abs().to(torch.int64)]
    return (mag | ((v < 0).to(torch.int64) << 7)).to(torch.uint8)


def e4m3_value(b):
    """uint8 e4m3 codes -> float64 (finite codes only)"""
    b = b.to(torch.int64)
    e, m = (b >> 3) & 15, b & 7
    mag = torch.where(e == 0, m.double() / 8 * 2.0 ** -6, (1 + m.double() / 8) * torch.exp2(e.double() - 7))
    return torch.where((b & 0x80) != 0, -mag, mag)


def fp8_tile(M, N):
    """the tile rule of avec_gemm_nt_fp8 (the entry point notes no kernel name)"""
    if N > 64 and ((M + 127) // 128) * ((N + 127) // 128) >= 384:
        return "128,128,2"
    return "128,64,2" if ((M + 127) // 128) * ((N + 63) // 64) >= 384 else "64,64,4"


def _fp8(cid, tile, M, N, K, amax_a=448.0, amax_w=448.0, **kw):
    c = _nt(cid, "gemm_nt_fp8_kernel<%s>" % tile, M, N, K, **kw)
    c.update(amax_a=amax_a, amax_w=amax_w, tile=tile)
    return c


FP8_CASES = [
    _fp8("fp8_64_one_tile_k16", "64,64,4", 37, 40, 16, bias="int"),
    _fp8("fp8_64_ragged_relu_res_k656", "64,64,4", 300, 70, 656, lda=672, da=0.5, dw=0.5, bias="int", act=2, out_pre=True, res="bf16", ldo=72, ldres=72, ldpre=72),
    _fp8("fp8_64_dropout", "64,64,4", 300, 72, 64, bias="int", drop=True, res="bf16", alpha=0.5),
    _fp8("fp8_64_n_odd_dropout_f32", "64,64,4", 133, 71, 64, bias="int", drop=True, res="f32", out_f32=True),
    _fp8("fp8_64_half_scale", "64,64,4", 100, 72, 64, amax_a=224.0, bias="int", out_f32=True),
    _fp8("fp8_128x64", "128,64,2", M384, 40, 272, da=0.5, dw=0.5, bias="half", res="bf16"),
    _fp8("fp8_128x128", "128,128,2", M384, 130, 32, bias="int", res="f32", alpha=0.5, out_f32=True, lda=48),
]


# ---- avec_gemm_tn family: O += P^T Q ---------------------------------------------------------------------------------------------------------------------
_TN_DEF = dict(dtype="bf16", entry="tn", q_f32=False, ldp=None, ldq=None, ldo=None, off_p=0, off_q=0, init=0.5, colsum=False, dp=1.0, dq=1.0)


def _tn(cid, kernel, M, I, J, **kw):
    assert set(kw) <= set(_TN_DEF), kw
    return dict(_TN_DEF, id=cid, kernel=kernel, M=M, I=I, J=J, **kw)


TN_TR, TN_GEN = "gemm_tn_tr_kernel<%s,0,2,0,32>", "gemm_tn_kernel<%s>"
TN_CASES = [
    # transposed-read kernel: both operands 16-byte aligned, rows (padded to) whole 8-element pieces
    _tn("tn_tr_64_m1003_j245", TN_TR % "64,64", 1003, 72, 245, ldq=248, ldo=250, dp=0.5, dq=0.5),      # 8 slices of 128 rows, the last with 107; last K tile of 11 rows
    _tn("tn_tr_64_m37_one_tile", TN_TR % "64,64", 37, 64, 64),
    _tn("tn_tr_64_iq_pad", TN_TR % "64,64", 203, 45, 90, ldp=48, ldq=96),
    _tn("tn_tr_128_by_tiles", TN_TR % "128,128", 101, 760, 1021, ldq=1024, ldo=1024),                    # 6 x 8 = 48 tiles of 128 x 128
    _tn("tn_tr_128_by_m", TN_TR % "128,128", 32773, 136, 130, ldq=136, dp=0.25, dq=0.25),               # M >= 32768: 114 slices of 288 rows, the last with 229
    _tn("tn_tr_wide_64x128", TN_TR % "64,128", 32773, 56, 136, dp=0.25, dq=0.25),
    _tn("tn_bias_fused", TN_TR % "64,64", 1003, 72, 80, entry="bias", colsum=True, dp=0.5, dq=0.5, init=-1.5),
    # register-staged kernel
    _tn("tn_bias_separate_pass", TN_GEN % "bf16,64,64,0,0,0", 1003, 72, 80, entry="bias", colsum=True, off_q=2, dp=0.5, dq=0.5),
    _tn("tn_gen_unaligned_i70", TN_GEN % "bf16,64,64,0,0,0", 1003, 70, 66, off_p=2, ldo=68, dp=0.5, dq=0.5),
    _tn("tn_gen_m37", TN_GEN % "bf16,64,64,0,0,0", 37, 70, 66, off_q=2),
    _tn("tn_gen_f32src_aligned", TN_GEN % "bf16,64,64,0,1,1", 203, 72, 72, q_f32=True, ldq=76),
    _tn("tn_gen_f32src_unaligned", TN_GEN % "bf16,64,64,0,1,0", 203, 72, 68, q_f32=True, off_q=1),
    _tn("tn_gen_128_unaligned", TN_GEN % "bf16,128,128,0,0,0", 101, 760, 1021, off_p=2, ldq=1024),
    _tn("tn_f32_unaligned", TN_GEN % "float,64,64,0,0,0", 203, 68, 70, dtype="f32", off_q=1),
    _tn("tn_f32_aligned_j70", TN_GEN % "float,64,64,0,0,1", 1003, 68, 70, dtype="f32", ldq=72, ldo=72, dp=0.5, dq=0.5),
    _tn("tn_f32_128", TN_GEN % "float,128,128,0,0,1", 101, 760, 1021, dtype="f32", ldq=1024),
]


def tn_operands(c, alter=None):
    """alter: (m, i) raises P[m][i] by 1 (the negative control)"""
    gen = _gen(c["id"])
    M, I, J = c["M"], c["I"], c["J"]
    P, Q = activations(gen, (M, I), c["dp"]), activations(gen, (M, J), c["dq"])
    if alter:
        P[alter] += 1
    prod, total = P.t() @ Q, P.abs().t() @ Q.abs()
    o = dict(P=P, Q=Q, prod=prod, out=prod + c["init"])
    o["check"] = {"dw": [(total, c["init"])], "f32": [o["out"]], "nonzero": [prod], "sums": []}
    if c["colsum"]:
        o["colsum"] = P.sum(0) + 0.5
        o["check"]["sums"].append(P); o["check"]["f32"].append(o["colsum"])
    return o


# batched products: P [B][H][M][I] (one matrix per batch and head), Q [B][M][H * d (+ pad)] (heads side by side in a row: a head starts on element h * d), O [B][I][H * d (+ pad)]
def _bt(cid, kernel, B, H, M, I, d, store=False, pad=0):
    return dict(id=cid, kernel=kernel, B=B, H=H, M=M, I=I, d=d, store=store, pad=pad, init=0.0 if store else 0.5)


BATCHED_CASES = [
    _bt("bt_acc_d45", TN_GEN % "bf16,64,64,0,0,0", 2, 3, 77, 50, 45, pad=1),
    _bt("bt_acc_d90", TN_GEN % "bf16,64,64,0,0,0", 2, 3, 37, 50, 90),
    _bt("bt_store_d45", TN_GEN % "bf16,64,64,0,0,0", 2, 3, 77, 50, 45, store=True, pad=1),
    _bt("bt_store_d90", TN_GEN % "bf16,64,64,0,0,0", 2, 3, 37, 50, 90, store=True),
    _bt("bt_store_single_aligned", TN_GEN % "bf16,64,64,0,0,1", 1, 1, 101, 64, 72, store=True),
    _bt("bt_acc_128", TN_GEN % "bf16,128,128,0,0,0", 6, 8, 37, 128, 130),
]
# avec_gemm_tn_batched_multi: (kernel, problems).  A problem joins the common launch when it takes the 64 x 64 register-staged kernel; 128 x 128 tiles run alone, before it
MULTI_CASES = [
    ("gemm_tn_multi_kernel<3>", [_bt("mu3_a", None, 2, 3, 77, 50, 45, pad=1), _bt("mu3_b", None, 1, 4, 37, 40, 90, store=True), _bt("mu3_c", None, 3, 1, 50, 98, 46)]),
    ("gemm_tn_multi_kernel<2>", [_bt("mu2_a", None, 2, 3, 37, 50, 45, store=True, pad=1), _bt("mu2_alone", None, 6, 8, 37, 128, 130), _bt("mu2_b", None, 1, 2, 77, 34, 90)]),
    ("gemm_tn_multi_kernel<1>", [_bt("mu1_a", None, 1, 5, 37, 50, 46)]),
]


def batched_operands(c):
    gen = _gen(c["id"])
    B, H, M, I, d = c["B"], c["H"], c["M"], c["I"], c["d"]
    P, Q = activations(gen, (B, H, M, I)), activations(gen, (B, M, H, d))
    prod = torch.einsum("bhmi,bmhd->bihd", P, Q)
    total = torch.einsum("bhmi,bmhd->bihd", P.abs(), Q.abs())
    o = dict(P=P, Q=Q, out=prod + c["init"])
    o["check"] = {"dw": [(total.reshape(-1, d), c["init"])], "nonzero": [prod], ("bf16" if c["store"] else "f32"): [o["out"]]}
    return o


# grouped products: items (M, I, J, q_step, colsum?), ld == width (I = 180 / 90: rows of 360 / 180 bytes run into the next row)
def _gi(cid, M, I, J, step=0, colsum=False, init=0.5):
    return dict(id=cid, M=M, I=I, J=J, step=step, colsum=colsum, init=init)


GROUPED = "gemm_tn_tr_grouped_kernel<%d,2,64>"
GROUPED_CASES = [
    (GROUPED % 64, [_gi("g64_a", 1003, 180, 90, colsum=True), _gi("g64_b", 37, 90, 180), _gi("g64_c", 300, 90, 44, step=2, init=-1.5), _gi("g64_d", 1500, 64, 72, colsum=True)]),
    (GROUPED % 64, [_gi("g64_alone", 1003, 180, 90, step=2, colsum=True)]),
    (GROUPED % 64, [_gi("g64_32_%d" % k, 37 + 29 * k, 36 + 4 * (k % 5), 40 + 6 * (k % 7), step=2 * (k % 3 == 1), colsum=k % 2 == 0) for k in range(32)]),
    (GROUPED % 128, [_gi("g128_%d" % k, 40 + 13 * k, 380 if k % 2 else 384, 128 if k % 3 else 122, colsum=k % 4 == 0) for k in range(32)]),      # 32 x 3 = 96 tiles of 128 x 128
]
G_ROWS_OUT = 25                   # the row remap of the items with step 2: source row (m / 25) * 50 + (m % 25) * 2


def grouped_operands(t):
    gen = _gen(t["id"])
    P, Q = activations(gen, (t["M"], t["I"])), activations(gen, (t["M"], t["J"]))
    prod, total = P.t() @ Q, P.abs().t() @ Q.abs()
    o = dict(P=P, Q=Q, out=prod + t["init"])
    o["check"] = {"dw": [(total, t["init"])], "f32": [o["out"]], "nonzero": [prod], "sums": []}
    if t["colsum"]:
        o["colsum"] = P.sum(0) + 0.5
        o["check"]["sums"].append(P); o["check"]["f32"].append(o["colsum"])
    return o


def measure_gelu_host_fp32():
    """worst per-element ratio of the plain fp32 host evaluation of GELU against float64 over the pre-activations of the GELU cases"""
    worst = 0.0
    for c in NT_CASES:
        if c["act"] == 3:
            pre = nt_operands(c)["pre"]
            ref, scale = act_value(3, pre)
            worst = max(worst, RW.worst(gelu_(pre.float()), ref, scale))
    return worst


def all_operand_sets():
    """(id, builder) of every operand set the GPU file uses"""
    sets = [(c["id"], (lambda c=c: nt_operands(c))) for c in NT_CASES + FP8_CASES]
    sets += [(c["id"], (lambda c=c: tn_operands(c))) for c in TN_CASES]
    sets += [(c["id"], (lambda c=c: batched_operands(c))) for c in BATCHED_CASES + [p for _, ps in MULTI_CASES for p in ps]]
    sets += [(t["id"], (lambda t=t: grouped_operands(t))) for _, ts in GROUPED_CASES for t in ts]
    return sets
