"""Host-side pieces of the relative-position attention kernel tests (tests/test_gpu_attention.py): the fp64 reference of avec_relpos_attention_fwd / _bwd
(avec_amd/csrc/attention.hip, attention_mfma.hip) with per-element error scales, host models of the kernels' declared rounding points, the case table, the
restatement of the host dispatch (which kernel instance a shape reaches) and the tolerances.  Pure torch on the host -- tests/test_attention_ref.py pins every
formula to something independent of it, checks the preconditions of the case table and seeds faults into the host model, without a GPU.

Layout (per case): q, dO [B][T][H][d]; k, v [B][Tk][H][d]; e, de [R][H][d], R = Tk + T - 1; keep [B][T][Tk] (bool).

    s_ij  = scale * q_i . (k_j + e_{(T-1) - i + j})
    P     = softmax_j over the kept keys (a masked key has probability exactly 0; a row without a kept key is uniform over all Tk keys: the kernels and the
            reference model add -1e9 in fp32, which absorbs every score below 32 in magnitude -- max|s| < 32 is a precondition on the case table)
    O     = P V                                 (m, l) = (row maximum of the masked scores, sum_j exp(s_ij - m))
    dV    = P^T dO        dP = dO V^T           dS = P o (dP - rowsum(P o dP)) * scale
    dQ    = dS (K + E_skew)                     dK = dS^T Q
    dSrel[i][r] = dS[i][r - (T-1) + i] (zero elsewhere)         dE_r = de0_r + sum_b sum_i dSrel[b][i][r] q_i

Every result comes with a scale: the same formula with every term taken by its magnitude.  The judgement is rowwise_ref.ratio:
|got - ref| <= TOL * scale + half a bf16 ulp (bf16 outputs) + 2^-126.

Host models (evaluate(..., model)): they exist ONLY to measure what the declared rounding points cost, and so to set the tolerances.
    valu_f32    fp32 throughout; exp = exp2(fl32(x * log2 e)) (rowwise_ref.exp_)
    valu_bf16   the same on bf16 inputs with bf16-stored O / P / dS / dQ / dK / dV; the column pass reads the stored P and dS, the row pass uses the unrounded dS for dQ
    mfma_bf16   P rounded to bf16 before P.V, dS rounded to bf16 before dQ, delta from the bf16 O, fp32 sums
"""
import math

import numpy as np
import torch

from tests import rowwise_ref as RW

D64, F32 = torch.float64, torch.float32
NEG = -1e9
FAMILIES = ("O", "lse", "P", "dS", "dSrel", "dQ", "dK", "dV", "dE")
MODELS = ("valu_f32", "valu_bf16", "mfma_bf16")


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def skew_index(T, Tk):
    """[T][Tk]: the E row of the pair (i, j)"""
    return (T - 1) - torch.arange(T)[:, None] + torch.arange(Tk)[None, :]


def gather_rel(x, idx):
    """x [..][T][R] -> [..][T][Tk]: y[i][j] = x[i][(T-1) - i + j]"""
    return torch.gather(x, -1, idx.expand(x.shape[:-2] + idx.shape))


def scatter_rel(y, idx, R):
    """y [..][T][Tk] -> [..][T][R]: the dsrel layout of attention.h, zero elsewhere"""
    out = torch.zeros(y.shape[:-1] + (R,), dtype=y.dtype)
    return out.scatter_(-1, idx.expand(y.shape[:-2] + idx.shape), y)


def keep_mask(B, T, Tk, lens=None, len_div=1, q_full=0, mask=None, fault=None):
    """bool [B][T][Tk]: key j of batch element b is kept for query i.  A dense mask overrides lens / q_full (attention.h key_keep)"""
    if mask is not None:
        return (mask != 0).expand(B, T, Tk).clone()
    i, j = torch.arange(T)[None, :, None], torch.arange(Tk)[None, None, :]
    keep = torch.ones(B, T, Tk, dtype=torch.bool)
    if lens is not None:
        klen = torch.as_tensor(lens, dtype=torch.int64) // len_div
        if fault == "ceil_len_div":
            klen = -(-torch.as_tensor(lens, dtype=torch.int64) // len_div)
        if fault == "klen_inclusive":
            klen = klen + 1
        keep = keep & (j < klen[:, None, None])
    qf = q_full if q_full > 0 else T
    if fault == "q_full_plus_one" and q_full > 0:
        qf = q_full + 1
    return keep & (i < qf)


def evaluate(inp, model="f64", fwd=None, bwd_model=None, fault=None):
    """-> {name: value} (model) or {name: (value, scale)} (fp64).  `fwd`: the forward results a backward model reads (m, l, O as stored) -- by default the same
    model's; bwd_model: the model of the backward passes when it differs from the forward's (bf16 MFMA forward, bf16 VALU backward).  `fault`: a seeded defect
    (tests/test_attention_ref.py)"""
    ref = model == "f64"
    c = D64 if ref else F32
    bmodel = bwd_model or model
    st_f = _bf if model.endswith("bf16") else (lambda x: x)
    st_b = _bf if bmodel.endswith("bf16") else (lambda x: x)
    q, k, v, e = (inp[n].to(c) for n in ("q", "k", "v", "e"))
    B, T, H, d = q.shape
    Tk, R = k.shape[1], e.shape[0]
    scale = torch.tensor(inp["scale"], dtype=c)
    keep = inp["keep"]
    if fault in ("ceil_len_div", "klen_inclusive", "q_full_plus_one") and inp.get("mask") is None:
        keep = keep_mask(B, T, Tk, inp.get("lens"), inp.get("len_div", 1), inp.get("q_full", 0), None, fault)
    if fault == "drop_tile_last" and Tk >= 32:
        keep = keep.clone(); keep[:, :, 31] = False
    keep = keep[:, None]                                                  # [B][1][T][Tk]
    qh, kh, vh, eh = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), e.permute(1, 0, 2)
    idx = skew_index(T, Tk)
    if fault == "skew_off_by_one":
        idx = idx.clone(); i0 = 32 if T > 32 else 0; idx[i0] = (idx[i0] + 1).clamp_max(R - 1)
    s = scale * (qh @ kh.transpose(-1, -2) + gather_rel(torch.einsum("bhtd,hrd->bhtr", qh, eh), idx))
    anyk = keep.any(-1, keepdim=True)
    if ref:
        sm = torch.where(anyk, torch.where(keep, s, torch.full_like(s, -math.inf)), torch.zeros_like(s))
    else:
        sm = s + torch.where(keep, torch.zeros_like(s), torch.full_like(s, NEG))
        if fault == "masked_row_over_klen":
            lens = inp.get("lens")
            if lens is not None and inp.get("mask") is None:
                klen = (torch.as_tensor(lens, dtype=torch.int64) // inp.get("len_div", 1)).clamp(1, Tk)
                inside = torch.arange(Tk)[None, None, None, :] < klen[:, None, None, None]
                sm = torch.where(anyk | inside, sm, torch.full_like(sm, -math.inf))
    if fault == "phantom_key":                                            # a key beyond Tk (the clamped copy of the last one) takes part in the softmax
        sm = torch.cat([sm, s[..., -1:]], -1); vh = torch.cat([vh, vh[:, :, -1:]], 2)
    m = sm.amax(-1, keepdim=True)
    pu = RW.exp_(sm - m)
    l = pu.sum(-1, keepdim=True)
    if model == "mfma_bf16":
        O = (_bf(pu) @ vh) * (1 / l)
    else:
        O = (pu @ vh) / l
    if fault == "no_inv_l":
        O = O.clone(); O[:, :, T // 2] = (pu @ vh)[:, :, T // 2]
    if fault == "phantom_key":
        pu, vh, sm = pu[..., :-1], vh[:, :, :-1], sm[..., :-1]
    O = st_f(O)
    out = {"O": O.permute(0, 2, 1, 3), "m": torch.where(anyk, m, torch.full_like(m, NEG))[..., 0] if ref else m[..., 0], "l": l[..., 0]}
    if ref:
        p = pu / l
        smag = scale * (qh.abs() @ kh.abs().transpose(-1, -2) + gather_rel(torch.einsum("bhtd,hrd->bhtr", qh.abs(), eh.abs()), idx))
        out["s"] = s
        out["full_masked"] = ~anyk[..., 0].expand(B, H, T)
        out["lse"] = (m + l.log())[..., 0], ((p * smag).sum(-1) + l.log()[..., 0].abs())
        out["O"] = out["O"], (p @ vh.abs()).permute(0, 2, 1, 3)
    if "dO" not in inp:
        return out

    # ---- backward ----
    g = inp["dO"].to(c).permute(0, 2, 1, 3)
    if ref:
        dP = g @ vh.transpose(-1, -2)
        delta = (p * dP).sum(-1, keepdim=True)
        dS = p * (dP - delta) * scale
        dPm = g.abs() @ vh.abs().transpose(-1, -2)
        dSm = p * (dPm + (p * dPm).sum(-1, keepdim=True)) * scale
        Pst, dSst, dSq = p, dS, dS
    else:
        f = fwd or out
        fm, fl, fO = f["m"].to(c)[..., None], f["l"].to(c)[..., None], f["O"].to(c).permute(0, 2, 1, 3)
        delta = (g * fO).sum(-1, keepdim=True)
        p = RW.exp_(sm - fm) * (1 / fl)
        dS = p * (g @ vh.transpose(-1, -2) - delta) * scale
        Pst, dSst = st_b(p), st_b(dS)
        dSq = dSst if bmodel == "mfma_bf16" else dS
    de0 = inp["de0"].to(c).permute(1, 0, 2)
    rel_q, rel_st = scatter_rel(dSq, idx, R), scatter_rel(dSst, idx, R)
    dQ = dSq @ kh + torch.einsum("bhtr,hrd->bhtd", rel_q, eh)
    dK, dV = dSst.transpose(-1, -2) @ qh, Pst.transpose(-1, -2) @ g
    dEs = torch.einsum("bhtr,bhtd->hrd", rel_st, qh)
    if fault == "de_row_shift":
        dEs = dEs.roll(1, 1)
    dE = dEs if fault == "de_overwrite" else de0 + dEs
    back = lambda x: x.permute(0, 2, 1, 3)
    if not ref:
        out.update(P=Pst, dS=dSst, dSrel=rel_st, dQ=back(st_b(dQ)), dK=back(st_b(dK)), dV=back(st_b(dV)), dE=dE.permute(1, 0, 2))
        return out
    rel_m = scatter_rel(dSm, idx, R)
    out.update(P=(p, p), dS=(dS, dSm), dSrel=(rel_st, rel_m),
               dQ=(back(dQ), back(dSm @ kh.abs() + torch.einsum("bhtr,hrd->bhtd", rel_m, eh.abs()))),
               dK=(back(dK), back(dSm.transpose(-1, -2) @ qh.abs())), dV=(back(dV), back(p.transpose(-1, -2) @ g.abs())),
               dE=(dE.permute(1, 0, 2), (de0.abs() + torch.einsum("bhtr,bhtd->hrd", rel_m, qh.abs())).permute(1, 0, 2)))
    return out


# ---- which kernel instance a launch reaches: a restatement of attn_mfma_fwd / attn_mfma_bwd_rows / launch_bwd, used to choose and document shapes; the GPU test
# reads the instance that really ran from avec_last_kernel() and compares ------------------------------------------------------------------------------------------
LDS_LIMIT = 160 * 1024


def mfma_geom(T, d, bwd):
    """(lds bytes, alias) of attention_mfma.hip's mfma_geom, or None when not even the alias image set fits 160 KB"""
    pitch = 128 if d <= 64 else 256
    Tp = (T + 31) // 32 * 32
    for alias in (0, 1):
        total = (1 if alias else 2) * Tp * pitch + (Tp + 64) * pitch + 64 * pitch * (2 if bwd else 1) + 2 * 8192
        if total <= LDS_LIMIT:
            return total, alias
    return None


def mfma_instance(T, d, bwd):
    """"<PITCH,NTM,ALIAS,DKS>" or None"""
    g = mfma_geom(T, d, bwd) if (d <= 96 and T <= 384) else None
    if g is None:
        return None
    pitch, dks = (128 if d <= 64 else 256), (d + 15) // 16
    ntm = 7 if (T <= 224 and not g[1]) else 12
    k = dks if (pitch == 128 and dks in (3, 4)) or (pitch == 256 and dks == 6) else 0
    return "<%d,%d,%d,%d>" % (pitch, ntm, g[1], k)


def valu_lds(d, bwd):
    """dynamic LDS of attn_rows_kernel: K, V tiles of 64 rows, the E window of 95, Q (and dO) tiles of 32, rows of d | 1 floats, + 4 x 64 probabilities"""
    return (2 * 64 + 95 + (64 if bwd else 32)) * (d | 1) * 4 + 1024


def route(dtype, T, d, Tk, has_mask, dsrel, ld=None):
    """(forward name, backward name); ld: the smallest row stride of q / k / v / e / dout (rows of fewer than dpad - d elements are not staged by the MFMA kernels: the
    16-byte chunks of the rows before the last one would run past the end of the tensor).  None when the call is rejected before any launch: the column pass serves d <= 96, and the VALU row kernels' LDS request passes
    160 KB above d = 159 (forward) / d = 141 (backward) although the argument check admits d <= 192"""
    inst_f = inst_b = None
    if dtype == "bf16" and not has_mask and Tk == T and not (ld is not None and ld + d < (d + 15) // 16 * 16):
        inst_f, inst_b = mfma_instance(T, d, False), mfma_instance(T, d, True)
    fwd = "attn_mfma_fwd" + inst_f if inst_f else ("attn_rows<%s,fwd>" % dtype if valu_lds(d, False) <= LDS_LIMIT else None)
    cols = not dsrel and Tk == T
    if (cols and d > 96) or (not inst_b and valu_lds(d, True) > LDS_LIMIT):
        return fwd, None
    bwd = "attn_mfma_bwd" + inst_b if inst_b else "attn_rows<%s,bwd>" % dtype
    if cols:
        bwd += "+cols<%d>" % (48 if d <= 48 else 64 if d <= 64 else 96)
    return fwd, bwd


# every instance the dispatch can select (AVEC_PICK_ATTN, attn_rows_kernel, LB()).  <256,12,0,*> is instantiated but unreachable: a pitch-256 image set without
# aliasing fits only T <= 128, where NTM = 7 is chosen
MFMA_INSTANCES = ["<128,%d,%d,%d>" % (n, a, k) for n, a in ((7, 0), (12, 0), (12, 1)) for k in (4, 3, 0)] + ["<256,%d,%d,%d>" % (n, a, k) for n, a in ((7, 0), (12, 1)) for k in (6, 0)]
REACHABLE_FWD = ["attn_mfma_fwd" + i for i in MFMA_INSTANCES] + ["attn_rows<f32,fwd>", "attn_rows<bf16,fwd>"]
REACHABLE_BWD_ROWS = ["attn_mfma_bwd" + i for i in MFMA_INSTANCES] + ["attn_rows<f32,bwd>", "attn_rows<bf16,bwd>"]
REACHABLE_COLS = [(dt, c) for dt in ("f32", "bf16") for c in (48, 64, 96)]


# ---- the case table --------------------------------------------------------------------------------------------------------------------------------------
def C(name, B, H, T, d, lens=None, len_div=1, q_full=0, mask=None, Tk=0, dsrel=False, spike=0, strided=False):
    return dict(name=name, B=B, H=H, T=T, d=d, lens=lens, len_div=len_div, q_full=q_full, mask=mask, Tk=Tk or T, dsrel=dsrel, spike=spike, strided=strided)


# mask: (kind, Bm), kind in random / causal / zero_row.  lens are in frames: klen = lens // len_div.  spike: 1 = even pairs through the key, odd through the E
# row; 2 = the other way round.  Both dtypes run every case (f32 always takes the VALU kernels)
CASES = [
    # ---- T and d edges on the plain path (bf16: MFMA where it serves the shape) ----
    C("T1_d1", 1, 1, 1, 1),                                                   # rows of one element: VALU in both dtypes (see route)
    C("T2_d8", 2, 3, 2, 8, lens=[2, 1]),
    C("T31_d16", 2, 2, 31, 16, lens=[31, 30], spike=1),                       # <128,7,0,0>, one wave half empty
    C("T32_d17", 3, 3, 32, 17, lens=[32, 19, 1], spike=2),                    # odd head offsets, d % 8 != 0 on the last head of the last row
    C("T33_d45", 2, 3, 33, 45, lens=[33, 20], q_full=30, spike=1),            # <128,7,0,3>; second wave holds one query
    C("T33_d45_div3", 2, 3, 33, 45, lens=[100, 62], len_div=3, q_full=32),    # klen = 33 (all), 20; the ceiling would give 34, 21
    C("T63_d46", 2, 2, 63, 46, lens=[62, 50], spike=2, dsrel=True),
    C("T64_d48", 2, 2, 64, 48, lens=[64, 33], spike=1),                       # cols<48>
    C("T65_d64", 2, 2, 65, 64, lens=[65, 52], q_full=64, spike=2),            # <128,7,0,4>, cols<64>, two workgroups
    C("T65_d1", 1, 3, 65, 1, lens=[64]),                                      # rows of 3 elements: VALU; the MFMA staging read past the end of k / v / e here
    C("T97_d65", 2, 2, 97, 65, lens=[97, 32], spike=1),                       # <256,7,0,0>, cols<96>
    C("T64_d96", 1, 2, 64, 96, lens=[63], spike=2),                           # <256,7,0,6>
    C("T33_lens0", 3, 2, 33, 16, lens=[0, 1, 33], q_full=1),                  # lens 0: every key masked; q_full = 1: one live query
    C("T33_qfull", 2, 2, 33, 64, lens=[33, 32], q_full=32, dsrel=True),       # q_full = T - 1
    C("T224_d64", 1, 2, 224, 64, lens=[211], spike=1),                        # last NTM = 7 length
    C("T225_d45", 1, 2, 225, 45, spike=2, dsrel=True),                        # <128,12,0,3>
    C("T225_d64", 1, 2, 225, 64, lens=[224], q_full=224, dsrel=True),         # <128,12,0,4>
    C("T320_d16", 1, 2, 320, 16, lens=[307], spike=1, dsrel=True),            # <128,12,0,0>: last length before K and V share an image
    C("T321_d64", 1, 2, 321, 64, lens=[308], spike=2),                        # <128,12,1,4>
    C("T384_d48", 2, 2, 384, 48, lens=[384, 32], spike=1, dsrel=True),        # <128,12,1,3>
    C("T384_d8", 1, 1, 384, 8, lens=[383], spike=0, dsrel=True),              # <128,12,1,0>
    C("T385_d64", 2, 2, 385, 64, lens=[385, 372], q_full=384, spike=2),                   # beyond the MFMA limit: bf16 VALU rows + cols<64>; the largest shape
    # ---- pitch 256 (d = 90): alias and fall-back switches, and the band with an MFMA forward and a VALU backward ----
    C("T128_d90", 1, 2, 128, 90, lens=[115], spike=1),                        # <256,7,0,6>
    C("T129_d90", 1, 2, 129, 90, spike=2),                                    # <256,12,1,6>
    C("T129_d65", 1, 2, 129, 65, lens=[128], dsrel=True),                     # <256,12,1,0>
    C("T192_d90", 1, 2, 192, 90, lens=[179], spike=1, dsrel=True),            # last MFMA backward
    C("T193_d90", 1, 2, 193, 90, lens=[180], spike=2),                        # MFMA forward, VALU backward reading its (m, l) and O
    C("T224_d90", 1, 2, 224, 90, spike=1, dsrel=True),                        # the same, last MFMA forward
    C("T225_d90", 1, 2, 225, 90, lens=[637], len_div=3, spike=2),                        # VALU both ways, cols<96>
    # ---- wide heads: VALU in both dtypes; the column pass serves d <= 96 ----
    C("T33_d97", 2, 2, 33, 97, lens=[33, 20], q_full=30, dsrel=True),
    C("T33_d97_reject", 1, 2, 33, 97),                                        # no dsrel: rejected before any launch
    C("T33_d150", 1, 2, 33, 150, lens=[32], dsrel=True, spike=1),             # forward only: the backward row pass asks for more than 160 KB of LDS and is rejected
    C("T31_d192", 2, 1, 31, 192, lens=[31, 18], dsrel=True),                  # admitted by the argument check, rejected by the LDS request in both directions
    # ---- dense masks (VALU) ----
    C("mask_random_Bm1", 2, 2, 33, 45, mask=("random", 1)),
    C("mask_random_BmB", 2, 2, 65, 64, mask=("random", 2), dsrel=True),
    C("mask_causal_BmB", 2, 3, 64, 16, mask=("causal", 2)),
    C("mask_zero_row_Bm1", 3, 2, 33, 48, mask=("zero_row", 1)),
    C("mask_zero_row_BmB", 2, 2, 97, 90, mask=("zero_row", 2)),
    # ---- key/value cache (Tk > T): forward and probability pass ----
    C("Tk_plus1", 2, 2, 33, 45, Tk=34, lens=[34, 21]),
    C("Tk_plus37", 2, 3, 31, 64, Tk=68, lens=[206, 121], len_div=3, spike=1),
    C("Tk_plus64", 2, 2, 1, 16, Tk=65),
    C("Tk_plus64_mask", 2, 2, 33, 90, Tk=97, mask=("causal", 2)),
    # ---- strided rows (ld, ldo, lde, lddq, ldd, ldde, ldt, ldr larger than the width), finite garbage in the gaps ----
    C("strided_T65_d45", 2, 3, 65, 45, lens=[65, 52], strided=True, spike=1),
    C("strided_T33_d90_dsrel", 2, 2, 33, 90, lens=[33, 20], strided=True, dsrel=True),
    C("strided_T225_d90", 1, 2, 225, 90, lens=[212], strided=True),
]
CASE = {c["name"]: c for c in CASES}
SPIKE_SCORE = 14.0


def make_mask(kind, Bm, T, Tk, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "causal":                                                  # causal-like: query i sees the cache and the keys up to itself
        return (torch.arange(Tk)[None, None, :] <= torch.arange(T)[None, :, None] + (Tk - T)).float().repeat(Bm, 1, 1)
    m = (torch.rand(Bm, T, Tk, generator=g) < 0.6).float()
    m[:, :, 0 if kind == "random" else -1] = 1                            # no empty row ...
    if kind == "zero_row":
        m[-1, T // 2] = 0                                                 # ... but these two
        m[0, T - 1] = 0
    return m


def spike_pairs(case, b):
    """([(i, j*, via)], klen): queries and the edge keys they are made to concentrate on in batch element b, via 'k' (the key) or 'e' (the E row: last batch element
    only, an E row is shared by the batch).  The queries are ordered so that the pairs lie on different diagonals"""
    T, Tk, B = case["T"], case["Tk"], case["B"]
    klen = Tk if case["lens"] is None else min(case["lens"][b] // case["len_div"], Tk)
    js = []
    for j in (0, 31, 32, 63, 64, T - 1, klen - 1):
        if 0 <= j < klen and j not in js:
            js.append(j)
    qf = case["q_full"] or T
    qs = list(dict.fromkeys(i for i in (qf - 1, 0, 33, 31, 1, 64, 32, 63, 30, 65, 96) if 0 <= i < qf))
    return [(qs[n], j, "e" if (b == B - 1 and (n + case["spike"]) % 2 == 0) else "k") for n, j in enumerate(js) if n < len(qs)], klen


def make_inputs(case, dtype, with_bwd=True):
    """inputs as fp64 tensors holding values of `dtype`; scores with a standard deviation near 2 (q, k, e ~ N(0, sqrt 2): s = q.(k + e) / sqrt d)"""
    B, H, T, d, Tk = (case[n] for n in ("B", "H", "T", "d", "Tk"))
    R = Tk + T - 1
    seed = 5000 + 7 * T + 13 * d + 101 * B + Tk
    sg = 2.0 ** 0.25
    q, k, e = RW.gauss((B, T, H, d), seed) * sg, RW.gauss((B, Tk, H, d), seed + 1) * sg, RW.gauss((R, H, d), seed + 2) * sg
    v = RW.gauss((B, Tk, H, d), seed + 3)
    scale = float(np.float32(1.0 / math.sqrt(d)))
    spikes = []

    def lift(b, i, j, via):
        """raise s_ij of every head to SPIKE_SCORE by adding a multiple of q_i to the key or to the E row"""
        for h in range(H):
            qi = q[b, i, h]
            add = (SPIKE_SCORE - scale * float(qi @ (k[b, j, h] + e[T - 1 - i + j, h]))) / (scale * float(qi @ qi)) * qi
            if via == "k":
                k[b, j, h] += add
            else:
                e[T - 1 - i + j, h] += add
    if case["spike"]:
        todo = [(b,) + pr for b in range(B) for pr in spike_pairs(case, b)[0]]
        for via in ("e", "k"):                                            # the E rows first: a key is lifted against the final E
            for b, i, j, w in todo:
                if w == via:
                    lift(b, i, j, via)
        spikes = [(b, i, j) for b, i, j, _ in todo]
        for b in range(B):                                                # the first masked key spikes too, for the first pair's query: it must come out as exactly 0
            pairs, klen = spike_pairs(case, b)
            if klen < Tk and pairs:
                lift(b, pairs[0][0], klen, "k")
    rd = lambda x: RW.rd(x, dtype)
    mask = make_mask(case["mask"][0], case["mask"][1], T, Tk, seed + 9) if case["mask"] else None
    inp = dict(q=rd(q), k=rd(k), v=rd(v), e=rd(e), scale=scale, lens=case["lens"], len_div=case["len_div"], q_full=case["q_full"], mask=mask, spikes=spikes,
               keep=keep_mask(B, T, Tk, case["lens"], case["len_div"], case["q_full"], mask))
    if with_bwd:
        inp["dO"] = rd(RW.gauss((B, T, H, d), seed + 4))
        inp["de0"] = RW.rd(RW.gauss((R, H, d), seed + 5) * 0.5, "f32")
    return inp


def case_route(case, dtype):
    """route() of a case as tests/test_gpu_attention.py lays it out: unstrided rows are H * d wide"""
    return route(dtype, case["T"], case["d"], case["Tk"], case["mask"] is not None, case["dsrel"], ld=case["H"] * case["d"])


def models_of(case, dtype):
    """(forward model, backward model) of a launch of `case` in `dtype`"""
    if dtype == "f32":
        return "valu_f32", "valu_f32"
    f, b = case_route(case, dtype)
    return ("mfma_bf16" if (f and "mfma" in f) else "valu_bf16"), ("mfma_bf16" if (b and "mfma" in b) else "valu_bf16")


def host_ratios(case, dtype, fault=None):
    """{family: worst ratio} of the host model of (case, dtype) against fp64"""
    inp = make_inputs(case, dtype)
    ref = evaluate(inp)
    fm, bm = models_of(case, dtype)
    got = evaluate(inp, fm, bwd_model=bm, fault=fault)
    return judge_all(got, ref, dtype, case), (fm, bm)


def judge_all(got, ref, dtype, case):
    """{family: worst ratio}; the (m, l) pair of a fully masked row is m == -1e9 and l == Tk exactly (a sum of Tk ones); zeros owed exactly (masked P, out-of-band dSrel) have scale 0"""
    out = {}
    live = ~ref["full_masked"]
    lse = got["m"].double() + got["l"].double().log()
    out["lse"] = float(RW.ratio(lse[live], ref["lse"][0][live], ref["lse"][1][live]).max()) if bool(live.any()) else 0.0
    dead = ~live
    if bool(dead.any()) and not (bool((got["m"][dead] == NEG).all()) and bool((got["l"][dead] == case["Tk"]).all())):
        out["lse"] = math.inf
    act = {"O": dtype, "P": dtype, "dS": dtype, "dSrel": dtype, "dQ": dtype, "dK": dtype, "dV": dtype, "dE": "f32"}
    for fam, odt in act.items():
        if fam in got and fam in ref:
            out[fam] = RW.worst(got[fam], ref[fam][0], ref[fam][1], odt)
    return out


def measure_host():
    """{model: {family: worst ratio over the case table}}; forward families under the forward model, backward families under the backward model"""
    out = {m: {f: 0.0 for f in FAMILIES} for m in MODELS}
    for case in CASES:
        for dtype in ("f32", "bf16"):
            r, (fm, bm) = host_ratios(case, dtype)
            for fam, w in r.items():
                mdl = fm if fam in ("O", "lse") else bm
                out[mdl][fam] = max(out[mdl][fam], w)
    return out


# Per-element tolerance: |got - ref| <= TOL[model][family] * scale (+ the bf16 and subnormal terms of rowwise_ref.ratio).  8 x the worst ratio that the HOST model of
# the same rounding points reaches over the case table above: the project's margin for device summation order and FMA contraction.  Measured on the CPU
# (measure_host; tests/test_attention_ref.py re-measures); no figure comes from a GPU run.
#                 O        m + log l  P         dS        dSrel     dQ        dK        dV        dE
HOST_WORST = {
    "valu_f32":  {"O": 1.90e-6, "lse": 3.05e-7, "P": 1.00e-5, "dS": 2.47e-6, "dSrel": 2.47e-6, "dQ": 2.62e-7, "dK": 4.04e-7, "dV": 2.73e-6, "dE": 3.87e-7},
    "valu_bf16": {"O": 2.27e-7, "lse": 8.78e-8, "P": 2.03e-6, "dS": 2.77e-3, "dSrel": 2.77e-3, "dQ": 1.54e-3, "dK": 1.79e-3, "dV": 3.64e-3, "dE": 1.52e-3},
    "mfma_bf16": {"O": 2.38e-3, "lse": 1.03e-7, "P": 1.37e-6, "dS": 9.02e-4, "dSrel": 9.02e-4, "dQ": 6.11e-4, "dK": 6.41e-4, "dV": 2.51e-3, "dE": 9.75e-4},
}
TOL = {m: {f: 8 * w for f, w in fam.items()} for m, fam in HOST_WORST.items()}
