"""Host-side pieces of the loss / optimizer kernel tests (tests/test_gpu_loss_optim.py): fp64 references of every operation of avec_amd/csrc/loss_optim.hip,
a restatement of the CTC launcher's routing, the case builders and the error metrics.  Pure torch on the host -- tests/test_loss_optim_ref.py pins each
reference to something independent of it, without a GPU.

ctc_route restates avec_ctc_loss.  It is used ONLY to choose and document shapes; which kernel a launch really took is read from avec_last_kernel() on the GPU.
"""
import functools
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24             # unit round-off of fp32
TINY32 = 2.0 ** -126           # the smallest normal fp32: below it the absolute spacing is constant (2^-149), so |x| + TINY32 is the scale of one rounding of x
CTC_MAX_HEADS = 8


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def f32(x):
    """the value a float argument has once it crossed the C ABI"""
    return float(np.float32(x))


# ---- CTC ---------------------------------------------------------------------------------------------------------------------------------------
def ctc_ref(logits, in_lens, targets, tgt_lens, zero_infinity=True, dtype=torch.float64):
    """(nll [B], grad [B, T, V]) of sum_b nll_b w.r.t. the logits: aten's CPU CTC (blank 0, reduction "none") on log_softmax(logits) in `dtype`.
    With zero_infinity an infeasible utterance has loss 0 and a zero gradient; without it the loss is inf and aten's gradient rows are NaN."""
    x = logits.detach().to(dtype).clone().requires_grad_(True)
    lp = torch.log_softmax(x, -1).transpose(0, 1)
    nll = F.ctc_loss(lp, targets.long(), in_lens.long(), tgt_lens.long(), blank=0, reduction="none", zero_infinity=bool(zero_infinity))
    nll.sum().backward()
    return nll.detach(), x.grad.detach()


def ctc_brute(logits, target):
    """-log of the summed probability of every frame labelling that collapses to `target` (all V^T of them), and its gradient by autograd: fp64, one utterance
    logits [T, V].  No recursion, no log-space tricks."""
    T, V = logits.shape
    x = logits.detach().double().clone().requires_grad_(True)
    lp = torch.log_softmax(x, -1)
    paths = torch.tensor(list(itertools.product(range(V), repeat=T)), dtype=torch.int64).reshape(-1, T)
    keep = []
    for p in paths.tolist():
        c = [k for k, _ in itertools.groupby(p) if k != 0]
        keep.append(c == list(target))
    keep = torch.tensor(keep)
    if not bool(keep.any()):
        return float("inf"), torch.zeros(T, V, dtype=torch.float64)
    sel = paths[keep]
    score = lp[torch.arange(T).unsqueeze(0).expand_as(sel), sel].sum(-1)
    nll = -torch.logsumexp(score, 0)
    nll.backward()
    return float(nll.detach()), x.grad.detach()


def ctc_feasible(in_len, labels):
    """an alignment exists iff there is a frame for every label and a blank frame between equal neighbours"""
    labels = list(labels)
    return in_len >= len(labels) + sum(a == b for a, b in zip(labels, labels[1:])) and (in_len > 0 or not labels)


def ctc_route(T, Lmax, V):
    """avec_ctc_loss's choice for a shape: (kernel, waves per utterance or None, bytes of dynamic LDS).  "optin": the wave count the launcher takes when the device
    grants the 128 KB opt-in (4 if it refuses)."""
    S = 2 * Lmax + 1
    lds_fast = (3 * T * S + T + 4 * V + S) * 4
    if lds_fast <= 64 * 1024:
        lds16 = lds_fast + 12 * V * 4
        nw = 16 if lds16 <= 128 * 1024 else 4
        return "ctc_lds_kernel", nw, (lds16 if nw == 16 else lds_fast)
    lds_alpha = (T * S + T + 3 * S) * 4
    if lds_alpha <= 150 * 1024:
        return "ctc_alpha_lds_kernel", None, lds_alpha
    return "ctc_kernel", None, (2 * S + V) * 4 + S * 4


def ctc_multi_fits(T, V, Lmax):
    S = 2 * Lmax + 1
    return (3 * T * S + T + 4 * V + S) * 4 <= 64 * 1024


# (T, Lmax, V) -> the route the launcher's formulas give (tests/test_loss_optim_ref.py checks this table against ctc_route, the GPU test against the library's report)
CTC_SHAPES = [
    ((60, 12, 40), "ctc_lds_kernel w16"),            # baseline, S = 25
    ((80, 32, 32), "ctc_lds_kernel w16"),            # S = 65 > 64 lanes; 65 028 B, no opt-in
    ((80, 32, 40), "ctc_lds_kernel w16"),            # 65 540 B: 4 B over the limit, 16 waves through the 128 KB opt-in
    ((100, 20, 256), "ctc_lds_kernel w16"),          # the shipped vocabulary and frame count: opt-in
    ((10, 3, 2100), "ctc_lds_kernel w4"),            # 135 308 B > 128 KB: fallback wave count, V strided 33 times
    ((140, 130, 40), "ctc_alpha_lds_kernel"),        # S = 261 > 256 threads (149 852 B)
    ((188, 45, 40), "ctc_alpha_lds_kernel"),
    ((160, 150, 40), "ctc_kernel"),                  # S = 301, global workspace
]
# the rows of every CTC batch (all nine fit all eight shapes: none is dropped)
CTC_ROWS = ["random", "norepeat", "exactfit", "oneshort", "allequal", "empty", "oneframe", "peaky", "noframes"]
PEAKY = 20.0


def norepeat_labels(L, V):
    """L labels in [1, V) without equal neighbours (nor equal next-but-one neighbours)"""
    y = 1 + (torch.arange(L) * 7) % (V - 1)
    assert L < 2 or bool((y[1:] != y[:-1]).all())
    return y


def repeat_labels(L, V):
    """the same with several adjacent repeats, one of them a run of three"""
    y = norepeat_labels(L, V).clone()
    pos = sorted({1, L // 3, L // 3 + 1, L - 1}) if L >= 6 else [1]
    for i in pos:
        y[i] = y[i - 1]
    return y


def n_repeats(y):
    y = list(int(v) for v in y)
    return sum(a == b for a, b in zip(y, y[1:]))


@functools.lru_cache(maxsize=None)
def ctc_case(T, Lmax, V, seed=11):
    """(logits [9, T, V] fp32, in_lens, targets [9, Lmax] padded with 1, tgt_lens, feasible [9]) -- the rows of CTC_ROWS; built once, never modified"""
    g = _gen(seed + T + 1000 * Lmax)
    B = len(CTC_ROWS)
    x = torch.randn(B, T, V, generator=g)
    tg = torch.ones(B, Lmax, dtype=torch.int64)
    il, tl = torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)
    nr, rp = norepeat_labels(Lmax, V), repeat_labels(Lmax, V)
    Leq = min(Lmax, (T + 1) // 2)
    rows = {
        "random": (T, torch.randint(1, V, (Lmax,), generator=g)),
        "norepeat": (T, nr),
        "exactfit": (Lmax + n_repeats(rp), rp),
        "oneshort": (Lmax + n_repeats(rp) - 1, rp),
        "allequal": (2 * Leq - 1, torch.full((Leq,), int(nr[-1]))),
        "empty": (max(T // 2, 1), nr[:0]),
        "oneframe": (1, nr[:1]),
        "peaky": (T, nr),
        "noframes": (0, nr[:min(2, Lmax)]),
    }
    feas = []
    for b, name in enumerate(CTC_ROWS):
        n, y = rows[name]
        assert 0 <= n <= T and len(y) <= Lmax
        il[b], tl[b] = n, len(y)
        tg[b, :len(y)] = y
        feas.append(ctc_feasible(n, y.tolist()))
    x[CTC_ROWS.index("peaky")] *= PEAKY
    return x, il, tg, tl, torch.tensor(feas)


MH_T = [50, 25, 100, 13, 40, 77, 31, 64]                 # frames of the heads of the multi-head cases: all different
MH_W = [0.5, 0.3, 1.0, 0.25, 0.7, 0.15, 0.9, 0.05]       # and so are the weights
MH_V, MH_LMAX = 32, 6


@functools.lru_cache(maxsize=None)
def ctc_multi_case(n_heads, seed=17):
    """(targets [9, 6], tgt_lens, [(logits [9, T_h, 32], in_lens, feasible)] per head): the labels are shared, every head has its own frame count and its own
    lengths; the rows are those of CTC_ROWS"""
    V, Lmax = MH_V, MH_LMAX
    g = _gen(seed + n_heads)
    B = len(CTC_ROWS)
    nr, rp = norepeat_labels(Lmax, V), repeat_labels(Lmax, V)
    labels = [torch.randint(1, V, (Lmax,), generator=g), nr, rp, rp, torch.full((4,), 9), nr[:0], nr[:1], nr, nr[:2]]
    tg = torch.ones(B, Lmax, dtype=torch.int64)
    for b, y in enumerate(labels):
        tg[b, :len(y)] = y
    tl = torch.tensor([len(y) for y in labels])
    heads = []
    for h in range(n_heads):
        T = MH_T[h]
        x = torch.randn(B, T, V, generator=g)
        x[CTC_ROWS.index("peaky")] *= PEAKY
        fit = Lmax + n_repeats(rp)
        il = torch.tensor([T, T - 3 - h, fit, fit - 1, 7, T // 2 + h, 1, T, 0])
        assert int(il.max()) <= T and int(il.min()) == 0
        heads.append((x, il, torch.tensor([ctc_feasible(int(n), y.tolist()) for n, y in zip(il, labels)])))
    return tg, tl, heads


def row_rel(got, ref):
    """max-norm relative error of each utterance on its own: [B].  A NaN anywhere in a row gives inf."""
    B = ref.shape[0]
    d = (got.double() - ref.double()).reshape(B, -1).abs().amax(1)
    s = ref.double().reshape(B, -1).abs().amax(1)
    r = torch.where(s > 0, d / s.clamp_min(1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    return torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)


# ---- softmax cross-entropy -----------------------------------------------------------------------------------------------------------------------
def softmax_ce_ref(x, y, ignore_index=-100, dtype=torch.float64):
    """(loss [M], grad [M, V], mean): loss = logsumexp(x) - x[y]; 0 with a zero gradient row when y == ignore_index or y is outside [0, V); mean over ALL M rows"""
    x = x.to(dtype)
    M, V = x.shape
    ok = (y != ignore_index) & (y >= 0) & (y < V)
    ys = torch.where(ok, y, torch.zeros_like(y))
    lse = torch.logsumexp(x, -1)
    loss = torch.where(ok, lse - x.gather(1, ys[:, None])[:, 0], torch.zeros_like(lse))
    grad = torch.softmax(x, -1)
    grad[torch.arange(M), ys] -= 1
    grad = torch.where(ok[:, None], grad, torch.zeros_like(grad))
    return loss, grad, loss.sum() / M


CE_SHAPES = [(1, 5), (7, 63), (9, 64), (130, 65), (33, 500), (5, 2100)]
CE_PEAKY = 30.0


@functools.lru_cache(maxsize=None)
def ce_case(M, V, seed=21):
    """(x [M, V] fp32, y [M]): row 0 has its logits times 30; the rows from the end backwards are y == -100, y == -1 and y == V, as far as M allows (M = 1: the
    ignore and out-of-range rows come from ce_case_ys instead)"""
    g = _gen(seed + M + 100 * V)
    x = torch.randn(M, V, generator=g)
    y = torch.randint(0, V, (M,), generator=g)
    x[0] *= CE_PEAKY
    for k, v in enumerate([-100, -1, V]):
        if M - 1 - k >= 1:
            y[M - 1 - k] = v
    return x, y


def ce_case_ys(M, V):
    """the target vectors a shape is run with: the case's own, and for M = 1 (no room for the special rows beside the peaky one) one vector per special target"""
    x, y = ce_case(M, V)
    if M > 3:
        return [y]
    return [y] + [torch.full_like(y, v) for v in (-100, -1, V)]


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd, gscale, dtype=torch.float64):
    """one step of csrc/loss_optim.hip's adam_kernel in `dtype`: (p_new, m_new, v_new).
        g' = g * gscale + wd * p;  m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2;  p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
    The hyperparameters, the step and lr are rounded to fp32 first: those are the values the kernel receives."""
    t = lambda s: torch.tensor(f32(s), dtype=dtype)
    b1, b2, ep, w, gs, st, l = t(beta1), t(beta2), t(eps), t(wd), t(gscale), t(step), t(lr)
    p, g, m, v = p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)
    bc1, bc2s = 1 - b1 ** st, torch.sqrt(1 - b2 ** st)
    gr = g * gs + w * p
    m = m + (1 - b1) * (gr - m)
    v = b2 * v + (1 - b2) * gr * gr
    return p - (l / bc1) * (m / (torch.sqrt(v) / bc2s + ep)), m, v


def adam_scales(p, g, m, v, step, lr, beta1, beta2, eps, wd, gscale):
    """(s_update, s_m, s_v) fp64: the magnitude of the TERMS each result of adam_ref is summed from -- one fp32 rounding of a term is 2^-24 of it, whatever is left
    of the sum after cancellation (m_new = 0.9 m + 0.1 g' vanishes where g' ~ -9 m; an error measured against |m_new| itself would be ruled by the one element of
    the tensor that cancels most).
        a = |g gscale| + |wd p|;  s_m = |m| + a;  s_v = beta2 v + (1 - beta2) a^2;  s_update = |p| + kappa lr / (1 - beta1^step) * s_m / (sqrt(v_new) / sqrt(1 - beta2^step) + eps)
    each plus 2^-126, the spacing scale of the subnormal range."""
    t = lambda s: torch.tensor(f32(s), dtype=torch.float64)
    b1, b2, ep, w, gs, st, l = t(beta1), t(beta2), t(eps), t(wd), t(gscale), t(step), t(lr)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    a = (g * gs).abs() + (w * p).abs()
    sm = m.abs() + a
    sv = b2 * v + (1 - b2) * a * a
    v_new = adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd, gscale)[2]
    # the bias corrections 1 - beta^step cancel at small steps: one rounding of beta^step (which fp32 cannot avoid) is beta^s / (1 - beta^s) roundings of the
    # correction -- 250 of them, halved by the square root, for beta2 = 0.999 at step 2.  The same factor for every element of a launch.
    kappa = 1 + b1 ** st / (1 - b1 ** st) + 0.5 * b2 ** st / (1 - b2 ** st)
    su = p.abs() + kappa * (l / (1 - b1 ** st)) * sm / (torch.sqrt(v_new) / torch.sqrt(1 - b2 ** st) + ep)
    return su + TINY32, sm + TINY32, sv + TINY32


def noam_lr(step, warmup=10000, dim=360, factor=2):
    s = float(step)
    return factor * dim ** -0.5 * min(s * warmup ** -1.5, s ** -0.5)


def adam_inputs(n, seed):
    """(p, g, m, v) fp32: gradients of every magnitude the kernel meets -- the first quarter are exact zeros with v = 0 (the denominator is eps alone where wd = 0; half of them have m = 0 as well),
    the second near 1e-20 (g^2 is a subnormal), the third near 1e4, the rest of order one; m and v elsewhere are those of a run in progress"""
    g_ = _gen(seed)
    p = 0.1 * torch.randn(n, generator=g_)
    g = torch.randn(n, generator=g_)
    m = 0.1 * torch.randn(n, generator=g_)
    v = 0.01 * torch.rand(n, generator=g_)
    q = max(n // 4, 1)
    g[:q], v[:q] = 0, 0
    m[1:q:2] = 0                                           # every other one with m = 0 too; the rest keep m: their update is lr m_new / (bc1 eps) when wd = 0
    g[q:2 * q] *= 1e-20
    g[2 * q:3 * q] *= 1e4
    return p, g, m, v


def scaled_err(got, ref, floor):
    """max_i |got_i - ref_i| / (|ref_i| + floor_i): every element judged at its own magnitude, in units of which one fp32 rounding is 2^-24.  NaN -> inf"""
    e = (got.double() - ref.double()).abs() / (ref.double().abs() + floor)
    e = torch.where(torch.isnan(e), torch.full_like(e, math.inf), e)
    return float(e.max())


# ---- shadow refresh -----------------------------------------------------------------------------------------------------------------------------------
def shadow_blocks(A, Tm, C):
    return Tm * ((A + 63) // 64) * ((C + 63) // 64)


def shadow_table(entries):
    """entries: dicts with src, fwd, bwd, A, Tm, C and optionally Cp (default C) and ldb (default 0) -> int64 [n, 10] table with first_block / n_blocks filled in,
    and the total number of blocks"""
    rows, first = [], 0
    for e in entries:
        nb = shadow_blocks(e["A"], e["Tm"], e["C"])
        rows.append([e["src"], e["fwd"], e["bwd"], e["A"], e["Tm"], e["C"], first, nb, e.get("Cp", e["C"]), e.get("ldb", 0)])
        first += nb
    return torch.tensor(rows, dtype=torch.int64), first


def shadow_ref(master, table_row, dtype):
    """the two images of one table entry: (fwd_pos, fwd_val, bwd_pos, bwd_val) -- flat positions in the shadow buffer and the values there, cast to `dtype` with
    torch's round-to-nearest-even.  forward: [A][Tm][C] as the master has it, or [A][Cp] when padded (Tm = 1, Cp > C; the pad columns are not part of the image);
    backward: [C][Tm][A] with row pitch ldb (0: Tm * A).  An offset of -1 gives an empty image."""
    src, fwd, bwd, A, Tm, C, _, _, Cp, ldb = (int(v) for v in table_row)
    W = master[src:src + A * Tm * C].reshape(A, Tm, C)
    a, t, c = torch.meshgrid(torch.arange(A), torch.arange(Tm), torch.arange(C), indexing="ij")
    none = torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=dtype)
    if fwd >= 0:
        padded = Cp > C and Tm == 1
        ldf = Cp if padded else Tm * C
        fpos = fwd + a * ldf + (0 if padded else t * C) + c
        f = fpos.reshape(-1), W.to(dtype).reshape(-1)
    else:
        f = none
    if bwd >= 0:
        pitch = ldb if ldb > 0 else Tm * A
        bpos = bwd + c * pitch + t * A + a
        b = bpos.reshape(-1), W.to(dtype).reshape(-1)
    else:
        b = none
    return f[0], f[1], b[0], b[1]


def shadow_case():
    """(master fp32, entries, shadow_len): hand-built table -- (A, Tm, C) = (64, 1, 64), (130, 1, 72), (10, 1, 24), (64, 1, 245) padded to 248 without a backward image, (96, 9, 32), (7, 3, 5), (6, 1, 4), a fused group of
    three (8, 1, 12) weights, a (6, 1, 8) entry whose backward rows are padded to a pitch of 8, an (8, 1, 8) entry whose forward offset alone is odd and one whose three offsets are all odd.  Images are
    laid out one after the other with a gap of 5..8 elements (so that the next aligned offset is a multiple of 4) between them."""
    shapes = [dict(A=64, Tm=1, C=64), dict(A=130, Tm=1, C=72), dict(A=10, Tm=1, C=24), dict(A=64, Tm=1, C=245, Cp=248, nobwd=True), dict(A=96, Tm=9, C=32),
              dict(A=7, Tm=3, C=5), dict(A=6, Tm=1, C=4)]
    entries, so, sh = [], 0, 8
    al4 = lambda n: (n + 8) // 4 * 4
    for s in shapes:
        n = s["A"] * s["Tm"] * s["C"]
        e = dict(A=s["A"], Tm=s["Tm"], C=s["C"], src=so, fwd=sh)
        if "Cp" in s:
            e["Cp"] = s["Cp"]
        sh = al4(sh + s["A"] * s.get("Cp", s["Tm"] * s["C"]) if "Cp" in s else sh + n)
        if s.get("nobwd"):
            e["bwd"] = -1
        else:
            e["bwd"] = sh
            sh = al4(sh + n)
        so = al4(so + n)
        entries.append(e)
    base = sh                                              # fused group: three [8][12] weights side by side in one [12][24] backward image
    sh = al4(sh + 12 * 24)
    for k in range(3):
        entries.append(dict(A=8, Tm=1, C=12, src=so, fwd=sh, bwd=base + k * 8, ldb=24))
        so, sh = al4(so + 96), al4(sh + 96)
    # a backward image whose pitch is padded (A = 6 in rows of 8): aligned offset and pitch, so only A % 4 keeps the backward store element-wise -- a vector store
    # there would write the two pad elements of every row
    entries.append(dict(A=6, Tm=1, C=8, src=so, fwd=sh, bwd=sh + 56, ldb=8))
    so, sh = al4(so + 48), al4(sh + 56 + 64)
    entries.append(dict(A=8, Tm=1, C=8, src=so, fwd=sh + 1, bwd=sh + 72))      # aligned source and backward image, odd forward offset: only the forward store is element-wise
    assert so % 4 == 0 and (sh + 1) % 2 and (sh + 72) % 4 == 0
    so, sh = al4(so + 64), al4(sh + 72 + 64)
    so, sh = so + 1, sh + 1                                # odd source, forward and backward offsets: the three element-wise paths
    e = dict(A=8, Tm=1, C=8, src=so, fwd=sh, bwd=sh + 64 + 6)
    assert e["src"] % 2 and e["fwd"] % 2 and e["bwd"] % 2
    entries.append(e)
    so, sh = so + 64, e["bwd"] + 64 + 7
    master = torch.randn(so + 16, generator=_gen(31)) * 3
    return master, entries, sh
