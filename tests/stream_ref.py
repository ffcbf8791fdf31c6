"""Host-side pieces of the streaming-encoder tests (tests/test_stream_ref.py, tests/test_gpu_stream_kernels.py): fp64 references of avec_glu_dwconv_stream and
avec_relpos_attention_stream (avec_amd/csrc/convmod.hip, attention.hip) in CHUNKED form -- carried context rows, ring cache, per-slot position counters, restart
flags, exactly the state the kernels keep -- beside the plain offline formulas on the whole utterance, the push schedule that both the host and the GPU tests
walk, per-element error scales and the tolerances.  Pure torch on the host.

Every formula is written once, in the dtype of its arguments (tests/rowwise_ref.py): fp64 arguments give the reference and its scale, fp32 arguments the plain
host fp32 evaluation whose own error sets the tolerance.  `scale` is the same formula with every term taken by its magnitude; the judgement is rowwise_ref.ratio.

Layouts: u [T][2C] (pre-GLU), w [K][C] (tap-major), ss [2][C] (eval-mode BatchNorm scale | shift); q, k, v [T][H][d], E [L + 1][H][d] (row delta = i - j).
"""
import torch

from tests import rowwise_ref as RW

D64 = torch.float64
GARBAGE = 7.25           # what the state buffers hold before the first push: must never be seen (a restart hides it by position, not by clearing)


# ---- the convolution module's middle --------------------------------------------------------------------------------------------------------------
def _conv_rows(gp, gm, w, bias, ss, stride, To):
    """gp / gm [K - 1 + n][C]: GLU outputs (and magnitudes) with the left context in front; output row o reads rows o * stride + k, taps in the kernel's order"""
    K, C = w.shape
    idx = torch.arange(To) * stride
    acc = (bias if bias is not None else torch.zeros(C, dtype=gp.dtype)).expand(To, C).clone()
    mag = acc.abs()
    for k in range(K):
        acc = acc + w[k] * gp[idx + k]
        mag = mag + w[k].abs() * gm[idx + k]
    pre, pmag = acc * ss[0] + ss[1], mag * ss[0].abs() + ss[1].abs()
    return RW.swish_(pre), RW.swish_mag(pre) + RW.dswish_mag(pre) * pmag


def _glu(u):
    C = u.shape[-1] // 2
    a, b = u[..., :C], u[..., C:]
    return a * RW.sigmoid_(b), a.abs() * RW.sig_mag(b)


def conv_offline(u, w, bias, ss, stride):
    """Swish(BN_eval(depthwise_causal(GLU(u)))) of a whole utterance u [T][2C] -> (out [To][C], scale), To = (T - 1) // stride + 1 (zero GLU rows in front)"""
    K, C = w.shape
    g, gm = _glu(u)
    z = torch.zeros(K - 1, C, dtype=u.dtype)
    return _conv_rows(torch.cat([z, g]), torch.cat([z, gm]), w, bias, ss, stride, (u.shape[0] - 1) // stride + 1)


class ConvStream:
    """avec_glu_dwconv_stream's state and semantics: ctx [B][K - 1][2C] (last rows of u), pos [B] (stage frames since the restart)"""

    def __init__(self, B, C, K, dtype=D64):
        self.ctx = torch.full((B, K - 1, 2 * C), GARBAGE, dtype=dtype)
        self.pos = [0] * B

    def push(self, u, w, bias, ss, stride, n=None, reset=()):
        """u [B][Tq][2C]; slot b takes n[b] rows (default all); -> (out [B][Tq / stride][C], scale).  Rows at or past n[b] are computed from u as passed"""
        B, Tq, _ = u.shape
        K, C = w.shape
        outs, scs = [], []
        for b in range(B):
            if b in reset:
                self.pos[b] = 0
            p0, nb = self.pos[b], (Tq if n is None else n[b])
            g, gm = _glu(torch.cat([self.ctx[b], u[b]]))
            absent = torch.arange(K - 1 + Tq) < (K - 1) - p0               # context rows older than the restart
            g, gm = g.masked_fill(absent[:, None], 0), gm.masked_fill(absent[:, None], 0)
            o, s = _conv_rows(g, gm, w, bias, ss, stride, Tq // stride)
            outs.append(o), scs.append(s)
            self.ctx[b] = torch.cat([self.ctx[b], u[b, :nb]])[nb:nb + K - 1] if K > 1 else self.ctx[b]
            self.pos[b] = p0 + nb
        return torch.stack(outs), torch.stack(scs)


# ---- relative-position attention over the band -------------------------------------------------------------------------------------------------------
def attn_offline(q, k, v, E, scale, keep):
    """q, k, v [T][H][d], E [L + 1][H][d], keep [T][T] bool (no empty row) -> (O [T][H][d], scale): s_ij = scale q_i . (k_j + E[i - j]) over the kept keys"""
    T, L = q.shape[0], E.shape[0] - 1
    dl = (torch.arange(T)[:, None] - torch.arange(T)[None, :]).clamp(0, L)          # (a pair outside 0 .. L is never kept)
    qh, kh, vh = q.permute(1, 0, 2), k.permute(1, 0, 2), v.permute(1, 0, 2)
    s = scale * (qh @ kh.transpose(1, 2) + torch.einsum("hid,ijhd->hij", qh, E[dl]))
    s = s.masked_fill(~keep[None], -float("inf"))
    pu = RW.exp_(s - s.amax(-1, keepdim=True))
    p = pu / pu.sum(-1, keepdim=True)
    return (p @ vh).permute(1, 0, 2), (p @ vh.abs()).permute(1, 0, 2)


class AttnStream:
    """avec_relpos_attention_stream's state and semantics: rings kc / vc [B][cap = L + Tq][H][d] (frame p in row p mod cap), pos [B]"""

    def __init__(self, B, H, d, L, Tq, dtype=D64):
        self.L, self.Tq, self.cap = L, Tq, L + Tq
        self.kc = torch.full((B, self.cap, H, d), GARBAGE, dtype=dtype)
        self.vc = torch.full((B, self.cap, H, d), GARBAGE, dtype=dtype)
        self.pos = [0] * B

    def push(self, q, k, v, E, scale, n=None, reset=()):
        """q, k, v [B][Tq][H][d] -> (O [B][Tq][H][d], scale).  The chunk's first n[b] rows are appended BEFORE the window is read (the kernel's query tiles append
        in any order): the rows they overwrite are older than any frame a query of this push may see"""
        B, Tq, L, cap = q.shape[0], self.Tq, self.L, self.cap
        outs, scs = [], []
        for b in range(B):
            if b in reset:
                self.pos[b] = 0
            p0, nb = self.pos[b], (Tq if n is None else n[b])
            for i in range(nb):
                self.kc[b, (p0 + i) % cap], self.vc[b, (p0 + i) % cap] = k[b, i], v[b, i]
            c = torch.arange(cap)                                           # window column c = position p0 - L + c
            p = p0 - L + c
            ring = p.clamp_min(0) % cap
            kw = torch.where((c < L)[:, None, None], self.kc[b, ring], k[b, (c - L).clamp_min(0)])
            vw = torch.where((c < L)[:, None, None], self.vc[b, ring], v[b, (c - L).clamp_min(0)])
            dl = torch.arange(Tq)[:, None] + L - c[None, :]
            keep = (dl >= 0) & (dl <= L) & (p >= 0)[None, :]
            qh, kh, vh = q[b].permute(1, 0, 2), kw.permute(1, 0, 2), vw.permute(1, 0, 2)
            s = scale * (qh @ kh.transpose(1, 2) + torch.einsum("hid,ijhd->hij", qh, E[dl.clamp(0, L)]))
            s = s.masked_fill(~keep[None], -float("inf"))
            pu = RW.exp_(s - s.amax(-1, keepdim=True))
            pr = pu / pu.sum(-1, keepdim=True)
            vh = vh.masked_fill(~(p >= 0)[None, :, None], 0)                 # (absent rows hold GARBAGE: probability 0, but 0 * garbage must not be formed from NaN / inf)
            outs.append((pr @ vh).permute(1, 0, 2)), scs.append((pr @ vh.abs()).permute(1, 0, 2))
            self.pos[b] = p0 + nb
        return torch.stack(outs), torch.stack(scs)


def band(T, L, S):
    """the offline stack's mask at a stage behind total stride S: oracle.context_mask at the input rate, strided [::S, ::S] -> bool [T][T]"""
    from oracle import avec_oracle as O
    return O.context_mask(T * S, None, L, 0)[0, 0, ::S, ::S][:T, :T] != 0


# ---- the push schedule ------------------------------------------------------------------------------------------------------------------------------------
def schedule(utts, Tq):
    """utts: per slot, the lengths of the utterances it receives one after the other -> list of pushes; a push = per slot (utterance index or None, first frame,
    frames taken n, restart).  An utterance whose length is no multiple of Tq ends with a short chunk; the slot's next utterance starts with a restart; a slot that
    has run out takes n = 0 frames of whatever is passed"""
    cur = [[0, 0] for _ in utts]                  # utterance index, frames done
    pushes = []
    while any(c[0] < len(u) for c, u in zip(cur, utts)):
        row = []
        for c, u in zip(cur, utts):
            if c[0] >= len(u):
                row.append((None, 0, 0, False))
                continue
            n = min(Tq, u[c[0]] - c[1])
            row.append((c[0], c[1], n, c[1] == 0))
            c[1] += n
            if c[1] >= u[c[0]]:
                c[0], c[1] = c[0] + 1, 0
        pushes.append(row)
    return pushes


def chunk_of(data, row, Tq, filler):
    """data[b][utterance] [T][...] -> the push's input [B][Tq][...]: the frames taken, then `filler` (finite garbage: rows past n are outside the contract)"""
    out = []
    for b, (ui, t0, n, _) in enumerate(row):
        ref = data[b][0]
        x = torch.full((Tq,) + tuple(ref.shape[1:]), filler, dtype=ref.dtype)
        if ui is not None:
            x[:n] = data[b][ui][t0:t0 + n]
        out.append(x)
    return torch.stack(out)


# ---- tolerances ----------------------------------------------------------------------------------------------------------------------------------------------
# Attention: the kernel's arithmetic is attn_rows_kernel's (fp32 VALU scores, exp, online softmax, fp32 P.V, output stored in the activation dtype): the "O" family of
# tests/attention_ref.py's valu_f32 / valu_bf16 host models applies as it stands (attention_ref.TOL).
# Convolution: 8 x the worst ratio of the plain host fp32 evaluation of conv_offline over the GPU test's case table (measure_conv_host; re-measured by
# tests/test_stream_ref.py); inputs of either activation dtype, the bf16 output's own rounding is the half ulp of rowwise_ref.ratio.  Measured on the CPU.
CONV_HOST_WORST = 1.0e-7          # measured 9.92e-8 (both activation dtypes, 24 cases x 6 utterances)
CONV_TOL = 8 * CONV_HOST_WORST
CONV_CASES = [(C, K, s, Tq) for C in (8, 36) for K in (3, 15) for s in (1, 2) for Tq in (2, 4, 16)]
CONV_UTTS = lambda Tq: [[3 * Tq, 2 * Tq], [Tq, 2 * Tq + max(Tq // 2, 1), Tq], [4 * Tq]]       # B = 3: slot 1 restarts in push 2, ends short in push 4, restarts; slot 2 runs out


def conv_inputs(C, K, s, Tq, dtype, seed=0):
    """(data[b][utterance] [T][2C], w, bias, ss) as fp64 tensors holding values of `dtype` (activations) / fp32 (parameters)"""
    sd = 9000 + 131 * C + 17 * K + 5 * s + Tq + seed
    data = [[RW.rd(RW.gauss((T, 2 * C), sd + 100 * b + u) * 1.5, dtype) for u, T in enumerate(ut)] for b, ut in enumerate(CONV_UTTS(Tq))]
    w = RW.rd(RW.gauss((K, C), sd + 1) * 0.4, "f32")
    bias = RW.rd(RW.coef(C, 1) * 0.3, "f32")
    ss = RW.rd(torch.stack([RW.coef(C, 2, positive=True), RW.coef(C, 3) * 0.5]), "f32")
    return data, w, bias, ss


def measure_conv_host():
    worst = 0.0
    for C, K, s, Tq in CONV_CASES:
        for dtype in ("f32", "bf16"):
            data, w, bias, ss = conv_inputs(C, K, s, Tq, dtype)
            for utts in data:
                for u in utts:
                    ref, sc = conv_offline(u, w, bias, ss, s)
                    got, _ = conv_offline(u.float(), w.float(), bias.float(), ss.float(), s)
                    worst = max(worst, RW.worst(got, ref, sc))
    return worst
