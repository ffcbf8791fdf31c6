"""Host-side pieces of the look-ahead streaming tests (tests/test_stream_la_ref.py, tests/test_gpu_stream_la_kernels.py, tests/test_gpu_stream_la_stack.py): fp64
references, in CHUNKED form, of avec_relpos_attention_stream_la (two-sided band over a window, ring of committed rows), of the window bookkeeping of
avec_stream_window / avec_stream_window_advance (carried tail, pend, pos, ended, the commit rule) and a toy stack (attention -> stride-2 convolution -> attention at
half rate) that pins the look-ahead LA and its rounding LAe.  avec_glu_dwconv_stream_la needs no reference of its own: it is stream_ref.ConvStream.push on the window
rows with n = the committed rows.  Pure torch on the host; layouts and the error scales are those of tests/stream_ref.py.
"""
import torch

from tests import rowwise_ref as RW
from tests import stream_ref as SR

D64 = torch.float64
GARBAGE = SR.GARBAGE


def lookahead(strides, R):
    """strides: the conv stride of every block, in order -> (LA, LAe, S): block b's attention, behind total stride div_b, sees R // div_b frames of its own rate"""
    div, la = 1, 0
    for s in strides:
        la += R // div * div
        div *= s
    return la, -(-la // div) * div, div


def band(T, L, R, S):
    """the offline stack's mask at a stage behind total stride S: oracle.context_mask(left L, right R) at the input rate, strided [::S, ::S] -> bool [T][T]"""
    from oracle import avec_oracle as O
    return O.context_mask(T * S, None, L, R)[0, 0, ::S, ::S][:T, :T] != 0


def attn_offline(q, k, v, E, scale, keep, R):
    """stream_ref.attn_offline with E [L + R + 1][H][d], row delta + R for delta = i - j = -R .. L.  That function reads E[i - j]: the queries are moved R rows down
    (R zero queries in front that keep themselves, R zero keys behind that nobody keeps), so that row i + R reads E[i + R - j]"""
    T = q.shape[0]
    z = torch.zeros((R,) + tuple(q.shape[1:]), dtype=q.dtype)
    keep2 = torch.zeros(T + R, T + R, dtype=torch.bool)
    keep2[R:, :T] = keep
    keep2[torch.arange(R), torch.arange(R)] = True
    o, sc = SR.attn_offline(torch.cat([z, q]), torch.cat([k, z]), torch.cat([v, z]), E, scale, keep2)
    return o[R:], sc[R:]


class AttnStreamLA:
    """avec_relpos_attention_stream_la's state and semantics: rings kc / vc [B][cap = L + Tq][H][d] (frame p in row p mod cap), pos [B] (COMMITTED stage frames)"""

    def __init__(self, B, H, d, L, R, Tq, dtype=D64):
        self.L, self.R, self.Tq, self.cap = L, R, Tq, L + Tq
        self.kc = torch.full((B, self.cap, H, d), GARBAGE, dtype=dtype)
        self.vc = torch.full((B, self.cap, H, d), GARBAGE, dtype=dtype)
        self.pos = [0] * B

    def push(self, q, k, v, E, scale, n, c, reset=()):
        """q, k, v [B][Wq][H][d]: slot b has n[b] valid window rows of which the first c[b] (<= Tq) are committed -> (O [B][Wq][H][d], scale).  A query that keeps
        no key gives zeros.  The committed rows are appended BEFORE the window is read (the kernel's query tiles append in any order)"""
        B, Wq, L, R, cap = q.shape[0], q.shape[1], self.L, self.R, self.cap
        outs, scs = [], []
        for b in range(B):
            if b in reset:
                self.pos[b] = 0
            p0, nb, cb = self.pos[b], n[b], c[b]
            assert 0 <= cb <= min(nb, self.Tq) and nb <= Wq
            for i in range(cb):
                self.kc[b, (p0 + i) % cap], self.vc[b, (p0 + i) % cap] = k[b, i], v[b, i]
            col = torch.arange(L + Wq)                                     # window column = position p0 - L + col
            p = p0 - L + col
            ring = p.clamp_min(0) % cap
            kw = torch.where((col < L)[:, None, None], self.kc[b, ring], k[b, (col - L).clamp_min(0)])
            vw = torch.where((col < L)[:, None, None], self.vc[b, ring], v[b, (col - L).clamp_min(0)])
            valid = torch.where(col < L, p >= 0, col - L < nb)
            dl = torch.arange(Wq)[:, None] + L - col[None, :]
            keep = (dl >= -R) & (dl <= L) & valid[None, :]
            some = keep.any(-1)
            qh, kh, vh = q[b].permute(1, 0, 2), kw.permute(1, 0, 2), vw.permute(1, 0, 2)
            s = scale * (qh @ kh.transpose(1, 2) + torch.einsum("hid,ijhd->hij", qh, E[(dl + R).clamp(0, L + R)]))
            s = s.masked_fill(~keep[None], -float("inf")).masked_fill(~some[None, :, None], 0.0)
            pu = RW.exp_(s - s.amax(-1, keepdim=True))
            pr = (pu / pu.sum(-1, keepdim=True)).masked_fill(~some[None, :, None], 0.0)
            vh = vh.masked_fill(~valid[None, :, None], 0)                  # (absent rows: probability 0, but 0 * garbage must not be formed from NaN / inf)
            outs.append((pr @ vh).permute(1, 0, 2)), scs.append((pr @ vh.abs()).permute(1, 0, 2))
            self.pos[b] = p0 + cb
        return torch.stack(outs), torch.stack(scs)


class Window:
    """avec_stream_window / avec_stream_window_advance: per slot the tail of frames heard and not final [LAe][...], pend, pos (committed input frames), ended.
    `extra`: frames committed beyond the rule (0: the rule; the tests show that S more is an error)"""

    def __init__(self, B, Tc, LAe, S, shape, dtype=D64, extra=0):
        self.B, self.Tc, self.LAe, self.S, self.W, self.extra = B, Tc, LAe, S, Tc + LAe, extra
        self.tail = torch.full((B, LAe) + tuple(shape), GARBAGE, dtype=dtype)
        self.pend, self.pos, self.ended = [0] * B, [0] * B, [False] * B

    def begin(self, x_new, n_new, last=(), reset=()):
        """x_new [B][Tc][...] -> X [B][W][...] = [tail[:pend] | x_new[:n_new] | zeros] and per slot nvalid, ncommit, emit"""
        X = torch.zeros((self.B, self.W) + tuple(x_new.shape[2:]), dtype=x_new.dtype)
        nvalid, ncommit, emit = [], [], []
        for b in range(self.B):
            pe, en = (0, False) if b in reset else (self.pend[b], self.ended[b])
            nn = 0 if en else min(max(int(n_new[b]), 0), self.Tc)
            n = pe + nn
            X[b, :pe], X[b, pe:n] = self.tail[b, :pe], x_new[b, :nn]
            c = min(n // self.S * self.S, max(0, n - self.LAe) // self.S * self.S + self.extra)
            nvalid.append(n), ncommit.append(0 if b in last else c), emit.append(n if b in last else c)
        self._now = (nvalid, ncommit, set(last), set(reset))
        return X, nvalid, ncommit, emit

    def advance(self, X):
        nvalid, ncommit, last, reset = self._now
        for b in range(self.B):
            n, c = nvalid[b], ncommit[b]
            if b not in last:
                self.tail[b, :n - c] = X[b, c:n]
            self.pend[b] = 0 if b in last else n - c
            self.pos[b] = (0 if b in reset else self.pos[b]) + c
            self.ended[b] = (False if b in reset else self.ended[b]) or b in last


def schedule(utts, Tc):
    """stream_ref.schedule with the `last` flag: per push, per slot (utterance index or None, first frame, frames taken, restart, last)"""
    return [[(ui, t0, n, rs, ui is not None and t0 + n == utts[b][ui]) for b, (ui, t0, n, rs) in enumerate(row)] for row in SR.schedule(utts, Tc)]


def walk(utts, Tc, LAe, S, data, step, filler=3.0, extra=0):
    """Drive a Window over the schedule: step(X [B][W][...], nvalid, ncommit, reset) -> rows [B][W / S][...] per push.  -> per (slot, utterance) the emitted rows
    concatenated (a running slot: the first ncommit / S rows; a slot in `last`: all ceil(nvalid / S)), and the Window"""
    B = len(utts)
    win = Window(B, Tc, LAe, S, data[0][0].shape[1:], data[0][0].dtype, extra)
    got = [[[] for _ in u] for u in utts]
    for row in schedule(utts, Tc):
        x = SR.chunk_of(data, [r[:4] for r in row], Tc, filler)
        last, reset = {b for b, r in enumerate(row) if r[4]}, {b for b, r in enumerate(row) if r[3]}
        X, nvalid, ncommit, emit = win.begin(x, [r[2] for r in row], last, reset)
        out = step(X, nvalid, ncommit, reset)
        win.advance(X)
        for b, (ui, _, _, _, _) in enumerate(row):
            if ui is not None:
                got[b][ui].append(out[b][:-(-emit[b] // S)])
    return [[torch.cat(g) for g in gb] for gb in got], win


class Toy:
    """attention (band L, R) -> GLU + causal depthwise convolution of stride 2 -> attention at half rate (band L // 2, R // 2), with fixed linear maps in between:
    the smallest stack whose look-ahead is LA = R + R // 2 * 2, LAe = LA rounded up to 2"""

    def __init__(self, H, d, L, R, K, seed=0):
        self.H, self.d, self.L, self.R, self.K = H, d, L, R, K
        D = H * d
        g = lambda shape, i, a: RW.gauss(shape, 500 + seed + i) * a
        self.P1, self.P2 = [g((D, D), i, 0.4) for i in range(3)], [g((D, D), 3 + i, 0.4) for i in range(3)]
        self.Pu, self.w, self.bias = g((D, 2 * D), 6, 0.4), g((K, D), 7, 0.4), g((D,), 8, 0.3)
        self.ss = torch.stack([RW.coef(D, 2, positive=True), RW.coef(D, 3) * 0.5])
        self.E1, self.E2 = g((L + R + 1, H, d), 9, 1.0), g((L // 2 + R // 2 + 1, H, d), 10, 1.0)
        self.scale = 1.0 / d ** 0.5
        self.la, self.lae, self.S = lookahead([2, 1], R)

    def _qkv(self, x, P):
        return [(x @ p).view(x.shape[:-1] + (self.H, self.d)) for p in P]

    def offline(self, x):
        """x [T][D] -> [ceil(T / 2)][D]"""
        T = x.shape[0]
        a, _ = attn_offline(*self._qkv(x, self.P1), self.E1, self.scale, band(T, self.L, self.R, 1), self.R)
        y, _ = SR.conv_offline((x + a.reshape(T, -1)) @ self.Pu, self.w, self.bias, self.ss, 2)
        o, _ = attn_offline(*self._qkv(y, self.P2), self.E2, self.scale, band(y.shape[0], self.L, self.R, 2), self.R // 2)
        return y + o.reshape(y.shape[0], -1)

    def session(self, B, Tc, extra=0):
        """-> step(X [B][W][D], nvalid, ncommit, reset) of walk(); `extra`: room in the rings for a commit beyond the rule"""
        a1 = AttnStreamLA(B, self.H, self.d, self.L, self.R, Tc + extra)
        cv = SR.ConvStream(B, self.H * self.d, self.K)
        a2 = AttnStreamLA(B, self.H, self.d, self.L // 2, self.R // 2, (Tc + extra) // 2)

        def step(X, nvalid, ncommit, reset):
            W = X.shape[1]
            a, _ = a1.push(*self._qkv(X, self.P1), self.E1, self.scale, nvalid, ncommit, reset)
            y, _ = cv.push((X + a.reshape(B, W, -1)) @ self.Pu, self.w, self.bias, self.ss, 2, ncommit, reset)
            o, _ = a2.push(*self._qkv(y, self.P2), self.E2, self.scale, [-(-n // 2) for n in nvalid], [c // 2 for c in ncommit], reset)
            return y + o.reshape(B, W // 2, -1)
        return step
