"""Host-side pieces of the streamed audio front-end tests (tests/test_stream_front_ref.py, tests/test_gpu_stream_front_kernels.py, tests/test_gpu_stream_front.py):
an fp64 reference of the front-end in CHUNKED form -- a sample carry per slot, a counter and an `ended` flag, nothing else -- written from the arithmetic alone
(no kernel, no ops call), beside the offline chain on a whole utterance (oracle.mel_frontend + oracle.audio_stem), the push schedule, and seeded parameters.

Arithmetic (16 kHz, n_fft 512, window 400, hop 160, stem stride 2; n = samples a slot has received since its restart):
  mel frame f reads samples [160 f - 200, 160 f + 200); left reflection x[-s] = x[s] (frames 0 and 1), right reflection x[s] = x[2 (Ta - 1) - s] once the end is known;
  stem frame t reads mel frames 2t - 1, 2t, 2t + 1; mel frame -1 and mel frames >= Ta // 160 + 1 are the convolution's zero padding (zero in the log-mel domain);
  E(n) = 0 if n < 360 else (n - 40) // 320 stem frames are computable before the end, Ta // 320 + 1 at the end;
  after a push a slot keeps samples [max(0, 320 E(n) - 360), n).
Layouts: stem weight w [C][1][3][3], BatchNorm of C channels, Linear [D][C * n_mels / 2]; stem rows [frames][C * n_mels / 2] (channel-major, as the offline reshape).
"""
import math

import torch
import torch.nn.functional as F

from oracle import avec_oracle as O

D64 = torch.float64
N_FFT, WIN, HOP = 512, 400, 160
GARBAGE = float("nan")          # what a carry holds before the first push / behind its valid part: never read

LENGTHS = [257, 319, 320, 359, 360, 361, 640, 679, 680, 681, 799, 800, 960, 2599, 2600]
SPLITS = [0, 1, 40, 159, 160, 161, 320, 360]


def ready(n):
    return 0 if n < 360 else (n - 40) // 320


def first_kept(E):
    return max(0, 320 * E - 360)


def params(n_mels, C, D, seed):
    """seeded fp64 parameters under the oracle's state-dict keys (prefix "m"): stem conv, BatchNorm2d with non-identity running statistics, Linear"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=D64)
    Fo = n_mels // 2
    p = "m.subsampling_module.layers.0."
    return {p + "0.weight": 0.3 * r(C, 1, 3, 3), p + "0.bias": 0.1 * r(C), p + "1.weight": 1.0 + 0.2 * r(C), p + "1.bias": 0.2 * r(C),
            p + "1.running_mean": 0.3 * r(C), p + "1.running_var": 0.5 + torch.rand(C, generator=g, dtype=D64), p + "1.num_batches_tracked": torch.tensor(3),
            "m.linear.weight": r(D, C * Fo) / math.sqrt(C * Fo), "m.linear.bias": 0.1 * r(D)}


def offline(sd, x, n_mels):
    """the offline chain on one whole utterance x [Ta] fp64 -> (mel [n_mels][Ta // 160 + 1], stem rows [Ta // 320 + 1][C Fo], features [Ta // 320 + 1][D])"""
    mel = O.mel_frontend(x[None], None, N_FFT, WIN, HOP, n_mels)
    z = F.conv2d(F.pad(mel[:, None], (1, 1, 1, 1)), sd["m.subsampling_module.layers.0.0.weight"], sd["m.subsampling_module.layers.0.0.bias"], stride=2)
    z = O.swish(O.batch_norm(sd, "m.subsampling_module.layers.0.1", z, False))
    rows = z.reshape(1, -1, z.shape[-1]).transpose(1, 2)[0]
    feat, flen = O.audio_stem(sd, "m", mel, torch.tensor([mel.shape[-1]]), False, {})
    assert int(flen[0]) == rows.shape[0] == x.shape[0] // 320 + 1
    return mel[0], rows, feat[0]


class FrontStream:
    """the chunked front-end: per slot a carry (the kept samples, exactly), n and ended"""

    def __init__(self, B, sd, n_mels):
        self.B, self.sd, self.n_mels = B, sd, n_mels
        self.carry = [torch.full((7,), GARBAGE, dtype=D64) for _ in range(B)]
        self.n, self.ended = [0] * B, [False] * B
        p = "m.subsampling_module.layers.0."
        self.w, self.bias = sd[p + "0.weight"], sd[p + "0.bias"]
        self.scale = sd[p + "1.weight"] / torch.sqrt(sd[p + "1.running_var"] + 1e-5)
        self.shift = sd[p + "1.bias"] - sd[p + "1.running_mean"] * self.scale
        self.fb = O.mel_filterbank(N_FFT // 2 + 1, 0.0, 8000.0, n_mels, 16000).to(D64)
        self.window = torch.zeros(N_FFT, dtype=D64)
        self.window[(N_FFT - WIN) // 2:(N_FFT - WIN) // 2 + WIN] = torch.hann_window(WIN, periodic=True, dtype=D64)

    def _mel_column(self, samples):
        fr = torch.zeros(N_FFT, dtype=D64)
        fr[(N_FFT - WIN) // 2:(N_FFT - WIN) // 2 + WIN] = samples
        spec = torch.fft.rfft(fr * self.window)
        return ((spec.real ** 2 + spec.imag ** 2) @ self.fb + 1e-9).log()

    def push(self, chunks, last=(), reset=()):
        """chunks[b]: the samples slot b takes in this push (1-D fp64, possibly empty); last / reset: sets of slots.  -> per slot (mel block [n_mels][2 k + 1] of mel
        frames 2 E0 - 1 .. 2 E1 - 1 with zero columns where the stem pads, validity of each column, stem rows [k][C Fo], features [k][D]), k = E1 - E0"""
        out = []
        for b in range(self.B):
            if b in reset:
                self.n[b], self.ended[b], self.carry[b] = 0, False, torch.full((11,), GARBAGE, dtype=D64)
            if self.ended[b]:
                assert chunks[b].numel() == 0, "an ended slot takes no samples"
                out.append((torch.zeros(self.n_mels, 1, dtype=D64), [False], torch.zeros(0, self.w.shape[0] * (self.n_mels // 2), dtype=D64), None))
                continue
            n0, ns = self.n[b], chunks[b].numel()
            E0, n1, fin = ready(n0), n0 + ns, b in last
            c0 = first_kept(E0)
            V = torch.cat([self.carry[b][:n0 - c0], chunks[b]])           # global sample s sits at V[s - c0]
            assert V.numel() == n1 - c0
            E1 = n1 // 320 + 1 if fin else ready(n1)
            assert not fin or n1 > N_FFT // 2

            def samples(m):
                s = torch.arange(WIN) + HOP * m - WIN // 2
                assert fin or int(s[-1]) < n1
                s = torch.where(s < 0, -s, torch.where(s >= n1, 2 * (n1 - 1) - s, s))
                assert c0 <= int(s.min()) and int(s.max()) < n1, (m, c0, n1)
                return V[s - c0]
            k = E1 - E0
            cols, valid = [], []
            for m in range(2 * E0 - 1, 2 * E1):
                ok = k > 0 and m >= 0 and (not fin or m < n1 // HOP + 1)
                valid.append(ok)
                cols.append(self._mel_column(samples(m)) if ok else torch.zeros(self.n_mels, dtype=D64))
            mel = torch.stack(cols, dim=1)
            if k > 0:
                z = F.conv2d(F.pad(mel[None, None], (0, 0, 1, 1)), self.w, self.bias, stride=2)[0]            # [C][Fo][k]: time is padded by the block itself
                z = z * self.scale[:, None, None] + self.shift[:, None, None]
                rows = (z * torch.sigmoid(z)).reshape(-1, k).t()
                feat = rows @ self.sd["m.linear.weight"].t() + self.sd["m.linear.bias"]
            else:
                rows, feat = torch.zeros(0, self.w.shape[0] * (self.n_mels // 2), dtype=D64), None
            out.append((mel, valid, rows, feat))
            self.n[b] = n1
            if fin:
                self.ended[b] = True
            else:
                c1 = first_kept(ready(n1))
                self.carry[b] = torch.cat([V[c1 - c0:], torch.full((3,), GARBAGE, dtype=D64)])
                assert n1 - c1 < 720
        return out


def split_sizes(Ta, s):
    """the sample counts of the pushes that deliver an utterance of Ta samples in pieces of s (s = 0: empty pushes between pieces of 200, and an empty last push)"""
    if s == 0:
        sizes = []
        while sum(sizes) < Ta:
            sizes += [0, min(200, Ta - sum(sizes))]
        return sizes + [0]
    return [min(s, Ta - i) for i in range(0, Ta, s)]


def schedule_sizes(Ta, Tc):
    """the session's schedule: 320 Tc + 40 samples first, 320 Tc in every later push, the rest in the last"""
    sizes, left = [], Ta
    while left > 0:
        c = min(left, 320 * Tc + (40 if not sizes else 0))
        sizes.append(c)
        left -= c
    return sizes


def run_utterance(fs, b, x, sizes, restart=True):
    """push utterance x through slot b of `fs` in pieces of `sizes` (the other slots idle) -> (stem rows, features) concatenated, and the frames each push gave"""
    rows, feats, per_push, at = [], [], [], 0
    for i, c in enumerate(sizes):
        chunks = [torch.zeros(0, dtype=D64) for _ in range(fs.B)]
        chunks[b] = x[at:at + c]
        at += c
        out = fs.push(chunks, last={b} if i == len(sizes) - 1 else (), reset={b} if (i == 0 and restart) else ())[b]
        per_push.append(out[2].shape[0])
        if out[2].shape[0]:
            rows.append(out[2]), feats.append(out[3])
    assert at == x.numel()
    return torch.cat(rows), torch.cat(feats), per_push
